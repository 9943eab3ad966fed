"""The GroupNorm statistics hand-off between launches (csrc/norm.hip, the row epilogue of csrc/gemm.hip): no stale or unwritten sum
may pass.

The wrappers take every statistics buffer from ``torch.empty`` and the other tests launch the same input twice in a row, so the caching
allocator hands back the block that already holds the right sums of that very input: a skipped store, an entry read before it was
written or a consumer one launch behind compares equal (tests/test_stats_handoff_cpu.py shows each on an emulation).  Here
  (a) two operand sets of different mean and scale alternate (handoff.SCHEDULE) on ONE test-owned buffer without a host
      synchronisation, from a NaN-filled, a stale (the other set's correct statistics) and a zeroed buffer; every output must be
      bit-equal to a launch of ITS set on a fresh NaN-filled buffer, which is checked per element against float64;
  (b) after one launch on a NaN-filled buffer every entry of the documented extent is written, nothing beyond it changed (guard
      bands: test_footprint_gpu.Guarded) and every entry is within its derived bound of float64 (tests/stats_handoff.py), at shapes
      with empty K-split blocks, a ragged last sweep, two passes of the channel loop, and the smallest producers;
  (c) the product's arrangement: producer -> GroupNorm and the split paths in one captured graph, replayed with changing inputs;
  (d) the CFG duplication of a tensor that carries producer statistics.
The buffers are the test's own through the raw C ABI.  No tolerance other than the derived bounds and bit-equality.

Every case prints ``PARITY stats <case> max|err|/bound=<r>`` (pytest -s shows it)."""
import contextlib
import math
import os

import pytest
import torch

import parity as P
import stats_handoff as S
from test_footprint_gpu import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
EPS = 1e-5
FILLS = ("nan", "other", "zero")


@pytest.fixture
def force_plan():
    """gmd_gemm_plan_override is refused unless the process has GMD_TUNING=1 (include/gmd_hip.h)."""
    from gm_diffusion._native import lib

    prev = os.environ.get("GMD_TUNING")
    os.environ["GMD_TUNING"] = "1"

    def force(bm, bn, pf, ks):
        assert lib().gmd_gemm_plan_override(bm, bn, pf, ks) == 0

    yield force
    torch.cuda.synchronize()
    lib().gmd_gemm_plan_override(0, 0, 0, 0)
    if prev is None:
        os.environ.pop("GMD_TUNING", None)
    else:
        os.environ["GMD_TUNING"] = prev


def _report(case, r):
    print(f"PARITY stats {case} max|err|/bound={r:.3f}")
    return r


def _lib():
    from gm_diffusion._native import lib

    return lib()


def _ops():
    from gm_diffusion import hip_ops

    return hip_ops


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    assert rc == 0, f"{what}: {_lib().gmd_last_error()}"


class Owned:
    """A statistics buffer of the test's own: ``extent`` floats (the documented extent) and SPARE more inside the guard bands of
    test_footprint_gpu.Guarded, NaN-filled (handoff.nan_words).  Everything here is stream-ordered: no host synchronisation."""
    SPARE = 1024

    def __init__(self, extent):
        self.extent = extent
        self.gd = Guarded(extent + self.SPARE, F32)
        self.t = self.gd.t
        self.fill("nan")

    def fill(self, kind):
        if kind == "nan":
            S.nan_fill(self.t)
        elif kind == "zero":
            self.t[:self.extent].zero_()
        self.gd.before = self.gd.buf.clone()  # what the launches may change from here on: the extent, nothing else

    def view(self, *shape):
        return self.t[:self.extent].view(*shape)

    def assert_footprint(self, what, all_written):
        """After a synchronisation: guard bands and the spare words unchanged; ``all_written``: the buffer was NaN-filled before the
        launch and no word of the extent may still hold its fill."""
        window = torch.zeros(self.t.numel(), dtype=torch.bool, device=DEV)
        window[:self.extent] = True
        self.gd.assert_untouched_outside(window, what)
        if all_written:
            idx = S.unwritten(self.t, self.extent)
            assert idx.numel() == 0, f"{what}: {idx.numel()} of {self.extent} words were not written; first at word {int(idx[0])} = entry {int(idx[0]) // 2}"


def _gn_sets(B, HW, C, dtype, seed):
    """Two operand sets of different mean and scale (mean / std 0.25 and 4.3): a stale statistic is far outside any bound."""
    g = torch.Generator().manual_seed(seed)
    sets = []
    for scale, shift in ((2.0, 0.5), (0.7, -3.0)):
        sets.append(dict(x=(torch.randn(B, HW, C, generator=g) * scale + shift).to(dtype).to(DEV), gamma=torch.randn(C, generator=g).to(DEV),
                         beta=torch.randn(C, generator=g).to(DEV)))
    return sets


def _split_launch(s, dims, code, ws, silu=True):
    B, HW, C, G = dims
    y = torch.empty_like(s["x"])
    _ok(_lib().gmd_groupnorm_split(_p(s["x"]), _p(y), code, B, HW, C, G, EPS, _p(s["gamma"]), _p(s["beta"]), _p(ws.t), int(silu), _stream()), "gmd_groupnorm_split")
    return y


def _stats_apply_launch(s, dims, code, ws, ss, silu=True):
    B, HW, C, G = dims
    y = torch.empty_like(s["x"])
    _ok(_lib().gmd_groupnorm_stats(_p(s["x"]), code, B, HW, C, G, EPS, _p(s["gamma"]), _p(s["beta"]), _p(ws.t), _p(ss.t), _stream()), "gmd_groupnorm_stats")
    _ok(_lib().gmd_groupnorm_apply(_p(s["x"]), _p(y), code, B, HW, C, _p(ss.t), int(silu), _stream()), "gmd_groupnorm_apply")
    return y


def _bits(t):
    """Outputs are compared as bits (a pre-split float32 tensor holds float16 pairs: any pattern, NaNs included)."""
    return t.view(torch.int32) if t.dtype == F32 else t.view(torch.int16)


def _geometry(dims, dtype, want_empty):
    """(nsplit, height) of the library's split of HW rows; asserts the number of empty blocks the case is about."""
    B, HW, C, G = dims
    nsplit = _lib().gmd_groupnorm_nsplit(HW)
    per, ranges = S.block_rows(HW, nsplit)
    empty = S.empty_blocks(HW, nsplit)
    assert empty == want_empty, (f"gmd_groupnorm_nsplit({HW}) = {nsplit} (per = {per}) gives {empty} empty blocks, this case is about {want_empty}: "
                                 "the split rule moved, re-pick HW")
    assert S.partial_geometry(C, dtype)[4] <= S.LDS_LIMIT
    return nsplit, S.partial_height(HW, nsplit, C, dtype)


def _check_norm(y, s, G, dtype, height, what, silu=True, presplit=False):
    ref, bound = P.groupnorm_ref_bound(s["x"], G, s["gamma"], s["beta"], EPS, F32 if presplit else dtype, height, silu)
    if presplit:  # read hi + lo back: the split's residual on top (2^-22 |x| + 2^-25, parity.split_product_bound's r_x)
        y = P.unsplit(y)
        bound = bound + 2.0 ** -22 * (ref.abs() + bound) + 2.0 ** -25
    return _report(what, P.assert_elementwise(y, ref, bound, what, (64, 8)))


def _sequences(launch, prime, sets, refs, owned, what):
    """The alternating schedule from the three starting states of the buffers in ``owned``."""
    for fill in FILLS:
        for o in owned:
            o.fill("nan" if fill == "other" else fill)
        if fill == "other":  # the other set's CORRECT statistics, left by a launch of it
            prime(sets[1 - S.SCHEDULE[0]])
        outs = [launch(sets[i]) for i in S.SCHEDULE]
        torch.cuda.synchronize()
        S.assert_sequence([tuple(_bits(t) for t in o) for o in outs], [tuple(_bits(t) for t in r) for r in refs], f"{what} fill={fill}")
        for o in owned:
            o.assert_footprint(f"{what} fill={fill}", fill != "zero")
        print(f"HANDOFF stats {what} fill={fill} launches={len(S.SCHEDULE)} ok")


# ---------------------------------------------------------------------------------------------------------------------------
# (a) alternation on one buffer: the statistics passes of csrc/norm.hip
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "bf16", "f16", "f32sa"])
def test_groupnorm_split_alternating_operand_sets_on_one_workspace(kind):
    """gmd_groupnorm_split (partial sums -> an apply that folds them itself) at the shape whose last K-split block is empty."""
    ops = _ops()
    dims = B, HW, C, G = 2, 2079, 64, 8
    dtype = {"f32": F32, "bf16": BF16, "f16": F16, "f32sa": F32}[kind]
    code = ops.GMD_F32SA if kind == "f32sa" else ops.dtype_code(dtype)
    nsplit, height = _geometry(dims, dtype, 1)
    sets = _gn_sets(B, HW, C, dtype, 11)
    extent = B * nsplit * G * 2
    refs = []
    for i, s in enumerate(sets):
        fresh = Owned(extent)
        refs.append((_split_launch(s, dims, code, fresh),))
        torch.cuda.synchronize()
        fresh.assert_footprint(f"split {kind} reference {i}", True)
        _check_norm(refs[-1][0], s, G, dtype, height, f"split {kind} {B}x{HW}x{C} set{i}", presplit=kind == "f32sa")
    ws = Owned(extent)
    _sequences(lambda s: (_split_launch(s, dims, code, ws),), lambda s: _split_launch(s, dims, code, ws), sets, refs, [ws], f"split {kind} {B}x{HW}x{C}")


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_groupnorm_stats_apply_alternating_on_one_workspace_and_scale_shift(dtype):
    """gmd_groupnorm_stats + gmd_groupnorm_apply: BOTH hand-offs (partial sums -> finalize, scale_shift -> apply) on buffers that are
    reused launch after launch."""
    ops = _ops()
    dims = B, HW, C, G = 2, 2079, 64, 8
    code = ops.dtype_code(dtype)
    nsplit, height = _geometry(dims, dtype, 1)
    sets = _gn_sets(B, HW, C, dtype, 12)
    refs = []
    for i, s in enumerate(sets):
        fw, fs = Owned(B * nsplit * G * 2), Owned(B * C * 2)
        refs.append((_stats_apply_launch(s, dims, code, fw, fs), fs.view(B, C, 2).clone()))
        torch.cuda.synchronize()
        fw.assert_footprint(f"stats+apply {dtype} reference {i} workspace", True)
        fs.assert_footprint(f"stats+apply {dtype} reference {i} scale_shift", True)
        _check_norm(refs[-1][0], s, G, dtype, height, f"stats+apply {dtype} {B}x{HW}x{C} set{i}")
    ws, ss = Owned(B * nsplit * G * 2), Owned(B * C * 2)
    _sequences(lambda s: (_stats_apply_launch(s, dims, code, ws, ss), ss.view(B, C, 2).clone()), lambda s: _stats_apply_launch(s, dims, code, ws, ss),
               sets, refs, [ws, ss], f"stats+apply {dtype} {B}x{HW}x{C}")


# ---------------------------------------------------------------------------------------------------------------------------
# (b) every entry written, every entry right: the statistics passes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("B,HW,C,G,empty,what", [(2, 2079, 64, 8, 1, "last block starts at HW"), (1, 16385, 64, 8, 3, "three blocks start beyond HW"),
                                                 (3, 1000, 64, 8, 0, "PY > 1, ragged last sweep"), (1, 300, 2560, 32, 0, "C / V > 256")])
def test_every_partial_sum_and_scale_shift_is_written_and_right(B, HW, C, G, empty, what, dtype):
    ops = _ops()
    dims = (B, HW, C, G)
    code = ops.dtype_code(dtype)
    nsplit, height = _geometry(dims, dtype, empty)
    CV, CVB, PY, passes, lds = S.partial_geometry(C, dtype)
    if C == 2560:  # two passes of the channel loop (three at float32, whose [1][2560] x 2 floats of LDS stay far below the 64 KiB limit)
        assert passes == (3 if dtype == F32 else 2) and PY == 1 and lds == 20480
    elif HW == 1000:
        assert PY > 1 and -(-HW // nsplit) % PY != 0
    s = _gn_sets(B, HW, C, dtype, HW + C)[1]  # |mean| / std = 4.3: the E[x^2] - mean^2 form at work
    ws, ss, ws2 = Owned(B * nsplit * G * 2), Owned(B * C * 2), Owned(B * nsplit * G * 2)
    y = _stats_apply_launch(s, dims, code, ws, ss)
    y2 = _split_launch(s, dims, code, ws2)
    torch.cuda.synchronize()
    case = f"{B}x{HW}x{C} {dtype}"
    for o, name in ((ws, "workspace"), (ss, "scale_shift"), (ws2, "workspace of gmd_groupnorm_split")):
        o.assert_footprint(f"{case} {name}", True)
    ref, bound = S.partial_ref_bound(s["x"], G, nsplit)
    got = ws.view(B, nsplit, G, 2)
    r1 = S.assert_entries(got, ref, bound, f"{case} partial sums ({what})")
    if empty:
        assert bool((bound[:, -empty:] == 0).all()) and not bool(got[:, -empty:].view(torch.int32).any()), f"{case}: an empty block must store exactly {{+0, +0}}"
    assert torch.equal(ws2.view(-1).view(torch.int32), ws.view(-1).view(torch.int32)), f"{case}: the two entry points' partial launches differ"
    ref, bound = S.scale_shift_ref_bound(s["x"], G, s["gamma"], s["beta"], EPS, height)
    r2 = S.assert_entries(ss.view(B, C, 2), ref, bound, f"{case} scale_shift")
    _report(f"{case} h={height} partial", r1)
    _report(f"{case} h={height} scale_shift", r2)
    _check_norm(y, s, G, dtype, height, f"{case} stats+apply output")
    _check_norm(y2, s, G, dtype, height, f"{case} split output")


# ---------------------------------------------------------------------------------------------------------------------------
# producers: gmd_gemm_nt / gmd_conv3x3 with test-owned statistics
# ---------------------------------------------------------------------------------------------------------------------------
def _gemm(s, st, bucket, kind):
    """y = a w^T + bias (+ residual | + rowbias with rows_per_group = 96: the seam falls inside the second 64-row block)."""
    ops = _ops()
    a, w = s["a"], s["w"]
    (M, K), N = a.shape, w.shape[0]
    code = ops.dtype_code(a.dtype)
    out = torch.empty(M, N, dtype=a.dtype, device=DEV)
    rb, rpg, res = (s["rb"], 96, None) if kind == "rowbias" else (None, 0, s["res"])
    _ok(_lib().gmd_gemm_nt(_p(a), _p(w), _p(out), code, code, M, N, K, K, K, N, 1, 0, 0, 0, _p(s["bias"]), _p(rb), rpg, N if rb is not None else 0, _p(res), N, 0,
                           1.0, 0, _p(st.t), bucket, _p(ops._workspace(a.device)), ops.WORKSPACE_BYTES, _stream()), "gmd_gemm_nt")
    return out


def _conv(s, st, bucket, B, H, W, up):
    ops = _ops()
    x, w = s["x"], s["w"]
    cin, cout = x.shape[-1], w.shape[0]
    code = ops.dtype_code(x.dtype)
    ho, wo = (2 * H, 2 * W) if up else (H, W)
    out = torch.empty(B, ho * wo, cout, dtype=x.dtype, device=DEV)
    _ok(_lib().gmd_conv3x3(_p(x), _p(w), _p(out), code, code, B, H, W, cin, cout, 1, int(up), 0, _p(s["bias"]), None, 0, None, 1.0, _p(st.t),
                           bucket, _p(ops._workspace(x.device)), ops.WORKSPACE_BYTES, _stream()), "gmd_conv3x3")
    return out


def _gemm_sets(M, N, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    sets = []
    for scale, shift in ((1.0, 0.5), (0.4, -2.0)):
        sets.append(dict(a=(torch.randn(M, K, generator=g) * scale).to(dtype).to(DEV), w=(torch.randn(N, K, generator=g) / math.sqrt(K)).to(dtype).to(DEV),
                         bias=(torch.randn(N, generator=g) + shift).to(DEV), res=(torch.randn(M, N, generator=g) * scale).to(dtype).to(DEV),
                         rb=torch.randn(-(-M // 96), N, generator=g).to(DEV), gamma=torch.randn(N, generator=g).to(DEV), beta=torch.randn(N, generator=g).to(DEV)))
    return sets


def _conv_sets(B, H, W, cin, cout, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    sets = []
    for scale, shift in ((1.0, 0.5), (0.4, -2.0)):
        sets.append(dict(x=(torch.randn(B, H * W, cin, generator=g) * scale).to(dtype).to(DEV), w=(torch.randn(cout, 9 * cin, generator=g) / math.sqrt(9 * cin)).to(dtype).to(DEV),
                         bias=(torch.randn(cout, generator=g) + shift).to(DEV), gamma=torch.randn(cout, generator=g).to(DEV), beta=torch.randn(cout, generator=g).to(DEV)))
    return sets


def _assert_colstats_plan(dtype, M, N, K, bucket, want):
    """The launch can emit statistics and takes the kernel the case names: ``want`` = (tile rows, tile columns, kernel code) and the
    allowed numbers of K slices."""
    ops = _ops()
    assert _lib().gmd_gemm_colstats_plan(ops.dtype_code(dtype), M, N, K, 1, ops.WORKSPACE_BYTES, bucket) == 1, f"{M}x{N}x{K}: no statistics from this plan"
    info = ops.gemm_plan_info(dtype, M, N, K)
    assert info[:3] == want[0] and info[3] in want[1], f"{M}x{N}x{K}: plan {info}, this case is about {want}"
    return info


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("N", [160, 320, 128, 256])
@pytest.mark.parametrize("M", [128, 256])
def test_every_bucket_entry_of_the_smallest_producers_is_written_and_right(M, N, dtype, force_plan):
    """One and two tiles of 160 and of 128 columns (buckets of 10 and of 8: half a tile must hold whole buckets), one 128-row ring
    tile (forced: the heuristic gives so small a launch 64 x 64 tiles) and one 256-row ping-pong tile (what the co-running plan family
    picks), three epilogues: bias + residual, bias + row bias with the seam inside a 64-row block, the upsampling convolution."""
    ops = _ops()
    bn, bucket, K = (160, 10, 320) if N % 160 == 0 else (128, 8, 320)
    extent = (M // 64) * (N // bucket) * 2
    if M == 128:
        force_plan(128, bn, 9, 1)
        want = ((128, bn, 0), (1,))
    else:
        want = ((256, bn, 283), (1,))
    with ops.plan_family(1) if M != 128 else contextlib.nullcontext():
        _assert_colstats_plan(dtype, M, N, K, bucket, want)
        s = _gemm_sets(M, N, K, dtype, M + N)[1]
        Bc, Hc, Wc, cin = 1, (4 if M == 128 else 8), 8, 64  # upsampled to 8 x 16 / 16 x 16 pixels = M rows
        _assert_colstats_plan(dtype, M, N, 9 * cin, bucket, want)
        sc = _conv_sets(Bc, Hc, Wc, cin, N, dtype, M + N + 1)[1]
        runs = []
        for kind in ("residual", "rowbias", "conv_up"):
            st = Owned(extent)
            y = _conv(sc, st, bucket, Bc, Hc, Wc, True).view(M, N) if kind == "conv_up" else _gemm(s, st, bucket, kind)
            runs.append((kind, st, y))
        torch.cuda.synchronize()
    for kind, st, y in runs:
        case = f"producer {kind} {M}x{N} {dtype} tile {want[0][0]}x{bn}"
        assert bool(torch.isfinite(y.float()).all())
        st.assert_footprint(case, True)
        ref, bound = S.bucket_ref_bound(y, bucket)
        _report(case, S.assert_entries(st.view(M // 64, N // bucket, 2), ref, bound, case))


# ---------------------------------------------------------------------------------------------------------------------------
# (a) alternation on one buffer: producer statistics -> gmd_groupnorm_colstats
# ---------------------------------------------------------------------------------------------------------------------------
def _colstats_norm(y, B, HW, C, G, s, sa, Ca, sb, bucket=10, silu=True):
    ops = _ops()
    out = torch.empty_like(y)
    _ok(_lib().gmd_groupnorm_colstats(_p(y), _p(out), ops.dtype_code(y.dtype), B, HW, C, G, EPS, _p(s["gamma"]), _p(s["beta"]), _p(sa.t), Ca,
                                      None if sb is None else _p(sb.t), bucket, int(silu), _stream()), "gmd_groupnorm_colstats")
    return out


def _check_colstats_reference(y, out, st_list, s, B, HW, G, dtype, what):
    """A reference launch (fresh NaN-filled statistics): every entry written and within its bound of the STORED producer output, the
    normalised tensor within groupnorm_ref_bound of it (height: producer_height)."""
    col = 0
    for st, c in st_list:
        st.assert_footprint(what, True)
        ref, bound = S.bucket_ref_bound(y.reshape(B * HW, -1)[:, col:col + c].contiguous(), 10)
        _report(what + " buckets", S.assert_entries(st.view(B * HW // 64, c // 10, 2), ref, bound, what + " buckets"))
        col += c
    ref, bound = P.groupnorm_ref_bound(y, G, s["gamma"], s["beta"], EPS, dtype, S.producer_height(10), True)
    _report(what, P.assert_elementwise(out, ref, bound, what, (64, 10)))


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("producer", ["gemm", "conv", "gemm_two_k_slices"])
def test_colstats_alternating_operand_sets_on_one_statistics_buffer(producer, dtype):
    """producer -> gmd_groupnorm_colstats, the producer writing into the SAME statistics buffer every time, under the co-running plan
    family: a 256-row ping-pong tile unsplit (gemm K = 320, conv K = 576) and as two K slices whose last one reduces inside the kernel
    and leaves through the row epilogue, statistics included (K = 1280)."""
    ops = _ops()
    B, HW, C, G = 2, 128, 320, 32
    M = B * HW
    with ops.plan_family(1):
        if producer == "conv":
            cin = 64
            _assert_colstats_plan(dtype, M, C, 9 * cin, 10, ((256, 160, 283), (1,)))
            sets = _conv_sets(B, 8, 16, cin, C, dtype, 21)
            produce = lambda s, st: _conv(s, st, 10, B, 8, 16, False)  # noqa: E731
        else:
            K = 1280 if producer == "gemm_two_k_slices" else 320
            info = _assert_colstats_plan(dtype, M, C, K, 10, ((256, 160, 283), (2, 3, 4) if K == 1280 else (1,)))
            assert K == 320 or _lib().gmd_splitk_fixup_max(-1) >= info[3], "the in-kernel reduction is switched off in this process"
            sets = _gemm_sets(M, C, K, dtype, 22)
            produce = lambda s, st: _gemm(s, st, 10, "residual").view(B, HW, C)  # noqa: E731

        def launch(s, st):
            y = produce(s, st)
            return y, _colstats_norm(y, B, HW, C, G, s, st, C, None)

        what = f"colstats {producer} {M}x{C} {dtype}"
        refs = []
        for i, s in enumerate(sets):
            fresh = Owned((M // 64) * (C // 10) * 2)
            refs.append(launch(s, fresh))
            torch.cuda.synchronize()
            _check_colstats_reference(refs[-1][0], refs[-1][1], [(fresh, C)], s, B, HW, G, dtype, f"{what} set{i}")
        st = Owned((M // 64) * (C // 10) * 2)
        _sequences(lambda s: launch(s, st), lambda s: launch(s, st), sets, refs, [st], what)


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_colstats_of_two_producers_alternating(dtype):
    """The skip concatenation: channels [0, 320) from one producer, [320, 480) from another, their statistics side by side (Ca < C);
    480 / 16 = 30 channels per group, so group 10 (channels 300 .. 329) straddles the seam."""
    ops = _ops()
    B, HW, Ca, Cb, G, K = 2, 128, 320, 160, 16, 320
    M, C = B * HW, Ca + Cb
    with ops.plan_family(1):
        for c in (Ca, Cb):
            _assert_colstats_plan(dtype, M, c, K, 10, ((256, 160, 283), (1,)))
        sa_sets, sb_sets = _gemm_sets(M, Ca, K, dtype, 31), _gemm_sets(M, Cb, K, dtype, 32)
        g = torch.Generator().manual_seed(33)
        sets = [dict(a=sa_sets[i], b=sb_sets[i], gamma=torch.randn(C, generator=g).to(DEV), beta=torch.randn(C, generator=g).to(DEV)) for i in range(2)]

        def launch(s, sta, stb):
            ya, yb = _gemm(s["a"], sta, 10, "residual"), _gemm(s["b"], stb, 10, "rowbias")
            x = ops.concat_channels(ya.view(B, HW, Ca), yb.view(B, HW, Cb))
            return x, _colstats_norm(x, B, HW, C, G, s, sta, Ca, stb)

        what = f"colstats two producers {M}x({Ca}+{Cb}) {dtype}"
        ea, eb = (M // 64) * (Ca // 10) * 2, (M // 64) * (Cb // 10) * 2
        refs = []
        for i, s in enumerate(sets):
            fa, fb = Owned(ea), Owned(eb)
            refs.append(launch(s, fa, fb))
            torch.cuda.synchronize()
            _check_colstats_reference(refs[-1][0], refs[-1][1], [(fa, Ca), (fb, Cb)], s, B, HW, G, dtype, f"{what} set{i}")
        sta, stb = Owned(ea), Owned(eb)
        _sequences(lambda s: launch(s, sta, stb), lambda s: launch(s, sta, stb), sets, refs, [sta, stb], what)


# ---------------------------------------------------------------------------------------------------------------------------
# (c) replay with changing inputs
# ---------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_with_changing_inputs():
    """producer -> groupnorm (statistics from the producer), groupnorm (partial sums -> apply) and groupnorm_split (partial ->
    finalize -> apply) through the wrappers in ONE captured graph, one stream, as the product runs them: the statistics buffers are
    the graph's own and are reused by every replay.  Six replays, the static inputs overwritten in SCHEDULE order; every replay must be
    bit-equal to the eager result of its set."""
    ops = _ops()
    B, HW, C, G, K = 2, 128, 320, 32, 320
    dims2 = B2, HW2, C2, G2 = 2, 2079, 64, 8
    M = B * HW
    _geometry(dims2, F32, 1)
    assert HW2 * (C2 // G2) * 4 > ops.GN_FUSED_MAX_SLAB_VEC16, "the wrapper's dispatch rule moved: groupnorm no longer takes gmd_groupnorm_split here"
    gs, xs = _gemm_sets(M, C, K, BF16, 41), _gn_sets(B2, HW2, C2, F32, 42)

    def run(a, res, x, i):
        y = ops.gemm_nt(a, gs[0]["w"], bias=gs[0]["bias"], residual=res, colstats=True)
        assert getattr(y, "_colstats", None) is not None, "the producer left no statistics"
        before = ops.colstats_uses
        n1 = ops.groupnorm(ops.carry_colstats(y.view(B, HW, C), y), B, G, gs[0]["gamma"], gs[0]["beta"], EPS, silu=True)
        assert ops.colstats_uses == before + 1
        n2 = ops.groupnorm(x, B2, G2, xs[0]["gamma"], xs[0]["beta"], EPS, silu=True)
        n3 = ops.groupnorm_split(x, B2, G2, xs[0]["gamma"], xs[0]["beta"], EPS, silu=False)
        assert ops.colstats_uses == before + 1
        return y, n1, n2, n3

    with ops.plan_family(1):
        _assert_colstats_plan(BF16, M, C, K, 10, ((256, 160, 283), (1,)))
        refs = []
        for i in range(2):
            refs.append(run(gs[i]["a"], gs[i]["res"], xs[i]["x"], i))
            torch.cuda.synchronize()
        static = [gs[0]["a"].clone(), gs[0]["res"].clone(), xs[0]["x"].clone()]
        ws = ops.new_workspace(torch.device(DEV))
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with ops.workspace_scope(ws), torch.cuda.graph(gr):
            g_outs = run(*static, 0)
        clones = []
        for i in S.SCHEDULE:
            for t, src in zip(static, (gs[i]["a"], gs[i]["res"], xs[i]["x"])):
                t.copy_(src)
            gr.replay()
            clones.append(tuple(t.clone() for t in g_outs))
        torch.cuda.synchronize()
    S.assert_sequence([tuple(_bits(t) for t in o) for o in clones], [tuple(_bits(t) for t in r) for r in refs], "graph replay")
    print(f"HANDOFF stats graph producer+colstats+split+stats/apply launches={len(S.SCHEDULE)} ok")


# ---------------------------------------------------------------------------------------------------------------------------
# (d) CFG duplication
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16])
def test_cfg_duplication_carries_the_statistics_to_both_halves(dtype):
    """A producer's output that goes through carry_colstats and UNet2DConditionModel._dup_batch: GroupNorm of the duplicated tensor is
    served from the duplicated statistics and both halves equal, bit for bit, GroupNorm of the unduplicated tensor from the producer's
    statistics.  Against gmd_groupnorm_split of each half (its own statistics pass over the stored tensor) bits may differ: the
    producer sums 64 rows x 10 channels in float32 (producer_height), the partial kernel a block's rows per thread (partial_height),
    and the two sets of float32 sums are folded in double in different groupings -- so that comparison uses the groupnorm_ref_bound
    bounds: both results within their bound of ONE float64 reference.  The statistics buffer is the test's own, NaN-filled before
    the producer runs."""
    from gm_diffusion.components import UNet2DConditionModel

    ops = _ops()
    B, HW, C, G, K = 2, 128, 320, 32, 320
    M = B * HW
    s = _gemm_sets(M, C, K, dtype, 51)[1]
    st = Owned((M // 64) * (C // 10) * 2)
    with ops.plan_family(1):
        _assert_colstats_plan(dtype, M, C, K, 10, ((256, 160, 283), (1,)))
        y = _gemm(s, st, 10, "residual")
    y._colstats = (st.view(M // 64, C // 10, 2), C)
    y3 = ops.carry_colstats(y.view(B, HW, C), y)
    dup = UNet2DConditionModel._dup_batch(y3)
    assert tuple(dup.shape) == (2 * B, HW, C) and tuple(dup._colstats[0].shape) == (2 * M // 64, C // 10, 2)
    before = ops.colstats_uses
    nd = ops.groupnorm(dup, 2 * B, G, s["gamma"], s["beta"], EPS, silu=True)
    n1 = ops.groupnorm(y3, B, G, s["gamma"], s["beta"], EPS, silu=True)
    assert ops.colstats_uses == before + 2
    nsplit = _lib().gmd_groupnorm_nsplit(HW)
    ws = Owned(2 * B * nsplit * G * 2)
    own = _split_launch(dict(x=dup, gamma=s["gamma"], beta=s["beta"]), (2 * B, HW, C, G), ops.dtype_code(dtype), ws)
    torch.cuda.synchronize()
    st.assert_footprint(f"cfg dup {dtype} producer statistics", True)
    ws.assert_footprint(f"cfg dup {dtype} workspace", True)
    assert torch.equal(dup[:B], y3) and torch.equal(dup[B:], y3)
    assert torch.equal(nd[:B], n1) and torch.equal(nd[B:], n1), "the two halves of the duplicated batch are not normalised like the original"
    sd = dict(x=dup, gamma=s["gamma"], beta=s["beta"])
    _check_norm(nd, sd, G, dtype, S.producer_height(10), f"cfg dup {dtype} from producer statistics")
    _check_norm(own, sd, G, dtype, S.partial_height(HW, nsplit, C, dtype), f"cfg dup {dtype} own statistics pass")
