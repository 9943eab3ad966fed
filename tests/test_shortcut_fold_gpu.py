"""conv2(h) + conv_shortcut(x) as ONE launch (gmd_conv3x3_tail: K2 more channels of a second operand behind the nine taps).

Per-element bounds from tests/parity.py against a float64 reference: gemm_bound with K = 9 Cin + K2 and abs_dot the sum of both parts.
The shapes are the smallest at which the loader of the 256-row ping-pong kernel takes each of its paths: one tile with the tail starting
at step 9; ragged M and N with a sample seam inside the tile; split-K with a slice boundary inside the taps, exactly on the tap / tail
seam and inside the tail (in-kernel fix-up and slab reduction, which must agree bit for bit); a full 256 x 160 tile for the row epilogue
and its column statistics.  Every case prints ``PARITY fold <case> max|err|/bound=<r>``."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
PP = 283  # the ping-pong kernel's plan code


@pytest.fixture
def force_plan():
    """gmd_gemm_plan_override is refused unless the process has GMD_TUNING=1 (include/gmd_hip.h)."""
    from gm_diffusion._native import lib

    prev = os.environ.get("GMD_TUNING")
    os.environ["GMD_TUNING"] = "1"
    fix = lib().gmd_splitk_fixup_max(-1)

    def force(bm, bn, pf, ks):
        assert lib().gmd_gemm_plan_override(bm, bn, pf, ks) == 0

    yield force
    lib().gmd_gemm_plan_override(0, 0, 0, 0)
    lib().gmd_conv_patch_override(0)
    lib().gmd_splitk_fixup_max(fix)
    if prev is None:
        os.environ.pop("GMD_TUNING", None)
    else:
        os.environ["GMD_TUNING"] = prev


def _conv64(x, w, B, H, W):
    ci, co = x.shape[-1], w.shape[0]
    xi = x.view(B, H, W, ci).permute(0, 3, 1, 2)
    wt = w.view(co, 3, 3, ci).permute(0, 3, 1, 2)
    return F.conv2d(xi, wt, padding=1).permute(0, 2, 3, 1).reshape(B, -1, co)


def _inputs(B, H, W, ci, k2, co, dtype, seed, ldx2=None):
    g = torch.Generator().manual_seed(seed)
    ldx2 = ldx2 or k2
    x = torch.randn(B, H * W, ci, generator=g).to(dtype).to(DEV)
    x2 = torch.randn(B, H * W, ldx2, generator=g).to(dtype).to(DEV)  # columns k2 .. ldx2 are live values the launch must not read
    w2 = (torch.randn(co, 9 * ci, generator=g) * 0.03).to(dtype).to(DEV)
    wsc = (torch.randn(co, k2, generator=g) * 0.05).to(dtype).to(DEV)
    b2, bsc = torch.randn(co, generator=g).to(DEV), torch.randn(co, generator=g).to(DEV)
    tb = torch.randn(B, co, generator=g).to(DEV)
    return x, x2, w2, wsc, b2, bsc, tb


def _reference(x, x2, w2, wsc, B, H, W, k2):
    """(float64 accumulator value, float64 sum of |products|) of both parts."""
    xs = x2.double()[..., :k2]
    ref = _conv64(x.double(), w2.double(), B, H, W) + xs @ wsc.double().T
    ad = _conv64(x.double().abs(), w2.double().abs(), B, H, W) + xs.abs() @ wsc.double().abs().T
    return ref, ad


def _check(ops, what, tile, B, H, W, ci, k2, co, dtype, seed, out_dtype=None, rowbias=True, ldx2=None, colstats=False):
    x, x2, w2, wsc, b2, bsc, tb = _inputs(B, H, W, ci, k2, co, dtype, seed, ldx2)
    w, b = ops.pack_shortcut(w2, b2, wsc, bsc)
    ref_acc, abs_dot = _reference(x, x2, w2, wsc, B, H, W, k2)
    ex = [b.double().expand_as(ref_acc)] + ([tb.double()[:, None, :].expand_as(ref_acc)] if rowbias else [])
    y, _, _ = ops.conv3x3_tail(x, x2, w, B, H, W, bias=b, rowbias=tb if rowbias else None, out_dtype=out_dtype, ldx2=ldx2, k2=k2,
                               colstats=colstats)
    M = B * H * W
    ref = ref_acc + sum(ex)
    r = P.assert_elementwise(y.reshape(M, co), ref.reshape(M, co),
                             P.gemm_bound(ref_acc, abs_dot, 9 * ci + k2, out_dtype or dtype, 1.0, ex).reshape(M, co), what, tile)
    print(f"PARITY fold {what} max|err|/bound={r:.3f}")
    return y


def _check_colstats(ops, y, what):
    """{sum, sum of squares} of the STORED output per 64-row block and 10-column bucket against float64 sums of that output.  A float32
    sum of n values along any tree is within (n - 1) 2^-24 sum |x| of the exact one; the squares (exact in float32 for 16-bit values)
    likewise: n 2^-24 sum x^2.  n = 64 rows x 10 columns."""
    assert getattr(y, "_colstats", None) is not None, f"{what}: the launch did not emit column statistics"
    st, n = y._colstats
    M, co = y.shape[0] * y.shape[1], y.shape[2]
    assert n == co and st.shape == (M // 64, co // ops.COLSTATS_BUCKET, 2)
    y64 = y.double().reshape(M // 64, 64, co // ops.COLSTATS_BUCKET, ops.COLSTATS_BUCKET)
    s, q = y64.sum((1, 3)), (y64 * y64).sum((1, 3))
    nv = 64 * ops.COLSTATS_BUCKET
    P.assert_elementwise(st[..., 0], s, (nv - 1) * P.U_F32 * y64.abs().sum((1, 3)) + 1e-30, f"{what}: colstats sums")
    P.assert_elementwise(st[..., 1], q, nv * P.U_F32 * q + 1e-30, f"{what}: colstats squares")


# (name, B, H, W, Cin, K2, Cout, forced tile): one tile, the tail begins at K step 9 | ragged M (105 rows) and N (320 = 2 x 160), the seams of
# three samples inside the one row tile | a full 256 x 160 tile: the row epilogue
SHAPES = [
    ("one-tile", 2, 8, 8, 64, 128, 64, (256, 128)),
    ("ragged", 3, 5, 7, 128, 64, 320, (256, 160)),
    ("full-tile", 1, 16, 16, 64, 128, 160, (256, 160)),
]


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_tail_per_element(shape, dtype, force_plan):
    from gm_diffusion import hip_ops as ops

    name, B, H, W, ci, k2, co, (bm, bn) = shape
    force_plan(bm, bn, PP, 1)
    assert ops.gemm_plan_info(dtype, B * H * W, co, 9 * ci + k2) == (bm, bn, PP, 1)
    assert ops.shortcut_fold_ok(dtype, B, H, W, ci, k2, co)
    n0 = ops.shortcut_fold_uses
    _check(ops, f"{name} {dtype} bias", (bm, bn), B, H, W, ci, k2, co, dtype, 11, rowbias=False)
    _check(ops, f"{name} {dtype} rowbias", (bm, bn), B, H, W, ci, k2, co, dtype, 12)
    _check(ops, f"{name} {dtype} -> float32", (bm, bn), B, H, W, ci, k2, co, dtype, 13, out_dtype=F32)
    _check(ops, f"{name} {dtype} ldx2 > K2", (bm, bn), B, H, W, ci, k2, co, dtype, 14, ldx2=k2 + 72)
    # column statistics come out of the full-tile row epilogue only (M % 256 == 0, N % 160 == 0: gmd_gemm_colstats_plan): the one-tile
    # shape (128 rows, 64 columns) and the ragged one (105 rows) cannot emit them -- asked for, the launch must then run without
    y = _check(ops, f"{name} {dtype} colstats", (bm, bn), B, H, W, ci, k2, co, dtype, 15, colstats=True)
    if name == "full-tile":
        _check_colstats(ops, y, f"{name} {dtype}")
    else:
        assert getattr(y, "_colstats", None) is None
    assert ops.shortcut_fold_uses == n0 + 5


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_tail_colstats_match_the_stored_output(dtype, force_plan):
    """Column statistics of a K-tail launch over two row tiles, with a per-sample row bias."""
    from gm_diffusion import hip_ops as ops

    B, H, W, ci, k2, co = 2, 16, 16, 64, 128, 160
    force_plan(256, 160, PP, 1)
    y = _check(ops, f"colstats {dtype}", (256, 160), B, H, W, ci, k2, co, dtype, 21, colstats=True)
    _check_colstats(ops, y, f"colstats {dtype}")


# (name, Cin, K2, slices): K steps = 9 Cin / 64 + K2 / 64, a slice = ceil(steps / slices) of them.
#   128 + 192, 2 slices: 21 steps, boundary at 11 (inside the taps; the last slice crosses the seam at 18)
#   128 + 192, 3 slices: boundaries at 7 and 14 (the channel-block / tap state of a slice that starts mid-tap)
#   64 + 576, 2 slices:  18 steps, boundary at 9 = exactly the tap / tail seam (the second slice starts in the tail)
#   64 + 576, 3 slices:  boundaries at 6 and 12: the last one inside the tail
SPLITS = [("taps-2", 128, 192, 2), ("taps-3", 128, 192, 3), ("seam", 64, 576, 2), ("in-tail", 64, 576, 3)]


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("case", SPLITS, ids=[s[0] for s in SPLITS])
def test_tail_split_k_fixup_and_slabs_agree(case, dtype, force_plan):
    """Split-K over the whole K = taps + tail: in-kernel fix-up and slab reduction are each inside the per-element bound and agree bit
    for bit; two back-to-back launches on the one workspace take different inputs (a stale fragment or slab of the first would show)."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    name, ci, k2, ks = case
    B, H, W, co = 2, 16, 16, 160   # two full 256 x 160 tiles
    force_plan(256, 160, PP, ks)
    assert ops.gemm_plan_info(dtype, B * H * W, co, 9 * ci + k2) == (256, 160, PP, ks)
    outs = {}
    for fix in (4, 0):  # in-kernel reduction | slabs + reduction launch
        lib().gmd_splitk_fixup_max(fix)
        for seed in (31, 32):
            y = outs[fix, seed] = _check(ops, f"split {name} {dtype} fixup_max={fix} seed={seed}", (256, 160), B, H, W, ci, k2, co, dtype, seed,
                                         colstats=True)
            if fix:  # the finisher of the in-kernel reduction runs the row epilogue of an unsplit launch, statistics included
                _check_colstats(ops, y, f"split {name} {dtype} seed={seed}")
            else:    # the slab path reduces in a second launch, which emits none (gmd_gemm_colstats_plan answers 0)
                assert getattr(y, "_colstats", None) is None
    for seed in (31, 32):
        assert torch.equal(outs[4, seed], outs[0, seed]), f"fix-up and slab path differ ({name}, seed {seed})"
    assert not torch.equal(outs[4, 31], outs[4, 32])


# conv_patch_cont_kernel (gmd_conv_patch_override(2)): blocks of 64 channels, nine K steps per block of X and ONE per block of the tail.
#   64 + 128, unsplit:   the issue's case (16 x 16, Cin = 64, plan (256, 160)): one conv block, two tail blocks (tail -> tail patch hand-over)
#   128 + 128, 2 slices: 2 + 2 blocks, the slice boundary exactly on the seam (the second slice is tail only)
#   128 + 256, 2 slices: 2 + 4 blocks, three per slice: the first slice crosses the seam, the second starts inside the tail
PATCH = [("16x16-64", 64, 128, 1), ("seam", 128, 128, 2), ("in-tail", 128, 256, 2)]


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("case", PATCH, ids=[c[0] for c in PATCH])
def test_tail_patch_kernel_per_element(case, dtype, force_plan):
    """The K tail in the patch-resident convolution kernel, forced plan (256, 160): bias, rowbias, float32 output, ldx2 > K2, column
    statistics; split-K by fix-up and by slabs, bit-identical, with the inputs varied between back-to-back launches.  With two channel
    blocks the patch kernel adds in another order (block-major) than the per-tap kernel (tap-major): their float32 outputs differ in
    some bits, which is the evidence that this test ran the patch kernel."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    name, ci, k2, ks = case
    B, H, W, co = 2, 16, 16, 160
    force_plan(256, 160, PP, ks)
    assert ops.gemm_plan_info(dtype, B * H * W, co, 9 * ci + k2) == (256, 160, PP, ks)
    tag = f"patch {name} {dtype}"
    assert lib().gmd_conv_patch_override(0) == 0
    per_tap = _check(ops, f"{tag} (per-tap kernel)", (256, 160), B, H, W, ci, k2, co, dtype, 63, out_dtype=F32)
    assert lib().gmd_conv_patch_override(2) == 0
    y32 = _check(ops, f"{tag} -> float32", (256, 160), B, H, W, ci, k2, co, dtype, 63, out_dtype=F32)
    if ci > 64:
        assert not torch.equal(y32, per_tap), "same bits as the per-tap kernel: the patch kernel did not run"
    _check(ops, f"{tag} bias", (256, 160), B, H, W, ci, k2, co, dtype, 61, rowbias=False)
    _check(ops, f"{tag} ldx2 > K2", (256, 160), B, H, W, ci, k2, co, dtype, 64, ldx2=k2 + 72)
    outs = {}
    for fix in ((4, 0) if ks > 1 else (4,)):
        lib().gmd_splitk_fixup_max(fix)
        for seed in (65, 66):
            y = outs[fix, seed] = _check(ops, f"{tag} rowbias fixup_max={fix} seed={seed}", (256, 160), B, H, W, ci, k2, co, dtype, seed, colstats=True)
            if fix:
                _check_colstats(ops, y, f"{tag} seed={seed}")
    if ks > 1:
        for seed in (65, 66):
            assert torch.equal(outs[4, seed], outs[0, seed]), f"fix-up and slab path differ ({tag}, seed {seed})"


def run_cblk_cases():
    """Body of test_tail_with_channel_blocks; runs in a process whose library was loaded with GMD_CONV_CBLK=64."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    B, H, W, ci, k2, co = 2, 16, 16, 128, 192, 160
    for ks in (1, 2, 3):  # 21 K steps: two channel blocks of nine, three tail steps; slices of 11 / 7 start inside block 1 (and block 0)
        assert lib().gmd_gemm_plan_override(256, 160, PP, ks) == 0
        assert ops.gemm_plan_info(BF16, B * H * W, co, 9 * ci + k2) == (256, 160, PP, ks)
        for fix in ((4, 0) if ks > 1 else (4,)):
            lib().gmd_splitk_fixup_max(fix)
            _check(ops, f"cblk=64 ks={ks} fixup_max={fix}", (256, 160), B, H, W, ci, k2, co, BF16, 71 + ks)
            _check(ops, f"cblk=64 ks={ks} fixup_max={fix} -> float32", (256, 160), B, H, W, ci, k2, co, BF16, 75 + ks, out_dtype=F32, rowbias=False)
    print("CBLK_CASES_OK")


def test_tail_with_channel_blocks():
    """The ring K order with a channel block smaller than Cin (GMD_CONV_CBLK=64 at Cin = 128: all nine taps of channels 0..63, then of
    64..127, then the tail): the hand-over block -> block and last block -> tail, unsplit and with slices that start inside the second
    block.  No production shape takes a block below Cin with a tail behind it, and the block is read from the environment when the
    library is loaded, so the cases run in a child process."""
    env = dict(os.environ, GMD_TUNING="1", GMD_CONV_CBLK="64")
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r, %r]; import test_shortcut_fold_gpu as T; T.run_cblk_cases()" % (
        here, os.path.dirname(here), os.path.join(os.path.dirname(here), "gm-diffusion_amd"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "CBLK_CASES_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_tail_refusals(force_plan):
    """Stride 2, upsampling, K2 not a multiple of 64 and float32 are refused with GMD_ERR_INVALID before any launch; so is a plan whose
    kernel has no K-tail loader."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import HipExtensionError

    B, H, W, ci, k2, co = 2, 8, 8, 64, 128, 64
    x, x2, w2, wsc, b2, bsc, _ = _inputs(B, H, W, ci, k2, co, BF16, 41)
    w, b = ops.pack_shortcut(w2, b2, wsc, bsc)
    force_plan(256, 128, PP, 1)
    n0 = ops.shortcut_fold_uses
    for kw in (dict(stride=2), dict(upsample=True)):
        with pytest.raises(HipExtensionError, match="gmd error 1"):
            ops.conv3x3_tail(x, x2, w, B, H, W, bias=b, **kw)
    with pytest.raises(HipExtensionError, match="gmd error 1"):  # K2 = 96
        ops.conv3x3_tail(x, x2[..., :96].contiguous(), w[:, : 9 * ci + 96].contiguous(), B, H, W, bias=b)
    with pytest.raises(HipExtensionError, match="gmd error 1"):
        ops.conv3x3_tail(x.float(), x2.float(), w.float(), B, H, W, bias=b)
    assert not ops.shortcut_fold_ok(F32, B, H, W, ci, k2, co) and not ops.shortcut_fold_ok(BF16, B, H, W, ci, 96, co)
    force_plan(128, 128, 9, 1)  # the ring kernel: no K-tail loader
    assert not ops.shortcut_fold_ok(BF16, B, H, W, ci, k2, co)
    with pytest.raises(HipExtensionError, match="gmd error 1"):
        ops.conv3x3_tail(x, x2, w, B, H, W, bias=b)
    assert ops.shortcut_fold_uses == n0


def test_tail_matches_the_two_launches_it_replaces(force_plan):
    """Against conv_shortcut (gemm_nt, rounded to 16 bits) + conv2 with ``residual=``: the fused launch skips that one rounding, so the
    two differ by at most the rounding of the shortcut tensor plus the rounding of either stored output."""
    from gm_diffusion import hip_ops as ops

    B, H, W, ci, k2, co = 2, 16, 16, 64, 128, 160
    x, x2, w2, wsc, b2, bsc, _ = _inputs(B, H, W, ci, k2, co, BF16, 51)
    force_plan(256, 160, PP, 1)
    w, b = ops.pack_shortcut(w2, b2, wsc, bsc)
    y1, _, _ = ops.conv3x3_tail(x, x2, w, B, H, W, bias=b)
    sc = ops.gemm_nt(x2.view(-1, k2), wsc, bias=bsc).view(B, H * W, co)
    y0, _, _ = ops.conv3x3(x, w2, B, H, W, bias=b2, residual=sc)
    _, abs_dot = _reference(x, x2, w2, wsc, B, H, W, k2)
    u = P.unit_roundoff(BF16)
    # one rounding of the shortcut tensor, one of each stored output, and the float32 accumulation of either path (order unknown)
    tol = u * sc.double().abs() + 2 * u * y0.double().abs().clamp_min(y1.double().abs()) + 2 * P.accumulate_bound(abs_dot, 9 * ci + k2) + 1e-30
    assert bool(((y1.double() - y0.double()).abs() <= tol).all())
