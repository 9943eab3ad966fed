"""Tile-edge sweeps of the four attention kernels (csrc/attention.hip: attn_fwd_kernel and attn40_kernel; csrc/attention_ip.hip;
csrc/attention_split.hip): key counts on, next to and one 8-key chunk away from every tile edge, query counts on every wave and
query-block edge, every workgroup count the XCD remap distinguishes, the causal diagonal at tile edges, every image-key count.

Every case is per element with ZERO violations against the float64 reference and the derived bounds of tests/parity.py /
tests/ip_adapter_ref.py (no tolerance of this file's own), on the edge-weighted operands of tests/attn_cases.py -- a dropped, duplicated
or admitted edge key moves a designated row by ~|v| at any key count; tests/test_attn_edges_cpu.py shows that each such defect breaks
these very bounds for every case below -- and in attn_cases.HostileLayout: column-offset Q and K, padded strides, NaN in every element
the kernel may not use, the output inside a NaN-prefilled guarded buffer of which nothing outside the [B, Nq, H D] window may change
and everything inside must be finite.  Each case prints ``PARITY attention-edges <case> max|err|/bound=<r>`` (pytest -s)."""
import pytest
import torch

import attn_cases as C
import ip_adapter_ref as R
import parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
NAME = {BF16: "bf16", F16: "f16", F32: "f32"}


@pytest.fixture
def split_mode():
    from gm_diffusion import hip_ops as ops

    prev = ops.set_f32_mode("split")
    yield ops
    ops.set_f32_mode(prev)


def _report(case, r):
    print(f"PARITY attention-edges {case} max|err|/bound={r:.3f}")
    return r


def _ok(rc, what):
    from gm_diffusion._native import lib

    assert rc == 0, f"{what}: status {rc}: {lib().gmd_last_error()}"
    torch.cuda.synchronize()


def _plain_case(B, H, Nq, Nk, D, dtype, seed, what, causal=False, shared=False):
    """One case of gmd_attention (16-bit types, or float32 through the split kernel) over all its rotations: footprint, then per element."""
    from gm_diffusion import hip_ops as ops

    worst = 0.0
    for rot in range(C.rotations(Nq, Nk, causal=causal)):
        q, k, v, _ = C.edge_weighted_qkv(B, H, Nq, Nk, D, dtype, seed, causal=causal, rotate=rot)
        lay = C.HostileLayout(q, k, v, DEV, shared=shared)
        w = f"{what} rot={rot}"
        _ok(C.launch_attention(lay, D ** -0.5, causal=causal, code=ops.GMD_F32S if dtype == F32 else None), w)
        lay.assert_footprint(w)
        if dtype == F32:
            ref, bound = P.attention_split_bound(q.to(DEV), k.to(DEV), v.to(DEV), D ** -0.5)
        else:
            ref, bound = P.attention_bound(q.to(DEV), k.to(DEV), v.to(DEV), D ** -0.5, dtype, causal=causal)
        worst = max(worst, P.assert_elementwise(lay.out(), ref, bound, w, tile=(32, D)))
    return _report(what, worst)


def _scales(value, idx, n=16):
    """A 16-entry device array with ``value`` at ``idx`` and a value that would be noticed (1e4) everywhere else."""
    s = torch.full((n,), 1.0e4, dtype=torch.float32)
    s[idx] = value
    return s.to(DEV)


def _ip_case(B, H, Nq, Nk, Nip, D, dtype, ip_scale, idx, seed, what, shared=False):
    worst = 0.0
    for rot in range(C.rotations(Nq, Nk, Nip=Nip)):
        q, k, v, kip, vip, _ = C.edge_weighted_qkv(B, H, Nq, Nk, D, dtype, seed, rotate=rot, Nip=Nip)
        lay = C.HostileLayout(q, k, v, DEV, shared=shared, kip=kip, vip=vip)
        w = f"{what} rot={rot}"
        _ok(C.launch_attention_ip(lay, D ** -0.5, _scales(ip_scale, idx), idx), w)
        lay.assert_footprint(w)
        ref, bound = R.decoupled_bound(q.to(DEV), k.to(DEV), v.to(DEV), kip.to(DEV), vip.to(DEV), D ** -0.5, ip_scale, dtype)
        worst = max(worst, P.assert_elementwise(lay.out(), ref, bound, w, tile=(32, D)))
    return _report(what, worst)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D", C.HEAD_DIMS)
def test_key_edges(D, dtype):
    """All 61 key counts of K_EDGES at B = 1, H = 2, Nq = 160: two query blocks, the second with one valid wave.  K alternates between
    the fused Q|K buffer and a buffer of its own."""
    for i, Nk in enumerate(C.K_EDGES):
        _plain_case(1, 2, 160, Nk, D, dtype, 1000 * D + Nk, f"keys D={D} {NAME[dtype]} Nk={Nk}", shared=i % 2 == 0)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D", C.HEAD_DIMS)
def test_query_edges(D, dtype):
    """All of Q_EDGES against a ragged (77) and an exactly full three-tile (192) key count.  Nq = 1 has fewer rows than designated
    keys and runs once per role (attn_cases.rotations)."""
    for i, Nq in enumerate(C.Q_EDGES):
        for Nk in (77, 192):
            _plain_case(1, 2, Nq, Nk, D, dtype, 1000 * D + 7 * Nq + Nk, f"queries D={D} {NAME[dtype]} Nq={Nq} Nk={Nk}", shared=i % 2 == 1)


@pytest.mark.parametrize("kernel", ["d32", "d40", "ip40", "split40"])
def test_grid_sweep(kernel, split_mode):
    """Every workgroup count 1 .. 33, 63, 64, 65 (nwg & 7 = 0 .. 7 with nwg >> 3 = 0 and >= 1) through the XCD remap of each kernel:
    attn_fwd_kernel (D = 32), attn40_kernel (D = 40; bfloat16: fixed stabiliser, float16: lagged), attn_ip (D = 40) and the float32
    split kernel (D = 40), Nk = 72.  A remap that is not a bijection leaves a block NaN or stores one twice with another's data."""
    D = 32 if kernel == "d32" else 40
    for B, H, Nq in C.GRIDS:
        n = C.workgroups(B, H, Nq)
        for dtype in ((F32,) if kernel == "split40" else (BF16, F16)):
            what = f"grid {kernel} {NAME[dtype]} nwg={n} B={B} H={H} Nq={Nq}"
            if kernel == "ip40":
                _ip_case(B, H, Nq, 72, 4, D, dtype, 0.6, n % 16, 100 * n + D, what, shared=n % 2 == 0)
            else:
                _plain_case(B, H, Nq, 72, D, dtype, 100 * n + D, what, shared=n % 2 == 0)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D", [32, 64])
def test_causal_edges(D, dtype):
    """Nq = Nk over CAUSAL_N: the diagonal key at every tile edge dominates its own row, and its copy in the row above would be
    dominated by the first masked key (attn_cases.edge_weighted_qkv, three rotations)."""
    for i, N in enumerate(C.CAUSAL_N):
        _plain_case(1, 2, N, N, D, dtype, 1000 * D + N, f"causal D={D} {NAME[dtype]} N={N}", causal=True, shared=i % 2 == 0)


@pytest.mark.parametrize("D", [40, 64, 80, 160])
def test_split_key_edges(D, split_mode):
    """The float32 three-product kernel over K_EDGES at B = 1, H = 4 (H D whole 32-element chunks), Nq = 160: the plain output in the
    hostile layout, and the pre-split output (GMD_F32SA: contiguous rows, so ldo = H D inside the guarded buffer) read back through the
    documented layout."""
    ops = split_mode
    B, H, Nq = 1, 4, 160
    for i, Nk in enumerate(C.K_EDGES):
        what = f"split D={D} Nk={Nk}"
        worst = _plain_case(B, H, Nq, Nk, D, F32, 1000 * D + Nk, what, shared=i % 2 == 0)
        q, k, v, _ = C.edge_weighted_qkv(B, H, Nq, Nk, D, F32, 1000 * D + Nk)
        lay = C.HostileLayout(q, k, v, DEV, shared=i % 2 == 1, tight_out=True)
        _ok(C.launch_attention(lay, D ** -0.5, code=ops.GMD_F32SA), what + " pre-split")
        lay.guard.assert_untouched_outside(lay.window, what + " pre-split")
        stored = lay.guard.t.view(B, Nq, H * D)
        assert not bool(P.split_layout_violations(stored).any()), what + ": a stored piece is not a (hi, lo) split (or was never written)"
        ref, bound = P.attention_split_bound(q.to(DEV), k.to(DEV), v.to(DEV), D ** -0.5)
        got = P.unsplit(stored).view(B, Nq, H, D).permute(0, 2, 1, 3)
        worst = max(worst, P.assert_elementwise(got, ref, P.presplit_read_bound(ref, bound), what + " pre-split", tile=(32, D)))
        _report(what + " pre-split", worst)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D", C.HEAD_DIMS)
def test_ip_image_key_edges(D, dtype):
    """Every image-key count 1 .. 64 (one tile: every chunk validity of the image branch), the text key count cycling through
    8 / 63 / 64 / 65 / 77; the first and last image key and the text edge keys dominate designated rows.  The scale cycles over the
    four values of tests/test_ip_adapter_gpu.py; each count runs with two consecutive ones, so none is left with ip_scale = 0 only."""
    for i, Nip in enumerate(range(1, 65)):
        for s in (C.IP_SCALES[i % 4], C.IP_SCALES[(i + 1) % 4]):
            _ip_case(1, 2, 160, C.IP_NK[i % 5], Nip, D, dtype, s, (0, 15)[i % 2], 1000 * D + Nip,
                     f"ip D={D} {NAME[dtype]} Nip={Nip} Nk={C.IP_NK[i % 5]} s={s}", shared=i % 2 == 0)


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_attn40_ring_is_repeatable_at_edges(dtype):
    """The three-stage LDS-DMA ring of attn40_kernel with its hand-counted waits, at one, two, three and six exactly full tiles and one
    key past them: five launches of the same operands store the same bits (a wait that is one piece short reads a stage before its
    DMA landed, which shows as a run-to-run difference long before it shows as an error).  A plain repeat on an idle device; the
    co-running variant is tests/test_attn40_fixed_gpu.py's."""
    D, B, H, Nq = 40, 2, 5, 300
    for Nk in (64, 65, 128, 192, 193, 384):
        q, k, v, _ = C.edge_weighted_qkv(B, H, Nq, Nk, D, dtype, 40000 + Nk)
        lay = C.HostileLayout(q, k, v, DEV, shared=Nk % 2 == 0)
        what = f"attn40 repeat {NAME[dtype]} Nk={Nk}"
        first = None
        for n in range(5):
            lay.fresh_output()
            _ok(C.launch_attention(lay, D ** -0.5), what)
            if first is None:
                lay.assert_footprint(what)
                ref, bound = P.attention_bound(q.to(DEV), k.to(DEV), v.to(DEV), D ** -0.5, dtype)
                _report(what, P.assert_elementwise(lay.out(), ref, bound, what, tile=(32, D)))
                first = lay.guard.buf.clone()
            else:
                diff = lay.guard.buf != first
                assert not bool(diff.any()), f"{what}: launch {n + 1} differs from the first in {int(diff.sum())} bytes"
