"""The d = 40 attention kernel on bfloat16 with ONE softmax stabiliser per query row (csrc/attention.hip, kFixedStab): the
maximum of the row's first 64 keys, never updated.  Per element against float64 (parity.attention_bound, zero violations), over
the tile geometry (one tile, a partial last tile, a partial query block, a wrapped 3-stage ring, the fused Q|K buffer), rows whose
maximum arrives tiles after the stabiliser was fixed (P far above 1, no fallback), rows that overflow the fixed stabiliser (the
row-sum net must send the block down the classic path), rows whose later P underflow to zero, and run-to-run determinism.

Every case prints ``PARITY attn40_fixed <case> max|err|/bound=<r>`` (pytest -s shows it)."""
import math

import pytest
import torch

import parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
D = 40
SCALE = D ** -0.5


def _heads(t, heads):
    B, N, C = t.shape
    return t.reshape(B, N, heads, C // heads).transpose(1, 2)


def _poisoned_vt(v, Nk):
    B, _, C = v.shape
    vt = torch.full((B, C, (Nk + 7) // 8 * 8), float("nan"), dtype=v.dtype, device=v.device)  # pad columns: the kernel must mask them
    vt[:, :, :Nk] = v.transpose(1, 2)
    return vt


def _check(q, k, v, heads, what, k_col=0, qk=None):
    """q, k, v: bfloat16 [B, N, heads * D] on the device (qk: the fused buffer that holds q and k, with k at column k_col)."""
    from gm_diffusion import hip_ops as ops

    Nk = v.shape[1]
    vt = _poisoned_vt(v, Nk)
    if qk is None:
        got = ops.attention(q, k, vt, heads, Nk, SCALE)
    else:
        got = ops.attention(qk, qk, vt, heads, Nk, SCALE, k_col=k_col)
    ref, bound = P.attention_bound(_heads(q, heads), _heads(k, heads), _heads(v, heads), SCALE, BF16)
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    r = P.assert_elementwise(_heads(got, heads), ref, bound, what, (32, D))
    print(f"PARITY attn40_fixed {what} max|err|/bound={r:.3f}")
    return got


def _late_gap_log2(q, k):
    """Per query row: (largest score over all keys) - (largest score over the first 64 keys), in log2 units -- how far P = 2^(score -
    stabiliser) rises above 1 under the fixed stabiliser.  float64 from the bfloat16 values; q, k: [B, N, D], one head."""
    s = (q.double() @ k.double().transpose(-1, -2)) * (SCALE * math.log2(math.e))
    return s.amax(-1) - s[..., :64].amax(-1)


@pytest.mark.parametrize("Nq,Nk", [(128, 64), (64, 77), (200, 130), (256, 320)])
def test_fixed_stabiliser_tile_geometry(Nq, Nk):
    """One tile; the cross-attention's partial second tile; a partial query block with a partial last tile; five tiles (the ring wraps)."""
    heads, B = 2, 2
    g = torch.Generator().manual_seed(D * 7 + Nq + Nk)
    q, k, v = (torch.randn(B, n, heads * D, generator=g).to(BF16).to(DEV) for n in (Nq, Nk, Nk))
    _check(q, k, v, heads, f"Nq={Nq} Nk={Nk}")


def test_fixed_stabiliser_fused_qk_buffer():
    heads, B, N = 8, 2, 256
    C = heads * D
    g = torch.Generator().manual_seed(5)
    qk = torch.randn(B, N, 2 * C, generator=g).to(BF16).to(DEV)
    v = torch.randn(B, N, C, generator=g).to(BF16).to(DEV)
    _check(qk[:, :, :C], qk[:, :, C:], v, heads, "fused-qk N=256 heads=8", k_col=C, qk=qk)


def _spiked(spike):
    """The generator of test_kernels_gpu.test_attention_rescale_branch_spiked_keys: query 5 meets a huge score at key 200 (4th tile),
    query 100 a larger one at key 310 (5th tile)."""
    N = 320
    g = torch.Generator().manual_seed(77)
    q = torch.randn(1, N, D, generator=g)
    k = torch.randn(1, N, D, generator=g) * 0.3
    v = torch.randn(1, N, D, generator=g)
    k[0, 200] = q[0, 5] * spike
    k[0, 310] = q[0, 100] * (spike + 1.0)
    return q.to(BF16).to(DEV), k.to(BF16).to(DEV), v.to(BF16).to(DEV)


@pytest.mark.parametrize("spike", [1.5, 3.0, 8.0, 16.0])
def test_row_maximum_arrives_late_without_fallback(spike):
    """The row maximum lies tiles after the stabiliser was fixed: P rises far above 1 (up to ~2^117 at spike 16) but every row sum stays
    below the net's 2^120, so the fixed-stabiliser result itself is what is checked."""
    q, k, v = _spiked(spike)
    gap = float(_late_gap_log2(q, k).max())
    print(f"spike {spike}: largest score - first-tile maximum = {gap:.1f} log2 units")
    assert gap < 119.0, "this case is meant to stay under the overflow net"
    _check(q, k, v, 1, f"late maximum spike={spike}")


@pytest.mark.parametrize("spike", [20.0, 30.0])
def test_overflow_net_takes_the_classic_path(spike):
    """Rows more than 128 log2 units above their first tile: P overflows to +inf, the row-sum net must catch it and the block must
    come back finite and within the bound through the classic maximum-first path."""
    q, k, v = _spiked(spike)
    gap = _late_gap_log2(q, k)
    print(f"spike {spike}: {int((gap > 128).sum())} rows more than 128 log2 units above their first tile (max {float(gap.max()):.1f})")
    assert int((gap > 128).sum()) >= 1, "this case is meant to overflow the fixed stabiliser"
    _check(q, k, v, 1, f"overflow net spike={spike}")


def test_first_tile_far_above_the_rest():
    """k[7] = 25 q[9]: row 9 fixes a stabiliser so high that every later P underflows to zero."""
    N = 200
    g = torch.Generator().manual_seed(9)
    q = torch.randn(1, N, D, generator=g)
    k = torch.randn(1, N, D, generator=g) * 0.3
    v = torch.randn(1, N, D, generator=g)
    k[0, 7] = q[0, 9] * 25.0
    q, k, v = (t.to(BF16).to(DEV) for t in (q, k, v))
    _check(q, k, v, 1, "first tile far above the rest")


def test_two_launches_are_bit_identical():
    from gm_diffusion import hip_ops as ops

    heads, B, Nq, Nk = 2, 2, 200, 320
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(B, n, heads * D, generator=g).to(BF16).to(DEV) for n in (Nq, Nk, Nk))
    vt = _poisoned_vt(v, Nk)
    a = ops.attention(q, k, vt, heads, Nk, SCALE)
    b = ops.attention(q, k, vt, heads, Nk, SCALE)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
