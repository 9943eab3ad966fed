"""CPU: the host side of the conv2 + conv_shortcut fold (hip_ops.pack_shortcut / shortcut_fold_ok, gmd_conv3x3_tail): weight and bias
packing, the planner's K-step count for K = 9 Cin + K2, argument validation without a GPU, and the golden plan table left as it was."""
import json

import pytest
import torch

import plan_table


@pytest.fixture(scope="module")
def lib():
    import os

    from gm_diffusion import _native

    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _native.lib()


# SD-1.5's ResnetBlock2D with a conv_shortcut, per forward at a 64 x 64 latent: (side, conv2 Cin = Cout, shortcut K2).  Fourteen: the
# first resnet of down blocks 1 and 2 (the last down block keeps 1280 channels) and all twelve up-block resnets.
SD15_SHORTCUTS = [(32, 640, 320), (16, 1280, 640),
                  (8, 1280, 2560), (8, 1280, 2560), (8, 1280, 2560),
                  (16, 1280, 2560), (16, 1280, 2560), (16, 1280, 1920),
                  (32, 640, 1920), (32, 640, 1280), (32, 640, 960),
                  (64, 320, 960), (64, 320, 640), (64, 320, 640)]


def test_the_shape_list_is_the_models():
    from gm_diffusion.components import UNet2DConditionModel

    keys = UNet2DConditionModel().expected_keys()
    sc = [tuple(v)[:2] for k, v in keys.items() if k.endswith(".conv_shortcut.weight")]
    assert len(sc) == 14 and sorted(sc) == sorted((c, k2) for _, c, k2 in SD15_SHORTCUTS)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_pack_shortcut_copies_bits_and_sums_biases_in_float32(dtype):
    from gm_diffusion import hip_ops as ops

    g = torch.Generator().manual_seed(3)
    co, ci, k2 = 48, 64, 128
    w2 = torch.randn(co, 9 * ci, generator=g).to(dtype)
    wsc = torch.randn(co, k2, generator=g).to(dtype)
    b2 = torch.randn(co, generator=g) * 1e3
    bsc = torch.randn(co, generator=g) * 1e-3   # far apart: a 16-bit sum would lose the small one
    w, b = ops.pack_shortcut(w2, b2, wsc, bsc)
    assert w.shape == (co, 9 * ci + k2) and w.dtype == dtype and w.is_contiguous()
    assert torch.equal(w[:, : 9 * ci].view(torch.int16), w2.view(torch.int16)) and torch.equal(w[:, 9 * ci:].view(torch.int16), wsc.view(torch.int16))
    assert b.dtype == torch.float32 and torch.equal(b, b2 + bsc)
    assert torch.equal(ops.pack_shortcut(w2, None, wsc, bsc)[1], bsc) and ops.pack_shortcut(w2, None, wsc, None)[1] is None
    with pytest.raises(ops.HipExtensionError):
        ops.pack_shortcut(w2, b2, wsc[:-1], bsc)
    with pytest.raises(ops.HipExtensionError):
        ops.pack_shortcut(w2, b2, wsc.to(torch.float32), bsc)


def _slices(nk, ks):
    """K-step ranges of the slices of a split-K launch, as the kernels cut them: ceil(nk / ks) steps each."""
    per = -(-nk // ks)
    return [(s * per, min(nk, (s + 1) * per)) for s in range(ks)]


@pytest.mark.parametrize("batch", [4, 8])
@pytest.mark.parametrize("family", [0, 1])
def test_planner_counts_the_tail_in_k_steps(lib, batch, family):
    """The plan of a K-tail launch is the plan of K = 9 Cin + K2: its slices cut (9 Cin + K2) / 64 steps, every slice gets work, and
    shortcut_fold_ok says yes exactly where that plan is the 256-row ping-pong kernel."""
    from gm_diffusion import hip_ops as ops

    prev = lib.gmd_gemm_plan_family(family)
    try:
        n_ok = 0
        for side, c, k2 in SD15_SHORTCUTS:
            M, K = batch * side * side, 9 * c + k2
            bm, bn, pf, ks = ops.gemm_plan_info(torch.bfloat16, M, c, K)
            assert (bm, bn, pf, ks) == tuple(plan_table.plan_info(lib, plan_table.BF16, M, c, K, 1, ops.WORKSPACE_BYTES, 0)[1:])
            sl = _slices(K // 64, ks)
            assert sl[0][0] == 0 and sl[-1][1] == K // 64 and all(a < b for a, b in sl), (side, c, k2, ks, sl)
            ok = ops.shortcut_fold_ok(torch.bfloat16, batch, side, side, c, k2, c)
            assert ok == (pf == 283 and bm == 256)
            n_ok += ok
        if family == 1:  # the co-running family puts every level with >= 256 rows on 256-row tiles
            assert n_ok == len(SD15_SHORTCUTS)
    finally:
        lib.gmd_gemm_plan_family(prev)
    assert not ops.shortcut_fold_ok(torch.float32, 8, 64, 64, 320, 640, 320)
    assert not ops.shortcut_fold_ok(torch.bfloat16, 8, 64, 64, 320, 96, 320)


def test_tail_entry_validates_without_a_gpu(lib):
    """GMD_ERR_INVALID (1) before any launch: no second operand, float32, stride 2, upsampling, K2 % 64, a short or odd ldx2."""
    from gm_diffusion._native import GMD_BF16, GMD_F32

    a = 1 << 20  # (never dereferenced: every call is refused)

    def call(dtype=GMD_BF16, x2=a, k2=128, ldx2=128, stride=1, up=0, pad=0):
        return lib.gmd_conv3x3_tail(a, x2, a, a, dtype, dtype, 1, 8, 8, 64, k2, ldx2, 64, stride, up, pad, None, None, 0, None, 1.0, None, 0, None, 0, None)

    for kw in (dict(x2=None), dict(k2=0), dict(dtype=GMD_F32), dict(stride=2), dict(up=1), dict(stride=2, pad=1), dict(k2=96, ldx2=96), dict(ldx2=64),
               dict(ldx2=132)):
        assert call(**kw) == 1, kw
        assert b"gmd_conv3x3" in lib.gmd_last_error()


def test_golden_plan_table_rows_are_untouched(lib):
    """A sample of the golden table (every 17th census row; tests/test_gemm_plan_cpu.py checks all of them): the K tail added no branch to
    the planner."""
    with open(plan_table.TABLE) as f:
        table = json.load(f)
    ws = table["workspaces"]
    for r in table["census"][::17]:
        assert plan_table.query(lib, *r[:4], ws[r[5]], r[4]) == table["answers"][r[6]], r[:6]
