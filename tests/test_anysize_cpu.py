"""CPU: what the any-size support (image height / width divisible by 8, as the reference pipelines accept) rests on --
the nearest-neighbour index map of the fused upsample, the test-local yardstick, and the C ABI's validation of the output size."""
import os

import pytest
import torch
import torch.nn.functional as F

from anysize_ref import anysize_forward, bind


def test_nearest_to_2n_or_2n_minus_1_reads_dst_shift_1():
    """The kernels read source index ``dst >> 1`` for an upsample to ``2 n`` AND to ``2 n - 1`` (only the bound of the virtual
    image differs): pinned to torch's ``F.interpolate(size=..., mode="nearest")`` for every n in 1..599 and both sizes."""
    for n in range(1, 600):
        src = torch.arange(n, dtype=torch.float32).view(1, 1, 1, n)
        for out in (2 * n - 1, 2 * n):
            got = F.interpolate(src, size=(1, out), mode="nearest").view(-1).long()
            assert torch.equal(got, torch.arange(out) >> 1), (n, out)
            got_h = F.interpolate(src.view(1, 1, n, 1), size=(out, 1), mode="nearest").view(-1).long()
            assert torch.equal(got_h, torch.arange(out) >> 1), (n, out)


@pytest.mark.parametrize("in_ch", [4, 8])
def test_anysize_reference_equals_the_stock_oracle_on_aligned_sizes(in_ch):
    from oracle import fixtures

    ou = fixtures.build_unet("tiny", in_ch)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, in_ch, 16, 24, generator=g)
    ctx = torch.randn(2, 77, ou.config.cross_attention_dim, generator=g)
    with torch.no_grad():
        ref = ou(x, torch.tensor(500), encoder_hidden_states=ctx)[0]
        got = anysize_forward(ou, x, torch.tensor(500), encoder_hidden_states=ctx)[0]
        assert torch.equal(got, ref)
        assert torch.equal(bind(ou)(x, torch.tensor(500), encoder_hidden_states=ctx)[0], ref)


@pytest.mark.parametrize("hw", [(17, 13), (15, 30), (9, 11), (27, 48)])
def test_anysize_reference_runs_where_the_stock_oracle_raises(hw):
    from oracle import fixtures

    ou = fixtures.build_unet("tiny", 8)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 8, *hw, generator=g)
    ctx = torch.randn(1, 77, ou.config.cross_attention_dim, generator=g)
    with torch.no_grad():
        with pytest.raises(RuntimeError):
            ou(x, torch.tensor(500), encoder_hidden_states=ctx)
        y = anysize_forward(ou, x, torch.tensor(500), encoder_hidden_states=ctx)[0]
    assert y.shape == (1, 4, *hw) and bool(torch.isfinite(y).all())


@pytest.fixture(scope="module")
def native():
    from gm_diffusion import _native

    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _native


def _up(ho, wo):
    return (ho << 16) | wo  # GMD_UPSAMPLE_TO(Hout, Wout) of include/gmd_hip.h


def test_upsample_size_validation_without_gpu(native):
    """An output size outside {2 Hin - 1, 2 Hin} per axis is GMD_ERR_INVALID with a message that names it, before any pointer is
    looked at (so before any launch); the fusable query answers 0 for it."""
    lib = native.lib()

    def conv(up, dtype=native.GMD_BF16, H=17, W=30):
        out_dtype = native.GMD_F32 if dtype == native.GMD_F32S else dtype
        return lib.gmd_conv3x3(None, None, None, dtype, out_dtype, 1, H, W, 64, 64, 1, up, 0, None, None, 0, None, 1.0, None, 0, None, 0, None)

    for dtype in (native.GMD_F32, native.GMD_BF16, native.GMD_F16, native.GMD_F32S):
        for ho, wo in ((32, 60), (35, 60), (34, 58), (34, 61), (17, 30), (33, 1)):
            assert conv(_up(ho, wo), dtype) == 1, (ho, wo)  # GMD_ERR_INVALID
            assert f"{ho}x{wo}".encode() in lib.gmd_last_error() and b"17x30" in lib.gmd_last_error()
    assert conv(2) == 1 and conv(65535) == 1 and conv(-1) == 1  # neither a flag nor a packed size
    # the accepted sizes get past the size check: what stops them here is the null pointer
    for ho, wo in ((33, 60), (34, 59), (33, 59), (34, 60)):
        assert conv(_up(ho, wo)) == 1 and b"pointer" in lib.gmd_last_error()
    assert conv(1) == 1 and b"pointer" in lib.gmd_last_error()
    assert lib.gmd_conv3x3(None, None, None, native.GMD_BF16, native.GMD_BF16, 1, 17, 30, 64, 64, 2, _up(33, 60), 0, None, None, 0, None, 1.0,
                           None, 0, None, 0, None) == 1 and b"stride" in lib.gmd_last_error()
    assert lib.gmd_conv3x3_gn_fusable(native.GMD_BF16, 8, 8, 8, 1280, 1280, 1, _up(14, 16), 0, 32, 1 << 27) == 0
    assert lib.gmd_conv3x3_groupnorm(None, None, None, None, native.GMD_BF16, 8, 8, 8, 1280, 1280, 1, _up(15, 18), 0, None, None, 0, None, 1.0,
                                     32, 1e-5, None, None, 1, None, 0, None) == 1


def test_host_op_validates_out_size():
    from gm_diffusion import hip_ops
    from gm_diffusion._native import HipExtensionError

    assert hip_ops.upsample_code(17, 30, (34, 60)) == 1
    assert hip_ops.upsample_code(17, 30, (33, 59)) == (33 << 16) | 59
    for bad in ((32, 60), (35, 60), (34, 61), (0, 60)):
        with pytest.raises(HipExtensionError, match="out_size"):
            hip_ops.upsample_code(17, 30, bad)
