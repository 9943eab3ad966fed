"""CPU: the host side of the upsampling convolution as four 2x2 phase convolutions (hip_ops.pack_upsample_phases /
upsample_phases_ok, gmd_conv3x3_up2_plan, gmd_conv3x3_up2): the tap map and the padding in float64, the single rounding of the packed
weights, the plan query and the argument checks that need no GPU."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64


def phase_convs(x, wp):
    """Reference use of the packed weights, written from the documented layout alone: x [B, Cin, H, W], wp [4, Cout, 4*Cin] ->
    [B, Cout, 2H, 2W].  Tap (a, b) of phase (py, px) reads source pixel (i + a + py - 1, j + b + px - 1), zero outside the image."""
    B, ci, H, W = x.shape
    co = wp.shape[1]
    xp = F.pad(x, (1, 1, 1, 1))  # xp[.., u + 1, v + 1] = x[.., u, v]
    out = torch.zeros(B, co, 2 * H, 2 * W, dtype=x.dtype)
    for py, px in itertools.product(range(2), range(2)):
        acc = torch.zeros(B, co, H, W, dtype=x.dtype)
        for a, b in itertools.product(range(2), range(2)):
            wt = wp[2 * py + px, :, (2 * a + b) * ci:(2 * a + b + 1) * ci]  # [Cout, Cin]
            src = xp[:, :, a + py:a + py + H, b + px:b + px + W]           # source pixel (i + a + py - 1, j + b + px - 1)
            acc += torch.einsum("bchw,oc->bohw", src, wt)
        out[:, :, py::2, px::2] = acc
    return out


@pytest.mark.parametrize("H,W", [(h, w) for h in (1, 2, 3, 8) for w in (1, 2, 3, 8)])
def test_packing_and_four_phase_convolutions_equal_the_upsampled_conv3x3(H, W):
    """float64: interleaving the four 2x2 convolutions over the low-resolution image gives conv3x3(nearest 2x) to round-off, at
    every size in {1, 2, 3, 8}^2 (1: every tap but the centre window is padding; non-square: the x and y rules are not swapped)."""
    from gm_diffusion import hip_ops as ops

    g = torch.Generator().manual_seed(100 * H + W)
    B, ci, co = 2, 3, 5
    x = torch.randn(B, ci, H, W, generator=g, dtype=F64)
    w = torch.randn(co, ci, 3, 3, generator=g, dtype=F64)
    bias = torch.randn(co, generator=g)
    wp, b = ops.pack_upsample_phases(w.permute(0, 2, 3, 1).reshape(co, 9 * ci).contiguous(), bias)
    assert wp.shape == (4, co, 4 * ci) and wp.dtype == F64 and b is bias
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    got = phase_convs(x, wp)
    # every output is a sum of 9 Cin products (4 Cin after merging): a few float64 roundings of sum |x||w|
    mag = F.conv2d(F.interpolate(x.abs(), scale_factor=2, mode="nearest"), w.abs(), padding=1)
    assert bool(((got - ref).abs() <= 32 * 2.0 ** -53 * mag + 1e-300).all()), float((got - ref).abs().max())


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_packed_weights_are_float32_sums_rounded_once(dtype):
    from gm_diffusion import hip_ops as ops

    g = torch.Generator().manual_seed(5)
    co, ci = 7, 64
    w = (torch.randn(co, 9 * ci, generator=g) * 0.05).to(dtype)
    wp, b = ops.pack_upsample_phases(w)
    assert b is None and wp.dtype == dtype and wp.shape == (4, co, 4 * ci) and wp.is_contiguous()
    w9 = w.float().view(co, 3, 3, ci)
    rows = (((0,), (1, 2)), ((0, 1), (2,)))
    for py, px, a, bb in itertools.product(range(2), repeat=4):
        s = sum(w9[:, ky, kx] for ky in rows[py][a] for kx in rows[px][bb])  # at most four float32 adds of 16-bit values
        assert torch.equal(wp[2 * py + px, :, (2 * a + bb) * ci:(2 * a + bb + 1) * ci], s.to(dtype)), (py, px, a, bb)
    # the corner taps are single nine-tap weights: copied bit for bit
    assert torch.equal(wp[0, :, :ci], w[:, :ci]) and torch.equal(wp[3, :, 3 * ci:], w[:, 8 * ci:])


def test_pack_refuses_what_it_cannot_pack():
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import HipExtensionError

    with pytest.raises(HipExtensionError):
        ops.pack_upsample_phases(torch.zeros(4, 100))
    w = torch.zeros(4, 9 * 64, dtype=BF16)
    w._alpha = 0.5
    with pytest.raises(HipExtensionError):
        ops.pack_upsample_phases(w)


@pytest.fixture
def family():
    from gm_diffusion._native import lib

    prev = lib().gmd_gemm_plan_family(-1)

    def set_family(f):
        lib().gmd_gemm_plan_family(f)

    yield set_family
    lib().gmd_gemm_plan_family(prev)


def test_plan_query_of_the_phase_launch(family):
    """gmd_conv3x3_up2_plan is host arithmetic: the SD-1.5 UNet and VAE upsamplers under both plan families, and the refusals."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    def plan(dtype, B, H, W, ci, co, bucket=0):
        out = (ctypes.c_int * 4)()
        ok = lib().gmd_conv3x3_up2_plan(ops.dtype_code(dtype), B, H, W, ci, co, bucket, ops.WORKSPACE_BYTES, ctypes.addressof(out))
        return tuple(out) if ok else None

    family(1)  # the co-running family: 256-row tiles everywhere, filled up with K slices
    assert plan(BF16, 8, 32, 32, 640, 640, 10) == (256, 160, 283, 1)     # 128 M-panels x 4 N tiles
    assert plan(BF16, 8, 16, 16, 1280, 1280, 10) == (256, 160, 283, 1)   # 32 x 8 = 256 tiles
    assert plan(BF16, 8, 8, 8, 1280, 1280, 10) == (256, 160, 283, 2)     # 8 x 8 tiles: two K slices of 40 steps
    assert plan(F16, 4, 8, 8, 1280, 1280, 10) == (256, 160, 283, 4)
    assert plan(BF16, 3, 8, 8, 128, 160, 10) == (256, 160, 283, 1)       # a partial panel (192 rows) with statistics
    assert plan(BF16, 1, 16, 16, 64, 128) == (256, 128, 283, 1)
    # statistics need 64-row blocks inside a sample and whole 10-channel buckets per wave tile (80 columns, not 64)
    assert plan(BF16, 4, 6, 6, 128, 160, 10) is None and plan(BF16, 4, 6, 6, 128, 160) == (256, 160, 283, 1)
    assert plan(BF16, 1, 16, 16, 64, 128, 10) is None
    for bad in ((F32, 8, 32, 32, 640, 640), (BF16, 8, 32, 32, 96, 640), (BF16, 0, 32, 32, 640, 640), (BF16, 8, 32, 32, 640, 100)):
        assert plan(*bad) is None, bad
    assert lib().gmd_conv3x3_up2_plan(ops.GMD_BF16, 8, 32, 32, 640, 640, 0, ops.WORKSPACE_BYTES, None) == 1  # out4 may be NULL
    family(0)  # launch by launch: the ping-pong kernel only from 256 tiles up
    assert plan(BF16, 8, 32, 32, 640, 640, 10) == (256, 160, 283, 1)
    assert plan(BF16, 4, 64, 64, 512, 512) == (256, 128, 283, 1)         # the VAE decoder's upsamplers at a 512 x 512 image
    assert plan(BF16, 4, 128, 128, 512, 512) == (256, 128, 283, 1)
    assert plan(BF16, 4, 256, 256, 256, 256) == (256, 128, 283, 1)
    assert plan(BF16, 4, 16, 16, 1280, 1280) is None                    # 128 tiles: the loader / consumer kernels' territory
    # the nine-tap launches' plans are what they were (the query asks make_plan, it does not change it)
    assert ops.gemm_plan_info(BF16, 8 * 64 * 64, 640, 9 * 640) == (256, 160, 283, 1)


def test_upsample_phases_ok_conditions(family, monkeypatch):
    from gm_diffusion import hip_ops as ops

    family(1)
    assert ops.upsample_phases_ok(BF16, 8, 32, 32, 640, 640, (64, 64), colstats=True)
    assert ops.upsample_phases_ok(BF16, 8, 32, 32, 640, 640)                       # out_size None = exactly 2x
    assert not ops.upsample_phases_ok(BF16, 8, 32, 32, 640, 640, (63, 64))         # 2H - 1: the nine-tap launch
    assert not ops.upsample_phases_ok(BF16, 8, 32, 32, 640, 640, (64, 63))
    assert not ops.upsample_phases_ok(F32, 8, 32, 32, 640, 640) and not ops.upsample_phases_ok(BF16, 8, 32, 32, 96, 640)
    assert ops.upsample_phases_plan(BF16, 8, 8, 8, 1280, 1280, colstats=True) == (256, 160, 283, 2)
    monkeypatch.setattr(ops, "USE_UPSAMPLE_PHASES", False)                         # GMD_UPSAMPLE_PHASES=0
    assert not ops.upsample_phases_ok(BF16, 8, 32, 32, 640, 640, (64, 64))


def test_entry_point_validates_without_a_gpu():
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    a = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before a launch

    def call(dtype=ops.GMD_BF16, out_dtype=ops.GMD_BF16, B=1, H=8, W=8, ci=64, co=64, x=a, bias=None, cs=None, bucket=0):
        return lib().gmd_conv3x3_up2(x, a, a, dtype, out_dtype, B, H, W, ci, co, bias, None, 0, None, cs, bucket, None, 0, None)

    assert call(dtype=ops.GMD_F32, out_dtype=ops.GMD_F32) == 1 and b"16-bit" in lib().gmd_last_error()
    assert call(ci=96) == 1 and b"multiple of 64" in lib().gmd_last_error()
    assert call(x=None) == 1 and call(out_dtype=ops.GMD_F16) == 1 and call(H=0) == 1
    assert call(bias=ctypes.c_void_p(4100)) == 1
    assert call(cs=a, bucket=0) == 1
    assert call(B=0) == 0  # an empty batch is a no-op
    assert call(B=1, H=2, W=2) == 3 and b"gmd_conv3x3_up2_plan" in lib().gmd_last_error()  # 16 rows: no ping-pong plan (UNSUPPORTED)
