"""CPU: the two resampling definitions of csrc/resample.hip (tests/resample_ref.py) against torch's and PIL's own resizers, and the
argument validation of the two entry points -- no GPU is touched."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_ref as R

SHAPES = [((8, 16), (37, 53)), ((64, 64), (135, 240)), ((37, 53), (8, 16)), ((100, 7), (9, 7)), ((20, 36), (20, 36))]


@pytest.mark.parametrize("src,dst", SHAPES)
def test_definitions_agree_with_interpolate_in_float64(src, dst):
    (h, w), (H, W) = src, dst
    x = torch.rand(2, 3, h, w, dtype=torch.float64, generator=torch.Generator().manual_seed(h * w + H))
    plain = R.resize(x, R.bilinear_matrix(h, H), R.bilinear_matrix(w, W))
    err = float((plain - F.interpolate(x, (H, W), mode="bilinear", align_corners=False)).abs().max())
    print(f"bilinear {src}->{dst}: max |def - F.interpolate| = {err:.3e}")
    assert err <= 1e-12
    aa = R.resize(x, R.antialias_matrix(h, H), R.antialias_matrix(w, W))
    err = float((aa - F.interpolate(x, (H, W), mode="bilinear", align_corners=False, antialias=True)).abs().max())
    print(f"antialias {src}->{dst}: max |def - F.interpolate| = {err:.3e}")
    assert err <= 1e-12
    if (h, w) == (H, W):
        assert torch.equal(plain, x) and torch.equal(aa, x)


@pytest.mark.parametrize("src,dst", SHAPES)
def test_antialias_definition_within_one_code_of_pil(src, dst):
    """PIL rounds to a byte after each of its two passes (<= 1.0 code from exact); rounding the definition adds <= 0.5: the integer
    difference is below 2.  Measured here: 1 code at most on these shapes."""
    from PIL import Image

    (h, w), (H, W) = src, dst
    u8 = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(h + 7 * W))
    ours = torch.round(R.resize(u8.permute(2, 0, 1), R.antialias_matrix(h, H), R.antialias_matrix(w, W))).permute(1, 2, 0)
    pil = torch.from_numpy(np.array(Image.fromarray(u8.numpy()).resize((W, H), Image.BILINEAR))).to(torch.float64)
    diff = float((ours - pil).abs().max())
    print(f"{src}->{dst}: max |round(255 def) - PIL| = {diff:.0f} codes")
    assert diff <= 1


def test_weights_are_rows_of_a_partition_of_unity():
    for n_in, n_out in ((53, 16), (16, 53), (2160, 288), (7, 7), (1, 5), (5, 1)):
        for m in (R.bilinear_matrix(n_in, n_out), R.antialias_matrix(n_in, n_out)):
            assert m.shape == (n_out, n_in) and bool((m >= 0).all())
            assert float((m.sum(1) - 1).abs().max()) <= 1e-15


@pytest.fixture(scope="module")
def native():
    from gm_diffusion import _native

    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _native


def test_entry_points_reject_bad_arguments_without_a_gpu(native):
    lib = native.lib()
    buf = ctypes.create_string_buffer(64)  # a non-null, 16-byte-capable address that is never dereferenced: every call below is refused
    p = (ctypes.addressof(buf) + 15) & ~15
    INVALID = 1

    def tail(sdr=p, hs=8, ws=8, gm=p, hg=8, wg=8, dtype=0, layout=0, B=1, H=16, W=16, flags=0, outs=(None,) * 8):
        return lib.gmd_hdr_tail_resized(sdr, hs, ws, gm, hg, wg, dtype, layout, B, H, W, 99.0, 1 / 64, flags, *outs, None)

    assert tail(sdr=None) == INVALID and b"null" in lib.gmd_last_error()
    assert tail(gm=None) == INVALID
    assert tail(B=0) == INVALID
    for kw in (dict(hs=0), dict(ws=-3), dict(hg=0), dict(wg=0), dict(H=0), dict(W=0), dict(H=16385), dict(ws=1 << 20), dict(hg=16385)):
        assert tail(**kw) == INVALID, kw
        assert b"1..16384" in lib.gmd_last_error()
    assert tail(layout=3) == INVALID and b"in_layout" in lib.gmd_last_error()
    assert tail(layout=-1) == INVALID
    assert tail(dtype=3) == INVALID and b"dtype" in lib.gmd_last_error()
    assert tail(flags=4) == INVALID and b"flags" in lib.gmd_last_error()
    assert tail(flags=2, hs=8, ws=8, H=16, W=16) == INVALID and b"uint8 source" in lib.gmd_last_error()
    assert tail(gm=p + 2) == INVALID and b"unaligned" in lib.gmd_last_error()      # float32 operand on a 2-byte boundary
    assert tail(sdr=p + 1, dtype=1) == INVALID and b"unaligned" in lib.gmd_last_error()
    for k, off in ((0, 2), (4, 1), (5, 2), (6, 1), (7, 2)):                        # sdr, hdr, hdr_file (4), hdr_u16 (2), hdr_rgbe (4)
        outs = [None] * 8
        outs[k] = p + off
        assert tail(outs=tuple(outs)) == INVALID and b"unaligned output" in lib.gmd_last_error(), k

    def prep(src=p, B=1, h=8, w=8, out=p, dtype=0, layout=0, cp=8, H=4, W=4):
        return lib.gmd_prepare_sdr(src, B, h, w, out, dtype, layout, cp, H, W, None)

    assert prep(src=None) == INVALID and b"null" in lib.gmd_last_error()
    assert prep(out=None) == INVALID
    assert prep(B=0) == INVALID
    for kw in (dict(h=0), dict(w=0), dict(H=0), dict(W=-1), dict(h=16385), dict(W=16385)):
        assert prep(**kw) == INVALID, kw
        assert b"1..16384" in lib.gmd_last_error()
    assert prep(layout=2) == INVALID and b"out_layout" in lib.gmd_last_error()
    assert prep(layout=1, cp=2) == INVALID and b"cp" in lib.gmd_last_error()
    assert prep(layout=1, cp=65) == INVALID
    assert prep(dtype=4) == INVALID and b"dtype" in lib.gmd_last_error()
    assert prep(out=p + 2) == INVALID and b"unaligned" in lib.gmd_last_error()
    assert prep(out=p + 1, dtype=2) == INVALID


def test_front_ends_refuse_host_tensors():
    from gm_diffusion import hdr, hip_ops
    from gm_diffusion._native import HipExtensionError

    z = torch.zeros(1, 3, 8, 8)
    with pytest.raises(HipExtensionError):
        hip_ops.hdr_tail_resized(z, z, 0, (16, 16))
    with pytest.raises(HipExtensionError):
        hip_ops.prepare_sdr(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 4))
    with pytest.raises(HipExtensionError):
        hdr.prepare_sdr(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 4))
    with pytest.raises(HipExtensionError):
        hdr.recompose(z, z, out_size=(16, 16))
