"""GPU: the two resampling kernels (csrc/resample.hip) against the float64 definitions of tests/resample_ref.py, element by element
(allowed violations: 0), their identity cases against the existing tail bit for bit, their write footprint, and the full-resolution
path end to end on the tiny GM pipeline."""
import os

import numpy as np
import pytest
import torch

import parity as P
import resample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
QMAX = 99.0
SEVEN = ("sdr", "gm", "sdr_u8", "gm_u8", "hdr", "hdr_file", "hdr_u16")
EIGHT = SEVEN + ("hdr_rgbe",)


def ops():
    from gm_diffusion import hip_ops

    return hip_ops


def _lay(x, layout):
    """NCHW decoder output -> the tail's layout (2: a fourth channel the kernel must ignore)."""
    if layout == 0:
        return x.contiguous()
    n = x.permute(0, 2, 3, 1)
    if layout == 2:
        n = torch.cat([n, torch.full_like(n[..., :1], 7.0)], -1)
    return n.reshape(x.shape[0], x.shape[2] * x.shape[3], -1).contiguous()


def _dec(shape, dtype, g):
    """Decoder-like values: mostly inside [-1, 1], some beyond (the clamp's two sides)."""
    return (torch.rand(shape, generator=g) * 2.4 - 1.2).to(dtype)


def _u8_codes(x64):
    return torch.floor(x64 * 255).clamp(0, 255)


def _check_integer_outputs(out, ref, what):
    """Quantisers: exact given the kernel's OWN float outputs (oracle restatements), and every code within 1 of the float64 reference's."""
    from oracle import hdr_ops as H

    for k in ("sdr", "gm"):
        own = out[k].cpu().numpy()
        assert np.array_equal(out[k + "_u8"].cpu().numpy(), H.quantize_u8_trunc(own)), f"{what}: {k}_u8 is not trunc(255 x) of the kernel's {k}"
        d = (out[k + "_u8"].cpu().to(torch.float64) - _u8_codes(ref[k])).abs().max()
        assert float(d) <= 1, f"{what}: {k}_u8 is {float(d)} codes from the float64 reference"
    hf = out["hdr_file"].cpu().numpy()
    assert np.array_equal(out["hdr_u16"].cpu().numpy(), H.quantize_u16_codes(hf)), f"{what}: hdr_u16"
    ref_u16 = torch.from_numpy(np.rint(np.clip(ref["hdr_file"].numpy() * 65535.0, 0, 65535.0)))
    d = (torch.from_numpy(out["hdr_u16"].cpu().numpy().astype(np.float64)) - ref_u16).abs().max()
    assert float(d) <= 1, f"{what}: hdr_u16 is {float(d)} codes from the float64 reference"
    px = out["hdr_rgbe"].cpu().numpy()
    assert np.array_equal(px, H.rgbe_encode(hf)), f"{what}: hdr_rgbe is not Ward's encoding of the kernel's hdr_file"
    assert torch.equal(out["hdr_rgbe"], ops().rgbe_encode(out["hdr_file"])), f"{what}: hdr_rgbe differs from gmd_rgbe_encode"
    # against the float64 reference: the shared exponent byte within 1 everywhere; where it agrees, every mantissa byte within 1; where
    # the brightest channel sits on a power of two and the exponent byte moved, the mantissas are on another scale (255 <-> 128) and
    # the decoded values are compared instead, to one code step of the larger exponent
    rpx = H.rgbe_encode(ref["hdr_file"].numpy().astype(np.float32)).astype(np.int64)
    gpx = px.astype(np.int64)
    assert np.abs(gpx[..., 3] - rpx[..., 3]).max() <= 1, f"{what}: RGBE exponent byte more than 1 from the reference"
    same = gpx[..., 3] == rpx[..., 3]
    assert np.abs(gpx[same][:, :3] - rpx[same][:, :3]).max(initial=0) <= 1, f"{what}: RGBE mantissa byte more than 1 from the reference"
    if (~same).any():
        step = np.ldexp(1.0, np.maximum(gpx[..., 3], rpx[..., 3])[~same] - 136)[:, None]
        assert (np.abs(H.rgbe_decode(px)[~same].astype(np.float64) - H.rgbe_decode(rpx.astype(np.uint8))[~same]) <= step).all(), what


# (sdr size or None for a uint8 source, gain-map size, output size)
TAIL_CASES = [((8, 16), (8, 16), (37, 53)), ((20, 36), (20, 36), (67, 120)), ((9, 7), (9, 7), (5, 3)), (None, (16, 24), (37, 53))]


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_resized_tail_within_derived_bounds(layout, dtype):
    """B = 2; up-scale, larger up-scale over several blocks, down-scale to an odd size, and a uint8 source at 37 x 53 (odd pixel count;
    the first and last rows and columns clamp).  float outputs: per-element bounds of tests/resample_ref.py, zero violations."""
    o = ops()
    B = 2
    for n, (ss, gs, (H, W)) in enumerate(TAIL_CASES):
        g = torch.Generator().manual_seed(100 * n + 10 * layout + 1)
        gm_dec = _dec((B, 3) + gs, dtype, g)
        g_ref, e_gm = R.bilinear_ref_bound(gm_dec, H, W)
        if ss is None:
            src = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
            s_ref = src.to(torch.float64) / 255
            e_sdr = torch.full_like(s_ref, R.U_F32)  # float(u8) is exact; the division rounds once, values <= 1
            out = o.hdr_tail_resized(src.to(DEV), _lay(gm_dec, layout).to(DEV), layout, (H, W), gm_hw=gs, qmax=QMAX, source_u8=True, want=EIGHT)
        else:
            sdr_dec = _dec((B, 3) + ss, dtype, g)
            s_ref, e_sdr = R.bilinear_ref_bound(sdr_dec, H, W)
            out = o.hdr_tail_resized(_lay(sdr_dec, layout).to(DEV), _lay(gm_dec, layout).to(DEV), layout, (H, W), sdr_hw=ss, gm_hw=gs,
                                     qmax=QMAX, want=EIGHT)
        torch.cuda.synchronize()
        what = f"hdr_tail_resized sdr {ss} gm {gs} -> {(H, W)} layout {layout} {dtype}"
        assert set(out) == set(EIGHT) and all(v.shape == (B, H, W, 4 if k == "hdr_rgbe" else 3) for k, v in out.items())
        r1 = P.assert_elementwise(out["sdr"], s_ref, e_sdr, what + " sdr")
        r2 = P.assert_elementwise(out["gm"], g_ref, e_gm, what + " gm")
        hdr_ref = R.eq1_ref(s_ref, g_ref, QMAX)
        hb = R.hdr_bound(s_ref, g_ref, e_sdr, e_gm, QMAX)
        r3 = P.assert_elementwise(out["hdr"], hdr_ref, hb, what + " hdr")
        r4 = P.assert_elementwise(out["hdr_file"], hdr_ref / (QMAX + 1), hb / (QMAX + 1), what + " hdr_file")
        print(f"{what}: max |err| / bound  sdr {r1:.3f}  gm {r2:.3f}  hdr {r3:.3f}  hdr_file {r4:.3f}")
        _check_integer_outputs(out, {"sdr": s_ref, "gm": g_ref, "hdr_file": hdr_ref / (QMAX + 1)}, what)


def test_resized_tail_mixed_operand_sizes_and_clamp():
    """The two operands at sizes of their own (sdr 12 x 20 already at the output size: lambda = 0, the tap itself; gm 5 x 9 up-scaled),
    and the clamped Eq. 1 (flags bit 0) against the unclamped output clamped on the host."""
    o = ops()
    g = torch.Generator().manual_seed(77)
    B, (H, W) = 2, (12, 20)
    sdr_dec, gm_dec = _dec((B, 3, H, W), F32, g), _dec((B, 3, 5, 9), F32, g)
    out = o.hdr_tail_resized(sdr_dec.to(DEV), gm_dec.to(DEV), 0, (H, W), qmax=9.0, want=("sdr", "gm", "hdr"))
    assert torch.equal(out["sdr"].cpu(), (sdr_dec / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1))
    g_ref, e_gm = R.bilinear_ref_bound(gm_dec, H, W)
    P.assert_elementwise(out["gm"], g_ref, e_gm, "mixed sizes: gm")
    out_c = o.hdr_tail_resized(sdr_dec.to(DEV), gm_dec.to(DEV), 0, (H, W), qmax=9.0, clamp=True, want=("hdr",))
    assert torch.equal(out_c["hdr"], out["hdr"].clamp(0.0, 10.0))


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("size", [(20, 36), (37, 31)])
def test_resized_tail_identity_equals_hdr_tail_bit_for_bit(layout, dtype, size):
    """Operands already at the output size: every weight is 0 or 1 and all seven outputs equal gmd_hdr_tail's on the same inputs.
    20 x 36 in float32 layout 2 is 4-aligned: the existing tail takes its vec4 path there; 37 x 31 takes the generic kernel."""
    o = ops()
    B, (H, W) = 2, size
    g = torch.Generator().manual_seed(5 + layout)
    sdr, gm = _lay(_dec((B, 3, H, W), dtype, g), layout).to(DEV), _lay(_dec((B, 3, H, W), dtype, g), layout).to(DEV)
    for clamp in (False, True):
        want = o.hdr_tail(sdr, gm, layout, B, H, W, qmax=QMAX, clamp=clamp)
        got = o.hdr_tail_resized(sdr, gm, layout, (H, W), sdr_hw=(H, W), gm_hw=(H, W), qmax=QMAX, clamp=clamp, want=SEVEN)
        for k in SEVEN:
            assert torch.equal(got[k], want[k]), f"{k} layout {layout} {dtype} {size} clamp={clamp}"


PREP_CASES = [((37, 53), (8, 16)), ((135, 240), (64, 64)), ((100, 7), (9, 7)), ((16, 24), (16, 24)), ((16, 24), (37, 53))]


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_prepare_sdr_within_derived_bound(layout, dtype):
    """Down-scales (odd sizes, 135 x 240 -> 64 x 64 over several blocks, one axis unchanged), the identity (ToTensor + Normalize
    exactly) and an up-scale; B = 2; NCHW and the encoder's padded channels-last input (padding channels zero)."""
    o = ops()
    B, cp = 2, 8
    for n, ((h, w), (H, W)) in enumerate(PREP_CASES):
        u8 = torch.randint(0, 256, (B, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(31 + n))
        got = o.prepare_sdr(u8.to(DEV), (H, W), dtype, layout=layout, cp=cp)
        torch.cuda.synchronize()
        if layout == "nhwc":
            assert got.shape == (B, H * W, cp) and got.dtype == dtype
            assert not bool(got[:, :, 3:].any()), "padding channels must be zero"
            got = got[:, :, :3].reshape(B, H, W, 3).permute(0, 3, 1, 2)
        else:
            assert got.shape == (B, 3, H, W) and got.dtype == dtype
        ref, bound = R.prepare_ref_bound(u8, H, W, dtype)
        r = P.assert_elementwise(got, ref, bound, f"prepare_sdr {(h, w)} -> {(H, W)} {layout} {dtype}")
        print(f"prepare_sdr {(h, w)} -> {(H, W)} {layout} {dtype}: max |err| / bound {r:.3f}")
        if (h, w) == (H, W):
            exact = ((u8.to(F32) / 255.0 - 0.5) / 0.5).permute(0, 3, 1, 2).to(dtype)
            assert torch.equal(got.cpu(), exact), "equal sizes must be ToTensor + Normalize exactly"


# ---- write footprint (the style of tests/test_footprint_gpu.py: guard bands of the test's own memory, nothing provokes a fault) ----
GUARD = 65536


class Guarded:
    """``numel`` elements of ``dtype`` between two guard bands filled with the pattern (i * 131 + 89) mod 251."""

    def __init__(self, numel, dtype):
        self.nbytes = numel * torch.empty((), dtype=dtype).element_size()
        self.buf = ((torch.arange(2 * GUARD + self.nbytes, device=DEV, dtype=torch.int64) * 131 + 89) % 251).to(torch.uint8)
        self.before = self.buf.clone()
        self.t = self.buf[GUARD:GUARD + self.nbytes].view(dtype)

    def assert_guards_untouched(self, what):
        changed = self.buf != self.before
        assert not bool(changed[:GUARD].any()), f"{what}: {int(changed[:GUARD].sum())} bytes of the guard band BEFORE the output changed"
        assert not bool(changed[GUARD + self.nbytes:].any()), f"{what}: {int(changed[GUARD + self.nbytes:].sum())} bytes of the guard band AFTER the output changed"


def _poisoned(t):
    """A copy of ``t`` with NaN (float) or 255 (uint8) all round it: a read outside the logical tensor shows in the result."""
    n = GUARD // t.element_size()
    buf = torch.full((2 * n + t.numel(),), 255 if t.dtype == torch.uint8 else float("nan"), dtype=t.dtype, device=DEV)
    buf[n:n + t.numel()] = t.reshape(-1).to(DEV)
    return buf[n:n + t.numel()].view(t.shape)


@pytest.mark.parametrize("layout", [0, 2])
@pytest.mark.parametrize("source_u8", [False, True])
def test_resized_tail_stores_only_its_eight_outputs(layout, source_u8):
    """All eight outputs at 37 x 31 (1147 pixels per image) from 10 x 9 operands surrounded by NaN: a guarded launch equals a plain
    one and no byte outside the tensors changes."""
    from gm_diffusion._native import lib

    B, H, W, hs, ws = 2, 37, 31, 10, 9
    g = torch.Generator().manual_seed(6)
    gm = _poisoned(_lay(_dec((B, 3, hs, ws), F32, g), layout))
    if source_u8:
        sdr, shs, sws = _poisoned(torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)), H, W
    else:
        sdr, shs, sws = _poisoned(_lay(_dec((B, 3, hs, ws), F32, g), layout)), hs, ws
    n = B * H * W * 3
    kinds = [(n, F32), (n, F32), (n, torch.uint8), (n, torch.uint8), (n, F32), (n, F32), (n, torch.int16), (B * H * W * 4, torch.uint8)]

    def run(bufs):
        rc = lib().gmd_hdr_tail_resized(sdr.data_ptr(), shs, sws, gm.data_ptr(), hs, ws, 0, layout, B, H, W, 99.0, 1 / 64, 1 | (2 if source_u8 else 0),
                                        *[b.data_ptr() for b in bufs], torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib().gmd_last_error()
        torch.cuda.synchronize()

    plain = [torch.empty(k, dtype=d, device=DEV) for k, d in kinds]
    run(plain)
    gds = [Guarded(k, d) for k, d in kinds]
    run([gd.t for gd in gds])
    for i, (gd, pl) in enumerate(zip(gds, plain)):
        assert torch.equal(gd.t, pl), f"hdr_tail_resized output {i}: the guarded launch differs from the plain one"
        gd.assert_guards_untouched(f"hdr_tail_resized output {i} layout {layout} source_u8={source_u8}")
    assert all(bool(torch.isfinite(plain[i]).all()) for i in (0, 1, 4, 5)), "a tap was read outside the operands"


@pytest.mark.parametrize("layout,dtype", [(0, F32), (1, F32), (1, BF16), (0, F16)])
def test_prepare_sdr_stores_only_its_output(layout, dtype):
    """53 x 47 -> 37 x 31 (and the up-scale 9 x 10 -> 37 x 31): guarded output, source surrounded by 255s."""
    from gm_diffusion._native import lib

    B, H, W, cp = 2, 37, 31, 8
    o = ops()
    for h, w in ((53, 47), (9, 10)):
        src = _poisoned(torch.randint(0, 200, (B, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(h)))
        n = B * 3 * H * W if layout == 0 else B * H * W * cp
        plain = torch.empty(n, dtype=dtype, device=DEV)
        gd = Guarded(n, dtype)
        for buf in (plain, gd.t):
            rc = lib().gmd_prepare_sdr(src.data_ptr(), B, h, w, buf.data_ptr(), o.dtype_code(dtype), layout, cp, H, W, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib().gmd_last_error()
        torch.cuda.synchronize()
        assert torch.equal(gd.t, plain), "the guarded launch differs from the plain one"
        gd.assert_guards_untouched(f"prepare_sdr {(h, w)} layout {layout} {dtype}")
        assert float(plain.float().max()) <= (199 / 255 - 0.5) / 0.5 + 1e-2, "a source byte was read outside the picture"


def test_front_ends_report_to_the_kernel_timer():
    from gm_diffusion import profiling

    o = ops()
    g = torch.Generator().manual_seed(2)
    dec = _dec((1, 3, 8, 8), F32, g).to(DEV)
    u8 = torch.randint(0, 256, (1, 20, 20, 3), dtype=torch.uint8, generator=g).to(DEV)
    tm = profiling.KernelTimer()
    profiling.set_timer(tm)
    try:
        out = o.hdr_tail_resized(dec, dec, 0, (16, 16), want=("hdr", "hdr_rgbe"))
        x = o.prepare_sdr(u8, (8, 8))
    finally:
        profiling.set_timer(None)
    torch.cuda.synchronize()
    s = tm.summary()
    assert s["hdr_tail_resized"]["launches"] == 1 and s["prepare_sdr"]["launches"] == 1
    assert s["hdr_tail_resized"]["bytes"] == 2 * 3 * 64 * 4 + out["hdr"].numel() * 4 + out["hdr_rgbe"].numel()
    assert s["prepare_sdr"]["bytes"] == u8.numel() + x.numel() * 4


# ---- end to end ----
def _tiny_gm_pipe():
    from gm_diffusion.components import AutoencoderKL, PNDMScheduler, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionGMPipeline
    from oracle import fixtures

    def hip(cls, om):
        m = cls(**vars(om.config))
        m.load_state_dict(om.state_dict())
        return m.to(DEV, F32)

    pipe = StableDiffusionGMPipeline(
        vae=hip(AutoencoderKL, fixtures.build_vae("tiny", with_encoder=True)), text_encoder=None, tokenizer=None,
        unet=hip(UNet2DConditionModel, fixtures.build_unet("tiny", 8)),
        scheduler=PNDMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", skip_prk_steps=True, steps_offset=1,
                                set_alpha_to_one=False),
        safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    return pipe


def test_sdr_to_hdr_end_to_end(tmp_path):
    """72 x 104 uint8 sources through a 32 x 48 model: hdr, original_hdr and hdr_rgbe come back at 72 x 104 and equal the same steps
    composed by hand; decode_to_hdr without the new arguments still is gmd_hdr_tail on the decodes; the written .hdr decodes to
    hdr_file within one RGBE code step."""
    from gm_diffusion import hdr
    from oracle import fixtures, hdr_ops as H

    o = ops()
    pipe = _tiny_gm_pipe()
    B, (h, w), (mh, mw) = 2, (72, 104), (32, 48)
    pe, ne, _ = fixtures.make_inputs(B, mh // 8, mw // 8, cross_dim=64)
    kw = dict(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), guidance_scale=7.5)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    base = torch.stack([(yy * 3 + xx) % 256, (yy + 2 * xx) % 256, (5 * yy + xx) % 256], -1)
    src = torch.stack([base, (base * 7 + 13) % 256], 0).to(torch.uint8).to(DEV)

    out = hdr.sdr_to_hdr(pipe, src, (mh, mw), num_inference_steps=3, generator=torch.Generator(device=DEV).manual_seed(42), qmax=99,
                         original=True, want=("hdr", "hdr_file", "hdr_rgbe"), **kw)
    assert out["hdr"].shape == out["original_hdr"].shape == (B, h, w, 3) and out["hdr_rgbe"].shape == (B, h, w, 4)
    assert bool(torch.isfinite(out["hdr"]).all()) and float(out["hdr"].max()) > 0

    # the same steps by hand
    gen = torch.Generator(device=DEV).manual_seed(42)
    x = hdr.prepare_sdr(src, (mh, mw), F32)
    assert x.shape == (B, 3, mh, mw)
    sdr_latent = pipe.vae.encode(x).latent_dist.sample(gen) * pipe.vae.config.scaling_factor
    gm_latent = pipe(sdr_latent, num_inference_steps=3, generator=gen, output_type="latent", **kw).images
    assert torch.equal(sdr_latent, out["sdr_latent"]) and torch.equal(gm_latent, out["gm_latent"])
    hand = hdr.decode_to_hdr(pipe.vae, sdr_latent, gm_latent, qmax=99, out_size=(h, w), want=("hdr", "hdr_file", "hdr_rgbe"))
    for k in ("hdr", "hdr_file", "hdr_rgbe"):
        assert torch.equal(hand[k], out[k]), k
    org = hdr.decode_to_hdr(pipe.vae, None, gm_latent, qmax=99, source_u8=src, want=("hdr", "sdr"))
    assert torch.equal(org["hdr"], out["original_hdr"])
    assert torch.equal(org["sdr"].cpu(), src.cpu().to(F32) / 255.0)

    # without the new arguments: today's path, gmd_hdr_tail on the two decodes at the decoder's size
    dec, Hd, Wd = pipe.vae.decode_nhwc(o.tmo(torch.cat([sdr_latent, gm_latent], 0), 5, mu=1.0 / pipe.vae.config.scaling_factor))
    assert (Hd, Wd) == (mh, mw)
    old = hdr.decode_to_hdr(pipe.vae, sdr_latent, gm_latent, qmax=99)
    direct = o.hdr_tail(dec[:B], dec[B:], 2, B, Hd, Wd, qmax=99.0)
    assert set(old) == set(direct) == set(SEVEN)
    for k in SEVEN:
        assert torch.equal(old[k], direct[k]), k
    with pytest.raises(ValueError):
        hdr.decode_to_hdr(pipe.vae, sdr_latent, gm_latent, want=("hdr", "hdr_rgbe"))  # the key exists only with out_size / source_u8

    # the file
    path = os.path.join(tmp_path, "full.hdr")
    hdr.save_hdr_image(out["hdr_rgbe"][1], path)
    raw = open(path, "rb").read()
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {h} +X {w}\n".encode()
    assert raw.startswith(head)
    px = H.rgbe_rle_decode(raw[len(head):], h, w)
    assert np.array_equal(px, out["hdr_rgbe"][1].cpu().numpy())
    val, hf = H.rgbe_decode(px).astype(np.float64), out["hdr_file"][1].cpu().numpy().astype(np.float64)
    step = np.ldexp(1.0, px[..., 3].astype(np.int32) - 136)[..., None]  # one code of the pixel's shared exponent: 2^e / 256
    assert (np.abs(val - np.maximum(hf, 0)) <= step).all()
    # the float path of the writer gives the same file
    path2 = os.path.join(tmp_path, "full_float.hdr")
    hdr.save_hdr_image(out["hdr_file"][1], path2)
    assert open(path2, "rb").read() == raw
