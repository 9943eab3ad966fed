"""GPU: the small kernels (latent step, pack / unpack, elementwise, HDR tail, row softmax) where the suite did not look so far.

A. The SECOND LAP of every grid-stride loop: launches larger than ``cap * 256`` (tests/small_ref.py LAP_*), compared bit for bit with the
   torch expressions the existing tests of these kernels use -- each lap test asserts ``n > lap`` itself.
B. Per-element bounds (tests/small_ref.py, allowed violations: 0) and bit-exact checks at edge shapes and edge values.

Every launch goes through the raw C ABI into buffers of the test's own: outputs pre-filled with NaN (float) or 0xFF (integer), so an
element that is never written shows; operand padding the kernel must not read is NaN."""

import numpy as np
import pytest
import torch

import parity as P
import resample_ref as R
import small_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]


def ops():
    from gm_diffusion import hip_ops

    return hip_ops


def call(name, *args):
    from gm_diffusion._native import lib

    rc = getattr(lib(), name)(*args, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (name, rc, lib().gmd_last_error())


def ptr(t):
    return None if t is None else t.data_ptr()


def prefilled(shape, dtype):
    """A device output buffer nobody has written: NaN (float) or 0xFF bytes (integer)."""
    if dtype.is_floating_point:
        return torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(255)
    return t


def code(dtype):
    return ops().dtype_code(dtype)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# =============================================================================================================================
# A. the second lap, bit for bit
# =============================================================================================================================
LAT_B, LAT_SHAPE = 2, (4, 257, 257)
LAT_CHW = 4 * 257 * 257
GS, GR = 7.5, 0.7


def _latent_inputs(do_cfg, seed):
    g = gen(seed)
    eps_in = torch.randn((2 * LAT_B if do_cfg else LAT_B,) + LAT_SHAPE, generator=g)
    rest = [torch.randn((LAT_B,) + LAT_SHAPE, generator=g) for _ in range(6)]
    ratio = torch.tensor([0.25, 3.0])  # two very different entries: the lap boundary falls inside sample 1
    return eps_in, rest, ratio


@pytest.mark.parametrize("do_cfg", [False, True])
def test_latent_step_second_lap(do_cfg):
    n = LAT_B * LAT_CHW
    assert n > S.LAP_LATENT and LAT_CHW < S.LAP_LATENT < n, "not a two-lap launch with the lap boundary inside sample 1"
    eps_in, (x, cur, e1, e2, e3, _), ratio = _latent_inputs(do_cfg, 21)
    eps = S.guided_eps(eps_in, LAT_B, do_cfg, GS, ratio, GR)
    d = [t.to(DEV) for t in (eps_in, x, cur, e1, e2, e3, ratio)]
    coefs = (1.01, 0.02, 0.97, 0.8, 0.6)
    for mode in range(5):
        hist = (e1, e2, e3)[: (0, 1, 1, 2, 3)[mode]]
        xp_ref, x0_ref = S.latent_step_ref(eps, x, mode, coefs, cur=cur, hist=hist)
        oe, op, o0 = (prefilled((LAT_B,) + LAT_SHAPE, F32) for _ in range(3))
        h = [ptr(t) for t in d[3:3 + len(hist)]] + [None] * (3 - len(hist))
        call("gmd_latent_step", ptr(d[0]), ptr(d[1]), ptr(d[2]), h[0], h[1], h[2], LAT_B, LAT_CHW, int(do_cfg), GS, ptr(d[6]), GR, mode, *coefs,
             ptr(oe), ptr(op), ptr(o0))
        torch.cuda.synchronize()
        what = f"latent_step mode {mode} do_cfg={do_cfg}"
        S.assert_bit_equal(oe, eps, what + " eps_out")
        S.assert_bit_equal(o0, x0_ref, what + " x0")
        S.assert_bit_equal(op, xp_ref, what + " x_prev")


@pytest.mark.parametrize("do_cfg", [False, True])
def test_dpm_step_second_lap(do_cfg):
    n = LAT_B * LAT_CHW
    assert n > S.LAP_LATENT
    eps_in, (x, m1, *_), ratio = _latent_inputs(do_cfg, 22)
    eps = S.guided_eps(eps_in, LAT_B, do_cfg, GS, ratio, GR)
    d_eps, d_x, d_m1, d_ratio = (t.to(DEV) for t in (eps_in, x, m1, ratio))
    coefs = (0.5, 0.85, 0.9, -0.12, -0.06, 1.3, 0.8, 0.6)
    for order in (1, 2):
        m0_ref, xp_ref, x0_ref = S.dpm_step_ref(eps, x, order, coefs, m1=m1)
        om, op, o0 = (prefilled((LAT_B,) + LAT_SHAPE, F32) for _ in range(3))
        call("gmd_dpm_step", ptr(d_eps), ptr(d_x), ptr(d_m1), LAT_B, LAT_CHW, int(do_cfg), GS, ptr(d_ratio), GR, order, *coefs, ptr(om), ptr(op), ptr(o0))
        torch.cuda.synchronize()
        what = f"dpm_step order {order} do_cfg={do_cfg}"
        S.assert_bit_equal(om, m0_ref, what + " m0")
        S.assert_bit_equal(o0, x0_ref, what + " x0")
        S.assert_bit_equal(op, xp_ref, what + " x_prev")


@pytest.mark.parametrize("do_cfg", [False, True])
def test_ddpm_step_second_lap(do_cfg):
    n = LAT_B * LAT_CHW
    assert n > S.LAP_LATENT
    eps_in, (x, noise, *_), ratio = _latent_inputs(do_cfg, 23)
    eps = S.guided_eps(eps_in, LAT_B, do_cfg, GS, ratio, GR)
    d_eps, d_x, d_noise, d_ratio = (t.to(DEV) for t in (eps_in, x, noise, ratio))
    sa, s1, c0, ct, ns, pa, p1 = coefs = (0.9, 0.43, 0.3, 0.69, 0.1, 0.8, 0.6)
    for clip in (None, 1.0):
        for nz in (noise, None):
            xp_ref, x0_ref = S.ddpm_step_ref(eps, x, coefs, noise=nz, clip_range=clip)
            op, o0 = prefilled((LAT_B,) + LAT_SHAPE, F32), prefilled((LAT_B,) + LAT_SHAPE, F32)
            call("gmd_ddpm_step", ptr(d_eps), ptr(d_x), None if nz is None else ptr(d_noise), LAT_B, LAT_CHW, int(do_cfg), GS, ptr(d_ratio), GR, sa, s1,
                 int(clip is not None), float(clip or 0.0), c0, ct, ns, pa, p1, ptr(op), ptr(o0))
            torch.cuda.synchronize()
            what = f"ddpm_step clip={clip} noise={nz is not None} do_cfg={do_cfg}"
            S.assert_bit_equal(o0, x0_ref, what + " x0")
            S.assert_bit_equal(op, xp_ref, what + " x_prev")


def _pack_case(B, C0, C1, HW, CP, dup, dtype, seed):
    g = gen(seed)
    s0 = torch.randn(B, C0, HW, 1, generator=g)
    s1 = torch.randn(B, C1, HW, 1, generator=g) if C1 else None
    out = prefilled((dup * B, HW, CP), dtype)
    d0, d1 = s0.to(DEV), None if s1 is None else s1.to(DEV)
    call("gmd_pack_unet_input", ptr(d0), C0, ptr(d1), C1, B, HW, dup, ptr(out), CP, code(dtype))
    torch.cuda.synchronize()
    what = f"pack_unet_input B={B} C0={C0} C1={C1} HW={HW} CP={CP} dup={dup} {dtype}"
    S.assert_bit_equal(out, S.pack_ref(s0, s1, dup, CP, dtype), what)
    o = out.cpu()
    assert not bool(o[:, :, C0 + C1:].float().abs().ne(0).any()), what + ": padding channels must be exactly zero"
    if dup == 2:
        assert torch.equal(o[:B].view(torch.int16 if dtype != F32 else torch.int32), o[B:].view(torch.int16 if dtype != F32 else torch.int32)), what + ": the two duplicates differ"


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_pack_unet_input_second_lap(dtype):
    B, HW, CP = 3, 135 * 240, 64
    assert B * HW * (CP // 8) > S.LAP_LATENT  # one thread per (pixel, 8-channel group)
    _pack_case(B, 4, 4, HW, CP, 2, dtype, 31)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_unet_input_small_shapes(dtype):
    for n, (B, C0, C1, CP, dup) in enumerate([(3, 4, 4, 8, 2), (2, 4, 4, 16, 1), (2, 4, 0, 8, 1), (1, 4, 0, 16, 2), (3, 3, 2, 8, 2), (2, 4, 4, 16, 2)]):
        _pack_case(B, C0, C1, 37, CP, dup, dtype, 40 + n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_unpack_nchw_second_lap(dtype):
    B, C, HW, ld = 3, 4, 257 * 257, 64
    assert B * C * HW > S.LAP_LATENT and HW % 256 != 0
    x = torch.full((B, HW, ld), float("nan"), dtype=dtype)
    x[:, :, :C] = torch.randn(B, HW, C, generator=gen(5)).to(dtype)
    out = prefilled((B, C, HW), F32)
    dx = x.to(DEV)
    call("gmd_unpack_nchw", ptr(dx), code(dtype), ld, B, C, HW, ptr(out))
    torch.cuda.synchronize()
    S.assert_bit_equal(out, S.unpack_ref(x, C), f"unpack_nchw {dtype}")


def test_dup_batch_second_lap():
    nvec = (1 << 20) + 257
    assert nvec > S.LAP_ELEMENTWISE
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (nvec * 4,), dtype=torch.int32, generator=gen(6))
    out = prefilled((2, nvec * 4), torch.int32)
    d = src.to(DEV)
    call("gmd_dup_batch", ptr(d), ptr(out), 16 * nvec)
    torch.cuda.synchronize()
    S.assert_bit_equal(out, torch.stack([src, src]), "dup_batch")


def test_concat_channels_second_lap():
    rows, Ca, Cb = 8200, 640, 640
    assert rows * (Ca + Cb) // 8 > S.LAP_ELEMENTWISE
    g = gen(7)
    a, b = torch.randn(rows, Ca, generator=g).to(BF16), torch.randn(rows, Cb, generator=g).to(BF16)
    out = prefilled((rows, Ca + Cb), BF16)
    da, db = a.to(DEV), b.to(DEV)
    call("gmd_concat_channels", ptr(da), Ca, ptr(db), Cb, ptr(out), code(BF16), rows)
    torch.cuda.synchronize()
    S.assert_bit_equal(out, torch.cat([a, b], -1), "concat_channels")


def _embedding_case(B, T, C, vocab, dtype, seed):
    g = gen(seed)
    ids = torch.randint(0, vocab, (B, T), generator=g, dtype=torch.int32)
    ids.view(-1)[0], ids.view(-1)[-1] = 0, vocab - 1
    ids.view(-1)[(B * T) // 2] = vocab - 1
    table, pos = torch.randn(vocab, C, generator=g).to(dtype), torch.randn(T, C, generator=g).to(dtype)
    out = prefilled((B, T, C), dtype)
    di, dt, dp = ids.to(DEV), table.to(DEV), pos.to(DEV)
    call("gmd_embedding_lookup", ptr(di), ptr(dt), ptr(dp), ptr(out), code(dtype), B * T, T, C, vocab)
    torch.cuda.synchronize()
    ref = (table.float()[ids.long()] + pos.float()[None]).to(dtype)  # one float32 add, one rounding
    S.assert_bit_equal(out, ref, f"embedding_lookup B={B} T={T} C={C} {dtype}")


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_embedding_lookup_second_lap_and_small(dtype):
    assert 20 * 77 * 768 > S.LAP_ELEMENTWISE
    _embedding_case(20, 77, 768, 1000, dtype, 8)
    _embedding_case(3, 77, 8, 50, dtype, 9)
    _embedding_case(1, 77, 768, 1000, dtype, 10)
    _embedding_case(1, 5, 8, 2, dtype, 11)


N_EW = (1 << 20) + 257


def test_tmo_kinds_second_lap():
    from oracle import hdr_ops as H

    assert N_EW > S.LAP_ELEMENTWISE
    q, mu = 9.0, 500.0
    x = torch.rand(N_EW, generator=gen(12)) * 12 - 1
    xp = x.abs()  # the logarithmic operators are defined for non-negative inputs
    xn, xpn = x.numpy(), xp.numpy()
    dx, dxp = x.to(DEV), xp.to(DEV)
    sf = 0.18215
    refs = {0: (H.linear_scale_tmo(xn, q), 0.0, q, mu), 1: (H.hard_clip_tmo(xn), 0.0, q, mu), 2: (H.mulog_tmo(xpn, q, mu), 2.4e-7, q, mu),
            3: (H.tmo_cuda(xpn), 2.4e-7, q, mu), 4: (H.denorm_clamp(xn), 0.0, q, mu), 5: (xn * np.float32(sf), 0.0, 0.0, sf), 6: (xn / np.float32(sf), 0.0, 0.0, sf)}
    for kind, (ref, allow, qq, mm) in refs.items():
        out = prefilled((N_EW,), F32)
        call("gmd_tmo", ptr(dxp if kind in (2, 3) else dx), ptr(out), N_EW, kind, qq, mm)
        torch.cuda.synchronize()
        ref = torch.from_numpy(np.asarray(ref, np.float32))
        if allow == 0.0:
            S.assert_bit_equal(out, ref, f"tmo kind {kind}")
        else:
            r = P.assert_elementwise(out, ref.double(), torch.full((N_EW,), allow, dtype=torch.float64), f"tmo kind {kind}")
            print(f"tmo kind {kind}: max |err| / allowance {r:.3f}")


def test_apply_gm_and_quantisers_second_lap():
    """apply_gm_to_sdr against the oracle within ITS existing allowance (4e-6 (q + 1), test_hdr_ops_against_reference_golden), per element;
    the quantisers and the RGBE encoder bit for bit."""
    from oracle import hdr_ops as H

    assert N_EW > S.LAP_ELEMENTWISE
    g = gen(13)
    gm, sdr = torch.rand(N_EW, generator=g) * 1.2 - 0.1, torch.rand(N_EW, generator=g) * 1.2 - 0.1
    dg, ds = gm.to(DEV), sdr.to(DEV)
    for q, clamp in ((9.0, True), (99.0, False)):
        out = prefilled((N_EW,), F32)
        call("gmd_apply_gm_to_sdr", ptr(dg), ptr(ds), ptr(out), N_EW, q, 1 / 64, int(clamp))
        torch.cuda.synchronize()
        ref = torch.from_numpy(H.apply_gm_to_sdr(gm.numpy(), sdr.numpy(), qmax=q, clamp=clamp)).double()
        r = P.assert_elementwise(out, ref, torch.full((N_EW,), 4e-6 * (q + 1), dtype=torch.float64), f"apply_gm_to_sdr q={q}")
        print(f"apply_gm_to_sdr q={q}: max |err| / allowance {r:.3f}")
    x = torch.rand(N_EW, generator=g) * 1.1 - 0.05
    dx = x.to(DEV)
    of, oc = prefilled((N_EW,), F32), prefilled((N_EW,), torch.int16)
    call("gmd_discretize_u16", ptr(dx), ptr(of), ptr(oc), N_EW)
    torch.cuda.synchronize()
    S.assert_bit_equal(oc, torch.from_numpy(H.quantize_u16_codes(x.numpy()).view(np.int16)), "discretize_u16 codes")
    S.assert_bit_equal(of, torch.from_numpy(H.discretize_to_uint16(x.numpy())), "discretize_u16 float")
    x01 = x.clamp(0, 1)
    d01 = x01.to(DEV)
    o8 = prefilled((N_EW,), torch.uint8)
    call("gmd_quantize_u8", ptr(d01), ptr(o8), N_EW)
    torch.cuda.synchronize()
    S.assert_bit_equal(o8, torch.from_numpy(H.quantize_u8_trunc(x01.numpy())), "quantize_u8")
    rgb = torch.rand(N_EW, 3, generator=g) * 30 - 0.2
    drgb = rgb.to(DEV)
    ope = prefilled((N_EW, 4), torch.uint8)
    call("gmd_rgbe_encode", ptr(drgb), ptr(ope), N_EW)
    torch.cuda.synchronize()
    S.assert_bit_equal(ope, torch.from_numpy(H.rgbe_encode(rgb.numpy())), "rgbe_encode")


def test_gamut_and_stage1_chain_second_lap():
    from oracle import hdr_ops as H

    B, HW = 3, 350003
    assert B * HW > S.LAP_ELEMENTWISE and HW < S.LAP_ELEMENTWISE
    g = gen(14)
    sdr, gm = torch.rand(B, 3, HW, 1, generator=g) * 1.2 - 0.1, torch.rand(B, 3, HW, 1, generator=g) * 1.2 - 0.1
    ds, dg = sdr.to(DEV), gm.to(DEV)
    out = prefilled((B, 3, HW, 1), F32)
    call("gmd_gamut_compress", ptr(ds), ptr(out), B, HW)
    torch.cuda.synchronize()
    n = sdr.numel()
    r = P.assert_elementwise(out, torch.from_numpy(H.gamut_compress(sdr.numpy())).double(), torch.full(sdr.shape, 2.4e-7, dtype=torch.float64), "gamut_compress")
    print(f"gamut_compress: max |err| / allowance {r:.3f}")
    out = prefilled((B, 3, HW, 1), F32)
    call("gmd_stage1_chain", ptr(dg), ptr(ds), ptr(out), B, HW, 49.0)
    torch.cuda.synchronize()
    r = P.assert_elementwise(out, torch.from_numpy(H.stage1_chain(gm.numpy(), sdr.numpy(), 49)).double(), torch.full(sdr.shape, 1e-6, dtype=torch.float64), "stage1_chain")
    print(f"stage1_chain: max |err| / allowance {r:.3f}")
    assert n == B * 3 * HW


def _tail(sdr, gm, layout, B, H, W, names, dtype_code=0, q=99.0):
    kinds = {"sdr": F32, "gm": F32, "sdr_u8": torch.uint8, "gm_u8": torch.uint8, "hdr": F32, "hdr_file": F32, "hdr_u16": torch.int16}
    out = {k: prefilled((B, H, W, 3), kinds[k]) for k in names}
    call("gmd_hdr_tail", ptr(sdr), ptr(gm), dtype_code, layout, B, H, W, q, 1 / 64, 0, *[ptr(out.get(k)) for k in kinds])
    torch.cuda.synchronize()
    return out


THREE = ("sdr_u8", "hdr_file", "hdr_u16")


def test_hdr_tail_generic_second_lap_vs_oracle():
    from oracle import hdr_ops as H

    B, Hh, W = 1, 1025, 1024
    assert B * Hh * W > S.LAP_ELEMENTWISE
    g = gen(15)
    s3, g3 = torch.rand(B, Hh * W, 3, generator=g) * 2.6 - 1.3, torch.rand(B, Hh * W, 3, generator=g) * 2.6 - 1.3
    out = _tail(s3.to(DEV), g3.to(DEV), 1, B, Hh, W, THREE)
    sdr, gm = H.denorm_clamp(s3.numpy()).reshape(B, Hh, W, 3), H.denorm_clamp(g3.numpy()).reshape(B, Hh, W, 3)
    S.assert_bit_equal(out["sdr_u8"], torch.from_numpy(H.quantize_u8_trunc(sdr)), "hdr_tail generic sdr_u8")
    hf = out["hdr_file"].cpu()
    S.assert_bit_equal(out["hdr_u16"], torch.from_numpy(H.quantize_u16_codes(hf.numpy()).view(np.int16)), "hdr_tail generic hdr_u16 of its own hdr_file")
    s64, g64 = torch.from_numpy(sdr).double(), torch.from_numpy(gm).double()
    zero = torch.zeros_like(s64)
    ref, b = R.eq1_ref(s64, g64, 99.0) / 100.0, R.hdr_bound(s64, g64, zero, zero, 99.0) / 100.0
    r = P.assert_elementwise(hf, ref, b, "hdr_tail generic hdr_file")
    print(f"hdr_tail generic two laps: hdr_file max |err| / bound {r:.3f}")


def test_hdr_tail_vec4_second_lap_equals_generic():
    B, Hh, W = 2, 1025, 2048
    assert B * Hh * W // 4 > S.LAP_ELEMENTWISE and (B * Hh * W) % 4 == 0
    g = gen(16)
    s3 = (torch.rand(B, Hh * W, 3, generator=g) * 2.6 - 1.3).to(DEV)
    g3 = (torch.rand(B, Hh * W, 3, generator=g) * 2.6 - 1.3).to(DEV)
    pad = lambda x: torch.cat([x, torch.full_like(x[..., :1], float("nan"))], -1).contiguous()  # the fourth channel must not be used
    s4, g4 = pad(s3), pad(g3)
    assert s4.data_ptr() % 16 == 0 and g4.data_ptr() % 16 == 0
    fast = _tail(s4, g4, 2, B, Hh, W, THREE)
    del s4, g4
    slow = _tail(s3, g3, 1, B, Hh, W, THREE)
    for k in THREE:
        assert bool(torch.isfinite(slow["hdr_file"]).all())
        S.assert_bit_equal(fast[k], slow[k], f"hdr_tail vec4 vs generic {k}")


def test_hdr_tail_resized_second_lap():
    from test_resample_gpu import EIGHT, _check_integer_outputs

    B, (hs, ws), (H, W) = 1, (20, 36), (1100, 2000)
    assert B * H * W > S.LAP_RESAMPLE
    g = gen(17)
    sdr_dec, gm_dec = torch.rand(B, 3, hs, ws, generator=g) * 2.4 - 1.2, torch.rand(B, 3, hs, ws, generator=g) * 2.4 - 1.2
    kinds = {"sdr": F32, "gm": F32, "sdr_u8": torch.uint8, "gm_u8": torch.uint8, "hdr": F32, "hdr_file": F32, "hdr_u16": torch.uint16, "hdr_rgbe": torch.uint8}
    assert tuple(kinds) == EIGHT
    out = {k: prefilled((B, H, W, 4 if k == "hdr_rgbe" else 3), kinds[k]) for k in kinds}
    ds, dg = sdr_dec.to(DEV), gm_dec.to(DEV)
    call("gmd_hdr_tail_resized", ptr(ds), hs, ws, ptr(dg), hs, ws, 0, 0, B, H, W, 99.0, 1 / 64, 0, *[ptr(out[k]) for k in kinds])
    torch.cuda.synchronize()
    s_ref, e_sdr = R.bilinear_ref_bound(sdr_dec, H, W)
    g_ref, e_gm = R.bilinear_ref_bound(gm_dec, H, W)
    what = "hdr_tail_resized 20x36 -> 1100x2000"
    r1 = P.assert_elementwise(out["sdr"], s_ref, e_sdr, what + " sdr")
    r2 = P.assert_elementwise(out["gm"], g_ref, e_gm, what + " gm")
    hdr_ref = R.eq1_ref(s_ref, g_ref, 99.0)
    hb = R.hdr_bound(s_ref, g_ref, e_sdr, e_gm, 99.0)
    r3 = P.assert_elementwise(out["hdr"], hdr_ref, hb, what + " hdr")
    r4 = P.assert_elementwise(out["hdr_file"], hdr_ref / 100.0, hb / 100.0, what + " hdr_file")
    print(f"{what}: max |err| / bound  sdr {r1:.3f}  gm {r2:.3f}  hdr {r3:.3f}  hdr_file {r4:.3f}")
    _check_integer_outputs(out, {"sdr": s_ref, "gm": g_ref, "hdr_file": hdr_ref / 100.0}, what)


@pytest.mark.parametrize("src,size,lap", [((2900, 2900), (1450, 1450), True), ((2160, 3840), (288, 512), False)])
def test_prepare_sdr_second_lap_and_product_ratio(src, size, lap):
    """2.1 M output pixels (two laps), and the product's own ratio 2160 x 3840 -> 288 x 512 (7.5x: 15 x 15 non-zero taps)."""
    (h, w), (H, W) = src, size
    if lap:
        assert H * W > S.LAP_RESAMPLE
    u8 = torch.randint(0, 256, (1, h, w, 3), dtype=torch.uint8, generator=gen(h))
    out = prefilled((1, 3, H, W), F32)
    d = u8.to(DEV)
    call("gmd_prepare_sdr", ptr(d), 1, h, w, ptr(out), 0, 0, 8, H, W)
    torch.cuda.synchronize()
    ref, bound = R.prepare_ref_bound(u8, H, W, F32)
    r = P.assert_elementwise(out, ref, bound, f"prepare_sdr {src} -> {size}")
    print(f"prepare_sdr {src} -> {size}: max |err| / bound {r:.3f}")


# =============================================================================================================================
# B. per-element bounds at edge shapes and values
# =============================================================================================================================
@pytest.mark.parametrize("out_dtype", DTYPES)
@pytest.mark.parametrize("in_dtype", DTYPES)
def test_cast_every_pair_bit_equal(in_dtype, out_dtype):
    sizes = [1, 255, 256, 257, 1001, (1 << 20) + 257]
    assert sizes[-1] > S.LAP_ELEMENTWISE
    for n in sizes:
        x = S.cast_input(n, in_dtype)
        out = prefilled((n,), out_dtype)
        dx = x.to(DEV)
        call("gmd_cast", ptr(dx), code(in_dtype), ptr(out), code(out_dtype), n)
        torch.cuda.synchronize()
        S.assert_bit_equal(out, x.to(out_dtype), f"cast {in_dtype} -> {out_dtype} n={n}")


def _geglu_case(rows, Fh, dtype, seed):
    g = gen(seed)
    x = torch.randn(rows, 2 * Fh, generator=g) * 2
    sat = torch.tensor([10.0, -10.0, 40.0, -40.0])  # erf saturates
    x[0, Fh:Fh + 4] = sat
    x[-1, -4:] = sat.flip(0)
    x = x.to(dtype)
    out = prefilled((rows, Fh), dtype)
    dx = x.to(DEV)
    call("gmd_geglu", ptr(dx), ptr(out), code(dtype), rows, Fh)
    torch.cuda.synchronize()
    ref, bound, c = S.geglu_ref_bound(x, dtype)
    r = P.assert_elementwise(out, ref, bound, f"geglu rows={rows} F={Fh} {dtype}")
    return r, c


@pytest.mark.parametrize("dtype", DTYPES)
def test_geglu_within_measured_bound(dtype):
    worst, cs = 0.0, []
    for n, (rows, Fh) in enumerate([(1, 8), (37, 8), (1, 1280), (37, 1280)]):
        r, c = _geglu_case(rows, Fh, dtype, 50 + n)
        worst = max(worst, r)
        cs.append(c)
    print(f"geglu {dtype}: max |err| / bound {worst:.3f}; measured constants c = {['%.3f' % c for c in cs]}")


def test_geglu_second_lap_float32():
    rows, Fh = 3300, 1280
    assert rows * Fh // 4 > S.LAP_ELEMENTWISE
    r, c = _geglu_case(rows, Fh, F32, 60)
    print(f"geglu two laps float32: max |err| / bound {r:.3f}; measured constant c = {c:.3f}")


SOFTMAX_COLS = [1, 5, 63, 64, 65, 255, 256, 257, 1000, 4099]


@pytest.mark.parametrize("dtype", DTYPES)
def test_softmax_rows_within_derived_bound(dtype):
    worst = 0.0
    for cols in SOFTMAX_COLS:
        lds, ldp = cols + 5, (cols + 7) // 8 * 8 + 8
        for kind, scale in ((0, 0.3), (1, 0.3), (2, 0.5)):
            rows = 9
            s = S.softmax_rows_input(kind, rows, cols, lds, 100 * cols + kind)
            out = prefilled((rows, ldp), dtype)
            ds = s.to(DEV)
            call("gmd_softmax_rows", ptr(ds), lds, ptr(out), code(dtype), ldp, rows, cols, scale, 0)
            torch.cuda.synchronize()
            ref, bound = S.softmax_ref_bound(s, cols, scale, dtype, ldp)
            what = f"softmax_rows cols={cols} kind={kind} {dtype}"
            worst = max(worst, P.assert_elementwise(out, ref, bound, what))
            assert not bool(out[:, cols:].float().ne(0).any()), what + ": the tail must be exactly zero"
    print(f"softmax_rows {dtype}: max |err| / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_softmax_rows_causal_within_derived_bound(dtype):
    worst = 0.0
    for cols in (5, 77, 257):
        rows, lds, ldp = 2 * cols, cols + 5, (cols + 7) // 8 * 8 + 8
        s = S.softmax_rows_input(0, rows, cols, lds, 7000 + cols)
        out = prefilled((rows, ldp), dtype)
        ds = s.to(DEV)
        call("gmd_softmax_rows", ptr(ds), lds, ptr(out), code(dtype), ldp, rows, cols, 0.3, cols)
        torch.cuda.synchronize()
        ref, bound = S.softmax_ref_bound(s, cols, 0.3, dtype, ldp, causal_nq=cols)
        worst = max(worst, P.assert_elementwise(out, ref, bound, f"softmax_rows causal cols={cols} {dtype}"))
    print(f"softmax_rows causal {dtype}: max |err| / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_timestep_embedding_within_derived_bound(dtype):
    worst = 0.0
    for dim in (2, 256, 320, 1280):
        for B in (1, 3, 16):
            for flip in (0, 1):
                for shift in (0, 1):
                    if dim == 2 and shift == 1:
                        continue  # half - shift = 0
                    for t in (0.0, 1.0, 20.5, 501.0, 981.0, 999.0):
                        td = torch.tensor([t], device=DEV)
                        out = prefilled((B, dim), dtype)
                        call("gmd_timestep_embedding", ptr(td), ptr(out), code(dtype), B, dim, flip, float(shift))
                        ref, bound = S.temb_ref_bound(t, B, dim, flip, shift, dtype)
                        worst = max(worst, P.assert_elementwise(out, ref, bound, f"timestep_embedding dim={dim} B={B} flip={flip} shift={shift} t={t} {dtype}"))
    print(f"timestep_embedding {dtype}: max |err| / bound {worst:.3f}")


def test_cfg_std_ratio_within_derived_bound():
    worst = 0.0
    for B in (1, 3):
        for chw in (2, 3, 255, 256, 257, 1024, 129600):
            for off in (0.0, 100.0):
                eps = torch.randn(2 * B, chw, generator=gen(B * 1000 + chw)) + off
                de = eps.to(DEV)
                for gs in (0.0, 1.0, 7.5):
                    out = prefilled((B,), F32)
                    call("gmd_cfg_std_ratio", ptr(de), B, chw, gs, ptr(out))
                    torch.cuda.synchronize()
                    ref, bound = S.cfg_ratio_ref_bound(eps, gs)
                    worst = max(worst, P.assert_elementwise(out, ref, bound, f"cfg_std_ratio B={B} chw={chw} gs={gs} offset={off}"))
    print(f"cfg_std_ratio: max |err| / bound {worst:.3f}")


def test_u8_quantiser_boundary_values():
    """sdr_u8 and gm_u8 of gmd_hdr_tail at every code boundary, against the oracle's float32 restatement, bit for bit."""
    from oracle import hdr_ops as H

    v = S.u8_boundary_inputs()
    n = (v.numel() + 2) // 3
    x = torch.cat([v, v[: 3 * n - v.numel()]]).reshape(1, n, 3)
    y = x.flip(1).contiguous()
    out = _tail(x.to(DEV), y.to(DEV), 1, 1, 1, n, ("sdr_u8", "gm_u8", "sdr", "gm"))
    for k, src in (("sdr", x), ("gm", y)):
        img = H.denorm_clamp(src.numpy()).reshape(1, 1, n, 3)
        S.assert_bit_equal(out[k], torch.from_numpy(img), f"hdr_tail {k} at the code boundaries")
        S.assert_bit_equal(out[k + "_u8"], torch.from_numpy(H.quantize_u8_trunc(img)), f"hdr_tail {k}_u8 at the code boundaries")


def test_u16_discretiser_half_codes_and_ends():
    from oracle import hdr_ops as H

    x, found = S.u16_half_code_inputs()
    assert found >= 100, f"only {found} inputs with x * 65535 == k + 0.5 in float32 were found"
    of, oc = prefilled(x.shape, F32), prefilled(x.shape, torch.int16)
    dx = x.to(DEV)
    call("gmd_discretize_u16", ptr(dx), ptr(of), ptr(oc), x.numel())
    torch.cuda.synchronize()
    S.assert_bit_equal(oc, torch.from_numpy(H.quantize_u16_codes(x.numpy()).view(np.int16)), "discretize_u16 codes at k + 0.5")
    # the float output by value and NaN mask, every non-zero element in its bits: for the input -0 the oracle's clip returns -0 and the
    # device's fmaxf(-0, 0) +0 (IEEE 754 leaves that sign open; the code is 0 either way)
    S.assert_bit_equal(of, torch.from_numpy(H.discretize_to_uint16(x.numpy())), "discretize_u16 float at k + 0.5", zero_sign=False)


def test_rgbe_boundary_values_and_tail_identity():
    from oracle import hdr_ops as H

    px = S.rgbe_boundary_pixels()
    n = px.shape[0]
    out = prefilled((n, 4), torch.uint8)
    dpx = px.to(DEV)
    call("gmd_rgbe_encode", ptr(dpx), ptr(out), n)
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        ref = H.rgbe_encode(px.numpy())
    S.assert_bit_equal(out, torch.from_numpy(ref), "rgbe_encode at the exponent boundaries")
    # The tail's hdr_file = ((s^2.2 + 1/64)(1 + 99 g) - 1/64) / 100 cannot be steered onto most of that table (it lives in [-1.6e-4, 1.02]),
    # so the identity-size resized tail is shown the quantiser boundary values instead and its hdr_rgbe must be Ward's encoding of ITS OWN
    # hdr_file (oracle) and equal gmd_rgbe_encode of it, bit for bit -- the two encoders are one function.
    v = S.u8_boundary_inputs()
    W = (v.numel() + 2) // 3
    x = torch.cat([v, v[: 3 * W - v.numel()]]).reshape(1, 3, 1, W)
    y = x.flip(3).contiguous()
    hf, pe = prefilled((1, 1, W, 3), F32), prefilled((1, 1, W, 4), torch.uint8)
    dx, dy = x.to(DEV), y.to(DEV)
    call("gmd_hdr_tail_resized", ptr(dx), 1, W, ptr(dy), 1, W, 0, 0, 1, 1, W, 99.0, 1 / 64, 0, None, None, None, None, None, ptr(hf), None, ptr(pe))
    torch.cuda.synchronize()
    S.assert_bit_equal(pe, torch.from_numpy(H.rgbe_encode(hf.cpu().numpy())), "hdr_tail_resized hdr_rgbe of its own hdr_file")
    pe2 = prefilled((W, 4), torch.uint8)
    call("gmd_rgbe_encode", ptr(hf), ptr(pe2), W)
    torch.cuda.synchronize()
    S.assert_bit_equal(pe.reshape(W, 4), pe2, "hdr_tail_resized hdr_rgbe vs gmd_rgbe_encode")
