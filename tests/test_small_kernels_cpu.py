"""CPU: the checks of tests/small_ref.py have teeth (the companion of tests/test_small_kernels_gpu.py, in the way tests/test_parity_cpu.py
accompanies the parity tests).  For every checker a clean torch emulation of the kernel must pass and at least one faulty emulation --
the faults a grid-stride loop, a cast, a softmax, an embedding, a variance or a quantiser really can have -- must fail."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity as P
import small_ref as S

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gm-diffusion_amd", "csrc")


def must_fail(fn, match=None):
    with pytest.raises(AssertionError, match=match):
        fn()


# ---- the lap constants ----
def test_lap_constants_quote_the_grid_caps():
    """LAP_* = (the cap of the file's grid_for) * 256 threads; a changed cap must be followed here, or the GPU tests' n > lap assertions
    would guard the wrong number."""
    for name, lap in (("latent_step.hip", S.LAP_LATENT), ("elementwise.hip", S.LAP_ELEMENTWISE), ("hdr_tail.hip", S.LAP_ELEMENTWISE), ("resample.hip", S.LAP_RESAMPLE)):
        src = open(os.path.join(CSRC, name)).read()
        body = src[src.index("inline int grid_for"):]
        cap = re.search(r"if \(g > ([0-9* ]+)\) g = ([0-9* ]+);", body)
        assert cap and cap.group(1) == cap.group(2), name
        assert re.search(r"constexpr int kThreads = 256;", src), name
        assert eval(cap.group(1)) * 256 == lap, (name, cap.group(1), lap)
    # the float32 slab reducer (tests/split_cases.py LAP_REDUCE; tests/test_split_parity_gpu.py asserts the second lap's rows): one
    # thread per four columns, the grid capped where launch_split_any launches it
    import split_cases

    src = open(os.path.join(CSRC, "gemm_split.hip")).read()
    launch = src[src.index("int launch_split_any"):]
    m = re.search(r"const int64_t total = \(int64_t\)p\.M \* \(\(p\.N \+ 3\) / 4\);\s*int64_t g = \(total \+ (\d+)\) / (\d+);\s*if \(g > (\d+)\) g = (\d+);\s*"
                  r"splitk_reduce_f32_kernel<<<\(int\)g, (\d+), 0, s>>>", launch)
    assert m and m.group(3) == m.group(4) and int(m.group(1)) + 1 == int(m.group(2)) == int(m.group(5)), "the reducer's launch moved"
    assert (int(m.group(3)), int(m.group(5))) == (split_cases.REDUCE_GRID_CAP, split_cases.REDUCE_THREADS)
    assert split_cases.LAP_REDUCE == int(m.group(3)) * int(m.group(5)) == 1 << 20
    assert "i += (int64_t)gridDim.x * blockDim.x" in src[src.index("void splitk_reduce_f32_kernel"):src.index("// ring kernel:")]
    M, N = split_cases.SECOND_LAP[1:3]
    assert split_cases.reducer_lap_start(M, N) == (3276, 1024) and split_cases.reducer_lap_start(4096, 1024) is None


# ---- second lap: never written / first lap's sample index ----
def _second_lap_unwritten(ref, lap):
    out = S.nan_filled(ref.shape, ref.dtype).reshape(-1)
    out[:lap] = ref.reshape(-1)[:lap]
    return out.reshape(ref.shape)


def test_bit_check_catches_an_unwritten_second_lap():
    B, chw = 2, 4 * 257 * 257
    n = B * chw
    assert n > S.LAP_LATENT
    g = torch.Generator().manual_seed(1)
    eps_in, x = torch.randn(2 * B, chw, generator=g), torch.randn(B, chw, generator=g)
    eps = S.guided_eps(eps_in, B, True, 7.5, torch.tensor([0.25, 3.0]), 0.7)
    xp, x0 = S.latent_step_ref(eps, x, 0, (1.01, 0.02, 0.97, 0.8, 0.6))
    S.assert_bit_equal(xp.clone(), xp, "clean")
    must_fail(lambda: S.assert_bit_equal(_second_lap_unwritten(xp, S.LAP_LATENT), xp, "x_prev"), match=f"{n - S.LAP_LATENT} of {n} elements differ; first at flat index {S.LAP_LATENT}")
    # integer outputs: the 0xFF pre-fill of a u8 image (a real code, so a random image hides 1/256 of it: the count says so)
    img = torch.randint(0, 255, (S.LAP_ELEMENTWISE + 257,), dtype=torch.uint8, generator=g)
    must_fail(lambda: S.assert_bit_equal(_second_lap_unwritten(img, S.LAP_ELEMENTWISE), img, "u8"), match=f"257 of .* first at flat index {S.LAP_ELEMENTWISE}")
    # one single element, the very last
    last = xp.clone()
    last.view(-1)[-1] = torch.nextafter(last.view(-1)[-1], torch.tensor(9.0))
    must_fail(lambda: S.assert_bit_equal(last, xp, "last"), match=f"1 of {n} elements differ; first at flat index {n - 1}")


def test_bit_check_catches_the_first_laps_sample_index():
    """ratio[i / chw] and i / HW evaluated with the FIRST lap's index (i - grid * 256) on the second lap."""
    B, chw = 2, 4 * 257 * 257
    g = torch.Generator().manual_seed(2)
    eps_in = torch.randn(2 * B, chw, generator=g)
    ratio = torch.tensor([0.25, 3.0])
    i = torch.arange(B * chw)
    good = S.guided_eps(eps_in, B, True, 7.5, ratio, 0.7)
    S.assert_bit_equal(S.guided_eps(eps_in, B, True, 7.5, ratio, 0.7, sample_of=i // chw), good, "clean")
    stale = torch.where(i >= S.LAP_LATENT, i - S.LAP_LATENT, i) // chw
    must_fail(lambda: S.assert_bit_equal(S.guided_eps(eps_in, B, True, 7.5, ratio, 0.7, sample_of=stale), good, "eps"), match=f"first at flat index {S.LAP_LATENT}")
    # with equal ratio entries the fault would be invisible: the reason the GPU test uses two very different ones
    same = torch.tensor([0.5, 0.5])
    S.assert_bit_equal(S.guided_eps(eps_in, B, True, 7.5, same, 0.7, sample_of=stale), S.guided_eps(eps_in, B, True, 7.5, same, 0.7), "equal ratios hide it")

    # unpack: out[i] = in[(b HW + p) ld + c], (b, c) from i / HW
    Bu, C, HW, ld = 3, 4, 257 * 257, 8
    assert Bu * C * HW > S.LAP_LATENT
    x = torch.full((Bu, HW, ld), float("nan"), dtype=BF16)
    x[:, :, :C] = torch.randn(Bu, HW, C, generator=g).to(BF16)

    def unpack_emu(stale_index):
        i = torch.arange(Bu * C * HW)
        j = torch.where(i >= S.LAP_LATENT, i - S.LAP_LATENT, i) if stale_index else i
        p, bc = i % HW, j // HW
        b = bc // C
        c = bc - b * C
        return x.reshape(-1)[(b * HW + p) * ld + c].float().reshape(Bu, C, HW)

    ref = S.unpack_ref(x, C)
    S.assert_bit_equal(unpack_emu(False), ref, "clean unpack")
    must_fail(lambda: S.assert_bit_equal(unpack_emu(True), ref, "unpack"), match=f"first at flat index {S.LAP_LATENT}")
    # pack: a padding channel left unwritten, a duplicate left unwritten
    s0, s1 = torch.randn(2, 4, 37, 1, generator=g), torch.randn(2, 4, 37, 1, generator=g)
    pr = S.pack_ref(s0, s1, 2, 16, F16)
    assert pr.shape == (4, 37, 16) and not bool(pr[:, :, 8:].ne(0).any()) and torch.equal(pr[:2], pr[2:])
    bad = pr.clone()
    bad[:, :, 15] = float("nan")
    must_fail(lambda: S.assert_bit_equal(bad, pr, "pack padding"))
    bad = pr.clone()
    bad[2:] = float("nan")
    must_fail(lambda: S.assert_bit_equal(bad, pr, "pack duplicate"))


def test_step_references_follow_the_schedulers_expressions():
    """The float32 expressions of small_ref against plain torch arithmetic with Python scalars (what the existing bit-exact tests use):
    identical bits, so the two-lap tests compare with the same thing at another size."""
    g = torch.Generator().manual_seed(3)
    eps, x, e1, e2, e3, cur = (torch.randn(2, 4, 9, 9, generator=g) for _ in range(6))
    sc, ad, dn, sa, s1 = coefs = (1.01, 0.02, 0.97, 0.8, 0.6)
    xp, x0 = S.latent_step_ref(eps, x, 4, coefs, hist=(e1, e2, e3))
    assert torch.equal(x0, (x - s1 * eps) / sa)
    assert torch.equal(xp, sc * x - ad * ((1 / 24) * (55 * eps - 59 * e1 + 37 * e2 - 9 * e3)) / dn)
    xp, _ = S.latent_step_ref(eps, x, 1, coefs, cur=cur, hist=(e1,))
    assert torch.equal(xp, sc * cur - ad * ((eps + e1) / 2) / dn)
    raw = torch.randn(4, 4, 9, 9, generator=g)
    u, c = raw.chunk(2)
    cfg = u + 7.5 * (c - u)
    assert torch.equal(S.guided_eps(raw, 2, True, 7.5), cfg)
    r = torch.tensor([0.25, 3.0])
    assert torch.equal(S.guided_eps(raw, 2, True, 7.5, r, 0.7), 0.7 * (cfg * r.view(2, 1, 1, 1)) + (1 - 0.7) * cfg)


# ---- cast ----
def test_cast_check_catches_truncation_and_lost_signs():
    x = S.cast_input(1001, F32)
    ref = x.to(BF16)
    S.assert_bit_equal(x.to(BF16), ref, "clean")
    trunc = (x.view(torch.int32) & -65536).view(F32).to(BF16)  # drop the low 16 bits: round toward zero
    must_fail(lambda: S.assert_bit_equal(trunc, ref, "truncating cast"))
    tab = S.cast_table()
    t16 = tab.to(F16)
    assert bool(torch.isinf(t16[tab == 65520.0]).all()) and float(t16[tab == 65519.99][0]) == 65504.0, "the float16 overflow tie is in the table"
    assert float(tab[tab == 1 + 2.0 ** -8].to(BF16)[0]) == 1.0 and float(tab[tab == 1 + 3 * 2.0 ** -8].to(BF16)[0]) == 1 + 2.0 ** -6, "bfloat16 ties to even"
    pos_zero = ref.clone()
    pos_zero[(ref == 0) & torch.signbit(ref)] = 0.0
    must_fail(lambda: S.assert_bit_equal(pos_zero, ref, "-0 stored as +0"))
    nan_as_inf = torch.where(torch.isnan(ref), torch.full_like(ref, float("inf")), ref)
    must_fail(lambda: S.assert_bit_equal(nan_as_inf, ref, "NaN stored as inf"))
    flushed = torch.where(ref.float().abs() < 2.0 ** -126, torch.zeros_like(ref), ref)
    must_fail(lambda: S.assert_bit_equal(flushed, ref, "subnormals flushed"))


# ---- softmax ----
def _softmax_emu(s, cols, scale, dtype, ldp, subtract_max=True, zero_to=None, causal_nq=0):
    """float32 torch emulation of softmax_rows_kernel into a NaN pre-filled [rows, ldp] buffer."""
    rows = s.shape[0]
    out = S.nan_filled((rows, ldp), dtype)
    zero_to = ldp if zero_to is None else zero_to
    for r in range(rows):
        n = min(cols, r % causal_nq + 1) if causal_nq else cols
        x = s[r, :n] * np.float32(scale)
        m = x.max() if subtract_max else torch.tensor(0.0)
        w = torch.exp(x - m)
        out[r, :zero_to] = 0
        out[r, :n] = (w * (torch.tensor(1.0) / w.sum())).to(dtype)
    return out


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_softmax_bound_passes_clean_and_catches_faults(dtype):
    for cols in (5, 65, 257):
        lds, ldp = cols + 5, (cols + 7) // 8 * 8 + 8
        for kind, scale in ((0, 0.3), (1, 0.3), (2, 0.5)):
            s = S.softmax_rows_input(kind, 6, cols, lds, cols + kind)
            ref, bound = S.softmax_ref_bound(s, cols, scale, dtype, ldp)
            P.assert_elementwise(_softmax_emu(s, cols, scale, dtype, ldp), ref, bound, "clean")
            # the zero fill stops at cols rounded up to 8: the last 8 columns keep the pre-fill
            must_fail(lambda: P.assert_elementwise(_softmax_emu(s, cols, scale, dtype, ldp, zero_to=(cols + 7) // 8 * 8), ref, bound, "short zero fill"))
        s = S.softmax_rows_input(2, 6, cols, lds, cols)
        ref, bound = S.softmax_ref_bound(s, cols, 0.5, dtype, ldp)
        # no max subtraction: exp(100) overflows float32 on the spiked row
        must_fail(lambda: P.assert_elementwise(_softmax_emu(s, cols, 0.5, dtype, ldp, subtract_max=False), ref, bound, "no max subtraction"))
    # causal rows, and a causal kernel that attends one column too many
    cols = 77
    s = S.softmax_rows_input(0, 2 * cols, cols, cols + 5, 9)
    ref, bound = S.softmax_ref_bound(s, cols, 0.3, dtype, 88, causal_nq=cols)
    P.assert_elementwise(_softmax_emu(s, cols, 0.3, dtype, 88, causal_nq=cols), ref, bound, "clean causal")
    must_fail(lambda: P.assert_elementwise(_softmax_emu(s, cols, 0.3, dtype, 88, causal_nq=cols + 1), ref, bound, "causal off by one"))
    # one column in eight wrong by half a bfloat16 ulp of ITS value: invisible to a 1.5e-2 RMS tolerance, not to the bound (float32 output)
    if dtype == F32:
        s = S.softmax_rows_input(0, 6, 256, 261, 4)
        ref, bound = S.softmax_ref_bound(s, 256, 0.3, F32, 264)
        bad = _softmax_emu(s, 256, 0.3, F32, 264)
        bad[:, 0:256:8] *= 1 + 2.0 ** -9
        assert float((bad.double() - ref).norm() / ref.norm()) < 1.5e-2
        must_fail(lambda: P.assert_elementwise(bad, ref, bound, "one column in eight"))


# ---- timestep embedding ----
def _temb_emu(t, B, dim, flip, shift, dtype, swap=False, ignore_shift=False):
    half = dim // 2
    k = torch.arange(half, dtype=F32)
    den = torch.tensor(float(half), dtype=F32) - (0.0 if ignore_shift else np.float32(shift))
    a = torch.tensor(t, dtype=F32) * torch.exp(torch.tensor(-S.LN_10000, dtype=F32) * k / den)
    sn, cs = torch.sin(a), torch.cos(a)
    first_cos = bool(flip) != swap
    return torch.cat([cs, sn] if first_cos else [sn, cs]).to(dtype)[None].expand(B, dim).contiguous()


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_timestep_embedding_bound_passes_clean_and_catches_faults(dtype):
    for dim in (2, 256, 320, 1280):
        for flip in (0, 1):
            for shift in (0, 1):
                if dim == 2 and shift:
                    continue
                for t in (0.0, 1.0, 20.5, 501.0, 981.0, 999.0):
                    ref, bound = S.temb_ref_bound(t, 3, dim, flip, shift, dtype)
                    P.assert_elementwise(_temb_emu(t, 3, dim, flip, shift, dtype), ref, bound, "clean")
                    must_fail(lambda: P.assert_elementwise(_temb_emu(t, 3, dim, flip, shift, dtype, swap=True), ref, bound, "halves swapped"))
                    if shift and t > 0:
                        must_fail(lambda: P.assert_elementwise(_temb_emu(t, 3, dim, flip, shift, dtype, ignore_shift=True), ref, bound, "half instead of half - shift"))
    # a single wrong column (index off by one in the last column of a half) at the largest argument, where the bound is loosest
    ref, bound = S.temb_ref_bound(999.0, 1, 320, 1, 0, F32)
    bad = _temb_emu(999.0, 1, 320, 1, 0, F32)
    bad[0, 159] = bad[0, 158]
    must_fail(lambda: P.assert_elementwise(bad, ref, bound, "one column"))


# ---- cfg_std_ratio ----
def _cfg_ratio_emu(eps_pair, gs, biased_guided=False):
    """The kernel's arithmetic: float32 guided value, double sums, (sum x^2 - (sum x)^2 / N) / (N - 1), float32 roots and division."""
    B = eps_pair.shape[0] // 2
    u, t = eps_pair[:B].reshape(B, -1), eps_pair[B:].reshape(B, -1)
    c = u + torch.tensor(gs, dtype=F32) * (t - u)
    N = u.shape[1]

    def var(v, div):
        v = v.double()
        return ((v * v).sum(1) - v.sum(1) ** 2 / N) / div

    return var(t, N - 1).sqrt().float() / var(c, N if biased_guided else N - 1).sqrt().float()


def test_cfg_std_ratio_bound_passes_clean_and_catches_a_biased_variance():
    """(Biasing BOTH variances cancels in the ratio, at every chw: no test can see that.  One biased variance does not cancel.)"""
    for B in (1, 3):
        for chw in (2, 3, 255, 257, 129600):
            for off in (0.0, 100.0):
                eps = torch.randn(2 * B, chw, generator=torch.Generator().manual_seed(chw + B)) + off
                for gs in (0.0, 1.0, 7.5):
                    ref, bound = S.cfg_ratio_ref_bound(eps, gs)
                    P.assert_elementwise(_cfg_ratio_emu(eps, gs), ref, bound, f"clean chw={chw} gs={gs} off={off}")
                    if chw <= 257:  # sqrt(N / (N - 1)) - 1 = 2e-3 at 257; at 129600 it is 3.9e-6, still 16x the bound
                        must_fail(lambda: P.assert_elementwise(_cfg_ratio_emu(eps, gs, biased_guided=True), ref, bound, "biased"))
    eps = torch.randn(2, 129600, generator=torch.Generator().manual_seed(5))
    ref, bound = S.cfg_ratio_ref_bound(eps, 7.5)
    must_fail(lambda: P.assert_elementwise(_cfg_ratio_emu(eps, 7.5, biased_guided=True), ref, bound, "biased at 129600"))
    # a float32 accumulation at mean / std = 100 loses the variance: caught
    eps = torch.randn(2, 129600, generator=torch.Generator().manual_seed(6)) + 100
    ref, bound = S.cfg_ratio_ref_bound(eps, 7.5)
    t32 = eps[1:].float()
    v32 = ((t32 * t32).sum(1) - t32.sum(1) ** 2 / 129600) / 129599
    c = eps[:1] + torch.tensor(7.5) * (eps[1:] - eps[:1])
    got = v32.clamp_min(1e-12).sqrt() / c.double().var(1).sqrt().float()
    must_fail(lambda: P.assert_elementwise(got, ref, bound, "float32 sums"))


# ---- GEGLU ----
@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_geglu_bound_passes_clean_and_catches_faults(dtype):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(37, 2 * 1280, generator=g) * 2
    x[0, 1280:1284] = torch.tensor([10.0, -10.0, 40.0, -40.0])
    x = x.to(dtype)
    ref, bound, c = S.geglu_ref_bound(x, dtype)
    assert 1.0 <= c <= 64.0, f"the measured constant {c} is not that of a float32 erf"
    h, gt = x.float().chunk(2, -1)
    P.assert_elementwise((h * F.gelu(gt)).to(dtype), ref, bound, "clean")
    if dtype == F16:  # the subnormal floor of the bound is needed: products below 2^-14 round to multiples of 2^-24
        _, no_floor, _ = S.geglu_ref_bound(x, dtype, floor=False)
        must_fail(lambda: P.assert_elementwise((h * F.gelu(gt)).to(dtype), ref, no_floor, "clean, bound without the floor"))
    # another float32 formulation of the same function (erfc of the negated argument): inside the factor 4
    alt = h * (0.5 * gt * torch.special.erfc(-gt * np.float32(0.7071067811865476)))
    P.assert_elementwise(alt.to(dtype), ref, bound, "erfc form")
    must_fail(lambda: P.assert_elementwise((h * F.gelu(gt, approximate="tanh")).to(dtype), ref, bound, "tanh approximation"))
    swapped = (gt * F.gelu(h)).to(dtype)
    must_fail(lambda: P.assert_elementwise(swapped, ref, bound, "value and gate swapped"))
    if dtype == F32:  # an evaluation through bfloat16 passes an RMS tolerance of 1.5e-2 and not the bound
        low = (h * F.gelu(gt).to(BF16).float())
        assert float((low.double() - ref).norm() / ref.norm()) < 1.5e-2
        must_fail(lambda: P.assert_elementwise(low, ref, bound, "gelu rounded to bfloat16"))


# ---- quantisers and RGBE ----
def test_quantiser_tables_catch_rounding_faults():
    from oracle import hdr_ops as H

    v = S.u8_boundary_inputs().numpy()
    img = H.denorm_clamp(v)
    good = torch.from_numpy(H.quantize_u8_trunc(img))
    S.assert_bit_equal(good.clone(), good, "clean")
    assert len(np.unique(good.numpy())) == 256, "every code appears in the table"
    rounded = torch.from_numpy(np.rint(img * np.float32(255)).astype(np.uint8))
    must_fail(lambda: S.assert_bit_equal(rounded, good, "u8 that rounds"))

    x, found = S.u16_half_code_inputs()
    assert found >= 100
    xn = x.numpy()
    good = torch.from_numpy(H.quantize_u16_codes(xn).view(np.int16))
    half_up = np.floor(np.clip(xn * np.float32(65535), 0, 65535).astype(np.float64) + 0.5).astype(np.uint16)
    must_fail(lambda: S.assert_bit_equal(torch.from_numpy(half_up.view(np.int16)), good, "round half up"))
    # the float output is compared with zero_sign=False: the oracle keeps the sign of a -0 input through its clip, fmaxf(-0, 0) need not
    goodf = torch.from_numpy(H.discretize_to_uint16(xn))
    assert bool(((goodf == 0) & torch.signbit(goodf)).any()), "the table holds the input -0, whose oracle value is -0"
    plus = torch.where(goodf == 0, torch.zeros_like(goodf), goodf)
    must_fail(lambda: S.assert_bit_equal(plus, goodf, "+0 for -0, signs compared"))
    S.assert_bit_equal(plus, goodf, "+0 for -0", zero_sign=False)
    ulp = plus.clone()
    ulp[plus == 1] = float(np.nextafter(np.float32(1), np.float32(0)))
    must_fail(lambda: S.assert_bit_equal(ulp, goodf, "one ulp off", zero_sign=False))
    tiny = torch.where(goodf == 0, torch.full_like(goodf, 1e-45), goodf)
    must_fail(lambda: S.assert_bit_equal(tiny, goodf, "a subnormal for a zero", zero_sign=False))
    no_clamp = np.rint(xn * np.float32(65535)).astype(np.int64).astype(np.uint16)
    must_fail(lambda: S.assert_bit_equal(torch.from_numpy(no_clamp.view(np.int16)), good, "no clamp beyond [0, 1]"))


def _rgbe_emu(rgb, round_mantissa=False, threshold=np.float32(1e-32)):
    x = np.maximum(rgb.astype(np.float32), np.float32(0))
    v = x.max(-1)
    m, e = np.frexp(v)
    ok = v >= threshold
    with np.errstate(all="ignore"):
        s = (m.astype(np.float32) * np.float32(256) / np.where(ok, v, np.float32(1))).astype(np.float32)
        prod = x * s[..., None]
        q = (np.rint(prod) if round_mantissa else prod).astype(np.int32)
    out = np.zeros(x.shape[:-1] + (4,), np.uint8)
    out[..., :3] = np.where(ok[..., None], q, 0).astype(np.uint8)
    out[..., 3] = np.where(ok, e + 128, 0).astype(np.uint8)
    return torch.from_numpy(out)


def test_rgbe_table_catches_rounding_and_threshold_faults():
    from oracle import hdr_ops as H

    px = S.rgbe_boundary_pixels().numpy()
    with np.errstate(all="ignore"):
        good = torch.from_numpy(H.rgbe_encode(px))
    S.assert_bit_equal(_rgbe_emu(px), good, "clean")
    must_fail(lambda: S.assert_bit_equal(_rgbe_emu(px, round_mantissa=True), good, "rounded mantissa"))
    must_fail(lambda: S.assert_bit_equal(_rgbe_emu(px, threshold=np.nextafter(np.float32(1e-32), np.float32(1))), good, "threshold one float32 up"))
    must_fail(lambda: S.assert_bit_equal(_rgbe_emu(px, threshold=np.float32(0)), good, "no threshold"))
    # the table reaches every exponent byte from 2^-106 to FLT_MAX's wrapped one
    assert set(range(128 - 106 + 1, 256)) <= set(np.unique(good[:, 3].numpy()).tolist())
