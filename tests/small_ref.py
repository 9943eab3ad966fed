"""References, per-element bounds and edge-value tables for the SMALL kernels (csrc/latent_step.hip, elementwise.hip, hdr_tail.hip, the
row softmax of norm.hip): plain helper module in the style of tests/parity.py and tests/resample_ref.py.  Nothing here uses the library;
bounded checks go through ``parity.assert_elementwise`` (allowed violations: 0), bit-exact ones through ``assert_bit_equal``.

Two kinds of checks:
  * bit-exact kernels (built with -ffp-contract=off, float32 operations in the order of the torch expressions): the references below ARE
    those torch expressions, evaluated in float32 on the CPU with every scalar coefficient held as a float32 0-dim tensor, so that no
    Python double sneaks into an operation the kernel performs in float32;
  * rounded kernels: float64 references with a bound derived from the kernel's operation order (u = 2^-24 throughout).

Grid-stride laps.  Every small kernel is ``for (i = global thread; i < n; i += grid * 256)`` under a capped grid (the three grid_for
functions): one lap covers ``cap * 256`` indices.  The constants below quote the caps; the GPU tests assert ``n > lap`` next to every
launch that is meant to take a thread round its loop a second time, so a later change of a cap cannot quietly turn them into one-lap tests.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import parity as P

LAP_LATENT = 2048 * 256       # csrc/latent_step.hip grid_for: latent / dpm / ddpm step, pack, unpack
LAP_ELEMENTWISE = 4096 * 256  # csrc/elementwise.hip and csrc/hdr_tail.hip grid_for (threads: vectors, pixels or elements, per kernel)
LAP_RESAMPLE = 8192 * 256     # csrc/resample.hip grid_for (output pixels)

U_F32 = 2.0 ** -24
F32 = torch.float32


# ---------------------------------------------------------------------------------------------------------------------------
# bit-exact comparison
# ---------------------------------------------------------------------------------------------------------------------------
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bit_mismatch(got, ref, zero_sign=True):
    """Boolean mask of the elements whose BITS differ (signs of zeros and infinities count); a NaN matches any NaN and nothing else.
    ``zero_sign=False`` lets +0 and -0 match each other (and nothing else): for outputs whose expression takes max(x, 0) of an x that can
    be -0 -- IEEE 754 leaves the sign of maxNum(-0, +0) open, numpy's and torch's clamp return -0 there, the device's fmaxf +0."""
    g, r = got.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    assert g.shape == r.shape, f"shapes differ: got {tuple(g.shape)} ref {tuple(r.shape)}"
    assert g.dtype == r.dtype, f"dtypes differ: got {g.dtype} ref {r.dtype}"
    iv = _INT_VIEW[g.element_size()]
    bits = g.view(iv) != r.view(iv)
    if g.is_floating_point():
        gn, rn = torch.isnan(g), torch.isnan(r)
        bad = (gn != rn) | (~gn & ~rn & bits)
        return bad if zero_sign else bad & ~((g == 0) & (r == 0))
    return bits


def assert_bit_equal(got, ref, what, zero_sign=True):
    """Fail if any element differs in its bits; the message names the count and the first element (flat index: with the lap constants
    above it says at once whether the fault starts at a lap boundary)."""
    bad = bit_mismatch(got, ref, zero_sign)
    n_bad = int(bad.sum())
    if n_bad == 0:
        return
    first = int(bad.reshape(-1).nonzero()[0])
    g, r = got.detach().cpu().reshape(-1)[first], ref.detach().cpu().reshape(-1)[first]
    show = (lambda v: f"{float(v):.9g}") if got.is_floating_point() else (lambda v: str(int(v.to(torch.int64)) & 0xFFFF if v.element_size() == 2 else int(v)))
    raise AssertionError(f"{what}: {n_bad} of {bad.numel()} elements differ; first at flat index {first}: got {show(g)} expected {show(r)}")


def nan_filled(shape, dtype):
    """An output buffer's pre-fill on the CPU side of the emulations: NaN (float) or all-ones bytes (integer)."""
    if dtype.is_floating_point:
        return torch.full(shape, float("nan"), dtype=dtype)
    return torch.full(shape, -1 if dtype in (torch.int16, torch.int32) else 255, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# the step kernels (csrc/latent_step.hip), as float32 torch expressions in the kernels' order
# ---------------------------------------------------------------------------------------------------------------------------
def _s(v):
    return torch.tensor(float(v), dtype=F32)  # a scalar the kernel receives as ``float``


def guided_eps(eps_in, B, do_cfg, gs, ratio=None, gr=0.0, sample_of=None):
    """eps after the CFG combine and the guidance rescale.  eps_in: [2B, ...] (uncond first) or [B, ...].  ``sample_of``: optional int64
    tensor [B * chw] naming the ratio entry each flat element reads (default: its own sample, ``i // chw``); the CPU tests pass a wrong
    one to emulate an index fault."""
    if not do_cfg:
        return eps_in.clone()
    u, t = eps_in[:B], eps_in[B:]
    eps = u + _s(gs) * (t - u)
    if ratio is not None:
        chw = eps[0].numel()
        if sample_of is None:
            sample_of = torch.arange(B * chw) // chw
        r = ratio.to(F32).cpu()[sample_of].reshape(eps.shape)
        resc = eps * r
        eps = _s(gr) * resc + (_s(1.0) - _s(gr)) * eps
    return eps


def latent_step_ref(eps, x, mode, coefs, cur=None, hist=()):
    """(x_prev, x0) of gmd_latent_step given the guided eps; coefs = (sample_coeff, alpha_delta, denom, sqrt_a, sqrt_1ma)."""
    sc, ad, dn, sa, s1 = (_s(c) for c in coefs)
    x0 = (x - s1 * eps) / sa
    smp = x
    if mode == 0:
        m = eps
    elif mode == 1:
        m, smp = (eps + hist[0]) / _s(2.0), cur
    elif mode == 2:
        m = (_s(3.0) * eps - hist[0]) / _s(2.0)
    elif mode == 3:
        m = (_s(23.0) * eps - _s(16.0) * hist[0] + _s(5.0) * hist[1]) / _s(12.0)
    else:
        m = (_s(1.0) / _s(24.0)) * (_s(55.0) * eps - _s(59.0) * hist[0] + _s(37.0) * hist[1] - _s(9.0) * hist[2])
    return sc * smp - ad * m / dn, x0


def dpm_step_ref(eps, x, order, coefs, m1=None):
    """(m0, x_prev, x0) of gmd_dpm_step; coefs = (sigma_s0, alpha_s0, c_x, c_m, c_h, inv_r0, sqrt_a, sqrt_1ma)."""
    sg, al, cx, cm, ch, ir, sa, s1 = (_s(c) for c in coefs)
    x0 = (x - s1 * eps) / sa
    m0 = (x - sg * eps) / al
    r = cx * x - cm * m0
    if order == 2:
        r = r - ch * (ir * (m0 - m1))
    return m0, r, x0


def ddpm_step_ref(eps, x, coefs, noise=None, clip_range=None):
    """(x_prev, x0) of gmd_ddpm_step; coefs = (sched_sqrt_a, sched_sqrt_1ma, x0_coeff, xt_coeff, noise_scale, sqrt_a, sqrt_1ma)."""
    ssa, ss1, c0, ct, ns, sa, s1 = (_s(c) for c in coefs)
    x0 = (x - s1 * eps) / sa
    p0 = (x - ss1 * eps) / ssa
    if clip_range is not None:
        p0 = p0.clamp(-float(clip_range), float(clip_range))
    r = c0 * p0 + ct * x
    if noise is not None:
        r = r + ns * noise
    return r, x0


def pack_ref(s0, s1, dup, cp, dtype):
    """gmd_pack_unet_input: NCHW float32 (+ a second source) -> [dup * B, HW, cp] channels-last of ``dtype``, padding channels zero."""
    src = s0 if s1 is None else torch.cat([s0, s1], 1)
    B, C = src.shape[:2]
    v = src.reshape(B, C, -1).permute(0, 2, 1).to(dtype)
    out = torch.zeros(B, v.shape[1], cp, dtype=dtype)
    out[:, :, :C] = v
    return torch.cat([out] * dup, 0)


def unpack_ref(x, C):
    """gmd_unpack_nchw: [B, HW, ld] -> float32 [B, C, HW] (first C channels)."""
    return x[:, :, :C].to(F32).permute(0, 2, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------
# gmd_cast: edge-value table
# ---------------------------------------------------------------------------------------------------------------------------
FLT_MAX = float(np.finfo(np.float32).max)


def cast_table():
    """float32 values every (in, out) pair of gmd_cast is shown (converted to the input type first, on the CPU):
    signed zeros and infinities, NaN, the smallest subnormal and smallest normal of each type, the float16 overflow boundary (65504 the
    largest finite, 65519.99 still rounds to it, 65520 is the tie that rounds to inf), FLT_MAX (inf in bfloat16), the round-to-nearest-
    even ties of bfloat16 (1 + 2^-8 rounds down to even, 1 + 3 2^-8 up) and of float16 (2^-11), and the ties below the smallest
    subnormals (half of it rounds to zero, three halves to twice it)."""
    pos = [0.0, float("inf"),
           2.0 ** -149, 2.0 ** -126,            # float32: smallest subnormal, smallest normal (also bfloat16's smallest normal)
           2.0 ** -24, 2.0 ** -14,              # float16
           2.0 ** -133,                         # bfloat16's smallest subnormal
           2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -134, 3 * 2.0 ** -134,  # ties under the smallest subnormals
           65504.0, 65519.99, 65520.0, FLT_MAX,
           1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,
           1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -11 + 2.0 ** -23]  # just above a tie: must round up
    vals = pos + [-v for v in pos] + [float("nan")]
    return torch.tensor(vals, dtype=torch.float64).to(F32)


def cast_input(n, in_dtype, seed=0):
    """n values of ``in_dtype``: the table (as far as it fits) followed by randn."""
    t = cast_table()
    x = torch.randn(max(n, 1), generator=torch.Generator().manual_seed(1000 + seed + n))
    k = min(n, t.numel())
    x[:k] = t[:k]
    return x[:n].to(in_dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# gmd_geglu
# ---------------------------------------------------------------------------------------------------------------------------
def geglu_ref_bound(x, out_dtype, floor=True):
    """x: [rows, 2F] stored values ([value | gate]).  Returns (float64 reference h gelu(g), bound, the measured constant).

    The kernel evaluates h * (0.5 g (1 + erff(g / sqrt 2))) in float32 and rounds once to the output type.  Per element
        bound = e + u_out (|ref| + e) + floor,   e = c * 2^-24 (|h gelu(g)| + |h g| / 2),
    floor = the output type's subnormal floor (parity._TINY: a product that lands in float16's subnormal range, |h gelu(g)| < 2^-14, is
    rounded to a multiple of 2^-24, an absolute error of up to 2^-25 that u_out |ref| does not contain; ``floor=False`` switches the term
    off for tests/test_small_kernels_cpu.py, where a clean float16 emulation then breaks the bound).
    The scale: a relative error d of the float32 value moves it by d |h gelu(g)|; an ABSOLUTE error d of erf (what an erf implementation
    has where 1 + erf cancels, g < 0) moves it by d |h g| / 2.  The constant c is not fixed in advance (the device erff carries no
    accuracy figure here): it is MEASURED on the same inputs from the reference,
        c = 4 * max_i |torch CPU float32 evaluation - float64 value|_i / (2^-24 (|h gelu(g)| + |h g| / 2)_i),
    the factor 4 covering a different erf implementation of equal grade."""
    h, g = x.to(torch.float64).chunk(2, -1)
    ref = h * F.gelu(g)
    scale = U_F32 * (ref.abs() + (h * g).abs() / 2)
    h32, g32 = x.to(F32).chunk(2, -1)
    cpu32 = (h32 * F.gelu(g32)).to(torch.float64)
    nz = scale > 0
    c = 4.0 * float(((cpu32 - ref).abs()[nz] / scale[nz]).max()) if bool(nz.any()) else 4.0
    e = c * scale
    return ref, e + P.unit_roundoff(out_dtype) * (ref.abs() + e) + (P._TINY[out_dtype] if floor else 0.0), c


# ---------------------------------------------------------------------------------------------------------------------------
# gmd_softmax_rows
# ---------------------------------------------------------------------------------------------------------------------------
def softmax_ref_bound(s, cols, scale, out_dtype, ldp, causal_nq=0):
    """s: float32 [rows, lds] (columns >= cols are padding the kernel must not read).  Returns float64 ([rows, ldp] reference, bound);
    columns >= the row's attended count (``cols``, or ``row % causal_nq + 1`` for causal rows) are exactly zero with bound 0.

    The kernel (csrc/norm.hip softmax_rows_kernel), per row: x_j = fl(scale s_j); m = max_j x_j (exact on the rounded x);
    w_j = expf(fl(x_j - m)); Z = the sum of the w_j, one thread adding ceil(cols / 256) terms serially, then 6 tree stages inside a wave
    and 2 across the four waves: h = ceil(cols / 256) + 8 additions on the longest path; p_j = fl(w_j * fl(1 / Z)), rounded once to the
    output type.  With exact x = scale s, m = max x:
      * x_j carries |x_j| u; the SAME rounded m enters every term, so its own rounding multiplies numerator and denominator alike and
        cancels; the subtraction rounds once more, |x_j - m| u.  With an FMA (fl(scale s_j - m), one rounding of the exact difference
        against the rounded m) the argument's error is at most |x_j - m| u + |m| u^2: smaller, same bound.  The issue's bound counts
        |x| + |m| + |x - m| for the argument: a superset;
      * expf: 1 ulp = 2u; so w_c is within (|x_c| + |x_c - m| + 2) u relative;
      * Z: the terms' own errors enter weighted by p_j: D u + 2u with D = sum_j p_j (|x_j| + |x_j - m|); its additions: h u;
      * 1 / Z and the product: 2u.
    Total (|x_c| + |x_c - m| + D + h + 6) u.  The bound used is  (2 (|x_c| + |m| + |x_c - m|) + h + 8) u,  which contains the total
    whenever D <= |x_c| + |x_c - m| + 2 |m| + 2.  D is dominated by the columns near the maximum, where |x_j| ~ |m| and x_j - m ~ 0, and
    |x_c| + |x_c - m| >= |m| by the triangle inequality, so the premise holds with room on the test's rows; it is ASSERTED here on the
    data, row by row, in its strongest form (the column with the smallest |x_c| + |x_c - m|), so an input that broke it would fail as a
    broken test and not as a kernel fault.
    Then one rounding to the output type, u_out p, and the output type's subnormal floor (parity._TINY): a probability that
    underflows there -- or whose float32 w_j is subnormal -- is off by at most that much."""
    rows = s.shape[0]
    scale = float(np.float32(scale))
    x = s[:, :cols].to(torch.float64) * scale
    if causal_nq > 0:
        n_att = (torch.arange(rows) % causal_nq + 1).clamp(max=cols)
    else:
        n_att = torch.full((rows,), cols)
    live = torch.arange(cols)[None, :] < n_att[:, None]
    assert bool(torch.isfinite(x[live]).all()), "softmax_ref_bound: non-finite logits inside the attended window"
    xm = torch.where(live, x, torch.full_like(x, -float("inf")))
    m = xm.amax(1, keepdim=True)
    t = torch.where(live, x - m, torch.full_like(x, -float("inf")))
    w = torch.exp(t)
    p = w / w.sum(1, keepdim=True)
    arg = torch.where(live, x.abs() + (x - m).abs(), torch.zeros_like(x))
    D = (p * arg).sum(1)
    least = torch.where(live, arg, torch.full_like(x, float("inf"))).amin(1)
    assert bool((D <= least + 2 * m.abs()[:, 0] + 2).all()), "softmax_ref_bound: the premise D <= |x| + |x - m| + 2 |m| + 2 fails on this input"
    h = math.ceil(cols / 256) + 8
    rel = (2 * (x.abs() + m.abs() + (x - m).abs()) + h + 8) * U_F32 + P.unit_roundoff(out_dtype)
    b = torch.where(live, p * rel + P._TINY[out_dtype], torch.zeros_like(x))
    ref = torch.zeros(rows, ldp, dtype=torch.float64)
    bound = torch.zeros(rows, ldp, dtype=torch.float64)
    ref[:, :cols] = torch.where(live, p, torch.zeros_like(p))
    bound[:, :cols] = b
    return ref, bound


def softmax_rows_input(kind, rows, cols, lds, seed):
    """float32 [rows, lds] logits with NaN in the padding.  kind 0: randn * 4; 1: every logit of a row equal (a different value per row);
    2: one logit per row 200 above the rest (the others' probabilities underflow to zero or a subnormal)."""
    g = torch.Generator().manual_seed(seed)
    s = torch.full((rows, lds), float("nan"))
    if kind == 0:
        v = torch.randn(rows, cols, generator=g) * 4
    elif kind == 1:
        v = (torch.randn(rows, 1, generator=g) * 4).expand(rows, cols).clone()
    else:
        v = torch.randn(rows, cols, generator=g)
        v[torch.arange(rows), torch.arange(rows) * 7 % cols] += 200.0
    s[:, :cols] = v
    return s


# ---------------------------------------------------------------------------------------------------------------------------
# gmd_timestep_embedding
# ---------------------------------------------------------------------------------------------------------------------------
LN_10000 = 9.210340371976184


def temb_ref_bound(t, B, dim, flip, shift, out_dtype):
    """Returns float64 ([B, dim] reference, bound) of gmd_timestep_embedding for the float32 timestep ``t``.

    Kernel: e_k = expf(fl(fl(-9.2103f * k) / (half - shift))), a = fl(t e_k), [sin a | cos a], stored as [cos | sin] when ``flip``.
      * the exponent's argument |arg| <= ln 10^4 = 9.2104 is rounded twice (product, division): the exponential moves by at most
        2 * 9.2104 u relative;
      * the float32 constant is 0.23 u off (2.1 u on e), expf is 1 ulp (2 u), the product t e rounds once (1 u): <= 6 u;
        |d a| <= a (2 * 9.2104 + 6) u, and sin / cos move by at most |d a|;
      * sinf / cosf themselves: 2u absolute (1 ulp of a value in [1/2, 1]);
      * one rounding to the output type: u_out |ref|.
    The bound is tight where a is small and loose where a ~ 10^3 (|d a| ~ 1.5e-3); a wrong index, flip, shift or store moves every
    column by far more than either."""
    half = dim // 2
    k = torch.arange(half, dtype=torch.float64)
    a = float(np.float32(t)) * torch.exp(-LN_10000 * k / (half - float(shift)))
    sn, cs = torch.sin(a), torch.cos(a)
    ref = torch.cat([cs, sn] if flip else [sn, cs])
    da = torch.cat([a, a]) * (2 * 9.2104 + 6) * U_F32
    bound = da + 2 * U_F32 + P.unit_roundoff(out_dtype) * ref.abs()
    return ref[None].expand(B, dim).contiguous(), bound[None].expand(B, dim).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------
# gmd_cfg_std_ratio
# ---------------------------------------------------------------------------------------------------------------------------
def cfg_ratio_ref_bound(eps_pair, gs):
    """eps_pair: float32 [2B, ...] (uncond first).  Returns float64 ([B] reference, bound).

    Kernel (one block per sample): the guided value in float32 in the order u + gs (t - u) (no contraction); sums and sums of squares
    of the text and the guided values in DOUBLE; unbiased variances in double; ratio = fl32(sqrt vt) / fl32(sqrt vc), one float32
    division.  Reference: the guided values formed in torch float32 in that order, both unbiased variances in float64 (two-pass),
    square roots rounded to float32, one float32 division.  Bound 4u relative: the two square-root roundings can differ by one float32
    ulp each if the double accumulations differ in their last bits (2u each, covering the double sums' own error, which is below
    1e-12 relative even at mean / std = 100), none in the division of equal operands -- 4u covers both sides moving."""
    B = eps_pair.shape[0] // 2
    u, t = eps_pair[:B].to(F32), eps_pair[B:].to(F32)
    c = u + _s(gs) * (t - u)
    vt = t.reshape(B, -1).to(torch.float64).var(1, unbiased=True)
    vc = c.reshape(B, -1).to(torch.float64).var(1, unbiased=True)
    assert bool((vc > 0).all()) and bool((vt > 0).all()), "cfg_ratio_ref_bound: a zero variance has no ratio"
    ref = (vt.sqrt().to(F32) / vc.sqrt().to(F32)).to(torch.float64)
    return ref, 4 * U_F32 * ref.abs()


# ---------------------------------------------------------------------------------------------------------------------------
# quantiser / RGBE boundary values
# ---------------------------------------------------------------------------------------------------------------------------
def u8_boundary_inputs():
    """Decoder values around every uint8 code boundary: x = float32(2k/255 - 1) for k = 0..255 (where clamp01(x/2 + 0.5) * 255 sits at
    the integer k up to rounding: truncation must not lose a code) with both float32 neighbours, and the clamp's two sides."""
    k = np.arange(256, dtype=np.float64)
    x = (2 * k / 255 - 1).astype(np.float32)
    extra = np.array([1.0, -1.0, 1.0000001, -1.0000001, 1.2, -1.2], np.float32)
    v = np.concatenate([x, np.nextafter(x, np.float32(2)), np.nextafter(x, np.float32(-2)), extra])
    return torch.from_numpy(v)


def u16_half_code_inputs():
    """float32 inputs x for which x * 65535 IN FLOAT32 is exactly k + 0.5 (the rounding mode of the quantiser decides the code: rintf is
    half-to-even), found by trying the five float32 values around (k + 0.5) / 65535 for every k, plus the two ends and values beyond
    [0, 1].  Returns (tensor, number of exact half codes found)."""
    k = np.arange(65535, dtype=np.float64)
    base = ((k + 0.5) / 65535).astype(np.float32)
    cands = [base]
    lo, hi = base, base
    for _ in range(2):
        lo, hi = np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(2))
        cands += [lo, hi]
    c = np.concatenate(cands)
    prod = c * np.float32(65535)
    exact = c[(prod - np.floor(prod)) == np.float32(0.5)]
    exact = np.unique(exact)
    step = max(1, exact.size // 600)
    pick = exact[::step]
    ends = np.array([0.0, 1.0, -0.0, 65535 / 65535, 1.0000001, 1.5, -1e-9, -0.5, 0.5 / 65535, 65534.5 / 65535, 7.6e-6, np.nextafter(np.float32(1), np.float32(0))],
                    np.float32)
    return torch.from_numpy(np.concatenate([pick, ends])), int(exact.size)


def rgbe_boundary_pixels():
    """float32 [N, 3] pixels at the edges of Ward's encoder: the brightest channel at 2^e for every e in -106..127 (frexp's mantissa 1/2:
    the scale is exactly 2^(8 - e - 1)) and at the float32 below it (mantissa 1 - 2^-24: the brightest byte 255, unless a ROUNDED
    mantissa overflows it), 1e-32f and the float32 below it (the zero-pixel threshold), FLT_MAX, and negative channels beside a positive
    one.  No NaN / inf (the oracle's maximum and the device's fmaxf differ there by definition)."""
    px = []
    for e in range(-106, 128):
        v = np.ldexp(np.float32(1), e).astype(np.float32)
        b = np.nextafter(v, np.float32(0))
        px += [(v, v * np.float32(0.75), np.float32(0)), (v * np.float32(0.3), v, v * np.float32(0.999)), (b, b * np.float32(0.5), b),
               (np.float32(0), b * np.float32(0.9), b), (-v, v, np.float32(-1)), (b, -b, v * np.float32(2.0 ** -30))]
    t = np.float32(1e-32)
    tb = np.nextafter(t, np.float32(0))
    fm = np.float32(FLT_MAX)
    px += [(t, np.float32(0), np.float32(0)), (tb, tb, tb), (np.float32(0), t, tb), (fm, np.float32(1), fm / np.float32(3)), (fm, fm, fm),
           (np.float32(-1), np.float32(-2), np.float32(-3)), (np.float32(0), np.float32(0), np.float32(0)), (np.float32(-0.0), np.float32(1), np.float32(0.5))]
    return torch.from_numpy(np.array(px, np.float32))
