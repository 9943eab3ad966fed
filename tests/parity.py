"""Per-element parity checker for the HIP kernels (plain helper module, like tests/anysize_ref.py).

A global norm ``|got - ref| / |ref|`` averages over millions of elements, so the faults tiled kernels really have -- a ragged
edge, one fragment, one K step of one tile, the last row of a sample -- vanish in it.  Here every element gets a bound of its own,
DERIVED from the arithmetic the kernel performs, and not one element may exceed it.

Everything is float64 torch and device-agnostic (the bounds are computed where the tensors live).  The reference of a check is
always float64 torch, never this library.  Unit roundoffs: bf16 2^-8, f16 2^-11, f32 2^-24 (round to nearest: |fl(x) - x| <= u |x|).
"""
import math

import torch
import torch.nn.functional as F

U_BF16, U_F16, U_F32 = 2.0 ** -8, 2.0 ** -11, 2.0 ** -24
# smallest spacing of the subnormal range / 2: the absolute error of a rounding that lands there (results below it may also be flushed
# to zero, which costs at most the same)
_TINY = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -126, torch.float64: 0.0}

# Terms of the bounds that tests/test_parity_cpu.py switches off ONE AT A TIME to show that each is needed (a clean emulation must
# then break the bound): names as used by ``_on`` below.  Always empty outside that test.
DISABLED = set()


def _on(term):
    return 0.0 if term in DISABLED else 1.0


# Lipschitz constants of the epilogue activations (an incoming error e becomes at most L e):
#   SiLU          f(x) = x s(x), s = logistic: f' = s (1 + x (1 - s)), maximal at the root of f'' (x = 2.3994): 1.09984; min -0.09984
#   quick-GELU    f(x) = x s(1.702 x): f'(x) = g(1.702 x) with g the derivative above -- the same range, 1.09984
#   erf-GELU      f(x) = x Phi(x): f' = Phi + x phi, f'' = phi (2 - x^2) = 0 at x = sqrt 2: Phi(1.41421) + 1.41421 phi(1.41421) = 1.12893
LIP_SILU = 1.0999
LIP_QUICK_GELU = 1.0999
LIP_GELU = 1.1290


def unit_roundoff(dtype):
    return {torch.bfloat16: U_BF16, torch.float16: U_F16, torch.float32: U_F32, torch.float64: 2.0 ** -53}[dtype]


# ---------------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------------
def violations(got, ref64, bound64):
    """(mask, got64, ref64, bound64): the boolean mask of the elements that break their bound -- ``|got - ref| > bound``, or non-finite
    where ``ref`` is finite -- and the three operands as float64 on one device.  ``ref`` must be finite (asserted): a reference with
    inf / NaN in it is a broken test, not a kernel fault."""
    g = got.detach().to(torch.float64)
    r = ref64.detach().to(device=g.device, dtype=torch.float64)
    b = bound64.detach().to(device=g.device, dtype=torch.float64)
    assert g.shape == r.shape == b.shape, f"shapes differ: got {tuple(g.shape)} ref {tuple(r.shape)} bound {tuple(b.shape)}"
    assert bool(torch.isfinite(b).all()) and bool((b >= 0).all()), "a bound must be finite and non-negative"
    assert bool(torch.isfinite(r).all()), "the float64 reference must be finite"
    bad = ~torch.isfinite(g) & torch.isfinite(r)
    return bad | ((g - r).abs() > b), g, r, b


def assert_elementwise(got, ref64, bound64, what, tile=None):
    """Fail if ANY element has ``|got - ref| > bound`` or is non-finite where ``ref`` is finite (allowed violations: 0).

    The message names the count, the worst element's index, ``got``, ``ref``, ``bound`` there and, with ``tile=(bm, bn)``, the tile
    coordinates (over the last two dimensions) of the worst element and the number of distinct tiles with violations, so a failure
    points at a fragment.  Returns max |err| / bound for reports."""
    bad, g, r, b = violations(got, ref64, bound64)
    n_bad = int(bad.sum())
    ratio = (g - r).abs() / b.clamp_min(1e-300)
    if n_bad == 0:
        return float(ratio.max()) if ratio.numel() else 0.0
    score = torch.where(bad, torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf"))), torch.zeros_like(ratio))
    flat = int(score.reshape(-1).argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), g.shape)) if g.dim() else ()
    msg = (f"{what}: {n_bad} of {g.numel()} elements outside their bound; worst at {idx}: got {float(g[idx]):.9g} "
           f"ref {float(r[idx]):.9g} |err| {abs(float(g[idx]) - float(r[idx])):.3e} bound {float(b[idx]):.3e}")
    if tile is not None and g.dim() >= 2:
        bm, bn = tile
        rows, cols = g.shape[-2], g.shape[-1]
        b2 = bad.reshape(-1, rows, cols)
        nz = b2.nonzero()
        tiles = torch.unique(torch.stack([nz[:, 0], nz[:, 1] // bm, nz[:, 2] // bn], 1), dim=0)
        msg += (f"; worst element in tile (row block {idx[-2] // bm}, column block {idx[-1] // bn}) of {bm}x{bn} tiles, "
                f"at ({idx[-2] % bm}, {idx[-1] % bn}) inside it; {tiles.shape[0]} distinct tiles hold violations")
    raise AssertionError(msg)


# ---------------------------------------------------------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------------------------------------------------------
def _act_ref(v, act):
    if act in (None, "none"):
        return v
    if act == "silu":
        return F.silu(v)
    if act == "quick_gelu":
        return v * torch.sigmoid(1.702 * v)
    if act == "gelu":
        return F.gelu(v)
    raise ValueError(act)


def act_eval_error(v, act):
    """Error of the kernels' float32 EVALUATION of an activation at an exact argument v (csrc/gmd_common.h silu_f, gemm_shared.h
    apply_act / fast_erf), from the documented accuracy of the instructions: v_exp_f32 and v_rcp_f32 are 1 ulp (2^-23 relative).

    SiLU = v * rcp(1 + __expf(-v)), quick-GELU = v / (1 + __expf(-1.702 v)).  __expf(t) = exp2(t * log2 e): the rounded product
    moves the exponent by at most 2^-24 |t log2 e| ln 2 = 2^-24 |t| relative, the instruction adds 2^-23: e = exp(t) carries
    (|t| + 2) 2^-24.  s = 1 / (1 + e): the error of e enters weighted by e / (1 + e) = 1 - s <= 1, the add rounds once (2^-24), the
    reciprocal / division is within 2^-23, the final product rounds once: relative error of the result
        <= ((1 - s) (|t| + 2) + 1 + 2 + 1) 2^-24 <= ((1 - s) |t| + 6) 2^-24.
    (1 - s)|t| <= |t| for negative v and decays like |t| e^-|t| <= 0.37 for positive v.  When e overflows (t > 88) the result is -0
    for a true value below 1e-36: covered by the absolute floor.

    erf-GELU (GEGLU epilogue) uses Abramowitz & Stegun 7.1.26, absolute error of erf <= 1.5e-7 plus the float32 evaluation of a
    degree-5 Horner form (six roundings of terms <= 1.5: 9 2^-24) and the exp2 / rcp instructions (2 2^-23 of a factor <= 1):
    |d erf| <= 1.5e-7 + 13 2^-24 <= 9.3e-7, so |d gelu| <= |v| / 2 * 9.3e-7 + 2 2^-24 |gelu(v)|."""
    v = v.to(torch.float64)
    if act in (None, "none"):
        return torch.zeros_like(v)
    if act in ("silu", "quick_gelu"):
        t = v if act == "silu" else 1.702 * v
        one_minus_s = torch.sigmoid(-t)
        return _act_ref(v, act).abs() * ((one_minus_s * t.abs() + 6.0) * U_F32) + 1e-36
    if act == "gelu":
        return v.abs() * 0.5 * 9.3e-7 + 2 * U_F32 * F.gelu(v).abs()
    raise ValueError(act)


def _finish(value, err_in, out_dtype, act=None):
    """Bound of ``store(act(value + e))``, |e| <= err_in: Lipschitz constant of the activation times the incoming bound, the
    activation's own evaluation error, then ONE rounding of the stored value: u_out (|exact result| + everything accumulated so far)
    plus the subnormal floor of the output type."""
    lip = {None: 1.0, "none": 1.0, "silu": LIP_SILU, "quick_gelu": LIP_QUICK_GELU, "gelu": LIP_GELU}[act]
    e = lip * err_in + _on("act_eval") * act_eval_error(value, act)
    out = _act_ref(value, act)
    return e + _on("out_round") * unit_roundoff(out_dtype) * (out.abs() + e) + _TINY[out_dtype]


# ---------------------------------------------------------------------------------------------------------------------------
# contractions
# ---------------------------------------------------------------------------------------------------------------------------
def mfma_height(n_products, kstep, slices=1):
    """Largest number of float32 additions any ONE product passes through in a K loop of matrix-core instructions that each add
    ``kstep`` products to the accumulator they are chained through (csrc: mfma_f32_16x16x32_bf16 / _f16 in gemm.hip, gemm_split.hip and
    ff_fused.hip: kstep = 32; mfma_f32_32x32x16_f16 in attention_split.hip: kstep = 16).  Inside its own instruction a product meets
    at most kstep - 1 additions, in whatever order the hardware takes them (no assumption about the instruction's internals beyond
    float32-or-better adds); afterwards the accumulator it sits in is added to once per LATER instruction of the chain, at most
    ceil(n_products / kstep) of them (all of a tile's instructions run through ONE accumulator register per output element: see the
    acc[i][j] = mfma(.., acc[i][j]) loops); the split-K / fix-up reduction adds at most ``slices`` partial sums on top."""
    return (kstep - 1) + -(-n_products // kstep) + slices


def accumulate_bound(abs_dot, K, c=2.0, height=None):
    """float32 accumulation of K exact products.  A sum evaluated along ANY tree has error <= h 2^-24 sum |a_k w_k| to first order,
    h = the largest number of additions one term passes through.  ``height`` gives h for kernels whose K loop is known (mfma_height);
    without it the order is taken as unknown: h = K - 1 <= K (a serial chain, which is what the exact float32 FMA kernel and a CPU
    library may do).  c = 2 covers matrix-core adds that do not round to nearest (truncation: one whole ulp = 2 u per add).

    Why float32 OUTPUTS still sit well under the bound (|err| / bound of a few 0.01 on random data, even with ``height``): the bound
    is in terms of sum |a_k w_k|, which is what a worst-case sign pattern needs; with random signs the partial sums are ~sqrt(K)
    instead of ~K of a product's size (a factor 1/20 at K = 640) and the h roundings add like sqrt(h).  Neither is a property of the
    kernel, so neither may be used; what ``height`` removes is the part that IS one (3840 -> 214 additions at K = 640 for the split
    kernels), enough for a fragment that loses float32 precision to stand out (tests/test_parity_cpu.py)."""
    return _on("accumulate") * c * (K if height is None else height) * U_F32 * abs_dot


def gemm_bound(ref_acc, abs_dot, K, out_dtype, alpha=1.0, extras=(), act=None, product_err=None, height=None):
    """Bound for ``store(act(alpha * (A @ W^T) + sum(extras)))`` of the 16-bit kernels (and the exact float32 kernel).

    ref_acc: float64 A @ W^T; abs_dot: float64 |A| @ |W|^T (conv3x3: |x| convolved with |w|, K = 9 Cin); extras: the float64 terms
    the epilogue adds (bias, rowbias, residual, broadcast to the output's shape).  Products of two bf16 / f16 values are exact in
    float32 (8 + 8 / 11 + 11 significand bits <= 24), so the errors are
      * float32 accumulation: accumulate_bound (c = 2), scaled by |alpha| -- along the kernel's K loop when ``height`` (mfma_height)
        is given, in an unknown order (h = K) otherwise;
      * product_err (optional): a per-element bound of the products' own error, for the float32-split types (split_product_bound);
        for exact float32 operands each product rounds once: pass U_F32 * abs_dot;
      * the float32 epilogue: one rounding for alpha * acc and one per added term, each of a partial sum bounded by the sum of the
        magnitudes: (1 + len(extras)) 2^-24 (|alpha acc| + sum |extra|);
      * activation and the one rounding of the stored value: _finish.
    For GEGLU use geglu_bound on the two halves."""
    value, e = preact_bound(ref_acc, abs_dot, K, alpha, extras, product_err, height)
    return _finish(value, e, out_dtype, act)


def preact_bound(ref_acc, abs_dot, K, alpha=1.0, extras=(), product_err=None, height=None):
    """(exact pre-activation value, bound of the float32 value the kernel holds before the activation): see gemm_bound."""
    ref_acc, abs_dot = ref_acc.to(torch.float64), abs_dot.to(torch.float64)
    value = alpha * ref_acc
    mag = value.abs()
    for t in extras:
        value = value + t.to(torch.float64)
        mag = mag + t.to(torch.float64).abs()
    e = abs(alpha) * accumulate_bound(abs_dot, K, height=height)
    if product_err is not None:
        e = e + abs(alpha) * product_err
    e = e + _on("epilogue") * (1 + len(extras)) * U_F32 * (mag + e)
    return value, e


def geglu_bound(val, e_val, gate, e_gate, out_dtype):
    """h * gelu(g) by the product rule: |d(h f(g))| <= |f(g)| e_h + |h| (L e_g + eval(g)) + e_h (L e_g + eval(g)), then one float32
    rounding of the product and the rounding of the stored value."""
    dg = LIP_GELU * e_gate + act_eval_error(gate, "gelu")
    out = val * F.gelu(gate)
    e = F.gelu(gate).abs() * e_val + val.abs() * dg + e_val * dg
    e = e + U_F32 * (out.abs() + e)
    return e + unit_roundoff(out_dtype) * (out.abs() + e) + _TINY[out_dtype]


def split_parts(x):
    """The float32-split representation (include/gmd_hip.h): hi = f16(x), lo = f16(x - hi), both returned as float32."""
    x = x.to(torch.float32)
    hi = x.to(torch.float16).to(torch.float32)
    lo = (x - hi).to(torch.float16).to(torch.float32)
    return hi, lo


def unsplit(t):
    """Read a float32 tensor stored in the pre-split activation layout (GMD_F32SA, include/gmd_hip.h) back as float64 hi + lo: every
    32-element chunk of a row is [hi 64 B | lo 64 B] of float16; inside each half, 16-byte piece q holds elements
    {4q .. 4q+3, 16+4q .. 16+4q+3}.  What a contraction reads from it: the value up to the split's own residual
    (<= 2^-22 |x| + 2^-25, see split_product_bound)."""
    C = t.shape[-1]
    h = t.contiguous().view(torch.float16).reshape(-1, C // 32, 2, 4, 2, 4).to(torch.float64)  # [row, chunk, hi|lo, q, low|high 16, 4]
    v = h[:, :, 0] + h[:, :, 1]                                                             # [row, chunk, q, half, 4]
    return v.permute(0, 1, 3, 2, 4).reshape(t.shape)                                       # element = 16 half + 4 q + j


def split_store(x):
    """float32 [..., C] (C % 32 == 0) -> the same values in the pre-split activation layout, held in a float32 tensor of the same shape:
    the inverse of ``unsplit`` up to the split's residual (what gmd_store_split4 / gmd_split_weights write)."""
    hi, lo = split_parts(x)
    C = x.shape[-1]
    h = torch.stack([hi, lo], 0).to(torch.float16).reshape(2, -1, C // 32, 2, 4, 4)  # [hi|lo, row, chunk, low|high 16, q, 4]
    return h.permute(1, 2, 0, 4, 3, 5).contiguous().view(-1).view(torch.float32).reshape(x.shape)


def presplit_read_bound(ref64, bound64):
    """Bound of a result that was stored pre-split and read back through ``unsplit``: the bound of the float32 value v the kernel held
    (|v - ref| <= bound) plus the split's own residual |v - (hi + lo)| <= 2^-22 |v| + 2^-25 (r_x of split_product_bound), with
    |v| <= |ref| + bound."""
    return bound64 + 2.0 ** -22 * (ref64.abs() + bound64) + 2.0 ** -25


def split_layout_violations(t):
    """Mask of the elements of a pre-split tensor (layout: see ``unsplit``) whose two halves are not a split: hi = f16(x) and
    lo = f16(x - hi) give, for ANY x in float16's range,
        |lo| <= 2^-11 |hi| (1 + 2^-10) + 2^-24
    (round to nearest: |x - hi| <= half a unit in the last place of hi = 2^-11 2^e <= 2^-11 |hi| for a normal hi in [2^e, 2^(e+1));
    lo rounds that difference once: a factor 1 + 2^-11; a subnormal hi has spacing 2^-24).  ``unsplit`` reads hi + lo, which
    does not change when the two halves trade places -- a store that puts lo where hi belongs (or the halves of two different
    pieces together) is invisible to a value check and is caught here: the swapped pair has |"lo"| = |hi| 2^11."""
    C = t.shape[-1]
    h = t.contiguous().view(torch.float16).reshape(-1, C // 32, 2, 4, 2, 4).to(torch.float64)
    hi, lo = h[:, :, 0], h[:, :, 1]
    bad = ~torch.isfinite(hi) | ~torch.isfinite(lo) | (lo.abs() > 2.0 ** -11 * hi.abs() * (1 + 2.0 ** -10) + 2.0 ** -24)
    return bad.permute(0, 1, 3, 2, 4).reshape(t.shape)


def im2col3x3(x, B, H, W, stride=1, upsample=False, pad_mode=0, out_size=None):
    """The explicit [B Ho Wo, 9 C] operand of conv3x3 as the implicit-GEMM kernels walk it (include/gmd_hip.h, gmd_conv3x3): x is
    [B, H W, C] channels-last, column k = tap * C + c with tap = 3 ky + kx, rows of ZEROS where a tap falls into the padding.  Modes:
    stride 1 / 2 with padding 1; ``pad_mode=1``: stride 2 over the map padded by one row / column at the bottom / right only
    (diffusers' Downsample2D with padding 0); ``upsample``: the nearest-2x image; ``out_size=(Ho, Wo)``: the nearest image of that
    size, each side 2 in - 1 or 2 in (source index = destination >> 1 in both: for 2 in - 1, floor(d in / (2 in - 1)) = d >> 1 for every
    d < 2 in - 1).  Pure indexing: the values are x's own, so the GEMM bounds apply to (im2col(x), w) unchanged.  Returns (matrix, Ho, Wo)."""
    C = x.shape[-1]
    xi = x.reshape(B, H * W, C)
    if out_size is not None or upsample:
        hv, wv = (int(out_size[0]), int(out_size[1])) if out_size is not None else (2 * H, 2 * W)
        ho, wo, st, lo, up = hv, wv, 1, 1, True
    elif pad_mode == 1:
        hv, wv, ho, wo, st, lo, up = H, W, (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1, 2, 0, False
    else:
        hv, wv, ho, wo, st, lo, up = H, W, (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1, stride, 1, False
    oy = torch.arange(ho, device=x.device).view(ho, 1, 1, 1)
    ox = torch.arange(wo, device=x.device).view(1, wo, 1, 1)
    ky = torch.arange(3, device=x.device).view(1, 1, 3, 1)
    kx = torch.arange(3, device=x.device).view(1, 1, 1, 3)
    vy, vx = oy * st + ky - lo, ox * st + kx - lo                        # position in the (virtual) image the taps walk
    inside = (vy >= 0) & (vy < hv) & (vx >= 0) & (vx < wv)
    sy, sx = (vy >> 1, vx >> 1) if up else (vy, vx)
    idx = torch.where(inside, sy * W + sx, torch.full_like(sy * W + sx, H * W)).reshape(ho * wo * 9)  # H W = the zero row appended below
    xz = torch.cat([xi, torch.zeros(B, 1, C, dtype=x.dtype, device=x.device)], 1)
    return xz[:, idx].reshape(B * ho * wo, 9 * C), ho, wo


def split_matmul_emulation(a, w):
    """a @ w^T as the split kernels compute it: three float32-accumulated products of float16 halves."""
    ah, al = split_parts(a)
    wh, wl = split_parts(w)
    return ah @ wh.T + (ah @ wl.T + al @ wh.T)


def split_product_bound(a, w):
    """Per-output bound of the three-product scheme's own error, sum_k |a_k w_k - (ah wh + ah wl + al wh)_k| (float64 [M, N]).

    x = hi + lo + r.  |x - hi| <= 2^-11 |x| and lo rounds that difference to float16: in the normal range |r| <= 2^-11 2^-11 |x| =
    2^-22 |x|.  When |x - hi| < 2^-14 (the smallest normal float16) lo is subnormal with spacing 2^-24: |r| <= 2^-25 ABSOLUTE,
    whatever |x|; that happens whenever |x| < 2^-3 (then 2^-11 |x| < 2^-14) -- the reason scale_weight exists -- and the same term
    covers values whose hi is itself subnormal.  So |r_x| <= 2^-22 |x| + 2^-25 [|x| < 2^-3].
    a w - (ah wh + ah wl + al wh) = al wl + r_a w + (ah + al) r_w, with |al| <= 2^-11 |a|, |wl| <= 2^-11 |w|:
        <= 2^-22 |a||w|  (dropped lo lo)  +  |r_a| |w|  +  |a| |r_w|
        <= 3 2^-22 |a||w| + 2^-25 ([|a| < 2^-3] |w| + |a| [|w| < 2^-3]).
    The partial products are exact in float32 (11 + 11 bits); their 3 K terms are accumulated in float32: callers pass K' = 3 K to
    the accumulation term by handing ``3 * K`` to gemm_bound."""
    a64, w64 = a.to(torch.float64).abs(), w.to(torch.float64).abs()
    sa, sw = (a64 < 2.0 ** -3).to(torch.float64), (w64 < 2.0 ** -3).to(torch.float64)
    return _on("split_rel") * 3 * 2.0 ** -22 * (a64 @ w64.T) + _on("split_abs") * 2.0 ** -25 * (sa @ w64.T + a64 @ sw.T)


# ---------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------
def attention_bound(q, k, v, scale, dtype, causal=False, q_rounded=None):
    """Bound for O = softmax(scale Q K^T) V of the flash kernels (csrc/attention.hip), per head: q [.., Nq, D], k, v [.., Nk, D] (the
    16-bit values, any float dtype).  Returns (float64 reference, float64 bound).

    16-bit roundings the kernels perform (u = unit roundoff of ``dtype``), counted in csrc/attention.hip:
      1. P = 2^(score - stabiliser) is packed to 16 bits before the P V product (Half::pack2 of st[][]): every p_j carries u relative.
         The numerator sum_j p_j v_j moves by <= u sum_j p_j |v_j|; the row sum (taken on the matrix core from the SAME rounded P where
         a spare V^T row exists, from the unrounded p otherwise) by <= u relative, which moves O by u |O| <= u (P |V|): 2 u (P |V|);
      2. the output is rounded once when stored: u |O| <= u (P |V|).
         => c = 3 on (P_ref @ |V|).
      3. the lagged-stabiliser kernels (head dims with a spare K column, e.g. 40 -- "attn40") fold scale log2(e) into Q and round Q
         to 16 bits again: score_ij moves by d_ij <= u scale sum_d |q_id| |k_jd|.  The stabiliser itself is kept representable and
         is subtracted exactly (it cancels between numerator and row sum: no term).  A perturbed score multiplies p_j by
         exp(d_j): to first order O moves by sum_j p_j d_j |v_j| + |O| sum_j p_j d_j, and the second order is covered by the
         factor exp(2 max_j d_ij).  ``q_rounded`` (default: D % 16 != 0, the condition of kLagged = spare V^T row AND spare K column; 40 among
         the instantiated head dims) switches the 16-bit part of d on; the classic kernels scale the float32 scores and carry only its float32 part.
      float32 terms: the score accumulation (D products, 2 D 2^-24 of sum |q||k| scale: added to d_ij), exp2 (1 ulp), the per-tile
      rescale of the accumulator (3 roundings per 64-key tile) and the P V accumulation (unknown order, c = 2):
      (2 Nk + 3 ceil(Nk / 64) + 8) 2^-24 (P |V|).
      float16 only: p below 2^-14 is subnormal in float16 (absolute error 2^-25 per key against a row sum >= 1/2 after
      stabilisation): 2^-24 sum_j |v_j|."""
    u = unit_roundoff(dtype)
    q64, k64, v64 = q.to(torch.float64), k.to(torch.float64), v.to(torch.float64)
    Nq, Nk, D = q64.shape[-2], k64.shape[-2], q64.shape[-1]
    s = (q64 @ k64.transpose(-1, -2)) * scale
    sabs = (q64.abs() @ k64.abs().transpose(-1, -2)) * abs(scale)
    if causal:
        mask = torch.ones(Nq, Nk, dtype=torch.bool, device=s.device).tril()
        s = s.masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, -1)
    vabs = v64.abs()
    ref = p @ v64
    pv = p @ vabs
    if q_rounded is None:
        q_rounded = D % 16 != 0  # kLagged of csrc/attention.hip: a spare K column (D % 16 != 0) and with it a spare V^T row
    d = ((u * _on("attn_q_round") if q_rounded else 0.0) + 2 * D * U_F32 + 4 * U_F32) * sabs
    if causal:
        d = d.masked_fill(~mask, 0.0)
    pd = p * d
    second = torch.exp(2 * d.amax(-1, keepdim=True))
    score_term = (pd @ vabs + pd.sum(-1, keepdim=True) * pv) * second
    bound = (2 * _on("attn_p_round") + _on("out_round")) * u * pv + score_term + (2 * Nk + 3 * math.ceil(Nk / 64) + 8) * U_F32 * pv + _TINY[dtype]
    if dtype == torch.float16:
        bound = bound + 2.0 ** -24 * vabs.sum(-2, keepdim=True)
    return ref, bound


def attention_split_bound(q, k, v, scale):
    """Bound for the float32 flash kernel (csrc/attention_split.hip): both contractions as three float16 products (see
    split_product_bound), classic online softmax in float32, float32 output.  q, k, v: float32 values [.., N, D].
      scores: the split's own error 3 2^-22 scale sum |q||k| + 2^-25 scale ([|q| < 2^-3] |k| + |q| [|k| < 2^-3]) plus the float32
              accumulation of 3 D products (c = 2) and the scaling / exp2 (4 2^-24): the perturbation d_ij, propagated through the
              softmax exactly as in attention_bound;
      P V:    P is carried as 2^11 p and split: 2^-22 relative while p >= 2^-14 of the row maximum, 2^-36 absolute per key below
              that; V splits with 2^-22 |v| + 2^-25 [|v| < 2^-3]; the dropped lo lo product 2^-22: 3 2^-22 (P |V|) + 2^-25 + 2^-36 sum |v_j|;
              accumulation along the kernel's loops (mfma_height, kstep = 16: 3 D products per score, 3 Nk products per output
              element plus one rescale multiplication per 64-key tile; c = 2), the row sum (a lane adds its 32 probabilities of a
              tile serially, then one multiply and one add per later tile, then the half-wave swap: 34 + 2 tiles additions of
              positive terms), the final division and store (8).
    On random inputs the observed error stays at 0.01-0.02 of this bound (measured on the MI355X: 0.014 at most): the reason is the
    one given at accumulate_bound -- worst-case signs against random ones -- and not slack in the counted additions."""
    q64, k64, v64 = q.to(torch.float64), k.to(torch.float64), v.to(torch.float64)
    Nk, D = k64.shape[-2], q64.shape[-1]
    s = (q64 @ k64.transpose(-1, -2)) * scale
    qa, ka, va = q64.abs(), k64.abs(), v64.abs()
    sabs = (qa @ ka.transpose(-1, -2)) * abs(scale)
    sq, sk = (qa < 2.0 ** -3).to(torch.float64), (ka < 2.0 ** -3).to(torch.float64)
    p = torch.softmax(s, -1)
    ref, pv = p @ v64, p @ va
    nt = math.ceil(Nk / 64)
    d = (3 * 2.0 ** -22 + (2 * mfma_height(3 * D, 16) + 4) * U_F32) * sabs + 2.0 ** -25 * abs(scale) * (sq @ ka.transpose(-1, -2) + qa @ sk.transpose(-1, -2))
    pd = p * d
    score_term = (pd @ va + pd.sum(-1, keepdim=True) * pv) * torch.exp(2 * d.amax(-1, keepdim=True))
    bound = score_term + (3 * 2.0 ** -22 + (2 * mfma_height(3 * Nk, 16, nt) + 34 + 2 * nt + 8) * U_F32) * pv + 2.0 ** -25 + 2.0 ** -36 * va.sum(-2, keepdim=True)
    return ref, bound


# ---------------------------------------------------------------------------------------------------------------------------
# GroupNorm / LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------
def norm_bound(x, mean, var, gamma, beta, eps, out_dtype, height, absmean, sqmean, silu=False):
    """Bound for ``store([silu]((x - mean) rstd gamma + beta))`` with float32 statistics (csrc/norm.hip); all arguments float64 and
    broadcastable to x: ``mean`` / ``var`` the exact statistics of the element's group (row), ``absmean`` = mean |x|, ``sqmean`` =
    mean x^2 over the same set.

    height: the largest number of float32 additions any one element passes through in the kernel's reduction (per-thread serial
    chain + tree stages; the cross-workgroup folds run in double).  A sum of n terms evaluated along any tree of that height has
    error <= height 2^-24 sum |x_i|, so with g = (height + 2) 2^-24 (the + 2: the squaring's rounding and the float32 store of a
    partial sum):
        d_mean <= g mean|x|;   d_var <= g mean(x^2) + 2 |mean| d_mean + d_mean^2   (the E[x^2] - mean^2 form of the split path; the
        two-pass kernels are at most this);   rstd = (var + eps)^-1/2:  d_rstd / rstd <= d_var / (2 (var + eps)) (1 + d_var / (var + eps)) + 2 2^-24.
    Propagated through y = (x - mean) rstd gamma + beta:
        |d y| <= |gamma| rstd d_mean + |x - mean| rstd |gamma| (d_rstd / rstd)
                 + 4 2^-24 (|x| + |mean|) rstd |gamma| + 2 2^-24 |beta|       (float32 evaluation as x * scale + shift, scale = rstd gamma,
                                                                            shift = beta - mean scale: four roundings of terms of that size)
    then SiLU (Lipschitz constant, evaluation error) and u_out |result| from _finish."""
    g = _on("norm_stats") * (height + 2) * U_F32
    d_mean = g * absmean
    d_var = g * sqmean + 2 * mean.abs() * d_mean + d_mean ** 2
    rstd = (var + eps).rsqrt()
    rel_rstd = d_var / (2 * (var + eps)) * (1 + d_var / (var + eps)) + 2 * U_F32
    ga = gamma.abs()
    value = (x - mean) * rstd * gamma + beta
    e = ga * rstd * d_mean + (x - mean).abs() * rstd * ga * rel_rstd + _on("norm_eval") * (4 * U_F32 * (x.abs() + mean.abs()) * rstd * ga + 2 * U_F32 * beta.abs())
    return _act_ref(value, "silu" if silu else None), _finish(value, e, out_dtype, "silu" if silu else None)


def groupnorm_ref_bound(x, G, gamma, beta, eps, out_dtype, height, silu=False):
    """x: [B, HW, C] (stored values, any float dtype) -> (float64 reference, float64 bound), statistics per (sample, group)."""
    B, HW, C = x.shape
    x64 = x.to(torch.float64).reshape(B, HW, G, C // G)
    mean = x64.mean((1, 3), keepdim=True)
    var = ((x64 - mean) ** 2).mean((1, 3), keepdim=True)
    ga = gamma.to(torch.float64).reshape(1, 1, G, C // G)
    be = beta.to(torch.float64).reshape(1, 1, G, C // G)
    ref, b = norm_bound(x64, mean, var, ga, be, eps, out_dtype, height, x64.abs().mean((1, 3), keepdim=True),
                        (x64 ** 2).mean((1, 3), keepdim=True), silu)
    return ref.reshape(B, HW, C), b.reshape(B, HW, C)


def layernorm_ref_bound(x, gamma, beta, eps, out_dtype, height):
    x64 = x.to(torch.float64)
    mean = x64.mean(-1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(-1, keepdim=True)
    return norm_bound(x64, mean, var, gamma.to(torch.float64), beta.to(torch.float64), eps, out_dtype, height,
                      x64.abs().mean(-1, keepdim=True), (x64 ** 2).mean(-1, keepdim=True), False)
