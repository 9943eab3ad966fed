"""Float64 restatement of the two resampling definitions of csrc/resample.hip and the per-element bounds of their tests (plain
helper module, like tests/parity.py).  Everything is exact-integer weights turned into float64 matrices: ``resize(x, Wy, Wx)`` is
``Wy @ x @ Wx^T`` over the two spatial axes, and nothing here uses the library.

Definitions (per axis, output index i, n_in -> n_out):
  bilinear (half-pixel centres, edge clamp; cv2.INTER_LINEAR on float32 = F.interpolate(mode="bilinear", align_corners=False)):
      num = max((2i+1) n_in - n_out, 0), den = 2 n_out, i0 = num // den, lam = (num - i0 den) / den, i1 = min(i0 + 1, n_in - 1)
      row i of the matrix: (1 - lam) at i0, + lam at i1
  antialiased triangle (PIL Image.resize(BILINEAR) / F.interpolate(mode="bilinear", antialias=True)):
      n_in >= n_out: tap j weighs max(0, 2 n_in - |(2j+1) n_out - (2i+1) n_in|), normalised by the integer sum over the in-range taps;
      n_in <  n_out: the bilinear row above.
"""
import numpy as np
import torch

U_F32 = 2.0 ** -24
U_OUT = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def bilinear_matrix(n_in, n_out):
    """float64 [n_out, n_in]; at most two non-zeros per row."""
    m = np.zeros((n_out, n_in), np.float64)
    for i in range(n_out):
        num = max((2 * i + 1) * n_in - n_out, 0)
        den = 2 * n_out
        i0 = num // den
        r = num - i0 * den
        i1 = min(i0 + 1, n_in - 1)
        m[i, i0] += (den - r) / den
        m[i, i1] += r / den
    return torch.from_numpy(m)


def bilinear_taps(n_in, n_out):
    """(i0, i1) index tensors [n_out] of the bilinear definition."""
    i = np.arange(n_out, dtype=np.int64)
    i0 = np.maximum((2 * i + 1) * n_in - n_out, 0) // (2 * n_out)
    return torch.from_numpy(i0), torch.from_numpy(np.minimum(i0 + 1, n_in - 1))


def antialias_matrix(n_in, n_out):
    """float64 [n_out, n_in]: integer numerators over their integer row sums."""
    if n_in < n_out:
        return bilinear_matrix(n_in, n_out)
    j = np.arange(n_in, dtype=np.int64)[None, :]
    i = np.arange(n_out, dtype=np.int64)[:, None]
    num = np.maximum(0, 2 * n_in - np.abs((2 * j + 1) * n_out - (2 * i + 1) * n_in))
    return torch.from_numpy(num.astype(np.float64) / num.sum(1, keepdims=True).astype(np.float64))


def resize(x, wy, wx):
    """x: [..., h, w] (any dtype) -> float64 [..., H, W] = wy @ x @ wx^T."""
    x = x.to(torch.float64)
    return torch.einsum("yh,...hw,xw->...yx", wy.to(x.device), x, wx.to(x.device))


def denorm(x):
    """clamp(x/2 + 0.5, 0, 1) in float64.  On float32 / bf16 / f16 inputs the float32 evaluation is exact up to ONE rounding of the sum
    (x/2 is exact), which the bilinear bound's count includes."""
    return (x.to(torch.float64) / 2 + 0.5).clamp(0, 1)


def bilinear_ref_bound(dec_nchw, H, W):
    """Reference and bound of one resampled operand of gmd_hdr_tail_resized.  dec_nchw: decoder output [B,3,h,w] (stored values).
    Returns float64 ([B,H,W,3] reference, [B,H,W,3] bound).

    Bound 16 * 2^-24 * M, M = the largest of the four taps (u = 2^-24, taps p in [0, 1], weights in [0, 1]):
      * a tap p = clamp01(x/2 + 0.5): x/2 is exact, the sum rounds once: u M per tap;
      * a one-axis weight: lam = fl(r / den) is within u (both conversions exact, one division), 1 - lam rounds once more: every
        weight is within 2u ABSOLUTE of the exact one;
      * inner pair (1-lx) p00 + lx p01, counted generously as seven roundings of values <= M: the two taps' own (2), two weight
        errors of <= 2u each against taps <= M (counted 2: the pair's weights sum to 1, so at most 2u M + u M in all), two products
        and one sum (3): 7 u M -- the same for the other row; the outer combination weighs the two inner values by (1-ly) and ly,
        which sum to 1, so the inner error enters ONCE;
      * outer: the two weight errors against inner values <= M, counted at their full 2u each (4 u M), two products and one sum (3 u M).
      total (7 + 4 + 3) u M = 14 u M <= 16 u M; the remaining 2 u M cover the second-order terms.
    When lam = 0 on both axes the kernel's value is the tap itself (error: the tap's one rounding)."""
    _, _, h, w = dec_nchw.shape
    p = denorm(dec_nchw)
    wy, wx = bilinear_matrix(h, H), bilinear_matrix(w, W)
    ref = resize(p, wy, wx)
    y0, y1 = bilinear_taps(h, H)
    x0, x1 = bilinear_taps(w, W)
    m = torch.stack([p[:, :, ys][:, :, :, xs] for ys in (y0, y1) for xs in (x0, x1)], 0).amax(0)  # [B,3,H,W]: the largest of the four taps
    return ref.permute(0, 2, 3, 1).contiguous(), (16 * U_F32 * m).permute(0, 2, 3, 1).contiguous()


def eq1_ref(s, g, q, eps=1 / 64):
    return (s.clamp(0, 1) ** 2.2 + eps) * (1 + g * q) - eps


def hdr_bound(s, g, e_sdr, e_gm, q, eps=1 / 64):
    """Bound of hdr = (s^2.2 + eps)(1 + g q) - eps at the float64 reference operands s, g whose kernel values are within e_sdr, e_gm:
    d hdr/d g = q (lin + eps), d hdr/d s = 2.2 s^1.2 (1 + g q) (first order; s^1.2 is evaluated at s + e_sdr, the derivative's
    largest value on the interval, which makes the term rigorous), plus the project's own allowance for the float32 evaluation of
    Eq. 1 (powf, four operations), 4e-6 (q + 1) (tests/test_kernels_gpu.py).  hdr_file = hdr / (q + 1): the same bound over q + 1."""
    lin = s.clamp(0, 1) ** 2.2
    return q * (lin + eps) * e_gm + 2.2 * (s + e_sdr).clamp(0, 1) ** 1.2 * (1 + g * q) * e_sdr + 4e-6 * (q + 1)


def prepare_ref_bound(u8_bhwc, H, W, out_dtype):
    """Reference and bound of gmd_prepare_sdr.  u8_bhwc: uint8 [B,h,w,3].  Returns float64 ([B,3,H,W] reference, bound).

    Bound 2 (Kx + Ky + 8) 2^-24 + u_out |value|, K = the number of non-zero taps of the output's row / column, from the kernel's
    summation order (codes c in [0, 255], integer weight numerators n, integer sums s; u = 2^-24):
      * row value R = fl(A / fl(sx)), A = sum_j fl(nx_j) c_j accumulated in float32: every nx_j (<= 2^15) and every product
        (< 2^23) is exact, each of the Kx - 1 additions rounds only when the partial sum passes 2^24 (<= u A each), the conversion of
        sx and the division round once each: |R - exact| <= (Kx + 1) u * 255;
      * column value T = fl(sum_j fl(ny_j) R_j / fl(sy)): Ky product roundings that pass through weights summing to 1 (1 u), Ky - 1
        additions, the conversion of sy and the division: (Ky + 2) u * 255, plus the rows' error once (the weights sum to 1):
        |T - exact| <= (Kx + Ky + 3) u * 255;
      * v = fl(T / 255): (Kx + Ky + 3) u + u;   v - 0.5: one rounding of a value <= 1/2 (u / 2);   / 0.5 is exact and doubles it:
        2 (Kx + Ky + 4.5) u <= 2 (Kx + Ky + 8) u, the slack covering the second-order terms and sums beyond 2^24 (sides above ~4096
        shrunk by more than 16x);
      * ONE rounding to the output type: u_out |value| (float32 output: that rounding is the store of v itself, already counted)."""
    B, h, w, _ = u8_bhwc.shape
    wy, wx = antialias_matrix(h, H), antialias_matrix(w, W)
    x = u8_bhwc.permute(0, 3, 1, 2).to(torch.float64)
    ref = (resize(x, wy, wx) / 255 - 0.5) / 0.5
    ky = (wy > 0).sum(1).to(torch.float64)[:, None]
    kx = (wx > 0).sum(1).to(torch.float64)[None, :]
    bound = 2 * (kx + ky + 8) * U_F32 + U_OUT[out_dtype] * ref.abs()
    return ref, bound
