"""References for FreeU (plain helper module, like tests/lora_ref.py): diffusers' ``fourier_filter`` restated with ``torch.fft`` in
float64, the closed form the HIP kernel evaluates, the oracle UNet with FreeU hooked in front of the resnets of up blocks 0 and 1, a
CPU emulation of the kernel's arithmetic, and the DERIVED per-element bound of one FreeU site.

diffusers (``UNet2DConditionModel.enable_freeu`` -> ``apply_freeu`` in every up block whose ``resolution_idx`` is 0 or 1, in front of
each resnet):

    hidden[:, :C_h // 2] = hidden[:, :C_h // 2] * b_i
    res = fourier_filter(res, threshold=1, scale=s_i)
    x = cat([hidden, res], dim=1)

``fourier_filter``: fftn -> fftshift -> mask -> ifftshift -> ifftn -> .real in float32; the mask is ``scale`` on the shifted bins
``[H//2 - 1 : H//2 + 1, W//2 - 1 : W//2 + 1]`` and 1 elsewhere.  The zero frequency sits at shifted index H//2, so the masked bins are
the frequencies {0, -1} x {0, -1}; an axis of length 1 holds {0} alone (the slice -1:1 on length 1 is 0:1), an axis of length 2 both of
its bins.  The set holds -1 without +1: it is not conjugate-symmetric, which is why diffusers takes ``.real``.
"""
import copy
import math

import torch

import parity as P

# error of one entry of the kernel's cos / sin tables and of the mixed-bin products formed from them, in units of 2^-24 (see
# site_ref_bound)
TABLE_ULPS = 12.0
PIX_LANES = 32  # csrc/freeu.hip kPixLanes: the pixel-strided threads of one vector column


def bin_set(H, W):
    """The masked frequencies as (u, v) with u, v in {0, 1} standing for {0, -1}: u = 1 only for H > 1, v = 1 only for W > 1."""
    return [(u, v) for u in ((0, 1) if H > 1 else (0,)) for v in ((0, 1) if W > 1 else (0,))]


def fourier_filter64(x, scale, threshold=1):
    """diffusers' fourier_filter on x [..., H, W], in float64 (independent of the closed form: torch.fft)."""
    x = x.to(torch.float64)
    f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    H, W = x.shape[-2:]
    mask = torch.ones(x.shape, dtype=torch.float64)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    f = torch.fft.ifftshift(f * mask, dim=(-2, -1))
    return torch.fft.ifftn(f, dim=(-2, -1)).real


def _phases(H, W):
    th = 2 * math.pi * torch.arange(H, dtype=torch.float64) / H
    ph = 2 * math.pi * torch.arange(W, dtype=torch.float64) / W
    return th[:, None], ph[None, :]


def closed_form64(x, scale, bins=None):
    """X + (scale - 1) low, low = 1/(HW) sum_{(u,v)} (c_uv cos(u th + v ph) + d_uv sin(u th + v ph)) on x [..., H, W], float64.
    ``bins``: the (u, v) frequency pairs to sum over (default: bin_set), for the deliberately wrong variants of the CPU test."""
    x = x.to(torch.float64)
    H, W = x.shape[-2:]
    th, ph = _phases(H, W)
    low = torch.zeros_like(x)
    for u, v in (bin_set(H, W) if bins is None else bins):
        a = u * th + v * ph
        c = (x * a.cos()).sum((-2, -1), keepdim=True)
        d = (x * a.sin()).sum((-2, -1), keepdim=True)
        low = low + c * a.cos() + d * a.sin()
    return x + (scale - 1.0) * low / (H * W)


def apply_freeu(hidden, res, b, s):
    """One site on NCHW tensors: (hidden with its first half of channels scaled by b, the filtered skip), in the inputs' dtype."""
    hidden = hidden.clone()
    half = hidden.shape[1] // 2
    hidden[:, :half] = hidden[:, :half] * b
    return hidden, fourier_filter64(res, s).to(res.dtype)


def hooked_oracle(ou, s1, s2, b1, b2):
    """A deep copy of the oracle UNet with a forward_pre_hook on each resnet of up_blocks[0] and up_blocks[1]: the concatenated input
    is split at the backbone width (the previous resnet's output channels; for the first resnet of a block the previous block's or
    the mid block's), ``apply_freeu`` runs with (b1, s1) / (b2, s2), and the parts are concatenated again."""
    m = copy.deepcopy(ou)
    width = m.mid_block.resnets[-1].conv2.out_channels
    for i, blk in enumerate(m.up_blocks):
        for r in blk.resnets:
            if i < 2:
                b, s = ((b1, s1), (b2, s2))[i]

                def pre(mod, args, width=width, b=b, s=s):
                    x = args[0]
                    h, res = apply_freeu(x[:, :width], x[:, width:], b, s)
                    return (torch.cat([h, res], dim=1),) + tuple(args[1:])

                r.register_forward_pre_hook(pre)
            width = r.conv2.out_channels
    return m


def _f32(v):
    return torch.tensor(v, dtype=torch.float64).to(torch.float32)


def emulate_site(S, B, H, W, s, dtype, bins=None):
    """The kernel's arithmetic on the skip S [B*H*W, Cs] (values of ``dtype``), in float32 torch on the CPU: per pixel lane (pixel p
    goes to lane p % 32) the products are added serially in pixel order, the 32 lanes serially, lane 0 first; the correction is
    g c_00 + sum_k w_k c_k with g = (s - 1) / HW and w_k = g t_k, added to x, rounded ONCE to ``dtype``.  The tables are the float64
    cos / sin rounded to float32, the mixed bin (1, 1) formed from products as the kernel does.  ``bins``: other frequency sets (the
    wrong variants); u, v in {-1, 0, 1}."""
    bins = bin_set(H, W) if bins is None else bins
    HW, C = H * W, S.shape[-1]
    X = S.to(torch.float32).reshape(B, HW, C)
    th, ph = _phases(H, W)
    cy, sy, cx, sx = (t.to(torch.float32) for t in (th.cos(), th.sin(), ph.cos(), ph.sin()))

    def table(u, v):
        if (u, v) == (0, 0):
            return [torch.ones(H, W, dtype=torch.float32)]
        if (u, v) == (1, 1):
            return [cy * cx - sy * sx, sy * cx + cy * sx]
        a = u * th + v * ph
        return [a.cos().to(torch.float32), a.sin().to(torch.float32)]

    tabs = [t.expand(H, W).reshape(HW) for u, v in bins for t in table(u, v)]
    n = -(-HW // PIX_LANES)
    pad = n * PIX_LANES - HW
    Xp = torch.cat([X, torch.zeros(B, pad, C)], 1).reshape(B, n, PIX_LANES, C)
    coefs = []
    for t in tabs:
        tp = torch.cat([t, torch.zeros(pad)]).reshape(1, n, PIX_LANES, 1)
        acc = torch.zeros(B, PIX_LANES, C)
        for k in range(n):
            acc = acc + Xp[:, k] * tp[:, k]
        c = torch.zeros(B, C)
        for lane in range(PIX_LANES):
            c = c + acc[:, lane]
        coefs.append(c)
    g = (_f32(s) - 1.0) / _f32(float(HW))
    d = None
    for t, c in zip(tabs, coefs):
        term = (g * t).reshape(1, HW, 1) * c.reshape(B, 1, C)
        d = term if d is None else d + term
    return (X + d).to(dtype).reshape(B * HW, C)


def site_ref_bound(A, S, B, H, W, b, s, dtype):
    """(float64 reference [B*H*W, Ca + Cs], per-element bound) of one FreeU site: A [B*H*W, Ca] and S [B*H*W, Cs] hold values of
    ``dtype``; b and s are the float32 values the kernel reads.  The reference of the skip is ``fourier_filter64`` (torch.fft).

    Backbone: float(a) * b rounds once in float32 (U_F32 |value|), then the one rounding of the store (parity._finish); the second
    half is a copy (bound 0).  b == 1 / s == 1 are raw copies (bound 0).

    Skip, per (sample, channel), with M1 = sum over the pixels of |X| and g = (s - 1) / (H W); u32 = 2^-24:
      1. every coefficient c_k = sum_p X_p t_k(p), |t_k| <= 1: each product rounds once (u32 M1 in all); the sum runs along the
         kernel's tree -- a thread adds its ceil(HW / 32) pixels serially, the 32 pixel lanes are then added serially, so no term
         passes through more than h = ceil(HW / 32) + 32 additions: parity.accumulate_bound(M1, HW, c=1, height=h);
      2. the phase tables: cos / sin of pi m / n with m / n in [0, 1/2] reduced in INTEGERS; the one rounded quotient moves the angle
         by <= pi 2^-26 (0.79 u32), sinpif / cospif are within 2 ulp (2 u32): tau_1 <= 3 u32 per entry; the mixed bin's
         cos(th + ph) = cy cx - sy sx and sin(th + ph) = sy cx + cy sx carry tau_1 (|cy| + |cx| + |sy| + |sx|) <= 2 sqrt 2 tau_1 plus
         three roundings of values <= 1: <= 11.5 u32.  tau = TABLE_ULPS u32 = 12 u32 for every entry.  In pass 1 it moves a coefficient
         by <= tau M1; in pass 2 it moves the n_t - 1 non-constant terms of the correction by <= tau |g| |c_k| <= tau |g| M1 each
         (n_t = 1 + 2 (number of bins - 1) real terms: 7, 3 on a line, 1 on a point);
         => E_c = (h + 1 + 12) u32 M1 per coefficient, reaching the output through |g| sum_k |t_k| E_c <= |g| n_t E_c;
      3. float32 evaluation of the correction: s - 1, the division by HW, w_k = g t_k, w_k c_k round once each and a term passes
         through at most n_t - 1 additions: (n_t + 3) u32 of |g| sum_k |t_k| |c_k| <= |g| n_t M1;
      => E_d = |g| M1 u32 (n_t (h + 13) + 12 (n_t - 1) + n_t (n_t + 3)), times 1.01 for the second-order products of these terms;
      4. x + d rounds once in float32, then ONE rounding of the stored value: parity._finish."""
    u32 = P.U_F32
    b, s = float(_f32(b)), float(_f32(s))
    A64, S64 = A.to(torch.float64), S.to(torch.float64)
    Ca, Cs, HW = A.shape[-1], S.shape[-1], H * W
    # backbone
    ref_a = A64.clone()
    ref_a[:, :Ca // 2] = A64[:, :Ca // 2] * b
    bound_a = torch.zeros_like(A64)
    if b != 1.0:
        v = ref_a[:, :Ca // 2]
        bound_a[:, :Ca // 2] = P._finish(v, u32 * v.abs(), dtype)
    # skip
    X = S64.reshape(B, HW, Cs)
    ref_s = fourier_filter64(X.permute(0, 2, 1).reshape(B, Cs, H, W), s).reshape(B, Cs, HW).permute(0, 2, 1)
    if s == 1.0:
        return torch.cat([ref_a, S64], -1), torch.cat([bound_a, torch.zeros_like(S64)], -1)
    n_t = 1 + 2 * (len(bin_set(H, W)) - 1)
    h = -(-HW // PIX_LANES) + PIX_LANES
    M1 = X.abs().sum(1, keepdim=True)
    g = abs(s - 1.0) / HW
    e_c = P.accumulate_bound(M1, HW, c=1.0, height=h) + (1 + TABLE_ULPS) * u32 * M1
    e_d = 1.01 * g * (n_t * e_c + (TABLE_ULPS * (n_t - 1) + n_t * (n_t + 3)) * u32 * M1)
    d = (ref_s - X).abs()
    e = e_d + u32 * (X.abs() + d + e_d)
    bound_s = P._finish(ref_s, e.expand_as(ref_s) if e.shape != ref_s.shape else e, dtype)
    return torch.cat([ref_a, ref_s.reshape(B * HW, Cs)], -1), torch.cat([bound_a, bound_s.reshape(B * HW, Cs)], -1)
