"""LoRA on the wider target set (``targets="transformer"``): plain helper module beside tests/lora_ref.py, which it reuses by import.
Synthetic adapters over all TWELVE targets of the tiny oracle UNet (the eight attention projections, ff.net.0.proj, ff.net.2,
proj_in, proj_out) in the key conventions, the merged and hooked CPU oracles for that set, the value / gate interleave of the
feed-forward's first projection restated in torch, and the per-element bound of the fused update + GEGLU launch (gmd_lora_geglu)."""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

import lora_ref as R
import parity as P

FF = ("ff.net.0.proj", "ff.net.2")
PROJ = ("proj_in", "proj_out")
FAMILIES = {"attention": R.PROJECTIONS, "ff1": FF[:1], "ff2": FF[1:], "proj_in": PROJ[:1], "proj_out": PROJ[1:]}
CONVENTIONS = ("peft", "diffusers_old", "kohya")  # the processor convention names attention projections only


def target_modules(ou, families=None):
    """{module name: nn.Linear or 1x1 nn.Conv2d} of the twelve targets of every Transformer2DModel of the oracle UNet ``ou`` (or of
    the named ``families`` of FAMILIES only)."""
    suffixes = tuple(s for f in (families or FAMILIES) for s in FAMILIES[f])
    out = {}
    for n, m in ou.named_modules():
        if not n.endswith(suffixes):
            continue
        if isinstance(m, nn.Linear) and (".transformer_blocks." in n or n.endswith(PROJ)):
            out[n] = m
        elif isinstance(m, nn.Conv2d) and n.endswith(PROJ):
            assert m.kernel_size == (1, 1)
            out[n] = m
    return out


def canonical(ou, rank, seed, gain, alpha=None, dtype=torch.float32, families=None):
    """lora_ref.canonical over the wider set: {module: (A [r, K], B [N, r], alpha)} -- always 2-D, a 1x1 convolution counted as the
    matrix it is.  ff.net.0.proj's B is in checkpoint row order (value half, then gate half)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, mod in sorted(target_modules(ou, families).items()):
        n, k = mod.weight.shape[:2]
        a = torch.randn(rank, k, generator=g) / k ** 0.5
        b = gain * torch.randn(n, rank, generator=g) / rank ** 0.5
        out[name] = (a.to(dtype).float(), b.to(dtype).float(), alpha)
    return out


def to_convention(canon, convention, conv_names=()):
    """lora_ref.to_convention; kohya writes the factors of the modules in ``conv_names`` (1x1 convolutions) 4-D, [r, in, 1, 1] and
    [out, r, 1, 1], as kohya / LoCon do."""
    sd = R.to_convention(canon, convention)
    if convention == "kohya":
        for name in conv_names:
            if name in canon:
                flat = "lora_unet_" + name.replace(".", "_")
                for part in ("lora_down", "lora_up"):
                    sd[f"{flat}.{part}.weight"] = sd[f"{flat}.{part}.weight"][:, :, None, None].contiguous()
    return sd


def conv_targets(ou):
    return tuple(n for n, m in target_modules(ou).items() if isinstance(m, nn.Conv2d))


def merged_oracle(ou, canon, scale=1.0):
    """Reference (a): W + s (alpha / r) B A formed in float64 and loaded into a COPY of the oracle (a 1x1 convolution's weight is
    the same matrix with two trailing unit dimensions)."""
    m = copy.deepcopy(ou)
    mods = target_modules(m)
    with torch.no_grad():
        for name, (a, b, alpha) in canon.items():
            w = mods[name].weight
            d = scale * R._factor(a, alpha) * (b.double() @ a.double())
            w.copy_((w.double() + d.reshape(w.shape)).to(w.dtype))
    return m


def hooked_oracle(ou, canon, scale=1.0):
    """Reference (b): the weights untouched; a forward hook on every adapted module adds s (alpha / r) B (A x) -- over the channel
    dimension of an NCHW map for a 1x1 convolution."""
    m = copy.deepcopy(ou)
    mods = target_modules(m)
    for name, (a, b, alpha) in canon.items():
        f = scale * R._factor(a, alpha)
        conv = isinstance(mods[name], nn.Conv2d)

        def hook(mod, inp, out, a=a, b=b, f=f, conv=conv):
            x = inp[0]
            if conv:
                x = x.permute(0, 2, 3, 1)
            u = f * ((x @ a.T.to(x.dtype)) @ b.T.to(x.dtype))
            return out + (u.permute(0, 3, 1, 2) if conv else u)

        mods[name].register_forward_hook(hook)
    return m


# ---------------------------------------------------------------------------------------------------------------------------
# the interleaved layout of the feed-forward's first projection
# ---------------------------------------------------------------------------------------------------------------------------
def interleave_rows(t, group=16):
    """[2F, ...] from [value half | gate half] to value rows 0-15, gate rows 0-15, value rows 16-31, ... (what the UNet does to the
    ff1 weight; restated here, not imported)."""
    half = t.shape[0] // 2
    idx = torch.arange(half).view(half // group, group)
    return t[torch.stack([idx, idx + half], 1).reshape(-1)]


def deinterleave_cols(y, group=16):
    """[M, 2F] in the interleaved column layout -> (value [M, F], gate [M, F])."""
    M, n = y.shape
    y = y.view(M, n // (2 * group), 2, group)
    return y[:, :, 0].reshape(M, n // 2), y[:, :, 1].reshape(M, n // 2)


def geglu_halves(y):
    """GEGLU of diffusers over [value half | gate half]: value * gelu_erf(gate)."""
    v, g = y.chunk(2, dim=-1)
    return v * F.gelu(g)


# ---------------------------------------------------------------------------------------------------------------------------
# the fused launch's per-element bound
# ---------------------------------------------------------------------------------------------------------------------------
def _gelu_erf_eval_error(g):
    """Error of the float32 evaluation 0.5 g (1 + erff(g c)), c = 1 / sqrt 2, at an exact argument g.  The rounded constant and the
    rounded product move the argument z by <= 2 2^-24 |z|, which erf passes on weighted by |z erf'(z)| <= 0.5; the device library's
    erff is taken at 4 ulp of a value <= 1 (8 2^-24; its documented accuracy is tighter); the add rounds a sum <= 2 once (2 2^-24):
    |d (1 + erf)| <= 11 2^-24, an ABSOLUTE error -- for g << 0 the factor itself is far smaller, and the term 0.5 |g| 11 2^-24 is
    what remains.  The two multiplications round once each: 2 2^-24 |gelu(g)|."""
    return 0.5 * g.abs() * 11 * P.U_F32 + 2 * P.U_F32 * F.gelu(g).abs()


def geglu_update_ref_bound(x, a, b, y, s, dtype, route="fused"):
    """(float64 F, per-element bound) of ``geglu(y + s (x a^T) b^T)`` for x [M, C], a [Rp, C], b [8C, Rp] and y [M, 8C] in the
    INTERLEAVED layout, all holding values of ``dtype``; F [M, 4C].  Terms 1-4 are lora_ref.update_ref_bound's (the first product, the
    ONE rounding of T, the second product, the float32 scale), then
      5. v = float(y_v) + s U_v and g = float(y_g) + s U_g: one float32 add each (or none: an FMA); NOT rounded to ``dtype``;
      6. gelu_erf(g) in float32: LIP_GELU e_g + its evaluation error (_gelu_erf_eval_error);
      7. the product, by the product rule, rounds once in float32; then the ONE rounding of the stored value.
    ``route="composed"``: lora_update (its own fused launch, which ROUNDS v and g to ``dtype`` in y) and then the GEGLU kernel on the
    rounded values."""
    u = P.unit_roundoff(dtype)
    x64, a64, b64, y64 = (t.to(torch.float64) for t in (x, a, b, y))
    s = float(s)
    K, Rp = a.shape[1], a.shape[0]
    T = x64 @ a64.T
    e1 = P.accumulate_bound(x64.abs() @ a64.abs().T, K, height=P.mfma_height(K, 32))
    eT = e1 + u * (T.abs() + e1) + P._TINY[dtype]
    U = T @ b64.T
    absU = (T.abs() + eT) @ b64.abs().T
    eU = eT @ b64.abs().T + P.accumulate_bound(absU, Rp, height=P.mfma_height(Rp, 32))
    pre = y64 + s * U
    e = abs(s) * eU + P.U_F32 * abs(s) * (U.abs() + eU)               # 4.
    e = e + P.U_F32 * (y64.abs() + abs(s) * (U.abs() + eU) + e)      # 5.
    if route == "composed":
        e = e + u * (pre.abs() + e) + P._TINY[dtype]                  # y is stored in between
    (v, g), (ev, eg) = deinterleave_cols(pre), deinterleave_cols(e)
    gel = F.gelu(g)
    dg = P.LIP_GELU * eg + _gelu_erf_eval_error(g)                    # 6.
    out = v * gel
    eo = gel.abs() * ev + v.abs() * dg + ev * dg                      # 7.
    eo = eo + P.U_F32 * (out.abs() + eo)
    return out, eo + u * (out.abs() + eo) + P._TINY[dtype]
