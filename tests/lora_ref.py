"""LoRA references (plain helper module, like tests/ip_adapter_ref.py): synthetic adapters for the tiny UNet in the three key
conventions, TWO independent CPU references on the oracle UNet (merged weights; forward hooks), and the per-element bound of the
rank-update kernel in the style of tests/parity.py.

diffusers and peft are not installed: the key conventions are this repository's restatement of what their loaders accept
(gm_diffusion/components/lora.py), and the references restate what a LoRA IS -- W + s (alpha / r) B A -- on the oracle's own
nn.Linear modules."""
import copy

import torch
import torch.nn as nn

import parity as P

PROJECTIONS = tuple(f"{a}.{p}" for a in ("attn1", "attn2") for p in ("to_q", "to_k", "to_v", "to_out.0"))
CONVENTIONS = ("peft", "diffusers_old", "diffusers_processor", "kohya")


def target_linears(ou):
    """{module name: nn.Linear} of the eight attention projections of every BasicTransformerBlock of the oracle UNet ``ou``."""
    return {n: m for n, m in ou.named_modules() if isinstance(m, nn.Linear) and ".transformer_blocks." in n and n.endswith(PROJECTIONS)}


def canonical(ou, rank, seed, gain, alpha=None, dtype=torch.float32):
    """{module: (A [r, K], B [N, r], alpha)}: A ~ N(0, 1 / K), B ~ gain N(0, 1 / r), so every delta is ~gain times a unit-variance
    projection (a trained adapter's B is nowhere near zero; gain sets how far the adapted UNet moves).  ``dtype``: the factors are
    rounded to it (and returned as float32), so that a 16-bit model holds exactly these values."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, lin in sorted(target_linears(ou).items()):
        n, k = lin.weight.shape
        a = torch.randn(rank, k, generator=g) / k ** 0.5
        b = gain * torch.randn(n, rank, generator=g) / rank ** 0.5
        out[name] = (a.to(dtype).float(), b.to(dtype).float(), alpha)
    return out


def to_convention(canon, convention):
    """The canonical dict written with the keys of one convention.  ``diffusers_old`` / ``diffusers_processor`` have no alpha."""
    sd = {}
    for name, (a, b, alpha) in canon.items():
        if convention == "peft":
            sd[f"unet.{name}.lora_A.weight"], sd[f"unet.{name}.lora_B.weight"] = a, b
            if alpha is not None:
                sd[f"unet.{name}.alpha"] = torch.tensor(float(alpha))
        elif convention == "diffusers_old":
            assert alpha is None
            sd[f"unet.{name}.lora.down.weight"], sd[f"unet.{name}.lora.up.weight"] = a, b
        elif convention == "diffusers_processor":
            assert alpha is None
            blk, proj = name.rsplit(".to_", 1)
            proj = "to_" + proj.replace("out.0", "out")
            sd[f"unet.{blk}.processor.{proj}_lora.down.weight"], sd[f"unet.{blk}.processor.{proj}_lora.up.weight"] = a, b
        elif convention == "kohya":
            flat = "lora_unet_" + name.replace(".", "_")
            sd[f"{flat}.lora_down.weight"], sd[f"{flat}.lora_up.weight"] = a, b
            if alpha is not None:
                sd[f"{flat}.alpha"] = torch.tensor(float(alpha))
        else:
            raise ValueError(convention)
    return sd


def make_state_dict(unet_config, rank, seed, gain, convention="peft", alpha=None):
    from oracle import unet as OU

    torch.manual_seed(0)
    return to_convention(canonical(OU.UNet2DConditionModel(**unet_config), rank, seed, gain, alpha), convention)


def _factor(a, alpha):
    return 1.0 if alpha is None else float(alpha) / a.shape[0]


def merged_oracle(ou, canon, scale=1.0):
    """Reference (a): W + s (alpha / r) B A formed in float64 and loaded into a COPY of the oracle."""
    m = copy.deepcopy(ou)
    lin = target_linears(m)
    with torch.no_grad():
        for name, (a, b, alpha) in canon.items():
            w = lin[name].weight
            w.copy_((w.double() + scale * _factor(a, alpha) * (b.double() @ a.double())).to(w.dtype))
    return m


def hooked_oracle(ou, canon, scale=1.0):
    """Reference (b): the weights untouched; a forward hook on every adapted nn.Linear adds s (alpha / r) B (A x)."""
    m = copy.deepcopy(ou)
    lin = target_linears(m)
    for name, (a, b, alpha) in canon.items():
        f = scale * _factor(a, alpha)

        def hook(mod, inp, out, a=a, b=b, f=f):
            return out + f * ((inp[0] @ a.T.to(inp[0].dtype)) @ b.T.to(inp[0].dtype))

        lin[name].register_forward_hook(hook)
    return m


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel's per-element bound
# ---------------------------------------------------------------------------------------------------------------------------
def update_ref_bound(x, a, b, y, s, dtype, route="fused"):
    """(float64 reference, per-element bound) of ``y + s (x a^T) b^T`` for x [M, K], a [Rp, K], b [N, Rp], y [M, N] holding values of
    ``dtype`` and s a float32 value.  Every term named (u = unit roundoff of ``dtype``; products of two 16-bit values are exact in
    float32):
      1. first product T = x a^T: float32 accumulation on the matrix cores, K products chained through 16x16x32 instructions
         (accumulate_bound with mfma_height(K, 32));
      2. the ONE rounding of T to ``dtype``: u (|T| + e1) + the subnormal floor; eT = e1 + that.  It reaches the output through
         sum_j eT[m, j] |b[n, j]|;
      3. second product: float32 accumulation of Rp products of |That| <= |T| + eT with |b|;
      4. the scale: s * acc rounds once in float32 (or not at all when the compiler contracts it with the add into one FMA);
      5. the add to float(y) rounds once in float32, then the ONE rounding of the stored value (parity._finish).
    ``route="composed"``: two gemm_nt launches and scaled_add -- the K loops' order is the launch plan's (height unknown: K), and U is
    rounded to ``dtype`` once more before the scaled add."""
    u = P.unit_roundoff(dtype)
    x64, a64, b64, y64 = (t.to(torch.float64) for t in (x, a, b, y))
    s = float(s)
    K, Rp = a.shape[1], a.shape[0]
    fused = route == "fused"
    T = x64 @ a64.T
    e1 = P.accumulate_bound(x64.abs() @ a64.abs().T, K, height=P.mfma_height(K, 32) if fused else None)
    eT = e1 + u * (T.abs() + e1) + P._TINY[dtype]
    U = T @ b64.T
    absU = (T.abs() + eT) @ b64.abs().T
    eU = eT @ b64.abs().T + P.accumulate_bound(absU, Rp, height=P.mfma_height(Rp, 32) if fused else None)
    if not fused:
        eU = eU + u * (U.abs() + eU) + P._TINY[dtype]
    value = y64 + s * U
    e = abs(s) * eU + P.U_F32 * abs(s) * (U.abs() + eU)             # 4.
    e = e + P.U_F32 * (y64.abs() + abs(s) * (U.abs() + eU) + e)    # 5. the float32 add
    return value, P._finish(value, e, dtype)


def update_ref_bound_f32(x, a, b, y, s, mode):
    """The composed float32 route against float64: as above with float32 roundings of T and U, products that round once each
    ("exact": U_F32 |x||a|) or carry the split scheme's residual ("split": parity.split_product_bound, three partial products per
    product in the accumulation), K loops in an unknown order."""
    x64, a64, b64, y64 = (t.to(torch.float64) for t in (x, a, b, y))
    s = float(s)
    K, Rp = a.shape[1], a.shape[0]
    u = P.U_F32

    def product(p, q, k):
        absd = p.abs() @ q.abs().T
        if mode == "split":
            return P.accumulate_bound(absd, 3 * k) + P.split_product_bound(p, q)
        return P.accumulate_bound(absd, k) + u * absd

    T = x64 @ a64.T
    e1 = product(x64, a64, K)
    eT = e1 + u * (T.abs() + e1) + P._TINY[torch.float32]
    U = T @ b64.T
    That_abs = T.abs() + eT
    eU = eT @ b64.abs().T + product(That_abs, b64, Rp)
    eU = eU + u * (U.abs() + eU) + P._TINY[torch.float32]
    value = y64 + s * U
    e = abs(s) * eU + 2 * u * (y64.abs() + abs(s) * (U.abs() + eU))
    return value, P._finish(value, e, torch.float32)
