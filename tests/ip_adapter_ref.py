"""References of the IP-Adapter tests (test_ip_adapter_cpu.py, test_ip_adapter_gpu.py): plain helper module in the style of
tests/controlnet_ref.py.  Nothing here uses the library.

  * ``decoupled_ref`` / ``decoupled_bound``: float64 ``softmax(s q k^T) v + ip_scale softmax(s q kip^T) vip`` and its per-element bound,
    built from the two calls of parity.attention_bound (one per branch);
  * ``emulate``: a float64 emulation of the fused kernel's arithmetic (P rounded to the 16-bit type, row sums from the unrounded
    probabilities, ONE store rounding), with the two faults the bound exists for: a maximum or a row sum shared between the branches;
  * ``independence_inputs``: inputs on which every image score exceeds every text score by ~40 at scale (or the mirror);
  * ``attn2_layers`` / ``expected_shapes`` / ``make_state_dict``: the adapter's checkpoint layout restated from diffusers
    (``{k}.to_k_ip.weight``, k = 1, 3, 5, ... in ``attn_processors`` order: down blocks, up blocks, mid block);
  * ``ImageProjection`` and ``IPAdapterRef``: the oracle UNet (oracle/unet.py blocks) with each ``attn2`` wrapped to add the image branch;
  * ``dual_loop_ip_adapter``: oracle.pipelines.dual_loop with the image-prompted SDR UNet.
"""
import copy

import torch
import torch.nn as nn

import parity as P
from oracle import pipelines as OP
from oracle import unet as OU


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel: reference, bound, emulation
# ---------------------------------------------------------------------------------------------------------------------------
def decoupled_ref(q, k, v, kip, vip, scale, ip_scale):
    """float64 O = softmax(scale q k^T) v + ip_scale softmax(scale q kip^T) vip; q [.., Nq, D], k / v [.., Nk, D], kip / vip [.., Nip, D]."""
    q64 = q.to(torch.float64)

    def branch(kk, vv):
        s = (q64 @ kk.to(torch.float64).transpose(-1, -2)) * scale
        return torch.softmax(s, -1) @ vv.to(torch.float64)

    return branch(k, v) + ip_scale * branch(kip, vip)


def decoupled_bound(q, k, v, kip, vip, scale, ip_scale, dtype, q_rounded=False):
    """(float64 reference, float64 per-element bound) of the fused kernel (csrc/attention_ip.hip).

    Each branch is one flash attention of its own -- a maximum, a row sum, a 16-bit P -- so each carries parity.attention_bound's terms:
        bound = b_text + |ip_scale| b_ip + 4 2^-24 (P_text |V| + |ip_scale| P_ip |V_ip|).
    ``q_rounded`` False: the kernel scales the float32 scores and never rounds Q again, for every head dim (there is no lagged
    stabiliser in it).  The single rounding of the stored sum, u |O| <= u (P_text |V| + |ip_scale| P_ip |V_ip|), is what the two
    branches' ``out_round`` terms add up to.  The last term is the float32 combine, counted in the kernel: the text accumulator times
    1 / l_text (one rounding of a value <= P_text |V|), the factor ip_scale / l_ip (a division: <= 2 roundings, relative, on the image
    term) and the fused multiply-add ot + f * oi (one rounding of the sum): 4 roundings of quantities bounded by the bracket.  The
    divisions 1 / l themselves are among the "+ 8" of attention_bound.  No rounding of the kernel is left uncounted."""
    ref_t, b_t = P.attention_bound(q, k, v, scale, dtype, q_rounded=q_rounded)
    ref_i, b_i = P.attention_bound(q, kip, vip, scale, dtype, q_rounded=q_rounded)
    q64 = q.to(torch.float64)
    pv_t = torch.softmax((q64 @ k.to(torch.float64).transpose(-1, -2)) * scale, -1) @ v.to(torch.float64).abs()
    pv_i = torch.softmax((q64 @ kip.to(torch.float64).transpose(-1, -2)) * scale, -1) @ vip.to(torch.float64).abs()
    a = abs(float(ip_scale))
    return ref_t + ip_scale * ref_i, b_t + a * b_i + 4 * P.U_F32 * (pv_t + a * pv_i)


def composed_bound(q, k, v, kip, vip, scale, ip_scale, dtype):
    """The composed 16-bit route: each branch is stored (its own ``out_round``, already in attention_bound, with the head dim's own Q
    treatment), then a + b * s in float32 (two roundings) and ONE more store rounding of the sum."""
    ref_t, b_t = P.attention_bound(q, k, v, scale, dtype)
    ref_i, b_i = P.attention_bound(q, kip, vip, scale, dtype)
    a = abs(float(ip_scale))
    ref = ref_t + ip_scale * ref_i
    mag = ref_t.abs() + a * ref_i.abs()
    e = b_t + a * b_i
    e = e + 2 * P.U_F32 * (mag + e)
    return ref, e + P.unit_roundoff(dtype) * (mag + e) + P._TINY[dtype]


def split_composed_bound(q, k, v, kip, vip, scale, ip_scale):
    """The composed float32 route on the matrix cores: two attention_split_bound branches and the float32 a + b * s (two roundings)."""
    ref_t, b_t = P.attention_split_bound(q, k, v, scale)
    ref_i, b_i = P.attention_split_bound(q, kip, vip, scale)
    a = abs(float(ip_scale))
    e = b_t + a * b_i
    return ref_t + ip_scale * ref_i, e + 2 * P.U_F32 * (ref_t.abs() + a * ref_i.abs() + e)


def exact_composed_bound(q, k, v, kip, vip, scale, ip_scale):
    """The composed exact float32 route (gemm -> row softmax -> gemm per branch, then a + b * s), from the GEMM bounds: scores are a
    float32 accumulation of D exact-operand products (each product rounds once, the sum in an unknown order: parity.accumulate_bound
    with h = D) and the scaling / exp (4 roundings), propagated through the softmax as in attention_bound; P is stored in float32 (one
    rounding, the row sum <= Nk + 2 roundings) and P V is a float32 accumulation of Nk rounded products."""
    def branch(kk, vv):
        q64, k64, v64 = q.to(torch.float64), kk.to(torch.float64), vv.to(torch.float64)
        n, D = k64.shape[-2], q64.shape[-1]
        s = (q64 @ k64.transpose(-1, -2)) * scale
        sabs = (q64.abs() @ k64.abs().transpose(-1, -2)) * abs(scale)
        d = (2 * D + 1 + 4) * P.U_F32 * sabs
        p = torch.softmax(s, -1)
        va = v64.abs()
        pv = p @ va
        pd = p * d
        score_term = (pd @ va + pd.sum(-1, keepdim=True) * pv) * torch.exp(2 * d.amax(-1, keepdim=True))
        return p @ v64, score_term + (2 * n + 1 + (n + 2) + 1 + 8) * P.U_F32 * pv + 2.0 ** -126

    ref_t, b_t = branch(k, v)
    ref_i, b_i = branch(kip, vip)
    a = abs(float(ip_scale))
    e = b_t + a * b_i
    return ref_t + ip_scale * ref_i, e + 2 * P.U_F32 * (ref_t.abs() + a * ref_i.abs() + e)


def _round16(x64, dtype):
    """Round a float64 tensor to the 16-bit type (round to nearest even, subnormals of the type kept, below them zero) -> float64."""
    return x64.to(torch.float32).to(dtype).to(torch.float64)


def emulate(q, k, v, kip, vip, scale, ip_scale, dtype, fault=None):
    """The fused kernel's arithmetic in float64 with its 16-bit roundings: per branch p = exp(s - m), the row sum from the unrounded p,
    the numerator from p rounded to ``dtype``; the two normalised branches are combined and the sum is rounded ONCE.
    fault: None (clean); "shared_max": both branches subtract the maximum over all text AND image scores; "shared_sum": both branches
    divide by the sum of both row sums (one softmax over all keys with the image part scaled)."""
    q64 = q.to(torch.float64)
    st = (q64 @ k.to(torch.float64).transpose(-1, -2)) * scale
    si = (q64 @ kip.to(torch.float64).transpose(-1, -2)) * scale
    mt, mi = st.amax(-1, keepdim=True), si.amax(-1, keepdim=True)
    if fault == "shared_max":
        mt = mi = torch.maximum(mt, mi)
    pt, pi = torch.exp(st - mt), torch.exp(si - mi)
    lt, li = pt.sum(-1, keepdim=True), pi.sum(-1, keepdim=True)
    if fault == "shared_sum":
        lt = li = lt + li
    ot = (_round16(pt, dtype) @ v.to(torch.float64)) / lt
    oi = (_round16(pi, dtype) @ vip.to(torch.float64)) / li
    return _round16(ot + ip_scale * oi, dtype)


def make_qkv(B, H, Nq, Nk, Nip, D, dtype, seed=0):
    """Seeded operands as the 16-bit (or float32) values the kernel reads: q [B, H, Nq, D], k / v [B, H, Nk, D], kip / vip [B, H, Nip, D]."""
    g = torch.Generator().manual_seed(seed)
    mk = lambda n: torch.randn(B, H, n, D, generator=g).to(dtype)
    return mk(Nq), mk(Nk), mk(Nk), mk(Nip), mk(Nip)


def independence_inputs(B, H, Nq, Nk, Nip, D, dtype, scale, image_dominates=True, gap=40.0, seed=0):
    """Operands on which every score of one branch exceeds every score of the other by ~``gap`` at scale: the dominant branch's keys
    carry +c in every coordinate where q carries +c (q = c + small noise, dominant keys = +c + noise, the others = -c + noise), with c
    chosen so that scale * D * 2 c^2 = gap.  A kernel that shares a stabiliser in a narrow type, or a row sum, returns ~0 for the weak
    branch; its own softmax is an ordinary one."""
    g = torch.Generator().manual_seed(seed)
    c = (gap / (2.0 * scale * D)) ** 0.5
    noise = lambda n: 0.05 * c * torch.randn(B, H, n, D, generator=g)
    q = (c + noise(Nq)).to(dtype)
    hi, lo = c, -c
    k = ((lo if image_dominates else hi) + noise(Nk)).to(dtype)
    kip = ((hi if image_dominates else lo) + noise(Nip)).to(dtype)
    v = torch.randn(B, H, Nk, D, generator=g).to(dtype)
    vip = torch.randn(B, H, Nip, D, generator=g).to(dtype)
    return q, k, v, kip, vip


# ---------------------------------------------------------------------------------------------------------------------------
# the checkpoint layout
# ---------------------------------------------------------------------------------------------------------------------------
def _cfg_of(cfg):
    c = dict(OU.SD15_UNET_CONFIG)
    c.update(cfg)
    return c


def attn2_layers(cfg):
    """[(k, module path of the transformer block, inner dim)] of the adapter's to_k_ip / to_v_ip weights for a UNet config: diffusers
    numbers ``unet.attn_processors`` in module order -- down blocks, up blocks, mid block -- with attn1 on the even and attn2 on the odd
    numbers, and stores the attn2 weights under their own number."""
    c = _cfg_of(cfg)
    ch = list(c["block_out_channels"])
    n = c["layers_per_block"]
    depth = c["transformer_layers_per_block"]
    depth = list(depth) if isinstance(depth, (list, tuple)) else [depth] * len(ch)
    out = []
    for i, t in enumerate(c["down_block_types"]):
        if t.startswith("CrossAttn"):
            out += [(f"down_blocks.{i}.attentions.{j}.transformer_blocks.{m}", ch[i]) for j in range(n) for m in range(depth[i])]
    rev, rdepth = list(reversed(ch)), list(reversed(depth))
    for i, t in enumerate(c["up_block_types"]):
        if t.startswith("CrossAttn"):
            out += [(f"up_blocks.{i}.attentions.{j}.transformer_blocks.{m}", rev[i]) for j in range(n + 1) for m in range(rdepth[i])]
    out += [(f"mid_block.attentions.0.transformer_blocks.{m}", ch[-1]) for m in range(depth[-1])]
    return [(2 * i + 1, path, dim) for i, (path, dim) in enumerate(out)]


def expected_shapes(cfg, tokens, clip_dim):
    """({image_proj key: shape}, {ip_adapter key: shape}) of a plain IP-Adapter for a UNet config."""
    cross = _cfg_of(cfg)["cross_attention_dim"]
    proj = {"proj.weight": (tokens * cross, clip_dim), "proj.bias": (tokens * cross,), "norm.weight": (cross,), "norm.bias": (cross,)}
    kv = {}
    for k, _, dim in attn2_layers(cfg):
        kv[f"{k}.to_k_ip.weight"] = (dim, cross)
        kv[f"{k}.to_v_ip.weight"] = (dim, cross)
    return proj, kv


def make_state_dict(cfg, tokens=4, clip_dim=32, seed=0, device=None, gain=1.0):
    """A seeded adapter {"image_proj": ..., "ip_adapter": ...}; ``device="meta"`` gives shapes without storage (SD-1.5: 22 M values)."""
    proj, kv = expected_shapes(cfg, tokens, clip_dim)
    if device == "meta":
        return {"image_proj": {k: torch.empty(s, device="meta") for k, s in proj.items()},
                "ip_adapter": {k: torch.empty(s, device="meta") for k, s in kv.items()}}
    g = torch.Generator().manual_seed(seed)
    sd = {"image_proj": {}, "ip_adapter": {}}
    for k, s in proj.items():
        if k == "norm.weight":
            sd["image_proj"][k] = 1.0 + 0.1 * torch.randn(s, generator=g)
        elif k.endswith("bias"):
            sd["image_proj"][k] = 0.1 * torch.randn(s, generator=g)
        else:
            sd["image_proj"][k] = torch.randn(s, generator=g) * s[1] ** -0.5
    for k, s in kv.items():
        sd["ip_adapter"][k] = gain * torch.randn(s, generator=g) * s[1] ** -0.5
    return sd


# ---------------------------------------------------------------------------------------------------------------------------
# the image-prompted oracle UNet
# ---------------------------------------------------------------------------------------------------------------------------
class ImageProjection(nn.Module):
    """diffusers ImageProjection: linear -> reshape to T tokens -> LayerNorm (eps 1e-5)."""

    def __init__(self, clip_dim, cross_dim, tokens):
        super().__init__()
        self.tokens, self.cross_dim = tokens, cross_dim
        self.proj = nn.Linear(clip_dim, tokens * cross_dim)
        self.norm = nn.LayerNorm(cross_dim, eps=1e-5)

    def forward(self, image_embeds):
        b = image_embeds.shape[0]
        return self.norm(self.proj(image_embeds).reshape(b, self.tokens, self.cross_dim))


class _IPAttention(nn.Module):
    """An oracle cross-attention with diffusers' IPAdapterAttnProcessor: the text attention, plus ``scale`` times an attention of the
    SAME query over the image tokens through to_k_ip / to_v_ip, summed in front of the out-projection."""

    def __init__(self, attn, to_k_ip, to_v_ip, owner):
        super().__init__()
        self.attn = attn
        self.to_k_ip = nn.Linear(to_k_ip.shape[1], to_k_ip.shape[0], bias=False)
        self.to_v_ip = nn.Linear(to_v_ip.shape[1], to_v_ip.shape[0], bias=False)
        with torch.no_grad():
            self.to_k_ip.weight.copy_(to_k_ip)
            self.to_v_ip.weight.copy_(to_v_ip)
        self._owner = [owner]  # a list: the owner is not a sub-module of this one

    def forward(self, x, context=None):
        a, own = self.attn, self._owner[0]
        B, N, C = x.shape
        H = a.heads
        heads = lambda t: t.view(B, t.shape[1], H, C // H).transpose(1, 2)
        q = heads(a.to_q(x))
        sc = (C // H) ** -0.5
        o = torch.softmax(q @ heads(a.to_k(context)).transpose(-1, -2) * sc, -1) @ heads(a.to_v(context))
        tok = own.ip_tokens.to(x.dtype)
        oi = torch.softmax(q @ heads(self.to_k_ip(tok)).transpose(-1, -2) * sc, -1) @ heads(self.to_v_ip(tok))
        o = o + own.scale * oi
        return a.to_out[0](o.transpose(1, 2).reshape(B, N, C))


class IPAdapterRef(nn.Module):
    """A deep copy of an oracle UNet with a plain IP-Adapter installed from ``state_dict``.  ``set_image_embeds`` takes
    [rows, n_images, clip_dim] (rows ordered like the text rows); the call signature is the oracle UNet's."""

    def __init__(self, unet, state_dict, scale=1.0):
        super().__init__()
        self.unet = copy.deepcopy(unet)
        self.config = self.unet.config
        pw = state_dict["image_proj"]["proj.weight"]
        cross = self.config.cross_attention_dim
        self.image_proj = ImageProjection(pw.shape[1], cross, pw.shape[0] // cross)
        self.image_proj.load_state_dict({k: v.to(pw.dtype) for k, v in state_dict["image_proj"].items()})
        self.image_proj.to(next(self.unet.parameters()).dtype)
        self.scale = float(scale)
        self.ip_tokens = None
        cfg = {k: getattr(self.config, k) for k in OU.SD15_UNET_CONFIG if hasattr(self.config, k)}
        for k, path, _ in attn2_layers(cfg):
            blk = self.unet.get_submodule(path)
            blk.attn2 = _IPAttention(blk.attn2, state_dict["ip_adapter"][f"{k}.to_k_ip.weight"],
                                     state_dict["ip_adapter"][f"{k}.to_v_ip.weight"], self).to(next(self.unet.parameters()).dtype)
        self.eval().requires_grad_(False)

    @torch.no_grad()
    def set_image_embeds(self, image_embeds):
        rows, n_img, clip = image_embeds.shape
        tok = self.image_proj(image_embeds.reshape(rows * n_img, clip).to(self.image_proj.proj.weight.dtype))
        self.ip_tokens = tok.reshape(rows, n_img * self.image_proj.tokens, -1)
        return self.ip_tokens

    def forward(self, sample, timestep, encoder_hidden_states=None, **kw):
        assert self.ip_tokens is not None and self.ip_tokens.shape[0] == sample.shape[0], "set_image_embeds first (one row per sample)"
        return self.unet(sample, timestep, encoder_hidden_states=encoder_hidden_states, **kw)


@torch.no_grad()
def dual_loop_ip_adapter(unet, gm_unet, state_dict, scheduler, prompt_embeds, negative_prompt_embeds, latents, image_embeds,
                         num_inference_steps=50, guidance_scale=7.5, ip_scale=1.0, record=None):
    """oracle.pipelines.dual_loop with the SDR UNet image-prompted.  ``image_embeds``: [(2 if guidance else 1) * B, n_images, clip_dim],
    [negative; positive] rows like the text.  The GM UNet is untouched."""
    ref = IPAdapterRef(unet, state_dict, ip_scale)
    ref.set_image_embeds(image_embeds)
    return OP.dual_loop(ref, gm_unet, scheduler, prompt_embeds, negative_prompt_embeds, latents,
                        num_inference_steps=num_inference_steps, guidance_scale=guidance_scale, record=record)
