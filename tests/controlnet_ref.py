"""References of the ControlNet tests (test_controlnet_cpu.py, test_controlnet_gpu.py): plain helper module in the style of
tests/anysize_ref.py and tests/small_ref.py.  Nothing here uses the library.

  * ``ControlNetRef``: diffusers' SD-1.5 ControlNet on the CPU, assembled from the oracle's blocks (oracle/unet.py: DownBlock, MidBlock,
    TimestepEmbedding) with the conditioning embedding and the zero convolutions written from their specification, under diffusers'
    state-dict names;
  * ``unet_forward_with_residuals``: the oracle UNet's any-size forward (tests/anysize_ref.py) with diffusers' two additions: every skip
    gets its residual before the up blocks read it, the mid block's output gets the mid residual;
  * ``concat_add_ref`` / ``assert_concat``: the torch expression gmd_concat_channels_add must equal bit for bit;
  * ``assert_stats``: the float64 sums of the STORED B part per 64-row block and bucket, with the per-entry bound of
    tests/stats_handoff.py, and no entry left unwritten;
  * ``dual_loop_controlnet``: oracle.pipelines.dual_loop with the SDR UNet steered by a ControlNet, as diffusers'
    StableDiffusionControlNetPipeline steers its UNet (guidance window, guess mode).
"""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

import small_ref as S
import stats_handoff as SH
from oracle import unet as OU
from oracle.pipelines import _cfg

N_RES = 13  # twelve down residuals and the mid residual of an SD-1.5 ControlNet


def tiny_controlnet_config():
    """The encoder of oracle.unet.tiny_unet_config with a tiny conditioning embedding."""
    cfg = OU.tiny_unet_config(4)
    cfg["conditioning_embedding_out_channels"] = (8, 8, 16, 16)
    return cfg


class CondEmbedding(nn.Module):
    """diffusers ControlNetConditioningEmbedding: conv_in, (e_i -> e_i, e_i -> e_{i+1} stride 2) per level, each followed by SiLU,
    then conv_out without activation.  Three stride-2 convolutions for four widths: the image is 8x the latent side."""

    def __init__(self, out_channels, cond_channels, widths):
        super().__init__()
        e = list(widths)
        self.conv_in = nn.Conv2d(cond_channels, e[0], 3, padding=1)
        blocks = []
        for i in range(len(e) - 1):
            blocks += [nn.Conv2d(e[i], e[i], 3, padding=1), nn.Conv2d(e[i], e[i + 1], 3, padding=1, stride=2)]
        self.blocks = nn.ModuleList(blocks)
        self.conv_out = nn.Conv2d(e[-1], out_channels, 3, padding=1)

    def forward(self, x):
        x = F.silu(self.conv_in(x))
        for b in self.blocks:
            x = F.silu(b(x))
        return self.conv_out(x)


class ControlNetRef(nn.Module):
    def __init__(self, conditioning_channels=3, conditioning_embedding_out_channels=(16, 32, 96, 256), **overrides):
        super().__init__()
        cfg = dict(OU.SD15_UNET_CONFIG)
        cfg.update(overrides)
        cfg.update(conditioning_channels=conditioning_channels, conditioning_embedding_out_channels=tuple(conditioning_embedding_out_channels))
        self.config = type("cfg", (), {})()
        for k, v in cfg.items():
            setattr(self.config, k, v)
        ch = list(cfg["block_out_channels"])
        L = len(ch)
        heads = cfg["attention_head_dim"]
        heads = list(heads) if isinstance(heads, (list, tuple)) else [heads] * L
        cross, groups, eps, n = cfg["cross_attention_dim"], cfg["norm_num_groups"], cfg["norm_eps"], cfg["layers_per_block"]
        temb = ch[0] * 4
        self.conv_in = nn.Conv2d(cfg["in_channels"], ch[0], 3, padding=1)
        self.time_embedding = OU.TimestepEmbedding(ch[0], temb)
        self.controlnet_cond_embedding = CondEmbedding(ch[0], conditioning_channels, conditioning_embedding_out_channels)
        downs, zero, cout = [], [nn.Conv2d(ch[0], ch[0], 1)], ch[0]
        for i, t in enumerate(cfg["down_block_types"]):
            cin, cout = cout, ch[i]
            downs.append(OU.DownBlock(cin, cout, temb, n, heads[i], cross, t.startswith("CrossAttn"), i != L - 1, groups, eps))
            zero += [nn.Conv2d(cout, cout, 1) for _ in range(n + (1 if i != L - 1 else 0))]
        self.down_blocks = nn.ModuleList(downs)
        self.controlnet_down_blocks = nn.ModuleList(zero)
        self.mid_block = OU.MidBlock(ch[-1], temb, heads[-1], cross, groups, eps)
        self.controlnet_mid_block = nn.Conv2d(ch[-1], ch[-1], 1)

    def zero_the_zero_convs(self):
        """diffusers' zero_module on the thirteen zero convolutions and the embedding's conv_out (a fresh ControlNet: from_unet)."""
        with torch.no_grad():
            for m in list(self.controlnet_down_blocks) + [self.controlnet_mid_block, self.controlnet_cond_embedding.conv_out]:
                m.weight.zero_()
                m.bias.zero_()
        return self

    def forward(self, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale=1.0, guess_mode=False):
        if not torch.is_tensor(timestep):
            timestep = torch.tensor([timestep], dtype=torch.float32)
        t = timestep.reshape(-1).expand(sample.shape[0])
        temb = OU.timestep_embedding(t, self.config.block_out_channels[0], self.config.flip_sin_to_cos, self.config.freq_shift)
        temb = self.time_embedding(temb.to(sample.dtype))
        x = self.conv_in(sample) + self.controlnet_cond_embedding(controlnet_cond)
        skips = [x]
        for blk in self.down_blocks:
            x, outs = blk(x, temb, encoder_hidden_states)
            skips.extend(outs)
        x = self.mid_block(x, temb, encoder_hidden_states)
        down = [z(s) for s, z in zip(skips, self.controlnet_down_blocks)]
        mid = self.controlnet_mid_block(x)
        sc = guess_scales(conditioning_scale) if guess_mode else [float(conditioning_scale)] * N_RES
        return [d * s for d, s in zip(down, sc[:-1])], mid * sc[-1]


def guess_scales(scale):
    """diffusers' guess-mode ramp (controlnet.py: ``torch.logspace(-1, 0, len(down) + 1) * conditioning_scale``) as floats."""
    return [float(v) for v in torch.logspace(-1, 0, N_RES) * scale]


def keep_window(n, start, end):
    """diffusers' ``controlnet_keep``: 1.0 - float(i / n < start or (i + 1) / n > end), as booleans."""
    return [bool(1.0 - float(i / n < start or (i + 1) / n > end)) for i in range(n)]


def controlnet_param_count(cfg):
    """Closed-form parameter count of the conditioning embedding and the zero convolutions over a config, plus the encoder's count
    taken from an oracle UNet of the same config (conv_in, time embedding, down blocks, mid block)."""
    ch = list(cfg["block_out_channels"])
    e = list(cfg["conditioning_embedding_out_channels"])
    n = cfg.get("layers_per_block", 2)
    conv = lambda ci, co, k: co * ci * k * k + co
    emb = conv(cfg.get("conditioning_channels", 3), e[0], 3) + conv(e[-1], ch[0], 3)
    emb += sum(conv(e[i], e[i], 3) + conv(e[i], e[i + 1], 3) for i in range(len(e) - 1))
    skip = [ch[0]]
    for i, c in enumerate(ch):
        skip += [c] * (n + (1 if i != len(ch) - 1 else 0))
    zero = sum(conv(c, c, 1) for c in skip) + conv(ch[-1], ch[-1], 1)
    u = OU.UNet2DConditionModel(**{k: v for k, v in cfg.items() if k in OU.SD15_UNET_CONFIG})
    enc = sum(p.numel() for nm, p in u.named_parameters() if nm.startswith(("conv_in.", "time_embedding.", "down_blocks.", "mid_block.")))
    return enc + emb + zero


# ---------------------------------------------------------------------------------------------------------------------------
# the UNet with residuals
# ---------------------------------------------------------------------------------------------------------------------------
def unet_forward_with_residuals(unet, sample, timestep, encoder_hidden_states, down_res=None, mid_res=None):
    """tests/anysize_ref.anysize_forward with diffusers' ``down_block_additional_residuals`` / ``mid_block_additional_residual``."""
    if not torch.is_tensor(timestep):
        timestep = torch.tensor([timestep], dtype=torch.float32)
    t = timestep.reshape(-1).expand(sample.shape[0])
    temb = OU.timestep_embedding(t, unet.config.block_out_channels[0], unet.config.flip_sin_to_cos, unet.config.freq_shift)
    temb = unet.time_embedding(temb.to(sample.dtype))
    x = unet.conv_in(sample)
    skips = [x]
    for blk in unet.down_blocks:
        x, outs = blk(x, temb, encoder_hidden_states)
        skips.extend(outs)
    x = unet.mid_block(x, temb, encoder_hidden_states)
    if down_res is not None:
        assert len(down_res) == len(skips)
        skips = [s + r for s, r in zip(skips, down_res)]
        x = x + mid_res
    for blk in unet.up_blocks:
        size = skips[-(len(blk.resnets) + 1)].shape[-2:] if blk.has_up else None
        for i, r in enumerate(blk.resnets):
            x = r(torch.cat([x, skips.pop()], dim=1), temb)
            if blk.has_attn:
                x = blk.attentions[i](x, encoder_hidden_states)
        if blk.has_up:
            x = blk.upsamplers[0].conv(F.interpolate(x, size=tuple(size), mode="nearest"))
    return unet.conv_out(F.silu(unet.conv_norm_out(x)))


# ---------------------------------------------------------------------------------------------------------------------------
# the fused concat
# ---------------------------------------------------------------------------------------------------------------------------
def concat_add_ref(a, b, ra, rb, scales, ia, ib, r_row0, fault=None):
    """``cat([a + ra * scales[ia], b + rb * scales[ib]], -1)`` on the rows from ``r_row0`` on, a plain copy before: torch's own
    arithmetic on CPU tensors of the kernel's dtype (product in float32, rounded; sum in float32, rounded).  ``fault``: the two mistakes
    the checker exists for -- "row0_ignored" (the residual lands on the FIRST rows) and "scale_after_add" ((s + r) * scale)."""
    def part(s, r, i):
        s = s.clone()
        if r is None:
            return s
        k = float(scales[i])
        n = r.shape[0]
        lo = 0 if fault == "row0_ignored" else r_row0
        if fault == "scale_after_add":
            s[lo:lo + n] = (s[lo:lo + n] + r) * k
        else:
            s[lo:lo + n] = s[lo:lo + n] + r * k
        return s

    return torch.cat([part(a, ra, ia), part(b, rb, ib)], -1)


def assert_concat(got, a, b, ra, rb, scales, ia, ib, r_row0, what):
    S.assert_bit_equal(got, concat_add_ref(a, b, ra, rb, scales, ia, ib, r_row0), what)


def edge_values(dtype):
    """Values a fused skip + scale * residual can get wrong, as (skip, residual) pairs: +-0 on either side; a residual whose product with
    0.3 is subnormal in float16 (2^-15 * 0.3 < 2^-14); a sum that lies exactly between two neighbours of the dtype and must round to
    even (1 + u with scale 1: ties to 1; 1 + 2^-k + u: ties up)."""
    u = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]
    s = [0.0, -0.0, 0.0, -0.0, 1.0, 1.0, 1.0 + 2 * u, 3.0, -1.0, 65000.0 if dtype != torch.float16 else 1000.0]
    r = [0.0, 0.0, -0.0, -0.0, 2.0 ** -15, u, u, 2.0 ** -15, -u, 1.0]
    return torch.tensor(s, dtype=torch.float64).to(dtype), torch.tensor(r, dtype=torch.float64).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# the statistics of the stored B part
# ---------------------------------------------------------------------------------------------------------------------------
def assert_stats(got, stored_b, bucket, what):
    """``got`` float32 [rows / 64, Cb / bucket, 2] against the float64 {sum, sum of squares} of the STORED B-part values
    ``stored_b`` [rows, Cb]: every entry written (finite) and inside stats_handoff.bucket_ref_bound's per-entry bound."""
    ref, bound = SH.bucket_ref_bound(stored_b.reshape(-1, stored_b.shape[-1]).cpu(), bucket)
    g = got.detach().cpu()
    assert not bool(torch.isnan(g).any()), f"{what}: {int(torch.isnan(g).sum())} statistics entries were never written (NaN pre-fill)"
    return SH.assert_entries(g, ref, bound, what)


# ---------------------------------------------------------------------------------------------------------------------------
# the dual loop with a ControlNet
# ---------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def dual_loop_controlnet(unet, gm_unet, controlnet, scheduler, prompt_embeds, negative_prompt_embeds, latents, control_image,
                         num_inference_steps=50, guidance_scale=7.5, conditioning_scale=1.0, guess_mode=False,
                         control_guidance_start=0.0, control_guidance_end=1.0, record=None):
    """oracle.pipelines.dual_loop with the SDR UNet's call replaced by ControlNet -> UNet with residuals.  The GM UNet is untouched.
    ``controlnet`` None: the plain loop through the same restated UNet forward."""
    do_cfg = guidance_scale > 1
    embeds = torch.cat([negative_prompt_embeds, prompt_embeds]) if do_cfg else prompt_embeds
    gm_embeds = embeds[negative_prompt_embeds.shape[0]:] if do_cfg else embeds
    scheduler.set_timesteps(num_inference_steps)
    n = len(scheduler.timesteps)
    keep = keep_window(n, control_guidance_start, control_guidance_end)
    half = guess_mode and do_cfg
    image = control_image if (half or not do_cfg) else torch.cat([control_image] * 2)
    latents = latents * scheduler.init_noise_sigma
    gm_latents = latents.clone()
    gm_scheduler = copy.deepcopy(scheduler)
    for i, t in enumerate(scheduler.timesteps):
        x = torch.cat([latents] * 2) if do_cfg else latents
        x = scheduler.scale_model_input(x, t)
        gm_latents = gm_scheduler.scale_model_input(gm_latents, t)
        down = mid = None
        if controlnet is not None and keep[i]:
            c_in = scheduler.scale_model_input(latents, t) if half else x
            c_emb = embeds[negative_prompt_embeds.shape[0]:] if half else embeds
            down, mid = controlnet(c_in, t, c_emb, image, conditioning_scale=conditioning_scale, guess_mode=guess_mode)
            if half:  # the unconditional half is left unchanged
                down = [torch.cat([torch.zeros_like(d), d]) for d in down]
                mid = torch.cat([torch.zeros_like(mid), mid])
        eps = unet_forward_with_residuals(unet, x, t, embeds, down, mid)
        if do_cfg:
            eps = _cfg(eps, guidance_scale, 0.0)
        a = scheduler.alphas_cumprod.to(eps.device)[t].view(-1, 1, 1, 1)
        x0 = (latents - (1 - a).sqrt() * eps) / a.sqrt()
        latents = scheduler.step(eps, t, latents, return_dict=False)[0]
        gm_eps = gm_unet(torch.cat([x0, gm_latents], dim=1), t, encoder_hidden_states=gm_embeds, return_dict=False)[0]
        gm_latents = gm_scheduler.step(gm_eps, t, gm_latents, return_dict=False)[0]
        if record is not None:
            record.append((latents.clone(), gm_latents.clone()))
    return latents, gm_latents
