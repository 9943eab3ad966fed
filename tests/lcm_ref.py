"""The yardstick of the few-step (latent-consistency, LCM) path, shared by tests/test_lcm_cpu.py and tests/test_lcm_gpu.py and built
like tests/anysize_ref.py: from the oracle's own modules, nothing of the code under test.

  * ``lcm_forward`` / ``build_lcm_unet``: the oracle UNet's forward with diffusers' ``TimestepEmbedding.cond_proj`` in front of
    ``time_embedding.linear_1`` -- ``temb_in = sinusoid.to(dtype) + cond_proj(timestep_cond)`` -- where ``cond_proj`` is one
    ``nn.Linear(time_cond_proj_dim, block_out_channels[0], bias=False)`` hung on the oracle's ``time_embedding``.  The up loop is the
    any-size one of tests/anysize_ref.py (the GPU file runs a 5 x 7 latent).  With a zero or absent ``timestep_cond`` it equals the
    stock oracle forward bit for bit (tests/test_lcm_cpu.py).
  * ``lcm_step_f32`` / ``RefLCMScheduler``: the LCM step as plain float32 torch expressions, and a scheduler written from the
    specification (schedule in numpy, boundary scalings in Python floats) that drives the reference loops.
  * ``guidance_embedding``: the ``timestep_cond`` the reference pipelines build from ``guidance_scale - 1``.
  * ``gm_loop`` / ``dual_loop``: oracle.pipelines' two loops with that conditioning handed to each UNet that has a ``cond_proj``.
"""
import copy
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import fixtures
from oracle.pipelines import _cfg
from oracle.unet import timestep_embedding

F32 = torch.float32
COND_DIM = 32  # time_cond_proj_dim of the tiny LCM UNets


# ---------------------------------------------------------------------------------------------------------------------------
# the UNet
# ---------------------------------------------------------------------------------------------------------------------------
def lcm_forward(self, sample, timestep, encoder_hidden_states=None, timestep_cond=None, cross_attention_kwargs=None,
                added_cond_kwargs=None, return_dict=False):
    if not torch.is_tensor(timestep):
        timestep = torch.tensor([timestep], dtype=torch.float32, device=sample.device)
    t = timestep.reshape(-1).to(sample.device).expand(sample.shape[0])
    temb_in = timestep_embedding(t, self.config.block_out_channels[0], self.config.flip_sin_to_cos, self.config.freq_shift).to(sample.dtype)
    if timestep_cond is not None:
        temb_in = temb_in + self.time_embedding.cond_proj(timestep_cond.to(sample.dtype))
    temb = self.time_embedding.linear_2(F.silu(self.time_embedding.linear_1(temb_in)))
    x = self.conv_in(sample)
    skips = [x]
    for blk in self.down_blocks:
        x, outs = blk(x, temb, encoder_hidden_states)
        skips.extend(outs)
    x = self.mid_block(x, temb, encoder_hidden_states)
    for blk in self.up_blocks:
        size = skips[-(len(blk.resnets) + 1)].shape[-2:] if blk.has_up else None  # taken before the pops
        for i, r in enumerate(blk.resnets):
            x = r(torch.cat([x, skips.pop()], dim=1), temb)
            if blk.has_attn:
                x = blk.attentions[i](x, encoder_hidden_states)
        if blk.has_up:
            x = blk.upsamplers[0].conv(F.interpolate(x, size=tuple(size), mode="nearest"))
    x = self.conv_out(F.silu(self.conv_norm_out(x)))
    return (x,)


def build_lcm_unet(in_channels=4, cond_dim=COND_DIM, seed=4321):
    """The tiny oracle UNet (the weights of ``fixtures.build_unet("tiny", in_channels)``) with ``time_cond_proj_dim = cond_dim``: a
    bias-free ``cond_proj`` with uniform +-1/sqrt(cond_dim) weights from its own generator, and the forward above.  Its
    ``state_dict()`` then carries ``time_embedding.cond_proj.weight``, the key a diffusers LCM checkpoint has."""
    u = fixtures.build_unet("tiny", in_channels, time_cond_proj_dim=cond_dim)
    ch0 = u.config.block_out_channels[0]
    proj = nn.Linear(cond_dim, ch0, bias=False)
    g = torch.Generator().manual_seed(seed + in_channels)
    with torch.no_grad():
        proj.weight.copy_((torch.rand(ch0, cond_dim, generator=g) * 2 - 1) * cond_dim ** -0.5)
    u.time_embedding.cond_proj = proj.requires_grad_(False)
    u.forward = types.MethodType(lcm_forward, u)
    return u


def guidance_embedding(w, dim, dtype=F32):
    """[len(w), dim]: [sin | cos] of 1000 w exp(-ln(10000) i / (half - 1)), a zero column behind them for an odd ``dim`` (float32
    torch arithmetic in the order of the formula, as the reference pipelines evaluate it)."""
    half = dim // 2
    step = torch.log(torch.tensor(10000.0)) / (half - 1)
    freqs = torch.exp(torch.arange(half, dtype=dtype) * -step)
    arg = (w * 1000.0).to(dtype)[:, None] * freqs[None, :]
    out = torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)
    return F.pad(out, (0, 1)) if dim % 2 else out


def cond_for(unet, guidance_scale, rows):
    dim = getattr(unet.config, "time_cond_proj_dim", None)
    if dim is None:
        return None
    return guidance_embedding(torch.tensor(guidance_scale - 1).repeat(rows), dim)


# ---------------------------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------------------------
def _s(v):
    return torch.tensor(float(v), dtype=F32)  # a scalar the kernel receives as ``float``


def lcm_step_f32(eps, x, coefs, noise=None, clip_range=None):
    """(x_prev, x0, denoised) of gmd_lcm_step given the guided eps; coefs = (sched_sqrt_a, sched_sqrt_1ma, c_skip, c_out, sqrt_a_prev,
    sqrt_b_prev, sqrt_a, sqrt_1ma).  Works on host and device tensors alike (0-d float32 scalars)."""
    ssa, ss1, cs, co, sp, bp, sa, s1 = (_s(c).to(x.device) for c in coefs)
    x0 = (x - s1 * eps) / sa
    p0 = (x - ss1 * eps) / ssa
    if clip_range is not None:
        p0 = p0.clamp(-float(clip_range), float(clip_range))
    den = co * p0 + cs * x
    prev = den if noise is None else sp * den + bp * noise
    return prev, x0, den


class _Cfg(dict):
    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


class RefLCMScheduler:
    """LCM sampling written from its specification: scaled-linear betas, the schedule ``origin[floor(linspace(0, len, n))]`` over the
    reversed training timesteps ``k, 2k, ... - 1``, boundary scalings with sigma_data = 0.5 and timestep_scaling = 10 in Python
    floats, noise from ``torch.randn(generator)`` at every step but the last.  The protocol of oracle.schedulers' classes."""

    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, original_inference_steps=50, timestep_scaling=10.0):
        self.config = _Cfg(num_train_timesteps=num_train_timesteps, original_inference_steps=original_inference_steps,
                           timestep_scaling=timestep_scaling)
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=F32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.timesteps = None
        self._i = 0

    def set_timesteps(self, n, device=None):
        c = self.config
        k = c.num_train_timesteps // c.original_inference_steps
        origin = (np.arange(1, c.original_inference_steps + 1) * k - 1)[::-1]
        idx = np.floor(np.linspace(0, len(origin), n, endpoint=False)).astype(np.int64)
        self.timesteps = torch.from_numpy(origin[idx].astype(np.int64))
        self._i = 0

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        t = int(timestep)
        assert t == int(self.timesteps[self._i])
        last = self._i == len(self.timesteps) - 1
        prev_t = t if last else int(self.timesteps[self._i + 1])
        a_t, a_p = self.alphas_cumprod[t], self.alphas_cumprod[prev_t]
        s = t * self.config.timestep_scaling
        coefs = (a_t ** 0.5, (1 - a_t) ** 0.5, 0.25 / (s * s + 0.25), s / (s * s + 0.25) ** 0.5, a_p ** 0.5, (1 - a_p) ** 0.5, 1.0, 0.0)
        noise = None if last else torch.randn(sample.shape, generator=generator, dtype=sample.dtype)
        prev, _, den = lcm_step_f32(model_output, sample, coefs, noise=noise)
        self._i += 1
        return (prev, den)


# ---------------------------------------------------------------------------------------------------------------------------
# the loops (oracle.pipelines.gm_loop / dual_loop plus the guidance-scale conditioning)
# ---------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def gm_loop(unet, scheduler, sdr_latent, prompt_embeds, negative_prompt_embeds, latents, num_inference_steps=4, guidance_scale=7.5,
            generator=None):
    cond = cond_for(unet, guidance_scale, latents.shape[0])
    do_cfg = guidance_scale > 1 and cond is None  # a guidance-embedded UNet runs without the CFG duplicate
    embeds = torch.cat([negative_prompt_embeds, prompt_embeds]) if do_cfg else prompt_embeds
    scheduler.set_timesteps(num_inference_steps)
    latents = latents * scheduler.init_noise_sigma
    for t in scheduler.timesteps:
        cat_latents = torch.cat([sdr_latent, latents], dim=1)
        x = torch.cat([cat_latents] * 2) if do_cfg else cat_latents
        eps = unet(x, t, encoder_hidden_states=embeds, timestep_cond=cond, return_dict=False)[0]
        if do_cfg:
            eps = _cfg(eps, guidance_scale, 0.0)
        latents = scheduler.step(eps, t, latents, generator=generator, return_dict=False)[0]
    return latents


@torch.no_grad()
def dual_loop(unet, gm_unet, scheduler, prompt_embeds, negative_prompt_embeds, latents, num_inference_steps=4, guidance_scale=7.5,
              generator=None):
    """Each UNet gets the embedding of its own width iff it has a ``cond_proj``; the generator is shared, SDR step before GM step."""
    cond = cond_for(unet, guidance_scale, latents.shape[0])
    gm_cond = cond_for(gm_unet, guidance_scale, latents.shape[0])
    do_cfg = guidance_scale > 1 and cond is None
    embeds = torch.cat([negative_prompt_embeds, prompt_embeds]) if do_cfg else prompt_embeds
    gm_embeds = embeds[negative_prompt_embeds.shape[0]:] if do_cfg else embeds
    scheduler.set_timesteps(num_inference_steps)
    latents = latents * scheduler.init_noise_sigma
    gm_latents = latents.clone()
    gm_scheduler = copy.deepcopy(scheduler)
    for t in scheduler.timesteps:
        x = torch.cat([latents] * 2) if do_cfg else latents
        eps = unet(x, t, encoder_hidden_states=embeds, timestep_cond=cond, return_dict=False)[0]
        if do_cfg:
            eps = _cfg(eps, guidance_scale, 0.0)
        a = scheduler.alphas_cumprod[t].view(-1, 1, 1, 1)
        x0 = (latents - (1 - a).sqrt() * eps) / a.sqrt()  # pre-step latents
        latents = scheduler.step(eps, t, latents, generator=generator, return_dict=False)[0]
        gm_eps = gm_unet(torch.cat([x0, gm_latents], dim=1), t, encoder_hidden_states=gm_embeds, timestep_cond=gm_cond, return_dict=False)[0]
        gm_latents = gm_scheduler.step(gm_eps, t, gm_latents, generator=generator, return_dict=False)[0]
    return latents, gm_latents
