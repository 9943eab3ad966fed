"""References for the img2img / inpainting tests (tests/test_img2img_cpu.py, tests/test_img2img_gpu.py), written from the feature's
definition and sharing no code with the package:

* ``blend_f32``: gmd_inpaint_blend as float32 torch expressions on the CPU, evaluated op by op in the kernel's order;
* ``add_noise_*`` / ``noise_index``: diffusers' ``add_noise`` of the three scheduler families and its index rule, restated;
* ``dual_img2img_loop``: the dual-UNet loop with ``image`` / ``strength`` / ``mask_image`` over the oracle UNets and the reference
  schedulers the other suites use (oracle PNDM and DPM-Solver++ 2M, tests/ddim_ref.py, tests/euler_ref.py).
"""
import copy

import torch

F32 = torch.float32


def _s(v):
    return torch.tensor(float(v), dtype=F32)  # a scalar the kernel receives as ``float``


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------------
def blend_f32(z0, x_prev=None, x0=None, mask=None, noise=None, ca=1.0, cb=0.0):
    """(x_prev, x0) after gmd_inpaint_blend.  z0 / x_prev / x0 / noise: [B, C, h, w]; mask: [1 | B, 1, h, w] (broadcast by torch as
    the kernel indexes it).  Every line is one torch op per arithmetic operation of the kernel, in its order."""
    keep = z0 if noise is None else _s(ca) * z0 + _s(cb) * noise
    if mask is None:
        return keep.clone(), None
    out_prev = None if x_prev is None else (1 - mask) * keep + mask * x_prev
    out_x0 = None if x0 is None else (1 - mask) * z0 + mask * x0
    return out_prev, out_x0


def masks(B, h, w):
    """Per-sample latent masks [B, 1, h, w] with values in {0, 1}: 1 = repaint.  Sample b is a disc (odd b: the outside of one) whose
    centre moves with b; each keeps and repaints at least a quarter of the pixels and no edge is a rectangle's."""
    yy, xx = torch.meshgrid(torch.arange(h, dtype=F32), torch.arange(w, dtype=F32), indexing="ij")
    out = []
    for b in range(B):
        cy, cx = h * (0.45 + 0.1 * (b % 2)), w * (0.5 - 0.08 * (b % 3))
        r2 = ((yy - cy) / h) ** 2 + ((xx - cx) / w) ** 2
        disc = (r2 < 0.36 ** 2).to(F32)
        out.append(1 - disc if b % 2 else disc)
    m = torch.stack(out)[:, None]
    for b in range(B):
        frac = float(m[b].mean())
        assert 0.25 <= frac <= 0.75, f"mask {b} repaints {frac:.2f} of its pixels: outside [1/4, 3/4]"
    return m


# ---------------------------------------------------------------------------------------------------------------------------
# diffusers' add_noise, restated per family (float32 tables, as there)
# ---------------------------------------------------------------------------------------------------------------------------
def _per_sample(c, like):
    c = c.flatten()
    while len(c.shape) < len(like.shape):
        c = c.unsqueeze(-1)
    return c


def add_noise_vp(alphas_cumprod, x, noise, timesteps):
    """DDPM / DDIM / PNDM / LCM: sqrt(a_t) x + sqrt(1 - a_t) noise."""
    ac = alphas_cumprod.to(dtype=x.dtype)
    timesteps = torch.as_tensor(timesteps).reshape(-1).long()
    return _per_sample(ac[timesteps] ** 0.5, x) * x + _per_sample((1 - ac[timesteps]) ** 0.5, x) * noise


def add_noise_dpm(sigmas, x, noise, indices):
    """DPM-Solver / UniPC: alpha_t x + sigma_t noise from sigmas[index]."""
    sigma = _per_sample(sigmas.to(dtype=x.dtype)[indices], x)
    alpha_t = 1 / ((sigma ** 2 + 1) ** 0.5)
    sigma_t = sigma * alpha_t
    return alpha_t * x + sigma_t * noise


def add_noise_sigma(sigmas, x, noise, indices):
    """Euler / Euler ancestral / LMS: x + noise sigma."""
    return x + noise * _per_sample(sigmas.to(dtype=x.dtype)[indices], x)


def noise_index(schedule, timestep, begin_index, step_index):
    """diffusers' index rule of ``add_noise``: no begin index -> the timestep's entry of the schedule (the second when it occurs
    twice); a step index -> that; otherwise the begin index."""
    if begin_index is None:
        hits = [k for k, v in enumerate(schedule) if v == timestep]
        return hits[1] if len(hits) > 1 else hits[0]
    return step_index if step_index is not None else begin_index


# ---------------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------------
def get_t_start(num_inference_steps, strength):
    """diffusers' ``get_timesteps``."""
    init = min(int(num_inference_steps * strength), num_inference_steps)
    return max(num_inference_steps - init, 0)


def _kind(scheduler):
    if hasattr(scheduler, "index"):
        return "sigma"  # tests/euler_ref.py: a counter selects the step
    return "dpm" if hasattr(scheduler, "_step_index") else "vp"


def _noised(scheduler, z0, noise, k, timesteps):
    """add_noise(z0, noise, .) at entry ``k`` of the schedule, from the reference scheduler's own tables."""
    kind = _kind(scheduler)
    if kind == "vp":
        return add_noise_vp(scheduler.alphas_cumprod, z0, noise, timesteps[k:k + 1])
    if kind == "dpm":
        return add_noise_dpm(scheduler.sigmas, z0, noise, [k])
    return add_noise_sigma(torch.tensor(scheduler.sigmas, dtype=F32), z0, noise, [k])


@torch.no_grad()
def dual_img2img_loop(unet, gm_unet, scheduler, prompt_embeds, negative_prompt_embeds, z0, noise, num_inference_steps, strength,
                      mask=None, guidance_scale=7.5, generator=None, count=None):
    """The dual loop started from a picture's latents ``z0`` (already scaled), as the issue defines it:

    * the SDR branch enters the schedule at ``t_start * order`` from ``add_noise(z0, noise)`` (pure noise for a mask at strength 1);
    * the GM branch runs the whole schedule from ``noise * init_noise_sigma``; until the SDR branch enters, its SDR operand is z0;
    * with a mask, after every SDR step ``latents = (1 - m) keep + m latents`` with keep = z0 re-noised to the next timestep (z0 at
      the last) and the GM UNet's x0 is ``(1 - m) z0 + m x0``;
    * a shared generator is consumed by the GM scheduler alone before the SDR branch enters, SDR first and GM second afterwards.

    ``count``: a dict that receives the number of SDR / GM UNet evaluations.  Returns (latents, gm_latents)."""
    from oracle.pipelines import _cfg

    do_cfg = guidance_scale > 1
    embeds = torch.cat([negative_prompt_embeds, prompt_embeds]) if do_cfg else prompt_embeds
    gm_embeds = embeds[negative_prompt_embeds.shape[0]:] if do_cfg else embeds
    scheduler.set_timesteps(num_inference_steps)
    timesteps = scheduler.timesteps
    gm_scheduler = copy.deepcopy(scheduler)
    first = get_t_start(num_inference_steps, strength) * scheduler.order
    kind = _kind(scheduler)
    if kind == "sigma":
        scheduler.index = first
    elif kind == "dpm":
        scheduler._step_index = first
    gm_latents = noise * scheduler.init_noise_sigma
    if mask is not None and strength == 1.0:
        latents = noise * scheduler.init_noise_sigma
    else:
        latents = _noised(scheduler, z0, noise, first, timesteps)
    step_kw = {"generator": generator}
    n_sdr = n_gm = 0
    for i, t in enumerate(timesteps):
        if i >= first:
            x = torch.cat([latents] * 2) if do_cfg else latents
            eps = unet(scheduler.scale_model_input(x, t), t, encoder_hidden_states=embeds, return_dict=False)[0]
            n_sdr += 1
            if do_cfg:
                eps = _cfg(eps, guidance_scale, 0.0)
            if kind == "sigma":
                latents, x0 = scheduler.step(eps, t, latents, **step_kw, return_dict=False)
            else:
                a = scheduler.alphas_cumprod[t].view(-1, 1, 1, 1)
                x0 = (latents - (1 - a).sqrt() * eps) / a.sqrt()
                kw = step_kw if kind != "vp" or hasattr(scheduler, "eta") else {}  # the oracle's PNDM takes no generator
                latents = scheduler.step(eps, t, latents, **kw, return_dict=False)[0]
            if mask is not None:
                keep = z0 if i == len(timesteps) - 1 else _noised(scheduler, z0, noise, i + 1, timesteps)
                latents = (1 - mask) * keep + mask * latents
                x0 = (1 - mask) * z0 + mask * x0
        else:
            x0 = z0
        gm_x = gm_scheduler.scale_model_input(gm_latents, t) if kind == "sigma" else gm_latents
        gm_eps = gm_unet(torch.cat([x0, gm_x], dim=1), t, encoder_hidden_states=gm_embeds, return_dict=False)[0]
        n_gm += 1
        kw = step_kw if kind != "vp" or hasattr(gm_scheduler, "eta") else {}
        gm_latents = gm_scheduler.step(gm_eps, t, gm_latents, **kw, return_dict=False)[0]
    if count is not None:
        count.update(sdr=n_sdr, gm=n_gm)
    return latents, gm_latents
