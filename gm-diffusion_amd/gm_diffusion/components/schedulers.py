"""
Schedulers for the MI355X build: ``PNDMScheduler`` (PLMS, the "50 PNDM steps" configuration of
scripts/stage2/train_gm_unet.py:171-176), ``DDPMScheduler`` (scripts/inference/generate_hdr.py:162),
``DDIMScheduler`` (scripts/stage2/train_gm_unet.py:48, scheduler_tuning.py:178-188),
``LCMScheduler`` (few-step sampling of a guidance-embedded UNet), ``DPMSolverMultistepScheduler``, ``UniPCMultistepScheduler`` (predictor-corrector) and the sigma-space ``EulerDiscreteScheduler`` / ``EulerAncestralDiscreteScheduler`` /
``LMSDiscreteScheduler`` (the only ones whose ``init_noise_sigma`` and ``scale_model_input`` do something).  In the reference they come from ``diffusers``; these
classes keep the protocol the pipelines rely on (stable_diffusion_gm.py:216-241, 610-625, 715,
1037, 1048, 1071; stable_diffusion_dual_unet.py:1037, 1072): ``config`` (dict-like, attribute
access), ``set_timesteps``, ``timesteps``, ``order``, ``init_noise_sigma``,
``scale_model_input``, ``step(...)``, ``alphas_cumprod``, ``from_config`` and survival under
``copy.deepcopy``; for img2img and inpainting also diffusers' ``add_noise`` (every class), ``set_begin_index`` / ``begin_index`` (the
classes that select a step by ``step_index``) and the host query ``add_noise_coefs(t)``: the float32 pair with
``add_noise == ca * x + cb * noise`` that the fused blend kernel takes.

The schedulers are host-side state machines; the per-element update runs in the
``gmd_latent_step`` HIP kernel for device tensors (same float32 operation order as the torch
expressions, so the two agree bit for bit) and in plain torch for host tensors, which is what the
reference itself executes on CPU tensors.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np
import torch

from .. import hip_ops as ops
from .configuration import ConfigMixin
from .image_processor import _Output, randn_tensor


@dataclass
class SchedulerOutput(_Output):
    prev_sample: torch.Tensor


@dataclass
class DDIMSchedulerOutput(_Output):
    prev_sample: torch.Tensor
    pred_original_sample: torch.Tensor = None


def _betas(beta_schedule, beta_start, beta_end, n, trained_betas=None):
    if trained_betas is not None:
        return torch.tensor(trained_betas, dtype=torch.float32)
    if beta_schedule == "linear":
        return torch.linspace(beta_start, beta_end, n, dtype=torch.float32)
    if beta_schedule == "scaled_linear":
        return torch.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=torch.float32) ** 2
    raise NotImplementedError(f"{beta_schedule} is not implemented")


class _SchedulerBase(ConfigMixin):
    config_name = "scheduler_config.json"
    order = 1

    @classmethod
    def from_pretrained(cls, path, subfolder=None, **overrides):
        d = os.path.join(path, subfolder) if subfolder else path
        return cls.from_config(cls.load_config(d), **overrides)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def __len__(self):
        return self.config.num_train_timesteps

    # ---- what the pipelines ask a scheduler (stable_diffusion_gm.py: _use_fused, _predraw_step_noise) ------------------------------
    has_fused_step = True  # ``fused_step`` runs the CFG combine, x0 and the update as ONE HIP kernel pass on device tensors
    predraws_noise = False  # True: ``step`` consumes the generator, and the pipelines may draw the noise of every step up front

    def draws_noise(self, timestep, eta=0.0):
        """True when ``step`` at this timestep consumes the generator.  Here: never, the step is deterministic."""
        return False

    # ---- what the constructors share -----------------------------------------------------------------------------------------------
    def _merge_config(self, kwargs):
        """``_defaults`` overridden by ``kwargs`` as a dict; a key ``_defaults`` does not hold is refused."""
        cfg = dict(self._defaults)
        bad = [k for k in kwargs if k not in cfg]
        if bad:
            raise TypeError(f"{type(self).__name__}: unexpected arguments {bad}")
        cfg.update(kwargs)
        return cfg

    def _register_betas(self, cfg):
        """``cfg`` becomes ``self.config``; ``betas``, ``alphas`` and ``alphas_cumprod`` are the float32 tables of diffusers."""
        self.register_to_config(**cfg)
        self.betas = _betas(cfg["beta_schedule"], cfg["beta_start"], cfg["beta_end"], cfg["num_train_timesteps"], cfg["trained_betas"])
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)

    # ---- what the device steps share -----------------------------------------------------------------------------------------------
    @staticmethod
    def _on_device(model_output, sample):
        """True when ``step`` runs as the fused HIP kernel: float32 device tensors."""
        return model_output.is_cuda and model_output.dtype == torch.float32 and sample.dtype == torch.float32

    @staticmethod
    def _guidance_ratio(eps_in, do_cfg, guidance_scale, guidance_rescale):
        """The per-sample std ratio of ``rescale_noise_cfg`` (one reduction kernel), or None when the step does not rescale."""
        return ops.cfg_std_ratio(eps_in, guidance_scale) if (do_cfg and guidance_rescale > 0.0) else None

    @staticmethod
    def _step_noise(sample, generator):
        """One step's noise for a device step, drawn where ``step`` draws it: float32, on the sample's device."""
        return randn_tensor(sample.shape, generator=generator, device=sample.device, dtype=torch.float32)

    @staticmethod
    def _x0_coefs(a):
        """(sqrt(a), sqrt(1 - a)) of the pipeline's own x0 (dual_unet.py:1072-1075), from ``alphas_cumprod`` of the loop timestep."""
        return a.sqrt().item(), (1 - a).sqrt().item()

    # ---- forward noising: where img2img starts and what inpainting keeps (diffusers' ``add_noise``) ----------------------------------
    def add_noise_coefs(self, timestep):
        """The two float32 values ``(ca, cb)``, as Python floats, with ``add_noise(x, noise, [timestep]) == ca * x + cb * noise``: what
        the pipelines hand to ``hip_ops.inpaint_blend``.  Here the variance-preserving pair of diffusers' PNDM / DDPM / DDIM / LCM
        classes, ``alphas_cumprod[t] ** 0.5`` and ``(1 - alphas_cumprod[t]) ** 0.5`` on the float32 table."""
        a = self.alphas_cumprod[int(timestep)]
        return (a ** 0.5).item(), ((1 - a) ** 0.5).item()

    @staticmethod
    def _per_sample(coef, like):
        """A per-timestep coefficient [n] shaped to broadcast over ``like`` ([n | any, ...]), as diffusers does it."""
        coef = coef.flatten()
        while coef.dim() < like.dim():
            coef = coef.unsqueeze(-1)
        return coef

    def add_noise(self, original_samples, noise, timesteps):
        """diffusers' ``add_noise`` of the variance-preserving classes: ``timesteps`` holds one integer timestep, or one per sample."""
        timesteps = torch.as_tensor(timesteps).reshape(-1).to(device=original_samples.device, dtype=torch.long)
        alphas_cumprod = self.alphas_cumprod.to(device=original_samples.device, dtype=original_samples.dtype)
        sqrt_alpha_prod = self._per_sample(alphas_cumprod[timesteps] ** 0.5, original_samples)
        sqrt_one_minus_alpha_prod = self._per_sample((1 - alphas_cumprod[timesteps]) ** 0.5, original_samples)
        return sqrt_alpha_prod * original_samples + sqrt_one_minus_alpha_prod * noise


class _StepIndexMixin:
    """What the classes that select a step by ``step_index`` share beyond it: diffusers' ``set_begin_index`` / ``begin_index`` (an
    img2img pipeline enters the schedule part-way down and says so before the first ``step``) and the index rule of ``add_noise``.
    ``set_timesteps`` resets the begin index, as in diffusers.  A class gives ``_index_for_timestep``."""

    _begin_index = None

    @property
    def begin_index(self):
        return self._begin_index

    def set_begin_index(self, begin_index=0):
        self._begin_index = int(begin_index)

    def _init_step_index(self, timestep):
        self._step_index = self._index_for_timestep(timestep) if self._begin_index is None else self._begin_index

    def _noise_indices(self, timesteps):
        """diffusers' rule: no begin index (training, or a pipeline that sets none) -> the timestep's own entry; a step index already
        set -> that one (the inpaint re-noise after a step, to the level of the next one); otherwise the begin index (the start of
        img2img, before the first step)."""
        if self._begin_index is None:
            return [self._index_for_timestep(t) for t in timesteps]
        return [self._begin_index if self._step_index is None else self._step_index] * len(timesteps)


class PNDMScheduler(_SchedulerBase):
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                     trained_betas=None, skip_prk_steps=False, set_alpha_to_one=False, prediction_type="epsilon",
                     timestep_spacing="leading", steps_offset=0, clip_sample=False)

    def __init__(self, **kwargs):
        cfg = self._merge_config(kwargs)
        if cfg["prediction_type"] != "epsilon":
            raise NotImplementedError("only epsilon prediction is implemented")
        self._register_betas(cfg)
        self.final_alpha_cumprod = torch.tensor(1.0) if cfg["set_alpha_to_one"] else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.pndm_order = 4
        self.cur_model_output = 0
        self.counter = 0
        self.cur_sample = None
        self.ets = []
        self.num_inference_steps = None
        self._timesteps = np.arange(0, cfg["num_train_timesteps"])[::-1].copy()
        self.prk_timesteps = None
        self.plms_timesteps = None
        self.timesteps = None

    def set_timesteps(self, num_inference_steps, device=None):
        c = self.config
        self.num_inference_steps = num_inference_steps
        if c.timestep_spacing == "linspace":
            self._timesteps = np.linspace(0, c.num_train_timesteps - 1, num_inference_steps).round().astype(np.int64)
        elif c.timestep_spacing == "leading":
            ratio = c.num_train_timesteps // num_inference_steps
            self._timesteps = (np.arange(0, num_inference_steps) * ratio).round()
            self._timesteps += c.steps_offset
        elif c.timestep_spacing == "trailing":
            ratio = c.num_train_timesteps / num_inference_steps
            self._timesteps = np.round(np.arange(c.num_train_timesteps, 0, -ratio))[::-1].astype(np.int64)
            self._timesteps -= 1
        else:
            raise ValueError(f"{c.timestep_spacing} is not supported")
        if c.skip_prk_steps:
            self.prk_timesteps = np.array([])
            self.plms_timesteps = np.concatenate([self._timesteps[:-1], self._timesteps[-2:-1], self._timesteps[-1:]])[::-1].copy()
        else:
            raise NotImplementedError("Runge-Kutta warm-up (skip_prk_steps=False) is not implemented; SD-1.5 uses skip_prk_steps=True")
        timesteps = np.concatenate([self.prk_timesteps, self.plms_timesteps]).astype(np.int64)
        self.timesteps = torch.from_numpy(timesteps).to(device)
        self.ets = []
        self.counter = 0
        self.cur_model_output = 0
        self.cur_sample = None

    # ---- PLMS planning (host) ------------------------------------------------------------------
    def _plan(self, timestep):
        """Which PLMS branch the next step takes: (mode, effective timestep, previous timestep)."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        timestep = int(timestep)
        ratio = self.config.num_train_timesteps // self.num_inference_steps
        prev = timestep - ratio
        n_after = len(self.ets[-3:]) + 1 if self.counter != 1 else len(self.ets)
        if self.counter == 1:
            prev, timestep = timestep, timestep + ratio
        if n_after == 1 and self.counter == 0:
            mode = 0
        elif n_after == 1 and self.counter == 1:
            mode = 1
        else:
            mode = min(n_after, 4)
        return mode, timestep, prev

    def _coefs(self, timestep, prev_timestep):
        """diffusers ``_get_prev_sample`` coefficients, evaluated on float32 0-d tensors exactly as there."""
        a_t = self.alphas_cumprod[timestep]
        a_prev = self.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod
        b_t, b_prev = 1 - a_t, 1 - a_prev
        sample_coeff = (a_prev / a_t) ** 0.5
        denom = a_t * b_prev ** 0.5 + (a_t * b_t * a_prev) ** 0.5
        return sample_coeff, a_prev - a_t, denom

    def _commit(self, mode, eps, sample):
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(eps)
        if mode == 0:
            self.cur_sample = sample
        elif mode == 1:
            self.cur_sample = None
        self.counter += 1

    def step(self, model_output, timestep, sample, return_dict=True):
        mode, t_eff, prev = self._plan(timestep)
        sc, ad, dn = self._coefs(t_eff, prev)
        if model_output.is_cuda:
            hist = [e for e in reversed(self.ets[-3:])] if self.counter != 1 else [self.ets[-1]]
            x = sample.contiguous()
            nh = {0: 0, 1: 1, 2: 1, 3: 2, 4: 3}[mode]
            eps_copy, prev_sample, _ = ops.latent_step(model_output.contiguous(), x, mode, (sc.item(), ad.item(), dn.item(), 1.0, 0.0),
                                                       False, 1.0, cur_sample=self.cur_sample, hist=hist[:nh])
            # keep the kernel's private copy in the history: `model_output` may be the static output buffer of a
            # captured graph that the next replay overwrites
            self._commit(mode, eps_copy, sample)
        else:
            e = (self.ets[-3:] + [model_output]) if self.counter != 1 else self.ets
            smp = sample
            if mode == 0:
                m = model_output
            elif mode == 1:
                m = (model_output + e[-1]) / 2
                smp = self.cur_sample
            elif mode == 2:
                m = (3 * e[-1] - e[-2]) / 2
            elif mode == 3:
                m = (23 * e[-1] - 16 * e[-2] + 5 * e[-3]) / 12
            else:
                m = (1 / 24) * (55 * e[-1] - 59 * e[-2] + 37 * e[-3] - 9 * e[-4])
            prev_sample = sc * smp - ad * m / dn
            self._commit(mode, model_output, sample)
        return (prev_sample,) if not return_dict else SchedulerOutput(prev_sample=prev_sample)

    def fused_step(self, eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale=0.0, want_x0=False):
        """CFG combine (+rescale) + x0 + PLMS update in ONE HIP kernel pass (device tensors only).
        eps_in: raw UNet output ([2B,...] when do_cfg).  Returns (prev_sample, x0 | None)."""
        mode, t_eff, prev = self._plan(timestep)
        sc, ad, dn = self._coefs(t_eff, prev)
        a = self.alphas_cumprod[int(timestep)]  # dual_unet.py:1072 uses the loop timestep
        ratio = self._guidance_ratio(eps_in, do_cfg, guidance_scale, guidance_rescale)
        hist = [e for e in reversed(self.ets[-3:])] if self.counter != 1 else [self.ets[-1]]
        nh = {0: 0, 1: 1, 2: 1, 3: 2, 4: 3}[mode]
        eps, prev_sample, x0 = ops.latent_step(eps_in, sample.contiguous(), mode, (sc.item(), ad.item(), dn.item(), *self._x0_coefs(a)),
                                               do_cfg, guidance_scale, cur_sample=self.cur_sample, hist=hist[:nh], ratio=ratio,
                                               guidance_rescale=guidance_rescale, want_x0=want_x0)
        self._commit(mode, eps, sample)
        return prev_sample, x0


class DDPMScheduler(_SchedulerBase):
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     variance_type="fixed_small", clip_sample=True, prediction_type="epsilon", thresholding=False,
                     dynamic_thresholding_ratio=0.995, clip_sample_range=1.0, sample_max_value=1.0,
                     timestep_spacing="leading", steps_offset=0, rescale_betas_zero_snr=False)

    def __init__(self, **kwargs):
        cfg = self._merge_config(kwargs)
        if cfg["prediction_type"] != "epsilon" or cfg["thresholding"] or cfg["rescale_betas_zero_snr"]:
            raise NotImplementedError("only epsilon prediction without thresholding / zero-SNR rescale is implemented")
        if cfg["variance_type"] not in ("fixed_small", "fixed_small_log", "fixed_large"):
            raise NotImplementedError(cfg["variance_type"])
        self._register_betas(cfg)
        self.one = torch.tensor(1.0)
        self.init_noise_sigma = 1.0
        self.custom_timesteps = False
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, cfg["num_train_timesteps"])[::-1].copy())

    def set_timesteps(self, num_inference_steps=None, device=None, timesteps=None):
        c = self.config
        if timesteps is not None:
            timesteps = np.array(timesteps, dtype=np.int64)
            self.custom_timesteps = True
            self.num_inference_steps = len(timesteps)
        else:
            if num_inference_steps > c.num_train_timesteps:
                raise ValueError("num_inference_steps cannot exceed num_train_timesteps")
            self.num_inference_steps = num_inference_steps
            self.custom_timesteps = False
            if c.timestep_spacing == "linspace":
                timesteps = np.linspace(0, c.num_train_timesteps - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
            elif c.timestep_spacing == "leading":
                ratio = c.num_train_timesteps // num_inference_steps
                timesteps = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64)
                timesteps += c.steps_offset
            elif c.timestep_spacing == "trailing":
                ratio = c.num_train_timesteps / num_inference_steps
                timesteps = np.round(np.arange(c.num_train_timesteps, 0, -ratio)).astype(np.int64) - 1
            else:
                raise ValueError(f"{c.timestep_spacing} is not supported")
        self.timesteps = torch.from_numpy(timesteps).to(device)

    def previous_timestep(self, timestep):
        if self.custom_timesteps:
            idx = (self.timesteps == timestep).nonzero(as_tuple=True)[0][0]
            return torch.tensor(-1) if idx == self.timesteps.shape[0] - 1 else self.timesteps[idx + 1]
        n = self.num_inference_steps if self.num_inference_steps else self.config.num_train_timesteps
        return timestep - self.config.num_train_timesteps // n

    def _get_variance(self, t):
        prev_t = self.previous_timestep(t)
        a_t = self.alphas_cumprod[t]
        a_p = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
        cur_b = 1 - a_t / a_p
        variance = torch.clamp((1 - a_p) / (1 - a_t) * cur_b, min=1e-20)
        vt = self.config.variance_type
        if vt == "fixed_small_log":
            variance = torch.exp(0.5 * torch.log(variance))
        elif vt == "fixed_large":
            variance = cur_b
        return variance

    predraws_noise = True

    def draws_noise(self, timestep, eta=0.0):
        """True when ``step`` at this timestep consumes the generator (every step but t == 0)."""
        return int(timestep) > 0

    def _device_step(self, eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale, want_x0, generator, noise=None):
        """One HIP kernel pass (gmd_ddpm_step): CFG combine (+rescale), pipeline x0, clipped x0 prediction, posterior mean
        and the variance noise.  The noise is drawn HERE with ``randn_tensor`` exactly where ``step`` draws it, so the
        generator the dual pipeline shares between its two schedulers (stable_diffusion_dual_unet.py:1015, 1077, 1093) is
        consumed in the reference's order."""
        t = int(timestep)
        prev_t = int(self.previous_timestep(t))
        a_t = self.alphas_cumprod[t]
        a_p = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
        b_t, b_p = 1 - a_t, 1 - a_p
        cur_a = a_t / a_p
        cur_b = 1 - cur_a
        x0_coeff = (a_p ** 0.5 * cur_b) / b_t
        xt_coeff = cur_a ** 0.5 * b_p / b_t
        scale = 0.0  # (noise: the caller's pre-drawn tensor, or drawn below)
        if t > 0:
            if noise is None:  # (the pipelines pre-draw a CPU generator's noise for all steps, in call order: see fused_step)
                noise = self._step_noise(sample, generator)
            v = self._get_variance(t)
            scale = (v if self.config.variance_type == "fixed_small_log" else v ** 0.5).item()
        ratio = self._guidance_ratio(eps_in, do_cfg, guidance_scale, guidance_rescale)
        return ops.ddpm_step(eps_in.contiguous(), sample.contiguous(),
                             ((a_t ** 0.5).item(), (b_t ** 0.5).item(), x0_coeff.item(), xt_coeff.item(), scale, *self._x0_coefs(a_t)),
                             do_cfg, guidance_scale, noise=noise, ratio=ratio, guidance_rescale=guidance_rescale,
                             clip_range=self.config.clip_sample_range if self.config.clip_sample else None, want_x0=want_x0)

    def fused_step(self, eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale=0.0, want_x0=False, generator=None, noise=None):
        """Same contract as ``PNDMScheduler.fused_step`` plus the generator (device float32 tensors only).
        ``noise``: this step's variance noise already drawn from ``generator`` by the caller (a CPU generator forces a
        synchronous host draw + copy per step; the pipelines draw all steps up front, in the order the steps consume
        them, so the host keeps running ahead of the GPU).  Returns (prev_sample, x0 | None)."""
        return self._device_step(eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale, want_x0, generator, noise)

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, noise=None):
        if self._on_device(model_output, sample):
            prev, _ = self._device_step(model_output, timestep, sample, False, 1.0, 0.0, False, generator, noise)
            return (prev,) if not return_dict else SchedulerOutput(prev_sample=prev)
        return self._host_step(model_output, timestep, sample, generator, return_dict)

    def _host_step(self, model_output, timestep, sample, generator=None, return_dict=True):
        """The torch expressions of diffusers' ``DDPMScheduler.step`` (host tensors; also the reference for the kernel test)."""
        t = int(timestep)
        prev_t = int(self.previous_timestep(t))
        a_t = self.alphas_cumprod[t]
        a_p = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
        b_t, b_p = 1 - a_t, 1 - a_p
        cur_a = a_t / a_p
        cur_b = 1 - cur_a
        dev = model_output.device
        x0 = (sample - (b_t ** 0.5).to(dev) * model_output) / (a_t ** 0.5).to(dev)
        if self.config.clip_sample:
            x0 = x0.clamp(-self.config.clip_sample_range, self.config.clip_sample_range)
        x0_coeff = ((a_p ** 0.5 * cur_b) / b_t).to(dev)
        xt_coeff = (cur_a ** 0.5 * b_p / b_t).to(dev)
        prev = x0_coeff * x0 + xt_coeff * sample
        if t > 0:
            noise = randn_tensor(model_output.shape, generator=generator, device=dev, dtype=model_output.dtype)
            v = self._get_variance(t).to(dev)
            prev = prev + (v * noise if self.config.variance_type == "fixed_small_log" else (v ** 0.5) * noise)
        return (prev,) if not return_dict else SchedulerOutput(prev_sample=prev)


class DDIMScheduler(_SchedulerBase):
    """DDIM: the deterministic single-history sampler the pipelines' docstrings name first (stable_diffusion_gm.py:188,
    stable_diffusion_dual_unet.py:188; scripts/stage2/train_gm_unet.py:48, scripts/stage2/experiments/scheduler_tuning.py:178-188)
    and the one scheduler that uses their ``eta`` argument (:612, :843): ``eta`` = 0 is DDIM, 1 is DDPM's variance.  Implements
    diffusers' epsilon-prediction path with ``clip_sample`` and ``use_clipped_model_output``; v-prediction, thresholding and
    zero-SNR betas raise NotImplementedError.  It keeps no history.  ``step`` / ``fused_step`` run as ONE HIP kernel
    (gmd_ddim_step) for float32 device tensors, as the same torch expressions (``_host_step``) otherwise."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     clip_sample=True, set_alpha_to_one=True, steps_offset=0, prediction_type="epsilon", thresholding=False,
                     dynamic_thresholding_ratio=0.995, clip_sample_range=1.0, sample_max_value=1.0,
                     timestep_spacing="leading", rescale_betas_zero_snr=False)

    def __init__(self, **kwargs):
        cfg = self._merge_config(kwargs)
        if cfg["prediction_type"] != "epsilon" or cfg["thresholding"] or cfg["rescale_betas_zero_snr"]:
            raise NotImplementedError("only epsilon prediction without thresholding / zero-SNR rescale is implemented")
        self._register_betas(cfg)
        self.final_alpha_cumprod = torch.tensor(1.0) if cfg["set_alpha_to_one"] else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, cfg["num_train_timesteps"])[::-1].copy().astype(np.int64))

    def set_timesteps(self, num_inference_steps, device=None):
        c = self.config
        if num_inference_steps > c.num_train_timesteps:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than `self.config.train_timesteps`:"
                             f" {c.num_train_timesteps} as the unet model trained with this scheduler can only handle"
                             f" maximal {c.num_train_timesteps} timesteps.")
        self.num_inference_steps = num_inference_steps
        if c.timestep_spacing == "linspace":
            timesteps = np.linspace(0, c.num_train_timesteps - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
        elif c.timestep_spacing == "leading":
            ratio = c.num_train_timesteps // num_inference_steps
            timesteps = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64)
            timesteps += c.steps_offset
        elif c.timestep_spacing == "trailing":
            ratio = c.num_train_timesteps / num_inference_steps
            timesteps = np.round(np.arange(c.num_train_timesteps, 0, -ratio)).astype(np.int64)
            timesteps -= 1
        else:
            raise ValueError(f"{c.timestep_spacing} is not supported. Please make sure to choose one of 'leading' or 'trailing'.")
        self.timesteps = torch.from_numpy(timesteps).to(device)

    predraws_noise = True

    def draws_noise(self, timestep, eta=0.0):
        """True when ``step`` at this timestep consumes the generator: iff eta > 0, at EVERY step (the last one included, where
        the standard deviation may be 0) -- n steps take n draws, where DDPM takes n - 1 when it reaches t == 0."""
        return eta > 0

    def _coefs(self, timestep, eta):
        """The step's coefficients as float32 0-d tensors, evaluated exactly as diffusers' ``DDIMScheduler.step`` evaluates them:
        (a_t ** 0.5, (1 - a_t) ** 0.5, a_prev ** 0.5, (1 - a_prev - std^2) ** 0.5, std = eta * variance ** 0.5, a_t)."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        b_t, b_prev = 1 - a_t, 1 - a_prev
        variance = (b_prev / b_t) * (1 - a_t / a_prev)  # _get_variance
        std = eta * variance ** 0.5
        dir_coeff = (1 - a_prev - std ** 2) ** 0.5
        return a_t ** 0.5, b_t ** 0.5, a_prev ** 0.5, dir_coeff, std, a_t

    def _device_step(self, eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale, want_x0, generator, noise=None,
                     eta=0.0, use_clipped_model_output=False, want_pred_x0=False):
        """One HIP kernel pass (gmd_ddim_step): CFG combine (+rescale), pipeline x0, clipped x0 prediction, the DDIM update and
        the variance noise.  The noise is drawn HERE with ``randn_tensor`` exactly where ``step`` draws it (iff eta > 0), so a
        generator shared by the two schedulers of the dual pipeline is consumed in the reference's order.
        Returns (prev_sample, x0 | None, pred_original_sample | None)."""
        sa, s1, sp, dc, sd, a_t = self._coefs(timestep, eta)
        if eta > 0:
            if noise is None:  # (the pipelines pre-draw a CPU generator's noise for all steps, in call order: see fused_step)
                noise = self._step_noise(sample, generator)
        else:
            noise = None
        ratio = self._guidance_ratio(eps_in, do_cfg, guidance_scale, guidance_rescale)
        return ops.ddim_step(eps_in.contiguous(), sample.contiguous(),
                             (sa.item(), s1.item(), sp.item(), dc.item(), sd.item(), *self._x0_coefs(a_t)),
                             do_cfg, guidance_scale, noise=noise, ratio=ratio, guidance_rescale=guidance_rescale,
                             clip_range=self.config.clip_sample_range if self.config.clip_sample else None,
                             use_clipped=use_clipped_model_output, want_x0=want_x0, want_pred_x0=want_pred_x0)

    def fused_step(self, eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale=0.0, want_x0=False, generator=None, noise=None,
                   eta=0.0, use_clipped_model_output=False):
        """Same contract as ``DDPMScheduler.fused_step`` plus ``eta`` / ``use_clipped_model_output`` (device float32 tensors
        only).  ``noise``: this step's variance noise already drawn from ``generator`` by the caller; used iff eta > 0.
        Returns (prev_sample, x0 | None)."""
        prev, x0, _ = self._device_step(eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale, want_x0, generator, noise,
                                        eta, use_clipped_model_output)
        return prev, x0

    def step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None, variance_noise=None,
             return_dict=True, noise=None):
        """diffusers' signature; ``noise`` (not in diffusers) is the pipelines' pre-drawn tensor: what ``generator`` would have
        given at this step, so it may come together with the generator."""
        if generator is not None and variance_noise is not None:
            raise ValueError("Cannot pass both generator and variance_noise. Please make sure that either `generator` or"
                             " `variance_noise` stays `None`.")
        if variance_noise is None:
            variance_noise = noise
        if self._on_device(model_output, sample):
            prev, _, p0 = self._device_step(model_output, timestep, sample, False, 1.0, 0.0, False, generator, variance_noise, eta,
                                            use_clipped_model_output, want_pred_x0=True)
            return (prev, p0) if not return_dict else DDIMSchedulerOutput(prev_sample=prev, pred_original_sample=p0)
        return self._host_step(model_output, timestep, sample, eta, use_clipped_model_output, generator, variance_noise, return_dict)

    def _host_step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None, variance_noise=None,
                   return_dict=True):
        """The torch expressions of diffusers' ``DDIMScheduler.step`` (host tensors; also the reference for the kernel test)."""
        dev = model_output.device
        sa, s1, sp, dc, sd, _ = (c.to(dev) for c in self._coefs(timestep, eta))
        p0 = (sample - s1 * model_output) / sa
        pred_epsilon = model_output
        if self.config.clip_sample:
            p0 = p0.clamp(-self.config.clip_sample_range, self.config.clip_sample_range)
        if use_clipped_model_output:
            pred_epsilon = (sample - sa * p0) / s1
        prev = sp * p0 + dc * pred_epsilon
        if eta > 0:
            if variance_noise is None:
                variance_noise = randn_tensor(model_output.shape, generator=generator, device=dev, dtype=model_output.dtype)
            prev = prev + sd * variance_noise
        return (prev, p0) if not return_dict else DDIMSchedulerOutput(prev_sample=prev, pred_original_sample=p0)


@dataclass
class LCMSchedulerOutput(_Output):
    prev_sample: torch.Tensor
    denoised: torch.Tensor = None


class LCMScheduler(_StepIndexMixin, _SchedulerBase):
    """Latent-consistency (LCM) multistep sampling: the few-step scheduler (2-8 steps) of a guidance-embedded UNet (config
    ``time_cond_proj_dim``; the branch of the reference pipelines at stable_diffusion_gm.py:1028-1034), which runs without the
    classifier-free-guidance duplicate.  Restates diffusers' ``LCMScheduler`` for epsilon prediction with ``clip_sample``;
    v-prediction / sample prediction, thresholding and zero-SNR betas raise NotImplementedError.  Each step predicts x0, applies the
    boundary-condition scalings (``denoised = c_out * x0 + c_skip * x``) and, at every step but the last, re-noises the result to
    the next timestep of the schedule: n steps take n - 1 draws, as with DDPM.  ``step`` / ``fused_step`` run as ONE HIP kernel
    (gmd_lcm_step) for float32 device tensors, as the same torch expressions (``_host_step``) otherwise."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", trained_betas=None,
                     original_inference_steps=50, clip_sample=False, clip_sample_range=1.0, set_alpha_to_one=True, steps_offset=0,
                     prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0,
                     timestep_spacing="leading", timestep_scaling=10.0, rescale_betas_zero_snr=False)

    def __init__(self, **kwargs):
        cfg = self._merge_config(kwargs)
        if cfg["prediction_type"] != "epsilon" or cfg["thresholding"] or cfg["rescale_betas_zero_snr"]:
            raise NotImplementedError("only epsilon prediction without thresholding / zero-SNR rescale is implemented")
        self._register_betas(cfg)
        self.final_alpha_cumprod = torch.tensor(1.0) if cfg["set_alpha_to_one"] else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.custom_timesteps = False
        self.timesteps = torch.from_numpy(np.arange(0, cfg["num_train_timesteps"])[::-1].copy().astype(np.int64))
        self._ts_host = [int(v) for v in self.timesteps]
        self._step_index = None

    @property
    def step_index(self):
        return self._step_index

    def set_timesteps(self, num_inference_steps=None, device=None, original_inference_steps=None, timesteps=None, strength=1.0):
        """The LCM schedule: the ``original_inference_steps`` training timesteps ``k, 2k, ... - 1`` (k = num_train_timesteps //
        original_inference_steps; the first ``strength`` of them), reversed, then ``num_inference_steps`` of those picked at evenly
        spaced indices.  ``timesteps=`` gives a custom strictly descending schedule instead."""
        c = self.config
        if num_inference_steps is None and timesteps is None:
            raise ValueError("Must pass exactly one of `num_inference_steps` or `timesteps`.")
        if num_inference_steps is not None and timesteps is not None:
            raise ValueError("Can only pass one of `num_inference_steps` or `timesteps`.")
        orig = original_inference_steps if original_inference_steps is not None else c.original_inference_steps
        if orig > c.num_train_timesteps:
            raise ValueError(f"`original_steps`: {orig} cannot be larger than `self.config.train_timesteps`: {c.num_train_timesteps}"
                             " as the unet model trained with this scheduler can only handle maximal"
                             f" {c.num_train_timesteps} timesteps.")
        k = c.num_train_timesteps // orig
        origin = np.arange(1, int(orig * strength) + 1) * k - 1
        if timesteps is not None:
            ts = np.array(timesteps, dtype=np.int64)
            if ts.ndim != 1 or len(ts) == 0:
                raise ValueError("`timesteps` must be a non-empty list of ints.")
            if any(ts[i] >= ts[i - 1] for i in range(1, len(ts))):
                raise ValueError("`timesteps` must be in descending order.")
            if ts[0] >= c.num_train_timesteps:
                raise ValueError(f"`timesteps` must start before `self.config.train_timesteps`: {c.num_train_timesteps}.")
            if ts[-1] < 0:
                raise ValueError("`timesteps` must not be negative.")
            num_inference_steps = len(ts)
            self.custom_timesteps = True
        else:
            if num_inference_steps > c.num_train_timesteps:
                raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than `self.config.train_timesteps`:"
                                 f" {c.num_train_timesteps} as the unet model trained with this scheduler can only handle"
                                 f" maximal {c.num_train_timesteps} timesteps.")
            if num_inference_steps > orig:
                raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than `original_inference_steps`: {orig}"
                                 " because the final timestep schedule will be a subset of the `original_inference_steps`-sized"
                                 " initial timestep schedule.")
            skipping = len(origin) // num_inference_steps if num_inference_steps > 0 else 0
            if skipping < 1:
                raise ValueError(f"The combination of `original_steps x strength`: {orig} x {strength} is smaller than"
                                 f" `num_inference_steps`: {num_inference_steps}. Make sure to either reduce `num_inference_steps` to a"
                                 f" value smaller than {int(orig * strength)} or increase `strength` to a value higher than"
                                 f" {float(num_inference_steps / orig)}.")
            origin = origin[::-1].copy()
            idx = np.floor(np.linspace(0, len(origin), num=num_inference_steps, endpoint=False)).astype(np.int64)
            ts = origin[idx].astype(np.int64)
            self.custom_timesteps = False
        self.num_inference_steps = num_inference_steps
        self.timesteps = torch.from_numpy(ts).to(device=device, dtype=torch.long)
        self._ts_host = [int(v) for v in ts]
        self._step_index = None
        self._begin_index = None

    def _index_for_timestep(self, timestep):
        t = int(timestep)
        idx = [k for k, v in enumerate(self._ts_host) if v == t]
        if not idx:
            raise ValueError(f"timestep {t} is not in the schedule {self._ts_host}")
        return idx[1] if len(idx) > 1 else idx[0]

    predraws_noise = True

    def draws_noise(self, timestep, eta=0.0):
        """True when ``step`` at this timestep consumes the generator: every step but the schedule's last."""
        return int(timestep) != self._ts_host[-1]

    def get_scalings_for_boundary_condition_discrete(self, timestep):
        """(c_skip, c_out) of the consistency model's boundary condition, in Python floats: sigma_data = 0.5."""
        s = int(timestep) * self.config.timestep_scaling
        return 0.25 / (s * s + 0.25), s / (s * s + 0.25) ** 0.5

    def _plan(self, timestep):
        """Host side of one step: (last, the step's coefficients as float32 0-d tensors) -- a_t ** 0.5, (1 - a_t) ** 0.5, c_skip,
        c_out, a_prev ** 0.5, (1 - a_prev) ** 0.5, a_t -- with the previous timestep taken from the schedule (the timestep itself
        at the last step).  c_skip / c_out are evaluated in Python floats and rounded to float32 once."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self._step_index is None:
            self._init_step_index(timestep)
        t = int(timestep)
        nxt = self._step_index + 1
        last = nxt >= len(self._ts_host)
        prev_t = t if last else self._ts_host[nxt]
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        c_skip, c_out = self.get_scalings_for_boundary_condition_discrete(t)
        f32 = lambda v: torch.tensor(v, dtype=torch.float32)
        return last, (a_t ** 0.5, (1 - a_t) ** 0.5, f32(c_skip), f32(c_out), a_prev ** 0.5, (1 - a_prev) ** 0.5, a_t)

    def _device_step(self, eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale, want_x0, generator, noise=None,
                     want_denoised=False):
        """One HIP kernel pass (gmd_lcm_step): CFG combine (+rescale), pipeline x0, (clipped) x0 prediction, boundary scalings and
        the re-noising.  The noise is drawn HERE with ``randn_tensor`` exactly where ``step`` draws it (every step but the last), so
        a generator shared by the two schedulers of the dual pipeline is consumed in the reference's order.
        Returns (prev_sample, x0 | None, denoised | None)."""
        last, (sa, s1, cs, co, sp, bp, a_t) = self._plan(timestep)
        if last:
            noise = None
        elif noise is None:  # (the pipelines pre-draw a CPU generator's noise for all steps, in call order: see fused_step)
            noise = self._step_noise(sample, generator)
        ratio = self._guidance_ratio(eps_in, do_cfg, guidance_scale, guidance_rescale)
        out = ops.lcm_step(eps_in.contiguous(), sample.contiguous(),
                           (sa.item(), s1.item(), cs.item(), co.item(), sp.item(), bp.item(), *self._x0_coefs(a_t)),
                           do_cfg, guidance_scale, noise=noise, ratio=ratio, guidance_rescale=guidance_rescale,
                           clip_range=self.config.clip_sample_range if self.config.clip_sample else None,
                           want_x0=want_x0, want_denoised=want_denoised)
        self._step_index += 1
        return out

    def fused_step(self, eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale=0.0, want_x0=False, generator=None, noise=None):
        """Same contract as ``DDPMScheduler.fused_step`` (device float32 tensors only).  ``noise``: this step's noise already drawn
        from ``generator`` by the caller; ignored at the last step, which adds none.  Returns (prev_sample, x0 | None)."""
        prev, x0, _ = self._device_step(eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale, want_x0, generator, noise)
        return prev, x0

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, noise=None):
        """diffusers' signature; ``noise`` (not in diffusers) is the pipelines' pre-drawn tensor: what ``generator`` would have given
        at this step, so it may come together with the generator, which it leaves untouched."""
        if self._on_device(model_output, sample):
            prev, _, den = self._device_step(model_output, timestep, sample, False, 1.0, 0.0, False, generator, noise, want_denoised=True)
            return (prev, den) if not return_dict else LCMSchedulerOutput(prev_sample=prev, denoised=den)
        return self._host_step(model_output, timestep, sample, generator, return_dict, noise)

    def _host_step(self, model_output, timestep, sample, generator=None, return_dict=True, noise=None):
        """The torch expressions of diffusers' ``LCMScheduler.step`` (host tensors; also the reference for the kernel test)."""
        dev = model_output.device
        last, coefs = self._plan(timestep)
        sa, s1, cs, co, sp, bp, _ = (c.to(dev) for c in coefs)
        p0 = (sample - s1 * model_output) / sa
        if self.config.clip_sample:
            p0 = p0.clamp(-self.config.clip_sample_range, self.config.clip_sample_range)
        denoised = co * p0 + cs * sample
        if last:
            prev = denoised
        else:
            if noise is None:
                noise = randn_tensor(model_output.shape, generator=generator, device=dev, dtype=denoised.dtype)
            prev = sp * denoised + bp * noise
        self._step_index += 1
        return (prev, denoised) if not return_dict else LCMSchedulerOutput(prev_sample=prev, denoised=denoised)


class _MultistepSolverBase(_StepIndexMixin, _SchedulerBase):
    """What ``DPMSolverMultistepScheduler`` and ``UniPCMultistepScheduler`` share (same config keys, same arithmetic): the state a
    constructor leaves, the timestep / sigma tables of ``set_timesteps``, the step-index rule and sigma -> (alpha_t, sigma_t)."""

    def _init_solver(self, cfg):
        self._register_betas(cfg)
        self.sigmas = ((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.linspace(0, cfg["num_train_timesteps"] - 1, cfg["num_train_timesteps"], dtype=np.float32)[::-1].copy())
        self.model_outputs = [None] * cfg["solver_order"]
        self.lower_order_nums = 0
        self._step_index = None

    @property
    def step_index(self):
        return self._step_index

    def set_timesteps(self, num_inference_steps=None, device=None):
        c = self.config
        last = c.num_train_timesteps
        if c.timestep_spacing == "linspace":
            ts = np.linspace(0, last - 1, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif c.timestep_spacing == "leading":
            ratio = last // (num_inference_steps + 1)
            ts = (np.arange(0, num_inference_steps + 1) * ratio).round()[::-1][:-1].copy().astype(np.int64)
            ts += c.steps_offset
        elif c.timestep_spacing == "trailing":
            ratio = c.num_train_timesteps / num_inference_steps
            ts = np.arange(last, 0, -ratio).round().copy().astype(np.int64) - 1
        else:
            raise ValueError(f"{c.timestep_spacing} is not supported")
        sig = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        sig = np.interp(ts, np.arange(0, len(sig)), sig)
        if c.final_sigmas_type == "sigma_min":
            sigma_last = ((1 - self.alphas_cumprod[0]) / self.alphas_cumprod[0]) ** 0.5
        elif c.final_sigmas_type == "zero":
            sigma_last = 0
        else:
            raise ValueError(f"`final_sigmas_type` must be one of 'zero', or 'sigma_min', but got {c.final_sigmas_type}")
        self.sigmas = torch.from_numpy(np.concatenate([sig, [sigma_last]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts).to(device=device, dtype=torch.int64)
        self._ts_host = [int(v) for v in ts]
        self.num_inference_steps = len(ts)
        self.model_outputs = [None] * c.solver_order
        self.lower_order_nums = 0
        self._step_index = None
        self._begin_index = None

    @staticmethod
    def _sigma_to_alpha_sigma_t(sigma):
        alpha_t = 1 / ((sigma ** 2 + 1) ** 0.5)
        return alpha_t, sigma * alpha_t

    def _index_for_timestep(self, timestep):
        t = int(timestep)
        idx = [k for k, v in enumerate(self._ts_host) if v == t]
        if not idx:
            return len(self._ts_host) - 1
        return idx[1] if len(idx) > 1 else idx[0]

    def _noise_sigmas(self, timesteps):
        """``sigmas[index]`` of ``add_noise``'s index rule, one float32 entry per timestep."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        return self.sigmas[self._noise_indices(timesteps)]

    def add_noise_coefs(self, timestep):
        """``(alpha_t, sigma_t)`` of ``sigmas[index]`` (diffusers' DPM-Solver / UniPC ``add_noise``), the index by ``_noise_indices``."""
        alpha_t, sigma_t = self._sigma_to_alpha_sigma_t(self._noise_sigmas([timestep])[0])
        return alpha_t.item(), sigma_t.item()

    def add_noise(self, original_samples, noise, timesteps):
        """diffusers' ``add_noise`` of the DPM-Solver / UniPC classes: ``alpha_t * x + sigma_t * noise`` from ``sigmas[index]``."""
        sigma = self._noise_sigmas(torch.as_tensor(timesteps).reshape(-1)).to(device=original_samples.device, dtype=original_samples.dtype)
        alpha_t, sigma_t = self._sigma_to_alpha_sigma_t(self._per_sample(sigma, original_samples))
        return alpha_t * original_samples + sigma_t * noise


class DPMSolverMultistepScheduler(_MultistepSolverBase):
    """DPM-Solver++ multistep scheduler: the one the reference swaps in for the dual-UNet text->HDR runs
    (``DPMSolverMultistepScheduler.from_config(pipeline.scheduler.config)``,
    scripts/inference/experiments/formal_improved.py:195; scripts/stage2/experiments/scheduler_tuning.py:190-201).
    Implements diffusers' ``dpmsolver++`` and ``sde-dpmsolver++`` ("DPM++ 2M SDE") algorithms with the ``midpoint`` and ``heun``
    solver types on the epsilon-prediction path, ``solver_order`` 1-2, ``lower_order_final``, ``euler_at_final`` and
    ``final_sigmas_type`` zero / sigma_min; Karras / exponential / beta sigma schedules, the non-``++`` algorithms, order 3 and
    thresholding raise NotImplementedError.  The reference's runs pass ``eta=0.7  # Controls stochasticity`` to the pipeline
    (formal_improved.py:267), which this solver has no argument for: ``algorithm_type="sde-dpmsolver++"`` is the stochastic
    sampling that comment intends.  The SDE algorithm draws noise once per step, the last included, after the x0 prediction.
    A host-side state machine over the scheduler protocol: ``step`` / ``fused_step`` run as ONE HIP kernel (gmd_dpm_step, or
    gmd_dpm_sde_step for the SDE algorithm) for float32 device tensors, as the same torch expressions on the host otherwise
    (SURVEY.md §8f-2)."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                     sample_max_value=1.0, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
                     euler_at_final=False, use_karras_sigmas=False, use_exponential_sigmas=False, use_beta_sigmas=False,
                     final_sigmas_type="zero", timestep_spacing="linspace", steps_offset=0, clip_sample=False)

    def __init__(self, **kwargs):
        cfg = self._merge_config(kwargs)
        if (cfg["algorithm_type"] not in ("dpmsolver++", "sde-dpmsolver++") or cfg["solver_type"] not in ("midpoint", "heun")
                or cfg["prediction_type"] != "epsilon" or cfg["thresholding"] or cfg["use_karras_sigmas"]
                or cfg["use_exponential_sigmas"] or cfg["use_beta_sigmas"] or cfg["solver_order"] not in (1, 2)):
            raise NotImplementedError("only dpmsolver++ / sde-dpmsolver++, midpoint / heun, epsilon, solver_order <= 2, plain sigmas"
                                      " are implemented")
        self._init_solver(cfg)
        self.alpha_t = torch.sqrt(self.alphas_cumprod)
        self.sigma_t = torch.sqrt(1 - self.alphas_cumprod)
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)

    def _plan_step(self, timestep):
        """Host side of one step: (order, float32 0-dim coefficient tensors) computed exactly as diffusers computes them."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self._step_index is None:
            self._init_step_index(timestep)
        c = self.config
        i, n = self._step_index, len(self._ts_host)
        lower_order_final = (i == n - 1) and (c.euler_at_final or (c.lower_order_final and n < 15) or c.final_sigmas_type == "zero")
        lower_order_second = (i == n - 2) and c.lower_order_final and n < 15
        alpha_s0, sigma_s0 = self._sigma_to_alpha_sigma_t(self.sigmas[i])
        alpha_t, sigma_t = self._sigma_to_alpha_sigma_t(self.sigmas[i + 1])
        lambda_t = torch.log(alpha_t) - torch.log(sigma_t)
        lambda_s0 = torch.log(alpha_s0) - torch.log(sigma_s0)
        h = lambda_t - lambda_s0
        first = c.solver_order == 1 or self.lower_order_nums < 1 or lower_order_final
        r0 = None
        if not first:
            assert c.solver_order == 2 or self.lower_order_nums < 2 or lower_order_second
            alpha_s1, sigma_s1 = self._sigma_to_alpha_sigma_t(self.sigmas[i - 1])
            lambda_s1 = torch.log(alpha_s1) - torch.log(sigma_s1)
            r0 = (lambda_s0 - lambda_s1) / h
        return first, alpha_s0, sigma_s0, alpha_t, sigma_t, h, r0

    def _advance(self, x0_pred):
        c = self.config
        for k in range(c.solver_order - 1):
            self.model_outputs[k] = self.model_outputs[k + 1]
        self.model_outputs[-1] = x0_pred
        if self.lower_order_nums < c.solver_order:
            self.lower_order_nums += 1
        self._step_index += 1

    def draws_noise(self, timestep, eta=0.0):
        """True when ``step`` at this timestep consumes the generator: iff the algorithm is an SDE one, then at EVERY step (the last
        included, where the noise coefficient may be 0)."""
        return self.config.algorithm_type == "sde-dpmsolver++"

    @property
    def predraws_noise(self):
        return self.draws_noise(None)

    def _update_coefs(self, first, alpha_t, sigma_t, sigma_s0, h):
        """(c_x, c_m, c_h, c_n) of ``x_prev = c_x x + c_m D0 + c_h D1 + c_n noise`` (SDE) or ``c_x x - c_m D0 - c_h D1`` (deterministic;
        c_n None) as float32 0-d tensors, each evaluated left to right as diffusers writes it.  c_h is None at first order.  The
        deterministic heun term is ``+ k D1``: its c_h is ``-k``, and ``a - (-k) d`` is the same float32 value as ``a + k d``."""
        c = self.config
        heun = c.solver_type == "heun"
        if c.algorithm_type == "sde-dpmsolver++":
            c_x = sigma_t / sigma_s0 * torch.exp(-h)
            c_m = alpha_t * (1 - torch.exp(-2.0 * h))
            c_n = sigma_t * torch.sqrt(1.0 - torch.exp(-2.0 * h))
            c_h = None if first else (alpha_t * ((1.0 - torch.exp(-2.0 * h)) / (-2.0 * h) + 1.0) if heun else 0.5 * c_m)
            return c_x, c_m, c_h, c_n
        c_x = sigma_t / sigma_s0
        c_m = alpha_t * (torch.exp(-h) - 1.0)
        c_h = None if first else (-(alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0)) if heun else 0.5 * c_m)
        return c_x, c_m, c_h, None

    def _device_step(self, eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale, want_x0, generator=None, noise=None):
        """One HIP kernel pass (gmd_dpm_step; gmd_dpm_sde_step for the SDE algorithm): CFG combine (+rescale), pipeline x0, x0
        prediction and the multistep update.  The SDE noise is drawn HERE with ``randn_tensor`` exactly where ``step`` draws it, so
        a generator shared by the two schedulers of the dual pipeline is consumed in the reference's order."""
        first, alpha_s0, sigma_s0, alpha_t, sigma_t, h, r0 = self._plan_step(timestep)
        c_x, c_m, c_h, c_n = self._update_coefs(first, alpha_t, sigma_t, sigma_s0, h)
        if c_h is None:
            c_h = torch.tensor(0.0)
        inv_r0 = (1.0 / r0) if r0 is not None else torch.tensor(0.0)
        a = self.alphas_cumprod[int(timestep)]  # the pipeline's own x0 (dual_unet.py:1072) uses the loop timestep
        if c_n is not None and noise is None:  # (the pipelines pre-draw a CPU generator's noise for all steps, in call order)
            noise = self._step_noise(sample, generator)
        ratio = self._guidance_ratio(eps_in, do_cfg, guidance_scale, guidance_rescale)
        m1 = None if first else self.model_outputs[-1]
        if c_n is None:
            m0, prev, x0 = ops.dpm_step(eps_in.contiguous(), sample.contiguous(), 1 if first else 2,
                                        (sigma_s0.item(), alpha_s0.item(), c_x.item(), c_m.item(), c_h.item(), inv_r0.item(),
                                         *self._x0_coefs(a)),
                                        do_cfg, guidance_scale, m1=m1, ratio=ratio, guidance_rescale=guidance_rescale, want_x0=want_x0)
        else:
            m0, prev, x0 = ops.dpm_sde_step(eps_in.contiguous(), sample.contiguous(), 1 if first else 2,
                                            (sigma_s0.item(), alpha_s0.item(), c_x.item(), c_m.item(), c_h.item(), inv_r0.item(),
                                             c_n.item(), *self._x0_coefs(a)),
                                            do_cfg, guidance_scale, noise.contiguous(), m1=m1, ratio=ratio,
                                            guidance_rescale=guidance_rescale, want_x0=want_x0)
        self._advance(m0)
        return prev, x0

    def fused_step(self, eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale=0.0, want_x0=False, generator=None, noise=None):
        """Same contract as ``DDPMScheduler.fused_step`` (device float32 tensors only).  ``generator`` and ``noise`` (this step's
        noise already drawn from ``generator`` by the caller) are used by the SDE algorithm only: the deterministic one never
        draws.  Returns (prev_sample, x0 | None)."""
        return self._device_step(eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale, want_x0, generator, noise)

    def step(self, model_output, timestep, sample, generator=None, variance_noise=None, return_dict=True, noise=None):
        """diffusers' signature; ``noise`` (not in diffusers) is the pipelines' pre-drawn tensor.  Either replaces the draw of the SDE
        algorithm, and the generator is then not touched; the deterministic algorithm ignores all three."""
        if variance_noise is None:
            variance_noise = noise
        if self._on_device(model_output, sample):
            prev, _ = self._device_step(model_output, timestep, sample, False, 1.0, 0.0, False, generator, variance_noise)
            return (prev,) if not return_dict else SchedulerOutput(prev_sample=prev)
        prev = self._host_step(model_output, timestep, sample, generator, variance_noise)
        return (prev,) if not return_dict else SchedulerOutput(prev_sample=prev)

    def _host_step(self, model_output, timestep, sample, generator=None, variance_noise=None):
        """The torch expressions of diffusers' ``DPMSolverMultistepScheduler.step`` (host tensors and 16-bit device tensors; also the
        reference for the kernel tests).  Returns prev_sample."""
        first, alpha_s0, sigma_s0, alpha_t, sigma_t, h, r0 = self._plan_step(timestep)
        x0_pred = (sample - sigma_s0 * model_output) / alpha_s0  # convert_model_output: dpmsolver++, epsilon
        m1 = self.model_outputs[-1]
        c = self.config
        sde, heun = c.algorithm_type == "sde-dpmsolver++", c.solver_type == "heun"
        if sde and variance_noise is None:
            variance_noise = randn_tensor(model_output.shape, generator=generator, device=model_output.device, dtype=torch.float32)
        sample = sample.to(torch.float32)
        D0 = x0_pred
        D1 = None if first else (1.0 / r0) * (x0_pred - m1)
        if sde:
            noise = variance_noise.to(torch.float32)
            if first:
                prev = ((sigma_t / sigma_s0 * torch.exp(-h)) * sample + (alpha_t * (1 - torch.exp(-2.0 * h))) * D0
                        + (sigma_t * torch.sqrt(1.0 - torch.exp(-2.0 * h))) * noise)
            elif heun:
                prev = ((sigma_t / sigma_s0 * torch.exp(-h)) * sample + (alpha_t * (1 - torch.exp(-2.0 * h))) * D0
                        + (alpha_t * ((1.0 - torch.exp(-2.0 * h)) / (-2.0 * h) + 1.0)) * D1
                        + (sigma_t * torch.sqrt(1.0 - torch.exp(-2.0 * h))) * noise)
            else:
                prev = ((sigma_t / sigma_s0 * torch.exp(-h)) * sample + (alpha_t * (1 - torch.exp(-2.0 * h))) * D0
                        + 0.5 * (alpha_t * (1 - torch.exp(-2.0 * h))) * D1
                        + (sigma_t * torch.sqrt(1.0 - torch.exp(-2.0 * h))) * noise)
        elif first:
            prev = (sigma_t / sigma_s0) * sample - (alpha_t * (torch.exp(-h) - 1.0)) * x0_pred
        elif heun:
            prev = ((sigma_t / sigma_s0) * sample - (alpha_t * (torch.exp(-h) - 1.0)) * D0
                    + (alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0)) * D1)
        else:
            prev = ((sigma_t / sigma_s0) * sample - (alpha_t * (torch.exp(-h) - 1.0)) * D0
                    - 0.5 * (alpha_t * (torch.exp(-h) - 1.0)) * D1)
        self._advance(x0_pred)
        return prev.to(model_output.dtype)


@dataclass
class EulerSchedulerOutput(_Output):
    prev_sample: torch.Tensor
    pred_original_sample: torch.Tensor = None


class _SigmaSchedulerBase(_StepIndexMixin, _SchedulerBase):
    """What the sigma-space (variance-exploding) schedulers share: the sigma / timestep tables of diffusers' ``set_timesteps``
    (float64 numpy, stored as float32 tensors), ``init_noise_sigma``, ``scale_model_input`` and the step index.  Unlike the
    variance-preserving schedulers above, the UNet input is ``sample / (sigma**2 + 1) ** 0.5`` and the timesteps are float32,
    fractional for ``linspace`` spacing and Karras sigmas: a step is selected by ``step_index``, never by an integer timestep."""

    sigma_space = True  # the pipelines' fused loops divide the UNet input by ``input_divisor`` inside the pack kernel
    _name = "_SigmaSchedulerBase"

    def _init_sigma_space(self, kwargs):
        cfg = self._merge_config(kwargs)
        if cfg["prediction_type"] != "epsilon":
            raise NotImplementedError(f"{self._name}: only prediction_type 'epsilon' is implemented (got {cfg['prediction_type']!r})")
        if cfg.get("interpolation_type", "linear") != "linear":
            raise NotImplementedError(f"{self._name}: only interpolation_type 'linear' is implemented")
        if cfg.get("timestep_type", "discrete") != "discrete":
            raise NotImplementedError(f"{self._name}: only timestep_type 'discrete' is implemented")
        if cfg.get("final_sigmas_type", "zero") != "zero":
            raise NotImplementedError(f"{self._name}: only final_sigmas_type 'zero' is implemented")
        if cfg.get("use_exponential_sigmas", False) or cfg.get("use_beta_sigmas", False):
            raise NotImplementedError(f"{self._name}: exponential and beta sigmas are not implemented (plain and Karras sigmas are)")
        if cfg.get("rescale_betas_zero_snr", False):
            raise NotImplementedError(f"{self._name}: rescale_betas_zero_snr is not implemented")
        self._register_betas(cfg)
        sigmas = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).flip(0)
        ts = np.linspace(0, cfg["num_train_timesteps"] - 1, cfg["num_train_timesteps"], dtype=float)[::-1].copy()
        self.timesteps = torch.from_numpy(ts).to(dtype=torch.float32)
        self.sigmas = torch.cat([sigmas, torch.zeros(1)])
        self._ts_host = self.timesteps.tolist()
        self.num_inference_steps = None
        self._step_index = None

    @property
    def step_index(self):
        return self._step_index

    @property
    def init_noise_sigma(self):
        max_sigma = self.sigmas.max()
        if self.config.timestep_spacing in ("linspace", "trailing"):
            return max_sigma
        return (max_sigma ** 2 + 1) ** 0.5

    def _train_sigmas(self):
        """((1 - a) / a) ** 0.5 of the float32 table, as float64."""
        return (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy().astype(np.float64)

    @staticmethod
    def _sigma_to_t(sigma, log_sigmas):
        """diffusers' ``_sigma_to_t``: the fractional train timestep whose log-sigma (linear between table entries) is log(sigma)."""
        log_sigma = np.log(np.maximum(sigma, 1e-10))
        dists = log_sigma - log_sigmas[:, np.newaxis]
        low_idx = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
        high_idx = low_idx + 1
        low, high = log_sigmas[low_idx], log_sigmas[high_idx]
        w = np.clip((low - log_sigma) / (low - high), 0, 1)
        return ((1 - w) * low_idx + w * high_idx).reshape(np.shape(sigma))

    def set_timesteps(self, num_inference_steps=None, device=None, timesteps=None, sigmas=None):
        """diffusers' tables.  ``sigmas``: a custom schedule INCLUDING its terminal value (the last entry, usually 0, gets no
        timestep); ``timesteps``: custom (possibly fractional) timesteps.  Everything is computed in float64 numpy and stored as
        float32 (diffusers takes the logarithms of the sigma table in float32; here they are float64 like the rest)."""
        c = self.config
        if timesteps is not None and sigmas is not None:
            raise ValueError("Only one of `timesteps` or `sigmas` should be set.")
        if num_inference_steps is None and timesteps is None and sigmas is None:
            raise ValueError("Must pass exactly one of `num_inference_steps` or `timesteps` or `sigmas.")
        if (timesteps is not None or sigmas is not None) and c.get("use_karras_sigmas", False):
            raise ValueError("Cannot set `timesteps` or `sigmas` with `config.use_karras_sigmas = True`.")
        train = self._train_sigmas()
        log_sigmas = np.log(train)
        T = c.num_train_timesteps
        if sigmas is not None:
            sigmas = np.array(sigmas).astype(np.float32)
            if sigmas.ndim != 1 or len(sigmas) < 2 or not np.all(sigmas[:-1] > 0) or not np.all(np.diff(sigmas) < 0):
                raise ValueError("custom `sigmas` must be positive and decreasing, followed by their terminal value")
            ts = self._sigma_to_t(sigmas[:-1].astype(np.float64), log_sigmas)
        else:
            if timesteps is not None:
                ts = np.array(timesteps).astype(np.float32)
            elif c.timestep_spacing == "linspace":
                ts = np.linspace(0, T - 1, num_inference_steps, dtype=np.float32)[::-1].copy()
            elif c.timestep_spacing == "leading":
                ratio = T // num_inference_steps
                ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.float32)
                ts += c.steps_offset
            elif c.timestep_spacing == "trailing":
                ratio = T / num_inference_steps
                ts = (np.arange(T, 0, -ratio)).round().copy().astype(np.float32)
                ts -= 1
            else:
                raise ValueError(f"{c.timestep_spacing} is not supported. Please make sure to choose one of 'linspace', 'leading' or 'trailing'.")
            sig = np.interp(ts, np.arange(0, len(train)), train)
            if c.get("use_karras_sigmas", False):
                sig = self._convert_to_karras(sig, len(ts))
                ts = self._sigma_to_t(sig, log_sigmas)
            sigmas = np.concatenate([sig, [0.0]]).astype(np.float32)
        ts32 = ts.astype(np.float32)
        if len(np.unique(ts32)) != len(ts32):
            # e.g. custom sigmas above the training range, which all map to the last train timestep: the step could no longer be
            # told from the timestep, and diffusers' rule for a repeated timestep (take the second) would skip the first sigma
            raise ValueError(f"{self._name}: the schedule holds a timestep twice ({ts32.tolist()}); every step needs its own timestep"
                             " (custom sigmas must lie inside the training range)")
        self.num_inference_steps = len(ts)
        self.sigmas = torch.from_numpy(sigmas).to(dtype=torch.float32)  # host: the step's scalars are computed from 0-d views of it
        self.timesteps = torch.from_numpy(ts32).to(device=device)
        self._ts_host = torch.from_numpy(ts32).tolist()
        self._step_index = None
        self._begin_index = None

    @staticmethod
    def _convert_to_karras(in_sigmas, num_inference_steps):
        """Karras et al. (2022) noise levels between the schedule's own ends, rho = 7."""
        sigma_min, sigma_max = float(in_sigmas[-1]), float(in_sigmas[0])
        rho = 7.0
        ramp = np.linspace(0, 1, num_inference_steps)
        min_inv_rho, max_inv_rho = sigma_min ** (1 / rho), sigma_max ** (1 / rho)
        return (max_inv_rho + ramp * (min_inv_rho - max_inv_rho)) ** rho

    def _index_for_timestep(self, timestep):
        """The entry equal to ``timestep`` as a float32 value (``set_timesteps`` refuses a schedule in which one occurs twice)."""
        t = float(timestep)
        idx = [k for k, v in enumerate(self._ts_host) if v == t]
        if not idx:
            raise ValueError(f"{self._name}: timestep {t!r} is not in the schedule set by `set_timesteps` (timesteps are float32"
                             " values and may be fractional: pass them on unchanged)")
        return idx[0]

    def add_noise_coefs(self, timestep):
        """``(1, sigmas[index])``: in sigma space ``add_noise`` is ``x + noise * sigma``, the index by ``_noise_indices``."""
        return 1.0, self.sigmas[self._noise_indices([timestep])[0]].item()

    def add_noise(self, original_samples, noise, timesteps):
        """diffusers' ``add_noise`` of the sigma-space classes: ``x + noise * sigmas[index]``."""
        sigma = self.sigmas[self._noise_indices(torch.as_tensor(timesteps).reshape(-1))]
        sigma = self._per_sample(sigma.to(device=original_samples.device, dtype=original_samples.dtype), original_samples)
        return original_samples + noise * sigma

    def _sigma(self, timestep):
        """The current step's sigma as a float32 0-d tensor (fixes the step index from ``timestep`` on first use)."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self._step_index is None:
            if timestep is None:
                raise ValueError(f"{self._name}: a timestep is needed until the first call has fixed the step index")
            self._init_step_index(timestep)
        return self.sigmas[self._step_index]

    def input_divisor(self, timestep=None):
        """(sigma**2 + 1) ** 0.5 of the current step as a float: what ``scale_model_input`` divides by, evaluated on a float32 0-d
        tensor exactly as there.  The fused loops hand it to the UNet's input pack."""
        sigma = self._sigma(timestep)
        return float((sigma ** 2 + 1) ** 0.5)

    def scale_model_input(self, sample, timestep=None):
        sigma = self._sigma(timestep)
        return sample / ((sigma ** 2 + 1) ** 0.5).to(sample.device)

    def _finish(self, prev, p0, return_dict):
        self._step_index += 1
        return (prev, p0) if not return_dict else EulerSchedulerOutput(prev_sample=prev, pred_original_sample=p0)


class EulerDiscreteScheduler(_SigmaSchedulerBase):
    """Euler (Karras et al. 2022, algorithm 2 without churn): the scheduler an SDXL-base checkpoint names, in sigma space.
    Implements diffusers' epsilon-prediction path with the three timestep spacings, plain or Karras sigmas and custom
    ``sigmas`` / ``timesteps``; v-prediction, ``s_churn`` > 0, log-linear interpolation, continuous timesteps, a non-zero final
    sigma and exponential / beta sigmas raise NotImplementedError.  It draws no noise.  ``step`` / ``fused_step`` run as ONE HIP
    kernel (gmd_euler_step) for float32 device tensors, as the same torch expressions (``_host_step``) otherwise; the host computes
    the step's scalars on float32 0-d tensors exactly as diffusers does."""

    _name = "EulerDiscreteScheduler"
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     prediction_type="epsilon", interpolation_type="linear", use_karras_sigmas=False, use_exponential_sigmas=False,
                     use_beta_sigmas=False, sigma_min=None, sigma_max=None, timestep_spacing="linspace", timestep_type="discrete",
                     steps_offset=0, rescale_betas_zero_snr=False, final_sigmas_type="zero")

    def __init__(self, **kwargs):
        self._init_sigma_space(kwargs)
        if self.config.sigma_min is not None or self.config.sigma_max is not None:
            raise NotImplementedError("EulerDiscreteScheduler: sigma_min / sigma_max overrides of the Karras range are not implemented")

    def _coefs(self, timestep, s_churn):
        if s_churn > 0:
            raise NotImplementedError("EulerDiscreteScheduler: s_churn > 0 (stochastic churn) is not implemented")
        sigma = self._sigma(timestep)
        sigma_hat = sigma * (0.0 + 1)  # gamma == 0
        return sigma_hat, self.sigmas[self._step_index + 1] - sigma_hat

    def _device_step(self, eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale, want_x0, s_churn=0.0):
        """One HIP kernel pass (gmd_euler_step): CFG combine (+rescale), x0 prediction and the Euler update.
        Returns (prev_sample, pred_original_sample | None)."""
        sigma_hat, dt = self._coefs(timestep, s_churn)
        ratio = self._guidance_ratio(eps_in, do_cfg, guidance_scale, guidance_rescale)
        out = ops.euler_step(eps_in.contiguous(), sample.contiguous(), (sigma_hat.item(), dt.item(), 0.0), do_cfg, guidance_scale,
                             ratio=ratio, guidance_rescale=guidance_rescale, want_pred_x0=want_x0)
        self._step_index += 1
        return out

    def fused_step(self, eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale=0.0, want_x0=False, generator=None, noise=None):
        """Same contract as ``DDIMScheduler.fused_step`` (device float32 tensors only); ``generator`` and ``noise`` are accepted and
        unused.  The x0 returned is ``sample - sigma * eps``: in sigma space the pipeline's x0 and pred_original_sample coincide.
        Returns (prev_sample, x0 | None)."""
        return self._device_step(eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale, want_x0)

    def step(self, model_output, timestep, sample, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0, generator=None,
             return_dict=True, noise=None):
        """diffusers' signature; ``noise`` (not in diffusers) is what the pipelines pass to every stochastic scheduler: unused here."""
        if self._on_device(model_output, sample):
            prev, p0 = self._device_step(model_output, timestep, sample, False, 1.0, 0.0, True, s_churn)
            return (prev, p0) if not return_dict else EulerSchedulerOutput(prev_sample=prev, pred_original_sample=p0)
        return self._host_step(model_output, timestep, sample, s_churn, return_dict)

    def _host_step(self, model_output, timestep, sample, s_churn=0.0, return_dict=True):
        """The torch expressions of diffusers' ``EulerDiscreteScheduler.step`` (host tensors; also the reference for the kernel test)."""
        sigma_hat, dt = (c.to(model_output.device) for c in self._coefs(timestep, s_churn))
        sample = sample.to(torch.float32)
        p0 = sample - sigma_hat * model_output
        derivative = (sample - p0) / sigma_hat
        prev = sample + derivative * dt
        return self._finish(prev.to(model_output.dtype), p0, return_dict)


class EulerAncestralDiscreteScheduler(_SigmaSchedulerBase):
    """Euler ancestral sampling (k-diffusion's ``sample_euler_ancestral`` as diffusers restates it): an Euler step down to
    ``sigma_down`` followed by fresh noise of standard deviation ``sigma_up``.  Noise is drawn from the caller's generator at EVERY
    step, the last included (where sigma_up is 0): n steps take n draws.  Same spacings and limits as ``EulerDiscreteScheduler``;
    ``use_karras_sigmas`` is accepted here too (diffusers' class has plain sigmas only).  ``step`` / ``fused_step`` run as ONE HIP
    kernel (gmd_euler_step with a noise tensor) for float32 device tensors, as the torch expressions (``_host_step``) otherwise."""

    _name = "EulerAncestralDiscreteScheduler"
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     prediction_type="epsilon", use_karras_sigmas=False, timestep_spacing="linspace", steps_offset=0,
                     rescale_betas_zero_snr=False)

    def __init__(self, **kwargs):
        self._init_sigma_space(kwargs)

    predraws_noise = True

    def draws_noise(self, timestep, eta=0.0):
        """True: ``step`` consumes the generator at every step, the last included."""
        return True

    def _coefs(self, timestep):
        """(sigma, dt = sigma_down - sigma, sigma_up) as float32 0-d tensors, evaluated exactly as diffusers evaluates them."""
        sigma = self._sigma(timestep)
        sigma_from, sigma_to = self.sigmas[self._step_index], self.sigmas[self._step_index + 1]
        sigma_up = (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5
        sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
        return sigma, sigma_down - sigma, sigma_up

    def _device_step(self, eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale, want_x0, generator=None, noise=None):
        """One HIP kernel pass (gmd_euler_step): CFG combine (+rescale), x0 prediction, the Euler update to sigma_down and the
        ancestral noise.  The noise is drawn HERE with ``randn_tensor`` exactly where ``step`` draws it, so a generator shared by the
        two schedulers of the dual pipeline is consumed in call order (SDR first, GM second)."""
        sigma, dt, sigma_up = self._coefs(timestep)
        if noise is None:  # (the pipelines pre-draw a CPU generator's noise for all steps, in call order)
            noise = self._step_noise(sample, generator)
        ratio = self._guidance_ratio(eps_in, do_cfg, guidance_scale, guidance_rescale)
        out = ops.euler_step(eps_in.contiguous(), sample.contiguous(), (sigma.item(), dt.item(), sigma_up.item()), do_cfg, guidance_scale,
                             noise=noise.contiguous(), ratio=ratio, guidance_rescale=guidance_rescale, want_pred_x0=want_x0)
        self._step_index += 1
        return out

    def fused_step(self, eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale=0.0, want_x0=False, generator=None, noise=None):
        """Same contract as ``DDPMScheduler.fused_step`` (device float32 tensors only).  ``noise``: this step's noise already drawn
        from ``generator`` by the caller.  Returns (prev_sample, x0 | None) with x0 = ``sample - sigma * eps``."""
        return self._device_step(eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale, want_x0, generator, noise)

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, noise=None):
        """diffusers' signature; ``noise`` (not in diffusers) is the pipelines' pre-drawn tensor: what ``generator`` would have
        given at this step, so it may come together with the generator, which is then not touched."""
        if self._on_device(model_output, sample):
            prev, p0 = self._device_step(model_output, timestep, sample, False, 1.0, 0.0, True, generator, noise)
            return (prev, p0) if not return_dict else EulerSchedulerOutput(prev_sample=prev, pred_original_sample=p0)
        return self._host_step(model_output, timestep, sample, generator, return_dict, noise)

    def _host_step(self, model_output, timestep, sample, generator=None, return_dict=True, noise=None):
        """The torch expressions of diffusers' ``EulerAncestralDiscreteScheduler.step`` (host tensors; the kernel test's reference)."""
        dev = model_output.device
        sigma, dt, sigma_up = (c.to(dev) for c in self._coefs(timestep))
        sample = sample.to(torch.float32)
        p0 = sample - sigma * model_output
        derivative = (sample - p0) / sigma
        prev = sample + derivative * dt
        if noise is None:
            noise = randn_tensor(model_output.shape, generator=generator, device=dev, dtype=model_output.dtype)
        prev = prev + noise * sigma_up
        return self._finish(prev.to(model_output.dtype), p0, return_dict)


# 4-point Gauss-Legendre rule on [-1, 1]: +-_GL_X[k] with weight _GL_W[k].  Exact for polynomials of degree <= 7; the LMS basis
# polynomials have degree <= 3.  The two weights sum to exactly 1.0 in float64, so a constant integrand (order 1) gives b - a exactly.
_GL_X = (0.8611363115940526, 0.3399810435848563)
_GL_W = (0.34785484513745385, 0.6521451548625461)


class LMSDiscreteScheduler(_SigmaSchedulerBase):
    """Linear multistep (Adams-Bashforth in sigma, k-diffusion's ``sample_lms`` as diffusers restates it), orders 1-4: the update is
    ``sample + sum_j c_j d_j`` over the derivatives ``d = (sample - pred_original_sample) / sigma`` of this step and of up to three
    earlier ones, with ``c_j`` the integral over [sigma, sigma_next] of the j-th Lagrange basis polynomial on the last ``order``
    sigmas.  One UNet evaluation per step, no noise.  Tables, spacings, Karras / custom sigmas, ``init_noise_sigma``,
    ``scale_model_input`` and the limits (epsilon prediction only, no exponential / beta sigmas) are ``_SigmaSchedulerBase``'s.
    ``step`` / ``fused_step`` run as ONE HIP kernel (gmd_lms_step) for float32 device tensors, as diffusers' torch expressions
    (``_host_step``) otherwise.

    Unlike diffusers (``scipy.integrate.quad(..., epsrel=1e-4)`` on an integrand evaluated through float32 0-d tensors), the
    coefficients take the float32 sigmas as float64 and integrate the product form of the basis with a 4-point Gauss-Legendre
    rule, which is exact for these polynomials up to float64 rounding; each is rounded to float32 once, where it meets the
    derivative."""

    _name = "LMSDiscreteScheduler"
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     use_karras_sigmas=False, use_exponential_sigmas=False, use_beta_sigmas=False, prediction_type="epsilon",
                     timestep_spacing="linspace", steps_offset=0)
    MAX_ORDER = 4  # gmd_lms_step reads at most three earlier derivatives

    def __init__(self, **kwargs):
        self._init_sigma_space(kwargs)
        self.derivatives = []

    def set_timesteps(self, num_inference_steps=None, device=None, timesteps=None, sigmas=None):
        super().set_timesteps(num_inference_steps, device=device, timesteps=timesteps, sigmas=sigmas)
        self._sig64 = self.sigmas.numpy().astype(np.float64).tolist()
        self.derivatives = []

    def get_lms_coefficient(self, order, t, current_order):
        """The integral over [sigma_t, sigma_{t+1}] of the Lagrange basis polynomial that is 1 at sigma_{t - current_order} and 0 at
        the other nodes sigma_{t-k}, k < order, as a Python float (float64).  The integrand stays in product form: expanded into
        monomial coefficients it would lose four digits to cancellation."""
        if not 0 <= current_order < order <= t + 1:
            raise ValueError(f"{self._name}: no coefficient {current_order} of order {order} at step {t}")
        s = self._sig64 if self.num_inference_steps is not None else self.sigmas.numpy().astype(np.float64).tolist()
        a, b = s[t], s[t + 1]
        mid, half = 0.5 * (a + b), 0.5 * (b - a)
        node = s[t - current_order]
        others = [s[t - k] for k in range(order) if k != current_order]

        def basis(tau):
            prod = 1.0
            for o in others:
                prod *= (tau - o) / (node - o)
            return prod

        total = 0.0
        for gx, gw in zip(_GL_X, _GL_W):
            total += gw * (basis(mid - half * gx) + basis(mid + half * gx))
        return half * total

    def _plan(self, timestep, order):
        """(sigma as a float32 0-d tensor, effective order k, [c_0 .. c_{k-1}] as Python floats) of the next step.  k is
        ``min(step_index + 1, order)``, and never more than the history allows (one more than the derivatives kept, which differs
        from ``step_index`` only when the caller raises ``order`` in mid-trajectory)."""
        order = int(order)
        if not 1 <= order <= self.MAX_ORDER:
            raise ValueError(f"{self._name}: order must be in 1..{self.MAX_ORDER} (got {order})")
        sigma = self._sigma(timestep)
        i = self._step_index
        k = min(i + 1, order, len(self.derivatives) + 1)
        return sigma, k, [self.get_lms_coefficient(k, i, j) for j in range(k)]

    def _keep(self, derivative, order):
        self.derivatives.append(derivative)
        del self.derivatives[:-int(order)]

    def _device_step(self, eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale, want_x0, order=4):
        """One HIP kernel pass (gmd_lms_step): CFG combine (+rescale), x0 prediction, the derivative and the multistep update.  The
        derivative kept as history is the kernel's own output, never ``eps_in`` (which may be the static output buffer of a captured
        graph that the next replay overwrites).  Returns (prev_sample, pred_original_sample | None)."""
        sigma, k, coeffs = self._plan(timestep, order)
        ratio = self._guidance_ratio(eps_in, do_cfg, guidance_scale, guidance_rescale)
        hist = list(reversed(self.derivatives))[:k - 1]
        d, prev, p0 = ops.lms_step(eps_in.contiguous(), sample.contiguous(), k, [sigma.item()] + coeffs + [0.0] * (4 - k), do_cfg,
                                   guidance_scale, hist=hist, ratio=ratio, guidance_rescale=guidance_rescale, want_pred_x0=want_x0)
        self._keep(d, order)
        self._step_index += 1
        return prev, p0

    def fused_step(self, eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale=0.0, want_x0=False, generator=None, noise=None,
                   order=4):
        """Same contract as ``EulerDiscreteScheduler.fused_step`` (device float32 tensors only); ``generator`` and ``noise`` are
        accepted and unused.  Returns (prev_sample, x0 | None) with x0 = ``sample - sigma * eps``."""
        return self._device_step(eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale, want_x0, order)

    def step(self, model_output, timestep, sample, order=4, return_dict=True, **ignored):
        """diffusers' signature.  ``generator`` and ``noise``, which the pipelines hand to the stochastic schedulers, are accepted
        as keywords and ignored; they are not named parameters, so ``prepare_extra_step_kwargs`` (which reads this signature)
        passes neither, as for diffusers' class."""
        bad = [k for k in ignored if k not in ("generator", "noise")]
        if bad:
            raise TypeError(f"{self._name}.step: unexpected arguments {bad}")
        if self._on_device(model_output, sample):
            prev, p0 = self._device_step(model_output, timestep, sample, False, 1.0, 0.0, True, order)
            return (prev, p0) if not return_dict else EulerSchedulerOutput(prev_sample=prev, pred_original_sample=p0)
        return self._host_step(model_output, timestep, sample, order, return_dict)

    def _host_step(self, model_output, timestep, sample, order=4, return_dict=True):
        """The torch expressions of diffusers' ``LMSDiscreteScheduler.step`` (host tensors; also the reference for the kernel test).
        ``sum`` starts from the int 0, so the first addition is ``0 + c_0 * d``."""
        sigma, k, lms_coeffs = self._plan(timestep, order)
        sigma = sigma.to(model_output.device)
        p0 = sample - sigma * model_output
        derivative = (sample - p0) / sigma
        self._keep(derivative, order)
        prev = sample + sum(coeff * derivative for coeff, derivative in zip(lms_coeffs, reversed(self.derivatives)))
        return self._finish(prev, p0, return_dict)


class _UniPCPlan:
    """The scalars of one UniPC step, each a float32 0-d CPU tensor: corrector order ``p`` (0 = off) with ``c_x, c_m, c_b``, ``c_rho``
    (p entries) and ``c_r`` (p - 1 entries), predictor order ``q`` with ``p_x, p_m, p_b``, ``p_rho`` and ``p_r`` (q - 1 entries each)."""

    __slots__ = ("p", "q", "sigma_s", "alpha_s", "c_x", "c_m", "c_b", "c_rho", "c_r", "p_x", "p_m", "p_b", "p_rho", "p_r")

    def floats(self):
        """The 17 scheduler scalars of gmd_unipc_step in its order; a slot beyond the orders in use is 0.0 (the kernel never reads it)."""
        pad = lambda v, k: [t.item() for t in v] + [0.0] * (k - len(v))
        corr = ([self.c_x.item(), self.c_m.item(), self.c_b.item()] + pad(self.c_rho, 3) + pad(self.c_r, 2)) if self.p else [0.0] * 8
        pred = [self.p_x.item(), self.p_m.item(), self.p_b.item() if self.q > 1 else 0.0] + pad(self.p_rho, 2) + pad(self.p_r, 2)
        return [self.sigma_s.item(), self.alpha_s.item()] + corr + pred


class UniPCMultistepScheduler(_MultistepSolverBase):
    """UniPC (Zhao et al. 2023, diffusers' ``UniPCMultistepScheduler``): a multistep predictor of order 1-3 whose previous update is
    repaired by a corrector that re-uses the model output of the CURRENT step, so the correction costs no UNet evaluation.  The sampler
    for 8-20 steps with an ordinary checkpoint.  Implemented: ``predict_x0`` with epsilon prediction, ``solver_type`` bh1 / bh2,
    ``solver_order`` 1-3, ``lower_order_final``, ``disable_corrector``, ``final_sigmas_type`` zero / sigma_min, the three spacings;
    Karras / exponential / beta / flow sigmas, ``predict_x0=False``, ``solver_p``, thresholding, zero-SNR betas and other prediction
    types raise NotImplementedError.  Variance-preserving: ``init_noise_sigma`` is 1 and ``scale_model_input`` the identity; tables and
    the step-index rule are those of ``DPMSolverMultistepScheduler`` (``_MultistepSolverBase``).  A host-side state machine: ``step`` / ``fused_step`` run as ONE HIP
    kernel (gmd_unipc_step: x0, corrector and predictor) for float32 device tensors, as the torch expressions of ``_host_step``
    otherwise.

    Two deliberate differences from diffusers.  The weighted sum over the history differences is written as float32 products and adds
    from left to right (the corrector's ``x0 - m0`` term last) where diffusers calls ``einsum``: equal up to rounding, and reproducible
    bit for bit by the kernel.  At order 1 the ``B_h`` term is omitted, not multiplied by a zero: at the last step of a schedule that
    ends at sigma 0, h is +inf and diffusers' bh1 multiplies -inf by the integer 0 there."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                     sample_max_value=1.0, predict_x0=True, solver_type="bh2", lower_order_final=True, disable_corrector=[],
                     solver_p=None, use_karras_sigmas=False, use_exponential_sigmas=False, use_beta_sigmas=False, use_flow_sigmas=False,
                     flow_shift=1.0, timestep_spacing="linspace", steps_offset=0, final_sigmas_type="zero", rescale_betas_zero_snr=False,
                     clip_sample=False)
    MAX_ORDER = 3  # gmd_unipc_step reads at most three earlier x0 predictions

    def __init__(self, **kwargs):
        cfg = self._merge_config(kwargs)
        cfg["disable_corrector"] = list(cfg["disable_corrector"] or [])
        if cfg["solver_type"] in ("midpoint", "heun", "logrho"):  # another solver's config (from_config): diffusers falls to bh2 too
            cfg["solver_type"] = "bh2"
        for key in ("use_karras_sigmas", "use_exponential_sigmas", "use_beta_sigmas", "use_flow_sigmas", "thresholding",
                    "rescale_betas_zero_snr"):
            if cfg[key]:
                raise NotImplementedError(f"UniPCMultistepScheduler: {key}=True is not implemented")
        if not cfg["predict_x0"]:
            raise NotImplementedError("UniPCMultistepScheduler: predict_x0=False is not implemented")
        if cfg["solver_p"] is not None:
            raise NotImplementedError("UniPCMultistepScheduler: solver_p is not implemented")
        if cfg["prediction_type"] != "epsilon":
            raise NotImplementedError(f"UniPCMultistepScheduler: prediction_type={cfg['prediction_type']!r} is not implemented (epsilon only)")
        if cfg["solver_type"] not in ("bh1", "bh2"):
            raise NotImplementedError(f"UniPCMultistepScheduler: solver_type={cfg['solver_type']!r} is not implemented (bh1, bh2)")
        if cfg["solver_order"] not in (1, 2, 3):
            raise NotImplementedError(f"UniPCMultistepScheduler: solver_order={cfg['solver_order']!r} is not implemented (1..{self.MAX_ORDER})")
        self._init_solver(cfg)
        self.last_sample = None
        self.this_order = None

    def set_timesteps(self, num_inference_steps=None, device=None):
        super().set_timesteps(num_inference_steps, device)
        self.last_sample = None
        self.this_order = None

    def _lambda(self, k):
        """(alpha, sigma, lambda) of sigma-table entry k as float32 0-d tensors."""
        alpha, sigma = self._sigma_to_alpha_sigma_t(self.sigmas[k])
        return alpha, sigma, torch.log(alpha) - torch.log(sigma)

    def _rb(self, h, rks):
        """(R, b, phi_1, B_h) of the UniPC paper's linear system for step size ``h`` and the nodes ``rks`` (the last one is 1)."""
        hh = -h
        phi_1 = torch.expm1(hh)
        B_h = hh if self.config.solver_type == "bh1" else torch.expm1(hh)
        rks = torch.stack(rks)
        h_phi_k = phi_1 / hh - 1
        f = 1
        R, b = [], []
        for j in range(1, len(rks) + 1):
            R.append(torch.pow(rks, j - 1))
            b.append(h_phi_k * f / B_h)
            f *= j + 1
            h_phi_k = h_phi_k / hh - 1 / f
        return torch.stack(R), torch.stack(b), phi_1, B_h

    def _plan_step(self, timestep):
        """Host side of one step: a ``_UniPCPlan``.  Reads the state, changes nothing but the step index's initialisation."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self._step_index is None:
            self._init_step_index(timestep)
        c = self.config
        i, n = self._step_index, len(self._ts_host)
        pl = _UniPCPlan()
        alpha_s, sigma_s, lambda_s = self._lambda(i)
        pl.sigma_s, pl.alpha_s = sigma_s, alpha_s
        one = torch.tensor(1.0)
        # corrector: repairs the update from sigma_{i-1} to sigma_i with the order that update was predicted with
        pl.p = self.this_order if (i > 0 and (i - 1) not in c.disable_corrector and self.last_sample is not None) else 0
        if pl.p:
            _, sigma_p, lambda_p = self._lambda(i - 1)
            h = lambda_s - lambda_p
            pl.c_r = [(self._lambda(i - 1 - k)[2] - lambda_p) / h for k in range(1, pl.p)]
            R, b, phi_1, B_h = self._rb(h, pl.c_r + [one])
            pl.c_rho = [torch.tensor(0.5)] if pl.p == 1 else list(torch.linalg.solve(R, b))
            pl.c_x, pl.c_m, pl.c_b = sigma_s / sigma_p, alpha_s * phi_1, alpha_s * B_h
        # predictor
        q = min(c.solver_order, n - i) if c.lower_order_final else c.solver_order
        pl.q = q = min(q, self.lower_order_nums + 1)
        alpha_t, sigma_t, lambda_t = self._lambda(i + 1)
        h = lambda_t - lambda_s
        if q > 1 and not torch.isfinite(h):
            raise ValueError(f"UniPCMultistepScheduler: the last step ends at sigma 0 (h is not finite) and would run at order {q}, whose"
                             " coefficients are not finite; use lower_order_final=True or final_sigmas_type=\"sigma_min\"")
        pl.p_r = [(self._lambda(i - k)[2] - lambda_s) / h for k in range(1, q)]
        R, b, phi_1, B_h = self._rb(h, pl.p_r + [one])
        pl.p_rho = [] if q == 1 else [torch.tensor(0.5)] if q == 2 else list(torch.linalg.solve(R[:-1, :-1], b[:-1]))
        pl.p_x, pl.p_m, pl.p_b = sigma_t / sigma_s, alpha_t * phi_1, alpha_t * B_h
        return pl

    def _advance(self, x0_pred, corrected, pl):
        c = self.config
        for k in range(c.solver_order - 1):
            self.model_outputs[k] = self.model_outputs[k + 1]
        self.model_outputs[-1] = x0_pred
        self.this_order = pl.q
        self.last_sample = corrected
        if self.lower_order_nums < c.solver_order:
            self.lower_order_nums += 1
        self._step_index += 1

    def _device_step(self, eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale, want_x0):
        """One HIP kernel pass (gmd_unipc_step): CFG combine (+rescale), pipeline x0, x0 prediction, corrector and predictor.  What is
        kept as history (the x0 prediction and the corrected sample) are the kernel's own outputs, never ``eps_in`` (which may be the
        static output buffer of a captured graph) nor the caller's ``sample``.  Returns (prev_sample, x0 | None)."""
        pl = self._plan_step(timestep)
        a = self.alphas_cumprod[int(timestep)]  # the pipeline's own x0 (dual_unet.py:1072) uses the loop timestep
        ratio = self._guidance_ratio(eps_in, do_cfg, guidance_scale, guidance_rescale)
        hist = list(reversed(self.model_outputs))[:max(pl.p, pl.q - 1)]
        m0, corrected, prev, x0 = ops.unipc_step(eps_in.contiguous(), sample.contiguous(), pl.p, pl.q,
                                                 pl.floats() + [*self._x0_coefs(a)], do_cfg, guidance_scale,
                                                 last_sample=self.last_sample if pl.p else None, hist=hist, ratio=ratio,
                                                 guidance_rescale=guidance_rescale, want_x0=want_x0)
        self._advance(m0, corrected, pl)
        return prev, x0

    def fused_step(self, eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale=0.0, want_x0=False, generator=None, noise=None):
        """Same contract as ``DPMSolverMultistepScheduler.fused_step`` (device float32 tensors only); ``generator`` and ``noise`` are
        accepted and unused.  Returns (prev_sample, x0 | None)."""
        return self._device_step(eps_in, timestep, sample, do_cfg, guidance_scale, guidance_rescale, want_x0)

    def step(self, model_output, timestep, sample, return_dict=True):
        if self._on_device(model_output, sample):
            prev, _ = self._device_step(model_output, timestep, sample, False, 1.0, 0.0, False)
        else:
            prev = self._host_step(model_output, timestep, sample)
        return (prev,) if not return_dict else SchedulerOutput(prev_sample=prev)

    def _host_step(self, model_output, timestep, sample):
        """The step as torch expressions (host tensors and 16-bit device tensors; also the reference for the kernel tests): float32
        throughout, every scalar a float32 0-d tensor, sums from left to right.  Returns prev_sample."""
        pl = self._plan_step(timestep)
        eps, x = model_output.to(torch.float32), sample.to(torch.float32)
        x0_pred = (x - pl.sigma_s * eps) / pl.alpha_s  # from the sample as it comes in
        if pl.p:
            m0 = self.model_outputs[-1]
            acc = None
            for k in range(1, pl.p):
                term = pl.c_rho[k - 1] * ((self.model_outputs[-(k + 1)] - m0) / pl.c_r[k - 1])
                acc = term if acc is None else acc + term
            term = pl.c_rho[pl.p - 1] * (x0_pred - m0)
            acc = term if acc is None else acc + term
            x = pl.c_x * self.last_sample - pl.c_m * m0 - pl.c_b * acc
        elif x is sample:
            x = x.clone()  # kept as last_sample: never the caller's own tensor
        self._advance(x0_pred, x, pl)
        prev = pl.p_x * x - pl.p_m * x0_pred
        if pl.q > 1:
            acc = None
            for k in range(1, pl.q):
                term = pl.p_rho[k - 1] * ((self.model_outputs[-(k + 1)] - x0_pred) / pl.p_r[k - 1])
                acc = term if acc is None else acc + term
            prev = prev - pl.p_b * acc
        return prev.to(model_output.dtype)
