"""Reference for the DDIM step (csrc/latent_step.hip ddim_step_kernel, components.DDIMScheduler): plain helper module in the style of
tests/small_ref.py.  Nothing here uses the product class or the library.

  * ``ddim_step64``: the step of diffusers' ``DDIMScheduler.step`` (epsilon prediction) restated in float64 as a plain function of
    (eps, x, noise, a_t, a_prev, eta, clip, use_clipped), with the magnitude expression A that the per-element bound is built on;
  * ``ddim_step_f32``: the same expressions in float32 with every scalar held as a float32 0-dim tensor, in the kernel's order -- what
    the kernel must reproduce bit for bit given its float coefficients;
  * ``RefDDIMScheduler``: a small CPU scheduler object around ``ddim_step64`` with ``eta`` / ``use_clipped_model_output`` fixed at
    construction and the ``step(model_output, t, sample, generator=None, return_dict=True)`` signature the loops of oracle/pipelines.py
    drive (they pass only ``generator``).

The bound.  Per element the float32 step is
    p0 = (x - s1 eps) / sa;  [clamp];  pe = use_clipped ? (x - sa p0) / s1 : eps;  r = sp p0 + dc pe [+ sd noise]
with sa = a_t^.5, s1 = (1 - a_t)^.5, sp = a_prev^.5, sd = eta var^.5, dc = (1 - a_prev - sd^2)^.5, all float32.  A is that expression with
every operand replaced by its magnitude and every subtraction by an addition (the clamp only ever shrinks |p0|, so it is left out of A;
the subtractions under dc's root become additions too, which keeps the absolute rounding error of that cancelling difference covered):
    A_p0 = (|x| + s1 |eps|) / sa;  A_pe = use_clipped ? (|x| + sa A_p0) / s1 : |eps|;  A = sp A_p0 + (1 + a_prev + sd^2)^.5 A_pe + sd |noise|.
A float32 evaluation differs from the exact value by at most (number of roundings on the longest path) 2^-24 A to first order; the
longest path, the use_clipped one, has: s1 (2: the difference and the root), the product, the difference, the quotient by sa (1 + 1), the
product sa p0, the difference, the quotient by s1, the product with dc (dc itself: 2 differences, the square, the root), the sum: 16.
"""
from types import SimpleNamespace

import numpy as np
import torch

U_F32 = 2.0 ** -24
ROUNDINGS = 16
F32, F64 = torch.float32, torch.float64


def coefs64(a_t, a_prev, eta):
    """(sa, s1, sp, dc, sd) in float64 from the two cumulative alphas (Python floats: the float32 table entries, exactly)."""
    a_t, a_prev, eta = float(a_t), float(a_prev), float(eta)
    variance = (1.0 - a_prev) / (1.0 - a_t) * (1.0 - a_t / a_prev)
    sd = eta * variance ** 0.5
    return a_t ** 0.5, (1.0 - a_t) ** 0.5, a_prev ** 0.5, max(1.0 - a_prev - sd * sd, 0.0) ** 0.5, sd


def ddim_step64(eps, x, noise, a_t, a_prev, eta, clip=None, use_clipped=False):
    """(x_prev, p0, A) in float64.  ``noise`` is added iff eta > 0 (it may be None otherwise); ``clip``: None or the clip range."""
    sa, s1, sp, dc, sd = coefs64(a_t, a_prev, eta)
    e, s = eps.to(F64), x.to(F64)
    p0 = (s - s1 * e) / sa
    a_p0 = (s.abs() + s1 * e.abs()) / sa
    if clip is not None:
        p0 = p0.clamp(-float(clip), float(clip))
    if use_clipped:
        pe = (s - sa * p0) / s1
        a_pe = (s.abs() + sa * a_p0) / s1
    else:
        pe, a_pe = e, e.abs()
    r = sp * p0 + dc * pe
    a = sp * a_p0 + (1.0 + float(a_prev) + sd * sd) ** 0.5 * a_pe
    if eta > 0:
        r = r + sd * noise.to(F64)
        a = a + sd * noise.to(F64).abs()
    return r, p0, a


def bound(a):
    return ROUNDINGS * U_F32 * a


def _s(v):
    return torch.tensor(float(v), dtype=F32)  # a scalar the kernel receives as ``float``


def ddim_step_f32(eps, x, coefs, noise=None, clip_range=None, use_clipped=False):
    """(x_prev, x0, pred_x0) of gmd_ddim_step given the guided eps, as float32 torch expressions in the kernel's order;
    coefs = (sched_sqrt_a, sched_sqrt_1ma, sqrt_a_prev, dir_coeff, std, sqrt_a, sqrt_1ma).  The noise is added whenever it is given."""
    ssa, ss1, sp, dc, sd, sa, s1 = (_s(c) for c in coefs)
    x0 = (x - s1 * eps) / sa
    p0 = (x - ss1 * eps) / ssa
    if clip_range is not None:
        p0 = p0.clamp(-float(clip_range), float(clip_range))
    pe = (x - ssa * p0) / ss1 if use_clipped else eps
    r = sp * p0 + dc * pe
    if noise is not None:
        r = r + sd * noise
    return r, x0, p0


class RefDDIMScheduler:
    """The scheduler protocol of oracle/pipelines.py around ``ddim_step64`` (leading spacing, as the oracle's own schedulers)."""

    order = 1

    def __init__(self, eta=0.0, use_clipped_model_output=False, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                 beta_schedule="scaled_linear", clip_sample=False, clip_sample_range=1.0, set_alpha_to_one=True, steps_offset=1):
        self.eta, self.use_clipped = float(eta), bool(use_clipped_model_output)
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, steps_offset=steps_offset, clip_sample=clip_sample,
                                      clip_sample_range=clip_sample_range, set_alpha_to_one=set_alpha_to_one)
        if beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=F32)
        else:
            assert beta_schedule == "scaled_linear"
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=F32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.init_noise_sigma = 1.0
        self.timesteps = None

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        ratio = self.config.num_train_timesteps // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + self.config.steps_offset
        self.timesteps = torch.from_numpy(ts)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def alphas(self, timestep):
        t = int(timestep)
        p = t - self.config.num_train_timesteps // self.num_inference_steps
        a_prev = float(self.alphas_cumprod[p]) if p >= 0 else (1.0 if self.config.set_alpha_to_one else float(self.alphas_cumprod[0]))
        return float(self.alphas_cumprod[t]), a_prev

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        a_t, a_prev = self.alphas(timestep)
        noise = None
        if self.eta > 0:  # drawn at EVERY step, the last included
            noise = torch.randn(model_output.shape, generator=generator, dtype=model_output.dtype,
                                device=generator.device if generator is not None else model_output.device).to(model_output.device)
        prev, p0, _ = ddim_step64(model_output, sample, noise, a_t, a_prev, self.eta,
                                  self.config.clip_sample_range if self.config.clip_sample else None, self.use_clipped)
        prev, p0 = prev.to(model_output.dtype), p0.to(model_output.dtype)
        return (prev, p0) if not return_dict else SimpleNamespace(prev_sample=prev, pred_original_sample=p0)
