"""Reference for the sigma-space schedulers (components.EulerDiscreteScheduler / EulerAncestralDiscreteScheduler, csrc/latent_step.hip
euler_step_kernel and the scaled pack_kernel): plain helper module in the style of tests/ddim_ref.py.  Nothing here uses the product classes
or the library.  The arithmetic restates diffusers ~0.33 from memory (SURVEY.md convention [3P-memory]); this file is the pin.

  * ``schedule64``: the sigma / timestep tables in float64 (three spacings, plain or Karras rho = 7, custom sigmas).  As in diffusers
    the ``linspace`` timesteps are rounded to float32 BEFORE the sigma table is interpolated at them.  The fractional timestep of a
    Karras / custom sigma is the inverse of the piecewise-linear log-sigma table, written here with ``np.interp``;
  * ``step64``: one step in float64 as a plain function of (eps, x, noise, sigma, dt, sigma_up), with the magnitude expressions the
    bound is built on; ``euler_coefs64`` / ``ancestral_coefs64`` give (dt, sigma_up) from the two float32 sigmas of a step;
  * ``euler_step_f32``: the same expressions in float32 with every scalar held as a float32 0-dim tensor, in the kernel's order -- what
    gmd_euler_step must reproduce bit for bit given its float coefficients;
  * ``RefEulerScheduler`` / ``RefEulerAncestralScheduler``: small CPU schedulers around ``step64`` with the protocol the loops of
    oracle/pipelines.py drive; ``dual_loop_sigma``: the dual-UNet loop in sigma space (no reference behaviour exists, see there).

The bound (u = 2^-24, first order).  Per element the float32 step is
    p0 = x - s eps;   d = (x - p0) / s;   r = x + d dt;   [r = r + n su]
with s, dt, su float32 scalars.  Write A_p0 = |x| + s |eps|, A_d = (|x| + A_p0) / s (every operand replaced by its magnitude, every
subtraction by an addition) and A = |x| + A_d |dt| + |n| su.  Given exact scalars:
    p0: two roundings (product, difference) of terms <= A_p0                                     |d p0| <= 2 u A_p0
    x - p0: carries d p0 and rounds once, |x - p0| <= |x| + A_p0: <= u (3 A_p0 + |x|) <= 3 u s A_d
    d: that over s plus one rounding of |d| <= A_d                                               |d d| <= 4 u A_d
    d dt: (4 u A_d) |dt| + one rounding;  x + d dt: one rounding of |r| <= |x| + A_d |dt|         <= u (6 A_d |dt| + |x|)
    n su: one rounding;  the sum: one rounding of <= A                                           <= u (7 A_d |dt| + 2 |x| + 2 |n| su)
so the whole step stays within 7 u A: ROUNDINGS = 7, the count of roundings on the longest path (product, difference, difference,
quotient, product, sum, sum).  The scalars add A_d |D dt| + |n| |D su|, where D dt and D su are the errors of the host's float32
scalars against the exact functions of the same two float32 sigmas sf > st (``coef_err``):
    Euler      dt = fl(st - sf): one rounding                                                    |D dt| <= u |dt|
    ancestral  su = fl(sqrt(fl(fl(fl(st^2) fl(fl(sf^2) - fl(st^2))) / fl(sf^2)))): the difference c = sf^2 - st^2 has absolute error
               u (sf^2 + st^2 + c), relative rho_c = u (1 + (sf^2 + st^2) / c); the product and the quotient add 4 u (two operand and
               two own roundings); the root halves the sum and rounds once:                      rho_su = u (3.5 + (sf^2 + st^2) / (2 c))
               sd = fl(sqrt(fl(fl(st^2) - fl(su^2)))), exact value st^2 / sf: the difference m = st^4 / sf^2 has absolute error
               u st^2 + (2 rho_su + u) su^2 + u m; the root halves its relative error and rounds:  rho_sd = rho_m / 2 + u
               dt = fl(sd - sf):                                                                 |D dt| <= rho_sd sd + u |dt|
The pred_original_sample p0 is within 2 u A_p0.

Identities (tests/test_euler_cpu.py), each per step from a common state.  E32 / D32 are the product's float32 host steps, E64 / D64
the float64 functions here and in tests/ddim_ref.py; the test scales its input in float64 and rounds once, xs = fl(x c), c = (1 + sf^2)^.5,
and divides the result in float64 by cn = (1 + st^2)^.5:
    |E32(xs) / cn - D32(x)| <= |E32(xs) - E64(xs)| / cn  +  |E64(xs) / cn - D64(x)|  +  |D64(x) - D32(x)|.
The first term is the bound above, the third ddim_ref.bound.  The middle one (``identity_slack``) is exact arithmetic on slightly
different scalars: with sigma* = ((1 - a) / a)^.5 exactly, E(x c*) / cn* == D(x) (x' = x c*/cn* + eps (st* - sf*) / cn*, and
su*^2 / (1 + st*^2) is DDIM's variance at eta = 1), while the table holds sigma = sigma* (1 + delta), |delta| <= 3 u (difference,
quotient and a root of at most one ulp), which moves c by at most 3 u relative as well.  Hence
    x term      xs / cn against x c* / cn*: (1 + u)(1 + 3u) / (1 - 3u)                            <= 7 u |x| c / cn
    eps term    Euler: |D(st - sf)| <= 3 u (sf + st), over cn: + 3 u |dt|                         <= 6 u |eps| (sf + st) / cn
                ancestral: sd = st^2 / sf moves by 9 u sd, sf by 3 u sf, cn by 3 u                <= 12 u |eps| (sd + sf) / cn
    noise term  su^2 = st^2 - st^4 / sf^2: |D su^2| <= 3 u (2 st^2 + 6 st^4 / sf^2), D su = D su^2 / (2 su), cn: + 3 u su
                                                                                                 <= |n| (3 u (st^2 + 3 st^4 / sf^2) / su + 3 u su) / cn
The perfect predictor: x = fl(x0 + sf e) rounded once from float64 (u |x|, and the exact step has slope 1 in x), model output e: the
step lands on x0 + st e within the step's own bound plus u |x|.
"""
import copy
from types import SimpleNamespace

import numpy as np
import torch

U_F32 = 2.0 ** -24
ROUNDINGS = 7
F32, F64 = torch.float32, torch.float64


# ---------------------------------------------------------------------------------------------------------------------------
# schedules
# ---------------------------------------------------------------------------------------------------------------------------
def alphas_cumprod(beta_start=0.0001, beta_end=0.02, beta_schedule="linear", num_train_timesteps=1000):
    """The float32 table every scheduler of the project starts from (torch float32 cumprod, as diffusers builds it)."""
    if beta_schedule == "linear":
        betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=F32)
    else:
        assert beta_schedule == "scaled_linear"
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=F32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def train_sigmas(ac):
    """((1 - a) / a) ** 0.5 evaluated in float32 on the table (diffusers does), as float64 values."""
    return (((1 - ac) / ac) ** 0.5).numpy().astype(np.float64)


def sigma_to_t(sigma, table):
    """The fractional train timestep at which the log-sigma table, linear between its entries, equals log(sigma); clipped to the ends."""
    return np.interp(np.log(np.maximum(sigma, 1e-10)), np.log(table), np.arange(len(table), dtype=np.float64))


def schedule64(ac, n=None, spacing="linspace", karras=False, steps_offset=0, sigmas=None):
    """(timesteps [n], sigmas [n + 1]) in float64.  ``sigmas``: a custom schedule including its terminal value."""
    table = train_sigmas(ac)
    T = len(table)
    if sigmas is not None:
        sig = np.asarray(sigmas, np.float32).astype(np.float64)
        return sigma_to_t(sig[:-1], table), sig
    if spacing == "linspace":
        ts = np.linspace(0, T - 1, n)[::-1].astype(np.float32).astype(np.float64)  # rounded to float32 before the interpolation
    elif spacing == "leading":
        ts = (np.arange(0, n) * (T // n)).round()[::-1].astype(np.float64) + steps_offset
    else:
        assert spacing == "trailing"
        ts = np.arange(T, 0, -T / n).round() - 1
    sig = np.interp(ts, np.arange(T), table)
    if karras:
        lo, hi = sig[-1] ** (1 / 7.0), sig[0] ** (1 / 7.0)
        sig = (hi + np.linspace(0, 1, n) * (lo - hi)) ** 7.0
        ts = sigma_to_t(sig, table)
    return ts, np.concatenate([sig, [0.0]])


def init_noise_sigma64(sigmas, spacing):
    m = float(np.max(sigmas))
    return m if spacing in ("linspace", "trailing") else (m * m + 1) ** 0.5


def ulp32(v):
    """The float32 spacing at |v| (float64 array in, float64 out); 0 at 0, where a float32 result must be exact."""
    v = np.abs(np.asarray(v, np.float64))
    return np.where(v == 0, 0.0, np.spacing(v.astype(np.float32)).astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------------------
# steps
# ---------------------------------------------------------------------------------------------------------------------------
def euler_coefs64(sf, st):
    """(dt, sigma_up) of the Euler step between the float32 sigmas sf > st (Python floats)."""
    return float(st) - float(sf), 0.0


def ancestral_coefs64(sf, st):
    """(dt = sigma_down - sf, sigma_up) of the ancestral step, in their well-conditioned forms: sigma_down = st^2 / sf,
    sigma_up = st ((sf - st)(sf + st))^.5 / sf."""
    sf, st = float(sf), float(st)
    return st * st / sf - sf, st * ((sf - st) * (sf + st)) ** 0.5 / sf


def coef_err(sf, st, ancestral):
    """(|D dt|, |D sigma_up|): the host's float32 scalars against the exact functions of the same float32 sigmas (module docstring)."""
    sf, st, u = float(sf), float(st), U_F32
    if not ancestral:
        return u * abs(st - sf), 0.0
    if st == 0.0:
        return 0.0, 0.0  # su = sd = 0 and dt = fl(0 - sf) = -sf, all exact
    dt, su = ancestral_coefs64(sf, st)
    c = sf * sf - st * st
    rho_su = u * (3.5 + (sf * sf + st * st) / (2 * c))
    m = st ** 4 / sf ** 2
    rho_m = (u * st * st + (2 * rho_su + u) * su * su + u * m) / m
    rho_sd = rho_m / 2 + u
    return rho_sd * (st * st / sf) + u * abs(dt), rho_su * su


def step64(eps, x, noise, sigma, dt, sigma_up=0.0):
    """(x_prev, p0, mags) in float64; ``noise`` None = no noise term.  mags = (A, A_d, A_p0, |noise|) for ``bound``."""
    e, s = eps.to(F64), x.to(F64)
    sigma, dt, sigma_up = float(sigma), float(dt), float(sigma_up)
    p0 = s - sigma * e
    d = (s - p0) / sigma
    r = s + d * dt
    a_p0 = s.abs() + sigma * e.abs()
    a_d = (s.abs() + a_p0) / sigma
    a = s.abs() + a_d * abs(dt)
    n_abs = torch.zeros_like(s)
    if noise is not None:
        r = r + noise.to(F64) * sigma_up
        n_abs = noise.to(F64).abs()
        a = a + n_abs * sigma_up
    return r, p0, (a, a_d, a_p0, n_abs)


def bound(mags, d_dt=0.0, d_su=0.0):
    a, a_d, _, n_abs = mags
    return ROUNDINGS * U_F32 * a + a_d * d_dt + n_abs * d_su


def bound_p0(mags):
    return 2 * U_F32 * mags[2]


def identity_slack(x, eps, noise, sf, st, ancestral):
    """|E64(xs) / cn - D64(x)| of the DDIM identity (module docstring), per element, float64."""
    sf, st, u = float(sf), float(st), U_F32
    c, cn = (1 + sf * sf) ** 0.5, (1 + st * st) ** 0.5
    xa, ea = x.to(F64).abs(), eps.to(F64).abs()
    out = 7 * u * xa * c / cn
    if not ancestral:
        return out + 6 * u * ea * (sf + st) / cn
    dt, su = ancestral_coefs64(sf, st)
    out = out + 12 * u * ea * (st * st / sf + sf) / cn
    if su > 0:
        out = out + noise.to(F64).abs() * (3 * u * (st * st + 3 * st ** 4 / sf ** 2) / su + 3 * u * su) / cn
    return out


def _s(v):
    return torch.tensor(float(v), dtype=F32)  # a scalar the kernel receives as ``float``


def euler_step_f32(eps, x, coefs, noise=None):
    """(x_prev, pred_x0) of gmd_euler_step given the guided eps, as float32 torch expressions in the kernel's order;
    coefs = (sigma_hat, dt, sigma_up).  The noise is added whenever it is given."""
    sh, dt, su = (_s(c) for c in coefs)
    p0 = x - sh * eps
    d = (x - p0) / sh
    r = x + d * dt
    if noise is not None:
        r = r + noise * su
    return r, p0


def pack_scaled_ref(s0, s1, div, dup, cp, dtype):
    """gmd_pack_unet_input_scaled: (x / div).to(dtype) per source, NCHW -> [dup * B, HW, cp] channels-last, padding channels zero."""
    parts = [(s0 / _s(div[0])).to(dtype)] + ([] if s1 is None else [(s1 / _s(div[1])).to(dtype)])
    src = torch.cat(parts, 1)
    B, C = src.shape[:2]
    out = torch.zeros(B, src[0, 0].numel(), cp, dtype=dtype)
    out[:, :, :C] = src.reshape(B, C, -1).permute(0, 2, 1)
    return torch.cat([out] * dup, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# schedulers for the oracle loops
# ---------------------------------------------------------------------------------------------------------------------------
class RefEulerScheduler:
    """The scheduler protocol of oracle/pipelines.py around ``step64``.  The step is selected by a counter (the loops call
    ``scale_model_input`` and ``step`` once per iteration, in that order); timesteps are float32, sigmas float32 values."""

    order = 1
    ancestral = False

    def __init__(self, timestep_spacing="linspace", use_karras_sigmas=False, steps_offset=0, num_train_timesteps=1000, beta_start=0.00085,
                 beta_end=0.012, beta_schedule="scaled_linear"):
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, steps_offset=steps_offset, timestep_spacing=timestep_spacing,
                                      use_karras_sigmas=use_karras_sigmas)
        self.alphas_cumprod = alphas_cumprod(beta_start, beta_end, beta_schedule, num_train_timesteps)
        self.timesteps = self.sigmas = None
        self.index = 0

    def set_timesteps(self, num_inference_steps, device=None):
        c = self.config
        ts, sig = schedule64(self.alphas_cumprod, num_inference_steps, c.timestep_spacing, c.use_karras_sigmas, c.steps_offset)
        self.timesteps = torch.from_numpy(ts.astype(np.float32))
        self.sigmas = [float(v) for v in sig.astype(np.float32)]
        self.index = 0

    @property
    def init_noise_sigma(self):
        return float(np.float32(init_noise_sigma64(np.array(self.sigmas), self.config.timestep_spacing)))

    def divisor(self):
        return float(np.float32((np.float32(self.sigmas[self.index]) ** 2 + np.float32(1)) ** np.float32(0.5)))

    def scale_model_input(self, sample, timestep=None):
        return sample / self.divisor()

    def coefs(self):
        sf, st = self.sigmas[self.index], self.sigmas[self.index + 1]
        return (sf,) + (ancestral_coefs64(sf, st) if self.ancestral else euler_coefs64(sf, st))

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        sf, dt, su = self.coefs()
        noise = None
        if self.ancestral:  # drawn at EVERY step, the last included
            noise = torch.randn(model_output.shape, generator=generator, dtype=model_output.dtype,
                                device=generator.device if generator is not None else model_output.device).to(model_output.device)
        prev, p0, _ = step64(model_output, sample, noise, sf, dt, su)
        prev, p0 = prev.to(model_output.dtype), p0.to(model_output.dtype)
        self.index += 1
        return (prev, p0) if not return_dict else SimpleNamespace(prev_sample=prev, pred_original_sample=p0)


class RefEulerAncestralScheduler(RefEulerScheduler):
    ancestral = True


@torch.no_grad()
def dual_loop_sigma(unet, gm_unet, scheduler, prompt_embeds, negative_prompt_embeds, latents, num_inference_steps=50, guidance_scale=7.5,
                    guidance_rescale=0.0, generator=None, record=None):
    """The dual-UNet loop with a sigma-space scheduler, defined by the mathematics (the reference's loop cannot run one: it indexes
    alphas_cumprod with the timestep and overwrites the GM state with its scaled copy): the SDR UNet reads latents / (sigma^2 + 1)^.5;
    x0 = latents - sigma eps (the pre-step latents); the GM UNet reads cat([x0, gm_latents / (sigma^2 + 1)^.5]) -- x0 unscaled; neither
    state is ever scaled; a shared generator is consumed SDR first, GM second.  Otherwise oracle.pipelines.dual_loop."""
    from oracle.pipelines import _cfg

    do_cfg = guidance_scale > 1
    embeds = torch.cat([negative_prompt_embeds, prompt_embeds]) if do_cfg else prompt_embeds
    gm_embeds = embeds[negative_prompt_embeds.shape[0]:] if do_cfg else embeds
    scheduler.set_timesteps(num_inference_steps)
    latents = latents * scheduler.init_noise_sigma
    gm_latents = latents.clone()
    gm_scheduler = copy.deepcopy(scheduler)
    for t in scheduler.timesteps:
        x = torch.cat([latents] * 2) if do_cfg else latents
        eps = unet(scheduler.scale_model_input(x, t), t, encoder_hidden_states=embeds, return_dict=False)[0]
        if do_cfg:
            eps = _cfg(eps, guidance_scale, guidance_rescale)
        latents, x0 = scheduler.step(eps, t, latents, generator=generator, return_dict=False)
        gm_in = torch.cat([x0, gm_scheduler.scale_model_input(gm_latents, t)], dim=1)
        gm_eps = gm_unet(gm_in, t, encoder_hidden_states=gm_embeds, return_dict=False)[0]
        gm_latents = gm_scheduler.step(gm_eps, t, gm_latents, generator=generator, return_dict=False)[0]
        if record is not None:
            record.append((latents.clone(), gm_latents.clone()))
    return latents, gm_latents
