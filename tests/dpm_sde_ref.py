"""Reference for the DPM-Solver++ / SDE-DPM-Solver++ multistep step (csrc/latent_step.hip dpm_step_kernel and dpm_sde_step_kernel,
components.DPMSolverMultistepScheduler): plain helper module in the style of tests/ddim_ref.py.  Nothing here uses the product class or
the library.

  * ``scalars64`` / ``dpm_step64``: the six update rows of diffusers' ``DPMSolverMultistepScheduler`` (epsilon prediction; algorithm
    dpmsolver++ or sde-dpmsolver++; first order, second-order midpoint, second-order heun) restated in float64 as a plain function of
    (eps, x, m1, noise) and the two or three sigma-table entries of the step, with the magnitude expression A the per-element bound is
    built on;
  * ``dpm_step_f32``: the kernels' float32 expressions, in the kernels' order, from the raw coefficients the launchers receive -- what
    they must reproduce bit for bit;
  * ``RefDPMSolverScheduler``: a small CPU scheduler object around ``dpm_step64`` (leading spacing, as the oracle's own schedulers) with
    the ``step(model_output, t, sample, generator=None, return_dict=True)`` signature the loops of oracle/pipelines.py drive.  It keeps
    the multistep history and draws noise at EVERY step when the algorithm is the SDE one.

The update.  With s = sigma-table entry, alpha = 1 / (s^2 + 1)^.5, sigma = s alpha, lambda = log alpha - log sigma, h = lambda_t - lambda_s0,
h0 = lambda_s0 - lambda_s1, r0 = h0 / h, E = exp(-h), E2 = exp(-2h), m0 = (x - sigma_s0 eps) / alpha_s0, D1 = (1 / r0) (m0 - m1):
    dpmsolver++      x_prev = c_x x - c_m m0 [- c_h D1]           c_x = sigma_t / sigma_s0,    c_m = alpha_t (E - 1)
                     c_h = .5 c_m (midpoint),  -alpha_t ((E - 1) / h + 1) (heun)
    sde-dpmsolver++  x_prev = c_x x + c_m m0 [+ c_h D1] + c_n z   c_x = sigma_t / sigma_s0 E,  c_m = alpha_t (1 - E2),  c_n = sigma_t (1 - E2)^.5
                     c_h = .5 c_m (midpoint),  alpha_t ((1 - E2) / (-2h) + 1) (heun)

The bound.  A float32 evaluation differs from the exact value by at most (number of roundings on the longest path) 2^-24 (magnitude of
that path) to first order.  One rounding = one relative error of 2^-24: +, -, *, / and the square root are correctly rounded (1 each);
log and exp of the float32 library are taken as faithful (below one ulp = 2 roundings each).  An error passes through log as an ABSOLUTE
error and through exp as a relative one, so the magnitudes carry the factor
    Lam = 1 + L_t + L_s0 + L_s1,   L = |log alpha| + |log sigma|      (L_s1 = 0 at first order; L_t = 0 when s_t = 0: see below)
and every cancelling difference is replaced by the sum of its terms' magnitudes, as in ddim_ref.py.  Counting, with u = 2^-24:
    alpha  4 (square, sum, root, quotient)            sigma  5 (alpha, product)
    lambda: |err| <= u (4 + 2 |log alpha| + 5 + 2 |log sigma| + L) <= 9 u (1 + L);   h, h0: |err| <= 18 u Lam
    E   = exp(-h):   relative 18 Lam + 2        -> 20 roundings on E Lam
    E2  = exp(-2h):  relative 36 Lam + 2        -> 38 roundings on E2 Lam
    1 - E2  : 38 + 1 -> 39 on G  = 1 + E2 Lam;     E - 1 : 20 + 1 -> 21 on Gd = 1 + E Lam
    sde  c_x = sigma_t / sigma_s0 E : 5 + 5 + 1 + 20 + 1 = 32 on (sigma_t / sigma_s0) E Lam
         c_m = alpha_t (1 - E2)     : 4 + 39 + 1         = 44 on alpha_t G
         c_n = sigma_t (1 - E2)^.5  : the root halves a relative error, i.e. divides the absolute one by 2 (1 - E2)^.5:
                                      39 / 2 + 1 -> 21 on G / (1 - E2)^.5;  5 + 21 + 1 = 27 on sigma_t G / (1 - E2)^.5
         c_h heun: (1 - E2) / (-2h): 39 (numerator) + 18 Lam / h (denominator, relative) + 1 -> 40 on Q = G / (2h) (1 + Lam / h);
                   + 1 -> 41 on Q + 1;  4 + 41 + 1 = 46 on alpha_t (Q + 1).      c_h midpoint = .5 c_m exactly: 44 on .5 alpha_t G
    ode  c_x = sigma_t / sigma_s0   : 11;   c_m = alpha_t (E - 1) : 4 + 21 + 1 = 26 on alpha_t Gd
         c_h heun: (E - 1) / h : 21 + 18 Lam / h + 1 -> 22 on Qd = Gd / h (1 + Lam / h);  + 1 -> 23;  4 + 23 + 1 = 28 on alpha_t (Qd + 1)
    m0   = (x - sigma_s0 eps) / alpha_s0 : 5 + 1 + 1 + 4 + 1 = 12 on A_m0 = (|x| + sigma_s0 |eps|) / alpha_s0
    1/r0 = 1 / (h0 / h) : relative 18 Lam / h0 + 18 Lam / h + 2 -> 18 on (1 / r0) rho,  rho = 1 + Lam / h + Lam / h0
    D1   = (1 / r0) (m0 - m1) : 12 + 1 + 18 + 1 = 32 on A_D1 = (1 / r0) rho (A_m0 + |m1|)
    terms (coefficient + operand + product):  c_x x : 33;  c_m m0 : 44 + 12 + 1 = 57;  c_h D1 (sde heun) : 46 + 32 + 1 = 79;  c_n z : 28
    x_prev: three sums, each one rounding on a partial sum no larger than A; the longest path is c_h D1 through the last two sums:
                                      ROUNDINGS = 79 + 2 = 81
(the deterministic rows are shorter: 28 + 32 + 1 + 1 = 62) on
    A = |c_x| Lam |x| + alpha_t G' A_m0 + C_h A_D1 + sigma_t G / (1 - E2)^.5 |z|
with G' = G (sde) or Gd (ode), C_h = alpha_t (Q + 1) / alpha_t (Qd + 1) (heun) or .5 alpha_t G' (midpoint), and the last term only for sde.
m0 itself is bounded by 12 u A_m0 <= ROUNDINGS u A_m0.

The last step of a ``final_sigmas_type="zero"`` schedule has s_t = 0: sigma_t = 0, alpha_t = 1, lambda_t = +inf, h = +inf, E = E2 = 0, all
EXACTLY in float32 as in float64 (log 0 = -inf and exp(-inf) = 0 are exact), so c_x = 0, |c_m| = 1, c_n = 0 carry no error; L_t, which would
be infinite and multiplies only E and E2, is taken as 0 there.  That step is always first order.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

U_F32 = 2.0 ** -24
ROUNDINGS = 81
F32, F64 = torch.float32, torch.float64
SDE, ODE = "sde-dpmsolver++", "dpmsolver++"


def _alpha_sigma_lambda(s):
    s = float(s)
    alpha = 1.0 / (s * s + 1.0) ** 0.5
    sigma = s * alpha
    if s == 0.0:
        return alpha, sigma, math.inf, 0.0
    return alpha, sigma, math.log(alpha) - math.log(sigma), abs(math.log(alpha)) + abs(math.log(sigma))


def scalars64(s_s0, s_t, s_s1=None):
    """The step's scalars in float64 from its sigma-table entries (Python floats: the float32 table entries, exactly).  ``s_s1`` None =
    first order.  Returns a namespace: alpha_s0, sigma_s0, alpha_t, sigma_t, h, E, E2, inv_r0 (0 at first order), Lam, rho."""
    a0, g0, l0, L0 = _alpha_sigma_lambda(s_s0)
    at, gt, lt, Lt = _alpha_sigma_lambda(s_t)
    h = lt - l0
    lam, inv_r0, rho = 1.0 + Lt + L0, 0.0, 1.0
    if s_s1 is not None:
        _, _, l1, L1 = _alpha_sigma_lambda(s_s1)
        h0 = l0 - l1
        lam += L1
        inv_r0 = h / h0
        rho = 1.0 + lam / h + lam / h0
    return SimpleNamespace(alpha_s0=a0, sigma_s0=g0, alpha_t=at, sigma_t=gt, h=h, E=math.exp(-h), E2=math.exp(-2.0 * h), inv_r0=inv_r0,
                           Lam=lam, rho=rho)


def coefs64(sc, algorithm, solver_type, order):
    """(c_x, c_m, c_h, c_n) of x_prev = c_x x + c_m m0 + c_h D1 + c_n z -- signs included, so the deterministic rows have c_m, c_h with
    the sign of the table's minus -- and their magnitudes (C_x, C_m, C_h, C_n) as the module docstring defines them."""
    heun = solver_type == "heun"
    if algorithm == SDE:
        v = 1.0 - sc.E2
        G = 1.0 + sc.E2 * sc.Lam
        c_x, c_m, c_n = sc.sigma_t / sc.sigma_s0 * sc.E, sc.alpha_t * v, sc.sigma_t * v ** 0.5
        C_x, C_m = c_x * sc.Lam, sc.alpha_t * G
        C_n = sc.sigma_t * G / v ** 0.5 if sc.sigma_t > 0 else 0.0
        c_h = C_h = 0.0
        if order == 2:
            Q = G / (2.0 * sc.h) * (1.0 + sc.Lam / sc.h)
            c_h, C_h = (sc.alpha_t * (v / (-2.0 * sc.h) + 1.0), sc.alpha_t * (Q + 1.0)) if heun else (0.5 * c_m, 0.5 * C_m)
        return (c_x, c_m, c_h, c_n), (C_x, C_m, C_h, C_n)
    assert algorithm == ODE
    Gd = 1.0 + sc.E * sc.Lam
    c_x, c_m = sc.sigma_t / sc.sigma_s0, -(sc.alpha_t * (sc.E - 1.0))
    C_x, C_m = c_x * sc.Lam, sc.alpha_t * Gd
    c_h = C_h = 0.0
    if order == 2:
        Qd = Gd / sc.h * (1.0 + sc.Lam / sc.h)
        c_h, C_h = (sc.alpha_t * ((sc.E - 1.0) / sc.h + 1.0), sc.alpha_t * (Qd + 1.0)) if heun else (0.5 * c_m, 0.5 * C_m)
    return (c_x, c_m, c_h, 0.0), (C_x, C_m, C_h, 0.0)


def dpm_step64(eps, x, m1, noise, s_s0, s_t, s_s1, algorithm, solver_type):
    """(x_prev, m0, A, A_m0) in float64.  ``s_s1`` None = first order (``m1`` is then unused); ``noise`` is added iff the algorithm is
    the SDE one (it may be None otherwise)."""
    order = 1 if s_s1 is None else 2
    sc = scalars64(s_s0, s_t, s_s1)
    (c_x, c_m, c_h, c_n), (C_x, C_m, C_h, C_n) = coefs64(sc, algorithm, solver_type, order)
    e, s = eps.to(F64), x.to(F64)
    m0 = (s - sc.sigma_s0 * e) / sc.alpha_s0
    a_m0 = (s.abs() + sc.sigma_s0 * e.abs()) / sc.alpha_s0
    r = c_x * s + c_m * m0
    a = C_x * s.abs() + C_m * a_m0
    if order == 2:
        p = m1.to(F64)
        r = r + c_h * (sc.inv_r0 * (m0 - p))
        a = a + C_h * (abs(sc.inv_r0) * sc.rho * (a_m0 + p.abs()))
    if algorithm == SDE:
        z = noise.to(F64)
        r = r + c_n * z
        a = a + C_n * z.abs()
    return r, m0, a, a_m0


def bound(a):
    return ROUNDINGS * U_F32 * a


def _s(v):
    return torch.tensor(float(v), dtype=F32)  # a scalar the kernel receives as ``float``


def dpm_step_f32(eps, x, order, coefs, noise=None, m1=None, sde=True):
    """(x_prev, m0, x0) of gmd_dpm_sde_step (``sde``; the noise is always added) or gmd_dpm_step (not ``sde``) given the guided eps, as
    float32 torch expressions in the kernel's order; coefs = (sigma_s0, alpha_s0, c_x, c_m, c_h, inv_r0, c_n, sqrt_a, sqrt_1ma) -- the
    launcher's own scalars, c_n unused when not ``sde``."""
    g0, a0, c_x, c_m, c_h, inv_r0, c_n, sa, s1 = (_s(c) for c in coefs)
    x0 = (x - s1 * eps) / sa
    m0 = (x - g0 * eps) / a0
    if sde:
        r = c_x * x + c_m * m0
        if order == 2:
            r = r + c_h * (inv_r0 * (m0 - m1))
        r = r + c_n * noise
    else:
        r = c_x * x - c_m * m0
        if order == 2:
            r = r - c_h * (inv_r0 * (m0 - m1))
    return r, m0, x0


class RefDPMSolverScheduler:
    """The scheduler protocol of oracle/pipelines.py around ``dpm_step64`` (leading spacing, as the oracle's own schedulers): the
    sigma table, the order rule (first step, ``solver_order`` 1 and the lower-order final step are first order) and the history."""

    order = 1

    def __init__(self, algorithm_type=ODE, solver_type="midpoint", solver_order=2, num_train_timesteps=1000, beta_start=0.00085,
                 beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1, lower_order_final=True, euler_at_final=False,
                 final_sigmas_type="zero"):
        assert algorithm_type in (SDE, ODE) and solver_type in ("midpoint", "heun") and solver_order in (1, 2)
        self.config = SimpleNamespace(algorithm_type=algorithm_type, solver_type=solver_type, solver_order=solver_order,
                                      num_train_timesteps=num_train_timesteps, steps_offset=steps_offset, lower_order_final=lower_order_final,
                                      euler_at_final=euler_at_final, final_sigmas_type=final_sigmas_type)
        if beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=F32)
        else:
            assert beta_schedule == "scaled_linear"
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=F32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.init_noise_sigma = 1.0
        self.timesteps = None

    def set_timesteps(self, num_inference_steps, device=None):
        c = self.config
        ratio = c.num_train_timesteps // (num_inference_steps + 1)
        ts = (np.arange(0, num_inference_steps + 1) * ratio).round()[::-1][:-1].copy().astype(np.int64) + c.steps_offset
        table = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        sig = np.interp(ts, np.arange(0, len(table)), table)
        last = float(table[0]) if c.final_sigmas_type == "sigma_min" else 0.0
        self.sigmas = [float(v) for v in np.concatenate([sig, [last]]).astype(np.float32)]
        self.timesteps = torch.from_numpy(ts)
        self.num_inference_steps = len(ts)
        self.i = 0
        self.m1 = None

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        c, i, n = self.config, self.i, self.num_inference_steps
        assert int(timestep) == int(self.timesteps[i])
        lower_final = i == n - 1 and (c.euler_at_final or (c.lower_order_final and n < 15) or c.final_sigmas_type == "zero")
        first = c.solver_order == 1 or i == 0 or lower_final
        noise = None
        if c.algorithm_type == SDE:  # drawn at EVERY step, the last included
            noise = torch.randn(model_output.shape, generator=generator, dtype=F32,
                                device=generator.device if generator is not None else model_output.device).to(model_output.device)
        prev, m0, _, _ = dpm_step64(model_output, sample, self.m1, noise, self.sigmas[i], self.sigmas[i + 1],
                                    None if first else self.sigmas[i - 1], c.algorithm_type, c.solver_type)
        self.m1 = m0
        self.i += 1
        prev = prev.to(model_output.dtype)
        return (prev,) if not return_dict else SimpleNamespace(prev_sample=prev)
