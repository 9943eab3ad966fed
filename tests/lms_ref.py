"""Reference for components.LMSDiscreteScheduler and csrc/latent_step.hip lms_step_kernel: plain helper module in the style of
tests/euler_ref.py, whose float64 schedules (``schedule64``) it reuses.  Nothing here uses the product classes or the library.  The
arithmetic restates diffusers ~0.33 from memory (SURVEY.md convention [3P-memory]); this file is the pin.

  * ``coef_exact``: the integral over [s_t, s_{t+1}] of the Lagrange basis polynomial on the nodes s_{t-k}, k < order, in exact rational
    arithmetic (``fractions.Fraction``) over the float32 table values; ``coefs64`` rounds each to float64 once;
    ``interpolant_integral64``: the integral of the interpolating polynomial through given samples, in Newton's form;
  * ``step64``: one step in float64 as a plain function of (eps, x, sigma, coefficients, history), with the magnitude expressions the bound
    is built on;
  * ``lms_step_f32``: the same expressions in float32 with every scalar held as a float32 0-dim tensor, in the kernel's order -- what
    gmd_lms_step must reproduce bit for bit given its float coefficients;
  * ``RefLMSScheduler``: a small CPU scheduler around ``step64`` with the protocol the loops of oracle/pipelines.py and
    euler_ref.dual_loop_sigma drive.

The bound (u = 2^-24, first order).  Per element the float32 step of order k is
    p0 = x - s eps;   d0 = (x - p0) / s;   acc = 0 + c0 d0;   acc = acc + cj dj (j = 1 .. k-1);   r = x + acc
with s and the cj float32 scalars and d1 .. d(k-1) float32 tensors handed in (exact inputs).  Write A_p0 = |x| + s |eps|,
D0 = (|x| + A_p0) / s (every operand replaced by its magnitude, every subtraction by an addition: the derivative's magnitude expression;
the computed d0 comes out of a cancelling difference, so its error scales with |x| / s, not with |d0|), Dj = |dj| for j >= 1,
S = sum_j |cj| Dj and A = |x| + s |eps| + S.  Given exact scalars:
    p0: two roundings (product, difference) of terms <= A_p0                                       |d p0| <= 2 u A_p0
    x - p0: carries d p0 and rounds once, |x - p0| <= |x| + A_p0 = s D0:                            <= u (2 A_p0 + s D0) <= 3 u s D0
    d0: that over s plus one rounding of |d0| <= D0                                                |d d0| <= 4 u D0
    c0 d0: 4 u |c0| D0 plus one rounding                                                           <= 5 u |c0| D0
    0 + c0 d0: exact
    cj dj (j >= 1): one rounding each                                                              <= u |cj| Dj
    the k - 1 <= 3 additions into acc: every partial sum is <= S, one rounding each                <= 3 u S
    x + acc: one rounding of <= |x| + S                                                            <= u (|x| + S)
in total <= 5 u S + 3 u S + u (|x| + S) <= 9 u A: ROUNDINGS = 9, the count of roundings on the longest path (product, difference,
difference, quotient, product, three sums, the last sum).  It scales with sum |cj| Dj, NOT with |dt| = |s_{t+1} - s_t|: the coefficients
alternate in sign and sum |cj| / |dt| reaches 175 on the schedules of the tests.
The scalars add sum_j |D cj| Dj, with D cj the error of the float32 coefficient the step uses against the exact rational one: one rounding
to float32 of a float64 value that is itself within 2^-48 sum |c| of exact (tests/test_lms_cpu.py checks that), so
|D cj| <= u |cj| + 2^-48 sum_i |ci| (``coef_err``).  s is a float32 table value: both sides use it exactly.
The pred_original_sample p0 is within 2 u A_p0, the derivative within 4 u D0.
"""
from fractions import Fraction
from types import SimpleNamespace

import torch

import euler_ref as E

U_F32 = 2.0 ** -24
ROUNDINGS = 9
COEF_TOL = 2.0 ** -48  # of sum_j |c_j|: what the float64 coefficients of the product are held to
F32, F64 = torch.float32, torch.float64


# ---------------------------------------------------------------------------------------------------------------------------
# coefficients
# ---------------------------------------------------------------------------------------------------------------------------
def coef_exact(sigmas, order, t, j):
    """Exact integral over [sigmas[t], sigmas[t + 1]] of prod_{k < order, k != j} (tau - s_{t-k}) / (s_{t-j} - s_{t-k}) as a Fraction;
    ``sigmas``: float32 table values (any floats: each is taken as the exact rational it is)."""
    s = [Fraction(float(v)) for v in sigmas]
    poly = [Fraction(1)]  # ascending powers of tau
    for k in range(order):
        if k == j:
            continue
        den = s[t - j] - s[t - k]
        nxt = [Fraction(0)] * (len(poly) + 1)
        for p, c in enumerate(poly):  # times (tau - s_{t-k}) / den
            nxt[p + 1] += c / den
            nxt[p] -= c * s[t - k] / den
        poly = nxt
    a, b = s[t], s[t + 1]
    return sum(c * (b ** (p + 1) - a ** (p + 1)) / (p + 1) for p, c in enumerate(poly))


def coefs_exact(sigmas, order, t):
    return [coef_exact(sigmas, order, t, j) for j in range(order)]


def coefs64(sigmas, order, t):
    """The exact coefficients rounded once to float64 (Python floats)."""
    return [float(c) for c in coefs_exact(sigmas, order, t)]


def interpolant_integral64(nodes, values, a, b):
    """Integral over [a, b] of the polynomial of degree len(nodes) - 1 through (nodes[m], values[m]), by Newton's divided differences:
    the differences per element in float64 (``values``: tensors), the integrals of the Newton basis prod_{l < m} (tau - nodes[l]) in
    exact rational arithmetic.  Shares nothing with the Lagrange form of ``coef_exact``."""
    z = [Fraction(float(v)) for v in nodes]
    a, b = Fraction(float(a)), Fraction(float(b))
    dd = [v.to(F64) for v in values]
    total, poly = 0.0, [Fraction(1)]  # ascending powers of tau
    for m in range(len(z)):
        basis = sum(c * (b ** (p + 1) - a ** (p + 1)) / (p + 1) for p, c in enumerate(poly))
        total = total + dd[0] * float(basis)
        dd = [(dd[q + 1] - dd[q]) / float(z[q + m + 1] - z[q]) for q in range(len(dd) - 1)]
        nxt = [Fraction(0)] * (len(poly) + 1)
        for p, c in enumerate(poly):  # times (tau - nodes[m])
            nxt[p + 1] += c
            nxt[p] -= c * z[m]
        poly = nxt
    return total


def coef_err(coefs):
    """|D c_j| per coefficient: the float32 rounding of a float64 value within COEF_TOL sum |c| of the exact one (module docstring)."""
    tot = sum(abs(float(c)) for c in coefs)
    return [U_F32 * abs(float(c)) + COEF_TOL * tot for c in coefs]


# ---------------------------------------------------------------------------------------------------------------------------
# steps
# ---------------------------------------------------------------------------------------------------------------------------
def step64(eps, x, sigma, coefs, hist=()):
    """(x_prev, p0, d, mags) in float64.  ``coefs``: c_0 .. c_{k-1} (floats); ``hist``: the derivatives of the previous steps, newest
    first, of which the first k - 1 are used.  mags = (A, S, D = [D_0 .. D_{k-1}], A_p0) for ``bound``."""
    e, s = eps.to(F64), x.to(F64)
    sigma = float(sigma)
    k = len(coefs)
    assert len(hist) >= k - 1
    p0 = s - sigma * e
    d = (s - p0) / sigma
    ds = [d] + [h.to(F64) for h in hist[:k - 1]]
    r = s + sum(float(c) * dj for c, dj in zip(coefs, ds))
    a_p0 = s.abs() + sigma * e.abs()
    mag_d = [(s.abs() + a_p0) / sigma] + [dj.abs() for dj in ds[1:]]
    big_s = sum(abs(float(c)) * m for c, m in zip(coefs, mag_d))
    return r, p0, d, (s.abs() + sigma * e.abs() + big_s, big_s, mag_d, a_p0)


def bound(mags, d_coefs=None):
    """ROUNDINGS u A plus the scalars' own error sum_j |D c_j| D_j (``d_coefs`` = coef_err(coefs); None: exact scalars)."""
    a, _, mag_d, _ = mags
    out = ROUNDINGS * U_F32 * a
    for dc, m in zip(d_coefs or (), mag_d):
        out = out + dc * m
    return out


def bound_p0(mags):
    return 2 * U_F32 * mags[3]


def bound_d(mags):
    return 4 * U_F32 * mags[2][0]


def _s(v):
    return torch.tensor(float(v), dtype=F32)  # a scalar the kernel receives as ``float``


def lms_step_f32(eps, x, coefs, hist=()):
    """(d, x_prev, pred_x0) of gmd_lms_step given the guided eps, as float32 torch expressions in the kernel's order;
    coefs = (sigma, c_0, .. c_{k-1}): the order is the number of coefficients.  Independent of the scheduler class."""
    sg, cs = _s(coefs[0]), [_s(c) for c in coefs[1:]]
    p0 = x - sg * eps
    d = (x - p0) / sg
    acc = torch.zeros((), dtype=F32) + cs[0] * d  # Python's sum() starts from 0: 0 + (-0.0) is +0.0
    for c, h in zip(cs[1:], hist):
        acc = acc + c * h
    assert len(hist) >= len(cs) - 1
    return d, x + acc, p0


# ---------------------------------------------------------------------------------------------------------------------------
# scheduler for the oracle loops
# ---------------------------------------------------------------------------------------------------------------------------
class RefLMSScheduler(E.RefEulerScheduler):
    """The scheduler protocol of oracle/pipelines.py around ``step64``: tables via euler_ref.schedule64 (float32 values), exact-rational
    coefficients, float64 history.  The step is selected by a counter, as in RefEulerScheduler; the generator the loops pass is unused."""

    def __init__(self, order=4, **kw):
        super().__init__(**kw)
        self.lms_order = order
        self.derivatives = []

    def set_timesteps(self, num_inference_steps, device=None):
        super().set_timesteps(num_inference_steps, device)
        self.derivatives = []

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        i = self.index
        k = min(i + 1, self.lms_order)
        prev, p0, d, _ = step64(model_output, sample, self.sigmas[i], coefs64(self.sigmas, k, i), list(reversed(self.derivatives)))
        self.derivatives = (self.derivatives + [d])[-self.lms_order:]
        prev, p0 = prev.to(model_output.dtype), p0.to(model_output.dtype)
        self.index += 1
        return (prev, p0) if not return_dict else SimpleNamespace(prev_sample=prev, pred_original_sample=p0)
