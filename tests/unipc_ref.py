"""Reference for components.UniPCMultistepScheduler and csrc/latent_step.hip unipc_step_kernel: plain helper module in the style of
tests/lms_ref.py and tests/dpm_sde_ref.py.  Nothing here uses the product class or the library.

  * ``tables64``: timesteps and sigmas (the float32 ``alphas_cumprod`` table every scheduler starts from, everything after it in float64);
  * ``orders``: the corrector / predictor order rule;  ``scalars``: the scalars of one step from the sigma table, written ONCE over an
    arithmetic that is either Python floats (float64 values) or ``Err`` (float64 values that carry a first-order bound on the error of
    the same chain evaluated in float32);
  * ``step64``: one step in float64 as a plain function of (eps, x, last_sample, history) with the magnitude expressions the bound is
    built on;  ``bounds``: the per-element bound;
  * ``unipc_step_f32``: the kernel's float32 expressions in the kernel's order, from the 19 floats the launcher receives -- what
    gmd_unipc_step must reproduce bit for bit;
  * ``RefUniPCScheduler``: the whole scheduler in float64, with the protocol the loops of oracle/pipelines.py drive.

The step (sigma_k = table entry, alpha = 1 / (s^2 + 1)^.5, sg = s alpha, lambda = log alpha - log sg; h1, h2, h3 = the x0 predictions of
the previous 1, 2, 3 steps, newest first; ``last`` = the corrected sample of the previous step):
    x0   = (x - sg_i eps) / alpha_i
    corrector of order p (off: xc = x):  D_k = (h_{k+1} - h1) / r_k (k < p),  acc = sum_{k<p} rho_k D_k + rho_p (x0 - h1),
                                         xc = c_x last - c_m h1 - c_b acc
    predictor of order q:                D'_k = (h_k - x0) / r'_k (k < q),    acc' = sum_{k<q} rho'_k D'_k,
                                         prev = p_x xc - p_m x0 [- p_b acc']           (no p_b term at q = 1)
with c_x = sg_t / sg_s, c_m = alpha_t expm1(-h), c_b = alpha_t B(h) (B = -h for bh1, expm1(-h) for bh2) of the interval, r_k the ratios
of lambda differences, rho the solution of the UniPC paper's system R rho = b (0.5 when it has one unknown).

The bound (u = 2^-24, first order).  Given EXACT scalars, with every operand replaced by its magnitude and every difference by a sum:
    A0  = (|x| + sg |eps|) / alpha                 x0: product, difference, quotient                                 3 u A0
    AD_k = (|h_{k+1}| + |h1|) / |r_k|              D_k: difference, quotient (the h are float32 tensors handed in)   2 u AD_k
    ADp = A0 + |h1|                                x0 - h1: the error of x0 and one rounding                         4 u ADp
    S   = sum_k |rho_k| AD_k + |rho_p| ADp         each product one more rounding (<= 5 u), two sums into acc (<= 2 u S):  7 u S
    Ac  = |c_x||last| + |c_m||h1| + |c_b| S        c_b acc: 8;  c_x last, c_m h1: 1 each;  two differences: 2 on the first two, 1 on all
                                                   xc within 9 u Ac                                  (corrector off: xc = x, Ac = |x|, 0)
    AD'_k = (|h_k| + A0) / |r'_k|                  D'_k: the error of x0, difference, quotient                       5 u AD'_k
    S'  = sum_k |rho'_k| AD'_k                     products 6, one sum 7;  p_b acc': 8
    Ap  = |p_x| Ac + |p_m| A0 + |p_b| S'           p_x xc: 9 + 1 = 10;  p_m x0: 4;  two differences: + 2
                                                   prev within 12 u Ap
ROUNDINGS = 12: the longest path is x0 -> x0 - h1 -> product -> two sums -> c_b acc -> two differences (xc: 9) -> p_x xc -> two differences.
The scalars are not exact: they are float32 chains through log, expm1, cancelling differences of lambdas, h_phi_k = phi_1 / hh - 1 (which
loses 1 / h digits, then 1 / h^2) and a small linear solve.  Their error D c is not counted by hand: ``scalars`` runs the SAME chain once
more over ``Err`` numbers, which carry a running first-order bound -- every +, -, *, / adds one rounding u |result| to the propagated
error of its operands, log / expm1 / ** 0.5 (library functions, taken as faithful) add 2 u |result|, an error passes through log as
e / |v|, through expm1 as exp(v) e.  The solve (LAPACK's LU with partial pivoting, whose operation order is not ours) is bounded by its
backward error, Higham, Accuracy and Stability, Theorem 9.5: (R + DR) rho^ = b with ||DR||_inf <= n^2 gamma_{3n} g_n ||R||_inf,
gamma_{3n} = 3 n u, growth g_n <= 2^(n-1), so |D rho| <= |R^-1| ((E_R + ||DR||_inf) |rho| + E_b) elementwise, E_R and E_b the errors
the entries came in with.  Each D c then multiplies the magnitude of what c multiplies (``bounds``):
    E_x0 = (D sg |eps| + A0 D alpha) / alpha
    E_acc = sum_k (D rho_k AD_k + |rho_k| AD_k D r_k / |r_k|) + D rho_p ADp + |rho_p| E_x0
    E_xc = D c_x |last| + D c_m |h1| + D c_b S + |c_b| E_acc
    E_acc' = sum_k (D rho'_k AD'_k + |rho'_k| (AD'_k D r'_k + E_x0) / |r'_k|)
    E_prev = D p_x Ac + |p_x| E_xc + D p_m A0 + |p_m| E_x0 + D p_b S' + |p_b| E_acc'
The last step of a schedule that ends at sigma 0 has sg_t = 0, alpha_t = 1, h = +inf, expm1(-h) = -1, all EXACTLY in float32 as in
float64: p_x = 0 and p_m = -1 carry no error there, and that step is first order.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

import euler_ref as E

U_F32 = 2.0 ** -24
ROUNDINGS, ROUNDINGS_XC, ROUNDINGS_X0 = 12, 9, 3
F32, F64 = torch.float32, torch.float64


# ---------------------------------------------------------------------------------------------------------------------------
# tables and orders
# ---------------------------------------------------------------------------------------------------------------------------
def tables64(ac, n, spacing="linspace", steps_offset=0, final_sigmas_type="zero"):
    """(timesteps [n] int64, sigmas [n + 1] float64) from the float32 alphas_cumprod table ``ac`` (a torch tensor)."""
    N = len(ac)
    if spacing == "linspace":
        ts = np.linspace(0, N - 1, n + 1).round()[::-1][:-1]
    elif spacing == "leading":
        ts = (np.arange(0, n + 1) * (N // (n + 1))).round()[::-1][:-1] + steps_offset
    else:
        assert spacing == "trailing"
        ts = np.arange(N, 0, -N / n).round() - 1
    ts = ts.astype(np.int64)
    a = ac.numpy().astype(np.float64)
    table = ((1 - a) / a) ** 0.5
    last = table[0] if final_sigmas_type == "sigma_min" else 0.0
    return ts, np.concatenate([np.interp(ts, np.arange(N), table), [last]])


def orders(i, n, solver_order, lower_order_final, disable_corrector=(), prev=None):
    """(corrector order p, predictor order q) of step i of n.  ``prev``: the predictor order of step i - 1 (None: derived from the
    rule, which needs no state: lower_order_nums is min(i, solver_order))."""
    def pred(j):
        q = min(solver_order, n - j) if lower_order_final else solver_order
        return min(q, min(j, solver_order) + 1)

    p = 0
    if i > 0 and (i - 1) not in disable_corrector:
        p = pred(i - 1) if prev is None else prev
    return p, pred(i)


# ---------------------------------------------------------------------------------------------------------------------------
# scalars, over floats or over numbers that carry a running error bound
# ---------------------------------------------------------------------------------------------------------------------------
class Err:
    """A float64 value ``v`` with a first-order bound ``e`` on the error of the same chain evaluated in float32 (module docstring)."""

    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v, self.e = float(v), float(e)

    @staticmethod
    def of(o):
        return o if isinstance(o, Err) else Err(o)

    def _r(self, v, e, k=1):
        return Err(v, e + k * U_F32 * abs(v))

    def __add__(self, o):
        o = Err.of(o)
        return self._r(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = Err.of(o)
        return self._r(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Err.of(o) - self

    def __mul__(self, o):
        o = Err.of(o)
        return self._r(self.v * o.v, abs(self.v) * o.e + abs(o.v) * self.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Err.of(o)
        q = self.v / o.v
        return self._r(q, (self.e + abs(q) * o.e) / abs(o.v))

    def __rtruediv__(self, o):
        return Err.of(o) / self

    def __neg__(self):
        return Err(-self.v, self.e)


def _val(a):
    return a.v if isinstance(a, Err) else a


def _err(a):
    return a.e if isinstance(a, Err) else 0.0


def _log(a):
    return a._r(math.log(a.v), a.e / abs(a.v), 2) if isinstance(a, Err) else math.log(a)


def _expm1(a):
    return a._r(math.expm1(a.v), math.exp(a.v) * a.e, 2) if isinstance(a, Err) else math.expm1(a)


def _sqrt(a):
    return a._r(a.v ** 0.5, 0.5 * a.e / a.v ** 0.5, 2) if isinstance(a, Err) else a ** 0.5


def _solve(R, b):
    """rho = R^-1 b; over Err entries the bound of the module docstring."""
    Rv, bv = np.array([[_val(x) for x in row] for row in R]), np.array([_val(x) for x in b])
    rho = np.linalg.solve(Rv, bv)
    if not any(isinstance(x, Err) for row in R for x in row) and not any(isinstance(x, Err) for x in b):
        return [float(v) for v in rho]
    n = len(b)
    ER, Eb = np.array([[_err(x) for x in row] for row in R]), np.array([_err(x) for x in b])
    backward = n * n * 3 * n * U_F32 * 2 ** (n - 1) * np.abs(Rv).sum(axis=1).max()
    d = np.abs(np.linalg.inv(Rv)) @ ((ER + backward) @ np.abs(rho) + Eb)
    return [Err(v, e) for v, e in zip(rho, d)]


def _lambda(s):
    """(alpha, sg, lambda) of the sigma-table entry s (> 0)."""
    alpha = 1.0 / _sqrt(s * s + 1.0)
    sg = s * alpha
    return alpha, sg, _log(alpha) - _log(sg)


def _rb(h, rks, solver_type):
    hh = -h
    phi_1 = _expm1(hh)
    B_h = hh if solver_type == "bh1" else _expm1(hh)
    h_phi_k = phi_1 / hh - 1.0
    f = 1
    R, b = [], []
    for j in range(1, len(rks) + 1):
        R.append([1.0 if j == 1 else r if j == 2 else r * r for r in rks])
        b.append(h_phi_k * float(f) / B_h)
        f *= j + 1
        c = 1.0 / f  # a Python float in the product, rounded to float32 where it meets the tensor: 1 / 6 is not exact there
        h_phi_k = h_phi_k / hh - (Err(c, U_F32 * c) if isinstance(h, Err) else c)
    return R, b, phi_1, B_h


def scalars(sig, i, p, q, solver_type="bh2", with_err=False):
    """The scalars of step i with corrector order p (0: off) and predictor order q from the sigma table ``sig`` (floats: the float32
    table values, exactly).  Fields: sigma_s, alpha_s; c_x, c_m, c_b, c_rho [p], c_r [p - 1]; p_x, p_m, p_b, p_rho [q - 1], p_r [q - 1];
    floats, or ``Err`` numbers with ``with_err``."""
    num = (lambda v: Err(v)) if with_err else float
    lam = lambda k: _lambda(num(sig[k]))
    sc = SimpleNamespace(p=p, q=q, c_rho=[], c_r=[], p_rho=[], p_r=[], c_x=None, c_m=None, c_b=None)
    alpha_s, sg_s, lambda_s = lam(i)
    sc.sigma_s, sc.alpha_s = sg_s, alpha_s
    if p:
        _, sg_p, lambda_p = lam(i - 1)
        h = lambda_s - lambda_p
        sc.c_r = [(lam(i - 1 - k)[2] - lambda_p) / h for k in range(1, p)]
        R, b, phi_1, B_h = _rb(h, sc.c_r + [num(1.0)], solver_type)
        sc.c_rho = [num(0.5)] if p == 1 else _solve(R, b)
        sc.c_x, sc.c_m, sc.c_b = sg_s / sg_p, alpha_s * phi_1, alpha_s * B_h
    if float(sig[i + 1]) == 0.0:  # exact in float32 as in float64 (module docstring)
        assert q == 1, "a step that ends at sigma 0 has h = +inf: only first order is finite"
        sc.p_x, sc.p_m, sc.p_b = num(0.0), num(-1.0), None
        return sc
    alpha_t, sg_t, lambda_t = lam(i + 1)
    h = lambda_t - lambda_s
    sc.p_r = [(lam(i - k)[2] - lambda_s) / h for k in range(1, q)]
    R, b, phi_1, B_h = _rb(h, sc.p_r + [num(1.0)], solver_type)
    sc.p_rho = [] if q == 1 else [num(0.5)] if q == 2 else _solve([row[:-1] for row in R[:-1]], b[:-1])
    sc.p_x, sc.p_m, sc.p_b = sg_t / sg_s, alpha_t * phi_1, alpha_t * B_h
    return sc


# ---------------------------------------------------------------------------------------------------------------------------
# steps
# ---------------------------------------------------------------------------------------------------------------------------
def step64(eps, x, sc, last=None, hist=()):
    """(prev, xc, x0, mags) in float64.  ``sc``: ``scalars`` (floats or Err: the values are used); ``hist``: the x0 predictions of the
    previous steps, newest first; ``last``: the corrected sample of the previous step.  mags: the magnitudes ``bounds`` needs."""
    v = lambda a: _val(a)
    e, s = eps.to(F64), x.to(F64)
    h = [t.to(F64) for t in hist]
    x0 = (s - v(sc.sigma_s) * e) / v(sc.alpha_s)
    m = SimpleNamespace(eps=e.abs(), A0=(s.abs() + v(sc.sigma_s) * e.abs()) / v(sc.alpha_s), AD=[], ADq=[], S=0.0, Sq=0.0)
    xc, m.Ac = s, s.abs()
    if sc.p:
        acc = 0.0
        for k in range(1, sc.p):
            acc = acc + v(sc.c_rho[k - 1]) * ((h[k] - h[0]) / v(sc.c_r[k - 1]))
            m.AD.append((h[k].abs() + h[0].abs()) / abs(v(sc.c_r[k - 1])))
        acc = acc + v(sc.c_rho[sc.p - 1]) * (x0 - h[0])
        m.AD.append(m.A0 + h[0].abs())
        m.S = sum(abs(v(r)) * a for r, a in zip(sc.c_rho, m.AD))
        m.last, m.h1 = last.to(F64).abs(), h[0].abs()
        xc = v(sc.c_x) * last.to(F64) - v(sc.c_m) * h[0] - v(sc.c_b) * acc
        m.Ac = abs(v(sc.c_x)) * m.last + abs(v(sc.c_m)) * m.h1 + abs(v(sc.c_b)) * m.S
    prev = v(sc.p_x) * xc - v(sc.p_m) * x0
    m.Ap = abs(v(sc.p_x)) * m.Ac + abs(v(sc.p_m)) * m.A0
    if sc.q > 1:
        acc = 0.0
        for k in range(1, sc.q):
            acc = acc + v(sc.p_rho[k - 1]) * ((h[k - 1] - x0) / v(sc.p_r[k - 1]))
            m.ADq.append((h[k - 1].abs() + m.A0) / abs(v(sc.p_r[k - 1])))
        m.Sq = sum(abs(v(r)) * a for r, a in zip(sc.p_rho, m.ADq))
        prev = prev - v(sc.p_b) * acc
        m.Ap = m.Ap + abs(v(sc.p_b)) * m.Sq
    return prev, xc, x0, m


def bounds(m, sc, extra=0):
    """(bound of prev, of xc, of x0) per element: ROUNDINGS u A plus the scalars' own error (module docstring).  ``sc``: ``scalars`` with
    ``with_err=True``; ``extra``: roundings added on every path (inputs that are themselves roundings of the quantities compared)."""
    v, d = _val, _err
    e_x0 = (d(sc.sigma_s) * m.eps + m.A0 * d(sc.alpha_s)) / v(sc.alpha_s)
    e_xc = 0.0
    if sc.p:
        e_acc = d(sc.c_rho[-1]) * m.AD[-1] + abs(v(sc.c_rho[-1])) * e_x0
        for rho, r, ad in zip(sc.c_rho, sc.c_r, m.AD):
            e_acc = e_acc + d(rho) * ad + abs(v(rho)) * ad * d(r) / abs(v(r))
        e_xc = d(sc.c_x) * m.last + d(sc.c_m) * m.h1 + d(sc.c_b) * m.S + abs(v(sc.c_b)) * e_acc
    e_prev = d(sc.p_x) * m.Ac + abs(v(sc.p_x)) * e_xc + d(sc.p_m) * m.A0 + abs(v(sc.p_m)) * e_x0
    if sc.q > 1:
        e_acc = 0.0
        for rho, r, ad in zip(sc.p_rho, sc.p_r, m.ADq):
            e_acc = e_acc + d(rho) * ad + abs(v(rho)) * (ad * d(r) + e_x0) / abs(v(r))
        e_prev = e_prev + d(sc.p_b) * m.Sq + abs(v(sc.p_b)) * e_acc
    return ((ROUNDINGS + extra) * U_F32 * m.Ap + e_prev, (ROUNDINGS_XC + extra) * U_F32 * m.Ac + e_xc,
            (ROUNDINGS_X0 + extra) * U_F32 * m.A0 + e_x0)


def _s(v):
    return torch.tensor(float(v), dtype=F32)  # a scalar the kernel receives as ``float``


def unipc_step_f32(eps, x, p, q, coefs, last=None, hist=()):
    """(m0, x_corr, x_prev, x0) of gmd_unipc_step given the guided eps, as float32 torch expressions in the kernel's order; ``coefs``:
    the launcher's 19 floats (a NaN beyond the orders in use is never touched).  Independent of the scheduler class."""
    (sg, al, c_x, c_m, c_b, cr1, cr2, cr3, cq1, cq2, p_x, p_m, p_b, pr1, pr2, pq1, pq2, sa, s1) = (_s(c) for c in coefs)
    x0 = (x - s1 * eps) / sa
    m0 = (x - sg * eps) / al
    xc = x.clone()
    if p >= 1:
        h1 = hist[0]
        if p == 1:
            acc = cr1 * (m0 - h1)
        else:
            acc = cr1 * ((hist[1] - h1) / cq1)
            if p == 3:
                acc = acc + cr2 * ((hist[2] - h1) / cq2)
            acc = acc + (cr3 if p == 3 else cr2) * (m0 - h1)
        xc = c_x * last - c_m * h1 - c_b * acc
    r = p_x * xc - p_m * m0
    if q >= 2:
        acc = pr1 * ((hist[0] - m0) / pq1)
        if q == 3:
            acc = acc + pr2 * ((hist[1] - m0) / pq2)
        r = r - p_b * acc
    return m0, xc, r, x0


# ---------------------------------------------------------------------------------------------------------------------------
# the whole scheduler in float64
# ---------------------------------------------------------------------------------------------------------------------------
class RefUniPCScheduler:
    """UniPC in float64 with the scheduler protocol of oracle/pipelines.py: tables via ``tables64`` (rounded to float32 once, as the
    product's are), order rule, history and corrector state.  The step is selected by a counter."""

    order = 1
    init_noise_sigma = 1.0

    def __init__(self, solver_order=2, solver_type="bh2", lower_order_final=True, disable_corrector=(), timestep_spacing="linspace",
                 steps_offset=0, final_sigmas_type="zero", beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear"):
        self.config = SimpleNamespace(solver_order=solver_order, solver_type=solver_type, lower_order_final=lower_order_final,
                                      disable_corrector=tuple(disable_corrector), timestep_spacing=timestep_spacing,
                                      steps_offset=steps_offset, final_sigmas_type=final_sigmas_type, num_train_timesteps=1000)
        self.alphas_cumprod = E.alphas_cumprod(beta_start, beta_end, beta_schedule)
        self.timesteps = None

    def set_timesteps(self, num_inference_steps, device=None):
        c = self.config
        ts, sig = tables64(self.alphas_cumprod, num_inference_steps, c.timestep_spacing, c.steps_offset, c.final_sigmas_type)
        self.sigmas = [float(v) for v in sig.astype(np.float32)]
        self.timesteps = torch.from_numpy(ts)
        self.num_inference_steps = len(ts)
        self.index, self.hist, self.last, self.prev_order = 0, [], None, None

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        c, i = self.config, self.index
        assert int(timestep) == int(self.timesteps[i])
        p, q = orders(i, self.num_inference_steps, c.solver_order, c.lower_order_final, c.disable_corrector, self.prev_order)
        sc = scalars(self.sigmas, i, p, q, c.solver_type)
        prev, xc, x0, _ = step64(model_output, sample, sc, self.last, self.hist)
        self.hist = ([x0] + self.hist)[:c.solver_order]
        self.last, self.prev_order = xc, q
        self.index += 1
        prev = prev.to(model_output.dtype)
        return (prev,) if not return_dict else SimpleNamespace(prev_sample=prev)
