"""CPU: components.DPMSolverMultistepScheduler with the SDE algorithm ("DPM++ 2M SDE") and the heun solver type -- coefficient identities
that pin the formulas without diffusers, the known answer of an x0-consistent model, the host step against the float64 restatement
(tests/dpm_sde_ref.py; per element, allowed violations: 0), generator accounting, the pipelines' pre-draw, deepcopy in mid-trajectory, the
config protocol and the argument validation of gmd_dpm_sde_step.  No GPU is touched."""
import copy
import inspect

import pytest
import torch

import dpm_sde_ref as D
import parity as P

SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SHAPE = (3, 4, 8, 8)
U = D.U_F32
VARIANTS = [(a, s) for a in (D.ODE, D.SDE) for s in ("midpoint", "heun")]


def dpm(**kw):
    from gm_diffusion.components import DPMSolverMultistepScheduler

    return DPMSolverMultistepScheduler(**SD, **kw)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _first(s, i):
    """The order rule, restated: the first step, solver_order 1 and the lower-order final step are first order."""
    c, n = s.config, s.num_inference_steps
    lower_final = i == n - 1 and (c.euler_at_final or (c.lower_order_final and n < 15) or c.final_sigmas_type == "zero")
    return c.solver_order == 1 or i == 0 or lower_final


# ---------------------------------------------------------------------------------------------------------------------------
# coefficient identities
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,final", [(8, "zero"), (16, "sigma_min"), (25, "zero")])
@pytest.mark.parametrize("spacing", ["leading", "linspace", "trailing"])
def test_coefficient_identities(spacing, n, final):
    """With e^-h = (sigma_t / alpha_t) (alpha_s0 / sigma_s0):
        sde:  c_x alpha_s0 + c_m = alpha_t        (the x0 part of the marginal mean is carried over)
              c_x^2 sigma_s0^2 + c_n^2 = sigma_t^2   (the noise part of the marginal variance is carried over)
        ode:  c_x alpha_s0 - c_m = alpha_t
    evaluated in float64 on the product's float32 coefficients.  Allowances from the counts of tests/dpm_sde_ref.py (u = 2^-24; Lam, G, Gd
    as defined there), each term's roundings times its magnitude, the largest count taken for all terms of an identity:
        (1) c_x alpha_s0: 32 + 4 on c_x alpha_s0 Lam;  c_m: 44 on alpha_t G;  alpha_t: 4     ->  44 u (c_x alpha_s0 Lam + alpha_t G + alpha_t)
        (2) c_x^2 sigma_s0^2: 2 * 32 + 2 * 5 = 74 on c_x^2 sigma_s0^2 Lam;  c_n^2: 2 c_n |err c_n| = 54 on sigma_t^2 G;  sigma_t^2: 10
                                                                                    ->  74 u (c_x^2 sigma_s0^2 Lam + sigma_t^2 G + sigma_t^2)
        (3) c_x alpha_s0: 11 + 4;  c_m: 26 on alpha_t Gd;  alpha_t: 4                        ->  26 u (c_x alpha_s0 + alpha_t Gd + alpha_t)"""
    worst = [0.0, 0.0, 0.0]
    for alg in (D.SDE, D.ODE):
        s = dpm(algorithm_type=alg, timestep_spacing=spacing, final_sigmas_type=final)
        s.set_timesteps(n)
        for i, t in enumerate(s.timesteps.tolist()):
            s._step_index = i
            s.lower_order_nums = min(i, 2)
            first, a0, g0, at, gt, h, r0 = s._plan_step(t)
            c_x, c_m, c_h, c_n = (None if v is None else float(v) for v in s._update_coefs(first, at, gt, g0, h))
            a0, g0, at, gt = float(a0), float(g0), float(at), float(gt)
            sc = D.scalars64(float(s.sigmas[i]), float(s.sigmas[i + 1]))
            if alg == D.SDE:
                G = 1.0 + sc.E2 * sc.Lam
                tol1 = 44 * U * (c_x * a0 * sc.Lam + at * G + at)
                tol2 = 74 * U * (c_x ** 2 * g0 ** 2 * sc.Lam + gt ** 2 * G + gt ** 2)
                e1, e2 = abs(c_x * a0 + c_m - at), abs(c_x ** 2 * g0 ** 2 + c_n ** 2 - gt ** 2)
                assert e1 <= tol1, (spacing, n, i, e1, tol1)
                assert e2 <= tol2, (spacing, n, i, e2, tol2)
                assert c_n >= 0.0
                worst[0], worst[1] = max(worst[0], e1 / tol1), max(worst[1], e2 / tol2 if tol2 else 0.0)
            else:
                Gd = 1.0 + sc.E * sc.Lam
                tol3 = 26 * U * (c_x * a0 + at * Gd + at)
                e3 = abs(c_x * a0 - c_m - at)
                assert e3 <= tol3, (spacing, n, i, e3, tol3)
                assert c_n is None
                worst[2] = max(worst[2], e3 / tol3)
        if final == "zero":  # the last step: h = +inf gives c_x = 0, |c_m| = 1, c_n = 0 and no NaN
            assert float(h) == float("inf") and c_x == 0.0 and abs(c_m) == 1.0 and first
    print(f"{spacing} n={n} {final}: max |err| / allowance = {worst[0]:.3f} {worst[1]:.3f} {worst[2]:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------
# known answer
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise_from", ["zeros", "generator"])
@pytest.mark.parametrize("alg,solver", VARIANTS)
def test_x0_consistent_model_ends_on_x0(alg, solver, noise_from):
    """With eps = (x - alpha x0) / sigma and final_sigmas_type="zero" every variant ends on x0, whatever noise the SDE steps added on
    the way (atol of test_dpm_solver_pp_known_answer_and_oracle_agreement)."""
    for n in (20, 8):
        s = dpm(algorithm_type=alg, solver_type=solver, steps_offset=1, timestep_spacing="leading")
        s.set_timesteps(n)
        x0 = torch.full((1, 4, 2, 2), 0.6)
        a0, s0 = s._sigma_to_alpha_sigma_t(s.sigmas[0])
        x = a0 * x0 + s0 * torch.full((1, 4, 2, 2), -0.9)
        g = gen(3)
        for i, t in enumerate(s.timesteps):
            a, s_ = s._sigma_to_alpha_sigma_t(s.sigmas[i])
            eps = (x - a * x0) / s_
            kw = dict(variance_noise=torch.zeros_like(x)) if noise_from == "zeros" else dict(generator=g)
            x = s.step(eps, t, x, return_dict=False, **kw)[0]
            assert bool(torch.isfinite(x).all())
        assert torch.allclose(x, x0, atol=1e-4), float((x - x0).abs().max())


# ---------------------------------------------------------------------------------------------------------------------------
# the host step against the float64 function
# ---------------------------------------------------------------------------------------------------------------------------
def _trajectory_within_bound(s, n, alg, solver, what):
    s.set_timesteps(n)
    g = gen(11)
    x = torch.randn(SHAPE, generator=g)
    worst, orders = 0.0, []
    for i, t in enumerate(s.timesteps.tolist()):
        eps, noise = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
        first = _first(s, i)
        orders.append(1 if first else 2)
        m1 = s.model_outputs[-1]
        ref, m0_ref, a, a_m0 = D.dpm_step64(eps, x, m1, noise, float(s.sigmas[i]), float(s.sigmas[i + 1]),
                                            None if first else float(s.sigmas[i - 1]), alg, solver)
        out = s.step(eps, t, x, variance_noise=noise if alg == D.SDE else None).prev_sample
        assert out.dtype == torch.float32
        worst = max(worst, P.assert_elementwise(out, ref, D.bound(a), f"{what}: host step prev_sample i={i} t={t}"))
        P.assert_elementwise(s.model_outputs[-1], m0_ref, D.bound(a_m0), f"{what}: x0 prediction i={i} t={t}")
        x = out
    print(f"{what}: orders {orders}, max |err| / bound = {worst:.3f}")
    return orders


@pytest.mark.parametrize("spacing", ["leading", "linspace", "trailing"])
@pytest.mark.parametrize("alg,solver", VARIANTS)
def test_host_step_within_bound_of_float64(alg, solver, spacing):
    """Whole trajectories, unit-normal inputs, |host step - float64| <= 81 2^-24 A per element at every step:
    n = 8 (below 15: lower-order final step, h = +inf) and n = 16 with final_sigmas_type="sigma_min" (second order on the last step)."""
    s = dpm(algorithm_type=alg, solver_type=solver, timestep_spacing=spacing)
    assert _trajectory_within_bound(s, 8, alg, solver, f"{alg} {solver} {spacing} n=8") == [1] + [2] * 6 + [1]
    s = dpm(algorithm_type=alg, solver_type=solver, timestep_spacing=spacing, final_sigmas_type="sigma_min")
    assert _trajectory_within_bound(s, 16, alg, solver, f"{alg} {solver} {spacing} n=16 sigma_min") == [1] + [2] * 15


@pytest.mark.parametrize("alg,solver", VARIANTS)
def test_host_step_within_bound_order_one_and_euler_at_final(alg, solver):
    s = dpm(algorithm_type=alg, solver_type=solver, solver_order=1, timestep_spacing="leading", steps_offset=1)
    assert _trajectory_within_bound(s, 8, alg, solver, f"{alg} {solver} solver_order=1") == [1] * 8
    s = dpm(algorithm_type=alg, solver_type=solver, euler_at_final=True, final_sigmas_type="sigma_min", timestep_spacing="leading",
            steps_offset=1)
    assert _trajectory_within_bound(s, 16, alg, solver, f"{alg} {solver} euler_at_final") == [1] + [2] * 14 + [1]


def test_defaults_unchanged_bit_for_bit():
    """The default configuration (dpmsolver++ / midpoint) still evaluates the expressions it evaluated before, written out here."""
    s = dpm(steps_offset=1, timestep_spacing="leading")
    s.set_timesteps(9)
    g = gen(2)
    x = torch.randn(SHAPE, generator=g)
    m1 = None
    for i, t in enumerate(s.timesteps.tolist()):
        eps = torch.randn(SHAPE, generator=g)
        a0, g0 = s._sigma_to_alpha_sigma_t(s.sigmas[i])
        at, gt = s._sigma_to_alpha_sigma_t(s.sigmas[i + 1])
        h = (torch.log(at) - torch.log(gt)) - (torch.log(a0) - torch.log(g0))
        m0 = (x - g0 * eps) / a0
        if _first(s, i):
            want = (gt / g0) * x - (at * (torch.exp(-h) - 1.0)) * m0
        else:
            a1, g1 = s._sigma_to_alpha_sigma_t(s.sigmas[i - 1])
            r0 = ((torch.log(a0) - torch.log(g0)) - (torch.log(a1) - torch.log(g1))) / h
            want = (gt / g0) * x - (at * (torch.exp(-h) - 1.0)) * m0 - 0.5 * (at * (torch.exp(-h) - 1.0)) * ((1.0 / r0) * (m0 - m1))
        x = s.step(eps, t, x, generator=g).prev_sample
        assert torch.equal(x, want), i
        m1 = m0


# ---------------------------------------------------------------------------------------------------------------------------
# generator accounting
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg,solver", VARIANTS)
def test_generator_is_advanced_once_per_step_iff_sde(alg, solver):
    n = 7
    s = dpm(algorithm_type=alg, solver_type=solver)
    s.set_timesteps(n)
    g, twin = gen(9), gen(9)
    x = torch.randn(SHAPE, generator=gen(1))
    for t in s.timesteps.tolist():
        assert s.draws_noise(t) == (alg == D.SDE)
        x = s.step(torch.randn(SHAPE, generator=gen(100 + t)), t, x, generator=g).prev_sample
    for _ in range(n if alg == D.SDE else 0):  # n float32 tensors of the sample's shape: the last step (c_n == 0) draws too
        torch.randn(SHAPE, generator=twin, dtype=torch.float32)
    assert torch.equal(g.get_state(), twin.get_state())


@pytest.mark.parametrize("name", ["variance_noise", "noise"])
def test_given_noise_is_used_and_leaves_the_generator_alone(name):
    s = dpm(algorithm_type=D.SDE)
    s.set_timesteps(6)
    a, b = copy.deepcopy(s), copy.deepcopy(s)
    g = gen(4)
    before = g.get_state()
    x = torch.randn(SHAPE, generator=gen(1))
    for t in s.timesteps.tolist():
        eps, z = torch.randn(SHAPE, generator=gen(100 + t)), torch.randn(SHAPE, generator=gen(200 + t))
        got = a.step(eps, t, x, generator=g, **{name: z}).prev_sample
        want = b.step(eps, t, x, generator=gen(200 + t)).prev_sample  # the draw the generator would have given
        assert torch.equal(got, want)
        x = got
    assert torch.equal(g.get_state(), before)
    assert "noise" in inspect.signature(s.fused_step).parameters and "eta" not in inspect.signature(s.step).parameters


def test_sixteen_bit_host_path_keeps_the_dtype_and_draws_float32():
    s = dpm(algorithm_type=D.SDE, solver_type="heun")
    s.set_timesteps(5)
    g, twin = gen(6), gen(6)
    x = torch.randn(SHAPE, generator=gen(1)).to(torch.bfloat16)
    for t in s.timesteps.tolist():
        x = s.step(torch.randn(SHAPE, generator=gen(t)).to(torch.bfloat16), t, x, generator=g).prev_sample
        assert x.dtype == torch.bfloat16
    for _ in range(5):
        torch.randn(SHAPE, generator=twin, dtype=torch.float32)
    assert torch.equal(g.get_state(), twin.get_state())


# ---------------------------------------------------------------------------------------------------------------------------
# the pipelines' pre-draw
# ---------------------------------------------------------------------------------------------------------------------------
def test_predrawn_noise_slots_cover_every_step_sdr_before_gm():
    from gm_diffusion.components.image_processor import randn_tensor
    from gm_diffusion.pipelines import StableDiffusionGMPipeline as Pipe

    n = 4
    s1 = dpm(algorithm_type=D.SDE)
    s1.set_timesteps(n)
    s2 = copy.deepcopy(s1)
    ts = [int(t) for t in s1.timesteps]
    shape = (2, 4, 8, 8)
    g0 = gen(5)
    pre = Pipe._predraw_step_noise([s1, s2], ts, shape, g0, "cpu")
    g = gen(5)
    for i in range(n):
        for k in range(2):
            assert torch.equal(pre[k][i], randn_tensor(shape, generator=g, device="cpu", dtype=torch.float32)), (i, k)
    assert torch.equal(g0.get_state(), g.get_state())  # advanced by 2 n draws
    assert Pipe._predraw_step_noise([s1, s2], ts, shape, None, "cpu") is None  # no generator: the steps draw for themselves
    d1 = dpm(solver_type="heun")
    d1.set_timesteps(n)
    g1 = gen(5)
    assert Pipe._predraw_step_noise([d1, copy.deepcopy(d1)], ts, shape, g1, "cpu") is None  # deterministic pair
    assert Pipe._predraw_step_noise([s1, d1], ts, shape, g1, "cpu") is None
    assert torch.equal(g1.get_state(), gen(5).get_state())
    old = Pipe.PREDRAW_NOISE_BYTES
    try:
        Pipe.PREDRAW_NOISE_BYTES = 4 * 2 * 4 * 8 * 8 * 3  # room for three draws only
        assert Pipe._predraw_step_noise([s1, s2], ts, shape, g1, "cpu") is None
    finally:
        Pipe.PREDRAW_NOISE_BYTES = old
    assert torch.equal(g1.get_state(), gen(5).get_state())


def test_pipeline_step_kwargs_for_the_sde_scheduler():
    from gm_diffusion.pipelines import StableDiffusionGMPipeline as Pipe

    g = gen(0)
    pipe = Pipe.__new__(Pipe)
    pipe.scheduler = dpm(algorithm_type=D.SDE)
    kw = pipe.prepare_extra_step_kwargs(g, 0.7)  # eta has nowhere to go: the algorithm type is the dial
    assert kw == {"generator": g} and Pipe._fused_step_kwargs(kw) == {"generator": g}


# ---------------------------------------------------------------------------------------------------------------------------
# deep copy, config protocol
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg,solver", VARIANTS)
def test_deepcopy_in_mid_trajectory_continues_bit_identically(alg, solver):
    s = dpm(algorithm_type=alg, solver_type=solver, steps_offset=1, timestep_spacing="leading")
    s.set_timesteps(8)
    g = gen(2)
    x = torch.randn(SHAPE, generator=g)
    c = xc = None
    for i, t in enumerate(s.timesteps.tolist()):
        if i == 3:
            c, xc = copy.deepcopy(s), x.clone()
        eps = torch.randn(SHAPE, generator=g)
        x = s.step(eps, t, x, generator=gen(50 + t)).prev_sample
        if c is not None:
            xc = c.step(eps, t, xc, generator=gen(50 + t)).prev_sample
            assert torch.equal(x, xc), i
    assert c.step_index == s.step_index == 8 and c.model_outputs[-1] is not s.model_outputs[-1]


def test_from_config_round_trip_keeps_the_algorithm_override():
    from gm_diffusion.components import DDPMScheduler, DPMSolverMultistepScheduler

    ddpm = DDPMScheduler(steps_offset=1, clip_sample=False, **SD)
    p = DPMSolverMultistepScheduler.from_config(ddpm.config, algorithm_type="sde-dpmsolver++")
    assert p.config.algorithm_type == "sde-dpmsolver++" and p.config.solver_type == "midpoint" and p.draws_noise(0)
    assert p.config.timestep_spacing == "leading" and p.config.steps_offset == 1 and p.config.beta_schedule == "scaled_linear"
    q = DPMSolverMultistepScheduler.from_config(p.config, solver_type="heun", euler_at_final=True)
    assert q.config.algorithm_type == "sde-dpmsolver++" and q.config.solver_type == "heun" and q.config.euler_at_final is True
    back = DDPMScheduler.from_config(q.config)
    assert back.config.steps_offset == 1 and "algorithm_type" not in back.config
    assert not DPMSolverMultistepScheduler.from_config(ddpm.config).draws_noise(0)


# ---------------------------------------------------------------------------------------------------------------------------
# ABI without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_dpm_sde_step_argument_validation_without_gpu():
    from gm_diffusion import _native as native

    lib = native.lib()
    assert hasattr(lib, "gmd_dpm_sde_step") and "gmd_dpm_sde_step" in native.SIGNATURES
    assert lib.gmd_abi_version() == 14 and native.ABI_VERSION == 14  # added within v14
    one = 1  # any non-null address: validation happens before a launch, nothing is dereferenced
    nan = float("nan")

    def call(eps=one, x=one, m1=None, noise=one, B=1, chw=16, order=1, g0=0.43, a0=0.9, c_x=0.8, c_m=0.3, c_h=0.1, inv_r0=1.0, c_n=0.2,
             sa=0.9, s1=0.43, m0=one, xp=one, x0=None):
        return lib.gmd_dpm_sde_step(eps, x, m1, noise, B, chw, 0, 1.0, None, 0.0, order, g0, a0, c_x, c_m, c_h, inv_r0, c_n, sa, s1, m0, xp,
                                    x0, None)

    for kw, word in ((dict(eps=None), b"null"), (dict(x=None), b"null"), (dict(m0=None), b"null"), (dict(xp=None), b"null"),
                     (dict(noise=None), b"noise"), (dict(order=2), b"previous"), (dict(B=-1), b"shape"), (dict(chw=0), b"shape"),
                     (dict(chw=-3), b"shape"), (dict(order=0), b"order"), (dict(order=3), b"order"), (dict(a0=0.0), b"zero"),
                     (dict(x0=one, sa=0.0), b"zero"), (dict(c_n=-0.1), b"c_n"), (dict(c_n=nan), b"c_n")):
        assert call(**kw) == 1, kw  # GMD_ERR_INVALID
        assert word in lib.gmd_last_error(), (kw, lib.gmd_last_error())
    assert call(B=0, eps=None, x=None, noise=None, m0=None, xp=None) == 0  # an empty batch is a no-op


def test_dpm_sde_step_refuses_host_tensors():
    from gm_diffusion import hip_ops
    from gm_diffusion._native import HipExtensionError

    assert "dpm_sde_step" in hip_ops.__all__
    z = torch.zeros(1, 4, 8, 8)
    with pytest.raises(HipExtensionError):
        hip_ops.dpm_sde_step(z, z, 1, (0.43, 0.9, 0.8, 0.3, 0.0, 0.0, 0.2, 0.9, 0.43), False, 1.0, z)
