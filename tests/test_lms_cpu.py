"""CPU: components.LMSDiscreteScheduler -- the multistep coefficients against exact rational arithmetic (tests/lms_ref.py), identities
that tie it to code written earlier (the coefficients sum to dt, order 1 is the Euler scheduler, polynomial derivatives are integrated
exactly, the perfect predictor), the host step per element against float64 (allowed violations: 0), history and order handling, the config
and pipeline protocol, and the argument validation of gmd_lms_step.  No GPU is touched."""
import copy

import pytest
import torch

import lms_ref as L
import parity as P

SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SHAPE = (2, 4, 9, 7)
SPACINGS = ("linspace", "leading", "trailing")
NS = (1, 2, 3, 4, 5, 8, 20, 50)


def lms(**kw):
    from gm_diffusion.components import LMSDiscreteScheduler

    return LMSDiscreteScheduler(**kw)


def euler(**kw):
    from gm_diffusion.components import EulerDiscreteScheduler

    return EulerDiscreteScheduler(**kw)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def sig(s):
    """The schedule's float32 sigmas as Python floats (exact)."""
    return [float(v) for v in s.sigmas]


# ---------------------------------------------------------------------------------------------------------------------------
# coefficients
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("spacing", SPACINGS)
def test_coefficients_against_exact_rational(spacing, karras):
    """Every step, every order reached, every coefficient: within 2^-48 sum_j |c_j| of the integral in exact rational arithmetic over the
    same float32 sigmas; and their sum is sigma_next - sigma within the same bound (the basis polynomials sum to 1)."""
    worst, worst_ratio = 0.0, 0.0
    for n in NS:
        s = lms(timestep_spacing=spacing, use_karras_sigmas=karras, **SD)
        s.set_timesteps(n)
        sg = sig(s)
        for t in range(n):
            for order in range(1, min(t + 1, 4) + 1):
                exact = L.coefs_exact(sg, order, t)
                got = [s.get_lms_coefficient(order, t, j) for j in range(order)]
                assert all(type(c) is float for c in got)
                tot = float(sum(abs(c) for c in exact))
                tol = L.COEF_TOL * tot
                for j in range(order):
                    err = abs(float(got[j] - exact[j]))  # float - Fraction is exact up to the final rounding
                    worst = max(worst, err / tot)
                    assert err <= tol, f"{spacing} karras={karras} n={n} t={t} order={order} j={j}: {err:.3e} > {tol:.3e}"
                dt = sg[t + 1] - sg[t]
                assert abs(sum(got) - dt) <= tol, f"{spacing} karras={karras} n={n} t={t} order={order}: sum != dt"
                assert sum(exact) == L.Fraction(sg[t + 1]) - L.Fraction(sg[t])
                worst_ratio = max(worst_ratio, tot / abs(dt))
    print(f"{spacing} karras={karras}: worst |c - exact| / sum|c| = {worst:.2e}; worst sum|c| / |dt| = {worst_ratio:.1f}")


@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("spacing", SPACINGS)
def test_coefficients_within_quad_tolerance_of_diffusers(spacing, karras):
    """diffusers integrates with scipy's quad at epsrel = 1e-4: every coefficient (every step, every order reached) is within that tolerance
    of quad on the float64 nodes."""
    integrate = pytest.importorskip("scipy.integrate")
    for n in NS:
        s = lms(timestep_spacing=spacing, use_karras_sigmas=karras, **SD)
        s.set_timesteps(n)
        sg = sig(s)
        for t in range(n):
            for order in range(1, min(t + 1, 4) + 1):
                for j in range(order):
                    def f(tau):
                        prod = 1.0
                        for k in range(order):
                            if k != j:
                                prod *= (tau - sg[t - k]) / (sg[t - j] - sg[t - k])
                        return prod

                    ref = integrate.quad(f, sg[t], sg[t + 1], epsrel=1e-4)[0]
                    got = s.get_lms_coefficient(order, t, j)
                    assert abs(got - ref) <= 1e-4 * abs(ref), (spacing, karras, n, t, order, j, got, ref)


def test_get_lms_coefficient_refuses_what_the_schedule_cannot_give():
    s = lms(**SD)
    s.set_timesteps(5)
    for order, t, j in ((3, 1, 0), (2, 1, 2), (2, 1, -1)):
        with pytest.raises(ValueError):
            s.get_lms_coefficient(order, t, j)


# ---------------------------------------------------------------------------------------------------------------------------
# identities
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("spacing", SPACINGS)
def test_order_1_trajectory_is_the_euler_scheduler(spacing, karras):
    """A whole host trajectory at order = 1 equals EulerDiscreteScheduler's by value (the sign of a zero may differ: 0 + c0 d), and the
    order-1 coefficient rounded to float32 is Euler's float32 dt bit for bit."""
    for n in (1, 2, 7, 20):
        kw = dict(timestep_spacing=spacing, use_karras_sigmas=karras, **SD)
        a, b = lms(**kw), euler(**kw)
        a.set_timesteps(n)
        b.set_timesteps(n)
        assert torch.equal(a.timesteps, b.timesteps) and torch.equal(a.sigmas, b.sigmas) and float(a.init_noise_sigma) == float(b.init_noise_sigma)
        g = gen(4)
        x = torch.randn(SHAPE, generator=g) * a.init_noise_sigma
        xa = xb = x
        for i, t in enumerate(a.timesteps.tolist()):
            eps = torch.randn(SHAPE, generator=g)
            c0 = a.get_lms_coefficient(1, i, 0)
            assert float(torch.tensor(c0, dtype=torch.float32)) == float(b.sigmas[i + 1] - b.sigmas[i])
            oa, ob = a._host_step(eps, t, xa, order=1), b._host_step(eps, t, xb)
            assert torch.equal(oa.prev_sample, ob.prev_sample), f"{spacing} karras={karras} n={n} step {i}"
            assert torch.equal(oa.pred_original_sample, ob.pred_original_sample)
            assert len(a.derivatives) == 1
            xa, xb = oa.prev_sample, ob.prev_sample


@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("spacing", SPACINGS)
def test_polynomial_derivatives_are_integrated_exactly(spacing, karras):
    """With k derivatives given (float32 samples of a per-element polynomial of degree k - 1 in sigma, a cubic at order 4), the order-k
    update is x + the exact integral over [sigma, sigma_next] of THE polynomial of degree k - 1 through those samples, within the
    per-element bound.  The integral is evaluated in Newton's divided-difference form, which shares nothing with the Lagrange basis."""
    s = lms(timestep_spacing=spacing, use_karras_sigmas=karras, **SD)
    n = 8
    s.set_timesteps(n)
    sg = sig(s)
    g = gen(6)
    a = [torch.randn(SHAPE, generator=g).double() / (sg[0] ** m) for m in range(4)]  # q(sigma) = sum_m a_m sigma^m, O(1) on the schedule
    x = torch.randn(SHAPE, generator=g)
    worst = 0.0
    for i, t in enumerate(s.timesteps.tolist()):
        k = min(i + 1, 4)
        q = lambda v: sum(a[m] * v ** m for m in range(k))
        s.derivatives = [q(sg[i - j]).float() for j in range(k - 1, 0, -1)]  # oldest first, as the scheduler keeps them
        eps = q(sg[i]).float()
        hist = list(reversed(s.derivatives))
        out = s._host_step(eps, t, x)
        integral = L.interpolant_integral64([sg[i - j] for j in range(k)], [eps] + hist, sg[i], sg[i + 1])
        cs = L.coefs64(sg, k, i)
        _, _, _, mags = L.step64(eps, x, sg[i], cs, hist)
        b = L.bound(mags, L.coef_err(cs))
        worst = max(worst, P.assert_elementwise(out.prev_sample, x.double() + integral, b, f"{spacing} karras={karras} step {i} order {k}"))
    print(f"{spacing} karras={karras}: max |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("spacing", SPACINGS)
def test_perfect_predictor_lands_on_x0_plus_sigma_next_eps(spacing, karras):
    """A perfect predictor (the model output is the constant e, and so is every earlier derivative): with x0 := x - sigma e taken from
    the float32 x in float64, every step lands on x0 + sigma_next e within the per-element bound, the last one on x0; x is carried
    along the trajectory."""
    s = lms(timestep_spacing=spacing, use_karras_sigmas=karras, **SD)
    s.set_timesteps(8)
    sg = sig(s)
    g = gen(3)
    e = torch.randn(SHAPE, generator=g)
    x = (torch.randn(SHAPE, generator=g).double() + sg[0] * e.double()).float()
    for i, t in enumerate(s.timesteps.tolist()):
        k = min(i + 1, 4)
        s.derivatives = [e.clone() for _ in range(k - 1)]
        x0 = x.double() - sg[i] * e.double()
        got = s.step(e, t, x).prev_sample
        cs = L.coefs64(sg, k, i)
        _, _, _, mags = L.step64(e, x, sg[i], cs, [e] * (k - 1))
        P.assert_elementwise(got, x0 + sg[i + 1] * e.double(), L.bound(mags, L.coef_err(cs)), f"{spacing} karras={karras} step {i} order {k}")
        x = got
    assert sg[-1] == 0.0 and k == 4


# ---------------------------------------------------------------------------------------------------------------------------
# the host step against the float64 function
# ---------------------------------------------------------------------------------------------------------------------------
def _plain_f32(eps, x, sigma, coefs, hist):
    """diffusers' expressions written out here (not the product class), with Python-float coefficients: what the bound is confirmed on."""
    sigma = torch.tensor(sigma, dtype=torch.float32)
    p0 = x - sigma * eps
    d = (x - p0) / sigma
    ds = [d] + list(hist)
    return x + sum(c * dj for c, dj in zip(coefs, ds)), p0, d


@pytest.mark.parametrize("n", [3, 8, 50])
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("spacing", SPACINGS)
def test_host_step_within_bound_of_float64(spacing, karras, n):
    """Whole trajectories on unit-normal model outputs: per element, |host step - float64 step on the same float32 history| <=
    9 2^-24 A + sum_j |D c_j| D_j for prev_sample, 2 2^-24 A_p0 for pred_original_sample and 4 2^-24 D0 for the kept derivative, after
    confirming that the plain float32 expressions sit inside the same bounds.  No element is excluded."""
    s = lms(timestep_spacing=spacing, use_karras_sigmas=karras, **SD)
    s.set_timesteps(n)
    sg = sig(s)
    g = gen(11)
    x = torch.randn(SHAPE, generator=g) * s.init_noise_sigma
    worst = 0.0
    for i, t in enumerate(s.timesteps.tolist()):
        eps = torch.randn(SHAPE, generator=g)
        k = min(i + 1, 4)
        hist = list(reversed(s.derivatives))[:k - 1]
        cs = L.coefs64(sg, k, i)
        ref, p0_ref, d_ref, mags = L.step64(eps, x, sg[i], cs, hist)
        b = L.bound(mags, L.coef_err(cs))
        plain, plain_p0, plain_d = _plain_f32(eps, x, sg[i], cs, hist)
        P.assert_elementwise(plain, ref, b, f"plain float32 expression step {i}")
        P.assert_elementwise(plain_p0, p0_ref, L.bound_p0(mags), f"plain float32 p0 step {i}")
        P.assert_elementwise(plain_d, d_ref, L.bound_d(mags), f"plain float32 derivative step {i}")
        out = s._host_step(eps, t, x)
        worst = max(worst, P.assert_elementwise(out.prev_sample, ref, b, f"host step prev_sample step {i}"))
        P.assert_elementwise(out.pred_original_sample, p0_ref, L.bound_p0(mags), f"host step pred_original_sample step {i}")
        P.assert_elementwise(s.derivatives[-1], d_ref, L.bound_d(mags), f"host step derivative step {i}")
        assert out.prev_sample.dtype == torch.float32 and out[0] is out.prev_sample and s.step_index == i + 1
        x = out.prev_sample
    assert sg[-1] == 0.0
    print(f"{spacing} karras={karras} n={n}: max |err| / bound = {worst:.3f}")


def test_lms_step_f32_is_the_host_step():
    """The test reference of the GPU file (float32 0-d tensor scalars, the kernel's order) against the product's host expressions
    (Python-float coefficients): bit-identical, zeros' signs included."""
    import small_ref as S

    s = lms(timestep_spacing="leading", use_karras_sigmas=True, **SD)
    s.set_timesteps(6)
    g = gen(2)
    x = torch.randn(SHAPE, generator=g)
    x.view(-1)[:4] = torch.tensor([0.0, -0.0, 0.0, -0.0])
    for i, t in enumerate(s.timesteps.tolist()):
        eps = torch.randn(SHAPE, generator=g)
        eps.view(-1)[:4] = torch.tensor([0.0, 0.0, -0.0, -0.0])
        k = min(i + 1, 4)
        hist = list(reversed(s.derivatives))[:k - 1]
        cs = [s.get_lms_coefficient(k, i, j) for j in range(k)]
        d, prev, p0 = L.lms_step_f32(eps, x, [float(s.sigmas[i])] + cs, hist)
        out = s._host_step(eps, t, x)
        S.assert_bit_equal(out.prev_sample, prev, f"step {i} prev_sample")
        S.assert_bit_equal(out.pred_original_sample, p0, f"step {i} pred_original_sample")
        S.assert_bit_equal(s.derivatives[-1], d, f"step {i} derivative")
        x = out.prev_sample


# ---------------------------------------------------------------------------------------------------------------------------
# history and order
# ---------------------------------------------------------------------------------------------------------------------------
def _orders(s, n, order=None):
    """The effective order of every step of an n-step trajectory, read off ``_plan`` right before the step."""
    s.set_timesteps(n)
    g = gen(1)
    x = torch.randn(SHAPE, generator=g)
    seen = []
    for t in s.timesteps.tolist():
        kw = {} if order is None else {"order": order}
        seen.append(s._plan(t, order or 4)[1])
        x = s.step(torch.randn(SHAPE, generator=g), t, x, **kw).prev_sample
        assert len(s.derivatives) <= (order or 4)
    return seen


def test_order_ramp_history_and_deepcopy():
    s = lms(**SD)
    assert _orders(s, 7) == [1, 2, 3, 4, 4, 4, 4] and len(s.derivatives) == 4
    assert _orders(s, 2) == [1, 2] and len(s.derivatives) == 2   # set_timesteps cleared the history
    assert _orders(s, 3) == [1, 2, 3] and len(s.derivatives) == 3
    assert _orders(s, 6, order=2) == [1, 2, 2, 2, 2, 2] and len(s.derivatives) == 2
    assert _orders(s, 4, order=1) == [1, 1, 1, 1] and len(s.derivatives) == 1
    s.set_timesteps(5)
    assert s.derivatives == [] and s.step_index is None
    x = torch.zeros(SHAPE)
    for bad in (0, 5):
        with pytest.raises(ValueError, match="order"):
            s.step(x, s.timesteps[0], x, order=bad)
    assert s.derivatives == [] and s.step_index in (None, 0)
    # a deep copy in mid-trajectory goes on exactly as the original does
    g = gen(8)
    x = torch.randn(SHAPE, generator=g)
    ts = s.timesteps.tolist()
    for t in ts[:3]:
        x = s.step(torch.randn(SHAPE, generator=g), t, x).prev_sample
    c = copy.deepcopy(s)
    assert c.step_index == 3 and len(c.derivatives) == 3 and all(a is not b and torch.equal(a, b) for a, b in zip(c.derivatives, s.derivatives))
    xc = x.clone()
    for t in ts[3:]:
        eps = torch.randn(SHAPE, generator=g)
        x, xc = s.step(eps, t, x).prev_sample, c.step(eps, t, xc).prev_sample
        assert torch.equal(x, xc)
    # raising the order in mid-trajectory never outruns the history
    s.set_timesteps(6)
    ts = s.timesteps.tolist()
    for t in ts[:3]:
        x = s.step(x, t, x, order=1).prev_sample
    assert s._plan(ts[3], 4)[1] == 2


def test_step_on_host_tensors_is_the_host_step():
    a, b = lms(**SD), lms(**SD)
    a.set_timesteps(6)
    b.set_timesteps(6)
    g = gen(2)
    x = torch.randn(SHAPE, generator=g)
    for t in a.timesteps:
        eps = torch.randn(SHAPE, generator=g)
        o1 = a.step(eps, t, x, return_dict=False, generator=g, noise=None)  # what the pipelines may hand over: accepted, ignored
        o2 = b._host_step(eps, t, x, return_dict=False)
        assert torch.equal(o1[0], o2[0]) and torch.equal(o1[1], o2[1]) and torch.equal(a.derivatives[-1], b.derivatives[-1])
        x = o1[0]
    with pytest.raises(TypeError):
        a.step(x, a.timesteps[0], x, eta=0.0)


def test_scale_model_input_divides_by_the_current_sigma():
    s = lms(**SD)
    s.set_timesteps(7)
    x = torch.randn(SHAPE, generator=gen(3))
    for i, t in enumerate(s.timesteps):
        want = x / ((s.sigmas[i] ** 2 + 1) ** 0.5)
        assert torch.equal(s.scale_model_input(x, t), want) and s.step_index == i
        assert torch.equal(x / torch.tensor(s.input_divisor(t), dtype=torch.float32), want)  # the float the pack kernel gets
        x = s.step(x, t, x).prev_sample


# ---------------------------------------------------------------------------------------------------------------------------
# protocol and pipelines (host only)
# ---------------------------------------------------------------------------------------------------------------------------
def test_config_protocol_and_unsupported_configs():
    from gm_diffusion.components import DDIMScheduler, EulerDiscreteScheduler, LMSDiscreteScheduler, PNDMScheduler

    d = LMSDiscreteScheduler()
    assert dict(d.config) == {**dict(d.config), **dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                                                     trained_betas=None, use_karras_sigmas=False, use_exponential_sigmas=False,
                                                     use_beta_sigmas=False, prediction_type="epsilon", timestep_spacing="linspace", steps_offset=0)}
    s = LMSDiscreteScheduler.from_config(PNDMScheduler(skip_prk_steps=True, steps_offset=1, timestep_spacing="leading", **SD).config)
    assert s.config.steps_offset == 1 and s.config.timestep_spacing == "leading" and s.config.beta_schedule == "scaled_linear"
    assert "skip_prk_steps" not in s.config and s.config.use_karras_sigmas is False and s.order == 1 and len(s) == 1000
    assert s.sigma_space and s.draws_noise(None) is False
    e = EulerDiscreteScheduler.from_config(s.config)
    back = LMSDiscreteScheduler.from_config(e.config)  # and back: Euler's extra keys are dropped
    assert back.config.timestep_spacing == "leading" and "final_sigmas_type" not in back.config
    DDIMScheduler.from_config(s.config)
    assert float(lms().init_noise_sigma) == float(lms().sigmas.max())  # before set_timesteps: the 1000-entry table
    with pytest.raises(NotImplementedError, match="epsilon"):
        LMSDiscreteScheduler(prediction_type="v_prediction")
    with pytest.raises(NotImplementedError, match="exponential"):
        LMSDiscreteScheduler(use_exponential_sigmas=True)
    with pytest.raises(NotImplementedError, match="beta sigmas"):
        LMSDiscreteScheduler(use_beta_sigmas=True)
    with pytest.raises(TypeError):
        LMSDiscreteScheduler(clip_sample=False)
    with pytest.raises(ValueError):
        LMSDiscreteScheduler().step(torch.zeros(1), 0, torch.zeros(1))  # set_timesteps not called
    with pytest.raises(ValueError, match="twice"):
        lms(**SD).set_timesteps(timesteps=[900, 900, 10])


def test_pipeline_recognition_step_kwargs_and_predraw():
    from gm_diffusion.pipelines import StableDiffusionGMPipeline as Pipe

    g = gen(0)
    pipe = Pipe.__new__(Pipe)
    s = lms(**SD)
    pipe.scheduler = s
    kw = pipe.prepare_extra_step_kwargs(g, 0.7)
    assert kw == {} and Pipe._fused_step_kwargs(kw) == {}  # deterministic: neither eta nor the generator
    s.set_timesteps(4)
    assert Pipe._pack_div(s, s.timesteps.tolist()[0]) == s.input_divisor() > 1.0
    assert Pipe._predraw_step_noise([s, copy.deepcopy(s)], s.timesteps.tolist(), (2, 4, 8, 8), g, "cpu") is None
    assert torch.equal(g.get_state(), gen(0).get_state())

    class FakeLatents:
        is_cuda = True

    from gm_diffusion.components import UNet2DConditionModel

    unet = UNet2DConditionModel.__new__(UNet2DConditionModel)
    assert pipe._use_fused(FakeLatents(), unet, s) and not pipe._use_fused(FakeLatents(), object(), s)
    assert not pipe._use_fused(FakeLatents(), unet, object())


def test_dual_pipeline_generic_branch_refuses_it_with_a_reason():
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline as Dual
    from oracle import fixtures

    pe, ne, lat = fixtures.make_inputs(1, 16, 16, cross_dim=64)
    pipe = Dual(vae=fixtures.build_vae("tiny"), text_encoder=None, tokenizer=None, unet=fixtures.build_unet("tiny", 4),
                gm_unet=fixtures.build_unet("tiny", 8), scheduler=lms(steps_offset=1, **SD), safety_checker=None, feature_extractor=None,
                requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    assert not pipe._use_fused(lat, pipe.unet, pipe.scheduler)
    with pytest.raises(ValueError, match="sigma-space scheduler"):
        pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, height=128, width=128, num_inference_steps=3, guidance_scale=7.5,
             output_type="latent")


def test_pipeline_from_pretrained_loads_the_scheduler_the_checkpoint_names(tmp_path):
    """A diffusers-layout directory whose scheduler/scheduler_config.json names LMSDiscreteScheduler (the original SD-1.x release's
    choice, with the foreign keys such a file carries): ``Pipeline.from_pretrained`` builds THAT class with the config on disk."""
    import json
    import os

    from gm_diffusion.components import LMSDiscreteScheduler
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline, StableDiffusionGMPipeline
    from oracle import fixtures

    on_disk = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", trained_betas=None,
                   prediction_type="epsilon", timestep_spacing="leading", steps_offset=1, use_karras_sigmas=True,
                   clip_sample=False, set_alpha_to_one=False, skip_prk_steps=True)  # the last three: foreign keys
    models = dict(vae=fixtures.build_vae("tiny"), unet=fixtures.build_unet("tiny", 8), text_encoder=None, tokenizer=None, safety_checker=None,
                  requires_safety_checker=False)
    root = tmp_path / "ckpt"
    os.makedirs(root / "scheduler")
    json.dump({"_class_name": "LMSDiscreteScheduler", "_diffusers_version": "0.33.0", **on_disk}, open(root / "scheduler" / "scheduler_config.json", "w"))
    json.dump({"_class_name": "StableDiffusionPipeline", "unet": ["diffusers", "UNet2DConditionModel"], "vae": ["diffusers", "AutoencoderKL"],
               "text_encoder": ["transformers", "CLIPTextModel"], "tokenizer": ["transformers", "CLIPTokenizer"],
               "scheduler": ["diffusers", "LMSDiscreteScheduler"]}, open(root / "model_index.json", "w"))
    for pipe in (StableDiffusionGMPipeline.from_pretrained(str(root), **models),
                 StableDiffusionDualUNetPipeline.from_pretrained(str(root), gm_unet=models["unet"], **models)):
        s = pipe.scheduler
        assert type(s) is LMSDiscreteScheduler
        assert s.config.timestep_spacing == "leading" and s.config.steps_offset == 1 and s.config.beta_schedule == "scaled_linear"
        assert s.config.use_karras_sigmas is True and "skip_prk_steps" not in s.config and "clip_sample" not in s.config
        s.set_timesteps(4)
        assert len(s.timesteps) == 4 and float(s.timesteps[0]) == 751.0 and float(s.init_noise_sigma) > 1.0
    one = LMSDiscreteScheduler.from_pretrained(str(root), subfolder="scheduler")
    assert one.config.beta_start == 0.00085


# ---------------------------------------------------------------------------------------------------------------------------
# ABI without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_abi_symbol_and_argument_validation_without_gpu():
    import os
    import re
    from ctypes import c_float, c_int, c_int64, c_void_p

    from gm_diffusion import _native as native

    lib = native.lib()
    assert lib.gmd_abi_version() == 14 and native.ABI_VERSION == 14
    P_, I, F = c_void_p, c_int, c_float
    want = [P_] * 5 + [I, c_int64, I, F, P_, F, I] + [F] * 5 + [P_] * 4
    assert native.SIGNATURES["gmd_lms_step"] == want and lib.gmd_lms_step.argtypes == want
    # the header declares the same argument list
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gmd_hip.h")).read()
    decl = re.search(r"int gmd_lms_step\((.*?)\);", header, re.S).group(1)
    kinds = []
    for arg in (a.strip() for a in decl.split(",")):
        kinds.append(P_ if ("*" in arg or arg.startswith("gmd_stream_t")) else c_int64 if arg.startswith("int64_t") else I if arg.startswith("int ") else F)
        assert kinds[-1] is not F or arg.startswith("float "), arg
    assert kinds == want
    one = 1  # any non-null address: validation happens before a launch, nothing is dereferenced
    nan, inf = float("nan"), float("inf")

    def step(eps=one, x=one, d1=None, d2=None, d3=None, B=1, chw=16, order=1, sigma=1.5, c=(-0.5, 0.0, 0.0, 0.0), d=one, xp=one, p0=None):
        return lib.gmd_lms_step(eps, x, d1, d2, d3, B, chw, 0, 1.0, None, 0.0, order, sigma, *c, d, xp, p0, None)

    for kw, word in ((dict(order=0), b"order 0"), (dict(order=5, d1=one, d2=one, d3=one), b"order 5"), (dict(sigma=0.0), b"sigma"),
                     (dict(sigma=nan), b"sigma"), (dict(sigma=-1.0), b"sigma"), (dict(c=(nan, 0.0, 0.0, 0.0)), b"c0"),
                     (dict(c=(inf, 0.0, 0.0, 0.0)), b"c0"), (dict(order=2, d1=one, c=(0.5, -inf, 0.0, 0.0)), b"c1"),
                     (dict(order=4, d1=one, d2=one, d3=one, c=(0.5, 0.5, 0.5, nan)), b"c3"),
                     (dict(order=3, d1=one, d2=None), b"needs d2"), (dict(order=2), b"needs d1"), (dict(order=4, d1=one, d2=one), b"needs d3"),
                     (dict(d=None), b"null"), (dict(xp=None), b"null"), (dict(eps=None), b"null"), (dict(x=None), b"null"),
                     (dict(B=-1), b"shape"), (dict(chw=0), b"shape")):
        assert step(**kw) == 1, kw  # GMD_ERR_INVALID
        assert word in lib.gmd_last_error(), (kw, lib.gmd_last_error())
    assert step(B=0, eps=None, x=None, d=None, xp=None) == 0  # an empty batch is a no-op
    assert step(B=0, order=3) == 0  # ... that needs no history either
    assert step(B=0, sigma=0.0) == 1  # ... but not an excuse for a bad scalar
    assert step(B=0, order=2, c=(0.5, 0.5, nan, inf)) == 0  # a coefficient beyond the order is not looked at


def test_wrapper_refuses_host_tensors():
    from gm_diffusion import hip_ops
    from gm_diffusion._native import HipExtensionError

    assert "lms_step" in hip_ops.__all__
    z = torch.zeros(1, 4, 8, 8)
    with pytest.raises(HipExtensionError):
        hip_ops.lms_step(z, z, 1, (1.5, -0.5, 0.0, 0.0, 0.0), False, 1.0)
    with pytest.raises(HipExtensionError):
        hip_ops.lms_step(z, z, 2, (1.5, -0.5, 0.1, 0.0, 0.0), False, 1.0, hist=(z,))
