"""CPU: components.EulerDiscreteScheduler / EulerAncestralDiscreteScheduler -- schedule tables against the float64 restatement
(tests/euler_ref.py), the host steps per element against float64 (allowed violations: 0), three identities that tie them to code written
earlier (DDIM at eta 0 and 1, the perfect predictor), generator accounting, the config protocol, and the argument validation of
gmd_euler_step / gmd_pack_unet_input_scaled.  No GPU is touched."""
import copy

import numpy as np
import pytest
import torch

import ddim_ref as D
import euler_ref as E
import parity as P

SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SHAPE = (3, 4, 8, 8)
SPACINGS = ("linspace", "leading", "trailing")
AYS = [14.615, 6.315, 3.771, 2.181, 1.342, 0.862, 0.555, 0.380, 0.234, 0.113, 0.0]  # a published 10-step sigma schedule for SDXL


def euler(**kw):
    from gm_diffusion.components import EulerDiscreteScheduler

    return EulerDiscreteScheduler(**kw)


def ancestral(**kw):
    from gm_diffusion.components import EulerAncestralDiscreteScheduler

    return EulerAncestralDiscreteScheduler(**kw)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def assert_2ulp(got, ref64, what):
    assert got.dtype == torch.float32, what
    g = got.numpy().astype(np.float64)
    assert g.shape == ref64.shape, (what, g.shape, ref64.shape)
    err, tol = np.abs(g - ref64), 2 * E.ulp32(ref64)
    assert bool((err <= tol).all()), f"{what}: worst {float((err - tol).max()):.3e} over 2 ulp at index {int((err - tol).argmax())}"


# ---------------------------------------------------------------------------------------------------------------------------
# schedule tables
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [euler, ancestral])
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("spacing", SPACINGS)
def test_schedule_tables_within_2ulp_of_float64(spacing, karras, cls):
    ac = E.alphas_cumprod(**SD)
    for n in (1, 2, 7, 8, 30):
        for offset in ((0, 1) if spacing == "leading" else (0,)):
            s = cls(timestep_spacing=spacing, use_karras_sigmas=karras, steps_offset=offset, **SD)
            s.set_timesteps(n)
            ts, sig = E.schedule64(ac, n, spacing, karras, offset)
            what = f"{spacing} karras={karras} n={n} offset={offset}"
            assert_2ulp(s.timesteps, ts, what + " timesteps")
            assert_2ulp(s.sigmas, sig, what + " sigmas")
            assert s.sigmas[-1] == 0 and len(s.sigmas) == n + 1 and s.num_inference_steps == n and s.step_index is None
            assert bool((s.sigmas[:-1] > 0).all()) and bool((s.sigmas[1:] < s.sigmas[:-1]).all())
            ins = s.init_noise_sigma
            ref = E.init_noise_sigma64(sig, spacing)
            assert abs(float(ins) - ref) <= 2 * float(E.ulp32(ref)), what
            assert (float(ins) == float(s.sigmas.max())) == (spacing != "leading")


def test_custom_sigmas_and_retrieve_timesteps():
    from gm_diffusion.pipelines import retrieve_timesteps

    ac = E.alphas_cumprod(**SD)
    ts, sig = E.schedule64(ac, sigmas=AYS)
    for s in (euler(**SD), ancestral(**SD)):
        got_ts, n = retrieve_timesteps(s, None, None, None, AYS)  # the sigmas= branch of the pipelines' helper
        assert n == 10 and got_ts is s.timesteps
        assert_2ulp(s.timesteps, ts, "custom sigmas: timesteps")
        assert torch.equal(s.sigmas, torch.tensor(AYS, dtype=torch.float32))
        assert s.timesteps[0] == 999.0 and 844 < float(s.timesteps[1]) < 846
        with pytest.raises(ValueError):
            s.set_timesteps(timesteps=[999, 500], sigmas=AYS)
        with pytest.raises(ValueError):
            s.set_timesteps(sigmas=[1.0, 2.0, 0.0])
    s = euler(**SD)
    s.set_timesteps(timesteps=[900.5, 400.25, 10])
    assert s.timesteps.tolist() == [900.5, 400.25, 10.0]
    with pytest.raises(ValueError):
        euler(use_karras_sigmas=True, **SD).set_timesteps(sigmas=AYS)


def test_seven_linspace_timesteps_are_fractional_float32_bit_for_bit():
    want = np.linspace(0, 999, 7, dtype=np.float32)[::-1].copy()
    assert want[1] == np.float32(832.5) and any(float(v) != int(v) for v in want)
    for s in (euler(**SD), ancestral(**SD)):
        assert s.config.timestep_spacing == "linspace"  # the class default
        s.set_timesteps(7)
        assert s.timesteps.dtype == torch.float32 and s.timesteps.numpy().tobytes() == want.tobytes()
        c = copy.deepcopy(s)
        x = torch.randn(SHAPE, generator=gen(0))
        for i, t in enumerate(s.timesteps.tolist()):  # the host list the pipelines walk: every value finds its own step
            assert c.input_divisor(t) == float((s.sigmas[i] ** 2 + 1) ** 0.5) and c.step_index == i
            c.step(x, t, x, generator=gen(1))
        s.set_timesteps(8)
        assert float(s.timesteps[1]) == float(np.float32(999 * 6 / 7)) and float(s.timesteps[1]) != int(s.timesteps[1])
        with pytest.raises(ValueError, match="not in the schedule"):
            s.step(x, int(s.timesteps[1]), x)  # a truncated timestep is refused, not matched to a neighbour


# ---------------------------------------------------------------------------------------------------------------------------
# the host step against the float64 function
# ---------------------------------------------------------------------------------------------------------------------------
def _plain_f32(eps, x, noise, sf, st, is_ancestral):
    """The diffusers expressions on float32 0-d tensors, written out here (not the product class): what the bound is confirmed on."""
    sf, st = torch.tensor(sf, dtype=torch.float32), torch.tensor(st, dtype=torch.float32)
    p0 = x - sf * eps
    d = (x - p0) / sf
    if not is_ancestral:
        return x + d * (st - sf), p0
    su = (st ** 2 * (sf ** 2 - st ** 2) / sf ** 2) ** 0.5
    sd = (st ** 2 - su ** 2) ** 0.5
    return x + d * (sd - sf) + noise * su, p0


@pytest.mark.parametrize("n", [1, 7, 30])
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("is_ancestral", [False, True])
def test_host_step_within_bound_of_float64(is_ancestral, spacing, karras, n):
    """Whole trajectories on unit-normal model outputs: |host step - float64| <= 7 2^-24 A + A_d |D dt| + |n| |D su| per element for
    prev_sample, 2 2^-24 A_p0 for pred_original_sample, after confirming that the plain float32 expressions sit inside the same bounds.
    The last step is the do-nothing edge: dt = -sigma (the result is the x0 prediction) and sigma_up = 0 (the noise is added as 0)."""
    s = (ancestral if is_ancestral else euler)(timestep_spacing=spacing, use_karras_sigmas=karras, **SD)
    s.set_timesteps(n)
    g = gen(11)
    x = torch.randn(SHAPE, generator=g) * s.init_noise_sigma
    worst = 0.0
    for i, t in enumerate(s.timesteps.tolist()):
        eps, noise = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
        sf, st = float(s.sigmas[i]), float(s.sigmas[i + 1])
        dt, su = (E.ancestral_coefs64 if is_ancestral else E.euler_coefs64)(sf, st)
        d_dt, d_su = E.coef_err(sf, st, is_ancestral)
        ref, p0_ref, mags = E.step64(eps, x, noise if is_ancestral else None, sf, dt, su)
        b = E.bound(mags, d_dt, d_su)
        plain, plain_p0 = _plain_f32(eps, x, noise, sf, st, is_ancestral)
        P.assert_elementwise(plain, ref, b, f"plain float32 expression step {i}")
        P.assert_elementwise(plain_p0, p0_ref, E.bound_p0(mags), f"plain float32 p0 step {i}")
        assert s.step_index in (None, i)
        out = s._host_step(eps, t, x, noise=noise) if is_ancestral else s._host_step(eps, t, x)
        worst = max(worst, P.assert_elementwise(out.prev_sample, ref, b, f"host step prev_sample step {i}"))
        P.assert_elementwise(out.pred_original_sample, p0_ref, E.bound_p0(mags), f"host step pred_original_sample step {i}")
        assert out.prev_sample.dtype == torch.float32 and out[0] is out.prev_sample and s.step_index == i + 1
        if i == n - 1:
            assert st == 0.0 and dt == -sf and su == 0.0
            P.assert_elementwise(out.prev_sample, p0_ref, b, "last step: prev_sample is the x0 prediction")
        x = out.prev_sample
    print(f"ancestral={is_ancestral} {spacing} karras={karras} n={n}: max |err| / bound = {worst:.3f}")


def test_step_on_host_tensors_is_the_host_step():
    for mk, kw in ((euler, {}), (ancestral, dict(generator=None))):
        a, b = mk(**SD), mk(**SD)
        a.set_timesteps(5)
        b.set_timesteps(5)
        g = gen(2)
        x = torch.randn(SHAPE, generator=g)
        for t in a.timesteps:
            eps, noise = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
            nk = dict(noise=noise) if mk is ancestral else {}
            o1 = a.step(eps, t, x, return_dict=False, **nk)
            o2 = b._host_step(eps, t, x, return_dict=False, **nk)
            assert torch.equal(o1[0], o2[0]) and torch.equal(o1[1], o2[1])
            x = o1[0]


def test_scale_model_input_divides_by_the_current_sigma():
    s = euler(**SD)
    s.set_timesteps(7)
    x = torch.randn(SHAPE, generator=gen(3))
    for i, t in enumerate(s.timesteps):
        want = x / ((s.sigmas[i] ** 2 + 1) ** 0.5)
        assert torch.equal(s.scale_model_input(x, t), want) and s.step_index == i
        assert torch.equal(x / torch.tensor(s.input_divisor(t), dtype=torch.float32), want)  # the float the pack kernel gets
        x = s.step(x, t, x).prev_sample


# ---------------------------------------------------------------------------------------------------------------------------
# identities
# ---------------------------------------------------------------------------------------------------------------------------
def _ddim_alphas(d, t):
    p = int(t) - d.config.num_train_timesteps // d.num_inference_steps
    return float(d.alphas_cumprod[int(t)]), (float(d.alphas_cumprod[p]) if p >= 0 else 1.0), p


@pytest.mark.parametrize("n", [8, 30])
@pytest.mark.parametrize("is_ancestral", [False, True])
def test_step_in_scaled_coordinates_is_ddim(is_ancestral, n):
    """An Euler step on x (1 + sigma^2)^.5, divided by (1 + sigma_next^2)^.5, is the DDIM step (eta = 0; leading, steps_offset 1,
    clip off, set_alpha_to_one) on x; the ancestral step is the same DDIM step at eta = 1 with the same variance_noise.  Per step from a
    common state, per element, within the sum of the three derived bounds (tests/euler_ref.py, "Identities")."""
    from gm_diffusion.components import DDIMScheduler

    kw = dict(timestep_spacing="leading", steps_offset=1, **SD)
    s = (ancestral if is_ancestral else euler)(**kw)
    d = DDIMScheduler(clip_sample=False, set_alpha_to_one=True, **kw)
    s.set_timesteps(n)
    d.set_timesteps(n)
    assert s.timesteps.tolist() == [float(v) for v in d.timesteps.tolist()]
    eta = 1.0 if is_ancestral else 0.0
    g = gen(5)
    worst = 0.0
    for i, t in enumerate(d.timesteps.tolist()):
        x, eps, noise = (torch.randn(SHAPE, generator=g) for _ in range(3))
        sf, st = float(s.sigmas[i]), float(s.sigmas[i + 1])
        c, cn = (1 + sf * sf) ** 0.5, (1 + st * st) ** 0.5
        xs = (x.double() * c).float()
        one = copy.deepcopy(s)  # a common state: this step only
        got = (one._host_step(eps, float(t), xs, noise=noise) if is_ancestral else one._host_step(eps, float(t), xs)).prev_sample
        assert one.step_index == i + 1
        ddim = d._host_step(eps, t, x, eta=eta, variance_noise=noise if is_ancestral else None).prev_sample
        dt, su = (E.ancestral_coefs64 if is_ancestral else E.euler_coefs64)(sf, st)
        _, _, mags = E.step64(eps, xs, noise if is_ancestral else None, sf, dt, su)
        a_t, a_prev, p = _ddim_alphas(d, t)
        _, _, a_ddim = D.ddim_step64(eps, x, noise, a_t, a_prev, eta)
        b = E.bound(mags, *E.coef_err(sf, st, is_ancestral)) / cn + E.identity_slack(x, eps, noise, sf, st, is_ancestral) + D.bound(a_ddim)
        worst = max(worst, P.assert_elementwise(got.double() / cn, ddim.double(), b, f"step {i} (t={t})"))
    assert p < 0 and st == 0.0, "the trajectory must end on the step that uses alpha = 1 / sigma = 0"
    print(f"ancestral={is_ancestral} n={n}: max |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("spacing", SPACINGS)
def test_perfect_predictor_lands_on_x0_plus_sigma_next_eps(spacing, karras):
    """x = x0 + sigma e with the model output == e: every Euler step lands on x0 + sigma_next e, the last one on x0."""
    s = euler(timestep_spacing=spacing, use_karras_sigmas=karras, **SD)
    s.set_timesteps(8)
    g = gen(3)
    x0, e = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
    for i, t in enumerate(s.timesteps.tolist()):
        sf, st = float(s.sigmas[i]), float(s.sigmas[i + 1])
        x = (x0.double() + sf * e.double()).float()
        one = copy.deepcopy(s)
        got = one.step(e, t, x).prev_sample
        _, _, mags = E.step64(e, x, None, sf, st - sf)
        b = E.bound(mags, *E.coef_err(sf, st, False)) + E.U_F32 * x.double().abs()
        P.assert_elementwise(got, x0.double() + st * e.double(), b, f"step {i}")
    assert st == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# generator accounting
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_ancestral", [False, True])
def test_generator_is_advanced_once_per_step_iff_ancestral(is_ancestral):
    s = (ancestral if is_ancestral else euler)(**SD)
    s.set_timesteps(7)
    g, twin = gen(9), gen(9)
    x = torch.randn(SHAPE, generator=gen(1))
    for t in s.timesteps.tolist():
        assert s.draws_noise(t) == is_ancestral
        x = s.step(torch.randn(SHAPE, generator=gen(100)), t, x, generator=g).prev_sample
    for _ in range(7 if is_ancestral else 0):  # n tensors of the sample's shape: the last step (sigma_up == 0) draws too
        torch.randn(SHAPE, generator=twin)
    assert torch.equal(g.get_state(), twin.get_state())


def test_predrawn_noise_slots_cover_every_step_sdr_before_gm():
    from gm_diffusion.components.image_processor import randn_tensor
    from gm_diffusion.pipelines import StableDiffusionGMPipeline as Pipe

    shape = (2, 4, 8, 8)
    e1 = euler(**SD)
    e1.set_timesteps(4)
    assert Pipe._predraw_step_noise([e1, copy.deepcopy(e1)], e1.timesteps.tolist(), shape, gen(5), "cpu") is None  # nothing to draw
    s1 = ancestral(**SD)
    s1.set_timesteps(4)
    s2 = copy.deepcopy(s1)
    ts = s1.timesteps.tolist()
    g0 = gen(5)
    pre = Pipe._predraw_step_noise([s1, s2], ts, shape, g0, "cpu")
    g = gen(5)
    for i in range(len(ts)):
        for k in range(2):
            assert torch.equal(pre[k][i], randn_tensor(shape, generator=g, device="cpu", dtype=torch.float32)), (i, k)
    assert torch.equal(g0.get_state(), g.get_state())
    # a pre-drawn tensor replaces the draw: the generator handed along with it is not touched
    g1 = gen(6)
    a = s1.step(pre[0][0], ts[0], pre[0][1], generator=g1, noise=pre[1][0]).prev_sample
    b = s2.step(pre[0][0], ts[0], pre[0][1], noise=pre[1][0]).prev_sample
    assert torch.equal(a, b) and torch.equal(g1.get_state(), gen(6).get_state())


def test_pipeline_step_kwargs_and_fused_recognition():
    from gm_diffusion.pipelines import StableDiffusionGMPipeline as Pipe

    g = gen(0)
    pipe = Pipe.__new__(Pipe)
    for s in (euler(**SD), ancestral(**SD)):
        pipe.scheduler = s
        kw = pipe.prepare_extra_step_kwargs(g, 0.7)
        assert kw == {"generator": g} and Pipe._fused_step_kwargs(kw) == {"generator": g}
        s.set_timesteps(3)
        assert Pipe._pack_div(s, s.timesteps.tolist()[0]) == s.input_divisor() > 1.0
    from gm_diffusion.components import PNDMScheduler

    assert Pipe._pack_div(PNDMScheduler(skip_prk_steps=True, **SD), 981) is None


# ---------------------------------------------------------------------------------------------------------------------------
# config protocol, unsupported configurations
# ---------------------------------------------------------------------------------------------------------------------------
def test_config_protocol_and_unsupported_configs():
    from gm_diffusion.components import DDIMScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler, PNDMScheduler

    e = EulerDiscreteScheduler.from_config(PNDMScheduler(skip_prk_steps=True, steps_offset=1, timestep_spacing="leading", **SD).config)
    assert e.config.steps_offset == 1 and e.config.timestep_spacing == "leading" and e.config.beta_schedule == "scaled_linear"
    assert "skip_prk_steps" not in e.config and e.config.use_karras_sigmas is False and e.order == 1 and len(e) == 1000
    a = EulerAncestralDiscreteScheduler.from_config(e.config)
    assert a.config.timestep_spacing == "leading" and "final_sigmas_type" not in a.config
    DDIMScheduler.from_config(a.config)  # and back
    assert float(euler().init_noise_sigma) == float(euler().sigmas.max())  # before set_timesteps: the 1000-entry table
    for cls in (EulerDiscreteScheduler, EulerAncestralDiscreteScheduler):
        with pytest.raises(NotImplementedError, match="epsilon"):
            cls(prediction_type="v_prediction")
        with pytest.raises(TypeError):
            cls(clip_sample=False)
        with pytest.raises(ValueError):
            cls().step(torch.zeros(1), 0, torch.zeros(1))  # set_timesteps not called
    for bad, word in ((dict(interpolation_type="log_linear"), "interpolation_type"), (dict(timestep_type="continuous"), "timestep_type"),
                      (dict(final_sigmas_type="sigma_min"), "final_sigmas_type"), (dict(use_exponential_sigmas=True), "exponential"),
                      (dict(use_beta_sigmas=True), "beta sigmas")):
        with pytest.raises(NotImplementedError, match=word):
            EulerDiscreteScheduler(**bad)
    s = euler(**SD)
    s.set_timesteps(3)
    x = torch.zeros(SHAPE)
    with pytest.raises(NotImplementedError, match="s_churn"):
        s.step(x, s.timesteps[0], x, s_churn=0.5)
    assert s.step_index in (None, 0)


def test_dual_pipeline_generic_branch_refuses_sigma_space_with_a_reason():
    """Host latents cannot take the fused path; the generic dual loop restates the reference, which cannot run a sigma-space scheduler
    (it indexes alphas_cumprod with the timestep): a ValueError that says so, before any UNet call, not an IndexError."""
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline as Dual
    from oracle import fixtures

    pe, ne, lat = fixtures.make_inputs(1, 16, 16, cross_dim=64)
    for mk in (euler, ancestral):
        pipe = Dual(vae=fixtures.build_vae("tiny"), text_encoder=None, tokenizer=None, unet=fixtures.build_unet("tiny", 4),
                    gm_unet=fixtures.build_unet("tiny", 8), scheduler=mk(steps_offset=1, **SD), safety_checker=None, feature_extractor=None,
                    requires_safety_checker=False)
        pipe.set_progress_bar_config(disable=True)
        assert not pipe._use_fused(lat, pipe.unet, pipe.scheduler)
        with pytest.raises(ValueError, match="sigma-space scheduler"):
            pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, height=128, width=128, num_inference_steps=3, guidance_scale=7.5,
                 output_type="latent")


def test_pipeline_from_pretrained_loads_the_scheduler_the_checkpoint_names(tmp_path):
    """A diffusers-layout directory whose model_index.json names EulerDiscreteScheduler (an SDXL-base checkpoint's scheduler/ folder,
    with the foreign keys such a file carries) or EulerAncestralDiscreteScheduler: ``Pipeline.from_pretrained`` builds THAT class with
    the config on disk, not the PNDM fallback of an unknown scheduler name.  The models are passed in, so only the scheduler is loaded."""
    import json
    import os

    from gm_diffusion.components import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline, StableDiffusionGMPipeline
    from oracle import fixtures

    on_disk = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", trained_betas=None,
                   prediction_type="epsilon", timestep_spacing="leading", steps_offset=1, use_karras_sigmas=False,
                   clip_sample=False, set_alpha_to_one=False, skip_prk_steps=True, sample_max_value=1.0)  # the last four: foreign keys
    models = dict(vae=fixtures.build_vae("tiny"), unet=fixtures.build_unet("tiny", 8), text_encoder=None, tokenizer=None, safety_checker=None,
                  requires_safety_checker=False)
    for cls, extra in ((EulerDiscreteScheduler, dict(interpolation_type="linear", timestep_type="discrete", final_sigmas_type="zero")),
                       (EulerAncestralDiscreteScheduler, {})):
        root = tmp_path / cls.__name__
        os.makedirs(root / "scheduler")
        json.dump({"_class_name": cls.__name__, "_diffusers_version": "0.33.0", **on_disk, **extra}, open(root / "scheduler" / "scheduler_config.json", "w"))
        json.dump({"_class_name": "StableDiffusionPipeline", "unet": ["diffusers", "UNet2DConditionModel"], "vae": ["diffusers", "AutoencoderKL"],
                   "text_encoder": ["transformers", "CLIPTextModel"], "tokenizer": ["transformers", "CLIPTokenizer"],
                   "scheduler": ["diffusers", cls.__name__]}, open(root / "model_index.json", "w"))
        for pipe in (StableDiffusionGMPipeline.from_pretrained(str(root), **models),
                     StableDiffusionDualUNetPipeline.from_pretrained(str(root), gm_unet=models["unet"], **models)):
            s = pipe.scheduler
            assert type(s) is cls
            assert s.config.timestep_spacing == "leading" and s.config.steps_offset == 1 and s.config.beta_schedule == "scaled_linear"
            assert s.config.beta_start == 0.00085 and "skip_prk_steps" not in s.config and "clip_sample" not in s.config
            s.set_timesteps(4)
            assert s.timesteps.tolist() == [751.0, 501.0, 251.0, 1.0] and float(s.init_noise_sigma) > 1.0


def test_a_schedule_that_repeats_a_timestep_is_refused():
    """Custom sigmas above the training range all map to the last train timestep; the step could not be told from the timestep (and the
    pipelines walk the schedule from its first entry): refused by set_timesteps.  input_divisor needs a timestep until a step is fixed."""
    for s in (euler(**SD), ancestral(**SD)):
        with pytest.raises(ValueError, match="twice"):
            s.set_timesteps(sigmas=[40.0, 20.0, 5.0, 1.0, 0.0])
        with pytest.raises(ValueError, match="twice"):
            s.set_timesteps(timesteps=[900, 900, 10])
        s.set_timesteps(sigmas=[14.0, 5.0, 1.0, 0.0])
        with pytest.raises(ValueError, match="timestep is needed"):
            s.input_divisor()
        assert s.input_divisor(s.timesteps[0]) == s.input_divisor() == float((s.sigmas[0] ** 2 + 1) ** 0.5) and s.step_index == 0


# ---------------------------------------------------------------------------------------------------------------------------
# ABI without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_argument_validation_without_gpu():
    from ctypes import c_float, c_int, c_int64, c_void_p

    from gm_diffusion import _native as native

    lib = native.lib()
    assert lib.gmd_abi_version() == 14 and native.ABI_VERSION == 14
    P_, I, L, F = c_void_p, c_int, c_int64, c_float
    assert native.SIGNATURES["gmd_euler_step"] == [P_, P_, P_, I, L, I, F, P_, F, F, F, F, P_, P_, P_]
    assert native.SIGNATURES["gmd_pack_unet_input_scaled"] == [P_, I, F, P_, I, F, I, L, I, P_, I, I, P_]
    assert lib.gmd_euler_step.argtypes == native.SIGNATURES["gmd_euler_step"]
    assert lib.gmd_pack_unet_input_scaled.argtypes == native.SIGNATURES["gmd_pack_unet_input_scaled"]
    one = 1  # any non-null address: validation happens before a launch, nothing is dereferenced
    nan, inf = float("nan"), float("inf")

    def step(eps=one, x=one, noise=None, B=1, chw=16, sh=1.5, dt=-0.5, su=0.0, xp=one, p0=None):
        return lib.gmd_euler_step(eps, x, noise, B, chw, 0, 1.0, None, 0.0, sh, dt, su, xp, p0, None)

    for kw, word in ((dict(eps=None), b"null"), (dict(x=None), b"null"), (dict(xp=None), b"null"), (dict(B=-1), b"shape"),
                     (dict(chw=0), b"shape"), (dict(sh=0.0), b"sigma_hat"), (dict(sh=-1.0), b"sigma_hat"), (dict(sh=nan), b"sigma_hat"),
                     (dict(su=-0.1), b"sigma_up"), (dict(su=nan), b"sigma_up"), (dict(dt=nan), b"dt"), (dict(dt=inf), b"dt"),
                     (dict(dt=-inf), b"dt")):
        assert step(**kw) == 1, kw  # GMD_ERR_INVALID
        assert word in lib.gmd_last_error(), (kw, lib.gmd_last_error())
    assert step(B=0, eps=None, x=None, xp=None) == 0  # an empty batch is a no-op
    assert step(B=0, sh=0.0) == 1  # ... but not an excuse for a bad scalar

    def pack(s0=one, c0=4, d0=1.5, s1=one, c1=4, d1=1.5, B=1, hw=16, dup=1, out=one, cp=8, dt=0):
        return lib.gmd_pack_unet_input_scaled(s0, c0, d0, s1, c1, d1, B, hw, dup, out, cp, dt, None)

    for kw, word in ((dict(d0=0.0), b"div0"), (dict(d0=-1.0), b"div0"), (dict(d0=nan), b"div0"), (dict(d1=0.0), b"div1"),
                     (dict(d1=nan), b"div1"), (dict(s0=None), b"null"), (dict(out=None), b"null"), (dict(s1=None), b"src1"),
                     (dict(cp=12), b"CP"), (dict(cp=4), b"CP"), (dict(dup=3), b"dup"), (dict(dt=9), b"dtype"), (dict(c0=0), b"shape")):
        assert pack(**kw) == 1, kw
        assert word in lib.gmd_last_error(), (kw, lib.gmd_last_error())
    assert pack(B=0, s0=None, out=None) == 0
    assert pack(B=0, s1=None, c1=0, d1=nan) == 0  # a second divisor without a second source is not read


def test_wrappers_refuse_host_tensors():
    from gm_diffusion import hip_ops
    from gm_diffusion._native import HipExtensionError

    assert "euler_step" in hip_ops.__all__
    z = torch.zeros(1, 4, 8, 8)
    with pytest.raises(HipExtensionError):
        hip_ops.euler_step(z, z, (1.5, -0.5, 0.0), False, 1.0)
    with pytest.raises(HipExtensionError):
        hip_ops.pack_unet_input(z, None, 1, 8, torch.float32, div=(1.5, 1.0))
