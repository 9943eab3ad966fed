"""CPU: components.DDIMScheduler -- timestep tables, the host step against the float64 restatement (tests/ddim_ref.py; per element,
allowed violations: 0), identities that tie it to code written earlier (DDPM's ancestral step, the perfect predictor, PNDM's first-order
update), generator accounting, the config protocol, and the argument validation of gmd_ddim_step.  No GPU is touched."""
import copy
import math

import pytest
import torch

import ddim_ref as D
import parity as P

SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SHAPE = (3, 4, 8, 8)


def ddim(**kw):
    from gm_diffusion.components import DDIMScheduler

    return DDIMScheduler(**kw)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------
# timestep tables, known answers
# ---------------------------------------------------------------------------------------------------------------------------
def test_timestep_tables_known_answers():
    s = ddim(steps_offset=1, **SD)
    s.set_timesteps(50)
    assert s.timesteps.tolist() == list(range(981, 0, -20)) and s.timesteps.dtype == torch.int64
    s = ddim(timestep_spacing="trailing", **SD)
    s.set_timesteps(50)
    assert s.timesteps.tolist() == list(range(999, 0, -20)) and s.timesteps[-1] == 19
    s = ddim(timestep_spacing="linspace", **SD)
    s.set_timesteps(10)
    assert s.timesteps.tolist() == [999, 888, 777, 666, 555, 444, 333, 222, 111, 0]
    assert s.init_noise_sigma == 1.0 and s.order == 1 and len(s) == 1000
    x = torch.ones(2)
    assert s.scale_model_input(x, 5) is x


# ---------------------------------------------------------------------------------------------------------------------------
# the host step against the float64 function
# ---------------------------------------------------------------------------------------------------------------------------
def _alphas(s, t):
    """(a_t, a_prev) of the product scheduler's own table as Python floats, prev_t by the rule of the issue (t - T // n)."""
    p = int(t) - s.config.num_train_timesteps // s.num_inference_steps
    a_prev = float(s.alphas_cumprod[p]) if p >= 0 else (1.0 if s.config.set_alpha_to_one else float(s.alphas_cumprod[0]))
    return float(s.alphas_cumprod[int(t)]), a_prev, p


def _plain_f32(eps, x, noise, a_t, a_prev, eta, clip, use_clipped):
    """The diffusers expressions on float32 0-d tensors, written out here (not the product class): what the bound is confirmed on."""
    a_t, a_prev = torch.tensor(a_t, dtype=torch.float32), torch.tensor(a_prev, dtype=torch.float32)
    b_t = 1 - a_t
    p0 = (x - b_t ** 0.5 * eps) / a_t ** 0.5
    pe = eps
    if clip is not None:
        p0 = p0.clamp(-clip, clip)
    variance = ((1 - a_prev) / b_t) * (1 - a_t / a_prev)
    std = eta * variance ** 0.5
    if use_clipped:
        pe = (x - a_t ** 0.5 * p0) / b_t ** 0.5
    prev = a_prev ** 0.5 * p0 + (1 - a_prev - std ** 2) ** 0.5 * pe
    if eta > 0:
        prev = prev + std * noise
    return prev, p0


@pytest.mark.parametrize("set_alpha_to_one", [True, False])
@pytest.mark.parametrize("use_clipped", [False, True])
@pytest.mark.parametrize("clip", [None, 1.5])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_host_step_within_bound_of_float64(eta, clip, use_clipped, set_alpha_to_one):
    """A full 7-step trajectory (the last step has prev_t < 0), unit-normal inputs: |host step - float64| <= 16 2^-24 A per element
    for prev_sample and pred_original_sample, after confirming that the plain float32 expressions sit inside the same bound."""
    s = ddim(clip_sample=clip is not None, clip_sample_range=clip or 1.0, set_alpha_to_one=set_alpha_to_one, **SD)
    s.set_timesteps(7)
    g = gen(11)
    x = torch.randn(SHAPE, generator=g)
    worst = 0.0
    for t in s.timesteps.tolist():
        eps, noise = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
        a_t, a_prev, p = _alphas(s, t)
        ref, p0_ref, a = D.ddim_step64(eps, x, noise, a_t, a_prev, eta, clip, use_clipped)
        a_p0 = (x.double().abs() + (1 - a_t) ** 0.5 * eps.double().abs()) / a_t ** 0.5
        plain, plain_p0 = _plain_f32(eps, x, noise, a_t, a_prev, eta, clip, use_clipped)
        P.assert_elementwise(plain, ref, D.bound(a), f"plain float32 expression t={t}")
        P.assert_elementwise(plain_p0, p0_ref, D.bound(a_p0), f"plain float32 p0 t={t}")
        out = s._host_step(eps, t, x, eta=eta, use_clipped_model_output=use_clipped, variance_noise=noise if eta > 0 else None)
        worst = max(worst, P.assert_elementwise(out.prev_sample, ref, D.bound(a), f"host step prev_sample t={t}"))
        P.assert_elementwise(out.pred_original_sample, p0_ref, D.bound(a_p0), f"host step pred_original_sample t={t}")
        assert out.prev_sample.dtype == torch.float32 and out[0] is out.prev_sample
        tup = s.step(eps, t, x, eta=eta, use_clipped_model_output=use_clipped, variance_noise=noise if eta > 0 else None, return_dict=False)
        assert torch.equal(tup[0], out.prev_sample) and torch.equal(tup[1], out.pred_original_sample)  # host tensors: step IS _host_step
        x = out.prev_sample
    assert p < 0, "the trajectory must end on the step that uses final_alpha_cumprod"
    print(f"eta={eta} clip={clip} use_clipped={use_clipped} one={set_alpha_to_one}: max |err| / bound = {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------
# identities
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_eta_one_clipped_output_equals_ddpm_fixed_small(seed, clip):
    """(a) eta = 1 with use_clipped_model_output is DDPM's ancestral step (fixed_small): 1000 inference steps (prev = t - 1), same clip
    setting, same noise tensor.  Measured 1.3e-5 .. 3.5e-5 over seeds and timestep choices; gate 1e-4 (about 3-5x, for seed spread)."""
    from gm_diffusion.components import DDPMScheduler

    d = ddim(clip_sample=clip, set_alpha_to_one=True, **SD)
    p = DDPMScheduler(clip_sample=clip, variance_type="fixed_small", **SD)
    d.set_timesteps(1000)
    p.set_timesteps(1000)
    g = gen(seed)
    worst = 0.0
    for t in (999, 750, 500, 250, 20, 1, 0):
        x, eps = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
        noise = torch.randn(SHAPE, generator=gen(1000 + t))  # the tensor DDPM draws from a generator with the same seed
        got = d._host_step(eps, t, x, eta=1.0, use_clipped_model_output=True, variance_noise=noise).prev_sample
        ref = p._host_step(eps, t, x, generator=gen(1000 + t), return_dict=False)[0]  # t == 0: DDPM adds no noise, DDIM's std is 0
        worst = max(worst, float((got - ref).abs().max()))
    print(f"seed {seed} clip {clip}: max abs {worst:.2e}")
    assert worst <= 1e-4


@pytest.mark.parametrize("n,offset", [(7, 0), (10, 0), (50, 1)])
def test_perfect_predictor_lands_on_the_forward_marginals(n, offset):
    """(b) x_T = sqrt(a_T) x0 + sqrt(1 - a_T) e with the model output == e, eta = 0, clip off: every step lands on
    sqrt(a_prev) x0 + sqrt(1 - a_prev) e, the last one (set_alpha_to_one) on x0.  Measured 1.3e-6 / 1.7e-6 / 6.7e-6; gate 2e-5."""
    s = ddim(clip_sample=False, set_alpha_to_one=True, steps_offset=offset, **SD)
    s.set_timesteps(n)
    g = gen(3)
    x0, e = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
    a_T = s.alphas_cumprod[int(s.timesteps[0])]
    x = a_T.sqrt() * x0 + (1 - a_T).sqrt() * e
    worst = 0.0
    for t in s.timesteps.tolist():
        x = s.step(e, t, x, eta=0.0).prev_sample
        _, a_prev, p = _alphas(s, t)
        want = math.sqrt(a_prev) * x0.double() + math.sqrt(1 - a_prev) * e.double()
        worst = max(worst, float((x.double() - want).abs().max()))
    assert p < 0
    worst = max(worst, float((x - x0).abs().max()))
    print(f"{n} steps: max abs {worst:.2e}")
    assert worst <= 2e-5


def test_eta_zero_equals_pndm_first_order_update():
    """(c) eta = 0 without clipping is PNDM's first-order update sc x - (a_prev - a_t) eps / denom (PNDMScheduler._coefs), at every t of
    a 50-step table with prev_t >= 0.  Measured 7.7e-7 .. 9.5e-7; gate 4e-6."""
    from gm_diffusion.components import PNDMScheduler

    s = ddim(clip_sample=False, steps_offset=1, **SD)
    pn = PNDMScheduler(skip_prk_steps=True, steps_offset=1, **SD)
    s.set_timesteps(50)
    g = gen(4)
    worst, n = 0.0, 0
    for t in s.timesteps.tolist():
        prev_t = t - 20
        if prev_t < 0:
            continue
        x, eps = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
        sc, ad, dn = pn._coefs(t, prev_t)
        ref = sc * x - ad * eps / dn
        worst = max(worst, float((s.step(eps, t, x).prev_sample - ref).abs().max()))
        n += 1
    assert n == 49
    print(f"max abs {worst:.2e}")
    assert worst <= 4e-6


# ---------------------------------------------------------------------------------------------------------------------------
# generator accounting
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta,draws", [(0.0, 0), (0.5, 7), (1.0, 7)])
def test_generator_is_advanced_once_per_step_iff_eta_positive(eta, draws):
    s = ddim(clip_sample=False, **SD)
    s.set_timesteps(7)
    g, twin = gen(9), gen(9)
    x = torch.randn(SHAPE, generator=gen(1))
    for t in s.timesteps.tolist():
        assert s.draws_noise(t, eta) == (eta > 0)
        x = s.step(torch.randn(SHAPE, generator=gen(100 + t)), t, x, eta=eta, generator=g).prev_sample
    for _ in range(draws):  # n tensors of the sample's shape: the last step (std == 0 with set_alpha_to_one) draws too
        torch.randn(SHAPE, generator=twin)
    assert torch.equal(g.get_state(), twin.get_state())
    with pytest.raises(ValueError):
        s.step(x, 0, x, eta=eta, generator=g, variance_noise=x)


def test_predrawn_noise_slots_cover_every_step_sdr_before_gm():
    """The pipelines' pre-draw: with DDIM every (step, scheduler) is a slot iff eta > 0, SDR before GM within an iteration."""
    from gm_diffusion.components.image_processor import randn_tensor
    from gm_diffusion.pipelines import StableDiffusionGMPipeline as Pipe

    s1 = ddim(clip_sample=False, **SD)
    s1.set_timesteps(4)
    s2 = copy.deepcopy(s1)
    ts = [int(t) for t in s1.timesteps]
    shape = (2, 4, 8, 8)
    assert Pipe._predraw_step_noise([s1, s2], ts, shape, gen(5), "cpu") is None  # eta defaults to 0: nothing to draw
    assert Pipe._predraw_step_noise([s1, s2], ts, shape, gen(5), "cpu", eta=0.0) is None
    g0 = gen(5)
    pre = Pipe._predraw_step_noise([s1, s2], ts, shape, g0, "cpu", eta=0.7)
    g = gen(5)
    for i in range(len(ts)):
        for k in range(2):
            assert torch.equal(pre[k][i], randn_tensor(shape, generator=g, device="cpu", dtype=torch.float32)), (i, k)
    assert torch.equal(g0.get_state(), g.get_state())


# ---------------------------------------------------------------------------------------------------------------------------
# config protocol
# ---------------------------------------------------------------------------------------------------------------------------
def test_config_protocol():
    from gm_diffusion.components import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, PNDMScheduler

    d = DDIMScheduler.from_config(DDPMScheduler(steps_offset=1, clip_sample=False, **SD).config)
    assert d.config.steps_offset == 1 and d.config.clip_sample is False and d.config.beta_schedule == "scaled_linear"
    assert d.config.set_alpha_to_one is True and "variance_type" not in d.config  # foreign keys are ignored, own defaults kept
    d = DDIMScheduler.from_config(PNDMScheduler(skip_prk_steps=True, steps_offset=1, **SD).config)
    assert d.config.set_alpha_to_one is False and "skip_prk_steps" not in d.config
    assert torch.equal(d.final_alpha_cumprod, d.alphas_cumprod[0])
    DPMSolverMultistepScheduler.from_config(d.config)  # and back
    d.set_timesteps(7)
    c = copy.deepcopy(d)
    g = gen(2)
    x, eps = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
    for t in d.timesteps.tolist():
        a = d.step(eps, t, x, eta=0.5, generator=gen(t)).prev_sample
        b = c.step(eps, t, x, eta=0.5, generator=gen(t)).prev_sample
        assert torch.equal(a, b)
    for bad in (dict(prediction_type="v_prediction"), dict(thresholding=True), dict(rescale_betas_zero_snr=True)):
        with pytest.raises(NotImplementedError):
            DDIMScheduler(**bad)
    with pytest.raises(TypeError):
        DDIMScheduler(variance_type="fixed_small")
    with pytest.raises(ValueError):
        DDIMScheduler().set_timesteps(1001)
    with pytest.raises(ValueError):
        DDIMScheduler().step(x, 0, x)  # set_timesteps not called


def test_pipeline_passes_eta_only_to_a_scheduler_that_takes_it():
    from gm_diffusion.components import DDPMScheduler, PNDMScheduler
    from gm_diffusion.pipelines import StableDiffusionGMPipeline as Pipe

    g = gen(0)
    pipe = Pipe.__new__(Pipe)
    pipe.scheduler = ddim(**SD)
    kw = pipe.prepare_extra_step_kwargs(g, 0.7)
    assert kw == {"eta": 0.7, "generator": g} and Pipe._fused_step_kwargs(kw) == {"generator": g, "eta": 0.7}
    pipe.scheduler = DDPMScheduler(**SD)
    kw = pipe.prepare_extra_step_kwargs(g, 0.7)
    assert kw == {"generator": g} and Pipe._fused_step_kwargs(kw) == {"generator": g}
    pipe.scheduler = PNDMScheduler(skip_prk_steps=True, **SD)
    kw = pipe.prepare_extra_step_kwargs(g, 0.7)
    assert kw == {} and Pipe._fused_step_kwargs(kw) == {}


# ---------------------------------------------------------------------------------------------------------------------------
# ABI without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_ddim_step_argument_validation_without_gpu():
    from gm_diffusion import _native as native

    lib = native.lib()
    assert lib.gmd_abi_version() == 14 and native.ABI_VERSION == 14
    one = 1  # any non-null address: validation happens before a launch, nothing is dereferenced
    nan = float("nan")

    def call(eps=one, x=one, noise=None, B=1, chw=16, ssa=0.9, ss1=0.43, clip=0, cr=0.0, uc=0, sp=0.95, dc=0.3, sd=0.0, sa=0.9, s1=0.43,
             xp=one, x0=None, p0=None):
        return lib.gmd_ddim_step(eps, x, noise, B, chw, 0, 1.0, None, 0.0, ssa, ss1, clip, cr, uc, sp, dc, sd, sa, s1, xp, x0, p0, None)

    for kw, word in ((dict(eps=None), b"null"), (dict(x=None), b"null"), (dict(xp=None), b"null"), (dict(B=-1), b"shape"),
                     (dict(chw=0), b"shape"), (dict(ssa=0.0), b"zero"), (dict(uc=1, ss1=0.0), b"zero"), (dict(x0=one, sa=0.0), b"zero"),
                     (dict(clip=1, cr=0.0), b"clip_range"), (dict(clip=1, cr=-1.0), b"clip_range"), (dict(clip=1, cr=nan), b"clip_range"),
                     (dict(dc=-0.1), b"dir_coeff"), (dict(dc=nan), b"dir_coeff"), (dict(sd=-0.1), b"std_dev"), (dict(sd=nan), b"std_dev")):
        assert call(**kw) == 1, kw  # GMD_ERR_INVALID
        assert word in lib.gmd_last_error(), (kw, lib.gmd_last_error())
    assert call(B=0, eps=None, x=None, xp=None) == 0  # an empty batch is a no-op


def test_ddim_step_refuses_host_tensors():
    from gm_diffusion import hip_ops
    from gm_diffusion._native import HipExtensionError

    assert "ddim_step" in hip_ops.__all__
    z = torch.zeros(1, 4, 8, 8)
    with pytest.raises(HipExtensionError):
        hip_ops.ddim_step(z, z, (0.9, 0.43, 0.95, 0.3, 0.0, 0.9, 0.43), False, 1.0)
