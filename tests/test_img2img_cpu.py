"""CPU: img2img / inpainting of the dual-UNet pipeline -- the schedulers' ``add_noise`` / ``add_noise_coefs`` / ``set_begin_index``
against diffusers' expressions restated in tests/img2img_ref.py (bit for bit), ``VaeImageProcessor.preprocess``, the mask
preparation, the keywords' validation, the generic loop against the reference loop, the exact identities, the accounting of UNet
evaluations and generator draws, and the C ABI of gmd_inpaint_blend (refusals return an error before any launch)."""
import numpy as np
import pytest
import torch

import ddim_ref as D
import img2img_ref as R
import small_ref as S
from oracle import fixtures

F32 = torch.float32
RMS_TOL = 1e-3  # north star: "within 1e-3 latent RMS"
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
STEPS = 8


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rms(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b) ** 2).mean().sqrt())


# =============================================================================================================================
# schedulers
# =============================================================================================================================
def _schedulers():
    """The ten schedulers: name -> (factory, family)."""
    from gm_diffusion import components as C

    return {
        "pndm": (lambda: C.PNDMScheduler(skip_prk_steps=True, steps_offset=1, **SD), "vp"),
        "ddpm": (lambda: C.DDPMScheduler(clip_sample=False, **SD), "vp"),
        "ddim": (lambda: C.DDIMScheduler(clip_sample=False, steps_offset=1, **SD), "vp"),
        "lcm": (lambda: C.LCMScheduler(), "vp"),
        "dpm": (lambda: C.DPMSolverMultistepScheduler(steps_offset=1, timestep_spacing="leading", **SD), "dpm"),
        "dpm_sde": (lambda: C.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++", **SD), "dpm"),
        "unipc": (lambda: C.UniPCMultistepScheduler(**SD), "dpm"),
        "euler": (lambda: C.EulerDiscreteScheduler(**SD), "sigma"),
        "euler_a": (lambda: C.EulerAncestralDiscreteScheduler(**SD), "sigma"),
        "lms": (lambda: C.LMSDiscreteScheduler(**SD), "sigma"),
    }


SCHEDULERS = ["pndm", "ddpm", "ddim", "lcm", "dpm", "dpm_sde", "unipc", "euler", "euler_a", "lms"]


def _ref_add_noise(s, family, x, noise, timesteps, index):
    if family == "vp":
        return R.add_noise_vp(s.alphas_cumprod, x, noise, timesteps)
    fn = R.add_noise_dpm if family == "dpm" else R.add_noise_sigma
    return fn(s.sigmas, x, noise, [index] * len(timesteps))


def _check_add_noise(s, family, t, index, what):
    """add_noise at timestep ``t`` (expected table entry ``index``) for one timestep and for one per sample; the coefficient pair
    reproduces it bit for bit as ca * x + cb * noise; in sigma space that is x + noise * sigma itself."""
    g = gen(3)
    x, noise = torch.randn(2, 4, 5, 3, generator=g), torch.randn(2, 4, 5, 3, generator=g)
    for ts in (torch.tensor([t]), torch.tensor([t, t])):
        S.assert_bit_equal(s.add_noise(x, noise, ts), _ref_add_noise(s, family, x, noise, ts, index), f"{what} add_noise {tuple(ts.shape)}")
    ca, cb = s.add_noise_coefs(t)
    assert isinstance(ca, float) and isinstance(cb, float) and ca == float(np.float32(ca)) and cb == float(np.float32(cb))
    ref = _ref_add_noise(s, family, x, noise, torch.tensor([t]), index)
    S.assert_bit_equal(R._s(ca) * x + R._s(cb) * noise, ref, f"{what} ca * x + cb * noise")
    if family == "sigma":
        assert ca == 1.0
        S.assert_bit_equal(ref, x + noise * s.sigmas[index], f"{what} x + noise * sigma")


@pytest.mark.parametrize("name", SCHEDULERS)
def test_add_noise_and_coefs_equal_diffusers_expressions(name):
    make, family = _schedulers()[name]
    s = make()
    s.set_timesteps(STEPS)
    sched = s.timesteps.tolist()
    stepper = family != "vp" or name == "lcm"
    assert hasattr(s, "set_begin_index") == stepper, "set_begin_index where diffusers has it: the step-index classes"
    # (1) no index set: the timestep is looked up
    k = 3
    _check_add_noise(s, family, s.timesteps[k], R.noise_index(sched, sched[k], None, None), f"{name} no index")
    if not stepper:
        return
    assert s.begin_index is None and s.step_index is None
    # (2) at a begin index, before the first step: the begin index, whatever timestep is named
    s.set_begin_index(2)
    assert s.begin_index == 2
    _check_add_noise(s, family, s.timesteps[5], 2, f"{name} begin index")
    # (3) after a step: the step index (the inpaint re-noise to the next level)
    g = gen(4)
    x, eps = torch.randn(1, 4, 5, 3, generator=g), torch.randn(1, 4, 5, 3, generator=g)
    s.step(eps, s.timesteps[2], x, **({"generator": g} if name in ("lcm", "dpm_sde", "euler_a") else {}))
    assert s.step_index == 3
    _check_add_noise(s, family, s.timesteps[3], 3, f"{name} after a step")
    # set_timesteps forgets the begin index, as in diffusers
    s.set_timesteps(STEPS)
    assert s.begin_index is None and s.step_index is None


@pytest.mark.parametrize("name", ["lcm", "dpm", "unipc", "euler", "euler_a", "lms"])
def test_set_begin_index_selects_the_first_step(name):
    """With a begin index the first ``step`` runs at that index even when the timestep names another entry; without one the timestep
    is looked up.  Both against a twin that reaches the same index by its timestep."""
    make, family = _schedulers()[name]
    g = gen(9)
    x, eps = torch.randn(1, 4, 5, 3, generator=g), torch.randn(1, 4, 5, 3, generator=g)
    a, b = make(), make()
    a.set_timesteps(STEPS)
    b.set_timesteps(STEPS)
    kw = lambda: {"generator": gen(1)} if name in ("lcm", "euler_a") else {}
    a.set_begin_index(3)
    t_named = a.timesteps[3] if name == "lcm" else a.timesteps[0]  # LCM reads alphas_cumprod[timestep] too: name the same one
    out_a = a.step(eps, t_named, x, **kw(), return_dict=False)[0]
    out_b = b.step(eps, b.timesteps[3], x, **kw(), return_dict=False)[0]
    assert a.step_index == b.step_index == 4
    S.assert_bit_equal(out_a, out_b, f"{name}: first step at the begin index")
    if family == "sigma":  # scale_model_input fixes the index first in the pipelines' loops: the begin index there too
        c = make()
        c.set_timesteps(STEPS)
        c.set_begin_index(3)
        S.assert_bit_equal(c.scale_model_input(x, c.timesteps[0]), x / ((c.sigmas[3] ** 2 + 1) ** 0.5), f"{name}: scale_model_input")
        assert c.step_index == 3


# =============================================================================================================================
# input preparation
# =============================================================================================================================
def test_preprocess_normalises_and_lays_out_nchw_only():
    from gm_diffusion.components import VaeImageProcessor

    p = VaeImageProcessor(vae_scale_factor=8)
    g = gen(2)
    u8 = torch.randint(0, 256, (2, 16, 24, 3), generator=g, dtype=torch.uint8)
    want = 2.0 * (u8.permute(0, 3, 1, 2).float() / 255.0) - 1.0
    for given in (u8, u8.numpy(), [u8[0].numpy(), u8[1]]):
        got = p.preprocess(given, 16, 24)
        assert got.dtype == F32 and got.is_contiguous() and torch.equal(got, want)
    assert torch.equal(p.preprocess(u8[0], 16, 24), want[:1])
    fl = torch.rand(2, 3, 16, 24, generator=g)
    assert torch.equal(p.preprocess(fl, 16, 24), 2.0 * fl - 1.0) and torch.equal(p.preprocess(fl[1], 16, 24), 2.0 * fl[1:] - 1.0)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        pil = Image.fromarray(u8[0].numpy())
        assert torch.equal(p.preprocess(pil, 16, 24), want[:1]) and torch.equal(p.preprocess([pil, pil], 16, 24), want[[0, 0]])
    with pytest.raises(ValueError, match="prepare_sdr"):
        p.preprocess(u8, 24, 16)
    with pytest.raises(ValueError, match="prepare_sdr"):
        p.preprocess(fl, 32, 48)
    with pytest.raises(ValueError):
        p.preprocess(torch.rand(2, 5, 16, 24), 16, 24)
    with pytest.raises(ValueError):
        p.preprocess(np.zeros((16, 24, 3), np.float64), 16, 24)


def test_mask_preparation_is_diffusers_binarise_then_nearest():
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline as P

    g = gen(6)
    m = torch.rand(2, 1, 64, 48, generator=g)
    want = torch.nn.functional.interpolate((m >= 0.5).float(), size=(8, 6))
    assert torch.equal(P._prepare_inpaint_mask(m, 64, 48, 8, 6, 2, "cpu"), want)
    assert torch.equal(P._prepare_inpaint_mask(m[0, 0], 64, 48, 8, 6, 2, "cpu"), want[:1])
    u8 = (m[:1] * 255).round().to(torch.uint8)
    want_u8 = torch.nn.functional.interpolate((u8.float() / 255.0 >= 0.5).float(), size=(8, 6))
    assert torch.equal(P._prepare_inpaint_mask(u8, 64, 48, 8, 6, 2, "cpu"), want_u8)
    assert torch.equal(P._prepare_inpaint_mask(u8[0, 0].numpy(), 64, 48, 8, 6, 2, "cpu"), want_u8)
    try:
        from PIL import Image

        assert torch.equal(P._prepare_inpaint_mask(Image.fromarray(u8[0, 0].numpy()), 64, 48, 8, 6, 2, "cpu"), want_u8)
    except ImportError:
        pass
    lat = torch.rand(2, 1, 8, 6, generator=g)  # a latent-size float mask is taken as it is: fractional values stay
    assert torch.equal(P._prepare_inpaint_mask(lat, 64, 48, 8, 6, 2, "cpu"), lat)
    for bad in (torch.rand(3, 1, 64, 48), torch.rand(2, 2, 64, 48), torch.rand(2, 1, 32, 48), torch.zeros(64, 48, dtype=torch.int32)):
        with pytest.raises(ValueError, match="mask_image"):
            P._prepare_inpaint_mask(bad, 64, 48, 8, 6, 2, "cpu")


# =============================================================================================================================
# the pipeline's generic loop over the oracle UNets (duck-typed components on the CPU)
# =============================================================================================================================
class FakeVae:
    """A VAE by duck typing: ``encode(x).latent_dist.sample(generator)`` draws one tensor of the latents' shape, as the real one."""

    class config:
        block_out_channels = [1, 2, 3, 4]
        scaling_factor = 0.18215

    def encode(self, x):
        from gm_diffusion.components.image_processor import randn_tensor

        mean = torch.nn.functional.avg_pool2d(x, 8)
        mean = torch.cat([mean, mean[:, :1]], 1)

        class Dist:
            def sample(self, generator=None):
                return mean + 0.1 * randn_tensor(mean.shape, generator=generator, device=mean.device, dtype=mean.dtype)

        return type("Out", (), {"latent_dist": Dist()})()


def _hip_scheduler(kind, eta=0.0):
    from gm_diffusion import components as C

    if kind == "pndm":
        return C.PNDMScheduler(skip_prk_steps=True, steps_offset=1, **SD)
    if kind == "ddim":
        return C.DDIMScheduler(clip_sample=False, steps_offset=1, **SD)
    if kind == "euler":
        return C.EulerDiscreteScheduler(**SD)
    return C.DPMSolverMultistepScheduler(steps_offset=1, timestep_spacing="leading", **SD)


def _ref_scheduler(kind):
    import euler_ref as E
    from oracle import schedulers as OS

    if kind == "pndm":
        return OS.PNDMScheduler()
    if kind == "ddim":
        return D.RefDDIMScheduler(eta=0.7)
    if kind == "euler":
        return E.RefEulerScheduler()
    return OS.DPMSolverMultistepScheduler()


ETA = {"pndm": 0.0, "ddim": 0.7, "euler": 0.0, "dpm": 0.0}


@pytest.fixture(scope="module")
def case():
    """Inputs shared by the pipeline tests, drawn once and left unchanged: embeddings, the picture's latents z0, the noise, the
    per-sample masks; the oracle UNets; a pipeline over them."""
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline

    pe, ne, noise = fixtures.make_inputs(2, 16, 16, cross_dim=64)
    z0 = 0.8 * torch.randn(2, 4, 16, 16, generator=gen(55))
    u4, u8 = fixtures.build_unet("tiny", 4), fixtures.build_unet("tiny", 8)
    pipe = StableDiffusionDualUNetPipeline(vae=FakeVae(), text_encoder=None, tokenizer=None, unet=u4, gm_unet=u8, scheduler=_hip_scheduler("pndm"),
                                           safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    return dict(pe=pe, ne=ne, noise=noise, z0=z0, mask=R.masks(2, 16, 16), u4=u4, u8=u8, pipe=pipe)


def _run(case, kind, generator=None, **kw):
    pipe = case["pipe"]
    pipe.scheduler = _hip_scheduler(kind)
    kw.setdefault("latents", case["noise"])
    return pipe(prompt_embeds=case["pe"], negative_prompt_embeds=case["ne"], height=128, width=128, num_inference_steps=STEPS,
                guidance_scale=7.5, eta=ETA[kind], generator=generator, output_type="latent", **kw)


REF_CASES = [(0.5, False), (0.5, True), (1.0, True)]  # (strength, with a mask)


@pytest.mark.parametrize("strength,masked", REF_CASES)
@pytest.mark.parametrize("kind", ["pndm", "ddim", "dpm"])
def test_generic_loop_matches_reference_loop(case, kind, strength, masked):
    """Both final latents within RMS_TOL of the reference loop (float64 steps where the reference scheduler has them).  On the parent
    commit the keywords are ignored and the strength 0.5 cases miss by O(1)."""
    mask = case["mask"] if masked else None
    rs, rg = R.dual_img2img_loop(case["u4"], case["u8"], _ref_scheduler(kind), case["pe"], case["ne"], case["z0"], case["noise"], STEPS,
                                 strength, mask=mask, generator=gen(123))
    s, g = _run(case, kind, gen(123), image=case["z0"], strength=strength, **({"mask_image": mask} if masked else {}))
    print(f"{kind} strength={strength} masked={masked}: latent RMS sdr={rms(s, rs):.2e} gm={rms(g, rg):.2e}")
    assert rms(s, rs) <= RMS_TOL and rms(g, rg) <= RMS_TOL


def test_generic_loop_still_refuses_sigma_space(case):
    with pytest.raises(ValueError, match="sigma-space"):
        _run(case, "euler", image=case["z0"], strength=0.5)


@pytest.mark.parametrize("kind", ["pndm", "ddim", "dpm"])
def test_identities(case, kind):
    """m == 1 at strength 1 with the picture given as latents: both latents equal the plain call's with the same generator (the picture
    never enters).  m == 0: the final SDR latents are z0.  torch.equal equates +0 and -0."""
    ones, zeros = torch.ones(1, 1, 16, 16), torch.zeros(2, 1, 16, 16)
    for latents in (case["noise"], None):  # given noise, and noise drawn from the generator where the plain call draws its latents
        plain = _run(case, kind, gen(5), latents=latents)
        s, g = _run(case, kind, gen(5), latents=latents, image=case["z0"], mask_image=ones, strength=1.0)
        assert torch.equal(s, plain[0]) and torch.equal(g, plain[1])
    for strength in (1.0, 0.5):
        s, g = _run(case, kind, gen(5), image=case["z0"], mask_image=zeros, strength=strength)
        assert torch.equal(s, case["z0"])


def _count_forwards(case):
    counts = {"sdr": 0, "gm": 0}
    hooks = [case["u4"].register_forward_hook(lambda *a: counts.__setitem__("sdr", counts["sdr"] + 1)),
             case["u8"].register_forward_hook(lambda *a: counts.__setitem__("gm", counts["gm"] + 1))]
    return counts, hooks


@pytest.mark.parametrize("kind", ["pndm", "ddim", "dpm"])
@pytest.mark.parametrize("strength", [0.3, 0.5, 1.0])
def test_unet_evaluations(case, kind, strength):
    """SDR evaluations = len(timesteps) - t_start * order, GM evaluations = len(timesteps): N - t_start and N, except that PNDM's
    schedule holds N + 1 timesteps (its second one twice), of which diffusers' slicing drops t_start as well."""
    counts, hooks = _count_forwards(case)
    try:
        _run(case, kind, gen(1), image=case["z0"], strength=strength)
    finally:
        for h in hooks:
            h.remove()
    n = STEPS + (1 if kind == "pndm" else 0)
    t_start = R.get_t_start(STEPS, strength)
    assert t_start == {0.3: 6, 0.5: 4, 1.0: 0}[strength]
    assert counts == {"sdr": n - t_start, "gm": n}
    ref = {}
    R.dual_img2img_loop(case["u4"], case["u8"], _ref_scheduler(kind), case["pe"], case["ne"], case["z0"], case["noise"], STEPS, strength, count=ref)
    assert ref == counts


@pytest.mark.parametrize("pixels", [False, True])
def test_generator_is_advanced_by_the_documented_draws(case, pixels):
    """DDIM at eta = 0.7 draws at every step of either scheduler.  Order: the encoder's sample (pixels only), the noise, then per
    iteration GM alone until the SDR branch enters and SDR + GM afterwards: 1 (+ 1) + t_start + 2 (N - t_start) draws of the latents'
    shape.  The draws' order is checked through the values: the GM latents of a run whose generator is re-seeded equal a run with
    the noise passed in and a generator advanced past the encoder's and the noise's draws."""
    image = torch.rand(2, 3, 128, 128, generator=gen(8)) if pixels else case["z0"]  # one picture per row: a draw of the latents' shape
    g, twin = gen(31), gen(31)
    s, gm = _run(case, "ddim", g, latents=None, image=image, strength=0.5)
    t_start = R.get_t_start(STEPS, 0.5)
    shape = case["noise"].shape
    first = [torch.randn(shape, generator=twin) for _ in range(2 if pixels else 1)]
    mid = twin.get_state()
    for _ in range(t_start + 2 * (STEPS - t_start)):
        torch.randn(shape, generator=twin)
    assert torch.equal(g.get_state(), twin.get_state())
    if not pixels:  # the same run with the noise handed over: the steps' draws start where `mid` stands
        g2 = gen(0)
        g2.set_state(mid)
        s2, gm2 = _run(case, "ddim", g2, latents=first[0], image=image, strength=0.5)
        assert torch.equal(s2, s) and torch.equal(gm2, gm)


def test_one_image_is_repeated_and_pixels_are_encoded(case):
    """[1, 3, H, W] pixels for two rows: encoded once (one draw of [1, 4, h, w]), scaled and repeated: z0 shows at m == 0."""
    image = torch.rand(1, 3, 128, 128, generator=gen(8))
    x = 2.0 * image - 1.0
    want = (FakeVae().encode(x).latent_dist.sample(gen(77)) * FakeVae.config.scaling_factor).expand(2, -1, -1, -1)
    s, _ = _run(case, "pndm", gen(77), image=image, mask_image=torch.zeros(128, 128), strength=0.5)
    assert torch.equal(s, want)
    u8 = (image[0].permute(1, 2, 0) * 255).round().to(torch.uint8)
    want = (FakeVae().encode(2.0 * (u8.permute(2, 0, 1)[None].float() / 255.0) - 1.0).latent_dist.sample(gen(77))
            * FakeVae.config.scaling_factor).expand(2, -1, -1, -1)
    s, _ = _run(case, "pndm", gen(77), image=u8.numpy(), mask_image=torch.zeros(128, 128, dtype=torch.uint8), strength=0.5)
    assert torch.equal(s, want)


def test_keyword_validation(case):
    z0 = case["z0"]
    with pytest.raises(ValueError, match="image"):
        _run(case, "pndm", mask_image=case["mask"])
    with pytest.raises(ValueError, match="image"):
        _run(case, "pndm", strength=0.5)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="strength"):
            _run(case, "pndm", image=z0, strength=bad)
    with pytest.raises(ValueError, match="< 1"):
        _run(case, "pndm", image=z0, strength=0.1)  # int(8 * 0.1) == 0
    with pytest.raises(ValueError, match="prepare_sdr"):
        _run(case, "pndm", image=torch.rand(1, 3, 64, 64))
    with pytest.raises(ValueError, match="latents of shape"):
        _run(case, "pndm", image=torch.rand(1, 4, 8, 8))
    with pytest.raises(ValueError, match="mask_image"):
        _run(case, "pndm", image=z0, mask_image=torch.rand(3, 1, 16, 16))
    for key in ("padding_mask_crop", "masked_image_latents"):
        with pytest.raises(NotImplementedError, match=key):
            _run(case, "pndm", image=z0, mask_image=case["mask"], **{key: 32})
    pipe = case["pipe"]
    old = pipe.unet.config.in_channels
    try:
        pipe.unet.config.in_channels = 9
        with pytest.raises(NotImplementedError, match="in_channels == 9"):
            _run(case, "pndm", image=z0, mask_image=case["mask"])
    finally:
        pipe.unet.config.in_channels = old


def test_defaults_of_strength(case):
    """0.8 without a mask, 1.0 with one (diffusers' two defaults)."""
    a = _run(case, "ddim", gen(2), image=case["z0"])
    b = _run(case, "ddim", gen(2), image=case["z0"], strength=0.8)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a = _run(case, "ddim", gen(2), image=case["z0"], mask_image=case["mask"])
    b = _run(case, "ddim", gen(2), image=case["z0"], mask_image=case["mask"], strength=1.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_lcm_takes_the_strength_in_set_timesteps(case):
    """Nothing is sliced: the schedule is the one LCMScheduler builds for the strength, and both UNets run at every step."""
    from gm_diffusion.components import LCMScheduler

    pipe = case["pipe"]
    pipe.scheduler = LCMScheduler()
    twin = LCMScheduler()
    twin.set_timesteps(4, strength=0.5)
    counts, hooks = _count_forwards(case)
    try:
        pipe(prompt_embeds=case["pe"], negative_prompt_embeds=case["ne"], height=128, width=128, num_inference_steps=4, guidance_scale=7.5,
             generator=gen(1), output_type="latent", image=case["z0"], strength=0.5)
    finally:
        for h in hooks:
            h.remove()
    assert torch.equal(pipe.scheduler.timesteps, twin.timesteps) and int(twin.timesteps[0]) < 500
    assert counts == {"sdr": 4, "gm": 4}


def test_plain_call_never_reaches_the_blend(case, monkeypatch):
    from gm_diffusion import hip_ops

    before = _run(case, "pndm")

    def boom(*a, **k):
        raise AssertionError("inpaint_blend reached without `image`")

    monkeypatch.setattr(hip_ops, "inpaint_blend", boom)
    after = _run(case, "pndm")
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


def test_predraw_order_gm_alone_then_sdr_before_gm():
    """``_predraw_step_noise(first=...)``: the slots are drawn in the loop's order -- per iteration the schedulers that step there."""
    from gm_diffusion.components import DDIMScheduler
    from gm_diffusion.pipelines import StableDiffusionGMPipeline as Base

    s = [DDIMScheduler(**SD), DDIMScheduler(**SD)]
    ts, shape = [10, 7, 4, 1], (1, 2, 3)
    pre = Base._predraw_step_noise(s, ts, shape, gen(4), "cpu", eta=0.5, first=(2, 0))
    twin = gen(4)
    order = [(0, 1), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1)]
    for i, k in order:
        assert torch.equal(pre[k][i], torch.randn(shape, generator=twin)), (i, k)
    assert pre[0][0] is None and pre[0][1] is None
    old = Base._predraw_step_noise(s, ts, shape, gen(4), "cpu", eta=0.5)
    both = Base._predraw_step_noise(s, ts, shape, gen(4), "cpu", eta=0.5, first=(0, 0))
    assert all(torch.equal(a, b) for ra, rb in zip(old, both) for a, b in zip(ra, rb))


# =============================================================================================================================
# the C ABI
# =============================================================================================================================
@pytest.fixture(scope="module")
def native():
    import os

    from gm_diffusion import _native

    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _native


def test_abi_of_inpaint_blend(native):
    import ctypes

    lib = native.lib()
    assert hasattr(lib, "gmd_inpaint_blend") and lib.gmd_abi_version() == 14 == native.ABI_VERSION
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert native.SIGNATURES["gmd_inpaint_blend"] == [P, P, P, P, P, I, I, L, I, F, F, P]


def test_inpaint_blend_refusals_return_an_error_without_launching(native):
    """Every refusal comes back as GMD_ERR_INVALID from the host checks: the pointers are never dereferenced (they are not memory)."""
    lib = native.lib()
    p = 4096  # stands for a non-null device pointer
    ok = (p, p, p, p, p, 2, 4, 15, 2, 0.5, 0.5, None)
    cases = {
        "null z0": (p, p, p, None, p, 2, 4, 15, 2, 0.5, 0.5, None),
        "both outputs": (None, None, p, p, p, 2, 4, 15, 2, 0.5, 0.5, None),
        "x0 is blended by the mask": (p, p, None, p, p, 2, 4, 15, 1, 0.5, 0.5, None),
        "mask_rows": (p, p, p, p, p, 2, 4, 15, 3, 0.5, 0.5, None),
        "negative": (p, p, p, p, p, -1, 4, 15, 1, 0.5, 0.5, None),
    }
    for what, args in cases.items():
        assert lib.gmd_inpaint_blend(*args) == 1, what
        assert what.encode() in lib.gmd_last_error(), (what, lib.gmd_last_error())
    assert lib.gmd_inpaint_blend(p, p, p, p, p, 2, 4, 15, 0, 0.5, 0.5, None) == 1  # mask_rows 0
    for empty in ((0, 4, 15), (2, 0, 15), (2, 4, 0)):  # nothing to do: GMD_OK before any pointer is looked at
        assert lib.gmd_inpaint_blend(None, None, None, None, None, *empty, 1, 0.5, 0.5, None) == 0
    assert len(ok) == len(native.SIGNATURES["gmd_inpaint_blend"])


def test_hip_op_refuses_host_tensors_and_bad_shapes():
    from gm_diffusion import hip_ops
    from gm_diffusion._native import HipExtensionError

    z = torch.zeros(1, 4, 8, 8)
    with pytest.raises(HipExtensionError):
        hip_ops.inpaint_blend(z, x_prev=z.clone())
