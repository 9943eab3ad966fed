"""CPU: the few-step (LCM) path without a GPU -- LCMScheduler's timestep tables, errors, noise draws and config protocol, its host step
against the plain torch step of tests/lcm_ref.py, the guidance-scale embedding against its formula in float64, the yardstick's own
forward against the stock oracle, the UNet's key surface with ``time_cond_proj_dim``, the generic pipelines with duck-typed oracle
UNets, and the argument validation of the two new entry points."""
import copy
import math

import pytest
import torch

import lcm_ref as L

SHAPE = (2, 4, 8, 8)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def lcm(**kw):
    from gm_diffusion.components import LCMScheduler

    return LCMScheduler(**kw)


class FakeVae:
    class config:
        block_out_channels = [1, 2, 3, 4]
        scaling_factor = 0.18215


# ---------------------------------------------------------------------------------------------------------------------------
# schedule
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kw,want", [(4, {}, [999, 759, 499, 259]), (8, {}, [999, 879, 759, 639, 499, 379, 259, 139]), (2, {}, [999, 499]),
                                       (1, {}, [999]), (4, dict(strength=0.5), [499, 379, 259, 139])])
def test_timestep_tables_known_answers(n, kw, want):
    s = lcm()
    s.set_timesteps(n, **kw)
    assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == want and s.num_inference_steps == n
    assert s.order == 1 and s.init_noise_sigma == 1.0 and s.step_index is None
    if not kw:
        r = L.RefLCMScheduler()
        r.set_timesteps(n)
        assert r.timesteps.tolist() == want


def test_set_timesteps_errors():
    s = lcm()
    with pytest.raises(ValueError):
        s.set_timesteps()  # neither
    with pytest.raises(ValueError):
        s.set_timesteps(4, timesteps=[999, 499])  # both
    with pytest.raises(ValueError, match="original_inference_steps"):
        s.set_timesteps(51)  # num_inference_steps > O
    with pytest.raises(ValueError):
        s.set_timesteps(4, original_inference_steps=1001)  # O > num_train_timesteps
    with pytest.raises(ValueError, match="strength"):
        s.set_timesteps(30, strength=0.5)  # len(origin) // n < 1
    with pytest.raises(ValueError, match="descending"):
        s.set_timesteps(timesteps=[499, 999])
    with pytest.raises(ValueError, match="descending"):
        s.set_timesteps(timesteps=[999, 499, 499])  # strictly
    with pytest.raises(ValueError):
        s.set_timesteps(timesteps=[1000, 499])  # below num_train_timesteps
    with pytest.raises(ValueError):
        lcm().step(torch.zeros(SHAPE), 999, torch.zeros(SHAPE))  # set_timesteps not called
    assert lcm(original_inference_steps=20).set_timesteps(20) is None  # n == O is allowed
    s.set_timesteps(4, original_inference_steps=100)
    assert s.timesteps.tolist() == [999, 749, 499, 249]


def test_custom_timesteps():
    s = lcm()
    s.set_timesteps(timesteps=[900, 500, 37, 0])
    assert s.timesteps.tolist() == [900, 500, 37, 0] and s.num_inference_steps == 4 and s.timesteps.dtype == torch.int64
    assert [s.draws_noise(t) for t in (900, 500, 37, 0)] == [True, True, True, False]
    g = gen(1)
    x, eps = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
    for i, t in enumerate([900, 500, 37, 0]):
        out = s.step(eps, t, x, generator=gen(3))
        nxt = [500, 37, 0, 0][i]
        a_t, a_p = s.alphas_cumprod[t], s.alphas_cumprod[nxt]
        sc = t * 10.0
        coefs = (a_t ** 0.5, (1 - a_t) ** 0.5, 0.25 / (sc * sc + 0.25), sc / (sc * sc + 0.25) ** 0.5, a_p ** 0.5, (1 - a_p) ** 0.5, 1.0, 0.0)
        noise = torch.randn(SHAPE, generator=gen(3)) if i < 3 else None
        prev, _, den = L.lcm_step_f32(eps, x, coefs, noise=noise)
        assert torch.equal(out.prev_sample, prev) and torch.equal(out.denoised, den) and s.step_index == i + 1


# ---------------------------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_host_step_equals_the_plain_torch_step_and_draws_n_minus_1(n):
    """Whole trajectories of ``step`` on host tensors against RefLCMScheduler (written from the specification), bit for bit, with a CPU
    generator advanced n - 1 times; the last step's prev_sample is the denoised sample."""
    s, r = lcm(), L.RefLCMScheduler()
    s.set_timesteps(n)
    r.set_timesteps(n)
    g = gen(n)
    x = torch.randn(SHAPE, generator=g)
    xr = x.clone()
    gs, gr, twin = gen(50), gen(50), gen(50)
    for i, t in enumerate(s.timesteps):
        assert s.draws_noise(t) == (i < n - 1)
        eps = torch.randn(SHAPE, generator=g)
        out = s.step(eps, t, x, generator=gs)
        ref = r.step(eps, t, xr, generator=gr)
        assert torch.equal(out.prev_sample, ref[0]) and torch.equal(out.denoised, ref[1]), i
        if i == n - 1:
            assert torch.equal(out.prev_sample, out.denoised)
        else:
            assert not torch.equal(out.prev_sample, out.denoised)
        x, xr = out.prev_sample, ref[0]
        assert s.step_index == i + 1
    for _ in range(n - 1):
        torch.randn(SHAPE, generator=twin)
    assert torch.equal(gs.get_state(), twin.get_state()), "n steps take n - 1 draws"
    tup = lcm()
    tup.set_timesteps(n)
    assert isinstance(tup.step(eps, tup.timesteps[0], x, generator=gen(0), return_dict=False), tuple)


def test_noise_argument_replaces_the_draw_and_leaves_the_generator():
    s, s2 = lcm(), lcm()
    s.set_timesteps(4)
    s2.set_timesteps(4)
    g = gen(0)
    x, eps, nz = (torch.randn(SHAPE, generator=g) for _ in range(3))
    g1 = gen(7)
    before = g1.get_state()
    a = s.step(eps, 999, x, generator=g1, noise=nz).prev_sample
    assert torch.equal(g1.get_state(), before)
    a_t, a_p = s.alphas_cumprod[999], s.alphas_cumprod[759]
    den = s2.step(eps, 999, x, generator=gen(7)).denoised
    assert torch.equal(a, a_p ** 0.5 * den + (1 - a_p) ** 0.5 * nz)
    assert float(a_t) < float(a_p)


def test_predrawn_noise_is_shared_sdr_before_gm():
    """_predraw_step_noise with two LCM schedulers: a slot per (step, scheduler) at every step but the last, SDR before GM."""
    from gm_diffusion.components.image_processor import randn_tensor
    from gm_diffusion.pipelines import StableDiffusionGMPipeline as Pipe

    s1 = lcm()
    s1.set_timesteps(4)
    s2 = copy.deepcopy(s1)
    ts = s1.timesteps.tolist()
    g0 = gen(5)
    pre = Pipe._predraw_step_noise([s1, s2], ts, SHAPE, g0, "cpu")
    g = gen(5)
    for i in range(4):
        for k in range(2):
            if i == 3:
                assert pre[k][i] is None
            else:
                assert torch.equal(pre[k][i], randn_tensor(SHAPE, generator=g, device="cpu", dtype=torch.float32)), (i, k)
    assert torch.equal(g0.get_state(), g.get_state())
    s1.set_timesteps(1)
    assert Pipe._predraw_step_noise([s1], [999], SHAPE, gen(5), "cpu") is None  # one step: nothing to draw


def test_boundary_scalings():
    s = lcm()
    assert s.get_scalings_for_boundary_condition_discrete(0) == (1.0, 0.0)
    cs, co = s.get_scalings_for_boundary_condition_discrete(999)
    assert cs == 0.25 / (9990.0 ** 2 + 0.25) and co == 9990.0 / (9990.0 ** 2 + 0.25) ** 0.5
    # at t = 0 the step returns its input: c_skip = 1, c_out = 0 (0 * p0 + 1 * x)
    s.set_timesteps(timesteps=[0])
    g = gen(2)
    x, eps = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
    assert torch.equal(s.step(eps, 0, x).prev_sample, 0.0 * ((x - (1 - s.alphas_cumprod[0]) ** 0.5 * eps) / s.alphas_cumprod[0] ** 0.5) + x)


def test_clip_sample_clamps_the_x0_prediction():
    s, p = lcm(clip_sample=True, clip_sample_range=0.5), lcm()
    for q in (s, p):
        q.set_timesteps(2)
    g = gen(4)
    x, eps = torch.randn(SHAPE, generator=g) * 3, torch.randn(SHAPE, generator=g)
    a_t = s.alphas_cumprod[999]
    p0 = ((x - (1 - a_t) ** 0.5 * eps) / a_t ** 0.5).clamp(-0.5, 0.5)
    cs, co = (torch.tensor(v, dtype=torch.float32) for v in s.get_scalings_for_boundary_condition_discrete(999))
    assert torch.equal(s.step(eps, 999, x, generator=gen(1)).denoised, co * p0 + cs * x)
    assert not torch.equal(p.step(eps, 999, x, generator=gen(1)).denoised, co * p0 + cs * x)


def test_config_protocol():
    from gm_diffusion.components import DDIMScheduler, LCMScheduler, PNDMScheduler
    from gm_diffusion.pipelines.pipeline_utils import DiffusionPipeline  # noqa: F401  (the scheduler table lives beside it)
    from gm_diffusion.pipelines import pipeline_utils

    want = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", trained_betas=None,
                original_inference_steps=50, clip_sample=False, clip_sample_range=1.0, set_alpha_to_one=True, steps_offset=0,
                prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0,
                timestep_spacing="leading", timestep_scaling=10.0, rescale_betas_zero_snr=False)
    s = LCMScheduler()
    assert {k: s.config[k] for k in want} == want
    assert float(s.final_alpha_cumprod) == 1.0 and torch.equal(LCMScheduler(set_alpha_to_one=False).final_alpha_cumprod, s.alphas_cumprod[0])
    d = LCMScheduler.from_config(PNDMScheduler(skip_prk_steps=True, steps_offset=1, beta_start=0.0001, beta_end=0.02, beta_schedule="linear").config)
    assert d.config.beta_schedule == "linear" and d.config.steps_offset == 1 and "skip_prk_steps" not in d.config
    assert d.config.original_inference_steps == 50
    DDIMScheduler.from_config(d.config)  # and back
    assert any(v is LCMScheduler for v in vars(pipeline_utils).values() if isinstance(v, type))
    assert any(isinstance(v, dict) and v.get("LCMScheduler") is LCMScheduler for v in vars(pipeline_utils).values())
    s.set_timesteps(4)
    c = copy.deepcopy(s)
    g = gen(2)
    x, eps = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
    for i, t in enumerate(s.timesteps.tolist()):
        a, b = s.step(eps, t, x, generator=gen(t)).prev_sample, c.step(eps, t, x, generator=gen(t)).prev_sample
        assert torch.equal(a, b) and c.step_index == s.step_index == i + 1
    for bad in (dict(prediction_type="v_prediction"), dict(prediction_type="sample"), dict(thresholding=True), dict(rescale_betas_zero_snr=True)):
        with pytest.raises(NotImplementedError):
            LCMScheduler(**bad)
    with pytest.raises(TypeError):
        LCMScheduler(variance_type="fixed_small")


# ---------------------------------------------------------------------------------------------------------------------------
# the guidance-scale embedding
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [32, 256, 33, 7])
def test_guidance_scale_embedding_against_the_formula_in_float64(dim):
    """Bound: the float32 argument 1000 w f_i carries a few roundings (w * 1000, the frequency's exp, the product): at most 4 ulp of an
    argument below 1000 * 6.5, i.e. 4 * 2^-24 * 6500 = 1.6e-3 in the angle and so in sin / cos, plus their own rounding."""
    from gm_diffusion.pipelines import StableDiffusionGMPipeline as Pipe

    pipe = Pipe.__new__(Pipe)
    w = torch.tensor([6.5, 0.0, 1.25])
    got = pipe.get_guidance_scale_embedding(w, embedding_dim=dim)
    half = dim // 2
    assert got.shape == (3, dim) and got.dtype == torch.float32
    i = torch.arange(half, dtype=torch.float64)
    arg = 1000.0 * w.double()[:, None] * torch.exp(-math.log(10000.0) * i / (half - 1))[None, :]
    ref = torch.cat([arg.sin(), arg.cos()], dim=1)
    tol = 4 * 2.0 ** -24 * 6500.0 + 2.0 ** -23
    assert float((got[:, :2 * half].double() - ref).abs().max()) <= tol
    if dim % 2:
        assert bool((got[:, -1] == 0).all())
    assert torch.equal(got[1, :half], torch.zeros(half)) and torch.equal(got[1, half:2 * half], torch.ones(half))  # w = 0: sin 0, cos 0
    assert torch.equal(got, L.guidance_embedding(w, dim))
    assert pipe.get_guidance_scale_embedding(w, embedding_dim=dim, dtype=torch.float64).dtype == torch.float64
    with pytest.raises(ValueError):
        pipe.get_guidance_scale_embedding(w[None], embedding_dim=dim)


# ---------------------------------------------------------------------------------------------------------------------------
# the yardstick's forward, and the UNet's key surface
# ---------------------------------------------------------------------------------------------------------------------------
def test_lcm_ref_forward_with_a_zero_cond_is_the_stock_oracle_forward():
    from oracle import fixtures

    for in_ch in (4, 8):
        lu, ou = L.build_lcm_unet(in_ch), fixtures.build_unet("tiny", in_ch)
        g = gen(3)
        x = torch.randn(2, in_ch, 8, 8, generator=g)
        ctx = torch.randn(2, 77, 64, generator=g)
        ref = ou(x, torch.tensor(981), encoder_hidden_states=ctx)[0]
        assert torch.equal(lu(x, torch.tensor(981), encoder_hidden_states=ctx, timestep_cond=torch.zeros(2, L.COND_DIM))[0], ref)
        assert torch.equal(lu(x, torch.tensor(981), encoder_hidden_states=ctx)[0], ref)
        cond = L.cond_for(lu, 7.5, 2)
        assert cond.shape == (2, L.COND_DIM)
        moved = lu(x, torch.tensor(981), encoder_hidden_states=ctx, timestep_cond=cond)[0]
        assert float((moved - ref).norm() / ref.norm()) > 1e-2, "the conditioning must change the result"


def test_unet_key_surface_and_round_trip(tmp_path):
    from gm_diffusion.components import UNet2DConditionModel

    lu = L.build_lcm_unet(4)
    cfg = vars(lu.config)
    m = UNet2DConditionModel(**cfg)
    keys = m.expected_keys()
    assert keys["time_embedding.cond_proj.weight"] == (64, L.COND_DIM) and "time_embedding.cond_proj.bias" not in keys
    plain = UNet2DConditionModel(**{**cfg, "time_cond_proj_dim": None})
    assert set(keys) - set(plain.expected_keys()) == {"time_embedding.cond_proj.weight"}
    m.load_state_dict(lu.state_dict(), strict=True)
    sd = {k: v for k, v in lu.state_dict().items() if k != "time_embedding.cond_proj.weight"}
    with pytest.raises(KeyError):
        m.load_state_dict(sd, strict=True)
    with pytest.raises(KeyError):
        plain.load_state_dict(lu.state_dict(), strict=True)  # unexpected key for a UNet without the projection
    m.load_state_dict(lu.state_dict())
    m.save_pretrained(str(tmp_path))
    back = UNet2DConditionModel.from_pretrained(str(tmp_path))
    assert back.config.time_cond_proj_dim == L.COND_DIM
    assert torch.equal(back.state_dict()["time_embedding.cond_proj.weight"], lu.state_dict()["time_embedding.cond_proj.weight"])
    assert set(back.state_dict()) == set(keys)
    r = UNet2DConditionModel(**cfg).init_random(seed=3)
    w = r.state_dict()["time_embedding.cond_proj.weight"]
    assert w.shape == (64, L.COND_DIM) and float(w.abs().max()) <= L.COND_DIM ** -0.5 and float(w.abs().max()) > 0
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="time_cond_proj_dim"):
            UNet2DConditionModel(**{**cfg, "time_cond_proj_dim": bad})
    assert not m.supports_cfg_shared() and plain.supports_cfg_shared()


# ---------------------------------------------------------------------------------------------------------------------------
# the generic (host) pipelines with duck-typed oracle UNets
# ---------------------------------------------------------------------------------------------------------------------------
class _Spy:
    """Wraps an oracle UNet: records the ``timestep_cond`` and the batch of every call."""

    def __init__(self, unet):
        self.unet, self.config, self.seen = unet, unet.config, []

    dtype = torch.float32

    def __call__(self, sample, t, **kw):
        self.seen.append((kw.get("timestep_cond"), sample.shape[0]))
        return self.unet(sample, t, **kw)


def test_generic_gm_pipeline_passes_timestep_cond_and_runs_without_cfg():
    from gm_diffusion.pipelines import StableDiffusionGMPipeline
    from oracle import fixtures

    spy = _Spy(L.build_lcm_unet(8))
    pipe = StableDiffusionGMPipeline(vae=FakeVae(), text_encoder=None, tokenizer=None, unet=spy, scheduler=lcm(steps_offset=1),
                                     safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    pe, ne, lat = fixtures.make_inputs(2, 8, 8, cross_dim=64)
    sdr = torch.randn(2, 4, 8, 8, generator=gen(77))
    g = gen(42)
    out = pipe(sdr, prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=4, guidance_scale=7.5, generator=g,
               output_type="latent").images
    assert not pipe.do_classifier_free_guidance and len(spy.seen) == 4
    want = L.guidance_embedding(torch.tensor([6.5, 6.5]), L.COND_DIM)
    for cond, rows in spy.seen:
        assert rows == 2 and cond is not None and cond.shape == (2, L.COND_DIM) and torch.equal(cond, want)
    ref = L.gm_loop(L.build_lcm_unet(8), L.RefLCMScheduler(), sdr, pe, ne, lat, 4, guidance_scale=7.5, generator=gen(42))
    assert torch.equal(out, ref)  # same torch expressions on the same host
    twin = gen(42)
    for _ in range(3):
        torch.randn(lat.shape, generator=twin)
    assert torch.equal(g.get_state(), twin.get_state())
    # a UNet without the projection is handed None, as before
    plain = _Spy(fixtures.build_unet("tiny", 8))
    pipe.unet = plain
    pipe(sdr, prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, guidance_scale=7.5, generator=gen(1), output_type="latent")
    assert pipe.do_classifier_free_guidance and all(c is None and rows == 4 for c, rows in plain.seen)


@pytest.mark.parametrize("gm_has_cond", [True, False])
def test_generic_dual_pipeline_gives_each_unet_its_own_cond(gm_has_cond):
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline
    from oracle import fixtures

    mk_gm = (lambda: L.build_lcm_unet(8, cond_dim=16)) if gm_has_cond else (lambda: fixtures.build_unet("tiny", 8))
    sdr_spy, gm_spy = _Spy(L.build_lcm_unet(4)), _Spy(mk_gm())
    pipe = StableDiffusionDualUNetPipeline(vae=FakeVae(), text_encoder=None, tokenizer=None, unet=sdr_spy, gm_unet=gm_spy,
                                           scheduler=lcm(steps_offset=1), safety_checker=None, feature_extractor=None,
                                           requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    pe, ne, lat = fixtures.make_inputs(1, 8, 8, cross_dim=64)
    s, g = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, height=64, width=64, num_inference_steps=4, guidance_scale=7.5,
                generator=gen(9), output_type="latent")
    assert all(c is not None and c.shape == (1, L.COND_DIM) and rows == 1 for c, rows in sdr_spy.seen) and len(sdr_spy.seen) == 4
    if gm_has_cond:
        assert all(c is not None and c.shape == (1, 16) for c, _ in gm_spy.seen)  # its own width, not the SDR UNet's
    else:
        assert all(c is None for c, _ in gm_spy.seen)
    rs, rg = L.dual_loop(L.build_lcm_unet(4), mk_gm(), L.RefLCMScheduler(), pe, ne, lat, 4, guidance_scale=7.5, generator=gen(9))
    assert torch.equal(s, rs) and torch.equal(g, rg)
    assert float((s - g).abs().max()) > 0.1


# ---------------------------------------------------------------------------------------------------------------------------
# ABI without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_lcm_step_argument_validation_without_gpu():
    from gm_diffusion import _native as native

    lib = native.lib()
    assert lib.gmd_abi_version() == 14 and native.ABI_VERSION == 14
    one = 1  # any non-null address: validation happens before a launch, nothing is dereferenced
    nan, inf = float("nan"), float("inf")

    def call(eps=one, x=one, noise=None, B=1, chw=16, ssa=0.9, ss1=0.43, clip=0, cr=0.0, cs=0.1, co=0.99, sp=0.95, bp=0.3, sa=0.9, s1=0.43,
             xp=one, x0=None, den=None):
        return lib.gmd_lcm_step(eps, x, noise, B, chw, 0, 1.0, None, 0.0, ssa, ss1, clip, cr, cs, co, sp, bp, sa, s1, xp, x0, den, None)

    for kw, word in ((dict(eps=None), b"null"), (dict(x=None), b"null"), (dict(xp=None), b"null"), (dict(B=-1), b"shape"), (dict(chw=0), b"shape"),
                     (dict(ssa=0.0), b"zero"), (dict(x0=one, sa=0.0), b"zero"), (dict(clip=1, cr=0.0), b"clip_range"),
                     (dict(clip=1, cr=nan), b"clip_range"), (dict(ssa=nan), b"sched_sqrt_alpha"), (dict(ss1=nan), b"sched_sqrt_one_minus_alpha"),
                     (dict(cs=nan), b"c_skip"), (dict(co=nan), b"c_out"), (dict(sp=nan), b"sqrt_alpha_prev"), (dict(bp=nan), b"sqrt_beta_prev"),
                     (dict(bp=inf), b"sqrt_beta_prev"), (dict(x0=one, s1=nan), b"x0"), (dict(x0=one, sa=nan), b"x0")):
        assert call(**kw) == 1, kw  # GMD_ERR_INVALID
        assert word in lib.gmd_last_error(), (kw, lib.gmd_last_error())
    assert call(B=0, eps=None, x=None, xp=None) == 0  # an empty batch is a no-op

    def temb(t=one, add=one, out=2, dtype=0, B=1, dim=64):
        return lib.gmd_timestep_embedding_add(t, add, out, dtype, B, dim, 1, 0.0, None)

    for kw, word in ((dict(t=None), b"null"), (dict(add=None), b"null"), (dict(out=None), b"null"), (dict(out=one), b"alias"),
                     (dict(dim=63), b"shape"), (dict(B=0), b"shape"), (dict(dtype=9), b"dtype")):
        assert temb(**kw) == 1, kw
        assert word in lib.gmd_last_error(), (kw, lib.gmd_last_error())


def test_new_ops_refuse_host_tensors():
    from gm_diffusion import hip_ops
    from gm_diffusion._native import HipExtensionError

    assert "lcm_step" in hip_ops.__all__ and "timestep_embedding_add" in hip_ops.__all__
    z = torch.zeros(1, 4, 8, 8)
    with pytest.raises(HipExtensionError):
        hip_ops.lcm_step(z, z, (0.9, 0.43, 0.1, 0.99, 0.95, 0.3, 0.9, 0.43), False, 1.0)
    with pytest.raises(HipExtensionError):
        hip_ops.timestep_embedding_add(torch.zeros(1), torch.zeros(1, 64), 1, 64, torch.float32)
