"""GPU: gmd_ddim_step and components.DDIMScheduler on the device -- the second grid-stride lap bit for bit through the raw C ABI, the
write footprint, edge values, a whole trajectory of the scheduler object against its own torch expressions (bit-identical), and both
pipelines at tiny width against the oracle loops driven by the float64 scheduler of tests/ddim_ref.py."""
import pytest
import torch

import ddim_ref as D
import small_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
RMS_TOL = 1e-3  # north star: "within 1e-3 latent RMS"
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ptr(t):
    return None if t is None else t.data_ptr()


def call(*args):
    from gm_diffusion._native import lib

    rc = lib().gmd_ddim_step(*args, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (rc, lib().gmd_last_error())


def nan_dev(shape):
    return torch.full(shape, float("nan"), dtype=F32, device=DEV)


def rms(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b) ** 2).mean().sqrt())


# =============================================================================================================================
# the second lap, bit for bit, through the raw C ABI
# =============================================================================================================================
LAT_B, LAT_SHAPE = 2, (4, 257, 257)
LAT_CHW = 4 * 257 * 257
GS, GR = 7.5, 0.7
COEFS = (0.9, 0.43, 0.95, 0.3, 0.1, 0.8, 0.6)  # sched_sqrt_a, sched_sqrt_1ma, sqrt_a_prev, dir_coeff, std, sqrt_a, sqrt_1ma


@pytest.fixture(scope="module")
def lap_inputs():
    """Inputs of the two-lap launches, drawn once and left unchanged (both do_cfg cases read the first B samples of eps_in)."""
    g = gen(31)
    eps_in = torch.randn((2 * LAT_B,) + LAT_SHAPE, generator=g)
    x, noise = (torch.randn((LAT_B,) + LAT_SHAPE, generator=g) for _ in range(2))
    ratio = torch.tensor([0.25, 3.0])  # two very different entries: the lap boundary falls inside sample 1
    return eps_in, x, noise, ratio, tuple(t.to(DEV) for t in (eps_in, x, noise, ratio))


@pytest.mark.parametrize("do_cfg", [False, True])
def test_ddim_step_second_lap(lap_inputs, do_cfg):
    n = LAT_B * LAT_CHW
    assert n > S.LAP_LATENT and LAT_CHW < S.LAP_LATENT < n, "not a two-lap launch with the lap boundary inside sample 1"
    eps_in, x, noise, ratio, (d_eps, d_x, d_noise, d_ratio) = lap_inputs
    eps_in = eps_in if do_cfg else eps_in[:LAT_B]
    eps = S.guided_eps(eps_in, LAT_B, do_cfg, GS, ratio, GR)
    d_nan = nan_dev((LAT_B,) + LAT_SHAPE)   # stands where noise == NULL is passed elsewhere; and the ratio of a do_cfg == 0 launch
    d_ratio = d_ratio if do_cfg else nan_dev((LAT_B,))
    sa, s1, sp, dc, sd, pa, p1 = COEFS
    for clip in (None, 1.0):
        for uc in (False, True):
            for nz in (noise, None):
                for want in (True, False):
                    xp_ref, x0_ref, p0_ref = D.ddim_step_f32(eps, x, COEFS, noise=nz, clip_range=clip, use_clipped=uc)
                    op, o0, o1 = (nan_dev((LAT_B,) + LAT_SHAPE) for _ in range(3))
                    d_nz = d_noise if nz is not None else d_nan
                    call(ptr(d_eps), ptr(d_x), ptr(d_nz) if nz is not None else None, LAT_B, LAT_CHW, int(do_cfg), GS, ptr(d_ratio), GR, sa, s1,
                         int(clip is not None), float(clip or 0.0), int(uc), sp, dc, sd, pa, p1, ptr(op), ptr(o0) if want else None,
                         ptr(o1) if want else None)
                    torch.cuda.synchronize()
                    what = f"ddim_step clip={clip} use_clipped={uc} noise={nz is not None} outputs={want} do_cfg={do_cfg}"
                    S.assert_bit_equal(op, xp_ref, what + " x_prev")
                    if want:
                        S.assert_bit_equal(o0, x0_ref, what + " x0")
                        S.assert_bit_equal(o1, p0_ref, what + " pred_x0")
                    else:
                        assert bool(torch.isnan(o0).all()) and bool(torch.isnan(o1).all()), what + ": an output that was not asked for was written"


# =============================================================================================================================
# write footprint
# =============================================================================================================================
GUARD = 16384  # float32 elements of sentinel before and after every output


@pytest.mark.parametrize("do_cfg", [False, True])
def test_ddim_step_stores_only_its_three_tensors(do_cfg):
    """B = 3 latents of chw = 3 * 7 * 5 = 105 elements (no multiple of 4 or 64): guard bands of a sentinel around x_prev, x0 and
    pred_x0 stay untouched, every element inside is written."""
    B, shape, chw = 3, (3, 3, 7, 5), 105
    n = B * chw
    g = gen(12)
    eps_in = torch.randn((2 * B if do_cfg else B,) + shape[1:], generator=g)
    x, noise = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    eps = S.guided_eps(eps_in, B, do_cfg, GS)
    refs = D.ddim_step_f32(eps, x, COEFS, noise=noise, clip_range=1.0, use_clipped=True)
    sentinel = -12345.678
    bufs = [torch.full((2 * GUARD + n,), sentinel, dtype=F32, device=DEV) for _ in range(3)]
    outs = [b[GUARD:GUARD + n] for b in bufs]
    sa, s1, sp, dc, sd, pa, p1 = COEFS
    d_eps, d_x, d_noise = eps_in.to(DEV), x.to(DEV), noise.to(DEV)
    call(ptr(d_eps), ptr(d_x), ptr(d_noise), B, chw, int(do_cfg), GS, None, 0.0, sa, s1, 1, 1.0, 1, sp, dc, sd, pa, p1, ptr(outs[0]), ptr(outs[1]),
         ptr(outs[2]))
    torch.cuda.synchronize()
    for b, o, r, nm in zip(bufs, outs, refs, ("x_prev", "x0", "pred_x0")):
        assert bool((b[:GUARD] == sentinel).all()) and bool((b[GUARD + n:] == sentinel).all()), f"{nm}: a guard band changed"
        assert not bool((o == sentinel).any()), f"{nm}: an element inside was not written"
        S.assert_bit_equal(o.view(shape), r, f"ddim_step footprint {nm} do_cfg={do_cfg}")


# =============================================================================================================================
# edge values, bit-exact
# =============================================================================================================================
def test_ddim_step_edge_values():
    """p0 exactly at +-clip_range; std = 0 with a noise tensor present (the add still happens: -0.0 + 0.0 is +0.0, not -0.0);
    dir_coeff = 0 (the last step of a set_alpha_to_one schedule)."""
    from gm_diffusion import hip_ops as ops

    # (1) sched_sqrt_a = 1, sched_sqrt_1ma = 0.5, eps = 0: p0 = x exactly; x straddles the clip range by one ulp either side
    one = torch.tensor(1.0)
    up, dn = torch.nextafter(one, torch.tensor(2.0)), torch.nextafter(one, torch.tensor(0.0))
    x = torch.stack([one, -one, up, -up, dn, -dn, torch.tensor(0.0), torch.tensor(-0.0)]).reshape(1, 8, 1, 1)
    eps = torch.zeros_like(x)
    coefs = (1.0, 0.5, 0.75, 0.25, 0.0, 1.0, 0.5)
    for uc in (False, True):
        ref = D.ddim_step_f32(eps, x, coefs, clip_range=1.0, use_clipped=uc)
        got = ops.ddim_step(eps.to(DEV), x.to(DEV), coefs, False, 1.0, clip_range=1.0, use_clipped=uc, want_x0=True, want_pred_x0=True)
        for g_, r_, nm in zip(got, ref, ("x_prev", "x0", "pred_x0")):
            S.assert_bit_equal(g_, r_, f"clip edge use_clipped={uc} {nm}")
        assert got[2].cpu().reshape(-1)[:6].abs().max() == 1.0
    # (2) std = 0 with noise: both products of sqrt_a_prev p0 + dir_coeff pe underflow to -0.0 for small negative p0 and eps (all inputs
    # are normal numbers), the sum is -0.0; adding 0 * noise = +0.0 gives +0.0
    x = torch.tensor([-1e-30, 1e-30, -1e-30, 1.5]).reshape(1, 4, 1, 1)
    eps = torch.tensor([-1e-30, 1e-30, -1e-30, -0.5]).reshape(1, 4, 1, 1)
    noise = torch.tensor([1.0, 1.0, -1.0, 2.0]).reshape(1, 4, 1, 1)
    coefs = (0.9, 0.43, 1e-30, 1e-30, 0.0, 0.8, 0.6)
    with_noise = D.ddim_step_f32(eps, x, coefs, noise=noise)[0]
    without = D.ddim_step_f32(eps, x, coefs)[0]
    assert int(S.bit_mismatch(with_noise, without).sum()) >= 1, "the test's inputs must tell the two apart"
    S.assert_bit_equal(ops.ddim_step(eps.to(DEV), x.to(DEV), coefs, False, 1.0, noise=noise.to(DEV))[0], with_noise, "std = 0 with noise")
    S.assert_bit_equal(ops.ddim_step(eps.to(DEV), x.to(DEV), coefs, False, 1.0)[0], without, "std = 0 without noise")
    # (3) dir_coeff = 0, sqrt_a_prev = 1: x_prev is p0, whatever eps (finite) says
    g = gen(8)
    x, eps = torch.randn(2, 4, 5, 3, generator=g), torch.randn(2, 4, 5, 3, generator=g)
    coefs = (0.9, 0.43, 1.0, 0.0, 0.0, 0.9, 0.43)
    for uc in (False, True):
        ref = D.ddim_step_f32(eps, x, coefs, use_clipped=uc)
        got = ops.ddim_step(eps.to(DEV), x.to(DEV), coefs, False, 1.0, use_clipped=uc, want_pred_x0=True)
        S.assert_bit_equal(got[0], ref[0], f"dir_coeff = 0 use_clipped={uc} x_prev")
        S.assert_bit_equal(got[2], ref[2], f"dir_coeff = 0 use_clipped={uc} pred_x0")
    with pytest.raises(ops.HipExtensionError):
        ops.ddim_step(eps.to(DEV), x.to(DEV), coefs, False, 1.0, noise=noise.to(DEV))  # noise of another shape


# =============================================================================================================================
# whole trajectory, scheduler object
# =============================================================================================================================
def _ddim(**kw):
    from gm_diffusion.components import DDIMScheduler

    return DDIMScheduler(**SD, **kw)


@pytest.mark.parametrize("use_clipped", [False, True])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("spacing", ["leading", "linspace", "trailing"])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_ddim_scheduler_device_steps_bit_exact_vs_torch(eta, spacing, clip, use_clipped):
    """gmd_ddim_step against the torch expressions of DDIMScheduler._host_step over a whole trajectory (CFG + guidance rescale + pipeline
    x0 + clipped x0 prediction + eta noise): bit-identical x_prev, pipeline x0 and pred_x0; the last step has prev_t < 0 (leading, linspace)."""
    from gm_diffusion.pipelines import rescale_noise_cfg

    mk = lambda: _ddim(clip_sample=clip, clip_sample_range=1.5, timestep_spacing=spacing)
    dev_s, host_s = mk(), mk()
    dev_s.set_timesteps(7)
    host_s.set_timesteps(7)
    g = gen(5)
    x = torch.randn(3, 4, 8, 8, generator=g)
    xd = x.to(DEV)
    gs, gr = 6.5, 0.3
    kw = dict(eta=eta, use_clipped_model_output=use_clipped)
    for t in dev_s.timesteps.tolist():
        eps2 = torch.randn(6, 4, 8, 8, generator=g)
        u, c = eps2.chunk(2)
        e = u + gs * (c - u)
        e = rescale_noise_cfg(e, c, guidance_rescale=gr)
        a = host_s.alphas_cumprod[t]
        x0_ref = (x - (1 - a).sqrt() * e) / a.sqrt()
        x_ref, p0_ref = host_s._host_step(e, t, x, generator=gen(100 + t), return_dict=False, **kw)
        xd_new, x0_dev = dev_s.fused_step(eps2.to(DEV), t, xd, True, gs, gr, want_x0=True, generator=gen(100 + t), **kw)
        one, _, p0_dev = dev_s._device_step(eps2.to(DEV), t, xd, True, gs, gr, False, gen(100 + t), want_pred_x0=True, **kw)
        S.assert_bit_equal(x0_dev, x0_ref, f"x0 t={t}")
        S.assert_bit_equal(xd_new, x_ref, f"x_prev t={t}")
        S.assert_bit_equal(one, x_ref, f"x_prev (pred_x0 launch) t={t}")
        S.assert_bit_equal(p0_dev, p0_ref, f"pred_x0 t={t}")
        out = dev_s.step(e.to(DEV), t, xd, generator=gen(100 + t), **kw)  # the public step on device tensors: the same kernel without CFG
        S.assert_bit_equal(out.prev_sample, x_ref, f"step prev_sample t={t}")
        S.assert_bit_equal(out.pred_original_sample, p0_ref, f"step pred_original_sample t={t}")
        x, xd = x_ref, xd_new
    assert (t - 1000 // 7 < 0) == (spacing != "trailing")  # leading / linspace end at t = 0: final_alpha_cumprod; trailing ends on prev_t = 0


# =============================================================================================================================
# pipelines at tiny width
# =============================================================================================================================
def _hip(model_cls, oracle_model):
    m = model_cls(**vars(oracle_model.config))
    m.load_state_dict(oracle_model.state_dict())
    return m.to(DEV, F32)


def _dual_pipe(scheduler):
    from gm_diffusion.components import AutoencoderKL, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline
    from oracle import fixtures

    pipe = StableDiffusionDualUNetPipeline(
        vae=_hip(AutoencoderKL, fixtures.build_vae("tiny")), text_encoder=None, tokenizer=None,
        unet=_hip(UNet2DConditionModel, fixtures.build_unet("tiny", 4)), gm_unet=_hip(UNet2DConditionModel, fixtures.build_unet("tiny", 8)),
        scheduler=scheduler, safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    return pipe


STEPS = 8


@pytest.fixture(scope="module")
def dual_case():
    """Inputs, the HIP dual pipeline with DDIM, and the oracle loop's latents per eta (computed once, left unchanged)."""
    from oracle import fixtures
    from oracle import pipelines as OP

    pe, ne, lat = fixtures.make_inputs(2, 16, 16, cross_dim=64)
    refs = {}
    for eta in (0.0, 0.7):
        refs[eta] = OP.dual_loop(fixtures.build_unet("tiny", 4), fixtures.build_unet("tiny", 8), D.RefDDIMScheduler(eta=eta), pe, ne, lat, STEPS,
                                 guidance_scale=7.5, generator=gen(123))
    pipe = _dual_pipe(_ddim(clip_sample=False, steps_offset=1))
    return pipe, pe, ne, lat, refs


def _run_dual(case, eta, generator, **attrs):
    pipe, pe, ne, lat, _ = case
    for k, v in attrs.items():
        setattr(pipe, k, v)
    return pipe(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), latents=lat.to(DEV), height=128, width=128,
                num_inference_steps=STEPS, guidance_scale=7.5, eta=eta, generator=generator, output_type="latent")


@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_dual_pipeline_ddim_matches_oracle(dual_case, eta):
    """Fused gmd_ddim_step under graphs + two streams and eager on one stream, against oracle.pipelines.dual_loop driven by the float64
    scheduler of tests/ddim_ref.py with the same CPU generator (shared by both schedulers: SDR noise before GM noise)."""
    pipe, pe, ne, lat, refs = dual_case
    rs, rg = refs[eta]
    assert pipe._use_fused(lat.to(DEV), pipe.unet, pipe.scheduler)
    g = gen(123)
    s1, g1 = _run_dual(dual_case, eta, g, use_hip_graphs=True, overlap_streams=True)
    if eta > 0:  # 2 draws per iteration, the last included (the latents were passed in: no draw for them)
        twin = gen(123)
        for _ in range(2 * STEPS):
            torch.randn(lat.shape, generator=twin)
        assert torch.equal(g.get_state(), twin.get_state())
    else:
        assert torch.equal(g.get_state(), gen(123).get_state())
    s2, g2 = _run_dual(dual_case, eta, gen(123), use_hip_graphs=False, overlap_streams=False)
    print(f"eta={eta}: latent RMS sdr={rms(s1, rs):.2e} gm={rms(g1, rg):.2e}")
    assert rms(s1, rs) <= RMS_TOL and rms(g1, rg) <= RMS_TOL
    assert rms(s2, rs) <= RMS_TOL and rms(g2, rg) <= RMS_TOL
    assert torch.equal(s1, s2) and torch.equal(g1, g2), "graphs + two streams and eager single stream must agree bit for bit"
    if eta > 0:  # the two latents must NOT have received the same noise
        assert rms(s1, rg) > 0.1
    # the pre-draw against the per-step draw: the same final latents, bit for bit
    from gm_diffusion.pipelines import StableDiffusionGMPipeline as Base  # _predraw_step_noise reads the ceiling from this class

    old = Base.PREDRAW_NOISE_BYTES
    try:
        Base.PREDRAW_NOISE_BYTES = 0
        assert Base._predraw_step_noise([pipe.scheduler], [1], lat.shape, gen(1), "cpu", eta=0.7) is None
        s3, g3 = _run_dual(dual_case, eta, gen(123), use_hip_graphs=True, overlap_streams=True)
    finally:
        Base.PREDRAW_NOISE_BYTES = old
    assert torch.equal(s3, s1) and torch.equal(g3, g1)
    # generic scheduler-protocol path (torch expressions of the reference loop on the HIP models)
    pipe._use_fused = lambda *args: False
    try:
        s4, g4 = _run_dual(dual_case, eta, gen(123))
    finally:
        del pipe._use_fused
    assert rms(s4, rs) <= RMS_TOL and rms(g4, rg) <= RMS_TOL


def test_dual_pipeline_generator_advanced_by_one_plus_two_per_step(dual_case):
    """Without ``latents`` the pipeline draws them first: the generator is advanced by exactly 1 + 2 * 8 draws for the dual run."""
    pipe, pe, ne, lat, _ = dual_case
    g, twin = gen(77), gen(77)
    pipe.use_hip_graphs, pipe.overlap_streams = True, True
    pipe(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), height=128, width=128, num_inference_steps=STEPS, guidance_scale=7.5,
         eta=0.7, generator=g, output_type="latent")
    for _ in range(1 + 2 * STEPS):
        torch.randn(lat.shape, generator=twin)
    assert torch.equal(g.get_state(), twin.get_state())


def test_eta_changes_ddim_and_leaves_pndm_alone(dual_case):
    from gm_diffusion.components import PNDMScheduler

    a = _run_dual(dual_case, 0.0, gen(123), use_hip_graphs=True, overlap_streams=True)
    b = _run_dual(dual_case, 0.7, gen(123))
    assert rms(a[0], b[0]) > 0.1 and rms(a[1], b[1]) > 0.1
    pipe = dual_case[0]
    ddim_s = pipe.scheduler
    pipe.scheduler = PNDMScheduler(skip_prk_steps=True, steps_offset=1, **SD)
    try:
        c = _run_dual(dual_case, 0.0, gen(123))
        d = _run_dual(dual_case, 0.7, gen(123))
    finally:
        pipe.scheduler = ddim_s
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])


@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_gm_pipeline_ddim_matches_oracle(eta):
    from gm_diffusion.components import AutoencoderKL, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionGMPipeline
    from oracle import fixtures
    from oracle import pipelines as OP

    ou = fixtures.build_unet("tiny", 8)
    pipe = StableDiffusionGMPipeline(
        vae=_hip(AutoencoderKL, fixtures.build_vae("tiny")), text_encoder=None, tokenizer=None, unet=_hip(UNet2DConditionModel, ou),
        scheduler=_ddim(clip_sample=False, steps_offset=1), safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    pe, ne, lat = fixtures.make_inputs(1, 16, 16, cross_dim=64)
    sdr_lat = torch.randn(1, 4, 16, 16, generator=gen(77))
    ref = OP.gm_loop(ou, D.RefDDIMScheduler(eta=eta), sdr_lat, pe, ne, lat, STEPS, guidance_scale=7.5, generator=gen(42))
    run = lambda: pipe(sdr_lat.to(DEV), prompt=None, prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), latents=lat.to(DEV),
                       num_inference_steps=STEPS, guidance_scale=7.5, eta=eta, generator=gen(42), output_type="latent").images
    assert pipe._use_fused(lat.to(DEV), pipe.unet, pipe.scheduler)
    out = run()
    print(f"eta={eta}: latent RMS {rms(out, ref):.2e}")
    assert rms(out, ref) <= RMS_TOL
    pipe.use_hip_graphs = False
    assert torch.equal(run(), out)
    pipe._use_fused = lambda *args: False
    assert rms(run(), ref) <= RMS_TOL
