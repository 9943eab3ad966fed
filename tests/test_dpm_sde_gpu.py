"""GPU: gmd_dpm_sde_step and components.DPMSolverMultistepScheduler (SDE algorithm, heun solver type) on the device -- the second
grid-stride lap bit for bit through the raw C ABI, the write footprint, edge values, whole trajectories of the scheduler object against its
own torch expressions (bit-identical), and both pipelines at tiny width against the oracle loops driven by the float64 scheduler of
tests/dpm_sde_ref.py."""
import pytest
import torch

import dpm_sde_ref as D
import small_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
RMS_TOL = 1e-3  # north star: "within 1e-3 latent RMS"
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
VARIANTS = [(a, s) for a in (D.ODE, D.SDE) for s in ("midpoint", "heun")]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ptr(t):
    return None if t is None else t.data_ptr()


def call(*args):
    from gm_diffusion._native import lib

    rc = lib().gmd_dpm_sde_step(*args, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (rc, lib().gmd_last_error())


def nan_dev(shape):
    return torch.full(shape, float("nan"), dtype=F32, device=DEV)


def rms(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b) ** 2).mean().sqrt())


def _dpm(**kw):
    from gm_diffusion.components import DPMSolverMultistepScheduler

    return DPMSolverMultistepScheduler(**SD, **kw)


# =============================================================================================================================
# the second lap, bit for bit, through the raw C ABI
# =============================================================================================================================
LAT_B, LAT_SHAPE = 2, (4, 257, 257)
LAT_CHW = 4 * 257 * 257
GS, GR = 7.5, 0.7
COEFS = (0.43, 0.9, 0.8, 0.35, 0.2, 1.3, 0.25, 0.8, 0.6)  # sigma_s0, alpha_s0, c_x, c_m, c_h, inv_r0, c_n, sqrt_a, sqrt_1ma


@pytest.fixture(scope="module")
def lap_inputs():
    """Inputs of the two-lap launches, drawn once and left unchanged (both do_cfg cases read the first B samples of eps_in)."""
    g = gen(31)
    eps_in = torch.randn((2 * LAT_B,) + LAT_SHAPE, generator=g)
    x, m1, noise = (torch.randn((LAT_B,) + LAT_SHAPE, generator=g) for _ in range(3))
    ratio = torch.tensor([0.25, 3.0])  # two very different entries: the lap boundary falls inside sample 1
    return eps_in, x, m1, noise, ratio, tuple(t.to(DEV) for t in (eps_in, x, m1, noise, ratio))


@pytest.mark.parametrize("do_cfg", [False, True])
def test_dpm_sde_step_second_lap(lap_inputs, do_cfg):
    n = LAT_B * LAT_CHW
    assert n > S.LAP_LATENT and LAT_CHW < S.LAP_LATENT < n, "not a two-lap launch with the lap boundary inside sample 1"
    eps_in, x, m1, noise, ratio, (d_eps, d_x, d_m1, d_noise, d_ratio) = lap_inputs
    eps_in = eps_in if do_cfg else eps_in[:LAT_B]
    eps = S.guided_eps(eps_in, LAT_B, do_cfg, GS, ratio, GR)
    d_ratio = d_ratio if do_cfg else nan_dev((LAT_B,))  # the ratio of a do_cfg == 0 launch must not be read
    for order in (1, 2):
        xp_ref, m0_ref, x0_ref = D.dpm_step_f32(eps, x, order, COEFS, noise=noise, m1=m1)
        d_m = d_m1 if order == 2 else nan_dev((LAT_B,) + LAT_SHAPE)  # the history of a first-order launch must not be read
        for want in (True, False):
            om, op, o0 = (nan_dev((LAT_B,) + LAT_SHAPE) for _ in range(3))
            call(ptr(d_eps), ptr(d_x), ptr(d_m), ptr(d_noise), LAT_B, LAT_CHW, int(do_cfg), GS, ptr(d_ratio), GR, order, *COEFS, ptr(om),
                 ptr(op), ptr(o0) if want else None)
            torch.cuda.synchronize()
            what = f"dpm_sde_step order={order} x0={want} do_cfg={do_cfg}"
            S.assert_bit_equal(op, xp_ref, what + " x_prev")
            S.assert_bit_equal(om, m0_ref, what + " m0")
            if want:
                S.assert_bit_equal(o0, x0_ref, what + " x0")
            else:
                assert bool(torch.isnan(o0).all()), what + ": an output that was not asked for was written"


# =============================================================================================================================
# write footprint
# =============================================================================================================================
GUARD = 16384  # float32 elements of sentinel before and after every output


@pytest.mark.parametrize("do_cfg", [False, True])
def test_dpm_sde_step_stores_only_its_three_tensors(do_cfg):
    """B = 3 latents of chw = 3 * 7 * 5 = 105 elements (no multiple of 4 or 64): guard bands of a sentinel around m0_out, x_prev and x0
    stay untouched, every element inside is written."""
    B, shape, chw = 3, (3, 3, 7, 5), 105
    n = B * chw
    g = gen(12)
    eps_in = torch.randn((2 * B if do_cfg else B,) + shape[1:], generator=g)
    x, m1, noise = (torch.randn(shape, generator=g) for _ in range(3))
    eps = S.guided_eps(eps_in, B, do_cfg, GS)
    xp_ref, m0_ref, x0_ref = D.dpm_step_f32(eps, x, 2, COEFS, noise=noise, m1=m1)
    sentinel = -12345.678
    bufs = [torch.full((2 * GUARD + n,), sentinel, dtype=F32, device=DEV) for _ in range(3)]
    outs = [b[GUARD:GUARD + n] for b in bufs]
    d_eps, d_x, d_m1, d_noise = eps_in.to(DEV), x.to(DEV), m1.to(DEV), noise.to(DEV)
    call(ptr(d_eps), ptr(d_x), ptr(d_m1), ptr(d_noise), B, chw, int(do_cfg), GS, None, 0.0, 2, *COEFS, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]))
    torch.cuda.synchronize()
    for b, o, r, nm in zip(bufs, outs, (m0_ref, xp_ref, x0_ref), ("m0_out", "x_prev", "x0")):
        assert bool((b[:GUARD] == sentinel).all()) and bool((b[GUARD + n:] == sentinel).all()), f"{nm}: a guard band changed"
        assert not bool((o == sentinel).any()), f"{nm}: an element inside was not written"
        S.assert_bit_equal(o.view(shape), r, f"dpm_sde_step footprint {nm} do_cfg={do_cfg}")


# =============================================================================================================================
# edge values, bit-exact
# =============================================================================================================================
def test_dpm_sde_step_edge_values():
    """c_n = 0 with a noise tensor present (the add still happens: -0.0 + 0.0 is +0.0, not -0.0); the real last-step coefficients of a
    final_sigmas_type="zero" schedule; noise of another shape; an empty batch."""
    from gm_diffusion import hip_ops as ops

    # (1) c_n = 0: both products of c_x x + c_m m0 underflow to -0.0 for small negative x and m0 (all inputs are normal numbers), the
    # sum is -0.0; adding 0 * noise = +0.0 gives +0.0
    x = torch.tensor([-1e-30, 1e-30, -1e-30, 1.5]).reshape(1, 4, 1, 1)
    eps = torch.tensor([1e-30, -1e-30, 1e-30, -0.5]).reshape(1, 4, 1, 1)
    noise = torch.tensor([1.0, 1.0, -1.0, 2.0]).reshape(1, 4, 1, 1)
    coefs = (0.43, 0.9, 1e-30, 1e-30, 0.0, 0.0, 0.0, 0.8, 0.6)
    added, m0, _ = D.dpm_step_f32(eps, x, 1, coefs, noise=noise)
    skipped = torch.tensor(coefs[2]) * x + torch.tensor(coefs[3]) * m0  # the partial sum, as a kernel that skips the add would store it
    assert int(S.bit_mismatch(added, skipped).sum()) >= 1, "the test's inputs must tell 'added' from 'skipped' apart"
    assert bool((m0.reshape(-1)[:3].abs() > 1e-31).all())  # normal numbers, not zeros: the -0.0 comes from the products
    got = ops.dpm_sde_step(eps.to(DEV), x.to(DEV), 1, coefs, False, 1.0, noise.to(DEV))
    S.assert_bit_equal(got[1], added, "c_n = 0 with noise: x_prev")
    # (2) the last step of a "zero" schedule: c_x = 0, c_m = 1, c_n = 0 -- x_prev is m0 (+ 0.0), whatever x and the noise say
    for solver in ("midpoint", "heun"):
        s = _dpm(algorithm_type=D.SDE, solver_type=solver, steps_offset=1, timestep_spacing="leading")
        s.set_timesteps(8)
        s._step_index, s.lower_order_nums = 7, 2
        first, a0, g0, at, gt, h, r0 = s._plan_step(int(s.timesteps[-1]))
        c_x, c_m, c_h, c_n = s._update_coefs(first, at, gt, g0, h)
        assert first and c_h is None and (float(c_x), float(c_m), float(c_n)) == (0.0, 1.0, 0.0) and float(h) == float("inf")
        g = gen(8)
        x, eps, noise = (torch.randn(2, 4, 5, 3, generator=g) for _ in range(3))
        coefs = (g0.item(), a0.item(), 0.0, 1.0, 0.0, 0.0, 0.0, 0.9, 0.43)
        ref = D.dpm_step_f32(eps, x, 1, coefs, noise=noise)
        got = ops.dpm_sde_step(eps.to(DEV), x.to(DEV), 1, coefs, False, 1.0, noise.to(DEV), want_x0=True)
        for g_, r_, nm in zip(got, (ref[1], ref[0], ref[2]), ("m0", "x_prev", "x0")):
            S.assert_bit_equal(g_, r_, f"last step ({solver}) {nm}")
        assert bool(torch.isfinite(got[1]).all())
    # (3) noise of another shape, no noise
    with pytest.raises(ops.HipExtensionError):
        ops.dpm_sde_step(eps.to(DEV), x.to(DEV), 1, coefs, False, 1.0, noise[:1].to(DEV))
    with pytest.raises(ops.HipExtensionError):
        ops.dpm_sde_step(eps.to(DEV), x.to(DEV), 1, coefs, False, 1.0, None)
    # (4) B = 0 is a no-op
    e = torch.empty(0, 4, 5, 3, device=DEV)
    m0, xp, x0 = ops.dpm_sde_step(e, e, 1, coefs, False, 1.0, e, want_x0=True)
    assert m0.shape == xp.shape == x0.shape == (0, 4, 5, 3)


# =============================================================================================================================
# whole trajectories, scheduler object
# =============================================================================================================================
@pytest.mark.parametrize("gr", [0.0, 0.7])
@pytest.mark.parametrize("n,final", [(9, "zero"), (16, "sigma_min")])
@pytest.mark.parametrize("spacing", ["leading", "linspace", "trailing"])
@pytest.mark.parametrize("alg,solver", VARIANTS)
def test_dpm_scheduler_device_steps_vs_torch(alg, solver, spacing, n, final, gr):
    """gmd_dpm_sde_step / gmd_dpm_step against the torch expressions of DPMSolverMultistepScheduler._host_step over a whole trajectory
    (CFG + pipeline x0 + history + per-step noise from the same seeds): bit-identical x_prev and pipeline x0 with guidance_rescale = 0;
    with guidance_rescale = 0.7 the std ratio is reduced in another order on the device (atol of test_dpm_step_kernel_bit_exact_vs_torch)."""
    from gm_diffusion.pipelines import rescale_noise_cfg

    mk = lambda: _dpm(algorithm_type=alg, solver_type=solver, timestep_spacing=spacing, final_sigmas_type=final)
    fused_s, step_s, host_s = mk(), mk(), mk()
    for s in (fused_s, step_s, host_s):
        s.set_timesteps(n)
    g = gen(5)
    x = torch.randn(3, 4, 8, 8, generator=g)
    xd = xs = x.to(DEV)
    gs = 6.5
    for t in host_s.timesteps.tolist():
        eps2 = torch.randn(6, 4, 8, 8, generator=g)
        u, c = eps2.chunk(2)
        e = u + gs * (c - u)
        if gr > 0:
            e = rescale_noise_cfg(e, c, guidance_rescale=gr)
        a = host_s.alphas_cumprod[t]
        x0_ref = (x - (1 - a).sqrt() * e) / a.sqrt()
        x_ref = host_s.step(e, t, x, generator=gen(100 + t), return_dict=False)[0]
        xd, x0_dev = fused_s.fused_step(eps2.to(DEV), t, xd, True, gs, gr, want_x0=True, generator=gen(100 + t))
        # the public step on device tensors: the same kernel without CFG, fed the host's guided eps and the host's trajectory
        xs = step_s.step(e.to(DEV), t, x.to(DEV), generator=gen(100 + t)).prev_sample
        S.assert_bit_equal(xs, x_ref, f"step prev_sample t={t}")
        if gr == 0.0:
            S.assert_bit_equal(x0_dev, x0_ref, f"x0 t={t}")
            S.assert_bit_equal(xd, x_ref, f"x_prev t={t}")
        else:
            assert torch.allclose(xd.cpu(), x_ref, atol=2e-5) and torch.allclose(x0_dev.cpu(), x0_ref, atol=2e-5), t
        x = x_ref
    assert fused_s.step_index == step_s.step_index == host_s.step_index == n
    assert bool(torch.isfinite(xd).all())


# =============================================================================================================================
# pipelines at tiny width
# =============================================================================================================================
def _hip(model_cls, oracle_model):
    m = model_cls(**vars(oracle_model.config))
    m.load_state_dict(oracle_model.state_dict())
    return m.to(DEV, F32)


STEPS = 8
PIPE_VARIANTS = [(D.SDE, "midpoint"), (D.SDE, "heun"), (D.ODE, "heun")]


@pytest.fixture(scope="module")
def dual_case():
    """Inputs, the HIP dual pipeline, and the oracle loop's latents per variant (computed once, left unchanged)."""
    from gm_diffusion.components import AutoencoderKL, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline
    from oracle import fixtures
    from oracle import pipelines as OP

    pe, ne, lat = fixtures.make_inputs(2, 16, 16, cross_dim=64)
    u4, u8 = fixtures.build_unet("tiny", 4), fixtures.build_unet("tiny", 8)
    refs = {v: OP.dual_loop(u4, u8, D.RefDPMSolverScheduler(*v), pe, ne, lat, STEPS, guidance_scale=7.5, generator=gen(123)) for v in PIPE_VARIANTS}
    pipe = StableDiffusionDualUNetPipeline(
        vae=_hip(AutoencoderKL, fixtures.build_vae("tiny")), text_encoder=None, tokenizer=None, unet=_hip(UNet2DConditionModel, u4),
        gm_unet=_hip(UNet2DConditionModel, u8), scheduler=_dpm(steps_offset=1, timestep_spacing="leading"), safety_checker=None,
        feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    return pipe, pe, ne, lat, refs


def _run_dual(case, variant, generator, with_latents=True, **attrs):
    pipe, pe, ne, lat, _ = case
    pipe.scheduler = _dpm(algorithm_type=variant[0], solver_type=variant[1], steps_offset=1, timestep_spacing="leading")
    for k, v in attrs.items():
        setattr(pipe, k, v)
    kw = dict(latents=lat.to(DEV)) if with_latents else {}
    return pipe(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), height=128, width=128, num_inference_steps=STEPS,
                guidance_scale=7.5, eta=0.7, generator=generator, output_type="latent", **kw)


@pytest.mark.parametrize("variant", PIPE_VARIANTS)
def test_dual_pipeline_matches_oracle(dual_case, variant):
    """Fused step under graphs + two streams and eager on one stream, against oracle.pipelines.dual_loop driven by the float64 scheduler
    of tests/dpm_sde_ref.py with the same CPU generator (shared by both schedulers: SDR noise before GM noise)."""
    pipe, pe, ne, lat, refs = dual_case
    rs, rg = refs[variant]
    sde = variant[0] == D.SDE
    g = gen(123)
    seen = {}
    predraw = pipe._predraw_step_noise
    pipe._predraw_step_noise = lambda *a, **k: seen.setdefault("pre", predraw(*a, **k))  # what the loop hands to the two schedulers
    try:
        s1, g1 = _run_dual(dual_case, variant, g, use_hip_graphs=True, overlap_streams=True)
    finally:
        del pipe._predraw_step_noise
    assert pipe._use_fused(lat.to(DEV), pipe.unet, pipe.scheduler)
    if sde:  # every (step, scheduler) is a slot, and the SDR and GM latents do NOT receive the same noise
        assert all(seen["pre"][k][i] is not None for k in range(2) for i in range(STEPS))
        assert not any(torch.equal(seen["pre"][0][i], seen["pre"][1][i]) for i in range(STEPS))
    else:
        assert seen["pre"] is None
    twin = gen(123)
    for _ in range(2 * STEPS if sde else 0):  # 2 draws per iteration, the last included (the latents were passed in: no draw for them)
        torch.randn(lat.shape, generator=twin)
    assert torch.equal(g.get_state(), twin.get_state())
    s2, g2 = _run_dual(dual_case, variant, gen(123), use_hip_graphs=False, overlap_streams=False)
    print(f"{variant}: latent RMS sdr={rms(s1, rs):.2e} gm={rms(g1, rg):.2e}")
    assert rms(s1, rs) <= RMS_TOL and rms(g1, rg) <= RMS_TOL
    assert rms(s2, rs) <= RMS_TOL and rms(g2, rg) <= RMS_TOL
    assert torch.equal(s1, s2) and torch.equal(g1, g2), "graphs + two streams and eager single stream must agree bit for bit"
    # the pre-draw against the per-step draw: the same final latents, bit for bit
    from gm_diffusion.pipelines import StableDiffusionGMPipeline as Base  # _predraw_step_noise reads the ceiling from this class

    old = Base.PREDRAW_NOISE_BYTES
    try:
        Base.PREDRAW_NOISE_BYTES = 0
        assert Base._predraw_step_noise([pipe.scheduler], [1], lat.shape, gen(1), "cpu") is None
        s3, g3 = _run_dual(dual_case, variant, gen(123), use_hip_graphs=True, overlap_streams=True)
    finally:
        Base.PREDRAW_NOISE_BYTES = old
    assert torch.equal(s3, s1) and torch.equal(g3, g1)
    # generic scheduler-protocol path (torch expressions of the reference loop on the HIP models)
    pipe._use_fused = lambda *args: False
    try:
        s4, g4 = _run_dual(dual_case, variant, gen(123))
    finally:
        del pipe._use_fused
    assert rms(s4, rs) <= RMS_TOL and rms(g4, rg) <= RMS_TOL


def test_dual_pipeline_generator_advanced_by_one_plus_two_per_step(dual_case):
    """Without ``latents`` the pipeline draws them first: the generator is advanced by exactly 1 + 2 * 8 draws for the dual run."""
    lat = dual_case[3]
    g, twin = gen(77), gen(77)
    _run_dual(dual_case, (D.SDE, "midpoint"), g, with_latents=False, use_hip_graphs=True, overlap_streams=True)
    for _ in range(1 + 2 * STEPS):
        torch.randn(lat.shape, generator=twin)
    assert torch.equal(g.get_state(), twin.get_state())


def test_sde_run_differs_from_the_deterministic_run(dual_case):
    a = _run_dual(dual_case, (D.ODE, "midpoint"), gen(123), use_hip_graphs=True, overlap_streams=True)
    b = _run_dual(dual_case, (D.SDE, "midpoint"), gen(123))
    assert rms(a[0], b[0]) > 0.1 and rms(a[1], b[1]) > 0.1


@pytest.mark.parametrize("variant", PIPE_VARIANTS)
def test_gm_pipeline_matches_oracle(variant):
    from gm_diffusion.components import AutoencoderKL, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionGMPipeline
    from oracle import fixtures
    from oracle import pipelines as OP

    ou = fixtures.build_unet("tiny", 8)
    mk = lambda: _dpm(algorithm_type=variant[0], solver_type=variant[1], steps_offset=1, timestep_spacing="leading")
    pipe = StableDiffusionGMPipeline(
        vae=_hip(AutoencoderKL, fixtures.build_vae("tiny")), text_encoder=None, tokenizer=None, unet=_hip(UNet2DConditionModel, ou),
        scheduler=mk(), safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    pe, ne, lat = fixtures.make_inputs(1, 16, 16, cross_dim=64)
    sdr_lat = torch.randn(1, 4, 16, 16, generator=gen(77))
    ref = OP.gm_loop(ou, D.RefDPMSolverScheduler(*variant), sdr_lat, pe, ne, lat, STEPS, guidance_scale=7.5, generator=gen(42))

    def run(g, **kw):
        pipe.scheduler = mk()
        kw = kw or dict(latents=lat.to(DEV))
        return pipe(sdr_lat.to(DEV), prompt=None, prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), num_inference_steps=STEPS,
                    guidance_scale=7.5, eta=0.7, generator=g, output_type="latent", **kw).images

    g = gen(42)
    out = run(g)
    assert pipe._use_fused(lat.to(DEV), pipe.unet, pipe.scheduler)
    twin = gen(42)
    for _ in range(STEPS if variant[0] == D.SDE else 0):
        torch.randn(lat.shape, generator=twin)
    assert torch.equal(g.get_state(), twin.get_state())
    print(f"{variant}: latent RMS {rms(out, ref):.2e}")
    assert rms(out, ref) <= RMS_TOL
    pipe.use_hip_graphs = False
    assert torch.equal(run(gen(42)), out)
    g, twin = gen(9), gen(9)
    run(g, height=128, width=128)  # no latents: one more draw
    for _ in range(1 + (STEPS if variant[0] == D.SDE else 0)):
        torch.randn(lat.shape, generator=twin)
    assert torch.equal(g.get_state(), twin.get_state())
    pipe._use_fused = lambda *args: False
    assert rms(run(gen(42)), ref) <= RMS_TOL
