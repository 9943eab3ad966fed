"""GPU: gmd_euler_step, gmd_pack_unet_input_scaled and the two sigma-space schedulers on the device -- the second grid-stride lap bit for
bit through the raw C ABI, the write footprint, edge values, the scaled pack against ``(x / div).to(dtype)``, whole trajectories of the
scheduler objects against their own torch expressions (bit-identical), both pipelines at tiny width against the loops driven by the
float64 schedulers of tests/euler_ref.py, the fractional timesteps the UNets read, and the untouched plain pack of the other schedulers."""
import copy

import pytest
import torch

import euler_ref as E
import small_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
RMS_TOL = 1e-3  # the project's gate (tests/test_ddim_gpu.py): "within 1e-3 latent RMS"
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SPACINGS = ("linspace", "leading", "trailing")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ptr(t):
    return None if t is None else t.data_ptr()


def call(*args):
    from gm_diffusion._native import lib

    rc = lib().gmd_euler_step(*args, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (rc, lib().gmd_last_error())


def nan_dev(shape):
    return torch.full(shape, float("nan"), dtype=F32, device=DEV)


def rms(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b) ** 2).mean().sqrt())


def euler(**kw):
    from gm_diffusion.components import EulerDiscreteScheduler

    return EulerDiscreteScheduler(**SD, **kw)


def ancestral(**kw):
    from gm_diffusion.components import EulerAncestralDiscreteScheduler

    return EulerAncestralDiscreteScheduler(**SD, **kw)


# =============================================================================================================================
# the second lap, bit for bit, through the raw C ABI
# =============================================================================================================================
LAT_B, LAT_SHAPE = 2, (4, 257, 257)
LAT_CHW = 4 * 257 * 257
GS, GR = 7.5, 0.7
COEFS = (3.25, -1.4, 0.9)  # sigma_hat, dt, sigma_up


@pytest.fixture(scope="module")
def lap_inputs():
    """Inputs of the two-lap launches, drawn once and left unchanged (both do_cfg cases read the first B samples of eps_in)."""
    g = gen(31)
    eps_in = torch.randn((2 * LAT_B,) + LAT_SHAPE, generator=g)
    x, noise = (torch.randn((LAT_B,) + LAT_SHAPE, generator=g) for _ in range(2))
    ratio = torch.tensor([0.25, 3.0])  # two very different entries: the lap boundary falls inside sample 1
    return eps_in, x, noise, ratio, tuple(t.to(DEV) for t in (eps_in, x, noise, ratio))


@pytest.mark.parametrize("do_cfg", [False, True])
def test_euler_step_second_lap(lap_inputs, do_cfg):
    n = LAT_B * LAT_CHW
    assert n > S.LAP_LATENT and LAT_CHW < S.LAP_LATENT < n and n % 256 != 0, "not a two-lap launch with a ragged tail"
    eps_in, x, noise, ratio, (d_eps, d_x, d_noise, d_ratio) = lap_inputs
    eps_in = eps_in if do_cfg else eps_in[:LAT_B]
    eps = S.guided_eps(eps_in, LAT_B, do_cfg, GS, ratio, GR)
    d_ratio = d_ratio if do_cfg else nan_dev((LAT_B,))  # a do_cfg == 0 launch must not read the ratio
    sh, dt, su = COEFS
    for nz in (noise, None):
        for want in (True, False):
            xp_ref, p0_ref = E.euler_step_f32(eps, x, COEFS, noise=nz)
            op, o0 = (nan_dev((LAT_B,) + LAT_SHAPE) for _ in range(2))
            call(ptr(d_eps), ptr(d_x), ptr(d_noise) if nz is not None else None, LAT_B, LAT_CHW, int(do_cfg), GS, ptr(d_ratio), GR, sh, dt, su,
                 ptr(op), ptr(o0) if want else None)
            torch.cuda.synchronize()
            what = f"euler_step noise={nz is not None} pred_x0={want} do_cfg={do_cfg}"
            S.assert_bit_equal(op, xp_ref, what + " x_prev")
            if want:
                S.assert_bit_equal(o0, p0_ref, what + " pred_x0")
            else:
                assert bool(torch.isnan(o0).all()), what + ": an output that was not asked for was written"


# =============================================================================================================================
# write footprint
# =============================================================================================================================
GUARD = 16384  # float32 elements of sentinel before and after every output


@pytest.mark.parametrize("do_cfg", [False, True])
def test_euler_step_stores_only_its_two_tensors(do_cfg):
    """B = 3 latents of chw = 3 * 7 * 5 = 105 elements (no multiple of 4 or 64): guard bands of a sentinel around x_prev and pred_x0 stay
    untouched, every element inside is written, and the three inputs are left as they were."""
    B, shape, chw = 3, (3, 3, 7, 5), 105
    n = B * chw
    g = gen(12)
    eps_in = torch.randn((2 * B if do_cfg else B,) + shape[1:], generator=g)
    x, noise = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    eps = S.guided_eps(eps_in, B, do_cfg, GS)
    refs = E.euler_step_f32(eps, x, COEFS, noise=noise)
    sentinel = -12345.678
    bufs = [torch.full((2 * GUARD + n,), sentinel, dtype=F32, device=DEV) for _ in range(2)]
    outs = [b[GUARD:GUARD + n] for b in bufs]
    sh, dt, su = COEFS
    d_eps, d_x, d_noise = eps_in.to(DEV), x.to(DEV), noise.to(DEV)
    call(ptr(d_eps), ptr(d_x), ptr(d_noise), B, chw, int(do_cfg), GS, None, 0.0, sh, dt, su, ptr(outs[0]), ptr(outs[1]))
    torch.cuda.synchronize()
    for b, o, r, nm in zip(bufs, outs, refs, ("x_prev", "pred_x0")):
        assert bool((b[:GUARD] == sentinel).all()) and bool((b[GUARD + n:] == sentinel).all()), f"{nm}: a guard band changed"
        assert not bool((o == sentinel).any()), f"{nm}: an element inside was not written"
        S.assert_bit_equal(o.view(shape), r, f"euler_step footprint {nm} do_cfg={do_cfg}")
    for d, h, nm in ((d_eps, eps_in, "eps_in"), (d_x, x, "x"), (d_noise, noise, "noise")):
        S.assert_bit_equal(d, h, f"input {nm} changed")


# =============================================================================================================================
# edge values, bit-exact
# =============================================================================================================================
def test_euler_step_edge_values():
    """sigma_hat at 2^-20 and 2^10, dt = -sigma_hat (the last step: x_prev is the x0 prediction up to rounding), +-0.0 inputs, and
    noise = -0.0 with sigma_up = 0 (the add still happens: the sign of a zero result is torch's)."""
    from gm_diffusion import hip_ops as ops

    g = gen(8)
    base = torch.randn(2, 4, 5, 3, generator=g)
    x = base.clone()
    x.view(-1)[:6] = torch.tensor([0.0, -0.0, 0.0, -0.0, 1.0, -1.0])
    eps = torch.randn(2, 4, 5, 3, generator=g)
    eps.view(-1)[:6] = torch.tensor([0.0, 0.0, -0.0, -0.0, 0.0, -0.0])
    for sh in (2.0 ** -20, 2.0 ** 10):
        for dt in (-sh, -0.5 * sh, 0.0):
            ref = E.euler_step_f32(eps, x, (sh, dt, 0.0))
            got = ops.euler_step(eps.to(DEV), x.to(DEV), (sh, dt, 0.0), False, 1.0, want_pred_x0=True)
            S.assert_bit_equal(got[0], ref[0], f"sigma_hat={sh} dt={dt} x_prev")
            S.assert_bit_equal(got[1], ref[1], f"sigma_hat={sh} dt={dt} pred_x0")
    # noise = -0.0 with sigma_up = 0: the product is -0.0; x_prev + -0.0 keeps x_prev's sign of zero, and a -0.0 result must come back
    # as -0.0.  x = -0.0, eps = +0.0: p0 = -0.0 - 0 = -0.0, d = (-0.0 - -0.0) / s = +0.0, d dt = -0.0 (dt < 0), x + d dt = -0.0
    x = torch.tensor([-0.0, 0.0, -0.0, 1.5]).reshape(1, 4, 1, 1)
    eps = torch.tensor([0.0, 0.0, 0.0, -0.5]).reshape(1, 4, 1, 1)
    for nz in (torch.tensor([-0.0, -0.0, 0.0, -0.0]).reshape(1, 4, 1, 1), None):
        ref = E.euler_step_f32(eps, x, (2.0, -2.0, 0.0), noise=nz)[0]
        got = ops.euler_step(eps.to(DEV), x.to(DEV), (2.0, -2.0, 0.0), False, 1.0, noise=None if nz is None else nz.to(DEV))[0]
        S.assert_bit_equal(got, ref, f"sigma_up = 0, noise={'given' if nz is not None else 'absent'}")
    with_minus = E.euler_step_f32(eps, x, (2.0, -2.0, 0.0), noise=torch.full((1, 4, 1, 1), -0.0))[0]
    with_plus = E.euler_step_f32(eps, x, (2.0, -2.0, 0.0), noise=torch.full((1, 4, 1, 1), 0.0))[0]
    assert int(S.bit_mismatch(with_minus, with_plus).sum()) >= 1, "the test's inputs must tell -0.0 noise from +0.0 noise"
    S.assert_bit_equal(ops.euler_step(eps.to(DEV), x.to(DEV), (2.0, -2.0, 0.0), False, 1.0, noise=torch.full((1, 4, 1, 1), 0.0, device=DEV))[0],
                       with_plus, "sigma_up = 0, noise = +0.0")
    with pytest.raises(ops.HipExtensionError):
        ops.euler_step(eps.to(DEV), x.to(DEV), (2.0, -2.0, 0.0), False, 1.0, noise=base.to(DEV))  # noise of another shape
    with pytest.raises(ops.HipExtensionError, match="sigma_hat"):
        ops.euler_step(eps.to(DEV), x.to(DEV), (0.0, -2.0, 0.0), False, 1.0)


# =============================================================================================================================
# the scaled pack
# =============================================================================================================================
PACK_HW = {1: (2, 1, 1), 63: (2, 7, 9), "lap": (1, 724, 725)}  # B, h, w


@pytest.fixture(scope="module")
def pack_inputs():
    g = gen(41)
    return {k: tuple(torch.randn(B, 4, h, w, generator=g) * 3 for _ in range(2)) for k, (B, h, w) in PACK_HW.items()}


@pytest.mark.parametrize("hw", [1, 63, "lap"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_pack_scaled_bit_equal(pack_inputs, dtype, hw):
    from gm_diffusion import hip_ops as ops

    s0, s1 = pack_inputs[hw]
    B, h, w = PACK_HW[hw]
    d0, d1 = tuple(t.to(DEV) for t in (s0, s1))
    div = (14.648818969726562, 1.2345600128173828)  # (1 + sigma^2)^.5 at the top of an SD schedule, and something near 1
    for c1 in (0, 4):
        for cp in (8, 16):
            if hw == "lap":
                assert B * h * w * (cp // 8) > S.LAP_LATENT and (B * h * w * (cp // 8)) % 256 != 0, "not a two-lap launch with a ragged tail"
            for dup in (1, 2):
                a, b = (s0, s1 if c1 else None), (d0, d1 if c1 else None)
                what = f"{dtype} C1={c1} CP={cp} dup={dup} HW={h * w}"
                got = ops.pack_unet_input(b[0], b[1], dup, cp, dtype, div=div)
                S.assert_bit_equal(got, E.pack_scaled_ref(a[0], a[1], div, dup, cp, dtype), what)
                assert not bool(got[:, :, 4 + c1:].any()), what + ": padding channels must be zero"
                if c1:  # each divisor on its own half: swapped divisors give another result, and match the swapped reference
                    sw = ops.pack_unet_input(b[0], b[1], dup, cp, dtype, div=div[::-1])
                    S.assert_bit_equal(sw, E.pack_scaled_ref(a[0], a[1], div[::-1], dup, cp, dtype), what + " swapped divisors")
                    assert int(S.bit_mismatch(sw, got).sum()) > 0
                plain = ops.pack_unet_input(b[0], b[1], dup, cp, dtype)
                S.assert_bit_equal(ops.pack_unet_input(b[0], b[1], dup, cp, dtype, div=(1.0, 1.0)), plain, what + " div = (1, 1) against the plain pack")
                S.assert_bit_equal(plain, S.pack_ref(a[0], a[1], dup, cp, dtype), what + " plain pack")
    out = torch.empty(2 * B, h * w, 8, dtype=dtype, device=DEV)
    assert ops.pack_unet_input(d0, d1, 2, 8, dtype, out=out, div=div) is out
    with pytest.raises(ops.HipExtensionError, match="div1"):
        ops.pack_unet_input(d0, d1, 1, 8, dtype, div=(1.0, 0.0))


def test_unet_pack_input_takes_the_divisors():
    from gm_diffusion.components import UNet2DConditionModel
    from oracle import fixtures

    g = gen(3)
    a, b = torch.randn(1, 4, 16, 16, generator=g), torch.randn(1, 4, 16, 16, generator=g)
    u8 = _hip(UNet2DConditionModel, fixtures.build_unet("tiny", 8))
    got = u8.pack_input((a.to(DEV), b.to(DEV)), dup=2, div=(1.0, 3.5))
    S.assert_bit_equal(got, E.pack_scaled_ref(a, b, (1.0, 3.5), 2, got.shape[-1], got.dtype), "pack_input (cond, x)")
    u4 = _hip(UNet2DConditionModel, fixtures.build_unet("tiny", 4))
    got = u4.pack_input(a.to(DEV), div=3.5)
    S.assert_bit_equal(got, E.pack_scaled_ref(a, None, (3.5, 1.0), 1, got.shape[-1], got.dtype), "pack_input x")
    S.assert_bit_equal(u4.pack_input(a.to(DEV)), S.pack_ref(a, None, 1, got.shape[-1], got.dtype), "pack_input without div")


# =============================================================================================================================
# whole trajectories, scheduler objects
# =============================================================================================================================
@pytest.mark.parametrize("do_cfg", [False, True])
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("mk", [euler, ancestral])
def test_scheduler_device_steps_bit_exact_vs_torch(mk, spacing, karras, do_cfg):
    """gmd_euler_step against the torch expressions of ``_host_step`` over a whole 8-step trajectory (CFG + guidance rescale + x0 +
    ancestral noise from a CPU generator): bit-identical x_prev and x0, through fused_step and through the public step."""
    from gm_diffusion.pipelines import rescale_noise_cfg

    make = lambda: mk(timestep_spacing=spacing, use_karras_sigmas=karras)
    dev_s, host_s, step_s = make(), make(), make()
    for s in (dev_s, host_s, step_s):
        s.set_timesteps(8)
    g = gen(5)
    x = torch.randn(3, 4, 8, 8, generator=g) * host_s.init_noise_sigma
    xd = x.to(DEV)
    gs, gr = 6.5, 0.3
    anc = mk is ancestral
    for i, t in enumerate(dev_s.timesteps.tolist()):
        eps2 = torch.randn(6, 4, 8, 8, generator=g)
        if do_cfg:
            u, c = eps2.chunk(2)
            e = rescale_noise_cfg(u + gs * (c - u), c, guidance_rescale=gr)
            eps_dev = eps2.to(DEV)
        else:
            e = eps2[:3].clone()
            eps_dev = e.to(DEV)
        assert dev_s.input_divisor(t) == host_s.input_divisor(t) == float((host_s.sigmas[i] ** 2 + 1) ** 0.5)
        ref = host_s._host_step(e, t, x, generator=gen(100 + i)) if anc else host_s._host_step(e, t, x)
        kw = lambda: dict(generator=gen(100 + i)) if anc else {}  # a fresh generator per call: each draws the tensor the host step drew
        xd_new, x0_dev = dev_s.fused_step(eps_dev, t, xd, do_cfg, gs, gr if do_cfg else 0.0, want_x0=True, **kw())
        S.assert_bit_equal(xd_new, ref.prev_sample, f"x_prev step {i}")
        S.assert_bit_equal(x0_dev, ref.pred_original_sample, f"x0 step {i}")
        out = step_s.step(e.to(DEV), t, xd, **kw())  # the public step on device tensors: the same kernel without CFG
        S.assert_bit_equal(out.prev_sample, ref.prev_sample, f"step prev_sample step {i}")
        S.assert_bit_equal(out.pred_original_sample, ref.pred_original_sample, f"step pred_original_sample step {i}")
        assert dev_s.step_index == host_s.step_index == step_s.step_index == i + 1
        x, xd = ref.prev_sample, xd_new
    assert float(host_s.sigmas[-1]) == 0.0


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
KINDS = {"euler": (euler, E.RefEulerScheduler), "ancestral": (ancestral, E.RefEulerAncestralScheduler)}


@pytest.fixture(scope="module")
def dual_case():
    """Inputs, ONE HIP dual pipeline (its scheduler is swapped per kind), and dual_loop_sigma's latents per kind (computed once, left
    unchanged).  Default spacing: linspace, whose 8-step timesteps are fractional."""
    from oracle import fixtures

    pe, ne, lat = fixtures.make_inputs(2, 16, 16, cross_dim=64)
    refs = {k: E.dual_loop_sigma(fixtures.build_unet("tiny", 4), fixtures.build_unet("tiny", 8), ref(), pe, ne, lat, STEPS, guidance_scale=7.5,
                                 generator=gen(123)) for k, (_, ref) in KINDS.items()}
    pipe = _dual_pipe(euler(steps_offset=1))
    return pipe, pe, ne, lat, refs


def _run_dual(case, kind, generator, steps=STEPS, **attrs):
    pipe, pe, ne, lat, _ = case
    pipe.scheduler = KINDS[kind][0](steps_offset=1)
    for k, v in attrs.items():
        setattr(pipe, k, v)
    return pipe(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), latents=lat.to(DEV), height=128, width=128,
                num_inference_steps=steps, guidance_scale=7.5, generator=generator, output_type="latent")


@pytest.mark.parametrize("kind", ["euler", "ancestral"])
def test_dual_pipeline_matches_dual_loop_sigma(dual_case, kind):
    """Fused gmd_euler_step + scaled pack under graphs + two streams and eager on one stream, against dual_loop_sigma driven by the
    float64 scheduler of tests/euler_ref.py with the same CPU generator (shared by both schedulers: SDR noise before GM noise)."""
    pipe, pe, ne, lat, refs = dual_case
    rs, rg = refs[kind]
    g = gen(123)
    s1, g1 = _run_dual(dual_case, kind, g, use_hip_graphs=True, overlap_streams=True)
    assert pipe._use_fused(lat.to(DEV), pipe.unet, pipe.scheduler) and pipe.scheduler.step_index == STEPS == pipe.gm_scheduler.step_index
    twin = gen(123)
    for _ in range(2 * STEPS if kind == "ancestral" else 0):  # 2 draws per iteration, the last included (the latents were passed in)
        torch.randn(lat.shape, generator=twin)
    assert torch.equal(g.get_state(), twin.get_state())
    s2, g2 = _run_dual(dual_case, kind, gen(123), use_hip_graphs=False, overlap_streams=False)
    print(f"{kind}: latent RMS sdr={rms(s1, rs):.2e} gm={rms(g1, rg):.2e} (eager: {rms(s2, rs):.2e} {rms(g2, rg):.2e})")
    assert rms(s1, rs) <= RMS_TOL and rms(g1, rg) <= RMS_TOL
    assert rms(s2, rs) <= RMS_TOL and rms(g2, rg) <= RMS_TOL
    assert torch.equal(s1, s2) and torch.equal(g1, g2), "graphs + two streams and eager single stream must agree bit for bit"
    if kind == "ancestral":
        assert rms(s1, rg) > 0.1, "the two latents must NOT have received the same noise"
        # the pre-draw against the per-step draw: the same final latents, bit for bit
        from gm_diffusion.pipelines import StableDiffusionGMPipeline as Base  # _predraw_step_noise reads the ceiling from this class

        old = Base.PREDRAW_NOISE_BYTES
        try:
            Base.PREDRAW_NOISE_BYTES = 0
            assert Base._predraw_step_noise([pipe.scheduler], [1.0], lat.shape, gen(1), "cpu") is None
            s3, g3 = _run_dual(dual_case, kind, gen(123), use_hip_graphs=True, overlap_streams=True)
        finally:
            Base.PREDRAW_NOISE_BYTES = old
        assert torch.equal(s3, s1) and torch.equal(g3, g1)


@pytest.mark.parametrize("kind", ["euler", "ancestral"])
def test_gm_pipeline_matches_oracle(kind):
    """oracle.pipelines.gm_loop scales the concatenated 8-channel tensor (the reference's line): both halves of the pack are divided."""
    from gm_diffusion.components import AutoencoderKL, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionGMPipeline
    from oracle import fixtures
    from oracle import pipelines as OP

    mk, ref_cls = KINDS[kind]
    ou = fixtures.build_unet("tiny", 8)
    pipe = StableDiffusionGMPipeline(
        vae=_hip(AutoencoderKL, fixtures.build_vae("tiny")), text_encoder=None, tokenizer=None, unet=_hip(UNet2DConditionModel, ou),
        scheduler=mk(steps_offset=1), safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    pe, ne, lat = fixtures.make_inputs(1, 16, 16, cross_dim=64)
    sdr_lat = torch.randn(1, 4, 16, 16, generator=gen(77))
    ref = OP.gm_loop(ou, ref_cls(), sdr_lat, pe, ne, lat, STEPS, guidance_scale=7.5, generator=gen(42))

    def run(g):
        pipe.scheduler = mk(steps_offset=1)
        return pipe(sdr_lat.to(DEV), prompt=None, prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), latents=lat.to(DEV),
                    num_inference_steps=STEPS, guidance_scale=7.5, generator=g, output_type="latent").images

    assert pipe._use_fused(lat.to(DEV), pipe.unet, pipe.scheduler)
    g = gen(42)
    out = run(g)
    twin = gen(42)
    for _ in range(STEPS if kind == "ancestral" else 0):
        torch.randn(lat.shape, generator=twin)
    assert torch.equal(g.get_state(), twin.get_state())
    print(f"{kind}: latent RMS {rms(out, ref):.2e}")
    assert rms(out, ref) <= RMS_TOL
    pipe.use_hip_graphs = False
    assert torch.equal(run(gen(42)), out), "graphs and eager launches must agree bit for bit"
    if kind == "ancestral":
        # the pre-draw against the draw inside fused_step: the same final latents bit for bit, the generator advanced alike
        old = StableDiffusionGMPipeline.PREDRAW_NOISE_BYTES
        try:
            StableDiffusionGMPipeline.PREDRAW_NOISE_BYTES = 0
            assert StableDiffusionGMPipeline._predraw_step_noise([pipe.scheduler], [1.0], lat.shape, gen(1), "cpu") is None
            for graphs in (True, False):
                pipe.use_hip_graphs = graphs
                g = gen(42)
                assert torch.equal(run(g), out), f"per-step draw (graphs={graphs}) against the pre-drawn run"
                assert torch.equal(g.get_state(), twin.get_state())
        finally:
            StableDiffusionGMPipeline.PREDRAW_NOISE_BYTES = old
    pipe._use_fused = lambda *args: False  # the generic scheduler-protocol path: scale_model_input on the concatenated tensor
    assert rms(run(gen(42)), ref) <= RMS_TOL


# =============================================================================================================================
# fractional timesteps reach the UNets unchanged
# =============================================================================================================================
def test_dual_pipeline_unets_read_the_fractional_timesteps(dual_case):
    pipe = dual_case[0]
    seen = []
    pipe._step_probe = lambda i, sdr, gm: seen.append((i, pipe.unet._t_dev.clone(), pipe.gm_unet._t_dev.clone()))
    try:
        _run_dual(dual_case, "euler", None, steps=7, use_hip_graphs=True, overlap_streams=True)
    finally:
        pipe._step_probe = None
    ts = pipe.scheduler.timesteps.cpu()
    assert ts.dtype == F32 and len(seen) == 7 and float(ts[1]) == 832.5
    for i, a, b in seen:
        S.assert_bit_equal(a.reshape(()), ts[i], f"SDR UNet timestep {i}")
        S.assert_bit_equal(b.reshape(()), ts[i], f"GM UNet timestep {i}")


def test_gm_pipeline_unet_reads_the_fractional_timesteps():
    from gm_diffusion.components import AutoencoderKL, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionGMPipeline
    from oracle import fixtures

    pipe = StableDiffusionGMPipeline(
        vae=_hip(AutoencoderKL, fixtures.build_vae("tiny")), text_encoder=None, tokenizer=None,
        unet=_hip(UNet2DConditionModel, fixtures.build_unet("tiny", 8)), scheduler=ancestral(steps_offset=1), safety_checker=None,
        feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    pe, ne, lat = fixtures.make_inputs(1, 16, 16, cross_dim=64)
    seen = []

    def cb(p, i, t, kw):
        seen.append((i, t.clone(), p.unet._t_dev.clone()))
        return {}

    pipe(torch.randn(1, 4, 16, 16, generator=gen(7)).to(DEV), prompt=None, prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV),
         latents=lat.to(DEV), num_inference_steps=7, guidance_scale=7.5, generator=gen(1), output_type="latent", callback_on_step_end=cb)
    ts = pipe.scheduler.timesteps.cpu()
    assert ts.dtype == F32 and len(seen) == 7 and float(ts[2]) == 666.0 and float(ts[1]) == 832.5
    for i, t, buf in seen:
        S.assert_bit_equal(buf.reshape(()), ts[i], f"UNet timestep {i}")
        S.assert_bit_equal(t.cpu(), ts[i], f"loop timestep {i}")


# =============================================================================================================================
# untouched paths
# =============================================================================================================================
def test_pndm_keeps_the_plain_pack(dual_case, monkeypatch):
    """With PNDM the dual pipeline's launches are the parent's: every input pack goes through hip_ops.pack_unet_input WITHOUT ``div``
    (the plain gmd_pack_unet_input), gmd_euler_step is never called, and the sigma-space run differs from it."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion.components import PNDMScheduler

    pipe, pe, ne, lat, _ = dual_case
    calls, real_pack, real_step = [], ops.pack_unet_input, ops.euler_step

    def pack(*a, **kw):
        calls.append(("pack", "div" in kw))
        return real_pack(*a, **kw)

    def step(*a, **kw):
        calls.append(("euler_step", True))
        return real_step(*a, **kw)

    monkeypatch.setattr(ops, "pack_unet_input", pack)
    monkeypatch.setattr(ops, "euler_step", step)
    pipe.scheduler = PNDMScheduler(skip_prk_steps=True, steps_offset=1, **SD)
    pipe.use_hip_graphs, pipe.overlap_streams = True, True
    run = lambda: pipe(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), latents=lat.to(DEV), height=128, width=128,
                       num_inference_steps=4, guidance_scale=7.5, output_type="latent")
    a = run()
    assert len([c for c in calls if c[0] == "pack"]) == 2 * len(pipe.scheduler.timesteps) and not any(flag for _, flag in calls), calls
    calls.clear()
    pipe.scheduler = euler(steps_offset=1)
    b = run()
    assert all(flag for _, flag in calls) and ("euler_step", True) in calls and len(calls) == 4 * 4
    assert rms(a[0], b[0]) > 0.1
