"""GPU: gmd_lms_step and components.LMSDiscreteScheduler on the device -- the second grid-stride lap bit for bit through the raw C ABI at
every order, the write footprint, edge values, whole trajectories of the scheduler object against its own torch expressions
(bit-identical, history included, also when the caller's eps buffer is overwritten), both pipelines at tiny width against the loops driven
by the float64 scheduler of tests/lms_ref.py at every iteration, and the launches of the neighbouring schedulers, which must not change."""
import pytest
import torch

import euler_ref as E
import lms_ref as L
import small_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
RMS_TOL = 1e-3  # the project's gate (tests/test_euler_gpu.py, tests/test_ddim_gpu.py): "within 1e-3 latent RMS"
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SPACINGS = ("linspace", "leading", "trailing")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ptr(t):
    return None if t is None else t.data_ptr()


def call(*args):
    from gm_diffusion._native import lib

    rc = lib().gmd_lms_step(*args, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (rc, lib().gmd_last_error())


def nan_dev(shape):
    return torch.full(shape, float("nan"), dtype=F32, device=DEV)


def rms(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b) ** 2).mean().sqrt())


def lms(**kw):
    from gm_diffusion.components import LMSDiscreteScheduler

    return LMSDiscreteScheduler(**SD, **kw)


# =============================================================================================================================
# the second lap, bit for bit, through the raw C ABI
# =============================================================================================================================
LAT_B, LAT_SHAPE = 2, (4, 257, 257)
LAT_CHW = 4 * 257 * 257
GS, GR = 7.5, 0.7
SIGMA, CS = 3.25, (-1.9, 1.3, -0.7, 0.2)  # alternating signs, as the real coefficients have


@pytest.fixture(scope="module")
def lap_inputs():
    """Inputs of the two-lap launches, drawn once and left unchanged (both do_cfg cases read the first B samples of eps_in)."""
    g = gen(31)
    eps_in = torch.randn((2 * LAT_B,) + LAT_SHAPE, generator=g)
    x = torch.randn((LAT_B,) + LAT_SHAPE, generator=g)
    hist = [torch.randn((LAT_B,) + LAT_SHAPE, generator=g) for _ in range(3)]  # three distinct history tensors
    ratio = torch.tensor([0.25, 3.0])  # two very different entries: the lap boundary falls inside sample 1
    return eps_in, x, hist, ratio, tuple(t.to(DEV) for t in (eps_in, x, *hist, ratio))


@pytest.mark.parametrize("do_cfg", [False, True])
def test_lms_step_second_lap(lap_inputs, do_cfg):
    n = LAT_B * LAT_CHW
    assert n == 528392 and n > S.LAP_LATENT and LAT_CHW < S.LAP_LATENT < n and n % 256 != 0, "not a two-lap launch with a ragged tail"
    eps_all, x, hist, ratio, (d_eps, d_x, d_h1, d_h2, d_h3, d_ratio) = lap_inputs
    d_hist = [d_h1, d_h2, d_h3]
    poison = nan_dev((LAT_B,) + LAT_SHAPE)  # handed in for every history slot beyond order - 1: it must never be read
    nan_ratio = nan_dev((LAT_B,))  # handed to the do_cfg == 0 launches; bound to a name so that it outlives them
    eps_in = eps_all if do_cfg else eps_all[:LAT_B]
    for use_ratio in ((False, True) if do_cfg else (False,)):
        eps = S.guided_eps(eps_in, LAT_B, do_cfg, GS, ratio if use_ratio else None, GR)
        # a do_cfg == 0 launch must not read the ratio: it gets a NaN buffer
        r_ptr = ptr(d_ratio) if use_ratio else (None if do_cfg else ptr(nan_ratio))
        for order in (1, 2, 3, 4):
            refs = L.lms_step_f32(eps, x, (SIGMA,) + CS[:order], hist[:order - 1])
            assert all(bool(torch.isfinite(r).all()) for r in refs)
            hp = [ptr(d_hist[j]) if j < order - 1 else ptr(poison) for j in range(3)]
            cs = CS[:order] + (float("nan"),) * (4 - order)  # nor is a coefficient beyond the order
            for want in (True, False):
                od, op, o0 = (nan_dev((LAT_B,) + LAT_SHAPE) for _ in range(3))
                call(ptr(d_eps), ptr(d_x), *hp, LAT_B, LAT_CHW, int(do_cfg), GS, r_ptr, GR, order, SIGMA, *cs, ptr(od), ptr(op),
                     ptr(o0) if want else None)
                torch.cuda.synchronize()
                what = f"lms_step order={order} ratio={use_ratio} pred_x0={want} do_cfg={do_cfg}"
                S.assert_bit_equal(od, refs[0], what + " d_out")
                S.assert_bit_equal(op, refs[1], what + " x_prev")
                if want:
                    S.assert_bit_equal(o0, refs[2], what + " pred_x0")
                else:
                    assert bool(torch.isnan(o0).all()), what + ": an output that was not asked for was written"
    # the orders differ from each other on these inputs: a kernel that ignored `order` could not pass all four
    outs = [L.lms_step_f32(eps, x, (SIGMA,) + CS[:k], hist[:k - 1])[1] for k in (1, 2, 3, 4)]
    assert all(int(S.bit_mismatch(outs[k], outs[k + 1]).sum()) > n // 2 for k in range(3))


# =============================================================================================================================
# write footprint
# =============================================================================================================================
GUARD = 16384  # float32 elements of sentinel before and after every output


@pytest.mark.parametrize("do_cfg", [False, True])
def test_lms_step_stores_only_its_three_tensors(do_cfg):
    """B = 3 latents of chw = 3 * 7 * 5 = 105 elements (no multiple of 4 or 64): guard bands of a sentinel around d_out, x_prev and
    pred_x0 stay untouched, every element inside is written, and eps_in, x and the three history tensors are left as they were."""
    B, shape, chw = 3, (3, 3, 7, 5), 105
    n = B * chw
    g = gen(12)
    eps_in = torch.randn((2 * B if do_cfg else B,) + shape[1:], generator=g)
    x = torch.randn(shape, generator=g)
    hist = [torch.randn(shape, generator=g) for _ in range(3)]
    eps = S.guided_eps(eps_in, B, do_cfg, GS)
    refs = L.lms_step_f32(eps, x, (SIGMA,) + CS, hist)
    sentinel = -12345.678
    bufs = [torch.full((2 * GUARD + n,), sentinel, dtype=F32, device=DEV) for _ in range(3)]
    outs = [b[GUARD:GUARD + n] for b in bufs]
    d_eps, d_x, d_hist = eps_in.to(DEV), x.to(DEV), [h.to(DEV) for h in hist]
    call(ptr(d_eps), ptr(d_x), *(ptr(h) for h in d_hist), B, chw, int(do_cfg), GS, None, 0.0, 4, SIGMA, *CS, *(ptr(o) for o in outs))
    torch.cuda.synchronize()
    for b, o, r, nm in zip(bufs, outs, refs, ("d_out", "x_prev", "pred_x0")):
        assert bool((b[:GUARD] == sentinel).all()) and bool((b[GUARD + n:] == sentinel).all()), f"{nm}: a guard band changed"
        assert not bool((o == sentinel).any()), f"{nm}: an element inside was not written"
        S.assert_bit_equal(o.view(shape), r, f"lms_step footprint {nm} do_cfg={do_cfg}")
    for d, h, nm in ((d_eps, eps_in, "eps_in"), (d_x, x, "x"), (d_hist[0], hist[0], "d1"), (d_hist[1], hist[1], "d2"), (d_hist[2], hist[2], "d3")):
        S.assert_bit_equal(d, h, f"input {nm} changed")


# =============================================================================================================================
# edge values, bit-exact
# =============================================================================================================================
def _dev_step(eps, x, coefs, hist=()):
    from gm_diffusion import hip_ops as ops

    order = len(coefs) - 1
    return ops.lms_step(eps.to(DEV), x.to(DEV), order, tuple(coefs) + (0.0,) * (4 - order), False, 1.0, hist=[h.to(DEV) for h in hist],
                        want_pred_x0=True)


def _check(eps, x, coefs, hist, what):
    ref = L.lms_step_f32(eps, x, coefs, hist)
    got = _dev_step(eps, x, coefs, hist)
    for g_, r_, nm in zip(got, ref, ("d", "x_prev", "pred_x0")):
        S.assert_bit_equal(g_, r_, f"{what} {nm}")


def test_lms_step_edge_values():
    """sigma at 2^-20 and 2^10; a zero and a negative coefficient; history entries of +-0.0; the last step of a real schedule
    (sigma_next = 0); and the sign of a zero sum: with x = -0.0, eps = +0.0 and c0 < 0, c0 d is -0.0, torch's sum() gives
    0 + (-0.0) = +0.0 and x_prev = -0.0 + 0.0 = +0.0, where a kernel without the leading 0.0f would return -0.0."""
    from gm_diffusion import hip_ops as ops

    g = gen(8)
    shape = (2, 4, 5, 3)
    x = torch.randn(shape, generator=g)
    x.view(-1)[:6] = torch.tensor([0.0, -0.0, 0.0, -0.0, 1.0, -1.0])
    eps = torch.randn(shape, generator=g)
    eps.view(-1)[:6] = torch.tensor([0.0, 0.0, -0.0, -0.0, 0.0, -0.0])
    hist = [torch.randn(shape, generator=g) for _ in range(3)]
    for h, pat in zip(hist, ([0.0, -0.0, -0.0, 0.0], [-0.0, -0.0, 0.0, 0.0], [-0.0, 0.0, -0.0, 0.0])):
        h.view(-1)[:4] = torch.tensor(pat)
        h.view(-1)[8:12] = torch.tensor(pat)
    for sg in (2.0 ** -20, 2.0 ** 10):
        for cs in ((-sg,), (0.0,), (-0.0,), (-1.5 * sg, 0.5 * sg), (0.0, -0.25 * sg), (-2.0 * sg, 1.5 * sg, -0.5 * sg),
                   (-2.25 * sg, 2.5 * sg, -1.5 * sg, 0.25 * sg), (0.0, 0.0, 0.0, 0.0), (-0.0, 0.0, -0.0, -sg)):
            _check(eps, x, (sg,) + cs, hist[:len(cs) - 1], f"sigma={sg} coefs={cs}")
    # the last step of a real schedule: sigma_next == 0, the coefficients sum to -sigma
    s = lms(use_karras_sigmas=True)
    s.set_timesteps(8)
    cs = tuple(s.get_lms_coefficient(4, 7, j) for j in range(4))
    assert float(s.sigmas[8]) == 0.0 and abs(sum(cs) + float(s.sigmas[7])) < 1e-12
    _check(eps, x, (float(s.sigmas[7]),) + cs, hist, "last step")
    # the sign of a zero sum at order 1
    xz = torch.tensor([-0.0, 0.0, -0.0, 1.5]).reshape(1, 4, 1, 1)
    ez = torch.tensor([0.0, 0.0, -0.0, -0.5]).reshape(1, 4, 1, 1)
    coefs = (2.0, -2.0)
    ref = L.lms_step_f32(ez, xz, coefs)[1]
    sg_, c0 = L._s(coefs[0]), L._s(coefs[1])
    without_zero = xz + c0 * ((xz - (xz - sg_ * ez)) / sg_)  # what a sum started from the first product gives
    assert torch.equal(ref, without_zero) and int(S.bit_mismatch(ref, without_zero).sum()) >= 1, "the test's inputs must tell +0.0 from -0.0"
    assert ref.view(-1)[0].item() == 0.0 and not torch.signbit(ref.view(-1)[0]) and bool(torch.signbit(without_zero.view(-1)[0]))
    S.assert_bit_equal(_dev_step(ez, xz, coefs)[1], ref, "0 + (-0.0) at order 1")
    # the wrapper's own refusals
    xd, ed = x.to(DEV), eps.to(DEV)
    with pytest.raises(ops.HipExtensionError, match="earlier derivatives"):
        ops.lms_step(ed, xd, 3, (1.0, -0.5, 0.1, 0.1, 0.0), False, 1.0, hist=[hist[0].to(DEV)])
    with pytest.raises(ops.HipExtensionError, match="shape"):
        ops.lms_step(ed, xd, 2, (1.0, -0.5, 0.1, 0.0, 0.0), False, 1.0, hist=[torch.zeros(1, 4, 5, 3, device=DEV)])
    with pytest.raises(ops.HipExtensionError, match="sigma"):
        ops.lms_step(ed, xd, 1, (0.0, -0.5, 0.0, 0.0, 0.0), False, 1.0)


# =============================================================================================================================
# whole trajectories, scheduler objects
# =============================================================================================================================
@pytest.mark.parametrize("do_cfg", [False, True])
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("spacing", SPACINGS)
def test_scheduler_device_steps_bit_exact_vs_torch(spacing, karras, do_cfg):
    """gmd_lms_step against the torch expressions of ``_host_step`` over whole 8-step trajectories (orders 1, 2, 3, 4, 4, 4, 4, 4; CFG
    with guidance_rescale = 0.7): bit-identical prev_sample, pred_original_sample and kept derivatives, the host being fed the guided
    eps the kernel forms (the per-sample ratio is the device's own).  Second pass: eps_in is overwritten with NaN right after each step --
    the history must be the scheduler's own tensors, not views of the caller's buffer (a graph's static output, overwritten by the next
    replay)."""
    from gm_diffusion import hip_ops as ops

    gs, gr = 6.5, 0.7
    for poison in (False, True):
        make = lambda: lms(timestep_spacing=spacing, use_karras_sigmas=karras)
        dev_s, host_s, step_s = make(), make(), make()
        for s in (dev_s, host_s, step_s):
            s.set_timesteps(8)
        g = gen(5)
        x = torch.randn(3, 4, 8, 8, generator=g) * host_s.init_noise_sigma
        xd = x.to(DEV)
        for i, t in enumerate(dev_s.timesteps.tolist()):
            eps2 = torch.randn(6, 4, 8, 8, generator=g)
            if do_cfg:
                eps_dev = eps2.to(DEV)
                e = S.guided_eps(eps2, 3, True, gs, ops.cfg_std_ratio(eps_dev, gs).cpu(), gr)
            else:
                e = eps2[:3].clone()
                eps_dev = e.to(DEV)
            ref = host_s._host_step(e, t, x)
            xd_new, x0_dev = dev_s.fused_step(eps_dev, t, xd, do_cfg, gs, gr if do_cfg else 0.0, want_x0=True)
            e_dev = e.to(DEV)
            out = step_s.step(e_dev, t, xd)  # the public step on device tensors: the same kernel without CFG
            if poison:
                eps_dev.fill_(float("nan"))
                e_dev.fill_(float("nan"))
            S.assert_bit_equal(xd_new, ref.prev_sample, f"x_prev step {i}")
            S.assert_bit_equal(x0_dev, ref.pred_original_sample, f"x0 step {i}")
            S.assert_bit_equal(out.prev_sample, ref.prev_sample, f"step prev_sample step {i}")
            S.assert_bit_equal(out.pred_original_sample, ref.pred_original_sample, f"step pred_original_sample step {i}")
            assert dev_s.step_index == host_s.step_index == step_s.step_index == i + 1
            assert len(dev_s.derivatives) == len(host_s.derivatives) == len(step_s.derivatives) == min(i + 1, 4)
            for a, b, c in zip(dev_s.derivatives, step_s.derivatives, host_s.derivatives):
                assert a.is_cuda and b.is_cuda
                S.assert_bit_equal(a, c, f"kept derivative (fused_step) after step {i}")
                S.assert_bit_equal(b, c, f"kept derivative (step) after step {i}")
            x, xd = ref.prev_sample, xd_new
        assert float(host_s.sigmas[-1]) == 0.0 and bool(torch.isfinite(xd).all())


# =============================================================================================================================
# pipelines at tiny width
# =============================================================================================================================
def _hip(model_cls, oracle_model):
    m = model_cls(**vars(oracle_model.config))
    m.load_state_dict(oracle_model.state_dict())
    return m.to(DEV, F32)


STEPS = 8  # orders ramp 1 -> 4, then four steady steps


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


@pytest.fixture(scope="module")
def dual_case():
    """Inputs, ONE HIP dual pipeline, and dual_loop_sigma's latents of every iteration under RefLMSScheduler (computed once, left
    unchanged).  Default spacing: linspace, whose 8-step timesteps are fractional."""
    from oracle import fixtures

    pe, ne, lat = fixtures.make_inputs(2, 16, 16, cross_dim=64)
    record = []
    E.dual_loop_sigma(fixtures.build_unet("tiny", 4), fixtures.build_unet("tiny", 8), L.RefLMSScheduler(), pe, ne, lat, STEPS, guidance_scale=7.5,
                      record=record)
    return _dual_pipe(lms(steps_offset=1)), pe, ne, lat, record


def _run_dual(case, scheduler, steps=STEPS, **attrs):
    pipe, pe, ne, lat, _ = case
    pipe.scheduler = scheduler
    for k, v in attrs.items():
        setattr(pipe, k, v)
    return pipe(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), latents=lat.to(DEV), height=128, width=128,
                num_inference_steps=steps, guidance_scale=7.5, generator=gen(1), output_type="latent")


def test_dual_pipeline_matches_dual_loop_sigma(dual_case):
    """Fused gmd_lms_step + scaled pack under graphs + two streams, against dual_loop_sigma driven by the float64 scheduler of
    tests/lms_ref.py: latent RMS within the gate at EVERY iteration, both UNets reading the fractional float32 timesteps; then eager on
    one stream, bit for bit the same."""
    pipe, pe, ne, lat, record = dual_case
    seen = []
    pipe._step_probe = lambda i, sdr, gm: seen.append((sdr.clone(), gm.clone(), pipe.unet._t_dev.clone(), pipe.gm_unet._t_dev.clone()))
    try:
        s1, g1 = _run_dual(dual_case, lms(steps_offset=1), use_hip_graphs=True, overlap_streams=True)
    finally:
        pipe._step_probe = None
    assert pipe._use_fused(lat.to(DEV), pipe.unet, pipe.scheduler) and pipe.scheduler.step_index == STEPS == pipe.gm_scheduler.step_index
    assert len(pipe.scheduler.derivatives) == 4 == len(pipe.gm_scheduler.derivatives)
    assert pipe.scheduler.derivatives[0] is not pipe.gm_scheduler.derivatives[0]
    ts = pipe.scheduler.timesteps.cpu()
    assert ts.dtype == F32 and len(seen) == STEPS == len(record) and float(ts[1]) != int(ts[1])
    for i, ((sdr, gm, ta, tb), (rs, rg)) in enumerate(zip(seen, record)):
        print(f"iteration {i}: latent RMS sdr={rms(sdr, rs):.2e} gm={rms(gm, rg):.2e}")
        assert rms(sdr, rs) <= RMS_TOL and rms(gm, rg) <= RMS_TOL, f"iteration {i}"
        S.assert_bit_equal(ta.reshape(()), ts[i], f"SDR UNet timestep {i}")
        S.assert_bit_equal(tb.reshape(()), ts[i], f"GM UNet timestep {i}")
    assert torch.equal(seen[-1][0], s1) and torch.equal(seen[-1][1], g1)
    s2, g2 = _run_dual(dual_case, lms(steps_offset=1), use_hip_graphs=False, overlap_streams=False)
    assert torch.equal(s1, s2) and torch.equal(g1, g2), "graphs + two streams and eager single stream must agree bit for bit"
    s3, g3 = _run_dual(dual_case, lms(steps_offset=1), use_hip_graphs=True, overlap_streams=True)  # without the probe's synchronisation
    assert torch.equal(s1, s3) and torch.equal(g1, g3)


def test_gm_pipeline_matches_oracle():
    """oracle.pipelines.gm_loop scales the concatenated 8-channel tensor (the reference's line): both halves of the pack are divided."""
    from gm_diffusion.components import AutoencoderKL, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionGMPipeline
    from oracle import fixtures
    from oracle import pipelines as OP

    ou = fixtures.build_unet("tiny", 8)
    pipe = StableDiffusionGMPipeline(
        vae=_hip(AutoencoderKL, fixtures.build_vae("tiny")), text_encoder=None, tokenizer=None, unet=_hip(UNet2DConditionModel, ou),
        scheduler=lms(steps_offset=1), safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    pe, ne, lat = fixtures.make_inputs(1, 16, 16, cross_dim=64)
    sdr_lat = torch.randn(1, 4, 16, 16, generator=gen(77))
    record = []
    OP.gm_loop(ou, L.RefLMSScheduler(), sdr_lat, pe, ne, lat, STEPS, guidance_scale=7.5, record=record)
    seen = []

    def cb(p, i, t, kw):
        seen.append((kw["latents"].clone(), t.clone(), p.unet._t_dev.clone()))
        return {}

    def run(**kw):
        pipe.scheduler = lms(steps_offset=1)
        return pipe(sdr_lat.to(DEV), prompt=None, prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), latents=lat.to(DEV),
                    num_inference_steps=STEPS, guidance_scale=7.5, generator=gen(42), output_type="latent", **kw).images

    assert pipe._use_fused(lat.to(DEV), pipe.unet, pipe.scheduler) and pipe.use_hip_graphs
    out = run(callback_on_step_end=cb)
    ts = pipe.scheduler.timesteps.cpu()
    assert len(seen) == STEPS == len(record) and ts.dtype == F32 and float(ts[1]) != int(ts[1])
    for i, ((got, t, buf), ref) in enumerate(zip(seen, record)):
        print(f"iteration {i}: latent RMS {rms(got, ref):.2e}")
        assert rms(got, ref) <= RMS_TOL, f"iteration {i}"
        S.assert_bit_equal(buf.reshape(()), ts[i], f"UNet timestep {i}")
        S.assert_bit_equal(t.cpu(), ts[i], f"loop timestep {i}")
    assert torch.equal(seen[-1][0], out) and pipe.scheduler.step_index == STEPS and len(pipe.scheduler.derivatives) == 4
    pipe.use_hip_graphs = False
    assert torch.equal(run(), out), "graphs and eager launches must agree bit for bit"
    pipe._use_fused = lambda *args: False  # the generic scheduler-protocol path: scale_model_input on the concatenated tensor
    assert rms(run(), record[-1]) <= RMS_TOL


# =============================================================================================================================
# untouched paths
# =============================================================================================================================
def test_neighbours_never_launch_lms_step_and_lms_launches_it_once_per_step(dual_case, monkeypatch):
    """With gmd_lms_step and gmd_euler_step wrapped by counters: a PNDM run and an Euler run of the dual pipeline call gmd_lms_step zero
    times; an LMS run calls it once per scheduler per step (2 x steps) and gmd_euler_step zero times."""
    from gm_diffusion._native import lib
    from gm_diffusion.components import EulerDiscreteScheduler, PNDMScheduler

    pipe = dual_case[0]
    counts = {"gmd_lms_step": 0, "gmd_euler_step": 0}

    def counted(name):
        real = getattr(lib(), name)

        def f(*a):
            counts[name] += 1
            return real(*a)

        return f

    for name in counts:
        monkeypatch.setattr(lib(), name, counted(name))
    steps = 5
    _run_dual(dual_case, PNDMScheduler(skip_prk_steps=True, steps_offset=1, **SD), steps=steps, use_hip_graphs=True, overlap_streams=True)
    assert counts == {"gmd_lms_step": 0, "gmd_euler_step": 0}
    _run_dual(dual_case, EulerDiscreteScheduler(steps_offset=1, **SD), steps=steps, use_hip_graphs=True, overlap_streams=True)
    assert counts == {"gmd_lms_step": 0, "gmd_euler_step": 2 * steps}
    counts["gmd_euler_step"] = 0
    _run_dual(dual_case, lms(steps_offset=1), steps=steps, use_hip_graphs=True, overlap_streams=True)
    assert counts == {"gmd_lms_step": 2 * steps, "gmd_euler_step": 0}
