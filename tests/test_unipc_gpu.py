"""GPU: gmd_unipc_step and components.UniPCMultistepScheduler on the device -- the second grid-stride lap bit for bit through the raw C
ABI at every corrector x predictor order, the write footprint, whole trajectories of the scheduler object against its own torch
expressions (bit-identical, history and last_sample included, also when the caller's eps and sample buffers are overwritten), both
pipelines at tiny width against the loops driven by the float64 scheduler of tests/unipc_ref.py at every iteration, and the launches of
the neighbouring schedulers, which must not change."""
import pytest
import torch

import small_ref as S
import unipc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
RMS_TOL = 1e-3  # the project's gate (tests/test_lms_gpu.py, tests/test_euler_gpu.py): "within 1e-3 latent RMS"
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SPACINGS = ("linspace", "leading", "trailing")
NAN = float("nan")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ptr(t):
    return None if t is None else t.data_ptr()


def call(*args):
    from gm_diffusion._native import lib

    rc = lib().gmd_unipc_step(*args, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (rc, lib().gmd_last_error())


def nan_dev(shape):
    return torch.full(shape, NAN, dtype=F32, device=DEV)


def rms(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b) ** 2).mean().sqrt())


def unipc(**kw):
    from gm_diffusion.components import UniPCMultistepScheduler

    return UniPCMultistepScheduler(**SD, **kw)


# =============================================================================================================================
# the second lap, bit for bit, through the raw C ABI
# =============================================================================================================================
LAT_B, LAT_SHAPE = 2, (4, 257, 257)
LAT_CHW = 4 * 257 * 257
GS, GR = 7.5, 0.7
# sigma_s, alpha_s | c_x, c_m, c_b, c_rho1..3, c_r1, c_r2 | p_x, p_m, p_b, p_rho1, p_rho2, p_r1, p_r2 | sqrt_alpha, sqrt_one_minus_alpha
HEAD, CORR, PRED, TAIL = (0.83, 0.55), (0.9, -0.31, -0.37, 0.21, -0.34, 0.47, -1.3, -2.6), (0.78, -0.42, -0.45, 0.52, -0.13, -1.1, -2.3), (0.6, 0.8)
ORDERS = [(p, q) for p in (0, 1, 2, 3) for q in (1, 2, 3)]


def coefs_for(p, q, fill=NAN):
    """The 19 floats with ``fill`` in every slot the orders do not use: c_rho slots p.., c_r slots p - 1.., all eight at p = 0; p_b at
    q = 1, p_rho and p_r slots q - 1..  The corrector's rho multiplying (x0 - h1) is c_rho<p>."""
    c = list(CORR[:3]) + [CORR[3 + k] if k < p else fill for k in range(3)] + [CORR[6 + k] if k < p - 1 else fill for k in range(2)]
    if p == 0:
        c = [fill] * 8
    d = [PRED[0], PRED[1], PRED[2] if q > 1 else fill] + [PRED[3 + k] if k < q - 1 else fill for k in range(2)]
    d += [PRED[5 + k] if k < q - 1 else fill for k in range(2)]
    return list(HEAD) + c + d + list(TAIL)


@pytest.fixture(scope="module")
def lap_inputs():
    """Inputs of the two-lap launches, drawn once and left unchanged (both do_cfg cases read the first B samples of eps_in)."""
    g = gen(31)
    eps_in = torch.randn((2 * LAT_B,) + LAT_SHAPE, generator=g)
    x, last = (torch.randn((LAT_B,) + LAT_SHAPE, generator=g) for _ in range(2))
    hist = [torch.randn((LAT_B,) + LAT_SHAPE, generator=g) for _ in range(3)]
    ratio = torch.tensor([0.25, 3.0])  # two very different entries: the lap boundary falls inside sample 1
    return eps_in, x, last, hist, ratio, tuple(t.to(DEV) for t in (eps_in, x, last, *hist, ratio))


@pytest.mark.parametrize("do_cfg", [False, True])
def test_unipc_step_second_lap(lap_inputs, do_cfg):
    n = LAT_B * LAT_CHW
    assert n == 528392 and n > S.LAP_LATENT and LAT_CHW < S.LAP_LATENT < n and n % 256 != 0, "not a two-lap launch with a ragged tail"
    eps_all, x, last, hist, ratio, (d_eps, d_x, d_last, d_h1, d_h2, d_h3, d_ratio) = lap_inputs
    d_hist = [d_h1, d_h2, d_h3]
    poison = nan_dev((LAT_B,) + LAT_SHAPE)  # handed in for every history slot and last_sample beyond the orders: never read
    nan_ratio = nan_dev((LAT_B,))  # handed to the do_cfg == 0 launches; bound to a name so that it outlives them
    eps_in = eps_all if do_cfg else eps_all[:LAT_B]
    for use_ratio in ((False, True) if do_cfg else (False,)):
        eps = S.guided_eps(eps_in, LAT_B, do_cfg, GS, ratio if use_ratio else None, GR)
        r_ptr = ptr(d_ratio) if use_ratio else (None if do_cfg else ptr(nan_ratio))
        for p, q in ORDERS:
            need = max(p, q - 1)
            cs = coefs_for(p, q)
            refs = R.unipc_step_f32(eps, x, p, q, cs, last if p else None, hist[:need])
            assert all(bool(torch.isfinite(r).all()) for r in refs)
            hp = [ptr(d_hist[j]) if j < need else ptr(poison) for j in range(3)]
            for want in (True, False):
                outs = [nan_dev((LAT_B,) + LAT_SHAPE) for _ in range(4)]
                call(ptr(d_eps), ptr(d_x), ptr(d_last) if p else ptr(poison), *hp, LAT_B, LAT_CHW, int(do_cfg), GS, r_ptr, GR, p, q, *cs,
                     *(ptr(o) for o in outs[:3]), ptr(outs[3]) if want else None)
                torch.cuda.synchronize()
                what = f"unipc_step corrector={p} predictor={q} ratio={use_ratio} x0={want} do_cfg={do_cfg}"
                for o, r, nm in zip(outs[:3], refs, ("m0_out", "x_corr", "x_prev")):
                    S.assert_bit_equal(o, r, f"{what} {nm}")
                if want:
                    S.assert_bit_equal(outs[3], refs[3], what + " x0")
                else:
                    assert bool(torch.isnan(outs[3]).all()), what + ": an output that was not asked for was written"
    # the twelve order combinations differ from each other on these inputs: a kernel that ignored an order could not pass them all
    prevs = [R.unipc_step_f32(eps, x, p, q, coefs_for(p, q), last, hist)[2] for p, q in ORDERS]
    for a in range(len(ORDERS)):
        for b in range(a + 1, len(ORDERS)):
            assert int(S.bit_mismatch(prevs[a], prevs[b]).sum()) > n // 2, (ORDERS[a], ORDERS[b])


# =============================================================================================================================
# write footprint
# =============================================================================================================================
GUARD = 16384  # float32 elements of sentinel before and after every output


@pytest.mark.parametrize("B,shape", [(1, (3, 5, 7)), (LAT_B, LAT_SHAPE)])
def test_unipc_step_stores_only_its_four_tensors(B, shape):
    """Full order (corrector 3, predictor 3, CFG, the pipeline's x0) at a ragged size of 3 * 5 * 7 = 105 elements and at the two-lap
    size: guard bands of a sentinel around m0_out, x_corr, x_prev and x0 stay untouched, every element inside is written, and the
    inputs are left as they were."""
    full = (B,) + shape
    chw = shape[0] * shape[1] * shape[2]
    n = B * chw
    g = gen(12)
    eps_in = torch.randn((2 * B,) + shape, generator=g)
    x, last = (torch.randn(full, generator=g) for _ in range(2))
    hist = [torch.randn(full, generator=g) for _ in range(3)]
    cs = coefs_for(3, 3)
    refs = R.unipc_step_f32(S.guided_eps(eps_in, B, True, GS), x, 3, 3, cs, last, hist)
    sentinel = -12345.678
    bufs = [torch.full((2 * GUARD + n,), sentinel, dtype=F32, device=DEV) for _ in range(4)]
    outs = [b[GUARD:GUARD + n] for b in bufs]
    ins = [t.to(DEV) for t in (eps_in, x, last, *hist)]
    call(*(ptr(t) for t in ins), B, chw, 1, GS, None, 0.0, 3, 3, *cs, *(ptr(o) for o in outs))
    torch.cuda.synchronize()
    for b, o, r, nm in zip(bufs, outs, refs, ("m0_out", "x_corr", "x_prev", "x0")):
        assert bool((b[:GUARD] == sentinel).all()) and bool((b[GUARD + n:] == sentinel).all()), f"{nm}: a guard band changed"
        assert not bool((o == sentinel).any()), f"{nm}: an element inside was not written"
        S.assert_bit_equal(o.view(full), r, f"unipc_step footprint {nm}")
    for d, h, nm in zip(ins, (eps_in, x, last, *hist), ("eps_in", "x", "last_sample", "h1", "h2", "h3")):
        S.assert_bit_equal(d, h, f"input {nm} changed")


# =============================================================================================================================
# whole trajectories, scheduler objects
# =============================================================================================================================
@pytest.mark.parametrize("solver_type", ["bh1", "bh2"])
@pytest.mark.parametrize("solver_order", [1, 2, 3])
def test_scheduler_device_steps_bit_exact_vs_torch(solver_order, solver_type):
    """gmd_unipc_step against the torch expressions of ``_host_step`` over whole 8-step trajectories (three spacings x disable_corrector
    [] and [0, 3]; CFG with guidance_rescale = 0.7 through ``fused_step``, no CFG through the public ``step``): bit-identical prev_sample,
    kept x0 predictions and last_sample, the host being fed the guided eps the kernel forms (the per-sample ratio is the device's own).
    Second pass: the caller's eps and sample buffers are overwritten with NaN right after each call -- the history must be the kernel's own
    copies, not views of a graph's static output or of the caller's latents."""
    from gm_diffusion import hip_ops as ops

    gs, gr, shape = 6.5, 0.7, (2, 4, 24, 40)
    for spacing in SPACINGS:
        for disable in ([], [0, 3]):
            for poison in (False, True):
                make = lambda: unipc(solver_order=solver_order, solver_type=solver_type, timestep_spacing=spacing, disable_corrector=disable)
                dev_s, host_s, step_s = make(), make(), make()
                for s in (dev_s, host_s, step_s):
                    s.set_timesteps(8)
                g = gen(5)
                x = torch.randn(shape, generator=g)
                xd = x.to(DEV)
                for i, t in enumerate(dev_s.timesteps.tolist()):
                    eps2 = torch.randn((4,) + shape[1:], generator=g)
                    eps_dev = eps2.to(DEV)
                    e = S.guided_eps(eps2, 2, True, gs, ops.cfg_std_ratio(eps_dev, gs).cpu(), gr)
                    a = host_s.alphas_cumprod[int(t)]
                    x0_ref = (x - (1 - a).sqrt() * e) / a.sqrt()
                    ref = host_s._host_step(e, t, x)
                    xd_in, e_dev = xd.clone(), e.to(DEV)
                    xd_new, x0_dev = dev_s.fused_step(eps_dev, t, xd, True, gs, gr, want_x0=True)
                    out = step_s.step(e_dev, t, xd_in).prev_sample  # the public step on device tensors: the same kernel without CFG
                    if poison:
                        for buf in (eps_dev, e_dev, xd, xd_in):
                            buf.fill_(NAN)
                    what = f"order {solver_order} {solver_type} {spacing} disable={disable} poison={poison} step {i}"
                    S.assert_bit_equal(xd_new, ref, what + " fused_step prev_sample")
                    S.assert_bit_equal(out, ref, what + " step prev_sample")
                    S.assert_bit_equal(x0_dev, x0_ref, what + " pipeline x0")
                    for s in (dev_s, step_s):
                        assert s.step_index == host_s.step_index == i + 1 and s.this_order == host_s.this_order
                        assert s.lower_order_nums == host_s.lower_order_nums and s.last_sample.is_cuda
                        S.assert_bit_equal(s.last_sample, host_s.last_sample, what + " last_sample")
                        for m, r in zip(s.model_outputs, host_s.model_outputs):
                            assert (m is None) == (r is None)
                            if m is not None:
                                S.assert_bit_equal(m, r, what + " kept x0 prediction")
                    x, xd = ref, xd_new
                assert float(host_s.sigmas[-1]) == 0.0 and bool(torch.isfinite(xd).all())


# =============================================================================================================================
# pipelines at tiny width
# =============================================================================================================================
def _hip(model_cls, oracle_model):
    m = model_cls(**vars(oracle_model.config))
    m.load_state_dict(oracle_model.state_dict())
    return m.to(DEV, F32)


STEPS = 8
GUIDE = dict(guidance_scale=7.5, guidance_rescale=0.7)
CONFIGS = {"order2-bh2": dict(solver_order=2, solver_type="bh2"), "order3-bh1": dict(solver_order=3, solver_type="bh1")}


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
    """Inputs, ONE HIP dual pipeline, and oracle.pipelines.dual_loop's latents of every iteration under RefUniPCScheduler for the two
    configurations (computed once, left unchanged)."""
    from oracle import fixtures
    from oracle import pipelines as OP

    pe, ne, lat = fixtures.make_inputs(2, 16, 16, cross_dim=64)
    records = {}
    for name, kw in CONFIGS.items():
        records[name] = []
        OP.dual_loop(fixtures.build_unet("tiny", 4), fixtures.build_unet("tiny", 8), R.RefUniPCScheduler(**kw), pe, ne, lat, STEPS,
                     record=records[name], **GUIDE)
    return _dual_pipe(unipc()), pe, ne, lat, records


def _run_dual(case, scheduler, steps=STEPS, **attrs):
    pipe, pe, ne, lat, _ = case
    pipe.scheduler = scheduler
    for k, v in attrs.items():
        setattr(pipe, k, v)
    return pipe(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), latents=lat.to(DEV), height=128, width=128,
                num_inference_steps=steps, generator=gen(1), output_type="latent", **GUIDE)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_dual_pipeline_matches_dual_loop(dual_case, name):
    """Fused gmd_unipc_step under graphs + two streams (CFG 7.5, rescale 0.7), against oracle.pipelines.dual_loop driven by the float64
    scheduler of tests/unipc_ref.py: latent RMS within the gate at EVERY iteration; then eager on one stream, bit for bit the same."""
    pipe, pe, ne, lat, records = dual_case
    record, kw = records[name], CONFIGS[name]
    seen = []
    pipe._step_probe = lambda i, sdr, gm: seen.append((sdr.clone(), gm.clone()))
    try:
        s1, g1 = _run_dual(dual_case, unipc(**kw), use_hip_graphs=True, overlap_streams=True)
    finally:
        pipe._step_probe = None
    assert pipe._use_fused(lat.to(DEV), pipe.unet, pipe.scheduler) and pipe.scheduler.step_index == STEPS == pipe.gm_scheduler.step_index
    assert pipe.scheduler.last_sample is not pipe.gm_scheduler.last_sample and pipe.scheduler.model_outputs[-1] is not pipe.gm_scheduler.model_outputs[-1]
    assert all(m is not None for s in (pipe.scheduler, pipe.gm_scheduler) for m in s.model_outputs)
    assert len(seen) == STEPS == len(record)
    for i, ((sdr, gm), (rs, rg)) in enumerate(zip(seen, record)):
        print(f"{name} iteration {i}: latent RMS sdr={rms(sdr, rs):.2e} gm={rms(gm, rg):.2e}")
        assert rms(sdr, rs) <= RMS_TOL and rms(gm, rg) <= RMS_TOL, f"iteration {i}"
    assert torch.equal(seen[-1][0], s1) and torch.equal(seen[-1][1], g1)
    s2, g2 = _run_dual(dual_case, unipc(**kw), use_hip_graphs=False, overlap_streams=False)
    assert torch.equal(s1, s2) and torch.equal(g1, g2), "graphs + two streams and eager single stream must agree bit for bit"
    s3, g3 = _run_dual(dual_case, unipc(**kw), use_hip_graphs=True, overlap_streams=True)  # without the probe's synchronisation
    assert torch.equal(s1, s3) and torch.equal(g1, g3)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_gm_pipeline_matches_oracle(name):
    from gm_diffusion.components import AutoencoderKL, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionGMPipeline
    from oracle import fixtures
    from oracle import pipelines as OP

    kw = CONFIGS[name]
    ou = fixtures.build_unet("tiny", 8)
    pipe = StableDiffusionGMPipeline(
        vae=_hip(AutoencoderKL, fixtures.build_vae("tiny")), text_encoder=None, tokenizer=None, unet=_hip(UNet2DConditionModel, ou),
        scheduler=unipc(**kw), safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    pe, ne, lat = fixtures.make_inputs(1, 16, 16, cross_dim=64)
    sdr_lat = torch.randn(1, 4, 16, 16, generator=gen(77))
    record = []
    OP.gm_loop(ou, R.RefUniPCScheduler(**kw), sdr_lat, pe, ne, lat, STEPS, record=record, **GUIDE)
    seen = []

    def cb(p, i, t, kw_):
        seen.append(kw_["latents"].clone())
        return {}

    def run(**more):
        pipe.scheduler = unipc(**kw)
        return pipe(sdr_lat.to(DEV), prompt=None, prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), latents=lat.to(DEV),
                    num_inference_steps=STEPS, generator=gen(42), output_type="latent", **GUIDE, **more).images

    assert pipe._use_fused(lat.to(DEV), pipe.unet, pipe.scheduler) and pipe.use_hip_graphs
    out = run(callback_on_step_end=cb)
    assert len(seen) == STEPS == len(record)
    for i, (got, ref) in enumerate(zip(seen, record)):
        print(f"{name} iteration {i}: latent RMS {rms(got, ref):.2e}")
        assert rms(got, ref) <= RMS_TOL, f"iteration {i}"
    assert torch.equal(seen[-1], out) and pipe.scheduler.step_index == STEPS
    pipe.use_hip_graphs = False
    assert torch.equal(run(), out), "graphs and eager launches must agree bit for bit"


# =============================================================================================================================
# untouched paths
# =============================================================================================================================
def test_neighbours_never_launch_unipc_step_and_unipc_launches_it_once_per_step(dual_case, monkeypatch):
    """With gmd_unipc_step and gmd_dpm_step wrapped by counters: a PNDM run and a DPM run of the dual pipeline call gmd_unipc_step zero
    times; a UniPC run calls it once per scheduler per step (2 x steps) and gmd_dpm_step zero times."""
    from gm_diffusion._native import lib
    from gm_diffusion.components import DPMSolverMultistepScheduler, PNDMScheduler

    counts = {"gmd_unipc_step": 0, "gmd_dpm_step": 0}

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
    assert counts == {"gmd_unipc_step": 0, "gmd_dpm_step": 0}
    _run_dual(dual_case, DPMSolverMultistepScheduler(steps_offset=1, **SD), steps=steps, use_hip_graphs=True, overlap_streams=True)
    assert counts == {"gmd_unipc_step": 0, "gmd_dpm_step": 2 * steps}
    counts["gmd_dpm_step"] = 0
    _run_dual(dual_case, unipc(), steps=steps, use_hip_graphs=True, overlap_streams=True)
    assert counts == {"gmd_unipc_step": 2 * steps, "gmd_dpm_step": 0}
