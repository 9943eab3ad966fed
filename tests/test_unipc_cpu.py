"""CPU: components.UniPCMultistepScheduler -- schedule tables and the order schedule against the float64 restatement of
tests/unipc_ref.py, the host step per element against float64 (allowed violations: 0), identities that tie it to code written earlier
(the perfect predictor, first order without corrector is DPM-Solver++), what the corrector and the order are for (an analytic model whose
exact solution is known), refusals, the config and pipeline protocol, and the argument validation of gmd_unipc_step.  No GPU is touched."""
import copy

import numpy as np
import pytest
import torch

import euler_ref as E
import parity as P
import unipc_ref as R

SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SHAPE = (2, 4, 9, 7)
SPACINGS = ("linspace", "leading", "trailing")
STEPS = 8


def unipc(**kw):
    from gm_diffusion.components import UniPCMultistepScheduler

    return UniPCMultistepScheduler(**kw)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def sig(s):
    """The schedule's float32 sigmas as Python floats (exact)."""
    return [float(v) for v in s.sigmas]


def state(s):
    """(last_sample, history newest first) of the scheduler before a step."""
    return s.last_sample, [m for m in reversed(s.model_outputs) if m is not None]


# ---------------------------------------------------------------------------------------------------------------------------
# tables and orders
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("final", ["zero", "sigma_min"])
@pytest.mark.parametrize("spacing", SPACINGS)
def test_schedule_tables_against_float64(spacing, final):
    """Timesteps equal; every sigma within 4 2^-24 of the float64 value on the same float32 alphas_cumprod table: the product evaluates
    ((1 - a) / a) ** 0.5 in float32 (difference, quotient, and a library power that halves what came in and adds at most one ulp = two
    roundings: (1 + 1) / 2 + 2 = 3) and rounds the float64 interpolation to float32 once more."""
    for steps_offset in ((0, 1) if spacing == "leading" else (0,)):
        for n in (1, 2, 3, 8, 20):
            s = unipc(timestep_spacing=spacing, final_sigmas_type=final, steps_offset=steps_offset, **SD)
            s.set_timesteps(n)
            ts, sg = R.tables64(E.alphas_cumprod(**SD), n, spacing, steps_offset, final)
            assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == ts.tolist() and s.num_inference_steps == n
            got = s.sigmas.double().numpy()
            assert s.sigmas.dtype == torch.float32 and got.shape == sg.shape == (n + 1,)
            assert np.all(np.abs(got - sg) <= 4 * R.U_F32 * np.abs(sg)), (spacing, final, n)
            assert (got[-1] == 0.0) if final == "zero" else (got[-1] == float(s.sigmas.new_tensor(sg[-1])) > 0.0)
            assert s.model_outputs == [None] * 2 and s.lower_order_nums == 0 and s.last_sample is None and s.this_order is None
            assert s.step_index is None and float(s.init_noise_sigma) == 1.0
            x = torch.ones(3)
            assert s.scale_model_input(x, ts[0]) is x


ORDER_TABLE = {1: ([1] * 8, [0] + [1] * 7), 2: ([1, 2, 2, 2, 2, 2, 2, 1], [0, 1, 2, 2, 2, 2, 2, 2]),
               3: ([1, 2, 3, 3, 3, 3, 2, 1], [0, 1, 2, 3, 3, 3, 3, 2])}


def _orders_used(s, n):
    s.set_timesteps(n)
    g = gen(1)
    x = torch.randn(SHAPE, generator=g)
    pred, corr = [], []
    for t in s.timesteps.tolist():
        pl = s._plan_step(t)
        pred.append(pl.q)
        corr.append(pl.p)
        x = s.step(torch.randn(SHAPE, generator=g), t, x).prev_sample
        assert s.this_order == pl.q
    return pred, corr


@pytest.mark.parametrize("solver_order", [1, 2, 3])
def test_order_schedule(solver_order):
    """The order actually used by every step of 8, read off the plan right before the step: the table of the design with
    ``lower_order_final``; without it (on a schedule that ends at sigma_min: at sigma 0 the high-order last step is refused) the ramp
    1, 2, 3 and then ``solver_order`` to the end.  ``disable_corrector`` removes exactly the named corrections."""
    pred, corr = ORDER_TABLE[solver_order]
    assert _orders_used(unipc(solver_order=solver_order, **SD), STEPS) == (pred, corr)
    flat = [min(i + 1, solver_order) for i in range(STEPS)]
    got = _orders_used(unipc(solver_order=solver_order, lower_order_final=False, final_sigmas_type="sigma_min", **SD), STEPS)
    assert got == (flat, [0] + flat[:-1])
    got = _orders_used(unipc(solver_order=solver_order, disable_corrector=[0, 3], **SD), STEPS)
    assert got == (pred, [0 if i in (1, 4) else c for i, c in enumerate(corr)])
    for i in range(STEPS):
        assert R.orders(i, STEPS, solver_order, True) == (corr[i], pred[i])
        assert R.orders(i, STEPS, solver_order, False) == (([0] + flat[:-1])[i], flat[i])


# ---------------------------------------------------------------------------------------------------------------------------
# the host step against the float64 function
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("disable", [[], [0, 3], list(range(STEPS))])
@pytest.mark.parametrize("solver_type", ["bh1", "bh2"])
@pytest.mark.parametrize("solver_order", [1, 2, 3])
def test_host_step_within_bound_of_float64(solver_order, solver_type, disable):
    """Whole 8-step trajectories on unit-normal model outputs (three spacings): per element, |host step - float64 step on the same float32
    history| <= 12 2^-24 A + the scalars' own error for prev_sample, 9 2^-24 Ac + ... for the corrected sample kept as ``last_sample``
    and 3 2^-24 A0 + ... for the x0 prediction kept as history.  No element is excluded.  The float32 restatement the GPU tests compare the
    kernel with (``unipc_step_f32``, fed the scheduler's own scalars) is the host step bit for bit."""
    import small_ref as S

    worst = 0.0
    for spacing in SPACINGS:
        s = unipc(solver_order=solver_order, solver_type=solver_type, disable_corrector=disable, timestep_spacing=spacing, **SD)
        s.set_timesteps(STEPS)
        sg = sig(s)
        g = gen(11)
        x = torch.randn(SHAPE, generator=g)
        for i, t in enumerate(s.timesteps.tolist()):
            eps = torch.randn(SHAPE, generator=g)
            last, hist = state(s)
            p, q = R.orders(i, STEPS, solver_order, True, disable)
            sc = R.scalars(sg, i, p, q, solver_type, with_err=True)
            ref, xc_ref, x0_ref, mags = R.step64(eps, x, sc, last, hist)
            b_prev, b_xc, b_x0 = R.bounds(mags, sc)
            pl = s._plan_step(t)
            f32 = R.unipc_step_f32(eps, x, pl.p, pl.q, pl.floats() + [1.0, 0.0], last, hist)
            out = s._host_step(eps, t, x)
            what = f"order {solver_order} {solver_type} disable={disable} {spacing} step {i} (p={p}, q={q})"
            worst = max(worst, P.assert_elementwise(out, ref, b_prev, what + " prev_sample"))
            P.assert_elementwise(s.model_outputs[-1], x0_ref, b_x0, what + " x0 prediction")
            if p:
                P.assert_elementwise(s.last_sample, xc_ref, b_xc, what + " corrected sample")
            else:
                assert torch.equal(s.last_sample, x) and s.last_sample is not x
            for got, want, nm in zip((s.model_outputs[-1], s.last_sample, out), f32, ("m0", "x_corr", "x_prev")):
                S.assert_bit_equal(got, want, what + " unipc_step_f32 " + nm)
            assert out.dtype == torch.float32 and s.step_index == i + 1
            x = out
        assert sg[-1] == 0.0 and bool(torch.isfinite(x).all())
    print(f"order {solver_order} {solver_type} disable={disable}: max |err| / bound = {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------
# identities
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver_type", ["bh1", "bh2"])
@pytest.mark.parametrize("solver_order", [1, 2, 3])
def test_perfect_predictor_lands_on_the_noised_x0(solver_order, solver_type):
    """A perfect predictor, eps = (x - alpha X0) / sg for a fixed X0 (every earlier x0 prediction is X0, the previous corrected sample is
    alpha_prev X0 + sg_prev E): every step lands on alpha_next X0 + sg_next E, the last one on X0.  E is taken in float64 from the
    float32 tensor the update starts from (``last_sample`` when the corrector runs, x otherwise); the eps handed in is the float64 value
    rounded to float32, one more rounding on every path through x0 (``extra=1``).  The float64 scheduler does the same to 1e-13."""
    s = unipc(solver_order=solver_order, solver_type=solver_type, **SD)
    s.set_timesteps(STEPS)
    sg = sig(s)
    g = gen(3)
    X0, E0 = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
    al = lambda k: 1.0 / (sg[k] ** 2 + 1.0) ** 0.5
    noised = lambda k, e: al(k) * X0.double() + sg[k] * al(k) * e
    x = noised(0, E0.double()).float()
    for i, t in enumerate(s.timesteps.tolist()):
        p, q = R.orders(i, STEPS, solver_order, True)
        if i:
            s.model_outputs = [X0.clone() for _ in range(solver_order)]
        e_x = (x.double() - al(i) * X0.double()) / (sg[i] * al(i))
        e_t = (s.last_sample.double() - al(i - 1) * X0.double()) / (sg[i - 1] * al(i - 1)) if p else e_x
        eps = e_x.float()
        last, hist = state(s)
        sc = R.scalars(sg, i, p, q, solver_type, with_err=True)
        _, _, _, mags = R.step64(eps, x, sc, last, hist)
        got = s.step(eps, t, x).prev_sample
        P.assert_elementwise(got, noised(i + 1, e_t), R.bounds(mags, sc, extra=1)[0], f"order {solver_order} {solver_type} step {i}")
        x = got
    assert sg[-1] == 0.0
    P.assert_elementwise(x, X0.double(), R.bounds(mags, sc, extra=1)[0], "the last step lands on X0")
    r = R.RefUniPCScheduler(solver_order=solver_order, solver_type=solver_type)
    r.set_timesteps(STEPS)
    sg = r.sigmas  # its own table: the product's float32 entries may differ from it by an ulp
    x64 = noised(0, E0.double())
    for i, t in enumerate(r.timesteps.tolist()):
        x64 = r.step((x64 - al(i) * X0.double()) / (sg[i] * al(i)), t, x64).prev_sample
        assert float((x64 - noised(i + 1, E0.double())).abs().max()) <= 1e-13
    assert float((x64 - X0.double()).abs().max()) <= 1e-13


@pytest.mark.parametrize("spacing", SPACINGS)
def test_first_order_without_corrector_is_dpm_solver(spacing):
    """solver_order = 1, bh2, the corrector disabled everywhere: DPMSolverMultistepScheduler(solver_order=1) on the same inputs, within
    the sum of the two per-element bounds against the one float64 step (not bitwise: expm1(-h) here, exp(-h) - 1 there)."""
    import dpm_sde_ref as D
    from gm_diffusion.components import DPMSolverMultistepScheduler

    kw = dict(solver_order=1, timestep_spacing=spacing, **SD)
    a, b = unipc(disable_corrector=list(range(STEPS)), **kw), DPMSolverMultistepScheduler(**kw)
    a.set_timesteps(STEPS)
    b.set_timesteps(STEPS)
    assert torch.equal(a.timesteps, b.timesteps) and torch.equal(a.sigmas, b.sigmas)
    sg = sig(a)
    g = gen(4)
    x = torch.randn(SHAPE, generator=g)
    for i, t in enumerate(a.timesteps.tolist()):
        eps = torch.randn(SHAPE, generator=g)
        sc = R.scalars(sg, i, 0, 1, "bh2", with_err=True)
        ref, _, _, mags = R.step64(eps, x, sc)
        ref_d, _, a_d, _ = D.dpm_step64(eps, x, None, None, sg[i], sg[i + 1], None, D.ODE, "midpoint")
        assert float((ref - ref_d).abs().max()) <= 1e-13 * float(ref.abs().max())  # the two float64 restatements are one function
        oa, ob = a.step(eps, t, x).prev_sample, b.step(eps, t, x).prev_sample
        P.assert_elementwise(oa, ref, R.bounds(mags, sc)[0], f"{spacing} step {i} UniPC")
        P.assert_elementwise(ob, oa.double(), R.bounds(mags, sc)[0] + D.bound(a_d), f"{spacing} step {i} DPM-Solver++ against UniPC")
        x = oa


@pytest.mark.parametrize("solver_type", ["bh1", "bh2"])
@pytest.mark.parametrize("n", [8, 10, 20])
def test_corrector_and_order_reduce_the_error_of_an_analytic_model(n, solver_type):
    """x0 ~ N(0, 0.7^2): eps(x, sigma) = sg x / (alpha^2 0.49 + sg^2) is the exact model and the ODE solution at sigma = 0 is
    x_init 0.7 / (alpha_0^2 0.49 + sg_0^2)^.5.  RMS error over 4096 samples, strictly ordered: (order 1, no corrector) > (order 1 with
    corrector) > (order 2 with corrector); and the product's figures are the float64 scheduler's to 1e-5."""
    rms = {}
    for name, order, disable in (("p1", 1, list(range(n))), ("pc1", 1, []), ("pc2", 2, [])):
        for kind in ("product", "float64"):
            if kind == "product":
                s = unipc(solver_order=order, solver_type=solver_type, disable_corrector=disable, **SD)
                dt = torch.float32
            else:
                s = R.RefUniPCScheduler(solver_order=order, solver_type=solver_type, disable_corrector=disable)
                dt = torch.float64
            s.set_timesteps(n)
            sg = [float(v) for v in s.sigmas]
            al = [1.0 / (v * v + 1.0) ** 0.5 for v in sg]
            var0 = al[0] ** 2 * 0.49 + (sg[0] * al[0]) ** 2
            x_init = torch.randn(4096, generator=gen(0), dtype=torch.float64) * var0 ** 0.5
            x = x_init.to(dt)
            for i, t in enumerate(s.timesteps.tolist()):
                eps = (sg[i] * al[i] * x.double() / (al[i] ** 2 * 0.49 + (sg[i] * al[i]) ** 2)).to(dt)
                x = s.step(eps, t, x).prev_sample
            rms[name, kind] = float(((x.double() - x_init * 0.7 / var0 ** 0.5) ** 2).mean().sqrt())
    print(f"n={n} {solver_type}: " + " ".join(f"{k[0]}/{k[1]}={v:.4f}" for k, v in rms.items()))
    for kind in ("product", "float64"):
        assert rms["p1", kind] > rms["pc1", kind] > rms["pc2", kind], (kind, rms)
    for name in ("p1", "pc1", "pc2"):
        assert abs(rms[name, "product"] - rms[name, "float64"]) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------------
# refusals and object behaviour
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_option():
    from gm_diffusion.components import UniPCMultistepScheduler as U

    for kw, word in ((dict(use_karras_sigmas=True), "use_karras_sigmas"), (dict(use_exponential_sigmas=True), "use_exponential_sigmas"),
                     (dict(use_beta_sigmas=True), "use_beta_sigmas"), (dict(use_flow_sigmas=True), "use_flow_sigmas"),
                     (dict(predict_x0=False), "predict_x0"), (dict(solver_p=object()), "solver_p"), (dict(thresholding=True), "thresholding"),
                     (dict(rescale_betas_zero_snr=True), "rescale_betas_zero_snr"), (dict(prediction_type="v_prediction"), "prediction_type"),
                     (dict(prediction_type="sample"), "prediction_type"), (dict(solver_order=4), "solver_order"),
                     (dict(solver_order=0), "solver_order"), (dict(solver_type="bh3"), "solver_type")):
        with pytest.raises(NotImplementedError, match=word):
            U(**kw)
    with pytest.raises(TypeError, match="algorithm_type"):
        U(algorithm_type="dpmsolver++")
    with pytest.raises(ValueError, match="set_timesteps"):
        U().step(torch.zeros(1), 0, torch.zeros(1))
    with pytest.raises(ValueError, match="final_sigmas_type"):
        U(final_sigmas_type="one").set_timesteps(4)
    with pytest.raises(ValueError, match="not supported"):
        U(timestep_spacing="log").set_timesteps(4)
    # the last step at sigma 0 with an order above 1: the coefficients are not finite
    s = U(solver_order=2, lower_order_final=False, **SD)
    s.set_timesteps(3)
    x = torch.randn(SHAPE, generator=gen(0))
    ts = s.timesteps.tolist()
    for t in ts[:2]:
        x = s.step(x, t, x).prev_sample
    before = (s.step_index, s.lower_order_nums, s.this_order, s.last_sample.clone(), [m.clone() for m in s.model_outputs])
    with pytest.raises(ValueError, match=r'lower_order_final=True or final_sigmas_type="sigma_min"'):
        s.step(x, ts[2], x)
    assert (s.step_index, s.lower_order_nums, s.this_order) == before[:3] and torch.equal(s.last_sample, before[3])
    assert all(torch.equal(a, b) for a, b in zip(s.model_outputs, before[4]))  # the refused step changed nothing
    for remedy in (dict(lower_order_final=True), dict(lower_order_final=False, final_sigmas_type="sigma_min")):
        s = U(solver_order=3, **remedy, **SD)
        s.set_timesteps(4)
        x = torch.randn(SHAPE, generator=gen(0))
        for t in s.timesteps.tolist():
            x = s.step(x * 0.1, t, x).prev_sample
        assert bool(torch.isfinite(x).all())


def test_deepcopy_config_protocol_and_name_map(tmp_path):
    import json
    import os

    from gm_diffusion.components import (DDIMScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler, PNDMScheduler,
                                         UniPCMultistepScheduler)
    from gm_diffusion.pipelines import StableDiffusionGMPipeline as Pipe
    from gm_diffusion.pipelines import pipeline_utils

    d = UniPCMultistepScheduler()
    assert dict(d.config) == dict(
        num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None, solver_order=2,
        prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0, predict_x0=True,
        solver_type="bh2", lower_order_final=True, disable_corrector=[], solver_p=None, use_karras_sigmas=False,
        use_exponential_sigmas=False, use_beta_sigmas=False, use_flow_sigmas=False, flow_shift=1.0, timestep_spacing="linspace",
        steps_offset=0, final_sigmas_type="zero", rescale_betas_zero_snr=False, clip_sample=False)
    assert d.order == 1 and len(d) == 1000 and d.draws_noise(None) is False and not getattr(d, "sigma_space", False)
    # a deep copy in mid-trajectory goes on exactly as the original does
    s = unipc(solver_order=3, **SD)
    s.set_timesteps(7)
    g = gen(8)
    x = torch.randn(SHAPE, generator=g)
    ts = s.timesteps.tolist()
    for t in ts[:3]:
        x = s.step(torch.randn(SHAPE, generator=g), t, x).prev_sample
    c = copy.deepcopy(s)
    assert c.step_index == 3 and c.this_order == 3 and c.lower_order_nums == 3 and c.last_sample is not s.last_sample
    assert all(a is not b and torch.equal(a, b) for a, b in zip(c.model_outputs, s.model_outputs)) and torch.equal(c.last_sample, s.last_sample)
    xc = x.clone()
    for t in ts[3:]:
        eps = torch.randn(SHAPE, generator=g)
        x, xc = s.step(eps, t, x).prev_sample, c.step(eps, t, xc, return_dict=False)[0]
        assert torch.equal(x, xc)
    # from_config from the other schedulers' configs, foreign keys dropped; another solver's solver_type falls to bh2
    p = PNDMScheduler(skip_prk_steps=True, steps_offset=1, timestep_spacing="leading", **SD)
    u = UniPCMultistepScheduler.from_config(p.config)
    assert u.config.steps_offset == 1 and u.config.timestep_spacing == "leading" and u.config.beta_schedule == "scaled_linear"
    assert "skip_prk_steps" not in u.config and u.config.solver_type == "bh2" and u.config.solver_order == 2
    u = UniPCMultistepScheduler.from_config(DPMSolverMultistepScheduler(solver_type="heun", final_sigmas_type="sigma_min", **SD).config)
    assert u.config.solver_type == "bh2" and u.config.final_sigmas_type == "sigma_min" and "algorithm_type" not in u.config
    u = UniPCMultistepScheduler.from_config(EulerDiscreteScheduler(timestep_spacing="trailing", **SD).config, solver_order=3, solver_type="bh1")
    assert u.config.timestep_spacing == "trailing" and u.config.solver_order == 3 and u.config.solver_type == "bh1"
    assert UniPCMultistepScheduler.from_config(u.config).config == u.config
    for cls in (PNDMScheduler, DDIMScheduler, EulerDiscreteScheduler):
        assert cls.from_config(u.config).config.beta_schedule == "scaled_linear"
    import gm_diffusion.components.schedulers as M

    every = [c for c in vars(M).values() if isinstance(c, type) and issubclass(c, M._SchedulerBase) and not c.__name__.startswith("_")]
    assert len(every) >= 9 and UniPCMultistepScheduler in every
    for cls in every:  # every scheduler of the file, at its defaults and at the SD betas
        assert UniPCMultistepScheduler.from_config(cls().config).config.beta_schedule == cls().config.beta_schedule
        assert UniPCMultistepScheduler.from_config(cls(**SD).config).config.beta_end == 0.012
    # the pipelines: name map, from_pretrained, step kwargs, nothing to pre-draw, fused recognition
    assert pipeline_utils._LOADABLE["UniPCMultistepScheduler"] is UniPCMultistepScheduler
    os.makedirs(tmp_path / "scheduler")
    json.dump({"_class_name": "UniPCMultistepScheduler", "_diffusers_version": "0.33.0", "solver_order": 3, "set_alpha_to_one": False, **SD},
              open(tmp_path / "scheduler" / "scheduler_config.json", "w"))
    one = UniPCMultistepScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")
    assert one.config.solver_order == 3 and one.config.beta_start == 0.00085 and "set_alpha_to_one" not in one.config
    pipe = Pipe.__new__(Pipe)
    pipe.scheduler = s
    kw = pipe.prepare_extra_step_kwargs(g, 0.7)
    assert kw == {} and Pipe._fused_step_kwargs(kw) == {} and Pipe._pack_div(s, ts[0]) is None
    assert Pipe._predraw_step_noise([s, copy.deepcopy(s)], ts, (2, 4, 8, 8), gen(0), "cpu") is None

    class FakeLatents:
        is_cuda = True

    from gm_diffusion.components import UNet2DConditionModel

    unet = UNet2DConditionModel.__new__(UNet2DConditionModel)
    assert pipe._use_fused(FakeLatents(), unet, s) and not pipe._use_fused(FakeLatents(), object(), s)


@pytest.mark.parametrize("final", ["zero", "sigma_min"])
def test_tiny_step_counts_and_16_bit_tensors(final):
    """n = 1, 2, 3 (shorter than the order ramp) and 50, every order and solver type, float32 and bfloat16 host tensors: finite, the
    caller's dtype back, float32 history."""
    for n in (1, 2, 3, 50):
        for order in (1, 2, 3):
            for solver_type in ("bh1", "bh2"):
                for dt in (torch.float32, torch.bfloat16):
                    s = unipc(solver_order=order, solver_type=solver_type, final_sigmas_type=final, **SD)
                    s.set_timesteps(n)
                    g = gen(n)
                    x = torch.randn(SHAPE, generator=g).to(dt)
                    for t in s.timesteps:
                        x = s.step(torch.randn(SHAPE, generator=g).to(dt), t, x).prev_sample
                    assert x.dtype == dt and bool(torch.isfinite(x).all()) and s.step_index == n
                    assert s.model_outputs[-1].dtype == torch.float32 and s.last_sample.dtype == torch.float32


def test_pipeline_from_pretrained_loads_the_scheduler_the_checkpoint_names(tmp_path):
    import json
    import os

    from gm_diffusion.components import UniPCMultistepScheduler
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline, StableDiffusionGMPipeline
    from oracle import fixtures

    models = dict(vae=fixtures.build_vae("tiny"), unet=fixtures.build_unet("tiny", 8), text_encoder=None, tokenizer=None, safety_checker=None,
                  requires_safety_checker=False)
    root = tmp_path / "ckpt"
    os.makedirs(root / "scheduler")
    json.dump({"_class_name": "UniPCMultistepScheduler", "_diffusers_version": "0.33.0", "timestep_spacing": "leading", "steps_offset": 1,
               "solver_type": "bh1", "skip_prk_steps": True, **SD}, open(root / "scheduler" / "scheduler_config.json", "w"))
    json.dump({"_class_name": "StableDiffusionPipeline", "unet": ["diffusers", "UNet2DConditionModel"], "vae": ["diffusers", "AutoencoderKL"],
               "text_encoder": ["transformers", "CLIPTextModel"], "tokenizer": ["transformers", "CLIPTokenizer"],
               "scheduler": ["diffusers", "UniPCMultistepScheduler"]}, open(root / "model_index.json", "w"))
    for pipe in (StableDiffusionGMPipeline.from_pretrained(str(root), **models),
                 StableDiffusionDualUNetPipeline.from_pretrained(str(root), gm_unet=models["unet"], **models)):
        s = pipe.scheduler
        assert type(s) is UniPCMultistepScheduler and s.config.solver_type == "bh1" and s.config.steps_offset == 1
        assert "skip_prk_steps" not in s.config
        s.set_timesteps(4)
        assert s.timesteps.tolist() == [801, 601, 401, 201]


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
    want = [P_] * 6 + [I, c_int64, I, F, P_, F, I, I] + [F] * 19 + [P_] * 5
    assert native.SIGNATURES["gmd_unipc_step"] == want and lib.gmd_unipc_step.argtypes == want
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gmd_hip.h")).read()
    decl = re.search(r"int gmd_unipc_step\((.*?)\);", header, re.S).group(1)
    kinds = []
    for arg in (a.strip() for a in decl.split(",")):
        kinds.append(P_ if ("*" in arg or arg.startswith("gmd_stream_t")) else c_int64 if arg.startswith("int64_t") else I if arg.startswith("int ") else F)
        assert kinds[-1] is not F or arg.startswith("float "), arg
    assert kinds == want
    one = 1  # any non-null address: validation happens before a launch, nothing is dereferenced
    nan, inf = float("nan"), float("inf")
    names = ("sigma_s", "alpha_s", "c_x", "c_m", "c_b", "c_rho1", "c_rho2", "c_rho3", "c_r1", "c_r2", "p_x", "p_m", "p_b", "p_rho1", "p_rho2",
             "p_r1", "p_r2", "sqrt_alpha", "sqrt_one_minus_alpha")
    good = dict(zip(names, (0.9, 0.4, 0.8, -0.3, -0.3, 0.2, 0.3, 0.5, -1.5, -2.5, 0.7, -0.4, -0.4, 0.4, 0.1, -1.2, -2.2, 0.5, 0.8)))

    def step(eps=one, x=one, last=one, h1=one, h2=one, h3=one, B=1, chw=16, p=3, q=3, m0=one, xc=one, xp=one, x0=one, **c):
        f = dict(good, **c)
        return lib.gmd_unipc_step(eps, x, last, h1, h2, h3, B, chw, 0, 1.0, None, 0.0, p, q, *(f[k] for k in names), m0, xc, xp, x0, None)

    bad = [(dict(p=-1), b"corrector order -1"), (dict(p=4), b"corrector order 4"), (dict(q=0), b"predictor order 0"),
           (dict(q=4), b"predictor order 4"), (dict(B=-1), b"shape"), (dict(chw=0), b"shape"), (dict(alpha_s=0.0), b"alpha_s"),
           (dict(sqrt_alpha=0.0), b"sqrt_alpha"), (dict(c_r1=0.0), b"c_r1"), (dict(c_r2=-0.0), b"c_r2"), (dict(p_r1=0.0), b"p_r1"),
           (dict(p_r2=0.0), b"p_r2"), (dict(p=2, h2=None, q=1), b"needs h2"), (dict(p=0, q=3, h2=None), b"needs h2"),
           (dict(p=3, h3=None), b"needs h3"), (dict(p=1, q=1, h1=None), b"needs h1"), (dict(p=0, q=2, h1=None), b"needs h1"),
           (dict(p=1, last=None), b"needs last_sample")]
    bad += [(dict(**{k: v}), k.encode()) for k in names for v in (nan, inf)]
    bad += [(dict(**{k: None}), b"null") for k in ("eps", "x", "m0", "xc", "xp")]
    for kw, word in bad:
        assert step(**kw) == 1, kw  # GMD_ERR_INVALID
        assert word in lib.gmd_last_error(), (kw, lib.gmd_last_error())
    # a pointer or scalar beyond the orders in use is neither read nor checked
    assert step(B=0, eps=None, x=None, m0=None, xc=None, xp=None, last=None, h1=None, h2=None, h3=None) == 0  # an empty batch is a no-op
    assert step(B=0, p=0, q=1, c_x=nan, c_m=inf, c_b=nan, c_rho1=nan, c_rho2=nan, c_rho3=nan, c_r1=0.0, c_r2=nan, p_b=-inf, p_rho1=nan,
                p_rho2=nan, p_r1=0.0, p_r2=nan) == 0
    assert step(B=0, p=1, q=2, c_rho2=nan, c_rho3=nan, c_r1=0.0, c_r2=nan, p_rho2=nan, p_r2=0.0) == 0
    assert step(B=0, p=2, q=3, c_rho3=nan, c_r2=0.0) == 0
    assert step(B=0, x0=None, sqrt_alpha=0.0, sqrt_one_minus_alpha=nan) == 0  # the pipeline's x0 is not asked for
    assert step(B=0, p=1, c_x=nan) == 1 and step(B=0, q=2, p_b=inf) == 1  # ... and an empty batch is no excuse for a bad scalar


def test_wrapper_refuses_host_tensors_and_short_history():
    from gm_diffusion import hip_ops
    from gm_diffusion._native import HipExtensionError

    assert "unipc_step" in hip_ops.__all__
    z = torch.zeros(1, 4, 8, 8)
    with pytest.raises(HipExtensionError):
        hip_ops.unipc_step(z, z, 0, 1, [0.5] * 19, False, 1.0)
    with pytest.raises(HipExtensionError):
        hip_ops.unipc_step(z, z, 1, 2, [0.5] * 19, False, 1.0, last_sample=z, hist=(z,))
