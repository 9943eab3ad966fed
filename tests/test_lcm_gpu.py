"""GPU: the few-step (LCM) path on the device -- gmd_lcm_step bit for bit against the torch expressions on the same device tensors
(shapes, CFG, rescale, clip, noise, every NULL combination of the optional outputs, the second grid-stride lap, the write footprint,
edge values, refused coefficients), gmd_timestep_embedding_add against its torch expression in the three dtypes, whole trajectories
of LCMScheduler on the device against its own ``_host_step``, the guidance-embedded UNet against tests/lcm_ref.py (eager, captured,
re-conditioned), and both pipelines at tiny width against the loops of tests/lcm_ref.py."""
import itertools

import pytest
import torch

import lcm_ref as L
import small_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
RMS_TOL = 1e-3  # the project's gate (tests/test_euler_gpu.py:16): "within 1e-3 latent RMS"
# the gates of the existing tiny-UNet model tests: tests/test_models_gpu.py:33 (float32 2e-5, bfloat16 3e-2), tests/test_f16_gpu.py:122
# (float16 4e-3 for the tiny UNet)
UNET_TOL = {torch.float32: 2e-5, torch.bfloat16: 3e-2, torch.float16: 4e-3}
GS, GR = 7.5, 0.7
# sched_sqrt_a, sched_sqrt_1ma, c_skip, c_out, sqrt_a_prev, sqrt_b_prev, sqrt_a, sqrt_1ma
COEFS = (0.31, 0.95, 0.0123, 0.9871, 0.62, 0.78, 0.29, 0.957)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ptr(t):
    return None if t is None else t.data_ptr()


def raw(*args):
    from gm_diffusion._native import lib

    return lib().gmd_lcm_step(*args, torch.cuda.current_stream().cuda_stream)


def call(*args):
    from gm_diffusion._native import lib

    rc = raw(*args)
    assert rc == 0, (rc, lib().gmd_last_error())


def nan_dev(shape):
    return torch.full(shape, float("nan"), dtype=F32, device=DEV)


def rms(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b) ** 2).mean().sqrt())


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def sc(v):
    return torch.tensor(float(v), dtype=F32, device=DEV)  # a 0-d DEVICE scalar: torch then divides, never multiplies by a reciprocal


def guided_dev(eps_in, B, do_cfg, gs, ratio=None, gr=0.0):
    """The CFG combine and guidance rescale as torch expressions on the device tensors (the kernel's order, tests/small_ref.py)."""
    if not do_cfg:
        return eps_in.clone()
    u, t = eps_in[:B], eps_in[B:]
    eps = u + sc(gs) * (t - u)
    if ratio is not None:
        resc = eps * ratio.view(B, *([1] * (eps.dim() - 1)))
        eps = sc(gr) * resc + (sc(1.0) - sc(gr)) * eps
    return eps


def lcm(**kw):
    from gm_diffusion.components import LCMScheduler

    return LCMScheduler(**kw)


# =============================================================================================================================
# the kernel, bit for bit
# =============================================================================================================================
@pytest.mark.parametrize("do_cfg", [0, 1])
@pytest.mark.parametrize("shape", [(4, 5, 7), (4, 8, 8)])
@pytest.mark.parametrize("B", [1, 3])
def test_lcm_step_bit_equal(B, shape, do_cfg):
    """rescale in {0, 0.7} x clip in {None, 1.0} x noise given / NULL x every NULL combination of x0 and denoised, through the raw C ABI:
    what is asked for equals the torch expressions on the same device tensors, what is not asked for is not written."""
    from gm_diffusion import hip_ops as ops

    chw = shape[0] * shape[1] * shape[2]
    g = gen(100 * B + chw + do_cfg)
    eps_in = (torch.randn(((2 if do_cfg else 1) * B,) + shape, generator=g)).to(DEV)
    x, noise = ((torch.randn((B,) + shape, generator=g) * 2).to(DEV) for _ in range(2))
    ratio = ops.cfg_std_ratio(eps_in, GS) if do_cfg else None
    for gr, clip, nz, want_x0, want_den in itertools.product((0.0, GR), (None, 1.0), (noise, None), (True, False), (True, False)):
        use_ratio = ratio if (do_cfg and gr > 0.0) else None
        eps = guided_dev(eps_in, B, do_cfg, GS, use_ratio, gr)
        prev_ref, x0_ref, den_ref = L.lcm_step_f32(eps, x, COEFS, noise=nz, clip_range=clip)
        op, o0, od = (nan_dev((B,) + shape) for _ in range(3))
        d_ratio = use_ratio if do_cfg else nan_dev((B,))  # a do_cfg == 0 launch must not read the ratio
        call(ptr(eps_in), ptr(x), ptr(nz), B, chw, do_cfg, GS, ptr(d_ratio), gr, COEFS[0], COEFS[1], int(clip is not None), float(clip or 0.0),
             *COEFS[2:], ptr(op), ptr(o0) if want_x0 else None, ptr(od) if want_den else None)
        torch.cuda.synchronize()
        what = f"B={B} chw={chw} do_cfg={do_cfg} gr={gr} clip={clip} noise={nz is not None} x0={want_x0} denoised={want_den}"
        S.assert_bit_equal(op, prev_ref, what + " x_prev")
        for buf, ref, want, nm in ((o0, x0_ref, want_x0, "x0"), (od, den_ref, want_den, "denoised")):
            if want:
                S.assert_bit_equal(buf, ref, f"{what} {nm}")
            else:
                assert bool(torch.isnan(buf).all()), f"{what}: {nm} was not asked for and was written"
        if nz is None:
            S.assert_bit_equal(op, den_ref, what + ": without noise x_prev is the denoised sample")
        if clip is not None:
            assert float(((x - sc(COEFS[1]) * eps) / sc(COEFS[0])).abs().max()) > 1.0, "the inputs must reach the clip"
    # the wrapper: the same launch, outputs allocated by it
    got = ops.lcm_step(eps_in, x, COEFS, bool(do_cfg), GS, noise=noise, ratio=ratio, guidance_rescale=GR if do_cfg else 0.0, clip_range=1.0,
                       want_x0=True, want_denoised=True)
    eps = guided_dev(eps_in, B, do_cfg, GS, ratio, GR)
    for a, b, nm in zip(got, L.lcm_step_f32(eps, x, COEFS, noise=noise, clip_range=1.0), ("x_prev", "x0", "denoised")):
        S.assert_bit_equal(a, b, "hip_ops.lcm_step " + nm)
    assert ops.lcm_step(eps_in, x, COEFS, bool(do_cfg), GS)[1:] == (None, None)


# the second lap, sized as tests/test_euler_gpu.py::test_euler_step_second_lap sizes its own
LAT_B, LAT_SHAPE = 2, (4, 257, 257)
LAT_CHW = 4 * 257 * 257


@pytest.fixture(scope="module")
def lap_inputs():
    """Inputs of the two-lap launches, drawn once and left unchanged (both do_cfg cases read the first B samples of eps_in)."""
    g = gen(31)
    eps_in = torch.randn((2 * LAT_B,) + LAT_SHAPE, generator=g)
    x, noise = (torch.randn((LAT_B,) + LAT_SHAPE, generator=g) for _ in range(2))
    ratio = torch.tensor([0.25, 3.0])  # two very different entries: the lap boundary falls inside sample 1
    return tuple(t.to(DEV) for t in (eps_in, x, noise, ratio))


@pytest.mark.parametrize("do_cfg", [False, True])
def test_lcm_step_second_lap(lap_inputs, do_cfg):
    n = LAT_B * LAT_CHW
    assert n > S.LAP_LATENT and LAT_CHW < S.LAP_LATENT < n and n % 256 != 0, "not a two-lap launch with a ragged tail"
    d_eps, d_x, d_noise, d_ratio = lap_inputs
    d_eps = d_eps if do_cfg else d_eps[:LAT_B]
    eps = guided_dev(d_eps, LAT_B, do_cfg, GS, d_ratio, GR)
    ratio = d_ratio if do_cfg else nan_dev((LAT_B,))
    for nz, want in ((d_noise, True), (None, False)):
        refs = L.lcm_step_f32(eps, d_x, COEFS, noise=nz, clip_range=1.0)
        op, o0, od = (nan_dev((LAT_B,) + LAT_SHAPE) for _ in range(3))
        call(ptr(d_eps), ptr(d_x), ptr(nz), LAT_B, LAT_CHW, int(do_cfg), GS, ptr(ratio), GR, COEFS[0], COEFS[1], 1, 1.0, *COEFS[2:],
             ptr(op), ptr(o0) if want else None, ptr(od) if want else None)
        torch.cuda.synchronize()
        what = f"lcm_step two laps noise={nz is not None} do_cfg={do_cfg}"
        S.assert_bit_equal(op, refs[0], what + " x_prev")
        if want:
            S.assert_bit_equal(o0, refs[1], what + " x0")
            S.assert_bit_equal(od, refs[2], what + " denoised")
        else:
            assert bool(torch.isnan(o0).all()) and bool(torch.isnan(od).all()), what + ": an output that was not asked for was written"


GUARD = 16384  # float32 elements of sentinel before and after every output


@pytest.mark.parametrize("do_cfg", [False, True])
def test_lcm_step_stores_only_its_three_tensors(do_cfg):
    """B = 3 latents of chw = 3 * 7 * 5 = 105 elements (no multiple of 4 or 64): guard bands of a sentinel around x_prev, x0 and denoised
    stay untouched, every element inside is written, and the three inputs are left as they were."""
    B, shape, chw = 3, (3, 3, 7, 5), 105
    n = B * chw
    g = gen(12)
    eps_in = torch.randn((2 * B if do_cfg else B,) + shape[1:], generator=g)
    x, noise = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    d_eps, d_x, d_noise = eps_in.to(DEV), x.to(DEV), noise.to(DEV)
    refs = L.lcm_step_f32(guided_dev(d_eps, B, do_cfg, GS), d_x, COEFS, noise=d_noise)
    sentinel = -12345.678
    bufs = [torch.full((2 * GUARD + n,), sentinel, dtype=F32, device=DEV) for _ in range(3)]
    outs = [b[GUARD:GUARD + n] for b in bufs]
    call(ptr(d_eps), ptr(d_x), ptr(d_noise), B, chw, int(do_cfg), GS, None, 0.0, COEFS[0], COEFS[1], 0, 0.0, *COEFS[2:], *(ptr(o) for o in outs))
    torch.cuda.synchronize()
    for b, o, r, nm in zip(bufs, outs, refs, ("x_prev", "x0", "denoised")):
        assert bool((b[:GUARD] == sentinel).all()) and bool((b[GUARD + n:] == sentinel).all()), f"{nm}: a guard band changed"
        assert not bool((o == sentinel).any()), f"{nm}: an element inside was not written"
        S.assert_bit_equal(o.view(shape), r, f"lcm_step footprint {nm} do_cfg={do_cfg}")
    for d, h, nm in ((d_eps, eps_in, "eps_in"), (d_x, x, "x"), (d_noise, noise, "noise")):
        S.assert_bit_equal(d, h, f"input {nm} changed")


def test_lcm_step_edge_values():
    """+-0, denormals, +-inf and a NaN in eps (and +-0 / denormals in x and the noise), with and without the clip: signs of zeros, flushed
    or kept denormals and the NaN through the clamp are torch's."""
    from gm_diffusion import hip_ops as ops

    g = gen(8)
    tiny = 2.0 ** -140
    specials = torch.tensor([0.0, -0.0, tiny, -tiny, float("inf"), float("-inf"), float("nan"), 1.0, -1.0, 2.0 ** -126])
    k = specials.numel()
    x = torch.randn(2, 4, 5, 3, generator=g)
    eps = torch.randn(2, 4, 5, 3, generator=g)
    noise = torch.randn(2, 4, 5, 3, generator=g)
    eps.view(-1)[:k] = specials
    eps.view(-1)[k:2 * k] = specials
    x.view(-1)[k:2 * k] = torch.tensor([0.0, -0.0, -0.0, 0.0, 1.0, -1.0, 0.5, tiny, -tiny, 0.0])
    noise.view(-1)[k:2 * k] = torch.tensor([-0.0, 0.0, tiny, -tiny, 0.0, -0.0, 1.0, -0.0, 0.0, -tiny])
    d_eps, d_x, d_noise = eps.to(DEV), x.to(DEV), noise.to(DEV)
    for coefs in (COEFS, (1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0), (2.0 ** -10, 1.0, 0.0, 1.0, 0.0, 1.0, 2.0 ** -10, 1.0)):
        for clip in (None, 1.0):
            for nz in (d_noise, None):
                ref = L.lcm_step_f32(d_eps, d_x, coefs, noise=nz, clip_range=clip)
                got = ops.lcm_step(d_eps, d_x, coefs, False, 1.0, noise=nz, clip_range=clip, want_x0=True, want_denoised=True)
                for a, b, nm in zip(got, ref, ("x_prev", "x0", "denoised")):
                    S.assert_bit_equal(a, b, f"coefs={coefs} clip={clip} noise={nz is not None} {nm}")
                assert bool(torch.isnan(got[0].view(-1)[6])), "a NaN eps must come back as NaN, clipped or not"
    with pytest.raises(ops.HipExtensionError):
        ops.lcm_step(d_eps, d_x, COEFS, False, 1.0, noise=d_noise[:1])  # noise of another shape


def test_lcm_step_refuses_nan_coefficients():
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    x = torch.zeros(1, 4, 8, 8, device=DEV)
    out = nan_dev((1, 4, 8, 8))
    for i in range(6):
        c = list(COEFS)
        c[i] = float("nan")
        with pytest.raises(ops.HipExtensionError, match="finite"):
            ops.lcm_step(x, x, c, False, 1.0)
        assert raw(ptr(x), ptr(x), None, 1, 256, 0, 1.0, None, 0.0, c[0], c[1], 0, 0.0, *c[2:], ptr(out), None, None) == 1  # GMD_ERR_INVALID
        assert b"finite" in lib().gmd_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call must not launch"
    c = list(COEFS)
    c[6] = float("nan")
    ops.lcm_step(x, x, c, False, 1.0)  # the pipeline-x0 coefficients are not read without an x0 output
    with pytest.raises(ops.HipExtensionError, match="finite"):
        ops.lcm_step(x, x, c, False, 1.0, want_x0=True)


# =============================================================================================================================
# the time embedding with an addend
# =============================================================================================================================
@pytest.mark.parametrize("dim", [64, 320])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_timestep_embedding_add_bit_equal(dtype, B, dim):
    """out = round(float(round(sinusoid)) + float(addend)) -- diffusers' t_emb.to(dtype) + cond_proj(cond) -- against that torch
    expression on the plain kernel's own sinusoid; with a zero addend it IS the plain kernel's result."""
    from gm_diffusion import hip_ops as ops

    g = gen(B * dim)
    addend = (torch.randn(B, dim, generator=g) * 0.7).to(dtype).to(DEV)
    for t, flip, shift in ((999.0, True, 0.0), (41.0, False, 1.0), (0.0, True, 0.0)):
        td = torch.tensor([t], dtype=F32, device=DEV)
        plain = ops.timestep_embedding(td, B, dim, dtype, flip, shift)
        got = ops.timestep_embedding_add(td, addend, B, dim, dtype, flip, shift)
        assert got.dtype == dtype and got.shape == (B, dim)
        S.assert_bit_equal(got, (plain.float() + addend.float()).to(dtype), f"{dtype} B={B} dim={dim} t={t}")
        S.assert_bit_equal(got, plain + addend, f"{dtype} B={B} dim={dim} t={t}: the dtype's own add")
        S.assert_bit_equal(ops.timestep_embedding_add(td, torch.zeros_like(addend), B, dim, dtype, flip, shift), plain, f"{dtype} zero addend t={t}")
        if B > 1:
            assert int(S.bit_mismatch(got[0], got[1]).sum()) > 0, "every row must read its own addend"
    with pytest.raises(ops.HipExtensionError):
        ops.timestep_embedding_add(td, addend[:, :-2].contiguous(), B, dim, dtype)
    with pytest.raises(ops.HipExtensionError):
        ops.timestep_embedding_add(td, addend.to(torch.float64), B, dim, dtype)


# =============================================================================================================================
# whole trajectories, scheduler object
# =============================================================================================================================
@pytest.mark.parametrize("do_cfg", [False, True])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("n", [4, 8])
def test_scheduler_device_steps_bit_exact_vs_host_step(n, clip, do_cfg):
    """gmd_lcm_step against the torch expressions of ``_host_step`` over a whole trajectory (CFG + guidance rescale + x0 + the noise from
    a CPU generator): bit-identical x_prev, x0 and denoised, through fused_step and through the public step."""
    from gm_diffusion.pipelines import rescale_noise_cfg

    make = lambda: lcm(clip_sample=clip, clip_sample_range=2.0)
    dev_s, host_s, step_s = make(), make(), make()
    for s in (dev_s, host_s, step_s):
        s.set_timesteps(n)
    g = gen(5 + n)
    x = torch.randn(3, 4, 8, 8, generator=g)
    xd = x.to(DEV)
    gs, gr = 6.5, 0.3
    for i, t in enumerate(dev_s.timesteps.tolist()):
        eps2 = torch.randn(6, 4, 8, 8, generator=g)
        if do_cfg:
            u, c = eps2.chunk(2)
            e = rescale_noise_cfg(u + gs * (c - u), c, guidance_rescale=gr)
            eps_dev = eps2.to(DEV)
        else:
            e = eps2[:3].clone()
            eps_dev = e.to(DEV)
        ref = host_s._host_step(e, t, x, generator=gen(100 + i))
        a = host_s.alphas_cumprod[t]
        x0_ref = (x - (1 - a).sqrt() * e) / a.sqrt()  # the pipeline's x0 (dual.py:1075), never clipped
        xd_new, x0_dev = dev_s.fused_step(eps_dev, t, xd, do_cfg, gs, gr if do_cfg else 0.0, want_x0=True, generator=gen(100 + i))
        S.assert_bit_equal(xd_new, ref.prev_sample, f"x_prev step {i}")
        S.assert_bit_equal(x0_dev, x0_ref, f"x0 step {i}")
        out = step_s.step(e.to(DEV), t, xd, generator=gen(100 + i))  # the public step on device tensors: the same kernel without CFG
        S.assert_bit_equal(out.prev_sample, ref.prev_sample, f"step prev_sample step {i}")
        S.assert_bit_equal(out.denoised, ref.denoised, f"step denoised step {i}")
        assert dev_s.step_index == host_s.step_index == step_s.step_index == i + 1
        if i == n - 1:
            S.assert_bit_equal(out.prev_sample, out.denoised, "the last step returns the denoised sample")
        x, xd = ref.prev_sample, xd_new
    # device tensors that are not float32 take the torch expressions
    h = lcm()
    h.set_timesteps(2)
    o = h.step(eps_dev[:3].double(), 999, xd.double(), generator=gen(1))
    assert o.prev_sample.dtype == torch.float64 and o.prev_sample.is_cuda


# =============================================================================================================================
# the guidance-embedded UNet
# =============================================================================================================================
def _hip(model_cls, oracle_model, dtype=F32):
    m = model_cls(**vars(oracle_model.config))
    m.load_state_dict(oracle_model.state_dict())
    return m.to(DEV, dtype)


@pytest.fixture(scope="module")
def unet_case():
    """The tiny LCM oracle UNet, inputs at 8 x 8 and 5 x 7, two conditionings with different rows, and the yardstick's outputs (computed
    once, left unchanged)."""
    ou = L.build_lcm_unet(4)
    g = gen(3)
    ctx = torch.randn(2, 77, 64, generator=g)
    conds = [L.guidance_embedding(torch.tensor(w), L.COND_DIM) for w in ([6.5, 2.0], [0.5, 11.0])]
    xs = {hw: torch.randn(2, 4, *hw, generator=g) for hw in ((8, 8), (5, 7))}
    refs = {(hw, k): ou(xs[hw], torch.tensor(759), encoder_hidden_states=ctx, timestep_cond=c)[0] for hw in xs for k, c in enumerate(conds + [None])}
    return ou, ctx, conds, xs, refs


@pytest.mark.parametrize("hw", [(8, 8), (5, 7)])
@pytest.mark.parametrize("dtype,mode", [(torch.float32, "split"), (torch.float32, "exact"), (torch.bfloat16, "split"), (torch.float16, "split")])
def test_lcm_unet_forward_graph_and_recondition(unet_case, dtype, mode, hw):
    from gm_diffusion import hip_ops as ops
    from gm_diffusion.components import UNet2DConditionModel

    ou, ctx, conds, xs, refs = unet_case
    tol = UNET_TOL[dtype]
    prev = ops.set_f32_mode(mode)
    try:
        hu = _hip(UNet2DConditionModel, ou, dtype)
        x, dctx = xs[hw].to(DEV), ctx.to(DEV)
        dconds = [c.to(DEV) for c in conds]
        got = hu(x, 759, encoder_hidden_states=dctx, timestep_cond=dconds[0], return_dict=False)[0]
        e0 = rel_err(got, refs[(hw, 0)])
        print(f"{dtype} {mode} {hw}: rel err {e0:.2e} (gate {tol:.0e})")
        assert got.shape == refs[(hw, 0)].shape and e0 < tol, e0
        assert rel_err(refs[(hw, 0)], refs[(hw, 2)]) > 1e-2, "the conditioning must matter to the yardstick"
        # never conditioned / None: zeros in the buffer, diffusers' timestep_cond=None
        none = hu(x, 759, encoder_hidden_states=dctx, return_dict=False)[0]
        assert rel_err(none, refs[(hw, 2)]) < tol
        # captured graph: replay == eager bit for bit, and a changed set_timestep_cond is picked up by the same capture
        c = hu.prepare_context(dctx)
        hu.set_timestep(759)
        hu.set_timestep_cond(dconds[0], 2)
        gph = hu.graphed_forward(2, hw[0], hw[1], c)
        hu.pack_input(x, out=gph.x)
        assert torch.equal(gph.replay(), got)
        buf = hu.set_timestep_cond(dconds[1], 2)
        assert buf.dtype == dtype and buf.shape == (2, 64) and hu.set_timestep_cond(dconds[1], 2) is buf
        got2 = gph.replay().clone()
        eager2 = hu(x, 759, encoder_hidden_states=dctx, timestep_cond=dconds[1], return_dict=False)[0]
        assert torch.equal(got2, eager2), "graph replay with a changed conditioning against an eager forward"
        assert rel_err(got2, refs[(hw, 1)]) < tol and rel_err(got2, refs[(hw, 0)]) > 1e-2
        hu.set_timestep_cond(None, 2)
        assert torch.equal(gph.replay(), none)
        with pytest.raises(ValueError, match="time_cond_proj_dim"):
            hu.set_timestep_cond(dconds[0][:, :16].contiguous(), 2)
    finally:
        ops.set_f32_mode(prev)


def test_plain_unet_refuses_a_timestep_cond_and_launches_what_it_launched(monkeypatch):
    from gm_diffusion import hip_ops as ops
    from gm_diffusion.components import UNet2DConditionModel
    from oracle import fixtures

    hu = _hip(UNet2DConditionModel, fixtures.build_unet("tiny", 4))
    x, ctx = torch.randn(1, 4, 8, 8, generator=gen(1)).to(DEV), torch.randn(1, 77, 64, generator=gen(2)).to(DEV)
    with pytest.raises(ValueError, match="time_cond_proj_dim"):
        hu(x, 500, encoder_hidden_states=ctx, timestep_cond=torch.zeros(1, 32, device=DEV))
    calls = []
    real_plain, real_add = ops.timestep_embedding, ops.timestep_embedding_add
    monkeypatch.setattr(ops, "timestep_embedding", lambda *a, **k: (calls.append("plain"), real_plain(*a, **k))[1])
    monkeypatch.setattr(ops, "timestep_embedding_add", lambda *a, **k: (calls.append("add"), real_add(*a, **k))[1])
    hu(x, 500, encoder_hidden_states=ctx)
    assert calls == ["plain"]
    calls.clear()
    lu = _hip(UNet2DConditionModel, L.build_lcm_unet(4))
    lu(x, 500, encoder_hidden_states=ctx)
    assert calls == ["add"], "a guidance-embedded forward has the launch count of a plain one"


# =============================================================================================================================
# pipelines at tiny width
# =============================================================================================================================
STEPS = 4


def _dual_pipe(ou, og):
    from gm_diffusion.components import AutoencoderKL, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline
    from oracle import fixtures

    pipe = StableDiffusionDualUNetPipeline(
        vae=_hip(AutoencoderKL, fixtures.build_vae("tiny")), text_encoder=None, tokenizer=None, unet=_hip(UNet2DConditionModel, ou),
        gm_unet=_hip(UNet2DConditionModel, og), scheduler=lcm(steps_offset=1), safety_checker=None, feature_extractor=None,
        requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    return pipe


@pytest.mark.parametrize("gm_has_cond", [True, False])
def test_dual_pipeline_matches_lcm_ref(gm_has_cond, monkeypatch):
    """Fused gmd_lcm_step under graphs + two streams and eager on one stream, against lcm_ref.dual_loop with the same CPU generator
    (shared by both schedulers: SDR noise before GM noise); with a GM UNet that has a cond_proj of its own width (16) and with a plain
    GM UNet, which is then handed no conditioning."""
    from gm_diffusion import hip_ops as ops
    from oracle import fixtures

    mk_gm = (lambda: L.build_lcm_unet(8, cond_dim=16)) if gm_has_cond else (lambda: fixtures.build_unet("tiny", 8))
    ou, og = L.build_lcm_unet(4), mk_gm()
    pe, ne, lat = fixtures.make_inputs(2, 8, 8, cross_dim=64)
    rs, rg = L.dual_loop(ou, og, L.RefLCMScheduler(), pe, ne, lat, STEPS, guidance_scale=7.5, generator=gen(123))
    pipe = _dual_pipe(ou, og)

    def run(g, **attrs):
        pipe.scheduler = lcm(steps_offset=1)
        for k, v in attrs.items():
            setattr(pipe, k, v)
        return pipe(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), latents=lat.to(DEV), height=64, width=64,
                    num_inference_steps=STEPS, guidance_scale=7.5, generator=g, output_type="latent")

    g = gen(123)
    s1, g1 = run(g, use_hip_graphs=True, overlap_streams=True)
    assert pipe._use_fused(lat.to(DEV), pipe.unet, pipe.scheduler) and not pipe.do_classifier_free_guidance
    assert pipe.scheduler.step_index == STEPS == pipe.gm_scheduler.step_index
    twin = gen(123)
    for _ in range(2 * (STEPS - 1)):  # two draws per iteration but the last (the latents were passed in)
        torch.randn(lat.shape, generator=twin)
    assert torch.equal(g.get_state(), twin.get_state())
    steps = []
    real = ops.lcm_step
    monkeypatch.setattr(ops, "lcm_step", lambda *a, **k: (steps.append(1), real(*a, **k))[1])
    s2, g2 = run(gen(123), use_hip_graphs=False, overlap_streams=False)
    assert len(steps) == 2 * STEPS, "one launch per scheduler step"
    print(f"gm_has_cond={gm_has_cond}: latent RMS sdr={rms(s1, rs):.2e} gm={rms(g1, rg):.2e} (eager: {rms(s2, rs):.2e} {rms(g2, rg):.2e})")
    assert rms(s1, rs) <= RMS_TOL and rms(g1, rg) <= RMS_TOL
    assert rms(s2, rs) <= RMS_TOL and rms(g2, rg) <= RMS_TOL
    assert torch.equal(s1, s2) and torch.equal(g1, g2), "graphs + two streams and eager single stream must agree bit for bit"
    assert rms(s1, rg) > 0.1, "the two latents must NOT have received the same noise"
    # another guidance scale through the same captures: the conditioning buffer is rewritten, not the graph
    n_graphs = len(pipe.unet._graphs)
    pipe.scheduler = lcm(steps_offset=1)
    s3, _ = pipe(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), latents=lat.to(DEV), height=64, width=64, num_inference_steps=STEPS,
                 guidance_scale=3.0, generator=gen(123), output_type="latent")
    r3, _ = L.dual_loop(ou, og, L.RefLCMScheduler(), pe, ne, lat, STEPS, guidance_scale=3.0, generator=gen(123))
    assert len(pipe.unet._graphs) == n_graphs and rms(s3, r3) <= RMS_TOL and rms(s3, rs) > 10 * RMS_TOL


def test_gm_pipeline_matches_lcm_ref():
    from gm_diffusion.components import AutoencoderKL, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionGMPipeline
    from oracle import fixtures

    ou = L.build_lcm_unet(8)
    pipe = StableDiffusionGMPipeline(
        vae=_hip(AutoencoderKL, fixtures.build_vae("tiny")), text_encoder=None, tokenizer=None, unet=_hip(UNet2DConditionModel, ou),
        scheduler=lcm(steps_offset=1), safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    pe, ne, lat = fixtures.make_inputs(2, 8, 8, cross_dim=64)
    sdr_lat = torch.randn(2, 4, 8, 8, generator=gen(77))
    ref = L.gm_loop(ou, L.RefLCMScheduler(), sdr_lat, pe, ne, lat, STEPS, guidance_scale=7.5, generator=gen(42))

    def run(g):
        pipe.scheduler = type(pipe.scheduler).from_config(lcm(steps_offset=1).config)  # the documented swap
        return pipe(sdr_lat.to(DEV), prompt=None, prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), latents=lat.to(DEV),
                    num_inference_steps=STEPS, guidance_scale=7.5, generator=g, output_type="latent").images

    assert pipe._use_fused(lat.to(DEV), pipe.unet, pipe.scheduler)
    g = gen(42)
    out = run(g)
    twin = gen(42)
    for _ in range(STEPS - 1):
        torch.randn(lat.shape, generator=twin)
    assert torch.equal(g.get_state(), twin.get_state())
    print(f"gm: latent RMS {rms(out, ref):.2e}")
    assert rms(out, ref) <= RMS_TOL
    pipe.use_hip_graphs = False
    assert torch.equal(run(gen(42)), out), "graphs and eager launches must agree bit for bit"
    # the pre-draw against the draw inside fused_step: the same final latents bit for bit, the generator advanced alike
    old = StableDiffusionGMPipeline.PREDRAW_NOISE_BYTES
    try:
        StableDiffusionGMPipeline.PREDRAW_NOISE_BYTES = 0
        g = gen(42)
        assert torch.equal(run(g), out) and torch.equal(g.get_state(), twin.get_state())
    finally:
        StableDiffusionGMPipeline.PREDRAW_NOISE_BYTES = old
    pipe._use_fused = lambda *args: False  # the generic scheduler-protocol path: the HIP UNet takes timestep_cond= per call
    assert rms(run(gen(42)), ref) <= RMS_TOL


def test_pndm_with_a_plain_unet_keeps_its_launches(monkeypatch):
    """With PNDM and UNets without time_cond_proj_dim the dual pipeline never reaches the new entry points."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion.components import PNDMScheduler
    from oracle import fixtures

    pipe = _dual_pipe(fixtures.build_unet("tiny", 4), fixtures.build_unet("tiny", 8))
    pipe.scheduler = PNDMScheduler(skip_prk_steps=True, steps_offset=1, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    pipe.use_hip_graphs = False
    calls = []
    for name in ("lcm_step", "timestep_embedding_add", "timestep_embedding", "latent_step"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, (lambda real, name: lambda *a, **k: (calls.append(name), real(*a, **k))[1])(real, name))
    pe, ne, lat = fixtures.make_inputs(1, 8, 8, cross_dim=64)
    pipe(prompt_embeds=pe.to(DEV), negative_prompt_embeds=ne.to(DEV), latents=lat.to(DEV), height=64, width=64, num_inference_steps=4,
         guidance_scale=7.5, output_type="latent")
    n = len(pipe.scheduler.timesteps)
    assert calls.count("lcm_step") == 0 and calls.count("timestep_embedding_add") == 0
    assert calls.count("timestep_embedding") == 2 * n and calls.count("latent_step") == 2 * n
    assert pipe.do_classifier_free_guidance
