"""GPU: gmd_inpaint_blend bit for bit against the torch expressions of tests/img2img_ref.py evaluated on the CPU (every pointer
combination, both mask layouts, the second grid-stride lap, the write footprint, the refusals), and img2img / inpainting of the
dual-UNet pipeline on the fused device path -- graphs + two streams and eager on one stream -- and on the generic loop, against the
reference loop of tests/img2img_ref.py, with the exact identities and the accounting of UNet evaluations and generator draws."""
import pytest
import torch

import ddim_ref as D
import img2img_ref as R
import small_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
RMS_TOL = 1e-3  # north star: "within 1e-3 latent RMS"
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
STEPS = 8
GUARD = 4096  # float32 elements of NaN canary before and after either output


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ptr(t):
    return None if t is None else t.data_ptr()


def rms(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b) ** 2).mean().sqrt())


def raw(*args):
    from gm_diffusion._native import lib

    return lib().gmd_inpaint_blend(*args, torch.cuda.current_stream().cuda_stream)


# =============================================================================================================================
# the kernel
# =============================================================================================================================
SHAPES = {"small": (2, 4, 15, 17), "second_lap": (3, 4, 210, 209)}
CA, CB = 0.8125, 0.58203125


@pytest.fixture(scope="module")
def blend_inputs():
    """Per shape: z0, noise, x_prev, x0 and two masks with fractional values ([1, 1, h, w] and per-sample [B, 1, h, w], the samples'
    masks all different), drawn once and left unchanged, on the host and on the device."""
    out = {}
    for name, (B, C, h, w) in SHAPES.items():
        g = gen(17)
        z0, noise, x_prev, x0 = (torch.randn(B, C, h, w, generator=g) for _ in range(4))
        masks = {1: torch.rand(1, 1, h, w, generator=g), B: torch.rand(B, 1, h, w, generator=g)}
        for m in masks.values():  # fractional values with exact 0 and 1 among them
            m.view(-1)[::7] = 0.0
            m.view(-1)[3::11] = 1.0
        host = dict(z0=z0, noise=noise, x_prev=x_prev, x0=x0, masks=masks)
        dev = dict(z0=z0.to(DEV), noise=noise.to(DEV), masks={k: v.to(DEV) for k, v in masks.items()})
        out[name] = (host, dev)
    return out


def _guarded(t):
    """A device copy of ``t`` (or of NaN when t is None ... see callers) between two NaN canaries: (buffer, the view inside)."""
    n = t.numel()
    buf = torch.full((2 * GUARD + n,), float("nan"), dtype=F32, device=DEV)
    buf[GUARD:GUARD + n] = t.reshape(-1).to(DEV)
    return buf, buf[GUARD:GUARD + n]


def _canaries_intact(buf, n):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())


@pytest.mark.parametrize("shape", list(SHAPES))
def test_inpaint_blend_bit_equal_and_footprint(blend_inputs, shape):
    """Every combination the entry point takes -- mask_rows 1 and B, null noise (the last step), null x0, null x_prev, and the null
    mask (the img2img start) -- equals the CPU's torch expressions bit for bit; NaN canaries around both outputs stay; an output
    that is not passed is not written (nothing to write to); the null-mask call overwrites a NaN-filled x_prev completely."""
    B, C, h, w = SHAPES[shape]
    n = B * C * h * w
    if shape == "second_lap":
        assert n > S.LAP_LATENT, "not a two-lap launch"
    host, dev = blend_inputs[shape]
    for rows in (1, B):
        m, dm = host["masks"][rows], dev["masks"][rows]
        for with_noise in (True, False):
            for with_prev, with_x0 in ((True, True), (True, False), (False, True)):
                nz = host["noise"] if with_noise else None
                rp, r0 = R.blend_f32(host["z0"], host["x_prev"] if with_prev else None, host["x0"] if with_x0 else None, m, nz, CA, CB)
                bp, vp = _guarded(host["x_prev"])
                b0, v0 = _guarded(host["x0"])
                rc = raw(ptr(vp) if with_prev else None, ptr(v0) if with_x0 else None, ptr(dm), ptr(dev["z0"]),
                         ptr(dev["noise"]) if with_noise else None, B, C, h * w, rows, CA, CB)
                assert rc == 0
                torch.cuda.synchronize()
                what = f"{shape} mask_rows={rows} noise={with_noise} x_prev={with_prev} x0={with_x0}"
                assert _canaries_intact(bp, n) and _canaries_intact(b0, n), what + ": a canary changed"
                S.assert_bit_equal(vp.view(B, C, h, w), rp if with_prev else host["x_prev"], what + " x_prev")
                S.assert_bit_equal(v0.view(B, C, h, w), r0 if with_x0 else host["x0"], what + " x0")
    for with_noise in (True, False):  # the img2img start: no mask, x_prev is written and never read
        rp, _ = R.blend_f32(host["z0"], None, None, None, host["noise"] if with_noise else None, CA, CB)
        bp = torch.full((2 * GUARD + n,), float("nan"), dtype=F32, device=DEV)
        vp = bp[GUARD:GUARD + n]
        assert raw(ptr(vp), None, None, ptr(dev["z0"]), ptr(dev["noise"]) if with_noise else None, B, C, h * w, 1, CA, CB) == 0
        torch.cuda.synchronize()
        assert _canaries_intact(bp, n), f"{shape} null mask noise={with_noise}: a canary changed"
        assert not bool(torch.isnan(vp).any()), f"{shape} null mask: an element of x_prev was not written"
        S.assert_bit_equal(vp.view(B, C, h, w), rp, f"{shape} null mask noise={with_noise} x_prev")


def test_inpaint_blend_has_no_shortcut_and_the_op_wraps_it():
    """m = 0 with an infinite x_prev (or x0): 0 * inf is NaN, as torch gives.  m = 1 with an infinite keep likewise.  Through
    hip_ops.inpaint_blend, which updates in place and returns its two outputs."""
    from gm_diffusion import hip_ops as ops

    inf = float("inf")
    z0 = torch.tensor([1.0, 2.0, inf, 4.0, -0.0, 6.0]).reshape(1, 1, 2, 3)
    x_prev = torch.tensor([inf, -inf, 3.0, 4.0, 5.0, -0.0]).reshape(1, 1, 2, 3)
    x0 = torch.tensor([-inf, 2.0, 3.0, inf, 5.0, 6.0]).reshape(1, 1, 2, 3)
    mask = torch.tensor([0.0, 0.0, 1.0, 0.25, 1.0, 0.0]).reshape(1, 1, 2, 3)
    noise = torch.tensor([0.5, -0.5, 0.5, -0.5, 0.0, 0.5]).reshape(1, 1, 2, 3)
    rp, r0 = R.blend_f32(z0, x_prev, x0, mask, noise, CA, CB)
    assert bool(torch.isnan(rp.view(-1)[:3]).all()) and bool(torch.isnan(r0.view(-1)[0])), "the test's inputs must reach 0 * inf"
    dp, d0 = x_prev.to(DEV), x0.to(DEV)
    out = ops.inpaint_blend(z0.to(DEV), x_prev=dp, x0=d0, mask=mask.to(DEV), noise=noise.to(DEV), coefs=(CA, CB))
    assert out[0] is dp and out[1] is d0
    S.assert_bit_equal(dp, rp, "edge x_prev")
    S.assert_bit_equal(d0, r0, "edge x0")
    z = z0.to(DEV)
    for bad in (dict(x_prev=dp.view(1, 1, 3, 2)), dict(x_prev=dp, mask=mask.to(DEV).view(1, 2, 3)), dict(x_prev=dp, noise=noise.to(DEV).double()),
                dict(x_prev=dp, mask=torch.ones(2, 1, 2, 3, device=DEV)), dict(x0=d0), dict()):
        with pytest.raises(ops.HipExtensionError):
            ops.inpaint_blend(z, **bad)


def test_inpaint_blend_refusals_launch_nothing():
    """Each refusal returns GMD_ERR_INVALID and leaves both NaN-filled outputs as they were."""
    B, C, h, w = 2, 4, 5, 3
    n = B * C * h * w
    z0, noise = torch.randn(B, C, h, w, device=DEV), torch.randn(B, C, h, w, device=DEV)
    mask = torch.rand(B, 1, h, w, device=DEV)
    xp, x0 = (torch.full((n,), float("nan"), dtype=F32, device=DEV) for _ in range(2))
    for args in ((ptr(xp), ptr(x0), ptr(mask), None, ptr(noise), B, C, h * w, B),        # null z0
                 (None, None, ptr(mask), ptr(z0), ptr(noise), B, C, h * w, B),           # both outputs null
                 (ptr(xp), ptr(x0), None, ptr(z0), ptr(noise), B, C, h * w, 1),          # x0 without a mask
                 (ptr(xp), ptr(x0), ptr(mask), ptr(z0), ptr(noise), B, C, h * w, 3),     # mask_rows not in {1, B}
                 (ptr(xp), ptr(x0), ptr(mask), ptr(z0), ptr(noise), B, C, h * w, 0)):
        assert raw(*args, CA, CB) == 1
    assert raw(None, None, None, None, None, B, 0, h * w, 1, CA, CB) == 0  # nothing to do
    torch.cuda.synchronize()
    assert bool(torch.isnan(xp).all()) and bool(torch.isnan(x0).all())


# =============================================================================================================================
# the pipeline at tiny width
# =============================================================================================================================
def _hip(model_cls, oracle_model):
    m = model_cls(**vars(oracle_model.config))
    m.load_state_dict(oracle_model.state_dict())
    return m.to(DEV, F32)


def _hip_scheduler(kind):
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


KINDS = ["pndm", "ddim", "euler", "dpm"]
ETA = {"pndm": 0.0, "ddim": 0.7, "euler": 0.0, "dpm": 0.0}
REF_CASES = [(0.5, False), (0.5, True), (1.0, True)]  # (strength, with a mask)


@pytest.fixture(scope="module")
def case():
    """Inputs (drawn once, left unchanged), the HIP dual pipeline over the oracle's tiny weights, and the reference loop's latents for
    every (scheduler, strength, mask) case, each computed once on the CPU."""
    from gm_diffusion.components import AutoencoderKL, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline
    from oracle import fixtures

    pe, ne, noise = fixtures.make_inputs(2, 16, 16, cross_dim=64)
    z0 = 0.8 * torch.randn(2, 4, 16, 16, generator=gen(55))
    mask = R.masks(2, 16, 16)
    u4, u8 = fixtures.build_unet("tiny", 4), fixtures.build_unet("tiny", 8)
    refs = {}
    for kind in KINDS:
        for strength, masked in REF_CASES:
            refs[kind, strength, masked] = R.dual_img2img_loop(u4, u8, _ref_scheduler(kind), pe, ne, z0, noise, STEPS, strength,
                                                               mask=mask if masked else None, generator=gen(123))
    pipe = StableDiffusionDualUNetPipeline(
        vae=_hip(AutoencoderKL, fixtures.build_vae("tiny", with_encoder=True)), text_encoder=None, tokenizer=None,
        unet=_hip(UNet2DConditionModel, u4), gm_unet=_hip(UNet2DConditionModel, u8), scheduler=_hip_scheduler("pndm"),
        safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    dev = lambda t: t.to(DEV)
    return dict(pipe=pipe, pe=dev(pe), ne=dev(ne), noise=dev(noise), z0=dev(z0), mask=dev(mask), refs=refs)


def _run(case, kind, generator=None, graphs=True, **kw):
    pipe = case["pipe"]
    pipe.scheduler = _hip_scheduler(kind)
    pipe.use_hip_graphs, pipe.overlap_streams = graphs, graphs
    kw.setdefault("latents", case["noise"])
    return pipe(prompt_embeds=case["pe"], negative_prompt_embeds=case["ne"], height=128, width=128, num_inference_steps=STEPS,
                guidance_scale=7.5, eta=ETA[kind], generator=generator, output_type="latent", **kw)


@pytest.mark.parametrize("strength,masked", REF_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_fused_and_generic_loops_match_reference_loop(case, kind, strength, masked):
    """The fused loop under graphs + two streams and eager on one stream: both latents within RMS_TOL of the reference loop, and the
    two bit-identical to each other.  The generic loop on the same HIP models: within RMS_TOL (a sigma-space scheduler is refused
    there, as without a picture).  On the parent commit the keywords are ignored and the strength 0.5 cases miss by O(1)."""
    rs, rg = case["refs"][kind, strength, masked]
    pipe = case["pipe"]
    kw = dict(image=case["z0"], strength=strength, **({"mask_image": case["mask"]} if masked else {}))
    s1, g1 = _run(case, kind, gen(123), graphs=True, **kw)
    assert pipe._use_fused(case["noise"], pipe.unet, pipe.scheduler)
    s2, g2 = _run(case, kind, gen(123), graphs=False, **kw)
    print(f"{kind} strength={strength} masked={masked}: latent RMS sdr={rms(s1, rs):.2e} gm={rms(g1, rg):.2e}")
    assert rms(s1, rs) <= RMS_TOL and rms(g1, rg) <= RMS_TOL
    assert rms(s2, rs) <= RMS_TOL and rms(g2, rg) <= RMS_TOL
    assert torch.equal(s1, s2) and torch.equal(g1, g2), "graphs + two streams and eager single stream must agree bit for bit"
    pipe._use_fused = lambda *args: False
    try:
        if kind == "euler":
            with pytest.raises(ValueError, match="sigma-space"):
                _run(case, kind, gen(123), **kw)
        else:
            s3, g3 = _run(case, kind, gen(123), **kw)
            print(f"   generic loop: latent RMS sdr={rms(s3, rs):.2e} gm={rms(g3, rg):.2e}")
            assert rms(s3, rs) <= RMS_TOL and rms(g3, rg) <= RMS_TOL
    finally:
        del pipe._use_fused


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_identities(case, kind, graphs):
    """m == 1 at strength 1 with the picture given as latents: both latents equal the plain call's with the same generator.  m == 0:
    the final SDR latents are z0 (on the parent commit they are a sample from noise).  torch.equal equates +0 and -0."""
    ones, zeros = torch.ones(1, 1, 16, 16, device=DEV), torch.zeros(2, 1, 16, 16, device=DEV)
    for latents in (case["noise"], None):
        plain = _run(case, kind, gen(5), graphs, latents=latents)
        s, g = _run(case, kind, gen(5), graphs, latents=latents, image=case["z0"], mask_image=ones, strength=1.0)
        assert torch.equal(s, plain[0]) and torch.equal(g, plain[1])
    for strength in (1.0, 0.5):
        s, _ = _run(case, kind, gen(5), graphs, image=case["z0"], mask_image=zeros, strength=strength)
        assert torch.equal(s, case["z0"])


@pytest.mark.parametrize("kind", KINDS)
def test_unet_evaluations(case, kind):
    """Counted through the forwards of the eager fused loop: SDR = len(timesteps) - t_start * order, GM = len(timesteps); N - t_start
    and N, except that PNDM's schedule holds N + 1 timesteps, of which diffusers' slicing drops t_start as well."""
    pipe = case["pipe"]
    counts = {"sdr": 0, "gm": 0}

    def counted(model, key):
        inner = model.forward_packed

        def wrapper(*a, **k):
            counts[key] += 1
            return inner(*a, **k)
        return wrapper

    pipe.unet.forward_packed, pipe.gm_unet.forward_packed = counted(pipe.unet, "sdr"), counted(pipe.gm_unet, "gm")
    try:
        for strength in (0.3, 0.5, 1.0):
            counts.update(sdr=0, gm=0)
            _run(case, kind, gen(1), graphs=False, image=case["z0"], strength=strength)
            n = STEPS + (1 if kind == "pndm" else 0)
            assert counts == {"sdr": n - R.get_t_start(STEPS, strength), "gm": n}, (kind, strength, counts)
    finally:
        del pipe.unet.forward_packed, pipe.gm_unet.forward_packed


@pytest.mark.parametrize("pixels", [False, True])
def test_generator_is_advanced_by_the_documented_draws(case, pixels):
    """DDIM at eta = 0.7 on the fused path (the steps' noise is pre-drawn in the loop's order): the encoder's sample (pixels only), the
    noise, then per iteration GM alone until the SDR branch enters and SDR + GM afterwards.  The order shows in the values: a run with
    the noise handed over and a generator advanced past the first draws gives the same latents; so does the per-step draw."""
    from gm_diffusion.pipelines import StableDiffusionGMPipeline as Base

    image = torch.rand(2, 3, 128, 128, generator=gen(8)).to(DEV) if pixels else case["z0"]
    g, twin = gen(31), gen(31)
    s, gm = _run(case, "ddim", g, latents=None, image=image, strength=0.5)
    t_start = R.get_t_start(STEPS, 0.5)
    shape = case["noise"].shape
    first = [torch.randn(shape, generator=twin) for _ in range(2 if pixels else 1)]
    mid = twin.get_state()
    for _ in range(t_start + 2 * (STEPS - t_start)):
        torch.randn(shape, generator=twin)
    assert torch.equal(g.get_state(), twin.get_state())
    if not pixels:
        g2 = gen(0)
        g2.set_state(mid)
        s2, gm2 = _run(case, "ddim", g2, latents=first[0].to(DEV), image=image, strength=0.5)
        assert torch.equal(s2, s) and torch.equal(gm2, gm)
    old = Base.PREDRAW_NOISE_BYTES
    try:
        Base.PREDRAW_NOISE_BYTES = 0  # every step draws for itself, in the loop
        g3 = gen(31)
        s3, gm3 = _run(case, "ddim", g3, latents=None, image=image, strength=0.5)
    finally:
        Base.PREDRAW_NOISE_BYTES = old
    assert torch.equal(s3, s) and torch.equal(gm3, gm) and torch.equal(g3.get_state(), g.get_state())


def test_pixels_are_encoded_on_the_device_and_one_image_is_repeated(case):
    """A uint8 picture: preprocess, AutoencoderKL.encode on HIP, one sample from the generator, times scaling_factor, repeated for both
    rows: with m == 0 the SDR latents come back as exactly that."""
    pipe = case["pipe"]
    u8 = torch.randint(0, 256, (128, 128, 3), generator=gen(3), dtype=torch.uint8)
    x = pipe.image_processor.preprocess(u8, 128, 128).to(DEV)
    want = (pipe.vae.encode(x).latent_dist.sample(gen(77)).to(F32) * pipe.vae.config.scaling_factor).expand(2, -1, -1, -1)
    s, _ = _run(case, "pndm", gen(77), image=u8.numpy(), mask_image=torch.zeros(128, 128, dtype=torch.uint8), strength=0.5)
    assert torch.equal(s, want)


def test_controlnet_and_freeu_keep_working_with_a_picture(case):
    """A ControlNet inside a guidance window that opens after the SDR branch has entered and closes before the end (both the plain and
    the control graph are replayed; the window counts the SDR branch's steps, as in diffusers' img2img ControlNet pipeline) plus FreeU,
    with a picture, a mask and strength 0.5: graphs + two streams equal eager on one stream bit for bit, the generic loop agrees within
    RMS_TOL, and the ControlNet changes the result."""
    import controlnet_ref as CR
    from gm_diffusion.components import ControlNetModel
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline

    base = case["pipe"]
    torch.manual_seed(5)
    cn_ref = CR.ControlNetRef(**CR.tiny_controlnet_config()).eval().requires_grad_(False)
    cn = ControlNetModel(**CR.tiny_controlnet_config())
    cn.load_state_dict(cn_ref.state_dict())
    pipe = StableDiffusionDualUNetPipeline(vae=base.vae, text_encoder=None, tokenizer=None, unet=base.unet, gm_unet=base.gm_unet,
                                           scheduler=_hip_scheduler("dpm"), safety_checker=None, feature_extractor=None,
                                           requires_safety_checker=False, controlnet=cn.to(DEV, F32))
    pipe.set_progress_bar_config(disable=True)
    cimg = torch.rand(1, 3, 128, 128, generator=gen(8)).to(DEV)
    kw = dict(prompt_embeds=case["pe"], negative_prompt_embeds=case["ne"], latents=case["noise"], height=128, width=128,
              num_inference_steps=STEPS, guidance_scale=7.5, output_type="latent", image=case["z0"], mask_image=case["mask"], strength=0.5,
              control_image=cimg, control_guidance_start=0.25, control_guidance_end=0.75)
    pipe.enable_freeu(0.9, 0.2, 1.2, 1.4)
    try:
        pipe.use_hip_graphs, pipe.overlap_streams = True, True
        a = pipe(**kw)
        pipe.use_hip_graphs, pipe.overlap_streams = False, False
        b = pipe(**kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        off = pipe(**dict(kw, controlnet_conditioning_scale=0.0))
        assert rms(a[0], off[0]) > 1e-3, "the ControlNet must have run inside its window"
        pipe._use_fused = lambda *args: False
        c = pipe(**kw)
        print(f"controlnet + freeu + inpaint: generic against fused latent RMS sdr={rms(c[0], a[0]):.2e} gm={rms(c[1], a[1]):.2e}")
        assert rms(c[0], a[0]) <= RMS_TOL and rms(c[1], a[1]) <= RMS_TOL
    finally:
        pipe.disable_freeu()


def test_pixels_with_a_16_bit_vae_are_refused_with_the_way_out(case):
    """The encoder's 8-channel quant_conv is no 16-bit matrix-core shape: pixels need a float32 AutoencoderKL; latents pass."""
    from gm_diffusion.components import AutoencoderKL
    from oracle import fixtures

    pipe = case["pipe"]
    ov = fixtures.build_vae("tiny", with_encoder=True)
    half = AutoencoderKL(**vars(ov.config))
    half.load_state_dict(ov.state_dict())
    old, pipe.vae = pipe.vae, half.to(DEV, torch.bfloat16)
    try:
        with pytest.raises(ValueError, match="float32 AutoencoderKL"):
            _run(case, "pndm", gen(1), image=torch.rand(1, 3, 128, 128, device=DEV), strength=0.5)
        _run(case, "pndm", gen(1), image=case["z0"], strength=0.5)
    finally:
        pipe.vae = old


def test_plain_call_never_reaches_the_blend(case, monkeypatch):
    from gm_diffusion import hip_ops

    before = _run(case, "pndm")

    def boom(*a, **k):
        raise AssertionError("inpaint_blend reached without `image`")

    monkeypatch.setattr(hip_ops, "inpaint_blend", boom)
    after = _run(case, "pndm")
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    with pytest.raises(AssertionError, match="inpaint_blend reached"):
        _run(case, "pndm", image=case["z0"], strength=0.5)
