"""CPU: the ControlNet reference (tests/controlnet_ref.py), the host side of ``components.ControlNetModel`` (config, key set, parameter
count, safetensors round trip, refusals), the pipeline's window rule and guess-mode scales, and each checker of the GPU file shown
failing on the fault it exists for (the project's convention: tests/test_stats_handoff_cpu.py, tests/test_parity_cpu.py)."""
import pytest
import torch

import controlnet_ref as R
import stats_handoff as SH
from oracle import fixtures, unet as OU


def _tiny_ref(seed=5):
    torch.manual_seed(seed)
    return R.ControlNetRef(**R.tiny_controlnet_config()).eval().requires_grad_(False)


def _inputs(B=2, h=8, w=8, cross=64, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 4, h, w, generator=g), torch.randn(B, 77, cross, generator=g), torch.rand(B, 3, 8 * h, 8 * w, generator=g))


# ---------------------------------------------------------------------------------------------------------------------------
# zero-conv identity
# ---------------------------------------------------------------------------------------------------------------------------
def test_zeroed_zero_convs_give_zero_residuals_and_the_unet_unchanged():
    ref = _tiny_ref().zero_the_zero_convs()
    ou = fixtures.build_unet("tiny", 4)
    x, ctx, img = _inputs()
    down, mid = ref(x, torch.tensor(501), ctx, img)
    assert len(down) == 12 and all(not bool(d.any()) for d in down) and not bool(mid.any())
    assert [tuple(d.shape[1:]) for d in down] == [(64, 8, 8)] * 3 + [(64, 4, 4)] + [(128, 4, 4)] * 2 + [(128, 2, 2)] * 3 + [(128, 1, 1)] * 3
    plain = ou(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
    with_res = R.unet_forward_with_residuals(ou, x, torch.tensor(501), ctx, down, mid)
    assert torch.equal(with_res, plain)
    assert torch.equal(R.unet_forward_with_residuals(ou, x, torch.tensor(501), ctx), plain)  # the restatement is the oracle's forward
    # and a live ControlNet does change the result
    live = _tiny_ref()
    down, mid = live(x, torch.tensor(501), ctx, img)
    assert not torch.equal(R.unet_forward_with_residuals(ou, x, torch.tensor(501), ctx, down, mid), plain)


def test_reference_scales_and_odd_sizes():
    ref = _tiny_ref()
    x, ctx, img = _inputs(B=1, h=6, w=10)
    d1, m1 = ref(x, torch.tensor(77), ctx, img)
    assert [tuple(d.shape[2:]) for d in d1] == [(6, 10)] * 3 + [(3, 5)] * 3 + [(2, 3)] * 3 + [(1, 2)] * 3 and tuple(m1.shape[2:]) == (1, 2)
    d2, m2 = ref(x, torch.tensor(77), ctx, img, conditioning_scale=0.5, guess_mode=True)
    sc = torch.logspace(-1, 0, 13) * 0.5
    for a, b, s in zip(d1 + [m1], d2 + [m2], sc):
        assert torch.equal(b, a * float(s))


# ---------------------------------------------------------------------------------------------------------------------------
# key set, parameter count, round trip
# ---------------------------------------------------------------------------------------------------------------------------
def test_expected_keys_and_parameter_count_sd15():
    from gm_diffusion.components import ControlNetModel

    m = ControlNetModel()  # the SD-1.5 ControlNet configuration
    ref = R.ControlNetRef()
    sd = ref.state_dict()
    want = m.expected_keys()
    assert set(want) == set(sd), (sorted(set(want) ^ set(sd))[:8])
    assert all(tuple(sd[k].shape) == tuple(want[k]) for k in want)
    for prefix in ("time_embedding.", "conv_in.", "down_blocks.", "mid_block.", "controlnet_cond_embedding.conv_in.", "controlnet_cond_embedding.conv_out.",
                   "controlnet_mid_block.") + tuple(f"controlnet_cond_embedding.blocks.{i}." for i in range(6)) + tuple(f"controlnet_down_blocks.{i}." for i in range(12)):
        assert any(k.startswith(prefix) for k in want), prefix
    assert not any(k.startswith(("controlnet_cond_embedding.blocks.6.", "controlnet_down_blocks.12.", "up_blocks.", "conv_out.")) for k in want)
    count = 0
    for shp in want.values():
        n = 1
        for s in shp:
            n *= s
        count += n
    cfg = dict(OU.SD15_UNET_CONFIG, conditioning_embedding_out_channels=(16, 32, 96, 256), conditioning_channels=3)
    assert count == R.controlnet_param_count(cfg) == sum(p.numel() for p in ref.parameters())


def test_save_from_pretrained_round_trip_is_exact(tmp_path):
    from gm_diffusion.components import ControlNetModel

    cfg = R.tiny_controlnet_config()
    m = ControlNetModel(**cfg).init_random(7)
    assert all(bool(v.any()) for k, v in m.state_dict().items() if k.startswith("controlnet_") and k.endswith("weight"))  # non-zero zero-convs
    m.save_pretrained(str(tmp_path / "cn"))
    back = ControlNetModel.from_pretrained(str(tmp_path), subfolder="cn", torch_dtype=torch.bfloat16)
    as_json = lambda c: {k: (list(v) if isinstance(v, (tuple, list)) else v) for k, v in c.items()}  # JSON has no tuples
    assert back.dtype == torch.bfloat16 and as_json(back.config) == as_json(m.config)
    a, b = m.state_dict(), back.state_dict()
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    # the reference's own weights load under diffusers' names
    ref = _tiny_ref()
    ControlNetModel(**cfg).load_state_dict(ref.state_dict())


def test_from_unet_copies_the_encoder_and_zeroes_the_zero_convs():
    from gm_diffusion.components import ControlNetModel, UNet2DConditionModel

    ou = fixtures.build_unet("tiny", 4)
    hu = UNet2DConditionModel(**vars(ou.config))
    hu.load_state_dict(ou.state_dict())
    cn = ControlNetModel.from_unet(hu, conditioning_embedding_out_channels=(8, 8, 16, 16))
    sd, src = cn.state_dict(), hu.state_dict()
    for k, v in sd.items():
        if k in src:
            assert torch.equal(v, src[k]), k
        elif cn._is_zero_conv(k):
            assert not bool(v.any()), k
        elif k.endswith("weight"):
            assert bool(v.any()), k
    assert sum(1 for k in sd if k in src) == sum(1 for k in src if k.startswith(("conv_in.", "time_embedding.", "down_blocks.", "mid_block.")))


# ---------------------------------------------------------------------------------------------------------------------------
# window, scales, refusals
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 7, 50])
@pytest.mark.parametrize("start,end", [(0.0, 1.0), (0.5, 1.0), (0.0, 0.5), (0.25, 0.75), (0.3, 0.31), (0.9, 1.0)])
def test_window_rule_against_the_one_liner(n, start, end):
    from gm_diffusion.components.controlnet import control_window
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline as P

    want = [bool(1.0 - float(i / n < start or (i + 1) / n > end)) for i in range(n)]
    assert [control_window(i, n, start, end) for i in range(n)] == want == R.keep_window(n, start, end) == P._control_keep(n, start, end)


@pytest.mark.parametrize("scale", [1.0, 0.3, 0.0, 2.5])
def test_scales_against_the_one_liner(scale):
    from gm_diffusion.components.controlnet import control_scales

    assert torch.equal(control_scales(scale, True), torch.logspace(-1, 0, 13) * scale)
    assert torch.equal(control_scales(scale, False), torch.full((13,), scale, dtype=torch.float32))
    assert control_scales(scale, True).dtype == torch.float32 and [float(v) for v in control_scales(scale, True)] == R.guess_scales(scale)


def _cpu_pipe(controlnet):
    from gm_diffusion.components import PNDMScheduler, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline

    def hip(om):
        m = UNet2DConditionModel(**vars(om.config))
        return m.load_state_dict(om.state_dict())

    sch = PNDMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", skip_prk_steps=True, steps_offset=1)
    return StableDiffusionDualUNetPipeline(vae=None, text_encoder=None, tokenizer=None, unet=hip(fixtures.build_unet("tiny", 4)),
                                           gm_unet=hip(fixtures.build_unet("tiny", 8)), scheduler=sch, safety_checker=None,
                                           feature_extractor=None, requires_safety_checker=False, controlnet=controlnet)


def test_refusals_raise_before_touching_a_gpu():
    from gm_diffusion.components import ControlNetModel
    from gm_diffusion.pipelines import StableDiffusionDualUNetImprovedPipeline, StableDiffusionDualUNetPipeline

    cfg = R.tiny_controlnet_config()
    for key, val in (("controlnet_conditioning_channel_order", "bgr"), ("global_pool_conditions", True)):
        with pytest.raises(NotImplementedError, match=key):
            ControlNetModel(**dict(cfg, **{key: val}))
    cn = ControlNetModel(**cfg).init_random(1)
    with pytest.raises(NotImplementedError):
        _cpu_pipe([cn, cn])
    assert issubclass(StableDiffusionDualUNetImprovedPipeline, StableDiffusionDualUNetPipeline)
    pipe = _cpu_pipe(cn)
    assert pipe.controlnet is cn and "controlnet" in pipe.components
    pos, neg, lat = fixtures.make_inputs(1, 8, 8, cross_dim=64)
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, latents=lat, height=64, width=64, num_inference_steps=2, output_type="latent")
    with pytest.raises(ValueError, match="control_image"):
        pipe(**kw)  # missing
    with pytest.raises(ValueError, match="control_image"):
        pipe(control_image=torch.rand(1, 3, 32, 64), **kw)  # wrong size
    with pytest.raises(ValueError, match="control_image"):
        pipe(control_image=torch.rand(3, 3, 64, 64), **kw)  # wrong count
    with pytest.raises(NotImplementedError):
        pipe(control_image=torch.rand(1, 3, 64, 64), controlnet_conditioning_scale=[1.0, 0.5], **kw)
    with pytest.raises(ValueError, match="window"):
        pipe(control_image=torch.rand(1, 3, 64, 64), control_guidance_start=0.8, control_guidance_end=0.2, **kw)


def test_without_a_controlnet_the_five_keywords_are_ignored():
    """controlnet=None: the keywords stay unknown keywords (no validation, no effect): the call gets as far as the HIP models, which
    refuse the CPU -- with and without the keywords alike."""
    from gm_diffusion._native import HipExtensionError

    pipe = _cpu_pipe(None)
    assert pipe.controlnet is None
    pos, neg, lat = fixtures.make_inputs(1, 8, 8, cross_dim=64)
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, latents=lat, height=64, width=64, num_inference_steps=2, output_type="latent")
    errs = []
    for extra in ({}, dict(control_image="not even an image", controlnet_conditioning_scale=[1, 2], guess_mode=True,
                           control_guidance_start=0.9, control_guidance_end=0.1)):
        with pytest.raises(HipExtensionError) as e:
            pipe(**kw, **extra)
        errs.append(str(e.value))
    assert errs[0] == errs[1]


# ---------------------------------------------------------------------------------------------------------------------------
# the checkers, shown failing
# ---------------------------------------------------------------------------------------------------------------------------
def _concat_case(dtype=torch.bfloat16, rows=128, r_row0=64, seed=1):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(rows, 24, generator=g).to(dtype), torch.randn(rows, 40, generator=g).to(dtype)
    ra, rb = torch.randn(rows - r_row0, 24, generator=g).to(dtype), torch.randn(rows - r_row0, 40, generator=g).to(dtype)
    scales = torch.linspace(0.1, 1.3, 13)
    return a, b, ra, rb, scales


def test_concat_checker_passes_the_expression_and_fails_on_its_two_faults():
    a, b, ra, rb, scales = _concat_case()
    good = R.concat_add_ref(a, b, ra, rb, scales, 12, 5, 64)
    R.assert_concat(good, a, b, ra, rb, scales, 12, 5, 64, "clean")
    assert torch.equal(good[:64], torch.cat([a, b], -1)[:64]) and not torch.equal(good[64:], torch.cat([a, b], -1)[64:])
    with pytest.raises(AssertionError, match="differ"):
        R.assert_concat(R.concat_add_ref(a, b, ra, rb, scales, 12, 5, 64, fault="row0_ignored"), a, b, ra, rb, scales, 12, 5, 64, "r_row0 ignored")
    with pytest.raises(AssertionError, match="differ"):
        R.assert_concat(R.concat_add_ref(a, b, ra, rb, scales, 12, 5, 64, fault="scale_after_add"), a, b, ra, rb, scales, 12, 5, 64, "scale after add")
    with pytest.raises(AssertionError, match="differ"):  # the wrong entry of the scales array
        R.assert_concat(R.concat_add_ref(a, b, ra, rb, scales, 12, 4, 64), a, b, ra, rb, scales, 12, 5, 64, "wrong scale index")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_edge_values_do_what_their_names_say(dtype):
    s, r = R.edge_values(dtype)
    one = torch.ones(13)
    out = R.concat_add_ref(s[:, None].repeat(1, 8), s[:, None].repeat(1, 8), r[:, None].repeat(1, 8), None, one, 0, 0, 0)[:, 0]
    assert torch.signbit(out[3]) and not torch.signbit(out[1]) and not torch.signbit(out[2])  # -0 + -0 = -0; a +0 on either side wins
    assert float(out[5]) == 1.0 and float(out[6]) > float(s[6])  # both exact ties: to even (down to 1, up from 1 + 2u)
    if dtype == torch.float16:
        p = r[4] * 0.3
        assert 0 < float(p) < 2.0 ** -14  # subnormal product


def test_stats_checker_passes_fresh_sums_and_fails_on_stale_and_unwritten_entries():
    g = torch.Generator().manual_seed(2)
    skip = torch.randn(128, 20, generator=g).to(torch.bfloat16)
    res = torch.randn(128, 20, generator=g).to(torch.bfloat16)
    stored = skip + res * 0.7
    fresh = SH.bucket_sums(stored, 10).float()
    R.assert_stats(fresh, stored, 10, "fresh")
    stale = SH.bucket_sums(skip, 10).float()  # what the skip's producer left: right for the skip, wrong for the sum
    with pytest.raises(AssertionError, match="outside their bound"):
        R.assert_stats(stale, stored, 10, "stale")
    holed = fresh.clone()
    holed[1, 0, 1] = float("nan")
    with pytest.raises(AssertionError, match="never written"):
        R.assert_stats(holed, stored, 10, "unwritten")
