"""GPU: image heights / widths divisible by 8 but not by 64 (latent sides not multiples of 2 ** (levels - 1)), as the reference
pipelines accept them -- the fused nearest upsample to a given output size in every conv kernel family, the UNets against the
test-local yardstick (tests/anysize_ref.py), the VAE with odd latent sides, both pipelines, and a 1920x1080 run by properties.
Every gate is the one the existing test of the same object and dtype uses."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from anysize_ref import bind

pytestmark = pytest.mark.gpu
DEV = "cuda"
RMS_TOL = 1e-3  # tests/test_pipeline_gpu.py


def ops():
    from gm_diffusion import hip_ops

    return hip_ops


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def tol(dtype):  # tests/test_kernels_gpu.py
    return 2e-5 if dtype == torch.float32 else (1.5e-2 if dtype == torch.bfloat16 else 2e-3)


MODES = [(torch.float32, "exact"), (torch.float32, "split"), (torch.bfloat16, "split"), (torch.float16, "split")]


@pytest.fixture
def force_plan():
    """gmd_gemm_plan_override is refused unless the process has GMD_TUNING=1 (include/gmd_hip.h); reset afterwards."""
    from gm_diffusion._native import lib

    prev = os.environ.get("GMD_TUNING")
    os.environ["GMD_TUNING"] = "1"

    def force(bm, bn, pf, ks):
        assert lib().gmd_gemm_plan_override(bm, bn, pf, ks) == 0

    yield force
    lib().gmd_gemm_plan_override(0, 0, 0, 0)
    if prev is None:
        os.environ.pop("GMD_TUNING", None)
    else:
        os.environ["GMD_TUNING"] = prev


@pytest.fixture(params=["split", "exact"])
def f32_mode(request):
    prev = ops().set_f32_mode(request.param)
    yield request.param
    ops().set_f32_mode(prev)


def _sizes(H, W):
    return [(2 * H - 1, 2 * W), (2 * H, 2 * W - 1), (2 * H - 1, 2 * W - 1)]


def _conv_case(B, H, W, Cin, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    bias = torch.randn(Cout, generator=g)
    tb = torch.randn(B, Cout, generator=g)
    return g, x, w, bias, tb


def _check_conv(dtype, B, H, W, Cin, Cout, sizes, seed=0, gate=None):
    """conv3x3(out_size=...) with bias + rowbias + residual and with out_dtype=float32, against float64
    F.conv2d(F.interpolate(x, size=..., mode="nearest"), w, padding=1) of the operands as rounded to ``dtype``."""
    o = ops()
    gate = gate or tol(dtype)
    g, x, w, bias, tb = _conv_case(B, H, W, Cin, Cout, seed or H * W + Cin + Cout)
    x, w = x.to(dtype), w.to(dtype)
    xl = x.permute(0, 2, 3, 1).reshape(B, H * W, Cin).contiguous().to(DEV)
    wl = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous().to(DEV)
    for Ho, Wo in sizes:
        ref = F.conv2d(F.interpolate(x.double(), size=(Ho, Wo), mode="nearest"), w.double(), bias.double(), padding=1)
        res = torch.randn(B, Ho * Wo, Cout, generator=g).to(dtype)
        y, ho, wo = o.conv3x3(xl, wl, B, H, W, bias=bias.to(DEV), rowbias=tb.to(DEV), residual=res.to(DEV), out_size=(Ho, Wo))
        assert (ho, wo) == (Ho, Wo) and y.shape == (B, Ho * Wo, Cout) and y.dtype == dtype
        full = (ref + tb.double()[:, :, None, None]).permute(0, 2, 3, 1).reshape(B, Ho * Wo, Cout) + res.double()
        e1 = rel_err(y.float(), full)
        y32, _, _ = o.conv3x3(xl, wl, B, H, W, bias=bias.to(DEV), out_dtype=torch.float32, out_size=(Ho, Wo))
        e2 = rel_err(y32, ref.permute(0, 2, 3, 1).reshape(B, Ho * Wo, Cout))
        print(f"conv {dtype} {B}x{H}x{W} {Cin}->{Cout} to {Ho}x{Wo}: {e1:.3e} {e2:.3e} (gate {gate:.1e})")
        assert y32.dtype == torch.float32 and e1 < gate and e2 < gate, (Ho, Wo, e1, e2)


# (2, 4, 6, 128, 64): a handful of rows (64x64 ring tiles);  (1, 16, 12, 128, 320) / (3, 12, 10, 128, 320): ragged M on the planner's tiles;
# (4, 16, 16, 320, 320): ~3.8k rows, the loader/consumer range;  (2, 33, 31, 64, 320): 8k rows, 256-row tiles + the division path of the
# pixel decomposition;  (8, 8, 8, 1280, 1280): the split-K range of the 16x16 level
SHAPES = [(2, 4, 6, 128, 64), (1, 16, 12, 128, 320), (3, 12, 10, 128, 320), (4, 16, 16, 320, 320), (2, 33, 31, 64, 320), (8, 8, 8, 1280, 1280)]


@pytest.mark.parametrize("dtype,mode", MODES)
@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_conv3x3_upsample_to_size_planner_shapes(dtype, mode, B, H, W, Cin, Cout):
    prev = ops().set_f32_mode(mode)
    try:
        _check_conv(dtype, B, H, W, Cin, Cout, _sizes(H, W))
    finally:
        ops().set_f32_mode(prev)


@pytest.mark.parametrize("dtype,mode", MODES)
@pytest.mark.parametrize("H,W,C,size", [(17, 30, 1280, (34, 60)), (34, 60, 1280, (68, 120)), (68, 120, 640, (135, 240))])
def test_conv3x3_upsampling_convolutions_of_sd15_at_1920x1080(dtype, mode, H, W, C, size):
    """The three upsampling convolutions of SD-1.5 on a 1920x1080 frame (latent 135x240): two exact 2x through the new argument, and
    the odd one (the 320-wide level has no upsampler)."""
    prev = ops().set_f32_mode(mode)
    try:
        _check_conv(dtype, 1, H, W, C, C, [size])
    finally:
        ops().set_f32_mode(prev)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("plan", [(256, 160, 283, 1), (256, 128, 283, 1), (128, 160, 244, 1), (64, 160, 244, 1), (256, 160, 283, 2), (256, 128, 283, 3),
                                  (128, 160, 9, 1), (128, 128, 9, 2), (64, 64, 9, 1)])
def test_conv3x3_upsample_to_size_every_16bit_kernel_family(dtype, plan, force_plan):
    """Through the debug plan override: the ping-pong kernel (256-row tiles), the loader / consumer kernel (128- and 64-row tiles), the
    ring kernels, and split-K over each -- odd sizes, a sample seam inside a tile, ragged last tile."""
    B, H, W, ci, co = 3, 12, 10, 128, 320
    force_plan(*plan)  # (pf 9 = the LDS-DMA ring kernels, 283 = ping-pong, 244 = loader / consumer)
    _check_conv(dtype, B, H, W, ci, co, _sizes(H, W), seed=sum(plan))


@pytest.mark.parametrize("dtype,mode", MODES)
def test_conv3x3_exact_2x_through_out_size_is_the_upsample_launch(dtype, mode):
    o = ops()
    prev = o.set_f32_mode(mode)
    try:
        g = torch.Generator().manual_seed(3)
        B, H, W, ci, co = 2, 12, 10, 128, 320
        x = torch.randn(B, H * W, ci, generator=g).to(dtype).to(DEV)
        w = (torch.randn(co, 9 * ci, generator=g) * 0.03).to(dtype).to(DEV)
        b = torch.randn(co, generator=g).to(DEV)
        y1, h1, w1 = o.conv3x3(x, w, B, H, W, bias=b, upsample=True)
        y2, h2, w2 = o.conv3x3(x, w, B, H, W, bias=b, out_size=(2 * H, 2 * W))
        assert (h1, w1) == (h2, w2) == (2 * H, 2 * W) and torch.equal(y1, y2)
        # ... and the packed form of the C ABI for the same size is the same launch too
        from gm_diffusion._native import check, lib

        y3 = torch.empty_like(y1)
        code = o.GMD_F32S if (dtype == torch.float32 and mode == "split") else o.dtype_code(dtype)
        ws = o.new_workspace(x.device)
        check(lib().gmd_conv3x3(x.data_ptr(), w.data_ptr(), y3.data_ptr(), code, o.dtype_code(dtype), B, H, W, ci, co, 1, (2 * H << 16) | (2 * W), 0,
                                b.data_ptr(), None, 0, None, 1.0, None, 0, ws.data_ptr(), o.WORKSPACE_BYTES, None), "gmd_conv3x3")
        torch.cuda.synchronize()
        assert torch.equal(y1, y3)
        with pytest.raises(o.HipExtensionError, match="out_size"):
            o.conv3x3(x, w, B, H, W, bias=b, out_size=(2 * H + 1, 2 * W))
    finally:
        o.set_f32_mode(prev)


@pytest.mark.parametrize("dtype,mode", [(torch.bfloat16, "split"), (torch.float16, "split"), (torch.float32, "split")])
def test_conv3x3_groupnorm_fusion_over_split_k_slabs_with_upsample_to_size(dtype, mode):
    """gmd_conv3x3_groupnorm (split-K slabs summed by the GroupNorm kernel) sees Hout * Wout rows: 8 x 8 -> 15 x 16 / 16 x 15 / 15 x 15 at
    1280 channels, batch 8 (the fusable range), against gmd_conv3x3 + groupnorm (bit-identical by the entry point's contract) and
    against float64."""
    from gm_diffusion._native import check, lib

    o = ops()
    prev = o.set_f32_mode(mode)
    try:
        B, H, W, C, G = 8, 8, 8, 1280, 32
        g, x, w, bias, tb = _conv_case(B, H, W, C, C, 77)
        x, w = x.to(dtype), w.to(dtype)
        xl = x.permute(0, 2, 3, 1).reshape(B, H * W, C).contiguous().to(DEV)
        wl = w.permute(0, 2, 3, 1).reshape(C, 9 * C).contiguous().to(DEV)
        gamma, beta = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
        bd, tbd = bias.to(DEV), tb.to(DEV)
        code = o.GMD_F32S if dtype == torch.float32 else o.dtype_code(dtype)
        ws = o.new_workspace(xl.device)
        for Ho, Wo in _sizes(H, W):
            up = (Ho << 16) | Wo
            assert lib().gmd_conv3x3_gn_fusable(code, B, H, W, C, C, 1, up, 0, G, o.WORKSPACE_BYTES) == 1
            yr = torch.empty((B, Ho * Wo, C), dtype=dtype, device=DEV)
            yn = torch.empty_like(yr)
            check(lib().gmd_conv3x3_groupnorm(xl.data_ptr(), wl.data_ptr(), yr.data_ptr(), yn.data_ptr(), code, B, H, W, C, C, 1, up, 0,
                                              bd.data_ptr(), tbd.data_ptr(), C, None, 1.0, G, 1e-5, gamma.data_ptr(), beta.data_ptr(), 1,
                                              ws.data_ptr(), o.WORKSPACE_BYTES, None), "gmd_conv3x3_groupnorm")
            torch.cuda.synchronize()
            y, _, _ = o.conv3x3(xl, wl, B, H, W, bias=bd, rowbias=tbd, out_size=(Ho, Wo))
            n = o.groupnorm(y, B, G, gamma, beta, 1e-5, silu=True)
            assert torch.equal(yr, y) and torch.equal(yn, n)
            ref = F.conv2d(F.interpolate(x.double(), size=(Ho, Wo), mode="nearest"), w.double(), bias.double(), padding=1) + tb.double()[:, :, None, None]
            assert rel_err(yr.float(), ref.permute(0, 2, 3, 1).reshape(B, Ho * Wo, C)) < tol(dtype)
            rn = F.silu(F.group_norm(ref, G, gamma.double().cpu(), beta.double().cpu(), 1e-5)).permute(0, 2, 3, 1).reshape(B, Ho * Wo, C)
            assert rel_err(yn.float(), rn) < tol(dtype)
    finally:
        o.set_f32_mode(prev)


# ---------------------------------------------------------------------------------------------
# UNet against the test-local yardstick
# ---------------------------------------------------------------------------------------------
def _hip(cls, om, dtype):
    m = cls(**vars(om.config))
    m.load_state_dict(om.state_dict())
    return m.to(DEV, dtype)


def _hip_unet(ou, dtype):
    from gm_diffusion.components import UNet2DConditionModel

    return _hip(UNet2DConditionModel, ou, dtype)


@pytest.mark.parametrize("in_ch", [4, 8])
@pytest.mark.parametrize("dtype,mode,gate", [(torch.float32, "split", 2e-5), (torch.float32, "exact", 2e-5), (torch.bfloat16, "split", 3e-2)])
def test_tiny_unet_forward_odd_latents(in_ch, dtype, mode, gate):
    from oracle import fixtures

    prev = ops().set_f32_mode(mode)
    try:
        ou = bind(fixtures.build_unet("tiny", in_ch))
        hu = _hip_unet(ou, dtype)
        for h, w in ((17, 13), (15, 30), (27, 48)):
            g = torch.Generator().manual_seed(3 + h)
            x = torch.randn(2, in_ch, h, w, generator=g)
            ctx = torch.randn(2, 77, ou.config.cross_attention_dim, generator=g)
            for t in (981, 41):
                ref = ou(x, torch.tensor(t), encoder_hidden_states=ctx)[0]
                got = hu(x.to(DEV), t, encoder_hidden_states=ctx.to(DEV), return_dict=False)[0]
                e = rel_err(got, ref)
                print(f"tiny unet {in_ch}ch {dtype} {mode} {h}x{w} t={t}: {e:.3e} (gate {gate:.0e})")
                assert got.dtype == torch.float32 and got.shape == ref.shape and e < gate, (h, w, t, e)
        # tuple input (conditioning first) and the captured graph, at an odd size
        if in_ch == 8:
            a, b = x[:, :4].contiguous(), x[:, 4:].contiguous()
            got_t = hu((a.to(DEV), b.to(DEV)), 41, encoder_hidden_states=ctx.to(DEV), return_dict=False)[0]
            assert torch.equal(got_t, got)
        c = hu.prepare_context(ctx.to(DEV))
        hu.set_timestep(41)
        gph = hu.graphed_forward(2, 27, 48, c)
        hu.pack_input(x.to(DEV), out=gph.x)
        assert torch.equal(gph.replay(), got)
    finally:
        ops().set_f32_mode(prev)


@pytest.mark.parametrize("dtype,mode,gate", [(torch.float32, "split", 3e-5), (torch.float32, "exact", 3e-5), (torch.bfloat16, "split", 4e-2),
                                             (torch.float16, "split", 6e-3)])
def test_tiny_sdxl_style_unet_forward_odd_latent(dtype, mode, gate):
    from oracle import unet as OU

    o = ops()
    prev = o.set_f32_mode(mode)
    try:
        torch.manual_seed(77)
        ou = bind(OU.UNet2DConditionModel(**OU.tiny_sdxl_unet_config()).eval().requires_grad_(False))
        hu = _hip_unet(ou, dtype)
        c_ = ou.config
        g = torch.Generator().manual_seed(50)
        x = torch.randn(2, c_.in_channels, 17, 11, generator=g)
        ctx = torch.randn(2, 9, c_.cross_attention_dim, generator=g)
        P = c_.projection_class_embeddings_input_dim - 6 * c_.addition_time_embed_dim
        kw = dict(text_embeds=torch.randn(2, P, generator=g), time_ids=torch.tensor([[1024.0, 768, 0, 16, 1024, 768], [512, 512, 32, 0, 640, 512]]))
        ref = ou(x, torch.tensor(333), encoder_hidden_states=ctx, added_cond_kwargs=kw)[0]
        dkw = {k: v.to(DEV) for k, v in kw.items()}
        got = hu(x.to(DEV), 333, encoder_hidden_states=ctx.to(DEV), added_cond_kwargs=dkw, return_dict=False)[0]
        e = rel_err(got, ref)
        print(f"sdxl-style unet {dtype} {mode} 17x11: {e:.3e} (gate {gate:.0e})")
        assert got.shape == ref.shape and e < gate, e
        c = hu.prepare_context(ctx.to(DEV))
        hu.set_timestep(333)
        hu.set_added_cond(dkw, 2)
        gph = hu.graphed_forward(2, 17, 11, c)
        hu.pack_input(x.to(DEV), out=gph.x)
        assert torch.equal(gph.replay(), got)
    finally:
        o.set_f32_mode(prev)


@pytest.mark.parametrize("h,w", [(9, 11), (34, 33)])
def test_sd15_unet_forward_f32_odd_latents(h, w):
    """Full SD-1.5 channel configuration; 34x33: 1122 tokens at the top level (>= 1024, not a multiple of 64: the GroupNorms and the
    self-attention projections take their general routes)."""
    from oracle import fixtures

    ou = bind(fixtures.build_unet("sd15", 8))
    hu = _hip_unet(ou, torch.float32)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 8, h, w, generator=g)
    ctx = torch.randn(1, 77, 768, generator=g)
    ref = ou(x, torch.tensor(701), encoder_hidden_states=ctx)[0]
    got = hu(x.to(DEV), 701, encoder_hidden_states=ctx.to(DEV), return_dict=False)[0]
    e = rel_err(got, ref)
    print(f"sd15 unet f32 {h}x{w}: {e:.3e} (gate 3e-5)")
    assert got.shape == ref.shape and e < 3e-5, e


@pytest.mark.parametrize("dtype,gate", [(torch.float32, 1e-5), (torch.bfloat16, 2e-2)])
def test_unet_cfg_shared_prefix_equals_duplicated_batch_odd_latent(dtype, gate):
    from oracle import fixtures

    ou = bind(fixtures.build_unet("tiny", 4))
    hu = _hip_unet(ou, dtype)
    g = torch.Generator().manual_seed(23)
    lat = torch.randn(3, 4, 17, 13, generator=g)
    ctx = torch.randn(6, 77, ou.config.cross_attention_dim, generator=g)
    ref = ou(torch.cat([lat, lat]), torch.tensor(601), encoder_hidden_states=ctx)[0]
    hu._ensure()
    c = hu.prepare_context(ctx.to(DEV))
    hu.set_timestep(601)
    full = hu.forward_packed(hu.pack_input(lat.to(DEV), dup=2), 6, 17, 13, c)
    shared = hu.forward_packed(hu.pack_input(lat.to(DEV), dup=1), 6, 17, 13, c, cfg_shared=True)
    assert shared.shape == full.shape == (6, 4, 17, 13)
    assert rel_err(shared, full) < gate and rel_err(shared, ref) < max(gate, 3e-5 if dtype == torch.float32 else 3e-2)
    assert not torch.equal(shared[:3], shared[3:])
    gph = hu.graphed_forward(6, 17, 13, c, cfg_shared=True)
    hu.pack_input(lat.to(DEV), dup=1, out=gph.x)
    assert torch.equal(gph.replay(), shared)


# ---------------------------------------------------------------------------------------------
# VAE with odd latent sides (image 136 x 104 = latent 17 x 13: 221 tokens in the mid-block attention)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,gate", [(torch.float32, 2e-5), (torch.bfloat16, 3e-2)])
def test_tiny_vae_decode_odd_latent(dtype, gate):
    from gm_diffusion.components import AutoencoderKL
    from oracle import fixtures

    ov = fixtures.build_vae("tiny")
    hv = _hip(AutoencoderKL, ov, dtype)
    z = torch.randn(2, 4, 17, 13, generator=torch.Generator().manual_seed(9)) * 3
    ref = ov.decode(z)[0]
    got = hv.decode(z.to(DEV), return_dict=False)[0]
    e = rel_err(got, ref)
    print(f"tiny vae decode {dtype} 17x13: {e:.3e} (gate {gate:.0e})")
    assert got.shape == ref.shape == (2, 3, 136, 104) and e < gate, e


def test_tiny_vae_encode_f32_odd_latent():
    from gm_diffusion.components import AutoencoderKL
    from oracle import fixtures

    ov = fixtures.build_vae("tiny", with_encoder=True)
    hv = _hip(AutoencoderKL, ov, torch.float32)
    x = torch.rand(1, 3, 136, 104, generator=torch.Generator().manual_seed(2)) * 2 - 1
    ref = ov.encode(x).latent_dist
    got = hv.encode(x.to(DEV)).latent_dist
    assert tuple(got.mean.shape) == (1, 4, 17, 13)
    assert rel_err(got.mean, ref.mean) < 2e-5 and rel_err(got.std, ref.std) < 2e-5
    s1 = got.sample(torch.Generator().manual_seed(5)).cpu()
    s2 = ref.sample(torch.Generator().manual_seed(5))
    assert rel_err(s1, s2) < 2e-5


def test_composed_attention_walks_query_rows_in_chunks(monkeypatch):
    """The score matrix of the VAE mid-block attention is held for a bounded number of query rows at a time (1920x1080: 32,400 tokens
    would need 4.2 GB at once): with the bound lowered so that 221 tokens take several ragged chunks the decode must not change
    beyond the float32 gate (a row's softmax needs only its own scores)."""
    from gm_diffusion.components import AutoencoderKL, unet_2d_condition as U
    from oracle import fixtures

    ov = fixtures.build_vae("tiny")
    hv = _hip(AutoencoderKL, ov, torch.float32)
    z = (torch.randn(1, 4, 33, 31, generator=torch.Generator().manual_seed(9)) * 3).to(DEV)  # 1023 tokens
    whole = hv.decode(z, return_dict=False)[0]
    monkeypatch.setattr(U, "SCORE_CHUNK_BYTES", 256 * 1024 * 4)  # 256 rows of 1024 scores: chunks of 256, 256, 256, 255
    chunked = hv.decode(z, return_dict=False)[0]
    assert rel_err(chunked, whole) < 2e-5 and rel_err(chunked, ov.decode(z.cpu())[0]) < 2e-5


# ---------------------------------------------------------------------------------------------
# pipelines, image 136 x 104
# ---------------------------------------------------------------------------------------------
def _pndm():
    from gm_diffusion.components import PNDMScheduler

    return PNDMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", skip_prk_steps=True, steps_offset=1, set_alpha_to_one=False)


def _rms(a, b):
    from oracle import pipelines as opipe

    return opipe.latent_rms(a.detach().cpu() if torch.is_tensor(a) else a, b)


def _dual_pipe(dtype, ou, og, ov):
    from gm_diffusion.components import AutoencoderKL, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline

    pipe = StableDiffusionDualUNetPipeline(vae=_hip(AutoencoderKL, ov, dtype), text_encoder=None, tokenizer=None, unet=_hip(UNet2DConditionModel, ou, dtype),
                                           gm_unet=_hip(UNet2DConditionModel, og, dtype), scheduler=_pndm(), safety_checker=None,
                                           feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    return pipe


def test_dual_pipeline_f32_136x104_matches_oracle_loop(f32_mode):
    import numpy as np

    from gm_diffusion import hdr
    from gm_diffusion.pipelines import StableDiffusionDualUNetImprovedPipeline
    from oracle import fixtures, pipelines as opipe, schedulers as osched

    ou, og, ov = bind(fixtures.build_unet("tiny", 4)), bind(fixtures.build_unet("tiny", 8)), fixtures.build_vae("tiny")
    pos, neg, lat = fixtures.make_inputs(1, 17, 13, cross_dim=ou.config.cross_attention_dim)
    rec = []
    ref_sdr, ref_gm = opipe.dual_loop(ou, og, osched.PNDMScheduler(), pos, neg, lat, num_inference_steps=4, guidance_scale=7.5, record=rec)
    ref_tail = opipe.decode_tail(ov, ref_sdr, ref_gm, qmax=99)
    pipe = _dual_pipe(torch.float32, ou, og, ov)
    steps = []
    kw = dict(prompt_embeds=pos.to(DEV), negative_prompt_embeds=neg.to(DEV), latents=lat.to(DEV), height=136, width=104, num_inference_steps=4,
              guidance_scale=7.5, output_type="latent")
    pipe.use_hip_graphs, pipe.overlap_streams = False, False
    pipe.co_run_plans = True  # one plan family for eager / graphs / two streams, as tests/test_pipeline_gpu.py pins it
    pipe._step_probe = lambda i, a, b: steps.append((a.float().cpu(), b.float().cpu()))  # both latents of every iteration
    sdr, gm = pipe(**kw)
    pipe._step_probe = None
    assert len(rec) == 5 and len(steps) == len(rec)
    per_step = [(_rms(a, rec[i][0]), _rms(b, rec[i][1])) for i, (a, b) in enumerate(steps)]
    print(f"dual 136x104 {f32_mode}: per-step (sdr, gm) latent RMS {per_step}")
    assert max(max(p_) for p_ in per_step) <= RMS_TOL, per_step
    assert sdr.shape == (1, 4, 17, 13) and _rms(sdr, ref_sdr) <= RMS_TOL and _rms(gm, ref_gm) <= RMS_TOL
    # graphs and two streams: bit for bit what the eager single-stream run gave
    pipe.use_hip_graphs = True
    b = pipe(**kw)
    pipe.overlap_streams = True
    c = pipe(**kw)
    torch.cuda.synchronize()
    for x in (b, c):
        assert torch.equal(sdr, x[0]) and torch.equal(gm, x[1])
    # the alias class takes the same sizes
    assert issubclass(StableDiffusionDualUNetImprovedPipeline, type(pipe))
    tail = hdr.decode_to_hdr(pipe.vae, sdr, gm, qmax=99)
    assert tail["hdr"].shape == (1, 136, 104, 3)
    assert _rms(tail["sdr"], ref_tail["sdr"]) <= 1e-4 and _rms(tail["gm"], ref_tail["gm"]) <= 1e-4
    ref_hdr = ref_tail["hdr"]
    assert _rms(tail["hdr"], ref_hdr) <= 1e-3 * max(1.0, float(np.abs(ref_hdr).max()))


def test_gm_pipeline_f32_136x104_matches_oracle_loop(f32_mode):
    from gm_diffusion.components import AutoencoderKL, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionGMPipeline
    from oracle import fixtures, pipelines as opipe, schedulers as osched

    og, ov = bind(fixtures.build_unet("tiny", 8)), fixtures.build_vae("tiny")
    pos, neg, lat = fixtures.make_inputs(1, 17, 13, cross_dim=og.config.cross_attention_dim)
    sdr_latent = torch.randn(1, 4, 17, 13, generator=torch.Generator().manual_seed(8))
    rec = []
    ref = opipe.gm_loop(og, osched.PNDMScheduler(), sdr_latent, pos, neg, lat, num_inference_steps=4, guidance_scale=7.5, record=rec)
    pipe = StableDiffusionGMPipeline(vae=_hip(AutoencoderKL, ov, torch.float32), text_encoder=None, tokenizer=None,
                                     unet=_hip(UNet2DConditionModel, og, torch.float32), scheduler=_pndm(), safety_checker=None,
                                     feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    steps = []
    kw = dict(prompt_embeds=pos.to(DEV), negative_prompt_embeds=neg.to(DEV), latents=lat.to(DEV), num_inference_steps=4, guidance_scale=7.5,
              output_type="latent")
    pipe.use_hip_graphs = False
    out = pipe(sdr_latent.to(DEV), **kw, callback_on_step_end=lambda p, i, t, k: (steps.append(k["latents"].cpu()) or {})).images
    per_step = [_rms(s, rec[i]) for i, s in enumerate(steps)]
    print(f"gm 136x104 {f32_mode}: per-step latent RMS {per_step}")
    assert len(per_step) == len(rec) == 5 and max(per_step) <= RMS_TOL, per_step
    assert out.shape == (1, 4, 17, 13) and _rms(out, ref) <= RMS_TOL
    pipe.use_hip_graphs = True
    assert torch.equal(pipe(sdr_latent.to(DEV), **kw).images, out)
    img = pipe(sdr_latent.to(DEV), **dict(kw, output_type="pt")).images
    assert tuple(img.shape[-2:]) == (136, 104)


# ---------------------------------------------------------------------------------------------
# 1920 x 1080, by properties (style of tests/test_fullsize_gpu.py)
# ---------------------------------------------------------------------------------------------
def test_dual_pipeline_1920x1080_bf16_properties():
    from gm_diffusion import hdr
    from gm_diffusion.components import AutoencoderKL, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline

    dt = torch.bfloat16
    pipe = StableDiffusionDualUNetPipeline(vae=AutoencoderKL().init_random(9).to(DEV, dt), text_encoder=None, tokenizer=None,
                                           unet=UNet2DConditionModel(in_channels=4).init_random(7).to(DEV, dt),
                                           gm_unet=UNet2DConditionModel(in_channels=8).init_random(8).to(DEV, dt), scheduler=_pndm(),
                                           safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    g = torch.Generator().manual_seed(1080)
    pe, ne = torch.randn(2, 77, 768, generator=g).to(DEV), torch.randn(2, 77, 768, generator=g).to(DEV)
    lat = torch.randn(2, 4, 135, 240, generator=g).to(DEV)
    kw = dict(height=1080, width=1920, num_inference_steps=2, guidance_scale=7.5, output_type="latent")
    one = dict(kw, prompt_embeds=pe[:1], negative_prompt_embeds=ne[:1], latents=lat[:1])
    pipe.co_run_plans = True
    pipe.use_hip_graphs, pipe.overlap_streams = True, True
    a = pipe(**one)
    pipe.use_hip_graphs, pipe.overlap_streams = False, False
    e = pipe(**one)
    assert a[0].shape == a[1].shape == (1, 4, 135, 240)
    assert torch.equal(a[0], e[0]) and torch.equal(a[1], e[1])
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()
    # batch independence: sample 0 of a batch of 2 is the batch-1 run, to bf16 rounding (the launches' plans differ with the batch:
    # the bound of test_unet_1024_batch_independence)
    two = pipe(**dict(kw, prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat))
    for k in (0, 1):
        assert rel_err(two[k][:1].float(), a[k].float()) < 3e-2
    out = hdr.decode_to_hdr(pipe.vae, a[0], a[1], qmax=99.0, want=("sdr", "gm", "hdr"))
    assert out["hdr"].shape == (1, 1080, 1920, 3) and torch.isfinite(out["hdr"]).all()
    assert float(out["sdr"].min()) >= 0 and float(out["sdr"].max()) <= 1
    img = pipe.vae.decode(a[0] / pipe.vae.config.scaling_factor, return_dict=False)[0]
    assert tuple(img.shape) == (1, 3, 1080, 1920) and torch.isfinite(img).all()
    assert torch.equal(ops().apply_gm_to_sdr(out["gm"], out["sdr"], qmax=99.0, eps=1 / 64, clamp=False), out["hdr"])
