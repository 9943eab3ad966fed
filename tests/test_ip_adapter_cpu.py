"""CPU: the host side of IP-Adapter image prompting -- checkpoint conversion (key -> layer), every refusal, the reference's
``prepare_ip_adapter_image_embeds`` / ``encode_image`` against a literal transcription of its expressions, local-file loading, the
distributed row slice -- and the per-element bound of the fused kernel (tests/ip_adapter_ref.py) shown to hold for a clean emulation
of its arithmetic and to break for the two faults it exists for (the project's convention: tests/test_parity_cpu.py)."""
import pytest
import torch

import ip_adapter_ref as R
from oracle import unet as OU


def _hip_unet(cfg=None):
    from gm_diffusion.components import UNet2DConditionModel

    return UNet2DConditionModel(**(OU.tiny_unet_config(4) if cfg is None else cfg))


def _pipe(unet=None, gm_unet=None, **kw):
    from gm_diffusion.components import PNDMScheduler
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline

    return StableDiffusionDualUNetPipeline(vae=None, text_encoder=None, tokenizer=None, unet=unet or _hip_unet(), gm_unet=gm_unet or _hip_unet(OU.tiny_unet_config(8)),
                                           scheduler=PNDMScheduler(skip_prk_steps=True, steps_offset=1), safety_checker=None,
                                           feature_extractor=kw.pop("feature_extractor", None), requires_safety_checker=False, **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# checkpoint conversion
# ---------------------------------------------------------------------------------------------------------------------------
def test_key_to_layer_tiny_round_trip():
    cfg = OU.tiny_unet_config(4)
    m = _hip_unet(cfg)
    sd = R.make_state_dict(cfg, tokens=4, clip_dim=32, seed=3)
    assert [(k, p) for k, p, _ in R.attn2_layers(cfg)] == m.ip_adapter_layers()
    m.load_ip_adapter(sd)
    assert m.has_ip_adapter and m._ip_raw["tokens"] == 4 and m._ip_raw["clip_dim"] == 32
    for k, path, dim in R.attn2_layers(cfg):  # each weight sits under its own number, untouched
        for nm in ("to_k_ip", "to_v_ip"):
            got = m._ip_raw["kv"][f"{k}.{nm}.weight"]
            assert tuple(got.shape) == (dim, 64) and torch.equal(got, sd["ip_adapter"][f"{k}.{nm}.weight"])
    assert all(torch.equal(m._ip_raw["proj"][k], v) for k, v in sd["image_proj"].items())
    m.unload_ip_adapter()
    assert not m.has_ip_adapter
    m.load_ip_adapter(sd)  # loading again after an unload is not "a second adapter"


def test_key_to_layer_sd15_shapes_only():
    m = _hip_unet({})  # the SD-1.5 configuration: no weights are created
    layers = m.ip_adapter_layers()
    assert [k for k, _ in layers] == list(range(1, 33, 2)) and len(layers) == 16
    assert layers[0] == (1, "down_blocks.0.attentions.0.transformer_blocks.0")
    assert layers[6] == (13, "up_blocks.1.attentions.0.transformer_blocks.0")
    assert layers[-1] == (31, "mid_block.attentions.0.transformer_blocks.0")
    assert [(k, p) for k, p, _ in R.attn2_layers({})] == layers
    proj, kv = m.ip_adapter_expected_keys(4, 1024)
    rp, rkv = R.expected_shapes({}, 4, 1024)
    assert proj == rp and kv == rkv
    assert kv["1.to_k_ip.weight"] == (320, 768) and kv["31.to_v_ip.weight"] == (1280, 768) and kv["13.to_k_ip.weight"] == (1280, 768)
    assert kv["29.to_k_ip.weight"] == (320, 768) and proj["proj.weight"] == (3072, 1024)
    # a shapes-only checkpoint (meta tensors) passes every check up to the copy
    meta = R.make_state_dict({}, 4, 1024, device="meta")
    bad = {"image_proj": meta["image_proj"], "ip_adapter": dict(meta["ip_adapter"])}
    bad["ip_adapter"]["31.to_k_ip.weight"] = torch.empty(640, 768, device="meta")
    with pytest.raises(ValueError, match=r"ip_adapter\.31\.to_k_ip\.weight.*\(1280, 768\).*\(640, 768\)"):
        m.load_ip_adapter(bad)


# ---------------------------------------------------------------------------------------------------------------------------
# refusals (none touches a GPU: the models are never placed on one)
# ---------------------------------------------------------------------------------------------------------------------------
def test_variants_are_refused_by_name():
    cfg = OU.tiny_unet_config(4)
    sd = R.make_state_dict(cfg, 4, 32)
    for extra, word in (("latents", "Plus"), ("proj.0.weight", "Full-Face"), ("perceiver_resampler.proj_in.weight", "FaceID")):
        m = _hip_unet(cfg)
        with pytest.raises(NotImplementedError, match=word):
            m.load_ip_adapter({"image_proj": {**sd["image_proj"], extra: torch.zeros(1)}, "ip_adapter": sd["ip_adapter"]})
        assert not m.has_ip_adapter
    m = _hip_unet(cfg).load_ip_adapter(sd)
    with pytest.raises(NotImplementedError, match="several adapters"):
        m.load_ip_adapter(sd)
    for bad in ([0.5, 0.5], {"down": 1.0}):
        with pytest.raises(NotImplementedError):
            m.set_ip_adapter_scale(bad)
    m.set_ip_adapter_scale(0.6)  # a float is recorded on the host; the device array is written when it exists
    assert m._ip_scale == 0.6
    with pytest.raises(ValueError, match="no IP-Adapter"):
        _hip_unet(cfg).set_ip_adapter_scale(1.0)


def test_shape_mismatch_names_key_expected_and_found():
    cfg = OU.tiny_unet_config(4)
    sd = R.make_state_dict(cfg, 4, 32)
    bad = {"image_proj": dict(sd["image_proj"]), "ip_adapter": dict(sd["ip_adapter"])}
    bad["ip_adapter"]["5.to_v_ip.weight"] = torch.zeros(64, 64)
    with pytest.raises(ValueError, match=r"ip_adapter\.5\.to_v_ip\.weight.*\(128, 64\).*\(64, 64\)"):
        _hip_unet(cfg).load_ip_adapter(bad)
    bad = {"image_proj": dict(sd["image_proj"], **{"norm.bias": torch.zeros(32)}), "ip_adapter": sd["ip_adapter"]}
    with pytest.raises(ValueError, match=r"image_proj\.norm\.bias.*\(64,\).*\(32,\)"):
        _hip_unet(cfg).load_ip_adapter(bad)
    bad = {"image_proj": dict(sd["image_proj"], **{"proj.weight": torch.zeros(100, 32)}), "ip_adapter": sd["ip_adapter"]}
    with pytest.raises(ValueError, match=r"proj\.weight"):
        _hip_unet(cfg).load_ip_adapter(bad)
    missing = {"image_proj": sd["image_proj"], "ip_adapter": {k: v for k, v in sd["ip_adapter"].items() if not k.startswith("31.")}}
    with pytest.raises(KeyError):
        _hip_unet(cfg).load_ip_adapter(missing)


def test_too_many_image_keys_and_missing_adapter_raise_before_any_launch():
    cfg = OU.tiny_unet_config(4)
    m = _hip_unet(cfg).load_ip_adapter(R.make_state_dict(cfg, 4, 32))
    with pytest.raises(ValueError, match="68 image keys"):  # 17 images x 4 tokens: refused on the host, the model is not even on a device
        m.prepare_ip_context(torch.zeros(2, 17, 32))
    with pytest.raises(ValueError, match=r"\[rows, n_images, 32\]"):
        m.prepare_ip_context(torch.zeros(2, 1, 48))
    with pytest.raises(ValueError, match="no IP-Adapter"):
        _hip_unet(cfg).prepare_ip_context(torch.zeros(2, 1, 32))
    with pytest.raises(NotImplementedError, match="several IP-Adapters"):
        m._single_adapter_embeds([torch.zeros(2, 1, 32)] * 2)
    assert m._single_adapter_embeds([torch.zeros(2, 32)]).shape == (2, 1, 32)


def test_pipeline_refusals():
    from gm_diffusion.pipelines import StableDiffusionGMPipeline

    pipe = _pipe()
    e = torch.zeros(2, 1, 32)
    with pytest.raises(ValueError, match="Provide either"):
        pipe.check_inputs("p", 64, 64, None, ip_adapter_image=e, ip_adapter_image_embeds=[e])
    with pytest.raises(ValueError, match="has to be of type `list`"):
        pipe.check_inputs("p", 64, 64, None, ip_adapter_image_embeds=e)
    with pytest.raises(ValueError, match="3D or 4D"):
        pipe.check_inputs("p", 64, 64, None, ip_adapter_image_embeds=[torch.zeros(2, 32)])
    pipe.check_inputs("p", 64, 64, None, ip_adapter_image_embeds=[e])
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        pipe._image_prompt_rows(None, [e], "cpu", 1, True)
    pipe.load_ip_adapter(R.make_state_dict(OU.tiny_unet_config(4), 4, 32))
    assert pipe.unet.has_ip_adapter and not pipe.gm_unet.has_ip_adapter
    with pytest.raises(ValueError, match="image_encoder"):  # an image without an encoder
        pipe._image_prompt_rows(torch.zeros(1, 3, 8, 8), None, "cpu", 1, True)
    with pytest.raises(ValueError, match="rows"):  # [negative; positive] of TWO prompts handed to a call with one row: repeated, never broadcast
        pipe._image_prompt_rows(None, [torch.zeros(4, 1, 32)], "cpu", 3, False)
    with pytest.raises(NotImplementedError, match="several"):
        pipe._image_prompt_rows(None, [e, e], "cpu", 1, True)
    with pytest.raises(NotImplementedError, match="Plus"):
        pipe._image_prompt_rows(None, [torch.zeros(2, 1, 5, 32)], "cpu", 1, True)
    with pytest.raises(NotImplementedError, match="Plus"):
        pipe.encode_image(torch.zeros(1, 3, 8, 8), "cpu", 1, output_hidden_states=True)
    with pytest.raises(NotImplementedError):
        pipe.set_ip_adapter_scale([1.0])
    pipe.unload_ip_adapter()
    assert not pipe.unet.has_ip_adapter
    # the single-UNet pipeline keeps refusing, and says where image prompts run
    gm = StableDiffusionGMPipeline.__new__(StableDiffusionGMPipeline)
    with pytest.raises(NotImplementedError, match="StableDiffusionDualUNetPipeline"):
        gm.check_inputs("p", 64, 64, None, ip_adapter_image_embeds=[e])


# ---------------------------------------------------------------------------------------------------------------------------
# prepare_ip_adapter_image_embeds / encode_image against the reference's expressions, transcribed
# ---------------------------------------------------------------------------------------------------------------------------
class _StubEncoder(torch.nn.Module):
    """image_encoder(pixels).image_embeds, duck-typed like transformers' CLIPVisionModelWithProjection."""

    def __init__(self, clip_dim=32):
        super().__init__()
        self.lin = torch.nn.Linear(3, clip_dim)

    def forward(self, pixels):
        return type("Out", (), {"image_embeds": self.lin(pixels.mean((2, 3)))})()


def _reference_prepare(encoder, n_adapters, ip_adapter_image, ip_adapter_image_embeds, device, num_images_per_prompt, do_classifier_free_guidance):
    """stable_diffusion_dual_unet.py:518-585 for plain adapters (ImageProjection layers: output_hidden_state False), expression by
    expression; ``encoder`` stands for self.image_encoder, tensors stand for already-extracted pixel values."""
    def encode_image(image, device, num_images_per_prompt):
        dtype = next(encoder.parameters()).dtype
        image = image.to(device=device, dtype=dtype)
        image_embeds = encoder(image).image_embeds
        image_embeds = image_embeds.repeat_interleave(num_images_per_prompt, dim=0)
        uncond_image_embeds = torch.zeros_like(image_embeds)
        return image_embeds, uncond_image_embeds

    image_embeds = []
    if do_classifier_free_guidance:
        negative_image_embeds = []
    if ip_adapter_image_embeds is None:
        if not isinstance(ip_adapter_image, list):
            ip_adapter_image = [ip_adapter_image]
        if len(ip_adapter_image) != n_adapters:
            raise ValueError("`ip_adapter_image` must have same length as the number of IP Adapters.")
        for single_ip_adapter_image in ip_adapter_image:
            single_image_embeds, single_negative_image_embeds = encode_image(single_ip_adapter_image, device, 1)
            image_embeds.append(single_image_embeds[None, :])
            if do_classifier_free_guidance:
                negative_image_embeds.append(single_negative_image_embeds[None, :])
    else:
        for single_image_embeds in ip_adapter_image_embeds:
            if do_classifier_free_guidance:
                single_negative_image_embeds, single_image_embeds = single_image_embeds.chunk(2)
                negative_image_embeds.append(single_negative_image_embeds)
            image_embeds.append(single_image_embeds)
    ip_adapter_image_embeds = []
    for i, single_image_embeds in enumerate(image_embeds):
        single_image_embeds = torch.cat([single_image_embeds] * num_images_per_prompt, dim=0)
        if do_classifier_free_guidance:
            single_negative_image_embeds = torch.cat([negative_image_embeds[i]] * num_images_per_prompt, dim=0)
            single_image_embeds = torch.cat([single_negative_image_embeds, single_image_embeds], dim=0)
        single_image_embeds = single_image_embeds.to(device=device)
        ip_adapter_image_embeds.append(single_image_embeds)
    return ip_adapter_image_embeds


@pytest.mark.parametrize("do_cfg", [True, False])
@pytest.mark.parametrize("batch,nipp", [(1, 1), (2, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("source", ["embeds", "image", "two_images"])
def test_prepare_ip_adapter_image_embeds_equals_the_reference(do_cfg, batch, nipp, source):
    torch.manual_seed(11)
    enc = _StubEncoder().eval().requires_grad_(False)
    pipe = _pipe(image_encoder=enc)
    pipe.load_ip_adapter(R.make_state_dict(OU.tiny_unet_config(4), 4, 32))
    g = torch.Generator().manual_seed(5)
    rows = batch * nipp  # what __call__ hands over as ``num_images_per_prompt`` (dual.py:991)
    if source == "embeds":
        image, embeds = None, [torch.randn(2 if do_cfg else 1, 3, 32, generator=g)]
    else:
        image, embeds = torch.rand(1 if source == "image" else 2, 3, 8, 8, generator=g), None
    got = pipe.prepare_ip_adapter_image_embeds(image, embeds, "cpu", rows, do_cfg)
    want = _reference_prepare(enc, 1, image, embeds, "cpu", rows, do_cfg)
    assert len(got) == len(want) == 1 and torch.equal(got[0], want[0])
    n_img = 3 if source == "embeds" else image.shape[0]
    assert tuple(got[0].shape) == ((2 if do_cfg else 1) * rows, n_img, 32)
    if do_cfg and source != "embeds":
        assert not bool(got[0][:rows].any()) and bool(got[0][rows:].any())  # zeros are the negative image embedding
    e = pipe._image_prompt_rows(image, embeds, "cpu", rows, do_cfg)
    assert torch.equal(e, want[0])
    # encode_image on its own
    if image is not None:
        a, b = pipe.encode_image(image, "cpu", nipp)
        assert torch.equal(a, enc(image).image_embeds.repeat_interleave(nipp, dim=0)) and torch.equal(b, torch.zeros_like(a))


def test_feature_extractor_is_used_for_non_tensor_images():
    enc = _StubEncoder().eval().requires_grad_(False)
    px = torch.rand(1, 3, 8, 8)
    calls = []

    def extractor(image, return_tensors=None):
        calls.append((image, return_tensors))
        return type("B", (), {"pixel_values": px})()

    pipe = _pipe(image_encoder=enc, feature_extractor=extractor)
    a, _ = pipe.encode_image("a picture", "cpu", 1)
    assert calls == [("a picture", "pt")] and torch.equal(a, enc(px).image_embeds)
    with pytest.raises(ValueError, match="feature_extractor"):
        _pipe(image_encoder=enc).encode_image("a picture", "cpu", 1)


# ---------------------------------------------------------------------------------------------------------------------------
# local files
# ---------------------------------------------------------------------------------------------------------------------------
def test_load_from_safetensors_bin_and_dict(tmp_path):
    from safetensors.torch import save_file

    cfg = OU.tiny_unet_config(4)
    sd = R.make_state_dict(cfg, 4, 32, seed=9)
    flat = {f"{part}.{k}": v.contiguous() for part in sd for k, v in sd[part].items()}
    (tmp_path / "models").mkdir()
    save_file(flat, str(tmp_path / "models" / "ip-adapter.safetensors"))
    torch.save(sd, str(tmp_path / "models" / "ip-adapter.bin"))

    def same(m):
        return (all(torch.equal(m._ip_raw["proj"][k], v) for k, v in sd["image_proj"].items())
                and all(torch.equal(m._ip_raw["kv"][k], v) for k, v in sd["ip_adapter"].items()))

    for args, kw in (((str(tmp_path),), dict(subfolder="models", weight_name="ip-adapter.safetensors")),
                     ((str(tmp_path / "models" / "ip-adapter.safetensors"),), {}),
                     ((str(tmp_path),), dict(subfolder="models", weight_name="ip-adapter.bin")),
                     ((sd,), {})):
        pipe = _pipe()
        pipe.load_ip_adapter(*args, **kw)
        assert same(pipe.unet) and not pipe.gm_unet.has_ip_adapter
    with pytest.raises(FileNotFoundError):
        _pipe().load_ip_adapter(str(tmp_path), subfolder="models", weight_name="absent.safetensors")
    with pytest.raises(ValueError, match="weight_name"):
        _pipe().load_ip_adapter(str(tmp_path))
    with pytest.raises(ValueError, match="image_proj"):
        _pipe().load_ip_adapter({"ip_adapter": sd["ip_adapter"]})
    # a pickle that is not plain tensors is not executed (weights_only=True)
    import pickle

    class Evil:
        def __reduce__(self):
            return (print, ("executed",))

    torch.save({"image_proj": Evil(), "ip_adapter": {}}, str(tmp_path / "evil.bin"))
    with pytest.raises(pickle.UnpicklingError):
        _pipe().load_ip_adapter(str(tmp_path / "evil.bin"))


def test_image_rows_shard_like_the_prompts():
    from gm_diffusion import distributed as gd

    e = torch.arange(8 * 2 * 3, dtype=torch.float32).reshape(8, 2, 3)  # [negative(4); positive(4)]
    got = gd.shard_image_embeds(e, (1, 3), 4, True)
    assert torch.equal(got, torch.cat([e[1:3], e[5:7]]))
    assert torch.equal(gd.shard_image_embeds(e[:4], (1, 3), 4, False), e[1:3])
    with pytest.raises(ValueError):
        gd.shard_image_embeds(e, (0, 2), 4, False)


# ---------------------------------------------------------------------------------------------------------------------------
# the bound of the fused kernel
# ---------------------------------------------------------------------------------------------------------------------------
CASES = [(40, 33, 77, 4), (32, 5, 130, 20), (160, 17, 64, 64), (64, 9, 1, 1), (80, 12, 77, 8)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D,Nq,Nk,Nip", CASES)
@pytest.mark.parametrize("ip_scale", [0.0, 1.0, 0.6, -0.5])
def test_clean_emulation_stays_inside_the_bound(dtype, D, Nq, Nk, Nip, ip_scale):
    q, k, v, kip, vip = R.make_qkv(2, 2, Nq, Nk, Nip, D, dtype, seed=D + Nk)
    scale = D ** -0.5
    ref, bound = R.decoupled_bound(q, k, v, kip, vip, scale, ip_scale, dtype)
    assert torch.equal(ref, R.decoupled_ref(q, k, v, kip, vip, scale, ip_scale))
    got = R.emulate(q, k, v, kip, vip, scale, ip_scale, dtype)
    bad = ((got - ref).abs() > bound) | ~torch.isfinite(got)
    assert int(bad.sum()) == 0, f"{int(bad.sum())} violations of a clean emulation"  # the cap is 0


@pytest.mark.parametrize("image_dominates", [True, False])
def test_branch_independence_inputs_break_a_shared_softmax_state(image_dominates):
    """On inputs where one branch's scores exceed the other's by ~40 at scale, the clean emulation has 0 violations in both types;
    sharing the ROW SUM breaks the bound in both types (the weak branch comes out ~e^-40 of its value); sharing the MAXIMUM breaks it
    in float16, whose P = 2^-58 underflows to zero (0 / 0 or a zero branch).  In bfloat16 a shared maximum at this gap is not a fault
    the arithmetic can show -- bfloat16 has float32's exponent range, P = e^-40 keeps its 8 bits and cancels against its own row sum --
    so the emulation stays inside the bound there, and is asserted to: the bound is not vacuous in the other direction either."""
    D, scale = 40, 40 ** -0.5
    for dtype in (torch.bfloat16, torch.float16):
        q, k, v, kip, vip = R.independence_inputs(2, 2, 33, 77, 4, D, dtype, scale, image_dominates)
        q64 = q.double()
        st, si = q64 @ k.double().transpose(-1, -2) * scale, q64 @ kip.double().transpose(-1, -2) * scale
        gap = float(si.min() - st.max()) if image_dominates else float(st.min() - si.max())
        assert 35.0 < gap < 45.0, gap
        ref, bound = R.decoupled_bound(q, k, v, kip, vip, scale, 0.6, dtype)

        def n_bad(fault):
            got = R.emulate(q, k, v, kip, vip, scale, 0.6, dtype, fault)
            return int((((got - ref).abs() > bound) | ~torch.isfinite(got)).sum())

        assert n_bad(None) == 0
        assert n_bad("shared_sum") > ref.numel() // 2
        if dtype == torch.float16:
            assert n_bad("shared_max") > ref.numel() // 2
        else:
            assert n_bad("shared_max") == 0


def test_composed_and_float32_bounds_hold_for_their_emulations():
    """The bounds of the composed routes (used by the GPU file) against float64 emulations of those routes: every branch stored, then
    a + b * s and one more rounding (16-bit); plain float32 arithmetic (float32)."""
    D, scale = 40, 40 ** -0.5
    for dtype in (torch.bfloat16, torch.float16):
        q, k, v, kip, vip = R.make_qkv(1, 2, 19, 77, 4, D, dtype, seed=2)
        ref, bound = R.composed_bound(q, k, v, kip, vip, scale, 0.6, dtype)
        a = R.emulate(q, k, v, kip, vip, scale, 0.0, dtype)
        b = R.emulate(q, kip, vip, kip, vip, scale, 0.0, dtype)
        got = R._round16(a + 0.6 * b, dtype)
        assert int(((got - ref).abs() > bound).sum()) == 0
    q, k, v, kip, vip = R.make_qkv(1, 2, 19, 77, 4, D, torch.float32, seed=2)
    got = (torch.softmax(q @ k.transpose(-1, -2) * scale, -1) @ v + 0.6 * (torch.softmax(q @ kip.transpose(-1, -2) * scale, -1) @ vip)).double()
    for fn in (R.split_composed_bound, R.exact_composed_bound):
        ref, bound = fn(q, k, v, kip, vip, scale, 0.6)
        assert int(((got - ref).abs() > bound).sum()) == 0 and float(bound.max()) < 1e-3


# ---------------------------------------------------------------------------------------------------------------------------
# the reference UNet
# ---------------------------------------------------------------------------------------------------------------------------
def test_reference_unet_scale_zero_is_the_plain_unet_and_the_image_moves_it():
    from oracle import fixtures

    ou = fixtures.build_unet("tiny", 4)
    cfg = OU.tiny_unet_config(4)
    sd = R.make_state_dict(cfg, 4, 32, seed=4)
    g = torch.Generator().manual_seed(8)
    x, ctx = torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 77, 64, generator=g)
    img = torch.randn(2, 1, 32, generator=g)
    plain = ou(x, torch.tensor(301), encoder_hidden_states=ctx)[0]
    ref0 = R.IPAdapterRef(ou, sd, scale=0.0)
    assert tuple(ref0.set_image_embeds(img).shape) == (2, 4, 64)
    assert torch.allclose(ref0(x, torch.tensor(301), encoder_hidden_states=ctx)[0], plain, atol=1e-6)
    ref1 = R.IPAdapterRef(ou, sd, scale=1.0)
    ref1.set_image_embeds(img)
    y = ref1(x, torch.tensor(301), encoder_hidden_states=ctx)[0]
    assert float((y - plain).abs().max()) > 1e-3
    ref1.set_image_embeds(torch.randn(2, 2, 32, generator=g))  # two images: 8 image tokens
    assert tuple(ref1.ip_tokens.shape) == (2, 8, 64)
    assert torch.equal(ou(x, torch.tensor(301), encoder_hidden_states=ctx)[0], plain)  # the wrapped copy left the original alone
