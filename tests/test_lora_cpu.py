"""CPU: the LoRA loader (gm_diffusion/components/lora.py) -- the three key conventions, alpha / r, kohya's flattened names, every refused
family by name, ignore_unsupported -- and the two CPU references of tests/lora_ref.py against each other on the tiny oracle UNet."""
import functools
import warnings

import pytest
import torch

import lora_ref as R

RANK, GAIN, SEED = 4, 2.0, 11
MODEL_TOL_LOOSEST = 3e-2  # tests/test_models_gpu.py MODEL_TOL[bfloat16]: the loosest gate the GPU tests apply to this UNet


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import fixtures

    return fixtures.build_unet("tiny", 4)


def _hip_model():
    from gm_diffusion.components import UNet2DConditionModel

    ou = _oracle()
    m = UNet2DConditionModel(**vars(ou.config))
    m.load_state_dict(ou.state_dict())
    return m


def _names():
    return _hip_model().lora_module_names()


def _same(p, q):
    assert sorted(p) == sorted(q)
    for k in p:
        assert torch.equal(p[k][0], q[k][0]) and torch.equal(p[k][1], q[k][1]) and p[k][2] == q[k][2], k


def test_the_three_conventions_parse_to_the_same_canonical_dict():
    from gm_diffusion.components.lora import parse_lora_state_dict

    canon = R.canonical(_oracle(), RANK, SEED, GAIN)
    assert len(canon) == 8 * 16  # eight projections in each of the sixteen transformer blocks
    for conv in R.CONVENTIONS:
        _same(parse_lora_state_dict(R.to_convention(canon, conv), _names()), canon)
    # the "unet." prefix is optional
    sd = {k[len("unet."):]: v for k, v in R.to_convention(canon, "peft").items()}
    _same(parse_lora_state_dict(sd, _names()), canon)
    # make_state_dict is the same thing from the config
    from oracle import unet as OU

    _same(parse_lora_state_dict(R.make_state_dict(OU.tiny_unet_config(4), RANK, SEED, GAIN, "kohya"), _names()), canon)


@pytest.mark.parametrize("conv", ["peft", "kohya"])
def test_alpha_over_rank(conv):
    from gm_diffusion.components.lora import factor, parse_lora_state_dict

    canon = R.canonical(_oracle(), 8, SEED, GAIN, alpha=2.0)
    got = parse_lora_state_dict(R.to_convention(canon, conv), _names())
    _same(got, canon)
    assert all(factor(a.shape[0], al) == 0.25 for a, _, al in got.values())
    assert factor(8, None) == 1.0


def test_kohya_names_resolve_through_the_module_table():
    from gm_diffusion.components.lora import parse_lora_state_dict

    name = "up_blocks.1.attentions.2.transformer_blocks.0.attn1.to_out.0"
    a, b = torch.randn(3, 128), torch.randn(128, 3)
    flat = "lora_unet_up_blocks_1_attentions_2_transformer_blocks_0_attn1_to_out_0"
    got = parse_lora_state_dict({f"{flat}.lora_down.weight": a, f"{flat}.lora_up.weight": b, f"{flat}.alpha": torch.tensor(6.0)}, _names())
    assert list(got) == [name] and got[name][2] == 6.0 and torch.equal(got[name][0], a)
    with pytest.raises(NotImplementedError, match="lora_unet_up_blocks_9_attn1_to_q"):
        parse_lora_state_dict({"lora_unet_up_blocks_9_attn1_to_q.lora_down.weight": a, "lora_unet_up_blocks_9_attn1_to_q.lora_up.weight": b},
                              _names())


BLK = "down_blocks.0.attentions.0.transformer_blocks.0"
REFUSED = {
    "ff": (f"unet.{BLK}.ff.net.0.proj", f"{BLK}.ff.net.0.proj"),
    "ff2": (f"unet.{BLK}.ff.net.2", f"{BLK}.ff.net.2"),
    "proj_in": ("unet.down_blocks.0.attentions.0.proj_in", "down_blocks.0.attentions.0.proj_in"),
    "proj_out": ("unet.down_blocks.0.attentions.0.proj_out", "down_blocks.0.attentions.0.proj_out"),
    "resnet_conv": ("unet.down_blocks.0.resnets.0.conv1", "down_blocks.0.resnets.0.conv1"),
    "time_emb_proj": ("unet.down_blocks.0.resnets.0.time_emb_proj", "down_blocks.0.resnets.0.time_emb_proj"),
}


@pytest.mark.parametrize("family", sorted(REFUSED))
def test_refused_targets_raise_and_name_the_module(family):
    from gm_diffusion.components.lora import parse_lora_state_dict

    prefix, name = REFUSED[family]
    sd = {f"{prefix}.lora_A.weight": torch.randn(4, 64), f"{prefix}.lora_B.weight": torch.randn(64, 4)}
    with pytest.raises(NotImplementedError) as e:
        parse_lora_state_dict(sd, _names())
    assert name in str(e.value)


@pytest.mark.parametrize("key", [
    f"lora_unet_{BLK.replace('.', '_')}_attn1_to_q.hada_w1_a", f"lora_unet_{BLK.replace('.', '_')}_attn1_to_q.lokr_w1",
    f"unet.{BLK}.attn1.to_q.dora_scale", f"lora_unet_{BLK.replace('.', '_')}_attn1_to_q.lora_mid.weight",
    "text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_A.weight", "lora_te_text_model_encoder_layers_0_mlp_fc1.lora_down.weight"])
def test_foreign_families_and_text_encoder_keys_raise_by_name(key):
    from gm_diffusion.components.lora import parse_lora_state_dict

    sd = R.to_convention(R.canonical(_oracle(), RANK, SEED, GAIN), "peft")
    sd[key] = torch.randn(4, 4)
    with pytest.raises(NotImplementedError) as e:
        parse_lora_state_dict(sd, _names())
    assert key.split(".lora")[0].rsplit(".hada", 1)[0].rsplit(".lokr", 1)[0].rsplit(".dora", 1)[0] in str(e.value)


def test_rank_above_128_and_a_second_adapter_are_refused():
    from gm_diffusion.components.lora import parse_lora_state_dict

    name = f"{BLK}.attn1.to_q"
    sd = {f"unet.{name}.lora_A.weight": torch.randn(129, 64), f"unet.{name}.lora_B.weight": torch.randn(64, 129)}
    with pytest.raises(NotImplementedError, match="rank 129"):
        parse_lora_state_dict(sd, _names())
    m = _hip_model()
    good = R.to_convention(R.canonical(_oracle(), RANK, SEED, GAIN), "peft")
    m.load_lora(good)
    assert m.has_lora
    with pytest.raises(NotImplementedError, match="already loaded"):
        m.load_lora(good)
    m.unload_lora()
    assert not m.has_lora
    m.load_lora(good)
    with pytest.raises(ValueError):  # a factor that does not fit the projection
        _hip_model().load_lora({f"unet.{name}.lora_A.weight": torch.randn(4, 32), f"unet.{name}.lora_B.weight": torch.randn(64, 4)})


def test_rank_zero_and_stray_keys_are_named_for_what_they_are():
    from gm_diffusion import hip_ops as ops
    from gm_diffusion.components import lora
    from gm_diffusion.components.lora import parse_lora_state_dict

    assert lora.MAX_RANK == ops.LORA_MAX_RANK == 128  # one number: the kernel's limit
    name = f"{BLK}.attn1.to_q"
    with pytest.raises(NotImplementedError, match=r"rank 0 outside \[1, 128\]"):
        parse_lora_state_dict({f"unet.{name}.lora_A.weight": torch.zeros(0, 64), f"unet.{name}.lora_B.weight": torch.zeros(64, 0)}, _names())
    sd = R.to_convention(R.canonical(_oracle(), RANK, SEED, GAIN), "peft")
    sd["ss_training_comment"] = torch.zeros(1)
    with pytest.raises(NotImplementedError, match="ss_training_comment: not a LoRA tensor"):
        parse_lora_state_dict(sd, _names())


def test_ignore_unsupported_skips_and_warns_once():
    from gm_diffusion.components.lora import parse_lora_state_dict

    canon = R.canonical(_oracle(), RANK, SEED, GAIN)
    sd = R.to_convention(canon, "peft")
    for fam in ("ff", "proj_in", "time_emb_proj"):
        sd[f"{REFUSED[fam][0]}.lora_A.weight"], sd[f"{REFUSED[fam][0]}.lora_B.weight"] = torch.randn(4, 64), torch.randn(64, 4)
    sd["text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_A.weight"] = torch.randn(4, 4)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = parse_lora_state_dict(sd, _names(), ignore_unsupported=True)
    assert len(w) == 1
    for fam in ("ff", "proj_in", "time_emb_proj"):
        assert REFUSED[fam][1] in str(w[0].message)
    _same(got, canon)
    with warnings.catch_warnings(record=True) as w:  # the model's loader passes the switch on
        warnings.simplefilter("always")
        m = _hip_model().load_lora(sd, ignore_unsupported=True)
    assert len(w) == 1 and m.has_lora


@functools.lru_cache(maxsize=None)
def _case():
    g = torch.Generator().manual_seed(61)
    lat, ctx = torch.randn(1, 4, 16, 16, generator=g), torch.randn(2, 77, 64, generator=g)
    return torch.cat([lat, lat]), ctx


def test_the_two_references_agree_and_the_adapter_moves_the_output():
    ou = _oracle()
    x, ctx = _case()
    canon = R.canonical(ou, RANK, SEED, GAIN, alpha=2.0)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    with torch.no_grad():
        plain = ou(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
        for s in (1.0, 0.5):
            merged = R.merged_oracle(ou, canon, s)(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
            hooked = R.hooked_oracle(ou, canon, s)(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
            e = rel(hooked, merged)
            print(f"scale {s}: merged vs hooked {e:.3e}; adapter moves the output by {rel(merged, plain):.3f}")
            assert e < 2e-5  # float32 round-off through the whole UNet (the gate of a float32 model against its oracle)
            # the condition the GPU tests rely on, for the reference alone: far more than 10 x the loosest model tolerance
            assert rel(merged, plain) > 10 * MODEL_TOL_LOOSEST
        zero = R.merged_oracle(ou, canon, 0.0)(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
        assert torch.equal(zero, plain)


def test_update_bound_holds_for_a_clean_emulation_and_catches_a_dropped_k_step():
    """The derived bound of the kernel against a CPU emulation of its arithmetic (float32 accumulation, ONE rounding of T, one of the
    store): zero violations.  An emulation that loses one K step of the first product must break it."""
    import parity as P

    g = torch.Generator().manual_seed(3)
    for dtype in (torch.bfloat16, torch.float16):
        x, a = torch.randn(161, 128, generator=g).to(dtype), (torch.randn(32, 128, generator=g) / 11).to(dtype)
        b, y = torch.randn(200, 32, generator=g).to(dtype), torch.randn(161, 200, generator=g).to(dtype)
        a[8:], b[:, 8:] = 0, 0
        s = float(torch.tensor(0.7, dtype=torch.float32))
        that = (x.float() @ a.float().T).to(dtype)
        u = that.float() @ b.float().T
        got = (y.float() + s * u).to(dtype)
        ref, bound = R.update_ref_bound(x, a, b, y, s, dtype)
        P.assert_elementwise(got, ref, bound, f"emulation {dtype}")
        # teeth: the same emulation with the second K step of the first product dropped breaks it
        bad = (y.float() + s * ((x[:, :64].float() @ a[:, :64].float().T).to(dtype).float() @ b.float().T)).to(dtype)
        assert int(P.violations(bad, ref, bound)[0].sum()) > ref.numel() // 4


def test_hip_ops_lora_update_refuses_host_tensors():
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import HipExtensionError

    x, a, b, y = torch.zeros(8, 64), torch.zeros(32, 64), torch.zeros(64, 32), torch.zeros(8, 64)
    with pytest.raises(HipExtensionError):
        ops.lora_update(x, a, b, y, torch.ones(1), 0)


def test_load_lora_weights_on_a_missing_path_raises_file_not_found(tmp_path):
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline
    from gm_diffusion.components import PNDMScheduler

    pipe = StableDiffusionDualUNetPipeline(vae=None, text_encoder=None, tokenizer=None, unet=_hip_model(), gm_unet=_hip_model(),
                                           scheduler=PNDMScheduler(), safety_checker=None, feature_extractor=None,
                                           requires_safety_checker=False)
    with pytest.raises(FileNotFoundError):
        pipe.load_lora_weights(str(tmp_path / "nothing.safetensors"))
    with pytest.raises(FileNotFoundError):
        pipe.load_lora_weights(str(tmp_path), weight_name="nothing.bin")
    for call in (lambda: pipe.fuse_lora(), lambda: pipe.set_adapters(["a"]), lambda: pipe.load_lora_weights({}, adapter_name="a")):
        with pytest.raises(NotImplementedError):
            call()
    # a local torch pickle loads through the pipeline into the SDR UNet only
    sd = R.to_convention(R.canonical(_oracle(), RANK, SEED, GAIN), "kohya")
    torch.save(sd, tmp_path / "pytorch_lora_weights.bin")
    pipe.load_lora_weights(str(tmp_path))
    assert pipe.unet.has_lora and not pipe.gm_unet.has_lora
    pipe.unload_lora_weights()
    assert not pipe.unet.has_lora
