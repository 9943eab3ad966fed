"""CPU: the opt-in wider LoRA target set (``targets="transformer"``: ff.net.0.proj, ff.net.2, proj_in, proj_out beside the eight
attention projections) in the loader, the defaults that stay as they were, the two CPU references of tests/lora_ff_ref.py against
each other, and the value / gate interleave the device side applies to ff.net.0.proj's up factor."""
import functools
import warnings

import pytest
import torch

import lora_ff_ref as FR
import lora_ref as R

RANK, GAIN, SEED = 4, 2.0, 11
MODEL_TOL_LOOSEST = 3e-2  # tests/test_models_gpu.py MODEL_TOL[bfloat16]: the loosest gate the GPU tests apply to this UNet
BLK = "down_blocks.0.attentions.0.transformer_blocks.0"
TRF = "down_blocks.0.attentions.0"
NEW = {"ff1": f"{BLK}.ff.net.0.proj", "ff2": f"{BLK}.ff.net.2", "proj_in": f"{TRF}.proj_in", "proj_out": f"{TRF}.proj_out"}
SHAPE = {"ff1": (512, 64), "ff2": (64, 256), "proj_in": (64, 64), "proj_out": (64, 64)}  # [N, K] at the tiny UNet's first level


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


@functools.lru_cache(maxsize=None)
def _names():
    return tuple(_hip_model().lora_module_names())


def _same(p, q):
    assert sorted(p) == sorted(q)
    for k in p:
        assert torch.equal(p[k][0], q[k][0]) and torch.equal(p[k][1], q[k][1]) and p[k][2] == q[k][2], k


def test_the_twelve_targets_parse_in_every_convention_to_the_canonical_factors():
    from gm_diffusion.components.lora import parse_lora_state_dict

    ou = _oracle()
    canon = FR.canonical(ou, RANK, SEED, GAIN)
    assert len(canon) == 12 * 16  # twelve targets in each of the sixteen Transformer2DModels (one block each)
    convs = FR.conv_targets(ou)
    assert len(convs) == 2 * 16  # SD-1.5 flavour: proj_in / proj_out are 1x1 convolutions
    for conv in FR.CONVENTIONS:
        sd = FR.to_convention(canon, conv, conv_names=convs)
        if conv == "kohya":  # 4-D factors of the convolutions, squeezed by the loader
            flat = "lora_unet_" + NEW["proj_in"].replace(".", "_")
            assert sd[f"{flat}.lora_down.weight"].shape == (RANK, 64, 1, 1) and sd[f"{flat}.lora_up.weight"].shape == (64, RANK, 1, 1)
        got = parse_lora_state_dict(sd, _names(), targets="transformer")
        _same(got, canon)
        assert all(a.dim() == 2 and b.dim() == 2 for a, b, _ in got.values())
    # alpha / r, peft and kohya
    canon_a = FR.canonical(ou, 8, SEED, GAIN, alpha=2.0)
    for conv in ("peft", "kohya"):
        _same(parse_lora_state_dict(FR.to_convention(canon_a, conv, conv_names=convs), _names(), targets="transformer"), canon_a)
    # the attention-only adapter parses alike under both settings
    att = R.canonical(ou, RANK, SEED, GAIN)
    _same(parse_lora_state_dict(R.to_convention(att, "diffusers_processor"), _names(), targets="transformer"), att)
    # ff.net.0.proj's up factor arrives in checkpoint row order: [8C, r] at C = 64
    assert canon[NEW["ff1"]][1].shape == (512, RANK) and canon[NEW["ff2"]][0].shape == (RANK, 256)


@pytest.mark.parametrize("family", sorted(NEW))
def test_the_default_still_refuses_the_four_families_and_names_them(family):
    from gm_diffusion.components.lora import parse_lora_state_dict

    n, k = SHAPE[family]
    sd = {f"unet.{NEW[family]}.lora_A.weight": torch.randn(4, k), f"unet.{NEW[family]}.lora_B.weight": torch.randn(n, 4)}
    for kw in ({}, {"targets": "attention"}):
        with pytest.raises(NotImplementedError) as e:
            parse_lora_state_dict(sd, _names(), **kw)
        assert NEW[family] in str(e.value) and "targets='transformer'" in str(e.value)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert parse_lora_state_dict(sd, _names(), ignore_unsupported=True) == {}
    assert len(w) == 1 and NEW[family] in str(w[0].message)
    got = parse_lora_state_dict(sd, _names(), targets="transformer")
    assert list(got) == [NEW[family]]


@pytest.mark.parametrize("prefix,name", [
    ("unet.down_blocks.0.resnets.0.conv1", "down_blocks.0.resnets.0.conv1"),
    ("unet.down_blocks.0.resnets.0.time_emb_proj", "down_blocks.0.resnets.0.time_emb_proj"),
    ("unet.down_blocks.0.resnets.0.conv_shortcut", "down_blocks.0.resnets.0.conv_shortcut"),
    ("unet.conv_in", "conv_in"),
])
def test_resnet_and_convolution_targets_are_refused_under_both_settings(prefix, name):
    from gm_diffusion.components.lora import parse_lora_state_dict

    sd = {f"{prefix}.lora_A.weight": torch.randn(4, 64), f"{prefix}.lora_B.weight": torch.randn(64, 4)}
    for targets in ("attention", "transformer"):
        with pytest.raises(NotImplementedError) as e:
            parse_lora_state_dict(sd, _names(), targets=targets)
        assert name in str(e.value) and "targets='transformer'" not in str(e.value)


@pytest.mark.parametrize("key", [
    "text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_A.weight", "lora_te_text_model_encoder_layers_0_mlp_fc1.lora_down.weight",
    f"lora_unet_{BLK.replace('.', '_')}_ff_net_0_proj.hada_w1_a", f"lora_unet_{BLK.replace('.', '_')}_ff_net_2.lokr_w1",
    f"unet.{TRF}.proj_in.dora_scale"])
def test_text_encoder_and_foreign_families_are_refused_under_transformer(key):
    from gm_diffusion.components.lora import parse_lora_state_dict

    sd = FR.to_convention(FR.canonical(_oracle(), RANK, SEED, GAIN), "peft")
    sd[key] = torch.randn(4, 4)
    with pytest.raises(NotImplementedError) as e:
        parse_lora_state_dict(sd, _names(), targets="transformer")
    assert key.split(".lora")[0].rsplit(".hada", 1)[0].rsplit(".lokr", 1)[0].rsplit(".dora", 1)[0] in str(e.value)


def test_a_3x3_factor_a_rank_above_128_and_a_second_adapter_are_refused():
    from gm_diffusion.components.lora import parse_lora_state_dict

    flat = "lora_unet_" + NEW["proj_in"].replace(".", "_")
    sd = {f"{flat}.lora_down.weight": torch.randn(4, 64, 3, 3), f"{flat}.lora_up.weight": torch.randn(64, 4, 1, 1)}
    with pytest.raises(NotImplementedError, match="convolution LoRA") as e:
        parse_lora_state_dict(sd, _names(), targets="transformer")
    assert NEW["proj_in"] in str(e.value)
    # 4-D factors on a module that is no 1x1 convolution of a transformer stay convolution LoRA too
    sd = {f"unet.{NEW['ff2']}.lora_A.weight": torch.randn(4, 256, 1, 1), f"unet.{NEW['ff2']}.lora_B.weight": torch.randn(64, 4, 1, 1)}
    with pytest.raises(NotImplementedError, match="convolution LoRA"):
        parse_lora_state_dict(sd, _names(), targets="transformer")
    sd = {f"unet.{NEW['ff2']}.lora_A.weight": torch.randn(129, 256), f"unet.{NEW['ff2']}.lora_B.weight": torch.randn(64, 129)}
    with pytest.raises(NotImplementedError, match="rank 129"):
        parse_lora_state_dict(sd, _names(), targets="transformer")
    m = _hip_model()
    full = FR.to_convention(FR.canonical(_oracle(), RANK, SEED, GAIN), "peft")
    m.load_lora(full, targets="transformer")
    with pytest.raises(NotImplementedError, match="already loaded"):
        m.load_lora(full, targets="transformer")


def test_a_bad_targets_value_is_a_value_error_everywhere():
    from gm_diffusion.components.lora import parse_lora_state_dict, supported

    sd = R.to_convention(R.canonical(_oracle(), RANK, SEED, GAIN), "peft")
    for bad in ("all", "Transformer", None, ""):
        with pytest.raises(ValueError, match="targets"):
            parse_lora_state_dict(sd, _names(), targets=bad)
        with pytest.raises(ValueError, match="targets"):
            _hip_model().load_lora(sd, targets=bad)
        with pytest.raises(ValueError, match="targets"):
            supported(NEW["ff1"], bad)
    assert supported(NEW["ff1"], "transformer") and not supported(NEW["ff1"]) and supported(f"{BLK}.attn1.to_q")
    assert supported(NEW["proj_out"], "transformer") and not supported("down_blocks.0.resnets.0.proj_in", "transformer")


def test_load_lora_checks_the_shapes_of_the_new_projections():
    m = _hip_model()
    canon = FR.canonical(_oracle(), RANK, SEED, GAIN)
    with pytest.raises(NotImplementedError, match=r"ff\.net\.0\.proj"):  # the default of load_lora is the default of the loader
        m.load_lora(FR.to_convention(canon, "peft"))
    assert not m.has_lora
    for fam, shape in (("ff1", (256, 64)), ("ff2", (64, 64)), ("proj_in", (128, 64)), ("proj_out", (64, 128))):
        n, k = shape
        bad = dict(canon)
        bad[NEW[fam]] = (torch.randn(RANK, k), torch.randn(n, RANK), None)
        with pytest.raises(ValueError, match=NEW[fam].replace(".", r"\.")):
            m.load_lora(FR.to_convention(bad, "peft"), targets="transformer")
        assert not m.has_lora
    m.load_lora(FR.to_convention(canon, "kohya", conv_names=FR.conv_targets(_oracle())), targets="transformer")
    assert m.has_lora and len(m._lora_raw) == 12 * 16
    m.unload_lora()
    assert not m.has_lora


def test_the_pipelines_pass_targets_through():
    import inspect

    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline, StableDiffusionGMPipeline

    for cls in (StableDiffusionDualUNetPipeline, StableDiffusionGMPipeline):
        assert inspect.signature(cls.load_lora_weights).parameters["targets"].default == "attention"
    from gm_diffusion.components import UNet2DConditionModel
    from gm_diffusion.components.lora import parse_lora_state_dict

    assert inspect.signature(UNet2DConditionModel.load_lora).parameters["targets"].default == "attention"
    assert inspect.signature(parse_lora_state_dict).parameters["targets"].default == "attention"


@functools.lru_cache(maxsize=None)
def _oracle_case():
    ou = _oracle()
    g = torch.Generator().manual_seed(5)
    x, ctx = torch.randn(2, 4, 16, 16, generator=g), torch.randn(2, 77, 64, generator=g)
    with torch.no_grad():
        base = ou(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
    return x, ctx, base


@pytest.mark.parametrize("families", [None, ("ff2",), ("proj_out",), ("ff1", "proj_in")])
def test_merged_and_hooked_oracles_agree(families):
    ou = _oracle()
    x, ctx, base = _oracle_case()
    canon = FR.canonical(ou, RANK, SEED, GAIN, alpha=2.0, families=families)
    assert len(canon) == 16 * sum(len(FR.FAMILIES[f]) for f in (families or FR.FAMILIES))
    with torch.no_grad():
        for scale in (1.0, 0.5):
            a = FR.merged_oracle(ou, canon, scale)(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
            b = FR.hooked_oracle(ou, canon, scale)(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
            rel = float((a - b).norm() / b.norm())
            moved = float((a - base).norm() / base.norm())
            assert rel < 1e-5, rel
            assert moved > 10 * MODEL_TOL_LOOSEST * (0.1 if families else 1.0), (families, scale, moved)


def test_the_wider_adapter_moves_the_output_beyond_the_attention_only_one():
    ou = _oracle()
    x, ctx, base = _oracle_case()
    full = FR.canonical(ou, RANK, SEED, GAIN)
    att = {k: v for k, v in full.items() if k.endswith(R.PROJECTIONS)}
    with torch.no_grad():
        a = FR.merged_oracle(ou, full)(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
        b = R.merged_oracle(ou, att)(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
    assert float((a - b).norm() / b.norm()) > 10 * MODEL_TOL_LOOSEST  # a thinner adapter is another model


def test_the_interleave_is_undone_by_a_halves_layout_geglu():
    """geglu over the de-interleaved columns of x W_i^T equals diffusers' GEGLU over the halves of x W^T, bit for bit in float64; the
    permutation hip_ops applies to the adapter's up factor is the one the UNet applies to the ff1 weight, and applying the inverse
    index restores checkpoint order."""
    from gm_diffusion import hip_ops as ops

    g = torch.Generator().manual_seed(3)
    for C in (16, 64, 320):
        w = torch.randn(8 * C, C, generator=g, dtype=torch.float64)
        x = torch.randn(5, C, generator=g, dtype=torch.float64)
        wi = FR.interleave_rows(w)
        assert torch.equal(ops.geglu_interleave(w), wi) and torch.equal(ops.geglu_interleave(w[:, 0]), wi[:, 0])
        v, gate = FR.deinterleave_cols(x @ wi.T)
        assert torch.equal(v * torch.nn.functional.gelu(gate), FR.geglu_halves(x @ w.T))
        perm = FR.interleave_rows(torch.arange(8 * C))
        assert torch.equal(perm[:16], torch.arange(16)) and torch.equal(perm[16:32], torch.arange(16) + 4 * C)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(8 * C)
        assert torch.equal(wi[inv], w) and sorted(perm.tolist()) == list(range(8 * C))
    from gm_diffusion._native import HipExtensionError

    with pytest.raises(HipExtensionError):
        ops.geglu_interleave(torch.zeros(24, 4))


def test_ensure_lora_layout_matches_the_model_s_ff1_weight():
    """Host side of _ensure_lora, restated on the raw tensors: in the 16-bit modes the block's ff1 weight is interleave_rows of the
    checkpoint's, so the up factor must be too -- (W + B A) interleaved == W interleaved + (B interleaved) A."""
    ou = _oracle()
    canon = FR.canonical(ou, RANK, SEED, GAIN)
    name = NEW["ff1"]
    a, b, _ = canon[name]
    w = dict(ou.named_modules())[name].weight.detach().double()
    assert torch.equal(FR.interleave_rows(w + b.double() @ a.double()), FR.interleave_rows(w) + FR.interleave_rows(b).double() @ a.double())
