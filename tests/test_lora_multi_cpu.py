"""CPU: several LoRA adapters at once -- the host-side packing (column ranges, zero padding, the two scale tables, the 256 limit),
names and refusals of UNet2DConditionModel / the pipelines, the one-adapter invariant at host level, the merged and hooked
references for a weighted set of adapters, and the stacked launch's bound against a torch emulation of its contract."""
import functools

import pytest
import torch

import lora_ff_ref as FR
import lora_multi_ref as MR
import lora_ref as R
import parity as P

GAIN = 1.0  # two adapters on top of each other: at gain 2 the perturbed tiny UNet amplifies float32 round-off past the 2e-5 gate


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


def _adapter(rank, seed, alpha=None, families=("attention",)):
    """(canonical dict, state dict) of an adapter on ``families`` of the tiny UNet."""
    canon = FR.canonical(_oracle(), rank, seed, GAIN, alpha=alpha, families=families)
    return canon, FR.to_convention(canon, "peft")


def _fake(rank, modules, alpha, seed, K=64, N=96):
    g = torch.Generator().manual_seed(seed)
    return {m: (torch.randn(rank, K, generator=g), torch.randn(N, rank, generator=g), alpha) for m in modules}


# ---------------------------------------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------------------------------------
def test_packing_ranges_padding_tables_and_the_limit():
    from gm_diffusion import hip_ops as ops
    from gm_diffusion.components import lora

    assert ops.LORA_MAX_STACKED_RANK == 256 and ops.LORA_MAX_RANK == 128
    # load order: "style" (rank 3, alpha 6), "subject" (rank 5, no alpha), "detail" (rank 8, alpha 4) on overlapping, unequal sets
    adapters = {"style": _fake(3, ["m.a", "m.b", "m.d"], 6.0, 1), "subject": _fake(5, ["m.b", "m.c"], None, 2),
                "detail": _fake(8, ["m.b", "m.d", "m.e"], 4.0, 3)}
    pk = lora.pack_adapters(adapters)
    assert list(pk.modules) == ["m.a", "m.b", "m.c", "m.d", "m.e"]
    got = {m: (mp.adapters, mp.ranks, mp.ranges, mp.rank, mp.padded, mp.row, mp.slots) for m, mp in pk.modules.items()}
    assert got["m.a"] == (["style"], [3], [(0, 3)], 3, 32, None, [0])
    assert got["m.b"] == (["style", "subject", "detail"], [3, 5, 8], [(0, 3), (3, 8), (8, 16)], 16, 32, 0, [1, 2, 3])
    assert got["m.c"] == (["subject"], [5], [(0, 5)], 5, 32, None, [4])
    assert got["m.d"] == (["style", "detail"], [3, 8], [(0, 3), (3, 11)], 11, 32, 1, [5, 6])
    assert got["m.e"] == (["detail"], [8], [(0, 8)], 8, 32, None, [7])
    assert pk.slots == [("m.a", "style"), ("m.b", "style"), ("m.b", "subject"), ("m.b", "detail"), ("m.c", "subject"), ("m.d", "style"),
                        ("m.d", "detail"), ("m.e", "detail")]
    assert (pk.rows, pk.width) == (2, 32)
    assert [mp.stacked for mp in pk.modules.values()] == [False, True, False, True, False]
    # the stack: tight, in load order, zeros beyond the sum
    a, b = lora.stack_factors(adapters, "m.b", pk.modules["m.b"])
    assert a.shape == (32, 64) and b.shape == (96, 32)
    for n, (c0, c1) in zip(("style", "subject", "detail"), ((0, 3), (3, 8), (8, 16))):
        assert torch.equal(a[c0:c1], adapters[n]["m.b"][0]) and torch.equal(b[:, c0:c1], adapters[n]["m.b"][1])
    assert not a[16:].any() and not b[:, 16:].any()
    # tables: s * w_a * alpha_a / r_a; "subject" is not named: weight 0
    scalars, columns = lora.scale_tables(adapters, pk, {"style": 0.8, "detail": -0.5}, scale=0.7)
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    style, detail = f32(f32(6.0 / 3) * f32(0.7 * 0.8)), f32(f32(4.0 / 8) * f32(0.7 * -0.5))
    assert scalars.dtype == columns.dtype == torch.float32
    assert scalars.tolist() == [style, style, 0.0, detail, 0.0, style, detail, detail]
    assert columns.shape == (2, 32)
    assert columns[0].tolist() == [style] * 3 + [0.0] * 5 + [detail] * 8 + [0.0] * 16
    assert columns[1].tolist() == [style] * 3 + [detail] * 8 + [0.0] * 21
    assert abs(style - 0.7 * 0.8 * 2.0) < 1e-6 and abs(detail + 0.7 * 0.5 * 0.5) < 1e-6
    # a multiple-of-32 sum is not padded further; 33 columns take 64
    two = lora.pack_adapters({"a": _fake(16, ["m"], None, 4), "b": _fake(16, ["m"], None, 5)})
    assert two.modules["m"].padded == 32
    assert lora.pack_adapters({"a": _fake(16, ["m"], None, 4), "b": _fake(17, ["m"], None, 5)}).modules["m"].padded == 64
    assert lora.pack_adapters({"a": _fake(128, ["m"], None, 4), "b": _fake(128, ["m"], None, 5)}).modules["m"].padded == 256
    # no stacked module at all: a [1, 1] table of zeros keeps the launches' pointer argument valid
    one = lora.pack_adapters({"a": _fake(4, ["m", "n"], 2.0, 6)})
    s1, c1 = lora.scale_tables({"a": _fake(4, ["m", "n"], 2.0, 6)}, one, {"a": 1.0}, 0.5)
    assert (one.rows, one.width) == (0, 0) and c1.shape == (1, 1) and s1.tolist() == [0.25, 0.25]
    # the limit: 128 + 128 + 1 pads to 288 > 256
    big = {"a": _fake(128, ["m.x", "m.y"], None, 7), "b": _fake(128, ["m.y"], None, 8), "c": _fake(1, ["m.y", "m.x"], None, 9)}
    with pytest.raises(NotImplementedError) as e:
        lora.pack_adapters(big)
    msg = str(e.value)
    assert "m.y" in msg and "128 + 128 + 1" in msg and "288" in msg and "256" in msg and "m.x" not in msg


def test_the_model_refuses_a_stack_above_256_and_stays_as_it_was():
    m = _hip_model()
    name = "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q"

    def sd(rank, seed):
        g = torch.Generator().manual_seed(seed)
        return {f"unet.{name}.lora_A.weight": torch.randn(rank, 64, generator=g), f"unet.{name}.lora_B.weight": torch.randn(64, rank, generator=g)}

    m.load_lora(sd(128, 1), adapter_name="a").load_lora(sd(128, 2), adapter_name="b")
    before = (m.list_adapters(), dict(m._lora_weights), m._lora_id, m._lora_version, m._lora_raw)
    with pytest.raises(NotImplementedError, match=r"attn1\.to_q.*128 \+ 128 \+ 1.*256"):
        m.load_lora(sd(1, 3), adapter_name="c")
    assert (m.list_adapters(), dict(m._lora_weights), m._lora_id, m._lora_version, m._lora_raw) == before
    assert m._lora_raw is before[4] and m.list_adapters() == ["a", "b"]


# ---------------------------------------------------------------------------------------------------------------------------
# names and refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_names_weights_and_refusals_on_the_model():
    m = _hip_model()
    (_, sa), (_, sb), (_, sc) = _adapter(4, 11), _adapter(8, 12, families=None), _adapter(2, 13)
    m.load_lora(sa)
    m.load_lora(sb, targets="transformer")
    assert m.list_adapters() == ["default_0", "default_1"] == m.active_adapters()
    m.load_lora(sc, adapter_name="style")
    assert m.list_adapters() == ["default_0", "default_1", "style"] and m._lora_weights == {"default_0": 1.0, "default_1": 1.0, "style": 1.0}
    with pytest.raises(ValueError, match="already loaded"):
        m.load_lora(sc, adapter_name="style")
    with pytest.raises(ValueError, match="already loaded"):
        m.load_lora(sc, adapter_name="default_1")
    with pytest.raises(NotImplementedError, match=r"ff\.net"):  # targets= is per adapter: the default refuses the wider set
        m.load_lora(sb, adapter_name="wide")
    assert "wide" not in m.list_adapters()
    # the SAME adapter a second time, under whatever name or key convention, is refused as already loaded: it would double its effect
    for again in (lambda: m.load_lora(sa), lambda: m.load_lora(FR.to_convention(_adapter(4, 11)[0], "kohya"), adapter_name="copy")):
        with pytest.raises(ValueError, match="already loaded as 'default_0'") as e:
            again()
        assert isinstance(e.value, NotImplementedError)  # what a second load raised while one adapter was all there was
    assert m.list_adapters() == ["default_0", "default_1", "style"]
    m.delete_adapters("default_0")
    m.load_lora(sa)  # diffusers' default name: the first free default_<n>
    assert m.list_adapters() == ["default_1", "style", "default_2"]
    v = m._lora_version
    m.set_adapters(["style", "default_1"], [0.8, -0.5])
    assert m._lora_weights == {"default_1": -0.5, "style": 0.8, "default_2": 0.0} and m.active_adapters() == ["default_1", "style"]
    assert m._lora_version == v + 1
    m.set_adapters("default_2")
    assert m._lora_weights == {"default_1": 0.0, "style": 0.0, "default_2": 1.0} and m.active_adapters() == ["default_2"]
    m.set_adapters(["style"], 0.25)
    assert m._lora_weights["style"] == 0.25
    for bad in (["nope"], "nope", ["style", "nope"]):
        with pytest.raises(ValueError, match="nope") as e:
            m.set_adapters(bad)
        assert isinstance(e.value, NotImplementedError)  # lora.LoraAdapterError is both
        with pytest.raises(ValueError, match="nope"):
            m.delete_adapters(bad)
    with pytest.raises(ValueError):
        m.set_adapters(["style", "default_1"], [1.0])
    with pytest.raises(NotImplementedError, match="per-block"):
        m.set_adapters(["style"], [{"down": 1.0, "mid": 0.5, "up": 1.0}])
    with pytest.raises(NotImplementedError, match="per-block"):
        m.set_adapters("style", {"down": 1.0})
    assert m._lora_weights == {"default_1": 0.0, "style": 0.25, "default_2": 0.0}  # a refused call changes nothing
    # disable / enable remember the weights; set_lora_scale stays the global factor
    m.set_lora_scale(0.7)
    m.disable_lora()
    assert m.active_adapters() == [] and m.has_lora and m._lora_scale == 0.7
    m.disable_lora()  # twice: the first memory is kept
    m.enable_lora()
    assert m._lora_weights == {"default_1": 0.0, "style": 0.25, "default_2": 0.0}
    m.enable_lora()  # nothing to restore: no change
    assert m._lora_weights["style"] == 0.25
    m.unload_lora()
    assert not m.has_lora and m.list_adapters() == [] and m._lora_scale == 1.0
    for call in (m.disable_lora, m.enable_lora, lambda: m.set_lora_scale(1.0)):
        with pytest.raises(ValueError, match="no LoRA adapter"):
            call()


def test_pipeline_names_and_refusals():
    from gm_diffusion.components import PNDMScheduler
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline

    pipe = StableDiffusionDualUNetPipeline(vae=None, text_encoder=None, tokenizer=None, unet=_hip_model(), gm_unet=_hip_model(),
                                           scheduler=PNDMScheduler(steps_offset=1), safety_checker=None, feature_extractor=None,
                                           requires_safety_checker=False)
    (_, sa), (_, sb) = _adapter(4, 11), _adapter(8, 12, families=None)
    assert pipe.get_list_adapters() == {"unet": []} and pipe.get_active_adapters() == []
    pipe.load_lora_weights(sa, adapter_name="style")
    pipe.load_lora_weights(sb, adapter_name="subject", targets="transformer")
    assert pipe.get_list_adapters() == {"unet": ["style", "subject"]} and not pipe.gm_unet.has_lora
    pipe.gm_unet.load_lora(sa, adapter_name="gm_look")
    assert pipe.get_list_adapters() == {"unet": ["style", "subject"], "gm_unet": ["gm_look"]}
    pipe.set_adapters(["style", "subject"], adapter_weights=[0.8, 0.5])
    assert pipe.unet._lora_weights == {"style": 0.8, "subject": 0.5}
    assert pipe.gm_unet._lora_weights == {"gm_look": 0.0}  # addressed with none of ITS names: all of them unnamed
    pipe.set_adapters(["gm_look", "subject"], [0.3, 0.6])  # each UNet for the names it has loaded
    assert pipe.unet._lora_weights == {"style": 0.0, "subject": 0.6} and pipe.gm_unet._lora_weights == {"gm_look": 0.3}
    assert pipe.get_active_adapters() == ["subject", "gm_look"]
    with pytest.raises(ValueError, match="nope"):
        pipe.set_adapters(["style", "nope"])
    with pytest.raises(ValueError, match="nope"):
        pipe.delete_adapters("nope")
    with pytest.raises(NotImplementedError, match="per-block"):
        pipe.set_adapters(["style"], [{"down": 1.0}])
    for refused in (pipe.fuse_lora, pipe.unfuse_lora):
        with pytest.raises(NotImplementedError, match="fuse_lora"):
            refused()
    pipe.disable_lora()
    assert pipe.get_active_adapters() == []
    pipe.enable_lora()
    assert pipe.get_active_adapters() == ["subject", "gm_look"]
    pipe.delete_adapters(["subject"])
    assert pipe.get_list_adapters() == {"unet": ["style"], "gm_unet": ["gm_look"]}
    pipe.unload_lora_weights()  # all adapters of the SDR UNet; the GM UNet's own stays
    assert pipe.get_list_adapters() == {"unet": [], "gm_unet": ["gm_look"]}


# ---------------------------------------------------------------------------------------------------------------------------
# the one-adapter invariant, host level
# ---------------------------------------------------------------------------------------------------------------------------
def _host_state(m):
    from gm_diffusion.components import lora

    pk = lora.pack_adapters(m._lora_adapters)
    scalars, columns = lora.scale_tables(m._lora_adapters, pk, m._lora_weights, m._lora_scale)
    return dict(names=m.list_adapters(), weights=dict(m._lora_weights), scale=m._lora_scale, saved=m._lora_saved,
                raw={k: [(n, a.clone(), b.clone(), al) for n, a, b, al in v] for k, v in m._lora_raw.items()},
                plan={k: (mp.adapters, mp.ranks, mp.ranges, mp.padded, mp.row, mp.slots) for k, mp in pk.modules.items()}, slots=pk.slots,
                scalars=scalars, columns=columns)


def test_load_a_load_b_delete_b_is_load_a():
    (_, sa), (_, sb) = _adapter(4, 11, alpha=2.0), _adapter(8, 12, families=None)
    only, both = _hip_model().load_lora(sa, adapter_name="a"), _hip_model().load_lora(sa, adapter_name="a")
    both.load_lora(sb, targets="transformer", adapter_name="b")
    assert len(both._lora_raw) == 12 * 16 and len(only._lora_raw) == 8 * 16
    both.delete_adapters(["b"])
    p, q = _host_state(only), _host_state(both)
    assert sorted(p) == sorted(q)
    for k in ("names", "weights", "scale", "saved", "plan", "slots"):
        assert p[k] == q[k], k
    assert torch.equal(p["scalars"], q["scalars"]) and torch.equal(p["columns"], q["columns"])
    assert list(p["raw"]) == list(q["raw"])
    for k in p["raw"]:
        for (n1, a1, b1, al1), (n2, a2, b2, al2) in zip(p["raw"][k], q["raw"][k]):
            assert n1 == n2 and al1 == al2 and torch.equal(a1, a2) and torch.equal(b1, b2)
    assert all(mp[4] is None for mp in q["plan"].values())  # no stacked module: every launch is the single-adapter one
    both.delete_adapters("a")
    assert not both.has_lora and both._lora_raw is None


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
def test_merged_and_hooked_oracles_agree_for_two_weighted_adapters():
    ou = _oracle()
    g = torch.Generator().manual_seed(61)
    lat, ctx = torch.randn(1, 4, 16, 16, generator=g), torch.randn(2, 77, 64, generator=g)
    x = torch.cat([lat, lat])
    (ca, _), (cb, _) = _adapter(4, 11, alpha=2.0), _adapter(8, 12, alpha=4.0, families=None)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    with torch.no_grad():
        plain = ou(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
        for s, (wa, wb) in ((1.0, (1.0, 1.0)), (0.7, (0.8, -0.5))):
            ads = [(ca, wa), (cb, wb)]
            merged = MR.merged_oracle(ou, ads, s)(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
            hooked = MR.hooked_oracle(ou, ads, s)(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
            e = rel(hooked, merged)
            print(f"scale {s} weights {wa} / {wb}: merged vs hooked {e:.3e}; the adapters move the output by {rel(merged, plain):.3f}")
            assert e < 2e-5  # tests/test_lora_cpu.py: float32 round-off through the whole UNet
            assert rel(merged, plain) > 10 * 3e-2  # ... and its MODEL_TOL_LOOSEST condition
        # one adapter with weight 1 is the one-adapter reference; weight 0 on both is the plain UNet
        one = MR.merged_oracle(ou, [(ca, 1.0), (cb, 0.0)], 0.5)(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
        assert torch.equal(one, R.merged_oracle(ou, ca, 0.5)(x, torch.tensor(501), encoder_hidden_states=ctx)[0])
        assert torch.equal(MR.merged_oracle(ou, [(ca, 0.0), (cb, 0.0)])(x, torch.tensor(501), encoder_hidden_states=ctx)[0], plain)


# ---------------------------------------------------------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_stacked_bound_holds_for_the_contract_and_catches_a_wrong_or_missing_scale(dtype):
    ranks = (3, 5, 8)
    x, a, b, y, cs = MR.stacked_operands(161, 128, ranks, 200, dtype, seed=3)
    assert a.shape[0] == 32 and not a[16:].any() and float(cs[16]) == 1.0e4
    ref, bound = MR.stacked_ref_bound(x, a, b, y, cs, dtype)
    worst = P.assert_elementwise(MR.emulate(x, a, b, y, cs, dtype), ref, bound, f"emulation {dtype}")
    print(f"stacked emulation {dtype}: max |err| / bound = {worst:.3f}")
    # the float64 reference is the sum of the adapters' own updates, each column at its own scale
    want = y.double()
    for c0, c1 in MR.column_ranges(ranks):
        want = want + ((x.double() @ a[c0:c1].double().T) * cs[c0:c1].double()) @ b[:, c0:c1].double().T
    assert float((ref - want).abs().max()) < 1e-9
    # teeth 1: the neighbouring column's scale
    wrong = cs.clone()
    wrong[:16] = cs[:16].roll(1)
    assert int(P.violations(MR.emulate(x, a, b, y, wrong, dtype), ref, bound)[0].sum()) > ref.numel() // 4
    # teeth 2: the last adapter's columns skipped
    skipped = cs.clone()
    skipped[8:16] = 0
    assert int(P.violations(MR.emulate(x, a, b, y, skipped, dtype), ref, bound)[0].sum()) > ref.numel() // 4
    # teeth 3: the scale BEHIND That's rounding (the single-adapter kernel's place for it) is another arithmetic, but within the same
    # bound up to That's rounding: no teeth are claimed there
    # the GEGLU form of the bound: an emulation of (value + U) * gelu(gate + U) passes, the skipped adapter fails
    C = 64
    xg, ag, bg, yg, csg = MR.stacked_operands(70, C, ranks, 8 * C, dtype, seed=5)
    that = (csg.float()[None, :] * (xg.float() @ ag.float().T)).to(dtype)
    v, gt = FR.deinterleave_cols(yg.float() + that.float() @ bg.float().T)
    fref, fbound = MR.stacked_geglu_ref_bound(xg, ag, bg, yg, csg, dtype)
    P.assert_elementwise((v * torch.nn.functional.gelu(gt)).to(dtype), fref, fbound, f"GEGLU emulation {dtype}")
    sk = csg.clone()
    sk[8:16] = 0
    that = (sk.float()[None, :] * (xg.float() @ ag.float().T)).to(dtype)
    v, gt = FR.deinterleave_cols(yg.float() + that.float() @ bg.float().T)
    assert int(P.violations((v * torch.nn.functional.gelu(gt)).to(dtype), fref, fbound)[0].sum()) > fref.numel() // 4


def test_hip_ops_stacked_entry_points_refuse_host_tensors_and_name_the_missing_route():
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import SIGNATURES, HipExtensionError

    assert "gmd_lora_update_stacked" in SIGNATURES and "gmd_lora_geglu_stacked" in SIGNATURES
    x, a, b, y = torch.zeros(8, 64, dtype=torch.bfloat16), torch.zeros(32, 64, dtype=torch.bfloat16), torch.zeros(64, 32, dtype=torch.bfloat16), \
        torch.zeros(8, 64, dtype=torch.bfloat16)
    with pytest.raises(HipExtensionError):
        ops.lora_update_stacked(x, a, b, y, torch.ones(1, 32), 0)
    with pytest.raises(HipExtensionError, match="parts"):  # float32 has no stacked kernel: the sequential route needs the parts
        ops.lora_update_stacked(x.float(), a.float(), b.float(), y.float(), torch.ones(1, 32), 0)
    with pytest.raises(HipExtensionError, match="parts"):
        ops.lora_geglu_stacked(x, a, b, y, torch.ones(1, 32), 0, fused=False)
