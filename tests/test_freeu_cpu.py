"""CPU: FreeU.  The closed form the HIP kernel evaluates against diffusers' ``fourier_filter`` restated with ``torch.fft`` (every
H x W in 1..40 x 1..40), known answers, the derived per-element bound of tests/freeu_ref.py against a CPU emulation of the kernel's
arithmetic and against three deliberately wrong variants, the host surface, and the condition the GPU model tests rest on.

What the whole-model comparisons can and cannot see: GroupNorm absorbs most of a channel scaling, so NO FreeU setting moves the tiny
UNet by 10 x the bfloat16 model gate (3e-2): the strongest one tried, (0.2, 0.2, 3.0, 3.0), moves it by ~0.13.  A 16-bit whole-model
comparison therefore cannot see a single dropped or mis-wired parameter.  That weight is carried by the float32 model test (each
parameter alone moves the output by more than 100 x the float32 gate), by the kernel's per-element tests and by the launch-count test
(tests/test_freeu_gpu.py)."""
import functools

import pytest
import torch

import freeu_ref as R
import parity as P

F32_MODEL_GATE = 2e-5   # tests/test_models_gpu.py MODEL_TOL[float32]
BF16_MODEL_GATE = 3e-2  # ... MODEL_TOL[bfloat16]
SETTING = dict(s1=0.9, s2=0.2, b1=1.5, b2=1.6)
STRONG = dict(s1=0.2, s2=0.2, b1=3.0, b2=3.0)


def test_closed_form_equals_the_fft_restatement_for_every_size_up_to_40():
    g = torch.Generator().manual_seed(1)
    worst = 0.0
    for H in range(1, 41):
        for W in range(1, 41):
            x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
            for s in (0.9, 0.2):
                e = float((R.closed_form64(x, s) - R.fourier_filter64(x, s)).abs().max())
                worst = max(worst, e)
                assert e < 1e-12, (H, W, s, e)  # float64 round-off of a 1600-point transform of N(0, 1) data
    print(f"closed form vs torch.fft, 1..40 x 1..40, two scales: max |diff| {worst:.2e}")


def test_known_answers():
    s = 0.2
    for H, W in ((1, 1), (1, 4), (2, 2), (3, 5), (8, 8), (17, 30)):
        c = torch.full((1, 1, H, W), 3.25, dtype=torch.float64)
        for f in (R.fourier_filter64, R.closed_form64):
            assert torch.allclose(f(c, s), s * c, rtol=0, atol=1e-13), (H, W)  # a constant field is the DC bin alone
    for H, W, factor in ((8, 8, (1 + s) / 2), (3, 5, (1 + s) / 2), (17, 1, (1 + s) / 2), (2, 6, s), (2, 1, s)):
        y = torch.arange(H, dtype=torch.float64)
        x = torch.cos(2 * torch.pi * y / H)[None, None, :, None].expand(1, 1, H, W)
        for f in (R.fourier_filter64, R.closed_form64):
            # the bin set holds -1 without +1: half of a real cosine is scaled (H > 2); at H = 2 the bin is its own conjugate
            assert torch.allclose(f(x, s), factor * x, rtol=0, atol=1e-13), (H, W)


def _site_inputs(B, H, W, Ca, Cs, dtype, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(B * H * W, Ca, generator=g) + offset).to(dtype)
    S = (torch.randn(B * H * W, Cs, generator=g) + offset).to(dtype)
    return A, S


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_bound_holds_for_a_clean_emulation_of_the_kernel(dtype):
    for (H, W), offset, s in (((1, 1), 0.0, 0.2), ((1, 4), 0.0, 0.9), ((2, 2), 50.0, 0.2), ((3, 5), 0.0, 0.2), ((8, 8), 50.0, 0.9),
                              ((17, 30), 50.0, 0.2), ((17, 30), 0.0, 0.9), ((34, 60), 50.0, 0.2)):
        B, Ca, Cs = 2, 16, 24
        A, S = _site_inputs(B, H, W, Ca, Cs, dtype, seed=H * 100 + W, offset=offset)
        ref, bound = R.site_ref_bound(A, S, B, H, W, 1.5, s, dtype)
        got_s = R.emulate_site(S, B, H, W, s, dtype)
        got_a = A.clone()
        got_a[:, :Ca // 2] = A[:, :Ca // 2] * 1.5
        r = P.assert_elementwise(torch.cat([got_a, got_s], -1), ref, bound, f"emulation {dtype} {H}x{W} mean {offset}")
        assert r <= 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_bound_catches_a_dropped_bin_the_symmetric_set_and_a_double_dc(dtype):
    """Each wrong variant must violate the bound on more than a quarter of the skip's elements."""
    s, B, Ca, Cs = 0.2, 2, 16, 24
    sym = [(u, v) for u in (-1, 0, 1) for v in (-1, 0, 1)]
    for (H, W), bins, what in (((3, 5), [(0, 0), (1, 0), (0, 1)], "the (-1, -1) bin dropped"),
                               ((8, 8), [(0, 0), (1, 0), (0, 1)], "the (-1, -1) bin dropped"),
                               ((3, 5), sym, "the conjugate-symmetric set"),
                               ((8, 8), sym, "the conjugate-symmetric set"),
                               ((5, 1), [(0, 0), (1, 0), (0, 1), (1, 1)], "the DC bin counted twice at W = 1"),
                               ((1, 1), [(0, 0), (1, 0), (0, 1), (1, 1)], "the DC bin counted four times at 1 x 1")):
        A, S = _site_inputs(B, H, W, Ca, Cs, dtype, seed=7 + H + W)
        ref, bound = R.site_ref_bound(A, S, B, H, W, 1.0, s, dtype)
        clean = R.emulate_site(S, B, H, W, s, dtype)
        assert int(P.violations(clean, ref[:, Ca:], bound[:, Ca:])[0].sum()) == 0
        bad = R.emulate_site(S, B, H, W, s, dtype, bins=bins)
        n = int(P.violations(bad, ref[:, Ca:], bound[:, Ca:])[0].sum())
        assert n > S.numel() // 4, f"{what} at {H}x{W} {dtype}: only {n} of {S.numel()} elements outside the bound"


# ---------------------------------------------------------------------------------------------------------------------------
# host surface
# ---------------------------------------------------------------------------------------------------------------------------
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


def test_enable_disable_and_the_property():
    m = _hip_model()
    assert m.freeu is None
    assert m.enable_freeu(0.9, 0.2, 1.5, 1.6) is m and m.freeu == (0.9, 0.2, 1.5, 1.6)
    m.enable_freeu(s1=1.0, s2=1.0, b1=1.0, b2=1.0)
    assert m.freeu == (1.0, 1.0, 1.0, 1.0)
    m.to("cpu", torch.bfloat16)  # .to keeps the setting
    assert m.freeu == (1.0, 1.0, 1.0, 1.0)
    assert m.disable_freeu() is m and m.freeu is None
    with pytest.raises(AttributeError):
        m.freeu = (1, 1, 1, 1)
    # out of scope, refused where a call could ask for it: another threshold, per-block settings
    with pytest.raises(NotImplementedError, match="threshold"):
        m.enable_freeu(0.9, 0.2, 1.5, 1.6, threshold=2)
    with pytest.raises(NotImplementedError, match="b1"):
        m.enable_freeu(0.9, 0.2, [1.5, 1.4], 1.6)
    assert m.freeu is None


@pytest.mark.parametrize("name", ["s1", "s2", "b1", "b2"])
@pytest.mark.parametrize("bad", [0.0, -0.5, float("inf"), float("nan")])
def test_values_must_be_finite_and_positive(name, bad):
    m = _hip_model()
    kw = dict(SETTING)
    kw[name] = bad
    with pytest.raises(ValueError, match=name):
        m.enable_freeu(**kw)
    assert m.freeu is None


def test_hip_op_refuses_host_tensors():
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import HipExtensionError

    with pytest.raises(HipExtensionError):
        ops.concat_channels_freeu(torch.zeros(4, 16), torch.zeros(4, 8), 1, 2, 2, torch.ones(4), 2, 0)


def test_pipelines_forward_to_their_unet_only():
    from gm_diffusion.components import PNDMScheduler
    from gm_diffusion.pipelines import (StableDiffusionDualUNetImprovedPipeline, StableDiffusionDualUNetPipeline,
                                        StableDiffusionGMPipeline)

    for cls in (StableDiffusionDualUNetPipeline, StableDiffusionDualUNetImprovedPipeline):
        pipe = cls(vae=None, text_encoder=None, tokenizer=None, unet=_hip_model(), gm_unet=_hip_model(), scheduler=PNDMScheduler(),
                   safety_checker=None, feature_extractor=None, requires_safety_checker=False)
        pipe.enable_freeu(**SETTING)
        assert pipe.unet.freeu == (0.9, 0.2, 1.5, 1.6) and pipe.gm_unet.freeu is None
        pipe.gm_unet.enable_freeu(**STRONG)
        pipe.disable_freeu()
        assert pipe.unet.freeu is None and pipe.gm_unet.freeu == (0.2, 0.2, 3.0, 3.0)
        with pytest.raises(ValueError, match="b2"):
            pipe.enable_freeu(s1=0.9, s2=0.2, b1=1.5, b2=0)
    pipe = StableDiffusionGMPipeline(vae=None, text_encoder=None, tokenizer=None, unet=_hip_model(), scheduler=PNDMScheduler(),
                                     safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe.enable_freeu(**SETTING)
    assert pipe.unet.freeu == (0.9, 0.2, 1.5, 1.6)
    pipe.disable_freeu()
    assert pipe.unet.freeu is None


# ---------------------------------------------------------------------------------------------------------------------------
# the condition the GPU model tests rest on, for the reference alone
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(side):
    """The inputs of tests/test_lora_cpu._case (seed 61), and the same draw at an 8 x 8 latent (FreeU levels 1 x 1 and 2 x 2)."""
    g = torch.Generator().manual_seed(61)
    lat, ctx = torch.randn(1, 4, side, side, generator=g), torch.randn(2, 77, 64, generator=g)
    return torch.cat([lat, lat]), ctx


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("side", [16, 8])
def test_every_parameter_alone_moves_the_reference_far_beyond_the_float32_gate(side):
    ou = _oracle()
    x, ctx = _case(side)
    t = torch.tensor(501)
    with torch.no_grad():
        plain = ou(x, t, encoder_hidden_states=ctx)[0]
        ones = R.hooked_oracle(ou, 1.0, 1.0, 1.0, 1.0)(x, t, encoder_hidden_states=ctx)[0]
        assert torch.equal(ones, plain)  # all four at 1: bit-identical
        for name, value in SETTING.items():
            kw = dict(s1=1.0, s2=1.0, b1=1.0, b2=1.0)
            kw[name] = value
            moved = _rel(R.hooked_oracle(ou, **kw)(x, t, encoder_hidden_states=ctx)[0], plain)
            print(f"latent {side}x{side}: {name}={value} alone moves the output by {moved:.3e}")
            assert moved > 100 * F32_MODEL_GATE, (name, moved)
        strong = _rel(R.hooked_oracle(ou, **STRONG)(x, t, encoder_hidden_states=ctx)[0], plain)
        print(f"latent {side}x{side}: {STRONG} moves the output by {strong:.3f}")
        assert strong > 3 * BF16_MODEL_GATE
