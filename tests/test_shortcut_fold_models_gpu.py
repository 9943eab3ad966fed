"""The conv2 + conv_shortcut fold inside the models: tiny UNet and tiny VAE against the CPU oracle under the tolerances of
tests/test_models_gpu.py, with the fold on (no separate shortcut projection is launched) and off (every one is).

The tiny models' channel widths (64 / 128) never reach the 256-row ping-pong plan on their own, so every 16-bit contraction of these
forwards is put on it with gmd_gemm_plan_override(256, 128, 283, .) -- the kernel whose loader walks the K tail."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture
def pp_everywhere():
    from gm_diffusion._native import lib

    prev = os.environ.get("GMD_TUNING")
    os.environ["GMD_TUNING"] = "1"
    assert lib().gmd_gemm_plan_override(256, 128, 283, 0) == 0
    yield
    lib().gmd_gemm_plan_override(0, 0, 0, 0)
    if prev is None:
        os.environ.pop("GMD_TUNING", None)
    else:
        os.environ["GMD_TUNING"] = prev


@pytest.fixture(scope="module")
def unet_case():
    """(oracle UNet, inputs, oracle output): computed once, shared by both switch positions."""
    from oracle import fixtures

    ou = fixtures.build_unet("tiny", 8)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 16, 16, generator=g)
    ctx = torch.randn(2, 77, ou.config.cross_attention_dim, generator=g)
    return ou, x, ctx, ou(x, torch.tensor(981), encoder_hidden_states=ctx)[0]


@pytest.fixture(scope="module")
def vae_case():
    from oracle import fixtures

    ov = fixtures.build_vae("tiny")
    z = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(9)) * 3
    return ov, z, ov.decode(z)[0]


def _counts(ops):
    return ops.shortcut_fold_uses, ops.shortcut_launches


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_tiny_unet_with_and_without_the_fold(fused, unet_case, pp_everywhere, monkeypatch):
    from gm_diffusion import hip_ops as ops
    from gm_diffusion.components import UNet2DConditionModel

    ou, x, ctx, ref = unet_case
    monkeypatch.setattr(ops, "USE_SHORTCUT_FOLD", fused)
    hu = UNet2DConditionModel(**dict(vars(ou.config)))
    hu.load_state_dict(ou.state_dict())
    hu.to(DEV, BF16)
    n_sc = sum(k.endswith(".conv_shortcut.weight") for k in ou.state_dict())
    f0, s0 = _counts(ops)
    got = hu(x.to(DEV), 981, encoder_hidden_states=ctx.to(DEV), return_dict=False)[0]
    f1, s1 = _counts(ops)
    assert rel_err(got, ref) < 3e-2
    assert (f1 - f0, s1 - s0) == ((n_sc, 0) if fused else (0, n_sc)) and n_sc > 0


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_tiny_vae_decode_with_and_without_the_fold(fused, vae_case, pp_everywhere, monkeypatch):
    from gm_diffusion import hip_ops as ops
    from gm_diffusion.components import AutoencoderKL

    ov, z, ref = vae_case
    monkeypatch.setattr(ops, "USE_SHORTCUT_FOLD", fused)
    hv = AutoencoderKL(**dict(vars(ov.config)))
    hv.load_state_dict(ov.state_dict())
    hv.to(DEV, BF16)
    n_sc = sum(k.startswith("decoder.") and k.endswith(".conv_shortcut.weight") for k in ov.state_dict())
    f0, s0 = _counts(ops)
    got = hv.decode(z.to(DEV), return_dict=False)[0]
    f1, s1 = _counts(ops)
    assert got.shape == ref.shape and rel_err(got, ref) < 3e-2
    assert (f1 - f0, s1 - s0) == ((n_sc, 0) if fused else (0, n_sc)) and n_sc > 0
