"""Upsample2D (nearest 2x + conv3x3) as four 2x2 phase convolutions over the low-resolution image (gmd_conv3x3_up2: the phase mode
of the 256-row ping-pong kernel, K = 4 Cin instead of 9 Cin).

Per-element bounds from tests/parity.py against a float64 reference computed from the PACKED (rounded) weights: gemm_bound with
K = 4 Cin.  The shapes are the smallest at which the phase loader and the epilogue's row map take each of their paths (all under the
co-running plan family, whose plans put these small launches on the ping-pong kernel):
  one-tile   B=1 16x16  64->128   exactly one 256-row tile per phase, one K step per tap; power-of-two row decoding
  partial    B=3  8x8  128->160   192 rows per phase: the last 64-row wave tile of every panel does not exist; statistics
  non-square B=2  8x24 192->320   two panels per phase (256 + 128 rows), two N tiles, three K steps per tap, rows decoded by division
  ragged     B=3  6x6   64->128   108 rows: a wave tile that is cut inside (register epilogue), samples that straddle wave tiles
  split-k    B=2  8x8  512->160   four K slices through the in-kernel reduction, with wave tiles that do not exist; statistics
Every case prints ``PARITY up2 <case> max|err|/bound=<r>``."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
PP = 283
GUARD = 65536  # bytes
TINY = {BF16: 2.0 ** -126, F16: 2.0 ** -25}

# (name, B, H, W, Cin, Cout, plan under family 1, statistics?)
SHAPES = [
    ("one-tile", 1, 16, 16, 64, 128, (256, 128, PP, 1), False),
    ("partial", 3, 8, 8, 128, 160, (256, 160, PP, 1), True),
    ("non-square", 2, 8, 24, 192, 320, (256, 160, PP, 1), True),
    ("ragged", 3, 6, 6, 64, 128, (256, 128, PP, 1), False),
    ("split-k", 2, 8, 8, 512, 160, (256, 160, PP, 4), True),
]


def _nchw(x, B, H, W):
    return x.view(B, H, W, -1).permute(0, 3, 1, 2)


def _rows(y):
    return y.permute(0, 2, 3, 1).reshape(y.shape[0], -1, y.shape[1])


def _conv9(x, w, B, H, W):
    """float64 conv3x3 of the nearest-2x image; x [B, HW, Cin], w [Cout, 9 Cin] tap-major -> [B, 4HW, Cout]."""
    ci, co = x.shape[-1], w.shape[0]
    up = F.interpolate(_nchw(x, B, H, W), scale_factor=2, mode="nearest")
    return _rows(F.conv2d(up, w.view(co, 3, 3, ci).permute(0, 3, 1, 2), padding=1))


def _conv4(x, wp, B, H, W):
    """float64 phase convolutions from the packed weights [4, Cout, 4 Cin], written from the documented layout: tap (a, b) of phase
    (py, px) reads source pixel (i + a + py - 1, j + b + px - 1).  One 2x2 correlation over the padded image per phase: its output
    at (u, v) sums xp[u + a, v + b] = x[u + a - 1, v + b - 1], so pixel (i, j) of the phase is the output at (i + py, j + px)."""
    ci, co = x.shape[-1], wp.shape[1]
    xp = F.pad(_nchw(x, B, H, W), (1, 1, 1, 1))
    out = torch.zeros(B, co, 2 * H, 2 * W, dtype=x.dtype, device=x.device)
    for py, px in itertools.product(range(2), range(2)):
        k = wp[2 * py + px].view(co, 2, 2, ci).permute(0, 3, 1, 2)
        out[:, :, py::2, px::2] = F.conv2d(xp, k)[:, :, py:py + H, px:px + W]
    return _rows(out)


class Case:
    """Inputs of one (shape, dtype), the packed weights and the float64 references -- computed once, shared by every check."""

    def __init__(self, ops, shape, dtype, seed):
        self.name, self.B, self.H, self.W, self.ci, self.co, self.plan, self.stats = shape
        B, H, W, ci, co = self.B, self.H, self.W, self.ci, self.co
        g = torch.Generator().manual_seed(seed)
        self.dtype = dtype
        self.x = torch.randn(B, H * W, ci, generator=g).to(dtype).to(DEV)
        self.w9 = (torch.randn(co, 9 * ci, generator=g) * 0.03).to(dtype).to(DEV)
        self.bias = torch.randn(co, generator=g).to(DEV)
        self.tb = torch.randn(B, co, generator=g).to(DEV)
        self.res = torch.randn(B, 4 * H * W, co, generator=g).to(dtype).to(DEV)
        self.wp, _ = ops.pack_upsample_phases(self.w9)
        x64 = self.x.double()
        self.acc4 = _conv4(x64, self.wp.double(), B, H, W)
        self.abs4 = _conv4(x64.abs(), self.wp.double().abs(), B, H, W)
        self.acc9 = _conv9(x64, self.w9.double(), B, H, W)
        self.abs9 = _conv9(x64.abs(), self.w9.double().abs(), B, H, W)
        # |x| against the magnitude of the EXACT merged weights (float64 sums of the nine-tap weights): the term of the one extra rounding
        wm64, _ = ops.pack_upsample_phases(self.w9.double())
        self.abs_wm = _conv4(x64.abs(), wm64.abs(), B, H, W)

    def extras(self, bias, rowbias, residual):
        ex = []
        if bias:
            ex.append(self.bias.double().expand_as(self.acc4))
        if rowbias:
            ex.append(self.tb.double()[:, None, :].expand_as(self.acc4))
        if residual:
            ex.append(self.res.double())
        return ex

    def kwargs(self, bias, rowbias, residual):
        return dict(bias=self.bias if bias else None, rowbias=self.tb if rowbias else None, residual=self.res if residual else None)


@pytest.fixture(scope="module")
def cases():
    from gm_diffusion import hip_ops as ops

    cache = {}

    def get(shape, dtype):
        key = (shape[0], dtype)
        if key not in cache:
            cache[key] = Case(ops, shape, dtype, 1000 + len(cache))
        return cache[key]

    return get


def _check_stats(ops, y, c, what):
    """{sum, sum of squares} of the STORED output per 64-row block and 10-column bucket.  Block (b 4 + z)(HW / 64) + k holds pixels
    64k .. 64k + 63 (low-resolution, row-major) of phase z of sample b (include/gmd_hip.h); summed over a sample's blocks they are the
    per-sample sums a GroupNorm folds.  Tolerances as tests/test_shortcut_fold_gpu.py: a float32 sum of n values along any tree is
    within (n - 1) 2^-24 sum |x| of the exact one, the squares (exact in float32 for 16-bit values) n 2^-24 sum x^2; n = 64 x 10."""
    assert getattr(y, "_colstats", None) is not None, f"{what}: the launch did not emit column statistics"
    st, n = y._colstats
    B, H, W, co = c.B, c.H, c.W, c.co
    nb = co // ops.COLSTATS_BUCKET
    assert n == co and st.shape == (B * 4 * H * W // 64, nb, 2)
    # [b, 2i + py, 2j + px, c] -> [b, z, pixel block, 64 pixels, bucket, 10]
    y64 = y.double().view(B, H, 2, W, 2, co).permute(0, 2, 4, 1, 3, 5).reshape(B * 4 * (H * W // 64), 64, nb, ops.COLSTATS_BUCKET)
    s, q = y64.sum((1, 3)), (y64 * y64).sum((1, 3))
    nv = 64 * ops.COLSTATS_BUCKET
    P.assert_elementwise(st[..., 0], s, (nv - 1) * P.U_F32 * y64.abs().sum((1, 3)) + 1e-30, f"{what}: colstats sums")
    P.assert_elementwise(st[..., 1], q, nv * P.U_F32 * q + 1e-30, f"{what}: colstats squares")
    # per sample and bucket, whatever the order of the blocks inside a sample
    per = B, 4 * H * W // 64, nb
    P.assert_elementwise(st[..., 0].double().view(*per).sum(1), y.double().view(B, -1, nb, 10).sum((1, 3)),
                         (nv - 1) * P.U_F32 * y.double().abs().view(B, -1, nb, 10).sum((1, 3)) + 1e-30, f"{what}: per-sample sums")


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_phase_launch_per_element(shape, dtype, cases):
    from gm_diffusion import hip_ops as ops

    c = cases(shape, dtype)
    B, H, W, ci, co = c.B, c.H, c.W, c.ci, c.co
    u = P.unit_roundoff(dtype)
    with ops.plan_family(1):
        assert ops.upsample_phases_plan(dtype, B, H, W, ci, co, colstats=c.stats) == c.plan
        assert ops.upsample_phases_ok(dtype, B, H, W, ci, co, (2 * H, 2 * W), colstats=c.stats)
        n0 = ops.upsample_phase_uses
        runs = 0
        # (d) every combination of the epilogue's addends, 16-bit output; (a) each against the packed-weight reference
        for bias, rowbias, residual in ((1, 0, 0), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1), (0, 0, 0)):
            what = f"{c.name} {dtype} bias={bias} rowbias={rowbias} residual={residual}"
            ex = c.extras(bias, rowbias, residual)
            # (e) the output sits between guard bands of the test's own memory and starts as NaN
            total = 2 * (GUARD // 2) + c.acc4.numel()
            buf = torch.full((total,), float("nan"), dtype=dtype, device=DEV)
            before = buf.view(torch.int16).clone()
            out = buf[GUARD // 2: GUARD // 2 + c.acc4.numel()].view(B, 4 * H * W, co)
            y, ho, wo = ops.conv3x3_up2(c.x, c.wp, B, H, W, colstats=c.stats, out=out, **c.kwargs(bias, rowbias, residual))
            runs += 1
            torch.cuda.synchronize()
            assert (ho, wo) == (2 * H, 2 * W) and y.data_ptr() == out.data_ptr()
            after = buf.view(torch.int16)
            assert torch.equal(after[: GUARD // 2], before[: GUARD // 2]) and torch.equal(after[-(GUARD // 2):], before[-(GUARD // 2):]), \
                f"{what}: a store outside the output"
            assert not bool(torch.isnan(y).any()), f"{what}: {int(torch.isnan(y).any(-1).sum())} output rows were not written"
            ref = c.acc4 + sum(ex) if ex else c.acc4
            r = P.assert_elementwise(y, ref, P.gemm_bound(c.acc4, c.abs4, 4 * ci, dtype, 1.0, ex), what, (256, c.plan[1]))
            print(f"PARITY up2 {what} max|err|/bound={r:.3f}")
            if c.stats:  # (c)
                _check_stats(ops, y, c, what)
            else:
                assert getattr(y, "_colstats", None) is None
            # (b) against the nine-tap launch on the same inputs.  Both compute sum x W9 in exact arithmetic (the merged weight IS the
            # sum of the taps that read the same pixel); the phase launch rounds each merged weight once more -- u |Wm| per weight,
            # plus its float32 sum of at most four 16-bit values (3 2^-24 of the sum of their magnitudes) -- so the accumulators
            # differ by at most (u sum |x||Wm| + 3 2^-24 sum |x||W9|) plus either launch's float32 accumulation and epilogue
            # roundings; then each stored value is rounded once: u (|value| + that difference) on either side.
            y9, _, _ = ops.conv3x3(c.x, c.w9, B, H, W, upsample=True, **c.kwargs(bias, rowbias, residual))
            mag = c.acc9.abs() + sum(e.abs() for e in ex)
            d = (u * c.abs_wm + 3 * P.U_F32 * c.abs9 + P.accumulate_bound(c.abs4, 4 * ci) + P.accumulate_bound(c.abs9, 9 * ci)
                 + 2 * (1 + len(ex)) * P.U_F32 * (mag + u * c.abs_wm))
            tol = d + 2 * u * (mag + d) + 2 * TINY[dtype]
            P.assert_elementwise(y, y9.double(), tol, what + " vs nine-tap")
        # float32 output: the register epilogue with the phase row map (no statistics, no residual: the ABI's rules)
        ex = c.extras(1, 1, 0)
        y32, _, _ = ops.conv3x3_up2(c.x, c.wp, B, H, W, out_dtype=F32, **c.kwargs(1, 1, 0))
        runs += 1
        r = P.assert_elementwise(y32, c.acc4 + sum(ex), P.gemm_bound(c.acc4, c.abs4, 4 * ci, F32, 1.0, ex), f"{c.name} {dtype} -> float32", (256, c.plan[1]))
        print(f"PARITY up2 {c.name} {dtype} -> float32 max|err|/bound={r:.3f}")
        assert ops.upsample_phase_uses == n0 + runs
        # the workspace's arrival counters are back at zero (split-k)
        ws = ops._workspace(torch.device(DEV, torch.cuda.current_device()))
        assert not bool(ws[-(ops.WS_TAIL_BYTES // 4):].view(torch.int32).any())


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_split_k_back_to_back_launches_take_their_own_inputs(dtype, cases):
    """Two launches on the one workspace with different activations: a stale fragment of the first would show in the second."""
    from gm_diffusion import hip_ops as ops

    c = cases(SHAPES[4], dtype)
    B, H, W, ci, co = c.B, c.H, c.W, c.ci, c.co
    x2 = (c.x.float() * -0.5 + 0.25).to(dtype)
    acc = _conv4(x2.double(), c.wp.double(), B, H, W)
    ab = _conv4(x2.double().abs(), c.wp.double().abs(), B, H, W)
    with ops.plan_family(1):
        assert ops.upsample_phases_plan(dtype, B, H, W, ci, co)[3] == 4
        y1, _, _ = ops.conv3x3_up2(c.x, c.wp, B, H, W)
        y2, _, _ = ops.conv3x3_up2(x2, c.wp, B, H, W)
    P.assert_elementwise(y1, c.acc4, P.gemm_bound(c.acc4, c.abs4, 4 * ci, dtype), f"split-k first {dtype}", (256, 160))
    P.assert_elementwise(y2, acc, P.gemm_bound(acc, ab, 4 * ci, dtype), f"split-k second {dtype}", (256, 160))


def run_cblk_cases():
    """Body of test_phase_launch_with_channel_blocks; runs in a process whose library was loaded with GMD_CONV_CBLK=64."""
    from gm_diffusion import hip_ops as ops

    for shape in (SHAPES[2], SHAPES[4]):  # Cin = 192: three blocks of four taps; Cin = 512 in four K slices of two blocks each
        c = Case(ops, shape, BF16, 77)
        with ops.plan_family(1):
            assert ops.upsample_phases_plan(BF16, c.B, c.H, c.W, c.ci, c.co, colstats=c.stats) == c.plan
            y, _, _ = ops.conv3x3_up2(c.x, c.wp, c.B, c.H, c.W, bias=c.bias, colstats=c.stats)
        ex = c.extras(1, 0, 0)
        r = P.assert_elementwise(y, c.acc4 + ex[0], P.gemm_bound(c.acc4, c.abs4, 4 * c.ci, BF16, 1.0, ex), f"cblk=64 {c.name}", (256, 160))
        print(f"PARITY up2 cblk=64 {c.name} max|err|/bound={r:.3f}")
        _check_stats(ops, y, c, f"cblk=64 {c.name}")
    print("CBLK_CASES_OK")


def test_phase_launch_with_channel_blocks():
    """The K order with a channel block smaller than Cin (all four taps of channels 0..63, then of 64..127, ...): the block -> block
    hand-over of the phase loader, unsplit and with K slices that start at a block boundary.  No production shape takes a block below
    Cin here (the planner's blocks start at 3 MB of input rows per XCD), and the block is read from the environment when the library
    is loaded (GMD_TUNING=1), so the cases run in a child process."""
    import os
    import subprocess
    import sys

    env = dict(os.environ, GMD_TUNING="1", GMD_CONV_CBLK="64")
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r, %r]; import test_upsample_phases_gpu as T; T.run_cblk_cases()" % (
        here, os.path.dirname(here), os.path.join(os.path.dirname(here), "gm-diffusion_amd"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "CBLK_CASES_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_odd_target_size_keeps_the_nine_tap_launch(cases):
    """out_size 2H - 1 / 2W - 1: no phase launch (upsample_phases_ok), the nine-tap launch still passes its per-element bound."""
    from gm_diffusion import hip_ops as ops

    c = cases(SHAPES[1], BF16)
    B, H, W, ci, co = c.B, c.H, c.W, c.ci, c.co
    x64 = c.x.double()
    with ops.plan_family(1):
        n0 = ops.upsample_phase_uses
        for ho, wo in ((2 * H - 1, 2 * W), (2 * H, 2 * W - 1), (2 * H - 1, 2 * W - 1)):
            assert not ops.upsample_phases_ok(BF16, B, H, W, ci, co, (ho, wo))
            y, h2, w2 = ops.conv3x3(c.x, c.w9, B, H, W, bias=c.bias, out_size=(ho, wo))
            assert (h2, w2) == (ho, wo)

            def ref(xx, ww):
                up = F.interpolate(_nchw(xx, B, H, W), size=(ho, wo), mode="nearest")
                return _rows(F.conv2d(up, ww.view(co, 3, 3, ci).permute(0, 3, 1, 2), padding=1))

            acc, ab = ref(x64, c.w9.double()), ref(x64.abs(), c.w9.double().abs())
            ex = [c.bias.double().expand_as(acc)]
            P.assert_elementwise(y, acc + ex[0], P.gemm_bound(acc, ab, 9 * ci, BF16, 1.0, ex), f"nine-tap to {ho}x{wo}")
        assert ops.upsample_phase_uses == n0


def test_switch_and_refusals(cases, monkeypatch):
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import HipExtensionError

    c = cases(SHAPES[0], BF16)
    B, H, W = c.B, c.H, c.W
    n0 = ops.upsample_phase_uses
    with pytest.raises(HipExtensionError, match="gmd error 3"):  # family 0: four tiles never reach the ping-pong plan
        ops.conv3x3_up2(c.x, c.wp, B, H, W)
    with ops.plan_family(1):
        with pytest.raises(HipExtensionError):  # the nine-tap weight is not a phase weight
            ops.conv3x3_up2(c.x, c.w9, B, H, W)
        with pytest.raises(HipExtensionError):
            ops.conv3x3_up2(c.x.float(), c.wp.float(), B, H, W)
        monkeypatch.setattr(ops, "USE_UPSAMPLE_PHASES", False)
        assert not ops.upsample_phases_ok(BF16, B, H, W, c.ci, c.co)
    assert ops.upsample_phase_uses == n0


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def test_sd15_width_unet_takes_the_phase_path(monkeypatch):
    """SD-1.5-width UNet, 8x8 latents, batch 2, bfloat16 under the co-running plan family (what the dual pipeline's forwards run
    under): its three upsamplers take the phase launch and the forward meets the oracle bound of tests/test_f16_gpu.py (4e-2);
    with the switch off none does and the bound holds as before."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion.components import UNet2DConditionModel
    from oracle import fixtures

    g = torch.Generator().manual_seed(3)
    ou = fixtures.build_unet("sd15", 8)
    x = torch.randn(2, 8, 8, 8, generator=g)
    ctx = torch.randn(2, 77, ou.config.cross_attention_dim, generator=g)
    ref = ou(x, torch.tensor(701), encoder_hidden_states=ctx)[0]
    hu = UNet2DConditionModel(**vars(ou.config))
    hu.load_state_dict(ou.state_dict())
    hu.to(DEV, BF16)
    n_up = sum(k.endswith("upsamplers.0.conv.weight") for k in ou.state_dict())
    with ops.plan_family(1):
        n0 = ops.upsample_phase_uses
        got = hu(x.to(DEV), 701, encoder_hidden_states=ctx.to(DEV), return_dict=False)[0]
        e_on = rel_err(got, ref)
        assert ops.upsample_phase_uses - n0 == n_up == 3
        monkeypatch.setattr(ops, "USE_UPSAMPLE_PHASES", False)
        got0 = hu(x.to(DEV), 701, encoder_hidden_states=ctx.to(DEV), return_dict=False)[0]
        e_off = rel_err(got0, ref)
        assert ops.upsample_phase_uses - n0 == n_up
    print(f"sd15-width UNet bf16 rel err: phases {e_on:.3e}  nine-tap {e_off:.3e}")
    assert e_on < 4e-2 and e_off < 4e-2


def test_vae_decode_takes_the_phase_path():
    """Tiny VAE decoder (128 / 128 / 64 channels) under the co-running family: the two 128-channel upsamplers take the phase launch
    (64 columns have no ping-pong tile), and the decode meets the bound of tests/test_shortcut_fold_models_gpu.py (3e-2)."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion.components import AutoencoderKL
    from oracle import fixtures

    ov = fixtures.build_vae("tiny")
    z = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(9)) * 3
    ref = ov.decode(z)[0]
    hv = AutoencoderKL(**dict(vars(ov.config)))
    hv.load_state_dict(ov.state_dict())
    hv.to(DEV, BF16)
    with ops.plan_family(1):
        n0 = ops.upsample_phase_uses
        got = hv.decode(z.to(DEV), return_dict=False)[0]
        assert ops.upsample_phase_uses - n0 == 2
    assert got.shape == ref.shape and rel_err(got, ref) < 3e-2
