"""Case tables, references and bounds of the float32 split-path parity tests (plain helper module, like tests/parity.py): shared by
tests/test_split_parity_gpu.py (the kernels) and tests/test_split_parity_cpu.py (a clean emulation passes every one of these bounds, an
injected fault breaks it).  Device-agnostic: everything is computed where the tensors live.

The shapes were chosen by reading base_plan / f32_plan (csrc/gemm_plan.cpp); the GPU tests assert each expected plan through
gmd_split_plan_info before they launch, tests/test_gemm_plan_cpu.py asserts the same table without a GPU."""
import math

import torch

import parity as P

F32 = torch.float32
FORMS = ("F32S", "F32SW", "F32SA")                    # in-kernel split, pre-split weights, pre-split operand
FORM_CODE = {"F32S": 3, "F32SW": 4, "F32SA": 5}     # GMD_F32S / GMD_F32SW / GMD_F32SA of include/gmd_hip.h

# name -> (M, N, K, (tile rows, tile columns, K slices))
GEMM_CASES = {
    "128x160 full": (4096, 1280, 64, (128, 160, 1)),             # 32 x 8 = 256 tiles: the fewest that keep 128-row tiles unsplit
    "128x160 ragged in M": (4100, 1280, 96, (128, 160, 1)),
    "128x128 full": (4096, 1024, 64, (128, 128, 1)),
    "128x128 ragged in both": (4100, 1288, 96, (128, 128, 1)),
    "64x64 ragged": (300, 200, 320, (64, 64, 1)),
    "slabs 128x160": (256, 320, 2560, (128, 160, 5)),
    "slabs 128x128": (128, 128, 1536, (128, 128, 3)),
    "slabs 128x128 ragged": (200, 328, 2560, (128, 128, 5)),
    "slabs 64x64": (64, 320, 2048, (64, 64, 4)),
}
# The one production launch whose slab reduction takes a second grid-stride lap (see reducer_lap_start)
SECOND_LAP = ("reducer second lap", 4096, 1280, 10240, (128, 160, 2))

# splitk_reduce_f32_kernel (csrc/gemm_split.hip, launch_split_any): one thread per four columns of a row, total = M ceil(N / 4), in a
# grid capped at REDUCE_GRID_CAP workgroups of REDUCE_THREADS threads; thread i of the first lap comes back as i + LAP_REDUCE
REDUCE_GRID_CAP, REDUCE_THREADS = 4096, 256
LAP_REDUCE = REDUCE_GRID_CAP * REDUCE_THREADS  # 1,048,576 threads = 4,194,304 columns: the "M x N > 4,194,304" of a second lap


def reducer_lap_start(M, N):
    """(row, column) of the first output element the reduction writes in its SECOND lap, or None when one lap covers the launch."""
    nc = (N + 3) // 4
    if M * nc <= LAP_REDUCE:
        return None
    return LAP_REDUCE // nc, (LAP_REDUCE % nc) * 4


# epilogue variant -> (bias, rowbias, residual, alpha, activation)
EPILOGUES = {
    "bias+rowbias+residual": (True, True, True, 0.5, None),
    "silu": (True, False, False, 1.0, "silu"),
    "quick_gelu": (True, False, False, 1.0, "quick_gelu"),
    "plain": (False, False, False, 1.0, None),
}


def rows_per_group(M):
    """The row-bias seam falls inside a tile (and inside a 16-row fragment): every 100 rows, every 24 for the launches of one small tile."""
    return 100 if M > 100 else 24


def gemm_inputs(M, N, K, device="cpu"):
    g = torch.Generator().manual_seed(M + N + K)
    rpg = rows_per_group(M)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    rb = torch.randn((M + rpg - 1) // rpg, N, generator=g)
    return tuple(t.to(device) for t in (a, w, bias, res, rb)) + (rpg,)


def scaled(w):
    """hip_ops.scale_weight without the library: (w 2^s with the largest magnitude in [2^12, 2^13), 2^-s)."""
    amax = float(w.abs().max()) if w.numel() else 0.0
    s = 0 if amax == 0.0 or not math.isfinite(amax) else max(-60, min(60, 13 - math.frexp(amax)[1]))
    return w * (2.0 ** s), 2.0 ** -s


class Core:
    """The float64 products every epilogue variant of one (operand, effective weight) pair shares: computed once."""

    def __init__(self, a, weff, slices=1):
        a64, w64 = a.double(), weff.double()
        self.K = a.shape[-1]
        self.ref_acc = a64 @ w64.T
        self.abs_dot = a64.abs() @ w64.abs().T
        self.perr = P.split_product_bound(a, weff)
        # three instructions of 32 products per K step of 32 through ONE accumulator (gemm_split_kernel: compute()), then the slabs
        self.height = P.mfma_height(3 * self.K, 32, slices)


def extras_of(epi, bias, rb, rpg, res, shape):
    use_b, use_rb, use_res, alpha, act = EPILOGUES[epi]
    M = shape[0]
    ex = []
    if use_b:
        ex.append(bias.double().expand(shape))
    if use_rb:
        ex.append(rb.double().repeat_interleave(rpg, 0)[:M])
    if use_res:
        ex.append(res.double())
    return ex, alpha, act


def ref_and_bound(core, alpha, extras, act):
    """(float64 reference, per-element bound) of ``act(alpha (A W^T) + sum(extras))`` computed by the three-product kernels and stored
    as float32: parity.gemm_bound with 3 K accumulated products, the split's own product error and the kernel's K-loop height."""
    value = alpha * core.ref_acc
    for t in extras:
        value = value + t
    bound = P.gemm_bound(core.ref_acc, core.abs_dot, 3 * core.K, F32, alpha, extras, act, product_err=core.perr, height=core.height)
    return P._act_ref(value, act), bound


def exact_ref_and_bound(a, w, extras):
    """The exact float32 kernel (GMD_F32: an FMA chain in an order the test does not know): every product rounds once."""
    ref_acc, ad = a.double() @ w.double().T, a.double().abs() @ w.double().abs().T
    value = ref_acc
    for t in extras:
        value = value + t
    return value, P.gemm_bound(ref_acc, ad, a.shape[-1], F32, 1.0, extras, product_err=P.U_F32 * ad)


# ---------------------------------------------------------------------------------------------------------------------------
# conv3x3
# ---------------------------------------------------------------------------------------------------------------------------
MODES = ("s1", "s2", "pad1", "up", "up_to_odd")


def conv_kw(mode, out_size=None):
    return {"s1": dict(), "s2": dict(stride=2), "pad1": dict(stride=2, pad_mode=1), "up": dict(upsample=True), "up_to_odd": dict(out_size=out_size)}[mode]


# tile case -> (batch, Cin, Cout, {mode: (Hin, Win, out_size or None)}, (tile rows, tile columns, K slices)).  The input maps are
# chosen per mode so that every mode of a case puts the SAME number of pixels (so the same plan) on the chip: the stride-2 legs read
# an odd map, up_to_odd asks for the odd size (2 Hin - 1 and / or 2 Win - 1).
def _maps(s1, s2, pad1, up, odd, odd_size):
    return {"s1": (*s1, None), "s2": (*s2, None), "pad1": (*pad1, None), "up": (*up, None), "up_to_odd": (*odd, odd_size)}


CONV_TILES = {
    "64x64": (3, 128, 320, _maps((23, 20), (23, 20), (23, 20), (23, 20), (23, 20), (45, 39)), (64, 64, 1)),
    "128x160 full chip": (4, 32, 320, _maps((65, 63), (129, 125), (130, 126), (33, 32), (33, 32), (65, 63)), (128, 160, 1)),
    "128x128": (4, 32, 256, _maps((65, 63), (129, 125), (130, 126), (33, 32), (33, 32), (65, 63)), (128, 128, 1)),
    "64x64 slabs": (1, 256, 320, _maps((9, 7), (17, 13), (18, 14), (5, 4), (5, 4), (9, 7)), (64, 64, 4)),
    "128-row slabs": (2, 256, 320, _maps((12, 11), (23, 21), (24, 22), (6, 6), (6, 6), (12, 11)), (128, 160, 4)),
}
# 25 rows: every (mode, tile case) pair, the operand form walking a Latin square over them -- so every mode meets every form
# (a row of the square), every tile case meets every form (a column) and every mode meets every tile case.
CONV_CASES = [(mode, FORMS[(i + j) % 3], tile) for i, mode in enumerate(MODES) for j, tile in enumerate(CONV_TILES)]


def conv_inputs(tile, mode, device="cpu"):
    B, ci, co, maps, _ = CONV_TILES[tile]
    H, W, out_size = maps[mode]
    g = torch.Generator().manual_seed(H * W + ci + co + len(mode))
    x = torch.randn(B, H * W, ci, generator=g)
    w = torch.randn(co, 9 * ci, generator=g) / math.sqrt(9 * ci)
    bias = torch.randn(co, generator=g)
    tb = torch.randn(B, co, generator=g)
    kw = conv_kw(mode, out_size)
    ho, wo = P.im2col3x3(x[:1, :, :1], 1, H, W, **kw)[1:]
    res = torch.randn(B, ho * wo, co, generator=g)
    return tuple(t.to(device) for t in (x, w, bias, tb, res)) + (B, H, W, ho, wo, kw)


def conv_extras(bias, tb, res, B, hw, co):
    """bias + per-sample row bias + residual of the [B Ho Wo, Cout] output."""
    M = B * hw
    return [bias.double().expand(M, co), tb.double().repeat_interleave(hw, 0), res.double().reshape(M, co)]
