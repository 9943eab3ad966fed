"""Per-element parity of the HIP kernels against float64 torch (tests/parity.py: a derived bound for every element, zero violations
allowed), kernel family by kernel family, each case asserting the plan code / kernel it ran.  The global-norm assertions of the
other GPU files stay as they are; these add what those cannot see: one fragment, one row, one K step of one tile.

Every case prints ``PARITY <family> <case> max|err|/bound=<r>`` (pytest -s shows it): the figure a report quotes per family."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


@pytest.fixture
def force_plan():
    """gmd_gemm_plan_override is refused unless the process has GMD_TUNING=1 (include/gmd_hip.h)."""
    from gm_diffusion._native import lib

    prev = os.environ.get("GMD_TUNING")
    os.environ["GMD_TUNING"] = "1"
    fix = lib().gmd_splitk_fixup_max(-1)

    def force(bm, bn, pf, ks):
        assert lib().gmd_gemm_plan_override(bm, bn, pf, ks) == 0

    yield force
    lib().gmd_gemm_plan_override(0, 0, 0, 0)
    lib().gmd_conv_patch_override(0)
    lib().gmd_splitk_fixup_max(fix)
    if prev is None:
        os.environ.pop("GMD_TUNING", None)
    else:
        os.environ["GMD_TUNING"] = prev


def _report(family, case, r):
    print(f"PARITY {family} {case} max|err|/bound={r:.3f}")
    return r


# kernel -> (tile rows, tile columns, code passed to the override, code gmd_gemm_plan_info reports)
GEMM_PLANS = {
    "ring128x160": (128, 160, 9, 0), "ring128x128": (128, 128, 9, 0), "ring64x64": (64, 64, 9, 0),
    "pp256x160": (256, 160, 283, 283), "pp256x128": (256, 128, 283, 283),
    "lc128x160": (128, 160, 244, 244), "lc64x160": (64, 160, 244, 244), "lc128x128": (128, 128, 244, 244),
}


def _gemm_inputs(M, N, K, dtype, rpg):
    g = torch.Generator().manual_seed(M + N + K)  # the generators of test_gemm_nt
    a = torch.randn(M, K, generator=g).to(dtype).to(DEV)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dtype).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    res = torch.randn(M, N, generator=g).to(dtype).to(DEV)
    rb = torch.randn((M + rpg - 1) // rpg, N, generator=g).to(DEV)
    return a, w, bias, res, rb


def _check_gemm(ops, what, tile, a, w, bias, res, rb, rpg):
    """The epilogue variants of one (plan, shape): bias + rowbias (seam every ``rpg`` rows: inside tiles) + residual + alpha = 0.5
    with a 16-bit store; bias + SiLU with a float32 store; bias + rowbias + alpha with a float32 store; bias + quick-GELU with a
    16-bit store.  (The C ABI takes a residual only with out_dtype == dtype.)"""
    M, K = a.shape
    dtype = a.dtype
    ref_acc = a.double() @ w.double().T
    abs_dot = a.double().abs() @ w.double().abs().T
    rb_rows = rb.double().repeat_interleave(rpg, 0)[:M]
    worst = 0.0
    h = P.mfma_height(K, 32, 16)  # every 16-bit GEMM kernel chains mfma_f32_16x16x32 through one accumulator; at most 16 K slices
    ex = [bias.double().expand_as(ref_acc), rb_rows, res.double()]
    got = ops.gemm_nt(a, w, bias=bias, rowbias=rb, rows_per_group=rpg, residual=res, alpha=0.5)
    worst = max(worst, P.assert_elementwise(got, 0.5 * ref_acc + ex[0] + ex[1] + ex[2], P.gemm_bound(ref_acc, abs_dot, K, dtype, 0.5, ex, height=h), what + " bias+rowbias+residual", tile))
    ex = [bias.double().expand_as(ref_acc)]
    got = ops.gemm_nt(a, w, bias=bias, act=ops.ACT_SILU, out_dtype=F32)
    assert got.dtype == F32
    worst = max(worst, P.assert_elementwise(got, F.silu(ref_acc + ex[0]), P.gemm_bound(ref_acc, abs_dot, K, F32, 1.0, ex, "silu", height=h), what + " silu -> float32", tile))
    got = ops.gemm_nt(a, w, bias=bias, rowbias=rb, rows_per_group=rpg, alpha=0.5, out_dtype=F32)  # float32 straight from the accumulators
    worst = max(worst, P.assert_elementwise(got, 0.5 * ref_acc + ex[0] + rb_rows, P.gemm_bound(ref_acc, abs_dot, K, F32, 0.5, [ex[0], rb_rows], height=h), what + " -> float32", tile))
    got = ops.gemm_nt(a, w, bias=bias, act=ops.ACT_QUICK_GELU)
    v = ref_acc + ex[0]
    worst = max(worst, P.assert_elementwise(got, v * torch.sigmoid(1.702 * v), P.gemm_bound(ref_acc, abs_dot, K, dtype, 1.0, ex, "quick_gelu", height=h), what + " quick-gelu", tile))
    return worst


@pytest.mark.parametrize("plan", list(GEMM_PLANS))
def test_gemm_16bit_every_kernel_per_element(plan, force_plan):
    """Ring kernels (128x160, 128x128, 64x64), ping-pong (283, 160 and 128 columns), loader / consumer (244, 128- and 64-row): a
    full-tile shape, a ragged one (M = 1000; N = 328 where the kernel's existing cases have ragged N), K slices through BOTH reduction
    paths (slabs: gmd_splitk_fixup_max(0); in-kernel: the default), production shapes (8192 x 1280 x 640, the level-1 fused qk
    projection; 2048 x 1280 x 1280, level-2 projections; 4096 x 640 x 640 at f16), bf16 and f16."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    bm, bn, pf, code = GEMM_PLANS[plan]
    fix_default = lib().gmd_splitk_fixup_max(-1)
    n_ragged = 328 if pf != 244 else 3 * bn  # the 244 kernel's cases keep N on tile boundaries
    shapes = [("full", 1024, 4 * bn, 320, 1, BF16), ("ragged", 1000, n_ragged, 640, 1, BF16), ("ragged-f16", 1000, n_ragged, 640, 1, F16),
              ("ragged-2slices", 1000, n_ragged, 640, 2, BF16), ("production", 8192, 1280, 640, 1, BF16), ("production-2", 2048, 1280, 1280, 1, BF16),
              ("production-3-f16", 4096, 640, 640, 1, F16)]
    worst = 0.0
    for name, M, N, K, ks, dtype in shapes:
        a, w, bias, res, rb = _gemm_inputs(M, N, K, dtype, 100)
        for fix in ((0, fix_default) if ks > 1 else (fix_default,)):
            lib().gmd_splitk_fixup_max(fix)
            force_plan(bm, bn, pf, ks)
            assert ops.gemm_plan_info(dtype, M, N, K) == (bm, bn, code, ks), f"{plan} {name}: the override did not select the kernel"
            worst = max(worst, _check_gemm(ops, f"{plan} {name} {M}x{N}x{K} ks={ks} fixup_max={fix}", (bm, bn), a, w, bias, res, rb, 100))
        lib().gmd_splitk_fixup_max(fix_default)
    # batched (grid z = batch index: per-batch operand and output bases) with ldc > N, residual, alpha, on the ragged shape
    Bn, M, N, K = 3, 1000, n_ragged, 640
    ld = N + 24
    g = torch.Generator().manual_seed(Bn + M + N + K)
    a = torch.randn(Bn, M, K, generator=g).bfloat16().to(DEV)
    w = (torch.randn(Bn, N, K, generator=g) / math.sqrt(K)).bfloat16().to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    res = torch.randn(Bn, M, N, generator=g).bfloat16().to(DEV)
    force_plan(bm, bn, pf, 1)
    assert ops.gemm_plan_info(BF16, M, N, K, Bn) == (bm, bn, code, 1), f"{plan} batched: the override did not select the kernel"
    out = torch.full((Bn, M, ld), float("nan"), dtype=BF16, device=DEV)
    ops.gemm_nt(a, w, bias=bias, residual=res, alpha=0.5, out=out, ldc=ld)
    ref_acc = a.double() @ w.double().transpose(1, 2)
    abs_dot = a.double().abs() @ w.double().abs().transpose(1, 2)
    ex = [bias.double().expand_as(ref_acc), res.double()]
    worst = max(worst, P.assert_elementwise(out[:, :, :N], 0.5 * ref_acc + ex[0] + ex[1], P.gemm_bound(ref_acc, abs_dot, K, BF16, 0.5, ex, height=P.mfma_height(K, 32)),
                                            f"{plan} batched x{Bn} ldc={ld}", (bm, bn)))
    assert bool(torch.isnan(out[:, :, N:].float()).all()), f"{plan} batched: padding columns were written"
    _report("gemm16", plan, worst)


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_gemm_batched_with_padded_rows_per_element(dtype):
    """Batched, operand-swapped projection with ldc > N (test_gemm_batched_and_swapped's case): the logical window per element."""
    from gm_diffusion import hip_ops as ops

    g = torch.Generator().manual_seed(9)
    Bn, N, C, ld = 3, 72, 128, 80
    x = torch.randn(Bn, N, C, generator=g).to(dtype).to(DEV)
    wv = (torch.randn(C, C, generator=g) / math.sqrt(C)).to(dtype).to(DEV)
    assert ops.gemm_plan_info(dtype, C, N, C, Bn)[2] == 0
    vt = ops.gemm_nt(wv, x, ldc=ld)
    ref = torch.einsum("ck,bnk->bcn", wv.double(), x.double())
    ad = torch.einsum("ck,bnk->bcn", wv.double().abs(), x.double().abs())
    _report("gemm16", f"batched-ldc {dtype}", P.assert_elementwise(vt[:, :, :N], ref, P.gemm_bound(ref, ad, C, dtype), "batched ldc=80", (64, 64)))


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("plan,M", [("default", 300), ("pp256x128", 2048), ("lc128x128", 1024)])
def test_gemm_geglu_epilogue_per_element(plan, M, dtype, force_plan):
    """value * gelu_erf(gate) on the 16-row interleaved [value | gate] weight rows, written as [M, N / 2]."""
    from gm_diffusion import hip_ops as ops

    g = torch.Generator().manual_seed(11)  # the generators of test_pp_geglu_epilogue_vs_float64
    C = 320
    x = torch.randn(M, C, generator=g).to(dtype).to(DEV)
    w1 = (torch.randn(8 * C, C, generator=g) * 0.05).to(dtype)
    b1 = torch.randn(8 * C, generator=g) * 0.5
    half = 4 * C
    wi = torch.stack([w1[:half].reshape(half // 16, 16, -1), w1[half:].reshape(half // 16, 16, -1)], 1).reshape(2 * half, -1).contiguous().to(DEV)
    bi = torch.stack([b1[:half].reshape(half // 16, 16), b1[half:].reshape(half // 16, 16)], 1).reshape(2 * half).contiguous().to(DEV)
    if plan != "default":
        bm, bn, pf, code = GEMM_PLANS[plan]
        force_plan(bm, bn, pf, 1)
        assert ops.gemm_plan_info(dtype, M, 8 * C, C, 1, True) == (bm, bn, code, 1)
    else:
        bm, bn, code, _ = ops.gemm_plan_info(dtype, M, 8 * C, C, 1, True)
        assert code == 0
    y = ops.gemm_nt(x, wi, bias=bi, act=ops.ACT_GEGLU)
    w1d, b1d = w1.double().to(DEV), b1.double().to(DEV)
    acc = x.double() @ w1d.T
    ad = x.double().abs() @ w1d.abs().T
    val, ev = P.preact_bound(acc[:, :half], ad[:, :half], C, 1.0, [b1d[:half].expand(M, half)])
    gate, eg = P.preact_bound(acc[:, half:], ad[:, half:], C, 1.0, [b1d[half:].expand(M, half)])
    assert y.shape == (M, half)
    _report("gemm16", f"geglu {plan}", P.assert_elementwise(y, val * F.gelu(gate), P.geglu_bound(val, ev, gate, eg, dtype), f"geglu {plan}", (bm, bn // 2)))


# ---------------------------------------------------------------------------------------------------------------------------
# conv3x3
# ---------------------------------------------------------------------------------------------------------------------------
def _conv64(x, w, B, H, W, stride=1, upsample=False, pad_mode=0, out_size=None):
    ci, co = x.shape[-1], w.shape[0]
    xi = x.view(B, H, W, ci).permute(0, 3, 1, 2)
    wt = w.view(co, 3, 3, ci).permute(0, 3, 1, 2)
    if out_size is not None:
        xi = F.interpolate(xi, size=out_size, mode="nearest")
    elif upsample:
        xi = F.interpolate(xi, scale_factor=2, mode="nearest")
    y = F.conv2d(F.pad(xi, (0, 1, 0, 1)), wt, stride=2) if pad_mode == 1 else F.conv2d(xi, wt, stride=stride, padding=1)
    return y.permute(0, 2, 3, 1).reshape(B, -1, co)


CONV_KW = {"s1": dict(), "s2": dict(stride=2), "up": dict(upsample=True), "pad1": dict(stride=2, pad_mode=1), "up_to_odd": dict(out_size=(45, 39))}


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("mode", list(CONV_KW))
@pytest.mark.parametrize("plan", ["default", "pp256x160", "pp256x128", "lc128x160", "lc64x160", "ring128x160"])
def test_conv3x3_every_kernel_per_element(plan, mode, dtype, force_plan):
    """Odd feature map (23 x 20: the division path of the pixel decomposition, ragged B Ho Wo), stride 1 / 2, fused 2x upsample,
    GMD_UPSAMPLE_TO an odd size, the (0,1,0,1) pad; bias + per-sample row bias (seam inside a tile) + residual."""
    from gm_diffusion import hip_ops as ops

    kw = CONV_KW[mode]
    g = torch.Generator().manual_seed(len(mode) + 21)
    B, H, W, ci, co = 3, 23, 20, 128, 320
    x = torch.randn(B, H * W, ci, generator=g).to(dtype).to(DEV)
    w = (torch.randn(co, 9 * ci, generator=g) * 0.03).to(dtype).to(DEV)
    b = torch.randn(co, generator=g).to(DEV)
    tb = torch.randn(B, co, generator=g).to(DEV)
    ref_acc = _conv64(x.double(), w.double(), B, H, W, **kw)
    abs_dot = _conv64(x.double().abs(), w.double().abs(), B, H, W, **kw)
    r = torch.randn(ref_acc.shape, generator=g).to(dtype).to(DEV)
    M = ref_acc.shape[0] * ref_acc.shape[1]
    if plan != "default":
        bm, bn, pf, code = GEMM_PLANS[plan]
        force_plan(bm, bn, pf, 1)
        assert ops.gemm_plan_info(dtype, M, co, 9 * ci) == (bm, bn, code, 1)
    else:
        bm, bn = ops.gemm_plan_info(dtype, M, co, 9 * ci)[:2]
    y, ho, wo = ops.conv3x3(x, w, B, H, W, bias=b, rowbias=tb, residual=r, **kw)
    ex = [b.double().expand_as(ref_acc), tb.double()[:, None, :].expand_as(ref_acc), r.double()]
    assert y.shape == ref_acc.shape
    rr = P.assert_elementwise(y.reshape(M, co), (ref_acc + ex[0] + ex[1] + ex[2]).reshape(M, co),
                              P.gemm_bound(ref_acc, abs_dot, 9 * ci, dtype, 1.0, ex).reshape(M, co), f"conv {plan} {mode} {dtype}", (bm, bn))
    _report("conv3x3", f"{plan} {mode} {dtype}", rr)


@pytest.mark.parametrize("patch", [0, 1, 2])
def test_conv3x3_patch_modes_per_element(patch, force_plan):
    """Each gmd_conv_patch_override mode of the stride-1 convolution on 256-row ping-pong tiles, at a production shape (64 x 64,
    320 -> 320, batch 2)."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    g = torch.Generator().manual_seed(5)
    B, H, ci, co = 2, 64, 320, 320
    x = torch.randn(B, H * H, ci, generator=g).bfloat16().to(DEV)
    w = (torch.randn(co, 9 * ci, generator=g) * 0.02).bfloat16().to(DEV)
    b = torch.randn(co, generator=g).to(DEV)
    force_plan(256, 160, 283, 1)
    assert lib().gmd_conv_patch_override(patch) == 0
    assert ops.gemm_plan_info(BF16, B * H * H, co, 9 * ci) == (256, 160, 283, 1)
    y, _, _ = ops.conv3x3(x, w, B, H, H, bias=b)
    ref_acc = _conv64(x.double(), w.double(), B, H, H)
    abs_dot = _conv64(x.double().abs(), w.double().abs(), B, H, H)
    ex = [b.double().expand_as(ref_acc)]
    M = B * H * H
    _report("conv3x3", f"patch mode {patch}", P.assert_elementwise(y.reshape(M, co), (ref_acc + ex[0]).reshape(M, co),
                                                                   P.gemm_bound(ref_acc, abs_dot, 9 * ci, BF16, 1.0, ex).reshape(M, co), f"conv patch mode {patch}", (256, 160)))


# ---------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------
def _heads(t, heads):
    B, N, C = t.shape
    return t.reshape(B, N, heads, C // heads).transpose(1, 2)


def _check_attention(ops, q, k, v, heads, scale, what, causal=False, family="attention"):
    B, Nq, C = q.shape
    Nk, D = k.shape[1], C // heads
    ld = (Nk + 7) // 8 * 8
    vt = torch.full((B, C, ld), float("nan"), dtype=q.dtype, device=DEV)  # pad columns poisoned: the kernel must mask them
    vt[:, :, :Nk] = v.transpose(1, 2)
    got = ops.attention(q, k, vt, heads, Nk, scale, causal=causal)
    ref, bound = P.attention_bound(_heads(q, heads), _heads(k, heads), _heads(v, heads), scale, q.dtype, causal=causal)
    return _report(family, what, P.assert_elementwise(_heads(got, heads), ref, bound, what, (32, D)))


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D", [32, 40, 64, 80, 160])
def test_attention_every_head_dim_per_element(D, dtype):
    """One kernel instantiation per (head dim, element type) -- gmd_attention dispatches on exactly these two, so the head dim IS
    the kernel -- over key counts that end inside a tile (1, 7, 77, 130, 203) and on its edge (1024), query counts that are not a
    multiple of the 128-row query block."""
    from gm_diffusion import hip_ops as ops

    heads, B = 2, 2
    for Nq, Nk in [(16, 1), (200, 7), (64, 77), (200, 130), (333, 203), (1024, 1024)]:
        g = torch.Generator().manual_seed(D * 7 + Nq + Nk)  # the generators of test_attention_bf16
        q, k, v = (torch.randn(B, n, heads * D, generator=g).to(dtype).to(DEV) for n in (Nq, Nk, Nk))
        _check_attention(ops, q, k, v, heads, D ** -0.5, f"D={D} {dtype} Nq={Nq} Nk={Nk}")


@pytest.mark.parametrize("spike", [1.5, 3.0, 8.0])
def test_attention_spiked_keys_per_element(spike):
    """Both rescale branches of the lagged stabiliser (test_attention_rescale_branch_spiked_keys's generator)."""
    from gm_diffusion import hip_ops as ops

    D, N = 40, 320
    g = torch.Generator().manual_seed(77)
    q = torch.randn(1, N, D, generator=g)
    k = torch.randn(1, N, D, generator=g) * 0.3
    v = torch.randn(1, N, D, generator=g)
    k[0, 200] = q[0, 5] * spike
    k[0, 310] = q[0, 100] * (spike + 1.0)
    q, k, v = (t.bfloat16().to(DEV) for t in (q, k, v))
    _check_attention(ops, q, k, v, 1, D ** -0.5, f"spike {spike}")


@pytest.mark.parametrize("D", [40, 80])
def test_attention_all_negative_rows_per_element(D):
    from gm_diffusion import hip_ops as ops

    heads, N = 2, 200
    g = torch.Generator().manual_seed(D)  # test_attention_large_and_negative_logits's generator
    base = torch.randn(1, 1, heads * D, generator=g)
    q = base * 4.0 + 0.3 * torch.randn(1, N, heads * D, generator=g)
    k = -base * 4.0 + 0.3 * torch.randn(1, N, heads * D, generator=g)
    v = torch.randn(1, N, heads * D, generator=g)
    q, k, v = (t.bfloat16().to(DEV) for t in (q, k, v))
    _check_attention(ops, q, k, v, heads, D ** -0.5, f"all-negative D={D}")


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D,N", [(64, 77), (32, 77), (64, 200)])
def test_attention_causal_per_element(D, N, dtype):
    from gm_diffusion import hip_ops as ops

    heads = 2
    g = torch.Generator().manual_seed(D + N)
    q, k, v = (torch.randn(2, N, heads * D, generator=g).to(dtype).to(DEV) for _ in range(3))
    _check_attention(ops, q, k, v, heads, D ** -0.5, f"causal D={D} N={N} {dtype}", causal=True)


# ---------------------------------------------------------------------------------------------------------------------------
# GroupNorm / LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("B,HW,C,G,path", [(2, 64, 320, 32, "fused"), (2, 256, 1280, 32, "fused"), (3, 37, 64, 8, "fused"),
                                           (1, 4163, 320, 32, "split"), (4, 4100, 320, 32, "split"), (5, 4100, 320, 32, "split"),
                                           (8, 4100, 320, 32, "split"), (2, 3300, 640, 32, "split")])
def test_groupnorm_per_element(B, HW, C, G, path, dtype):
    """The single-launch kernel and the split path (every U instantiation of the apply pass with a ragged last workgroup:
    test_groupnorm_apply_pass_every_vector_count_and_ragged_ends's shapes), three element types.  ``height`` of the bound: a thread
    of the fused kernel sums HW (C / G) / 256 elements, a thread of the split path's partial kernel at most the HW / nsplit rows of
    its block (csrc/norm.hip), each followed by tree stages and folds counted as 16."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    g = torch.Generator().manual_seed(C + HW)
    x = (torch.randn(B, HW, C, generator=g) * 2 + 0.5).to(dtype).to(DEV)
    gamma, beta = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    cpg = C // G
    vec16 = (cpg * x.element_size()) % 16 == 0 and (C * x.element_size()) % 16 == 0
    fused = HW * cpg * x.element_size() <= (ops.GN_FUSED_MAX_SLAB_VEC16 if vec16 else ops.GN_FUSED_MAX_SLAB)
    assert fused == (path == "fused"), "the wrapper's dispatch rule moved: this case no longer exercises the kernel it names"
    if fused:
        height = -(-HW * cpg // 256) + 16
    else:
        height = -(-HW // lib().gmd_groupnorm_nsplit(HW)) + 16
    for silu in (False, True):
        got = ops.groupnorm(x, B, G, gamma, beta, 1e-5, silu=silu)
        ref, bound = P.groupnorm_ref_bound(x, G, gamma, beta, 1e-5, dtype, height, silu)
        _report("groupnorm", f"{path} {B}x{HW}x{C} {dtype} silu={silu}", P.assert_elementwise(got, ref, bound, f"groupnorm {path} {dtype} silu={silu}", (64, 8)))
    got = ops.groupnorm_split(x, B, G, gamma, beta, 1e-5, silu=True)  # statistics + finalize + apply launches
    ref, bound = P.groupnorm_ref_bound(x, G, gamma, beta, 1e-5, dtype, -(-HW // lib().gmd_groupnorm_nsplit(HW)) + 16, True)
    _report("groupnorm", f"three-launch {B}x{HW}x{C} {dtype}", P.assert_elementwise(got, ref, bound, f"groupnorm three-launch {dtype}", (64, 8)))


def _layernorm_branch(dtype, rows, C, aligned):
    """The launcher branch gmd_layernorm takes (csrc/norm.hip)."""
    if dtype == F32:
        return "wave<8,1>"
    if aligned and C == 320:
        return "packed<8,5>"
    if aligned and C == 640:
        return "packed<16,5>"
    if C <= 512 and rows >= 8192:
        return "wave<1,4>"  # four rows per wave
    if C <= 1024 and rows >= 4096:
        return "wave<2,2>"  # two rows per wave
    return "wave<4,1>"


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("rows,C,aligned,branch16", [
    (5, 320, True, "packed<8,5>"), (4099, 320, True, "packed<8,5>"), (130, 640, True, "packed<16,5>"), (1031, 640, True, "packed<16,5>"),
    (64, 1280, True, "wave<4,1>"), (3, 64, True, "wave<4,1>"), (9, 2048, True, "wave<4,1>"),
    (8200, 64, True, "wave<1,4>"), (8197, 512, True, "wave<1,4>"), (4100, 960, True, "wave<2,2>"), (4099, 1024, True, "wave<2,2>"),
    (8197, 320, False, "wave<1,4>"), (4099, 640, False, "wave<2,2>"), (131, 320, False, "wave<4,1>"),
])
def test_layernorm_per_element(rows, C, aligned, branch16, dtype):
    """Every launcher branch of gmd_layernorm for the 16-bit types (``branch16``; float32 has the one wave<8,1> kernel): the packed
    kernels (C = 320 / 640 with 16-byte aligned gamma / beta), one, two and four rows per wave, with row counts that end inside a
    wave's group of rows (_layernorm_branch mirrors the launcher at csrc/norm.hip, gmd_layernorm: a change of its branch order has
    to be mirrored there -- the ABI has no query for it); ``aligned=False`` hands over gamma / beta 4 bytes off a 16-byte boundary, which takes 320 / 640 off the
    packed kernels.  height of the bound: a lane sums at most C / 8 elements, plus the DPP tree."""
    from gm_diffusion import hip_ops as ops

    assert _layernorm_branch(dtype, rows, C, aligned) == ("wave<8,1>" if dtype == F32 else branch16)
    g = torch.Generator().manual_seed(rows)
    x = (torch.randn(rows, C, generator=g) * 3 - 1).to(dtype).to(DEV)
    off = 0 if aligned else 1
    gamma, beta = torch.randn(C + 4, generator=g).to(DEV)[off:off + C], torch.randn(C + 4, generator=g).to(DEV)[off:off + C]
    assert (gamma.data_ptr() % 16 == 0) == aligned and (beta.data_ptr() % 16 == 0) == aligned and gamma.is_contiguous()
    got = ops.layernorm(x, gamma, beta, 1e-5)
    ref, bound = P.layernorm_ref_bound(x, gamma, beta, 1e-5, dtype, C // 8 + 8)
    _report("layernorm", f"{rows}x{C} {dtype} {branch16}", P.assert_elementwise(got, ref, bound, f"layernorm {rows}x{C} {dtype}", (8, 8)))


# ---------------------------------------------------------------------------------------------------------------------------
# float32 GEMM: the three-product split (F32S / F32SW / F32SA) and the exact kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["F32S", "F32SW", "F32SA-operand", "F32SA-output", "F32-exact"])
@pytest.mark.parametrize("M,N,K", [(1024, 640, 640), (300, 200, 320), (2048, 1280, 1280), (8192, 640, 640)])
def test_gemm_float32_per_element(M, N, K, mode):
    """gemm_nt on float32 tensors: in-kernel split of both operands (GMD_F32S), pre-split scaled weights (F32SW), pre-split
    activation operand (F32SA), a pre-split OUTPUT read back through the documented layout (parity.unsplit), and the exact float32
    kernel.  The dtype code the wrapper hands to the C ABI is asserted (the plan query covers the 16-bit types only)."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    ex = [bias.double().expand(M, N)]
    if mode == "F32-exact":
        with ops.f32_mode_scope("exact"):
            assert ops._contract_code(a, w, K) == ops.GMD_F32
            got = ops.gemm_nt(a, w, bias=bias)
        ref_acc, ad = a.double() @ w.double().T, a.double().abs() @ w.double().abs().T
        bound = P.gemm_bound(ref_acc, ad, K, F32, 1.0, ex, product_err=P.U_F32 * ad)
        return _report("gemm32", f"{mode} {M}x{N}x{K}", P.assert_elementwise(got, ref_acc + ex[0], bound, f"{mode} {M}x{N}x{K}", (64, 64)))
    with ops.f32_mode_scope("split"):
        if mode == "F32S":
            weff, alpha = w, 1.0
            assert ops._contract_code(a, w, K) == ops.GMD_F32S
            got = ops.gemm_nt(a, w, bias=bias)
        else:
            weff = ops.scale_weight(w)
            alpha = weff._alpha
            ws = ops.split_weights(w)
            a_op = ops.split_activation(a) if mode == "F32SA-operand" else a
            assert ops._contract_code(a_op, ws, K, ops.is_asplit(a_op)) == (ops.GMD_F32SA if mode == "F32SA-operand" else ops.GMD_F32SW)
            got = ops.gemm_nt(a_op, ws, bias=bias, split_out=mode == "F32SA-output")
    ref_acc, ad = a.double() @ weff.double().T, a.double().abs() @ weff.double().abs().T
    # three instructions of 32 products per k-block through one accumulator (csrc/gemm_split.hip); up to 16 K slices
    bound = P.gemm_bound(ref_acc, ad, 3 * K, F32, alpha, ex, product_err=P.split_product_bound(a, weff), height=P.mfma_height(3 * K, 32, 16))
    ref = alpha * ref_acc + ex[0]
    if mode == "F32SA-output":
        can = bool(lib().gmd_gemm_out_split_ok(M, N, K, 0, ops.WORKSPACE_BYTES)) and N % 32 == 0
        assert ops.is_asplit(got) == can, "gmd_gemm_out_split_ok and the wrapper disagree"
        # only an unsplit launch of full 128-row tiles stores pre-split: of these shapes the one that fills the chip with them
        assert can == (M == 8192), "the split plan moved: re-pick the shape that stores a pre-split output"
        if can:  # read hi + lo back: the split's residual on top (2^-22 |x| + 2^-25, split_product_bound's r_x)
            got = P.unsplit(got)
            bound = bound + 2.0 ** -22 * (ref.abs() + bound) + 2.0 ** -25
    _report("gemm32", f"{mode} {M}x{N}x{K}", P.assert_elementwise(got, ref, bound, f"{mode} {M}x{N}x{K}", (64, 64)))


def test_unsplit_reads_the_documented_layout():
    from gm_diffusion import hip_ops as ops

    x = torch.randn(37, 96, generator=torch.Generator().manual_seed(1)).to(DEV) * 64
    back = P.unsplit(ops.split_activation(x))
    hi, lo = P.split_parts(x)
    assert torch.equal(back, hi.double() + lo.double())


# ---------------------------------------------------------------------------------------------------------------------------
# fused launches
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("B,tokens,C", [(8, 1024, 640), (8, 4096, 320), (8, 256, 1280)])
def test_gemm_qkv_vt_per_element(B, tokens, C, dtype):
    """gmd_gemm_qkv_vt: the row-major Q|K part and the transposed V tiles, each element against float64."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    g = torch.Generator().manual_seed(B + tokens + C)  # test_fused_qkv_projection_writes_v_transposed's generator
    n = torch.randn(B * tokens, C, generator=g).to(DEV, dtype)
    w = torch.cat([(torch.randn(C, C, generator=g) * C ** -0.5).to(DEV, dtype) for _ in range(3)], 0).contiguous()
    assert lib().gmd_gemm_qkv_vt_ok(ops.dtype_code(dtype), B * tokens, 3 * C, C, 2 * C, tokens, ops.WORKSPACE_BYTES), "the fused launch is not taken: no kernel exercised"
    bm, bn = ops.gemm_plan_info(dtype, B * tokens, 3 * C, C)[:2]
    qk, vt = ops.gemm_qkv_vt(n, w, 2 * C, tokens)
    ref = n.double() @ w.double().T
    bound = P.gemm_bound(ref, n.double().abs() @ w.double().abs().T, C, dtype)
    r1 = P.assert_elementwise(qk, ref[:, :2 * C], bound[:, :2 * C], "qkv_vt row-major part", (bm, bn))
    tr = lambda t: t[:, 2 * C:].reshape(B, tokens, C).transpose(1, 2)
    r2 = P.assert_elementwise(vt, tr(ref), tr(bound), "qkv_vt transposed V", (bn, bm))
    _report("gemm16", f"qkv_vt {B}x{tokens}x{C} {dtype}", max(r1, r2))


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("M", [128, 4096])
def test_ff_geglu_fused_per_element(M, dtype):
    """gmd_ff_geglu_fused: Y = round16(value gelu(gate)) W2^T + b2 + residual.  The bound composes geglu_bound of the on-chip [M, 4C]
    tensor (rounded once to the 16-bit type) with gemm_bound of the second product: the first stage's error e_h enters as a
    per-product error e_h |W2|^T and widens the magnitudes the accumulation term sees."""
    from gm_diffusion import hip_ops as ops

    C, half = 320, 1280
    g = torch.Generator().manual_seed(M)  # test_ff_geglu_fused_matches_two_gemms_and_float64's generator
    x = torch.randn(M, C, generator=g).to(dtype).to(DEV)
    res = torch.randn(M, C, generator=g).to(dtype).to(DEV)
    wf = (torch.randn(8 * C, C, generator=g) / math.sqrt(C)).to(dtype).to(DEV)
    bf = (torch.randn(8 * C, generator=g) * 0.2).to(DEV)
    w2 = (torch.randn(C, 4 * C, generator=g) / math.sqrt(4 * C)).to(dtype).to(DEV)
    b2 = (torch.randn(C, generator=g) * 0.2).to(DEV)
    wi = torch.stack([wf[:half].reshape(half // 16, 16, -1), wf[half:].reshape(half // 16, 16, -1)], 1).reshape(2 * half, -1).contiguous()
    bi = torch.stack([bf[:half].reshape(half // 16, 16), bf[half:].reshape(half // 16, 16)], 1).reshape(2 * half).contiguous()
    assert ops.ff_fused_ok(x, C, min_rows=0)
    got = ops.ff_geglu_fused(x, wi, bi, w2, b2, res)
    acc, ad = x.double() @ wf.double().T, x.double().abs() @ wf.double().abs().T
    val, ev = P.preact_bound(acc[:, :half], ad[:, :half], C, 1.0, [bf.double()[:half].expand(M, half)])
    gate, eg = P.preact_bound(acc[:, half:], ad[:, half:], C, 1.0, [bf.double()[half:].expand(M, half)])
    h, eh = val * F.gelu(gate), P.geglu_bound(val, ev, gate, eg, dtype)
    w2a = w2.double().abs()
    ex = [b2.double().expand(M, C), res.double()]
    bound = P.gemm_bound(h @ w2.double().T, (h.abs() + eh) @ w2a.T, 4 * C, dtype, 1.0, ex, product_err=eh @ w2a.T)
    _report("gemm16", f"ff_geglu_fused {M} {dtype}", P.assert_elementwise(got, h @ w2.double().T + ex[0] + ex[1], bound, f"ff_geglu_fused M={M} {dtype}", (128, 320)))


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_conv3x3_groupnorm_per_element(dtype):
    """gmd_conv3x3_groupnorm on an 8x8 level (split-K slabs summed by the GroupNorm kernel): Yraw against the float64 convolution,
    Ynorm against float64 GroupNorm + SiLU of the STORED raw tensor (the kernel normalises the rounded values)."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    B, H, ci, co, G = 8, 8, 1280, 1280, 32
    g = torch.Generator().manual_seed(B * 1000 + H + ci + co)
    x = torch.randn(B, H * H, ci, generator=g).to(DEV, dtype)
    w = (torch.randn(co, 9 * ci, generator=g) / math.sqrt(9 * ci)).to(DEV, dtype)
    bias = torch.randn(co, generator=g).to(DEV)
    tb = torch.randn(B, co, generator=g).to(DEV)
    res = torch.randn(B, H * H, co, generator=g).to(DEV, dtype)
    gamma, beta = torch.randn(co, generator=g).to(DEV), torch.randn(co, generator=g).to(DEV)
    assert lib().gmd_conv3x3_gn_fusable(ops.dtype_code(dtype), B, H, H, ci, co, 1, 0, 0, G, ops.WORKSPACE_BYTES), "not the fused launch"
    assert ops.gemm_plan_info(dtype, B * H * H, co, 9 * ci)[3] > 1
    yr, yn = ops.conv3x3_groupnorm(x, w, B, H, H, G, gamma, beta, 1e-5, silu=True, bias=bias, rowbias=tb, residual=res, want_raw=True)
    ref_acc = _conv64(x.double(), w.double(), B, H, H)
    abs_dot = _conv64(x.double().abs(), w.double().abs(), B, H, H)
    ex = [bias.double().expand_as(ref_acc), tb.double()[:, None, :].expand_as(ref_acc), res.double()]
    bm, bn = ops.gemm_plan_info(dtype, B * H * H, co, 9 * ci)[:2]
    r1 = P.assert_elementwise(yr.reshape(-1, co), (ref_acc + ex[0] + ex[1] + ex[2]).reshape(-1, co),
                              P.gemm_bound(ref_acc, abs_dot, 9 * ci, dtype, 1.0, ex).reshape(-1, co), f"conv3x3_groupnorm Yraw {dtype}", (bm, bn))
    ref, bound = P.groupnorm_ref_bound(yr, G, gamma, beta, 1e-5, dtype, -(-H * H * (co // G) // 256) + 16, True)
    r2 = P.assert_elementwise(yn, ref, bound, f"conv3x3_groupnorm Ynorm {dtype}", (64, 8))
    _report("conv3x3", f"conv3x3_groupnorm {dtype}", max(r1, r2))


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_groupnorm_from_producer_colstats_per_element(dtype):
    """gmd_groupnorm_colstats: one pass over X with the {sum, sum of squares} its producer left per 64 rows x 10 channels.  height of
    the bound: 32 rows summed serially per column strip, two strip adds, a bucket fold of 10 (csrc/gemm_shared.h colstats_pass /
    colstats_store): 44 float32 additions at most; the folds over row blocks run in double."""
    from gm_diffusion import hip_ops as ops

    B, H, ci, co, G = 8, 64, 320, 320, 32
    g = torch.Generator().manual_seed(3)  # test_pp_column_statistics_feed_groupnorm's generator
    x = torch.randn(B, H * H, ci, generator=g).to(dtype).to(DEV)
    w = (torch.randn(co, 9 * ci, generator=g) * 0.02).to(dtype).to(DEV)
    b = torch.randn(co, generator=g).to(DEV)
    gamma, beta = torch.randn(co, generator=g).to(DEV), torch.randn(co, generator=g).to(DEV)
    y, _, _ = ops.conv3x3(x, w, B, H, H, bias=b, colstats=True)
    assert getattr(y, "_colstats", None) is not None, "the producer left no statistics: gmd_groupnorm_colstats is not exercised"
    before = ops.colstats_uses
    for silu in (False, True):
        got = ops.groupnorm(y, B, G, gamma, beta, 1e-5, silu=silu)
        ref, bound = P.groupnorm_ref_bound(y, G, gamma, beta, 1e-5, dtype, 44 + 2, silu)
        _report("groupnorm", f"colstats {dtype} silu={silu}", P.assert_elementwise(got, ref, bound, f"groupnorm colstats {dtype}", (64, 10)))
    assert ops.colstats_uses == before + 2


# ---------------------------------------------------------------------------------------------------------------------------
# attention: float32 split kernel, fused Q|K buffer
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [40, 64, 80, 160])
def test_attention_split_float32_per_element(D):
    from gm_diffusion import hip_ops as ops

    heads, B = 2, 2
    with ops.f32_mode_scope("split"):
        assert ops.split_attention_ok(F32, D)
        for Nq, Nk in [(200, 7), (64, 77), (333, 203), (512, 1024)]:
            g = torch.Generator().manual_seed(D * 7 + Nq + Nk)
            q, k, v = (torch.randn(B, n, heads * D, generator=g).to(DEV) for n in (Nq, Nk, Nk))
            ld = (Nk + 7) // 8 * 8
            vt = torch.full((B, heads * D, ld), float("nan"), device=DEV)
            vt[:, :, :Nk] = v.transpose(1, 2)
            got = ops.attention(q, k, vt, heads, Nk, D ** -0.5)
            ref, bound = P.attention_split_bound(_heads(q, heads), _heads(k, heads), _heads(v, heads), D ** -0.5)
            _report("attention32", f"D={D} Nq={Nq} Nk={Nk}", P.assert_elementwise(_heads(got, heads), ref, bound, f"split attention D={D} Nk={Nk}", (32, D)))


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D", [40, 64])
def test_attention_fused_qk_buffer_per_element(D, dtype):
    """Q and K read from ONE [B, N, 2 H D] buffer (k_col = H D): the row stride differs from H D (test_attention_fused_qk_buffer)."""
    from gm_diffusion import hip_ops as ops

    heads, B, N = 8, 2, 256
    C = heads * D
    g = torch.Generator().manual_seed(5)
    qk = torch.randn(B, N, 2 * C, generator=g).to(dtype).to(DEV)
    v = torch.randn(B, N, C, generator=g).to(dtype).to(DEV)
    got = ops.attention(qk, qk, v.transpose(1, 2).contiguous(), heads, N, D ** -0.5, k_col=C)
    ref, bound = P.attention_bound(_heads(qk[:, :, :C], heads), _heads(qk[:, :, C:], heads), _heads(v, heads), D ** -0.5, dtype)
    _report("attention", f"fused-qk D={D} {dtype}", P.assert_elementwise(_heads(got, heads), ref, bound, f"fused qk D={D} {dtype}", (32, D)))
