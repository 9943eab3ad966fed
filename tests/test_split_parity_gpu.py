"""Per-element parity of the float32 matrix-core path (csrc/gemm_split.hip, csrc/attention_split.hip, the slab reducer, the
transposed-V / pre-split-output / GEGLU epilogues, the implicit-GEMM conv3x3) against float64 torch on the device: a derived bound for
every element (tests/parity.py), zero violations allowed.  This path is the accuracy anchor of the oracle-golden and 16-bit drift
tests, so a wrong fragment here moves their yardstick.  Every case first asserts, through gmd_split_plan_info, the kernel it names,
and prints ``PARITY gemm32|conv32|attention32 <case> max|err|/bound=<r>`` (pytest -s).  tests/test_split_parity_cpu.py shows that
the bounds used here report a dropped product, a skipped K step, a wrong conv tap, a stale slab row and a hi/lo swap.

What the asserted plans cover (tile shape, ragged / full, K slices, kernel):

    case                                        tiles     edge     slices  kernel                 operand forms
    gemm  128x160 full / ragged in M            128x160   f / r    1       ring                   F32S F32SW F32SA
    gemm  128x128 full / ragged in both         128x128   f / r    1       ring                   F32S F32SW F32SA
    gemm  64x64 ragged                          64x64     r        1       ring                   F32S F32SW F32SA
    gemm  slabs 128x160 / 128x128 (+ ragged)    128-row   f / r    5, 3, 5 ring + reducer         F32S F32SW F32SA
    gemm  slabs 64x64                           64x64     f        4       ring + reducer         F32S F32SW F32SA
    gemm  reducer second lap                    128x160   f        2       ring + reducer, 2 laps F32SW
    gemm  batched, swapped (ldc > N)            64x64     r        1       ring, grid z = batch   F32S
    gemm  GEGLU 300 / 4096 (+ pre-split out)    64 / 128  r / f    1       ring, GEGLU epilogues  F32S F32SW F32SA
    gemm  qkv_vt                                160 / 128 f        1       ring, transposed V     F32SW F32SA
    conv  25 pairwise rows + 5 exact-mode legs  all three f / r    1, 4    ring (CONV)            F32S F32SW F32SA, F32
    conv  + GroupNorm over slabs                128x160   f        5       ring + GroupNorm       F32SW
    gemm / conv loader-converter                128-row   r        1       lc, TN 5 and TN 4      F32SW
    attention (split_out, fused Q|K, spikes)    --        --       --      attn_split_kernel      D 40 64 80 160"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import parity as P
import split_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32


@pytest.fixture(autouse=True)
def split_mode():
    from gm_diffusion import hip_ops as ops

    prev = ops.set_f32_mode("split")
    yield
    ops.set_f32_mode(prev)


def _report(family, case, r):
    print(f"PARITY {family} {case} max|err|/bound={r:.3f}")
    return r


def _operands(ops, form, a, w):
    """(A operand, W operand, effective weight, the weight's alpha) of one operand form; the wrapper's dtype code is asserted."""
    if form == "F32S":
        a_op, w_op, weff, alpha_w = a, w, w, 1.0
    else:
        weff = ops.scale_weight(w)
        alpha_w = weff._alpha
        w_op = ops.split_weights(w)
        a_op = ops.split_activation(a.reshape(-1, a.shape[-1])).reshape(a.shape) if form == "F32SA" else a
        if form == "F32SA":
            ops._mark_asplit(a_op)
    assert ops._contract_code(a_op, w_op, a.shape[-1], ops.is_asplit(a_op)) == S.FORM_CODE[form]
    return a_op, w_op, weff, alpha_w


def _assert_plan(ops, form, M, N, K, plan, what, batch=1, geglu=False, code=0):
    bm, bn, ks = plan
    got = ops.split_plan_info(S.FORM_CODE[form], M, N, K, batch, geglu)
    assert got == (bm, bn, code, ks), f"{what}: planned {got}, the case names {(bm, bn, code, ks)}: re-pick the shape"


def _run_gemm_epilogues(ops, what, tile, a_op, w_op, core, alpha_w, bias, rb, rpg, res, epilogues):
    M, N = core.ref_acc.shape
    worst = 0.0
    for epi in epilogues:
        use_b, use_rb, use_res, alpha, act = S.EPILOGUES[epi]
        extras, _, _ = S.extras_of(epi, bias, rb, rpg, res, (M, N))
        kw = dict(alpha=alpha, act={None: ops.ACT_NONE, "silu": ops.ACT_SILU, "quick_gelu": ops.ACT_QUICK_GELU}[act])
        if use_b:
            kw["bias"] = bias
        if use_rb:
            kw.update(rowbias=rb, rows_per_group=rpg)
        if use_res:
            kw["residual"] = res
        got = ops.gemm_nt(a_op, w_op, **kw)
        assert got.dtype == F32 and got.shape == (M, N)
        ref, bound = S.ref_and_bound(core, alpha * alpha_w, extras, act)
        worst = max(worst, P.assert_elementwise(got, ref, bound, f"{what} {epi}", tile))
    return worst


@pytest.mark.parametrize("form", S.FORMS)
@pytest.mark.parametrize("case", list(S.GEMM_CASES))
def test_gemm_split_every_tile_shape_per_element(case, form):
    """The three instantiations of gemm_split_kernel, full and ragged tiles, unsplit and through slabs + splitk_reduce_f32_kernel,
    each with the four epilogue variants (the row-bias seam inside a tile)."""
    from gm_diffusion import hip_ops as ops

    M, N, K, plan = S.GEMM_CASES[case]
    _assert_plan(ops, form, M, N, K, plan, case)
    a, w, bias, res, rb, rpg = S.gemm_inputs(M, N, K, DEV)
    a_op, w_op, weff, alpha_w = _operands(ops, form, a, w)
    core = S.Core(a, weff, plan[2])
    r = _run_gemm_epilogues(ops, f"{case} {form} {M}x{N}x{K}", plan[:2], a_op, w_op, core, alpha_w, bias, rb, rpg, res, list(S.EPILOGUES))
    _report("gemm32", f"{case} {form}", r)


def test_gemm_split_reducer_second_lap_per_element():
    """splitk_reduce_f32_kernel is launched with min(ceil(M ceil(N / 4) / 256), 4096) workgroups of 256 threads, one thread per four
    columns of a row (launch_split_any: ``if (g > 4096) g = 4096``): 4096 x 256 = 1,048,576 threads cover 4,194,304 outputs, and thread
    i comes back for element i + 1,048,576.  At N = 1280 (320 threads per row) the second lap starts at row 3276, column 1024, and
    holds the last 819.2 rows of the 4096 -- the batch-8 32x32 up-block convolution's GEMM shape, the one production launch that gets
    there (tests/test_small_kernels_cpu.py quotes the cap from the source)."""
    from gm_diffusion import hip_ops as ops

    case, M, N, K, plan = S.SECOND_LAP
    form = "F32SW"
    _assert_plan(ops, form, M, N, K, plan, case)
    lap = S.reducer_lap_start(M, N)
    assert lap == (3276, 1024) and M * N > 4 * S.LAP_REDUCE
    a, w, bias, res, rb, rpg = S.gemm_inputs(M, N, K, DEV)
    a_op, w_op, weff, alpha_w = _operands(ops, form, a, w)
    core = S.Core(a, weff, plan[2])
    epi = "bias+rowbias+residual"
    extras, alpha, act = S.extras_of(epi, bias, rb, rpg, res, (M, N))
    got = ops.gemm_nt(a_op, w_op, bias=bias, rowbias=rb, rows_per_group=rpg, residual=res, alpha=alpha)
    ref, bound = S.ref_and_bound(core, alpha * alpha_w, extras, act)
    second = torch.zeros(M, N, dtype=torch.bool, device=DEV)
    second[lap[0] + 1:] = True
    second[lap[0], lap[1]:] = True
    assert int(second.sum()) == M * N - 4 * S.LAP_REDUCE
    bad = P.violations(got, ref, bound)[0]
    assert int((bad & second).sum()) == 0, f"{int((bad & second).sum())} elements of the reducer's SECOND lap are outside their bound"
    _report("gemm32", f"{case} {form}", P.assert_elementwise(got, ref, bound, f"{case} {M}x{N}x{K}", plan[:2]))


def test_gemm_split_batched_and_swapped_per_element():
    """test_split_batched_and_swapped's two cases (grid z = batch index, per-batch operand and output bases, no workspace) with
    ldc > N: the logical window per element, the padding columns keep their NaN fill."""
    from gm_diffusion import hip_ops as ops

    g = torch.Generator().manual_seed(9)
    Bn, N, C = 3, 72, 128
    x = torch.randn(Bn, N, C, generator=g).to(DEV)
    wv = (torch.randn(C, C, generator=g) / math.sqrt(C)).to(DEV)
    h = P.mfma_height(3 * C, 32, 1)
    worst = 0.0
    # V^T[b] = W_v x[b]^T: the weight is the (shared) A operand, the activation the batched W operand
    _assert_plan(ops, "F32S", C, N, C, (64, 64, 1), "swapped", batch=Bn)
    ld = 80
    out = torch.full((Bn, C, ld), float("nan"), device=DEV)
    ops.gemm_nt(wv, x, out=out, ldc=ld)
    ref = torch.einsum("ck,bnk->bcn", wv.double(), x.double())
    ad = torch.einsum("ck,bnk->bcn", wv.double().abs(), x.double().abs())
    perr = torch.stack([P.split_product_bound(wv, x[b]) for b in range(Bn)])
    bound = P.gemm_bound(ref, ad, 3 * C, F32, 1.0, (), product_err=perr, height=h)
    worst = max(worst, P.assert_elementwise(out[:, :, :N], ref, bound, "swapped batched ldc=80", (64, 64)))
    assert bool(torch.isnan(out[:, :, N:]).all()), "swapped batched: padding columns were written"
    # y[b] = x[b] W_b^T with one weight per batch entry
    wb = torch.stack([wv, wv * 2, wv * 3]).contiguous()
    _assert_plan(ops, "F32S", N, C, C, (64, 64, 1), "batched", batch=Bn)
    ld = C + 8
    out = torch.full((Bn, N, ld), float("nan"), device=DEV)
    ops.gemm_nt(x, wb, out=out, ldc=ld)
    ref = torch.einsum("bnk,bck->bnc", x.double(), wb.double())
    ad = torch.einsum("bnk,bck->bnc", x.double().abs(), wb.double().abs())
    perr = torch.stack([P.split_product_bound(x[b], wb[b]) for b in range(Bn)])
    bound = P.gemm_bound(ref, ad, 3 * C, F32, 1.0, (), product_err=perr, height=h)
    worst = max(worst, P.assert_elementwise(out[:, :, :C], ref, bound, "batched ldc=136", (64, 64)))
    assert bool(torch.isnan(out[:, :, C:]).all()), "batched: padding columns were written"
    _report("gemm32", "batched and swapped", worst)


@pytest.mark.parametrize("form", S.FORMS)
@pytest.mark.parametrize("M,plan", [(300, (64, 64, 1)), (4096, (128, 128, 1))])
def test_gemm_split_geglu_per_element(M, plan, form):
    """value * gelu_erf(gate) on the 16-row interleaved [value | gate] weight rows: ragged 64x64 tiles from registers (M = 300) and
    full 128x128 tiles through the LDS row epilogue (M = 4096), plain and pre-split weights, plain and pre-split operand; where the
    plan can store its output pre-split (gmd_gemm_out_split_ok) it is read back through the documented layout."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    C = 320
    half = 4 * C
    g = torch.Generator().manual_seed(M + C)
    x = torch.randn(M, C, generator=g).to(DEV)
    w1 = torch.randn(8 * C, C, generator=g) / math.sqrt(C)
    b1 = torch.randn(8 * C, generator=g)
    wi = torch.stack([w1[:half].reshape(half // 16, 16, -1), w1[half:].reshape(half // 16, 16, -1)], 1).reshape(2 * half, -1).contiguous().to(DEV)
    bi = torch.stack([b1[:half].reshape(half // 16, 16), b1[half:].reshape(half // 16, 16)], 1).reshape(2 * half).contiguous().to(DEV)
    _assert_plan(ops, form, M, 8 * C, C, plan, f"geglu M={M}", geglu=True)
    a_op, w_op, weff, alpha_w = _operands(ops, form, x, wi)
    core = S.Core(x, weff, 1)
    pick = lambda t, k: t.reshape(M, half // 16, 2, 16)[:, :, k].reshape(M, half)  # de-interleave the [value | gate] column groups
    bd = bi.double().expand(M, 2 * half)
    val, ev = P.preact_bound(pick(core.ref_acc, 0), pick(core.abs_dot, 0), 3 * C, alpha_w, [pick(bd, 0)], pick(core.perr, 0), core.height)
    gate, eg = P.preact_bound(pick(core.ref_acc, 1), pick(core.abs_dot, 1), 3 * C, alpha_w, [pick(bd, 1)], pick(core.perr, 1), core.height)
    ref, bound = val * F.gelu(gate), P.geglu_bound(val, ev, gate, eg, F32)
    tile = (plan[0], plan[1] // 2)
    y = ops.gemm_nt(a_op, w_op, bias=bi, act=ops.ACT_GEGLU)
    assert y.shape == (M, half) and not ops.is_asplit(y)
    worst = P.assert_elementwise(y, ref, bound, f"geglu M={M} {form}", tile)
    can = bool(lib().gmd_gemm_out_split_ok(M, 8 * C, C, 1, ops.WORKSPACE_BYTES))
    assert can == (M == 4096), "the split plan moved: re-pick the shape that stores a pre-split GEGLU output"
    ys = ops.gemm_nt(a_op, w_op, bias=bi, act=ops.ACT_GEGLU, split_out=True)
    assert ops.is_asplit(ys) == can, "gmd_gemm_out_split_ok and the wrapper disagree"
    _report("gemm32", f"geglu M={M} {form}", worst)
    if can:  # (its own line: the split's residual, 2^-22 |x|, is a tight term of a bound that small)
        assert not bool(P.split_layout_violations(ys).any()), "a stored piece is not a (hi, lo) split"
        _report("gemm32", f"geglu M={M} {form} pre-split output",
                P.assert_elementwise(P.unsplit(ys), ref, P.presplit_read_bound(ref, bound), f"geglu M={M} {form} pre-split output", tile))
    else:
        assert torch.equal(ys, y)


@pytest.mark.parametrize("form", S.FORMS)
def test_gemm_split_presplit_output_per_element(form):
    """The ``c_split`` store of the plain row epilogue (an unsplit launch of full 128-row tiles), 160- and 128-column tiles, with bias
    + row bias and with SiLU: read back through parity.unsplit, every stored piece a (hi, lo) split."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    worst = 0.0
    for case in ("128x160 full", "128x128 full"):
        M, N, K, plan = S.GEMM_CASES[case]
        _assert_plan(ops, form, M, N, K, plan, case)
        assert lib().gmd_gemm_out_split_ok(M, N, K, 0, ops.WORKSPACE_BYTES)
        a, w, bias, res, rb, rpg = S.gemm_inputs(M, N, K, DEV)
        a_op, w_op, weff, alpha_w = _operands(ops, form, a, w)
        core = S.Core(a, weff, 1)
        for kw, extras, alpha, act in ((dict(bias=bias, rowbias=rb, rows_per_group=rpg, alpha=0.5), [bias.double().expand(M, N), rb.double().repeat_interleave(rpg, 0)[:M]], 0.5, None),
                                       (dict(bias=bias, act=ops.ACT_SILU), [bias.double().expand(M, N)], 1.0, "silu")):
            got = ops.gemm_nt(a_op, w_op, split_out=True, **kw)
            assert ops.is_asplit(got), "the launch did not store pre-split"
            assert not bool(P.split_layout_violations(got).any()), "a stored piece is not a (hi, lo) split"
            ref, bound = S.ref_and_bound(core, alpha * alpha_w, extras, act)
            worst = max(worst, P.assert_elementwise(P.unsplit(got), ref, P.presplit_read_bound(ref, bound), f"{case} {form} pre-split output act={act}", plan[:2]))
    _report("gemm32", f"pre-split output {form}", worst)


def _smallest_qkv_vt(lib, ops, code, C, tokens):
    """The smallest batch of ``tokens``-row samples gmd_gemm_qkv_vt_ok accepts at width C (found by asking; asserted to be minimal)."""
    for B in range(1, 4096):
        if lib.gmd_gemm_qkv_vt_ok(code, B * tokens, 3 * C, C, 2 * C, tokens, ops.WORKSPACE_BYTES):
            return B
    raise AssertionError("gmd_gemm_qkv_vt_ok accepts no batch at this width")


@pytest.mark.parametrize("form", ["F32SW", "F32SA"])
@pytest.mark.parametrize("C,tokens,bn", [(160, 64, 160), (160, 256, 160), (128, 64, 128)])
def test_gemm_split_qkv_vt_per_element(C, tokens, bn, form):
    """gmd_gemm_qkv_vt on the float32 path: the row-major Q|K part and the transposed V tiles, at the smallest launch the query accepts
    for each column tile width (an unsplit launch of full 128-row tiles needs 256 of them); 64-token samples put two samples into one
    128-row tile."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    code = S.FORM_CODE[form]
    B = _smallest_qkv_vt(lib(), ops, code, C, tokens)
    M = B * tokens
    _assert_plan(ops, form, M, 3 * C, C, (128, bn, 1), f"qkv_vt C={C}")
    step = max(tokens, 128)  # whole samples AND whole 128-row tiles
    assert M % step == 0 and (M // 128) * (3 * C // bn) >= 256 > ((M - step) // 128) * (3 * C // bn), "not the smallest accepted launch"
    g = torch.Generator().manual_seed(B + tokens + C)
    n = torch.randn(M, C, generator=g).to(DEV)
    w = torch.cat([torch.randn(C, C, generator=g) * C ** -0.5 for _ in range(3)], 0).contiguous().to(DEV)
    a_op, w_op, weff, alpha_w = _operands(ops, form, n, w)
    res = ops.gemm_qkv_vt(a_op, w_op, 2 * C, tokens)
    assert res is not None, "the fused launch is not taken: no kernel exercised"
    qk, vt = res
    core = S.Core(n, weff, 1)
    ref, bound = S.ref_and_bound(core, alpha_w, [], None)
    r1 = P.assert_elementwise(qk, ref[:, :2 * C], bound[:, :2 * C], f"qkv_vt {form} row-major part", (128, bn))
    tr = lambda t: t[:, 2 * C:].reshape(B, tokens, C).transpose(1, 2)
    r2 = P.assert_elementwise(vt, tr(ref), tr(bound), f"qkv_vt {form} transposed V", (bn, 128))
    _report("gemm32", f"qkv_vt {B}x{tokens}x{C} {form}", max(r1, r2))


# ---------------------------------------------------------------------------------------------------------------------------
# conv3x3
# ---------------------------------------------------------------------------------------------------------------------------
def _conv_case(ops, tile, mode, form):
    x, w, bias, tb, res, B, H, W, ho, wo, kw = S.conv_inputs(tile, mode, DEV)
    _, ci, co, _, plan = S.CONV_TILES[tile]
    M = B * ho * wo
    amat, ho2, wo2 = P.im2col3x3(x, B, H, W, **kw)
    assert (ho2, wo2) == (ho, wo)
    extras = S.conv_extras(bias, tb, res, B, ho * wo, co)
    return x, w, bias, tb, res, B, H, W, ho, wo, kw, ci, co, plan, M, amat, extras


def test_case_table_is_pairwise_covering():
    """Every mode, every operand form and every tile case of the convolution table meets every other at least once (the same
    assertion runs without a GPU in tests/test_split_parity_cpu.py)."""
    pairs = lambda a, b: {(c[a], c[b]) for c in S.CONV_CASES}
    assert len(pairs(0, 1)) == len(S.MODES) * len(S.FORMS) and len(pairs(0, 2)) == len(S.MODES) * len(S.CONV_TILES)
    assert len(pairs(1, 2)) == len(S.FORMS) * len(S.CONV_TILES)


@pytest.mark.parametrize("mode,form,tile", S.CONV_CASES)
def test_conv3x3_split_per_element(mode, form, tile):
    """The implicit-GEMM convolution against the EXPLICIT float64 im2col product of the same float32 inputs (zero rows for padding), so
    the GEMM bound applies unchanged: stride 1, stride 2 on an odd map, the (0, 1, 0, 1) pad, fused 2x upsample and GMD_UPSAMPLE_TO
    an odd size, on every tile shape with and without slabs; bias + per-sample row bias + residual."""
    from gm_diffusion import hip_ops as ops

    x, w, bias, tb, res, B, H, W, ho, wo, kw, ci, co, plan, M, amat, extras = _conv_case(ops, tile, mode, form)
    _assert_plan(ops, form, M, co, 9 * ci, plan, f"conv {tile} {mode}")
    x_op, w_op, weff, alpha_w = _operands(ops, form, x, w)
    y, h2, w2 = ops.conv3x3(x_op, w_op, B, H, W, bias=bias, rowbias=tb, residual=res, **kw)
    assert (h2, w2) == (ho, wo) and y.shape == (B, ho * wo, co)
    ref, bound = S.ref_and_bound(S.Core(amat, weff, plan[2]), alpha_w, extras, None)
    _report("conv32", f"{tile} {mode} {form}", P.assert_elementwise(y.reshape(M, co), ref, bound, f"conv {tile} {mode} {form}", plan[:2]))


@pytest.mark.parametrize("mode", S.MODES)
def test_conv3x3_exact_float32_per_element(mode):
    """The exact-mode (GMD_F32) convolution on the 23 x 20 map: every product rounds once, the accumulation order is the kernel's own."""
    from gm_diffusion import hip_ops as ops

    x, w, bias, tb, res, B, H, W, ho, wo, kw, ci, co, plan, M, amat, extras = _conv_case(ops, "64x64", mode, "F32S")
    with ops.f32_mode_scope("exact"):
        assert ops._contract_code(x, w, ci) == ops.GMD_F32
        y, _, _ = ops.conv3x3(x, w, B, H, W, bias=bias, rowbias=tb, residual=res, **kw)
    ref, bound = S.exact_ref_and_bound(amat, w, extras)
    _report("conv32", f"exact float32 {mode}", P.assert_elementwise(y.reshape(M, co), ref, bound, f"exact conv {mode}", (64, 64)))


def test_conv3x3_groupnorm_split_per_element():
    """gmd_conv3x3_groupnorm in float32 at the smallest shape that fuses (8 samples x 32 groups = one workgroup per CU; 4 x 4 map,
    320 -> 640: K slices, no reduction launch): Yraw against the convolution, Ynorm against float64 GroupNorm + SiLU of the STORED raw
    tensor."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    B, H, ci, co, G = 8, 4, 320, 640, 32
    form = "F32SW"
    code = S.FORM_CODE[form]
    assert lib().gmd_conv3x3_gn_fusable(code, B, H, H, ci, co, 1, 0, 0, G, ops.WORKSPACE_BYTES), "not the fused launch"
    assert not lib().gmd_conv3x3_gn_fusable(code, B - 1, H, H, ci, co, 1, 0, 0, G, ops.WORKSPACE_BYTES), "a smaller batch fuses too: re-pick"
    M = B * H * H
    _assert_plan(ops, form, M, co, 9 * ci, (128, 160, 5), "conv3x3_groupnorm")
    g = torch.Generator().manual_seed(B * 1000 + H + ci + co)
    x = torch.randn(B, H * H, ci, generator=g).to(DEV)
    w = (torch.randn(co, 9 * ci, generator=g) / math.sqrt(9 * ci)).to(DEV)
    bias, tb = torch.randn(co, generator=g).to(DEV), torch.randn(B, co, generator=g).to(DEV)
    res = torch.randn(B, H * H, co, generator=g).to(DEV)
    gamma, beta = torch.randn(co, generator=g).to(DEV), torch.randn(co, generator=g).to(DEV)
    x_op, w_op, weff, alpha_w = _operands(ops, form, x, w)
    yr, yn = ops.conv3x3_groupnorm(x_op, w_op, B, H, H, G, gamma, beta, 1e-5, silu=True, bias=bias, rowbias=tb, residual=res, want_raw=True)
    amat = P.im2col3x3(x, B, H, H)[0]
    ref, bound = S.ref_and_bound(S.Core(amat, weff, 5), alpha_w, S.conv_extras(bias, tb, res, B, H * H, co), None)
    r1 = P.assert_elementwise(yr.reshape(M, co), ref, bound, "conv3x3_groupnorm Yraw float32", (128, 160))
    # one workgroup of 256 threads per (sample, group): a thread sums H W (C / G) / 256 elements, then tree stages and folds (16)
    ref, bound = P.groupnorm_ref_bound(yr, G, gamma, beta, 1e-5, F32, -(-H * H * (co // G) // 256) + 16, True)
    r2 = P.assert_elementwise(yn, ref, bound, "conv3x3_groupnorm Ynorm float32", (64, 8))
    _report("conv32", "conv3x3_groupnorm F32SW Yraw", r1)
    _report("conv32", "conv3x3_groupnorm F32SW Ynorm", r2)


# ---------------------------------------------------------------------------------------------------------------------------
# loader / converter kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def loader_converter():
    """gmd_gemm_plan_override(0, 0, 244, 0): the float32 path takes gemm_split_lc_kernel wherever it is instantiated (GMD_TUNING=1)."""
    from gm_diffusion._native import lib

    prev = os.environ.get("GMD_TUNING")
    os.environ["GMD_TUNING"] = "1"
    assert lib().gmd_gemm_plan_override(0, 0, 244, 0) == 0
    yield
    lib().gmd_gemm_plan_override(0, 0, 0, 0)
    if prev is None:
        os.environ.pop("GMD_TUNING", None)
    else:
        os.environ["GMD_TUNING"] = prev


@pytest.mark.parametrize("case", ["128x160 ragged in M", "128x128 ragged in both"])
def test_gemm_split_loader_converter_per_element(case, loader_converter):
    """gemm_split_lc_kernel<false, 5> and <false, 4> (pre-split weights, plain activation) under the same bound as the ring kernel."""
    from gm_diffusion import hip_ops as ops

    M, N, _, plan = S.GEMM_CASES[case]
    K = 128  # the kernel wants at least four K steps of 32
    assert ops.split_plan_info(S.FORM_CODE["F32SW"], M, N, K) == (plan[0], plan[1], 244, 1), "not the loader / converter kernel"
    assert ops.split_plan_info(S.FORM_CODE["F32SA"], M, N, K)[2] == 0 and ops.split_plan_info(S.FORM_CODE["F32S"], M, N, K)[2] == 0
    a, w, bias, res, rb, rpg = S.gemm_inputs(M, N, K, DEV)
    a_op, w_op, weff, alpha_w = _operands(ops, "F32SW", a, w)
    core = S.Core(a, weff, 1)
    r = _run_gemm_epilogues(ops, f"loader/converter {case}", plan[:2], a_op, w_op, core, alpha_w, bias, rb, rpg, res, list(S.EPILOGUES))
    _report("gemm32", f"loader/converter {case}", r)


@pytest.mark.parametrize("tile,mode", [("128x160 full chip", "s2"), ("128x128", "up_to_odd")])
def test_conv3x3_split_loader_converter_per_element(tile, mode, loader_converter):
    """gemm_split_lc_kernel<true, 5> and <true, 4>: the convolution addressing of the loader waves."""
    from gm_diffusion import hip_ops as ops

    x, w, bias, tb, res, B, H, W, ho, wo, kw, ci, co, plan, M, amat, extras = _conv_case(ops, tile, mode, "F32SW")
    assert ops.split_plan_info(S.FORM_CODE["F32SW"], M, co, 9 * ci) == (plan[0], plan[1], 244, 1), "not the loader / converter kernel"
    x_op, w_op, weff, alpha_w = _operands(ops, "F32SW", x, w)
    y, _, _ = ops.conv3x3(x_op, w_op, B, H, W, bias=bias, rowbias=tb, residual=res, **kw)
    ref, bound = S.ref_and_bound(S.Core(amat, weff, 1), alpha_w, extras, None)
    _report("conv32", f"loader/converter {tile} {mode}", P.assert_elementwise(y.reshape(M, co), ref, bound, f"loader/converter conv {tile} {mode}", plan[:2]))


def test_split_store_matches_the_library_layout():
    """parity.split_store (what the CPU leg builds its pre-split tensors with) writes the bytes of gmd_split_weights."""
    from gm_diffusion import hip_ops as ops

    x = torch.randn(37, 96, generator=torch.Generator().manual_seed(1)).to(DEV) * 64
    assert torch.equal(P.split_store(x).view(torch.uint8), ops.split_activation(x).view(torch.uint8))
    assert not bool(P.split_layout_violations(ops.split_activation(x)).any())


# ---------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------
def _heads(t, heads):
    B, N, C = t.shape
    return t.reshape(B, N, heads, C // heads).transpose(1, 2)


def _check_attention32(ops, q, k, v, heads, what, k_col=0, qk=None, split_out=True):
    """q, k, v: [B, N, H D] float32 values; ``qk``: the fused buffer the launch reads them from.  The V^T padding columns are NaN."""
    B, Nq, C = q.shape
    Nk, D = k.shape[1], C // heads
    ld = (Nk + 7) // 8 * 8
    vt = torch.full((B, C, ld), float("nan"), device=DEV)
    vt[:, :, :Nk] = v.transpose(1, 2)
    qa, ka = (qk, qk) if qk is not None else (q, k)
    ref, bound = P.attention_split_bound(_heads(q, heads), _heads(k, heads), _heads(v, heads), D ** -0.5)
    got = ops.attention(qa, ka, vt, heads, Nk, D ** -0.5, k_col=k_col)
    worst = P.assert_elementwise(_heads(got, heads), ref, bound, what, (32, D))
    if split_out:
        gs = ops.attention(qa, ka, vt, heads, Nk, D ** -0.5, k_col=k_col, split_out=True)
        assert ops.is_asplit(gs), "the launch did not store pre-split"
        assert not bool(P.split_layout_violations(gs).any()), what + ": a stored piece is not a (hi, lo) split"
        worst = max(worst, P.assert_elementwise(_heads(P.unsplit(gs), heads), ref, P.presplit_read_bound(ref, bound), what + " pre-split output", (32, D)))
    return _report("attention32", what, worst)


@pytest.mark.parametrize("D", [40, 64, 80, 160])
def test_attention_split_presplit_output_per_element(D):
    """``split_out=True``: O stored pre-split for the out-projection, read back through the documented layout; a key count inside
    one tile (7) and a ragged last tile (203), query counts that are no multiple of the 128-row block."""
    from gm_diffusion import hip_ops as ops

    heads, B = 4, 2  # H D a multiple of 32: whole chunks per row
    assert ops.split_attention_ok(F32, D)
    for Nq, Nk in [(200, 7), (333, 203)]:
        g = torch.Generator().manual_seed(D * 7 + Nq + Nk)
        q, k, v = (torch.randn(B, n, heads * D, generator=g).to(DEV) for n in (Nq, Nk, Nk))
        _check_attention32(ops, q, k, v, heads, f"D={D} Nq={Nq} Nk={Nk}")


@pytest.mark.parametrize("D", [40, 64])
def test_attention_split_fused_qk_buffer_per_element(D):
    """Q and K read from ONE [B, N, 2 H D] buffer (k_col = H D): the row stride differs from H D."""
    from gm_diffusion import hip_ops as ops

    heads, B, N = 8, 2, 256
    C = heads * D
    g = torch.Generator().manual_seed(5)
    qk = torch.randn(B, N, 2 * C, generator=g).to(DEV)
    v = torch.randn(B, N, C, generator=g).to(DEV)
    _check_attention32(ops, qk[:, :, :C].contiguous(), qk[:, :, C:].contiguous(), v, heads, f"fused-qk D={D}", k_col=C, qk=qk)


@pytest.mark.parametrize("spike", [1.5, 3.0, 8.0])
def test_attention_split_spiked_keys_per_element(spike):
    """test_attention_spiked_keys_per_element's generator in float32: single keys that dominate late in the sequence (the rescale
    branch of the online softmax)."""
    from gm_diffusion import hip_ops as ops

    D, N = 40, 320
    g = torch.Generator().manual_seed(77)
    q = torch.randn(1, N, D, generator=g)
    k = torch.randn(1, N, D, generator=g) * 0.3
    v = torch.randn(1, N, D, generator=g)
    k[0, 200] = q[0, 5] * spike
    k[0, 310] = q[0, 100] * (spike + 1.0)
    q, k, v = (t.to(DEV) for t in (q, k, v))
    _check_attention32(ops, q, k, v, 1, f"spike {spike}", split_out=False)  # (H D = 40: no whole chunks)


@pytest.mark.parametrize("D", [40, 80])
def test_attention_split_all_negative_rows_per_element(D):
    from gm_diffusion import hip_ops as ops

    heads, N = 2, 200
    g = torch.Generator().manual_seed(D)
    base = torch.randn(1, 1, heads * D, generator=g)
    q = base * 4.0 + 0.3 * torch.randn(1, N, heads * D, generator=g)
    k = -base * 4.0 + 0.3 * torch.randn(1, N, heads * D, generator=g)
    v = torch.randn(1, N, heads * D, generator=g)
    q, k, v = (t.to(DEV) for t in (q, k, v))
    _check_attention32(ops, q, k, v, heads, f"all-negative D={D}", split_out=(heads * D) % 32 == 0)
