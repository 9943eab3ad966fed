"""GPU: several LoRA adapters at once.  The stacked rank-update launches (gmd_lora_update_stacked / gmd_lora_geglu_stacked) per element
against float64 and the derived bound of tests/lora_multi_ref.py, with a DIFFERENT scale on every rank column; write footprints, grid
geometry, row independence, the device-resident table; the sequential route; the UNet with two adapters on unequal target sets
against the merged oracle; the dual pipeline (graphs, set_adapters between calls, disable / enable, ControlNet + IP-Adapter)."""
import functools
import itertools

import pytest
import torch

import lora_ff_ref as FR
import lora_multi_ref as MR
import lora_ref as R
import parity as P
import test_lora_gpu as T1  # the one-adapter tests: their gates (MODEL_TOL, MEASURED_16BIT_RMS), shapes and pipeline fixtures

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
CANARY = T1.CANARY
_pad = MR.pad


def _table(cs, idx, rows=7, extra=8):
    """A device table [rows, Rp + extra]: ``cs`` in row ``idx``; every other row and the pad columns of every row hold 1e4."""
    t = torch.full((rows, cs.numel() + extra), 1.0e4, dtype=F32)
    t[idx, :cs.numel()] = cs
    return t.to(DEV)


def _call(x, a, b, ybuf, yptr_off, M, N, ldy, tab, idx, trans=None, strideY=0):
    """gmd_lora_update_stacked through the C ABI; returns the status."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    batch, tokens = trans if trans else (1, M)
    return lib().gmd_lora_update_stacked(x.data_ptr(), a.data_ptr(), b.data_ptr(), ybuf.data_ptr() + yptr_off * ybuf.element_size(),
                                         ops.dtype_code(x.dtype), M, x.shape[1], a.shape[0], N, x.shape[1], ldy, int(trans is not None), batch,
                                         tokens, strideY, tab.data_ptr(), idx, tab.shape[1], torch.cuda.current_stream().cuda_stream)


def _run_plain(x, a, b, y0, ldy, col, tab, idx, extra_rows=0):
    """y0 embedded at columns [col, col + N) of a canary-filled [M + extra_rows, ldy] buffer; returns the buffer after the launch."""
    from gm_diffusion._native import check

    M, N = y0.shape
    buf = torch.full((M + extra_rows, ldy), CANARY, dtype=y0.dtype)
    buf[:M, col:col + N] = y0
    buf = buf.to(DEV)
    check(_call(x.to(DEV), a.to(DEV), b.to(DEV), buf, col, M, N, ldy, tab, idx), "gmd_lora_update_stacked")
    torch.cuda.synchronize()
    return buf.cpu()


def _run_trans(x, a, b, y0, batch, tokens, ldy, tab, idx):
    """y0 [M, N] as V^T [batch, N, ldy] with canary pad columns [tokens, ldy); returns the buffer after the launch."""
    from gm_diffusion._native import check

    M, N = y0.shape
    buf = torch.full((batch, N, ldy), CANARY, dtype=y0.dtype)
    buf[:, :, :tokens] = y0.view(batch, tokens, N).permute(0, 2, 1)
    buf = buf.to(DEV)
    check(_call(x.to(DEV), a.to(DEV), b.to(DEV), buf, 0, M, N, ldy, tab, idx, trans=(batch, tokens), strideY=N * ldy), "gmd_lora_update_stacked")
    torch.cuda.synchronize()
    return buf.cpu()


def _untrans(out, tokens, M, N):
    return out[:, :, :tokens].permute(0, 2, 1).reshape(M, N)


# ---------------------------------------------------------------------------------------------------------------------------
# kernel, per element: a pairwise-covering table
# ---------------------------------------------------------------------------------------------------------------------------
MS, KS, NS, WIDE, INDEX = (1, 63, 64, 161), (64, 128, 320), (64, 200, 320), (False, True), (0, 5)
# sums 4 ... 256; adapter boundaries off the 4- and the 16-column grid; padded ranks 32, 128, 160, 256 -- and (20, 30) for 64
RANKS = ((1, 3), (3, 5, 8), (16, 16), (64, 64), (40, 90), (128, 128), (20, 30))
TRANS = ((1, 77), (3, 77), (2, 130))
PLAIN_CASES = T1._pairwise((MS, KS, RANKS, NS, WIDE, INDEX))
TRANS_CASES = T1._pairwise((TRANS, KS, RANKS, NS, INDEX))


def test_case_tables_are_pairwise_covering():
    for cases, axes in ((PLAIN_CASES, (MS, KS, RANKS, NS, WIDE, INDEX)), (TRANS_CASES, (TRANS, KS, RANKS, NS, INDEX))):
        for i, j in itertools.combinations(range(len(axes)), 2):
            assert {(c[i], c[j]) for c in cases} == set(itertools.product(axes[i], axes[j]))
    assert {_pad(sum(r), 32) for r in RANKS} == {32, 64, 128, 160, 256}
    assert len(PLAIN_CASES) <= 48 and len(TRANS_CASES) <= 36


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_kernel_plain_per_element_zero_violations(dtype):
    """M x K x ranks x N x ldy (N, or N + 320 with the window at column 160) x table row, pairwise covering."""
    worst = 0.0
    for c, (M, K, ranks, N, wide, idx) in enumerate(PLAIN_CASES):
        x, a, b, y0, cs = MR.stacked_operands(M, K, ranks, N, dtype, seed=100 + 2 * c)
        ldy, col = (N + 320, 160) if wide else (N, 0)
        out = _run_plain(x, a, b, y0, ldy, col, _table(cs, idx), idx)
        ref, bound = MR.stacked_ref_bound(x, a, b, y0, cs, dtype)
        worst = max(worst, P.assert_elementwise(out[:, col:col + N], ref, bound, f"stacked {dtype} M={M} K={K} ranks={ranks} N={N} ldy={ldy} "
                                                f"row={idx}", tile=(16, 64)))
        if wide:
            assert bool((out[:, :col] == CANARY).all()) and bool((out[:, col + N:] == CANARY).all()), "columns outside [col, col + N) changed"
    print(f"lora_update_stacked plain {dtype}: {len(PLAIN_CASES)} cases, max |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_kernel_transposed_per_element_zero_violations(dtype):
    """(batch, tokens) x K x ranks x N x table row, pairwise covering; Y is V^T [batch, N, tokens padded to 8]."""
    worst = 0.0
    for c, ((batch, tokens), K, ranks, N, idx) in enumerate(TRANS_CASES):
        M, ldy = batch * tokens, _pad(tokens, 8)
        x, a, b, y0, cs = MR.stacked_operands(M, K, ranks, N, dtype, seed=500 + 2 * c)
        out = _run_trans(x, a, b, y0, batch, tokens, ldy, _table(cs, idx), idx)
        ref, bound = MR.stacked_ref_bound(x, a, b, y0, cs, dtype)
        worst = max(worst, P.assert_elementwise(_untrans(out, tokens, M, N), ref, bound, f"stacked^T {dtype} batch={batch} tokens={tokens} K={K} "
                                                f"ranks={ranks} N={N} row={idx}", tile=(64, 16)))
        assert bool((out[:, :, tokens:] == CANARY).all()), "pad columns [tokens, ldy) changed"
    print(f"lora_update_stacked transposed {dtype}: {len(TRANS_CASES)} cases, max |err| / bound = {worst:.3f}")


def _geglu_call(x, a, b, y, f, M, C, ldf, tab, idx):
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    return lib().gmd_lora_geglu_stacked(x.data_ptr(), a.data_ptr(), b.data_ptr(), y.data_ptr(), f.data_ptr(), ops.dtype_code(x.dtype), M, C,
                                        a.shape[0], C, 8 * C, ldf, tab.data_ptr(), idx, tab.shape[1], torch.cuda.current_stream().cuda_stream)


def _run_geglu(x, a, b, y0, tab, idx, ldf_extra=64, extra_rows=3):
    """F inside a canary-filled [M + extra_rows, 4C + ldf_extra] buffer; returns (the buffer, y after the launch)."""
    from gm_diffusion._native import check

    M, C = x.shape
    f = torch.full((M + extra_rows, 4 * C + ldf_extra), CANARY, dtype=x.dtype, device=DEV)
    dy = y0.to(DEV)
    check(_geglu_call(x.to(DEV), a.to(DEV), b.to(DEV), dy, f, M, C, 4 * C + ldf_extra, tab, idx), "gmd_lora_geglu_stacked")
    torch.cuda.synchronize()
    return f.cpu(), dy.cpu()


GEGLU_CASES = T1._pairwise(((1, 63, 161), (64, 128), RANKS, INDEX))


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_kernel_geglu_per_element_zero_violations(dtype):
    """M x C x ranks x table row: F against float64, Y unchanged, canaries round F (columns [4C, ldf) and the rows from M on)."""
    worst = 0.0
    for c, (M, C, ranks, idx) in enumerate(GEGLU_CASES):
        x, a, b, y0, cs = MR.stacked_operands(M, C, ranks, 8 * C, dtype, seed=900 + 2 * c)
        fbuf, y_after = _run_geglu(x, a, b, y0, _table(cs, idx), idx)
        ref, bound = MR.stacked_geglu_ref_bound(x, a, b, y0, cs, dtype)
        worst = max(worst, P.assert_elementwise(fbuf[:M, :4 * C], ref, bound, f"geglu stacked {dtype} M={M} C={C} ranks={ranks} row={idx}",
                                                tile=(16, 32)))
        assert torch.equal(y_after, y0), "Y is read-only"
        assert bool((fbuf[M:] == CANARY).all()) and bool((fbuf[:M, 4 * C:] == CANARY).all()), "F written outside [M, 4C]"
    print(f"lora_geglu_stacked {dtype}: {len(GEGLU_CASES)} cases, max |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_every_padded_rank_in_every_mode(dtype):
    """One small launch per instantiation: padded ranks 32, 64, ..., 256 x plain / transposed / GEGLU (two adapters, the boundary
    off the 16-column grid)."""
    for rp in range(32, 257, 32):
        ranks = (rp // 2 - 3, rp // 2 - 2)  # sums rp - 5: pads to rp
        assert _pad(sum(ranks), 32) == rp
        x, a, b, y0, cs = MR.stacked_operands(70, 128, ranks, 72, dtype, seed=rp)
        ref, bound = MR.stacked_ref_bound(x, a, b, y0, cs, dtype)
        P.assert_elementwise(_run_plain(x, a, b, y0, 72, 0, _table(cs, 1), 1), ref, bound, f"plain Rp={rp} {dtype}")
        out = _run_trans(x, a, b, y0, 1, 70, 72, _table(cs, 2), 2)
        P.assert_elementwise(_untrans(out, 70, 70, 72), ref, bound, f"transposed Rp={rp} {dtype}")
        assert bool((out[:, :, 70:] == CANARY).all())
        xg, ag, bg, yg, csg = MR.stacked_operands(70, 64, ranks, 512, dtype, seed=rp + 1)
        fbuf, _ = _run_geglu(xg, ag, bg, yg, _table(csg, 0), 0)
        fref, fbound = MR.stacked_geglu_ref_bound(xg, ag, bg, yg, csg, dtype)
        P.assert_elementwise(fbuf[:70, :256], fref, fbound, f"geglu Rp={rp} {dtype}")


# ---------------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16])
def test_kernel_several_n_tiles_per_workgroup(dtype):
    """The walk over N inside one workgroup, at the shapes tests/test_lora_gpu.py derives (2 and 3 tiles per workgroup plain, 2
    transposed), per element; the stacked ranks here pad to 32 and to 160."""
    for c, (M, K, _, N) in enumerate(T1.MULTI_TILE_PLAIN):
        assert T1._tiles_per_workgroup(_pad(M, 64) // 64, N) == (2, 3)[c]
        ranks = ((3, 5, 8), (40, 90))[c]
        x, a, b, y0, cs = MR.stacked_operands(M, K, ranks, N, dtype, seed=700 + c)
        out = _run_plain(x, a, b, y0, N + 64, 32, _table(cs, 5), 5)
        ref, bound = MR.stacked_ref_bound(x, a, b, y0, cs, dtype)
        P.assert_elementwise(out[:, 32:32 + N], ref, bound, f"stacked {dtype} M={M} K={K} ranks={ranks} N={N}, several tiles", tile=(16, 64))
        assert bool((out[:, :32] == CANARY).all()) and bool((out[:, 32 + N:] == CANARY).all())
    for c, ((batch, tokens), K, _, N) in enumerate(T1.MULTI_TILE_TRANS):
        assert T1._tiles_per_workgroup(batch * (_pad(tokens, 64) // 64), N) == 2
        ranks = ((40, 90), (1, 3))[c]
        M, ldy = batch * tokens, _pad(tokens, 8)
        x, a, b, y0, cs = MR.stacked_operands(M, K, ranks, N, dtype, seed=720 + c)
        out = _run_trans(x, a, b, y0, batch, tokens, ldy, _table(cs, 0), 0)
        ref, bound = MR.stacked_ref_bound(x, a, b, y0, cs, dtype)
        P.assert_elementwise(_untrans(out, tokens, M, N), ref, bound, f"stacked^T {dtype} batch={batch} tokens={tokens} ranks={ranks}, several "
                             "tiles", tile=(64, 16))
        assert bool((out[:, :, tokens:] == CANARY).all())


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_row_independence_across_grids(dtype):
    """The same rows give the same bits alone and inside a larger M, across DIFFERENT grids: N split five ways over gridDim.y (M = 64:
    one row block), one tile per workgroup at M = 1030, two tiles per workgroup at M = 8259 (129 row blocks); transposed: one batch
    entry alone against the first of 130."""
    K, N, ranks = 64, 320, (40, 90)
    assert T1._tiles_per_workgroup(1, N) == 1 and T1._tiles_per_workgroup(17, N) == 1 and T1._tiles_per_workgroup(130, N) == 2
    x, a, b, y0, cs = MR.stacked_operands(8259, K, ranks, N, dtype, seed=21)
    tab = _table(cs, 5)
    big = _run_plain(x, a, b, y0, N, 0, tab, 5)
    mid = _run_plain(x[:1030].contiguous(), a, b, y0[:1030].contiguous(), N, 0, tab, 5)
    small = _run_plain(x[:64].contiguous(), a, b, y0[:64].contiguous(), N, 0, tab, 5)
    assert torch.equal(big[:64].view(torch.int16), small.view(torch.int16)) and torch.equal(mid[:64].view(torch.int16), small.view(torch.int16))
    assert torch.equal(big[:1030].view(torch.int16), mid.view(torch.int16)) and not torch.equal(small, y0[:64])
    xb, ab, bb, yb, csb = MR.stacked_operands(130 * 64, K, (3, 5, 8), N, dtype, seed=24)
    tb = _table(csb, 0)
    many = _run_trans(xb, ab, bb, yb, 130, 64, 64, tb, 0)
    first = _run_trans(xb[:64].contiguous(), ab, bb, yb[:64].contiguous(), 1, 64, 64, tb, 0)
    assert torch.equal(many[:1].view(torch.int16), first.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------------------
# scales
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16])
def test_a_zero_column_scale_is_that_adapter_s_rows_zeroed(dtype):
    ranks = (3, 5, 8)
    x, a, b, y0, cs = MR.stacked_operands(161, 128, ranks, 200, dtype, seed=33)
    off = cs.clone()
    off[3:8] = 0.0  # the middle adapter's columns
    a0 = a.clone()
    a0[3:8] = 0
    by_scale = _run_plain(x, a, b, y0, 200, 0, _table(off, 0), 0)
    by_rows = _run_plain(x, a0, b, y0, 200, 0, _table(cs, 0), 0)
    assert torch.equal(by_scale.view(torch.int16), by_rows.view(torch.int16)) and not torch.equal(by_scale, y0)
    assert not torch.equal(by_scale, _run_plain(x, a, b, y0, 200, 0, _table(cs, 0), 0))
    xt, at, bt, yt, cst = MR.stacked_operands(3 * 77, 128, ranks, 200, dtype, seed=34)
    allz = torch.zeros_like(cst)
    zt = _run_trans(xt, at, bt, yt, 3, 77, 80, _table(allz, 0), 0)
    assert torch.equal(_untrans(zt, 77, 3 * 77, 200), yt)  # every column at 0: Y keeps its bits


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_one_graph_serves_every_table(dtype):
    from gm_diffusion import hip_ops as ops

    ranks = (40, 90)
    x, a, b, y0, cs = MR.stacked_operands(161, 128, ranks, 200, dtype, seed=31)
    dx, da, db, dy0 = (t.to(DEV) for t in (x, a, b, y0))
    tab = _table(cs, 5)
    y = dy0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.lora_update_stacked(dx, da, db, y, tab, 5, fused=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y.copy_(dy0)
        ops.lora_update_stacked(dx, da, db, y, tab, 5, fused=True)
    for seed in (1, 2):
        new = MR.column_scales(cs.numel(), sum(ranks), seed=77 + seed)
        tab[5, :cs.numel()] = new.to(DEV)
        g.replay()
        torch.cuda.synchronize()
        replayed = y.cpu()
        eager = ops.lora_update_stacked(dx, da, db, dy0.clone(), tab, 5, fused=True).cpu()
        assert torch.equal(replayed.view(torch.int16), eager.view(torch.int16))
        ref, bound = MR.stacked_ref_bound(x, a, b, y0, new, dtype)
        P.assert_elementwise(replayed, ref, bound, f"replay with table {seed} {dtype}")


# ---------------------------------------------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------------------------------------------
def _per_adapter_cs(rp, ranks, scalars):
    cs = torch.zeros(rp, dtype=F32)
    for (c0, c1), s in zip(MR.column_ranges(ranks), scalars):
        cs[c0:c1] = s
    return cs


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("mode", ["plain", "trans", "geglu"])
def test_fused_and_sequential_routes_each_inside_their_own_bound(dtype, mode):
    """The stacked launch against fused=False (what GMD_LORA_STACK_FUSED=0 selects: one lora_update per adapter, in load order, a
    scalar scale each).  Each route inside ITS OWN bound of float64 -- they are not bit-equal: the sequential route rounds Y between
    the adapters."""
    from gm_diffusion import hip_ops as ops

    assert ops.USE_LORA_STACK_FUSED  # the default route of the 16-bit types is the stacked launch
    ranks, scalars = (3, 5, 8), (0.8, -0.5, 1.3)
    batch, tokens = 3, 77
    M = batch * tokens
    K, N = (64, 512) if mode == "geglu" else (128, 200)
    x, a, b, y0, _ = MR.stacked_operands(M, K, ranks, N, dtype, seed=41)
    cs = _per_adapter_cs(a.shape[0], ranks, scalars)
    tab = _table(cs, 2)
    sc = torch.full((9,), 1.0e4, dtype=F32)
    sc[4:7] = torch.tensor(scalars)
    sc = sc.to(DEV)
    parts = MR.split_parts(a, b, cs, ranks, 32)
    dparts = [(pa.to(DEV), pb.to(DEV), sc, 4 + i) for i, (pa, pb) in enumerate(parts)]
    dx, da, db = x.to(DEV), a.to(DEV), b.to(DEV)
    one = lambda x_, a_, b_, y_, s_: R.update_ref_bound(x_, a_, b_, y_, torch.tensor(s_, dtype=F32), dtype)
    if mode == "geglu":
        f = ops.lora_geglu_stacked(dx, da, db, y0.to(DEV), tab, 2, fused=True).cpu()
        ys = y0.to(DEV)
        s = ops.lora_geglu_stacked(dx, None, None, ys, None, 0, fused=False, parts=dparts).cpu()
        ref, bound = MR.stacked_geglu_ref_bound(x, a, b, y0, cs, dtype)
        P.assert_elementwise(f, ref, bound, f"stacked geglu {dtype}")
        # sequential: Y after the adapters inside the chained bound, then the GEGLU kernel on those rounded values
        yref, ybound = MR.sequential_ref_bound(x, parts, scalars, y0, dtype, one)
        P.assert_elementwise(ys.cpu(), yref, ybound, f"sequential geglu {dtype}: y after the updates")
        (v, g), (ev, eg) = FR.deinterleave_cols(yref), FR.deinterleave_cols(ybound)
        gref, gbound = v * torch.nn.functional.gelu(g), P.geglu_bound(v, ev, g, eg, dtype)
        P.assert_elementwise(s, gref, gbound, f"sequential geglu {dtype}")
        return
    if mode == "trans":
        ldy = _pad(tokens, 8)
        yt = torch.zeros(batch, N, ldy, dtype=dtype)
        yt[:, :, :tokens] = y0.view(batch, tokens, N).permute(0, 2, 1)
        f = ops.lora_update_stacked(dx, da, db, yt.to(DEV), tab, 2, transposed=True, tokens=tokens, fused=True)
        s = ops.lora_update_stacked(dx, da, db, yt.to(DEV), tab, 2, transposed=True, tokens=tokens, fused=False, parts=dparts)
        assert bool((f[:, :, tokens:] == 0).all()) and bool((s[:, :, tokens:] == 0).all())
        f, s = (_untrans(t.cpu(), tokens, M, N) for t in (f, s))
    else:  # columns [64, 64 + N) of a wider buffer
        wide = torch.full((M, N + 128), CANARY, dtype=dtype)
        wide[:, 64:64 + N] = y0
        f = ops.lora_update_stacked(dx, da, db, wide.to(DEV), tab, 2, col=64, fused=True).cpu()
        s = ops.lora_update_stacked(dx, da, db, wide.to(DEV), tab, 2, col=64, fused=False, parts=dparts).cpu()
        for t in (f, s):
            assert bool((t[:, :64] == CANARY).all()) and bool((t[:, 64 + N:] == CANARY).all())
        f, s = f[:, 64:64 + N], s[:, 64:64 + N]
    ref, b_f = MR.stacked_ref_bound(x, a, b, y0, cs, dtype)
    sref, b_s = MR.sequential_ref_bound(x, parts, scalars, y0, dtype, one)
    assert float((ref - sref).abs().max()) < 1e-9  # one float64 reference, two bounds
    P.assert_elementwise(f, ref, b_f, f"stacked {dtype} {mode}")
    P.assert_elementwise(s, sref, b_s, f"sequential {dtype} {mode}")


@pytest.mark.parametrize("f32mode", ["split", "exact"])
@pytest.mark.parametrize("trans", [False, True])
def test_float32_takes_the_sequential_composed_route(f32mode, trans):
    """float32 has no stacked kernel: lora_update_stacked runs one composed lora_update per adapter, against lora_ref's float32 bound
    applied per adapter; the factors prepared as the model prepares them."""
    from gm_diffusion import hip_ops as ops

    ranks, scalars = (3, 5, 8), (0.8, -0.5, 1.3)
    batch, tokens, K, N = 3, 77, 128, 200
    M = batch * tokens
    mult = 32 if f32mode == "split" else 16
    x, a, b, y0, _ = MR.stacked_operands(M, K, ranks, N, F32, seed=51)
    parts = MR.split_parts(a, b, None, ranks, mult)
    sc = torch.full((9,), 1.0e4, dtype=F32)
    sc[4:7] = torch.tensor(scalars)
    sc = sc.to(DEV)
    prev = ops.set_f32_mode(f32mode)
    try:
        assert ops.lora_rank_multiple(F32) == mult
        prep_a = (lambda t: ops.split_weights(t.to(DEV))) if f32mode == "split" else (lambda t: t.to(DEV))
        prep_bt = (lambda t: ops.scale_weight(t.to(DEV))) if f32mode == "split" else (lambda t: t.to(DEV))
        dparts = [(prep_a(pa), prep_bt(pb) if trans else prep_a(pb), sc, 4 + i) for i, (pa, pb) in enumerate(parts)]
        if trans:
            ldy = _pad(tokens, 4)
            yt = torch.zeros(batch, N, ldy)
            yt[:, :, :tokens] = y0.view(batch, tokens, N).permute(0, 2, 1)
            got = ops.lora_update_stacked(x.to(DEV), None, None, yt.to(DEV), None, 0, transposed=True, tokens=tokens, parts=dparts)
            assert bool((got[:, :, tokens:] == 0).all())
            got = _untrans(got, tokens, M, N)
        else:
            got = ops.lora_update_stacked(x.to(DEV), None, None, y0.to(DEV), None, 0, parts=dparts)
        torch.cuda.synchronize()
    finally:
        ops.set_f32_mode(prev)
    one = lambda x_, a_, b_, y_, s_: R.update_ref_bound_f32(x_, a_, b_, y_, torch.tensor(s_, dtype=F32), f32mode)
    ref, bound = MR.sequential_ref_bound(x, parts, scalars, y0, F32, one)
    P.assert_elementwise(got.cpu(), ref, bound, f"float32 {f32mode} trans={trans}")


# ---------------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_and_empty_launches():
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import HipExtensionError, lib

    # X [8, 64] | Aw [<= 256, 64] | Bw [<= 512, <= 256] | Y [8, <= 512] | F [8, 256]: every operand of the largest launch below fits
    buf = torch.zeros(1 << 18, dtype=BF16, device=DEV)
    p, es = buf.data_ptr(), 2
    X, A, B_, Y, Fp = p, p + 16384 * es, p + 32768 * es, p + 163840 * es, p + 172032 * es
    assert 32768 + 512 * 256 <= 163840 and 163840 + 8 * 512 <= 172032 and 172032 + 8 * 256 <= buf.numel()
    tab = torch.ones(4, 264, dtype=F32, device=DEV)
    n, ng = lib().gmd_lora_update_stacked, lib().gmd_lora_geglu_stacked

    def args(**o):
        return [o.get("X", X), A, B_, o.get("Y", Y), o.get("dtype", 1), o.get("M", 8), o.get("K", 64), o.get("Rp", 32), o.get("N", 64),
                o.get("ldx", 64), o.get("ldy", 64), o.get("trans", 0), o.get("batch", 1), o.get("tokens", 8), o.get("strideY", 0),
                o.get("tab", tab.data_ptr()), o.get("idx", 0), o.get("ldc", 264), None]

    def gargs(**o):
        return [o.get("X", X), A, B_, o.get("Y", Y), o.get("F", Fp), o.get("dtype", 1), o.get("M", 8), 64, o.get("Rp", 32), 64, 512,
                o.get("ldf", 256), o.get("tab", tab.data_ptr()), o.get("idx", 0), o.get("ldc", 264), None]

    for call, mk in ((n, args), (ng, gargs)):
        assert call(*mk()) == 0
        assert call(*mk(Rp=256)) == 0 and call(*mk(Rp=160)) == 0 and call(*mk(idx=3)) == 0
        assert call(*mk(Rp=0)) == 1 and call(*mk(Rp=48)) == 1 and call(*mk(Rp=288)) == 1     # Rp: a multiple of 32 in [32, 256]
        assert call(*mk(tab=None)) == 1 and call(*mk(idx=-1)) == 1                            # the table
        assert call(*mk(Rp=64, ldc=32)) == 1 and call(*mk(ldc=-1)) == 1 and call(*mk(Rp=64, ldc=64)) == 0   # ldc < Rp
        assert call(*mk(X=X + 2)) == 1 and call(*mk(Y=Y + 2)) == 1                            # alignment
        assert call(*mk(dtype=0)) == 3 and call(*mk(dtype=3)) == 3                            # float32: the caller's sequential route
    assert b"gmd_lora_geglu_stacked" in lib().gmd_last_error()
    assert n(*args(Y=X)) == 1 and n(*args(Y=X + 64 * es)) == 1                                # X overlaps Y
    assert b"gmd_lora_update_stacked: X overlaps Y" in lib().gmd_last_error()
    assert n(*args(K=96)) == 1 and n(*args(ldy=56)) == 1 and n(*args(ldx=60)) == 1
    assert n(*args(trans=1, batch=2, tokens=8)) == 1 and n(*args(trans=1, batch=1, tokens=8, ldy=8, strideY=64 * 8)) == 0
    assert ng(*gargs(F=X)) == 1 and ng(*gargs(F=Y)) == 1 and ng(*gargs(ldf=248)) == 1        # F overlaps X / Y; ldf < 4C
    torch.cuda.synchronize()
    # empty launches return OK and write nothing -- with pointers that would fault if anything were launched
    canary = torch.full((4096,), CANARY, dtype=BF16, device=DEV)
    assert n(*args(M=0, Y=canary.data_ptr())) == 0 and ng(*gargs(M=0, F=canary.data_ptr())) == 0
    torch.cuda.synchronize()
    assert bool((canary == CANARY).all())
    x, a, b = buf[:512].view(8, 64), buf[16384:16384 + 2048].view(32, 64), buf[32768:32768 + 2048].view(64, 32)
    with pytest.raises(HipExtensionError):  # dtype mismatch
        ops.lora_update_stacked(x, a, b, torch.zeros(8, 64, dtype=F16, device=DEV), tab, 0)
    with pytest.raises(HipExtensionError):  # a row outside the table
        ops.lora_update_stacked(x, a, b, torch.zeros(8, 64, dtype=BF16, device=DEV), tab, 4)
    with pytest.raises(HipExtensionError):  # table rows shorter than the padded rank
        ops.lora_update_stacked(x, a, b, torch.zeros(8, 64, dtype=BF16, device=DEV), tab[:, :16].contiguous(), 0)


# ---------------------------------------------------------------------------------------------------------------------------
# UNet (tiny config, 16 x 16 latents, batch 2): attention-only rank 4 + transformer rank 8, weights (0.8, -0.5), global scale 0.7
# ---------------------------------------------------------------------------------------------------------------------------
GAIN, WEIGHTS, SCALE = 1.0, (0.8, -0.5), 0.7  # gain 1: see tests/test_lora_multi_cpu.py


@functools.lru_cache(maxsize=None)
def _refs():
    ou, og, _, _ = T1._refs()
    ca = FR.canonical(ou, 4, 11, GAIN, alpha=2.0, families=("attention",))
    cb = FR.canonical(ou, 8, 12, GAIN, alpha=4.0, families=None)
    return ou, og, ca, cb, FR.to_convention(ca, "kohya"), FR.to_convention(cb, "peft")


def _load_two(hu):
    _, _, _, _, sa, sb = _refs()
    hu.load_lora(sa, adapter_name="style")
    hu.load_lora(sb, targets="transformer", adapter_name="subject")
    hu.set_adapters(["style", "subject"], list(WEIGHTS))
    hu.set_lora_scale(SCALE)
    return hu


@functools.lru_cache(maxsize=None)
def _unet_case():
    ou, _, ca, cb, _, _ = _refs()
    g = torch.Generator().manual_seed(61)
    lat, ctx = torch.randn(1, 4, 16, 16, generator=g), torch.randn(2, 77, 64, generator=g)
    x = torch.cat([lat, lat])
    with torch.no_grad():
        eps = MR.merged_oracle(ou, [(ca, WEIGHTS[0]), (cb, WEIGHTS[1])], SCALE)(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
        only_b = MR.merged_oracle(ou, [(cb, WEIGHTS[1])], SCALE)(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
        plain = ou(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
    return lat, ctx, eps, only_b, plain


@functools.lru_cache(maxsize=None)
def _f32_unet_run():
    from gm_diffusion import hip_ops as ops

    ou = _refs()[0]
    lat, ctx, _, _, _ = _unet_case()
    prev = ops.set_f32_mode("split")
    try:
        out = _load_two(T1._hip_unet(ou, F32))(torch.cat([lat, lat]).to(DEV), 501, encoder_hidden_states=ctx.to(DEV), return_dict=False)[0]
        torch.cuda.synchronize()
    finally:
        ops.set_f32_mode(prev)
    return out.cpu()


@pytest.mark.parametrize("dtype,mode", [(F32, "split"), (F32, "exact"), (BF16, "split"), (F16, "split")])
def test_unet_with_two_adapters_against_the_merged_oracle(dtype, mode):
    """float32 (split and exact) against the merged oracle, the 16-bit types against the float32 run, at the one-adapter tests' gates
    (T1.MODEL_TOL); packed eager == graph replay == cfg_shared bit for bit; set_adapters keeps the graph and equals a fresh model."""
    from gm_diffusion import hip_ops as ops

    prev = ops.set_f32_mode(mode)
    try:
        ou = _refs()[0]
        lat, ctx, eps, only_b, plain = _unet_case()
        tol = T1.MODEL_TOL[dtype]
        hu = _load_two(T1._hip_unet(ou, dtype))
        dlat, dctx = lat.to(DEV), ctx.to(DEV)
        dx = torch.cat([dlat, dlat])
        got = hu(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0]
        ref = eps if dtype == F32 else _f32_unet_run()
        e = T1.rel_err(got, ref)
        print(f"UNet + two adapters {dtype} {mode}: rel err {e:.3e} vs {'the merged oracle' if dtype == F32 else 'the float32 run'} (tol "
              f"{tol:.0e}); the adapters move the output by {T1.rel_err(eps, plain):.3f}, the second one by {T1.rel_err(eps, only_b):.3f}")
        assert got.shape == eps.shape and e < tol, e
        # the references alone: both adapters together move the output by > 10 x the gate, and a model that lost the attention-only
        # adapter would still sit > 5 x the loosest gate from the reference
        assert T1.rel_err(eps, plain) > 10 * tol and T1.rel_err(eps, only_b) > 5 * tol
        if dtype != F32:
            assert T1.rel_err(ref, eps) < T1.MODEL_TOL[F32]
        c = hu.prepare_context(dctx)
        hu.set_timestep(501)
        full = hu.forward_packed(hu.pack_input(dlat, dup=2), 2, 16, 16, c)
        assert torch.equal(full, got)
        assert torch.equal(hu.forward_packed(hu.pack_input(dlat, dup=1), 2, 16, 16, c, cfg_shared=True), full)
        gph = hu.graphed_forward(2, 16, 16, c, cfg_shared=True)
        hu.pack_input(dlat, dup=1, out=gph.x)
        assert torch.equal(gph.replay(), full)
        # new weights: the same graph object, the bits of a fresh model given those weights from the start
        n_graphs, v = len(hu._graphs), hu._lora_version
        hu.set_adapters(["subject", "style"], [1.0, 0.25])
        assert hu._lora_version == v + 1
        assert hu.graphed_forward(2, 16, 16, c, cfg_shared=True) is gph and len(hu._graphs) == n_graphs
        moved = gph.replay().clone()
        fresh = T1._hip_unet(ou, dtype)
        _, _, _, _, sa, sb = _refs()
        fresh.load_lora(sa, adapter_name="style").load_lora(sb, targets="transformer", adapter_name="subject")
        fresh.set_adapters(["style", "subject"], [0.25, 1.0])
        fresh.set_lora_scale(SCALE)
        assert torch.equal(moved, fresh(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0]) and not torch.equal(moved, full)
    finally:
        ops.set_f32_mode(prev)


def _count_launches(fn):
    """Calls of the four LoRA entry points of hip_ops while ``fn`` runs: {name: count}."""
    from gm_diffusion import hip_ops as ops

    names = ("lora_update", "lora_update_stacked", "lora_geglu", "lora_geglu_stacked")
    calls, real = dict.fromkeys(names, 0), {n: getattr(ops, n) for n in names}

    def wrap(n):
        def f(*a, **k):
            calls[n] += 1
            return real[n](*a, **k)
        return f

    for n in names:
        setattr(ops, n, wrap(n))
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        for n in names:
            setattr(ops, n, real[n])
    return calls


def test_launch_counts_and_delete_back_to_one_adapter():
    """Modules with both adapters: one stacked launch each; modules with one: the existing launch; the total equals that of ONE
    adapter with the union target set.  delete_adapters back to one adapter: the bits of a model that only ever loaded that one."""
    ou, _, _, _, sa, sb = _refs()
    lat, ctx, _, _, _ = _unet_case()
    dx, dctx = torch.cat([lat, lat]).to(DEV), ctx.to(DEV)
    run = lambda m: (lambda: m(dx, 501, encoder_hidden_states=dctx, return_dict=False))
    two = _load_two(T1._hip_unet(ou, BF16))
    got = _count_launches(run(two))
    blocks = 16
    # (inside the stacked / single wrappers the sequential route is not taken: lora_update counts single-adapter modules only)
    assert got == {"lora_update_stacked": 8 * blocks, "lora_update": 3 * blocks, "lora_geglu": blocks, "lora_geglu_stacked": 0}, got
    union = T1._hip_unet(ou, BF16).load_lora(sb, targets="transformer")
    one = _count_launches(run(union))
    assert one == {"lora_update": 11 * blocks, "lora_geglu": blocks, "lora_update_stacked": 0, "lora_geglu_stacked": 0}, one
    assert sum(got.values()) == sum(one.values()) == 12 * blocks
    # both adapters on the feed-forward too: its update + GEGLU stays ONE launch
    sc = FR.to_convention(FR.canonical(ou, 8, 13, GAIN, alpha=4.0, families=None), "peft")
    ff = T1._hip_unet(ou, BF16).load_lora(sb, targets="transformer", adapter_name="p").load_lora(sc, targets="transformer", adapter_name="q")
    assert _count_launches(run(ff)) == {"lora_update_stacked": 11 * blocks, "lora_geglu_stacked": blocks, "lora_update": 0, "lora_geglu": 0}
    # back to one adapter
    for keep, drop, sd, kw in (("style", "subject", sa, {}), ("subject", "style", sb, dict(targets="transformer"))):
        m = T1._hip_unet(ou, BF16)
        m.load_lora(sa, adapter_name="style").load_lora(sb, targets="transformer", adapter_name="subject")
        both = m(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0].clone()
        m.delete_adapters(drop)
        only = T1._hip_unet(ou, BF16).load_lora(sd, adapter_name=keep, **kw)
        a, b = m(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0], only(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0]
        assert torch.equal(a, b) and not torch.equal(a, both), keep
        assert _count_launches(run(m)) == _count_launches(run(only))


# ---------------------------------------------------------------------------------------------------------------------------
# dual pipeline (tiny, 2 prompts, 4 PNDM steps, 64 x 64)
# ---------------------------------------------------------------------------------------------------------------------------
def _pipe(dtype, weights=WEIGHTS, controlnet=None):
    _, _, _, _, sa, sb = _refs()
    pipe = T1._pipe(dtype, adapter=False, controlnet=controlnet)
    pipe.co_run_plans = True  # one plan family for every mode
    pipe.load_lora_weights(sa, adapter_name="style")
    pipe.load_lora_weights(sb, adapter_name="subject", targets="transformer")
    pipe.set_adapters(["style", "subject"], adapter_weights=list(weights))
    return pipe


def _eq(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_pipeline_graphs_equal_eager_and_set_adapters_captures_nothing_new():
    pipe = _pipe(BF16)
    assert pipe.get_list_adapters() == {"unet": ["style", "subject"]} and pipe.get_active_adapters() == ["style", "subject"]
    pipe.use_hip_graphs, pipe.overlap_streams = False, False
    a = pipe(**T1._kw())
    pipe.use_hip_graphs, pipe.overlap_streams = True, True
    b = pipe(**T1._kw())
    torch.cuda.synchronize()
    assert _eq(a, b)
    counts = (len(pipe.unet._graphs), len(pipe.gm_unet._graphs))
    # the second call changes ONLY the weights (same prompt tensors): the cached cross-attention K / V^T must be refreshed
    kw = T1._kw()
    first = pipe(**kw)
    pipe.set_adapters(["style", "subject"], adapter_weights=[0.3, 1.1])
    c = pipe(**kw)
    torch.cuda.synchronize()
    assert (len(pipe.unet._graphs), len(pipe.gm_unet._graphs)) == counts  # no new capture
    assert _eq(first, b) and not torch.equal(c[0], b[0])
    d = _pipe(BF16, weights=(0.3, 1.1))(**T1._kw())  # a fresh pipeline given those weights from the start
    torch.cuda.synchronize()
    assert _eq(c, d)
    # an attention-only change (style alone) moves the result too: the K / V^T of attn2 carry it
    pipe.set_adapters(["style", "subject"], adapter_weights=[0.9, 1.1])
    e = pipe(**kw)
    torch.cuda.synchronize()
    assert not torch.equal(e[0], c[0]) and (len(pipe.unet._graphs), len(pipe.gm_unet._graphs)) == counts
    # the per-call scale on top of the weights, through the same graphs, gone with its call
    pipe.set_adapters(["style", "subject"], adapter_weights=[0.3, 1.1])
    h = pipe(**T1._kw(cross_attention_kwargs={"scale": 0.5}))
    again = pipe(**T1._kw())
    torch.cuda.synchronize()
    assert not torch.equal(h[0], c[0]) and _eq(again, c) and pipe.unet._lora_scale == 1.0
    assert (len(pipe.unet._graphs), len(pipe.gm_unet._graphs)) == counts


def test_pipeline_disable_and_enable_lora():
    """disable_lora(): the no-adapter result within the 16-bit gate of the one-adapter pipeline tests (2 x MEASURED_16BIT_RMS; not
    bitwise: the launches stay and an adapted block leaves ff_geglu_fused); enable_lora() restores the earlier bits."""
    pipe = _pipe(BF16)
    on = pipe(**T1._kw())
    counts = (len(pipe.unet._graphs), len(pipe.gm_unet._graphs))
    pipe.disable_lora()
    assert pipe.get_active_adapters() == [] and pipe.unet.has_lora
    off = pipe(**T1._kw())
    plain = T1._pipe(BF16, adapter=False)
    plain.co_run_plans = True
    base = plain(**T1._kw())
    torch.cuda.synchronize()
    e_sdr, e_gm = T1.rms(off[0], base[0]), T1.rms(off[1], base[1])
    m_sdr, m_gm = T1.MEASURED_16BIT_RMS[BF16]
    print(f"disable_lora vs a pipeline without adapters: latent RMS sdr={e_sdr:.3e} gm={e_gm:.3e}; the adapters move sdr by "
          f"{T1.rms(on[0], base[0]):.3e}")
    assert e_sdr <= 2 * m_sdr and e_gm <= 2 * m_gm
    assert T1.rms(on[0], base[0]) > 2 * e_sdr  # the adapters themselves move the result by far more than their zeroed launches do
    pipe.enable_lora()
    back = pipe(**T1._kw())
    torch.cuda.synchronize()
    assert _eq(back, on) and (len(pipe.unet._graphs), len(pipe.gm_unet._graphs)) == counts


def test_pipeline_two_adapters_with_controlnet_and_ip_adapter():
    import controlnet_ref as CR
    import ip_adapter_ref as IR
    from gm_diffusion.components import ControlNetModel
    from oracle import unet as OU

    torch.manual_seed(5)
    cn_ref = CR.ControlNetRef(**CR.tiny_controlnet_config()).eval().requires_grad_(False)
    cn = ControlNetModel(**CR.tiny_controlnet_config())
    cn.load_state_dict(cn_ref.state_dict())
    pipe = _pipe(BF16, controlnet=cn.to(DEV, BF16))
    pipe.load_ip_adapter(IR.make_state_dict(OU.tiny_unet_config(4), tokens=4, clip_dim=32, seed=7, gain=2.0))
    g = torch.Generator().manual_seed(8)
    cimg = torch.rand(1, 3, 64, 64, generator=g).to(DEV)
    img = torch.randn(1, 1, 32, generator=g)
    emb = [torch.cat([torch.zeros_like(img), img]).to(DEV)]
    kw = lambda **e: T1._kw(control_image=cimg, ip_adapter_image_embeds=emb, **e)
    pipe.use_hip_graphs, pipe.overlap_streams = False, False
    eager = pipe(**kw())
    pipe.use_hip_graphs, pipe.overlap_streams = True, True
    all4 = pipe(**kw())
    torch.cuda.synchronize()
    assert _eq(eager, all4)
    pipe.set_adapters(["subject"])
    no_style = pipe(**kw())
    pipe.set_adapters(["style", "subject"], list(WEIGHTS))
    no_ip = pipe(**T1._kw(control_image=cimg))
    no_cn = pipe(**kw(controlnet_conditioning_scale=0.0))
    torch.cuda.synchronize()
    for other in (no_style, no_ip, no_cn):
        assert T1.rms(all4[0], other[0]) > 1e-2
