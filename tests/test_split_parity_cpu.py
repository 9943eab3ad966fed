"""CPU: the bounds tests/test_split_parity_gpu.py holds the float32 split kernels to can FAIL.  For every GEMM and conv3x3 case of that
file (tests/split_cases.py) a clean emulation of the three-product scheme -- float16 halves, float32 accumulation, the slab sum of a
K-sliced launch, the float32 epilogue -- passes its bound with zero violations, and each of these faults is reported:

  * one of the three products dropped in a single 16x16 fragment;
  * one K step of 32 skipped in one tile;
  * one border pixel taking the wrong tap (conv);
  * one slab row left from a previous operand set (K-sliced shapes);
  * hi and lo swapped in one 4-element piece of a pre-split output.

Two limits, stated here because the GPU file inherits them:
  * A dropped LO product (a_hi w_lo or a_lo w_hi) is a float16-precision result: ~2^-12.8 |a||w| per product, random signs, so
    ~2.2e-4 / sqrt(K) of sum |a||w| over a row.  The bound's accumulation term is 2 (31 + 3K / 32 + slices) 2^-24 of the same sum: the
    fault stands above it up to K of a few hundred and sinks below it from K ~ 1000 on (tests/test_parity_cpu.py has the K = 640
    border case).  It is asserted where K <= 320; the dropped hi x hi product is asserted at every depth.  What ties the deep-K
    launches to the shallow ones beyond that is bit identity (tests/test_split_gpu.py: pre-split against in-kernel split, loader /
    converter against ring kernel), not this bound.
  * ``parity.unsplit`` reads hi + lo, which is the same number when the halves trade places: the value bound CANNOT see the swap
    (asserted below).  ``parity.split_layout_violations`` is the check that does, and every pre-split output of the GPU file goes
    through it.

Large cases are cut to a window of two tiles by two tiles (the bounds are per element: an element's bound depends on its own row of
A and of W only) with the full K, so the deepest case (K = 10240) stays a fraction of a second."""
import pytest
import torch
import torch.nn.functional as F

import parity as P
import split_cases as S

F32 = torch.float32


def _window(M, N, plan):
    bm, bn, _ = plan
    return min(M, 2 * bm + 4), min(N, 2 * bn + 8)


def _emulate_acc(a, weff, slices=1, drop=None, skip=None, stale=None):
    """A W^T as a launch of ``slices`` K slices computes it: per slice the three products of float16 halves accumulated in float32,
    the slabs then summed in order (splitk_reduce_f32_kernel).  Faults:
      drop  = (product, rows, cols): that fragment never adds "hh" (a_hi w_hi), "hl" (a_hi w_lo) or "lh" (a_lo w_hi);
      skip  = (rows, cols, k0): that tile skips the K step [k0, k0 + 32);
      stale = (slice, row, other A): that row of that slab still holds the product of another operand set."""
    ah, al = P.split_parts(a)
    wh, wl = P.split_parts(weff)
    K = a.shape[1]
    steps = K // 32
    per = -(-steps // slices) * 32
    acc = torch.zeros(a.shape[0], weff.shape[0])
    for s in range(slices):
        ks = slice(s * per, min(K, (s + 1) * per))
        parts = {"hl": ah[:, ks] @ wl[:, ks].T, "lh": al[:, ks] @ wh[:, ks].T, "hh": ah[:, ks] @ wh[:, ks].T}
        if drop is not None:
            parts[drop[0]][drop[1], drop[2]] = 0
        slab = parts["hl"] + parts["lh"] + parts["hh"]
        if skip is not None and ks.start <= skip[2] < ks.stop:
            rows, cols, k0 = skip
            kk = slice(k0, k0 + 32)
            slab[rows, cols] -= ah[rows, kk] @ wl[cols, kk].T + al[rows, kk] @ wh[cols, kk].T + ah[rows, kk] @ wh[cols, kk].T
        if stale is not None and stale[0] == s:
            r = stale[1]
            oh, ol = P.split_parts(stale[2][r:r + 1, ks])
            slab[r] = (oh @ wl[:, ks].T + ol @ wh[:, ks].T + oh @ wh[:, ks].T)[0]
        acc = acc + slab
    return acc


def _epilogue(acc, alpha, extras, act):
    """The kernels' float32 epilogue: (acc alpha + bias) + (residual + rowbias), activation, float32 store."""
    v = acc * alpha
    for t in extras:
        v = v + t.to(F32)
    return P._act_ref(v, act)


def _expect_violations(got, ref, bound, touched, what):
    bad = P.violations(got, ref, bound)[0]
    assert int(bad.sum()) > 0, f"{what}: the fault passes the bound"
    assert not bool((bad & ~touched).any()), f"{what}: violations outside the faulted elements"
    with pytest.raises(AssertionError, match="outside their bound"):
        P.assert_elementwise(got, ref, bound, what)


def _mask(shape, rows, cols=slice(None)):
    m = torch.zeros(shape, dtype=torch.bool)
    m[rows, cols] = True
    return m


CASES = {**S.GEMM_CASES, S.SECOND_LAP[0]: S.SECOND_LAP[1:]}


@pytest.mark.parametrize("form", ["plain weights", "scaled weights"])  # GMD_F32S; GMD_F32SW / GMD_F32SA (same values either way)
@pytest.mark.parametrize("case", list(CASES))
def test_gemm_bounds_pass_clean_and_report_every_fault(case, form):
    M, N, K, plan = CASES[case]
    bm, bn, slices = plan
    Mc, Nc = _window(M, N, plan)
    a, w, bias, res, rb, rpg = S.gemm_inputs(M, N, K)
    a, w, bias, res = a[:Mc], w[:Nc], bias[:Nc], res[:Mc, :Nc]
    rb = rb[:, :Nc]
    weff, alpha_w = (w, 1.0) if form == "plain weights" else S.scaled(w)
    core = S.Core(a, weff, slices)
    clean = _emulate_acc(a, weff, slices)
    frag = (slice(16, 32), slice(32, 48))
    tile = (slice(0, min(bm, Mc)), slice(0, min(bn, Nc)))
    g = torch.Generator().manual_seed(7)
    other = torch.randn(a.shape, generator=g)
    worst = 0.0
    for epi in (S.EPILOGUES if case != S.SECOND_LAP[0] else ["bias+rowbias+residual"]):
        extras, alpha, act = S.extras_of(epi, bias, rb, rpg, res, (Mc, Nc))
        ref, bound = S.ref_and_bound(core, alpha * alpha_w, extras, act)
        fin = lambda acc: _epilogue(acc, alpha * alpha_w, extras, act)
        worst = max(worst, P.assert_elementwise(fin(clean), ref, bound, f"{case} {form} {epi}: clean emulation", (bm, bn)))
        what = f"{case} {form} {epi}"
        products = ("hh", "hl", "lh") if K <= 320 else ("hh",)  # (the module docstring: the lo products' depth limit)
        for prod in products:
            _expect_violations(fin(_emulate_acc(a, weff, slices, drop=(prod, *frag))), ref, bound, _mask((Mc, Nc), *frag), f"{what}: {prod} dropped in one fragment")
        k0 = (K // 32 // 2) * 32
        _expect_violations(fin(_emulate_acc(a, weff, slices, skip=(*tile, k0))), ref, bound, _mask((Mc, Nc), *tile), f"{what}: one K step skipped in one tile")
        if slices > 1:
            row = min(Mc - 1, 37)
            _expect_violations(fin(_emulate_acc(a, weff, slices, stale=(slices - 1, row, other))), ref, bound, _mask((Mc, Nc), row), f"{what}: a stale slab row")
    print(f"PARITY-CPU gemm32 {case} {form} max|err|/bound={worst:.3f}")


def test_presplit_output_swap_is_invisible_to_the_value_bound_and_caught_by_the_layout_check():
    """The pre-split outputs of the GPU file are read through parity.unsplit and bounded by presplit_read_bound; a piece whose hi and
    lo halves trade places reads as the same values.  split_layout_violations reports exactly the four swapped elements."""
    M, N, K, plan = S.GEMM_CASES["128x160 full"]
    a, w, bias, res, rb, rpg = S.gemm_inputs(M, N, K)
    a, w, bias = a[:132], w[:320], bias[:320]
    weff, alpha_w = S.scaled(w)
    core = S.Core(a, weff, 1)
    extras, alpha, act = S.extras_of("silu", bias, None, rpg, None, (132, 320))
    ref, bound = S.ref_and_bound(core, alpha * alpha_w, extras, act)
    out = _epilogue(_emulate_acc(a, weff), alpha * alpha_w, extras, act)
    stored = P.split_store(out)
    rb_ = P.presplit_read_bound(ref, bound)
    P.assert_elementwise(P.unsplit(stored), ref, rb_, "clean pre-split output")
    assert not bool(P.split_layout_violations(stored).any())
    assert torch.equal(P.unsplit(stored), sum(t.double() for t in P.split_parts(out)))
    # swap hi and lo of ONE 8-byte piece: row 70, chunk 3, q = 2, the low 16 elements -> elements 96 + 8 .. 96 + 11
    h = stored.view(torch.float16).reshape(132, 320 // 32, 2, 4, 2, 4).clone()
    h[70, 3, :, 2, 0] = h[70, 3, :, 2, 0].flip(0)
    swapped = h.reshape(-1).view(F32).reshape(132, 320)
    assert int(P.violations(P.unsplit(swapped), ref, rb_)[0].sum()) == 0, "hi + lo is symmetric: the value bound cannot see the swap"
    bad = P.split_layout_violations(swapped)
    want = _mask((132, 320), 70, slice(104, 108))
    assert torch.equal(bad, want), f"the layout check reports {int(bad.sum())} elements, expected elements 104..107 of row 70"
    # a value the layout cannot hold (beyond float16's range) is reported too, and tiny values (subnormal halves) are not
    assert bool(P.split_layout_violations(P.split_store(torch.full((1, 32), 1.0e5))).all())
    assert not bool(P.split_layout_violations(P.split_store(torch.randn(4, 64) * 2.0 ** -20)).any())
    # the residual term of presplit_read_bound is needed: without it the clean stored tensor breaks the plain float32 store's bound
    # wherever the kernel's own error is small against 2^-22 |x| -- here, on values rounded to float32 exactly
    exact = torch.randn(64, 64, generator=torch.Generator().manual_seed(3))
    zero = torch.zeros(64, 64, dtype=torch.float64)
    assert int(P.violations(P.unsplit(P.split_store(exact)), exact.double(), zero)[0].sum()) > 0
    P.assert_elementwise(P.unsplit(P.split_store(exact)), exact.double(), P.presplit_read_bound(exact.double(), zero), "split residual alone")


@pytest.mark.parametrize("mode", S.MODES)
def test_im2col_reference_is_the_convolution(mode):
    """The explicit im2col matrix times the tap-major weight IS F.conv2d in float64 (odd maps, every mode; F.interpolate confirms the
    nearest map of the odd upsampled sizes)."""
    g = torch.Generator().manual_seed(len(mode))
    for B, H, W, C, co, odd in [(2, 23, 20, 8, 6, (45, 39)), (1, 9, 7, 4, 5, (17, 14)), (1, 6, 6, 3, 2, (12, 11)), (2, 5, 4, 2, 3, (9, 7))]:
        x = torch.randn(B, H * W, C, generator=g, dtype=torch.float64)
        w = torch.randn(co, 9 * C, generator=g, dtype=torch.float64)
        kw = S.conv_kw(mode, odd)
        m, ho, wo = P.im2col3x3(x, B, H, W, **kw)
        xi = x.view(B, H, W, C).permute(0, 3, 1, 2)
        wt = w.view(co, 3, 3, C).permute(0, 3, 1, 2)
        if mode == "up":
            xi = F.interpolate(xi, scale_factor=2, mode="nearest")
        elif mode == "up_to_odd":
            xi = F.interpolate(xi, size=odd, mode="nearest")
        y = F.conv2d(F.pad(xi, (0, 1, 0, 1)), wt, stride=2) if mode == "pad1" else F.conv2d(xi, wt, stride=2 if mode == "s2" else 1, padding=1)
        assert (ho, wo) == tuple(y.shape[-2:]) and m.shape == (B * ho * wo, 9 * C)
        ref = y.permute(0, 2, 3, 1).reshape(B * ho * wo, co)
        assert float(((m @ w.T) - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), (mode, H, W)
        assert m.dtype == x.dtype and bool(torch.isin(m, torch.cat([x.reshape(-1), x.new_zeros(1)])).all()), "pure indexing: x's own values and zeros"


def test_case_table_is_pairwise_covering():
    cases = S.CONV_CASES
    assert len(cases) == len(set(cases)) == 25
    for mode in S.MODES:
        assert {f for m, f, t in cases if m == mode} == set(S.FORMS), mode
        assert {t for m, f, t in cases if m == mode} == set(S.CONV_TILES), mode
    for tile in S.CONV_TILES:
        assert {f for m, f, t in cases if t == tile} == set(S.FORMS), tile


@pytest.mark.parametrize("mode,form,tile", S.CONV_CASES)
def test_conv_bounds_pass_clean_and_report_every_fault(mode, form, tile):
    x, w, bias, tb, res, B, H, W, ho, wo, kw = S.conv_inputs(tile, mode)
    _, ci, co, _, plan = S.CONV_TILES[tile]
    bm, bn, slices = plan
    amat, _, _ = P.im2col3x3(x, B, H, W, **kw)
    M = B * ho * wo
    Mc, Nc = _window(M, co, plan)
    extras = [t[:Mc, :Nc] for t in S.conv_extras(bias, tb, res, B, ho * wo, co)]
    a, wc = amat[:Mc], w[:Nc]
    weff, alpha_w = (wc, 1.0) if form == "F32S" else S.scaled(wc)
    core = S.Core(a, weff, slices)
    ref, bound = S.ref_and_bound(core, alpha_w, extras, None)
    fin = lambda acc: _epilogue(acc, alpha_w, extras, None)
    what = f"conv {tile} {mode} {form}"
    r = P.assert_elementwise(fin(_emulate_acc(a, weff, slices)), ref, bound, what + ": clean emulation", (bm, bn))
    print(f"PARITY-CPU conv32 {tile} {mode} {form} max|err|/bound={r:.3f}")
    # a border pixel whose padding tap reads a pixel instead of zeros: the centre tap's (what clamping the coordinate would fetch)
    pad = (a.view(Mc, 9, ci) == 0).all(-1)
    assert bool(pad.any()), "the window holds no border pixel"
    row, tap = (int(v) for v in pad.nonzero()[0])
    wrong = a.clone().view(Mc, 9, ci)
    wrong[row, tap] = wrong[row, 4]
    _expect_violations(fin(_emulate_acc(wrong.view(Mc, 9 * ci), weff, slices)), ref, bound, _mask((Mc, Nc), row), what + f": pixel {row} reads a pixel for padding tap {tap}")
    frag, tl = (slice(16, 32), slice(32, 48)), (slice(0, min(bm, Mc)), slice(0, min(bn, Nc)))
    _expect_violations(fin(_emulate_acc(a, weff, slices, drop=("hh", *frag))), ref, bound, _mask((Mc, Nc), *frag), what + ": hh dropped in one fragment")
    if 9 * ci <= 320:
        for prod in ("hl", "lh"):
            _expect_violations(fin(_emulate_acc(a, weff, slices, drop=(prod, *frag))), ref, bound, _mask((Mc, Nc), *frag), what + f": {prod} dropped in one fragment")
    k0 = 4 * ci + (ci // 32 // 2) * 32  # a K step of the centre tap: no pixel of the tile reads padding there
    _expect_violations(fin(_emulate_acc(a, weff, slices, skip=(*tl, k0))), ref, bound, _mask((Mc, Nc), *tl), what + ": one K step skipped in one tile")
    if slices > 1:
        other = torch.randn(a.shape, generator=torch.Generator().manual_seed(7))
        _expect_violations(fin(_emulate_acc(a, weff, slices, stale=(1, 5, other))), ref, bound, _mask((Mc, Nc), 5), what + ": a stale slab row")
    if tile == "64x64":  # the exact-mode (GMD_F32) leg of every mode: a float32 FMA chain passes its bound, the wrong tap does not
        value, eb = S.exact_ref_and_bound(a, wc, extras)
        exact = lambda m: _epilogue(m @ wc.T, 1.0, extras, None)
        P.assert_elementwise(exact(a), value, eb, what + ": exact float32, clean")
        _expect_violations(exact(wrong.view(Mc, 9 * ci)), value, eb, _mask((Mc, Nc), row), what + ": exact float32, wrong tap")
