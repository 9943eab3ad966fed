"""The per-element checker (tests/parity.py) tested without a GPU: CPU emulations of the kernels' arithmetic (16-bit inputs, float32
accumulation, float32 epilogue, ONE rounding of the stored value) must pass with zero violations in any summation order, and every
injected fault of the kind tiled kernels really have must be caught on most of the elements it touches.  Next to each fault: what
the global-norm threshold of the corresponding GPU test (|got - ref| / |ref| over the whole output) makes of it."""
import math

import pytest
import torch
import torch.nn.functional as F

import parity as P

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _caught(got, ref, bound, touched, what):
    """The fault must raise, and break the bound on MOST of the elements it touched (a fault that hides inside correct rounding on
    most of them would be a badly chosen fault, not a loose bound)."""
    with pytest.raises(AssertionError, match="outside their bound"):
        P.assert_elementwise(got, ref, bound, what, tile=(64, 64))
    bad, _, _, _ = P.violations(got, ref, bound)
    assert not bool((bad & ~touched).any()), f"{what}: violations outside the injected fault"
    frac = float(bad[touched].double().mean())
    assert frac > 0.5, f"{what}: only {frac:.2f} of the touched elements exceed their bound"


# ---------------------------------------------------------------------------------------------------------------------------
# the checker itself
# ---------------------------------------------------------------------------------------------------------------------------
def test_checker_allows_no_violation_and_reports_the_fragment():
    ref = torch.zeros(256, 320, dtype=torch.float64)
    bound = torch.full_like(ref, 1e-3)
    got = ref.clone()
    assert P.assert_elementwise(got, ref, bound, "clean") == 0.0
    got[200, 170] = 2e-3  # ONE element of 81920
    got[70, 3] = 1.5e-3
    with pytest.raises(AssertionError) as ei:
        P.assert_elementwise(got, ref, bound, "two", tile=(128, 160))
    msg = str(ei.value)
    assert "2 of 81920" in msg and "(200, 170)" in msg and "row block 1, column block 1" in msg and "(72, 10) inside" in msg
    assert "2 distinct tiles" in msg and "bound 1.000e-03" in msg
    got = ref.clone()
    got[5, 5] = float("nan")
    with pytest.raises(AssertionError, match="1 of 81920"):
        P.assert_elementwise(got, ref, bound, "nan")
    got[5, 5] = float("inf")
    with pytest.raises(AssertionError, match="1 of 81920"):
        P.assert_elementwise(got, ref, bound, "inf")
    got[5, 5] = 1e-3  # exactly on the bound is inside
    P.assert_elementwise(got, ref, bound, "edge")


def test_lipschitz_constants_and_activation_evaluation_bounds():
    x = torch.linspace(-30, 30, 2_000_001, dtype=torch.float64, requires_grad=True)
    for act, lip in (("silu", P.LIP_SILU), ("quick_gelu", P.LIP_QUICK_GELU), ("gelu", P.LIP_GELU)):
        (g,) = torch.autograd.grad(P._act_ref(x, act).sum(), x)
        assert float(g.abs().max()) <= lip < float(g.abs().max()) * 1.001, act  # an upper bound, and a tight one
    # the evaluation-error model against a float32 emulation of silu_f (exp and reciprocal correctly rounded here: the model,
    # which allows one ulp for each, must cover it)
    xf = torch.linspace(-100, 100, 1_000_001, dtype=torch.float32)
    emu = xf * (1.0 / (1.0 + torch.exp(-xf)))
    assert bool(((emu.double() - F.silu(xf.double())).abs() <= P.act_eval_error(xf.double(), "silu")).all())


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------------------------------
def _acc(a, w, order):
    """float32 accumulation of the exact 16-bit products in one of several summation orders."""
    af, wf = a.float(), w.float()
    K = af.shape[1]
    if order == "plain":
        return af @ wf.T
    if order == "reversed":
        return af.flip(1) @ wf.flip(1).T
    n = int(order)  # K split in n slices of whole 64-steps, re-added in slice order (split-K / fix-up)
    steps = K // 64
    cuts = [64 * (steps * i // n) for i in range(n + 1)]
    acc = None
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if hi > lo:
            part = af[:, lo:hi] @ wf[:, lo:hi].T
            acc = part if acc is None else acc + part
    return acc


def _epilogue(acc, alpha, bias, rb_rows, res, act, out_dtype):
    v = alpha * acc
    if bias is not None:
        v = v + bias
    if rb_rows is not None:
        v = v + rb_rows
    if res is not None:
        v = v + res.float()
    if act == "silu":
        v = v * (1.0 / (1.0 + torch.exp(-v)))
    elif act == "quick_gelu":
        v = v / (1.0 + torch.exp(-1.702 * v))
    return v.to(out_dtype)


def _gemm_case(M, N, K, dtype, seed=None, rpg=1000):
    g = torch.Generator().manual_seed(M + N + K if seed is None else seed)  # the generators of test_gemm_nt
    a = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dtype)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g).to(dtype)
    rb = torch.randn((M + rpg - 1) // rpg, N, generator=g)
    return a, w, bias, res, rb


def _gemm_ref_bound(a, w, bias, rb_rows, res, alpha, act, out_dtype):
    ref_acc = a.double() @ w.double().T
    abs_dot = a.double().abs() @ w.double().abs().T
    extras = [t.double() for t in (bias, rb_rows, res) if t is not None]
    value, _ = P.preact_bound(ref_acc, abs_dot, a.shape[1], alpha, extras)
    return P._act_ref(value, act), P.gemm_bound(ref_acc, abs_dot, a.shape[1], out_dtype, alpha, extras, act)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("M,N,K", [(128, 160, 64), (256, 320, 320), (1000, 328, 320), (1000, 384, 1280), (520, 256, 1920), (1024, 1280, 5120)])
def test_clean_gemm_emulation_passes_in_every_summation_order(M, N, K, dtype):
    a, w, bias, res, rb = _gemm_case(M, N, K, dtype, rpg=37)
    rb_rows = rb.repeat_interleave(37, 0)[:M]
    for act in (None, "silu", "quick_gelu"):
        for out_dtype in (dtype, F32):
            ref, bound = _gemm_ref_bound(a, w, bias, rb_rows, res, 0.5, act, out_dtype)
            for order in ("plain", "reversed", 2, 3, 5, 7):
                if isinstance(order, int) and K // 64 < order:
                    continue
                got = _epilogue(_acc(a, w, order), 0.5, bias, rb_rows, res, act, out_dtype)
                r = P.assert_elementwise(got, ref, bound, f"{M}x{N}x{K} {dtype} -> {out_dtype} act {act} order {order}", tile=(64, 64))
                assert r <= 1.0


def test_clean_geglu_emulation_passes():
    g = torch.Generator().manual_seed(11)
    M, C = 512, 320
    x = torch.randn(M, C, generator=g).bfloat16()
    w1 = (torch.randn(8 * C, C, generator=g) * 0.05).bfloat16()
    b1 = torch.randn(8 * C, generator=g) * 0.5
    h32 = x.float() @ w1.float().T + b1
    got = (h32[:, :4 * C] * F.gelu(h32[:, 4 * C:])).bfloat16()
    acc = x.double() @ w1.double().T
    ad = x.double().abs() @ w1.double().abs().T
    val, ev = P.preact_bound(acc[:, :4 * C], ad[:, :4 * C], C, 1.0, [b1[:4 * C].double()])
    gate, eg = P.preact_bound(acc[:, 4 * C:], ad[:, 4 * C:], C, 1.0, [b1[4 * C:].double()])
    P.assert_elementwise(got, val * F.gelu(gate), P.geglu_bound(val, ev, gate, eg, BF16), "geglu")


@pytest.fixture(scope="module")
def big():
    """The largest GEMM of the family: M = 16384, N = 1280, K = 640, bias + rowbias (seam every 1000 rows: inside tiles) +
    residual, alpha = 0.5, bf16."""
    M, N, K = 16384, 1280, 640
    a, w, bias, res, rb = _gemm_case(M, N, K, BF16)
    rb_rows = rb.repeat_interleave(1000, 0)[:M]
    ref, bound = _gemm_ref_bound(a, w, bias, rb_rows, res, 0.5, None, BF16)
    clean = _epilogue(_acc(a, w, "plain"), 0.5, bias, rb_rows, res, None, BF16)
    return dict(a=a, w=w, bias=bias, res=res, rb=rb, rb_rows=rb_rows, ref=ref, bound=bound, clean=clean)


def _block(big, rows, cols, a=None, w=None, bias=None, rb_rows=None, res="keep"):
    """Recompute one block of the big case with some of its operands replaced (the injected fault)."""
    A = big["a"][rows] if a is None else a
    W = big["w"][cols] if w is None else w
    b = big["bias"][cols] if bias is None else bias
    rbr = big["rb_rows"][rows][:, cols] if rb_rows is None else rb_rows
    r = big["res"][rows][:, cols] if isinstance(res, str) else res
    return _epilogue(A.float() @ W.float().T, 0.5, b, rbr, r, None, BF16)


def _mask(big, rows, cols):
    m = torch.zeros(big["ref"].shape, dtype=torch.bool)
    m[rows, cols] = True
    return m


def test_big_gemm_clean_passes(big):
    r = P.assert_elementwise(big["clean"], big["ref"], big["bound"], "clean 16384x1280x640", tile=(128, 160))
    assert 0.5 < r <= 1.0  # bf16 rounding alone reaches the bound's neighbourhood: the bound is not loose
    assert _rel(big["clean"], big["ref"]) < 2.5e-3


def test_fault_last_row_left_zero(big):
    got = big["clean"].clone()
    got[-1] = 0
    assert _rel(got, big["ref"]) < 1.2e-2  # the global-norm threshold of test_gemm_nt / the epilogue fuzz (1.2e-2) does NOT catch this
    _caught(got, big["ref"], big["bound"], _mask(big, slice(16383, 16384), slice(None)), "last row zero")


def test_fault_corner_of_garbage(big):
    got = big["clean"].clone()
    got[-16:, -8:] = (torch.randn(16, 8, generator=torch.Generator().manual_seed(1)) * 2).bfloat16()
    assert _rel(got, big["ref"]) < 1.2e-2  # 4.1e-3: NOT caught by 1.2e-2, and on the edge of the 4e-3 of tests/test_pp_gpu.py (N(0, 1) garbage: 3.4e-3)
    _caught(got, big["ref"], big["bound"], _mask(big, slice(16368, 16384), slice(1272, 1280)), "16x8 corner of garbage")


def test_fault_one_tile_skips_one_k_step(big):
    rows, cols = slice(4096 + 64, 4096 + 128), slice(640, 704)
    a = big["a"][rows].clone()
    a[:, 128:192] = 0  # the tile never accumulated K step 2
    got = big["clean"].clone()
    got[rows, cols] = _block(big, rows, cols, a=a)
    assert _rel(got, big["ref"]) < 4e-3  # not caught by 1.2e-2, nor by 4e-3
    _caught(got, big["ref"], big["bound"], _mask(big, rows, cols), "64x64 tile skipped a K step")


def test_fault_two_adjacent_rows_swapped(big):
    got = big["clean"].clone()
    got[[777, 778]] = got[[778, 777]]
    assert _rel(got, big["ref"]) < 1.2e-2  # not caught by 1.2e-2 (about 1.1e-2: two rows of 16384)
    _caught(got, big["ref"], big["bound"], _mask(big, slice(777, 779), slice(None)), "rows 777 / 778 swapped")


def test_fault_bias_shifted_by_one_fragment(big):
    rows, cols = slice(8192, 8256), slice(160, 176)
    got = big["clean"].clone()
    got[rows, cols] = _block(big, rows, cols, bias=big["bias"][176:192])
    assert _rel(got, big["ref"]) < 1.2e-2  # not caught by 1.2e-2
    _caught(got, big["ref"], big["bound"], _mask(big, rows, cols), "bias of the next 16-column fragment")


def test_fault_rowbias_of_the_neighbouring_group_after_a_seam(big):
    rows = slice(1000, 1001)  # first row of group 1 takes group 0's row bias
    got = big["clean"].clone()
    got[rows] = _block(big, rows, slice(None), rb_rows=big["rb"][0:1])
    assert _rel(got, big["ref"]) < 1.2e-2  # not caught by 1.2e-2 (one row)
    _caught(got, big["ref"], big["bound"], _mask(big, rows, slice(None)), "row bias across the group seam")


def test_fault_residual_skipped_on_the_edge_tile(big):
    rows, cols = slice(16384 - 128, 16384), slice(1280 - 160, 1280)
    got = big["clean"].clone()
    got[rows, cols] = _block(big, rows, cols, res=None)
    assert _rel(got, big["ref"]) < 4e-2  # a whole tile without its residual: 3.1e-2, the one fault of this list the global norm does catch
    _caught(got, big["ref"], big["bound"], _mask(big, rows, cols), "residual skipped on the last tile")


def _clean_violations(case):
    """Number of elements of a CLEAN emulation outside the bound as parity.DISABLED leaves it."""
    if case == "gemm16":  # 16-bit store
        a, w, bias, res, rb = _gemm_case(256, 320, 320, BF16, rpg=37)
        rbr = rb.repeat_interleave(37, 0)[:256]
        ref, bound = _gemm_ref_bound(a, w, bias, rbr, res, 0.5, None, BF16)
        got = _epilogue(_acc(a, w, "plain"), 0.5, bias, rbr, res, None, BF16)
    elif case == "gemm32":  # float32 store, deep K, reversed order: the accumulation error shows
        a, w, _, _, _ = _gemm_case(1024, 1280, 5120, BF16)
        ref, bound = _gemm_ref_bound(a, w, None, None, None, 1.0, None, F32)
        got = _epilogue(_acc(a, w, "reversed"), 1.0, None, None, None, None, F32)
    elif case in ("split_small", "split_scaled"):
        g = torch.Generator().manual_seed(7)
        a = torch.randn(256, 320, generator=g)
        w = torch.randn(320, 320, generator=g) / math.sqrt(320) * (2.0 ** -6 if case == "split_small" else 64.0)
        ah, al = P.split_parts(a)
        wh, wl = P.split_parts(w)
        got = ah.double() @ wh.double().T + ah.double() @ wl.double().T + al.double() @ wh.double().T  # the three products, summed exactly
        ref = a.double() @ w.double().T
        bound = P.split_product_bound(a, w)
    elif case == "attention":
        g = torch.Generator().manual_seed(64 * 7 + 1024)
        q, k, v = (torch.randn(n, 64, generator=g).bfloat16() for n in (200, 1024, 1024))
        ref, bound = P.attention_bound(q, k, v, 0.125, BF16)
        got = _attn_emulation(q, k, v, 0.125, BF16)
    elif case == "attention40":
        g = torch.Generator().manual_seed(40 * 7 + 1024)
        q, k, v = (torch.randn(n, 40, generator=g).bfloat16() for n in (200, 1024, 1024))
        ref, bound = P.attention_bound(q, k, v, 40 ** -0.5, BF16)
        got = _attn_emulation(q, k, v, 40 ** -0.5, BF16, q_rounded=True)
    elif case in ("groupnorm32", "groupnorm16"):
        dt = F32 if case == "groupnorm32" else BF16
        g = torch.Generator().manual_seed(320 + 4096)
        x = (torch.randn(1, 4096, 320, generator=g) * 2 + 0.5).to(dt)
        gamma, beta = torch.randn(320, generator=g), torch.randn(320, generator=g)
        ref, bound = P.groupnorm_ref_bound(x, 32, gamma, beta, 1e-5, dt, 4096 * 10 // 256 + 16, False)
        got = _gn_emulation(x, 32, gamma, beta, 1e-5, False)
    return int(P.violations(got, ref, bound)[0].sum())


@pytest.mark.parametrize("terms,case", [
    (("out_round",), "gemm16"), (("accumulate",), "gemm32"), (("split_abs",), "split_small"), (("split_rel",), "split_scaled"),
    (("attn_p_round", "out_round"), "attention"), (("attn_p_round", "out_round", "attn_q_round"), "attention40"),
    (("norm_stats",), "groupnorm32"), (("out_round",), "groupnorm16"),
])
def test_switching_a_bound_term_off_breaks_a_clean_case(terms, case):
    """Every term of the bounds that CAN be shown necessary by a correct computation is: with it switched off (parity.DISABLED) a
    clean emulation breaks the bound, with it on the same emulation passes.  The three 16-bit roundings of attention each stay
    below the sum of the others on these inputs (P |V| >= |O|), so they are switched off together; for head dim 40 the worst-case
    allowance for the rounded Q covers the P roundings as well and goes with them.  NOT demonstrable this way, because the
    worst-case accumulation / statistics terms beside them are far above what a correct computation uses: the float32 epilogue
    adds ("epilogue"), the activation evaluation error ("act_eval") and the norm evaluation term ("norm_eval") -- they are
    derived, a few 2^-24 each, and only ever matter for float32 outputs."""
    assert not P.DISABLED and _clean_violations(case) == 0
    try:
        P.DISABLED.update(terms)
        assert _clean_violations(case) > 0, f"without {terms} the clean {case} emulation still passes: the term is not needed there"
    finally:
        P.DISABLED.clear()


def test_one_allowed_violation_would_hide_a_single_wrong_element(big):
    """The allowed number of violations is 0: ONE wrong element of 21 million is reported."""
    got = big["clean"].clone()
    got[12345, 678] += 0.25
    with pytest.raises(AssertionError, match="1 of 20971520 elements"):
        P.assert_elementwise(got, big["ref"], big["bound"], "one element", tile=(128, 160))


# ---------------------------------------------------------------------------------------------------------------------------
# float32 on the matrix cores: the three-product split
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wscale", [1.0, 64.0, 2.0 ** -6])
@pytest.mark.parametrize("M,N,K", [(256, 320, 320), (300, 200, 1280)])
def test_split_emulation_confirms_the_derivation(M, N, K, wscale):
    """hi = f16(x), lo = f16(x - hi), three float32-accumulated products.  With N(0, 1/K) weights every |w| < 2^-3: the lo halves
    are float16 subnormals and the ABSOLUTE term of split_product_bound covers them.  At |w| ~ 2^-5 the relative term's worst-case
    sum still happens to cover the (randomly signed) absolute errors; for weights another 2^-6 smaller it no longer does -- without
    the absolute term the exact three-product sum breaks the bound (asserted below), which is why scale_weight exists; weights
    scaled by 64 need the relative term only."""
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K) * wscale
    got = P.split_matmul_emulation(a, w) / wscale
    ref_acc = a.double() @ w.double().T
    abs_dot = a.double().abs() @ w.double().abs().T
    perr = P.split_product_bound(a, w)
    bound = P.gemm_bound(ref_acc, abs_dot, 3 * K, F32, 1.0 / wscale, (), None, product_err=perr)
    r = P.assert_elementwise(got, ref_acc / wscale, bound, f"split {M}x{N}x{K} x{wscale}")
    # the products' own error alone (float64 sum of the float16 halves' exact products): the derivation, term by term
    ah, al = P.split_parts(a)
    wh, wl = P.split_parts(w)
    exact3 = ah.double() @ wh.double().T + ah.double() @ wl.double().T + al.double() @ wh.double().T
    assert bool(((exact3 - ref_acc).abs() <= perr).all())
    rel_only = 3 * 2.0 ** -22 * abs_dot
    n_bad = int(((exact3 - ref_acc).abs() > rel_only).sum())
    if wscale < 1.0:
        assert n_bad > 0, "subnormal lo halves must need the absolute term"
    if wscale > 1.0:
        assert n_bad == 0
    assert r <= 1.0


def test_split_fault_is_caught():
    g = torch.Generator().manual_seed(3)
    M, N, K = 1024, 640, 640
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K) * 64
    ref_acc = a.double() @ w.double().T
    bound = P.gemm_bound(ref_acc, a.double().abs() @ w.double().abs().T, 3 * K, F32, 1.0, (), None, product_err=P.split_product_bound(a, w))
    ah, al = P.split_parts(a)
    wh, wl = P.split_parts(w)
    got = ah @ wh.T + (ah @ wl.T + al @ wh.T)
    P.assert_elementwise(got, ref_acc, bound, "split clean")
    bad = got.clone()
    rows, cols = slice(128, 192), slice(64, 128)
    k0 = slice(0, 608)  # one tile skipped the last K step of 32
    bad[rows, cols] = ah[rows, k0] @ wh[cols, k0].T + (ah[rows, k0] @ wl[cols, k0].T + al[rows, k0] @ wh[cols, k0].T)
    m = torch.zeros(M, N, dtype=torch.bool)
    m[rows, cols] = True
    _caught(bad, ref_acc, bound, m, "one tile skipped a K step of 32")
    # (A tile that drops ONE lo product -- a float16-precision result, ~2^-12 per product with random signs -- is below the worst-case
    # accumulation term 2 * 3K * 2^-24 sum |a||w| at this K: a blind spot of an order-agnostic bound;
    # test_split_dropped_lo_product_is_caught_along_the_kernels_k_loop catches it with the bound taken along the kernel's K loop.)


def _blocked_split_matmul(ah, al, wh, wl, drop_lo=None):
    """The split kernels' K loop (csrc/gemm_split.hip): per block of 32 k's three matrix-core instructions, small terms first, all
    chained through ONE float32 accumulator.  drop_lo = (rows, cols): that tile never issues the a_lo w_hi instruction."""
    acc = torch.zeros(ah.shape[0], wh.shape[0])
    for k in range(0, ah.shape[1], 32):
        ks = slice(k, k + 32)
        acc = acc + ah[:, ks] @ wl[:, ks].T
        t = al[:, ks] @ wh[:, ks].T
        if drop_lo is not None:
            t[drop_lo[0], drop_lo[1]] = 0
        acc = acc + t
        acc = acc + ah[:, ks] @ wh[:, ks].T
    return acc


def test_split_dropped_lo_product_is_caught_along_the_kernels_k_loop():
    """With the accumulation term taken along the kernel's own K loop (parity.mfma_height: 31 + 3K / 32 + slices additions instead
    of 3K in an unknown order) a tile that drops one lo product -- a float16-precision result -- is reported at the product's depth,
    K = 640, which the order-agnostic bound cannot do."""
    g = torch.Generator().manual_seed(3)
    M, N, K = 512, 384, 640
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K) * 64
    ref_acc = a.double() @ w.double().T
    abs_dot = a.double().abs() @ w.double().abs().T
    bound = P.gemm_bound(ref_acc, abs_dot, 3 * K, F32, 1.0, (), None, product_err=P.split_product_bound(a, w), height=P.mfma_height(3 * K, 32, 16))
    loose = P.gemm_bound(ref_acc, abs_dot, 3 * K, F32, 1.0, (), None, product_err=P.split_product_bound(a, w))
    assert float((loose / bound).min()) > 15
    ah, al = P.split_parts(a)
    wh, wl = P.split_parts(w)
    P.assert_elementwise(_blocked_split_matmul(ah, al, wh, wl), ref_acc, bound, "split clean, blocked K loop")
    rows, cols = slice(128, 192), slice(64, 128)
    bad = _blocked_split_matmul(ah, al, wh, wl, drop_lo=(rows, cols))
    m = torch.zeros(M, N, dtype=torch.bool)
    m[rows, cols] = True
    with pytest.raises(AssertionError, match="1 distinct tiles hold violations"):
        P.assert_elementwise(bad, ref_acc, bound, "a_lo w_hi dropped on one tile, K = 640", tile=(64, 64))
    viol = P.violations(bad, ref_acc, bound)[0]
    # reported, and only inside the tile -- on about a third of its elements, not on most: the lost products carry random signs and sum
    # to ~sqrt(K) 2^-12 |a||w|, which clears a worst-case bound of 2 * 92..107 * 2^-24 sum |a||w| only where they happen to line up
    assert not bool((viol & ~m).any()) and float(viol[m].double().mean()) > 0.2
    assert int(P.violations(bad, ref_acc, loose)[0].sum()) == 0  # the unknown-order bound does not see it at all


def test_split_dropped_lo_product_is_caught_at_shallow_k():
    """One tile computes a_hi w_hi + a_hi w_lo only.  With K = 32 (one K step of the split kernels) the accumulation allowance is 96
    additions and the lost a_lo w_hi products -- 2^-12 |a||w| each -- stand above it on most elements."""
    g = torch.Generator().manual_seed(5)
    M, N, K = 256, 256, 32
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 64
    ref_acc = a.double() @ w.double().T
    bound = P.gemm_bound(ref_acc, a.double().abs() @ w.double().abs().T, 3 * K, F32, 1.0, (), None, product_err=P.split_product_bound(a, w))
    ah, al = P.split_parts(a)
    wh, wl = P.split_parts(w)
    got = ah @ wh.T + (ah @ wl.T + al @ wh.T)
    P.assert_elementwise(got, ref_acc, bound, "split clean K=32")
    rows, cols = slice(64, 128), slice(128, 192)
    got[rows, cols] = ah[rows] @ wh[cols].T + ah[rows] @ wl[cols].T
    m = torch.zeros(M, N, dtype=torch.bool)
    m[rows, cols] = True
    _caught(got, ref_acc, bound, m, "a_lo w_hi dropped on one tile")


# ---------------------------------------------------------------------------------------------------------------------------
# conv3x3
# ---------------------------------------------------------------------------------------------------------------------------
def _conv(x, w, B, H, W, stride=1, upsample=False, pad_mode=0, dt=torch.float32):
    """x [B, H*W, Cin], w [Cout, 9*Cin] tap-major -> [B, Ho*Wo, Cout] in ``dt`` arithmetic."""
    ci, co = x.shape[-1], w.shape[0]
    xi = x.to(dt).view(B, H, W, ci).permute(0, 3, 1, 2)
    wt = w.to(dt).view(co, 3, 3, ci).permute(0, 3, 1, 2)
    if upsample:
        xi = F.interpolate(xi, scale_factor=2, mode="nearest")
    y = F.conv2d(F.pad(xi, (0, 1, 0, 1)), wt, stride=2) if pad_mode == 1 else F.conv2d(xi, wt, stride=stride, padding=1)
    return y.permute(0, 2, 3, 1).reshape(B, -1, co)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("kw", [dict(), dict(stride=2), dict(upsample=True), dict(stride=2, pad_mode=1)])
def test_clean_conv_emulation_passes_and_faults_are_caught(kw, dtype):
    g = torch.Generator().manual_seed(len(kw) + 21)  # the generators of test_lc_kernel_conv3x3_vs_float64
    B, H, W, ci, co = 3, 23, 20, 128, 320
    x = torch.randn(B, H * W, ci, generator=g).to(dtype)
    w = (torch.randn(co, 9 * ci, generator=g) * 0.03).to(dtype)
    b = torch.randn(co, generator=g)
    tb = torch.randn(B, co, generator=g)
    acc32 = _conv(x, w, B, H, W, **kw)
    ref_acc = _conv(x, w, B, H, W, dt=torch.float64, **kw)
    abs_dot = _conv(x.double().abs(), w.double().abs(), B, H, W, dt=torch.float64, **kw)
    extras = [b.double().expand_as(ref_acc), tb.double()[:, None, :].expand_as(ref_acc)]
    ref = ref_acc + extras[0] + extras[1]
    bound = P.gemm_bound(ref_acc, abs_dot, 9 * ci, dtype, 1.0, extras, None)
    got = (acc32 + b + tb[:, None, :]).to(dtype)
    P.assert_elementwise(got, ref, bound, f"conv {kw} {dtype}", tile=(64, 64))
    # fault: the last output pixel of the last sample left unwritten (zero).  (One row of these 345 .. 1840: the global norm sees 2.4e-2 ..
    # 5.4e-2 here; at the 16384+ rows of the product's launches it is the 7.9e-3 of the GEMM case above: NOT caught by 1.2e-2.)
    bad = got.clone()
    bad[-1, -1] = 0
    m = torch.zeros_like(bad, dtype=torch.bool)
    m[-1, -1] = True
    _caught(bad, ref, bound, m, "last pixel unwritten")
    # fault: one 64-pixel x 64-channel fragment skipped the centre tap's first 64 input channels (one K step of 18): 1.4e-2 .. 2.5e-2 in
    # the global norm of these small tensors (4096 faulty elements of 110400 .. 588800), under 4e-3 from 16384 rows up
    xz = x.clone().float()
    wz = w.clone().float()
    wz.view(co, 9, ci)[:, 4, :64] = 0
    part = _conv(xz, wz, B, H, W, **kw) + b + tb[:, None, :]
    bad = got.clone()
    bad[1, 64:128, 64:128] = part[1, 64:128, 64:128].to(dtype)
    m = torch.zeros_like(bad, dtype=torch.bool)
    m[1, 64:128, 64:128] = True
    _caught(bad, ref, bound, m, "fragment skipped one K step of the centre tap")


# ---------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------
def _attn_emulation(q, k, v, scale, dtype, leak=None, wrong_sum_row=None, q_rounded=False):
    """float32 scores, P rounded to 16 bits, float32 P V and row sum of the rounded P, output rounded.  q [Nq, D], k, v [Nk, D].
    leak = (key row, value row): one pad column of the ragged last tile is NOT masked.  wrong_sum_row: that query row is divided
    by its neighbour's row sum.  q_rounded: the lagged-stabiliser kernel's Q, pre-multiplied by the scale and rounded to 16 bits."""
    qf, kf, vf = q.float(), k.float(), v.float()
    if q_rounded:
        qf, scale = (qf * scale).to(dtype).float(), 1.0
    if leak is not None:
        kf = torch.cat([kf, leak[0].float()[None]], 0)
        vf = torch.cat([vf, leak[1].float()[None]], 0)
    s = (qf @ kf.T) * scale
    p = torch.exp(s - s.amax(-1, keepdim=True)).to(dtype).float()
    num, den = p @ vf, p.sum(-1, keepdim=True)
    if wrong_sum_row is not None:
        den = den.clone()
        den[wrong_sum_row] = den[wrong_sum_row + 1]
    return (num / den).to(dtype)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D", [32, 40, 64, 80, 160])
@pytest.mark.parametrize("Nk", [1, 7, 77, 130, 203, 1024])
def test_clean_attention_emulation_passes(D, Nk, dtype):
    g = torch.Generator().manual_seed(D * 7 + Nk)
    Nq = 200
    q, k, v = (torch.randn(n, D, generator=g).to(dtype) for n in (Nq, Nk, Nk))
    ref, bound = P.attention_bound(q, k, v, D ** -0.5, dtype)
    r = P.assert_elementwise(_attn_emulation(q, k, v, D ** -0.5, dtype, q_rounded=D == 40), ref, bound, f"attention D {D} Nk {Nk} {dtype}", tile=(32, D))
    assert r <= 1.0


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D", [40, 64])
def test_attention_faults_are_caught(D, dtype):
    g = torch.Generator().manual_seed(D * 7 + 203)
    Nq, Nk = 1024, 203  # 203 keys: the ragged last 64-key tile holds 11 keys and 53 pad columns
    q, k, v = (torch.randn(n, D, generator=g).to(dtype) for n in (Nq, Nk, Nk))
    scale = D ** -0.5
    ref, bound = P.attention_bound(q, k, v, scale, dtype)
    clean = _attn_emulation(q, k, v, scale, dtype, q_rounded=D == 40)
    P.assert_elementwise(clean, ref, bound, "clean")
    m = torch.zeros(Nq, D, dtype=torch.bool)
    m[128:256] = True  # a kernel leaks per workgroup: one 128-row query block of the eight
    # one pad column not masked: its K row is zero-filled staging (score 0 -> weight e^-max of the row); its V^T column holds the NaN
    # the GPU cases poison the padding with
    got = clean.clone()
    got[128:256] = _attn_emulation(q, k, v, scale, dtype, leak=(torch.zeros(D), torch.full((D,), float("nan"))), q_rounded=D == 40)[128:256]
    _caught(got, ref, bound, m, "pad key leaks into one query block (poisoned padding)")
    # ... and a finite stale value there: a weight of ~3e-3 times a value of 16.  Global rel 1.7e-2 .. 2e-2 for this one block: the 1.2e-2
    # of test_attention_bf16 sees it only because the tensor is small; the per-element bound points at the block
    got = clean.clone()
    got[128:256] = _attn_emulation(q, k, v, scale, dtype, leak=(torch.zeros(D), torch.full((D,), 16.0)), q_rounded=D == 40)[128:256]
    _caught(got, ref, bound, m, "pad key leaks into one query block (stale finite value)")
    # one query row normalised with its neighbour's row sum (one row of 1024: 1e-2 .. 2e-2 in the global norm, on either side of the
    # 1.2e-2 of test_attention_bf16).  For the lagged kernel at bf16 the rounding of its pre-scaled Q (term 3 of attention_bound)
    # legitimately allows ~3e-2 |P V|, and a row sum that is off by the typical 20 % stays inside that on the elements with small
    # |O|: 23 % of the row exceed the bound -- reported, but not "on most elements"
    got = _attn_emulation(q, k, v, scale, dtype, wrong_sum_row=500, q_rounded=D == 40)
    m = torch.zeros(Nq, D, dtype=torch.bool)
    if D == 40 and dtype == BF16:
        # replaced by the nearest fault that does stand out there: the row's sum misses the other half-wave's keys (half_swap_sum
        # skipped: the sum holds 32 of every 64 keys), so the row comes out about twice too large
        qf = (q.float() * scale).to(dtype).float()
        s = qf @ k.float().T
        p = torch.exp(s - s.amax(-1, keepdim=True)).to(dtype).float()
        half = p.view(Nq, -1)[:, [j for j in range(Nk) if (j % 64) < 32]].sum(-1, keepdim=True)
        got = clean.clone()
        got[500] = ((p @ v.float())[500] / half[500]).to(dtype)
    m[500] = True
    _caught(got, ref, bound, m, "row 500: half-summed row sum" if D == 40 and dtype == BF16 else "row 500 divided by row 501's sum")


# ---------------------------------------------------------------------------------------------------------------------------
# GroupNorm / LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------
def _gn_emulation(x, G, gamma, beta, eps, silu, stats_from=None, gamma_shift=None):
    """float32 statistics per (sample, group), float32 normalisation, one rounding.  stats_from = (b, g, b2): group g of sample b
    uses sample b2's statistics.  gamma_shift = (c0,): channels c0..c0+7 use gamma of c0+8..c0+15."""
    B, HW, C = x.shape
    xf = x.float().reshape(B, HW, G, C // G)
    mean = xf.mean((1, 3), keepdim=True)
    var = ((xf - mean) ** 2).mean((1, 3), keepdim=True)
    if stats_from is not None:
        b, gi, b2 = stats_from
        mean, var = mean.clone(), var.clone()
        mean[b, 0, gi, 0], var[b, 0, gi, 0] = mean[b2, 0, gi, 0], var[b2, 0, gi, 0]
    ga = gamma.clone()
    if gamma_shift is not None:
        c0 = gamma_shift[0]
        ga[c0:c0 + 8] = gamma[c0 + 8:c0 + 16]
    y = ((xf - mean) * torch.rsqrt(var + eps)).reshape(B, HW, C) * ga + beta
    if silu:
        y = y * (1.0 / (1.0 + torch.exp(-y)))
    return y.to(x.dtype)


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("B,HW,C,G", [(2, 64, 320, 32), (1, 4096, 320, 32), (2, 256, 1280, 32), (3, 37, 64, 8), (2, 1024, 1920, 32)])
def test_clean_groupnorm_emulation_passes_and_faults_are_caught(B, HW, C, G, dtype):
    g = torch.Generator().manual_seed(C + HW)  # the generators of test_groupnorm
    x = (torch.randn(B, HW, C, generator=g) * 2 + 0.5).to(dtype)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    height = HW * (C // G) // 256 + 16
    for silu in (False, True):
        ref, bound = P.groupnorm_ref_bound(x, G, gamma, beta, 1e-5, dtype, height, silu)
        r = P.assert_elementwise(_gn_emulation(x, G, gamma, beta, 1e-5, silu), ref, bound, f"groupnorm {dtype} silu {silu}")
        assert r <= 1.0
    ref, bound = P.groupnorm_ref_bound(x, G, gamma, beta, 1e-5, dtype, height, False)
    # one 8-channel vector takes the next vector's gamma (one vector of C / 8 per row: about 1 / 40 .. 1 / 240 of the tensor; the global
    # norm of a 6e-3 threshold sees it only in the narrow tensors)
    got = _gn_emulation(x, G, gamma, beta, 1e-5, False, gamma_shift=(16,))
    m = torch.zeros_like(got, dtype=torch.bool)
    m[:, :, 16:24] = True
    _caught(got, ref, bound, m, "gamma of the next 8-channel vector")
    if B > 1 and dtype == F32:
        # one group's statistics taken from the neighbouring sample.  Samples of one generator have nearly equal statistics (they differ
        # by ~1 / sqrt(HW C / G)), so at 16-bit outputs this fault sits inside correct rounding on most elements and no honest bound can
        # flag it; the float32 element type exposes it (the 2e-6 / 6e-3 global thresholds of test_groupnorm do NOT: one group of B * G)
        got = _gn_emulation(x, G, gamma, beta, 1e-5, False, stats_from=(0, 3, 1))
        if B * G >= 64:
            assert _rel(got, ref) < 6e-3
        m = torch.zeros(B, HW, G, C // G, dtype=torch.bool)
        m[0, :, 3] = True
        _caught(got, ref, bound, m.reshape(B, HW, C), "statistics of the neighbouring sample")


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("rows,C", [(5, 320), (130, 640), (9, 2048), (4099, 320)])
def test_clean_layernorm_emulation_passes_and_faults_are_caught(rows, C, dtype):
    g = torch.Generator().manual_seed(rows)  # the generators of test_layernorm
    x = (torch.randn(rows, C, generator=g) * 3 - 1).to(dtype)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref, bound = P.layernorm_ref_bound(x, gamma, beta, 1e-5, dtype, C // 8 + 8)
    xf = x.float()
    mean = xf.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((xf - mean) ** 2).mean(-1, keepdim=True) + 1e-5)
    got = ((xf - mean) * rstd * gamma + beta).to(dtype)
    assert P.assert_elementwise(got, ref, bound, f"layernorm {rows}x{C} {dtype}") <= 1.0
    # the last row normalised with the statistics of the row before it (rows are independent draws: O(1) effect; one row of 4099 is
    # invisible to the 6e-3 global threshold of test_layernorm)
    bad = got.clone()
    bad[-1] = ((xf[-1] - mean[-2]) * rstd[-2] * gamma + beta).to(dtype)
    m = torch.zeros_like(bad, dtype=torch.bool)
    m[-1] = True
    _caught(bad, ref, bound, m, "statistics of the neighbouring row")
    if rows == 4099:
        assert _rel(bad, ref) < 6e-3
