"""Write-footprint canaries of the float32 matrix-core path: the float32 legs of tests/test_footprint_gpu.py (its ``Guarded`` /
``_poisoned`` helpers, its assertions).  For every launch: the output is finite with NaN all round every operand, bit-equal to the
plain launch, no byte changes outside the logical window, and the workspace's counter tail is still zero.  The kernel each case
names is asserted through gmd_split_plan_info.  All guards are the test's own memory: a stray access is detected, never a fault."""
import math

import pytest
import torch

import split_cases as S
from test_footprint_gpu import Guarded, _poisoned, _row_window, _stream, _ws_tail_is_zero

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32


@pytest.fixture(autouse=True)
def split_mode():
    from gm_diffusion import hip_ops as ops

    prev = ops.set_f32_mode("split")
    yield
    ops.set_f32_mode(prev)


def _poisoned_halves(t):
    """``_poisoned`` for a pre-split tensor: its neighbours are float16 NaNs (a float32 NaN is a NaN half beside a ZERO half)."""
    return _poisoned(t.view(torch.float16)).view(F32)


def _forms(ops, form, a, w):
    """(plain A, plain W, poisoned A, poisoned W, a_split flag) of one operand form: the pre-split tensors are embedded in NaN AFTER
    the split (the marks live on the tensor objects, so they are put back)."""
    if form == "F32S":
        return a, w, _poisoned(a), _poisoned(w), False
    ws = ops.split_weights(w)
    wp = _poisoned_halves(ws)
    wp._split, wp._alpha = True, ws._alpha
    if form == "F32SW":
        return a, ws, _poisoned(a), wp, False
    sa = ops.split_activation(a.reshape(-1, a.shape[-1])).reshape(a.shape)
    return ops._mark_asplit(sa), ws, _poisoned_halves(sa), wp, True


# (M, N, K, plan): ragged 1000 x 328 where the planner gives it the tile shape, the nearest ragged shape where it does not; the last
# row is the full-rows shape whose stores go through the LDS row epilogue (ldc a multiple of 4)
GEMM_FOOTPRINTS = [
    (1000, 328, 640, (64, 64, 1)), (70, 328, 2048, (64, 64, 4)),
    (4100, 1288, 96, (128, 128, 1)), (1000, 328, 2560, (128, 128, 5)),
    (4100, 1280, 96, (128, 160, 1)), (1000, 320, 2560, (128, 160, 5)),
    (4096, 1280, 64, (128, 160, 1)),
]


@pytest.mark.parametrize("form", S.FORMS)
@pytest.mark.parametrize("M,N,K,plan", GEMM_FOOTPRINTS)
def test_gemm_nt_split_stores_only_its_window(M, N, K, plan, form):
    from gm_diffusion import hip_ops as ops

    assert ops.split_plan_info(S.FORM_CODE[form], M, N, K) == (plan[0], plan[1], 0, plan[2])
    ld = N + 24
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    res = torch.randn(M, N, generator=g).to(DEV)
    a0, w0, ap, wp, a_split = _forms(ops, form, a, w)
    plain = ops.gemm_nt(a0, w0, bias=bias, residual=res, alpha=0.5)
    gd = Guarded(M * ld, F32)
    out = gd.t.view(M, ld)
    ops.gemm_nt(ap, wp, bias=_poisoned(bias), residual=_poisoned(res), alpha=0.5, out=out, ldc=ld, a_split=a_split)
    torch.cuda.synchronize()
    what = f"gemm_nt {form} {M}x{N}x{K} {plan}"
    assert bool(torch.isfinite(out[:, :N]).all()), what + ": a poisoned neighbour of an input was read"
    assert torch.equal(out[:, :N], plain), what + ": the guarded launch differs from the plain one"
    gd.assert_untouched_outside(_row_window(M, ld, N), what)
    assert _ws_tail_is_zero(ops), what + ": the workspace's counter tail is not zero after the launch"


CONV_MODES = [("s1", dict(stride=1, up=0, pad=0)), ("s2-odd", dict(stride=2, up=0, pad=0)), ("pad1-odd", dict(stride=2, up=0, pad=1)),
              ("up", dict(stride=1, up=1, pad=0)), ("up-to-odd", dict(stride=1, up=(45 << 16) | 39, pad=0))]


@pytest.mark.parametrize("form", S.FORMS)
@pytest.mark.parametrize("mode,kw", CONV_MODES)
def test_conv3x3_split_stores_only_its_tensor(mode, kw, form):
    """gmd_conv3x3 through the raw C ABI on the 23 x 20 map (ragged B Ho Wo against the 64-row tiles) in the five modes."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    B, H, W, ci, co = 3, 23, 20, 128, 320
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, H * W, ci, generator=g).to(DEV)
    w = (torch.randn(co, 9 * ci, generator=g) * 0.03).to(DEV)
    b = _poisoned(torch.randn(co, generator=g).to(DEV))
    tb = _poisoned(torch.randn(B, co, generator=g).to(DEV))
    x0, w0, xp, wp, _ = _forms(ops, form, x, w)
    okw = dict(stride=kw["stride"], pad_mode=kw["pad"])
    if kw["up"] == 1:
        okw["upsample"] = True
    elif kw["up"]:
        okw = dict(out_size=(45, 39))
    plain, ho, wo = ops.conv3x3(x0, w0, B, H, W, bias=b, rowbias=tb, **okw)
    code = S.FORM_CODE[form]
    assert ops.split_plan_info(code, B * ho * wo, co, 9 * ci) == (64, 64, 0, 1)
    gd = Guarded(B * ho * wo * co, F32)
    ws = ops._workspace(torch.device(DEV, torch.cuda.current_device()))
    rc = lib().gmd_conv3x3(xp.data_ptr(), wp.data_ptr(), gd.t.data_ptr(), code, ops.dtype_code(F32), B, H, W, ci, co, kw["stride"], kw["up"], kw["pad"],
                           b.data_ptr(), tb.data_ptr(), co, None, float(getattr(w0, "_alpha", 1.0)), None, 0, ws.data_ptr(), ops.WORKSPACE_BYTES, _stream())
    assert rc == 0, lib().gmd_last_error()
    torch.cuda.synchronize()
    what = f"conv3x3 {form} {mode}"
    assert bool(torch.isfinite(plain).all()) and torch.equal(gd.t.view(B, ho * wo, co), plain), what + ": differs from the plain launch"
    gd.assert_untouched_outside(torch.ones(B * ho * wo * co, dtype=torch.bool, device=DEV), what)
    assert _ws_tail_is_zero(ops), what + ": workspace counter tail"


@pytest.mark.parametrize("form", ["F32SW", "F32SA"])
@pytest.mark.parametrize("C,tokens,bn", [(160, 64, 160), (128, 64, 128)])
def test_gemm_qkv_vt_split_stores_only_its_windows(C, tokens, bn, form):
    """gmd_gemm_qkv_vt with ldc > vt_col0 and vt_ld > tokens: the transposed V tiles stay inside [C][tokens] of every sample."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    code = S.FORM_CODE[form]
    B = 172  # 86 x 3 = 258 tiles of 128 rows: the smallest launch that keeps them unsplit (tests/test_split_parity_gpu.py)
    M = B * tokens
    assert lib().gmd_gemm_qkv_vt_ok(code, M, 3 * C, C, 2 * C, tokens, ops.WORKSPACE_BYTES)
    assert ops.split_plan_info(code, M, 3 * C, C) == (128, bn, 0, 1)
    g = torch.Generator().manual_seed(B + tokens + C)
    n = torch.randn(M, C, generator=g).to(DEV)
    w = torch.cat([torch.randn(C, C, generator=g) * C ** -0.5 for _ in range(3)], 0).contiguous().to(DEV)
    n0, w0, npz, wp, _ = _forms(ops, form, n, w)
    qk, vt = ops.gemm_qkv_vt(n0, w0, 2 * C, tokens)
    ldc, vld = 2 * C + 24, tokens + 16
    gq, gv = Guarded(M * ldc, F32), Guarded(B * C * vld, F32)
    ws = ops._workspace(torch.device(DEV, torch.cuda.current_device()))
    rc = lib().gmd_gemm_qkv_vt(npz.data_ptr(), wp.data_ptr(), gq.t.data_ptr(), gv.t.data_ptr(), code, M, 3 * C, C, ldc, 2 * C, tokens, vld, float(w0._alpha),
                               ws.data_ptr(), ops.WORKSPACE_BYTES, _stream())
    assert rc == 0, lib().gmd_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(qk).all()) and bool(torch.isfinite(vt).all())
    assert torch.equal(gq.t.view(M, ldc)[:, :2 * C], qk) and torch.equal(gv.t.view(B, C, vld)[:, :, :tokens], vt)
    gq.assert_untouched_outside(_row_window(M, ldc, 2 * C), f"qkv_vt {form} row-major part")
    gv.assert_untouched_outside(_row_window(B * C, vld, tokens), f"qkv_vt {form} transposed V")
    assert _ws_tail_is_zero(ops)


@pytest.mark.parametrize("D,Nq", [(40, 161), (160, 130)])
def test_attention_split_stores_only_its_window(D, Nq):
    """attn_split_kernel through the raw C ABI: ldo > H D, a query count that ends inside a 128-row block, a ragged last key tile."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    B, H, Nk = 2, 2, 203
    C = H * D
    g = torch.Generator().manual_seed(D)
    q = _poisoned(torch.randn(B, Nq, C, generator=g).to(DEV))
    k = _poisoned(torch.randn(B, Nk, C, generator=g).to(DEV))
    ldvt = (Nk + 7) // 8 * 8
    vt = torch.full((B, C, ldvt), float("nan"), device=DEV)
    vt[:, :, :Nk] = torch.randn(B, C, Nk, generator=g).to(DEV)
    vt = _poisoned(vt)
    plain = ops.attention(q, k, vt, H, Nk, D ** -0.5)
    ldo = C + 24
    gd = Guarded(B * Nq * ldo, F32)
    rc = lib().gmd_attention(q.data_ptr(), k.data_ptr(), vt.data_ptr(), gd.t.data_ptr(), ops.GMD_F32S, B, H, D, Nq, Nk, C, C, ldvt, ldo, Nq * C, Nk * C,
                             C * ldvt, Nq * ldo, D ** -0.5, 0, _stream())
    assert rc == 0, lib().gmd_last_error()
    torch.cuda.synchronize()
    out = gd.t.view(B, Nq, ldo)
    assert bool(torch.isfinite(plain).all())
    assert torch.equal(out[:, :, :C], plain), f"split attention D={D}: ldo > H D changes the result"
    gd.assert_untouched_outside(_row_window(B * Nq, ldo, C), f"split attention D={D}")


@pytest.mark.parametrize("form", S.FORMS)
def test_gemm_presplit_output_stores_only_its_tensor(form):
    """The ``c_split`` layout of the GEMM row epilogue (out_dtype = GMD_F32SA through the wrapper's ``split_out``): every 8-byte piece
    lands inside the [M, N] tensor, the bytes are those of the plain launch split afterwards."""
    from gm_diffusion import hip_ops as ops

    M, N, K, plan = S.GEMM_CASES["128x160 full"]
    assert ops.split_plan_info(S.FORM_CODE[form], M, N, K) == (plan[0], plan[1], 0, plan[2])
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    a0, w0, ap, wp, a_split = _forms(ops, form, a, w)
    plain = ops.gemm_nt(a0, w0, bias=bias, act=ops.ACT_SILU, split_out=True)
    assert ops.is_asplit(plain), "the launch did not store pre-split"
    gd = Guarded(M * N, F32)
    got = ops.gemm_nt(ap, wp, bias=_poisoned(bias), act=ops.ACT_SILU, split_out=True, out=gd.t.view(M, N), a_split=a_split)
    torch.cuda.synchronize()
    assert ops.is_asplit(got)
    as_bytes = lambda t: t.contiguous().view(torch.uint8)
    assert bool(torch.isfinite(plain.view(torch.float16)).all()), "a poisoned neighbour of an input was read"
    assert torch.equal(as_bytes(got), as_bytes(plain)), "the guarded launch differs from the plain one"
    assert torch.equal(as_bytes(plain), as_bytes(ops.split_activation(ops.gemm_nt(a0, w0, bias=bias, act=ops.ACT_SILU))))
    gd.assert_untouched_outside(torch.ones(M * N, dtype=torch.bool, device=DEV), f"gemm_nt pre-split output {form}")
    assert _ws_tail_is_zero(ops)


@pytest.mark.parametrize("D,Nq", [(40, 161), (160, 130)])
def test_attention_presplit_output_stores_only_its_tensor(D, Nq):
    """The pre-split O of attn_split_kernel (GMD_F32SA: contiguous rows of whole 32-element chunks)."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    B, H, Nk = 2, 4, 203
    C = H * D
    g = torch.Generator().manual_seed(D)
    q = _poisoned(torch.randn(B, Nq, C, generator=g).to(DEV))
    k = _poisoned(torch.randn(B, Nk, C, generator=g).to(DEV))
    ldvt = (Nk + 7) // 8 * 8
    vt = torch.full((B, C, ldvt), float("nan"), device=DEV)
    vt[:, :, :Nk] = torch.randn(B, C, Nk, generator=g).to(DEV)
    vt = _poisoned(vt)
    plain = ops.attention(q, k, vt, H, Nk, D ** -0.5, split_out=True)
    assert ops.is_asplit(plain), "the launch did not store pre-split"
    gd = Guarded(B * Nq * C, F32)
    rc = lib().gmd_attention(q.data_ptr(), k.data_ptr(), vt.data_ptr(), gd.t.data_ptr(), ops.GMD_F32SA, B, H, D, Nq, Nk, C, C, ldvt, C, Nq * C, Nk * C,
                             C * ldvt, Nq * C, D ** -0.5, 0, _stream())
    assert rc == 0, lib().gmd_last_error()
    torch.cuda.synchronize()
    as_bytes = lambda t: t.contiguous().view(torch.uint8)
    assert bool(torch.isfinite(plain.view(torch.float16)).all())
    assert torch.equal(as_bytes(gd.t.view(B, Nq, C)), as_bytes(plain)), f"pre-split attention D={D}: the guarded launch differs from the plain one"
    assert torch.equal(as_bytes(plain), as_bytes(ops.split_activation(ops.attention(q, k, vt, H, Nk, D ** -0.5))))
    gd.assert_untouched_outside(torch.ones(B * Nq * C, dtype=torch.bool, device=DEV), f"pre-split attention D={D}")
