"""Write-footprint canaries: what a kernel stores OUTSIDE its logical output window.  The wrappers allocate outputs of exactly the
right size, so a stray store lands in a neighbouring tensor of the caching allocator and surfaces, if ever, as an unrelated flaky
failure.  Here every output lives inside one larger allocation of the test's own: a guard band of 64 KiB before and after it, filled
with a fixed byte pattern, and -- where the ABI has a leading dimension -- rows wider than the logical row with the padding columns
pre-filled too.  After the launch the logical window must equal an un-guarded launch bit for bit and every guard / padding byte must
be unchanged.  Inputs get the mirror treatment (NaN all round them).  All guards are the test's own memory: a stray access is
detected, never a fault; nothing here provokes one."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
GUARD = 65536  # bytes, before and after


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


class Guarded:
    """``numel`` elements of ``dtype`` in the middle of a byte buffer filled with the pattern (i * 131 + 89) mod 251: no run of equal
    bytes, never the bytes of a zero or of a plausible result."""

    def __init__(self, numel, dtype):
        self.nbytes = numel * torch.empty((), dtype=dtype).element_size()
        total = 2 * GUARD + self.nbytes
        self.buf = ((torch.arange(total, device=DEV, dtype=torch.int64) * 131 + 89) % 251).to(torch.uint8)
        self.before = self.buf.clone()
        self.t = self.buf[GUARD:GUARD + self.nbytes].view(dtype)

    def assert_untouched_outside(self, window_mask, what):
        """window_mask: bool tensor over the elements of ``t`` (True = the logical window, may change)."""
        es = self.t.element_size()
        changed = self.buf != self.before
        assert not bool(changed[:GUARD].any()), f"{what}: {int(changed[:GUARD].sum())} bytes of the guard band BEFORE the output changed"
        assert not bool(changed[GUARD + self.nbytes:].any()), f"{what}: {int(changed[GUARD + self.nbytes:].sum())} bytes of the guard band AFTER the output changed"
        inner = changed[GUARD:GUARD + self.nbytes].view(-1, es).any(1)
        stray = inner & ~window_mask.reshape(-1)
        if bool(stray.any()):
            first = int(stray.nonzero()[0])
            raise AssertionError(f"{what}: {int(stray.sum())} padding elements changed; first at flat element {first}")


def _poisoned(t):
    """A copy of ``t`` embedded in NaN (float) surroundings: reads outside the logical tensor poison the result."""
    n = GUARD // t.element_size()
    buf = torch.full((2 * n + t.numel(),), float("nan"), dtype=t.dtype, device=DEV)
    buf[n:n + t.numel()] = t.reshape(-1)
    return buf[n:n + t.numel()].view(t.shape)


def _ws_tail_is_zero(ops):
    ws = ops._workspace(torch.device(DEV, torch.cuda.current_device()))
    return not bool(ws[-(ops.WS_TAIL_BYTES // 4):].view(torch.int32).any())


def _row_window(rows, ld, n):
    m = torch.zeros(rows, ld, dtype=torch.bool, device=DEV)
    m[:, :n] = True
    return m


GEMM_PLANS = [("default", None), ("ring128x160", (128, 160, 9, 0)), ("ring128x128", (128, 128, 9, 0)), ("ring64x64", (64, 64, 9, 0)),
              ("pp256x160", (256, 160, 283, 283)), ("pp256x128", (256, 128, 283, 283)), ("lc128x160", (128, 160, 244, 244)),
              ("lc64x160", (64, 160, 244, 244)), ("lc128x128", (128, 128, 244, 244))]


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("name,plan,ks", [(n, p, ks) for n, p in GEMM_PLANS for ks in ((1,) if p is None else (1, 2))])  # (K slices are forced per kernel)
def test_gemm_nt_stores_only_its_window(name, plan, ks, dtype, force_plan):
    """Ragged M and N (1000 x 328; the 244 kernel: N on a tile boundary, as in its other cases), ldc = N + 24, 16-bit and float32
    stores, K slices through both reduction paths; the workspace's counter tail is zero afterwards."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    M, K = 1000, 640
    N = 3 * plan[1] if plan is not None and plan[2] == 244 else 328
    ld = N + 24
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).to(dtype).to(DEV)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dtype).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    res = torch.randn(M, N, generator=g).to(dtype).to(DEV)
    fix_default = lib().gmd_splitk_fixup_max(-1)
    for fix in ((0, fix_default) if ks > 1 else (fix_default,)):
        lib().gmd_splitk_fixup_max(fix)
        if plan is not None:
            force_plan(plan[0], plan[1], plan[2], ks)
            assert ops.gemm_plan_info(dtype, M, N, K) == (plan[0], plan[1], plan[3], ks)
        for out_dtype in (dtype, F32):
            rs = res if out_dtype == dtype else None  # (the ABI takes a residual only with out_dtype == dtype)
            plain = ops.gemm_nt(a, w, bias=bias, residual=rs, alpha=0.5, out_dtype=out_dtype)
            gd = Guarded(M * ld, out_dtype)
            out = gd.t.view(M, ld)
            ops.gemm_nt(_poisoned(a), _poisoned(w), bias=_poisoned(bias), residual=None if rs is None else _poisoned(rs), alpha=0.5, out_dtype=out_dtype, out=out,
                        ldc=ld)
            torch.cuda.synchronize()
            what = f"gemm_nt {name} ks={ks} fixup_max={fix} {dtype}->{out_dtype}"
            assert bool(torch.isfinite(out[:, :N].float()).all()), what + ": a poisoned neighbour of an input was read"
            assert torch.equal(out[:, :N], plain), what + ": the guarded launch differs from the plain one"
            gd.assert_untouched_outside(_row_window(M, ld, N), what)
            assert _ws_tail_is_zero(ops), what + ": the workspace's counter tail is not zero after the launch"
    lib().gmd_splitk_fixup_max(fix_default)


@pytest.mark.parametrize("dtype", [BF16, F16, F32])
def test_gemm_batched_and_geglu_store_only_their_windows(dtype):
    from gm_diffusion import hip_ops as ops

    g = torch.Generator().manual_seed(9)
    Bn, N, C, ld = 3, 72, 128, 80  # test_gemm_batched_and_swapped's case: it reads [:, :, :72] and never looks at the 8 padding columns
    x = torch.randn(Bn, N, C, generator=g).to(dtype).to(DEV)
    wv = (torch.randn(C, C, generator=g) / math.sqrt(C)).to(dtype).to(DEV)
    plain = ops.gemm_nt(wv, x, ldc=ld)
    gd = Guarded(Bn * C * ld, dtype)
    out = gd.t.view(Bn, C, ld)
    ops.gemm_nt(_poisoned(wv), _poisoned(x), ldc=ld, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out[:, :, :N], plain[:, :, :N])
    gd.assert_untouched_outside(_row_window(Bn * C, ld, N), f"batched gemm_nt {dtype}")
    if dtype == BF16:  # the fused GEGLU epilogue writes [M, N / 2]
        M, Cc = 300, 320
        xx = torch.randn(M, Cc, generator=g).bfloat16().to(DEV)
        wi = (torch.randn(8 * Cc, Cc, generator=g) * 0.05).bfloat16().to(DEV)
        bi = (torch.randn(8 * Cc, generator=g) * 0.5).to(DEV)
        plain = ops.gemm_nt(xx, wi, bias=bi, act=ops.ACT_GEGLU)
        ldg = 4 * Cc + 16
        gd = Guarded(M * ldg, BF16)
        out = gd.t.view(M, ldg)
        ops.gemm_nt(_poisoned(xx), _poisoned(wi), bias=_poisoned(bi), act=ops.ACT_GEGLU, out=out, ldc=ldg)
        torch.cuda.synchronize()
        assert torch.equal(out[:, :4 * Cc], plain)
        gd.assert_untouched_outside(_row_window(M, ldg, 4 * Cc), "GEGLU gemm_nt")
    assert _ws_tail_is_zero(ops)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D", [32, 40, 64, 80, 160])
def test_attention_stores_only_its_window(D, dtype):
    """ldo > H D, Nq not a multiple of the 128-row query block (333), a ragged last key tile (203), through the raw C ABI."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    B, H, Nq, Nk = 2, 2, 333, 203
    C = H * D
    g = torch.Generator().manual_seed(D)
    q = _poisoned(torch.randn(B, Nq, C, generator=g).to(dtype).to(DEV))
    k = _poisoned(torch.randn(B, Nk, C, generator=g).to(dtype).to(DEV))
    ldvt = (Nk + 7) // 8 * 8
    vt = torch.full((B, C, ldvt), float("nan"), dtype=dtype, device=DEV)
    vt[:, :, :Nk] = torch.randn(B, C, Nk, generator=g).to(dtype).to(DEV)
    vt = _poisoned(vt)
    plain = ops.attention(q, k, vt, H, Nk, D ** -0.5)
    ldo = C + 24
    gd = Guarded(B * Nq * ldo, dtype)
    rc = lib().gmd_attention(q.data_ptr(), k.data_ptr(), vt.data_ptr(), gd.t.data_ptr(), ops.dtype_code(dtype), B, H, D, Nq, Nk,
                             C, C, ldvt, ldo, Nq * C, Nk * C, C * ldvt, Nq * ldo, D ** -0.5, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib().gmd_last_error()
    torch.cuda.synchronize()
    out = gd.t.view(B, Nq, ldo)
    assert bool(torch.isfinite(plain.float()).all())
    assert torch.equal(out[:, :, :C], plain), f"attention D={D} {dtype}: ldo > H D changes the result"
    gd.assert_untouched_outside(_row_window(B * Nq, ldo, C), f"attention D={D} {dtype}")


@pytest.mark.parametrize("dtype", [BF16, F16, F32])
@pytest.mark.parametrize("rows,C", [(5, 320), (4099, 320), (9, 2048), (1031, 640), (8197, 64), (4099, 960)])  # packed, wave<4,1>, <1,4>, <2,2> (csrc/norm.hip)
def test_layernorm_stores_only_its_rows(rows, C, dtype):
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    g = torch.Generator().manual_seed(rows)
    x = _poisoned((torch.randn(rows, C, generator=g) * 3 - 1).to(dtype).to(DEV))
    gamma, beta = _poisoned(torch.randn(C, generator=g).to(DEV)), _poisoned(torch.randn(C, generator=g).to(DEV))
    plain = ops.layernorm(x, gamma, beta, 1e-5)
    gd = Guarded(rows * C, dtype)
    rc = lib().gmd_layernorm(x.data_ptr(), gd.t.data_ptr(), ops.dtype_code(dtype), rows, C, gamma.data_ptr(), beta.data_ptr(), 1e-5,
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib().gmd_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(plain.float()).all()) and torch.equal(gd.t.view(rows, C), plain)
    gd.assert_untouched_outside(torch.ones(rows, C, dtype=torch.bool, device=DEV), f"layernorm {rows}x{C} {dtype}")


@pytest.mark.parametrize("dtype", [BF16, F16, F32])
@pytest.mark.parametrize("B,HW,C,G", [(2, 64, 320, 32), (3, 37, 64, 8), (1, 4163, 320, 32), (5, 4100, 320, 32), (2, 3300, 640, 32)])
def test_groupnorm_stores_only_its_tensor(B, HW, C, G, dtype):
    """gmd_groupnorm_fused (where the slab fits), gmd_groupnorm_split (the range-checked stores of its loop-free apply pass, ragged
    last workgroup) and gmd_groupnorm_stats + gmd_groupnorm_apply, through the raw C ABI."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    g = torch.Generator().manual_seed(C + HW)
    x = _poisoned((torch.randn(B, HW, C, generator=g) * 2 + 0.5).to(dtype).to(DEV))
    gamma, beta = _poisoned(torch.randn(C, generator=g).to(DEV)), _poisoned(torch.randn(C, generator=g).to(DEV))
    stream = torch.cuda.current_stream().cuda_stream
    code = ops.dtype_code(dtype)
    whole = torch.ones(B, HW, C, dtype=torch.bool, device=DEV)
    plain = ops.groupnorm(x, B, G, gamma, beta, 1e-5, silu=True)
    assert bool(torch.isfinite(plain.float()).all())
    nsplit = lib().gmd_groupnorm_nsplit(HW)
    # split: partial sums + folding apply
    gd = Guarded(B * HW * C, dtype)
    gw = Guarded(B * nsplit * G * 2, F32)
    rc = lib().gmd_groupnorm_split(x.data_ptr(), gd.t.data_ptr(), code, B, HW, C, G, 1e-5, gamma.data_ptr(), beta.data_ptr(), gw.t.data_ptr(), 1, stream)
    assert rc == 0, lib().gmd_last_error()
    torch.cuda.synchronize()
    cpg = C // G
    vec16 = (cpg * x.element_size()) % 16 == 0 and (C * x.element_size()) % 16 == 0
    fused_expected = cpg % (2 if dtype != F32 else 1) == 0 and HW * cpg * x.element_size() <= (ops.GN_FUSED_MAX_SLAB_VEC16 if vec16 else ops.GN_FUSED_MAX_SLAB)
    assert fused_expected == (HW < 1000), "the wrapper's dispatch rule moved: re-pick the shapes so that both paths stay covered"
    if not fused_expected:  # ops.groupnorm took gmd_groupnorm_split for this slab: same launch, same bits
        assert torch.equal(gd.t.view(B, HW, C), plain), f"groupnorm_split {dtype}: the guarded launch differs from the plain one"
    else:  # the fused kernel's two-pass variance and this path's sums differ in the last bits only
        assert bool(torch.isfinite(gd.t.float()).all())
        assert float((gd.t.view(B, HW, C).double() - plain.double()).abs().max()) <= 2.0 ** -6 * float(plain.double().abs().max())
    gd.assert_untouched_outside(whole, f"groupnorm_split output {dtype}")
    gw.assert_untouched_outside(torch.ones(B * nsplit * G * 2, dtype=torch.bool, device=DEV), f"groupnorm_split workspace {dtype}")
    # fused single launch, where it is instantiated for this slab
    gd = Guarded(B * HW * C, dtype)
    rc = lib().gmd_groupnorm_fused(x.data_ptr(), gd.t.data_ptr(), code, B, HW, C, G, 1e-5, gamma.data_ptr(), beta.data_ptr(), 1, stream)
    torch.cuda.synchronize()
    if fused_expected:
        assert rc == 0, lib().gmd_last_error()
        assert torch.equal(gd.t.view(B, HW, C), plain), f"groupnorm_fused {dtype}: the guarded launch differs from the plain one"
        gd.assert_untouched_outside(whole, f"groupnorm_fused {dtype}")
    elif rc != 0:  # (slabs beyond 128 KiB are refused; between the wrapper's limit and that the kernel still runs)
        assert rc == 3 and not bool((gd.buf != gd.before).any()), "a refused launch must not write"
    else:
        gd.assert_untouched_outside(whole, f"groupnorm_fused {dtype}")
    # statistics + apply
    ss = Guarded(B * C * 2, F32)
    gw = Guarded(B * nsplit * G * 2, F32)
    rc = lib().gmd_groupnorm_stats(x.data_ptr(), code, B, HW, C, G, 1e-5, gamma.data_ptr(), beta.data_ptr(), gw.t.data_ptr(), ss.t.data_ptr(), stream)
    assert rc == 0, lib().gmd_last_error()
    gd = Guarded(B * HW * C, dtype)
    rc = lib().gmd_groupnorm_apply(x.data_ptr(), gd.t.data_ptr(), code, B, HW, C, ss.t.data_ptr(), 1, stream)
    assert rc == 0, lib().gmd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(gd.t.view(B, HW, C), ops.groupnorm_split(x, B, G, gamma, beta, 1e-5, silu=True))
    gd.assert_untouched_outside(whole, f"groupnorm_apply {dtype}")
    ss.assert_untouched_outside(torch.ones(B * C * 2, dtype=torch.bool, device=DEV), f"groupnorm_stats scale_shift {dtype}")
    gw.assert_untouched_outside(torch.ones(B * nsplit * G * 2, dtype=torch.bool, device=DEV), f"groupnorm_stats workspace {dtype}")


@pytest.mark.parametrize("dtype", [BF16, F16, F32])
def test_softmax_geglu_concat_store_only_their_windows(dtype):
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    stream = torch.cuda.current_stream().cuda_stream
    code = ops.dtype_code(dtype)
    g = torch.Generator().manual_seed(8)
    # row softmax, ldp > cols: the padding columns are ZERO as documented, the guards unchanged
    rows, cols, lds_, ldp = 70, 77, 80, 88
    s = torch.full((rows, lds_), float("nan"), device=DEV)
    s[:, :cols] = (torch.randn(rows, cols, generator=g) * 4).to(DEV)
    s = _poisoned(s)
    gd = Guarded(rows * ldp, dtype)
    rc = lib().gmd_softmax_rows(s.data_ptr(), lds_, gd.t.data_ptr(), code, ldp, rows, cols, 0.3, 0, stream)
    assert rc == 0, lib().gmd_last_error()
    torch.cuda.synchronize()
    p = gd.t.view(rows, ldp)
    assert torch.equal(p[:, :cols], ops.softmax_rows(s, cols, 0.3, dtype, ldp=ldp)[:, :cols])
    assert float(p[:, cols:].float().abs().max()) == 0.0
    gd.assert_untouched_outside(torch.ones(rows, ldp, dtype=torch.bool, device=DEV), f"softmax_rows {dtype}")
    # GEGLU: [rows, 2F] -> [rows, F]
    x = _poisoned(torch.randn(37, 2 * 1280, generator=g).to(dtype).to(DEV))
    gd = Guarded(37 * 1280, dtype)
    rc = lib().gmd_geglu(x.data_ptr(), gd.t.data_ptr(), code, 37, 1280, stream)
    assert rc == 0, lib().gmd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(gd.t.view(37, 1280), ops.geglu(x))
    gd.assert_untouched_outside(torch.ones(37, 1280, dtype=torch.bool, device=DEV), f"geglu {dtype}")
    # channel concat
    a, b = _poisoned(torch.randn(33, 640, generator=g).to(dtype).to(DEV)), _poisoned(torch.randn(33, 320, generator=g).to(dtype).to(DEV))
    gd = Guarded(33 * 960, dtype)
    rc = lib().gmd_concat_channels(a.data_ptr(), 640, b.data_ptr(), 320, gd.t.data_ptr(), code, 33, stream)
    assert rc == 0, lib().gmd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(gd.t.view(33, 960), torch.cat([a, b], -1))
    gd.assert_untouched_outside(torch.ones(33, 960, dtype=torch.bool, device=DEV), f"concat_channels {dtype}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("mode,kw", [("s1", dict(stride=1, up=0, pad=0)), ("s2-odd", dict(stride=2, up=0, pad=0)), ("pad1-odd", dict(stride=2, up=0, pad=1)),
                                     ("up", dict(stride=1, up=1, pad=0)), ("up-to-odd", dict(stride=1, up=(45 << 16) | 39, pad=0))])
@pytest.mark.parametrize("name,plan", [("default", None), ("pp256x160", (256, 160, 283, 283)), ("lc64x160", (64, 160, 244, 244)), ("ring128x160", (128, 160, 9, 0))])
def test_conv3x3_stores_only_its_tensor(name, plan, mode, kw, dtype, force_plan):
    """gmd_conv3x3 through the raw C ABI on a 23 x 20 map (odd height: ragged B Ho Wo against every tile height, stride 2 of odd
    sizes, GMD_UPSAMPLE_TO(45, 39)): the output is contiguous, so the ragged last row tile's stores are what the guards watch."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    B, H, W, ci, co = 3, 23, 20, 128, 320
    g = torch.Generator().manual_seed(21)
    x = _poisoned(torch.randn(B, H * W, ci, generator=g).to(dtype).to(DEV))
    w = _poisoned((torch.randn(co, 9 * ci, generator=g) * 0.03).to(dtype).to(DEV))
    b = _poisoned(torch.randn(co, generator=g).to(DEV))
    tb = _poisoned(torch.randn(B, co, generator=g).to(DEV))
    if plan is not None:
        force_plan(plan[0], plan[1], plan[2], 1)
    okw = dict(stride=kw["stride"], pad_mode=kw["pad"])
    if kw["up"] == 1:
        okw["upsample"] = True
    elif kw["up"]:
        okw = dict(out_size=(45, 39))
    plain, ho, wo = ops.conv3x3(x, w, B, H, W, bias=b, rowbias=tb, **okw)
    if plan is not None:
        assert ops.gemm_plan_info(dtype, B * ho * wo, co, 9 * ci) == (plan[0], plan[1], plan[3], 1)
    gd = Guarded(B * ho * wo * co, dtype)
    ws = ops._workspace(torch.device(DEV, torch.cuda.current_device()))
    code = ops.dtype_code(dtype)
    rc = lib().gmd_conv3x3(x.data_ptr(), w.data_ptr(), gd.t.data_ptr(), code, code, B, H, W, ci, co, kw["stride"], kw["up"], kw["pad"], b.data_ptr(),
                           tb.data_ptr(), co, None, 1.0, None, 0, ws.data_ptr(), ops.WORKSPACE_BYTES, _stream())
    assert rc == 0, lib().gmd_last_error()
    torch.cuda.synchronize()
    what = f"conv3x3 {name} {mode} {dtype}"
    assert bool(torch.isfinite(plain.float()).all()) and torch.equal(gd.t.view(B, ho * wo, co), plain), what + ": differs from the plain launch"
    gd.assert_untouched_outside(torch.ones(B * ho * wo * co, dtype=torch.bool, device=DEV), what)
    assert _ws_tail_is_zero(ops), what + ": workspace counter tail"


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("B,tokens,C", [(8, 1024, 640), (8, 256, 1280)])
def test_gemm_qkv_vt_stores_only_its_windows(B, tokens, C, dtype):
    """gmd_gemm_qkv_vt with ldc > vt_col0 and vt_ld > tokens: the transposed V tiles must stay inside [C][tokens] of every sample."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    g = torch.Generator().manual_seed(B + tokens + C)
    n = _poisoned(torch.randn(B * tokens, C, generator=g).to(DEV, dtype))
    w = _poisoned(torch.cat([(torch.randn(C, C, generator=g) * C ** -0.5).to(DEV, dtype) for _ in range(3)], 0).contiguous())
    M = B * tokens
    assert lib().gmd_gemm_qkv_vt_ok(ops.dtype_code(dtype), M, 3 * C, C, 2 * C, tokens, ops.WORKSPACE_BYTES)
    qk, vt = ops.gemm_qkv_vt(n, w, 2 * C, tokens)
    ldc, vld = 2 * C + 24, tokens + 16
    gq, gv = Guarded(M * ldc, dtype), Guarded(B * C * vld, dtype)
    ws = ops._workspace(torch.device(DEV, torch.cuda.current_device()))
    rc = lib().gmd_gemm_qkv_vt(n.data_ptr(), w.data_ptr(), gq.t.data_ptr(), gv.t.data_ptr(), ops.dtype_code(dtype), M, 3 * C, C, ldc, 2 * C, tokens, vld, 1.0,
                               ws.data_ptr(), ops.WORKSPACE_BYTES, _stream())
    assert rc == 0, lib().gmd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(gq.t.view(M, ldc)[:, :2 * C], qk) and torch.equal(gv.t.view(B, C, vld)[:, :, :tokens], vt)
    gq.assert_untouched_outside(_row_window(M, ldc, 2 * C), f"qkv_vt row-major part {dtype}")
    gv.assert_untouched_outside(_row_window(B * C, vld, tokens), f"qkv_vt transposed V {dtype}")
    assert _ws_tail_is_zero(ops)


@pytest.mark.parametrize("dtype", [BF16, F16, F32])
def test_pack_unpack_rgbe_store_only_their_tensors(dtype):
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    g = torch.Generator().manual_seed(4)
    B, HW, CP = 3, 37 * 5, 8
    s0, s1 = _poisoned(torch.randn(B, 4, 37, 5, generator=g).to(DEV)), _poisoned(torch.randn(B, 3, 37, 5, generator=g).to(DEV))
    plain = ops.pack_unet_input(s0, s1, 2, CP, dtype)
    gd = Guarded(2 * B * HW * CP, dtype)
    rc = lib().gmd_pack_unet_input(s0.data_ptr(), 4, s1.data_ptr(), 3, B, HW, 2, gd.t.data_ptr(), CP, ops.dtype_code(dtype), _stream())
    assert rc == 0, lib().gmd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(gd.t.view(plain.shape), plain) and bool(torch.isfinite(plain.float()).all())
    gd.assert_untouched_outside(torch.ones(plain.numel(), dtype=torch.bool, device=DEV), f"pack_unet_input {dtype}")
    # unpack: [B, HW, ld] (first C channels; the others poisoned) -> [B, C, HW] float32
    ld, C = 8, 4
    xin = torch.full((B, HW, ld), float("nan"), dtype=dtype, device=DEV)
    xin[:, :, :C] = torch.randn(B, HW, C, generator=g).to(dtype).to(DEV)
    xin = _poisoned(xin)
    go = Guarded(B * C * HW, F32)
    rc = lib().gmd_unpack_nchw(xin.data_ptr(), ops.dtype_code(dtype), ld, B, C, HW, go.t.data_ptr(), _stream())
    assert rc == 0, lib().gmd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(go.t.view(B, C, HW), xin[:, :, :C].float().transpose(1, 2))
    go.assert_untouched_outside(torch.ones(B * C * HW, dtype=torch.bool, device=DEV), f"unpack_nchw {dtype}")
    if dtype == F32:  # Radiance RGBE pixels, a pixel count that is not a multiple of 4
        npix = 4099
        rgb = _poisoned((torch.rand(npix, 3, generator=g) * 50).to(DEV))
        ge = Guarded(npix * 4, torch.uint8)
        rc = lib().gmd_rgbe_encode(rgb.data_ptr(), ge.t.data_ptr(), npix, _stream())
        assert rc == 0, lib().gmd_last_error()
        torch.cuda.synchronize()
        assert torch.equal(ge.t.view(npix, 4), ops.rgbe_encode(rgb).view(npix, 4))
        ge.assert_untouched_outside(torch.ones(npix * 4, dtype=torch.bool, device=DEV), "rgbe_encode")


@pytest.mark.parametrize("layout", [0, 1])
def test_hdr_tail_stores_only_its_seven_outputs(layout):
    """All seven outputs of gmd_hdr_tail, H W = 37 x 31 = 1147 pixels per image (not a multiple of 4: the vec4 path's tail)."""
    from gm_diffusion._native import lib

    B, H, W = 2, 37, 31
    g = torch.Generator().manual_seed(6)
    shape = (B, 3, H, W) if layout == 0 else (B, H, W, 3)
    sdr, gm = _poisoned(torch.randn(shape, generator=g).to(DEV)), _poisoned(torch.randn(shape, generator=g).to(DEV))
    n = B * H * W * 3
    kinds = [F32, F32, torch.uint8, torch.uint8, F32, F32, torch.int16]

    def run(bufs):
        rc = lib().gmd_hdr_tail(sdr.data_ptr(), gm.data_ptr(), 0, layout, B, H, W, 99.0, 1 / 64, 1, *[b.data_ptr() for b in bufs], _stream())
        assert rc == 0, lib().gmd_last_error()
        torch.cuda.synchronize()

    plain = [torch.empty(n, dtype=k, device=DEV) for k in kinds]
    run(plain)
    gds = [Guarded(n, k) for k in kinds]
    run([gd.t for gd in gds])
    for i, (gd, pl) in enumerate(zip(gds, plain)):
        assert torch.equal(gd.t, pl), f"hdr_tail output {i}: the guarded launch differs from the plain one"
        gd.assert_untouched_outside(torch.ones(n, dtype=torch.bool, device=DEV), f"hdr_tail output {i} layout {layout}")
    assert bool(torch.isfinite(plain[4]).all())


@pytest.mark.parametrize("do_cfg", [False, True])
def test_step_kernels_store_only_their_tensors(do_cfg):
    """gmd_latent_step / gmd_dpm_step / gmd_ddpm_step on B = 3 latents of chw = 3 * 7 * 5 = 105 elements (not a multiple of the
    4-element vector: the kernels' tails), every output guarded, inputs surrounded by NaN."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    B, shape = 3, (3, 3, 7, 5)
    chw = 105
    g = torch.Generator().manual_seed(12)
    mk = lambda *sh: _poisoned(torch.randn(*sh, generator=g).to(DEV))
    eps_in = mk(2 * B if do_cfg else B, *shape[1:])
    x, cur, e1, e2, e3, noise = (mk(*shape) for _ in range(6))
    n = B * chw
    whole = torch.ones(n, dtype=torch.bool, device=DEV)

    def same(gd, plain, what):
        torch.cuda.synchronize()
        assert bool(torch.isfinite(plain).all()) and torch.equal(gd.t.view(shape), plain), what + ": the guarded launch differs from the plain one"
        gd.assert_untouched_outside(whole, what)

    for mode in (0, 1, 4):
        coefs = (1.01, 0.02, 0.97, 0.8, 0.6)
        hist = (e1, e2, e3)[: {0: 0, 1: 1, 4: 3}[mode]]
        pe, pp_, p0 = ops.latent_step(eps_in, x, mode, coefs, do_cfg, 7.5, cur_sample=cur, hist=hist, want_x0=True)
        ge, gp, g0 = (Guarded(n, F32) for _ in range(3))
        h = [t.data_ptr() for t in hist] + [None] * (3 - len(hist))
        rc = lib().gmd_latent_step(eps_in.data_ptr(), x.data_ptr(), cur.data_ptr(), h[0], h[1], h[2], B, chw, int(do_cfg), 7.5, None, 0.0, mode,
                                   *coefs, ge.t.data_ptr(), gp.t.data_ptr(), g0.t.data_ptr(), _stream())
        assert rc == 0, lib().gmd_last_error()
        for gd, pl, nm in ((ge, pe, "eps_out"), (gp, pp_, "x_prev"), (g0, p0, "x0")):
            same(gd, pl, f"latent_step mode {mode} {nm}")
    for order in (1, 2):
        coefs = (0.5, 0.85, 0.9, -0.12, -0.06, 1.3, 0.8, 0.6)
        pm, pp_, p0 = ops.dpm_step(eps_in, x, order, coefs, do_cfg, 7.5, m1=e1, want_x0=True)
        gm_, gp, g0 = (Guarded(n, F32) for _ in range(3))
        rc = lib().gmd_dpm_step(eps_in.data_ptr(), x.data_ptr(), e1.data_ptr(), B, chw, int(do_cfg), 7.5, None, 0.0, order, *coefs,
                                gm_.t.data_ptr(), gp.t.data_ptr(), g0.t.data_ptr(), _stream())
        assert rc == 0, lib().gmd_last_error()
        for gd, pl, nm in ((gm_, pm, "m0"), (gp, pp_, "x_prev"), (g0, p0, "x0")):
            same(gd, pl, f"dpm_step order {order} {nm}")
    for ns in (noise, None):
        coefs = (0.9, 0.43, 0.3, 0.69, 0.1, 0.8, 0.6)
        pp_, p0 = ops.ddpm_step(eps_in, x, coefs, do_cfg, 7.5, noise=ns, clip_range=1.0, want_x0=True)
        gp, g0 = Guarded(n, F32), Guarded(n, F32)
        sa, s1, c0, ct, nsc, pa, p1 = coefs
        rc = lib().gmd_ddpm_step(eps_in.data_ptr(), x.data_ptr(), None if ns is None else ns.data_ptr(), B, chw, int(do_cfg), 7.5, None, 0.0, sa, s1, 1, 1.0,
                                 c0, ct, nsc, pa, p1, gp.t.data_ptr(), g0.t.data_ptr(), _stream())
        assert rc == 0, lib().gmd_last_error()
        for gd, pl, nm in ((gp, pp_, "x_prev"), (g0, p0, "x0")):
            same(gd, pl, f"ddpm_step noise={ns is not None} {nm}")


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_conv3x3_groupnorm_stores_only_its_two_tensors(dtype):
    """gmd_conv3x3_groupnorm (the GroupNorm kernel sums the split-K slabs): Yraw and Ynorm guarded, the slab workspace's counter
    tail zero afterwards."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    B, H, ci, co, G = 8, 8, 1280, 1280, 32
    g = torch.Generator().manual_seed(B * 1000 + H + ci + co)
    x = _poisoned(torch.randn(B, H * H, ci, generator=g).to(DEV, dtype))
    w = _poisoned((torch.randn(co, 9 * ci, generator=g) / math.sqrt(9 * ci)).to(DEV, dtype))
    bias, tb = _poisoned(torch.randn(co, generator=g).to(DEV)), _poisoned(torch.randn(B, co, generator=g).to(DEV))
    res = _poisoned(torch.randn(B, H * H, co, generator=g).to(DEV, dtype))
    gamma, beta = _poisoned(torch.randn(co, generator=g).to(DEV)), _poisoned(torch.randn(co, generator=g).to(DEV))
    code = ops.dtype_code(dtype)
    assert lib().gmd_conv3x3_gn_fusable(code, B, H, H, ci, co, 1, 0, 0, G, ops.WORKSPACE_BYTES), "not the fused launch"
    pr, pn = ops.conv3x3_groupnorm(x, w, B, H, H, G, gamma, beta, 1e-5, silu=True, bias=bias, rowbias=tb, residual=res, want_raw=True)
    n = B * H * H * co
    gr, gn = Guarded(n, dtype), Guarded(n, dtype)
    ws = ops._workspace(torch.device(DEV, torch.cuda.current_device()))
    rc = lib().gmd_conv3x3_groupnorm(x.data_ptr(), w.data_ptr(), gr.t.data_ptr(), gn.t.data_ptr(), code, B, H, H, ci, co, 1, 0, 0, bias.data_ptr(), tb.data_ptr(), co,
                                     res.data_ptr(), 1.0, G, 1e-5, gamma.data_ptr(), beta.data_ptr(), 1, ws.data_ptr(), ops.WORKSPACE_BYTES, _stream())
    assert rc == 0, lib().gmd_last_error()
    torch.cuda.synchronize()
    whole = torch.ones(n, dtype=torch.bool, device=DEV)
    assert bool(torch.isfinite(pn.float()).all()) and torch.equal(gr.t.view(pr.shape), pr) and torch.equal(gn.t.view(pn.shape), pn)
    gr.assert_untouched_outside(whole, f"conv3x3_groupnorm Yraw {dtype}")
    gn.assert_untouched_outside(whole, f"conv3x3_groupnorm Ynorm {dtype}")
    assert _ws_tail_is_zero(ops)


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_groupnorm_colstats_stores_only_its_tensor(dtype):
    """gmd_groupnorm_colstats fed by a producer's statistics (conv3x3 with colstats): the normalised tensor guarded."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    B, H, ci, co, G = 8, 64, 320, 320, 32
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, H * H, ci, generator=g).to(dtype).to(DEV)
    w = (torch.randn(co, 9 * ci, generator=g) * 0.02).to(dtype).to(DEV)
    b = torch.randn(co, generator=g).to(DEV)
    gamma, beta = _poisoned(torch.randn(co, generator=g).to(DEV)), _poisoned(torch.randn(co, generator=g).to(DEV))
    y, _, _ = ops.conv3x3(x, w, B, H, H, bias=b, colstats=True)
    st = getattr(y, "_colstats", None)
    assert st is not None, "the producer left no statistics: gmd_groupnorm_colstats is not exercised"
    before = ops.colstats_uses
    plain = ops.groupnorm(y, B, G, gamma, beta, 1e-5, silu=True)
    assert ops.colstats_uses == before + 1
    yp, sp = _poisoned(y), _poisoned(st[0])
    n = y.numel()
    gd = Guarded(n, dtype)
    rc = lib().gmd_groupnorm_colstats(yp.data_ptr(), gd.t.data_ptr(), ops.dtype_code(dtype), B, H * H, co, G, 1e-5, gamma.data_ptr(), beta.data_ptr(), sp.data_ptr(), co,
                                      None, ops.COLSTATS_BUCKET, 1, _stream())
    assert rc == 0, lib().gmd_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(plain.float()).all()) and torch.equal(gd.t.view(plain.shape), plain)
    gd.assert_untouched_outside(torch.ones(n, dtype=torch.bool, device=DEV), f"groupnorm_colstats {dtype}")
