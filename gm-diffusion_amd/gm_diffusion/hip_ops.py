"""
Thin torch-tensor front end of the C ABI (include/gmd_hip.h).

torch is used here for device memory and streams only: every function validates
its operands on the host, allocates the output with ``torch.empty`` and launches
the hand-written HIP kernel on ``torch.cuda.current_stream()``.  Nothing in this
module computes with torch ops, and nothing falls back to the CPU: tensors that
are not on a HIP device raise ``HipExtensionError``.

Activations are channels-last ``[B, H*W, C]`` (or ``[rows, C]``) in bf16 (MFMA path) or
float32 (parity path); biases / norm parameters / statistics are float32.
"""
from __future__ import annotations

import math
import os
import threading
import time

import torch

from . import profiling
from ._native import ACT_GEGLU, ACT_NONE, ACT_QUICK_GELU, ACT_SILU, GMD_BF16, GMD_F16, GMD_F32, GMD_F32S, GMD_F32SA, GMD_F32SW, HipExtensionError, check, lib

__all__ = [
    "ACT_NONE", "ACT_SILU", "ACT_GEGLU", "ACT_QUICK_GELU", "embedding_lookup", "dpm_step", "dpm_sde_step", "ddpm_step", "ddim_step", "lcm_step", "euler_step", "lms_step", "unipc_step", "HipExtensionError", "dtype_code", "gemm_nt", "conv3x3", "conv3x3_tail", "pack_shortcut", "shortcut_fold_ok", "conv3x3_up2", "pack_upsample_phases", "upsample_phases_ok", "attention", "attention_ip", "scaled_add", "softmax_rows", "set_f32_mode", "f32_split", "split_weights", "scale_weight", "split_attention_ok", "ff_fused_ok", "ff_geglu_fused", "gemm_qkv_vt", "dup_batch",
    "groupnorm_scale_shift", "groupnorm_apply", "groupnorm", "groupnorm_split", "layernorm", "geglu", "timestep_embedding", "timestep_embedding_add",
    "concat_channels", "concat_channels_add", "concat_channels_freeu", "silu_", "cast", "pack_unet_input", "unpack_nchw", "latent_step", "cfg_std_ratio", "hdr_tail", "hdr_tail_resized", "prepare_sdr",
    "apply_gm_to_sdr", "tmo", "gamut_compress", "stage1_chain", "discretize_u16", "quantize_u8",
]


def dtype_code(dt):
    if dt == torch.float32:
        return GMD_F32
    if dt == torch.bfloat16:
        return GMD_BF16
    if dt == torch.float16:
        return GMD_F16
    raise HipExtensionError(f"unsupported dtype {dt}: the HIP kernels take float32, bfloat16 or float16")


HALF_DTYPES = (torch.bfloat16, torch.float16)

# How float32 contractions (gemm_nt, conv3x3, attention) run:
#   "split" (default): on the matrix cores, every float32 operand taken as f16 hi + f16 lo and each product formed as three
#            float16 MFMA passes with float32 accumulation (GMD_F32S / GMD_F32SW, csrc/gemm_split.hip): float32-grade results
#            (~2^-22 relative per term) at matrix-core speed -- the reference's own float32 numerics
#            (scripts/inference/experiments/formal_improved.py:199), the path that meets the 1e-3 latent-RMS gate;
#   "exact": the float32 FMA kernels on the vector units (bit-for-bit an fp32 FMA chain, ~12x slower end to end).
_F32_DEFAULT = os.environ.get("GMD_F32_MODE", "split")  # the process default; read through f32_mode() / hip_ops.F32_MODE
if _F32_DEFAULT not in ("split", "exact"):
    raise HipExtensionError(f"GMD_F32_MODE={_F32_DEFAULT!r}: expected 'split' or 'exact'")
# Per-thread state: a module call that runs under its own float32 mode (components: _in_own_f32_mode), a graph capture's workspace
# (workspace_scope) and the plan family of a co-running forward (plan_family) are scoped to the CALLING THREAD -- two host threads
# driving a "split" and an "exact" module at the same time never see each other's mode.
_tls = threading.local()


def f32_mode():
    """The float32 contraction mode in effect for the calling thread: its scoped override (f32_mode_scope) or the process default."""
    return getattr(_tls, "f32_mode", None) or _F32_DEFAULT


def __getattr__(name):  # hip_ops.F32_MODE stays readable (tests, tools): the calling thread's effective mode
    if name == "F32_MODE":
        return f32_mode()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def set_f32_mode(mode):
    """Switch the PROCESS DEFAULT of float32 contractions between "split" (matrix cores, three float16 products) and "exact" (vector
    FMA); returns the previous default.  Models prepare their weights for the mode in effect when they are placed on the device and
    keep running under it (f32_mode_scope), whatever the default becomes later."""
    global _F32_DEFAULT
    if mode not in ("split", "exact"):
        raise HipExtensionError("f32 mode must be 'split' or 'exact'")
    prev, _F32_DEFAULT = _F32_DEFAULT, mode
    return prev


class f32_mode_scope:
    """Run the ``with`` block under ``mode`` on the calling thread only (other threads keep theirs)."""

    def __init__(self, mode):
        if mode not in ("split", "exact"):
            raise HipExtensionError("f32 mode must be 'split' or 'exact'")
        self.mode = mode

    def __enter__(self):
        self.prev = getattr(_tls, "f32_mode", None)
        _tls.f32_mode = self.mode
        return self

    def __exit__(self, *exc):
        _tls.f32_mode = self.prev
        return False


def f32_split():
    return f32_mode() == "split"


class plan_family:
    """Select the launch-plan family of the calling thread's 16-bit contractions for the ``with`` block (gmd_gemm_plan_family):
    1 = co-running (the dual-UNet pipeline's two overlapped forwards), 0 = a launch that has the chip to itself (the default)."""

    def __init__(self, family):
        self.family = 1 if family else 0

    def __enter__(self):
        self.prev = lib().gmd_gemm_plan_family(self.family)
        return self

    def __exit__(self, *exc):
        lib().gmd_gemm_plan_family(self.prev)
        return False


def check_split_range(what, *tensors, module=None):
    """Range guard of the float32 "split" path.  Every operand of a split contraction is taken as f16 hi + f16 lo: a value
    beyond float16's largest finite number (65504) becomes hi = inf, lo = -inf and the product NaN -- the exact float32 kernels
    have no such limit.  The kernels do not test for it (the split is already the vector-unit bottleneck); the models'
    consumers -- both pipelines on their final latents, ``hdr.decode_to_hdr`` on the decoded images -- call this once per run
    on their OUTPUTS (a NaN reaches them through every following layer).  One reduction and one host synchronisation; only for
    float32 tensors produced under "split".  Raises instead of returning poisoned images."""
    mode = getattr(module, "_f32_mode", None) or f32_mode()
    if mode != "split":
        return
    for t in tensors:
        if t is None or not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_cuda:
            continue
        if not bool(torch.isfinite(t).all()):
            raise HipExtensionError(
                f"{what}: non-finite values out of the float32 'split' path (matrix cores, three float16 products per float32 "
                "product).  Its operands must stay inside float16's range: an activation beyond 65504 splits into inf / -inf and "
                "poisons the product.  Re-run with GMD_F32_MODE=exact (or hip_ops.set_f32_mode('exact') before the models are "
                "placed on the device): the exact float32 kernels have no range limit.")


def split_weights(w):
    """float32 [N, K] (K % 32 == 0) -> the pre-split hi/lo float16 layout of gmd_split_weights, held in a float32 tensor of
    the same shape (same byte count) that is marked ``_split``: gemm_nt / conv3x3 then take it as the GMD_F32SW W operand."""
    _dev(w)
    _f32(w, "split_weights input")
    if w.dim() != 2 or w.shape[1] % 32:
        raise HipExtensionError("split_weights: [N, K] with K a multiple of 32")
    ws = scale_weight(w)
    out = torch.empty_like(w)
    check(lib().gmd_split_weights(_ptr(ws), _ptr(out), w.shape[0], w.shape[1], w.shape[1], _stream()), "gmd_split_weights")
    out._split = True
    out._alpha = ws._alpha
    return out


def scale_weight(w):
    """``w * 2^s`` with the largest magnitude brought into [2^12, 2^13), marked ``_alpha = 2^-s`` (gemm_nt / conv3x3 fold it
    into their alpha).  The lo half of a split operand is a float16 of ~2^-11 of the value: for typical weight magnitudes
    (1e-2) it would sit in float16's subnormal range and lose most of its bits; scaled, every weight down to 2^-15 of the
    largest keeps a full 11-bit lo.  A power of two, so the scaling itself is exact.  Weight preparation only (reads the
    maximum back to the host)."""
    _dev(w)
    _f32(w, "scale_weight input")
    amax = float(w.abs().max()) if w.numel() else 0.0
    s = 0 if amax == 0.0 or not math.isfinite(amax) else max(-60, min(60, 13 - math.frexp(amax)[1]))
    out = w * (2.0 ** s) if s else w.clone()
    out._alpha = 2.0 ** -s
    return out


# Round 4: float32 activations stored PRE-SPLIT between a producer and the contraction that reads them (GMD_F32SA, gmd_hip.h): the
# GroupNorm / LayerNorm apply kernels and the GEGLU epilogue write [hi 64 B | lo 64 B] per 32 elements, the split kernels then read both
# operands as ready float16 fragments.  Results are bit-identical to the in-kernel split.  GMD_F32SA=0 switches the format off (A/B).
USE_F32SA = os.environ.get("GMD_F32SA", "1") != "0"


def is_asplit(t):
    """The tensor holds float32 values in the pre-split activation layout (only ever the A / W operand of a contraction)."""
    return bool(getattr(t, "_asplit", False))


def _mark_asplit(t):
    t._asplit = True
    return t


def want_split_out(dtype, row_len):
    """A producer may store its float32 output pre-split: split mode on the matrix cores, rows of whole 32-element chunks."""
    return USE_F32SA and dtype == torch.float32 and f32_mode() == "split" and row_len % 32 == 0


def split_activation(x):
    """float32 [..., C] (C % 32 == 0) -> the same values in the pre-split activation layout (tests / tools; the product's producers
    write the layout themselves)."""
    _dev(x)
    _f32(x, "split_activation input")
    C = x.shape[-1]
    if C % 32:
        raise HipExtensionError("split_activation: rows must be multiples of 32 elements")
    x = x.contiguous()
    out = torch.empty_like(x)
    check(lib().gmd_split_weights(_ptr(x), _ptr(out), x.numel() // C, C, C, _stream()), "gmd_split_weights")
    return _mark_asplit(out)


def _contract_code(a, w, K, a_split=False):
    """dtype code of a contraction of ``a`` with the W operand ``w`` over K."""
    if a.dtype != torch.float32:
        if getattr(w, "_split", False):
            raise HipExtensionError("a pre-split float32 weight met a 16-bit activation")
        return dtype_code(a.dtype)
    if a_split:
        if not getattr(w, "_split", False):
            raise HipExtensionError("a pre-split activation needs a pre-split weight operand (GMD_F32SA)")
        return GMD_F32SA
    if getattr(w, "_split", False):
        return GMD_F32SW
    return GMD_F32S if (f32_mode() == "split" and K % 32 == 0) else GMD_F32


def is_half(dt):
    """The two 16-bit element types of the matrix-core path (same kernels, layouts and launch plans)."""
    return dt in HALF_DTYPES


def _dev(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise HipExtensionError(
                "gm_diffusion (MI355X build): tensor is on %s; the compute path is hand-written HIP and has no CPU fallback" % t.device)
        if not t.is_contiguous():
            raise HipExtensionError("non-contiguous tensor passed to a HIP kernel")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


_WS = {}
# 96 MB of split-K scratch + the tail the library reserves for its arrival counters (gmd_hip.h "WORKSPACE CONTRACT": zero when first
# handed over, left zero by every launch).  The same number goes to every launch AND every plan query.
WS_TAIL_BYTES = 65536
WORKSPACE_BYTES = (96 << 20) + WS_TAIL_BYTES


class workspace_scope:
    """Route every split-K launch the calling thread issues inside the ``with`` block to ``ws`` (a float32 device tensor of
    WORKSPACE_BYTES).  HIP-graph capture uses it: all captures run on torch's one capture stream, so the per-stream
    table below would hand the SAME scratch to two graphs that are later replayed concurrently on different streams."""

    def __init__(self, ws):
        self.ws = ws

    def __enter__(self):
        self.prev = getattr(_tls, "ws_override", None)
        _tls.ws_override = self.ws
        return self.ws

    def __exit__(self, *exc):
        _tls.ws_override = self.prev
        return False


def new_workspace(device):
    ws = torch.empty(WORKSPACE_BYTES // 4, dtype=torch.float32, device=device)
    ws[-(WS_TAIL_BYTES // 4):].zero_()  # the arrival counters of the in-kernel split-K reduction start at zero
    return ws


def _workspace(device):
    """Persistent float32 scratch, one per (device, stream) so that concurrent streams never share it; it lets
    under-filled GEMM/conv launches split K."""
    ov = getattr(_tls, "ws_override", None)
    if ov is not None:
        return ov
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _WS.get(key)
    if ws is None:
        ws = _WS[key] = new_workspace(device)
    return ws


def _rowbias(rb):
    """rowbias may be a float32 tensor [G, N] or a (tensor [G, ld], column offset) pair selecting N columns of a wider
    matrix (all ResnetBlock2D time-embedding projections of a UNet are produced by ONE GEMM)."""
    if rb is None:
        return None, 0
    if isinstance(rb, tuple):
        t, col = rb
        _dev(t)
        _f32(t, "rowbias")
        return t.data_ptr() + col * 4, t.shape[-1]
    _dev(rb)
    _f32(rb, "rowbias")
    return rb.data_ptr(), rb.shape[-1]


def _f32(t, name):
    if t is not None and t.dtype != torch.float32:
        raise HipExtensionError(f"{name} must be float32")
    return t


def _timed(kind):
    """(timer, start event) when a KernelTimer is active and wants ``kind``, else (None, None)."""
    tm = profiling.active()
    if tm is None or not tm.wants(kind):
        return None, None
    return tm, tm.begin()


# ----------------------------------------------------------------------------------------------
# dense contractions
# ----------------------------------------------------------------------------------------------
# Column statistics for a following GroupNorm (gmd_hip.h "Column statistics"): a producer launch called with ``colstats=True``
# leaves {sum, sum of squares} per 64-row block and per bucket of COLSTATS_BUCKET channels when its plan can (the 128-row ring
# kernels' row epilogue); the tensor it returns then carries them as ``._colstats`` and ``groupnorm`` skips its statistics pass.
# 10 divides every SD-1.5 group size (320/32, 640/32, 960/32, 1280/32, 1920/32, 2560/32) and half of a 160-column tile.
COLSTATS_BUCKET = 10
USE_COLSTATS = os.environ.get("GMD_COLSTATS", "1") != "0"  # A/B switch (tests, tools): off = separate statistics launches
colstats_uses = 0     # GroupNorm calls served from producer statistics (tests assert the path is really taken)


def _colstats_buffer(want, dtype, M, N, K, batch, out_dtype, device, code=None):
    """Buffer for the producer's column statistics when this launch can emit them: the 16-bit types, and (round 4) float32 on the
    matrix cores -- ``code`` is the launch's dtype code (GMD_F32S / GMD_F32SW there)."""
    if not want or not USE_COLSTATS or out_dtype != dtype or M % 64 or N % COLSTATS_BUCKET:
        return None
    if is_half(dtype):
        code = dtype_code(dtype)
    elif code not in (GMD_F32S, GMD_F32SW, GMD_F32SA):
        return None
    if not lib().gmd_gemm_colstats_plan(code, M, N, K, batch, WORKSPACE_BYTES, COLSTATS_BUCKET):
        return None
    return torch.empty((M // 64, N // COLSTATS_BUCKET, 2), dtype=torch.float32, device=device)


def gemm_plan_info(dtype, M, N, K, batch=1, geglu=False):
    """(tile rows, tile columns, kernel code, K slices) a 16-bit gemm_nt / conv3x3 launch of these dimensions takes (conv: M =
    B*Hout*Wout, N = Cout, K = 9*Cin); kernel code 283 = the ping-pong kernel.  For tests and measurement tools."""
    import ctypes

    out = (ctypes.c_int * 4)()
    check(lib().gmd_gemm_plan_info(dtype_code(dtype), M, N, K, batch, WORKSPACE_BYTES, int(geglu), ctypes.addressof(out)), "gmd_gemm_plan_info")
    return tuple(out)


def split_plan_info(code, M, N, K, batch=1, geglu=False):
    """(tile rows, tile columns, kernel code, K slices) a float32 matrix-core launch of these dimensions takes; ``code``: GMD_F32S,
    GMD_F32SW or GMD_F32SA (conv: M = B*Hout*Wout, N = Cout, K = 9*Cin); kernel code 0 = the ring kernel, 244 = the loader /
    converter kernel.  For tests and measurement tools."""
    import ctypes

    out = (ctypes.c_int * 4)()
    check(lib().gmd_split_plan_info(int(code), M, N, K, batch, WORKSPACE_BYTES, int(geglu), ctypes.addressof(out)), "gmd_split_plan_info")
    return tuple(out)


def stamp(buf, k, row=None):
    """Measurement only: write the device's 100 MHz counter into ``buf[row[0], k]`` (``buf``: int64 [rows, stride] device tensor,
    ``row``: int32 device scalar or None = row 0) at this point of the current stream -- also inside a graph capture (gmd_stamp)."""
    stride = buf.shape[-1] if buf.dim() == 2 else 0
    check(lib().gmd_stamp(buf.data_ptr(), _ptr(row), stride, int(k), _stream()), "gmd_stamp")


def carry_colstats(dst, src):
    """``dst`` is a view of ``src`` with the same rows x channels content: keep the producer statistics attached."""
    st = getattr(src, "_colstats", None)
    if st is not None:
        dst._colstats = st
    return dst


def gemm_nt(a, w, bias=None, rowbias=None, rows_per_group=0, residual=None, alpha=1.0, act=ACT_NONE,
            out_dtype=None, out=None, ldc=None, colstats=False, a_split=False, split_out=False):
    """``act(alpha * a @ w.T + bias + rowbias[m // rows_per_group] + residual)``.

    a: [M, K] or [batch, M, K]; w: [N, K] or [batch, N, K] (a 2-D operand is shared by the batch)."""
    _dev(a, w, bias, residual, out)
    rb_ptr, rb_ld = _rowbias(rowbias)
    if a.dtype != w.dtype:
        raise HipExtensionError(f"gemm_nt: dtype mismatch {a.dtype} vs {w.dtype}")
    batch = 1
    if a.dim() == 3 or w.dim() == 3:
        batch = a.shape[0] if a.dim() == 3 else w.shape[0]
    M, K = a.shape[-2], a.shape[-1]
    N = w.shape[-2]
    if w.shape[-1] != K:
        raise HipExtensionError(f"gemm_nt: K mismatch {a.shape} vs {w.shape}")
    a_split = bool(a_split) or is_asplit(a)   # ``a_split``: a VIEW of a pre-split activation (views do not carry the mark)
    dt = _contract_code(a, w, K, a_split)
    if getattr(a, "_split", False):
        raise HipExtensionError("gemm_nt: a pre-split weight can only be the W operand")
    alpha = float(alpha) * getattr(a, "_alpha", 1.0) * getattr(w, "_alpha", 1.0)  # weights stored scaled by a power of two
    sA = M * K if a.dim() == 3 else 0
    sW = N * K if w.dim() == 3 else 0
    out_dtype = out_dtype or a.dtype
    ldc = ldc or (N // 2 if act == ACT_GEGLU else N)  # the fused GEGLU epilogue writes [M, N/2]
    if out is None:
        out = torch.empty((batch, M, ldc) if batch > 1 or a.dim() == 3 or w.dim() == 3 else (M, ldc),
                          dtype=out_dtype, device=a.device)
    sC = M * ldc
    sR = 0
    if residual is not None:
        if residual.dtype != a.dtype or residual.shape[-1] != N or residual.shape[-2] != M:
            raise HipExtensionError("gemm_nt: residual must be [M, N] of the input dtype")
        sR = M * N if residual.dim() == 3 else 0
    if bias is not None and bias.numel() != N:
        raise HipExtensionError("gemm_nt: bias must have N elements")
    ws = _workspace(a.device) if batch == 1 else None
    # pre-split OUTPUT (the A operand of the next contraction): where the launch's plan can write it, else the plain tensor
    oc = dtype_code(out_dtype)
    c_split = False
    if (split_out and dt in (GMD_F32S, GMD_F32SW, GMD_F32SA) and batch == 1 and a.dim() == 2 and w.dim() == 2 and residual is None and not colstats
            and want_split_out(out_dtype, ldc) and ldc == (N // 2 if act == ACT_GEGLU else N)
            and lib().gmd_gemm_out_split_ok(M, N, K, int(act == ACT_GEGLU), WORKSPACE_BYTES)):
        oc, c_split = GMD_F32SA, True
    st = None
    if colstats and batch == 1 and a.dim() == 2 and w.dim() == 2 and act != ACT_GEGLU and ldc == N:
        st = _colstats_buffer(True, a.dtype, M, N, K, 1, out_dtype, a.device, code=dt)
    tm = profiling.active()
    tm = tm if tm is not None and tm.wants("gemm_nt") else None
    t0 = tm.begin() if tm else None
    check(lib().gmd_gemm_nt(_ptr(a), _ptr(w), _ptr(out), dt, oc, M, N, K, K, K, ldc, batch, sA, sW, sC,
                            _ptr(_f32(bias, "bias")), rb_ptr, rows_per_group, rb_ld,
                            _ptr(residual), N, sR, float(alpha), act, _ptr(st), COLSTATS_BUCKET if st is not None else 0,
                            _ptr(ws), WORKSPACE_BYTES, _stream()), "gmd_gemm_nt")
    if tm:
        es = a.element_size()
        tm.end("gemm_nt", 2.0 * batch * M * N * K, batch * (M * K + N * K + M * N) * es, t0)
    if st is not None:
        out._colstats = (st, N)
    elif getattr(out, "_colstats", None) is not None:  # a reused `out=` buffer must not keep an earlier producer's statistics
        del out._colstats
    if c_split:
        _mark_asplit(out)
    elif getattr(out, "_asplit", False):  # a reused `out=` buffer must not keep an earlier launch's layout mark
        del out._asplit
    return out


# Fused Q|K|V projection of a self-attention: the V column tiles leave the projection TRANSPOSED (gmd_gemm_qkv_vt), so the batched
# V^T GEMM of every attention disappears.  GMD_QKV_VT=0 keeps the two launches (A/B measurements, tests).
USE_QKV_VT = os.environ.get("GMD_QKV_VT", "1") != "0"


def gemm_qkv_vt(a, w, vt_col0, tokens):
    """a: [B*tokens, K] (16-bit, or float32 with pre-split weights), w: [N, K] = the stacked q | k | v projection weights.  Returns (qk [B*tokens, vt_col0],
    vt [B, N - vt_col0, tokens]) from ONE launch, or None when this launch's plan cannot write transposed V tiles (the caller then
    runs the two projections separately)."""
    _dev(a, w)
    M, K = a.shape
    N = w.shape[0]
    if not (USE_QKV_VT and a.dtype == w.dtype and a.dim() == 2 and w.dim() == 2 and w.shape[1] == K and tokens % 64 == 0 and M % tokens == 0
            and vt_col0 % 8 == 0):
        return None
    if is_half(a.dtype):
        if K % 64:
            return None
        code = dtype_code(a.dtype)
    else:  # float32 on the matrix cores: pre-split weights (and, with the pre-split activation format, a pre-split A operand)
        if not (a.dtype == torch.float32 and getattr(w, "_split", False) and K % 32 == 0):
            return None
        code = GMD_F32SA if is_asplit(a) else GMD_F32SW
    if not lib().gmd_gemm_qkv_vt_ok(code, M, N, K, vt_col0, tokens, WORKSPACE_BYTES):
        return None
    qk = torch.empty((M, vt_col0), dtype=a.dtype, device=a.device)
    vt = torch.empty((M // tokens, N - vt_col0, tokens), dtype=a.dtype, device=a.device)
    ws = _workspace(a.device)
    tm = profiling.active()
    tm = tm if tm is not None and tm.wants("gemm_nt") else None
    t0 = tm.begin() if tm else None
    check(lib().gmd_gemm_qkv_vt(_ptr(a), _ptr(w), _ptr(qk), _ptr(vt), code, M, N, K, vt_col0, vt_col0, tokens, tokens,
                                float(getattr(w, "_alpha", 1.0)), _ptr(ws), WORKSPACE_BYTES, _stream()), "gmd_gemm_qkv_vt")
    if tm:
        tm.end("gemm_nt", 2.0 * M * N * K, (M * K + N * K + M * N) * a.element_size(), t0)
    return qk, vt


# The GEGLU feed-forward as one launch (csrc/ff_fused.hip) where the kernel is instantiated; GMD_FUSED_FF=0 keeps the two
# GEMM launches (A/B measurements, tests).
USE_FUSED_FF = os.environ.get("GMD_FUSED_FF", "1") != "0"
# One 128-row workgroup per CU: below ~7/8 of the chip's 256 CUs the two tiled GEMM launches (two workgroups per CU, 512+ tiles)
# are faster -- tools/bench_ff.py: M = 32768 90 vs 124 us, M = 16384 (half the chip) 82 vs 67 us.
FUSED_FF_MIN_ROWS = int(os.environ.get("GMD_FUSED_FF_MIN_ROWS", str(224 * 128)))
# ... inside a co-running forward (plan family 1) from half the chip up: beside the other stream's kernels CU-time, not the launch's
# own time, is what counts, and 128 fused workgroups cost less of it than the 1280 + 256 of the two launches (round 5, interleaved
# A/B of whole bench.py runs: 752.7 -> 751.3 ms per batch, 3 of 3 rounds; fusion off altogether: 757.4)
FUSED_FF_MIN_ROWS_CO_RUN = int(os.environ.get("GMD_FUSED_FF_MIN_ROWS_CO_RUN", str(128 * 128)))


def ff_fused_ok(x, C, min_rows=None):
    if min_rows is None:
        min_rows = FUSED_FF_MIN_ROWS_CO_RUN if lib().gmd_gemm_plan_family(-1) == 1 else FUSED_FF_MIN_ROWS
    return (USE_FUSED_FF and is_half(x.dtype) and x.dim() == 2 and x.shape[0] >= min_rows and
            bool(lib().gmd_ff_geglu_fused_supported(dtype_code(x.dtype), x.shape[0], C)))


def ff_geglu_fused(x, w1i, b1i, w2, b2, residual):
    """``(value * gelu(gate)) @ w2.T + b2 + residual`` with ``[value | gate] = x @ w1i.T + b1i`` (interleaved rows)."""
    _dev(x, w1i, b1i, w2, b2, residual)
    M, C = x.shape
    if w1i.shape != (8 * C, C) or w2.shape != (C, 4 * C) or residual.shape != x.shape or not (x.dtype == w1i.dtype == w2.dtype == residual.dtype):
        raise HipExtensionError("ff_geglu_fused: operand shapes / dtypes inconsistent")
    y = torch.empty_like(x)
    tm = profiling.active()
    tm = tm if tm is not None and tm.wants("gemm_nt") else None
    t0 = tm.begin() if tm else None
    check(lib().gmd_ff_geglu_fused(_ptr(x), _ptr(w1i), _ptr(_f32(b1i, "b1")), _ptr(w2), _ptr(_f32(b2, "b2")), _ptr(residual), _ptr(y),
                                   dtype_code(x.dtype), M, C, _stream()), "gmd_ff_geglu_fused")
    if tm:  # both products' algorithmic FLOPs; bytes: x, residual, y once + the weights
        es = x.element_size()
        tm.end("gemm_nt", 2.0 * M * C * 8 * C + 2.0 * M * 4 * C * C, (3 * M * C + 12 * C * C) * es, t0)
    return y


def upsample_code(H, W, out_size):
    """The ``upsample`` argument of the C ABI for nearest upsampling of an H x W map to ``out_size`` = (Hout, Wout), each side
    ``2 * in - 1`` or ``2 * in`` (GMD_UPSAMPLE_TO of include/gmd_hip.h; exactly 2x is the plain ``1``, the launch of ``upsample=True``)."""
    ho, wo = (int(v) for v in out_size)
    if ho not in (2 * H - 1, 2 * H) or wo not in (2 * W - 1, 2 * W) or ho < 1 or wo < 1 or ho >= 1 << 15 or wo >= 1 << 16:
        raise HipExtensionError(f"conv3x3: out_size {ho}x{wo} from {H}x{W}: each side must be 2*in - 1 or 2*in")
    return 1 if (ho, wo) == (2 * H, 2 * W) else (ho << 16) | wo


def conv3x3(x, w, B, H, W, bias=None, rowbias=None, residual=None, stride=1, upsample=False, pad_mode=0, out_dtype=None,
            colstats=False, x_split=False, out_size=None):
    """x: [B, H*W, Cin]; w: [Cout, 9*Cin] (tap-major); returns ([B, Hout*Wout, Cout], Hout, Wout).  ``upsample=True`` convolves the
    nearest-2x image; ``out_size=(Hout, Wout)`` the nearest-upsampled image of that size (diffusers' ``Upsample2D(x, output_size)``;
    each side ``2 * in - 1`` or ``2 * in``)."""
    _dev(x, w, bias, residual)
    rb_ptr, rb_ld = _rowbias(rowbias)
    cin, cout = x.shape[-1], w.shape[0]
    if x.numel() != B * H * W * cin or w.shape[1] != 9 * cin or x.dtype != w.dtype:
        raise HipExtensionError(f"conv3x3: shape/dtype mismatch x={tuple(x.shape)} w={tuple(w.shape)} B,H,W={B},{H},{W}")
    up = int(bool(upsample))
    if out_size is not None:
        if stride != 1 or pad_mode != 0:
            raise HipExtensionError("conv3x3: out_size is the upsampling convolution's (stride 1, pad_mode 0)")
        up = upsample_code(H, W, out_size)
        ho, wo = int(out_size[0]), int(out_size[1])
    elif upsample:
        ho, wo = 2 * H, 2 * W
    elif pad_mode == 1:
        ho, wo = (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1
    else:
        ho, wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    out_dtype = out_dtype or x.dtype
    y = torch.empty((B, ho * wo, cout), dtype=out_dtype, device=x.device)
    if residual is not None and (residual.numel() != y.numel() or residual.dtype != x.dtype):
        raise HipExtensionError("conv3x3: residual shape/dtype mismatch")
    if rowbias is not None and (rowbias[0] if isinstance(rowbias, tuple) else rowbias).shape[0] != B:
        raise HipExtensionError("conv3x3: rowbias must have one row per sample")
    ws = _workspace(x.device)
    x_split = bool(x_split) or is_asplit(x)
    code = _contract_code(x, w, cin, x_split)
    st = _colstats_buffer(colstats, x.dtype, B * ho * wo, cout, 9 * cin, 1, out_dtype, x.device, code=code)
    tm = profiling.active()
    tm = tm if tm is not None and tm.wants("conv3x3") else None
    t0 = tm.begin() if tm else None
    check(lib().gmd_conv3x3(_ptr(x), _ptr(w), _ptr(y), code, dtype_code(out_dtype), B, H, W, cin, cout,
                            stride, up, pad_mode, _ptr(_f32(bias, "bias")), rb_ptr, rb_ld,
                            _ptr(residual), float(getattr(w, "_alpha", 1.0)), _ptr(st), COLSTATS_BUCKET if st is not None else 0,
                            _ptr(ws), WORKSPACE_BYTES, _stream()), "gmd_conv3x3")
    if tm:
        tm.end("conv3x3", 2.0 * B * ho * wo * cout * 9 * cin, x.numel() * x.element_size() + w.numel() * w.element_size()
               + y.numel() * y.element_size(), t0)
    if st is not None:
        y._colstats = (st, cout)
    return y, ho, wo


# ResnetBlock2D's conv2(h) + conv_shortcut(x) as ONE launch (gmd_conv3x3_tail): the shortcut projection is K2/64 more steps of conv2's
# K loop over the packed weight [W2 | Wsc], summed in the float32 accumulator; its [M, Cout] tensor is never written.
# GMD_FUSE_SHORTCUT=0 keeps the two launches (A/B measurements, tests).
USE_SHORTCUT_FOLD = os.environ.get("GMD_FUSE_SHORTCUT", "1") != "0"
shortcut_fold_uses = 0   # fused launches issued (tests assert the path is really taken)
shortcut_launches = 0    # separate conv_shortcut projections issued by the models' resnets


def pack_shortcut(w2, b2, wsc, bsc):
    """([W2 | Wsc] as one [Cout, 9*Cin + K2] matrix, b2 + bsc in float32) for conv3x3_tail.  The weights are copied bit for bit (no
    re-rounding); a side without a bias counts as zero."""
    if w2.dim() != 2 or wsc.dim() != 2 or w2.shape[0] != wsc.shape[0] or w2.dtype != wsc.dtype or w2.device != wsc.device:
        raise HipExtensionError(f"pack_shortcut: W2 {tuple(w2.shape)} {w2.dtype} and Wsc {tuple(wsc.shape)} {wsc.dtype} do not stack")
    if getattr(w2, "_split", False) or getattr(wsc, "_split", False) or getattr(w2, "_alpha", 1.0) != 1.0 or getattr(wsc, "_alpha", 1.0) != 1.0:
        raise HipExtensionError("pack_shortcut: plain (unscaled, unsplit) weights only")
    w = torch.cat([w2, wsc], 1).contiguous()
    b = None
    if b2 is not None or bsc is not None:
        zero = torch.zeros(w.shape[0], dtype=torch.float32, device=w.device)
        b = ((zero if b2 is None else _f32(b2, "bias")) + (zero if bsc is None else _f32(bsc, "bias"))).contiguous()
    return w, b


def shortcut_fold_ok(dtype, B, H, W, cin, k2, cout):
    """Does ``conv3x3_tail`` of these dimensions launch (16-bit, K2 a multiple of 64, and the 256-row ping-pong plan, the one kernel
    whose loader walks the tail)?  The calling thread's plan family counts, as for the launch itself."""
    if not USE_SHORTCUT_FOLD or not is_half(dtype) or k2 <= 0 or k2 % 64 or cin % 64:
        return False
    bm, bn, pf, _ = gemm_plan_info(dtype, B * H * W, cout, 9 * cin + k2)
    return pf == 283 and bm == 256 and bn in (128, 160)


def conv3x3_tail(x, x2, w, B, H, W, bias=None, rowbias=None, residual=None, out_dtype=None, colstats=False, ldx2=None, k2=None,
                 stride=1, upsample=False):
    """``conv3x3(x, w[:, :9*Cin]) + x2 @ w[:, 9*Cin:].T`` (+ bias, rowbias, residual) as one launch.  x: [B, H*W, Cin]; x2: [B, H*W, K2]
    (or rows of ``ldx2`` >= K2 elements of which the first ``k2`` count); w: [Cout, 9*Cin + K2] from ``pack_shortcut``.  Returns
    ([B, H*W, Cout], H, W).  Raises where ``shortcut_fold_ok`` is false (stride / upsample exist only to be refused by the library)."""
    global shortcut_fold_uses
    _dev(x, x2, w, bias, residual)
    rb_ptr, rb_ld = _rowbias(rowbias)
    cin, cout = x.shape[-1], w.shape[0]
    ldx2 = int(ldx2 or x2.shape[-1])
    k2 = int(k2 if k2 is not None else x2.shape[-1])
    if (x.numel() != B * H * W * cin or x2.numel() != B * H * W * ldx2 or w.shape[1] != 9 * cin + k2 or x.dtype != w.dtype
            or x2.dtype != w.dtype or k2 > ldx2):
        raise HipExtensionError(f"conv3x3_tail: shape/dtype mismatch x={tuple(x.shape)} x2={tuple(x2.shape)} w={tuple(w.shape)} B,H,W={B},{H},{W}")
    if getattr(w, "_split", False) or is_asplit(x) or is_asplit(x2):
        raise HipExtensionError("conv3x3_tail: plain operands only")
    out_dtype = out_dtype or x.dtype
    y = torch.empty((B, H * W, cout), dtype=out_dtype, device=x.device)
    if residual is not None and (residual.numel() != y.numel() or residual.dtype != x.dtype):
        raise HipExtensionError("conv3x3_tail: residual shape/dtype mismatch")
    if rowbias is not None and (rowbias[0] if isinstance(rowbias, tuple) else rowbias).shape[0] != B:
        raise HipExtensionError("conv3x3_tail: rowbias must have one row per sample")
    ws = _workspace(x.device)
    code = dtype_code(x.dtype)
    st = _colstats_buffer(colstats, x.dtype, B * H * W, cout, 9 * cin + k2, 1, out_dtype, x.device) if is_half(x.dtype) else None
    tm = profiling.active()
    tm = tm if tm is not None and tm.wants("conv3x3") else None
    t0 = tm.begin() if tm else None
    check(lib().gmd_conv3x3_tail(_ptr(x), _ptr(x2), _ptr(w), _ptr(y), code, dtype_code(out_dtype), B, H, W, cin, k2, ldx2, cout,
                                 int(stride), int(bool(upsample)), 0, _ptr(_f32(bias, "bias")), rb_ptr, rb_ld, _ptr(residual), 1.0,
                                 _ptr(st), COLSTATS_BUCKET if st is not None else 0, _ptr(ws), WORKSPACE_BYTES, _stream()), "gmd_conv3x3_tail")
    if tm:
        tm.end("conv3x3", 2.0 * B * H * W * cout * (9 * cin + k2), (x.numel() + x2.numel() + w.numel()) * x.element_size()
               + y.numel() * y.element_size(), t0)
    shortcut_fold_uses += 1
    if st is not None:
        y._colstats = (st, cout)
    return y, H, W


# Upsample2D (nearest 2x, then conv3x3) as four 2x2 phase convolutions over the low-resolution image (gmd_conv3x3_up2): output pixel
# (2i + py, 2j + px) reads only a 2x2 window of source pixels, so the nine taps collapse to four whose weights are sums of the taps
# that hit the same source pixel -- K = 4 Cin instead of 9 Cin.  GMD_UPSAMPLE_PHASES=0 keeps the nine-tap launches (A/B runs, tests).
USE_UPSAMPLE_PHASES = os.environ.get("GMD_UPSAMPLE_PHASES", "1") != "0"
upsample_phase_uses = 0  # phase launches issued (tests assert the path is really taken)
_PHASE_TAPS = (((0,), (1, 2)), ((0, 1), (2,)))  # [phase bit][a] -> the nine-tap indices that read source offset a + phase bit - 1


def pack_upsample_phases(w, bias=None):
    """(``[4, Cout, 4*Cin]`` phase weights, bias) for ``conv3x3_up2`` from the nine-tap ``w`` = [Cout, 9*Cin] (tap-major).  Phase
    ``z = 2*py + px``; inside a phase tap ``(a, b)`` (tap-major, ``2*a + b``) reads source pixel ``(i + a + py - 1, j + b + px - 1)`` and
    holds the sum of the nine-tap weights ``(ky, kx)`` that read that pixel: py = 0: a = 0 <- ky 0, a = 1 <- ky 1 + 2; py = 1: a = 0 <-
    ky 0 + 1, a = 1 <- ky 2; the same in x.  Sums are formed in float32 (a wider ``w`` in its own type) and rounded ONCE to ``w.dtype``."""
    if w.dim() != 2 or w.shape[1] % 9:
        raise HipExtensionError(f"pack_upsample_phases: w {tuple(w.shape)} is not [Cout, 9*Cin]")
    if getattr(w, "_split", False) or getattr(w, "_alpha", 1.0) != 1.0:
        raise HipExtensionError("pack_upsample_phases: plain (unscaled, unsplit) weights only")
    co, ci = w.shape[0], w.shape[1] // 9
    w9 = w.to(torch.float32 if is_half(w.dtype) else w.dtype).view(co, 3, 3, ci)
    out = torch.empty((4, co, 4, ci), dtype=w9.dtype, device=w.device)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    out[2 * py + px, :, 2 * a + b] = sum(w9[:, ky, kx] for ky in _PHASE_TAPS[py][a] for kx in _PHASE_TAPS[px][b])
    return out.view(4, co, 4 * ci).to(w.dtype).contiguous(), (None if bias is None else _f32(bias, "bias"))


def _up2_plan(dtype, B, H, W, cin, cout, bucket):
    import ctypes

    out = (ctypes.c_int * 4)()
    ok = lib().gmd_conv3x3_up2_plan(dtype_code(dtype), B, H, W, cin, cout, bucket, WORKSPACE_BYTES, ctypes.addressof(out))
    return tuple(out) if ok else None


def upsample_phases_plan(dtype, B, H, W, cin, cout, colstats=False):
    """(tile rows, tile columns, kernel code, K slices) of the phase launch, or None where there is none (tests, tools)."""
    return _up2_plan(dtype, B, H, W, cin, cout, COLSTATS_BUCKET if colstats else 0) if is_half(dtype) else None


def _up2_statistics(dtype, B, H, W, cin, cout, colstats):
    """None: no phase launch; else whether it emits column statistics.  A nine-tap launch that WOULD emit the statistics asked for
    keeps the launch when the phase form cannot (the next GroupNorm would need its own statistics pass)."""
    if not is_half(dtype) or cin % 64:
        return None
    if colstats and USE_COLSTATS and cout % COLSTATS_BUCKET == 0 and (4 * B * H * W) % 64 == 0:
        if _up2_plan(dtype, B, H, W, cin, cout, COLSTATS_BUCKET) is not None:
            return True
        if lib().gmd_gemm_colstats_plan(dtype_code(dtype), 4 * B * H * W, cout, 9 * cin, 1, WORKSPACE_BYTES, COLSTATS_BUCKET):
            return None
    return False if _up2_plan(dtype, B, H, W, cin, cout, 0) is not None else None


def upsample_phases_ok(dtype, B, H, W, cin, cout, out_size=None, colstats=False):
    """Does ``conv3x3_up2`` of these dimensions launch?  16-bit dtype, output exactly (2H, 2W) (``out_size`` None = that), Cin a
    multiple of 64, H*W a multiple of 64 when statistics are wanted (``colstats``) and would otherwise come out of the nine-tap
    launch, and the 256-row ping-pong plan (code 283) for the phase GEMM under the calling thread's plan family."""
    if not USE_UPSAMPLE_PHASES or (out_size is not None and (int(out_size[0]), int(out_size[1])) != (2 * H, 2 * W)):
        return False
    return _up2_statistics(dtype, B, H, W, cin, cout, colstats) is not None


def conv3x3_up2(x, wp, B, H, W, bias=None, rowbias=None, residual=None, out_dtype=None, colstats=False, out=None):
    """``conv3x3(x, w, upsample=True)`` from the phase weights ``wp = pack_upsample_phases(w)[0]``: x [B, H*W, Cin] -> ([B, 4*H*W, Cout],
    2H, 2W).  ``out``: a contiguous tensor of that shape to store into (tests).  Raises where ``upsample_phases_ok`` is false."""
    global upsample_phase_uses
    _dev(x, wp, bias, residual)
    rb_ptr, rb_ld = _rowbias(rowbias)
    cin = x.shape[-1]
    if wp.dim() != 3 or wp.shape[0] != 4 or wp.shape[2] != 4 * cin or x.numel() != B * H * W * cin or x.dtype != wp.dtype or not wp.is_contiguous():
        raise HipExtensionError(f"conv3x3_up2: shape/dtype mismatch x={tuple(x.shape)} wp={tuple(wp.shape)} B,H,W={B},{H},{W}")
    if getattr(wp, "_split", False) or is_asplit(x):
        raise HipExtensionError("conv3x3_up2: plain operands only")
    cout = wp.shape[1]
    out_dtype = out_dtype or x.dtype
    ho, wo = 2 * H, 2 * W
    if out is None:
        y = torch.empty((B, ho * wo, cout), dtype=out_dtype, device=x.device)
    else:
        _dev(out)
        if out.shape != (B, ho * wo, cout) or out.dtype != out_dtype or not out.is_contiguous():
            raise HipExtensionError(f"conv3x3_up2: out {tuple(out.shape)} {out.dtype} is not a contiguous [{B}, {ho * wo}, {cout}] {out_dtype}")
        y = out
    if residual is not None and (residual.numel() != y.numel() or residual.dtype != x.dtype):
        raise HipExtensionError("conv3x3_up2: residual shape/dtype mismatch")
    if rowbias is not None and (rowbias[0] if isinstance(rowbias, tuple) else rowbias).shape[0] != B:
        raise HipExtensionError("conv3x3_up2: rowbias must have one row per sample")
    ws = _workspace(x.device)
    st = None
    if out_dtype == x.dtype and _up2_statistics(x.dtype, B, H, W, cin, cout, colstats):
        st = torch.empty((B * ho * wo // 64, cout // COLSTATS_BUCKET, 2), dtype=torch.float32, device=x.device)
    tm = profiling.active()
    tm = tm if tm is not None and tm.wants("conv3x3") else None
    t0 = tm.begin() if tm else None
    check(lib().gmd_conv3x3_up2(_ptr(x), _ptr(wp), _ptr(y), dtype_code(x.dtype), dtype_code(out_dtype), B, H, W, cin, cout,
                                _ptr(_f32(bias, "bias")), rb_ptr, rb_ld, _ptr(residual), _ptr(st), COLSTATS_BUCKET if st is not None else 0,
                                _ptr(ws), WORKSPACE_BYTES, _stream()), "gmd_conv3x3_up2")
    if tm:  # the products the launch performs: 4 taps per output pixel
        tm.end("conv3x3", 2.0 * B * ho * wo * cout * 4 * cin, x.numel() * x.element_size() + wp.numel() * wp.element_size()
               + y.numel() * y.element_size(), t0)
    upsample_phase_uses += 1
    if st is not None:
        y._colstats = (st, cout)
    return y, ho, wo


USE_CONV_GN_FUSION = os.environ.get("GMD_CONV_GN", "1") != "0"  # (the switch: A/B measurements only)


def conv3x3_groupnorm(x, w, B, H, W, groups, gamma, beta, eps, silu=True, bias=None, rowbias=None, residual=None, want_raw=False,
                      colstats=False, split_out=False):
    """GroupNorm(+SiLU) of conv3x3(x): returns (raw or None, normalised).  Where the convolution runs split-K and the group slices
    are small (the 16x16 / 8x8 UNet levels) ONE GroupNorm launch sums the partial slabs, applies the convolution's epilogue and
    normalises (gmd_conv3x3_groupnorm: no reduce launch, the raw tensor is written only if ``want_raw``); everywhere else this
    is conv3x3 (+ producer statistics if ``colstats``) followed by groupnorm -- bit-identical either way."""
    _dev(x, w, bias, residual, gamma, beta)
    cin, cout = x.shape[-1], w.shape[0]
    code = _contract_code(x, w, cin, is_asplit(x)) if x.dtype == w.dtype and w.shape[1] == 9 * cin else -1
    if not (USE_CONV_GN_FUSION and code >= 0 and
            lib().gmd_conv3x3_gn_fusable(code, B, H, W, cin, cout, 1, 0, 0, groups, WORKSPACE_BYTES)):
        y, _, _ = conv3x3(x, w, B, H, W, bias=bias, rowbias=rowbias, residual=residual, colstats=colstats)
        return (y if want_raw else None), groupnorm(y, B, groups, gamma, beta, eps, silu=silu, split_out=split_out)
    if x.numel() != B * H * W * cin:
        raise HipExtensionError(f"conv3x3_groupnorm: shape mismatch x={tuple(x.shape)} B,H,W={B},{H},{W}")
    if residual is not None and (residual.numel() != B * H * W * cout or residual.dtype != x.dtype):
        raise HipExtensionError("conv3x3_groupnorm: residual shape/dtype mismatch")
    if rowbias is not None and (rowbias[0] if isinstance(rowbias, tuple) else rowbias).shape[0] != B:
        raise HipExtensionError("conv3x3_groupnorm: rowbias must have one row per sample")
    rb_ptr, rb_ld = _rowbias(rowbias)
    yn = torch.empty((B, H * W, cout), dtype=x.dtype, device=x.device)
    yr = torch.empty_like(yn) if want_raw else None
    ws = _workspace(x.device)
    tm = profiling.active()
    tm = tm if tm is not None and tm.wants("conv3x3") else None
    t0 = tm.begin() if tm else None
    check(lib().gmd_conv3x3_groupnorm(_ptr(x), _ptr(w), _ptr(yr), _ptr(yn), code, B, H, W, cin, cout, 1, 0, 0, _ptr(_f32(bias, "bias")),
                                      rb_ptr, rb_ld, _ptr(residual), float(getattr(w, "_alpha", 1.0)), groups, float(eps),
                                      _ptr(_f32(gamma, "gamma")), _ptr(_f32(beta, "beta")), int(silu), _ptr(ws), WORKSPACE_BYTES, _stream()),
          "gmd_conv3x3_groupnorm")
    if tm:  # counted as the convolution it replaces (its FLOPs; the GroupNorm's bytes ride along)
        tm.end("conv3x3", 2.0 * B * H * W * cout * 9 * cin, x.numel() * x.element_size() + w.numel() * w.element_size()
               + yn.numel() * yn.element_size(), t0)
    return yr, yn


SPLIT_ATTENTION_HEAD_DIMS = (40, 64, 80, 160)  # float32 flash kernel (attention_split.hip): SD-1.5's head dims and SDXL's 64


def split_attention_ok(dtype, d):
    """True when ``attention`` takes float32 tensors of this head dim (F32_MODE 'split')."""
    return dtype == torch.float32 and f32_split() and d in SPLIT_ATTENTION_HEAD_DIMS


def attention(q, k, vt, heads, nk, scale, k_col=0, causal=False, split_out=False):
    """q: [B, Nq, ldq] with Q in columns [0, H*D); k: [B, Nk, ldk] with K in columns [k_col, k_col+H*D)
    (q and k may be the same fused-projection buffer); vt: [B, H*D, ldvt] (V transposed, keys contiguous).
    ``split_out`` (float32 matrix-core mode): store O pre-split for the out-projection (the result carries the mark, is_asplit)."""
    _dev(q, k, vt)
    B, nq = q.shape[0], q.shape[1]
    hd = vt.shape[1]
    d = hd // heads
    ldq, ldk = q.shape[2], k.shape[2]
    if k.shape[1] < nk or vt.shape[2] < nk or k_col + hd > ldk or hd > ldq:
        raise HipExtensionError("attention: operand shapes inconsistent")
    o = torch.empty((B, nq, hd), dtype=q.dtype, device=q.device)
    if q.dtype == torch.float32:
        if not (f32_split() and d in SPLIT_ATTENTION_HEAD_DIMS):
            raise HipExtensionError("attention: float32 runs on the split (three float16 products) kernel, head dims 40/64/80/160, "
                                    "in F32_MODE 'split' only; the exact float32 path composes gemm_nt + softmax_rows")
        so = bool(split_out) and want_split_out(q.dtype, hd)
        code = GMD_F32SA if so else GMD_F32S
    else:
        so = False
        code = dtype_code(q.dtype)
    tm = profiling.active()
    tm = tm if tm is not None and tm.wants("attention") else None
    t0 = tm.begin() if tm else None
    check(lib().gmd_attention(_ptr(q), _ptr(k) + k_col * k.element_size(), _ptr(vt), _ptr(o), code, B, heads, d,
                              nq, nk, ldq, ldk, vt.shape[2], hd, nq * ldq, k.shape[1] * ldk, hd * vt.shape[2], nq * hd,
                              float(scale), int(bool(causal)), _stream()), "gmd_attention")
    if tm:  # QK^T + PV, algorithmic head dim (padding not counted)
        tm.end("attention", 4.0 * B * nq * nk * hd, (2 * B * nq * hd + 2 * B * nk * hd) * q.element_size(), t0)
    return _mark_asplit(o) if so else o


# Decoupled cross-attention of an IP-Adapter: the 16-bit types take ONE launch (gmd_attention_ip).  GMD_ATTN_IP_FUSED=0 (read once)
# sends them down the composed route instead -- two attention launches and scaled_add, what float32 always runs: the A/B switch.
USE_ATTN_IP_FUSED = os.environ.get("GMD_ATTN_IP_FUSED", "1") != "0"
ATTN_IP_MAX_KEYS = 64  # the image keys are one tile of the kernel


def _ip_scale_arg(ip_scales, ip_index, what):
    if ip_scales is None or ip_scales.dtype != torch.float32 or not ip_scales.is_contiguous():
        raise HipExtensionError(f"{what}: ip_scales must be a contiguous float32 device tensor")
    if not 0 <= int(ip_index) < ip_scales.numel():
        raise HipExtensionError(f"{what}: scale index {ip_index} outside [0, {ip_scales.numel()})")
    return int(ip_index)


def scaled_add(a, b, scales, index, out=None):
    """``a + b * scales[index]`` in float32, one rounding on the store (gmd_scaled_add); ``scales`` is a float32 device tensor read by
    the kernel.  ``out`` may be ``a`` (in place)."""
    _dev(a, b, scales)
    if a.dtype != b.dtype or a.shape != b.shape or not a.is_contiguous() or not b.is_contiguous():
        raise HipExtensionError("scaled_add: a and b must be contiguous tensors of one shape and dtype")
    if is_asplit(a) or is_asplit(b):
        raise HipExtensionError("scaled_add: an input is a pre-split activation (only contractions read that layout)")
    index = _ip_scale_arg(scales, index, "scaled_add")
    if out is None:
        out = torch.empty_like(a)
    elif out.dtype != a.dtype or out.shape != a.shape or not out.is_contiguous():
        raise HipExtensionError("scaled_add: out must match a")
    check(lib().gmd_scaled_add(_ptr(a), _ptr(b), _ptr(out), dtype_code(a.dtype), a.numel(), _ptr(scales), index, _stream()),
          "gmd_scaled_add")
    return out


def attention_ip_composed(q, k, vt, kip, vtip, heads, nk, nip, scale, ip_scales, ip_index):
    """The decoupled cross-attention as two ``attention`` launches and ``scaled_add``: float32 in F32_MODE 'split', and the baseline
    the fused kernel is measured against (16-bit types)."""
    index = _ip_scale_arg(ip_scales, ip_index, "attention_ip")
    o = attention(q, k, vt, heads, nk, scale)
    oi = attention(q, kip, vtip, heads, nip, scale)
    return scaled_add(o, oi, ip_scales, index, out=o)


def attention_ip(q, k, vt, kip, vtip, heads, nk, nip, scale, ip_scales, ip_index, fused=None):
    """``softmax(scale q k^T) v + ip_scales[ip_index] * softmax(scale q kip^T) vip``: two independent softmaxes over the text keys and
    the ``nip`` <= 64 image keys.  q: [B, Nq, ldq] and k: [B, Nk, ldk] with the heads in columns [0, H*D); vt: [B, H*D, ldvt]; kip:
    [B, Nip, ldkip]; vtip: [B, H*D, ldvtip] (zero pad columns, as vt).  ``ip_scales``: float32
    device tensor read by the kernel, so a captured graph serves every scale.  16-bit types: one launch (gmd_attention_ip) unless
    ``fused`` is False (default: USE_ATTN_IP_FUSED); float32: the composed route."""
    _dev(q, k, vt, kip, vtip, ip_scales)
    index = _ip_scale_arg(ip_scales, ip_index, "attention_ip")
    B, nq = q.shape[0], q.shape[1]
    hd = vt.shape[1]
    d = hd // heads
    ldq, ldk = q.shape[2], k.shape[2]
    if not 1 <= nip <= ATTN_IP_MAX_KEYS:
        raise HipExtensionError(f"attention_ip: {nip} image keys outside [1, {ATTN_IP_MAX_KEYS}]")
    if (k.shape[1] < nk or vt.shape[2] < nk or hd > ldk or hd > ldq or kip.shape[0] != B or kip.shape[1] < nip
            or kip.shape[2] < hd or vtip.shape[0] != B or vtip.shape[1] != hd or vtip.shape[2] < nip or k.shape[0] != B or vt.shape[0] != B):
        raise HipExtensionError("attention_ip: operand shapes inconsistent")
    fused = USE_ATTN_IP_FUSED if fused is None else bool(fused)
    if not (is_half(q.dtype) and fused):
        return attention_ip_composed(q, k, vt, kip, vtip, heads, nk, nip, scale, ip_scales, index)
    o = torch.empty((B, nq, hd), dtype=q.dtype, device=q.device)
    es = q.element_size()
    tm = profiling.active()
    tm = tm if tm is not None and tm.wants("attention") else None
    t0 = tm.begin() if tm else None
    check(lib().gmd_attention_ip(_ptr(q), _ptr(k), _ptr(vt), _ptr(kip), _ptr(vtip), _ptr(o), dtype_code(q.dtype),
                                 B, heads, d, nq, nk, nip, ldq, ldk, vt.shape[2], kip.shape[2], vtip.shape[2], hd,
                                 nq * ldq, k.shape[1] * ldk, hd * vt.shape[2], kip.shape[1] * kip.shape[2], hd * vtip.shape[2], nq * hd,
                                 float(scale), _ptr(ip_scales), index, _stream()), "gmd_attention_ip")
    if tm:  # both branches' QK^T + PV; Q and O move once
        tm.end("attention", 4.0 * B * nq * (nk + nip) * hd, (2 * B * nq * hd + 2 * B * (nk + nip) * hd) * es, t0)
    return o


# A LoRA adapter applied at run time: y += scales[index] * (x a^T) b^T.  The 16-bit types take ONE launch (gmd_lora_update);
# GMD_LORA_FUSED=0 (read once) sends them down the composed route instead -- two gemm_nt launches and scaled_add, what float32 always
# runs: the A/B switch.
USE_LORA_FUSED = os.environ.get("GMD_LORA_FUSED", "1") != "0"
LORA_MAX_RANK = 128  # the kernel's limit (components/lora.py refuses larger adapters at load with this very number)


def lora_rank_multiple(dtype, split=None):
    """Multiple the host zero-pads an adapter's rank to: 32 for the fused 16-bit launch, the K multiple of the float32 contraction
    mode otherwise (``split``: a module's own recorded mode; default: the calling thread's)."""
    split = (f32_mode() == "split") if split is None else bool(split)
    return 32 if (is_half(dtype) or split) else 16


def lora_update(x, a, b, y, scales, index, transposed=False, tokens=None, fused=None, col=0, x_split=False):
    """``y += scales[index] * (x @ a.T) @ b.T`` in place; returns ``y``.  x: [M, K]; a: [Rp, K] and b: [N, Rp], the adapter's factors
    with the rank zero-padded to ``lora_rank_multiple`` (float32: prepared like the model's weights, a pre-split ``a`` for a pre-split
    ``x``).  Plain mode: y is a contiguous [M, ldy] buffer and columns [col, col + N) of it are updated (the q and k ranges of a stacked
    q | k buffer).  ``transposed``: y is a contiguous V^T [batch, N, ldy] with M = batch * ``tokens`` and row b * tokens + tok of the
    update lands at y[b, n, tok]; the pad columns [tokens, ldy) are not touched.  ``scales``: float32 device tensor read by the kernels, so
    a captured graph serves every scale.  ``x_split``: x is a VIEW of a pre-split activation (views do not carry the mark).  16-bit types:
    one launch (gmd_lora_update) unless ``fused`` is False (default: USE_LORA_FUSED); float32: two gemm_nt launches and scaled_add."""
    _dev(x, a, b, y, scales)
    index = _ip_scale_arg(scales, index, "lora_update")
    if not (x.dtype == a.dtype == b.dtype == y.dtype):
        raise HipExtensionError(f"lora_update: dtype mismatch {x.dtype} / {a.dtype} / {b.dtype} / {y.dtype}")
    if x.dim() != 2 or a.dim() != 2 or b.dim() != 2 or a.shape[1] != x.shape[1] or b.shape[1] != a.shape[0]:
        raise HipExtensionError(f"lora_update: operand shapes inconsistent: x {tuple(x.shape)}, a {tuple(a.shape)}, b {tuple(b.shape)}")
    if is_asplit(y):
        raise HipExtensionError("lora_update: y is a pre-split activation (only contractions read that layout)")
    M, K = x.shape
    N, Rp = b.shape
    if transposed:
        if y.dim() != 3 or tokens is None or tokens <= 0 or y.shape[0] * tokens != M or y.shape[1] != N or y.shape[2] < tokens or col:
            raise HipExtensionError(f"lora_update: transposed y {tuple(y.shape)} does not hold [M / tokens, N, >= tokens] for M={M}, N={N}, "
                                    f"tokens={tokens}")
        batch, ldy = y.shape[0], y.shape[2]
    else:
        if y.dim() != 2 or y.shape[0] != M or col < 0 or col + N > y.shape[1]:
            raise HipExtensionError(f"lora_update: y {tuple(y.shape)} does not hold columns [{col}, {col + N}) of {M} rows")
        batch, tokens, ldy = 1, M, y.shape[1]
    fused = USE_LORA_FUSED if fused is None else bool(fused)
    if is_half(x.dtype) and K % 64:
        raise HipExtensionError(f"lora_update: K={K} must be a multiple of 64 in the 16-bit types (the fused launch and gemm_nt alike)")
    if is_half(x.dtype) and not transposed and N % 8:
        fused = False  # the fused launch moves Y in 16-byte pieces of a row: a ragged N takes the composed route
    if is_half(x.dtype) and fused:
        if Rp > LORA_MAX_RANK:
            raise HipExtensionError(f"lora_update: padded rank {Rp} above {LORA_MAX_RANK}")
        tm, t0 = _timed("lora_update")
        check(lib().gmd_lora_update(_ptr(x), _ptr(a), _ptr(b), y.data_ptr() + col * y.element_size(), dtype_code(x.dtype), M, K, Rp, N, K, ldy,
                                    int(bool(transposed)), batch, tokens, N * ldy, _ptr(scales), index, _stream()), "gmd_lora_update")
        if tm:
            tm.end("lora_update", 2.0 * M * Rp * (K + N), (M * K + 2 * M * N + Rp * (K + N)) * x.element_size(), t0)
        return y
    # composed: T = x a^T, U = T b^T in y's layout (zero where y is not updated: s * 0 leaves those elements), y += s U
    if is_half(x.dtype) and Rp % 64:  # the 16-bit gemm_nt contracts over multiples of 64: more zero rank columns (A/B route only)
        a = torch.nn.functional.pad(a, (0, 0, 0, 64 - Rp % 64))
        b = torch.nn.functional.pad(b, (0, 64 - Rp % 64))
        Rp = b.shape[1]
    t = gemm_nt(x, a, a_split=bool(x_split) or is_asplit(x))
    # zero where y is not updated; where the second product writes every element of u nothing needs clearing
    covers = (ldy == tokens) if transposed else (col == 0 and ldy == N)
    u = torch.empty_like(y) if covers else torch.zeros_like(y)
    if transposed:
        gemm_nt(b, t.view(batch, tokens, Rp), out=u, ldc=ldy)  # U[b] = b T[b]^T: [N, tokens], the V^T layout
    else:
        gemm_nt(t, b, out=u.view(-1)[col:], ldc=ldy)
    return scaled_add(y, u, scales, index, out=y)


# The update of a feed-forward's first projection with the GEGLU in the same launch (gmd_lora_geglu).  GMD_LORA_GEGLU_FUSED=0 (read
# once) composes lora_update and geglu_interleaved instead: the A/B switch, and the comparison route of the tests.
USE_LORA_GEGLU_FUSED = os.environ.get("GMD_LORA_GEGLU_FUSED", "1") != "0"
GEGLU_GROUP = 16  # rows of one value / gate group of an interleaved ff1 weight (UNet2DConditionModel._prepare_encoder)


def geglu_interleave(t):
    """Rows of ``t`` [2F, ...] from checkpoint order (value half, then gate half) to the order of the interleaved ff1 weight: value
    rows 0-15, gate rows 0-15, value rows 16-31, ...  F % 16 == 0."""
    half = t.shape[0] // 2
    if t.shape[0] != 2 * half or half % GEGLU_GROUP:
        raise HipExtensionError(f"geglu_interleave: {t.shape[0]} rows are not two halves of a multiple of {GEGLU_GROUP}")
    rest = t.shape[1:]
    return torch.stack([t[:half].reshape(half // GEGLU_GROUP, GEGLU_GROUP, *rest), t[half:].reshape(half // GEGLU_GROUP, GEGLU_GROUP, *rest)],
                       1).reshape(2 * half, *rest)


def geglu_interleaved(x):
    """``geglu`` over the interleaved column layout (``geglu_interleave`` of the projection's rows): [..., 2F] -> [..., F]."""
    _dev(x)
    if is_asplit(x):
        raise HipExtensionError("geglu_interleaved: the input is a pre-split activation (only contractions read that layout)")
    F2 = x.shape[-1]
    y = torch.empty(x.shape[:-1] + (F2 // 2,), dtype=x.dtype, device=x.device)
    check(lib().gmd_geglu_interleaved(_ptr(x), _ptr(y), dtype_code(x.dtype), x.numel() // F2, F2 // 2, _stream()), "gmd_geglu_interleaved")
    return y


def lora_geglu(x, a, b_interleaved, y, scales, index, fused=None, x_split=False):
    """``geglu(y + scales[index] * (x @ a.T) @ b.T)`` behind the first feed-forward GEMM of an adapted block; returns F [M, 4C].
    x: [M, C]; a: [Rp, C]; ``b_interleaved``: [8C, Rp] with its rows in the order of the interleaved ff1 weight (``geglu_interleave``);
    y: [M, 8C], the pre-activation in that column layout (bias included).  16-bit types: ONE launch (gmd_lora_geglu) that reads y once and
    leaves it unchanged, unless ``fused`` is False (default: USE_LORA_GEGLU_FUSED).  Composed (and float32): ``lora_update`` IN PLACE
    on y (its own one launch in the 16-bit types), then ``geglu_interleaved``: a read-modify-write of y and one more read of it."""
    _dev(x, a, b_interleaved, y, scales)
    index = _ip_scale_arg(scales, index, "lora_geglu")
    if not (x.dtype == a.dtype == b_interleaved.dtype == y.dtype):
        raise HipExtensionError(f"lora_geglu: dtype mismatch {x.dtype} / {a.dtype} / {b_interleaved.dtype} / {y.dtype}")
    if x.dim() != 2 or a.dim() != 2 or b_interleaved.dim() != 2 or y.dim() != 2:
        raise HipExtensionError("lora_geglu: x, a, b and y must be matrices")
    M, C = x.shape
    Rp = a.shape[0]
    if a.shape[1] != C or tuple(b_interleaved.shape) != (8 * C, Rp) or tuple(y.shape) != (M, 8 * C):
        raise HipExtensionError(f"lora_geglu: operand shapes inconsistent: x {tuple(x.shape)}, a {tuple(a.shape)}, b {tuple(b_interleaved.shape)}, "
                                f"y {tuple(y.shape)} (b must be [8C, Rp], y [M, 8C])")
    if is_asplit(y) or not (x.is_contiguous() and y.is_contiguous()):
        raise HipExtensionError("lora_geglu: x and y must be contiguous, y no pre-split activation")
    fused = USE_LORA_GEGLU_FUSED if fused is None else bool(fused)
    if not (is_half(x.dtype) and fused):
        return geglu_interleaved(lora_update(x, a, b_interleaved, y, scales, index, x_split=x_split))
    if Rp > LORA_MAX_RANK:
        raise HipExtensionError(f"lora_geglu: padded rank {Rp} above {LORA_MAX_RANK}")
    f = torch.empty((M, 4 * C), dtype=x.dtype, device=x.device)
    tm, t0 = _timed("lora_geglu")
    check(lib().gmd_lora_geglu(_ptr(x), _ptr(a), _ptr(b_interleaved), _ptr(y), _ptr(f), dtype_code(x.dtype), M, C, Rp, C, 8 * C, 4 * C,
                               _ptr(scales), index, _stream()), "gmd_lora_geglu")
    if tm:
        tm.end("lora_geglu", 2.0 * M * Rp * 9 * C, (M * 13 * C + Rp * 9 * C) * x.element_size(), t0)
    return f


# SEVERAL adapters on one projection: their factors stacked along the rank and ONE launch with a per-column scale
# (gmd_lora_update_stacked / gmd_lora_geglu_stacked).  GMD_LORA_STACK_FUSED=0 (read once) sends a stacked projection down the
# comparison route instead -- one lora_update per adapter, in load order, each with its own scalar scale -- what float32 always runs
# (there is no float32 stacked kernel): the A/B switch, and the yardstick of tools/bench_lora_multi.py.
USE_LORA_STACK_FUSED = os.environ.get("GMD_LORA_STACK_FUSED", "1") != "0"
LORA_MAX_STACKED_RANK = 256  # the stacked kernel's limit on the padded SUM of the ranks (components/lora.py refuses more at load)


def _lora_stack_route(name, x, a, b, colscales, fused, parts):
    """True: the one stacked launch; False: the sequential route over ``parts``.  A missing operand of the chosen route is an error."""
    fused = (USE_LORA_STACK_FUSED if fused is None else bool(fused)) and is_half(x.dtype)
    if fused:
        if a is None or b is None or colscales is None:
            raise HipExtensionError(f"{name}: the stacked launch needs the stacked factors a, b and the table of column scales")
        if colscales.dtype != torch.float32 or colscales.dim() != 2 or not colscales.is_contiguous():
            raise HipExtensionError(f"{name}: colscales must be a contiguous float32 [rows, ldc] device tensor")
        if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[1] or a.shape[1] != x.shape[1]:
            raise HipExtensionError(f"{name}: operand shapes inconsistent: x {tuple(x.shape)}, a {tuple(a.shape)}, b {tuple(b.shape)}")
        if a.shape[0] > LORA_MAX_STACKED_RANK:
            raise HipExtensionError(f"{name}: padded stacked rank {a.shape[0]} above {LORA_MAX_STACKED_RANK}")
        if colscales.shape[1] < a.shape[0]:
            raise HipExtensionError(f"{name}: colscales rows of {colscales.shape[1]} columns are shorter than the padded rank {a.shape[0]}")
    elif not parts:
        raise HipExtensionError(f"{name}: the sequential route (float32, GMD_LORA_STACK_FUSED=0, fused=False) needs parts=[(a, b, scales, "
                                "index), ...], the adapters one by one")
    return fused


def lora_update_stacked(x, a, b, y, colscales, index, transposed=False, tokens=None, fused=None, col=0, x_split=False, parts=None):
    """``y += ((x @ a.T) * colscales[index, :Rp]) @ b.T`` in place, the column scale applied in float32 in front of the ONE rounding of
    the intermediate; returns ``y``.  a: [Rp, K] and b: [N, Rp] hold several adapters' factors side by side along the rank, the SUM of
    the ranks zero-padded to a multiple of 32, Rp <= ``LORA_MAX_STACKED_RANK``; ``colscales``: float32 device table [rows, ldc >= Rp]
    read by the kernel, so one captured graph serves every weight setting.  x, y, ``transposed`` / ``tokens`` / ``col`` / ``x_split``
    as ``lora_update``.  16-bit types: ONE launch (gmd_lora_update_stacked) that reads and writes y once.  ``parts``: the same adapters
    one by one, ``[(a_i, b_i, scales, index_i), ...]`` in load order (each as ``lora_update`` takes them) -- the sequential route, one
    ``lora_update`` each: what float32 always takes and what ``fused=False`` (default: USE_LORA_STACK_FUSED) selects; it rounds y
    between the adapters, so the two routes agree within their bounds, not bit for bit."""
    if not _lora_stack_route("lora_update_stacked", x, a, b, colscales, fused, parts):
        for pa, pb, ps, pi in parts:
            lora_update(x, pa, pb, y, ps, pi, transposed=transposed, tokens=tokens, col=col, x_split=x_split)
        return y
    _dev(x, a, b, y, colscales)
    if not isinstance(index, int) or isinstance(index, bool) or not 0 <= index < colscales.shape[0]:
        raise HipExtensionError(f"lora_update_stacked: row index {index!r} outside the table of {colscales.shape[0]} rows")
    if not (x.dtype == a.dtype == b.dtype == y.dtype):
        raise HipExtensionError(f"lora_update_stacked: dtype mismatch {x.dtype} / {a.dtype} / {b.dtype} / {y.dtype}")
    M, K = x.shape
    N, Rp = b.shape
    if transposed:
        if y.dim() != 3 or tokens is None or tokens <= 0 or y.shape[0] * tokens != M or y.shape[1] != N or y.shape[2] < tokens or col:
            raise HipExtensionError(f"lora_update_stacked: transposed y {tuple(y.shape)} does not hold [M / tokens, N, >= tokens] for M={M}, "
                                    f"N={N}, tokens={tokens}")
        batch, ldy = y.shape[0], y.shape[2]
    else:
        if y.dim() != 2 or y.shape[0] != M or col < 0 or col + N > y.shape[1]:
            raise HipExtensionError(f"lora_update_stacked: y {tuple(y.shape)} does not hold columns [{col}, {col + N}) of {M} rows")
        batch, tokens, ldy = 1, M, y.shape[1]
    tm, t0 = _timed("lora_update")
    check(lib().gmd_lora_update_stacked(_ptr(x), _ptr(a), _ptr(b), y.data_ptr() + col * y.element_size(), dtype_code(x.dtype), M, K, Rp, N, K,
                                        ldy, int(bool(transposed)), batch, tokens, N * ldy, _ptr(colscales), index, colscales.shape[1],
                                        _stream()), "gmd_lora_update_stacked")
    if tm:
        tm.end("lora_update", 2.0 * M * Rp * (K + N), (M * K + 2 * M * N + Rp * (K + N)) * x.element_size(), t0)
    return y


def lora_geglu_stacked(x, a, b_interleaved, y, colscales, index, fused=None, x_split=False, parts=None):
    """``lora_geglu`` for several adapters stacked along the rank (operands as ``lora_update_stacked``; ``b_interleaved`` [8C, Rp] with
    its rows in the order of the interleaved ff1 weight): returns F [M, 4C].  16-bit types: ONE launch (gmd_lora_geglu_stacked), y read
    once and left unchanged.  Sequential route (``parts``; float32, ``fused=False``): one ``lora_update`` per adapter IN PLACE on y, then
    ``geglu_interleaved``."""
    if not _lora_stack_route("lora_geglu_stacked", x, a, b_interleaved, colscales, fused, parts):
        for pa, pb, ps, pi in parts:
            lora_update(x, pa, pb, y, ps, pi, x_split=x_split)
        return geglu_interleaved(y)
    _dev(x, a, b_interleaved, y, colscales)
    if not isinstance(index, int) or isinstance(index, bool) or not 0 <= index < colscales.shape[0]:
        raise HipExtensionError(f"lora_geglu_stacked: row index {index!r} outside the table of {colscales.shape[0]} rows")
    if not (x.dtype == a.dtype == b_interleaved.dtype == y.dtype):
        raise HipExtensionError(f"lora_geglu_stacked: dtype mismatch {x.dtype} / {a.dtype} / {b_interleaved.dtype} / {y.dtype}")
    M, C = x.shape
    Rp = a.shape[0]
    if y.dim() != 2 or tuple(b_interleaved.shape) != (8 * C, Rp) or tuple(y.shape) != (M, 8 * C):
        raise HipExtensionError(f"lora_geglu_stacked: operand shapes inconsistent: x {tuple(x.shape)}, a {tuple(a.shape)}, b "
                                f"{tuple(b_interleaved.shape)}, y {tuple(y.shape)} (b must be [8C, Rp], y [M, 8C])")
    if is_asplit(y) or not (x.is_contiguous() and y.is_contiguous()):
        raise HipExtensionError("lora_geglu_stacked: x and y must be contiguous, y no pre-split activation")
    f = torch.empty((M, 4 * C), dtype=x.dtype, device=x.device)
    tm, t0 = _timed("lora_geglu")
    check(lib().gmd_lora_geglu_stacked(_ptr(x), _ptr(a), _ptr(b_interleaved), _ptr(y), _ptr(f), dtype_code(x.dtype), M, C, Rp, C, 8 * C, 4 * C,
                                       _ptr(colscales), index, colscales.shape[1], _stream()), "gmd_lora_geglu_stacked")
    if tm:
        tm.end("lora_geglu", 2.0 * M * Rp * 9 * C, (M * 13 * C + Rp * 9 * C) * x.element_size(), t0)
    return f


def softmax_rows(s, cols, scale, out_dtype, ldp=None, causal_nq=0):
    _dev(s)
    _f32(s, "softmax_rows input")
    lds_ = s.shape[-1]
    rows = s.numel() // lds_
    ldp = ldp or lds_
    p = torch.empty(s.shape[:-1] + (ldp,), dtype=out_dtype, device=s.device)
    check(lib().gmd_softmax_rows(_ptr(s), lds_, _ptr(p), dtype_code(out_dtype), ldp, rows, cols, float(scale), int(causal_nq), _stream()),
          "gmd_softmax_rows")
    return p


# ----------------------------------------------------------------------------------------------
# normalisation / elementwise
# ----------------------------------------------------------------------------------------------
def groupnorm_scale_shift(x, B, groups, gamma, beta, eps):
    """x: [B, HW, C] -> float32 [B, C, 2] = {rstd*gamma, beta - mean*rstd*gamma}."""
    _dev(x, gamma, beta)
    C = x.shape[-1]
    HW = x.numel() // (B * C)
    nsplit = lib().gmd_groupnorm_nsplit(HW)
    ws = torch.empty(B * nsplit * groups * 2, dtype=torch.float32, device=x.device)
    ss = torch.empty((B, C, 2), dtype=torch.float32, device=x.device)
    check(lib().gmd_groupnorm_stats(_ptr(x), dtype_code(x.dtype), B, HW, C, groups, float(eps), _ptr(_f32(gamma, "gamma")),
                                    _ptr(_f32(beta, "beta")), _ptr(ws), _ptr(ss), _stream()), "gmd_groupnorm_stats")
    return ss


def groupnorm_apply(x, B, ss, silu):
    _dev(x, ss)
    C = x.shape[-1]
    HW = x.numel() // (B * C)
    y = torch.empty_like(x)
    check(lib().gmd_groupnorm_apply(_ptr(x), _ptr(y), dtype_code(x.dtype), B, HW, C, _ptr(ss), int(silu), _stream()),
          "gmd_groupnorm_apply")
    return y


# bytes of one (sample, group) slab up to which the single-launch kernel wins (tools/bench_gn.py, MI355X): 5-21 us against
# 14-27 us for the three-launch path on the 16x16 / 8x8 UNet levels.  The kernel walks one group's channels of every pixel,
# so it needs long enough channel rows: with 16-byte accesses (C/G a multiple of 8 bf16) it wins up to 40 KiB, with 8- or
# 4-byte accesses only up to 24 KiB; beyond that the strided re-reads lose to the row-contiguous split kernels.
GN_FUSED_MAX_SLAB = 24 * 1024
GN_FUSED_MAX_SLAB_VEC16 = 40 * 1024


def _usable_colstats(x, B, HW, C, cpg):
    """Producer statistics attached to ``x`` (one producer, or the two halves of a channel concatenation) when they cover
    exactly this tensor: ((stats_a, Ca), (stats_b, Cb) | None), else None."""
    st = getattr(x, "_colstats", None)
    if st is None or HW % 64 or cpg % COLSTATS_BUCKET:
        return None
    parts = st if isinstance(st, list) else [st]
    rows = B * HW // 64
    if sum(c for _, c in parts) != C or any(t.shape[0] != rows or t.shape[1] * COLSTATS_BUCKET != c for t, c in parts):
        return None
    return (parts[0], parts[1] if len(parts) == 2 else None) if len(parts) <= 2 else None


def groupnorm(x, B, groups, gamma, beta, eps, silu=False, split_out=False):
    """GroupNorm(+SiLU).  A tensor that still carries its producer's column statistics (``colstats=True`` of gemm_nt /
    conv3x3, possibly through concat_channels) is normalised in one pass over it; otherwise small group slabs (16x16 / 8x8
    UNet levels) take the single-launch fused kernel and larger ones the split-statistics path (partial + apply)."""
    _dev(x, gamma, beta)
    C = x.shape[-1]
    HW = x.numel() // (B * C)
    epw = 2 if is_half(x.dtype) else 1
    cpg = C // groups
    vec16 = (cpg * x.element_size()) % 16 == 0 and (C * x.element_size()) % 16 == 0
    # algorithmic HBM bytes of a GroupNorm: the activation is read once and written once (the statistics pass of the split
    # path re-reads it: that second read is what the roofline fraction of this kind exposes)
    nbytes = 2 * x.numel() * x.element_size()
    if is_asplit(x):
        raise HipExtensionError("groupnorm: the input is a pre-split activation (only contractions read that layout)")
    # ``split_out``: store the float32 result pre-split for the contraction that reads it (the two large-slab paths; the single-launch
    # kernel of the small levels keeps the plain layout) -- the result then carries the mark (is_asplit)
    so = bool(split_out) and want_split_out(x.dtype, C)
    st = _usable_colstats(x, B, HW, C, cpg)
    if st is not None:
        global colstats_uses
        colstats_uses += 1
        (sa, ca), sb = st
        y = torch.empty_like(x)
        tm, t0 = _timed("groupnorm")
        check(lib().gmd_groupnorm_colstats(_ptr(x), _ptr(y), GMD_F32SA if so else dtype_code(x.dtype), B, HW, C, groups, float(eps),
                                           _ptr(_f32(gamma, "gamma")), _ptr(_f32(beta, "beta")), _ptr(sa), ca,
                                           _ptr(sb[0]) if sb is not None else None, COLSTATS_BUCKET, int(silu), _stream()),
              "gmd_groupnorm_colstats")
        if tm:
            tm.end("groupnorm", 0.0, nbytes, t0)
        return _mark_asplit(y) if so else y
    if cpg % epw == 0 and HW * cpg * x.element_size() <= (GN_FUSED_MAX_SLAB_VEC16 if vec16 else GN_FUSED_MAX_SLAB):
        y = torch.empty_like(x)
        tm, t0 = _timed("groupnorm")
        check(lib().gmd_groupnorm_fused(_ptr(x), _ptr(y), dtype_code(x.dtype), B, HW, C, groups, float(eps), _ptr(_f32(gamma, "gamma")),
                                        _ptr(_f32(beta, "beta")), int(silu), _stream()), "gmd_groupnorm_fused")
        if tm:
            tm.end("groupnorm", 0.0, nbytes, t0)
        return y
    nsplit = lib().gmd_groupnorm_nsplit(HW)
    ws = torch.empty(B * nsplit * groups * 2, dtype=torch.float32, device=x.device)
    y = torch.empty_like(x)
    tm, t0 = _timed("groupnorm")
    check(lib().gmd_groupnorm_split(_ptr(x), _ptr(y), GMD_F32SA if so else dtype_code(x.dtype), B, HW, C, groups, float(eps), _ptr(_f32(gamma, "gamma")),
                                    _ptr(_f32(beta, "beta")), _ptr(ws), int(silu), _stream()), "gmd_groupnorm_split")
    if tm:
        tm.end("groupnorm", 0.0, nbytes, t0)
    return _mark_asplit(y) if so else y


def groupnorm_split(x, B, groups, gamma, beta, eps, silu=False):
    return groupnorm_apply(x, B, groupnorm_scale_shift(x, B, groups, gamma, beta, eps), silu)


def layernorm(x, gamma, beta, eps=1e-5, split_out=False):
    """``split_out``: store the float32 result pre-split for the projections that read it (the result carries the mark, is_asplit)."""
    _dev(x, gamma, beta)
    if is_asplit(x):
        raise HipExtensionError("layernorm: the input is a pre-split activation (only contractions read that layout)")
    C = x.shape[-1]
    so = bool(split_out) and want_split_out(x.dtype, C)
    y = torch.empty_like(x)
    tm, t0 = _timed("layernorm")
    check(lib().gmd_layernorm(_ptr(x), _ptr(y), GMD_F32SA if so else dtype_code(x.dtype), x.numel() // C, C, _ptr(_f32(gamma, "gamma")),
                              _ptr(_f32(beta, "beta")), float(eps), _stream()), "gmd_layernorm")
    if tm:
        tm.end("layernorm", 0.0, 2 * x.numel() * x.element_size(), t0)
    return _mark_asplit(y) if so else y


def geglu(x):
    _dev(x)
    F2 = x.shape[-1]
    y = torch.empty(x.shape[:-1] + (F2 // 2,), dtype=x.dtype, device=x.device)
    check(lib().gmd_geglu(_ptr(x), _ptr(y), dtype_code(x.dtype), x.numel() // F2, F2 // 2, _stream()), "gmd_geglu")
    return y


def timestep_embedding(t_dev, B, dim, dtype, flip_sin_to_cos=True, freq_shift=0.0):
    """t_dev: float32 device scalar (shape [1])."""
    _dev(t_dev)
    _f32(t_dev, "timestep")
    out = torch.empty((B, dim), dtype=dtype, device=t_dev.device)
    check(lib().gmd_timestep_embedding(_ptr(t_dev), _ptr(out), dtype_code(dtype), B, dim, int(flip_sin_to_cos),
                                       float(freq_shift), _stream()), "gmd_timestep_embedding")
    return out


def timestep_embedding_add(t_dev, addend, B, dim, dtype, flip_sin_to_cos=True, freq_shift=0.0):
    """``timestep_embedding`` plus a per-row addend [B, dim] of ``dtype``, each rounded as diffusers rounds it: the sinusoid to
    ``dtype``, then the sum to ``dtype`` (``t_emb.to(dtype) + cond_proj(timestep_cond)``).  One launch, like the plain embedding."""
    _dev(t_dev, addend)
    _f32(t_dev, "timestep")
    if addend.dtype != dtype or tuple(addend.shape) != (B, dim) or not addend.is_contiguous():
        raise HipExtensionError(f"timestep_embedding_add: the addend must be a contiguous [{B}, {dim}] tensor of {dtype} "
                                f"(got {tuple(addend.shape)} of {addend.dtype})")
    out = torch.empty((B, dim), dtype=dtype, device=t_dev.device)
    check(lib().gmd_timestep_embedding_add(_ptr(t_dev), _ptr(addend), _ptr(out), dtype_code(dtype), B, dim, int(flip_sin_to_cos),
                                           float(freq_shift), _stream()), "gmd_timestep_embedding_add")
    return out


def concat_channels(a, b):
    _dev(a, b)
    ca, cb = a.shape[-1], b.shape[-1]
    rows = a.numel() // ca
    if b.numel() // cb != rows or a.dtype != b.dtype:
        raise HipExtensionError("concat_channels: row count / dtype mismatch")
    out = torch.empty(a.shape[:-1] + (ca + cb,), dtype=a.dtype, device=a.device)
    tm, t0 = _timed("concat")
    check(lib().gmd_concat_channels(_ptr(a), ca, _ptr(b), cb, _ptr(out), dtype_code(a.dtype), rows, _stream()),
          "gmd_concat_channels")
    if tm:
        tm.end("concat", 0.0, 2 * out.numel() * out.element_size(), t0)
    sa, sb = getattr(a, "_colstats", None), getattr(b, "_colstats", None)
    if sa is not None and sb is not None and not isinstance(sa, list) and not isinstance(sb, list):
        out._colstats = [sa, sb]  # a following GroupNorm reads the two producers' statistics side by side
    return out


# ControlNet residuals are added where the up blocks read their skips anyway (gmd_concat_channels_add).  The skip producer's column
# statistics are WRONG for the sum, so they are never forwarded: the result carries none and the following GroupNorm takes its general
# route.  The launch CAN leave fresh statistics of the stored B part (the GroupNorm then stays one-pass), but as measured that does not
# pay: the statistics pass costs 13-42 us per concat on the 64x64 / 32x32 levels and saves 8-12 us in the GroupNorm, +0.5 ... +0.9 % on the
# whole ControlNet step (profiles/controlnet.txt).  So it is OFF by default; GMD_CONCAT_STATS=1 switches it on (A/B measurements, tests).
CONTROL_RESIDUALS = 13  # an SD-1.5 ControlNet: twelve down-block residuals and the mid-block residual
USE_CONCAT_STATS = os.environ.get("GMD_CONCAT_STATS", "0") == "1"
CONCAT_STATS_MAX_CB = 4096  # the statistics pass keeps 16 bytes of LDS per B-part channel


def concat_channels_add(a, b, ra=None, rb=None, ia=0, ib=0, scales=None, r_row0=0, hw=None):
    """``cat([a + ra * scales[ia], b + rb * scales[ib]], -1)`` over channels-last rows, each sum rounded as torch rounds
    ``s + r * scale`` (gmd_concat_channels_add).  ``ra`` / ``rb``: residuals of the rows from ``r_row0`` on, or None (that part is a
    copy); ``scales``: float32 device tensor of CONTROL_RESIDUALS entries, read by the kernel.  ``hw``: rows per sample -- given, and with
    USE_CONCAT_STATS on, the launch leaves fresh column statistics of the B part for the following GroupNorm (``out._colstats``).  A
    part that a residual modified never passes its producer's statistics on."""
    _dev(a, b, ra, rb, scales)
    ca, cb = a.shape[-1], b.shape[-1]
    rows = a.numel() // ca
    if b.numel() // cb != rows or a.dtype != b.dtype:
        raise HipExtensionError("concat_channels_add: row count / dtype mismatch")
    r_row0 = int(r_row0)
    if not 0 <= r_row0 <= rows:
        raise HipExtensionError(f"concat_channels_add: r_row0={r_row0} outside [0, {rows}]")
    for r, c, i, nm in ((ra, ca, ia, "ra"), (rb, cb, ib, "rb")):
        if r is None:
            continue
        if r.dtype != a.dtype or r.shape[-1] != c or r.numel() != (rows - r_row0) * c:
            raise HipExtensionError(f"concat_channels_add: {nm} must hold {rows - r_row0} rows of {c} channels of {a.dtype} "
                                    f"(got {tuple(r.shape)} of {r.dtype})")
        if not 0 <= int(i) < CONTROL_RESIDUALS:
            raise HipExtensionError(f"concat_channels_add: scale index {i} outside [0, {CONTROL_RESIDUALS})")
    if ra is not None or rb is not None:
        if scales is None or scales.dtype != torch.float32 or scales.numel() != CONTROL_RESIDUALS:
            raise HipExtensionError(f"concat_channels_add: scales must be a float32 device tensor of {CONTROL_RESIDUALS} entries")
    out = torch.empty(a.shape[:-1] + (ca + cb,), dtype=a.dtype, device=a.device)
    sa = None if ra is not None else getattr(a, "_colstats", None)
    sb = None if rb is not None else getattr(b, "_colstats", None)
    if isinstance(sa, list):
        sa = None
    if isinstance(sb, list):
        sb = None
    st = None
    if (rb is not None and sa is not None and USE_CONCAT_STATS and USE_COLSTATS and hw and hw % 64 == 0 and rows % hw == 0
            and cb % COLSTATS_BUCKET == 0 and cb <= CONCAT_STATS_MAX_CB):
        st = torch.empty((rows // 64, cb // COLSTATS_BUCKET, 2), dtype=torch.float32, device=a.device)
        sb = (st, cb)
    tm, t0 = _timed("concat")
    check(lib().gmd_concat_channels_add(_ptr(a), ca, _ptr(ra), int(ia), _ptr(b), cb, _ptr(rb), int(ib), _ptr(scales), r_row0, _ptr(out),
                                        dtype_code(a.dtype), rows, _ptr(st), COLSTATS_BUCKET if st is not None else 0, _stream()),
          "gmd_concat_channels_add")
    if tm:
        extra = sum(r.numel() for r in (ra, rb) if r is not None)
        tm.end("concat", 0.0, (2 * out.numel() + extra) * out.element_size(), t0)
    if sa is not None and sb is not None:
        out._colstats = [sa, sb]  # both parts' statistics describe what was stored: side by side, as concat_channels leaves them
    return out


# FreeU (diffusers' enable_freeu): the skip concat of one FreeU site as ONE launch (gmd_concat_channels_freeu).  The first half of the
# backbone channels is scaled by params[ib]; the skip goes through diffusers' fourier_filter at threshold 1 -- X + (params[is] - 1) * low,
# low = the inverse transform of the bins {0, -1} x {0, -1}, a seven-coefficient reduction per (sample, channel), no FFT.
FREEU_PARAMS = 4  # the device table of UNet2DConditionModel.enable_freeu: [s1, s2, b1, b2]


def _freeu_rows(t, rows, name):
    """Row stride (elements) of ``t`` seen as [rows, C] channels-last: contiguous, or a column range of a wider contiguous buffer."""
    c = t.shape[-1]
    try:
        v = t.view(rows, c)
    except RuntimeError:
        v = None
    if v is None or (c > 1 and v.stride(1) != 1):
        raise HipExtensionError(f"concat_channels_freeu: {name} must hold {rows} channels-last rows with one row stride "
                                f"(got {tuple(t.shape)}, strides {t.stride()})")
    return v.stride(0) if rows > 1 else c


def concat_channels_freeu(a, s, B, H, W, params, ib, is_, out=None):
    """``cat([a[..., :Ca/2] * params[ib], a[..., Ca/2:], fourier_filter(s, threshold=1, scale=params[is_])], -1)`` over the channels-last
    rows of ``B`` samples of ``H x W`` pixels, one launch (gmd_concat_channels_freeu); float32 inside, one rounding per element.
    ``params``: float32 device tensor read by the kernel, so a captured graph serves every setting.  ``out``: None (a new tensor), or
    the result buffer -- which may be the very buffer ``a`` and ``s`` are the column views ``[..., :Ca]`` / ``[..., Ca:]`` of (in place,
    behind ``concat_channels_add``).  The result carries no ``_colstats``: the producers' statistics describe neither part any more, so
    the following GroupNorm takes its general route."""
    for t in (a, s, params, out):
        if t is not None and not t.is_cuda:
            raise HipExtensionError(
                "gm_diffusion (MI355X build): tensor is on %s; the compute path is hand-written HIP and has no CPU fallback" % t.device)
    if is_asplit(a) or is_asplit(s):
        raise HipExtensionError("concat_channels_freeu: an input is a pre-split activation (only contractions read that layout)")
    B, H, W = int(B), int(H), int(W)
    if B < 0 or H < 1 or W < 1:
        raise HipExtensionError(f"concat_channels_freeu: bad sizes B={B}, H={H}, W={W}")
    if a.dtype != s.dtype:
        raise HipExtensionError(f"concat_channels_freeu: dtype mismatch {a.dtype} / {s.dtype}")
    rows = B * H * W
    ca, cs = a.shape[-1], s.shape[-1]
    lda, lds = _freeu_rows(a, rows, "a"), _freeu_rows(s, rows, "s")
    if params is None or params.dtype != torch.float32 or not params.is_contiguous():
        raise HipExtensionError("concat_channels_freeu: params must be a contiguous float32 device tensor")
    for i, nm in ((ib, "ib"), (is_, "is_")):
        if not 0 <= int(i) < params.numel():
            raise HipExtensionError(f"concat_channels_freeu: {nm}={i} outside [0, {params.numel()})")
    if out is None:
        out = torch.empty(a.shape[:-1] + (ca + cs,), dtype=a.dtype, device=a.device)
    elif out.dtype != a.dtype or out.shape[-1] < ca + cs or out.shape[:-1] != a.shape[:-1]:
        raise HipExtensionError(f"concat_channels_freeu: out {tuple(out.shape)} of {out.dtype} does not hold {tuple(a.shape[:-1])} rows of "
                                f"{ca + cs} channels of {a.dtype}")
    ldo = _freeu_rows(out, rows, "out")
    if rows == 1:  # a single row has no stride: the in-place form is then recognised by its pointers alone
        lda = lds = ldo
    tm, t0 = _timed("concat_freeu")
    check(lib().gmd_concat_channels_freeu(_ptr(a), ca, lda, _ptr(s), cs, lds, _ptr(out), ldo, dtype_code(a.dtype), B, H, W, _ptr(params),
                                          int(ib), int(is_), _stream()), "gmd_concat_channels_freeu")
    if tm:  # the skip is read twice (coefficients, then the correction)
        tm.end("concat_freeu", 16.0 * rows * cs, (2 * rows * (ca + cs) + rows * cs) * out.element_size(), t0)
    if getattr(out, "_colstats", None) is not None:
        del out._colstats
    return out


def silu_(x):
    """``x * sigmoid(x)`` in place (gmd_silu: the formula of the GroupNorm + SiLU kernels); returns ``x``."""
    _dev(x)
    if is_asplit(x):
        raise HipExtensionError("silu_: the input is a pre-split activation (only contractions read that layout)")
    check(lib().gmd_silu(_ptr(x), dtype_code(x.dtype), x.numel(), _stream()), "gmd_silu")
    if getattr(x, "_colstats", None) is not None:  # the statistics described the values before the activation
        del x._colstats
    return x


_SIDE_STREAMS = {}


def side_stream(device):
    """The second HIP stream of ``device`` (the GM UNet's, stable_diffusion_dual_unet.py).  ONE per device and process, shared by
    every pipeline object: HIP multiplexes its streams onto a few hardware queues in the order they are first used, and a stream
    drawn from torch's pool after a number of others (graph captures take several) can land on the queue the main stream uses --
    the two UNets then run one after the other.  Measured in bench.py: a second pipeline with its own late stream 2036 ms per batch,
    with this shared one 1817 ms (float32 path).  Default priority and HIP's default queue count on purpose: a high-priority GM
    stream costs 1393 instead of 851 ms per batch, GPU_MAX_HW_QUEUES=8 1158 ms, =2 852 ms (tools/ab_queues.sh, bfloat16)."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    s = _SIDE_STREAMS.get(key)
    if s is None:
        s = _SIDE_STREAMS[key] = _stream_beside_current(device)
    return s


_SPIN_TICKS = 1_000_000  # ~0.4 ms of torch.cuda._sleep at the MI355X shader clock
_CAPTURES_IN_FLIGHT = 0  # HIP-graph captures this package has open (components: graphed_forward) -- on ANY stream or thread
_CAPTURES_LOCK = threading.Lock()  # the count is deliberately process-wide (a capture on another thread matters too): guarded
_PROBE_WARNED = False


class capture_in_flight:
    """Marks a HIP-graph capture of this package as open: the side-stream probe synchronises, which would invalidate a capture
    in progress on another stream, so it does not run while one is open."""

    def __enter__(self):
        global _CAPTURES_IN_FLIGHT
        with _CAPTURES_LOCK:
            _CAPTURES_IN_FLIGHT += 1

    def __exit__(self, *exc):
        global _CAPTURES_IN_FLIGHT
        with _CAPTURES_LOCK:
            _CAPTURES_IN_FLIGHT -= 1
        return False


def _probe_note(msg):
    global _PROBE_WARNED
    if not _PROBE_WARNED:
        _PROBE_WARNED = True
        import warnings

        warnings.warn("gm_diffusion: " + msg + " -- the GM UNet's stream may share the hardware queue of the main stream (the two "
                      "UNets then run one after the other, ~20 % slower; results are unaffected).  GMD_SIDE_STREAM_SKIP=<n> picks "
                      "the (n+1)-th new stream without probing.", RuntimeWarning, stacklevel=3)


def _stream_beside_current(device, candidates=8):
    """A new stream that really runs BESIDE the current one.  Of the streams a process creates, about every fourth lands on the
    hardware queue of the null stream (tools/stream_queue_probe.py: pool streams 6, 10, 14, ... of a fresh process), so the
    first candidate is not taken on trust: one single-thread spinning kernel on each of the two streams must take the time of one
    spin, not of two.  ~3 ms, once per device and process.  The probe is wall-clock based, so it is an optimisation with escape
    hatches, never a reason to fail: it does not run while a graph capture is open (its synchronisation would invalidate the
    capture) or when GMD_SIDE_STREAM_SKIP=<n> names the stream to take (the (n+1)-th created here; a host that knows its queue
    layout, or a shared / busy GPU where timing is noise); when no candidate passes -- or the probe cannot run -- the first
    candidate is used and ONE RuntimeWarning says so."""
    skip = os.environ.get("GMD_SIDE_STREAM_SKIP")
    if skip is not None:
        try:
            n = max(0, int(skip))
        except ValueError:  # a malformed escape hatch is no reason to fail either: say so once and probe as usual
            _probe_note(f"GMD_SIDE_STREAM_SKIP={skip!r} is not an integer; ignored")
            n = None
        if n is not None:
            junk = [torch.cuda.Stream(device=device) for _ in range(n)]
            st = torch.cuda.Stream(device=device)
            del junk
            return st
    first = torch.cuda.Stream(device=device)
    try:
        with torch.cuda.device(device):
            if _CAPTURES_IN_FLIGHT > 0 or torch.cuda.is_current_stream_capturing():
                _probe_note("side-stream probe skipped (a HIP-graph capture is in progress)")
                return first
            cur = torch.cuda.current_stream()

            def wall(fn, st):
                cur.synchronize(); st.synchronize()  # the two streams of the probe only: no device-wide synchronisation
                t0 = time.perf_counter()
                fn()
                cur.synchronize(); st.synchronize()
                return time.perf_counter() - t0

            def both(st):
                with torch.cuda.stream(st):
                    torch.cuda._sleep(_SPIN_TICKS)
                torch.cuda._sleep(_SPIN_TICKS)

            torch.cuda._sleep(_SPIN_TICKS)
            one = min(wall(lambda: torch.cuda._sleep(_SPIN_TICKS), first) for _ in range(2))
            st = first
            for _ in range(candidates):
                both(st)
                if min(wall(lambda: both(st), st) for _ in range(2)) < 1.5 * one:
                    return st
                st = torch.cuda.Stream(device=device)
            _probe_note(f"none of {candidates} candidate streams ran beside the current stream in the probe (busy or shared GPU?)")
    except Exception as e:  # pragma: no cover -- the probe is an optimisation, never a reason to fail
        _probe_note(f"side-stream probe failed ({e!r})")
    return first


def dup_batch(t):
    """[B, ...] -> [2B, ...] with both halves equal to ``t`` (one read, two writes; the CFG duplication of a shared-prefix tensor)."""
    _dev(t)
    out = torch.empty((2 * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    nbytes = t.numel() * t.element_size()
    if nbytes % 16 or os.environ.get("GMD_DUP_KERNEL", "1") == "0":  # (the switch: A/B measurements only)
        out[: t.shape[0]].copy_(t)
        out[t.shape[0]:].copy_(t)
        return out
    check(lib().gmd_dup_batch(_ptr(t), _ptr(out), nbytes, _stream()), "gmd_dup_batch")
    return out


def embedding_lookup(ids, table, pos):
    """ids: integer [B, T] on the device; table [vocab, C], pos [>=T, C] -> [B, T, C] = table[ids] + pos[:T]."""
    _dev(ids, table, pos)
    if table.dtype != pos.dtype or table.shape[1] != pos.shape[1] or pos.shape[0] < ids.shape[1]:
        raise HipExtensionError("embedding_lookup: table / position shapes or dtypes inconsistent")
    B, T = ids.shape
    ids32 = ids.to(torch.int32).contiguous()
    out = torch.empty((B, T, table.shape[1]), dtype=table.dtype, device=table.device)
    check(lib().gmd_embedding_lookup(_ptr(ids32), _ptr(table), _ptr(pos), _ptr(out), dtype_code(table.dtype), B * T, T, table.shape[1],
                                     table.shape[0], _stream()), "gmd_embedding_lookup")
    return out


def cast(x, dtype):
    _dev(x)
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    check(lib().gmd_cast(_ptr(x), dtype_code(x.dtype), _ptr(out), dtype_code(dtype), x.numel(), _stream()), "gmd_cast")
    return out


# ----------------------------------------------------------------------------------------------
# latent-side
# ----------------------------------------------------------------------------------------------
def pack_unet_input(src0, src1, dup, cp, dtype, out=None, div=None):
    """src0 [B,C0,h,w] (+ src1 [B,C1,h,w]) float32 NCHW -> [dup*B, h*w, cp] channels-last of `dtype`
    (written into `out` when given: the static input buffer of a captured graph).  ``div`` = (d0, d1): each source is divided by
    its own float32 divisor before the cast (gmd_pack_unet_input_scaled: a sigma-space scheduler's scale_model_input); None is
    the plain pack, the launch every other caller makes."""
    _dev(src0, src1, out)
    _f32(src0, "src0")
    _f32(src1, "src1")
    B, c0 = src0.shape[0], src0.shape[1]
    hw = src0.shape[2] * src0.shape[3]
    c1 = 0 if src1 is None else src1.shape[1]
    if out is None:
        out = torch.empty((dup * B, hw, cp), dtype=dtype, device=src0.device)
    elif tuple(out.shape) != (dup * B, hw, cp) or out.dtype != dtype:
        raise HipExtensionError("pack_unet_input: `out` has the wrong shape/dtype")
    if div is None:
        check(lib().gmd_pack_unet_input(_ptr(src0), c0, _ptr(src1), c1, B, hw, dup, _ptr(out), cp, dtype_code(dtype), _stream()),
              "gmd_pack_unet_input")
    else:
        d0, d1 = (float(v) for v in div)
        check(lib().gmd_pack_unet_input_scaled(_ptr(src0), c0, d0, _ptr(src1), c1, d1, B, hw, dup, _ptr(out), cp, dtype_code(dtype),
                                               _stream()), "gmd_pack_unet_input_scaled")
    return out


def unpack_nchw(x, B, C, h, w):
    """x: [B, h*w, ld] -> float32 [B, C, h, w] (first C channels)."""
    _dev(x)
    out = torch.empty((B, C, h, w), dtype=torch.float32, device=x.device)
    check(lib().gmd_unpack_nchw(_ptr(x), dtype_code(x.dtype), x.shape[-1], B, C, h * w, _ptr(out), _stream()), "gmd_unpack_nchw")
    return out


def cfg_std_ratio(eps_pair, guidance_scale):
    _dev(eps_pair)
    B = eps_pair.shape[0] // 2
    ratio = torch.empty(B, dtype=torch.float32, device=eps_pair.device)
    check(lib().gmd_cfg_std_ratio(_ptr(_f32(eps_pair, "eps")), B, eps_pair[0].numel(), float(guidance_scale), _ptr(ratio), _stream()),
          "gmd_cfg_std_ratio")
    return ratio


def inpaint_blend(z0, x_prev=None, x0=None, mask=None, noise=None, coefs=(1.0, 0.0)):
    """The img2img start / inpaint blend of one step as ONE launch (gmd_inpaint_blend), in place on ``x_prev`` and ``x0``:
    ``keep = ca * z0 + cb * noise`` (``z0`` itself without ``noise``), ``x_prev = (1 - m) * keep + m * x_prev`` (``keep`` without a
    mask: ``x_prev`` is then written, never read) and ``x0 = (1 - m) * z0 + m * x0``.  z0 / noise / x_prev / x0: float32
    [B, C, h, w]; mask: float32 [1 | B, 1, h, w]; coefs = (ca, cb) of the scheduler's ``add_noise_coefs``.  Returns (x_prev, x0)."""
    _dev(z0, x_prev, x0, mask, noise)
    for t in (z0, x_prev, x0, mask, noise):
        _f32(t, "latent tensors")
    if z0.dim() != 4 or _shape_differs(z0, x_prev, x0, noise):
        raise HipExtensionError("inpaint_blend: z0 must be [B, C, h, w] and x_prev, x0 and noise must have its shape")
    B, C, h, w = z0.shape
    if mask is not None and (mask.dim() != 4 or mask.shape[1:] != (1, h, w)):
        raise HipExtensionError(f"inpaint_blend: mask must be [1 | {B}, 1, {h}, {w}] (got {tuple(mask.shape)})")
    ca, cb = (float(v) for v in coefs)
    check(lib().gmd_inpaint_blend(_ptr(x_prev), _ptr(x0), _ptr(mask), _ptr(z0), _ptr(noise), B, C, h * w,
                                  1 if mask is None else mask.shape[0], ca, cb, _stream()), "gmd_inpaint_blend")
    return x_prev, x0


def _shape_differs(x, *tensors):
    return any(t is not None and t.shape != x.shape for t in tensors)


def _fused_step(entry, eps_in, x, inputs, guide, scalars, n_out, want=(), hist=None, refuse=()):
    """What the fused latent steps share: every gmd_*_step takes (eps_in, x, <inputs>, B, chw, <guide>, <scalars>, <outputs>, stream).
    ``inputs``: the entry point's further input tensors in its order (None = a null pointer); ``hist``: a history that follows them,
    newest first, of which three entries are passed (None-padded; None: the entry point takes no history); ``guide`` = (do_cfg, guidance_scale, ratio, guidance_rescale);
    ``refuse``: (condition, message) pairs of the caller's own refusals, looked at in order after the device and float32 checks.
    Returns ``n_out`` tensors like ``x`` and then one per ``want`` flag (None where it is false), allocated HERE at every call:
    what a scheduler keeps as history is never the static buffer of a captured graph.  ``entry`` is looked up on ``lib()`` now."""
    do_cfg, guidance_scale, ratio, guidance_rescale = guide
    _dev(eps_in, x, ratio, *inputs, *(hist or ()))
    for t in (eps_in, x, *inputs, *(hist or ())):
        _f32(t, "latent tensors")
    for bad, message in refuse:
        if bad:
            raise HipExtensionError(message)
    if hist is not None:
        inputs = (*inputs, *hist[:3], *[None] * (3 - len(hist[:3])))
    outs = [torch.empty_like(x) for _ in range(n_out)] + [torch.empty_like(x) if w else None for w in want]
    check(getattr(lib(), entry)(_ptr(eps_in), _ptr(x), *(_ptr(t) for t in inputs), x.shape[0], x.shape[1:].numel(), int(do_cfg),
                                float(guidance_scale), _ptr(ratio), float(guidance_rescale), *scalars, *(_ptr(t) for t in outs),
                                _stream()), entry)
    return tuple(outs)


def latent_step(eps_in, x, mode, coefs, do_cfg, guidance_scale, cur_sample=None, hist=(), ratio=None,
                guidance_rescale=0.0, want_x0=False):
    """Fused CFG + x0 + PLMS update.  coefs = (sample_coeff, alpha_delta, denom, sqrt_alpha, sqrt_one_minus_alpha).
    Returns (eps, x_prev, x0|None)."""
    sc, ad, dn, sa, s1 = (float(c) for c in coefs)
    return _fused_step("gmd_latent_step", eps_in, x, (cur_sample,), (do_cfg, guidance_scale, ratio, guidance_rescale),
                       (mode, sc, ad, dn, sa, s1), 2, (want_x0,), hist=hist)


def dpm_step(eps_in, x, order, coefs, do_cfg, guidance_scale, m1=None, ratio=None, guidance_rescale=0.0, want_x0=False):
    """Fused CFG + x0 + DPM-Solver++ (orders 1-2) update.  coefs = (sigma_s0, alpha_s0, c_x, c_m, c_h, inv_r0, sqrt_alpha,
    sqrt_one_minus_alpha).  Returns (m0, x_prev, x0|None)."""
    return _fused_step("gmd_dpm_step", eps_in, x, (m1,), (do_cfg, guidance_scale, ratio, guidance_rescale),
                       (int(order), *(float(v) for v in coefs)), 2, (want_x0,))


def dpm_sde_step(eps_in, x, order, coefs, do_cfg, guidance_scale, noise, m1=None, ratio=None, guidance_rescale=0.0, want_x0=False):
    """Fused CFG + x0 + SDE-DPM-Solver++ (orders 1-2) update.  coefs = (sigma_s0, alpha_s0, c_x, c_m, c_h, inv_r0, c_n, sqrt_alpha,
    sqrt_one_minus_alpha); ``noise`` is required and added at every step (also with c_n == 0).  Returns (m0, x_prev, x0|None)."""
    return _fused_step("gmd_dpm_sde_step", eps_in, x, (m1, noise), (do_cfg, guidance_scale, ratio, guidance_rescale),
                       (int(order), *(float(v) for v in coefs)), 2, (want_x0,),
                       refuse=[(noise is None or _shape_differs(x, noise), "dpm_sde_step: noise must have the sample's shape")])


def ddpm_step(eps_in, x, coefs, do_cfg, guidance_scale, noise=None, ratio=None, guidance_rescale=0.0, clip_range=None,
              want_x0=False):
    """Fused CFG + x0 + DDPM ancestral update.  coefs = (sched_sqrt_alpha, sched_sqrt_one_minus_alpha, x0_coeff, xt_coeff,
    noise_scale, sqrt_alpha, sqrt_one_minus_alpha); ``noise`` is None at the last step (t == 0); ``clip_range`` None = no
    clip_sample.  Returns (x_prev, x0|None)."""
    sa, s1, c0, ct, ns, pa, p1 = (float(v) for v in coefs)
    return _fused_step("gmd_ddpm_step", eps_in, x, (noise,), (do_cfg, guidance_scale, ratio, guidance_rescale),
                       (sa, s1, int(clip_range is not None), float(clip_range or 0.0), c0, ct, ns, pa, p1), 1, (want_x0,),
                       refuse=[(_shape_differs(x, noise), "ddpm_step: noise must have the sample's shape")])


def ddim_step(eps_in, x, coefs, do_cfg, guidance_scale, noise=None, ratio=None, guidance_rescale=0.0, clip_range=None,
              use_clipped=False, want_x0=False, want_pred_x0=False):
    """Fused CFG + x0 + DDIM update.  coefs = (sched_sqrt_alpha, sched_sqrt_one_minus_alpha, sqrt_alpha_prev, dir_coeff, std_dev,
    sqrt_alpha, sqrt_one_minus_alpha); ``noise`` is None when eta == 0 and is added whenever given (also with std_dev == 0);
    ``clip_range`` None = no clip_sample; ``use_clipped`` = use_clipped_model_output.  Returns (x_prev, x0|None, pred_x0|None):
    x0 is the pipeline's never-clipped prediction, pred_x0 diffusers' (clipped) pred_original_sample."""
    sa, s1, sp, dc, sd, pa, p1 = (float(v) for v in coefs)
    return _fused_step("gmd_ddim_step", eps_in, x, (noise,), (do_cfg, guidance_scale, ratio, guidance_rescale),
                       (sa, s1, int(clip_range is not None), float(clip_range or 0.0), int(bool(use_clipped)), sp, dc, sd, pa, p1),
                       1, (want_x0, want_pred_x0), refuse=[(_shape_differs(x, noise), "ddim_step: noise must have the sample's shape")])


def lcm_step(eps_in, x, coefs, do_cfg, guidance_scale, noise=None, ratio=None, guidance_rescale=0.0, clip_range=None,
             want_x0=False, want_denoised=False):
    """Fused CFG + x0 + latent-consistency (LCM) update.  coefs = (sched_sqrt_alpha, sched_sqrt_one_minus_alpha, c_skip, c_out,
    sqrt_alpha_prev, sqrt_beta_prev, sqrt_alpha, sqrt_one_minus_alpha); ``noise`` is None at the last step, where x_prev is the
    denoised sample itself; ``clip_range`` None = no clip_sample.  Returns (x_prev, x0|None, denoised|None): x0 is the pipeline's
    never-clipped prediction, denoised = c_out * p0 + c_skip * x.  The outputs are allocated here, so nothing the scheduler keeps
    is ever the static buffer of a captured graph."""
    sa, s1, cs, co, sp, bp, pa, p1 = (float(v) for v in coefs)
    return _fused_step("gmd_lcm_step", eps_in, x, (noise,), (do_cfg, guidance_scale, ratio, guidance_rescale),
                       (sa, s1, int(clip_range is not None), float(clip_range or 0.0), cs, co, sp, bp, pa, p1), 1, (want_x0, want_denoised),
                       refuse=[(_shape_differs(x, noise), "lcm_step: noise must have the sample's shape")])


def euler_step(eps_in, x, coefs, do_cfg, guidance_scale, noise=None, ratio=None, guidance_rescale=0.0, want_pred_x0=False):
    """Fused CFG + Euler / Euler-ancestral update.  coefs = (sigma_hat, dt, sigma_up); ``noise`` is None for the deterministic
    scheduler and is added whenever given (also with sigma_up == 0).  Returns (x_prev, pred_x0|None): pred_x0 = x - sigma_hat eps."""
    sh, dt, su = (float(v) for v in coefs)
    return _fused_step("gmd_euler_step", eps_in, x, (noise,), (do_cfg, guidance_scale, ratio, guidance_rescale), (sh, dt, su), 1,
                       (want_pred_x0,), refuse=[(_shape_differs(x, noise), "euler_step: noise must have the sample's shape")])


def lms_step(eps_in, x, order, coefs, do_cfg, guidance_scale, hist=(), ratio=None, guidance_rescale=0.0, want_pred_x0=False):
    """Fused CFG + linear multistep (LMS, orders 1-4) update.  coefs = (sigma, c0, c1, c2, c3); ``hist``: the derivatives of the
    previous steps, newest first, of which the first order - 1 are read.  Returns (d, x_prev, pred_x0|None): d = the step's
    derivative, pred_x0 = x - sigma eps.  The three outputs are allocated here, so the derivative the caller keeps as history is
    never the static buffer of a captured graph."""
    order = int(order)
    sg, c0, c1, c2, c3 = (float(v) for v in coefs)
    return _fused_step("gmd_lms_step", eps_in, x, (), (do_cfg, guidance_scale, ratio, guidance_rescale), (order, sg, c0, c1, c2, c3), 2,
                       (want_pred_x0,), hist=hist,
                       refuse=[(len(hist) < order - 1, f"lms_step: order {order} needs {order - 1} earlier derivatives (got {len(hist)})"),
                               (_shape_differs(x, *hist), "lms_step: a history tensor must have the sample's shape")])


def unipc_step(eps_in, x, corr_order, pred_order, coefs, do_cfg, guidance_scale, last_sample=None, hist=(), ratio=None, guidance_rescale=0.0,
               want_x0=False):
    """Fused CFG + UniPC corrector (order 0 = off .. 3) + predictor (order 1-3) update.  coefs = the 19 floats of gmd_unipc_step in its
    order: (sigma_s, alpha_s, c_x, c_m, c_b, c_rho1, c_rho2, c_rho3, c_r1, c_r2, p_x, p_m, p_b, p_rho1, p_rho2, p_r1, p_r2, sqrt_alpha,
    sqrt_one_minus_alpha).  ``hist``: the x0 predictions of the previous steps, newest first (at most three are passed on);
    ``last_sample``: the corrected sample of the previous step.  Returns (m0, x_corr, x_prev, x0|None), all allocated here, so what the
    caller keeps as history is never the static buffer of a captured graph nor the caller's own sample."""
    p, q = int(corr_order), int(pred_order)
    need = max(p, q - 1)
    c = [float(v) for v in coefs]
    return _fused_step("gmd_unipc_step", eps_in, x, (last_sample,), (do_cfg, guidance_scale, ratio, guidance_rescale), (p, q, *c), 3,
                       (want_x0,), hist=hist,
                       refuse=[(len(hist) < need, f"unipc_step: corrector order {p} / predictor order {q} needs {need} earlier x0"
                                                  f" predictions (got {len(hist)})"),
                               (p >= 1 and last_sample is None, f"unipc_step: corrector order {p} needs last_sample"),
                               (_shape_differs(x, last_sample, *hist),
                                "unipc_step: history tensors and last_sample must have the sample's shape"),
                               (len(c) != 19, f"unipc_step: 19 coefficients expected (got {len(c)})")])


# ----------------------------------------------------------------------------------------------
# HDR tail
# ----------------------------------------------------------------------------------------------
def hdr_tail(sdr_dec, gm_dec, layout, B, H, W, qmax=99.0, eps=1 / 64, clamp=False,
             want=("sdr", "gm", "sdr_u8", "gm_u8", "hdr", "hdr_file", "hdr_u16")):
    """layout 0: [B,3,H,W]; 1: [B,H*W,3]; 2: [B,H*W,4].  Returns dict of [B,H,W,3] tensors."""
    _dev(sdr_dec, gm_dec)
    if sdr_dec.dtype != gm_dec.dtype:
        raise HipExtensionError("hdr_tail: dtype mismatch")
    dev = sdr_dec.device
    shp = (B, H, W, 3)
    kinds = {"sdr": torch.float32, "gm": torch.float32, "sdr_u8": torch.uint8, "gm_u8": torch.uint8,
             "hdr": torch.float32, "hdr_file": torch.float32, "hdr_u16": torch.uint16}
    out = {k: torch.empty(shp, dtype=kinds[k], device=dev) for k in want}
    g = lambda k: _ptr(out.get(k))
    tm, t0 = _timed("hdr_tail")
    check(lib().gmd_hdr_tail(_ptr(sdr_dec), _ptr(gm_dec), dtype_code(sdr_dec.dtype), layout, B, H, W, float(qmax), float(eps),
                             1 if clamp else 0, g("sdr"), g("gm"), g("sdr_u8"), g("gm_u8"), g("hdr"), g("hdr_file"),
                             g("hdr_u16"), _stream()), "gmd_hdr_tail")
    if tm:  # 2 x 3 float32 read per pixel + every requested output written once
        px = B * H * W
        tm.end("hdr_tail", 0.0, px * 2 * 3 * sdr_dec.element_size() + sum(v.numel() * v.element_size() for v in out.values()), t0)
    return out


_TAIL_KINDS = {"sdr": torch.float32, "gm": torch.float32, "sdr_u8": torch.uint8, "gm_u8": torch.uint8,
               "hdr": torch.float32, "hdr_file": torch.float32, "hdr_u16": torch.uint16, "hdr_rgbe": torch.uint8}


def _operand_hw(t, layout, hw, name):
    """(h, w) of a tail operand: read off a [B,3,h,w] tensor, given by the caller for the flattened channels-last layouts."""
    if layout == 0 and t.dim() == 4:
        h, w = int(t.shape[2]), int(t.shape[3])
        if hw is not None and tuple(hw) != (h, w):
            raise HipExtensionError(f"hdr_tail_resized: {name}_hw={tuple(hw)} but the tensor is {h}x{w}")
        return h, w
    if hw is None:
        raise HipExtensionError(f"hdr_tail_resized: {name}_hw is needed for layout {layout}")
    h, w = int(hw[0]), int(hw[1])
    ch = (3, 3, 4)[layout]
    if t.numel() != t.shape[0] * h * w * ch:
        raise HipExtensionError(f"hdr_tail_resized: {name} has {t.numel()} elements, expected B x {h} x {w} x {ch}")
    return h, w


def hdr_tail_resized(sdr, gm_dec, layout, out_size, sdr_hw=None, gm_hw=None, qmax=99.0, eps=1 / 64, clamp=False, source_u8=False,
                     want=("sdr", "gm", "sdr_u8", "gm_u8", "hdr", "hdr_file", "hdr_u16", "hdr_rgbe")):
    """The fused tail at ``out_size`` = (H, W): both operands (layouts of ``hdr_tail``; ``sdr_hw`` / ``gm_hw`` give the sizes of
    flattened channels-last operands) are bilinearly resampled onto it inside the kernel (gmd_hdr_tail_resized).  ``source_u8``: ``sdr``
    is a uint8 [B,H,W,3] picture already at the output size.  Returns a dict of [B,H,W,3] tensors (``hdr_rgbe``: [B,H,W,4] uint8)."""
    _dev(sdr, gm_dec)
    H, W = int(out_size[0]), int(out_size[1])
    B = gm_dec.shape[0]
    if source_u8:
        if sdr.dtype != torch.uint8 or tuple(sdr.shape) != (B, H, W, 3):
            raise HipExtensionError(f"hdr_tail_resized: source_u8 expects a uint8 [{B}, {H}, {W}, 3] picture, got {sdr.dtype} {tuple(sdr.shape)}")
        hs, ws = H, W
    else:
        if sdr.dtype != gm_dec.dtype:
            raise HipExtensionError("hdr_tail_resized: dtype mismatch")
        if sdr.shape[0] != B:
            raise HipExtensionError("hdr_tail_resized: batch mismatch")
        hs, ws = _operand_hw(sdr, layout, sdr_hw, "sdr")
    hg, wg = _operand_hw(gm_dec, layout, gm_hw, "gm")
    unknown = [k for k in want if k not in _TAIL_KINDS]
    if unknown:
        raise HipExtensionError(f"hdr_tail_resized: unknown outputs {unknown}")
    dev = gm_dec.device
    out = {k: torch.empty((B, H, W, 4 if k == "hdr_rgbe" else 3), dtype=_TAIL_KINDS[k], device=dev) for k in want}
    g = lambda k: _ptr(out.get(k))
    tm, t0 = _timed("hdr_tail_resized")
    check(lib().gmd_hdr_tail_resized(_ptr(sdr), hs, ws, _ptr(gm_dec), hg, wg, dtype_code(gm_dec.dtype), layout, B, H, W, float(qmax),
                                     float(eps), (1 if clamp else 0) | (2 if source_u8 else 0), g("sdr"), g("gm"), g("sdr_u8"),
                                     g("gm_u8"), g("hdr"), g("hdr_file"), g("hdr_u16"), g("hdr_rgbe"), _stream()), "gmd_hdr_tail_resized")
    if tm:  # the operands are read once from HBM (the four taps of neighbouring pixels hit the caches) + every requested output written once
        rd = B * 3 * (hg * wg * gm_dec.element_size() + hs * ws * sdr.element_size())
        tm.end("hdr_tail_resized", 0.0, rd + sum(v.numel() * v.element_size() for v in out.values()), t0)
    return out


def prepare_sdr(images_u8, size, dtype=torch.float32, layout="nchw", cp=8):
    """uint8 [B,h,w,3] pictures -> the normalised VAE input at ``size`` = (H, W): antialiased bilinear resize, ToTensor,
    Normalize([0.5], [0.5]) in one kernel (gmd_prepare_sdr).  layout "nchw": [B,3,H,W]; "nhwc": [B,H*W,cp] channels-last with the
    padding channels zeroed (what ``AutoencoderKL.encode_nhwc`` consumes)."""
    _dev(images_u8)
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[-1] != 3:
        raise HipExtensionError(f"prepare_sdr expects uint8 [B, h, w, 3], got {images_u8.dtype} {tuple(images_u8.shape)}")
    if layout not in ("nchw", "nhwc"):
        raise HipExtensionError("prepare_sdr: layout must be 'nchw' or 'nhwc'")
    B, h, w = (int(v) for v in images_u8.shape[:3])
    H, W = int(size[0]), int(size[1])
    out = torch.empty((B, 3, H, W) if layout == "nchw" else (B, H * W, cp), dtype=dtype, device=images_u8.device)
    tm, t0 = _timed("prepare_sdr")
    check(lib().gmd_prepare_sdr(_ptr(images_u8), B, h, w, _ptr(out), dtype_code(dtype), 0 if layout == "nchw" else 1, int(cp), H, W, _stream()),
          "gmd_prepare_sdr")
    if tm:  # the picture read once + the output written once
        tm.end("prepare_sdr", 0.0, images_u8.numel() + out.numel() * out.element_size(), t0)
    return out


def apply_gm_to_sdr(gm, sdr, qmax=9, eps=1 / 64, clamp=True):
    _dev(gm, sdr)
    gm, sdr = torch.broadcast_tensors(gm, sdr)
    gm, sdr = _f32(gm.contiguous(), "gm"), _f32(sdr.contiguous(), "sdr")
    out = torch.empty_like(sdr)
    check(lib().gmd_apply_gm_to_sdr(_ptr(gm), _ptr(sdr), _ptr(out), sdr.numel(), float(qmax), float(eps), int(clamp), _stream()),
          "gmd_apply_gm_to_sdr")
    return out


def tmo(x, kind, qmax=0.0, mu=500.0):
    _dev(x)
    _f32(x, "tmo input")
    out = torch.empty_like(x)
    check(lib().gmd_tmo(_ptr(x), _ptr(out), x.numel(), kind, float(qmax), float(mu), _stream()), "gmd_tmo")
    return out


def gamut_compress(x):
    _dev(x)
    _f32(x, "gamut_compress input")
    if x.dim() != 4 or x.shape[1] != 3:
        raise HipExtensionError("gamut_compress expects (B, 3, H, W)")
    out = torch.empty_like(x)
    check(lib().gmd_gamut_compress(_ptr(x), _ptr(out), x.shape[0], x.shape[2] * x.shape[3], _stream()), "gmd_gamut_compress")
    return out


def stage1_chain(gm, sdr, qmax):
    _dev(gm, sdr)
    _f32(gm, "gm")
    _f32(sdr, "sdr")
    out = torch.empty_like(sdr)
    check(lib().gmd_stage1_chain(_ptr(gm), _ptr(sdr), _ptr(out), sdr.shape[0], sdr.shape[2] * sdr.shape[3], float(qmax), _stream()),
          "gmd_stage1_chain")
    return out


def discretize_u16(x, codes=False):
    _dev(x)
    _f32(x, "discretize input")
    outf = torch.empty_like(x)
    outc = torch.empty(x.shape, dtype=torch.uint16, device=x.device) if codes else None
    check(lib().gmd_discretize_u16(_ptr(x), _ptr(outf), _ptr(outc), x.numel(), _stream()), "gmd_discretize_u16")
    return (outf, outc) if codes else outf


def quantize_u8(x):
    _dev(x)
    _f32(x, "quantize input")
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(lib().gmd_quantize_u8(_ptr(x), _ptr(out), x.numel(), _stream()), "gmd_quantize_u8")
    return out


def gemm_raw(a_ptr, w_ptr, c_ptr, dtype, out_dtype, M, N, K, lda, ldw, ldc, batch=1, sA=0, sW=0, sC=0,
             bias=None, alpha=1.0, act=ACT_NONE, exact=False):
    """Pointer-level gmd_gemm_nt for strided sub-blocks (per-head attention products of the parity path).
    a_ptr/w_ptr/c_ptr are integer device addresses; the caller keeps the owning tensors alive."""
    _dev(bias)
    code = GMD_F32S if (dtype == torch.float32 and f32_mode() == "split" and K % 32 == 0 and not exact) else dtype_code(dtype)
    check(lib().gmd_gemm_nt(a_ptr, w_ptr, c_ptr, code, dtype_code(out_dtype), M, N, K, lda, ldw, ldc, batch,
                            sA, sW, sC, _ptr(_f32(bias, "bias")), None, 0, 0, None, 0, 0, float(alpha), act, None, 0, None, 0, _stream()),
          "gmd_gemm_nt")


def rgbe_encode(rgb):
    """float32 [..., 3] non-negative RGB -> uint8 [..., 4] Radiance RGBE pixels."""
    _dev(rgb)
    _f32(rgb, "rgbe input")
    if rgb.shape[-1] != 3:
        raise HipExtensionError("rgbe_encode expects [..., 3]")
    out = torch.empty(rgb.shape[:-1] + (4,), dtype=torch.uint8, device=rgb.device)
    check(lib().gmd_rgbe_encode(_ptr(rgb), _ptr(out), rgb.numel() // 3, _stream()), "gmd_rgbe_encode")
    return out
