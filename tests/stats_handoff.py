"""Helpers of the GroupNorm statistics hand-off tests (test_stats_handoff_gpu.py, test_stats_handoff_cpu.py).

Every GroupNorm that does not fit the single-launch kernel takes its statistics from float32 numbers ANOTHER launch left in memory:
  partial sums   workspace[b][split][g] = {sum, sumsq}      gn_partial_kernel -> gn_apply_ws_kernel / gn_finalize_kernel (csrc/norm.hip)
  scale / shift  scale_shift[b][c] = {rstd gamma, beta - mean rstd gamma}      gn_finalize_kernel -> gn_apply_kernel
  bucket sums    colstats[M/64][N/bucket] = {sum, sumsq}    row epilogue of gmd_gemm_nt / gmd_conv3x3 (csrc/gemm.hip, gemm_shared.h:
                                                            colstats_pass / colstats_store) -> gn_apply_cs_kernel
A consumer that reads an entry its producer did not write this launch reads what the LAST launch left there: in a denoising loop the
almost-right sums of the previous step.  Here: float64 references of the three buffers with a derived bound per entry (zero
violations allowed, as in tests/parity.py), ``unwritten`` for NaN-pre-filled buffers, and a toy emulation of partial -> fold -> apply
with the faults the checks exist for.  Plain functions of tensors, any device; the reference is always float64 torch.
"""
import torch

import parity as P
from handoff import SCHEDULE, assert_sequence, first_mismatch, nan_words  # noqa: F401  (re-exported: one import for the two test files)

U_F32 = P.U_F32
KTHREADS = 256      # kThreads of csrc/norm.hip
LDS_LIMIT = 65536   # the launchers' check of the partial kernel's dynamic LDS: PY * C * 2 floats


# ---------------------------------------------------------------------------------------------------------------------------
# geometry of gn_partial_kernel
# ---------------------------------------------------------------------------------------------------------------------------
def nsplit_rule(HW):
    """gmd_groupnorm_nsplit as csrc/norm.hip has it today (the GPU tests ask the library and assert what follows from its answer;
    this copy serves the CPU file): HW / 64 from 4096 pixels up, HW / 32 below, clamped to [1, 256]."""
    n = HW // 64 if HW >= 4096 else HW // 32
    return max(1, min(256, n))


def block_rows(HW, nsplit):
    """(per, [(p0, p1)] per block): block ``split`` owns the rows [p0, p1) with per = ceil(HW / nsplit), p0 = split * per, p1 = min(p0 + per, HW).
    A trailing block with p0 >= HW is EMPTY (p1 <= p0; p1 < p0 when it starts beyond HW): it must still store {0, 0}."""
    per = -(-HW // nsplit)
    return per, [(s * per, min(s * per + per, HW)) for s in range(nsplit)]


def empty_blocks(HW, nsplit):
    return sum(1 for p0, p1 in block_rows(HW, nsplit)[1] if p1 <= p0)


def vec_elems(dtype):
    """Elements of one 16-byte access (Elem<T>::kVec)."""
    return 4 if dtype == torch.float32 else 8


def partial_geometry(C, dtype):
    """(CV, CVB, PY, passes, lds_bytes) of gn_partial_kernel: CV = C / V 16-byte chunks per pixel row, CVB = min(CV, 256) of them side
    by side, PY = 256 / CVB pixel rows per sweep of the workgroup, ``passes`` = trips of the channel loop (2 and more once C / V > 256),
    and the dynamic LDS [PY][C] x {sum, sumsq} floats that the launchers refuse beyond 64 KiB."""
    V = vec_elems(dtype)
    CV = C // V
    CVB = min(CV, KTHREADS)
    PY = KTHREADS // CVB
    return CV, CVB, PY, -(-CV // CVB), PY * C * 2 * 4


def partial_height(HW, nsplit, C, dtype):
    """Longest float32 addition chain of one workspace entry: thread (py, cx) adds the rows p0 + py, p0 + py + PY, ... of its block
    one after the other into a[j] / q[j] -- ceil(per / PY) rows -- and nothing else happens in float32: the fold of the [PY][C/G]
    per-thread sums of a group runs in double, and so do the folds over the splits in gn_finalize_kernel / gn_apply_ws_kernel."""
    per = -(-HW // nsplit)
    return -(-per // partial_geometry(C, dtype)[2])


def producer_height(bucket):
    """Longest float32 addition chain of one bucket entry (csrc/gemm_shared.h): colstats_pass adds the 32 rows of a strip serially per
    column (32 additions, the first onto zero), once per 32-row half of the 64-row wave tile (2 additions onto cs / cq), and
    colstats_store folds ``bucket`` adjacent columns serially: 32 + 2 + bucket (44 at the bucket of 10)."""
    return 32 + 2 + bucket


# ---------------------------------------------------------------------------------------------------------------------------
# float64 references and per-entry bounds
# ---------------------------------------------------------------------------------------------------------------------------
def sum_bounds(abs_sum, sq_sum, height):
    """Bounds of a float32 {sum, sum of squares} whose terms pass through at most ``height`` float32 additions, stacked like the entry.

    A sum evaluated along any tree in which one term meets at most h additions has error <= h 2^-24 sum |x_i| to first order
    (parity.accumulate_bound).  The + 2: the rounding of x * x before it is added (sum of squares), and the one rounding when a
    double fold is stored as float32 (partial sums; the producers keep float32 throughout and have that unit spare).  The second
    order, (1 + u)^h - 1 - h u <= h^2 u^2, is below 10^-5 of the bound for h <= 300 and sits inside the same + 2.  The inputs are
    exact in float32 (bf16 / f16 values convert exactly), so nothing else enters:
        |d sum| <= (h + 2) 2^-24 sum |x|,      |d sumsq| <= (h + 2) 2^-24 sum x^2.
    An entry over no elements (an empty block) gets the bound 0: exactly {0, 0} or a violation."""
    g = (height + 2) * U_F32
    return torch.stack([g * abs_sum, g * sq_sum], -1)


def partial_ref_bound(x, G, nsplit, dtype=None):
    """x: [B, HW, C] stored values -> (ref, bound), float64 [B, nsplit, G, 2]: the workspace gn_partial_kernel must leave, by the
    kernel's row ranges (block_rows), and sum_bounds with partial_height."""
    B, HW, C = x.shape
    dtype = dtype or x.dtype
    per = -(-HW // nsplit)
    x64 = x.to(torch.float64).reshape(B, HW, G, C // G)
    rows = torch.stack([x64.sum(3), (x64 * x64).sum(3), x64.abs().sum(3)], -1)                 # [B, HW, G, 3]
    pad = torch.zeros(B, nsplit * per - HW, G, 3, dtype=torch.float64, device=x.device)    # rows at or beyond HW: nothing
    blocks = torch.cat([rows, pad], 1).reshape(B, nsplit, per, G, 3).sum(2)                  # [B, nsplit, G, 3]
    return blocks[..., :2].contiguous(), sum_bounds(blocks[..., 2], blocks[..., 1], partial_height(HW, nsplit, C, dtype))


def scale_shift_ref_bound(x, G, gamma, beta, eps, height):
    """x: [B, HW, C] -> (ref, bound), float64 [B, C, 2]: scale_shift of gmd_groupnorm_stats.

    gn_finalize_kernel adds the float32 partial sums in double: the group's sum and sum of squares carry g sum|x| and g sum x^2 with
    g = (height + 2) 2^-24 (sum_bounds) and nothing from the fold.  With n = HW C / G, in double:
        d_mean <= g mean|x|;      var = sumsq / n - mean^2:  d_var <= g mean(x^2) + 2 |mean| d_mean + d_mean^2
    (parity.norm_bound's terms).  Then four float32 roundings on the way to the two stored numbers:
        s_mean = (float) mean                               |d| <= d_mean + u (|mean| + d_mean)
        s_rstd = (float) (var + eps)^-1/2                   relative r = d_var / (2 (var + eps)) (1 + d_var / (var + eps)), then (1 + u)
        scale  = s_rstd * gamma[c]                          one rounding: relative (1 + r) (1 + u)^2 - 1 of |gamma| rstd
        shift  = beta[c] - s_mean * scale                   product rule on s_mean * scale, one rounding of the product, one of the
                                                            difference (of terms bounded by |beta| + |mean scale| + what came before)"""
    B, HW, C = x.shape
    u = U_F32
    x64 = x.to(torch.float64).reshape(B, HW, G, C // G)
    mean = x64.mean((1, 3))
    var = ((x64 - mean[:, None, :, None]) ** 2).mean((1, 3))
    g = (height + 2) * u
    d_mean = g * x64.abs().mean((1, 3))
    d_var = g * (x64 * x64).mean((1, 3)) + 2 * mean.abs() * d_mean + d_mean ** 2
    rstd = (var + eps).rsqrt()
    r = d_var / (2 * (var + eps)) * (1 + d_var / (var + eps))

    def per_channel(t):  # [B, G] -> [B, C]
        return t[:, :, None].expand(B, G, C // G).reshape(B, C)

    ga, be = gamma.to(torch.float64)[None, :], beta.to(torch.float64)[None, :]
    mean_c, rstd_c = per_channel(mean), per_channel(rstd)
    scale = rstd_c * ga
    shift = be - mean_c * scale
    e_scale = scale.abs() * ((1 + per_channel(r)) * (1 + u) ** 2 - 1)
    e_mean = per_channel(d_mean) + u * (mean_c.abs() + per_channel(d_mean))
    prod = (mean_c * scale).abs()
    e_prod = e_mean * (scale.abs() + e_scale) + mean_c.abs() * e_scale
    e_prod = e_prod + u * (prod + e_prod)
    e_shift = e_prod + u * (be.abs() + prod + e_prod)
    return torch.stack([scale, shift], -1), torch.stack([e_scale, e_shift], -1)


def bucket_sums(y, bucket):
    """float64 {sum, sumsq} of the stored values per 64-row block and per bucket of adjacent columns: [M/64, N/bucket, 2]."""
    M, N = y.shape
    v = y.double().view(M // 64, 64, N // bucket, bucket)
    return torch.stack([v.sum((1, 3)), (v * v).sum((1, 3))], -1)


def bucket_ref_bound(y, bucket):
    """y: [M, N] STORED output of a producer -> (ref, bound), float64 [M/64, N/bucket, 2].  The reference is the float64 sum of the
    stored values, as include/gmd_hip.h defines the statistics ("of the STORED (rounded) outputs"); sum_bounds with producer_height."""
    M, N = y.shape
    v = y.to(torch.float64).view(M // 64, 64, N // bucket, bucket)
    return bucket_sums(y, bucket), sum_bounds(v.abs().sum((1, 3)), (v * v).sum((1, 3)), producer_height(bucket))


def assert_entries(got, ref, bound, what):
    """parity.assert_elementwise on a statistics buffer ([..., 2] entries): zero violations; returns max |err| / bound."""
    return P.assert_elementwise(got.reshape(ref.shape), ref, bound, what)


# ---------------------------------------------------------------------------------------------------------------------------
# NaN-pre-filled buffers
# ---------------------------------------------------------------------------------------------------------------------------
def nan_fill(buf):
    """Fill a float32 buffer with handoff.nan_words (in place, stream-ordered); returns it."""
    buf.view(torch.int32).copy_(nan_words(buf.numel(), buf.device))
    return buf


def unwritten(buf_after, extent):
    """Indices (int64 tensor) of the words inside the documented extent -- the first ``extent`` floats: B nsplit G 2 of a workspace,
    B C 2 of scale_shift, (M / 64) (N / bucket) 2 of producer statistics -- of a nan_fill-ed buffer that still hold their fill word
    after a launch: entries the launch did not write.  Raises if a word at or beyond the extent changed (the buffer must be longer than
    the extent for that to mean anything; the guard bands round it are test_footprint_gpu.Guarded's)."""
    words = buf_after.reshape(-1).view(torch.int32)
    assert 0 <= extent <= words.numel()
    pat = nan_words(words.numel(), words.device)
    beyond = words[extent:] != pat[extent:]
    if bool(beyond.any()):
        raise AssertionError(f"{int(beyond.sum())} words at or beyond the documented extent of {extent} floats changed; first at word "
                             f"{extent + int(beyond.nonzero()[0])}")
    return (words[:extent] == pat[:extent]).nonzero().reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------
# Toy emulation of partial -> fold -> apply and of the producer's column pass, with switchable faults
# ---------------------------------------------------------------------------------------------------------------------------
class StatsEmulation:
    """GroupNorm of x [B, HW, C] as the split path computes it, on buffers that outlive the launch: ``ws`` (partial sums, SLACK spare
    words behind the extent), ``ss`` (scale / shift) and ``cs`` (bucket sums of a producer).  float32 where the kernels use float32, in
    the kernels' order (a thread's serial chain over its rows; the serial row / half / bucket chains of the column pass), double where
    they use double.  ``dtype`` is the element type: it sets the 16-byte vector width (hence PY and the chain length) and the rounding
    of the output.

    Faults (``fault`` = (kind, ...) or None):
      ("skip_store", b, split)     that block of the partial launch does not store its entry
      ("skip_empty_store",)        blocks without rows return before the store
      ("short_fold",)              the fold reads the entries 0 .. nsplit - 2
      ("stale_consumer",)          the consumer reads the buffer as it was BEFORE this launch's producer ran
      ("bucket_neighbour", r, k)   bucket entry (r, k) holds the value of entry (r, k + 1)"""
    SLACK = 64

    def __init__(self, B, HW, C, G, dtype=torch.float32, nsplit=None, bucket=10, eps=1e-5, fault=None):
        self.B, self.HW, self.C, self.G, self.dtype, self.eps, self.fault, self.bucket = B, HW, C, G, dtype, eps, fault, bucket
        self.nsplit = nsplit_rule(HW) if nsplit is None else nsplit
        self.PY = partial_geometry(C, dtype)[2]
        self.extent = B * self.nsplit * G * 2
        self.ws = torch.zeros(self.extent + self.SLACK, dtype=torch.float32)
        self.ss = torch.zeros(B * C * 2 + self.SLACK, dtype=torch.float32)
        self.cs = None

    def height(self):
        return partial_height(self.HW, self.nsplit, self.C, self.dtype)

    def fill(self, kind, buf="ws"):
        t = getattr(self, buf)
        if kind == "nan":
            nan_fill(t)
        else:
            t.zero_()

    # -- producers ---------------------------------------------------------------------------------------------------------
    def partial(self, x):
        B, HW, C, G, ns, PY = self.B, self.HW, self.C, self.G, self.nsplit, self.PY
        per, ranges = block_rows(HW, ns)
        steps = -(-per // PY)
        x = x.to(torch.float32)
        idx = torch.tensor([p0 for p0, _ in ranges])[:, None] + torch.arange(steps * PY)[None, :]       # [ns, steps PY]
        live = idx < torch.tensor([p1 for _, p1 in ranges])[:, None]
        rows = x[:, idx.clamp(max=HW - 1)] * live[None, :, :, None]                                      # rows past p1: + 0, exact
        rows = rows.reshape(B, ns, steps, PY, C)
        a = torch.zeros(B, ns, PY, C)
        q = torch.zeros(B, ns, PY, C)
        for t in range(steps):  # thread (py, cx): row p0 + py + t PY
            a = a + rows[:, :, t]
            q = q + rows[:, :, t] * rows[:, :, t]
        out = torch.stack([a.double().reshape(B, ns, PY, G, C // G).sum((2, 4)), q.double().reshape(B, ns, PY, G, C // G).sum((2, 4))], -1)
        out = out.to(torch.float32)                                                                      # [B, ns, G, 2]
        view = self.ws[:self.extent].view(B, ns, G, 2)
        keep = view.clone()
        view.copy_(out)
        if self.fault and self.fault[0] == "skip_store":
            _, b, s = self.fault
            view[b, s] = keep[b, s]
        if self.fault and self.fault[0] == "skip_empty_store":
            for s, (p0, p1) in enumerate(ranges):
                if p1 <= p0:
                    view[:, s] = keep[:, s]

    def produce_buckets(self, y):
        """The column pass of the row epilogue on the stored tensor y [M, N] into ``cs`` (allocated on first use)."""
        M, N = y.shape
        bk = self.bucket
        v = y.to(torch.float32).view(M // 64, 2, 32, N)
        s = torch.zeros(M // 64, 2, N)
        q = torch.zeros(M // 64, 2, N)
        for r in range(32):
            s = s + v[:, :, r]
            q = q + v[:, :, r] * v[:, :, r]
        cs, cq = s[:, 0] + s[:, 1], q[:, 0] + q[:, 1]
        cs, cq = cs.view(M // 64, N // bk, bk), cq.view(M // 64, N // bk, bk)
        bs = torch.zeros(M // 64, N // bk)
        bq = torch.zeros(M // 64, N // bk)
        for e in range(bk):
            bs = bs + cs[..., e]
            bq = bq + cq[..., e]
        out = torch.stack([bs, bq], -1)
        if self.fault and self.fault[0] == "bucket_neighbour":
            _, r, k = self.fault
            out[r, k] = out[r, k + 1]
        n = out.numel()
        if self.cs is None:
            self.cs = torch.zeros(n + self.SLACK, dtype=torch.float32)
        self.cs[:n] = out.reshape(-1)
        return n

    # -- consumers ---------------------------------------------------------------------------------------------------------
    def _scale_shift(self, s, s2, gamma, beta):
        """[B, G] double sums -> float32 [B, C, 2] as gn_finalize_kernel / the apply kernels' prologue compute it."""
        B, C, G = self.B, self.C, self.G
        n = float(self.HW * (C // G))
        mean = s / n
        var = (s2 / n - mean * mean).clamp_min(0.0)
        mean_f = mean.to(torch.float32)
        rstd_f = (1.0 / (var + self.eps).sqrt()).to(torch.float32)
        rep = lambda t: t[:, :, None].expand(B, G, C // G).reshape(B, C)  # noqa: E731
        sc = rep(rstd_f) * gamma[None, :]
        return torch.stack([sc, beta[None, :] - rep(mean_f) * sc], -1)

    def _apply(self, x, ss, silu):
        y = x.to(torch.float32) * ss[:, None, :, 0] + ss[:, None, :, 1]
        if silu:
            y = y * torch.sigmoid(y)
        return y.to(self.dtype)

    def _fold_ws(self, src):
        view = src[:self.extent].view(self.B, self.nsplit, self.G, 2).double()
        if self.fault and self.fault[0] == "short_fold":
            view = view[:, :-1]
        return view[..., 0].sum(1), view[..., 1].sum(1)

    def launch_split(self, x, gamma, beta, silu=False):
        """gmd_groupnorm_split: partial, then an apply whose workgroups fold the partials themselves."""
        before = self.ws.clone()
        self.partial(x)
        src = before if self.fault and self.fault[0] == "stale_consumer" else self.ws
        return self._apply(x, self._scale_shift(*self._fold_ws(src), gamma, beta), silu)

    def launch_stats_apply(self, x, gamma, beta, silu=False):
        """gmd_groupnorm_stats (partial, finalize into ``ss``) + gmd_groupnorm_apply."""
        before = self.ss.clone()
        self.partial(x)
        n = self.B * self.C * 2
        self.ss[:n] = self._scale_shift(*self._fold_ws(self.ws), gamma, beta).reshape(-1)
        src = before if self.fault and self.fault[0] == "stale_consumer" else self.ss
        return self._apply(x, src[:n].view(self.B, self.C, 2), silu)

    def launch_colstats(self, y, gamma, beta, silu=False):
        """Producer column pass over the stored y [B, HW, C] (HW % 64 == 0), then gmd_groupnorm_colstats."""
        B, HW, C, G, bk = self.B, self.HW, self.C, self.G, self.bucket
        before = None if self.cs is None else self.cs.clone()
        n = self.produce_buckets(y.reshape(B * HW, C))
        src = before if self.fault and self.fault[0] == "stale_consumer" and before is not None else self.cs
        v = src[:n].view(B, HW // 64, G, C // G // bk, 2).double()
        return self._apply(y, self._scale_shift(v[..., 0].sum((1, 3)), v[..., 1].sum((1, 3)), gamma, beta), silu)
