"""Helpers of the split-K hand-off tests (test_splitk_handoff_gpu.py, test_splitk_handoff_cpu.py): the launch schedule, the NaN fill
of the scratch, the documented scratch extents (include/gmd_hip.h "WORKSPACE CONTRACT"), the checks themselves, and a toy emulation of
the in-kernel reduction (csrc/gemm.hip: splitk_fixup) with the two faults the checks exist for.  The checks are plain functions of
tensors, so the CPU file can show each of them failing on its fault; they work on any device."""
import torch

# operand set of each launch of a sequence: both transitions (0 -> 1, 1 -> 0), a repeat (1 -> 1), three launches of each set
SCHEDULE = (0, 1, 1, 0, 1, 0)
TAIL_BYTES = 65536  # GMD_WS_TAIL_BYTES
GUARD = 65536       # bytes of guard band before and after a test-owned workspace


def nan_words(n, device="cpu"):
    """n int32 words, every one a float32 quiet NaN (exponent all ones, bit 22 set), payloads varying from word to word and never
    zero in the low bits: no two neighbours equal, nothing a kernel would compute."""
    i = torch.arange(n, device=device, dtype=torch.int64)
    return (0x7FC00000 | ((i * 2654435761 + 12345) & 0x3FFFFE) | 1).to(torch.int32)


def slab_bytes(ks, M, N):
    """Slab extent without the tail: one float32 [M, N] slab per K slice."""
    return ks * M * N * 4


def fragment_bytes(ks, M, N, bm, bn):
    """Fragment extent without the tail: whole accumulator tiles of the slices 0 .. ks-2."""
    tiles = -(-M // bm) * -(-N // bn)
    return (ks - 1) * tiles * bm * bn * 4


def expected_reduction(ks_forced, M, N, bm, bn, ws_bytes, fixup_max=4):
    """(K slices, path, scratch bytes written) a forced-ks 16-bit launch takes with a workspace of ``ws_bytes`` (tail included), by the
    WORKSPACE CONTRACT: unsplit if the slabs do not fit the usable bytes; in-kernel only if the fragments fit as well."""
    usable = max(0, ws_bytes - TAIL_BYTES)
    if ks_forced <= 1 or slab_bytes(ks_forced, M, N) > usable:
        return 1, "unsplit", 0
    frag = fragment_bytes(ks_forced, M, N, bm, bn)
    tiles = -(-M // bm) * -(-N // bn)
    if ks_forced <= fixup_max and frag <= usable and tiles <= TAIL_BYTES // 4:
        return ks_forced, "fixup", frag
    return ks_forced, "slab", slab_bytes(ks_forced, M, N)


def first_mismatch(outs, refs, schedule=SCHEDULE):
    """Index of the first launch whose outputs (a tuple of tensors) are not bit-equal to the reference of ITS operand set, or None.
    NaNs never compare equal: a fragment read before it was written fails here."""
    for i, (o, s) in enumerate(zip(outs, schedule)):
        for got, ref in zip(o, refs[s]):
            if got.shape != ref.shape or got.dtype != ref.dtype or not torch.equal(got, ref):
                return i
    return None


def assert_sequence(outs, refs, what, schedule=SCHEDULE):
    bad = first_mismatch(outs, refs, schedule)
    if bad is not None:
        got, ref = outs[bad][0], refs[schedule[bad]][0]
        nan = int(torch.isnan(got.float()).sum())
        diff = int((got != ref).sum())
        raise AssertionError(f"{what}: launch {bad} of {len(outs)} (operand set {schedule[bad]}, after set "
                             f"{schedule[bad - 1] if bad else 'none'}) differs from its own reference in {diff} elements ({nan} NaN)")


def scratch_violations(before, after, ws_bytes, written_bytes=None, guard=GUARD, tail=TAIL_BYTES):
    """What a launch did to a test-owned allocation [guard | W bytes | guard] (uint8 tensors ``before`` / ``after``) that the
    WORKSPACE CONTRACT forbids, given the workspace_bytes = ``ws_bytes`` <= W it was told: a list of messages, empty = clean.
      * a guard byte changed;            * a byte at offset >= ws_bytes changed;
      * the tail [ws_bytes - tail, ws_bytes) is not all zero;
      * with ``written_bytes``: a byte of the usable region at or beyond the documented extent changed."""
    total = before.numel()
    w = total - 2 * guard
    assert 0 < ws_bytes <= w and after.numel() == total
    changed = before != after
    out = []

    def region(lo, hi, name):
        c = changed[lo:hi]
        if bool(c.any()):
            out.append(f"{int(c.sum())} bytes of {name} changed; first at workspace offset {lo + int(c.nonzero()[0]) - guard}")

    region(0, guard, "the guard band BEFORE the workspace")
    region(guard + w, total, "the guard band AFTER the workspace")
    region(guard + ws_bytes, guard + w, "the bytes at or beyond workspace_bytes")
    t = after[guard + max(0, ws_bytes - tail):guard + ws_bytes]
    if bool(t.any()):
        out.append(f"{int((t != 0).sum())} non-zero bytes in the counter tail; first at tail offset {int(t.nonzero()[0])}")
    if written_bytes is not None:
        region(guard + written_bytes, guard + max(written_bytes, ws_bytes - tail), "the usable bytes beyond the documented scratch extent")
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Toy emulation of splitk_fixup: what the checks above must catch, and what a re-launch of the same inputs cannot see
# ---------------------------------------------------------------------------------------------------------------------------
class FixupEmulation:
    """C = A W^T on tiles of ``t`` x ``t`` with ``ks`` K slices, float32, on a workspace of float32 words followed by one arrival
    counter per tile.  Producers (slices 0 .. ks-2) store their tile's partial product at word (slice * tiles + tile) * t * t and add 1
    to the tile's counter; the finisher (slice ks-1) reads them back, forms (s_0 + s_1 + ..) + own and resets the counter -- the order
    of the slab reduction, which ``reference`` computes without any workspace.

    Faults (``fault`` = (kind, tile, slice) or None):
      "stale":       that tile's finisher reads, for that slice, what the workspace held BEFORE this launch -- the previous launch's
                     fragment still sitting in a cache that the load did not bypass;
      "not_written": that fragment's store lands only after the finisher has read the location."""

    def __init__(self, M=8, N=8, K=12, t=4, ks=3, fault=None):
        assert M % t == 0 and N % t == 0 and K % ks == 0
        self.M, self.N, self.K, self.t, self.ks, self.fault = M, N, K, t, ks, fault
        self.tiles = (M // t) * (N // t)
        self.usable = (ks - 1) * self.tiles * t * t
        self.ws = torch.zeros(self.usable, dtype=torch.float32)
        self.cnt = torch.zeros(self.tiles, dtype=torch.int32)

    def fill(self, kind):
        if kind == "nan":
            self.ws = nan_words(self.usable).view(torch.float32).clone()
        else:
            self.ws.zero_()

    def _partial(self, a, w, tile, s):
        t, kc = self.t, self.K // self.ks
        r, c = divmod(tile, self.N // t)
        return a[r * t:(r + 1) * t, s * kc:(s + 1) * kc] @ w[c * t:(c + 1) * t, s * kc:(s + 1) * kc].T

    def reference(self, a, w):
        out = torch.empty(self.M, self.N, dtype=torch.float32)
        t = self.t
        for tile in range(self.tiles):
            r, c = divmod(tile, self.N // t)
            acc = self._partial(a, w, tile, 0)
            for s in range(1, self.ks - 1):
                acc = acc + self._partial(a, w, tile, s)
            out[r * t:(r + 1) * t, c * t:(c + 1) * t] = acc + self._partial(a, w, tile, self.ks - 1)
        return out

    def launch(self, a, w):
        t, tt = self.t, self.t * self.t
        before = self.ws.clone()
        late = []
        for s in range(self.ks - 1):  # producers
            for tile in range(self.tiles):
                off = (s * self.tiles + tile) * tt
                frag = self._partial(a, w, tile, s).reshape(-1)
                if self.fault == ("not_written", tile, s):
                    late.append((off, frag))
                else:
                    self.ws[off:off + tt] = frag
                self.cnt[tile] += 1
        out = torch.empty(self.M, self.N, dtype=torch.float32)
        for tile in range(self.tiles):  # finishers
            assert int(self.cnt[tile]) == self.ks - 1
            r, c = divmod(tile, self.N // t)
            acc = None
            for s in range(self.ks - 1):
                off = (s * self.tiles + tile) * tt
                src = before if self.fault == ("stale", tile, s) else self.ws
                f = src[off:off + tt].reshape(t, t)
                acc = f.clone() if acc is None else acc + f
            out[r * t:(r + 1) * t, c * t:(c + 1) * t] = acc + self._partial(a, w, tile, self.ks - 1)
            self.cnt[tile] = 0
        for off, frag in late:
            self.ws[off:off + tt] = frag
        return out
