"""Case tables, the edge-weighted input generator and the hostile operand layout of the attention tile-edge sweeps
(tests/test_attn_edges_cpu.py, tests/test_attn_edges_gpu.py): plain helper module in the style of tests/split_cases.py.  The tables and
the generator are host-only; ``HostileLayout`` and the launchers touch the device and the library and import both lazily.

Why the inputs are weighted: with plain randn operands one key holds ~1 / Nk of a query's softmax mass, so a kernel that drops,
duplicates or admits ONE key at a tile edge moves the output by ~|v| / Nk -- inside the 16-bit rounding bound from a few hundred keys
on.  Here every edge key (key 0, key Nk - 1, the first and the last key of every 64-key tile) is made to DOMINATE one designated
query: ``k[e] = q[r_e] * g sqrt(D) / |q[r_e]|^2`` puts the scaled score of (r_e, e) at exactly g = 8 (before the 16-bit rounding of
k) against scores of ~N(0, 1) for the other keys, which is 0.8 .. 1.0 of the row's mass.  Whatever happens to that key changes row
r_e by ~|v|, at any key count.  One more designated query (the "repelled" one) has a score of about -12 with EVERY key -- all keys
carry +a in the last head-dim coordinate, which every other query leaves at zero, and it carries -a: a zero-filled key admitted
beyond Nk (score 0) takes that row over, while an ordinary row would lose 1 / (Nk + 1) of its mass to it.  (One key of its own is
repelled three times less, so the row's true output is that key's V row -- of size ~1 -- and not an average over Nk of them.)
"""
import math

import torch

KV = 64                              # keys per tile of all four kernels
QB = 128                             # queries per workgroup
HEAD_DIMS = (32, 40, 64, 80, 160)
IP_SCALES = (0.0, 1.0, 0.6, -0.5)    # the four values of tests/test_ip_adapter_gpu.py
IP_NK = (8, 63, 64, 65, 77)

# every residue mod 4 and mod 8, tile counts 1 .. 7 with exactly full 1, 2, 3, 4 and 6 tiles (every count mod 2 and mod 3: the ring depths)
K_EDGES = tuple(sorted(set(range(1, 17)) | {KV * t + r for t in (1, 2, 3, 4, 6) for r in (-9, -8, -7, -1, 0, 1, 7, 8, 9)}))
# wave (32) and query-block (128) edges: the last block has one to four valid waves, its last valid wave 1 .. 32 valid lanes
Q_EDGES = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 255, 256, 257)
CAUSAL_N = (1, 2, 31, 32, 33, 63, 64, 65, 77, 127, 128, 129, 200, 257)

GRID_COUNTS = tuple(range(1, 34)) + (63, 64, 65)  # workgroups per launch: every nwg & 7, with nwg >> 3 == 0 and >= 1
GRID_HEADS = (20, 10, 8, 5, 3, 1)
GRID_NQ = (300, 130, 40)                          # three, two, one query block


def workgroups(B, H, Nq):
    return B * H * ((Nq + QB - 1) // QB)


def _grid_for(n):
    """The (B, H, Nq) of GRID_HEADS x GRID_NQ with B H ceil(Nq / 128) == n and the smallest batch (ties: more heads, more blocks)."""
    best = None
    for H in GRID_HEADS:
        for Nq in GRID_NQ:
            per = H * ((Nq + QB - 1) // QB)
            if n % per == 0 and (best is None or n // per < best[0]):
                best = (n // per, H, Nq)
    return best


GRIDS = tuple(_grid_for(n) for n in GRID_COUNTS)

GAIN = {32: 8.0, 40: 8.0, 64: 8.0, 80: 8.0, 160: 8.0}  # scaled score of an edge key with its designated query, per head dim
REPEL = 12.0                                           # minus the scaled score of the repelled query with every key


def edge_keys(Nk):
    """Key 0, key Nk - 1 and the first and last key of every 64-key tile, most important first: the last key, the first key of the
    last tile, key 0, then the tile edges from the last tile down (the order in which designated queries are handed out)."""
    order = [Nk - 1, (Nk - 1) // KV * KV, 0]
    for t in reversed(range((Nk + KV - 1) // KV)):
        order += [min(t * KV + KV - 1, Nk - 1), t * KV]
    return list(dict.fromkeys(order))


def _noncausal_roles(Nk, Nip):
    roles = [("key", e) for e in edge_keys(Nk)]
    extra = ([("ip", e) for e in dict.fromkeys((Nip - 1, 0))] if Nip else []) + [("neg", None)]
    return roles[:2] + extra + roles[2:]


def rotations(Nq, Nk, causal=False, Nip=0):
    """How many ``rotate`` values edge_weighted_qkv needs before every role had a query of its own.  Non-causal: 1 unless there are
    fewer queries than roles (Nq = 1).  Causal (a key's designated query is the key's own row): 3 -- see edge_weighted_qkv."""
    return 3 if causal else -(-len(_noncausal_roles(Nk, Nip)) // Nq)


def edge_weighted_qkv(B, H, Nq, Nk, D, dtype, seed, causal=False, rotate=0, Nip=0):
    """(q [B, H, Nq, D], k, v [B, H, Nk, D], roles) -- with Nip > 0: (q, k, v, kip, vip [B, H, Nip, D], roles) -- as CPU tensors of
    ``dtype`` holding the values the kernel reads; everything differs per (batch, head); V rows are i.i.d. randn, so two swapped keys
    differ.  ``roles``: tuples (kind, query row, key), the same rows for every (batch, head):
      ("key", r, e)    key e dominates query r: scaled score GAIN[D] before k is rounded;
      ("ip", r, e)     image key e dominates query r in the image branch;
      ("above", r, e)  causal only, r = e - 1: q[r] is a copy of q[e], so key e -- which row r must NOT see -- would dominate it;
      ("neg", r, None) the repelled query: about -REPEL with every key of both branches.
    Non-causal: role i of m sits at query Nq - 1 - floor(i Nq / m): distinct rows spread over all query waves, the last key on the
    last valid lane of the last valid wave.  With fewer queries than roles, ``rotate`` selects which Nq of them are served.
    Causal (Nq == Nk): a key can only dominate a row at or below the diagonal; it dominates ITS OWN row (the diagonal element at every
    tile edge) and, copied into the row above, the first masked element next to it.  rotate = 0: where e - 1 is an edge key itself
    (63 | 64) row e - 1 keeps its own key; rotate = 1: it takes the copy instead; rotate = 2: the LAST row is the repelled query (for
    it the first masked key is the zero-filled one beyond Nk); otherwise the repelled query is a row no other role uses."""
    g = torch.Generator().manual_seed(seed)
    mk = lambda n: torch.randn(B, H, n, D, generator=g, dtype=torch.float64)
    q, k, v = mk(Nq), mk(Nk), mk(Nk)
    kip, vip = (mk(Nip), mk(Nip)) if Nip else (None, None)
    a = math.sqrt(REPEL * math.sqrt(D))  # a * a / sqrt(D) = REPEL
    q[..., D - 1] = 0.0
    roles = []
    if causal:
        assert Nq == Nk and not Nip
        E = set(edge_keys(Nk))
        aligned = set(E)
        if rotate == 1:
            aligned -= {e - 1 for e in E if e - 1 in E}
        if rotate == 2:
            neg = Nk - 1
        else:
            free = [n for n in range(Nk) if n not in E and n + 1 not in E]
            neg = free[len(free) // 2] if free else None
        aligned.discard(neg)
        copies = [(e - 1, e) for e in sorted(aligned) if e >= 1 and e - 1 != neg and e - 1 not in aligned]
        for r, e in copies:
            q[:, :, r] = q[:, :, e]
        roles += [("key", e, e) for e in sorted(aligned)] + [("above", r, e) for r, e in copies]
        if neg is not None:
            roles.append(("neg", neg, None))
    else:
        every = _noncausal_roles(Nk, Nip)
        served = every[rotate * Nq:(rotate + 1) * Nq]
        assert served, f"rotate={rotate}: no role left for Nq={Nq} Nk={Nk}"
        m = len(served)
        roles = [(kind, Nq - 1 - (i * Nq) // m, e) for i, (kind, e) in enumerate(served)]
    for kind, r, _ in roles:
        if kind == "neg":
            q[:, :, r] = 0.1 * q[:, :, r]
            q[:, :, r, D - 1] = -a
    q = q.to(dtype)
    q64 = q.to(torch.float64)
    for kind, r, e in roles:
        if kind in ("key", "ip"):
            qr = q64[:, :, r]
            (k if kind == "key" else kip)[:, :, e] = qr * (GAIN[D] * math.sqrt(D)) / (qr * qr).sum(-1, keepdim=True)
    k[..., D - 1] = a
    if Nip:
        kip[..., D - 1] = a
    for kind, r, _ in roles:  # the repelled row favours ONE key (-REPEL / 3): its output is that key's V row, not a small average
        if kind == "neg":
            k[:, :, (r if causal else Nk - 1) // 2, D - 1] = a / 3
            if Nip:
                kip[:, :, (Nip - 1) // 2, D - 1] = a / 3
    if Nip:
        return q, k.to(dtype), v.to(dtype), kip.to(dtype), vip.to(dtype), roles
    return q, k.to(dtype), v.to(dtype), roles


def role_mass(q, k, roles, causal=False, kip=None):
    """{role: smallest softmax mass over (batch, head)} in float64 from the ROUNDED operands: for "key" / "ip" the mass of the key in
    its designated row (``causal``: over keys 0 .. r), for "above" the mass key e would take in row e - 1 if it were admitted (keys
    0 .. e), for "neg" the mass one zero-filled extra key would take."""
    q64, k64 = q.to(torch.float64), k.to(torch.float64)
    scale = q.shape[-1] ** -0.5
    out = {}
    for kind, r, e in roles:
        kk = kip.to(torch.float64) if kind == "ip" else k64
        s = (q64[:, :, r:r + 1] @ kk.transpose(-1, -2))[:, :, 0] * scale  # [B, H, keys]
        if kind == "neg":
            if causal:
                s = s[..., :r + 1]
            out[(kind, r, e)] = float((1.0 / (1.0 + torch.exp(s).sum(-1))).min())
            continue
        if kind == "above":
            s = s[..., :e + 1]
        elif causal:
            s = s[..., :r + 1]
        out[(kind, r, e)] = float(torch.softmax(s, -1)[..., e].min())
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# device side: the most hostile legal layout, and the raw launches
# ---------------------------------------------------------------------------------------------------------------------------
PAD = 4096  # elements of NaN before every operand buffer (and, with the rows a partial last tile may touch, after it)


def _pad8(n):
    return (n + 7) // 8 * 8


def _nan_rows(t, rows, ld, col, stride, dev):
    """[B, H, N, D] -> (flat NaN buffer, element offset of row 0 / column 0 of batch 0): the heads at columns [col, col + H D) of rows
    [0, N) of a [B][rows][ld] slab with batch stride ``stride`` >= rows ld; every other element is NaN -- rows >= N, row tails,
    batch gaps, PAD elements before and PAD + 64 rows after."""
    B, H, N, D = t.shape
    flat = torch.full((PAD + (B - 1) * stride + rows * ld + KV * ld + PAD,), float("nan"), dtype=t.dtype, device=dev)
    flat.as_strided((B, N, H * D), (stride, ld, 1), PAD + col).copy_(t.permute(0, 2, 1, 3).reshape(B, N, H * D).to(dev))
    return flat


def _nan_vt(t, ld, stride, dev):
    """[B, H, N, D] -> flat NaN buffer holding V^T [B][H D][ld] (batch stride ``stride``) at element PAD: columns >= N are NaN."""
    B, H, N, D = t.shape
    flat = torch.full((PAD + (B - 1) * stride + H * D * ld + KV + PAD,), float("nan"), dtype=t.dtype, device=dev)
    flat.as_strided((B, H * D, N), (stride, ld, 1), PAD).copy_(t.permute(0, 1, 3, 2).reshape(B, H * D, N).to(dev))
    return flat


class HostileLayout:
    """Device operands of one launch in the most hostile layout the ABI allows (include/gmd_hip.h, gmd_attention):
      * Q at column 16 of a buffer wider than H D; K either in the SAME buffer (a fused projection: column 16 + H D + 8, rows =
        max(Nq, Nk)) or in a buffer of its own at column 8;
      * batch strides 40 elements larger than rows x ld;
      * ldvt 16 wider than Nk rounded up to 8, the V^T batch stride 24 larger than H D ldvt;
      * ldo = H D + 8, the output batch stride 16 larger than Nq ldo, inside a Guarded buffer (tests/test_footprint_gpu.py) prefilled
        with NaN; ``tight_out``: ldo = H D, contiguous (what a pre-split output needs);
      * every element the kernel may not use is NaN: K rows >= Nk, V^T columns >= Nk, row tails, batch gaps, the surroundings.
    Image operands (``kip``, ``vip``: gmd_attention_ip) get the same treatment: Kip at column 8 of its own buffer."""

    def __init__(self, q, k, v, dev, shared=False, kip=None, vip=None, tight_out=False):
        from test_footprint_gpu import Guarded

        B, H, Nq, D = q.shape
        Nk, hd, es = k.shape[2], H * D, q.element_size()
        self.shape, self.Nk, self.dtype, self.es = (B, H, Nq, D), Nk, q.dtype, es
        if shared:
            rows, ld = max(Nq, Nk), 16 + hd + 8 + hd + 24
            stride = rows * ld + 40
            self.qbuf = _nan_rows(q, rows, ld, 16, stride, dev)
            self.qbuf.as_strided((B, Nk, hd), (stride, ld, 1), PAD + 16 + hd + 8).copy_(k.permute(0, 2, 1, 3).reshape(B, Nk, hd).to(dev))
            self.kbuf = self.qbuf
            self.q_ptr, self.k_ptr = self.qbuf.data_ptr() + (PAD + 16) * es, self.qbuf.data_ptr() + (PAD + 16 + hd + 8) * es
            self.ldq = self.ldk = ld
            self.sq = self.sk = stride
        else:
            self.ldq, self.ldk = 16 + hd + 24, 8 + hd + 16
            self.sq, self.sk = Nq * self.ldq + 40, Nk * self.ldk + 40
            self.qbuf, self.kbuf = _nan_rows(q, Nq, self.ldq, 16, self.sq, dev), _nan_rows(k, Nk, self.ldk, 8, self.sk, dev)
            self.q_ptr, self.k_ptr = self.qbuf.data_ptr() + (PAD + 16) * es, self.kbuf.data_ptr() + (PAD + 8) * es
        self.ldvt = _pad8(Nk) + 16
        self.svt = hd * self.ldvt + 24
        self.vbuf = _nan_vt(v, self.ldvt, self.svt, dev)
        self.vt_ptr = self.vbuf.data_ptr() + PAD * es
        if kip is not None:
            self.Nip = kip.shape[2]
            self.ldkip, self.ldvtip = 8 + hd + 16, _pad8(self.Nip) + 16
            self.skip, self.svtip = self.Nip * self.ldkip + 40, hd * self.ldvtip + 24
            self.kipbuf, self.vipbuf = _nan_rows(kip, self.Nip, self.ldkip, 8, self.skip, dev), _nan_vt(vip, self.ldvtip, self.svtip, dev)
            self.kip_ptr, self.vtip_ptr = self.kipbuf.data_ptr() + (PAD + 8) * es, self.vipbuf.data_ptr() + PAD * es
        self.ldo = hd if tight_out else hd + 8
        self.so = Nq * self.ldo + (0 if tight_out else 16)
        n_out = (B - 1) * self.so + Nq * self.ldo
        self.guard = Guarded(n_out, q.dtype)
        self.guard.t.fill_(float("nan"))
        self.guard.before = self.guard.buf.clone()
        self.window = torch.zeros(n_out, dtype=torch.bool, device=dev)
        self.window.as_strided((B, Nq, hd), (self.so, self.ldo, 1), 0).fill_(True)

    def out(self):
        """The logical output window as [B, H, Nq, D] (a view of the guarded buffer)."""
        B, H, Nq, D = self.shape
        t = self.guard.t  # (as_strided counts its offset from the start of the storage: the guard band comes first)
        return t.as_strided((B, Nq, H, D), (self.so, self.ldo, D, 1), t.storage_offset()).permute(0, 2, 1, 3)

    def fresh_output(self):
        """Forget what a launch stored: the guarded buffer is NaN again."""
        self.guard.buf.copy_(self.guard.before)

    def assert_footprint(self, what):
        """Every element of the [B, Nq, H D] window is finite (written, and from no poisoned neighbour of an input) and nothing
        outside it changed: pad columns, batch gaps, the guard bands."""
        o = self.out()
        bad = ~torch.isfinite(o.float())
        if bool(bad.any()):
            b, h, r, d = (int(x) for x in bad.nonzero()[0])
            raise AssertionError(f"{what}: {int(bad.sum())} elements of the output window are not finite (never written, or a poisoned "
                                 f"neighbour of an input was used); first at batch {b} head {h} query {r} column {d}")
        self.guard.assert_untouched_outside(self.window, what)


def launch_attention(lay, scale, causal=False, code=None):
    """gmd_attention through the raw C ABI (the wrapper cannot pass an ldo); ``code``: the dtype code (default: that of the operands'
    16-bit type).  Returns the library's status."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    B, H, Nq, D = lay.shape
    return lib().gmd_attention(lay.q_ptr, lay.k_ptr, lay.vt_ptr, lay.guard.t.data_ptr(), ops.dtype_code(lay.dtype) if code is None else code,
                               B, H, D, Nq, lay.Nk, lay.ldq, lay.ldk, lay.ldvt, lay.ldo, lay.sq, lay.sk, lay.svt, lay.so, float(scale),
                               int(bool(causal)), torch.cuda.current_stream().cuda_stream)


def launch_attention_ip(lay, scale, scales, index):
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    B, H, Nq, D = lay.shape
    return lib().gmd_attention_ip(lay.q_ptr, lay.k_ptr, lay.vt_ptr, lay.kip_ptr, lay.vtip_ptr, lay.guard.t.data_ptr(), ops.dtype_code(lay.dtype),
                                  B, H, D, Nq, lay.Nk, lay.Nip, lay.ldq, lay.ldk, lay.ldvt, lay.ldkip, lay.ldvtip, lay.ldo, lay.sq, lay.sk,
                                  lay.svt, lay.skip, lay.svtip, lay.so, float(scale), scales.data_ptr(), int(index),
                                  torch.cuda.current_stream().cuda_stream)
