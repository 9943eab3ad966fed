"""The attention tile-edge sweeps (tests/test_attn_edges_gpu.py) shown to notice, without a GPU: for every case of every table of
tests/attn_cases.py, in float64 only,
  * condition: after the operands are rounded to the kernel's type, every designated key holds >= 0.5 of its designated query's softmax
    mass (attn_cases.role_mass), for all five head dims;
  * must-pass: the float64 result rounded to the output type has zero violations of the bound the GPU test uses;
  * must-fail: each defect of the kind an index slip at a tile edge produces -- applied to the float64 result, no kernel involved --
    breaks that bound, and breaks it IN THE ROW of every query designated to the key the defect touches (stronger than "somewhere").
A defect is judged in the rotations (attn_cases.edge_weighted_qkv) that serve the role it needs; every defect that applies to a case
must have been judged at least once for that case."""
import math

import pytest
import torch

import attn_cases as C
import ip_adapter_ref as R
import parity as P

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
MIN_MASS = 0.5


@pytest.fixture(autouse=True)
def one_thread():
    """Thousands of float64 products of a few hundred rows: a thread pool costs more than it gives at that size (6 x here)."""
    prev = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(prev)


# ---------------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------------
def test_key_table_covers_residues_tile_counts_and_ring_depths():
    assert len(C.K_EDGES) == 61 and len(set(C.K_EDGES)) == 61 and max(C.K_EDGES) == 393
    assert set(range(1, 17)) <= set(C.K_EDGES)
    assert {n % 8 for n in C.K_EDGES} == set(range(8)) and {n % 4 for n in C.K_EDGES} == set(range(4))
    tiles = {math.ceil(n / C.KV) for n in C.K_EDGES}
    assert tiles == set(range(1, 8))
    assert {n // C.KV for n in C.K_EDGES if n % C.KV == 0} == {1, 2, 3, 4, 6}  # exactly full tiles
    assert {t % 2 for t in tiles} == {0, 1} and {t % 3 for t in tiles} == {0, 1, 2}
    for t in (1, 2, 3, 4, 6):  # one key and one 8-key chunk either side of every covered tile edge
        assert {C.KV * t + r for r in (-9, -8, -7, -1, 0, 1, 7, 8, 9)} <= set(C.K_EDGES)
    # the multiples of 8 next to an edge and one key either side, as the issue names them
    assert {63, 64, 65, 127, 129, 191, 192, 193, 56, 72, 120, 136} <= set(C.K_EDGES)


def test_query_table_covers_valid_waves_and_lanes():
    last_block = {(n - 1) % C.QB + 1 for n in C.Q_EDGES}                 # valid queries of the last block
    assert {math.ceil(v / 32) for v in last_block} == {1, 2, 3, 4}      # one to four valid waves
    assert {(v - 1) % 32 + 1 for v in last_block} >= {1, 31, 32}        # a single valid lane, all but one, a full wave
    assert {math.ceil(n / C.QB) for n in C.Q_EDGES} == {1, 2, 3}
    for edge in (32, 64, 96, 128, 160, 256):
        assert {edge - 1, edge, edge + 1} <= set(C.Q_EDGES)


def test_grid_table_covers_every_remainder_of_the_xcd_remap():
    counts = [C.workgroups(*g) for g in C.GRIDS]
    assert sorted(counts) == sorted(set(range(1, 34)) | {63, 64, 65}) and len(counts) == len(set(counts))
    assert {n & 7 for n in counts if n >> 3 == 0} == set(range(1, 8))  # qq = 0: fewer workgroups than XCDs
    assert {n & 7 for n in counts if n >> 3 >= 1} == set(range(8))     # qq >= 1, every rr
    assert {n & 7 for n in counts if n >> 3 >= 2} == set(range(8))
    assert {g[1] for g in C.GRIDS} <= {1, 3, 5, 8, 10, 20} and {5, 8, 10, 20} <= {g[1] for g in C.GRIDS}  # the models' head counts
    assert {g[2] for g in C.GRIDS} == {40, 130, 300}
    assert {b for b, _, _ in C.GRIDS if b > 1} and {h for _, h, _ in C.GRIDS if h > 1}


def test_causal_table_and_edge_keys():
    assert set(C.CAUSAL_N) == {1, 2, 31, 32, 33, 63, 64, 65, 77, 127, 128, 129, 200, 257}
    assert C.edge_keys(1) == [0] and C.edge_keys(64) == [63, 0] and C.edge_keys(65) == [64, 0, 63]
    assert set(C.edge_keys(193)) == {0, 63, 64, 127, 128, 191, 192}
    for Nk in C.K_EDGES:  # Nq = 160 serves every role at once; rows are distinct and reach every wave the role count allows
        _, _, _, roles = C.edge_weighted_qkv(1, 1, 160, Nk, 32, F32, 0)
        rows = [r for _, r, _ in roles]
        assert C.rotations(160, Nk) == 1 and len(set(rows)) == len(rows) and max(rows) == 159
        assert {e for kind, _, e in roles if kind == "key"} == set(C.edge_keys(Nk)) and ("neg" in {kind for kind, _, _ in roles})
        if len(rows) >= 10:
            assert {r // 32 for r in rows} == set(range(5))


# ---------------------------------------------------------------------------------------------------------------------------
# float64 attention with one defect
# ---------------------------------------------------------------------------------------------------------------------------
def _drop(t, j):
    return torch.cat([t[..., :j, :], t[..., j + 1:, :]], -2)


def _pad(t):
    return torch.cat([t, torch.zeros_like(t[..., :1, :])], -2)


def _swap_rows(t, a, b):
    idx = list(range(t.shape[-2]))
    idx[a], idx[b] = b, a
    return t[..., idx, :]


def _attn(q, k, v, causal=False, diag=0):
    """float64 softmax(q k^T / sqrt D) v; causal: row r sees keys 0 .. r + diag (with diag = 1 and a zero-filled key appended by the
    caller, the last row's key r + 1 is that one)."""
    q, k, v = q.double(), k.double(), v.double()
    s = (q @ k.transpose(-1, -2)) * q.shape[-1] ** -0.5
    if causal:
        Nq, Nk = s.shape[-2:]
        s = s.masked_fill(~torch.ones(Nq, Nk, dtype=torch.bool).tril(diag), float("-inf"))
    return torch.softmax(s, -1) @ v


def _rows(roles, kind, key=None):
    return [r for kd, r, e in roles if kd == kind and (key is None or e in key)]


def _must_fail(got, ref, bound, rows, what):
    """The defect must raise, and break the bound in every designated row of every (batch, head)."""
    with pytest.raises(AssertionError, match="outside their bound"):
        P.assert_elementwise(got, ref, bound, what)
    bad = P.violations(got, ref, bound)[0]
    for r in rows:
        assert bool(bad[..., r, :].any(-1).all()), f"{what}: the designated row {r} stays inside its bound for some (batch, head)"


class Judged:
    """Which defects were judged for one case, over its rotations."""

    def __init__(self, what):
        self.what, self.seen = what, set()

    def fail(self, name, got, ref, bound, rows):
        if rows:
            _must_fail(got, ref, bound, rows, f"{self.what}: {name}")
            self.seen.add(name)

    def require(self, names):
        assert set(names) <= self.seen, f"{self.what}: never judged: {sorted(set(names) - self.seen)}"


def _out_dtype(kind, dtype):
    return F32 if kind == "split" else dtype


def _bound(kind, q, k, v, dtype, causal=False):
    scale = q.shape[-1] ** -0.5
    if kind == "split":  # the larger of the two bounds the GPU test uses (plain and pre-split output): a defect caught here is caught by both
        ref, b = P.attention_split_bound(q, k, v, scale)
        return ref, P.presplit_read_bound(ref, b)
    return P.attention_bound(q, k, v, scale, dtype, causal=causal)


def _blocks_differ(Nq, Nk):
    """Two query blocks exist and can be told apart: with ONE key every row of a (batch, head) is v[0], whatever block it sits in."""
    return Nq > C.QB and Nk > 1


def _common_defects(j, ref, bound, roles, Nq, Nk):
    """Outputs that land in the wrong place: every head holds its neighbour's output, every batch its neighbour's (with two: swapped),
    two query blocks swapped."""
    B, H = ref.shape[:2]
    keyrows = _rows(roles, "key")
    if H >= 2:
        j.fail("heads swapped", ref.roll(1, 1), ref, bound, keyrows)
    if B >= 2:
        j.fail("batches swapped", ref.roll(1, 0), ref, bound, keyrows)
    if _blocks_differ(Nq, Nk):
        n = min(C.QB, Nq - C.QB)
        got = ref.clone()
        got[..., :n, :], got[..., C.QB:C.QB + n, :] = ref[..., C.QB:C.QB + n, :], ref[..., :n, :]
        j.fail("query blocks swapped", got, ref, bound, [r for r in keyrows if r < n or C.QB <= r < C.QB + n])


def _judge_plain(kind, B, H, Nq, Nk, D, dtype, seed):
    """One non-causal case of gmd_attention: condition, must-pass and must-fail over all its rotations."""
    what = f"{kind} B={B} H={H} Nq={Nq} Nk={Nk} D={D} {dtype}"
    j = Judged(what)
    for rot in range(C.rotations(Nq, Nk)):
        q, k, v, roles = C.edge_weighted_qkv(B, H, Nq, Nk, D, dtype, seed, rotate=rot)
        mass = C.role_mass(q, k, roles)
        assert min(mass.values()) >= MIN_MASS, f"{what}: designated mass {min(mass.values()):.3f} ({min(mass, key=mass.get)}): raise GAIN[{D}]"
        ref, bound = _bound(kind, q, k, v, dtype)
        assert int(P.violations(ref.to(_out_dtype(kind, dtype)), ref, bound)[0].sum()) == 0, what + ": the rounded reference breaks the bound"
        last, first = Nk - 1, (Nk - 1) // C.KV * C.KV
        j.fail("last key dropped", _attn(q, _drop(k, last), _drop(v, last)), ref, bound, _rows(roles, "key", {last}))
        j.fail("first key of the last tile dropped", _attn(q, _drop(k, first), _drop(v, first)), ref, bound, _rows(roles, "key", {first}))
        j.fail("a zero key beyond Nk admitted", _attn(q, _pad(k), _pad(v)), ref, bound, _rows(roles, "neg"))
        if Nk > C.KV:
            b = first  # the last tile boundary: keys b - 1 | b, edge keys both
            j.fail("V rows across a tile boundary swapped", _attn(q, k, _swap_rows(v, b - 1, b)), ref, bound, _rows(roles, "key", {b - 1, b}))
        _common_defects(j, ref, bound, roles, Nq, Nk)
    need = ["last key dropped", "first key of the last tile dropped", "a zero key beyond Nk admitted"]
    need += ["V rows across a tile boundary swapped"] if Nk > C.KV else []
    need += ["heads swapped"] if H >= 2 else []
    need += ["batches swapped"] if B >= 2 else []
    need += ["query blocks swapped"] if _blocks_differ(Nq, Nk) else []
    j.require(need)


# ---------------------------------------------------------------------------------------------------------------------------
# one test per GPU test
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D", C.HEAD_DIMS)
def test_key_edges_harness_notices(D, dtype):
    for Nk in C.K_EDGES:
        _judge_plain("h16", 1, 2, 160, Nk, D, dtype, seed=1000 * D + Nk)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D", C.HEAD_DIMS)
def test_query_edges_harness_notices(D, dtype):
    for Nq in C.Q_EDGES:
        for Nk in (77, 192):
            _judge_plain("h16", 1, 2, Nq, Nk, D, dtype, seed=1000 * D + 7 * Nq + Nk)


@pytest.mark.parametrize("D", [40, 64, 80, 160])
def test_split_key_edges_harness_notices(D):
    for Nk in C.K_EDGES:
        _judge_plain("split", 1, 4, 160, Nk, D, F32, seed=1000 * D + Nk)


@pytest.mark.parametrize("kernel", ["d32", "d40", "ip40", "split40"])
def test_grid_sweep_harness_notices(kernel):
    D = 32 if kernel == "d32" else 40
    for B, H, Nq in C.GRIDS:
        for dtype in ((F32,) if kernel == "split40" else (BF16, F16)):
            seed = 100 * C.workgroups(B, H, Nq) + D
            if kernel == "ip40":
                _judge_ip(B, H, Nq, 72, 4, D, dtype, 0.6, seed)
            else:
                _judge_plain("split" if kernel == "split40" else "h16", B, H, Nq, 72, D, dtype, seed)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D", [32, 64])
def test_causal_edges_harness_notices(D, dtype):
    for N in C.CAUSAL_N:
        what = f"causal N={N} D={D} {dtype}"
        j = Judged(what)
        for rot in range(C.rotations(N, N, causal=True)):
            q, k, v, roles = C.edge_weighted_qkv(1, 2, N, N, D, dtype, 1000 * D + N, causal=True, rotate=rot)
            mass = C.role_mass(q, k, roles, causal=True)
            assert min(mass.values()) >= MIN_MASS, f"{what}: designated mass {min(mass.values()):.3f} ({min(mass, key=mass.get)}): raise GAIN[{D}]"
            ref, bound = P.attention_bound(q, k, v, D ** -0.5, dtype, causal=True)
            assert int(P.violations(ref.to(dtype), ref, bound)[0].sum()) == 0, what + ": the rounded reference breaks the bound"
            # the diagonal key masked: every row loses its own key (row 0 loses its only one: not finite, which counts)
            j.fail("diagonal key masked", _attn(q, k, v, causal=True, diag=-1), ref, bound, _rows(roles, "key"))
            # key q + 1 admitted; for the last row that is the zero-filled key beyond Nk
            above = _rows(roles, "above") + [r for r in _rows(roles, "neg") if r == N - 1]
            j.fail("key q+1 admitted", _attn(q, _pad(k), _pad(v), causal=True, diag=1), ref, bound, above)
            _common_defects(j, ref, bound, roles, N, N)
        j.require(["diagonal key masked", "key q+1 admitted", "heads swapped"] + (["query blocks swapped"] if N > C.QB else []))


def _judge_ip(B, H, Nq, Nk, Nip, D, dtype, ip_scale, seed):
    what = f"ip B={B} H={H} Nq={Nq} Nk={Nk} Nip={Nip} D={D} {dtype} s={ip_scale}"
    j = Judged(what)
    scale = D ** -0.5
    for rot in range(C.rotations(Nq, Nk, Nip=Nip)):
        q, k, v, kip, vip, roles = C.edge_weighted_qkv(B, H, Nq, Nk, D, dtype, seed, rotate=rot, Nip=Nip)
        mass = C.role_mass(q, k, roles, kip=kip)
        assert min(mass.values()) >= MIN_MASS, f"{what}: designated mass {min(mass.values()):.3f} ({min(mass, key=mass.get)}): raise GAIN[{D}]"
        ref, bound = R.decoupled_bound(q, k, v, kip, vip, scale, ip_scale, dtype)
        assert int(P.violations(ref.to(dtype), ref, bound)[0].sum()) == 0, what + ": the rounded reference breaks the bound"
        last = Nk - 1
        j.fail("last text key dropped", R.decoupled_ref(q, _drop(k, last), _drop(v, last), kip, vip, scale, ip_scale), ref, bound, _rows(roles, "key", {last}))
        j.fail("a zero text key beyond Nk admitted", R.decoupled_ref(q, _pad(k), _pad(v), kip, vip, scale, ip_scale), ref, bound, _rows(roles, "neg"))
        if ip_scale != 0.0:
            j.fail("last image key dropped", R.decoupled_ref(q, k, v, _drop(kip, Nip - 1), _drop(vip, Nip - 1), scale, ip_scale), ref, bound,
                   _rows(roles, "ip", {Nip - 1}))
            if Nip >= 2:
                j.fail("first image key dropped", R.decoupled_ref(q, k, v, _drop(kip, 0), _drop(vip, 0), scale, ip_scale), ref, bound, _rows(roles, "ip", {0}))
            j.fail("a zero image key beyond Nip admitted", R.decoupled_ref(q, k, v, _pad(kip), _pad(vip), scale, ip_scale), ref, bound, _rows(roles, "neg"))
        _common_defects(j, ref, bound, roles, Nq, Nk)
    need = ["last text key dropped", "a zero text key beyond Nk admitted"]
    if ip_scale != 0.0:
        need += ["last image key dropped", "a zero image key beyond Nip admitted"] + (["first image key dropped"] if Nip >= 2 else [])
    need += ["heads swapped"] if H >= 2 else []
    need += ["batches swapped"] if B >= 2 else []
    need += ["query blocks swapped"] if _blocks_differ(Nq, Nk) else []
    j.require(need)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D", C.HEAD_DIMS)
def test_ip_image_key_edges_harness_notices(D, dtype):
    """Every image-key count runs with two consecutive scales of the cycle, so none is left with ip_scale = 0 only."""
    for i, Nip in enumerate(range(1, 65)):
        for s in (C.IP_SCALES[i % 4], C.IP_SCALES[(i + 1) % 4]):
            _judge_ip(1, 2, 160, C.IP_NK[i % 5], Nip, D, dtype, s, seed=1000 * D + Nip)
