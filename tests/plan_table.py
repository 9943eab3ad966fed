"""The GEMM launch planner as a table: every answer the plan queries of the C ABI give for the shapes of the two shape censuses
and for a grid around the planner's branch points.  ``tests/golden/gemm_plan_table.json`` holds the table of the commit before the
planner moved into csrc/gemm_plan.cpp; tests/test_gemm_plan_cpu.py asserts that the built library still reproduces every row.

No GPU is needed: the queries are host arithmetic.  Regenerate (only when a plan is MEANT to change) with

    python tests/plan_table.py --write           # the default legs
    GMD_TUNING=1 python tests/plan_table.py --tuning   # prints the GMD_TUNING=1 leg (the test runs it in a child process)
"""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gm-diffusion_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

TABLE = os.path.join(ROOT, "tests", "golden", "gemm_plan_table.json")
CENSUSES = ("profiles/r05_gemm_shape_census.jsonl", "profiles/r04_gemm_shape_census.jsonl")

GRID_M = (64, 95, 96, 128, 255, 256, 512, 1024, 2048, 4096, 8192, 32768)
GRID_N = (64, 96, 128, 160, 256, 320, 640, 1280, 2560, 5120, 10240)
GRID_K = (64, 512, 1280, 1536, 5760, 10240, 23040)
GRID_BATCH = (1, 8)
DTYPES = (0, 1, 2, 3, 4, 5)  # GMD_F32, BF16, F16, F32S, F32SW, F32SA
BF16, F16, F32S, F32SW, F32SA = 1, 2, 3, 4, 5


def workspaces():
    from gm_diffusion import hip_ops

    return (0, 64 << 10, hip_ops.WORKSPACE_BYTES)


def census_shapes():
    """[(M, N, K, batch, conv)] of every gemm_nt / conv3x3 row of the censuses; conv = (B, Hin, Win, Cin, Cout) or None."""
    seen, out = set(), []
    for path in CENSUSES:
        for line in open(os.path.join(ROOT, path)):
            try:
                row = json.loads(line)
            except ValueError:
                continue
            kind, key = row.get("kind"), row.get("key")
            if kind == "gemm_nt" and isinstance(key[1], int):  # (the fused feed-forward rows are not plan queries)
                shape = (key[0], key[1], key[2], key[3], None)
            elif kind == "conv3x3":
                B, H, W, cin, cout, tag = key
                ho, wo = (2 * H, 2 * W) if tag == "up" else (((H - 1) // 2 + 1, (W - 1) // 2 + 1) if tag == "s2" else (H, W))
                shape = (B * ho * wo, cout, 9 * cin, 1, (B, H, W, cin, cout))
            else:
                continue
            if shape not in seen:
                seen.add(shape)
                out.append(shape)
    return out


def grid_shapes():
    return [(m, n, k, b, None) for m, n, k, b in itertools.product(GRID_M, GRID_N, GRID_K, GRID_BATCH)]


def plan_info(lib, dtype, M, N, K, batch, ws, geglu):
    out = (ctypes.c_int * 4)()
    rc = lib.gmd_gemm_plan_info(dtype, M, N, K, batch, ws, geglu, ctypes.addressof(out))
    return [rc, *out]


def query(lib, M, N, K, batch, ws, conv):
    """Every answer for one (shape, workspace) under plan family 0, then family 1: a flat list of ints."""
    ans = []
    prev = lib.gmd_gemm_plan_family(-1)
    try:
        for family in (0, 1):
            lib.gmd_gemm_plan_family(family)
            for dtype in (BF16, F16):
                for geglu in (0, 1):
                    ans += plan_info(lib, dtype, M, N, K, batch, ws, geglu)
            for bucket in (10, 8):
                ans += [lib.gmd_gemm_colstats_plan(d, M, N, K, batch, ws, bucket) for d in DTYPES]
            ans.append(lib.gmd_split_plan_ksplit(M, N, K, ws))
            ans += [lib.gmd_gemm_out_split_ok(M, N, K, g, ws) for g in (0, 1)]
            for tokens in (64, 4096):
                if N % 3 == 0 and M % tokens == 0:
                    ans += [lib.gmd_gemm_qkv_vt_ok(d, M, N, K, 2 * N // 3, tokens, ws) for d in (BF16, F16, F32SW, F32SA)]
            if conv:
                B, H, W, cin, cout = conv
                for b, (stride, up) in itertools.product((B, 2 * B), ((1, 0), (2, 0), (1, 1))):
                    ans += [lib.gmd_conv3x3_gn_fusable(d, b, H, W, cin, cout, stride, up, 0, 32, ws) for d in (BF16, F16, F32S, F32SW, F32SA)]
    finally:
        lib.gmd_gemm_plan_family(prev)
    return ans


def default_legs(lib):
    """{"census": [[M, N, K, batch, conv, ws index, answer index] ...], "grid": [answer index ...] in grid_shapes() x workspaces()
    order, "answers": the distinct answer lists}"""
    answers, index = [], {}

    def intern(a):
        if tuple(a) not in index:
            index[tuple(a)] = len(answers)
            answers.append(a)
        return index[tuple(a)]

    ws = workspaces()
    census = [[*s, w, intern(query(lib, *s[:4], ws[w], s[4]))] for s in census_shapes() for w in range(len(ws))]
    grid = [intern(query(lib, *s[:4], w, None)) for s in grid_shapes() for w in ws]
    return {"workspaces": list(ws), "census": census, "grid": grid, "answers": answers}


# ---- the GMD_TUNING=1 leg: process-wide overrides, so only ever in a child process of its own ----
FORCED = (9, 1, 2, 103, 104, 122, 123, 124, 143, 244, 283)  # one per kernel-family code of gmd_gemm_plan_override
TUNING_SHAPES = ((4096, 1280, 1280, 1), (256, 160, 512, 1), (2048, 1280, 11520, 1), (320, 4096, 320, 8))


def tuning_leg(lib):
    assert os.environ.get("GMD_TUNING") == "1"
    ws = workspaces()[-1]
    out = {"forced": [], "fixup0": []}
    for pf in FORCED:
        for bm, bn, ks in ((0, 0, 0), (128, 160, 0), (128, 128, 2), (64, 64, 0)):
            assert lib.gmd_gemm_plan_override(bm, bn, pf, ks) == 0
            out["forced"].append([pf, bm, bn, ks, [query(lib, *s, ws, None) for s in TUNING_SHAPES]])
    assert lib.gmd_gemm_plan_override(0, 0, 0, 0) == 0
    prev = lib.gmd_splitk_fixup_max(0)  # no in-kernel reduction: a split plan can no longer emit column statistics
    out["fixup_prev"] = prev
    out["fixup0"] = [query(lib, m, n, k, 1, ws, None) for m, n, k in ((2048, 1280, 11520), (1024, 1280, 5760), (256, 320, 23040), (4096, 320, 2880))]
    lib.gmd_splitk_fixup_max(prev)
    return out


if __name__ == "__main__":
    from gm_diffusion import _native

    if "--tuning" in sys.argv:
        json.dump(tuning_leg(_native.lib()), sys.stdout)
    elif "--write" in sys.argv:
        table = default_legs(_native.lib())
        table["tuning"] = json.loads(os.popen(f"GMD_TUNING=1 {sys.executable} {os.path.abspath(__file__)} --tuning").read())
        with open(TABLE, "w") as f:
            json.dump(table, f, separators=(",", ":"))
        print(f"wrote {TABLE}: {len(table['census'])} census rows, {len(table['grid'])} grid rows, {len(table['answers'])} distinct answers")
