"""CPU: the GEMM launch planner (csrc/gemm_plan.cpp) answers exactly as it did before it became one host-only unit -- every row of
tests/golden/gemm_plan_table.json (plan_table.py) -- and the decisions the C ABI does not expose hold under the sanitizers."""
import json
import os
import shutil
import subprocess
import sys

import pytest

import plan_table

ROOT = plan_table.ROOT
CSRC = os.path.join(ROOT, "gm-diffusion_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from gm_diffusion import _native

    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _native.lib()


@pytest.fixture(scope="module")
def table():
    with open(plan_table.TABLE) as f:
        return json.load(f)


def _mismatches(got, want, label):
    return [f"{label(i)}: got {g} expected {w}" for i, (g, w) in enumerate(zip(got, want)) if g != w]


def test_plan_table_inputs_are_the_censuses_and_the_grid(table):
    """The table covers what it says: every gemm_nt / conv3x3 shape of the two censuses at the three workspaces, and the whole grid."""
    assert table["workspaces"] == list(plan_table.workspaces())
    want = [[*s, w] for s in plan_table.census_shapes() for w in range(3)]
    assert [[*r[:4], tuple(r[4]) if r[4] else None, r[5]] for r in table["census"]] == want and len(want) >= 300
    assert len(table["grid"]) == 12 * 11 * 7 * 2 * 3


def test_census_shapes_plan_as_before(lib, table):
    ws = table["workspaces"]
    got = [plan_table.query(lib, *r[:4], ws[r[5]], r[4]) for r in table["census"]]
    bad = _mismatches(got, [table["answers"][r[6]] for r in table["census"]], lambda i: table["census"][i][:6])
    assert not bad, f"{len(bad)} census rows changed:\n" + "\n".join(bad[:10])


def test_grid_plans_as_before(lib, table):
    inputs = [(s, w) for s in plan_table.grid_shapes() for w in table["workspaces"]]
    got = [plan_table.query(lib, *s[:4], w, None) for s, w in inputs]
    bad = _mismatches(got, [table["answers"][i] for i in table["grid"]], lambda i: inputs[i])
    assert not bad, f"{len(bad)} of {len(inputs)} grid rows changed:\n" + "\n".join(bad[:10])
    assert lib.gmd_gemm_plan_family(-1) == 0  # the queries left the thread's family as they found it


def test_forced_plans_and_fixup_off_in_a_tuning_child(lib, table):
    """gmd_gemm_plan_override (one forced plan per kernel-family code) and gmd_splitk_fixup_max(0) are process-wide state: they are
    exercised in a child process with GMD_TUNING=1, never in this one."""
    env = dict(os.environ, GMD_TUNING="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "plan_table.py"), "--tuning"], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got, want = json.loads(out.stdout), table["tuning"]
    assert got["fixup_prev"] == want["fixup_prev"] == 4
    assert [r[:4] for r in got["forced"]] == [r[:4] for r in want["forced"]] and len(want["forced"]) == 4 * len(plan_table.FORCED)
    bad = _mismatches(got["forced"], want["forced"], lambda i: want["forced"][i][:4]) + _mismatches(got["fixup0"], want["fixup0"], lambda i: f"fixup0 {i}")
    assert not bad, "\n".join(bad[:10])
    # and nothing leaked into this process: overrides are still refused here, the default plan still answers
    if os.environ.get("GMD_TUNING") != "1":
        assert lib.gmd_gemm_plan_override(128, 160, 9, 1) == 3  # GMD_ERR_UNSUPPORTED
    first = table["census"][2]  # (at the default workspace)
    assert plan_table.query(lib, *first[:4], table["workspaces"][first[5]], first[4]) == table["answers"][first[6]]


def test_split_plan_info_names_the_float32_kernels(lib, table):
    """gmd_split_plan_info: every case table of the float32 parity tests (tests/split_cases.py) plans as the tests name it, the K
    slices agree with gmd_split_plan_ksplit and the full-rows predicate with gmd_gemm_out_split_ok over the whole grid, other element
    types are refused -- and in a GMD_TUNING=1 child the override that selects the loader / converter kernel shows as code 244 for
    pre-split weights with a plain activation only."""
    import ctypes

    import split_cases as S
    from gm_diffusion import hip_ops as ops

    def info(code, M, N, K, batch=1, ws=ops.WORKSPACE_BYTES, geglu=0):
        out = (ctypes.c_int * 4)()
        rc = lib.gmd_split_plan_info(code, M, N, K, batch, ws, geglu, ctypes.addressof(out))
        return (rc, *out)

    for name, (M, N, K, (bm, bn, ks)) in {**S.GEMM_CASES, S.SECOND_LAP[0]: S.SECOND_LAP[1:]}.items():
        for code in S.FORM_CODE.values():
            assert info(code, M, N, K) == (0, bm, bn, 0, ks), name
            assert ops.split_plan_info(code, M, N, K) == (bm, bn, 0, ks)
    for tile, (B, ci, co, maps, (bm, bn, ks)) in S.CONV_TILES.items():
        for mode in S.MODES:
            ho, wo = S.conv_inputs(tile, mode)[8:10]
            assert info(4, B * ho * wo, co, 9 * ci) == (0, bm, bn, 0, ks), (tile, mode)
    assert info(3, 128, 72, 128, batch=3) == (0, 64, 64, 0, 1) and info(3, 72, 128, 128, batch=3) == (0, 64, 64, 0, 1)
    assert info(4, 300, 2560, 320, geglu=1) == (0, 64, 64, 0, 1) and info(4, 4096, 2560, 320, geglu=1) == (0, 128, 128, 0, 1)
    for code in (0, 1, 2, 6):
        assert info(code, 4096, 1280, 64)[0] == 1  # GMD_ERR_INVALID
    assert info(4, 4096, 1280, 48)[0] == 1
    for (M, N, K, batch, _), ws in ((s, w) for s in plan_table.grid_shapes() for w in table["workspaces"]):
        rc, bm, bn, code, ks = info(4, M, N, K, batch, ws)
        assert rc == 0 and code == 0 and (bm, bn) in ((128, 160), (128, 128), (64, 64))
        if batch == 1:
            assert ks == lib.gmd_split_plan_ksplit(M, N, K, ws)
            full = bm == 128 and ks == 1 and M % 128 == 0 and N % bn == 0
            assert bool(lib.gmd_gemm_out_split_ok(M, N, K, 0, ws)) == full
        else:
            assert ks == 1
    child = ("import sys, json; sys.path[:0] = [%r, %r]\n"
             "from gm_diffusion import hip_ops as ops\nfrom gm_diffusion._native import lib\n"
             "assert lib().gmd_gemm_plan_override(0, 0, 244, 0) == 0\n"
             "print(json.dumps([ops.split_plan_info(c, *s) for c in (3, 4, 5) for s in ((4100, 1280, 128), (4100, 1288, 128), (4100, 1280, 96), (300, 200, 320))]))\n"
             % (ROOT, os.path.join(ROOT, "gm-diffusion_amd")))
    out = subprocess.run([sys.executable, "-c", child], env=dict(os.environ, GMD_TUNING="1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    ring = [[128, 160, 0, 1], [128, 128, 0, 1], [128, 160, 0, 1], [64, 64, 0, 1]]
    lc = [[128, 160, 244, 1], [128, 128, 244, 1], [128, 160, 0, 1], [64, 64, 0, 1]]  # (fewer than four K steps, 64-row tiles: the ring kernel)
    assert json.loads(out.stdout) == ring + lc + ring
    assert ops.split_plan_info(4, 4100, 1280, 128) == (128, 160, 0, 1)  # nothing leaked into this process


def test_unexposed_planner_decisions_under_sanitizers(tmp_path):
    """tests/gemm_plan_check.cpp + gemm_plan.cpp + gmd_error.cpp, built by the host compiler with AddressSanitizer and
    UndefinedBehaviorSanitizer and run as a program of its own: known answers of pick_tile_group / conv_channel_block / conv_patch_ok /
    split_lc_fits / fixup_plan_ok, and a sweep up to M = 2^31 - 1 and 2^62 workspace bytes (slabs inside the workspace, fragment
    extents below 0xFFFF0000)."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan"]  # (clang links its runtime statically by default)
    exe = str(tmp_path / "gemm_plan_check")
    srcs = [os.path.join(ROOT, "tests", "gemm_plan_check.cpp"), os.path.join(CSRC, "gemm_plan.cpp"), os.path.join(CSRC, "gmd_error.cpp")]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, *srcs, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("GMD_")}  # the planner's own knobs at their defaults
    run = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    print(run.stdout[-2000:])
    assert run.returncode == 0 and "0 failures" in run.stdout and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, (
        run.stdout[-2000:] + run.stderr[-3000:])
