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
