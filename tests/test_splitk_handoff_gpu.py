"""The split-K hand-off between workgroups of one launch (csrc/gemm.hip: splitk_fixup) and the scratch it runs on.

The bit-identity tests of test_pp_gpu.py re-launch the SAME inputs: a finisher that reads the previous launch's fragment reads the bits
it should have read (tests/test_splitk_handoff_cpu.py shows it on an emulation).  Here every sequence alternates two operand sets,
launch after launch on ONE test-owned workspace without a host synchronisation in between, once on zeroed scratch and once on scratch
pre-filled with NaNs of varying payload, and every output must be bit-equal to the slab-path reference of ITS OWN operand set -- which
itself is checked per element against float64 with the bounds of tests/parity.py.  The second half hands the library workspaces
smaller than the default one inside guard bands and walks workspace_bytes across the two scratch extents of the WORKSPACE CONTRACT
(include/gmd_hip.h).  No tolerance of its own: bit-equality, and parity.py for the float64 leg.

Every case prints ``HANDOFF <kernel> <shape> ks=<n> fill=<zero|nan> launches=<k> ok`` (pytest -s shows it)."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import handoff as H
import parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32

# kernel -> (tile rows, tile columns, code for the override = code gmd_gemm_plan_info reports)
KERNELS = {"pp256x160": (256, 160, 283), "pp256x128": (256, 128, 283), "lc128x160": (128, 160, 244), "lc128x128": (128, 128, 244),
           "lc64x160": (64, 160, 244), "lc64x128": (64, 128, 244)}
FILLS = ("zero", "nan")


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
    torch.cuda.synchronize()
    lib().gmd_gemm_plan_override(0, 0, 0, 0)
    lib().gmd_conv_patch_override(0)
    lib().gmd_splitk_fixup_max(fix)
    if prev is None:
        os.environ.pop("GMD_TUNING", None)
    else:
        os.environ["GMD_TUNING"] = prev


_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_pattern():
    """The NaN pattern (the size of a workspace) lives for this module's tests only."""
    yield
    _CACHE.clear()


def _conv64(x, w, B, H_, W_):
    """float64 stride-1 3 x 3 convolution of [B, H W, Cin] with tap-major weights (test_parity_gpu._conv64)."""
    ci, co = x.shape[-1], w.shape[0]
    y = F.conv2d(x.view(B, H_, W_, ci).permute(0, 3, 1, 2), w.view(co, 3, 3, ci).permute(0, 3, 1, 2), padding=1)
    return y.permute(0, 2, 3, 1).reshape(B, -1, co)


def _pattern(ops):
    """The NaN words of the whole usable region, built once."""
    if "pattern" not in _CACHE:
        _CACHE["pattern"] = H.nan_words((ops.WORKSPACE_BYTES - ops.WS_TAIL_BYTES) // 4, DEV)
    return _CACHE["pattern"]


def _fill(ops, ws, fill):
    """Stream-ordered fill of the usable region; the counter tail is never touched."""
    usable = (ops.WORKSPACE_BYTES - ops.WS_TAIL_BYTES) // 4
    if fill == "nan":
        ws.view(torch.int32)[:usable].copy_(_pattern(ops))
    else:
        ws[:usable].zero_()


def _tail_is_zero(ops, ws):
    return not bool(ws[-(ops.WS_TAIL_BYTES // 4):].view(torch.int32).any())


def _assert_fragment_footprint(ops, ws, frag_bytes, what):
    """After a NaN-filled sequence through the in-kernel reduction: the last word of the documented fragment extent was written (the
    launches did take that path), and no usable word at or beyond it was."""
    words = ws.view(torch.int32)
    pat = _pattern(ops)
    n = frag_bytes // 4
    assert int(words[n - 1]) != int(pat[n - 1]), what + ": the fragment extent's last word was never written (not the in-kernel reduction?)"
    beyond = words[n:pat.numel()] != pat[n:]
    assert not bool(beyond.any()), what + f": {int(beyond.sum())} scratch words beyond the fragment extent changed; first at word {n + int(beyond.nonzero()[0])}"


def _references(ops, launch, sets, ref_ws):
    """Each set's slab-path result on a fresh workspace, a host synchronisation after every launch."""
    from gm_diffusion._native import lib

    torch.cuda.synchronize()
    fix = lib().gmd_splitk_fixup_max(0)
    refs = []
    with ops.workspace_scope(ref_ws):
        for s in sets:
            refs.append(launch(s))
            torch.cuda.synchronize()
    lib().gmd_splitk_fixup_max(fix)
    return refs


def _assert_fixup_on(ks):
    from gm_diffusion._native import lib

    assert lib().gmd_splitk_fixup_max(-1) >= ks, "the in-kernel reduction is switched off for this many slices in this process: nothing to test"


def _sequences(ops, launch, sets, refs, ws, kernel, shape, ks, frag_bytes=None, schedule=H.SCHEDULE):
    for fill in FILLS:
        _fill(ops, ws, fill)
        with ops.workspace_scope(ws):
            outs = [launch(sets[s]) for s in schedule]
        torch.cuda.synchronize()
        what = f"{kernel} {shape} ks={ks} fill={fill}"
        H.assert_sequence(outs, refs, what, schedule)
        assert _tail_is_zero(ops, ws), what + ": the workspace's counter tail is not zero after the sequence"
        if fill == "nan" and frag_bytes is not None:
            _assert_fragment_footprint(ops, ws, frag_bytes, what)
        print(f"HANDOFF {kernel} {shape} ks={ks} fill={fill} launches={len(schedule)} ok")


def _with_stats(y):
    st = getattr(y, "_colstats", None)
    return (y,) if st is None else (y, st[0])


def _gemm_sets(M, N, K, dtype, seed, same_w, rpg=100):
    """Two operand sets: A, bias, residual and row bias always differ, W unless ``same_w``."""
    g = torch.Generator().manual_seed(seed)
    sets = []
    for i in range(2):
        a = torch.randn(M, K, generator=g).to(dtype).to(DEV)
        w = sets[0]["w"] if (i and same_w) else (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dtype).to(DEV)
        sets.append(dict(a=a, w=w, bias=torch.randn(N, generator=g).to(DEV), res=torch.randn(M, N, generator=g).to(dtype).to(DEV),
                         rb=torch.randn((M + rpg - 1) // rpg, N, generator=g).to(DEV), rpg=rpg))
    return sets


def _launch_bias_residual(ops, colstats=False):
    return lambda s: _with_stats(ops.gemm_nt(s["a"], s["w"], bias=s["bias"], residual=s["res"], colstats=colstats))


def _launch_f32_rowbias(ops):
    return lambda s: (ops.gemm_nt(s["a"], s["w"], bias=s["bias"], rowbias=s["rb"], rows_per_group=s["rpg"], out_dtype=F32),)


def _check_gemm_refs(refs, sets, what, tile, f32_rowbias=False):
    """Each reference per element against float64: gemm_bound with mfma_height(K, 32, 16), as test_parity_gpu._check_gemm."""
    for i, (r, s) in enumerate(zip(refs, sets)):
        a, w = s["a"], s["w"]
        M, K = a.shape
        ref_acc = a.double() @ w.double().T
        abs_dot = a.double().abs() @ w.double().abs().T
        h = P.mfma_height(K, 32, 16)
        if f32_rowbias:
            ex = [s["bias"].double().expand_as(ref_acc), s["rb"].double().repeat_interleave(s["rpg"], 0)[:M]]
            bound = P.gemm_bound(ref_acc, abs_dot, K, F32, 1.0, ex, height=h)
        else:
            ex = [s["bias"].double().expand_as(ref_acc), s["res"].double()]
            bound = P.gemm_bound(ref_acc, abs_dot, K, a.dtype, 1.0, ex, height=h)
        P.assert_elementwise(r[0], ref_acc + ex[0] + ex[1], bound, f"{what} slab reference of set {i}", tile)


# ---------------------------------------------------------------------------------------------------------------------------
# 1a. alternating inputs, back to back, one workspace
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_gemm_alternating_operand_sets_on_one_workspace(kernel, dtype, force_plan):
    """Forced (tile, kernel, K slices): the ragged shape 1000 x N x 640 (10 K steps) with 2, 3 and 4 slices (4: a shorter last slice;
    the ragged last row tile leaves through the register epilogue), full tiles 1024 x 4 bn x 1280 with 4 slices (row epilogue, with
    column statistics where the plan can emit them), bias + residual; and bias + row bias with a float32 store.  X0, X1, X1, X0, X1, X0."""
    from gm_diffusion import hip_ops as ops

    bm, bn, pf = KERNELS[kernel]
    n_ragged = 328 if pf != 244 else 3 * bn  # the 244 kernel's cases keep N on tile boundaries
    ws, ref_ws = ops.new_workspace(torch.device(DEV)), ops.new_workspace(torch.device(DEV))
    cases = [("ragged", 1000, n_ragged, 640, 2, "res"), ("ragged", 1000, n_ragged, 640, 3, "res"), ("ragged", 1000, n_ragged, 640, 4, "res"),
             ("full", 1024, 4 * bn, 1280, 4, "res+colstats"), ("ragged-f32-rowbias", 1000, n_ragged, 640, 3, "f32")]
    for name, M, N, K, ks, epi in cases:
        sets = _gemm_sets(M, N, K, dtype, seed=M + N + K + ks, same_w=(ks == 2))
        force_plan(bm, bn, pf, ks)
        assert ops.gemm_plan_info(dtype, M, N, K) == (bm, bn, pf, ks), f"{kernel} {name}: the override did not select the kernel"
        _assert_fixup_on(ks)
        launch = _launch_f32_rowbias(ops) if epi == "f32" else _launch_bias_residual(ops)
        refs = _references(ops, launch, sets, ref_ws)
        shape = f"{name}-{M}x{N}x{K}-{str(dtype).split('.')[-1]}"
        _check_gemm_refs(refs, sets, f"{kernel} {shape} ks={ks}", (bm, bn), f32_rowbias=epi == "f32")
        if epi.endswith("colstats"):
            # The slab path cannot emit column statistics (they come out of the finisher's row epilogue), so their reference is a
            # quiet launch of the in-kernel path -- fresh workspace, host synchronisation -- whose OUTPUT must be the slab path's bits.
            # The statistics leg is therefore SELF-REFERENTIAL: busy launches against a quiet launch of the same path, never against
            # independent sums of the stored output (test_groupnorm_from_producer_colstats_per_element checks their values).  That is
            # what a hand-off test needs: a stale or early fragment changes the sums the finisher forms.
            from gm_diffusion._native import lib

            can = N % ops.COLSTATS_BUCKET == 0 and bool(lib().gmd_gemm_colstats_plan(ops.dtype_code(dtype), M, N, K, 1, ops.WORKSPACE_BYTES, ops.COLSTATS_BUCKET))
            assert can == (bm >= 128 and bn == 160), "the column-statistics plan rule moved: re-pick which kernels this case covers"
            launch = _launch_bias_residual(ops, colstats=True)
            quiet = []
            with ops.workspace_scope(ref_ws):
                for s_ in sets:
                    quiet.append(launch(s_))
                    torch.cuda.synchronize()
            for q, r in zip(quiet, refs):
                assert (len(q) == 2) == can, "gmd_gemm_colstats_plan and the wrapper disagree"
                assert torch.equal(q[0], r[0]), f"{kernel} {shape}: the quiet in-kernel launch differs from the slab path"
            refs = quiet
        _sequences(ops, launch, sets, refs, ws, kernel, shape, ks, frag_bytes=H.fragment_bytes(ks, M, N, bm, bn))


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("M,N,K,family", [(2048, 1280, 1280, 1), (1024, 1280, 5120, 0)])
def test_gemm_alternating_operand_sets_default_policy(M, N, K, family, dtype):
    """Nothing forced: the co-running family's 256-row ping-pong tiles with K slices, and the launch-by-launch family's loader /
    consumer kernel with K slices -- what the pipelines run."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    ws, ref_ws = ops.new_workspace(torch.device(DEV)), ops.new_workspace(torch.device(DEV))
    sets = _gemm_sets(M, N, K, dtype, seed=M + K + family, same_w=False)
    with ops.plan_family(family):
        bm, bn, code, ks = ops.gemm_plan_info(dtype, M, N, K)
        assert code == (283 if family else 244) and 2 <= ks <= lib().gmd_splitk_fixup_max(-1), (bm, bn, code, ks)
        launch = _launch_bias_residual(ops)
        refs = _references(ops, launch, sets, ref_ws)
        _assert_fixup_on(ks)
        kernel = f"default-family{family}-{bm}x{bn}/{code}"
        shape = f"{M}x{N}x{K}-{str(dtype).split('.')[-1]}"
        _check_gemm_refs(refs, sets, f"{kernel} {shape}", (bm, bn))
        _sequences(ops, launch, sets, refs, ws, kernel, shape, ks, frag_bytes=H.fragment_bytes(ks, M, N, bm, bn))


# ---------------------------------------------------------------------------------------------------------------------------
# 1b. convolutions
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("kernel,patch,Hh,Ww", [("pp256x160", 0, 23, 20), ("pp256x160", 1, 16, 16), ("pp256x160", 2, 16, 16), ("lc128x160", 0, 23, 20)])
def test_conv3x3_alternating_operand_sets_on_one_workspace(kernel, patch, Hh, Ww, dtype, force_plan):
    """Batch 3, 128 -> 320, two K slices (<= Cin / 64, which the patch-resident kernels require); bias + per-sample row bias + residual.
      * 23 x 20 (test_conv3x3_every_kernel_per_element's shape: ragged B Ho Wo): the per-tap ping-pong kernel (patch mode 0) and the
        loader / consumer kernel.  The patch-resident kernels do NOT take this shape, whatever the mode: conv_patch_ok (csrc/gemm.hip)
        wants a power-of-two width and 256-pixel tiles of whole image rows.
      * 16 x 16 (one image per 256-row tile: 3 row tiles x 2 column tiles): the patch-resident kernels, ping-pong (mode 1) and
        continuous (mode 2) consumers.  gmd_gemm_plan_info reports the same plan for them as for the per-tap kernel, so that they ran
        is shown by their result: their K order differs, so a float32 store of the same operands is not bit-equal to mode 0's."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    bm, bn, pf = KERNELS[kernel]
    B, ci, co, ks = 3, 128, 320, 2
    M = B * Hh * Ww
    same_w = kernel == "pp256x160" and patch == 0  # one case with shared weights; every family has one with distinct weights
    g = torch.Generator().manual_seed(21 + patch)
    sets = []
    for i in range(2):
        sets.append(dict(x=torch.randn(B, Hh * Ww, ci, generator=g).to(dtype).to(DEV),
                         w=sets[0]["w"] if (i and same_w) else (torch.randn(co, 9 * ci, generator=g) * 0.03).to(dtype).to(DEV),
                         b=torch.randn(co, generator=g).to(DEV), tb=torch.randn(B, co, generator=g).to(DEV),
                         r=torch.randn(B, Hh * Ww, co, generator=g).to(dtype).to(DEV)))
    force_plan(bm, bn, pf, ks)
    assert ops.gemm_plan_info(dtype, M, co, 9 * ci) == (bm, bn, pf, ks)
    _assert_fixup_on(ks)
    if patch:  # the patch-resident kernel is what runs: not the per-tap kernel's bits
        s0 = sets[0]
        raw = {}
        for mode in (0, patch):
            assert lib().gmd_conv_patch_override(mode) == 0
            raw[mode] = ops.conv3x3(s0["x"], s0["w"], B, Hh, Ww, bias=s0["b"], out_dtype=F32)[0]
        torch.cuda.synchronize()
        assert bool(torch.isfinite(raw[patch]).all())
        assert not torch.equal(raw[0], raw[patch]), (f"patch mode {patch} gives the per-tap kernel's bits on {Hh} x {Ww}: the patch-resident kernel did not run "
                                                     "(conv_patch_ok moved? re-pick the shape)")
    assert lib().gmd_conv_patch_override(patch) == 0
    launch = lambda s: (ops.conv3x3(s["x"], s["w"], B, Hh, Ww, bias=s["b"], rowbias=s["tb"], residual=s["r"])[0],)
    ws, ref_ws = ops.new_workspace(torch.device(DEV)), ops.new_workspace(torch.device(DEV))
    refs = _references(ops, launch, sets, ref_ws)
    for i, (r, s) in enumerate(zip(refs, sets)):
        ref_acc = _conv64(s["x"].double(), s["w"].double(), B, Hh, Ww)
        abs_dot = _conv64(s["x"].double().abs(), s["w"].double().abs(), B, Hh, Ww)
        ex = [s["b"].double().expand_as(ref_acc), s["tb"].double()[:, None, :].expand_as(ref_acc), s["r"].double()]
        P.assert_elementwise(r[0].reshape(M, co), (ref_acc + ex[0] + ex[1] + ex[2]).reshape(M, co),
                             P.gemm_bound(ref_acc, abs_dot, 9 * ci, dtype, 1.0, ex).reshape(M, co), f"conv {kernel} patch {patch} slab reference of set {i}", (bm, bn))
    shape = f"conv-{B}x{Hh}x{Ww}-{ci}to{co}-patch{patch}-{str(dtype).split('.')[-1]}"
    _sequences(ops, launch, sets, refs, ws, kernel if not patch else f"{kernel}-patch-resident", shape, ks, frag_bytes=H.fragment_bytes(ks, M, co, bm, bn))


# ---------------------------------------------------------------------------------------------------------------------------
# 1c / 1e. mixed shapes on one workspace, eagerly and from a captured graph with changing inputs
# ---------------------------------------------------------------------------------------------------------------------------
def _mixed(ops, force_plan, kernel, dtype):
    """P = the full-tile shape with 4 slices, Q = the ragged shape with 2: fragment offsets and counter indices overlap."""
    bm, bn, pf = KERNELS[kernel]
    n_ragged = 328 if pf != 244 else 3 * bn
    shp = {"P": (1024, 4 * bn, 1280, 4), "Q": (1000, n_ragged, 640, 2)}
    sets = {k: _gemm_sets(M, N, K, dtype, seed=M + N + K + 7, same_w=False) for k, (M, N, K, ks) in shp.items()}

    _assert_fixup_on(4)

    def run(which, s, out=None):
        M, N, K, ks = shp[which]
        force_plan(bm, bn, pf, ks)
        assert ops.gemm_plan_info(dtype, M, N, K) == (bm, bn, pf, ks)
        return ops.gemm_nt(s["a"], s["w"], bias=s["bias"], residual=s["res"], out=out)

    return shp, sets, run


def _mixed_references(ops, shp, sets, run, what, tile):
    ref_ws = ops.new_workspace(torch.device(DEV))
    refs = {}
    for which in shp:
        refs[which] = _references(ops, lambda s: (run(which, s),), sets[which], ref_ws)
        _check_gemm_refs(refs[which], sets[which], f"{what} {which}", tile)
    return refs


@pytest.mark.parametrize("kernel", ["pp256x160", "lc128x160", "lc64x128"])
def test_mixed_shapes_share_one_workspace(kernel, force_plan):
    from gm_diffusion import hip_ops as ops

    shp, sets, run = _mixed(ops, force_plan, kernel, BF16)
    refs = _mixed_references(ops, shp, sets, run, f"mixed {kernel}", KERNELS[kernel][:2])
    ws = ops.new_workspace(torch.device(DEV))
    order = [("P", 0), ("Q", 0), ("P", 1), ("Q", 1)]
    for fill in FILLS:
        _fill(ops, ws, fill)
        with ops.workspace_scope(ws):
            outs = [run(which, sets[which][i]) for which, i in order]
        torch.cuda.synchronize()
        for n, ((which, i), y) in enumerate(zip(order, outs)):
            assert torch.equal(y, refs[which][i][0]), f"mixed {kernel} fill={fill}: launch {n} ({which}, operand set {i}) differs from its own reference"
        assert _tail_is_zero(ops, ws), f"mixed {kernel} fill={fill}: counter tail"
        print(f"HANDOFF {kernel} mixed-P{'x'.join(map(str, shp['P'][:3]))}-Q{'x'.join(map(str, shp['Q'][:3]))} ks=4+2 fill={fill} launches={len(order)} ok")


@pytest.mark.parametrize("beside", [False, True])
def test_graph_replay_with_changing_inputs(beside, force_plan):
    """The four launches of the mixed case captured into ONE graph that reads static input buffers; before each of 6 replays the other
    operand set is copied into them on the replay stream.  ``beside``: a second stream issues the same launches on a workspace of its
    own meanwhile (the arrangement of test_splitk_fixup_under_a_second_streams_load)."""
    from gm_diffusion import hip_ops as ops

    kernel = "pp256x160"
    shp, sets, run = _mixed(ops, force_plan, kernel, BF16)
    refs = _mixed_references(ops, shp, sets, run, f"graph {kernel}", KERNELS[kernel][:2])
    # two slots of static buffers: the graph is P(slot 0), Q(slot 0), P(slot 1), Q(slot 1), and every replay gets operand set i in
    # slot 0 and the other one in slot 1 -- the operands change inside a replay and between replays
    static = [{k: {n: t.clone() for n, t in sets[k][0].items() if torch.is_tensor(t)} for k in shp} for _ in range(2)]
    order = [("P", 0), ("Q", 0), ("P", 1), ("Q", 1)]
    ws = ops.new_workspace(torch.device(DEV))
    _fill(ops, ws, "nan")
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with ops.workspace_scope(ws), torch.cuda.graph(gr):
        g_outs = [run(which, static[slot][which]) for which, slot in order]
    side = ops.side_stream(DEV) if beside else None
    ws2 = ops.new_workspace(torch.device(DEV)) if beside else None
    clones = []
    for it in range(6):
        i = H.SCHEDULE[it]
        if beside:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), ops.workspace_scope(ws2):
                for which, slot in order:
                    run(which, sets[which][slot])
        for slot in range(2):
            for k in shp:
                for n, t in static[slot][k].items():
                    t.copy_(sets[k][i ^ slot][n])
        gr.replay()
        clones.append((i, [y.clone() for y in g_outs]))
    torch.cuda.synchronize()
    for it, (i, ys) in enumerate(clones):
        for n, ((which, slot), y) in enumerate(zip(order, ys)):
            assert torch.equal(y, refs[which][i ^ slot][0]), (f"graph replay {it}, launch {n} ({which}, operand set {i ^ slot}): differs from the eager "
                                                              "reference of its set")
    for t in (ws, ws2):
        assert t is None or _tail_is_zero(ops, t)
    print(f"HANDOFF {kernel} graph-mixed{'-beside-a-second-stream' if beside else ''} ks=4+2 fill=nan launches={4 * 6} ok")


# ---------------------------------------------------------------------------------------------------------------------------
# 1d. slab consumers that read across a launch boundary
# ---------------------------------------------------------------------------------------------------------------------------
SPLIT_SHAPE = (256, 640, 2560)


def _split_sets(M, N, K, ops):
    g = torch.Generator().manual_seed(M + N + K)
    sets = []
    for _ in range(2):
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV)
        sets.append(dict(a=torch.randn(M, K, generator=g).to(DEV), w=w, weff=ops.scale_weight(w), ws=ops.split_weights(w), bias=torch.randn(N, generator=g).to(DEV)))
    return sets


def test_float32_split_slab_reduction_alternating_operand_sets():
    """csrc/gemm_split.hip: slabs + splitk_reduce_f32_kernel, a second launch that reads what the first one wrote."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    M, N, K = SPLIT_SHAPE
    ks = lib().gmd_split_plan_ksplit(M, N, K, ops.WORKSPACE_BYTES)
    assert ks > 1, "the float32 planner no longer splits this shape: re-pick it"
    with ops.f32_mode_scope("split"):
        sets = _split_sets(M, N, K, ops)
        launch = lambda s: (ops.gemm_nt(s["a"], s["ws"], bias=s["bias"]),)
        assert ops._contract_code(sets[0]["a"], sets[0]["ws"], K) == ops.GMD_F32SW
        ws, ref_ws = ops.new_workspace(torch.device(DEV)), ops.new_workspace(torch.device(DEV))
        refs = []
        with ops.workspace_scope(ref_ws):
            for s in sets:
                refs.append(launch(s))
                torch.cuda.synchronize()
        for i, (r, s) in enumerate(zip(refs, sets)):
            a, weff = s["a"], s["weff"]
            ref_acc, ad = a.double() @ weff.double().T, a.double().abs() @ weff.double().abs().T
            ex = [s["bias"].double().expand(M, N)]
            bound = P.gemm_bound(ref_acc, ad, 3 * K, F32, weff._alpha, ex, product_err=P.split_product_bound(a, weff), height=P.mfma_height(3 * K, 32, 16))
            P.assert_elementwise(r[0], weff._alpha * ref_acc + ex[0], bound, f"float32 split quiet reference of set {i}", (64, 64))
        _sequences(ops, launch, sets, refs, ws, "f32split-slab", f"{M}x{N}x{K}", ks)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("B", [2, 8])
def test_conv3x3_groupnorm_over_slabs_alternating_operand_sets(B, dtype):
    """conv3x3_groupnorm on an 8 x 8 level, 1280 -> 1280, 32 groups.  gmd_conv3x3_gn_fusable admits the fused launch (the GroupNorm
    kernel sums the convolution's split-K slabs) from B x groups >= 256 on, so batch 8 is the smallest that takes it; batch 2 is
    asserted NOT to fuse and runs the other slab consumer instead: 16 slabs of the ring kernel summed by splitk_reduce_kernel, then
    GroupNorm.  Both read in a later launch what an earlier one wrote."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    Hh, ci, co, G = 8, 1280, 1280, 32
    fused = bool(lib().gmd_conv3x3_gn_fusable(ops.dtype_code(dtype), B, Hh, Hh, ci, co, 1, 0, 0, G, ops.WORKSPACE_BYTES))
    assert fused == (B * G >= 256), "the fusion rule moved: re-pick the batch sizes so that the fused launch stays covered"
    ks = ops.gemm_plan_info(dtype, B * Hh * Hh, co, 9 * ci)[3]
    assert ks > 1 and (fused or ks > lib().gmd_splitk_fixup_max(-1)), "slabs are not what this launch reduces through"
    g = torch.Generator().manual_seed(B * 1000 + Hh + ci)
    sets = []
    for _ in range(2):
        sets.append(dict(x=torch.randn(B, Hh * Hh, ci, generator=g).to(DEV, dtype), w=(torch.randn(co, 9 * ci, generator=g) / math.sqrt(9 * ci)).to(DEV, dtype),
                         bias=torch.randn(co, generator=g).to(DEV), tb=torch.randn(B, co, generator=g).to(DEV),
                         res=torch.randn(B, Hh * Hh, co, generator=g).to(DEV, dtype), gamma=torch.randn(co, generator=g).to(DEV), beta=torch.randn(co, generator=g).to(DEV)))
    launch = lambda s: ops.conv3x3_groupnorm(s["x"], s["w"], B, Hh, Hh, G, s["gamma"], s["beta"], 1e-5, silu=True, bias=s["bias"], rowbias=s["tb"],
                                             residual=s["res"], want_raw=True)
    ws, ref_ws = ops.new_workspace(torch.device(DEV)), ops.new_workspace(torch.device(DEV))
    refs = []
    with ops.workspace_scope(ref_ws):
        for s in sets:
            refs.append(launch(s))
            torch.cuda.synchronize()
    for i, (r, s) in enumerate(zip(refs, sets)):  # the raw tensor per element, as test_conv3x3_groupnorm_per_element
        ref_acc = _conv64(s["x"].double(), s["w"].double(), B, Hh, Hh)
        abs_dot = _conv64(s["x"].double().abs(), s["w"].double().abs(), B, Hh, Hh)
        ex = [s["bias"].double().expand_as(ref_acc), s["tb"].double()[:, None, :].expand_as(ref_acc), s["res"].double()]
        P.assert_elementwise(r[0].reshape(-1, co), (ref_acc + ex[0] + ex[1] + ex[2]).reshape(-1, co),
                             P.gemm_bound(ref_acc, abs_dot, 9 * ci, dtype, 1.0, ex).reshape(-1, co), f"conv3x3_groupnorm quiet Yraw of set {i}", (64, 64))
        ref, bound = P.groupnorm_ref_bound(r[0], G, s["gamma"], s["beta"], 1e-5, dtype, -(-Hh * Hh * (co // G) // 256) + 16, True)
        P.assert_elementwise(r[1], ref, bound, f"conv3x3_groupnorm quiet Ynorm of set {i}", (64, 8))
    _sequences(ops, launch, sets, refs, ws, "conv3x3_groupnorm-slab" if fused else "conv3x3-slab+groupnorm", f"{B}x{Hh}x{Hh}-{ci}to{co}-{str(dtype).split('.')[-1]}", ks)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. workspace footprint: [64 KiB guard | W bytes | 64 KiB guard], workspace_bytes = W' <= W
# ---------------------------------------------------------------------------------------------------------------------------
class GuardedWorkspace:
    """One allocation of the test's own.  ``arm(wp)``: guards = the byte pattern of test_footprint_gpu.Guarded, all W bytes = the NaN
    words, then the tail of the first ``wp`` bytes zeroed; ``ptr`` is the workspace pointer to hand over with workspace_bytes = wp."""

    def __init__(self, w_bytes):
        assert w_bytes % 4 == 0
        self.w = w_bytes
        total = 2 * H.GUARD + w_bytes
        self.pattern = ((torch.arange(total, device=DEV, dtype=torch.int64) * 131 + 89) % 251).to(torch.uint8)
        self.pattern[H.GUARD:H.GUARD + w_bytes] = H.nan_words(w_bytes // 4, DEV).view(torch.uint8)
        self.buf = torch.empty_like(self.pattern)
        self.ptr = self.buf.data_ptr() + H.GUARD
        assert self.ptr % 16 == 0

    def arm(self, wp):
        assert H.TAIL_BYTES < wp <= self.w and wp % 4 == 0
        self.buf.copy_(self.pattern)
        self.buf[H.GUARD + wp - H.TAIL_BYTES:H.GUARD + wp].zero_()
        self.before = self.buf.clone()

    def check(self, wp, written_bytes, what):
        v = H.scratch_violations(self.before, self.buf, wp, written_bytes=written_bytes)
        assert not v, what + ": " + "; ".join(v)
        if written_bytes:  # the path the contract names did run: the last word of its extent was written
            last = slice(H.GUARD + written_bytes - 4, H.GUARD + written_bytes)
            assert not torch.equal(self.buf[last], self.before[last]), what + ": the last word of the documented scratch extent was never written"


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("kernel,ks", [("pp256x160", 2), ("lc128x160", 2), ("pp256x160", 4)])
def test_gemm_scratch_stays_inside_the_workspace_it_was_given(kernel, ks, force_plan):
    """The ragged shape of the alternating test, forced K slices, bf16, bias + residual, gmd_gemm_nt called directly with
    workspace_bytes = W' and gmd_gemm_plan_info asked with the same W'.  W' walks the documented extents (tail included): roomy; the
    slab extent and 4 bytes below it (below: the plan must report one slice); the fragment extent and 4 bytes below it; between the
    two.  With TWO slices of this shape the fragment extent lies BELOW the slab extent on every kernel (tiles bm bn < 2 M N), so the
    window "slabs fit, fragments do not" is empty and W' at / under the fragment extent are further unsplit cases; with FOUR slices
    on 256 x 160 tiles it is not (3 x 12 tiles x 160 KB > 4 M N 4 bytes): that case takes the slab fall-back with the in-kernel
    reduction switched on."""
    import ctypes

    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    bm, bn, pf = KERNELS[kernel]
    M, K = 1000, 640
    N = 328 if pf != 244 else 3 * bn
    s = _gemm_sets(M, N, K, BF16, seed=M + N + K, same_w=False)[0]
    a, w, bias, res = s["a"], s["w"], s["bias"], s["res"]
    T = H.TAIL_BYTES
    slab_ext, frag_ext = H.slab_bytes(ks, M, N) + T, H.fragment_bytes(ks, M, N, bm, bn) + T
    sizes = {"roomy": max(slab_ext, frag_ext) + (1 << 20), "slab-extent": slab_ext, "slab-extent-4": slab_ext - 4, "fragment-extent": frag_ext,
             "fragment-extent-4": frag_ext - 4, "half-the-slab-extent": (slab_ext // 2) // 16 * 16}
    if frag_ext - slab_ext >= 16:
        sizes["between"] = (slab_ext + frag_ext) // 2 // 4 * 4
    assert ("between" in sizes) == (ks == 4), "the shapes moved: re-derive which case has a window between the extents"
    gw = GuardedWorkspace(sizes["roomy"] + (1 << 20))
    fixup_max = lib().gmd_splitk_fixup_max(-1)
    # the same launch on the default workspace, split and unsplit; the float64 leg for the unsplit one
    force_plan(bm, bn, pf, ks)
    assert ops.gemm_plan_info(BF16, M, N, K) == (bm, bn, pf, ks)
    plain = {ks: ops.gemm_nt(a, w, bias=bias, residual=res)}
    force_plan(bm, bn, pf, 1)
    plain[1] = ops.gemm_nt(a, w, bias=bias, residual=res)
    force_plan(bm, bn, pf, ks)
    ref_acc, abs_dot = a.double() @ w.double().T, a.double().abs() @ w.double().abs().T
    ex = [bias.double().expand_as(ref_acc), res.double()]
    bound = P.gemm_bound(ref_acc, abs_dot, K, BF16, 1.0, ex, height=P.mfma_height(K, 32, 16))
    seen = set()
    for name, wp in sizes.items():
        exp_ks, path, written = H.expected_reduction(ks, M, N, bm, bn, wp, fixup_max)
        plan = (ctypes.c_int * 4)()
        assert lib().gmd_gemm_plan_info(ops.GMD_BF16, M, N, K, 1, wp, 0, ctypes.addressof(plan)) == 0
        what = f"{kernel} ks={ks} W'={name} ({wp} bytes: {path})"
        assert tuple(plan) == (bm, bn, pf, exp_ks), what + f": the plan query reports {tuple(plan)}"
        gw.arm(wp)
        out = torch.full((M, N), float("nan"), dtype=BF16, device=DEV)
        rc = lib().gmd_gemm_nt(a.data_ptr(), w.data_ptr(), out.data_ptr(), ops.GMD_BF16, ops.GMD_BF16, M, N, K, K, K, N, 1, 0, 0, M * N, bias.data_ptr(), None, 0, 0,
                               res.data_ptr(), N, 0, 1.0, ops.ACT_NONE, None, 0, gw.ptr, wp, _stream())
        assert rc == 0, lib().gmd_last_error()
        torch.cuda.synchronize()
        gw.check(wp, written, what)
        assert bool(torch.isfinite(out.float()).all()), what + ": non-finite output (scratch read before it was written)"
        assert torch.equal(out, plain[exp_ks]), what + ": differs from the same plan's launch on the default workspace"
        if exp_ks == 1:  # against the split launch: another summation order, so per element within the parity bound
            P.assert_elementwise(out, ref_acc + ex[0] + ex[1], bound, what + " unsplit", (bm, bn))
        seen.add(path)
        print(f"HANDOFF {kernel} footprint-{M}x{N}x{K}-{name} ks={exp_ks} fill=nan launches=1 ok")
    assert seen == ({"fixup", "unsplit"} if ks == 2 else {"fixup", "slab", "unsplit"}), seen


def test_conv3x3_scratch_stays_inside_the_workspace_it_was_given(force_plan):
    """gmd_conv3x3 directly, 3 x 23 x 20, 128 -> 320 on forced 256 x 160 tiles with two K slices: roomy, at the slab extent, 4 bytes
    below it."""
    import ctypes

    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    bm, bn, pf, ks = 256, 160, 283, 2
    B, Hh, Ww, ci, co = 3, 23, 20, 128, 320
    M = B * Hh * Ww
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, Hh * Ww, ci, generator=g).bfloat16().to(DEV)
    w = (torch.randn(co, 9 * ci, generator=g) * 0.03).bfloat16().to(DEV)
    b, tb = torch.randn(co, generator=g).to(DEV), torch.randn(B, co, generator=g).to(DEV)
    T = H.TAIL_BYTES
    slab_ext = H.slab_bytes(ks, M, co) + T
    assert H.fragment_bytes(ks, M, co, bm, bn) + T < slab_ext
    force_plan(bm, bn, pf, ks)
    plain = {ks: ops.conv3x3(x, w, B, Hh, Ww, bias=b, rowbias=tb)[0]}
    force_plan(bm, bn, pf, 1)
    plain[1] = ops.conv3x3(x, w, B, Hh, Ww, bias=b, rowbias=tb)[0]
    force_plan(bm, bn, pf, ks)
    gw = GuardedWorkspace(slab_ext + (2 << 20))
    fixup_max = lib().gmd_splitk_fixup_max(-1)
    for name, wp in (("roomy", slab_ext + (1 << 20)), ("slab-extent", slab_ext), ("slab-extent-4", slab_ext - 4)):
        exp_ks, path, written = H.expected_reduction(ks, M, co, bm, bn, wp, fixup_max)
        plan = (ctypes.c_int * 4)()
        assert lib().gmd_gemm_plan_info(ops.GMD_BF16, M, co, 9 * ci, 1, wp, 0, ctypes.addressof(plan)) == 0
        what = f"conv3x3 ks={ks} W'={name} ({wp} bytes: {path})"
        assert tuple(plan) == (bm, bn, pf, exp_ks), what
        gw.arm(wp)
        out = torch.full((B, Hh * Ww, co), float("nan"), dtype=BF16, device=DEV)
        rc = lib().gmd_conv3x3(x.data_ptr(), w.data_ptr(), out.data_ptr(), ops.GMD_BF16, ops.GMD_BF16, B, Hh, Ww, ci, co, 1, 0, 0, b.data_ptr(), tb.data_ptr(), co,
                               None, 1.0, None, 0, gw.ptr, wp, _stream())
        assert rc == 0, lib().gmd_last_error()
        torch.cuda.synchronize()
        gw.check(wp, written, what)
        assert bool(torch.isfinite(out.float()).all()) and torch.equal(out, plain[exp_ks]), what + ": differs from the same plan's launch on the default workspace"
        print(f"HANDOFF pp256x160 footprint-conv-{B}x{Hh}x{Ww}-{ci}to{co}-{name} ks={exp_ks} fill=nan launches=1 ok")


def test_float32_split_scratch_stays_inside_the_workspace_it_was_given():
    """The float32 matrix-core path's slabs at the shape of the alternating test: W' at the slab extent (the planner's slices, bit-
    equal to the default workspace's launch) and 4 bytes below it (one slice, no scratch byte written, per element within the bound)."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    M, N, K = SPLIT_SHAPE
    ks = lib().gmd_split_plan_ksplit(M, N, K, ops.WORKSPACE_BYTES)
    assert ks > 1
    slab_ext = H.slab_bytes(ks, M, N) + H.TAIL_BYTES
    gw = GuardedWorkspace(slab_ext + (1 << 20))
    with ops.f32_mode_scope("split"):
        s = _split_sets(M, N, K, ops)[0]
        plain = ops.gemm_nt(s["a"], s["ws"], bias=s["bias"])
    a, weff = s["a"], s["weff"]
    ref_acc, ad = a.double() @ weff.double().T, a.double().abs() @ weff.double().abs().T
    ex = [s["bias"].double().expand(M, N)]
    bound = P.gemm_bound(ref_acc, ad, 3 * K, F32, weff._alpha, ex, product_err=P.split_product_bound(a, weff), height=P.mfma_height(3 * K, 32, 16))
    for name, wp, exp_ks in (("slab-extent", slab_ext, ks), ("slab-extent-4", slab_ext - 4, 1)):
        what = f"float32 split W'={name} ({wp} bytes)"
        assert lib().gmd_split_plan_ksplit(M, N, K, wp) == exp_ks, what
        gw.arm(wp)
        out = torch.full((M, N), float("nan"), device=DEV)
        rc = lib().gmd_gemm_nt(a.data_ptr(), s["ws"].data_ptr(), out.data_ptr(), ops.GMD_F32SW, ops.GMD_F32, M, N, K, K, K, N, 1, 0, 0, M * N, s["bias"].data_ptr(),
                               None, 0, 0, None, N, 0, float(s["ws"]._alpha), ops.ACT_NONE, None, 0, gw.ptr, wp, _stream())
        assert rc == 0, lib().gmd_last_error()
        torch.cuda.synchronize()
        gw.check(wp, H.slab_bytes(ks, M, N) if exp_ks > 1 else 0, what)
        P.assert_elementwise(out, weff._alpha * ref_acc + ex[0], bound, what, (64, 64))
        if exp_ks > 1:
            assert torch.equal(out, plain), what + ": differs from the launch on the default workspace"
        print(f"HANDOFF f32split-slab footprint-{M}x{N}x{K}-{name} ks={exp_ks} fill=nan launches=1 ok")
