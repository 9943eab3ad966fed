#!/usr/bin/env python
"""What LoRA on the feed-forward and proj_in / proj_out (targets="transformer") costs on one MI355X -> profiles/lora_ff.txt.

(a) per launch: the update of ff.net.0.proj with the GEGLU in the same launch (gmd_lora_geglu: reads Y [M, 8C] once, writes F
    [M, 4C] once) against the composed route (gmd_lora_update in place on Y, then gmd_geglu_interleaved: a read-modify-write of Y and
    one more read of it) at the SD-1.5 bench shapes M = 4*4096 / C = 320, 4*1024 / 640, 4*256 / 1280, ranks 16 and 128, bfloat16;
(b) per forward: one SDR-UNet forward (SD-1.5 widths, random weights, UNet batch 8, 64x64 latents, captured graph, CFG shared prefix)
    without an adapter, without one but off ff_geglu_fused (GMD_FUSED_FF=0: what leaving the one-launch feed-forward costs by
    itself), with a rank-16 adapter on the eight attention projections, and with a rank-16 adapter on all twelve transformer targets
    through the fused launch and through the composed route; beside them the attention-only figure profiles/lora.txt recorded.
Method as tools/bench_lora.py: each variant is ONE captured graph of `sets` launches over rotating operand buffers, replayed between
device events; the variants of a comparison alternate inside one process for `--rounds` rounds; median over the rounds [min .. max].
Usage: bench_lora_ff.py [--rounds 5] [--reps 5] [--skip-unet] [--out profiles/lora_ff.txt]"""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gm-diffusion_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from gm_diffusion import hip_ops as ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--skip-unet", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_ff.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_lora_ff.py measures on the GPU only"
assert a.rounds >= 5, "at least 5 rounds"
DEV, DT = "cuda", torch.bfloat16
lines = []
WS = ops.new_workspace(torch.device(DEV, 0))


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def graph_of(fn):
    """``fn`` captured once (after a warm-up on a side stream)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), ops.workspace_scope(WS):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.workspace_scope(WS), torch.cuda.graph(g):
        fn()
    return g


def timed(g, reps, per):
    """Median microseconds per launch of ``reps`` replays of a graph holding ``per`` launches."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        g.replay()
        e.record()
    torch.cuda.synchronize()
    return statistics.median(s.elapsed_time(e) for s, e in ev) * 1e3 / per


def fmt(v):
    return f"{statistics.median(v):7.1f} [{min(v):6.1f} .. {max(v):6.1f}]"


say(f"# LoRA on the feed-forward and proj_in / proj_out on one MI355X ({torch.cuda.get_device_name(0)}), bfloat16; every variant a captured "
    f"graph over rotating buffers, variants alternating, rounds={a.rounds}, median of {a.reps} replays per round; columns: median over "
    f"rounds [min .. max]")
say()
say("## (a) F = geglu(Y + s (x a^T) b^T), Y [M, 8C] interleaved, F [M, 4C]: microseconds per call; GB/s = (M*C + M*8C + M*4C) * 2 bytes / "
    "fused time")
say(f"{'M':>6s} {'C':>5s} {'rank':>5s} {'sets':>5s} {'fused (1 launch)':>26s} {'composed (2 launches)':>26s} {'fused/composed':>15s} {'GB/s':>7s}")
scales = torch.full((16,), 0.7, device=DEV)
slower = []
for M, C in ((4 * 4096, 320), (4 * 1024, 640), (4 * 256, 1280)):
    nbytes = 13 * M * C * 2
    sets = max(2, min(24, -(-(640 << 20) // nbytes)))  # rotate through > 640 MB of operands (beyond the last-level cache), 2..24 sets
    g0 = torch.Generator(DEV).manual_seed(M + C)
    xs = [torch.randn(M, C, generator=g0, device=DEV).to(DT) for _ in range(sets)]
    ys = [torch.randn(M, 8 * C, generator=g0, device=DEV).to(DT) for _ in range(sets)]
    for rank in (16, 128):
        rp = (rank + 31) // 32 * 32
        fa, fb = torch.zeros(rp, C, device=DEV), torch.zeros(8 * C, rp, device=DEV)
        fa[:rank], fb[:, :rank] = torch.randn(rank, C, generator=g0, device=DEV) / C ** 0.5, 0.05 * torch.randn(8 * C, rank, generator=g0, device=DEV) / rank ** 0.5
        fa, fb = fa.to(DT), fb.to(DT)

        def run(fused):
            # the composed route updates y in place: the small update keeps the values in range over the replays, and both routes
            # do the same arithmetic whatever the values are
            for x, y in zip(xs, ys):
                ops.lora_geglu(x, fa, fb, y, scales, 3, fused=fused)

        gf, gc = graph_of(lambda: run(True)), graph_of(lambda: run(False))
        res = {"fused": [], "composed": []}
        for _ in range(a.rounds):
            res["fused"].append(timed(gf, a.reps, sets))
            res["composed"].append(timed(gc, a.reps, sets))
        mf, mc = statistics.median(res["fused"]), statistics.median(res["composed"])
        say(f"{M:6d} {C:5d} {rank:5d} {sets:5d} {fmt(res['fused']):>26s} {fmt(res['composed']):>26s} {mf / mc:15.3f} {nbytes / mf / 1e3:7.0f}")
        if max(res["composed"]) < min(res["fused"]):
            slower.append((M, C, rank))
        del gf, gc
    del xs, ys
say("=> " + ("the fused launch is not slower than the composed route at any shape beyond the rounds' spread: it is the default "
             "(hip_ops.USE_LORA_GEGLU_FUSED)." if not slower else
             f"the fused launch is SLOWER than the composed route at (M, C, rank) = {slower}."))
say()

if not a.skip_unet:
    from gm_diffusion.components import UNet2DConditionModel
    from gm_diffusion.components import lora as lora_names

    base_unet = UNet2DConditionModel(in_channels=4).init_random(1234, device=DEV).to(DEV, DT)

    def clone():
        m = UNet2DConditionModel(in_channels=4)
        m.load_state_dict(base_unet.state_dict())
        return m.to(DEV, DT)

    ga = torch.Generator("cpu").manual_seed(7)
    shapes = base_unet.expected_keys()
    sd_att, sd_all = {}, {}
    for name in base_unet.lora_module_names():
        if not lora_names.supported(name, "transformer"):
            continue
        n, k = shapes[name + ".weight"][:2]
        fa, fb = torch.randn(16, k, generator=ga) / k ** 0.5, 0.1 * torch.randn(n, 16, generator=ga) / 4.0
        sd_all[f"unet.{name}.lora_A.weight"], sd_all[f"unet.{name}.lora_B.weight"] = fa, fb
        if lora_names.supported(name):
            sd_att[f"unet.{name}.lora_A.weight"], sd_att[f"unet.{name}.lora_B.weight"] = fa, fb
    B, h = 8, 64
    ctx = torch.randn(B, 77, 768, generator=ga).to(DEV)
    lat = torch.randn(B // 2, 4, h, h, generator=ga).to(DEV)
    variants = (("no adapter", None, {}),
                ("no adapter, GMD_FUSED_FF=0", None, {"USE_FUSED_FF": False}),
                ("rank-16 attention adapter", sd_att, {}),
                ("rank-16 transformer adapter", sd_all, {}),
                ("... composed lora_geglu", sd_all, {"USE_LORA_GEGLU_FUSED": False}))
    graphs = {}
    for k, sd, switches in variants:
        m = base_unet if sd is None and not switches else clone()
        if sd is not None:
            m.load_lora(sd, targets="transformer")
        saved = {s: getattr(ops, s) for s in switches}
        for s, v in switches.items():  # read when the launches are issued, i.e. at capture
            setattr(ops, s, v)
        try:
            c = m.prepare_context(ctx)
            m.set_timestep(501)
            g = m.graphed_forward(B, h, h, c, cfg_shared=True)
            m.pack_input(lat, dup=1, out=g.x)
            g.replay()
        finally:
            for s, v in saved.items():
                setattr(ops, s, v)
        graphs[k] = (g, m)
    torch.cuda.synchronize()
    res = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, (g, _) in graphs.items():
            res[k].append(timed(g.graph, 10, 1) / 1e3)
    say(f"## (b) one SDR-UNet forward, SD-1.5 widths, random weights, UNet batch {B}, {h}x{h} latents, captured graph, CFG shared prefix: "
        f"milliseconds per forward (median of 10 replays per round)")
    base = statistics.median(res["no adapter"])
    for k, v in res.items():
        m = statistics.median(v)
        say(f"{k:30s} {m:8.3f} [{min(v):7.3f} .. {max(v):7.3f}]   {100 * (m / base - 1):+6.2f} % against no adapter")
    parent = None
    try:
        with open(os.path.join(ROOT, "profiles", "lora.txt")) as f:
            mm = re.search(r"^rank-16 attention adapter\s+([0-9.]+) \[.*?\]\s+([+-][0-9.]+) %", f.read(), re.M)
        parent = (float(mm.group(1)), float(mm.group(2))) if mm else None
    except OSError:
        pass
    if parent:
        say(f"{'(profiles/lora.txt, attention)':30s} {parent[0]:8.3f}                        {parent[1]:+6.2f} % against its own no-adapter run")
    nt = len(graphs["rank-16 transformer adapter"][1]._transformers)
    med = {k: statistics.median(v) for k, v in res.items()}
    say(f"=> the transformer adapter runs 9 rank updates and one lora_geglu per block and forward ({nt} blocks; the 2 x {nt} "
        f"cross-attention K / V updates run once per prompt) and takes the two-GEMM feed-forward in every block; it adds "
        f"{100 * (med['rank-16 transformer adapter'] / base - 1):.2f} % to the forward against {100 * (med['rank-16 attention adapter'] / base - 1):.2f} % "
        f"for the attention-only adapter.  Leaving ff_geglu_fused alone (no adapter, the blocks that took it) costs "
        f"{100 * (med['no adapter, GMD_FUSED_FF=0'] / base - 1):+.2f} %.  The composed lora_geglu route: "
        f"{100 * (med['... composed lora_geglu'] / med['rank-16 transformer adapter'] - 1):+.2f} % against the fused one.")

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
