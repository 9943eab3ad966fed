#!/usr/bin/env python
"""What a LoRA adapter applied at run time costs on one MI355X -> profiles/lora.txt.

(a) per launch: the fused rank update (gmd_lora_update) against the composed route (two gmd_gemm_nt launches and
    gmd_scaled_add; full-width windows, so no memset) at every (M, K = N) an attention projection of the SD-1.5 UNets runs at the bench configuration (512x512, batch 4:
    the SDR UNet under guidance at UNet batch 8, the GM UNet at 4), ranks 4 / 16 / 64, bfloat16, plain mode; and the achieved bytes per
    second of the fused launch against the M*K + 2*M*N elements it has to move;
(b) per forward: one SDR-UNet forward (SD-1.5 widths, random weights, UNet batch 8, 64x64 latents, captured graph, CFG shared prefix)
    without an adapter and with a rank-16 adapter on the eight attention projections of every transformer block.
Each variant is ONE captured graph of `sets` launches over rotating operand buffers (so a launch does not find its operands in the
cache because the previous one left them there), replayed between device events; the variants of a comparison alternate inside one
process for `--rounds` rounds; the figures are the median over the rounds and [min .. max].
Usage: bench_lora.py [--rounds 5] [--reps 5] [--skip-unet] [--out profiles/lora.txt]"""
import argparse
import os
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_lora.py measures on the GPU only"
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
    with ops.workspace_scope(WS), torch.cuda.graph(g):  # the composed route's gemm_nt launches: one split-K scratch, made outside capture
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


say(f"# LoRA adapters applied at run time on one MI355X ({torch.cuda.get_device_name(0)}), bfloat16; every variant a captured graph over "
    f"rotating buffers, variants alternating, rounds={a.rounds}, median of {a.reps} replays per round; columns: median over rounds [min .. max]")
say()
say("## (a) y += s (x a^T) b^T, plain mode, K = N = C: microseconds per launch; GB/s = (M*K + 2*M*N) * 2 bytes / fused time")
say(f"{'UNet':>5s} {'M':>6s} {'C':>5s} {'rank':>5s} {'sets':>5s} {'fused (1 launch)':>26s} {'composed (3 launches)':>26s} {'fused/composed':>15s} {'GB/s':>7s}")
scales = torch.full((16,), 0.7, device=DEV)
slower = []
for unet, ms in (("SDR", (32768, 8192, 2048, 512)), ("GM", (16384, 4096, 1024, 256))):
    for M, C in zip(ms, (320, 640, 1280, 1280)):
        nbytes = 3 * M * C * 2
        sets = max(2, min(24, -(-(640 << 20) // nbytes)))  # rotate through > 640 MB of operands (beyond the last-level cache), 2..24 sets
        g0 = torch.Generator(DEV).manual_seed(M + C)
        xs = [torch.randn(M, C, generator=g0, device=DEV).to(DT) for _ in range(sets)]
        ys = [torch.randn(M, C, generator=g0, device=DEV).to(DT) for _ in range(sets)]
        for rank in (4, 16, 64):
            rp = (rank + 31) // 32 * 32
            fa, fb = torch.zeros(rp, C, device=DEV), torch.zeros(C, rp, device=DEV)
            fa[:rank], fb[:, :rank] = torch.randn(rank, C, generator=g0, device=DEV) / C ** 0.5, torch.randn(C, rank, generator=g0, device=DEV) / rank ** 0.5
            fa, fb = fa.to(DT), fb.to(DT)
            # the composed route's 16-bit gemm_nt contracts over multiples of 64: padded ONCE here, not inside the timed graph
            rc = (rank + 63) // 64 * 64
            ca, cb = torch.zeros(rc, C, dtype=DT, device=DEV), torch.zeros(C, rc, dtype=DT, device=DEV)
            ca[:rp], cb[:, :rp] = fa, fb

            def run(fused, A, B):
                for x, y in zip(xs, ys):
                    ops.lora_update(x, A, B, y, scales, 3, fused=fused)

            gf, gc = graph_of(lambda: run(True, fa, fb)), graph_of(lambda: run(False, ca, cb))
            res = {"fused": [], "composed": []}
            for _ in range(a.rounds):
                res["fused"].append(timed(gf, a.reps, sets))
                res["composed"].append(timed(gc, a.reps, sets))
            mf, mc = statistics.median(res["fused"]), statistics.median(res["composed"])
            say(f"{unet:>5s} {M:6d} {C:5d} {rank:5d} {sets:5d} {fmt(res['fused']):>26s} {fmt(res['composed']):>26s} {mf / mc:15.3f} {nbytes / mf / 1e3:7.0f}")
            if min(res["fused"]) > max(res["composed"]):
                slower.append((M, C, rank))
            del gf, gc
        del xs, ys
say("=> " + ("the fused launch is not slower than the composed route at any shape beyond the rounds' spread: every 16-bit shape takes it."
             if not slower else f"the fused launch is SLOWER than the composed route at (M, C, rank) = {slower}: route those shapes to the composed path."))
say()

if not a.skip_unet:
    from gm_diffusion.components import UNet2DConditionModel

    unet = UNet2DConditionModel(in_channels=4).init_random(1234, device=DEV).to(DEV, DT)
    adapted = UNet2DConditionModel(in_channels=4)
    adapted.load_state_dict(unet.state_dict())
    adapted = adapted.to(DEV, DT)
    ga = torch.Generator("cpu").manual_seed(7)
    shapes = adapted.expected_keys()
    sd = {}
    for name in adapted.lora_module_names():
        if ".transformer_blocks." in name and name.endswith(("to_q", "to_k", "to_v", "to_out.0")) and ".attn" in name:
            n, k = shapes[name + ".weight"][:2]
            sd[f"unet.{name}.lora_A.weight"] = torch.randn(16, k, generator=ga) / k ** 0.5
            sd[f"unet.{name}.lora_B.weight"] = 0.1 * torch.randn(n, 16, generator=ga) / 4.0
    adapted.load_lora(sd)
    B, h = 8, 64
    ctx = torch.randn(B, 77, 768, generator=ga).to(DEV)
    lat = torch.randn(B // 2, 4, h, h, generator=ga).to(DEV)
    graphs = {}
    for k, m in (("no adapter", unet), ("rank-16 attention adapter", adapted)):
        c = m.prepare_context(ctx)
        m.set_timestep(501)
        g = m.graphed_forward(B, h, h, c, cfg_shared=True)
        m.pack_input(lat, dup=1, out=g.x)
        g.replay()
        graphs[k] = g
    torch.cuda.synchronize()
    res = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, g in graphs.items():
            res[k].append(timed(g.graph, 10, 1) / 1e3)
    say(f"## (b) one SDR-UNet forward, SD-1.5 widths, random weights, UNet batch {B}, {h}x{h} latents, captured graph, CFG shared prefix: "
        f"milliseconds per forward (median of 10 replays per round)")
    base = statistics.median(res["no adapter"])
    for k, v in res.items():
        m = statistics.median(v)
        say(f"{k:28s} {m:8.3f} [{min(v):7.3f} .. {max(v):7.3f}]   {100 * (m / base - 1):+6.2f} % against no adapter")
    n_upd = 6 * len(adapted._transformers)
    say(f"=> {n_upd} rank updates per forward (the 2 x {len(adapted._transformers)} cross-attention K / V updates run once per prompt, outside the "
        f"forward) add {100 * (statistics.median(res['rank-16 attention adapter']) / base - 1):.2f} % to the forward; the expectation from "
        f"bytes alone was 5-10 %.")

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
