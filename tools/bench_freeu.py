#!/usr/bin/env python
"""What FreeU (enable_freeu) costs on one MI355X -> profiles/freeu.txt.

(a) per launch: the fused FreeU skip concat (gmd_concat_channels_freeu: backbone scaling + Fourier-filtered skip) beside the plain
    concat (gmd_concat_channels) at the six FreeU sites of an SD-1.5 UNet at 512x512 (three at 8x8, three at 16x16), UNet batch 8 (the
    SDR UNet under guidance at batch 4) and 4 (the GM UNet), bfloat16; and the in-place form (behind gmd_concat_channels_add) at the
    same sites;
(b) per forward: one SDR-UNet forward (SD-1.5 widths, random weights, UNet batch 8, 64x64 latents, captured graph, CFG shared prefix)
    without and with FreeU.
Each variant is ONE captured graph of `sets` launches over rotating operand buffers, replayed between device events; the variants of a
comparison alternate inside one process for `--rounds` rounds; the figures are the median over the rounds and [min .. max].
(The A/B of bench.py with FreeU off against the parent commit is tools/ab_bench.py's: appended to the same file by hand.)
Usage: bench_freeu.py [--rounds 5] [--reps 5] [--skip-unet] [--out profiles/freeu.txt]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freeu.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_freeu.py measures on the GPU only"
assert a.rounds >= 5, "at least 5 rounds"
DEV, DT = "cuda", torch.bfloat16
SETS = 24
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def graph_of(fn):
    """``fn`` captured once (after a warm-up on a side stream)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
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
    return f"{statistics.median(v):6.1f} [{min(v):5.1f} .. {max(v):5.1f}]"


say(f"# FreeU on one MI355X ({torch.cuda.get_device_name(0)}), bfloat16; every variant a captured graph of {SETS} launches over rotating "
    f"buffers, variants alternating, rounds={a.rounds}, median of {a.reps} replays per round; columns: median over rounds [min .. max]")
say()
say("## (a) the skip concat of one FreeU site, microseconds per launch: plain concat_channels | concat_channels_freeu (s = 0.2, b = 1.6) | "
    "concat_channels_freeu in place on the concatenated buffer (the ControlNet route's extra launch)")
say(f"{'batch':>5s} {'HxW':>7s} {'Ca':>5s} {'Cs':>5s} {'concat':>24s} {'concat_freeu':>24s} {'in place':>24s} {'freeu - concat':>15s}")
table = torch.tensor([0.9, 0.2, 1.5, 1.6], dtype=torch.float32, device=DEV)
extra = {8: 0.0, 4: 0.0}
for B in (8, 4):
    for (H, W), Ca, Cs, idx in (((8, 8), 1280, 1280, 0), ((8, 8), 1280, 1280, 0), ((8, 8), 1280, 1280, 0), ((16, 16), 1280, 1280, 1),
                                ((16, 16), 1280, 1280, 1), ((16, 16), 1280, 640, 1)):
        g0 = torch.Generator(DEV).manual_seed(B * 100 + H + Cs)
        xs = [torch.randn(B, H * W, Ca, generator=g0, device=DEV).to(DT) for _ in range(SETS)]
        ss = [torch.randn(B, H * W, Cs, generator=g0, device=DEV).to(DT) for _ in range(SETS)]
        bufs = [torch.cat([x, s], -1) for x, s in zip(xs, ss)]

        def plain():
            for x, s in zip(xs, ss):
                ops.concat_channels(x, s)

        def freeu():
            for x, s in zip(xs, ss):
                ops.concat_channels_freeu(x, s, B, H, W, table, 2 + idx, idx)

        def in_place():
            for b in bufs:
                ops.concat_channels_freeu(b[..., :Ca], b[..., Ca:], B, H, W, table, 2 + idx, idx, out=b)

        graphs = {"concat": graph_of(plain), "freeu": graph_of(freeu), "in_place": graph_of(in_place)}
        res = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, g in graphs.items():
                res[k].append(timed(g, a.reps, SETS))
        d = statistics.median(res["freeu"]) - statistics.median(res["concat"])
        extra[B] += d
        say(f"{B:5d} {H:3d}x{W:<3d} {Ca:5d} {Cs:5d} {fmt(res['concat']):>24s} {fmt(res['freeu']):>24s} {fmt(res['in_place']):>24s} {d:15.1f}")
        del graphs, xs, ss, bufs
for B, d in extra.items():
    say(f"=> UNet batch {B}: the six sites together cost {d:.1f} us more per forward than the six plain concats")
say()

if not a.skip_unet:
    from gm_diffusion.components import UNet2DConditionModel

    unet = UNet2DConditionModel(in_channels=4).init_random(1234, device=DEV).to(DEV, DT)
    fu = UNet2DConditionModel(in_channels=4)
    fu.load_state_dict(unet.state_dict())
    fu = fu.to(DEV, DT).enable_freeu(0.9, 0.2, 1.5, 1.6)
    ga = torch.Generator("cpu").manual_seed(7)
    B, h = 8, 64
    ctx = torch.randn(B, 77, 768, generator=ga).to(DEV)
    lat = torch.randn(B // 2, 4, h, h, generator=ga).to(DEV)
    graphs = {}
    for k, m in (("no FreeU", unet), ("FreeU (0.9, 0.2, 1.5, 1.6)", fu)):
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
    base = statistics.median(res["no FreeU"])
    for k, v in res.items():
        m = statistics.median(v)
        say(f"{k:28s} {m:8.3f} [{min(v):7.3f} .. {max(v):7.3f}]   {100 * (m / base - 1):+6.2f} % against no FreeU")
    say("=> six concat_channels_freeu launches in place of six concat_channels launches; the GroupNorm behind each of the six takes its "
        "general route (the producers' column statistics describe neither part any more).")

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
