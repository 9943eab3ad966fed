#!/usr/bin/env python
"""Upsample2D's convolution, shape by shape: the nine-tap launch over the virtual 2H x 2W image (hip_ops.conv3x3(.., upsample=True))
against the four 2x2 phase convolutions over the low-resolution image (hip_ops.conv3x3_up2, 4/9 of the products), device time inside
ONE HIP graph per variant (`reps` launches, operands rotated over `sets` buffer sets so a launch does not find its inputs in L2 /
Infinity Cache), `rounds` timed replays each, the two variants interleaved round by round.  SD-1.5's three UNet upsamplers at a
64 x 64 latent, UNet batch 4 and 8, both launch-plan families; then the AutoencoderKL decoder's three at a 512 x 512 image, batch 4,
family 0 (the VAE runs alone on the chip).  A shape counts as a win only when the phase launch's SLOWEST round beats the nine-tap
launch's FASTEST one.
Usage: bench_upsample_phases.py [--batches 4,8] [--families 0,1] [--vae-batches 4] [--rounds 7] [--reps 12] [--sets 4] [--dtype bf16]"""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gm-diffusion_amd")):
    sys.path.insert(0, p)
import torch
from gm_diffusion import hip_ops as ops
from gm_diffusion._native import lib

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="4,8")
ap.add_argument("--families", default="0,1")
ap.add_argument("--vae-batches", default="4")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--sets", type=int, default=4)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
a = ap.parse_args()
dt = {"bf16": torch.bfloat16, "f16": torch.float16}[a.dtype]
dev = "cuda"

# (input side, Cin = Cout): up_blocks.0 / .1 / .2 of SD-1.5 at a 64 x 64 latent; the decoder's up_blocks.0 / .1 / .2 at 512 x 512
SHAPES = [(8, 1280), (16, 1280), (32, 640)]
VAE_SHAPES = [(64, 512), (128, 512), (256, 256)]


def capture(fns, reps):
    for f in fns:
        f()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    ws = ops.new_workspace(dev)
    with torch.cuda.stream(s):
        with ops.workspace_scope(ws), torch.cuda.graph(gr):
            for r in range(reps):
                fns[r % len(fns)]()
    torch.cuda.synchronize()
    gr.replay(); torch.cuda.synchronize()
    return gr, ws


def replay_us(gr, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); gr.replay(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


rnd = lambda *s, scale=1.0: (torch.randn(*s, device=dev) * scale).to(dt)
print(f"# {a.dtype}; us per launch, median [min .. max] of {a.rounds} graph replays of {a.reps} launches over {a.sets} buffer sets")
print(f"# {'family B  side    C':24s} {'plan (nine-tap | phases)':36s} {'nine-tap':26s} {'phases':26s} {'ratio':>6s}  verdict")
tot = {}


def run(fam, B, side, c, cs, reps, nsets, tag):
    sets = []
    for _ in range(nsets):
        x, w, b = rnd(B, side * side, c), rnd(c, 9 * c, scale=0.01), torch.randn(c, device=dev)
        sets.append((x, w, b, ops.pack_upsample_phases(w)[0]))
    p9 = ops.gemm_plan_info(dt, 4 * B * side * side, c, 9 * c)
    p4 = ops.upsample_phases_plan(dt, B, side, side, c, c, colstats=cs)
    plans = f"{p9[0]}x{p9[1]} pf{p9[2]} ks{p9[3]} | " + (f"{p4[0]}x{p4[1]} pf{p4[2]} ks{p4[3]}" if p4 else "--")
    head = f"  {fam}      {B}  {side:4d} {c:5d}"
    g9, ws9 = capture([(lambda t=t: ops.conv3x3(t[0], t[1], B, side, side, bias=t[2], upsample=True, colstats=cs)) for t in sets], reps)
    if not ops.upsample_phases_ok(dt, B, side, side, c, c, colstats=cs):
        t9 = [replay_us(g9, reps) for _ in range(a.rounds)]
        print(f"{head:24s} {plans:36s} {statistics.median(t9):7.1f} [{min(t9):6.1f} ..{max(t9):6.1f}] {'-- (no phase launch under this plan)':26s}", flush=True)
        return
    g4, ws4 = capture([(lambda t=t: ops.conv3x3_up2(t[0], t[3], B, side, side, bias=t[2], colstats=cs)) for t in sets], reps)
    t9, t4 = [], []
    for _ in range(a.rounds):
        t9.append(replay_us(g9, reps))
        t4.append(replay_us(g4, reps))
    m9, m4 = statistics.median(t9), statistics.median(t4)
    win, lose = max(t4) < min(t9), min(t4) > max(t9)
    print(f"{head:24s} {plans:36s} {m9:7.1f} [{min(t9):6.1f} ..{max(t9):6.1f}] {m4:7.1f} [{min(t4):6.1f} ..{max(t4):6.1f}] {m4 / m9:6.2f}  "
          f"{'faster' if win else ('SLOWER' if lose else 'within scatter')}", flush=True)
    k = (tag, fam, B)
    tot[k] = tuple(u + v for u, v in zip(tot.get(k, (0.0, 0.0)), (m9, m4)))


for fam in [int(v) for v in a.families.split(",")]:
    lib().gmd_gemm_plan_family(fam)
    for B in [int(v) for v in a.batches.split(",")]:
        for side, c in SHAPES:
            run(fam, B, side, c, 4 * side * side >= 1024, a.reps, a.sets, "UNet")  # statistics as UNet2DConditionModel._wants_colstats
            torch.cuda.empty_cache()
print(f"# AutoencoderKL decoder, 512 x 512 image, family 0, no statistics; {max(2, a.reps // 3)} launches over 2 buffer sets")
lib().gmd_gemm_plan_family(0)
for B in [int(v) for v in a.vae_batches.split(",") if v]:
    for side, c in VAE_SHAPES:
        run(0, B, side, c, False, max(2, a.reps // 3), 2, "VAE")
        torch.cuda.empty_cache()
for (tag, fam, B), (m9, m4) in tot.items():
    print(f"# {tag} family {fam} batch {B}: per forward (shapes with a phase launch) nine-tap {m9:8.1f} us, phases {m4:8.1f} us, gain {m9 - m4:+7.1f} us")
