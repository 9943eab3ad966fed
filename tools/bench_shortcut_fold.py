#!/usr/bin/env python
"""ResnetBlock2D tail, shape by shape: conv_shortcut (gemm_nt) + conv2 with `residual=` against the one fused launch
(hip_ops.conv3x3_tail), device time inside ONE HIP graph per variant (`reps` launches, operands rotated over `sets` buffer sets so a
launch does not find its inputs in L2 / Infinity Cache), `rounds` timed replays each, the two variants interleaved round by round.
SD-1.5's fourteen shortcut resnets at a 64 x 64 latent, UNet batch 4 and 8, both launch-plan families; then the AutoencoderKL's four
(decoder and encoder of a 512 x 512 image, batch 1 and 4, family 0: the VAE runs alone on the chip).  A shape counts as a win only when
the fused launch's SLOWEST round beats the pair's FASTEST one.
Usage: bench_shortcut_fold.py [--batches 4,8] [--families 0,1] [--vae-batches 1,4] [--rounds 7] [--reps 12] [--sets 4] [--dtype bf16]"""
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
ap.add_argument("--vae-batches", default="1,4")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--sets", type=int, default=4)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
a = ap.parse_args()
dt = {"bf16": torch.bfloat16, "f16": torch.float16}[a.dtype]
dev = "cuda"

# (side, conv2 Cin = Cout, shortcut K2, resnets of this shape per forward)
SHAPES = [(64, 320, 640, 2), (64, 320, 960, 1), (32, 640, 320, 1), (32, 640, 960, 1), (32, 640, 1280, 1), (32, 640, 1920, 1),
          (16, 1280, 640, 1), (16, 1280, 1920, 1), (16, 1280, 2560, 2), (8, 1280, 2560, 3)]
# AutoencoderKL at a 512 x 512 image: decoder up blocks 2 / 3 (first resnet), encoder down blocks 1 / 2 (first resnet)
VAE_SHAPES = [(256, 256, 512, 1), (512, 128, 256, 1), (256, 256, 128, 1), (128, 512, 256, 1)]


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
print(f"# {a.dtype}; us per resnet tail, median [min .. max] of {a.rounds} graph replays of {a.reps} launches over {a.sets} buffer sets")
print(f"# {'family B  side  Cin   K2  x':28s} {'plan (pair conv2 | fused)':34s} {'shortcut + conv2':26s} {'fused':26s} {'gain':>7s}  verdict")
tot = {}


def run(fam, B, side, c, k2, mult, cs, reps, nsets, tag):
    M = B * side * side
    sets = []
    for _ in range(nsets):
        h, x = rnd(B, side * side, c), rnd(B, side * side, k2)
        w2, wsc = rnd(c, 9 * c, scale=0.01), rnd(c, k2, scale=0.02)
        b2, bsc = torch.randn(c, device=dev), torch.randn(c, device=dev)
        sets.append((h, x, w2, wsc, b2, bsc) + ops.pack_shortcut(w2, b2, wsc, bsc))

    def pair(t):
        h, x, w2, wsc, b2, bsc = t[:6]
        def f():
            r = ops.gemm_nt(x.view(-1, k2), wsc, bias=bsc).view(B, side * side, c)
            return ops.conv3x3(h, w2, B, side, side, bias=b2, residual=r, colstats=cs)
        return f

    def fused(t):
        h, x, w, b = t[0], t[1], t[6], t[7]
        return lambda: ops.conv3x3_tail(h, x, w, B, side, side, bias=b, colstats=cs)

    p_pair, p_fused = ops.gemm_plan_info(dt, M, c, 9 * c), ops.gemm_plan_info(dt, M, c, 9 * c + k2)
    plans = f"{p_pair[0]}x{p_pair[1]} pf{p_pair[2]} ks{p_pair[3]} | {p_fused[0]}x{p_fused[1]} pf{p_fused[2]} ks{p_fused[3]}"
    head = f"  {fam}      {B}  {side:4d} {c:4d} {k2:4d}  {mult}"
    g_pair, ws_p = capture([pair(t) for t in sets], reps)
    if not ops.shortcut_fold_ok(dt, B, side, side, c, k2, c):
        tp = [replay_us(g_pair, reps) for _ in range(a.rounds)]
        print(f"{head:28s} {plans:34s} {statistics.median(tp):7.1f} [{min(tp):6.1f} ..{max(tp):6.1f}] {'-- (no K-tail loader for this plan)':26s}", flush=True)
        return
    g_fused, ws_f = capture([fused(t) for t in sets], reps)
    tp, tf = [], []
    for _ in range(a.rounds):
        tp.append(replay_us(g_pair, reps))
        tf.append(replay_us(g_fused, reps))
    mp, mf = statistics.median(tp), statistics.median(tf)
    win, lose = max(tf) < min(tp), min(tf) > max(tp)
    print(f"{head:28s} {plans:34s} {mp:7.1f} [{min(tp):6.1f} ..{max(tp):6.1f}] {mf:7.1f} [{min(tf):6.1f} ..{max(tf):6.1f}] {mp - mf:+7.1f}  "
          f"{'faster' if win else ('SLOWER' if lose else 'within scatter')}", flush=True)
    k = (tag, fam, B)
    tot[k] = tuple(u + v * mult for u, v in zip(tot.get(k, (0.0, 0.0)), (mp, mf)))


for fam in [int(v) for v in a.families.split(",")]:
    lib().gmd_gemm_plan_family(fam)
    for B in [int(v) for v in a.batches.split(",")]:
        for side, c, k2, mult in SHAPES:
            run(fam, B, side, c, k2, mult, side * side >= 1024, a.reps, a.sets, "UNet")  # statistics as UNet2DConditionModel._wants_colstats
            torch.cuda.empty_cache()
print("# AutoencoderKL, 512 x 512 image (decoder 256^2 512->256, 512^2 256->128; encoder 256^2 128->256, 128^2 256->512), family 0, no statistics; "
      f"{max(2, a.reps // 3)} launches over 2 buffer sets")
lib().gmd_gemm_plan_family(0)
for B in [int(v) for v in a.vae_batches.split(",") if v]:
    for side, c, k2, mult in VAE_SHAPES:
        run(0, B, side, c, k2, mult, False, max(2, a.reps // 3), 2, "VAE")
        torch.cuda.empty_cache()
for (tag, fam, B), (mp, mf) in tot.items():
    print(f"# {tag} family {fam} batch {B}: per forward (foldable shapes x their count) pair {mp:8.1f} us, fused {mf:8.1f} us, gain {mp - mf:+7.1f} us")
