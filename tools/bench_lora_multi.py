#!/usr/bin/env python
"""What SEVERAL LoRA adapters on one projection cost on one MI355X -> profiles/lora_multi.txt.  The file's head -- the compiler's
resource report of the stacked instantiations, from a cross-compile -- is kept: only the text from the MARK line on is rewritten.

(a) per projection: the ONE stacked launch (gmd_lora_update_stacked) against the N sequential gmd_lora_update launches it replaces --
    the GMD_LORA_STACK_FUSED=0 route, `fused=False` here -- at every (M, K = N = C) an attention projection of the SDR UNet runs at the
    bench configuration (512x512, batch 4 under guidance: UNet batch 8), rank pairs 16 + 16, 64 + 64 and 64 + 128, bfloat16, plain mode.
(b) per forward: one SDR-UNet forward (SD-1.5 widths, random weights, UNet batch 8, 64x64 latents, captured graph, CFG shared prefix)
    with two rank-16 adapters on all twelve transformer targets, against one rank-16 adapter and against none.
Each variant is ONE captured graph of `sets` launches over rotating operand buffers (so a launch does not find its operands in the
cache because the previous one left them there), replayed between device events; the variants of a comparison alternate inside one
process for `--rounds` rounds; the figures are the median over the rounds and [min .. max].
Usage: bench_lora_multi.py [--rounds 5] [--reps 5] [--skip-unet] [--out FILE]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_multi.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_lora_multi.py measures on the GPU only"
assert a.rounds >= 5, "at least 5 rounds"
DEV, DT = "cuda", torch.bfloat16
MARK = "# ==== measured on the GPU (tools/bench_lora_multi.py rewrites everything from this line on) ===="
lines = [MARK]


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
    """Median microseconds per unit of ``reps`` replays of a graph holding ``per`` units."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        g.replay()
        e.record()
    torch.cuda.synchronize()
    return statistics.median(s.elapsed_time(e) for s, e in ev) * 1e3 / per


def fmt(v):
    return f"{statistics.median(v):7.1f} [{min(v):6.1f} .. {max(v):6.1f}]"


def pad(n, m):
    return (n + m - 1) // m * m


say(f"# Several LoRA adapters on one projection on one MI355X ({torch.cuda.get_device_name(0)}), bfloat16; every variant a captured graph "
    f"over rotating buffers, variants alternating, rounds={a.rounds}, median of {a.reps} replays per round; columns: median over rounds "
    "[min .. max]")
say()
say("## (a) y += sum_a s_a (x A_a^T) B_a^T, plain mode, K = N = C: microseconds per PROJECTION; GB/s = (M*K + 2*M*N) * 2 bytes / stacked time")
say(f"{'M':>6s} {'C':>5s} {'ranks':>9s} {'Rp':>4s} {'sets':>5s} {'stacked (1 launch)':>26s} {'sequential (N launches)':>26s} {'stacked/seq':>12s} {'GB/s':>7s}")
slower = []
for M, C in zip((32768, 8192, 2048, 512), (320, 640, 1280, 1280)):
    nbytes = 3 * M * C * 2
    sets = max(2, min(24, -(-(640 << 20) // nbytes)))  # rotate through > 640 MB of operands (beyond the last-level cache), 2..24 sets
    g0 = torch.Generator(DEV).manual_seed(M + C)
    xs = [torch.randn(M, C, generator=g0, device=DEV).to(DT) for _ in range(sets)]
    ys = [torch.randn(M, C, generator=g0, device=DEV).to(DT) for _ in range(sets)]
    for ranks in ((16, 16), (64, 64), (64, 128)):
        rp = pad(sum(ranks), 32)
        sa, sb = torch.zeros(rp, C, device=DEV), torch.zeros(C, rp, device=DEV)
        parts, c0 = [], 0
        scal = torch.tensor([0.7, -0.4], device=DEV)
        cols = torch.zeros(3, rp + 8, device=DEV)
        for i, r in enumerate(ranks):
            fa, fb = torch.randn(r, C, generator=g0, device=DEV) / C ** 0.5, torch.randn(C, r, generator=g0, device=DEV) / r ** 0.5
            sa[c0:c0 + r], sb[:, c0:c0 + r] = fa, fb
            cols[1, c0:c0 + r] = scal[i]
            pa, pb = torch.zeros(pad(r, 32), C, device=DEV), torch.zeros(C, pad(r, 32), device=DEV)
            pa[:r], pb[:, :r] = fa, fb
            parts.append((pa.to(DT), pb.to(DT), scal, i))
            c0 += r
        sa, sb = sa.to(DT), sb.to(DT)

        def run(fused):
            for x, y in zip(xs, ys):
                ops.lora_update_stacked(x, sa, sb, y, cols, 1, fused=fused, parts=parts)

        gf, gs = graph_of(lambda: run(True)), graph_of(lambda: run(False))
        res = {"stacked": [], "sequential": []}
        for _ in range(a.rounds):
            res["stacked"].append(timed(gf, a.reps, sets))
            res["sequential"].append(timed(gs, a.reps, sets))
        mf, ms = statistics.median(res["stacked"]), statistics.median(res["sequential"])
        say(f"{M:6d} {C:5d} {'+'.join(map(str, ranks)):>9s} {rp:4d} {sets:5d} {fmt(res['stacked']):>26s} {fmt(res['sequential']):>26s} "
            f"{mf / ms:12.3f} {nbytes / mf / 1e3:7.0f}")
        if min(res["stacked"]) > max(res["sequential"]):
            slower.append((M, C, ranks))
        del gf, gs
    del xs, ys
say("=> " + ("the stacked launch is not slower than the sequential launches at any shape beyond the rounds' spread: every stacked 16-bit "
             "projection takes it." if not slower else
             f"the stacked launch is SLOWER than the sequential launches at (M, C, ranks) = {slower}: route those shapes to the sequential launches."))
say()

if not a.skip_unet:
    from gm_diffusion.components import UNet2DConditionModel
    from gm_diffusion.components import lora as _lora

    base = UNet2DConditionModel(in_channels=4).init_random(1234, device=DEV).to(DEV, DT)

    def clone():
        m = UNet2DConditionModel(in_channels=4)
        m.load_state_dict(base.state_dict())
        return m.to(DEV, DT)

    def adapter(seed):
        ga = torch.Generator("cpu").manual_seed(seed)
        shapes, sd = base.expected_keys(), {}
        for name in base.lora_module_names():
            if _lora.supported(name, "transformer"):
                n, k = shapes[name + ".weight"][:2]
                sd[f"unet.{name}.lora_A.weight"] = torch.randn(16, k, generator=ga) / k ** 0.5
                sd[f"unet.{name}.lora_B.weight"] = 0.1 * torch.randn(n, 16, generator=ga) / 4.0
        return sd

    one, two = clone().load_lora(adapter(7), targets="transformer"), clone().load_lora(adapter(7), targets="transformer")
    two.load_lora(adapter(8), targets="transformer")
    two.set_adapters(["default_0", "default_1"], [0.6, 0.4])
    B, h = 8, 64
    ga = torch.Generator("cpu").manual_seed(7)
    ctx = torch.randn(B, 77, 768, generator=ga).to(DEV)
    lat = torch.randn(B // 2, 4, h, h, generator=ga).to(DEV)
    graphs = {}
    for k, m in (("no adapter", base), ("one rank-16 adapter", one), ("two rank-16 adapters", two)):
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
    say(f"## (b) one SDR-UNet forward, SD-1.5 widths, random weights, UNet batch {B}, {h}x{h} latents, captured graph, CFG shared prefix; the "
        "adapters on all twelve transformer targets: milliseconds per forward (median of 10 replays per round)")
    b0 = statistics.median(res["no adapter"])
    for k, v in res.items():
        m = statistics.median(v)
        say(f"{k:24s} {m:8.3f} [{min(v):7.3f} .. {max(v):7.3f}]   {100 * (m / b0 - 1):+6.2f} % against no adapter")
    m1, m2 = statistics.median(res["one rank-16 adapter"]), statistics.median(res["two rank-16 adapters"])
    say(f"=> the second adapter adds {100 * (m2 / m1 - 1):+.2f} % to the forward of the one-adapter model, at the same number of launches "
        "(the stacks pad 16 + 16 to the 32 rank columns one rank-16 adapter already occupies).")

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
head = ""
if os.path.exists(a.out):
    with open(a.out) as f:
        head = f.read().split(MARK)[0]
with open(a.out, "w") as f:
    f.write(head + "\n".join(lines) + "\n")
