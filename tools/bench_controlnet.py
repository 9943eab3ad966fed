#!/usr/bin/env python
"""What ControlNet conditioning costs on one MI355X -> profiles/controlnet.txt.  Recorded, not gated.

(a) gmd_concat_channels_add against gmd_concat_channels on the twelve SD-1.5 up-block concat shapes at UNet batch 8 (64x64 latents),
    with and without the in-kernel statistics of the B part;
(b) the GroupNorm that follows, served from those statistics (one pass) against its general route (statistics launch + apply);
(c) the dual pipeline at the bench configuration (SD-1.5 widths, random weights, 512x512, batch 4, 50 PNDM steps, graphs + two
    streams, latents out) without a ControlNet, with one (in-kernel statistics on / off) and in guess mode.
Every comparison runs its variants round-robin inside one process (`--rounds`), as tools/ab_bench.py does across processes: the
machines differ by 1-2 % and drift, so only figures of one run are compared.  Times are device events (a, b) or a host clock around
a device synchronise (c).
Usage: bench_controlnet.py [--rounds 3] [--reps 20] [--steps 2] [--skip-pipeline] [--out profiles/controlnet.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gm-diffusion_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from gm_diffusion import hip_ops as ops  # noqa: E402
from gm_diffusion._native import check, lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--steps", type=int, default=2)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--res", type=int, default=512)
ap.add_argument("--inference-steps", type=int, default=50)
ap.add_argument("--skip-pipeline", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "controlnet.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_controlnet.py measures on the GPU only"
DEV, DT = "cuda", torch.bfloat16
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps):
    """Median microseconds of ``reps`` launches, each between its own pair of device events."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return statistics.median(s.elapsed_time(e) for s, e in ev) * 1e3


def interleaved(variants, rounds, reps):
    """{name: [median us per round]} with the variants taken round-robin in every round; one untimed warm-up launch each."""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            res[k].append(timed(fn, reps))
    return res


def fmt(v):
    return f"{statistics.median(v):8.1f} [{min(v):7.1f} .. {max(v):7.1f}]"


# the twelve concats of an SD-1.5 up path: (x channels, skip channels, latent side at 64x64 latents)
SHAPES = [(1280, 1280, 8)] * 3 + [(1280, 1280, 16), (1280, 1280, 16), (1280, 640, 16), (1280, 640, 32), (640, 640, 32), (640, 320, 32),
                                  (640, 320, 64), (320, 320, 64), (320, 320, 64)]
UB = 8  # UNet batch: 4 prompts under classifier-free guidance
say(f"# ControlNet conditioning on one MI355X ({torch.cuda.get_device_name(0)}), bfloat16; rounds={a.rounds} interleaved, "
    f"median of {a.reps} launches per round; columns: median over rounds [min .. max]")
say()
say("## (a) skip concat with residual add, UNet batch 8, 64x64 latents: microseconds per launch")
say(f"{'Ca+Cb @ side':>18s} {'concat_channels':>30s} {'concat_add (Rb)':>30s} {'concat_add (Rb) + statistics':>30s}")
scales = torch.full((13,), 0.7, device=DEV)
tot = {"cat": 0.0, "add": 0.0, "stat": 0.0}
gn_rows = []
for k, (Ca, Cb, side) in enumerate(SHAPES):
    HW = side * side
    rows = UB * HW
    g = torch.Generator(DEV).manual_seed(k)
    x, s, r = (torch.randn(rows, c, generator=g, device=DEV).to(DT) for c in (Ca, Cb, Cb))
    mid = torch.randn(rows, Ca, generator=g, device=DEV).to(DT) if k == 0 else None
    out = torch.empty(rows, Ca + Cb, dtype=DT, device=DEV)
    st = torch.empty(rows // 64, Cb // 10, 2, device=DEV)
    cs = torch.cuda.current_stream().cuda_stream
    code = ops.dtype_code(DT)
    p = lambda t: None if t is None else t.data_ptr()

    def cat():
        check(lib().gmd_concat_channels(p(x), Ca, p(s), Cb, p(out), code, rows, cs), "concat")

    def add(stats=None):
        check(lib().gmd_concat_channels_add(p(x), Ca, p(mid), 12, p(s), Cb, p(r), k, p(scales), 0, p(out), code, rows, p(stats),
                                            10 if stats is not None else 0, cs), "concat_add")

    res = interleaved({"cat": cat, "add": add, "stat": lambda: add(st)}, a.rounds, a.reps)
    for n in tot:
        tot[n] += statistics.median(res[n])
    say(f"{Ca:5d}+{Cb:4d} @ {side:3d}{' +Ra' if mid is not None else '    '} {fmt(res['cat']):>30s} {fmt(res['add']):>30s} {fmt(res['stat']):>30s}")
    if HW >= 1024:  # (b): the levels whose GroupNorms take the two-launch route (UNet2DConditionModel._wants_colstats)
        add(st)
        xs = out.view(UB, HW, Ca + Cb)
        v = x.double().view(rows // 64, 64, Ca // 10, 10)
        sa = torch.stack([v.sum((1, 3)), (v * v).sum((1, 3))], -1).float().contiguous()
        gamma, beta = torch.ones(Ca + Cb, device=DEV), torch.zeros(Ca + Cb, device=DEV)
        plain = xs.clone()
        xs._colstats = [(sa, Ca), (st, Cb)]
        before = ops.colstats_uses
        y1 = ops.groupnorm(xs, UB, 32, gamma, beta, 1e-5, silu=True)
        assert ops.colstats_uses == before + 1
        y0 = ops.groupnorm(plain, UB, 32, gamma, beta, 1e-5, silu=True)
        err = float((y1.float() - y0.float()).abs().max())
        rg = interleaved({"stats": lambda: ops.groupnorm(xs, UB, 32, gamma, beta, 1e-5, silu=True),
                          "general": lambda: ops.groupnorm(plain, UB, 32, gamma, beta, 1e-5, silu=True)}, a.rounds, a.reps)
        gn_rows.append((Ca, Cb, side, rg, statistics.median(res["stat"]) - statistics.median(res["add"]), err))
    del x, s, r, out, st
say(f"{'sum of the twelve':>18s} {tot['cat']:30.1f} {tot['add']:30.1f} {tot['stat']:30.1f}")
say()
say("## (b) the GroupNorm(+SiLU) that follows, on the fresh statistics (one pass) against the general route: microseconds")
say(f"{'C @ side':>18s} {'statistics path':>30s} {'general path':>30s} {'saved':>8s} {'statistics cost in (a)':>24s} {'max |diff|':>11s}")
net = 0.0
for Ca, Cb, side, rg, cost, err in gn_rows:
    saved = statistics.median(rg["general"]) - statistics.median(rg["stats"])
    net += saved - cost
    say(f"{Ca + Cb:11d} @ {side:3d} {fmt(rg['stats']):>30s} {fmt(rg['general']):>30s} {saved:8.1f} {cost:24.1f} {err:11.3e}")
say(f"net per UNet forward over these {len(gn_rows)} concats (saved in GroupNorm minus spent in the concat): {net:+.1f} us")
say()

if not a.skip_pipeline:
    from gm_diffusion.components import ControlNetModel, PNDMScheduler, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline

    def sched():
        return PNDMScheduler(num_train_timesteps=1000, skip_prk_steps=True, set_alpha_to_one=False, beta_start=0.00085, beta_end=0.012,
                             beta_schedule="scaled_linear", steps_offset=1)

    def pipe_of(u, gm, cn):
        pp = StableDiffusionDualUNetPipeline(vae=None, text_encoder=None, tokenizer=None, unet=u, gm_unet=gm, scheduler=sched(),
                                             safety_checker=None, feature_extractor=None, requires_safety_checker=False, controlnet=cn)
        pp.set_progress_bar_config(disable=True)
        return pp

    unet = UNet2DConditionModel(in_channels=4).init_random(1234, device=DEV).to(DEV, DT)
    gm_unet = UNet2DConditionModel(in_channels=8).init_random(1238, device=DEV).to(DEV, DT)
    unet2 = UNet2DConditionModel(in_channels=4)
    unet2.load_state_dict(unet.state_dict())
    unet2.to(DEV, DT)  # the same weights: its control graph is captured with the in-kernel statistics switched off
    cn = ControlNetModel().init_random(1240, device=DEV).to(DEV, DT)
    B, h = a.batch, a.res // 8
    ge = torch.Generator("cpu").manual_seed(1)
    pos, neg = torch.randn(B, 77, 768, generator=ge).to(DEV), torch.randn(B, 77, 768, generator=ge).to(DEV)
    lat = torch.randn(B, 4, h, h, generator=torch.Generator("cpu").manual_seed(42)).to(DEV)
    img = torch.rand(B, 3, a.res, a.res, generator=torch.Generator("cpu").manual_seed(7)).to(DEV)
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, latents=lat, height=a.res, width=a.res, num_inference_steps=a.inference_steps,
              guidance_scale=7.5, output_type="latent")
    plain, with_cn, with_stats = pipe_of(unet, gm_unet, None), pipe_of(unet, gm_unet, cn), pipe_of(unet2, gm_unet, cn)
    assert not ops.USE_CONCAT_STATS, "unset GMD_CONCAT_STATS: this tool switches the in-kernel statistics itself"

    def run_with_stats():
        ops.USE_CONCAT_STATS = True  # read when the control graph is captured (the first call); the replays keep what was captured
        try:
            return with_stats(control_image=img, **kw)
        finally:
            ops.USE_CONCAT_STATS = False

    variants = {"no ControlNet": lambda: plain(**kw), "ControlNet": lambda: with_cn(control_image=img, **kw),
                "ControlNet, statistics on": run_with_stats, "ControlNet, guess mode": lambda: with_cn(control_image=img, guess_mode=True, **kw)}
    outs = {}
    for k, fn in variants.items():  # warm-up: weight preparation, graph capture, one replayed call
        fn()
        outs[k] = fn()
    torch.cuda.synchronize()
    res = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            for _ in range(a.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                res[k].append((time.perf_counter() - t0) * 1e3)
    n_it = a.inference_steps + 1
    say(f"## (c) dual pipeline, SD-1.5 widths, random weights, {a.res}x{a.res}, batch {B}, {a.inference_steps} PNDM steps ({n_it} iterations), "
        f"graphs + two streams, latents out: milliseconds per call ({a.steps} calls per round)")
    base = statistics.median(res["no ControlNet"])
    for k, v in res.items():
        m = statistics.median(v)
        say(f"{k:30s} {m:9.1f} [{min(v):8.1f} .. {max(v):8.1f}]   {m / n_it:7.2f} ms per iteration   {100 * (m / base - 1):+6.1f} % against no ControlNet")
    med = {k: statistics.median(v) for k, v in res.items()}
    spread = max((max(v) - min(v)) / med[k] for k, v in res.items())
    d_stats = med["ControlNet, statistics on"] / med["ControlNet"] - 1
    verdict = "inside the rounds' scatter: no gain to show" if abs(d_stats) <= spread else ("they pay" if d_stats < 0 else "they do NOT pay")
    say(f"=> a ControlNet adds {100 * (med['ControlNet'] / base - 1):.1f} % to the plain step ({100 * (med['ControlNet, guess mode'] / base - 1):.1f} % "
        f"in guess mode, where it runs the conditional half only); the in-kernel statistics change the ControlNet step by "
        f"{100 * d_stats:+.2f} % (largest spread of a variant over the rounds {100 * spread:.2f} %): {verdict}.")
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())
    say(f"latents, statistics on against off (same weights, same inputs): relative L2 sdr {rel(outs['ControlNet, statistics on'][0], outs['ControlNet'][0]):.3e} "
        f"gm {rel(outs['ControlNet, statistics on'][1], outs['ControlNet'][1]):.3e}; ControlNet against none: sdr "
        f"{rel(outs['ControlNet'][0], outs['no ControlNet'][0]):.3e}")

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
