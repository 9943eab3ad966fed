#!/usr/bin/env python
"""What IP-Adapter image prompting costs on one MI355X -> profiles/ip_adapter.txt.

(a) per kernel: the fused decoupled cross-attention (gmd_attention_ip, one launch) against the composed route (two gmd_attention
    launches and gmd_scaled_add) at the three SD-1.5 cross-attention shapes of the bench configuration -- 4096 / 1024 / 256 queries,
    head dim 40 / 80 / 160, 8 heads, 77 text + 4 image keys, UNet batch 8, bfloat16 -- and the plain text attention for scale;
(b) per step: the dual pipeline at the bench configuration (SD-1.5 widths, random weights, 512x512, batch 4, bfloat16, graphs + two
    streams, latents out) without an adapter, with an adapter loaded but no image prompt, and with the image prompt (fused route and,
    in a pipeline of its own, the composed route).
Every comparison runs its variants round-robin inside one process (`--rounds`): the machines differ by 1-2 % and drift, so only
figures of one run are compared.  Times are device events (a) or a host clock around a device synchronise (b).
Usage: bench_ip_adapter.py [--rounds 5] [--reps 50] [--steps 2] [--inference-steps 50] [--skip-pipeline] [--out profiles/ip_adapter.txt]"""
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

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--steps", type=int, default=2)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--res", type=int, default=512)
ap.add_argument("--inference-steps", type=int, default=50)
ap.add_argument("--skip-pipeline", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ip_adapter.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_ip_adapter.py measures on the GPU only"
DEV, DT = "cuda", torch.bfloat16
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps):
    """Median microseconds of ``reps`` calls, each between its own pair of device events."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return statistics.median(s.elapsed_time(e) for s, e in ev) * 1e3


def interleaved(variants, rounds, reps):
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


UB, H, NK, NIP = 2 * a.batch, 8, 77, 4
say(f"# IP-Adapter image prompting on one MI355X ({torch.cuda.get_device_name(0)}), bfloat16; rounds={a.rounds} interleaved, median of "
    f"{a.reps} calls per round; columns: median over rounds [min .. max]")
say()
say(f"## (a) decoupled cross-attention, UNet batch {UB}, {H} heads, {NK} text + {NIP} image keys: microseconds per call")
say(f"{'queries x head dim':>20s} {'text only (1 launch)':>30s} {'fused (1 launch)':>30s} {'composed (3 launches)':>30s} {'fused / composed':>17s}")
slower = []
scales = torch.full((16,), 0.6, device=DEV)
for nq, d in ((4096, 40), (1024, 80), (256, 160)):
    g = torch.Generator(DEV).manual_seed(nq)
    C = H * d
    q = torch.randn(UB, nq, C, generator=g, device=DEV).to(DT)
    k = torch.randn(UB, NK, C, generator=g, device=DEV).to(DT)
    kip = torch.randn(UB, NIP, C, generator=g, device=DEV).to(DT)
    vt = torch.zeros(UB, C, 80, dtype=DT, device=DEV)
    vt[:, :, :NK] = torch.randn(UB, C, NK, generator=g, device=DEV).to(DT)
    vtip = torch.zeros(UB, C, 8, dtype=DT, device=DEV)
    vtip[:, :, :NIP] = torch.randn(UB, C, NIP, generator=g, device=DEV).to(DT)
    sc = d ** -0.5
    res = interleaved({"text": lambda: ops.attention(q, k, vt, H, NK, sc),
                       "fused": lambda: ops.attention_ip(q, k, vt, kip, vtip, H, NK, NIP, sc, scales, 3, fused=True),
                       "composed": lambda: ops.attention_ip(q, k, vt, kip, vtip, H, NK, NIP, sc, scales, 3, fused=False)}, a.rounds, a.reps)
    ratio = statistics.median(res["fused"]) / statistics.median(res["composed"])
    say(f"{nq:13d} x {d:4d} {fmt(res['text']):>30s} {fmt(res['fused']):>30s} {fmt(res['composed']):>30s} {ratio:17.3f}")
    if min(res["fused"]) > max(res["composed"]):
        slower.append((nq, d))
    del q, k, kip, vt, vtip
say("=> " + ("the fused kernel is not slower than the composed route at any shape beyond the rounds' spread: every 16-bit shape takes it."
             if not slower else f"the fused kernel is SLOWER than the composed route at {slower}: route those shapes to the composed path."))
say()

if not a.skip_pipeline:
    from gm_diffusion.components import PNDMScheduler, UNet2DConditionModel
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline

    def sched():
        return PNDMScheduler(num_train_timesteps=1000, skip_prk_steps=True, set_alpha_to_one=False, beta_start=0.00085, beta_end=0.012,
                             beta_schedule="scaled_linear", steps_offset=1)

    def pipe_of(u, gm):
        pp = StableDiffusionDualUNetPipeline(vae=None, text_encoder=None, tokenizer=None, unet=u, gm_unet=gm, scheduler=sched(),
                                             safety_checker=None, feature_extractor=None, requires_safety_checker=False)
        pp.set_progress_bar_config(disable=True)
        return pp

    def same_weights(u):
        m = UNet2DConditionModel(in_channels=u.config.in_channels)
        m.load_state_dict(u.state_dict())
        return m.to(DEV, DT)

    unet = UNet2DConditionModel(in_channels=4).init_random(1234, device=DEV).to(DEV, DT)
    gm_unet = UNet2DConditionModel(in_channels=8).init_random(1238, device=DEV).to(DEV, DT)
    unet_ip, unet_comp = same_weights(unet), same_weights(unet)
    # a seeded plain adapter of the published SD-1.5 shape: 4 tokens per image, CLIP ViT-H projection width 1024
    proj, kv = unet.ip_adapter_expected_keys(4, 1024)
    ga = torch.Generator("cpu").manual_seed(1242)
    sd = {"image_proj": {n: (torch.ones(s) if n == "norm.weight" else torch.zeros(s) if n.endswith("bias") else torch.randn(s, generator=ga) * s[1] ** -0.5)
                         for n, s in proj.items()},
          "ip_adapter": {n: torch.randn(s, generator=ga) * s[1] ** -0.5 for n, s in kv.items()}}
    B, h = a.batch, a.res // 8
    ge = torch.Generator("cpu").manual_seed(1)
    pos, neg = torch.randn(B, 77, 768, generator=ge).to(DEV), torch.randn(B, 77, 768, generator=ge).to(DEV)
    lat = torch.randn(B, 4, h, h, generator=torch.Generator("cpu").manual_seed(42)).to(DEV)
    img = torch.cat([torch.zeros(1, 1, 1024), torch.randn(1, 1, 1024, generator=ge)]).to(DEV)  # [negative; positive] of one picture
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, latents=lat, height=a.res, width=a.res, num_inference_steps=a.inference_steps,
              guidance_scale=7.5, output_type="latent")
    plain, with_ip, with_comp = pipe_of(unet, gm_unet), pipe_of(unet_ip, gm_unet), pipe_of(unet_comp, gm_unet)
    with_ip.load_ip_adapter(sd)
    with_comp.load_ip_adapter(sd)
    assert ops.USE_ATTN_IP_FUSED, "unset GMD_ATTN_IP_FUSED: this tool switches the route itself"

    def run_composed():
        ops.USE_ATTN_IP_FUSED = False  # read when the graph is captured (the first call); the replays keep what was captured
        try:
            return with_comp(ip_adapter_image_embeds=[img], **kw)
        finally:
            ops.USE_ATTN_IP_FUSED = True

    variants = {"no adapter": lambda: plain(**kw), "adapter loaded, no image prompt": lambda: with_ip(**kw),
                "image prompt, fused": lambda: with_ip(ip_adapter_image_embeds=[img], **kw), "image prompt, composed": run_composed}
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
    say(f"## (b) dual pipeline, SD-1.5 widths, random weights, {a.res}x{a.res}, batch {B}, {a.inference_steps} PNDM steps ({n_it} iterations), "
        f"graphs + two streams, latents out: milliseconds per call ({a.steps} calls per round)")
    base = statistics.median(res["no adapter"])
    for k, v in res.items():
        m = statistics.median(v)
        say(f"{k:34s} {m:9.1f} [{min(v):8.1f} .. {max(v):8.1f}]   {m / n_it:7.2f} ms per iteration   {100 * (m / base - 1):+6.2f} % against no adapter")
    med = {k: statistics.median(v) for k, v in res.items()}
    spread = max((max(v) - min(v)) / med[k] for k, v in res.items())
    say(f"=> the image prompt adds {100 * (med['image prompt, fused'] / base - 1):.2f} % to the plain step on the fused route "
        f"({100 * (med['image prompt, composed'] / base - 1):.2f} % composed); a loaded adapter without an image prompt changes it by "
        f"{100 * (med['adapter loaded, no image prompt'] / base - 1):+.2f} % (largest spread of a variant over the rounds {100 * spread:.2f} %): "
        f"it launches what the plain pipeline launches.")
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())
    same = torch.equal(outs["adapter loaded, no image prompt"][0], outs["no adapter"][0])
    say(f"latents: adapter loaded without an image prompt {'bit-identical to' if same else 'DIFFERENT from'} no adapter; fused against composed "
        f"relative L2 sdr {rel(outs['image prompt, fused'][0], outs['image prompt, composed'][0]):.3e}; image prompt against none: sdr "
        f"{rel(outs['image prompt, fused'][0], outs['no adapter'][0]):.3e}")

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
