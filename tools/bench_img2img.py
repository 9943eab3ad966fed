#!/usr/bin/env python
"""What img2img and inpainting cost in the dual-UNet pipeline on one MI355X -> profiles/img2img.txt.

The bench configuration (SD-1.5 widths, random weights, 512x512, bfloat16, batch 4, PNDM, guidance 7.5, captured graphs, two streams),
latents out.  Four calls alternate inside one process for `--rounds` rounds, each timed between two device synchronisations:
  plain            no picture: the joint loop
  inpaint s=1.0    image (as latents) + mask at strength 1: the joint loop plus ONE gmd_inpaint_blend launch per step
  img2img s=0.5    image (as latents) at strength 0.5: len(T) GM forwards, len(T) - t_start SDR forwards, one launch for the start
  img2img pixels   the same from a [1, 3, 512, 512] picture: plus preprocess, AutoencoderKL.encode (float32) and the sample
The figures are the median over the rounds and [min .. max].
Usage: bench_img2img.py [--rounds 5] [--steps 50] [--out profiles/img2img.txt]"""
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

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--res", type=int, default=512)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "img2img.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_img2img.py measures on the GPU only"
assert a.rounds >= 5, "at least 5 rounds"
DEV, DT = "cuda", torch.bfloat16
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


from gm_diffusion.components import AutoencoderKL, PNDMScheduler, UNet2DConditionModel  # noqa: E402
from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline  # noqa: E402

unet = UNet2DConditionModel(in_channels=4).init_random(1234, device=DEV).to(DEV, DT)
gm_unet = UNet2DConditionModel(in_channels=8).init_random(1238, device=DEV).to(DEV, DT)
vae = AutoencoderKL().init_random(1334, with_encoder=True, device=DEV).to(DEV, torch.float32)  # pixels are encoded in float32
sched = PNDMScheduler(num_train_timesteps=1000, skip_prk_steps=True, set_alpha_to_one=False, beta_start=0.00085, beta_end=0.012,
                      beta_schedule="scaled_linear", steps_offset=1)
pipe = StableDiffusionDualUNetPipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, gm_unet=gm_unet, scheduler=sched,
                                       safety_checker=None, feature_extractor=None, requires_safety_checker=False)
pipe.set_progress_bar_config(disable=True)
B, h = a.batch, a.res // 8
ge = torch.Generator("cpu").manual_seed(1)
cross = unet.config.cross_attention_dim
pos, neg = (torch.randn(B, 77, cross, generator=ge).to(DT).to(DEV) for _ in range(2))
lat = torch.randn(B, 4, h, h, generator=torch.Generator("cpu").manual_seed(42)).to(DEV)
z0 = (0.8 * torch.randn(B, 4, h, h, generator=torch.Generator("cpu").manual_seed(43))).to(DEV)
yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(h, dtype=torch.float32), indexing="ij")
mask = (((yy - h / 2) ** 2 + (xx - h / 2) ** 2) < (0.36 * h) ** 2).to(torch.float32)[None, None].to(DEV)
picture = torch.rand(1, 3, a.res, a.res, generator=torch.Generator("cpu").manual_seed(44)).to(DEV)
common = dict(prompt_embeds=pos, negative_prompt_embeds=neg, latents=lat, height=a.res, width=a.res, num_inference_steps=a.steps,
              guidance_scale=7.5, output_type="latent")
calls = {
    "plain": {},
    "inpaint s=1.0": dict(image=z0, mask_image=mask, strength=1.0),
    "img2img s=0.5": dict(image=z0, strength=0.5),
    "img2img pixels s=0.5": dict(image=picture, strength=0.5, generator=None),
}


def run(kw):
    kw = dict(kw)
    if "generator" in kw:
        kw["generator"] = torch.Generator("cpu").manual_seed(7)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pipe(**common, **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for kw in calls.values():  # warm-up: graph captures, plan tables, allocator
    run(kw)
res = {k: [] for k in calls}
for _ in range(a.rounds):
    for k, kw in calls.items():
        res[k].append(run(kw))
n_t = a.steps + 1  # PNDM's schedule holds its second timestep twice
t_start = max(a.steps - min(int(a.steps * 0.5), a.steps), 0)
say(f"# img2img / inpainting of the dual-UNet pipeline on one MI355X ({torch.cuda.get_device_name(0)}): SD-1.5 widths, random weights, "
    f"{a.res}x{a.res}, bfloat16, batch {B}, PNDM {a.steps} steps ({n_t} UNet iterations), guidance 7.5, graphs + two streams, latents out; the "
    f"calls alternate, rounds={a.rounds}; milliseconds per call: median over rounds [min .. max]")
say(f"# command: python tools/bench_img2img.py --rounds {a.rounds} --steps {a.steps} --batch {B} --res {a.res}")
base = statistics.median(res["plain"])
for k, v in res.items():
    m = statistics.median(v)
    say(f"{k:24s} {m:9.2f} [{min(v):9.2f} .. {max(v):9.2f}]   {100 * (m / base - 1):+7.2f} % against plain   {(m - base) / n_t * 1e3:+9.1f} us per iteration")
say(f"=> inpaint at strength 1 is the joint loop plus one gmd_inpaint_blend launch per step: the difference per iteration is that launch "
    f"(and its place in front of the GM stream's wait).")
say(f"=> img2img at strength 0.5 runs {n_t} GM forwards and {n_t - t_start} SDR forwards (t_start = {t_start}): the first {t_start} "
    f"iterations are the GM UNet alone.")

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
