#!/usr/bin/env python
"""The few-step line beside bench.py's: bench.py's workload (SD-v1-5 dual-UNet 512x512, batch 4, bf16, synthetic weights, graphs + two
streams, two VAE decodes + the HDR tail) with guidance-embedded UNets (time_cond_proj_dim 256) and LCMScheduler at --inference-steps
(default 4) instead of plain UNets and 50 PNDM steps.  No classifier-free-guidance duplicate: the guidance scale goes into the UNets.
Prints one JSON line with bench.py's keys `value` (HDR images/s) and `ms_per_step` (per batch).  Compare it with bench.py only inside
one lease, interleaved (profiles/lcm_steps.txt).  The weights are random: this times the work, it says nothing about image quality.
Usage: bench_lcm_steps.py [--steps 6] [--warmup 2] [--inference-steps 4] [--batch 4] [--res 512] [--dtype bf16]"""
import argparse, json, os, sys, time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gm-diffusion_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=6)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--inference-steps", type=int, default=4)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--res", type=int, default=512)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
ap.add_argument("--cond-dim", type=int, default=256)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_lcm_steps.py needs an MI355X: the hot path is hand-written HIP with no CPU fallback")

from gm_diffusion import hdr
from gm_diffusion.components import AutoencoderKL, LCMScheduler, UNet2DConditionModel
from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline

dev = torch.device("cuda", 0)
dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
torch.set_num_threads(16)
unet = UNet2DConditionModel(in_channels=4, time_cond_proj_dim=a.cond_dim).init_random(1234, device=dev).to(dev, dtype)
gm_unet = UNet2DConditionModel(in_channels=8, time_cond_proj_dim=a.cond_dim).init_random(1238, device=dev).to(dev, dtype)
vae = AutoencoderKL().init_random(1334, device=dev).to(dev, dtype)
sched = LCMScheduler(steps_offset=1)
pipe = StableDiffusionDualUNetPipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, gm_unet=gm_unet, scheduler=sched,
                                       safety_checker=None, feature_extractor=None, requires_safety_checker=False)
pipe.set_progress_bar_config(disable=True)
B, h = a.batch, a.res // 8
ge = torch.Generator("cpu").manual_seed(1)
pos = torch.randn(B, 77, unet.config.cross_attention_dim, generator=ge).to(dtype).to(dev)
neg = torch.randn(B, 77, unet.config.cross_attention_dim, generator=ge).to(dtype).to(dev)
lat = torch.randn(B, 4, h, h, generator=torch.Generator("cpu").manual_seed(42)).to(dev)
unet._ensure(); gm_unet._ensure(); vae._ensure()
torch.cuda.synchronize()


def step():
    g = torch.Generator("cpu").manual_seed(1234)  # one CPU generator shared by both scheduler steps, as bench.py --scheduler ddpm
    sdr, gm = pipe(prompt_embeds=pos, negative_prompt_embeds=neg, latents=lat, height=a.res, width=a.res, num_inference_steps=a.inference_steps,
                   guidance_scale=7.5, generator=g, output_type="latent")
    return hdr.decode_to_hdr(vae, sdr, gm, qmax=99.0, want=("sdr_u8", "gm_u8", "hdr", "hdr_u16"))


for _ in range(a.warmup):
    out = step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(a.steps):
    out = step()
torch.cuda.synchronize()
el = time.perf_counter() - t0
finite = bool(torch.isfinite(out["hdr"]).all())
print(json.dumps({"metric": f"HDR images/sec @ {a.res}x{a.res}, {a.inference_steps} LCM steps, dual-UNet (guidance-embedded, no CFG duplicate)",
                  "value": round(B * a.steps / el, 4), "unit": "HDR images/s", "n_gpus": 1, "steps": a.steps, "warmup": a.warmup,
                  "ms_per_step": round(1000 * el / a.steps, 2), "dtype": a.dtype, "data": "synthetic", "batch": B,
                  "fused": bool(pipe._use_fused(lat, pipe.unet, pipe.scheduler)), "cfg_duplicate": bool(pipe.do_classifier_free_guidance),
                  "outputs_finite": finite}))
