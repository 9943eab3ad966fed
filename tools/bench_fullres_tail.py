#!/usr/bin/env python
"""Device time of the full-resolution tail (profiles/fullres_tail.txt).

  fused        hip_ops.hdr_tail_resized: decoded [2B, h*w, 4] float32 images (288 x 512) -> hdr_file + hdr_rgbe at 2160 x 3840
  composition  the same result without the fused kernel: hip_ops.hdr_tail at 288 x 512 (sdr, gm), two F.interpolate calls to
               2160 x 3840, hip_ops.apply_gm_to_sdr, a division by qmax + 1 and hip_ops.rgbe_encode at full size
  prepare      hip_ops.prepare_sdr 2160 x 3840 uint8 -> 288 x 512

The decodes themselves are common to both forms and left out: the operands are seeded random decoder-like images.  Times are HIP
events around `--reps` back-to-back calls after a warm-up, the two forms alternating, several rounds; bytes are the algorithm's (each
requested output written once, the small operands read once) over the fused time.  Needs a GPU: there is no CPU path."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gm-diffusion_amd"))
import torch
import torch.nn.functional as F

from gm_diffusion import hip_ops as ops

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--model", type=int, nargs=2, default=(288, 512))
ap.add_argument("--out", type=int, nargs=2, default=(2160, 3840))
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_fullres_tail needs a GPU"
B, (h, w), (H, W), q = a.batch, a.model, a.out, 99.0
g = torch.Generator().manual_seed(0)
dec = (torch.rand(2 * B, h * w, 4, generator=g) * 2.4 - 1.2).cuda()
src = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).cuda()
WANT = ("hdr_file", "hdr_rgbe")


def fused():
    return ops.hdr_tail_resized(dec[:B], dec[B:], 2, (H, W), sdr_hw=(h, w), gm_hw=(h, w), qmax=q, want=WANT)


def composition():
    t = ops.hdr_tail(dec[:B], dec[B:], 2, B, h, w, qmax=q, want=("sdr", "gm"))
    up = lambda x: F.interpolate(x.permute(0, 3, 1, 2), (H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).contiguous()
    hdr = ops.apply_gm_to_sdr(up(t["gm"]), up(t["sdr"]), qmax=q, clamp=False)
    hf = ops.tmo(hdr, 0, qmax=q)
    return {"hdr_file": hf, "hdr_rgbe": ops.rgbe_encode(hf)}


def prepare():
    return ops.prepare_sdr(src, (h, w), torch.float32)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(a.reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / a.reps


x, y = fused(), composition()
torch.cuda.synchronize()
d = (x["hdr_file"] - y["hdr_file"]).abs().max().item()
same = (x["hdr_rgbe"] == y["hdr_rgbe"]).all(-1).float().mean().item()
print(f"B={B} {h}x{w} -> {H}x{W}: max |fused - composition| of hdr_file {d:.3e}; RGBE pixels identical {100 * same:.3f} %")
for fn in (fused, composition, prepare):
    for _ in range(5):
        fn()
torch.cuda.synchronize()
rows = {"fused": [], "composition": [], "prepare": []}
for r in range(a.rounds):
    for name, fn in (("fused", fused), ("composition", composition), ("prepare", prepare)):
        rows[name].append(timed(fn))
for name, v in rows.items():
    print(f"{name:12s} ms per call over {a.rounds} rounds of {a.reps}: " + " ".join(f"{t:.4f}" for t in v) + f"   median {sorted(v)[len(v) // 2]:.4f}")
fb = 2 * B * 3 * h * w * 4 + B * H * W * (3 * 4 + 4)
pb = B * H * W * 3 + B * 3 * h * w * 4
mf, mp = sorted(rows["fused"])[a.rounds // 2], sorted(rows["prepare"])[a.rounds // 2]
print(f"fused: {fb / 1e6:.1f} MB algorithmic -> {fb / mf / 1e6:.1f} GB/s;  prepare: {pb / 1e6:.1f} MB -> {pb / mp / 1e6:.1f} GB/s;  "
      f"composition / fused = {sorted(rows['composition'])[a.rounds // 2] / mf:.2f}x")
