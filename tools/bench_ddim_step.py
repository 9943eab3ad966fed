#!/usr/bin/env python
"""Device time of gmd_ddim_step beside gmd_ddpm_step on the same buffers (redirect the output to profiles/ddim_step.txt).

Both kernels read the CFG pair of eps, the sample and the noise and write x_prev and the pipeline's x0: the same bytes.  Two sizes: the
bench latent (B = 4, 4 x 64 x 64, CFG) and the two-lap size of the tests (B = 2, 4 x 257 x 257, CFG).  Times are HIP events around
`--reps` back-to-back launches through the raw C ABI into preallocated outputs after a warm-up, the two kernels alternating, several
rounds; at the bench latent the figure is the launch rate of the stream, not the kernel.  Reported, not gated.  Needs a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gm-diffusion_amd"))
import torch

from gm_diffusion._native import lib

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_ddim_step needs a GPU"
GS, GR = 7.5, 0.0


def case(B, shape):
    g = torch.Generator().manual_seed(0)
    eps = torch.randn((2 * B,) + shape, generator=g).cuda()
    x, noise = torch.randn((B,) + shape, generator=g).cuda(), torch.randn((B,) + shape, generator=g).cuda()
    xp, x0 = torch.empty_like(x), torch.empty_like(x)
    chw = x[0].numel()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def ddpm():
        rc = lib().gmd_ddpm_step(p(eps), p(x), p(noise), B, chw, 1, GS, None, GR, 0.9, 0.43, 0, 0.0, 0.3, 0.69, 0.1, 0.9, 0.43, p(xp), p(x0), st)
        assert rc == 0, lib().gmd_last_error()

    def ddim():
        rc = lib().gmd_ddim_step(p(eps), p(x), p(noise), B, chw, 1, GS, None, GR, 0.9, 0.43, 0, 0.0, 0, 0.95, 0.3, 0.1, 0.9, 0.43, p(xp), p(x0), None, st)
        assert rc == 0, lib().gmd_last_error()

    def ddim_clipped():  # the longest path: use_clipped_model_output, and the third output (pred_x0) written as well
        rc = lib().gmd_ddim_step(p(eps), p(x), p(noise), B, chw, 1, GS, None, GR, 0.9, 0.43, 1, 1.0, 1, 0.95, 0.3, 0.1, 0.9, 0.43, p(xp), p(x0), p(noise2), st)
        assert rc == 0, lib().gmd_last_error()

    noise2 = torch.empty_like(x)
    return (("ddpm_step", ddpm), ("ddim_step", ddim), ("ddim_step clip+use_clipped+pred_x0", ddim_clipped)), B * chw


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(a.reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / a.reps * 1e3


for B, shape in ((4, (4, 64, 64)), (2, (4, 257, 257))):
    fns, n = case(B, shape)
    for _, fn in fns:
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    rows = {name: [] for name, _ in fns}
    for _ in range(a.rounds):
        for name, fn in fns:
            rows[name].append(timed(fn))
    nbytes = n * 4 * 6  # eps pair, x, noise read; x_prev, x0 written
    print(f"B={B} {shape[0]}x{shape[1]}x{shape[2]} CFG: {n} elements, {nbytes / 1e6:.2f} MB algorithmic (two outputs)")
    for name, v in rows.items():
        med = sorted(v)[len(v) // 2]
        print(f"  {name:36s} us per launch over {a.rounds} rounds of {a.reps}: " + " ".join(f"{t:.2f}" for t in v) +
              f"   median {med:.2f}   ({nbytes / med / 1e3:.1f} GB/s at two outputs)")
