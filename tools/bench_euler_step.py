#!/usr/bin/env python
"""Device time of gmd_euler_step beside gmd_ddim_step, and of gmd_pack_unet_input_scaled beside gmd_pack_unet_input, on the same buffers
(redirect the output to profiles/euler_step.txt).

The two step kernels read the CFG pair of eps, the sample and the noise and write x_prev and one x0: the same bytes.  The two packs read
eight float32 channels and write sixteen padded 16-bit channels for a CFG pair: the same bytes, the scaled one with a float32 division per
element.  Two sizes: the bench latent (B = 4, 4 x 64 x 64, CFG) and the two-lap size of the tests (B = 2, 4 x 257 x 257, CFG).  Times are
HIP events around `--reps` back-to-back launches through the raw C ABI into preallocated outputs after a warm-up, the kernels
alternating, several rounds; at the bench latent the figure is the launch rate of the stream, not the kernel.  Reported, not gated.
Needs a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gm-diffusion_amd"))
import torch

from gm_diffusion._native import GMD_BF16, lib

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_euler_step needs a GPU"
GS, GR = 7.5, 0.0


def case(B, shape):
    g = torch.Generator().manual_seed(0)
    eps = torch.randn((2 * B,) + shape, generator=g).cuda()
    x, noise = torch.randn((B,) + shape, generator=g).cuda(), torch.randn((B,) + shape, generator=g).cuda()
    xp, x0 = torch.empty_like(x), torch.empty_like(x)
    chw, hw = x[0].numel(), shape[1] * shape[2]
    packed = torch.empty(2 * B, hw, 16, dtype=torch.bfloat16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def ddim():
        rc = lib().gmd_ddim_step(p(eps), p(x), p(noise), B, chw, 1, GS, None, GR, 0.9, 0.43, 0, 0.0, 0, 0.95, 0.3, 0.1, 0.9, 0.43, p(xp), p(x0), None, st)
        assert rc == 0, lib().gmd_last_error()

    def euler():
        rc = lib().gmd_euler_step(p(eps), p(x), p(noise), B, chw, 1, GS, None, GR, 3.25, -1.4, 0.9, p(xp), p(x0), st)
        assert rc == 0, lib().gmd_last_error()

    def pack():
        rc = lib().gmd_pack_unet_input(p(x), shape[0], p(noise), shape[0], B, hw, 2, p(packed), 16, GMD_BF16, st)
        assert rc == 0, lib().gmd_last_error()

    def pack_scaled():
        rc = lib().gmd_pack_unet_input_scaled(p(x), shape[0], 14.648819, p(noise), shape[0], 14.648819, B, hw, 2, p(packed), 16, GMD_BF16, st)
        assert rc == 0, lib().gmd_last_error()

    step_bytes = B * chw * 4 * 6                              # eps pair, x, noise read; x_prev, x0 written
    pack_bytes = B * chw * 4 * 2 + 2 * B * hw * 16 * 2        # two float32 sources read; the padded bf16 CFG pair written
    return ((("ddim_step", ddim, step_bytes), ("euler_step", euler, step_bytes)),
            (("pack_unet_input", pack, pack_bytes), ("pack_unet_input_scaled", pack_scaled, pack_bytes))), B * chw


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(a.reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / a.reps * 1e3


for B, shape in ((4, (4, 64, 64)), (2, (4, 257, 257))):
    pairs, n = case(B, shape)
    print(f"B={B} {shape[0]}x{shape[1]}x{shape[2]} CFG: {n} latent elements")
    for fns in pairs:
        for _, fn, _ in fns:
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        rows = {name: [] for name, _, _ in fns}
        for _ in range(a.rounds):
            for name, fn, _ in fns:
                rows[name].append(timed(fn))
        med = {}
        for name, _, nbytes in fns:
            v = rows[name]
            med[name] = sorted(v)[len(v) // 2]
            print(f"  {name:24s} us per launch over {a.rounds} rounds of {a.reps}: " + " ".join(f"{t:.2f}" for t in v) +
                  f"   median {med[name]:.2f}   ({nbytes / 1e6:.2f} MB algorithmic, {nbytes / med[name] / 1e3:.1f} GB/s)")
        (base, _, _), (new, _, _) = fns
        print(f"  ratio {new} / {base}: {med[new] / med[base]:.3f}")
