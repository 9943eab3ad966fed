#!/usr/bin/env python
"""Device time of gmd_lms_step at order 1 and order 4 beside gmd_euler_step on the same buffers (redirect the output to
profiles/lms_step.txt).

All three read the CFG pair of eps and the sample.  Euler writes x_prev and x0 (three tensors read, two written); LMS also writes the
derivative, and at order 4 reads three history tensors (six read, three written).  Two sizes: the bench latent (B = 4, 4 x 64 x 64, CFG)
and the two-lap size of the tests (B = 2, 4 x 257 x 257, CFG).  Times are HIP events around `--reps` back-to-back launches through the raw
C ABI into preallocated outputs after a warm-up, the kernels alternating, several rounds, the median reported; at the bench latent the
figure is the launch rate of the stream, not the kernel.  Reported, not gated.  Needs a GPU."""
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
assert torch.cuda.is_available(), "bench_lms_step needs a GPU"
GS, GR = 7.5, 0.0


def case(B, shape):
    g = torch.Generator().manual_seed(0)
    eps = torch.randn((2 * B,) + shape, generator=g).cuda()
    x, d1, d2, d3 = (torch.randn((B,) + shape, generator=g).cuda() for _ in range(4))
    d, xp, x0 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    chw = x[0].numel()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def euler():
        rc = lib().gmd_euler_step(p(eps), p(x), None, B, chw, 1, GS, None, GR, 3.25, -1.4, 0.0, p(xp), p(x0), st)
        assert rc == 0, lib().gmd_last_error()

    def lms1():
        rc = lib().gmd_lms_step(p(eps), p(x), None, None, None, B, chw, 1, GS, None, GR, 1, 3.25, -1.4, 0.0, 0.0, 0.0, p(d), p(xp), p(x0), st)
        assert rc == 0, lib().gmd_last_error()

    def lms4():
        rc = lib().gmd_lms_step(p(eps), p(x), p(d1), p(d2), p(d3), B, chw, 1, GS, None, GR, 4, 3.25, -2.9, 2.7, -1.6, 0.4, p(d), p(xp), p(x0), st)
        assert rc == 0, lib().gmd_last_error()

    tensor = B * chw * 4
    return (("euler_step", euler, 5 * tensor), ("lms_step order 1", lms1, 6 * tensor), ("lms_step order 4", lms4, 9 * tensor)), B * chw


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
    print(f"B={B} {shape[0]}x{shape[1]}x{shape[2]} CFG: {n} latent elements")
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
        print(f"  {name:18s} us per launch over {a.rounds} rounds of {a.reps}: " + " ".join(f"{t:.2f}" for t in v) +
              f"   median {med[name]:.2f}   ({nbytes / 1e6:.2f} MB algorithmic, {nbytes / med[name] / 1e3:.1f} GB/s)")
    for name in ("lms_step order 1", "lms_step order 4"):
        print(f"  ratio {name} / euler_step: {med[name] / med['euler_step']:.3f}")
