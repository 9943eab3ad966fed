#!/usr/bin/env python
"""Device time of gmd_unipc_step at (corrector off, predictor 1) and (corrector 3, predictor 3) beside gmd_dpm_step at order 2 on the
same buffers (redirect the output to profiles/unipc_step.txt).

All three read the CFG pair of eps and the sample and write the pipeline's x0.  DPM order 2 reads one history tensor and writes m0 and
x_prev (4 float32 streams read, 3 written: 28 bytes per element).  UniPC always writes m0, x_corr and x_prev: 3 read, 4 written at
(off, 1) (28 bytes per element); at (3, 3) it also reads last_sample and three history tensors (7 read, 4 written: 44 bytes per element).
Two sizes: the bench latent (B = 4, 4 x 64 x 64, CFG) and the two-lap size of the tests (B = 2, 4 x 257 x 257, CFG).  Times are HIP
events around `--reps` back-to-back launches through the raw C ABI into preallocated outputs after a warm-up, the kernels alternating,
several rounds, the median reported; at the bench latent the figure is the launch rate of the stream, not the kernel.  Reported, not
gated.  Needs a GPU."""
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
assert torch.cuda.is_available(), "bench_unipc_step needs a GPU"
GS, GR = 7.5, 0.0
HEAD, TAIL = (0.83, 0.55), (0.6, 0.8)
CORR = (0.9, -0.31, -0.37, 0.21, -0.34, 0.47, -1.3, -2.6)
PRED = (0.78, -0.42, -0.45, 0.52, -0.13, -1.1, -2.3)


def case(B, shape):
    g = torch.Generator().manual_seed(0)
    eps = torch.randn((2 * B,) + shape, generator=g).cuda()
    x, last, h1, h2, h3 = (torch.randn((B,) + shape, generator=g).cuda() for _ in range(5))
    m0, xc, xp, x0 = (torch.empty_like(x) for _ in range(4))
    chw = x[0].numel()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def dpm2():
        rc = lib().gmd_dpm_step(p(eps), p(x), p(h1), B, chw, 1, GS, None, GR, 2, *HEAD, 0.78, -0.42, -0.21, -0.9, *TAIL, p(m0), p(xp), p(x0), st)
        assert rc == 0, lib().gmd_last_error()

    def unipc01():
        rc = lib().gmd_unipc_step(p(eps), p(x), None, None, None, None, B, chw, 1, GS, None, GR, 0, 1, *HEAD, *([0.0] * 8), PRED[0], PRED[1],
                                  *([0.0] * 5), *TAIL, p(m0), p(xc), p(xp), p(x0), st)
        assert rc == 0, lib().gmd_last_error()

    def unipc33():
        rc = lib().gmd_unipc_step(p(eps), p(x), p(last), p(h1), p(h2), p(h3), B, chw, 1, GS, None, GR, 3, 3, *HEAD, *CORR, *PRED, *TAIL, p(m0),
                                  p(xc), p(xp), p(x0), st)
        assert rc == 0, lib().gmd_last_error()

    tensor = B * chw * 4
    return (("dpm_step order 2", dpm2, 7 * tensor), ("unipc_step (off, 1)", unipc01, 7 * tensor), ("unipc_step (3, 3)", unipc33, 11 * tensor)), B * chw


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
        print(f"  {name:20s} us per launch over {a.rounds} rounds of {a.reps}: " + " ".join(f"{t:.2f}" for t in v) +
              f"   median {med[name]:.2f}   ({nbytes // n} B per element, {nbytes / 1e6:.2f} MB algorithmic, {nbytes / med[name] / 1e3:.1f} GB/s)")
    for name in ("unipc_step (off, 1)", "unipc_step (3, 3)"):
        print(f"  ratio {name} / dpm_step order 2: {med[name] / med['dpm_step order 2']:.3f}")
