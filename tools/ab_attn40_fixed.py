#!/usr/bin/env python
"""A/B of the two bfloat16 instantiations of attn40_kernel in ONE build: the fixed softmax stabiliser (default) against the lagged
one (GMD_ATTN40_FIXED=0; the switch is read once per process, so every measurement is a child process of tools/bench_attn.py).
The variants alternate for `rounds` rounds on one box; per d = 40 shape the median [min .. max] of each is printed, and whether the
new variant's slowest round beats the old one's fastest (the only outcome that counts as a gain).  Usage: ab_attn40_fixed.py [rounds]"""
import os, re, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
res = {"lagged": {}, "fixed": {}}
for r in range(rounds):
    for name, val in (("lagged", "0"), ("fixed", "1")):
        env = dict(os.environ, GMD_ATTN40_FIXED=val)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_attn.py")], env=env, capture_output=True, text=True)
        if p.returncode != 0:
            sys.exit(f"round {r} {name}: bench_attn.py exited with {p.returncode}\n{p.stderr[-2000:]}")
        for line in p.stdout.splitlines():
            m = re.match(r"attn (.* d=40): +([0-9.]+) us", line)
            if m:
                res[name].setdefault(m.group(1), []).append(float(m.group(2)))
    print(f"round {r} done", flush=True)
fmt = lambda v: f"{statistics.median(v):7.1f} [{min(v):7.1f} .. {max(v):7.1f}] us"
for shape, old in res["lagged"].items():
    new = res["fixed"][shape]
    verdict = "gain" if max(new) < min(old) else "no gain beyond the spread"
    print(f"{shape:34s} lagged {fmt(old)}   fixed {fmt(new)}   median {100 * (statistics.median(new) / statistics.median(old) - 1):+.1f} %   {verdict}")
