#!/usr/bin/env python3
"""SWQG cadence: steps/s of the single-layer shallow-water QG
model against TwoLayerQG on the same grid, stepper (IFMAB3) and library, at
the drivers' 512² and at 2048².

    python tools/swqg_cadence.py [--sizes 512 2048] [--pairs 3] [--seconds S] [--out FILE]

Both problems live in one process; their timed windows alternate (SWQG, 2LQG,
SWQG, …), each after a warm-up block, `--pairs` times.  One JSON line per pair
with the two rates, one per size for SWQG with `unfused = 1` (the separate
column kernels), and one per size with the per-kernel times of
sw_profile_steps and each kernel's algorithmic bytes over the HBM peak.
Hardware counters are not collected here.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E (bench.py)


def rate(prob, seconds, block):
    prob.stepforward(block)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        prob.stepforward(block)
        n += block
    return n / (time.perf_counter() - t0)


def profile(prob, nsteps=200):
    out = []
    for s in prob.ctx.profile(nsteps):
        if s["launches"]:
            gbps = s["alg_bytes"] / (s["avg_ms"] * 1e-3) / 1e9
            out.append(dict(kernel=s["name"], us=1e3 * s["avg_ms"], alg_MB=s["alg_bytes"] / 1e6,
                            hbm_frac=gbps / HBM_PEAK_GBPS))
    return out


def main():
    from juliaraytracingsw_amd import drivers

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", type=int, default=[512, 2048])
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []
    for n in a.sizes:
        block = 200 if n <= 1024 else 50
        sq, _ = drivers.swqg_problem(n, "IFMAB3")
        qg, _ = drivers.qg2_problem(n, "IFMAB3")
        for pair in range(a.pairs):
            lines.append(dict(n=n, stepper="IFMAB3", pair=pair, swqg=rate(sq, a.seconds, block),
                              qg2=rate(qg, a.seconds, block)))
            print(json.dumps(lines[-1]), flush=True)
        lines.append(dict(n=n, model="swqg", profile=profile(sq)))
        lines.append(dict(n=n, model="qg2", profile=profile(qg)))
        sq.close()
        qg.close()
        un, _ = drivers.swqg_problem(n, "IFMAB3", unfused=True)
        lines.append(dict(n=n, model="swqg", unfused=1, steps_per_s=rate(un, a.seconds, block), profile=profile(un)))
        un.close()
        for ln in lines[-3:]:
            print(json.dumps(ln), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
