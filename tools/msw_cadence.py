#!/usr/bin/env python3
"""Cadence of the modified and the Lindborg shallow-water models (DESIGN.md
§11): steps/s of RSW, MSW and LSW on the same grid, stepper and library, at the
drivers' 512² and at 2048², with IFMAB3 and FilteredAB3.

    python tools/msw_cadence.py [--sizes 512 2048] [--rounds 3] [--seconds S] [--out FILE]

The three problems of one (size, stepper) live in one process; their timed
windows alternate (RSW, MSW, LSW, RSW, …), each after a warm-up block,
`--rounds` times.  One JSON line per round with the three rates and the ratios
to RSW, then one per model with the per-kernel times of sw_profile_steps and
each kernel's algorithmic bytes over the HBM peak.  Hardware counters are not
collected here.

The problems are RSWDriver's (drivers.rsw_parameters, the shafer initial
condition) without the blow-up check: FilteredAB3 at the driver parameters is
linearly unstable below 2048² (tests/test_oracle.py), and the kernels' time
does not depend on the values they move.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E (bench.py)
VARIANTS = ("rsw", "modified", "lindborg")


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


def problem(drivers, variant, n, stepper):
    P = drivers.rsw_parameters(n)
    kw = {"order": P["filter_order"]} if stepper == "FilteredAB3" else {}
    prob = drivers.RSW_VARIANTS[variant].Problem("gpu", nx=n, Lx=P["Lx"], dt=P["dt"], f=P["f"], Cg=P["Cg"],
                                                 nnu=P["nnu"], nu=P["nu"], stepper=stepper, check_nan=False, **kw)
    drivers.set_shafer_initial_condition(prob, P["Kg"], P["Kw"], P["ag"], P["aw"], P["f"], P["Cg"] ** 2,
                                         np.random.default_rng(20261015))
    return prob


def main():
    from juliaraytracingsw_amd import drivers

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", type=int, default=[512, 2048])
    ap.add_argument("--steppers", nargs="*", default=["IFMAB3", "FilteredAB3"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []
    for n in a.sizes:
        block = 200 if n <= 1024 else 50
        for stepper in a.steppers:
            probs = {v: problem(drivers, v, n, stepper) for v in VARIANTS}
            for rnd in range(a.rounds):
                r = {v: rate(probs[v], a.seconds, block) for v in VARIANTS}
                lines.append(dict(n=n, stepper=stepper, round=rnd, **r, msw_over_rsw=r["modified"] / r["rsw"],
                                  lsw_over_rsw=r["lindborg"] / r["rsw"]))
                print(json.dumps(lines[-1]), flush=True)
            for v in VARIANTS:
                lines.append(dict(n=n, stepper=stepper, model=v, profile=profile(probs[v])))
                print(json.dumps(lines[-1]), flush=True)
                probs[v].close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
