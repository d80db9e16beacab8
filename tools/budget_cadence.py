#!/usr/bin/env python3
"""RSW budget cadence: one ``Budget.accumulate`` (transfers +
spectra) against one RSW IFMAB3 step, and ``Budget.step(n, every)`` at the
analysis cadence of the reference (one sample per output frame,
rsw/RSWDriver.jl:152: every = output_dt / dt steps, output_dt = 0.025/f).

    python tools/budget_cadence.py [--only 512 2048] [--seconds S] [--every N] [--out FILE]
    python tools/budget_cadence.py --qg [--only 512 2048] [--seconds S] [--every N] [--out FILE]

``--qg``: the same for ``QGBudget`` on the SWQG and 2LQG
drivers' IFMAB3 problems, one line per (model, grid); every defaults to 100
steps (the QG drivers' output cadence is set per run).

Per grid one JSON line: steps/s of sw_step alone and of sw_budget_step at
``every`` and at every = 1, ms per accumulate (transfers + spectra, spectra
alone) as stream-synchronised wall time over blocks of calls, and their ratio
to one step.  Kernel times: run with --trace under a kernel tracer.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(nx, **kw):
    from juliaraytracingsw_amd import Budget, drivers

    prob, P = drivers.rsw_problem(nx, "IFMAB3")
    return prob, P, Budget(prob, **kw)


def rate(fn, seconds, block):
    """calls of fn(block) per second × block over a window of at least `seconds` (after a warm-up block)"""
    fn(block)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn(block)
        n += block
    return n / (time.perf_counter() - t0)


def make_qg(model):
    def mk(nx, **kw):
        from juliaraytracingsw_amd import QGBudget, drivers

        prob, P = (drivers.swqg_problem if model == "swqg" else drivers.qg2_problem)(nx, "IFMAB3")
        return prob, P, QGBudget(prob, **kw)

    return mk


def cadence(nx, seconds, every, make=make, model="rsw"):
    prob, P, bud = make(nx)
    # rsw/RSWParameters.jl:23: output_dt = 0.025/f; the QG drivers set theirs per run: 100 steps
    every = every or (max(int(0.025 / P["f"] / P["dt"]), 1) if model == "rsw" else 100)
    out = dict(model=model, nx=nx, every=every, step=rate(prob.stepforward, seconds, 100))
    out["budget_step"] = rate(lambda n: bud.step(n, every), seconds, max(100, every))
    out["budget_step_every1"] = rate(lambda n: bud.step(n, 1), seconds, 20)
    out["accumulate_ms"] = 1e3 / rate(lambda n: [bud.accumulate() for _ in range(n)], seconds, 20)
    prob.close()
    prob, _, spec = make(nx, transfers=False)
    out["spectra_ms"] = 1e3 / rate(lambda n: [spec.accumulate() for _ in range(n)], seconds / 2, 20)
    prob.close()
    out["accumulate_steps"] = out["accumulate_ms"] * 1e-3 * out["step"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", type=int, default=[512, 2048])
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--every", type=int, default=0, help="0: the reference's output_dt / dt")
    ap.add_argument("--out")
    ap.add_argument("--trace", action="store_true", help="5 accumulates only (for a kernel tracer)")
    ap.add_argument("--qg", action="store_true", help="QGBudget on SWQG and 2LQG instead of the RSW budget")
    a = ap.parse_args()
    cases = [(m, make_qg(m)) for m in ("swqg", "qg2")] if a.qg else [("rsw", make)]
    if a.trace:
        for _, mk in cases:
            for nx in a.only:
                prob, _, bud = mk(nx)
                for _ in range(5):
                    bud.accumulate()
                prob.close()
        return
    lines = [cadence(nx, a.seconds, a.every, mk, m) for m, mk in cases for nx in a.only]
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
