#!/usr/bin/env python3
"""k–ω recorder cadence: RSW IFMAB3 with the PARTS set (or the
``--fields`` named), one recorded column and 16, against plain stepping of the
same problem in the same process.

    python tools/komega_cadence.py [--only 512 2048] [--cols 1 16] [--fields parts cubic]
                                   [--seconds S] [--no-transform] [--out FILE]

Per (grid, columns, field set) one JSON line: steps/s of sw_step alone (measured before the
recorder exists) and of ``KOmega.step`` at every = 1 and every = 10, ms per
``record`` and its ratio to one step, and ms of transform + shells (from a full
recorder to the shell power on the host side of the call, the D2H copy of the
shells included, the transform's readback not) at T = 1024 and T = 4096.  All
times are host clocks around calls that end in a stream synchronise, over
windows of at least ``--seconds`` after a warm-up block; the transform + shells
time is the median of ``--repeats`` runs, each from a freshly filled recorder.
Kernel times: run with --trace under a kernel tracer.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rate(fn, seconds, block):
    """calls of fn(block) per second × block over a window of at least `seconds` (after a warm-up block)"""
    fn(block)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn(block)
        n += block
    return n / (time.perf_counter() - t0)


def columns(ncols, kc):
    """ncols columns spread over the live band, kr = 0 among them"""
    return sorted({int(i * kc / ncols) for i in range(ncols)})


def cadence(nx, ncols, seconds, repeats, fields="parts", transform=True):
    from juliaraytracingsw_amd import KOmega, _lib, drivers

    prob, _ = drivers.rsw_problem(nx, "IFMAB3")
    cols = columns(ncols, _lib.slab_geometry(prob.ctx.cfg, 0)["kc"])
    out = dict(nx=nx, ncols=len(cols), fields=fields, step=rate(prob.stepforward, seconds, 100))
    T = 1024
    kw = KOmega(prob, T, cols, fields)

    def stepper(every):
        def run(n):  # n a multiple of `every`; the recorder is emptied when the next block would not fit
            if kw.frames + n // every > T:
                kw.reset()
            kw.step(n, every)
        return run

    def records(n):
        if kw.frames + n > T:
            kw.reset()
        for _ in range(n):
            kw.record()

    out["komega_step_every1"] = rate(stepper(1), seconds, 100)
    out["komega_step_every10"] = rate(stepper(10), seconds, 100)
    out["record_ms"] = 1e3 / rate(records, seconds, 32)
    out["record_steps"] = out["record_ms"] * 1e-3 * out["step"]
    kw.close()
    for T in (1024, 4096) if transform else ():
        kw = KOmega(prob, T, cols, fields)
        ms = []
        for _ in range(repeats + 1):  # (the first run warms the kernels up)
            kw.reset()
            kw.step(T, 1)
            t0 = time.perf_counter()
            kw.shells()
            ms.append(1e3 * (time.perf_counter() - t0))
        out[f"transform_shells_ms_T{T}"] = statistics.median(ms[1:])
        out[f"transform_shells_steps_T{T}"] = out[f"transform_shells_ms_T{T}"] * 1e-3 * out["step"]
        kw.close()
    prob.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", type=int, default=[512, 2048])
    ap.add_argument("--cols", nargs="*", type=int, default=[1, 16])
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fields", nargs="+", default=["parts"], choices=["state", "parts", "cubic", "cubic_state"],
                    help="field sets, measured in turn per (grid, columns): name a set twice for alternating windows")
    ap.add_argument("--no-transform", action="store_true", help="skip the transform + shells timing")
    ap.add_argument("--out")
    ap.add_argument("--trace", action="store_true", help="one fill, transform and shells at T = 1024 (for a kernel tracer)")
    a = ap.parse_args()
    if a.trace:
        from juliaraytracingsw_amd import KOmega, drivers

        for nx in a.only:
            prob, _ = drivers.rsw_problem(nx, "IFMAB3")
            kw = KOmega(prob, 1024, [0], a.fields[0])
            kw.step(1024, 1)
            kw.shells()
            prob.close()
        return
    lines = []
    for nx in a.only:
        for nc in a.cols:
            for fields in a.fields:
                lines.append(cadence(nx, nc, a.seconds, a.repeats, fields, not a.no_transform))
                print(json.dumps(lines[-1]), flush=True)
                if a.out:  # (written as it goes: a later configuration's failure keeps the earlier lines)
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "w") as f:
                        f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
