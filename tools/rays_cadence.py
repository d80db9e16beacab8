#!/usr/bin/env python3
"""Ray-tracing cadence: the per-step loop of the reference's
ray-tracing drivers (raytracing/RaytracingDriver.jl:250-288: flow step,
get_velocity_info, raytrace!) at its two GPU configurations and one larger:

    rsw512    rsw/RSWRaytracingParameters.jl        512², 16,384 packets
    qg2_512   swqg/TwoLayerRaytracingParameters.jl  512², 262,144 packets
    rsw2048   RSW 2048², 262,144 packets

    python tools/rays_cadence.py [--only NAME ...] [--seconds S] [--out FILE]
                                 [--unbatched [--rounds R]]

Per configuration, one JSON line with steps/s of
  step        sw_step alone (one block of steps)
  rays_step   sw_rays_step: step + snapshot + packet advance on the device
  host_loop   the only alternative without sw_rays_*: per step sw_step(1) plus
              five sw_get_physical downloads, the host integration counted as free
and ms per call of snapshot and advance alone (stream-synchronised wall time;
kernel times: run this tool with --only NAME --trace under a kernel tracer).

--unbatched: the batched snapshot (the default of sw_rays_create) against the
five one-field inverses (sw_rays_config.unbatched = 1) in this one process: two
problems per configuration, timed in alternating windows of --seconds, R
rounds, one JSON line per configuration, variant and round (no host_loop).

A/B of the quad split against one thread per packet (sw_rays.hip,
-DSW_RAYS_PER_THREAD): build the comparison library with
    build.build_lib(out=PATH, force=True, extra_flags=["-DSW_RAYS_PER_THREAD"])
and pass --ab PATH.  The two libraries run in alternating child processes
(A B A B …), each warmed, each window --seconds long, advance alone at 16,384
and 262,144 packets on the RSW 512² flow.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CONFIGS = {"rsw512": ("rsw", 512, 128), "qg2_512": ("qg2", 512, 512), "rsw2048": ("rsw", 2048, 512)}


def make(name, unbatched=False):
    from juliaraytracingsw_amd import Rays, drivers, generate_initial_wavepackets

    model, nx, sq = CONFIGS[name]
    prob, P = (drivers.rsw_problem if model == "rsw" else drivers.qg2_problem)(nx, "IFMAB3")
    Cg = P["Cg"] if model == "rsw" else P["background_Cg"]
    xk, sign = generate_initial_wavepackets(P["Lx"], np.sqrt(3.0) * P["f"] / Cg, sq)  # ω0 = 2f
    rays = Rays(prob, xk, sign, f=P["f"], Cg=Cg, unbatched=unbatched)
    rays.snapshot()
    return prob, rays


def rate(fn, seconds, block):
    """calls of fn(block) per second × block over a window of at least `seconds` (after a warm-up block)"""
    fn(block)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn(block)
        n += block
    return n / (time.perf_counter() - t0)


def cadence(name, seconds):
    prob, rays = make(name)
    ids = (0, 1, 2, 3, 0) if CONFIGS[name][0] == "rsw" else (0, 1, 8, 9, 5)  # five fields' worth of downloads
    g = prob.grid

    def host_loop(n):
        for _ in range(n):
            prob.stepforward(1)
            for fid in ids:
                prob.ctx.physical(fid, g.ny, g.nx)

    out = dict(config=name, nx=g.nx, packets=rays.n, **windows(prob, rays, seconds),
               host_loop=rate(host_loop, seconds, 5))
    prob.close()
    return out


def windows(prob, rays, seconds):
    out = dict(step=rate(prob.stepforward, seconds, 100), rays_step=rate(rays.step, seconds, 100))
    out["snapshot_ms"] = 1e3 / rate(lambda n: [rays.snapshot() for _ in range(n)], seconds / 2, 20)
    out["advance_ms"] = 1e3 / rate(lambda n: [rays.advance(prob.clock.dt) for _ in range(n)], seconds / 2, 20)
    return out


def alternate(name, seconds, rounds):
    """batched and unbatched snapshots of one configuration in alternating windows"""
    sets = {"batched": make(name), "unbatched": make(name, unbatched=True)}
    lines = [dict(config=name, variant=tag, round=r, packets=rays.n, **windows(prob, rays, seconds))
             for r in range(rounds) for tag, (prob, rays) in sets.items()]
    for prob, _ in sets.values():
        prob.close()
    return lines


def ab_child(sq, seconds):
    """advance alone on the RSW 512² flow, sq² packets: ms per call (this process's library)"""
    from juliaraytracingsw_amd import Rays, drivers, generate_initial_wavepackets

    prob, P = drivers.rsw_problem(512, "IFMAB3")
    xk, sign = generate_initial_wavepackets(P["Lx"], np.sqrt(3.0) * P["f"] / P["Cg"], sq)
    rays = Rays(prob, xk, sign, f=P["f"], Cg=P["Cg"])
    rays.snapshot()
    prob.stepforward(1)
    rays.snapshot()
    print(json.dumps(dict(packets=sq * sq, advance_ms=1e3 / rate(lambda n: [rays.advance(prob.clock.dt) for _ in range(n)],
                                                                  seconds, 50))))


def ab(lib_b, seconds, rounds=3):
    res = []
    for sq in (128, 512):
        for r in range(rounds):
            for tag, lib in (("quad", None), ("per_thread", lib_b)):
                env = dict(os.environ, **({"LIBSW_PATH": lib} if lib else {}))
                o = subprocess.run([sys.executable, __file__, "--ab-child", str(sq), "--seconds", str(seconds)],
                                   env=env, capture_output=True, text=True, check=True, timeout=120)
                res.append(dict(json.loads(o.stdout.strip().splitlines()[-1]), variant=tag, round=r))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=list(CONFIGS))
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--out")
    ap.add_argument("--ab")
    ap.add_argument("--unbatched", action="store_true", help="batched against one-field snapshots, alternating windows")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ab-child", type=int)
    ap.add_argument("--trace", action="store_true", help="20 rays_step steps only (for a kernel tracer)")
    a = ap.parse_args()
    if a.ab_child:
        return ab_child(a.ab_child, a.seconds)
    lines = []
    if a.trace:
        for name in a.only:
            prob, rays = make(name)
            rays.step(20)
            prob.close()
        return
    if a.ab:
        lines = ab(a.ab, a.seconds)
    elif a.unbatched:
        lines = [ln for name in a.only for ln in alternate(name, a.seconds, a.rounds)]
    else:
        lines = [cadence(name, a.seconds) for name in a.only]
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
