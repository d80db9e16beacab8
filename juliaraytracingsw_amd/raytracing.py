"""Wave packets traced through the evolving flow on the device
(raytracing/GPURaytracing.jl, raytracing/RaytracingDriver.jl:250-288).

The reference follows every flow step with ``get_velocity_info`` (five inverse
transforms of the ray streamfunction) and ``raytrace!`` (an ODE solve over the
packets with bilinear texture reads).  Here both stay in libsw next to the
state (``sw_rays_*``): ``Rays.step(n)`` is n × {flow step,
snapshot, packet advance} with no host round trip.
"""
from __future__ import annotations

import numpy as np

from . import _lib

PSI = {"default": _lib.SW_RAYS_PSI_DEFAULT, "layer1": _lib.SW_RAYS_PSI_LAYER1, "layer2": _lib.SW_RAYS_PSI_LAYER2}
BLEND = {"linear": _lib.SW_RAYS_BLEND_LINEAR, "new": _lib.SW_RAYS_BLEND_NEW}


def generate_initial_wavepackets(L, k0, sqrt_npackets):
    """``generate_initial_wavepackets`` (raytracing/RaytracingDriver.jl:27-47):
    packets at the midpoints of a sqrt_npackets² lattice over [-L/2, L/2]², x
    running fastest; wavenumbers of magnitude k0 at the phases 2π J/N, J = 1 … N;
    frequency signs alternating, the first packet negative.
    Returns ``(packets (N, 4): x, y, k, l; frequency_sign (N,))``."""
    s = int(sqrt_npackets)
    n = s * s
    mid = (np.arange(s) + 0.5) * (L / s) - L / 2
    phase = 2 * np.pi * np.arange(1, n + 1) / n
    packets = np.column_stack([np.tile(mid, s), np.repeat(mid, s), k0 * np.cos(phase), k0 * np.sin(phase)])
    sign = np.where(np.arange(n) % 2 == 0, -1.0, 1.0)
    return packets, sign


class Rays:
    """The ray set of ``prob`` (one per problem): ``packets`` (n, 4) = x, y, k,
    l and ``frequency_sign`` (n,) of ±1, with the packet physics ``f``, ``Cg``.

    ``psi``: "default" (RSW: the QG streamfunction of rsw/RSWRaytracingDriver.jl
    :63-67; two-layer models: the baroclinic (ψ1 − ψ2)/2; SWQG: its own ψ,
    swqg/RaytracingDriver.jl:251), "layer1", "layer2" (two-layer models only).
    The stationary background flow of swqg/RaytracingParameters.jl is one
    ``snapshot()`` followed by repeated ``advance()``, with no flow step between.
    ``blend``: "linear" (the field interpolated from the old to the new
    snapshot over an advance) or "new" (frozen at the newest snapshot, what the
    reference effectively integrates through).
    ``unbatched``: False (the default) forms a snapshot with the batched kernel
    pair: three column inverses of ψ, l ψ, l² ψ and one row pass that writes the
    texels.  True runs the five one-field inverses and the pack kernel, the
    slower reference path kept for tests and A/B timing; the two agree to
    rounding."""

    def __init__(self, prob, packets, frequency_sign, *, f, Cg, psi="default", blend="linear", unbatched=False):
        if psi not in PSI or blend not in BLEND:
            raise ValueError(f"psi must be one of {list(PSI)} and blend one of {list(BLEND)}")
        xk = np.asarray(packets, dtype=np.float64)
        if xk.ndim != 2 or xk.shape[1] != 4:
            raise ValueError(f"packets must be (n, 4), got {xk.shape}")
        self.prob, self._ctx = prob, prob.ctx
        self._ctx.rays_create(xk.T, frequency_sign, f=f, Cg=Cg, psi=PSI[psi], blend=BLEND[blend],
                              unbatched=unbatched)
        self.n = xk.shape[0]

    def snapshot(self):
        """old ← new; new ← u, v, u_x, u_y, v_x of the current state
        (``get_velocity_info``).  The first call fills both."""
        self._ctx.rays_snapshot()

    def advance(self, duration, nsub=1):
        """``raytrace!`` over ``duration``: nsub classical RK4 substeps."""
        self._ctx.rays_advance(duration, nsub)

    def step(self, nsteps, nsub=1):
        """nsteps × {``stepforward!(prob, 1)``; snapshot; advance(dt, nsub)}."""
        self._ctx.rays_step(nsteps, nsub)

    @property
    def packets(self):
        """A host copy of the packets, (n, 4): x, y, k, l."""
        return np.ascontiguousarray(self._ctx.rays_get().T)

    def sample(self):
        """``savepacketdata!``: the newest snapshot at the packets →
        ``(U (n, 2): u, v; gradU (n, 4): u_x, u_y, v_x, v_y)``."""
        U, G = self._ctx.rays_sample()
        return np.ascontiguousarray(U.T), np.ascontiguousarray(G.T)

    def close(self):
        if self._ctx is not None:
            self._ctx.rays_destroy()
            self._ctx = None
