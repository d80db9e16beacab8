"""``SWQG`` module mirror (swqg/SWQG.jl): the single-layer shallow-water QG
model.

Same names, argument meaning and defaults as the reference's ``Problem``
(:70-99).  One spectral field q̂ with ψ̂ = -q̂/(K² + Kd²), Kd² = f²/Cg² (:88,
:105-107), the Jacobian calcN (:140-170) and the real diagonal L = -ν K^(2nν)
(:181-191); "IFMAB3" is the ``diagonal=true`` branch of utils/IFMAB3.jl (a real
factor exp(L dt) per mode).  ``prob.sol`` is numpy ``(1, nl, nkr)``, the memory
of Julia's ``(nkr, nl, 1)``.  Stochastic forcing (``calcF!``) is not carried.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .problem import Diagnostic, Problem as _Problem, increment, stepforward  # noqa: F401


def Problem(dev="gpu", *, nx=128, ny=None, Lx=2 * np.pi, Ly=None, nu=1.0e-16, nnu=4, f=1.0, Cg=1.0,
            stepper="IFMAB3", dt=5e-2, aliased_fraction=1 / 3, T=np.float64, use_filter=False,
            device=0, check_nan=True, unfused=False, **stepper_kwargs):
    """``SWQG.Problem(dev; nx, ny, Lx, Ly, ν, nν, f, Cg, stepper, dt,
    aliased_fraction, T, use_filter, stepper_kwargs...)`` (:70-99).

    ``T`` is the element type of the caller-side arrays (``prob.sol``,
    ``updatevars``); libsw computes in fp64 either way.  Steppers: "IFMAB3",
    "FilteredAB3", "IFMRK4", "FilteredRK4".  Power-of-two grids on one GPU."""
    if dev not in ("gpu", "GPU", "GPU()"):
        raise _lib.LibSWError("libsw runs on the GPU only (dev='gpu')")
    ny = nx if ny is None else ny
    Ly = Lx if Ly is None else Ly
    params = dict(nu=float(nu), nnu=int(nnu), f=float(f), Cg=float(Cg))
    return _Problem(_lib.SW_MODEL_SWQG, nx=nx, ny=ny, Lx=Lx, Ly=Ly, dt=dt,
                    aliased_fraction=aliased_fraction, stepper=stepper, params=params,
                    use_filter=use_filter, filter_kw=stepper_kwargs, device=device,
                    check_nan=check_nan, T=T, unfused=unfused)


def Kd2(prob):
    """``params.Kd2`` = f²/Cg² (:88)."""
    return prob.params["f"] ** 2 / prob.params["Cg"] ** 2


def set_solution(prob, psi0h):
    """``set_solution!(prob, ψ0h)`` (:193-203): q̂ = -(K² + Kd²) ψ̂0
    (pvfromstreamfunction!), uploaded and dealiased.  ``psi0h``: [nl][nkr]."""
    psi0h = np.asarray(psi0h)
    prob.sol = (-(prob.grid.Krsq + Kd2(prob)) * psi0h.reshape(prob.grid.Krsq.shape))[None]


def updatevars(prob):
    """``updatevars!(prob)`` (:109-125): q, ψ, ζ, u, v of the dealiased state,
    each [ny][nx]."""
    g = prob.grid
    ids = (("q", _lib.SW_PHYS_Q), ("psi", _lib.SW_PHYS_PSI), ("zeta", _lib.SW_PHYS_ZETA),
           ("u", _lib.SW_PHYS_U), ("v", _lib.SW_PHYS_V))
    return {name: prob.ctx.physical(fid, g.ny, g.nx) for name, fid in ids}


def kinetic_energy(prob):
    """``kinetic_energy(prob)`` (:205-212): parsevalsum2(K ψ̂)/(2 Lx Ly)."""
    return prob.ctx.diag(_lib.SW_DIAG_KE)


def potential_energy(prob):
    """``potential_energy(prob)`` (:215-221): Kd² parsevalsum2(ψ̂)/(2 Lx Ly)."""
    return prob.ctx.diag(_lib.SW_DIAG_PE)


def energy(prob):
    """``energy(prob)`` (:223-225)."""
    return kinetic_energy(prob) + potential_energy(prob)


def cfl(prob):
    """clock.dt · max(max|u|/dx, max|v|/dy) (swqg/SWQGDriver.jl:91-92),
    reduced on the device."""
    return prob.ctx.diag(_lib.SW_DIAG_CFL)


kinetic_energy._sw_energy = "ke"
potential_energy._sw_energy = "pe"
