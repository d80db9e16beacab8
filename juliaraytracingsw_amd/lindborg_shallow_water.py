"""``LinborgShallowWater`` module mirror (rsw/LinborgShallowWater.jl; the file name's spelling is the reference's).

RSW's fields and linear operator; only the rotational (non-divergent) part of
the velocity advects u, v and η (``include/sw.h`` SW_MODEL_LSW).
The ``Problem`` keywords, ``set_solution``, ``updatevars``, the energies and
``cfl`` are ``rotating_shallow_water``'s (the reference files share them);
calcN, the linear operator and the stepping run in libsw on the GPU.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .problem import Diagnostic, Problem as _Problem, increment, stepforward  # noqa: F401
from .rotating_shallow_water import (cfl, energy, kinetic_energy, potential_energy, set_solution,  # noqa: F401
                                     updatevars)


def Problem(dev="gpu", *, nx=128, ny=None, Lx=2 * np.pi, Ly=None, nu=1.0e-16, nnu=4, f=1.0, Cg=1.0,
            stepper="IFMAB3", dt=5e-2, aliased_fraction=1 / 3, T=np.float64, use_filter=False,
            device=0, check_nan=True, nop_calcN=False, unfused=False,
            decomposition=None, aliased_state=False, **stepper_kwargs):
    """``LinborgShallowWater.Problem(dev; nx, ny, Lx, Ly, ν, nν, f, Cg, stepper, dt,
    aliased_fraction, T, use_filter, stepper_kwargs...)``: the keywords of
    ``RotatingShallowWater.Problem``.  Steppers "IFMAB3", "FilteredAB3",
    "IFMRK4", "FilteredRK4"; power-of-two grids on one device; slab
    decompositions and ``aliased_state`` are refused by libsw."""
    if dev not in ("gpu", "GPU", "GPU()"):
        raise _lib.LibSWError("libsw runs on the GPU only (dev='gpu')")
    ny = nx if ny is None else ny
    Ly = Lx if Ly is None else Ly
    params = dict(nu=float(nu), nnu=int(nnu), f=float(f), Cg=float(Cg))
    prob = _Problem(_lib.SW_MODEL_LSW, nx=nx, ny=ny, Lx=Lx, Ly=Ly, dt=dt,
                    aliased_fraction=aliased_fraction, stepper=stepper, params=params,
                    use_filter=use_filter, filter_kw=stepper_kwargs, device=device,
                    check_nan=check_nan, T=T, nop_calcN=nop_calcN, unfused=unfused,
                    **(decomposition or {}), aliased_state=aliased_state)
    prob.params["Cg2"] = float(Cg) ** 2
    return prob
