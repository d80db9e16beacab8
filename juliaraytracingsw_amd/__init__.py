"""juliaraytracingsw_amd — MI355X-native pseudo-spectral time-step core.

The hot path (calcN + stepper update of the FourierFlows models used by
ndefilippis/JuliaRaytracingSW) runs in ``libsw.so``: hand-written HIP kernels
for gfx950 behind the C ABI of ``include/sw.h``.  This package is the host-side
mirror of the reference's module interfaces:

* ``rotating_shallow_water`` — rsw/RotatingShallowWater.jl
* ``modified_shallow_water`` — rsw/ModifiedShallowWater.jl (``drivers.rsw_problem(variant="modified")``)
* ``lindborg_shallow_water`` — rsw/LinborgShallowWater.jl (``variant="lindborg"``)
* ``two_layer_qg``           — swqg/TwoLayerQG.jl
* ``single_layer_qg``        — swqg/SWQG.jl (one-field shallow-water QG; ``drivers.swqg_problem``)
* ``thomas_yamada``          — thomasyamada/ThomasYamada.jl (ETDRK4)
* ``multilayer_qg``          — GeophysicalFlows MultiLayerQG (FilteredRK4), simulation/TwoLayerSimulation.jl
* ``output``                 — snapshot output / restart (FF Output, utils/SequencedOutputs.jl)
* ``drivers``                — rsw/RSWDriver.jl, swqg/TwoLayerDriver.jl setup
* ``raytracing``             — raytracing/GPURaytracing.jl, RaytracingDriver.jl: packets traced on the device
* ``budget``                 — analysis/Notebooks/rsw_suite RSWTransferFunction.jl, RSWEnergetics.jl: RSW
  wave-vortex transfers and spectra averaged on the device; ``QGBudget``: the SWQG and 2LQG transfer
  functions (analysis/Notebooks/QGTransferFunctionComputation, TwoLQGTransferFunctionComputation)
* ``komega``                 — rsw/fourier-analysis/FourierRSW.jl, swqg/fourier-analysis/Fourier*.jl,
  analysis/Notebooks/MakeOmegaKPlots.jl: wavenumber–frequency spectra recorded and transformed on the device
"""
from ._lib import LibSWError, load, LIB_PATH  # noqa: F401
from .raytracing import Rays, generate_initial_wavepackets  # noqa: F401
from .budget import Budget, QGBudget  # noqa: F401
from .komega import KOmega  # noqa: F401
from . import single_layer_qg  # noqa: F401
from . import modified_shallow_water, lindborg_shallow_water  # noqa: F401
from .drivers import swqg_problem  # noqa: F401

__all__ = ["LibSWError", "load", "LIB_PATH", "Rays", "generate_initial_wavepackets", "Budget", "QGBudget", "KOmega", "single_layer_qg",
           "swqg_problem", "modified_shallow_water", "lindborg_shallow_water"]
