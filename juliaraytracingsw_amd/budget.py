"""Wave-vortex spectral transfers and spectra of RSW, averaged on the device
(analysis/Notebooks/rsw_suite/RSWTransferFunction.jl, RSWEnergetics.jl).

The reference saves three-field snapshots and, offline, splits each frame into
its geostrophic and wave parts (rsw/RSWUtils.jl:wave_balanced_decomposition),
builds the triad-resolved transfers ggg / ggw / gww / www of energy and linear
potential enstrophy with some sixty 2-D FFTs, and averages over the frames.
Here the same planes accumulate in libsw next to the state (``sw_budget_*``,
DESIGN.md §12): ``Budget.step(n, every)`` is n flow steps with a sample after
every ``every``-th, with no host round trip and no snapshot download.

``QGBudget`` is the same for the QG runs (analysis/Notebooks/
QGTransferFunctionComputation, TwoLQGTransferFunctionComputation; DESIGN.md
§12.1): SWQG's energy and enstrophy transfers, and for 2LQG their split into
barotropic/baroclinic triads with the linear planes that close the budget.
"""
from __future__ import annotations

import numpy as np

from . import _lib

SPECTRA, TRANSFERS = "spectra", "transfers"
SETS = {SPECTRA: _lib.SW_BUDGET_SPECTRA, TRANSFERS: _lib.SW_BUDGET_TRANSFERS}
NAMES = {
    TRANSFERS: ("E", "E_ggg", "E_ggw", "E_gww", "E_www", "Z", "Z_ggg", "Z_ggw", "Z_gww", "Z_www"),
    SPECTRA: ("KE", "APE", "KE_g", "APE_g", "KE_w", "APE_w", "Z2", "ZETA2"),
}


QG_NAMES = {
    _lib.SW_MODEL_SWQG: {TRANSFERS: ("E", "Z", "E_lin", "Z_lin"), SPECTRA: ("KE", "APE", "Z2")},
    _lib.SW_MODEL_QG2: {
        TRANSFERS: ("E", "E_TTT", "E_TCC", "E_CTC", "E_CCT", "Z", "Z_TTT", "Z_TCC", "Z_CTC", "Z_CCT", "E_lin", "Z_lin"),
        SPECTRA: ("KE_1", "KE_2", "APE", "KE_T", "KE_C", "Z2_1", "Z2_2")},
}


class Budget:
    """The budget of an RSW ``prob`` (one per problem).  Every plane carries the
    factor 1/(nx ny)², so its Hermitian-weighted sum over the modes (weight 1 at
    kr = 0, else 2) is a domain mean; readers return the mean over the frames
    accumulated so far.  ``NAMES`` (the planes of each set, in the readers' order)
    and ``FLAGS`` (ORed into ``what``) are what a subclass for another model
    replaces (``QGBudget``)."""

    NAMES, FLAGS = NAMES, 0

    def __init__(self, prob, spectra=True, transfers=True):
        what = (SETS[SPECTRA] if spectra else 0) | (SETS[TRANSFERS] if transfers else 0) | self.FLAGS
        self.prob, self._ctx = prob, prob.ctx
        self._ctx.budget_create(what)

    def accumulate(self):
        """Add the current state's planes to the accumulators; frames += 1."""
        self._ctx.budget_accumulate()

    def step(self, n, every=1):
        """n × ``stepforward!(prob, 1)``, with ``accumulate()`` after each step whose
        ``clock.step % every == 0``."""
        self._ctx.budget_step(n, every)

    def reset(self):
        self._ctx.budget_reset()

    @property
    def frames(self):
        return self._ctx.budget_dims()[2]

    def modes(self, set):
        """name → (nl, nkr) array (numpy's view of Julia's (nkr, nl), like
        ``prob.sol``); 0 on the modes dealias! removes."""
        a = self._ctx.budget_modes(SETS[set], len(self.NAMES[set]))
        return dict(zip(self.NAMES[set], a))

    def shells(self, set):
        """``(K, name → (nshell,))``: the sums over the shells ⌊K/dk + ½⌋ of the
        live modes, K = dk · arange(nshell), dk = max(2π/Lx, 2π/Ly)."""
        nshell, dk, _ = self._ctx.budget_dims()
        a = self._ctx.budget_shells(SETS[set], len(self.NAMES[set]))
        return dk * np.arange(nshell), dict(zip(self.NAMES[set], a))

    def close(self):
        if self._ctx is not None:
            self._ctx.budget_destroy()
            self._ctx = None


class QGBudget(Budget):
    """The budget of an SWQG or 2LQG ``prob`` (``SW_BUDGET_QG``; the planes of
    ``NAMES`` are defined in include/sw.h): ``E`` is the notebooks' ``Rh``; for
    2LQG it is the sum of the four triad terms, KE_1 + KE_2 + APE is the model's
    energy density and -(E + E_lin) its tendency."""

    FLAGS = _lib.SW_BUDGET_QG

    def __init__(self, prob, spectra=True, transfers=True):
        # another model: the names are moot, sw_budget_create refuses it
        self.NAMES = QG_NAMES.get(prob.model, QG_NAMES[_lib.SW_MODEL_QG2])
        super().__init__(prob, spectra, transfers)
