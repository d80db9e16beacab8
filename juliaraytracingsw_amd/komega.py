"""Wavenumber–frequency (k–ω) spectra of the flow, recorded and transformed on
the device (rsw/fourier-analysis/FourierRSW.jl, swqg/fourier-analysis/
FourierSWQG.jl, Fourier2LQG.jl, thomasyamada/TY_k_omega.jl, consumed by
analysis/Notebooks/MakeOmegaKPlots.jl).

The reference saves thousands of snapshots, re-reads them in a job array (one
job per few ``kr`` columns), takes the time series of every ``l`` of a column —
for RSW of its geostrophic and wave parts — and runs ``clean_fft`` (detrend,
Hann window, FFT along time); the notebook sums ``abs2`` into radial shells per
ω.  Here the series of the chosen columns is recorded next to the state
(``sw_komega_*``): ``KOmega.step(n, every)`` is n flow steps with
a frame after every ``every``-th, without a host round trip, and the transform
and the shell sums run on the device once the recorder is full.
"""
from __future__ import annotations

import numpy as np

from . import _lib

SETS = {"state": _lib.SW_KOMEGA_STATE, "psi": _lib.SW_KOMEGA_PSI, "parts": _lib.SW_KOMEGA_PARTS,
        "cubic": _lib.SW_KOMEGA_CUBIC, "cubic_state": _lib.SW_KOMEGA_CUBIC_STATE}
_SW = (_lib.SW_MODEL_RSW, _lib.SW_MODEL_MSW, _lib.SW_MODEL_LSW)


def field_names(model, fields):
    """The names of a set's fields for a model, in the library's order."""
    if fields == "parts":
        return ("u_g", "v_g", "eta_g", "u_w", "v_w", "eta_w")
    if fields == "cubic":
        return ("mu_g", "mv_g", "eta_g", "mu_w", "mv_w", "eta_w")
    if fields == "cubic_state":
        return ("mu", "mv", "eta")
    one = model == _lib.SW_MODEL_SWQG
    if fields == "psi":
        return ("psi",) if one else ("psi1", "psi2")
    return ("u", "v", "eta") if model in _SW else (("q",) if one else ("q1", "q2"))


class KOmega:
    """The k–ω recorder of ``prob`` (one per problem): ``nframes`` = T frames (a
    power of two in 32 … 8192) of a field set at the 0-based ``kr`` column
    indices ``columns`` (None: every live column).  Field sets: "state" (the
    model's state fields), "psi" (SWQG ψ; 2LQG / MultiLayerQG ψ₁, ψ₂), "parts"
    (the shallow-water models' geostrophic and wave parts), "cubic" (what
    FourierRSW.jl saves: the spectra of √(1+η_p)·u_p, √(1+η_p)·v_p and η̂_p of
    each part, the ``mu*`` and ``mv*`` lines on all ``nl`` rows), "cubic_state"
    (the same of the whole state).  ``detrend=False``
    is the window alone (TY_k_omega.jl:99-104)."""

    def __init__(self, prob, nframes, columns=None, fields="parts", detrend=True):
        if fields not in SETS:
            raise ValueError(f"unknown field set {fields!r}; expected one of {list(SETS)}")
        self.prob, self._ctx, self.nframes = prob, prob.ctx, int(nframes)
        if columns is None:
            columns = np.arange(_lib.slab_geometry(prob.ctx.cfg, 0)["kc"])
        self.columns = np.asarray(columns, np.int32).ravel()
        self.names = field_names(prob.model, fields)
        self._ctx.komega_create(self.nframes, self.columns, SETS[fields], int(detrend))

    def record(self):
        """The current state's fields into the next frame."""
        self._ctx.komega_record()

    def step(self, n, every=1):
        """n × ``stepforward!(prob, 1)``, with ``record()`` after each step whose
        ``clock.step % every == 0``."""
        self._ctx.komega_step(n, every)

    def reset(self):
        """Drop the frames (and the transform): back to recording."""
        self._ctx.komega_reset()

    @property
    def frames(self):
        return self._ctx.komega_dims()[4]

    @property
    def times(self):
        """t_n of the frames recorded so far."""
        return self._ctx.komega_times()[:self.frames]

    @property
    def omega(self):
        """ω_j = 2π·fftfreq(T, Δt), Δt = (t_{T−1} − t_0)/(T−1), of the full recorder."""
        t = self._ctx.komega_times()
        return 2 * np.pi * np.fft.fftfreq(self.nframes, (t[-1] - t[0]) / (self.nframes - 1))

    def series(self):
        """name → (ncols, nl, T) complex: the frames as recorded (zero past ``frames``)."""
        return dict(zip(self.names, self._ctx.komega_lines(False).transpose(1, 0, 2, 3)))

    def transform(self):
        """name → (ncols, nl, T) complex: ``clean_fft`` of every line, frequencies
        in FFT order (``omega``), unnormalised.  Runs on the first call."""
        return dict(zip(self.names, self._ctx.komega_lines(True).transpose(1, 0, 2, 3)))

    def shells(self):
        """``(K, omega, name → (nshell, T))``: Σ h_c |X̂|² over the recorded live modes
        of shell ⌊K/dk + ½⌋ (h_c = 1 at kr = 0, else 2), K = dk · arange(nshell)."""
        P = self._ctx.komega_shells()  # (refused before the recorder is full: no ω axis yet)
        _, _, nshell, dk, _ = self._ctx.komega_dims()
        return dk * np.arange(nshell), self.omega, dict(zip(self.names, P))

    def close(self):
        if self._ctx is not None:
            self._ctx.komega_destroy()
            self._ctx = None
