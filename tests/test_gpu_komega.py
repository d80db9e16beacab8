"""Wavenumber–frequency spectra on the device (sw_komega_*) against
plain fp64 numpy on series collected on the host (loop: stepforward, record, keep
prob.sol): the geostrophic/wave split of rsw/RSWUtils.jl and the streamfunctions,
clean_fft of rsw/fourier-analysis/FourierRSW.jl in its centred form, np.fft.fft
along time and np.bincount for the shells of analysis/Notebooks/MakeOmegaKPlots.jl.
Tolerance: the project's 1e-10 of each reference array's maximum."""
import ctypes

import numpy as np
import pytest

import sw_oracle as O
import test_msw
import test_swqg
from juliaraytracingsw_amd import KOmega, LibSWError, _lib, multilayer_qg as MLQG, thomas_yamada as TY
from test_gpu_rays import RTOL, _flow, _lib_loaded  # noqa: F401

pytestmark = pytest.mark.gpu
CASES = {"rsw": "rsw_ifmab3", "qg2": "qg2_ifmab3", "mlqg": "mlqg_frk4"}


def _problem(case, nx, ny, **kw):
    """(p, grid, prob) with a flow in it; p: model, f, Cg and the oracle's QG parameters."""
    if case == "msw":  # a tenth of test_msw's amplitude: thousands of steps of the explicit pressure term
        prob, P, grid, _ = test_msw._problem("msw", nx, ny, **kw)
        prob.sol = 0.1 * test_msw._state(grid, P, 3)
        return dict(model="rsw", f=P["f"], Cg=P["Cg"]), grid, prob
    if case == "swqg":
        prob, P = test_swqg._problem(nx, ny, **kw)
        grid = test_swqg._grid(nx, ny)
        prob.sol = test_swqg._decaying_q(grid, 7)[None]
        return dict(model="swqg", f=P["f"], Cg=P["Cg"]), grid, prob
    return _flow(CASES[case], nx, ny, **kw)


def _fields(p, grid, sol, fields):
    """name → (nl, nkr) of one state, the Definitions read literally."""
    k, l = grid.kr[None, :], grid.l[:, None]
    if fields == "state":
        return dict(zip({1: ("q",), 2: ("q1", "q2"), 3: ("u", "v", "eta")}[len(sol)], sol))
    if fields == "psi":
        if p["model"] == "swqg":
            return {"psi": -sol[0] / (grid.Krsq + p["f"] ** 2 / p["Cg"] ** 2)}
        if p["model"] == "mlqg":
            ps = O.mlqg_streamfunction(sol, grid, O.MLQGParams(p["f0"], p["H"], p["b"], p["U"], p["mu"]))
        else:
            ps = O.qg2_streamfunction(sol, grid, O.QG2Params(p["U"], p["mu"], p["nu"], p["nnu"], F=p["F"]))
        return {"psi1": ps[0], "psi2": ps[1]}
    f, Cg2 = p["f"], p["Cg"] ** 2  # rsw/RSWUtils.jl:9-20
    psi = -(1j * k * sol[1] - 1j * l * sol[0] - f * sol[2]) / (grid.Krsq + f * f / Cg2)
    g = [-1j * l * psi, 1j * k * psi, f / Cg2 * psi]
    return dict(zip(("u_g", "v_g", "eta_g", "u_w", "v_w", "eta_w"), g + [s - x for s, x in zip(sol, g)]))


def _clean_fft(t, x, detrend):
    """clean_fft along the last axis: y = x − m c, c = t − t̄, m = Σ c x / Σ c² (the
    reference's detrend(t, data), FourierRSW.jl:22-35, centred), periodic Hann, fft."""
    c = t - t.mean()
    if detrend:
        x = x - (x @ c / (c @ c))[..., None] * c
    return np.fft.fft(0.5 * (1 - np.cos(2 * np.pi * np.arange(len(t)) / len(t))) * x, axis=-1)


def _shells(grid, cols, X):
    """(nshell, T): Σ h_c |X̂|² of X (ncols, nl, T) over the live modes by ⌊K/dk + ½⌋."""
    dk = max(2 * np.pi / grid.Lx, 2 * np.pi / grid.Ly)
    live = grid.live[:, cols].T
    s = np.floor(np.sqrt(grid.Krsq[:, cols].T) / dk + 0.5).astype(int)[live]
    P = (np.where(cols == 0, 1.0, 2.0)[:, None, None] * np.abs(X) ** 2)[live]
    return np.stack([np.bincount(s, weights=P[:, j], minlength=s.max() + 1) for j in range(X.shape[-1])], 1)


def _record_loop(prob, kw, T, every):
    """The manual loop; (t, the host states (T, nf, nl, nkr))."""
    sols, t = [], []
    for _ in range(T):
        prob.stepforward(every)
        kw.record()
        sols.append(prob.sol)
        t.append(prob.clock.t)
    return np.array(t), np.stack(sols)


def _reference(p, grid, cols, t, sols, fields, detrend):
    """name → (transform (ncols, nl, T), shells (nshell, T)) from the host states."""
    per = [_fields(p, grid, s, fields) for s in sols]
    out = {}
    for name in per[0]:
        x = np.stack([f[name][:, cols] for f in per], -1).transpose(1, 0, 2)  # (ncols, nl, T)
        X = _clean_fft(t, np.where(grid.live[:, cols].T[..., None], x, 0), detrend)
        out[name] = (X, _shells(grid, cols, X))
    return out


def _check(kw, ref, grid, cols, transform=True):
    K, om, gsh = kw.shells()
    got = kw.transform() if transform else {}
    for name, (X, sh) in ref.items():
        assert gsh[name].shape == sh.shape
        es = np.abs(gsh[name] - sh).max() / sh.max()
        et = np.abs(got[name] - X).max() / np.abs(X).max() if transform else 0.0
        print(f"{name}: transform {et:.2e} shells {es:.2e}")
        assert et < RTOL and es < RTOL, (name, et, es)
        if transform:
            assert not got[name][~grid.live[:, cols].T].any()
    assert K[1] == max(2 * np.pi / grid.Lx, 2 * np.pi / grid.Ly)
    return om


@pytest.mark.parametrize("case,fields,nx,ny,T,detrend", [
    ("rsw", "parts", 32, 32, 32, True), ("rsw", "parts", 32, 64, 256, True), ("rsw", "parts", 64, 32, 256, True),
    ("msw", "state", 32, 32, 2048, True), ("swqg", "psi", 32, 32, 8192, True), ("qg2", "psi", 32, 32, 64, False),
    ("mlqg", "state", 32, 32, 4096, True)])
def test_transform_and_shells_against_numpy(case, fields, nx, ny, T, detrend):
    p, grid, prob = _problem(case, nx, ny)
    cols = np.array([0, 1, grid.kc - 1])
    try:
        kw = KOmega(prob, T, cols, fields, detrend)
        t, sols = _record_loop(prob, kw, T, 1)
        assert np.array_equal(kw.times, t)
        om = _check(kw, _reference(p, grid, cols, t, sols, fields, detrend), grid, cols)
        ref_om = 2 * np.pi * np.fft.fftfreq(T, (t[-1] - t[0]) / (T - 1))
        assert np.abs(om - ref_om).max() <= 1e-14 * np.abs(ref_om).max()
    finally:
        prob.close()


@pytest.mark.parametrize("every", [1, 3])
def test_step_is_the_manual_loop_and_leaves_stepping_alone(every):
    T, cols = 32, [0, 1, 9]
    _, _, plain = _problem("rsw", 32, 32)
    plain.stepforward(T * every)
    want = plain.sol
    plain.close()
    runs = []
    for fused in (False, True, True):
        _, _, prob = _problem("rsw", 32, 32)
        kw = KOmega(prob, T, cols, "parts")
        if fused:
            kw.step(T * every, every)
        else:
            _record_loop(prob, kw, T, every)
        assert kw.frames == T and np.array_equal(prob.sol, want)
        runs.append(list(kw.series().values()) + list(kw.transform().values()) + list(kw.shells()[2].values()))
        prob.close()
    for a, b, c in zip(*runs):
        assert np.array_equal(a, b) and np.array_equal(b, c)


def test_all_live_columns_shells():
    p, grid, prob = _problem("rsw", 32, 32)
    try:
        kw = KOmega(prob, 32)
        assert np.array_equal(kw.columns, np.arange(grid.kc))
        t, sols = _record_loop(prob, kw, 32, 1)
        _check(kw, _reference(p, grid, kw.columns, t, sols, "parts", True), grid, kw.columns, transform=False)
    finally:
        prob.close()


def _full(prob, **kw):
    k = KOmega(prob, 32, [0, 1], "state", **kw)
    k.step(32, 1)
    return k


def _bytes(prob):
    KOmega(prob, 32, [0], "state")
    buf = np.empty(31)
    rc = prob.ctx.lib.sw_komega_get_times(prob.ctx._h, ctypes.c_void_p(buf.ctypes.data), buf.nbytes)
    prob.ctx._check(rc, "sw_komega_get_times")


REFUSALS = {  # name: (a case of _problem or a constructor, the refused call, the code)
    "ty": (lambda: TY.Problem("gpu", nx=32), lambda q: KOmega(q, 32, [0], "state"), _lib.SW_E_INVALID),
    "generic": (lambda: MLQG.Problem(2, "gpu", nx=96, ny=48), lambda q: KOmega(q, 32, [0], "state"),
                _lib.SW_E_INVALID),
    "slabs": (lambda: _problem("rsw", 64, 64, decomposition=dict(nranks=2, local_slabs=2))[2],
              lambda q: KOmega(q, 32, [0]), _lib.SW_E_INVALID),
    "aliased_state": (lambda: _problem("rsw", 32, 32, aliased_state=True)[2], lambda q: KOmega(q, 32, [0]),
                      _lib.SW_E_INVALID),
    "rsw_psi": ("rsw", lambda q: KOmega(q, 32, [0], "psi"), _lib.SW_E_INVALID),
    "qg2_parts": ("qg2", lambda q: KOmega(q, 32, [0], "parts"), _lib.SW_E_INVALID),
    "T_48": ("rsw", lambda q: KOmega(q, 48, [0]), _lib.SW_E_INVALID),
    "T_16": ("rsw", lambda q: KOmega(q, 16, [0]), _lib.SW_E_INVALID),
    "T_16384": ("rsw", lambda q: KOmega(q, 16384, [0]), _lib.SW_E_INVALID),
    "cols_empty": ("rsw", lambda q: KOmega(q, 32, []), _lib.SW_E_INVALID),
    "cols_unsorted": ("rsw", lambda q: KOmega(q, 32, [2, 1]), _lib.SW_E_INVALID),
    "cols_duplicate": ("rsw", lambda q: KOmega(q, 32, [1, 1]), _lib.SW_E_INVALID),
    "cols_negative": ("rsw", lambda q: KOmega(q, 32, [-1, 0]), _lib.SW_E_INVALID),
    "cols_dealiased": ("rsw", lambda q: KOmega(q, 32, [0, 10]), _lib.SW_E_INVALID),
    "cols_out_of_range": ("rsw", lambda q: KOmega(q, 32, [0, 17]), _lib.SW_E_INVALID),
    "detrend_2": ("rsw", lambda q: KOmega(q, 32, [0], detrend=2), _lib.SW_E_INVALID),
    "bytes": ("rsw", _bytes, _lib.SW_E_INVALID),
    "step_too_many": ("rsw", lambda q: KOmega(q, 32, [0]).step(33, 1), _lib.SW_E_INVALID),
    "no_recorder": ("rsw", lambda q: q.ctx.komega_record(), _lib.SW_E_STATE),
    "second_create": ("rsw", lambda q: (KOmega(q, 32, [0]), KOmega(q, 32, [0])), _lib.SW_E_STATE),
    "record_full": ("rsw", lambda q: _full(q).record(), _lib.SW_E_STATE),
    "transform_early": ("rsw", lambda q: KOmega(q, 32, [0]).transform(), _lib.SW_E_STATE),
    "shells_early": ("rsw", lambda q: KOmega(q, 32, [0]).shells(), _lib.SW_E_STATE),
    "series_after_transform": ("rsw", lambda q: (lambda k: (k.transform(), k.series()))(_full(q)), _lib.SW_E_STATE),
    "record_after_transform": ("rsw", lambda q: (lambda k: (k.shells(), k.record()))(_full(q)), _lib.SW_E_STATE),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(name):
    make, call, code = REFUSALS[name]
    prob = _problem(make, 32, 32)[2] if isinstance(make, str) else make()
    try:
        with pytest.raises(LibSWError) as ei:
            call(prob)
        assert ei.value.code == code
    finally:
        prob.close()
