"""The mass-weighted k–ω sets (SW_KOMEGA_CUBIC, _CUBIC_STATE) against plain
fp64 numpy on host states: the split of rsw/RSWUtils.jl, np.fft.irfft2, √max(0, 1 + η),
np.fft.rfft2 (FourierRSW.jl:164-174), then clean_fft and the shells as test_gpu_komega.py.
The mu*/mv* lines are compared on all nl rows, the eta* lines on the live ones.
Tolerance: the project's 1e-10 of each reference array's maximum."""
import numpy as np
import pytest

import test_msw
from juliaraytracingsw_amd import KOmega, LibSWError, _lib, thomas_yamada as TY
from test_gpu_komega import RTOL, _clean_fft, _fields, _lib_loaded, _problem, _record_loop, _shells  # noqa: F401

pytestmark = pytest.mark.gpu


def _lsw(nx, ny):
    prob, P, grid, _ = test_msw._problem("lsw", nx, ny)
    prob.sol = 0.1 * test_msw._state(grid, P, 5)
    return dict(model="rsw", f=P["f"], Cg=P["Cg"]), grid, prob


def _cubic(p, grid, sol, fields):
    """(name → (nl, nkr), min of 1 + η_p) of one state, the Definitions read literally."""
    sol = np.where(grid.live, sol, 0)
    src = _fields(p, grid, sol, "parts" if fields == "cubic" else "state")
    out, hmin = {}, np.inf
    for sfx in ("_g", "_w") if fields == "cubic" else ("",):
        u, v, eta = (np.fft.irfft2(src[n + sfx], s=(grid.ny, grid.nx)) for n in ("u", "v", "eta"))
        s = np.sqrt(np.maximum(0, 1 + eta))
        out["mu" + sfx], out["mv" + sfx], out["eta" + sfx] = np.fft.rfft2(s * u), np.fft.rfft2(s * v), src["eta" + sfx]
        hmin = min(hmin, (1 + eta).min())
    return out, hmin


def _lines(per, name, grid, cols):
    """(ncols, nl, T) of a field; the eta lines keep zeros in the rows dealias! removes."""
    x = np.stack([f[name][:, cols] for f in per], -1).transpose(1, 0, 2)
    return x if name.startswith("m") else np.where(grid.live[:, cols].T[..., None], x, 0)


@pytest.mark.parametrize("case,fields,nx,ny", [
    ("rsw", "cubic", 32, 32), ("rsw", "cubic", 32, 64), ("rsw", "cubic", 64, 32), ("msw", "cubic", 32, 32),
    ("lsw", "cubic_state", 32, 32), ("rsw", "cubic", 1024, 32), ("rsw", "cubic", 4096, 32), ("rsw", "cubic", 32, 2048)])
def test_transform_and_shells_against_numpy(case, fields, nx, ny):
    T = 32
    p, grid, prob = _lsw(nx, ny) if case == "lsw" else _problem(case, nx, ny)
    cols = np.array([0, 1, grid.kc - 1])
    try:
        kw = KOmega(prob, T, cols, fields)
        t, sols = _record_loop(prob, kw, T, 1)
        per, hmin = zip(*[_cubic(p, grid, s, fields) for s in sols])
        assert min(hmin) > 0  # the clamp is inactive
        got, gsh = kw.transform(), kw.shells()[2]
        assert list(got) == list(per[0])
        for name in per[0]:
            X = _clean_fft(t, _lines(per, name, grid, cols), True)
            sh = _shells(grid, cols, X)
            assert np.all(np.isfinite(X)) and gsh[name].shape == sh.shape
            et, es = np.abs(got[name] - X).max() / np.abs(X).max(), np.abs(gsh[name] - sh).max() / sh.max()
            print(f"{name}: transform {et:.2e} shells {es:.2e}")
            assert et < RTOL and es < RTOL, (name, et, es)
    finally:
        prob.close()


def test_clamp():
    p, grid, prob = _problem("rsw", 32, 32)
    cols = np.array([0, 1, grid.kc - 1])
    try:
        sol = prob.sol
        eta_w = np.fft.irfft2(_fields(p, grid, sol, "parts")["eta_w"], s=(grid.ny, grid.nx))
        prob.sol = sol * (-1.5 / eta_w.min())  # the split is linear: min η_w = -1.5
        kw = KOmega(prob, 32, cols, "cubic")
        kw.record()
        ref, _ = _cubic(p, grid, prob.sol, "cubic")
        assert (1 + np.fft.irfft2(ref["eta_w"], s=(grid.ny, grid.nx))).min() < 0
        for name, x in kw.series().items():
            X = _lines([ref], name, grid, cols)[..., 0]
            assert np.abs(x[..., 0] - X).max() < RTOL * np.abs(X).max(), name
    finally:
        prob.close()


@pytest.mark.parametrize("every", [1, 3])
def test_step_is_the_manual_loop_and_leaves_stepping_alone(every):
    T, cols = 32, [0, 1, 9]
    plain = _problem("rsw", 32, 32)[2]
    plain.stepforward(T * every)
    want = plain.sol
    plain.close()
    runs = []
    for fused in (False, True, True):
        prob = _problem("rsw", 32, 32)[2]
        kw = KOmega(prob, T, cols, "cubic")
        if fused:
            kw.step(T * every, every)
        else:
            _record_loop(prob, kw, T, every)
        assert kw.frames == T and np.array_equal(prob.sol, want)
        runs.append(list(kw.series().values()) + list(kw.transform().values()) + list(kw.shells()[2].values()))
        prob.close()
    for a, b, c in zip(*runs):
        assert np.array_equal(a, b) and np.array_equal(b, c)


@pytest.mark.parametrize("make,fields", [("swqg", "cubic"), ("qg2", "cubic"), ("mlqg", "cubic_state"), ("ty", "cubic")])
def test_refusals(make, fields):
    prob = TY.Problem("gpu", nx=32) if make == "ty" else _problem(make, 32, 32)[2]
    try:
        with pytest.raises(LibSWError) as ei:
            KOmega(prob, 32, [0], fields)
        assert ei.value.code == _lib.SW_E_INVALID
    finally:
        prob.close()
