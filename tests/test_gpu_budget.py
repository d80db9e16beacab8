"""RSW wave-vortex transfers and spectra on the device (sw_budget_*)
against a plain fp64 numpy restatement of analysis/Notebooks/rsw_suite
RSWTransferFunction.jl / RSWEnergetics.jl: irfft2 / rfft2 on the (ny, nkr) arrays,
Q_η in flux form, planes E and Z from the total field against the total terms.
Tolerance: the project's 1e-10 of each reference plane's maximum; planes that are
rounding noise in the reference are compared on the scale of their family
(_scale_name)."""
import numpy as np
import pytest

import sw_cases
from juliaraytracingsw_amd import Budget, LibSWError, _lib
from juliaraytracingsw_amd.budget import NAMES, SPECTRA, TRANSFERS
from test_gpu_rays import RTOL, _flow, _lib_loaded  # noqa: F401

pytestmark = pytest.mark.gpu


def _reference(p, grid, sol):
    """{set: (nplanes, nl, nkr)} of one state, the Definitions read literally."""
    nx, ny, f, Cg2 = grid.nx, grid.ny, p["f"], p["Cg"] ** 2
    k, l, n2 = grid.kr[None, :], grid.l[:, None], float(nx * ny) ** 2
    ir = lambda h: np.fft.irfft2(h, s=(ny, nx))  # noqa: E731
    rf = lambda a: np.fft.rfft2(a) * grid.live  # noqa: E731
    qh = lambda s: 1j * k * s[1] - 1j * l * s[0] - f * s[2]  # noqa: E731
    den = grid.Krsq + f * f / Cg2
    psi = np.where(den == 0, 0, -qh(sol) / np.where(den == 0, 1, den))
    g = np.stack([-1j * l * psi, 1j * k * psi, f / Cg2 * psi])
    w = sol - g

    def Q(a, b):
        ua, va, ea, ub, vb = ir(a[0]), ir(a[1]), ir(a[2]), ir(b[0]), ir(b[1])
        return np.stack([-rf(ua * ir(1j * k * b[0]) + va * ir(1j * l * b[0])),
                         -rf(ua * ir(1j * k * b[1]) + va * ir(1j * l * b[1])),
                         -1j * k * rf(ea * ub) - 1j * l * rf(ea * vb)])

    E = lambda c, q: np.real(0.5 * (np.conj(c[0]) * q[0] + np.conj(c[1]) * q[1]) + 0.5 * Cg2 * np.conj(c[2]) * q[2]) / n2  # noqa: E731
    Z = lambda c, q: np.real(np.conj(qh(c)) * (1j * k * q[1] - 1j * l * q[0] - f * q[2])) / n2  # noqa: E731
    gg, gw, ww, tt = Q(g, g), Q(g, w) + Q(w, g), Q(w, w), Q(sol, sol)
    T = []
    for F in (E, Z):
        T += [F(sol, tt), F(g, gg), F(g, gw) + F(w, gg), F(g, ww) + F(w, gw), F(w, ww)]
    ke = lambda s: 0.5 * (abs(s[0]) ** 2 + abs(s[1]) ** 2) / n2  # noqa: E731
    ape = lambda s: 0.5 * Cg2 * abs(s[2]) ** 2 / n2  # noqa: E731
    S = [ke(sol), ape(sol), ke(g), ape(g), ke(w), ape(w), abs(qh(sol)) ** 2 / n2,
         abs(1j * k * sol[1] - 1j * l * sol[0]) ** 2 / n2]
    return {TRANSFERS: np.stack(T), SPECTRA: np.stack(S)}


def _shells(grid, planes):
    """np.bincount of the live modes by ⌊K/dk + ½⌋, Hermitian weights 1 (kr = 0) or 2."""
    dk = max(2 * np.pi / grid.Lx, 2 * np.pi / grid.Ly)
    s = np.floor(np.sqrt(grid.Krsq) / dk + 0.5).astype(int)[grid.live]
    wt = np.where(np.arange(grid.nkr) == 0, 1.0, 2.0)[None, :]
    return np.stack([np.bincount(s, weights=(wt * pl)[grid.live], minlength=s.max() + 1) for pl in planes])


def _state(p, grid, kind, seed=7):
    """(a) "mixed": û, v̂, η̂ independent with a decaying spectrum; (b) "balanced": the
    g-part of a random ψ̂.  Spectra of real fields, dealiased, max|η| = 0.1."""
    rng = np.random.default_rng(seed)
    k, l = grid.kr[None, :], grid.l[:, None]
    n = 1 if kind == "balanced" else 3
    s = grid.dealias(np.fft.rfft2(rng.standard_normal((n, grid.ny, grid.nx))) / (1 + grid.Krsq) ** 1.5)
    if kind == "balanced":
        s = np.stack([-1j * l * s[0], 1j * k * s[0], p["f"] / p["Cg"] ** 2 * s[0]])
        return s * (0.1 / np.abs(np.fft.irfft2(s[2], s=(grid.ny, grid.nx))).max())
    return np.stack([x * (0.1 / np.abs(np.fft.irfft2(x, s=(grid.ny, grid.nx))).max()) for x in s])


def _scale_name(name, kind):
    """the plane whose maximum scales the comparison of ``name``"""
    if name in ("Z_gww", "Z_www"):  # zero analytically
        return "Z"
    if kind == "balanced" and name[1:] in ("_ggw", "_gww", "_www"):  # noise in the reference
        return name[0] + "_ggg"
    if kind == "balanced" and name.endswith("_w"):
        return name[:-2]
    return name


def _check(bud, grid, ref, kind):
    for which in (TRANSFERS, SPECTRA):
        got, (K, gsh) = bud.modes(which), bud.shells(which)
        rsh = _shells(grid, ref[which])
        assert len(K) == rsh.shape[1] and K[1] == max(2 * np.pi / grid.Lx, 2 * np.pi / grid.Ly)
        for i, name in enumerate(NAMES[which]):
            j = NAMES[which].index(_scale_name(name, kind))
            em = np.abs(got[name] - ref[which][i]).max() / np.abs(ref[which][j]).max()
            es = np.abs(gsh[name] - rsh[i]).max() / np.abs(rsh[j]).max()
            print(f"{which} {name}: modes {em:.2e} shells {es:.2e}")
            assert em < RTOL and es < RTOL, (name, em, es)
            assert not got[name][~grid.live].any()


@pytest.mark.parametrize("kind", ["mixed", "balanced"])
@pytest.mark.parametrize("nx,ny", [(32, 32), (32, 64), (64, 32), (4096, 32), (32, 4096), (8192, 32), (32, 8192)])
def test_planes_and_shells_against_numpy(nx, ny, kind):
    p, grid, prob = _flow("rsw_ifmab3", nx, ny, ic=False)
    prob.sol = sol = _state(p, grid, kind)
    bud = Budget(prob)
    bud.accumulate()
    try:
        _check(bud, grid, _reference(p, grid, sol), kind)
    finally:
        prob.close()


def _all(bud):
    return [a for which in (TRANSFERS, SPECTRA)
            for a in list(bud.modes(which).values()) + list(bud.shells(which)[1].values())]


def test_time_mean_and_reset():
    p, grid, prob = _flow("rsw_ifmab3", 32, 64, ic=False)
    A, B = _state(p, grid, "mixed", 1), _state(p, grid, "mixed", 2)
    rA, rB = _reference(p, grid, A), _reference(p, grid, B)
    bud = Budget(prob)
    prob.sol = A
    bud.accumulate()
    prob.sol = B
    bud.accumulate()
    assert bud.frames == 2
    _check(bud, grid, {w: 0.5 * (rA[w] + rB[w]) for w in rA}, "mixed")
    bud.reset()
    assert bud.frames == 0
    bud.accumulate()
    after_reset = _all(bud)
    prob.close()
    fresh = []
    for _ in range(2):
        _, _, q = _flow("rsw_ifmab3", 32, 64, ic=False)
        q.sol = B
        b2 = Budget(q)
        b2.accumulate()
        fresh.append(_all(b2))
        q.close()
    for x, y, z in zip(after_reset, *fresh):
        assert np.array_equal(x, y) and np.array_equal(y, z)


@pytest.mark.parametrize("case", ["rsw_fab3", "rsw_ifmab3"])
def test_stepping_undisturbed_and_fused_loop(case):
    _, _, plain = _flow(case, 64, 64)
    plain.stepforward(6)
    want = (plain.sol, (plain.clock.t, plain.clock.step))
    plain.close()
    out = []
    for fused in (True, False):
        _, _, prob = _flow(case, 64, 64)
        bud = Budget(prob)
        if fused:
            bud.step(6, every=2)
        else:
            for _ in range(6):
                prob.stepforward(1)
                if prob.clock.step % 2 == 0:
                    bud.accumulate()
        assert bud.frames == 3
        assert np.array_equal(prob.sol, want[0]) and (prob.clock.t, prob.clock.step) == want[1]
        out.append(_all(bud))
        prob.close()
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def test_refusals():
    import test_msw

    _, _, qg = _flow("qg2_ifmab3", 32, 32, ic=False)
    msw = test_msw._problem("msw", 32, 32)[0]
    _, _, rsw = _flow("rsw_ifmab3", 32, 32)
    try:
        for prob, kw in ((qg, {}), (msw, {}), (rsw, dict(spectra=False, transfers=False))):
            with pytest.raises(LibSWError) as ei:
                Budget(prob, **kw)
            assert ei.value.code == _lib.SW_E_INVALID
        with pytest.raises(LibSWError) as ei:
            Budget(rsw).modes(SPECTRA)
        assert ei.value.code == _lib.SW_E_STATE
    finally:
        for prob in (qg, msw, rsw):
            prob.close()
