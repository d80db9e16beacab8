"""Spectral transfers and spectra of SWQG and 2LQG on the device (sw_budget_* with
SW_BUDGET_QG) against a plain fp64 numpy restatement of the
Definitions in include/sw.h, read literally: irfft2 / rfft2 on the (ny, nkr)
arrays, times grid.live.  "The model's 2×2 L" is the oracle's qg2_L
(swqg/TwoLayerQG.jl:184-198 with its Float32 literals, which the stepper carries).
Tolerance: the project's 1e-10 of each reference plane's maximum; planes that are
rounding noise in the reference (a barotropic state's baroclinic planes) are
compared on the scale of their family's barotropic plane (_scale_name).

Shapes: 32×32, 32×64, 64×32 (swapped roles) and, in each direction with the other
dimension 32, a line of every length from 128 to 8192 points: the lines per
block go 16, 8, 4, 2, 1 up to 512 points, then the block grows with the line (128,
256, 512, 1024 threads), with the halved gradient loads and the 128-VGPR column
kernels from 4096 and the 128-VGPR rows at 8192."""
import numpy as np
import pytest

import sw_oracle as O
import test_swqg as SQ
from juliaraytracingsw_amd import Budget, LibSWError, QGBudget, _lib
from juliaraytracingsw_amd.budget import SPECTRA, TRANSFERS
from test_gpu_budget import _shells
from test_gpu_rays import RTOL, _flow, _lib_loaded  # noqa: F401

pytestmark = pytest.mark.gpu
SHAPES = [(32, 32), (32, 64), (64, 32)] + [s for n in (128, 256, 512, 1024, 2048, 4096, 8192) for s in ((n, 32), (32, n))]


def _problem(model, nx, ny):
    """(p, grid, prob); 2LQG runs the driver's nonzero U, μ, ν"""
    if model == "qg2_ifmab3":
        return _flow(model, nx, ny, ic=False)
    prob, P = SQ._problem(nx, ny)
    return dict(P, model="swqg"), SQ._grid(nx, ny), prob


def _state(p, grid, kind, seed=7):
    """ "mixed": independent layers with a decaying spectrum; "barotropic": q̂₁ = q̂₂.
    Spectra of real fields, dealiased, max|q| = 1."""
    n = 1 if p["model"] == "swqg" or kind == "barotropic" else 2
    rng = np.random.default_rng(seed)
    s = grid.dealias(np.fft.rfft2(rng.standard_normal((n, grid.ny, grid.nx))) / (1 + grid.Krsq) ** 1.5)
    s = np.stack([x / np.abs(np.fft.irfft2(x, s=(grid.ny, grid.nx))).max() for x in s])
    return s if p["model"] == "swqg" or n == 2 else np.stack([s[0], s[0]])


def _reference(p, grid, sol):
    """{set: (nplanes, nl, nkr)} of one state, the Definitions read literally."""
    nx, ny, K2 = grid.nx, grid.ny, grid.Krsq
    k, l, n2 = grid.kr[None, :], grid.l[:, None], float(nx * ny) ** 2
    ir = lambda h: np.fft.irfft2(h, s=(ny, nx))  # noqa: E731
    N = lambda ps, q: -np.fft.rfft2(ir(-1j * l * ps) * ir(1j * k * q) + ir(1j * k * ps) * ir(1j * l * q)) * grid.live  # noqa: E731
    re = lambda a, b: np.real(np.conj(a) * b) / n2  # noqa: E731
    if p["model"] == "swqg":
        q, Kd2, D = sol[0], p["f"] ** 2 / p["Cg"] ** 2, -p["nu"] * K2 ** p["nnu"]
        ps = -q / (K2 + Kd2)
        T = [re(ps, N(ps, q)), re(q, N(ps, q)), re(ps, D * q), re(q, D * q)]
        S = [K2 * abs(ps) ** 2 / 2 / n2, Kd2 * abs(ps) ** 2 / 2 / n2, abs(q) ** 2 / 2 / n2]
        return {TRANSFERS: np.stack(T), SPECTRA: np.stack(S)}
    P = O.QG2Params(p["U"], p["mu"], p["nu"], p["nnu"], F=p["F"])
    ps = O.qg2_streamfunction(sol, grid, P)
    Lq = np.einsum("...rc,c...->r...", O.qg2_L(grid, P), sol)
    part = lambda x: (0.5 * (x[0] + x[1]), 0.5 * (x[0] - x[1]))  # noqa: E731
    (pT, pC), (qT, qC) = part(ps), part(sol)
    NTT, NCC, NTC, NCT = N(pT, qT), N(pC, qC), N(pT, qC), N(pC, qT)
    T = []
    for c in (ps, sol):
        cT, cC = part(c)
        T += [re(c[0], N(ps[0], sol[0])) + re(c[1], N(ps[1], sol[1])),
              2 * re(cT, NTT), 2 * re(cT, NCC), 2 * re(cC, NTC), 2 * re(cC, NCT)]
    T += [re(ps[0], Lq[0]) + re(ps[1], Lq[1]), re(sol[0], Lq[0]) + re(sol[1], Lq[1])]
    S = [K2 * abs(ps[0]) ** 2 / 2, K2 * abs(ps[1]) ** 2 / 2, P.F * abs(ps[0] - ps[1]) ** 2 / 2,
         K2 * abs(pT) ** 2, K2 * abs(pC) ** 2, abs(sol[0]) ** 2 / 2, abs(sol[1]) ** 2 / 2]
    return {TRANSFERS: np.stack(T), SPECTRA: np.stack(S) / n2}


def _scale_name(name, kind):
    """the plane whose maximum scales the comparison of ``name``"""
    if kind != "barotropic":
        return name
    if name in ("KE_C", "APE"):
        return "KE_T"
    return name[:2] + "TTT" if "C" in name else name


def _hsum(grid, plane):
    """Hermitian-weighted sum over the modes (weight 1 at kr = 0, else 2)"""
    return (np.where(np.arange(grid.nkr) == 0, 1.0, 2.0)[None, :] * plane).sum()


def _check(bud, grid, ref, kind):
    for which in (TRANSFERS, SPECTRA):
        names, got, (K, gsh) = bud.NAMES[which], bud.modes(which), bud.shells(which)
        rsh = _shells(grid, ref[which])
        assert len(K) == rsh.shape[1] and K[1] == max(2 * np.pi / grid.Lx, 2 * np.pi / grid.Ly)
        for i, name in enumerate(names):
            j = names.index(_scale_name(name, kind))
            em = np.abs(got[name] - ref[which][i]).max() / np.abs(ref[which][j]).max()
            es = np.abs(gsh[name] - rsh[i]).max() / np.abs(rsh[j]).max()
            print(f"{which} {name}: modes {em:.2e} shells {es:.2e}")
            assert em < RTOL and es < RTOL, (name, em, es)
            assert not got[name][~grid.live].any()
    got = bud.modes(TRANSFERS)
    for name in [n for n in ("E", "E_TTT", "Z") if n in got]:  # ∫ψ J(ψ, ·) = 0, ∫q J(·, q) = 0
        r = abs(_hsum(grid, got[name])) / _hsum(grid, np.abs(got[name]))
        print(f"Galerkin {name}: {r:.2e}")
        assert r < RTOL, (name, r)


CASES = [("swqg_ifmab3", "mixed"), ("qg2_ifmab3", "mixed"), ("qg2_ifmab3", "barotropic")]


@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("model,kind", CASES)
def test_planes_and_shells_against_numpy(model, kind, nx, ny):
    p, grid, prob = _problem(model, nx, ny)
    prob.sol = sol = _state(p, grid, kind)
    try:
        bud = QGBudget(prob)
        bud.accumulate()
        _check(bud, grid, _reference(p, grid, sol), kind)
    finally:
        prob.close()


def _all(bud):
    return [a for which in (TRANSFERS, SPECTRA)
            for a in list(bud.modes(which).values()) + list(bud.shells(which)[1].values())]


def test_time_mean_reset_and_bitwise_repeat():
    p, grid, prob = _problem("qg2_ifmab3", 32, 64)
    A, B = _state(p, grid, "mixed", 1), _state(p, grid, "mixed", 2)
    rA, rB = _reference(p, grid, A), _reference(p, grid, B)
    bud = QGBudget(prob)
    for s in (A, B):
        prob.sol = s
        bud.accumulate()
    assert bud.frames == 2
    _check(bud, grid, {w: 0.5 * (rA[w] + rB[w]) for w in rA}, "mixed")
    bud.reset()
    assert bud.frames == 0
    bud.accumulate()
    runs = [_all(bud)]
    prob.close()
    for _ in range(2):
        _, _, q = _problem("qg2_ifmab3", 32, 64)
        q.sol = B
        b2 = QGBudget(q)
        b2.accumulate()
        runs.append(_all(b2))
        q.close()
    for x, y, z in zip(*runs):
        assert np.array_equal(x, y) and np.array_equal(y, z)


@pytest.mark.parametrize("model", ["swqg_ifmab3", "qg2_ifmab3"])
def test_stepping_undisturbed_and_fused_loop(model):
    def fresh():
        p, grid, prob = _problem(model, 64, 64)
        prob.sol = 0.5 * _state(p, grid, "mixed")
        return prob

    plain = fresh()
    plain.stepforward(6)
    want = (plain.sol, (plain.clock.t, plain.clock.step))
    plain.close()
    out = []
    for fused in (True, False):
        prob = fresh()
        bud = QGBudget(prob)
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
    def code(f):
        with pytest.raises(LibSWError) as ei:
            f()
        return ei.value.code

    probs = [_flow(c, 32, 32, ic=False)[2] for c in ("rsw_ifmab3", "mlqg_frk4", "ty_etdrk4", "qg2_ifmab3")]
    try:
        for prob in probs[:3]:
            assert code(lambda: QGBudget(prob)) == _lib.SW_E_INVALID
        qg = probs[3]
        assert code(lambda: QGBudget(qg, spectra=False, transfers=False)) == _lib.SW_E_INVALID  # the QG bit alone
        assert code(lambda: Budget(qg)) == _lib.SW_E_INVALID  # what = 3
        assert code(lambda: qg.ctx.budget_create(8 | 3)) == _lib.SW_E_INVALID
        bud = QGBudget(qg, transfers=False)
        assert code(lambda: bud.modes(SPECTRA)) == _lib.SW_E_STATE  # before the first frame
        bud.accumulate()
        assert code(lambda: bud.modes(TRANSFERS)) == _lib.SW_E_INVALID  # a set it was not created with
    finally:
        for prob in probs:
            prob.close()
