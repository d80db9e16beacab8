"""The single-layer shallow-water QG model (SW_MODEL_SWQG, swqg/SWQG.jl)
against a plain fp64 numpy restatement of its equations:

  ψ̂ = -q̂/(K² + Kd²), Kd² = f²/Cg²;  N = -il F(ψx q) + ik F(ψy q) of the
  dealiased input;  L = -ν K^(2nν);  IFMAB3 with the real factor exp(L dt)
  (utils/IFMAB3.jl, diagonal = true) and FourierFlows' FilteredAB3.

Tolerance as tests/test_gpu_parity.py: max|a-b| / max|b| over the live modes
<= 1e-10; the Galerkin invariants as tests/test_gpu_invariants.py bounds the
2LQG ones (1e-15)."""
import numpy as np
import pytest

import invariants as I
import sw_oracle as O
from juliaraytracingsw_amd import _lib, drivers, single_layer_qg as SWQG
from juliaraytracingsw_amd.raytracing import Rays

RTOL = 1e-10
TOL_INV = 1e-15
gpu = pytest.mark.gpu


def _psi(q, g, Kd2):
    return -q / (g.kr[None, :] ** 2 + g.l[:, None] ** 2 + Kd2)


def ref_calcN(q, g, Kd2):
    """swqg/SWQG.jl:140-170 on q [nl][nkr] (dealiased in place)."""
    g.dealias(q)
    kr, l = g.kr[None, :], g.l[:, None]
    psi, qp = _psi(q, g, Kd2), g.irfft(q)
    A = g.rfft(g.irfft(1j * kr * psi) * qp)
    B = g.rfft(g.irfft(1j * l * psi) * qp)
    return -1j * l * A + 1j * kr * B


def ref_steps(q, g, P, stepper, nsteps):
    """nsteps of IFMAB3 (diagonal) or FilteredAB3 from rest history."""
    Kd2, dt = P["f"] ** 2 / P["Cg"] ** 2, P["dt"]
    L = -P["nu"] * (g.kr[None, :] ** 2 + g.l[:, None] ** 2) ** P["nnu"]
    E, E2 = np.exp(L * dt), np.exp(2 * L * dt)
    filt = O.makefilter(g, order=P["filter_order"])
    h1 = h2 = np.zeros_like(q)
    for step in range(nsteps):
        N = ref_calcN(q, g, Kd2)
        if stepper == "IFMAB3":
            inc = N if step < 3 else 23 / 12 * N - 16 / 12 * E * h1 + 5 / 12 * E2 * h2
            q = E * (q + dt * inc)
            h2, h1 = h1, N
        else:
            rhs = N + L * q
            inc = rhs if step < 3 else 23 / 12 * rhs - 16 / 12 * h1 + 5 / 12 * h2
            q = (q + dt * inc) * filt
            h2, h1 = h1, rhs
    return q


def _grid(nx, ny):
    return O.TwoDGrid(nx, ny=ny)


def _decaying_q(g, seed):
    K2 = g.kr[None, :] ** 2 + g.l[:, None] ** 2
    qh = g.rfft(np.random.default_rng(seed).standard_normal((g.ny, g.nx))) / (1 + K2) ** 1.5
    return g.dealias(qh)


def _problem(nx, ny, stepper="IFMAB3", **kw):
    P = drivers.swqg_parameters(nx)
    fk = {"order": P["filter_order"]} if stepper == "FilteredAB3" else {}
    prob = SWQG.Problem("gpu", nx=nx, ny=ny, Lx=P["Lx"], dt=P["dt"], f=P["f"], Cg=P["Cg"], nnu=P["nnu"],
                        nu=P["nu"], stepper=stepper, **fk, **kw)
    return prob, P


@gpu
@pytest.mark.parametrize("nx,ny", [(32, 32), (128, 64), (512, 512), (2048, 2048)])
def test_calcN(libsw, nx, ny):
    g = _grid(nx, ny)
    prob, P = _problem(nx, ny)
    q = _decaying_q(g, seed=nx + ny)
    N = prob.calcN(q[None])
    prob.close()
    ref = ref_calcN(q.copy(), g, P["f"] ** 2 / P["Cg"] ** 2)
    e = O.parity_error(N, ref[None], g)
    print(f"swqg calcN {nx}x{ny}: {e:.3e}")
    assert e < RTOL
    assert np.all(N[0][~g.live] == 0)


@gpu
@pytest.mark.parametrize("stepper", ["IFMAB3", "FilteredAB3"])
@pytest.mark.parametrize("nx,ny", [(32, 32), (128, 64), (512, 512)])
def test_steps(libsw, nx, ny, stepper):
    g = _grid(nx, ny)
    prob, P = _problem(nx, ny, stepper)
    # an O(1) flow at the driver's time step: q̂ scaled to max|u| = ag
    q = _decaying_q(g, seed=7)
    u = g.irfft(-1j * g.l[:, None] * _psi(q, g, P["f"] ** 2 / P["Cg"] ** 2))
    q *= P["ag"] / np.max(np.abs(u))
    prob.sol = q[None]
    prob.stepforward(12)  # 3 Euler start-up steps, then AB3
    got = prob.sol
    prob.close()
    e = O.parity_error(got, ref_steps(q.copy(), g, P, stepper, 12)[None], g)
    print(f"swqg {stepper} {nx}x{ny} 12 steps: {e:.3e}")
    assert e < RTOL


@gpu
def test_unfused_bitwise(libsw):
    out = []
    for unfused in (False, True):
        prob, P = _problem(512, 512, unfused=unfused)
        prob.sol = _decaying_q(_grid(512, 512), seed=3)[None]
        prob.stepforward(12)
        out.append(prob.sol)
        prob.close()
    assert np.array_equal(out[0], out[1])


@gpu
@pytest.mark.parametrize("n", [64, 512])
def test_galerkin_invariants(libsw, n):
    g = _grid(n, n)
    prob, P = _problem(n, n)
    q = I.random_real_spectrum(g, 1, seed=n + 5)
    N = prob.calcN(q)
    prob.close()
    r = {"enstrophy": I.rel(q[0], N[0]), "energy": I.rel(_psi(q[0], g, P["f"] ** 2 / P["Cg"] ** 2), N[0])}
    print(f"swqg {n}² invariants: {r}")
    assert max(r.values()) < TOL_INV, r
    assert np.max(np.abs(N)) > 0


@gpu
def test_single_mode_fields_and_energies(libsw):
    """ψ = cos(kx + ly): q = -(K² + Kd²) ψ, ζ = -K² ψ, u = l sin, v = -k sin;
    KE = K²/4, PE = Kd²/4 (the mean of cos² is 1/2)."""
    n, k, l = 64, 3, 5
    prob, P = _problem(n, n)
    g, Kd2, K2 = prob.grid, P["f"] ** 2 / P["Cg"] ** 2, k * k + l * l
    ph = k * g.x[None, :] + l * g.y[:, None]
    SWQG.set_solution(prob, np.fft.rfft2(np.cos(ph)))
    v = SWQG.updatevars(prob)
    want = {"psi": np.cos(ph), "q": -(K2 + Kd2) * np.cos(ph), "zeta": -K2 * np.cos(ph), "u": l * np.sin(ph),
            "v": -k * np.sin(ph)}
    for name, w in want.items():
        assert np.max(np.abs(v[name] - w)) < 1e-12 * np.max(np.abs(w)), name
    assert abs(SWQG.kinetic_energy(prob) - K2 / 4) < 1e-12 * K2
    assert abs(SWQG.potential_energy(prob) - Kd2 / 4) < 1e-12 * Kd2
    prob.close()


@gpu
def test_rays_sample_at_nodes(libsw):
    n = 64
    prob, P = drivers.swqg_problem(n)
    g = prob.grid
    i, j = np.meshgrid(np.arange(0, n, 4), np.arange(0, n, 4))  # 256 packets on grid nodes
    packets = np.column_stack([g.x[i.ravel()], g.y[j.ravel()], np.ones(256), np.zeros(256)])
    rays = Rays(prob, packets, np.ones(256), f=P["f"], Cg=P["Cg"])
    rays.snapshot()
    U, _ = rays.sample()
    u = prob.ctx.physical(_lib.SW_PHYS_U, n, n)
    v = prob.ctx.physical(_lib.SW_PHYS_V, n, n)
    tol = 1e-12 * np.max(np.abs(u))
    assert np.max(np.abs(U[:, 0] - u[j.ravel(), i.ravel()])) <= tol
    assert np.max(np.abs(U[:, 1] - v[j.ravel(), i.ravel()])) <= tol
    with pytest.raises(_lib.LibSWError):
        Rays(prob, packets, np.ones(256), f=P["f"], Cg=P["Cg"], psi="layer1")
    prob.close()


@pytest.mark.parametrize("kw", [dict(nx=96), dict(aliased_state=1), dict(nranks=2, local_slabs=2),
                                dict(nranks=2, local_slabs=1, rank=0), dict(stepper=_lib.SW_STEP_ETDRK4), dict(Cg=0.0)],
                         ids=["not-pow2", "aliased-state", "slabs-one-process", "slabs-many-processes", "etdrk4", "cg-zero"])
def test_refusals(libsw, kw):
    cfg = _lib.default_config()
    cfg.model, cfg.stepper, cfg.nx, cfg.ny = _lib.SW_MODEL_SWQG, _lib.SW_STEP_IFMAB3, 64, 64
    for k, v in kw.items():
        setattr(cfg, k, v)
    with pytest.raises(_lib.LibSWError) as ei:
        _lib.Context(cfg)
    assert ei.value.code == _lib.SW_E_INVALID
    assert "SWQG" in str(ei.value)
