"""Wave-packet ray tracing on the device (sw_rays_*) against a
plain fp64 numpy restatement: the five fields of get_velocity_info
(raytracing/RaytracingDriver.jl:132-154) by numpy.fft.irfft2 from prob.sol,
periodic bilinear sampling at the grid nodes, classical RK4 of dxkdt
(raytracing/GPURaytracing.jl:32-65).  Tolerance: the project's parity 1e-10 as
max|a−b|/scale — positions against L, wavenumbers against max|k|, fields
against max|field|."""
import functools

import numpy as np
import pytest

import sw_cases
import sw_oracle as O
from juliaraytracingsw_amd import LibSWError, Rays, _lib

pytestmark = pytest.mark.gpu

RTOL = 1e-10
F_PKT, CG_PKT = 3.0, 1.5  # packet physics (their own, not the flow's)


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded(libsw):
    return libsw


def _flow(case, nx, ny, ic=True, **kw):
    p = sw_cases.case_params(case, nx)
    grid = O.TwoDGrid(nx, ny=ny, aliased_fraction=p.get("af", 1 / 3))
    prob = sw_cases.libsw_problem(p, ny=ny, **kw)
    if ic:
        prob.sol = sw_cases.initial_condition(p, grid)
    return p, grid, prob


def _fields(p, grid, sol, psi="default"):
    """(5, ny, nx): u, v, u_x, u_y, v_x of the ray streamfunction of ``sol``."""
    k, l = grid.kr[None, :], grid.l[:, None]
    if p["model"] == "rsw":  # rsw/RSWRaytracingDriver.jl:63-67
        ph = (1j * k * sol[1] - 1j * l * sol[0] - p["f"] * sol[2]) / -(grid.Krsq + p["f"] ** 2 / p["Cg"] ** 2)
    else:
        if p["model"] == "mlqg":
            ps = O.mlqg_streamfunction(sol, grid, O.MLQGParams(p["f0"], p["H"], p["b"], p["U"], p["mu"]))
        else:
            ps = O.qg2_streamfunction(sol, grid, O.QG2Params(p["U"], p["mu"], p["nu"], p["nnu"], F=p["F"]))
        ph = {"default": 0.5 * (ps[0] - ps[1]), "layer1": ps[0], "layer2": ps[1]}[psi]
    spec = [-1j * l * ph, 1j * k * ph, k * l * ph, l * l * ph, -k * k * ph]
    return np.stack([np.fft.irfft2(s, s=(grid.ny, grid.nx)) for s in spec])


def _bilinear(grid, F, x, y):
    """(5, n): periodic bilinear, nodes at x_i = -Lx/2 + i dx, y_j = -Ly/2 + j dy."""
    s, t = (x + grid.Lx / 2) / grid.dx, (y + grid.Ly / 2) / grid.dy
    i0, j0 = np.floor(s).astype(int), np.floor(t).astype(int)
    fx, fy = s - i0, t - j0
    i0, j0, i1, j1 = i0 % grid.nx, j0 % grid.ny, (i0 + 1) % grid.nx, (j0 + 1) % grid.ny
    return ((1 - fx) * (1 - fy) * F[:, j0, i0] + fx * (1 - fy) * F[:, j0, i1]) + \
           ((1 - fx) * fy * F[:, j1, i0] + fx * fy * F[:, j1, i1])


def _rk4(grid, Fo, Fn, xk, sg, T, nsub, blend):
    def rhs(s, a):
        Fa = _bilinear(grid, Fn, s[:, 0], s[:, 1])
        if blend == "linear":
            Fa = (1 - a) * _bilinear(grid, Fo, s[:, 0], s[:, 1]) + a * Fa
        u, v, ux, uy, vx = Fa
        k, l = s[:, 2], s[:, 3]
        om = sg * np.sqrt(F_PKT ** 2 + CG_PKT ** 2 * (k * k + l * l))
        return np.stack([u + CG_PKT ** 2 * k / om, v + CG_PKT ** 2 * l / om, -(ux * k + vx * l), -(uy * k - ux * l)], 1)

    h = T / nsub
    for m in range(nsub):
        k1 = rhs(xk, m / nsub)
        k2 = rhs(xk + h / 2 * k1, (m + 0.5) / nsub)
        k3 = rhs(xk + h / 2 * k2, (m + 0.5) / nsub)
        k4 = rhs(xk + h * k3, (m + 1) / nsub)
        xk = xk + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return xk


def _packets(grid, n, seed=7, span=3.0):
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 2 * np.pi, n)
    xk = np.column_stack([rng.uniform(-span, span, n) * grid.Lx, rng.uniform(-span, span, n) * grid.Ly,
                          5 * np.cos(ph), 5 * np.sin(ph)])
    return xk, np.where(np.arange(n) % 2 == 0, -1.0, 1.0)


def _field_errors(U, G, ref):
    """sample() against ref (5, n) fields, each relative to the reference field's max"""
    got = np.column_stack([U, G])  # u v ux uy vx vy
    want = np.vstack([ref, -ref[2:3]]).T
    return np.max(np.abs(got - want), 0) / np.max(np.abs(want), 0)


def _packet_errors(a, b, grid):
    return max(np.max(np.abs(a[:, :2] - b[:, :2])) / grid.Lx, np.max(np.abs(a[:, 2:] - b[:, 2:])) / np.max(np.abs(b[:, 2:])))


@pytest.mark.parametrize("case,psi", [("rsw_ifmab3", "default"), ("qg2_ifmab3", "default"), ("qg2_ifmab3", "layer1"),
                                      ("qg2_ifmab3", "layer2"), ("mlqg_frk4", "default")])
def test_fields_at_the_nodes(case, psi):
    p, grid, prob = _flow(case, 32, 64)
    X, Y = np.meshgrid(grid.x, grid.y)
    xk = np.column_stack([X.ravel(), Y.ravel(), np.ones(X.size), np.ones(X.size)])
    rays = Rays(prob, xk, np.ones(X.size), f=F_PKT, Cg=CG_PKT, psi=psi)
    rays.snapshot()
    e = _field_errors(*rays.sample(), _fields(p, grid, prob.sol, psi).reshape(5, -1))
    prob.close()
    assert np.all(e < RTOL), e


def test_off_node_sampling_and_wrap():
    p, grid, prob = _flow("rsw_ifmab3", 32, 64)
    xk, sg = _packets(grid, 257)
    xk[0, :2] = grid.x[3], grid.y[5]                                         # an exact node
    xk[1, :2] = grid.x[-1] + 0.3 * grid.dx, grid.y[-1] + 0.6 * grid.dy       # the last cell: wraps to 0
    xk[2, :2] = grid.x[-1], grid.y[-1] + 0.25 * grid.dy
    xk[3, :2] = -grid.Lx / 2 + grid.Lx, -grid.Ly / 2 + grid.Ly                # the period exactly
    xk[4, :2] = np.nextafter(-grid.Lx / 2, -np.inf), -grid.Ly / 2 - 2 * grid.Ly  # just below node 0
    rays = Rays(prob, xk, sg, f=F_PKT, Cg=CG_PKT)
    rays.snapshot()
    e = _field_errors(*rays.sample(), _bilinear(grid, _fields(p, grid, prob.sol), xk[:, 0], xk[:, 1]))
    assert np.array_equal(rays.packets, xk)  # positions are never wrapped in storage
    prob.close()
    assert np.all(e < RTOL), e


@functools.lru_cache(None)
def _evolving_fields(case, n, nsteps):
    """the fields of the state after 0 … nsteps flow steps (stepping is deterministic)"""
    p, grid, prob = _flow(case, n, n)
    out = [_fields(p, grid, prob.sol)]
    for _ in range(nsteps):
        prob.stepforward(1)
        out.append(_fields(p, grid, prob.sol))
    prob.close()
    return out


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("blend", ["linear", "new"])
@pytest.mark.parametrize("nsub", [1, 3])
def test_trace_through_an_evolving_flow(nsub, blend, n):
    F = _evolving_fields("rsw_ifmab3", 64, 3)
    p, grid, prob = _flow("rsw_ifmab3", 64, 64)
    xk, sg = _packets(grid, n, span=1.0)
    rays = Rays(prob, xk, sg, f=F_PKT, Cg=CG_PKT, blend=blend)
    rays.snapshot()
    ref = xk
    for s in range(3):
        prob.stepforward(1)
        rays.snapshot()
        rays.advance(p["dt"], nsub)
        ref = _rk4(grid, F[s], F[s + 1], ref, sg, p["dt"], nsub, blend)
    e = _packet_errors(rays.packets, ref, grid)
    prob.close()
    assert e < RTOL, e


def test_closed_form_in_a_flow_at_rest():
    p, grid, prob = _flow("rsw_ifmab3", 32, 64, ic=False)
    xk, sg = _packets(grid, 257)
    rays = Rays(prob, xk, sg, f=F_PKT, Cg=CG_PKT)
    rays.snapshot()
    rays.advance(0.7, 2)
    om = sg * np.sqrt(F_PKT ** 2 + CG_PKT ** 2 * (xk[:, 2] ** 2 + xk[:, 3] ** 2))
    want = xk.copy()
    want[:, :2] += CG_PKT ** 2 * xk[:, 2:] / om[:, None] * 0.7
    got = rays.packets
    prob.close()
    assert np.array_equal(got[:, 2:], xk[:, 2:]) and _packet_errors(got, want, grid) < RTOL


@pytest.mark.parametrize("case", ["rsw_fab3", "rsw_ifmab3", "qg2_ifmab3"])
def test_stepping_undisturbed(case):
    p, grid, a = _flow(case, 64, 64)
    _, _, b = _flow(case, 64, 64)
    rays = Rays(b, *_packets(grid, 257), f=F_PKT, Cg=CG_PKT)
    rays.snapshot()
    rays.step(5)
    a.stepforward(5)
    same = np.array_equal(a.sol, b.sol) and (a.clock.t, a.clock.step) == (b.clock.t, b.clock.step)
    a.close(), b.close()
    assert same


def test_fused_loop_and_slabs():
    out = []
    for fused, dec in ((True, None), (False, None), (True, dict(nranks=2, local_slabs=2))):
        p, grid, prob = _flow("rsw_ifmab3", 64, 64, decomposition=dec)
        rays = Rays(prob, *_packets(grid, 257, span=1.0), f=F_PKT, Cg=CG_PKT)
        rays.snapshot()
        if fused:
            rays.step(4, nsub=2)
        else:
            for _ in range(4):
                prob.stepforward(1)
                rays.snapshot()
                rays.advance(p["dt"], 2)
        out.append(rays.packets)
        prob.close()
    assert np.array_equal(out[0], out[1])
    assert _packet_errors(out[2], out[0], grid) < RTOL


@pytest.mark.parametrize("case,n,kw,rkw,code,why", [
    ("qg2_ifmab3", 64, dict(aliased_state=True), {}, _lib.SW_E_INVALID, "aliased_state"),
    ("ty_etdrk4", 32, {}, {}, _lib.SW_E_INVALID, "TY"),
    ("mlqg_frk4", 96, {}, {}, _lib.SW_E_INVALID, "power-of-two"),
    ("rsw_ifmab3", 32, {}, dict(psi="layer1"), _lib.SW_E_INVALID, "RSW has no layer"),
    ("rsw_ifmab3", 32, {}, {}, _lib.SW_E_STATE, "no snapshot"),
])
def test_refusals(case, n, kw, rkw, code, why):
    p, grid, prob = _flow(case, n, n, ic=False, **kw)
    with pytest.raises(LibSWError, match=why) as ei:
        Rays(prob, *_packets(grid, 5), f=F_PKT, Cg=CG_PKT, **rkw).advance(0.1)
    prob.close()
    assert ei.value.code == code
