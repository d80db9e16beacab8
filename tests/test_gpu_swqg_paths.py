"""SW_MODEL_SWQG beyond tests/test_swqg.py: its RK4 steppers, the long-line row and column kernels,
the K = 0 / Kd = 0 guard and the ABI boundary (checkpoint, history, fp32 buffers, NaN, records, CFL).

The reference is a plain fp64 numpy restatement of the four steppers for the real diagonal
L = -ν K^(2nν) (class Ref below): test_swqg.ref_steps' IFMAB3 and FilteredAB3, plus the oracle's
IFMRK4 and FilteredRK4 definitions (oracle/sw_oracle.py) written out for one field:

  IFMRK4, E = exp(L dt), H = exp(L dt/2):  k1 = N(u); k2 = N(H(u + dt/2 k1)); k3 = N(H u + dt/2 k2);
      k4 = N(E u + dt H k3);  u <- E u + dt/6 (E k1 + 2H(k2 + k3) + k4); filter
  FilteredRK4, R(x) = N(x) + L x:  R1 = R(u); R2 = R(u + dt/2 R1); R3 = R(u + dt/2 R2); R4 = R(u + dt R3);
      u <- (u + dt (R1/6 + R2/3 + R3/3 + R4/6)) filter

Tolerances are the suite's: parity_error < 1e-10 for states and N (test_swqg.RTOL, test_gpu_parity.py),
1e-12 relative for physical fields and scalar diagnostics, np.array_equal for "bitwise".

A stepped comparison is blind to N when dt·N is tiny next to q̂, so every stepped case asserts, on the
reference alone, that its state differs from the same number of linear steps (N ≡ 0) by at least 1e-4
of max|q̂| (SHARP, 10⁶ × RTOL).

The ids name the kernel variant each shape reaches, read off LenOps::row, roww, row_prunable, row_kc
(sw_kernels.hip), Geom::isplit and use_fused (sw_api.cpp):
  row: nx <= 512 Stockham, kc at compile time; 1024/2048/4096 decimated W = 2/4/8, pruned when
       8 kc <= 3 nx, kc at compile time when kc = nx/3; 8192 Stockham with stage twiddles per stage;
  column inverse: one of Q, Ψ, Ψy per block (split) for ny <= 512, all three per block above;
  step: fused k_col_step for ny <= 2048 (not FilteredRK4), col_fwd + step_elem + col_inv above."""
import numpy as np
import pytest

import sw_oracle as O
from juliaraytracingsw_amd import _lib, drivers, problem, single_layer_qg as SWQG, two_layer_qg as QG2
from test_swqg import _decaying_q, _grid, _problem, _psi, ref_calcN

RTOL, SHARP = 1e-10, 1e-4
pytestmark = pytest.mark.gpu
STEPPERS = ("IFMAB3", "FilteredAB3", "IFMRK4", "FilteredRK4")


def _kd2(P):
    return P["f"] ** 2 / P["Cg"] ** 2


def calcN_guarded(q, g, Kd2):
    """ref_calcN with ψ̂ = 0 where K² + Kd² = 0 (f = 0 at K = 0; include/sw.h)."""
    g.dealias(q)
    kr, l = g.kr[None, :], g.l[:, None]
    den = g.Krsq + Kd2
    psi, qp = np.where(den == 0, 0.0, -q / np.where(den == 0, 1.0, den)), g.irfft(q)
    A = g.rfft(g.irfft(1j * kr * psi) * qp)
    B = g.rfft(g.irfft(1j * l * psi) * qp)
    return -1j * l * A + 1j * kr * B


class Ref:
    """The four steppers on q̂ [nl][nkr] for L = -ν K^(2nν); `filt`: the filter array of the Filtered
    steppers, or of an IF stepper with use_filter; `linear`: N ≡ 0."""

    def __init__(self, q, g, P, stepper, filt=None, linear=False, calcN=ref_calcN):
        self.q, self.g, self.dt, self.stepper, self.Kd2 = q.copy(), g, P["dt"], stepper, _kd2(P)
        self.L = -P["nu"] * g.Krsq ** P["nnu"]
        self.E, self.H, self.E2 = np.exp(self.L * self.dt), np.exp(self.L * self.dt / 2), np.exp(2 * self.L * self.dt)
        if filt is None:
            filt = O.makefilter(g, order=P["filter_order"]) if stepper.startswith("Filtered") else 1.0
        self.filt, self.linear, self.calcN = filt, linear, calcN
        self.h1 = self.h2 = np.zeros_like(q)
        self.euler = 3

    def N(self, x):
        return np.zeros_like(x) if self.linear else self.calcN(x, self.g, self.Kd2)

    def reset_history(self):
        self.euler = 3

    def step(self, n=1):
        dt, L, E, H = self.dt, self.L, self.E, self.H
        for _ in range(n):
            q = self.q
            if self.stepper == "IFMAB3":
                N = self.N(q)
                inc = N if self.euler else 23 / 12 * N - 16 / 12 * E * self.h1 + 5 / 12 * self.E2 * self.h2
                q = E * (q + dt * inc)
                self.h2, self.h1 = self.h1, N
            elif self.stepper == "FilteredAB3":
                rhs = self.N(q)
                rhs = rhs + L * q  # (q dealiased in place by calcN)
                inc = rhs if self.euler else 23 / 12 * rhs - 16 / 12 * self.h1 + 5 / 12 * self.h2
                q = q + dt * inc
                self.h2, self.h1 = self.h1, rhs
            elif self.stepper == "IFMRK4":
                k1 = self.N(q)
                k2 = self.N(H * (q + dt / 2 * k1))
                k3 = self.N(H * q + dt / 2 * k2)
                k4 = self.N(E * q + dt * H * k3)
                q = E * q + dt / 6 * (E * k1 + 2 * H * (k2 + k3) + k4)
            else:
                def R(x):
                    n_ = self.N(x)
                    return n_ + L * x

                R1 = R(q)
                R2 = R(q + dt / 2 * R1)
                R3 = R(q + dt / 2 * R2)
                R4 = R(q + dt * R3)
                q = q + dt * (R1 / 6 + R2 / 3 + R3 / 3 + R4 / 6)
            self.q = q * self.filt
            self.euler = max(0, self.euler - 1)
        assert np.all(np.isfinite(self.q))  # the reference itself stays finite
        return self.q


def _fkw(stepper, P):
    """the stepper kwargs drivers.swqg_problem passes"""
    return {"order": P["filter_order"]} if stepper.startswith("Filtered") else {}


def _tall_P(nx, ny):
    """the driver's parameters at ny with dx = dy: Lx = L nx/ny, Ly = L"""
    P = drivers.swqg_parameters(ny)
    return dict(P, Lx=P["Lx"] * nx / ny, Ly=P["Lx"])


def _make(nx, ny, stepper="IFMAB3", P=None, **kw):
    """test_swqg._problem (the driver's parameters at nx, Lx = Ly = 2π), or SWQG.Problem on the given P"""
    if P is None:
        if stepper == "FilteredRK4":
            kw = dict(_fkw(stepper, drivers.swqg_parameters(nx)), **kw)
        return _problem(nx, ny, stepper, **kw)
    prob = SWQG.Problem("gpu", nx=nx, ny=ny, Lx=P["Lx"], Ly=P.get("Ly"), dt=P["dt"], f=P["f"], Cg=P["Cg"],
                        nnu=P["nnu"], nu=P["nu"], stepper=stepper, **_fkw(stepper, P), **kw)
    return prob, P


def _gridP(nx, ny, P=None, af=1 / 3):
    return O.TwoDGrid(nx, P["Lx"] if P else 2 * np.pi, ny, P.get("Ly") if P else None, af)


def _o1_state(g, P, seed=7, calcpsi=_psi, amp=1.0):
    """test_swqg.test_steps' state: a decaying spectrum scaled to max|u| = amp·ag at the driver's dt"""
    q = _decaying_q(g, seed)
    u = g.irfft(-1j * g.l[:, None] * calcpsi(q, g, _kd2(P)))
    return q * (amp * P["ag"] / np.max(np.abs(u)))


def _band_state(g, P, seed=7):
    """for the tall grids, whose kx spacing (ny/nx) leaves test_swqg's K-decaying spectrum one column:
    unit-variance noise damped by the mode *indices*, (1 + i² + j²)^-3/2, scaled to max(|u|, |v|) = ag"""
    i2 = (g.kr[None, :] * g.Lx / (2 * np.pi)) ** 2 + (g.l[:, None] * g.Ly / (2 * np.pi)) ** 2
    q = g.dealias(g.rfft(np.random.default_rng(seed).standard_normal((g.ny, g.nx))) / (1 + i2) ** 1.5)
    psi = _psi(q, g, _kd2(P))
    um = max(np.max(np.abs(g.irfft(-1j * g.l[:, None] * psi))), np.max(np.abs(g.irfft(1j * g.kr[None, :] * psi))))
    return q * (P["ag"] / um)


def _sharp(ref_q, q0, g, P, stepper, n, filt=None):
    """the reference's departure from n linear steps, over max|q̂| (live modes)"""
    lin = Ref(q0, g, P, stepper, filt=filt, linear=True).step(n)
    return np.max(np.abs(np.where(g.live, ref_q - lin, 0))) / np.max(np.abs(np.where(g.live, ref_q, 0)))


def _check_steps(prob, q0, g, P, stepper, n, tag, filt=None):
    prob.sol = q0[None]
    prob.stepforward(n)
    got = prob.sol
    prob.close()
    want = Ref(q0, g, P, stepper, filt=filt).step(n)
    e, s = O.parity_error(got, want[None], g), _sharp(want, q0, g, P, stepper, n, filt)
    print(f"swqg {tag} {stepper} {g.nx}x{g.ny} {n} steps: {e:.3e} (nonlinear part {s:.1e})")
    assert s >= SHARP
    assert e < RTOL


# --- 1. steppers ------------------------------------------------------------------------------
@pytest.mark.parametrize("stepper,nx,ny", [(s, nx, ny) for s in ("IFMRK4", "FilteredRK4") for nx, ny in ((32, 32), (128, 64))]
                         + [("IFMRK4", 512, 512)])
def test_steps_rk4(libsw, stepper, nx, ny):
    """IFMRK4: the fused four-stage k_col_step<MODEL_SWQG, L, OP_RK4>; FilteredRK4: k_step_elem<1, OP_FRK4>."""
    g = _grid(nx, ny)
    prob, P = _make(nx, ny, stepper)
    _check_steps(prob, _o1_state(g, P), g, P, stepper, 12, "rk4")


@pytest.mark.parametrize("stepper", ["IFMAB3", "IFMRK4"])
def test_if_steppers_with_filter(libsw, stepper):
    """use_filter on the IF steppers: the filter after the update (utils/IFMAB3.jl:160), with the
    kwargs the driver passes them (none: FF's defaults)."""
    nx, ny = 128, 64
    g = _grid(nx, ny)
    prob, P = _make(nx, ny, stepper, use_filter=True)
    filt = O.makefilter(g)
    assert np.min(filt[g.live]) < 0.5  # the filter reaches into the live band
    _check_steps(prob, _o1_state(g, P), g, P, stepper, 12, "use_filter", filt=filt)


# --- 2. row and column variants -----------------------------------------------------------------
CALCN_LONG = [
    pytest.param(1024, 32, id="1024x32-row-W2-pruned-kc-col-split"),
    pytest.param(4096, 32, id="4096x32-row-W8-pruned-kc-col-split"),
    pytest.param(8192, 32, id="8192x32-row-stockham-fly-kc-col-split"),
    pytest.param(32, 1024, id="32x1024-row-short-kc-col-unsplit"),
    pytest.param(32, 4096, id="32x4096-row-short-kc-col-unsplit-fly"),
    pytest.param(32, 8192, id="32x8192-row-short-kc-col-unsplit-fly"),
    pytest.param(1024, 1024, id="1024x1024-row-W2-pruned-kc-col-unsplit"),
]


@pytest.mark.parametrize("nx,ny", CALCN_LONG)
def test_calcN_long_lines(libsw, nx, ny):
    g = _grid(nx, ny)
    prob, P = _make(nx, ny)
    q = _decaying_q(g, seed=nx + ny)
    N = prob.calcN(q[None])
    prob.close()
    e = O.parity_error(N, ref_calcN(q.copy(), g, _kd2(P))[None], g)
    print(f"swqg calcN {nx}x{ny}: {e:.3e}")
    assert e < RTOL
    assert np.all(N[0][~g.live] == 0)


# On the wide grids dt ∝ 1/nx while the energetic modes sit at K ~ 1: at max|u| = ag six steps move q̂ by
# 8e-5 (nx = 1024) to 2.6e-5 (8192) of max|q̂|, under SHARP; max|u| = 8 ag (an x-CFL of 0.8 over six
# steps; the reference stays finite) gives 6.4e-4 to 2.1e-4
WIDE_AMP = 8.0
_WIDE = [(1024, 32, "row-W2-pruned-kc"), (4096, 32, "row-W8-pruned-kc"), (8192, 32, "row-stockham-fly-kc")]
_TALL = [(32, 1024, "col-unsplit-fused-step"), (32, 2048, "col-unsplit-fused-step"),
         (32, 4096, "col-separate-kernels"), (32, 8192, "col-separate-kernels")]
STEPS_LONG = [pytest.param(nx, ny, s, id=f"{nx}x{ny}-{s}-{v}") for nx, ny, v in _WIDE + _TALL for s in ("IFMAB3", "IFMRK4")] + [
    pytest.param(1024, 32, "FilteredAB3", id="1024x32-FilteredAB3-row-W2-pruned-kc"),
    pytest.param(32, 4096, "FilteredAB3", id="32x4096-FilteredAB3-col-separate-kernels")]


@pytest.mark.parametrize("nx,ny,stepper", STEPS_LONG)
def test_steps_long_lines(libsw, nx, ny, stepper):
    """6 steps: the Euler start-up plus three AB3 steps.  Wide: the driver's parameters at nx on 2π × 2π;
    tall: the driver's at ny on (2π nx/ny) × 2π, so dx = dy and the driver's dt ν kmax⁸ and CFL hold."""
    if nx >= ny:
        g = _grid(nx, ny)
        prob, P = _make(nx, ny, stepper)
        q = _o1_state(g, P, amp=WIDE_AMP)
    else:
        P = _tall_P(nx, ny)
        g = _gridP(nx, ny, P)
        prob, _ = _make(nx, ny, stepper, P)
        q = _band_state(g, P)
    _check_steps(prob, q, g, P, stepper, 6, "long lines")


ALIASED = [
    pytest.param(256, 1 / 2, id="256-af-half-row-short-runtime-kc"),
    pytest.param(1024, 1 / 2, id="1024-af-half-row-W2-pruned-runtime-kc"),
    pytest.param(256, 0.2, id="256-af-0.2-row-short-runtime-kc"),
    pytest.param(1024, 0.2, id="1024-af-0.2-row-W2-unpruned-runtime-kc"),
]


@pytest.mark.parametrize("nx,af", ALIASED)
def test_aliased_fraction_variants(libsw, nx, af):
    """aliased_fraction ≠ 1/3: kc = nx/4 (1/2: 8 kc <= 3 nx, pruned where the row is decimated) and
    kc = floor(0.4 nx) (0.2: 8 kc > 3 nx, the full decimated transforms), both with kc at run time."""
    ny = 32
    g = _gridP(nx, ny, af=af)
    assert g.kc == (nx // 4 if af == 1 / 2 else int(0.4 * nx)) and (8 * g.kc <= 3 * nx) == (af == 1 / 2)
    prob, P = _make(nx, ny, aliased_fraction=af)
    q = _decaying_q(g, seed=nx)
    N = prob.calcN(q[None])
    e = O.parity_error(N, ref_calcN(q.copy(), g, _kd2(P))[None], g)
    print(f"swqg calcN {nx}x{ny} aliased_fraction {af:.3f}: {e:.3e}")
    assert e < RTOL
    assert np.all(N[0][~g.live] == 0)
    _check_steps(prob, _o1_state(g, P, amp=WIDE_AMP), g, P, "IFMAB3", 6, f"aliased_fraction {af:.3f}")


# --- 3. K = 0 and Kd = 0 --------------------------------------------------------------------------
def test_f_zero(libsw):
    """f = 0: ψ̂(0,0) = 0 whatever q̂(0,0) (include/sw.h), no potential energy."""
    nx = ny = 64
    g = _grid(nx, ny)
    P = dict(drivers.swqg_parameters(nx), f=0.0)
    prob, _ = _make(nx, ny, "IFMAB3", P)

    def psi0(q, g_, Kd2):
        return np.where(g_.Krsq + Kd2 == 0, 0.0, -q / np.where(g_.Krsq + Kd2 == 0, 1.0, g_.Krsq + Kd2))

    q = _o1_state(g, P, seed=5, calcpsi=psi0)
    q[0, 0] += 0.7 * nx * ny
    N = prob.calcN(q[None])
    e = O.parity_error(N, calcN_guarded(q.copy(), g, 0.0)[None], g)
    print(f"swqg f=0 calcN: {e:.3e}")
    assert e < RTOL and np.all(np.isfinite(N))
    prob.sol = q[None]
    psi = SWQG.updatevars(prob)["psi"]
    assert np.all(np.isfinite(psi)) and abs(np.mean(psi)) <= 1e-12 * np.max(np.abs(psi))
    assert np.max(np.abs(psi - g.irfft(psi0(q, g, 0.0)))) <= 1e-12 * np.max(np.abs(psi))
    assert SWQG.potential_energy(prob) == 0.0
    prob.stepforward(12)
    got = prob.sol
    prob.close()
    want = Ref(q, g, P, "IFMAB3", calcN=calcN_guarded).step(12)
    assert np.all(np.isfinite(got))
    e = O.parity_error(got, want[None], g)
    s = np.max(np.abs(want - Ref(q, g, P, "IFMAB3", linear=True).step(12))[g.live]) / np.max(np.abs(want[g.live]))
    print(f"swqg f=0 IFMAB3 12 steps: {e:.3e} (nonlinear part {s:.1e})")
    assert s >= SHARP and e < RTOL


# --- 4. boundary paths ------------------------------------------------------------------------------
@pytest.mark.parametrize("stepper,n", [(s, 32) for s in STEPPERS] + [("IFMAB3", 512)])
def test_checkpoint_restart_bitwise(libsw, stepper, n):
    g = _grid(n, n)
    a, P = _make(n, n, stepper)
    a.sol = _o1_state(g, P, seed=9)[None]
    a.stepforward(5)
    blob = a.ctx.get_checkpoint()
    a.stepforward(4)
    b = _make(n, n, stepper)[0]
    b.ctx.set_checkpoint(blob)
    assert b.clock.step == 5
    b.stepforward(4)
    assert np.array_equal(a.sol, b.sol)
    other = QG2.Problem("gpu", nx=n, ny=n, T=np.float64, stepper=stepper if stepper != "FilteredRK4" else "IFMAB3")
    with pytest.raises(_lib.LibSWError):  # the header's model id is checked
        other.ctx.set_checkpoint(blob)
    for p in (a, b, other):
        p.close()


@pytest.mark.parametrize("stepper", STEPPERS)
def test_history_slots_hold_N(libsw, stepper):
    """get_history(1/2): N₋₁, N₋₂ of IFMAB3 (in the fused pass N lives only there), RHS₋₁, RHS₋₂ of
    FilteredAB3; the RK4 steppers keep none."""
    nx, ny = 128, 64
    g = _grid(nx, ny)
    prob, P = _make(nx, ny, stepper)
    if stepper in ("IFMRK4", "FilteredRK4"):
        assert prob.ctx.history_slots() == 0
        with pytest.raises(_lib.LibSWError):
            prob.ctx.get_history(1)
        prob.close()
        return
    assert prob.ctx.history_slots() == 2
    q = _o1_state(g, P)
    prob.sol = q[None]
    prob.stepforward(5)
    ref = Ref(q, g, P, stepper)
    ref.step(5)
    for slot, want in ((1, ref.h1), (2, ref.h2)):
        e = O.parity_error(prob.ctx.get_history(slot), want[None], g)
        print(f"swqg {stepper} history slot {slot}: {e:.3e}")
        assert e < RTOL
    prob.close()


@pytest.mark.parametrize("stepper", ["IFMAB3", "FilteredAB3"])
def test_reset_history_restarts_with_euler(libsw, stepper):
    nx, ny = 128, 64
    g = _grid(nx, ny)
    prob, P = _make(nx, ny, stepper)
    q = _o1_state(g, P)
    prob.sol = q[None]
    prob.stepforward(5)
    prob.ctx.reset_history()
    prob.stepforward(4)
    got = prob.sol
    prob.close()
    ref, plain = Ref(q, g, P, stepper), Ref(q, g, P, stepper).step(9)
    ref.step(5)
    ref.reset_history()
    want = ref.step(4)  # three Euler steps, then AB3
    e = O.parity_error(got, want[None], g)
    d = O.parity_error(plain[None], want[None], g)
    print(f"swqg {stepper} reset_history: {e:.3e} (the reset moves the reference by {d:.1e})")
    assert d > 1e3 * RTOL  # the comparison can tell an ignored reset
    assert e < RTOL


@pytest.mark.parametrize("stepper", ["IFMAB3", "FilteredRK4"])
def test_float32_buffers(libsw, stepper):
    nx, ny = 128, 64
    g = _grid(nx, ny)
    (p32, P), p64 = _make(nx, ny, stepper, T=np.float32), _make(nx, ny, stepper)[0]
    s0 = _o1_state(g, P, seed=13)[None].astype(np.complex64)
    p32.sol, p64.sol = s0, s0.astype(np.complex128)
    p32.stepforward(5)
    p64.stepforward(5)
    assert p32.sol.dtype == np.complex64 and np.array_equal(p32.sol, p64.sol.astype(np.complex64))
    assert np.max(np.abs(p32.sol)) > 0
    with pytest.raises(_lib.LibSWError) as ei:  # an fp64-sized buffer on the fp32 context
        wrong = np.zeros(p32.ctx.state_shape, np.complex128)
        p32.ctx._check(p32.ctx.lib.sw_get_state(p32.ctx._h, wrong.ctypes.data, wrong.nbytes), "sw_get_state")
    assert ei.value.code == _lib.SW_E_INVALID
    p32.close()
    p64.close()


@pytest.mark.parametrize("stepper", ["IFMAB3", "IFMRK4"])
def test_nop_calcN_linear_exactness(libsw, stepper):
    """nop_calcN (the one flag the SWQG mirror does not forward): 5 steps are exp(5 dt L) per mode; the
    K = 0 mode (L = 0) is unchanged exactly."""
    nx, ny = 128, 64
    g, P = _grid(nx, ny), drivers.swqg_parameters(nx)
    prob = problem.Problem(_lib.SW_MODEL_SWQG, nx=nx, ny=ny, Lx=P["Lx"], Ly=P["Lx"], dt=P["dt"], aliased_fraction=1 / 3,
                           stepper=stepper, params=dict(nu=P["nu"], nnu=P["nnu"], f=P["f"], Cg=P["Cg"]), nop_calcN=True)
    q = _o1_state(g, P, seed=11)
    q[0, 0] = 0.3 * nx * ny
    prob.sol = q[None]
    prob.stepforward(5)
    got = prob.sol
    prob.close()
    L = -P["nu"] * g.Krsq ** P["nnu"]
    want = np.exp(5 * P["dt"] * L) * q
    assert np.min(np.exp(5 * P["dt"] * L)[g.live]) < 0.9  # the factor is not 1 across the band
    e = O.parity_error(got, want[None], g)
    print(f"swqg {stepper} exp(L t): {e:.3e}")
    assert e < RTOL
    assert got[0, 0, 0] == q[0, 0]


@pytest.mark.parametrize("stepper", ["IFMAB3", "FilteredRK4"])
def test_nan_detection(libsw, stepper):
    """one non-finite live mode -> SW_E_NAN from the stepper's own update (fused column step, elementwise)."""
    nx, ny = 128, 64
    g = _grid(nx, ny)
    prob, P = _make(nx, ny, stepper)
    q = _o1_state(g, P)
    prob.sol = q[None]
    prob.stepforward(2)
    assert prob.ctx.diag(_lib.SW_DIAG_NAN) == 0.0
    q[3, 5] = np.nan
    prob.sol = q[None]
    with pytest.raises(_lib.LibSWError) as ei:
        prob.stepforward(1)
    assert ei.value.code == _lib.SW_E_NAN
    assert prob.ctx.diag(_lib.SW_DIAG_NAN) == 1.0
    prob.close()


def _energies(q, g, P):
    """swqg/SWQG.jl:205-221: parsevalsum2(K ψ̂)/(2 Lx Ly), Kd² parsevalsum2(ψ̂)/(2 Lx Ly) of the live modes:
    Σ h |K ψ̂|² and Kd² Σ h |ψ̂|² over 2 (nx ny)², h = 1 on the kr = 0 and Nyquist columns, 2 between."""
    psi = _psi(g.dealias(q.copy()), g, _kd2(P))
    h = np.full(g.nkr, 2.0)
    h[0] = h[-1] = 1.0
    den = 2.0 * (g.nx * g.ny) ** 2
    return np.sum(h * g.Krsq * np.abs(psi) ** 2) / den, _kd2(P) * np.sum(h * np.abs(psi) ** 2) / den


@pytest.mark.parametrize("stepper", ["IFMAB3", "IFMRK4"])
def test_energy_records_and_step_record(libsw, stepper):
    nx, ny = 128, 64
    g = _grid(nx, ny)
    (a, P), b, c = _make(nx, ny, stepper), _make(nx, ny, stepper)[0], _make(nx, ny, stepper)[0]
    q = _o1_state(g, P)
    a.sol = b.sol = c.sol = q[None]
    a.ctx.set_energy_diagnostics(2, 16)
    a.stepforward(8)
    recs = a.ctx.energy_diagnostics()
    assert [r[0] for r in recs] == [2, 4, 6, 8]
    for step, t, ke, ke2, pe, wg in recs:
        b.stepforward(2)  # an identical problem, two steps at a time
        wke, wpe = _energies(b.sol[0], g, P)
        assert t == pytest.approx(step * P["dt"], rel=1e-12)
        assert ke == pytest.approx(wke, rel=1e-12) and pe == pytest.approx(wpe, rel=1e-12)
        assert wke > 0 and wpe > 0 and ke2 == 0.0 and wg == (0.0, 0.0, 0.0, 0.0)
    assert c.ctx.step_record(2) == recs[0]
    for p in (a, b, c):
        p.close()


@pytest.mark.parametrize("square", [True, False], ids=["Ly=Lx", "Ly=Lx/2"])
def test_cfl_diagnostic(libsw, square):
    """SW_DIAG_CFL = dt max(max|u|/dx, max|v|/dy); with Ly = Lx/2 (the one rectangular-domain case, dy ≠ dx)
    calcN and the fields as well."""
    nx, ny = 128, 64
    P = drivers.swqg_parameters(nx)
    P = dict(P, Ly=P["Lx"] if square else P["Lx"] / 2)
    g = _gridP(nx, ny, P)
    prob, _ = _make(nx, ny, "IFMAB3", P)
    q = _o1_state(g, P, seed=3)
    prob.sol = q[None]
    psi = _psi(q, g, _kd2(P))
    u, v = g.irfft(-1j * g.l[:, None] * psi), g.irfft(1j * g.kr[None, :] * psi)
    got = SWQG.updatevars(prob)
    for name, w in (("u", u), ("v", v), ("psi", g.irfft(psi))):
        assert np.max(np.abs(got[name] - w)) <= 1e-12 * np.max(np.abs(w)), name
    want = P["dt"] * max(np.max(np.abs(u)) / g.dx, np.max(np.abs(v)) / g.dy)
    assert SWQG.cfl(prob) == pytest.approx(want, rel=1e-12)
    if not square:
        e =O.parity_error(prob.calcN(q[None]), ref_calcN(q.copy(), g, _kd2(P))[None], g)
        print(f"swqg calcN {nx}x{ny} Ly = Lx/2: {e:.3e}")
        assert e < RTOL
    prob.close()


@pytest.mark.parametrize("stepper,nx,ny", [("FilteredAB3", 512, 512), ("IFMRK4", 512, 512), ("FilteredRK4", 512, 512),
                                           ("IFMAB3", 32, 2048), ("IFMAB3", 2048, 32)])
def test_fused_equals_unfused_every_stepper(libsw, stepper, nx, ny):
    out = []
    P = _tall_P(nx, ny) if ny > nx else None  # (dx = dy on the tall grid, as test_steps_long_lines)
    for unfused in (False, True):
        prob, Pp = _make(nx, ny, stepper, P, unfused=unfused)
        prob.sol = (_band_state(_gridP(nx, ny, P), P, seed=3) if P else _o1_state(_grid(nx, ny), Pp, seed=3))[None]
        prob.stepforward(12)
        out.append(prob.sol)
        prob.close()
    assert np.max(np.abs(out[0])) > 0 and np.all(np.isfinite(out[0]))
    assert np.array_equal(out[0], out[1])
