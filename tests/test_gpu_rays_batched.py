"""The batched ray snapshot (sw_rays_config.unbatched = 0): three
column inverses of ψ, l ψ, l² ψ and one row pass that writes the texels, against
the numpy.fft.irfft2 reference of tests/test_gpu_rays.py at its tolerance
(RTOL = 1e-10 of each field's maximum), with packets on every grid node, so
both rows of every two-row line group and every x of every lane are compared.

Shapes: 32×64 for every ψ expression; 32×32 and 64×32 for several lines per
block and swapped roles (32×32 is the smallest grid sw_create accepts: the
power-of-two engine starts at 32 points, a 16×16 grid is refused on the parent
commit too); 4096- and 8192-point rows and columns for the 128-VGPR instances
of each kernel; two slabs in one process for the three-field exchange and the
y0 offset of the texel writes."""
import numpy as np
import pytest

import test_swqg as SQ
from juliaraytracingsw_amd import LibSWError, Rays, _lib
from test_gpu_rays import CG_PKT, F_PKT, RTOL, _field_errors, _fields, _flow, _lib_loaded, _packets  # noqa: F401

pytestmark = pytest.mark.gpu


def _swqg_flow(nx, ny):
    """the SWQG problem and state of tests/test_swqg.py; its ray streamfunction is ψ̂ = -q̂/(K² + f²/Cg²)"""
    grid, (prob, P) = SQ._grid(nx, ny), SQ._problem(nx, ny)
    prob.sol = SQ._decaying_q(grid, seed=11)[None]
    k, l = grid.kr[None, :], grid.l[:, None]
    ph = -prob.sol[0] / (grid.Krsq + P["f"] ** 2 / P["Cg"] ** 2)
    spec = [-1j * l * ph, 1j * k * ph, k * l * ph, l * l * ph, -k * k * ph]
    return grid, prob, np.stack([np.fft.irfft2(s, s=(ny, nx)) for s in spec])


def _node_errors(case, psi, nx, ny, dec=None, **rkw):
    if case == "swqg":
        grid, prob, ref = _swqg_flow(nx, ny)
    else:
        p, grid, prob = _flow(case, nx, ny, **({"decomposition": dec} if dec else {}))
        ref = _fields(p, grid, prob.sol, psi)
    X, Y = np.meshgrid(grid.x, grid.y)
    xk = np.column_stack([X.ravel(), Y.ravel(), np.ones(X.size), np.ones(X.size)])
    rays = Rays(prob, xk, np.ones(X.size), f=F_PKT, Cg=CG_PKT, psi=psi, **rkw)
    rays.snapshot()
    e = _field_errors(*rays.sample(), ref.reshape(5, -1))
    prob.close()
    return e


SLABS = dict(nranks=2, local_slabs=2)


@pytest.mark.parametrize("case,psi,nx,ny,dec", [
    ("rsw_ifmab3", "default", 32, 64, None), ("qg2_ifmab3", "default", 32, 64, None),
    ("qg2_ifmab3", "layer1", 32, 64, None), ("qg2_ifmab3", "layer2", 32, 64, None),
    ("mlqg_frk4", "default", 32, 64, None), ("swqg", "default", 32, 64, None),
    ("rsw_ifmab3", "default", 32, 32, None), ("rsw_ifmab3", "default", 64, 32, None),
    ("rsw_ifmab3", "default", 4096, 32, None), ("rsw_ifmab3", "default", 32, 4096, None),
    ("rsw_ifmab3", "default", 8192, 32, None), ("rsw_ifmab3", "default", 32, 8192, None),
    ("rsw_ifmab3", "default", 64, 64, SLABS)])
def test_batched_fields_at_every_node(case, psi, nx, ny, dec):
    e = _node_errors(case, psi, nx, ny, dec)
    print(f"batched {case} {psi} {nx}x{ny} {dec}: {e}")
    assert np.all(e < RTOL), e


@pytest.mark.parametrize("case", ["rsw_ifmab3", "qg2_ifmab3"])
def test_unbatched_flag_reaches_the_one_field_path(case):
    """the two paths agree through the reference (not bitwise: the multiplication order differs)"""
    e = _node_errors(case, "default", 32, 64, unbatched=True)
    print(f"unbatched {case}: {e}")
    assert np.all(e < RTOL), e


@pytest.mark.parametrize("case", ["rsw_fab3", "rsw_ifmab3", "qg2_ifmab3"])
def test_stepping_undisturbed_and_fused_loop(case):
    """snapshots use the mixed arrays as scratch: the flow of a problem with rays
    steps bitwise as one without, and rays.step is the explicit loop bitwise"""
    p, grid, plain = _flow(case, 64, 64)
    plain.stepforward(5)
    out = []
    for fused in (True, False):
        _, _, prob = _flow(case, 64, 64)
        rays = Rays(prob, *_packets(grid, 257, span=1.0), f=F_PKT, Cg=CG_PKT)
        rays.snapshot()
        if fused:
            rays.step(5)
        else:
            for _ in range(5):
                prob.stepforward(1)
                rays.snapshot()
                rays.advance(p["dt"])
        out.append((prob.sol, (prob.clock.t, prob.clock.step), rays.packets))
        prob.close()
    want = (plain.sol, (plain.clock.t, plain.clock.step))
    plain.close()
    for sol, clock, _ in out:
        assert np.array_equal(sol, want[0]) and clock == want[1]
    assert np.array_equal(out[0][2], out[1][2])


def test_unbatched_out_of_range_is_refused():
    p, grid, prob = _flow("rsw_ifmab3", 32, 32, ic=False)
    with pytest.raises(LibSWError, match="unbatched") as ei:
        Rays(prob, *_packets(grid, 5), f=F_PKT, Cg=CG_PKT, unbatched=2)
    prob.close()
    assert ei.value.code == _lib.SW_E_INVALID
