"""generate_initial_wavepackets (raytracing/RaytracingDriver.jl:27-47): host set-up, no GPU."""
import numpy as np

from juliaraytracingsw_amd import generate_initial_wavepackets


def test_initial_wavepackets_lattice_phases_signs():
    L, k0, s = 2 * np.pi, 7.5, 4
    xk, sign = generate_initial_wavepackets(L, k0, s)
    assert xk.shape == (16, 4) and sign.shape == (16,)
    mid = -L / 2 + (np.arange(s) + 0.5) * L / s  # the lattice cells' midpoints
    np.testing.assert_allclose(xk[:, 0].reshape(s, s), np.broadcast_to(mid, (s, s)), rtol=0, atol=1e-15)  # x fastest
    np.testing.assert_allclose(xk[:, 1].reshape(s, s), np.broadcast_to(mid[:, None], (s, s)), rtol=0, atol=1e-15)
    np.testing.assert_allclose(xk[:, 2] ** 2 + xk[:, 3] ** 2, k0 ** 2, rtol=1e-14)
    phase = 2 * np.pi * np.arange(1, 17) / 16  # J = 1 … N: the last packet points along +x
    np.testing.assert_allclose(xk[:, 2:], k0 * np.column_stack([np.cos(phase), np.sin(phase)]), rtol=0, atol=1e-14 * k0)
    assert np.array_equal(sign, np.tile([-1.0, 1.0], 8))
