"""CPU checks of the yardstick tests/gaugefix_restatement.py by facts that do not depend on it: the functional never
decreases, gauge-invariant quantities do not move, the returned g reproduces the half-sweep as a gauge transformation,
and a pure gauge comes back to the trivial field.  The kernels are compared with this yardstick in
tests/test_gaugefix_emu.py (host build) and tests/test_gaugefix_gpu.py."""
import numpy as np
import pytest

import gaugefix_restatement as gf
from oracle import su3 as osu3

L = (4, 2, 6, 2)
NB = 2


@pytest.fixture(scope='module')
def links():
    return gf.random_links(np.random.default_rng(7), NB, L)


@pytest.mark.parametrize('omega', [1.0, 1.7])
@pytest.mark.parametrize('D', [gf.LANDAU, gf.coulomb(1)])
def test_functional_never_decreases_and_plaquette_stays(links, D, omega):
    x = links
    p0 = osu3.plaqs(x)
    f = gf.condition(x, D)[0]
    for _ in range(6):
        for parity in (0, 1):
            x, _ = gf.half_sweep(x, D, parity, omega)
            f1 = gf.condition(x, D)[0]
            assert (f1 - f >= -1e-14).all(), (f, f1)
            f = f1
    assert (f > gf.condition(links, D)[0] + 0.05).all()
    assert np.abs(osu3.plaqs(x) - p0).max() <= 1e-12
    assert np.abs(osu3.adj(x) @ x - np.eye(3)).max() <= 1e-12


@pytest.mark.parametrize('D', gf.MASKS)
def test_half_sweep_is_the_gauge_transformation_it_returns(links, D):
    for parity in (0, 1):
        out, g = gf.half_sweep(links, D, parity, 1.7)
        here = gf.parity_mask(L, parity)
        assert np.array_equal(g[:, ~here], np.broadcast_to(np.eye(3), g[:, ~here].shape))
        assert (np.abs(g[:, here] - np.eye(3)).max((-2, -1)) > 1e-6).all()
        assert np.abs(osu3.adj(g) @ g - np.eye(3)).max() <= 1e-13
        assert np.abs(gf.apply(links, g) - out).max() <= 1e-13
        # every link has one end on the parity: none stays
        assert (np.abs(out - links).max((-2, -1)) > 1e-6).all()


def test_stationary_point_and_residual():
    """the trivial field is a maximum: F = 1, theta = 0, and a sweep leaves it alone; theta of a random field is O(1)"""
    cold = np.broadcast_to(np.eye(3, dtype=np.complex128), (1, 4, *L, 3, 3)).copy()
    for D in gf.MASKS:
        F, theta = gf.condition(cold, D)
        assert F[0] == 1.0 and theta[0] == 0.0
        assert np.array_equal(gf.sweep(cold, D, 1.7), cold)
    F, theta = gf.condition(gf.random_links(np.random.default_rng(3), 1, L), gf.LANDAU)
    assert abs(F[0]) < 0.1 and 0.5 < theta[0] < 20.0


@pytest.mark.parametrize('D', [gf.LANDAU, gf.coulomb(0)])
def test_smooth_pure_gauge_returns_to_the_trivial_field(D):
    x = gf.pure_gauge(np.random.default_rng(17), 2, (4, 4, 4, 4), amp=0.3)
    assert (gf.condition(x, D)[0] < 0.99).all()
    assert np.abs(osu3.plaqs(x) - 1.0).max() <= 1e-13
    for n in range(200):
        x = gf.sweep(x, D, 1.0)
        if (1.0 - gf.condition(x, D)[0] <= 1e-12).all():
            break
    F, theta = gf.condition(x, D)
    print(f'mask {D}: 1 - F = {1.0 - F} after {n + 1} sweeps, theta = {theta}')
    assert (1.0 - F <= 1e-12).all()
