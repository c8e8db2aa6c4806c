"""CPU checks of the yardstick tests/smear_restatement.py by facts that do not depend on it: gauge covariance, what
alpha = 0, the cold start, a pure gauge and a uniform abelian flux must give, that an APE mask keeps the other
directions out and a spatial mask keeps time slices apart, and that smearing smooths.  The kernels are compared with
this yardstick in tests/test_smear_emu.py (host build) and tests/test_smear_gpu.py."""
import numpy as np
import pytest

import gaugefix_restatement as gf
import smear_restatement as sm
from oracle import su3 as osu3

L = (4, 2, 6, 2)
NB = 2
OPS = {'ape_spatial': lambda x: sm.ape_step(x, 0.5, sm.spatial(0)), 'ape_4d': lambda x: sm.ape_step(x, 0.7, 15),
       'ape_pair': lambda x: sm.ape_step(x, 0.5, 6), 'hyp': lambda x: sm.hyp_step(x)}


@pytest.fixture(scope='module')
def links():
    return sm.smooth_input(L, NB)


@pytest.mark.parametrize('op', list(OPS))
def test_gauge_covariance(links, op):
    g = gf.random_su3(np.random.default_rng(5), (NB, *L))
    d = float(np.abs(OPS[op](gf.apply(links, g)) - gf.apply(OPS[op](links), g)).max())
    print(f'{op}: |smear(g x) - g smear(x)| = {d:.3g}')
    assert d <= 1e-13


def test_alpha_zero_returns_the_input(links):
    for D in sm.APE_MASKS:
        assert np.abs(sm.ape_step(links, 0.0, D) - links).max() <= 1e-14
    assert np.abs(sm.hyp_step(links, (0.0, 0.0, 0.0)) - links).max() <= 1e-14


@pytest.mark.parametrize('op', list(OPS))
def test_cold_start_is_a_fixed_point(op):
    cold = np.broadcast_to(np.eye(3, dtype=np.complex128), (1, 4, *L, 3, 3)).copy()
    assert np.abs(OPS[op](cold) - cold).max() <= 1e-15


@pytest.mark.parametrize('op', list(OPS))
def test_pure_gauge_stays_a_pure_gauge(op):
    x = gf.pure_gauge(np.random.default_rng(17), NB, L, amp=0.3)
    y = OPS[op](x)
    assert np.abs(osu3.plaqs(y) - 1.0).max() <= 1e-13
    assert np.abs(y - x).max() <= 1e-13                     # covariance and the fixed point: the same pure gauge


def flux_field(phis):
    """U_mu(x) = diag(exp(i phi_mu,c)) at every site: every staple is the link itself"""
    x = np.zeros((1, 4, *L, 3, 3), dtype=np.complex128)
    for mu in range(4):
        for c in range(3):
            x[:, mu, ..., c, c] = np.exp(1j * phis[mu][c])
    return x


def test_uniform_abelian_flux_is_a_fixed_point():
    """a constant diagonal field commutes with itself: S_nu[A, B] = 2 B, so the blend is a positive multiple of U while
    (1 - alpha) + (alpha / 2n) sum 2 cos(0) = 1 stays positive in every colour component -- and it always does"""
    rng = np.random.default_rng(23)
    ph = rng.uniform(-1.0, 1.0, size=(4, 3))
    ph[:, 2] = -ph[:, 0] - ph[:, 1]                          # det = 1
    x = flux_field(ph)
    for op in OPS.values():
        assert np.abs(op(x) - x).max() <= 1e-14


FLUX_L = (8, 2, 2, 2)


def twisted_flux(n):
    """U_mu(x) = diag(exp(i phi_c x_nu)) for one pair (mu, nu) = (1, 0), phi_c = 2 pi k_c / N_nu: a uniform abelian flux
    through the (nu, mu) plane, every other link the identity.  The staples of direction nu around U_mu are U_mu times
    exp(+-i phi_c)."""
    T = FLUX_L[0]
    k = np.array([n, 2 * n, -3 * n])
    x = np.zeros((1, 4, *FLUX_L, 3, 3), dtype=np.complex128)
    x[..., 0, 0] = x[..., 1, 1] = x[..., 2, 2] = 1.0
    for t in range(T):
        for c in range(3):
            x[:, 1, t, ..., c, c] = np.exp(2j * np.pi * k[c] * t / T)
    return x, 2.0 * np.pi * k / T


def test_uniform_flux_through_a_plane_is_a_fixed_point_while_the_blend_stays_positive():
    """the staples of direction 0 around U_1 carry the phases exp(+-i phi_c): U_1 -> Proj[((1 - alpha) + (alpha / 2n)
    (2 cos phi_c + 2 (n - 1))) U_1], a fixed point while that factor is positive in every colour component"""
    x, phi = twisted_flux(1)                                 # phi = (pi/4, pi/2, -3 pi/4) on T = 8: three different factors
    for alpha, D in ((0.5, 15), (0.7, 15), (0.5, 3), (0.4, 3)):
        n = len(sm.dirs(D)) - 1
        factor = (1.0 - alpha) + (alpha / (2 * n)) * (2.0 * np.cos(phi) + 2.0 * (n - 1))
        assert (factor > 0).all(), (alpha, D, factor)
        assert np.abs(sm.ape_step(x, alpha, D) - x).max() <= 1e-14, (alpha, D)
    # the plaquette of the flux is not trivial: the fixed point is not the cold start in disguise
    assert abs(osu3.plaqs(x)[0] - 1.0) > 0.05


@pytest.mark.parametrize('D', sm.APE_MASKS[1:])
def test_directions_outside_the_mask_are_copied_and_enter_no_staple(links, D):
    out = sm.ape_step(links, 0.5, D)
    inside = sm.dirs(D)
    outside = [mu for mu in range(4) if mu not in inside]
    for mu in outside:
        assert np.array_equal(out[:, mu], links[:, mu])
    for mu in inside:
        assert (np.abs(out[:, mu] - links[:, mu]).max((-2, -1)) > 1e-6).all()
    # other links outside the mask: the same result inside it, bit for bit
    other = links.copy()
    other[:, outside] = gf.random_links(np.random.default_rng(3), NB, L)[:, outside]
    assert np.array_equal(sm.ape_step(other, 0.5, D)[:, inside], out[:, inside])


@pytest.mark.parametrize('time_dir', range(4))
def test_spatial_mask_keeps_time_slices_apart(links, time_dir):
    other = links.copy()
    idx = [slice(None)] * 6
    idx[2 + time_dir] = 1                                    # every link that starts in slice 1
    other[tuple(idx)] = gf.random_su3(np.random.default_rng(11), other[tuple(idx)].shape[:-2], 0.3)
    a, b = (sm.ape(v, 0.5, sm.spatial(time_dir), 2) for v in (links, other))
    for k in range(L[time_dir]):
        idx[2 + time_dir] = k
        same = np.array_equal(a[tuple(idx)], b[tuple(idx)])
        assert same == (k != 1), (time_dir, k)


@pytest.mark.parametrize('op', list(OPS))
def test_mean_plaquette_rises(op):
    x = sm.smooth_input((4, 4, 4, 4), NB)
    p0 = osu3.plaqs(x)
    y = OPS[op](x)
    p1 = osu3.plaqs(y)
    print(f'{op}: plaquette {p0} -> {p1}')
    assert (p1 > p0 + 0.01).all()
    assert np.abs(osu3.adj(y) @ y - np.eye(3)).max() <= 1e-13 and np.abs(np.linalg.det(y) - 1.0).max() <= 1e-13


def test_yardsticks_and_input_rule():
    """the figures that the tolerances of the emulation and GPU tests are built on, measured again on the small lattices:
    no yardstick beyond the recorded one (twice it: another LAPACK build rounds its SVD differently), the worst
    condition number far inside the input rule"""
    for lat in sm.KERNEL_LATTICES:
        y = sm.yardsticks(sm.smooth_input(lat), [(a, m, 1) for a, m in sm.APE_CASES])
        print(lat, {k: float(f'{v:.3g}') for k, v in y.items()})
        assert y['cond'] <= 3.0
        for k, v in sm.YARDSTICK.items():
            assert y[k] <= 2.0 * v, (lat, k, y[k], v)
    assert all(abs(sm.TOL[k] - 32.0 * sm.YARDSTICK[k]) < 1e-30 for k in sm.YARDSTICK)
    # Haar-random links break the input rule in a HYP step and in a 4D APE step: the restatement refuses them
    x = gf.random_links(np.random.default_rng(1), 3, (4, 4, 4, 4))
    for op in ('hyp', 'ape_4d'):
        with pytest.raises(AssertionError, match='input rule'):
            OPS[op](x)
