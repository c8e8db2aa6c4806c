"""CPU tier of the pseudofermion force: the numpy restatement tests/wilson_force_restatement.py, which every kernel and
GPU test of the dynamical Wilson fermions is held against, is itself held against central differences of the action,
its identities, and the properties of the leapfrog built from it (dense solves throughout, except where the CG is the
subject)."""
import numpy as np
import pytest

import wilson_force_restatement as wf
import wilson_restatement as wr
from oracle import su3 as osu3

KAPPA = 0.124


@pytest.mark.parametrize('ap', [False, True])
@pytest.mark.parametrize('L', wf.FD_LATTICES)
def test_force_against_finite_differences(L, ap):
    """sum <p, F> against the Richardson combination (4 D(h/2) - D(h)) / 3 of the central differences of S_f at h = 1e-3:
    relative difference <= 1e-8, and the two raw differences in the ratio 4 of their h^2 terms (a wrong factor in the
    force would pass a loose bound, not this)."""
    x, phi, p = wf.fd_inputs(L)
    X, Y = wf.dense_normal(x, phi, KAPPA, ap)
    want = wf.pair(p, wf.force(x, X, Y, KAPPA, ap))
    d, d1, d2 = wf.richardson(x, phi, p, KAPPA, ap, h=1e-3)
    rel = np.abs(d - want) / np.abs(want)
    ratio = (d1 - want) / (d2 - want)
    print(L, ap, 'relative', rel, 'raw', np.abs(d1 - want) / np.abs(want), 'ratio', ratio)
    assert (rel <= 1e-8).all(), rel
    assert ((ratio > 3.5) & (ratio < 4.5)).all(), ratio


@pytest.mark.parametrize('L', wf.FD_LATTICES)
def test_identities(L):
    nb, npf = 2, 2
    x, phi = wr.links(L, nb), wr.spinors(L, nb, npf)
    X, Y = wf.dense_normal(x, phi, KAPPA)
    # S_f = phi^H (M^H M)^-1 phi = sum |Y|^2
    s = wr.norm2(Y).sum(1)
    direct = (phi.conj() * X).sum(axis=tuple(range(1, 8)))
    assert np.abs(direct.imag).max() <= 1e-12 * s.max() and np.abs(direct.real - s).max() <= 1e-12 * s.max()
    assert np.array_equal(wf.fermion_action(x, phi, KAPPA), s)
    # the heatbath: S_f(M^H eta) = |eta|^2
    eta = wf.gaussian_eta(L, nb, npf)
    ph, s0 = wf.refresh(x, eta, KAPPA)
    assert np.abs(wf.fermion_action(x, ph, KAPPA) - s0).max() <= 1e-12 * s0.max()
    assert abs((np.abs(eta) ** 2).mean() - 1.0) < 0.2                       # density exp(-eta^H eta): <|eta|^2> = 1
    # exactly anti-Hermitian, traceless to rounding
    F = wf.force(x, X, Y, KAPPA)
    assert np.array_equal(F, -wf.adj(F))
    assert np.abs(np.einsum('...ii->...', F)).max() <= 1e-13 * np.abs(F).max()
    # gauge covariance: U -> g(x) U g(x+mu)^H, phi -> g phi gives F -> g F g^H
    rng = np.random.default_rng(31)
    g = osu3.project_su(rng.standard_normal((nb, *L, 3, 3)) + 1j * rng.standard_normal((nb, *L, 3, 3)))
    xg = np.stack([g @ x[:, mu] @ wf.adj(np.roll(g, -1, axis=1 + mu)) for mu in range(4)], 1)
    rot = lambda f: np.einsum('btxyzij,brtxyzaj->brtxyzai', g, f)           # noqa: E731
    Xg, Yg = wf.dense_normal(xg, rot(phi), KAPPA)
    Fg = wf.force(xg, Xg, Yg, KAPPA)
    assert np.abs(Fg - g[:, None] @ F @ wf.adj(g)[:, None]).max() <= 1e-10 * np.abs(F).max()
    # kappa = 0: M = 1, no force
    assert not wf.force(x, phi, phi, 0.0).any()
    # linear in the fields: two fields give the sum of the single-field forces
    one = [wf.force(x, X[:, r:r + 1], Y[:, r:r + 1], KAPPA) for r in range(npf)]
    assert np.abs(F - (one[0] + one[1])).max() <= 4 * 2.0 ** -52 * np.abs(F).max()


@pytest.mark.parametrize('L', wf.TRAJ_LATTICES)
def test_trajectory(L):
    """reversibility to rounding, and dH ~ eps^2 at fixed trajectory length -- also at beta = 0, where the gauge force
    cannot carry the ratio (it lies in (3.5, 4.5) at the same step sizes there: no halving was needed)"""
    x, v, phi, s0 = wf.traj_inputs(L)
    T = wf.TRAJ
    assert np.abs(wf.fermion_action(x, phi, T['kappa']) - s0).max() <= 1e-12 * s0.max()
    x1, v1, dh = wf.delta_h(x, v, phi, **T)
    x2, v2 = wf.leapfrog(x1, -v1, phi, T['beta'], T['kappa'], T['eps'], T['nleapfrog'])
    rev = max(np.abs(x2 - x).max(), np.abs(v2 + v).max())
    print(L, 'reversibility', rev)
    assert rev <= 1e-13
    for beta in (T['beta'], 0.0):
        a = dh if beta else wf.delta_h(x, v, phi, 0.0, T['kappa'], T['eps'], T['nleapfrog'])[2]
        b = wf.delta_h(x, v, phi, beta, T['kappa'], T['eps'] / 2, 2 * T['nleapfrog'])[2]
        print(L, 'beta', beta, 'dH', a, b, 'ratio', a / b)
        assert ((a / b > 3.5) & (a / b < 4.5)).all(), (beta, a / b)


@pytest.mark.parametrize('kappa', wr.SOLVE_KAPPAS)
def test_normal_cg(kappa):
    L = (4, 2, 6, 2)
    x, phi = wr.links(L, 2), wr.spinors(L, 2, 2)
    Xd, Yd = wf.dense_normal(x, phi, kappa)
    for tol in (1e-6, 1e-10):
        X, Y, info = wf.normal_cg(x, phi, kappa, tol=tol)
        assert info['converged'].all() and (info['residual'] <= 2 * tol).all(), (tol, info)
        assert np.abs(X - Xd).max() <= 100 * tol * np.abs(Xd).max()          # |dX| <= cond(M^H M) * residual; cond < 100
        assert np.array_equal(info['action'], wr.norm2(Y))
    assert (wf.normal_cg(x, phi, kappa, tol=1e-6)[2]['iters'] < info['iters']).all()
    # a frozen system keeps its bits when another system joins the batch; phi = 0 gives X = 0
    X1 = wf.normal_cg(x[:1], phi[:1, :1], kappa, tol=1e-10)[0]
    assert np.array_equal(X1[0, 0], X[0, 0])
    big = phi.copy()
    big[1, 1] = 0.0
    Xb, _, ib = wf.normal_cg(x, big, kappa, tol=1e-10)
    assert not Xb[1, 1].any() and ib['iters'][1, 1] == 0 and ib['residual'][1, 1] == 0.0
    assert np.array_equal(Xb[0], X[0])
    # never raises: too few iterations are reported
    info = wf.normal_cg(x, phi, kappa, tol=1e-10, max_iter=3)[2]
    assert not info['converged'].any() and (info['iters'] == 3).all()


def test_yardstick_of_the_small_lattices():
    """the extended-precision distance of `force`, re-measured on the small lattices, stays within the recorded figure"""
    assert wf.TOL == 32.0 * wf.YARDSTICK
    assert wf.measure(wr.KERNEL_LATTICES) <= wf.YARDSTICK
