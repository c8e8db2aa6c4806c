"""CPU tier of the dynamical clover quarks: the numpy restatement tests/wilson_clover_force_restatement.py, which the
kernels of csrc/su3_clover_force.hip and the GPU tests of `WilsonCloverHMC` are held against, is itself held against
central differences of its action (the determinant term alone, the pseudofermion term alone, both), against the
unimproved even-odd restatement at c_sw = 0, and against the properties of the leapfrog built from it (dense solves
throughout)."""
import numpy as np
import pytest

import wilson_clover_force_restatement as wcf
import wilson_clover_restatement as wc
import wilson_eo_restatement as we
import wilson_force_restatement as wf
import wilson_restatement as wr

KAPPA = wcf.KAPPA


def test_inputs_are_positive_definite():
    """every test input needs A > 0: the smallest eigenvalue on both kinds of links at both c_sw"""
    for L in [(2, 2, 2, 2), (4, 2, 2, 2), (4, 2, 6, 2), (4, 4, 4, 4)]:
        for kind in wc.INPUTS:
            for c_sw in wc.C_SWS:
                assert wc.min_eig(wc.clover(wc.INPUTS[kind](L, 2), KAPPA * c_sw)) >= 0.55, (L, kind, c_sw)
    with pytest.raises(AssertionError, match='positive definite'):
        wcf.terms(wr.links((4, 4, 4, 4), 2), KAPPA, wc.C_SW_BAD)


def test_leaf_factors_are_the_leaves():
    x = wc.hot_links((4, 2, 6, 2), 2)
    for mu, nu in wcf.PLANES:
        q = wc.leaves(x, mu, nu)
        assert np.abs(wcf.leaves_from_factors(x, mu, nu) - q).max() <= 16 * 2.0 ** -52 * np.abs(q).max(), (mu, nu)


@pytest.mark.parametrize('case', wcf.FD_CASES, ids=[c[0] for c in wcf.FD_CASES])
@pytest.mark.parametrize('c_sw', wc.C_SWS)
@pytest.mark.parametrize('ap', [False, True])
@pytest.mark.parametrize('L', we.FD_LATTICES)
def test_force_against_finite_differences(L, ap, c_sw, case):
    """sum <p, F> against the Richardson combination (4 D(h/2) - D(h)) / 3 of the central differences of the action under
    U -> exp(+-h p) U at h = 1e-3: relative difference <= 32 x the recorded figure of the restatement itself, and the two
    raw differences in the ratio 4 of their h^2 terms (a wrong factor in the force would pass a loose bound, not this)."""
    name, pf, det = case
    tr = wcf.Trajectory(c_sw, pf, det)
    for kind in wc.INPUTS:
        x, phi, p = wcf.fd_inputs(kind, L)
        want = wf.pair(p, tr.fermion_force(x, phi, KAPPA, ap))
        d, d1, d2 = wf.richardson(x, phi, p, KAPPA, ap, h=1e-3, action=lambda xx: tr.fermion_action(xx, phi, KAPPA, ap))
        rel = np.abs(d - want) / np.abs(want)
        ratio = (d1 - want) / (d2 - want)
        print(L, ap, c_sw, name, kind, 'relative', rel, 'raw', np.abs(d1 - want) / np.abs(want), 'ratio', ratio)
        assert (rel <= 32.0 * wcf.DENSE_FD).all(), (kind, rel)
        assert ((ratio > 3.5) & (ratio < 4.5)).all(), (kind, ratio)


@pytest.mark.parametrize('L', we.FD_LATTICES)
def test_identities(L):
    nb, npf, c_sw = 2, 2, 1.769
    x, phi, _ = wcf.fd_inputs('hot', L, nb, npf)
    a, ainv = wcf.terms(x, KAPPA, c_sw)
    tr = wcf.Trajectory(c_sw)
    Xe, Ye = tr.solve(x, phi, KAPPA, True, None)
    # the pseudofermion part is phi_e^H (Mhat^H Mhat)^-1 phi_e = sum |Y_e|^2; the determinant part is -2 npf log det A_oo
    s, ld = tr.parts(x, phi, KAPPA)
    direct = (phi.conj() * Xe).sum(axis=tuple(range(1, 8)))
    assert np.abs(direct.imag).max() <= 1e-12 * s.max() and np.abs(direct.real - s).max() <= 1e-12 * s.max()
    assert np.array_equal(ld, -2.0 * npf * wc.logdet(a)[:, 1])
    assert not (Xe * we.mask(L, 1)).any() and not (Ye * we.mask(L, 1)).any()
    # the heatbath: the pseudofermion part of S_f(Mhat^H eta_e) is |eta_e|^2
    ph, s0 = wcf.refresh(x, we.gaussian_eta_e(L, nb, npf), KAPPA, c_sw)
    assert np.abs(wcf.Trajectory(c_sw, det=False).fermion_action(x, ph, KAPPA) - s0).max() <= 1e-12 * s0.max()
    # G is anti-Hermitian with a trace; the two terms add; the force is exactly anti-Hermitian, traceless to rounding
    X, Y = wr.spinors(L, nb, 12)[:, :npf], wr.spinors(L, nb, 12)[:, 6:6 + npf]
    g = wcf.g_field(X, Y, ainv, KAPPA * c_sw, npf, L)
    assert np.array_equal(g, -wf.adj(g)) and np.abs(np.einsum('...ii->...', g)).max() > 1e-3
    parts = wcf.g_field(X, Y, None, KAPPA * c_sw, 0.0, L) + wcf.g_field(None, None, ainv, KAPPA * c_sw, npf, L)
    assert np.abs(g - parts).max() <= 4 * 2.0 ** -52 * np.abs(g).max()
    assert not (wcf.g_field(None, None, ainv, KAPPA * c_sw, npf, L) * we.mask(L, 0)).any()     # odd sites only
    F = wcf.clover_force(x, X, Y, ainv, KAPPA, c_sw, npf)
    assert np.array_equal(F, -wf.adj(F))
    assert np.abs(np.einsum('...ii->...', F)).max() <= 1e-13 * np.abs(F).max()
    # the workspace layout keeps all of G
    gw = wcf.pack_g(g)
    assert gw.shape == (nb, 6, 9, int(np.prod(L))) and np.abs(gw).max() == max(np.abs(g.real).max(), np.abs(g.imag).max())


@pytest.mark.parametrize('L', we.FD_LATTICES)
def test_c_sw_zero_is_the_unimproved_action(L):
    """A = 1: log det A = 0 exactly, and force and action are those of `wilson_eo_restatement`"""
    x, phi, _ = wcf.fd_inputs('smooth', L)
    tr = wcf.Trajectory(0.0)
    pf, ld = tr.parts(x, phi, KAPPA)
    assert not np.asarray(ld).any()
    s = we.fermion_action(x, phi, KAPPA)
    assert np.abs(pf - s).max() <= 1e-12 * s.max()
    F = we.fermion_force(x, phi, KAPPA)
    assert np.abs(tr.fermion_force(x, phi, KAPPA) - F).max() <= 1e-11 * np.abs(F).max()
    assert not wcf.clover_force(x, phi, phi, np.broadcast_to(np.eye(12, dtype=complex), (2, *L, 12, 12)), KAPPA, 0.0, 2).any()


@pytest.mark.parametrize('L', wf.TRAJ_LATTICES)
def test_trajectory(L):
    """reversibility to rounding, and dH ~ eps^2 at fixed trajectory length at wf.TRAJ with c_sw = 1.769: dH(eps) / dH(eps
    / 2) in (3.5, 4.5), as tests/test_wilson_force_host.py holds its own.  Measured: (2,2,2,2) 3.913, 3.890; (4,2,2,2)
    3.844, 3.888.  Also at beta = 0, where the gauge force cannot carry the ratio, one halving further down: there chain 0
    of (2,2,2,2) has dH(0.05) = 0.0017, an eighth of the other chain's (its eps^2 term nearly cancels, as
    `wf.traj_inputs` records for another momentum), so the eps^4 term shows at eps = 0.05 (ratio 5.28) and the ratio is
    asymptotic only from eps / 2 on.  Measured dH(eps / 2) / dH(eps / 4) at beta = 0: (2,2,2,2) 4.346, 3.980; (4,2,2,2)
    3.987, 3.965 (at beta = 5.5 the same pair gives 3.979, 3.973; 3.962, 3.972)."""
    tr = wcf.Trajectory(wcf.TRAJ_C_SW)
    x, v, phi, s0 = wcf.traj_inputs(L)
    T = wf.TRAJ
    pf, _ = tr.parts(x, phi, T['kappa'])
    assert np.abs(pf - s0).max() <= 1e-12 * s0.max()
    x1, v1, dh = tr.delta_h(x, v, phi, **T)
    x2, v2 = tr.leapfrog(x1, -v1, phi, T['beta'], T['kappa'], T['eps'], T['nleapfrog'])
    rev = max(np.abs(x2 - x).max(), np.abs(v2 + v).max())
    print(L, 'reversibility', rev)
    assert rev <= 1e-13
    for beta, k in ((T['beta'], 1), (0.0, 2)):
        a = dh if beta else tr.delta_h(x, v, phi, beta, T['kappa'], T['eps'] / k, k * T['nleapfrog'])[2]
        b = tr.delta_h(x, v, phi, beta, T['kappa'], T['eps'] / (2 * k), 2 * k * T['nleapfrog'])[2]
        print(L, 'beta', beta, 'eps', T['eps'] / k, 'dH', a, b, 'ratio', a / b)
        assert ((a / b > 3.5) & (a / b < 4.5)).all(), (beta, a / b)


def test_yardsticks_of_the_small_lattices():
    """the extended-precision distances of `g_field` and `clover_force`, re-measured on the small lattices, stay within
    the recorded figures"""
    assert wcf.TOL_G == 32.0 * wcf.YARD_G and wcf.TOL_F == 32.0 * wcf.YARD_F
    g, f = wcf.measure(we.EO_KERNEL_LATTICES)
    assert g <= wcf.YARD_G and f <= wcf.YARD_F
