"""CPU tier of the multi-shift CG and the one-flavour rational pseudofermion: the numpy restatement
tests/wilson_multishift_restatement.py held against dense linear algebra on the Mhat of `wilson_eo_restatement`, so that
the GPU tests stand on something checked.  Every configuration's spectrum is asserted to lie inside the [ra, rb] of the
approximation it is used with (`ms.assert_spectrum`).

Bounds.  |S_R - phi^H A^(-1/2) phi| <= delta phi^H A^(-1/2) phi is derived, not measured: in the eigenbasis of A = Mhat^H
Mhat both sides are sums over eigenvalues y of |phi_y|^2 times R(y) and y^(-1/2), and |R(y) - y^(-1/2)| <= delta y^(-1/2)
for every y in [ra, rb]; the dense solves add their rounding, for which 1e-12 (relative) is allowed.  The CG distances are
the restatement's own named constants, measured by its --measure (profiles/su3_wilson_multishift/restatement_measure.txt),
and are held here."""
import numpy as np
import pytest

import wilson_eo_restatement as we
import wilson_force_restatement as wfr
import wilson_multishift_restatement as ms
import wilson_restatement as wr


@pytest.fixture(scope='module')
def rat():
    return ms.rational()


@pytest.mark.parametrize('L', ms.SOLVER_LATTICES)
def test_multishift_cg_against_dense_solves(L):
    x, phi = wr.links(L, 2), wr.spinors(L, 2, 2) * we.mask(L, 0)
    phi[1, 1] = 0.0                                                      # a zero right-hand side stays zero
    X, info = ms.multishift_cg(x, phi, ms.K, ms.SHIFTS, tol=ms.SOLVE_TOL)
    want = ms.dense_shifted(x, phi, ms.K, ms.SHIFTS)
    d = float(np.abs(X - want).max())
    print(L, f'max |X_cg - X_dense| = {d:.3g}', info['iters'].tolist(), info['shift_iters'].tolist())
    assert d <= ms.CG_X
    assert info['converged'].all() and (info['residual'] <= ms.SOLVE_TOL).all()
    assert not X[1, 1].any() and (info['shift_iters'][1, 1] == 0).all() and info['iters'][1, 1] == 0
    # a larger shift never freezes later, and no shift after its system
    si = info['shift_iters']
    assert (np.diff(si, axis=-1) <= 0).all() and (si <= info['iters'][..., None]).all()
    # freezing changes nothing beyond the tolerance, and a system's bits do not depend on the batch
    X2, info2 = ms.multishift_cg(x, phi, ms.K, ms.SHIFTS, tol=ms.SOLVE_TOL, freeze=False)
    assert np.abs(X2 - want).max() <= ms.CG_X and (info2['shift_iters'] == info2['iters'][..., None]).all()
    X1, _ = ms.multishift_cg(x[1:], phi[1:, :1], ms.K, ms.SHIFTS, tol=ms.SOLVE_TOL)
    assert np.array_equal(X1[0, 0], X[1, 0])
    # shifts = [0] is the normal-equation solve
    X0, _ = ms.multishift_cg(x, phi, ms.K, [0.0], tol=ms.SOLVE_TOL)
    Xn = we.normal_cg_eo(x, phi, ms.K, tol=ms.SOLVE_TOL)[0]
    assert np.abs(X0[:, :, 0] - Xn).max() <= 2 * ms.CG_X


@pytest.mark.parametrize('L', ms.LATTICES)
def test_action_and_heatbath(L, rat):
    kap = wfr.TRAJ['kappa']
    x, v, phi_l, phi_s = ms.traj_inputs(L)
    ms.assert_spectrum(x, kap, rat)
    sd, ex = ms.rat_action(x, phi_s, kap, rat), ms.exact_action(x, phi_s, kap)
    rel = np.abs(sd - ex) / ex
    print(L, f'|S_R - S_exact| / S_exact = {rel}, delta {rat.delta:.3g}')
    assert (rel <= rat.delta + 1e-12).all()
    assert (rel > 1e-3 * rat.delta).any()                                # the bound is not vacuous: R's error is seen
    sc = ms.rat_action(x, phi_s, kap, rat, tol=wfr.TRAJ_TOL_H)
    assert (np.abs(sc - sd) <= ms.CG_S * sd).all()
    # S(C eta) = |eta|^2, dense and with both solves by the multi-shift CG
    eta = we.gaussian_eta_e(L, 2, 1, seed=1)
    for tol, bound in ((None, ms.CG_S0), (wfr.TRAJ_TOL_H, ms.CG_S0)):
        phi, s0 = ms.rat_refresh(x, eta, kap, rat, tol=tol)
        assert not (phi * we.mask(L, 1)).any()
        s = ms.rat_action(x, phi, kap, rat, tol=tol)
        assert (np.abs(s - s0) <= bound * s0).all(), (tol, np.abs(s - s0) / s0)


@pytest.mark.parametrize('ap', [False, True])
@pytest.mark.parametrize('L', we.FD_LATTICES)
def test_force_against_differences(L, ap, rat):
    x, phi, p = ms.fd_inputs(L)
    ms.assert_spectrum(x, ms.K, rat, ap)
    want = wfr.pair(p, ms.rat_force(x, phi, ms.K, rat, ap))
    d, d1, d2 = ms.richardson(x, phi, p, ms.K, rat, ap)
    rel = np.abs(d - want) / np.abs(want)
    ratio = (d1 - want) / (d2 - want)
    print(L, ap, rel, ratio)
    assert (rel <= ms.CG_FD).all()
    assert ((ratio > 3.5) & (ratio < 4.5)).all()                         # the raw differences converge as h^2
    f = ms.rat_force(x, phi, ms.K, rat, ap)
    # exactly anti-Hermitian; traceless to the rounding of the three diagonal entries (the trace part is subtracted in
    # floating point: one ulp of the largest entry each, and one for the sum)
    assert np.abs(f + wfr.adj(f)).max() == 0.0
    assert np.abs(np.einsum('...ii->...', f)).max() <= 4 * 2.0 ** -52 * np.abs(f).max()


def test_leapfrog_is_reversible_and_dh_scales(rat):
    L = (2, 2, 2, 2)
    x, v, phi_l, phi_s = ms.traj_inputs(L)
    kw = dict(wfr.TRAJ, rat=rat, kappa_light=ms.KAPPA_LIGHT)
    x1, v1, dh = ms.delta_h(x, v, phi_l, phi_s, **kw)
    ms.assert_spectrum(x1, wfr.TRAJ['kappa'], rat)
    xb, vb = ms.leapfrog(x1, -v1, phi_l, phi_s, **kw)
    assert np.abs(xb - x).max() <= 1e-12 and np.abs(vb + v).max() <= 1e-12
    half = dict(kw, eps=kw['eps'] / 2, nleapfrog=2 * kw['nleapfrog'])
    ratio = dh / ms.delta_h(x, v, phi_l, phi_s, **half)[2]
    print('dH', dh, 'ratio', ratio)
    assert ((ratio > 3.5) & (ratio < 4.5)).all()
