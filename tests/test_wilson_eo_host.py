"""CPU tier of even-odd preconditioning: the numpy restatement tests/wilson_eo_restatement.py held against identities
that do not depend on it -- the Schur identity of the full operator, the adjoint, det M = det Mhat, a dense solve of the
full M, the long-form force on the completed fields against Richardson differences of the even-odd action -- and the
iteration counts of the preconditioned CGNR against the unpreconditioned one.  No kernel runs here."""
import numpy as np
import pytest

import wilson_eo_restatement as we
import wilson_force_restatement as wfr
import wilson_restatement as wr

EPS = 2.0 ** -52


@pytest.mark.parametrize('L', we.EO_KERNEL_LATTICES)
def test_split_and_merge_are_inverse(L):
    psi = wr.spinors(L, 2, 3)
    V = int(np.prod(L))
    halves = [we.pack_half(psi, p) for p in (0, 1)]
    assert all(h.shape == (2, 3, 12, V // 2) for h in halves)
    assert np.array_equal(we.unpack_half(halves[0], L, 0) + we.unpack_half(halves[1], L, 1), psi)
    for p in (0, 1):
        assert np.array_equal(we.pack_half(we.unpack_half(halves[p], L, p), p), halves[p])
        assert np.array_equal(we.unpack_half(halves[p], L, p), psi * we.mask(L, p))
        s = we.sites(L, p)
        assert np.array_equal(s >> 1, np.arange(V // 2))            # entry h is the site 2h or 2h + 1
        assert np.array_equal(we.parity(L).reshape(-1)[s], np.full(V // 2, p))
    # H couples opposite parities only
    x = wr.links(L, 2)
    for p in (0, 1):
        assert not (wr.hop(x, psi * we.mask(L, p)) * we.mask(L, p)).any()


@pytest.mark.parametrize('L', we.EO_KERNEL_LATTICES)
def test_schur_identity_and_adjoint(L):
    """(M psi)_e + kappa H_eo (M psi)_o = Mhat psi_e for any full psi; <phi_e, Mhat psi_e> = <Mhat^H phi_e, psi_e>.  Sums
    of at most 24 V products of O(1) numbers, each output entry of size <= 40: a few hundred eps."""
    x, psi, phi = wr.links(L, 2), wr.spinors(L, 2, 2), wr.spinors(L, 2, 4)[:, 2:]
    V = int(np.prod(L))
    for dagger, ap in wr.FLAGS:
        m = wr.wilson(x, psi, we.K, dagger, ap)
        lhs = we.hop_eo(x, m, 0, dagger, ap, a=we.K, aux=m, b=1.0)
        rhs = we.schur(x, psi, we.K, dagger, ap)
        assert not (rhs * we.mask(L, 1)).any()
        assert np.abs(lhs - rhs).max() <= 64 * EPS, (dagger, ap)
        a = (phi.conj() * we.mask(L, 0) * rhs).sum(axis=(2, 3, 4, 5, 6, 7))
        b = (we.schur(x, phi, we.K, not dagger, ap).conj() * psi).sum(axis=(2, 3, 4, 5, 6, 7))
        assert np.abs(a - b).max() <= 24 * V * EPS * 8 * np.abs(a).max(), (dagger, ap)


@pytest.mark.parametrize('ap', [False, True])
@pytest.mark.parametrize('kappa', wr.SOLVE_KAPPAS)
def test_determinant(kappa, ap):
    """det M = det Mhat: the even-odd ensemble is the two-flavour ensemble"""
    L = (2, 2, 2, 2)
    x = wr.links(L, 1)
    m, mh = wr.dense(x, kappa, ap), we.dense_schur(x, kappa, ap)
    assert mh.shape == (96, 96)
    psi = wr.spinors(L, 1, 1)                                      # the dense Mhat is the operator
    got = (mh @ we.pack_half(psi, 0)[0, 0].T.reshape(-1)).reshape(8, 12).T
    assert np.abs(got - we.pack_half(we.schur(x, psi, kappa, False, ap), 0)[0, 0]).max() <= 64 * EPS
    d, dh = np.linalg.det(m), np.linalg.det(mh)
    assert abs(d - dh) <= 1e-12 * abs(d), (d, dh)


def test_solve_against_dense_and_iteration_counts():
    L = (2, 2, 2, 2)
    x, b = wr.links(L, 2), wr.spinors(L, 2, 2)
    for kappa in wr.SOLVE_KAPPAS:
        psi, info = we.solve_eo(x, b, kappa, tol=1e-12)
        assert info['converged'].all() and info['residual'].max() <= 2e-12
        for c in range(2):
            m = wr.dense(x[c:c + 1], kappa)
            smin = np.linalg.svd(m, compute_uv=False)[-1]
            for j in range(2):
                want = np.linalg.solve(m, b[c, j].reshape(-1))
                d = np.linalg.norm(psi[c, j].reshape(-1) - want)
                assert d <= 2e-12 * np.linalg.norm(b[c, j]) / smin, (kappa, c, j, d)
    zero = np.zeros_like(b)
    pz, iz = we.solve_eo(x, zero, 0.12)
    assert not pz.any() and (iz['iters'] == 0).all() and (iz['residual'] == 0).all()
    # the iteration condition: at most half the iterations of the full system, system by system
    L = (4, 4, 4, 4)
    x, b = wr.links(L, 2), wr.spinors(L, 2, 2)
    for kappa in wr.SOLVE_KAPPAS:
        full = we.full_cgnr(x, b, kappa, check_every=1)[1]
        eo = we.solve_eo(x, b, kappa, check_every=1)[1]
        print(kappa, 'full', full.ravel(), 'even-odd', eo['iters'].ravel(), 'residual', eo['residual'].max())
        assert eo['converged'].all() and eo['residual'].max() <= 2e-10
        assert (2 * eo['iters'] <= full).all()


@pytest.mark.parametrize('ap', [False, True])
def test_force_on_completed_fields_and_by_differences(ap):
    """The even-odd force is `wfr.force` on the completed fields; it is the derivative of the even-odd action (Richardson
    differences, dense solves: the 1e-8 of tests/test_wilson_force_host.py); and the even-odd action is not the full one"""
    L = (2, 2, 2, 2)
    x, phi, p = we.fd_inputs(L)
    Xe, Ye = we.dense_normal_eo(x, phi, we.K, ap)
    assert np.abs(we.schur(x, we.schur(x, Xe, we.K, False, ap), we.K, True, ap) - phi).max() <= 1e-12
    X, Y = we.completed(x, Xe, Ye, we.K, ap)
    # the completed fields: (M X)_o = 0 and (M^H Y)_o = 0, so Y^H dM X is the even-odd variation
    assert np.abs(wr.wilson(x, X, we.K, False, ap) * we.mask(L, 1)).max() <= 64 * EPS
    assert np.abs(wr.wilson(x, Y, we.K, True, ap) * we.mask(L, 1)).max() <= 64 * EPS
    f = we.fermion_force(x, phi, we.K, ap)
    assert np.array_equal(f, wfr.force(x, X, Y, we.K, ap))
    want = wfr.pair(p, f)
    d, d1, d2 = wfr.richardson(x, phi, p, we.K, ap, action=lambda xx: we.fermion_action(xx, phi, we.K, ap))
    rel = np.abs(d - want) / np.abs(want)
    print(ap, rel, (d1 - want) / (d2 - want))
    assert (rel <= 1e-8).all(), rel
    assert np.abs(we.fermion_action(x, phi, we.K, ap) - wfr.fermion_action(x, phi, we.K, ap)).min() > 1e-3


def test_refresh_and_leapfrog():
    L = (2, 2, 2, 2)
    x, v, phi, s0 = we.traj_inputs(L)
    assert not (phi * we.mask(L, 1)).any()
    s = we.fermion_action(x, phi, wfr.TRAJ['kappa'])
    assert np.abs(s - s0).max() <= 1e-12 * s0.max()
    x1, v1, dh = we.delta_h(x, v, phi, **wfr.TRAJ)
    x2, v2 = we.leapfrog(x1, -v1, phi, **wfr.TRAJ)
    assert max(np.abs(x2 - x).max(), np.abs(v2 + v).max()) <= 1e-12
    _, _, dh2 = we.delta_h(x, v, phi, **{**wfr.TRAJ, 'eps': wfr.TRAJ['eps'] / 2, 'nleapfrog': 2 * wfr.TRAJ['nleapfrog']})
    print('dH', dh, dh2, dh / dh2)
    assert ((dh / dh2 > 3.5) & (dh / dh2 < 4.5)).all()


def test_yardstick_holds():
    """the small lattices measured again: the recorded yardstick bounds them"""
    assert we.measure(we.EO_KERNEL_LATTICES[:2], nb=2, nrhs=3) <= we.YARDSTICK
