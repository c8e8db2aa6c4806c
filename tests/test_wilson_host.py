"""CPU tier of the Wilson fermions: the numpy restatement tests/wilson_restatement.py pinned by what the operator must
satisfy whatever the kernel does -- the Clifford algebra, the adjoint and gamma5 identities, the free dispersion relation
(which fixes the normalisation in any basis), gauge covariance, a dense solve -- and the pure functions
`pion_correlator` / `effective_mass` on hand-made inputs.  These validate the ruler that tests/test_wilson_gpu.py and
tests/test_wilson_emu.py measure with."""
import numpy as np
import pytest
import torch

import gaugefix_restatement as gf
import wilson_restatement as wr

SMALL = [(2, 2, 2, 2), (4, 2, 6, 2), (3, 4, 5, 2), (4, 1, 6, 2)]


def inner(a, b):
    """<a, b> per system"""
    return (a.conj() * b).sum(axis=tuple(range(2, a.ndim)))


def test_gamma_matrices():
    g = wr.GAMMA
    for mu in range(4):
        assert np.array_equal(g[mu], g[mu].conj().T)
        for nu in range(4):
            assert np.array_equal(g[mu] @ g[nu] + g[nu] @ g[mu], 2.0 * (mu == nu) * np.eye(4)), (mu, nu)
        assert np.array_equal(g[4] @ g[mu], -g[mu] @ g[4])
    assert np.array_equal(g[4], np.diag([-1, -1, 1, 1])) and np.array_equal(g[4], g[4].conj().T)
    assert np.array_equal(g[4], g[0] @ g[1] @ g[2] @ g[3])
    # the project's own table is the same basis
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    assert np.array_equal(LatticeSU3.gamma_matrices().numpy(), g)


@pytest.mark.parametrize('ap', [False, True])
@pytest.mark.parametrize('L', SMALL)
def test_adjoint_and_gamma5(L, ap):
    x, psi = wr.links(L, 2), wr.spinors(L, 2, 3)
    phi = wr.spinors(L, 2, 6)[:, 3:]
    m, md = wr.wilson(x, psi, wr.KAPPA, False, ap), wr.wilson(x, phi, wr.KAPPA, True, ap)
    # 24 V products of O(1) numbers per inner product: rounding stays below 24 V eps times a few
    tol = 24 * np.prod(L) * 2.0 ** -52 * 8
    assert np.abs(inner(phi, m) - inner(md, psi)).max() <= tol * np.abs(inner(phi, m)).max()
    g5 = np.diag(wr.GAMMA[4]).real[:, None]
    assert np.abs(g5 * wr.wilson(x, g5 * psi, wr.KAPPA, False, ap) - wr.wilson(x, psi, wr.KAPPA, True, ap)).max() <= wr.TOL


@pytest.mark.parametrize('ap', [False, True])
@pytest.mark.parametrize('L,n', [((4, 4, 4, 4), (1, 0, 3, 2)), ((3, 4, 5, 2), (2, 1, 4, 1)), ((4, 1, 6, 2), (0, 0, 5, 1)),
                                 ((1, 2, 2, 3), (0, 1, 0, 2))])
def test_free_dispersion(L, n, ap):
    for dagger in (False, True):
        x, psi, want = wr.free_wave(L, wr.KAPPA, n, ap)
        got = wr.norm2(wr.wilson(x, psi, wr.KAPPA, dagger, ap)) / wr.norm2(psi)
        assert abs(float(got[0, 0]) - want) <= 1e-13 * max(1.0, want), (dagger, got, want)


@pytest.mark.parametrize('L', SMALL[:3])
def test_gauge_covariance(L):
    x, psi = wr.links(L, 2), wr.spinors(L, 2, 2)
    g = gf.random_su3(np.random.default_rng(41), (2, *L))
    xg = np.stack([g @ x[:, mu] @ np.roll(g, -1, axis=1 + mu).conj().swapaxes(-1, -2) for mu in range(4)], 1)
    gpsi = np.einsum('btxyzij,brtxyzaj->brtxyzai', g, psi)
    for dagger, ap in wr.FLAGS:
        a = wr.wilson(xg, gpsi, wr.KAPPA, dagger, ap)
        b = np.einsum('btxyzij,brtxyzaj->brtxyzai', g, wr.wilson(x, psi, wr.KAPPA, dagger, ap))
        assert np.abs(a - b).max() <= wr.TOL, (dagger, ap)


@pytest.mark.parametrize('L', SMALL)
def test_yardstick_of_small_lattices(L):
    assert wr.measure([L]) <= wr.YARDSTICK


@pytest.mark.parametrize('L', [(2, 2, 2, 2), (4, 2, 2, 2)])
def test_cgnr_against_dense_solve(L):
    tol = 1e-10
    x = wr.links(L, 1)
    b = wr.spinors(L, 1, 2)
    for kappa in wr.SOLVE_KAPPAS:
        m = wr.dense(x, kappa)
        smin = np.linalg.svd(m, compute_uv=False)[-1]
        psi, info = wr.cgnr(x, b, kappa, tol=tol, max_iter=200)
        assert info['converged'].all() and (info['residual'] <= 2 * tol).all()
        for j in range(2):
            want = np.linalg.solve(m, b[0, j].reshape(-1))
            bound = 2 * tol * np.linalg.norm(b[0, j]) / smin
            assert np.linalg.norm(psi[0, j].reshape(-1) - want) <= bound, (kappa, j)


def test_restatement_iteration_counts():
    """what the GPU solver test leans on: on its inputs the restatement alone converges well inside max_iter = 200, within
    63 iterations at kappa = 0.10 and within 123 at 0.12 (looked at every 10: found at the checks at 70 and 130 at the
    latest; on these two lattices it is found at 40 - 50 and 60 - 80)"""
    for L in [(2, 2, 2, 2), (3, 4, 5, 2)]:
        x, b = wr.links(L, 3), wr.spinors(L, 3, 2)
        for kappa, most in zip(wr.SOLVE_KAPPAS, (70, 130)):
            _, info = wr.cgnr(x, b, kappa, tol=1e-10, max_iter=200)
            print(L, kappa, info['iters'].max())
            assert info['converged'].all() and info['iters'].max() <= most, (L, kappa, info['iters'])


def test_zero_source_and_max_iter():
    L = (2, 2, 2, 2)
    x, b = wr.links(L, 1), wr.spinors(L, 1, 2)
    b[0, 1] = 0.0
    psi, info = wr.cgnr(x, b, 0.10)
    assert not psi[0, 1].any() and info['converged'].all() and info['iters'][0, 1] == 0 and info['residual'][0, 1] == 0
    _, info = wr.cgnr(x, b[:, :1], 0.10, max_iter=5)
    assert not info['converged'].any() and (info['iters'] == 5).all()


def test_pion_correlator_and_effective_mass():
    from l2hmc.lattice.su3.pytorch.lattice import effective_mass, pion_correlator
    nb, T = 2, 5
    S = torch.zeros((nb, T, 2, 1, 3, 4, 3, 4, 3), dtype=torch.complex128)
    S[0, :, 1, 0, 2, 3, 1, 0, 2] = torch.tensor([1.0, 2.0j, 3.0, -4.0, 5.0j])
    S[0, 2, 0, 0, 0, 1, 1, 1, 1] = 1.0 + 1.0j
    S[1] = 0.5
    C = pion_correlator(S)
    assert C.shape == (nb, T)
    assert torch.equal(C[0], torch.tensor([1.0, 4.0, 11.0, 16.0, 25.0], dtype=torch.float64))
    assert torch.equal(C[1], torch.full((T,), 0.25 * 6 * 144, dtype=torch.float64))
    assert torch.equal(pion_correlator(S, 2)[0], torch.tensor([11.0, 16.0, 25.0, 1.0, 4.0], dtype=torch.float64))
    assert np.array_equal(wr.pion_correlator(S.numpy(), 2), pion_correlator(S, 2).numpy())
    # an exact exponential gives its mass everywhere; a non-positive ratio gives NaN and nothing raises
    c = torch.exp(-0.7 * torch.arange(6, dtype=torch.float64))[None]
    m = effective_mass(c)
    assert m.shape == (1, 5) and float((m - 0.7).abs().max()) <= 1e-14
    bad = torch.tensor([[1.0, -1.0, 2.0, 0.0]], dtype=torch.float64)
    assert effective_mass(bad).shape == (1, 3) and bool(torch.isnan(effective_mass(bad)).all())
    with pytest.raises(ValueError):
        pion_correlator(torch.zeros(2, 4, 4, 4, 4, 4, 3))


def test_free_correlator_is_symmetric():
    """unit links: C(t) = C(T - t), periodic or antiperiodic (|S|^2 does not see the sign)"""
    L = (6, 2, 2, 2)
    x = np.broadcast_to(np.eye(3, dtype=complex), (1, 4, *L, 3, 3)).copy()
    for ap in (False, True):
        S, info = wr.propagator(x, 0.10, tol=1e-12, antiperiodic_t=ap)
        assert info['converged'].all()
        C = wr.pion_correlator(S)[0]
        assert (C > 0).all()
        # the solver leaves a relative error of tol / sigma_min(M) <= 1e-12 / (1 - 8 kappa) in S, twice that in C
        assert np.abs(C[1:] - C[1:][::-1]).max() <= 4 * 1e-12 / (1 - 0.8) * C.max(), C
        # the source moved along with t_source gives the same correlator
        S1, _ = wr.propagator(x, 0.10, source=(1, 0, 1, 0), tol=1e-12, antiperiodic_t=ap)
        assert np.abs(wr.pion_correlator(S1, 1)[0] - C).max() <= 4 * 1e-12 / (1 - 0.8) * C.max()
