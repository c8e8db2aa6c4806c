"""GPU tests of the Wilson-fermion kernels (csrc/su3_wilson.hip) and of what is built on them: single launches of the
operator against the numpy restatement tests/wilson_restatement.py, then the public interface of LatticeSU3 (the two
layouts, the adjoint identity, gauge covariance, the free dispersion relation), the batched CGNR solver (convergence,
true residual, a dense solve, systems that freeze independently) and the propagator with its pion correlator.

Inputs are the smooth links of the smearing tests and Gaussian spinors from a fixed seed (wr.links, wr.spinors).  The
tolerance of a single application is wr.TOL = 32 x the extended-precision yardstick (2.56e-14; derivation in
tests/wilson_restatement.py and profiles/su3_wilson.md)."""
import functools

import numpy as np
import pytest
import torch

import gaugefix_restatement as gf
import wilson_restatement as wr
from wilson_gpu_util import dev, host, unit_links

gpu = pytest.mark.gpu
NB = 3
TOL_SOLVE = 1e-10


@functools.lru_cache(maxsize=None)
def reference(L):
    """links, spinors and the restatement's M psi for flags 0..3 at nrhs = 12 (nrhs = 1 is its first column)"""
    x, psi = wr.links(L, NB), wr.spinors(L, NB, 12)
    return x, psi, [wr.wilson(x, psi, wr.KAPPA, dagger, ap) for dagger, ap in wr.FLAGS]


@gpu
@pytest.mark.parametrize('L', wr.GPU_LATTICES)
def test_apply_against_restatement(L):
    from l2hmc import _ops as ops
    x, psi, want = reference(L)
    V = int(np.prod(L))
    xn = ops.su3_pack(dev(x))
    keepx = xn.clone()
    worst = worstn = 0.0
    for nrhs in (1, 12):
        pn = ops.su3_spinor_pack(dev(psi[:, :nrhs]))
        keep = pn.clone()
        for (dagger, ap), w in zip(wr.FLAGS, want):
            out, part = ops.su3_wilson_apply_n(xn, pn, wr.KAPPA, L, dagger, ap, norm=True)
            assert out.shape == pn.shape and out.data_ptr() != pn.data_ptr()
            assert part.shape == (NB, nrhs, ops.su3_wilson_norm_parts(L)) and part.shape[-1] == -(-V // 256)
            got = host(ops.su3_spinor_unpack(out, L))
            d = float(np.abs(got - w[:, :nrhs]).max())
            worst = max(worst, d)
            assert d <= wr.TOL, (nrhs, dagger, ap, d)
            n2 = wr.norm2(w[:, :nrhs])
            rel = float((np.abs(host(part).sum(-1) - n2) / n2).max())
            worstn = max(worstn, rel)
            assert rel <= wr.norm_bound(V), (nrhs, dagger, ap, rel)
            assert torch.equal(ops.su3_wilson_apply_n(xn, pn, wr.KAPPA, L, dagger, ap), out)     # the norm changes nothing
        assert torch.equal(pn, keep)
        # an output given by the caller is the one written and returned
        mine = torch.full_like(pn, -7.0)
        assert ops.su3_wilson_apply_n(xn, pn, wr.KAPPA, L, out=mine) is mine
        assert np.abs(host(ops.su3_spinor_unpack(mine, L)) - want[2][:, :nrhs]).max() <= wr.TOL   # the defaults: flags 2
    assert torch.equal(xn, keepx)
    print(f'{L}: worst deviation / tolerance {worst / wr.TOL:.3g}, norm {worstn / wr.norm_bound(V):.3g}')


@gpu
@pytest.mark.parametrize('L', wr.API_LATTICES)
def test_public_interface(L):
    from l2hmc import _ops as ops
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    lat = LatticeSU3(NB, list(L))
    V = int(np.prod(L))
    x0, psi0 = wr.links(L, NB), wr.spinors(L, NB, 4)
    x, psi = dev(x0), dev(psi0)
    phi0 = wr.spinors(L, NB, 8)[:, 4:]
    keepx, keepp = x.clone(), psi.clone()
    xn, pn = lat.pack(x).clone(), ops.su3_spinor_pack(psi)
    for dagger, ap in wr.FLAGS:
        y = lat.wilson_dirac(x, psi, wr.KAPPA, dagger, ap)
        yn = lat.wilson_dirac_n(xn, pn, wr.KAPPA, dagger, ap)
        assert y.shape == psi.shape and yn.shape == pn.shape
        assert torch.equal(ops.su3_spinor_unpack(yn, L), y)                              # one code path, two layouts
        assert np.abs(host(y) - wr.wilson(x0, psi0, wr.KAPPA, dagger, ap)).max() <= wr.TOL
        # a field without the nrhs axis comes back without it
        y1 = lat.wilson_dirac(x, psi[:, 1], wr.KAPPA, dagger, ap)
        assert y1.shape == psi[:, 1].shape and torch.equal(y1, y[:, 1])
        assert torch.equal(lat.wilson_dirac_n(xn, pn[:, 1], wr.KAPPA, dagger, ap), yn[:, 1])
        # <phi, M psi> = <M^H phi, psi> per chain and right-hand side: 24 V products of O(1) numbers each
        m = host(y)
        md = host(lat.wilson_dirac(x, dev(phi0), wr.KAPPA, not dagger, ap))
        a, b = (phi0.conj() * m).sum(axis=(2, 3, 4, 5, 6, 7)), (md.conj() * psi0).sum(axis=(2, 3, 4, 5, 6, 7))
        assert np.abs(a - b).max() <= 24 * V * 2.0 ** -52 * 8 * np.abs(a).max(), (dagger, ap)
    assert torch.equal(lat.wilson_dirac(x, psi, wr.KAPPA), lat.wilson_dirac(x, psi, wr.KAPPA, False, True))
    assert torch.equal(x, keepx) and torch.equal(psi, keepp)                            # inputs are never written
    # gauge covariance through the project's own gauge_transform: M[U^g](g psi) = g M[U] psi
    g0 = gf.random_su3(np.random.default_rng(41), (NB, *L))
    gx = lat.gauge_transform(x, dev(g0))
    gpsi = np.einsum('btxyzij,brtxyzaj->brtxyzai', g0, psi0)
    for dagger, ap in wr.FLAGS:
        lhs = host(lat.wilson_dirac(gx, dev(gpsi), wr.KAPPA, dagger, ap))
        rhs = np.einsum('btxyzij,brtxyzaj->brtxyzai', g0, host(lat.wilson_dirac(x, psi, wr.KAPPA, dagger, ap)))
        d = float(np.abs(lhs - rhs).max())
        assert d <= wr.TOL, (dagger, ap, d)
    # the free dispersion relation on unit links (fixes the normalisation in any basis)
    for ap in (False, True):
        xu, wave, want = wr.free_wave(L, wr.KAPPA, (1, 2, 3, 1), ap)
        for dagger in (False, True):
            mw = host(LatticeSU3(1, list(L)).wilson_dirac(dev(xu), dev(wave), wr.KAPPA, dagger, ap))
            got = float((wr.norm2(mw) / wr.norm2(wave))[0, 0])
            assert abs(got - want) <= 1e-13 * max(1.0, want), (ap, dagger, got, want)


@functools.lru_cache(maxsize=None)
def solver_inputs(L):
    return wr.links(L, NB), wr.spinors(L, NB, 2)


@gpu
@pytest.mark.parametrize('kappa', wr.SOLVE_KAPPAS)
@pytest.mark.parametrize('L', [(3, 4, 5, 2), (4, 4, 4, 4), (4, 4, 4, 10)])
def test_solver_converges(L, kappa):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    lat = LatticeSU3(NB, list(L))
    x0, b0 = solver_inputs(L)
    x, b = dev(x0), dev(b0)
    keep = b.clone()
    psi, info = lat.wilson_solve(x, b, kappa, tol=TOL_SOLVE, max_iter=200)
    assert torch.equal(b, keep) and psi.shape == b.shape
    for k in ('iters', 'residual', 'converged'):
        assert tuple(info[k].shape) == (NB, 2), k
    print(f"{L} kappa {kappa}: iters {host(info['iters']).tolist()}, residual {host(info['residual']).max():.3g}")
    assert bool(info['converged'].all())
    assert int(info['iters'].max()) <= 200 and int(info['iters'].min()) > 0
    assert float(info['residual'].max()) <= 2 * TOL_SOLVE
    # the residual recomputed by the restatement from the returned solution
    res = np.sqrt(wr.norm2(b0 - wr.wilson(x0, host(psi), kappa)) / wr.norm2(b0))
    assert res.max() <= 2 * TOL_SOLVE, res
    # a single right-hand side without the nrhs axis
    p1, i1 = lat.wilson_solve(x, b[:, 1], kappa, tol=TOL_SOLVE, max_iter=200)
    assert p1.shape == b[:, 1].shape and tuple(i1['iters'].shape) == (NB, 1) and torch.equal(p1, psi[:, 1])


@gpu
def test_solver_against_dense_solve():
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (2, 2, 2, 2)
    x0, b0 = solver_inputs(L)
    lat = LatticeSU3(NB, list(L))
    for kappa in wr.SOLVE_KAPPAS:
        psi, info = lat.wilson_solve(dev(x0), dev(b0), kappa, tol=TOL_SOLVE, max_iter=200)
        assert bool(info['converged'].all())
        for c in range(NB):
            m = wr.dense(x0[c:c + 1], kappa)
            smin = np.linalg.svd(m, compute_uv=False)[-1]
            for j in range(2):
                want = np.linalg.solve(m, b0[c, j].reshape(-1))
                d = np.linalg.norm(host(psi)[c, j].reshape(-1) - want)
                assert d <= 2 * TOL_SOLVE * np.linalg.norm(b0[c, j]) / smin, (kappa, c, j, d)


@gpu
def test_systems_freeze_independently():
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (3, 4, 5, 2)
    x0, b0 = solver_inputs(L)
    x0 = x0.copy()
    x0[1] = unit_links(1, L)[0]                       # the free field converges many checks earlier
    b0 = b0.copy()
    b0[2, 1] = 0.0                                    # and a zero right-hand side at once
    x, b = dev(x0), dev(b0)
    lat3, lat1 = LatticeSU3(NB, list(L)), LatticeSU3(1, list(L))
    psi, info = lat3.wilson_solve(x, b, 0.12, tol=TOL_SOLVE, max_iter=200)
    it = host(info['iters'])
    print('iters', it.tolist())
    assert bool(info['converged'].all()) and float(info['residual'].max()) <= 2 * TOL_SOLVE
    assert it[1].max() < it[0].min() and it[1].max() < it[2, 0]
    assert it[2, 1] == 0 and not bool(psi[2, 1].any()) and float(info['residual'][2, 1]) == 0.0
    # any one chain, any one right-hand side alone: the same bits (freezing and the partial sums do not see the batch)
    for c in range(NB):
        pc, ic = lat1.wilson_solve(x[c:c + 1].clone(), b[c:c + 1].clone(), 0.12, tol=TOL_SOLVE, max_iter=200)
        assert torch.equal(pc, psi[c:c + 1]) and torch.equal(ic['iters'], info['iters'][c:c + 1]), c
    for j in range(2):
        pj, ij = lat3.wilson_solve(x, b[:, j:j + 1].clone(), 0.12, tol=TOL_SOLVE, max_iter=200)
        assert torch.equal(pj, psi[:, j:j + 1]) and torch.equal(ij['iters'], info['iters'][:, j:j + 1]), j
    # too few iterations: nothing raises
    _, i5 = lat3.wilson_solve(x, b[:, :1].clone(), 0.12, tol=TOL_SOLVE, max_iter=5)
    assert not bool(i5['converged'].any()) and bool((i5['iters'] == 5).all()) and float(i5['residual'].min()) > TOL_SOLVE


@gpu
def test_propagator_against_dense_inverse():
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 2, 2, 2)
    x0 = wr.links(L, NB)
    x = dev(x0)
    lat = LatticeSU3(NB, list(L))
    kappa, src = 0.10, (2, 1, 0, 1)
    S, info = lat.quark_propagator(x, kappa, source=src, tol=TOL_SOLVE, max_iter=200)
    assert S.shape == (NB, *L, 4, 3, 4, 3) and tuple(info['iters'].shape) == (NB, 12) and bool(info['converged'].all())
    bsrc = wr.point_sources(NB, L, src)
    for c in range(NB):
        m = wr.dense(x0[c:c + 1], kappa)
        smin = np.linalg.svd(m, compute_uv=False)[-1]
        inv = np.linalg.solve(m, bsrc[c].reshape(12, -1).T)                  # [12 V, 12 sources]
        got = host(S)[c].reshape(-1, 12)
        assert np.linalg.norm(got - inv, axis=0).max() <= 2 * TOL_SOLVE / smin, c
    # column j is wilson_solve of that source alone, bit for bit
    b = dev(bsrc)
    for j in (0, 7, 11):
        pj, _ = lat.wilson_solve(x, b[:, j], kappa, tol=TOL_SOLVE, max_iter=200)
        assert torch.equal(pj, S[..., j // 3, j % 3]), j
    with pytest.raises(ValueError, match='source'):
        lat.quark_propagator(x, kappa, source=(4, 0, 0, 0))


@gpu
def test_pion_correlator():
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3, effective_mass, pion_correlator
    L = (6, 2, 2, 2)
    lat = LatticeSU3(NB, list(L))
    x0 = wr.links(L, NB)
    x0[1] = unit_links(1, L)[0]
    x = dev(x0)
    S, info = lat.quark_propagator(x, 0.10, tol=TOL_SOLVE, max_iter=200)
    assert bool(info['converged'].all())
    C = pion_correlator(S)
    assert C.shape == (NB, L[0]) and bool((C > 0).all())
    assert effective_mass(C).shape == (NB, L[0] - 1)
    # a sum of n = 2 * 144 * X Y Z squares per entry, in another order than numpy's: relative n eps at most, doubled
    cr = wr.pion_correlator(host(S))
    assert (np.abs(host(C) - cr) <= 2 * (288 * 8) * 2.0 ** -53 * cr).all()
    # unit links: symmetric under t -> T - t to the solver's tolerance (relative error of S at most tol / sigma_min,
    # sigma_min >= 1 - 8 kappa for the free operator; twice that in C, and two entries compared)
    c = host(C)[1]
    bound = 4 * TOL_SOLVE / (1 - 0.8) * c.max()
    assert np.abs(c[1:] - c[1:][::-1]).max() <= bound, c
    # and the restatement's own free correlator
    Sr, _ = wr.propagator(x0[1:2], 0.10, tol=TOL_SOLVE)
    assert np.abs(c - wr.pion_correlator(Sr)[0]).max() <= bound
    # the source moved to (1, 0, 1, 0), t counted from it: the same free correlator
    S1, _ = lat.quark_propagator(x, 0.10, source=(1, 0, 1, 0), tol=TOL_SOLVE, max_iter=200)
    assert np.abs(host(pion_correlator(S1, t_source=1))[1] - c).max() <= bound
    assert float((pion_correlator(S1, t_source=1)[0] - C[0]).abs().max()) > 1e-6        # not so on a real gauge field
    # smeared links are links
    xs = lat.hyp_smear(x)
    psi, inf = lat.wilson_solve(xs, dev(wr.spinors(L, NB, 1)), 0.10, tol=TOL_SOLVE, max_iter=200)
    assert bool(inf['converged'].all())
    res = np.sqrt(wr.norm2(wr.spinors(L, NB, 1) - wr.wilson(host(xs), host(psi), 0.10)) / wr.norm2(wr.spinors(L, NB, 1)))
    assert res.max() <= 2 * TOL_SOLVE
