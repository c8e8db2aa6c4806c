"""CPU tier of the product's own CG loops: `LatticeSU3.wilson_solve_n` and `wilson_solve_normal_n`, and their even-odd
forms `wilson_solve_eo_n` and `wilson_solve_schur_normal_n`, run on CPU tensors with the five kernel entries of
`l2hmc._ops` they call replaced by numpy stand-ins built on tests/wilson_restatement.py and tests/wilson_eo_restatement.py
(`ops.sum_parts`, `su3_spinor_split_eo` and `su3_spinor_merge_eo` stay the real ones: they are pure torch).  What
tests/test_wilson_host.py and tests/test_wilson_force_host.py assert of the numpy CGs `wr.cgnr` / `wf.normal_cg` is
asserted here of the loops the GPU runs, with the same bounds: the dense solve, the freeze semantics, never raising --
and the launch sequence, which only the product has."""
import functools

import numpy as np
import pytest
import torch

import wilson_eo_restatement as we
import wilson_force_restatement as wf
import wilson_restatement as wr
from l2hmc import _ops as ops
from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3

LATTICES = [(4, 2, 6, 2), (2, 2, 2, 2)]
NB, NRHS = 2, 2


def norm_part(f):
    """[nb, nrhs, 1] float64: |f|^2 per system of a native spinor field, one partial sum each, summed row by row (a
    system's bits do not depend on the batch)"""
    a = f.numpy()
    return torch.from_numpy((a.real ** 2 + a.imag ** 2).reshape(*a.shape[:2], -1).sum(-1))[..., None]


class StandIns:
    """`su3_wilson_apply_n`, `su3_wilson_hop_eo_n`, `su3_spinor_cg_update_`, `su3_spinor_xpay_` and
    `su3_wilson_norm_parts` of `l2hmc._ops` on CPU tensors, with their signatures; `log` lists the calls as (entry,
    dagger, norm requested), a hop as ('hop', parity, dagger, norm requested)."""
    NAMES = ('su3_wilson_apply_n', 'su3_wilson_hop_eo_n', 'su3_spinor_cg_update_', 'su3_spinor_xpay_',
             'su3_wilson_norm_parts')

    def __init__(self, monkeypatch=None):
        self.log = []
        if monkeypatch is not None:
            for name in self.NAMES:
                monkeypatch.setattr(ops, name, getattr(self, name))

    def su3_wilson_norm_parts(self, lat):
        return 1

    def su3_wilson_apply_n(self, xn, psin, kappa, lat, dagger=False, antiperiodic_t=True, out=None, norm=False):
        want_norm = isinstance(norm, torch.Tensor) or bool(norm)
        self.log.append(('apply', bool(dagger), want_norm))
        psi = wr.unpack_spinor(psin.numpy(), lat)
        res = wr.wilson(wf.unpack_links(xn.numpy(), lat), psi, kappa, dagger, antiperiodic_t)
        out = torch.empty_like(psin) if out is None else out
        out.copy_(torch.from_numpy(wr.pack_spinor(res)))
        if not want_norm:
            return out
        part = norm if isinstance(norm, torch.Tensor) else torch.empty((*psin.shape[:2], 1), dtype=torch.float64)
        return out, part.copy_(norm_part(out))

    def su3_wilson_hop_eo_n(self, xn, src, lat, parity, dagger=False, antiperiodic_t=True, a=1.0, aux=None, b=0.0,
                            out=None, norm=False):
        want_norm = isinstance(norm, torch.Tensor) or bool(norm)
        self.log.append(('hop', int(parity), bool(dagger), want_norm))
        res = we.hop_eo(wf.unpack_links(xn.numpy(), lat), we.unpack_half(src.numpy(), lat, 1 - parity), parity, dagger,
                        antiperiodic_t, a, None if aux is None else we.unpack_half(aux.numpy(), lat, parity), b)
        out = torch.empty_like(src) if out is None else out              # out may be aux: res is complete by now
        out.copy_(torch.from_numpy(we.pack_half(res, parity)))
        if not want_norm:
            return out
        part = norm if isinstance(norm, torch.Tensor) else torch.empty((*src.shape[:2], 1), dtype=torch.float64)
        return out, part.copy_(norm_part(out))

    def su3_spinor_cg_update_(self, x, r, p, q, alpha, part=None):
        self.log.append(('update', None, None))
        a = alpha.reshape(*x.shape[:2], 1, 1)
        x.add_(a * p)
        r.sub_(a * q)
        part = torch.empty((*x.shape[:2], 1), dtype=torch.float64) if part is None else part
        return part.copy_(norm_part(r))

    def su3_spinor_xpay_(self, p, z, beta):
        self.log.append(('xpay', None, None))
        return p.mul_(beta.reshape(*p.shape[:2], 1, 1)).add_(z)


@pytest.fixture
def standins(monkeypatch):
    return StandIns(monkeypatch)


def inputs(L, nb=NB, nrhs=NRHS):
    """(lattice, x, b, xn, bn): the links and right-hand sides of the numpy tests, and their native CPU tensors"""
    x, b = wr.links(L, nb), wr.spinors(L, nb, nrhs)
    return LatticeSU3(nb, list(L)), x, b, torch.from_numpy(wf.pack_links(x)), torch.from_numpy(wr.pack_spinor(b))


@functools.lru_cache(maxsize=None)
def dense(L, kappa):
    """per chain of `inputs(L)`: (M dense, its smallest and largest singular value)"""
    out = []
    for c in range(NB):
        m = wr.dense(wr.links(L, NB)[c:c + 1], kappa)
        s = np.linalg.svd(m, compute_uv=False)
        out.append((m, s[-1], s[0]))
    return out


def solve(lat, which, xn, bn, kappa, **kw):
    """(solution, info) of one of the four solvers; 'schur_normal' takes the even half of bn for its right-hand side"""
    if which in ('cgnr', 'eo'):
        return (lat.wilson_solve_n if which == 'cgnr' else lat.wilson_solve_eo_n)(xn, bn, kappa, **kw)
    if which == 'schur_normal':
        X, _, info = lat.wilson_solve_schur_normal_n(xn, ops.su3_spinor_split_eo(bn, lat._lattice_shape)[0], kappa, **kw)
    else:
        X, _, info = lat.wilson_solve_normal_n(xn, bn, kappa, **kw)
    return X, info


@pytest.mark.parametrize('L', LATTICES)
def test_cgnr_against_dense_solve(standins, L):
    """the bound of test_wilson_host.py::test_cgnr_against_dense_solve: |psi - M^-1 b| <= 2 tol |b| / sigma_min(M)"""
    tol = 1e-10
    lat, x, b, xn, bn = inputs(L)
    for kappa in wr.SOLVE_KAPPAS:
        psin, info = lat.wilson_solve_n(xn, bn, kappa, tol=tol, max_iter=200)
        assert info['converged'].all() and (info['residual'] <= 2 * tol).all(), (kappa, info)
        psi = wr.unpack_spinor(psin.numpy(), L)
        for c, (m, smin, _) in enumerate(dense(L, kappa)):
            for j in range(NRHS):
                want = np.linalg.solve(m, b[c, j].reshape(-1))
                err, bound = np.linalg.norm(psi[c, j].reshape(-1) - want), 2 * tol * np.linalg.norm(b[c, j]) / smin
                print(L, kappa, c, j, 'iters', int(info['iters'][c, j]), 'error', err, 'bound', bound)
                assert err <= bound, (kappa, c, j)


@pytest.mark.parametrize('L', LATTICES)
def test_normal_cg_against_dense_solve(standins, L):
    """the bound of test_wilson_force_host.py::test_normal_cg: |dX| <= cond(M^H M) * residual, cond < 100 (held here
    from the singular values of the dense M), and info['action'] = |Y|^2 by the same sums"""
    lat, x, b, xn, bn = inputs(L)
    for kappa in wr.SOLVE_KAPPAS:
        assert all((smax / smin) ** 2 < 100 for _, smin, smax in dense(L, kappa))
        Xd = np.stack([np.linalg.solve(m.conj().T @ m, b[c].reshape(NRHS, -1).T).T.reshape(b.shape[1:])
                       for c, (m, _, _) in enumerate(dense(L, kappa))])
        for tol in (1e-6, 1e-10):
            Xn, Yn, info = lat.wilson_solve_normal_n(xn, bn, kappa, tol=tol)
            assert info['converged'].all() and (info['residual'] <= 2 * tol).all(), (kappa, tol, info)
            err = np.abs(wr.unpack_spinor(Xn.numpy(), L) - Xd).max()
            print(L, kappa, tol, 'iters', info['iters'].tolist(), 'error', err, 'bound', 100 * tol * np.abs(Xd).max())
            assert err <= 100 * tol * np.abs(Xd).max()
            assert torch.equal(info['action'], ops.sum_parts(norm_part(Yn)))
            assert torch.equal(Yn, standins.su3_wilson_apply_n(xn, Xn, kappa, L))


@pytest.mark.parametrize('which', ['cgnr', 'normal'])
@pytest.mark.parametrize('L', LATTICES)
def test_freeze_semantics(standins, L, which):
    kappa = wr.SOLVE_KAPPAS[1]
    lat, x, b, xn, bn = inputs(L)
    X, info = solve(lat, which, xn, bn, kappa, tol=1e-10)
    assert info['converged'].all()
    # a looser tolerance stops at an earlier check
    loose = solve(lat, which, xn, bn, kappa, tol=1e-6)[1]
    print(L, which, 'iters', info['iters'].tolist(), 'at 1e-6', loose['iters'].tolist())
    assert loose['converged'].all() and (loose['iters'] < info['iters']).all()
    assert (info['iters'] % 10 == 0).all() and (loose['iters'] % 10 == 0).all()
    # a system keeps its bits when others join the batch
    X1, i1 = solve(lat, which, xn[:1], bn[:1, :1].contiguous(), kappa, tol=1e-10)
    assert torch.equal(X1[0, 0], X[0, 0]) and torch.equal(i1['iters'][0, 0], info['iters'][0, 0])
    assert torch.equal(i1['residual'][0, 0], info['residual'][0, 0])
    # b = 0: a zero solution in zero iterations, and the others as before
    big = bn.clone()
    big[1, 1] = 0.0
    Xb, ib = solve(lat, which, xn, big, kappa, tol=1e-10)
    assert not Xb[1, 1].any() and ib['iters'][1, 1] == 0 and ib['residual'][1, 1] == 0.0 and ib['converged'].all()
    assert torch.equal(Xb[0], X[0])
    # never raises: too few iterations are reported
    few = solve(lat, which, xn, bn, kappa, tol=1e-10, max_iter=3)[1]
    assert not few['converged'].any() and (few['iters'] == 3).all()


@pytest.mark.parametrize('which', ['cgnr', 'normal'])
def test_launch_sequence_and_check_arithmetic(standins, which):
    """tol = 1e-30 cannot be met, so max_iter = 7 at check_every = 3 runs inner loops of 3, 3 and 1: 7 iterations, not
    9, iters = 7; 2 * 7 + 2 applies, 7 + 2 updates and 7 xpays, in the order the kernels' fused norms dictate"""
    L = LATTICES[1]
    lat, x, b, xn, bn = inputs(L)
    del standins.log[:]
    _, info = solve(lat, which, xn, bn, wr.SOLVE_KAPPAS[0], tol=1e-30, max_iter=7, check_every=3)
    assert not info['converged'].any() and (info['iters'] == 7).all()
    apply, applyh, update, xpay = ('apply', False, True), ('apply', True, True), ('update', None, None), ('xpay', None, None)
    if which == 'cgnr':
        want = [update, applyh] + 7 * [apply, update, applyh, xpay] + [apply, update]
    else:
        applyh = ('apply', True, False)
        want = [update] + 7 * [apply, applyh, update, xpay] + [apply, applyh, update]
    assert standins.log == want
    names = [e[0] for e in standins.log]
    assert (names.count('apply'), names.count('update'), names.count('xpay')) == (16, 9, 7)
    # a tolerance that is met: found at a check, that is at a multiple of 3 or at the last iteration
    _, info = solve(lat, which, xn, bn, wr.SOLVE_KAPPAS[0], tol=1e-2, max_iter=7, check_every=3)
    print(which, 'iters at tol 1e-2', info['iters'].tolist())
    assert ((info['iters'] % 3 == 0) | (info['iters'] == 7)).all() and (info['iters'] > 0).all()


def test_bad_arguments_name_the_public_method(standins):
    lat, x, b, xn, bn = inputs(LATTICES[1])
    for kw in (dict(tol=0.0), dict(tol=float('nan')), dict(max_iter=-1), dict(max_iter=True), dict(check_every=0),
               dict(check_every=2.5)):
        with pytest.raises(ValueError, match=r'LatticeSU3\.wilson_solve: need tol > 0'):
            lat.wilson_solve_n(xn, bn, 0.1, **kw)
        with pytest.raises(ValueError, match=r'LatticeSU3\.wilson_solve_normal: need tol > 0'):
            lat.wilson_solve_normal_n(xn, bn, 0.1, **kw)
    assert standins.log == []


# ------------------------------------------------------------------ the even-odd solvers through the same stand-ins
@functools.lru_cache(maxsize=None)
def dense_schur(L, kappa):
    """per chain of `inputs(L)`: (Mhat dense, its smallest and largest singular value)"""
    out = []
    for c in range(NB):
        m = we.dense_schur(wr.links(L, NB)[c:c + 1], kappa)
        s = np.linalg.svd(m, compute_uv=False)
        out.append((m, s[-1], s[0]))
    return out


@pytest.mark.parametrize('L', LATTICES)
def test_eo_cgnr_against_dense_solve(standins, L):
    """`wilson_solve_eo_n` solves the full system: the bound of `test_cgnr_against_dense_solve` against the full dense M,
    |psi - M^-1 b| <= 2 tol |b| / sigma_min(M)"""
    tol = 1e-10
    lat, x, b, xn, bn = inputs(L)
    for kappa in wr.SOLVE_KAPPAS:
        psin, info = lat.wilson_solve_eo_n(xn, bn, kappa, tol=tol, max_iter=200)
        assert info['converged'].all() and (info['residual'] <= 2 * tol).all(), (kappa, info)
        psi = wr.unpack_spinor(psin.numpy(), L)
        for c, (m, smin, _) in enumerate(dense(L, kappa)):
            for j in range(NRHS):
                want = np.linalg.solve(m, b[c, j].reshape(-1))
                err, bound = np.linalg.norm(psi[c, j].reshape(-1) - want), 2 * tol * np.linalg.norm(b[c, j]) / smin
                print(L, kappa, c, j, 'iters', int(info['iters'][c, j]), 'error', err, 'bound', bound)
                assert err <= bound, (kappa, c, j)


@pytest.mark.parametrize('L', LATTICES)
def test_schur_normal_cg_against_dense_solve(standins, L):
    """the bound of `test_normal_cg_against_dense_solve` on the Schur complement: |dX_e| <= cond(Mhat^H Mhat) * residual,
    cond < 100 (held here from the singular values of `we.dense_schur`), and info['action'] = |Y_e|^2 by the same sums"""
    lat, x, b, xn, bn = inputs(L)
    pe = ops.su3_spinor_split_eo(bn, L)[0]
    for kappa in wr.SOLVE_KAPPAS:
        assert all((smax / smin) ** 2 < 100 for _, smin, smax in dense_schur(L, kappa))
        # rows of Mhat: even site, then spin and colour; a native half field is [12, V/2]
        Xd = np.stack([np.linalg.solve(m.conj().T @ m, pe[c].numpy().transpose(2, 1, 0).reshape(-1, NRHS))
                       .reshape(-1, 12, NRHS).transpose(2, 1, 0) for c, (m, _, _) in enumerate(dense_schur(L, kappa))])
        for tol in (1e-6, 1e-10):
            Xn, Yn, info = lat.wilson_solve_schur_normal_n(xn, pe, kappa, tol=tol)
            assert info['converged'].all() and (info['residual'] <= 2 * tol).all(), (kappa, tol, info)
            err = np.abs(Xn.numpy() - Xd).max()
            print(L, kappa, tol, 'iters', info['iters'].tolist(), 'error', err, 'bound', 100 * tol * np.abs(Xd).max())
            assert err <= 100 * tol * np.abs(Xd).max()
            assert torch.equal(info['action'], ops.sum_parts(norm_part(Yn)))
            assert torch.equal(Yn, lat.wilson_schur_n(xn, Xn, kappa))


@pytest.mark.parametrize('which', ['eo', 'schur_normal'])
@pytest.mark.parametrize('L', LATTICES)
def test_eo_freeze_semantics(standins, L, which):
    kappa = wr.SOLVE_KAPPAS[1]
    lat, x, b, xn, bn = inputs(L)
    X, info = solve(lat, which, xn, bn, kappa, tol=1e-10)
    print(L, which, 'iters', info['iters'].tolist())
    assert info['converged'].all()
    # a system keeps its bits when others join the batch
    X1, i1 = solve(lat, which, xn[:1], bn[:1, :1].contiguous(), kappa, tol=1e-10)
    assert torch.equal(X1[0, 0], X[0, 0]) and torch.equal(i1['iters'][0, 0], info['iters'][0, 0])
    assert torch.equal(i1['residual'][0, 0], info['residual'][0, 0])
    # b = 0: a zero solution in zero iterations, and the others as before
    big = bn.clone()
    big[1, 1] = 0.0
    Xb, ib = solve(lat, which, xn, big, kappa, tol=1e-10)
    assert not Xb[1, 1].any() and ib['iters'][1, 1] == 0 and ib['residual'][1, 1] == 0.0 and ib['converged'].all()
    assert torch.equal(Xb[0], X[0])
    # never raises: too few iterations are reported
    few = solve(lat, which, xn, bn, kappa, tol=1e-10, max_iter=3)[1]
    assert not few['converged'].any() and (few['iters'] == 3).all()


@pytest.mark.parametrize('which', ['eo', 'schur_normal'])
def test_eo_launch_sequence(standins, which):
    """as `test_launch_sequence_and_check_arithmetic`: 7 iterations, iters = 7, and the whole list of calls.  Mhat is
    two hops, odd then even, the fused norm from the second.  `wilson_solve_eo_n` adds |b_e|^2 and |b_o|^2 (two updates),
    the source, the reconstruction and one full apply for its residual: 34 hops, 1 apply, 11 updates, 7 xpays."""
    L = LATTICES[1]
    lat, x, b, xn, bn = inputs(L)
    del standins.log[:]
    _, info = solve(lat, which, xn, bn, wr.SOLVE_KAPPAS[0], tol=1e-30, max_iter=7, check_every=3)
    assert not info['converged'].any() and (info['iters'] == 7).all()
    update, xpay = ('update', None, None), ('xpay', None, None)
    mhat = [('hop', 1, False, False), ('hop', 0, False, True)]
    if which == 'eo':
        mhath = [('hop', 1, True, False), ('hop', 0, True, True)]
        want = [update, update, ('hop', 0, False, False), update] + mhath + 7 * (mhat + [update] + mhath + [xpay]) \
            + mhat + [('hop', 1, False, False), ('apply', False, False), update]
        counts = (34, 1, 11, 7)
    else:
        mhath = [('hop', 1, True, False), ('hop', 0, True, False)]
        want = [update] + 7 * (mhat + mhath + [update, xpay]) + mhat + mhath + [update]
        counts = (32, 0, 9, 7)
    assert standins.log == want
    names = [e[0] for e in standins.log]
    assert tuple(names.count(n) for n in ('hop', 'apply', 'update', 'xpay')) == counts
