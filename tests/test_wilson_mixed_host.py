"""CPU tier of the mixed-precision even-odd solves.  First the numpy restatement tests/wilson_mixed_restatement.py, whose
defect-correction solves are held against dense solves.  Then the product's own loop (`_MixedSolve` and the `_CG` it
runs on complex64 fields, l2hmc/lattice/su3/pytorch/wilson.py) on CPU tensors, the kernel entries of `l2hmc._ops`
replaced by numpy stand-ins: those of tests/test_wilson_cg_host.py for the fp64 entries, and stand-ins built on the
restatement for the six fp32 entries.  Held: the dense solve, the freeze semantics, b = 0, the three caps (never
raising), the per-system inner target, and the launch sequence."""
import numpy as np
import pytest
import torch

import wilson_eo_restatement as we
import wilson_force_restatement as wf
import wilson_mixed_restatement as wm
import wilson_restatement as wr
from l2hmc import _ops as ops
from l2hmc.lattice.su3.pytorch import wilson
from test_wilson_cg_host import NB, NRHS, StandIns, dense, dense_schur, inputs, norm_part

LATTICES = [(2, 2, 2, 2), (4, 2, 2, 2)]
C64 = np.complex64


class MixedStandIns(StandIns):
    """the fp64 stand-ins and, on complex64 CPU tensors, the six fp32 entries; a fp32 hop is logged as ('hop32', parity,
    dagger, norm requested), the others by their name"""
    NAMES = StandIns.NAMES + ('su3_links_demote_eo_n', 'su3_wilson_hop_eo_f32_n', 'su3_spinor_cg_update_f32_',
                              'su3_spinor_xpay_f32_', 'su3_spinor_demote', 'su3_spinor_promote_axpy_')

    def su3_links_demote_eo_n(self, xn, lat, out=None):
        self.log.append(('links', None, None))
        return torch.from_numpy(wm.links_eo_f32(wf.unpack_links(xn.numpy(), lat)))

    def su3_wilson_hop_eo_f32_n(self, x32, src, lat, parity, dagger=False, antiperiodic_t=True, a=1.0, aux=None, b=0.0,
                                out=None, norm=False):
        want_norm = isinstance(norm, torch.Tensor) or bool(norm)
        self.log.append(('hop32', int(parity), bool(dagger), want_norm))
        assert x32.dtype == src.dtype == torch.complex64
        full = np.zeros((x32.shape[0], 4, 9, 2 * x32.shape[-1]), C64)
        for p in (0, 1):
            full[..., we.sites(lat, p)] = x32[:, p].numpy()
        res = we.hop_eo(wf.unpack_links(full, lat), we.unpack_half(src.numpy(), lat, 1 - parity), parity, dagger,
                        antiperiodic_t, np.float32(a), None if aux is None else we.unpack_half(aux.numpy(), lat, parity),
                        np.float32(b))
        assert res.dtype == C64
        out = torch.empty_like(src) if out is None else out
        out.copy_(torch.from_numpy(we.pack_half(res, parity)))
        if not want_norm:
            return out
        part = norm if isinstance(norm, torch.Tensor) else torch.empty((*src.shape[:2], 1), dtype=torch.float64)
        return out, part.copy_(norm_part(out.to(torch.complex128)))

    def su3_spinor_cg_update_f32_(self, x, r, p, q, alpha, part=None):
        self.log.append(('update32', None, None))
        assert x.dtype == torch.complex64 and alpha.dtype == torch.float64
        a = alpha.to(torch.float32).reshape(*x.shape[:2], 1, 1)
        x.add_(a * p)
        r.sub_(a * q)
        part = torch.empty((*x.shape[:2], 1), dtype=torch.float64) if part is None else part
        return part.copy_(norm_part(r.to(torch.complex128)))

    def su3_spinor_xpay_f32_(self, p, z, beta):
        self.log.append(('xpay32', None, None))
        assert p.dtype == torch.complex64 and beta.dtype == torch.float64
        return p.mul_(beta.to(torch.float32).reshape(*p.shape[:2], 1, 1)).add_(z)

    def su3_spinor_demote(self, f64, scale, out=None):
        self.log.append(('demote', None, None))
        res = (f64 * scale.reshape(*f64.shape[:2], 1, 1)).to(torch.complex64)
        return res if out is None else out.copy_(res)

    def su3_spinor_promote_axpy_(self, x64, e32, scale):
        self.log.append(('promote', None, None))
        sc = scale.reshape(*x64.shape[:2], 1, 1)
        x64.copy_(torch.where(sc != 0, x64 + sc * e32.to(torch.complex128), x64))
        return x64


@pytest.fixture
def standins(monkeypatch):
    return MixedStandIns(monkeypatch)


# ------------------------------------------------------------------ the restatement against dense solves
@pytest.mark.parametrize('L', LATTICES)
def test_restatement_against_dense_solves(L):
    """the bounds of test_wilson_cg_host.py: |psi - M^-1 b| <= 2 tol |b| / sigma_min(M) for the solve of the full system,
    |dX_e| <= cond(Mhat^H Mhat) * residual with cond < 100 for the normal form; at 1e-12 no single fp32 cycle can do"""
    x, b = wr.links(L, NB), wr.spinors(L, NB, NRHS)
    for kappa in wr.SOLVE_KAPPAS:
        for tol in (1e-10, 1e-12):
            psi, info = wm.solve_eo_mixed(x, b, kappa, tol=tol)
            assert info['converged'].all() and (info['residual'] <= tol).all(), (kappa, tol, info)
            assert tol > 1e-11 or (info['outer'] >= 2).all()
            for c, (m, smin, _) in enumerate(dense(L, kappa)):
                for j in range(NRHS):
                    want = np.linalg.solve(m, b[c, j].reshape(-1))
                    err, bound = np.linalg.norm(psi[c, j].reshape(-1) - want), 2 * tol * np.linalg.norm(b[c, j]) / smin
                    print(L, kappa, tol, c, j, 'iters', int(info['iters'][c, j]), 'outer', int(info['outer'][c, j]),
                          'error', err, 'bound', bound)
                    assert err <= bound
        phi = b * we.mask(L, 0)
        assert all((smax / smin) ** 2 < 100 for _, smin, smax in dense_schur(L, kappa))
        Xd = we.dense_normal_eo(x, phi, kappa)[0]
        for tol in (1e-6, 1e-10):
            X, Y, info = wm.normal_eo_mixed(x, phi, kappa, tol=tol)
            assert info['converged'].all() and (info['residual'] <= tol).all()
            err = np.abs(X - Xd).max()
            print(L, kappa, tol, 'normal: iters', info['iters'].tolist(), 'outer', info['outer'].tolist(), 'error', err)
            assert err <= 100 * tol * np.abs(Xd).max()
            assert np.array_equal(info['action'], wr.norm2(Y))


# ------------------------------------------------------------------ the product's loop through the stand-ins
def solve(lat, which, xn, bn, kappa, **kw):
    """(solution, info) of one of the two mixed solvers; 'normal' takes the even half of bn for its right-hand side"""
    if which == 'eo':
        return lat.wilson_solve_eo_mixed_n(xn, bn, kappa, **kw)
    X, _, info = lat.wilson_solve_schur_normal_mixed_n(xn, ops.su3_spinor_split_eo(bn, lat._lattice_shape)[0], kappa, **kw)
    return X, info


KEYS = ('iters', 'outer', 'converged', 'residual')


@pytest.mark.parametrize('L', LATTICES)
def test_product_loop_against_dense_solves(standins, L):
    lat, x, b, xn, bn = inputs(L)
    for kappa in wr.SOLVE_KAPPAS:
        for tol in (1e-10, 1e-12):
            psin, info = lat.wilson_solve_eo_mixed_n(xn, bn, kappa, tol=tol)
            assert sorted(info) == sorted(KEYS) and all(info[k].shape == (NB, NRHS) for k in KEYS)
            assert info['converged'].all() and (info['residual'] <= tol).all(), (kappa, tol, info)
            assert tol > 1e-11 or (info['outer'] >= 2).all()
            psi = wr.unpack_spinor(psin.numpy(), L)
            for c, (m, smin, _) in enumerate(dense(L, kappa)):
                for j in range(NRHS):
                    want = np.linalg.solve(m, b[c, j].reshape(-1))
                    err, bound = np.linalg.norm(psi[c, j].reshape(-1) - want), 2 * tol * np.linalg.norm(b[c, j]) / smin
                    assert err <= bound, (kappa, tol, c, j, err, bound)
        pe = ops.su3_spinor_split_eo(bn, L)[0]
        Xd = we.pack_half(we.dense_normal_eo(x, b * we.mask(L, 0), kappa)[0], 0)
        for tol in (1e-6, 1e-10):
            Xn, Yn, info = lat.wilson_solve_schur_normal_mixed_n(xn, pe, kappa, tol=tol)
            assert sorted(info) == sorted(KEYS + ('action',))
            assert info['converged'].all() and (info['residual'] <= tol).all(), (kappa, tol, info)
            assert np.abs(Xn.numpy() - Xd).max() <= 100 * tol * np.abs(Xd).max()
            assert torch.equal(info['action'], ops.sum_parts(norm_part(Yn)))
            assert torch.equal(Yn, lat.wilson_schur_n(xn, Xn, kappa))


@pytest.mark.parametrize('which', ['eo', 'normal'])
@pytest.mark.parametrize('L', LATTICES)
def test_freezing_zero_rhs_and_caps(standins, L, which):
    kappa = wr.SOLVE_KAPPAS[1]
    lat, x, b, xn, bn = inputs(L)
    X, info = solve(lat, which, xn, bn, kappa, tol=1e-12)
    print(L, which, {k: info[k].tolist() for k in KEYS})
    assert info['converged'].all() and (info['outer'] >= 2).all() and (info['iters'] % 10 == 0).all()
    # a system keeps its bits, and every entry of its info, when others join the batch
    X1, i1 = solve(lat, which, xn[:1], bn[:1, :1].contiguous(), kappa, tol=1e-12)
    assert torch.equal(X1[0, 0], X[0, 0])
    assert all(torch.equal(i1[k][0, 0], info[k][0, 0]) for k in info)
    # b = 0: a zero solution in no cycle, and the others as before
    big = bn.clone()
    big[1, 1] = 0.0
    Xb, ib = solve(lat, which, xn, big, kappa, tol=1e-12)
    assert not Xb[1, 1].any() and ib['iters'][1, 1] == 0 and ib['outer'][1, 1] == 0 and ib['residual'][1, 1] == 0.0
    assert ib['converged'].all() and torch.equal(Xb[0], X[0])
    # the three caps: reported, never raised
    few = solve(lat, which, xn, bn, kappa, tol=1e-12, max_iter=3)[1]
    assert not few['converged'].any() and (few['iters'] == 3).all() and (few['outer'] == 1).all()
    few = solve(lat, which, xn, bn, kappa, tol=1e-12, max_outer=1)[1]
    assert not few['converged'].any() and (few['outer'] == 1).all() and (few['residual'] > 1e-12).all()
    few = solve(lat, which, xn, bn, kappa, tol=1e-12, max_inner=5, max_outer=2)[1]
    assert not few['converged'].any() and (few['iters'] == 10).all() and (few['outer'] == 2).all()
    # (no cycle: the Schur solution stays zero; the full solution is then its reconstruction psi_o = b_o alone)
    def even(X):
        return ops.su3_spinor_split_eo(X, L)[0] if which == 'eo' else X
    X0, none = solve(lat, which, xn, bn, kappa, tol=1e-12, max_outer=0)
    assert not even(X0).any() and not none['converged'].any() and (none['iters'] == 0).all() and (none['residual'] > 0.1).all()
    X0, none = solve(lat, which, xn, bn, kappa, tol=1e-12, max_iter=0)
    assert not even(X0).any() and not none['converged'].any() and (none['outer'] == 0).all()


def test_per_system_inner_target(standins, monkeypatch):
    """the inner `_CG` gets tol = inner_tol and bb = (target / inner_tol)^2 per system, target = max(inner_tol,
    MIXED_SAFETY tol sqrt(bb) / |r|), and bb = 0 for a system that is not live"""
    L = LATTICES[1]
    lat, x, b, xn, bn = inputs(L)
    seen = []

    class Spy(wilson._CG):
        def __init__(self, what, b_, single, op, tol, max_iter, check_every, bb=None):
            if b_.dtype == torch.complex64:
                seen.append((float(tol), int(max_iter), bb.clone()))
            super().__init__(what, b_, single, op, tol, max_iter, check_every, bb=bb)
    monkeypatch.setattr(wilson, '_CG', Spy)
    big = bn.clone()
    big[1, 0] = 0.0
    kappa, tol, inner_tol = wr.SOLVE_KAPPAS[1], 1e-2, 1e-6
    _, info = lat.wilson_solve_eo_mixed_n(xn, big, kappa, tol=tol, inner_tol=inner_tol, max_inner=77)
    assert info['converged'].all() and (info['outer'][big.abs().sum((2, 3)) > 0] == 1).all() and info['outer'][1, 0] == 0
    assert len(seen) == 1 and seen[0][0] == inner_tol and seen[0][1] == 77
    bz = b.copy()
    bz[1, 0] = 0.0
    bhat = we.hop_eo(x, bz * we.mask(L, 1), 0, False, True, a=kappa, aux=bz * we.mask(L, 0), b=1.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        target = np.maximum(wilson.MIXED_SAFETY * tol * np.sqrt(wr.norm2(bz) / wr.norm2(bhat)), inner_tol)
    want = np.where(wr.norm2(bz) > 0, (target / inner_tol) ** 2, 0.0)
    assert (want[wr.norm2(bz) > 0] > 1e6).all() and want[1, 0] == 0.0            # relaxed far above inner_tol
    np.testing.assert_allclose(seen[0][2].numpy(), want, rtol=1e-12)
    # a tight outer tolerance leaves the first cycle at inner_tol itself: bb = 1 for the live systems
    del seen[:]
    lat.wilson_solve_eo_mixed_n(xn, big, kappa, tol=1e-12, inner_tol=1e-4)
    assert len(seen) >= 2 and torch.equal(seen[0][2], torch.from_numpy((wr.norm2(bz) > 0).astype(np.float64)))
    assert (seen[-1][2] >= 1.0).logical_or(seen[-1][2] == 0.0).all()


@pytest.mark.parametrize('which', ['eo', 'normal'])
def test_launch_sequence(standins, which):
    """tol = 1e-30 cannot be met: max_outer = 2 cycles of max_inner = 3 iterations.  Per cycle: demote, the inner `_CG` on
    the fp32 entries (its |b|^2 by one update, then the loop body of the fp64 solver: two fp32 hops per Mhat, the fused
    norm from the second), promote, the true residual by the fp64 hops and one fp64 update."""
    L = LATTICES[0]
    lat, x, b, xn, bn = inputs(L)
    del standins.log[:]
    _, info = solve(lat, which, xn, bn, wr.SOLVE_KAPPAS[0], tol=1e-30, max_inner=3, max_outer=2)
    assert not info['converged'].any() and (info['iters'] == 6).all() and (info['outer'] == 2).all()
    update, links = ('update', None, None), ('links', None, None)
    u32, x32, dem, pro = ('update32', None, None), ('xpay32', None, None), ('demote', None, None), ('promote', None, None)
    mhat = [('hop', 1, False, False), ('hop', 0, False, False)]
    mhath = [('hop', 1, True, False), ('hop', 0, True, False)]
    m32 = [('hop32', 1, False, False), ('hop32', 0, False, True)]
    if which == 'eo':
        m32h = [('hop32', 1, True, False), ('hop32', 0, True, True)]
        cycle = [dem, u32] + m32h + 3 * (m32 + [u32] + m32h + [x32]) + [pro] + mhat + [update]
        want = [update, update, ('hop', 0, False, False), links, update] + 2 * cycle + [('hop', 1, False, False)]
    else:
        m32h = [('hop32', 1, True, False), ('hop32', 0, True, False)]
        cycle = [dem, u32] + 3 * (m32 + m32h + [u32, x32]) + [pro] + mhat + mhath + [update]
        want = [links, update] + 2 * cycle + [('hop', 1, False, False), ('hop', 0, False, True)]
    assert standins.log == want


def test_mixed_keywords_reach_the_mixed_solver(standins):
    """`pseudofermion_action_n` / `_force_fields_n` / `quark_propagator_n` with mixed=True run the mixed solvers: fp32
    hops appear in the log, and the results agree with the fp64 path to the solver tolerance"""
    L = LATTICES[0]
    lat, x, b, xn, bn = inputs(L)
    pe = ops.su3_spinor_split_eo(bn, L)[0]
    kappa = wr.SOLVE_KAPPAS[1]
    s64, _ = lat.pseudofermion_action_n(xn, pe, kappa, even_odd=True, tol=1e-12)
    assert not any(e[0] == 'hop32' for e in standins.log)
    s32, info = lat.pseudofermion_action_n(xn, pe, kappa, even_odd=True, mixed=True, tol=1e-12, inner_tol=1e-3)
    assert any(e[0] == 'hop32' for e in standins.log) and 'outer' in info
    assert (torch.abs(s32 - s64) <= 32 * wm.CG_S0 * s64 + 1e-12 * s64).all()
    X64, Y64, _ = lat._force_fields_n('pseudofermion_force', xn, pe, kappa, True, tol=1e-10)
    X32, Y32, info = lat._force_fields_n('pseudofermion_force', xn, pe, kappa, True, tol=1e-10, mixed=True, max_inner=100)
    assert 'outer' in info and (X32 - X64).abs().max() <= 100 * 2e-10 * X64.abs().max()
    del standins.log[:]
    S, info = lat.quark_propagator_n(xn, kappa, even_odd=True, mixed=True, tol=1e-10)
    assert any(e[0] == 'hop32' for e in standins.log) and info['converged'].all() and S.shape == (NB, 12, 12, 16)
