"""CPU tier of the clover-improved Wilson operator: the properties of the restatement tests/wilson_clover_restatement.py
that the GPU tests lean on (gamma5-Hermiticity, A Hermitian, block diagonal and equal to the sigma.(E +- B) block form,
gauge covariance, the Schur identity, c_sw = 0, the dense solve, positive-definite test inputs, the recorded yardsticks),
and the product's own host loop -- `LatticeSU3.wilson_clover_solve_n` and what it stands on -- run on CPU tensors with
the kernel entries of `l2hmc._ops` replaced by numpy stand-ins built on the restatement, the way
tests/test_wilson_cg_host.py does it: the dense solve, the launch sequence, the freezing, clover=, and what must raise."""
import numpy as np
import pytest
import torch

import wilson_clover_restatement as wc
import wilson_eo_restatement as we
import wilson_force_restatement as wf
import wilson_restatement as wr
from l2hmc import _ops as ops
from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
from test_wilson_cg_host import StandIns, norm_part

SMALL = [(2, 2, 2, 2), (4, 2, 6, 2)]
K = wc.KAPPA


# ------------------------------------------------------------------ the restatement
def test_inputs_are_positive_definite():
    """every input of a test of the inverse has 0.5 < eig(A) < 2 (so cond < 4: wc.PIVOT_BOUND); c_sw = 10 has not"""
    for L in wc.MEASURE_LATTICES + we.SOLVE_LATTICES:
        for kind in wc.INPUTS:
            for c_sw in wc.C_SWS:
                ev = np.linalg.eigvalsh(wc.clover(wc.INPUTS[kind](L, wc.NB), K * c_sw))
                print(L, kind, c_sw, f'{ev.min():.3f} {ev.max():.3f}')
                assert ev.min() > 0.5 and ev.max() < 2.0, (L, kind, c_sw)
    assert wc.min_eig(wc.clover(wr.links((4, 4, 4, 4), 2), K * wc.C_SW_BAD)) < 0


@pytest.mark.parametrize('L', SMALL)
def test_clover_term_structure(L):
    for kind in wc.INPUTS:
        x = wc.INPUTS[kind](L, 2)
        a = wc.clover(x, K * 1.769)
        assert np.abs(a - np.swapaxes(a.conj(), -1, -2)).max() <= 4 * 2.0 ** -53              # Hermitian
        assert np.abs(a[..., :6, 6:]).max() == 0 and np.abs(a[..., 6:, :6]).max() == 0        # block diagonal
        g5 = np.kron(wr.GAMMA[4], np.eye(3))
        assert np.abs(a @ g5 - g5 @ a).max() == 0                                             # commutes with gamma5
        up, dn = wc.block_form(x, K * 1.769)
        assert max(np.abs(a[..., :6, :6] - up).max(), np.abs(a[..., 6:, 6:] - dn).max()) <= wc.TOL_A
        assert np.abs(wc.unpack_blocks(wc.pack_blocks(a), L) - a).max() <= 4 * 2.0 ** -53       # the block layout round trip


@pytest.mark.parametrize('L', SMALL)
def test_gamma5_hermiticity_and_adjoint(L):
    x, psi = wr.links(L, 2), wr.spinors(L, 2, 4)
    g5 = wr.GAMMA[4].diagonal().real[:, None]
    for ap in (False, True):
        m = wc.wilson_clover(x, psi, K, 1.769, False, ap)
        md = wc.wilson_clover(x, psi, K, 1.769, True, ap)
        assert np.abs(md - g5 * wc.wilson_clover(x, g5 * psi, K, 1.769, False, ap)).max() <= wc.TOL_M
        phi, chi = psi[:, :2], psi[:, 2:]
        lhs, rhs = np.vdot(phi, m[:, 2:]), np.vdot(md[:, :2], chi)                          # <phi, M chi> = <M^H phi, chi>
        assert abs(lhs - rhs) <= wc.TOL_M * np.sqrt(wr.norm2(phi).sum() * chi.size)


def gauge_transform(x, g):
    """U'_mu(x) = g(x) U_mu(x) g(x + mu)^H"""
    return np.stack([g @ x[:, mu] @ np.swapaxes(np.roll(g, -1, axis=1 + mu).conj(), -1, -2) for mu in range(4)], 1)


@pytest.mark.parametrize('L', SMALL)
def test_gauge_covariance(L):
    """M_sw[U^g] (g psi) = g (M_sw[U] psi): each side is within TOL_M of its exact value, so they differ by 2 TOL_M"""
    x, psi, g = wr.links(L, 2), wr.spinors(L, 2, 2), wc.hot_links(L, 2)[:, 0]
    rot = lambda f: np.einsum('ntxyzij,nrtxyzaj->nrtxyzai', g, f)
    for c_sw in wc.C_SWS:
        d = wc.wilson_clover(gauge_transform(x, g), rot(psi), K, c_sw) - rot(wc.wilson_clover(x, psi, K, c_sw))
        assert np.abs(d).max() <= 2 * wc.TOL_M


@pytest.mark.parametrize('L', SMALL)
def test_schur_identity_and_csw_zero(L):
    """with b = M_sw psi: Mhat psi_e = bhat_e and the reconstruction returns psi (three kernel applications each way: 3
    TOL_HOP); c_sw = 0 is the plain Schur complement"""
    x, psi = wc.hot_links(L, 2), wr.spinors(L, 2, 2)
    for c_sw in wc.C_SWS:
        a = wc.clover(x, K * c_sw)
        ainv = wc.inverse(a)
        b = wc.wilson_clover(x, psi, K, c_sw, a=a)
        pe = psi * we.mask(L, 0)
        assert np.abs(wc.schur_clover(x, pe, K, a, ainv) - wc.prepare(x, b, K, ainv)).max() <= 3 * wc.TOL_HOP
        assert np.abs(wc.reconstruct(x, pe, b, K, ainv) - psi).max() <= 3 * wc.TOL_HOP
    one = wc.clover(x, 0.0)
    assert np.array_equal(one, np.broadcast_to(np.eye(12), one.shape))
    for dagger in (False, True):
        d = wc.schur_clover(x, psi, K, one, wc.inverse(one), dagger) - we.schur(x, psi, K, dagger)
        assert np.abs(d).max() <= we.TOL


def test_dense_solve():
    """|psi - M_sw^-1 b| <= 2 tol |b| / sigma_min(M_sw), the bound of test_wilson_host.py::test_cgnr_against_dense_solve"""
    L, tol = (2, 2, 2, 2), 1e-10
    x, b = wr.links(L, 2), wr.spinors(L, 2, 2)
    for c_sw in wc.C_SWS:
        psi, info = wc.solve_clover(x, b, 0.12, c_sw, tol=tol)
        assert info['converged'].all() and (info['residual'] <= 2 * tol).all()
        for c in range(2):
            m = wc.dense(x[c:c + 1], 0.12, c_sw)
            smin = np.linalg.svd(m, compute_uv=False)[-1]
            for j in range(2):
                err = np.linalg.norm(psi[c, j].reshape(-1) - np.linalg.solve(m, b[c, j].reshape(-1)))
                assert err <= 2 * tol * np.linalg.norm(b[c, j]) / smin, (c_sw, c, j)


def test_yardsticks_hold_on_the_small_lattices():
    for L, kind, c_sw in [((2, 2, 2, 2), 'smooth', 1.0), ((2, 2, 2, 2), 'hot', 1.769), ((4, 2, 6, 2), 'hot', 1.769)]:
        got = wc.measure_one(L, kind, c_sw)
        print(L, kind, c_sw, got)
        assert got['A'] <= wc.YARD_A and got['HOP'] <= wc.YARD_HOP and got['M'] <= wc.YARD_M and got['INV'] <= wc.YARD_INV


# ------------------------------------------------------------------ the product's host loop on stand-ins
def ldl_pivots(a):
    """the pivots of the unpivoted L D L^H of both blocks, any sign: ratios of leading minors, [..., 12]"""
    out = []
    for s in (0, 6):
        minors = [np.ones(a.shape[:-2])] + [np.linalg.det(a[..., s:s + n, s:s + n]).real for n in range(1, 7)]
        out += [minors[n + 1] / minors[n] for n in range(6)]
    return np.stack(out, -1)


class CloverStandIns(StandIns):
    """the stand-ins of test_wilson_cg_host.py and those of the four entries of csrc/su3_wilson_clover.hip; a clover hop
    is logged as ('chop', parity, cmode, dagger, norm requested)"""
    NAMES = StandIns.NAMES + ('su3_clover_term_n', 'su3_clover_invert_n', 'su3_wilson_clover_hop_eo_n', 'su3_clover_apply_n')

    def su3_clover_term_n(self, xn, coef, lat, out=None):
        self.log.append(('term', None, None))
        return torch.from_numpy(wc.pack_blocks(wc.clover(wf.unpack_links(xn.numpy(), lat), coef)))

    def su3_clover_invert_n(self, cl, lat, out=None, logdet=True):
        self.log.append(('invert', None, None))
        a = wc.unpack_blocks(cl.numpy(), lat)
        piv = ldl_pivots(a).reshape(a.shape[0], -1, 12)
        with np.errstate(invalid='ignore'):
            lg = np.log(piv)
        sites = [we.sites(lat, p) for p in (0, 1)]
        mp = np.stack([piv[:, s].min((1, 2)) for s in sites], 1)[..., None]
        ld = np.stack([lg[:, s].sum((1, 2)) for s in sites], 1)[..., None]
        return torch.from_numpy(wc.pack_blocks(np.linalg.inv(a))), torch.from_numpy(mp), torch.from_numpy(ld)

    def su3_wilson_clover_hop_eo_n(self, xn, src, lat, parity, c, cmode, dagger=False, antiperiodic_t=True, a=1.0,
                                   aux=None, b=0.0, out=None, norm=False):
        want_norm = isinstance(norm, torch.Tensor) or bool(norm)
        self.log.append(('chop', int(parity), int(cmode), bool(dagger), want_norm))
        assert (c is None) == (cmode == 0)
        res = wc.hop_clover(wf.unpack_links(xn.numpy(), lat), we.unpack_half(src.numpy(), lat, 1 - parity), parity,
                            None if c is None else wc.unpack_blocks(c.numpy(), lat), cmode, dagger, antiperiodic_t, a,
                            None if aux is None else we.unpack_half(aux.numpy(), lat, parity), b)
        out = torch.empty_like(src) if out is None else out
        out.copy_(torch.from_numpy(we.pack_half(res, parity)))
        if not want_norm:
            return out
        part = norm if isinstance(norm, torch.Tensor) else torch.empty((*src.shape[:2], 1), dtype=torch.float64)
        return out, part.copy_(norm_part(out))

    def su3_clover_apply_n(self, c, src, lat, parity, out=None, norm=False):
        self.log.append(('capply', int(parity), None))
        res = wc.apply_site(wc.unpack_blocks(c.numpy(), lat), we.unpack_half(src.numpy(), lat, parity))
        return torch.from_numpy(we.pack_half(res, parity))


@pytest.fixture
def standins(monkeypatch):
    return CloverStandIns(monkeypatch)


def inputs(L, nb=2, nrhs=2):
    x, b = wr.links(L, nb), wr.spinors(L, nb, nrhs)
    return LatticeSU3(nb, list(L)), x, b, torch.from_numpy(wf.pack_links(x)), torch.from_numpy(wr.pack_spinor(b))


@pytest.mark.parametrize('L', SMALL)
def test_host_loop_against_restatement_and_dense(standins, L):
    tol = 1e-10
    lat, x, b, xn, bn = inputs(L)
    for c_sw in wc.C_SWS:
        standins.log.clear()
        psin, info = lat.wilson_clover_solve_n(xn, bn, 0.12, c_sw, tol=tol, max_iter=200)
        assert set(info) == {'iters', 'converged', 'residual'}
        assert info['converged'].all() and (info['residual'] <= 2 * tol).all(), info
        want, winfo = wc.solve_clover(x, b, 0.12, c_sw, tol=tol, max_iter=200)
        assert np.array_equal(info['iters'].numpy(), winfo['iters'])
        psi = wr.unpack_spinor(psin.numpy(), L)
        for c in range(2 if L == (2, 2, 2, 2) else 0):                   # the dense solve on the smallest lattice
            m = wc.dense(x[c:c + 1], 0.12, c_sw)
            smin = np.linalg.svd(m, compute_uv=False)[-1]
            for j in range(2):
                err = np.linalg.norm(psi[c, j].reshape(-1) - np.linalg.solve(m, b[c, j].reshape(-1)))
                assert err <= 2 * tol * np.linalg.norm(b[c, j]) / smin
        # the launch sequence: A and A^-1 once; the source from kernels 4 and 3; per operator application two clover
        # hops, odd (cmode 2, no norm) then even (cmode 1, fused norm); reconstruction; the full residual from two hops
        log = standins.log
        assert log[:2] == [('term', None, None), ('invert', None, None)]
        assert [e for e in log if e[0] in ('term', 'invert')] == log[:2]
        ch = [e for e in log if e[0] in ('chop', 'capply')]
        assert ch[:2] == [('capply', 1, None), ('chop', 0, 0, False, False)]
        assert ch[-3:] == [('chop', 1, 2, False, False), ('chop', 0, 1, False, False), ('chop', 1, 1, False, False)]
        body = ch[2:-3]
        assert len(body) % 2 == 0 and all(o[:3] == ('chop', 1, 2) and not o[4] and e[:3] == ('chop', 0, 1) and e[4]
                                          and o[3] == e[3] for o, e in zip(body[::2], body[1::2]))
        assert not any(e[0] in ('hop', 'apply') for e in log)


def test_host_loop_freezes_and_takes_a_prebuilt_term(standins):
    L = (2, 2, 2, 2)
    lat, x, b, xn, bn = inputs(L, nrhs=3)
    bn[:, 1] = 0                                                   # b = 0: psi = 0, converged at once
    psin, info = lat.wilson_clover_solve_n(xn, bn, 0.12, 1.0, check_every=3)
    assert (psin[:, 1] == 0).all() and (info['iters'][:, 1] == 0).all() and (info['residual'][:, 1] == 0).all()
    alone, ainfo = lat.wilson_clover_solve_n(xn, bn[:, 2].contiguous(), 0.12, 1.0, check_every=3)
    assert torch.equal(alone, psin[:, 2]) and torch.equal(ainfo['iters'][:, 0], info['iters'][:, 2])
    cl = lat.clover_term_n(xn, 0.12, 1.0)
    assert tuple(cl.a.shape) == tuple(cl.ainv.shape) == (2, 2, 2, 36, 8) and tuple(cl.min_pivot.shape) == (2,)
    assert tuple(cl.logdet.shape) == (2, 2) and (cl.kappa, cl.c_sw) == (0.12, 1.0)
    assert np.allclose(cl.logdet.numpy(), wc.logdet(wc.clover(x, 0.12)), rtol=0, atol=1e-12)
    standins.log.clear()
    again, _ = lat.wilson_clover_solve_n(xn, bn, 0.12, 1.0, check_every=3, clover=cl)
    assert torch.equal(again, psin) and not any(e[0] in ('term', 'invert') for e in standins.log)
    never, ninfo = lat.wilson_clover_solve_n(xn, bn, 0.12, 1.0, max_iter=2, clover=cl)        # never raises
    assert not ninfo['converged'][:, 0].any() and (ninfo['iters'][:, 0] == 2).all()
    # c_sw = 0 is the plain even-odd solve
    p0, i0 = lat.wilson_clover_solve_n(xn, bn, 0.12, 0.0)
    p1, i1 = lat.wilson_solve_eo_n(xn, bn, 0.12)
    assert torch.equal(i0['iters'], i1['iters']) and (p0 - p1).abs().max() <= 1e-10 * p1.abs().max()
    # the operator, the Schur complement and the propagator (native layout: the reference layout needs the pack kernels)
    psi = wr.spinors(L, 2, 2)
    pn = torch.from_numpy(wr.pack_spinor(psi))
    got = lat.wilson_clover_dirac_n(xn, pn, K, 1.769, dagger=True)
    assert np.abs(wr.unpack_spinor(got.numpy(), L) - wc.wilson_clover(x, psi, K, 1.769, True)).max() <= wc.TOL_M
    a = wc.clover(x, K * 1.769)
    got = lat.wilson_clover_schur_n(xn, ops.su3_spinor_split_eo(pn, L)[0], K, 1.769)
    want = wc.schur_clover(x, psi, K, a, wc.inverse(a))
    assert np.abs(got.numpy() - we.pack_half(want, 0)).max() <= 2 * wc.TOL_HOP
    S, sinfo = lat.quark_propagator_n(xn, 0.12, source=(1, 0, 1, 0), c_sw=1.0)
    assert tuple(S.shape) == (2, 12, 12, 16) and sinfo['converged'].all()
    want, _ = wc.solve_clover(x, wr.point_sources(2, L, (1, 0, 1, 0)), 0.12, 1.0)
    assert np.abs(S.numpy() - wr.pack_spinor(want)).max() <= 1e-9


def test_what_must_raise(standins):
    L = (4, 4, 4, 4)
    lat, x, b, xn, bn = inputs(L, nrhs=1)
    half = ops.su3_spinor_split_eo(bn, L)[0]
    with pytest.raises(ValueError, match=r'chain 0.*pivot -?[0-9.]+'):
        lat.wilson_clover_solve_n(xn, bn, K, wc.C_SW_BAD)
    with pytest.raises(ValueError, match='positive definite'):
        lat.wilson_clover_schur_n(xn, half, K, wc.C_SW_BAD)
    with pytest.raises(ValueError, match='positive definite'):
        lat.quark_propagator_n(xn, K, c_sw=wc.C_SW_BAD)
    bad = lat.clover_term_n(xn, K, wc.C_SW_BAD)                                  # building it does not raise
    assert (bad.min_pivot <= 0).all()
    lat.wilson_clover_dirac_n(xn, bn, K, wc.C_SW_BAD, clover=bad)                # ... nor does M_sw itself
    standins.log.clear()
    for call in (lambda: lat.wilson_clover_solve_n(xn, bn, float('nan'), 1.0),
                 lambda: lat.wilson_clover_solve_n(xn, bn, K, float('inf')),
                 lambda: lat.wilson_clover_solve_n(xn, bn, K, None),
                 lambda: lat.clover_term_n(xn, K, float('nan')),
                 lambda: lat.wilson_clover_dirac_n(xn, bn, None, 1.0),
                 lambda: lat.wilson_clover_schur_n(xn, half, K, float('-inf')),
                 lambda: lat.quark_propagator_n(xn, K, c_sw=float('nan')),
                 lambda: lat.quark_propagator_n(xn, K, c_sw=1.0, even_odd=False),
                 lambda: lat.quark_propagator_n(xn, K, c_sw=1.0, even_odd=True, mixed=True),
                 lambda: lat.quark_propagator_n(xn, K, c_sw=1.0, inner_tol=1e-3),
                 lambda: lat.quark_propagator_n(xn, K, clover=bad),
                 lambda: lat.wilson_clover_solve_n(xn, bn, K, 1.0, tol=0.0),
                 lambda: lat.wilson_clover_solve_n(xn, bn, K, 1.0, clover=bad),          # another c_sw
                 lambda: lat.wilson_clover_solve_n(xn[:1], bn[:1], K, wc.C_SW_BAD, clover=bad),   # another batch
                 lambda: lat.wilson_clover_solve_n(xn, bn, K, 1.0, clover=(bad.a, bad.ainv)),
                 lambda: lat.wilson_clover_schur_n(xn, bn, K, 1.0)):                     # a full field for a half one
        with pytest.raises(ValueError):
            call()
    gx, gb = xn.clone().requires_grad_(True), bn.clone().requires_grad_(True)
    for call in (lambda: lat.wilson_clover_solve_n(gx, bn, K, 1.0), lambda: lat.wilson_clover_solve_n(xn, gb, K, 1.0),
                 lambda: lat.clover_term_n(gx, K, 1.0), lambda: lat.wilson_clover_dirac_n(xn, gb, K, 1.0),
                 lambda: lat.wilson_clover_schur_n(gx, half, K, 1.0), lambda: lat.quark_propagator_n(gx, K, c_sw=1.0)):
        with pytest.raises(RuntimeError, match='autograd'):
            call()
    assert not any(e[0] in ('chop', 'capply', 'hop', 'apply', 'update') for e in standins.log)    # before any solve
    odd = LatticeSU3(2, [3, 4, 5, 2])
    on = torch.zeros(2, 4, 9, 120, dtype=torch.complex128)
    fn = torch.zeros(2, 1, 12, 120, dtype=torch.complex128)
    for call in (lambda: odd.clover_term_n(on, K, 1.0), lambda: odd.wilson_clover_dirac_n(on, fn, K, 1.0),
                 lambda: odd.wilson_clover_solve_n(on, fn, K, 1.0), lambda: odd.quark_propagator_n(on, K, c_sw=1.0),
                 lambda: odd.wilson_clover_schur_n(on, fn[..., :60], K, 1.0)):
        with pytest.raises(ValueError, match=r'even extents.*\[3, 4, 5, 2\]'):
            call()
