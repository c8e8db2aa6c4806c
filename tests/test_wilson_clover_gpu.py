"""GPU tests of the clover-improved Wilson operator: the four kernels of csrc/su3_wilson_clover.hip against the numpy
restatement tests/wilson_clover_restatement.py, and the public interface on top (`clover_term`, `wilson_clover_dirac`,
`wilson_clover_schur`, `wilson_clover_solve`, `quark_propagator(c_sw=...)`).

Tolerances (derivations and the measured yardsticks: tests/wilson_clover_restatement.py): wc.TOL_A for the entries of A,
wc.TOL_HOP for one application of the hop kernel, wc.TOL_M for M_sw psi and the site-local apply on exact blocks,
wc.TOL_INV for max |A A^-1 - 1|, wc.PIVOT_BOUND and wc.logdet_tol for the pivots, wr.norm_bound for norm partials.
Where the operator runs on the blocks that the clover kernel made, those are within TOL_A of exact and enter a sum of 12
terms times |psi|: TOL_DIRAC = TOL_M + 12 max|psi| TOL_A.  Two solves that both stop at a recomputed residual of at most 2
tol |b| (asserted) satisfy |M_sw (psi_1 - psi_2)| <= 4 tol |b|, which needs no singular value."""
import functools

import numpy as np
import pytest
import torch

import gaugefix_restatement as gf
import wilson_clover_restatement as wc
import wilson_eo_restatement as we
import wilson_restatement as wr
from wilson_gpu_util import dev, host

gpu = pytest.mark.gpu
NB, NRHS = wc.NB, wc.NRHS
K = wc.KAPPA
TOL_SOLVE = 1e-10
CASES = [(kind, c_sw) for kind in wc.INPUTS for c_sw in wc.C_SWS]


@functools.lru_cache(maxsize=None)
def reference(L, kind, c_sw):
    """(x, a, ainv) of the restatement"""
    return wc.fields(kind, L, c_sw, NB)


def tol_dirac(psi):
    return wc.TOL_M + 12 * float(np.abs(psi).max()) * wc.TOL_A


@gpu
@pytest.mark.parametrize('kind,c_sw', CASES)
@pytest.mark.parametrize('L', we.EO_GPU_LATTICES)
def test_clover_term_and_inverse(L, kind, c_sw):
    from l2hmc import _ops as ops
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    V = int(np.prod(L))
    Vh, parts = V // 2, -(-(V // 2) // 256)
    x, a, _ = reference(L, kind, c_sw)
    xn = ops.su3_pack(dev(x))
    keep = xn.clone()
    cl = ops.su3_clover_term_n(xn, K * c_sw, L)
    assert cl.shape == (NB, 2, 2, 36, Vh) and cl.dtype == torch.float64 and torch.equal(xn, keep)
    d = float(np.abs(host(cl) - wc.pack_blocks(a)).max())
    assert d <= wc.TOL_A, d
    keepc = cl.clone()
    inv, mp, ld = ops.su3_clover_invert_n(cl, L)
    assert inv.shape == cl.shape and mp.shape == ld.shape == (NB, 2, parts) and torch.equal(cl, keepc)
    inv2, mp2, none = ops.su3_clover_invert_n(cl, L, logdet=False)
    assert none is None and torch.equal(inv2, inv) and torch.equal(mp2, mp)
    ak = wc.unpack_blocks(host(cl), L)                                   # the kernel's own A: the input of its inverse
    dinv = wc.inv_defect(ak, wc.unpack_blocks(host(inv), L))
    print(f'{L} {kind} {c_sw}: A {d / wc.TOL_A:.3g} of its tolerance, |A Ainv - 1| {dinv:.3g} (np.linalg.inv '
          f'{wc.inv_defect(ak, np.linalg.inv(ak)):.3g})')
    assert dinv <= wc.TOL_INV, dinv
    piv = wc.pivots(ak)
    lp, sld = np.log(piv).reshape(NB, V, 12), wc.logdet(ak)
    for p in (0, 1):
        want = wc.half_min(piv, p)
        assert (np.abs(host(mp)[:, p].min(-1) - want) <= wc.PIVOT_BOUND * want).all(), p
        sabs = np.abs(lp[:, we.sites(L, p)]).sum((1, 2))
        assert (np.abs(host(ld)[:, p].sum(-1) - sld[:, p]) <= wc.logdet_tol(12 * Vh, sabs)).all(), p
    lat = LatticeSU3(NB, list(L))
    t = lat.clover_term_n(xn, K, c_sw)
    assert torch.equal(t.a, cl) and torch.equal(t.ainv, inv) and (t.kappa, t.c_sw) == (K, c_sw)
    assert t.min_pivot.shape == (NB,) and t.logdet.shape == (NB, 2)
    assert torch.equal(t.min_pivot, mp.amin((1, 2))) and torch.equal(t.logdet, ops.sum_parts(ld))
    assert bool((t.min_pivot > 0.5).all())                               # min eig > 0.5 bounds every pivot from below
    t2 = lat.clover_term(dev(x), K, c_sw)
    assert torch.equal(t2.a, cl) and torch.equal(t2.ainv, inv)


@gpu
@pytest.mark.parametrize('kind,c_sw', [('smooth', 1.769), ('hot', 1.0)])
@pytest.mark.parametrize('L', we.EO_GPU_LATTICES)
def test_hop_and_apply_against_restatement(L, kind, c_sw):
    from l2hmc import _ops as ops
    x, a, ainv = reference(L, kind, c_sw)
    Vh = int(np.prod(L)) // 2
    psi, aux = wr.spinors(L, NB, NRHS), we.aux_field(L, NB, NRHS)
    xn = ops.su3_pack(dev(x))
    blocks = {'a': dev(wc.pack_blocks(a)), 'ainv': dev(wc.pack_blocks(ainv)), None: None}
    site = {'a': a, 'ainv': ainv, None: None}
    worst = 0.0
    for nrhs in (1, NRHS):
        src = [dev(we.pack_half(psi[:, :nrhs], p)) for p in (0, 1)]
        au = [dev(we.pack_half(aux[:, :nrhs], p)) for p in (0, 1)]
        keep = [t.clone() for t in src + au + [blocks['a'], blocks['ainv'], xn]]
        for p in (0, 1):
            for fl, (dagger, ap) in enumerate(wr.FLAGS):
                for name, cmode, blk, _, ca, cb, with_aux in wc.uses():
                    kw = dict(a=ca, aux=au[p], b=cb) if with_aux else dict(a=ca)
                    out, part = ops.su3_wilson_clover_hop_eo_n(xn, src[1 - p], L, p, blocks[blk], cmode, dagger, ap,
                                                               norm=True, **kw)
                    assert out.shape == (NB, nrhs, 12, Vh) and part.shape == (NB, nrhs, -(-Vh // 256))
                    w = we.pack_half(wc.hop_clover(x, psi[:, :nrhs], p, site[blk], cmode, dagger, ap, ca,
                                                   aux[:, :nrhs] if with_aux else None, cb), p)
                    d = float(np.abs(host(out) - w).max())
                    worst = max(worst, d)
                    assert d <= wc.TOL_HOP, (nrhs, p, fl, name, d)
                    n2 = (w.real ** 2 + w.imag ** 2).sum((2, 3))
                    assert float((np.abs(host(part).sum(-1) - n2) / n2).max()) <= wr.norm_bound(Vh), (nrhs, p, fl, name)
                    mine = torch.full_like(out, -7.0)                      # the norm changes nothing; out given is out returned
                    assert ops.su3_wilson_clover_hop_eo_n(xn, src[1 - p], L, p, blocks[blk], cmode, dagger, ap, out=mine,
                                                          **kw) is mine
                    assert torch.equal(mine, out)
                    if with_aux and fl == 2:                               # out == aux: the same bits
                        inplace = au[p].clone()
                        ops.su3_wilson_clover_hop_eo_n(xn, src[1 - p], L, p, blocks[blk], cmode, dagger, ap, a=ca,
                                                       aux=inplace, b=cb, out=inplace)
                        assert torch.equal(inplace, out)
                    if cmode == 0:                                         # the existing hop, within its own tolerance
                        old = ops.su3_wilson_hop_eo_n(xn, src[1 - p], L, p, dagger, ap, **kw)
                        assert float((old - out).abs().max()) <= we.TOL, (nrhs, p, fl, name)
            for blk in ('a', 'ainv'):
                out, part = ops.su3_clover_apply_n(blocks[blk], src[p], L, p, norm=True)
                w = we.pack_half(wc.apply_site(site[blk], psi[:, :nrhs]) * we.mask(L, p), p)
                assert float(np.abs(host(out) - w).max()) <= wc.TOL_M, (nrhs, p, blk)
                n2 = (w.real ** 2 + w.imag ** 2).sum((2, 3))
                assert float((np.abs(host(part).sum(-1) - n2) / n2).max()) <= wr.norm_bound(Vh), (nrhs, p, blk)
                inplace = src[p].clone()
                assert ops.su3_clover_apply_n(blocks[blk], inplace, L, p, out=inplace) is inplace
                assert torch.equal(inplace, out)
        assert all(torch.equal(t, k) for t, k in zip(src + au + [blocks['a'], blocks['ainv'], xn], keep))
    print(f'{L} {kind} {c_sw}: worst hop deviation / tolerance {worst / wc.TOL_HOP:.3g}')


@gpu
@pytest.mark.parametrize('L', [(4, 2, 6, 2), (4, 4, 4, 10)])
def test_dirac_layouts_adjoint_covariance_and_schur_identity(L):
    from l2hmc import _ops as ops
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    V = int(np.prod(L))
    lat = LatticeSU3(NB, list(L))
    c_sw = 1.769
    x0, a0, _ = reference(L, 'smooth', c_sw)
    psi0, phi0 = wr.spinors(L, NB, 3), wr.spinors(L, NB, 6)[:, 3:]
    tol = tol_dirac(psi0)
    x, psi = dev(x0), dev(psi0)
    xn, pn = lat.pack(x).clone(), ops.su3_spinor_pack(psi)
    cl = lat.clover_term_n(xn, K, c_sw)
    keep = [t.clone() for t in (x, psi, xn, pn, cl.a, cl.ainv)]
    for dagger, ap in wr.FLAGS:
        y = lat.wilson_clover_dirac(x, psi, K, c_sw, dagger, ap)
        yn = lat.wilson_clover_dirac_n(xn, pn, K, c_sw, dagger, ap)
        assert y.shape == psi.shape and torch.equal(ops.su3_spinor_pack(y), yn)              # one code path, two layouts
        d = float(np.abs(host(y) - wc.wilson_clover(x0, psi0, K, c_sw, dagger, ap, a0)).max())
        assert d <= tol, (dagger, ap, d)
        assert torch.equal(lat.wilson_clover_dirac_n(xn, pn, K, c_sw, dagger, ap, clover=cl), yn)
        y1 = lat.wilson_clover_dirac(x, psi[:, 1], K, c_sw, dagger, ap)
        assert y1.shape == psi[:, 1].shape and torch.equal(y1, y[:, 1])
        # <phi, M psi> = <M^H phi, psi>: sums of 12 V products of two kernel outputs in different orders
        md = host(lat.wilson_clover_dirac(x, dev(phi0), K, c_sw, not dagger, ap))
        lhs = (phi0.conj() * host(y)).sum(axis=(2, 3, 4, 5, 6, 7))
        rhs = (md.conj() * psi0).sum(axis=(2, 3, 4, 5, 6, 7))
        assert np.abs(lhs - rhs).max() <= 24 * V * 2.0 ** -52 * 8 * np.abs(lhs).max(), (dagger, ap)
        # the Schur identity, kernels only: (M psi)_e + kappa H_eo A_oo^-1 (M psi)_o = Mhat psi_e
        me, mo = ops.su3_spinor_split_eo(yn, L)
        lhs = ops.su3_wilson_clover_hop_eo_n(xn, ops.su3_clover_apply_n(cl.ainv, mo, L, 1), L, 0, None, 0, dagger, ap,
                                             a=K, aux=me, b=1.0)
        pe = ops.su3_spinor_split_eo(pn, L)[0]
        rhs = lat.wilson_clover_schur_n(xn, pe, K, c_sw, dagger, ap, clover=cl)
        assert float((lhs - rhs).abs().max()) <= 3 * wc.TOL_HOP, (dagger, ap)
        ys = lat.wilson_clover_schur(x, psi, K, c_sw, dagger, ap)
        halves = ops.su3_spinor_split_eo(ops.su3_spinor_pack(ys), L)
        assert torch.equal(halves[0], rhs) and not bool(halves[1].any())
    assert all(torch.equal(t, k) for t, k in zip((x, psi, xn, pn, cl.a, cl.ainv), keep))
    # gauge covariance through the project's own gauge_transform: M_sw[U^g] (g psi) = g M_sw[U] psi
    g0 = gf.random_su3(np.random.default_rng(43), (NB, *L))
    gx = lat.gauge_transform(x, dev(g0))
    gpsi = np.einsum('btxyzij,brtxyzaj->brtxyzai', g0, psi0)
    lhs = host(lat.wilson_clover_dirac(gx, dev(gpsi), K, c_sw))
    rhs = np.einsum('btxyzij,brtxyzaj->brtxyzai', g0, host(lat.wilson_clover_dirac(x, psi, K, c_sw)))
    assert float(np.abs(lhs - rhs).max()) <= 2 * tol


def residual(x0, b0, psi, kappa, c_sw):
    return np.sqrt(wr.norm2(b0 - wc.wilson_clover(x0, psi, kappa, c_sw)) / wr.norm2(b0))


@gpu
@pytest.mark.parametrize('kappa', wr.SOLVE_KAPPAS)
@pytest.mark.parametrize('L', we.SOLVE_LATTICES)
def test_solve_against_restatement(L, kappa):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    lat = LatticeSU3(NB, list(L))
    x0, b0 = wr.links(L, NB), wr.spinors(L, NB, 2)
    x, b = dev(x0), dev(b0)
    keep = b.clone()
    plain = lat.wilson_solve_eo(x, b, kappa, tol=TOL_SOLVE, max_iter=200)[1]['iters']
    for c_sw in wc.C_SWS:
        psi, info = lat.wilson_clover_solve(x, b, kappa, c_sw, tol=TOL_SOLVE, max_iter=200)
        assert torch.equal(b, keep) and psi.shape == b.shape and sorted(info) == ['converged', 'iters', 'residual']
        for k in info:
            assert tuple(info[k].shape) == (NB, 2), k
        print(f"{L} kappa {kappa} c_sw {c_sw}: iters {host(info['iters']).tolist()} (plain {host(plain).tolist()}), "
              f"residual {host(info['residual']).max():.3g}")
        assert bool(info['converged'].all()) and int(info['iters'].min()) > 0
        assert float(info['residual'].max()) <= 2 * TOL_SOLVE
        assert residual(x0, b0, host(psi), kappa, c_sw).max() <= 2 * TOL_SOLVE
        want, winfo = wc.solve_clover(x0, b0, kappa, c_sw, tol=TOL_SOLVE, max_iter=200)
        assert winfo['residual'].max() <= 2 * TOL_SOLVE
        diff = np.sqrt(wr.norm2(wc.wilson_clover(x0, host(psi) - want, kappa, c_sw)) / wr.norm2(b0))
        assert diff.max() <= 4 * TOL_SOLVE, diff
        p1, i1 = lat.wilson_clover_solve(x, b[:, 1], kappa, c_sw, tol=TOL_SOLVE, max_iter=200)
        assert p1.shape == b[:, 1].shape and tuple(i1['iters'].shape) == (NB, 1) and torch.equal(p1, psi[:, 1])


@gpu
def test_solve_against_dense():
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (2, 2, 2, 2)
    x0, b0 = wr.links(L, NB), wr.spinors(L, NB, 2)
    lat = LatticeSU3(NB, list(L))
    for kappa in wr.SOLVE_KAPPAS:
        for c_sw in wc.C_SWS:
            psi, info = lat.wilson_clover_solve(dev(x0), dev(b0), kappa, c_sw, tol=TOL_SOLVE, max_iter=200)
            assert bool(info['converged'].all()) and float(info['residual'].max()) <= 2 * TOL_SOLVE
            for c in range(NB):
                m = wc.dense(x0[c:c + 1], kappa, c_sw)
                smin = np.linalg.svd(m, compute_uv=False)[-1]
                for j in range(2):
                    err = np.linalg.norm(host(psi)[c, j].reshape(-1) - np.linalg.solve(m, b0[c, j].reshape(-1)))
                    assert err <= 2 * TOL_SOLVE * np.linalg.norm(b0[c, j]) / smin, (kappa, c_sw, c, j)


@gpu
def test_systems_freeze_prebuilt_term_and_csw_zero():
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 2, 6, 2)
    x0, b0 = wr.links(L, 3).copy(), wr.spinors(L, 3, 2).copy()
    x0[1] = wc.hot_links(L, 1)[0]                      # another configuration: another iteration count
    b0[2, 1] = 0.0                                     # a zero right-hand side converges at once
    x, b = dev(x0), dev(b0)
    lat3, lat1 = LatticeSU3(3, list(L)), LatticeSU3(1, list(L))
    kw = dict(tol=TOL_SOLVE, max_iter=300, check_every=2)
    psi, info = lat3.wilson_clover_solve(x, b, 0.12, 1.0, **kw)
    it = host(info['iters'])
    print('iters', it.tolist())
    assert bool(info['converged'].all()) and float(info['residual'].max()) <= 2 * TOL_SOLVE
    assert it[2, 1] == 0 and not bool(psi[2, 1].any()) and float(info['residual'][2, 1]) == 0.0
    assert len(set(it.reshape(-1).tolist())) > 2       # the systems leave the loop at different checks
    for c in range(3):
        pc, ic = lat1.wilson_clover_solve(x[c:c + 1].clone(), b[c:c + 1].clone(), 0.12, 1.0, **kw)
        assert torch.equal(pc, psi[c:c + 1]) and torch.equal(ic['iters'], info['iters'][c:c + 1]), c
    for j in range(2):
        pj, ij = lat3.wilson_clover_solve(x, b[:, j:j + 1].clone(), 0.12, 1.0, **kw)
        assert torch.equal(pj, psi[:, j:j + 1]) and torch.equal(ij['iters'], info['iters'][:, j:j + 1]), j
    _, i5 = lat3.wilson_clover_solve(x, b[:, :1].clone(), 0.12, 1.0, tol=TOL_SOLVE, max_iter=5)
    assert not bool(i5['converged'].any()) and bool((i5['iters'] == 5).all()) and float(i5['residual'].min()) > TOL_SOLVE
    # a prebuilt term gives the bits of the call that builds it
    cl = lat3.clover_term(x, 0.12, 1.0)
    again, ainfo = lat3.wilson_clover_solve(x, b, 0.12, 1.0, clover=cl, **kw)
    assert torch.equal(again, psi) and torch.equal(ainfo['iters'], info['iters'])
    # c_sw = 0: A = 1 exactly, the plain even-odd solve; both stop at a residual <= 2 tol |b|
    p0, i0 = lat3.wilson_clover_solve(x, b, 0.12, 0.0, **kw)
    pe, ie = lat3.wilson_solve_eo(x, b, 0.12, **kw)
    zero = lat3.clover_term(x, 0.12, 0.0)
    assert bool((zero.min_pivot == 1.0).all()) and bool((zero.logdet == 0.0).all())
    assert float(i0['residual'].max()) <= 2 * TOL_SOLVE and float(ie['residual'].max()) <= 2 * TOL_SOLVE
    bb = np.where(wr.norm2(b0) > 0, wr.norm2(b0), 1.0)
    assert np.sqrt(wr.norm2(wr.wilson(x0, host(p0 - pe), 0.12)) / bb).max() <= 4 * TOL_SOLVE


@gpu
@pytest.mark.parametrize('src', [(2, 1, 0, 1), (1, 1, 0, 1)])               # an even and an odd site
def test_propagator(src):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3, pion_correlator
    L = (4, 2, 2, 2)
    x0 = wr.links(L, NB)
    x = dev(x0)
    lat = LatticeSU3(NB, list(L))
    kappa, c_sw = 0.10, 1.0
    S, info = lat.quark_propagator(x, kappa, source=src, c_sw=c_sw, tol=TOL_SOLVE, max_iter=200)
    assert S.shape == (NB, *L, 4, 3, 4, 3) and tuple(info['iters'].shape) == (NB, 12) and bool(info['converged'].all())
    assert float(info['residual'].max()) <= 2 * TOL_SOLVE
    bsrc = wr.point_sources(NB, L, src)
    for j in (0, 7, 11):                                                    # the twelve solves, one by one: the same bits
        pj, _ = lat.wilson_clover_solve(x, dev(bsrc)[:, j], kappa, c_sw, tol=TOL_SOLVE, max_iter=200)
        assert torch.equal(pj, S[..., j // 3, j % 3])
    for c in range(NB):
        m = wc.dense(x0[c:c + 1], kappa, c_sw)
        smin = np.linalg.svd(m, compute_uv=False)[-1]
        inv = np.linalg.solve(m, bsrc[c].reshape(12, -1).T)
        assert np.linalg.norm(host(S)[c].reshape(-1, 12) - inv, axis=0).max() <= 2 * TOL_SOLVE / smin, c
    C = host(pion_correlator(S, src[0]))
    assert C.shape == (NB, L[0]) and (C > 0).all()
    S2, _ = lat.quark_propagator(x, kappa, source=src, c_sw=c_sw, clover=lat.clover_term(x, kappa, c_sw), even_odd=True,
                                 tol=TOL_SOLVE, max_iter=200)
    assert torch.equal(S2, S)
    Sw, _ = lat.quark_propagator(x, kappa, source=src, even_odd=True, tol=TOL_SOLVE, max_iter=200)
    assert not torch.equal(Sw, S)                                           # the clover term is really there


@gpu
def test_what_must_raise():
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 4, 4, 4)
    lat = LatticeSU3(2, list(L))
    x, b = dev(wr.links(L, 2)), dev(wr.spinors(L, 2, 1))
    with pytest.raises(ValueError, match=r'chain [01].*pivot -[0-9.]+'):
        lat.wilson_clover_solve(x, b, K, wc.C_SW_BAD)
    with pytest.raises(ValueError, match='positive definite'):
        lat.quark_propagator(x, K, c_sw=wc.C_SW_BAD)
    with pytest.raises(ValueError, match='positive definite'):
        lat.wilson_clover_schur(x, b, K, wc.C_SW_BAD)
    bad = lat.clover_term(x, K, wc.C_SW_BAD)
    assert bool((bad.min_pivot <= 0).all())
    lat.wilson_clover_dirac(x, b, K, wc.C_SW_BAD, clover=bad)                # M_sw itself needs no inverse
    for call in (lambda: lat.wilson_clover_solve(x, b, float('nan'), 1.0), lambda: lat.wilson_clover_solve(x, b, K, float('inf')),
                 lambda: lat.clover_term(x, K, None), lambda: lat.quark_propagator(x, K, c_sw=1.0, even_odd=False),
                 lambda: lat.quark_propagator(x, K, c_sw=1.0, even_odd=True, mixed=True),
                 lambda: lat.wilson_clover_solve(x, b, K, 1.0, clover=bad),
                 lambda: lat.wilson_clover_solve(x[:1], b[:1], K, wc.C_SW_BAD, clover=bad)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError, match='autograd'):
        lat.wilson_clover_solve(x.clone().requires_grad_(True), b, K, 1.0)
    odd = LatticeSU3(2, [3, 4, 5, 2])
    xo = torch.zeros(2, 4, 3, 4, 5, 2, 3, 3, dtype=torch.complex128, device='cuda')
    fo = torch.zeros(2, 1, 3, 4, 5, 2, 4, 3, dtype=torch.complex128, device='cuda')
    for call in (lambda: odd.clover_term(xo, K, 1.0), lambda: odd.wilson_clover_dirac(xo, fo, K, 1.0),
                 lambda: odd.wilson_clover_solve(xo, fo, K, 1.0), lambda: odd.quark_propagator(xo, K, c_sw=1.0)):
        with pytest.raises(ValueError, match=r'even extents.*\[3, 4, 5, 2\]'):
            call()
