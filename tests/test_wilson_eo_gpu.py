"""GPU tests of even-odd preconditioning: the half-lattice hop kernel (csrc/su3_wilson_eo.hip) against the numpy
restatement tests/wilson_eo_restatement.py, the Schur identity against the project's own full operator, the public
interface on top (`wilson_schur`, `wilson_solve_eo`, the propagator, the even-odd pseudofermions) and the trajectory of
`WilsonHMCEvenOdd`.

The tolerance of a single hop is we.TOL = 32 x the extended-precision yardstick of the hop (1.73e-13: with a = 1 the
outputs are ~1/kappa larger than those of M).  Where a CG solve stands against a dense one the bound is 32 x the
restatement's own distance between its CG and its dense solve (we.CG_S0, we.CG_FD, we.CG_TRAJ, measured on the CPU;
derivations in tests/wilson_eo_restatement.py and profiles/su3_wilson_eo.md).
Mhat psi_e is two hops: the first is within we.TOL of exact on entries of size up to ~40, the second carries that error
through at most 16 terms of unit size and adds its own rounding on an input ~40 times larger than the yardstick's, all
times kappa^2: at most kappa^2 (16 + 40) we.TOL = 0.86 we.TOL at kappa = wr.KAPPA.  SCHUR_TOL = we.TOL covers it."""
import functools

import numpy as np
import pytest
import torch

import gaugefix_restatement as gf
import wilson_eo_restatement as we
import wilson_force_restatement as wf
import wilson_restatement as wr
import wilson_gpu_util
from wilson_gpu_util import dev, host, unit_links

gpu = pytest.mark.gpu
NB = 3
TOL_SOLVE = 1e-10
SCHUR_TOL = we.TOL                                       # see the head of the file


@functools.lru_cache(maxsize=None)
def reference(L):
    """links, src and aux at nrhs = 12 (nrhs = 1 is the first column) and the restatement's hop for parity x flags x use"""
    x, psi, aux = wr.links(L, NB), wr.spinors(L, NB, 12), we.aux_field(L, NB, 12)
    want = {(p, fl, u): we.pack_half(we.hop_eo(x, psi, p, dagger, ap, a, aux if with_aux else None, b), p)
            for p in (0, 1) for fl, (dagger, ap) in enumerate(wr.FLAGS) for u, (_, a, b, with_aux) in enumerate(we.uses())}
    return x, psi, aux, want


@gpu
@pytest.mark.parametrize('L', we.EO_GPU_LATTICES)
def test_hop_against_restatement(L):
    from l2hmc import _ops as ops
    x, psi, aux, want = reference(L)
    Vh = int(np.prod(L)) // 2
    xn = ops.su3_pack(dev(x))
    keepx = xn.clone()
    worst = worstn = 0.0
    for nrhs in (1, 12):
        src = [dev(we.pack_half(psi[:, :nrhs], p)) for p in (0, 1)]
        au = [dev(we.pack_half(aux[:, :nrhs], p)) for p in (0, 1)]
        keep = [t.clone() for t in src + au]
        for p in (0, 1):
            for fl, (dagger, ap) in enumerate(wr.FLAGS):
                for u, (name, a, b, with_aux) in enumerate(we.uses()):
                    kw = dict(a=a, aux=au[p], b=b) if with_aux else dict(a=a)
                    out, part = ops.su3_wilson_hop_eo_n(xn, src[1 - p], L, p, dagger, ap, norm=True, **kw)
                    assert out.shape == (NB, nrhs, 12, Vh) and part.shape == (NB, nrhs, -(-Vh // 256))
                    w = want[p, fl, u][:, :nrhs]
                    d = float(np.abs(host(out) - w).max())
                    worst = max(worst, d)
                    assert d <= we.TOL, (nrhs, p, fl, name, d)
                    n2 = (w.real ** 2 + w.imag ** 2).sum((2, 3))
                    rel = float((np.abs(host(part).sum(-1) - n2) / n2).max())
                    worstn = max(worstn, rel)
                    assert rel <= wr.norm_bound(Vh), (nrhs, p, fl, name, rel)
                    # the norm changes nothing; an output given by the caller is the one written and returned
                    mine = torch.full_like(out, -7.0)
                    assert ops.su3_wilson_hop_eo_n(xn, src[1 - p], L, p, dagger, ap, out=mine, **kw) is mine
                    assert torch.equal(mine, out)
                    if with_aux and fl == 2:                         # out == aux: the same bits
                        inplace = au[p].clone()
                        ops.su3_wilson_hop_eo_n(xn, src[1 - p], L, p, dagger, ap, a=a, aux=inplace, b=b, out=inplace)
                        assert torch.equal(inplace, out)
        assert all(torch.equal(t, k) for t, k in zip(src + au, keep))      # inputs are never written
    assert torch.equal(xn, keepx)
    print(f'{L}: worst deviation / tolerance {worst / we.TOL:.3g}, norm {worstn / wr.norm_bound(Vh):.3g}')


@gpu
@pytest.mark.parametrize('L', we.EO_GPU_LATTICES)
def test_schur_identity_against_the_full_operator(L):
    """(M psi)_e + kappa H_eo (M psi)_o = Mhat psi_e, M by `su3_wilson_apply_n`: no restatement involved.  Both sides are
    a handful of kernel launches on the same inputs, each within we.TOL of exact; and split / merge are inverse"""
    from l2hmc import _ops as ops
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    lat = LatticeSU3(NB, list(L))
    xn = ops.su3_pack(dev(wr.links(L, NB)))
    pn = ops.su3_spinor_pack(dev(wr.spinors(L, NB, 2)))
    pe, po = ops.su3_spinor_split_eo(pn, L)
    assert torch.equal(ops.su3_spinor_merge_eo(pe, po, L), pn)
    assert torch.equal(pe, dev(we.pack_half(wr.spinors(L, NB, 2), 0))) and torch.equal(po, dev(we.pack_half(wr.spinors(L, NB, 2), 1)))
    for dagger, ap in wr.FLAGS:
        me, mo = ops.su3_spinor_split_eo(ops.su3_wilson_apply_n(xn, pn, we.K, L, dagger, ap), L)
        lhs = ops.su3_wilson_hop_eo_n(xn, mo, L, 0, dagger, ap, a=we.K, aux=me, b=1.0)
        rhs = lat.wilson_schur_n(xn, pe, we.K, dagger, ap)
        d = float((lhs - rhs).abs().max())
        assert d <= 2 * SCHUR_TOL, (dagger, ap, d)
        # H alone: the two halves of the full hop, (psi - M psi) / kappa, M psi within wr.TOL of exact
        ho = ops.su3_wilson_hop_eo_n(xn, pe, L, 1, dagger, ap)
        he = ops.su3_wilson_hop_eo_n(xn, po, L, 0, dagger, ap)
        full = (pn - ops.su3_wilson_apply_n(xn, pn, we.K, L, dagger, ap)) / we.K
        assert float((ops.su3_spinor_merge_eo(he, ho, L) - full).abs().max()) <= we.TOL + wr.TOL / we.K, (dagger, ap)


@gpu
def test_wilson_schur_layouts_adjoint_and_gauge_covariance():
    from l2hmc import _ops as ops
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 2, 6, 2)
    V = int(np.prod(L))
    lat = LatticeSU3(NB, list(L))
    x0, psi0, phi0 = wr.links(L, NB), wr.spinors(L, NB, 3), wr.spinors(L, NB, 6)[:, 3:]
    x, psi = dev(x0), dev(psi0)
    xn = lat.pack(x).clone()
    pe = dev(we.pack_half(psi0, 0))
    keep = [t.clone() for t in (x, psi, pe)]
    for dagger, ap in wr.FLAGS:
        y = lat.wilson_schur(x, psi, we.K, dagger, ap)                       # only the even sites of psi are read
        yn = lat.wilson_schur_n(xn, pe, we.K, dagger, ap)
        assert y.shape == psi.shape and yn.shape == pe.shape
        assert torch.equal(ops.su3_spinor_split_eo(ops.su3_spinor_pack(y), L)[0], yn)       # one code path, two layouts
        assert not bool(ops.su3_spinor_split_eo(ops.su3_spinor_pack(y), L)[1].any())        # the odd sites come back zero
        assert np.abs(host(y) - we.schur(x0, psi0, we.K, dagger, ap)).max() <= SCHUR_TOL
        y1 = lat.wilson_schur(x, psi[:, 1], we.K, dagger, ap)
        assert y1.shape == psi[:, 1].shape and torch.equal(y1, y[:, 1])
        assert torch.equal(lat.wilson_schur_n(xn, pe[:, 1], we.K, dagger, ap), yn[:, 1])
        md = host(lat.wilson_schur(x, dev(phi0), we.K, not dagger, ap))
        a = (phi0.conj() * host(y)).sum(axis=(2, 3, 4, 5, 6, 7))
        b = (md.conj() * psi0).sum(axis=(2, 3, 4, 5, 6, 7))
        assert np.abs(a - b).max() <= 24 * V * 2.0 ** -52 * 8 * np.abs(a).max(), (dagger, ap)
    assert all(torch.equal(t, k) for t, k in zip((x, psi, pe), keep))
    # gauge covariance through the project's own gauge_transform: Mhat[U^g](g psi) = g Mhat[U] psi
    g0 = gf.random_su3(np.random.default_rng(43), (NB, *L))
    gx = lat.gauge_transform(x, dev(g0))
    gpsi = np.einsum('btxyzij,brtxyzaj->brtxyzai', g0, psi0)
    for dagger, ap in wr.FLAGS:
        lhs = host(lat.wilson_schur(gx, dev(gpsi), we.K, dagger, ap))
        rhs = np.einsum('btxyzij,brtxyzaj->brtxyzai', g0, host(lat.wilson_schur(x, psi, we.K, dagger, ap)))
        assert float(np.abs(lhs - rhs).max()) <= 2 * SCHUR_TOL, (dagger, ap)


@functools.lru_cache(maxsize=None)
def solver_inputs(L):
    return wr.links(L, NB), wr.spinors(L, NB, 2)


@gpu
@pytest.mark.parametrize('kappa', wr.SOLVE_KAPPAS)
@pytest.mark.parametrize('L', we.SOLVE_LATTICES)
def test_solver_converges_in_fewer_iterations(L, kappa):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    lat = LatticeSU3(NB, list(L))
    x0, b0 = solver_inputs(L)
    x, b = dev(x0), dev(b0)
    keep = b.clone()
    psi, info = lat.wilson_solve_eo(x, b, kappa, tol=TOL_SOLVE, max_iter=200)
    full, finfo = lat.wilson_solve(x, b, kappa, tol=TOL_SOLVE, max_iter=200)
    assert torch.equal(b, keep) and psi.shape == b.shape
    for k in ('iters', 'residual', 'converged'):
        assert tuple(info[k].shape) == (NB, 2), k
    assert sorted(info) == sorted(finfo)
    print(f"{L} kappa {kappa}: iters {host(info['iters']).tolist()} (full {host(finfo['iters']).tolist()}), residual "
          f"{host(info['residual']).max():.3g}")
    assert bool(info['converged'].all()) and int(info['iters'].min()) > 0
    assert float(info['residual'].max()) <= 2 * TOL_SOLVE
    res = np.sqrt(wr.norm2(b0 - wr.wilson(x0, host(psi), kappa)) / wr.norm2(b0))
    assert res.max() <= 2 * TOL_SOLVE, res
    assert bool((info['iters'] < finfo['iters']).all())
    p1, i1 = lat.wilson_solve_eo(x, b[:, 1], kappa, tol=TOL_SOLVE, max_iter=200)
    assert p1.shape == b[:, 1].shape and tuple(i1['iters'].shape) == (NB, 1) and torch.equal(p1, psi[:, 1])


@gpu
def test_solver_against_the_full_solve_and_dense():
    """(2, 2, 2, 2): both solves stop at a residual of at most 2 tol |b| (asserted), so each is within 2 tol |b| /
    sigma_min of the exact solution and they are within 4 tol |b| / sigma_min of each other"""
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (2, 2, 2, 2)
    x0, b0 = solver_inputs(L)
    lat = LatticeSU3(NB, list(L))
    for kappa in wr.SOLVE_KAPPAS:
        psi, info = lat.wilson_solve_eo(dev(x0), dev(b0), kappa, tol=TOL_SOLVE, max_iter=200)
        full, finfo = lat.wilson_solve(dev(x0), dev(b0), kappa, tol=TOL_SOLVE, max_iter=200)
        assert bool(info['converged'].all()) and bool(finfo['converged'].all())
        assert float(info['residual'].max()) <= 2 * TOL_SOLVE and float(finfo['residual'].max()) <= 2 * TOL_SOLVE
        for c in range(NB):
            m = wr.dense(x0[c:c + 1], kappa)
            smin = np.linalg.svd(m, compute_uv=False)[-1]
            for j in range(2):
                nb_ = np.linalg.norm(b0[c, j])
                want = np.linalg.solve(m, b0[c, j].reshape(-1))
                assert np.linalg.norm(host(psi)[c, j].reshape(-1) - want) <= 2 * TOL_SOLVE * nb_ / smin, (kappa, c, j)
                assert np.linalg.norm(host(psi - full)[c, j]) <= 4 * TOL_SOLVE * nb_ / smin, (kappa, c, j)


@gpu
def test_systems_freeze_independently():
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 2, 6, 2)
    x0, b0 = solver_inputs(L)
    x0 = x0.copy()
    x0[1] = unit_links(1, L)[0]                       # the free field converges earlier
    b0 = b0.copy()
    b0[2, 1] = 0.0                                    # and a zero right-hand side at once
    x, b = dev(x0), dev(b0)
    lat3, lat1 = LatticeSU3(NB, list(L)), LatticeSU3(1, list(L))
    psi, info = lat3.wilson_solve_eo(x, b, 0.12, tol=TOL_SOLVE, max_iter=200, check_every=2)
    it = host(info['iters'])
    print('iters', it.tolist())
    assert bool(info['converged'].all()) and float(info['residual'].max()) <= 2 * TOL_SOLVE
    assert it[1].max() < it[0].min() and it[1].max() < it[2, 0]
    assert it[2, 1] == 0 and not bool(psi[2, 1].any()) and float(info['residual'][2, 1]) == 0.0
    for c in range(NB):
        pc, ic = lat1.wilson_solve_eo(x[c:c + 1].clone(), b[c:c + 1].clone(), 0.12, tol=TOL_SOLVE, max_iter=200, check_every=2)
        assert torch.equal(pc, psi[c:c + 1]) and torch.equal(ic['iters'], info['iters'][c:c + 1]), c
    for j in range(2):
        pj, ij = lat3.wilson_solve_eo(x, b[:, j:j + 1].clone(), 0.12, tol=TOL_SOLVE, max_iter=200, check_every=2)
        assert torch.equal(pj, psi[:, j:j + 1]) and torch.equal(ij['iters'], info['iters'][:, j:j + 1]), j
    _, i5 = lat3.wilson_solve_eo(x, b[:, :1].clone(), 0.12, tol=TOL_SOLVE, max_iter=5)
    assert not bool(i5['converged'].any()) and bool((i5['iters'] == 5).all()) and float(i5['residual'].min()) > TOL_SOLVE


@gpu
@pytest.mark.parametrize('src', [(2, 1, 0, 1), (1, 1, 0, 1)])               # an even and an odd site
def test_propagator(src):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3, pion_correlator
    L = (4, 2, 2, 2)
    x0 = wr.links(L, NB)
    x = dev(x0)
    lat = LatticeSU3(NB, list(L))
    kappa = 0.10
    S, info = lat.quark_propagator(x, kappa, source=src, tol=TOL_SOLVE, max_iter=200, even_odd=True)
    Sf, finfo = lat.quark_propagator(x, kappa, source=src, tol=TOL_SOLVE, max_iter=200)
    assert S.shape == (NB, *L, 4, 3, 4, 3) and tuple(info['iters'].shape) == (NB, 12) and bool(info['converged'].all())
    assert float(info['residual'].max()) <= 2 * TOL_SOLVE and bool((info['iters'] <= finfo['iters']).all())
    bsrc = wr.point_sources(NB, L, src)
    C, Cf = host(pion_correlator(S, src[0])), host(pion_correlator(Sf, src[0]))
    for c in range(NB):
        m = wr.dense(x0[c:c + 1], kappa)
        smin = np.linalg.svd(m, compute_uv=False)[-1]
        inv = np.linalg.solve(m, bsrc[c].reshape(12, -1).T)                  # [12 V, 12 sources]
        got = host(S)[c].reshape(-1, 12)
        assert np.linalg.norm(got - inv, axis=0).max() <= 2 * TOL_SOLVE / smin, c
        # C = |S|^2 summed: each propagator within 2 tol / sigma_min of the exact one column by column, so a time slice
        # differs by at most 2 |S| (4 tol / sigma_min) sqrt(12) over its twelve columns, |S| <= sqrt(C.sum())
        bound = 2 * np.sqrt(Cf[c].sum()) * 4 * TOL_SOLVE / smin * np.sqrt(12.0)
        assert np.abs(C[c] - Cf[c]).max() <= bound, (c, np.abs(C[c] - Cf[c]).max(), bound)
    pj, _ = lat.wilson_solve_eo(x, dev(bsrc)[:, 7], kappa, tol=TOL_SOLVE, max_iter=200)
    assert torch.equal(pj, S[..., 7 // 3, 7 % 3])


@gpu
def test_pseudofermion_refresh_and_action():
    from l2hmc import _ops as ops
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L, nb = (4, 2, 2, 2), 4
    lat = LatticeSU3(nb, list(L))
    x = dev(wr.links(L, 3)[[0, 1, 2, 0]])
    xn = lat.pack(x)
    g = torch.Generator(device='cuda')
    g.manual_seed(3)
    phi, s0 = lat.pseudofermion_refresh_eo_n(xn, 0.12, 2, g)
    assert phi.shape == (nb, 2, 12, 16) and s0.shape == (nb,)
    sf, info = lat.pseudofermion_action_n(xn, phi, 0.12, tol=wf.TRAJ_TOL_H, max_iter=2000, even_odd=True)
    assert bool(info['converged'].all())
    # 32 x the restatement's CG figure, plus the rounding of the two sums of 2 * 24 * 16 squares in their own orders
    bound = 32 * we.CG_S0 + 2 * wr.norm_bound(2 * 16)
    rel = float(((sf - s0).abs() / s0).max())
    print(f'|S_f - S0| / S0 = {rel:.3g}, bound {bound:.3g}')
    assert rel <= bound
    assert abs(float(s0.mean()) / (2 * 12 * 16) - 1.0) < 0.25                   # <|eta|^2> = 1 per complex component
    # the reference layout: the full shape, zero on the odd sites, and only the even sites are read back
    g.manual_seed(3)
    phir, s0r = lat.pseudofermion_refresh_eo(x, 0.12, 2, g)
    assert phir.shape == (nb, 2, *L, 4, 3) and torch.equal(s0r, s0)
    pe, po = ops.su3_spinor_split_eo(ops.su3_spinor_pack(phir), L)
    assert torch.equal(pe, phi) and not bool(po.any())
    junk = phir + dev(wr.spinors(L, 3, 2)[[0, 1, 2, 0]] * we.mask(L, 1))
    sr, _ = lat.pseudofermion_action(x, junk, 0.12, tol=wf.TRAJ_TOL_H, max_iter=2000, even_odd=True)
    assert torch.equal(sr, sf)
    # the restatement's heatbath of the same noise is the same field; a CPU generator gives the same numbers again
    gc = torch.Generator()
    gc.manual_seed(3)
    p1, _ = lat.pseudofermion_refresh_eo_n(xn, 0.12, 2, gc)
    gc.manual_seed(3)
    eta = torch.view_as_complex(torch.randn((nb, 2, 12, 16, 2), dtype=torch.float64, generator=gc) * float(np.sqrt(0.5)))
    want, s0w = we.refresh(host(x), we.unpack_half(eta.numpy(), L, 0), 0.12)
    assert np.abs(host(p1) - we.pack_half(want, 0)).max() <= SCHUR_TOL
    gc.manual_seed(3)
    assert torch.equal(p1, lat.pseudofermion_refresh_eo_n(xn, 0.12, 2, gc)[0])


@gpu
@pytest.mark.parametrize('ap', [False, True])
@pytest.mark.parametrize('L', we.FD_LATTICES)
def test_force_against_restatement_and_differences(L, ap):
    """`pseudofermion_force(even_odd=True)` against the restatement's even-odd force (dense solves) and sum <p, F>
    against the Richardson difference of `pseudofermion_action(even_odd=True)`, all solves at tol = 1e-13: within 32 x the
    error the restatement has with its own CG at that tol (we.CG_FD)"""
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    lat = LatticeSU3(2, list(L))
    x0, phi0, p = we.fd_inputs(L)
    kw = dict(tol=wf.FD_TOL, max_iter=4000, antiperiodic_t=ap, even_odd=True)
    phi = dev(phi0)
    F, s, info = lat.pseudofermion_force(dev(x0), phi, we.K, **kw)
    assert bool(info['converged'].all())
    Fn, sn, _ = lat.pseudofermion_force_n(lat.pack(dev(x0)), dev(we.pack_half(phi0, 0)), we.K, **kw)
    assert torch.equal(lat.unpack(Fn), F) and torch.equal(sn, s)
    m = host(Fn).reshape(2, 4, 3, 3, -1)                                           # exactly anti-Hermitian
    t = np.swapaxes(m, 2, 3)
    assert np.array_equal(t.real, -m.real) and np.array_equal(t.imag, m.imag)
    Fw = we.fermion_force(x0, phi0, we.K, ap)
    want = wf.pair(p, host(F))
    # the force is linear in X and Y, which carry the solver's error: the relative bound of the pairing serves entry-wise
    # against the largest entry
    assert np.abs(host(F) - Fw).max() <= 32 * we.CG_FD * np.abs(Fw).max()
    assert np.abs(host(s) - we.fermion_action(x0, phi0, we.K, ap)).max() <= 1e-10 * host(s).max()

    def action(xx):
        sf, i = lat.pseudofermion_action(dev(xx), phi, we.K, **kw)
        assert bool(i['converged'].all())
        return host(sf)
    d, d1, d2 = wf.richardson(x0, phi0, p, we.K, ap, h=1e-3, action=action)
    rel = np.abs(d - want) / np.abs(want)
    ratio = (d1 - want) / (d2 - want)
    print(f'{L} ap {ap}: relative {rel}, bound {32 * we.CG_FD:.3g}, ratio of the raw differences {ratio}')
    assert (rel <= 32 * we.CG_FD).all(), rel
    assert ((ratio > 3.5) & (ratio < 4.5)).all(), ratio


_hmc = functools.partial(wilson_gpu_util._hmc, cls='WilsonHMCEvenOdd')
_native = functools.partial(wilson_gpu_util._native, half=True)


@gpu
@pytest.mark.parametrize('L', wf.TRAJ_LATTICES)
def test_trajectory_against_restatement(L):
    """`leapfrog_n` and `hamiltonian_n` of `WilsonHMCEvenOdd` against the restatement's even-odd trajectory with dense
    solves: within 32 x the distance of the restatement's own trajectory with CG solves at the same tolerances from it"""
    from l2hmc import _ops as ops
    x, v, phi, s0 = we.traj_inputs(L)
    x1w, v1w, dhw = we.delta_h(x, v, phi, **wf.TRAJ)
    lat, hmc = _hmc(L, tol_md=wf.TRAJ_TOL_MD, tol_h=wf.TRAJ_TOL_H)
    xn, vn, pn = _native(x, v, phi)
    keep = [t.clone() for t in (xn, vn, pn)]
    x1, v1, info = hmc.leapfrog_n(xn, vn, pn)
    assert all(torch.equal(a, b) for a, b in zip((xn, vn, pn), keep))
    assert info['unconverged'] == 0 and info['cg_iters'].shape == (wf.TRAJ['nleapfrog'] + 1, 2, 1)
    dh = host(hmc.hamiltonian_n(x1, v1, pn) - hmc.hamiltonian_n(xn, vn, pn))
    got = {'x': np.abs(host(ops.su3_unpack(x1, L)) - x1w).max(), 'v': np.abs(host(ops.su3_unpack(v1, L)) - v1w).max(),
           'dH': np.abs(dh - dhw).max()}
    print(L, {k: f'{got[k] / (32 * we.CG_TRAJ[k]):.3g} of the bound' for k in got}, 'dH', dh)
    for k in got:
        assert got[k] <= 32 * we.CG_TRAJ[k], (k, got[k])
    sf, _ = lat.pseudofermion_action_n(xn, pn, wf.TRAJ['kappa'], tol=wf.TRAJ_TOL_H, even_odd=True)
    assert np.abs(host(sf) - s0).max() <= 1e-10 * s0.max()


@gpu
def test_reversibility_and_step_size_scaling():
    """(4, 4, 4, 4), as the test of the full operator with its bounds: leapfrog, momentum flip, leapfrog returns links
    and momentum within 1e-9 at tol_md = 1e-12 (the solver tolerance through 18 forces, not rounding), and dH(0.05, 8) /
    dH(0.025, 16) lies in (3.5, 4.5)"""
    L = (4, 4, 4, 4)
    x, v, phi, _ = we.traj_inputs(L)
    lat, hmc = _hmc(L, tol_md=1e-12)
    xn, vn, pn = _native(x, v, phi)
    x1, v1, info = hmc.leapfrog_n(xn, vn, pn)
    x2, v2, _ = hmc.leapfrog_n(x1, -v1, pn)
    rev = max(float((x2 - xn).abs().max()), float((v2 + vn).abs().max()))
    assert info['unconverged'] == 0 and float((x1 - xn).abs().max()) > 0.1
    h0 = hmc.hamiltonian_n(xn, vn, pn)
    a = host(hmc.hamiltonian_n(x1, v1, pn) - h0)
    _, half = _hmc(L, tol_md=1e-12, eps=wf.TRAJ['eps'] / 2, nleapfrog=2 * wf.TRAJ['nleapfrog'])
    x3, v3, _ = half.leapfrog_n(xn, vn, pn)
    b = host(half.hamiltonian_n(x3, v3, pn) - h0)
    print(f'reversibility {rev:.3g}; dH {a} / {b} = {a / b}')
    assert rev <= 1e-9
    assert ((a / b > 3.5) & (a / b < 4.5)).all()


@gpu
def test_trajectory_accept_reject_and_seed():
    L, nb = (4, 2, 2, 2), 4
    lat, hmc = _hmc(L, nb, npf=2)
    x = dev(wr.links(L, 3)[[0, 1, 2, 0]])

    def run(h):
        g = torch.Generator(device='cuda')
        g.manual_seed(11)
        return h.trajectory(x, generator=g)
    keep = x.clone()
    xo, m = run(hmc)
    xo2, m2 = run(hmc)
    assert torch.equal(x, keep)
    assert torch.equal(xo, xo2) and all(torch.equal(m[k], m2[k]) for k in ('acc', 'acc_mask', 'dH', 'plaq'))
    _, mf = run(_hmc(L, nb, cls='WilsonHMC', npf=2)[1])
    assert sorted(m) == sorted(mf)                                               # the same metrics
    assert m['unconverged'] == 0 and 0 < m['cg_iters_md']['mean'] < mf['cg_iters_md']['mean'] and m['cg_iters_h']['max'] > 0
    assert tuple(m['dH'].shape) == (nb,) and bool(torch.isfinite(m['dH']).all())
    _, wild = _hmc(L, nb, npf=2, eps=0.6, nleapfrog=3)
    xr, mr = run(wild)
    for xx, mm in ((xo, m), (xr, mr)):
        for c in range(nb):
            assert torch.equal(xx[c], x[c]) == (float(mm['acc_mask'][c]) == 0.0), c
    assert float(mr['acc_mask'].sum()) == 0.0 and float(mr['dH'].min()) > 10.0
    assert float(m['acc_mask'].sum()) > 0.0


@gpu
def test_kappa_zero():
    """kappa = 0: Mhat = 1, the fermions decouple: S_f = |phi_e|^2 and the leapfrog is the pure-gauge one"""
    from l2hmc import _ops as ops
    L = (4, 2, 2, 2)
    x, v, phi, _ = we.traj_inputs(L)
    lat, hmc = _hmc(L, kappa=0.0)
    xn, vn, pn = _native(x, v, phi)
    sf, _ = lat.pseudofermion_action_n(xn, pn, 0.0, even_odd=True)
    n2 = wr.norm2(phi).sum(1)
    assert np.abs(host(sf) - n2).max() <= wr.norm_bound(16) * n2.max()
    x1, v1, _ = hmc.leapfrog_n(xn, vn, pn)
    eps, n, beta = wf.TRAJ['eps'], wf.TRAJ['nleapfrog'], wf.TRAJ['beta']
    xg, vg = xn.clone(), vn.clone()
    ops.su3_force_kick_n(xg, beta, -0.5 * eps, vg, L)
    for k in range(n):
        xg = ops.su3_expm_mul_n(xg, vg, eps)
        ops.su3_force_kick_n(xg, beta, -(1.0 if k + 1 < n else 0.5) * eps, vg, L)
    assert float((x1 - xg).abs().max()) <= 1e-14 and float((v1 - vg).abs().max()) <= 1e-14
    h0, h1 = hmc.hamiltonian_n(xn, vn, pn), hmc.hamiltonian_n(x1, v1, pn)
    hg = ops.su3_kinetic_n(vg) + lat.action_n(xg, beta) - ops.su3_kinetic_n(vn) - lat.action_n(xn, beta)
    assert float(((h1 - h0) - hg).abs().max()) <= 1e-9                           # the pure-gauge dH
