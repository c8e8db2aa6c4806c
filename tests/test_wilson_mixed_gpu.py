"""GPU tests of the mixed-precision even-odd Wilson solves: the kernels of csrc/su3_wilson_f32.hip (the fp32 hop, the
parity-ordered fp32 link copy, the fp32 BLAS-1 kernels, demote and promote) against the numpy restatement
tests/wilson_mixed_restatement.py, the defect-correction solves `wilson_solve_eo_mixed_n` and
`wilson_solve_schur_normal_mixed_n`, the `mixed=True` keyword of the propagator and the pseudofermions, and the
trajectory of `WilsonHMCMixed`.

The tolerance of a single fp32 hop is wm.TOL_F32 = 32 x the extended-precision yardstick of the fp32 hop.  The outer
loop of a mixed solve stops on the fp64 test of the fp64 solver, so info['residual'] <= tol is derived, not measured.
Where a mixed solve stands against a dense one or against the fp64 path the bound is 32 x the restatement's own distance
between its mixed solves and its dense solves (wm.CG_X, wm.CG_S0, wm.CG_FD, wm.CG_TRAJ, measured on the CPU;
profiles/su3_wilson_mixed.md); against the fp64 path, whose own constants are we.CG_*, the two add."""
import functools

import numpy as np
import pytest
import torch

import wilson_eo_restatement as we
import wilson_force_restatement as wf
import wilson_mixed_restatement as wm
import wilson_restatement as wr
import wilson_gpu_util
from wilson_gpu_util import dev, host

gpu = pytest.mark.gpu
NB = 3
C64 = np.complex64
KAPPA = 0.124


@functools.lru_cache(maxsize=None)
def reference(L):
    """links, src and aux at nrhs = 12 (nrhs = 1 is the first column), rounded to complex64, and the restatement's fp32
    hop for parity x flags x use"""
    x, psi, aux = wr.links(L, NB), wr.spinors(L, NB, 12).astype(C64), we.aux_field(L, NB, 12).astype(C64)
    want = {(p, fl, u): we.pack_half(wm.hop_eo_f32(x, psi, p, dagger, ap, a, aux if with_aux else None, b), p)
            for p in (0, 1) for fl, (dagger, ap) in enumerate(wr.FLAGS) for u, (_, a, b, with_aux) in enumerate(we.uses())}
    return x, psi, aux, want


def sq(f):
    return (f.real.astype(np.float64) ** 2 + f.imag.astype(np.float64) ** 2).sum((-2, -1))


@gpu
@pytest.mark.parametrize('L', we.EO_GPU_LATTICES)
def test_f32_kernels_against_restatement(L):
    from l2hmc import _ops as ops
    x, psi, aux, want = reference(L)
    Vh = int(np.prod(L)) // 2
    xn = ops.su3_pack(dev(x))
    keepx = xn.clone()
    # the link copy: exactly float32 of every link, parity-ordered; twice the same bits
    x32 = ops.su3_links_demote_eo_n(xn, L)
    assert x32.shape == (NB, 2, 4, 9, Vh) and x32.dtype == torch.complex64
    assert np.array_equal(host(x32), wm.links_eo_f32(x))
    mine = torch.full_like(x32, -7.0)
    assert ops.su3_links_demote_eo_n(xn, L, out=mine) is mine and torch.equal(mine, x32)
    worst = worstn = 0.0
    for nrhs in (1, 12):
        src = [dev(we.pack_half(psi[:, :nrhs], p)) for p in (0, 1)]
        au = [dev(we.pack_half(aux[:, :nrhs], p)) for p in (0, 1)]
        keep = [t.clone() for t in src + au]
        for p in (0, 1):
            for fl, (dagger, ap) in enumerate(wr.FLAGS):
                for u, (name, a, b, with_aux) in enumerate(we.uses()):
                    kw = dict(a=a, aux=au[p], b=b) if with_aux else dict(a=a)
                    out, part = ops.su3_wilson_hop_eo_f32_n(x32, src[1 - p], L, p, dagger, ap, norm=True, **kw)
                    assert out.shape == (NB, nrhs, 12, Vh) and out.dtype == torch.complex64
                    assert part.shape == (NB, nrhs, -(-Vh // 256)) and part.dtype == torch.float64
                    d = float(np.abs(host(out) - want[p, fl, u][:, :nrhs]).max())
                    worst = max(worst, d)
                    assert d <= wm.TOL_F32, (nrhs, p, fl, name, d)
                    n2 = sq(host(out))
                    rel = float((np.abs(host(part).sum(-1) - n2) / n2).max())
                    worstn = max(worstn, rel)
                    assert rel <= wm.norm_bound_f32(Vh), (nrhs, p, fl, name, rel)
                    # called again: identical bits, field and partials; the norm changes nothing
                    mine = torch.full_like(out, -7.0)
                    mp = torch.full_like(part, -7.0)
                    assert ops.su3_wilson_hop_eo_f32_n(x32, src[1 - p], L, p, dagger, ap, out=mine, norm=mp, **kw)[0] is mine
                    assert torch.equal(mine, out) and torch.equal(mp, part)
                    mine.fill_(-7.0)
                    ops.su3_wilson_hop_eo_f32_n(x32, src[1 - p], L, p, dagger, ap, out=mine, **kw)
                    assert torch.equal(mine, out)
                    if with_aux and fl == 2:                         # out == aux: the same bits
                        inplace = au[p].clone()
                        ops.su3_wilson_hop_eo_f32_n(x32, src[1 - p], L, p, dagger, ap, a=a, aux=inplace, b=b, out=inplace)
                        assert torch.equal(inplace, out)
        assert all(torch.equal(t, k) for t, k in zip(src + au, keep))      # inputs are never written
        # the BLAS-1 kernels, demote and promote: the exact result of the float32 operands rounded once
        rng = np.random.default_rng(11)
        scal = rng.standard_normal((3, NB, nrhs))
        scal[:, 0, 0] = 0.0
        al, be, sc = (dev(s) for s in scal)
        a32, b32 = (s.astype(np.float32).astype(np.float64)[..., None, None] for s in scal[:2])
        xs, rs, ps, qs = (host(t).astype(np.complex128) for t in src + au)
        ulp = 2.0 ** -23
        for rep in range(2):
            xf, rf, pf = src[0].clone(), src[1].clone(), au[0].clone()
            part = ops.su3_spinor_cg_update_f32_(xf, rf, pf, au[1], al)
            ops.su3_spinor_xpay_f32_(pf, au[1], be)
            f64 = dev(we.pack_half(wr.spinors(L, NB, 12)[:, 12 - nrhs:], 0))
            dem = ops.su3_spinor_demote(f64, sc)
            x64 = ops.su3_spinor_promote_axpy_(f64.clone(), src[0], sc)
            got = [xf, rf, pf, part, dem, x64]
            if rep:
                assert all(torch.equal(g, f) for g, f in zip(got, first))
            first = got
        for got, w, size in ((xf, xs + a32 * ps, np.abs(xs) + np.abs(a32 * ps)), (rf, rs - a32 * qs, np.abs(rs) + np.abs(a32 * qs)),
                             (pf, qs + b32 * ps, np.abs(qs) + np.abs(b32 * ps))):
            assert (np.abs(host(got) - w) <= ulp * size).all()
        assert torch.equal(xf[0, 0], src[0][0, 0]) and torch.equal(rf[0, 0], src[1][0, 0])       # alpha = 0: the same bits
        rel = float((np.abs(host(part).sum(-1) - sq(host(rf))) / sq(host(rf))).max())
        assert rel <= wm.norm_bound_f32(Vh), rel
        f0, s0 = host(f64), scal[2][..., None, None]
        want_dem = ((s0 * f0.real).astype(np.float32) + 1j * (s0 * f0.imag).astype(np.float32)).astype(C64)
        assert np.array_equal(host(dem), want_dem)
        assert (np.abs(host(x64) - (f0 + s0 * xs)) <= 2.0 ** -52 * (np.abs(f0) + np.abs(s0 * xs))).all()
        assert torch.equal(x64[0, 0], f64[0, 0]) and not torch.equal(x64[1, 0], f64[1, 0])         # scale = 0: untouched
    assert torch.equal(xn, keepx)
    print(f'{L}: worst deviation / tolerance {worst / wm.TOL_F32:.3g}, norm {worstn / wm.norm_bound_f32(Vh):.3g}')


def norm2_t(f):
    """|f|^2 per system [nb, nrhs] of a native field, by torch"""
    return (f.real ** 2 + f.imag ** 2).sum((2, 3))


@functools.lru_cache(maxsize=None)
def solver_inputs(L):
    return wr.links(L, NB), wr.spinors(L, NB, 2)


@gpu
@pytest.mark.parametrize('tol', [1e-10, 1e-12])
@pytest.mark.parametrize('L', we.SOLVE_LATTICES)
def test_mixed_solves_converge_to_the_fp64_test(L, tol):
    from l2hmc import _ops as ops
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    lat = LatticeSU3(NB, list(L))
    x0, b0 = solver_inputs(L)
    xn, bn = ops.su3_pack(dev(x0)), ops.su3_spinor_pack(dev(b0))
    keep = bn.clone()
    psi, info = lat.wilson_solve_eo_mixed_n(xn, bn, KAPPA, tol=tol, max_iter=400)
    ref, rinfo = lat.wilson_solve_eo_n(xn, bn, KAPPA, tol=tol, max_iter=400)
    assert torch.equal(bn, keep) and psi.shape == bn.shape and psi.dtype == torch.complex128
    assert sorted(info) == ['converged', 'iters', 'outer', 'residual'] and all(tuple(v.shape) == (NB, 2) for v in info.values())
    rel = float((psi - ref).abs().max() / ref.abs().max())
    print(f"{L} tol {tol}: inner iters {host(info['iters']).tolist()} outer {host(info['outer']).tolist()} (fp64 iters "
          f"{host(rinfo['iters']).tolist()}), residual {float(info['residual'].max()):.3g}, |psi - psi64| / |psi64| {rel:.3g}")
    assert bool(info['converged'].all()) and bool(rinfo['converged'].all())
    assert float(info['residual'].max()) <= tol                                  # derived: the fp64 stopping test itself
    res = np.sqrt(wr.norm2(b0 - wr.wilson(x0, wr.unpack_spinor(host(psi), L), KAPPA)) / wr.norm2(b0))
    assert res.max() <= 2 * tol, res                                             # ... and the full system's, by numpy
    if tol < 1e-11:
        assert int(info['outer'].min()) >= 2                                     # fp32 alone cannot reach 1e-12
    assert rel <= 32 * (wm.CG_X + wf.CG_X)                                       # each solve against a dense one
    # the normal form on the Schur complement, against the fp64 one
    pe = ops.su3_spinor_split_eo(bn, L)[0].contiguous()
    X, Y, ninfo = lat.wilson_solve_schur_normal_mixed_n(xn, pe, KAPPA, tol=tol, max_iter=400)
    Xr, Yr, nr = lat.wilson_solve_schur_normal_n(xn, pe, KAPPA, tol=tol, max_iter=400)
    assert bool(ninfo['converged'].all()) and float(ninfo['residual'].max()) <= tol
    assert tol > 1e-11 or int(ninfo['outer'].min()) >= 2
    assert torch.equal(Y, lat.wilson_schur_n(xn, X, KAPPA))
    assert float((X - Xr).abs().max() / Xr.abs().max()) <= 32 * (wm.CG_X + wf.CG_X)
    # |Y|^2 = X^H A X: an X with the residual r has |Y|^2 off by 2 Re(X^H r) + O(r^2), at most 2 |X| tol |phi| (a CG
    # iterate is orthogonal to its residual, a defect-corrected one is not): 3 covers both solves
    first = 3 * tol * torch.sqrt(norm2_t(pe) * norm2_t(Xr)) / nr['action']
    dact = (ninfo['action'] - nr['action']).abs() / nr['action']
    assert bool((dact <= 32 * (wm.CG_S0 + we.CG_S0) + first + 2 * wr.norm_bound(int(np.prod(L)) // 2)).all()), dact


@gpu
def test_solver_against_dense():
    """(2, 2, 2, 2) and (4, 2, 2, 2): the mixed solve stops at a true residual of at most tol |b|, so it is within
    tol |b| / sigma_min(M) of the dense solution"""
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    for L in we.FD_LATTICES:
        x0, b0 = solver_inputs(L)
        lat = LatticeSU3(NB, list(L))
        for kappa in wr.SOLVE_KAPPAS:
            for tol in (1e-10, 1e-12):
                psi, info = lat.wilson_solve_eo_mixed(dev(x0), dev(b0), kappa, tol=tol)
                assert bool(info['converged'].all()) and float(info['residual'].max()) <= tol
                for c in range(NB):
                    m = wr.dense(x0[c:c + 1], kappa)
                    smin = np.linalg.svd(m, compute_uv=False)[-1]
                    for j in range(2):
                        want = np.linalg.solve(m, b0[c, j].reshape(-1))
                        err = np.linalg.norm(host(psi)[c, j].reshape(-1) - want)
                        assert err <= 2 * tol * np.linalg.norm(b0[c, j]) / smin, (L, kappa, tol, c, j, err)


@gpu
@pytest.mark.parametrize('which', ['eo', 'normal'])
def test_a_system_alone_and_in_a_batch(which):
    """x and every info entry of one system are the same bits alone and inside a 3 x 3 batch, one of whose systems is
    the free field (it converges earlier) and one a zero right-hand side"""
    from l2hmc import _ops as ops
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 2, 6, 2)
    x0, b0 = wr.links(L, NB).copy(), wr.spinors(L, NB, 3).copy()
    x0[1] = wilson_gpu_util.unit_links(1, L)[0]
    b0[2, 1] = 0.0
    lat3, lat1 = LatticeSU3(NB, list(L)), LatticeSU3(1, list(L))
    xn, bn = ops.su3_pack(dev(x0)), ops.su3_spinor_pack(dev(b0))
    if which == 'normal':
        bn = ops.su3_spinor_split_eo(bn, L)[0].contiguous()

    def solve(lat, xx, bb):
        if which == 'eo':
            return lat.wilson_solve_eo_mixed_n(xx, bb, 0.12, tol=1e-12, check_every=2)
        X, _, info = lat.wilson_solve_schur_normal_mixed_n(xx, bb, 0.12, tol=1e-12, check_every=2)
        return X, info
    psi, info = solve(lat3, xn, bn)
    print(which, {k: host(v).tolist() for k, v in info.items() if k != 'action'})
    assert bool(info['converged'].all()) and float(info['residual'].max()) <= 1e-12
    assert int(info['iters'][2, 1]) == 0 and int(info['outer'][2, 1]) == 0 and float(info['residual'][2, 1]) == 0.0
    assert not bool((psi[2, 1] if which == 'normal' else ops.su3_spinor_split_eo(psi, L)[0][2, 1]).any())
    assert len(set(host(info['iters']).reshape(-1).tolist())) > 1                # the systems stop at different checks
    for c in range(NB):
        for j in range(3):
            p1, i1 = solve(lat1, xn[c:c + 1].clone(), bn[c:c + 1, j:j + 1].clone())
            assert torch.equal(p1[0, 0], psi[c, j]), (c, j)
            assert all(torch.equal(i1[k][0, 0], info[k][c, j]) for k in info), (c, j)


@gpu
@pytest.mark.parametrize('src', [(2, 1, 0, 1), (1, 1, 0, 1)])               # an even and an odd site
def test_propagator(src):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 2, 2, 2)
    tol, kappa = 1e-10, 0.10
    x0 = wr.links(L, NB)
    x = dev(x0)
    lat = LatticeSU3(NB, list(L))
    S, info = lat.quark_propagator(x, kappa, source=src, tol=tol, max_iter=200, even_odd=True, mixed=True)
    Sf, finfo = lat.quark_propagator(x, kappa, source=src, tol=tol, max_iter=200, even_odd=True)
    assert S.shape == (NB, *L, 4, 3, 4, 3) and tuple(info['iters'].shape) == (NB, 12) and 'outer' in info
    assert bool(info['converged'].all()) and float(info['residual'].max()) <= tol
    bsrc = wr.point_sources(NB, L, src)
    for c in range(NB):
        m = wr.dense(x0[c:c + 1], kappa)
        smin = np.linalg.svd(m, compute_uv=False)[-1]
        inv = np.linalg.solve(m, bsrc[c].reshape(12, -1).T)                  # [12 V, 12 sources]
        assert np.linalg.norm(host(S)[c].reshape(-1, 12) - inv, axis=0).max() <= 2 * tol / smin, c
        assert np.linalg.norm(host(S - Sf)[c].reshape(-1, 12), axis=0).max() <= 4 * tol / smin, c
    S2, _ = lat.quark_propagator(x, kappa, source=src, tol=tol, max_iter=200, even_odd=True, mixed=True, inner_tol=1e-3,
                                 max_inner=100, max_outer=10)
    assert float((S2 - S).abs().max()) <= 4 * tol / smin


@gpu
@pytest.mark.parametrize('ap', [False, True])
@pytest.mark.parametrize('L', we.FD_LATTICES)
def test_force_against_restatement_differences_and_fp64(L, ap):
    """`pseudofermion_force(even_odd=True, mixed=True)` against the restatement's even-odd force (dense solves), the sum
    <p, F> against the Richardson difference of `pseudofermion_action(even_odd=True, mixed=True)`, all solves at tol =
    1e-13: within 32 x the error the restatement has with its own mixed solves at that tol (wm.CG_FD); and against the
    fp64 path, whose own figure is we.CG_FD"""
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    lat = LatticeSU3(2, list(L))
    x0, phi0, p = we.fd_inputs(L)
    kw = dict(tol=wf.FD_TOL, max_iter=4000, antiperiodic_t=ap, even_odd=True)
    phi = dev(phi0)
    F, s, info = lat.pseudofermion_force(dev(x0), phi, we.K, mixed=True, **kw)
    assert bool(info['converged'].all()) and int(info['outer'].min()) >= 2 and float(info['residual'].max()) <= wf.FD_TOL
    Fn, sn, _ = lat.pseudofermion_force_n(lat.pack(dev(x0)), dev(we.pack_half(phi0, 0)), we.K, mixed=True, **kw)
    assert torch.equal(lat.unpack(Fn), F) and torch.equal(sn, s)
    assert wilson_gpu_util.antihermitian_bits(host(Fn))
    F64, s64, _ = lat.pseudofermion_force(dev(x0), phi, we.K, **kw)
    Fw = we.fermion_force(x0, phi0, we.K, ap)
    want = wf.pair(p, host(F))
    assert np.abs(host(F) - Fw).max() <= 32 * wm.CG_FD * np.abs(Fw).max()
    assert float((F - F64).abs().max()) <= 32 * (wm.CG_FD + we.CG_FD) * np.abs(Fw).max()
    assert np.abs(host(s) - we.fermion_action(x0, phi0, we.K, ap)).max() <= 1e-10 * host(s).max()
    assert float(((s - s64).abs() / s64).max()) <= 32 * (wm.CG_S0 + we.CG_S0) + 2 * wr.norm_bound(2 * int(np.prod(L)) // 2)

    def action(xx):
        sf, i = lat.pseudofermion_action(dev(xx), phi, we.K, mixed=True, **kw)
        assert bool(i['converged'].all())
        return host(sf)
    d, d1, d2 = wf.richardson(x0, phi0, p, we.K, ap, h=1e-3, action=action)
    rel = np.abs(d - want) / np.abs(want)
    ratio = (d1 - want) / (d2 - want)
    print(f'{L} ap {ap}: relative {rel}, bound {32 * wm.CG_FD:.3g}, ratio of the raw differences {ratio}')
    assert (rel <= 32 * wm.CG_FD).all(), rel
    assert ((ratio > 3.5) & (ratio < 4.5)).all(), ratio


_hmc = functools.partial(wilson_gpu_util._hmc, cls='WilsonHMCMixed')
_hmc64 = functools.partial(wilson_gpu_util._hmc, cls='WilsonHMCEvenOdd')
_native = functools.partial(wilson_gpu_util._native, half=True)


@gpu
@pytest.mark.parametrize('L', wf.TRAJ_LATTICES)
def test_trajectory_against_restatement_and_even_odd(L):
    """`leapfrog_n` and `hamiltonian_n` of `WilsonHMCMixed` against the restatement's even-odd trajectory with dense solves
    (within 32 x wm.CG_TRAJ) and against `WilsonHMCEvenOdd` (whose own distance is we.CG_TRAJ: the two add); then one
    `trajectory` of each from the same generator: the same draws, the same accept decisions, dH within the same bound"""
    from l2hmc import _ops as ops
    x, v, phi, s0 = we.traj_inputs(L)
    x1w, v1w, dhw = we.delta_h(x, v, phi, **wf.TRAJ)
    tols = dict(tol_md=wf.TRAJ_TOL_MD, tol_h=wf.TRAJ_TOL_H)
    lat, hmc = _hmc(L, **tols)
    _, hmc64 = _hmc64(L, **tols)
    xn, vn, pn = _native(x, v, phi)
    keep = [t.clone() for t in (xn, vn, pn)]
    x1, v1, info = hmc.leapfrog_n(xn, vn, pn)
    x1r, v1r, _ = hmc64.leapfrog_n(xn, vn, pn)
    assert all(torch.equal(a, b) for a, b in zip((xn, vn, pn), keep))
    assert info['unconverged'] == 0 and info['cg_iters'].shape == (wf.TRAJ['nleapfrog'] + 1, 2, 1)
    dh = host(hmc.hamiltonian_n(x1, v1, pn) - hmc.hamiltonian_n(xn, vn, pn))
    dhr = host(hmc64.hamiltonian_n(x1r, v1r, pn) - hmc64.hamiltonian_n(xn, vn, pn))
    got = {'x': np.abs(host(ops.su3_unpack(x1, L)) - x1w).max(), 'v': np.abs(host(ops.su3_unpack(v1, L)) - v1w).max(),
           'dH': np.abs(dh - dhw).max()}
    both = {'x': float((x1 - x1r).abs().max()), 'v': float((v1 - v1r).abs().max()), 'dH': np.abs(dh - dhr).max()}
    print(L, {k: f'{got[k] / (32 * wm.CG_TRAJ[k]):.3g} of the bound' for k in got}, 'against even-odd', both, 'dH', dh)
    for k in got:
        assert got[k] <= 32 * wm.CG_TRAJ[k], (k, got[k])
        assert both[k] <= 32 * (wm.CG_TRAJ[k] + we.CG_TRAJ[k]), (k, both[k])

    def run(h):
        g = torch.Generator(device='cuda')
        g.manual_seed(11)
        return h.trajectory_n(xn, generator=g)
    xo, m = run(hmc)
    xor, mr = run(hmc64)
    assert sorted(m) == sorted(mr) and m['unconverged'] == 0 and m['cg_iters_md']['max'] > 0
    assert torch.equal(m['acc_mask'], mr['acc_mask'])
    assert float((m['dH'] - mr['dH']).abs().max()) <= 32 * (wm.CG_TRAJ['dH'] + we.CG_TRAJ['dH'])
    assert float((xo - xor).abs().max()) <= 32 * (wm.CG_TRAJ['x'] + we.CG_TRAJ['x'])


@gpu
def test_reversibility_and_step_size_scaling():
    """(4, 4, 4, 4), the bounds of the even-odd test: leapfrog, momentum flip, leapfrog returns links and momentum within
    1e-9 at tol_md = 1e-12, and dH(0.05, 8) / dH(0.025, 16) lies in (3.5, 4.5)"""
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
