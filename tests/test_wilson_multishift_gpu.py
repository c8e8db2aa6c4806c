"""GPU tests of the multi-shift CG and the one-flavour RHMC: the three kernels of csrc/su3_spinor_mshift.hip against their
numpy restatements (tests/wilson_multishift_restatement.py), the solver against dense solves, the rational pseudofermion's
public paths against the restatement and finite differences, and the trajectory of `WilsonRHMC`.

Tolerances.  A kernel output is a short chain of fma on operands of order one: one rounding (2^-52) per operation of the
sum of the sizes of its terms, as in tests/test_wilson_multishift_emu.py.  Where a CG solve stands against a dense one the
bound is 32 x the restatement's own distance between its multi-shift CG and its dense solves (ms.CG_X, ms.CG_S0, ms.CG_FD,
ms.CG_TRAJ, measured on the CPU: profiles/su3_wilson_multishift/restatement_measure.txt); a test of a sum adds the bound
of the sum's own order (wr.norm_bound)."""
import functools

import numpy as np
import pytest
import torch

import hmc_golden
import wilson_clover_restatement as wc
import wilson_eo_restatement as we
import wilson_force_restatement as wf
import wilson_multishift_restatement as ms
import wilson_restatement as wr
import wilson_gpu_util
from wilson_gpu_util import dev, host

gpu = pytest.mark.gpu
ULP = 2.0 ** -52
_native = functools.partial(wilson_gpu_util._native, half=True)


def shifted_native(X, L):
    """[nb, nrhs, ns, T, X, Y, Z, 4, 3] (zero on the odd sites) -> the native [nb, nrhs, ns, 12, V/2]"""
    nb, nrhs, ns = X.shape[:3]
    return we.pack_half(X.reshape(nb, nrhs * ns, *X.shape[3:]), 0).reshape(nb, nrhs, ns, 12, -1)


# ------------------------------------------------------------------ the kernels
@gpu
@pytest.mark.parametrize('ns', ms.KERNEL_NS)
@pytest.mark.parametrize('L', we.EO_GPU_LATTICES)
def test_kernels_against_restatement(L, ns):
    from l2hmc import _ops as ops
    from l2hmc import native
    V = int(np.prod(L)) // 2
    f, c, live = ms.kernel_inputs(V, ns)
    xw, pw, bw = ms.mshift_update(f['x'], f['ps'], f['p'], f['r'], c['a'], c['b'], c['zeta'], c['beta'], live)
    rw, _ = ms.axmy_norm(f['r'], f['z'], c['alpha'])
    lw = ms.lincomb(f['x'], c['w'])
    F = {k: dev(v) for k, v in f.items()}
    Cd = {k: dev(v) for k, v in c.items()}
    lv = dev(live)
    keep = [t.clone() for t in (*F.values(), *Cd.values(), lv)]

    def run(sl=slice(None)):
        x, ps, p, r = (F[k][sl].clone() for k in ('x', 'ps', 'p', 'r'))
        ops.su3_spinor_mshift_update_(x, ps, p, F['r'][sl].contiguous(), *(Cd[k][sl].contiguous() for k in ('a', 'b', 'zeta', 'beta')),
                                      lv[sl].contiguous())
        part = ops.su3_spinor_axmy_norm_(r, F['z'][sl].contiguous(), Cd['alpha'][sl].contiguous())
        lin = ops.su3_spinor_lincomb(F['x'][sl].contiguous(), Cd['w'][sl].contiguous())
        return x, ps, p, r, part, lin
    got = run()
    x, ps, p, r2, part, lin = (host(t) for t in got)
    e = lambda v: np.abs(v)[..., None, None]                                  # noqa: E731
    assert (np.abs(x - xw) <= ULP * (np.abs(f['x']) + e(c['a']) * np.abs(f['ps']))).all()
    assert (np.abs(ps - pw) <= 2 * ULP * (e(c['zeta']) * np.abs(f['r'])[:, :, None] + e(c['b']) * np.abs(f['ps']))).all()
    assert (np.abs(p - bw) <= ULP * (np.abs(f['r']) + e(c['beta']) * np.abs(f['p']))).all()
    assert (np.abs(r2 - rw) <= ULP * (np.abs(f['r']) + e(c['alpha']) * np.abs(f['z']))).all()
    size = sum(e(c['w'][:, :, k]) * np.abs(f['x'][:, :, k]) for k in range(ns))
    assert (np.abs(lin - lw) <= ns * ULP * size).all()
    mine = (r2.real ** 2 + r2.imag ** 2).sum((-2, -1))
    assert part.shape == (2, 2, -(-V // 256))
    assert (np.abs(part.sum(-1) - mine) <= wr.norm_bound(V) * mine).all()
    # one shift frozen: its fields keep their bits, the others moved
    dead = live == 0
    assert dead.any() and np.array_equal(x[dead], f['x'][dead]) and np.array_equal(ps[dead], f['ps'][dead])
    alive = (live != 0) & (c['a'] != 0)
    assert not np.array_equal(x[alive], f['x'][alive])
    # the same bits on a second call, for one chain alone, and under either block order
    assert all(torch.equal(a, b) for a, b in zip(got, run()))
    assert all(torch.equal(a[1:], b) for a, b in zip(got, run(slice(1, 2))))
    try:
        for swz in (0, 1):
            native.set_tuning('xcd_swizzle', swz)
            assert all(torch.equal(a, b) for a, b in zip(got, run())), swz
    finally:
        native.set_tuning('xcd_swizzle', 1)                                      # the default
    assert all(torch.equal(a, b) for a, b in zip((*F.values(), *Cd.values(), lv), keep))      # no input is written


# ------------------------------------------------------------------ the solver
@gpu
@pytest.mark.parametrize('L', [(4, 4, 4, 4), (4, 2, 6, 2)])
def test_solver_against_dense_solves(L):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    lat = LatticeSU3(2, list(L))
    x, phi = wr.links(L, 2), wr.spinors(L, 2, 2) * we.mask(L, 0)
    phi[1, 1] = 0.0
    want = ms.dense_shifted(x, phi, ms.K, ms.SHIFTS)
    X, info = lat.wilson_solve_multishift(dev(x), dev(phi), ms.K, ms.SHIFTS, tol=ms.SOLVE_TOL)
    assert X.shape == (2, 2, len(ms.SHIFTS), *L, 4, 3)
    d = float(np.abs(host(X) - want).max())
    print(L, f'max |X - X_dense| = {d:.3g}, bound {32 * ms.CG_X:.3g}', host(info['iters']).tolist(),
          host(info['shift_iters']).tolist(), f"residual {float(info['residual'].max()):.3g}")
    assert d <= 32 * ms.CG_X
    assert bool(info['converged'].all()) and float(info['residual'].max()) <= ms.SOLVE_TOL
    assert info['residual'].shape == info['shift_iters'].shape == (2, 2, len(ms.SHIFTS))
    si, it = host(info['shift_iters']), host(info['iters'])
    assert (si <= it[..., None]).all() and (np.diff(si, axis=-1) <= 0).all() and (si[:, :, -1] < it)[it > 0].all()
    assert not host(X)[1, 1].any() and it[1, 1] == 0 and (si[1, 1] == 0).all()
    # the native entry: the same numbers in the half layout; a system's bits do not depend on the batch; freezing off
    xn, pe = lat.pack(dev(x)), dev(we.pack_half(phi, 0))
    Xn, _ = lat.wilson_solve_multishift_n(xn, pe, ms.K, ms.SHIFTS, tol=ms.SOLVE_TOL)
    assert np.array_equal(host(Xn), shifted_native(host(X), L))
    alone, ia = lat.wilson_solve_multishift_n(xn[1:], pe[1:, :1], ms.K, ms.SHIFTS, tol=ms.SOLVE_TOL)
    assert torch.equal(alone[0, 0], Xn[1, 0]) and torch.equal(ia['shift_iters'][0, 0], info['shift_iters'][1, 0])
    Xf, inf = lat.wilson_solve_multishift_n(xn, pe, ms.K, ms.SHIFTS, tol=ms.SOLVE_TOL, freeze=False)
    assert np.abs(shifted_native(want, L) - host(Xf)).max() <= 32 * ms.CG_X
    assert torch.equal(inf['shift_iters'], inf['iters'][..., None].expand(-1, -1, len(ms.SHIFTS)))
    single, i1 = lat.wilson_solve_multishift_n(xn, pe[:, 0], ms.K, ms.SHIFTS, tol=ms.SOLVE_TOL)
    assert torch.equal(single, Xn[:, 0]) and i1['residual'].shape == (2, len(ms.SHIFTS))


@gpu
def test_solver_residuals_on_a_large_lattice():
    """(4, 4, 4, 10): too large for a dense solve; the recomputed residuals meet tol, Zolotarev shifts over four decades"""
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 4, 4, 10)
    lat = LatticeSU3(2, list(L))
    xn, pe = lat.pack(dev(wr.links(L, 2))), dev(we.pack_half(wr.spinors(L, 2, 2) * we.mask(L, 0), 0))
    shifts = ms.rational(10).poles
    X, info = lat.wilson_solve_multishift_n(xn, pe, 0.12, shifts, tol=1e-10)
    print(host(info['iters']).tolist(), host(info['shift_iters'])[0, 0].tolist(), f"{float(info['residual'].max()):.3g}")
    assert bool(info['converged'].all()) and float(info['residual'].max()) <= 1e-10
    assert int(info['shift_iters'].min()) < int(info['iters'].max())               # some shift froze early
    short, i2 = lat.wilson_solve_multishift_n(xn, pe, 0.12, shifts, tol=1e-10, max_iter=10)
    assert not bool(i2['converged'].any()) and int(i2['iters'].min()) == 10 and float(i2['residual'].max()) > 1e-10


@gpu
def test_zero_shift_is_the_normal_solve():
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 4, 4, 4)
    lat = LatticeSU3(2, list(L))
    x, phi = wr.links(L, 2), wr.spinors(L, 2, 2) * we.mask(L, 0)
    xn, pe = lat.pack(dev(x)), dev(we.pack_half(phi, 0))
    keep = pe.clone()
    X, info = lat.wilson_solve_multishift_n(xn, pe, ms.K, [0.0], tol=ms.SOLVE_TOL)
    assert torch.equal(pe, keep)                                                  # ns = 1: the right-hand side is not written
    Xn, _, ninfo = lat.wilson_solve_schur_normal_n(xn, pe, ms.K, tol=ms.SOLVE_TOL)
    # both are within tol |b| / lambda_min of the solution: twice the restatement's CG distance, 32 x
    assert float((X[:, :, 0] - Xn).abs().max()) <= 2 * 32 * ms.CG_X
    assert torch.equal(info['iters'], ninfo['iters'])


@gpu
def test_solver_with_the_clover_term():
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L, c_sw = (4, 2, 6, 2), wc.C_SWS[0]
    lat = LatticeSU3(2, list(L))
    x, phi = wr.links(L, 2), wr.spinors(L, 2, 2) * we.mask(L, 0)

    def dense(xc, kappa, ap):
        a = wc.clover(xc, kappa * c_sw)
        ainv = wc.inverse(a)
        n = 12 * int(np.prod(L))
        idx = we.even_index(L)
        basis = np.eye(n, dtype=complex)[idx].reshape(1, len(idx), *L, 4, 3)
        return wc.schur_clover(xc, basis, kappa, a, ainv, False, ap).reshape(len(idx), n).T[idx]
    want = ms.dense_shifted(x, phi, ms.K, ms.SHIFTS, dense=dense)
    xn, pe = lat.pack(dev(x)), dev(we.pack_half(phi, 0))
    cl = lat.clover_term_n(xn, ms.K, c_sw)
    X, info = lat.wilson_solve_multishift_n(xn, pe, ms.K, ms.SHIFTS, tol=ms.SOLVE_TOL, clover=cl)
    d = float(np.abs(host(X) - shifted_native(want, L)).max())
    print(f'clover: max |X - X_dense| = {d:.3g}', f"residual {float(info['residual'].max()):.3g}")
    assert d <= 32 * ms.CG_X and float(info['residual'].max()) <= ms.SOLVE_TOL
    plain, _ = lat.wilson_solve_multishift_n(xn, pe, ms.K, ms.SHIFTS, tol=ms.SOLVE_TOL)
    assert float((plain - X).abs().max()) > 1e-3                                  # the clover term is in it
    with pytest.raises(ValueError, match='clover= must be'):
        lat.wilson_solve_multishift_n(xn, pe, 0.1, ms.SHIFTS, clover=cl)           # another kappa


# ------------------------------------------------------------------ the public paths of the one-flavour pseudofermion
@gpu
@pytest.mark.parametrize('L', ms.LATTICES)
def test_refresh_and_action_against_restatement(L):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    nb, kap, rat = 2, wf.TRAJ['kappa'], ms.rational()
    lat = LatticeSU3(nb, list(L))
    x = wr.links(L, nb)
    ms.assert_spectrum(x, kap, rat)
    xd = dev(x)
    xn = lat.pack(xd)
    Vh = int(np.prod(L)) // 2
    g = torch.Generator()
    g.manual_seed(5)
    phi, s0 = lat.rhmc_pseudofermion_refresh_n(xn, kap, rat, 2, g, tol=wf.TRAJ_TOL_H)
    assert phi.shape == (nb, 2, 12, Vh) and s0.shape == (nb,)
    g.manual_seed(5)
    eta = torch.view_as_complex(torch.randn((nb, 2, 12, Vh, 2), dtype=torch.float64, generator=g) * float(np.sqrt(0.5)))
    etaf = we.unpack_half(eta.numpy(), L, 0)
    phiw, s0w = ms.rat_refresh(x, etaf, kap, rat)
    # phi is linear in the Z_k, which carry the solver's error
    # (through Mhat, of norm <= 1 + 64 kappa^2 < 2, and through nu_k)
    assert np.abs(we.unpack_half(host(phi), L, 0) - phiw).max() <= 32 * ms.CG_X * (np.abs(rat.c) * (2 + rat.nu)).sum() / np.sqrt(rat.A)
    assert (np.abs(host(s0) - s0w) <= wr.norm_bound(2 * Vh) * s0w).all()
    # S_1(C eta) = |eta|^2: 32 x the restatement's CG figure plus the rounding of the sums in their own orders
    s, info = lat.rhmc_pseudofermion_action_n(xn, phi, kap, rat, tol=wf.TRAJ_TOL_H, max_iter=2000)
    assert bool(info['converged'].all()) and info['action'].shape == (nb, 2)
    bound = 32 * ms.CG_S0 + (2 + 2 * rat.n) * wr.norm_bound(2 * Vh)
    rel = float(((s - s0).abs() / s0).max())
    print(L, f'|S_1 - S0| / S0 = {rel:.3g}, bound {bound:.3g}')
    assert rel <= bound
    # against the restatement's action (dense solves) of the same field: 32 x its CG figure plus the sums' own orders
    sw = ms.rat_action(x, we.unpack_half(host(phi), L, 0), kap, rat)
    assert (np.abs(host(s) - sw) <= (32 * ms.CG_S + (2 + 2 * rat.n) * wr.norm_bound(2 * Vh)) * sw).all()
    # the reference layout: the full shape, zero on the odd sites; the same numbers
    g.manual_seed(5)
    phir, s0r = lat.rhmc_pseudofermion_refresh(xd, kap, rat, 2, g, tol=wf.TRAJ_TOL_H)
    assert phir.shape == (nb, 2, *L, 4, 3) and torch.equal(s0r, s0)
    assert np.array_equal(host(phir), we.unpack_half(host(phi), L, 0))
    sr, _ = lat.rhmc_pseudofermion_action(xd, phir, kap, rat, tol=wf.TRAJ_TOL_H, max_iter=2000)
    assert torch.equal(sr, s)
    # the spectrum helper: both estimates are Rayleigh quotients of Mhat^H Mhat, so they lie inside the true spectrum (the
    # slack 1e-9 is the inverse iteration's solver tolerance 1e-10 with a margin of 10), below the rigorous bound, and the
    # Rayleigh quotient of a power (inverse) iteration is monotone in the iteration count from the same start vector
    ev = ms.spectrum(x, kap)
    est = {}
    for iters in (3, 12):
        g.manual_seed(9)
        est[iters] = [host(t) for t in lat.schur_spectrum_n(xn, kap, iters=iters, generator=g)]
        lo, hi = est[iters]
        assert (lo >= ev.min(1) * (1 - 1e-9)).all() and (hi <= ev.max(1) * (1 + 1e-9)).all() and (lo < hi).all()
        assert (hi <= (1 + 64 * kap ** 2) ** 2).all()
    assert (est[12][0] <= est[3][0] * (1 + 1e-9)).all() and (est[12][1] >= est[3][1] * (1 - 1e-9)).all()
    print(L, 'spectrum', ev.min(1), ev.max(1), 'estimates', est[12])


@gpu
@pytest.mark.parametrize('ap', [False, True])
@pytest.mark.parametrize('L', we.FD_LATTICES)
def test_force_against_restatement_and_differences(L, ap):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    lat = LatticeSU3(2, list(L))
    rat = ms.rational()
    x0, phi0, p = ms.fd_inputs(L)
    ms.assert_spectrum(x0, ms.K, rat, ap)
    kw = dict(tol=wf.FD_TOL, max_iter=4000, antiperiodic_t=ap)
    phi = dev(phi0)
    F, info = lat.rhmc_pseudofermion_force(dev(x0), phi, ms.K, rat, **kw)
    assert F.shape == (2, 4, *L, 3, 3) and bool(info['converged'].all())
    Fn, _ = lat.rhmc_pseudofermion_force_n(lat.pack(dev(x0)), dev(we.pack_half(phi0, 0)), ms.K, rat, **kw)
    assert wilson_gpu_util.antihermitian_bits(host(Fn))
    Fw = ms.rat_force(x0, phi0, ms.K, rat, ap)
    assert np.abs(host(F) - Fw).max() <= 32 * ms.CG_FD * np.abs(Fw).max()
    want = wf.pair(p, host(F))

    def action(xx):
        s, i = lat.rhmc_pseudofermion_action(dev(xx), phi, ms.K, rat, **kw)
        assert bool(i['converged'].all())
        return host(s)
    d, d1, d2 = wf.richardson(x0, phi0, p, ms.K, ap, h=1e-3, action=action)
    rel = np.abs(d - want) / np.abs(want)
    ratio = (d1 - want) / (d2 - want)
    print(f'{L} ap {ap}: relative {rel}, bound {32 * ms.CG_FD:.3g}, ratio of the raw differences {ratio}')
    assert (rel <= 32 * ms.CG_FD).all(), rel
    assert ((ratio > 3.5) & (ratio < 4.5)).all(), ratio


# ------------------------------------------------------------------ the trajectory
def _rhmc(L, light=True, **kw):
    return wilson_gpu_util._hmc(L, cls='WilsonRHMC', rat=ms.rational(), kappa_light=ms.KAPPA_LIGHT if light else None, **kw)


@gpu
@pytest.mark.parametrize('light', [True, False])
@pytest.mark.parametrize('L', wf.TRAJ_LATTICES)
def test_leapfrog_and_hamiltonian_against_restatement(L, light):
    from l2hmc import _ops as ops
    x, v, phi_l, phi_s = ms.traj_inputs(L, light=light)
    kw = dict(wf.TRAJ, rat=ms.rational(), kappa_light=ms.KAPPA_LIGHT if light else None)
    x1w, v1w, dhw = ms.delta_h(x, v, phi_l, phi_s, **kw)
    ms.assert_spectrum(x, wf.TRAJ['kappa'], kw['rat'])
    ms.assert_spectrum(x1w, wf.TRAJ['kappa'], kw['rat'])
    lat, hmc = _rhmc(L, light, tol_md=wf.TRAJ_TOL_MD, tol_h=wf.TRAJ_TOL_H)
    xn, vn, ps = _native(x, v, phi_s)
    pn = (dev(we.pack_half(phi_l, 0)) if light else None, ps)
    keep = [t.clone() for t in (xn, vn, ps)]
    x1, v1, info = hmc.leapfrog_n(xn, vn, pn)
    assert all(torch.equal(a, b) for a, b in zip((xn, vn, ps), keep))
    assert info['unconverged'] == 0 and info['cg_iters'].shape == (wf.TRAJ['nleapfrog'] + 1, 2, 1)
    assert info['cg_iters_ms'].shape == info['cg_iters'].shape and int(info['cg_iters_ms'].min()) > 0
    dh = host(hmc.hamiltonian_n(x1, v1, pn) - hmc.hamiltonian_n(xn, vn, pn))
    got = {'x': np.abs(host(ops.su3_unpack(x1, L)) - x1w).max(), 'v': np.abs(host(ops.su3_unpack(v1, L)) - v1w).max(),
           'dH': np.abs(dh - dhw).max()}
    print(L, light, {k: f'{got[k] / (32 * ms.CG_TRAJ[k]):.3g} of the bound' for k in got}, 'dH', dh)
    for k in got:
        assert got[k] <= 32 * ms.CG_TRAJ[k], (k, got[k])


@gpu
@pytest.mark.parametrize('L', wf.TRAJ_LATTICES)
def test_trajectory_against_restatement_with_a_cpu_generator(L):
    """`WilsonRHMC.trajectory` with a CPU generator: the same draws on the host, in the documented order (momentum, light,
    strange, accept), through the restatement's heatbaths and its dense trajectory give the same dH and the same accept"""
    from l2hmc import _ops as ops
    nb, Vh = 2, int(np.prod(L)) // 2
    lat, hmc = _rhmc(L, True, tol_md=wf.TRAJ_TOL_MD, tol_h=wf.TRAJ_TOL_H)
    x = wr.links(L, nb)
    g = torch.Generator()
    g.manual_seed(17)
    xo, m = hmc.trajectory(dev(x), generator=g)
    g.manual_seed(17)
    vn = ops.su3_assemble_tah_n(torch.randn((8, nb, 4, 2 * Vh), dtype=torch.float64, generator=g).cuda())
    v = host(ops.su3_unpack(vn, L))
    etas = [we.unpack_half((torch.view_as_complex(torch.randn((nb, 1, 12, Vh, 2), dtype=torch.float64, generator=g))
                            * float(np.sqrt(0.5))).numpy(), L, 0) for _ in range(2)]
    u = torch.rand((nb,), dtype=torch.float64, generator=g).numpy()
    rat, kap = ms.rational(), wf.TRAJ['kappa']
    phi_l = we.refresh(x, etas[0], ms.KAPPA_LIGHT)[0]
    phi_s = ms.rat_refresh(x, etas[1], kap, rat)[0]
    x1w, _, dhw = ms.delta_h(x, v, phi_l, phi_s, **wf.TRAJ, rat=rat, kappa_light=ms.KAPPA_LIGHT)
    dh = host(m['dH'])
    print(L, 'dH', dh, 'restatement', dhw, m['cg_iters_md'], m['cg_iters_ms_md'], m['cg_iters_ms_h'])
    # H0 takes |eta|^2 for both actions: add the heatbath identities' figures (relative to S0 ~ 12 V/2 per field)
    s0 = sum((e.real ** 2 + e.imag ** 2).sum((1, 2, 3, 4, 5, 6, 7)) for e in etas)
    bound = 32 * ms.CG_TRAJ['dH'] + (32 * (ms.CG_S0 + we.CG_S0) + (4 + 2 * rat.n) * wr.norm_bound(2 * Vh)) * s0.max()
    assert np.abs(dh - dhw).max() <= bound, (np.abs(dh - dhw).max(), bound)
    accw = u < np.exp(np.minimum(-dhw, 0.0))
    assert np.array_equal(host(m['acc_mask']) != 0, accw)
    want = np.where(accw[:, None, None, None, None, None, None, None], x1w, x)
    assert np.abs(host(xo) - want).max() <= 32 * ms.CG_TRAJ['x']
    assert m['unconverged'] == 0 and m['cg_iters_ms_md']['max'] > 0 and m['cg_iters_ms_h']['max'] > 0
    only = _rhmc(L, False)[1]
    g.manual_seed(17)
    _, m1 = only.trajectory(dev(x), generator=g)
    assert sorted(m1) == sorted(m) and m1['cg_iters_md'] == m1['cg_iters_ms_md']


@gpu
def test_reversibility_and_step_size_scaling():
    """(4, 4, 4, 4) with the light field: leapfrog, momentum flip, leapfrog returns links and momentum within 1e-9 at tol_md
    = 1e-12 (the bound of the two-flavour test: the solver tolerance through the forces, not rounding), and dH(0.05, 8) /
    dH(0.025, 16) lies in (3.5, 4.5)"""
    from l2hmc import _ops as ops
    L, nb = (4, 4, 4, 4), 2
    lat, hmc = _rhmc(L, True, tol_md=1e-12)
    xn = lat.pack(dev(wr.links(L, nb)))
    vn = ops.su3_pack(dev(wf.momentum(L, nb, 1)))
    g = torch.Generator()
    g.manual_seed(3)
    lo, hi = lat.schur_spectrum_n(xn, wf.TRAJ['kappa'], iters=40, generator=g)
    assert float(lo.min()) > 2 * ms.RA and float(hi.max()) < ms.RB                 # the estimates, with a margin of 2
    pn, _ = hmc._refresh_n(xn, g)
    x1, v1, info = hmc.leapfrog_n(xn, vn, pn)
    x2, v2, _ = hmc.leapfrog_n(x1, -v1, pn)
    rev = max(float((x2 - xn).abs().max()), float((v2 + vn).abs().max()))
    assert info['unconverged'] == 0 and float((x1 - xn).abs().max()) > 0.1
    h0 = hmc.hamiltonian_n(xn, vn, pn)
    a = host(hmc.hamiltonian_n(x1, v1, pn) - h0)
    _, half = _rhmc(L, True, tol_md=1e-12, eps=wf.TRAJ['eps'] / 2, nleapfrog=2 * wf.TRAJ['nleapfrog'])
    x3, v3, _ = half.leapfrog_n(xn, vn, pn)
    b = host(half.hamiltonian_n(x3, v3, pn) - h0)
    print(f'reversibility {rev:.3g}; dH {a} / {b} = {a / b}')
    assert rev <= 1e-9
    assert ((a / b > 3.5) & (a / b < 4.5)).all()


@gpu
@pytest.mark.parametrize('cls', hmc_golden.CLASSES)
def test_existing_hmc_classes_give_the_bits_of_the_parent(cls):
    """One trajectory of each existing HMC class on (4, 2, 2, 2) with a CPU generator: the links, dH, the accept mask and the
    plaquette are the bits recorded from the commit before the multi-shift CG (tests/golden/fermion_hmc_parent.npz, made
    by tests/hmc_golden.py there), also after a `WilsonRHMC` trajectory has run"""
    want = np.load(hmc_golden.PATH)
    _rhmc((4, 2, 2, 2), True)[1].trajectory(dev(wr.links((4, 2, 2, 2), 2)), generator=torch.Generator().manual_seed(1))
    for key, got in hmc_golden.run(cls).items():
        w = want[f'{cls}.{key}']
        assert got.dtype == w.dtype and got.shape == w.shape and np.array_equal(got.view(np.uint8), w.view(np.uint8)), (cls, key)
