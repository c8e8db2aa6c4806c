"""GPU tests of the dynamical Wilson fermions: the pseudofermion force kernel (csrc/su3_wilson_force.hip) against the
numpy restatement tests/wilson_force_restatement.py, the CG on M^H M, the force through the whole path against finite
differences of the action, and the HMC trajectory of l2hmc/dynamics/pytorch/fermion_hmc.py.

The tolerance of a single launch is wf.TOL = 32 x the extended-precision yardstick (8e-14).  Where a CG solve stands
against a dense one the bound is 32 x the restatement's own distance between its CG and its dense solve (wf.CG_X,
wf.CG_FD, wf.CG_TRAJ, measured on the CPU; derivations in tests/wilson_force_restatement.py)."""
import functools

import numpy as np
import pytest
import torch

import wilson_force_restatement as wf
import wilson_restatement as wr
from oracle import su3 as osu3
from wilson_gpu_util import _hmc, _native, antihermitian_bits, dev, host

gpu = pytest.mark.gpu
NB = 3
COEF = -0.05


@functools.lru_cache(maxsize=None)
def reference(L, npf):
    """links, X, Y, a momentum field and the restatement's force for both boundary conditions"""
    x, X, Y = wf.force_inputs(L, NB, npf)
    return x, X, Y, wf.momentum(L, NB), [wf.force(x, X, Y, wr.KAPPA, ap) for ap in (False, True)]


@gpu
@pytest.mark.parametrize('npf', [1, 2])
@pytest.mark.parametrize('L', wr.GPU_LATTICES)
def test_kernel_against_restatement(L, npf):
    from l2hmc import _ops as ops, native
    x, X, Y, v, want = reference(L, npf)
    xn, vn = ops.su3_pack(dev(x)), ops.su3_pack(dev(v))
    Xn, Yn = ops.su3_spinor_pack(dev(X)), ops.su3_spinor_pack(dev(Y))
    keep = [t.clone() for t in (xn, Xn, Yn, vn)]
    worst = 0.0
    for ap, w in zip((False, True), want):
        f = ops.su3_wilson_force_n(xn, Xn, Yn, wr.KAPPA, L, ap, out=torch.full_like(xn, -7.0))
        kick = ops.su3_wilson_force_n(xn, Xn, Yn, wr.KAPPA, L, ap, coef=COEF, f_in=vn, out=torch.full_like(xn, -7.0))
        inplace = vn.clone()
        assert ops.su3_wilson_force_n(xn, Xn, Yn, wr.KAPPA, L, ap, coef=COEF, f_in=inplace, out=inplace) is inplace
        for name, got, ww in (('force', f, w), ('kick', kick, v + COEF * w), ('in place', inplace, v + COEF * w)):
            d = float(np.abs(host(ops.su3_unpack(got, L)) - ww).max())
            worst = max(worst, d)
            assert d <= wf.TOL, (ap, name, d)
            assert antihermitian_bits(host(got)), (ap, name)
        assert torch.equal(kick, inplace)
        # the same bits again, for chain 1 on its own, and under either block order
        assert torch.equal(ops.su3_wilson_force_n(xn, Xn, Yn, wr.KAPPA, L, ap), f)
        alone = ops.su3_wilson_force_n(xn[1:2].contiguous(), Xn[1:2].contiguous(), Yn[1:2].contiguous(), wr.KAPPA, L, ap)
        assert torch.equal(alone[0], f[1])
        try:
            for swz in (0, 1):
                native.set_tuning('xcd_swizzle', swz)
                assert torch.equal(ops.su3_wilson_force_n(xn, Xn, Yn, wr.KAPPA, L, ap), f), swz
        finally:
            native.set_tuning('xcd_swizzle', 1)                    # the default
    for t, k in zip((xn, Xn, Yn, vn), keep):
        assert torch.equal(t, k)
    print(f'{L} npf {npf}: worst deviation / tolerance {worst / wf.TOL:.3g}')


@gpu
@pytest.mark.parametrize('kappa', wr.SOLVE_KAPPAS)
@pytest.mark.parametrize('L', wr.API_LATTICES)
def test_solve_normal(L, kappa):
    from l2hmc import _ops as ops
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    lat = LatticeSU3(2, list(L))
    V = int(np.prod(L))
    x0, phi0 = wr.links(L, 2), wr.spinors(L, 2, 2)
    Xw, Yw, iw = wf.normal_cg(x0, phi0, kappa, tol=wf.SOLVE_TOL)
    x, phi = dev(x0), dev(phi0)
    xn, pn = lat.pack(x).clone(), ops.su3_spinor_pack(phi)
    keepx, keepp = xn.clone(), pn.clone()
    Xn, Yn, info = lat.wilson_solve_normal_n(xn, pn, kappa, tol=wf.SOLVE_TOL)
    assert torch.equal(xn, keepx) and torch.equal(pn, keepp)
    assert bool(info['converged'].all()) and float(info['residual'].max()) <= 2 * wf.SOLVE_TOL
    d = float(np.abs(host(ops.su3_spinor_unpack(Xn, L)) - Xw).max())
    print(f'{L} kappa {kappa}: |X - X_restatement| / bound {d / (32 * wf.CG_X):.3g}, iterations {host(info["iters"]).ravel()} '
          f'(restatement {iw["iters"].ravel()})')
    assert d <= 32 * wf.CG_X
    n2 = wr.norm2(host(ops.su3_spinor_unpack(Yn, L)))
    assert float((np.abs(host(info['action']) - n2) / n2).max()) <= wr.norm_bound(V)
    assert float(np.abs(host(ops.su3_spinor_unpack(Yn, L)) - Yw).max()) <= 32 * wf.CG_X * 4        # |M| <= 1 + 8 kappa < 4
    # the reference layout, with and without the field axis
    X2, Y2, _ = lat.wilson_solve_normal(x, phi, kappa, tol=wf.SOLVE_TOL)
    assert torch.equal(X2, ops.su3_spinor_unpack(Xn, L)) and torch.equal(Y2, ops.su3_spinor_unpack(Yn, L))
    X3, Y3, i3 = lat.wilson_solve_normal_n(xn, pn[:, 0], kappa, tol=wf.SOLVE_TOL)
    assert X3.shape == pn[:, 0].shape and torch.equal(X3, Xn[:, 0]) and torch.equal(Y3, Yn[:, 0])
    # a system's bits are the same alone and in the batch; phi = 0 gives X = 0
    Xa, Ya, ia = lat.wilson_solve_normal_n(xn[1:2].contiguous(), pn[1:2, 1:2].contiguous(), kappa, tol=wf.SOLVE_TOL)
    assert torch.equal(Xa[0, 0], Xn[1, 1]) and torch.equal(Ya[0, 0], Yn[1, 1])
    assert torch.equal(ia['action'][0, 0], info['action'][1, 1])
    pz = pn.clone()
    pz[0, 1] = 0
    Xz, Yz, iz = lat.wilson_solve_normal_n(xn, pz, kappa, tol=wf.SOLVE_TOL)
    assert not bool(Xz[0, 1].any()) and int(iz['iters'][0, 1]) == 0 and float(iz['residual'][0, 1]) == 0.0
    assert torch.equal(Xz[1], Xn[1]) and torch.equal(Xz[0, 0], Xn[0, 0])
    # never raises: too few iterations are reported
    i4 = lat.wilson_solve_normal_n(xn, pn, kappa, tol=wf.SOLVE_TOL, max_iter=3)[2]
    assert not bool(i4['converged'].any()) and bool((i4['iters'] == 3).all())
    # S_f and the force's own S_f are the sum of the fields' actions
    s, _ = lat.pseudofermion_action_n(xn, pn, kappa, tol=wf.SOLVE_TOL)
    assert torch.equal(s, info['action'][:, 0] + info['action'][:, 1])


@gpu
@pytest.mark.parametrize('ap', [False, True])
def test_force_by_finite_differences(ap):
    """sum <p, F> of `pseudofermion_force` against the Richardson difference of `pseudofermion_action`, both at tol =
    1e-13: within 32 x the error the restatement has with its own CG at that tol (wf.CG_FD; not the 1e-8 of the CPU test,
    whose solves are dense)"""
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = wf.FD_GPU_LATTICE
    lat = LatticeSU3(2, list(L))
    x0, phi0, p = wf.fd_inputs(L)
    kw = dict(tol=wf.FD_TOL, max_iter=4000, antiperiodic_t=ap)
    phi = dev(phi0)
    F, s, info = lat.pseudofermion_force(dev(x0), phi, wr.KAPPA, **kw)
    assert bool(info['converged'].all())
    want = wf.pair(p, host(F))
    assert np.abs(host(s) - wf.fermion_action(x0, phi0, wr.KAPPA, ap)).max() <= 1e-10 * host(s).max()

    def action(xx):
        sf, i = lat.pseudofermion_action(dev(xx), phi, wr.KAPPA, **kw)
        assert bool(i['converged'].all())
        return host(sf)
    d, d1, d2 = wf.richardson(x0, phi0, p, wr.KAPPA, ap, h=1e-3, action=action)
    rel = np.abs(d - want) / np.abs(want)
    ratio = (d1 - want) / (d2 - want)
    print(f'ap {ap}: relative {rel}, bound {32 * wf.CG_FD:.3g}, ratio of the raw differences {ratio}')
    assert (rel <= 32 * wf.CG_FD).all(), rel
    assert ((ratio > 3.5) & (ratio < 4.5)).all(), ratio


@gpu
@pytest.mark.parametrize('L', wf.TRAJ_LATTICES)
def test_trajectory_against_restatement(L):
    """`leapfrog_n` and `hamiltonian_n` against the restatement's trajectory with dense solves: within 32 x the distance
    of the restatement's own trajectory with CG solves at the same tolerances from it (wf.CG_TRAJ)"""
    from l2hmc import _ops as ops
    x, v, phi, s0 = wf.traj_inputs(L)
    x1w, v1w, dhw = wf.delta_h(x, v, phi, **wf.TRAJ)
    lat, hmc = _hmc(L, tol_md=wf.TRAJ_TOL_MD, tol_h=wf.TRAJ_TOL_H)
    xn, vn, pn = _native(x, v, phi)
    keep = [t.clone() for t in (xn, vn, pn)]
    x1, v1, info = hmc.leapfrog_n(xn, vn, pn)
    assert all(torch.equal(a, b) for a, b in zip((xn, vn, pn), keep))
    assert info['unconverged'] == 0 and info['cg_iters'].shape == (wf.TRAJ['nleapfrog'] + 1, 2, 1)
    dh = host(hmc.hamiltonian_n(x1, v1, pn) - hmc.hamiltonian_n(xn, vn, pn))
    got = {'x': np.abs(host(ops.su3_unpack(x1, L)) - x1w).max(), 'v': np.abs(host(ops.su3_unpack(v1, L)) - v1w).max(),
           'dH': np.abs(dh - dhw).max()}
    print(L, {k: f'{got[k] / (32 * wf.CG_TRAJ[k]):.3g} of the bound' for k in got}, 'dH', dh)
    for k in got:
        assert got[k] <= 32 * wf.CG_TRAJ[k], (k, got[k])
    # the starting S_f is the heatbath's |eta|^2
    sf, _ = lat.pseudofermion_action_n(xn, pn, wf.TRAJ['kappa'], tol=wf.TRAJ_TOL_H)
    assert np.abs(host(sf) - s0).max() <= 1e-10 * s0.max()


@gpu
def test_reversibility_and_step_size_scaling():
    """(4, 4, 4, 4): leapfrog, momentum flip, leapfrog returns links and momentum within 1e-9 at tol_md = 1e-12 -- a
    bound that follows from the solver tolerance (each of the 18 forces carries the error of a solve stopped at a
    residual of 1e-12, times the condition of M^H M and the size of the force), not from rounding, which is why it is
    not the 1e-13 of the restatement's dense solves; and dH(0.05, 8) / dH(0.025, 16) lies in (3.5, 4.5)."""
    L = (4, 4, 4, 4)
    x, v, phi, _ = wf.traj_inputs(L)
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
    from l2hmc import _ops as ops
    L, nb = (4, 2, 2, 2), 4
    lat, hmc = _hmc(L, nb, npf=2)
    x = dev(wr.links(L, 3)[[0, 1, 2, 0]])

    def run(h, fn='trajectory'):
        g = torch.Generator(device='cuda')
        g.manual_seed(11)
        return getattr(h, fn)(x, *((2,) if fn == 'thermalize' else ()), generator=g)
    keep = x.clone()
    xo, m = run(hmc)
    xo2, m2 = run(hmc)
    assert torch.equal(x, keep)
    assert torch.equal(xo, xo2) and all(torch.equal(m[k], m2[k]) for k in ('acc', 'acc_mask', 'dH', 'plaq'))
    assert m['unconverged'] == 0 and m['cg_iters_md']['max'] >= m['cg_iters_md']['mean'] > 0 and m['cg_iters_h']['max'] > 0
    assert tuple(m['dH'].shape) == (nb,) and bool(torch.isfinite(m['dH']).all())
    assert np.allclose(host(m['plaq']), osu3.plaqs(host(xo)), atol=1e-12)
    # a step far too large: every chain is rejected and comes back bit for bit; accepted chains moved
    _, wild = _hmc(L, nb, npf=2, eps=0.6, nleapfrog=3)
    xr, mr = run(wild)
    for xx, mm in ((xo, m), (xr, mr)):
        for c in range(nb):
            assert torch.equal(xx[c], x[c]) == (float(mm['acc_mask'][c]) == 0.0), c
    assert float(mr['acc_mask'].sum()) == 0.0 and float(mr['dH'].min()) > 10.0
    assert float(m['acc_mask'].sum()) > 0.0
    xt, hist = run(hmc, 'thermalize')
    assert len(hist) == 2 and torch.equal(hist[0]['dH'], m['dH']) and xt.shape == x.shape
    # S0 of the refresh is the action of the same phi, within the solve's tolerance
    g = torch.Generator(device='cuda')
    g.manual_seed(3)
    xn = lat.pack(x)
    phi, s0 = lat.pseudofermion_refresh_n(xn, 0.12, 2, g)
    assert phi.shape == (nb, 2, 12, 32)
    sf, info = lat.pseudofermion_action_n(xn, phi, 0.12, tol=1e-10)
    assert float(((sf - s0).abs() / s0).max()) <= 1e-10
    assert abs(float(s0.mean()) / (2 * 12 * 32) - 1.0) < 0.2                  # <|eta|^2> = 1 per complex component
    # a CPU generator gives the same field on any device order of calls
    gc = torch.Generator()
    gc.manual_seed(3)
    p1, _ = lat.pseudofermion_refresh_n(xn, 0.12, 2, gc)
    gc.manual_seed(3)
    assert torch.equal(p1, lat.pseudofermion_refresh_n(xn, 0.12, 2, gc)[0])


@gpu
def test_kappa_zero():
    """kappa = 0: M = 1, the fermions decouple: the fermion kick leaves the momentum the same bits, S_f = |phi|^2, and the
    leapfrog is the pure-gauge one"""
    from l2hmc import _ops as ops
    L = (4, 2, 2, 2)
    x, v, phi, _ = wf.traj_inputs(L)
    lat, hmc = _hmc(L, kappa=0.0)
    xn, vn, pn = _native(x, v, phi)
    X, Y, info = lat.wilson_solve_normal_n(xn, pn, 0.0)
    assert torch.equal(ops.su3_wilson_force_n(xn, X, Y, 0.0, L, coef=-0.3, f_in=vn), vn)
    sf, _ = lat.pseudofermion_action_n(xn, pn, 0.0)
    n2 = wr.norm2(phi).sum(1)
    assert np.abs(host(sf) - n2).max() <= wr.norm_bound(32) * n2.max()
    x1, v1, _ = hmc.leapfrog_n(xn, vn, pn)
    eps, n, beta = wf.TRAJ['eps'], wf.TRAJ['nleapfrog'], wf.TRAJ['beta']
    xg, vg = xn.clone(), vn.clone()
    ops.su3_force_kick_n(xg, beta, -0.5 * eps, vg, L)
    for k in range(n):
        xg = ops.su3_expm_mul_n(xg, vg, eps)
        ops.su3_force_kick_n(xg, beta, -(1.0 if k + 1 < n else 0.5) * eps, vg, L)
    assert float((x1 - xg).abs().max()) <= 1e-14 and float((v1 - vg).abs().max()) <= 1e-14
