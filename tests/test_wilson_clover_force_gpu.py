"""GPU tier of the dynamical clover quarks: the two kernels of csrc/su3_clover_force.hip against the restatement
tests/wilson_clover_force_restatement.py (held against finite differences on the CPU by test_wilson_clover_force_host.py),
the public path `clover_pseudofermion_force` / `clover_pseudofermion_action` against finite differences and against the
unimproved even-odd path at c_sw = 0, and `WilsonCloverHMC` against the restatement's trajectory.  Tolerances: 32 x the
extended-precision yardsticks for a single launch (wcf.TOL_G, wcf.TOL_F), 32 x the restatement's own CG-against-dense
distances (wcf.CG_FD, wcf.CG_TRAJ) where a CG stands against a dense solve."""
import functools

import numpy as np
import pytest
import torch

import wilson_clover_force_restatement as wcf
import wilson_clover_restatement as wc
import wilson_eo_restatement as we
import wilson_force_restatement as wf
import wilson_gpu_util
import wilson_restatement as wr
from wilson_gpu_util import antihermitian_bits, dev, host

gpu = pytest.mark.gpu
NB = wcf.NB
COEF = -0.05
KINDS = {1: ('hot', 1.769), 2: ('smooth', 1.0)}                              # npf -> input, c_sw


@functools.lru_cache(maxsize=None)
def reference(L, npf):
    """the inputs of one kernel case and the restatement's G, force, and the force of either term alone"""
    kind, c_sw = KINDS[npf]
    x, X, Y, ainv = wcf.force_inputs(kind, L, c_sw, NB, npf)
    kc = wc.KAPPA * c_sw
    return (x, X, Y, ainv, wf.momentum(L, NB), kc, wcf.pack_g(wcf.g_field(X, Y, ainv, kc, npf, L)),
            wcf.clover_force(x, X, Y, ainv, wc.KAPPA, c_sw, npf), wcf.clover_force(x, None, None, ainv, wc.KAPPA, c_sw, npf),
            wcf.clover_force(x, X, Y, None, wc.KAPPA, c_sw, 0.0))


@gpu
@pytest.mark.parametrize('npf', [1, 2])
@pytest.mark.parametrize('L', we.EO_GPU_LATTICES)
def test_kernels_against_restatement(L, npf):
    from l2hmc import _ops as ops
    from l2hmc import native
    x, X, Y, ainv, v, kc, want_g, want, want_det, want_pf = reference(L, npf)
    V = int(np.prod(L))
    xn, vn = ops.su3_pack(dev(x)), ops.su3_pack(dev(v))
    Xn, Yn = ops.su3_spinor_pack(dev(X)), ops.su3_spinor_pack(dev(Y))
    ci = dev(wc.pack_blocks(ainv))
    keep = [t.clone() for t in (xn, vn, Xn, Yn, ci)]

    def force(**kw):
        return ops.su3_clover_force_n(xn, Xn, Yn, ci, kc, L, det_weight=npf, **kw)
    f = force()
    g = host(native._WS.buf[:NB * 54 * V * 8].view(torch.float64).reshape(NB, 6, 9, V))
    d = float(np.abs(g - want_g).max())
    print(f'{L} npf {npf}: G deviation / tolerance {d / wcf.TOL_G:.3g}')
    assert d <= wcf.TOL_G, d
    kick = force(coef=COEF, f_in=vn)
    inplace = vn.clone()
    assert force(coef=COEF, f_in=inplace, out=inplace) is inplace
    assert torch.equal(kick, inplace)
    det = ops.su3_clover_force_n(xn, None, None, ci, kc, L, det_weight=npf)
    pf = ops.su3_clover_force_n(xn, Xn, Yn, None, kc, L)
    worst = 0.0
    for name, got, w in (('force', f, want), ('kick', kick, v + COEF * want), ('determinant only', det, want_det),
                         ('pseudofermions only', pf, want_pf), ('the sum of the two', det + pf, want)):
        d = float(np.abs(host(ops.su3_unpack(got, L)) - w).max())
        worst = max(worst, d)
        assert d <= wcf.TOL_F, (name, d)
        assert name == 'the sum of the two' or antihermitian_bits(host(got)), name
    assert float((det + pf - f).abs().max()) <= wcf.TOL_F
    # the same bits on a second call, for one chain alone and under either block order
    assert torch.equal(force(), f)
    alone = ops.su3_clover_force_n(xn[1:2].contiguous(), Xn[1:2].contiguous(), Yn[1:2].contiguous(), ci[1:2].contiguous(),
                                   kc, L, det_weight=npf)
    assert torch.equal(alone[0], f[1])
    try:
        for swz in (0, 1):
            native.set_tuning('xcd_swizzle', swz)
            assert torch.equal(force(), f), swz
    finally:
        native.set_tuning('xcd_swizzle', 1)                        # the default
    for t, k in zip((xn, vn, Xn, Yn, ci), keep):
        assert torch.equal(t, k)
    print(f'{L} npf {npf}: worst force deviation / tolerance {worst / wcf.TOL_F:.3g}')


@gpu
@pytest.mark.parametrize('c_sw', wc.C_SWS)
@pytest.mark.parametrize('ap', [False, True])
def test_public_force_against_finite_differences(ap, c_sw):
    """`clover_pseudofermion_force` against the restatement's force (dense solves) and sum <p, F> against the Richardson
    difference of `clover_pseudofermion_action` on (4, 2, 2, 2), every solve at wf.FD_TOL: within 32 x the error the
    restatement has with its own CG at that tolerance (wcf.CG_FD)"""
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 2, 2, 2)
    lat = LatticeSU3(2, list(L))
    x0, phi0, p = wcf.fd_inputs('smooth', L)
    kw = dict(tol=wf.FD_TOL, max_iter=4000, antiperiodic_t=ap)
    phi = dev(phi0)
    F, s, info = lat.clover_pseudofermion_force(dev(x0), phi, wcf.KAPPA, c_sw, **kw)
    assert bool(info['converged'].all())
    Fn, sn, _ = lat.clover_pseudofermion_force_n(lat.pack(dev(x0)), dev(we.pack_half(phi0, 0)), wcf.KAPPA, c_sw, **kw)
    assert torch.equal(lat.unpack(Fn), F) and torch.equal(sn, s)
    assert antihermitian_bits(host(Fn))
    tr = wcf.Trajectory(c_sw)
    Fw = tr.fermion_force(x0, phi0, wcf.KAPPA, ap)
    assert np.abs(host(F) - Fw).max() <= 32 * wcf.CG_FD * np.abs(Fw).max()
    pfw, ldw = tr.parts(x0, phi0, wcf.KAPPA, ap)
    assert np.abs(host(s) - (pfw + ldw)).max() <= 1e-10 * np.abs(pfw).max()
    # 12 V/2 pivots per chain, |log d_i| < 1 (the eigenvalues of A lie in (0.5, 2)), times the 2 npf of the action
    assert np.abs(host(info['logdet']) - ldw).max() <= 4 * wc.logdet_tol(12 * 16, 12 * 16 * 1.0)
    assert torch.equal(s, lat._sum_fields(info['action']) + info['logdet'])
    want = wf.pair(p, host(F))

    def action(xx):
        sf, i = lat.clover_pseudofermion_action(dev(xx), phi, wcf.KAPPA, c_sw, **kw)
        assert bool(i['converged'].all())
        return host(sf)
    d, d1, d2 = wf.richardson(x0, phi0, p, wcf.KAPPA, ap, h=1e-3, action=action)
    rel = np.abs(d - want) / np.abs(want)
    ratio = (d1 - want) / (d2 - want)
    print(f'c_sw {c_sw} ap {ap}: relative {rel}, bound {32 * wcf.CG_FD:.3g}, ratio of the raw differences {ratio}')
    assert (rel <= 32 * wcf.CG_FD).all(), rel
    assert ((ratio > 3.5) & (ratio < 4.5)).all(), ratio


@gpu
def test_c_sw_zero_is_the_even_odd_path():
    """at c_sw = 0 A = 1: `clover_pseudofermion_force` is `pseudofermion_force(even_odd=True)` to the launch tolerances
    of the two force kernels, and the determinant part of the action is 0"""
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 2, 2, 2)
    lat = LatticeSU3(2, list(L))
    x0, phi0, _ = wcf.fd_inputs('smooth', L)
    xn, pn = lat.pack(dev(x0)), dev(we.pack_half(phi0, 0))
    kw = dict(tol=wf.FD_TOL, max_iter=4000)
    F, s, info = lat.clover_pseudofermion_force_n(xn, pn, wcf.KAPPA, 0.0, **kw)
    Fe, se, _ = lat.pseudofermion_force_n(xn, pn, wcf.KAPPA, even_odd=True, **kw)
    d = float((F - Fe).abs().max())
    print(f'c_sw = 0: force distance {d:.3g}, bound {wf.TOL + wcf.TOL_F:.3g}')
    assert d <= wf.TOL + wcf.TOL_F
    assert not bool(info['logdet'].any())
    assert float((s - se).abs().max()) <= 1e-12 * float(se.max())
    sa, ia = lat.clover_pseudofermion_action_n(xn, pn, wcf.KAPPA, 0.0, **kw)
    assert not bool(ia['logdet'].any()) and float((sa - se).abs().max()) <= 1e-12 * float(se.max())


_hmc = functools.partial(wilson_gpu_util._hmc, cls='WilsonCloverHMC')
_native = functools.partial(wilson_gpu_util._native, half=True)


@gpu
@pytest.mark.parametrize('L', wf.TRAJ_LATTICES)
def test_trajectory_against_restatement(L):
    """`leapfrog_n` and `hamiltonian_n` of `WilsonCloverHMC` against the restatement's trajectory with dense solves:
    within 32 x the distance of the restatement's own trajectory with CG solves at the same tolerances from it"""
    from l2hmc import _ops as ops
    x, v, phi, s0 = wcf.traj_inputs(L)
    x1w, v1w, dhw = wcf.Trajectory(wcf.TRAJ_C_SW).delta_h(x, v, phi, **wf.TRAJ)
    lat, hmc = _hmc(L, c_sw=wcf.TRAJ_C_SW, tol_md=wf.TRAJ_TOL_MD, tol_h=wf.TRAJ_TOL_H)
    xn, vn, pn = _native(x, v, phi)
    keep = [t.clone() for t in (xn, vn, pn)]
    x1, v1, info = hmc.leapfrog_n(xn, vn, pn)
    assert all(torch.equal(a, b) for a, b in zip((xn, vn, pn), keep))
    assert info['unconverged'] == 0 and info['cg_iters'].shape == (wf.TRAJ['nleapfrog'] + 1, 2, 1)
    dh = host(hmc.hamiltonian_n(x1, v1, pn) - hmc.hamiltonian_n(xn, vn, pn))
    got = {'x': np.abs(host(ops.su3_unpack(x1, L)) - x1w).max(), 'v': np.abs(host(ops.su3_unpack(v1, L)) - v1w).max(),
           'dH': np.abs(dh - dhw).max()}
    print(L, {k: f'{got[k] / (32 * wcf.CG_TRAJ[k]):.3g} of the bound' for k in got}, 'dH', dh)
    for k in got:
        assert got[k] <= 32 * wcf.CG_TRAJ[k], (k, got[k])
    # the refresh's S0 is the pseudofermion part on these links; the Hamiltonian carries the determinant part besides
    sf, i = lat.clover_pseudofermion_action_n(xn, pn, wf.TRAJ['kappa'], wcf.TRAJ_C_SW, tol=wf.TRAJ_TOL_H)
    assert np.abs(host(lat._sum_fields(i['action'])) - s0).max() <= 1e-10 * s0.max()
    assert float(i['logdet'].abs().min()) > 0.0


@gpu
def test_reversibility():
    """(4, 4, 4, 4), with the bound of the even-odd test: leapfrog, momentum flip, leapfrog returns links and momentum within
    1e-9 at tol_md = 1e-12 (the solver tolerance through 18 forces, not rounding)"""
    L = (4, 4, 4, 4)
    x, v, phi, _ = wcf.traj_inputs(L)
    lat, hmc = _hmc(L, c_sw=wcf.TRAJ_C_SW, tol_md=1e-12)
    xn, vn, pn = _native(x, v, phi)
    x1, v1, info = hmc.leapfrog_n(xn, vn, pn)
    x2, v2, _ = hmc.leapfrog_n(x1, -v1, pn)
    rev = max(float((x2 - xn).abs().max()), float((v2 + vn).abs().max()))
    print(f'reversibility {rev:.3g}')
    assert info['unconverged'] == 0 and float((x1 - xn).abs().max()) > 0.1
    assert rev <= 1e-9


@gpu
def test_trajectory_seed_and_c_sw_zero():
    """a trajectory from a CPU generator is reproducible and leaves its input alone; at c_sw = 0 the trajectory is that
    of `WilsonHMCEvenOdd`: x', v' and dH within 32 x wcf.CG_TRAJ"""
    from l2hmc import _ops as ops
    L, nb = (4, 2, 2, 2), 2
    lat, hmc = _hmc(L, nb, c_sw=wcf.TRAJ_C_SW, npf=2)
    x = dev(wr.links(L, nb))

    def run(h):
        g = torch.Generator()
        g.manual_seed(11)
        return h.trajectory(x, generator=g)
    keep = x.clone()
    xo, m = run(hmc)
    xo2, m2 = run(hmc)
    assert torch.equal(x, keep)
    assert torch.equal(xo, xo2) and all(torch.equal(m[k], m2[k]) for k in ('acc', 'acc_mask', 'dH', 'plaq'))
    _, plain = wilson_gpu_util._hmc(L, nb, cls='WilsonHMCEvenOdd', npf=2)
    _, mp = run(plain)
    assert sorted(m) == sorted(mp)                                               # the same metrics
    assert m['unconverged'] == 0 and m['cg_iters_md']['mean'] > 0 and m['cg_iters_h']['max'] > 0
    assert tuple(m['dH'].shape) == (nb,) and bool(torch.isfinite(m['dH']).all())
    # c_sw = 0 against the unimproved class on the same fields
    xs, v, phi, _ = we.traj_inputs(L)
    xn, vn, pn = _native(xs, v, phi)
    _, zero = _hmc(L, nb, c_sw=0.0, tol_md=wf.TRAJ_TOL_MD, tol_h=wf.TRAJ_TOL_H)
    _, eo = wilson_gpu_util._hmc(L, nb, cls='WilsonHMCEvenOdd', tol_md=wf.TRAJ_TOL_MD, tol_h=wf.TRAJ_TOL_H)
    out = []
    for h in (zero, eo):
        x1, v1, _ = h.leapfrog_n(xn, vn, pn)
        out.append((x1, v1, h.hamiltonian_n(x1, v1, pn) - h.hamiltonian_n(xn, vn, pn)))
    got = {k: float((a - b).abs().max()) for k, a, b in zip(('x', 'v', 'dH'), *out)}
    print('c_sw = 0 against WilsonHMCEvenOdd:', got)
    for k in got:
        assert got[k] <= 32 * wcf.CG_TRAJ[k], (k, got[k])
    assert float((ops.su3_unpack(out[0][0], L) - dev(xs)).abs().max()) > 0.1


@gpu
def test_what_must_raise():
    from l2hmc import _ops as ops
    from l2hmc.dynamics.pytorch.fermion_hmc import WilsonCloverHMC
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 4, 4, 4)
    lat = LatticeSU3(2, list(L))
    x = dev(wr.links(L, 2))
    phi = dev(wr.spinors(L, 2, 1) * we.mask(L, 0))
    xn, pn = lat.pack(x), dev(we.pack_half(wr.spinors(L, 2, 1), 0))
    # odd extents
    odd = LatticeSU3(2, [3, 4, 4, 4])
    xo = dev(wr.links((3, 4, 4, 4), 2))
    po = dev(wr.spinors((3, 4, 4, 4), 2, 1))
    for fn in (odd.clover_pseudofermion_force, odd.clover_pseudofermion_action, odd.wilson_clover_solve_schur_normal):
        with pytest.raises(ValueError, match='even extents'):
            fn(xo, po, 0.12, 1.0)
    with pytest.raises(ValueError, match='even extents'):
        odd.clover_pseudofermion_refresh(xo, 0.12, 1.0)
    with pytest.raises(ValueError, match='even'):
        WilsonCloverHMC(odd, 5.5, 0.12, 1.0, 0.05, 4)
    # no autograd
    for t in (x, phi):
        g = t.clone().requires_grad_(True)
        args = (g, phi) if t is x else (x, g)
        for fn in (lat.clover_pseudofermion_force, lat.clover_pseudofermion_action, lat.wilson_clover_solve_schur_normal):
            with pytest.raises(ValueError, match='autograd'):
                fn(*args, 0.12, 1.0)
    with pytest.raises(ValueError, match='autograd'):
        lat.clover_pseudofermion_refresh(x.clone().requires_grad_(True), 0.12, 1.0)
    # a clover term of another kappa, c_sw or batch
    cl = lat.clover_term_n(xn, 0.12, 1.0)
    for kappa, c_sw in ((0.124, 1.0), (0.12, 1.769)):
        for fn in (lat.clover_pseudofermion_force_n, lat.clover_pseudofermion_action_n):
            with pytest.raises(ValueError, match='clover= must be'):
                fn(xn, pn, kappa, c_sw, clover=cl)
        with pytest.raises(ValueError, match='clover= must be'):
            lat.clover_pseudofermion_refresh_n(xn, kappa, c_sw, clover=cl)
    with pytest.raises(ValueError, match='clover= must be'):
        lat.clover_pseudofermion_force_n(xn[:1].contiguous(), pn[:1].contiguous(), 0.12, 1.0, clover=cl)
    assert bool(lat.clover_pseudofermion_force_n(xn, pn, 0.12, 1.0, clover=cl)[2]['converged'].all())
    # not positive definite: ValueError naming chain and pivot, before any solve and before any draw
    kb = wc.KAPPA
    for fn in (lat.clover_pseudofermion_force_n, lat.clover_pseudofermion_action_n, lat.wilson_clover_solve_schur_normal_n):
        with pytest.raises(ValueError, match=r'chain \d+ is not positive definite.*pivot -?\d'):
            fn(xn, pn, kb, wc.C_SW_BAD, max_iter=0)
    gen = torch.Generator()
    gen.manual_seed(5)
    state = gen.get_state()
    with pytest.raises(ValueError, match=r'chain \d+ is not positive definite.*pivot'):
        lat.clover_pseudofermion_refresh_n(xn, kb, wc.C_SW_BAD, generator=gen)
    assert torch.equal(gen.get_state(), state)
    hmc = WilsonCloverHMC(lat, 5.5, kb, wc.C_SW_BAD, 0.05, 2)
    vn = ops.su3_pack(dev(wf.momentum(L, 2)))
    with pytest.raises(ValueError, match=r'chain \d+ is not positive definite.*pivot'):
        hmc.leapfrog_n(xn, vn, pn)
    with pytest.raises(ValueError, match=r'chain \d+ is not positive definite.*pivot'):
        hmc.trajectory_n(xn, generator=gen)
