"""GPU tests of the SU(3) gauge-fixing kernels (csrc/su3_gaugefix.hip) and of what is built on them: single launches
against the numpy restatement tests/gaugefix_restatement.py, and the public interface of LatticeSU3 by what gauge fixing
must do whatever the restatement says: converge, raise the functional, leave gauge-invariant quantities alone, undo a
pure gauge, treat the chains of a batch independently."""
import functools

import numpy as np
import pytest
import torch

import gaugefix_restatement as gf
from native_layout import pack_g, unpack_g

gpu = pytest.mark.gpu
NB = 3
# x + mu == x - mu; V/2 = 48: a partial wavefront; V/2 = 256: whole blocks; V/2 = 320: several blocks, the last partial
LATTICES = [(2, 2, 2, 2), (4, 2, 6, 2), (2, 4, 2, 6), (4, 4, 4, 8), (4, 4, 4, 10)]
OMEGAS = [1.0, 1.7]


@functools.lru_cache(maxsize=None)
def reference(L):
    """links, a transformation, and the restatement's answers for every (mask, omega, parity), computed once"""
    rng = np.random.default_rng(2000 + LATTICES.index(L))
    x = gf.random_links(rng, NB, L)
    g0 = gf.random_su3(rng, (NB, *L))
    sweeps = {(m, om, p): gf.half_sweep(x, m, p, om) for m in gf.MASKS for om in OMEGAS for p in (0, 1)}
    return x, g0, sweeps, {m: gf.condition(x, m) for m in gf.MASKS}, gf.apply(x, g0)


@functools.lru_cache(maxsize=None)
def smooth(L):
    return gf.smooth_links(np.random.default_rng(3000 + sum(L)), NB, L, 0.3)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@gpu
@pytest.mark.parametrize('L', LATTICES)
def test_kernels_against_restatement(L):
    from l2hmc import _ops as ops
    x, g0, sweeps, conds, applied = reference(L)
    xn0, gn0 = ops.su3_pack(dev(x)), dev(pack_g(g0))
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device='cuda')
    worst = [0.0, 0.0, 0.0, 0.0, 0.0]
    for mask in gf.MASKS:
        for omega in OMEGAS:
            for parity in (0, 1):
                wx, wg = sweeps[mask, omega, parity]
                for with_g in (False, True):
                    xn, gn = xn0.clone(), gn0.clone()
                    ops.su3_gaugefix_sweep_(xn, parity, mask, omega, L, gn if with_g else None, active)
                    got = host(ops.su3_unpack(xn, L))
                    assert np.array_equal(got[1], x[1]) and torch.equal(gn[1], gn0[1])       # the inactive chain
                    dx = float(np.abs(got[0::2] - wx[0::2]).max())
                    assert dx <= 1e-11, (mask, omega, parity, dx)
                    worst[0] = max(worst[0], dx)
                    if with_g:
                        dg = float(np.abs(unpack_g(host(gn), L)[0::2] - (wg @ g0)[0::2]).max())
                        assert dg <= 1e-11, (mask, omega, parity, dg)
                        worst[1] = max(worst[1], dg)
                    else:
                        assert torch.equal(gn, gn0)
        c = host(ops.su3_gauge_condition_n(xn0, mask, L))
        F, theta = conds[mask]
        dF, dth = float(np.abs(c[:, 0] - F).max()), float(np.abs(c[:, 1] / theta - 1.0).max())
        assert dF <= 1e-12 and dth <= 1e-12, (mask, dF, dth)
        worst[2:4] = [max(worst[2], dF), max(worst[3], dth)]
    # no active array: every chain moves
    xn = xn0.clone()
    ops.su3_gaugefix_sweep_(xn, 1, 13, 1.7, L)
    assert np.abs(host(ops.su3_unpack(xn, L)) - sweeps[13, 1.7, 1][0]).max() <= 1e-11
    worst[4] = float(np.abs(host(ops.su3_unpack(ops.su3_gauge_apply_n(xn0, gn0, L), L)) - applied).max())
    assert worst[4] <= 1e-12
    print(f'{L}: worst |dU| / 1e-11 = {worst[0] / 1e-11:.3g}, |dG| / 1e-11 = {worst[1] / 1e-11:.3g}, |dF| / 1e-12 = '
          f'{worst[2] / 1e-12:.3g}, |dtheta / theta| / 1e-12 = {worst[3] / 1e-12:.3g}, apply / 1e-12 = '
          f'{worst[4] / 1e-12:.3g}')


@gpu
@pytest.mark.parametrize('gauge,time_dir', [('landau', 0), ('coulomb', 1)])
@pytest.mark.parametrize('L', [(4, 4, 4, 4), (4, 2, 6, 2)])
def test_public_interface(L, gauge, time_dir):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    lat = LatticeSU3(NB, list(L))
    x = dev(smooth(L))
    keep = x.clone()
    tol = 1e-13
    y, info = lat.gauge_fix(x, gauge=gauge, time_dir=time_dir, tol=tol, max_sweeps=400)
    assert torch.equal(x, keep) and y.shape == x.shape
    print(f'{L} {gauge}: sweeps {host(info["sweeps"])}, theta {host(info["theta"])}, F {host(info["functional0"])} -> '
          f'{host(info["functional"])}')
    assert bool(info['converged'].all()) and info['converged'].dtype == torch.bool
    for k in ('theta', 'functional', 'sweeps', 'converged', 'theta0', 'functional0'):
        assert tuple(info[k].shape) == (NB,), k
    assert 'g' not in info
    c = lat.gauge_condition(y, gauge=gauge, time_dir=time_dir)
    assert float(c.theta.max()) <= tol
    assert torch.equal(c.theta, info['theta']) and torch.equal(c.F, info['functional'])
    assert bool((info['functional'] >= info['functional0']).all())
    assert bool((info['sweeps'] > 0).all()) and bool((info['sweeps'] <= 400).all())
    c0 = lat.gauge_condition(x, gauge=gauge, time_dir=time_dir)
    assert torch.equal(c0.theta, info['theta0']) and torch.equal(c0.F, info['functional0'])
    # gauge-invariant quantities
    assert float((lat.plaqs(y) - lat.plaqs(x)).abs().max()) <= 1e-12
    assert float((lat.wilson_loop_table(y, 2, 2) - lat.wilson_loop_table(x, 2, 2)).abs().max()) <= 1e-12
    assert float((lat.polyakov(y).abs() - lat.polyakov(x).abs()).abs().max()) <= 1e-12
    # the transformation that did it
    z, info = lat.gauge_fix(x, gauge=gauge, time_dir=time_dir, tol=tol, max_sweeps=400, reunitarize=False,
                            return_transform=True)
    assert tuple(info['g'].shape) == (NB, *L, 3, 3)
    assert float((lat.gauge_transform(x, info['g']) - z).abs().max()) <= 1e-11
    assert float((z - y).abs().max()) <= 1e-12                 # the projection at the end moves rounding only
    gh = host(info['g'])
    assert np.abs(gh.conj().swapaxes(-1, -2) @ gh - np.eye(3)).max() <= 1e-12


@gpu
@pytest.mark.parametrize('omega', OMEGAS)
def test_functional_is_monotone(omega):
    from l2hmc import _ops as ops
    L = (4, 2, 6, 2)
    xn0 = ops.su3_pack(dev(reference(L)[0]))
    for mask in (15, 13):
        xn = xn0.clone()
        f = host(ops.su3_gauge_condition_n(xn, mask, L))[:, 0]
        f0, drop = f, 0.0
        for _ in range(20):
            for parity in (0, 1):
                ops.su3_gaugefix_sweep_(xn, parity, mask, omega, L)
                f1 = host(ops.su3_gauge_condition_n(xn, mask, L))[:, 0]
                drop = max(drop, float((f - f1).max()))
                assert (f1 - f >= -1e-14).all(), (mask, f, f1)
                f = f1
        print(f'omega {omega} mask {mask}: F {f0} -> {f}, largest decrease {drop:.3g}')
        assert (f > f0 + 0.2).all()


@gpu
@pytest.mark.parametrize('omega', [1.0, None])
def test_pure_gauge_comes_back(omega):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 4, 4, 4)
    lat = LatticeSU3(NB, list(L))
    x = dev(gf.pure_gauge(np.random.default_rng(9), NB, L))              # a rough (Haar-like) transformation
    assert float(lat.gauge_condition(x).F.abs().max()) < 0.2
    y, info = lat.gauge_fix(x, tol=1e-26, max_sweeps=400, omega=omega)
    one = torch.eye(3, dtype=torch.complex128, device='cuda')
    print(f'pure gauge, omega {omega}: 1 - F = {host(1.0 - info["functional"])}, max |U - 1| = '
          f'{float((y - one).abs().max()):.3g}, sweeps {host(info["sweeps"])}')
    assert float((1.0 - info['functional']).max()) <= 1e-12
    assert float((y - one).abs().max()) <= 1e-6


@gpu
def test_chains_are_independent_and_fixing_is_idempotent():
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 4, 4, 4)
    rng = np.random.default_rng(12)
    # chains 0 and 2 are closer to / further from their maximum than chain 1: they freeze at other checks
    x = dev(np.concatenate([gf.smooth_links(rng, 1, L, amp) for amp in (0.02, 0.3, 0.8)]))
    kw = dict(tol=1e-13, max_sweeps=2000, check_every=5, reunitarize=False)
    y, info = LatticeSU3(3, list(L)).gauge_fix(x, **kw)
    y1, info1 = LatticeSU3(1, list(L)).gauge_fix(x[1:2].clone(), **kw)
    s = host(info['sweeps'])
    print(f'sweeps together {s}, chain 1 alone {host(info1["sweeps"])}')
    assert bool(info["converged"].all()) and s[0] != s[1] and s[2] != s[1]
    assert torch.equal(y[1:2], y1) and int(info1['sweeps'][0]) == int(s[1])
    assert torch.equal(info['theta'][1:2], info1['theta'])
    # fixing the fixed field: no sweep, the same bits
    z, info2 = LatticeSU3(3, list(L)).gauge_fix(y, **kw)
    assert torch.equal(z, y) and int(info2['sweeps'].abs().sum()) == 0 and bool(info2['converged'].all())
    assert torch.equal(info2['theta'], info['theta']) and torch.equal(info2['theta0'], info['theta'])


@gpu
def test_refusals_and_limits():
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 2, 6, 2)
    lat = LatticeSU3(NB, list(L))
    x = dev(reference(L)[0])
    with pytest.raises(ValueError):
        lat.gauge_fix(x.clone().requires_grad_(True))
    odd = LatticeSU3(1, [2, 3, 2, 2])
    xo = odd.random().cuda()
    with pytest.raises(ValueError):
        odd.gauge_fix(xo)
    # the condition and a transformation take odd extents
    c = odd.gauge_condition(xo, 'coulomb', 3)
    F, theta = gf.condition(host(xo), 7)
    assert abs(float(c.F[0]) - F[0]) <= 1e-12 and abs(float(c.theta[0]) / theta[0] - 1.0) <= 1e-12
    g = gf.random_su3(np.random.default_rng(4), (1, 2, 3, 2, 2))
    assert np.abs(host(odd.gauge_transform(xo, dev(g))) - gf.apply(host(xo), g)).max() <= 1e-12
    # a hot field does not get there in 3 sweeps: nothing raises, the count is what was done
    y, info = lat.gauge_fix(x, max_sweeps=3, check_every=2)
    assert not bool(info['converged'].any()) and host(info['sweeps']).tolist() == [3, 3, 3]
    assert bool((info['functional'] > info['functional0']).all())
    y0, info0 = lat.gauge_fix(x, max_sweeps=0, reunitarize=False)
    assert torch.equal(y0, x) and not bool(info0['converged'].any())
