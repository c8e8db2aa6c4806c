"""GPU tests of the SU(3) smearing kernels (csrc/su3_smear.hip) and of what is built on them: single launches of each
entry point against the numpy restatement tests/smear_restatement.py, then the public interface of LatticeSU3: iterated
smearing against the iterated restatement, and what smearing must do whatever the restatement says (leave the input
alone, treat chains independently, commute with gauge transformations, keep a pure gauge trivial, feed the loop table).

Inputs are the smooth links of sm.smooth_input (the input rule: every pre-projection matrix stays far below condition
number 100; the restatement asserts it on every link).  Tolerances are sm.TOL = 32 x the measured projection yardstick
(about 1.8e-13, derivation in tests/smear_restatement.py and profiles/su3_smear.md)."""
import functools

import numpy as np
import pytest
import torch

import gaugefix_restatement as gf
import loops_restatement as lr
import smear_restatement as sm
from native_layout import pack_dec, unpack_dec

gpu = pytest.mark.gpu
NB = 3


@functools.lru_cache(maxsize=None)
def reference(L):
    """the links and the restatement's answer for every launch, computed once"""
    x = sm.smooth_input(L, NB)
    a1, a2, a3 = sm.HYP_ALPHAS
    b1 = sm.hyp_level1(x, a3)
    b2 = sm.hyp_level2(x, b1, a2)
    return x, [sm.ape_step(x, alpha, D) for alpha, D in sm.APE_CASES], b1, b2, sm.hyp_level3(x, b2, a1)


@functools.lru_cache(maxsize=None)
def iterated(L):
    """the iterated restatement for the interface tests: {(what, nsteps): field}"""
    x = sm.smooth_input(L, NB)
    out = {}
    for n in sm.API_STEPS:
        out['spatial0', n] = sm.ape(x, 0.5, sm.spatial(0), n)
        out['spatial2', n] = sm.ape(x, 0.4, sm.spatial(2), n)
        out['all', n] = sm.ape(x, 0.7, 15, n)
        out['hyp', n] = sm.hyp(x, sm.HYP_ALPHAS, n)
    return x, out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@gpu
@pytest.mark.parametrize('L', sm.GPU_LATTICES)
def test_kernels_against_restatement(L):
    from l2hmc import _ops as ops
    x, apes, b1, b2, v = reference(L)
    a1, a2, a3 = sm.HYP_ALPHAS
    xn = ops.su3_pack(dev(x))
    keep = xn.clone()
    worst = {k: 0.0 for k in ('ape', 'level1', 'level2', 'level3')}
    for (alpha, D), want in zip(sm.APE_CASES, apes):
        got = host(ops.su3_unpack(ops.su3_ape_smear_n(xn, alpha, D, L), L))
        for mu in range(4):
            if not (D >> mu) & 1:
                assert np.array_equal(got[:, mu], x[:, mu]), (D, mu)               # copied bit for bit
        d = float(np.abs(got - want).max())
        assert d <= sm.TOL['ape'], (alpha, D, d)
        worst['ape'] = max(worst['ape'], d)
    b1n, b2n = dev(pack_dec(sm.dec_stack(b1))), dev(pack_dec(sm.dec_stack(b2)))
    worst['level1'] = float(np.abs(unpack_dec(host(ops.su3_hyp_level1_n(xn, a3, L)), L) - sm.dec_stack(b1)).max())
    worst['level2'] = float(np.abs(unpack_dec(host(ops.su3_hyp_level2_n(xn, b1n, a2, L)), L)
                                   - sm.dec_stack(b2)).max())
    worst['level3'] = float(np.abs(host(ops.su3_unpack(ops.su3_hyp_level3_n(xn, b2n, a1, L), L)) - v).max())
    print(f'{L}: worst deviation / tolerance: ' + ', '.join(f'{k} {worst[k] / sm.TOL[k]:.3g}' for k in worst))
    for k in ('level1', 'level2', 'level3'):
        assert worst[k] <= sm.TOL[k], (k, worst[k])
    assert torch.equal(xn, keep)
    # an output given by the caller is the one written and returned
    out = torch.full_like(xn, -7.0)
    assert ops.su3_ape_smear_n(xn, 0.5, 14, L, out=out) is out
    assert np.abs(host(ops.su3_unpack(out, L)) - apes[1]).max() <= sm.TOL['ape']


@gpu
@pytest.mark.parametrize('L', sm.API_LATTICES)
def test_public_interface_against_iterated_restatement(L):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    lat = LatticeSU3(NB, list(L))
    x0, want = iterated(L)
    x = dev(x0)
    keep = x.clone()
    xn = lat.pack(x).clone()
    keepn = xn.clone()
    worst = 0.0
    for n in sm.API_STEPS:
        calls = {'spatial0': (lambda f, a: f(a, nsteps=n), lat.ape_smear, lat.ape_smear_n, 'ape'),
                 'spatial2': (lambda f, a: f(a, 0.4, n, 'spatial', 2), lat.ape_smear, lat.ape_smear_n, 'ape'),
                 'all': (lambda f, a: f(a, alpha=0.7, nsteps=n, dirs='all'), lat.ape_smear, lat.ape_smear_n, 'ape'),
                 'hyp': (lambda f, a: f(a, nsteps=n), lat.hyp_smear, lat.hyp_smear_n, 'hyp')}
        for what, (call, f, fn, tol) in calls.items():
            y = call(f, x)
            yn = call(fn, xn)
            assert y.shape == x.shape and yn.shape == xn.shape and y.data_ptr() != x.data_ptr()
            assert torch.equal(lat.unpack(yn), y), (what, n)                        # one code path, two layouts
            d = float(np.abs(host(y) - want[what, n]).max())
            worst = max(worst, d / sm.TOL[tol])
            assert d <= sm.TOL[tol], (what, n, d)
            if n == 0:
                assert torch.equal(y, x) and yn is xn
    print(f'{L}: worst deviation / tolerance over nsteps {sm.API_STEPS}: {worst:.3g}')
    assert torch.equal(x, keep) and torch.equal(xn, keepn)                          # the input is never written
    # the defaults: spatial, time_dir 0, alpha 0.5, one step; (0.75, 0.6, 0.3), one step
    assert torch.equal(lat.ape_smear(x), lat.ape_smear(x, 0.5, 1, 'spatial', 0))
    assert torch.equal(lat.hyp_smear(x), lat.hyp_smear(x, (0.75, 0.6, 0.3), 1))
    assert torch.equal(lat.hyp_smear(x, [0.75, 0.6, 0.3]), lat.hyp_smear(x))


@gpu
def test_chains_are_independent():
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (3, 4, 5, 2)
    x = dev(sm.smooth_input(L, NB))
    lat3, lat1 = LatticeSU3(NB, list(L)), LatticeSU3(1, list(L))
    for smear in (lambda lat, v: lat.ape_smear(v, 0.5, 3), lambda lat, v: lat.ape_smear(v, 0.7, 2, 'all'),
                  lambda lat, v: lat.hyp_smear(v, nsteps=2)):
        y = smear(lat3, x)
        for c in range(NB):
            assert torch.equal(smear(lat1, x[c:c + 1].clone()), y[c:c + 1]), c


@gpu
def test_gauge_covariance():
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 2, 6, 2)
    lat = LatticeSU3(NB, list(L))
    x = dev(sm.smooth_input(L, NB))
    g = dev(gf.random_su3(np.random.default_rng(41), (NB, *L)))                    # a rough transformation
    gx = lat.gauge_transform(x, g)
    for name, smear, tol in (('ape spatial', lambda v: lat.ape_smear(v, 0.5, 1, 'spatial', 1), 'ape'),
                             ('ape 4D', lambda v: lat.ape_smear(v, 0.7, 1, 'all'), 'ape'),
                             ('hyp', lambda v: lat.hyp_smear(v), 'hyp')):
        d = float((smear(gx) - lat.gauge_transform(smear(x), g)).abs().max())
        print(f'{name}: |smear(g x) - g smear(x)| / tolerance = {d / sm.TOL[tol]:.3g}')
        assert d <= sm.TOL[tol], (name, d)


@gpu
def test_pure_gauge_stays_trivial():
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 4, 4, 4)
    lat = LatticeSU3(NB, list(L))
    x = dev(gf.pure_gauge(np.random.default_rng(9), NB, L))                         # a rough (Haar-like) transformation
    assert float((lat.polyakov(x) - 1.0).abs().max()) <= 1e-12
    for name, y in (('ape spatial', lat.ape_smear(x, 0.5, 3)), ('ape 4D', lat.ape_smear(x, 0.7, 3, 'all')),
                    ('hyp', lat.hyp_smear(x, nsteps=2))):
        dp = float((lat.plaqs(y) - 1.0).abs().max())
        dw = float((lat.wilson_loop_table(y, 3, 3) - 1.0).abs().max())
        dl = float((lat.polyakov(y) - 1.0).abs().max())
        print(f'{name}: |plaq - 1| = {dp:.3g}, |W - 1| = {dw:.3g}, |P - 1| = {dl:.3g}')
        assert dp <= 1e-12 and dw <= 1e-12 and dl <= 1e-12
        assert float((y - x).abs().max()) <= 1e-12                                  # the same pure gauge


def table_from_restatement(xa, xh, rmax, tmax, td, V):
    """W(R, T) from the lines of the torch restatement: R lines of xa along mu != td, T lines of xh along td"""
    a, h = torch.from_numpy(xa), torch.from_numpy(xh)
    out = torch.empty((xa.shape[0], rmax, tmax), dtype=torch.float64)
    k = [lr.pair_index(mu, td) for mu in range(4) if mu != td]
    for r in range(1, rmax + 1):
        for t in range(1, tmax + 1):
            s, _ = lr.loop_sums(lr.line(a, r), r, lr.line(h, t), t)
            out[:, r - 1, t - 1] = s[:, k].real.mean(-1) / (3.0 * V)
    return out


@gpu
@pytest.mark.parametrize('time_dir', [0, 2])
def test_loop_tables_with_two_fields(time_dir):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 4, 4, 4)
    lat = LatticeSU3(NB, list(L))
    x = dev(sm.smooth_input(L, NB))
    rmax = tmax = 3
    thin = lat.wilson_loop_table(x, rmax, tmax, time_dir)
    # xt = x: the table of wilson_loop_table, bit for bit (from the same tensor and from a copy of it)
    assert torch.equal(lat.wilson_loop_table_xt(x, x, rmax, tmax, time_dir), thin)
    assert torch.equal(lat.wilson_loop_table_xt(x, x.clone(), rmax, tmax, time_dir), thin)
    xa = lat.ape_smear(x, 0.5, 4, 'spatial', time_dir)
    xh = lat.hyp_smear(x)
    got = lat.wilson_loop_table_xt(xa, xh, rmax, tmax, time_dir)
    want = table_from_restatement(host(xa), host(xh), rmax, tmax, time_dir, lat.volume)
    d = float((got.cpu() - want).abs().max())
    print(f'time_dir {time_dir}: |W(xa, xh) - restatement| = {d:.3g}')
    # entries are means of O(1) traces over 3 V loops of at most 12 links each, in fp64: rounding stays below 1e-13
    assert d <= 1e-13
    # the two roles are not interchangeable: the table does see which field carries which lines
    assert float((lat.wilson_loop_table_xt(xh, xa, rmax, tmax, time_dir) - got).abs().max()) > 1e-4
    # smeared_loop_table is that composition
    s = lat.smeared_loop_table(x, rmax, tmax, time_dir, ape_alpha=0.5, ape_steps=4)
    assert torch.equal(s, got)
    assert torch.equal(lat.smeared_loop_table(x, rmax, tmax, time_dir, ape_steps=0, hyp_alphas=None), thin)
    assert torch.equal(lat.smeared_loop_table(x, rmax, tmax, time_dir, ape_steps=0),
                       lat.wilson_loop_table_xt(x, xh, rmax, tmax, time_dir))
    assert torch.equal(lat.smeared_loop_table(x, rmax, tmax, time_dir, ape_steps=4, hyp_alphas=None),
                       lat.wilson_loop_table(xa, rmax, tmax, time_dir))
    if time_dir == 0:
        assert torch.equal(lat.smeared_loop_table(x, rmax, tmax),
                           lat.wilson_loop_table_xt(lat.ape_smear(x, 0.5, 10), xh, rmax, tmax))
    # on a smooth field smearing raises every loop
    print(f'thin {host(thin[0]).round(4).tolist()} smeared {host(s[0]).round(4).tolist()}')
    assert bool((s > thin).all())
