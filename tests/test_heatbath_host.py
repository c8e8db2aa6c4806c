"""CPU checks of the yardstick tests/heatbath_restatement.py by facts that do not depend on it: the Kennedy-Pendleton
sampler against the analytic SU(2) density, forced rejection / acceptance, what overrelaxation conserves, and the
strong-coupling plaquette that heatbath sweeps equilibrate to.  The kernels are compared with this yardstick in
tests/test_heatbath_emu.py (host build) and tests/test_heatbath_gpu.py."""
import numpy as np
import pytest

import heatbath_restatement as hb
from oracle import su3 as osu3

L = (2, 4, 2, 4)
NB = 2


@pytest.fixture(scope='module')
def links():
    return hb.random_links(np.random.default_rng(5), NB, L)


def exact_mean_b0(alpha):
    """int t sqrt(1 - t^2) e^(alpha t) dt / int sqrt(1 - t^2) e^(alpha t) dt over [-1, 1], Gauss-Chebyshev of the
    second kind (weight sqrt(1 - t^2)): exact to rounding for the entire function e^(alpha t) at 200 nodes"""
    k = np.arange(1, 201)
    t = np.cos(k * np.pi / 201)
    w = np.sin(k * np.pi / 201) ** 2 * np.exp(alpha * (t - 1.0))
    return float((w * t).sum() / w.sum())


def test_su2_sampler_against_the_density():
    rng = np.random.default_rng(11)
    n = 400000
    accs = []
    for alpha in (0.2, 2.0, 8.0, 16.0):
        b0, ok, _ = hb.kp_try(alpha, *rng.random((4, n)))
        s = b0[ok]
        assert s.min() >= -1.0 and s.max() <= 1.0
        se = s.std(ddof=1) / np.sqrt(s.size)
        dev = (s.mean() - exact_mean_b0(alpha)) / se
        print(f'alpha {alpha}: acceptance {ok.mean():.3f}, <b0> {s.mean():.5f}, exact {exact_mean_b0(alpha):.5f}, '
              f'{dev:+.2f} standard errors')
        assert abs(dev) <= 4.0, (alpha, dev)
        accs.append(ok.mean())
    assert all(a < b for a, b in zip(accs, accs[1:])), accs
    # the direction is uniform on the sphere: |b| = 1, and the three vector components average to zero
    b = hb.kp_direction(np.full(n, 0.3), *rng.random((2, n)))
    assert np.abs((b * b).sum(0) - 1.0).max() < 1e-14
    assert np.abs(b[1:].mean(1)).max() < 4.0 * np.sqrt((1 - 0.09) / 3 / n)


def test_forced_reject_and_forced_accept(links):
    rng = np.random.default_rng(12)
    vh = int(np.prod(L)) // 2
    for ntry in (1, 3):
        u = rng.random((NB, 3, 4 * ntry + 2, vh))
        u[:, :, 3:4 * ntry:4] = 0.0                           # v4 = 1: 1 <= 1 - delta/2 never holds (delta > 0)
        for mu in range(4):
            for parity in (0, 1):
                out, fails, _ = hb.heatbath(links, 5.7, mu, parity, u, ntry)
                assert np.array_equal(out, links)
                assert np.array_equal(fails, np.full(NB, 3.0 * vh))
        u = rng.random((NB, 3, 4 * ntry + 2, vh))
        u[:, :, 0:4 * ntry:4] *= 0.01                         # delta <= 0.0201 / alpha
        u[:, :, 2:4 * ntry:4] *= 0.01
        u[:, :, 3:4 * ntry:4] = 1.0 - 1e-9                    # v4^2 = 1e-18
        out, fails, _ = hb.heatbath(links, 5.7, 1, 0, u, ntry)
        assert np.array_equal(fails, np.zeros(NB))
        assert not np.array_equal(out, links)


def test_overrelaxation(links):
    V = int(np.prod(L))
    s0 = osu3.action(links, 1.0)
    for mu in range(4):
        for parity in (0, 1):
            out = hb.overrelax(links, mu, parity)
            assert np.abs(osu3.action(out, 1.0) / s0 - 1.0).max() <= 1e-13
            idx = hb.half_sites(L, parity)
            other = np.setdiff1d(np.arange(V), idx)
            new, old = out.reshape(NB, 4, V, 3, 3), links.reshape(NB, 4, V, 3, 3)
            assert (np.abs(new[:, mu][:, idx] - old[:, mu][:, idx]).max((-2, -1)) > 1e-6).all()
            assert np.array_equal(new[:, mu][:, other], old[:, mu][:, other])
            for nu in range(4):
                if nu != mu:
                    assert np.array_equal(new[:, nu], old[:, nu])
            upd = new[:, mu][:, idx]
            assert np.abs(osu3.adj(upd) @ upd - np.eye(3)).max() <= 1e-12
            assert np.abs(osu3.det3(upd) - 1.0).max() <= 1e-12


def test_heatbath_step_keeps_the_rest_and_the_group(links):
    rng = np.random.default_rng(13)
    V = int(np.prod(L))
    u = rng.random((NB, 3, 18, V // 2))
    out, fails, margin = hb.heatbath(links, 5.7, 2, 1, u, 4)
    idx = hb.half_sites(L, 1)
    other = np.setdiff1d(np.arange(V), idx)
    new, old = out.reshape(NB, 4, V, 3, 3), links.reshape(NB, 4, V, 3, 3)
    assert np.array_equal(new[:, 2][:, other], old[:, 2][:, other])
    assert all(np.array_equal(new[:, nu], old[:, nu]) for nu in (0, 1, 3))
    upd = new[:, 2][:, idx]
    assert np.abs(osu3.adj(upd) @ upd - np.eye(3)).max() <= 1e-12 and np.abs(osu3.det3(upd) - 1.0).max() <= 1e-12
    assert np.isfinite(margin[:, :, 0]).all() and margin.shape == (NB, 3, 4, V // 2)


@pytest.mark.parametrize('ntry', [1, 6])
def test_equilibrium_at_strong_coupling(ntry):
    """<Re tr P / 3> at beta = 1 on 4^4 against the strong-coupling series beta/18 + beta^2/216 = 0.0602, within 5
    standard errors from the spread over independent chains (8 chains, 8 sweeps to equilibrate, 24 measured)."""
    rng = np.random.default_rng(20 + ntry)
    x = hb.random_links(rng, 8, (4, 4, 4, 4))
    rows = []
    for sweep in range(32):
        x, _ = hb.heatbath_sweep(x, 1.0, ntry, rng)
        if sweep >= 8:
            rows.append(osu3.plaqs(x))
    per_chain = np.mean(rows, 0)
    mean, se = per_chain.mean(), per_chain.std(ddof=1) / np.sqrt(per_chain.size)
    print(f'ntry {ntry}: plaquette {mean:.5f} +- {se:.5f} (series 0.0602)')
    assert abs(mean - 0.0602) <= 5.0 * se, (mean, se)


def test_python_surface_and_refusals():
    """what exists, and what raises before any kernel runs (so without a GPU)"""
    import inspect

    import torch
    from l2hmc import _ops as ops
    from l2hmc import native
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.trainers.pytorch.trainer import Trainer
    assert callable(ops.su3_heatbath_) and callable(ops.su3_overrelax_)
    assert 'l2q_su3_heatbath' in native.SIGNATURES and 'l2q_su3_overrelax' in native.SIGNATURES
    p = inspect.signature(LatticeSU3.heatbath_n).parameters
    assert list(p) == ['self', 'xn', 'beta', 'nsweeps', 'nover', 'ntry', 'generator', 'reunitarize']
    assert [p[k].default for k in ('nsweeps', 'nover', 'ntry', 'generator', 'reunitarize')] == [1, 0, 4, None, True]
    assert list(inspect.signature(LatticeSU3.heatbath).parameters)[1:] == ['x', *list(p)[2:]]
    assert inspect.signature(LatticeSU3.overrelax).parameters['nsweeps'].default == 1
    assert inspect.signature(LatticeSU3.overrelax_n).parameters['nsweeps'].default == 1
    t = inspect.signature(Trainer.thermalize).parameters
    assert list(t) == ['self', 'beta', 'x', 'nsweeps', 'nover']
    assert (t['x'].default, t['nsweeps'].default, t['nover'].default) == (None, 50, 3)
    lat = LatticeSU3(1, [2, 2, 2, 4])
    x = torch.zeros(1, 4, 2, 2, 2, 4, 3, 3, dtype=torch.complex128)
    for bad in (dict(beta=0.0), dict(beta=-1.0), dict(beta=float('nan')), dict(ntry=0), dict(ntry=17),
                dict(nsweeps=-1), dict(nover=-1)):
        with pytest.raises(ValueError):
            lat.heatbath(x, **{'beta': 5.7, **bad})
        with pytest.raises(ValueError):
            lat.heatbath_n(torch.zeros(1, 4, 9, 32, dtype=torch.complex128), **{'beta': 5.7, **bad})
    with pytest.raises(ValueError):
        lat.overrelax(x, nsweeps=-1)
    with pytest.raises(ValueError):
        lat.heatbath(x.clone().requires_grad_(True), 5.7)
    with pytest.raises(ValueError):
        lat.overrelax_n(torch.zeros(1, 4, 9, 32, dtype=torch.complex128).requires_grad_(True))
    odd = LatticeSU3(1, [2, 3, 2, 2])
    xo = torch.zeros(1, 4, 2, 3, 2, 2, 3, 3, dtype=torch.complex128)
    imp = LatticeSU3(1, [2, 2, 2, 4], c1=-0.331)
    for la, xa in ((odd, xo), (imp, x)):
        with pytest.raises(ValueError):
            la.heatbath(xa, 5.7)
        with pytest.raises(ValueError):
            la.overrelax(xa)
