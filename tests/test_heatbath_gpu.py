"""GPU tests of the SU(3) heatbath / overrelaxation kernels (csrc/su3_heatbath.hip) and of what is built on them:
the kernels against the numpy restatement tests/heatbath_restatement.py from the same uniforms, the public interface
of LatticeSU3 / Trainer, and two checks that do not rest on the restatement: the plaquette that the sweeps equilibrate
to at strong coupling, and its stationarity under the project's own HMC at beta = 5.7."""
import functools

import numpy as np
import pytest
import torch

import heatbath_restatement as hb
from native_layout import pack, unpack
from oracle import su3 as osu3

gpu = pytest.mark.gpu
NB = 3
# x + nu == x - nu; V/2 = 48: a partial wavefront; V/2 = 256: whole blocks; V/2 = 320: several blocks, the last partial
LATTICES = [(2, 2, 2, 2), (4, 2, 6, 2), (2, 4, 2, 6), (4, 4, 4, 8), (4, 4, 4, 10)]
CASES = [(0.3, 1), (5.7, 4)]
LEFT_OUT = [0]                      # links left out of the comparison over the whole module: at most one


@functools.lru_cache(maxsize=None)
def reference(L, case):
    """the links, the uniforms of the 8 launches and the restatement's answers, computed once per (lattice, case)"""
    beta, ntry = CASES[case]
    rng = np.random.default_rng(1000 * LATTICES.index(L) + case)
    x = hb.random_links(rng, NB, L)
    u = rng.random((8, NB, 3, 4 * ntry + 2, int(np.prod(L)) // 2))
    return x, u, [hb.heatbath(x, beta, l // 2, l % 2, u[l], ntry) for l in range(8)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def split(new, old, mu, parity, L):
    """(updated links of new, of old, every other link of new, of old)"""
    V = int(np.prod(L))
    idx = hb.half_sites(L, parity)
    n, o = (a.reshape(a.shape[0], 4, V, 3, 3).transpose(1, 2, 0, 3, 4) for a in (new, old))
    keep = np.ones((4, V), dtype=bool)
    keep[mu, idx] = False
    return n[mu][idx].transpose(1, 0, 2, 3), o[mu][idx].transpose(1, 0, 2, 3), n[keep], o[keep]


@pytest.mark.parametrize('case', range(len(CASES)))
@pytest.mark.parametrize('L', LATTICES)
def test_seeds_have_no_marginal_accept(L, case):
    """CPU: no accept decision of the GPU comparison below sits within 1e-12 of its threshold, so no link of it is
    expected to be left out"""
    assert min(float(m.min()) for _, _, m in reference(L, case)[2]) >= 1e-12


@gpu
@pytest.mark.parametrize('case', range(len(CASES)))
@pytest.mark.parametrize('L', LATTICES)
def test_heatbath_kernel_against_restatement(L, case):
    from l2hmc import _ops as ops
    beta, ntry = CASES[case]
    x, u, want = reference(L, case)
    xn0 = dev(pack(x))
    vh = int(np.prod(L)) // 2
    worst = 0.0
    for l in range(8):
        mu, parity = l // 2, l % 2
        xn = xn0.clone()
        fails = host(ops.su3_heatbath_(xn, beta, mu, parity, dev(u[l]), ntry, L))
        got = unpack(host(xn), L)
        wx, wf, margin = want[l]
        skip = margin.min((1, 2)) < 1e-12
        LEFT_OUT[0] += int(skip.sum())
        assert LEFT_OUT[0] <= 1
        g_upd, w_upd, g_rest, x_rest = split(got, wx, mu, parity, L)
        assert np.array_equal(g_rest, split(x, x, mu, parity, L)[2]), (mu, parity)      # untouched: bit-identical
        d = np.where(skip, 0.0, np.abs(g_upd - w_upd).max((-2, -1)))
        worst = max(worst, float(d.max()))
        assert d.max() <= 1e-11, (mu, parity, d.max())
        if not skip.any():
            assert np.array_equal(fails, wf), (mu, parity, fails, wf)
        if ntry == 1:
            assert ((fails > 0) & (fails < 3 * vh)).all(), fails                      # the fallback is exercised
    print(f'heatbath {L} beta {beta} ntry {ntry}: worst |dU| / 1e-11 = {worst / 1e-11:.3g}')


@gpu
@pytest.mark.parametrize('L', LATTICES)
def test_overrelax_kernel(L):
    from l2hmc import _ops as ops
    x = reference(L, 0)[0]
    xn0 = dev(pack(x))
    s0 = osu3.action(x, 1.0)
    worst = [0.0, 0.0, 0.0]
    for l in range(8):
        mu, parity = l // 2, l % 2
        xn = xn0.clone()
        ops.su3_overrelax_(xn, mu, parity, L)
        got = unpack(host(xn), L)
        g_upd, x_upd, g_rest, x_rest = split(got, x, mu, parity, L)
        assert np.array_equal(g_rest, x_rest), (mu, parity)
        assert (np.abs(g_upd - x_upd).max((-2, -1)) > 1e-6).all()
        ds = float(np.abs(osu3.action(got, 1.0) / s0 - 1.0).max())
        dsu = max(float(np.abs(osu3.adj(g_upd) @ g_upd - np.eye(3)).max()), float(np.abs(osu3.det3(g_upd) - 1).max()))
        dre = float(np.abs(got - hb.overrelax(x, mu, parity)).max())
        worst = [max(a, b) for a, b in zip(worst, (ds, dsu, dre))]
        assert ds <= 1e-12 and dsu <= 1e-12 and dre <= 1e-11, (mu, parity, ds, dsu, dre)
    print(f'overrelax {L}: worst |dS/S| / 1e-12 = {worst[0] / 1e-12:.3g}, SU(3) / 1e-12 = {worst[1] / 1e-12:.3g}, '
          f'|dU| / 1e-11 = {worst[2] / 1e-11:.3g}')


@gpu
def test_public_interface():
    from l2hmc import _ops as ops
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (2, 4, 2, 6)
    V = int(np.prod(L))
    lat = LatticeSU3(NB, list(L))
    x = dev(reference(L, 1)[0])
    x_before = x.clone()
    kw = dict(nsweeps=2, nover=1, ntry=3)
    a, info = lat.heatbath(x, 5.7, generator=torch.Generator().manual_seed(5), **kw)
    b, _ = lat.heatbath(x, 5.7, generator=torch.Generator().manual_seed(5), **kw)
    assert torch.equal(a, b) and torch.equal(x, x_before) and a.shape == x.shape
    assert not torch.equal(a, x)
    # the sweep by hand, in the documented draw order
    gen = torch.Generator().manual_seed(5)
    xn = ops.su3_pack(x).clone()
    fails = torch.zeros(NB, dtype=torch.float64, device='cuda')
    for _ in range(2):
        for mu in range(4):
            for parity in (0, 1):
                u = torch.rand((NB, 3, 4 * 3 + 2, V // 2), dtype=torch.float64, generator=gen).cuda()
                fails += ops.su3_heatbath_(xn, 5.7, mu, parity, u, 3, L)
        for mu in range(4):
            for parity in (0, 1):
                ops.su3_overrelax_(xn, mu, parity, L)
        xn = ops.su3_project_su_n(xn)
    assert torch.equal(a, ops.su3_unpack(xn, L))
    assert torch.equal(info['fail_frac'], fails / (3 * 4 * V * 2))
    assert info['fail_frac'].shape == (NB,) and float(info['fail_frac'].max()) < 0.5
    # the native entry, the device generator, no reunitarisation, overrelaxation alone
    xn0 = ops.su3_pack(x)
    keep = xn0.clone()
    yn, info = lat.heatbath_n(xn0, 5.7, nsweeps=1, reunitarize=False)
    assert torch.equal(xn0, keep) and yn.shape == xn0.shape and not torch.equal(yn, xn0)
    assert float(ops.su3_check_su_n(yn).max()) < 1e-12
    o = lat.overrelax(x, nsweeps=2)
    assert torch.equal(x, x_before) and not torch.equal(o, x)
    assert float(((lat.action(o, 1.0) - lat.action(x, 1.0)) / lat.action(x, 1.0)).abs().max()) < 1e-12
    assert torch.equal(lat.heatbath(x, 5.7, nsweeps=0)[0], x) and torch.equal(lat.overrelax_n(xn0, 0), xn0)
    # refusals
    for bad in (dict(beta=0.0), dict(beta=-1.0), dict(ntry=0), dict(ntry=17), dict(nsweeps=-1), dict(nover=-1)):
        with pytest.raises(ValueError):
            lat.heatbath(x, **{'beta': 5.7, **bad})
    with pytest.raises(ValueError):
        lat.overrelax(x, nsweeps=-1)
    with pytest.raises(ValueError):
        lat.heatbath(x.clone().requires_grad_(True), 5.7)
    with pytest.raises(ValueError):
        lat.overrelax(x.clone().requires_grad_(True))
    odd = LatticeSU3(1, [2, 3, 2, 2])
    with pytest.raises(ValueError):
        odd.heatbath(odd.random().cuda(), 5.7)
    with pytest.raises(ValueError):
        odd.overrelax(odd.random().cuda())
    imp = LatticeSU3(NB, list(L), c1=-0.331)
    with pytest.raises(ValueError):
        imp.heatbath(x, 5.7)
    with pytest.raises(ValueError):
        imp.overrelax(x)


@gpu
def test_trainer_thermalize():
    import l2hmc.configs as cfgs
    from l2hmc.trainers.pytorch.trainer import Trainer
    tr = Trainer(cfgs.get_config(['+experiment=su3', 'dynamics.nchains=4', 'network.units=[8]', 'seed=7']))
    x = tr.thermalize(5.7, nsweeps=3, nover=1)
    assert tuple(x.shape) == tuple(tr.dynamics.unflatten(tr.lattice.random().cuda()).shape) == (4, 4, 4, 4, 4, 4, 3, 3)
    p = tr.lattice.plaqs(x)
    assert float(p.min()) > 0.2                                  # three sweeps from a hot start (plaquette 0) at 5.7
    y = tr.thermalize(torch.tensor(5.7), x=x, nsweeps=1, nover=0)
    assert y.shape == x.shape and not torch.equal(x, y)
    tu = Trainer(cfgs.get_config(['dynamics.group=U1', 'dynamics.latvolume=[4,4]', 'dynamics.nchains=4',
                                  'dynamics.nleapfrog=2', 'dynamics.verbose=false', 'network.units=[4]', 'conv=none']))
    with pytest.raises(NotImplementedError):
        tu.thermalize(2.0)


@gpu
def test_stationary_under_hmc():
    """4^4, 64 chains, beta = 5.7: after 30 heatbath sweeps (nover = 1) from a hot start, 20 plain-HMC trajectories of
    the project's own sampler at the same beta must not move the plaquette: the chain mean of the paired difference is
    zero within 4 of its standard errors.  (A heatbath at the wrong coupling, a factor 2 in alpha say, makes HMC drift.)
    Measured on an MI355X: 0.55397 after the heatbath, HMC - heatbath = +0.00565 +- 0.00179 (3.16 standard errors),
    acceptance 0.81.  beta = 5.7 is next to the N_t = 4 deconfinement transition, where 30 sweeps from a hot start are
    barely enough: a 300-sweep heatbath history stays at 0.5595 +- 0.0013 from sweep 30 on, which is where the HMC of
    this test ends (0.5596), and HMC after those 300 sweeps moves the plaquette by -0.002 ... -0.006 +- 0.002 from a
    last heatbath value of 0.5630 (profiles/su3_heatbath.md)."""
    torch.set_default_dtype(torch.float64)
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    torch.manual_seed(41)
    np.random.seed(41)
    nb, L, beta = 64, [4, 4, 4, 4], 5.7
    lat = LatticeSU3(nb, L)
    x, info = lat.heatbath(lat.random().cuda(), beta, nsweeps=30, nover=1)
    p_hb = lat.plaqs(x).clone()
    dc = cfgs.DynamicsConfig(nchains=nb, group='SU3', latvolume=L, nleapfrog=10, eps=0.05, eps_hmc=0.05,
                             use_split_xnets=False, use_separate_networks=False, verbose=False)
    dyn = Dynamics(lat.action, dc, None).eval()
    acc = []
    for _ in range(20):
        x, m = dyn.apply_transition_hmc((x, torch.tensor(beta)), eps=0.05, nleapfrog=10)
        x = lat.g.compat_proj(dyn.unflatten(x.detach()))
        acc.append(float(m['acc'].mean()))
    d = host(lat.plaqs(x) - p_hb)
    mean, se = d.mean(), d.std(ddof=1) / np.sqrt(nb)
    print(f'stationarity: plaquette after heatbath {float(p_hb.mean()):.5f}, after HMC - after heatbath = {mean:+.5f} '
          f'+- {se:.5f} ({mean / se:+.2f} standard errors), HMC acceptance {np.mean(acc):.3f}, '
          f'heatbath fail_frac {float(info["fail_frac"].max()):.2e}')
    assert np.mean(acc) > 0.6
    assert 0.5 < float(p_hb.mean()) < 0.6
    assert abs(mean) <= 4.0 * se, (mean, se)


@gpu
@pytest.mark.parametrize('ntry', [1, 6])
def test_equilibrium_at_strong_coupling(ntry):
    """<Re tr P / 3> at beta = 1 on 4^4 against beta/18 + beta^2/216 = 0.0602 within 5 standard errors from the spread
    over 64 independent chains (10 sweeps to equilibrate, 20 measured)."""
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    torch.manual_seed(50 + ntry)
    lat = LatticeSU3(64, [4, 4, 4, 4])
    xn = lat.pack(lat.random().cuda())
    rows = []
    for sweep in range(30):
        xn, _ = lat.heatbath_n(xn, 1.0, ntry=ntry)
        if sweep >= 10:
            rows.append(lat.plaq_sums_n(xn)[:, 0] / (18 * lat.volume))
    per_chain = host(torch.stack(rows).mean(0))
    mean, se = per_chain.mean(), per_chain.std(ddof=1) / np.sqrt(per_chain.size)
    print(f'strong coupling ntry {ntry}: plaquette {mean:.5f} +- {se:.5f} (series 0.0602), '
          f'{(mean - 0.0602) / se:+.2f} standard errors')
    assert abs(mean - 0.0602) <= 5.0 * se, (mean, se)
