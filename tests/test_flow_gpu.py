"""GPU tier of the Wilson flow / clover observables: the kernels behind l2q_su3_clover_reduce, l2q_su3_flow_stage
and l2q_su3_flow_step and the LatticeSU3 surface on top of them, against the independent restatement
tests/flow_restatement.py (torch on the CPU; validated on its own in tests/test_flow_host.py)."""
import math

import numpy as np
import pytest
import torch

import flow_restatement as fr
from oracle import su3 as osu3

pytestmark = pytest.mark.gpu

LATTICES = [(2, 2, 2, 2), (1, 3, 2, 5), (4, 4, 4, 4), (3, 5, 2, 7), (2, 2, 8, 8), (3, 2, 4, 16), (3, 8, 8, 8),
            (2, 4, 8, 16), (1, 2, 8, 8), (2, 4, 4, 12), (2, 16, 4, 4), (5, 4, 4, 4), (2, 2, 2, 32), (4, 3, 8, 8)]


@pytest.fixture(scope='module')
def ops():
    from l2hmc import _ops
    return _ops


@pytest.fixture()
def tuning():
    """set_tuning for the test, the defaults back afterwards"""
    from l2hmc import native
    yield native.set_tuning
    native.set_tuning('force_tile', 5)
    native.set_tuning('xcd_swizzle', 1)


def dev(a):
    a = a.numpy() if isinstance(a, torch.Tensor) else a
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu()


def err(a, b):
    return float((torch.as_tensor(a) - torch.as_tensor(b)).abs().max())


def hot(nb, L, rng):
    """hot start of the stencil tests: projectSU of a complex Gaussian"""
    return torch.from_numpy(osu3.project_su(rng.normal(size=(nb, 4, *L, 3, 3))
                                            + 1j * rng.normal(size=(nb, 4, *L, 3, 3))))


def vol(L):
    return int(np.prod(L))


# ------------------------------------------------------------------ 1. raw clover sums
@pytest.mark.parametrize('L', LATTICES)
def test_clover_sums_vs_restatement(ops, tuning, L):
    """|sum - yardstick| <= 1e-12 S, S = the yardstick's sum of the absolute per-site terms (floor V): 100 x the
    ~1e-14 that a ~400-operation fp64 chain on unit-size entries gives per term."""
    rng = np.random.default_rng(7)
    nb = 3
    x = hot(nb, L, rng)
    xn = ops.su3_pack(dev(x))
    want, scale = fr.clover_sums(x)
    scale = scale.clamp(min=float(vol(L)))
    plaq = host(ops.su3_plaq_sums_n(xn, L))[:, 0]
    for swz in (0, 1):
        tuning('xcd_swizzle', swz)
        got = host(ops.su3_clover_sums_n(xn, L))
        rel = ((got - want).abs() / scale).max(0).values
        print(f'L={L} swz={swz} |d|/S = {rel.tolist()}')
        assert float(rel.max()) <= 1e-12
        assert err(got[:, 2], plaq) <= 1e-10


# ------------------------------------------------------------------ 2. flux configurations
@pytest.mark.parametrize('n01,n23', [(1, 1), (2, -1), (1, 0)])
def test_flux_on_the_gpu(ops, n01, n23):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 6, 4, 8)
    x = fr.flux_config(L, n01, n23)
    lat = LatticeSU3(1, list(L))
    c = lat.clover(dev(x))
    qc, ec = fr.flux_closed_form(L, n01, n23)
    print(f'flux {n01, n23}: dQ = {abs(float(c.Q[0]) - qc):.2e} dE = {abs(float(c.E[0]) - ec):.2e}')
    assert abs(float(c.Q[0]) - qc) <= 1e-12 and abs(float(c.E[0]) - ec) <= 1e-12
    assert err(host(c.Eplaq), fr.plaq_energy(x)) <= 1e-12
    assert err(host(lat.topological_charge(dev(x))), host(c.Q)) == 0.0
    assert err(host(lat.energy_density(dev(x))), host(c.E)) == 0.0
    assert err(host(lat.energy_density(dev(x), kind='plaq')), host(c.Eplaq)) == 0.0
    # a gauge-rotated copy has the same sums
    g = fr.rand_su3((1, *L), 3.0, torch.Generator().manual_seed(9))
    xr = fr.gauge_rotate(x, g)
    s0 = host(ops.su3_clover_sums_n(ops.su3_pack(dev(x)), L))
    s1 = host(ops.su3_clover_sums_n(ops.su3_pack(dev(xr)), L))
    scale = fr.clover_sums(x)[1].clamp(min=float(vol(L)))
    print(f'gauge rotation: |d|/S = {((s0 - s1).abs() / scale).max(0).values.tolist()}')
    assert float(((s0 - s1).abs() / scale).max()) <= 1e-12
    # a fixed point of the flow: one step moves no link
    x1 = host(lat.flow(dev(x), 0.05, eps=0.05))
    print(f'flow step on flux: max |dU| = {err(x1, x):.2e}')
    assert err(x1, x) <= 1e-13


# ------------------------------------------------------------------ 3. one stage
@pytest.mark.parametrize('L', LATTICES)
def test_flow_stage(ops, tuning, L):
    rng = np.random.default_rng(13)
    nb = 3
    x = hot(nb, L, rng)
    p = torch.from_numpy(osu3.rand_tah3(rng.normal(size=(8, nb, 4, *L))))
    xn, pn = ops.su3_pack(dev(x)), ops.su3_pack(dev(p))
    c, s = -32.0 / 17.0, 0.02
    for p_in, p_in_n in ((p, pn), (None, None)):
        want_p, want_x = fr.flow_stage(x, p_in, c, s)
        for variant in (2, 5, 7):
            for swz in (0, 1):
                tuning('force_tile', variant)
                tuning('xcd_swizzle', swz)
                x_keep, p_keep = xn.clone(), pn.clone()
                po, xo = ops.su3_flow_stage_n(xn, p_in_n, c, s, L)
                ep, ex = err(host(ops.su3_unpack(po, L)), want_p), err(host(ops.su3_unpack(xo, L)), want_x)
                print(f'L={L} P_in={p_in is not None} tile={variant} swz={swz}: |dP| = {ep:.2e} |dX| = {ex:.2e}')
                assert ep <= 1e-12 and ex <= 1e-13
                assert torch.equal(xn, x_keep) and torch.equal(pn, p_keep)
                # the same stage composed from the force kick at beta = 3 and the unmasked x-update
                if p_in_n is not None:
                    pc = torch.full_like(xn, float('nan'))
                    ops.su3_force_kick_n(xn, 3.0, c, pc, L, v_src=p_in_n)
                    # p_out aliased to p_in: the same bits
                    pa = p_in_n.clone()
                    pa2, xa = ops.su3_flow_stage_n(xn, pa, c, s, L, p_out=pa)
                    assert pa2 is pa and torch.equal(pa, po) and torch.equal(xa, xo)
                else:
                    pc = ops.su3_force_n(xn, 3.0 * c, L)
                xc = ops.su3_expm_mul_n(xn, pc, s)
                assert err(host(pc), host(po)) <= 1e-13 and err(host(xc), host(xo)) <= 1e-13


def test_flow_stage_reference_anchor(ops, golden):
    """stage (None, 1, 0) on the golden links: P_out = (3 / beta) force of the reference, X_out = X_in"""
    g = golden('su3_ops')
    L = tuple(int(i) for i in g['latvolume'])
    beta = float(g['beta'])
    xn = ops.su3_pack(dev(g['x']))
    po, xo = ops.su3_flow_stage_n(xn, None, 1.0, 0.0, L)
    e = err(host(ops.su3_unpack(po, L)), torch.from_numpy((3.0 / beta) * g['force']))
    print(f'anchor: |P_out - 3/beta force| = {e:.2e}')
    assert e <= 1e-13
    assert err(host(xo), host(xn)) <= 1e-15


# ------------------------------------------------------------------ 4. n steps
def growth(x, eps, n, gen):
    """the yardstick's own response to a 1e-9 perturbation of the start: (flowed x, A = growth of the link
    difference, sensitivity of E and Q per unit link difference at the start)"""
    xp = torch.matrix_exp(1e-9 * fr.tah(torch.complex(torch.randn(x.shape, dtype=torch.float64, generator=gen),
                                                      torch.randn(x.shape, dtype=torch.float64, generator=gen)))) @ x
    d0 = float((xp - x).abs().max())
    y, yp = fr.flow(x, eps, n), fr.flow(xp, eps, n)
    e, q = fr.clover_obs(y)
    e_, q_ = fr.clover_obs(yp)
    amp = float((yp - y).abs().max()) / d0
    sens = max(1.0, float((e - e_).abs().max()) / d0, float((q - q_).abs().max()) / d0)
    return y, amp, sens


@pytest.mark.parametrize('L,eps,n', [((4, 4, 4, 4), 0.02, 20), ((1, 3, 2, 5), 0.01, 40), ((2, 2, 2, 2), 0.02, 20)])
def test_flow_steps_vs_restatement(ops, L, eps, n):
    """links within 3 n 1e-13 max(1, A), A = the growth of a 1e-9 perturbation measured in the yardstick alone;
    E, Q within 10 x that x the yardstick's own sensitivity.  Measured with these inputs on the CPU: A in
    1.0 - 6.7, sensitivity <= 2.1."""
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    gen = torch.Generator().manual_seed(21)
    nb = 3
    x = fr.rand_su3((nb, 4, *L), 3.0, gen)
    lat = LatticeSU3(nb, list(L))
    # the plaquette sum never decreases along the flow: in the yardstick first ...
    ys = x
    per_chain = [fr.clover_sums(x)[0][:, 2]]
    for _ in range(n):
        ys = fr.flow_step(ys, eps)
        per_chain.append(fr.clover_sums(ys)[0][:, 2])
    per_chain = torch.stack(per_chain)
    assert bool((per_chain[1:] >= per_chain[:-1]).all())
    y, amp, sens = growth(x, eps, n, gen)
    assert err(y, ys) == 0.0
    tol = 3.0 * n * 1e-13 * max(1.0, amp)
    # ... then in the product
    obs = lat.flow_observables(dev(x), n * eps, eps=eps)
    got_p = host(obs['Eplaq'])
    assert bool((got_p[1:] <= got_p[:-1]).all())
    xn = ops.su3_pack(dev(x))
    yn = lat.flow_n(xn, n, eps)
    got = host(ops.su3_unpack(yn, L))
    e, q = fr.clover_obs(y)
    c = lat.clover_n(yn)
    de, dq = err(host(c.E), e), err(host(c.Q), q)
    print(f'L={L} eps={eps} n={n}: A = {amp:.3g} sens = {sens:.3g} tol = {tol:.2e} |dU| = {err(got, y):.2e} '
          f'|dE| = {de:.2e} |dQ| = {dq:.2e}')
    assert err(got, y) <= tol
    assert de <= 10 * tol * sens and dq <= 10 * tol * sens
    assert err(host(obs['E'][-1]), host(c.E)) == 0.0 and err(host(obs['Q'][-1]), host(c.Q)) == 0.0
    assert float(ops.su3_check_su_n(yn).max()) <= 1e-12
    # a chain run alone equals the same chain in the batch
    for k in range(nb):
        alone = LatticeSU3(1, list(L)).flow_n(xn[k:k + 1].contiguous(), n, eps)
        assert err(host(alone), host(yn[k:k + 1])) <= 1e-14
    # the input is never written
    assert torch.equal(xn, ops.su3_pack(dev(x)))


# ------------------------------------------------------------------ 5. sizes users run
@pytest.mark.parametrize('L,nb,chains,n', [((8, 8, 8, 8), 256, (0, 37, 255), 2), ((16, 16, 16, 16), 4, (3,), 1)])
def test_flow_sizes_users_run(ops, L, nb, chains, n):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    eps = 0.01
    gen = torch.Generator().manual_seed(33)
    x = fr.rand_su3((nb, 4, *L), 3.0, gen)
    lat = LatticeSU3(nb, list(L))
    xn = ops.su3_pack(dev(x))
    yn = lat.flow_n(xn, n, eps)
    c = lat.clover_n(yn)
    raw = host(ops.su3_clover_sums_n(yn, L))
    sel = list(chains)
    xs = x[sel].contiguous()
    y, amp, sens = growth(xs, eps, n, gen)
    tol = 3.0 * n * 1e-13 * max(1.0, amp)
    got = host(ops.su3_unpack(yn[sel].contiguous(), L))
    e, q = fr.clover_obs(y)
    want, scale = fr.clover_sums(y)
    de, dq = err(host(c.E)[sel], e), err(host(c.Q)[sel], q)
    # the clover pass alone, on the product's own flowed links
    want_g, scale_g = fr.clover_sums(got)
    rel = ((raw[sel] - want_g).abs() / scale_g.clamp(min=float(vol(L)))).max(0).values
    print(f'L={L} nb={nb}: A = {amp:.3g} sens = {sens:.3g} tol = {tol:.2e} |dU| = {err(got, y):.2e} '
          f'|dE| = {de:.2e} |dQ| = {dq:.2e} clover |d|/S = {rel.tolist()}')
    assert err(got, y) <= tol
    assert de <= 10 * tol * sens and dq <= 10 * tol * sens
    assert float(rel.max()) <= 1e-12
    assert float(ops.su3_check_su_n(yn).max()) <= 1e-12
    assert torch.equal(xn, ops.su3_pack(dev(x)))


# ------------------------------------------------------------------ 6. the Python surface
def test_flow_observables_and_metrics(ops):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (4, 4, 4, 6)
    nb = 2
    gen = torch.Generator().manual_seed(44)
    x = dev(fr.rand_su3((nb, 4, *L), 3.0, gen))
    x0 = dev(fr.rand_su3((nb, 4, *L), 3.0, gen))
    lat = LatticeSU3(nb, list(L))
    eps, n = 0.02, 6
    obs = lat.flow_observables(x, n * eps, eps=eps, every=2)
    assert set(obs) == {'t', 'E', 'Eplaq', 'Q', 't2E'}
    assert obs['t'].shape == (n // 2 + 1,) and all(obs[k].shape == (n // 2 + 1, nb) for k in ('E', 'Eplaq', 'Q', 't2E'))
    for row, k in enumerate(range(0, n + 1, 2)):
        c = lat.clover(lat.flow(x, k * eps, eps=eps))
        assert abs(float(obs['t'][row]) - k * eps) <= 1e-15
        assert torch.equal(obs['E'][row], c.E) and torch.equal(obs['Q'][row], c.Q)
        assert torch.equal(obs['Eplaq'][row], c.Eplaq)
        assert torch.equal(obs['t2E'][row], obs['t'][row] ** 2 * c.E)
    assert torch.equal(lat.flow(x, 0.0), x)
    # calc_metrics without the new argument is exactly what it was
    beta = torch.tensor(5.7)
    m = lat.calc_metrics(x, beta)
    assert list(m) == ['plaqs', 'sinQ', 'intQ', 'action', 'dsdx']
    w = lat.plaq_sums(x)
    s, dsdx = lat.action_with_grad(x, beta)
    assert torch.equal(m['plaqs'], w.re / (18 * lat.volume)) and torch.equal(m['sinQ'], w.im / (18 * lat.volume))
    assert torch.equal(m['intQ'], w.im / (32 * np.pi ** 2))
    assert torch.equal(m['action'], s) and torch.equal(m['dsdx'], dsdx)
    m1 = lat.calc_metrics(x, beta, xinit=x0)
    assert list(m1) == ['plaqs', 'sinQ', 'intQ', 'action', 'dsdx', 'daction', 'dplaqs', 'dQint', 'dQsin']
    # with a flow time: exactly Qflow and t2E more (and dQflow with xinit)
    mf = lat.calc_metrics(x, beta, flow_time=0.1, flow_eps=0.02)
    assert list(mf) == list(m) + ['Qflow', 't2E']
    for k in m:
        assert torch.equal(mf[k], m[k])
    c = lat.clover(lat.flow(x, 0.1, eps=0.02))
    assert torch.equal(mf['Qflow'], c.Q) and torch.equal(mf['t2E'], 0.1 ** 2 * c.E)
    mf1 = lat.calc_metrics(x, beta, xinit=x0, flow_time=0.1, flow_eps=0.02)
    assert list(mf1) == list(m1) + ['Qflow', 't2E', 'dQflow']
    c0 = lat.clover(lat.flow(x0, 0.1, eps=0.02))
    assert torch.equal(mf1['dQflow'], (c.Q - c0.Q).abs())
    assert math.isfinite(float(mf1['dQflow'].sum()))
