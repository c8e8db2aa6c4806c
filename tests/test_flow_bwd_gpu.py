"""GPU tier of the differentiable Wilson flow: l2q_su3_force_vjp, l2q_su3_flow_stage_bwd and the reverse sweep behind
LatticeSU3.flow_autograd against torch.autograd of the restatement tests/flow_restatement.py (computed on the CPU in
complex128), their determinism and gauge covariance, and the SU(3) train step on the flowed clover charge."""
import functools

import numpy as np
import pytest
import torch

import clover_helpers as ch
import flow_restatement as fr
import helpers

pytestmark = pytest.mark.gpu

NB = 2
BETA = 2.7
# extents 1 and 2, no whole workgroup, several workgroups per chain; the last two are whole 64-site spatial tiles,
# where the forward kernels of the flow take their slice-resident variants (the VJP has one variant)
LATTICES = [(1, 3, 2, 5), (3, 5, 2, 7), (2, 5, 8, 8), (4, 4, 4, 4), (3, 4, 4, 8)]
EPS = 0.02
STAGES = [(1.0, -0.25 * EPS), (-32.0 / 17.0, (17.0 / 36.0) * EPS), (27.0 / 17.0, -(17.0 / 36.0) * EPS)]
FLOWS = [((2, 3, 4, 5), 2, 0.02), ((4, 4, 4, 4), 3, 0.01)]


@pytest.fixture(scope='module')
def ops():
    from l2hmc import _ops
    return _ops


@pytest.fixture()
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def dev(a):
    return a.detach().contiguous().cuda()


def host(t):
    return t.detach().cpu()


def cnormal(rng, shape):
    return torch.from_numpy(rng.normal(size=shape) + 1j * rng.normal(size=shape))


# ------------------------------------------------------------------ l2q_su3_force_vjp
@functools.lru_cache(maxsize=None)
def force_reference(L):
    """links, a general cotangent of the force and the yardstick's cotangent of the links (native layout): once"""
    x = ch.random_links(NB, L, 23)
    gf = cnormal(np.random.default_rng(43), (NB, 4, *L, 3, 3))
    xg = x.clone().requires_grad_(True)
    f = (BETA / 3.0) * fr.tah(xg @ fr.staples(xg))
    (want,) = torch.autograd.grad((gf.conj() * f).real.sum(), xg)
    return x, gf, ch.native(want)


def run_vjp(ops, x, gf, L, g0=None):
    xn, gn = ops.su3_pack(dev(x)), ops.su3_pack(dev(gf))
    gx = torch.zeros_like(xn) if g0 is None else dev(g0)
    ops.su3_force_vjp_(gx, xn, gn, BETA, L)
    return host(gx)


@pytest.mark.parametrize('L', LATTICES)
def test_force_vjp_vs_autograd(ops, L):
    x, gf, want = force_reference(L)
    V = int(np.prod(L))
    g0 = cnormal(np.random.default_rng(31), (NB, 4, 9, V))
    got = run_vjp(ops, x, gf, L, g0)                         # gx += : starts from g0
    err, ref = float((got - (g0 + want)).abs().max()), float(want.abs().max())
    print(f'L={L}: max |got - want| = {err:.3e}, max |want| = {ref:.3e}')
    assert ref > 0.0
    assert err <= 1e-12 * max(1.0, ref), L


@pytest.mark.parametrize('L', LATTICES)
def test_force_vjp_is_deterministic_and_batch_independent(ops, L):
    x, gf, _ = force_reference(L)
    a, b = run_vjp(ops, x, gf, L), run_vjp(ops, x, gf, L)
    assert torch.equal(a, b)
    alone = run_vjp(ops, x[:1], gf[:1], L)
    assert torch.equal(alone[0], a[0])


# ------------------------------------------------------------------ l2q_su3_flow_stage_bwd
@functools.lru_cache(maxsize=None)
def stage_reference(L, k, with_p):
    """one stage with the scheme's k-th (c, s): inputs, the stage's P_out, the cotangents fed in and the yardstick's
    cotangents of X_in and P_in"""
    c, s = STAGES[k]
    rng = np.random.default_rng(100 + 10 * k + int(with_p))
    x = ch.random_links(NB, L, 51 + k)
    p_in = fr.tah(cnormal(rng, (NB, 4, *L, 3, 3))) if with_p else torch.zeros((NB, 4, *L, 3, 3), dtype=fr.C128)
    gx_out, gp0 = cnormal(rng, (NB, 4, *L, 3, 3)), cnormal(rng, (NB, 4, *L, 3, 3))
    xg, pg = x.clone().requires_grad_(True), p_in.clone().requires_grad_(True)
    p_out, x_out = fr.flow_stage(xg, pg, c, s)
    want_x, want_p = torch.autograd.grad((gx_out.conj() * x_out).real.sum() + (gp0.conj() * p_out).real.sum(),
                                         (xg, pg))
    return x, p_out.detach(), gx_out, gp0, ch.native(want_x), ch.native(want_p)


@pytest.mark.parametrize('with_p', [False, True], ids=['p_in absent', 'p_in present'])
@pytest.mark.parametrize('k', [0, 1, 2])
@pytest.mark.parametrize('L', [(3, 5, 2, 7), (4, 4, 4, 4)])
def test_flow_stage_bwd_vs_autograd(ops, L, k, with_p):
    c, s = STAGES[k]
    x, p_out, gx_out, gp0, want_x, want_p = stage_reference(L, k, with_p)
    gp = ops.su3_pack(dev(gp0))                              # a non-zero incoming cotangent of P_out
    gx = ops.su3_flow_stage_bwd_n(ops.su3_pack(dev(x)), ops.su3_pack(dev(p_out)), c, s, ops.su3_pack(dev(gx_out)),
                                  gp, L)
    for name, got, want in (('gx_in', host(gx), want_x), ('gp', host(gp), want_p)):
        err, ref = float((got - want).abs().max()), float(want.abs().max())
        print(f'L={L} stage {k} with_p={with_p} {name}: max |got - want| = {err:.3e}, max |want| = {ref:.3e}')
        assert ref > 0.0
        assert err <= 2e-11 * max(1.0, ref), (L, k, with_p, name)


# ------------------------------------------------------------------ flow_autograd
@functools.lru_cache(maxsize=None)
def flow_reference(L, nsteps, eps):
    """links, weight cases and the yardstick's cotangents of (w . clover_sums(flow(x))).sum(): once"""
    x = ch.random_links(NB, L, 61)
    xg = x.clone().requires_grad_(True)
    sums = fr.clover_sums(fr.flow(xg, eps, nsteps))[0]
    ws = ch.weight_cases(NB, 29)
    wants = [torch.autograd.grad((w * sums).sum(), xg, retain_graph=True)[0] for w in ws]
    return x, ws, wants


def flowed_sums(lat, x, t, eps):
    from l2hmc import _autograd as AG
    return AG.SU3CloverSums.apply(lat.flow_autograd(x, t, eps), lat._lattice_shape)


@pytest.mark.parametrize('L,nsteps,eps', FLOWS)
def test_flow_autograd_vs_restatement(ops, L, nsteps, eps):
    """measured on the MI355X (profiles/su3_flow_bwd.md): the worst case of each lattice is printed below"""
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    x, ws, wants = flow_reference(L, nsteps, eps)
    lat = LatticeSU3(NB, list(L))
    xd = dev(x)
    plain = lat.flow(xd, nsteps * eps, eps)
    assert torch.equal(lat.flow_autograd(xd, nsteps * eps, eps), plain)
    xg = xd.clone().requires_grad_(True)
    y = lat.flow_autograd(xg, nsteps * eps, eps)
    assert torch.equal(y.detach(), plain) and y.requires_grad          # the forward value: the bits of flow()
    sums = flowed_sums(lat, xg, nsteps * eps, eps)
    assert torch.equal(sums.detach(), ops.su3_clover_sums_n(ops.su3_pack(plain), L))
    for i, (w, want) in enumerate(zip(ws, wants)):
        (got,) = torch.autograd.grad((dev(w) * sums).sum(), xg, retain_graph=True)
        err, ref = float((host(got) - want).abs().max()), float(want.abs().max())
        print(f'L={L} {nsteps} x {eps} w#{i}: max |got - want| = {err:.3e}, max |want| = {ref:.3e}, '
              f'bound {3 * nsteps * 2e-11 * max(1.0, ref):.3e}')
        assert ref > 0.0
        assert err <= 3 * nsteps * 2e-11 * max(1.0, ref), (L, i)


def test_no_flow_step_is_the_clover_gradient(ops):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L = (3, 4, 4, 8)
    lat = LatticeSU3(NB, list(L))
    xd = dev(ch.random_links(NB, L, 23))
    w = dev(ch.weight_cases(NB, 29)[3])
    grads = []
    for kw in ({}, dict(flow_time=0.0, eps=0.02)):
        xg = xd.clone().requires_grad_(True)
        assert lat.flow_autograd(xg, 0.0, 0.02) is xg
        o = lat.clover_autograd(xg, **kw)
        grads.append(torch.autograd.grad((w[:, 0] * o.E + w[:, 1] * o.Q + w[:, 2] * o.Eplaq).sum(), xg)[0])
    assert float(grads[0].abs().max()) > 0.0
    assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize('L', [(3, 5, 2, 7), (4, 4, 4, 4)])
def test_flow_autograd_gauge_covariance(ops, L):
    """the flowed clover sums are gauge invariant, so the cotangent at x^g is the cotangent at x rotated like a
    link: g(x) gx_mu(x) g(x + mu)^H"""
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    lat = LatticeSU3(NB, list(L))
    x = ch.random_links(NB, L, 23)
    w = dev(ch.weight_cases(NB, 29)[3])
    g = fr.rand_su3((NB, *L), 3.0, torch.Generator().manual_seed(9))

    def grad_at(xx):
        xg = dev(xx).requires_grad_(True)
        (gx,) = torch.autograd.grad((w * flowed_sums(lat, xg, 2 * EPS, EPS)).sum(), xg)
        return host(gx)
    gx, gxr = grad_at(x), grad_at(fr.gauge_rotate(x, g))
    err, ref = float((gxr - fr.gauge_rotate(gx, g)).abs().max()), float(gx.abs().max())
    print(f'L={L}: gauge covariance max |d| = {err:.3e}, max |gx| = {ref:.3e}')
    assert ref > 0.0
    assert err <= 1e-12 * ref                               # test_clover_bwd_gauge_covariance's tolerance


# ------------------------------------------------------------------ the train step
def _su3_train_step(g, route, **charge):
    """(loss, {parameter: grad}) of the su3_train fixture's step with the charge term on the clover charge"""
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch import training as T
    from l2hmc.loss.pytorch.loss import LatticeLoss
    dyn, lat, _ = helpers.build_su3_train_dynamics(g)
    loss_fn = LatticeLoss(lat, cfgs.LossConfig(
        use_mixed_loss=bool(g['use_mixed_loss']), charge_weight=float(g['charge_weight']),
        plaq_weight=float(g['plaq_weight']), rmse_weight=float(g['rmse_weight']), charge_kind='clover', **charge))
    assert float(g['charge_weight']) > 0
    dyn._inject = {'normals': g['normals'], 'u': g['u']}
    beta = torch.tensor(float(g['beta']))
    xin = dyn.g.compat_proj(dyn.unflatten(torch.from_numpy(g['x']).to(dyn.device)))
    if route == 'product':
        T.ParamArena(dyn).zero_grad()
        _, _, loss = T.train_forward_backward(dyn, loss_fn, xin, beta)
    else:
        xin.requires_grad_(True)
        _, m = dyn((xin, beta))
        loss = loss_fn(x_init=xin, x_prop=m['mc_states'].proposed.x, acc=m['acc'])
        loss.backward()
    dyn._inject = None
    return float(loss.detach()), {k: host(p.grad) for k, p in dyn.named_parameters() if p.grad is not None}


def test_su3_train_step_on_the_flowed_clover_charge(golden, f64, monkeypatch):
    from l2hmc import _ops
    g = golden('su3_train')
    flow = dict(charge_flow_time=0.04, charge_flow_eps=0.02)
    loss_p, g_p = _su3_train_step(g, 'product', **flow)
    loss_a, g_a = _su3_train_step(g, 'autograd', **flow)
    assert np.isfinite(loss_p) and abs(loss_p - loss_a) <= 1e-7 * abs(loss_a), (loss_p, loss_a)
    assert len(g_a) > 0 and set(g_a) <= set(g_p)
    assert all(not v.any() for k, v in g_p.items() if k not in g_a)
    gn = np.sqrt(sum(float((v ** 2).sum()) for v in g_a.values()))
    worst = 0.0
    for k, v in g_a.items():
        scale = max(float(v.abs().max()), 1e-6 * gn)         # check_train_step's grad_rel, atol_rel = 1e-6
        worst = max(worst, float((g_p[k] - v).abs().max()) / scale)
    print(f'flowed clover train step: loss = {loss_p:.6g}, grad_rel (product vs autograd) = {worst:.3e}')
    assert worst < 1e-5                                      # test_su3_train_step_on_the_clover_charge's bound
    # no flow time: the clover step as it was, bit for bit, and no flow kernel launched
    loss_c, g_c = _su3_train_step(g, 'product')
    launched = []
    for name in ('su3_flow_step_n', 'su3_flow_step_bwd_n', 'su3_force_vjp_'):
        monkeypatch.setattr(_ops, name, lambda *a, _n=name, **k: launched.append(_n))
    loss_0, g_0 = _su3_train_step(g, 'product', charge_flow_time=0.0, charge_flow_eps=0.02)
    assert launched == []
    assert loss_0 == loss_c and set(g_0) == set(g_c) and all(torch.equal(g_0[k], g_c[k]) for k in g_c)
    # the term is live: both routes differ from the unflowed step
    top = max(float(v.abs().max()) for v in g_c.values())
    for loss_f, g_f in ((loss_p, g_p), (loss_a, g_a)):
        assert abs(loss_f - loss_c) > 1e-6 * abs(loss_c)
        assert max(float((g_f[k] - g_c[k]).abs().max()) for k in g_f) > 1e-3 * top
