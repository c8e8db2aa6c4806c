"""GPU tier of the differentiable clover sums: l2q_su3_clover_bwd against torch.autograd of the restatement
tests/flow_restatement.clover_sums (computed on the CPU), its determinism and gauge covariance, the autograd node
and the loss on top of it, and the SU(3) train step on the clover charge."""
import functools

import numpy as np
import pytest
import torch

import clover_helpers as ch
import flow_restatement as fr
import helpers

pytestmark = pytest.mark.gpu

NB = 3
# extents 1 and 2, no whole workgroup, several workgroups per chain; the last two are whole 64-site spatial tiles,
# where the forward behind SU3CloverSums takes its slice-resident kernel (the VJP has one variant)
LATTICES = [(1, 3, 2, 5), (3, 5, 2, 7), (2, 5, 8, 8), (4, 4, 4, 4), (3, 4, 4, 8)]


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


@functools.lru_cache(maxsize=None)
def reference(L):
    """links, weight cases and the yardstick's cotangents (native layout) of one lattice: computed once"""
    x = ch.random_links(NB, L, 23)
    xg = x.clone().requires_grad_(True)
    sums = fr.clover_sums(xg)[0]
    ws = ch.weight_cases(NB, 29)
    wants = [ch.native(torch.autograd.grad((w * sums).sum(), xg, retain_graph=True)[0]) for w in ws]
    return x, ws, wants


def run(ops, x, w, L, g0=None):
    xn = ops.su3_pack(dev(x))
    gx = torch.zeros_like(xn) if g0 is None else dev(g0)
    ops.su3_clover_bwd_(gx, xn, dev(w), L)
    return host(gx)


@pytest.mark.parametrize('L', LATTICES)
def test_clover_bwd_vs_autograd(ops, L):
    x, ws, wants = reference(L)
    V = int(np.prod(L))
    rng = np.random.default_rng(31)
    for i, (w, want) in enumerate(zip(ws, wants)):
        g0 = torch.from_numpy(rng.normal(size=(NB, 4, 9, V)) + 1j * rng.normal(size=(NB, 4, 9, V)))
        got = run(ops, x, w, L, g0)                      # gx += : starts from g0
        err, ref = float((got - (g0 + want)).abs().max()), float(want.abs().max())
        print(f'L={L} w#{i}: max |got - want| = {err:.3e}, max |want| = {ref:.3e}')
        assert ref > 0.0
        assert err <= 1e-12 * max(1.0, ref), (L, i)


@pytest.mark.parametrize('L', LATTICES)
def test_clover_bwd_is_deterministic_and_batch_independent(ops, L):
    x, ws, _ = reference(L)
    w = ws[3]
    a, b = run(ops, x, w, L), run(ops, x, w, L)
    assert torch.equal(a, b)
    for k in range(NB):
        alone = run(ops, x[k:k + 1], w[k:k + 1], L)
        assert torch.equal(alone[0], a[k]), k


@pytest.mark.parametrize('L', [(3, 5, 2, 7), (4, 4, 4, 4)])
def test_clover_bwd_gauge_covariance(ops, L):
    """the sums are gauge invariant, so the cotangent at x^g is the cotangent at x rotated like a link:
    g(x) gx_mu(x) g(x + mu)^H"""
    x, ws, _ = reference(L)
    w = ws[3]
    g = fr.rand_su3((NB, *L), 3.0, torch.Generator().manual_seed(9))
    unpack = lambda gn: gn.permute(0, 1, 3, 2).reshape(NB, 4, *L, 3, 3)
    gx = unpack(run(ops, x, w, L))
    gxr = unpack(run(ops, fr.gauge_rotate(x, g), w, L))
    err, ref = float((gxr - fr.gauge_rotate(gx, g)).abs().max()), float(gx.abs().max())
    print(f'L={L}: gauge covariance max |d| = {err:.3e}, max |gx| = {ref:.3e}')
    assert err <= 1e-12 * ref


def test_autograd_through_lattice_and_loss(ops, f64):
    import l2hmc.configs as cfgs
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.loss.pytorch.loss import LatticeLoss
    L = (3, 4, 4, 8)
    x, _, _ = reference(L)
    V = int(np.prod(L))
    lat = LatticeSU3(NB, list(L))
    xd = dev(x)
    plain = lat.clover(xd)
    a, b, c = (dev(torch.from_numpy(np.random.default_rng(k).normal(size=NB))) for k in (1, 2, 3))
    xg = xd.clone().requires_grad_(True)
    o = lat.clover_autograd(xg)
    for got, ref in zip(o, plain):
        assert torch.equal(got.detach(), ref)
    for got, ref in zip(lat.clover_autograd(xd), plain):
        assert torch.equal(got, ref) and not got.requires_grad
    (got,) = torch.autograd.grad((a * o.E + b * o.Q + c * o.Eplaq).sum(), xg)
    # the same seeded by hand: E = s0 / V, Q = s1 / 4 pi^2, Eplaq = 36 - 2 s2 / V
    w = torch.stack([a / V, b / (4 * np.pi ** 2), -(2.0 / V) * c], 1)
    xn = ops.su3_pack(xd)
    want = ops.su3_unpack(ops.su3_clover_bwd_(torch.zeros_like(xn), xn, w, L), L)
    # (1e-14: autograd's own seed may differ from this one in the last bit)
    assert got.shape == xd.shape
    assert float((got - want.reshape(got.shape)).abs().max()) <= 1e-14 * float(want.abs().max())
    with pytest.raises(RuntimeError, match='no autograd'):
        lat.clover(xd.clone().requires_grad_(True))
    # charge_loss on the clover charge: d loss / d x_prop = the kernel seeded with d loss / d Q
    x1 = dev(ch.random_links(NB, L, 37))
    acc = dev(torch.tensor([0.3, 0.9, 0.6]))
    loss_fn = LatticeLoss(lat, cfgs.LossConfig(use_mixed_loss=True, charge_weight=0.1, charge_kind='clover'))
    x1g = x1.clone().requires_grad_(True)
    loss = loss_fn.charge_loss(xd, x1g, acc)
    (got,) = torch.autograd.grad(loss, x1g)
    q0 = plain.Q
    q1 = lat.clover(x1).Q.clone().requires_grad_(True)
    by_hand = loss_fn._mixed(acc * (q1 - q0) ** 2, loss_fn.charge_weight, None)
    assert float((by_hand - loss).detach().abs()) <= 1e-14 * float(loss.detach().abs())
    (gq,) = torch.autograd.grad(by_hand, q1)
    w = torch.zeros(NB, 3, dtype=torch.float64, device=gq.device)
    w[:, 1] = gq / (4 * np.pi ** 2)
    x1n = ops.su3_pack(x1)
    want = ops.su3_unpack(ops.su3_clover_bwd_(torch.zeros_like(x1n), x1n, w, L), L).reshape(got.shape)
    assert float(want.abs().max()) > 0.0
    assert float((got - want).abs().max()) <= 1e-14 * float(want.abs().max())


def _su3_train_step(g, route, kind):
    """(loss, {parameter: grad}) of the su3_train fixture's step with the charge term on `kind`"""
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch import training as T
    from l2hmc.loss.pytorch.loss import LatticeLoss
    dyn, lat, _ = helpers.build_su3_train_dynamics(g)
    loss_fn = LatticeLoss(lat, cfgs.LossConfig(
        use_mixed_loss=bool(g['use_mixed_loss']), charge_weight=float(g['charge_weight']),
        plaq_weight=float(g['plaq_weight']), rmse_weight=float(g['rmse_weight']), charge_kind=kind))
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


def test_su3_train_step_on_the_clover_charge(golden, f64):
    g = golden('su3_train')
    loss_p, g_p = _su3_train_step(g, 'product', 'clover')
    loss_a, g_a = _su3_train_step(g, 'autograd', 'clover')
    assert np.isfinite(loss_p) and abs(loss_p - loss_a) <= 1e-7 * abs(loss_a), (loss_p, loss_a)
    assert len(g_a) > 0 and set(g_a) <= set(g_p)
    assert all(not v.any() for k, v in g_p.items() if k not in g_a)
    gn = np.sqrt(sum(float((v ** 2).sum()) for v in g_a.values()))
    worst = 0.0
    for k, v in g_a.items():
        scale = max(float(v.abs().max()), 1e-6 * gn)         # check_train_step's grad_rel, atol_rel = 1e-6
        worst = max(worst, float((g_p[k] - v).abs().max()) / scale)
    print(f'clover train step: loss = {loss_p:.6g}, grad_rel (product vs autograd) = {worst:.3e}')
    assert worst < 1e-5                                      # test_su3_train_step_matches_reference's bound
    loss_q, g_q = _su3_train_step(g, 'product', 'plaq')
    assert abs(loss_q - loss_p) > 1e-6 * abs(loss_p)
    assert max(float((g_q[k] - g_p[k]).abs().max()) for k in g_p) \
        > 1e-3 * max(float(v.abs().max()) for v in g_p.values())


@pytest.mark.parametrize('autograd', [False, True], ids=['trainer', 'autograd'])
def test_su3_train_step_charge_kind_plaq_meets_the_golden_values(autograd, golden, f64):
    import l2hmc.configs as cfgs
    from l2hmc.loss.pytorch.loss import LatticeLoss
    g = golden('su3_train')
    dyn, lat, _ = helpers.build_su3_train_dynamics(g)
    loss_fn = LatticeLoss(lat, cfgs.LossConfig(
        use_mixed_loss=bool(g['use_mixed_loss']), charge_weight=float(g['charge_weight']),
        plaq_weight=float(g['plaq_weight']), rmse_weight=float(g['rmse_weight']), charge_kind='plaq'))
    out = helpers.check_train_step(g, dyn, loss_fn, rtol=1e-7, atol_rel=1e-6, adam_min_grad=1e-6, autograd=autograd)
    assert out['grad_rel'] < 1e-5, out
    assert out['param_abs'] < 1e-6, out
