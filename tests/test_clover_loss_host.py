"""CPU tier of the clover charge loss: LossConfig.charge_kind, LatticeSU3.clover_autograd, LatticeLoss and the
reverse sweep's clover seed, with the libl2q.so entry points replaced by torch restatements (tests/emu_native.py,
tests/clover_helpers.py).  The kernel behind it is checked in test_clover_bwd_emu.py and test_clover_bwd_gpu.py."""
import numpy as np
import pytest
import torch

import clover_helpers as ch
import emu_native
import flow_restatement as fr

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason='host-logic tests for the CPU container')


@pytest.fixture
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


@pytest.fixture
def emu(monkeypatch):
    emu_native.install(monkeypatch)
    ch.install_emu_clover(monkeypatch)


def test_charge_kind_config():
    import l2hmc.configs as cfgs
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.lattice.u1.pytorch.lattice import LatticeU1
    from l2hmc.loss.pytorch.loss import LatticeLoss
    plain = cfgs.LossConfig(charge_weight=0.1)
    assert plain.charge_kind == 'plaq'
    assert plain.to_str() == 'qw-0.1_pw-0.0_rw-0.0_aw-0.0_mixed-False'            # as before the field existed
    assert cfgs.LossConfig(charge_weight=0.1, charge_kind='plaq').to_str() == plain.to_str()
    assert cfgs.LossConfig(charge_weight=0.1, charge_kind='clover').to_str() == plain.to_str() + '_qk-clover'
    with pytest.raises(ValueError):
        cfgs.LossConfig(charge_kind='wilson')
    with pytest.raises(ValueError):
        LatticeLoss(LatticeU1(2, [4, 4]), cfgs.LossConfig(charge_kind='clover'))
    # a config whose field was changed after construction is still refused where it is used
    bad = cfgs.LossConfig()
    bad.charge_kind = 'wilson'
    with pytest.raises(ValueError):
        LatticeLoss(LatticeSU3(2, [2, 2, 2, 2]), bad)
    assert LatticeLoss(LatticeU1(2, [4, 4]), cfgs.LossConfig()).charge_kind == 'plaq'
    assert LatticeLoss(LatticeSU3(2, [2, 2, 2, 2]), cfgs.LossConfig(charge_kind='clover')).charge_kind == 'clover'


@pytest.mark.parametrize('loss', ['default', 'su3'])
def test_charge_kind_command_line_override(loss):
    import l2hmc.configs as cfgs
    base = ['dynamics.group=SU3', 'dynamics.latvolume=[2,2,2,2]', 'dynamics.nchains=2', f'loss={loss}']
    assert cfgs.instantiate(cfgs.get_config(base)).loss.charge_kind == 'plaq'
    cfg = cfgs.instantiate(cfgs.get_config(base + ['loss.charge_kind=clover']))
    assert isinstance(cfg.loss, cfgs.LossConfig) and cfg.loss.charge_kind == 'clover'
    assert cfg.loss.to_str().endswith('_qk-clover')
    with pytest.raises(ValueError):
        cfgs.instantiate(cfgs.get_config(base + ['loss.charge_kind=wilson']))


def test_clover_autograd_vs_restatement(emu, f64):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L, nb = [2, 2, 2, 4], 2
    lat = LatticeSU3(nb, L)
    x = ch.random_links(nb, L, 5)
    e, q = fr.clover_obs(x)
    ep = fr.plaq_energy(x)
    plain = lat.clover(x)
    for c in (lat.clover_autograd(x), lat.clover_autograd(x.clone().requires_grad_(True))):
        for got, want, ref in ((c.E, e, plain.E), (c.Q, q, plain.Q), (c.Eplaq, ep, plain.Eplaq)):
            assert float((got.detach() - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
            assert torch.equal(got.detach(), ref)
    assert not lat.clover_autograd(x).Q.requires_grad
    # differentiable: d (a . E + b . Q + c . Eplaq) / dx against autograd of the restatement
    a, b, c = (torch.from_numpy(np.random.default_rng(k).normal(size=nb)) for k in (1, 2, 3))
    xg = x.clone().requires_grad_(True)
    o = lat.clover_autograd(xg)
    (got,) = torch.autograd.grad((a * o.E + b * o.Q + c * o.Eplaq).sum(), xg)
    xr = x.clone().requires_grad_(True)
    er, qr = fr.clover_obs(xr)
    (want,) = torch.autograd.grad((a * er + b * qr + c * fr.plaq_energy(xr)).sum(), xr)
    assert got.shape == x.shape
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    # the observables that are not differentiable still say so
    for name in ('clover', 'topological_charge', 'energy_density'):
        with pytest.raises(RuntimeError, match='no autograd'):
            getattr(lat, name)(x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match='no autograd'):
        lat.flow(x.clone().requires_grad_(True), 0.02, eps=0.02)
    with pytest.raises(RuntimeError, match='no autograd'):
        lat.flow_observables(x.clone().requires_grad_(True), [0.02], eps=0.02)


def test_charge_loss_uses_the_clover_charge(emu, f64):
    import l2hmc.configs as cfgs
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.loss.pytorch.loss import LatticeLoss
    L, nb = [2, 2, 2, 4], 2
    lat = LatticeSU3(nb, L)
    x0, x1 = ch.random_links(nb, L, 5), ch.random_links(nb, L, 6)
    acc = torch.tensor([0.3, 0.9])
    for mixed in (False, True):
        kw = dict(use_mixed_loss=mixed, charge_weight=0.1)
        clover = LatticeLoss(lat, cfgs.LossConfig(charge_kind='clover', **kw))
        plaq = LatticeLoss(lat, cfgs.LossConfig(**kw))
        dq2 = acc * (fr.clover_obs(x1)[1] - fr.clover_obs(x0)[1]) ** 2
        want = (0.1 / (dq2 + 1e-4) - (dq2 + 1e-4) / 0.1).mean() if mixed else (-dq2 / 0.1).mean()
        for got in (clover.charge_loss(x0, x1, acc), clover.calc_loss(x0, x1, acc)):
            assert float((got - want).abs()) <= 1e-6 * float(want.abs())      # (the weight is a float32 tensor)
        assert float((plaq.charge_loss(x0, x1, acc) - want).abs()) > 1e-3 * float(want.abs())
        # _charge_loss is the reference's helper on plaquette sums, whatever the kind
        w0, w1 = lat.plaq_sums(x0), lat.plaq_sums(x1)
        assert torch.equal(clover._charge_loss(w0, w1, acc), plaq._charge_loss(w0, w1, acc))
        assert torch.equal(plaq._charge_loss(w0, w1, acc), plaq.charge_loss(x0, x1, acc))


OV = ['dynamics.group=SU3', 'dynamics.latvolume=[2,2,2,2]', 'dynamics.nchains=4',
      'dynamics.nleapfrog=1', 'dynamics.eps=0.02', 'dynamics.verbose=false',
      'dynamics.use_split_xnets=false', 'dynamics.use_separate_networks=false',
      'network.units=[4]', 'network.dropout_prob=0.0', 'network.use_batch_norm=false',
      'network.activation_fn=tanh', 'loss.aux_weight=0.0', 'learning_rate.clip_norm=0.0',
      'conv=none', 'loss.charge_weight=0.1']


def _train_step(kind, route):
    """(loss, {parameter: grad}) of one SU(3) train step on identical inputs"""
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch import training as T
    from l2hmc.trainers.pytorch.trainer import Trainer
    torch.manual_seed(1)
    np.random.seed(1)
    tr = Trainer(cfgs.get_config(OV + [f'loss.charge_kind={kind}']))
    dyn, loss_fn = tr.dynamics, tr.loss_fn
    assert loss_fn.charge_kind == kind
    dyn.train()
    x = dyn.g.compat_proj(tr.lattice.random())
    nrm = torch.randn(8, 4, 4, 2, 2, 2, 2, generator=torch.Generator().manual_seed(7))
    dyn._inject = {'normals': nrm.numpy(), 'u': np.full(4, 0.5)}
    beta = torch.tensor(6.0)
    if route == 'product':
        T.ParamArena(dyn).zero_grad()
        _, _, loss = T.train_forward_backward(dyn, loss_fn, x, beta)
    else:
        x.requires_grad_(True)
        _, m = dyn((x, beta))
        loss = loss_fn(x_init=x, x_prop=m['mc_states'].proposed.x, acc=m['acc'])
        loss.backward()
    dyn._inject = None
    grads = {k: p.grad.detach().clone() for k, p in dyn.named_parameters() if p.grad is not None}
    return float(loss.detach()), grads


def test_su3_train_step_on_the_clover_charge(emu, f64, monkeypatch):
    from l2hmc import _ops as ops
    calls = []
    inner = ops.su3_clover_bwd_
    monkeypatch.setattr(ops, 'su3_clover_bwd_', lambda *a: (calls.append(1), inner(*a))[1])
    loss_p, g_p = _train_step('clover', 'product')
    assert len(calls) == 1                                  # the reverse sweep's seed
    loss_a, g_a = _train_step('clover', 'autograd')
    assert len(calls) == 3                                  # SU3CloverSums.backward of x_init (a leaf here) and x_prop
    assert np.isfinite(loss_p) and abs(loss_p - loss_a) <= 1e-7 * abs(loss_a)
    # (the arena gives every parameter a gradient; what autograd leaves None is zero there)
    assert len(g_a) > 0 and set(g_a) <= set(g_p)
    assert all(not g.any() for k, g in g_p.items() if k not in g_a)
    gn = np.sqrt(sum(float((g ** 2).sum()) for g in g_a.values()))
    worst = 0.0
    for k, g in g_a.items():
        scale = max(float(g.abs().max()), 1e-6 * gn)        # check_train_step's grad_rel, atol_rel = 1e-6
        worst = max(worst, float((g_p[k] - g).abs().max()) / scale)
    print(f'clover train step: loss = {loss_p:.6g}, grad_rel (product vs autograd) = {worst:.3e}')
    assert worst <= 1e-7
    # the term is wired: another charge, another gradient; and 'plaq' launches nothing new
    loss_q, g_q = _train_step('plaq', 'product')
    assert len(calls) == 3
    assert abs(loss_q - loss_p) > 1e-6 * abs(loss_p)
    assert max(float((g_q[k] - g_p[k]).abs().max()) for k in g_p) \
        > 1e-3 * max(float(g.abs().max()) for g in g_p.values())
