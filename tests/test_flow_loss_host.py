"""CPU tier of the differentiable Wilson flow: the argument checks of the new entry points, LossConfig.charge_flow_time,
LatticeSU3.flow_autograd / clover_autograd(flow_time=), LatticeLoss on the flowed clover charge and the trainer's
reverse sweep through the flow, with the libl2q.so entry points replaced by torch restatements (tests/emu_native.py,
tests/clover_helpers.py, tests/flow_helpers.py).  The kernel behind it is checked in test_flow_bwd_emu.py and
test_flow_bwd_gpu.py."""
import numpy as np
import pytest
import torch

import clover_helpers as ch
import emu_native
import flow_helpers as fh
import flow_restatement as fr


@pytest.fixture
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


@pytest.fixture
def emu(monkeypatch):
    if torch.cuda.is_available():
        pytest.skip('host-logic tests for the CPU container')
    emu_native.install(monkeypatch)
    ch.install_emu_clover(monkeypatch)
    fh.install_emu_flow(monkeypatch)


def test_flow_bwd_symbols_and_argument_errors():
    from l2hmc import native
    lib = native.load()
    for name in ('l2q_su3_force_vjp', 'l2q_su3_flow_stage_bwd', 'l2q_su3_flow_step_bwd',
                 'l2q_su3_flow_stage_bwd_ws_bytes', 'l2q_su3_flow_step_bwd_ws_bytes'):
        assert hasattr(lib, name) and name in native.SIGNATURES
    # (addresses are never dereferenced: every check below comes before any HIP call)
    x, p, g, h, k, w = 4096, 8192, 12288, 16384, 20480, 24576
    big = 1 << 30

    def bad(rc, text, code=-1):
        assert rc == code and text in lib.l2q_last_error(), (rc, lib.l2q_last_error())
    bad(lib.l2q_su3_force_vjp(None, g, 3.0, h, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(lib.l2q_su3_force_vjp(x, None, 3.0, h, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(lib.l2q_su3_force_vjp(x, g, 3.0, None, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(lib.l2q_su3_force_vjp(x, g, 3.0, h, 1, 2, 0, 2, 2, None), b'size')
    bad(lib.l2q_su3_force_vjp(x, g, 3.0, x, 1, 2, 2, 2, 2, None), b'alias')
    bad(lib.l2q_su3_force_vjp(x, g, 3.0, g, 1, 2, 2, 2, 2, None), b'alias')
    bad(lib.l2q_su3_flow_stage_bwd(x, p, 1.0, 0.1, g, h, None, 1, 2, 2, 2, 2, w, big, None), b'null pointer')
    bad(lib.l2q_su3_flow_stage_bwd(x, p, 1.0, 0.1, g, h, k, 1, 2, 2, 2, 2, None, big, None), b'null pointer')
    bad(lib.l2q_su3_flow_stage_bwd(x, p, 1.0, 0.1, g, h, k, 0, 2, 2, 2, 2, w, big, None), b'size')
    bad(lib.l2q_su3_flow_stage_bwd(x, p, 1.0, 0.1, g, h, g, 1, 2, 2, 2, 2, w, big, None), b'alias')
    bad(lib.l2q_su3_flow_stage_bwd(x, p, 1.0, 0.1, g, g, k, 1, 2, 2, 2, 2, w, big, None), b'alias')
    bad(lib.l2q_su3_flow_step_bwd(None, 0.1, g, k, 1, 2, 2, 2, 2, w, big, None), b'null pointer')
    bad(lib.l2q_su3_flow_step_bwd(x, 0.1, g, k, 1, 2, 2, -2, 2, w, big, None), b'size')
    bad(lib.l2q_su3_flow_step_bwd(x, 0.1, g, x, 1, 2, 2, 2, 2, w, big, None), b'alias')
    # the workspace: seven fields and the stage's scratch, less than eight fields; one byte short is refused
    for nb, L in ((1, (2, 2, 2, 2)), (3, (1, 3, 2, 5)), (256, (8, 8, 8, 8))):
        V = int(np.prod(L))
        field = nb * 36 * V * 16
        stage = lib.l2q_su3_flow_stage_bwd_ws_bytes(nb, *L)
        step = lib.l2q_su3_flow_step_bwd_ws_bytes(nb, *L)
        assert stage == nb * (1 + 4 * ((V + 255) // 256)) * 8
        assert step == 7 * field + stage and step <= 8 * field
        bad(lib.l2q_su3_flow_stage_bwd(x, p, 1.0, 0.1, g, h, k, nb, *L, w, stage - 1, None), b'workspace', -2)
        bad(lib.l2q_su3_flow_step_bwd(x, 0.1, g, k, nb, *L, w, step - 1, None), b'workspace', -2)
    assert lib.l2q_su3_flow_step_bwd_ws_bytes(0, 2, 2, 2, 2) == 0


def test_charge_flow_config():
    import l2hmc.configs as cfgs
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.loss.pytorch.loss import LatticeLoss
    plain = cfgs.LossConfig(charge_weight=0.1)
    assert plain.charge_flow_time == 0.0 and plain.charge_flow_eps == 0.01
    assert plain.to_str() == 'qw-0.1_pw-0.0_rw-0.0_aw-0.0_mixed-False'            # as before the fields existed
    clover = cfgs.LossConfig(charge_weight=0.1, charge_kind='clover')
    assert clover.to_str() == plain.to_str() + '_qk-clover'
    assert cfgs.LossConfig(charge_weight=0.1, charge_kind='clover', charge_flow_eps=0.05).to_str() == clover.to_str()
    flowed = cfgs.LossConfig(charge_weight=0.1, charge_kind='clover', charge_flow_time=0.04, charge_flow_eps=0.02)
    assert flowed.to_str() == clover.to_str() + '_qt-0.04'
    for kw in (dict(charge_flow_time=0.04),                                        # needs the clover charge
               dict(charge_kind='plaq', charge_flow_time=0.04, charge_flow_eps=0.02),
               dict(charge_kind='clover', charge_flow_time=-0.02, charge_flow_eps=0.02),
               dict(charge_kind='clover', charge_flow_time=0.03, charge_flow_eps=0.02),
               dict(charge_kind='clover', charge_flow_time=0.04, charge_flow_eps=0.0)):
        with pytest.raises(ValueError):
            cfgs.LossConfig(**kw)
    lat = LatticeSU3(2, [2, 2, 2, 2])
    assert LatticeLoss(lat, clover).charge_flow_steps == 0
    assert LatticeLoss(lat, flowed).charge_flow_steps == 2
    # a config whose fields were changed after construction is still refused where it is used
    for field, value in (('charge_flow_time', 0.03), ('charge_flow_time', -0.02), ('charge_kind', 'plaq')):
        bad = cfgs.LossConfig(charge_kind='clover', charge_flow_time=0.04, charge_flow_eps=0.02)
        setattr(bad, field, value)
        with pytest.raises(ValueError):
            LatticeLoss(lat, bad)


@pytest.mark.parametrize('loss', ['default', 'su3'])
def test_charge_flow_command_line_override(loss):
    import l2hmc.configs as cfgs
    base = ['dynamics.group=SU3', 'dynamics.latvolume=[2,2,2,2]', 'dynamics.nchains=2', f'loss={loss}']
    cfg = cfgs.instantiate(cfgs.get_config(base))
    assert cfg.loss.charge_flow_time == 0.0 and cfg.loss.charge_flow_eps == 0.01
    cfg = cfgs.instantiate(cfgs.get_config(
        base + ['loss.charge_flow_time=0.04', 'loss.charge_flow_eps=0.02', 'loss.charge_kind=clover']))
    assert isinstance(cfg.loss, cfgs.LossConfig)
    assert (cfg.loss.charge_kind, cfg.loss.charge_flow_time, cfg.loss.charge_flow_eps) == ('clover', 0.04, 0.02)
    assert cfg.loss.to_str().endswith('_qk-clover_qt-0.04')
    with pytest.raises(ValueError):
        cfgs.instantiate(cfgs.get_config(base + ['loss.charge_flow_time=0.04', 'loss.charge_flow_eps=0.02']))


def test_flow_autograd_vs_restatement(emu, f64):
    from l2hmc import _autograd as AG
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    L, nb = [2, 2, 2, 4], 2
    lat = LatticeSU3(nb, L)
    x = ch.random_links(nb, L, 5)
    plain = lat.flow(x, 0.04, eps=0.02)
    assert float((plain - fr.flow(x, 0.02, 2)).abs().max()) <= 1e-13
    # without a gradient: the numbers of flow(), no graph; no step: x itself
    got = lat.flow_autograd(x, 0.04, eps=0.02)
    assert torch.equal(got, plain) and not got.requires_grad
    assert lat.flow_autograd(x, 0.0) is x
    xg = x.clone().requires_grad_(True)
    assert lat.flow_autograd(xg, 0.0, eps=0.02) is xg
    with torch.no_grad():
        assert not lat.flow_autograd(xg, 0.04, eps=0.02).requires_grad
    with pytest.raises(ValueError):
        lat.flow_autograd(x, 0.03, eps=0.02)
    with pytest.raises(ValueError):
        lat.flow_autograd(x, -0.02, eps=0.02)
    # with one: the same numbers, the native original attached, and the restatement's gradient
    y = lat.flow_autograd(xg, 0.04, eps=0.02)
    assert torch.equal(y.detach(), plain) and y.requires_grad and y.shape == x.shape
    assert AG.native_of(y) is not None and torch.equal(AG.native_of(y), lat.pack(plain))
    w = torch.from_numpy(np.random.default_rng(3).normal(size=(nb, 3)))
    o = lat.clover_autograd(y)
    a, b, c = w[:, 0], w[:, 1], w[:, 2]
    (got,) = torch.autograd.grad((a * o.E + b * o.Q + c * o.Eplaq).sum(), xg)
    xr = x.clone().requires_grad_(True)
    yr = fr.flow(xr, 0.02, 2)
    er, qr = fr.clover_obs(yr)
    (want,) = torch.autograd.grad((a * er + b * qr + c * fr.plaq_energy(yr)).sum(), xr)
    assert got.shape == x.shape and float(want.abs().max()) > 0.0
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    # the flow matters to the gradient, so the comparison can tell
    e0, q0 = fr.clover_obs(xr)
    (unflowed,) = torch.autograd.grad((a * e0 + b * q0 + c * fr.plaq_energy(xr)).sum(), xr)
    assert float((unflowed - want).abs().max()) > 0.05 * float(want.abs().max())
    # clover_autograd(flow_time=) is the same composition; its default is today's
    xg2 = x.clone().requires_grad_(True)
    o2 = lat.clover_autograd(xg2, flow_time=0.04, eps=0.02)
    (got2,) = torch.autograd.grad((a * o2.E + b * o2.Q + c * o2.Eplaq).sum(), xg2)
    assert torch.equal(got2, got)
    for u, v in zip(lat.clover_autograd(x), lat.clover(x)):
        assert torch.equal(u, v)
    for u, v in zip(lat.clover_autograd(x, flow_time=0.04, eps=0.02), lat.clover(plain)):
        assert torch.equal(u, v)
    # the methods that are not differentiable still say so
    with pytest.raises(RuntimeError, match='no autograd'):
        lat.flow(x.clone().requires_grad_(True), 0.02, eps=0.02)
    with pytest.raises(RuntimeError, match='no autograd'):
        lat.flow_observables(x.clone().requires_grad_(True), 0.02, eps=0.02)
    with pytest.raises(RuntimeError, match='no autograd'):
        lat.clover(x.clone().requires_grad_(True))


def test_charge_loss_uses_the_flowed_clover_charge(emu, f64):
    import l2hmc.configs as cfgs
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.loss.pytorch.loss import LatticeLoss
    L, nb = [2, 2, 2, 4], 2
    lat = LatticeSU3(nb, L)
    x0, x1 = ch.random_links(nb, L, 5), ch.random_links(nb, L, 6)
    acc = torch.tensor([0.3, 0.9])
    for mixed in (False, True):
        kw = dict(use_mixed_loss=mixed, charge_weight=0.1, charge_kind='clover')
        flowed = LatticeLoss(lat, cfgs.LossConfig(charge_flow_time=0.04, charge_flow_eps=0.02, **kw))
        unflowed = LatticeLoss(lat, cfgs.LossConfig(**kw))
        dq2 = acc * (fr.clover_obs(fr.flow(x1, 0.02, 2))[1] - fr.clover_obs(fr.flow(x0, 0.02, 2))[1]) ** 2
        want = (0.1 / (dq2 + 1e-4) - (dq2 + 1e-4) / 0.1).mean() if mixed else (-dq2 / 0.1).mean()
        for got in (flowed.charge_loss(x0, x1, acc), flowed.calc_loss(x0, x1, acc)):
            assert float((got - want).abs()) <= 1e-6 * float(want.abs())      # (the weight is a float32 tensor)
        assert float((unflowed.charge_loss(x0, x1, acc) - want).abs()) > 1e-3 * float(want.abs())
        # differentiable in the proposal
        x1g = x1.clone().requires_grad_(True)
        (got,) = torch.autograd.grad(flowed.charge_loss(x0, x1g, acc), x1g)
        x1r = x1.clone().requires_grad_(True)
        dq2 = acc * (fr.clover_obs(fr.flow(x1r, 0.02, 2))[1] - fr.clover_obs(fr.flow(x0, 0.02, 2))[1]) ** 2
        wt = flowed.charge_weight.to(torch.float64)
        (ref,) = torch.autograd.grad((wt / (dq2 + 1e-4) - (dq2 + 1e-4) / wt).mean() if mixed else (-dq2 / wt).mean(),
                                     x1r)
        assert float(ref.abs().max()) > 0.0
        assert float((got - ref).abs().max()) <= 1e-11 * float(ref.abs().max())


OV = ['dynamics.group=SU3', 'dynamics.latvolume=[2,2,2,2]', 'dynamics.nchains=4',
      'dynamics.nleapfrog=1', 'dynamics.eps=0.02', 'dynamics.verbose=false',
      'dynamics.use_split_xnets=false', 'dynamics.use_separate_networks=false',
      'network.units=[4]', 'network.dropout_prob=0.0', 'network.use_batch_norm=false',
      'network.activation_fn=tanh', 'loss.aux_weight=0.0', 'learning_rate.clip_norm=0.0',
      'conv=none', 'loss.charge_weight=0.1', 'loss.charge_kind=clover', 'loss.charge_flow_eps=0.02']


def _train_step(flow_time, route):
    """(loss, {parameter: grad}) of one SU(3) train step on identical inputs"""
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch import training as T
    from l2hmc.trainers.pytorch.trainer import Trainer
    torch.manual_seed(1)
    np.random.seed(1)
    tr = Trainer(cfgs.get_config(OV + [f'loss.charge_flow_time={flow_time}']))
    dyn, loss_fn = tr.dynamics, tr.loss_fn
    assert loss_fn.charge_flow_steps == round(flow_time / 0.02)
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


def test_su3_train_step_on_the_flowed_clover_charge(emu, f64, monkeypatch):
    from l2hmc import _ops as ops
    calls = []
    inner = ops.su3_flow_step_bwd_n
    monkeypatch.setattr(ops, 'su3_flow_step_bwd_n', lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    loss_p, g_p = _train_step(0.04, 'product')
    assert len(calls) == 2                                  # the reverse sweep: two steps
    loss_a, g_a = _train_step(0.04, 'autograd')
    assert len(calls) == 4                                  # SU3Flow.backward of x_prop; x_init is flowed without a graph
    assert np.isfinite(loss_p) and abs(loss_p - loss_a) <= 1e-7 * abs(loss_a)
    # (the arena gives every parameter a gradient; what autograd leaves None is zero there)
    assert len(g_a) > 0 and set(g_a) <= set(g_p)
    assert all(not g.any() for k, g in g_p.items() if k not in g_a)
    gn = np.sqrt(sum(float((g ** 2).sum()) for g in g_a.values()))
    worst = 0.0
    for k, g in g_a.items():
        scale = max(float(g.abs().max()), 1e-6 * gn)        # check_train_step's grad_rel, atol_rel = 1e-6
        worst = max(worst, float((g_p[k] - g).abs().max()) / scale)
    print(f'flowed clover train step: loss = {loss_p:.6g}, grad_rel (product vs autograd) = {worst:.3e}')
    assert worst <= 1e-7                                    # test_clover_loss_host's bound for the unflowed step
    # the term is live: no flow, another loss and another gradient; and no flow launches nothing new
    loss_0, g_0 = _train_step(0.0, 'product')
    assert len(calls) == 4
    assert abs(loss_0 - loss_p) > 1e-6 * abs(loss_p)
    assert max(float((g_0[k] - g_p[k]).abs().max()) for k in g_p) \
        > 1e-3 * max(float(g.abs().max()) for g in g_p.values())
