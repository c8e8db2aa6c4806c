"""CPU tests of training with `activation_fn=swish` through a conv stack and in half precision (host side:
tape, reverse sweep, Adam) against the reference's swish fixtures (tests/golden/make_golden_swish.py), with
the libl2q.so entry points replaced by the torch restatement in tests/emu_native.py plus the two entry
points of tests/swish_helpers.py.  Tolerances are those of the leaky_relu twins (test_train_emu.py,
test_conv_f64_emu.py).  The kernels themselves are checked on the GPU (test_swish_train_gpu.py)."""
import numpy as np
import pytest
import torch

import emu_native
import helpers
from f64conv_helpers import install_emu_f64, train_fixture
from swish_helpers import install_emu_swish

cpu_only = pytest.mark.skipif(torch.cuda.is_available(), reason='host-logic test for the CPU container')


@pytest.fixture(autouse=True)
def _f32_default():
    torch.set_default_dtype(torch.float32)       # (conftest puts the previous default back)
    yield


@cpu_only
@pytest.mark.parametrize('autograd', [False, True], ids=['trainer', 'autograd'])
def test_swish_train_step_host_logic_conv_f32(autograd, golden, monkeypatch):
    g = golden('u1_train_swish_conv')
    assert str(g['activation']) == 'swish'
    emu_native.install(monkeypatch)
    install_emu_swish(monkeypatch)
    dyn, lat, loss_fn = helpers.build_u1_train_dynamics(g)
    out = helpers.check_train_step(g, dyn, loss_fn, rtol=2e-4, atol_rel=1e-3,
                                   adam_min_grad=1e-3, autograd=autograd)
    assert out['grad_rel'] < 2e-2, out
    assert out['param_abs'] < 2e-5, out


@cpu_only
@pytest.mark.parametrize('autograd', [False, True], ids=['trainer', 'autograd'])
def test_swish_train_step_host_logic_conv_f64(autograd, golden, monkeypatch):
    torch.set_default_dtype(torch.float64)
    g = train_fixture(golden, 'u1_train_swish_conv_f64')
    assert str(g['activation']) == 'swish'
    emu_native.install(monkeypatch)
    install_emu_f64(monkeypatch)
    install_emu_swish(monkeypatch)
    dyn, lat, loss_fn = helpers.build_u1_train_dynamics(g)
    out = helpers.check_train_step(g, dyn, loss_fn, rtol=1e-9, atol_rel=1e-6, autograd=autograd)
    assert out['grad_rel'] < 1e-7, out
    assert out['param_abs'] < 1e-7, out


@cpu_only
@pytest.mark.parametrize('route', ['trainer', 'autograd'])
@pytest.mark.parametrize('name', ['u1_train_swish_fp16_conv', 'u1_train_swish_bf16'])
def test_swish_half_precision_train_step_host_logic(name, route, golden, monkeypatch):
    """autocast + GradScaler training with swish against the real reference run that way: accept masks
    bit-equal, gradients within twice the reference's own 16-bit-vs-fp32 distance."""
    g = golden(name)
    assert str(g['activation']) == 'swish'
    emu_native.install(monkeypatch)
    install_emu_swish(monkeypatch)
    out = helpers.check_half_train_step(g, route)
    print(name, route, out)
    helpers.assert_half_train_step(g, name, route, out)


@cpu_only
@pytest.mark.parametrize('extra', [[], ['precision=fp16', 'conv=none']], ids=['conv_f32', 'dense_fp16'])
def test_trainer_train_step_swish_host_logic(extra, monkeypatch):
    """Trainer(cfg).train_step with network.activation_fn=swish: the default conv network in fp32, and
    the dense network at precision=fp16 -- finite losses, the parameters move, evaluation still runs."""
    import l2hmc.configs as cfgs
    from l2hmc.trainers.pytorch.trainer import Trainer
    emu_native.install(monkeypatch)
    install_emu_swish(monkeypatch)
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = cfgs.get_config(['dynamics.group=U1', 'dynamics.latvolume=[4,4]', 'dynamics.nchains=8',
                           'dynamics.nleapfrog=2', 'dynamics.verbose=false', 'network.units=[8,8]',
                           'network.activation_fn=swish'] + extra)
    tr = Trainer(cfg)
    x = tr.warmup(beta=2.0, nsteps=2)
    before = {k: v.detach().clone() for k, v in tr.dynamics.named_parameters()}
    for _ in range(2):
        x, m = tr.train_step((x, 2.0))
        assert np.isfinite(float(m['loss'])), m
    moved = sum(int(not torch.equal(p.detach(), before[k])) for k, p in tr.dynamics.named_parameters())
    assert moved >= 0.9 * len(before), (moved, len(before))
    _, me = tr.eval_step((x, 2.0))
    assert torch.isfinite(me['acc']).all()
