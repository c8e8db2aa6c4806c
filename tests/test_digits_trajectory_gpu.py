"""The sampler with its vnet inputs carried as int8 digit images (ops.USE_DIGIT_INPUTS; csrc/digits.hpp) against the
same sampler on fp64 inputs: the digits are those the sliced input layer makes itself, so a trajectory has the
same bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def build(L, nb, verbose):
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.network.pytorch.network import NetworkFactory
    torch.manual_seed(0)
    np.random.seed(0)
    V = int(np.prod(L))
    dc = cfgs.DynamicsConfig(nchains=nb, group='SU3', latvolume=list(L), nleapfrog=2, eps=0.02, eps_hmc=0.02,
                             verbose=verbose, use_split_xnets=False, use_separate_networks=False)
    spec = cfgs.InputSpec(xshape=tuple(dc.xshape), xnet={'x': [32 * V], 'v': [32 * V]},
                          vnet={'x': [32 * V], 'v': [32 * V]})
    nc = cfgs.NetworkConfig(units=[64], activation_fn='tanh', dropout_prob=0.0, use_batch_norm=False)
    lat = LatticeSU3(nb, list(L))
    dyn = Dynamics(lat.action, dc, NetworkFactory(spec, nc, cfgs.ConvolutionConfig())).cuda().eval()
    x = lat.g.compat_proj(lat.random().cuda())
    return dyn, x


def draws(L, nb, seed):
    g = torch.Generator().manual_seed(seed)
    return {'normals': torch.randn(8, nb, 4, *L, generator=g, dtype=torch.float64).numpy(),
            'u': torch.rand(nb, generator=g).numpy()}


def same(a, b):
    (xa, ma), (xb, mb) = a, b
    assert torch.equal(xa, xb)
    for k in ('acc', 'sumlogdet', 'acc_mask'):
        assert torch.equal(ma[k], mb[k]), k


@pytest.fixture
def counted(monkeypatch):
    """lift the size rule of the sliced layer (a 4^4 lattice takes it) and count the digit launches"""
    from l2hmc import _ops as ops
    monkeypatch.setattr(ops, 'gemm_sliced_pays', ops.gemm_sliced_ok)
    calls = {'gemm_digits': 0, 'su3_expm_mul2_digits_n': 0, 'su3_projsu_digits_n': 0}
    for name in calls:
        def wrap(*a, _f=getattr(ops, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, wrap)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield ops, calls
    ops.USE_DIGIT_INPUTS[0] = True
    torch.set_default_dtype(old)


@pytest.mark.parametrize('verbose', [False, True], ids=['plain', 'verbose'])
def test_trajectory_on_digit_inputs_has_the_same_bits(counted, verbose):
    ops, calls = counted
    L, nb = (4, 4, 4, 4), 64
    dyn, x = build(L, nb, verbose)
    beta = 6.0
    out = {}
    for digits in (False, True, False):
        ops.USE_DIGIT_INPUTS[0] = digits
        before = dict(calls)
        dyn._inject = draws(L, nb, 3)
        xo, m = dyn((x, beta))
        dyn._inject = None
        used = {k: calls[k] - before[k] for k in calls}
        if digits:
            # (the first trajectory of the module built the weight images on fp64 activations)
            assert min(used.values()) > 0, used
            same((xo, m), out[False])
        else:
            assert not any(used.values()), used
            if False in out:
                same((xo, m), out[False])
        out[digits] = (xo.clone(), {k: m[k].clone() for k in ('acc', 'sumlogdet', 'acc_mask')})
    assert bool(torch.isfinite(out[True][1]['acc']).all())
    # device draws: same seed, same trajectory
    for digits in (False, True):
        ops.USE_DIGIT_INPUTS[0] = digits
        torch.cuda.manual_seed(7)
        out[digits] = dyn((x, beta))
    same(out[True], out[False])


def test_graphed_trajectory_on_digit_inputs(counted):
    ops, calls = counted
    L, nb = (4, 4, 4, 4), 64
    dyn, x = build(L, nb, False)
    beta = 6.0
    dyn._inject = {k: torch.from_numpy(v).cuda() for k, v in draws(L, nb, 4).items()}
    eager = dyn((x, beta))                           # (builds the weight images)
    n0 = calls['gemm_digits']
    eager = dyn((x, beta))
    assert calls['gemm_digits'] > n0
    gt = dyn.make_graphed(x, beta)
    n1 = calls['gemm_digits']
    for _ in range(2):                               # replays launch nothing from Python
        same(gt(x), eager)
    assert calls['gemm_digits'] == n1
    # the switch is part of the graph's key
    ops.USE_DIGIT_INPUTS[0] = False
    same(gt(x), eager)
    assert gt.captures == 2
    dyn._inject = None


def test_unserved_lattice_declines_digit_inputs(counted):
    ops, calls = counted
    L, nb = (2, 2, 2, 6), 64                         # V = 48
    dyn, x = build(L, nb, False)
    out = {}
    for digits in (False, True, True):
        ops.USE_DIGIT_INPUTS[0] = digits
        dyn._inject = draws(L, nb, 5)
        out[digits] = dyn((x, 6.0))
        dyn._inject = None
    assert not any(calls.values()), calls
    same(out[True], out[False])
