"""The sampler with the Hamiltonian's terms taken from the kernels that hold them (ops.USE_KERNEL_ENERGIES:
l2q_su3_force_action, the sliced heads kernel's sum |v_out|^2, l2q_su3_assemble_tah_norm2) against the same sampler
on the separate plaquette / kinetic passes: the same trajectory and accept decisions, energies to rounding, and the
passes are gone from the launch sequence."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def host(t):
    return t.detach().cpu().numpy()


_SAMPLERS = {}


@pytest.fixture(scope='module', autouse=True)
def _samplers():
    """one sampler per lattice for the whole module (8^4: 1.4 GB of weights), released with it"""
    yield
    _SAMPLERS.clear()
    torch.cuda.empty_cache()


def build(L, nb, verbose):
    if (L, nb) not in _SAMPLERS:
        old = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)
        try:
            _SAMPLERS[(L, nb)] = _build(L, nb)
        finally:
            torch.set_default_dtype(old)
    dyn, x = _SAMPLERS[(L, nb)]
    dyn.config.verbose = verbose
    return dyn, x


# random heads are O(1) per entry and every chain rejects; scaled by this (the weights are inputs of the test), the
# accept probabilities lie inside (0, 1) and the trajectories below accept some chains and reject others
HEAD_SCALE = {(4, 4, 4, 4): 0.35, (8, 8, 8, 8): 0.2}


def _build(L, nb):
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.network.pytorch.network import NetworkFactory
    torch.manual_seed(0)
    np.random.seed(0)
    V = int(np.prod(L))
    dc = cfgs.DynamicsConfig(nchains=nb, group='SU3', latvolume=list(L), nleapfrog=2, eps=0.02, eps_hmc=0.02,
                             verbose=False, use_split_xnets=False, use_separate_networks=False,
                             merge_directions=True)
    spec = cfgs.InputSpec(xshape=tuple(dc.xshape), xnet={'x': [32 * V], 'v': [32 * V]},
                          vnet={'x': [32 * V], 'v': [32 * V]})
    # units [256]: the heads run on the int8-sliced kernel, the one that emits sum |v_out|^2
    nc = cfgs.NetworkConfig(units=[256], activation_fn='tanh', dropout_prob=0.0, use_batch_norm=False)
    lat = LatticeSU3(nb, list(L))
    dyn = Dynamics(lat.action, dc, NetworkFactory(spec, nc, cfgs.ConvolutionConfig())).cuda().eval()
    head_scale = HEAD_SCALE[L]
    with torch.no_grad():
        for lin in (dyn.vnet.scale.layer, dyn.vnet.transl, dyn.vnet.transf.layer):
            lin.weight.mul_(head_scale)
            lin.bias.mul_(head_scale)
    x = lat.g.compat_proj(lat.random().cuda())
    return dyn, x


@pytest.fixture
def counted(monkeypatch):
    """float64 defaults, the sliced input layer's size rule lifted (a 4^4 lattice takes it), and the native entry
    points counted by name"""
    from l2hmc import _ops as ops
    from l2hmc import native
    monkeypatch.setattr(ops, 'gemm_sliced_pays', ops.gemm_sliced_ok)
    calls = {}

    def call(name, *a, _f=native.call):
        calls[name] = calls.get(name, 0) + 1
        return _f(name, *a)
    monkeypatch.setattr(native, 'call', call)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield ops, calls
    ops.USE_KERNEL_ENERGIES[0] = True
    torch.set_default_dtype(old)


def run(dyn, x, mode, seed, calls):
    torch.cuda.manual_seed(seed)
    before = dict(calls)
    if mode == 'hmc':
        xo, m = dyn.apply_transition_hmc((x, 6.0))
    else:
        xo, m = dyn((x, 6.0))
    used = {k: calls[k] - before.get(k, 0) for k in calls if calls[k] != before.get(k, 0)}
    return xo.clone(), {k: v.clone() for k, v in m.items() if isinstance(v, torch.Tensor)}, used


def close(a, b, what):
    """energies and acc: the tolerance tests/test_sizes_gpu.py applies between two kernels for the same trajectory"""
    a, b = host(a), host(b)
    assert a.shape == b.shape, what
    d = float(np.abs(a - b).max())
    print(f'{what}: max difference {d:.3e} at scale {max(1.0, float(np.abs(b).max())):.3e}')
    assert d <= 1e-7 * max(1.0, float(np.abs(b).max())), (what, d)


CASES = [((4, 4, 4, 4), 16), ((8, 8, 8, 8), 4)]


@pytest.mark.parametrize('mode', ['l2hmc', 'l2hmc-verbose', 'hmc'])
@pytest.mark.parametrize('L,nb', CASES, ids=['4x4', '8x4'])
def test_trajectory_with_kernel_energies(counted, L, nb, mode):
    ops, calls = counted
    dyn, x = build(L, nb, mode == 'l2hmc-verbose')
    out = {}
    for on in (False, True, False):
        ops.USE_KERNEL_ENERGIES[0] = on
        xo, m, used = run(dyn, x, mode, 5, calls)
        if on:
            # the separate passes are gone: one plaquette reduction (the opening potential) per trajectory,
            # plain HMC keeps its closing Hamiltonian (its kick emits nothing)
            want = {'l2hmc': (1, 0), 'l2hmc-verbose': (1, 0), 'hmc': (2, 1)}[mode]
            assert used.get('l2q_su3_plaq_reduce', 0) == want[0], used
            assert used.get('l2q_su3_kinetic_reduce', 0) == want[1], used
            assert used.get('l2q_su3_assemble_tah_norm2', 0) == 1 and 'l2q_su3_assemble_tah' not in used, used
            if mode != 'hmc':
                # the first force of a trajectory has no consumer for its potential; without per-step metrics
                # only the closing one has
                nforce = 2 * dyn.config.nleapfrog + 1
                na = nforce - 1 if mode == 'l2hmc-verbose' else 1
                assert used.get('l2q_su3_force_action', 0) == na, used
                assert used.get('l2q_su3_force', 0) == nforce - na >= 1, used
        else:
            assert 'l2q_su3_force_action' not in used and 'l2q_su3_assemble_tah_norm2' not in used, used
        if False in out:
            x0, m0 = out[False]
            assert torch.equal(m['acc_mask'], m0['acc_mask'])
            assert torch.equal(xo, x0)
            for k in m0:
                if k == 'acc_mask':
                    continue
                if on:
                    close(m[k], m0[k], f'{mode} {L} {k}')
                else:
                    assert torch.equal(m[k], m0[k]), k            # (the switch leaves nothing behind)
        out[on] = (xo, m)
    acc = host(out[True][1]['acc_mask'])
    assert bool(torch.isfinite(out[True][1]['acc']).all())
    if mode != 'hmc':
        assert 0 < acc.sum() < acc.size, acc                      # some chains accept, some reject


@pytest.mark.parametrize('verbose', [False, True], ids=['plain', 'verbose'])
def test_graphed_trajectory_with_kernel_energies(counted, verbose):
    """a captured trajectory replays the new launches: the same results as eager launches on the same draws"""
    ops, calls = counted
    L, nb = (4, 4, 4, 4), 16
    dyn, x = build(L, nb, verbose)
    g = torch.Generator().manual_seed(9)
    dyn._inject = {'u': torch.rand(nb, generator=g, dtype=torch.float64).cuda()}
    try:
        dyn((x, 6.0))                                    # (builds the weight images)
        gt = dyn.make_graphed(x, 6.0)
        n0 = calls.get('l2q_su3_force_action', 0)
        assert n0 > 0
        for seed in (3, 4):
            torch.cuda.manual_seed(seed)
            xg, mg = gt(x)
            xg, mg = xg.clone(), {k: v.clone() for k, v in mg.items() if isinstance(v, torch.Tensor)}
            torch.cuda.manual_seed(seed)
            xe, me = dyn((x, 6.0))
            assert torch.equal(xg, xe)
            for k in ('acc', 'sumlogdet', 'acc_mask'):
                assert torch.equal(mg[k], me[k]), k
        # the switch is part of the graph's key
        ops.USE_KERNEL_ENERGIES[0] = False
        gt(x)
        assert gt.captures == 2
    finally:
        dyn._inject = None
