"""GPU parity of the product ``l2hmc.Dynamics`` (HIP kernels through the C ABI) against the
golden vectors produced by the reference's PyTorch-CPU path on identical (lattice, beta, draws):
bit-exact accept/reject masks; plaquette / charge / dH within the stated tolerances."""
import numpy as np
import pytest
import torch

import helpers
from helpers import build_su3_dynamics, build_u1_dynamics, su3_oracle

pytestmark = pytest.mark.gpu


def host(t):
    return t.detach().cpu().numpy()


def err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(autouse=True)
def _f64_default():
    old = torch.get_default_dtype()
    yield
    torch.set_default_dtype(old)


def test_su3_lattice_api(golden):
    torch.set_default_dtype(torch.float64)
    g = golden('su3_ops')
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.group.su3.pytorch import utils as U
    L = [int(i) for i in g['latvolume']]
    lat = LatticeSU3(2, L)
    x, beta = dev(g['x']), torch.tensor(float(g['beta']))
    assert err(host(lat.action(x, beta)), g['action']) < 1e-10
    assert err(host(lat._plaquettes(x)), g['plaqs']) < 1e-14
    assert err(host(lat.sin_charges(x)), g['sinQ']) < 1e-14
    assert err(host(lat.int_charges(x)), g['intQ']) < 1e-13
    assert err(host(lat.grad_action(x, beta)), g['force']) < 1e-13
    assert err(host(lat.kinetic_energy(dev(g['v']))), g['kinetic']) < 1e-10
    m = lat.calc_metrics(x)
    assert err(host(m['plaqs']), g['plaqs']) < 1e-14
    gen = dev(g['general'])
    assert err(host(U.projectSU(gen)), g['projsu_general']) < 1e-12
    assert err(host(U.projectTAH(gen)), g['tah_general']) < 1e-15
    assert err(host(lat.g.exp(gen)), g['expm_general']) < 1e-11
    assert err(host(lat.g.group_to_vec(x)), g['vec_x']) < 1e-12
    assert err(host(lat.g.update_gauge(x, 0.3 * dev(g['v']))), g['expm_v_x']) < 1e-13
    a, b = gen, dev(g['projsu_general'])
    assert err(host(lat.g.mul(a, b, adjoint_b=True)), g['general'] @ np.conj(np.swapaxes(g['projsu_general'], -1, -2))) < 1e-13
    av, mx = U.checkSU(x)
    assert err(np.stack([host(av), host(mx)]), g['checksu_x']) < 1e-14
    torch.manual_seed(22)
    v = lat.random_momentum()
    assert err(host(v), g['v']) < 1e-15        # same CPU generator stream as the reference


def test_su3_hmc_trajectory(golden):
    torch.set_default_dtype(torch.float64)
    g = golden('su3_hmc')
    dyn, lat = build_su3_dynamics(g, with_nets=False)
    dyn._inject = {'normals': g['normals'], 'u': g['u']}
    xo, m = dyn.apply_transition_hmc((dev(g['x']), torch.tensor(float(g['beta']))),
                                     eps=float(g['eps']), nleapfrog=int(g['nleapfrog']))
    mc = m['mc_states']
    assert err(host(mc.init.v), g['v_init']) < 1e-15
    assert err(host(mc.proposed.x), g['x_prop']) < 1e-12
    assert err(host(mc.proposed.v), g['v_prop']) < 1e-11
    assert err(host(m['energy']), g['energy']) < 1e-8         # |H| ~ 2e3
    assert err(host(m['acc']), g['acc']) < 1e-8
    assert np.array_equal(host(m['acc_mask']), g['acc_mask'])  # bit-exact accept/reject
    assert err(host(xo), g['x_out'].reshape(xo.shape)) < 1e-12
    margin = np.abs(g['acc'] - g['u']).min()
    assert margin > 1e-3, margin


def test_su3_l2hmc_subupdates(golden):
    torch.set_default_dtype(torch.float64)
    from l2hmc.dynamics.pytorch.dynamics import State
    g = golden('su3_l2hmc')
    dyn, lat = build_su3_dynamics(g)
    beta = torch.tensor(float(g['beta']))
    x, v = dev(g['x']), dev(g['v0'])
    f = dyn.grad_potential(x, beta)
    assert err(host(f), g['force0']) < 1e-12
    s, t, q = dyn._call_vnet(0, (x, f))
    # vnet input = su3_to_vec(projectSU(force)): ill-conditioned in the reference itself
    # (numpy vs torch on identical input differ by 3e-9, tests/test_oracle_golden.py)
    tol = 1e-6
    assert max(err(host(s), g['s']), err(host(t), g['t']), err(host(q), g['q'])) < tol
    st, ld = dyn._update_v_fwd(0, State(x, v, beta))
    assert err(host(st.v), g['v_fwd']) < 1e-7 and err(host(ld), g['logdet_v_fwd']) < 1e-7
    st, ld = dyn._update_v_bwd(1, State(x, v, beta))
    assert err(host(st.v), g['v_bwd']) < 1e-7 and err(host(ld), g['logdet_v_bwd']) < 1e-7
    m0, mb0 = dyn._get_mask(0)
    st, ld = dyn._update_x_fwd(0, State(x, dev(g['v_fwd']), beta), m0, first=True)
    assert err(host(st.x), g['x_fwd']) < 1e-13 and float(ld.abs().max()) == 0.0
    st, _ = dyn._update_x_bwd(1, State(x, dev(g['v_fwd']), beta), mb0, first=False)
    assert err(host(st.x), g['x_bwd']) < 1e-13
    st, ld = dyn._forward_lf(0, State(x, v, beta))
    assert err(host(st.x), g['lf_fwd_x']) < 1e-8 and err(host(st.v), g['lf_fwd_v']) < 1e-7
    assert err(host(ld), g['lf_fwd_logdet']) < 1e-7


def test_su3_native_output_cache(golden):
    """A sampler loop feeds the returned x straight back: the second transition then starts from
    the native original it still holds (no reference -> native transpose).  Same result as from a
    copy of x (cache miss) and with the cache off; an in-place edit of x invalidates the entry."""
    torch.set_default_dtype(torch.float64)
    g = golden('su3_l2hmc')
    dyn, lat = build_su3_dynamics(g)
    dyn.config.verbose = False
    beta = torch.tensor(float(g['beta']))

    def two_steps(mode):
        dyn._xcache = None
        dyn.cache_native_output = mode != 'off'
        dyn._inject = {'normals': g['normals'], 'u': g['u']}
        x1, _ = dyn((dev(g['x']), beta))
        if mode == 'copy':
            x1 = x1.clone()
        elif mode == 'edit':
            x1.mul_(1.0)                                  # bumps the version counter
        hit = dyn._xcache is not None and dyn._xcache[0] is x1 and dyn._xcache[1] == x1._version
        dyn._inject = {'normals': g['normals'], 'u': g['u']}
        x2, m2 = dyn((x1, beta))
        return host(x2), host(m2['acc']), hit

    ref = two_steps('hit')
    assert ref[2]
    for mode in ('copy', 'edit', 'off'):
        out = two_steps(mode)
        assert mode == 'off' or not out[2]
        assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1]), mode
    dyn.cache_native_output = True
    # the lazily selected output momentum equals the eager selection
    dyn._inject = {'normals': g['normals'], 'u': g['u']}
    xo, m = dyn((dev(g['x']), beta))
    mc = m['mc_states']
    ma = host(m['acc_mask'])[:, None]
    want = ma * host(mc.proposed.v).reshape(ma.shape[0], -1) + (1 - ma) * host(mc.init.v).reshape(ma.shape[0], -1)
    assert err(host(mc.out.v).reshape(ma.shape[0], -1), want) == 0.0


def test_su3_l2hmc_trajectory(golden):
    torch.set_default_dtype(torch.float64)
    g = golden('su3_l2hmc')
    dyn, lat = build_su3_dynamics(g)
    dyn._inject = {'normals': g['normals'], 'u': g['u']}
    xo, m = dyn((dev(g['x']), torch.tensor(float(g['beta']))))
    mc = m['mc_states']
    assert err(host(mc.init.v), g['v_init']) < 1e-15
    assert err(host(mc.proposed.x), g['x_prop']) < 1e-7
    assert err(host(mc.proposed.v), g['v_prop']) < 1e-6
    assert err(host(m['energy']), g['energy']) < 1e-5          # dH tolerance, |H| ~ 2.4e3
    assert err(host(m['logdet']), g['logdet']) < 1e-6
    assert err(host(m['acc']), g['acc']) < 1e-5
    assert np.array_equal(host(m['acc_mask']), g['acc_mask'])  # bit-exact accept/reject
    assert err(host(m['sumlogdet']), g['sumlogdet']) < 1e-6
    assert err(host(xo), g['x_out'].reshape(xo.shape)) < 1e-7
    # observables of the output configuration vs the reference's
    from oracle import su3 as osu3
    xo_ref = g['x_out'].reshape(g['x'].shape)
    met = lat.calc_metrics(xo.reshape(g['x'].shape))
    assert err(host(met['plaqs']), osu3.plaqs(xo_ref)) < 1e-9
    assert err(host(met['intQ']), osu3.int_charges(xo_ref)) < 1e-9
    # verbose=False takes the lean path and must give the same proposal
    dyn.config.verbose = False
    xo2, m2 = dyn((dev(g['x']), torch.tensor(float(g['beta']))))
    # (the lean path pairs adjacent v-updates in one kernel: same arithmetic, equal to rounding)
    assert err(host(xo2), host(xo)) < 1e-13 and err(host(m2['acc']), host(m['acc'])) < 1e-10
    assert err(host(m2['sumlogdet']), g['sumlogdet']) < 1e-6
    # the x-update that also emits vec8(x') (fuse_x_vec8) changes nothing
    dyn.fuse_x_vec8 = False
    xo3, m3 = dyn((dev(g['x']), torch.tensor(float(g['beta']))))
    dyn.fuse_x_vec8 = True
    assert err(host(xo3), host(xo2)) < 1e-13 and err(host(m3['acc']), host(m2['acc'])) < 1e-10
    assert m2['acc'].dtype == torch.float64 and m2['acc_mask'].dtype == torch.float32
    dyn.pair_v_updates = False
    xo2b, m2b = dyn((dev(g['x']), torch.tensor(float(g['beta']))))
    assert err(host(xo2b), host(xo)) == 0.0 and err(host(m2b['acc']), host(m['acc'])) == 0.0
    # the structural optimisations (same arithmetic, fewer passes) can be switched off:
    # reuse of the v-update inputs is bitwise neutral, the fused double x-update agrees to
    # rounding (the compiler contracts the fused kernel's FMAs differently)
    dyn.reuse_v_inputs = False
    xo4, m4 = dyn((dev(g['x']), torch.tensor(float(g['beta']))))
    assert err(host(xo4), host(xo)) == 0.0 and err(host(m4['acc']), host(m['acc'])) == 0.0
    assert err(host(m4['sumlogdet']), host(m2b['sumlogdet'])) == 0.0
    dyn.fuse_x_updates = False
    xo5, m5 = dyn((dev(g['x']), torch.tensor(float(g['beta']))))
    print('fused-x-update vs two kernels:', err(host(xo5), host(xo)))
    assert err(host(xo5), host(xo)) < 1e-13 and err(host(m5['acc']), host(m['acc'])) < 1e-10
    # un-fused heads / v-update path gives the same trajectory
    dyn.fuse_heads = False
    xo3, m3 = dyn((dev(g['x']), torch.tensor(float(g['beta']))))
    assert err(host(xo3), host(xo)) < 1e-12 and err(host(m3['acc']), host(m['acc'])) < 1e-9


@pytest.mark.parametrize('name', ['u1_conv', 'u1_c1'])
def test_u1_trajectories(golden, name):
    torch.set_default_dtype(torch.float32)
    from l2hmc.dynamics.pytorch.dynamics import State
    g = golden(name)
    dyn, lat = build_u1_dynamics(g)
    beta = torch.tensor(float(g['beta']))
    x = dev(g['x'])
    nb = x.shape[0]
    assert err(host(lat.action(x, beta)), g['action']) < 2e-4
    assert err(host(lat.grad_action(x, beta)), g['force']) < 1e-5
    assert err(host(lat.plaqs(x)), g['plaqs']) < 1e-6
    assert err(host(lat.int_charges(x)), g['intQ']) < 1e-5
    v = dev(g['normals'].reshape(nb, -1))
    f = dyn.grad_potential(x, beta)
    s, t, q = dyn._call_vnet(0, (x, f))
    assert max(err(host(s), g['vnet_s']), err(host(t), g['vnet_t']), err(host(q), g['vnet_q'])) < 2e-5
    st, ld = dyn._update_v_fwd(0, State(x, v, beta))
    assert err(host(st.v), g['v_fwd']) < 2e-5 and err(host(ld), g['logdet_v_fwd']) < 1e-4
    m0, mb0 = dyn._get_mask(0)
    xm = dyn.unflatten(m0.cuda()) * x
    s, t, q = dyn._call_xnet(0, (xm, v), first=True)
    assert max(err(host(s), g['xnet_s']), err(host(t), g['xnet_t']), err(host(q), g['xnet_q'])) < 2e-5
    st, ld = dyn._update_x_fwd(0, State(x, v, beta), m0, first=True)
    d = np.abs(np.angle(np.exp(1j * (host(st.x) - g['x_fwd']))))
    assert d.max() < 3e-5 and err(host(ld), g['logdet_x_fwd']) < 1e-4
    st, ld = dyn._update_x_bwd(0, State(x, v, beta), mb0, first=False)
    d = np.abs(np.angle(np.exp(1j * (host(st.x) - g['x_bwd']))))
    assert d.max() < 3e-5 and err(host(ld), g['logdet_x_bwd']) < 1e-4
    # plain HMC
    dyn._inject = {'normals': g['hmc_normals'], 'u': g['hmc_u']}
    xo, m = dyn.apply_transition_hmc((x, beta), eps=float(g['hmc_eps']),
                                     nleapfrog=int(g['hmc_nleapfrog']))
    assert err(host(m['energy']), g['hmc_energy']) < 5e-3
    assert err(host(m['acc']), g['hmc_acc']) < 5e-3
    assert np.array_equal(host(m['acc_mask']), g['hmc_acc_mask'])
    d = np.abs(np.angle(np.exp(1j * (host(xo) - g['hmc_x_out'].reshape(nb, -1)))))
    assert d.max() < 1e-4
    # merged L2HMC trajectory
    dyn._inject = {'normals': g['normals'], 'u': g['u']}
    xo, m = dyn((x, beta))
    assert err(host(m['energy']), g['energy']) < 2e-2
    assert err(host(m['logdet']), g['logdet']) < 2e-3
    assert err(host(m['acc']), g['acc']) < 1e-2
    assert np.array_equal(host(m['acc_mask']), g['acc_mask'])  # bit-exact accept/reject
    d = np.abs(np.angle(np.exp(1j * (host(xo) - g['x_out'].reshape(nb, -1)))))
    assert d.max() < 2e-3
    assert sorted(k for k in m if k != 'mc_states') == sorted(
        ['energy', 'logprob', 'logdet', 'sldf', 'sldb', 'sld', 'xeps', 'veps', 'acc',
         'sumlogdet', 'acc_mask', 'beta'])


def test_state_dict_layout():
    """networks listed under both `networks.*` and `xnet.*`/`vnet.*` plus xeps/veps
    (50 keys / 26 unique parameters for the smallest SU(3) model)."""
    torch.set_default_dtype(torch.float64)
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.network.pytorch.network import NetworkFactory
    L = [2, 2, 2, 2]
    dc = cfgs.DynamicsConfig(nchains=2, group='SU3', latvolume=L, nleapfrog=1,
                             use_split_xnets=False, use_separate_networks=False)
    nc = cfgs.NetworkConfig(units=[1], activation_fn='tanh', dropout_prob=0.0, use_batch_norm=False)
    spec = cfgs.InputSpec(xshape=tuple(dc.xshape), xnet={'x': [512], 'v': [512]},
                          vnet={'x': [512], 'v': [512]})
    dyn = Dynamics(LatticeSU3(2, L).action, dc, NetworkFactory(spec, nc, cfgs.ConvolutionConfig()))
    keys = list(dyn.state_dict().keys())
    assert len(keys) == 50 and len(list(dyn.parameters())) == 26
    assert 'networks.vnet.scale.coeff' in keys and 'vnet.scale.coeff' in keys and 'xeps.0' in keys
    assert dyn.xnet.input_layer.xlayer.weight.shape == (1, 2 * 36 * 16)
    m = dyn.masks[0]
    assert m.shape == (1, dyn.xdim) and m.dtype == torch.float32 and int(m.sum()) == dyn.xdim // 2


@pytest.mark.parametrize('name', ['u1_c1'])
def test_graphed_transition_u1(golden, name):
    """a transition captured into a HIP graph replays to the same result as the eager path"""
    torch.set_default_dtype(torch.float32)
    g = golden(name)
    dyn, lat = build_u1_dynamics(g, verbose=False)
    x = dev(g['x'])
    beta = float(g['beta'])
    inj = {'normals': dev(g['normals']), 'u': dev(g['u'])}
    dyn._inject = inj
    xo_e, m_e = dyn((x, beta))
    gt = dyn.make_graphed(x, beta)
    xo_g, m_g = gt(x)
    assert err(host(xo_g), host(xo_e)) == 0.0
    assert np.array_equal(host(m_g['acc_mask']), g['acc_mask'])
    assert err(host(m_g['acc']), host(m_e['acc'])) == 0.0
    # replay with another input: equals the eager result for that input
    x2 = dev(np.roll(g['x'], 1, axis=0))
    xo_e2, _ = dyn((x2, beta))
    xo_g2, _ = gt(x2)
    assert err(host(xo_g2), host(xo_e2)) == 0.0
    # HMC flavour
    dyn._inject = {'normals': dev(g['hmc_normals']), 'u': dev(g['hmc_u'])}
    gh = dyn.make_graphed(x, beta, mode='hmc', eps=float(g['hmc_eps']),
                          nleapfrog=int(g['hmc_nleapfrog']))
    xo_h, m_h = gh(x)
    assert np.array_equal(host(m_h['acc_mask']), g['hmc_acc_mask'])


def test_graphed_transition_follows_model_changes(golden):
    """a replay after the model changed must not use the weights / step sizes frozen
    at capture time, and growing the global workspace must not invalidate the graph."""
    torch.set_default_dtype(torch.float32)
    from l2hmc import native, _ops as ops
    g = golden('u1_c1')
    dyn, lat = build_u1_dynamics(g, verbose=False)
    x, beta = dev(g['x']), float(g['beta'])
    dyn._inject = {'normals': dev(g['normals']), 'u': dev(g['u'])}
    gt = dyn.make_graphed(x, beta)
    xo0 = gt(x)[0].clone()
    assert gt.captures == 1
    if native._WS.buf is None:                       # (nothing before this test needed scratch)
        native.workspace(1 << 16, x.device)
        gt = dyn.make_graphed(x, beta)
        xo0 = gt(x)[0].clone()
    ws0 = native._WS.buf
    # (1) a larger workspace request: the block the graph points at must stay alive and intact
    big = native.workspace(ws0.numel() * 4 + (1 << 20), x.device)
    assert big is not ws0 and any(b is ws0 for b in native._WS.pinned)
    junk = [torch.full((ws0.numel() // 4 + 64,), 7.0, device=x.device) for _ in range(4)]
    xo1 = gt(x)[0].clone()
    assert gt.captures == 1 and err(host(xo1), host(xo0)) == 0.0
    del junk
    # (2) parameters modified in place (what the fused Adam step does through the arena)
    with torch.no_grad():
        for p in dyn.vnet.parameters():
            p.mul_(0.5)
    ops.PARAM_GENERATION[0] += 1
    xo_e = dyn((x, beta))[0].clone()
    xo2 = gt(x)[0].clone()
    assert gt.captures == 2
    assert err(host(xo2), host(xo_e)) == 0.0 and err(host(xo2), host(xo0)) > 1e-4
    # (3) new step sizes, (4) new masks
    dyn.assign_eps(0.07)
    xo_e = dyn((x, beta))[0].clone()
    assert err(host(gt(x)[0]), host(xo_e)) == 0.0 and gt.captures == 3
    dyn.set_masks([1.0 - m.numpy().reshape(-1) for m in dyn.masks])
    xo_e = dyn((x, beta))[0].clone()
    assert err(host(gt(x)[0]), host(xo_e)) == 0.0 and gt.captures == 4
    # unchanged model: plain replays
    gt(x); gt(x)
    assert gt.captures == 4


def test_graphed_transition_su3(golden):
    torch.set_default_dtype(torch.float64)
    g = golden('su3_l2hmc')
    dyn, lat = build_su3_dynamics(g, verbose=False)
    x = dev(g['x'])
    dyn._inject = {'normals': dev(g['normals']), 'u': dev(g['u'])}
    xo_e, m_e = dyn((x, float(g['beta'])))
    gt = dyn.make_graphed(x, float(g['beta']))
    xo_g, m_g = gt(x)
    assert err(host(xo_g), host(xo_e)) == 0.0
    assert np.array_equal(host(m_g['acc_mask']), g['acc_mask'])


def test_u1_large_lattice_vs_oracle():
    """BASELINE cfg-3 lattice (64 x 64) at a small chain count: kernels vs the numpy oracle"""
    torch.set_default_dtype(torch.float32)
    from oracle import u1 as ou1
    from l2hmc.lattice.u1.pytorch.lattice import LatticeU1
    from l2hmc import _ops as ops
    rng = np.random.default_rng(4)
    L = (64, 64)
    x = ou1.compat_proj((2 * np.pi * rng.random((5, 2, *L))).astype(np.float32))
    lat = LatticeU1(5, list(L))
    xd = dev(x)
    assert err(host(lat.action(xd, torch.tensor(6.0))), ou1.action(x, 6.0)) < 5e-2     # |S| ~ 2.4e4
    assert err(host(lat.grad_action(xd, torch.tensor(6.0))), ou1.grad_action(x, 6.0)) < 2e-5
    assert err(host(lat.plaqs(xd)), ou1.plaqs(x)) < 1e-6
    assert err(host(lat.int_charges(xd)), ou1.int_charges(x)) < 1e-3
    v = rng.normal(size=(5, 2 * 64 * 64)).astype(np.float32)
    vd = dev(v)
    ops.u1_force_kick_(xd, 6.0, -0.05, vd, L)
    assert err(host(vd), v - 0.05 * ou1.grad_action(x, 6.0).reshape(5, -1)) < 2e-5


@pytest.mark.parametrize('lat,nb,units,act,bn', [((8, 8), 128, [16, 16, 16, 16], 'leaky_relu', True),
                                                 ((4, 6), 5, [8, 6], 'tanh', False),
                                                 ((16, 16), 37, [16, 16], 'relu', True),
                                                 ((32, 32), 9, [64], 'elu', False),
                                                 ((8, 8), 3, [5, 7, 3], 'swish', True)])
def test_u1_fused_substeps_equal_unfused(lat, nb, units, act, bn):
    """The one-launch U(1) sub-updates (l2q_u1_vstep_f32 / l2q_u1_xstep_f32: force or cos/sin +
    whole LeapfrogLayer + update) against the multi-kernel path (force, GEMMs, update kernels)
    on the same state: every sub-update of a leapfrog step in both directions, ragged chain
    counts, 1-3 hidden layers, all activations, folded BatchNorm."""
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.u1.pytorch.lattice import LatticeU1
    from l2hmc.network.pytorch.network import NetworkFactory
    torch.set_default_dtype(torch.float32)
    torch.manual_seed(5)
    np.random.seed(5)
    dc = cfgs.DynamicsConfig(nchains=nb, group='U1', latvolume=list(lat), nleapfrog=2, eps=0.1,
                             eps_hmc=0.1, verbose=False)
    nc = cfgs.NetworkConfig(units=units, activation_fn=act, dropout_prob=0.0, use_batch_norm=bn)
    spec = cfgs.InputSpec(xshape=tuple(dc.xshape), xnet={'x': [dc.xdim, 2], 'v': [dc.xdim]},
                          vnet={'x': [dc.xdim], 'v': [dc.xdim]})
    latt = LatticeU1(nb, list(lat))
    dyn = Dynamics(latt.action, dc, NetworkFactory(spec, nc, cfgs.ConvolutionConfig())).eval()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n_, p in dyn.named_parameters():
            if n_.endswith('coeff'):
                p.copy_(0.3 * torch.randn(p.shape, generator=g).to(p.device))
        for n_, b in dyn.named_buffers():
            if n_.endswith('running_mean'):
                b.copy_(0.1 * torch.randn(b.shape, generator=g).to(b.device))
            if n_.endswith('running_var'):
                b.copy_(1.0 + 0.2 * torch.rand(b.shape, generator=g).to(b.device))
    x0 = latt.random().to(dyn.device)
    v0 = torch.randn(nb, dc.xdim, generator=g).to(dyn.device)
    for forward in (True, False):
        res = {}
        for fused in (True, False):
            dyn.fuse_u1_steps = fused
            xn, vn = dyn._pack(x0), v0.clone()
            ld = dyn._lf_n(1, xn, vn, 2.5, forward)
            res[fused] = (xn.clone(), vn.clone(), ld.clone())
        assert dyn._fused_u1(dyn._get_vnet(0)) is None      # switch is honoured
        dyn.fuse_u1_steps = True
        assert dyn._fused_u1(dyn._get_vnet(0)) is not None
        dx = torch.remainder(res[True][0] - res[False][0] + np.pi, 2 * np.pi) - np.pi
        assert float(dx.abs().max()) < 2e-4, float(dx.abs().max())
        scale = max(1.0, float(res[False][1].abs().max()))
        assert float((res[True][1] - res[False][1]).abs().max()) < 2e-4 * scale
        lscale = max(1.0, float(res[False][2].abs().max()))
        assert float((res[True][2] - res[False][2]).abs().max()) < 5e-4 * lscale


@pytest.mark.parametrize('group', ['U1', 'SU3'])
def test_apply_transition_both_and_hmc_helpers(group, golden):
    """apply_transition_both (dynamics.py:744-803) against the oracle's two single-direction
    kernels mixed with the same direction / accept masks; get_metrics; the *_hmc sub-update
    helpers; complexify / _stack_as_xy."""
    import oracle.su3 as osu3
    import oracle.u1 as ou1
    from l2hmc.dynamics.pytorch.dynamics import Dynamics, State
    if group == 'SU3':
        torch.set_default_dtype(torch.float64)
        g = golden('su3_l2hmc')
        dyn, lat = helpers.build_su3_dynamics(g, verbose=False)
        orc = helpers.su3_oracle(g)
        tol = 1e-9
    else:
        torch.set_default_dtype(torch.float32)
        g = golden('u1_c1')
        dyn, lat = helpers.build_u1_dynamics(g, verbose=False)
        orc = helpers.u1_oracle(g)
        tol = 5e-3
    orc.merge_directions = False
    x = torch.from_numpy(g['x'])
    nb = x.shape[0]
    beta = float(g['beta'])
    gen = np.random.default_rng(3)
    shape = (8, nb, 4, *[int(i) for i in g['latvolume']]) if group == 'SU3' else \
        (nb, 2, *[int(i) for i in g['latvolume']])
    nf, nbk = gen.standard_normal(shape), gen.standard_normal(shape)
    if group == 'U1':
        nf, nbk = nf.astype(np.float32), nbk.astype(np.float32)
    dirmask = (gen.random(nb) > 0.5).astype(np.float32)
    u = gen.random(nb).astype(np.float64 if group == 'SU3' else np.float32)
    draws = iter([nf, nbk])
    real_mom = dyn._momentum_n

    def momentum(n):
        dyn._inject = {'normals': next(draws)}
        try:
            return real_mom(n)
        finally:
            dyn._inject = None
    dyn._momentum_n = momentum
    dyn._get_direction_masks = lambda batch_size: (torch.from_numpy(dirmask).to(dyn.device),
                                                   torch.from_numpy(1 - dirmask).to(dyn.device))
    dyn._uniform = lambda acc: torch.from_numpy(u).to(acc)
    xo, m = dyn.apply_transition_both((x, torch.tensor(beta)))
    # oracle: the two single-direction kernels (dynamics.py:1031-1063 incl. its swapped accept args)
    xin = ou1.compat_proj(g['x']) if False else g['x']
    res = {}
    for name, nrm, fwd in (('f', nf, True), ('b', nbk, False)):
        v0 = orc.random_momentum(nrm)
        xx, vv = xin.reshape(nb, -1) if group == 'U1' else xin, v0
        sld = np.zeros(nb)
        for step in range(orc.nlf):
            xx, vv, ld = (orc.forward_lf if fwd else orc.backward_lf)(step, xx, vv, beta)
            sld = sld + ld
        h0 = orc.hamiltonian(xin.reshape(nb, -1) if group == 'U1' else xin, v0, beta)
        h1 = orc.hamiltonian(xx, vv, beta)
        res[name] = (xx.reshape(nb, -1), orc.accept_prob(h1, h0, sld), sld)
    mf = dirmask
    acc = mf * res['f'][1] + (1 - mf) * res['b'][1]
    xp = mf[:, None] * res['f'][0] + (1 - mf)[:, None] * res['b'][0]
    ma = (acc > u).astype(np.float32)
    xo_ref = ma[:, None] * xp + (1 - ma)[:, None] * g['x'].reshape(nb, -1)
    np.testing.assert_allclose(m['acc'].cpu().numpy(), acc, rtol=tol, atol=tol)
    assert np.array_equal(m['acc_mask'].cpu().numpy(), ma)
    got = xo.cpu().numpy()
    if group == 'U1':
        d = np.abs(np.angle(np.exp(1j * (got - xo_ref)))).max()
    else:
        d = np.abs(got - xo_ref).max()
    assert d < 10 * tol, d
    # get_metrics on a reference-layout state == hamiltonian pieces
    st = State(x=x.to(dyn.device), v=dyn.g.random_momentum(list(x.shape)).to(dyn.device)
               if group == 'SU3' else torch.randn(nb, dyn.xdim).to(dyn.device), beta=torch.tensor(beta))
    ld = torch.zeros(nb, dtype=torch.get_default_dtype(), device=dyn.device)
    mt = dyn.get_metrics(st, ld, step=0)
    assert torch.allclose(mt['energy'], dyn.hamiltonian(st), rtol=1e-5)
    # trainable-step HMC helpers: v -/+ eps/2 F and update_gauge(x, +-eps v)
    ev, ex = dyn._eps('v', 0), dyn._eps('x', 0)
    F = dyn.grad_potential(st.x, st.beta).reshape(st.v.shape)
    assert torch.allclose(dyn._update_v_fwd_hmc(0, st), st.v - 0.5 * ev * F, atol=1e-5)
    assert torch.allclose(dyn._update_v_bwd_hmc(0, st), st.v + 0.5 * ev * F, atol=1e-5)
    xf = dyn._update_x_fwd_hmc(0, st)
    xb = dyn._update_x_bwd_hmc(0, State(xf, st.v, st.beta))
    dxx = (xb.reshape(st.x.shape) - st.x)
    if group == 'U1':
        dxx = torch.remainder(dxx + np.pi, 2 * np.pi) - np.pi
    assert float(dxx.abs().max()) < 1e-5                      # x -> x' -> x
    # complexify / _stack_as_xy
    r = torch.randn(3, 2, 4, 5)
    assert torch.equal(Dynamics.complexify(r, 1), torch.complex(r[:, 0], r[:, 1]))
    r2 = torch.randn(3, 4, 5, 2)
    # dim != 1: the reference's two transposes leave the middle axes swapped (dynamics.py:1525-1531)
    assert torch.equal(Dynamics.complexify(r2, 3),
                       torch.complex(r2[..., 0], r2[..., 1]).transpose(1, 2))
    if group == 'U1':
        xy = dyn._stack_as_xy(x)
        assert torch.allclose(xy[..., 0].cpu(), x.cos(), atol=1e-6)
        assert torch.allclose(xy[..., 1].cpu(), x.sin(), atol=1e-6)


@pytest.mark.parametrize('hd', ['fp16', 'bf16'])
@pytest.mark.parametrize('lat,nb,units,act,bn', [((8, 8), 128, [32, 32], 'leaky_relu', True),
                                                 ((16, 16), 37, [64], 'tanh', False),
                                                 ((64, 64), 24, [128, 96], 'relu', False)])
def test_u1_half_precision_networks(hd, lat, nb, units, act, bn):
    """BASELINE cfg-3 "fp16 nets / fp32 action": Dynamics.set_net_precision.  (i) the network
    outputs of the 16-bit path equal the emulator's autocast restatement; (ii) one leapfrog step
    stays within half-precision distance of the fp32 step; (iii) the merged trajectory runs,
    is deterministic, and its accept probabilities track the fp32 ones."""
    import emu_native
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.u1.pytorch.lattice import LatticeU1
    from l2hmc.network.pytorch.network import NetworkFactory
    from l2hmc import native
    torch.set_default_dtype(torch.float32)
    torch.manual_seed(5)
    np.random.seed(5)
    dc = cfgs.DynamicsConfig(nchains=nb, group='U1', latvolume=list(lat), nleapfrog=2, eps=0.1,
                             eps_hmc=0.1, verbose=False)
    nc = cfgs.NetworkConfig(units=units, activation_fn=act, dropout_prob=0.0, use_batch_norm=bn)
    spec = cfgs.InputSpec(xshape=tuple(dc.xshape), xnet={'x': [dc.xdim, 2], 'v': [dc.xdim]},
                          vnet={'x': [dc.xdim], 'v': [dc.xdim]})
    latt = LatticeU1(nb, list(lat))
    dyn = Dynamics(latt.action, dc, NetworkFactory(spec, nc, cfgs.ConvolutionConfig())).eval()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n_, p in dyn.named_parameters():
            if n_.endswith('coeff'):
                p.copy_(0.3 * torch.randn(p.shape, generator=g).to(p.device))
    x0 = latt.random().to(dyn.device)
    v0 = torch.randn(nb, dc.xdim, generator=g).to(dyn.device)
    ulp = 2.0 ** -10 if hd == 'fp16' else 2.0 ** -7
    # (i) network outputs vs the emulator (CPU restatement of the rounding points)
    dyn.set_net_precision(hd)
    assert dyn._fused_u1(dyn._get_vnet(0)) is None
    vnet = dyn._get_vnet(0)
    f0 = dyn.grad_potential(x0, torch.tensor(2.5))
    got = vnet.forward_flat(x0.reshape(nb, -1).contiguous(), f0.reshape(nb, -1).contiguous())
    w = vnet.kernel_weights()
    cpu_w = {'h': {'wx': w['h']['wx'].cpu(), 'wv': w['h']['wv'].cpu(), 'bx': w['h']['bx'].cpu(),
                   'bv': w['h']['bv'].cpu(),
                   'hidden': [(a.cpu(), b.cpu()) for a, b in w['h']['hidden']],
                   'heads': {k: tuple(None if t is None else t.cpu() for t in v)
                             for k, v in w['h']['heads'].items()}}}
    real_call = native.call
    native.call = emu_native.call
    try:
        want = vnet.forward_flat(x0.reshape(nb, -1).cpu().contiguous(),
                                 f0.reshape(nb, -1).cpu().contiguous(), cpu_w)
    finally:
        native.call = real_call
    for a, b in zip(got, want):
        d = (a.cpu() - b).abs()
        assert float(d.max()) < 8 * ulp * max(1.0, float(b.abs().max())), float(d.max())
    # (ii) one leapfrog step, both directions, vs fp32
    for forward in (True, False):
        res = {}
        for prec in (None, hd):
            dyn.set_net_precision(prec)
            dyn.fuse_u1_steps = False
            xn, vn = dyn._pack(x0), v0.clone()
            ld = dyn._lf_n(1, xn, vn, 2.5, forward)
            res[prec] = (xn.clone(), vn.clone(), ld.clone())
        dx = torch.remainder(res[hd][0] - res[None][0] + np.pi, 2 * np.pi) - np.pi
        assert float(dx.abs().max()) < 40 * ulp, float(dx.abs().max())
        scale = max(1.0, float(res[None][1].abs().max()))
        assert float((res[hd][1] - res[None][1]).abs().max()) < 40 * ulp * scale
        assert float((res[hd][2] - res[None][2]).abs().max()) < 2 * ulp * dc.xdim ** 0.5 * 8
        # heads + update in one kernel == 16-bit head GEMMs followed by the fp32 update kernels
        dyn.set_net_precision(hd)
        dyn.fuse_half_heads = False
        xn, vn = dyn._pack(x0), v0.clone()
        ld = dyn._lf_n(1, xn, vn, 2.5, forward)
        dyn.fuse_half_heads = True
        dx = torch.remainder(res[hd][0] - xn + np.pi, 2 * np.pi) - np.pi
        # (the fused epilogue uses the hardware exp / log / sin / cos: ~1e-6 per operation; and the
        # two paths accumulate the 16-bit layers in different orders, so a pre-activation that
        # sits on a 16-bit rounding boundary may round to the other neighbour -- one ulp_16 of one
        # s / t / q entry, a whole chain's worth when it happens in a hidden activation.  The
        # pin to the reference's own 16-bit results is test_u1_{fp16,bf16}_reference_golden.)
        tol = max(1e-3, 0.5 * ulp)
        assert float(dx.abs().max()) < tol, float(dx.abs().max())
        assert float((res[hd][1] - vn).abs().max()) < tol * scale
        assert float((res[hd][2] - ld).abs().max()) < tol * max(1.0, float(ld.abs().max()))
    # (iii) whole merged trajectory
    dyn.fuse_u1_steps = True
    beta = torch.tensor(2.5)
    out = {}
    for prec in (None, hd, hd):
        dyn.set_net_precision(prec)
        nrm = torch.randn(nb, dc.xdim, generator=torch.Generator().manual_seed(3))
        dyn._inject = {'normals': nrm.numpy(), 'u': np.full(nb, 0.5, dtype=np.float32)}
        xo, m = dyn((x0, beta))
        out.setdefault(prec, []).append((xo.clone(), m['acc'].clone()))
    assert torch.equal(out[hd][0][0], out[hd][1][0]) and torch.equal(out[hd][0][1], out[hd][1][1])
    da = (out[hd][0][1] - out[None][0][1]).abs()
    assert float(da.max()) < 400 * ulp, float(da.max())
    assert bool(torch.isfinite(out[hd][0][0]).all())


def _half_golden_check(g, dyn, fused: bool, has_conv: bool, hd: str = 'bf16'):
    """Compare Dynamics.set_net_precision('bf16' | 'fp16') with the REAL reference run under
    torch.autocast('cpu', dtype=torch.bfloat16 | torch.float16) (tests/golden/make_golden_bf16.py).
    Tolerances in ulps of the 16-bit type (2^-7 resp. 2^-10 relative to the largest magnitude): the 16-bit layers round after every Linear
    and activation like autocast does; the one structural difference is that the input layer's two
    Linears share one fp32 accumulator here (one rounding) while autocast rounds each and their
    sum (three roundings), so outputs agree to ~1-2 ulp with about half of the entries bit-equal."""
    from l2hmc.dynamics.pytorch.dynamics import State
    ulp = 2.0 ** -7 if hd == 'bf16' else 2.0 ** -10
    dyn.set_net_precision(hd)
    dyn.fuse_half_heads = fused
    x = torch.from_numpy(g['x']).to(dyn.device)
    beta = torch.tensor(float(g['beta']))
    nb = x.shape[0]
    v = torch.from_numpy(g['normals']).reshape(nb, -1).to(dyn.device)
    f = dyn.grad_potential(x, beta)
    assert err(host(f), g['force']) < 1e-5
    exact = []

    def close_ulps(got, ref, n_ulp):
        got, ref = host(got).reshape(ref.shape), ref
        scale = max(1.0, float(np.abs(ref).max()))
        e = float(np.abs(got - ref).max())
        assert e <= n_ulp * ulp * scale, (e, n_ulp * ulp * scale)
        exact.append(float((got == ref).mean()))
    for a, k in zip(dyn._call_vnet(0, (x, f)), ('vnet_s', 'vnet_t', 'vnet_q')):
        close_ulps(a, g[k], 2.5 if not has_conv else 4)
    m0, mb0 = dyn._get_mask(0)
    xm = dyn.unflatten(m0.to(dyn.device)) * x
    for a, k in zip(dyn._call_xnet(0, (xm, v), first=True), ('xnet_s', 'xnet_t', 'xnet_q')):
        close_ulps(a, g[k], 2.5 if not has_conv else 4)
    assert min(exact) > (0.3 if not has_conv else 0.15), exact      # rounding points line up
    # sub-updates (fp32 lattice arithmetic on 16-bit network outputs): 1e-3 = eps/2 * 2 ulp
    st, ld = dyn._update_v_fwd(0, State(x, v, beta))
    assert err(host(st.v).reshape(nb, -1), g['v_fwd'].reshape(nb, -1)) < 2e-3
    assert err(host(ld), g['logdet_v_fwd']) < 8e-3
    for key, fn, mk, first in (('x_fwd', dyn._update_x_fwd, m0, True), ('x_bwd', dyn._update_x_bwd, mb0, False)):
        st, ld = fn(0, State(x, v, beta), mk, first=first)
        dx = np.abs(np.angle(np.exp(1j * (host(st.x) - g[key]))))
        assert dx.max() < 2e-3, (key, dx.max())
        assert err(host(ld), g['logdet_' + key]) < 8e-3
    # merged trajectory: the reference's own bf16-vs-fp32 distance is the yardstick
    dyn._inject = {'normals': g['normals'], 'u': g['u']}
    xo, m = dyn((x, beta))
    dyn._inject = None
    yard = float(np.abs(g['acc'] - g['acc_fp32']).max())
    assert err(host(m['acc']), g['acc']) < max(3 * yard, 5e-3)
    assert np.array_equal(host(m['acc_mask']), g['acc_mask'])          # bit-exact accept / reject
    margin = float(np.abs(g['acc'] - g['u']).min())
    assert margin > 0.05, margin
    dx = np.abs(np.angle(np.exp(1j * (host(xo) - g['x_out'].reshape(nb, -1)))))
    assert dx.max() < 5e-3, dx.max()
    assert err(host(m['energy']), g['energy']) < 0.1                   # |H| ~ 1e2, dH within bf16 noise


@pytest.mark.parametrize('name', ['u1_bf16', 'u1_bf16_tanh', 'u1_bf16_conv'])
@pytest.mark.parametrize('fused', [True, False])
def test_u1_bf16_reference_golden(golden, name, fused):
    """BASELINE cfg-3 ("16-bit nets / fp32 action") pinned to the reference itself."""
    torch.set_default_dtype(torch.float32)
    g = golden(name)
    dyn, lat = build_u1_dynamics(g)
    _half_golden_check(g, dyn, fused, has_conv=bool(g['conv_filters'].size), hd='bf16')


@pytest.mark.parametrize('name', ['u1_fp16', 'u1_fp16_tanh', 'u1_fp16_conv'])
@pytest.mark.parametrize('fused', [True, False])
def test_u1_fp16_reference_golden(golden, name, fused):
    """BASELINE cfg-3's stated dtype -- fp16 nets / fp32 action -- pinned to the reference itself
    (the same generator with torch.float16)."""
    torch.set_default_dtype(torch.float32)
    g = golden(name)
    dyn, lat = build_u1_dynamics(g)
    _half_golden_check(g, dyn, fused, has_conv=bool(g['conv_filters'].size), hd='fp16')


def test_su3_improved_action_c1(golden):
    """c1 != 0 (lattice/su3/pytorch/lattice.py:83-112, 180-196, 252-308): rectangle sum, action,
    force of LatticeSU3(c1) against the reference's goldens; Dynamics with the improved action as
    potential_fn reproduces the reference's plain-HMC transition (rectangles enter H only, the
    leapfrog force stays the Wilson force -- the reference's own split, dynamics.py:134-135)."""
    torch.set_default_dtype(torch.float64)
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from oracle import su3 as osu3
    g = golden('su3_c1')
    L = [int(i) for i in g['latvolume']]
    x = dev(g['x'])
    nb = x.shape[0]
    beta, c1 = torch.tensor(float(g['beta'])), float(g['c1'])
    lat = LatticeSU3(nb, L, c1=c1)
    xn = lat.pack(x)
    assert err(host(lat.rect_sums_n(xn)), g['rect_sum']) < 1e-11
    assert err(host(lat.action(x, beta)), g['action']) < 1e-11
    assert err(host(lat.grad_action(x, beta)), g['force']) < 1e-12
    s, f = lat.action_with_grad(x, beta)
    assert err(host(s), g['action']) < 1e-11 and err(host(f), g['force']) < 1e-12
    ps, rs = lat._wilson_loops(x, needs_rect=True)              # the reference's trace fields [6, ...], [12, ...]
    assert tuple(rs.shape) == g['rects'].shape and err(host(rs), g['rects']) < 1e-13
    assert err(host(lat._re_sum(ps)), g['plaq_sum']) < 1e-11
    assert err(host(rs.real.sum(tuple(range(2, rs.dim()))).sum(0)), g['rect_sum']) < 1e-11
    assert err(host(lat._action((ps, rs), beta)), -g['action']) < 1e-11
    assert err(host(lat._action((lat.plaq_sums(x), lat.rect_sums_n(xn)), beta)), -g['action']) < 1e-11
    urul, uuud = lat._rectangles(x, 2, 1)
    assert err(host(urul), g['rect_21_urul']) < 1e-13 and err(host(uuud), g['rect_21_uuud']) < 1e-13
    _, rects = lat._plaquette_field(x, needs_rect=True)
    tr = torch.diagonal(rects, dim1=-2, dim2=-1).sum(-1)
    assert err(host(tr), g['rects']) < 1e-13
    # larger, ragged lattice against the oracle (kernel blocks not full, wrap in every direction)
    L2 = [3, 5, 2, 6]
    lat2 = LatticeSU3(3, L2, c1=-1.4088)
    x2 = lat2.random()
    assert err(host(lat2.action(x2, beta)), osu3.action_c1(host(x2), float(beta), -1.4088)) < 1e-10
    assert err(host(lat2.grad_action(x2, beta)),
               osu3.grad_action_c1(host(x2), float(beta), -1.4088)) < 1e-11
    # Dynamics: improved action in H, Wilson force in the integrator
    dc = cfgs.DynamicsConfig(nchains=nb, group='SU3', latvolume=L, nleapfrog=2, eps=0.02,
                             eps_hmc=0.05, use_split_xnets=False, use_separate_networks=False,
                             verbose=True)
    dyn = Dynamics(lat.action, dc, None).eval()
    assert dyn.potential_c1 == c1
    dyn._inject = {'normals': g['hmc_normals'], 'u': g['hmc_u']}
    xo, m = dyn.apply_transition_hmc((x, beta), eps=0.05, nleapfrog=3)
    assert err(host(m['energy']), g['hmc_energy']) < 1e-9
    assert err(host(m['acc']), g['hmc_acc']) < 1e-9
    assert np.array_equal(host(m['acc_mask']), g['hmc_acc_mask'])
    assert err(host(xo), g['hmc_x_out'].reshape(xo.shape)) < 1e-12


@pytest.mark.parametrize('group', ['SU3', 'U1'])
def test_hmc_merged_half_kicks_equal_unmerged(group):
    """Plain HMC without per-step metrics evaluates the force nleapfrog + 1 times (adjacent
    half-kicks merged) instead of 2 nleapfrog: same trajectory up to one rounding of v per step."""
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.lattice.u1.pytorch.lattice import LatticeU1
    if group == 'SU3':
        torch.set_default_dtype(torch.float64)
        L, nb, beta, eps, tol = [4, 2, 2, 4], 3, 6.0, 0.03, 1e-12
        lat = LatticeSU3(nb, L)
    else:
        torch.set_default_dtype(torch.float32)
        L, nb, beta, eps, tol = [8, 6], 5, 3.0, 0.1, 2e-5
        lat = LatticeU1(nb, L)
    dc = cfgs.DynamicsConfig(nchains=nb, group=group, latvolume=L, nleapfrog=3, eps=eps,
                             eps_hmc=eps, verbose=False, use_split_xnets=False,
                             use_separate_networks=False)
    dyn = Dynamics(lat.action, dc, None).eval()
    torch.manual_seed(2)
    x = lat.random().to(dyn.device)
    dyn._inject = None
    xn = dyn._pack(x)
    vn = dyn._momentum_n(nb)
    res = {}
    for merged in (True, False):
        dyn.merge_hmc_kicks = merged
        x_, v_, hist = dyn._kernel_hmc_n(xn, vn, beta, eps=eps, nleapfrog=5)
        res[merged] = (x_.clone(), v_.clone(), hist['acc'].clone())
    for a, b in zip(res[True], res[False]):
        d = a - b
        if group == 'U1' and a.shape == res[True][0].shape:
            d = torch.remainder(d + np.pi, 2 * np.pi) - np.pi
        assert float(d.abs().max()) < tol * max(1.0, float(b.abs().max()))
    torch.set_default_dtype(torch.float32)


@pytest.mark.parametrize('hd', ['fp16', 'bf16'])
def test_u1_half_precision_conv_stack(hd):
    """precision = fp16 | bf16 with the default-style conv stack in front of the xnet / vnet:
    the 16-bit conv path equals the fp32 conv path to half precision, a whole trajectory runs
    and is deterministic."""
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.u1.pytorch.lattice import LatticeU1
    from l2hmc.network.pytorch.network import NetworkFactory
    torch.set_default_dtype(torch.float32)
    torch.manual_seed(5)
    np.random.seed(5)
    lat, nb = (16, 16), 24
    dc = cfgs.DynamicsConfig(nchains=nb, group='U1', latvolume=list(lat), nleapfrog=2, eps=0.1,
                             eps_hmc=0.1, verbose=False)
    nc = cfgs.NetworkConfig(units=[16, 16], activation_fn='leaky_relu', dropout_prob=0.0,
                            use_batch_norm=True)
    cc = cfgs.ConvolutionConfig(filters=[8, 16, 32, 64, 128], sizes=[5, 3, 3, 3, 2],
                                pool=[2, 2, 2, 2, 2])
    spec = cfgs.InputSpec(xshape=tuple(dc.xshape), xnet={'x': [dc.xdim, 2], 'v': [dc.xdim]},
                          vnet={'x': [dc.xdim], 'v': [dc.xdim]})
    latt = LatticeU1(nb, list(lat))
    dyn = Dynamics(latt.action, dc, NetworkFactory(spec, nc, cc)).eval()
    x0 = latt.random().to(dyn.device)
    ulp = 2.0 ** -10 if hd == 'fp16' else 2.0 ** -7
    cs = dyn._get_vnet(0).input_layer.conv_stack
    want = cs(x0)
    dyn.set_net_precision(hd)
    assert cs.half_dtype is not None
    got = cs(x0)
    assert got.dtype == torch.float32 and got.shape == want.shape
    scale = max(1.0, float(want.abs().max()))
    assert float((got - want).abs().max()) < 60 * ulp * scale, float((got - want).abs().max())
    out = []
    for _ in range(2):
        nrm = torch.randn(nb, dc.xdim, generator=torch.Generator().manual_seed(3))
        dyn._inject = {'normals': nrm.numpy(), 'u': np.full(nb, 0.5, dtype=np.float32)}
        xo, m = dyn((x0, torch.tensor(2.5)))
        out.append((xo.clone(), m['acc'].clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert bool(torch.isfinite(out[0][0]).all())
    dyn.set_net_precision(None)
    dyn._inject = {'normals': nrm.numpy(), 'u': np.full(nb, 0.5, dtype=np.float32)}
    xo32, m32 = dyn((x0, torch.tensor(2.5)))
    assert float((m32['acc'] - out[0][1]).abs().max()) < 600 * ulp


@pytest.mark.parametrize('ncp', [True, False])
@pytest.mark.parametrize('sep,split', [(False, False), (True, False), (False, True), (True, True)])
def test_u1_network_sharing_modes_vs_oracle(sep, split, ncp):
    """use_separate_networks / use_split_xnets (dynamics.py:226-237, network.py:669-801): which
    LeapfrogLayer a sub-update calls -- one shared pair, one per leapfrog step, first / second
    xnets -- and the x-update form (use_ncp, dynamics.py:1386-1477) against the oracle driven by
    the same state_dict, on a merged trajectory."""
    import l2hmc.configs as cfgs
    from oracle import network as onet
    from oracle.dynamics import DynamicsOracle
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.u1.pytorch.lattice import LatticeU1
    from l2hmc.network.pytorch.network import NetworkFactory
    torch.set_default_dtype(torch.float32)
    torch.manual_seed(21)
    np.random.seed(21)
    L, nb, nlf, beta = [6, 4], 5, 3, 2.0
    dc = cfgs.DynamicsConfig(nchains=nb, group='U1', latvolume=L, nleapfrog=nlf, eps=0.07,
                             eps_hmc=0.1, verbose=False, use_split_xnets=split,
                             use_separate_networks=sep, use_ncp=ncp)
    nc = cfgs.NetworkConfig(units=[8, 6], activation_fn='tanh', dropout_prob=0.0,
                            use_batch_norm=False)
    spec = cfgs.InputSpec(xshape=tuple(dc.xshape), xnet={'x': [dc.xdim, 2], 'v': [dc.xdim]},
                          vnet={'x': [dc.xdim], 'v': [dc.xdim]})
    lat = LatticeU1(nb, L)
    dyn = Dynamics(lat.action, dc, NetworkFactory(spec, nc, cfgs.ConvolutionConfig())).eval()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n_, p in dyn.named_parameters():
            if n_.endswith('coeff'):
                p.copy_(0.3 * torch.randn(p.shape, generator=g).to(p.device))
    sd = {k: v.detach().cpu().numpy() for k, v in dyn.state_dict().items()
          if not k.startswith('networks.')}
    kw = dict(nunits=2, activation='tanh', conv=None, use_batch_norm=False)

    def vnet(step, x, f):
        pre = f'vnet.{step}.' if sep else 'vnet.'
        return onet.leapfrog_layer(x, f, helpers.sub(sd, pre), **kw)

    def xnet(step, first, x, v):
        pre = 'xnet.'
        if sep:
            pre += f'{step}.'
            if split:
                pre += 'first.' if first else 'second.'
        return onet.leapfrog_layer(x, v, helpers.sub(sd, pre), **kw)
    orc = DynamicsOracle('U1', tuple(L), nlf, [sd[f'xeps.{i}'] for i in range(nlf)],
                         [sd[f'veps.{i}'] for i in range(nlf)],
                         np.stack([host(m)[0] for m in dyn.masks]), vnet=vnet, xnet=xnet,
                         use_ncp=ncp, dtype=np.float32)
    x = lat.random()
    nrm = torch.randn(nb, 2, *L, generator=g).numpy()
    u = np.full(nb, 0.5, dtype=np.float32)
    want_x, want_m = orc.apply_transition_fb(host(x), beta, nrm, u)
    for fused in (True, False):
        dyn.fuse_u1_steps = fused
        dyn._inject = {'normals': nrm, 'u': u}
        xo, m = dyn((x, torch.tensor(beta)))
        assert err(host(m['acc']), want_m['acc']) < 2e-3, (sep, split, fused)
        d = np.abs(np.angle(np.exp(1j * (host(xo) - want_x.reshape(nb, -1)))))
        assert d.max() < 2e-4, (sep, split, fused, d.max())


def test_u1_net_weights_vs_oracle():
    """NetWeights (configs.py NetWeight s / t / q multipliers of the xnet and vnet outputs, set by
    NetworkFactory and Experiment.set_net_weights) against the oracle's `nw` scaling, on a merged
    trajectory; (0, 0, 0) weights reduce L2HMC to a reversible leapfrog with zero log-Jacobian."""
    import l2hmc.configs as cfgs
    from oracle import network as onet
    from oracle.dynamics import DynamicsOracle
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.u1.pytorch.lattice import LatticeU1
    from l2hmc.network.pytorch.network import NetworkFactory
    torch.set_default_dtype(torch.float32)
    torch.manual_seed(23)
    np.random.seed(23)
    L, nb, nlf, beta = [4, 6], 4, 2, 2.5
    nwx, nwv = (0.5, 2.0, 0.0), (1.5, 0.0, 0.7)
    dc = cfgs.DynamicsConfig(nchains=nb, group='U1', latvolume=L, nleapfrog=nlf, eps=0.08,
                             eps_hmc=0.1, verbose=False)
    nc = cfgs.NetworkConfig(units=[8], activation_fn='leaky_relu', dropout_prob=0.0,
                            use_batch_norm=False)
    spec = cfgs.InputSpec(xshape=tuple(dc.xshape), xnet={'x': [dc.xdim, 2], 'v': [dc.xdim]},
                          vnet={'x': [dc.xdim], 'v': [dc.xdim]})
    lat = LatticeU1(nb, L)
    nws = cfgs.NetWeights(x=cfgs.NetWeight(*nwx), v=cfgs.NetWeight(*nwv))
    dyn = Dynamics(lat.action, dc, NetworkFactory(spec, nc, cfgs.ConvolutionConfig(),
                                                  net_weights=nws)).eval()
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for n_, p in dyn.named_parameters():
            if n_.endswith('coeff'):
                p.copy_(0.3 * torch.randn(p.shape, generator=g).to(p.device))
    sd = {k: v.detach().cpu().numpy() for k, v in dyn.state_dict().items()
          if not k.startswith('networks.')}
    kw = dict(nunits=1, activation='leaky_relu', conv=None, use_batch_norm=False)

    def vnet(step, x, f):
        return onet.leapfrog_layer(x, f, helpers.sub(sd, f'vnet.{step}.'), nw=nwv, **kw)

    def xnet(step, first, x, v):
        which = 'first' if first else 'second'
        return onet.leapfrog_layer(x, v, helpers.sub(sd, f'xnet.{step}.{which}.'), nw=nwx, **kw)
    orc = DynamicsOracle('U1', tuple(L), nlf, [sd[f'xeps.{i}'] for i in range(nlf)],
                         [sd[f'veps.{i}'] for i in range(nlf)],
                         np.stack([host(m)[0] for m in dyn.masks]), vnet=vnet, xnet=xnet,
                         dtype=np.float32)
    x = lat.random()
    nrm = torch.randn(nb, 2, *L, generator=g).numpy()
    u = np.full(nb, 0.5, dtype=np.float32)
    want_x, want_m = orc.apply_transition_fb(host(x), beta, nrm, u)
    for fused in (True, False):
        dyn.fuse_u1_steps = fused
        dyn._inject = {'normals': nrm, 'u': u}
        xo, m = dyn((x, torch.tensor(beta)))
        assert err(host(m['acc']), want_m['acc']) < 2e-3, fused
        d = np.abs(np.angle(np.exp(1j * (host(xo) - want_x.reshape(nb, -1)))))
        assert d.max() < 2e-4, (fused, d.max())
    # all multipliers zero: generic leapfrog, sum of log-Jacobians vanishes
    from l2hmc.network.pytorch.network import LeapfrogLayer
    for mod in dyn.networks.modules():
        if isinstance(mod, LeapfrogLayer):
            mod.set_net_weight(cfgs.NetWeight(0., 0., 0.))
    dyn._inject = {'normals': nrm, 'u': u}
    xo, m = dyn((x, torch.tensor(beta)))
    assert float(m['sumlogdet'].abs().max()) < 1e-4


@pytest.mark.parametrize('sep', [False, True])
def test_su3_separate_networks_vs_oracle(sep):
    """SU(3) with one vnet per leapfrog step (use_separate_networks) or a shared one, freshly
    initialised weights, against the oracle on a merged trajectory -- the fused heads / paired
    v-update / cached-input paths must pick the right network for each step."""
    import l2hmc.configs as cfgs
    from oracle import network as onet
    from oracle.dynamics import DynamicsOracle
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.network.pytorch.network import NetworkFactory
    torch.set_default_dtype(torch.float64)
    torch.manual_seed(31)
    np.random.seed(31)
    L, nb, nlf, beta = [2, 4, 2, 2], 3, 3, 5.8
    V = int(np.prod(L))
    dc = cfgs.DynamicsConfig(nchains=nb, group='SU3', latvolume=L, nleapfrog=nlf, eps=0.02,
                             eps_hmc=0.02, verbose=False, use_split_xnets=False,
                             use_separate_networks=sep)
    nc = cfgs.NetworkConfig(units=[6, 4], activation_fn='tanh', dropout_prob=0.0,
                            use_batch_norm=False)
    spec = cfgs.InputSpec(xshape=tuple(dc.xshape), xnet={'x': [32 * V], 'v': [32 * V]},
                          vnet={'x': [32 * V], 'v': [32 * V]})
    lat = LatticeSU3(nb, L)
    dyn = Dynamics(lat.action, dc, NetworkFactory(spec, nc, cfgs.ConvolutionConfig())).eval()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n_, p in dyn.vnet.named_parameters():
            if n_.endswith('coeff'):
                p.copy_(0.3 * torch.randn(p.shape, generator=g, dtype=torch.float64).to(p.device))
    sd = {k: v.detach().cpu().numpy() for k, v in dyn.vnet.state_dict().items()}

    def vnet(step, xv, fv):
        return onet.leapfrog_layer(xv, fv, helpers.sub(sd, f'{step}.') if sep else sd, nunits=2,
                                   activation='tanh')
    xeps = [float(e.detach()) for e in dyn.xeps]
    veps = [float(e.detach()) for e in dyn.veps]
    orc = DynamicsOracle('SU3', tuple(L), nlf, xeps, veps,
                         np.stack([host(m)[0] for m in dyn.masks]), vnet=vnet)
    x = lat.random()
    nrm = torch.randn(8, nb, 4, *L, generator=g, dtype=torch.float64).numpy()
    u = np.full(nb, 0.5)
    want_x, want_m = orc.apply_transition_fb(host(x), beta, nrm, u)
    dyn._inject = {'normals': nrm, 'u': u}
    xo, m = dyn((x, torch.tensor(beta)))
    assert err(host(m['acc']), want_m['acc']) < 1e-6
    assert err(host(xo), want_x.reshape(nb, -1)) < 1e-8
    # same trajectory without the structural savings (input cache, paired v-updates, fused heads)
    dyn.reuse_v_inputs = dyn.pair_v_updates = False
    dyn._inject = {'normals': nrm, 'u': u}
    xo2, m2 = dyn((x, torch.tensor(beta)))
    assert err(host(xo2), host(xo)) < 1e-10 and err(host(m2['acc']), host(m['acc'])) < 1e-9


@pytest.mark.parametrize('group', ['U1', 'SU3'])
def test_save_load_init_weights_reversibility(group, tmp_path):
    """Dynamics.save / load (networks/dynamics.pt + xeps.npy / veps.npy, dynamics.py:537-614):
    a second instance restored from disk reproduces the trajectory bit for bit; init_weights
    changes it; test_reversibility: the U(1) generalised leapfrog is reversible to fp32 round-off,
    the SU(3) one only approximately."""
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.lattice.u1.pytorch.lattice import LatticeU1
    from l2hmc.network.pytorch.network import NetworkFactory

    def build(seed, ncp=True):
        torch.manual_seed(seed)
        np.random.seed(3)                    # masks come from numpy: same masks in both builds
        if group == 'U1':
            if torch.get_default_dtype() != torch.float64:
                torch.set_default_dtype(torch.float32)
            L, nb = [4, 6], 4
            dc = cfgs.DynamicsConfig(nchains=nb, group='U1', latvolume=L, nleapfrog=2, eps=0.05,
                                     eps_hmc=0.1, verbose=False, use_ncp=ncp)
            spec = cfgs.InputSpec(xshape=tuple(dc.xshape), xnet={'x': [dc.xdim, 2], 'v': [dc.xdim]},
                                  vnet={'x': [dc.xdim], 'v': [dc.xdim]})
            lat = LatticeU1(nb, L)
        else:
            torch.set_default_dtype(torch.float64)
            L, nb = [2, 2, 2, 4], 3
            V = int(np.prod(L))
            dc = cfgs.DynamicsConfig(nchains=nb, group='SU3', latvolume=L, nleapfrog=2, eps=0.01,
                                     eps_hmc=0.02, verbose=False, use_split_xnets=False,
                                     use_separate_networks=False)
            spec = cfgs.InputSpec(xshape=tuple(dc.xshape), xnet={'x': [32 * V], 'v': [32 * V]},
                                  vnet={'x': [32 * V], 'v': [32 * V]})
            lat = LatticeSU3(nb, L)
        nc = cfgs.NetworkConfig(units=[6], activation_fn='tanh', dropout_prob=0.0,
                                use_batch_norm=False)
        return Dynamics(lat.action, dc, NetworkFactory(spec, nc, cfgs.ConvolutionConfig())).eval(), lat
    a, lat = build(1)
    with torch.no_grad():
        for i, e in enumerate(a.xeps):
            e.fill_(0.03 + 0.01 * i)
    a.save(tmp_path)
    # as in the reference, save() hands its own `networks/` directory to save_eps(), which
    # appends another one (dynamics.py:537-557); restore_eps() reads from there, load() does not
    assert (tmp_path / 'networks' / 'dynamics.pt').exists()
    assert (tmp_path / 'networks' / 'networks' / 'xeps.npy').exists()
    b, _ = build(2)                              # different weights ...
    with pytest.raises(FileNotFoundError):
        b.load(tmp_path)                         # (the reference's load() has the same mismatch)
    b.load_state_dict(torch.load(tmp_path / 'networks' / 'dynamics.pt'))
    b.restore_eps(tmp_path)                      # ... until restored
    x = lat.random()
    beta = torch.tensor(2.0 if group == 'U1' else 6.0)
    shape = (x.shape[0], 2, 4, 6) if group == 'U1' else (8, x.shape[0], 4, 2, 2, 2, 4)
    nrm = np.random.default_rng(5).standard_normal(shape)
    nrm = nrm.astype(np.float32) if group == 'U1' else nrm
    u = np.full(x.shape[0], 0.5, dtype=np.float32 if group == 'U1' else np.float64)
    outs = []
    for d_ in (a, b):
        d_._inject = {'normals': nrm, 'u': u}
        xo, m = d_((x, beta))
        outs.append((xo.clone(), m['acc'].clone(), m['mc_states'].proposed.x.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert abs(b._eps('x', 1) - a._eps('x', 1)) < 1e-7
    b.init_weights('xavier_uniform')
    b._inject = {'normals': nrm, 'u': u}
    xo, m = b((x, beta))
    # (the PROPOSAL: x_out coincides whenever every chain rejects under both sets of weights)
    assert not torch.equal(m['mc_states'].proposed.x, outs[0][2])
    rev = a.test_reversibility()
    if group == 'U1':
        # the reference's NCP backward x-update (dynamics.py:1430-1477) is not the exact inverse of
        # its forward one: reversible to O(eps^2) only
        d = np.abs(np.angle(np.exp(1j * rev['dx'])))
        assert d.max() < 5e-2, d.max()
    else:
        assert rev['dx'].max() < 5e-2                    # not exactly reversible in the reference either


@pytest.mark.parametrize('name', helpers.MODES_U1 + helpers.MODES_SU3)
def test_from_seed_trajectory(golden, name):
    """From (lattice, beta, seed) ALONE to the reference's chain (north_star; VERDICT r03 missing
    #1, weak #2): the product is built under the fixture's seed -- no weights, masks or draws are
    injected -- and must hold the reference's networks bit for bit, leave the generator where the
    reference leaves it, draw the same start configuration, and -- with `rng_device = 'cpu'`, the
    reference's CPU stream -- reproduce its transition: direction (merge_directions=False),
    momenta, accept uniforms, **bit-exact accept mask**, energies / log-dets / x_out within the
    tolerance of the arithmetic.  The fixtures (tests/golden/make_golden_modes.py, real reference)
    cover merge_directions=False in both directions, all four U(1) network-sharing modes, SU(3)
    separate networks, BatchNorm + Dropout networks (construction-time dummy forward)."""
    g = golden(name)
    su3 = str(g['group']) == 'SU3'
    torch.set_default_dtype(torch.float64 if su3 else torch.float32)
    dyn, lat = helpers.build_from_seed(g)
    assert helpers.check_init_state(dyn, g) > 10
    assert np.array_equal(np.stack([host(m)[0] for m in dyn.masks]), g['masks'])
    assert np.array_equal(torch.rand(4).numpy(), g['probe'])
    helpers.apply_pert(dyn, g)
    dyn.eval()
    dyn.rng_device = 'cpu'
    helpers.seed_all(int(g['seed']) + 2)
    x = lat.random()
    nb = x.shape[0]
    if su3:
        assert err(host(x), g['x']) < 1e-10     # projectSU of a Gaussian matrix: conditioning ~1e3
    else:
        assert np.abs(np.angle(np.exp(1j * (host(x) - g['x'])))).max() < 1e-6
    beta = torch.tensor(float(g['beta']))
    te, ta, tx = (1e-5, 1e-5, 1e-7) if su3 else (2e-2, 1e-2, 2e-3)
    variants = [{}]
    if su3:
        variants.append({'reuse_v_inputs': False, 'pair_v_updates': False, 'fuse_heads': False})
    else:
        variants.append({'fuse_u1_steps': False})
    for kv in variants:
        for k, v_ in kv.items():
            setattr(dyn, k, v_)
        helpers.seed_all(int(g['traj_seed']))
        xo, m = dyn((x, beta))
        mc = m['mc_states']
        assert err(host(mc.init.v).reshape(nb, -1), g['v_init'].reshape(nb, -1)) < (1e-15 if su3 else 0.0 + 1e-7)
        assert np.array_equal(host(m['acc_mask']), g['acc_mask']), kv          # bit-exact
        assert err(host(m['acc']), g['acc']) < ta, kv
        assert err(host(m['energy']), g['energy']) < te, kv
        assert err(host(m['logdet']), g['logdet']) < te, kv
        assert err(host(m['sumlogdet']), g['sumlogdet']) < te, kv
        if su3:
            assert err(host(mc.proposed.x), g['x_prop']) < tx, kv
            assert err(host(xo), g['x_out']) < tx, kv
        else:
            d = np.abs(np.angle(np.exp(1j * (host(xo) - g['x_out'].reshape(nb, -1)))))
            assert d.max() < tx, (kv, d.max())


def test_auto_graphed_small_u1_transitions(golden):
    """Dynamics.auto_graph: eval-mode transitions of a launch-bound U(1) lattice replay a HIP graph behind the
    ordinary `forward` / `apply_transition_hmc` calls.  The caller owns the outputs (a second call does not
    touch them), the same device seed gives the same result as the captured graph itself, a changed model is
    re-captured, and injected draws / train mode / `auto_graph = False` stay on eager launches."""
    torch.set_default_dtype(torch.float32)
    from l2hmc import _ops as ops
    g = golden('u1_c1')
    dyn, lat = build_u1_dynamics(g, verbose=False)
    dyn.eval()
    x, beta = dev(g['x']), float(g['beta'])
    assert dyn._inject is None and not dyn._graphs
    # a key is captured the third time it is seen (a beta / step-size sweep never pays for captures), and the
    # capture leaves the device generator where it was: the draw after it is the one an eager run would make
    assert dyn.auto_graph_after == 3
    dyn((x, beta))
    dyn((x, beta))
    assert not dyn._graphs
    torch.cuda.manual_seed(5)
    xo_c, _ = dyn((x, beta))                              # captures (2 warm-up trajectories + 1), then replays
    assert len(dyn._graphs) == 1
    after_capture = torch.rand(4, device='cuda')
    torch.cuda.manual_seed(5)
    xo_r, _ = dyn((x, beta))                              # replays only
    assert torch.equal(xo_c, xo_r) and torch.equal(after_capture, torch.rand(4, device='cuda'))
    dyn._graphs.clear()
    dyn._graph_seen.clear()
    dyn.auto_graph_after = 1
    xo1, m1 = dyn((x, beta))
    assert len(dyn._graphs) == 1
    gt = next(iter(dyn._graphs.values()))
    keep = {k: v.clone() for k, v in (('x', xo1), ('acc', m1['acc']), ('px', m1['mc_states'].proposed.x))}
    xo2, m2 = dyn((x, beta))
    assert err(host(xo1), host(keep['x'])) == 0.0 and err(host(m1['acc']), host(keep['acc'])) == 0.0
    assert err(host(m1['mc_states'].proposed.x), host(keep['px'])) == 0.0
    assert err(host(m2['mc_states'].proposed.x), host(keep['px'])) > 0.0          # fresh momenta
    assert xo1.data_ptr() != xo2.data_ptr() != gt.out_x.data_ptr()
    # same device seed -> the captured graph's own result, copied out
    torch.cuda.manual_seed(11)
    xo_a, m_a = dyn((x, beta))
    torch.cuda.manual_seed(11)
    xo_g, m_g = gt(x)
    assert err(host(xo_a), host(xo_g)) == 0.0 and err(host(m_a['acc']), host(m_g['acc'])) == 0.0
    assert gt.captures == 1
    # the model changes: re-captured, still one graph
    with torch.no_grad():
        for p in dyn.vnet.parameters():
            p.mul_(0.5)
    ops.PARAM_GENERATION[0] += 1
    dyn((x, beta))
    assert gt.captures == 2 and len(dyn._graphs) == 1
    # HMC flavour gets its own graph
    xh, mh = dyn.apply_transition_hmc((x, beta), eps=0.1, nleapfrog=4)
    assert len(dyn._graphs) == 2 and bool(torch.isfinite(mh['acc']).all())
    # eager routes: injected draws (parity), the switch, train mode
    n = len(dyn._graphs)
    dyn._inject = {'normals': dev(g['normals']), 'u': dev(g['u'])}
    xo_e, m_e = dyn((x, beta))
    dyn._inject = None
    dyn.auto_graph = False
    dyn((x, beta))
    dyn.auto_graph = True
    dyn.train()
    assert dyn._auto_graphed('fb', x, beta) is None
    dyn.eval()
    assert len(dyn._graphs) == n and gt.captures == 2


def test_auto_graphed_su3_transitions(golden):
    """Dynamics.auto_graph_su3 (opt-in; fields <= 1 GiB): eval-mode `forward` replays a HIP graph; x_out and the
    [nb] metrics are the caller's own copies, the lazily formed mc_states read the replay's native buffers -- equal
    to the captured graph's own result under the same device seed -- and REFUSE to be read once the sampler has
    moved on; injected draws and `auto_graph = False` stay eager."""
    torch.set_default_dtype(torch.float64)
    g = golden('su3_l2hmc')
    dyn, lat = build_su3_dynamics(g, verbose=False)
    dyn.eval()
    x, beta = dev(g['x']), float(g['beta'])
    assert dyn._inject is None and not dyn._graphs
    dyn((x, beta))
    assert not dyn._graphs                               # SU(3): opt-in
    dyn.auto_graph_su3 = True
    dyn.auto_graph_after = 1
    torch.cuda.manual_seed(3)
    xo1, m1 = dyn((x, beta))
    assert len(dyn._graphs) == 1
    gt = next(iter(dyn._graphs.values()))
    px1 = m1['mc_states'].proposed.x.clone()            # read right after the call: fine
    keep = xo1.clone()
    torch.cuda.manual_seed(4)
    xo2, m2 = dyn((x, beta))
    px2 = m2['mc_states'].proposed.x                      # (formed now: the caller's tensor from here on)
    assert err(host(xo1), host(keep)) == 0.0 and xo1.data_ptr() != xo2.data_ptr() != gt.out_x.data_ptr()
    with pytest.raises(RuntimeError, match='NEXT transition'):
        m1['mc_states'].init.v                           # first access after the sampler moved on
    assert err(host(m1['mc_states'].proposed.x), host(px1)) == 0.0   # (already formed: the caller's tensor)
    # same device seed -> the captured graph's own result
    torch.cuda.manual_seed(4)
    xo_g, m_g = gt(x)
    assert err(host(xo2), host(xo_g)) == 0.0 and err(host(m2['acc']), host(m_g['acc'])) == 0.0
    assert err(host(px2), host(m_g['mc_states'].proposed.x)) == 0.0
    # a big device-to-host copy on the null stream between two replays (what `x_out.cpu()` in a sampler loop is):
    # on ROCm 7.0 it corrupts replayed graphs that contain a memset NODE -- the launch paths record none
    # (csrc/l2q_common.hpp::launch_zero, gemm_sliced.hip::gs_flag_dev); same seed -> same trajectory, before and after
    big = torch.zeros(8 << 20, dtype=torch.uint8, device='cuda').cpu()
    torch.cuda.manual_seed(4)
    xo3, m3 = dyn((x, beta))
    assert bool(torch.isfinite(m3['acc']).all())
    assert err(host(xo3), host(xo2)) == 0.0 and err(host(m3['acc']), host(m2['acc'])) == 0.0
    # eager routes
    n = len(dyn._graphs)
    dyn._inject = {'normals': dev(g['normals']), 'u': dev(g['u'])}
    xo_e, m_e = dyn((x, beta))
    assert np.array_equal(host(m_e['acc_mask']), g['acc_mask'])
    dyn._inject = None
    dyn.auto_graph = False
    dyn((x, beta))
    assert len(dyn._graphs) == n


@pytest.mark.parametrize('merge', [True, False], ids=['merged', 'single'])
def test_su3_sampler_and_tape_trajectories_agree(merge):
    """The sampler (eval mode: in-place steps, fused pair kernels -- units [16] is a whole K-slab, so verbose=True
    takes the mid-point pair kernel and the metrics of a step arrive one call late) and the training tape
    (functional steps, tape kernels) drive ONE trajectory loop (dynamics/pytorch/trajectory.py): on the same
    draws their verbose histories have the same keys and shapes and agree in value.  Odd extents (wrap-around);
    the merged sampler's first step reads its input in place; single direction: forward and backward."""
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.network.pytorch.network import NetworkFactory
    torch.set_default_dtype(torch.float64)
    torch.manual_seed(37)
    np.random.seed(37)
    L, nb, nlf, beta = [3, 4, 5, 3], 3, 2, 5.8
    V = int(np.prod(L))
    dc = cfgs.DynamicsConfig(nchains=nb, group='SU3', latvolume=L, nleapfrog=nlf, eps=0.02, eps_hmc=0.02,
                             verbose=True, use_split_xnets=False, use_separate_networks=False,
                             merge_directions=merge)
    nc = cfgs.NetworkConfig(units=[16], activation_fn='tanh', dropout_prob=0.0, use_batch_norm=False)
    spec = cfgs.InputSpec(xshape=tuple(dc.xshape), xnet={'x': [32 * V], 'v': [32 * V]},
                          vnet={'x': [32 * V], 'v': [32 * V]})
    lat = LatticeSU3(nb, L)
    dyn = Dynamics(lat.action, dc, NetworkFactory(spec, nc, cfgs.ConvolutionConfig()))
    assert dyn._can_pair_mid() and dyn.pair_v_updates_verbose
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n_, p in dyn.vnet.named_parameters():
            if n_.endswith('coeff'):
                p.copy_(0.3 * torch.randn(p.shape, generator=g, dtype=torch.float64).to(p.device))
    x = lat.random()
    nrm = torch.randn(8, nb, 4, *L, generator=g, dtype=torch.float64).numpy()
    seeds = {}                                      # direction the host generator draws -> a seed that draws it
    for s in range(16):
        torch.manual_seed(s)
        seeds.setdefault(bool(torch.rand(1) > 0.5), s)
    assert len(seeds) == 2
    for seed in ([seeds[True]] if merge else [seeds[True], seeds[False]]):
        rel = helpers.sampler_vs_tape(dyn, x, beta, nrm, np.full(nb, 0.5), seed)
        print(merge, seed, rel)
        # two kernel routes through one trajectory: the bound of test_sizes_gpu.py (the kernels round
        # differently at 1e-16 and projectSU(force) in front of the vnet amplifies that by ~1e7 per step)
        assert max(rel.values()) <= 1e-7, rel
