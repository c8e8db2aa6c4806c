"""The sampler's leapfrog step lives in two places -- `trajectory.SamplerStepper` (everything local to one trajectory:
kept v-update inputs, paired and deferred v-updates, kernel energies) and the stateless `Dynamics._lf_n` -- and the
other trajectory tests compare VALUES between knob settings.  Here: the ORDER of the launches of one trajectory, and
the stepper against a loop over the stateless step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L, BETA = (4, 4, 4, 4), 6.0


def build(nb, units, separate, verbose, merge=True):
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.network.pytorch.network import NetworkFactory
    torch.manual_seed(0)
    np.random.seed(0)
    V = int(np.prod(L))
    dc = cfgs.DynamicsConfig(nchains=nb, group='SU3', latvolume=list(L), nleapfrog=2, eps=0.02, eps_hmc=0.02,
                             verbose=verbose, use_split_xnets=False, use_separate_networks=separate,
                             merge_directions=merge)
    spec = cfgs.InputSpec(xshape=tuple(dc.xshape), xnet={'x': [32 * V], 'v': [32 * V]},
                          vnet={'x': [32 * V], 'v': [32 * V]})
    nc = cfgs.NetworkConfig(units=units, activation_fn='tanh', dropout_prob=0.0, use_batch_norm=False)
    lat = LatticeSU3(nb, list(L))
    dyn = Dynamics(lat.action, dc, NetworkFactory(spec, nc, cfgs.ConvolutionConfig())).cuda().eval()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():                            # (ScaledTanh coefficients start at 0: s = q = 0 without this)
        for n_, p in dyn.vnet.named_parameters():
            if n_.endswith('coeff'):
                p.copy_(0.3 * torch.randn(p.shape, generator=g, dtype=torch.float64).to(p.device))
    x = lat.g.compat_proj(lat.random().cuda())
    draws = {'normals': torch.randn(8, nb, 4, *L, generator=g, dtype=torch.float64).numpy(),
             'u': torch.rand(nb, generator=g).numpy()}
    return dyn, x, draws


@pytest.fixture
def launches(monkeypatch):
    """the entry points of libl2q.so in the order they are called; the size rule of the sliced layers lifted
    (a 4^4 lattice takes them, as in test_digits_trajectory_gpu.py)"""
    from l2hmc import _ops as ops
    from l2hmc import native
    monkeypatch.setattr(ops, 'gemm_sliced_pays', ops.gemm_sliced_ok)
    names = []

    def call(name, *args, _call=native.call):
        names.append(name.removeprefix('l2q_'))
        return _call(name, *args)
    monkeypatch.setattr(native, 'call', call)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield names
    torch.set_default_dtype(old)


# The launches of ONE Dynamics.forward (merged directions, nleapfrog = 2, injected draws), second trajectory of the
# module (the first also builds the digit images of the weights).  Recorded on the commit BEFORE the step moved into
# SamplerStepper (l2hmc at "Single-source the int8-sliced input layer's GEMM core"), one line per v-slot + x-update.
HEAD = 'su3_pack su3_assemble_tah su3_kinetic_reduce su3_plaq_reduce '
TAIL = ' accept su3_unpack_select'
# units [256], 64 chains: digit inputs, int8-sliced heads (one entry point for single and paired updates); the closing
# force launch returns the potential, the closing heads kernel the kinetic energy
SLICED = 'su3_projsu_digits gemm_digits_f64 vnet_heads_vupdate_sliced_f64'
DEFAULT = (HEAD + f'su3_force su3_projsu_digits {SLICED} su3_expm_mul2_digits '
           + 3 * f'su3_force {SLICED} su3_expm_mul2_digits '
           + f'su3_force_action {SLICED}' + TAIL)
# ... verbose: the potential of every x a step produced comes out of the force launch on it
DEFAULT_VERBOSE = (HEAD + f'su3_force su3_projsu_digits {SLICED} su3_expm_mul2_digits '
                   + 3 * f'su3_force_action {SLICED} su3_expm_mul2_digits '
                   + f'su3_force_action {SLICED}' + TAIL)
# units [16], one vnet per leapfrog step: adjacent v-updates on DIFFERENT networks are two single updates on one force
# and one projection; the direction change (same step, same network) is the pair kernel with the flip inside; fp64
# heads emit no |v|^2 (the closing kinetic energy is a pass)
ONE = 'gemm_f64 vnet_heads_vupdate_f64'
SEPARATE = (HEAD + 'su3_force su3_projsu_vec8 su3_projsu_vec8 gemm_f64 vnet_heads_vupdate_to_f64 su3_expm_mul2_vec8 '
            + f'su3_force su3_projsu_vec8 {ONE} {ONE} su3_expm_mul2_vec8 '
            + 'su3_force su3_projsu_vec8 gemm_f64 vnet_heads_vupdate_pair_f64 su3_expm_mul2_vec8 '
            + f'su3_force su3_projsu_vec8 {ONE} {ONE} su3_expm_mul2_vec8 '
            + f'su3_force_action su3_projsu_vec8 {ONE} su3_kinetic_reduce' + TAIL)
# ... verbose: the kinetic energy between two single updates is a pass, the mid-point pair kernel returns its own
SEPARATE_VERBOSE = (
    HEAD + 'su3_force su3_projsu_vec8 su3_projsu_vec8 gemm_f64 vnet_heads_vupdate_to_f64 su3_expm_mul2_vec8 '
    + f'su3_force_action su3_projsu_vec8 {ONE} su3_kinetic_reduce {ONE} su3_expm_mul2_vec8 '
    + 'su3_force_action su3_projsu_vec8 gemm_f64 vnet_heads_vupdate_pair_mid_f64 su3_expm_mul2_vec8 '
    + f'su3_force_action su3_projsu_vec8 {ONE} su3_kinetic_reduce {ONE} su3_expm_mul2_vec8 '
    + f'su3_force_action su3_projsu_vec8 {ONE} su3_kinetic_reduce' + TAIL)


@pytest.mark.parametrize('nb,units,separate,verbose,want', [
    (64, [256], False, False, DEFAULT), (64, [256], False, True, DEFAULT_VERBOSE),
    (4, [16], True, False, SEPARATE), (4, [16], True, True, SEPARATE_VERBOSE)],
    ids=['default', 'default-verbose', 'separate', 'separate-verbose'])
def test_launch_sequence_of_a_trajectory(launches, nb, units, separate, verbose, want):
    dyn, x, draws = build(nb, units, separate, verbose)
    for _ in range(2):
        dyn._inject = draws
        del launches[:]
        dyn((x, BETA))
        dyn._inject = None
    assert launches == want.split()


@pytest.mark.parametrize('directions', [(True, False), (True,), (False,)], ids=['merged', 'forward', 'backward'])
@pytest.mark.parametrize('nb,units,separate', [(64, [64], False), (3, [18], False), (3, [16], True)],
                         ids=['u64', 'u18', 'separate'])
def test_stepper_equals_a_loop_over_the_stateless_step(launches, nb, units, separate, directions):
    """With nothing kept between steps (reuse_v_inputs = pair_v_updates = False, kernel energies off) the stepper's
    trajectory is the stateless `Dynamics._lf_n` in a loop, bit for bit: proposal, sum of logdets, accept probability
    (the merged stepper still reads its input in place where the loop works on copies)."""
    from l2hmc import _ops as ops
    from l2hmc.dynamics.pytorch.trajectory import SamplerStepper, run_trajectory
    merged = len(directions) == 2
    dyn, x, draws = build(nb, units, separate, False, merged)
    dyn.reuse_v_inputs = dyn.pair_v_updates = False
    nlf = dyn.config.nleapfrog
    dyn._inject = draws
    xn, vn = dyn._pack(x), dyn._momentum_n(nb)
    dyn._inject = None
    ops.USE_KERNEL_ENERGIES[0] = False
    try:
        x1, v1, hist, _, _ = run_trajectory(dyn, SamplerStepper(dyn, BETA, merged), xn, vn, BETA, directions)
        x2, v2 = xn.clone(), vn.clone()
        h0, sld = dyn._hamiltonian_n(xn, vn, BETA), dyn._zeros_nb(nb)
        for i, forward in enumerate(directions):
            if i > 0:
                dyn._flip_v_n(v2)
            for step in range(nlf):
                sld = sld + dyn._lf_n(step, x2, v2, BETA, forward)
        h1 = dyn._hamiltonian_n(x2, v2, BETA)
        acc = dyn._accept_prob_n(h0, h1, sld) if merged else dyn._accept_prob_n(h1, h0, sld)
    finally:
        ops.USE_KERNEL_ENERGIES[0] = True
    assert torch.equal(x1, x2) and torch.equal(v1, v2)
    assert torch.equal(hist['sumlogdet'], sld) and torch.equal(hist['acc'], acc)
    assert bool(torch.isfinite(acc).all()) and float(sld.abs().max()) > 0
