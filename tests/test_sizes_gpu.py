"""GPU parity at the BASELINE shapes themselves (VERDICT r01 "next" item 1).

The reference goldens are 3x4x5x3 lattices (spatial volume 60 => only the fall-back kernels run).
These tests run the kernels that cfg-4 / cfg-5 actually launch -- slice-resident plaquette /
force, split-K input GEMM with K = 262 144 (8^4) / 4 194 304 (16^4), fused heads with
N = 147 456 / 2 359 296 -- against the numpy oracle on the same seeded inputs:

* cfg-4: ``Dynamics`` at 8^4, vnet units [256], one merged nleapfrog = 4 trajectory with injected
  draws (x_prop, energies, acc, bit-exact accept mask with one accept and one reject).
* cfg-5: 16^4 with a full 256-chain allocation (9.66 GB per field: byte offsets past 2^32,
  chain * 36 * V element offsets up to 6e8).  The 256 chains are copies of 2 distinct chains
  (chain c = base[c % 2]), every chain of every kernel output is compared on the device with
  the oracle's result for its base chain -- so an index that wraps anywhere in the allocation
  shows up.  Kernels, a plain-HMC transition and one merged L2HMC trajectory (nleapfrog = 1,
  units [256]: 23 GB of fp64 weights).
* cfg-2 / cfg-3: U(1) 16 x 16, beta 4, **2048 chains**, nleapfrog 8, fp32 and
  64 x 64, beta 6, **8192 chains**, fp16 nets / fp32 action, each with the reference's default conv
  network and a dense one, against fixtures the REAL reference produced at those shapes on two
  chains (tests/golden/make_golden_sizes.py; the weights -- up to 2.3e9 numbers -- are the
  counter-based ones of tests/golden/seeded.py, regenerated here on the device).  The chains are
  copies of the fixture's two; every chain is compared on the device, accept masks bit-exact.
"""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(autouse=True)
def _f64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)
    gc.collect()
    torch.cuda.empty_cache()


def _build(L, nb, nlf, units, eps, head_scale, seed):
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.network.pytorch.network import NetworkFactory
    V = int(np.prod(L))
    torch.manual_seed(seed)
    np.random.seed(seed)
    dc = cfgs.DynamicsConfig(nchains=nb, group='SU3', latvolume=list(L), nleapfrog=nlf, eps=eps,
                             eps_hmc=eps, verbose=True, use_split_xnets=False,
                             use_separate_networks=False, merge_directions=True)
    nc = cfgs.NetworkConfig(units=list(units), activation_fn='tanh', dropout_prob=0.0,
                            use_batch_norm=False)
    spec = cfgs.InputSpec(xshape=tuple(dc.xshape), xnet={'x': [32 * V], 'v': [32 * V]},
                          vnet={'x': [32 * V], 'v': [32 * V]})
    lat = LatticeSU3(nb, list(L))
    nf = NetworkFactory(spec, nc, cfgs.ConvolutionConfig(),
                        cfgs.NetWeights(x=cfgs.NetWeight(0., 1., 1.), v=cfgs.NetWeight(1., 1., 1.)))
    dyn = Dynamics(lat.action, dc, nf)
    # random-init heads are O(1) per entry: dH ~ -50 over a trajectory and every chain rejects
    # with acc = 1e-20.  Scaling the three head layers (weights are inputs of the test, the
    # same numbers go to the oracle) puts acc strictly inside (0, 1).
    with torch.no_grad():
        for lin in (dyn.vnet.scale.layer, dyn.vnet.transl, dyn.vnet.transf.layer):
            lin.weight.mul_(head_scale)
            lin.bias.mul_(head_scale)
    dyn.eval()
    return dyn, lat


def _oracle(dyn, L, nlf, units):
    from oracle import network as onet
    from oracle.dynamics import DynamicsOracle
    w = {k: host(v) for k, v in dyn.vnet.state_dict().items()}

    def vnet(step, xv, fv):
        return onet.leapfrog_layer(xv, fv, w, nunits=len(units), activation='tanh')
    xe = [float(p) for p in dyn.xeps]
    ve = [float(p) for p in dyn.veps]
    masks = [host(m).reshape(-1) for m in dyn.masks]
    return DynamicsOracle('SU3', tuple(L), nlf, xe, ve, masks, vnet=vnet)


def _hot(rng, nb, L):
    from oracle import su3 as osu3
    z = rng.normal(size=(nb, 4, *L, 3, 3)) + 1j * rng.normal(size=(nb, 4, *L, 3, 3))
    return osu3.project_su(z)


def _warm(rng, nb, L, delta=0.1):
    """near-cold start exp(delta * TAH): plaquette ~0.95.  From a hot start the leapfrog energy
    error has one sign (H decreases, acc = 1 for every chain); here dH < 0 with acc inside (0, 1),
    so accept AND reject outcomes can be pinned."""
    from oracle import su3 as osu3
    return osu3.expm(delta * osu3.rand_tah3(rng.normal(size=(8, nb, 4, *L))))


def _mixed_uniforms(acc):
    """accept uniforms giving alternating accept / reject with a margin of half the gap"""
    assert np.all(acc > 1e-3) and np.all(acc < 1 - 1e-3), f'acc not inside (0,1): {acc}'
    u = np.where(np.arange(acc.size) % 2 == 0, 0.5 * (1.0 + acc), 0.5 * acc)
    return u


def test_cfg4_trajectory_8x4_units256():
    """8^4, units [256], nleapfrog 4 merged: the shapes bench.py times."""
    L, nb, nlf, units = (8, 8, 8, 8), 2, 4, [256]
    dyn, lat = _build(L, nb, nlf, units, eps=0.01, head_scale=0.03, seed=11)
    orc = _oracle(dyn, L, nlf, units)
    rng = np.random.default_rng(4)
    x = _hot(rng, nb, L)
    nrm = rng.normal(size=(8, nb, 4, *L))
    beta = 6.0
    xo_ref, mo = orc.apply_transition_fb(x, beta, nrm, np.zeros(nb), history=True)
    u = _mixed_uniforms(mo['acc'])
    xo_ref, mo = orc.apply_transition_fb(x, beta, nrm, u, history=True)
    assert mo['acc_mask'].tolist() == [0.0, 1.0]
    from l2hmc import _ops as ops
    for verbose in (True, False):
        dyn.config.verbose = verbose
        dyn._inject = {'normals': nrm, 'u': u}
        xo, m = dyn((dev(x), torch.tensor(beta)))
        mc = m['mc_states']
        assert np.abs(host(mc.init.v) - mo['v_init']).max() < 1e-14
        # same conditioning as the 3x4x5x3 golden (projectSU(force) feeds the vnet)
        assert np.abs(host(mc.proposed.x) - mo['x_prop']).max() < 1e-7
        assert np.abs(host(mc.proposed.v) - mo['v_prop']).max() < 1e-6
        assert np.abs(host(m['acc']) - mo['acc']).max() < 1e-5
        assert np.array_equal(host(m['acc_mask']), mo['acc_mask'])       # bit-exact
        assert np.abs(host(m['sumlogdet']) - mo['acc_mask'] * mo['sumlogdet']).max() < 1e-6
        assert np.abs(host(xo) - xo_ref.reshape(nb, -1)).max() < 1e-7
        if verbose:
            assert m['energy'].shape == (2 * nlf + 1, nb)
            assert np.abs(host(m['energy']) - mo['energy']).max() < 1e-5  # |H| ~ 2.6e2
            assert np.abs(host(m['logdet']) - mo['logdet']).max() < 1e-6
    # verbose=True with and without the mid-point pair kernel (9 vs 16 heads kernels): the same
    # per-step history (energy, logdet, forward / backward partial sums) to rounding
    hist = {}
    for pv in (True, False):
        dyn.config.verbose = True
        dyn.pair_v_updates_verbose = pv
        dyn._inject = {'normals': nrm, 'u': u}
        xo_v, m_v = dyn((dev(x), torch.tensor(beta)))
        hist[pv] = {k: host(m_v[k]) for k in ('energy', 'logprob', 'logdet', 'sldf', 'sldb', 'sld', 'acc')}
        hist[pv]['x'] = host(xo_v)
    dyn.pair_v_updates_verbose = True
    dyn.config.verbose = False
    for k, a in hist[True].items():
        b = hist[False][k]
        assert a.shape == b.shape, k
        # the two kernels round differently at 1e-16 and projectSU(force) in front of the vnet
        # amplifies that by ~1e7 per step (see the golden's conditioning note): 1e-7, one order
        # inside the tolerance against the oracle above
        assert np.abs(a - b).max() <= 1e-7 * max(1.0, np.abs(b).max()), (k, np.abs(a - b).max())
    # the heads ran on the int8-sliced kernel (units [256] qualifies; csrc/heads_sliced.hip); the fp64
    # MFMA heads give the same trajectory to rounding
    vn = dyn._get_vnet(0)
    pm = dyn._perms()
    assert vn.kernel_weights(pm['in'], pm['out'])['heads_scaled'].get('sliced') is not None
    try:
        ops.USE_SLICED_HEADS[0] = False
        dyn._inject = {'normals': nrm, 'u': u}
        xo_f, m_f = dyn((dev(x), torch.tensor(beta)))
    finally:
        ops.USE_SLICED_HEADS[0] = True
    assert np.array_equal(host(m_f['acc_mask']), mo['acc_mask'])
    assert np.abs(host(xo_f) - host(xo)).max() <= 1e-7
    assert np.abs(host(m_f['acc']) - host(m['acc'])).max() <= 1e-7
    # observables of the output configuration through the slice-resident plaquette kernel
    from oracle import su3 as osu3
    met = lat.calc_metrics(xo.reshape(x.shape))
    xo4 = xo_ref.reshape(x.shape)
    assert np.abs(host(met['plaqs']) - osu3.plaqs(xo4)).max() < 1e-10
    assert np.abs(host(met['intQ']) - osu3.int_charges(xo4)).max() < 1e-9
    assert np.abs(host(met['sinQ']) - osu3.sin_charges(xo4)).max() < 1e-9
    # all variants of the force kernel agree at this shape, and so does the plaquette kernel
    xn = ops.su3_pack(dev(x))
    f_ref = osu3.grad_action(x, beta)
    from l2hmc import native
    try:
        for ft in (7, 5, 2):
            native.set_tuning('force_tile', ft)
            f = ops.su3_unpack(ops.su3_force_n(xn, beta, L), L)
            assert np.abs(host(f) - f_ref).max() < 1e-12, ft
    finally:
        native.set_tuning('force_tile', 5)
    s = host(ops.su3_plaq_sums_n(xn, L))
    re, im = osu3.plaq_sums(x)
    assert np.abs(s - np.stack([re, im], 1)).max() < 1e-8


def test_cfg4_trajectory_8x4_256chains():
    """cfg-4 AS ITSELF: 8^4, beta 6, **256 chains**, units [256], nleapfrog 4 merged -- the exact
    launches bench.py times (M = 256 x N = 147 456 sliced heads with 4 row groups per column
    worker, the 256-chain split-K input GEMM, 1 048 576-site force / update kernels).  The chains
    are copies of two distinct chains (chain c = base[c % 2]) whose oracle trajectory has one
    accept and one reject; EVERY chain of every output is compared on the device (VERDICT r03
    weak #3)."""
    L, nb, nlf, units = (8, 8, 8, 8), 256, 4, [256]
    dyn, lat = _build(L, nb, nlf, units, eps=0.01, head_scale=0.03, seed=11)
    orc = _oracle(dyn, L, nlf, units)
    rng = np.random.default_rng(4)
    x2 = _hot(rng, 2, L)
    nrm2 = rng.normal(size=(8, 2, 4, *L))
    beta = 6.0
    _, mo = orc.apply_transition_fb(x2, beta, nrm2, np.zeros(2), history=True)
    u2 = _mixed_uniforms(mo['acc'])
    xo_ref, mo = orc.apply_transition_fb(x2, beta, nrm2, u2, history=True)
    assert mo['acc_mask'].tolist() == [0.0, 1.0]
    x = _tile(dev(x2), nb)
    nrm = dev(nrm2).repeat(1, nb // 2, *([1] * 5)).contiguous()
    u = dev(u2).repeat(nb // 2)
    want_mask = torch.from_numpy(mo['acc_mask']).repeat(nb // 2)
    from l2hmc import _ops as ops
    vn = dyn._get_vnet(0)
    pm = dyn._perms()
    # (heads on the int8 cores, input layer on the int8 cores): both are the default at this shape; the
    # fp64 MFMA kernels behind the switches give the same trajectory to rounding
    for verbose in (False, True):
        for sliced, sliced_in in ((True, True), (False, True), (True, False)):
            dyn.config.verbose = verbose
            try:
                ops.USE_SLICED_HEADS[0] = sliced
                ops.USE_SLICED_INPUT[0] = sliced_in
                dyn._inject = {'normals': nrm, 'u': u}
                xo, m = dyn((x, torch.tensor(beta)))
            finally:
                ops.USE_SLICED_HEADS[0] = True
                ops.USE_SLICED_INPUT[0] = True
            kw = vn.kernel_weights(pm['in'], pm['out'])
            if sliced:
                assert kw['heads_scaled'].get('sliced') is not None
            if sliced_in:
                assert kw.get('input_img') is not None            # csrc/gemm_sliced.hip ran
            tag = (verbose, sliced, sliced_in)
            assert torch.equal(m['acc_mask'].cpu(), want_mask), tag                  # bit-exact
            assert _maxdiff_tiled(m['acc'], dev(mo['acc'])) < 1e-5, tag
            assert _maxdiff_tiled(xo, dev(xo_ref.reshape(2, -1))) < 1e-7, tag
            assert _maxdiff_tiled(m['sumlogdet'], dev(mo['acc_mask'] * mo['sumlogdet'])) < 1e-6, tag
            mc = m['mc_states']
            assert _maxdiff_tiled(mc.proposed.x, dev(mo['x_prop'])) < 1e-7, tag
            assert _maxdiff_tiled(mc.proposed.v, dev(mo['v_prop'])) < 1e-6, tag
            if verbose:
                e = m['energy']
                assert e.shape == (2 * nlf + 1, nb)
                d = (e.reshape(e.shape[0], nb // 2, 2) - dev(mo['energy']).reshape(-1, 1, 2)).abs().max()
                assert float(d) < 1e-5, (tag, float(d))
                d = (m['logdet'].reshape(e.shape[0], nb // 2, 2)
                     - dev(mo['logdet']).reshape(-1, 1, 2)).abs().max()
                assert float(d) < 1e-6, (tag, float(d))
            del xo, m, mc
    # observables of all 256 output chains through the slice-resident plaquette kernel
    from oracle import su3 as osu3
    dyn.config.verbose = False
    dyn._inject = {'normals': nrm, 'u': u}
    xo, m = dyn((x, torch.tensor(beta)))
    met = lat.calc_metrics(xo.reshape(x.shape))
    xo4 = xo_ref.reshape(x2.shape)
    assert _maxdiff_tiled(met['plaqs'], dev(osu3.plaqs(xo4))) < 1e-10
    assert _maxdiff_tiled(met['intQ'], dev(osu3.int_charges(xo4))) < 1e-9


# --------------------------------------------------------------------------- cfg-5 shapes
L16 = (16, 16, 16, 16)
NB16 = 256


def _tile(a2, nb=256):
    """[2, ...] device tensor -> [nb, ...] with chain c = a2[c % 2]"""
    assert a2.shape[0] == 2
    return a2.repeat(nb // 2, *([1] * (a2.dim() - 1))).contiguous()


def _maxdiff_tiled(out, ref2):
    """max |out[c] - ref2[c % 2]| over all chains, computed on the device in slabs"""
    nb = out.shape[0]
    ref2 = ref2.to(out.device)
    worst = 0.0
    for c0 in range(0, nb, 32):
        blk = out[c0:c0 + 32]
        d = (blk.reshape(blk.shape[0] // 2, 2, -1) - ref2.reshape(1, 2, -1)).abs().max()
        worst = max(worst, float(d))
    return worst


def test_cfg5_kernels_16x4_256chains():
    """Every SU(3) kernel of the trajectory on a 256-chain 16^4 allocation (9.66 GB per field)."""
    from l2hmc import _ops as ops
    from oracle import su3 as osu3
    L, V = L16, 16 ** 4
    rng = np.random.default_rng(16)
    x2 = _hot(rng, 2, L)
    v2 = osu3.rand_tah3(rng.normal(size=(8, 2, 4, *L)))
    beta, eps = 6.2, 0.05
    xn2 = ops.su3_pack(dev(x2))
    vn2 = ops.su3_pack(dev(v2))
    xn = _tile(xn2)
    vn = _tile(vn2)
    assert xn.numel() * 16 > 2 ** 32 and xn.shape == (NB16, 4, 9, V)

    def as_native(a):           # oracle result (reference layout, 2 chains) -> native, device
        return ops.su3_pack(dev(a))

    # plaquette sums / per-plane sums / kinetic energy / checkSU
    re, im = osu3.plaq_sums(x2)
    s = ops.su3_plaq_sums_n(xn, L)
    assert _maxdiff_tiled(s, dev(np.stack([re, im], 1))) < 1e-7          # sums ~ 1e4
    ke = ops.su3_kinetic_n(vn)
    assert _maxdiff_tiled(ke, dev(osu3.kinetic_energy(v2))) < 1e-6       # ~ 1e6
    av, mx = osu3.check_su(x2)      # (the closed-form projectSU itself is unitary to ~1e-9)
    assert _maxdiff_tiled(ops.su3_check_su_n(xn), dev(np.stack([av, mx], 1))) < 1e-13
    # force (slice-resident kernel) and the fused kick
    f_ref = as_native(osu3.grad_action(x2, beta))
    f = ops.su3_force_n(xn, beta, L)
    assert _maxdiff_tiled(f, f_ref) < 1e-12
    vk = vn.clone()
    ops.su3_force_kick_n(xn, beta, -0.5 * eps, vk, L)
    assert _maxdiff_tiled(vk, vn2 - 0.5 * eps * f_ref) < 1e-12
    vk2 = torch.empty_like(vn)                     # out of place: same bits
    ops.su3_force_kick_n(xn, beta, -0.5 * eps, vk2, L, v_src=vn)
    assert torch.equal(vk2, vk)
    del vk, vk2
    # su3_to_vec(projectSU(.)) of links and of the force
    xv = ops.su3_projsu_vec8_n(xn)
    xv_ref = dev(osu3.group_to_vec(x2))                                   # [2,4,T,X,Y,Z,8]
    xv_ref_n = xv_ref.reshape(2, 4, V, 8).permute(0, 1, 3, 2).contiguous()
    assert _maxdiff_tiled(xv.reshape(NB16, -1), xv_ref_n.reshape(2, -1)) < 1e-12
    del xv
    # masked expm update, both halves in one kernel
    m = (rng.random(36 * V) < 0.5).astype(np.float32)
    mn = ops.pack_entries(dev(m).reshape(1, -1), V).reshape(-1).contiguous()
    m4 = m.reshape(1, 4, *L, 3, 3)
    e = osu3.expm(eps * v2)
    y = m4 * x2 + e @ ((1 - m4) * x2)
    y = (1 - m4) * y + e @ (m4 * y)
    out = ops.su3_expm_mul2_n(xn, vn, eps, mn, False)
    assert _maxdiff_tiled(out, as_native(y)) < 1e-13
    del out, f
    # momenta from normals (randTAH3 order), tiled normals
    nrm2 = rng.normal(size=(8, 2, 4, V))
    nrm = dev(nrm2).repeat(1, NB16 // 2, 1, 1).contiguous()
    va = ops.su3_assemble_tah_n(nrm)
    assert _maxdiff_tiled(va, as_native(osu3.rand_tah3(nrm2.reshape(8, 2, 4, *L)))) < 1e-15


def test_cfg5_hmc_transition_16x4_256chains():
    """apply_transition_hmc on 256 chains of 16^4: kick / expm / plaquette / kinetic / accept /
    select at cfg-5 addresses; cold-start and unitarity properties."""
    from oracle import su3 as osu3
    from oracle.dynamics import DynamicsOracle
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.group.su3.pytorch import utils as U
    L, nb = L16, NB16
    dc = cfgs.DynamicsConfig(nchains=nb, group='SU3', latvolume=list(L), nleapfrog=1, eps=0.02,
                             eps_hmc=0.02, verbose=False, use_split_xnets=False,
                             use_separate_networks=False, merge_directions=True)
    lat = LatticeSU3(nb, list(L))
    dyn = Dynamics(lat.action, dc, None)
    rng = np.random.default_rng(160)
    x2 = _warm(rng, 2, L)
    nrm2 = rng.normal(size=(8, 2, 4, *L))
    beta, eps, nlf = 6.2, 0.01, 1
    orc = DynamicsOracle('SU3', L, 1, [eps], [eps], [np.zeros(36 * 16 ** 4, np.float32)])
    _, mo = orc.apply_transition_hmc(x2, beta, nrm2, np.zeros(2), eps, nlf)
    u2 = _mixed_uniforms(mo['acc'])
    xo_ref, mo = orc.apply_transition_hmc(x2, beta, nrm2, u2, eps, nlf)
    x = _tile(dev(x2))
    nrm = dev(nrm2).repeat(1, nb // 2, *([1] * 5)).contiguous()
    u = dev(u2).repeat(nb // 2)
    dyn.merge_hmc_kicks = False
    dyn._inject = {'normals': nrm, 'u': u}
    xo, m = dyn.apply_transition_hmc((x, torch.tensor(beta)), eps=eps, nleapfrog=nlf)
    del x, nrm
    assert _maxdiff_tiled(m['acc'], dev(mo['acc'])) < 1e-6               # |H| ~ 1e6
    assert torch.equal(m['acc_mask'].cpu(), torch.from_numpy(mo['acc_mask']).repeat(nb // 2))
    assert _maxdiff_tiled(xo, dev(xo_ref.reshape(2, -1))) < 1e-12
    xp = m['mc_states'].proposed.x
    assert _maxdiff_tiled(xp, dev(mo['x_prop'])) < 1e-12
    av, mx = U.checkSU(xp)
    assert float(mx.max()) < 1e-13
    del xp, xo, m
    gc.collect()
    torch.cuda.empty_cache()
    # cold start: every plaquette = 1, force = 0, at every chain offset
    eye = torch.eye(3, dtype=torch.complex128, device='cuda')
    xc = eye.expand(nb, 4, *L, 3, 3).contiguous()
    met = lat.calc_metrics(xc)
    assert float((met['plaqs'] - 1.0).abs().max()) < 1e-14
    assert float(met['intQ'].abs().max()) < 1e-12
    f = lat.grad_action(xc, torch.tensor(beta))
    assert float(f.abs().max()) < 1e-14


def test_cfg5_l2hmc_trajectory_16x4_256chains():
    """One merged L2HMC trajectory (nleapfrog = 1) of the cfg-5 per-GPU shard: 16^4, 256 chains,
    units [256] (K = 4 194 304 split-K input GEMM, N = 2 359 296 heads)."""
    L, nb, nlf, units = L16, NB16, 1, [256]
    free, total = torch.cuda.mem_get_info()
    if total < 200 * 2 ** 30:
        pytest.skip('needs the 288 GB of an MI355X')
    # calibrated with tools/cal_cfg5.py: from the near-cold start the element-masked x half-updates
    # (which leave the group manifold) give dH ~ -9e6 eps^2; eps = 3e-4 => dH = -0.83, acc = 0.436
    dyn, lat = _build(L, nb, nlf, units, eps=3e-4, head_scale=0.003, seed=12)
    orc = _oracle(dyn, L, nlf, units)
    rng = np.random.default_rng(5)
    x2 = _warm(rng, 2, L)
    nrm2 = rng.normal(size=(8, 2, 4, *L))
    beta = 6.2
    _, mo = orc.apply_transition_fb(x2, beta, nrm2, np.zeros(2))
    u2 = _mixed_uniforms(mo['acc'])
    xo_ref, mo = orc.apply_transition_fb(x2, beta, nrm2, u2)
    x = _tile(dev(x2))
    nrm = dev(nrm2).repeat(1, nb // 2, *([1] * 5)).contiguous()
    dyn.config.verbose = False
    dyn._inject = {'normals': nrm, 'u': dev(u2).repeat(nb // 2)}
    xo, m = dyn((x, torch.tensor(beta)))
    del x, nrm
    assert _maxdiff_tiled(m['acc'], dev(mo['acc'])) < 1e-4               # |H| ~ 1e6, 16x the sites
    assert torch.equal(m['acc_mask'].cpu(), torch.from_numpy(mo['acc_mask']).repeat(nb // 2))
    assert _maxdiff_tiled(xo, dev(xo_ref.reshape(2, -1))) < 1e-7
    assert _maxdiff_tiled(m['sumlogdet'], dev(mo['acc_mask'] * mo['sumlogdet'])) < 1e-6


# --------------------------------------------------------------------------- cfg-2 / cfg-3 shapes
def _wrap(d):
    return torch.remainder(d + np.pi, 2 * np.pi) - np.pi


def _angle_diff_tiled(out, ref2):
    """max |wrap(out[c] - ref2[c % 2])| over all chains, on the device"""
    ref2 = ref2.to(out.device).reshape(1, 2, -1)
    worst = 0.0
    for c0 in range(0, out.shape[0], 512):
        blk = out[c0:c0 + 512]
        worst = max(worst, float(_wrap(blk.reshape(blk.shape[0] // 2, 2, -1) - ref2).abs().max()))
    return worst


def _u1_full_size(golden, name, nb, tol_x, tol_acc, tol_h, fused_variants=(True,)):
    import helpers
    torch.set_default_dtype(torch.float32)
    g = golden(name)
    prec = str(g['precision'])
    dyn, lat = helpers.build_u1_seeded_dynamics(g, nb)
    if prec != 'fp32':
        dyn.set_net_precision(prec)
    L = [int(i) for i in g['latvolume']]
    assert nb % 2 == 0 and g['x'].shape[0] == 2
    x = _tile(dev(g['x']), nb)
    nrm = _tile(dev(g['normals']), nb)
    u = dev(g['u']).repeat(nb // 2)
    beta = torch.tensor(float(g['beta']))
    want_mask = torch.from_numpy(g['acc_mask']).repeat(nb // 2)
    assert g['acc_mask'].tolist() == [0.0, 1.0] and float(np.abs(g['acc'] - g['u']).min()) > 0.05
    res = {}
    for verbose in (False, True):
        for fused in fused_variants:
            dyn.config.verbose = verbose
            dyn.fuse_u1_steps = fused
            dyn._inject = {'normals': nrm, 'u': u}
            xo, m = dyn((x, beta))
            dyn._inject = None
            mc = m['mc_states']
            assert torch.equal(m['acc_mask'].cpu(), want_mask), (name, verbose, fused)   # bit-exact
            assert _maxdiff_tiled(m['acc'], dev(g['acc'])) < tol_acc, (name, verbose, fused)
            assert _angle_diff_tiled(mc.proposed.x, dev(g['x_prop'])) < tol_x, (name, verbose, fused)
            sc = float(np.abs(g['v_prop']).max())
            assert _maxdiff_tiled(mc.proposed.v, dev(g['v_prop'])) < tol_x * max(1.0, sc)
            assert _angle_diff_tiled(xo, dev(g['x_out'])) < tol_x
            assert _maxdiff_tiled(m['sumlogdet'], dev(g['sumlogdet'])) < tol_h
            if verbose:
                e = m['energy']                                   # [2 nlf + 1, nb]
                assert e.shape == (2 * int(g['nleapfrog']) + 1, nb)
                d = (e.reshape(e.shape[0], nb // 2, 2) - dev(g['energy']).reshape(-1, 1, 2)).abs().max()
                assert float(d) < tol_h, (name, float(d))
                d = (m['logdet'].reshape(e.shape[0], nb // 2, 2)
                     - dev(g['logdet']).reshape(-1, 1, 2)).abs().max()
                assert float(d) < tol_h, (name, float(d))
            res[(verbose, fused)] = float(m['acc'].mean())
    # observables of the output configuration at this chain count
    from oracle import u1 as ou1
    xo2 = g['x_out'].reshape(2, 2, *L)
    met = lat.calc_metrics(xo.reshape(nb, 2, *L))
    assert _maxdiff_tiled(met['plaqs'], dev(ou1.plaqs(xo2).astype(np.float32))) < 1e-5
    assert _maxdiff_tiled(met['intQ'], dev(ou1.int_charges(xo2).astype(np.float32))) < 2e-2
    return g, dyn


def test_cfg2_dense_16x16_2048chains(golden):
    """BASELINE cfg-2 as itself: 16 x 16, beta 4, 2048 chains, nleapfrog 8, fp32, units [16]*4
    (the fused one-launch-per-sub-update kernels and the multi-kernel path)."""
    _u1_full_size(golden, 'u1_cfg2_dense', 2048, tol_x=2e-4, tol_acc=2e-3, tol_h=5e-3,
                  fused_variants=(True, False))


def test_cfg2_conv_16x16_2048chains(golden):
    """cfg-2 with the reference's default network (conv [8,16,32,64,128] + units [16]*4)."""
    _u1_full_size(golden, 'u1_cfg2_conv', 2048, tol_x=2e-4, tol_acc=2e-3, tol_h=5e-3)


def test_cfg3_dense_fp16_64x64_8192chains(golden):
    """BASELINE cfg-3 as itself: 64 x 64, beta 6, 8192 chains, nleapfrog 8, fp16 nets / fp32 action,
    units [256, 256]: M = 8192 row tiles of gemm_h / u1_heads_update_h, 256 MiB fields.  The fixture
    is the reference under torch.autocast('cpu', float16); tolerances are multiples of the
    reference's own fp16-vs-fp32 distance (stored in the fixture)."""
    g = golden('u1_cfg3_fp16_dense')
    yard = float(np.abs(g['acc'] - g['acc_fp32']).max())
    _u1_full_size(golden, 'u1_cfg3_fp16_dense', 8192, tol_x=5e-3, tol_acc=max(3 * yard, 5e-3),
                  tol_h=0.1)


def test_cfg3_conv_fp16_64x64_8192chains(golden):
    """cfg-3 with the reference's default conv network at its real shapes: the
    8192 x 8192 x 51 200 Linear on gemm_h_dma_kernel, the LDS-patch and gather conv kernels on
    8192 x 64 x 64 images, 16-bit max-pool (nleapfrog 2: six networks of 1.7 GB each)."""
    free, total = torch.cuda.mem_get_info()
    if total < 100 * 2 ** 30:
        pytest.skip('needs > 100 GB of HBM')
    g = golden('u1_cfg3_fp16_conv')
    yard = float(np.abs(g['acc'] - g['acc_fp32']).max())
    _u1_full_size(golden, 'u1_cfg3_fp16_conv', 8192, tol_x=5e-3, tol_acc=max(3 * yard, 5e-3),
                  tol_h=0.1)
