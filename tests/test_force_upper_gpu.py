"""The upper-plane SU(3) force (include/l2q.h: l2q_su3_force_upper) and its two readers.  The force is anti-Hermitian,
so the sampler's force kernel stores six of its nine planes, and the digit projection and the int8-sliced heads kernel
read that form.  Everything here is BITWISE against the full field: the six planes of the force, the plaquette sum of
the action variant, the bytes of the projection's digit image (and its out-of-range flag), every output of the heads
kernel, and a whole trajectory with `dyn.upper_plane_force` on and off -- from a cold start (F = 0 everywhere: the
sign-of-zero case) and from a hot one."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LATTICES = [(4, 4, 4, 4), (4, 4, 4, 8)]          # V = 256 (in-LDS mask 7) and 512 (mask 6)
IDS = ['4x4x4x4', '4x4x4x8']
UP = [0, 4, 8, 1, 2, 5]                          # the stored planes, in order


@pytest.fixture(scope='module')
def ops():
    from l2hmc import _ops
    return _ops


def bits(t):
    return torch.view_as_real(t).contiguous().view(torch.int64) if t.is_complex() else t.contiguous().view(torch.int64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


_LINKS = {}


def links(L, nb):
    """random NON-unitary links in the native layout (the force kernel takes any matrices), made once per shape"""
    if (L, nb) not in _LINKS:
        g = torch.Generator(device='cuda').manual_seed(101 + nb + L[3])
        V = int(np.prod(L))
        re, im = (torch.randn((nb, 4, 9, V), dtype=torch.float64, device='cuda', generator=g) for _ in range(2))
        _LINKS[(L, nb)] = torch.complex(re, im)
    return _LINKS[(L, nb)]


@pytest.mark.parametrize('nb', [2, 3])
@pytest.mark.parametrize('L', LATTICES, ids=IDS)
def test_force_upper_has_the_bits_of_the_six_planes(ops, L, nb):
    xn = links(L, nb)
    full = ops.su3_force_n(xn, 5.7, L)
    up, none = ops.su3_force_upper_n(xn, 5.7, L)
    assert none is None and up.buf.shape == (nb, 4, 6, xn.shape[-1])
    assert same(up.buf, full[:, :, UP])
    assert float(full.abs().max()) > 1.0
    # the real diagonal is a signed zero in both; the three planes that are not stored are the images of the others
    assert same(up.full(), full)
    fa, plaq = ops.su3_force_action_n(xn, 5.7, L)
    ua, uplaq = ops.su3_force_upper_n(xn, 5.7, L, want_plaq=True)
    assert same(fa, full) and same(ua.buf, up.buf)
    assert same(uplaq, plaq) and float(plaq.abs().max()) > 0


@pytest.mark.parametrize('L', LATTICES, ids=IDS)
def test_projection_from_six_planes_has_the_bytes_of_the_full_field(ops, L):
    nb, n = 64, 64
    V = int(np.prod(L))
    up, _ = ops.su3_force_upper_n(links(L, 3).repeat(22, 1, 1, 1)[:nb].contiguous(), 5.7, L)
    img_f, img_u = ops.su3_projsu_digits_n(up.full()), ops.su3_projsu_digits_n(up)
    assert img_u.shape == img_f.shape == (nb, 32 * V) and img_u.exp == img_f.exp
    assert torch.equal(img_u.buf, img_f.buf)
    # one link out of range and one NaN: the same bytes, and the flag poisons the next layer once on either route
    g = torch.Generator(device='cuda').manual_seed(3)
    w = (torch.rand((n, 32 * V), dtype=torch.float64, device='cuda', generator=g) * 2 - 1) / np.sqrt(32 * V)
    b = 0.1 * torch.randn(n, dtype=torch.float64, device='cuda', generator=g)
    wimg = ops.gemm_sliced_build(w)
    clean = ops.gemm_digits(img_u, wimg, n, b, act='tanh')
    assert bool(torch.isfinite(clean).all())
    bad = ops.UpperForce(up.buf.clone())
    bad.buf[5, 2, :, 17] *= 1e200
    bad.buf[9, 1, 4, 33] = complex(float('nan'), 0.25)
    ib_f, ib_u = ops.su3_projsu_digits_n(bad.full()), ops.su3_projsu_digits_n(bad)
    assert torch.equal(ib_u.buf, ib_f.buf)
    assert bool(torch.isnan(ops.gemm_digits(ib_u, wimg, n, b, act='tanh')).all())
    assert torch.equal(ops.gemm_digits(img_u, wimg, n, b, act='tanh'), clean)       # (the flag is taken: clean again)
    for src in (bad, bad.full()):                    # each route raises it by itself
        img = ops.su3_projsu_digits_n(src)
        assert bool(torch.isnan(ops.gemm_digits(img, wimg, n, b, act='tanh')).all())
        assert torch.equal(ops.gemm_digits(img_u, wimg, n, b, act='tanh'), clean)
    # a field of zeros (the force of a cold start): +0 in every stored real part; whatever the projection makes of a
    # singular matrix, it makes the same of it on both routes (the layer call takes the flag it may have raised)
    zero = ops.UpperForce(torch.zeros_like(up.buf))
    assert torch.equal(ops.su3_projsu_digits_n(zero).buf, ops.su3_projsu_digits_n(zero.full()).buf)
    ops.gemm_digits(img_u, wimg, n, b, act='tanh')
    assert torch.equal(ops.gemm_digits(img_u, wimg, n, b, act='tanh'), clean)


_HEADS = {}


def heads_for(ops, L, k=256):
    """per-entry-scaled head weights [36 V, 256] with their slice image, made once per lattice"""
    if L not in _HEADS:
        n = 36 * int(np.prod(L))
        g = torch.Generator(device='cuda').manual_seed(7 + L[3])
        rnd = lambda *s: torch.randn(s, dtype=torch.float64, device='cuda', generator=g)
        sl = {}
        for nm in 'stq':
            w = (torch.rand((n, k), dtype=torch.float64, device='cuda', generator=g) * 2 - 1) / 16
            sl[nm] = (w, 0.1 * rnd(n), None if nm == 't' else torch.exp(0.3 * rnd(n)))
        sl['sliced'] = ops.heads_sliced_build(sl)
        _HEADS[L] = sl
    return _HEADS[L]


@pytest.mark.parametrize('m', [3, 70])
@pytest.mark.parametrize('L', LATTICES, ids=IDS)
def test_sliced_heads_read_the_upper_plane_force(ops, L, m):
    sl = heads_for(ops, L)
    assert sl['sliced'] is not None and ops.USE_SLICED_HEADS[0]
    n, k = 36 * int(np.prod(L)), 256
    g = torch.Generator(device='cuda').manual_seed(11 * m)
    rnd = lambda *s: torch.randn(s, dtype=torch.float64, device='cuda', generator=g)
    z = torch.tanh(rnd(m, k))
    v = torch.complex(rnd(m, n), rnd(m, n))
    xn = links(L, 3).repeat(24, 1, 1, 1)[:m].contiguous()
    xn = xn * torch.linspace(0.5, 1.5, m, dtype=torch.float64, device='cuda').reshape(m, 1, 1, 1)   # (distinct chains)
    up, _ = ops.su3_force_upper_n(xn, 5.7, L)
    f = ops.su3_force_n(xn, 5.7, L).reshape(m, -1)
    assert ops.heads_take_upper_force(sl)
    nw = (0.9, 1.1, 0.8)

    def both(call):
        res = []
        for force in (f, up):
            vv = v.clone()
            out = call(vv, force)
            res.append([vv] + [o for o in (out if isinstance(out, tuple) else (out,))])
        assert len(res[0]) == len(res[1])
        for a, b in zip(*res):
            assert same(a, b)
        assert bool(torch.isfinite(res[1][0]).all()) and not same(res[1][0], v)
        return res[1]

    both(lambda vv, force: ops.vnet_heads_vupdate_(z, sl, nw, vv, force, 0.07, True))               # single forward

    def single_backward_norm2(vv, force):
        got = []
        ld = ops.vnet_heads_vupdate_(z, sl, nw, vv, force, 0.07, False, v_src=v.clone(), norm2=got)
        assert len(got) == 1
        return ld, got[0]
    both(single_backward_norm2)
    both(lambda vv, force: ops.vnet_heads_vupdate_pair_(z, sl, nw, vv, force, 0.07, True, False, 0.05, True))
    both(lambda vv, force: ops.vnet_heads_vupdate_pair_(z, sl, nw, vv, force, 0.07, True, True, 0.07, False))
    ld, ld1, n2 = both(lambda vv, force: ops.vnet_heads_vupdate_pair_mid_(z, sl, nw, vv, force, 0.07, False, True,
                                                                          0.05, True))[1:]
    assert float(ld.abs().max()) > 0 and float(ld1.abs().max()) > 0 and float(n2.min()) > 0
    # F = 0 (a cold start): the rebuilt planes read -0 where the full field holds +0, and t != 0 absorbs it
    zero = ops.UpperForce(torch.zeros_like(up.buf))
    f, up = zero.full().reshape(m, -1), zero
    assert same(f, torch.zeros_like(f))
    both(lambda vv, force: ops.vnet_heads_vupdate_pair_(z, sl, nw, vv, force, 0.07, True, True, 0.07, False))
    # the fp64 heads kernels read the full field only: an upper-plane force there is an error, not a wrong answer
    from l2hmc import native
    fp = {nm: sl[nm] for nm in 'stq'}
    with pytest.raises(native.L2QError):
        ops.vnet_heads_vupdate_(z, fp, nw, v.clone(), up, 0.07, True)


def build(nb, L):
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.network.pytorch.network import NetworkFactory
    torch.manual_seed(0)
    np.random.seed(0)
    V = int(np.prod(L))
    dc = cfgs.DynamicsConfig(nchains=nb, group='SU3', latvolume=list(L), nleapfrog=2, eps=0.02, eps_hmc=0.02,
                             verbose=False, use_split_xnets=False, use_separate_networks=False)
    spec = cfgs.InputSpec(xshape=tuple(dc.xshape), xnet={'x': [32 * V], 'v': [32 * V]},
                          vnet={'x': [32 * V], 'v': [32 * V]})
    nc = cfgs.NetworkConfig(units=[256], activation_fn='tanh', dropout_prob=0.0, use_batch_norm=False)
    lat = LatticeSU3(nb, list(L))
    dyn = Dynamics(lat.action, dc, NetworkFactory(spec, nc, cfgs.ConvolutionConfig())).cuda().eval()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():                            # (ScaledTanh coefficients start at 0: s = q = 0 without this)
        for n_, p in dyn.vnet.named_parameters():
            if n_.endswith('coeff'):
                p.copy_(0.3 * torch.randn(p.shape, generator=g, dtype=torch.float64).to(p.device))
    return dyn, lat


@pytest.fixture
def launches(monkeypatch):
    """the entry points of libl2q.so in the order they are called; the size rule of the sliced layers lifted (a 4^4
    lattice takes them, as in test_sampler_step_gpu.py)"""
    from l2hmc import _ops
    from l2hmc import native
    monkeypatch.setattr(_ops, 'gemm_sliced_pays', _ops.gemm_sliced_ok)
    names = []

    def call(name, *args, _call=native.call):
        names.append(name.removeprefix('l2q_'))
        return _call(name, *args)
    monkeypatch.setattr(native, 'call', call)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield names
    torch.set_default_dtype(old)


NEW = {'su3_force': 'su3_force_upper', 'su3_force_action': 'su3_force_action_upper',
       'su3_projsu_digits': 'su3_projsu_digits_upper',
       'vnet_heads_vupdate_sliced_f64': 'vnet_heads_vupdate_sliced_upper_f64'}


@pytest.mark.parametrize('start', ['cold', 'hot'])
def test_trajectory_with_the_upper_plane_force_on_and_off(launches, start):
    L, nb = (4, 4, 4, 4), 64
    dyn, lat = build(nb, L)
    assert dyn.upper_plane_force is True
    if start == 'cold':                              # x = 1: F = 0 everywhere, the sign-of-zero case
        x = torch.eye(3, dtype=torch.complex128, device='cuda').expand(nb, 4, *L, 3, 3).contiguous()
    else:
        x = lat.g.compat_proj(lat.random().cuda())
    torch.cuda.manual_seed(3)
    dyn((x, 6.0))                                    # (the first trajectory of a module builds the weight images)
    got = {}
    for on in (False, True, False):
        dyn.upper_plane_force = on
        torch.cuda.manual_seed(7)
        del launches[:]
        xo, m = dyn((x, 6.0))
        res = ({'x_out': xo.clone(), **{k: m[k].clone() for k in ('acc', 'acc_mask', 'sumlogdet')}}, list(launches))
        if on in got:
            assert res[1] == got[on][1] and all(same(res[0][k], got[on][0][k]) for k in res[0])
        got[on] = res
    (off, seq_off), (on, seq_on) = got[False], got[True]
    for k in off:
        assert same(on[k], off[k]), k
    if start == 'hot':       # (a cold start has F = 0, whose projection is not a number on either route: equal bits)
        assert bool(torch.isfinite(on['acc']).all()) and float(on['sumlogdet'].abs().max()) > 0
    # the new entries stand where the old ones stood: the same number of launches, nothing else moved
    assert not set(NEW.values()) & set(seq_off)
    assert len(seq_on) == len(seq_off) and [NEW.get(n, n) for n in seq_off] == seq_on
    for name in NEW.values():
        assert name in seq_on, name
    assert seq_on.count('su3_force_upper') + seq_on.count('su3_force_action_upper') == 2 * 2 + 1
