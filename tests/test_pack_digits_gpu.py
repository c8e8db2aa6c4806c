"""The trajectory's fused entry, l2q_su3_pack_digits (csrc/su3_kernels.hip): from one read of the reference-layout
field it writes the native planes -- the bits of l2q_su3_pack -- and the digit image of su3_to_vec(projectSU(x))
-- the bytes of l2q_su3_projsu_digits on those planes; it raises the producers' out-of-range flag as they do,
refuses what the projection refuses, and a trajectory that enters through it computes what it computed before."""
import numpy as np
import pytest
import torch

from oracle import su3 as osu3

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from l2hmc import _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def field(rng, nb, L, noise=0.05):
    """general matrices near SU(3): the projection has work to do"""
    shape = (nb, 4, *L, 3, 3)
    x = osu3.project_su(rng.normal(size=shape) + 1j * rng.normal(size=shape))
    return x + noise * (rng.normal(size=shape) + 1j * rng.normal(size=shape))


# V = 64: one wavefront of a 256-thread block holds sites, the other three only wait; the 64-site tile spans both
# t-slices (32 sites each).  V = 256: one whole block, four t-slices.  V = 576: three blocks, the last a quarter
# full, tiles that straddle the 72-site t-slices.
@pytest.mark.parametrize('L', [(2, 2, 4, 4), (4, 4, 4, 4), (8, 2, 6, 6)], ids=['V64', 'V256', 'V576'])
@pytest.mark.parametrize('nb', [1, 3, 5])
def test_planes_and_image_equal_the_two_launches(ops, L, nb):
    rng = np.random.default_rng(11 + nb)
    x = dev(field(rng, nb, L))
    xn = ops.su3_pack(x)
    img = ops.su3_projsu_digits_n(xn)
    got = ops.su3_pack_digits(x)
    assert got is not None and img is not None
    gn, gi = got
    assert gn.shape == xn.shape and gn.dtype == xn.dtype
    assert torch.equal(torch.view_as_real(gn).view(torch.int64), torch.view_as_real(xn).view(torch.int64))
    assert gi.shape == img.shape and gi.exp == img.exp and gi.buf.shape == img.buf.shape
    assert torch.equal(gi.buf, img.buf)
    # not all zero: the comparison above saw digits
    assert int(gi.buf.count_nonzero()) > gi.buf.numel() // 2


def test_flag_raised_as_the_other_producers_raise_it(ops):
    """the flag is read (and cleared) by the reduce of the next sliced layer: its output is NaN once"""
    rng = np.random.default_rng(9)
    L, nb, n = (2, 2, 4, 4), 64, 64
    V = int(np.prod(L))
    w = dev(rng.uniform(-1, 1, size=(n, 32 * V)) / np.sqrt(32 * V))
    wimg = ops.gemm_sliced_build(w)
    b = dev(0.1 * rng.normal(size=n))

    def layer(x, a_exp=2):
        return ops.gemm_digits(ops.su3_pack_digits(dev(x), a_exp)[1], wimg, n, b, act='tanh')

    good = field(rng, nb, L)
    clean = layer(good)
    assert bool(torch.isfinite(clean).all())
    assert torch.equal(clean, ops.gemm_digits(ops.su3_projsu_digits_n(ops.su3_pack(dev(good))), wimg, n, b, act='tanh'))
    # a NaN entry of one link
    bad = good.copy()
    bad[5, 2, 1, 0, 3, 1, 1, 2] = complex(float('nan'), 0.0)
    assert bool(torch.isnan(layer(bad)).all())
    assert torch.equal(layer(good), clean)
    # one link whose vec8 leaves the declared range: operand exponent 0 serves |v| < 1; links exp(i 0.1 lambda_1)
    # have vec8 = (0, -2 sin 0.1, 0, ...) inside it, the planted exp(i 0.8 lambda_1) has -2 sin 0.8 = -1.43
    def rot(t):
        m = np.eye(3, dtype=complex)
        m[0, 0] = m[1, 1] = np.cos(t)
        m[0, 1] = m[1, 0] = 1j * np.sin(t)
        return m
    small = np.broadcast_to(rot(0.1), (nb, 4, *L, 3, 3)).copy()
    assert bool(torch.isfinite(layer(small, 0)).all())
    planted = small.copy()
    planted[63, 3, 1, 1, 3, 3] = rot(0.8)
    assert bool(torch.isnan(layer(planted, 0)).all())
    assert bool(torch.isfinite(layer(small, 0)).all())
    assert bool(torch.isfinite(layer(planted, 2)).all())


def test_refusals_return_error_codes_without_a_launch(ops):
    from l2hmc import native
    lib = native.load()
    EINVAL, ESHAPE = -1, -2
    x = torch.zeros(1, 4, 64, 3, 3, dtype=torch.complex128, device='cuda')
    xn = torch.full((1, 4, 9, 64), 7.0, dtype=torch.complex128, device='cuda')
    buf = torch.full((1, 32, 7, 64), 7, dtype=torch.uint8, device='cuda')
    raw = torch.zeros(4096 + 64, dtype=torch.uint8, device='cuda')
    p, pn, pi = x.data_ptr(), xn.data_ptr(), buf.data_ptr()
    f = lib.l2q_su3_pack_digits
    for args, code, word in (((None, pn, pi, 2, 1, 64), EINVAL, b'x_ref'),
                             ((p, None, pi, 2, 1, 64), EINVAL, b'x_nat'),
                             ((p, pn, None, 2, 1, 64), EINVAL, b'image'),
                             ((p, p, pi, 2, 1, 64), EINVAL, b'alias'),
                             ((p, pn, pi, 2, 0, 64), EINVAL, b'V'),
                             ((p, pn, pi, 2, 1, 48), EINVAL, b'V % 64'),
                             ((p, pn, pi, 2, 1, 96), EINVAL, b'V % 64'),
                             ((p, pn, pi, 2, 1, 65), EINVAL, b'V % 64'),
                             ((p, pn, pi, 2, 1, 0), EINVAL, b'V'),
                             ((p, pn, pi, 1000, 1, 64), EINVAL, b'a_exp'),
                             ((p, pn, pi, -1000, 1, 64), EINVAL, b'a_exp'),
                             ((p, pn, raw.data_ptr() + 8, 2, 1, 64), ESHAPE, b'image'),
                             ((p + 8, pn, pi, 2, 1, 64), ESHAPE, b'x_ref'),
                             ((p, pn + 8, pi, 2, 1, 64), ESHAPE, b'x_nat')):
        assert f(*args, None) == code, args
        assert word in lib.l2q_last_error(), (args, lib.l2q_last_error())
    torch.cuda.synchronize()
    assert bool((xn == 7.0).all()) and bool((buf == 7).all())          # nothing ran
    assert native.kernel_name('l2q_su3_pack_digits', (4, 4, 4, 4)) == 'su3_pack_digits_kernel'
    # the Python wrapper declines a lattice the image does not serve, as su3_projsu_digits_n does
    assert ops.su3_pack_digits(torch.zeros(2, 4, 2, 2, 2, 6, 3, 3, dtype=torch.complex128, device='cuda')) is None


def build(nb, units):
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch.dynamics import Dynamics
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.network.pytorch.network import NetworkFactory
    L = (4, 4, 4, 4)
    torch.manual_seed(0)
    np.random.seed(0)
    V = int(np.prod(L))
    dc = cfgs.DynamicsConfig(nchains=nb, group='SU3', latvolume=list(L), nleapfrog=2, eps=0.02, eps_hmc=0.02,
                             verbose=False, use_split_xnets=False, use_separate_networks=False)
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
    return dyn, lat.g.compat_proj(lat.random().cuda())


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


def outputs(xo, m):
    st = m['mc_states']
    out = {'x': xo, **{k: v for k, v in m.items() if isinstance(v, torch.Tensor)}}
    for name, s in (('init', st.init), ('proposed', st.proposed), ('out', st.out)):
        out[name + '.x'], out[name + '.v'] = s.x, s.v
    return {k: v.clone() for k, v in out.items()}


# 4 chains: the sliced input layer serves whole 64-row tiles, so this trajectory carries fp64 network inputs and the
# fused entry must stand aside (the pack and the projection stay two launches).  64 chains: digit inputs, the
# configuration the fused entry is for.
@pytest.mark.parametrize('nb,fused', [(4, False), (64, True)], ids=['4chains', '64chains'])
def test_trajectory_with_the_fused_entry_on_and_off(launches, nb, fused):
    dyn, x = build(nb, [256])
    torch.cuda.manual_seed(3)
    dyn((x, 6.0))                                    # (the first trajectory of a module builds the weight images)
    got = {}
    for on in (False, True, False):
        dyn.fuse_entry_digits = on
        torch.cuda.manual_seed(7)
        del launches[:]
        xo, m = dyn((x, 6.0))
        seq = list(launches)                         # (before the lazy states are read: they launch their unpacks)
        res = (outputs(xo, m), seq)
        if on in got:
            assert res[1] == got[on][1]
            assert all(torch.equal(res[0][k], got[on][0][k]) for k in res[0])
        got[on] = res
    (off, seq_off), (on, seq_on) = got[False], got[True]
    assert sorted(on) == sorted(off) and len(on) >= 10
    for k in off:
        a, b = on[k], off[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert torch.equal(a, b), k
    assert bool(torch.isfinite(on['acc']).all()) and float(on['sumlogdet'].abs().max()) > 0
    assert seq_off[0] == 'su3_pack' and seq_off.count('su3_pack') == 1
    if not fused:
        assert seq_on == seq_off and 'su3_projsu_digits' not in seq_off
        return
    # the entry replaces the pack and the one projection of x that the first v-update asked for (the first
    # su3_projsu_digits of the sequence; the one after it is the force's); everything else runs as before, in order
    assert seq_on[0] == 'su3_pack_digits' and 'su3_pack' not in seq_on
    rest = seq_off[1:]
    rest.remove('su3_projsu_digits')
    assert seq_on[1:] == rest
    assert seq_off.count('su3_projsu_digits') == seq_on.count('su3_projsu_digits') + 1
