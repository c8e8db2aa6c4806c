"""GPU parity tests of the individual HIP kernels (through the C ABI) against the numpy
oracle and the golden vectors generated from the reference."""
import numpy as np
import pytest
import torch

from oracle import su3 as osu3, u1 as ou1, network as onet

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from l2hmc import _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def err(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())


def test_pack_roundtrip(ops):
    rng = np.random.default_rng(1)
    L = (3, 2, 5, 4)
    x = rng.normal(size=(2, 4, *L, 3, 3)) + 1j * rng.normal(size=(2, 4, *L, 3, 3))
    xn = ops.su3_pack(dev(x))
    ref = np.moveaxis(x.reshape(2, 4, -1, 9), 2, 3)
    assert err(host(xn), ref) == 0.0
    assert err(host(ops.su3_unpack(xn, L)), x) == 0.0
    a = rng.normal(size=(2, 4 * 120 * 9))
    an = ops.pack_entries(dev(a), 120)
    idx = host(ops.native_index(120, 9, 'cuda'))
    assert err(host(an), a[:, idx]) == 0.0
    assert err(host(ops.unpack_entries(an, 120)), a) == 0.0
    m = rng.integers(0, 2, size=(1, 4 * 120 * 9)).astype(np.float32)
    assert err(host(ops.pack_entries(dev(m), 120)), m[:, idx]) == 0.0


def test_su3_ops_golden(ops, golden):
    g = golden('su3_ops')
    L = tuple(int(i) for i in g['latvolume'])
    V = int(np.prod(L))
    beta = float(g['beta'])
    xn = ops.su3_pack(dev(g['x']))
    vn = ops.su3_pack(dev(g['v']))
    s = host(ops.su3_plaq_sums_n(xn, L))
    assert err(-(beta / 3) * s[:, 0], g['action']) < 1e-10
    assert err(s[:, 0] / (18 * V), g['plaqs']) < 1e-14
    assert err(s[:, 1] / (18 * V), g['sinQ']) < 1e-14
    assert err(s[:, 1] / (32 * np.pi ** 2), g['intQ']) < 1e-13
    fn = ops.su3_force_n(xn, beta, L)
    assert err(host(ops.su3_unpack(fn, L)), g['force']) < 1e-13
    assert err(host(ops.su3_kinetic_n(vn)), g['kinetic']) < 1e-10
    nrm = dev(g['normals'].reshape(8, 2, 4, V))
    assert err(host(ops.su3_unpack(ops.su3_assemble_tah_n(nrm), L)), g['v']) < 1e-15
    e = ops.su3_expm_mul_n(xn, vn, float(g['eps_expm']))
    assert err(host(ops.su3_unpack(e, L)), g['expm_v_x']) < 1e-13
    # general (non anti-Hermitian) matrices: expm, projectSU, projectTAH, su3_to_vec
    gen = g['general']                                # [4, 7, 3, 3]
    nlinks = gen.shape[0] * gen.shape[1]
    pad = np.zeros((1, 4, nlinks, 3, 3), complex)
    pad[0, :] = gen.reshape(1, nlinks, 3, 3)
    gn = ops.su3_pack(dev(pad))
    eye = np.zeros_like(pad); eye[..., range(3), range(3)] = 1
    eg = ops.su3_expm_mul_n(ops.su3_pack(dev(eye)), gn, 1.0)
    got = host(eg).reshape(4, 3, 3, nlinks)[0].transpose(2, 0, 1).reshape(gen.shape)
    assert err(got, g['expm_general']) < 1e-11
    ps = host(ops.su3_project_su_n(gn)).reshape(4, 3, 3, nlinks)[0].transpose(2, 0, 1)
    assert err(ps.reshape(gen.shape), g['projsu_general']) < 1e-12
    pt = host(ops.su3_project_tah_n(gn)).reshape(4, 3, 3, nlinks)[0].transpose(2, 0, 1)
    assert err(pt.reshape(gen.shape), g['tah_general']) < 1e-15
    vx = host(ops.su3_projsu_vec8_n(xn))              # [nb, 4, 8, V]
    assert err(np.moveaxis(vx, 2, 3).reshape(g['vec_x'].shape), g['vec_x']) < 1e-12
    vf = host(ops.su3_projsu_vec8_n(fn))
    # ill-conditioned in the reference itself (see tests/test_oracle_golden.py)
    assert err(np.moveaxis(vf, 2, 3).reshape(g['vec_force'].shape), g['vec_force']) < 1e-7
    chk = host(ops.su3_check_su_n(xn))
    assert err(chk.T, g['checksu_x']) < 1e-14
    # one HMC leapfrog step with the fused kick
    v1 = vn.clone()
    ops.su3_force_kick_n(xn, beta, -0.5 * 0.05, v1, L)
    x1 = ops.su3_expm_mul_n(xn, v1, 0.05)
    ops.su3_force_kick_n(x1, beta, -0.5 * 0.05, v1, L)
    assert err(host(ops.su3_unpack(x1, L)), g['hmc_x1']) < 1e-13
    assert err(host(ops.su3_unpack(v1, L)), g['hmc_v1']) < 1e-12


@pytest.mark.parametrize('L', [(2, 2, 2, 2), (1, 3, 2, 5), (4, 4, 4, 4), (3, 5, 2, 7), (2, 2, 8, 8),
                               (3, 2, 4, 16), (3, 8, 8, 8), (2, 4, 8, 16), (1, 2, 8, 8),
                               (2, 4, 4, 12), (2, 16, 4, 4), (5, 4, 4, 4), (2, 2, 2, 32), (4, 3, 8, 8)])
def test_su3_stencils_vs_oracle(ops, L):
    """edge shapes: extent 1 and 2 (forward == backward neighbour), odd sizes, V not a
    multiple of the block size."""
    rng = np.random.default_rng(7)
    nb = 3
    x = osu3.project_su(rng.normal(size=(nb, 4, *L, 3, 3)) + 1j * rng.normal(size=(nb, 4, *L, 3, 3)))
    xn = ops.su3_pack(dev(x))
    re, im = osu3.plaq_sums(x)
    s = host(ops.su3_plaq_sums_n(xn, L))
    assert err(s, np.stack([re, im], 1)) < 1e-10
    f = host(ops.su3_unpack(ops.su3_force_n(xn, 5.7, L), L))
    assert err(f, osu3.grad_action(x, 5.7)) < 1e-12
    from l2hmc import native
    # every force kernel design, with and without the XCD remap, must give the same numbers.  The plaquette runs
    # the slice kernel where X Y Z % 128 == 0 and the flat kernel elsewhere, whatever the force design.
    # force_tile 7 = plaquettes shared between their four links, one 8-wavefront workgroup per CU, su3_force_plaq.hip
    # (plain force only): taken where the (y, z) plane is the 64-site tile and T >= 2 -- (3,8,8,8), (2,2,8,8),
    # (4,3,8,8): x extent 8, 2 (both x neighbours are the same plane) and odd -- and falls back to 5 elsewhere;
    # force_tile 5 (the default) = thread per link with streamed factors, su3_force_link.hip, where X Y Z % 64 == 0;
    # its four tile-residency specialisations -- Z | 64, Y Z | 64, X Y Z | 64, none -- and T = 1 are covered above;
    # force_tile 2 = the slice-resident thread-per-link kernel where X Y Z % 128 == 0.
    # Both 5 and 2 fall back to the LDS-tiled kernel on the other lattices.
    for variant in (2, 5, 7):
        for swz in (0, 1):
            native.set_tuning('force_tile', variant)
            native.set_tuning('xcd_swizzle', swz)
            assert err(host(ops.su3_plaq_sums_n(xn, L)), s) < 1e-10
            assert err(host(ops.su3_unpack(ops.su3_force_n(xn, 5.7, L), L)), f) < 1e-13
            v = xn.clone()
            ops.su3_force_kick_n(xn, 5.7, -0.3, v, L)
            assert err(host(ops.su3_unpack(v, L)), x - 0.3 * f) < 1e-12
            # out of place (l2q_su3_force_kick_to): the same bits, the source untouched
            src = xn.clone(); v2 = torch.full_like(xn, float('nan'))
            ops.su3_force_kick_n(xn, 5.7, -0.3, v2, L, v_src=src)
            assert torch.equal(v2, v) and torch.equal(src, xn)
    native.set_tuning('force_tile', 5)
    native.set_tuning('xcd_swizzle', 1)


def test_su3_cold_start(ops):
    L = (4, 2, 6, 2)
    x = np.zeros((2, 4, *L, 3, 3), complex); x[..., range(3), range(3)] = 1
    V = int(np.prod(L))
    xn = ops.su3_pack(dev(x))
    s = host(ops.su3_plaq_sums_n(xn, L))
    assert np.allclose(s[:, 0], 18 * V) and np.allclose(s[:, 1], 0)
    assert float(ops.su3_force_n(xn, 6.0, L).abs().max()) == 0.0
    assert np.allclose(host(ops.su3_kinetic_n(torch.zeros_like(xn))), -0.5 * 8 * 4 * V)


def test_expm_mul_masked(ops, golden):
    g = golden('su3_l2hmc')
    L = tuple(int(i) for i in g['latvolume'])
    V = int(np.prod(L))
    xn = ops.su3_pack(dev(g['x']))
    vn = ops.su3_pack(dev(g['v_fwd']))
    eps = float(g['xeps'][0]); eps = eps / (1 + eps)
    m = ops.pack_entries(dev(g['masks'][0:1]), V).reshape(-1)
    got = ops.su3_expm_mul_n(xn, vn, eps, m, False)
    assert err(host(ops.su3_unpack(got, L)), g['x_fwd']) < 1e-13
    eps1 = float(g['xeps'][1]); eps1 = eps1 / (1 + eps1)
    got = ops.su3_expm_mul_n(xn, vn, -eps1, m, True)     # keeps (1 - m)
    assert err(host(ops.su3_unpack(got, L)), g['x_bwd']) < 1e-13


def test_expm_mul2_vec8(ops, golden):
    """l2q_su3_expm_mul2_vec8 == l2q_su3_expm_mul2 followed by l2q_su3_projsu_vec8, and both
    against the reference's two half-updates / su3_to_vec(projectSU(.)) via the oracle."""
    from oracle import su3 as osu3
    g = golden('su3_l2hmc')
    L = tuple(int(i) for i in g['latvolume'])
    V = int(np.prod(L))
    xn = ops.su3_pack(dev(g['x']))
    vn = ops.su3_pack(dev(g['v_fwd']))
    eps = 0.037
    m = ops.pack_entries(dev(g['masks'][0:1]), V).reshape(-1)
    for comp in (False, True):
        x2 = ops.su3_expm_mul2_n(xn, vn, eps, m, comp)
        v8 = ops.su3_projsu_vec8_n(x2)
        xf, vf = ops.su3_expm_mul2_vec8_n(xn, vn, eps, m, comp)
        assert err(host(xf), host(x2)) < 1e-15
        assert err(host(vf), host(v8)) < 1e-13
        m4 = g['masks'][0].reshape(1, 4, *L, 3, 3)
        keep = (1 - m4) if comp else m4
        e = osu3.expm(eps * g['v_fwd'])
        y = keep * g['x'] + e @ ((1 - keep) * g['x'])
        y = (1 - keep) * y + e @ (keep * y)
        assert err(host(ops.su3_unpack(xf, L)), y) < 1e-13
        ref = np.moveaxis(osu3.group_to_vec(y).reshape(y.shape[0], 4, V, 8), -1, -2)
        assert err(host(vf), ref) < 1e-11
    # in place (out aliases xn), as the trajectory calls it
    xc = xn.clone()
    xo, vo = ops.su3_expm_mul2_vec8_n(xc, vn, eps, m, True, out=xc)
    assert xo.data_ptr() == xc.data_ptr() and err(host(xo), host(xf)) == 0.0 and err(host(vo), host(vf)) == 0.0


def test_v_update_su3(ops, golden):
    g = golden('su3_l2hmc')
    L = tuple(int(i) for i in g['latvolume'])
    V = int(np.prod(L))
    vn = ops.su3_pack(dev(g['v0']))
    fn = ops.su3_pack(dev(g['force0']))
    s, t, q = (ops.pack_entries(dev(g[k]), V) for k in ('s', 't', 'q'))
    eps = float(g['veps'][0]); eps = eps / (1 + eps)
    v = vn.clone()
    ld = ops.v_update_(v, fn, s, t, q, eps, True)
    assert err(host(ops.su3_unpack(v, L)), g['v_fwd']) < 1e-13
    assert err(host(ld), g['logdet_v_fwd']) < 1e-12


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('shape', [(3, 5, 40, 0), (128, 96, 700, 36), (257, 130, 4100, 0),
                                   (2, 300, 16, 16), (130, 1000, 6, 0)])
def test_gemm(ops, dtype, shape):
    m, n, k, k2 = shape
    rng = np.random.default_rng(5)
    a = rng.normal(size=(m, k)).astype(dtype); w = (rng.normal(size=(n, k)) / np.sqrt(k)).astype(dtype)
    b = rng.normal(size=n).astype(dtype); co = (0.3 * rng.normal(size=n)).astype(dtype)
    a2 = w2 = b2 = None
    ref = a.astype(np.float64) @ w.astype(np.float64).T + b
    if k2:
        a2 = rng.normal(size=(m, k2)).astype(dtype); w2 = rng.normal(size=(n, k2)).astype(dtype)
        b2 = rng.normal(size=n).astype(dtype)
        ref = ref + a2.astype(np.float64) @ w2.astype(np.float64).T + b2
    tol = 1e-12 if dtype == np.float64 else 2e-4
    for act in (None, 'tanh', 'leaky_relu', 'elu', 'swish', 'relu'):
        want = 0.7 * np.exp(co) * onet.act(act, ref) if act else 0.7 * np.exp(co) * ref
        got = ops.gemm(dev(a), dev(w), dev(b), a2=None if a2 is None else dev(a2),
                       w2=None if w2 is None else dev(w2), bias2=None if b2 is None else dev(b2),
                       coeff=dev(co), scale=0.7, act=act)
        assert err(host(got), want) < tol * max(1.0, np.abs(want).max()), (act, shape)
    got = ops.gemm(dev(a), dev(w))
    assert err(host(got), a.astype(np.float64) @ w.astype(np.float64).T) < tol * 10


@pytest.mark.parametrize('L', [(32, 32), (64, 64), (16, 64), (64, 36), (24, 44)])
def test_u1_force_staged_f32_vs_oracle(ops, L):
    """fp32 lattices of 1024 .. 4096 sites with X % 4 == 0 take the LDS-staged force kernel (float4 rows in and
    out); (24, 44) stays on the scalar kernel.  Force and the fused kick v += coef F against the oracle."""
    from oracle import u1 as ou1
    rng = np.random.default_rng(5)
    nb = 7
    xh = rng.uniform(-np.pi, np.pi, size=(nb, 2, *L))
    vh = rng.normal(size=(nb, 2, *L))
    want = ou1.grad_action(xh, 3.7).reshape(nb, -1)
    x = torch.from_numpy(xh).float().cuda()
    got = ops.u1_force(x, 3.7, L).reshape(nb, -1)
    assert got.dtype == torch.float32
    assert err(host(got), want) < 2e-5
    v = torch.from_numpy(vh).float().cuda().reshape(nb, -1).clone()
    ops.u1_force_kick_(x, 3.7, -0.07, v, L)
    assert err(host(v), vh.reshape(nb, -1) - 0.07 * want) < 2e-5


@pytest.mark.parametrize('name', ['u1_conv', 'u1_c1'])
def test_u1_ops_golden(ops, golden, name):
    g = golden(name)
    L = tuple(int(i) for i in g['latvolume'])
    V = int(np.prod(L))
    beta = float(g['beta'])
    x = dev(g['x'])
    nb = x.shape[0]
    s = host(ops.u1_plaq_sums(x, L))
    assert err(beta * (V - s[:, 0]), g['action']) < 2e-4
    assert err(s[:, 0] / V, g['plaqs']) < 1e-6
    assert err(s[:, 1] / (2 * np.pi), g['sinQ']) < 1e-5
    assert err(s[:, 2] / (2 * np.pi), g['intQ']) < 1e-5
    assert err(host(ops.u1_force(x, beta, L)), g['force']) < 1e-5
    v = dev(g['normals'].reshape(nb, -1))
    assert err(host(ops.u1_kinetic(v)), g['kinetic']) < 1e-4
    # v update with the golden network heads
    f = ops.u1_force(x, beta, L).reshape(nb, -1)
    sd_eps = float(g['sd.veps.0']); eps = sd_eps / (1 + sd_eps)
    v1 = v.clone()
    ld = ops.v_update_(v1, f, dev(g['vnet_s']), dev(g['vnet_t']), dev(g['vnet_q']), eps, True)
    assert err(host(v1), g['v_fwd']) < 1e-5
    assert err(host(ld), g['logdet_v_fwd']) < 1e-4
    # x update (NCP) forward with mask m, backward with the complement
    xe = float(g['sd.xeps.0']); xeps = xe / (1 + xe)
    m0 = dev(g['masks'][0])
    x1 = x.clone().reshape(nb, -1)
    ld = ops.u1_x_update_(x1, v, dev(g['xnet_s']), dev(g['xnet_t']), dev(g['xnet_q']), m0, False,
                          xeps, True)
    d = np.abs(np.angle(np.exp(1j * (host(x1).reshape(g['x_fwd'].shape) - g['x_fwd']))))
    assert d.max() < 2e-5 and err(host(ld), g['logdet_x_fwd']) < 1e-4
    xm = ops.u1_masked_cos_sin(x, m0, False, L)
    want = ou1.group_to_vec(g['masks'][0].reshape(1, 2, *L) * g['x'])
    assert err(host(xm), want) < 1e-6
    assert err(host(ops.u1_wrap(x * 3)), ou1.compat_proj(g['x'] * np.float32(3))) < 1e-5


def test_conv2d_periodic(ops):
    rng = np.random.default_rng(3)
    x = rng.normal(size=(3, 4, 5, 6)).astype(np.float32)
    for k, pool, act in [(3, 1, None), (2, 2, 'leaky_relu'), (5, 1, 'tanh'), (2, 3, 'relu')]:
        w = rng.normal(size=(7, 4, k, k)).astype(np.float32)
        b = rng.normal(size=7).astype(np.float32)
        want = onet.conv2d_valid(onet.periodic_pad(x, k - 1), w, b)
        if pool > 1:
            want = onet.maxpool2d(want, pool)
        if act:
            want = onet.act(act, want)
        got = host(ops.conv2d_periodic(dev(x), dev(w), dev(b), pool, act))
        assert got.shape == want.shape and err(got, want) < 1e-4
        # implicit-GEMM path (NHWC out), from NCHW and from NHWC input
        g1 = host(ops.conv2d_periodic_gemm(dev(x), 'nchw', dev(w), dev(b), pool, act))
        assert err(g1.transpose(0, 3, 1, 2), want) < 1e-4
        xh = dev(np.ascontiguousarray(x.transpose(0, 2, 3, 1)))
        g2 = host(ops.conv2d_periodic_gemm(xh, 'nhwc', dev(w), dev(b), pool, act))
        assert err(g2.transpose(0, 3, 1, 2), want) < 1e-4


def test_accept_select(ops):
    h0 = dev(np.array([1.0, 2.0, 3.0, -1.0])); h1 = dev(np.array([1.5, 1.0, 3.0, 0.0]))
    sld = dev(np.array([0.1, 0.0, -0.2, 0.0])); u = dev(np.array([0.5, 0.9, 0.9, 0.3]))
    acc, mask = ops.accept(h0, h1, sld, u)
    want = np.exp(np.minimum(0, host(h0) - host(h1) + host(sld)))
    assert err(host(acc), want) < 1e-15
    assert np.array_equal(host(mask), (want > host(u)).astype(np.float32))
    a = dev(np.arange(4 * 6, dtype=np.float64).reshape(4, 6)); b = -a
    out = host(ops.select_rows(a, b, mask))
    assert np.array_equal(out, np.where(host(mask)[:, None] > 0, host(a), host(b)))
    # a diverged chain (H = inf - inf = NaN): acc is NaN like torch.minimum gives, and it is rejected
    for dt in (np.float64, np.float32):
        h0 = dev(np.array([1.0, np.inf, np.nan, 2.0], dtype=dt)); h1 = dev(np.array([1.5, np.inf, 0.0, 1.0], dtype=dt))
        z = dev(np.zeros(4, dtype=dt)); u = dev(np.array([0.1, 0.0, 0.0, 0.5], dtype=dt))
        acc, mask = ops.accept(h0, h1, z, u)
        acc = host(acc)
        assert np.isnan(acc[1]) and np.isnan(acc[2]) and abs(acc[0] - np.exp(-0.5)) < 1e-6 and acc[3] == 1.0
        assert host(mask).tolist() == [1.0, 0.0, 0.0, 1.0]


@pytest.mark.parametrize('cplx', [True, False])
@pytest.mark.parametrize('shape', [(64, 48), (37, 50), (130, 16), (256, 8200), (300, 1000),
                                   # 32 row groups (cfg-2-like chain counts), and more row groups than
                                   # fit the chip at once
                                   (2048, 160), (4160, 64)])
def test_heads_sliced(ops, cplx, shape):
    """The int8-sliced heads + momentum-update kernel (csrc/heads_sliced.hip: fp64 products rebuilt from
    exact int8 slice products on v_mfma_i32_16x16x64_i8) against the fp64 MFMA kernel and against a
    long-double evaluation: as accurate as the fp64 kernel, every variant (in place, out of place, pair,
    pair with mid-point outputs), deterministic."""
    m, n = shape
    k = 256
    rng = np.random.default_rng(5)
    z = dev(np.maximum(rng.normal(size=(m, k)), 0.0))          # relu activations (exact zeros included)
    scaled = {}
    for nm in 'stq':
        w = dev(rng.uniform(-1, 1, size=(n, k)) / 16); b = dev(0.1 * rng.normal(size=n))
        c = None if nm == 't' else dev(np.exp(0.3 * rng.normal(size=n)))
        scaled[nm] = (w, b, c)
    nw = (0.9, 1.1, 0.8)
    if cplx:
        v = dev(rng.normal(size=(m, n)) + 1j * rng.normal(size=(m, n)))
        f = dev(rng.normal(size=(m, n)) + 1j * rng.normal(size=(m, n)))
    else:
        v = dev(rng.normal(size=(m, n))); f = dev(rng.normal(size=(m, n)))
    sl = dict(scaled)
    sl['sliced'] = ops.heads_sliced_build(scaled)
    assert sl['sliced'] is not None
    assert ops.USE_SLICED_HEADS[0]
    L = np.longdouble
    for fwd in (True, False):
        va = v.clone(); la = ops.vnet_heads_vupdate_(z, scaled, nw, va, f, 0.07, fwd)      # fp64 MFMA
        vb = v.clone(); lb = ops.vnet_heads_vupdate_(z, sl, nw, vb, f, 0.07, fwd)          # sliced
        assert float((va - vb).abs().max()) < 2e-14
        assert err(host(la), host(lb)) < 1e-12
        vb2 = v.clone(); lb2 = ops.vnet_heads_vupdate_(z, sl, nw, vb2, f, 0.07, fwd)
        assert torch.equal(vb, vb2) and torch.equal(lb, lb2)                               # deterministic
        if m * n <= 4096:
            # long-double reference of the whole update: the sliced kernel is as close to it as the fp64 one
            zz = host(z).astype(L)
            y = {nm: zz @ host(scaled[nm][0]).astype(L).T + host(scaled[nm][1]).astype(L) for nm in 'stq'}
            s = host(scaled['s'][2]).astype(L) * np.tanh(y['s'])
            q = host(scaled['q'][2]).astype(L) * np.tanh(y['q'])
            t = L(nw[1]) * y['t']
            h = L(0.035)
            es = np.exp(h * s if fwd else -h * s); eq = np.exp(L(0.07) * q)
            hv, hf = host(v), host(f)
            comps = [(hv.real.astype(L), hf.real.astype(L), t)]
            if cplx:
                comps.append((hv.imag.astype(L), hf.imag.astype(L), L(0) * t))
            for ci, (vc, fc, tc) in enumerate(comps):
                want = es * vc - h * (fc * eq + tc) if fwd else es * (vc + h * (fc * eq + tc))
                ga = host(va).real if ci == 0 else host(va).imag
                gb = host(vb).real if ci == 0 else host(vb).imag
                ea = float(np.abs(ga.astype(L) - want).max()); eb = float(np.abs(gb.astype(L) - want).max())
                assert eb < 2.0 * ea + 1e-15, (ea, eb)
        # out of place: the same bits, the source untouched
        v0 = v.clone(); v3 = torch.full_like(v, float('nan'))
        l3 = ops.vnet_heads_vupdate_(z, sl, nw, v3, f, 0.07, fwd, v_src=v0)
        assert torch.equal(v3, vb) and torch.equal(l3, lb) and torch.equal(v0, v)
        for flip in (False, True):
            for fwd2, eps2 in ((True, 0.05), (False, 0.05), (fwd, 0.07)):
                pa = v.clone(); qa = ops.vnet_heads_vupdate_pair_(z, scaled, nw, pa, f, 0.07, fwd, flip, eps2, fwd2)
                pb = v.clone(); qb = ops.vnet_heads_vupdate_pair_(z, sl, nw, pb, f, 0.07, fwd, flip, eps2, fwd2)
                assert float((pa - pb).abs().max()) < 2e-14 and err(host(qa), host(qb)) < 1e-12
                ma = v.clone(); ra = ops.vnet_heads_vupdate_pair_mid_(z, scaled, nw, ma, f, 0.07, fwd, flip, eps2, fwd2)
                mb = v.clone(); rb = ops.vnet_heads_vupdate_pair_mid_(z, sl, nw, mb, f, 0.07, fwd, flip, eps2, fwd2)
                assert torch.equal(mb, pb)
                assert float((ma - mb).abs().max()) < 2e-14
                for xa, xb in zip(ra, rb):
                    assert err(host(xa), host(xb)) < 1e-12 * max(1.0, float(xa.abs().max()))


def test_heads_sliced_edge_cases(ops):
    """what the slice image refuses, and how non-finite inputs travel"""
    rng = np.random.default_rng(6)
    m, n, k = 70, 40, 256
    mk = lambda: {nm: (dev(rng.uniform(-1, 1, size=(n, k)) / 16), dev(0.1 * rng.normal(size=n)),
                       None if nm == 't' else dev(np.ones(n))) for nm in 'stq'}
    # a weight vector dominated by one entry would keep too few bits of the others: refused
    hb = mk()
    hb['q'][0][5, :] *= 1e-9
    hb['q'][0][5, 7] = 1.0
    assert ops.heads_sliced_build(hb) is None
    # other widths and dtypes are not served (the caller keeps the fp64 / fp32 kernels)
    assert ops.heads_sliced_build({nm: (dev(rng.normal(size=(n, 128))), None, None) for nm in 'stq'}) is None
    hd = mk()
    assert ops.heads_sliced_build({nm: (hd[nm][0].float(), None, None) for nm in 'stq'}) is None
    # an image that would take more than its share of the free device memory is not built
    frac = ops.SLICED_IMAGE_MAX_FREE_FRACTION[0]
    try:
        ops.SLICED_IMAGE_MAX_FREE_FRACTION[0] = 0.0
        assert ops.heads_sliced_build(mk()) is None
    finally:
        ops.SLICED_IMAGE_MAX_FREE_FRACTION[0] = frac
    # zero rows / columns are exact; NaN and Inf poison exactly the outputs that use them
    hd = mk()
    hd['t'][0][3, :] = 0.0
    hd['sliced'] = ops.heads_sliced_build(hd)
    assert hd['sliced'] is not None
    z = dev(rng.normal(size=(m, k)))
    z[4, :] = 0.0
    z[9, 17] = float('nan')
    z[11, 200] = float('inf')
    v = dev(rng.normal(size=(m, n))); f = dev(rng.normal(size=(m, n)))
    ref = {nm: hd[nm] for nm in 'stq'}
    va = v.clone(); la = ops.vnet_heads_vupdate_(z, ref, (1.0, 1.0, 1.0), va, f, 0.1, True)
    vb = v.clone(); lb = ops.vnet_heads_vupdate_(z, hd, (1.0, 1.0, 1.0), vb, f, 0.1, True)
    bad = torch.zeros(m, dtype=torch.bool, device=v.device); bad[9] = True; bad[11] = True
    assert bool(torch.isfinite(vb[~bad]).all()) and bool(torch.isfinite(lb[~bad]).all())
    assert not bool(torch.isfinite(vb[bad]).any()) and not bool(torch.isfinite(lb[bad]).any())
    assert float((va[~bad] - vb[~bad]).abs().max()) < 2e-14
    # chain 4 (z = 0): the heads reduce to their biases
    want = (torch.exp(0.05 * torch.tanh(hd['s'][1])) * v[4]
            - 0.05 * (f[4] * torch.exp(0.1 * torch.tanh(hd['q'][1])) + hd['t'][1]))
    assert float((vb[4] - want).abs().max()) < 1e-15
    # scalar scales (no per-entry cs / cq): the call stays on the fp64 kernel even with a slice image
    hsc = {nm: (hd[nm][0], hd[nm][1], None) for nm in 'stq'}
    zc = dev(rng.normal(size=(m, k)))
    v1 = v.clone(); l1 = ops.vnet_heads_vupdate_(zc, hsc, (0.9, 1.1, 0.8), v1, f, 0.1, True)
    hsc['sliced'] = hd['sliced']
    v2 = v.clone(); l2 = ops.vnet_heads_vupdate_(zc, hsc, (0.9, 1.1, 0.8), v2, f, 0.1, True)
    assert torch.equal(v1, v2) and torch.equal(l1, l2)
    # a weight matrix with a non-finite entry poisons that output entry for every chain
    hn = mk()
    hn['s'][0][2, 3] = float('nan')
    hn['sliced'] = ops.heads_sliced_build(hn)
    assert hn['sliced'] is not None
    vc = v.clone(); ops.vnet_heads_vupdate_(dev(rng.normal(size=(m, k))), hn, (1.0, 1.0, 1.0), vc, f, 0.1, True)
    assert not bool(torch.isfinite(vc[:, 2]).any()) and bool(torch.isfinite(vc[:, 3:]).all())


@pytest.mark.parametrize('shape', [(64, 64, 128, 0), (128, 64, 16384 + 128, 192), (64, 128, 64, 64),
                                   (256, 256, 32768, 49152)])
def test_gemm_sliced(ops, shape):
    """The int8-sliced fp64 input layer (csrc/gemm_sliced.hip: digit images of the weights, activations
    sliced on the fly by helper wavefronts) against the fp64 MFMA layer and a long-double evaluation:
    one / several int32 ranges per operand, one / two operands, every epilogue."""
    m, n, k, k2 = shape
    rng = np.random.default_rng(12)
    a = dev(rng.uniform(-2.3, 2.3, size=(m, k)))
    w = dev(rng.uniform(-1, 1, size=(n, k)) / np.sqrt(k))
    a[3, 5] = 0.0
    a[1, 7] = -3.999                                   # inside the declared range (-4, 4)
    b1 = dev(0.1 * rng.normal(size=n)); b2 = dev(0.1 * rng.normal(size=n)) if k2 else None
    a2 = dev(rng.uniform(-2.3, 2.3, size=(m, k2))) if k2 else None
    w2 = dev(rng.uniform(-1, 1, size=(n, k2)) / np.sqrt(k2)) if k2 else None
    img = ops.gemm_sliced_build(w)
    img2 = ops.gemm_sliced_build(w2) if k2 else None
    assert img is not None and (img2 is not None or not k2)
    coeff = dev(0.2 * rng.normal(size=n))
    L = np.longdouble
    rows = [0, 1, 3, m - 1]
    pre = host(a)[rows].astype(L) @ host(w).astype(L).T + host(b1).astype(L)
    if k2:
        pre = pre + host(a2)[rows].astype(L) @ host(w2).astype(L).T + host(b2).astype(L)
    want_pre = None
    for act, co, sc in ((None, None, 1.0), ('tanh', None, 1.0), ('leaky_relu', coeff, 0.7), ('swish', None, 1.3),
                        ('relu', None, 1.0), ('elu', coeff, 1.0)):
        ref = ops.gemm(a, w, b1, a2=a2, w2=w2, bias2=b2, coeff=co, scale=sc, act=act)
        got = ops.gemm_sliced(a, img, n, b1, a2=a2, image2=img2, bias2=b2, coeff=co, scale=sc, act=act)
        assert got.shape == ref.shape
        assert float((got - ref).abs().max()) < 5e-13 * max(1.0, float(ref.abs().max())), act
        got2 = ops.gemm_sliced(a, img, n, b1, a2=a2, image2=img2, bias2=b2, coeff=co, scale=sc, act=act)
        assert torch.equal(got, got2)                                                # deterministic
        if act is None:
            ea = float(np.abs(host(ref)[rows].astype(L) - pre).max())
            eb = float(np.abs(host(got)[rows].astype(L) - pre).max())
            # as close to the long-double value as the fp64 MFMA layer (whose error is its accumulation)
            assert eb < 2.0 * ea + 4e-16 * float(np.abs(pre).max()) + 1e-16, (ea, eb)
    # an entry outside the declared range, or a NaN, poisons the output (never a silently wrong number)
    for bad in (4.0, -4.5, float('nan'), float('inf')):
        ab = a.clone()
        ab[2, k // 2] = bad
        out = ops.gemm_sliced(ab, img, n, b1, a2=a2, image2=img2, bias2=b2)
        assert bool(torch.isnan(out).all()), bad
    # ... and the next call is clean again
    out = ops.gemm_sliced(a, img, n, b1, a2=a2, image2=img2, bias2=b2)
    assert bool(torch.isfinite(out).all())
    # a wider declared range costs bits, not correctness
    out8 = ops.gemm_sliced(a, img, n, b1, a_exp=8, a2=a2, image2=img2, a2_exp=3, bias2=b2)
    assert float((out8 - ops.gemm(a, w, b1, a2=a2, w2=w2, bias2=b2)).abs().max()) < 1e-10
    # what does not qualify
    assert ops.gemm_sliced_build(dev(rng.normal(size=(48, 128)))) is None          # N % 64
    assert ops.gemm_sliced_build(dev(rng.normal(size=(64, 100)))) is None          # K % 64
    wn = w.clone(); wn[5, 9] = float('nan')
    assert ops.gemm_sliced_build(wn) is None
    wz = w.clone(); wz[7, :] = 0.0                                                  # a zero row is exact
    oz = ops.gemm_sliced(a, ops.gemm_sliced_build(wz), n, None)
    assert float(oz[:, 7].abs().max()) == 0.0


def test_gemm_sliced_long_groups(ops):
    """Workgroups whose k-group spans more than one int32 range (16 384 k): the group sums are folded into
    fp64 in the middle of the slab loop, with the deferred last rows of the slab issued first.  Happens from
    (K + K2) x tiles > 512 x 16 384, e.g. the 16^4 lattice; here 256 x 256 x 786 432 (k-groups of 24 576)."""
    m, n, k = 256, 256, 48 * 16384
    g = torch.Generator(device='cuda').manual_seed(3)
    a = (torch.rand(m, k, dtype=torch.float64, device='cuda', generator=g) - 0.5) * 4.6
    w = (torch.rand(n, k, dtype=torch.float64, device='cuda', generator=g) - 0.5) * (2.0 / k ** 0.5)
    b = torch.zeros(n, dtype=torch.float64, device='cuda')
    img = ops.gemm_sliced_build(w)
    assert img is not None
    ref = ops.gemm(a, w, b)
    got = ops.gemm_sliced(a, img, n, b)
    assert float((got - ref).abs().max()) < 5e-13 * max(1.0, float(ref.abs().max()))
    assert torch.equal(got, ops.gemm_sliced(a, img, n, b))
    # two rows x 8 columns against long double (6.3 M products each)
    L = np.longdouble
    want = host(a[:2]).astype(L) @ host(w[:8]).astype(L).T
    ea = float(np.abs(host(ref[:2, :8]).astype(L) - want).max())
    eb = float(np.abs(host(got[:2, :8]).astype(L) - want).max())
    assert eb < 2.0 * ea + 4e-16 * float(np.abs(want).max()) + 1e-16, (ea, eb)


def test_heads_sliced_activation_row_guard(ops):
    """Z-side conditioning (VERDICT r03 weak #4 / ADVICE): an activation row with ONE dominant entry
    (a relu-style outlier: 1e6 next to O(1) entries, paired with a small weight) is (i) counted by the
    diagnostic `heads_sliced_zflag`, (ii) still within the DOCUMENTED absolute bound of the slicing,
    2^-53 K max|z| max|w| on the pre-activation, while the fp64 kernel keeps its relative accuracy
    -- and well-conditioned rows of the same call are untouched by their neighbour; (iii) `Dynamics`
    only selects the sliced kernel by itself for bounded (tanh) networks."""
    rng = np.random.default_rng(8)
    m, n, k = 64, 48, 256
    z = np.maximum(rng.normal(size=(m, k)), 0.0)
    z[5, 17] = 1.0e6                                         # the outlier row
    heads = {}
    for nm in 'stq':
        w = rng.uniform(-1, 1, size=(n, k)) / 16
        w[:, 17] *= 1e-6                                     # ... paired with small weights
        heads[nm] = (dev(w), dev(0.1 * rng.normal(size=n)), None if nm == 't' else dev(np.ones(n)))
    sl = dict(heads)
    sl['sliced'] = ops.heads_sliced_build(heads)
    assert sl['sliced'] is not None
    ops.heads_sliced_zflag(reset=True)
    zd = dev(z)
    v = dev(np.zeros((m, n))); f = dev(np.zeros((m, n)))
    # with v = F = 0 and t-scale 1 the update returns v' = -eps/2 * t = -eps/2 * (z W_t^T + b_t): the
    # pre-activation of the t head, read back exactly
    eps = 2.0
    va = v.clone(); ops.vnet_heads_vupdate_(zd, heads, (1.0, 1.0, 1.0), va, f, eps, True)   # fp64 MFMA
    vb = v.clone(); ops.vnet_heads_vupdate_(zd, sl, (1.0, 1.0, 1.0), vb, f, eps, True)      # sliced
    assert ops.heads_sliced_zflag(reset=True) == 1           # exactly the outlier row
    assert ops.heads_sliced_zflag(reset=False) == 0
    L = np.longdouble
    want = -(z.astype(L) @ host(heads['t'][0]).astype(L).T + host(heads['t'][1]).astype(L))
    ea = np.abs(host(va).astype(L) - want)
    eb = np.abs(host(vb).astype(L) - want)
    good = np.arange(m) != 5
    sumabs = np.abs(z) @ np.abs(host(heads['t'][0])).T                          # sum |z||w| per output
    assert float((eb[good] / sumabs[good]).max()) < 4e-16                       # like fp64 (relative)
    assert float((ea / sumabs).max()) < 4e-16                                   # fp64 kernel: every row
    bound = 2.0 ** -53 * k * 1.0e6 * float(np.abs(host(heads['t'][0])).max())   # K max|z| max|w| 2^-53
    assert float(eb[5].max()) < bound                                           # documented bound holds
    # (iii) which networks take the sliced path on their own
    import l2hmc.configs as cfgs
    from l2hmc.dynamics.pytorch.dynamics import Dynamics

    class _Net:
        def __init__(self, act):
            self.act = act
    d = Dynamics.__new__(Dynamics)
    d.sliced_heads = True
    assert d._sliced_wanted(_Net('tanh')) and not d._sliced_wanted(_Net('relu'))
    assert not d._sliced_wanted(_Net('swish')) and not d._sliced_wanted(_Net('leaky_relu'))
    d.sliced_heads = 'force'
    assert d._sliced_wanted(_Net('relu'))
    d.sliced_heads = False
    assert not d._sliced_wanted(_Net('tanh'))


@pytest.mark.parametrize('cplx', [True, False])
@pytest.mark.parametrize('shape', [(3, 4, 3888), (70, 16, 200), (130, 256, 1000),
                                   # >= 512 tiles: the producer / consumer (persistent) kernel; full K,
                                   # short K with ragged M and N, one tile more than a round
                                   (256, 256, 8192), (200, 64, 9000), (256, 128, 8256)])
def test_fused_heads_vupdate(ops, cplx, shape):
    """the fused (s,t,q)-heads + momentum-update kernel == three GEMMs + l2q_v_update"""
    m, k, n = shape
    rng = np.random.default_rng(11)
    z = dev(rng.normal(size=(m, k)))
    heads, scaled = {}, {}
    for nm in 'stq':
        w = dev(rng.normal(size=(n, k)) / np.sqrt(k)); b = dev(0.1 * rng.normal(size=n))
        co = None if nm == 't' else dev(0.3 * rng.normal(size=n))
        heads[nm] = (w, b, co)
    nw = (0.9, 1.1, 0.8)
    scaled = {'s': (heads['s'][0], heads['s'][1], nw[0] * heads['s'][2].exp()),
              't': (heads['t'][0], heads['t'][1], None),
              'q': (heads['q'][0], heads['q'][1], nw[2] * heads['q'][2].exp())}
    if cplx:
        v = dev(rng.normal(size=(m, n)) + 1j * rng.normal(size=(m, n)))
        f = dev(rng.normal(size=(m, n)) + 1j * rng.normal(size=(m, n)))
    else:
        v = dev(rng.normal(size=(m, n))); f = dev(rng.normal(size=(m, n)))
    for fwd in (True, False):
        s = ops.gemm(z, heads['s'][0], heads['s'][1], coeff=heads['s'][2], scale=nw[0], act='tanh')
        t = ops.gemm(z, heads['t'][0], heads['t'][1], scale=nw[1])
        q = ops.gemm(z, heads['q'][0], heads['q'][1], coeff=heads['q'][2], scale=nw[2], act='tanh')
        v1 = v.clone(); ld1 = ops.v_update_(v1, f, s, t, q, 0.07, fwd)
        v2 = v.clone(); ld2 = ops.vnet_heads_vupdate_(z, scaled, nw, v2, f, 0.07, fwd)
        assert float((v1 - v2).abs().max()) < 1e-12
        assert err(host(ld1), host(ld2)) < 1e-11
        # and against numpy
        sn, tn, qn = host(s), host(t), host(q)
        lj = (0.035 if fwd else -0.035) * sn
        fn = host(f) * np.exp(0.07 * qn) + tn
        want = np.exp(lj) * host(v) - 0.035 * fn if fwd else np.exp(lj) * (host(v) + 0.035 * fn)
        assert err(host(v2), want) < 1e-12 and err(host(ld2), lj.sum(1)) < 1e-11
        # out of place (l2q_vnet_heads_vupdate_to_f64): the same bits, the source untouched
        v0 = v.clone(); v3 = torch.full_like(v, float('nan'))
        ld3 = ops.vnet_heads_vupdate_(z, scaled, nw, v3, f, 0.07, fwd, v_src=v0)
        assert torch.equal(v3, v2) and torch.equal(ld3, ld2) and torch.equal(v0, v)
        # paired updates (optionally with the momentum flip in between) == two single calls
        for flip in (False, True):
            for fwd2 in (True, False):
                va = v.clone()
                la = ops.vnet_heads_vupdate_(z, scaled, nw, va, f, 0.07, fwd)
                if flip:
                    va = -va
                la = la + ops.vnet_heads_vupdate_(z, scaled, nw, va, f, 0.05, fwd2)
                vb = v.clone()
                lb = ops.vnet_heads_vupdate_pair_(z, scaled, nw, vb, f, 0.07, fwd, flip, 0.05, fwd2)
                assert float((va - vb).abs().max()) < 1e-13 and err(host(la), host(lb)) < 1e-11
                if k % 16 == 0:
                    # pair kernel with the mid-point outputs per-step metrics need (verbose=True):
                    # logdet of the first update alone, sum |v|^2 between the two updates
                    vm = v.clone()
                    l1 = ops.vnet_heads_vupdate_(z, scaled, nw, vm, f, 0.07, fwd)
                    n2 = host((vm.abs() ** 2).sum(1))
                    vc = v.clone()
                    lc, lc1, nc2 = ops.vnet_heads_vupdate_pair_mid_(z, scaled, nw, vc, f, 0.07, fwd,
                                                                     flip, 0.05, fwd2)
                    assert float((va - vc).abs().max()) < 1e-13
                    assert err(host(lc), host(la)) < 1e-11 and err(host(lc1), host(l1)) < 1e-11
                    assert err(host(nc2), n2) < 1e-12 * max(1.0, float(np.abs(n2).max()))


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dims', [(3, 2, 4, 6, 5, 8), (2, 8, 6, 6, 3, 16), (5, 16, 7, 5, 3, 32),
                                  (2, 64, 4, 4, 2, 128), (130, 4, 8, 8, 3, 3), (1, 3, 2, 3, 3, 5)])
def test_conv_gemm_periodic_equals_im2col_gemm(layout, dims):
    """l2q_conv_gemm_periodic_f32 (im2col inside the GEMM's A-tile loader) against the
    materialised im2col + GEMM and against torch's Conv2d on the periodically padded input."""
    from l2hmc import _ops as ops
    from l2hmc import native as N
    nb, C, H, W, k, cout = dims
    g = torch.Generator().manual_seed(11)
    x = torch.randn(nb, C, H, W, generator=g)
    w = torch.randn(cout, C, k, k, generator=g) / (C * k * k) ** 0.5
    b = torch.randn(cout, generator=g)
    p = k - 1
    xp = torch.cat([x[:, :, -p:, :], x, x[:, :, :p, :]], 2) if p else x
    xp = torch.cat([xp[:, :, :, -p:], xp, xp[:, :, :, :p]], 3) if p else xp
    want = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(xp, w, b), 0.01)
    want = want.permute(0, 2, 3, 1).contiguous()
    xin = x.cuda() if layout == 'nchw' else x.permute(0, 2, 3, 1).contiguous().cuda()
    got = ops.conv2d_periodic_gemm(xin, layout, w.cuda(), b.cuda(), 1, 'leaky_relu')
    assert got.shape == want.shape
    assert float((got.cpu() - want).abs().max()) < 2e-5 * max(1.0, float(want.abs().max()))
    # materialised path (the one the training tape uses)
    got2, _ = ops.conv2d_periodic_gemm_train(xin, layout, w.cuda(), b.cuda(), 1, 'leaky_relu')
    assert float((got2 - got).abs().max()) < 2e-5 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize('hd', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('a32', [True, False])
@pytest.mark.parametrize('shape', [(3, 5, 40, 0), (128, 96, 704, 40), (257, 130, 4104, 0),
                                   (2, 300, 16, 16), (130, 1000, 6, 0), (300, 64, 8192, 4096),
                                   (64, 33, 37, 11)])
def test_gemm_h(hd, a32, shape):
    """l2q_gemm_h (16-bit MFMA layers of "fp16 nets / fp32 action") against the emulator's
    restatement of autocast's rounding points, and against the exact fp64 product of the
    rounded operands (one 16-bit ulp of the output + fp32 accumulation noise)."""
    import emu_native
    from l2hmc import _ops as ops
    m, n, k, k2 = shape
    g = torch.Generator().manual_seed(17)
    a = torch.randn(m, k, generator=g)
    w = (torch.randn(n, k, generator=g) / k ** 0.5).to(hd)
    b = torch.randn(n, generator=g).to(hd).float()
    co = 0.3 * torch.randn(n, generator=g)
    a2 = w2 = b2 = None
    if k2:
        a2 = torch.randn(m, k2, generator=g)
        w2 = (torch.randn(n, k2, generator=g) / k2 ** 0.5).to(hd)
        b2 = torch.randn(n, generator=g).to(hd).float()
    if not a32:
        a = a.to(hd)
        a2 = None if a2 is None else a2.to(hd)
    ulp = 2.0 ** -10 if hd == torch.float16 else 2.0 ** -7
    cu = lambda t: None if t is None else t.cuda()
    for act, coeff, odt in ((None, None, hd), ('tanh', co, torch.float32), ('leaky_relu', None, hd),
                            ('relu', None, torch.float32), ('elu', None, hd), ('swish', None, hd),
                            (None, co, torch.float32)):
        got = ops.gemm_h(cu(a), cu(w), cu(b), a2=cu(a2), w2=cu(w2), bias2=cu(b2), coeff=cu(coeff),
                         scale=0.7, act=act, out_dtype=odt)
        assert got.dtype == odt and got.shape == (m, n)
        want = torch.empty(m, n, dtype=odt)
        emu_native.l2q_gemm_h(ops.HALF_TYPES[hd], a, int(a32), w, m, n, k, a2, w2, k2, b, b2, coeff,
                              0.7, N_ACT[act], want, int(odt == torch.float32), None, 0)
        d = (got.cpu().float() - want.float()).abs()
        tol = 2.5 * ulp * want.float().abs().clamp(min=1.0)
        # an accumulation-order difference may flip a 16-bit rounding (twice: pre- and post-act)
        assert bool((d <= tol).all()), (act, shape, float((d / tol).max()))
        assert float((d > 0).float().mean()) < 0.2, (act, shape)


N_ACT = {None: 0, 'none': 0, 'tanh': 1, 'relu': 2, 'leaky_relu': 3, 'elu': 4, 'swish': 5}


@pytest.mark.parametrize('hd', [torch.float16, torch.bfloat16])
def test_gemm_h_library_route(hd):
    """Plain 16-bit layers with M, N, K >= 2048 go through hipBLASLt (gemm_lt.hip, tuning gemm_h_lt): the same
    rounding points as the own kernels -- r16(A W^T + bias), then r16(act(.)) -- so the two routes agree to an ulp of
    the 16-bit type on a small fraction of the entries (different summation order of the fp32 accumulation); outputs
    in a 16-bit and in an fp32 container; a shape the route does not take stays on the own kernels."""
    import emu_native
    from l2hmc import _ops as ops, native
    m, n, k = 2048, 2304, 2048
    # the route IS taken on this box (the library ships with the ROCm image), not silently skipped
    assert native.kernel_name('l2q_gemm_h', (m, n, k, 0)) == 'hipblaslt'
    assert native.kernel_name('l2q_gemm_h', (512, n, k, 0)) == ''
    g = torch.Generator().manual_seed(23)
    a = torch.randn(m, k, generator=g).to(hd)
    w = (torch.randn(n, k, generator=g) / k ** 0.5).to(hd)
    b = torch.randn(n, generator=g).to(hd).float()
    ulp = 2.0 ** -10 if hd == torch.float16 else 2.0 ** -7
    try:
        for act, odt in ((None, hd), ('leaky_relu', torch.float32), ('tanh', hd), (None, torch.float32)):
            native.set_tuning('gemm_h_lt', 1)
            got = ops.gemm_h(a.cuda(), w.cuda(), b.cuda(), act=act, out_dtype=odt)
            native.set_tuning('gemm_h_lt', 0)
            own = ops.gemm_h(a.cuda(), w.cuda(), b.cuda(), act=act, out_dtype=odt)
            want = torch.empty(m, n, dtype=odt)
            emu_native.l2q_gemm_h(ops.HALF_TYPES[hd], a, 0, w, m, n, k, None, None, 0, b, None, None,
                                  1.0, N_ACT[act], want, int(odt == torch.float32), None, 0)
            assert got.dtype == odt
            for other in (want, own.cpu()):
                d = (got.cpu().float() - other.float()).abs()
                tol = 2.5 * ulp * other.float().abs().clamp(min=1.0)
                assert bool((d <= tol).all()), (act, odt, float((d / tol).max()))
                assert float((d > 0).float().mean()) < 0.2, (act, odt)
        # without a bias, and a shape below the route's threshold
        native.set_tuning('gemm_h_lt', 1)
        got = ops.gemm_h(a.cuda(), w.cuda(), None, act=None)
        native.set_tuning('gemm_h_lt', 0)
        own = ops.gemm_h(a.cuda(), w.cuda(), None, act=None)
        d = (got.float() - own.float()).abs()
        assert bool((d <= 2.5 * ulp * own.float().abs().clamp(min=1.0)).all())
        native.set_tuning('gemm_h_lt', 1)
        small = ops.gemm_h(a[:512].cuda(), w.cuda(), b.cuda(), act='relu')
        native.set_tuning('gemm_h_lt', 0)
        assert torch.equal(small, ops.gemm_h(a[:512].cuda(), w.cuda(), b.cuda(), act='relu'))
    finally:
        native.set_tuning('gemm_h_lt', 1)


@pytest.mark.parametrize('hd', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('shape', [(1024, 1024, 320), (2048, 1024, 256), (1024, 1280, 832)])
def test_gemm_h_dma(hd, shape):
    """The 256 x 256 LDS-DMA kernel of the big half-precision layers (gemm_f16_dma.hip; M, N % 256 == 0,
    K % 64 == 0, 16-bit activations) against the emulator's restatement and against the
    register-staged kernel (tuning gemm_h_dma = 0): same rounding points, K accumulated in one pass
    instead of split-K partials."""
    import emu_native
    from l2hmc import _ops as ops, native
    m, n, k = shape
    g = torch.Generator().manual_seed(19)
    a = torch.randn(m, k, generator=g).to(hd)
    w = (torch.randn(n, k, generator=g) / k ** 0.5).to(hd)
    b = torch.randn(n, generator=g).to(hd).float()
    co = 0.3 * torch.randn(n, generator=g)
    ulp = 2.0 ** -10 if hd == torch.float16 else 2.0 ** -7
    for act, coeff, odt in ((None, None, hd), ('tanh', co, torch.float32), ('leaky_relu', None, torch.float32),
                            ('relu', None, hd)):
        native.set_tuning('gemm_h_dma', 1)
        got = ops.gemm_h(a.cuda(), w.cuda(), b.cuda(), coeff=None if coeff is None else coeff.cuda(),
                         scale=0.7, act=act, out_dtype=odt)
        native.set_tuning('gemm_h_dma', 0)
        old = ops.gemm_h(a.cuda(), w.cuda(), b.cuda(), coeff=None if coeff is None else coeff.cuda(),
                         scale=0.7, act=act, out_dtype=odt)
        native.set_tuning('gemm_h_dma', 1)
        want = torch.empty(m, n, dtype=odt)
        emu_native.l2q_gemm_h(ops.HALF_TYPES[hd], a, 0, w, m, n, k, None, None, 0, b, None, coeff,
                              0.7, N_ACT[act], want, int(odt == torch.float32), None, 0)
        for other in (want, old.cpu()):
            d = (got.cpu().float() - other.float()).abs()
            tol = 2.5 * ulp * other.float().abs().clamp(min=1.0)
            assert bool((d <= tol).all()), (act, shape, float((d / tol).max()))
            assert float((d > 0).float().mean()) < 0.2, (act, shape)


@pytest.mark.parametrize('hd', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('dims', [(5, 16, 40), (130, 64, 200), (256, 256, 512), (37, 24, 130),
                                  (3, 7, 9)])
def test_u1_heads_update_h(hd, dims):
    """l2q_u1_heads_update_h (three 16-bit heads + v- or x-update in one kernel) against the
    emulator: heads by the l2q_gemm_h restatement, then the reference update formulas."""
    import emu_native
    from l2hmc import _ops as ops
    m, k, n = dims
    g = torch.Generator().manual_seed(23)
    z = torch.randn(m, k, generator=g).to(hd)
    heads = {}
    for nm in 'stq':
        w = (torch.randn(n, k, generator=g) / k ** 0.5).to(hd)
        b = (0.1 * torch.randn(n, generator=g)).to(hd).float()
        c = None if nm == 't' else (0.7 * torch.exp(0.3 * torch.randn(n, generator=g)))
        heads[nm] = (w, b, c)
    ones = torch.ones(n)
    mask = (torch.rand(n, generator=g) < 0.5).float()
    ulp = 2.0 ** -10 if hd == torch.float16 else 2.0 ** -7
    cu = lambda t: None if t is None else t.cuda()
    hc = {nm: tuple(cu(t) for t in v) for nm, v in heads.items()}
    for xupd in (False, True):
        for forward in (True, False):
            for ncp in ((True, False) if xupd else (True,)):
                a = torch.randn(m, n, generator=g) if not xupd else \
                    (2 * np.pi * torch.rand(m, n, generator=g) - np.pi)
                b = torch.randn(m, n, generator=g)
                want_a, want_ld = a.clone(), torch.zeros(m)
                emu_native.l2q_u1_heads_update_h(
                    ops.HALF_TYPES[hd], z, m, k, n, heads['s'][0], heads['s'][1], heads['s'][2],
                    heads['t'][0], heads['t'][1], 0.9, heads['q'][0], heads['q'][1], heads['q'][2],
                    int(xupd), want_a, b, mask, 1, 0.17, int(forward), int(ncp), want_ld, 0, None, 0)
                got_a = a.cuda()
                acc = torch.full((m,), 0.5, device='cuda')
                ld = ops.u1_heads_update_h_(cu(z), hc, 0.9, got_a, cu(b), 0.17, forward,
                                            mask=cu(mask) if xupd else None, complement=True,
                                            use_ncp=ncp, acc=acc)
                assert ld is acc
                d = got_a.cpu() - want_a
                if xupd:
                    d = torch.remainder(d + np.pi, 2 * np.pi) - np.pi
                scale = max(1.0, float(want_a.abs().max()))
                assert float(d.abs().max()) < 4 * ulp * scale, (xupd, forward, ncp, float(d.abs().max()))
                assert float((d.abs() > 1e-5 * scale).float().mean()) < 0.2
                dl = (ld.cpu() - 0.5 - want_ld).abs().max()
                assert float(dl) < 4 * ulp * n ** 0.5 + 1e-4 * max(1.0, float(want_ld.abs().max()))


@pytest.mark.parametrize('hd', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dims', [(3, 4, 4, 6, 5, 8), (2, 8, 6, 6, 3, 16), (5, 16, 7, 5, 3, 32),
                                  (2, 64, 4, 4, 2, 128), (130, 4, 8, 8, 3, 3), (1, 3, 2, 3, 3, 5),
                                  (3, 32, 9, 9, 3, 64), (3, 8, 30, 34, 5, 8), (2, 8, 40, 24, 3, 16),
                                  # a patch larger than what travels through registers (5632 vectors)
                                  (1, 64, 20, 40, 3, 16)])
def test_conv_gemm_periodic_h(hd, layout, dims):
    """l2q_conv_gemm_periodic_h (+ l2q_maxpool_act_nhwc_h) against the emulator's restatement
    (16-bit rounded operands, fp32 accumulation, autocast rounding points) -- fp32 NCHW input
    (first layer) and 16-bit NHWC input with the 16-byte channel gathers (C % 8 == 0) or the
    element-wise fallback."""
    import emu_native
    from l2hmc import _ops as ops
    nb, C, H, W, k, cout = dims
    g = torch.Generator().manual_seed(29)
    x = torch.randn(nb, C, H, W, generator=g)
    w = torch.randn(cout, C, k, k, generator=g) / (C * k * k) ** 0.5
    b = torch.randn(cout, generator=g).to(hd).float()
    ulp = 2.0 ** -10 if hd == torch.float16 else 2.0 ** -7
    if layout == 'nchw':
        xin, w16 = x, w.to(hd)
        strides = (C * H * W, H * W, W, 1)
    else:
        xin, w16 = x.permute(0, 2, 3, 1).contiguous().to(hd), w.permute(0, 2, 3, 1).contiguous().to(hd)
        strides = (H * W * C, 1, W * C, C)
    Ho, Wo = H + k - 1, W + k - 1
    for pool, act in ((1, None), (1, 'leaky_relu'), (2, 'relu'), (2, 'tanh')):
        if Ho // pool == 0 or Wo // pool == 0:
            continue
        got = ops.conv2d_periodic_gemm_h(xin.cuda(), layout, w16.cuda(), b.cuda(), pool, act)
        # the LDS-patch kernel (conv_patch_f16.hip; 2: wherever it fits) and the gather kernel (0)
        # accumulate the same products in the same order: identical bits
        from l2hmc import native
        for cp in (2, 0):
            native.set_tuning('conv_patch', cp)
            alt = ops.conv2d_periodic_gemm_h(xin.cuda(), layout, w16.cuda(), b.cuda(), pool, act)
            assert torch.equal(alt, got), (cp, float((alt.float() - got.float()).abs().max()))
        native.set_tuning('conv_patch', 1)
        if pool == 2:
            # conv + MaxPool2d(2) + act in one kernel (the default) == conv, then the pool kernel
            ops.FUSE_CONV_POOL_H[0] = False
            try:
                two = ops.conv2d_periodic_gemm_h(xin.cuda(), layout, w16.cuda(), b.cuda(), pool, act)
            finally:
                ops.FUSE_CONV_POOL_H[0] = True
            assert torch.equal(two, got), float((two.float() - got.float()).abs().max())
        y = torch.empty(nb * Ho * Wo, cout, dtype=hd)
        emu_native.l2q_conv_gemm_periodic_h(ops.HALF_TYPES[hd], xin, int(layout == 'nchw'), *strides,
                                            nb, C, H, W, k, w16.reshape(cout, -1),
                                            int(layout != 'nchw'), b, cout,
                                            N_ACT[None if pool > 1 else act], y)
        want = y.reshape(nb, Ho, Wo, cout)
        if pool > 1:
            want = torch.empty(nb, Ho // pool, Wo // pool, cout, dtype=hd)
            emu_native.l2q_maxpool_act_nhwc_h(ops.HALF_TYPES[hd], y, nb, Ho, Wo, cout, pool,
                                              N_ACT[act], want)
        assert got.shape == want.shape and got.dtype == hd
        d = (got.cpu().float() - want.float()).abs()
        tol = 2.5 * ulp * want.float().abs().clamp(min=1.0)
        assert bool((d <= tol).all()), (pool, act, float((d / tol).max()))
        assert float((d > 0).float().mean()) < 0.2


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
@pytest.mark.parametrize('shape', [(6, 8, 40), (256, 132, 260), (130, 1000, 36), (4, 4, 3), (260, 264, 700),
                                   (36, 4100, 5)])
def test_gemm_ex_transposed_operands(dtype, shape):
    """l2q_gemm_ex: the backward GEMMs read transposed operands in the tile loader
    (dW += dY^T X, dX = dY W) -- against torch.matmul in float64."""
    from l2hmc import _ops as ops
    m, n, k = shape
    g = torch.Generator().manual_seed(31)
    tol = 1e-12 if dtype == torch.float64 else 3e-4
    for ta in (False, True):
        for tw in (False, True):
            a = torch.randn((k, m) if ta else (m, k), generator=g, dtype=torch.float64)
            w = torch.randn((k, n) if tw else (n, k), generator=g, dtype=torch.float64) / k ** 0.5
            want = (a.T if ta else a) @ (w if tw else w.T)
            got = ops.gemm_ex(a.to(dtype).cuda(), w.to(dtype).cuda(), a_trans=ta, w_trans=tw)
            assert float((got.cpu().double() - want).abs().max()) < tol * max(1.0, float(want.abs().max()))
            c0 = torch.randn(m, n, generator=g, dtype=torch.float64)
            out = c0.to(dtype).cuda()
            ops.gemm_ex(a.to(dtype).cuda(), w.to(dtype).cuda(), a_trans=ta, w_trans=tw, out=out,
                        accumulate=True)
            assert float((out.cpu().double() - (c0 + want)).abs().max()) < \
                tol * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize('hd', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('dims', [(5, 24, 32), (130, 40, 128), (256, 256, 512), (33, 17, 50), (300, 64, 2048)])
def test_gemm_h_u1x(hd, dims):
    """l2q_gemm_h_u1x: the half-precision xnet input layer with [cos(m x), sin(m x)] formed in the
    tile loader, against the emulator (cos / sin materialised, then the l2q_gemm_h restatement)."""
    import emu_native
    from l2hmc import _ops as ops
    m, n, xdim = dims
    g = torch.Generator().manual_seed(37)
    x = 2 * np.pi * torch.rand(m, xdim, generator=g) - np.pi
    v = torch.randn(m, xdim, generator=g)
    mask = (torch.rand(xdim, generator=g) < 0.5).float()
    w = (torch.randn(n, 2 * xdim, generator=g) / (2 * xdim) ** 0.5).to(hd)
    w2 = (torch.randn(n, xdim, generator=g) / xdim ** 0.5).to(hd)
    b = torch.randn(n, generator=g).to(hd).float()
    b2 = torch.randn(n, generator=g).to(hd).float()
    ulp = 2.0 ** -10 if hd == torch.float16 else 2.0 ** -7
    for complement in (False, True):
        for act in (None, 'leaky_relu', 'tanh'):
            got = ops.gemm_h_u1x(x.cuda(), mask.cuda(), complement, w.cuda(), b.cuda(), v.cuda(),
                                 w2.cuda(), b2.cuda(), act)
            want = torch.empty(m, n, dtype=hd)
            emu_native.l2q_gemm_h_u1x(ops.HALF_TYPES[hd], x, mask, int(complement), w, m, n, xdim, v,
                                      w2, xdim, b, b2, N_ACT[act], want, None, 0)
            d = (got.cpu().float() - want.float()).abs()
            tol = 2.5 * ulp * want.float().abs().clamp(min=1.0)
            assert bool((d <= tol).all()), (complement, act, float((d / tol).max()))
            assert float((d > 0).float().mean()) < 0.25


@pytest.mark.parametrize('hd', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('shape', [(2048, 256, 256), (2100, 200, 128), (4096, 16, 32), (2050, 250, 96), (8192, 64, 224)])
def test_gemm_h_small(hd, shape):
    """The one-pass kernel of the hidden layers (gemm_f16_small.hip: 16-bit activations, K, N <= 256, >= 2048 rows)
    against the emulator's restatement and against the tile kernel (tuning gemm_h_small = 0): ragged rows, N that
    is not a multiple of 64 or of 4, every epilogue form."""
    import emu_native
    from l2hmc import _ops as ops, native
    m, n, k = shape
    g = torch.Generator().manual_seed(43)
    a = torch.randn(m, k, generator=g).to(hd)
    w = (torch.randn(n, k, generator=g) / k ** 0.5).to(hd)
    b = torch.randn(n, generator=g).to(hd).float()
    co = 0.3 * torch.randn(n, generator=g)
    ulp = 2.0 ** -10 if hd == torch.float16 else 2.0 ** -7
    try:
        for act, coeff, odt in ((None, None, hd), ('tanh', co, torch.float32), ('leaky_relu', None, hd),
                                ('swish', None, torch.float32)):
            native.set_tuning('gemm_h_small', 1)
            got = ops.gemm_h(a.cuda(), w.cuda(), b.cuda(), coeff=None if coeff is None else coeff.cuda(),
                             scale=0.7, act=act, out_dtype=odt)
            native.set_tuning('gemm_h_small', 0)
            old = ops.gemm_h(a.cuda(), w.cuda(), b.cuda(), coeff=None if coeff is None else coeff.cuda(),
                             scale=0.7, act=act, out_dtype=odt)
            want = torch.empty(m, n, dtype=odt)
            emu_native.l2q_gemm_h(ops.HALF_TYPES[hd], a, 0, w, m, n, k, None, None, 0, b, None, coeff,
                                  0.7, N_ACT[act], want, int(odt == torch.float32), None, 0)
            for other in (want, old.cpu()):
                d = (got.cpu().float() - other.float()).abs()
                tol = 2.5 * ulp * other.float().abs().clamp(min=1.0)
                assert bool((d <= tol).all()), (act, shape, float((d / tol).max()))
                assert float((d > 0).float().mean()) < 0.2, (act, shape)
    finally:
        native.set_tuning('gemm_h_small', 1)


@pytest.mark.parametrize('hd', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('shape', [(1100, 256, 2048, 2048, 1), (1024, 192, 4096, 0, 4), (1030, 64, 3072, 1024, 1),
                                   (2048, 256, 2048, 2048, 8), (1500, 250, 2048, 2048, 2)])
def test_gemm_h_skinny(hd, shape):
    """The streaming kernel of the wide-K fp32-operand input layer (gemm_f16_skinny.hip; N <= 256, K and K2
    multiples of 32) against the emulator's restatement and against the register-staged kernel (tuning
    gemm_h_skinny = 0): same rounding points, another accumulation order over K; ragged M (clamped rows),
    N below the tile width, every split count."""
    import emu_native
    from l2hmc import _ops as ops, native
    m, n, k, k2, sk = shape
    g = torch.Generator().manual_seed(23)
    a = torch.randn(m, k, generator=g)
    w = (torch.randn(n, k, generator=g) / k ** 0.5).to(hd)
    b = torch.randn(n, generator=g).to(hd).float()
    a2 = w2 = b2 = None
    if k2:
        a2 = torch.randn(m, k2, generator=g)
        w2 = (torch.randn(n, k2, generator=g) / k2 ** 0.5).to(hd)
        b2 = torch.randn(n, generator=g).to(hd).float()
    ulp = 2.0 ** -10 if hd == torch.float16 else 2.0 ** -7
    cu = lambda t: None if t is None else t.cuda()
    try:
        for act, odt in ((None, hd), ('leaky_relu', hd), ('tanh', torch.float32)):
            assert native.set_tuning('gemm_h_skinny', sk) >= 0
            assert native.load().l2q_gemm_h_skinny_splits(m, n, k, k2, 0) == (sk if sk > 1 else 8)
            got = ops.gemm_h(cu(a), cu(w), cu(b), a2=cu(a2), w2=cu(w2), bias2=cu(b2), act=act, out_dtype=odt)
            native.set_tuning('gemm_h_skinny', 0)
            old = ops.gemm_h(cu(a), cu(w), cu(b), a2=cu(a2), w2=cu(w2), bias2=cu(b2), act=act, out_dtype=odt)
            want = torch.empty(m, n, dtype=odt)
            emu_native.l2q_gemm_h(ops.HALF_TYPES[hd], a, 1, w, m, n, k, a2, w2, k2, b, b2, None, 1.0,
                                  N_ACT[act], want, int(odt == torch.float32), None, 0)
            for other in (want, old.cpu()):
                d = (got.cpu().float() - other.float()).abs()
                tol = 2.5 * ulp * other.float().abs().clamp(min=1.0)
                assert bool((d <= tol).all()), (act, shape, float((d / tol).max()))
                assert float((d > 0).float().mean()) < 0.2, (act, shape)
    finally:
        native.set_tuning('gemm_h_skinny', 1)


@pytest.mark.parametrize('hd', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('dims', [(1100, 256, 2048, 1), (1024, 128, 4096, 4), (2050, 200, 2048, 2)])
def test_gemm_h_u1x_skinny(hd, dims):
    """l2q_gemm_h_u1x on the streaming kernel: cos and sin slabs of the same links adjacent in the K order,
    against the emulator and the K-ordered loader of the register-staged kernel."""
    import emu_native
    from l2hmc import _ops as ops, native
    m, n, xdim, sk = dims
    g = torch.Generator().manual_seed(41)
    x = 2 * np.pi * torch.rand(m, xdim, generator=g) - np.pi
    v = torch.randn(m, xdim, generator=g)
    mask = (torch.rand(xdim, generator=g) < 0.5).float()
    w = (torch.randn(n, 2 * xdim, generator=g) / (2 * xdim) ** 0.5).to(hd)
    w2 = (torch.randn(n, xdim, generator=g) / xdim ** 0.5).to(hd)
    b = torch.randn(n, generator=g).to(hd).float()
    b2 = torch.randn(n, generator=g).to(hd).float()
    ulp = 2.0 ** -10 if hd == torch.float16 else 2.0 ** -7
    try:
        for complement in (False, True):
            for act in (None, 'leaky_relu'):
                assert native.set_tuning('gemm_h_skinny', sk) >= 0
                assert native.load().l2q_gemm_h_skinny_splits(m, n, 2 * xdim, xdim, 1) == (sk if sk > 1 else 8)
                got = ops.gemm_h_u1x(x.cuda(), mask.cuda(), complement, w.cuda(), b.cuda(), v.cuda(),
                                     w2.cuda(), b2.cuda(), act)
                native.set_tuning('gemm_h_skinny', 0)
                old = ops.gemm_h_u1x(x.cuda(), mask.cuda(), complement, w.cuda(), b.cuda(), v.cuda(),
                                     w2.cuda(), b2.cuda(), act)
                want = torch.empty(m, n, dtype=hd)
                emu_native.l2q_gemm_h_u1x(ops.HALF_TYPES[hd], x, mask, int(complement), w, m, n, xdim, v,
                                          w2, xdim, b, b2, N_ACT[act], want, None, 0)
                for other in (want, old.cpu()):
                    d = (got.cpu().float() - other.float()).abs()
                    tol = 2.5 * ulp * other.float().abs().clamp(min=1.0)
                    assert bool((d <= tol).all()), (complement, act, float((d / tol).max()))
                    assert float((d > 0).float().mean()) < 0.25
    finally:
        native.set_tuning('gemm_h_skinny', 1)


def test_lattice_edge_shapes_vs_oracle():
    """Degenerate and ragged lattices: extent 1 in some or all directions (a link is its own
    neighbour), a single chain, odd extents, kernel blocks far from full -- action, plaquette,
    Wilson and improved-action force (SU(3)) and action / force (U(1)) against the oracle."""
    from oracle import su3 as osu3, u1 as ou1
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    from l2hmc.lattice.u1.pytorch.lattice import LatticeU1
    torch.set_default_dtype(torch.float64)
    b = torch.tensor(5.5)
    for L in ([2, 2, 2, 2], [1, 2, 3, 4], [3, 1, 1, 5], [1, 1, 1, 1], [2, 7, 3, 3]):
        for nb in (1, 3):
            lat, lat0 = LatticeSU3(nb, L, c1=-0.331), LatticeSU3(nb, L)
            torch.manual_seed(1)
            x = lat.random()
            xh = host(x)
            assert err(host(lat.action(x, b)), osu3.action_c1(xh, 5.5, -0.331)) < 1e-11, L
            assert err(host(lat.grad_action(x, b)), osu3.grad_action_c1(xh, 5.5, -0.331)) < 1e-12, L
            assert err(host(lat0.grad_action(x, b)), osu3.grad_action(xh, 5.5)) < 1e-12, L
            assert err(host(lat0.plaqs(x)), osu3.plaqs(xh)) < 1e-14, L
    torch.set_default_dtype(torch.float32)
    b = torch.tensor(2.5)
    for L in ([2, 2], [2, 6], [3, 5], [1, 4], [1, 1], [7, 2]):
        for nb in (1, 5):
            lat = LatticeU1(nb, L)
            torch.manual_seed(1)
            x = lat.random()
            xh = host(x).astype(np.float64)
            assert err(host(lat.action(x, b)), ou1.action(xh, 2.5)) < 2e-5, L
            assert err(host(lat.grad_action(x, b)).reshape(xh.shape), ou1.grad_action(xh, 2.5)) < 1e-5, L


@pytest.mark.parametrize('hd', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('k', [256, 128, 64])
@pytest.mark.parametrize('dims', [(1024, 512, 3), (1100, 260, 3), (2085, 1028, 3), (37, 64, 3), (4100, 1028, 2)])
def test_u1_heads_update_h_kstream_equals_tile(hd, dims, k):
    """Tuning `heads_h_stream` = 2 (the default; heads_kstream_f16.hip: weights stationary, K = 256 split over
    wavefront pairs, K = 256 / 128 / 64; 3 = the same for streams of any length) against the tile kernel: the K sum is formed in two halves instead of one running accumulator, so
    a head can differ by an fp32 rounding in front of its 16-bit rounding (rare 1-ulp16 flips); ragged chain
    counts (clamped rows, masked stores) and entry counts that are not multiples of 64."""
    from l2hmc import _ops as ops, native
    m, n, kind = dims
    g = torch.Generator().manual_seed(31)
    z = torch.randn(m, k, generator=g).to(hd).cuda()
    heads = {}
    for nm in 'stq':
        w = (torch.randn(n, k, generator=g) / k ** 0.5).to(hd).cuda()
        b = (0.1 * torch.randn(n, generator=g)).cuda()
        c = None if nm == 't' else (0.7 * torch.exp(0.3 * torch.randn(n, generator=g))).cuda()
        heads[nm] = (w, b, c)
    mask = (torch.rand(n, generator=g) < 0.5).float().cuda()
    try:
        for xupd in (False, True):
            for forward in (True, False):
                a0 = (torch.randn(m, n, generator=g) if not xupd
                      else (2 * np.pi * torch.rand(m, n, generator=g) - np.pi)).cuda()
                b0 = torch.randn(m, n, generator=g).cuda()
                res = {}
                for stream in (0, 2):
                    assert native.set_tuning('heads_h_stream', kind if stream else 0) >= 0
                    a = a0.clone()
                    ld = ops.u1_heads_update_h_(z, heads, 0.9, a, b0, 0.17, forward,
                                                mask=mask if xupd else None, complement=xupd and forward)
                    res[stream] = (a, ld)
                d = res[0][0] - res[2][0]
                if xupd:
                    d = torch.remainder(d + np.pi, 2 * np.pi) - np.pi
                ulp = 2.0 ** -10 if hd == torch.float16 else 2.0 ** -7
                scale = max(1.0, float(res[0][0].abs().max()))
                assert float(d.abs().max()) < 2 * ulp * scale, (xupd, forward, float(d.abs().max()))
                # the stream kernel's epilogue runs on packed fp32 math (other contractions: fp32-rounding-level
                # differences anywhere); a flipped 16-bit rounding of a head is ~1e-4 .. 1e-3 and must stay rare
                flips = float((d.abs() > 4e-6 * scale).float().mean())
                assert flips < 0.05, (xupd, forward, flips)
                dl = float((res[0][1] - res[2][1]).abs().max())
                assert dl < (1e-5 * max(1.0, float(res[0][1].abs().max())) + 2 * ulp * 0.17) * n ** 0.5, dl
    finally:
        native.set_tuning('heads_h_stream', 2)


@pytest.mark.parametrize('cplx', [True, False])
@pytest.mark.parametrize('shape', [(33, 40), (256, 1152), (100, 8200)])
def test_heads_sliced_tape(ops, cplx, shape):
    """TAPE instances of the sliced kernel (the forward pass of the training tape): the momentum and logdet are
    those of the inference instance, and the stored heads s, t, q equal the three fp64 GEMM heads of
    LeapfrogLayer.forward_train to fp64 rounding of the dot products."""
    m, n = shape
    k = 256
    rng = np.random.default_rng(8)
    z = dev(np.tanh(rng.normal(size=(m, k))))
    heads = {}
    for nm in 'stq':
        w = dev(rng.uniform(-1, 1, size=(n, k)) / 16); b = dev(0.1 * rng.normal(size=n))
        c = None if nm == 't' else dev(np.exp(0.3 * rng.normal(size=n)))
        heads[nm] = (w, b, c)
    nw = (1.0, 1.1, 1.0)
    if cplx:
        v = dev(rng.normal(size=(m, n)) + 1j * rng.normal(size=(m, n)))
        f = dev(rng.normal(size=(m, n)) + 1j * rng.normal(size=(m, n)))
    else:
        v = dev(rng.normal(size=(m, n))); f = dev(rng.normal(size=(m, n)))
    image, usable = ops.heads_sliced_build_into(heads['s'][0], heads['t'][0], heads['q'][0])
    assert usable
    sl = dict(heads)
    sl['sliced'] = image
    for fwd in (True, False):
        v0 = v.clone()
        vt, ld, s, t, q = ops.vnet_heads_vupdate_sliced_tape(z, image, heads['s'][1], heads['s'][2], heads['t'][1],
                                                             nw[1], heads['q'][1], heads['q'][2], v0, f, 0.07, fwd)
        assert torch.equal(v0, v)                                                   # out of place
        vb = v.clone(); lb = ops.vnet_heads_vupdate_(z, sl, nw, vb, f, 0.07, fwd)   # inference instance
        # (not bit for bit: hipcc contracts the update's multiply-adds differently in the two instances)
        assert float((vt - vb).abs().max()) < 4e-15 * max(1.0, float(vb.abs().max()))
        assert err(host(ld), host(lb)) < 1e-13
        # the heads as forward_train forms them: scale * exp(coeff) * tanh(z W^T + b), coeff = log(c)
        s_ref = ops.gemm(z, heads['s'][0], heads['s'][1], coeff=torch.log(heads['s'][2]), scale=1.0, act='tanh')
        t_ref = ops.gemm(z, heads['t'][0], heads['t'][1], scale=nw[1])
        q_ref = ops.gemm(z, heads['q'][0], heads['q'][1], coeff=torch.log(heads['q'][2]), scale=1.0, act='tanh')
        for got, want in ((s, s_ref), (t, t_ref), (q, q_ref)):
            assert float((got - want).abs().max()) < 5e-15 * max(1.0, float(want.abs().max()))
        # and the update from them is the v_update kernel's
        v2, l2 = ops.v_update(v, f, s, t, q, 0.07, fwd)
        assert float((v2 - vt).abs().max()) < 2e-14 and err(host(l2), host(ld)) < 1e-12


@pytest.mark.parametrize('lat', [(2, 3, 2, 4), (4, 4, 4, 4), (3, 5, 2, 7)])
def test_su3_unpack_select_equals_select_then_unpack(lat):
    """l2q_su3_unpack_select: the accept / reject select fused into the native -> reference transpose is
    bit-identical to l2q_select_rows followed by l2q_su3_unpack (all-accept, all-reject and mixed masks)."""
    from l2hmc import _ops as ops
    V = int(np.prod(lat))
    nb = 5
    g = torch.Generator().manual_seed(3)
    a = torch.randn(nb, 4, 9, V, dtype=torch.complex128, generator=g).cuda()
    b = torch.randn(nb, 4, 9, V, dtype=torch.complex128, generator=g).cuda()
    for mask in ([1, 0, 1, 1, 0], [0] * 5, [1] * 5):
        m = torch.tensor(mask, dtype=torch.float32, device='cuda')
        ref = ops.su3_unpack(ops.select_rows(a.reshape(nb, -1), b.reshape(nb, -1), m).reshape(a.shape), lat)
        got = ops.su3_unpack_select(a, b, m, lat)
        assert got.shape == ref.shape and torch.equal(got, ref)
