"""Activation digit images (csrc/digits.hpp) and the sliced input layer that takes them (csrc/gemm_digits.hip):
the producers write exactly the integer recoding of their fp64 outputs, and the layer has the bits of
l2q_gemm_sliced_f64."""
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


def host(t):
    return t.detach().cpu().numpy()


def recode(v, e=2):
    """fp64 [m, k] -> uint8 [m, k / 64, 7, 64]: X = rint(v 2^(54 - e)) in balanced base 256, digit planes 0 (top)
    .. 6, the 64 k of a slab at byte 16 g + 2 j + i for k = 8 j + 2 g + i (the k-order of the weight images).
    Integer arithmetic: exact."""
    m, k = v.shape
    x = np.rint(np.ldexp(v, 54 - e)).astype(np.int64)
    planes = np.empty((7, m, k), dtype=np.int64)
    for s in range(6, -1, -1):
        d = ((x + 128) & 255) - 128
        planes[s] = d
        x = (x - d) >> 8
    assert not x.any()
    kk = np.arange(64)
    pos = 16 * ((kk >> 1) & 3) + 2 * (kk >> 3) + (kk & 1)
    out = np.empty((m, k // 64, 7, 64), dtype=np.int8)
    out[..., pos] = np.moveaxis(planes.reshape(7, m, k // 64, 64), 0, 2)
    return out.view(np.uint8)


def links(rng, nb, L):
    x = osu3.project_su(rng.normal(size=(nb, 4, *L, 3, 3)) + 1j * rng.normal(size=(nb, 4, *L, 3, 3)))
    return x


@pytest.mark.parametrize('L', [(2, 2, 4, 4), (4, 4, 4, 4)], ids=['V64', 'V256'])
@pytest.mark.parametrize('nb', [3, 64])
def test_projection_digits_are_exact(ops, L, nb):
    rng = np.random.default_rng(5)
    # general matrices near SU(3): the projection has work to do
    x = links(rng, nb, L) + 0.05 * (rng.normal(size=(nb, 4, *L, 3, 3)) + 1j * rng.normal(size=(nb, 4, *L, 3, 3)))
    xn = ops.su3_pack(dev(x))
    vec = host(ops.su3_projsu_vec8_n(xn)).reshape(nb, -1)
    img = ops.su3_projsu_digits_n(xn)
    assert img is not None and img.shape == vec.shape and img.exp == 2
    assert np.array_equal(host(img.buf), recode(vec))


def test_slicer_digits_are_exact(ops):
    rng = np.random.default_rng(6)
    a = rng.uniform(-2.3, 2.3, size=(70, 320))
    a[0, :8] = [0.0, -0.0, 3.999999, -3.999999, 2.0 ** -52, -2.0 ** -53, 1.5 * 2.0 ** -52, 0.5 - 2.0 ** -54]
    a[1, :4] = [2.0 ** -30, -(2.0 ** -29), 127.5 * 2.0 ** -52, -128.5 * 2.0 ** -52]       # digit carries
    img = ops.gemm_digits_slice(dev(a))
    assert np.array_equal(host(img.buf), recode(a))
    img8 = ops.gemm_digits_slice(dev(a), a_exp=8)
    assert np.array_equal(host(img8.buf), recode(a, 8))
    assert ops.gemm_digits_slice(dev(a[:, :100])) is None                                  # K % 64


def test_x_update_digits(ops):
    rng = np.random.default_rng(7)
    L, nb, eps = (2, 2, 4, 4), 3, 0.07
    V = int(np.prod(L))
    xn = ops.su3_pack(dev(links(rng, nb, L)))
    vn = ops.su3_pack(dev(osu3.rand_tah3(rng.normal(size=(8, nb, 4, *L)))))
    m = dev(rng.integers(0, 2, size=(4, 9, V)).astype(np.float32))
    m[:] = m[:, :1]                                              # one mask value per link
    ones = torch.zeros_like(m)                                   # keep nothing: the unmasked update
    for mask in (m, ones):
        for comp in (False, True):
            xf, vf = ops.su3_expm_mul2_vec8_n(xn, vn, eps, mask, comp)
            xd, img = ops.su3_expm_mul2_digits_n(xn, vn, eps, mask, comp)
            assert torch.equal(xf, xd)
            assert np.array_equal(host(img.buf), recode(host(vf).reshape(nb, -1)))
    xc = xn.clone()
    xo, img = ops.su3_expm_mul2_digits_n(xc, vn, eps, m, True, out=xc)
    xf, vf = ops.su3_expm_mul2_vec8_n(xn, vn, eps, m, True)
    assert xo.data_ptr() == xc.data_ptr() and torch.equal(xo, xf)
    assert np.array_equal(host(img.buf), recode(host(vf).reshape(nb, -1)))
    # a lattice the producers do not serve: declined, nothing launched
    x6 = ops.su3_pack(dev(links(rng, 2, (2, 2, 2, 6))))
    assert ops.su3_projsu_digits_n(x6) is None
    assert ops.su3_expm_mul2_digits_n(x6, x6, eps, torch.zeros(4, 9, 48, dtype=torch.float32, device='cuda'),
                                      False) is None


@pytest.mark.parametrize('shape', [(64, 64, 4096, 0), (128, 64, 8192, 4096), (64, 128, 40960, 0)])
def test_gemm_digits_has_the_bits_of_gemm_sliced(ops, shape):
    m, n, k, k2 = shape
    rng = np.random.default_rng(12)
    a = dev(rng.uniform(-2.3, 2.3, size=(m, k)))
    w = dev(rng.uniform(-1, 1, size=(n, k)) / np.sqrt(k))
    a[3, 5] = 0.0
    a[1, 7] = -3.999
    b1 = dev(0.1 * rng.normal(size=n)); b2 = dev(0.1 * rng.normal(size=n)) if k2 else None
    a2 = dev(rng.uniform(-2.3, 2.3, size=(m, k2))) if k2 else None
    w2 = dev(rng.uniform(-1, 1, size=(n, k2)) / np.sqrt(k2)) if k2 else None
    img = ops.gemm_sliced_build(w)
    img2 = ops.gemm_sliced_build(w2) if k2 else None
    coeff = dev(0.2 * rng.normal(size=n))
    da = ops.gemm_digits_slice(a)
    da2 = ops.gemm_digits_slice(a2) if k2 else None
    for act, co, sc in ((None, None, 1.0), ('tanh', None, 1.0), ('leaky_relu', coeff, 0.7), ('swish', None, 1.3),
                        ('relu', None, 1.0), ('elu', coeff, 1.0)):
        want = ops.gemm_sliced(a, img, n, b1, a2=a2, image2=img2, bias2=b2, coeff=co, scale=sc, act=act)
        got = ops.gemm_digits(da, img, n, b1, a2=da2, image2=img2, bias2=b2, coeff=co, scale=sc, act=act)
        assert bool(torch.isfinite(got).all())
        assert torch.equal(got, want), act
    want = ops.gemm_sliced(a, img, n, None, a2=a2, image2=img2)
    assert torch.equal(ops.gemm_digits(da, img, n, None, a2=da2, image2=img2), want)


def test_producer_flag_poisons_the_layer_once(ops):
    rng = np.random.default_rng(9)
    L, nb, n = (2, 2, 4, 4), 64, 64
    V = int(np.prod(L))
    x = links(rng, nb, L)
    w = dev(rng.uniform(-1, 1, size=(n, 32 * V)) / np.sqrt(32 * V))
    img = ops.gemm_sliced_build(w)
    b = dev(0.1 * rng.normal(size=n))
    good = ops.su3_pack(dev(x))
    clean = ops.gemm_digits(ops.su3_projsu_digits_n(good), img, n, b, act='tanh')
    assert bool(torch.isfinite(clean).all())
    # the projection: a NaN entry of one link
    xb = good.clone()
    xb[5, 2, 4, 17] = float('nan')
    out = ops.gemm_digits(ops.su3_projsu_digits_n(xb), img, n, b, act='tanh')
    assert bool(torch.isnan(out).all())
    assert torch.equal(ops.gemm_digits(ops.su3_projsu_digits_n(good), img, n, b, act='tanh'), clean)
    # the x-update: a NaN momentum
    vn = ops.su3_pack(dev(osu3.rand_tah3(rng.normal(size=(8, nb, 4, *L)))))
    mask = torch.zeros(4, 9, V, dtype=torch.float32, device='cuda')
    vb = vn.clone()
    vb[7, 1, 0, 3] = float('nan')
    _, di = ops.su3_expm_mul2_digits_n(good, vb, 0.05, mask, False)
    assert bool(torch.isnan(ops.gemm_digits(di, img, n, b)).all())
    _, di = ops.su3_expm_mul2_digits_n(good, vn, 0.05, mask, False)
    assert bool(torch.isfinite(ops.gemm_digits(di, img, n, b)).all())
    # the slicer: a value at the edge of the declared range
    a = dev(rng.uniform(-2.3, 2.3, size=(nb, 32 * V)))
    for bad in (4.0, -4.5, float('nan'), float('inf')):
        ab = a.clone()
        ab[2, 100] = bad
        assert bool(torch.isnan(ops.gemm_digits(ops.gemm_digits_slice(ab), img, n, b)).all()), bad
        assert bool(torch.isfinite(ops.gemm_digits(ops.gemm_digits_slice(a), img, n, b)).all())


def test_gemm_digits_long_groups(ops):
    """Workgroups whose k-group spans more than one int32 range (16 384 k): the shared slab loop folds the group sums
    into fp64 after slab 256 and runs on.  256 x 256 x 278 528 (= 17 x 16 384) has k-groups of 17 408, the smallest
    such shape at this tile count; the workspace size pins the k-grouping so the flush stays reached."""
    from l2hmc import native as N
    m, n, k = 256, 256, 17 * 16384
    assert int(N.load().l2q_gemm_sliced_ws_bytes(m, n, k, 0)) == 16 * m * n * 8 + 512
    g = torch.Generator(device='cuda').manual_seed(4)
    a = (torch.rand(m, k, dtype=torch.float64, device='cuda', generator=g) - 0.5) * 4.6
    w = (torch.rand(n, k, dtype=torch.float64, device='cuda', generator=g) - 0.5) * (2.0 / k ** 0.5)
    b = 0.1 * torch.randn(n, dtype=torch.float64, device='cuda', generator=g)
    img = ops.gemm_sliced_build(w)
    assert img is not None
    want = ops.gemm_sliced(a, img, n, b)
    got = ops.gemm_digits(ops.gemm_digits_slice(a), img, n, b)
    assert torch.equal(got, want)
    ref = ops.gemm(a, w, b)
    assert float((got - ref).abs().max()) < 5e-13 * max(1.0, float(ref.abs().max()))
