"""GPU tier of the SU(3) per-link truth tests: the per-link kernels of csrc/su3_kernels.hip (through l2hmc._ops and
native.call) and the Python wrappers around them against mpmath at 60 digits (tests/su3_truth.py).

Fields are filled from 16-matrix pools by ``pool[(7 f + 13 s) % 16]`` at V in {1, 255, 256, 257, 513} (one below, at
and one above a 256-thread block and a multiple of one) with nb in {1, 3} chains or nf in {1, 5, 12} fields, so that
the launch indexing (f = blockIdx / nblk, mu = f & 3, the mask offset mu 9 V, the vec8 offset (f 8 + a) V) is
checked off the goldens' shapes.

Tolerances (u = 2^-53; none is tuned against the kernels):
  expm_mul     every entry of exp(eps v) x within B = K u max(1, |A|_F) max(1, max|exp A|), A = eps v, of truth --
               the bound of expm itself, K (and the tighter K of the anti-Hermitian classes) as in
               test_su3_group_host.py; the masked update keeps some entries of x and multiplies the rest, which is
               no larger
  expm_mul2    the second half-update multiplies the first one's error by E as well:
               B (1 + max_i sum_k |E_ik|)
  unitarity    check_su of exp(A) x, A anti-Hermitian and traceless, x unitary: <= 2 B   (E = E0 + d)
  reversibility  3 B
  projections  per class max(4 x the class-maximum error of oracle.su3 (the reference's closed form) against truth,
               32 u), computed here; the oracle's own error is asserted below 1e-10
  vec8 of an updated link   the near-unitary projection tolerance plus 7 B: the update's own error d (|d|_F <= 3 B)
               passes through the polar projection, which does not expand distances at a unitary point, and then
               through su3_to_vec, whose rows have absolute sum <= 4 / sqrt(3):  3 B 4 / sqrt(3) < 7 B
  products     entrywise 8 u (|a| |b|)_ij;  TAH 4 u max|x|;  assemble_tah 8 u x the sum of the moduli of an entry's
               terms;  reductions 64 u sum|terms| against math.fsum
"""
import math

import numpy as np
import pytest
import torch

import su3_truth as T
from oracle import su3 as osu3

pytestmark = pytest.mark.gpu

U = T.U
# measured by `python tests/su3_truth.py --measure`: worst ratio of torch.matrix_exp 43.13 (class nilpotent_30;
# every other class is below 10.1)
EXPM_TORCH_RATIO = 43.13
EXPM_K = 4 * EXPM_TORCH_RATIO
# A second, tighter bound by the same recipe for the anti-Hermitian classes alone -- normal matrices, what the
# trajectory feeds the kernel: there torch.matrix_exp's worst ratio is 10.09 (class alg_1)
EXPM_TORCH_RATIO_NORMAL = 10.09
EXPM_K_NORMAL = 4 * EXPM_TORCH_RATIO_NORMAL


def expm_k(name):
    return EXPM_K_NORMAL if name in T.EXPM_ANTIHERMITIAN else EXPM_K


VS = [1, 255, 256, 257, 513]
NBS = [1, 3]
NFS = [1, 5, 12]
EPS = 0.25                      # a power of two: A = eps v and v = A / eps are both exact


@pytest.fixture(scope='module')
def truth():
    """all pools and their mpmath truths, computed once for the module (about 15 s)"""
    t = T.Truth()
    for name in T.EXPM_CLASSES:
        t.expm(name, 1), t.expm(name, -1)
    for name in T.PROJ_CLASSES:
        t.polar_u(name), t.polar_su(name)
    t.unitary_su()
    return t


@pytest.fixture(scope='module')
def ops():
    from l2hmc import _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def adj(x):
    return np.conj(np.swapaxes(x, -1, -2))


def links(t, nf):
    """native [.., 9, V] tensor -> [nf, V, 3, 3] numpy"""
    a = host(t)
    return T.from_native(a.reshape(nf, 9, a.shape[-1]))


def native4(m, nb):
    """[nb * 4, V, 3, 3] numpy -> device tensor [nb, 4, 9, V]"""
    return dev(T.to_native(m)).reshape(nb, 4, 9, m.shape[1])


def expm_bound(truth, name, sign):
    a = truth.expm_pool(name)
    return expm_k(name) * T.expm_unit(a, truth.expm(name, sign))


def within(got, want, bound, what):
    """every link of got [nf, V, 3, 3] within bound [nf, V] (or scalar) of want, entry by entry"""
    err = np.abs(got.astype(T.CLD) - want).max((-2, -1)).astype(float)
    bad = err > bound
    assert not bad.any(), (what, f'worst err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3g}',
                           np.argwhere(bad)[:4].tolist())
    return float((err / np.maximum(bound, 1e-300)).max())


# ------------------------------------------------------------------------------------------- expm_mul
@pytest.mark.parametrize('V', VS)
@pytest.mark.parametrize('nb', NBS)
def test_expm_mul_unmasked(ops, truth, nb, V):
    nf = nb * 4
    idx = T.field_index(nf, V)
    xp = truth.unitary()
    xn = native4(xp[idx], nb)
    worst = 0.0
    for name in T.EXPM_CLASSES:
        a = truth.expm_pool(name)
        vn = native4((a / EPS)[idx], nb)
        for sign in (1, -1):
            want = (truth.expm(name, sign) @ xp.astype(T.CLD))[idx]
            got = links(ops.su3_expm_mul_n(xn, vn, sign * EPS), nf)
            worst = max(worst, within(got, want, expm_bound(truth, name, sign)[idx], (name, sign)))
    print(f'nb {nb} V {V}: worst err / bound {worst:.3f}')
    for name in ('alg_1e3', 'general_30', 'alg_1e-300'):
        vn = native4((truth.expm_pool(name) / EPS)[idx], nb)
        # eps = 0 returns x itself
        assert torch.equal(ops.su3_expm_mul_n(xn, vn, 0.0), xn), name
        # out aliasing xn, as the trajectory calls it: the same bits as out of place
        ref = ops.su3_expm_mul_n(xn, vn, EPS)
        xc = xn.clone()
        out = ops.su3_expm_mul_n(xc, vn, EPS, out=xc)
        assert out.data_ptr() == xc.data_ptr() and torch.equal(out, ref), name


def masks_entrywise(rng, V):
    """fp32 0/1, different per matrix entry, direction and site -> native [4, 9, V]"""
    return rng.integers(0, 2, size=(4, 9, V)).astype(np.float32)


def keep_links(mask, nb):
    """native mask [4, 9, V] -> keep [nb * 4, V, 3, 3] as the kernel reads it (mu = f & 3)"""
    k = np.moveaxis(mask, 1, 2).reshape(4, mask.shape[2], 3, 3).astype(np.float64)
    return np.tile(k, (nb, 1, 1, 1))


def half_update(e, x, keep):
    """keep (.) x + e @ ((1 - keep) (.) x) in long double"""
    return keep * x + np.einsum('fsik,fskj->fsij', e, (1 - keep) * x)


@pytest.mark.parametrize('V', VS)
@pytest.mark.parametrize('nb', NBS)
def test_expm_mul_masked_and_complement(ops, truth, nb, V):
    nf = nb * 4
    idx = T.field_index(nf, V)
    xl = truth.unitary()[idx]
    x = xl.astype(T.CLD)
    xn = native4(xl, nb)
    mask = masks_entrywise(np.random.default_rng(100 * nb + V), V)
    mn = dev(mask).reshape(-1)
    worst = 0.0
    for name in T.EXPM_CLASSES:
        vn = native4((truth.expm_pool(name) / EPS)[idx], nb)
        for sign, comp in ((1, False), (-1, True), (1, True)):
            k = keep_links(mask, nb)
            keep = 1 - k if comp else k
            want = half_update(truth.expm(name, sign)[idx], x, keep)
            got = links(ops.su3_expm_mul_n(xn, vn, sign * EPS, mn, comp), nf)
            worst = max(worst, within(got, want, expm_bound(truth, name, sign)[idx], (name, sign, comp)))
            # a column that is kept whole is x itself, bit for bit
            col = np.broadcast_to(keep.min(-2, keepdims=True) == 1, got.shape)
            assert np.array_equal(got[col], xl[col]), (name, sign, comp)
    print(f'nb {nb} V {V}: worst err / bound {worst:.3f}')


@pytest.mark.parametrize('V', VS)
@pytest.mark.parametrize('nb', NBS)
def test_expm_mul2_and_vec8(ops, truth, nb, V):
    nf = nb * 4
    idx = T.field_index(nf, V)
    xp = truth.unitary()
    x = xp[idx].astype(T.CLD)
    xn = native4(xp[idx], nb)
    rng = np.random.default_rng(200 * nb + V)
    mask = masks_entrywise(rng, V)
    mn = dev(mask).reshape(-1)
    # per-link masks (all nine entries alike, different per direction and site): both half-updates together
    # apply exp(eps v) to the whole link, so x' = E x stays unitary and its projection has a pool-sized truth
    mask_l = np.repeat(rng.integers(0, 2, size=(4, 1, V)), 9, axis=1).astype(np.float32)
    ml = dev(mask_l).reshape(-1)
    near = 'near_unitary_1e-15'
    e8 = float(T.maxerr(osu3.group_to_vec(truth.proj_pool(near)), T.vec8(truth.polar_su(near))).max())
    assert e8 < 1e-10
    tol8 = max(4 * e8, 32 * U)
    # E is unitary with det 1 to within u |A|_F (the structured classes are anti-Hermitian and traceless only to
    # rounding), far inside 7 B, so polar_su(E x) = E polar_su(x)
    su_x = truth.unitary_su()
    worst = worst8 = 0.0
    for name in T.EXPM_CLASSES:
        vn = native4((truth.expm_pool(name) / EPS)[idx], nb)
        for sign, comp in ((1, False), (-1, True)):
            e = truth.expm(name, sign)
            b = expm_bound(truth, name, sign)
            b2 = (b * (1 + np.abs(e).sum(-1).max(-1).astype(float)))[idx]
            k = keep_links(mask, nb)
            k1 = 1 - k if comp else k
            want = half_update(e[idx], half_update(e[idx], x, k1), 1 - k1)
            x2 = ops.su3_expm_mul2_n(xn, vn, sign * EPS, mn, comp)
            worst = max(worst, within(links(x2, nf), want, b2, (name, sign, comp)))
            xf, vf = ops.su3_expm_mul2_vec8_n(xn, vn, sign * EPS, mn, comp)
            within(links(xf, nf), want, b2, (name, sign, comp, 'vec8 variant'))
            # in place, as the trajectory calls it
            xc = xn.clone()
            xo, vo = ops.su3_expm_mul2_vec8_n(xc, vn, sign * EPS, mn, comp, out=xc)
            assert xo.data_ptr() == xc.data_ptr() and torch.equal(xo, xf), (name, sign, comp)
            if name not in T.EXPM_ANTIHERMITIAN_TRACELESS:
                continue              # exp of a general matrix is outside the projection's domain (up to e^50)
            assert bool(((vo == vf) | (vo.isnan() & vf.isnan())).all()), (name, sign, comp)
            xl, vl = ops.su3_expm_mul2_vec8_n(xn, vn, sign * EPS, ml, comp)
            within(links(xl, nf), (e @ xp.astype(T.CLD))[idx], b2, (name, sign, comp, 'per-link mask'))
            want8 = T.vec8(e @ su_x)[idx]                                    # [nf, V, 8]
            err8 = np.abs(np.moveaxis(host(vl).reshape(nf, 8, V), 1, 2) - want8).max(-1).astype(float)
            bound8 = tol8 + 7 * b[idx]
            assert (err8 <= bound8).all(), (name, sign, comp, float((err8 / bound8).max()))
            worst8 = max(worst8, float((err8 / bound8).max()))
    print(f'nb {nb} V {V}: worst err / bound: links {worst:.3f}, vec8 {worst8:.3f}')


@pytest.mark.parametrize('V', VS)
@pytest.mark.parametrize('nb', NBS)
def test_expm_mul_reversible_and_unitary(ops, truth, nb, V):
    nf = nb * 4
    idx = T.field_index(nf, V)
    xp = truth.unitary()
    xn = native4(xp[idx], nb)
    worst = worst_u = 0.0
    for name in T.EXPM_ANTIHERMITIAN:
        vn = native4((truth.expm_pool(name) / EPS)[idx], nb)
        b = expm_bound(truth, name, 1)
        x1 = ops.su3_expm_mul_n(xn, vn, EPS)
        back = links(ops.su3_expm_mul_n(x1, vn, -EPS), nf)
        worst = max(worst, within(back, xp[idx].astype(T.CLD), 3 * b[idx], name))
        if name in T.EXPM_ANTIHERMITIAN_TRACELESS:
            chk = host(ops.su3_check_su_n(x1))                        # [nb, 2]: (average, maximum) per chain
            bmax = b[idx].reshape(nb, -1).max(-1)
            assert (chk[:, 1] <= 2 * bmax).all() and (chk[:, 0] <= chk[:, 1]).all(), (name, chk, bmax)
            worst_u = max(worst_u, float((chk[:, 1] / (2 * bmax)).max()))
    print(f'nb {nb} V {V}: worst / bound: reversibility {worst:.3f}, unitarity {worst_u:.3f}')


# ------------------------------------------------------------------------------------------- projections
@pytest.mark.parametrize('V', VS)
@pytest.mark.parametrize('nf', NFS)
def test_projections(ops, truth, nf, V):
    idx = T.field_index(nf, V)
    for name in T.PROJ_CLASSES:
        pool = truth.proj_pool(name)
        xn = dev(T.to_native(pool[idx]))                                # [nf, 9, V]
        got = links(ops.su3_project_su_n(xn), nf)
        within(got, truth.polar_su(name)[idx], truth.proj_tol(name, True), (name, 'project_su'))
        got = links(ops.su3_project_u_n(xn), nf)
        within(got, truth.polar_u(name)[idx], truth.proj_tol(name, False), (name, 'project_u'))
        ref8 = T.vec8(truth.polar_su(name))
        e8 = float(T.maxerr(osu3.group_to_vec(pool), ref8).max())
        assert e8 < 1e-10, (name, e8)
        v = np.moveaxis(host(ops.su3_projsu_vec8_n(xn)), 1, 2)           # [nf, V, 8]
        err8 = float(np.abs(v - ref8[idx]).max())
        assert err8 <= max(4 * e8, 32 * U), (name, 'projsu_vec8', err8, e8)


def check_su_numpy(x, nb):
    """(average, maximum) per chain of the reference's checkSU measure, in long double with math.fsum"""
    x = x.astype(T.CLD)
    d = (np.abs(adj(x) @ x - np.eye(3)) ** 2).sum((-2, -1)) + np.abs(osu3.det3(x) - 1) ** 2
    d = d.reshape(nb, -1)
    return np.array([[math.sqrt(math.fsum(float(t) for t in c) / c.size / 20.0), math.sqrt(float(c.max()) / 20.0)]
                     for c in d])


@pytest.mark.parametrize('V', VS)
@pytest.mark.parametrize('nb', NBS)
def test_check_su(ops, truth, nb, V):
    """check_su of a projected field against its numpy value: both sides form x^H x - 1 and det x - 1 with an
    error of at most 8 u per entry (a 3-term complex dot product of entries <= 1), so the two 10-component
    deviation vectors differ by at most sqrt(10) 16 u in norm and the measures, norms over sqrt(20), by < 12 u.
    Of a field that is NOT unitary the measure is large and must agree to the reduction's 64 u relative, plus that
    same absolute term scaled by the size of the entries' products."""
    nf = nb * 4
    idx = T.field_index(nf, V)
    for name in T.PROJ_CLASSES:
        x = truth.proj_pool(name)[idx]
        xn = native4(x, nb)
        pn = ops.su3_project_su_n(xn)
        got = host(ops.su3_check_su_n(pn))
        assert np.abs(got - check_su_numpy(links(pn, nf), nb)).max() <= 12 * U, name
        want = check_su_numpy(x, nb)
        f = float(T.fro(x).max())
        got = host(ops.su3_check_su_n(xn))
        assert (np.abs(got - want) <= 64 * U * want + 12 * U * max(1.0, f ** 2, f ** 3)).all(), (name, got, want)


# ------------------------------------------------------------------------------------------- TAH, momenta
@pytest.mark.parametrize('V', VS)
@pytest.mark.parametrize('nf', NFS)
def test_project_tah(ops, truth, nf, V):
    idx = T.field_index(nf, V)
    for name in ('general_0.8', 'general_30', 'gaussian', 'sigma_1e3_2e3_5e2', 'alg_1'):
        pool = truth.expm_pool(name) if name in T.EXPM_CLASSES else truth.proj_pool(name)
        got = links(ops.su3_project_tah_n(dev(T.to_native(pool[idx]))), nf)
        within(got, T.tah(pool)[idx], (4 * U * np.abs(pool).max((-2, -1)))[idx], name)
        assert np.array_equal(got.real, -np.swapaxes(got.real, -1, -2))
        assert np.array_equal(got.imag, np.swapaxes(got.imag, -1, -2))


def assemble_truth(n):
    """normals [8, nf, V] -> (matrix [nf, V, 3, 3] clongdouble, sum of the moduli of each entry's terms)"""
    n = n.astype(T.LD)
    h = np.sqrt(T.LD(0.5))
    r3, r8 = h * n[0], h * n[1] / np.sqrt(T.LD(3))
    r01, r02, r12, i01, i02, i12 = (h * n[k] for k in range(2, 8))
    m = np.zeros(n.shape[1:] + (3, 3), dtype=T.CLD)
    s = np.zeros(n.shape[1:] + (3, 3), dtype=float)
    j = T.CLD(1j)
    m[..., 0, 0], m[..., 1, 1], m[..., 2, 2] = j * (r8 + r3), j * (r8 - r3), j * (-2 * r8)
    s[..., 0, 0] = s[..., 1, 1] = np.abs(r8) + np.abs(r3)
    s[..., 2, 2] = 2 * np.abs(r8)
    for (a, b), re, im in (((0, 1), r01, i01), ((0, 2), r02, i02), ((1, 2), r12, i12)):
        m[..., a, b], m[..., b, a] = re + j * im, -re + j * im
        s[..., a, b] = s[..., b, a] = np.maximum(np.abs(re), np.abs(im))
    return m, s


@pytest.mark.parametrize('V', VS)
@pytest.mark.parametrize('nf', NFS)
def test_assemble_tah(ops, nf, V):
    rng = np.random.default_rng(300 * nf + V)
    n = rng.normal(size=(8, nf, V))
    got = links(ops.su3_assemble_tah_n(dev(n)), nf)
    want, terms = assemble_truth(n)
    assert (np.abs(got.astype(T.CLD) - want) <= 8 * U * terms).all()
    # anti-Hermitian bit for bit in the entries the kernel writes as negations, the diagonal purely imaginary
    assert np.array_equal(got.real, -np.swapaxes(got.real, -1, -2))
    assert np.array_equal(got.imag, np.swapaxes(got.imag, -1, -2))
    tr = np.einsum('fsii->fs', got)
    assert (np.abs(tr) <= 8 * U * np.einsum('fsii->fs', terms)).all()


@pytest.mark.parametrize('V', VS)
@pytest.mark.parametrize('nb', NBS)
def test_kinetic_reduce(ops, nb, V):
    rng = np.random.default_rng(400 * nb + V)
    vn = ops.su3_assemble_tah_n(dev(rng.normal(size=(8, nb, 4, V))))          # [nb, 4, 9, V]
    got = host(ops.su3_kinetic_n(vn))
    p = host(vn).reshape(nb, -1)
    for c in range(nb):
        terms = [float(t) for t in np.concatenate([p[c].real.astype(T.LD) ** 2, p[c].imag.astype(T.LD) ** 2])]
        want = 0.5 * (math.fsum(terms) - 8.0 * 4 * V)
        assert abs(got[c] - want) <= 64 * U * (0.5 * math.fsum(terms) + 16.0 * V), (c, got[c], want)


# ------------------------------------------------------------------------------------------- products
@pytest.mark.parametrize('V', VS)
@pytest.mark.parametrize('nf', NFS)
def test_mul(ops, truth, nf, V):
    """all four adjoint combinations on non-Hermitian, non-symmetric Gaussians; b is read three pool places on
    from a, so a kernel that pairs the wrong links shows as well"""
    idx = T.field_index(nf, V)
    a, b = truth.expm_pool('general_3'), np.roll(truth.proj_pool('gaussian'), 3, axis=0)
    an, bn = dev(T.to_native(a[idx])), dev(T.to_native(b[idx]))
    for adj_a in (False, True):
        for adj_b in (False, True):
            want = T.mul(a, b, adj_a, adj_b)
            aa, bb = np.abs(adj(a) if adj_a else a), np.abs(adj(b) if adj_b else b)
            got = links(ops.su3_mul_n(an, bn, adj_a, adj_b), nf)
            assert (np.abs(got.astype(T.CLD) - want[idx]) <= 8 * U * (aa @ bb)[idx]).all(), (adj_a, adj_b)


# ------------------------------------------------------------------------------------------- Python wrappers
def test_group_wrappers(truth):
    """SU3.mul with every flag pair and the group's project_u / project_su through reference-layout tensors
    [nb, 4, T, X, Y, Z, 3, 3]: covers the _native / _reference conversions around the kernels"""
    from l2hmc.group.su3.pytorch.group import SU3
    nb, L = 2, (2, 3, 2, 4)
    V = int(np.prod(L))
    nf = nb * 4
    idx = T.field_index(nf, V)
    shape = (nb, 4, *L, 3, 3)
    g = SU3()

    def ref(m):
        return dev(np.ascontiguousarray(m[idx].astype(complex)).reshape(shape))

    def back(t):
        assert tuple(t.shape) == shape
        return host(t).reshape(nf, V, 3, 3)
    a, b = truth.expm_pool('general_3'), np.roll(truth.proj_pool('gaussian'), 3, axis=0)
    for adj_a in (False, True):
        for adj_b in (False, True):
            want = T.mul(a, b, adj_a, adj_b)
            aa, bb = np.abs(adj(a) if adj_a else a), np.abs(adj(b) if adj_b else b)
            got = back(g.mul(ref(a), ref(b), adj_a, adj_b))
            assert (np.abs(got.astype(T.CLD) - want[idx]) <= 8 * U * (aa @ bb)[idx]).all(), (adj_a, adj_b)
    for name in ('gaussian', 'sigma_2_2_0.5', 'near_unitary_1e-8'):
        x = ref(truth.proj_pool(name))
        within(back(g.projectSU(x)), truth.polar_su(name)[idx], truth.proj_tol(name, True), (name, 'projectSU'))
        within(back(g.projectU(x)), truth.polar_u(name)[idx], truth.proj_tol(name, False), (name, 'projectU'))
