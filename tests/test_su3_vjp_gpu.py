"""GPU tier of the SU(3) per-link VJP truth tests: the reverse-mode kernels of csrc/su3_train_kernels.hip
(l2q_su3_expm_mul_bwd, l2q_su3_expm_mul2_bwd, l2q_su3_projsu_vec8_bwd, through l2hmc._ops as training.py calls them)
against mpmath at 60 digits (tests/su3_truth.py): the Frechet derivative as the upper-right block of
mp.expm([[B, G], [0, B]]), the projection VJP as central differences of the mp.eigh polar projection.

Every pool place k holds one triple (x_k, A_k = eps v_k, g_k); fields are filled by ``pool[(7 f + 13 s) % 16]`` at V in
{1, 255, 256, 257, 513} with nb in {1, 3} chains or nf in {1, 5, 12} fields, so that a tail block, a full block,
one past it and a multi-block field stand behind f = blockIdx / nblk, mu = f & 3, the mask offset (mu 9 + i) V + s,
the gvec offset (f 8 + a) V + s, the per-thread LDS stash and the partial[blockIdx] -> deps[chain] reduction.  The
accumulating outputs (g_v, g_M) start from a non-zero pooled field.  Masks differ per entry, direction and site, so a
masked direction g y^H differs from link to link: it is combined in long double from the nine basis responses
L[e_ab] of the pool matrix (L is complex-linear).

Tolerances (u = 2^-53; none is tuned against the kernels).  B = (eps v)^H is the argument of the derivative, E =
exp(eps v), Bx = K u max(1, |B|_F) max(1, max|E|) the forward expm bound of test_su3_group_gpu.py, and
F = K_L u max(1, |B|_F) max(1, max|E|) the Frechet bound per unit |G|_F, K_L = 4 x the worst ratio that
torch.autograd.grad over torch.matrix_exp (CPU, complex128) shows against the same truth
(`python tests/su3_truth.py --measure`), the anti-Hermitian classes under the tighter K_L of their own:
  g_x          entry (i, j) of keep (.) g + (1 - keep) (.) (E^H g) within Bx sum_k |g_kj|
  g_v          every entry of the increment eps g_A within |eps| (F + 8 u |L|) |g|_F |y|_F + 2 u |g_v0|: the kernel
               rounds the direction g y^H (8 u |g|_F |y|_F, through L, whose norm |L| is bounded by the Frobenius
               norm of its 9x9 matrix) and the accumulation rounds once more
  deps[c]      against math.fsum of Re tr(g_A^H v) over the chain: the sum over its links of
               3 (F + 8 u |L|) |g|_F |y|_F |v|_F  (|Re tr(d^H v)| <= |d|_F |v|_F <= 3 max|d| |v|_F) plus the
               reduction's 64 u sum |g_A,ij| |v_ij|
  mul2         the same three with G = g y2^H + g' y1^H, |G|_F <= |g|_F |y2|_F + |g'|_F |y1|_F, times the
               (1 + max_i sum_k |E_ik|) of the forward expm_mul2 bound: the second half sees the first one's error
               through E
  projection   every entry of the increment within K_P u |g_y|_2 (sigma_max / sigma_min) / sigma_min + 2 u |g_M0|;
               K_P = max(4 x the worst class ratio of the numpy fp64 restatement
               su3_truth.projsu_vec8_vjp_numpy against truth, 32), see test_su3_vjp_host.py

Wall time on an MI355X host: 52.5 s for the 55 tests, 40.6 s of it the truth fixture (computed once); the slowest
test takes 1.2 s.
"""
import math
import time

import numpy as np
import pytest
import torch

import su3_truth as T

pytestmark = pytest.mark.gpu

U = T.U
# measured by `python tests/su3_truth.py --measure` (the constants of test_su3_vjp_host.py)
EXPM_K = 4 * 43.13
EXPM_K_NORMAL = 4 * 10.09
FRECHET_TORCH_RATIO = 103.352
FRECHET_K = 4 * FRECHET_TORCH_RATIO
FRECHET_TORCH_RATIO_NORMAL = 11.136
FRECHET_K_NORMAL = 4 * FRECHET_TORCH_RATIO_NORMAL
PROJ_NUMPY_RATIO = 21.082
PROJ_K = max(4 * PROJ_NUMPY_RATIO, 32.0)

VS = [1, 255, 256, 257, 513]
NBS = [1, 3]
NFS = [1, 5, 12]
EPS = 0.25                      # a power of two: A = eps v and v = A / eps are both exact
CLD = T.CLD


def expm_k(name):
    return EXPM_K_NORMAL if name in T.EXPM_ANTIHERMITIAN else EXPM_K


def frechet_k(name):
    return FRECHET_K_NORMAL if name in T.EXPM_ANTIHERMITIAN else FRECHET_K


@pytest.fixture(scope='module')
def truth():
    """all pools and their mpmath truths, computed once for the module"""
    t0 = time.time()
    t = T.Truth()
    for name in T.BASIS_CLASSES:
        t.frechet_basis(name)
    for name in T.EXPM_CLASSES:
        for sign in (1, -1):
            t.expm(name, sign), t.expm_vjp(name, sign), t.frechet_norm(name, sign)
    for name in T.PROJ_VJP_CLASSES:
        t.projsu_vec8_vjp(name)
    print(f'truth fixture: {time.time() - t0:.1f} s')
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


def masks_entrywise(rng, V):
    """fp32 0/1, different per matrix entry, direction and site -> native [4, 9, V]"""
    return rng.integers(0, 2, size=(4, 9, V)).astype(np.float32)


def keep_links(mask, nb):
    """native mask [4, 9, V] -> keep [nb * 4, V, 3, 3] as the kernel reads it (mu = f & 3)"""
    k = np.moveaxis(mask, 1, 2).reshape(4, mask.shape[2], 3, 3).astype(np.float64)
    return np.tile(k, (nb, 1, 1, 1))


def within(got, want, bound, what):
    """every entry of got within bound (broadcast against it) of want; -> worst err / bound"""
    assert np.isfinite(got).all(), (what, 'not finite')
    err = np.abs(got.astype(CLD) - want).astype(float)
    bound = np.broadcast_to(bound, err.shape)
    ratio = float((err / np.maximum(bound, 1e-320)).max())
    bad = err > bound
    assert not bad.any(), (what, f'worst err / bound {ratio:.3g}', np.argwhere(bad)[:4].tolist())
    return ratio


def mm(a, b):
    return np.einsum('...ik,...kj->...ij', a, b)


class Case:
    """the fields of one (class, sign, nb, V) and the pool-level pieces of the bounds"""

    def __init__(self, truth, name, sign, nb, V):
        self.name, self.sign, self.nb, self.nf, self.V = name, sign, nb, nb * 4, V
        self.idx = idx = T.field_index(self.nf, V)
        a = truth.expm_pool(name)
        e = truth.expm(name, sign)
        self.x, self.g, self.acc = truth.unitary()[idx], truth.cotangent()[idx], truth.accumulator()[idx]
        self.v = (a / EPS)[idx]
        self.e = e[idx]
        unit = T.expm_unit(a, e)
        self.bx = (expm_k(name) * unit)[idx]                                            # [nf, V]
        self.fl = (frechet_k(name) * unit + 8 * U * truth.frechet_norm(name, sign))[idx]  # F + 8 u |L|
        self.m2 = (1 + np.abs(e).sum(-1).max(-1).astype(float))[idx]
        self.xn, self.gn, self.vn = (native4(t, nb) for t in (self.x, self.g, self.v))
        self.gv0 = native4(self.acc, nb)
        self.vf = T.fro(self.v)

    def check(self, what, gx, gv, deps, gx_want, ga, gnorm, factor=1.0):
        """gx, gv, deps of one kernel call against g_x = gx_want, g_A = ga [nf, V, 3, 3] (long double) and
        |G|_F <= gnorm [nf, V]; factor: the mul2 factor"""
        nf, nb = self.nf, self.nb
        colsum = np.abs(self.g).sum(-2)[..., None, :]
        r_x = within(links(gx, nf), gx_want, (self.bx * factor)[..., None, None] * colsum, (what, 'gx'))
        b_a = self.fl * gnorm * factor                                                  # on every entry of g_A
        gv_want = self.acc.astype(CLD) + CLD(self.sign * EPS) * ga
        r_v = within(links(gv, nf), gv_want, EPS * b_a[..., None, None] + 2 * U * np.abs(self.acc), (what, 'gv'))
        terms = (np.conj(ga) * self.v.astype(CLD)).real.sum((-2, -1)).astype(float).reshape(nb, -1)
        mods = (np.abs(ga) * np.abs(self.v)).sum((-2, -1)).astype(float).reshape(nb, -1)
        slack = (3 * b_a * self.vf).reshape(nb, -1)
        got = host(deps)
        r_e = 0.0
        for c in range(nb):
            want = math.fsum(terms[c])
            bound = math.fsum(slack[c]) + 64 * U * math.fsum(mods[c])
            assert math.isfinite(got[c]) and abs(got[c] - want) <= bound, (what, 'deps', c, got[c], want, bound)
            r_e = max(r_e, abs(got[c] - want) / max(bound, 1e-320))
        return max(r_x, r_v, r_e)


# ------------------------------------------------------------------------------------------- expm_mul_bwd
@pytest.mark.parametrize('V', VS)
@pytest.mark.parametrize('nb', NBS)
def test_expm_mul_bwd_unmasked(ops, truth, nb, V):
    """every expm class, both signs: y = x, one direction g_k x_k^H per pool triple"""
    worst = 0.0
    for name in T.EXPM_CLASSES:
        for sign in (1, -1):
            c = Case(truth, name, sign, nb, V)
            gv = c.gv0.clone()
            gx, deps = ops.su3_expm_mul_bwd_n(c.xn, c.vn, sign * EPS, None, False, c.gn, gv)
            ga = truth.expm_vjp(name, sign)[c.idx]
            worst = max(worst, c.check((name, sign), gx, gv, deps, mm(adj(c.e), c.g.astype(CLD)), ga,
                                       T.fro(c.g) * T.fro(c.x)))
    print(f'nb {nb} V {V}: worst err / bound {worst:.3f}')


@pytest.mark.parametrize('V', VS)
@pytest.mark.parametrize('nb', NBS)
def test_expm_mul_bwd_masked_and_complement(ops, truth, nb, V):
    mask = masks_entrywise(np.random.default_rng(500 * nb + V), V)
    mn = dev(mask).reshape(-1)
    worst = 0.0
    for name in T.BASIS_CLASSES:
        for sign in (1, -1):
            c = Case(truth, name, sign, nb, V)
            basis = truth.frechet_basis(name, sign)[c.idx]
            for comp in (False, True):
                k = keep_links(mask, nb)
                keep = 1 - k if comp else k
                y = (1 - keep) * c.x
                gd = mm(c.g.astype(CLD), adj(y))                                   # g y^H, long double
                gx_want = keep * c.g + (1 - keep) * mm(adj(c.e), c.g.astype(CLD))
                gv = c.gv0.clone()
                gx, deps = ops.su3_expm_mul_bwd_n(c.xn, c.vn, sign * EPS, mn, comp, c.gn, gv)
                worst = max(worst, c.check((name, sign, comp), gx, gv, deps, gx_want, T.combine(basis, gd),
                                           T.fro(c.g) * T.fro(y)))
    print(f'nb {nb} V {V}: worst err / bound {worst:.3f}')


@pytest.mark.parametrize('V', VS)
@pytest.mark.parametrize('nb', NBS)
def test_expm_mul_bwd_zero_step_and_determinism(ops, truth, nb, V):
    """what the trajectory's tape relies on: eps = 0 hands g through bit for bit wherever keep is 0 or 1 (here
    everywhere), and a second call on the same inputs returns the same bits, deps included"""
    mask = masks_entrywise(np.random.default_rng(600 * nb + V), V)
    mn = dev(mask).reshape(-1)
    for name in ('alg_1e3', 'general_3', 'alg_1e-300'):
        c = Case(truth, name, 1, nb, V)
        for m, comp in ((None, False), (mn, False), (mn, True)):
            gv = c.gv0.clone()
            gx, deps = ops.su3_expm_mul_bwd_n(c.xn, c.vn, 0.0, m, comp, c.gn, gv)
            assert torch.equal(gx, c.gn), (name, comp)
            out = []
            for _ in range(2):
                gv = c.gv0.clone()
                gx, deps = ops.su3_expm_mul_bwd_n(c.xn, c.vn, -EPS, m, comp, c.gn, gv)
                out.append((gx, gv, deps))
            for a, b in zip(*out):
                assert torch.equal(a, b), (name, comp)
        gv = [c.gv0.clone(), c.gv0.clone()]
        out = [ops.su3_expm_mul2_bwd_n(c.xn, c.vn, EPS, mn, True, c.gn, gv[i]) for i in range(2)]
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and torch.equal(*gv), name


# ------------------------------------------------------------------------------------------- expm_mul2_bwd
@pytest.mark.parametrize('V', VS)
@pytest.mark.parametrize('nb', NBS)
def test_expm_mul2_bwd(ops, truth, nb, V):
    """both half-updates through one derivative: the truth of the two chained halves, the direction
    g y2^H + g' y1^H formed in long double from the truth E"""
    mask = masks_entrywise(np.random.default_rng(700 * nb + V), V)
    mn = dev(mask).reshape(-1)
    worst = 0.0
    for name in T.BASIS_CLASSES:
        for sign in (1, -1):
            c = Case(truth, name, sign, nb, V)
            basis = truth.frechet_basis(name, sign)[c.idx]
            g, eh = c.g.astype(CLD), adj(c.e)
            for comp in (False, True):
                k = keep_links(mask, nb)
                k1 = 1 - k if comp else k
                y1 = (1 - k1) * c.x
                y2 = k1 * (k1 * c.x + mm(c.e, y1.astype(CLD)))                     # (1 - k2) (.) x'
                g1 = (1 - k1) * g + k1 * mm(eh, g)                                 # g' = k2 g + (1 - k2) E^H g
                gx_want = k1 * g1 + (1 - k1) * mm(eh, g1)
                gd = mm(g, adj(y2)) + mm(g1, adj(y1))
                gnorm = T.fro(g) * T.fro(y2) + T.fro(g1) * T.fro(y1)
                gv = c.gv0.clone()
                gx, deps = ops.su3_expm_mul2_bwd_n(c.xn, c.vn, sign * EPS, mn, comp, c.gn, gv)
                worst = max(worst, c.check((name, sign, comp), gx, gv, deps, gx_want, T.combine(basis, gd),
                                           gnorm.astype(float), factor=c.m2))
    print(f'nb {nb} V {V}: worst err / bound {worst:.3f}')


# ------------------------------------------------------------------------------------------- projsu_vec8_bwd
@pytest.mark.parametrize('V', VS)
@pytest.mark.parametrize('nf', NFS)
def test_projsu_vec8_bwd(ops, truth, nf, V):
    """every projection class and exactly unitary links, as training.py calls the kernel on the links x (the
    unitary classes) and on the force (tah_gaussian); at nf = 12 with its shapes: fields [nb, 4, 9, V] and the
    cotangent flat per chain"""
    idx = T.field_index(nf, V)
    shape = (nf // 4, 4, 9, V) if nf % 4 == 0 else (nf, 9, V)
    acc = truth.accumulator()[idx]
    gvec = dev(np.moveaxis(truth.vec8_cotangent()[idx], 1, 2))                     # [nf, 8, V]
    if nf % 4 == 0:
        gvec = gvec.reshape(nf // 4, -1)
    worst = 0.0
    for name in T.PROJ_VJP_CLASSES:
        mn = dev(T.to_native(truth.proj_pool(name)[idx])).reshape(shape)
        gm = dev(T.to_native(acc)).reshape(shape)
        out = ops.su3_projsu_vec8_bwd_(gm, mn, gvec)
        assert out.data_ptr() == gm.data_ptr()
        want = acc.astype(CLD) + truth.projsu_vec8_vjp(name)[idx]
        bound = PROJ_K * truth.proj_vjp_unit(name)[idx][..., None, None] + 2 * U * np.abs(acc)
        worst = max(worst, within(links(gm, nf), want, bound, name))
    print(f'nf {nf} V {V}: worst err / bound {worst:.3f}')
