"""GPU tier for the trimmed per-link arithmetic of csrc/su3_math.hpp (early exit of m3_expm's coefficient loop,
m3_project_su_vec8): the x-update with vec8 and with digits and the projection kernels at V = 64 and V = 192 with
one chain (one and three wavefronts per field, the smallest lattices the digit path accepts), on fields whose
neighbouring lanes hold eps v of Frobenius norm 0, 1e-3, 0.03, 0.49, 0.51 and 30 in turn -- the lanes of one
wavefront leave the loop at different steps and some take squarings.

Truth is mpmath at 60 digits (tests/su3_truth.py); the bounds are those of tests/test_su3_group_gpu.py, u = 2^-53:
  links of the double half-update   B (1 + max_i sum_k |E_ik|),  B = K u max(1, |A|_F) max(1, max|exp A|), K the
                                    anti-Hermitian K of the expm tests (A = eps v is anti-Hermitian here)
  vec8 of an updated link           the near-unitary class tolerance max(4 x the oracle's class-maximum error,
                                    32 u) plus 7 B
  projections of the updated links  the near-unitary class tolerance plus 3 x the links' bound: the polar
                                    projection does not expand Frobenius distances at a unitary point, and a
                                    3x3 entrywise bound b is a Frobenius bound 3 b
The digit images must be the integer recoding of the fp64 vec8 output of the same launch arguments, byte for
byte (x-update: su3_expm_mul2_digits against su3_expm_mul2_vec8; projection: su3_projsu_digits against
su3_projsu_vec8), and su3_projsu_vec8 of the stored links must be the vec8 the x-update emitted for them.
"""
import numpy as np
import pytest
import torch

import su3_truth as T
from oracle import su3 as osu3

pytestmark = pytest.mark.gpu

U = T.U
EXPM_K_NORMAL = 4 * 10.09         # tests/test_su3_group_gpu.py: 4 x torch.matrix_exp's worst ratio, anti-Hermitian
EPS = 0.25                        # a power of two: A = eps v and v = A / eps are both exact
NORMS = [0.0, 1e-3, 0.03, 0.49, 0.51, 30.0]
NPOOL = 24                        # four matrices per norm; pool index k has norm NORMS[k % 6]
NEAR = 'near_unitary_1e-15'


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def recode(v, e=2):
    """fp64 [m, k] -> uint8 [m, k / 64, 7, 64]: rint(v 2^(54 - e)) in balanced base 256, digit planes 0 (top) .. 6,
    the 64 k of a slab at byte 16 g + 2 j + i for k = 8 j + 2 g + i (tests/test_gemm_digits_gpu.py)"""
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


@pytest.fixture(scope='module')
def ops():
    from l2hmc import _ops
    return _ops


@pytest.fixture(scope='module')
def ref():
    """pools and their truths, once for the module"""
    rng = np.random.default_rng(20240)
    v = osu3.project_tah(rng.normal(size=(NPOOL, 3, 3)) + 1j * rng.normal(size=(NPOOL, 3, 3)))
    norm = np.array([NORMS[k % len(NORMS)] for k in range(NPOOL)])
    a = v * (norm / T.fro(v))[:, None, None]
    t = T.Truth()
    x = t.unitary()
    e8 = float(T.maxerr(osu3.group_to_vec(t.proj_pool(NEAR)), T.vec8(t.polar_su(NEAR))).max())
    assert e8 < 1e-10
    e = T.expm(a)
    return {'a': a, 'e': e, 'b': EXPM_K_NORMAL * T.expm_unit(a, e), 'x': x, 'su_x': t.unitary_su(),
            'u_x': T.polar_u(x), 'tol8': max(4 * e8, 32 * U), 'tol_su': t.proj_tol(NEAR, True),
            'tol_u': t.proj_tol(NEAR, False)}


def links(tn, nf):
    a = host(tn)
    return T.from_native(a.reshape(nf, 9, a.shape[-1]))


def maxerr_links(got, want):
    return np.abs(got.astype(T.CLD) - want).max((-2, -1)).astype(float)


@pytest.mark.parametrize('V', [64, 192])
def test_mixed_norm_wavefronts(ops, ref, V):
    nb, nf = 1, 4
    f, s = np.meshgrid(np.arange(nf), np.arange(V), indexing='ij')
    ia = (5 * f + s) % NPOOL                     # neighbouring lanes: different norms
    ix = T.field_index(nf, V)
    assert len({NORMS[k % 6] for k in ia[0, :64]}) == len(NORMS)
    xn = dev(T.to_native(ref['x'][ix])).reshape(nb, 4, 9, V)
    vn = dev(T.to_native((ref['a'] / EPS)[ia])).reshape(nb, 4, 9, V)
    # per-link masks (all nine entries alike): both half-updates together apply exp(eps v) to the whole link
    rng = np.random.default_rng(V)
    mask = dev(np.repeat(rng.integers(0, 2, size=(4, 1, V)), 9, axis=1).astype(np.float32)).reshape(-1)
    e = ref['e'][ia]
    b = ref['b'][ia]
    b2 = b * (1 + np.abs(ref['e']).sum(-1).max(-1).astype(float)[ia])
    want = e @ ref['x'].astype(T.CLD)[ix]
    want_su = e @ ref['su_x'][ix]
    want_u = e @ ref['u_x'][ix]
    want8 = T.vec8(want_su)                                           # [nf, V, 8]
    for comp in (False, True):
        x2 = ops.su3_expm_mul2_n(xn, vn, EPS, mask, comp)
        err = maxerr_links(links(x2, nf), want)
        print(f'V {V} comp {comp}: links worst err / bound {float((err / b2).max()):.3f}')
        assert (err <= b2).all(), (comp, float((err / b2).max()), np.argwhere(err > b2)[:4].tolist())
        xf, vf = ops.su3_expm_mul2_vec8_n(xn, vn, EPS, mask, comp)
        assert torch.equal(xf, x2), comp
        err8 = np.abs(np.moveaxis(host(vf).reshape(nf, 8, V), 1, 2) - want8).max(-1).astype(float)
        bound8 = ref['tol8'] + 7 * b
        print(f'V {V} comp {comp}: vec8 worst err / bound {float((err8 / bound8).max()):.3f}')
        assert (err8 <= bound8).all(), (comp, float((err8 / bound8).max()))
        xd, img = ops.su3_expm_mul2_digits_n(xn, vn, EPS, mask, comp)
        assert torch.equal(xd, x2), comp
        assert np.array_equal(host(img.buf), recode(host(vf).reshape(nb, -1))), comp
        # the projection kernels on the stored links: vec8 against truth, the digits of that vec8, the matrices
        pv = ops.su3_projsu_vec8_n(x2)
        errp8 = np.abs(np.moveaxis(host(pv).reshape(nf, 8, V), 1, 2) - want8).max(-1).astype(float)
        print(f'V {V} comp {comp}: projsu_vec8 worst err / bound {float((errp8 / bound8).max()):.3f}')
        assert (errp8 <= bound8).all(), (comp, float((errp8 / bound8).max()))
        pimg = ops.su3_projsu_digits_n(x2)
        assert np.array_equal(host(pimg.buf), recode(host(pv).reshape(nb, -1))), comp
        # and the vec8 the x-update emitted for the link it stored (Dynamics.reuse_v_inputs relies on it)
        assert torch.equal(pv, vf), comp
        for got, truth, tol, what in ((ops.su3_project_su_n(x2), want_su, ref['tol_su'], 'project_su'),
                                      (ops.su3_project_u_n(x2), want_u, ref['tol_u'], 'project_u')):
            errp = maxerr_links(links(got, nf), truth)
            boundp = tol + 3 * b2
            print(f'V {V} comp {comp}: {what} worst err / bound {float((errp / boundp).max()):.3f}')
            assert (errp <= boundp).all(), (comp, what, float((errp / boundp).max()))
