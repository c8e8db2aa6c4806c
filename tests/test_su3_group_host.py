"""CPU tier of the SU(3) per-link truth tests: csrc/su3_math.hpp compiled for the host (stub <hip/hip_runtime.h> of
tests/native_host/) under AddressSanitizer + UBSan as a stand-alone executable, every input pool of
tests/su3_truth.py run through it and compared with mpmath at 60 digits.

Tolerances (u = 2^-53; none is tuned against the header):
  expm         err <= K u max(1, |A|_F) max(1, max|exp A|) per matrix, K = 4 x the worst value of that ratio that
               torch.matrix_exp (CPU, complex128) shows against the same truth over all pools
               (`python tests/su3_truth.py --measure`); the anti-Hermitian classes are held to the tighter K the same
               recipe gives over them alone
  unitarity    max|E^H E - 1| <= 2 x the expm bound for anti-Hermitian A      (E = E0 + d)
  reversibility  max|exp(A) exp(-A) - 1| <= 3 x the expm bound, anti-Hermitian A
  projections  per class max(4 x the class-maximum error of oracle.su3 (the reference's closed form) against truth,
               32 u), computed here, with the oracle's own error asserted below 1e-10
  products     entrywise 8 u (|a| |b|)_ij;   TAH: 4 u max|x|
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import su3_truth as T
from oracle import su3 as osu3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


@pytest.fixture(scope='module')
def truth():
    return T.Truth()


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """run(op, pool[, pool2]) -> [16, ...] through ONE process of the sanitised driver"""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = tmp_path_factory.mktemp('su3_group_host') / 'link_math_san'
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'tests', 'native_host'), '-I', os.path.join(ROOT, 'l2hmc-qcd_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'native_host', 'link_math.cpp'), '-o', str(exe)], check=True)

    def run(op, *pools):
        lines = []
        for k in range(len(pools[0])):
            vals = []
            for p in pools:
                for z in np.asarray(p[k], dtype=complex).reshape(-1):
                    vals += [repr(float(z.real)), repr(float(z.imag))]
            lines.append(op + ' ' + ' '.join(vals))
        r = subprocess.run([str(exe)], input='\n'.join(lines) + '\n', capture_output=True, text=True)
        assert r.returncode == 0, (op, r.returncode, r.stderr[-2000:])
        assert r.stderr == '', r.stderr[-2000:]
        v = np.array([float(x) for x in r.stdout.split()])
        if op == 'vec8':
            return v.reshape(len(pools[0]), 8)
        v = v.reshape(len(pools[0]), 9, 2)
        return (v[..., 0] + 1j * v[..., 1]).reshape(-1, 3, 3)
    return run


def adj(x):
    return np.conj(np.swapaxes(x, -1, -2))


@pytest.mark.parametrize('name', T.EXPM_CLASSES)
def test_expm_against_truth(host, truth, name):
    a = truth.expm_pool(name)
    eye = np.eye(3)
    got = {}
    for sign in (1, -1):
        e = truth.expm(name, sign)
        got[sign] = host('expm', sign * a)
        bound = expm_k(name) * T.expm_unit(a, e)
        ratio = T.maxerr(got[sign], e) / T.expm_unit(a, e)
        print(f'{name} sign {sign:+d}: worst err / unit = {ratio.max():.3f} (K = {expm_k(name):.1f})')
        assert (T.maxerr(got[sign], e) <= bound).all(), (name, sign, ratio)
        if name in T.EXPM_ANTIHERMITIAN:
            g = got[sign].astype(T.CLD)
            assert (T.maxerr(adj(g) @ g, eye) <= 2 * bound).all(), (name, sign)
    if name in T.EXPM_ANTIHERMITIAN:
        bound = expm_k(name) * T.expm_unit(a, truth.expm(name, 1))
        assert (T.maxerr(got[1].astype(T.CLD) @ got[-1].astype(T.CLD), eye) <= 3 * bound).all(), name
    if name == 'alg_0':
        assert np.array_equal(got[1], np.broadcast_to(eye, got[1].shape))


def test_expm_threshold_pools_straddle_the_boundary(truth):
    """the classes meant to sit on the scaling threshold and on the frexp boundaries really do: element 0 of the
    power-of-two pools has that Frobenius norm exactly, and the 0.5 (1 + 2^-52) pool lies above 0.5"""
    for key in ('0.5', '1', '2', '4'):
        a = truth.expm_pool('alg_' + key)[0]
        assert float((a.real ** 2 + a.imag ** 2).sum()) == float(key) ** 2
    n = T.fro(truth.expm_pool('alg_0.5+ulp'))
    assert (n > 0.5).any() and (n < 0.5 * (1 + 2.0 ** -50)).all()
    assert (T.fro(truth.expm_pool('alg_1e-300')) ** 2 == 0.0).all()        # the squares underflow


@pytest.mark.parametrize('name', T.PROJ_CLASSES)
def test_projections_against_truth(host, truth, name):
    x = truth.proj_pool(name)
    for op, ref, su in (('projsu', truth.polar_su(name), True), ('proju', truth.polar_u(name), False)):
        tol = truth.proj_tol(name, su)
        err = T.maxerr(host(op, x), ref)
        print(f'{name} {op}: err {err.max():.3e}  tol {tol:.3e}')
        assert (err <= tol).all(), (name, op, err.max(), tol)
    ref8 = T.vec8(truth.polar_su(name))
    e8 = float(T.maxerr(osu3.group_to_vec(x), ref8).max())
    assert e8 < 1e-10, (name, e8)
    tol8 = max(4 * e8, 32 * U)
    err = T.maxerr(host('vec8', x), ref8)
    print(f'{name} vec8: err {err.max():.3e}  tol {tol8:.3e}')
    assert (err <= tol8).all(), (name, err.max(), tol8)


@pytest.mark.parametrize('name', ['general_0.8', 'general_30', 'gaussian', 'sigma_1e3_2e3_5e2', 'alg_1'])
def test_tah_against_truth(host, truth, name):
    x = truth.expm_pool(name) if name in T.EXPM_CLASSES else truth.proj_pool(name)
    got = host('tah', x)
    assert (T.maxerr(got, T.tah(x)) <= 4 * U * np.abs(x).max((-2, -1))).all(), name
    # anti-Hermitian bit for bit: the real part antisymmetric (zero diagonal), the imaginary part symmetric
    assert np.array_equal(got.real, -np.swapaxes(got.real, -1, -2))
    assert np.array_equal(got.imag, np.swapaxes(got.imag, -1, -2))


@pytest.mark.parametrize('adj_a,adj_b', [(False, False), (False, True), (True, False), (True, True)])
def test_products_against_truth(host, truth, adj_a, adj_b):
    """non-Hermitian, non-symmetric Gaussians: transpose, conjugate and adjoint are all distinguishable"""
    a, b = truth.expm_pool('general_3'), truth.proj_pool('gaussian')
    got = host('mul_' + 'na'[adj_a] + 'na'[adj_b], a, b)
    ref = T.mul(a, b, adj_a, adj_b)
    aa, bb = np.abs(adj(a) if adj_a else a), np.abs(adj(b) if adj_b else b)
    assert (np.abs(got.astype(T.CLD) - ref) <= 8 * U * (aa @ bb)).all()
    # the other three combinations are far away: the check can tell them apart
    for oa in (False, True):
        for ob in (False, True):
            if (oa, ob) != (adj_a, adj_b):
                assert float(T.maxerr(T.mul(a, b, oa, ob), ref).min()) > 1e-3
