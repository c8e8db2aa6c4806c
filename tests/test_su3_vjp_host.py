"""CPU tier of the SU(3) per-link VJP truth tests: csrc/su3_train_math.hpp compiled for the host (stub
<hip/hip_runtime.h> of tests/native_host/, built the way test_native_host.py builds it), all 16 matrices of every
input class of tests/su3_truth.py run through m3_expm_frechet, m3_expm_frechet_series and m3_projsu_vec8_vjp and
compared with mpmath at 60 digits: the Frechet derivative as the upper-right block of mp.expm([[B, G], [0, B]]), the
projection VJP as central differences (step 1e-20) of the mp.eigh polar projection.

Tolerances (u = 2^-53; none is tuned against the header):
  Frechet      max|L - L_exp(B)[G]| <= K_L u max(1, |B|_F) max(1, max|exp B|) |G|_F per matrix, K_L = 4 x the worst
               value of that ratio that torch.autograd.grad over torch.matrix_exp (CPU, complex128) shows against
               the same truth over all pools and both signs (`python tests/su3_truth.py --measure`); the
               anti-Hermitian classes are held to the tighter K_L the same recipe gives over them alone.  The
               factor 4 is the forward tests' margin for a differently ordered fp64 evaluation.
  E beside L   the forward expm bound of test_su3_group_host.py, K u max(1, |B|_F) max(1, max|exp B|)
  projection   max|g_M - truth| <= K_P u |g_y|_2 (sigma_max / sigma_min) / sigma_min per matrix: the polar
               factor's derivative norm ~ 1 / sigma_min times the conditioning of the eigenproblem.  K_P =
               max(4 x the worst class ratio of a plain numpy fp64 restatement of the derivative
               (su3_truth.projsu_vec8_vjp_numpy, numpy.linalg.eigh) against truth, 32); `--measure` prints it and
               asserts that the restatement stays below 32 units on every class.  The floor 32 stands for the few
               tens of roundings of six Jacobi sweeps and six 3x3 products.  The reference's autograd cannot be
               the yardstick: it divides by eigenvalue gaps and is NaN or wrong on the degenerate classes.

Resolving power (measured on scratch copies of the header, one edit at a time): the file fails when dp1 loses its
p2 tr G term (the scalar and general classes), when the phase part of the projection VJP takes c / 2 for c / 3 (every
projection class), when the scalar recursion stops four terms early (n < 10: alg_0.25, alg_0.5, alg_1) and when the
scaling threshold is 1 instead of 0.25 (alg_1).  It does not fail, and no fp64 bound can make it fail, when the
recursion stops only two terms early (n < 12) or the threshold is 0.5: the two dropped terms are at most
0.25^12 / 12! |G| = 1.1 u |G| and every printed ratio stays the same to its last digit, and at |X|_F < 0.5 the 12
steps still leave 0.5^14 / 14! |G| = 6 u |G| (the worst ratio of alg_0.5 goes from 2.06 to 1.28, one squaring less).
Those two edits are not errors at this precision; the header has that much margin.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import su3_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = T.U

# measured by `python tests/su3_truth.py --measure`: worst ratio of torch.matrix_exp's forward error 43.13 (class
# nilpotent_30), 10.09 over the anti-Hermitian classes (the constants of test_su3_group_host.py)
EXPM_K = 4 * 43.13
EXPM_K_NORMAL = 4 * 10.09
# measured by the same command: worst ratio of torch.autograd.grad over torch.matrix_exp FRECHET_TORCH_RATIO
# (class nilpotent_30; every other class is below 15.7), over the anti-Hermitian classes FRECHET_TORCH_RATIO_NORMAL
# (class alg_0.5)
FRECHET_TORCH_RATIO = 103.352
FRECHET_K = 4 * FRECHET_TORCH_RATIO
FRECHET_TORCH_RATIO_NORMAL = 11.136
FRECHET_K_NORMAL = 4 * FRECHET_TORCH_RATIO_NORMAL
# measured by the same command: worst class ratio of the numpy restatement PROJ_NUMPY_RATIO (class
# near_unitary_1e-8)
PROJ_NUMPY_RATIO = 21.082
PROJ_K = max(4 * PROJ_NUMPY_RATIO, 32.0)


def expm_k(name):
    return EXPM_K_NORMAL if name in T.EXPM_ANTIHERMITIAN else EXPM_K


def frechet_k(name):
    return FRECHET_K_NORMAL if name in T.EXPM_ANTIHERMITIAN else FRECHET_K


@pytest.fixture(scope='module')
def truth():
    return T.Truth()


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """run(op, operand pools...) -> [16, n_out, 3, 3] through ONE process of the driver"""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = tmp_path_factory.mktemp('su3_vjp_host') / 'link_math'
    subprocess.run(['g++', '-O1', '-std=c++17', '-I', os.path.join(ROOT, 'tests', 'native_host'),
                    '-I', os.path.join(ROOT, 'l2hmc-qcd_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'native_host', 'link_math.cpp'), '-o', str(exe)], check=True)

    def run(op, *pools):
        lines = []
        for k in range(len(pools[0])):
            vals = []
            for p in pools:
                if np.iscomplexobj(p):
                    for z in np.asarray(p[k], dtype=complex).reshape(-1):
                        vals += [repr(float(z.real)), repr(float(z.imag))]
                else:
                    vals += [repr(float(t)) for t in np.asarray(p[k]).reshape(-1)]
            lines.append(op + ' ' + ' '.join(vals))
        r = subprocess.run([str(exe)], input='\n'.join(lines) + '\n', capture_output=True, text=True)
        assert r.returncode == 0, (op, r.returncode, r.stderr[-2000:])
        v = np.array([float(x) for x in r.stdout.split()]).reshape(len(pools[0]), -1, 9, 2)
        return (v[..., 0] + 1j * v[..., 1]).reshape(len(pools[0]), -1, 3, 3)
    return run


def adj(x):
    return np.conj(np.swapaxes(x, -1, -2))


@pytest.mark.parametrize('name', T.EXPM_CLASSES)
def test_frechet_against_truth(host, truth, name):
    """g_A = L_exp(A^H)[G], the call of the kernels: B = A^H, G the pooled fp64 direction g_k x_k^H"""
    b = adj(truth.expm_pool(name))
    g = truth.direction()
    e, l = truth.frechet_host(name)
    unit = T.expm_unit(b, e)
    for op in ('frechet', 'frechet_series'):
        got = host(op, b, g)
        re = T.maxerr(got[:, 0], e) / unit
        rl = T.maxerr(got[:, 1], l) / (unit * T.fro(g))
        print(f'{name} {op}: worst err / unit: L {rl.max():.3f} (K_L = {frechet_k(name):.1f}), '
              f'E {re.max():.3f} (K = {expm_k(name):.1f})')
        assert np.isfinite(got).all(), (name, op)
        assert (rl <= frechet_k(name)).all(), (name, op, rl)
        assert (re <= expm_k(name)).all(), (name, op, re)
    if name == 'alg_0':
        assert np.array_equal(got[:, 0], np.broadcast_to(np.eye(3), got[:, 0].shape))
        assert np.array_equal(got[:, 1], g)                     # L_exp(0) is the identity map


@pytest.mark.parametrize('name', T.PROJ_VJP_CLASSES)
def test_projsu_vec8_vjp_against_truth(host, truth, name):
    m = truth.proj_pool(name)
    gy = truth.vec8_cotangent()
    got = host('projsu_vjp', m, gy)[:, 0]
    assert np.isfinite(got).all(), name
    r = T.maxerr(got, truth.projsu_vec8_vjp(name)) / truth.proj_vjp_unit(name)
    print(f'{name}: worst err / unit {r.max():.3f} (K_P = {PROJ_K:.1f}), worst absolute '
          f'{T.maxerr(got, truth.projsu_vec8_vjp(name)).max():.3e}')
    assert (r <= PROJ_K).all(), (name, r)


def test_truths_agree_with_their_restatements(truth):
    """the yardstick's domain condition, on one cheap class each: the numpy restatement of the projection VJP
    stays below 32 units, and the basis responses combine to the directly computed Frechet derivative"""
    name = 'unitary'
    got = T.projsu_vec8_vjp_numpy(truth.proj_pool(name), truth.vec8_cotangent())
    assert (T.maxerr(got, truth.projsu_vec8_vjp(name)) < 32.0 * truth.proj_vjp_unit(name)).all()
    a, g = truth.expm_pool('general_3')[:2], truth.direction()[:2]
    plus, minus = T.frechet_basis(adj(a))
    for sign, basis in ((1, plus), (-1, minus)):
        e, l = (truth.frechet_host('general_3') if sign == 1 else T.expm_vjp(-a, g))
        assert float(T.maxerr(T.combine(basis, g), l[:2]).max()) <= 1e-17 * float(np.abs(l[:2]).max())
