"""CPU tier for the trimmed per-link arithmetic of csrc/su3_math.hpp: the early exit of m3_expm's coefficient
loop and m3_project_su_vec8 (Hermitian products, only the entries su3_to_vec reads, phase from det x), through
tests/native_host/link_math_valu/link_math_valu.cpp built for the host under AddressSanitizer + UBSan.  That
program carries the replaced forms -- the 20-step loop run to its end, the projection on full products -- as
yardsticks and runs both on the same input in one process.

  expm   BIT FOR BIT equal to the 20-step loop (the exit criterion is a proof, see the comment in m3_expm) on every
         pool of su3_truth.EXPM_CLASSES (both signs), on 20 000 seeded Gaussian complex matrices at each of ten
         Frobenius norms from 1e-3 to 30 (both sides of the 0.5 scaling threshold), on the zero matrix and on a
         matrix with a NaN entry; and the mean number of steps at |A|_F = 0.03 is below 12 of 20, so a criterion
         that never fires fails.
  vec8   against mpmath truth within the class tolerance of the projection tests, max(4 x the class-maximum error
         of oracle.su3 against truth, 32 u) (tests/test_su3_group_gpu.py::test_projections), on every pool of
         su3_truth.PROJ_CLASSES.  The yardstick's class-maximum error is printed next to the new routine's.
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
NORMS = [1e-3, 0.01, 0.03, 0.1, 0.3, 0.49, 0.51, 1.0, 3.0, 30.0]
NRAND = 20000


@pytest.fixture(scope='module')
def truth():
    return T.Truth()


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """run(lines) -> one list of floats per input line, through ONE process of the sanitised driver"""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = tmp_path_factory.mktemp('link_math_valu') / 'link_math_valu_san'
    src = os.path.join(ROOT, 'tests', 'native_host', 'link_math_valu', 'link_math_valu.cpp')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'tests', 'native_host'), '-I', os.path.join(ROOT, 'l2hmc-qcd_amd', 'csrc'),
                    src, '-o', str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input='\n'.join(lines) + '\n', capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        assert r.stderr == '', r.stderr[-2000:]
        out = [[float(x) for x in ln.split()] for ln in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def op_line(op, m):
    vals = []
    for z in np.asarray(m, dtype=complex).reshape(-1):
        vals += [repr(float(z.real)), repr(float(z.imag))]
    return op + ' ' + ' '.join(vals)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def run_expm(host, mats):
    out = np.array(host([op_line('expm', m) for m in mats]))
    return out[:, :18], out[:, 18:36], out[:, 36]


@pytest.mark.parametrize('name', T.EXPM_CLASSES)
def test_expm_pools_bit_identical(host, truth, name):
    a = truth.expm_pool(name)
    new, ref, steps = run_expm(host, list(a) + list(-a))
    print(f'{name}: steps min {steps.min():.0f} mean {steps.mean():.2f} max {steps.max():.0f}')
    assert same_bits(new, ref), (name, np.argwhere(new != ref)[:4].tolist())
    assert ((steps >= 1) & (steps <= 20)).all()


def test_expm_random_bit_identical_and_exits_early(host):
    out = host([f'rand {norm!r} {NRAND} {1000 + k}' for k, norm in enumerate(NORMS)])
    for norm, (entries, differ, far, mean_steps) in zip(NORMS, out):
        print(f'|A|_F = {norm:g}: {entries:.0f} entries, {differ:.0f} differ, {far:.0f} by more than 1 ulp, '
              f'mean steps {mean_steps:.2f} of 20')
    for norm, (entries, differ, far, mean_steps) in zip(NORMS, out):
        assert entries == 18 * NRAND
        assert differ == 0 and far == 0, (norm, differ, far)
    assert out[NORMS.index(0.03)][3] < 12.0


def test_expm_zero_and_nan(host):
    zero = np.zeros((3, 3), complex)
    nan = np.random.default_rng(5).normal(size=(3, 3)) * 0.02 + 0j
    nan[1, 2] = complex(float('nan'), 0.3)
    new, ref, steps = run_expm(host, [zero, nan])
    assert same_bits(new, ref)
    assert np.array_equal(new[0].reshape(9, 2), np.stack([np.eye(3).reshape(-1), np.zeros(9)], 1))
    assert steps[0] == 1                       # all terms are zero after the first step: nothing can follow
    assert np.isnan(new[1]).all() and steps[1] == 20      # a NaN never passes the exit test


@pytest.mark.parametrize('name', T.PROJ_CLASSES)
def test_project_su_vec8_against_truth(host, truth, name):
    x = truth.proj_pool(name)
    ref8 = T.vec8(truth.polar_su(name))
    e8 = float(T.maxerr(osu3.group_to_vec(x), ref8).max())
    assert e8 < 1e-10, (name, e8)
    tol8 = max(4 * e8, 32 * U)
    out = np.array(host([op_line('vec8', m) for m in x]))
    err_new = T.maxerr(out[:, :8], ref8)
    err_old = T.maxerr(out[:, 8:], ref8)
    print(f'{name} vec8: new err {err_new.max():.3e}  full-product form {err_old.max():.3e}  tol {tol8:.3e}')
    assert (err_new <= tol8).all(), (name, err_new.max(), tol8)
