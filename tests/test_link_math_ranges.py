"""CPU tier for the range-restricted arithmetic of the SU(3) projection (csrc/su3_math.hpp, L2Q_RANGED_MATH):
m_sincos_third on |t| <= pi / 3, the Newton reciprocal m_rcp and the coupled root m_sqrt_hrsq, built for the host
under AddressSanitizer + UBSan (tests/native_host/link_math_ranges/link_math_ranges.cpp) and compared with long
double on dense grids of the ranges they are called on; then the projection as a whole against mpmath truth with
the ranged routines on and off (the driver of tests/test_link_math_valu_host.py, compiled both ways).

Bounds, in ulp of the true value, from the routines' own construction (none is taken from what they returned):

  sincos   1 ulp.  The two polynomials are fdlibm's kernels (documented error below 2^-58 for sin, 2^-57 for cos,
           relative, on [-pi/4, pi/4]).  Each result is one rounding (0.5 ulp) of a sum whose small addend carries
           the earlier roundings: for the cosine series the rounding of z = u^2 enters through z / 2 with
           2^-54 z <= 0.31 ulp of a result in [0.7, 1); for the sine series the three roundings of z u p enter with
           |z u / 6| 3 2^-53 <= 0.24 ulp of a result in [0.5, 0.87] (less below 0.5: the term falls as u^3).  So 0.85
           at most, plus the polynomials' 0.03.  The fold adds nothing: uh = pio2_hi - |t| is exact and the low word
           of pi / 2 enters both series to first order (what it leaves, ul^2, is 2^-108).
  rcp      1 ulp: after two Newton steps the relative error is 2^-92, the third is a residual correction whose one
           rounding leaves at most half an ulp plus that.
  root     1 ulp for sqrt(x) (same argument: residual correction, one rounding).  h = 1 / (2 sqrt(x)) has no such
           correction and a coupled step does not correct roundings: those of g and h of the step before enter the
           residual r and with it the last h, then the last fma rounds -- three errors of up to 2^-53 relative, each
           up to one ulp of a value just above a power of two, and half an ulp for the last rounding: 4 ulp.
           (eigs3x3, its one user, takes a Newton step on what it forms from h.)
  The hardware estimates the host has not are replaced by the correctly rounded value cut to 24 bits, the
  accuracy class of v_rcp_f64 / v_rsq_f64 (2^29 ulp).

Accuracy condition of the projection: every class of su3_truth.PROJ_CLASSES stays within max(4 x the oracle's
error, 32 u), and its error does not grow by more than a factor of two against the library calls.
"""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import su3_truth as T
from oracle import su3 as osu3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = T.U
PI3 = math.pi / 3
NGRID = 2_000_001


def compile_host(out, src, *defs):
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    *defs, '-I', os.path.join(ROOT, 'tests', 'native_host'),
                    '-I', os.path.join(ROOT, 'l2hmc-qcd_amd', 'csrc'), src, '-o', str(out)], check=True)


def runner(exe):
    def run(lines):
        r = subprocess.run([str(exe)], input='\n'.join(lines) + '\n', capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        assert r.stderr == '', r.stderr[-2000:]
        out = [[float(x) for x in ln.split()] for ln in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    d = tmp_path_factory.mktemp('link_math_ranges')
    nh = os.path.join(ROOT, 'tests', 'native_host')
    compile_host(d / 'ranges', os.path.join(nh, 'link_math_ranges', 'link_math_ranges.cpp'))
    valu = os.path.join(nh, 'link_math_valu', 'link_math_valu.cpp')
    compile_host(d / 'valu_ranged', valu, '-DL2Q_RANGED_MATH=1')
    compile_host(d / 'valu_libm', valu, '-DL2Q_RANGED_MATH=0')
    return {k: runner(d / k) for k in ('ranges', 'valu_ranged', 'valu_libm')}


def test_sincos_on_its_range(host):
    run = host['ranges']
    (es, ec, ts, tc), = run([f'sincos {-PI3!r} {PI3!r} {NGRID}'])
    print(f'sincos on [-pi/3, pi/3], {NGRID} points: sin {es:.3f} ulp at {ts!r}, cos {ec:.3f} ulp at {tc!r}')
    assert es <= 1.0 and ec <= 1.0
    # both sides of the fold, dense: 2^20 points within 1e-9 of pi/4
    q = math.pi / 4
    for lo, hi in ((q - 1e-9, q + 1e-9), (-q - 1e-9, -q + 1e-9), (0.0, 1e-6), (PI3 - 1e-6, PI3)):
        (es, ec, _, _), = run([f'sincos {lo!r} {hi!r} {1 << 20}'])
        print(f'sincos on [{lo!r}, {hi!r}]: sin {es:.3f} ulp, cos {ec:.3f} ulp')
        assert es <= 1.0 and ec <= 1.0, (lo, hi)
    # the points the callers reach exactly: 0, the fold, the ends, a third of acos at its two clamps
    clamp = 1.0 - 1e-12
    pts = [0.0, -0.0, q, -q, np.nextafter(q, 1.0), np.nextafter(q, 0.0), PI3, -PI3,
           math.acos(clamp) / 3, math.acos(-clamp) / 3, 5e-324, 1e-300, 2.0 ** -27]
    out = run([f'sincos_at {float(t)!r}' for t in pts])
    for t, (es, ec, s, c) in zip(pts, out):
        assert es <= 1.0 and ec <= 1.0, (t, es, ec)
        assert math.copysign(1.0, s) == math.copysign(1.0, t) and c > 0.0, t
    assert out[0][2:] == [0.0, 1.0] and out[1][2:] == [0.0, 1.0]
    (_, _, s, c), = run(['sincos_at nan'])
    assert math.isnan(s) and math.isnan(c)


def test_reciprocal_and_roots(host):
    run = host['ranges']
    # d = w (se0 + se1) (se0 + se2) (se1 + se2) of the projection: sixth power of the singular-value scale, which
    # su3_truth keeps within 1e-20 .. 1e20; the roots see eigenvalues (its square) and q (its fourth power)
    (e, _, x, _), = run([f'rcp 1e-130 1e130 {NGRID}'])
    print(f'rcp on +-[1e-130, 1e130]: {e:.3f} ulp at {x!r}')
    assert e <= 1.0
    (eg, eh, xg, xh), = run([f'root 1e-90 1e90 {NGRID}'])
    print(f'root on [1e-90, 1e90]: sqrt {eg:.3f} ulp at {xg!r}, half reciprocal root {eh:.3f} ulp at {xh!r}')
    assert eg <= 1.0 and eh <= 4.0
    for lo, hi in ((0.5, 2.0), (1.0 - 1e-9, 1.0 + 1e-9), (3.999, 4.001)):
        (e, _, _, _), = run([f'rcp {lo!r} {hi!r} {1 << 20}'])
        (eg, eh, _, _), = run([f'root {lo!r} {hi!r} {1 << 20}'])
        assert e <= 1.0 and eg <= 1.0 and eh <= 4.0, (lo, hi)
    # what the division and the library root give at the ends of the number line
    out = run(['rcp_at 0.0', 'rcp_at -0.0', 'rcp_at inf', 'rcp_at -inf', 'rcp_at nan', 'rcp_at 1.0', 'rcp_at -4.0'])
    assert out[0] == [math.inf, math.inf] and out[1] == [-math.inf, -math.inf]
    assert out[2] == [0.0, 0.0] and math.copysign(1.0, out[3][0]) == -1.0 and out[3][0] == 0.0
    assert math.isnan(out[4][0]) and out[5] == [1.0, 1.0] and out[6] == [-0.25, -0.25]
    out = run(['root_at 0.0', 'root_at 1.0', 'root_at 4.0', 'root_at nan'])
    assert out[0] == [0.0, math.inf] and out[1] == [1.0, 0.5] and out[2] == [2.0, 0.25]
    assert math.isnan(out[3][0])


def op_line(op, m):
    vals = []
    for z in np.asarray(m, dtype=complex).reshape(-1):
        vals += [repr(float(z.real)), repr(float(z.imag))]
    return op + ' ' + ' '.join(vals)


@pytest.fixture(scope='module')
def truth():
    return T.Truth()


@pytest.mark.parametrize('name', T.PROJ_CLASSES)
def test_projection_classes_ranged_against_library_calls(host, truth, name):
    x = truth.proj_pool(name)
    ref8 = T.vec8(truth.polar_su(name))
    e8 = float(T.maxerr(osu3.group_to_vec(x), ref8).max())
    tol8 = max(4 * e8, 32 * U)
    lines = [op_line('vec8', m) for m in x]
    new = float(T.maxerr(np.array(host['valu_ranged'](lines))[:, :8], ref8).max())
    old = float(T.maxerr(np.array(host['valu_libm'](lines))[:, :8], ref8).max())
    print(f'{name} vec8: library calls {old:.3e}  ranged {new:.3e}  tol {tol8:.3e}')
    assert new <= tol8, (name, new, tol8)
    assert new <= 2.0 * old, (name, new, old)


def test_expm_every_second_step_is_the_twenty_step_loop(host):
    """(the pools of su3_truth.EXPM_CLASSES, the zero matrix and a NaN are tests/test_link_math_valu_host.py's, which
    runs on the same header; here the random matrices at its ten norms once more, and that the test still fires)"""
    norms = [1e-3, 0.01, 0.03, 0.1, 0.3, 0.49, 0.51, 1.0, 3.0, 30.0]
    out = host['valu_ranged']([f'rand {norm!r} 20000 {1000 + k}' for k, norm in enumerate(norms)])
    for norm, (entries, differ, far, mean_steps) in zip(norms, out):
        print(f'|A|_F = {norm:g}: {entries:.0f} entries, {differ:.0f} differ, mean steps {mean_steps:.2f} of 20')
        assert entries == 18 * 20000 and differ == 0 and far == 0, norm
    assert out[2][3] < 12.0
