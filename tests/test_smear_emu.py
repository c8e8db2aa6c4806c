"""CPU run of the kernels of csrc/su3_smear.hip themselves: the file is compiled for the host with g++ against the
stand-in HIP header of tests/native_host/loops_emu/ (every thread of a workgroup an OS thread), under AddressSanitizer
and UBSan as a stand-alone program run as a child process, and the four entry points are compared with the restatement
tests/smear_restatement.py.  Catches indexing, decorated-field order, wrap-around and out-of-bounds mistakes without a
GPU.  Every link of every output enters the comparison; the tolerances are sm.TOL (32 x the projection yardstick)."""
import os
import subprocess

import numpy as np
import pytest

import smear_restatement as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NH = os.path.join(ROOT, 'tests', 'native_host')
NB = 2          # 8 and 24 workgroups per launch: a multiple of the 8 XCDs, so that xcd_swizzle = 1 does permute them


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('smear_emu')
    exe = tmp / 'smear_emu'
    subprocess.run(['g++', '-std=c++20', '-O1', '-g', '-pthread', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=undefined', '-I', os.path.join(NH, 'loops_emu'),
                    '-I', os.path.join(ROOT, 'l2hmc-qcd_amd', 'csrc'),
                    os.path.join(NH, 'smear_emu', 'smear_emu.cpp'), '-o', str(exe)], check=True)

    def run(L, swz, cases, alphas, xn, b1n, b2n):
        fx, f1, f2, oa, o1, o2, ov = (str(tmp / n) for n in ('x.bin', 'b1.bin', 'b2.bin', 'oa.bin', 'o1.bin', 'o2.bin',
                                                            'ov.bin'))
        for a, f in ((xn, fx), (b1n, f1), (b2n, f2)):
            a.view(np.float64).tofile(f)
        subprocess.run([str(exe), str(NB), *map(str, L), str(swz), ','.join(str(m) for _, m in cases),
                        ','.join(repr(float(a)) for a, _ in cases), *(repr(float(a)) for a in alphas), fx, f1, f2, oa, o1,
                        o2, ov], check=True)
        V = int(np.prod(L))
        return (np.fromfile(oa).view(np.complex128).reshape(len(cases), NB, 4, 9, V),
                np.fromfile(o1).view(np.complex128).reshape(NB, 4, 3, 9, V),
                np.fromfile(o2).view(np.complex128).reshape(NB, 4, 3, 9, V),
                np.fromfile(ov).view(np.complex128).reshape(NB, 4, 9, V))
    return run


def pack(x):
    """x[nb, 4, T, X, Y, Z, 3, 3] -> the native layout xn[nb, 4, 9, V]"""
    return np.ascontiguousarray(x.reshape(x.shape[0], 4, -1, 9).transpose(0, 1, 3, 2))


def unpack(xn, L):
    return np.ascontiguousarray(xn.transpose(0, 1, 3, 2)).reshape(xn.shape[0], 4, *L, 3, 3)


def pack_dec(b):
    """a decorated dict -> the native layout [nb, 4, 3, 9, V]"""
    a = sm.dec_stack(b)
    return np.ascontiguousarray(a.reshape(a.shape[0], 4, 3, -1, 9).transpose(0, 1, 2, 4, 3))


def unpack_dec(bn, L):
    return np.ascontiguousarray(bn.transpose(0, 1, 2, 4, 3)).reshape(bn.shape[0], 4, 3, *L, 3, 3)


@pytest.mark.parametrize('L', sm.KERNEL_LATTICES)
def test_kernels_on_the_host(emu, L):
    x = sm.smooth_input(L, NB)
    a1, a2, a3 = sm.HYP_ALPHAS
    b1 = sm.hyp_level1(x, a3)
    b2 = sm.hyp_level2(x, b1, a2)
    v = sm.hyp_level3(x, b2, a1)
    apes = [sm.ape_step(x, alpha, D) for alpha, D in sm.APE_CASES]
    xn, b1n, b2n = pack(x), pack_dec(b1), pack_dec(b2)
    worst = {k: 0.0 for k in ('ape', 'level1', 'level2', 'level3')}
    for swz in (0, 1):
        oa, o1, o2, ov = emu(L, swz, sm.APE_CASES, sm.HYP_ALPHAS, xn, b1n, b2n)
        for i, (alpha, D) in enumerate(sm.APE_CASES):
            got = unpack(oa[i], L)
            for mu in range(4):
                if not (D >> mu) & 1:
                    assert np.array_equal(got[:, mu], x[:, mu]), (D, mu)       # copied bit for bit
            worst['ape'] = max(worst['ape'], float(np.abs(got - apes[i]).max()))
            assert worst['ape'] <= sm.TOL['ape'], (swz, alpha, D, worst['ape'])
        worst['level1'] = max(worst['level1'], float(np.abs(unpack_dec(o1, L) - sm.dec_stack(b1)).max()))
        worst['level2'] = max(worst['level2'], float(np.abs(unpack_dec(o2, L) - sm.dec_stack(b2)).max()))
        worst['level3'] = max(worst['level3'], float(np.abs(unpack(ov, L) - v).max()))
        for k in ('level1', 'level2', 'level3'):
            assert worst[k] <= sm.TOL[k], (swz, k, worst[k])
    print(f'{L}: worst deviation / tolerance: ' + ', '.join(f'{k} {worst[k] / sm.TOL[k]:.3g}' for k in worst))
