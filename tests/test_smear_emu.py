"""CPU run of the kernels of csrc/su3_smear.hip themselves: the file is compiled for the host with g++ against the
stand-in HIP header of tests/host_emu.py (every thread of a workgroup an OS thread), under AddressSanitizer
and UBSan as a stand-alone program run as a child process, and the four entry points are compared with the restatement
tests/smear_restatement.py.  Catches indexing, decorated-field order, wrap-around and out-of-bounds mistakes without a
GPU.  Every link of every output enters the comparison; the tolerances are sm.TOL (32 x the projection yardstick)."""
import numpy as np
import pytest

import host_emu
import smear_restatement as sm
from native_layout import pack, pack_dec, unpack, unpack_dec

NB = 2          # 8 and 24 workgroups per launch: a multiple of the 8 XCDs, so that xcd_swizzle = 1 does permute them


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = host_emu.build(tmp_path_factory.mktemp('smear_emu'), 'smear_emu')

    def run(L, swz, cases, alphas, xn, b1n, b2n):
        oa, o1, o2, ov = host_emu.run(exe, [NB, *L, swz, ','.join(str(m) for _, m in cases),
                                            ','.join(repr(float(a)) for a, _ in cases),
                                            *(repr(float(a)) for a in alphas)], [xn, b1n, b2n], 4)
        V = int(np.prod(L))
        return (oa.view(np.complex128).reshape(len(cases), NB, 4, 9, V),
                o1.view(np.complex128).reshape(NB, 4, 3, 9, V), o2.view(np.complex128).reshape(NB, 4, 3, 9, V),
                ov.view(np.complex128).reshape(NB, 4, 9, V))
    return run


@pytest.mark.parametrize('L', sm.KERNEL_LATTICES)
def test_kernels_on_the_host(emu, L):
    x = sm.smooth_input(L, NB)
    a1, a2, a3 = sm.HYP_ALPHAS
    b1 = sm.hyp_level1(x, a3)
    b2 = sm.hyp_level2(x, b1, a2)
    v = sm.hyp_level3(x, b2, a1)
    apes = [sm.ape_step(x, alpha, D) for alpha, D in sm.APE_CASES]
    xn, b1n, b2n = pack(x), pack_dec(sm.dec_stack(b1)), pack_dec(sm.dec_stack(b2))
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
