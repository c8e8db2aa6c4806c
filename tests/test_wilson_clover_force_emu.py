"""CPU run of the two kernels of csrc/su3_clover_force.hip themselves: the file is compiled for the host with g++ against
the stand-in HIP header of tests/host_emu.py (every thread of a workgroup an OS thread), under AddressSanitizer and UBSan
as a stand-alone program run as a child process, and compared with the restatement
tests/wilson_clover_force_restatement.py: the workspace G against `g_field`, the force against `clover_force` as force,
as kick out of place and as kick in place, and the determinant-only and pseudofermion-only calls, npf 1 and 3, either
block order.  Catches a wrong chirality sign, a wrong block-entry or plane order, a wrong half index of the odd sites,
extent-2 insertion mistakes and out-of-bounds accesses without a GPU.  Every entry of every output enters the comparison;
the tolerances are those of the restatement file.  (The program itself checks: the kick in place and a chain alone give
the same bits, no input is written, a short workspace is refused.)"""
import numpy as np
import pytest

import host_emu
import wilson_clover_force_restatement as wcf
import wilson_clover_restatement as wc
import wilson_eo_restatement as we
import wilson_force_restatement as wf
import wilson_restatement as wr
from native_layout import pack
from wilson_gpu_util import antihermitian_bits

NB = wcf.NB
COEF = -0.05
CASES = [(1, 'hot', 1.769), (3, 'smooth', 1.0)]                             # npf, input, c_sw


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = host_emu.build(tmp_path_factory.mktemp('wilson_clover_force_emu'), 'wilson_clover_force_emu')

    def run(L, npf, swz, kc, dw, *fields):
        V = int(np.prod(L))
        g, *outs = host_emu.run(exe, [NB, npf, *L, swz, repr(float(kc)), repr(COEF), repr(float(dw))], fields, 5)
        return [g.reshape(NB, 6, 9, V)] + [o.view(np.complex128).reshape(NB, 4, 9, V) for o in outs]
    return run


@pytest.mark.parametrize('npf,kind,c_sw', CASES)
@pytest.mark.parametrize('L', we.EO_KERNEL_LATTICES)
def test_kernels_on_the_host(emu, L, npf, kind, c_sw):
    x, X, Y, ainv = wcf.force_inputs(kind, L, c_sw, NB, npf)
    v = wf.momentum(L, NB)
    kc = wc.KAPPA * c_sw
    want_g = wcf.pack_g(wcf.g_field(X, Y, ainv, kc, npf, L))
    want = wcf.clover_force(x, X, Y, ainv, wc.KAPPA, c_sw, npf)
    want_det = wcf.clover_force(x, None, None, ainv, wc.KAPPA, c_sw, npf)
    want_pf = wcf.clover_force(x, X, Y, None, wc.KAPPA, c_sw, 0.0)
    worst = 0.0
    for swz in (0, 1):
        g, force, kick, det, pf = emu(L, npf, swz, kc, npf, pack(x), wr.pack_spinor(X), wr.pack_spinor(Y),
                                      wc.pack_blocks(ainv), wf.pack_links(v))
        d = float(np.abs(g - want_g).max())
        assert d <= wcf.TOL_G, (swz, 'G', d)
        for name, got, w in (('force', force, want), ('kick', kick, v + COEF * want), ('determinant only', det, want_det),
                             ('pseudofermions only', pf, want_pf)):
            d = float(np.abs(wf.unpack_links(got, L) - w).max())
            worst = max(worst, d)
            assert d <= wcf.TOL_F, (swz, name, d)
            assert antihermitian_bits(got), (swz, name)
    print(f'{L} npf {npf} {kind} c_sw {c_sw}: worst force deviation / tolerance: {worst / wcf.TOL_F:.3g}')
