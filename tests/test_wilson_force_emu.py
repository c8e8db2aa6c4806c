"""CPU run of the kernel of csrc/su3_wilson_force.hip itself: the file is compiled for the host with g++ against the
stand-in HIP header of tests/host_emu.py (every thread of a workgroup an OS thread), under AddressSanitizer and UBSan as
a stand-alone program run as a child process, and its three output forms are compared with the restatement
tests/wilson_force_restatement.py.  Catches projection, outer-product, indexing, wrap-around, seam-sign and
out-of-bounds mistakes without a GPU.  Every entry of every output enters the comparison at wf.TOL (32 x the
extended-precision yardstick); a kick adds |coef| < 1 times the force to entries of size ~1, whose own rounding is far
below that."""
import numpy as np
import pytest

import host_emu
import wilson_force_restatement as wf
import wilson_restatement as wr
from wilson_gpu_util import antihermitian_bits

NB = 2
COEF = -0.05


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = host_emu.build(tmp_path_factory.mktemp('wilson_force_emu'), 'wilson_force_emu')

    def run(L, npf, swz, xn, Xn, Yn, vn):
        V = int(np.prod(L))
        outs = host_emu.run(exe, [NB, npf, *L, swz, repr(wr.KAPPA), repr(COEF)], [xn, Xn, Yn, vn], 4)
        return [o.view(np.complex128).reshape(2, -1, 4, 9, V) for o in outs]
    return run


@pytest.mark.parametrize('npf', [1, 3])
@pytest.mark.parametrize('L', wr.KERNEL_LATTICES)
def test_force_kernel_on_the_host(emu, L, npf):
    x, X, Y = wf.force_inputs(L, NB, npf)
    v = wf.momentum(L, NB)
    want = [wf.force(x, X, Y, wr.KAPPA, ap) for ap in (False, True)]               # flags 0, 2
    worst = 0.0
    for swz in (0, 1):
        force, kick, inplace, alone = emu(L, npf, swz, wf.pack_links(x), wr.pack_spinor(X), wr.pack_spinor(Y),
                                          wf.pack_links(v))
        for fl in range(2):
            for name, got, w in (('force', force[fl], want[fl]), ('kick', kick[fl], v + COEF * want[fl]),
                                 ('in place', inplace[fl], v + COEF * want[fl])):
                d = float(np.abs(wf.unpack_links(got, L) - w).max())
                worst = max(worst, d)
                assert d <= wf.TOL, (swz, fl, name, d)
                assert antihermitian_bits(got), (swz, fl, name)
            assert np.array_equal(kick[fl], inplace[fl]), (swz, fl)
            assert alone[fl].shape[0] == 1 and np.array_equal(alone[fl][0], force[fl][0]), (swz, fl)
    print(f'{L} npf {npf}: worst deviation / tolerance: {worst / wf.TOL:.3g}')
