"""CPU run of the kernels of csrc/su3_wilson.hip themselves: the file is compiled for the host with g++ against the
stand-in HIP header of tests/host_emu.py (every thread of a workgroup an OS thread), under AddressSanitizer and UBSan as
a stand-alone program run as a child process, and the three entry points are compared with the restatement
tests/wilson_restatement.py.  Catches spin-projection, indexing, wrap-around, seam-sign and out-of-bounds mistakes
without a GPU.  Every entry of every output enters the comparison; the tolerance of the apply is wr.TOL (32 x the
extended-precision yardstick), that of the norm partials wr.norm_bound(V)."""
import numpy as np
import pytest

import host_emu
import wilson_restatement as wr
from native_layout import pack

NB = 2
EPS = 2.0 ** -52


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = host_emu.build(tmp_path_factory.mktemp('wilson_emu'), 'wilson_emu')

    def run(L, nrhs, swz, kappa, xn, psin, xrpq, coef):
        V = int(np.prod(L))
        parts = -(-V // 256)
        oa, on, ocg, orr, oxp = host_emu.run(exe, [NB, nrhs, *L, swz, repr(float(kappa))], [xn, psin, xrpq, coef], 5)
        return (oa.view(np.complex128).reshape(4, NB, nrhs, 12, V), on.reshape(4, NB, nrhs, parts),
                ocg.view(np.complex128).reshape(2, NB, nrhs, 12, V), orr.reshape(NB, nrhs, parts),
                oxp.view(np.complex128).reshape(NB, nrhs, 12, V))
    return run


@pytest.mark.parametrize('nrhs', [1, 3])
@pytest.mark.parametrize('L', wr.KERNEL_LATTICES)
def test_kernels_on_the_host(emu, L, nrhs):
    V = int(np.prod(L))
    x, psi = wr.links(L, NB), wr.spinors(L, NB, nrhs)
    want = [wr.wilson(x, psi, wr.KAPPA, dagger, ap) for dagger, ap in wr.FLAGS]      # flags 0..3
    # the fields of a CG update: four more Gaussian fields, a coefficient per system, alpha = 0 for the first system
    rng = np.random.default_rng(77 + V + nrhs)
    f = rng.standard_normal((2, 4, NB, nrhs, 12, V))
    xrpq = f[0] + 1j * f[1]
    coef = rng.standard_normal((2, NB, nrhs))
    coef[0, 0, 0] = 0.0
    a, b = coef[0][..., None, None], coef[1][..., None, None]
    cx, cr, cp, cq = xrpq
    worst = 0.0
    for swz in (0, 1):
        oa, on, ocg, orr, oxp = emu(L, nrhs, swz, wr.KAPPA, pack(x), wr.pack_spinor(psi), xrpq, coef)
        for fl in range(4):
            got = wr.unpack_spinor(oa[fl], L)
            d = float(np.abs(got - want[fl]).max())
            worst = max(worst, d)
            assert d <= wr.TOL, (swz, fl, d)
            n2 = wr.norm2(want[fl])
            rel = float((np.abs(on[fl].sum(-1) - n2) / n2).max())
            assert rel <= wr.norm_bound(V), (swz, fl, rel)
        # x += alpha p, r -= alpha q: one fused multiply-add per real entry against numpy's two roundings
        for got, w, t in ((ocg[0], cx + a * cp, np.abs(cx) + np.abs(a * cp)), (ocg[1], cr - a * cq, np.abs(cr) + np.abs(a * cq)),
                          (oxp, cq + b * cp, np.abs(cq) + np.abs(b * cp))):
            assert float((np.abs(got - w) / t).max()) <= 4 * EPS, swz
        assert np.array_equal(ocg[0][0, 0], cx[0, 0]) and np.array_equal(ocg[1][0, 0], cr[0, 0])     # alpha = 0: the same bits
        n2 = wr.norm2(ocg[1])
        assert float((np.abs(orr.sum(-1) - n2) / n2).max()) <= wr.norm_bound(V), swz
    print(f'{L} nrhs {nrhs}: worst deviation / tolerance: {worst / wr.TOL:.3g}')
