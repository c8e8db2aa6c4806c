"""CPU run of the kernel of csrc/su3_wilson_eo.hip itself: the file is compiled for the host with g++ against the stand-in
HIP header of tests/host_emu.py (every thread of a workgroup an OS thread), under AddressSanitizer and UBSan as a
stand-alone program run as a child process, and the half-lattice hop is compared with the restatement
tests/wilson_eo_restatement.py: both parities, flags 0..3, the four (a, b, aux) uses (out == aux included, in the
program), nrhs 1 and 3, either block order.  Catches half-index, parity, wrap-around (extent 2), seam-sign and
out-of-bounds mistakes without a GPU.  Every entry of every output enters the comparison; the tolerance is we.TOL (32 x the
extended-precision yardstick of the hop), that of the norm partials wr.norm_bound(V/2)."""
import numpy as np
import pytest

import host_emu
import wilson_eo_restatement as we
import wilson_restatement as wr
from native_layout import pack

NB = 2


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = host_emu.build(tmp_path_factory.mktemp('wilson_eo_emu'), 'wilson_eo_emu')

    def run(L, nrhs, swz, kappa, xn, src, aux):
        Vh = int(np.prod(L)) // 2
        of, on = host_emu.run(exe, [NB, nrhs, *L, swz, repr(float(kappa))], [xn, src, aux], 2)
        return (of.view(np.complex128).reshape(2, 4, 4, NB, nrhs, 12, Vh), on.reshape(2, 4, 4, NB, nrhs, -(-Vh // 256)))
    return run


@pytest.mark.parametrize('nrhs', [1, 3])
@pytest.mark.parametrize('L', we.EO_KERNEL_LATTICES)
def test_hop_on_the_host(emu, L, nrhs):
    Vh = int(np.prod(L)) // 2
    x, psi, aux = wr.links(L, NB), wr.spinors(L, NB, nrhs), we.aux_field(L, NB, nrhs)
    halves = [np.stack([we.pack_half(f, p) for p in (0, 1)]) for f in (psi, aux)]
    worst = 0.0
    for swz in (0, 1):
        of, on = emu(L, nrhs, swz, we.K, pack(x), *halves)
        for p in (0, 1):
            for fl, (dagger, ap) in enumerate(wr.FLAGS):
                for u, (name, a, b, with_aux) in enumerate(we.uses()):
                    want = we.hop_eo(x, psi, p, dagger, ap, a, aux if with_aux else None, b)
                    d = float(np.abs(of[p, fl, u] - we.pack_half(want, p)).max())
                    worst = max(worst, d)
                    assert d <= we.TOL, (swz, p, fl, name, d)
                    n2 = wr.norm2(want)
                    rel = float((np.abs(on[p, fl, u].sum(-1) - n2) / n2).max())
                    assert rel <= wr.norm_bound(Vh), (swz, p, fl, name, rel)
    print(f'{L} nrhs {nrhs}: worst deviation / tolerance: {worst / we.TOL:.3g}')
