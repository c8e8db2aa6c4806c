"""CPU run of the four kernels of csrc/su3_wilson_clover.hip themselves: the file is compiled for the host with g++
against the stand-in HIP header of tests/host_emu.py (every thread of a workgroup an OS thread), under AddressSanitizer
and UBSan as a stand-alone program run as a child process, and compared with the restatement
tests/wilson_clover_restatement.py: the clover term, the block inverse with its pivot and log-det partials, the hop kernel
on both parities, flags 0..3 and the six uses of `wc.uses()` (cmode 0, 1, 2; out == aux and the run without the partials
in the program, at flags 3), the site-local apply, nrhs 1 and 3, either block order.  Catches wrong half indices, a wrong
block-entry order, a missing conjugate below the diagonal, extent-2 leaf mistakes and out-of-bounds accesses without a GPU.  Every
entry of every output enters the comparison; the tolerances are those of the restatement file."""
import numpy as np
import pytest

import host_emu
import wilson_clover_restatement as wc
import wilson_eo_restatement as we
import wilson_restatement as wr
from native_layout import pack

NB = wc.NB
CASES = [(1, 'hot', 1.769, (0, 1)), (3, 'smooth', 1.0, (1,))]             # nrhs, input, c_sw, xcd_swizzle settings


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = host_emu.build(tmp_path_factory.mktemp('wilson_clover_emu'), 'wilson_clover_emu')

    def run(L, nrhs, swz, kappa, coef, xn, src, aux, ca, ci):
        Vh = int(np.prod(L)) // 2
        parts = -(-Vh // 256)
        cl, inv, pp, of, on, af, an = host_emu.run(exe, [NB, nrhs, *L, swz, repr(float(kappa)), repr(float(coef))],
                                                   [xn, src, aux, ca, ci], 7)
        return (cl.reshape(NB, 2, 2, 36, Vh), inv.reshape(NB, 2, 2, 36, Vh), pp.reshape(2, NB, 2, parts),
                of.view(np.complex128).reshape(2, 4, 6, NB, nrhs, 12, Vh), on.reshape(2, 4, 6, NB, nrhs, parts),
                af.view(np.complex128).reshape(2, NB, nrhs, 12, Vh), an.reshape(2, NB, nrhs, parts))
    return run


@pytest.mark.parametrize('nrhs,kind,c_sw,swizzles', CASES)
@pytest.mark.parametrize('L', we.EO_KERNEL_LATTICES)
def test_kernels_on_the_host(emu, L, nrhs, kind, c_sw, swizzles):
    V = int(np.prod(L))
    Vh = V // 2
    x, a, ainv = wc.fields(kind, L, c_sw, NB)
    psi, aux = wr.spinors(L, NB, nrhs), we.aux_field(L, NB, nrhs)
    halves = [np.stack([we.pack_half(f, p) for p in (0, 1)]) for f in (psi, aux)]
    blocks = {'a': a, 'ainv': ainv, None: None}
    piv = wc.pivots(a)
    wants = {(p, fl, u): wc.hop_clover(x, psi, p, blocks[blk], cmode, dagger, ap, ca, aux if with_aux else None, cb)
             for p in (0, 1) for fl, (dagger, ap) in enumerate(wr.FLAGS)
             for u, (_, cmode, blk, _, ca, cb, with_aux) in enumerate(wc.uses())}
    worst = 0.0
    for swz in swizzles:
        cl, inv, pp, of, on, af, an = emu(L, nrhs, swz, wc.KAPPA, wc.KAPPA * c_sw, pack(x), *halves, wc.pack_blocks(a),
                                          wc.pack_blocks(ainv))
        d = float(np.abs(cl - wc.pack_blocks(a)).max())
        assert d <= wc.TOL_A, (swz, 'term', d)
        d = wc.inv_defect(a, wc.unpack_blocks(inv, L))
        assert d <= wc.TOL_INV, (swz, 'inverse', d)
        for p in (0, 1):
            want = wc.half_min(piv, p)
            got = pp[0][:, p].min(-1)
            assert (np.abs(got - want) <= wc.PIVOT_BOUND * want).all(), (swz, p, got, want)
        ld, lp = wc.logdet(a), np.log(piv)
        for p in (0, 1):
            sabs = np.abs(lp).reshape(NB, V, 12)[:, we.sites(L, p)].sum((1, 2))
            assert (np.abs(pp[1][:, p].sum(-1) - ld[:, p]) <= wc.logdet_tol(12 * Vh, sabs)).all(), (swz, p, 'logdet')
        for p in (0, 1):
            for fl, (dagger, ap) in enumerate(wr.FLAGS):
                for u, name in enumerate(n[0] for n in wc.uses()):
                    want = wants[p, fl, u]
                    d = float(np.abs(of[p, fl, u] - we.pack_half(want, p)).max())
                    worst = max(worst, d)
                    assert d <= wc.TOL_HOP, (swz, p, fl, name, d)
                    n2 = wr.norm2(want)
                    rel = float((np.abs(on[p, fl, u].sum(-1) - n2) / n2).max())
                    assert rel <= wr.norm_bound(Vh), (swz, p, fl, name, rel)
            want = wc.apply_site(ainv, psi) * we.mask(L, p)
            d = float(np.abs(af[p] - we.pack_half(want, p)).max())
            assert d <= wc.TOL_M, (swz, p, 'apply', d)
            n2 = wr.norm2(want)
            assert float((np.abs(an[p].sum(-1) - n2) / n2).max()) <= wr.norm_bound(Vh), (swz, p, 'apply norm')
    print(f'{L} nrhs {nrhs} {kind} c_sw {c_sw}: worst hop deviation / tolerance: {worst / wc.TOL_HOP:.3g}')
