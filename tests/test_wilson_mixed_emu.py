"""CPU run of the kernels of csrc/su3_wilson_f32.hip themselves: the file is compiled for the host with g++ against the
stand-in HIP header of tests/host_emu.py (every thread of a workgroup an OS thread; float2 from the header beside the
program), under AddressSanitizer and UBSan as a stand-alone program run as a child process.  The fp32 half-lattice hop
is compared with the restatement tests/wilson_mixed_restatement.py within wm.TOL_F32 (32 x the extended-precision
yardstick of the fp32 hop): both parities, flags 0..3, the four (a, b, aux) uses (the fused norm and out == aux leaving
the same bits: in the program), nrhs 1 and 3, either block order, outputs pre-filled with -7.  The link copy is held
entry by entry, exactly; the two BLAS-1 kernels, demote and promote to one rounding of the exact result."""
import numpy as np
import pytest

import host_emu
import wilson_eo_restatement as we
import wilson_mixed_restatement as wm
import wilson_restatement as wr
from native_layout import pack

NB = 2
C64 = np.complex64


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = host_emu.build(tmp_path_factory.mktemp('wilson_f32_emu'), 'wilson_f32_emu')

    def run(L, nrhs, swz, kappa, xn, src, aux, f64, scal):
        Vh = int(np.prod(L)) // 2
        parts = -(-Vh // 256)
        links, of, on, b32, b64 = host_emu.run(exe, [NB, nrhs, *L, swz, repr(float(kappa))], [xn, src, aux, f64, scal], 5)
        field = (NB, nrhs, 12, Vh)
        return (links.view(C64).reshape(NB, 2, 4, 9, Vh), of.view(C64).reshape(2, 4, 4, *field),
                on.reshape(2, 4, 4, NB, nrhs, parts), b32.view(C64).reshape(4, *field),
                b64[:NB * nrhs * parts].reshape(NB, nrhs, parts), b64[NB * nrhs * parts:].view(np.complex128).reshape(field))
    return run


def sq(f):
    """|f|^2 per system of a native field in float64"""
    return (f.real.astype(np.float64) ** 2 + f.imag.astype(np.float64) ** 2).sum((-2, -1))


@pytest.mark.parametrize('nrhs', [1, 3])
@pytest.mark.parametrize('L', we.EO_KERNEL_LATTICES)
def test_f32_kernels_on_the_host(emu, L, nrhs):
    Vh = int(np.prod(L)) // 2
    x, psi, aux = wr.links(L, NB), wr.spinors(L, NB, nrhs).astype(C64), we.aux_field(L, NB, nrhs).astype(C64)
    halves = [np.stack([we.pack_half(f, p) for p in (0, 1)]) for f in (psi, aux)]
    f64 = we.pack_half(wr.spinors(L, NB, 12)[:, 12 - nrhs:], 0)
    rng = np.random.default_rng(11)
    scal = rng.standard_normal((3, NB, nrhs))
    scal[:, 0, 0] = 0.0                                                    # one system with alpha = beta = scale = 0
    worst = 0.0
    for swz in (0, 1):
        links, of, on, b32, part, x64 = emu(L, nrhs, swz, we.K, pack(x), *halves, f64, scal)
        # the link copy: exactly float32 of the link at the h-th site of each parity
        assert np.array_equal(links, wm.links_eo_f32(x))
        for p in (0, 1):
            for fl, (dagger, ap) in enumerate(wr.FLAGS):
                for u, (name, a, b, with_aux) in enumerate(we.uses()):
                    want = wm.hop_eo_f32(x, psi, p, dagger, ap, a, aux if with_aux else None, b)
                    assert want.dtype == C64
                    d = float(np.abs(of[p, fl, u] - we.pack_half(want, p)).max())
                    worst = max(worst, d)
                    assert d <= wm.TOL_F32, (swz, p, fl, name, d)
                    n2 = sq(of[p, fl, u])                                  # the partials against the kernel's own field
                    rel = float((np.abs(on[p, fl, u].sum(-1) - n2) / n2).max())
                    assert rel <= wm.norm_bound_f32(Vh), (swz, p, fl, name, rel)
        # BLAS-1: the exact result of the float32 operands, rounded once (fma): within one float32 ulp of its terms
        al, be, sc = (s[..., None, None] for s in scal)
        a32, b32c = al.astype(np.float32).astype(np.float64), be.astype(np.float32).astype(np.float64)
        xs, rs, ps, qs = (h.astype(np.complex128) for h in (*halves[0], *halves[1]))
        ulp = 2.0 ** -23
        for got, want, size in ((b32[0], xs + a32 * ps, np.abs(xs) + np.abs(a32 * ps)),
                                (b32[1], rs - a32 * qs, np.abs(rs) + np.abs(a32 * qs)),
                                (b32[2], qs + b32c * ps, np.abs(qs) + np.abs(b32c * ps))):
            assert (np.abs(got - want) <= ulp * size).all()
        assert np.array_equal(b32[0][0, 0], halves[0][0][0, 0]) and np.array_equal(b32[1][0, 0], halves[0][1][0, 0])
        rel = float((np.abs(part.sum(-1) - sq(b32[1])) / sq(b32[1])).max())
        assert rel <= wm.norm_bound_f32(Vh), rel
        # demote: the float64 product rounded to float32 once, exactly; promote: one rounding in float64
        dem = (sc * f64.real).astype(np.float32) + 1j * (sc * f64.imag).astype(np.float32)
        assert np.array_equal(b32[3], dem.astype(C64))
        assert (np.abs(x64 - (f64 + sc * xs)) <= 2.0 ** -52 * (np.abs(f64) + np.abs(sc * xs))).all()
        assert np.array_equal(x64[0, 0], f64[0, 0]) and not np.array_equal(x64[1, 0], f64[1, 0])   # scale = 0: untouched
    print(f'{L} nrhs {nrhs}: worst deviation / tolerance: {worst / wm.TOL_F32:.3g}')
