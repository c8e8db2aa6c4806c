"""CPU run of the kernels of csrc/su3_gaugefix.hip themselves: the file is compiled for the host with g++ against the
stand-in HIP header of tests/host_emu.py (every thread of a workgroup an OS thread), under AddressSanitizer
and UBSan as a stand-alone program run as a child process, and the three entry points are compared with the
restatement tests/gaugefix_restatement.py.  Catches indexing, checkerboard, wrap-around and out-of-bounds mistakes
without a GPU.  The update has no data-dependent accept decision: every link enters every comparison."""
import numpy as np
import pytest

import gaugefix_restatement as gf
import host_emu
from native_layout import pack, pack_g, unpack, unpack_g

NB = 3
# x + mu == x - mu; V/2 = 48: a partial wavefront, with the short extents in different places
LATTICES = [(2, 2, 2, 2), (4, 2, 6, 2), (2, 4, 2, 6)]
OMEGAS = [1.0, 1.7]


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = host_emu.build(tmp_path_factory.mktemp('gaugefix_emu'), 'gaugefix_emu')

    def run(what, L, swz, mask, omega, with_g, with_active, xn, gn):
        """what: 1 the two half-sweeps, 2 the condition, 4 the transformation (a sum of them)"""
        ox, og, oc, oa = host_emu.run(exe, [what, NB, *L, swz, mask, repr(float(omega)), int(with_g),
                                            int(with_active)], [xn, gn], 4)
        V = int(np.prod(L))
        return (ox.view(np.complex128).reshape(-1, NB, 4, 9, V), og.view(np.complex128).reshape(-1, NB, 9, V),
                oc.reshape(NB, 2), oa.view(np.complex128).reshape(NB, 4, 9, V))
    return run


@pytest.mark.parametrize('L', LATTICES)
def test_kernels_on_the_host(emu, L):
    rng = np.random.default_rng(37)
    x = gf.random_links(rng, NB, L)
    g0 = gf.random_su3(rng, (NB, *L))
    xn, gn = pack(x), pack_g(g0)
    worst = [0.0, 0.0, 0.0, 0.0, 0.0]
    want_apply = gf.apply(x, g0)
    for swz in (0, 1):
        for mask in gf.MASKS:
            # the condition with every mask and the transformation once per placement ride on the first sweep run
            what = 1 + 2 + (4 if mask == gf.LANDAU else 0)
            for omega in OMEGAS:
                want = [gf.half_sweep(x, mask, parity, omega) for parity in (0, 1)]
                for with_g in (False, True):
                    ox, og, cond, ap = emu(what, L, swz, mask, omega, with_g, True, xn, gn)
                    for parity in (0, 1):
                        wx, wg = want[parity]
                        got = unpack(ox[parity], L)
                        assert np.array_equal(got[1], x[1]), (mask, omega, parity)          # the inactive chain
                        assert np.array_equal(og[parity][1], gn[1])
                        dx = float(np.abs(got[0::2] - wx[0::2]).max())
                        assert dx <= 1e-11, (mask, omega, swz, parity, dx)
                        if with_g:
                            dg = float(np.abs(unpack_g(og[parity], L)[0::2] - (wg @ g0)[0::2]).max())
                            assert dg <= 1e-11, (mask, omega, swz, parity, dg)
                            worst[1] = max(worst[1], dg)
                        else:
                            assert np.array_equal(og[parity], gn)
                        worst[0] = max(worst[0], dx)
                    if what & 2:
                        F, theta = gf.condition(x, mask)
                        dF = float(np.abs(cond[:, 0] - F).max())
                        dth = float(np.abs(cond[:, 1] / theta - 1.0).max())
                        assert dF <= 1e-12 and dth <= 1e-12, (mask, swz, dF, dth)
                        worst[2:4] = [max(worst[2], dF), max(worst[3], dth)]
                    if what & 4:
                        da = float(np.abs(unpack(ap, L) - want_apply).max())
                        assert da <= 1e-12, (swz, da)
                        worst[4] = max(worst[4], da)
                    what = 1
    # no active array: every chain is updated
    ox, _, _, _ = emu(1, L, 1, 13, 1.7, False, False, xn, gn)
    for parity in (0, 1):
        assert np.abs(unpack(ox[parity], L) - gf.half_sweep(x, 13, parity, 1.7)[0]).max() <= 1e-11
    print(f'{L}: worst |dU| / 1e-11 = {worst[0] / 1e-11:.3g}, |dG| / 1e-11 = {worst[1] / 1e-11:.3g}, |dF| / 1e-12 = '
          f'{worst[2] / 1e-12:.3g}, |dtheta / theta| / 1e-12 = {worst[3] / 1e-12:.3g}, apply / 1e-12 = '
          f'{worst[4] / 1e-12:.3g}')
