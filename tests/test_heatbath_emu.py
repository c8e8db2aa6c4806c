"""CPU run of the kernels of csrc/su3_heatbath.hip themselves: the file is compiled for the host with g++ against the
stand-in HIP header of tests/host_emu.py (every thread of a workgroup an OS thread), under AddressSanitizer
and UBSan as a stand-alone program run as a child process, and both entry points are compared with the restatement
tests/heatbath_restatement.py from the same uniforms.  Catches indexing, checkerboard, wrap-around and out-of-bounds
mistakes without a GPU; the argument checks are those of the real cross-compiled library."""
import numpy as np
import pytest

import heatbath_restatement as hb
import host_emu
from native_layout import pack, unpack

NB = 3
# x + nu == x - nu; V/2 = 48: a partial wavefront, with the short extents in different places
LATTICES = [(2, 2, 2, 2), (4, 2, 6, 2), (2, 4, 2, 6)]
CASES = [(0.3, 1), (5.7, 4)]


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = host_emu.build(tmp_path_factory.mktemp('heatbath_emu'), 'heatbath_emu')

    def run(mode, L, swz, beta, ntry, xn, u):
        ox, of = host_emu.run(exe, [mode, NB, *L, swz, repr(float(beta)), ntry],
                              [xn, u if u is not None else np.zeros(1)], 2)
        return ox.view(np.complex128).reshape(8, NB, 4, 9, int(np.prod(L))), of.reshape(8, NB)
    return run


def compare(got, want, x, mu, parity, L, skip=None):
    """updated links to 1e-11, everything else bit-identical; skip: boolean [nb, V/2] of links left out"""
    V = int(np.prod(L))
    idx = hb.half_sites(L, parity)
    g, w, o = (a.reshape(NB, 4, V, 3, 3) for a in (got, want, x))
    d = np.abs(g[:, mu][:, idx] - w[:, mu][:, idx]).max((-2, -1))
    if skip is not None:
        d = np.where(skip, 0.0, d)
    assert d.max() <= 1e-11, (mu, parity, d.max())
    keep = np.ones((4, V), dtype=bool)
    keep[mu, idx] = False
    assert np.array_equal(g.transpose(1, 2, 0, 3, 4)[keep], o.transpose(1, 2, 0, 3, 4)[keep]), (mu, parity)
    return d.max()


@pytest.mark.parametrize('L', LATTICES)
def test_kernels_on_the_host(emu, L):
    rng = np.random.default_rng(31)
    x = hb.random_links(rng, NB, L)
    xn = pack(x)
    vh = int(np.prod(L)) // 2
    left_out = 0
    for swz in (0, 1):
        got, _ = emu('or', L, swz, 1.0, 1, xn, None)
        for mu in range(4):
            for parity in (0, 1):
                compare(unpack(got[2 * mu + parity], L), hb.overrelax(x, mu, parity), x, mu, parity, L)
        for beta, ntry in CASES:
            u = rng.random((8, NB, 3, 4 * ntry + 2, vh))
            got, fails = emu('hb', L, swz, beta, ntry, xn, u)
            for mu in range(4):
                for parity in (0, 1):
                    l = 2 * mu + parity
                    want, wf, margin = hb.heatbath(x, beta, mu, parity, u[l], ntry)
                    skip = margin.min((1, 2)) < 1e-12
                    left_out += int(skip.sum())
                    compare(unpack(got[l], L), want, x, mu, parity, L, skip)
                    if not skip.any():
                        assert np.array_equal(fails[l], wf), (mu, parity, fails[l], wf)
            if ntry == 1:
                assert 0 < fails.sum() < 8 * NB * 3 * vh            # the fallback is exercised
    assert left_out <= 1
    # without failure counts: no workspace, the same links
    beta, ntry = CASES[1]
    u = rng.random((8, NB, 3, 4 * ntry + 2, vh))
    a, _ = emu('hb', L, 1, beta, ntry, xn, u)
    b, _ = emu('hb_nofails', L, 1, beta, ntry, xn, u)
    assert np.array_equal(a, b)


def test_argument_errors_of_the_library():
    from l2hmc import native
    lib = native.load()
    hbk, orl = lib.l2q_su3_heatbath, lib.l2q_su3_overrelax
    p = 4096                                       # any non-null address: the checks come before every use of it
    ok = dict(xn=p, beta=5.7, mu=0, parity=0, u=p, ntry=4, fails=p, nb=1, T=2, X=2, Y=2, Z=2, ws=p, ws_bytes=4096)

    def call(**kw):
        a = {**ok, **kw}
        return hbk(a['xn'], a['beta'], a['mu'], a['parity'], a['u'], a['ntry'], a['fails'], a['nb'], a['T'], a['X'],
                   a['Y'], a['Z'], a['ws'], a['ws_bytes'], None)
    for kw in (dict(xn=None), dict(u=None), dict(ws=None), dict(mu=-1), dict(mu=4), dict(parity=2), dict(parity=-1),
               dict(ntry=0), dict(ntry=17), dict(beta=0.0), dict(beta=-1.0), dict(beta=float('inf')),
               dict(beta=float('nan')), dict(nb=0), dict(Z=0)):
        assert call(**kw) == -1, kw                                        # L2Q_EINVAL
    assert b'l2q_su3_heatbath' in lib.l2q_last_error()
    for kw in (dict(T=3), dict(X=5), dict(Y=1), dict(Z=7), dict(ws_bytes=0)):
        assert call(**kw) == -2, kw                                        # L2Q_ESHAPE
    assert orl(None, 0, 0, 1, 2, 2, 2, 2, None) == -1
    assert orl(p, 4, 0, 1, 2, 2, 2, 2, None) == -1 and orl(p, 0, 2, 1, 2, 2, 2, 2, None) == -1
    assert orl(p, 0, 0, 0, 2, 2, 2, 2, None) == -1
    assert orl(p, 0, 0, 1, 2, 2, 3, 2, None) == -2
    assert b'even extents' in lib.l2q_last_error()
