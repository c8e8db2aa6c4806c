"""GPU tier of the loop observables: the kernels behind l2q_su3_line_extend, l2q_su3_loop_reduce and l2q_su3_polyakov
and the LatticeSU3 surface on top of them, against the independent restatement tests/loops_restatement.py (torch on
the CPU; validated on its own in tests/test_loops_host.py).

Tolerance of every sum: |sum - yardstick| <= 1e-12 max(S, V), S = the yardstick's sum over sites of |tr W| -- the rule
of tests/test_flow_gpu.py.  A loop with R + T <= 16 is at most 32 products of matrices with unit-size entries, about
1e-13 per term.  Every measured ratio is printed."""
import functools
import math

import numpy as np
import pytest
import torch

import flow_restatement as fr
import loops_restatement as lr
from oracle import su3 as osu3

pytestmark = pytest.mark.gpu

LATTICES = [(2, 2, 2, 2), (1, 3, 2, 5), (3, 5, 2, 7), (4, 4, 4, 4), (2, 2, 8, 8), (3, 8, 8, 8), (2, 2, 2, 32)]
NB = 3
Z3 = complex(math.cos(2 * math.pi / 3), math.sin(2 * math.pi / 3))
UP = [(u, v) for u in range(1, 4) for v in range(u)]               # the planes of l2q_su3_plaq_planes, in its order


@pytest.fixture(scope='module')
def ops():
    from l2hmc import _ops
    return _ops


@pytest.fixture()
def tuning():
    """set_tuning for the test, the default back afterwards"""
    from l2hmc import native
    yield native.set_tuning
    native.set_tuning('xcd_swizzle', 1)


def lattice(nb, L):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    return LatticeSU3(nb, list(L))


def dev(a):
    a = a.numpy() if isinstance(a, torch.Tensor) else a
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu()


def vol(L):
    return int(np.prod(L))


def hot(nb, L, rng):
    """hot start as tests/test_flow_gpu.py: projectSU of a complex Gaussian"""
    return torch.from_numpy(osu3.project_su(rng.normal(size=(nb, 4, *L, 3, 3))
                                            + 1j * rng.normal(size=(nb, 4, *L, 3, 3))))


@functools.lru_cache(maxsize=None)
def reference(L):
    """the hot start of lattice L and the yardstick's 3 x 3 table of loop sums on it, computed once and only read"""
    x = hot(NB, L, np.random.default_rng(17))
    want, scale = lr.loop_table_sums(x, 3, 3)
    return x, want, scale.clamp(min=float(vol(L)))


def ratio(got, want, scale):
    return float(((got - want).abs() / scale).max())


# ------------------------------------------------------------------ 1. loop sums
@pytest.mark.parametrize('L', LATTICES)
def test_loop_sums_vs_restatement(ops, tuning, L):
    """all 12 pairs of the 3 x 3 table (on the small lattices R, T reach and pass an extent, and wrap), under both
    block orders; the inputs keep their bits; sums[R, T, k(mu, nu)] = conj sums[T, R, k(nu, mu)]"""
    x, want, scale = reference(L)
    xn = ops.su3_pack(dev(x))
    keep = xn.clone()
    lat = lattice(NB, L)
    for swz in (0, 1):
        tuning('xcd_swizzle', swz)
        got = host(lat.wilson_loop_sums_n(xn, 3, 3))
        assert got.shape == (NB, 3, 3, 12)
        rel = ratio(got, want, scale)
        print(f'L={L} swz={swz} loop sums |d|/max(S,V) = {rel:.3e}')
        assert rel <= 1e-12
        assert torch.equal(xn, keep)
        sym = 0.0
        for mu, nu in lr.PAIRS:
            k, kt = lr.pair_index(mu, nu), lr.pair_index(nu, mu)
            sym = max(sym, ratio(got[..., k], got[..., kt].transpose(1, 2).conj(), scale[..., k]))
        print(f'L={L} swz={swz} symmetry |d|/max(S,V) = {sym:.3e}')
        assert sym <= 1e-12
    # one call with two different line fields and shifts beyond every extent of the small lattices
    a, b = lr.line(x, 2), lr.line(x, 3)
    an, bn = ops.su3_pack(dev(a)), ops.su3_pack(dev(b))
    for r, t in ((2, 3), (5, 9)):
        w, s = lr.loop_sums(a, r, b, t)
        rel = ratio(host(ops.su3_loop_sums_n(an, r, bn, t, L)), w, s.clamp(min=float(vol(L))))
        print(f'L={L} a != b, r={r} t={t}: |d|/max(S,V) = {rel:.3e}')
        assert rel <= 1e-12


# ------------------------------------------------------------------ 2. anchor: the plaquette kernel
def check_anchor(ops, x, L):
    xn = ops.su3_pack(dev(x))
    s = host(ops.su3_loop_sums_n(xn, 1, xn, 1, L))
    p = torch.view_as_complex(host(ops.su3_plaq_planes_n(xn, L)).contiguous())
    up = s[:, [lr.pair_index(u, v) for u, v in UP]]
    dn = s[:, [lr.pair_index(v, u) for u, v in UP]]
    e = max(float((up - p).abs().max()), float((dn - p.conj()).abs().max()))
    print(f'L={tuple(L)} anchor: |loop sums(1, 1) - plaq planes| = {e:.3e}')
    assert e <= 1e-10


@pytest.mark.parametrize('L', LATTICES)
def test_anchor_is_the_plaquette_kernel(ops, L):
    check_anchor(ops, reference(L)[0], L)


def test_anchor_on_the_golden_links(ops, golden):
    g = golden('su3_ops')
    L = tuple(int(i) for i in g['latvolume'])
    check_anchor(ops, torch.from_numpy(g['x']), L)
    xn = ops.su3_pack(dev(g['x']))
    s = host(ops.su3_loop_sums_n(xn, 1, xn, 1, L))
    want = torch.from_numpy(g['wloops']).reshape(6, g['x'].shape[0], -1).sum(-1).T
    e = float((s[:, [lr.pair_index(u, v) for u, v in UP]] - want).abs().max())
    print(f'golden plaquettes: |d| = {e:.3e}')
    assert e <= 1e-10


# ------------------------------------------------------------------ 3. line_extend
@pytest.mark.parametrize('L', [(1, 3, 2, 5), (4, 4, 4, 4)])
def test_line_extend(ops, L):
    """lines of length n = 1..4 built link by link against the yardstick's line(x, n) to n 1e-14; the aliased call has
    the bits of the out-of-place one.  No extension at all (length 1) is a copy of the links; the kernel's shift n = 0
    is, by its formula, lines_in(x) U(x), and a shift of a whole extent is the same call."""
    x = reference(L)[0]
    xn = ops.su3_pack(dev(x))
    keep = xn.clone()
    cur = xn.clone()
    assert float((host(ops.su3_unpack(cur, L)) - lr.line(x, 1)).abs().max()) == 0.0
    for n in range(2, 5):
        out = ops.su3_line_extend_n(cur, xn, n - 1, L)
        assert out.data_ptr() != cur.data_ptr()
        alias = cur.clone()
        assert ops.su3_line_extend_n(alias, xn, n - 1, L, out=alias) is alias
        assert torch.equal(alias, out)
        e = float((host(ops.su3_unpack(out, L)) - lr.line(x, n)).abs().max())
        print(f'L={L} line length {n}: |d| = {e:.3e}')
        assert e <= n * 1e-14
        cur = out
    sq = ops.su3_line_extend_n(xn, xn, 0, L)
    assert float((host(ops.su3_unpack(sq, L)) - x @ x).abs().max()) <= 2e-14
    # the shift is taken modulo the extent of each direction: 60 is a multiple of every extent here
    assert torch.equal(ops.su3_line_extend_n(xn, xn, 60, L), sq)
    assert torch.equal(xn, keep)


# ------------------------------------------------------------------ 4. Polyakov loops
@pytest.mark.parametrize('L', LATTICES)
def test_polyakov(ops, L):
    x, want, scale = reference(L)
    lat = lattice(NB, L)
    xd = dev(x)
    xr = fr.gauge_rotate(x, fr.rand_su3((NB, *L), 3.0, torch.Generator().manual_seed(9)))
    xz = x.clone()
    xz[:, 0, L[0] - 1] *= Z3                                       # a centre element on every U_0 of one time slice
    xrd, xzd = dev(xr), dev(xz)
    for mu in range(4):
        p = lr.polyakov(x, mu)
        got = host(ops.su3_polyakov_n(ops.su3_pack(xd), mu, L))
        assert got.shape == p.shape == (NB, *L[:mu], *L[mu + 1:])
        e = float((got - p).abs().max())
        # the rotated copy: the kernel on it against the yardstick on it, to the same N_mu 1e-14; that the rotation
        # moves no value is then a statement about the yardstick alone (g = exp(3 TAH) is unitary to ~1e-14, and
        # tr g L g^H = tr L (g^H g): 1e-13 covers it, as tests/test_loops_host.py asks)
        pr = lr.polyakov(xr, mu)
        moved = float((pr - p).abs().max())
        er = float((host(ops.su3_polyakov_n(ops.su3_pack(xrd), mu, L)) - pr).abs().max())
        print(f'L={L} mu={mu} Polyakov per site |d| = {e:.3e}, gauge-rotated |d| = {er:.3e}, rotation moves the '
              f'yardstick by {moved:.3e}')
        assert e <= L[mu] * 1e-14 and er <= L[mu] * 1e-14 and moved <= 1e-13
        assert float((host(lat.polyakov_loops(xd, mu)) - p / 3.0).abs().max()) <= L[mu] * 1e-14
    # centre transformation: P_0 picks up the factor, per site and in the mean
    p0, p0z = host(lat.polyakov(xd, 0)), host(lat.polyakov(xzd, 0))
    ez = float((p0z - Z3 * p0).abs().max())
    print(f'L={L} centre: |P(zU) - z P(U)| = {ez:.3e}')
    assert ez <= 3 * L[0] * 1e-14
    assert float((p0 - (lr.polyakov(x, 0) / 3.0).reshape(NB, -1).mean(-1)).abs().max()) <= L[0] * 1e-14
    # ... and neither transformation moves the loop sums
    for name, y in (('gauge-rotated', xrd), ('centre', xzd)):
        rel = ratio(host(lat.wilson_loop_sums_n(ops.su3_pack(y), 3, 3)), want, scale)
        print(f'L={L} {name} loop sums |d|/max(S,V) = {rel:.3e}')
        assert rel <= 1e-12
    # the correlator, by FFT on the device against one roll per displacement
    for mu in (0, 3):
        c = host(lat.polyakov_correlator(xd, mu))
        p = lr.polyakov(x, mu) / 3.0
        ec = float((c - lr.polyakov_correlator(p)).abs().max())
        e0 = float((c.reshape(NB, -1)[:, 0] - (p.abs() ** 2).reshape(NB, -1).mean(-1)).abs().max())
        print(f'L={L} mu={mu} correlator |d| = {ec:.3e}, |C(0) - mean |P|^2| = {e0:.3e}')
        assert c.shape == p.shape and c.dtype == torch.float64
        assert ec <= 1e-13 and e0 <= 1e-13


# ------------------------------------------------------------------ 5. flux configurations through the Python surface
@pytest.mark.parametrize('n01,n23', [(1, 1), (2, -1), (1, 0)])
def test_flux_loop_table(n01, n23):
    """tr W = 1 + 2 cos(R T phi) in the two flux planes, 3 in the others (tests/test_loops_host.py), averaged the way
    `wilson_loop_table` averages"""
    L = (4, 6, 4, 8)
    x = dev(fr.flux_config(L, n01, n23))
    lat = lattice(1, L)
    p01, p23 = 2 * math.pi * n01 / (L[0] * L[1]), 2 * math.pi * n23 / (L[2] * L[3])
    r = torch.arange(1, 5, dtype=torch.float64)[:, None]
    for td, tmax, form in ((0, 4, lambda a: ((1 + 2 * torch.cos(a * p01)) + 6) / 9),
                           (3, 5, lambda a: ((1 + 2 * torch.cos(a * p23)) + 6) / 9),
                           (None, 4, lambda a: (2 * (1 + 2 * torch.cos(a * p01)) + 2 * (1 + 2 * torch.cos(a * p23))
                                                + 24) / 36)):
        t = torch.arange(1, tmax + 1, dtype=torch.float64)[None, :]
        w = host(lat.wilson_loop_table(x, 4, tmax, time_dir=td))
        e = float((w[0] - form(r * t)).abs().max())
        print(f'flux {n01, n23} time_dir={td}: |table - closed form| = {e:.3e}')
        assert w.shape == (1, 4, tmax) and e <= 1e-12


# ------------------------------------------------------------------ 6. sizes users run
@pytest.mark.parametrize('L,nb,chains', [((8, 8, 8, 8), 256, (0, 37, 255)), ((16, 16, 16, 16), 4, (3,))])
def test_loop_sizes_users_run(ops, L, nb, chains):
    gen = torch.Generator().manual_seed(33)
    x = fr.rand_su3((nb, 4, *L), 3.0, gen)
    lat = lattice(nb, L)
    xn = ops.su3_pack(dev(x))
    keep = xn.clone()
    got = host(lat.wilson_loop_sums_n(xn, 2, 2))
    sel = list(chains)
    xs = x[sel].contiguous()
    want, scale = lr.loop_table_sums(xs, 2, 2)
    rel = ratio(got[sel], want, scale.clamp(min=float(vol(L))))
    print(f'L={L} nb={nb} chains {chains}: loop sums |d|/max(S,V) = {rel:.3e}')
    assert rel <= 1e-12
    assert torch.equal(xn, keep)
    for mu in (0, 3):
        e = float((host(ops.su3_polyakov_n(xn, mu, L))[sel] - lr.polyakov(xs, mu)).abs().max())
        print(f'L={L} nb={nb} mu={mu} Polyakov per site |d| = {e:.3e}')
        assert e <= L[mu] * 1e-14


# ------------------------------------------------------------------ 7. the Python surface
def test_loops_surface(ops):
    L = (4, 4, 4, 6)
    nb = 2
    gen = torch.Generator().manual_seed(44)
    x = dev(fr.rand_su3((nb, 4, *L), 3.0, gen))
    x0 = dev(fr.rand_su3((nb, 4, *L), 3.0, gen))
    lat = lattice(nb, L)
    w = lat.wilson_loop_table(x, 3, 4)
    assert w.shape == (nb, 3, 4) and w.dtype == torch.float64
    assert lat.wilson_loop_table(x, 4, 6, time_dir=3).shape == (nb, 4, 6)
    assert lat.wilson_loop_table(x, 4, 4, time_dir=None).shape == (nb, 4, 4)
    for rmax, tmax, td in ((5, 1, 0), (1, 5, 0), (1, 7, 3), (0, 1, 0), (1, 0, 0), (1, 5, None), (1, 1, 7)):
        with pytest.raises(ValueError):
            lat.wilson_loop_table(x, rmax, tmax, time_dir=td)
    with pytest.raises(RuntimeError):
        lat.wilson_loop_table(x.clone().requires_grad_(True), 2, 2)
    with pytest.raises(RuntimeError):
        lat.polyakov(x.clone().requires_grad_(True))
    e = float((lat.wilson_loop_table(x, 1, 1, None)[:, 0, 0] * 1 - lat.plaqs(x)).abs().max())
    print(f'|W(1, 1) over all pairs - plaqs| = {e:.3e}')
    assert e <= 1e-13
    assert lat.polyakov_loops(x, 0).shape == (nb, 4, 4, 6) and lat.polyakov_loops(x, 3).shape == (nb, 4, 4, 4)
    assert lat.polyakov(x).shape == (nb,) and lat.polyakov(x).dtype == torch.complex128
    assert lat.polyakov_correlator(x, 3).shape == (nb, 4, 4, 4)
    # the table feeds the two pure functions
    from l2hmc.lattice.su3.pytorch.lattice import creutz_ratios, static_potential
    assert creutz_ratios(w).shape == (nb, 2, 3) and static_potential(w).shape == (nb, 3, 3)
    # calc_metrics is what it was, and the Polyakov entries come after every key of it
    beta = torch.tensor(5.7)
    m = lat.calc_metrics(x, beta)
    assert list(m) == ['plaqs', 'sinQ', 'intQ', 'action', 'dsdx']
    m1 = lat.calc_metrics(x, beta, xinit=x0)
    assert list(m1) == ['plaqs', 'sinQ', 'intQ', 'action', 'dsdx', 'daction', 'dplaqs', 'dQint', 'dQsin']
    mp = {**m, **lat.polyakov_metrics(x)}
    assert list(mp) == list(m) + ['ploop']
    assert torch.equal(mp['ploop'], lat.polyakov(x, 0).abs()) and mp['ploop'].shape == (nb,)
    mp1 = {**m1, **lat.polyakov_metrics(x, xinit=x0)}
    assert list(mp1) == list(m1) + ['ploop', 'dploop']
    assert torch.equal(mp1['dploop'], (lat.polyakov(x, 0).abs() - lat.polyakov(x0, 0).abs()).abs())
    # a chain run alone equals the same chain in the batch
    one = lattice(1, L)
    for k in range(nb):
        xk = x[k:k + 1].contiguous()
        assert float((one.wilson_loop_table(xk, 3, 4) - w[k:k + 1]).abs().max()) <= 1e-14
        assert float((one.polyakov_loops(xk, 0) - lat.polyakov_loops(x, 0)[k:k + 1]).abs().max()) <= 1e-14
