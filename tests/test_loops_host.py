"""CPU tier of the Wilson-loop / Polyakov-loop observables: the yardstick tests/loops_restatement.py against facts that
do not depend on it (the numpy oracle's plaquettes and the reference's recorded ones, the closed form of uniform
abelian flux, the cold start, gauge and centre transformations), and the two pure functions `creutz_ratios` and
`static_potential` against an exact area law.  These validate the ruler that tests/test_loops_gpu.py measures with."""
import math

import numpy as np
import pytest
import torch

import flow_restatement as fr
import loops_restatement as lr
from oracle import su3 as osu3

PLANES = [(u, v) for u in range(1, 4) for v in range(u)]          # the oracle's plane order


def hot(nb, L, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(osu3.project_su(rng.normal(size=(nb, 4, *L, 3, 3))
                                            + 1j * rng.normal(size=(nb, 4, *L, 3, 3))))


def test_pair_index_is_the_documented_one():
    assert [lr.pair_index(mu, nu) for mu, nu in lr.PAIRS] == list(range(12))
    assert lr.PAIRS[0] == (0, 1) and lr.PAIRS[3] == (1, 0) and lr.PAIRS[11] == (3, 2)


def test_yardstick_r1_t1_is_the_plaquette(golden):
    """R = T = 1 on the links: pairs u > v are the oracle's plaquette traces site by site, pairs u < v their
    conjugates; the same on the reference's recorded links and plaquettes"""
    g = golden('su3_ops')
    for x, want in ((hot(2, (3, 2, 4, 5), 2), None), (torch.from_numpy(g['x']), g['wloops'])):
        w = lr.loop_traces(x, 1, x, 1).numpy()
        ow = osu3.wilson_loops(x.numpy())
        for p, (u, v) in enumerate(PLANES):
            assert np.abs(w[lr.pair_index(u, v)] - ow[p]).max() <= 1e-13
            assert np.abs(w[lr.pair_index(v, u)] - ow[p].conj()).max() <= 1e-13
            if want is not None:
                assert np.abs(w[lr.pair_index(u, v)] - want[p]).max() <= 1e-13
        s, scale = lr.loop_sums(x, 1, x, 1)
        re, im = osu3.plaq_sums(x.numpy())
        up = [lr.pair_index(u, v) for u, v in PLANES]
        assert np.abs(s[:, up].sum(1).numpy() - (re + 1j * im)).max() <= 1e-11
        assert bool((scale >= s.abs() - 1e-9).all())
    assert torch.equal(lr.line(x, 1), x)


@pytest.mark.parametrize('n01,n23', [(1, 1), (2, -1), (1, 0)])
def test_yardstick_flux_closed_form(n01, n23):
    """uniform abelian flux along H = diag(1, -1, 0), phi_ab = 2 pi n_ab / (N_a N_b): on EVERY site, loops across the
    twisted boundary included, and for every R, T that does not wrap,
      tr W_01(R, T) = tr W_10 = 1 + 2 cos(R T phi01),   tr W_23(R, T) = tr W_32 = 1 + 2 cos(R T phi23),
    and tr W = 3 in the other planes."""
    L = (4, 6, 4, 8)
    x = fr.flux_config(L, n01, n23)
    phi = {(0, 1): 2 * math.pi * n01 / (L[0] * L[1]), (2, 3): 2 * math.pi * n23 / (L[2] * L[3])}
    lines = {n: lr.line(x, n) for n in range(1, max(L) + 1)}
    worst, checked = 0.0, 0
    for r in range(1, max(L) + 1):
        for t in range(1, max(L) + 1):
            w = lr.loop_traces(lines[r], r, lines[t], t)
            for mu, nu in lr.PAIRS:
                if r > L[mu] or t > L[nu]:                         # this loop would wrap
                    continue
                p = phi.get((min(mu, nu), max(mu, nu)))
                want = 3.0 if p is None else 1.0 + 2.0 * math.cos(r * t * p)
                worst = max(worst, float((w[lr.pair_index(mu, nu)] - want).abs().max()))
                checked += 1
    # every (R <= N_mu, T <= N_nu) of every ordered pair: 2 (4*6 + 4*4 + 4*8 + 6*4 + 6*8 + 4*8)
    assert checked == 352 and worst <= 1e-12, (checked, worst)
    # abelian lines along H: a Polyakov loop is tr diag(e^{i a}, e^{-i a}, 1) = 1 + 2 cos a, real
    for mu in range(4):
        p = lr.polyakov(x, mu)
        assert float(p.imag.abs().max()) <= 1e-12 and float(p.real.max()) <= 3.0 + 1e-12


def test_yardstick_cold_start():
    L = (2, 3, 4, 2)
    x = torch.eye(3, dtype=fr.C128).expand(2, 4, *L, 3, 3).contiguous()
    s, scale = lr.loop_table_sums(x, 2, 2)
    v = float(np.prod(L))
    assert torch.equal(s, torch.full_like(s, 3.0 * v)) and torch.equal(scale, s.real)
    for mu in range(4):
        p = lr.polyakov(x, mu) / 3.0
        assert p.shape == (2, *L[:mu], *L[mu + 1:]) and torch.equal(p, torch.ones_like(p))
        c = lr.polyakov_correlator(p)
        assert torch.equal(c, torch.ones_like(c))


def test_yardstick_symmetry_gauge_and_centre():
    """W_{nu mu}(T, R) is W_{mu nu}(R, T) run backwards; gauge rotations move neither the loop sums nor a Polyakov
    loop (its trace closes at one site); a centre element on one time slice multiplies P_0 and leaves the loops"""
    L = (3, 2, 4, 2)
    x = hot(2, L, 4)
    s, scale = lr.loop_table_sums(x, 3, 3)
    for mu, nu in lr.PAIRS:
        d = s[:, :, :, lr.pair_index(mu, nu)] - s[:, :, :, lr.pair_index(nu, mu)].transpose(1, 2).conj()
        assert float((d.abs() / scale[..., lr.pair_index(mu, nu)]).max()) <= 1e-13
    xr = fr.gauge_rotate(x, fr.rand_su3((2, *L), 3.0, torch.Generator().manual_seed(9)))
    sr, _ = lr.loop_table_sums(xr, 3, 3)
    assert float(((s - sr).abs() / scale).max()) <= 1e-13
    z = complex(math.cos(2 * math.pi / 3), math.sin(2 * math.pi / 3))
    xz = x.clone()
    xz[:, 0, 1] *= z
    sz, _ = lr.loop_table_sums(xz, 3, 3)
    assert float(((s - sz).abs() / scale).max()) <= 1e-13
    for mu in range(4):
        p = lr.polyakov(x, mu)
        assert float((p - lr.polyakov(xr, mu)).abs().max()) <= 1e-13
        assert float((lr.polyakov(xz, mu) - (z if mu == 0 else 1.0) * p).abs().max()) <= 1e-13
    p = lr.polyakov(x, 0) / 3.0
    c = lr.polyakov_correlator(p)
    assert float((c[:, 0, 0, 0] - (p.abs() ** 2).reshape(2, -1).mean(-1)).abs().max()) <= 1e-15
    # C(r) = C(-r)
    assert float((c - torch.roll(c.flip((1, 2, 3)), (1, 1, 1), dims=(1, 2, 3))).abs().max()) <= 1e-15


def test_creutz_ratios_and_static_potential():
    from l2hmc.lattice.su3.pytorch.lattice import creutz_ratios, static_potential
    sigma, m, c = 0.21, 0.37, 0.11
    r = torch.arange(1, 7, dtype=torch.float64)[:, None]
    t = torch.arange(1, 6, dtype=torch.float64)[None, :]
    w = torch.exp(-sigma * r * t - m * (r + t) - c)
    w = torch.stack([w, w])                                        # a leading chain axis
    chi = creutz_ratios(w)
    assert chi.shape == (2, 5, 4) and float((chi - sigma).abs().max()) <= 1e-13
    v = static_potential(w)
    assert v.shape == (2, 6, 4) and float((v - (sigma * r + m)).abs().max()) <= 1e-13
    # NaN where the argument of the logarithm is not positive; nothing raises
    bad = w.clone()
    bad[0, 2, 2] = -bad[0, 2, 2]
    bad[1, 0, 0] = 0.0
    chi, v = creutz_ratios(bad), static_potential(bad)
    assert bool(torch.isnan(chi[0, 1:3, 1:3]).all()) and bool(torch.isnan(chi[1, 0, 0]))
    assert bool(torch.isnan(v[0, 2, 1:3]).all()) and bool(torch.isnan(v[1, 0, 0]))
    assert int(torch.isnan(chi).sum()) == 5 and int(torch.isnan(v).sum()) == 3
    assert float((chi[~torch.isnan(chi)] - sigma).abs().max()) <= 1e-13
    assert creutz_ratios(w[:, :1]).shape == (2, 0, 4) and static_potential(w[..., :1]).shape == (2, 6, 0)
