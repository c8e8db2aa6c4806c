"""CPU tier of l2hmc/lattice/su3/pytorch/rational.py: Zolotarev's approximation of y^(-1/2), held to the theorems about it
with mpmath at 50 digits (tests/rational_restatement.py) on the float64 coefficients the module returns.

Tolerance of the equioscillation |e(y_i)| = delta, derived from the float64 evaluation: the error function is evaluated
exactly (50 digits) on the returned coefficients, so what separates |e(y_i)| from the returned delta is (a) the rounding of
the coefficients and (b) that of delta and A.  (a): sn and cn come back from `ellipj` to a few units u of absolute 1e-16
(they are <= 1; u = 4 eps is allowed), so a_r = rb cn^2 / sn^2 carries the relative error 2 u (1 / cn_r + 1 / sn_r), and e(y)
= sqrt(y) A prod (y + a_2k-1) / (y + a_2k) - 1 moves by at most sum_r |a_r / (y + a_r)| times that, <= sum_r 2 u (1 / cn_r + 1
/ sn_r); sn_r and cn_r follow from the returned a_r (cn^2 / sn^2 = a_r / rb).  (b): A and delta come from two values of
sqrt(y) prod (...), 2n + 2 roundings each on a value ~1: (2n + 2) eps.  The sum of the two is `eq_tol`; the measured
deviations are 5e-16 .. 6e-15 against tolerances 1e-14 .. 7e-13."""
import mpmath as mp
import numpy as np
import pytest

import rational_restatement as rr
from l2hmc.lattice.su3.pytorch.rational import Rational, zolotarev_inv_sqrt

EPS = 2.0 ** -52


def eq_tol(rat):
    t = rat.a / rat.rb
    sn, cn = 1.0 / np.sqrt(1.0 + t), np.sqrt(t / (1.0 + t))
    return float(np.sum(2 * 4 * EPS * (1.0 / cn + 1.0 / sn)) + (2 * rat.n + 2) * EPS)


@pytest.mark.parametrize('n,ratio', rr.CASES)
def test_equioscillation(n, ratio):
    rat = zolotarev_inv_sqrt(n, ratio * rr.RB, rr.RB)
    assert isinstance(rat, Rational) and rat.n == n and 0 < rat.delta < 1
    ext = rr.extrema(rat)
    assert len(ext) == 2 * n + 2, len(ext)
    signs = [mp.sign(e) for _, e in ext]
    assert all(signs[i] == -signs[i + 1] for i in range(len(ext) - 1)), signs
    dev = max(abs(abs(e) - mp.mpf(rat.delta)) for _, e in ext)
    print(f'n {n} ratio {ratio}: delta {rat.delta:.6g}, max | |e_i| - delta | = {float(dev):.3g}, tolerance {eq_tol(rat):.3g}')
    assert dev <= eq_tol(rat), (float(dev), eq_tol(rat))
    # nowhere on a grid is the error larger than delta (by more than the same tolerance)
    for i in range(401):
        y = mp.mpf(rat.ra) * (mp.mpf(rat.rb) / mp.mpf(rat.ra)) ** (mp.mpf(i) / 400)
        assert abs(rr.err(rat, y)) <= mp.mpf(rat.delta) + eq_tol(rat)


@pytest.mark.parametrize('n,ratio', rr.CASES)
def test_zeros_and_poles_interlace(n, ratio):
    rat = zolotarev_inv_sqrt(n, ratio * rr.RB, rr.RB)
    assert rat.a.shape == (2 * n,) and (np.diff(rat.a) < 0).all() and (rat.a > 0).all()
    assert np.array_equal(rat.zeros, rat.a[0::2]) and np.array_equal(rat.poles, rat.a[1::2])
    assert (rat.rho > 0).all() and np.isrealobj(rat.c)
    assert np.allclose(rat.mu ** 2, rat.poles, rtol=4 * EPS) and np.allclose(rat.nu ** 2, rat.zeros, rtol=4 * EPS)


@pytest.mark.parametrize('n,ratio', rr.CASES)
def test_partial_fractions_and_heatbath_factor(n, ratio):
    """rho_k and c_k are quotients of products of differences of neighbouring a_r: relative rounding n * 4 eps each, times
    the cancellation in a difference of neighbours, bounded here by max a_r / min |a_r - a_s| (mu, nu alike): the tolerance
    is that condition number times 8 n eps, asserted on the 50-digit values"""
    rat = zolotarev_inv_sqrt(n, ratio * rr.RB, rr.RB)
    gaps = lambda v: float(np.max(v) / np.min(np.abs(np.diff(np.sort(v))))) if len(v) > 1 else 1.0   # noqa: E731
    tol = 8 * n * EPS * max(gaps(rat.a), gaps(np.concatenate([rat.mu, rat.nu])))
    worst = 0.0
    for i in range(41):
        y = mp.mpf(rat.ra) * (mp.mpf(rat.rb) / mp.mpf(rat.ra)) ** (mp.mpf(i) / 40)
        d = abs(rr.R_pf(rat, y) / rr.R(rat, y) - 1)
        worst = max(worst, float(d))
        assert d <= tol, (float(y), float(d), tol)
        for q in (mp.sqrt(y), -mp.sqrt(y)):
            c = rr.C(rat, q)
            d = abs((c.real ** 2 + c.imag ** 2) * rr.R(rat, q * q) - 1)
            worst = max(worst, float(d))
            assert d <= tol, (float(q), float(d), tol)
    # and the float64 evaluations of the module agree with the 50-digit ones
    y = np.geomspace(rat.ra, rat.rb, 41)
    want = np.array([float(rr.R(rat, v)) for v in y])
    assert np.allclose(rat(y), want, rtol=(4 * n + 4) * EPS) and np.allclose(rat.partial_fractions(y), want, rtol=tol)
    cw = np.array([complex(rr.C(rat, v)) for v in np.sqrt(y)])
    assert np.allclose(rat.heatbath_factor(np.sqrt(y)), cw, rtol=tol)
    print(f'n {n} ratio {ratio}: worst {worst:.3g}, tolerance {tol:.3g}')


def test_bad_arguments():
    for bad in (dict(n=0, ra=0.1, rb=1.0), dict(n=1.5, ra=0.1, rb=1.0), dict(n=True, ra=0.1, rb=1.0),
                dict(n=2, ra=0.0, rb=1.0), dict(n=2, ra=1.0, rb=1.0), dict(n=2, ra=-1.0, rb=1.0),
                dict(n=2, ra=0.1, rb=float('inf')), dict(n=2, ra=float('nan'), rb=1.0)):
        with pytest.raises(ValueError, match='zolotarev_inv_sqrt'):
            zolotarev_inv_sqrt(**bad)
