"""TEST INFRASTRUCTURE: the properties of Zolotarev's approximation of y^(-1/2) (l2hmc/lattice/su3/pytorch/rational.py)
evaluated with mpmath at 50 digits from the float64 coefficients the module returns: the error function e(y) = sqrt(y)
R(y) - 1, its extrema on [ra, rb], the partial fractions and the heatbath factor.  Nothing here knows the elliptic
functions: the coefficients are taken as data and the theorems about the optimal approximation are checked on them."""
import mpmath as mp

mp.mp.dps = 50

CASES = [(1, 1e-1), (3, 1e-2), (6, 1e-3), (10, 1e-3), (4, 0.5)]          # (n, ra / rb); rb = 2.5 in the tests
RB = 2.5


def R(rat, y):
    """the product form at 50 digits"""
    y = mp.mpf(y)
    out = mp.mpf(rat.A)
    for z, p in zip(rat.zeros, rat.poles):
        out *= (y + mp.mpf(float(z))) / (y + mp.mpf(float(p)))
    return out


def err(rat, y):
    return mp.sqrt(mp.mpf(y)) * R(rat, y) - 1


def R_pf(rat, y):
    y = mp.mpf(y)
    return mp.mpf(rat.A) * (1 + sum(mp.mpf(float(r)) / (y + mp.mpf(float(p))) for r, p in zip(rat.rho, rat.poles)))


def C(rat, q):
    q = mp.mpf(q)
    s = sum(mp.mpf(float(c)) / (q + 1j * mp.mpf(float(nu))) for c, nu in zip(rat.c, rat.nu))
    return (1 + 1j * s) / mp.sqrt(mp.mpf(rat.A))


def extrema(rat, per_gap=64):
    """the extrema of e on [ra, rb]: the end points and the interior stationary points, found by bracketing de/dt = 0 in t
    = log y on a grid fine against the 2n oscillations and refining with mpmath's root finder.  Returns [(y, e(y))]."""
    a, b = mp.log(mp.mpf(rat.ra)), mp.log(mp.mpf(rat.rb))

    def f(t):
        return err(rat, mp.exp(t))

    def df(t):
        return mp.diff(f, t)
    m = per_gap * (2 * rat.n + 2)
    ts = [a + (b - a) * i / m for i in range(m + 1)]
    d = [df(t) for t in ts]
    pts = [(mp.mpf(rat.ra), f(a))]
    for i in range(m):
        if d[i] == 0 or d[i] * d[i + 1] < 0:
            t = mp.findroot(df, (ts[i], ts[i + 1]), solver='anderson', tol=mp.mpf(10) ** -30, verify=False)
            pts.append((mp.exp(t), f(t)))
    pts.append((mp.mpf(rat.rb), f(b)))
    return pts
