"""Zolotarev's optimal rational approximation of y^(-1/2) and what the one-flavour (RHMC) pseudofermion action of
``wilson.py`` needs of it.  Pure numpy / scipy, no GPU.

    R(y) = A prod_{k=1..n} (y + a_{2k-1}) / (y + a_{2k})  ~  y^(-1/2)  on [ra, rb],
    a_r = rb cn^2(r v, k) / sn^2(r v, k),  v = K(k) / (2n + 1),  k = sqrt(1 - ra / rb),  r = 1 .. 2n

(Zolotarev 1877; in this form: Chiu et al., hep-lat/0206007, and Luescher's openQCD notes "Rational approximations").
The a_r decrease with r, so zeros -a_{2k-1} and poles -a_{2k} interlace on the negative axis.  sqrt(y) R(y) - 1
equioscillates between 2n + 2 extrema of alternating sign on [ra, rb], the end points among them; A is fixed by making
the two end-point values symmetric about 1, and delta = max |1 - sqrt(y) R(y)| is their half distance.

Partial fractions:  R(y) = A (1 + sum_k rho_k / (y + a_{2k})),  rho_k > 0.
Heatbath factor: for Hermitian Q with Q^2 = y,
    C = A^(-1/2) prod_k (Q + i mu_k) (Q + i nu_k)^-1,  mu_k = sqrt(a_{2k}),  nu_k = sqrt(a_{2k-1}),
satisfies C C^H = R(Q^2)^-1 exactly, and C = A^(-1/2) [1 + i sum_k c_k (Q + i nu_k)^-1] with the real
    c_k = prod_j (mu_j - nu_k) / prod_{j != k} (nu_j - nu_k);   (Q + i nu)^-1 = (Q - i nu) (Q^2 + nu^2)^-1.
Only y^(-1/2) is needed: no Remez, no multiprecision at run time."""
from __future__ import annotations

import numpy as np
from scipy.special import ellipj, ellipk


class Rational:
    """The approximation and its derived coefficients, all float64 numpy arrays of length n (``a``: 2n): ``n``, ``ra``,
    ``rb``, ``A``, ``delta``, ``a`` (a_1 .. a_2n, decreasing), ``zeros`` = a_{2k-1}, ``poles`` = a_{2k}, ``rho``, ``mu``,
    ``nu``, ``c``."""

    def __init__(self, n: int, ra: float, rb: float, A: float, delta: float, a: np.ndarray):
        self.n, self.ra, self.rb, self.A, self.delta, self.a = n, ra, rb, A, delta, a
        self.zeros, self.poles = a[0::2].copy(), a[1::2].copy()
        z, p = self.zeros, self.poles
        self.rho = np.array([np.prod(z - p[k]) / np.prod(np.delete(p, k) - p[k]) for k in range(n)])
        self.mu, self.nu = np.sqrt(p), np.sqrt(z)
        self.c = np.array([np.prod(self.mu - self.nu[k]) / np.prod(np.delete(self.nu, k) - self.nu[k]) for k in range(n)])

    def __call__(self, y):
        """R(y) by the product"""
        y = np.asarray(y, dtype=np.float64)[..., None]
        return self.A * np.prod((y + self.zeros) / (y + self.poles), axis=-1)

    def partial_fractions(self, y):
        """R(y) by A (1 + sum_k rho_k / (y + a_2k))"""
        y = np.asarray(y, dtype=np.float64)[..., None]
        return self.A * (1.0 + np.sum(self.rho / (y + self.poles), axis=-1))

    def heatbath_factor(self, q):
        """C(q) for real q (complex), by its partial fractions"""
        q = np.asarray(q, dtype=np.float64)[..., None]
        return (1.0 + 1j * np.sum(self.c / (q + 1j * self.nu), axis=-1)) / np.sqrt(self.A)


def zolotarev_inv_sqrt(n: int, ra: float, rb: float) -> Rational:
    """Zolotarev's optimal degree-(n, n) approximation of y^(-1/2) on [ra, rb], 0 < ra < rb, as a `Rational`; its
    ``delta`` is the achieved relative error max |1 - sqrt(y) R(y)| on the interval."""
    if isinstance(n, bool) or int(n) != n or int(n) < 1:
        raise ValueError(f'zolotarev_inv_sqrt: the degree must be an integer >= 1, got {n!r}')
    ra, rb = float(ra), float(rb)
    if not (np.isfinite(ra) and np.isfinite(rb) and 0.0 < ra < rb):
        raise ValueError(f'zolotarev_inv_sqrt: need 0 < ra < rb, got {ra!r}, {rb!r}')
    n = int(n)
    m = 1.0 - ra / rb                                       # the parameter k^2
    v = ellipk(m) / (2 * n + 1)
    sn, cn, _, _ = ellipj(np.arange(1, 2 * n + 1) * v, m)
    a = rb * (cn / sn) ** 2

    def f(y):                                               # sqrt(y) R(y) / A
        return np.sqrt(y) * np.prod((y + a[0::2]) / (y + a[1::2]))
    fa, fb = f(ra), f(rb)                                   # the two outermost extrema, of opposite sign
    return Rational(n, ra, rb, 2.0 / (fa + fb), abs(fa - fb) / (fa + fb), a)
