"""TEST INFRASTRUCTURE: numpy restatement of the SU(3) Landau / Coulomb gauge fixing, vectorised over sites and written
from the formulas (include/l2q.h, "SU(3) Landau and Coulomb gauge fixing"), not from the kernels.  Reference layout
``x[nb, 4, T, X, Y, Z, 3, 3]`` complex128, ``g[nb, T, X, Y, Z, 3, 3]``; the gauge directions D are the 4-bit set of the
kernels (bit mu = direction mu)."""
import numpy as np

from heatbath_restatement import SUBGROUPS, embed, qconj, random_links, su2_part, unit   # noqa: F401
from oracle import su3 as osu3

LANDAU = 15
MASKS = [15, 14, 13, 11, 7]                      # Landau and the Coulomb gauges of time_dir 0, 1, 2, 3


def coulomb(time_dir):
    return 15 & ~(1 << time_dir)


def dirs(D):
    return [mu for mu in range(4) if (D >> mu) & 1]


def parity_mask(L, parity):
    t, x, y, z = np.meshgrid(*[np.arange(n) for n in L], indexing='ij')
    return ((t + x + y + z) & 1) == parity


def back(f, mu):
    """f(x - mu) for a site field f[nb, T, X, Y, Z, ...]"""
    return np.roll(f, +1, axis=mu + 1)


def power(a, omega):
    """a^omega of unit quaternions a [4, ...]: (cos(omega phi), n sin(omega phi)), phi = atan2(|a_vec|, a0); the
    identity where a_vec = 0"""
    sv = np.sqrt(a[1] * a[1] + a[2] * a[2] + a[3] * a[3])
    ok = sv > 0
    phi = omega * np.arctan2(sv, a[0])
    with np.errstate(divide='ignore', invalid='ignore'):
        f = np.where(ok, np.sin(phi) / np.where(ok, sv, 1.0), 0.0)
    return np.stack([np.where(ok, np.cos(phi), 1.0), a[1] * f, a[2] * f, a[3] * f])


def local_g(x, D, omega):
    """g(x) of the local step at every site, from the links as they are: [nb, T, X, Y, Z, 3, 3]"""
    k = sum(x[:, mu] + osu3.adj(back(x[:, mu], mu)) for mu in dirs(D))
    g = np.zeros_like(k)
    g[..., 0, 0] = g[..., 1, 1] = g[..., 2, 2] = 1.0
    w = k
    for i, j in SUBGROUPS:
        _, rh = unit(su2_part(w, i, j))          # (1, 0, 0, 0) where |r| is zero or not finite: the identity below
        e = embed(power(qconj(rh), omega), i, j)
        g, w = e @ g, e @ w
    return g


def half_sweep(x, D, parity, omega):
    """the local step at the sites of one parity -> (new links, g [nb, T, X, Y, Z, 3, 3] with the identity at the sites
    of the other parity)"""
    L = x.shape[2:6]
    here = parity_mask(L, parity)[None, ..., None, None]
    g = np.where(here, local_g(x, D, omega), np.eye(3))
    out = np.empty_like(x)
    for mu in range(4):
        u = np.where(here, g @ x[:, mu], x[:, mu])                       # U_mu(x) <- g U_mu(x)
        v = back(u, mu)                                                  # v(x) = U_mu(x - mu)
        v = np.where(here, v @ osu3.adj(g), v)                           # U_mu(x - mu) <- U_mu(x - mu) g^H
        out[:, mu] = np.roll(v, -1, axis=mu + 1)
    return out, g


def sweep(x, D, omega):
    for parity in (0, 1):
        x, _ = half_sweep(x, D, parity, omega)
    return x


def condition(x, D):
    """(F [nb], theta [nb])"""
    nb = x.shape[0]
    V = int(np.prod(x.shape[2:6]))
    d = dirs(D)
    F = sum(np.trace(x[:, mu], axis1=-2, axis2=-1).real.reshape(nb, -1).sum(1) for mu in d) / (3.0 * len(d) * V)

    def a_of(u):
        a = (u - osu3.adj(u)) / 2j
        return a - np.trace(a, axis1=-2, axis2=-1)[..., None, None] * np.eye(3) / 3.0
    delta = sum(a_of(x[:, mu]) - back(a_of(x[:, mu]), mu) for mu in d)
    theta = (np.abs(delta) ** 2).reshape(nb, -1).sum(1) / (3.0 * V)
    return F, theta


def apply(x, g):
    """U_mu(x) -> g(x) U_mu(x) g(x + mu)^H"""
    return np.stack([g @ x[:, mu] @ osu3.adj(np.roll(g, -1, axis=mu + 1)) for mu in range(4)], 1)


def random_su3(rng, shape, amp=None):
    """exp(i amp H), H random traceless Hermitian with unit-variance entries (amp None: Haar-like, as random_links)"""
    z = rng.normal(size=(*shape, 3, 3)) + 1j * rng.normal(size=(*shape, 3, 3))
    if amp is None:
        return osu3.project_su(osu3.project_su(z))
    h = 0.5 * (z + osu3.adj(z))
    h = h - np.trace(h, axis1=-2, axis2=-1)[..., None, None] * np.eye(3) / 3.0
    lam, vec = np.linalg.eigh(h)
    return (vec * np.exp(1j * amp * lam)[..., None, :]) @ osu3.adj(vec)


def smooth_links(rng, nb, L, amp):
    """links exp(i amp H): close to the identity for small amp"""
    return random_su3(rng, (nb, 4, *L), amp)


def pure_gauge(rng, nb, L, amp=None):
    """a random gauge transform of the cold start: U_mu(x) = g(x) g(x + mu)^H"""
    g = random_su3(rng, (nb, *L), amp)
    cold = np.broadcast_to(np.eye(3, dtype=np.complex128), (nb, 4, *L, 3, 3))
    return apply(cold, g)
