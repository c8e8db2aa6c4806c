"""High-precision truth for the per-link SU(3) routines of csrc/su3_math.hpp (TEST INFRASTRUCTURE, CPU only).

Every value here comes from mpmath at 60 digits, never from another fp64 routine:

  expm      mp.expm
  polar_u   X (X^H X)^(-1/2) from mp.eigh of X^H X -- deliberately NOT the cubic closed form the kernels and
            oracle/su3.py share
  polar_su  polar_u times exp(-i arg(det) / 3)
  tah       (X - X^H)/2 - tr(.)/3
  mul       the four products op(A) op(B), op = identity or adjoint
  vec8      oracle.su3.su3_to_vec of the truth projection (linear: adds no error that matters)

Truths are returned as numpy ``clongdouble`` so that the field-level combinations the GPU tests form from them
(masked half-updates, sums) round well below the fp64 unit u = 2^-53 the tolerances are written in.

Input classes are deterministic (``numpy.random.default_rng(seed)``) and each is a POOL of 16 matrices.  A field
of nf x V links is filled by ``pool[(7 f + 13 s) % 16]`` (``field_index``): neighbouring sites and fields hold
different matrices with a known truth, so any indexing slip shows, and the mpmath cost stays at the pool size.

Stated exclusions.  The projection the kernels implement is the reference's closed-form cubic, which is itself
wrong far from the unit circle: 8e-6 at condition number 1e4, garbage at 1e8 or at input scale 1e-30.  Matching
it there means nothing, so no class has a condition number >= 1e4 or an input scale below 1e-20 or above 1e20;
the sampled classes (plain Gaussians, TAH of Gaussians) are drawn by rejection at condition number <= 100, that
of the worst explicit class (1, 0.1, 0.01).  NaN and Inf inputs are left out as well.

``python tests/su3_truth.py --measure`` prints the figures the tolerances of tests/test_su3_group_*.py are
derived from: the error ratio of torch.matrix_exp (CPU, complex128) against truth per expm class, and the error
of oracle.su3.project_su / project_u against truth per projection class.
"""
from __future__ import annotations

import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import su3 as osu3  # noqa: E402

DPS = 60
POOL = 16
U = 2.0 ** -53
LD = np.longdouble
CLD = np.clongdouble

ALGEBRA_NORMS = {'0': 0.0, '1e-300': 1e-300, '1e-8': 1e-8, '0.25': 0.25, '0.5': 0.5,
                 '0.5+ulp': 0.5 * (1.0 + 2.0 ** -52), '1': 1.0, '2': 2.0, '4': 4.0, '10': 10.0, '100': 100.0,
                 '1e3': 1e3}
THETAS = {'1e-3': 1e-3, '1': 1.0, '30': 30.0}
GENERAL_SCALES = {'0.05': 0.05, '0.8': 0.8, '3': 3.0, '30': 30.0}
SIGMAS = {'1_1_1': (1.0, 1.0, 1.0), '2_2_0.5': (2.0, 2.0, 0.5), '1_0.5_0.5': (1.0, 0.5, 0.5),
          '3_1_0.1': (3.0, 1.0, 0.1), '1_0.1_0.01': (1.0, 0.1, 0.01), '1e3_1e3_1e3': (1e3, 1e3, 1e3),
          '1e-3_2e-3_3e-3': (1e-3, 2e-3, 3e-3), '1e3_2e3_5e2': (1e3, 2e3, 5e2)}
DELTAS = {'1e-15': 1e-15, '1e-12': 1e-12, '1e-8': 1e-8, '1e-4': 1e-4, '1e-2': 1e-2}
MAX_COND = 100.0

EXPM_ALGEBRA = ['alg_' + k for k in ALGEBRA_NORMS]
EXPM_ANTIHERMITIAN_TRACELESS = EXPM_ALGEBRA + [f'{s}_{t}' for s in ('degenerate', 'zero_eig') for t in THETAS]
EXPM_ANTIHERMITIAN = EXPM_ANTIHERMITIAN_TRACELESS + [f'scalar_{t}' for t in THETAS]
EXPM_CLASSES = EXPM_ANTIHERMITIAN + [f'nilpotent_{t}' for t in THETAS] + ['general_' + k for k in GENERAL_SCALES]
PROJ_CLASSES = (['sigma_' + k for k in SIGMAS] + ['near_unitary_' + k for k in DELTAS] + ['gaussian', 'tah_gaussian'])


# ----------------------------------------------------------------------------------------- numpy <-> mpmath
def _to_mp(a):
    return mp.matrix([[mp.mpc(float(a[i, j].real), float(a[i, j].imag)) for j in range(3)] for i in range(3)])


def _ld(x):
    return LD(mp.nstr(x, 25, min_fixed=0, max_fixed=0))


def _from_mp(m):
    out = np.zeros((3, 3), dtype=CLD)
    for i in range(3):
        for j in range(3):
            z = mp.mpc(m[i, j])
            out[i, j] = CLD(_ld(z.real)) + CLD(1j) * CLD(_ld(z.imag))
    return out


def _over_pool(fn, *pools):
    with mp.workdps(DPS):
        return np.stack([_from_mp(fn(*[_to_mp(p[k]) for p in pools])) for k in range(len(pools[0]))])


# ----------------------------------------------------------------------------------------- the truths
def _mp_polar_u(x):
    h = x.H * x
    ev, q = mp.eigh(h)
    d = mp.diag([1 / mp.sqrt(ev[k]) for k in range(3)])
    return x * (q * d * q.H)


def _mp_polar_su(x):
    m = _mp_polar_u(x)
    return m * mp.expj(-mp.arg(mp.det(m)) / 3)


def _mp_tah(x):
    r = (x - x.H) / 2
    return r - (r[0, 0] + r[1, 1] + r[2, 2]) / 3 * mp.eye(3)


def expm(pool, sign=1):
    """exp(sign * A) of every matrix of the pool -> [16, 3, 3] clongdouble"""
    return _over_pool(lambda a: mp.expm(sign * a), pool)


def polar_u(pool):
    return _over_pool(_mp_polar_u, pool)


def polar_su(pool):
    return _over_pool(_mp_polar_su, pool)


def tah(pool):
    return _over_pool(_mp_tah, pool)


def mul(pa, pb, adjoint_a=False, adjoint_b=False):
    return _over_pool(lambda a, b: (a.H if adjoint_a else a) * (b.H if adjoint_b else b), pa, pb)


def vec8(m):
    """su3_to_vec of (truth) matrices [..., 3, 3] -> [..., 8]; longdouble in, longdouble out"""
    return osu3.su3_to_vec(m)


# ----------------------------------------------------------------------------------------- input classes
def _gauss(rng, n=POOL, scale=1.0):
    return scale * (rng.normal(size=(n, 3, 3)) + 1j * rng.normal(size=(n, 3, 3)))


def random_su3(rng, n=POOL):
    """SU(3) to rounding: QR of a Gaussian with the phases of R's diagonal and of the determinant divided out"""
    q, r = np.linalg.qr(_gauss(rng, n))
    d = np.diagonal(r, axis1=-2, axis2=-1)
    q = q * (d / np.abs(d))[:, None, :]
    return q / (np.linalg.det(q) ** (1.0 / 3.0))[:, None, None]


def _seed(name):
    return [ord(c) for c in name]


def unitary_pool():
    return random_su3(np.random.default_rng(_seed('unitary')))


def boundary_matrix(norm):
    """anti-Hermitian traceless with four entries of modulus norm / 2 and zeros elsewhere: its Frobenius norm is
    `norm` EXACTLY in fp64 for a power of two, however the squares are summed -- the frexp boundary itself"""
    a = np.zeros((3, 3), complex)
    h = norm / 2.0
    a[0, 1], a[1, 0], a[0, 2], a[2, 0] = h, -h, 1j * h, 1j * h
    return a


def expm_pool(name):
    """the 16 matrices A of an expm class"""
    rng = np.random.default_rng(_seed(name))
    kind, _, key = name.rpartition('_')
    if kind == 'alg':
        norm = ALGEBRA_NORMS[key]
        v = osu3.project_tah(_gauss(rng))
        a = v * (norm / np.sqrt((np.abs(v) ** 2).sum((-2, -1))))[:, None, None]
        if key in ('0.5', '1', '2', '4'):
            a[0] = boundary_matrix(norm)
        return a
    if kind == 'general':
        return _gauss(rng, scale=GENERAL_SCALES[key])
    th = THETAS[key]
    q = random_su3(rng)
    if kind == 'nilpotent':
        d = np.zeros((3, 3), complex)
        d[0, 1] = d[1, 2] = th
    else:
        d = 1j * th * np.diag({'degenerate': [1.0, 1.0, -2.0], 'zero_eig': [1.0, -1.0, 0.0],
                               'scalar': [1.0, 1.0, 1.0]}[kind]).astype(complex)
    return q @ d @ osu3.adj(q)


def _cond(x):
    s = np.linalg.svd(x, compute_uv=False)
    return s[..., 0] / s[..., -1]


def _rejection(rng, draw):
    out = []
    while len(out) < POOL:
        out += [m for m in draw(rng) if _cond(m) <= MAX_COND]
    return np.stack(out[:POOL])


def proj_pool(name):
    """the 16 matrices X of a projection class"""
    rng = np.random.default_rng(_seed(name))
    if name.startswith('sigma_'):
        s = np.diag(SIGMAS[name[len('sigma_'):]]).astype(complex)
        return random_su3(rng) @ s @ random_su3(rng)
    if name.startswith('near_unitary_'):
        return random_su3(rng) + _gauss(rng, scale=DELTAS[name[len('near_unitary_'):]])
    if name == 'gaussian':
        return _rejection(rng, _gauss)
    if name == 'tah_gaussian':
        return _rejection(rng, lambda r: osu3.project_tah(_gauss(r)))
    raise KeyError(name)


# ----------------------------------------------------------------------------------------- fields
def field_index(nf, V):
    """pool index of link (f, s) -> [nf, V]"""
    f, s = np.meshgrid(np.arange(nf), np.arange(V), indexing='ij')
    return (7 * f + 13 * s) % POOL


def field(pool, nf, V):
    """[nf, V, 3, 3] links drawn from the pool by field_index"""
    return pool[field_index(nf, V)]


def to_native(m):
    """[nf, V, 3, 3] -> native planes [nf, 9, V]"""
    nf, V = m.shape[:2]
    return np.ascontiguousarray(np.moveaxis(m.reshape(nf, V, 9), 1, 2))


def from_native(p):
    """[nf, 9, V] -> [nf, V, 3, 3]"""
    nf, _, V = p.shape
    return np.moveaxis(p, 1, 2).reshape(nf, V, 3, 3)


# ----------------------------------------------------------------------------------------- bounds
def fro(a):
    return np.sqrt((np.abs(a) ** 2).sum((-2, -1)))


def expm_unit(a, e):
    """u max(1, |A|_F) max(1, max|exp A|) per matrix: the unit the expm bound K is counted in"""
    return U * np.maximum(1.0, fro(a)) * np.maximum(1.0, np.abs(e).max((-2, -1)).astype(float))


def maxerr(got, truth):
    """max |got - truth| over the trailing 3x3 (or 8), formed in long double"""
    d = np.abs(np.asarray(got).astype(CLD) - truth)
    return d.reshape(d.shape[0], -1).max(-1).astype(float) if d.ndim > 1 else d.astype(float)


class Truth:
    """lazily computed, cached pools and truths: one instance per test module"""

    def __init__(self):
        self._c = {}

    def _get(self, key, make):
        if key not in self._c:
            self._c[key] = make()
        return self._c[key]

    def unitary(self):
        return self._get(('unitary',), unitary_pool)

    def unitary_su(self):
        return self._get(('unitary_su',), lambda: polar_su(self.unitary()))

    def expm_pool(self, name):
        return self._get(('ep', name), lambda: expm_pool(name))

    def proj_pool(self, name):
        return self._get(('pp', name), lambda: proj_pool(name))

    def expm(self, name, sign=1):
        if sign == -1 and name.startswith('alg_'):
            # project_tah output is anti-Hermitian bit for bit, so exp(-A) is exp(A)^H exactly
            return self._get(('e', name, -1), lambda: np.conj(np.swapaxes(self.expm(name, 1), -1, -2)))
        return self._get(('e', name, sign), lambda: expm(self.expm_pool(name), sign))

    def polar_u(self, name):
        return self._get(('pu', name), lambda: polar_u(self.proj_pool(name)))

    def polar_su(self, name):
        return self._get(('ps', name), lambda: polar_su(self.proj_pool(name)))

    def oracle_error(self, name, su=True):
        """class-maximum error of the reference's closed form (oracle.su3) against truth on the pool"""
        x = self.proj_pool(name)
        if su:
            return float(maxerr(osu3.project_su(x), self.polar_su(name)).max())
        return float(maxerr(osu3.project_u(x), self.polar_u(name)).max())

    def proj_tol(self, name, su=True):
        """max(4 x the oracle's own class-maximum error, 32 u); the class must sit inside the formula's domain"""
        e = self.oracle_error(name, su)
        assert e < 1e-10, f'{name}: the reference formula errs by {e:.2e} here -- outside its domain'
        return max(4.0 * e, 32.0 * U)


def measure():
    import time

    import torch
    t0 = time.time()
    tr = Truth()
    worst = worst_ah = 0.0
    print('torch.matrix_exp (CPU, complex128) against mpmath, in units of u max(1,|A|_F) max(1,max|exp A|):')
    for name in EXPM_CLASSES:
        a = tr.expm_pool(name)
        r = 0.0
        for sign in (1, -1):
            e = tr.expm(name, sign)
            got = torch.matrix_exp(torch.from_numpy(sign * a)).numpy()
            r = max(r, float((maxerr(got, e) / expm_unit(a, e)).max()))
        worst = max(worst, r)
        if name in EXPM_ANTIHERMITIAN:
            worst_ah = max(worst_ah, r)
        print(f'  {name:<18s} {r:8.3f}')
    print(f'worst ratio {worst:.3f}  ->  K = 4 x worst = {4 * worst:.2f}')
    print(f'worst ratio over the anti-Hermitian classes {worst_ah:.3f}  ->  K_normal = {4 * worst_ah:.2f}')
    print('oracle.su3 closed-form projection against mpmath (class maximum):')
    for name in PROJ_CLASSES:
        print(f'  {name:<22s} project_su {tr.oracle_error(name, True):9.2e}   project_u '
              f'{tr.oracle_error(name, False):9.2e}   max cond {float(_cond(tr.proj_pool(name)).max()):9.3g}')
    print(f'({time.time() - t0:.1f} s)')


if __name__ == '__main__':
    if '--measure' in sys.argv:
        measure()
    else:
        print(__doc__)
