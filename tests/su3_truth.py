"""High-precision truth for the per-link SU(3) routines of csrc/su3_math.hpp (TEST INFRASTRUCTURE, CPU only).

Every value here comes from mpmath at 60 digits, never from another fp64 routine:

  expm      mp.expm
  polar_u   X (X^H X)^(-1/2) from mp.eigh of X^H X -- deliberately NOT the cubic closed form the kernels and
            oracle/su3.py share
  polar_su  polar_u times exp(-i arg(det) / 3)
  tah       (X - X^H)/2 - tr(.)/3
  mul       the four products op(A) op(B), op = identity or adjoint
  vec8      oracle.su3.su3_to_vec of the truth projection (linear: adds no error that matters)
  frechet   L_exp(A)[G] as the upper-right 3x3 block of mp.expm([[A, G], [0, A]]): valid for any complex A and
            shares nothing with the kernels' Cayley-Hamilton recursion; the cotangent identity of the VJP kernels
            is g_A = L_exp(A^H)[g_E] (expm_vjp).  L is complex-linear in G: the nine basis responses L[e_ab] of a
            pool matrix (frechet_basis) combine to any direction in long double (combine)
  projsu_vec8_vjp   the VJP of vec8(polar_su(M)) by central differences (step 1e-20, 18 real directions) of the
            same mp.eigh projection -- not the cubic and not a Sylvester solve.  Singular M is excluded.

Cotangents come from deterministic pools of 16 as well (complex Gaussian g per link, real Gaussian g_y[8], and a
non-zero start for the accumulating outputs), indexed like the inputs: the triples (x_k, A_k, g_k) repeat with
period 16 and every truth is computed at pool size.

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
of oracle.su3.project_su / project_u against truth per projection class.  For tests/test_su3_vjp_*.py it goes on to
print the error ratio of torch.autograd.grad over torch.matrix_exp against the Frechet truth per expm class (K_L)
and that of the numpy fp64 restatement projsu_vec8_vjp_numpy against the projection VJP's truth per class (K_P),
asserting that the restatement stays below 32 units everywhere.
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
# the projection VJP also takes exactly unitary input (unitary_pool): every v-net call of the training path
PROJ_VJP_CLASSES = PROJ_CLASSES + ['unitary']
# the classes whose nine basis responses are computed (masked directions differ from site to site)
BASIS_CLASSES = ['alg_0', 'alg_1e-300', 'alg_0.25', 'alg_0.5+ulp', 'alg_4', 'alg_1e3', 'degenerate_1', 'nilpotent_30',
                 'general_3']
# singular values well apart: the only classes on which autograd over the closed form is a meaningful comparison
PROJ_SEPARATED = ['sigma_3_1_0.1', 'sigma_1_0.1_0.01', 'sigma_1e-3_2e-3_3e-3', 'sigma_1e3_2e3_5e2', 'gaussian',
                  'tah_gaussian']


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


# ----------------------------------------------------------------------------------------- the truths: VJPs
def _mp_block_expm(a, g):
    """(exp A, L_exp(A)[G]) as the upper-left and upper-right 3x3 blocks of mp.expm([[A, G], [0, A]])"""
    z = mp.zeros(6)
    for i in range(3):
        for j in range(3):
            z[i, j] = z[i + 3, j + 3] = a[i, j]
            z[i, j + 3] = g[i, j]
    e = mp.expm(z)
    return e[0:3, 0:3], e[0:3, 3:6]


def frechet(pa, pg, py=None):
    """(exp A, L_exp(A)[G]) of every pool triple, each [16, 3, 3] clongdouble.  G is pg itself or, with py given,
    the product g y^H of the fp64 matrices formed inside mpmath, i.e. without a rounding of its own."""
    es, ls = [], []
    with mp.workdps(DPS):
        for k in range(len(pa)):
            g = _to_mp(pg[k])
            if py is not None:
                g = g * _to_mp(py[k]).H
            e, l = _mp_block_expm(_to_mp(pa[k]), g)
            es.append(_from_mp(e))
            ls.append(_from_mp(l))
    return np.stack(es), np.stack(ls)


def expm_vjp(pa, pg, py=None):
    """the cotangent identity the kernels use: for E = exp(A) and a cotangent g_E, g_A = L_exp(A^H)[g_E]
    -> (exp(A^H), g_A)"""
    return frechet(np.conj(np.swapaxes(pa, -1, -2)), pg, py)


def frechet_basis(pa):
    """the nine basis responses L_exp(+-A_k)[e_ab] of every pool matrix -> two [16, 9, 3, 3] clongdouble (for +A
    and for -A), the response to e_ab at index 3 a + b.  L is complex-linear in its direction, so any direction
    is combined from these in long double (``combine``).  The -A half costs no further 6x6 exponential: from
    exp(-(A + t G)) = exp(A + t G)^-1,  L_exp(-A)[G] = exp(-A) L_exp(A)[G] exp(-A),  evaluated at 60 digits."""
    plus, minus = [], []
    with mp.workdps(DPS):
        for k in range(len(pa)):
            a = _to_mp(pa[k])
            ei = mp.expm(-a)
            rp, rm = [], []
            for ab in range(9):
                g = mp.zeros(3)
                g[ab // 3, ab % 3] = 1
                l = _mp_block_expm(a, g)[1]
                rp.append(_from_mp(l))
                rm.append(_from_mp(ei * l * ei))
            plus.append(np.stack(rp))
            minus.append(np.stack(rm))
    return np.stack(plus), np.stack(minus)


def combine(basis, g):
    """L[G] = sum_ab G_ab L[e_ab] in long double: basis [..., 9, 3, 3], g [..., 3, 3] -> [..., 3, 3]"""
    g = np.asarray(g).astype(CLD)
    return (g.reshape(g.shape[:-2] + (9, 1, 1)) * basis).sum(-3)


def _mp_vec8(m):
    """oracle.su3.su3_to_vec restated for an mpmath matrix"""
    s = 1 / mp.sqrt(3)
    return [-2 * m[0, 1].imag, -2 * m[0, 1].real, m[1, 1].imag - m[0, 0].imag, -2 * m[0, 2].imag,
            -2 * m[0, 2].real, -2 * m[1, 2].imag, -2 * m[1, 2].real,
            s * (2 * m[2, 2].imag - m[1, 1].imag - m[0, 0].imag)]


FD_STEP = '1e-20'


def _mp_projsu_vec8_vjp(m, gy):
    """g_M = d phi / d Re M + i d phi / d Im M of phi(M) = g_y . vec8(polar_su(M)) by central differences with
    step 1e-20 over the 18 real directions, at 60 digits: truncation ~ h^2 = 1e-40, rounding ~ 1e-60 / h"""
    h = mp.mpf(FD_STEP)

    def phi(x):
        y = _mp_vec8(_mp_polar_su(x))
        return mp.fsum(gy[a] * y[a] for a in range(8))
    out = mp.zeros(3)
    for i in range(3):
        for j in range(3):
            d = []
            for step in (h, mp.mpc(0, h)):
                p, q = m.copy(), m.copy()
                p[i, j] += step
                q[i, j] -= step
                d.append((phi(p) - phi(q)) / (2 * h))
            out[i, j] = mp.mpc(d[0], d[1])
    return out


def projsu_vec8_vjp(pm, pgy):
    """VJP of vec8(polar_su(M)) for every pool pair (M [16, 3, 3], g_y [16, 8]) -> [16, 3, 3] clongdouble"""
    with mp.workdps(DPS):
        return np.stack([_from_mp(_mp_projsu_vec8_vjp(_to_mp(pm[k]), [mp.mpf(float(t)) for t in pgy[k]]))
                         for k in range(len(pm))])


_VEC8_MAP = None


def vec8_adjoint(gy):
    """g_W of y = su3_to_vec(W) for the cotangent g_y [..., 8] -> [..., 3, 3]: the map is real-linear, its matrix is
    read off oracle.su3.su3_to_vec at the 18 unit matrices"""
    global _VEC8_MAP
    if _VEC8_MAP is None:
        e = np.eye(9).reshape(9, 3, 3)
        _VEC8_MAP = osu3.su3_to_vec(e.astype(complex)) + 1j * osu3.su3_to_vec(1j * e)          # [9, 8]
    return (np.asarray(gy)[..., None, :] * _VEC8_MAP).sum(-1).reshape(np.shape(gy)[:-1] + (3, 3))


def projsu_vec8_vjp_numpy(m, gy):
    """Plain numpy fp64 restatement of the same derivative, the yardstick of the projection VJP's tolerance:
    polar_su(M) = W = U e^{i theta}, M = U H with U from numpy.linalg.svd and H = U^H M, theta = -arg(det U) / 3;
    g_U = e^{-i theta} g_W - (c / 3) i U with c = Re tr(g_W^H i W);  g_M = U (K - K^H) with H K + K H = U^H g_U
    solved in numpy.linalg.eigh's basis of H.  H is NOT taken as (M^H M)^(1/2): the squared matrix holds a small
    singular value only to u (sigma_max / sigma)^2, which at (1, 0.1, 0.01) costs 40 of the units the result is
    counted in.  m [..., 3, 3], gy [..., 8] -> [..., 3, 3] complex128."""
    adj = lambda x: np.conj(np.swapaxes(x, -1, -2))
    p, _, qh = np.linalg.svd(m)
    u = p @ qh
    h = adj(u) @ m
    h, v = np.linalg.eigh(0.5 * (h + adj(h)))
    theta = -np.angle(np.linalg.det(u)) / 3.0
    ph = np.exp(1j * theta)[..., None, None]
    gw = vec8_adjoint(gy)
    c = np.einsum('...ij,...ij->...', np.conj(gw), 1j * u * ph).real
    gu = np.conj(ph) * gw - (c / 3.0)[..., None, None] * 1j * u
    z = adj(v) @ (adj(u) @ gu) @ v
    k = v @ (z / (h[..., :, None] + h[..., None, :])) @ adj(v)
    return u @ (k - adj(k))


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


def cotangent_pool():
    """complex Gaussian link cotangents g, one per pool place"""
    return _gauss(np.random.default_rng(_seed('cotangent')))


def accumulator_pool():
    """what the accumulating outputs (g_v, g_M) hold before the call"""
    return _gauss(np.random.default_rng(_seed('accumulator')))


def vec8_cotangent_pool():
    """real Gaussian cotangents g_y[8] of the vec8 output"""
    return np.random.default_rng(_seed('vec8_cotangent')).normal(size=(POOL, 8))


def direction_pool():
    """fp64 directions G_k = g_k x_k^H (rounded once, here) for the host tier, where G is an operand"""
    return cotangent_pool() @ osu3.adj(unitary_pool())


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
    if name == 'unitary':
        return unitary_pool()
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

    # ---- VJPs.  Every pool place k holds one triple (x_k, A_k, g_k): a field filled by field_index repeats them
    def cotangent(self):
        return self._get(('cot',), cotangent_pool)

    def accumulator(self):
        return self._get(('acc',), accumulator_pool)

    def vec8_cotangent(self):
        return self._get(('cot8',), vec8_cotangent_pool)

    def direction(self):
        return self._get(('dir',), direction_pool)

    def frechet_host(self, name):
        """(exp B, L_exp(B)[G]) at B = A^H and the fp64 direction pool: what the host driver is handed"""
        return self._get(('fh', name), lambda: expm_vjp(self.expm_pool(name), self.direction()))

    def frechet_basis(self, name, sign=1):
        """basis responses of L_exp((sign A)^H) -> [16, 9, 3, 3]"""
        def make():
            return frechet_basis(np.conj(np.swapaxes(self.expm_pool(name), -1, -2)))
        return self._get(('fb', name), make)[0 if sign == 1 else 1]

    def expm_vjp(self, name, sign=1):
        """g_A = L_exp((sign A)^H)[g x^H] of the pool triples, the product g x^H exact -> [16, 3, 3]"""
        def make():
            g, x = self.cotangent(), self.unitary()
            if name in BASIS_CLASSES:
                return combine(self.frechet_basis(name, sign), g.astype(CLD) @ np.conj(np.swapaxes(x, -1, -2)))
            return expm_vjp(sign * self.expm_pool(name), g, x)[1]
        return self._get(('ev', name, sign), make)

    def frechet_norm(self, name, sign=1):
        """Frobenius norm of L_exp((sign A)^H) as a 9x9 matrix (>= its operator norm) per pool matrix, from fp64
        block exponentials: it only scales the small direction-rounding term of the bounds"""
        def make():
            import torch
            a = sign * np.conj(np.swapaxes(self.expm_pool(name), -1, -2))
            z = np.zeros((POOL, 9, 6, 6), complex)
            z[:, :, :3, :3] = z[:, :, 3:, 3:] = a[:, None]
            z[:, :, :3, 3:] = np.eye(9).reshape(9, 3, 3)
            l = torch.matrix_exp(torch.from_numpy(z)).numpy()[:, :, :3, 3:]
            return np.sqrt((np.abs(l) ** 2).sum((-3, -2, -1)))
        return self._get(('fn', name, sign), make)

    def projsu_vec8_vjp(self, name):
        return self._get(('pv', name), lambda: projsu_vec8_vjp(self.proj_pool(name), self.vec8_cotangent()))

    def proj_vjp_unit(self, name):
        """u |g_y|_2 (sigma_max / sigma_min) / sigma_min per pool matrix: the polar factor's derivative norm
        ~ 1 / sigma_min times the conditioning of the eigenproblem behind it"""
        s = np.linalg.svd(self.proj_pool(name), compute_uv=False)
        return U * np.sqrt((self.vec8_cotangent() ** 2).sum(-1)) * s[:, 0] / s[:, -1] ** 2

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
    measure_vjp()


def measure_vjp():
    """the two yardsticks of tests/test_su3_vjp_*.py"""
    import time

    import torch

    import emu_native
    t0 = time.time()
    tr = Truth()
    g = tr.direction()
    worst = worst_ah = 0.0
    print('torch.autograd.grad over torch.matrix_exp (CPU, complex128) against mpmath, g_A = L_exp(A^H)[G], in units '
          'of u max(1,|A|_F) max(1,max|exp A|) |G|_F:')
    for name in EXPM_CLASSES:
        r = 0.0
        for sign in (1, -1):
            a = sign * tr.expm_pool(name)
            e, l = tr.frechet_host(name) if sign == 1 else expm_vjp(a, g)
            ar = torch.from_numpy(a).requires_grad_(True)
            (got,) = torch.autograd.grad(torch.matrix_exp(ar), ar, torch.from_numpy(g))
            r = max(r, float((maxerr(got.numpy(), l) / (expm_unit(a, e) * fro(g))).max()))
        worst = max(worst, r)
        if name in EXPM_ANTIHERMITIAN:
            worst_ah = max(worst_ah, r)
        print(f'  {name:<18s} {r:8.3f}')
    print(f'worst ratio {worst:.3f}  ->  K_L = 4 x worst = {4 * worst:.2f}')
    print(f'worst ratio over the anti-Hermitian classes {worst_ah:.3f}  ->  K_L_normal = {4 * worst_ah:.2f}')
    print('numpy fp64 restatement of the projectSU -> vec8 VJP against mpmath, in units of '
          'u |g_y|_2 (sigma_max / sigma_min) / sigma_min (class maximum):')
    gy = tr.vec8_cotangent()
    worst = 0.0
    for name in PROJ_VJP_CLASSES:
        m = tr.proj_pool(name)
        r = float((maxerr(projsu_vec8_vjp_numpy(m, gy), tr.projsu_vec8_vjp(name)) / tr.proj_vjp_unit(name)).max())
        worst = max(worst, r)
        line = f'  {name:<22s} {r:8.3f}'
        if name in PROJ_SEPARATED:
            mr = torch.from_numpy(m).requires_grad_(True)
            (ref,) = torch.autograd.grad(emu_native._to_vec8(emu_native._proj_su(mr)), mr, torch.from_numpy(gy))
            ra = float((maxerr(ref.numpy(), tr.projsu_vec8_vjp(name)) / tr.proj_vjp_unit(name)).max())
            line += f'   (autograd over the closed form: {ra:.3g})'
        print(line)
        assert r < 32.0, f'{name}: the restatement errs by {r:.1f} units here -- outside the formula\'s domain'
    print(f'worst ratio {worst:.3f}  ->  K_P = max(4 x worst, 32) = {max(4 * worst, 32.0):.2f}')
    print(f'({time.time() - t0:.1f} s)')


if __name__ == '__main__':
    if '--measure' in sys.argv:
        measure()
    else:
        print(__doc__)
