"""TEST INFRASTRUCTURE: numpy restatement of the clover (Sheikholeslami-Wohlert) term and of the improved Wilson operator
with its asymmetric even-odd solve, built on `wr.hop` (tests/wilson_restatement.py) and the half-field helpers of
tests/wilson_eo_restatement.py.  Written from the formulas (include/l2q.h, "csrc/su3_wilson_clover.hip"), not from the
kernels:

    M_sw = A - kappa H,   A(x) = 1 + kappa c_sw i sum_{mu<nu} sigma_{mu nu} (x) Fhat_{mu nu}(x),
    sigma_{mu nu} = (i/2) [gamma_mu, gamma_nu] from wr.GAMMA,   Fhat_{mu nu} = (Q_{mu nu} - Q_{mu nu}^H) / 8,
    Q_{mu nu} the sum of the four leaves (np.roll products); Fhat keeps its trace.
    Mhat = A_ee - kappa^2 H_eo A_oo^-1 H_oe,  bhat_e = b_e + kappa H_eo A_oo^-1 b_o,  psi_o = A_oo^-1 (b_o + kappa H_oe psi_e).

A is held as a field of 12 x 12 matrices ``[nb, T, X, Y, Z, 12, 12]`` (index 3 spin + colour), built with np.kron from
sigma_{mu nu}, NOT from the block form; `block_form` is the block form, for the host test that compares the two.  Every
function computes in the type of its inputs (`measure()` runs the same expressions in np.clongdouble)."""
import functools

import numpy as np

import wilson_eo_restatement as we
import wilson_restatement as wr

KAPPA = wr.KAPPA
C_SWS = (1.0, 1.769)
C_SW_BAD = 10.0                  # on wr.links((4, 4, 4, 4)) A has a negative eigenvalue: the input of the min_pivot test


# ------------------------------------------------------------------ the clover term
def sigma(mu, nu, ct=complex):
    g = wr.GAMMA.astype(ct)
    return np.dtype(ct).type(0.5j) * (g[mu] @ g[nu] - g[nu] @ g[mu])


def _dag(m):
    return np.swapaxes(m.conj(), -1, -2)


def leaves(x, mu, nu):
    """Q_{mu nu} [nb, T, X, Y, Z, 3, 3]: the four leaves in the order L1..L4 of csrc/su3_flow.hip"""
    um, un = x[:, mu], x[:, nu]

    def sh(f, *steps):                                   # f(x + sum of steps), a step (direction, +-1)
        for d, s in steps:
            f = np.roll(f, -s, axis=1 + d)
        return f
    l1 = um @ sh(un, (mu, 1)) @ _dag(sh(um, (nu, 1))) @ _dag(un)
    l2 = un @ _dag(sh(um, (mu, -1), (nu, 1))) @ _dag(sh(un, (mu, -1))) @ sh(um, (mu, -1))
    l3 = _dag(sh(um, (mu, -1))) @ _dag(sh(un, (mu, -1), (nu, -1))) @ sh(um, (mu, -1), (nu, -1)) @ sh(un, (nu, -1))
    l4 = _dag(sh(un, (nu, -1))) @ sh(um, (nu, -1)) @ sh(un, (mu, 1), (nu, -1)) @ _dag(um)
    return l1 + l2 + l3 + l4


def fhat(x, mu, nu):
    q = leaves(x, mu, nu)
    return (q - _dag(q)) / x.real.dtype.type(8)


def clover(x, coef):
    """A [nb, T, X, Y, Z, 12, 12] = 1 + coef i sum_{mu<nu} kron(sigma_{mu nu}, Fhat_{mu nu}), coef = kappa c_sw"""
    ct = x.dtype
    a = np.zeros((*x.shape[:1], *x.shape[2:6], 12, 12), ct)
    for mu in range(4):
        for nu in range(mu + 1, 4):
            f = fhat(x, mu, nu)
            a += np.einsum('ab,ntxyzij->ntxyzaibj', sigma(mu, nu, ct), f).reshape(a.shape)
    return np.eye(12).astype(ct) + ct.type(1j) * x.real.dtype.type(coef) * a


def block_form(x, coef):
    """(A+, A-) [nb, T, X, Y, Z, 6, 6] from the block form: 1 -+ i coef sum_k sigma_k (x) (E_k +- B_k)"""
    ct = x.dtype
    e = [fhat(x, 0, k) for k in (1, 2, 3)]
    b = [fhat(x, 2, 3), -fhat(x, 1, 3), fhat(x, 1, 2)]
    out = []
    for sc, sb in ((-1.0, 1.0), (1.0, -1.0)):
        m = sum(np.einsum('ab,ntxyzij->ntxyzaibj', wr._S[k].astype(ct), e[k] + x.real.dtype.type(sb) * b[k])
                for k in range(3))
        m = m.reshape(*m.shape[:5], 6, 6)
        out.append(np.eye(6).astype(ct) + ct.type(1j) * x.real.dtype.type(sc * coef) * m)
    return out


def inverse(a):
    """A^-1 site by site (np.linalg.inv: complex128 only)"""
    return np.linalg.inv(a)


def apply_site(c, psi):
    """(C psi)(x) for a field of 12 x 12 matrices c and spinors psi [nb, nrhs, T, X, Y, Z, 4, 3]"""
    v = psi.reshape(*psi.shape[:6], 12)
    return np.einsum('ntxyzab,nrtxyzb->nrtxyza', c, v).reshape(psi.shape)


def pack_blocks(a):
    """the block field [nb, 2 parity, 2 chirality, 36, V/2] of A (or of any block-diagonal Hermitian site field): the 6
    diagonal entries, then (re, im) of the 15 entries above the diagonal, row-major; half index as `we.sites`"""
    nb, L = a.shape[0], a.shape[1:5]
    flat = a.reshape(nb, -1, 12, 12)
    iu = np.triu_indices(6, 1)
    out = np.empty((nb, 2, 2, 36, flat.shape[1] // 2), a.real.dtype)
    for p in (0, 1):
        s = we.sites(L, p)
        for chi in (0, 1):
            blk = flat[:, s, 6 * chi:6 * chi + 6, 6 * chi:6 * chi + 6]
            out[:, p, chi, :6] = np.moveaxis(np.diagonal(blk, axis1=-2, axis2=-1).real, -1, 1)
            up = blk[:, :, iu[0], iu[1]]                                          # [nb, Vh, 15]
            out[:, p, chi, 6::2] = np.moveaxis(up.real, -1, 1)
            out[:, p, chi, 7::2] = np.moveaxis(up.imag, -1, 1)
    return out


def unpack_blocks(cl, L):
    """the inverse of `pack_blocks`: [nb, T, X, Y, Z, 12, 12], Hermitian, zero between the chiralities"""
    nb = cl.shape[0]
    V = int(np.prod(L))
    flat = np.zeros((nb, V, 12, 12), complex)
    iu = np.triu_indices(6, 1)
    for p in (0, 1):
        s = we.sites(L, p)
        for chi in (0, 1):
            blk = np.zeros((nb, V // 2, 6, 6), complex)
            up = np.moveaxis(cl[:, p, chi, 6::2] + 1j * cl[:, p, chi, 7::2], 1, -1)
            blk[:, :, iu[0], iu[1]] = up
            blk[:, :, iu[1], iu[0]] = up.conj()
            blk[:, :, np.arange(6), np.arange(6)] = np.moveaxis(cl[:, p, chi, :6], 1, -1)
            flat[:, s, 6 * chi:6 * chi + 6, 6 * chi:6 * chi + 6] = blk
    return flat.reshape(nb, *L, 12, 12)


# ------------------------------------------------------------------ the operator and its even-odd form
def wilson_clover(x, psi, kappa, c_sw, dagger=False, antiperiodic_t=True, a=None):
    """M_sw psi (dagger: M_sw^H psi = gamma5 M_sw gamma5 psi); a: the clover term if already built"""
    if psi.ndim == 7:
        return wilson_clover(x, psi[:, None], kappa, c_sw, dagger, antiperiodic_t, a)[:, 0]
    a = clover(x, kappa * c_sw) if a is None else a
    return apply_site(a, psi) - psi.real.dtype.type(kappa) * wr.hop(x, psi, dagger, antiperiodic_t)


def hop_clover(x, src, p, c, cmode, dagger=False, antiperiodic_t=True, a=1.0, aux=None, b=0.0):
    """the one kernel: on the sites of parity p, zero elsewhere,
    cmode 0 b aux + a H src;  1 b (C aux) + a H src;  2 C (b aux + a H src)"""
    L = src.shape[2:6]
    rt = src.real.dtype.type
    m = we.mask(L, p)
    h = rt(a) * (wr.hop(x, src * we.mask(L, 1 - p), dagger, antiperiodic_t) * m)
    if cmode == 0:
        return h if aux is None else h + rt(b) * (aux * m)
    if cmode == 1:
        return h if aux is None else h + rt(b) * (apply_site(c, aux) * m)
    return apply_site(c, h if aux is None else h + rt(b) * (aux * m)) * m


def uses(kappa=KAPPA):
    """the uses (name, cmode, block 'a' / 'ainv' / None, output parity or None for both, a, b, aux given) of kernel 3"""
    return [('hop', 0, None, None, 1.0, 0.0, False), ('hop aux', 0, None, None, kappa, 1.0, True),
            ('schur first', 2, 'ainv', None, 1.0, 0.0, False), ('schur second', 1, 'a', None, -kappa * kappa, 1.0, True),
            ('reconstruct', 2, 'ainv', None, kappa, 1.0, True), ('full', 1, 'a', None, -kappa, 1.0, True)]


def schur_clover(x, psi, kappa, a, ainv, dagger=False, antiperiodic_t=True):
    """Mhat psi_e (dagger: Mhat^H psi_e) of the even part of psi; zero on the odd sites"""
    odd = hop_clover(x, psi, 1, ainv, 2, dagger, antiperiodic_t)
    return hop_clover(x, odd, 0, a, 1, dagger, antiperiodic_t, a=-kappa * kappa, aux=psi, b=1.0)


def prepare(x, b, kappa, ainv, antiperiodic_t=True):
    """bhat_e = b_e + kappa H_eo A_oo^-1 b_o"""
    L = b.shape[2:6]
    return hop_clover(x, apply_site(ainv, b) * we.mask(L, 1), 0, None, 0, False, antiperiodic_t, a=kappa, aux=b, b=1.0)


def reconstruct(x, pe, b, kappa, ainv, antiperiodic_t=True):
    """psi = psi_e + A_oo^-1 (b_o + kappa H_oe psi_e)"""
    return pe + hop_clover(x, pe, 1, ainv, 2, False, antiperiodic_t, a=kappa, aux=b, b=1.0)


def solve_clover(x, b, kappa, c_sw, tol=1e-10, max_iter=1000, check_every=10, antiperiodic_t=True):
    """M_sw psi = b through the asymmetric Schur complement, by `wr.cgnr_op` on Mhat from zero, stopping on |rhat|^2 <=
    tol^2 |b|^2 (|b|^2 of the full right-hand side).  (psi, info); info['residual'] is the full |b - M_sw psi| / |b|."""
    L = b.shape[2:6]
    a = clover(x, kappa * c_sw)
    ainv = inverse(a)
    bb = wr.norm2(b)
    bhat = prepare(x, b, kappa, ainv, antiperiodic_t)
    pe, iters, done = wr.cgnr_op(lambda p, d: schur_clover(x, p, kappa, a, ainv, d, antiperiodic_t), bhat, bb, tol,
                                 max_iter, check_every)
    psi = reconstruct(x, pe * we.mask(L, 0), b, kappa, ainv, antiperiodic_t)
    res = np.sqrt(wr.norm2(b - wilson_clover(x, psi, kappa, c_sw, False, antiperiodic_t, a)) / np.where(bb > 0, bb, 1.0))
    return psi, {'iters': iters, 'residual': res, 'converged': done}


def dense(x, kappa, c_sw, antiperiodic_t=True):
    """M_sw of chain 0 of x as a dense matrix [12 V, 12 V] in the index order (t, x, y, z, spin, colour)"""
    L = x.shape[2:6]
    n = 12 * int(np.prod(L))
    basis = np.eye(n, dtype=complex).reshape(1, n, *L, 4, 3)
    return wilson_clover(x[:1], basis, kappa, c_sw, False, antiperiodic_t).reshape(n, n).T


def logdet(a):
    """log det A per (chain, parity): [nb, 2]"""
    nb, L = a.shape[0], a.shape[1:5]
    ld = np.linalg.slogdet(a)[1].reshape(nb, -1)
    return np.stack([ld[:, we.sites(L, p)].sum(1) for p in (0, 1)], 1)


def pivots(a):
    """the pivots d_i of the unpivoted L D L^H of both blocks, [nb, T, X, Y, Z, 12]: the squared diagonal of the Cholesky
    factor (positive-definite blocks only)"""
    return np.concatenate([np.diagonal(np.linalg.cholesky(a[..., s, s]), axis1=-2, axis2=-1).real ** 2
                           for s in (slice(0, 6), slice(6, 12))], -1)


def half_min(f, p):
    """the smallest entry of a site field [nb, T, X, Y, Z, ...] over the sites of parity p: [nb]"""
    nb, L = f.shape[0], f.shape[1:5]
    return f.reshape(nb, int(np.prod(L)), -1)[:, we.sites(L, p)].min((1, 2))


# Relative bound on a pivot of the L D L^H of a 6 x 6 block against the same pivot from another factorisation: the
# backward error of either is gamma_7 |L| |D| |L^H| (Higham, Accuracy and Stability, thm 10.3), u = 2^-53, times 2 sqrt 2
# for complex products; a relative change of A moves a pivot (a ratio of leading minors) by at most the condition
# number times it, cond < 4 on the test inputs (0.5 < eig < 2, asserted in test_wilson_clover_host.py); two computations.
PIVOT_BOUND = 2.0 * 7 * 2.0 * 2.0 ** 0.5 * 4.0 * 2.0 ** -53


def logdet_tol(nterms, sum_abs):
    """absolute bound on sum log d_i over nterms pivots in any order against slogdet: every log d_i carries the relative
    error of its pivot as an absolute one (PIVOT_BOUND each; slogdet's LU has the same), and the sum itself (nterms - 1)
    u relative to sum |log d_i| plus the rounding of the terms, doubled as in `wr.norm_bound`"""
    return nterms * PIVOT_BOUND + 2.0 * nterms * 2.0 ** -53 * sum_abs


# ------------------------------------------------------------------ the inputs
@functools.lru_cache(maxsize=None)
def _hot(L, nb):
    rng = np.random.default_rng(4242 + 1000 * L[0] + 100 * L[1] + 10 * L[2] + L[3])
    z = rng.standard_normal((nb, 4, *L, 3, 3)) + 1j * rng.standard_normal((nb, 4, *L, 3, 3))
    q, r = np.linalg.qr(z)
    d = np.diagonal(r, axis1=-2, axis2=-1)
    q = q * (d / np.abs(d))[..., None, :]                                        # Haar on U(3)
    return q / np.linalg.det(q)[..., None, None] ** (1.0 / 3.0)                  # ... on SU(3)


def hot_links(L, nb=3):
    """Haar-random links from a seed fixed by the lattice; fewer chains are the first ones of three"""
    return _hot(tuple(L), 3)[:nb].copy()


INPUTS = {'smooth': wr.links, 'hot': hot_links}
NB, NRHS = 2, 3                                                                  # of the kernel tests


def fields(kind, L, c_sw, nb=NB):
    """(x, a, ainv) of a test input"""
    x = INPUTS[kind](L, nb)
    a = clover(x, KAPPA * c_sw)
    return x, a, inverse(a)


def min_eig(a):
    return float(np.linalg.eigvalsh(a).min())


# Yardsticks: the largest element-wise distance between this restatement in complex128 and the same functions on the
# same inputs in np.clongdouble, over we.EO_GPU_LATTICES and (4, 4, 4, 4), both inputs ('smooth' = wr.links, 'hot'), both
# C_SWS, nb = NB, nrhs = NRHS, all four wr.FLAGS, both parities (`python tests/wilson_clover_restatement.py --measure`):
#   A       the entries of the clover term `clover`;
#   HOP     one application of `hop_clover` per use of `uses()` (the block C the same float64 numbers on both sides);
#   M       M_sw psi by `wilson_clover`;
#   INV     max |A A^-1 - 1| of np.linalg.inv on the same blocks, the product formed in np.clongdouble.
# Measured per lattice (worst over inputs, c_sw, flags):
#   (2,2,2,2)   A 1.29e-16  HOP 5.63e-15  M 1.30e-15  INV 5.27e-16
#   (4,2,6,2)   A 1.42e-16  HOP 5.69e-15  M 1.25e-15  INV 4.66e-16
#   (2,4,2,6)   A 1.37e-16  HOP 6.68e-15  M 1.37e-15  INV 4.95e-16
#   (4,4,4,8)   A 1.58e-16  HOP 6.70e-15  M 1.84e-15  INV 5.00e-16
#   (4,4,4,10)  A 1.46e-16  HOP 7.66e-15  M 2.06e-15  INV 5.02e-16
#   (4,4,4,4)   A 1.73e-16  HOP 7.51e-15  M 1.57e-15  INV 4.85e-16
# worst A 1.73e-16 (the entries of A - 1 are below 0.3), HOP 7.66e-15 (the use a = 1: |out| up to ~40), M 2.06e-15, INV
# 5.27e-16.
# The tolerances are 32 x these, the margin of the other Wilson tests: they cover fma contraction and the order of the
# kernels' sums and nothing else.  tests/test_wilson_clover_host.py measures the small lattices again and holds them to
# these figures.
YARD_A = 1.8e-16
YARD_HOP = 7.7e-15
YARD_M = 2.1e-15
YARD_INV = 5.3e-16
TOL_A, TOL_HOP, TOL_M, TOL_INV = (32.0 * y for y in (YARD_A, YARD_HOP, YARD_M, YARD_INV))
MEASURE_LATTICES = we.EO_GPU_LATTICES + [(4, 4, 4, 4)]


def inv_defect(a, ainv):
    """max |A Ainv - 1| with the product in np.clongdouble"""
    d = np.matmul(a.astype(np.clongdouble), ainv.astype(np.clongdouble)) - np.eye(12)
    return float(np.abs(d).max())


def measure_one(L, kind, c_sw, nb=NB, nrhs=NRHS):
    """the four yardsticks on one input"""
    ld = np.longdouble
    x, a, ainv = fields(kind, L, c_sw, nb)
    psi, aux = wr.spinors(L, nb, nrhs), we.aux_field(L, nb, nrhs)
    xl, pl, al = (t.astype(np.clongdouble) for t in (x, psi, aux))
    blocks = {'a': a, 'ainv': ainv, None: None}
    wide = {k: (None if v is None else v.astype(np.clongdouble)) for k, v in blocks.items()}
    out = {'A': float(np.abs(a - clover(xl, ld(KAPPA) * ld(c_sw))).max()), 'HOP': 0.0, 'M': 0.0,
           'INV': inv_defect(a, ainv)}
    for dagger, ap in wr.FLAGS:
        d = wilson_clover(x, psi, KAPPA, c_sw, dagger, ap, a) - wilson_clover(xl, pl, ld(KAPPA), ld(c_sw), dagger, ap)
        out['M'] = max(out['M'], float(np.abs(d).max()))
        for _, cmode, blk, _, ca, cb, with_aux in uses():
            for p in (0, 1):
                d = hop_clover(x, psi, p, blocks[blk], cmode, dagger, ap, ca, aux if with_aux else None, cb) \
                    - hop_clover(xl, pl, p, wide[blk], cmode, dagger, ap, ld(ca), al if with_aux else None, ld(cb))
                out['HOP'] = max(out['HOP'], float(np.abs(d).max()))
    return out


def measure(lattices=None):
    worst = {}
    for L in lattices or MEASURE_LATTICES:
        here = {}
        for kind in INPUTS:
            for c_sw in C_SWS:
                for k, v in measure_one(L, kind, c_sw).items():
                    here[k] = max(here.get(k, 0.0), v)
        print(L, {k: f'{v:.3g}' for k, v in here.items()}, flush=True)
        worst = {k: max(worst.get(k, 0.0), v) for k, v in here.items()}
    print('worst:', {k: f'{v:.3g}' for k, v in worst.items()})
    return worst


def measure_eigs():
    for kind in INPUTS:
        for c_sw in C_SWS + (C_SW_BAD,):
            for L in MEASURE_LATTICES:
                print('min eig', kind, c_sw, L, f'{min_eig(clover(INPUTS[kind](L, NB), KAPPA * c_sw)):.3f}')


def measure_iters():
    """iteration counts with and without the clover term, check_every = 1 (profiles/su3_wilson_clover.md)"""
    for L in we.SOLVE_LATTICES:
        x, b = wr.links(L, 2), wr.spinors(L, 2, 2)
        for kappa in wr.SOLVE_KAPPAS:
            eo = we.solve_eo(x, b, kappa, check_every=1)[1]['iters']
            row = [f'plain {eo.min()}-{eo.max()}']
            for c_sw in C_SWS:
                it = solve_clover(x, b, kappa, c_sw, check_every=1)[1]
                row.append(f"c_sw {c_sw}: {it['iters'].min()}-{it['iters'].max()} (residual {it['residual'].max():.2g})")
            print('iters', L, kappa, *row, flush=True)


if __name__ == '__main__':
    import sys
    if '--measure' in sys.argv:
        measure()
    if '--measure-eigs' in sys.argv:
        measure_eigs()
    if '--measure-iters' in sys.argv:
        measure_iters()
