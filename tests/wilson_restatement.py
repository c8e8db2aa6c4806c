"""TEST INFRASTRUCTURE: numpy restatement of the Wilson-Dirac operator, its CGNR solve, the point-source propagator and
the pion correlator, vectorised over sites with `np.roll` shifts and `einsum`, written from the formulas (include/l2q.h,
"SU(3) Wilson fermions"), not from the kernels.  Links ``x[nb, 4, T, X, Y, Z, 3, 3]``, spinors ``psi[nb, nrhs, T, X, Y,
Z, 4, 3]`` (spin, then colour), complex128 -- or any other complex type: every function computes in the type of its
inputs, which is how `measure()` evaluates the same expressions in extended precision.

    M psi = psi - kappa H psi,
    H psi(x) = sum_mu [(1 - gamma_mu) U_mu(x) psi(x+mu) + (1 + gamma_mu) U_mu(x-mu)^H psi(x-mu)],
    M^H = gamma5 M gamma5: the projector signs swapped.
Periodic, except that with `antiperiodic_t` every hop across the t = T-1 -> 0 seam takes a factor -1."""
import numpy as np

import smear_restatement as sm

# ------------------------------------------------------------------ the gamma matrices: Hermitian, chiral
_S = [np.array([[0, 1], [1, 0]], complex), np.array([[0, -1j], [1j, 0]], complex), np.array([[1, 0], [0, -1]], complex)]
_B = [np.eye(2, dtype=complex)] + [-1j * s for s in _S]                       # gamma_mu = [[0, B_mu], [B_mu^H, 0]]


def gamma_matrices():
    """[5, 4, 4]: gamma_0 (T), gamma_1, gamma_2, gamma_3 (x, y, z) and gamma5 = g0 g1 g2 g3"""
    g = np.zeros((5, 4, 4), complex)
    for mu in range(4):
        g[mu, :2, 2:] = _B[mu]
        g[mu, 2:, :2] = _B[mu].conj().T
    g[4] = g[0] @ g[1] @ g[2] @ g[3]
    return g


GAMMA = gamma_matrices()


# ------------------------------------------------------------------ the operator
def hop(x, psi, dagger=False, antiperiodic_t=True):
    """H psi (dagger: gamma5 H gamma5 psi)"""
    ct = psi.dtype
    sg = -1.0 if dagger else 1.0
    eye = np.eye(4).astype(ct)
    out = np.zeros_like(psi)
    for mu in range(4):
        g = GAMMA[mu].astype(ct)
        u = x[:, mu]
        f = np.roll(psi, -1, axis=2 + mu)                                     # psi(x + mu)
        if antiperiodic_t and mu == 0:
            f = f.copy()
            f[:, :, -1] = -f[:, :, -1]
        out += np.einsum('ad,brtxyzdc->brtxyzac', eye - sg * g, np.einsum('btxyzij,brtxyzaj->brtxyzai', u, f))
        w = np.einsum('btxyzji,brtxyzaj->brtxyzai', u.conj(), psi)            # U_mu(x)^H psi(x), moved to x + mu
        w = np.roll(w, 1, axis=2 + mu)
        if antiperiodic_t and mu == 0:
            w[:, :, 0] = -w[:, :, 0]
        out += np.einsum('ad,brtxyzdc->brtxyzac', eye + sg * g, w)
    return out


def wilson(x, psi, kappa, dagger=False, antiperiodic_t=True):
    """M psi (dagger: M^H psi); psi with or without the nrhs axis"""
    if psi.ndim == 7:
        return wilson(x, psi[:, None], kappa, dagger, antiperiodic_t)[:, 0]
    return psi - psi.real.dtype.type(kappa) * hop(x, psi, dagger, antiperiodic_t)


def norm2(psi):
    """|psi|^2 per system, [nb, nrhs]"""
    return (psi.real ** 2 + psi.imag ** 2).sum(axis=tuple(range(2, psi.ndim)))


def dense(x, kappa, antiperiodic_t=True):
    """M of chain 0 of x as a dense matrix [12 V, 12 V] in the index order (t, x, y, z, spin, colour)"""
    L = x.shape[2:6]
    n = 12 * int(np.prod(L))
    basis = np.eye(n, dtype=complex).reshape(1, n, *L, 4, 3)
    return wilson(x[:1], basis, kappa, False, antiperiodic_t).reshape(n, n).T


def free_wave(L, kappa, n, ap):
    """a plane wave of momentum p times a constant spinor on unit links: (|M psi|^2 / |psi|^2, the formula)"""
    p = [2 * np.pi * n[mu] / L[mu] for mu in range(4)]
    if ap:
        p[0] = (2 * n[0] + 1) * np.pi / L[0]
    grids = np.meshgrid(*[np.arange(e) for e in L], indexing='ij')
    wave = np.exp(1j * sum(pm * c for pm, c in zip(p, grids)))
    rng = np.random.default_rng(5)
    const = rng.standard_normal((4, 3)) + 1j * rng.standard_normal((4, 3))
    psi = (wave[..., None, None] * const)[None, None]
    x = np.broadcast_to(np.eye(3, dtype=complex), (1, 4, *L, 3, 3)).copy()
    want = (1 - 2 * kappa * sum(np.cos(p))) ** 2 + 4 * kappa ** 2 * sum(np.sin(pm) ** 2 for pm in p)
    return x, psi, want


# ------------------------------------------------------------------ the solver
def _bc(a):
    return a.reshape(a.shape + (1,) * 6)


def cgnr_op(op, b, bb, tol=1e-10, max_iter=1000, check_every=10):
    """A psi = b by CG on A^H A with the true residual r = b - A psi carried along, op(p, dagger) the operator; per
    system alpha = |z|^2 / |A p|^2.  Convergence |r|^2 <= tol^2 bb (bb [nb, nrhs], the reference norm) is looked at every
    check_every iterations (and at 0 and max_iter); a converged system takes alpha = beta = 0 from then on.  Returns
    (psi, iters, done)."""
    psi = np.zeros_like(b)
    r = b.copy()
    z = op(r, True)
    p = z.copy()
    zz = norm2(z)
    rr = norm2(b)
    done = bb <= tol * tol * bb
    iters = np.where(done, 0, max_iter)
    k = 0
    while k < max_iter and not done.all():
        q = op(p, False)
        qq = norm2(q)
        live = ~done & (qq > 0)
        alpha = np.where(live, zz / np.where(live, qq, 1.0), 0.0)
        psi = psi + _bc(alpha) * p
        r = r - _bc(alpha) * q
        rr = norm2(r)
        z = op(r, True)
        zn = norm2(z)
        live = ~done & (zz > 0)
        beta = np.where(live, zn / np.where(live, zz, 1.0), 0.0)
        p = z + _bc(beta) * p
        zz = zn
        k += 1
        if k % check_every == 0 or k == max_iter:
            now = ~done & (rr <= tol * tol * bb)
            iters = np.where(now, k, iters)
            done = done | now
    return psi, iters, done


def cgnr(x, b, kappa, tol=1e-10, max_iter=1000, check_every=10, antiperiodic_t=True):
    """M psi = b by `cgnr_op` on M, stopping on |r|^2 <= tol^2 |b|^2; b with or without the nrhs axis.  Returns (psi,
    info), info = {'iters', 'residual', 'converged'} each [nb, nrhs]; residual is |b - M psi| / |b| recomputed at the
    end (0 for b = 0)."""
    squeeze = b.ndim == 7
    if squeeze:
        b = b[:, None]
    bb = norm2(b)
    psi, iters, done = cgnr_op(lambda p, d: wilson(x, p, kappa, d, antiperiodic_t), b, bb, tol, max_iter, check_every)
    res = np.sqrt(norm2(b - wilson(x, psi, kappa, False, antiperiodic_t)) / np.where(bb > 0, bb, 1.0))
    info = {'iters': iters, 'residual': res, 'converged': done}
    return (psi[:, 0] if squeeze else psi), info


def point_sources(nb, L, source=(0, 0, 0, 0)):
    """[nb, 12, T, X, Y, Z, 4, 3]: right-hand side 3 spin + colour is the unit spinor of that component at `source`"""
    b = np.zeros((nb, 12, *L, 4, 3), complex)
    for j in range(12):
        b[(slice(None), j, *source, j // 3, j % 3)] = 1.0
    return b


def propagator(x, kappa, source=(0, 0, 0, 0), **kw):
    """(S, info): S[nb, T, X, Y, Z, 4, 3, 4, 3] (sink spin, sink colour, source spin, source colour)"""
    nb, L = x.shape[0], x.shape[2:6]
    psi, info = cgnr(x, point_sources(nb, L, source), kappa, **kw)
    return np.moveaxis(psi, 1, -1).reshape(nb, *L, 4, 3, 4, 3), info


def pion_correlator(S, t_source=0):
    """C(t) [nb, T] = sum over space, spins and colours of |S|^2 at time t_source + t"""
    c = (S.real ** 2 + S.imag ** 2).sum(axis=(2, 3, 4, 5, 6, 7, 8))
    return np.roll(c, -t_source, axis=1)


def effective_mass(C):
    return np.log(C[..., :-1] / C[..., 1:])


# ------------------------------------------------------------------ native layout of a spinor field
def pack_spinor(psi):
    """[nb, nrhs, T, X, Y, Z, 4, 3] -> [nb, nrhs, 12, V]"""
    nb, nrhs = psi.shape[:2]
    return np.ascontiguousarray(psi.reshape(nb, nrhs, -1, 12).transpose(0, 1, 3, 2))


def unpack_spinor(pn, L):
    nb, nrhs = pn.shape[:2]
    return np.ascontiguousarray(pn.transpose(0, 1, 3, 2)).reshape(nb, nrhs, *L, 4, 3)


# ------------------------------------------------------------------ the inputs and the tolerance of the Wilson tests
KERNEL_LATTICES = sm.KERNEL_LATTICES                                            # host emulation and GPU
GPU_LATTICES = KERNEL_LATTICES + [(4, 4, 4, 8), (4, 4, 4, 10)]                  # whole blocks; a partial last block
API_LATTICES = [(4, 4, 4, 4), (3, 4, 5, 2)]
KAPPA = 0.124                                                                   # of the single applications
SOLVE_KAPPAS = (0.10, 0.12)
FLAGS = [(False, False), (True, False), (False, True), (True, True)]           # (dagger, antiperiodic_t) of flags 0..3


def links(L, nb=3):
    """the smooth links of the smearing tests; fewer chains are the first chains of the three"""
    return sm.smooth_input(L, 3)[:nb]


def spinors(L, nb=3, nrhs=12):
    """Gaussian spinors, unit variance per real component, from a seed fixed by the lattice: the field of 3 chains and
    12 right-hand sides, of which fewer chains or right-hand sides are the first ones"""
    rng = np.random.default_rng(9000 + 1000 * L[0] + 100 * L[1] + 10 * L[2] + L[3])
    a = rng.standard_normal((2, 3, 12, *L, 4, 3))
    return np.ascontiguousarray((a[0] + 1j * a[1])[:nb, :nrhs])


# Yardstick of a single application: the largest element-wise distance between this restatement in complex128 and the
# same functions run on the same inputs in np.clongdouble (x87 extended precision, 64-bit significand), over
# GPU_LATTICES and API_LATTICES at nb = 3, nrhs = 12 (every input of the emulation and GPU tests is a part of these
# fields), KAPPA, all four FLAGS.  `python tests/wilson_restatement.py --measure` prints it; measured per lattice
# (2,2,2,2) 5.93e-16, (4,2,6,2) 7.07e-16, (3,4,5,2) 7.42e-16, (4,1,6,2) 6.43e-16, (4,4,4,8) 7.75e-16, (4,4,4,10) 7.99e-16,
# (4,4,4,4) 7.72e-16: worst 7.99e-16, about one ulp of the largest output entries (|out| up to ~5).  The kernel differs
# from numpy by fma contraction and by the order in which the 8 hops and their 3-term colour sums are added: the
# tolerance is 32 x the yardstick, the margin of the smearing and gauge-fixing tests, and covers that and nothing else.
# tests/test_wilson_host.py measures the small lattices again and holds them to this figure.
YARDSTICK = 8.0e-16
TOL = 32.0 * YARDSTICK


def norm_bound(V):
    """relative bound on a sum of 24 V squares in any order against any other: (n - 1) eps for the additions plus the
    rounding of the terms, n = 12 V complex entries, doubled"""
    return 2.0 * 12 * V * 2.0 ** -53


def measure(lattices=None, nb=3, nrhs=12):
    worst = 0.0
    for L in lattices or GPU_LATTICES + API_LATTICES[:1]:
        x, psi = links(L, nb), spinors(L, nb, nrhs)
        xl, pl = x.astype(np.clongdouble), psi.astype(np.clongdouble)
        here = 0.0
        for dagger, ap in FLAGS:
            d = wilson(x, psi, KAPPA, dagger, ap) - wilson(xl, pl, np.longdouble(KAPPA), dagger, ap)
            here = max(here, float(np.abs(d).max()))
        print(L, f'{here:.3g}')
        worst = max(worst, here)
    print(f'worst: {worst:.3g}')
    return worst


if __name__ == '__main__':
    import sys
    if '--measure' in sys.argv:
        measure()
