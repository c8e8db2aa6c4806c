"""TEST INFRASTRUCTURE: numpy restatement of two flavours of dynamical clover (Sheikholeslami-Wohlert) quarks in the
asymmetric even-odd form: the action with its log det A_oo term, the clover part of its force on the links and the
leapfrog with both, on top of `wilson_clover_restatement` (the operator), `wilson_eo_restatement` (the half fields) and
`wilson_force_restatement` (the hop part of the force, the CG, the `Trajectory`).  Written from the formulas (include/l2q.h,
"csrc/su3_clover_force.hip") with the full 4 x 4 sigma_{mu nu} of `wc.sigma`, not from the kernels.

    S_f = sum_r phi_e,r^H (Mhat^H Mhat)^-1 phi_e,r - 2 npf log det A_oo,   Mhat = A_ee - kappa^2 H_eo A_oo^-1 H_oe,
    X_e = (Mhat^H Mhat)^-1 phi_e,  Y_e = Mhat X_e,  X_o = kappa A_oo^-1 H_oe X_e,  Y_o = kappa A_oo^-1 (H^H)_oe Y_e,
    dS_pf  = 2 kappa Re[Y^H dH X] - 2 Re sum_x Y(x)^H dA(x) X(x),     dS_det = -2 npf sum_{x odd} tr[A^-1(x) dA(x)],
    dA(x)  = kappa c_sw i sum_{mu<nu} sigma_{mu nu} (x) dFhat_{mu nu}(x).
The hop part is `wfr.force` of the completed (X, Y).  The rest is -2 kappa c_sw sum_x sum_{mu<nu} Re tr[dFhat_{mu nu}(x)
Lambda_{mu nu}(x)] with (a b^H the colour outer product, summed over spin)
    Lambda_{mu nu}(x) = i sum_r (sigma_{mu nu} X_r)(x) Y_r(x)^H  +  [x odd] npf i tr_spin[sigma_{mu nu} A^-1(x)].
Fhat = (Q - Q^H) / 8, so Re tr(Lambda dFhat) = 1/4 Re tr(Lambda_AH dQ), Lambda_AH = (Lambda - Lambda^H) / 2: `g_field` is
G = -(kappa c_sw / 2) Lambda_AH per site and plane (dS = sum Re tr(G dQ)), `insert` differentiates sum Re tr(G Q) with
respect to the links leaf by leaf (dS = sum Re tr(B_mu(x) dU_mu(x))), and under dU = p U the force is -TAH(U B).
tests/test_wilson_clover_force_host.py holds all of it against central differences of the action."""
import numpy as np

import wilson_clover_restatement as wc
import wilson_eo_restatement as we
import wilson_force_restatement as wfr
import wilson_restatement as wr

PLANES = ((0, 1), (2, 3), (0, 2), (1, 3), (0, 3), (1, 2))       # the order of the workspace gw[nb][6][9][V]
KAPPA = wc.KAPPA


def _sh(f, steps, sign=1):
    """f(x + sign * sum of steps) of a site field [nb, T, X, Y, Z, ...], a step (direction, +-1)"""
    for d, s in steps:
        f = np.roll(f, -sign * s, axis=1 + d)
    return f


def leaf_factors(mu, nu):
    """the four leaves of Q_{mu nu}(x) in the order of `wc.leaves`, each a list of its four factors (direction, the steps
    from x to the link's site, adjoint)"""
    return [[(mu, (), False), (nu, ((mu, 1),), False), (mu, ((nu, 1),), True), (nu, (), True)],
            [(nu, (), False), (mu, ((mu, -1), (nu, 1)), True), (nu, ((mu, -1),), True), (mu, ((mu, -1),), False)],
            [(mu, ((mu, -1),), True), (nu, ((mu, -1), (nu, -1)), True), (mu, ((mu, -1), (nu, -1)), False),
             (nu, ((nu, -1),), False)],
            [(nu, ((nu, -1),), True), (mu, ((nu, -1),), False), (nu, ((mu, 1), (nu, -1)), False), (mu, (), True)]]


def _factor(x, d, steps, dagger):
    m = _sh(x[:, d], steps)
    return wfr.adj(m) if dagger else m


def leaves_from_factors(x, mu, nu):
    """Q_{mu nu} from `leaf_factors`: the host test holds it to `wc.leaves`"""
    q = 0
    for leaf in leaf_factors(mu, nu):
        m = [_factor(x, *f) for f in leaf]
        q = q + m[0] @ m[1] @ m[2] @ m[3]
    return q


# ------------------------------------------------------------------ the clover part of the force
def g_field(X, Y, ainv, coef, det_weight, L):
    """G [nb, 6, T, X, Y, Z, 3, 3] = -(coef / 2) (Lambda - Lambda^H) / 2, coef = kappa c_sw, planes in the order PLANES.
    X, Y [nb, npf, T, X, Y, Z, 4, 3] or both None (the determinant term alone); ainv [nb, T, X, Y, Z, 12, 12] or None
    (the pseudofermion term alone); det_weight multiplies the determinant term (npf of the action)."""
    src = X if X is not None else ainv
    ct, rt = src.dtype, src.real.dtype.type
    nb = src.shape[0]
    odd = we.mask(L, 1)
    out = np.zeros((nb, 6, *L, 3, 3), ct)
    for pl, (mu, nu) in enumerate(PLANES):
        sg = wc.sigma(mu, nu, ct)
        lam = np.zeros((nb, *L, 3, 3), ct)
        if X is not None:
            sx = np.einsum('pq,nrtxyzqb->nrtxyzpb', sg, X)                        # sigma X
            lam = lam + np.einsum('nrtxyzpb,nrtxyzpa->ntxyzba', sx, Y.conj())     # (sigma X) Y^H, summed over spin and r
        if ainv is not None:
            ai = ainv.reshape(nb, *L, 4, 3, 4, 3)                                 # [.., s', b, s, a]
            lam = lam + rt(det_weight) * (np.einsum('pq,ntxyzqbpa->ntxyzba', sg, ai) * odd)
        lam = ct.type(1j) * lam
        out[:, pl] = rt(-0.5 * coef) * ((lam - wfr.adj(lam)) / rt(2))
    return out


def pack_g(g):
    """G as the kernel's workspace [nb, 6, 9, V] reals: per plane the diagonal's imaginary parts, then the real parts and
    the imaginary parts of the entries (0,1), (0,2), (1,2)"""
    nb = g.shape[0]
    f = g.reshape(nb, 6, -1, 3, 3)
    up = [(0, 1), (0, 2), (1, 2)]
    rows = [f[..., i, i].imag for i in range(3)] + [f[..., i, j].real for i, j in up] + [f[..., i, j].imag for i, j in up]
    return np.ascontiguousarray(np.stack(rows, 2))


def insert(x, g):
    """B [nb, 4, T, X, Y, Z, 3, 3] with d sum_x sum_planes Re tr(G Q) = sum Re tr(B_mu(x) dU_mu(x)): every factor of every
    leaf in turn; a factor U gives (what follows it) G (what precedes it) at the link's site, a factor U^H its adjoint.
    With extents 2 several factors are the same link: every occurrence is its own term."""
    b = np.zeros_like(x)
    eye = np.eye(3).astype(x.dtype)
    for pl, (mu, nu) in enumerate(PLANES):
        for leaf in leaf_factors(mu, nu):
            m = [_factor(x, *f) for f in leaf]
            for k, (d, steps, dagger) in enumerate(leaf):
                c = eye
                for f in m[k + 1:]:
                    c = c @ f
                c = c @ g[:, pl]
                for f in m[:k]:
                    c = c @ f
                b[:, d] += _sh(wfr.adj(c) if dagger else c, steps, -1)
    return b


def clover_force(x, X, Y, ainv, kappa, c_sw, det_weight):
    """the clover part of the force, -TAH(U B): X, Y the completed fields (or None), ainv A^-1 (or None)"""
    L = x.shape[2:6]
    return -wfr.tah(x @ insert(x, g_field(X, Y, ainv, kappa * c_sw, det_weight, L)))


# ------------------------------------------------------------------ the solves and the trajectory
def terms(x, kappa, c_sw):
    """(A, A^-1) of a configuration; A must be positive definite: every input of every test"""
    a = wc.clover(x, kappa * c_sw)
    assert wc.min_eig(a) > 0.0, 'the clover term is not positive definite'      # <=> every L D L^H pivot > 0
    return a, wc.inverse(a)


def dense_schur(x, kappa, a, ainv, antiperiodic_t=True):
    """Mhat of chain 0 as a dense matrix [12 V/2, 12 V/2], as `we.dense_schur`"""
    L = x.shape[2:6]
    n = 12 * int(np.prod(L))
    idx = we.even_index(L)
    basis = np.eye(n, dtype=complex)[idx].reshape(1, len(idx), *L, 4, 3)
    return wc.schur_clover(x[:1], basis, kappa, a[:1], ainv[:1], False, antiperiodic_t).reshape(len(idx), n).T[idx]


class Trajectory(wfr.Trajectory):
    """`wfr.Trajectory` for the clover action at one c_sw: the solves on the asymmetric Schur complement, the completed
    fields with A_oo^-1, the clover force next to the hop force and -2 npf log det A_oo in the action.  pf / det switch
    the two terms of the action (and of its force) for the finite-difference tests."""

    def __init__(self, c_sw, pf=True, det=True):
        self.c_sw, self.pf, self.det = c_sw, pf, det

    def solve(self, x, phi, kappa, antiperiodic_t, tol, t=None):
        a, ainv = t or terms(x, kappa, self.c_sw)
        if tol is not None:
            return wfr.normal_cg_op(lambda p, d: wc.schur_clover(x, p, kappa, a, ainv, d, antiperiodic_t), phi, tol,
                                    4000, 10)[:2]
        L = x.shape[2:6]
        idx = we.even_index(L)
        X = np.zeros_like(phi)
        for c in range(x.shape[0]):
            m = dense_schur(x[c:c + 1], kappa, a[c:c + 1], ainv[c:c + 1], antiperiodic_t)
            b = phi[c].reshape(phi.shape[1], -1)[:, idx].T
            flat = np.zeros((phi.shape[1], 12 * int(np.prod(L))), complex)
            flat[:, idx] = np.linalg.solve(m.conj().T @ m, b).T
            X[c] = flat.reshape(phi.shape[1:])
        return X, wc.schur_clover(x, X, kappa, a, ainv, False, antiperiodic_t)

    def parts(self, x, phi, kappa, antiperiodic_t=True, tol=None):
        """(the pseudofermion part sum_r |Y_e,r|^2, the determinant part -2 npf log det A_oo) [nb] each"""
        t = terms(x, kappa, self.c_sw)
        pf = wr.norm2(self.solve(x, phi, kappa, antiperiodic_t, tol, t)[1]).sum(1) if self.pf else 0.0
        return pf, (-2.0 * phi.shape[1] * wc.logdet(t[0])[:, 1] if self.det else 0.0)

    def fermion_action(self, x, phi, kappa, antiperiodic_t=True, tol=None):
        return sum(self.parts(x, phi, kappa, antiperiodic_t, tol))

    def fermion_force(self, x, phi, kappa, antiperiodic_t=True, tol=None):
        t = a, ainv = terms(x, kappa, self.c_sw)
        w = phi.shape[1] if self.det else 0.0
        if not self.pf:
            return clover_force(x, None, None, ainv, kappa, self.c_sw, w)
        Xe, Ye = self.solve(x, phi, kappa, antiperiodic_t, tol, t)
        X = Xe + wc.hop_clover(x, Xe, 1, ainv, 2, False, antiperiodic_t, a=kappa)
        Y = Ye + wc.hop_clover(x, Ye, 1, ainv, 2, True, antiperiodic_t, a=kappa)
        return wfr.force(x, X, Y, kappa, antiperiodic_t) + clover_force(x, X, Y, ainv if self.det else None, kappa,
                                                                         self.c_sw, w)


def refresh(x, eta_e, kappa, c_sw, antiperiodic_t=True):
    """(phi_e, S0): phi_e = Mhat^H eta_e, S0 = |eta_e|^2 [nb]"""
    L = eta_e.shape[2:6]
    eta_e = eta_e * we.mask(L, 0)
    a, ainv = terms(x, kappa, c_sw)
    return wc.schur_clover(x, eta_e, kappa, a, ainv, True, antiperiodic_t), wr.norm2(eta_e).sum(1)


# ------------------------------------------------------------------ the inputs and the tolerances
NB = wc.NB
TRAJ_C_SW = 1.769


def force_inputs(kind, L, c_sw, nb=NB, npf=3):
    """(x, X, Y, ainv) of the kernel tests: the links of `wc.fields`, the two Gaussian fields (not solutions) of
    `wfr.force_inputs`, the inverse of the clover term"""
    x, _, ainv = wc.fields(kind, L, c_sw, nb)
    s = wr.spinors(L, nb, 12)
    return x, np.ascontiguousarray(s[:, :npf]), np.ascontiguousarray(s[:, 6:6 + npf]), ainv


def fd_inputs(kind, L, nb=2, npf=2):
    """(x, phi_e, p) of the finite-difference tests: `we.fd_inputs` on either kind of links"""
    return wc.INPUTS[kind](L, nb), wr.spinors(L, nb, npf) * we.mask(L, 0), wfr.momentum(L, nb)


def traj_inputs(L, c_sw=TRAJ_C_SW, nb=2, npf=1):
    """(x, v, phi_e, S0) of the trajectory tests, as `we.traj_inputs`"""
    x = wr.links(L, nb)
    phi, s0 = refresh(x, we.gaussian_eta_e(L, nb, npf), wfr.TRAJ['kappa'], c_sw)
    return x, wfr.momentum(L, nb, 1), phi, s0


# Yardsticks of the two kernels: the largest element-wise distance between this restatement in complex128 and the same
# functions in np.clongdouble (A^-1 the same float64 numbers on both sides) on `force_inputs(kind, L, c_sw, NB, 3)` with
# det_weight = 3 over we.EO_GPU_LATTICES, both kinds of links, both wc.C_SWS
# (`python tests/wilson_clover_force_restatement.py --measure`):
#   G   the entries of `g_field`;   F   the entries of `clover_force`.
# Measured per lattice (worst over inputs and c_sw):
#   (2,2,2,2)   G 4.02e-16  F 1.91e-15
#   (4,2,6,2)   G 6.44e-16  F 1.98e-15
#   (2,4,2,6)   G 6.52e-16  F 2.35e-15
#   (4,4,4,8)   G 8.25e-16  F 2.49e-15
#   (4,4,4,10)  G 6.71e-16  F 2.18e-15
# worst G 8.25e-16, F 2.49e-15 (about two ulp of the largest entries).  Every input of the emulation and GPU tests is a
# part of these fields.  The tolerances are 32 x these, the project's margin: they cover fma contraction and the order of
# the kernels' sums and nothing else.
YARD_G = 8.3e-16
YARD_F = 2.5e-15
TOL_G, TOL_F = 32.0 * YARD_G, 32.0 * YARD_F

# The finite-difference figure of this restatement itself (`--measure-fd`): the largest relative Richardson error (h = 1e-3,
# dense solves) of the action against sum <p, F> over we.FD_LATTICES, both kinds of links, both boundary conditions, both
# wc.C_SWS and the three FD_CASES.  What is left at that h is the h^4 term of the differences and the rounding of the
# action divided by h, not the force: tests/test_wilson_clover_force_host.py allows 32 x it and asks for the ratio 4 of the
# two raw differences' h^2 terms besides.
FD_CASES = (('determinant', False, True), ('pseudofermions', True, False), ('both', True, True))      # name, pf, det
# Measured: worst 1.98e-9 ((4,2,2,2), smooth links, c_sw 1.769, periodic, the pseudofermion term: the h^4 term; the same
# input antiperiodic 1.18e-11); the determinant term alone stays below 3.4e-10 on (2,2,2,2) and 6.5e-11 on (4,2,2,2).
DENSE_FD = 2.0e-9

# CG against dense, as in `wilson_eo_restatement` (`--measure-cg`): CG_FD the relative Richardson error over
# we.FD_LATTICES, both boundary conditions, both wc.C_SWS, when action and force come from the CG at wfr.FD_TOL; CG_TRAJ the
# distances of `delta_h` over wfr.TRAJ_LATTICES at c_sw = TRAJ_C_SW between dense solves and the CG at wfr.TRAJ_TOL_MD /
# wfr.TRAJ_TOL_H.
# Measured: CG_FD (2,2,2,2) c_sw 1.0 2.66e-10 periodic, 2.17e-11 antiperiodic; c_sw 1.769 3.35e-10, 2.27e-11; (4,2,2,2)
# c_sw 1.0 4.29e-10, 2.35e-11; c_sw 1.769 1.90e-9, 9.12e-12 (the dense figure of that input is 1.98e-9: the h^4 term of
# the differences, not the solver).  CG_TRAJ (2,2,2,2) x 6.24e-14, v 1.05e-12, dH 4.75e-12; (4,2,2,2) x 3.67e-12, v
# 2.57e-11, dH 4.21e-10.
CG_FD = 2.0e-9
CG_TRAJ = {'x': 3.7e-12, 'v': 2.6e-11, 'dH': 4.3e-10}


def measure(lattices=None, npf=3):
    ld = np.longdouble
    worst = [0.0, 0.0]
    for L in lattices or we.EO_GPU_LATTICES:
        here = [0.0, 0.0]
        for kind in wc.INPUTS:
            for c_sw in wc.C_SWS:
                x, X, Y, ainv = force_inputs(kind, L, c_sw, NB, npf)
                xl, Xl, Yl, al = (t.astype(np.clongdouble) for t in (x, X, Y, ainv))
                g = g_field(X, Y, ainv, KAPPA * c_sw, npf, L) - g_field(Xl, Yl, al, ld(KAPPA) * ld(c_sw), ld(npf), L)
                f = clover_force(x, X, Y, ainv, KAPPA, c_sw, npf) - clover_force(xl, Xl, Yl, al, ld(KAPPA), ld(c_sw), ld(npf))
                here = [max(here[0], float(np.abs(g).max())), max(here[1], float(np.abs(f).max()))]
        print(L, f'G {here[0]:.3g}  F {here[1]:.3g}', flush=True)
        worst = [max(a, b) for a, b in zip(worst, here)]
    print(f'worst: G {worst[0]:.3g}  F {worst[1]:.3g}')
    return worst


def fd_error(tr, x, phi, p, kappa, ap, tol=None, h=1e-3):
    """the relative Richardson error of the action of the trajectory tr against <p, force>, per chain"""
    want = wfr.pair(p, tr.fermion_force(x, phi, kappa, ap, tol))
    d = wfr.richardson(x, phi, p, kappa, ap, h=h, action=lambda xx: tr.fermion_action(xx, phi, kappa, ap, tol))[0]
    return np.abs(d - want) / np.abs(want)


def measure_fd():
    worst = 0.0
    for L in we.FD_LATTICES:
        for kind in wc.INPUTS:
            x, phi, p = fd_inputs(kind, L)
            for c_sw in wc.C_SWS:
                for ap in (False, True):
                    for name, pf, det in FD_CASES:
                        rel = float(fd_error(Trajectory(c_sw, pf, det), x, phi, p, KAPPA, ap).max())
                        print('DENSE_FD', L, kind, c_sw, ap, name, f'{rel:.3g}', flush=True)
                        worst = max(worst, rel)
    print(f'DENSE_FD worst: {worst:.3g}')


def measure_cg():
    worst = 0.0
    for L in we.FD_LATTICES:
        x, phi, p = fd_inputs('smooth', L)
        for c_sw in wc.C_SWS:
            for ap in (False, True):
                rel = float(fd_error(Trajectory(c_sw), x, phi, p, KAPPA, ap, wfr.FD_TOL).max())
                print('CG_FD', L, c_sw, ap, f'{rel:.3g}', flush=True)
                worst = max(worst, rel)
    print(f'CG_FD worst: {worst:.3g}')
    w = {'x': 0.0, 'v': 0.0, 'dH': 0.0}
    tr = Trajectory(TRAJ_C_SW)
    for L in wfr.TRAJ_LATTICES:
        x, v, phi, _ = traj_inputs(L)
        a = tr.delta_h(x, v, phi, **wfr.TRAJ)
        b = tr.delta_h(x, v, phi, **wfr.TRAJ, tol=wfr.TRAJ_TOL_MD, tol_h=wfr.TRAJ_TOL_H)
        here = {k: float(np.abs(p - q).max()) for k, p, q in zip(('x', 'v', 'dH'), a, b)}
        print('CG_TRAJ', L, here, flush=True)
        w = {k: max(w[k], here[k]) for k in w}
    print('CG_TRAJ worst:', w)


if __name__ == '__main__':
    import sys
    if '--measure' in sys.argv:
        measure()
    if '--measure-fd' in sys.argv:
        measure_fd()
    if '--measure-cg' in sys.argv:
        measure_cg()
