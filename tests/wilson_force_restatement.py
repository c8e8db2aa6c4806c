"""TEST INFRASTRUCTURE: numpy restatement of the two-flavour Wilson pseudofermion action, its force on the links, the CG
on M^H M that feeds it, the pseudofermion heatbath and the HMC leapfrog with dynamical quarks, on top of
`wilson_restatement` (the operator) and `oracle.su3` (the gauge part: `grad_action`, `action`, `expm`).  Written from the
formulas (include/l2q.h, "SU(3) Wilson fermions"), in the long form with the full 4 x 4 gamma matrices, not from the
kernel.  Links ``x[nb, 4, T, X, Y, Z, 3, 3]``, pseudofermions ``phi[nb, npf, T, X, Y, Z, 4, 3]``, complex128; `force`
computes in the type of its inputs, which is how `measure()` evaluates it in extended precision.

    S_f = sum_r phi_r^H (M^H M)^-1 phi_r = sum_r |Y_r|^2,   X_r = (M^H M)^-1 phi_r,   Y_r = M X_r.
Convention of any force here: links move as dU/dt = p U with p traceless anti-Hermitian, the force F of an action S is the
TAH field with dS/dt = sum_links <p, F>, <a, b> = Re tr(a^H b); the kick is p <- p - eps F.  With s the seam sign of the
operator (-1 on a hop across t = T-1 -> 0 when antiperiodic, mu = 0), X' = s X(x+mu), Y' = s Y(x+mu) and a b^H the colour
outer product summed over spin,
    W_mu(x) = U_mu(x) sum_r [(1 - gamma_mu) X'_r] Y_r(x)^H - sum_r X_r(x) [(1 + gamma_mu) Y'_r]^H U_mu(x)^H,
    F_mu(x) = -2 kappa TAH(W_mu(x)),   TAH(W) = (W - W^H)/2 - (tr/3) 1.
tests/test_wilson_force_host.py holds this against central differences of S_f."""
import numpy as np

import wilson_restatement as wr
from oracle import su3 as osu3


def adj(m):
    return np.conj(np.swapaxes(m, -1, -2))


def tah(w):
    a = (w - adj(w)) / 2
    tr = np.einsum('...ii->...', a) / 3
    return a - tr[..., None, None] * np.eye(3).astype(w.dtype)


def _forward(f, mu, antiperiodic_t):
    """s f(x + mu)"""
    f = np.roll(f, -1, axis=2 + mu)
    if antiperiodic_t and mu == 0:
        f = f.copy()
        f[:, :, -1] = -f[:, :, -1]
    return f


# ------------------------------------------------------------------ the force
def force(x, X, Y, kappa, antiperiodic_t=True):
    """F_f [nb, 4, T, X, Y, Z, 3, 3] from X, Y [nb, npf, T, X, Y, Z, 4, 3]: the long form above"""
    ct = X.dtype
    eye = np.eye(4).astype(ct)
    out = np.zeros_like(x)
    for mu in range(4):
        g = wr.GAMMA[mu].astype(ct)
        u = x[:, mu]
        px = np.einsum('ad,brtxyzdc->brtxyzac', eye - g, _forward(X, mu, antiperiodic_t))      # (1 - gamma) X'
        py = np.einsum('ad,brtxyzdc->brtxyzac', eye + g, _forward(Y, mu, antiperiodic_t))      # (1 + gamma) Y'
        a = np.einsum('brtxyzai,brtxyzaj->btxyzij', px, Y.conj())
        b = np.einsum('brtxyzai,brtxyzaj->btxyzij', X, py.conj())
        out[:, mu] = tah(u @ a - b @ adj(u))
    return -2 * X.real.dtype.type(kappa) * out


def pair(p, f):
    """sum over links of <p, F> per chain"""
    return (p.conj() * f).real.reshape(p.shape[0], -1).sum(1)


# ------------------------------------------------------------------ the solves
def dense_normal(x, phi, kappa, antiperiodic_t=True):
    """(X, Y) by a dense solve of M^H M X = phi, chain by chain"""
    X = np.empty_like(phi)
    for c in range(x.shape[0]):
        m = wr.dense(x[c:c + 1], kappa, antiperiodic_t)
        b = phi[c].reshape(phi.shape[1], -1).T
        X[c] = np.linalg.solve(m.conj().T @ m, b).T.reshape(phi.shape[1:])
    return X, wr.wilson(x, X, kappa, False, antiperiodic_t)


def normal_cg_op(op, phi, tol=1e-10, max_iter=1000, check_every=10):
    """A^H A X = phi by CG from X = 0, op(p, dagger) the operator; per iteration q = A p, z = A^H q, alpha = |r|^2 /
    |q|^2, X += alpha p, r -= alpha z, beta = |r'|^2 / |r|^2, p = r + beta p.  |r|^2 <= tol^2 |phi|^2 is looked at every
    check_every iterations (and at 0 and max_iter); a converged system takes alpha = beta = 0 from then on.  Returns (X,
    Y, info), Y = A X, info = {'iters', 'converged', 'residual' (|phi - A^H A X| / |phi| recomputed, 0 for phi = 0),
    'action' (|Y|^2)} each [nb, npf]."""
    X = np.zeros_like(phi)
    r = phi.copy()
    p = phi.copy()
    bb = wr.norm2(phi)
    rr = bb.copy()
    done = rr <= tol * tol * bb
    iters = np.where(done, 0, max_iter)
    k = 0
    while k < max_iter and not done.all():
        q = op(p, False)
        qq = wr.norm2(q)
        z = op(q, True)
        live = ~done & (qq > 0)
        alpha = np.where(live, rr / np.where(live, qq, 1.0), 0.0)
        X = X + wr._bc(alpha) * p
        r = r - wr._bc(alpha) * z
        rn = wr.norm2(r)
        live = ~done & (rr > 0)
        beta = np.where(live, rn / np.where(live, rr, 1.0), 0.0)
        p = r + wr._bc(beta) * p
        rr = rn
        k += 1
        if k % check_every == 0 or k == max_iter:
            now = ~done & (rr <= tol * tol * bb)
            iters = np.where(now, k, iters)
            done = done | now
    Y = op(X, False)
    res = np.sqrt(wr.norm2(phi - op(Y, True)) / np.where(bb > 0, bb, 1.0))
    return X, Y, {'iters': iters, 'converged': done, 'residual': res, 'action': wr.norm2(Y)}


def normal_cg(x, phi, kappa, tol=1e-10, max_iter=1000, check_every=10, antiperiodic_t=True):
    """M^H M X = phi by `normal_cg_op` on M: (X, Y = M X, info)"""
    return normal_cg_op(lambda p, d: wr.wilson(x, p, kappa, d, antiperiodic_t), phi, tol, max_iter, check_every)


# ------------------------------------------------------------------ action, force, trajectory
class Trajectory:
    """The action, the force and the leapfrog of a pseudofermion action phi^H (A^H A)^-1 phi over its three pieces:
    dense(x, phi, kappa, antiperiodic_t) and cg(x, phi, kappa, tol=, max_iter=, antiperiodic_t=) solve A^H A X = phi and
    give (X, Y = A X, ...); complete(x, X, Y, kappa, antiperiodic_t) gives the full fields whose `force` is the
    action's.  Below for A = M; `wilson_eo_restatement` builds the one of the Schur complement."""

    def __init__(self, dense, cg, complete):
        self.dense, self.cg, self.complete = dense, cg, complete

    def solve(self, x, phi, kappa, antiperiodic_t, tol):
        """tol None: dense; else the CG at that tol"""
        if tol is None:
            return self.dense(x, phi, kappa, antiperiodic_t)
        return self.cg(x, phi, kappa, tol=tol, max_iter=4000, antiperiodic_t=antiperiodic_t)[:2]

    def fermion_action(self, x, phi, kappa, antiperiodic_t=True, tol=None):
        """S_f [nb] = sum_r |Y_r|^2"""
        return wr.norm2(self.solve(x, phi, kappa, antiperiodic_t, tol)[1]).sum(1)

    def fermion_force(self, x, phi, kappa, antiperiodic_t=True, tol=None):
        X, Y = self.complete(x, *self.solve(x, phi, kappa, antiperiodic_t, tol), kappa, antiperiodic_t)
        return force(x, X, Y, kappa, antiperiodic_t)

    def total_force(self, x, phi, beta, kappa, antiperiodic_t=True, tol=None):
        f = self.fermion_force(x, phi, kappa, antiperiodic_t, tol)
        return f + osu3.grad_action(x, beta) if beta != 0 else f

    def leapfrog(self, x, v, phi, beta, kappa, eps, nleapfrog, antiperiodic_t=True, tol=None):
        """half kick, nleapfrog link updates U <- exp(eps p) U with full kicks between them, half kick"""
        v = v - 0.5 * eps * self.total_force(x, phi, beta, kappa, antiperiodic_t, tol)
        for k in range(nleapfrog):
            x = osu3.expm(eps * v) @ x
            v = v - (1.0 if k + 1 < nleapfrog else 0.5) * eps * self.total_force(x, phi, beta, kappa, antiperiodic_t, tol)
        return x, v

    def hamiltonian(self, x, v, phi, beta, kappa, antiperiodic_t=True, tol=None):
        return osu3.kinetic_energy(v) + osu3.action(x, beta) + self.fermion_action(x, phi, kappa, antiperiodic_t, tol)

    def delta_h(self, x, v, phi, beta, kappa, eps, nleapfrog, tol=None, tol_h=None):
        """(x', v', H' - H) of one leapfrog"""
        x1, v1 = self.leapfrog(x, v, phi, beta, kappa, eps, nleapfrog, True, tol)
        return x1, v1, (self.hamiltonian(x1, v1, phi, beta, kappa, True, tol_h)
                        - self.hamiltonian(x, v, phi, beta, kappa, True, tol_h))

    def names(self):
        """the functions a restatement module exports under these names"""
        return self.fermion_action, self.fermion_force, self.total_force, self.leapfrog, self.hamiltonian, self.delta_h


fermion_action, fermion_force, total_force, leapfrog, hamiltonian, delta_h = Trajectory(
    dense_normal, normal_cg, lambda x, X, Y, kappa, antiperiodic_t: (X, Y)).names()


# ------------------------------------------------------------------ heatbath and inputs of a trajectory
def refresh(x, eta, kappa, antiperiodic_t=True):
    """(phi, S0): phi = M^H eta is distributed as exp(-S_f) for eta distributed as exp(-eta^H eta); S0 = |eta|^2 [nb]"""
    return wr.wilson(x, eta, kappa, True, antiperiodic_t), wr.norm2(eta).sum(1)


def gaussian_eta(L, nb, npf, seed=0):
    """complex Gaussian with density exp(-eta^H eta): variance 1/2 per real component"""
    rng = np.random.default_rng(4000 + seed + 1000 * L[0] + 100 * L[1] + 10 * L[2] + L[3])
    a = rng.standard_normal((2, nb, npf, *L, 4, 3)) * np.sqrt(0.5)
    return a[0] + 1j * a[1]


def momentum(L, nb, seed=0):
    rng = np.random.default_rng(6000 + seed + 1000 * L[0] + 100 * L[1] + 10 * L[2] + L[3])
    return osu3.rand_tah3(rng.standard_normal((8, nb, 4, *L)))


def richardson(x, phi, p, kappa, antiperiodic_t=True, h=1e-3, tol=None, action=None):
    """(d, d1, d2): the Richardson combination (4 D(h/2) - D(h)) / 3 of the central differences D of S_f under
    U -> exp(+-h p) U, and the two central differences themselves, per chain"""
    action = action or (lambda xx: fermion_action(xx, phi, kappa, antiperiodic_t, tol))

    def cd(hh):
        return (action(osu3.expm(hh * p) @ x) - action(osu3.expm(-hh * p) @ x)) / (2 * hh)
    d1, d2 = cd(h), cd(h / 2)
    return (4 * d2 - d1) / 3, d1, d2


# ------------------------------------------------------------------ the inputs and the tolerances of the force tests
FD_LATTICES = [(2, 2, 2, 2), (4, 1, 6, 2), (3, 2, 2, 1)]
TRAJ_LATTICES = [(2, 2, 2, 2), (4, 2, 2, 2)]
TRAJ = dict(beta=5.5, kappa=0.12, eps=0.05, nleapfrog=8)


def force_inputs(L, nb=3, npf=3):
    """(x, X, Y): the links and two Gaussian fields (not solutions) of the kernel tests -- right-hand sides 0..npf-1 and
    6..6+npf-1 of `wr.spinors`"""
    s = wr.spinors(L, nb, 12)
    return wr.links(L, nb), np.ascontiguousarray(s[:, :npf]), np.ascontiguousarray(s[:, 6:6 + npf])


def pack_links(f):
    """[nb, 4, T, X, Y, Z, 3, 3] -> the native [nb, 4, 9, V]"""
    nb = f.shape[0]
    return np.ascontiguousarray(f.reshape(nb, 4, -1, 9).transpose(0, 1, 3, 2))


def unpack_links(fn, L):
    nb = fn.shape[0]
    return np.ascontiguousarray(fn.transpose(0, 1, 3, 2)).reshape(nb, 4, *L, 3, 3)


# Yardstick of the force kernel: the largest element-wise distance between `force` in complex128 and in np.clongdouble
# on `force_inputs(L, 3, 3)` over wr.GPU_LATTICES at wr.KAPPA, both boundary conditions (every input of the emulation
# and GPU tests is a part of these fields).  `python tests/wilson_force_restatement.py --measure` prints it; measured per
# lattice (2,2,2,2) 1.59e-15, (4,2,6,2) 2.14e-15, (3,4,5,2) 2.17e-15, (4,1,6,2) 1.91e-15, (4,4,4,8) 2.47e-15,
# (4,4,4,10) 2.40e-15: worst 2.47e-15, about two ulp of the largest entries (|F| up to ~9).
# The kernel differs from numpy by fma contraction and the order of its sums (4 npf rank-1 updates, the 3-term colour
# sums): the tolerance is 32 x the yardstick, the project's margin, and covers that and nothing else.
# tests/test_wilson_force_host.py measures the small lattices again and holds them to this figure.
YARDSTICK = 2.5e-15
TOL = 32.0 * YARDSTICK

# Distances of the restatement from itself when its solves are its own CG instead of dense solves, measured on the CPU
# by `python tests/wilson_force_restatement.py --measure-cg` on the inputs of the GPU tests (tests/test_wilson_force_gpu.py
# allows 32 x each: a CG solve is not a dense solve, and what separates the two is the solver tolerance, not rounding):
#   CG_X     max |X_cg - X_dense| of `normal_cg` at SOLVE_TOL over wr.API_LATTICES x wr.SOLVE_KAPPAS, nb = 2, npf = 2;
#   CG_FD    the relative Richardson error of `richardson` on FD_GPU_LATTICE when action and force come from the CG at
#            FD_TOL (both boundary conditions);
#   CG_TRAJ  max |x' - x'_dense|, max |v' - v'_dense| and |dH - dH_dense| of `delta_h` over TRAJ_LATTICES when the
#            leapfrog solves at TRAJ_TOL_MD and the Hamiltonian at TRAJ_TOL_H.
SOLVE_TOL = 1e-10
FD_GPU_LATTICE = (4, 1, 6, 2)
FD_TOL = 1e-13
TRAJ_TOL_MD = 1e-10
TRAJ_TOL_H = 1e-12
# Measured: CG_X (4,4,4,4) 3.31e-11 (kappa 0.10), 1.05e-10 (0.12); (3,4,5,2) 8.99e-10, 2.99e-10.  CG_FD 6.01e-10 periodic,
# 5.28e-11 antiperiodic (the dense figure of the same lattice is 6.4e-10: the h^4 term of the differences, not the solver).
# CG_TRAJ (2,2,2,2) x 1.46e-11, v 4.79e-11, dH 1.19e-10; (4,2,2,2) x 2.97e-11, v 1.06e-10, dH 1.65e-9.
CG_X = 9.0e-10
CG_FD = 6.1e-10
CG_TRAJ = {'x': 3.0e-11, 'v': 1.1e-10, 'dH': 1.7e-9}


def fd_inputs(L, nb=2, npf=2):
    """(x, phi, p) of the finite-difference tests"""
    return wr.links(L, nb), wr.spinors(L, nb, npf), momentum(L, nb)


def traj_inputs(L, nb=2, npf=1):
    """(x, v, phi, S0) of the trajectory tests: phi from the heatbath of a fixed eta.  The momentum is seed 1: the
    ratio dH(eps) / dH(eps / 2) -> 4 is asymptotic, and with seed 0 chain 0 of (4, 2, 2, 2) has dH = -0.09 at eps =
    0.05, a third of every other chain's (its eps^2 term nearly cancels), where the eps^4 term shows: ratio 3.33.  With
    seed 1 every |dH(0.05)| at beta = 5.5 is 0.28 .. 0.45 and the ratios are 3.76 .. 3.91 (beta = 0: 3.94 .. 3.96)."""
    x = wr.links(L, nb)
    phi, s0 = refresh(x, gaussian_eta(L, nb, npf), TRAJ['kappa'])
    return x, momentum(L, nb, 1), phi, s0


def measure(lattices=None, nb=3, npf=3):
    worst = 0.0
    for L in lattices or wr.GPU_LATTICES:
        x, X, Y = force_inputs(L, nb, npf)
        xl, Xl, Yl = (a.astype(np.clongdouble) for a in (x, X, Y))
        here = 0.0
        for ap in (False, True):
            d = force(x, X, Y, wr.KAPPA, ap) - force(xl, Xl, Yl, np.longdouble(wr.KAPPA), ap)
            here = max(here, float(np.abs(d).max()))
        print(L, f'{here:.3g}')
        worst = max(worst, here)
    print(f'worst: {worst:.3g}')
    return worst


def measure_cg():
    """the three CG-against-dense distances above"""
    worst = 0.0
    for L in wr.API_LATTICES:
        x, phi = wr.links(L, 2), wr.spinors(L, 2, 2)
        for kappa in wr.SOLVE_KAPPAS:
            d = float(np.abs(normal_cg(x, phi, kappa, tol=SOLVE_TOL)[0] - dense_normal(x, phi, kappa)[0]).max())
            print('CG_X', L, kappa, f'{d:.3g}')
            worst = max(worst, d)
    print(f'CG_X worst: {worst:.3g}')
    worst = 0.0
    x, phi, p = fd_inputs(FD_GPU_LATTICE)
    for ap in (False, True):
        want = pair(p, fermion_force(x, phi, wr.KAPPA, ap, FD_TOL))
        d = richardson(x, phi, p, wr.KAPPA, ap, tol=FD_TOL)[0]
        rel = float((np.abs(d - want) / np.abs(want)).max())
        print('CG_FD', ap, f'{rel:.3g}')
        worst = max(worst, rel)
    print(f'CG_FD worst: {worst:.3g}')
    w = {'x': 0.0, 'v': 0.0, 'dH': 0.0}
    for L in TRAJ_LATTICES:
        x, v, phi, _ = traj_inputs(L)
        a = delta_h(x, v, phi, **TRAJ)
        b = delta_h(x, v, phi, **TRAJ, tol=TRAJ_TOL_MD, tol_h=TRAJ_TOL_H)
        here = {k: float(np.abs(p - q).max()) for k, p, q in zip(('x', 'v', 'dH'), a, b)}
        print('CG_TRAJ', L, here)
        w = {k: max(w[k], here[k]) for k in w}
    print('CG_TRAJ worst:', w)


if __name__ == '__main__':
    import sys
    if '--measure' in sys.argv:
        measure()
    if '--measure-cg' in sys.argv:
        measure_cg()
