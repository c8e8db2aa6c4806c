"""TEST INFRASTRUCTURE: numpy restatement of multi-shift CG (Jegerlehner, hep-lat/9612014) on the even-odd Schur
complement of `wilson_eo_restatement`, and of the one-flavour rational (RHMC) pseudofermion on it: action, heatbath,
force and the 2+1 leapfrog.  Written from the formulas (include/l2q.h, l2hmc/lattice/su3/pytorch/rational.py), not from
the kernels.  Half fields are full-shape fields [nb, nrhs, T, X, Y, Z, 4, 3] that are zero on the odd sites; shifted
fields carry the shift axis after nrhs: [nb, nrhs, ns, T, X, Y, Z, 4, 3].

With A = Mhat^H Mhat, R(y) = A_R (1 + sum_k rho_k / (y + a_2k)) ~ y^(-1/2) on [ra, rb] and Qhat = gamma5 Mhat:
    S_1 = phi^H R(A) phi = A_R (|phi|^2 + sum_k rho_k Re <phi, X_k>),  X_k = (A + a_2k)^-1 phi,
    phi = C eta = A_R^(-1/2) (eta + i gamma5 Mhat W + Vv),  W = sum_k c_k Z_k,  Vv = sum_k c_k nu_k Z_k,  Z_k = (A + nu_k^2)^-1 eta,
    F   = the two-flavour force of the fields X'_k = sqrt(A_R rho_k) X_k, Y'_k = Mhat X'_k, completed to the odd sites.
Precondition, asserted by `assert_spectrum`: the spectrum of A lies inside [ra, rb] of the approximation it is used with."""
import numpy as np

import wilson_eo_restatement as we
import wilson_force_restatement as wfr
import wilson_restatement as wr
from l2hmc.lattice.su3.pytorch.rational import zolotarev_inv_sqrt

osu3 = wfr.osu3


def _bs(a):
    """[nb, nrhs, ns] -> broadcastable over a shifted field"""
    return a[..., None, None, None, None, None, None]


def norm2s(f):
    """|f|^2 per (chain, rhs, shift) of a shifted field"""
    return (f.real ** 2 + f.imag ** 2).sum((-6, -5, -4, -3, -2, -1))


# ------------------------------------------------------------------ the three BLAS-1 kernels, on native-layout arrays
def mshift_update(x, ps, p, r, a, b, zeta, beta, live):
    """(x', ps', p') of l2q_su3_spinor_mshift_update: x, ps [nb, nrhs, ns, 12, V]; p, r [nb, nrhs, 12, V]; a, b, zeta, live
    [nb, nrhs, ns]; beta [nb, nrhs].  A shift that is not live keeps its fields."""
    lv = (live != 0)[..., None, None]
    xn = np.where(lv, x + a[..., None, None] * ps, x)
    pn = np.where(lv, zeta[..., None, None] * r[:, :, None] + b[..., None, None] * ps, ps)
    return xn, pn, r + beta[..., None, None] * p


def axmy_norm(r, z, alpha):
    """(r', |r'|^2 [nb, nrhs]) of l2q_su3_spinor_axmy_norm"""
    rn = r - alpha[..., None, None] * z
    return rn, (rn.real ** 2 + rn.imag ** 2).sum((-2, -1))


def lincomb(x, w):
    """sum_k w_k x_k [nb, nrhs, 12, V], summed in the order of k"""
    out = np.zeros_like(x[:, :, 0])
    for k in range(x.shape[2]):
        out = out + w[:, :, k, None, None] * x[:, :, k]
    return out


KERNEL_SITES = [8, 24, 320]                # a tiny grid, no multiple of the wave, a partial second block
KERNEL_NS = [1, 3]


def kernel_inputs(V, ns, nb=2, nrhs=2):
    """the operands of the kernel tests: Gaussian fields and coefficients of order one; system (0, 0) has every
    coefficient zero, and with ns > 1 shift 1 of every system is not live (ns = 1: the shift of system (1, 1))"""
    rng = np.random.default_rng(100 * V + ns)

    def field(*shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    f = dict(x=field(nb, nrhs, ns, 12, V), ps=field(nb, nrhs, ns, 12, V), p=field(nb, nrhs, 12, V),
             r=field(nb, nrhs, 12, V), z=field(nb, nrhs, 12, V))
    c = {k: rng.standard_normal((nb, nrhs, ns)) for k in ('a', 'b', 'zeta', 'w')}
    c.update({k: rng.standard_normal((nb, nrhs)) for k in ('beta', 'alpha')})
    for v in c.values():
        v[0, 0] = 0.0
    live = np.ones((nb, nrhs, ns), np.int32)
    if ns > 1:
        live[:, :, 1] = 0
    else:
        live[1, 1, 0] = 0
    return f, c, live


# ------------------------------------------------------------------ the solver
def multishift_cg_op(op, phi, shifts, tol=1e-10, max_iter=1000, check_every=10, freeze=True):
    """(A^H A + sigma_k) X_k = phi for all shifts at once from X_k = 0, op(p, dagger) the operator.  Per iteration q = A p,
    z = A^H q, alpha = |r|^2 / |q|^2, r -= alpha z, beta = |r'|^2 / |r|^2, then per shift
        zeta' = zeta zeta_old alpha_old / (alpha beta_old (zeta_old - zeta) + zeta_old alpha_old (1 + sigma alpha)),
        X_k += alpha (zeta' / zeta) p_k,   p_k = zeta' r + beta (zeta' / zeta)^2 p_k,
    and p = r + beta p.  |r|^2 <= tol^2 |phi|^2 is looked at every check_every iterations; a converged system is frozen;
    with freeze a single shift with zeta_k^2 |r|^2 <= tol^2 |phi|^2 at a check is frozen too.  Returns (X, info), info =
    {'iters', 'converged' [nb, nrhs]; 'shift_iters', 'residual' [nb, nrhs, ns]}."""
    sig = np.asarray(shifts, dtype=float)
    ns = len(sig)
    nb, nrhs = phi.shape[:2]
    X = np.zeros((nb, nrhs, ns, *phi.shape[2:]), phi.dtype)
    P = np.repeat(phi[:, :, None], ns, axis=2)
    r, p = phi.copy(), phi.copy()
    bb = wr.norm2(phi)
    rr = bb.copy()
    done = rr <= tol * tol * bb
    iters = np.where(done, 0, max_iter)
    slive = np.ones((nb, nrhs, ns), bool)
    shift_iters = np.where(done[..., None], 0, max_iter) * np.ones((1, 1, ns), int)
    zeta, zeta_old = np.ones((nb, nrhs, ns)), np.ones((nb, nrhs, ns))
    alpha_old, beta_old = np.ones((nb, nrhs)), np.zeros((nb, nrhs))
    k = 0
    while k < max_iter and not done.all():
        q = op(p, False)
        qq = wr.norm2(q)
        z = op(q, True)
        live = ~done & (qq > 0)
        alpha = np.where(live, rr / np.where(live, qq, 1.0), 0.0)
        r = r - wr._bc(alpha) * z
        rn = wr.norm2(r)
        live = ~done & (rr > 0)
        beta = np.where(live, rn / np.where(live, rr, 1.0), 0.0)
        al, bt, alo, bto = alpha[..., None], beta[..., None], alpha_old[..., None], beta_old[..., None]
        den = al * bto * (zeta_old - zeta) + zeta_old * alo * (1.0 + sig * al)
        lv = slive & (al > 0) & (den != 0)
        zn = np.where(lv, zeta * zeta_old * alo / np.where(lv, den, 1.0), zeta)
        rat = np.where(lv, zn / np.where(lv, zeta, 1.0), 0.0)
        X = np.where(_bs(lv), X + _bs(al * rat) * P, X)
        P = np.where(_bs(lv), _bs(zn) * r[:, :, None] + _bs(bt * rat * rat) * P, P)
        p = r + wr._bc(beta) * p
        zeta_old, zeta = np.where(lv, zeta, zeta_old), zn
        moved = alpha > 0
        alpha_old, beta_old = np.where(moved, alpha, alpha_old), np.where(moved, beta, beta_old)
        rr = rn
        k += 1
        if k % check_every == 0 or k == max_iter:
            bound = tol * tol * bb
            sdone = slive & ~done[..., None] & ((zeta * zeta * rr[..., None] <= bound[..., None]) if freeze
                                                else (rr <= bound)[..., None])
            shift_iters = np.where(sdone, k, shift_iters)
            slive = slive & ~sdone
            now = ~done & (rr <= bound)
            iters = np.where(now, k, iters)
            done = done | now
    flat = X.reshape(nb, nrhs * ns, *phi.shape[2:])
    ax = op(op(flat, False), True).reshape(X.shape) + _bs(sig[None, None]) * X
    res = np.sqrt(norm2s(phi[:, :, None] - ax) / np.where(bb > 0, bb, 1.0)[..., None])
    return X, {'iters': iters, 'converged': done, 'shift_iters': shift_iters, 'residual': res}


def multishift_cg(x, phi_e, kappa, shifts, tol=1e-10, max_iter=1000, check_every=10, antiperiodic_t=True, freeze=True):
    return multishift_cg_op(lambda p, d: we.schur(x, p, kappa, d, antiperiodic_t), phi_e, shifts, tol, max_iter,
                            check_every, freeze)


def dense_shifted(x, phi_e, kappa, shifts, antiperiodic_t=True, dense=we.dense_schur):
    """X [nb, nrhs, ns, ...] by dense solves of (Mhat^H Mhat + sigma_k) X_k = phi_e, chain by chain"""
    L = x.shape[2:6]
    idx = we.even_index(L)
    nb, nrhs = phi_e.shape[:2]
    X = np.zeros((nb, nrhs, len(shifts), *phi_e.shape[2:]), complex)
    for c in range(nb):
        m = dense(x[c:c + 1], kappa, antiperiodic_t)
        a = m.conj().T @ m
        b = phi_e[c].reshape(nrhs, -1)[:, idx].T
        for j, s in enumerate(shifts):
            flat = np.zeros((nrhs, 12 * int(np.prod(L))), complex)
            flat[:, idx] = np.linalg.solve(a + s * np.eye(len(idx)), b).T
            X[c, :, j] = flat.reshape(phi_e.shape[1:])
    return X


def shifted(x, phi_e, kappa, shifts, antiperiodic_t=True, tol=None):
    """tol None: dense; else the multi-shift CG at that tol"""
    if tol is None:
        return dense_shifted(x, phi_e, kappa, shifts, antiperiodic_t)
    return multishift_cg(x, phi_e, kappa, shifts, tol=tol, max_iter=4000, antiperiodic_t=antiperiodic_t)[0]


def spectrum(x, kappa, antiperiodic_t=True):
    """the eigenvalues of Mhat^H Mhat per chain: [nb, 12 V/2], ascending"""
    out = []
    for c in range(x.shape[0]):
        m = we.dense_schur(x[c:c + 1], kappa, antiperiodic_t)
        out.append(np.linalg.eigvalsh(m.conj().T @ m))
    return np.stack(out)


def assert_spectrum(x, kappa, rat, antiperiodic_t=True):
    ev = spectrum(x, kappa, antiperiodic_t)
    assert rat.ra <= ev.min() and ev.max() <= rat.rb, (ev.min(), ev.max(), rat.ra, rat.rb)
    return ev


# ------------------------------------------------------------------ the one-flavour pseudofermion
def gamma5(f):
    """gamma5 = diag(-1, -1, 1, 1) on the spin index"""
    return f * np.array([-1.0, -1.0, 1.0, 1.0])[:, None]


def dot_re(a, b):
    """Re <a, b> per (chain, rhs, shift) of shifted fields"""
    return (a.conj() * b).real.sum((-6, -5, -4, -3, -2, -1))


def rat_action(x, phi_e, kappa, rat, antiperiodic_t=True, tol=None):
    """S_1 [nb] = sum_r phi_r^H R(Mhat^H Mhat) phi_r by the partial fractions"""
    X = shifted(x, phi_e, kappa, rat.poles, antiperiodic_t, tol)
    s = wr.norm2(phi_e) + (rat.rho * dot_re(phi_e[:, :, None], X)).sum(-1)
    return rat.A * s.sum(1)


def exact_action(x, phi_e, kappa, antiperiodic_t=True):
    """sum_r phi_r^H (Mhat^H Mhat)^(-1/2) phi_r [nb] from the eigen-decomposition"""
    L = x.shape[2:6]
    idx = we.even_index(L)
    out = np.zeros(x.shape[0])
    for c in range(x.shape[0]):
        m = we.dense_schur(x[c:c + 1], kappa, antiperiodic_t)
        ev, vec = np.linalg.eigh(m.conj().T @ m)
        b = phi_e[c].reshape(phi_e.shape[1], -1)[:, idx].T
        out[c] = ((np.abs(vec.conj().T @ b) ** 2) / np.sqrt(ev)[:, None]).sum()
    return out


def rat_refresh(x, eta_e, kappa, rat, antiperiodic_t=True, tol=None):
    """(phi_e, S0): phi_e = C eta_e, S0 = |eta_e|^2 [nb]"""
    L = eta_e.shape[2:6]
    eta_e = eta_e * we.mask(L, 0)
    Z = shifted(x, eta_e, kappa, rat.nu ** 2, antiperiodic_t, tol)
    W = (_bs(rat.c[None, None]) * Z).sum(2)
    Vv = (_bs((rat.c * rat.nu)[None, None]) * Z).sum(2)
    phi = (eta_e + 1j * gamma5(we.schur(x, W, kappa, False, antiperiodic_t)) + Vv) / np.sqrt(rat.A)
    return phi, wr.norm2(eta_e).sum(1)


def rat_force(x, phi_e, kappa, rat, antiperiodic_t=True, tol=None):
    """F [nb, 4, T, X, Y, Z, 3, 3] of S_1"""
    X = shifted(x, phi_e, kappa, rat.poles, antiperiodic_t, tol)
    nb, nrhs, ns = X.shape[:3]
    Xe = (_bs(np.sqrt(rat.A * rat.rho)[None, None]) * X).reshape(nb, nrhs * ns, *X.shape[3:])
    Ye = we.schur(x, Xe, kappa, False, antiperiodic_t)
    return wfr.force(x, *we.completed(x, Xe, Ye, kappa, antiperiodic_t), kappa, antiperiodic_t)


# ------------------------------------------------------------------ the 2 + 1 trajectory
def total_force(x, phi_l, phi_s, beta, kappa, rat, kappa_light=None, tol=None):
    f = rat_force(x, phi_s, kappa, rat, True, tol)
    if phi_l is not None:
        f = we.fermion_force(x, phi_l, kappa_light, True, tol) + f
    return f + osu3.grad_action(x, beta) if beta != 0 else f


def leapfrog(x, v, phi_l, phi_s, beta, kappa, eps, nleapfrog, rat, kappa_light=None, tol=None):
    v = v - 0.5 * eps * total_force(x, phi_l, phi_s, beta, kappa, rat, kappa_light, tol)
    for k in range(nleapfrog):
        x = osu3.expm(eps * v) @ x
        v = v - (1.0 if k + 1 < nleapfrog else 0.5) * eps * total_force(x, phi_l, phi_s, beta, kappa, rat, kappa_light, tol)
    return x, v


def hamiltonian(x, v, phi_l, phi_s, beta, kappa, rat, kappa_light=None, tol=None):
    s = rat_action(x, phi_s, kappa, rat, True, tol)
    if phi_l is not None:
        s = we.fermion_action(x, phi_l, kappa_light, True, tol) + s
    return osu3.kinetic_energy(v) + osu3.action(x, beta) + s


def delta_h(x, v, phi_l, phi_s, beta, kappa, eps, nleapfrog, rat, kappa_light=None, tol=None, tol_h=None):
    x1, v1 = leapfrog(x, v, phi_l, phi_s, beta, kappa, eps, nleapfrog, rat, kappa_light, tol)
    return x1, v1, (hamiltonian(x1, v1, phi_l, phi_s, beta, kappa, rat, kappa_light, tol_h)
                    - hamiltonian(x, v, phi_l, phi_s, beta, kappa, rat, kappa_light, tol_h))


# ------------------------------------------------------------------ inputs and tolerances
LATTICES = [(2, 2, 2, 2), (4, 2, 2, 2)]
SOLVER_LATTICES = LATTICES + [(4, 4, 4, 4)]
K = we.K
SHIFTS = [0.0, 0.05, 1.3]
SOLVE_TOL = 1e-10
# [RA, RB] holds the spectrum of Mhat^H Mhat of every configuration the tests use (wr.links at K and wfr.TRAJ['kappa'],
# and the end points of the trajectories): `assert_spectrum` checks each where it is used.  Measured on wr.links:
# see profiles/su3_wilson_multishift/restatement_measure.txt.  RB is above the rigorous (1 + 64 K^2)^2 = 3.94.
RA, RB = 0.02, 4.0
DEGREE = 6
KAPPA_LIGHT = 0.11


def rational(n=DEGREE, ra=RA, rb=RB):
    return zolotarev_inv_sqrt(n, ra, rb)


def traj_inputs(L, nb=2, light=True):
    """(x, v, phi_l or None, phi_s): the links and momentum of `we.traj_inputs`, the light field from `we.refresh` at
    KAPPA_LIGHT (eta seed 0), the strange one from `rat_refresh` at wfr.TRAJ['kappa'] (eta seed 1)"""
    x = wr.links(L, nb)
    phi_l = we.refresh(x, we.gaussian_eta_e(L, nb, 1), KAPPA_LIGHT)[0] if light else None
    phi_s = rat_refresh(x, we.gaussian_eta_e(L, nb, 1, seed=1), wfr.TRAJ['kappa'], rational())[0]
    return x, wfr.momentum(L, nb, 1), phi_l, phi_s


# Distances of this restatement's multi-shift CG from its dense solves, measured on the CPU by `python
# tests/wilson_multishift_restatement.py --measure` (profiles/su3_wilson_multishift/restatement_measure.txt); the GPU
# tests allow 32 x each (the project's convention: what separates a CG solve from a dense one is the solver tolerance):
#   CG_X     max |X_cg - X_dense| at SOLVE_TOL over SOLVER_LATTICES and (4, 2, 6, 2), SHIFTS, nb = 2, nrhs = 2;
#   CG_S     |S_1(CG at wfr.TRAJ_TOL_H) - S_1(dense)| / S_1 on `traj_inputs` over LATTICES;
#   CG_S0    |S_1(C eta, both CG at wfr.TRAJ_TOL_H) - |eta|^2| / |eta|^2 over LATTICES;
#   CG_FD    the relative Richardson error of the force when action and force come from the CG at wfr.FD_TOL, h = 1e-3;
#   CG_TRAJ  max |x' - x'_dense|, max |v' - v'_dense|, |dH - dH_dense| of `delta_h` with the light field, the leapfrog at
#            wfr.TRAJ_TOL_MD and the Hamiltonian at wfr.TRAJ_TOL_H.
# Measured: CG_X (2,2,2,2) 4.09e-10, (4,2,2,2) 6.30e-10, (4,4,4,4) 2.23e-11, (4,2,6,2) 9.73e-10.  CG_S 0 on both lattices
# (the error of the action is second order in the residual: below one ulp at tol_h = 1e-12; the constant is one ulp, and a
# test adds the bound of its own sums).  CG_S0 (2,2,2,2) 4.28e-16, (4,2,2,2) 1.50e-16.  CG_FD (2,2,2,2) 1.104e-10 periodic,
# 8.19e-12 antiperiodic; (4,2,2,2) 8.21e-11, 3.34e-11 (the dense figures are the same: the h^4 term of the differences).
# CG_TRAJ with the light field (2,2,2,2) x 7.59e-13, v 3.73e-12, dH 4.41e-11; (4,2,2,2) x 1.18e-12, v 4.02e-12, dH
# 2.90e-11; strange only x 1.16e-12, v 4.08e-12, dH 2.92e-11 at worst.
CG_X = 9.8e-10
CG_S = 2.3e-16
CG_S0 = 4.3e-16
CG_FD = 1.11e-10
CG_TRAJ = {'x': 1.2e-12, 'v': 4.1e-12, 'dH': 4.5e-11}


def fd_inputs(L, nb=2, npf=2):
    return we.fd_inputs(L, nb, npf)


def richardson(x, phi, p, kappa, rat, antiperiodic_t=True, tol=None, h=1e-3):
    return wfr.richardson(x, phi, p, kappa, antiperiodic_t, h,
                          action=lambda xx: rat_action(xx, phi, kappa, rat, antiperiodic_t, tol))


def measure(out=None):
    lines = []

    def say(*a):
        lines.append(' '.join(str(v) for v in a))
        print(lines[-1])
    rat = rational()
    say(f'rational: n {rat.n} [{rat.ra}, {rat.rb}] delta {rat.delta:.3g}')
    for L in LATTICES:
        for kap in (K, wfr.TRAJ['kappa'], KAPPA_LIGHT):
            ev = spectrum(wr.links(L, 2), kap)
            say('spectrum', L, kap, f'{ev.min():.4g} {ev.max():.4g}')
    w = 0.0
    for L in SOLVER_LATTICES + [(4, 2, 6, 2)]:
        x, phi = wr.links(L, 2), wr.spinors(L, 2, 2) * we.mask(L, 0)
        X, info = multishift_cg(x, phi, K, SHIFTS, tol=SOLVE_TOL)
        d = float(np.abs(X - dense_shifted(x, phi, K, SHIFTS)).max())
        say('CG_X', L, f'{d:.3g}', 'iters', info['iters'].max(), 'shift_iters', info['shift_iters'].max((0, 1)),
            'residual', f"{info['residual'].max():.3g}")
        w = max(w, d)
    say(f'CG_X worst: {w:.3g}')
    kap = wfr.TRAJ['kappa']
    for L in LATTICES:
        x, v, phi_l, phi_s = traj_inputs(L)
        assert_spectrum(x, kap, rat)
        sd = rat_action(x, phi_s, kap, rat)
        sc = rat_action(x, phi_s, kap, rat, tol=wfr.TRAJ_TOL_H)
        say('CG_S', L, f'{float((np.abs(sc - sd) / sd).max()):.3g}')
        ex = exact_action(x, phi_s, kap)
        say('S_R vs exact', L, f'{float((np.abs(sd - ex) / ex).max()):.3g}', f'delta {rat.delta:.3g}')
        eta = we.gaussian_eta_e(L, 2, 1, seed=1)
        phi, s0 = rat_refresh(x, eta, kap, rat, tol=wfr.TRAJ_TOL_H)
        say('CG_S0', L, f'{float((np.abs(rat_action(x, phi, kap, rat, tol=wfr.TRAJ_TOL_H) - s0) / s0).max()):.3g}',
            'dense', f'{float((np.abs(rat_action(x, rat_refresh(x, eta, kap, rat)[0], kap, rat) - s0) / s0).max()):.3g}')
    for L in we.FD_LATTICES:
        x, phi, p = fd_inputs(L)
        assert_spectrum(x, K, rat)
        for ap in (False, True):
            for tol in (None, wfr.FD_TOL):
                want = wfr.pair(p, rat_force(x, phi, K, rat, ap, tol))
                d = richardson(x, phi, p, K, rat, ap, tol)[0]
                say('CG_FD' if tol else 'dense FD', L, ap, f'{float((np.abs(d - want) / np.abs(want)).max()):.3g}')
    for L in LATTICES:
        for light in (True, False):
            x, v, phi_l, phi_s = traj_inputs(L, light=light)
            kw = dict(wfr.TRAJ, rat=rat, kappa_light=KAPPA_LIGHT if light else None)
            a = delta_h(x, v, phi_l, phi_s, **kw)
            b = delta_h(x, v, phi_l, phi_s, **kw, tol=wfr.TRAJ_TOL_MD, tol_h=wfr.TRAJ_TOL_H)
            assert_spectrum(a[0], kap, rat)
            say('CG_TRAJ', L, 'light' if light else 'strange only',
                {k: f'{float(np.abs(p - q).max()):.3g}' for k, p, q in zip(('x', 'v', 'dH'), a, b)}, 'dH', a[2])
    if out:
        with open(out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    import sys
    if '--measure' in sys.argv:
        measure(sys.argv[sys.argv.index('--measure') + 1] if len(sys.argv) > sys.argv.index('--measure') + 1 else None)
