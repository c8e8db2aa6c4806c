"""TEST INFRASTRUCTURE: numpy restatement of even-odd preconditioning of the Wilson-Dirac operator, built on `wr.hop` /
`wr.wilson` (tests/wilson_restatement.py) with parity masks, and of what stands on it: the half-lattice hop, the Schur
complement Mhat, the preconditioned CGNR solve with reconstruction, the CG on Mhat^H Mhat, the even-odd pseudofermion
action, heatbath and force, and the leapfrog with them (the gauge part and the long-form force: `wilson_force_restatement`).
Written from the formulas (include/l2q.h, csrc/su3_wilson_eo.hip), not from the kernel.

The parity of a site is (t + x + y + z) & 1, 0 even.  H couples sites of opposite parity only, so with M = 1 - kappa H
    Mhat = 1 - kappa^2 H_eo H_oe,   Mhat psi_e = b_e + kappa H_eo b_o,   psi_o = b_o + kappa H_oe psi_e,   det M = det Mhat.
A half field is held here as a full-shape field ``[nb, nrhs, T, X, Y, Z, 4, 3]`` that is zero on the other parity;
`pack_half` / `unpack_half` go to and from the native half layout ``[nb, nrhs, 12, V/2]`` (the sites of one parity in
lexicographic order).  Every function computes in the type of its inputs, which is how `measure()` evaluates the same
expressions in extended precision."""
import functools

import numpy as np

import wilson_force_restatement as wfr
import wilson_restatement as wr


# ------------------------------------------------------------------ parities and the half layout
@functools.lru_cache(maxsize=None)
def parity(L):
    """[T, X, Y, Z] int: (t + x + y + z) & 1"""
    return sum(np.meshgrid(*[np.arange(e) for e in L], indexing='ij')) & 1


def mask(L, p):
    """[T, X, Y, Z, 1, 1] bool: the sites of parity p"""
    return (parity(tuple(L)) == p)[..., None, None]


def sites(L, p):
    """the lexicographic site indices of parity p, ascending: [V/2]"""
    return np.nonzero(parity(tuple(L)).reshape(-1) == p)[0]


def pack_half(psi, p):
    """full-shape [nb, nrhs, T, X, Y, Z, 4, 3] -> native half field [nb, nrhs, 12, V/2] of parity p"""
    return np.ascontiguousarray(wr.pack_spinor(psi)[..., sites(psi.shape[2:6], p)])


def unpack_half(hn, L, p):
    """native half field -> full-shape field, zero on the other parity"""
    full = np.zeros((*hn.shape[:3], int(np.prod(L))), hn.dtype)
    full[..., sites(L, p)] = hn
    return wr.unpack_spinor(full, L)


# ------------------------------------------------------------------ the hop and the Schur complement
def hop_eo(x, src, p, dagger=False, antiperiodic_t=True, a=1.0, aux=None, b=0.0):
    """out = b aux + a H src on the sites of parity p, zero on the others; of src only the other parity is read, of aux
    only parity p"""
    L = src.shape[2:6]
    rt = src.real.dtype.type
    out = rt(a) * (wr.hop(x, src * mask(L, 1 - p), dagger, antiperiodic_t) * mask(L, p))
    return out if aux is None else out + rt(b) * (aux * mask(L, p))


def schur(x, psi, kappa, dagger=False, antiperiodic_t=True):
    """Mhat psi_e (dagger: Mhat^H psi_e) of the even part of psi; zero on the odd sites"""
    odd = hop_eo(x, psi, 1, dagger, antiperiodic_t)
    return hop_eo(x, odd, 0, dagger, antiperiodic_t, a=-kappa * kappa, aux=psi, b=1.0)


def even_index(L):
    """the rows of `wr.dense` that belong to even sites: [12 V/2]"""
    return (12 * sites(L, 0)[:, None] + np.arange(12)).reshape(-1)


def dense_schur(x, kappa, antiperiodic_t=True):
    """Mhat of chain 0 of x as a dense matrix [12 V/2, 12 V/2], even sites in lexicographic order, then spin, colour"""
    L = x.shape[2:6]
    n = 12 * int(np.prod(L))
    idx = even_index(L)
    basis = np.eye(n, dtype=complex)[idx].reshape(1, len(idx), *L, 4, 3)
    return schur(x[:1], basis, kappa, False, antiperiodic_t).reshape(len(idx), n).T[idx]


# ------------------------------------------------------------------ the solves: `wr.cgnr_op` and `wfr.normal_cg_op`
def full_cgnr(x, b, kappa, tol=1e-10, max_iter=1000, check_every=10, antiperiodic_t=True):
    """`wr.cgnr_op` on the full M: (psi, iters) -- the unpreconditioned solve by the same loop, for the iteration counts"""
    psi, iters, _ = wr.cgnr_op(lambda p, d: wr.wilson(x, p, kappa, d, antiperiodic_t), b, wr.norm2(b), tol, max_iter,
                            check_every)
    return psi, iters


def solve_eo(x, b, kappa, tol=1e-10, max_iter=1000, check_every=10, antiperiodic_t=True):
    """M psi = b through the Schur complement: split, bhat_e = b_e + kappa H_eo b_o, CGNR on Mhat from zero stopping on
    |rhat|^2 <= tol^2 |b|^2 (|b|^2 of the full right-hand side), psi_o = b_o + kappa H_oe psi_e.  Returns (psi, info);
    info['residual'] is the full |b - M psi| / |b|."""
    L = b.shape[2:6]
    be, bo = b * mask(L, 0), b * mask(L, 1)
    bb = wr.norm2(b)
    bhat = hop_eo(x, bo, 0, False, antiperiodic_t, a=kappa, aux=be, b=1.0)
    pe, iters, done = wr.cgnr_op(lambda p, d: schur(x, p, kappa, d, antiperiodic_t), bhat, bb, tol, max_iter, check_every)
    psi = pe + hop_eo(x, pe, 1, False, antiperiodic_t, a=kappa, aux=bo, b=1.0)
    res = np.sqrt(wr.norm2(b - wr.wilson(x, psi, kappa, False, antiperiodic_t)) / np.where(bb > 0, bb, 1.0))
    return psi, {'iters': iters, 'residual': res, 'converged': done}


# ------------------------------------------------------------------ the even-odd pseudofermions
def dense_normal_eo(x, phi_e, kappa, antiperiodic_t=True):
    """(X_e, Y_e) by a dense solve of Mhat^H Mhat X_e = phi_e, chain by chain"""
    L = x.shape[2:6]
    idx = even_index(L)
    X = np.zeros_like(phi_e)
    for c in range(x.shape[0]):
        m = dense_schur(x[c:c + 1], kappa, antiperiodic_t)
        b = phi_e[c].reshape(phi_e.shape[1], -1)[:, idx].T
        flat = np.zeros((phi_e.shape[1], 12 * int(np.prod(L))), complex)
        flat[:, idx] = np.linalg.solve(m.conj().T @ m, b).T
        X[c] = flat.reshape(phi_e.shape[1:])
    return X, schur(x, X, kappa, False, antiperiodic_t)


def normal_cg_eo(x, phi_e, kappa, tol=1e-10, max_iter=1000, check_every=10, antiperiodic_t=True):
    """Mhat^H Mhat X_e = phi_e by `wfr.normal_cg_op` on the Schur complement: (X_e, Y_e = Mhat X_e, info)"""
    return wfr.normal_cg_op(lambda p, d: schur(x, p, kappa, d, antiperiodic_t), phi_e, tol, max_iter, check_every)


def completed(x, Xe, Ye, kappa, antiperiodic_t=True):
    """the full fields X = X_e + kappa H_oe X_e, Y = Y_e + kappa (H^H)_oe Y_e whose full-lattice force is the even-odd one"""
    return (Xe + hop_eo(x, Xe, 1, False, antiperiodic_t, a=kappa),
            Ye + hop_eo(x, Ye, 1, True, antiperiodic_t, a=kappa))


# S_f [nb] = sum_r |Y_e,r|^2 = sum_r phi_e,r^H (Mhat^H Mhat)^-1 phi_e,r, its force (that of the completed fields) and its leapfrog
fermion_action, fermion_force, total_force, leapfrog, hamiltonian, delta_h = wfr.Trajectory(
    dense_normal_eo, normal_cg_eo, completed).names()


def refresh(x, eta_e, kappa, antiperiodic_t=True):
    """(phi_e, S0): phi_e = Mhat^H eta_e, S0 = |eta_e|^2 [nb]"""
    L = eta_e.shape[2:6]
    eta_e = eta_e * mask(L, 0)
    return schur(x, eta_e, kappa, True, antiperiodic_t), wr.norm2(eta_e).sum(1)


# ------------------------------------------------------------------ the inputs and the tolerances of the even-odd tests
EO_KERNEL_LATTICES = [(2, 2, 2, 2), (4, 2, 6, 2), (2, 4, 2, 6)]                   # host emulation and GPU
EO_GPU_LATTICES = EO_KERNEL_LATTICES + [(4, 4, 4, 8), (4, 4, 4, 10)]              # V/2 = 256: whole blocks; 320: a partial one
SOLVE_LATTICES = [(4, 4, 4, 4), (4, 2, 6, 2), (4, 4, 4, 10)]
FD_LATTICES = [(2, 2, 2, 2), (4, 2, 2, 2)]
K = wr.KAPPA


def uses(kappa=K):
    """the four uses (name, a, b, aux given) of the one kernel"""
    return [('hop', 1.0, 0.0, False), ('schur', -kappa * kappa, 1.0, True), ('source', kappa, 1.0, True),
            ('reconstruct', kappa, 1.0, True)]


def aux_field(L, nb=3, nrhs=12):
    """the aux operand of the kernel tests: `wr.spinors` with the right-hand sides rotated by six"""
    return np.ascontiguousarray(np.roll(wr.spinors(L, 3, 12), 6, axis=1)[:nb, :nrhs])


# Yardstick of a single hop: the largest element-wise distance between `hop_eo` in complex128 and in np.clongdouble on
# wr.links / wr.spinors / aux_field at nb = 3, nrhs = 12 over EO_GPU_LATTICES, both parities, all four wr.FLAGS and the
# four uses at kappa = wr.KAPPA.  wr.TOL does not serve: with a = 1 the outputs are ~1/kappa larger than those of M (|out|
# up to ~40).  `python tests/wilson_eo_restatement.py --measure` prints the table (profiles/su3_wilson_eo.md); measured
# per lattice (2,2,2,2) 4.12e-15, (4,2,6,2) 4.76e-15, (2,4,2,6) 4.92e-15, (4,4,4,8) 5.39e-15, (4,4,4,10) 5.31e-15: worst
# 5.39e-15 (the use a = 1; the other three uses stay below 8.7e-16).  The tolerance is 32 x the yardstick, as for the other
# SU(3) kernels: it covers fma contraction and the order of the kernel's sums and nothing else.
YARDSTICK = 5.4e-15
TOL = 32.0 * YARDSTICK

# Distances of this restatement from itself when its solves are its own CG instead of dense solves, measured on the CPU
# by `python tests/wilson_eo_restatement.py --measure-cg` on the inputs of the GPU tests, which allow 32 x each (a CG solve
# is not a dense solve: what separates them is the solver tolerance, not rounding):
#   CG_S0    |S_f(CG at wfr.TRAJ_TOL_H) - S0| / S0 of `refresh` on `traj_inputs` over wfr.TRAJ_LATTICES;
#   CG_FD    the relative Richardson error of `wfr.richardson` over FD_LATTICES when action and force come from the CG at
#            wfr.FD_TOL (both boundary conditions), h = 1e-3;
#   CG_TRAJ  max |x' - x'_dense|, max |v' - v'_dense| and |dH - dH_dense| of `delta_h` over wfr.TRAJ_LATTICES when the
#            leapfrog solves at wfr.TRAJ_TOL_MD and the Hamiltonian at wfr.TRAJ_TOL_H.
# Measured: CG_S0 (2,2,2,2) 1.48e-16, (4,2,2,2) 1.39e-16 (the error of |Y|^2 is second order in the residual: at tol_h =
# 1e-12 only rounding is left; a test adds the bound of its own sums).  CG_FD (2,2,2,2) 1.93e-10 periodic, 1.49e-11
# antiperiodic; (4,2,2,2) 1.28e-10, 3.22e-11.  CG_TRAJ (2,2,2,2) x 3.76e-12, v 1.61e-11, dH 2.27e-10; (4,2,2,2) x 1.26e-11,
# v 3.58e-11, dH 7.32e-10.
CG_S0 = 1.5e-16
CG_FD = 2.0e-10
CG_TRAJ = {'x': 1.3e-11, 'v': 3.6e-11, 'dH': 7.4e-10}


def gaussian_eta_e(L, nb, npf, seed=0):
    return wfr.gaussian_eta(L, nb, npf, seed) * mask(L, 0)


def fd_inputs(L, nb=2, npf=2):
    """(x, phi_e, p) of the finite-difference tests"""
    return wr.links(L, nb), wr.spinors(L, nb, npf) * mask(L, 0), wfr.momentum(L, nb)


def traj_inputs(L, nb=2, npf=1):
    """(x, v, phi_e, S0) of the trajectory tests, as `wfr.traj_inputs` (momentum seed 1)"""
    x = wr.links(L, nb)
    phi, s0 = refresh(x, gaussian_eta_e(L, nb, npf), wfr.TRAJ['kappa'])
    return x, wfr.momentum(L, nb, 1), phi, s0


def measure(lattices=None, nb=3, nrhs=12):
    worst = 0.0
    for L in lattices or EO_GPU_LATTICES:
        x, psi, aux = wr.links(L, nb), wr.spinors(L, nb, nrhs), aux_field(L, nb, nrhs)
        xl, pl, al = (t.astype(np.clongdouble) for t in (x, psi, aux))
        here = {}
        for name, a, b, with_aux in uses():
            for p in (0, 1):
                for dagger, ap in wr.FLAGS:
                    d = hop_eo(x, psi, p, dagger, ap, a, aux if with_aux else None, b) \
                        - hop_eo(xl, pl, p, dagger, ap, np.longdouble(a), al if with_aux else None, np.longdouble(b))
                    here[name] = max(here.get(name, 0.0), float(np.abs(d).max()))
        print(L, {k: f'{v:.3g}' for k, v in here.items()})
        worst = max(worst, max(here.values()))
    print(f'worst: {worst:.3g}')
    return worst


def measure_cg():
    w0 = 0.0
    for L in wfr.TRAJ_LATTICES:
        x, _, phi, s0 = traj_inputs(L)
        d = float((np.abs(fermion_action(x, phi, wfr.TRAJ['kappa'], True, wfr.TRAJ_TOL_H) - s0) / s0).max())
        print('CG_S0', L, f'{d:.3g}')
        w0 = max(w0, d)
    print(f'CG_S0 worst: {w0:.3g}')
    worst = 0.0
    for L in FD_LATTICES:
        x, phi, p = fd_inputs(L)
        for ap in (False, True):
            want = wfr.pair(p, fermion_force(x, phi, K, ap, wfr.FD_TOL))
            d = wfr.richardson(x, phi, p, K, ap, action=lambda xx: fermion_action(xx, phi, K, ap, wfr.FD_TOL))[0]
            rel = float((np.abs(d - want) / np.abs(want)).max())
            print('CG_FD', L, ap, f'{rel:.3g}')
            worst = max(worst, rel)
    print(f'CG_FD worst: {worst:.3g}')
    w = {'x': 0.0, 'v': 0.0, 'dH': 0.0}
    for L in wfr.TRAJ_LATTICES:
        x, v, phi, _ = traj_inputs(L)
        a = delta_h(x, v, phi, **wfr.TRAJ)
        b = delta_h(x, v, phi, **wfr.TRAJ, tol=wfr.TRAJ_TOL_MD, tol_h=wfr.TRAJ_TOL_H)
        here = {k: float(np.abs(p - q).max()) for k, p, q in zip(('x', 'v', 'dH'), a, b)}
        print('CG_TRAJ', L, here)
        w = {k: max(w[k], here[k]) for k in w}
    print('CG_TRAJ worst:', w)


def measure_iters():
    """the iteration counts of the full and the even-odd CGNR, check_every = 1 (the table of profiles/su3_wilson_eo.md)"""
    for L in [(2, 2, 2, 2), (4, 4, 4, 4), (4, 2, 6, 2), (4, 4, 4, 10)]:
        x, b = wr.links(L, 3), wr.spinors(L, 3, 2)
        for kappa in wr.SOLVE_KAPPAS:
            full = full_cgnr(x, b, kappa, check_every=1)[1]
            eo = solve_eo(x, b, kappa, check_every=1)
            print('iters', L, kappa, f'full {full.min()}-{full.max()}', f"even-odd {eo[1]['iters'].min()}-{eo[1]['iters'].max()}",
                  f"residual {eo[1]['residual'].max():.3g}")


if __name__ == '__main__':
    import sys
    if '--measure' in sys.argv:
        measure()
    if '--measure-cg' in sys.argv:
        measure_cg()
    if '--measure-iters' in sys.argv:
        measure_iters()
