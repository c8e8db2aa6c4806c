"""TEST INFRASTRUCTURE: numpy restatement of the mixed-precision even-odd Wilson solves (csrc/su3_wilson_f32.hip,
`LatticeSU3.wilson_solve_eo_mixed_n` / `wilson_solve_schur_normal_mixed_n`), built by import on `wilson_eo_restatement`
and `wilson_restatement`, whose functions compute in the type of their inputs: the half-lattice hop in np.complex64, the
fp32 parity-ordered link copy, the fp32 inner CGs and the fp64 defect-correction loops around them, and the even-odd
pseudofermion action, force and leapfrog with mixed solves.  Written from the formulas (include/l2q.h), not from the
kernels.

Defect correction: x = 0, r = b; while |r|^2 > tol^2 bb: solve A e = r / |r| in fp32 from zero to the relative target
max(inner_tol, SAFETY tol sqrt(bb) / |r|), x += |r| e in fp64, r = b - A x in fp64.  A converged system is frozen."""
import numpy as np

import wilson_eo_restatement as we
import wilson_force_restatement as wfr
import wilson_restatement as wr

C64 = np.complex64
INNER_TOL = 1e-4            # the product's default (wilson.MIXED_INNER_TOL); chosen from `measure_iters`
MAX_INNER = 500
MAX_OUTER = 30
SAFETY = 0.5


# ------------------------------------------------------------------ the fp32 operands and the fp32 hop
def links_eo_f32(x):
    """x[nb, 4, T, X, Y, Z, 3, 3] -> the parity-ordered fp32 copy [nb, 2, 4, 9, V/2] complex64: entry h of parity p is
    the link at the h-th site of parity p"""
    L = x.shape[2:6]
    xn = wfr.pack_links(x)
    return np.ascontiguousarray(np.stack([xn[..., we.sites(L, p)] for p in (0, 1)], 1).astype(C64))


def hop_eo_f32(x, src, p, dagger=False, antiperiodic_t=True, a=1.0, aux=None, b=0.0):
    """`we.hop_eo` in single precision: links, fields and coefficients rounded to float32 / complex64, every operation
    of the hop in that type; full-shape complex64 out"""
    return we.hop_eo(x.astype(C64), src.astype(C64), p, dagger, antiperiodic_t, np.float32(a),
                     None if aux is None else aux.astype(C64), np.float32(b))


def schur_f32(x32, psi, kappa, dagger=False, antiperiodic_t=True):
    """Mhat psi_e in complex64 on the complex64 links x32 (full shape)"""
    return we.schur(x32, psi, np.float32(kappa), dagger, antiperiodic_t)


def norm2(psi):
    """|psi|^2 per system in float64, whatever the type of psi: the kernels sum their squares in double"""
    return (psi.real.astype(np.float64) ** 2 + psi.imag.astype(np.float64) ** 2).sum(axis=tuple(range(2, psi.ndim)))


def _ratio(live, num, den):
    ok = live & (den > 0)
    return np.where(ok, num / np.where(ok, den, 1.0), 0.0)


def _bc32(a):
    """a double coefficient per system, rounded to float32 as the fp32 BLAS-1 kernels do"""
    return wr._bc(a.astype(np.float32))


# ------------------------------------------------------------------ the inner fp32 CGs: test |r|^2 <= tol^2 bb, bb given
def inner_cgnr(op, b, bb, tol, max_iter, check_every):
    """A e = b by CGNR in the type of b with float64 norms, coefficients formed in float64 and rounded to float32:
    `wr.cgnr_op` with the norms of the fp32 kernels.  Returns (e, iters)."""
    e = np.zeros_like(b)
    r = b.copy()
    z = op(r, True)
    p = z.copy()
    zz = norm2(z)
    done = bb <= tol * tol * bb
    iters = np.where(done, 0, max_iter)
    k = 0
    while k < max_iter and not done.all():
        q = op(p, False)
        alpha = _ratio(~done, zz, norm2(q))
        e = e + _bc32(alpha) * p
        r = r - _bc32(alpha) * q
        z = op(r, True)
        zn = norm2(z)
        p = z + _bc32(_ratio(~done, zn, zz)) * p
        zz = zn
        k += 1
        if k % check_every == 0 or k == max_iter:
            now = ~done & (norm2(r) <= tol * tol * bb)
            iters = np.where(now, k, iters)
            done = done | now
    return e, iters


def inner_normal(op, b, bb, tol, max_iter, check_every):
    """A^H A E = b by CG in the type of b, as `wfr.normal_cg_op` with the norms of the fp32 kernels: (E, iters)"""
    E = np.zeros_like(b)
    r = b.copy()
    p = b.copy()
    rr = norm2(b)
    done = bb <= tol * tol * bb
    iters = np.where(done, 0, max_iter)
    k = 0
    while k < max_iter and not done.all():
        q = op(p, False)
        z = op(q, True)
        alpha = _ratio(~done, rr, norm2(q))
        E = E + _bc32(alpha) * p
        r = r - _bc32(alpha) * z
        rn = norm2(r)
        p = r + _bc32(_ratio(~done, rn, rr)) * p
        rr = rn
        k += 1
        if k % check_every == 0 or k == max_iter:
            now = ~done & (rr <= tol * tol * bb)
            iters = np.where(now, k, iters)
            done = done | now
    return E, iters


# ------------------------------------------------------------------ defect correction
def defect_correction(form, op64, op32, b, bb, tol=1e-10, max_iter=1000, check_every=10, inner_tol=INNER_TOL,
                      max_inner=MAX_INNER, max_outer=MAX_OUTER):
    """A x = b (form 'cgnr': A = op, 'normal': A = op^H op) by the loop of the module's head: op64(p, dagger) in
    complex128, op32 in complex64.  Returns (x, info): 'iters' (summed inner iterations), 'outer', 'converged',
    'residual' (the last |b - A x| / sqrt(bb)), each [nb, nrhs]."""
    A = (lambda v: op64(v, False)) if form == 'cgnr' else (lambda v: op64(op64(v, False), True))
    inner = inner_cgnr if form == 'cgnr' else inner_normal
    x = np.zeros_like(b)
    r = b.copy()
    rr = wr.norm2(r)
    live = ~(bb <= tol * tol * bb)
    iters = np.zeros(bb.shape, np.int64)
    outer = np.zeros(bb.shape, np.int64)
    cycles = 0
    while True:
        live = live & ~(rr <= tol * tol * bb)
        spent = int(np.where(live, iters, 0).max())
        if not live.any() or cycles >= max_outer or spent >= max_iter:
            break
        rn = np.sqrt(np.where(live, rr, 1.0))
        r32 = (wr._bc(np.where(live, 1.0 / rn, 0.0)) * r).astype(C64)
        target = np.maximum(SAFETY * tol * np.sqrt(bb) / rn, inner_tol)
        e, it = inner(op32, r32, np.where(live, (target / inner_tol) ** 2, 0.0), inner_tol,
                      min(max_inner, max_iter - spent), check_every)
        x = x + wr._bc(np.where(live, rn, 0.0)) * e.astype(b.dtype)
        iters = iters + np.where(live, it, 0)
        outer = outer + live
        cycles += 1
        r = b - A(x)
        rr = wr.norm2(r)
    return x, {'iters': iters, 'outer': outer, 'converged': ~live,
               'residual': np.sqrt(rr / np.where(bb > 0, bb, 1.0))}


def _ops(x, kappa, antiperiodic_t):
    x32 = x.astype(C64)
    return (lambda p, d: we.schur(x, p, kappa, d, antiperiodic_t),
            lambda p, d: schur_f32(x32, p, kappa, d, antiperiodic_t))


def solve_eo_mixed(x, b, kappa, tol=1e-10, max_iter=1000, check_every=10, antiperiodic_t=True, **mixed):
    """`we.solve_eo` with the Schur system solved by defect correction: (psi, info)"""
    L = b.shape[2:6]
    be, bo = b * we.mask(L, 0), b * we.mask(L, 1)
    bhat = we.hop_eo(x, bo, 0, False, antiperiodic_t, a=kappa, aux=be, b=1.0)
    op64, op32 = _ops(x, kappa, antiperiodic_t)
    pe, info = defect_correction('cgnr', op64, op32, bhat, wr.norm2(b), tol, max_iter, check_every, **mixed)
    return pe + we.hop_eo(x, pe, 1, False, antiperiodic_t, a=kappa, aux=bo, b=1.0), info


def normal_eo_mixed(x, phi_e, kappa, tol=1e-10, max_iter=1000, check_every=10, antiperiodic_t=True, **mixed):
    """`we.normal_cg_eo` by defect correction on Mhat^H Mhat: (X_e, Y_e = Mhat X_e in complex128, info with 'action')"""
    op64, op32 = _ops(x, kappa, antiperiodic_t)
    X, info = defect_correction('normal', op64, op32, phi_e, wr.norm2(phi_e), tol, max_iter, check_every, **mixed)
    Y = op64(X, False)
    return X, Y, {**info, 'action': wr.norm2(Y)}


# S_f, its force and its leapfrog with every CG solve mixed (tol None: the dense solves of `we`)
fermion_action, fermion_force, total_force, leapfrog, hamiltonian, delta_h = wfr.Trajectory(
    we.dense_normal_eo, normal_eo_mixed, we.completed).names()


# ------------------------------------------------------------------ the tolerances of the mixed-precision tests
MEASURE_LATTICES = we.EO_KERNEL_LATTICES + [(4, 4, 4, 8), (4, 4, 4, 10)]

# Yardstick of a single fp32 hop: the largest element-wise distance between `hop_eo_f32` (every operation in complex64)
# and `we.hop_eo` in np.clongdouble on the same float32-rounded operands (links, src, aux, a, b: what is measured is the
# arithmetic of the hop, not the rounding of its inputs, which kernel and restatement share), on wr.links / wr.spinors /
# we.aux_field at nb = 3, nrhs = 12 over MEASURE_LATTICES, both parities, all four wr.FLAGS and the four uses at kappa =
# wr.KAPPA.  `python tests/wilson_mixed_restatement.py --measure` prints the table (profiles/su3_wilson_mixed.md);
# measured per lattice (2,2,2,2) 2.61e-06, (4,2,6,2) 2.31e-06, (2,4,2,6) 2.38e-06, (4,4,4,8) 2.65e-06, (4,4,4,10)
# 2.95e-06: worst 2.95e-06 (the use a = 1, |out| up to ~40: about one float32 ulp of the largest entries; the other
# three uses stay below 5.6e-07).  The tolerance is 32 x the yardstick, the project's convention: it covers fma
# contraction and the order of the kernel's sums.
YARDSTICK_F32 = 3.0e-6
TOL_F32 = 32.0 * YARDSTICK_F32


def norm_bound_f32(Vh):
    """relative bound on the kernel's float64 norm partials against the float64 sum of squares of the kernel's own
    float32 output: the square of a float32 is exact in float64, so what is left is the order of n = 24 Vh float64
    additions (and the fma, which rounds once where square-then-add rounds once): the form of `wr.norm_bound`"""
    return wr.norm_bound(Vh)


# Distances of this restatement from itself when its solves are mixed-precision defect correction instead of dense
# solves, measured on the CPU by `python tests/wilson_mixed_restatement.py --measure-cg` on the inputs of the even-odd
# tests (`we.traj_inputs`, `we.fd_inputs`), the counterparts of we.CG_S0 / CG_FD / CG_TRAJ; the tests allow 32 x each:
#   CG_S0    |S_f(mixed at wfr.TRAJ_TOL_H) - S0| / S0 of `we.refresh` over wfr.TRAJ_LATTICES;
#   CG_FD    the relative Richardson error over we.FD_LATTICES when action and force come from mixed solves at wfr.FD_TOL;
#   CG_TRAJ  max |x' - x'_dense|, max |v' - v'_dense|, |dH - dH_dense| of `delta_h` over wfr.TRAJ_LATTICES, the leapfrog
#            solving at wfr.TRAJ_TOL_MD and the Hamiltonian at wfr.TRAJ_TOL_H.
#   CG_X     max |psi_mixed - psi_dense| / max |psi_dense| of `solve_eo_mixed` at tol 1e-10 on (2,2,2,2), (4,2,2,2) at
#            wr.SOLVE_KAPPAS (the solution-level figure of the GPU solve tests).
# Measured: CG_S0 (2,2,2,2) 1.48e-16, (4,2,2,2) 2.03e-13.  CG_FD (2,2,2,2) 1.91e-10 periodic, 1.26e-11 antiperiodic;
# (4,2,2,2) 1.27e-10, 3.34e-11.  CG_TRAJ (2,2,2,2) x 8.58e-12, v 3.73e-11, dH 4.11e-10; (4,2,2,2) x 1.00e-13, v 7.57e-13,
# dH 1.17e-11.  CG_X (2,2,2,2) 4.96e-14 (kappa 0.10), 1.10e-10 (0.12); (4,2,2,2) 1.38e-10 (0.10), 4.43e-13 (0.12).
CG_S0 = 2.1e-13
CG_FD = 2.0e-10
CG_TRAJ = {'x': 8.6e-12, 'v': 3.8e-11, 'dH': 4.2e-10}
CG_X = 1.4e-10


def measure(lattices=None, nb=3, nrhs=12):
    worst = 0.0
    for L in lattices or MEASURE_LATTICES:
        x, psi, aux = (t.astype(C64) for t in (wr.links(L, nb), wr.spinors(L, nb, nrhs), we.aux_field(L, nb, nrhs)))
        xl, pl, al = (t.astype(np.clongdouble) for t in (x, psi, aux))
        here = {}
        for name, a, b, with_aux in we.uses():
            a32, b32 = np.float32(a), np.float32(b)
            for p in (0, 1):
                for dagger, ap in wr.FLAGS:
                    d = hop_eo_f32(x, psi, p, dagger, ap, a32, aux if with_aux else None, b32) \
                        - we.hop_eo(xl, pl, p, dagger, ap, np.longdouble(a32), al if with_aux else None, np.longdouble(b32))
                    here[name] = max(here.get(name, 0.0), float(np.abs(d).max()))
        print(L, {k: f'{v:.3g}' for k, v in here.items()})
        worst = max(worst, max(here.values()))
    print(f'worst: {worst:.3g}')
    return worst


def measure_cg():
    w0 = 0.0
    for L in wfr.TRAJ_LATTICES:
        x, _, phi, s0 = we.traj_inputs(L)
        d = float((np.abs(fermion_action(x, phi, wfr.TRAJ['kappa'], True, wfr.TRAJ_TOL_H) - s0) / s0).max())
        print('CG_S0', L, f'{d:.3g}')
        w0 = max(w0, d)
    print(f'CG_S0 worst: {w0:.3g}')
    worst = 0.0
    for L in we.FD_LATTICES:
        x, phi, p = we.fd_inputs(L)
        for ap in (False, True):
            want = wfr.pair(p, fermion_force(x, phi, we.K, ap, wfr.FD_TOL))
            d = wfr.richardson(x, phi, p, we.K, ap, action=lambda xx: fermion_action(xx, phi, we.K, ap, wfr.FD_TOL))[0]
            rel = float((np.abs(d - want) / np.abs(want)).max())
            print('CG_FD', L, ap, f'{rel:.3g}')
            worst = max(worst, rel)
    print(f'CG_FD worst: {worst:.3g}')
    w = {'x': 0.0, 'v': 0.0, 'dH': 0.0}
    for L in wfr.TRAJ_LATTICES:
        x, v, phi, _ = we.traj_inputs(L)
        a = we.delta_h(x, v, phi, **wfr.TRAJ)
        b = delta_h(x, v, phi, **wfr.TRAJ, tol=wfr.TRAJ_TOL_MD, tol_h=wfr.TRAJ_TOL_H)
        here = {k: float(np.abs(p - q).max()) for k, p, q in zip(('x', 'v', 'dH'), a, b)}
        print('CG_TRAJ', L, here)
        w = {k: max(w[k], here[k]) for k in w}
    print('CG_TRAJ worst:', w)
    wx = 0.0
    for L in we.FD_LATTICES:
        x, b = wr.links(L, 2), wr.spinors(L, 2, 2)
        for kappa in wr.SOLVE_KAPPAS:
            psi = solve_eo_mixed(x, b, kappa, tol=1e-10)[0]
            here = 0.0
            for c in range(2):
                m = wr.dense(x[c:c + 1], kappa)
                want = np.linalg.solve(m, b[c].reshape(2, -1).T).T.reshape(b.shape[1:])
                here = max(here, float(np.abs(psi[c] - want).max() / np.abs(want).max()))
            print('CG_X', L, kappa, f'{here:.3g}')
            wx = max(wx, here)
    print(f'CG_X worst: {wx:.3g}')


def measure_iters(inner_tols=(1e-3, 1e-4, 1e-5, 1e-6), nb=3, nrhs=2):
    """summed inner iterations and outer cycles of `solve_eo_mixed` over we.SOLVE_LATTICES at kappa = 0.124, tol 1e-10
    and 1e-12, for each inner_tol; beside the fp64 even-odd CGNR (the table of profiles/su3_wilson_mixed.md)"""
    total = {t: 0 for t in inner_tols}
    for L in we.SOLVE_LATTICES:
        x, b = wr.links(L, nb), wr.spinors(L, nb, nrhs)
        for tol in (1e-10, 1e-12):
            ref = we.solve_eo(x, b, wr.KAPPA, tol=tol)[1]
            print('iters', L, tol, f"fp64 {ref['iters'].min()}-{ref['iters'].max()}")
            for it in inner_tols:
                info = solve_eo_mixed(x, b, wr.KAPPA, tol=tol, inner_tol=it)[1]
                total[it] += int(info['iters'].sum())
                print('iters', L, tol, f'inner_tol {it:g}', f"inner {info['iters'].min()}-{info['iters'].max()}",
                      f"outer {info['outer'].min()}-{info['outer'].max()}", f"residual {info['residual'].max():.3g}",
                      'converged' if info['converged'].all() else 'NOT CONVERGED')
    print('summed inner iterations:', {f'{k:g}': v for k, v in total.items()})
    return total


if __name__ == '__main__':
    import sys
    if '--measure' in sys.argv:
        measure()
    if '--measure-cg' in sys.argv:
        measure_cg()
    if '--measure-iters' in sys.argv:
        measure_iters()
