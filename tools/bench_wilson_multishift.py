#!/usr/bin/env python3
"""Measurements of the multi-shift CG and the one-flavour RHMC (csrc/su3_spinor_mshift.hip) for
profiles/su3_wilson_multishift.md, SU(3) 8^4 x --nb chains (256), complex128, kappa 0.12, links thermalised with --therm
heatbath sweeps at beta = 6:
  --kernels     the fused update `l2q_su3_spinor_mshift_update` at ns in --ns (1, 4, 10) on half fields by HIP events
                (--repeats windows of --iters calls after a warm-up, median and spread), its algorithmic bytes (r once, p
                read and written, four field streams per live shift) and the share of the HBM figure they give, beside
                `l2q_su3_spinor_cg_update` (x, r read and written, p, q read: 6 streams) measured in the same session,
                the two alternating; the residual step and the linear combination; the update with half the shifts frozen;
  --solver      time to --tol of `wilson_solve_multishift_n` with the ns = 10 poles of a Zolotarev approximation on [--ra,
                --rb], freezing on and off, beside one `wilson_solve_schur_normal_n` to the same tol, with iteration counts
                and the byte model (operator bytes + (3 + 4 ns) fields) / (operator bytes + 7 fields);
  --trajectory  one `WilsonRHMC` trajectory (N_f = 2 + 1) at --traj-nb chains (16), wall time, with the time inside the
                operator, the BLAS-1 kernels and the force, by timing each call with a device synchronise around it (which
                serialises the launches: the parts are upper estimates, the total is taken without it)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'l2hmc-qcd_amd'))
from l2hmc import _ops as ops  # noqa: E402
from l2hmc.dynamics.pytorch.fermion_hmc import WilsonRHMC  # noqa: E402
from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3  # noqa: E402
from l2hmc.lattice.su3.pytorch.rational import zolotarev_inv_sqrt  # noqa: E402

HBM_PEAK = 8.0e12       # B/s, the spec figure that DESIGN.md's fractions are taken against
SPINOR = 192            # bytes of one complex128 spinor (12 components)
OP_BYTES = 2 * (480 + 1152)   # per even site of one Mhat at nrhs = 1 (profiles/su3_wilson_eo.md: per site of the full lattice
                              # 480 B of spinors and 1152 B of links); Mhat^H Mhat is two of them


def windows(fn, iters, repeats, warm=3):
    """seconds per call in each of `repeats` windows of `iters` calls, by device events"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters * 1e-3)
    return out


def show(name, ts, nbytes, sites):
    t = statistics.median(ts)
    rate = nbytes * sites / t
    print(f'{name:52s} {t * 1e3:8.3f} ms (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f})  {nbytes:6.0f} B/site  '
          f'{rate / 1e12:5.2f} TB/s  {rate / HBM_PEAK:.3f} of 8 TB/s')
    return t


def links(nb, L, therm, dev):
    lat = LatticeSU3(nb, list(L))
    torch.manual_seed(0)
    xn = lat.pack(lat.heatbath(lat.random().to(dev), 6.0, nsweeps=therm, nover=3)[0])
    print(f'{L} x {nb} chains, beta 6.0 after {therm} heatbath sweeps (nover 3): plaquette '
          f'{float(lat.plaq_sums_n(xn)[:, 0].mean()) / (18.0 * lat.volume):.4f}')
    return lat, xn


def kernels(nb, L, ns_list, iters, repeats):
    dev = torch.device('cuda:0')
    Vh = L[0] * L[1] * L[2] * L[3] // 2
    sites = nb * Vh
    torch.manual_seed(1)

    def field(*shape):
        return torch.randn(shape, dtype=torch.complex128, device=dev)
    x, r, p, q = (field(nb, 1, 12, Vh) for _ in range(4))
    coef = torch.full((nb, 1), 1e-3, dtype=torch.float64, device=dev)
    rpart = torch.empty((nb, 1, -(-Vh // 256)), dtype=torch.float64, device=dev)
    print(f'half fields of {Vh} sites x {nb} chains: {x.numel() * 16 / 1e6:.0f} MB each; {iters} calls per window, {repeats} windows')
    yard = lambda: ops.su3_spinor_cg_update_(x, r, p, q, coef, rpart)          # noqa: E731
    show('cg_update (x, r rw; p, q r): the yardstick', windows(yard, iters, repeats), 6 * SPINOR, sites)
    show('axmy_norm (r rw; z r; |r|^2)', windows(lambda: ops.su3_spinor_axmy_norm_(r, q, coef, rpart), iters, repeats),
         3 * SPINOR, sites)
    for ns in ns_list:
        X, P = field(nb, 1, ns, 12, Vh), field(nb, 1, ns, 12, Vh)
        c = torch.full((nb, 1, ns), 1e-3, dtype=torch.float64, device=dev)
        one = torch.ones_like(c)
        live = torch.ones((nb, 1, ns), dtype=torch.int32, device=dev)
        fused = lambda: ops.su3_spinor_mshift_update_(X, P, p, r, c, one, c, coef, live)      # noqa: E731
        # the two alternating, twice: the spread between the passes is the session's
        for rep in range(2):
            show(f'mshift_update ns {ns} (pass {rep})', windows(fused, iters, repeats), (3 + 4 * ns) * SPINOR, sites)
            show(f'cg_update            (pass {rep})', windows(yard, iters, repeats), 6 * SPINOR, sites)
        if ns > 1:
            half = live.clone()
            half[:, :, ns // 2:] = 0
            nl = ns // 2
            show(f'mshift_update ns {ns}, {ns - nl} shifts frozen',
                 windows(lambda: ops.su3_spinor_mshift_update_(X, P, p, r, c, one, c, coef, half), iters, repeats),
                 (3 + 4 * nl) * SPINOR, sites)
        out = torch.empty_like(x)
        show(f'lincomb ns {ns}', windows(lambda: ops.su3_spinor_lincomb(X, c, out=out), iters, repeats), (ns + 1) * SPINOR, sites)
        del X, P


def solver(nb, L, therm, kappa, tol, n, ra, rb, repeats):
    dev = torch.device('cuda:0')
    lat, xn = links(nb, L, therm, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    lo, hi = lat.schur_spectrum_n(xn, kappa, iters=20, generator=g)
    print(f'spectrum estimates of Mhat^H Mhat over the chains: lambda_min {float(lo.min()):.4g} .. {float(lo.max()):.4g}, '
          f'lambda_max {float(hi.min()):.4g} .. {float(hi.max()):.4g}; rigorous bound {(1 + 64 * kappa ** 2) ** 2:.4g}')
    rat = zolotarev_inv_sqrt(n, ra, rb)
    print(f'Zolotarev n = {n} on [{ra}, {rb}]: delta {rat.delta:.3g}; shifts {rat.poles.min():.3g} .. {rat.poles.max():.3g}')
    phi = torch.randn((nb, 1, 12, lat.volume // 2), dtype=torch.complex128, device=dev)

    def timed(fn):
        fn()                                                                        # warm-up: every shape once
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), min(ts), max(ts), out
    res = {}
    for name, fn in (('schur_normal (one system)', lambda: lat.wilson_solve_schur_normal_n(xn, phi, kappa, tol=tol)[2]),
                     (f'multishift ns {n}, freezing on', lambda: lat.wilson_solve_multishift_n(xn, phi, kappa, rat.poles, tol=tol)[1]),
                     (f'multishift ns {n}, freezing off', lambda: lat.wilson_solve_multishift_n(xn, phi, kappa, rat.poles, tol=tol,
                                                                                               freeze=False)[1]),
                     ('schur_normal (again)', lambda: lat.wilson_solve_schur_normal_n(xn, phi, kappa, tol=tol)[2])):
        t, lo_, hi_, info = timed(fn)
        res[name] = t
        it = info['iters']
        extra = ''
        if 'shift_iters' in info:
            si = info['shift_iters'].to(torch.float64)
            extra = f"  shift_iters mean per shift {[round(float(v), 1) for v in si.mean((0, 1))]}"
        print(f"{name:36s} {t * 1e3:9.2f} ms (min {lo_ * 1e3:.2f}, max {hi_ * 1e3:.2f})  iters {int(it.min())}..{int(it.max())}  "
              f"residual max {float(info['residual'].max()):.3g}  converged {bool(info['converged'].all())}{extra}")
    base = res['schur_normal (one system)']
    # per iteration and even site: Mhat^H Mhat, then the BLAS-1 streams -- 7 fields for the normal CG (update 6 with x, xpay
    # 3, less r and p counted once ... the issue's model: 7), 3 + 4 ns for the fused update (the residual step's 3 apart)
    model = (2 * OP_BYTES + (3 + 4 * n) * SPINOR) / (2 * OP_BYTES + 7 * SPINOR)
    print(f'ratio multishift / normal: freezing on {res[f"multishift ns {n}, freezing on"] / base:.2f}, off '
          f'{res[f"multishift ns {n}, freezing off"] / base:.2f}; byte model (operator {2 * OP_BYTES:.0f} B/site + (3 + 4 ns) '
          f'fields) / (operator + 7 fields) = {model:.2f}')


class _Clock:
    """wraps functions of `ops` to add up the time spent in each group, with a synchronise around every call"""

    def __init__(self, groups):
        self.t = {g: 0.0 for g in groups}
        self.saved = []
        for g, names in groups.items():
            for n in names:
                fn = getattr(ops, n)
                self.saved.append((n, fn))
                setattr(ops, n, self.wrap(fn, g))

    def wrap(self, fn, g):
        def inner(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            self.t[g] += time.perf_counter() - t0
            return out
        return inner

    def restore(self):
        for n, fn in self.saved:
            setattr(ops, n, fn)


def trajectory(nb, L, therm, kappa, kappa_light, n, ra, rb):
    dev = torch.device('cuda:0')
    lat, xn = links(nb, L, therm, dev)
    rat = zolotarev_inv_sqrt(n, ra, rb)
    hmc = WilsonRHMC(lat, 6.0, kappa, 0.05, 8, rat=rat, kappa_light=kappa_light)
    g = torch.Generator(device=dev)

    def run():
        g.manual_seed(3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, m = hmc.trajectory_n(xn, g)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, m
    run()
    ts = [run() for _ in range(3)]
    t, m = sorted(ts, key=lambda v: v[0])[1]
    print(f'WilsonRHMC N_f = 2 + 1 (kappa_light {kappa_light}, kappa {kappa}, n = {n}, eps 0.05 x 8) on {L} x {nb} chains: '
          f'{t * 1e3:.1f} ms per trajectory (of 3: {[round(v[0] * 1e3, 1) for v in ts]}); acc {float(m["acc"].mean()):.2f}, '
          f'dH {float(m["dH"].abs().max()):.3g}, md iters light {m["cg_iters_md"]}, multishift {m["cg_iters_ms_md"]}, '
          f'unconverged {m["unconverged"]}')
    clock = _Clock({'operator': ['su3_wilson_hop_eo_n'],
                    'blas1': ['su3_spinor_mshift_update_', 'su3_spinor_axmy_norm_', 'su3_spinor_cg_update_',
                              'su3_spinor_xpay_', 'su3_spinor_lincomb', 'sum_parts'],
                    'force': ['su3_wilson_force_n', 'su3_force_kick_n', 'su3_spinor_merge_eo'],
                    'links': ['su3_expm_mul_n']})
    try:
        ts, _ = run()
    finally:
        clock.restore()
    rest = ts - sum(clock.t.values())
    print(f'with a synchronise around every call: {ts * 1e3:.1f} ms = ' + ', '.join(f'{k} {v * 1e3:.1f}' for k, v in clock.t.items())
          + f', the rest (torch tensor ops of the recurrences, host) {rest * 1e3:.1f} ms')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--solver', action='store_true')
    ap.add_argument('--trajectory', action='store_true')
    ap.add_argument('--nb', type=int, default=256)
    ap.add_argument('--traj-nb', type=int, default=16)
    ap.add_argument('--L', type=int, nargs=4, default=[8, 8, 8, 8])
    ap.add_argument('--ns', type=int, nargs='+', default=[1, 4, 10])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--therm', type=int, default=10)
    ap.add_argument('--kappa', type=float, default=0.12)
    ap.add_argument('--kappa-light', type=float, default=0.125)
    ap.add_argument('--tol', type=float, default=1e-10)
    ap.add_argument('--degree', type=int, default=10)
    ap.add_argument('--ra', type=float, default=0.01)
    ap.add_argument('--rb', type=float, default=4.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_wilson_multishift: needs the GPU; there is no CPU path')
    L = tuple(args.L)
    if args.kernels:
        kernels(args.nb, L, args.ns, args.iters, args.repeats)
    if args.solver:
        solver(args.nb, L, args.therm, args.kappa, args.tol, args.degree, args.ra, args.rb, 3)
    if args.trajectory:
        trajectory(args.traj_nb, L, args.therm, args.kappa, args.kappa_light, args.degree, args.ra, args.rb)
