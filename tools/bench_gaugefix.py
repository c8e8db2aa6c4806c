#!/usr/bin/env python3
"""Measurements of the gauge fixing (csrc/su3_gaugefix.hip) for profiles/su3_gaugefix.md, SU(3) 8^4, fp64:
  --kernels   one sweep (2 launches) with and without the accumulated transformation G, the gauge condition and the
              transformation kernel at --nb chains (256) by HIP events, with their algorithmic bytes and rates.  Run as
              the whole program of `rocprofv3 --kernel-trace --stats -- python tools/bench_gaugefix.py --kernels` for
              per-kernel times;
  --omega     sweeps and wall time to theta <= tol on chains thermalised at beta = 6 (`Trainer.thermalize`'s sweeps:
              heatbath with nover = 3), per omega in {1.0, 1.3, 1.5, 1.7, 1.9}, in Landau and in Coulomb gauge, and the
              share of the wall time that the reads of theta cost at check_every = 10."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'l2hmc-qcd_amd'))
from l2hmc import _ops as ops  # noqa: E402
from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3  # noqa: E402

HBM_PEAK = 8.0e12       # B/s, the spec figure that DESIGN.md's fractions are taken against
OMEGAS = (1.0, 1.3, 1.5, 1.7, 1.9)


def timeit(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def kernels(nb, L, iters):
    V = L[0] * L[1] * L[2] * L[3]
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    xn = ops.su3_project_su_n(torch.randn((nb, 4, 9, V), dtype=torch.complex128, device=dev))
    gn = ops.su3_project_su_n(torch.randn((nb, 1, 9, V), dtype=torch.complex128, device=dev)).reshape(nb, 9, V)
    active = torch.ones(nb, dtype=torch.int32, device=dev)
    field = xn.numel() * 16

    def sweep(g, mask=15, omega=1.7):
        for parity in (0, 1):
            ops.su3_gaugefix_sweep_(xn, parity, mask, omega, L, g, active)

    rows = (
        ('sweep, Landau (2 launches)', lambda: sweep(None), 4.0),
        ('sweep, Landau, with G (2 launches)', lambda: sweep(gn), 5.0),
        ('sweep, Coulomb (2 launches)', lambda: sweep(None, 14), 4.0),
        ('sweep, Landau, omega = 1', lambda: sweep(None, 15, 1.0), 4.0),
        ('l2q_su3_gauge_condition, Landau', lambda: ops.su3_gauge_condition_n(xn, 15, L), 1.0),
        ('l2q_su3_gauge_apply', lambda: ops.su3_gauge_apply_n(xn, gn, L), 2.25),
        ('field copy (clone)', lambda: xn.clone(), 2.0),
        ('overrelaxation sweep (8 launches)',
         lambda: [ops.su3_overrelax_(xn, mu, p, L) for mu in range(4) for p in (0, 1)], 20.0),
    )
    print(f'lattice {L} x {nb} chains, {field / 1e6:.0f} MB per field')
    for name, fn, fields in rows:
        t = timeit(fn, iters)
        rate = fields * field / t
        print(f'{name:42s} {t * 1e3:8.3f} ms  {fields:5.2f} fields  {rate / 1e12:6.2f} TB/s  '
              f'{rate / HBM_PEAK:.3f} of 8 TB/s')


def omega_table(nb, L, tol, max_sweeps, therm):
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    lat = LatticeSU3(nb, L)
    x = lat.heatbath(lat.random().to(dev), 6.0, nsweeps=therm, nover=3)[0]
    xn = lat.pack(x)
    print(f'{L} x {nb} chains, beta 6.0 after {therm} heatbath sweeps (nover 3): plaquette '
          f'{float(lat.plaqs(x).mean()):.5f}; tol {tol:g}, check_every 10, max_sweeps {max_sweeps}')
    lat.gauge_fix_n(xn, max_sweeps=20)                        # warm-up of allocator and kernels
    for gauge in ('landau', 'coulomb'):
        for omega in OMEGAS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, info = lat.gauge_fix_n(xn, gauge=gauge, omega=omega, tol=tol, max_sweeps=max_sweeps)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            s = info['sweeps'].double()
            print(f'{gauge:8s} omega {omega:.1f}: sweeps mean {float(s.mean()):7.1f} median {float(s.median()):6.0f} '
                  f'max {int(s.max()):5d}, converged {int(info["converged"].sum())}/{nb}, wall {t * 1e3:8.1f} ms, '
                  f'F {float(info["functional"].mean()):.5f} +- {float(info["functional"].std()):.5f}')
    # what the reads of theta cost: the same sweeps with one check at the end
    mask, omega, n = 15, 1.7, 200
    active = torch.ones(nb, dtype=torch.int32, device=dev)
    for every in (10, n):
        y = xn.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(n):
            for parity in (0, 1):
                ops.su3_gaugefix_sweep_(y, parity, mask, omega, L, None, active)
            if (k + 1) % every == 0:
                ops.su3_gauge_condition_n(y, mask, L).cpu()
        torch.cuda.synchronize()
        print(f'{n} Landau sweeps, theta read every {every}: {(time.perf_counter() - t0) * 1e3:.1f} ms wall')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nb', type=int, default=256)
    ap.add_argument('--L', type=int, nargs=4, default=[8, 8, 8, 8])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--omega', action='store_true')
    ap.add_argument('--omega-nb', type=int, default=16)
    ap.add_argument('--tol', type=float, default=1e-12)
    ap.add_argument('--max-sweeps', type=int, default=10000)
    ap.add_argument('--therm', type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    torch.set_default_dtype(torch.float64)
    if args.kernels:
        kernels(args.nb, args.L, args.iters)
    if args.omega:
        omega_table(args.omega_nb, args.L, args.tol, args.max_sweeps, args.therm)


if __name__ == '__main__':
    main()
