#!/usr/bin/env python3
"""Timings of the local-update kernels (csrc/su3_heatbath.hip) at the cfg-4 size (SU(3) 8^4, 256 chains, fp64) by HIP
events: one heatbath sweep and one overrelaxation sweep (8 launches each) with their algorithmic GB/s, beside one
`l2q_su3_force` call (which gathers the same staples for all links once) and one plain-HMC trajectory; then, with
--therm, the wall time from a hot start at beta = 6 until the chain-mean plaquette is within 2 standard errors of its
final value, for `Trainer.thermalize`'s sweeps (nover = 3) and for plain HMC trajectories (`Trainer.warmup`'s steps).
Run as the whole program of `rocprofv3 --kernel-trace --stats -- python tools/bench_heatbath.py` for per-kernel
times; profiles/su3_heatbath.md records the output."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'l2hmc-qcd_amd'))
import l2hmc.configs as cfgs  # noqa: E402
from l2hmc import _ops as ops  # noqa: E402
from l2hmc.dynamics.pytorch.dynamics import Dynamics  # noqa: E402
from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3  # noqa: E402

HBM_PEAK = 8.0e12       # B/s, the spec figure that DESIGN.md's fractions are taken against


def timeit(fn, iters, warm=2):
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


def history(step, x, lat, nsteps):
    """chain-mean plaquette and wall time after each of nsteps calls of x = step(x)"""
    torch.cuda.synchronize()
    t0, rows = time.perf_counter(), []
    for _ in range(nsteps):
        x = step(x)
        p = lat.plaqs(x)
        torch.cuda.synchronize()
        rows.append((time.perf_counter() - t0, float(p.mean()), float(p.std() / p.numel() ** 0.5)))
    return rows


def time_to_equilibrium(rows):
    """the final value: the mean over the last quarter of the steps; -> (wall time of the first step within 2 standard
    errors of it, steps, the final value)"""
    tail = rows[-max(len(rows) // 4, 1):]
    final = sum(r[1] for r in tail) / len(tail)
    for k, (t, p, se) in enumerate(rows):
        if abs(p - final) <= 2.0 * se:
            return t, k + 1, final
    return float('nan'), len(rows), final


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nb', type=int, default=256)
    ap.add_argument('--L', type=int, nargs=4, default=[8, 8, 8, 8])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--ntry', type=int, default=4)
    ap.add_argument('--therm', action='store_true', help='also time thermalisation from a hot start at beta = 6')
    ap.add_argument('--therm-nb', type=int, default=64)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    torch.set_default_dtype(torch.float64)
    L, nb, ntry = args.L, args.nb, args.ntry
    V = L[0] * L[1] * L[2] * L[3]
    torch.manual_seed(0)
    dev = torch.device('cuda:0')
    xn = ops.su3_project_su_n(torch.randn((nb, 4, 9, V), dtype=torch.complex128, device=dev))
    links = nb * 4 * V
    u = torch.rand((nb, 3, 4 * ntry + 2, V // 2), dtype=torch.float64, device=dev)

    def hb_sweep():
        for mu in range(4):
            for parity in (0, 1):
                ops.su3_heatbath_(xn, 5.7, mu, parity, u, ntry, L)

    def or_sweep():
        for mu in range(4):
            for parity in (0, 1):
                ops.su3_overrelax_(xn, mu, parity, L)

    rows = (
        (f'heatbath sweep, ntry {ntry} (8 launches, uniforms given)', hb_sweep, 20 * 144 + 24 * (4 * ntry + 2)),
        ('overrelaxation sweep (8 launches)', or_sweep, 20 * 144),
        ('l2q_su3_force (for scale: the staples of all links)', lambda: ops.su3_force_n(xn, 5.7, L), 288),
        ('torch.rand of the uniforms of one sweep (8 draws)',
         lambda: [torch.rand(u.shape, dtype=torch.float64, device=dev) for _ in range(8)], 24 * (4 * ntry + 2)),
        ('l2q_su3_project_su (the reunitarisation of a sweep)', lambda: ops.su3_project_su_n(xn), 288),
    )
    print(f'lattice {L} x {nb} chains = {links} links, {xn.numel() * 16 / 1e6:.0f} MB per field')
    for name, fn, bytes_per_link in rows:
        t = timeit(fn, args.iters)
        rate = bytes_per_link * links / t
        print(f'{name:58s} {t * 1e3:8.3f} ms  {bytes_per_link:6d} B/link  {rate / 1e9:8.1f} GB/s  '
              f'{rate / HBM_PEAK:.3f} of 8 TB/s')
    lat = LatticeSU3(nb, L)
    dc = cfgs.DynamicsConfig(nchains=nb, group='SU3', latvolume=L, nleapfrog=10, eps=0.05, eps_hmc=0.05,
                             use_split_xnets=False, use_separate_networks=False, verbose=False)
    dyn = Dynamics(lat.action, dc, None).eval()
    x = lat.unpack(xn)
    beta = torch.tensor(6.0)
    t = timeit(lambda: dyn.apply_transition_hmc((x, beta), eps=0.05, nleapfrog=10), 3, warm=1)
    print(f'one plain-HMC trajectory (10 leapfrog steps, eps 0.05): {t * 1e3:8.3f} ms')
    if not args.therm:
        return
    nbt = args.therm_nb
    lat = LatticeSU3(nbt, L)
    dc = cfgs.DynamicsConfig(nchains=nbt, group='SU3', latvolume=L, nleapfrog=10, eps=0.05, eps_hmc=0.05,
                             use_split_xnets=False, use_separate_networks=False, verbose=False)
    dyn = Dynamics(lat.action, dc, None).eval()
    x0 = lat.random().to(dev)

    def hmc(x):
        xo, _ = dyn.apply_transition_hmc((x, beta), eps=0.05, nleapfrog=10)
        return lat.g.compat_proj(dyn.unflatten(xo.detach()))

    for name, step, nsteps in (('heatbath sweep + 3 overrelaxation sweeps', lambda x: lat.heatbath(x, 6.0, nover=3)[0], 50),
                               ('plain-HMC trajectory (10 x 0.05)', hmc, 100)):
        step(x0)                                             # warm-up of allocator and kernels
        rows = history(step, x0, lat, nsteps)
        t_eq, k, final = time_to_equilibrium(rows)
        print(f'thermalisation at beta 6.0, {L} x {nbt} chains, {name}: plaquette {final:.5f}, reached after {k} steps '
              f'= {t_eq * 1e3:.1f} ms wall ({rows[-1][0] / nsteps * 1e3:.2f} ms per step)')


if __name__ == '__main__':
    main()
