#!/usr/bin/env python3
"""Measurements of the link smearing (csrc/su3_smear.hip) for profiles/su3_smear.md, SU(3) 8^4, complex128:
  --kernels   one APE step (spatial and 4D), each HYP level, a whole HYP step (3 launches), one `l2q_su3_flow_step` and a
              field copy at --nb chains (256) by HIP events: --repeats windows of --iters calls after a warm-up, median
              and spread, with each kernel's algorithmic bytes (compulsory reads plus the write), the rate they give and
              its share of the HBM figure DESIGN.md uses, and the ratio to the flow step.  Run as the whole program of
              `rocprofv3 --kernel-trace --stats -- python tools/bench_smear.py --kernels` for per-kernel times;
  --physics   the static potential V(R; T) = ln[W(R, T) / W(R, T+1)] from `smeared_loop_table` against thin links on
              --physics-nb chains thermalised with `heatbath` at beta = 6 (nover = 3)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'l2hmc-qcd_amd'))
from l2hmc import _ops as ops  # noqa: E402
from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3, static_potential  # noqa: E402

HBM_PEAK = 8.0e12       # B/s, the spec figure that DESIGN.md's fractions are taken against
LINK = 144              # bytes of one complex128 3 x 3 link
# algorithmic bytes per (chain, site): the fields a launch must read once plus what it writes
BYTES = {'ape': (4 + 4) * LINK, 'level1': (4 + 12) * LINK, 'level2': (4 + 12 + 12) * LINK, 'level3': (4 + 12 + 4) * LINK}
BYTES['hyp'] = BYTES['level1'] + BYTES['level2'] + BYTES['level3']


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


def kernels(nb, L, iters, repeats):
    V = L[0] * L[1] * L[2] * L[3]
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    xn = ops.su3_project_su_n(torch.randn((nb, 4, 9, V), dtype=torch.complex128, device=dev))
    out, out2, ws_p, ws_x = (torch.empty_like(xn) for _ in range(4))
    b1 = torch.empty((nb, 4, 3, 9, V), dtype=torch.complex128, device=dev)
    b2 = torch.empty_like(b1)
    a1, a2, a3 = 0.75, 0.6, 0.3
    ops.su3_hyp_level1_n(xn, a3, L, out=b1)
    ops.su3_hyp_level2_n(xn, b1, a2, L, out=b2)

    def hyp():
        ops.su3_hyp_level1_n(xn, a3, L, out=b1)
        ops.su3_hyp_level2_n(xn, b1, a2, L, out=b2)
        ops.su3_hyp_level3_n(xn, b2, a1, L, out=out)

    rows = (
        ('APE step, spatial (mask 14)', lambda: ops.su3_ape_smear_n(xn, 0.5, 14, L, out=out), BYTES['ape']),
        ('APE step, 4D (mask 15)', lambda: ops.su3_ape_smear_n(xn, 0.5, 15, L, out=out), BYTES['ape']),
        ('HYP level 1', lambda: ops.su3_hyp_level1_n(xn, a3, L, out=b1), BYTES['level1']),
        ('HYP level 2', lambda: ops.su3_hyp_level2_n(xn, b1, a2, L, out=b2), BYTES['level2']),
        ('HYP level 3', lambda: ops.su3_hyp_level3_n(xn, b2, a1, L, out=out), BYTES['level3']),
        ('HYP step (3 launches)', hyp, BYTES['hyp']),
        ('l2q_su3_flow_step', lambda: ops.su3_flow_step_n(xn, out2, ws_p, ws_x, 0.01, L), None),
        ('field copy (copy_)', lambda: out.copy_(xn), 2 * 4 * LINK),
    )
    print(f'lattice {L} x {nb} chains, {xn.numel() * 16 / 1e6:.0f} MB per link field, {iters} calls per window, '
          f'{repeats} windows')
    res = {}
    for name, fn, nbytes in rows:
        ts = windows(fn, iters, repeats)
        t = statistics.median(ts)
        res[name] = t
        line = f'{name:30s} {t * 1e3:8.3f} ms (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f})'
        if nbytes is not None:
            rate = nbytes * nb * V / t
            line += f'  {nbytes:5d} B/site  {rate / 1e12:6.2f} TB/s  {rate / HBM_PEAK:.3f} of 8 TB/s'
        print(line)
    flow = res['l2q_su3_flow_step']
    for name in list(res)[:6]:
        print(f'{name:30s} = {res[name] / flow:.3f} flow steps')


def physics(nb, L, therm, rmax, tmax, ape_steps):
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    lat = LatticeSU3(nb, L)
    x = lat.heatbath(lat.random().to(dev), 6.0, nsweeps=therm, nover=3)[0]
    print(f'{L} x {nb} chains, beta 6.0 after {therm} heatbath sweeps (nover 3): plaquette '
          f'{float(lat.plaqs(x).mean()):.5f}')
    thin = lat.wilson_loop_table(x, rmax, tmax)
    smeared = lat.smeared_loop_table(x, rmax, tmax, ape_steps=ape_steps)
    for name, w in (('thin', thin), (f'APE 0.5 x {ape_steps} / HYP (0.75, 0.6, 0.3)', smeared)):
        mean, err = w.mean(0), w.std(0) / nb ** 0.5
        v = static_potential(mean)
        print(f'{name}:')
        for r in range(rmax):
            print(f'  R = {r + 1}: W(R, T) = ' + ' '.join(f'{float(mean[r, t]):.5f}({float(err[r, t]):.5f})'
                                                         for t in range(tmax))
                  + '   V(R; T) = ' + ' '.join(f'{float(v[r, t]):.4f}' for t in range(tmax - 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nb', type=int, default=256)
    ap.add_argument('--L', type=int, nargs=4, default=[8, 8, 8, 8])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--physics', action='store_true')
    ap.add_argument('--physics-nb', type=int, default=16)
    ap.add_argument('--therm', type=int, default=50)
    ap.add_argument('--rmax', type=int, default=4)
    ap.add_argument('--tmax', type=int, default=4)
    ap.add_argument('--ape-steps', type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    torch.set_default_dtype(torch.float64)
    if args.kernels:
        kernels(args.nb, args.L, args.iters, args.repeats)
    if args.physics:
        physics(args.physics_nb, args.L, args.therm, args.rmax, args.tmax, args.ape_steps)


if __name__ == '__main__':
    main()
