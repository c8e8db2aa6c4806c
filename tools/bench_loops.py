#!/usr/bin/env python3
"""Timings of the loop observables (csrc/su3_loops.hip) at the cfg-4 size (SU(3) 8^4, 256 chains, fp64): the three
kernels by HIP events with their algorithmic GB/s, and `LatticeSU3.wilson_loop_table(x, 4, 4)` against the same
table written with torch.roll and matmul on the device (what a user without the kernels would write).  Run as the
whole program of `rocprofv3 --kernel-trace --stats -- python tools/bench_loops.py` for the per-kernel times that
profiles/su3_loops.md records."""
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


def wall(fn, iters, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters, out


def torch_loop_table(x, rmax, tmax, time_dir=0):
    """`wilson_loop_table` with torch ops on the reference layout x[nb, 4, T, X, Y, Z, 3, 3]"""
    def sh(f, mu, n):
        return torch.roll(f, -n, dims=mu + 1)

    def line(mu, n):
        m = x[:, mu]
        for k in range(1, n):
            m = m @ sh(x[:, mu], mu, k)
        return m
    nb = x.shape[0]
    vol = x[0, 0].numel() // 9
    out = torch.zeros((nb, rmax, tmax), dtype=torch.float64, device=x.device)
    for t in range(1, tmax + 1):
        b = line(time_dir, t)
        for mu in range(4):
            if mu == time_dir:
                continue
            for r in range(1, rmax + 1):
                a = line(mu, r)
                w = a @ sh(b, mu, r) @ sh(a, time_dir, t).conj().transpose(-1, -2) @ b.conj().transpose(-1, -2)
                out[:, r - 1, t - 1] += w.diagonal(dim1=-2, dim2=-1).sum(-1).real.reshape(nb, -1).sum(-1)
    return out / (9.0 * vol)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nb', type=int, default=256)
    ap.add_argument('--L', type=int, nargs=4, default=[8, 8, 8, 8])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--no-torch', action='store_true', help='skip the torch.roll table')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    L, nb = args.L, args.nb
    V = L[0] * L[1] * L[2] * L[3]
    torch.manual_seed(0)
    dev = torch.device('cuda:0')
    xn = ops.su3_project_su_n(torch.randn((nb, 4, 9, V), dtype=torch.complex128, device=dev))
    lat = LatticeSU3(nb, L)
    sites = nb * V
    a2, b3 = ops.su3_line_extend_n(xn, xn, 1, L), torch.empty_like(xn)
    ops.su3_line_extend_n(a2, xn, 2, L, out=b3)
    rows = (
        ('su3_line_extend', lambda: ops.su3_line_extend_n(a2, xn, 2, L, out=b3), 1728),
        ('su3_loop_reduce r=t=1 (a = b = links)', lambda: ops.su3_loop_sums_n(xn, 1, xn, 1, L), 576),
        ('su3_loop_reduce r=2 t=3 (a != b)', lambda: ops.su3_loop_sums_n(a2, 2, b3, 3, L), 1152),
        ('su3_polyakov mu=0', lambda: ops.su3_polyakov_n(xn, 0, L), 144 + 16 / L[0]),
        ('su3_polyakov mu=3', lambda: ops.su3_polyakov_n(xn, 3, L), 144 + 16 / L[3]),
        ('su3_plaq_reduce (for scale)', lambda: ops.su3_plaq_sums_n(xn, L), 576),
        ('su3_plaq_planes (for scale)', lambda: ops.su3_plaq_planes_n(xn, L), 576),
    )
    print(f'lattice {L} x {nb} chains = {sites} chain-sites, {xn.numel() * 16 / 1e6:.0f} MB per field')
    for name, fn, bytes_per_site in rows:
        t = timeit(fn, args.iters)
        rate = bytes_per_site * sites / t
        print(f'{name:42s} {t * 1e3:8.3f} ms  {bytes_per_site:7.1f} B/site  {rate / 1e9:8.1f} GB/s  '
              f'{rate / HBM_PEAK:.3f} of 8 TB/s')
    x = lat.unpack(xn)
    t_k, w_k = wall(lambda: lat.wilson_loop_table(x, 4, 4), 3)
    print(f'wilson_loop_table(x, 4, 4), kernels (pack + 16 reductions + 15 extensions): {t_k * 1e3:9.2f} ms wall')
    t_n, _ = wall(lambda: lat.wilson_loop_sums_n(xn, 4, 4), 3)
    print(f'wilson_loop_sums_n(xn, 4, 4), the same without the pack:                  {t_n * 1e3:9.2f} ms wall')
    if not args.no_torch:
        t_t, w_t = wall(lambda: torch_loop_table(x, 4, 4), 2)
        print(f'the same table with torch.roll + matmul on the device:                 {t_t * 1e3:9.2f} ms wall '
              f'({t_t / t_k:.1f} x), max |difference| = {float((w_k - w_t).abs().max()):.2e}')


if __name__ == '__main__':
    main()
