#!/usr/bin/env python3
"""l2q_act_bwd_sums (activation VJP + bias column sums in one pass) against the three launches it replaces
for an un-pooled swish conv layer (copy of the cotangent, l2q_act_bwd in place, l2q_colsum), stand-alone,
HIP-event timing.  Default shape: the first activated un-pooled layer of the default conv stack at cfg-2
(2048 chains x 22 x 22 pixels, 16 channels)."""
import argparse, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'l2hmc-qcd_amd'))
from l2hmc import _ops as ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--M', type=int, default=2048 * 22 * 22)
ap.add_argument('--N', type=int, default=16)
ap.add_argument('--dtype', default='float32', choices=['float32', 'float64'])
ap.add_argument('--iters', type=int, default=50)
a = ap.parse_args()
dt = getattr(torch, a.dtype)
torch.manual_seed(0)
z = torch.randn(a.M, a.N, dtype=dt, device='cuda')
dy = torch.randn(a.M, a.N, dtype=dt, device='cuda')
db1, db2 = (torch.zeros(a.N, dtype=dt, device='cuda') for _ in range(2))


def three():
    d = ops.act_bwd(dy.clone(), z, 'swish', from_preact=True)
    ops.colsum_(db1, d)
    return d


def one():
    return ops.act_bwd_sums(dy, z, 'swish', db2, from_preact=True)


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.iters


assert torch.equal(three(), one())
for rep in range(3):
    t3, t1 = timed(three), timed(one)
    gb = 3 * a.M * a.N * z.element_size() / 1e9              # dy and z read, dz written
    print(f'[{a.M} x {a.N}] {a.dtype}: clone + act_bwd + colsum {t3:.1f} us, act_bwd_sums {t1:.1f} us '
          f'({gb / t1 * 1e6 / 1e3:.2f} TB/s of its {gb * 1e3:.0f} MB), ratio {t3 / t1:.2f}')
