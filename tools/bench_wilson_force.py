#!/usr/bin/env python3
"""Measurements of the pseudofermion force (csrc/su3_wilson_force.hip) and of the trajectory with dynamical Wilson quarks
for profiles/su3_wilson_force.md, SU(3) 8^4, complex128:
  --kernels     `l2q_su3_wilson_force` at --nb chains (256) and each --npf (1 and 2), as the force (no f_in) and as the
                in-place kick, by HIP events: --repeats windows of --iters calls after a warm-up, median and spread, with
                the algorithmic bytes per (chain, site) (links 576 B, output 576 B, + 576 B of f_in, npf x 384 B of
                spinors), the rate they give and its share of the HBM figure DESIGN.md uses; and, from the same run, one
                `l2q_su3_wilson_apply` (nrhs = 1), one `l2q_su3_force` and one `l2q_su3_force_kick` as yardsticks;
  --trajectory  on --physics-nb chains thermalised with `heatbath` at beta = 6 (nover = 3, what `Trainer.thermalize`
                runs): one leapfrog of `WilsonHMC` stage by stage (each stage between device synchronisations: solves,
                fermion force, gauge kick, link update), then --ntraj trajectories: acceptance, CG iterations per solve,
                <exp(-dH)> with its standard error; with --even-odd the same split and trajectories again with
                `WilsonHMCEvenOdd` on the same thermalised links (profiles/su3_wilson_eo.md): its 'solves' stage is the
                solve on the Schur complement plus the two hops and merges that complete X and Y; with --mixed the
                even-odd run and then `WilsonHMCMixed` (every solve by fp32 inner CG and fp64 defect correction,
                profiles/su3_wilson_mixed.md; --inner-tol) on the same links, from the same seed.
With --c-sw (profiles/su3_clover_force.md; --kappa 0.12 there):
  --kernels     `l2q_su3_clover_force` on --nb chains thermalised with --clover-therm heatbath sweeps at beta = 6: the
                entry (both kernels) with both terms at each --npf, as force and as kick in place, the determinant term
                alone, and -- alternating window by window on the same links -- `l2q_su3_clover_bwd`, whose second pass
                is the same gather; with the algorithmic bytes of the two kernels and the time the G kernel's bytes take
                at the HBM figure.  Per-kernel times come from `rocprofv3 --kernel-trace --stats` on --profile-loop;
  --profile-loop  nothing but --iters alternating calls of the two entries (npf = --npf[0]), for the profiler;
  --trajectory  `WilsonHMCEvenOdd`, then `WilsonCloverHMC` at --c-sw on the same thermalised links, from the same seed;
                the stage split has two more stages: the clover term with its inverse, and the clover force."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'l2hmc-qcd_amd'))
from l2hmc import _ops as ops  # noqa: E402
from l2hmc.dynamics.pytorch.fermion_hmc import WilsonCloverHMC, WilsonHMC, WilsonHMCEvenOdd, WilsonHMCMixed  # noqa: E402
from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3  # noqa: E402

HBM_PEAK = 8.0e12       # B/s, the spec figure that DESIGN.md's fractions are taken against
SPINOR = 192            # bytes of one complex128 spinor (12 components)
LINKS = 4 * 144         # bytes of the four links of a site


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
    print(f'{name:40s} {t * 1e3:8.3f} ms (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f})  {nbytes:6.0f} B/site  '
          f'{rate / 1e12:5.2f} TB/s  {rate / HBM_PEAK:.3f} of 8 TB/s')
    return t


def kernels(nb, L, npf_list, iters, repeats):
    V = L[0] * L[1] * L[2] * L[3]
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    xn = ops.su3_project_su_n(torch.randn((nb, 4, 9, V), dtype=torch.complex128, device=dev))
    vn = ops.su3_assemble_tah_n(torch.randn((8, nb, 4, V), dtype=torch.float64, device=dev))
    f = torch.empty_like(xn)
    kappa, sites = 0.10, nb * V
    print(f'lattice {L} x {nb} chains: {xn.numel() * 16 / 1e6:.0f} MB of links, {iters} calls per window, {repeats} windows')
    for npf in npf_list:
        X = torch.randn((nb, npf, 12, V), dtype=torch.complex128, device=dev)
        Y = torch.randn_like(X)
        show(f'wilson_force npf {npf}', windows(lambda: ops.su3_wilson_force_n(xn, X, Y, kappa, L, out=f), iters, repeats),
             2 * LINKS + npf * 2 * SPINOR, sites)
        show(f'wilson_force npf {npf}, kick in place',
             windows(lambda: ops.su3_wilson_force_n(xn, X, Y, kappa, L, coef=-1e-6, f_in=vn, out=vn), iters, repeats),
             3 * LINKS + npf * 2 * SPINOR, sites)
        del X, Y
    psi = torch.randn((nb, 1, 12, V), dtype=torch.complex128, device=dev)
    out = torch.empty_like(psi)
    show('wilson_apply nrhs 1', windows(lambda: ops.su3_wilson_apply_n(xn, psi, kappa, L, out=out), iters, repeats),
         2 * SPINOR + LINKS, sites)
    show('su3_force (gauge)', windows(lambda: ops.su3_force_n(xn, 6.0, L), iters, repeats), 2 * LINKS, sites)
    show('su3_force_kick (gauge, in place)', windows(lambda: ops.su3_force_kick_n(xn, 6.0, -1e-6, vn, L), iters, repeats),
         3 * LINKS, sites)


def clover_setup(nb, L, therm, kappa, c_sw):
    """(lattice, thermalised native links, their clover term, a momentum) of the --c-sw kernel measurements"""
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    lat = LatticeSU3(nb, L)
    xn = lat.pack(lat.heatbath(lat.random().to(dev), 6.0, nsweeps=therm, nover=3)[0])
    term = lat.clover_term_n(xn, kappa, c_sw)
    vn = ops.su3_assemble_tah_n(torch.randn((8, nb, 4, lat.volume), dtype=torch.float64, device=dev))
    print(f'{L} x {nb} chains, beta 6.0 after {therm} heatbath sweeps (nover 3): plaquette '
          f'{float(lat.plaq_sums_n(xn)[:, 0].mean()) / (18.0 * lat.volume):.5f}; kappa {kappa}, c_sw {c_sw}, smallest pivot '
          f'{float(term.min_pivot.min()):.3f}')
    return lat, xn, term, vn


def clover_kernels(nb, L, npf_list, iters, repeats, therm, kappa, c_sw):
    lat, xn, term, vn = clover_setup(nb, L, therm, kappa, c_sw)
    V, sites, kc = lat.volume, nb * lat.volume, kappa * c_sw
    f = torch.empty_like(xn)
    G, BLOCKS = 54 * 8, 2 * 36 * 8 / 2              # bytes of G per site; of the two blocks of A^-1, odd sites only
    link_bytes = LINKS + G + LINKS                   # the link kernel: links and G read once, the force written
    w3 = torch.tensor([[0.3, -0.2, 0.0]], dtype=torch.float64, device=xn.device).repeat(nb, 1)
    gx = torch.zeros_like(xn)
    for npf in npf_list:
        X = torch.randn((nb, npf, 12, V), dtype=torch.complex128, device=xn.device)
        Y = torch.randn_like(X)
        g_bytes = npf * 2 * SPINOR + BLOCKS + G
        print(f'npf {npf}: G kernel {g_bytes:.0f} B/site = {g_bytes * sites / HBM_PEAK * 1e3:.3f} ms at 8 TB/s; link kernel '
              f'{link_bytes} B/site (+ {LINKS} of f_in) = {link_bytes * sites / HBM_PEAK * 1e3:.3f} ms')
        show(f'clover_force npf {npf} (both kernels)',
             windows(lambda: ops.su3_clover_force_n(xn, X, Y, term.ainv, kc, L, det_weight=npf, out=f), iters, repeats),
             g_bytes + link_bytes, sites)
        show(f'clover_force npf {npf}, kick in place',
             windows(lambda: ops.su3_clover_force_n(xn, X, Y, term.ainv, kc, L, det_weight=npf, coef=-1e-6, f_in=vn, out=vn),
                     iters, repeats), g_bytes + link_bytes + LINKS, sites)
        show(f'wilson_force npf {npf}, kick in place (the hop part)',
             windows(lambda: ops.su3_wilson_force_n(xn, X, Y, kappa, L, coef=-1e-6, f_in=vn, out=vn), iters, repeats),
             3 * LINKS + npf * 2 * SPINOR, sites)
        del X, Y
    show('clover_force, determinant term alone', windows(lambda: ops.su3_clover_force_n(xn, None, None, term.ainv, kc, L,
                                                                                        det_weight=1.0, out=f), iters, repeats),
         BLOCKS + G + link_bytes, sites)
    # the two entries window by window on the same links: the second kernel of either is the same gather
    X = torch.randn((nb, npf_list[0], 12, V), dtype=torch.complex128, device=xn.device)
    Y = torch.randn_like(X)
    fa, fb = [], []
    for _ in range(repeats):
        fa += windows(lambda: ops.su3_clover_force_n(xn, X, Y, term.ainv, kc, L, det_weight=1.0, out=f), iters, 1, warm=1)
        fb += windows(lambda: ops.su3_clover_bwd_(gx, xn, w3, L), iters, 1, warm=1)
    show(f'alternating: clover_force npf {npf_list[0]} (both kernels)', fa, npf_list[0] * 2 * SPINOR + BLOCKS + G + link_bytes, sites)
    show('alternating: clover_bwd (both kernels)', fb, 2 * LINKS + G + G + LINKS, sites)


def profile_loop(nb, L, npf, iters, therm, kappa, c_sw):
    lat, xn, term, vn = clover_setup(nb, L, therm, kappa, c_sw)
    X = torch.randn((nb, npf, 12, lat.volume), dtype=torch.complex128, device=xn.device)
    Y = torch.randn_like(X)
    w3 = torch.tensor([[0.3, -0.2, 0.0]], dtype=torch.float64, device=xn.device).repeat(nb, 1)
    f, gx = torch.empty_like(xn), torch.zeros_like(xn)
    for _ in range(iters):
        ops.su3_clover_force_n(xn, X, Y, term.ainv, kappa * c_sw, L, det_weight=npf, out=f)
        ops.su3_clover_bwd_(gx, xn, w3, L)
    torch.cuda.synchronize()


def trajectory(nb, L, therm, beta, kappa, eps, nleapfrog, npf, ntraj, even_odd=False, mixed=False, inner_tol=None,
               c_sw=None):
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    lat = LatticeSU3(nb, L)
    x = lat.heatbath(lat.random().to(dev), beta, nsweeps=therm, nover=3)[0]
    print(f'{L} x {nb} chains, beta {beta} after {therm} heatbath sweeps (nover 3): plaquette '
          f'{float(lat.plaqs(x).mean()):.5f}; kappa {kappa}, npf {npf}, eps {eps}, nleapfrog {nleapfrog}, '
          f'even_odd {even_odd}, mixed {mixed}' + (f', inner_tol {inner_tol}' if mixed and inner_tol else ''))
    if c_sw is not None:
        print(f'c_sw {c_sw}')
        hmc = WilsonCloverHMC(lat, beta, kappa, c_sw, eps, nleapfrog, npf=npf)
    elif mixed:
        hmc = WilsonHMCMixed(lat, beta, kappa, eps, nleapfrog, npf=npf, inner_tol=inner_tol)
    else:
        hmc = (WilsonHMCEvenOdd if even_odd else WilsonHMC)(lat, beta, kappa, eps, nleapfrog, npf=npf)
    xn = lat.pack(x)
    hmc.trajectory_n(xn)                                         # warm-up
    # one leapfrog stage by stage
    spent = {'solves': 0.0, 'fermion force': 0.0, 'gauge kick': 0.0, 'link update': 0.0}
    if c_sw is not None:
        spent.update({'clover term': 0.0, 'clover force': 0.0})
    iters = []

    def timed(key, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        spent[key] += time.perf_counter() - t0
        return r

    def kick(xn, vn, step):
        timed('gauge kick', lambda: ops.su3_force_kick_n(xn, beta, -step, vn, L))
        if c_sw is not None:
            cl = timed('clover term', lambda: hmc._clover(xn))
            X, Y, info = timed('solves', lambda: lat._clover_force_fields_n(xn, phin, kappa, c_sw, cl,
                                                                            **hmc._solve_kw(hmc.tol_md)))
            timed('fermion force', lambda: ops.su3_wilson_force_n(xn, X, Y, kappa, L, True, coef=-step, f_in=vn, out=vn))
            timed('clover force', lambda: ops.su3_clover_force_n(xn, X, Y, cl.ainv, kappa * c_sw, L, det_weight=npf,
                                                                 coef=-step, f_in=vn, out=vn))
            iters.append(info['iters'])
            return
        X, Y, info = timed('solves', lambda: lat._force_fields_n('pseudofermion_force', xn, phin, kappa, even_odd,
                                                                 **hmc._solve_kw(hmc.tol_md)))
        timed('fermion force', lambda: ops.su3_wilson_force_n(xn, X, Y, kappa, L, True, coef=-step, f_in=vn, out=vn))
        iters.append(info['iters'])

    vn = ops.su3_assemble_tah_n(torch.randn((8, nb, 4, lat.volume), dtype=torch.float64, device=dev))
    phin, _ = hmc._refresh_n(xn, None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kick(xn, vn, 0.5 * eps)
    x1 = xn
    for k in range(nleapfrog):
        x1 = timed('link update', lambda: ops.su3_expm_mul_n(x1, vn, eps))
        kick(x1, vn, (1.0 if k + 1 < nleapfrog else 0.5) * eps)
    total = time.perf_counter() - t0
    it = torch.stack(iters).to(torch.float64)
    print(f'one leapfrog ({nleapfrog + 1} kicks, {nleapfrog} link updates): {total * 1e3:.1f} ms wall; '
          + ', '.join(f'{k} {v * 1e3:.1f} ms' for k, v in spent.items())
          + f'; CG iterations per solve: mean {float(it.mean()):.1f}, max {int(it.max())}')
    # whole trajectories
    dh, acc, walls = [], [], []
    for _ in range(ntraj):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xn, m = hmc.trajectory_n(xn)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        dh.append(m['dH'])
        acc.append(m['acc_mask'].to(torch.float64))
        print(f'  trajectory: {walls[-1] * 1e3:.1f} ms, acc {float(acc[-1].mean()):.2f}, <dH> {float(m["dH"].mean()):+.4f}, '
              f'plaq {float(m["plaq"].mean()):.5f}, cg md {m["cg_iters_md"]}, cg H {m["cg_iters_h"]}, unconverged '
              f'{m["unconverged"]}')
    e = torch.exp(-torch.stack(dh)).flatten()
    print(f'{ntraj} trajectories x {nb} chains: acceptance {float(torch.stack(acc).mean()):.3f}, <exp(-dH)> = '
          f'{float(e.mean()):.4f} +- {float(e.std() / e.numel() ** 0.5):.4f}, median wall {statistics.median(walls) * 1e3:.1f} ms')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nb', type=int, default=256)
    ap.add_argument('--L', type=int, nargs=4, default=[8, 8, 8, 8])
    ap.add_argument('--npf', type=int, nargs='+', default=[1, 2])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--trajectory', action='store_true')
    ap.add_argument('--physics-nb', type=int, default=16)
    ap.add_argument('--therm', type=int, default=50)
    ap.add_argument('--beta', type=float, default=6.0)
    ap.add_argument('--kappa', type=float, default=0.10)
    ap.add_argument('--eps', type=float, default=0.02)
    ap.add_argument('--nleapfrog', type=int, default=25)
    ap.add_argument('--ntraj', type=int, default=10)
    ap.add_argument('--even-odd', action='store_true')
    ap.add_argument('--mixed', action='store_true')
    ap.add_argument('--inner-tol', type=float, default=None)
    ap.add_argument('--c-sw', type=float, default=None)
    ap.add_argument('--clover-therm', type=int, default=10)
    ap.add_argument('--profile-loop', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    torch.set_default_dtype(torch.float64)
    if args.profile_loop:
        profile_loop(args.nb, args.L, args.npf[0], args.iters, args.clover_therm, args.kappa, args.c_sw)
        return
    if args.kernels and args.c_sw is not None:
        clover_kernels(args.nb, args.L, args.npf, args.iters, args.repeats, args.clover_therm, args.kappa, args.c_sw)
    elif args.kernels:
        kernels(args.nb, args.L, args.npf, args.iters, args.repeats)
    if args.trajectory:
        modes = [(True, False), (True, True)] if args.mixed else [(False, False), (True, False)] if args.even_odd \
            else [(False, False)]
        if args.c_sw is not None:
            modes = [(True, False)]
        for eo, mixed in modes:
            trajectory(args.physics_nb, args.L, args.therm, args.beta, args.kappa, args.eps, args.nleapfrog, args.npf[0],
                       args.ntraj, eo, mixed, args.inner_tol)
        if args.c_sw is not None:
            trajectory(args.physics_nb, args.L, args.therm, args.beta, args.kappa, args.eps, args.nleapfrog, args.npf[0],
                       args.ntraj, True, False, None, args.c_sw)


if __name__ == '__main__':
    main()
