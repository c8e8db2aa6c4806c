#!/usr/bin/env python3
"""Measurements of the Wilson fermions (csrc/su3_wilson.hip) for profiles/su3_wilson.md, SU(3) 8^4, complex128:
  --kernels     `l2q_su3_wilson_apply` with and without the fused norm at --nb chains (256) and each --nrhs (1 and 12) by
                HIP events: --repeats windows of --iters calls after a warm-up, median and spread, with the algorithmic
                bytes (spinor read once and written once; links counted once per chain and, beside it, once per system),
                the rate they give and its share of the HBM figure DESIGN.md uses; then the four launches of one CG
                iteration (two applies with norm, the update, the xpay) one by one and the iteration as a whole (with
                the per-system alpha / beta arithmetic in between), and a spinor field copy;
  --torch       the same operator composed from torch `roll` / `einsum` on the GPU at --torch-nb chains: the only
                "before" there is;
  --propagator  one 12-column `quark_propagator` at kappa = 0.10 on --physics-nb chains thermalised with `heatbath` at
                beta = 6 (nover = 3), with the pion correlator and its effective mass;
  --eo          even-odd preconditioning (csrc/su3_wilson_eo.hip, profiles/su3_wilson_eo.md) at each --nrhs: the half-lattice
                hop `l2q_su3_wilson_hop_eo` beside the full apply; one CGNR iteration on M beside one on Mhat (four hops,
                the update and the xpay on half fields); and the time to solution of `wilson_solve_n` / `wilson_solve_eo_n`
                and `wilson_solve_normal_n` / `wilson_solve_schur_normal_n` at --eo-kappa, --eo-tol on --nb chains
                thermalised with --eo-therm heatbath sweeps at beta = 6, Gaussian right-hand sides;
  --mixed       the mixed-precision even-odd solves (csrc/su3_wilson_f32.hip, profiles/su3_wilson_mixed.md) on the inputs of
                --eo: per launch the fp32 hop with and without aux + norm beside the fp64 hop of the same session, the fp32
                update / xpay, demote / promote and the link copy; one CGNR iteration on Mhat in fp32 beside fp64; and the
                time to solution, inner iterations and outer cycles of `wilson_solve_eo_mixed_n` and
                `wilson_solve_schur_normal_mixed_n` at each --inner-tol beside their fp64 siblings;
  --clover      the clover term (csrc/su3_wilson_clover.hip, profiles/su3_wilson_clover.md) at --c-sw (1.0) on the inputs
                of --eo: `clover_term` + `clover_invert`; the two hops of the clover Mhat beside the two of the plain Mhat
                on the same links, with the algorithmic bytes of both; the site-local apply; and the time to solution of
                `wilson_clover_solve_n` beside `wilson_solve_eo_n`."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'l2hmc-qcd_amd'))
from l2hmc import _ops as ops  # noqa: E402
from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3, effective_mass, pion_correlator  # noqa: E402

HBM_PEAK = 8.0e12       # B/s, the spec figure that DESIGN.md's fractions are taken against
SPINOR = 192            # bytes of one complex128 spinor (12 components)
LINKS = 4 * 144         # bytes of the four links of a site
FLOPS = 1320            # per (system, site) of one application


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


def show(name, ts, nbytes=None, sites=0, alt=None):
    t = statistics.median(ts)
    line = f'{name:44s} {t * 1e3:8.3f} ms (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f})'
    if nbytes is not None:
        rate = nbytes * sites / t
        line += f'  {nbytes:6.0f} B/site  {rate / 1e12:5.2f} TB/s  {rate / HBM_PEAK:.3f} of 8 TB/s'
        if alt is not None:
            line += f'  (links per system: {alt:.0f} B/site, {alt * sites / t / HBM_PEAK:.3f})'
        line += f'  {FLOPS * sites / t / 1e12:5.2f} Tflop/s' if alt is not None else ''
    print(line)
    return t


def kernels(nb, L, nrhs_list, iters, repeats):
    V = L[0] * L[1] * L[2] * L[3]
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    xn = ops.su3_project_su_n(torch.randn((nb, 4, 9, V), dtype=torch.complex128, device=dev))
    kappa = 0.10
    for nrhs in nrhs_list:
        psi = torch.randn((nb, nrhs, 12, V), dtype=torch.complex128, device=dev)
        out, q, z, x = (torch.empty_like(psi) for _ in range(4))
        r, p = torch.randn_like(psi), torch.randn_like(psi)
        part = torch.empty((nb, nrhs, ops.su3_wilson_norm_parts(L)), dtype=torch.float64, device=dev)
        rpart = torch.empty_like(part)
        coef = torch.full((nb, nrhs), 1e-3, dtype=torch.float64, device=dev)
        x.zero_()
        sites = nb * nrhs * V
        once, per_sys = 2 * SPINOR + LINKS / nrhs, 2 * SPINOR + LINKS
        print(f'lattice {L} x {nb} chains x {nrhs} right-hand sides: {psi.numel() * 16 / 1e6:.0f} MB per spinor field, '
              f'{xn.numel() * 16 / 1e6:.0f} MB of links, {iters} calls per window, {repeats} windows')
        show('apply', windows(lambda: ops.su3_wilson_apply_n(xn, psi, kappa, L, out=out), iters, repeats), once, sites, per_sys)
        show('apply, dagger', windows(lambda: ops.su3_wilson_apply_n(xn, psi, kappa, L, True, out=out), iters, repeats),
             once, sites, per_sys)
        ta = show('apply + fused norm', windows(lambda: ops.su3_wilson_apply_n(xn, psi, kappa, L, out=out, norm=part),
                                                iters, repeats), once, sites, per_sys)
        tu = show('cg_update (x, r, p, q; |r|^2)', windows(lambda: ops.su3_spinor_cg_update_(x, r, p, q, coef, rpart),
                                                         iters, repeats), 6 * SPINOR, sites)
        tx = show('xpay (p, z)', windows(lambda: ops.su3_spinor_xpay_(p, z, coef), iters, repeats), 3 * SPINOR, sites)
        show('spinor field copy (copy_)', windows(lambda: out.copy_(psi), iters, repeats), 2 * SPINOR, sites)
        show('sum_parts (tree over the partials)', windows(lambda: ops.sum_parts(part), iters, repeats))

        def iteration():
            ops.su3_wilson_apply_n(xn, p, kappa, L, False, out=q, norm=part)
            qq = ops.sum_parts(part)
            ops.su3_spinor_cg_update_(x, r, p, q, (coef / (qq + 1.0)).contiguous(), rpart)
            ops.su3_wilson_apply_n(xn, r, kappa, L, True, out=z, norm=part)
            zn = ops.sum_parts(part)
            ops.su3_spinor_xpay_(p, z, (coef / (zn + 1.0)).contiguous())

        ti = show('one CG iteration, as launched', windows(iteration, iters, repeats))
        print(f'  four launches by themselves: 2 x {ta * 1e3:.3f} + {tu * 1e3:.3f} + {tx * 1e3:.3f} = '
              f'{(2 * ta + tu + tx) * 1e3:.3f} ms; the rest of {ti * 1e3:.3f} ms is the per-system arithmetic between them')
        del psi, out, q, z, x, r, p


def even_odd(nb, L, nrhs_list, iters, repeats, therm, kappa, tol):
    V = L[0] * L[1] * L[2] * L[3]
    Vh = V // 2
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    lat = LatticeSU3(nb, L)
    xn = lat.pack(lat.heatbath(lat.random().to(dev), 6.0, nsweeps=therm, nover=3)[0])
    print(f'{L} x {nb} chains, beta 6.0 after {therm} heatbath sweeps (nover 3): plaquette '
          f'{float(lat.plaq_sums_n(xn)[:, 0].mean()) / (18.0 * V):.5f}; kappa {kappa}, tol {tol}')
    for nrhs in nrhs_list:
        psi = torch.randn((nb, nrhs, 12, V), dtype=torch.complex128, device=dev)
        out, q, z, x = (torch.empty_like(psi) for _ in range(4))
        r, p = torch.randn_like(psi), torch.randn_like(psi)
        part = torch.empty((nb, nrhs, ops.su3_wilson_norm_parts(L)), dtype=torch.float64, device=dev)
        rpart = torch.empty_like(part)
        coef = torch.full((nb, nrhs), 1e-3, dtype=torch.float64, device=dev)
        x.zero_()
        sites, hsites = nb * nrhs * V, nb * nrhs * Vh
        print(f'lattice {L} x {nb} chains x {nrhs} right-hand sides, {iters} calls per window, {repeats} windows')
        # the kernels: a full apply is V sites, a hop V/2; bytes per (system, site of the launch), links once per chain
        ta = show('full apply + fused norm', windows(lambda: ops.su3_wilson_apply_n(xn, psi, kappa, L, out=out, norm=part),
                                                     iters, repeats), 2 * SPINOR + LINKS / nrhs, sites, 2 * SPINOR + LINKS)
        he, ho, hq, hz, hx = (torch.empty((nb, nrhs, 12, Vh), dtype=torch.complex128, device=dev) for _ in range(5))
        hr, hp = torch.randn_like(he), torch.randn_like(he)
        he.copy_(hr)
        hx.zero_()
        hpart = torch.empty((nb, nrhs, -(-Vh // 256)), dtype=torch.float64, device=dev)
        hrpart = torch.empty_like(hpart)
        t1 = show('hop (a = 1, no aux), odd sites', windows(lambda: ops.su3_wilson_hop_eo_n(xn, he, L, 1, out=ho), iters, repeats),
                  2 * SPINOR + 2 * LINKS / nrhs, hsites, 2 * SPINOR + 2 * LINKS)
        t2 = show('hop (aux, fused norm), even sites',
                  windows(lambda: ops.su3_wilson_hop_eo_n(xn, ho, L, 0, a=-kappa * kappa, aux=he, b=1.0, out=hq, norm=hpart),
                          iters, repeats), 3 * SPINOR + 2 * LINKS / nrhs, hsites, 3 * SPINOR + 2 * LINKS)
        print(f'  Mhat = two hops {(t1 + t2) * 1e3:.3f} ms against M = one full apply {ta * 1e3:.3f} ms: ratio '
              f'{(t1 + t2) / ta:.2f}')
        tu = show('cg_update, full fields', windows(lambda: ops.su3_spinor_cg_update_(x, r, p, q, coef, rpart), iters, repeats),
                  6 * SPINOR, sites)
        tuh = show('cg_update, half fields', windows(lambda: ops.su3_spinor_cg_update_(hx, hr, hp, hq, coef, hrpart),
                                                     iters, repeats), 6 * SPINOR, hsites)
        tx = show('xpay, full fields', windows(lambda: ops.su3_spinor_xpay_(p, z, coef), iters, repeats), 3 * SPINOR, sites)
        txh = show('xpay, half fields', windows(lambda: ops.su3_spinor_xpay_(hp, hz, coef), iters, repeats), 3 * SPINOR, hsites)

        def iteration():
            ops.su3_wilson_apply_n(xn, p, kappa, L, False, out=q, norm=part)
            qq = ops.sum_parts(part)
            ops.su3_spinor_cg_update_(x, r, p, q, (coef / (qq + 1.0)).contiguous(), rpart)
            ops.su3_wilson_apply_n(xn, r, kappa, L, True, out=z, norm=part)
            zn = ops.sum_parts(part)
            ops.su3_spinor_xpay_(p, z, (coef / (zn + 1.0)).contiguous())

        def schur(src, dst, dagger):
            ops.su3_wilson_hop_eo_n(xn, src, L, 1, dagger, out=ho)
            ops.su3_wilson_hop_eo_n(xn, ho, L, 0, dagger, a=-kappa * kappa, aux=src, b=1.0, out=dst, norm=hpart)
            return ops.sum_parts(hpart)

        def iteration_eo():
            qq = schur(hp, hq, False)
            ops.su3_spinor_cg_update_(hx, hr, hp, hq, (coef / (qq + 1.0)).contiguous(), hrpart)
            zn = schur(hr, hz, True)
            ops.su3_spinor_xpay_(hp, hz, (coef / (zn + 1.0)).contiguous())

        ti = show('one CGNR iteration on M, as launched', windows(iteration, iters, repeats))
        te = show('one CGNR iteration on Mhat, as launched', windows(iteration_eo, iters, repeats))
        print(f'  launches by themselves: full 2 x {ta * 1e3:.3f} + {tu * 1e3:.3f} + {tx * 1e3:.3f} = '
              f'{(2 * ta + tu + tx) * 1e3:.3f} ms; even-odd 2 x {(t1 + t2) * 1e3:.3f} + {tuh * 1e3:.3f} + {txh * 1e3:.3f} = '
              f'{(2 * (t1 + t2) + tuh + txh) * 1e3:.3f} ms; iteration ratio even-odd / full {te / ti:.2f}')
        del out, q, z, x, r, p, he, ho, hq, hz, hx, hr, hp
        # time to solution: the same right-hand sides through both paths
        kw = dict(tol=tol, max_iter=2000)

        def timed(name, fn):
            fn()                                                    # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            info = res[-1]
            print(f'{name:44s} {dt * 1e3:9.1f} ms  iterations {int(info["iters"].min())} .. {int(info["iters"].max())}, '
                  f'residual <= {float(info["residual"].max()):.3g}, all converged {bool(info["converged"].all())}')
            return dt
        tf = timed('wilson_solve_n', lambda: lat.wilson_solve_n(xn, psi, kappa, **kw))
        to = timed('wilson_solve_eo_n', lambda: lat.wilson_solve_eo_n(xn, psi, kappa, **kw))
        print(f'  time to solution, even-odd / full: {to / tf:.2f}')
        pe = ops.su3_spinor_split_eo(psi, L)[0].contiguous()
        tf = timed('wilson_solve_normal_n', lambda: lat.wilson_solve_normal_n(xn, psi, kappa, **kw))
        to = timed('wilson_solve_schur_normal_n', lambda: lat.wilson_solve_schur_normal_n(xn, pe, kappa, **kw))
        print(f'  time to solution, even-odd / full: {to / tf:.2f}')
        del psi, pe


def mixed(nb, L, nrhs_list, iters, repeats, therm, kappa, tol, inner_tols):
    V = L[0] * L[1] * L[2] * L[3]
    Vh = V // 2
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    lat = LatticeSU3(nb, L)
    xn = lat.pack(lat.heatbath(lat.random().to(dev), 6.0, nsweeps=therm, nover=3)[0])
    print(f'{L} x {nb} chains, beta 6.0 after {therm} heatbath sweeps (nover 3): plaquette '
          f'{float(lat.plaq_sums_n(xn)[:, 0].mean()) / (18.0 * V):.5f}; kappa {kappa}, tol {tol}')
    x32 = ops.su3_links_demote_eo_n(xn, L)
    S32, L32 = SPINOR // 2, LINKS // 2
    show('link copy (fp64 in, fp32 parity-ordered out)', windows(lambda: ops.su3_links_demote_eo_n(xn, L, out=x32), iters, repeats),
         LINKS + L32, nb * V)
    for nrhs in nrhs_list:
        hsites = nb * nrhs * Vh
        print(f'lattice {L} x {nb} chains x {nrhs} right-hand sides, {iters} calls per window, {repeats} windows')
        c64, c128 = torch.complex64, torch.complex128
        he, ho, hq, hz, hx = (torch.empty((nb, nrhs, 12, Vh), dtype=c128, device=dev) for _ in range(5))
        hr, hp = torch.randn_like(he), torch.randn_like(he)
        he.copy_(hr)
        hx.zero_()
        fe, fo, fq, fz, fx = (torch.empty((nb, nrhs, 12, Vh), dtype=c64, device=dev) for _ in range(5))
        fr, fp = hr.to(c64), hp.to(c64)
        fe.copy_(fr)
        fx.zero_()
        hpart = torch.empty((nb, nrhs, -(-Vh // 256)), dtype=torch.float64, device=dev)
        hrpart = torch.empty_like(hpart)
        coef = torch.full((nb, nrhs), 1e-3, dtype=torch.float64, device=dev)
        # bytes per (system, half-site), the 8 links once per chain (beside it: once per system)
        t1 = show('fp64 hop (a = 1, no aux), odd sites', windows(lambda: ops.su3_wilson_hop_eo_n(xn, he, L, 1, out=ho), iters, repeats),
                  2 * SPINOR + 2 * LINKS / nrhs, hsites, 2 * SPINOR + 2 * LINKS)
        t2 = show('fp64 hop (aux, fused norm), even sites',
                  windows(lambda: ops.su3_wilson_hop_eo_n(xn, ho, L, 0, a=-kappa * kappa, aux=he, b=1.0, out=hq, norm=hpart),
                          iters, repeats), 3 * SPINOR + 2 * LINKS / nrhs, hsites, 3 * SPINOR + 2 * LINKS)
        f1 = show('fp32 hop (a = 1, no aux), odd sites', windows(lambda: ops.su3_wilson_hop_eo_f32_n(x32, fe, L, 1, out=fo), iters, repeats),
                  2 * S32 + 2 * L32 / nrhs, hsites, 2 * S32 + 2 * L32)
        f2 = show('fp32 hop (aux, fused norm), even sites',
                  windows(lambda: ops.su3_wilson_hop_eo_f32_n(x32, fo, L, 0, a=-kappa * kappa, aux=fe, b=1.0, out=fq, norm=hpart),
                          iters, repeats), 3 * S32 + 2 * L32 / nrhs, hsites, 3 * S32 + 2 * L32)
        print(f'  Mhat in fp32 {(f1 + f2) * 1e3:.3f} ms against fp64 {(t1 + t2) * 1e3:.3f} ms: ratio {(f1 + f2) / (t1 + t2):.2f}')
        tu = show('fp64 cg_update, half fields', windows(lambda: ops.su3_spinor_cg_update_(hx, hr, hp, hq, coef, hrpart), iters, repeats),
                  6 * SPINOR, hsites)
        fu = show('fp32 cg_update, half fields', windows(lambda: ops.su3_spinor_cg_update_f32_(fx, fr, fp, fq, coef, hrpart), iters, repeats),
                  6 * S32, hsites)
        tx = show('fp64 xpay, half fields', windows(lambda: ops.su3_spinor_xpay_(hp, hz, coef), iters, repeats), 3 * SPINOR, hsites)
        fxp = show('fp32 xpay, half fields', windows(lambda: ops.su3_spinor_xpay_f32_(fp, fz, coef), iters, repeats), 3 * S32, hsites)
        show('demote (fp64 in, fp32 out)', windows(lambda: ops.su3_spinor_demote(hr, coef, out=fz), iters, repeats), SPINOR + S32, hsites)
        show('promote_axpy (x64 += s e32)', windows(lambda: ops.su3_spinor_promote_axpy_(hx, fz, coef), iters, repeats),
             2 * SPINOR + S32, hsites)

        def schur(src, dst, dagger):
            ops.su3_wilson_hop_eo_n(xn, src, L, 1, dagger, out=ho)
            ops.su3_wilson_hop_eo_n(xn, ho, L, 0, dagger, a=-kappa * kappa, aux=src, b=1.0, out=dst, norm=hpart)
            return ops.sum_parts(hpart)

        def schur32(src, dst, dagger):
            ops.su3_wilson_hop_eo_f32_n(x32, src, L, 1, dagger, out=fo)
            ops.su3_wilson_hop_eo_f32_n(x32, fo, L, 0, dagger, a=-kappa * kappa, aux=src, b=1.0, out=dst, norm=hpart)
            return ops.sum_parts(hpart)

        def iteration_eo():
            qq = schur(hp, hq, False)
            ops.su3_spinor_cg_update_(hx, hr, hp, hq, (coef / (qq + 1.0)).contiguous(), hrpart)
            zn = schur(hr, hz, True)
            ops.su3_spinor_xpay_(hp, hz, (coef / (zn + 1.0)).contiguous())

        def iteration_f32():
            qq = schur32(fp, fq, False)
            ops.su3_spinor_cg_update_f32_(fx, fr, fp, fq, (coef / (qq + 1.0)).contiguous(), hrpart)
            zn = schur32(fr, fz, True)
            ops.su3_spinor_xpay_f32_(fp, fz, (coef / (zn + 1.0)).contiguous())

        te = show('one CGNR iteration on Mhat, fp64, as launched', windows(iteration_eo, iters, repeats))
        tf = show('one CGNR iteration on Mhat, fp32, as launched', windows(iteration_f32, iters, repeats))
        print(f'  launches by themselves: fp64 2 x {(t1 + t2) * 1e3:.3f} + {tu * 1e3:.3f} + {tx * 1e3:.3f} = '
              f'{(2 * (t1 + t2) + tu + tx) * 1e3:.3f} ms; fp32 2 x {(f1 + f2) * 1e3:.3f} + {fu * 1e3:.3f} + {fxp * 1e3:.3f} = '
              f'{(2 * (f1 + f2) + fu + fxp) * 1e3:.3f} ms; iteration ratio fp32 / fp64 {tf / te:.2f}')
        del he, ho, hq, hz, hx, hr, hp, fe, fo, fq, fz, fx, fr, fp
        psi = torch.randn((nb, nrhs, 12, V), dtype=c128, device=dev)
        pe = ops.su3_spinor_split_eo(psi, L)[0].contiguous()
        kw = dict(tol=tol, max_iter=2000)

        def timed(name, fn):
            fn()                                                    # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            info = res[-1]
            outer = f', outer cycles {int(info["outer"].min())} .. {int(info["outer"].max())}' if 'outer' in info else ''
            print(f'{name:52s} {dt * 1e3:9.1f} ms  iterations {int(info["iters"].min())} .. {int(info["iters"].max())}{outer}, '
                  f'residual <= {float(info["residual"].max()):.3g}, all converged {bool(info["converged"].all())}')
            return dt
        t64 = timed('wilson_solve_eo_n (fp64)', lambda: lat.wilson_solve_eo_n(xn, psi, kappa, **kw))
        for it in inner_tols:
            tm = timed(f'wilson_solve_eo_mixed_n inner_tol {it:g}', lambda: lat.wilson_solve_eo_mixed_n(xn, psi, kappa, inner_tol=it, **kw))
            print(f'  time to solution, mixed / fp64: {tm / t64:.2f}')
        t64 = timed('wilson_solve_schur_normal_n (fp64)', lambda: lat.wilson_solve_schur_normal_n(xn, pe, kappa, **kw))
        for it in inner_tols:
            tm = timed(f'wilson_solve_schur_normal_mixed_n inner_tol {it:g}',
                       lambda: lat.wilson_solve_schur_normal_mixed_n(xn, pe, kappa, inner_tol=it, **kw))
            print(f'  time to solution, mixed / fp64: {tm / t64:.2f}')
        del psi, pe


BLOCKS = 2 * 36 * 8     # bytes of the two Hermitian 6 x 6 blocks of a site


def clover(nb, L, nrhs_list, iters, repeats, therm, kappa, tol, c_sw):
    """--clover: the clover term (csrc/su3_wilson_clover.hip, profiles/su3_wilson_clover.md) on the inputs of --eo"""
    V = L[0] * L[1] * L[2] * L[3]
    Vh = V // 2
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    lat = LatticeSU3(nb, L)
    xn = lat.pack(lat.heatbath(lat.random().to(dev), 6.0, nsweeps=therm, nover=3)[0])
    print(f'{L} x {nb} chains, beta 6.0 after {therm} heatbath sweeps (nover 3): plaquette '
          f'{float(lat.plaq_sums_n(xn)[:, 0].mean()) / (18.0 * V):.5f}; kappa {kappa}, c_sw {c_sw}, tol {tol}')
    cl = ops.su3_clover_term_n(xn, kappa * c_sw, L)
    inv = torch.empty_like(cl)
    # once per configuration: per site 18 links of each of 6 planes come from cache, 576 B of links and 576 B of blocks are
    # compulsory; the inverse reads and writes 576 B per site
    tt = show('clover_term (A, both parities)', windows(lambda: ops.su3_clover_term_n(xn, kappa * c_sw, L, out=cl), iters, repeats),
              LINKS + BLOCKS, nb * V)
    tv = show('clover_invert (A^-1, pivots, log det)', windows(lambda: ops.su3_clover_invert_n(cl, L, out=inv), iters, repeats),
              2 * BLOCKS, nb * V)
    term = lat.clover_term_n(xn, kappa, c_sw)
    print(f'  clover_term + clover_invert {(tt + tv) * 1e3:.3f} ms per configuration batch; smallest pivot '
          f'{float(term.min_pivot.min()):.4f}, log det A_oo per chain {float(term.logdet[:, 1].mean()):.4f}')
    for nrhs in nrhs_list:
        hsites = nb * nrhs * Vh
        he, ho, hq = (torch.empty((nb, nrhs, 12, Vh), dtype=torch.complex128, device=dev) for _ in range(3))
        he.copy_(torch.randn_like(he))
        hpart = torch.empty((nb, nrhs, -(-Vh // 256)), dtype=torch.float64, device=dev)
        print(f'lattice {L} x {nb} chains x {nrhs} right-hand sides, {iters} calls per window, {repeats} windows')
        b1, b2 = 2 * SPINOR + 2 * LINKS / nrhs, 3 * SPINOR + 2 * LINKS / nrhs
        p1 = show('plain hop (a = 1, no aux), odd sites', windows(lambda: ops.su3_wilson_hop_eo_n(xn, he, L, 1, out=ho), iters, repeats),
                  b1, hsites)
        p2 = show('plain hop (aux, fused norm), even sites',
                  windows(lambda: ops.su3_wilson_hop_eo_n(xn, ho, L, 0, a=-kappa * kappa, aux=he, b=1.0, out=hq, norm=hpart),
                          iters, repeats), b2, hsites)
        z1 = show('clover hop, cmode 0 (the plain hop), odd sites',
                  windows(lambda: ops.su3_wilson_clover_hop_eo_n(xn, he, L, 1, None, 0, out=ho), iters, repeats), b1, hsites)
        c1 = show('clover hop, cmode 2 (A_oo^-1 on the result), odd sites',
                  windows(lambda: ops.su3_wilson_clover_hop_eo_n(xn, he, L, 1, term.ainv, 2, out=ho), iters, repeats),
                  b1 + BLOCKS / nrhs, hsites)
        c2 = show('clover hop, cmode 1 (A_ee on aux, fused norm), even sites',
                  windows(lambda: ops.su3_wilson_clover_hop_eo_n(xn, ho, L, 0, term.a, 1, a=-kappa * kappa, aux=he, b=1.0,
                                                                 out=hq, norm=hpart), iters, repeats), b2 + BLOCKS / nrhs, hsites)
        show('clover_apply (A_oo^-1 src), odd sites', windows(lambda: ops.su3_clover_apply_n(term.ainv, he, L, 1, out=ho),
                                                             iters, repeats), 2 * SPINOR + BLOCKS / nrhs, hsites)
        plain_b, clover_b = b1 + b2, b1 + b2 + 2 * BLOCKS / nrhs
        print(f'  clover Mhat {(c1 + c2) * 1e3:.3f} ms against the plain Mhat {(p1 + p2) * 1e3:.3f} ms: time ratio '
              f'{(c1 + c2) / (p1 + p2):.3f}; algorithmic bytes per (system, even site) {clover_b:.0f} against {plain_b:.0f}: '
              f'byte ratio {clover_b / plain_b:.3f}; cmode 0 against the plain hop {z1 / p1:.3f}')
        del he, ho, hq
        psi = torch.randn((nb, nrhs, 12, V), dtype=torch.complex128, device=dev)
        kw = dict(tol=tol, max_iter=2000)

        def timed(name, fn):
            fn()                                                    # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            info = res[-1]
            print(f'{name:44s} {dt * 1e3:9.1f} ms  iterations {int(info["iters"].min())} .. {int(info["iters"].max())}, '
                  f'residual <= {float(info["residual"].max()):.3g}, all converged {bool(info["converged"].all())}')
            return dt
        tp = timed('wilson_solve_eo_n', lambda: lat.wilson_solve_eo_n(xn, psi, kappa, **kw))
        tc = timed('wilson_clover_solve_n (prebuilt term)', lambda: lat.wilson_clover_solve_n(xn, psi, kappa, c_sw, clover=term, **kw))
        tb = timed('wilson_clover_solve_n (builds the term)', lambda: lat.wilson_clover_solve_n(xn, psi, kappa, c_sw, **kw))
        print(f'  time to solution, clover / plain even-odd: {tc / tp:.2f} (building the term included: {tb / tp:.2f})')
        del psi


def torch_apply(x, psi, kappa, gam):
    """M psi from roll / einsum on reference-layout tensors (antiperiodic in t)"""
    eye = torch.eye(4, dtype=psi.dtype, device=psi.device)
    acc = torch.zeros_like(psi)
    for mu in range(4):
        f = torch.roll(psi, -1, 2 + mu)
        w = torch.roll(torch.einsum('btxyzji,brtxyzaj->brtxyzai', x[:, mu].conj(), psi), 1, 2 + mu)
        if mu == 0:
            f[:, :, -1] *= -1
            w[:, :, 0] *= -1
        acc += torch.einsum('ad,brtxyzdc->brtxyzac', eye - gam[mu], torch.einsum('btxyzij,brtxyzaj->brtxyzai', x[:, mu], f))
        acc += torch.einsum('ad,brtxyzdc->brtxyzac', eye + gam[mu], w)
    return psi - kappa * acc


def torch_compose(nb, L, nrhs_list, iters, repeats):
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    lat = LatticeSU3(nb, L)
    V = lat.volume
    x = lat.unpack(ops.su3_project_su_n(torch.randn((nb, 4, 9, V), dtype=torch.complex128, device=dev)))
    gam = LatticeSU3.gamma_matrices().to(dev)
    for nrhs in nrhs_list:
        psi = torch.randn((nb, nrhs, *L, 4, 3), dtype=torch.complex128, device=dev)
        d = float((torch_apply(x, psi, 0.1, gam) - lat.wilson_dirac(x, psi, 0.1)).abs().max())
        print(f'lattice {L} x {nb} chains x {nrhs} right-hand sides, |torch - kernel| = {d:.3g}')
        tt = show('torch roll / einsum', windows(lambda: torch_apply(x, psi, 0.1, gam), iters, repeats))
        pn = ops.su3_spinor_pack(psi)
        out = torch.empty_like(pn)
        xn = lat.pack(x)
        tk = show('l2q_su3_wilson_apply', windows(lambda: ops.su3_wilson_apply_n(xn, pn, 0.1, L, out=out), iters, repeats))
        print(f'  ratio {tt / tk:.1f}')


def propagator(nb, L, therm, kappa):
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    lat = LatticeSU3(nb, L)
    x = lat.heatbath(lat.random().to(dev), 6.0, nsweeps=therm, nover=3)[0]
    print(f'{L} x {nb} chains, beta 6.0 after {therm} heatbath sweeps (nover 3): plaquette '
          f'{float(lat.plaqs(x).mean()):.5f}')
    for name, links in (('thin links', x), ('one HYP step', lat.hyp_smear(x))):
        lat.quark_propagator(links, kappa)                      # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S, info = lat.quark_propagator(links, kappa)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        C = pion_correlator(S)
        print(f'{name}: kappa {kappa}: {dt * 1e3:.1f} ms for {nb} x 12 systems, iterations {int(info["iters"].min())} .. '
              f'{int(info["iters"].max())}, residual <= {float(info["residual"].max()):.3g}, all converged '
              f'{bool(info["converged"].all())}')
        print('  C(t)     = ' + ' '.join(f'{float(v):.4e}' for v in C.mean(0)))
        print('  m_eff(t) = ' + ' '.join(f'{float(v):.4f}' for v in effective_mass(C.mean(0))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nb', type=int, default=256)
    ap.add_argument('--L', type=int, nargs=4, default=[8, 8, 8, 8])
    ap.add_argument('--nrhs', type=int, nargs='+', default=[1, 12])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--torch', action='store_true')
    ap.add_argument('--torch-nb', type=int, default=32)
    ap.add_argument('--propagator', action='store_true')
    ap.add_argument('--physics-nb', type=int, default=16)
    ap.add_argument('--therm', type=int, default=50)
    ap.add_argument('--kappa', type=float, default=0.10)
    ap.add_argument('--eo', action='store_true')
    ap.add_argument('--eo-kappa', type=float, default=0.12)
    ap.add_argument('--eo-tol', type=float, default=1e-10)
    ap.add_argument('--eo-therm', type=int, default=10)
    ap.add_argument('--mixed', action='store_true')
    ap.add_argument('--inner-tol', type=float, nargs='+', default=[1e-3, 1e-4, 1e-5, 1e-6])
    ap.add_argument('--clover', action='store_true')
    ap.add_argument('--c-sw', type=float, default=1.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    torch.set_default_dtype(torch.float64)
    if args.kernels:
        kernels(args.nb, args.L, args.nrhs, args.iters, args.repeats)
    if args.torch:
        torch_compose(args.torch_nb, args.L, args.nrhs, max(2, args.iters // 4), args.repeats)
    if args.eo:
        even_odd(args.nb, args.L, args.nrhs, args.iters, args.repeats, args.eo_therm, args.eo_kappa, args.eo_tol)
    if args.mixed:
        mixed(args.nb, args.L, args.nrhs, args.iters, args.repeats, args.eo_therm, args.eo_kappa, args.eo_tol, args.inner_tol)
    if args.clover:
        clover(args.nb, args.L, args.nrhs, args.iters, args.repeats, args.eo_therm, args.eo_kappa, args.eo_tol, args.c_sw)
    if args.propagator:
        propagator(args.physics_nb, args.L, args.therm, args.kappa)


if __name__ == '__main__':
    main()
