#!/usr/bin/env python3
"""Micro-benchmark of the individual HIP kernels at the BASELINE cfg-4 size
(SU(3) 8^4, 256 chains, fp64).  Prints achieved algorithmic GB/s."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'l2hmc-qcd_amd'))
from l2hmc import _ops as ops, native  # noqa: E402


def timeit(fn, iters=10, warm=3):
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


def torch_clover_sums(x):
    """The clover sums of l2q_su3_clover_reduce written with torch ops on the reference layout
    x[nb, 4, T, X, Y, Z, 3, 3] (roll + matmul: what a user without the kernel would write) -- the baseline of
    the `su3_clover_reduce` row under --torch-clover."""
    def sh(f, mu, n=1):
        return torch.roll(f, -n, dims=mu + 1)

    def adj(m):
        return m.conj().transpose(-1, -2)

    def tr(m):
        return m.diagonal(dim1=-2, dim2=-1).sum(-1)

    def field(mu, nu):
        um, un = x[:, mu], x[:, nu]
        um_m, un_n = sh(um, mu, -1), sh(un, nu, -1)
        l1 = um @ sh(un, mu) @ adj(sh(um, nu)) @ adj(un)
        q = l1 + un @ adj(sh(um_m, nu)) @ adj(sh(un, mu, -1)) @ um_m
        q = q + adj(um_m) @ adj(sh(sh(un, mu, -1), nu, -1)) @ sh(um_m, nu, -1) @ un_n
        q = q + adj(un_n) @ sh(um, nu, -1) @ sh(sh(un, mu), nu, -1) @ adj(um)
        a = 0.5 * (q - adj(q))
        a = a - (tr(a) / 3.0)[..., None, None] * torch.eye(3, dtype=x.dtype, device=x.device)
        return 0.25 * a, tr(l1).real
    nb = x.shape[0]
    e = q = p = 0.0
    for k, (a, b), sign in ((1, (2, 3), 1.0), (2, (1, 3), -1.0), (3, (1, 2), 1.0)):
        f, p1 = field(0, k)
        g, p2 = field(a, b)
        e = e - tr(f @ f).real.reshape(nb, -1).sum(-1) - tr(g @ g).real.reshape(nb, -1).sum(-1)
        q = q - sign * tr(f @ g).real.reshape(nb, -1).sum(-1)
        p = p + p1.reshape(nb, -1).sum(-1) + p2.reshape(nb, -1).sum(-1)
    return torch.stack([e, q, p], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--torch-clover', action='store_true',
                    help='also time the clover sums written with torch roll / matmul and compare the outputs')
    ap.add_argument('--flow-only', action='store_true', help='only the Wilson-flow / clover rows')
    ap.add_argument('--clover-bwd', action='store_true',
                    help='only the clover VJP next to the clover sums and the plaquette VJP')
    ap.add_argument('--flow-bwd', action='store_true',
                    help='only the reverse sweep of the Wilson flow next to its forward and the clover VJP')
    ap.add_argument('--nb', type=int, default=256)
    ap.add_argument('--L', type=int, nargs=4, default=[8, 8, 8, 8])
    ap.add_argument('--gemm', action='store_true')
    a = ap.parse_args()
    L, nb = tuple(a.L), a.nb
    V = L[0] * L[1] * L[2] * L[3]
    dev = 'cuda'
    torch.manual_seed(0)
    xn = torch.randn(nb, 4, 9, V, dtype=torch.complex128, device=dev)
    xn = ops.su3_project_su_n(xn)
    vn = ops.su3_assemble_tah_n(torch.randn(8, nb, 4, V, dtype=torch.float64, device=dev))
    sites = nb * V
    mask = (torch.rand(36 * V, device=dev) > 0.5).float()
    stq = [0.01 * torch.randn(nb, 36 * V, dtype=torch.float64, device=dev) for _ in range(3)]
    rows = []

    def rec(name, t, bytes_per_site, flop_per_site=0):
        gbs = sites * bytes_per_site / t / 1e9
        tf = sites * flop_per_site / t / 1e12
        rows.append((name, t * 1e3, gbs, tf))
        print(f'{name:34s} {t*1e3:8.3f} ms  {gbs:8.1f} GB/s  ({gbs/8000*100:5.1f}% of 8 TB/s)'
              + (f'  {tf:6.2f} TFLOP/s' if flop_per_site else ''), flush=True)

    if a.clover_bwd:
        # the clover VJP: pass 1 reads the links and writes 54 reals per site (576 + 432 B, 72 products), pass 2 reads
        # links and those (576 + 432 B) and updates gx (1152 B), 4 links x 6 loops x 8 products; the plaquette VJP
        # reads the links and updates gx (4 links x 6 staples x 2 products)
        gx = torch.zeros_like(xn)
        w3 = torch.randn(nb, 3, dtype=torch.float64, device=dev)
        w6 = torch.randn(nb, 6, 2, dtype=torch.float64, device=dev)
        rec('su3_clover_reduce', timeit(lambda: ops.su3_clover_sums_n(xn, L)), 576, 72 * 216)
        rec('su3_plaq_bwd', timeit(lambda: ops.su3_plaq_bwd_(gx, xn, w6, L)), 1728, 48 * 216)
        rec('su3_clover_bwd', timeit(lambda: ops.su3_clover_bwd_(gx, xn, w3, L)), 3168, 264 * 216)
        return
    if a.flow_bwd:
        # the full force VJP reads the links and the force's cotangent and updates gx (576 + 576 + 1152 B): 4 links x
        # 3 directions x (7 + 6) products.  A flow step is three stages (force kick + exponential); its reverse
        # recomputes them (without the last exponential) and reverses each with an expm_mul_bwd and a force VJP.
        gx, gf = torch.zeros_like(xn), torch.randn_like(xn)
        w3 = torch.randn(nb, 3, dtype=torch.float64, device=dev)
        rec('su3_clover_bwd', timeit(lambda: ops.su3_clover_bwd_(gx, xn, w3, L)), 3168, 264 * 216)
        rec('su3_force_bwd (staples const)', timeit(lambda: ops.su3_force_bwd_(gx, xn, gf, 3.0, L)), 2304)
        rec('su3_force_vjp', timeit(lambda: ops.su3_force_vjp_(gx, xn, gf, 3.0, L)), 2304, 156 * 216)
        p2, x2, x3 = torch.empty_like(xn), torch.empty_like(xn), torch.empty_like(xn)
        rec('su3_flow_step (3 stages)', timeit(lambda: ops.su3_flow_step_n(xn, x2, p2, x3, 0.01, L)), 2880 + 2 * 3456)
        gp = torch.zeros_like(xn)
        rec('su3_flow_stage_bwd', timeit(lambda: ops.su3_flow_stage_bwd_n(xn, vn, -32.0 / 17.0, 17.0 / 36.0 * 0.01, gf,
                                                                         gp, L)), 5760)
        del p2, x3, gp
        ws = torch.empty(int(native.load().l2q_su3_flow_step_bwd_ws_bytes(nb, *L)), dtype=torch.uint8, device=dev)
        rec('su3_flow_step_bwd', timeit(lambda: ops.su3_flow_step_bwd_n(xn, 0.01, gf, L, gx_in=x2, ws=ws)), 0)
        return
    # Wilson flow / clover observables: the clover pass reads the links once (576 B / site, 72 3x3 products); a flow
    # stage is the force kick (reads X and P, writes P) and the x-update (reads P and X, writes X): 3456 B / site
    rec('su3_clover_reduce', timeit(lambda: ops.su3_clover_sums_n(xn, L)), 576, 72 * 216)
    if a.torch_clover:
        xr = ops.su3_unpack(xn, L)
        t = timeit(lambda: torch_clover_sums(xr), iters=3, warm=1)
        got, want = ops.su3_clover_sums_n(xn, L), torch_clover_sums(xr)
        rel = float(((got - want).abs() / want.abs().clamp(min=float(V))).max())
        rec('  torch roll/matmul clover', t, 576, 72 * 216)
        print(f'{"  kernel vs torch clover":34s} max |d| / max(|sum|, V) = {rel:.2e}', flush=True)
        del xr, want
    p2, x2 = torch.empty_like(xn), torch.empty_like(xn)
    cc, ss = -32.0 / 17.0, 17.0 / 36.0 * 0.01
    rec('su3_flow_stage', timeit(lambda: ops.su3_flow_stage_n(xn, vn, cc, ss, L, p_out=p2, x_out=x2)), 3456)

    def two_launch():
        ops.su3_force_kick_n(xn, 3.0, cc, p2, L, v_src=vn)
        ops.su3_expm_mul_n(xn, p2, ss, out=x2)
    rec('  force_kick_to + expm_mul', timeit(two_launch), 3456)
    x3 = torch.empty_like(xn)
    rec('su3_flow_step (3 stages)', timeit(lambda: ops.su3_flow_step_n(xn, x2, p2, x3, 0.01, L)), 2880 + 2 * 3456)
    # The step with its embedded error estimate: stages 1 and 2, the kick into P3 (1728 B) and ONE kernel that reads
    # W0, W2, P1, P2, P3, writes W3 and reduces d (4 links x 864 B).  Next to it what that kernel replaces: the
    # expm_mul for W3, the expm_mul for W' and a torch distance + amax (4 x 1296 B of algorithmic traffic), the two
    # sides alternating so that each is repeated under the same conditions.
    ws_p3 = torch.empty((3, *xn.shape), dtype=xn.dtype, device=dev)
    x4 = torch.empty_like(xn)
    ops.su3_flow_step_err_n(xn, x2, ws_p3, x3, 0.01, L)             # fills P1..P3 and W2 (x3) for the composition
    pq = 17.0 * ws_p3[1] - ws_p3[0]

    def composed():
        ops.su3_expm_mul_n(x3, ws_p3[2], -17.0 / 36.0 * 0.01, out=x4)
        ops.su3_expm_mul_n(xn, pq, 0.01 / 16.0, out=x2)
        return torch.linalg.vector_norm(x4 - x2, dim=2).amax((1, 2)) / 9.0
    for rnd in range(3):
        rec(f'  2 x expm_mul + torch distance [{rnd}]', timeit(composed), 4 * 1296)
        rec(f'su3_flow_step [{rnd}]', timeit(lambda: ops.su3_flow_step_n(xn, x2, p2, x4, 0.01, L)), 2880 + 2 * 3456)
        rec(f'su3_flow_step_err [{rnd}]', timeit(lambda: ops.su3_flow_step_err_n(xn, x2, ws_p3, x3, 0.01, L)),
            2880 + 3456 + 1728 + 3456)
    del pq, x4, p2, x2, x3, ws_p3
    if a.flow_only:
        return
    rec('su3_plaq_reduce', timeit(lambda: ops.su3_plaq_sums_n(xn, L)), 576, 2800)
    native.set_tuning('xcd_swizzle', 0)
    rec('su3_plaq_reduce noswz', timeit(lambda: ops.su3_plaq_sums_n(xn, L)), 576, 2800)
    native.set_tuning('xcd_swizzle', 1)
    f = torch.empty_like(xn)
    rec('su3_force', timeit(lambda: native.call('l2q_su3_force', xn, 6.0, f, nb, *L)), 1152, 11200)
    native.set_tuning('xcd_swizzle', 0)
    rec('su3_force noswz', timeit(lambda: native.call('l2q_su3_force', xn, 6.0, f, nb, *L)), 1152, 11200)
    native.set_tuning('xcd_swizzle', 1)
    rec('su3_force_kick', timeit(lambda: ops.su3_force_kick_n(xn, 6.0, -0.005, vn, L)), 576 * 3, 11200)
    out = torch.empty_like(xn)
    rec('su3_expm_mul (no mask)', timeit(lambda: ops.su3_expm_mul_n(xn, vn, 0.01, out=out)), 1728)
    rec('su3_expm_mul (masked)', timeit(lambda: ops.su3_expm_mul_n(xn, vn, 0.01, mask, False, out=out)), 1728)
    rec('su3_projsu_vec8', timeit(lambda: ops.su3_projsu_vec8_n(xn)), 832)
    rec('su3_project_su', timeit(lambda: ops.su3_project_su_n(xn)), 1152)
    rec('su3_kinetic_reduce', timeit(lambda: ops.su3_kinetic_n(vn)), 576)
    v2 = vn.clone()
    rec('v_update (complex)', timeit(lambda: ops.v_update_(v2, f, *stq, 0.01, True)), 2592)
    rec('su3_pack', timeit(lambda: ops.su3_pack(xn.reshape(nb, -1))), 1152)
    nrm = torch.randn(8, nb, 4, V, dtype=torch.float64, device=dev)
    rec('su3_assemble_tah', timeit(lambda: ops.su3_assemble_tah_n(nrm)), 4 * (64 + 144))
    # reference points: device copy bandwidth
    a_ = torch.empty(2 ** 28, dtype=torch.float32, device=dev); b_ = torch.empty_like(a_)
    t = timeit(lambda: b_.copy_(a_))
    print(f'{"torch copy 1 GiB":34s} {t*1e3:8.3f} ms  {2*a_.numel()*4/t/1e9:8.1f} GB/s', flush=True)
    if a.gemm:
        h = 256
        K = 32 * V
        xv = torch.randn(nb, K, dtype=torch.float64, device=dev)
        fv = torch.randn(nb, K, dtype=torch.float64, device=dev)
        wx = torch.randn(h, K, dtype=torch.float64, device=dev) / K ** 0.5
        wv = torch.randn(h, K, dtype=torch.float64, device=dev) / K ** 0.5
        bx = torch.randn(h, dtype=torch.float64, device=dev)
        t = timeit(lambda: ops.gemm(xv, wx, bx, a2=fv, w2=wv, bias2=bx, act='tanh'), iters=5, warm=2)
        fl = 2.0 * nb * h * 2 * K
        print(f'{"gemm in  [nb,2*32V]x[h,..]":34s} {t*1e3:8.3f} ms  {fl/t/1e12:7.2f} TFLOP/s fp64', flush=True)
        t = timeit(lambda: torch.addmm(bx, xv, wx.t()), iters=5, warm=2)
        print(f'{"  (rocBLAS addmm, half of it)":34s} {t*1e3:8.3f} ms  {fl/2/t/1e12:7.2f} TFLOP/s fp64', flush=True)
        z = torch.randn(nb, h, dtype=torch.float64, device=dev)
        N_ = 36 * V
        ws_ = torch.randn(N_, h, dtype=torch.float64, device=dev) / h ** 0.5
        bs = torch.randn(N_, dtype=torch.float64, device=dev)
        co = torch.zeros(N_, dtype=torch.float64, device=dev)
        t = timeit(lambda: ops.gemm(z, ws_, bs, coeff=co, act='tanh'), iters=5, warm=2)
        fl = 2.0 * nb * h * N_
        print(f'{"gemm head [nb,h]x[36V,h]":34s} {t*1e3:8.3f} ms  {fl/t/1e12:7.2f} TFLOP/s fp64', flush=True)
        t = timeit(lambda: torch.addmm(bs, z, ws_.t()), iters=5, warm=2)
        print(f'{"  (rocBLAS addmm)":34s} {t*1e3:8.3f} ms  {fl/t/1e12:7.2f} TFLOP/s fp64', flush=True)
        heads = {'s': (ws_, bs, co.exp()), 't': (ws_.clone(), bs, None), 'q': (ws_.clone(), bs, co.exp())}
        vv = vn.reshape(nb, -1).clone(); ff = f.reshape(nb, -1)
        t = timeit(lambda: ops.vnet_heads_vupdate_(z, heads, (1., 1., 1.), vv, ff, 0.01, True), iters=5, warm=2)
        print(f'{"fused 3 heads + v_update":34s} {t*1e3:8.3f} ms  {3*fl/t/1e12:7.2f} TFLOP/s fp64', flush=True)


if __name__ == '__main__':
    main()
