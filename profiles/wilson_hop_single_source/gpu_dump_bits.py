"""Bits on the GPU, parent against this commit: from one checkout (its package on its own library build) dump the sha256
of every array that the kernel entries, the four solvers, the pseudofermion force and one trajectory of each HMC class
return, as JSON.  Inputs: wr.links, wr.spinors, we.aux_field on (4, 4, 4, 4) and (4, 2, 6, 2), three chains, two
right-hand sides; the trajectories at wf.TRAJ on (4, 2, 2, 2) with a CPU generator seeded 11.

    python profiles/wilson_hop_single_source/gpu_dump_bits.py TREE OUT.json      # TREE: a checkout's root, built
    python profiles/wilson_hop_single_source/gpu_dump_bits.py --compare A.json B.json"""
import json
import os
import sys

from bits_common import compare, flat

NB, NRHS = 3, 2
KWS = {'default': {}, 'tol1e-6_every3': dict(tol=1e-6, check_every=3),
       'tol1e-30_max7_every3': dict(tol=1e-30, max_iter=7, check_every=3)}


def run(tree, dest):
    sys.path[:0] = [tree, os.path.join(tree, 'l2hmc-qcd_amd'), os.path.join(tree, 'tests')]
    import numpy as np
    import torch
    import wilson_eo_restatement as we
    import wilson_force_restatement as wf
    import wilson_restatement as wr
    from l2hmc import _ops as ops
    from l2hmc.dynamics.pytorch import fermion_hmc
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    assert os.path.abspath(ops.__file__).startswith(tree) and os.path.abspath(wr.__file__).startswith(tree)
    res = {}

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    for L in [(4, 4, 4, 4), (4, 2, 6, 2)]:
        lat = LatticeSU3(NB, list(L))
        psi, aux = wr.spinors(L, NB, NRHS), we.aux_field(L, NB, NRHS)
        xn, pn = ops.su3_pack(dev(wr.links(L, NB))), ops.su3_spinor_pack(dev(psi))
        src = [dev(we.pack_half(psi, p)) for p in (0, 1)]
        au = [dev(we.pack_half(aux, p)) for p in (0, 1)]
        for fl, (dagger, ap) in enumerate(wr.FLAGS):
            flat(f'su3_wilson_apply_n {L} flags {fl}', ops.su3_wilson_apply_n(xn, pn, wr.KAPPA, L, dagger, ap, norm=True), res)
            for p in (0, 1):
                for name, a, b, with_aux in we.uses():
                    kw = dict(a=a, aux=au[p], b=b) if with_aux else dict(a=a)
                    flat(f'su3_wilson_hop_eo_n {L} parity {p} flags {fl} {name}',
                         ops.su3_wilson_hop_eo_n(xn, src[1 - p], L, p, dagger, ap, norm=True, **kw), res)
        for kappa in wr.SOLVE_KAPPAS:
            for kn, kw in KWS.items():
                tag = f'{L} kappa={kappa} {kn}'
                flat(f'wilson_solve_n {tag}', lat.wilson_solve_n(xn, pn, kappa, **kw), res)
                flat(f'wilson_solve_eo_n {tag}', lat.wilson_solve_eo_n(xn, pn, kappa, **kw), res)
                flat(f'wilson_solve_normal_n {tag}', lat.wilson_solve_normal_n(xn, pn, kappa, **kw), res)
                flat(f'wilson_solve_schur_normal_n {tag}', lat.wilson_solve_schur_normal_n(xn, src[0], kappa, **kw), res)
            flat(f'pseudofermion_force_n {L} kappa={kappa}', lat.pseudofermion_force_n(xn, pn, kappa), res)
            flat(f'pseudofermion_force_n {L} kappa={kappa} even_odd', lat.pseudofermion_force_n(xn, src[0], kappa, even_odd=True), res)
        print(L, 'done', flush=True)
    L = (4, 2, 2, 2)
    lat = LatticeSU3(2, list(L))
    xn = ops.su3_pack(dev(wr.links(L, 2)))
    for cls in ('WilsonHMC', 'WilsonHMCEvenOdd'):
        g = torch.Generator().manual_seed(11)
        xo, metrics = getattr(fermion_hmc, cls)(lat, **wf.TRAJ).trajectory_n(xn, g)
        flat(f'{cls}.trajectory_n {L}', (xo, metrics, torch.randn(3, generator=g, dtype=torch.float64)), res)
        print(cls, {k: (v.tolist() if isinstance(v, torch.Tensor) else v) for k, v in metrics.items()}, flush=True)
    torch.cuda.synchronize()
    with open(dest, 'w') as f:
        json.dump(res, f, indent=0, sort_keys=True)
    print(f'{tree}: {len(res)} entries -> {dest}')


if __name__ == '__main__':
    if sys.argv[1] == '--compare':
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    run(os.path.abspath(sys.argv[1]), sys.argv[2])
