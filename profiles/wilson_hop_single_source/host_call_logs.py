"""Host call logs, parent against this commit: run one tree's `wilson.py` and `fermion_hmc.py` on CPU tensors through the
stand-ins of tests/test_wilson_cg_host.py (this commit's, for both trees) and write every call log and the sha256 of
every returned tensor as JSON.

    python profiles/wilson_hop_single_source/host_call_logs.py TREE OUT.json      # TREE: a checkout's root
    python profiles/wilson_hop_single_source/host_call_logs.py --compare A.json B.json

Three more entries get stand-ins here, on `oracle.su3` and `wf.force`: `su3_wilson_force_n`, `su3_force_kick_n` and
`su3_expm_mul_n`, which the force and the leapfrog call."""
import json
import os
import sys

from bits_common import compare, flat

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def run(tree, dest):
    sys.path[:0] = [tree, os.path.join(tree, 'l2hmc-qcd_amd'), os.path.join(ROOT, 'tests')]
    import numpy as np
    import torch
    import test_wilson_cg_host as host
    import wilson_force_restatement as wf
    import wilson_restatement as wr
    from l2hmc import _ops as ops
    from l2hmc.dynamics.pytorch.fermion_hmc import WilsonHMC, WilsonHMCEvenOdd
    from oracle import su3 as osu3
    assert os.path.abspath(ops.__file__).startswith(os.path.abspath(tree)), ops.__file__

    class StandIns(host.StandIns):
        NAMES = host.StandIns.NAMES + ('su3_wilson_force_n', 'su3_force_kick_n', 'su3_expm_mul_n')

        def su3_wilson_force_n(self, xn, X, Y, kappa, lat, antiperiodic_t=True, coef=1.0, f_in=None, out=None):
            self.log.append(('force', bool(antiperiodic_t), f_in is not None))
            f = wf.force(wf.unpack_links(xn.numpy(), lat), wr.unpack_spinor(X.numpy(), lat),
                         wr.unpack_spinor(Y.numpy(), lat), kappa, antiperiodic_t)
            res = coef * torch.from_numpy(wf.pack_links(f)) + (0 if f_in is None else f_in)
            return res if out is None else out.copy_(res)

        def su3_force_kick_n(self, xn, beta, coef, vn, lat):
            self.log.append(('gauge kick', None, None))
            return vn.add_(coef * torch.from_numpy(wf.pack_links(osu3.grad_action(wf.unpack_links(xn.numpy(), lat), beta))))

        def su3_expm_mul_n(self, xn, vn, eps):
            self.log.append(('link update', None, None))
            L = self.lattice
            x, v = wf.unpack_links(xn.numpy(), L), wf.unpack_links(vn.numpy(), L)
            return torch.from_numpy(wf.pack_links(osu3.expm(eps * v) @ x))

    st = StandIns()
    for name in st.NAMES:
        setattr(ops, name, getattr(st, name))
    res = {}

    def case(name, fn):
        del st.log[:]
        flat(name, fn(), res)
        res[name + ' call log'] = repr(st.log)

    kws = {'default': {}, 'tol1e-6_every3': dict(tol=1e-6, check_every=3),
           'tol1e-30_max7_every3': dict(tol=1e-30, max_iter=7, check_every=3)}
    for L in host.LATTICES:
        lat, x, b, xn, bn = host.inputs(L)
        st.lattice = L
        be = ops.su3_spinor_split_eo(bn, L)[0].contiguous()
        for kappa in wr.SOLVE_KAPPAS:
            for kn, kw in kws.items():
                tag = f'{L} kappa={kappa} {kn}'
                case(f'wilson_solve_n {tag}', lambda: lat.wilson_solve_n(xn, bn, kappa, **kw))
                case(f'wilson_solve_eo_n {tag}', lambda: lat.wilson_solve_eo_n(xn, bn, kappa, **kw))
                case(f'wilson_solve_normal_n {tag}', lambda: lat.wilson_solve_normal_n(xn, bn, kappa, **kw))
                case(f'wilson_solve_schur_normal_n {tag}', lambda: lat.wilson_solve_schur_normal_n(xn, be, kappa, **kw))
            for eo, phi in ((False, bn), (True, be)):
                tag = f'{L} kappa={kappa} even_odd={eo}'
                case(f'pseudofermion_action_n {tag}', lambda: lat.pseudofermion_action_n(xn, phi, kappa, even_odd=eo))
                case(f'pseudofermion_force_n {tag}',
                     lambda: lat.pseudofermion_force_n(xn, phi, kappa, even_odd=eo, tol=1e-8))
            for name in ('pseudofermion_refresh_n', 'pseudofermion_refresh_eo_n'):
                def refresh():
                    g = torch.Generator().manual_seed(7)
                    return getattr(lat, name)(xn, kappa, 2, g), torch.randn(3, generator=g, dtype=torch.float64)
                case(f'{name} {L} kappa={kappa}', refresh)
        case(f'wilson_solve_eo_n {L} zero rhs, no nrhs axis',
             lambda: (lat.wilson_solve_eo_n(xn, torch.zeros_like(bn), 0.1), lat.wilson_solve_eo_n(xn, bn[:, 0], 0.1)))
    L = (2, 2, 2, 2)
    lat, x, b, xn, bn = host.inputs(L)
    st.lattice = L
    vn = torch.from_numpy(wf.pack_links(wf.momentum(L, host.NB, 1)))
    for cls in (WilsonHMC, WilsonHMCEvenOdd):
        hmc = cls(lat, tol_md=1e-8, npf=2, **wf.TRAJ)
        phin = (lat.pseudofermion_refresh_eo_n if hmc.even_odd else lat.pseudofermion_refresh_n)(
            xn, hmc.kappa, 2, torch.Generator().manual_seed(3))[0]
        case(f'{cls.__name__}.leapfrog_n {L}', lambda: hmc.leapfrog_n(xn, vn, phin))
    with open(dest, 'w') as f:
        json.dump(res, f, indent=0, sort_keys=True)
    print(f'{tree}: {len(res)} entries -> {dest}')


if __name__ == '__main__':
    if sys.argv[1] == '--compare':
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    run(os.path.abspath(sys.argv[1]), sys.argv[2])
