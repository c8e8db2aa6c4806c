"""Restatement bits, parent against this commit: from one checkout's tests/ call the numpy CG loops and the trajectory
functions of the three Wilson restatement modules on the inputs of the host tests, dense and at each CG tolerance, and
write the sha256 of every returned array as JSON.

    python profiles/wilson_hop_single_source/restatement_bits.py TREE OUT.json     # TREE: a checkout's root
    python profiles/wilson_hop_single_source/restatement_bits.py --compare A.json B.json"""
import json
import os
import sys

from bits_common import compare, flat


def run(tree, dest):
    sys.path[:0] = [tree, os.path.join(tree, 'tests')]
    import wilson_eo_restatement as we
    import wilson_force_restatement as wfr
    import wilson_restatement as wr
    assert os.path.abspath(wr.__file__).startswith(os.path.abspath(tree)), wr.__file__
    res = {}

    def case(name, value):
        flat(name, value, res)

    for L in [(2, 2, 2, 2), (4, 2, 6, 2), (3, 4, 5, 2)]:
        x, b = wr.links(L, 2), wr.spinors(L, 2, 2)
        for kappa in wr.SOLVE_KAPPAS:
            for kn, kw in (('tol1e-10', dict(tol=1e-10, max_iter=200)), ('default', {}), ('max5', dict(max_iter=5)),
                           ('tol1e-6_every3', dict(tol=1e-6, check_every=3)), ('every1', dict(check_every=1))):
                tag = f'{L} kappa={kappa} {kn}'
                case(f'wr.cgnr {tag}', wr.cgnr(x, b, kappa, **kw))
                case(f'wfr.normal_cg {tag}', wfr.normal_cg(x, b, kappa, **kw))
                case(f'we.full_cgnr {tag}', we.full_cgnr(x, b, kappa, **kw))
                if all(e % 2 == 0 for e in L):
                    case(f'we.solve_eo {tag}', we.solve_eo(x, b, kappa, **kw))
                    case(f'we.normal_cg_eo {tag}', we.normal_cg_eo(x, b * we.mask(L, 0), kappa, **kw))
        case(f'wr.cgnr {L} no nrhs axis', wr.cgnr(x, b[:, 0], 0.10))
        big = b.copy()
        big[1, 1] = 0.0
        case(f'wr.cgnr {L} zero rhs', wr.cgnr(x, big, 0.12))
        case(f'wfr.normal_cg {L} zero rhs', wfr.normal_cg(x, big, 0.12))
    for mod, name, lattices in ((wfr, 'wfr', wfr.FD_LATTICES), (we, 'we', we.FD_LATTICES)):
        for L in lattices:
            x, phi, p = mod.fd_inputs(L)
            for ap in (False, True):
                for tol in (None, wfr.FD_TOL):
                    tag = f'{L} ap={ap} tol={tol}'
                    case(f'{name}.fermion_action {tag}', mod.fermion_action(x, phi, wr.KAPPA, ap, tol))
                    case(f'{name}.fermion_force {tag}', mod.fermion_force(x, phi, wr.KAPPA, ap, tol))
        for L in wfr.TRAJ_LATTICES:
            x, v, phi, s0 = mod.traj_inputs(L)
            case(f'{name}.traj_inputs {L}', (x, v, phi, s0))
            case(f'{name}.delta_h {L} dense', mod.delta_h(x, v, phi, **wfr.TRAJ))
            case(f'{name}.delta_h {L} cg', mod.delta_h(x, v, phi, **wfr.TRAJ, tol=wfr.TRAJ_TOL_MD, tol_h=wfr.TRAJ_TOL_H))
            case(f'{name}.delta_h {L} beta=0', mod.delta_h(x, v, phi, 0.0, wfr.TRAJ['kappa'], wfr.TRAJ['eps'],
                                                           wfr.TRAJ['nleapfrog']))
            case(f'{name}.leapfrog, hamiltonian, total_force {L}',
                 (mod.leapfrog(x, v, phi, 5.5, 0.12, 0.05, 2, True, 1e-10), mod.hamiltonian(x, v, phi, 5.5, 0.12, False, 1e-12),
                  mod.total_force(x, phi, 5.5, 0.12, False)))
    with open(dest, 'w') as f:
        json.dump(res, f, indent=0, sort_keys=True)
    print(f'{tree}: {len(res)} entries -> {dest}')


if __name__ == '__main__':
    if sys.argv[1] == '--compare':
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    run(os.path.abspath(sys.argv[1]), sys.argv[2])
