"""TEST INFRASTRUCTURE: one trajectory of each dynamical-quark HMC class of fermion_hmc.py that existed before the
multi-shift CG, on (4, 2, 2, 2) x 2 chains from `wr.links` with a CPU generator (the same numbers on any machine), as
arrays: the native links after the accept step, dH, the accept mask and the plaquette.  `python tests/hmc_golden.py OUT`
writes them to OUT (.npz); tests/golden/fermion_hmc_parent.npz is that file made on an MI355X at the commit before
`WilsonRHMC` was added, and tests/test_wilson_multishift_gpu.py holds the classes to its bits."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'golden', 'fermion_hmc_parent.npz')
L, NB, SEED = (4, 2, 2, 2), 2, 23
CLASSES = ['WilsonHMC', 'WilsonHMCEvenOdd', 'WilsonHMCMixed', 'WilsonCloverHMC']


def run(cls):
    import torch
    import wilson_force_restatement as wf
    import wilson_restatement as wr
    from l2hmc.dynamics.pytorch import fermion_hmc
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    lat = LatticeSU3(NB, list(L))
    kw = dict(wf.TRAJ)
    if cls == 'WilsonCloverHMC':
        kw['c_sw'] = 1.0
    hmc = getattr(fermion_hmc, cls)(lat, **kw)
    g = torch.Generator()
    g.manual_seed(SEED)
    x = torch.from_numpy(wr.links(L, NB)).cuda()
    xo, m = hmc.trajectory_n(lat.pack(x), g)
    out = {'x': xo, 'dH': m['dH'], 'acc_mask': m['acc_mask'], 'plaq': m['plaq']}
    return {k: np.ascontiguousarray(torch.view_as_real(v).cpu().numpy() if v.is_complex() else v.cpu().numpy())
            for k, v in out.items()}


if __name__ == '__main__':
    np.savez(sys.argv[1], **{f'{c}.{k}': v for c in CLASSES for k, v in run(c).items()})
    print('wrote', sys.argv[1])
