"""TEST INFRASTRUCTURE: what the Wilson-fermion GPU tests (test_wilson_gpu.py, test_wilson_force_gpu.py,
test_wilson_eo_gpu.py) and tests/test_wilson_force_emu.py share: moving arrays to and from the device, unit links, the
bit-level anti-Hermiticity check of a native force field, and the builders of an HMC object and its native fields."""
import numpy as np
import torch

import wilson_eo_restatement as we
import wilson_force_restatement as wf


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def unit_links(nb, L):
    return np.broadcast_to(np.eye(3, dtype=complex), (nb, 4, *L, 3, 3)).copy()


def antihermitian_bits(fn):
    """plane (j, i) is (-re, im) of plane (i, j), the diagonal has no real part"""
    m = fn.reshape(*fn.shape[:-2], 3, 3, fn.shape[-1])
    t = np.swapaxes(m, -3, -2)
    return np.array_equal(t.real, -m.real) and np.array_equal(t.imag, m.imag)


def _hmc(L, nb=2, cls='WilsonHMC', **kw):
    """(lattice, HMC object of class `cls` of fermion_hmc.py at wf.TRAJ with `kw` over it)"""
    from l2hmc.dynamics.pytorch import fermion_hmc
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    lat = LatticeSU3(nb, list(L))
    return lat, getattr(fermion_hmc, cls)(lat, **{**wf.TRAJ, **kw})


def _native(x, v, phi, half=False):
    """links, momentum and pseudofermion on the device in the native layout; half: phi as its even half field"""
    from l2hmc import _ops as ops
    return ops.su3_pack(dev(x)), ops.su3_pack(dev(v)), dev(we.pack_half(phi, 0)) if half else ops.su3_spinor_pack(dev(phi))
