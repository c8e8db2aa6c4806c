"""CPU run of the kernels of csrc/su3_clover_bwd.hip themselves: the file is compiled for the host with g++ against a
stand-in HIP header that executes every thread of a workgroup as an OS thread (tests/host_emu.py),
under AddressSanitizer and UBSan as a stand-alone program, and l2q_su3_clover_bwd is compared with torch.autograd
through the restatement tests/flow_restatement.clover_sums.  Catches wrong terms, signs, indexing, wrap-around and
out-of-bounds mistakes without a GPU; the GPU's own arithmetic is the business of tests/test_clover_bwd_gpu.py.
The kernel has one variant, so no lattice is needed to select another."""
import numpy as np
import pytest
import torch

import flow_restatement as fr
import host_emu
from native_layout import pack
from oracle import su3 as osu3

NB = 2
# extents 1 and 2 (the same link several times in one clover), a lattice that is no whole workgroup, and one of
# several workgroups per chain
LATTICES = [(1, 3, 2, 5), (3, 5, 2, 7), (2, 5, 8, 8)]


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = host_emu.build(tmp_path_factory.mktemp('clover_bwd_emu'), 'clover_bwd_emu')

    def run(L, swz, xn, w, gx):
        (out,) = host_emu.run(exe, [xn.shape[0], *L, swz], [xn, w, gx], 1)
        return torch.view_as_complex(torch.from_numpy(out).reshape(*gx.shape, 2))
    return run


def weights(rng):
    """one-hot in each of the three columns, and one random [nb, 3]"""
    ws = []
    for k in range(3):
        w = torch.zeros(NB, 3, dtype=torch.float64)
        w[:, k] = 1.0
        ws.append(w)
    ws.append(torch.from_numpy(rng.normal(size=(NB, 3))))
    return ws


@pytest.mark.parametrize('L', LATTICES)
def test_kernel_on_the_host_vs_autograd(emu, L):
    rng = np.random.default_rng(23)
    x = torch.from_numpy(osu3.project_su(rng.normal(size=(NB, 4, *L, 3, 3)) + 1j * rng.normal(size=(NB, 4, *L, 3, 3))))
    V = int(np.prod(L))
    x.requires_grad_(True)
    sums = fr.clover_sums(x)[0]
    xn = pack(x.detach())
    for i, w in enumerate(weights(rng)):
        want = pack(torch.autograd.grad((w * sums).sum(), x, retain_graph=True)[0])
        g0 = torch.from_numpy(rng.normal(size=(NB, 4, 9, V)) + 1j * rng.normal(size=(NB, 4, 9, V)))
        got = emu(L, i & 1, xn, w, g0)                 # gx += : the kernel starts from g0
        err, ref = float((got - (g0 + want)).abs().max()), float(want.abs().max())
        print(f'L={L} w#{i}: max |got - want| = {err:.3e}, max |want| = {ref:.3e}')
        assert ref > 0.0
        assert err <= 1e-12 * max(1.0, ref), (L, i)
