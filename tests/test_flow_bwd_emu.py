"""CPU run of the kernel of l2q_su3_force_vjp (csrc/su3_flow_bwd.hip) itself: the file is compiled for the host with
g++ against the stand-in HIP header of tests/host_emu.py (every thread of a workgroup an OS thread),
under AddressSanitizer and UBSan as a stand-alone program (tests/native_host/flow_bwd_emu/), and compared with
torch.autograd of sum Re(conj(gf) F), F = (beta/3) tah(x @ staples(x)) of the restatement tests/flow_restatement.py.
Catches wrong terms, signs, indexing, wrap-around and out-of-bounds mistakes without a GPU; the GPU's own arithmetic
and the stage / step reverses built on the kernel are the business of tests/test_flow_bwd_gpu.py.  The kernel has one
variant, so no lattice is needed to select another."""
import numpy as np
import pytest
import torch

import flow_restatement as fr
import host_emu
from native_layout import pack
from oracle import su3 as osu3

NB = 2
BETA = 2.7
# extents 1 and 2 (the same link several times in one loop), a lattice that is no whole workgroup, and one of
# several workgroups per chain
LATTICES = [(1, 3, 2, 5), (3, 5, 2, 7), (2, 5, 8, 8)]


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = host_emu.build(tmp_path_factory.mktemp('flow_bwd_emu'), 'flow_bwd_emu')

    def run(L, swz, xn, gf, gx):
        (out,) = host_emu.run(exe, [xn.shape[0], *L, swz, repr(BETA)], [xn, gf, gx], 1)
        return torch.view_as_complex(torch.from_numpy(out).reshape(*gx.shape, 2))
    return run


def cnormal(rng, shape):
    return torch.from_numpy(rng.normal(size=shape) + 1j * rng.normal(size=shape))


@pytest.mark.parametrize('L', LATTICES)
def test_kernel_on_the_host_vs_autograd(emu, L):
    rng = np.random.default_rng(41)
    x = torch.from_numpy(osu3.project_su(rng.normal(size=(NB, 4, *L, 3, 3)) + 1j * rng.normal(size=(NB, 4, *L, 3, 3))))
    gf = cnormal(rng, (NB, 4, *L, 3, 3))               # a general cotangent: the kernel projects it itself
    V = int(np.prod(L))
    x.requires_grad_(True)
    a = fr.staples(x)
    f = (BETA / 3.0) * fr.tah(x @ a)
    want = pack(torch.autograd.grad((gf.conj() * f).real.sum(), x)[0])
    # the cotangent with the staples held constant (l2q_su3_force_bwd): (beta/3) TAH(gf) A^H
    frozen = pack((BETA / 3.0) * fr.tah(gf) @ fr.adj(a.detach()))
    ref = float(want.abs().max())
    for swz in (0, 1):
        g0 = cnormal(rng, (NB, 4, 9, V))
        got = emu(L, swz, pack(x.detach()), pack(gf), g0)      # gx += : the kernel starts from g0
        err = float((got - (g0 + want)).abs().max())
        off = float((frozen - want).abs().max())
        print(f'L={L} swz={swz}: max |got - want| = {err:.3e}, max |want| = {ref:.3e}, '
              f'staples-constant cotangent off by {off / ref:.3f} max |want|')
        assert ref > 0.0
        assert err <= 1e-12 * max(1.0, ref), (L, swz)
        # the test tells the full VJP from the staples-constant one
        assert off > 0.05 * ref
        assert float((got - (g0 + frozen)).abs().max()) > 0.05 * ref
