"""CPU run of the kernels of csrc/su3_clover_bwd.hip themselves: the file is compiled for the host with g++ against a
stand-in HIP header that executes every thread of a workgroup as an OS thread (tests/native_host/clover_bwd_emu/),
under AddressSanitizer and UBSan as a stand-alone program, and l2q_su3_clover_bwd is compared with torch.autograd
through the restatement tests/flow_restatement.clover_sums.  Catches wrong terms, signs, indexing, wrap-around and
out-of-bounds mistakes without a GPU; the GPU's own arithmetic is the business of tests/test_clover_bwd_gpu.py.
The kernel has one variant, so no lattice is needed to select another."""
import os
import subprocess

import numpy as np
import pytest
import torch

import flow_restatement as fr
from oracle import su3 as osu3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, 'tests', 'native_host', 'clover_bwd_emu')
NB = 2
# extents 1 and 2 (the same link several times in one clover), a lattice that is no whole workgroup, and one of
# several workgroups per chain
LATTICES = [(1, 3, 2, 5), (3, 5, 2, 7), (2, 5, 8, 8)]


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('clover_bwd_emu')
    exe = tmp / 'clover_bwd_emu'
    subprocess.run(['g++', '-std=c++20', '-O1', '-g', '-pthread', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=undefined', '-I', EMU, '-I', os.path.join(ROOT, 'l2hmc-qcd_amd', 'csrc'),
                    os.path.join(EMU, 'clover_bwd_emu.cpp'), '-o', str(exe)], check=True)

    def run(L, swz, xn, w, gx):
        fx, fw, fg, fo = (str(tmp / n) for n in ('x.bin', 'w.bin', 'g.bin', 'o.bin'))
        torch.view_as_real(xn).numpy().tofile(fx)
        w.numpy().tofile(fw)
        torch.view_as_real(gx).numpy().tofile(fg)
        subprocess.run([str(exe), str(xn.shape[0]), *map(str, L), str(swz), fx, fw, fg, fo], check=True)
        return torch.view_as_complex(torch.from_numpy(np.fromfile(fo)).reshape(*gx.shape, 2))
    return run


def pack(x):
    """x[nb, 4, T, X, Y, Z, 3, 3] -> the native layout xn[nb, 4, 9, V]"""
    nb = x.shape[0]
    return x.reshape(nb, 4, -1, 9).permute(0, 1, 3, 2).contiguous()


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
