"""CPU run of the kernels of csrc/su3_loops.hip themselves: the file is compiled for the host with g++ against a
stand-in HIP header that executes every thread of a workgroup as an OS thread (tests/host_emu.py), under
AddressSanitizer and UBSan as a stand-alone program, and its three entry points are compared with the restatement
tests/loops_restatement.py.  Catches indexing, wrap-around and out-of-bounds mistakes without a GPU; rounding of the
GPU's own arithmetic is the business of tests/test_loops_gpu.py."""
import numpy as np
import pytest
import torch

import host_emu
import loops_restatement as lr
from native_layout import pack, unpack
from oracle import su3 as osu3

NB = 2
# extents 1 and 2, a lattice that is no whole workgroup, and one of several workgroups per chain
LATTICES = [(1, 3, 2, 5), (3, 5, 2, 7), (2, 5, 8, 8)]


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = host_emu.build(tmp_path_factory.mktemp('loops_emu'), 'loops_emu')

    def run(mode, L, p1, p2, swz, a, b):
        (out,) = host_emu.run(exe, [mode, a.shape[0], *L, p1, p2, swz], [a, b], 1)
        return torch.from_numpy(out)
    return run


@pytest.mark.parametrize('L', LATTICES)
def test_kernels_on_the_host(emu, L):
    rng = np.random.default_rng(17)
    x = torch.from_numpy(osu3.project_su(rng.normal(size=(NB, 4, *L, 3, 3)) + 1j * rng.normal(size=(NB, 4, *L, 3, 3))))
    V = int(np.prod(L))
    xn = pack(x)
    lines = {n: lr.line(x, n) for n in (1, 2, 3)}
    # loop sums: the plaquette, a true 2 x 3 loop from two different line fields, shifts beyond every extent
    for r, t, swz in ((1, 1, 0), (2, 3, 1), (5, 9, 0)):
        a, b = lines[min(r, 3)], lines[min(t, 3)]
        want, scale = lr.loop_sums(a, r, b, t)
        got = torch.view_as_complex(emu('loops', L, r, t, swz, pack(a), pack(b)).reshape(NB, 12, 2))
        assert float(((got - want).abs() / scale.clamp(min=float(V))).max()) <= 1e-14, (r, t)
    # one more link at shifts 0, 1 and past the extents; in place gives the same bits
    for n in (0, 1, 7):
        want = torch.stack([lines[2][:, mu] @ lr.sh(x[:, mu], mu, n) for mu in range(4)], 1)
        got = emu('extend', L, n, 0, n & 1, pack(lines[2]), xn)
        assert float((unpack(torch.view_as_complex(got.reshape(NB, 4, 9, V, 2)), L) - want).abs().max()) <= 1e-14, n
        assert torch.equal(emu('extend_alias', L, n, 0, n & 1, pack(lines[2]), xn), got), n
    for mu in range(4):
        want = lr.polyakov(x, mu)
        got = torch.view_as_complex(emu('polyakov', L, mu, 0, 0, xn, xn).reshape(NB, -1, 2)).reshape(want.shape)
        assert float((got - want).abs().max()) <= L[mu] * 1e-14, mu
