"""The 2x1 rectangle kernels (csrc/su3_rect_kernels.hip) past one workgroup and on degenerate extents:
l2q_su3_rect_reduce / _rect_force_add / _rect_bwd on lattices with an extent of 1, with every extent 2 (the long
side of the rectangle returns to its start), below one 256-thread block, with two blocks and a tail, and with three
blocks -- c = cb / nblk, blk = cb % nblk with nblk > 1 and the tail block run under a kernel-level check here.

References: oracle.su3.rect_sums and oracle.su3.grad_action_c1 (numpy restatement of the reference), the autograd
emulator tests/emu_native.py, and one identity that needs neither: with zero accumulators, force_add(coef) at link
(x, mu) equals coef TAH(U_mu(x) (gx / w)^H) with gx from rect_bwd(w) on the same field.
Tolerances as in test_train_gpu.py::test_su3_rect_kernels_vs_emulator: 1e-10 for sums, 1e-11 for fields."""
import numpy as np
import pytest
import torch

import emu_native
from oracle import su3 as osu3

pytestmark = pytest.mark.gpu

LATTICES = [(1, 3, 2, 5), (2, 2, 2, 2), (3, 5, 2, 7), (4, 4, 4, 5), (3, 4, 6, 8)]
NB = 3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope='module', params=LATTICES, ids=lambda L: 'x'.join(str(i) for i in L))
def case(request):
    """one random SU(3) field per lattice, shared by the tests below and left unchanged"""
    from l2hmc import _ops as ops
    L = request.param
    rng = np.random.default_rng(sum(L))
    shape = (NB, 4, *L, 3, 3)
    x = osu3.project_su(rng.normal(size=shape) + 1j * rng.normal(size=shape))
    acc = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    return {'L': L, 'x': x, 'xn': ops.su3_pack(dev(x)), 'acc': acc, 'accn': ops.su3_pack(dev(acc)), 'ops': ops}


def test_rect_sums_vs_oracle(case):
    ops, L = case['ops'], case['L']
    got = host(ops.su3_rect_sums_n(case['xn'], L))
    assert np.abs(got - osu3.rect_sums(case['x'])).max() < 1e-10


def test_rect_force_add_vs_oracle(case):
    """fn += coef TAH(U A_rect) on top of a random accumulator; the oracle's improved-action force minus its
    plaquette part is (beta c1 / 3) TAH(U A_rect)"""
    ops, L, x = case['ops'], case['L'], case['x']
    beta, c1 = 5.7, -0.331
    want = case['acc'] + osu3.grad_action_c1(x, beta, c1) - osu3.grad_action(x, osu3.coeffs(beta, c1)['plaq'])
    got = ops.su3_rect_force_add_n(case['xn'], beta * c1 / 3.0, case['accn'].clone(), L)
    assert np.abs(host(ops.su3_unpack(got, L)) - want).max() < 1e-11


def test_rect_bwd_vs_emulator(case):
    ops, L = case['ops'], case['L']
    w = torch.tensor([0.3, -1.2, 2.0], dtype=torch.float64)
    want = case['accn'].cpu().clone()
    emu_native.l2q_su3_rect_bwd(case['xn'].cpu(), w, want, NB, *L)
    got = ops.su3_rect_bwd_(case['accn'].clone(), case['xn'], w.cuda(), L)
    assert float((got.cpu() - want).abs().max()) < 1e-11


def test_rect_force_is_tah_of_link_times_cotangent(case):
    ops, L, x = case['ops'], case['L'], case['x']
    w = np.array([0.3, -1.2, 2.0])
    coef = 0.37
    zero = torch.zeros_like(case['xn'])
    gx = host(ops.su3_unpack(ops.su3_rect_bwd_(zero.clone(), case['xn'], dev(w), L), L))
    f = host(ops.su3_unpack(ops.su3_rect_force_add_n(case['xn'], coef, zero.clone(), L), L))
    g1 = gx / w.reshape(NB, 1, 1, 1, 1, 1, 1, 1)
    assert np.abs(f - coef * osu3.project_tah(x @ osu3.adj(g1))).max() < 1e-11
    assert np.abs(f).max() > 0.1                         # not vacuous
