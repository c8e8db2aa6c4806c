"""Emulator entries of the clover sums and their VJP (l2q_su3_clover_reduce, l2q_su3_clover_bwd) for the host-logic
tests: the sums are tests/flow_restatement.clover_sums, the VJP is torch.autograd of that restatement.  The kernels
themselves are checked in test_clover_bwd_emu.py (host build) and test_clover_bwd_gpu.py."""
import numpy as np
import torch

import emu_native
import flow_restatement as fr


def links(xn, nb, L):
    """native xn[nb, 4, 9, V] -> x[nb, 4, T, X, Y, Z, 3, 3]"""
    return emu_native._mats(xn.reshape(nb, 4, 9, -1)).reshape(nb, 4, *L, 3, 3)


def native(x):
    """x[nb, 4, T, X, Y, Z, 3, 3] -> native xn[nb, 4, 9, V]"""
    nb = x.shape[0]
    return emu_native._native(x.reshape(nb, 4, -1, 3, 3))


def l2q_su3_clover_reduce(xn, nb, T, X, Y, Z, out, ws, wsn):
    out.copy_(fr.clover_sums(links(xn, nb, (T, X, Y, Z)))[0])


def l2q_su3_clover_bwd(xn, w, gx, nb, T, X, Y, Z, ws, wsn):
    assert wsn >= nb * 54 * T * X * Y * Z * 8, 'workspace smaller than l2q.h asks for'
    x = links(xn, nb, (T, X, Y, Z)).detach().clone().requires_grad_(True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad((w.reshape(nb, 3) * fr.clover_sums(x)[0]).sum(), x)
    gx.add_(native(g).reshape(gx.shape))


def install_emu_clover(monkeypatch):
    """Call after emu_native.install(monkeypatch)."""
    monkeypatch.setitem(emu_native._TABLE, 'l2q_su3_clover_reduce', l2q_su3_clover_reduce)
    monkeypatch.setitem(emu_native._TABLE, 'l2q_su3_clover_bwd', l2q_su3_clover_bwd)


def clover_grad(x, w):
    """(sums [nb, 3], d (w . sums) / dx) of the restatement, x[nb, 4, T, X, Y, Z, 3, 3] on the CPU"""
    x = x.detach().clone().requires_grad_(True)
    sums = fr.clover_sums(x)[0]
    (g,) = torch.autograd.grad((w * sums).sum(), x)
    return sums.detach(), g


def random_links(nb, L, seed):
    from oracle import su3 as osu3
    rng = np.random.default_rng(seed)
    return torch.from_numpy(osu3.project_su(rng.normal(size=(nb, 4, *L, 3, 3)) + 1j * rng.normal(size=(nb, 4, *L, 3, 3))))


def weight_cases(nb, seed):
    """one-hot in each of the three columns, and one random [nb, 3]"""
    ws = []
    for k in range(3):
        w = torch.zeros(nb, 3, dtype=torch.float64)
        w[:, k] = 1.0
        ws.append(w)
    ws.append(torch.from_numpy(np.random.default_rng(seed).normal(size=(nb, 3))))
    return ws
