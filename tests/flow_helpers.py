"""Emulator entries of the Wilson flow and its reverse sweep (l2q_su3_flow_stage, l2q_su3_flow_step,
l2q_su3_force_vjp, l2q_su3_flow_stage_bwd, l2q_su3_flow_step_bwd) for the host-logic tests: the forward is
tests/flow_restatement.py, every VJP is torch.autograd of that restatement.  The kernel itself is checked in
test_flow_bwd_emu.py (host build) and test_flow_bwd_gpu.py."""
import torch

import emu_native
import flow_restatement as fr
from clover_helpers import links, native

FIELD = 36 * 16                                   # bytes of one chain's links per site


def _vjp(fn, x, cot):
    """d Re<cot, fn(x)> / dx in torch's convention for complex tensors"""
    x = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(fn(x), x, grad_outputs=cot)
    return g


def l2q_su3_flow_stage(x_in, p_in, c, s, p_out, x_out, nb, T, X, Y, Z):
    L = (T, X, Y, Z)
    p, x = fr.flow_stage(links(x_in, nb, L), None if p_in is None else links(p_in, nb, L), c, s)
    p_out.copy_(native(p).reshape(p_out.shape))
    x_out.copy_(native(x).reshape(x_out.shape))


def l2q_su3_flow_step(x_in, x_out, ws_p, ws_x, eps, nb, T, X, Y, Z):
    assert all(a.data_ptr() != b.data_ptr() for a, b in ((x_in, x_out), (x_in, ws_x), (x_out, ws_x)))
    x_out.copy_(native(fr.flow_step(links(x_in, nb, (T, X, Y, Z)), eps)).reshape(x_out.shape))


def l2q_su3_force_vjp(xn, gf, beta, gx, nb, T, X, Y, Z):
    L = (T, X, Y, Z)
    assert gx.data_ptr() not in (xn.data_ptr(), gf.data_ptr())
    g = _vjp(lambda x: (beta / 3.0) * fr.tah(x @ fr.staples(x)), links(xn, nb, L), links(gf, nb, L))
    gx.add_(native(g).reshape(gx.shape))


def l2q_su3_flow_stage_bwd(x_in, p_out, c, s, gx_out, gp, gx_in, nb, T, X, Y, Z, ws, wsn):
    L = (T, X, Y, Z)
    V = T * X * Y * Z
    assert wsn >= nb * (1 + 4 * ((V + 255) // 256)) * 8, 'workspace smaller than l2q.h asks for'
    x, p = links(x_in, nb, L), links(p_out, nb, L)
    # X_out = exp(s P_out) X_in with P_out a leaf, then P_out = P_in + c TAH(X_in A) at the summed cotangent of P_out
    xl, pl = x.detach().clone().requires_grad_(True), p.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        g_x, g_p = torch.autograd.grad(torch.matrix_exp(s * pl) @ xl, (xl, pl), grad_outputs=links(gx_out, nb, L))
    gp.add_(native(g_p).reshape(gp.shape))
    g_x = g_x + _vjp(lambda y: c * fr.tah(y @ fr.staples(y)), x, links(gp, nb, L))
    gx_in.copy_(native(g_x).reshape(gx_in.shape))


def l2q_su3_flow_step_bwd(x_in, eps, gx_out, gx_in, nb, T, X, Y, Z, ws, wsn):
    L = (T, X, Y, Z)
    V = T * X * Y * Z
    assert wsn >= 7 * nb * FIELD * V + nb * (1 + 4 * ((V + 255) // 256)) * 8, 'workspace smaller than l2q.h asks for'
    assert wsn <= 8 * nb * FIELD * V, 'more than eight fields'
    g = _vjp(lambda x: fr.flow_step(x, eps), links(x_in, nb, L), links(gx_out, nb, L))
    gx_in.copy_(native(g).reshape(gx_in.shape))


def install_emu_flow(monkeypatch):
    """Call after emu_native.install(monkeypatch)."""
    for fn in (l2q_su3_flow_stage, l2q_su3_flow_step, l2q_su3_force_vjp, l2q_su3_flow_stage_bwd,
               l2q_su3_flow_step_bwd):
        monkeypatch.setitem(emu_native._TABLE, fn.__name__, fn)
