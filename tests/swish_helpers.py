"""Emulator entries of the two entry points the swish training path adds (l2q_act_bwd_sums,
l2q_act_fwd_r16), restated with plain torch ops for the host-logic tests; the kernels themselves are
checked on the GPU (test_swish_train_gpu.py).  The emulator's max-pool backward is a VJP of its forward
and covers swish as it stands."""
import torch

import emu_native


def l2q_act_bwd_sums(dy, y, act, M, N, esz, dz, bgrad, ws=None, wsn=0):
    """dz = dy * act'(y) (swish: y is the pre-activation), bgrad += column sums of dz (double partials)"""
    out = torch.empty_like(dy)
    emu_native.l2q_act_bwd(dy, y, act, M * N, esz, out)
    dz.copy_(out)
    bgrad.add_(out.reshape(M, N).double().sum(0).to(bgrad.dtype).reshape(bgrad.shape))


def l2q_act_fwd_r16(ht, x, act, n, y):
    """r16(act(r16(x))) on fp32 containers: autocast's rounding points around an activation"""
    hd = torch.float16 if ht == 0 else torch.bfloat16
    r16 = lambda t: t.to(hd).float()
    y.copy_(r16(emu_native._act(r16(x), act)))


def install_emu_swish(monkeypatch):
    """Call after emu_native.install(monkeypatch).  Also keeps a surrounding torch.autocast region (the
    'autograd' route of helpers.check_half_train_step) out of the emulator: the HIP kernels do not see
    autocast, but the emulator's torch matmuls would run in 16 bit and round their result once more than
    the kernels do -- last-bit differences in the pre-activations, which swish' (unlike the piecewise
    constant derivatives) passes on to the gradients."""
    from l2hmc import native
    monkeypatch.setitem(emu_native._TABLE, 'l2q_act_bwd_sums', l2q_act_bwd_sums)
    monkeypatch.setitem(emu_native._TABLE, 'l2q_act_fwd_r16', l2q_act_fwd_r16)
    inner = native.call

    def call(name, *args):
        with torch.autocast('cpu', enabled=False):
            inner(name, *args)
    monkeypatch.setattr(native, 'call', call)
