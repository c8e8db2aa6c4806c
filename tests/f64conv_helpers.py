"""Fixtures of the fp64 conv stack (tests/golden/make_golden_f64conv.py) and the emulator entries
the host-logic tests route the fp64 conv kernels to."""
import numpy as np
import torch

# fp64 conv-stack entry points; the fp32 restatements in emu_native are dtype-generic torch code
F64_CONV_ENTRIES = ('l2q_conv_gemm_periodic', 'l2q_nchw_to_nhwc_pad', 'l2q_maxpool_act_nhwc',
                    'l2q_im2col_periodic', 'l2q_col2im_periodic', 'l2q_maxpool_act_nhwc_bwd')


def adam_sd1(g):
    """{'sd1.<param>': ...}: one torch.optim.Adam(lr) step of every parameter `sd.<param>` that has a
    stored gradient (`grad.<param>` or `grad.networks.<param>`) -- the reference's optimizer step."""
    out, params = {}, []
    for k in g:
        if not k.startswith('sd.'):
            continue
        name = k[3:]
        gk = 'grad.' + name if ('grad.' + name) in g else 'grad.networks.' + name
        if gk not in g:
            continue
        p = torch.nn.Parameter(torch.from_numpy(np.array(g[k], dtype=np.float64)))
        p.grad = torch.from_numpy(np.array(g[gk], dtype=np.float64))
        params.append((name, p))
    torch.optim.Adam([p for _, p in params], lr=float(g['lr'])).step()
    for name, p in params:
        out['sd1.' + name] = p.detach().numpy()
    return out


def train_fixture(golden, name='u1_train_conv_f64'):
    """The training fixture with its updated parameters restored (the file stores them as
    `sd1_params = 'adam(sd, grad, lr)'`, see make_golden_f64conv.py)."""
    g = golden(name)
    if str(g.get('sd1_params', '')) == 'adam(sd, grad, lr)':
        g = {**g, **adam_sd1(g)}
    return g


def install_emu_f64(monkeypatch):
    import emu_native
    for e in F64_CONV_ENTRIES:
        monkeypatch.setitem(emu_native._TABLE, e + '_f64', emu_native._TABLE[e + '_f32'])
