"""The U(1) conv stack in float64 (`precision=float64` with a conv network) on the MI355X: the fp64
conv kernels against torch in fp64, the sampler against the reference's float64 conv fixture
(tests/golden/u1_conv_f64.npz), the training step against tests/golden/u1_train_conv_f64.npz, and
the reference's CLI at precision=float64 end to end."""
import numpy as np
import pytest
import torch

import helpers
from f64conv_helpers import train_fixture

pytestmark = pytest.mark.gpu

F = torch.nn.functional


def host(t):
    return t.detach().cpu().numpy()


def err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(autouse=True)
def _f64_default():
    torch.set_default_dtype(torch.float64)       # (conftest puts the previous default back)
    yield
    # every launch of this module completes inside the test that made it: a device error is
    # reported here, not by whichever test synchronises next
    torch.cuda.synchronize()


def _ppad(x, k):
    """PeriodicPadding(k - 1) of an NCHW tensor (network.py's conv input)."""
    p = k - 1
    if p == 0:
        return x
    x = torch.cat([x[:, :, -p:, :], x, x[:, :, :p, :]], 2)
    return torch.cat([x[:, :, :, -p:], x, x[:, :, :, :p]], 3)


def _act(z, act):
    return {None: lambda t: t, 'tanh': torch.tanh, 'relu': torch.relu, 'elu': F.elu,
            'leaky_relu': lambda t: F.leaky_relu(t, 0.01)}[act](z)


def _conv_ref(x, w, b, pool, act):
    """torch fp64 (CPU): periodic pad -> Conv2d -> [MaxPool2d] -> act, NHWC out."""
    y = F.conv2d(_ppad(x, w.shape[-1]), w, b)
    if pool > 1:
        y = F.max_pool2d(y, pool)
    return _act(y, act).permute(0, 2, 3, 1).contiguous()


def _data(dims, seed=11):
    nb, C, H, W, k, cout = dims
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(nb, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(cout, C, k, k, generator=g, dtype=torch.float64) / (C * k * k) ** 0.5
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    return x, w, b


def _xin(x, layout):
    return x.cuda() if layout == 'nchw' else x.permute(0, 2, 3, 1).contiguous().cuda()


# (nb, C, H, W, k, cout): k = 1..5 (compile-time kernel sizes) and 6 (the generic one); cout <= 32, <= 64
# and > 64 select the 32 / 64 / 128-wide output-channel tiles; the ragged shapes of the fp32 test
# (test_kernels_gpu.py::test_conv_gemm_periodic_equals_im2col_gemm); odd C takes the element-wise gathers
CONV_DIMS = [(3, 2, 4, 6, 5, 8), (2, 8, 6, 6, 3, 16), (5, 16, 7, 5, 3, 32), (2, 64, 4, 4, 2, 128),
             (130, 4, 8, 8, 3, 3), (1, 3, 2, 3, 3, 5), (4, 6, 5, 7, 1, 40), (3, 4, 6, 6, 4, 70),
             (2, 5, 7, 8, 6, 20), (2, 12, 9, 9, 5, 64)]


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dims', CONV_DIMS)
def test_conv_gemm_periodic_f64(layout, dims):
    """l2q_conv_gemm_periodic_f64 (implicit GEMM on the f64 MFMA) against torch's fp64 Conv2d on the
    periodically padded input, and against the materialised im2col_f64 + GEMM of the training tape."""
    from l2hmc import _ops as ops
    x, w, b = _data(dims)
    want = _conv_ref(x, w, b, 1, 'leaky_relu')
    xin = _xin(x, layout)
    got = ops.conv2d_periodic_gemm(xin, layout, w.cuda(), b.cuda(), 1, 'leaky_relu')
    assert got.dtype == torch.float64 and got.shape == want.shape
    scale = max(1.0, float(want.abs().max()))
    assert float((got.cpu() - want).abs().max()) < 1e-13 * scale
    got2, ctx = ops.conv2d_periodic_gemm_train(xin, layout, w.cuda(), b.cuda(), 1, 'leaky_relu')
    assert ctx['col'].dtype == torch.float64
    assert float((got2 - got).abs().max()) < 1e-13 * scale


@pytest.mark.parametrize('act', ['tanh', 'relu', 'leaky_relu', 'elu'])
@pytest.mark.parametrize('dims,pool', [((3, 4, 6, 5, 3, 8), 2), ((2, 8, 4, 4, 2, 70), 2),
                                       ((2, 3, 5, 7, 2, 6), 3)])
def test_conv_pool_act_f64(dims, pool, act):
    """conv + MaxPool2d(pool) + activation (l2q_maxpool_act_nhwc_f64, vector and element-wise forms)
    and the first layer's channel pad (l2q_nchw_to_nhwc_pad_f64)."""
    from l2hmc import _ops as ops
    x, w, b = _data(dims, seed=5)
    want = _conv_ref(x, w, b, pool, act)
    scale = max(1.0, float(want.abs().max()))
    for layout in ('nchw', 'nhwc'):
        got = ops.conv2d_periodic_gemm(_xin(x, layout), layout, w.cuda(), b.cuda(), pool, act)
        assert float((got.cpu() - want).abs().max()) < 1e-13 * scale, layout
        got2, _ = ops.conv2d_periodic_gemm_train(_xin(x, layout), layout, w.cuda(), b.cuda(), pool, act)
        assert float((got2.cpu() - want).abs().max()) < 1e-13 * scale, layout
    C = x.shape[1]
    cpad = C + C % 2
    xp = ops.nchw_to_nhwc_pad(x.cuda(), cpad)
    assert xp.dtype == torch.float64 and xp.shape == (x.shape[0], x.shape[2], x.shape[3], cpad)
    assert torch.equal(xp[..., :C].cpu(), x.permute(0, 2, 3, 1)) and not bool(xp[..., C:].any())
    wp = F.pad(w.permute(0, 2, 3, 1), (0, cpad - C)).contiguous().cuda()
    got = ops.conv2d_periodic_gemm(xp, 'nhwc', wp.permute(0, 3, 1, 2), b.cuda(), pool, act, w_clast=wp)
    assert float((got.cpu() - want).abs().max()) < 1e-13 * scale


def _im2col_ref(x, k, clast):
    """col[(b, ho, wo)][(ci, i, j) | (i, j, ci)] of the periodic conv (include/l2q.h)."""
    nb, C = x.shape[:2]
    col = F.unfold(_ppad(x, k), k).transpose(1, 2).reshape(-1, C * k * k)
    if clast:
        col = col.reshape(-1, C, k, k).permute(0, 2, 3, 1).reshape(-1, C * k * k)
    return col


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dims', [(3, 2, 4, 6, 5, 8), (2, 8, 6, 6, 3, 16), (1, 3, 2, 3, 3, 5),
                                  (2, 5, 7, 8, 6, 20), (4, 6, 5, 7, 1, 40)])
def test_im2col_col2im_f64(layout, dims):
    """l2q_im2col_periodic_f64 against torch's unfold, l2q_col2im_periodic_f64 against torch.autograd
    of that unfold (its adjoint)."""
    from l2hmc import native as N
    nb, C, H, W, k, _ = dims
    x, _, _ = _data(dims, seed=7)
    clast = layout == 'nhwc'
    strides = (C * H * W, H * W, W, 1) if layout == 'nchw' else (H * W * C, 1, W * C, C)
    M, Kc = nb * (H + k - 1) * (W + k - 1), C * k * k
    col = torch.empty(M, Kc, device='cuda')
    N.call('l2q_im2col_periodic_f64', _xin(x, layout), *strides, nb, C, H, W, k, int(clast), col)
    assert torch.equal(col.cpu(), _im2col_ref(x, k, clast))
    g = torch.Generator().manual_seed(8)
    dcol = torch.randn(M, Kc, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    (want,) = torch.autograd.grad(_im2col_ref(xr, k, clast), xr, dcol)
    if layout == 'nhwc':
        want = want.permute(0, 2, 3, 1)
    dx = torch.empty(want.shape, device='cuda')
    N.call('l2q_col2im_periodic_f64', dcol.cuda(), *strides, nb, C, H, W, k, int(clast), dx)
    assert float((dx.cpu() - want).abs().max()) < 1e-13 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize('act', [None, 'tanh', 'relu', 'leaky_relu', 'elu'])
@pytest.mark.parametrize('shape,pool', [((3, 6, 5, 4), 2), ((2, 7, 9, 3), 3), ((2, 4, 4, 8), 2)])
def test_maxpool_act_nhwc_bwd_f64(shape, pool, act):
    """l2q_maxpool_act_nhwc_bwd_f64 against torch.autograd of MaxPool2d + activation (floor mode: the
    rows / columns the pool drops get zero)."""
    from l2hmc import native as N
    nb, H, W, C = shape
    g = torch.Generator().manual_seed(9)
    y = torch.randn(nb, H, W, C, generator=g, dtype=torch.float64)
    Ho, Wo = H // pool, W // pool
    dout = torch.randn(nb, Ho, Wo, C, generator=g, dtype=torch.float64)
    yr = y.clone().requires_grad_(True)
    o = _act(F.max_pool2d(yr.permute(0, 3, 1, 2), pool), act).permute(0, 2, 3, 1)
    (want,) = torch.autograd.grad(o, yr, dout)
    out = torch.empty(nb, Ho, Wo, C, device='cuda')
    N.call('l2q_maxpool_act_nhwc_f64', y.cuda(), nb, H, W, C, pool, N.ACT[act], out)
    assert float((out.cpu() - o.detach()).abs().max()) < 1e-14
    din = torch.empty_like(y, device='cuda')
    N.call('l2q_maxpool_act_nhwc_bwd_f64', dout.cuda(), out, y.cuda(), nb, H, W, C, pool, N.ACT[act], din)
    assert float((din.cpu() - want).abs().max()) < 1e-13 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dims,pool,act', [((3, 2, 4, 6, 3, 8), 2, 'leaky_relu'),
                                           ((2, 8, 6, 6, 2, 16), 1, 'tanh'),
                                           ((2, 4, 5, 4, 2, 70), 2, 'relu')])
def test_conv_layer_backward_f64(layout, dims, pool, act):
    """One conv layer's tape in fp64 (ops.conv2d_periodic_gemm_train / _bwd: im2col_f64, GEMM,
    maxpool_act_nhwc_bwd_f64 or act_bwd, col2im_f64) against torch.autograd of the same layer."""
    from l2hmc import _ops as ops
    x, w, b = _data(dims, seed=13)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    want = _conv_ref(xr, wr, br, pool, act)
    g = torch.Generator().manual_seed(14)
    dout = torch.randn(want.shape, generator=g, dtype=torch.float64)
    dx_w, dw_w, db_w = torch.autograd.grad(want, (xr, wr, br), dout)
    out, ctx = ops.conv2d_periodic_gemm_train(_xin(x, layout), layout, w.cuda(), b.cuda(), pool, act)
    assert float((out.cpu() - want.detach()).abs().max()) < 1e-13 * max(1.0, float(want.abs().max()))
    dw, db = torch.zeros_like(w, device='cuda'), torch.zeros_like(b, device='cuda')
    dx = ops.conv2d_periodic_gemm_bwd(ctx, dout.cuda(), w.cuda(), dw, db)
    if layout == 'nhwc':
        dx_w = dx_w.permute(0, 2, 3, 1)
    for got, ref in ((dx, dx_w), (dw, dw_w), (db, db_w)):
        assert got.dtype == torch.float64
        assert float((got.cpu() - ref).abs().max()) < 1e-12 * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------ sampler vs the reference
def test_u1_conv_f64_trajectory(golden):
    """vnet / xnet outputs, the sub-updates, plain HMC and the merged L2HMC trajectory of the fp64 conv
    network against the reference in float64 (the way test_dynamics_gpu.py::test_u1_trajectories
    checks u1_conv in fp32), at fp64 tolerances."""
    from l2hmc.dynamics.pytorch.dynamics import State
    from l2hmc.network.pytorch.network import ConvStack
    g = golden('u1_conv_f64')
    dyn, lat = helpers.build_u1_dynamics(g)
    stacks = [m for m in dyn.modules() if isinstance(m, ConvStack)]
    assert stacks and all(p.dtype == torch.float64 for m in stacks for p in m.parameters())
    beta = torch.tensor(float(g['beta']))
    x = dev(g['x'])
    nb = x.shape[0]
    assert err(host(lat.action(x, beta)), g['action']) < 1e-10
    assert err(host(lat.grad_action(x, beta)), g['force']) < 1e-11
    v = dev(g['normals'].reshape(nb, -1))
    f = dyn.grad_potential(x, beta)
    s, t, q = dyn._call_vnet(0, (x, f))
    assert s.dtype == torch.float64
    assert max(err(host(s), g['vnet_s']), err(host(t), g['vnet_t']), err(host(q), g['vnet_q'])) < 1e-10
    st, ld = dyn._update_v_fwd(0, State(x, v, beta))
    assert err(host(st.v), g['v_fwd']) < 1e-10 and err(host(ld), g['logdet_v_fwd']) < 1e-10
    m0, mb0 = dyn._get_mask(0)
    xm = dyn.unflatten(m0.cuda()) * x
    s, t, q = dyn._call_xnet(0, (xm, v), first=True)
    assert max(err(host(s), g['xnet_s']), err(host(t), g['xnet_t']), err(host(q), g['xnet_q'])) < 1e-10
    st, ld = dyn._update_x_fwd(0, State(x, v, beta), m0, first=True)
    d = np.abs(np.angle(np.exp(1j * (host(st.x) - g['x_fwd']))))
    assert d.max() < 1e-10 and err(host(ld), g['logdet_x_fwd']) < 1e-10
    st, ld = dyn._update_x_bwd(0, State(x, v, beta), mb0, first=False)
    d = np.abs(np.angle(np.exp(1j * (host(st.x) - g['x_bwd']))))
    assert d.max() < 1e-10 and err(host(ld), g['logdet_x_bwd']) < 1e-10
    # plain HMC
    dyn._inject = {'normals': g['hmc_normals'], 'u': g['hmc_u']}
    xo, m = dyn.apply_transition_hmc((x, beta), eps=float(g['hmc_eps']), nleapfrog=int(g['hmc_nleapfrog']))
    assert err(host(m['energy']), g['hmc_energy']) < 1e-9
    assert np.array_equal(host(m['acc_mask']), g['hmc_acc_mask'])
    # merged L2HMC trajectory
    dyn._inject = {'normals': g['normals'], 'u': g['u']}
    xo, m = dyn((x, beta))
    assert err(host(m['energy']), g['energy']) < 1e-9
    assert err(host(m['sumlogdet']), g['sumlogdet']) < 1e-9
    assert err(host(m['logdet']), g['logdet']) < 1e-9
    assert err(host(m['acc']), g['acc']) < 1e-9
    assert np.array_equal(host(m['acc_mask']), g['acc_mask'])      # bit-exact accept / reject
    d = np.abs(np.angle(np.exp(1j * (host(xo) - g['x_out'].reshape(nb, -1)))))
    assert d.max() < 1e-9


def test_u1_conv_f64_auto_graph_equals_eager(golden):
    """The same eval-mode trajectory four times at one shape: the third call captures it into a HIP graph
    (Dynamics.auto_graph_after = 3), the third and fourth replay it; with the same device seed every
    replay equals the eager trajectory bit for bit (the fp64 conv kernels allocate nothing and do not
    synchronise inside the captured region)."""
    g = golden('u1_conv_f64')
    dyn, lat = helpers.build_u1_dynamics(g, verbose=False)
    dyn.eval()
    x, beta = dev(g['x']), float(g['beta'])
    dyn.auto_graph = False
    torch.cuda.manual_seed(21)
    xo_e, m_e = dyn((x, beta))
    dyn.auto_graph = True
    assert dyn.auto_graph_after == 3 and not dyn._graphs
    outs = []
    for i in range(4):
        torch.cuda.manual_seed(21)
        outs.append(dyn((x, beta)))
        assert len(dyn._graphs) == (1 if i >= 2 else 0), i
    for xo, m in outs:
        assert torch.equal(xo, xo_e) and torch.equal(m['acc'], m_e['acc'])
        assert torch.equal(m['acc_mask'], m_e['acc_mask'])
    assert bool(torch.isfinite(xo_e).all())
    dyn._graphs.clear()                          # the captured graphs go with this test
    dyn.auto_graph = False


# ------------------------------------------------------------------ training step vs the reference
@pytest.mark.parametrize('autograd', [False, True], ids=['trainer', 'autograd'])
def test_train_step_matches_reference_conv_f64(autograd, golden):
    """The fp64 conv network's training step (forward tape, reverse sweep, Adam) against the reference's
    float64 gradients, at the tightness of the dense u1_train_f64 cases."""
    g = train_fixture(golden)
    dyn, lat, loss_fn = helpers.build_u1_train_dynamics(g)
    out = helpers.check_train_step(g, dyn, loss_fn, rtol=1e-9, atol_rel=1e-6, autograd=autograd)
    assert out['grad_rel'] < 1e-7, out
    assert out['param_abs'] < 1e-7, out


# ------------------------------------------------------------------ the reference's CLI
def test_cli_u1_float64_default_conv():
    """`python -m l2hmc precision=float64` with the default conv network (conf/conv/default.yaml), run the
    way a user runs it (a process of its own): training and evaluation finish with finite loss and
    acceptance."""
    import json
    import os
    import subprocess
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'l2hmc-qcd_amd')
    r = subprocess.run([sys.executable, '-m', 'l2hmc', 'mode=test', 'precision=float64', 'dynamics.nchains=16',
                        'dynamics.latvolume=[8,8]', 'steps.nera=1', 'steps.nepoch=2', 'steps.test=2', 'seed=3'],
                       cwd=pkg, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert {'train', 'eval', 'hmc'} <= set(out)
    assert out['train']['steps'] == 2 and np.isfinite(out['train']['loss_last'])
    assert np.isfinite(out['eval']['loss_last']) and 0.0 <= out['eval']['acc_mean'] <= 1.0
    assert out['eval']['steps'] == 2
