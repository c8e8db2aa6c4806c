"""Training with `activation_fn=swish` through a conv stack and in half precision on the MI355X: the
three kernels the path adds or extends -- l2q_maxpool_act_nhwc_bwd_* with swish, l2q_act_bwd_sums,
l2q_act_fwd_r16 -- against torch on the CPU, the training step against the reference's swish fixtures
(tests/golden/make_golden_swish.py) on both routes, and the reference's CLI with swish end to end."""
import numpy as np
import pytest
import torch

import helpers
from f64conv_helpers import train_fixture

pytestmark = pytest.mark.gpu

F = torch.nn.functional
DT = {4: torch.float32, 8: torch.float64}
TOL = {4: 2e-5, 8: 1e-12}                    # test_train_gpu.py's per-element tolerances
SWISH = 5


@pytest.fixture(autouse=True)
def _sync():
    torch.set_default_dtype(torch.float32)       # (conftest puts the previous default back)
    yield
    # every launch of this module completes inside the test that made it
    torch.cuda.synchronize()


# ------------------------------------------------------------------ (a) pooled swish backward
def _pool_swish_want(y, dout, pool):
    """torch autograd on the CPU in fp64: MaxPool2d(pool) then silu, NHWC in and out."""
    yr = y.double().clone().requires_grad_(True)
    o = F.silu(F.max_pool2d(yr.permute(0, 3, 1, 2), pool)).permute(0, 2, 3, 1)
    (want,) = torch.autograd.grad(o, yr, dout.double())
    return want


@pytest.mark.parametrize('esz', [4, 8])
@pytest.mark.parametrize('shape,pool', [((3, 7, 5, 3), 2), ((2, 7, 10, 5), 3), ((2, 6, 9, 6), 2),
                                        ((2, 8, 11, 7), 3)])
def test_maxpool_swish_bwd(shape, pool, esz):
    """l2q_maxpool_act_nhwc_bwd_{f32,f64} with swish: the derivative at the window maximum of `in`; H, W
    not divisible by the pool (the dropped rows / columns get zero), C not a multiple of 4; `out` is not read
    (a buffer of NaN is passed).  fp64 at the tolerance of test_maxpool_act_nhwc_bwd_f64, fp32 at that of
    test_train_gpu.py::test_maxpool_bwd."""
    from l2hmc import native as N
    nb, H, W, C = shape
    dt = DT[esz]
    g = torch.Generator().manual_seed(9)
    y = (2.0 * torch.randn(nb, H, W, C, generator=g, dtype=torch.float64)).to(dt)
    Ho, Wo = H // pool, W // pool
    dout = torch.randn(nb, Ho, Wo, C, generator=g, dtype=torch.float64).to(dt)
    want = _pool_swish_want(y, dout, pool)
    out = torch.full((nb, Ho, Wo, C), float('nan'), dtype=dt, device='cuda')
    din = torch.empty_like(y, device='cuda')
    N.call('l2q_maxpool_act_nhwc_bwd_' + ('f32' if esz == 4 else 'f64'), dout.cuda(), out, y.cuda(), nb, H, W, C,
           pool, SWISH, din)
    err = float((din.cpu().double() - want).abs().max())
    scale = max(1.0, float(want.abs().max()))
    print(f'maxpool swish bwd esz {esz} {shape} pool {pool}: err {err:.3e} scale {scale:.3e}')
    assert err <= (1e-5 if esz == 4 else 1e-13) * scale
    # the forward kernel and this one see the same maximum
    fwd = torch.empty((nb, Ho, Wo, C), dtype=dt, device='cuda')
    N.call('l2q_maxpool_act_nhwc_' + ('f32' if esz == 4 else 'f64'), y.cuda(), nb, H, W, C, pool, SWISH, fwd)
    ref = F.silu(F.max_pool2d(y.double().permute(0, 3, 1, 2), pool)).permute(0, 2, 3, 1)
    assert float((fwd.cpu().double() - ref).abs().max()) <= (1e-5 if esz == 4 else 1e-13) * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize('esz', [4, 8])
def test_maxpool_swish_bwd_large_arguments(esz):
    """|z| up to 1e4: exp(-z) overflows for the large negative ones -- the output stays finite, and is 0 where
    torch's gradient is 0."""
    from l2hmc import native as N
    nb, H, W, C, pool = 2, 5, 6, 3, 2
    dt = DT[esz]
    g = torch.Generator().manual_seed(10)
    mag = 10.0 ** (4.0 * torch.rand(nb, H, W, C, generator=g, dtype=torch.float64))
    y = (mag * torch.sign(torch.randn(nb, H, W, C, generator=g, dtype=torch.float64))).to(dt)
    y[0, :2, :2, :] = -torch.abs(y[0, :2, :2, :]) - 1.0e3         # a window whose maximum is large and negative
    Ho, Wo = H // pool, W // pool
    dout = torch.randn(nb, Ho, Wo, C, generator=g, dtype=torch.float64).to(dt)
    want = _pool_swish_want(y, dout, pool)
    out = torch.zeros((nb, Ho, Wo, C), dtype=dt, device='cuda')
    din = torch.empty_like(y, device='cuda')
    N.call('l2q_maxpool_act_nhwc_bwd_' + ('f32' if esz == 4 else 'f64'), dout.cuda(), out, y.cuda(), nb, H, W, C,
           pool, SWISH, din)
    got = din.cpu().double()
    assert bool(torch.isfinite(got).all())
    assert bool((got[want == 0] == 0).all())
    err = float((got - want).abs().max())
    print(f'maxpool swish bwd large |z| esz {esz}: err {err:.3e}, zeros {int((want == 0).sum())}/{want.numel()}')
    assert err <= (1e-5 if esz == 4 else 1e-13) * max(1.0, float(want.abs().max()))


# ------------------------------------------------------------------ (b) act_bwd + bias column sums
@pytest.mark.parametrize('esz', [4, 8])
@pytest.mark.parametrize('N_', [3, 8, 64, 130])
@pytest.mark.parametrize('M,mult', [(301, 20), (2049, 50), (70001, 500)])
def test_act_bwd_sums(M, mult, N_, esz):
    """l2q_act_bwd_sums: dz equals l2q_act_bwd bit for bit; bgrad (accumulated into a non-zero vector)
    against a float64 column sum at the tolerances of test_train_gpu.py::test_mul_axpy_rows_colsum (which
    grow with the number of rows the same way).  M is never a multiple of the row block (64 / 256 rows)."""
    from l2hmc import native as N
    dt = DT[esz]
    g = torch.Generator().manual_seed(77)
    z = (1.5 * torch.randn(M, N_, generator=g, dtype=torch.float64)).to(dt).cuda()
    dy = torch.randn(M, N_, generator=g, dtype=torch.float64).to(dt).cuda()
    b0 = torch.randn(N_, generator=g, dtype=torch.float64).to(dt)
    ws = torch.zeros(int(N.load().l2q_colsum_ws_bytes(M, N_)), dtype=torch.uint8, device='cuda')
    for act in (SWISH, 1):
        y = z if act == SWISH else torch.tanh(z)
        want = torch.empty_like(dy)
        N.call('l2q_act_bwd', dy, y, act, dy.numel(), esz, want)
        dz = torch.empty_like(dy)
        bg = b0.clone().cuda()
        N.call('l2q_act_bwd_sums', dy, y, act, M, N_, esz, dz, bg, ws, ws.numel())
        torch.cuda.synchronize()
        assert torch.equal(dz, want), (act, float((dz - want).abs().max()))
        ref = b0.double() + want.cpu().double().sum(0)
        err = float((bg.cpu().double() - ref).abs().max())
        scale = max(1.0, float(ref.abs().max()))
        assert err <= mult * TOL[esz] * scale, (act, err, scale)
    # in place on dy (what a caller without a use for dy afterwards may do)
    dz = dy.clone()
    bg = torch.zeros(N_, dtype=dt, device='cuda')
    N.call('l2q_act_bwd_sums', dz, z, SWISH, M, N_, esz, dz, bg, ws, ws.numel())
    want = torch.empty_like(dy)
    N.call('l2q_act_bwd', dy, z, SWISH, dy.numel(), esz, want)
    assert torch.equal(dz, want)


def test_act_bwd_sums_unaligned_rows_take_the_scalar_path():
    """A view that starts 4 bytes into an allocation (not 16-byte aligned) with N % 4 == 0: same bits."""
    from l2hmc import native as N
    M, N_ = 513, 16
    g = torch.Generator().manual_seed(78)
    base = torch.randn(2, M * N_ + 1, generator=g).cuda()
    z, dy = base[0, 1:].reshape(M, N_), base[1, 1:].reshape(M, N_)
    assert z.data_ptr() % 16 and z.is_contiguous()
    ws = torch.zeros(int(N.load().l2q_colsum_ws_bytes(M, N_)), dtype=torch.uint8, device='cuda')
    dz, bg = torch.empty(M, N_, device='cuda'), torch.zeros(N_, device='cuda')
    N.call('l2q_act_bwd_sums', dy, z, SWISH, M, N_, 4, dz, bg, ws, ws.numel())
    dz2, bg2 = torch.empty(M, N_, device='cuda'), torch.zeros(N_, device='cuda')
    N.call('l2q_act_bwd_sums', dy.clone(), z.clone(), SWISH, M, N_, 4, dz2, bg2, ws, ws.numel())
    assert torch.equal(dz, dz2)
    ref = dz.cpu().double().sum(0)
    for b in (bg, bg2):
        assert float((b.cpu().double() - ref).abs().max()) <= 50 * TOL[4] * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------ (c) r16(act(r16(x)))
def _ordered(bits16):
    """16-bit float patterns (as int64) -> integers whose difference counts representable values."""
    b = bits16 & 0xffff
    return torch.where(b >= 0x8000, 0x8000 - b, b)


@pytest.mark.parametrize('half', [torch.float16, torch.bfloat16], ids=['fp16', 'bf16'])
def test_act_fwd_r16_all_patterns(half):
    """l2q_act_fwd_r16 with swish over all 65 536 bit patterns of the 16-bit type against torch's CPU silu on
    the 16-bit tensor (the reference arithmetic): infinities and NaN by class, no value further than one
    16-bit ulp away; the count of one-ulp differences is printed (it is recorded, not gated)."""
    from l2hmc import _ops as ops
    bits = torch.arange(-32768, 32768, dtype=torch.int16)
    x16 = bits.view(half)
    want = F.silu(x16)
    x32 = x16.float()
    pad = torch.zeros(3)                       # 65 539 elements: the vector body and a scalar tail
    got32 = ops.act_fwd_r16(torch.cat([x32, pad]).cuda(), 'swish', half).cpu()
    assert bool((got32[65536:] == 0).all())
    got32 = got32[:65536]
    got = got32.to(half)
    assert torch.equal(got.float().nan_to_num(nan=7.0), got32.nan_to_num(nan=7.0))      # 16-bit valued
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.isinf(got), torch.isinf(want))
    fin = torch.isfinite(want)
    assert torch.equal(torch.signbit(got[fin & (want != 0)]), torch.signbit(want[fin & (want != 0)]))
    d = (_ordered(got.view(torch.int16).long()) - _ordered(want.view(torch.int16).long())).abs()[fin]
    n1, nbig = int((d == 1).sum()), int((d > 1).sum())
    print(f'act_fwd_r16 swish {half}: {n1} of {int(fin.sum())} finite results differ from torch by one ulp, '
          f'{nbig} by more')
    assert nbig == 0
    # the vector body and the unaligned / scalar path give the same bits
    shifted = torch.cat([torch.zeros(1), x32]).cuda()[1:]
    assert shifted.data_ptr() % 16
    got_s = ops.act_fwd_r16(shifted, 'swish', half).cpu()
    assert torch.equal(got_s.nan_to_num(nan=7.0), got32.nan_to_num(nan=7.0))


@pytest.mark.parametrize('half', [torch.float16, torch.bfloat16], ids=['fp16', 'bf16'])
@pytest.mark.parametrize('act', [None, 'tanh', 'relu', 'leaky_relu', 'elu', 'swish'])
def test_act_fwd_r16_rounds_like_the_fused_epilogue(act, half):
    """A layer whose activation runs in l2q_act_fwd_r16 gives the bits of the layer with the activation fused
    into l2q_gemm_h's epilogue."""
    from l2hmc import _ops as ops
    g = torch.Generator().manual_seed(5)
    a = torch.randn(37, 24, generator=g).cuda()
    w = (torch.randn(19, 24, generator=g) / 24 ** 0.5).to(half).cuda()
    b = torch.randn(19, generator=g).to(half).float().cuda()
    fused = ops.gemm_h(a, w, b, act=act, out_dtype=torch.float32)
    split = ops.act_fwd_r16(ops.gemm_h(a, w, b, act=None, out_dtype=torch.float32), act, half)
    assert torch.equal(fused, split)


# ------------------------------------------------------------------ one conv layer, torch autograd
@pytest.mark.parametrize('dt', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('pool', [1, 2])
def test_conv_layer_backward_swish(pool, dt):
    """ops.conv2d_periodic_gemm_train / _bwd with swish (pool 1: l2q_act_bwd_sums on the kept pre-activation,
    pool 2: the pooled kernel) against torch.autograd of PeriodicPadding -> Conv2d -> [MaxPool2d] -> silu in
    fp64."""
    from l2hmc import _ops as ops
    nb, C, H, W, k, cout = 3, 4, 5, 6, 2, 6
    g = torch.Generator().manual_seed(13)
    x = torch.randn(nb, C, H, W, generator=g, dtype=torch.float64).to(dt)
    w = (torch.randn(cout, C, k, k, generator=g, dtype=torch.float64) / (C * k * k) ** 0.5).to(dt)
    b = torch.randn(cout, generator=g, dtype=torch.float64).to(dt)
    xr, wr, br = (t.double().clone().requires_grad_(True) for t in (x, w, b))
    p = k - 1
    xp = torch.cat([xr[:, :, -p:, :], xr, xr[:, :, :p, :]], 2)
    xp = torch.cat([xp[:, :, :, -p:], xp, xp[:, :, :, :p]], 3)
    y = F.conv2d(xp, wr, br)
    if pool > 1:
        y = F.max_pool2d(y, pool)
    want = F.silu(y).permute(0, 2, 3, 1)
    dout = torch.randn(want.shape, generator=g, dtype=torch.float64).to(dt)
    dx_w, dw_w, db_w = torch.autograd.grad(want, (xr, wr, br), dout.double())
    tol = 1e-13 if dt == torch.float64 else 2e-5
    out, ctx = ops.conv2d_periodic_gemm_train(x.cuda(), 'nchw', w.cuda(), b.cuda(), pool, 'swish')
    want = want.detach()
    assert float((out.cpu().double() - want).abs().max()) <= tol * max(1.0, float(want.abs().max()))
    dw, db = torch.zeros_like(w, device='cuda'), torch.zeros_like(b, device='cuda')
    dx = ops.conv2d_periodic_gemm_bwd(ctx, dout.cuda(), w.cuda(), dw, db)
    for got, ref in ((dx, dx_w), (dw, dw_w), (db, db_w)):
        assert float((got.cpu().double() - ref).abs().max()) <= 10 * tol * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------ training step vs the reference
@pytest.mark.parametrize('autograd', [False, True], ids=['trainer', 'autograd'])
def test_swish_train_step_matches_reference_conv_f32(autograd, golden):
    g = golden('u1_train_swish_conv')
    dyn, lat, loss_fn = helpers.build_u1_train_dynamics(g)
    out = helpers.check_train_step(g, dyn, loss_fn, rtol=2e-4, atol_rel=1e-3, adam_min_grad=1e-3,
                                   autograd=autograd)
    print('u1_train_swish_conv', autograd, out)
    assert out['grad_rel'] < 2e-2, out
    assert out['param_abs'] < 2e-5, out


@pytest.mark.parametrize('autograd', [False, True], ids=['trainer', 'autograd'])
def test_swish_train_step_matches_reference_conv_f64(autograd, golden):
    torch.set_default_dtype(torch.float64)
    g = train_fixture(golden, 'u1_train_swish_conv_f64')
    dyn, lat, loss_fn = helpers.build_u1_train_dynamics(g)
    out = helpers.check_train_step(g, dyn, loss_fn, rtol=1e-9, atol_rel=1e-6, autograd=autograd)
    print('u1_train_swish_conv_f64', autograd, out)
    assert out['grad_rel'] < 1e-7, out
    assert out['param_abs'] < 1e-7, out


@pytest.mark.parametrize('route', ['trainer', 'autograd'])
@pytest.mark.parametrize('name', ['u1_train_swish_fp16_conv', 'u1_train_swish_bf16'])
def test_swish_half_precision_train_step_matches_reference(name, route, golden):
    """The reference's mixed-precision step with swish: accept masks bit-equal, gradients within twice the
    reference's own 16-bit-vs-fp32 distance, GradScaler's scale equal on the autograd route."""
    g = golden(name)
    out = helpers.check_half_train_step(g, route)
    print(name, route, out)
    helpers.assert_half_train_step(g, name, route, out)


# ------------------------------------------------------------------ the reference's CLI
@pytest.mark.parametrize('extra', [[], ['precision=fp16']], ids=['fp32', 'fp16'])
def test_cli_u1_swish_default_conv(extra):
    """`python -m l2hmc network.activation_fn=swish` with the default conv network, run the way a user runs
    it (a process of its own): three training steps and the evaluation finish with finite loss and
    acceptance."""
    import json
    import os
    import subprocess
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'l2hmc-qcd_amd')
    r = subprocess.run([sys.executable, '-m', 'l2hmc', 'mode=test', 'network.activation_fn=swish',
                        'dynamics.nchains=16', 'dynamics.latvolume=[8,8]', 'steps.nera=1', 'steps.nepoch=3',
                        'steps.test=2', 'seed=3'] + extra,
                       cwd=pkg, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert {'train', 'eval', 'hmc'} <= set(out)
    assert out['train']['steps'] == 3 and np.isfinite(out['train']['loss_last'])
    assert np.isfinite(out['eval']['loss_last']) and 0.0 <= out['eval']['acc_mean'] <= 1.0
    assert out['eval']['steps'] == 2
