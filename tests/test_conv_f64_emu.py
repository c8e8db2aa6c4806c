"""CPU test of the fp64 conv stack's training step (host side: tape, reverse sweep, Adam) against the
reference's float64 gradient fixture, with the libl2q.so entry points replaced by the torch
restatement in tests/emu_native.py; the fp64 conv entry points are routed to its dtype-generic fp32
restatements.  The kernels themselves are checked on the GPU (test_conv_f64_gpu.py)."""
import pytest
import torch

import emu_native
import helpers
from f64conv_helpers import install_emu_f64, train_fixture


@pytest.mark.skipif(torch.cuda.is_available(), reason='host-logic test for the CPU container')
@pytest.mark.parametrize('autograd', [False, True], ids=['trainer', 'autograd'])
def test_train_step_host_logic_conv_f64(autograd, golden, monkeypatch):
    torch.set_default_dtype(torch.float64)
    g = train_fixture(golden)
    emu_native.install(monkeypatch)
    install_emu_f64(monkeypatch)
    dyn, lat, loss_fn = helpers.build_u1_train_dynamics(g)
    out = helpers.check_train_step(g, dyn, loss_fn, rtol=1e-9, atol_rel=1e-6, autograd=autograd)
    assert out['grad_rel'] < 1e-7, out
    assert out['param_abs'] < 1e-7, out


@pytest.mark.skipif(torch.cuda.is_available(), reason='host-logic test for the CPU container')
def test_conv_ops_refuse_other_and_mixed_dtypes(monkeypatch):
    """fp32 and fp64 pass, any other dtype and an input / weight dtype mismatch are refused (no
    silent casts) before anything is launched."""
    from l2hmc import _ops as ops
    from l2hmc import native as N
    emu_native.install(monkeypatch)
    install_emu_f64(monkeypatch)
    x = torch.randn(2, 4, 5, 6, dtype=torch.float64)
    w = torch.randn(3, 4, 3, 3, dtype=torch.float64)
    b = torch.randn(3, dtype=torch.float64)
    y = ops.conv2d_periodic_gemm(x, 'nchw', w, b, 2, 'relu')
    assert y.dtype == torch.float64 and y.shape == (2, 3, 4, 3)
    y2, ctx = ops.conv2d_periodic_gemm_train(x, 'nchw', w, b, 2, 'relu')
    assert y2.dtype == torch.float64 and torch.allclose(y2, y, rtol=0, atol=1e-13)
    dw, db = torch.zeros_like(w), torch.zeros_like(b)
    dx = ops.conv2d_periodic_gemm_bwd(ctx, torch.ones_like(y2), w, dw, db)
    assert dx.dtype == torch.float64 and dx.shape == x.shape
    assert ops.nchw_to_nhwc_pad(x, 4).dtype == torch.float64
    with pytest.raises(N.L2QError, match='dtype mismatch'):
        ops.conv2d_periodic_gemm(x, 'nchw', w.float(), b, 1, None)
    with pytest.raises(N.L2QError, match='dtype mismatch'):
        ops.conv2d_periodic_gemm_train(x.float(), 'nchw', w, b.float(), 1, None)
    with pytest.raises(N.L2QError, match='dtype mismatch'):
        ops.conv2d_periodic_gemm_bwd(ctx, torch.ones_like(y2).float(), w, dw, db)
    with pytest.raises(N.L2QError, match='float32 or float64'):
        ops.conv2d_periodic_gemm(x.half(), 'nchw', w.half(), b.half(), 1, None)
    with pytest.raises(N.L2QError, match='float32 or float64'):
        ops.nchw_to_nhwc_pad(x.bfloat16(), 4)
    with pytest.raises(N.L2QError, match='fp32 containers'):
        ops.conv2d_periodic_gemm_train(x, 'nchw', w, b, 1, None, half=torch.float16)
