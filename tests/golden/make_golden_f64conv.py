#!/usr/bin/env python3
"""Golden vectors of the U(1) conv stack in float64 (`precision=float64` with a conv network) from the
REAL reference: the sampling case of make_golden.u1_case and the training step of
make_golden_train.train_case at the shapes of their fp32 conv twins (u1_conv, u1_train_conv).

    bash tests/golden/setup_reference_env.sh
    PYTHONPATH=/tmp/oracle_stubs:/tmp/oracle/src python3 tests/golden/make_golden_f64conv.py

The default dtype is float64 before the reference is imported (it captures the default dtype in
module-level constants at import, see make_golden.py).

Size: in float64 the training fixture holds 0.87 MB of incompressible parameters, gradients and
updated parameters.  The updated *parameters* (`sd1.<param>`) are one torch.optim.Adam step of
`sd.<param>` with the stored gradients, so they are checked here against exactly that step and then
dropped (`sd1_params='adam(sd, grad, lr)'`); the tests re-run the step (tests/f64conv_helpers.py:
adam_sd1).  The updated buffers (BatchNorm running statistics) stay in the file.
"""
import os
import sys

import numpy as np
import torch

torch.set_default_dtype(torch.float64)
OUT = os.path.dirname(os.path.abspath(__file__))
sys.argv = [sys.argv[0], 'f64']           # make_golden_train's float64 branch (imports make_golden)
sys.path.insert(0, OUT)
sys.path.insert(1, os.path.dirname(OUT))
import make_golden_train as mgt  # noqa: E402  (imports the reference, sets nothing else)
from f64conv_helpers import adam_sd1  # noqa: E402

mg = mgt.mg
cfgs = mgt.cfgs
CONV = {'filters': [2, 3, 4], 'sizes': [3, 2, 2], 'pool': [2, 2, 2]}


def compact_train(name):
    path = os.path.join(OUT, name + '.npz')
    g = dict(np.load(path))
    rebuilt = adam_sd1(g)
    worst = max(float(np.abs(g[k] - v).max()) for k, v in rebuilt.items())
    assert worst < 1e-15, f'{name}: sd1 is not one Adam step of sd (|diff| {worst:.3e})'
    for k in rebuilt:
        del g[k]
    g['sd1_params'] = 'adam(sd, grad, lr)'
    np.savez_compressed(path, **g)
    print(f'  {name}: {len(rebuilt)} updated parameters = Adam(sd, grad) to {worst:.1e}, dropped; '
          f'{os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    assert torch.get_default_dtype() == torch.float64
    mg.u1_case('u1_conv_f64', (4, 6), 3, 2, [8, 6], 'leaky_relu', CONV,
               beta=2.5, seed=100, bn=True, dropout=0.2)
    mgt.train_case('u1_train_conv_f64', (4, 6), 5, 2, [8, 6], 'leaky_relu', CONV, beta=2.5,
                   seed=340, bn=True, loss_cfg=cfgs.LossConfig(use_mixed_loss=True, charge_weight=0.01))
    compact_train('u1_train_conv_f64')
