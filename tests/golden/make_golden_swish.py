#!/usr/bin/env python3
"""Golden training-step vectors with `activation_fn=swish` from the REAL reference: the conv stack in
float32 and float64, and the mixed-precision step (fp16 with the conv stack, bf16 dense).  Every case is
make_golden_train.train_case at the shapes of its leaky_relu / tanh twin with the activation swapped.

    bash tests/golden/setup_reference_env.sh
    PYTHONPATH=/tmp/oracle_stubs:/tmp/oracle/src python3 tests/golden/make_golden_swish.py f32
    PYTHONPATH=/tmp/oracle_stubs:/tmp/oracle/src python3 tests/golden/make_golden_swish.py half
    PYTHONPATH=/tmp/oracle_stubs:/tmp/oracle/src python3 tests/golden/make_golden_swish.py f64

One invocation per precision: make_golden_train fixes the default dtype when it is imported (the
reference captures it in module-level constants).  The conv config has one convolution without an
activation (the first), one activated layer without pooling and one activated, pooled layer, so both
swish backward kernels of the conv stack are on the path.  The float64 fixture is compacted like its
twin (make_golden_f64conv.compact_train: the updated parameters are one Adam step of the stored ones).

Seeds: 340 for the fp32 / fp64 conv case (the twin's seed); 720 and 740 for the 16-bit cases (new cases,
their own seeds; train_case then picks the first draw whose accept margin is at least 0.05).
"""
import os
import sys

import torch

OUT = os.path.dirname(os.path.abspath(__file__))
WHICH = sys.argv[1] if len(sys.argv) > 1 else 'f32'
assert WHICH in ('f32', 'half', 'f64'), WHICH
CONV = {'filters': [2, 3, 4], 'sizes': [3, 2, 2], 'pool': [2, 2, 2]}

sys.path.insert(0, OUT)
if WHICH == 'f64':
    # make_golden_f64conv sets the float64 default dtype, then imports make_golden_train in its f64 branch
    import make_golden_f64conv as f64c  # noqa: E402
    mgt = f64c.mgt
else:
    sys.argv = [sys.argv[0], WHICH]
    import make_golden_train as mgt  # noqa: E402  (imports the reference)
cfgs = mgt.cfgs


if __name__ == '__main__':
    lc = cfgs.LossConfig(use_mixed_loss=True, charge_weight=0.01)
    if WHICH == 'f32':
        assert torch.get_default_dtype() == torch.float32
        mgt.train_case('u1_train_swish_conv', (4, 6), 5, 2, [8, 6], 'swish', CONV, beta=2.5, seed=340,
                       bn=True, loss_cfg=lc)
    elif WHICH == 'half':
        assert torch.get_default_dtype() == torch.float32
        mgt.train_case('u1_train_swish_fp16_conv', (4, 6), 5, 2, [8, 6], 'swish', CONV, beta=2.5, seed=720,
                       bn=False, loss_cfg=lc, half=torch.float16, init_scale=16.0)
        mgt.train_case('u1_train_swish_bf16', (4, 6), 5, 3, [8], 'swish', None, beta=3.0, seed=740,
                       bn=False, loss_cfg=lc, half=torch.bfloat16)
    else:
        assert torch.get_default_dtype() == torch.float64
        mgt.train_case('u1_train_swish_conv_f64', (4, 6), 5, 2, [8, 6], 'swish', CONV, beta=2.5, seed=340,
                       bn=True, loss_cfg=lc)
        f64c.compact_train('u1_train_swish_conv_f64')
