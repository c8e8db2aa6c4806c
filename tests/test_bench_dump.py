"""bench.py --dump-outputs (``bench.dump_outputs``) on host tensors: which files it writes, in which dtype and
shape, the seeded sample of a large output, and that two calls on the same outputs write the same bytes."""
import os

import numpy as np
import pytest
import torch

import bench
from l2hmc.dynamics.pytorch.dynamics import MonteCarloStates, State


def _outputs():
    g = torch.Generator().manual_seed(3)
    nb, n = 4, bench.DUMP_SAMPLE // 4 + 5          # x: 2 * nb * n float64 values, more than DUMP_SAMPLE
    x = torch.complex(torch.randn(nb, n, dtype=torch.float64, generator=g),
                      torch.randn(nb, n, dtype=torch.float64, generator=g))
    small = torch.randn(nb, 3, dtype=torch.complex128, generator=g)
    lazy = State(x=lambda: small * 2, v=lambda: small * 3, beta=torch.tensor(6.0), xshape=small.shape)
    plain = State(x=small, v=small + 1, beta=torch.tensor(6.0))
    metrics = {'acc': torch.rand(nb, dtype=torch.float64, generator=g),
               'acc_mask': torch.ones(nb, dtype=torch.float32),
               'half': torch.full((nb,), 0.5, dtype=torch.float16),
               'bf': torch.full((nb,), 0.25, dtype=torch.bfloat16),
               'count': torch.arange(nb),
               'loss': 1.25, 'step_skipped': False,
               'mc_states': MonteCarloStates(init=plain, proposed=lazy, out=plain),
               '_native': (torch.zeros(1),), 'note': 'not an array'}
    return x, metrics


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_files_dtypes_and_sample(tmp_path):
    x, metrics = _outputs()
    bench.dump_outputs(str(tmp_path / 'a'), (x, metrics))
    got = _read(tmp_path / 'a')
    want = {'x', 'acc', 'acc_mask', 'half', 'bf', 'count', 'loss', 'step_skipped'} | {
        f'mc_states.{s}.{f}' for s in ('init', 'proposed', 'out') for f in ('x', 'v')}
    assert set(got) == want                     # '_'-prefixed keys and non-numeric values are left out
    for k in ('acc_mask', 'half', 'bf'):
        assert got[k].dtype == np.float32
    for k in want - {'acc_mask', 'half', 'bf'}:
        assert got[k].dtype == np.float64
    assert got['loss'].shape == () and float(got['loss']) == 1.25
    assert float(got['step_skipped']) == 0.0
    np.testing.assert_array_equal(got['count'], np.arange(4.0))
    np.testing.assert_array_equal(got['half'], np.full(4, 0.5, np.float32))
    # complex -> trailing (re, im) axis; the lazy proposed state is formed
    small = metrics['mc_states'].init.x
    np.testing.assert_array_equal(got['mc_states.init.x'], torch.view_as_real(small).numpy())
    np.testing.assert_array_equal(got['mc_states.proposed.x'], torch.view_as_real(small * 2).numpy())
    np.testing.assert_array_equal(got['mc_states.proposed.v'], torch.view_as_real(small * 3).numpy())
    # x is larger than DUMP_SAMPLE: the values of the flattened (re, im) view at sorted indices drawn with seed 0
    flat = torch.view_as_real(x).reshape(-1).numpy()
    idx = np.sort(np.random.default_rng(0).choice(flat.size, bench.DUMP_SAMPLE, replace=False))
    assert got['x'].shape == (bench.DUMP_SAMPLE,)
    np.testing.assert_array_equal(got['x'], flat[idx])
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_MAX_BYTES


def test_dump_outputs_same_bytes_twice(tmp_path):
    bench.dump_outputs(str(tmp_path / 'a'), _outputs())
    bench.dump_outputs(str(tmp_path / 'b'), _outputs())
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == sorted(os.listdir(tmp_path / 'b'))
    for n in names:
        assert (tmp_path / 'a' / n).read_bytes() == (tmp_path / 'b' / n).read_bytes(), n


def test_dump_outputs_refuses_more_than_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 1 << 20)
    with pytest.raises(RuntimeError, match='exceed'):
        bench.dump_outputs(str(tmp_path / 'a'), _outputs())
    assert not (tmp_path / 'a').exists()            # nothing written when the cap is exceeded
