"""CPU tier of the drop-in boundary of the loop observables: the three exports of csrc/su3_loops.hip exist and refuse
bad arguments with an error text before any HIP call, and the Python surface on top of them is present."""
import inspect

import pytest
import torch


def test_loops_symbols_and_argument_errors():
    from l2hmc import native
    lib = native.load()
    for name in ('l2q_su3_line_extend', 'l2q_su3_loop_reduce', 'l2q_su3_polyakov'):
        assert hasattr(lib, name) and name in native.SIGNATURES
    # (addresses are never dereferenced: every check below comes before any HIP call)
    x, a, b, o, w = 4096, 8192, 12288, 16384, 20480

    def bad(rc, text):
        assert rc == -1 and text in lib.l2q_last_error(), (rc, lib.l2q_last_error())
    bad(lib.l2q_su3_line_extend(None, x, 1, o, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(lib.l2q_su3_line_extend(a, None, 1, o, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(lib.l2q_su3_line_extend(a, x, 1, None, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(lib.l2q_su3_line_extend(a, x, 1, o, 0, 2, 2, 2, 2, None), b'size')
    bad(lib.l2q_su3_line_extend(a, x, 1, o, 1, 2, 2, 0, 2, None), b'size')
    bad(lib.l2q_su3_line_extend(a, x, -1, o, 1, 2, 2, 2, 2, None), b'negative shift')
    bad(lib.l2q_su3_line_extend(a, x, 1, x, 1, 2, 2, 2, 2, None), b'alias')
    bad(lib.l2q_su3_loop_reduce(None, 1, b, 1, o, 1, 2, 2, 2, 2, w, 1 << 20, None), b'null pointer')
    bad(lib.l2q_su3_loop_reduce(a, 1, None, 1, o, 1, 2, 2, 2, 2, w, 1 << 20, None), b'null pointer')
    bad(lib.l2q_su3_loop_reduce(a, 1, b, 1, None, 1, 2, 2, 2, 2, w, 1 << 20, None), b'null pointer')
    bad(lib.l2q_su3_loop_reduce(a, 1, b, 1, o, 1, 2, 2, 2, 2, None, 1 << 20, None), b'null pointer')
    bad(lib.l2q_su3_loop_reduce(a, 0, b, 1, o, 1, 2, 2, 2, 2, w, 1 << 20, None), b'>= 1')
    bad(lib.l2q_su3_loop_reduce(a, 1, b, 0, o, 1, 2, 2, 2, 2, w, 1 << 20, None), b'>= 1')
    bad(lib.l2q_su3_loop_reduce(a, 1, b, 1, o, 1, 2, -2, 2, 2, w, 1 << 20, None), b'size')
    bad(lib.l2q_su3_polyakov(None, 0, o, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(lib.l2q_su3_polyakov(x, 0, None, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(lib.l2q_su3_polyakov(x, 4, o, 1, 2, 2, 2, 2, None), b'mu')
    bad(lib.l2q_su3_polyakov(x, -1, o, 1, 2, 2, 2, 2, None), b'mu')
    bad(lib.l2q_su3_polyakov(x, 0, o, 0, 2, 2, 2, 2, None), b'size')
    # the workspace of 24 sums per 256-site block: 6 x the per-pair size that l2q_reduce_ws_bytes counts
    assert lib.l2q_su3_loop_reduce(a, 1, b, 1, o, 3, 4, 4, 4, 5, w, 3 * 2 * 24 * 8 - 1, None) == -2      # L2Q_ESHAPE
    assert b'workspace' in lib.l2q_last_error()
    assert 6 * lib.l2q_reduce_ws_bytes(3, 4 * 4 * 4 * 5) >= 3 * 2 * 24 * 8


def test_loops_python_surface():
    from l2hmc import _ops as ops
    from l2hmc.lattice.su3.pytorch import lattice as lsu3
    for name in ('su3_line_extend_n', 'su3_loop_sums_n', 'su3_polyakov_n'):
        assert callable(getattr(ops, name)), name
    for name in ('wilson_loop_sums_n', 'wilson_loop_table', 'polyakov_loops', 'polyakov', 'polyakov_correlator',
                 'polyakov_metrics'):
        assert callable(getattr(lsu3.LatticeSU3, name)), name
    assert callable(lsu3.creutz_ratios) and callable(lsu3.static_potential)
    sig = inspect.signature(lsu3.LatticeSU3.wilson_loop_table)
    assert list(sig.parameters) == ['self', 'x', 'rmax', 'tmax', 'time_dir'] and sig.parameters['time_dir'].default == 0
    for name in ('polyakov_loops', 'polyakov', 'polyakov_correlator'):
        assert inspect.signature(getattr(lsu3.LatticeSU3, name)).parameters['mu'].default == 0
    # what raises before any kernel runs
    lat = lsu3.LatticeSU3(1, [4, 2, 3, 5])
    x = torch.zeros(1, 4, 4, 2, 3, 5, 3, 3, dtype=torch.complex128)
    for rmax, tmax, td in ((0, 1, 0), (1, 0, 0), (3, 1, 0), (2, 5, 0), (1, 3, 1), (4, 1, 1), (3, 1, None),
                           (1, 3, None), (1, 1, 4)):
        with pytest.raises(ValueError):
            lat.wilson_loop_table(x, rmax, tmax, time_dir=td)
    assert lat._loop_extents(0) == (2, 4) and lat._loop_extents(1) == (3, 2) and lat._loop_extents(None) == (2, 2)
    for name in ('wilson_loop_table', 'polyakov_loops', 'polyakov', 'polyakov_correlator', 'polyakov_metrics'):
        args = (2, 2) if name == 'wilson_loop_table' else ()
        with pytest.raises(RuntimeError):
            getattr(lat, name)(x.clone().requires_grad_(True), *args)
    with pytest.raises(RuntimeError):
        lat.wilson_loop_sums_n(torch.zeros(1, 4, 9, 120, dtype=torch.complex128).requires_grad_(True), 2, 2)
