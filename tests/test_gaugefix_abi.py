"""CPU tier of the drop-in boundary of the gauge fixing: the three exports of csrc/su3_gaugefix.hip exist, agree with
native.SIGNATURES and refuse bad arguments with an error text before any HIP call, and the Python surface on top of
them is present with its ValueErrors."""
import inspect

import pytest
import torch

NAMES = ('l2q_su3_gaugefix_sweep', 'l2q_su3_gauge_condition', 'l2q_su3_gauge_apply')


def test_gaugefix_symbols_and_signatures():
    import ctypes as C
    from l2hmc import native
    lib = native.load()
    P, I, D, Z = C.c_void_p, C.c_int, C.c_double, C.c_size_t
    want = {'l2q_su3_gaugefix_sweep': (I, [P, P, P, I, I, D, I, I, I, I, I, P]),
            'l2q_su3_gauge_condition': (I, [P, I, P, I, I, I, I, I, P, Z, P]),
            'l2q_su3_gauge_apply': (I, [P, P, P, I, I, I, I, I, P])}
    for name in NAMES:
        assert hasattr(lib, name) and native.SIGNATURES[name] == want[name], name
    header = open(native.os.path.join(native._HERE, '..', '..', 'include', 'l2q.h')).read()
    for name in NAMES:
        assert f'int {name}(' in header, name


def test_gaugefix_argument_errors():
    from l2hmc import native
    lib = native.load()
    swp, cnd, app = (getattr(lib, n) for n in NAMES)
    # (addresses are never dereferenced: every check below comes before any HIP call)
    x, g, a, o, w = 4096, 8192, 12288, 16384, 20480

    def bad(rc, text, code=-1):
        assert rc == code and text in lib.l2q_last_error(), (rc, lib.l2q_last_error())

    def sweep(**kw):
        p = {**dict(xn=x, gn=g, active=a, dirmask=15, parity=0, omega=1.7, nb=1, T=2, X=2, Y=2, Z=2), **kw}
        return swp(p['xn'], p['gn'], p['active'], p['dirmask'], p['parity'], p['omega'], p['nb'], p['T'], p['X'],
                   p['Y'], p['Z'], None)
    bad(sweep(xn=None), b'null pointer')
    bad(sweep(gn=x), b'alias')
    bad(sweep(parity=2), b'parity')
    bad(sweep(parity=-1), b'parity')
    for m in (0, 16, -1, 1, 2, 4, 8):
        bad(sweep(dirmask=m), b'dirmask')
    for om in (0.99, 2.0, 2.5, -1.0, float('inf'), float('nan')):
        bad(sweep(omega=om), b'omega')
    bad(sweep(nb=0), b'size')
    bad(sweep(Y=0), b'size')
    for kw in (dict(T=3), dict(X=5), dict(Y=1), dict(Z=7)):
        bad(sweep(**kw), b'even extents', -2)                                  # L2Q_ESHAPE
    assert b'l2q_su3_gaugefix_sweep' in lib.l2q_last_error()

    def cond(**kw):
        p = {**dict(xn=x, dirmask=14, out=o, nb=3, T=4, X=4, Y=4, Z=5, ws=w, ws_bytes=1 << 20), **kw}
        return cnd(p['xn'], p['dirmask'], p['out'], p['nb'], p['T'], p['X'], p['Y'], p['Z'], p['ws'], p['ws_bytes'],
                   None)
    for kw in (dict(xn=None), dict(out=None), dict(ws=None)):
        bad(cond(**kw), b'null pointer')
    for m in (0, 16, 1, 8):
        bad(cond(dirmask=m), b'dirmask')
    bad(cond(nb=0), b'size')
    bad(cond(T=-2), b'size')
    # two sums per 256-site block: V = 320 is two blocks
    bad(cond(ws_bytes=3 * 2 * 2 * 8 - 1), b'workspace', -2)
    assert lib.l2q_reduce_ws_bytes(3, 320) >= 3 * 2 * 2 * 8

    bad(app(None, g, o, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(app(x, None, o, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(app(x, g, None, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(app(x, g, x, 1, 2, 2, 2, 2, None), b'alias')
    bad(app(x, g, g, 1, 2, 2, 2, 2, None), b'alias')
    bad(app(x, g, o, 0, 2, 2, 2, 2, None), b'size')
    bad(app(x, g, o, 1, 2, 3, 0, 2, None), b'size')


def test_gaugefix_python_surface():
    from l2hmc import _ops as ops
    from l2hmc.lattice.su3.pytorch import lattice as lsu3
    for name in ('su3_gaugefix_sweep_', 'su3_gauge_condition_n', 'su3_gauge_apply_n'):
        assert callable(getattr(ops, name)), name
    assert list(inspect.signature(ops.su3_gaugefix_sweep_).parameters) == ['xn', 'parity', 'dirmask', 'omega', 'lat',
                                                                           'gn', 'active']
    assert list(inspect.signature(ops.su3_gauge_condition_n).parameters) == ['xn', 'dirmask', 'lat']
    assert list(inspect.signature(ops.su3_gauge_apply_n).parameters) == ['xn', 'gn', 'lat']
    p = inspect.signature(lsu3.LatticeSU3.gauge_fix).parameters
    assert list(p) == ['self', 'x', 'gauge', 'time_dir', 'omega', 'tol', 'max_sweeps', 'check_every', 'reunitarize',
                       'return_transform']
    assert [p[k].default for k in list(p)[2:]] == ['landau', 0, None, 1e-12, 10000, 10, True, False]
    pn = inspect.signature(lsu3.LatticeSU3.gauge_fix_n).parameters
    assert list(pn) == ['self', 'xn', *list(p)[2:]] and [pn[k].default for k in list(pn)[2:]] == \
        [p[k].default for k in list(p)[2:]]
    pc = inspect.signature(lsu3.LatticeSU3.gauge_condition).parameters
    assert list(pc) == ['self', 'x', 'gauge', 'time_dir'] and (pc['gauge'].default, pc['time_dir'].default) == \
        ('landau', 0)
    assert list(inspect.signature(lsu3.LatticeSU3.gauge_transform).parameters) == ['self', 'x', 'g']
    assert lsu3.GaugeCondition._fields == ('F', 'theta')
    assert 1.0 <= lsu3.GAUGEFIX_OMEGA < 2.0
    assert lsu3.LatticeSU3._gauge_dirmask('landau', 2, 't') == 15
    assert [lsu3.LatticeSU3._gauge_dirmask('coulomb', t, 't') for t in range(4)] == [14, 13, 11, 7]
    # what raises before any kernel runs
    lat = lsu3.LatticeSU3(1, [2, 2, 2, 4])
    x = torch.zeros(1, 4, 2, 2, 2, 4, 3, 3, dtype=torch.complex128)
    xn = torch.zeros(1, 4, 9, 32, dtype=torch.complex128)
    for kw in (dict(gauge='axial'), dict(gauge=None), dict(time_dir=4), dict(time_dir=-1), dict(time_dir=0.5),
               dict(omega=0.9), dict(omega=2.0), dict(omega=float('nan')), dict(tol=0.0), dict(tol=-1e-12),
               dict(tol=float('nan')), dict(check_every=0), dict(max_sweeps=-1)):
        with pytest.raises(ValueError):
            lat.gauge_fix(x, **kw)
        with pytest.raises(ValueError):
            lat.gauge_fix_n(xn, **kw)
    with pytest.raises(ValueError):
        lat.gauge_fix(x.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        lat.gauge_fix_n(xn.clone().requires_grad_(True))
    odd = lsu3.LatticeSU3(1, [2, 3, 2, 2])
    with pytest.raises(ValueError):
        odd.gauge_fix(torch.zeros(1, 4, 2, 3, 2, 2, 3, 3, dtype=torch.complex128))
    for kw in (dict(gauge='axial'), dict(gauge='coulomb', time_dir=4)):
        with pytest.raises(ValueError):
            lat.gauge_condition(x, **kw)
    with pytest.raises(ValueError):
        lat.gauge_condition(x.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        lat.gauge_transform(x, torch.zeros(1, 2, 2, 2, 2, 3, 3, dtype=torch.complex128))
    with pytest.raises(ValueError):
        lat.gauge_transform(x, torch.zeros(1, 2, 2, 2, 4, 3, 3, dtype=torch.complex128).requires_grad_(True))
