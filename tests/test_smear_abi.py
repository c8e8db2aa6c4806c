"""CPU tier of the drop-in boundary of the link smearing: the four exports of csrc/su3_smear.hip exist, agree with
native.SIGNATURES and the header, and refuse bad arguments with an error text before any HIP call; the Python surface on
top of them is present and raises what it should before any kernel runs."""
import inspect

import pytest
import torch

NAMES = ('l2q_su3_ape_smear', 'l2q_su3_hyp_level1', 'l2q_su3_hyp_level2', 'l2q_su3_hyp_level3')


def test_smear_symbols_and_signatures():
    import ctypes as C
    from l2hmc import native
    lib = native.load()
    P, I, D = C.c_void_p, C.c_int, C.c_double
    want = {'l2q_su3_ape_smear': (I, [P, D, I, P, I, I, I, I, I, P]),
            'l2q_su3_hyp_level1': (I, [P, D, P, I, I, I, I, I, P]),
            'l2q_su3_hyp_level2': (I, [P, P, D, P, I, I, I, I, I, P]),
            'l2q_su3_hyp_level3': (I, [P, P, D, P, I, I, I, I, I, P])}
    for name in NAMES:
        assert hasattr(lib, name) and native.SIGNATURES[name] == want[name], name
    header = open(native.os.path.join(native._HERE, '..', '..', 'include', 'l2q.h')).read()
    flat = ' '.join(header.split())
    for decl in ('int l2q_su3_ape_smear(const void* xn, double alpha, int dirmask, void* out, int nb, int T, int X, int Y, '
                 'int Z, void* stream);',
                 'int l2q_su3_hyp_level1(const void* xn, double alpha3, void* b1, int nb, int T, int X, int Y, int Z, '
                 'void* stream);',
                 'int l2q_su3_hyp_level2(const void* xn, const void* b1, double alpha2, void* b2, int nb, int T, int X, '
                 'int Y, int Z, void* stream);',
                 'int l2q_su3_hyp_level3(const void* xn, const void* b2, double alpha1, void* out, int nb, int T, int X, '
                 'int Y, int Z, void* stream);'):
        assert decl in flat, decl


def test_smear_argument_errors():
    from l2hmc import native
    lib = native.load()
    ape, l1, l2, l3 = (getattr(lib, n) for n in NAMES)
    # (addresses are never dereferenced: every check below comes before any HIP call)
    x, b, o = 4096, 8192, 12288
    nan, inf = float('nan'), float('inf')
    bad_alphas = (-1e-9, 1.0 + 1e-9, 2.0, -1.0, nan, inf, -inf)
    bad_dims = (dict(nb=0), dict(nb=-1), dict(T=0), dict(X=-3), dict(Y=0), dict(Z=0), dict(T=1 << 12, X=1 << 12, Y=8))

    def bad(rc, text, name):
        err = lib.l2q_last_error()
        assert rc == -1 and text in err and name.encode() in err, (rc, err)

    def f_ape(**kw):
        p = {**dict(xn=x, alpha=0.5, dirmask=14, out=o, nb=1, T=3, X=1, Y=2, Z=5), **kw}
        return ape(p['xn'], p['alpha'], p['dirmask'], p['out'], p['nb'], p['T'], p['X'], p['Y'], p['Z'], None)

    def f_l1(**kw):
        p = {**dict(xn=x, alpha=0.3, out=o, nb=1, T=3, X=1, Y=2, Z=5), **kw}
        return l1(p['xn'], p['alpha'], p['out'], p['nb'], p['T'], p['X'], p['Y'], p['Z'], None)

    def f_l23(fn):
        def call(**kw):
            p = {**dict(xn=x, dec=b, alpha=0.6, out=o, nb=1, T=3, X=1, Y=2, Z=5), **kw}
            return fn(p['xn'], p['dec'], p['alpha'], p['out'], p['nb'], p['T'], p['X'], p['Y'], p['Z'], None)
        return call

    for name, fn, ptrs in ((NAMES[0], f_ape, ('xn', 'out')), (NAMES[1], f_l1, ('xn', 'out')),
                           (NAMES[2], f_l23(l2), ('xn', 'dec', 'out')), (NAMES[3], f_l23(l3), ('xn', 'dec', 'out'))):
        for k in ptrs:
            bad(fn(**{k: None}), b'null pointer', name)
        for k in ptrs[:-1]:                                  # the output on top of any input
            bad(fn(out={'xn': x, 'dec': b}[k]), b'alias', name)
        for kw in bad_dims:
            bad(fn(**kw), b'size', name)
        for a in bad_alphas:
            bad(fn(alpha=a), b'alpha', name)
    for m in (0, 16, -1, 31, 1, 2, 4, 8):
        bad(f_ape(dirmask=m), b'dirmask', NAMES[0])


def test_smear_python_surface():
    from l2hmc import _ops as ops
    from l2hmc.lattice.su3.pytorch import lattice as lsu3
    sig = {'su3_ape_smear_n': ['xn', 'alpha', 'dirmask', 'lat', 'out'], 'su3_hyp_level1_n': ['xn', 'alpha3', 'lat', 'out'],
           'su3_hyp_level2_n': ['xn', 'b1', 'alpha2', 'lat', 'out'], 'su3_hyp_level3_n': ['xn', 'b2', 'alpha1', 'lat', 'out']}
    for name, params in sig.items():
        p = inspect.signature(getattr(ops, name)).parameters
        assert list(p) == params and p['out'].default is None, name
    LS = lsu3.LatticeSU3

    def defaults(fn):
        p = inspect.signature(fn).parameters
        return [(k, v.default) for k, v in list(p.items())[2:]]
    assert defaults(LS.ape_smear) == defaults(LS.ape_smear_n) == [('alpha', 0.5), ('nsteps', 1), ('dirs', 'spatial'),
                                                                  ('time_dir', 0)]
    assert defaults(LS.hyp_smear) == defaults(LS.hyp_smear_n) == [('alphas', (0.75, 0.6, 0.3)), ('nsteps', 1)]
    assert defaults(LS.wilson_loop_sums_n) == [('rmax', inspect.Parameter.empty), ('tmax', inspect.Parameter.empty),
                                               ('xtn', None)]
    # the table's own parameter list stays what it was; the two-field table is a method of its own
    assert defaults(LS.wilson_loop_table) == [('rmax', inspect.Parameter.empty), ('tmax', inspect.Parameter.empty),
                                              ('time_dir', 0)]
    assert list(inspect.signature(LS.wilson_loop_table_xt).parameters) == ['self', 'x', 'xt', 'rmax', 'tmax', 'time_dir']
    assert inspect.signature(LS.wilson_loop_table_xt).parameters['time_dir'].default == 0
    assert defaults(LS.smeared_loop_table) == [('rmax', inspect.Parameter.empty), ('tmax', inspect.Parameter.empty),
                                               ('time_dir', 0), ('ape_alpha', 0.5), ('ape_steps', 10),
                                               ('hyp_alphas', (0.75, 0.6, 0.3))]
    assert [LS._ape_dirmask('spatial', t) for t in range(4)] == [14, 13, 11, 7] and LS._ape_dirmask('all', 2) == 15
    # what raises before any kernel runs
    lat = LS(1, [2, 2, 2, 4])
    x = torch.zeros(1, 4, 2, 2, 2, 4, 3, 3, dtype=torch.complex128)
    xn = torch.zeros(1, 4, 9, 32, dtype=torch.complex128)
    for kw in (dict(dirs='temporal'), dict(dirs=None), dict(dirs=14), dict(nsteps=-1), dict(nsteps=1.5),
               dict(alpha=-0.1), dict(alpha=1.1), dict(alpha=float('nan')), dict(time_dir=4), dict(time_dir=-1)):
        with pytest.raises(ValueError):
            lat.ape_smear(x, **kw)
        with pytest.raises(ValueError):
            lat.ape_smear_n(xn, **kw)
    for kw in (dict(alphas=(0.75, 0.6)), dict(alphas=(0.75, 0.6, 0.3, 0.1)), dict(alphas=0.5), dict(alphas=None),
               dict(alphas=(0.75, 0.6, 1.2)), dict(alphas=(-0.1, 0.6, 0.3)), dict(alphas=(0.75, float('nan'), 0.3)),
               dict(alphas=('a', 'b', 'c')), dict(nsteps=-1), dict(nsteps=0.5)):
        with pytest.raises(ValueError):
            lat.hyp_smear(x, **kw)
        with pytest.raises(ValueError):
            lat.hyp_smear_n(xn, **kw)
    with pytest.raises(ValueError, match='time_dir'):
        lat.wilson_loop_table_xt(x, x, 1, 1, time_dir=None)
    with pytest.raises(ValueError):
        lat.wilson_loop_table_xt(x, x[:, :, :1], 1, 1)
    with pytest.raises(ValueError):
        lat.smeared_loop_table(x, 1, 1, time_dir=None)
    with pytest.raises(ValueError):
        lat.smeared_loop_table(x, 1, 1, ape_steps=-2)
    with pytest.raises(ValueError):
        lat.smeared_loop_table(x, 1, 1, ape_steps=0, hyp_alphas=(0.5, 0.5))
    # no autograd through any of them: LatticeSU3._no_grad, which raises for every measurement of this class
    g, gn = x.clone().requires_grad_(True), xn.clone().requires_grad_(True)
    for call in (lambda: lat.ape_smear(g), lambda: lat.ape_smear_n(gn), lambda: lat.hyp_smear(g),
                 lambda: lat.hyp_smear_n(gn), lambda: lat.smeared_loop_table(g, 1, 1),
                 lambda: lat.wilson_loop_table_xt(x, g, 1, 1), lambda: lat.wilson_loop_table_xt(g, x, 1, 1), lambda: lat.wilson_loop_sums_n(xn, 1, 1, gn)):
        with pytest.raises(RuntimeError, match='no autograd'):
            call()
