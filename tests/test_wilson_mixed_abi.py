"""CPU tier of the drop-in boundary of the mixed-precision even-odd solves: the exports of csrc/su3_wilson_f32.hip exist,
agree with native.SIGNATURES and the header, and refuse bad arguments with an error text before any HIP call; the Python
surface on top of them is present and opt-in, the existing signatures are what they were, and what should raise does so
before any kernel runs."""
import ctypes as C
import inspect

import pytest
import torch

P, I, L_, D = C.c_void_p, C.c_int, C.c_long, C.c_double
DECLS = {
    'l2q_su3_links_demote_eo': ((I, [P, P, I, I, I, I, I, P]),
                                'int l2q_su3_links_demote_eo(const void* xn, void* x32, int nb, int T, int X, int Y, '
                                'int Z, void* stream);'),
    'l2q_su3_wilson_hop_eo_f32': ((I, [P, P, P, P, P, D, D, I, I, I, I, I, I, I, I, P]),
                                  'int l2q_su3_wilson_hop_eo_f32(const void* x32, const void* src, const void* aux, '
                                  'void* out, double* norm_part, double a, double b, int flags, int parity, int nb, '
                                  'int nrhs, int T, int X, int Y, int Z, void* stream);'),
    'l2q_su3_spinor_cg_update_f32': ((I, [P, P, P, P, P, P, L_, L_, P]),
                                     'int l2q_su3_spinor_cg_update_f32(void* x, void* r, const void* p, const void* q, '
                                     'const double* alpha, double* rr_part, long nsys, long V, void* stream);'),
    'l2q_su3_spinor_xpay_f32': ((I, [P, P, P, L_, L_, P]),
                                'int l2q_su3_spinor_xpay_f32(void* p, const void* z, const double* beta, long nsys, '
                                'long V, void* stream);'),
    'l2q_su3_spinor_demote': ((I, [P, P, P, L_, L_, P]),
                              'int l2q_su3_spinor_demote(const void* in64, const double* scale, void* out32, long nsys, '
                              'long V, void* stream);'),
    'l2q_su3_spinor_promote_axpy': ((I, [P, P, P, L_, L_, P]),
                                    'int l2q_su3_spinor_promote_axpy(void* x64, const void* e32, const double* scale, '
                                    'long nsys, long V, void* stream);'),
}
EINVAL, ESHAPE = -1, -2


def test_symbols_and_signatures():
    from l2hmc import native
    lib = native.load()
    flat = ' '.join(open(native.os.path.join(native._HERE, '..', '..', 'include', 'l2q.h')).read().split())
    for name, (sig, decl) in DECLS.items():
        assert hasattr(lib, name), name
        assert native.SIGNATURES[name] == sig, name
        assert decl in flat, name
        assert flat.index('int l2q_su3_wilson_hop_eo(') < flat.index(decl)


def checker(lib, name):
    def bad(rc, code, text):
        err = lib.l2q_last_error()
        assert rc == code and text in err and name.encode() in err, (name, rc, err)
    return bad


def test_hop_argument_errors():
    """the checks of test_wilson_eo_abi.py on the fp32 hop (addresses are never dereferenced)"""
    from l2hmc import native
    lib = native.load()
    name = 'l2q_su3_wilson_hop_eo_f32'
    hop, bad = getattr(lib, name), checker(lib, name)
    x, s, a, o, n = 4096, 8192, 12288, 16384, 20480
    nan, inf = float('nan'), float('inf')

    def call(**kw):
        p = {**dict(xn=x, src=s, aux=a, out=o, part=n, a=0.5, b=1.0, flags=2, parity=0, nb=1, nrhs=2, T=2, X=4, Y=2, Z=6),
             **kw}
        return hop(p['xn'], p['src'], p['aux'], p['out'], p['part'], p['a'], p['b'], p['flags'], p['parity'], p['nb'],
                   p['nrhs'], p['T'], p['X'], p['Y'], p['Z'], None)

    for k in ('xn', 'src', 'out'):
        bad(call(**{k: None}), EINVAL, b'null pointer')
    bad(call(out=s), EINVAL, b'alias')
    bad(call(out=x), EINVAL, b'alias')
    for kw in (dict(a=nan), dict(a=inf), dict(b=-inf), dict(b=nan)):
        bad(call(**kw), EINVAL, b'finite')
    for fl in (-1, 4, 7, 1 << 20):
        bad(call(flags=fl), EINVAL, b'flags')
    for par in (-1, 2, 3):
        bad(call(parity=par), EINVAL, b'parity')
    for kw in (dict(nb=0), dict(nb=-1), dict(nrhs=0), dict(nrhs=-2), dict(T=0), dict(X=-4), dict(Y=0), dict(Z=0),
               dict(T=1 << 12, X=1 << 12, Y=8), dict(nb=64, nrhs=12, T=32, X=32, Y=32, Z=8)):
        bad(call(**kw), EINVAL, b'size')
    for kw in (dict(T=3), dict(X=1), dict(Y=5), dict(Z=7), dict(T=1, X=1, Y=1, Z=1)):
        bad(call(**kw), ESHAPE, b'needs even extents')


def test_other_argument_errors():
    from l2hmc import native
    lib = native.load()
    a, b, c, d, e, f = 4096, 8192, 12288, 16384, 20480, 24576
    name = 'l2q_su3_links_demote_eo'
    fn, bad = getattr(lib, name), checker(lib, name)
    bad(fn(None, b, 1, 2, 2, 2, 2, None), EINVAL, b'null pointer')
    bad(fn(a, None, 1, 2, 2, 2, 2, None), EINVAL, b'null pointer')
    bad(fn(a, a, 1, 2, 2, 2, 2, None), EINVAL, b'alias')
    for dims in ((0, 2, 2, 2, 2), (1, 0, 2, 2, 2), (1, 2, 2, 2, -2), (1, 1 << 12, 1 << 12, 8, 2)):
        bad(fn(a, b, *dims, None), EINVAL, b'size')
    for dims in ((1, 3, 2, 2, 2), (1, 2, 2, 2, 5), (1, 1, 1, 1, 1)):
        bad(fn(a, b, *dims, None), ESHAPE, b'needs even extents')
    name = 'l2q_su3_spinor_cg_update_f32'
    fn, bad = getattr(lib, name), checker(lib, name)
    ok = [a, b, c, d, e, f]
    for i in range(6):
        bad(fn(*[None if j == i else v for j, v in enumerate(ok)], 2, 8, None), EINVAL, b'null pointer')
    for args in ((a, a, c, d), (a, b, a, d), (a, b, c, a), (a, b, b, d), (a, b, c, b)):
        bad(fn(*args, e, f, 2, 8, None), EINVAL, b'alias')
    for nsys, V in ((0, 8), (2, 0), (-1, 8), (1 << 20, 1 << 20)):
        bad(fn(*ok, nsys, V, None), EINVAL, b'size')
    for name, alias in (('l2q_su3_spinor_xpay_f32', True), ('l2q_su3_spinor_demote', True),
                        ('l2q_su3_spinor_promote_axpy', True)):
        fn, bad = getattr(lib, name), checker(lib, name)
        ok = [a, b, c]
        for i in range(3):
            bad(fn(*[None if j == i else v for j, v in enumerate(ok)], 2, 8, None), EINVAL, b'null pointer')
        clash = (a, a, c) if name != 'l2q_su3_spinor_demote' else (a, b, a)       # demote: (in64, scale, out32)
        bad(fn(*clash, 2, 8, None), EINVAL, b'alias')
        for nsys, V in ((0, 8), (2, 0), (-1, 8), (1 << 20, 1 << 20)):
            bad(fn(*ok, nsys, V, None), EINVAL, b'size')


def test_python_surface_is_opt_in():
    from l2hmc import _ops as ops
    from l2hmc.dynamics.pytorch.fermion_hmc import WilsonHMC, WilsonHMCEvenOdd, WilsonHMCMixed
    from l2hmc.lattice.su3.pytorch import wilson
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3 as LS
    for name in ('su3_links_demote_eo_n', 'su3_wilson_hop_eo_f32_n', 'su3_spinor_cg_update_f32_', 'su3_spinor_xpay_f32_',
                 'su3_spinor_demote', 'su3_spinor_promote_axpy_'):
        assert callable(getattr(ops, name)), name
    p = inspect.signature(ops.su3_wilson_hop_eo_f32_n).parameters
    assert list(p) == ['x32', 'src', 'lat', 'parity', 'dagger', 'antiperiodic_t', 'a', 'aux', 'b', 'out', 'norm']
    assert [p[k].default for k in list(p)[4:]] == [False, True, 1.0, None, 0.0, None, False]
    # the mixed solvers: the arguments of their fp64 siblings, then inner_tol, max_inner, max_outer
    extra = ['inner_tol', 'max_inner', 'max_outer']
    for twin, base in (('wilson_solve_eo_mixed_n', 'wilson_solve_eo_n'), ('wilson_solve_eo_mixed', 'wilson_solve_eo'),
                       ('wilson_solve_schur_normal_mixed_n', 'wilson_solve_schur_normal_n')):
        q, r = inspect.signature(getattr(LS, twin)).parameters, inspect.signature(getattr(LS, base)).parameters
        assert list(q) == list(r) + extra, twin
        assert all(q[k].default == r[k].default for k in r), twin
        assert [q[k].default for k in extra] == [wilson.MIXED_INNER_TOL, wilson.MIXED_MAX_INNER, wilson.MIXED_MAX_OUTER]
    # no pinned signature changed: the fp64 solvers and the keyword-forwarding methods are what they were
    q = inspect.signature(LS.wilson_solve_schur_normal_n).parameters
    assert list(q)[1:] == ['xn', 'phi_e', 'kappa', 'tol', 'max_iter', 'check_every', 'antiperiodic_t']
    assert str(inspect.signature(LS.wilson_solve_eo_n)) == str(inspect.signature(LS.wilson_solve_n))
    for name in ('pseudofermion_action', 'pseudofermion_force', 'quark_propagator'):
        for fn in (getattr(LS, name), getattr(LS, name + '_n')):
            assert list(inspect.signature(fn).parameters)[-1] == 'solve_kwargs', name
    assert list(inspect.signature(LS._force_fields_n).parameters) == ['self', 'what', 'xn', 'phin', 'kappa', 'even_odd',
                                                                      'solve_kwargs']
    assert list(inspect.signature(wilson._CG.cgnr).parameters) == ['self', 'final']
    assert inspect.signature(wilson._CG.cgnr).parameters['final'].default is True
    assert inspect.signature(wilson._CG.normal).parameters['final'].default is True
    assert issubclass(WilsonHMCMixed, WilsonHMCEvenOdd) and WilsonHMCMixed.even_odd is True
    assert inspect.signature(WilsonHMCEvenOdd.__init__) == inspect.signature(WilsonHMC.__init__)
    q = inspect.signature(WilsonHMCMixed.__init__).parameters
    assert q['inner_tol'].kind is q['max_inner'].kind is inspect.Parameter.KEYWORD_ONLY
    lat = LS(2, [2, 2, 2, 2])
    h = WilsonHMCMixed(lat, 5.5, 0.1, 0.05, 4, inner_tol=1e-3, max_inner=50)
    assert h._solve_kw(1e-8) == dict(tol=1e-8, max_iter=2000, antiperiodic_t=True, mixed=True, inner_tol=1e-3, max_inner=50)
    assert WilsonHMCMixed(lat, 5.5, 0.1, 0.05, 4)._solve_kw(1e-8)['mixed'] is True
    assert 'mixed' not in WilsonHMCEvenOdd(lat, 5.5, 0.1, 0.05, 4)._solve_kw(1e-8)
    for kw in (dict(inner_tol=0.0), dict(inner_tol=1.0), dict(max_inner=0), dict(max_inner=2.5)):
        with pytest.raises(ValueError, match='inner_tol'):
            WilsonHMCMixed(lat, 5.5, 0.1, 0.05, 4, **kw)


def test_what_raises_before_any_kernel(monkeypatch):
    from l2hmc import _ops as ops
    from l2hmc import native
    from l2hmc.dynamics.pytorch.fermion_hmc import WilsonHMCMixed
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3 as LS

    def no_kernel(name, *args):
        raise AssertionError(f'{name} was called')
    monkeypatch.setattr(native, 'call', no_kernel)
    c128 = torch.complex128
    lat = LS(2, [2, 2, 2, 2])
    xn, x = torch.zeros(2, 4, 9, 16, dtype=c128), torch.zeros(2, 4, 2, 2, 2, 2, 3, 3, dtype=c128)
    fn, hn = torch.zeros(2, 1, 12, 16, dtype=c128), torch.zeros(2, 1, 12, 8, dtype=c128)
    f = torch.zeros(2, 1, 2, 2, 2, 2, 4, 3, dtype=c128)
    # mixed=True without even_odd=True
    for call in (lambda: lat.quark_propagator_n(xn, 0.1, mixed=True), lambda: lat.quark_propagator(x, 0.1, mixed=True),
                 lambda: lat.pseudofermion_action_n(xn, fn, 0.1, mixed=True),
                 lambda: lat.pseudofermion_action(x, f, 0.1, mixed=True),
                 lambda: lat.pseudofermion_force_n(xn, fn, 0.1, mixed=True),
                 lambda: lat.pseudofermion_force(x, f, 0.1, mixed=True),
                 lambda: lat._force_fields_n('pseudofermion_force', xn, fn, 0.1, False, mixed=True)):
        with pytest.raises(ValueError, match='mixed=True needs even_odd=True'):
            call()
    # the keywords of the mixed solves without mixed=True
    for call in (lambda: lat.pseudofermion_action_n(xn, hn, 0.1, even_odd=True, inner_tol=1e-3),
                 lambda: lat.quark_propagator_n(xn, 0.1, even_odd=True, max_outer=3),
                 lambda: lat.pseudofermion_force_n(xn, hn, 0.1, even_odd=True, max_inner=3)):
        with pytest.raises(ValueError, match='pass mixed=True'):
            call()
    # odd extents
    odd = LS(2, [3, 4, 5, 2])
    oxn, ox = torch.zeros(2, 4, 9, 120, dtype=c128), torch.zeros(2, 4, 3, 4, 5, 2, 3, 3, dtype=c128)
    ofn, ohn = torch.zeros(2, 1, 12, 120, dtype=c128), torch.zeros(2, 1, 12, 60, dtype=c128)
    of = torch.zeros(2, 1, 3, 4, 5, 2, 4, 3, dtype=c128)
    for call in (lambda: odd.wilson_solve_eo_mixed_n(oxn, ofn, 0.1), lambda: odd.wilson_solve_eo_mixed(ox, of, 0.1),
                 lambda: odd.wilson_solve_schur_normal_mixed_n(oxn, ohn, 0.1),
                 lambda: odd.quark_propagator_n(oxn, 0.1, even_odd=True, mixed=True),
                 lambda: odd.pseudofermion_action_n(oxn, ohn, 0.1, even_odd=True, mixed=True),
                 lambda: odd.pseudofermion_action(ox, of, 0.1, even_odd=True, mixed=True),
                 lambda: odd.pseudofermion_force_n(oxn, ohn, 0.1, even_odd=True, mixed=True),
                 lambda: odd.pseudofermion_force(ox, of, 0.1, even_odd=True, mixed=True),
                 lambda: WilsonHMCMixed(odd, 5.5, 0.1, 0.05, 4),
                 lambda: ops.su3_links_demote_eo_n(oxn, (3, 4, 5, 2)),
                 lambda: ops.su3_wilson_hop_eo_f32_n(oxn, ohn, (3, 4, 5, 2), 0)):
        with pytest.raises(ValueError, match=r'even extents.*\[3, 4, 5, 2\]'):
            call()
    # bad solver arguments name the public method
    for kw in (dict(tol=0.0), dict(max_iter=-1), dict(check_every=0)):
        with pytest.raises(ValueError, match=r'LatticeSU3\.wilson_solve_eo_mixed: need tol > 0'):
            lat.wilson_solve_eo_mixed_n(xn, fn, 0.1, **kw)
        with pytest.raises(ValueError, match=r'LatticeSU3\.wilson_solve_schur_normal_mixed: need tol > 0'):
            lat.wilson_solve_schur_normal_mixed_n(xn, hn, 0.1, **kw)
    for kw in (dict(inner_tol=0.0), dict(inner_tol=2.0), dict(inner_tol=None), dict(max_inner=0), dict(max_inner=True),
               dict(max_outer=-1), dict(max_outer=1.5)):
        with pytest.raises(ValueError, match=r'LatticeSU3\.wilson_solve_eo_mixed: need 0 < inner_tol < 1'):
            lat.wilson_solve_eo_mixed_n(xn, fn, 0.1, **kw)
        with pytest.raises(ValueError, match=r'LatticeSU3\.wilson_solve_schur_normal_mixed: need 0 < inner_tol < 1'):
            lat.wilson_solve_schur_normal_mixed_n(xn, hn, 0.1, **kw)
    with pytest.raises(ValueError, match='half field'):
        lat.wilson_solve_schur_normal_mixed_n(xn, fn, 0.1)
    with pytest.raises(ValueError, match='autograd'):
        lat.wilson_solve_schur_normal_mixed_n(xn.clone().requires_grad_(True), hn, 0.1)
    # the wrappers are strict about dtype, shape and contiguity; the existing ones keep refusing complex64
    c64 = torch.complex64
    x32, h32 = torch.zeros(2, 2, 4, 9, 8, dtype=c64), torch.zeros(2, 3, 12, 8, dtype=c64)
    h64 = torch.zeros(2, 3, 12, 8, dtype=c128)
    s = torch.zeros(2, 3, dtype=torch.float64)
    L = (2, 2, 2, 2)
    bad = [lambda: ops.su3_links_demote_eo_n(xn.to(c64), L), lambda: ops.su3_links_demote_eo_n(xn[:, :, :, :8], L),
           lambda: ops.su3_links_demote_eo_n(xn, L, out=x32.to(c128)),
           lambda: ops.su3_wilson_hop_eo_f32_n(x32.to(c128), h32, L, 0), lambda: ops.su3_wilson_hop_eo_f32_n(x32, h64, L, 0),
           lambda: ops.su3_wilson_hop_eo_f32_n(x32, h32[..., :7], L, 0), lambda: ops.su3_wilson_hop_eo_f32_n(x32, h32, L, 2),
           lambda: ops.su3_wilson_hop_eo_f32_n(x32, h32, L, 0, aux=h64),
           lambda: ops.su3_wilson_hop_eo_f32_n(x32, h32, L, 0, out=h32.transpose(0, 1)),
           lambda: ops.su3_wilson_hop_eo_f32_n(x32, h32, L, 0, norm=torch.zeros(2, 3, 2, dtype=torch.float64)),
           lambda: ops.su3_spinor_cg_update_f32_(h32, h32.clone(), h64, h32.clone(), s),
           lambda: ops.su3_spinor_cg_update_f32_(h32, h32.clone(), h32.clone(), h32.clone(), s.to(torch.float32)),
           lambda: ops.su3_spinor_xpay_f32_(h32, h64, s), lambda: ops.su3_spinor_xpay_f32_(h32, h32.clone(), s[:1]),
           lambda: ops.su3_spinor_demote(h32, s), lambda: ops.su3_spinor_demote(h64, s, out=h64.clone()),
           lambda: ops.su3_spinor_promote_axpy_(h32, h32.clone(), s), lambda: ops.su3_spinor_promote_axpy_(h64, h64.clone(), s),
           lambda: ops.su3_spinor_cg_update_(h32, h32.clone(), h32.clone(), h32.clone(), s),
           lambda: ops.su3_spinor_xpay_(h32, h32.clone(), s), lambda: ops.su3_wilson_hop_eo_n(xn, h32, L, 0)]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
