"""CPU tier of the drop-in boundary of the clover term: the four exports of csrc/su3_wilson_clover.hip exist, agree with
native.SIGNATURES and the header, and refuse bad arguments with an error text before any HIP call; the Python surface on
top of them is present and opt-in."""
import inspect

import pytest
import torch

TERM, INVERT, HOP, APPLY = ('l2q_su3_clover_term', 'l2q_su3_clover_invert', 'l2q_su3_wilson_clover_hop_eo',
                            'l2q_su3_clover_apply')
EINVAL, ESHAPE = -1, -2


def test_symbols_and_signatures():
    import ctypes as C
    from l2hmc import native
    lib = native.load()
    P, I, D = C.c_void_p, C.c_int, C.c_double
    want = {TERM: (I, [P, P, D, I, I, I, I, I, P]), INVERT: (I, [P, P, P, P, I, I, I, I, I, P]),
            HOP: (I, [P, P, P, P, P, P, D, D, I, I, I, I, I, I, I, I, I, P]), APPLY: (I, [P, P, P, P, I, I, I, I, I, I, I, P])}
    for name, sig in want.items():
        assert hasattr(lib, name) and native.SIGNATURES[name] == sig, name
    header = open(native.os.path.join(native._HERE, '..', '..', 'include', 'l2q.h')).read()
    flat = ' '.join(header.split())
    decls = ['int l2q_su3_clover_term(const void* xn, void* cl, double coef, int nb, int T, int X, int Y, int Z, void* stream);',
             'int l2q_su3_clover_invert(const void* cl, void* clinv, double* minpiv_part, double* logdet_part, int nb, int T, '
             'int X, int Y, int Z, void* stream);',
             'int l2q_su3_wilson_clover_hop_eo(const void* xn, const void* src, const void* aux, const void* c, void* out, '
             'double* norm_part, double a, double b, int flags, int parity, int cmode, int nb, int nrhs, int T, int X, int Y, '
             'int Z, void* stream);',
             'int l2q_su3_clover_apply(const void* c, const void* src, void* out, double* norm_part, int parity, int nb, '
             'int nrhs, int T, int X, int Y, int Z, void* stream);']
    at = flat.index('int l2q_su3_spinor_promote_axpy(')
    for d in decls:
        assert d in flat and flat.index(d) > at, d
        at = flat.index(d)
    for words in ('NOT made traceless', '[nb][2 parity][2 chirality][36][V/2]', 'Mhat = A_ee - kappa^2 H_eo A_oo^-1 H_oe',
                  'bhat_e = b_e + kappa H_eo A_oo^-1 b_o', 'psi_o = A_oo^-1 (b_o + kappa H_oe psi_e)'):
        assert words in flat, words


def test_argument_errors():
    from l2hmc import native
    lib = native.load()
    # (addresses are never dereferenced: every check below comes before any HIP call)
    x, s, a, c, o, n, m = 4096, 8192, 12288, 16384, 20480, 24576, 28672
    nan, inf = float('nan'), float('inf')

    def bad(name, rc, code, text):
        err = lib.l2q_last_error()
        assert rc == code and text in err and name.encode() in err, (name, rc, err)

    def term(**kw):
        p = {**dict(xn=x, cl=c, coef=0.2, nb=1, T=2, X=4, Y=2, Z=6), **kw}
        return lib.l2q_su3_clover_term(p['xn'], p['cl'], p['coef'], p['nb'], p['T'], p['X'], p['Y'], p['Z'], None)

    for k in ('xn', 'cl'):
        bad(TERM, term(**{k: None}), EINVAL, b'null pointer')
    bad(TERM, term(cl=x), EINVAL, b'alias')
    for v in (nan, inf, -inf):
        bad(TERM, term(coef=v), EINVAL, b'finite')
    for kw in (dict(nb=0), dict(T=0), dict(Z=-2), dict(T=1 << 12, X=1 << 12, Y=8)):
        bad(TERM, term(**kw), EINVAL, b'size')
    for kw in (dict(T=3), dict(X=1), dict(Y=5), dict(Z=7)):
        bad(TERM, term(**kw), ESHAPE, b'even extents')

    def invert(**kw):
        p = {**dict(cl=c, clinv=o, mp=n, ld=m, nb=1, T=2, X=4, Y=2, Z=6), **kw}
        return lib.l2q_su3_clover_invert(p['cl'], p['clinv'], p['mp'], p['ld'], p['nb'], p['T'], p['X'], p['Y'], p['Z'], None)

    for k in ('cl', 'clinv', 'mp'):
        bad(INVERT, invert(**{k: None}), EINVAL, b'null pointer')
    for kw in (dict(clinv=c), dict(mp=c), dict(mp=o), dict(ld=c), dict(ld=o), dict(ld=n)):
        bad(INVERT, invert(**kw), EINVAL, b'alias')
    bad(INVERT, invert(nb=0), EINVAL, b'size')
    for kw in (dict(T=3), dict(Z=1)):
        bad(INVERT, invert(**kw), ESHAPE, b'even extents')

    def hop(**kw):
        p = {**dict(xn=x, src=s, aux=a, c=c, out=o, part=n, a=0.5, b=1.0, flags=2, parity=0, cmode=1, nb=1, nrhs=2, T=2,
                    X=4, Y=2, Z=6), **kw}
        return lib.l2q_su3_wilson_clover_hop_eo(p['xn'], p['src'], p['aux'], p['c'], p['out'], p['part'], p['a'], p['b'],
                                                p['flags'], p['parity'], p['cmode'], p['nb'], p['nrhs'], p['T'], p['X'],
                                                p['Y'], p['Z'], None)

    for k in ('xn', 'src', 'out'):
        bad(HOP, hop(**{k: None}), EINVAL, b'null pointer')
    for cm in (-1, 3, 7):
        bad(HOP, hop(cmode=cm), EINVAL, b'cmode')
    for kw in (dict(c=None, cmode=1), dict(c=None, cmode=2), dict(cmode=0)):
        bad(HOP, hop(**kw), EINVAL, b'block field c')
    for kw in (dict(out=s), dict(out=x), dict(out=c)):
        bad(HOP, hop(**kw), EINVAL, b'alias')
    for kw in (dict(a=nan), dict(a=inf), dict(b=-inf), dict(b=nan)):
        bad(HOP, hop(**kw), EINVAL, b'finite')
    for fl in (-1, 4):
        bad(HOP, hop(flags=fl), EINVAL, b'flags')
    for par in (-1, 2):
        bad(HOP, hop(parity=par), EINVAL, b'parity')
    for kw in (dict(nb=0), dict(nrhs=0), dict(T=0), dict(nb=64, nrhs=12, T=32, X=32, Y=32, Z=8)):
        bad(HOP, hop(**kw), EINVAL, b'size')
    for kw in (dict(T=3), dict(X=1), dict(Y=5), dict(Z=7)):
        bad(HOP, hop(**kw), ESHAPE, b'needs even extents')

    def apply(**kw):
        p = {**dict(c=c, src=s, out=o, part=n, parity=1, nb=1, nrhs=2, T=2, X=4, Y=2, Z=6), **kw}
        return lib.l2q_su3_clover_apply(p['c'], p['src'], p['out'], p['part'], p['parity'], p['nb'], p['nrhs'], p['T'],
                                        p['X'], p['Y'], p['Z'], None)

    for k in ('c', 'src', 'out'):
        bad(APPLY, apply(**{k: None}), EINVAL, b'null pointer')
    bad(APPLY, apply(out=c), EINVAL, b'alias')
    bad(APPLY, apply(parity=2), EINVAL, b'parity')
    bad(APPLY, apply(nrhs=0), EINVAL, b'size')
    bad(APPLY, apply(X=3), ESHAPE, b'needs even extents')


def test_python_surface():
    from l2hmc import _ops as ops
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3 as LS
    from l2hmc.lattice.su3.pytorch.wilson import CloverTerm, _CloverSchurOp
    assert callable(_CloverSchurOp)
    p = inspect.signature(ops.su3_wilson_clover_hop_eo_n).parameters
    assert list(p) == ['xn', 'src', 'lat', 'parity', 'c', 'cmode', 'dagger', 'antiperiodic_t', 'a', 'aux', 'b', 'out', 'norm']
    for name in ('clover_term', 'wilson_clover_dirac', 'wilson_clover_schur', 'wilson_clover_solve'):
        q, qn = (inspect.signature(getattr(LS, name + sfx)).parameters for sfx in ('', '_n'))
        skip = 2 if name == 'clover_term' else 3                     # self and the tensors: x / xn, psi / psin, b / bn
        assert list(q)[skip:] == list(qn)[skip:] and [v.default for v in q.values()] == [v.default for v in qn.values()], name
    q = inspect.signature(LS.wilson_clover_solve).parameters
    assert list(q)[3:] == ['kappa', 'c_sw', 'tol', 'max_iter', 'check_every', 'antiperiodic_t', 'clover']
    assert [q[k].default for k in list(q)[5:]] == [1e-10, 1000, 10, True, None]
    q = inspect.signature(LS.wilson_clover_dirac).parameters
    assert list(q)[3:] == ['kappa', 'c_sw', 'dagger', 'antiperiodic_t', 'clover'] and q['dagger'].default is False
    # opt-in: the existing entry points keep their signatures; c_sw travels in the forwarded keywords
    for name in ('wilson_solve', 'wilson_solve_eo', 'wilson_dirac', 'wilson_schur'):
        assert 'c_sw' not in inspect.signature(getattr(LS, name)).parameters
    assert list(inspect.signature(LS.quark_propagator).parameters)[-1] == 'solve_kwargs'
    # the wrappers are strict about dtype, shape and contiguity
    L, Vh = (2, 2, 2, 2), 8
    xn = torch.zeros(2, 4, 9, 16, dtype=torch.complex128)
    half = torch.zeros(2, 3, 12, Vh, dtype=torch.complex128)
    cl = torch.zeros(2, 2, 2, 36, Vh, dtype=torch.float64)
    for wrong in (cl.to(torch.float32), cl[:1], cl[..., :7], cl.transpose(1, 2), torch.zeros(2, 2, 2, 35, Vh, dtype=torch.float64)):
        with pytest.raises(ValueError, match='block field'):
            ops.su3_wilson_clover_hop_eo_n(xn, half, L, 0, wrong, 1)
        with pytest.raises(ValueError, match='block field'):
            ops.su3_clover_apply_n(wrong, half, L, 0)
        if wrong.shape[0] == 2:                                      # (the inverse takes its batch from cl itself)
            with pytest.raises(ValueError, match='block field'):
                ops.su3_clover_invert_n(wrong, L)
        with pytest.raises(ValueError, match='block field'):
            ops.su3_clover_term_n(xn, 0.1, L, out=wrong)
    with pytest.raises(ValueError, match='cmode'):
        ops.su3_wilson_clover_hop_eo_n(xn, half, L, 0, cl, 3)
    with pytest.raises(ValueError, match='cmode'):
        ops.su3_wilson_clover_hop_eo_n(xn, half, L, 0, None, 1)
    with pytest.raises(ValueError, match='cmode'):
        ops.su3_wilson_clover_hop_eo_n(xn, half, L, 0, cl, 0)
    with pytest.raises(ValueError, match='parity'):
        ops.su3_clover_apply_n(cl, half, L, 2)
    with pytest.raises(ValueError, match='half field'):
        ops.su3_clover_apply_n(cl, half[..., :7], L, 0)
    with pytest.raises(ValueError, match='xn'):
        ops.su3_clover_term_n(xn.to(torch.complex64), 0.1, L)
    for fn in (lambda: ops.su3_clover_term_n(torch.zeros(2, 4, 9, 120, dtype=torch.complex128), 0.1, (3, 4, 5, 2)),
               lambda: ops.su3_clover_invert_n(cl, (3, 4, 5, 2)), lambda: ops.su3_clover_apply_n(cl, half, (3, 4, 5, 2), 0)):
        with pytest.raises(ValueError, match=r'even extents.*\[3, 4, 5, 2\]'):
            fn()
    t = CloverTerm(cl, cl, torch.ones(2), torch.zeros(2, 2), 0.1, 1.0)
    assert t.a is cl and t.kappa == 0.1 and t.c_sw == 1.0
