"""CPU tier of the drop-in boundary of the clover force: the export of csrc/su3_clover_force.hip exists, agrees with
native.SIGNATURES and the header, and refuses bad arguments with an error text before any HIP call; the Python surface on
top of it is present and opt-in."""
import inspect

import pytest
import torch

FORCE = 'l2q_su3_clover_force'
EINVAL, ESHAPE = -1, -2


def test_symbol_and_signature():
    import ctypes as C
    from l2hmc import native
    lib = native.load()
    P, I, D, Z = C.c_void_p, C.c_int, C.c_double, C.c_size_t
    assert hasattr(lib, FORCE)
    assert native.SIGNATURES[FORCE] == (I, [P, P, P, P, P, P, D, D, D, I, I, I, I, I, I, P, Z, P])
    header = open(native.os.path.join(native._HERE, '..', '..', 'include', 'l2q.h')).read()
    flat = ' '.join(header.split())
    decl = ('int l2q_su3_clover_force(const void* xn, const void* X, const void* Y, const void* clinv, const void* f_in, '
            'void* f_out, double kc, double coef, double det_weight, int nb, int npf, int T, int X_, int Y_, int Z, '
            'void* ws, size_t ws_bytes, void* stream);')
    assert decl in flat and flat.index(decl) > flat.index('int l2q_su3_clover_apply(')
    assert flat.index(decl) < flat.index('L2HMC momentum update')
    for words in ('- 2 npf log det A_oo', 'X_o = kappa A_oo^-1 H_oe X_e', 'Y_o = kappa A_oo^-1 (H^H)_oe Y_e',
                  'dS_det = -2 npf sum_{x odd} tr[A^-1(x) dA(x)]', 'F_sw = -TAH(U_mu(x) B_mu(x))', 'ws[nb][6][9][V]',
                  'ws_bytes >= nb * 54 * V * sizeof(double)'):
        assert words in flat, words


def test_argument_errors():
    from l2hmc import native
    lib = native.load()
    # (addresses are never dereferenced: every check below comes before any HIP call)
    x, fx, fy, ci, fi, fo, w = 4096, 8192, 12288, 16384, 20480, 24576, 28672
    nan, inf = float('nan'), float('inf')
    V = 2 * 4 * 2 * 6

    def bad(rc, code, text):
        err = lib.l2q_last_error()
        assert rc == code and text in err and FORCE.encode() in err, (rc, err)

    def force(**kw):
        p = {**dict(xn=x, X=fx, Y=fy, clinv=ci, f_in=fi, f_out=fo, kc=0.2, coef=-0.05, dw=2.0, nb=1, npf=2, T=2, X_=4,
                    Y_=2, Z=6, ws=w, ws_bytes=54 * V * 8), **kw}
        return lib.l2q_su3_clover_force(p['xn'], p['X'], p['Y'], p['clinv'], p['f_in'], p['f_out'], p['kc'], p['coef'],
                                        p['dw'], p['nb'], p['npf'], p['T'], p['X_'], p['Y_'], p['Z'], p['ws'],
                                        p['ws_bytes'], None)

    for k in ('xn', 'f_out', 'ws', 'X', 'Y'):
        bad(force(**{k: None}), EINVAL, b'null pointer')
    for kw in (dict(npf=0), dict(npf=0, X=None), dict(npf=0, Y=None), dict(npf=-1, X=None, Y=None)):
        bad(force(**kw), EINVAL, b'npf')
    bad(force(npf=0, X=None, Y=None, clinv=None), EINVAL, b'both halves absent')
    for kw in (dict(f_out=x), dict(f_out=fx), dict(f_out=fy), dict(f_out=ci), dict(f_out=w), dict(ws=x), dict(ws=fx),
               dict(ws=fy), dict(ws=ci), dict(ws=fi)):
        bad(force(**kw), EINVAL, b'alias')
    for k in ('kc', 'coef', 'dw'):
        for v in (nan, inf, -inf):
            bad(force(**{k: v}), EINVAL, b'finite')
    for kw in (dict(nb=0), dict(T=0), dict(Z=-2), dict(T=1 << 12, X_=1 << 12, Y_=8), dict(nb=64, npf=12, T=32, X_=32, Y_=32, Z=8)):
        bad(force(**kw), EINVAL, b'size')
    for kw in (dict(ws_bytes=54 * V * 8 - 1), dict(ws_bytes=0), dict(nb=2)):
        bad(force(**kw), EINVAL, b'workspace too small')
    for kw in (dict(T=3, ws_bytes=1 << 30), dict(X_=1), dict(Y_=5, ws_bytes=1 << 30), dict(Z=7, ws_bytes=1 << 30)):
        bad(force(**kw), ESHAPE, b'even extents')
    # what is legal passes every check and fails only at the launch: not tried here (no GPU); f_in may be null or f_out,
    # either half may be absent -- the refusals above name nothing of that
    for kw in (dict(f_in=None), dict(f_in=fo), dict(clinv=None), dict(npf=0, X=None, Y=None)):
        p = dict(T=3, ws_bytes=1 << 30)                           # ... seen through the last check, the odd extent
        bad(force(**kw, **p), ESHAPE, b'even extents')


def test_python_surface():
    from l2hmc import _ops as ops
    from l2hmc.dynamics.pytorch import fermion_hmc as fh
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3 as LS
    p = inspect.signature(ops.su3_clover_force_n).parameters
    assert list(p) == ['xn', 'X', 'Y', 'clinv', 'kc', 'lat', 'det_weight', 'coef', 'f_in', 'out']
    assert [p[k].default for k in ('det_weight', 'coef', 'f_in', 'out')] == [0.0, 1.0, None, None]
    for name in ('wilson_clover_solve_schur_normal', 'clover_pseudofermion_refresh', 'clover_pseudofermion_action',
                 'clover_pseudofermion_force'):
        q, qn = (inspect.signature(getattr(LS, name + sfx)).parameters for sfx in ('', '_n'))
        skip = 2 if name == 'clover_pseudofermion_refresh' else 3        # self and the tensors: x / xn, phi / phi_e
        assert list(q)[skip:] == list(qn)[skip:] and [v.default for v in q.values()] == [v.default for v in qn.values()], name
        assert 'c_sw' in q and q['clover'].default is None, name
    q = inspect.signature(LS.wilson_clover_solve_schur_normal_n).parameters
    assert list(q)[3:] == ['kappa', 'c_sw', 'tol', 'max_iter', 'check_every', 'antiperiodic_t', 'clover']
    q = inspect.signature(LS.clover_pseudofermion_refresh_n).parameters
    assert list(q)[2:] == ['kappa', 'c_sw', 'npf', 'generator', 'antiperiodic_t', 'clover']
    # opt-in: the existing entry points and classes keep their signatures
    for name in ('pseudofermion_action', 'pseudofermion_force', 'pseudofermion_refresh_eo', 'wilson_solve_schur_normal_n'):
        assert 'c_sw' not in inspect.signature(getattr(LS, name)).parameters
    for cls in (fh.WilsonHMC, fh.WilsonHMCEvenOdd, fh.WilsonHMCMixed):
        assert 'c_sw' not in inspect.signature(cls.__init__).parameters
    assert issubclass(fh.WilsonCloverHMC, fh.WilsonHMCEvenOdd) and not issubclass(fh.WilsonCloverHMC, fh.WilsonHMCMixed)
    assert list(inspect.signature(fh.WilsonCloverHMC.__init__).parameters)[1:7] == ['lattice', 'beta', 'kappa', 'c_sw', 'eps',
                                                                                 'nleapfrog']
    lat = LS(2, [2, 2, 2, 2])
    for c_sw in (float('nan'), float('inf'), 'one', None, True):
        with pytest.raises(ValueError, match='c_sw'):
            fh.WilsonCloverHMC(lat, 5.5, 0.12, c_sw, 0.05, 4)
    with pytest.raises(ValueError, match='even'):
        fh.WilsonCloverHMC(LS(2, [3, 2, 2, 2]), 5.5, 0.12, 1.0, 0.05, 4)
    assert fh.WilsonCloverHMC(lat, 5.5, 0.12, 1.0, 0.05, 4, npf=2).c_sw == 1.0
    # the wrapper is strict about dtype, shape and contiguity, before any native call
    L, V = (2, 2, 2, 2), 16
    xn = torch.zeros(2, 4, 9, V, dtype=torch.complex128)
    X = torch.zeros(2, 3, 12, V, dtype=torch.complex128)
    cl = torch.zeros(2, 2, 2, 36, V // 2, dtype=torch.float64)
    for wrong in (cl.to(torch.float32), cl[:1], cl[..., :7], cl.transpose(1, 2)):
        with pytest.raises(ValueError, match='block field'):
            ops.su3_clover_force_n(xn, X, X, wrong, 0.1, L)
    for wrong in (X.to(torch.complex64), X[:, :, :, :8], X.transpose(0, 1), X[:1]):
        with pytest.raises(ValueError, match='su3_clover_force_n'):
            ops.su3_clover_force_n(xn, wrong, X, cl, 0.1, L)
    with pytest.raises(ValueError, match='su3_clover_force_n'):
        ops.su3_clover_force_n(xn, X, X[:, :2], cl, 0.1, L)
    with pytest.raises(ValueError, match='together'):
        ops.su3_clover_force_n(xn, X, None, cl, 0.1, L)
    with pytest.raises(ValueError, match='or both'):
        ops.su3_clover_force_n(xn, None, None, None, 0.1, L)
    for name in ('f_in', 'out'):
        for wrong in (xn.to(torch.complex64), xn[:1], xn[..., :8]):
            with pytest.raises(ValueError, match=name):
                ops.su3_clover_force_n(xn, X, X, cl, 0.1, L, **{name: wrong})
    with pytest.raises(ValueError, match=r'even extents.*\[3, 4, 5, 2\]'):
        ops.su3_clover_force_n(torch.zeros(2, 4, 9, 120, dtype=torch.complex128), X, X, cl, 0.1, (3, 4, 5, 2))
