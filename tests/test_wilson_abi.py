"""CPU tier of the drop-in boundary of the Wilson fermions: the four exports of csrc/su3_wilson.hip exist, agree with
native.SIGNATURES and the header, and refuse bad arguments with an error text before any HIP call; the Python surface on
top of them is present and raises what it should before any kernel runs."""
import inspect

import pytest
import torch

NAMES = ('l2q_su3_wilson_apply', 'l2q_su3_spinor_cg_update', 'l2q_su3_spinor_xpay', 'l2q_su3_wilson_norm_parts')


def test_wilson_symbols_and_signatures():
    import ctypes as C
    from l2hmc import native
    lib = native.load()
    P, I, L, D = C.c_void_p, C.c_int, C.c_long, C.c_double
    want = {'l2q_su3_wilson_apply': (I, [P, P, P, P, D, I, I, I, I, I, I, I, P]),
            'l2q_su3_spinor_cg_update': (I, [P, P, P, P, P, P, L, L, P]),
            'l2q_su3_spinor_xpay': (I, [P, P, P, L, L, P]),
            'l2q_su3_wilson_norm_parts': (L, [I, I, I, I])}
    for name in NAMES:
        assert hasattr(lib, name) and native.SIGNATURES[name] == want[name], name
    header = open(native.os.path.join(native._HERE, '..', '..', 'include', 'l2q.h')).read()
    flat = ' '.join(header.split())
    for decl in ('int l2q_su3_wilson_apply(const void* xn, const void* psi, void* out, double* norm_part, double kappa, '
                 'int flags, int nb, int nrhs, int T, int X, int Y, int Z, void* stream);',
                 'int l2q_su3_spinor_cg_update(void* x, void* r, const void* p, const void* q, const double* alpha, '
                 'double* rr_part, long nsys, long V, void* stream);',
                 'int l2q_su3_spinor_xpay(void* p, const void* z, const double* beta, long nsys, long V, void* stream);',
                 'long l2q_su3_wilson_norm_parts(int T, int X, int Y, int Z);'):
        assert decl in flat, decl


def test_wilson_norm_parts():
    from l2hmc import native
    lib = native.load()
    for L, parts in (((2, 2, 2, 2), 1), ((4, 4, 4, 4), 1), ((4, 4, 4, 8), 2), ((4, 4, 4, 10), 3), ((8, 8, 8, 8), 16),
                     ((1, 1, 1, 257), 2), ((0, 2, 2, 2), 0), ((2, -1, 2, 2), 0), ((1 << 12, 1 << 12, 8, 1), 0)):
        assert lib.l2q_su3_wilson_norm_parts(*L) == parts, L


def test_wilson_argument_errors():
    from l2hmc import native
    lib = native.load()
    apply, upd, xpay = (getattr(lib, n) for n in NAMES[:3])
    # (addresses are never dereferenced: every check below comes before any HIP call)
    x, a, b, c, d, e = 4096, 8192, 12288, 16384, 20480, 24576
    nan, inf = float('nan'), float('inf')

    def bad(rc, text, name):
        err = lib.l2q_last_error()
        assert rc == -1 and text in err and name.encode() in err, (rc, err)

    def f_apply(**kw):
        p = {**dict(xn=x, psi=a, out=b, part=c, kappa=0.12, flags=2, nb=1, nrhs=2, T=3, X=1, Y=2, Z=5), **kw}
        return apply(p['xn'], p['psi'], p['out'], p['part'], p['kappa'], p['flags'], p['nb'], p['nrhs'], p['T'], p['X'],
                     p['Y'], p['Z'], None)

    for k in ('xn', 'psi', 'out'):
        bad(f_apply(**{k: None}), b'null pointer', NAMES[0])
    bad(f_apply(out=a), b'alias', NAMES[0])
    bad(f_apply(out=x), b'alias', NAMES[0])
    for kw in (dict(nb=0), dict(nb=-1), dict(nrhs=0), dict(nrhs=-2), dict(T=0), dict(X=-3), dict(Y=0), dict(Z=0),
               dict(T=1 << 12, X=1 << 12, Y=8),                       # the links of a chain past an int
               dict(nb=64, nrhs=12, T=32, X=32, Y=32, Z=8)):          # nb * nrhs * 12 * V = 2.4e9 past an int
        bad(f_apply(**kw), b'size', NAMES[0])
    for kap in (nan, inf, -inf):
        bad(f_apply(kappa=kap), b'kappa', NAMES[0])
    for fl in (-1, 4, 7, 1 << 20):
        bad(f_apply(flags=fl), b'flags', NAMES[0])

    def f_upd(**kw):
        p = {**dict(x=a, r=b, p=c, q=d, alpha=e, part=x, nsys=2, V=30), **kw}
        return upd(p['x'], p['r'], p['p'], p['q'], p['alpha'], p['part'], p['nsys'], p['V'], None)

    for k in ('x', 'r', 'p', 'q', 'alpha', 'part'):
        bad(f_upd(**{k: None}), b'null pointer', NAMES[1])
    for kw in (dict(r=a), dict(p=a), dict(q=a), dict(p=b), dict(q=b)):
        bad(f_upd(**kw), b'alias', NAMES[1])
    for kw in (dict(nsys=0), dict(nsys=-1), dict(V=0), dict(V=-5), dict(nsys=1 << 20, V=1 << 20)):
        bad(f_upd(**kw), b'size', NAMES[1])

    def f_xpay(**kw):
        p = {**dict(p=a, z=b, beta=e, nsys=2, V=30), **kw}
        return xpay(p['p'], p['z'], p['beta'], p['nsys'], p['V'], None)

    for k in ('p', 'z', 'beta'):
        bad(f_xpay(**{k: None}), b'null pointer', NAMES[2])
    bad(f_xpay(z=a), b'alias', NAMES[2])
    for kw in (dict(nsys=0), dict(V=0), dict(V=-5), dict(nsys=1 << 20, V=1 << 20)):
        bad(f_xpay(**kw), b'size', NAMES[2])


def test_wilson_python_surface():
    from l2hmc import _ops as ops
    from l2hmc.lattice.su3.pytorch import lattice as lsu3
    from l2hmc.lattice.u1.pytorch.lattice import LatticeU1
    p = inspect.signature(ops.su3_wilson_apply_n).parameters
    assert list(p) == ['xn', 'psin', 'kappa', 'lat', 'dagger', 'antiperiodic_t', 'out', 'norm']
    assert (p['dagger'].default, p['antiperiodic_t'].default, p['out'].default, p['norm'].default) == (False, True, None, False)
    for name in ('su3_spinor_pack', 'su3_spinor_unpack', 'su3_spinor_cg_update_', 'su3_spinor_xpay_'):
        assert callable(getattr(ops, name)), name
    LS = lsu3.LatticeSU3

    def defaults(fn):
        return [(k, v.default) for k, v in list(inspect.signature(fn).parameters.items())[2:]]
    E = inspect.Parameter.empty
    assert defaults(LS.wilson_dirac)[1:] == defaults(LS.wilson_dirac_n)[1:] == [('kappa', E), ('dagger', False),
                                                                                ('antiperiodic_t', True)]
    assert [k for k, _ in defaults(LS.wilson_solve)][1:] == [k for k, _ in defaults(LS.wilson_solve_n)][1:] == \
        ['kappa', 'tol', 'max_iter', 'check_every', 'antiperiodic_t']
    assert [v for _, v in defaults(LS.wilson_solve)][2:] == [v for _, v in defaults(LS.wilson_solve_n)][2:] == \
        [1e-10, 1000, 10, True]
    assert defaults(LS.quark_propagator)[:2] == defaults(LS.quark_propagator_n)[:2] == [('kappa', E), ('source', (0, 0, 0, 0))]
    assert callable(lsu3.pion_correlator) and callable(lsu3.effective_mass)
    assert tuple(LS.gamma_matrices().shape) == (5, 4, 4)
    for name in ('wilson_dirac', 'wilson_solve', 'quark_propagator', 'gamma_matrices'):
        assert not hasattr(LatticeU1, name), name
    # the spinor layouts
    psi = torch.arange(2 * 3 * 16 * 12, dtype=torch.float64).reshape(2, 3, 2, 2, 2, 2, 4, 3).to(torch.complex128)
    pn = ops.su3_spinor_pack(psi)
    assert pn.shape == (2, 3, 12, 16) and pn.is_contiguous()
    assert pn[1, 2, 3 * 2 + 1, 5] == psi[1, 2, 0, 1, 0, 1, 2, 1]                 # site ((t X + x) Y + y) Z + z
    assert torch.equal(ops.su3_spinor_unpack(pn, (2, 2, 2, 2)), psi)
    assert torch.equal(ops.sum_parts(torch.arange(7.0)[None]), torch.tensor([21.0]))
    # what raises before any kernel runs
    lat = LS(2, [2, 2, 2, 2])
    x = torch.zeros(2, 4, 2, 2, 2, 2, 3, 3, dtype=torch.complex128)
    xn = torch.zeros(2, 4, 9, 16, dtype=torch.complex128)
    for kap in (float('nan'), float('inf'), None, 'a'):
        with pytest.raises(ValueError, match='kappa'):
            lat.wilson_dirac(x, psi, kap)
        with pytest.raises(ValueError, match='kappa'):
            lat.wilson_solve_n(xn, pn, kap)
        with pytest.raises(ValueError, match='kappa'):
            lat.quark_propagator(x, kap)
    for wrong in (psi[:1], psi[..., :2], psi[:, :, :1], torch.zeros(2, 16, 12)):
        with pytest.raises(ValueError):
            lat.wilson_dirac(x, wrong, 0.1)
        with pytest.raises(ValueError):
            lat.wilson_solve(x, wrong, 0.1)
    for wrong in (pn[:1], pn[:, :, :11], pn[..., :15]):
        with pytest.raises(ValueError):
            lat.wilson_dirac_n(xn, wrong, 0.1)
    for kw in (dict(tol=0.0), dict(tol=-1.0), dict(tol=float('nan')), dict(max_iter=-1), dict(max_iter=1.5),
               dict(check_every=0), dict(check_every=2.5)):
        with pytest.raises(ValueError):
            lat.wilson_solve_n(xn, pn, 0.1, **kw)
    for src in ((2, 0, 0, 0), (0, 0, 0, -1), (0, 0, 0), (0, 0, 0, 0.5), None):
        with pytest.raises(ValueError, match='source'):
            lat.quark_propagator_n(xn, 0.1, source=src)
    # no autograd through any of them
    g, gn = x.clone().requires_grad_(True), xn.clone().requires_grad_(True)
    gp, gpn = psi.clone().requires_grad_(True), pn.clone().requires_grad_(True)
    for call in (lambda: lat.wilson_dirac(g, psi, 0.1), lambda: lat.wilson_dirac(x, gp, 0.1),
                 lambda: lat.wilson_dirac_n(gn, pn, 0.1), lambda: lat.wilson_dirac_n(xn, gpn, 0.1),
                 lambda: lat.wilson_solve(g, psi, 0.1), lambda: lat.wilson_solve(x, gp, 0.1),
                 lambda: lat.wilson_solve_n(gn, pn, 0.1), lambda: lat.wilson_solve_n(xn, gpn, 0.1),
                 lambda: lat.quark_propagator(g, 0.1), lambda: lat.quark_propagator_n(gn, 0.1)):
        with pytest.raises(RuntimeError, match='no autograd'):
            call()
