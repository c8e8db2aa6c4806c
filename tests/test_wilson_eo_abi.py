"""CPU tier of the drop-in boundary of even-odd preconditioning: the export of csrc/su3_wilson_eo.hip exists, agrees with
native.SIGNATURES and the header, and refuses bad arguments with an error text before any HIP call; the Python surface on
top of it is present and opt-in, and what should raise does so before any kernel runs."""
import inspect

import pytest
import torch

NAME = 'l2q_su3_wilson_hop_eo'


def test_symbol_and_signature():
    import ctypes as C
    from l2hmc import native
    lib = native.load()
    P, I, D = C.c_void_p, C.c_int, C.c_double
    assert hasattr(lib, NAME)
    assert native.SIGNATURES[NAME] == (I, [P, P, P, P, P, D, D, I, I, I, I, I, I, I, I, P])
    header = open(native.os.path.join(native._HERE, '..', '..', 'include', 'l2q.h')).read()
    flat = ' '.join(header.split())
    decl = ('int l2q_su3_wilson_hop_eo(const void* xn, const void* src, const void* aux, void* out, double* norm_part, '
            'double a, double b, int flags, int parity, int nb, int nrhs, int T, int X, int Y, int Z, void* stream);')
    assert decl in flat
    assert flat.index('int l2q_su3_wilson_force(') < flat.index(decl)


def test_argument_errors():
    from l2hmc import native
    lib = native.load()
    hop = getattr(lib, NAME)
    # (addresses are never dereferenced: every check below comes before any HIP call)
    x, s, a, o, n = 4096, 8192, 12288, 16384, 20480
    nan, inf = float('nan'), float('inf')

    def call(**kw):
        p = {**dict(xn=x, src=s, aux=a, out=o, part=n, a=0.5, b=1.0, flags=2, parity=0, nb=1, nrhs=2, T=2, X=4, Y=2, Z=6),
             **kw}
        return hop(p['xn'], p['src'], p['aux'], p['out'], p['part'], p['a'], p['b'], p['flags'], p['parity'], p['nb'],
                   p['nrhs'], p['T'], p['X'], p['Y'], p['Z'], None)

    def bad(rc, code, text):
        err = lib.l2q_last_error()
        assert rc == code and text in err and NAME.encode() in err, (rc, err)

    EINVAL, ESHAPE = -1, -2
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
               dict(T=1 << 12, X=1 << 12, Y=8),                       # the links of a chain past an int
               dict(nb=64, nrhs=12, T=32, X=32, Y=32, Z=8)):          # nb * nrhs * 12 * V = 2.4e9 past an int
        bad(call(**kw), EINVAL, b'size')
    for kw in (dict(T=3), dict(X=1), dict(Y=5), dict(Z=7), dict(T=1, X=1, Y=1, Z=1)):
        bad(call(**kw), ESHAPE, b'needs even extents')


def test_error_codes_are_the_headers():
    from l2hmc import native
    header = open(native.os.path.join(native._HERE, '..', '..', 'include', 'l2q.h')).read()
    flat = ' '.join(header.split())
    assert '#define L2Q_EINVAL (-1)' in flat and '#define L2Q_ESHAPE (-2)' in flat


def test_python_surface():
    from l2hmc import _ops as ops
    from l2hmc.dynamics.pytorch.fermion_hmc import WilsonHMC, WilsonHMCEvenOdd
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3 as LS
    p = inspect.signature(ops.su3_wilson_hop_eo_n).parameters
    assert list(p) == ['xn', 'src', 'lat', 'parity', 'dagger', 'antiperiodic_t', 'a', 'aux', 'b', 'out', 'norm']
    assert [p[k].default for k in list(p)[4:]] == [False, True, 1.0, None, 0.0, None, False]
    assert callable(ops.su3_spinor_split_eo) and callable(ops.su3_spinor_merge_eo)
    # even-odd is opt-in everywhere: the unpreconditioned entry points keep their signatures, the preconditioned ones
    # mirror them, `even_odd` travels in the keywords of those that forward keywords and defaults to False
    for name in ('wilson_solve', 'wilson_solve_n', 'pseudofermion_refresh', 'pseudofermion_refresh_n'):
        base = name[:-2] if name.endswith('_n') else name
        twin = base + '_eo' + ('_n' if name.endswith('_n') else '')
        assert 'even_odd' not in inspect.signature(getattr(LS, name)).parameters
        assert str(inspect.signature(getattr(LS, twin))) == str(inspect.signature(getattr(LS, name))), name
    for name in ('pseudofermion_action', 'pseudofermion_force', 'quark_propagator'):
        for fn in (getattr(LS, name), getattr(LS, name + '_n')):
            assert list(inspect.signature(fn).parameters)[-1] == 'solve_kwargs', name
    assert WilsonHMC.even_odd is False and WilsonHMCEvenOdd.even_odd is True and issubclass(WilsonHMCEvenOdd, WilsonHMC)
    assert inspect.signature(WilsonHMCEvenOdd.__init__) == inspect.signature(WilsonHMC.__init__)
    for fn in (LS.wilson_schur, LS.wilson_schur_n):
        q = inspect.signature(fn).parameters
        assert list(q)[3:] == ['kappa', 'dagger', 'antiperiodic_t'] and q['dagger'].default is False
    q = inspect.signature(LS.wilson_solve_schur_normal_n).parameters
    assert list(q)[1:] == ['xn', 'phi_e', 'kappa', 'tol', 'max_iter', 'check_every', 'antiperiodic_t']
    assert [q[k].default for k in list(q)[4:]] == [1e-10, 1000, 10, True]
    # split and merge on the host: inverse to each other, entry h of a half is the site 2h or 2h + 1 of that parity
    L = (2, 4, 2, 6)
    V = 96
    pn = torch.arange(2 * 3 * 12 * V, dtype=torch.float64).reshape(2, 3, 12, V).to(torch.complex128)
    e, o = ops.su3_spinor_split_eo(pn, L)
    assert e.shape == o.shape == (2, 3, 12, V // 2) and e.is_contiguous() and o.is_contiguous()
    assert torch.equal(ops.su3_spinor_merge_eo(e, o, L), pn)
    se, so = ops.su3_eo_sites(L, 'cpu')
    assert torch.equal(se >> 1, torch.arange(V // 2)) and torch.equal(so >> 1, torch.arange(V // 2))
    s = int(se[17])
    t, r = divmod(s, 48)
    xx, r = divmod(r, 12)
    yy, zz = divmod(r, 6)
    assert (t + xx + yy + zz) % 2 == 0 and e[1, 2, 5, 17] == pn[1, 2, 5, s]
    assert ops.su3_eo_sites(L, 'cpu')[0] is se                                   # cached
    # odd extents: ValueError naming the lattice, before any kernel runs
    odd = LS(2, [3, 4, 5, 2])
    xn = torch.zeros(2, 4, 9, 120, dtype=torch.complex128)
    x = torch.zeros(2, 4, 3, 4, 5, 2, 3, 3, dtype=torch.complex128)
    fn = torch.zeros(2, 1, 12, 120, dtype=torch.complex128)
    hn = torch.zeros(2, 1, 12, 60, dtype=torch.complex128)
    f = torch.zeros(2, 1, 3, 4, 5, 2, 4, 3, dtype=torch.complex128)
    for call in (lambda: odd.wilson_solve_eo_n(xn, fn, 0.1), lambda: odd.wilson_solve_eo(x, f, 0.1),
                 lambda: odd.quark_propagator_n(xn, 0.1, even_odd=True),
                 lambda: odd.wilson_schur_n(xn, hn, 0.1), lambda: odd.wilson_schur(x, f, 0.1),
                 lambda: odd.wilson_solve_schur_normal_n(xn, hn, 0.1),
                 lambda: odd.pseudofermion_refresh_eo_n(xn, 0.1), lambda: odd.pseudofermion_refresh_eo(x, 0.1),
                 lambda: odd.pseudofermion_action_n(xn, hn, 0.1, even_odd=True),
                 lambda: odd.pseudofermion_action(x, f, 0.1, even_odd=True),
                 lambda: odd.pseudofermion_force_n(xn, hn, 0.1, even_odd=True),
                 lambda: odd.pseudofermion_force(x, f, 0.1, even_odd=True),
                 lambda: WilsonHMCEvenOdd(odd, 5.5, 0.1, 0.05, 4),
                 lambda: ops.su3_wilson_hop_eo_n(xn, hn, (3, 4, 5, 2), 0),
                 lambda: ops.su3_spinor_split_eo(fn, (3, 4, 5, 2)), lambda: ops.su3_spinor_merge_eo(hn, hn, (3, 4, 5, 2))):
        with pytest.raises(ValueError, match=r'even extents.*\[3, 4, 5, 2\]'):
            call()
    assert WilsonHMC(odd, 5.5, 0.1, 0.05, 4).even_odd is False
    # wrong half-field shapes
    lat = LS(2, [2, 2, 2, 2])
    xn = torch.zeros(2, 4, 9, 16, dtype=torch.complex128)
    half = torch.zeros(2, 3, 12, 8, dtype=torch.complex128)
    for wrong in (half[:1], half[:, :, :11], half[..., :7], torch.zeros(2, 3, 12, 16, dtype=torch.complex128),
                  torch.zeros(2, 8, 12)):
        for call in (lambda w: lat.wilson_schur_n(xn, w, 0.1), lambda w: lat.wilson_solve_schur_normal_n(xn, w, 0.1),
                     lambda w: lat.pseudofermion_action_n(xn, w, 0.1, even_odd=True),
                     lambda w: lat.pseudofermion_force_n(xn, w, 0.1, even_odd=True)):
            with pytest.raises(ValueError, match='half field'):
                call(wrong)
    with pytest.raises(ValueError):
        ops.su3_wilson_hop_eo_n(xn, half[..., :7], (2, 2, 2, 2), 0)
    with pytest.raises(ValueError, match='parity'):
        ops.su3_wilson_hop_eo_n(xn, half, (2, 2, 2, 2), 2)
    with pytest.raises(ValueError, match='aux'):
        ops.su3_wilson_hop_eo_n(xn, half, (2, 2, 2, 2), 0, aux=half[:, :2])
    with pytest.raises(ValueError, match='out'):
        ops.su3_wilson_hop_eo_n(xn, half, (2, 2, 2, 2), 0, out=half.to(torch.complex64))
    with pytest.raises(ValueError, match='norm'):
        ops.su3_wilson_hop_eo_n(xn, half, (2, 2, 2, 2), 0, norm=torch.zeros(2, 3, 2, dtype=torch.float64))
    for kw in (dict(tol=0.0), dict(max_iter=-1), dict(check_every=0)):
        with pytest.raises(ValueError):
            lat.wilson_solve_schur_normal_n(xn, half, 0.1, **kw)
        with pytest.raises(ValueError):
            lat.wilson_solve_eo_n(xn, torch.zeros(2, 3, 12, 16, dtype=torch.complex128), 0.1, **kw)
    for kap in (float('nan'), None):
        with pytest.raises(ValueError, match='kappa'):
            lat.wilson_schur_n(xn, half, kap)
    # tensors that require grad
    gx, gh = xn.clone().requires_grad_(True), half.clone().requires_grad_(True)
    for call in (lambda: lat.wilson_schur_n(gx, half, 0.1), lambda: lat.wilson_schur_n(xn, gh, 0.1),
                 lambda: lat.wilson_solve_schur_normal_n(gx, half, 0.1), lambda: lat.wilson_solve_schur_normal_n(xn, gh, 0.1),
                 lambda: lat.pseudofermion_action_n(xn, gh, 0.1, even_odd=True),
                 lambda: lat.pseudofermion_force_n(gx, half, 0.1, even_odd=True),
                 lambda: lat.pseudofermion_refresh_eo_n(gx, 0.1)):
        with pytest.raises(ValueError, match='autograd'):
            call()
