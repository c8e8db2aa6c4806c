"""CPU tier of the drop-in boundary of the dynamical Wilson fermions: the export of csrc/su3_wilson_force.hip exists,
agrees with native.SIGNATURES and the header, and refuses bad arguments with an error text before any HIP call; the
Python surface on top of it is present and raises ValueError where it should before any kernel runs."""
import inspect

import pytest
import torch

NAME = 'l2q_su3_wilson_force'


def test_force_symbol_and_signature():
    import ctypes as C
    from l2hmc import native
    lib = native.load()
    P, I, D = C.c_void_p, C.c_int, C.c_double
    assert hasattr(lib, NAME)
    assert native.SIGNATURES[NAME] == (I, [P, P, P, P, P, D, D, I, I, I, I, I, I, I, P])
    header = open(native.os.path.join(native._HERE, '..', '..', 'include', 'l2q.h')).read()
    flat = ' '.join(header.split())
    assert ('int l2q_su3_wilson_force(const void* xn, const void* X, const void* Y, const void* f_in, void* f_out, '
            'double kappa, double coef, int flags, int nb, int npf, int T, int X_, int Y_, int Z, void* stream);') in flat
    assert flat.index('SU(3) Wilson fermions') < flat.index('int l2q_su3_wilson_force(') < flat.index('L2HMC momentum update')


def test_force_argument_errors():
    from l2hmc import native
    lib = native.load()
    force = getattr(lib, NAME)
    # (addresses are never dereferenced: every check below comes before any HIP call)
    x, a, b, c, d = 4096, 8192, 12288, 16384, 20480
    nan, inf = float('nan'), float('inf')

    def bad(rc, text):
        err = lib.l2q_last_error()
        assert rc == -1 and text in err and NAME.encode() in err, (rc, err)

    def f(**kw):
        p = {**dict(xn=x, X=a, Y=b, f_in=c, f_out=d, kappa=0.12, coef=-0.05, flags=2, nb=1, npf=2, T=3, X_=1, Y_=2, Z=5),
             **kw}
        return force(p['xn'], p['X'], p['Y'], p['f_in'], p['f_out'], p['kappa'], p['coef'], p['flags'], p['nb'], p['npf'],
                     p['T'], p['X_'], p['Y_'], p['Z'], None)

    for k in ('xn', 'X', 'Y', 'f_out'):
        bad(f(**{k: None}), b'null pointer')
    for other in (x, a, b):
        bad(f(f_out=other), b'alias')
    for kw in (dict(kappa=nan), dict(kappa=inf), dict(kappa=-inf)):
        bad(f(**kw), b'kappa')
    for kw in (dict(coef=nan), dict(coef=inf), dict(coef=-inf)):
        bad(f(**kw), b'coef')
    for kw in (dict(npf=0), dict(npf=-1), dict(nb=0), dict(nb=-2), dict(T=0), dict(X_=-3), dict(Y_=0), dict(Z=0),
               dict(T=1 << 12, X_=1 << 12, Y_=8),                     # the links of a chain past an int (su3_dims_ok)
               dict(nb=64, npf=12, T=32, X_=32, Y_=32, Z=8)):         # nb * npf * 12 * V = 2.4e9 past an int
        bad(f(**kw), b'size')
    for fl in (-1, 1, 3, 4, 6, 1 << 20):
        bad(f(flags=fl), b'flags')


def test_force_python_surface():
    from l2hmc import _ops as ops
    from l2hmc.dynamics.pytorch.fermion_hmc import WilsonHMC
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3 as LS
    from l2hmc.lattice.u1.pytorch.lattice import LatticeU1
    p = inspect.signature(ops.su3_wilson_force_n).parameters
    assert list(p) == ['xn', 'X', 'Y', 'kappa', 'lat', 'antiperiodic_t', 'coef', 'f_in', 'out']
    assert (p['coef'].default, p['f_in'].default, p['out'].default) == (1.0, None, None)

    def names(fn):
        return list(inspect.signature(fn).parameters)[2:]
    assert names(LS.wilson_solve_normal)[1:] == names(LS.wilson_solve_normal_n)[1:] == \
        ['kappa', 'tol', 'max_iter', 'check_every', 'antiperiodic_t']
    assert [v.default for v in inspect.signature(LS.wilson_solve_normal_n).parameters.values()][4:] == [1e-10, 1000, 10, True]
    assert names(LS.pseudofermion_refresh) == names(LS.pseudofermion_refresh_n) == ['kappa', 'npf', 'generator', 'antiperiodic_t']
    for name in ('pseudofermion_action', 'pseudofermion_force'):
        assert names(getattr(LS, name))[1:] == names(getattr(LS, name + '_n'))[1:] == ['kappa', 'solve_kwargs']
        assert not hasattr(LatticeU1, name)
    assert list(inspect.signature(WilsonHMC.__init__).parameters)[1:] == \
        ['lattice', 'beta', 'kappa', 'eps', 'nleapfrog', 'npf', 'tol_md', 'tol_h', 'max_iter', 'antiperiodic_t']
    for name in ('leapfrog_n', 'hamiltonian_n', 'trajectory', 'thermalize'):
        assert callable(getattr(WilsonHMC, name)), name
    # what raises before any kernel runs
    lat = LS(2, [2, 2, 2, 2])
    x = torch.zeros(2, 4, 2, 2, 2, 2, 3, 3, dtype=torch.complex128)
    xn = torch.zeros(2, 4, 9, 16, dtype=torch.complex128)
    phi = torch.zeros(2, 3, 2, 2, 2, 2, 4, 3, dtype=torch.complex128)
    pn = torch.zeros(2, 3, 12, 16, dtype=torch.complex128)
    for kap in (float('nan'), float('inf'), None, 'a'):
        for call in (lambda: lat.wilson_solve_normal_n(xn, pn, kap), lambda: lat.wilson_solve_normal(x, phi, kap),
                     lambda: lat.pseudofermion_refresh_n(xn, kap), lambda: lat.pseudofermion_refresh(x, kap),
                     lambda: lat.pseudofermion_action_n(xn, pn, kap), lambda: lat.pseudofermion_action(x, phi, kap),
                     lambda: lat.pseudofermion_force_n(xn, pn, kap), lambda: lat.pseudofermion_force(x, phi, kap)):
            with pytest.raises(ValueError, match='kappa'):
                call()
    for wrong in (phi[:1], phi[..., :2], phi[:, :, :1], torch.zeros(2, 16, 12)):
        for fn in (lat.wilson_solve_normal, lat.pseudofermion_action, lat.pseudofermion_force):
            with pytest.raises(ValueError):
                fn(x, wrong, 0.1)
    for wrong in (pn[:1], pn[:, :, :11], pn[..., :15]):
        for fn in (lat.wilson_solve_normal_n, lat.pseudofermion_action_n, lat.pseudofermion_force_n):
            with pytest.raises(ValueError):
                fn(xn, wrong, 0.1)
    for wrong in (pn[:1], pn[:, :0], pn[:, :, :11], pn[..., :15], pn.to(torch.complex64)):
        with pytest.raises(ValueError):
            ops.su3_wilson_force_n(xn, wrong, wrong, 0.1, (2, 2, 2, 2))
    with pytest.raises(ValueError):
        ops.su3_wilson_force_n(xn, pn, pn, 0.1, (2, 2, 2, 2), f_in=xn[:1])
    for npf in (0, -1, 1.5, None, True):
        with pytest.raises(ValueError, match='npf'):
            lat.pseudofermion_refresh_n(xn, 0.1, npf)
    for kw in (dict(tol=0.0), dict(tol=-1.0), dict(tol=float('nan')), dict(max_iter=-1), dict(max_iter=1.5),
               dict(check_every=0), dict(check_every=2.5)):
        for fn in (lat.wilson_solve_normal_n, lat.pseudofermion_action_n, lat.pseudofermion_force_n):
            with pytest.raises(ValueError):
                fn(xn, pn, 0.1, **kw)
    # no autograd through any of them: a ValueError
    g, gn = x.clone().requires_grad_(True), xn.clone().requires_grad_(True)
    gp, gpn = phi.clone().requires_grad_(True), pn.clone().requires_grad_(True)
    for call in (lambda: lat.wilson_solve_normal(g, phi, 0.1), lambda: lat.wilson_solve_normal(x, gp, 0.1),
                 lambda: lat.wilson_solve_normal_n(gn, pn, 0.1), lambda: lat.wilson_solve_normal_n(xn, gpn, 0.1),
                 lambda: lat.pseudofermion_refresh(g, 0.1), lambda: lat.pseudofermion_refresh_n(gn, 0.1),
                 lambda: lat.pseudofermion_action(g, phi, 0.1), lambda: lat.pseudofermion_action_n(xn, gpn, 0.1),
                 lambda: lat.pseudofermion_force(x, gp, 0.1), lambda: lat.pseudofermion_force_n(gn, pn, 0.1)):
        with pytest.raises(ValueError, match='autograd'):
            call()
    # the trajectory's parameters
    for kw in (dict(kappa=float('nan')), dict(beta=float('inf')), dict(eps=None), dict(nleapfrog=0), dict(nleapfrog=2.5),
               dict(npf=0), dict(tol_md=0.0), dict(tol_h=-1.0), dict(max_iter=-1)):
        with pytest.raises(ValueError):
            WilsonHMC(**{**dict(lattice=lat, beta=5.5, kappa=0.12, eps=0.05, nleapfrog=4), **kw})
    with pytest.raises(ValueError):
        WilsonHMC(LatticeU1(2, [4, 4]), 5.5, 0.12, 0.05, 4)
    hmc = WilsonHMC(lat, 5.5, 0.12, 0.05, 4)
    with pytest.raises(ValueError, match='autograd'):
        hmc.trajectory(g)
