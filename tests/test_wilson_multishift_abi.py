"""CPU tier of the drop-in boundary of the multi-shift CG and the one-flavour RHMC: the exports of
csrc/su3_spinor_mshift.hip exist, agree with native.SIGNATURES and the header, and refuse bad arguments with an error text
before any HIP call; the Python surface on top of them is present, and what should raise does so before any kernel runs."""
import ctypes as C
import inspect

import pytest
import torch

P, L_, I = C.c_void_p, C.c_long, C.c_int
DECLS = {
    'l2q_su3_spinor_mshift_update': ((I, [P, P, P, P, P, P, P, P, P, L_, L_, L_, P]),
                                     'int l2q_su3_spinor_mshift_update(void* x, void* ps, void* p, const void* r, '
                                     'const double* a, const double* b, const double* zeta, const double* beta, '
                                     'const int* live, long nsys, long ns, long V, void* stream);'),
    'l2q_su3_spinor_axmy_norm': ((I, [P, P, P, P, L_, L_, P]),
                                 'int l2q_su3_spinor_axmy_norm(void* r, const void* z, const double* alpha, '
                                 'double* rr_part, long nsys, long V, void* stream);'),
    'l2q_su3_spinor_lincomb': ((I, [P, P, P, L_, L_, L_, P]),
                               'int l2q_su3_spinor_lincomb(const void* x, const double* w, void* out, long nsys, long ns, '
                               'long V, void* stream);'),
}
EINVAL = -1


def test_symbols_and_signatures():
    from l2hmc import native
    lib = native.load()
    flat = ' '.join(open(native.os.path.join(native._HERE, '..', '..', 'include', 'l2q.h')).read().split())
    for name, (sig, decl) in DECLS.items():
        assert hasattr(lib, name), name
        assert native.SIGNATURES[name] == sig, name
        assert decl in flat, name
        assert flat.index('int l2q_su3_spinor_xpay(') < flat.index(decl)


def checker(lib, name):
    def bad(rc, code, text):
        err = lib.l2q_last_error()
        assert rc == code and text in err and name.encode() in err, (name, rc, err)
    return bad


def test_argument_errors():
    """addresses are never dereferenced: every call is refused before a launch"""
    from l2hmc import native
    lib = native.load()
    M = 1 << 24                                                    # far apart: fields of 2 * 3 * 12 * 8 * 16 B = 9216 B
    x, ps, p, r, a, b, zeta, beta, live = (M * (i + 1) for i in range(9))
    ok = [x, ps, p, r, a, b, zeta, beta, live]
    name = 'l2q_su3_spinor_mshift_update'
    fn, bad = getattr(lib, name), checker(lib, name)
    for i in range(9):
        bad(fn(*[None if j == i else v for j, v in enumerate(ok)], 2, 3, 8, None), EINVAL, b'null pointer')
    one = 2 * 12 * 8 * 16                                          # bytes of an unshifted field; a shifted one: 3 x
    # r the same as, or inside, any x_k, p_k or p; and the written fields among themselves
    for rr in (x, x + one, x + 2 * one, x + 3 * one - 16, ps, ps + one, ps + 3 * one - 16, p, p + one - 16, x - one + 16):
        bad(fn(x, ps, p, rr, a, b, zeta, beta, live, 2, 3, 8, None), EINVAL, b'alias')
    assert fn(x, ps, p, x + 3 * one, a, b, zeta, beta, live, 0, 3, 8, None) == EINVAL          # adjacent is no alias: size
    for args in ((x, x, p), (x, x + one, p), (x, ps, x + 2 * one), (x, ps, ps)):
        bad(fn(*args, r, a, b, zeta, beta, live, 2, 3, 8, None), EINVAL, b'alias')
    for ns in (0, -1):
        bad(fn(*ok, 2, ns, 8, None), EINVAL, b'ns must be >= 1')
    for nsys, ns, V in ((0, 3, 8), (2, 3, 0), (-1, 3, 8), (1 << 10, 1 << 10, 1 << 10), (1 << 40, 1 << 40, 1), (4, 6, 1 << 23)):
        bad(fn(*ok, nsys, ns, V, None), EINVAL, b'size')

    name = 'l2q_su3_spinor_axmy_norm'
    fn, bad = getattr(lib, name), checker(lib, name)
    ok = [r, p, a, b]
    for i in range(4):
        bad(fn(*[None if j == i else v for j, v in enumerate(ok)], 2, 8, None), EINVAL, b'null pointer')
    bad(fn(r, r, a, b, 2, 8, None), EINVAL, b'alias')
    for nsys, V in ((0, 8), (2, 0), (-1, 8), (1 << 20, 1 << 20)):
        bad(fn(*ok, nsys, V, None), EINVAL, b'size')

    name = 'l2q_su3_spinor_lincomb'
    fn, bad = getattr(lib, name), checker(lib, name)
    ok = [x, a, p]
    for i in range(3):
        bad(fn(*[None if j == i else v for j, v in enumerate(ok)], 2, 3, 8, None), EINVAL, b'null pointer')
    for out in (x, x + one, x + 3 * one - 16):
        bad(fn(x, a, out, 2, 3, 8, None), EINVAL, b'alias')
    bad(fn(*ok, 2, 0, 8, None), EINVAL, b'ns must be >= 1')
    for nsys, ns, V in ((0, 3, 8), (2, 3, 0), (1 << 10, 1 << 10, 1 << 10), (4, 6, 1 << 23)):
        bad(fn(*ok, nsys, ns, V, None), EINVAL, b'size')


def test_python_surface():
    from l2hmc import _ops as ops
    from l2hmc.dynamics.pytorch.fermion_hmc import WilsonHMCEvenOdd, WilsonRHMC
    from l2hmc.lattice.su3.pytorch import rational, wilson
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3 as LS
    for name in ('su3_spinor_mshift_update_', 'su3_spinor_axmy_norm_', 'su3_spinor_lincomb'):
        assert callable(getattr(ops, name)), name
    q = inspect.signature(LS.wilson_solve_multishift_n).parameters
    assert list(q)[1:10] == ['xn', 'phi_e', 'kappa', 'shifts', 'tol', 'max_iter', 'check_every', 'antiperiodic_t', 'clover']
    assert [q[k].default for k in ('tol', 'max_iter', 'check_every', 'antiperiodic_t', 'clover')] == [1e-10, 1000, 10, True, None]
    r = inspect.signature(LS.wilson_solve_multishift).parameters
    assert list(r)[3:] == list(q)[3:]
    for name in ('rhmc_pseudofermion_refresh', 'rhmc_pseudofermion_action', 'rhmc_pseudofermion_force', 'schur_spectrum_n'):
        assert callable(getattr(LS, name)), name
    assert list(inspect.signature(LS.rhmc_pseudofermion_refresh_n).parameters)[1:7] == [
        'xn', 'kappa', 'rat', 'npf', 'generator', 'antiperiodic_t']
    assert callable(wilson._CG.multishift) and issubclass(WilsonRHMC, WilsonHMCEvenOdd)
    # the pinned signatures of the existing solvers are what they were
    assert list(inspect.signature(wilson._CG.normal).parameters) == ['self', 'final']
    assert list(inspect.signature(wilson._CG.iterations).parameters) == ['self', 'rnorm']
    lat = LS(2, [2, 2, 2, 2])
    rat = rational.zolotarev_inv_sqrt(4, 0.05, 4.0)
    h = WilsonRHMC(lat, 5.5, 0.12, 0.05, 4, rat=rat, kappa_light=0.11)
    assert h.kappa_light == 0.11 and h.rat is rat and h.even_odd is True
    assert WilsonRHMC(lat, 5.5, 0.12, 0.05, 4, rat=rat).kappa_light is None
    with pytest.raises(ValueError, match='rat must be'):
        WilsonRHMC(lat, 5.5, 0.12, 0.05, 4, rat=None)
    with pytest.raises(ValueError, match='kappa_light'):
        WilsonRHMC(lat, 5.5, 0.12, 0.05, 4, rat=rat, kappa_light=float('nan'))
    with pytest.raises(ValueError, match='even extents'):
        WilsonRHMC(LS(2, [3, 2, 2, 2]), 5.5, 0.12, 0.05, 4, rat=rat)


def test_what_raises_before_any_kernel(monkeypatch):
    from l2hmc import _ops as ops
    from l2hmc import native
    from l2hmc.lattice.su3.pytorch import rational
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3 as LS

    def no_kernel(name, *args):
        raise AssertionError(f'{name} was called')
    monkeypatch.setattr(native, 'call', no_kernel)
    c128 = torch.complex128
    lat = LS(2, [2, 2, 2, 2])
    rat = rational.zolotarev_inv_sqrt(2, 0.05, 4.0)
    xn, x = torch.zeros(2, 4, 9, 16, dtype=c128), torch.zeros(2, 4, 2, 2, 2, 2, 3, 3, dtype=c128)
    hn, fn = torch.zeros(2, 1, 12, 8, dtype=c128), torch.zeros(2, 1, 12, 16, dtype=c128)
    f = torch.zeros(2, 1, 2, 2, 2, 2, 4, 3, dtype=c128)
    for shifts in ([], None, [0.1, -0.2], [float('nan')], [float('inf')], ['a'], 0.3):
        with pytest.raises(ValueError, match=r'wilson_solve_multishift: shifts must be a non-empty sequence'):
            lat.wilson_solve_multishift_n(xn, hn, 0.1, shifts)
        with pytest.raises(ValueError, match=r'wilson_solve_multishift: shifts must be a non-empty sequence'):
            lat.wilson_solve_multishift(x, f, 0.1, shifts)
    for kw in (dict(tol=0.0), dict(max_iter=-1), dict(check_every=0)):
        with pytest.raises(ValueError, match=r'LatticeSU3\.wilson_solve_multishift: need tol > 0'):
            lat.wilson_solve_multishift_n(xn, hn, 0.1, [0.1], **kw)
    with pytest.raises(ValueError, match='half field'):
        lat.wilson_solve_multishift_n(xn, fn, 0.1, [0.1])
    with pytest.raises(ValueError, match='autograd'):
        lat.wilson_solve_multishift_n(xn.clone().requires_grad_(True), hn, 0.1, [0.1])
    with pytest.raises(ValueError, match='kappa must be a finite number'):
        lat.wilson_solve_multishift_n(xn, hn, float('inf'), [0.1])
    with pytest.raises(ValueError, match='clover= must be'):
        lat.wilson_solve_multishift_n(xn, hn, 0.1, [0.1], clover='no')
    odd = LS(2, [3, 4, 5, 2])
    oxn, ohn = torch.zeros(2, 4, 9, 120, dtype=c128), torch.zeros(2, 1, 12, 60, dtype=c128)
    for call in (lambda: odd.wilson_solve_multishift_n(oxn, ohn, 0.1, [0.1]),
                 lambda: odd.rhmc_pseudofermion_refresh_n(oxn, 0.1, rat),
                 lambda: odd.rhmc_pseudofermion_action_n(oxn, ohn, 0.1, rat),
                 lambda: odd.rhmc_pseudofermion_force_n(oxn, ohn, 0.1, rat),
                 lambda: odd.schur_spectrum_n(oxn, 0.1)):
        with pytest.raises(ValueError, match=r'even extents.*\[3, 4, 5, 2\]'):
            call()
    for call in (lambda: lat.rhmc_pseudofermion_refresh_n(xn, 0.1, 'r'), lambda: lat.rhmc_pseudofermion_action_n(xn, hn, 0.1, 3),
                 lambda: lat.rhmc_pseudofermion_force_n(xn, hn, 0.1, None)):
        with pytest.raises(ValueError, match='rat must be'):
            call()
    with pytest.raises(ValueError, match='npf must be'):
        lat.rhmc_pseudofermion_refresh_n(xn, 0.1, rat, npf=0)
    with pytest.raises(ValueError, match='iters must be'):
        lat.schur_spectrum_n(xn, 0.1, iters=0)
    # the wrappers are strict about dtype, shape and contiguity
    X, p = torch.zeros(2, 2, 3, 12, 8, dtype=c128), torch.zeros(2, 2, 12, 8, dtype=c128)
    s3, s2 = torch.zeros(2, 2, 3, dtype=torch.float64), torch.zeros(2, 2, dtype=torch.float64)
    lv = torch.ones(2, 2, 3, dtype=torch.int32)
    bad = [lambda: ops.su3_spinor_mshift_update_(X.to(torch.complex64), X.clone(), p, p.clone(), s3, s3, s3, s2, lv),
           lambda: ops.su3_spinor_mshift_update_(X, X.clone()[:, :, :2], p, p.clone(), s3, s3, s3, s2, lv),
           lambda: ops.su3_spinor_mshift_update_(X, X.clone(), p[..., :7], p.clone(), s3, s3, s3, s2, lv),
           lambda: ops.su3_spinor_mshift_update_(X, X.clone(), p, p.clone(), s3, s2, s3, s2, lv),
           lambda: ops.su3_spinor_mshift_update_(X, X.clone(), p, p.clone(), s3, s3, s3, s3, lv),
           lambda: ops.su3_spinor_mshift_update_(X, X.clone(), p, p.clone(), s3, s3, s3, s2, lv.to(torch.int64)),
           lambda: ops.su3_spinor_mshift_update_(X, X.clone(), p, p.clone(), s3, s3, s3, s2, lv.bool()),
           lambda: ops.su3_spinor_mshift_update_(p, p.clone(), p, p.clone(), s3, s3, s3, s2, lv),
           lambda: ops.su3_spinor_axmy_norm_(p, p.clone(), s3), lambda: ops.su3_spinor_axmy_norm_(p, X, s2),
           lambda: ops.su3_spinor_axmy_norm_(p, p.clone(), s2, part=torch.zeros(2, 2, 2, dtype=torch.float64)),
           lambda: ops.su3_spinor_lincomb(p, s3), lambda: ops.su3_spinor_lincomb(X, s2),
           lambda: ops.su3_spinor_lincomb(X, s3, out=X.clone())]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
