"""GPU tier of the adaptive-step Wilson flow: the kernel behind l2q_su3_flow_step_err, the controller-driven flow and
the t0 / w0 scale setting of LatticeSU3 on top of it, against the independent restatements tests/flow_restatement.py and
tests/flow_adaptive_restatement.py (torch on the CPU; validated on their own in tests/test_flow_host.py and
tests/test_flow_adaptive_host.py)."""
import numpy as np
import pytest
import torch

import flow_adaptive_restatement as far
import flow_restatement as fr

pytestmark = pytest.mark.gpu

LATTICES = [(2, 2, 2, 2), (1, 3, 2, 5), (4, 4, 4, 4), (3, 5, 2, 7), (2, 4, 4, 12)]
L4 = (4, 4, 4, 4)


@pytest.fixture(scope='module')
def ops():
    from l2hmc import _ops
    return _ops


def lattice(nb, L):
    from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
    return LatticeSU3(nb, list(L))


def dev(a):
    a = a.numpy() if isinstance(a, torch.Tensor) else a
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu()


def err(a, b):
    return float((torch.as_tensor(a) - torch.as_tensor(b)).abs().max())


@pytest.fixture(scope='module')
def x4():
    """the input of tests 2 - 5: 4^4, two chains, never written"""
    return fr.rand_su3((2, 4, *L4), 2.0, torch.Generator().manual_seed(5))


def step_err(ops, xn, eps, L):
    """one step with fresh NaN-filled buffers -> (x_out, d)"""
    out, ws_x = (torch.full_like(xn, float('nan')) for _ in range(2))
    ws_p3 = torch.full((3, *xn.shape), float('nan'), dtype=xn.dtype, device=xn.device)
    d = ops.su3_flow_step_err_n(xn, out, ws_p3, ws_x, eps, L)
    return out, d


def replay(x, eps_list):
    """the restated steps of the given sizes -> (flowed x, d [n, nb])"""
    ds = []
    for e in eps_list:
        x, d = far.flow_step_err(x, e)
        ds.append(d)
    return x, torch.stack(ds)


def growth(x, eps_list, gen):
    """the yardstick's own response to a 1e-9 perturbation of the start (the helper of tests/test_flow_gpu.py, for
    steps of the given sizes): A = growth of the link difference"""
    xp = torch.matrix_exp(1e-9 * fr.tah(torch.complex(torch.randn(x.shape, dtype=torch.float64, generator=gen),
                                                      torch.randn(x.shape, dtype=torch.float64, generator=gen)))) @ x
    d0 = float((xp - x).abs().max())
    y, yp = x, xp
    for e in eps_list:
        y, yp = fr.flow_step(y, e), fr.flow_step(yp, e)
    return float((yp - y).abs().max()) / d0


# ------------------------------------------------------------------ 1. one step
@pytest.mark.parametrize('L', LATTICES)
def test_one_step_with_error(ops, L):
    nb, eps = 3, 0.02
    x = fr.rand_su3((nb, 4, *L), 3.0, torch.Generator().manual_seed(17))
    xn = ops.su3_pack(dev(x))
    keep = xn.clone()
    out, d = step_err(ops, xn, eps, L)
    want_x, want_d = far.flow_step_err(x, eps)
    # the step itself: the existing kernels up to the one hosting the last product
    ref = ops.su3_flow_step_n(xn, torch.empty_like(xn), torch.empty_like(xn), torch.empty_like(xn), eps, L)
    e_ref, e_x, e_d = err(host(out), host(ref)), err(host(ops.su3_unpack(out, L)), want_x), err(host(d), want_d)
    print(f'L={L}: |x_out - flow_step| = {e_ref:.2e} |x_out - restatement| = {e_x:.2e} d = {host(d).tolist()} '
          f'|dd| = {e_d:.2e}')
    assert e_ref <= 1e-15
    assert e_x <= 1e-13 and e_d <= 1e-13
    assert torch.equal(xn, keep)                                   # the input is never written
    # a chain alone equals the same chain in the batch, bit for bit
    for k in range(nb):
        o1, d1 = step_err(ops, xn[k:k + 1].contiguous(), eps, L)
        assert torch.equal(o1[0], out[k]) and torch.equal(d1[0], d[k])
    # a link that is not finite: +inf for its chain, the other chains untouched
    bad = xn.clone()
    bad[1, 2, 4, int(np.prod(L)) - 1] = complex(float('nan'), 0.0)
    ob, db = step_err(ops, bad, eps, L)
    assert float(db[1]) == float('inf') and torch.equal(db[[0, 2]], d[[0, 2]]) and torch.equal(ob[[0, 2]], out[[0, 2]])


def test_step_argument_errors(ops):
    from l2hmc import native
    L, nb = (2, 2, 2, 2), 1
    xn = ops.su3_pack(dev(fr.rand_su3((nb, 4, *L), 1.0, torch.Generator().manual_seed(1))))
    out, ws_x, ws_p3 = torch.empty_like(xn), torch.empty_like(xn), torch.empty((3, *xn.shape), dtype=xn.dtype).cuda()
    d = torch.empty(nb, dtype=torch.float64).cuda()
    need = int(native.load().l2q_su3_flow_step_err_ws_bytes(nb, *L))
    assert need == nb * 4 * 1 * 8
    ws = torch.empty(need, dtype=torch.uint8).cuda()

    def rc(x_in, x_out, p3, wx, dd, w, nbytes):
        p = [native.ptr(a) if a is not None else None for a in (x_in, x_out, p3, wx)]
        return native.load().l2q_su3_flow_step_err(p[0], p[1], p[2], p[3], 0.01, None if dd is None else native.ptr(dd),
                                                   nb, *L, None if w is None else native.ptr(w), nbytes, None)
    assert rc(xn, out, ws_p3, ws_x, d, ws, need) == 0
    torch.cuda.synchronize()
    for a in ((None, out, ws_p3, ws_x, d, ws), (xn, None, ws_p3, ws_x, d, ws), (xn, out, None, ws_x, d, ws),
              (xn, out, ws_p3, None, d, ws), (xn, out, ws_p3, ws_x, None, ws), (xn, out, ws_p3, ws_x, d, None),
              (xn, xn, ws_p3, ws_x, d, ws), (xn, out, ws_p3, out, d, ws), (xn, out, ws_p3, xn, d, ws),
              (xn, ws_p3[1], ws_p3, ws_x, d, ws), (xn, out, ws_p3, ws_p3[2], d, ws), (ws_p3[0], out, ws_p3, ws_x, d, ws)):
        assert rc(*a, need) == -1, [None if t is None else t.data_ptr() for t in a]          # L2Q_EINVAL
    assert b'l2q_su3_flow_step_err' in native.load().l2q_last_error()
    assert rc(xn, out, ws_p3, ws_x, d, ws, need - 1) == -2                                    # L2Q_ESHAPE
    with pytest.raises(ValueError):
        ops.su3_flow_step_err_n(xn, out, ws_p3[:2], ws_x, 0.01, L)


# ------------------------------------------------------------------ 2. an adaptive run on the same steps
def test_adaptive_run_vs_restatement(ops, x4):
    """links within 3 n 1e-13 max(1, A) of the restatement replaying the step sizes the run chose, every d within
    1e-13 max(1, A).  Measured with the restatement alone: 37 steps, none rejected, the largest d 9.1e-6."""
    t, tol = 0.6, 1e-5
    lat = lattice(2, L4)
    xn = ops.su3_pack(dev(x4))
    keep = xn.clone()
    yn, info = lat.flow_adaptive_n(xn, t, tol=tol)
    eps, d = info['eps'], info['d']
    n = info['nsteps']
    assert set(info) == {'eps', 'd', 'nsteps', 'nreject'}
    assert eps.shape == (n,) and d.shape == (n, 2) and eps.dtype == d.dtype == torch.float64
    print(f'nsteps = {n} nreject = {info["nreject"]} eps = {eps[0]:.4f} .. {float(eps.max()):.4f} sum = {float(eps.sum())!r}')
    assert abs(float(eps.sum()) - t) <= 1e-12
    assert bool((d <= tol).all())
    eps_list = [float(e) for e in eps]
    want, want_d = replay(x4, eps_list)
    amp = growth(x4, eps_list, torch.Generator().manual_seed(6))
    bound = 3.0 * n * 1e-13 * max(1.0, amp)
    e_x, e_d = err(host(ops.su3_unpack(yn, L4)), want), err(d, want_d)
    print(f'A = {amp:.3g}: |dU| = {e_x:.2e} (bound {bound:.2e}) |dd| = {e_d:.2e}')
    assert e_x <= bound
    assert e_d <= 1e-13 * max(1.0, amp)
    # every step size is the controller's formula on the step before it, except where a step was shortened to land
    # on t (the last one) -- which holds step to step because no step was rejected
    assert info['nreject'] == 0
    ctl = ops.FlowStepController(tol)
    assert eps_list[0] == 0.01
    for k in range(n - 1):
        nxt = ctl.next_eps(eps_list[k], float(d[k].max()))
        want_e = eps_list[k] * min(2.0, 0.95 * (tol / float(d[k].max())) ** (1.0 / 3.0))
        assert abs(nxt - want_e) <= 1e-15 * want_e
        if k + 1 < n - 1:
            assert abs(eps_list[k + 1] - want_e) <= 1e-15 * want_e, k
        else:
            assert eps_list[k + 1] <= want_e * (1 + 1e-15)          # shortened
    assert float(ops.su3_check_su_n(yn).max()) <= 1e-12
    assert torch.equal(xn, keep)
    # the reference-layout form is the same run
    y, info2 = lat.flow_adaptive(dev(x4), t, tol=tol)
    assert torch.equal(y, ops.su3_unpack(yn, L4)) and torch.equal(info2['eps'], eps) and torch.equal(info2['d'], d)
    y0, info0 = lat.flow_adaptive(dev(x4), 0.0)
    assert torch.equal(y0, dev(x4)) and info0['nsteps'] == 0 and info0['d'].shape == (0, 2)


# ------------------------------------------------------------------ 3. accuracy ordering
def test_default_tolerance_is_no_worse_than_the_fixed_step(ops, x4):
    """relative error of E at t = 1 against the existing fixed-step flow at eps = 0.0025 (not code under test): the
    adaptive flow at its default tol = 1e-6 is no worse than the fixed step eps = 0.02.  Measured with the restatement
    on the CPU: 3.2e-7 against 7.2e-6."""
    lat = lattice(2, L4)
    xn = ops.su3_pack(dev(x4))
    ref = lat.clover_n(lat.flow_n(xn, 400, 0.0025)).E
    fixed = lat.clover(lat.flow(dev(x4), 1.0, eps=0.02)).E
    y, info = lat.flow_adaptive(dev(x4), 1.0, tol=1e-6)
    adaptive = lat.clover(y).E
    e_fixed = float(((fixed - ref).abs() / ref).max())
    e_adapt = float(((adaptive - ref).abs() / ref).max())
    print(f'relative error of E(t = 1): fixed eps = 0.02 (50 steps) {e_fixed:.2e}, adaptive tol = 1e-6 '
          f'({info["nsteps"]} steps, {info["nreject"]} rejected) {e_adapt:.2e}')
    assert e_adapt <= e_fixed


# ------------------------------------------------------------------ 4. scales
def test_flow_scales(ops, x4):
    from l2hmc.lattice.su3.pytorch.lattice import scales_from_flow
    lat = lattice(2, L4)
    x = dev(x4)
    tmax, dt = 0.6, 0.05
    s = lat.flow_scales(x, tmax=tmax, dt=dt)
    assert set(s) == {'t0', 'w0', 't_reached', 'table'}
    t0, w0 = host(s['t0']), host(s['w0'])
    print(f't0 = {t0.tolist()} w0 = {w0.tolist()} w0^2 = {(w0 ** 2).tolist()} t_reached = {s["t_reached"]}')
    assert not bool(torch.isnan(t0).any() | torch.isnan(w0).any())
    # checked with the restatement for both chains: t^2 E crosses 0.3 in (0.30, 0.35), W in (0.20, 0.25)
    assert bool(((t0 > 0.30) & (t0 < 0.35)).all()) and bool(((w0 ** 2 > 0.20) & (w0 ** 2 < 0.25)).all())
    assert s['t_reached'] < tmax
    # the early stop does not change the answer: the whole table on the same grid gives the same bits
    grid = [k * dt for k in range(1, 13)]
    full = lat.flow_observables_adaptive(x, grid)
    assert set(full) == {'t', 'E', 'Eplaq', 'Q', 't2E', 'eps', 'd', 'nsteps', 'nreject'}
    assert full['t'].shape == (13,) and all(full[k].shape == (13, 2) for k in ('E', 'Eplaq', 'Q', 't2E'))
    assert float(full['t'][0]) == 0.0 and torch.equal(full['t'][1:], dev(torch.tensor(grid, dtype=torch.float64)))
    assert abs(float(full['eps'].sum()) - tmax) <= 1e-12
    sf = scales_from_flow(full['t'], full['E'])
    assert torch.equal(sf['t0'], s['t0']) and torch.equal(sf['w0'], s['w0'])
    rows = s['table']['t'].shape[0]
    assert rows < 13 and float(s['table']['t'][-1]) == s['t_reached']
    for k in ('t', 'E', 'Eplaq', 'Q', 't2E'):
        assert torch.equal(s['table'][k], full[k][:rows]), k
    # row 0 is the unflowed field, every row the observables of the field flowed there
    c0 = lat.clover(x)
    assert torch.equal(full['E'][0], c0.E) and torch.equal(full['Q'][0], c0.Q)
    assert torch.equal(full['t2E'], full['t'][:, None] ** 2 * full['E'])
    y1, i1 = lat.flow_adaptive(x, grid[0])
    c1 = lat.clover(y1)
    assert torch.equal(full['E'][1], c1.E) and torch.equal(full['Eplaq'][1], c1.Eplaq)
    assert torch.equal(full['eps'][:i1['nsteps']], i1['eps'])
    # the plaquette energy crosses near t = 0.10
    sp = lat.flow_scales(x, tmax=tmax, dt=dt, kind='plaq')
    tp, wp = host(sp['t0']), host(sp['w0'])
    print(f'plaq: t0 = {tp.tolist()} w0 = {wp.tolist()} t_reached = {sp["t_reached"]}')
    assert not bool(torch.isnan(tp).any() | torch.isnan(wp).any())
    assert bool(((tp > 0.05) & (tp < 0.15)).all()) and sp['t_reached'] < s['t_reached']
    sfp = scales_from_flow(full['t'], full['Eplaq'])
    assert torch.equal(sfp['t0'], sp['t0']) and torch.equal(sfp['w0'], sp['w0'])
    # a target that is never reached: NaN at tmax, no exception
    sn = lat.flow_scales(x, tmax=0.2, dt=dt, target=5.0)
    assert bool(torch.isnan(sn['t0']).all()) and bool(torch.isnan(sn['w0']).all()) and abs(sn['t_reached'] - 0.2) < 1e-12
    with pytest.raises(ValueError):
        lat.flow_scales(x, tmax=0.6, dt=0.07)
    with pytest.raises(ValueError):
        lat.flow_scales(x, tmax=0.6, kind='wilson')
    with pytest.raises(ValueError):
        lat.flow_observables_adaptive(x, [0.1, 0.1])


# ------------------------------------------------------------------ 5. the Python surface
def test_surface(ops, x4):
    lat = lattice(2, L4)
    x = dev(x4)
    x0 = dev(fr.rand_su3((2, 4, *L4), 2.0, torch.Generator().manual_seed(8)))
    beta = torch.tensor(5.7)
    # calc_metrics is what it was, the fixed-step flow (its parameter list is pinned by tests/test_flow_host.py, so
    # the adaptive flow has no keyword there); the adaptive counterpart of its flowed entries is two lines
    fixed = lat.calc_metrics(x, beta, xinit=x0, flow_time=0.1)
    cf, cf0 = lat.clover(lat.flow(x, 0.1, eps=0.01)), lat.clover(lat.flow(x0, 0.1, eps=0.01))
    assert torch.equal(fixed['Qflow'], cf.Q) and torch.equal(fixed['t2E'], 0.1 ** 2 * cf.E)
    assert torch.equal(fixed['dQflow'], (cf.Q - cf0.Q).abs())
    assert list(lat.calc_metrics(x, beta)) == ['plaqs', 'sinQ', 'intQ', 'action', 'dsdx']
    y, info = lat.flow_adaptive(x, 0.1)
    assert y.shape == x.shape and info['nsteps'] >= 4 and bool(torch.isfinite(lat.clover(y).Q).all())
    # no gradient through the adaptive flow
    xg = x.clone().requires_grad_(True)
    for call in (lambda: lat.flow_adaptive(xg, 0.1), lambda: lat.flow_observables_adaptive(xg, [0.1]),
                 lambda: lat.flow_scales(xg, 0.6)):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError):
        lat.flow_adaptive(x, -0.1)


# ------------------------------------------------------------------ 6. one size users run
def test_adaptive_steps_at_the_size_users_run(ops):
    """8^4 x 256 chains, two accepted steps from eps0 = 0.01 driven by the controller; chains 0, 37, 255 against the
    restatement on the step sizes taken"""
    L, nb, sel, tol = (8, 8, 8, 8), 256, [0, 37, 255], 1e-5
    gen = torch.Generator().manual_seed(33)
    x = fr.rand_su3((nb, 4, *L), 3.0, gen)
    xn = ops.su3_pack(dev(x))
    keep = xn.clone()
    bufs = [torch.empty_like(xn) for _ in range(2)]
    ws_x = torch.empty_like(xn)
    ws_p3 = torch.empty((3, *xn.shape), dtype=xn.dtype, device=xn.device)
    ctl = ops.FlowStepController(tol, eps0=0.01)
    cur, eps_list, ds = xn, [], []
    while len(eps_list) < 2:
        e = ctl.propose()
        out = bufs[len(eps_list) & 1]
        d = host(ops.su3_flow_step_err_n(cur, out, ws_p3, ws_x, e, L))
        if ctl.update(e, float(d.max()), sum(eps_list)):
            eps_list.append(e)
            ds.append(d)
            cur = out
    xs = x[sel].contiguous()
    want, want_d = replay(xs, eps_list)
    amp = growth(xs, eps_list, gen)
    bound = 3.0 * 2 * 1e-13 * max(1.0, amp)
    got = host(ops.su3_unpack(cur[sel].contiguous(), L))
    e_d = err(torch.stack(ds)[:, sel], want_d)
    print(f'eps = {eps_list} rejected = {ctl.nreject} max d = {[float(d.max()) for d in ds]} A = {amp:.3g}: '
          f'|dU| = {err(got, want):.2e} (bound {bound:.2e}) |dd| = {e_d:.2e}')
    assert eps_list[0] <= 0.01 and all(float(d.max()) <= tol for d in ds)
    assert err(got, want) <= bound
    assert e_d <= 1e-13 * max(1.0, amp)
    assert float(ops.su3_check_su_n(cur).max()) <= 1e-12
    assert torch.equal(xn, keep)
