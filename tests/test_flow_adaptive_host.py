"""CPU tier of the adaptive-step Wilson flow: the step-size controller on a synthetic error d = C eps^3, the scale
finder `scales_from_flow` on closed forms, and the order of the restated error estimate
(tests/flow_adaptive_restatement.py) itself."""
import math

import pytest
import torch

import flow_adaptive_restatement as far
import flow_restatement as fr


def controller(*a, **kw):
    from l2hmc._ops import FlowStepController
    return FlowStepController(*a, **kw)


def drive(ctl, C, targets):
    """the loop of the adaptive flow on d = C e^3: [(t before, e, d, accepted, shortened, proposal before)]"""
    log, t = [], 0.0
    for target in targets:
        while t < target:
            before = ctl.eps
            e = ctl.propose(target - t)
            d = C * e ** 3
            ok = ctl.update(e, d, t)
            log.append((t, e, d, ok, e < before, before))
            if ok:
                t = target if ctl.landed else t + e
    return log, t


@pytest.mark.parametrize('eps0', [1e-4, 0.01, 0.3])
def test_controller_converges_on_a_cubic_error(eps0):
    tol, C = 1e-6, 3.0
    star = (0.95 ** 3 * tol / C) ** (1.0 / 3.0)
    ctl = controller(tol, eps0)
    log, t = drive(ctl, C, [1.0])
    assert t == 1.0 and abs(sum(e for _, e, _, ok, _, _ in log if ok) - 1.0) <= 1e-12
    for _, e, d, ok, _, _ in log:
        assert ok == (d <= tol)                                   # never accepts d > tol, never refuses d <= tol
    # every proposal follows the formula; a rejection shrinks the step; growth is at most `grow`
    for (_, e, d, ok, short, _), (_, e1, _, _, short1, before1) in zip(log, log[1:]):
        want = e * min(2.0, 0.95 * (tol / d) ** (1.0 / 3.0))
        assert abs(before1 - want) <= 1e-15 * want
        assert before1 <= 2.0 * e * (1 + 1e-15)
        if not ok:
            assert before1 < e and e1 < e
    # converged: all steps but the first few and the shortened last one are eps*
    tail = [e for _, e, _, ok, short, _ in log[12:] if ok and not short]
    assert len(tail) > 20 and all(abs(e - star) <= 1e-12 * star for e in tail)
    assert ctl.nreject == sum(1 for r in log if not r[3]) and (ctl.nreject > 0) == (eps0 > star)


def test_controller_landing_times_do_not_shrink_the_step():
    tol, C = 1e-6, 3.0
    star = (0.95 ** 3 * tol / C) ** (1.0 / 3.0)                   # 0.006587
    # landing times that leave remainders from nearly a whole step down to a 1e-6 sliver
    targets, t = [], 0.0
    for k, rem in enumerate([0.9, 0.5, 1e-2, 1e-4, 0.3, 1e-6, 0.7]):
        t += (3 + rem) * star
        targets.append(t)
    ctl = controller(tol, star)
    log, tend = drive(ctl, C, targets)
    assert tend == targets[-1] and ctl.nreject == 0
    assert abs(sum(r[1] for r in log) - targets[-1]) <= 1e-12
    nshort = 0
    for (_, e, d, ok, short, before), nxt in zip(log, log[1:] + [(0, 0, 0, True, False, ctl.eps)]):
        assert ok and d <= tol
        if short:
            nshort += 1
            assert nxt[5] >= before                               # the carried step is not smaller than before
            own = e * min(2.0, 0.95 * (tol / d) ** (1.0 / 3.0))
            assert nxt[5] == max(own, before)
        else:
            assert abs(e - star) <= 1e-12 * star
    assert nshort == len(targets)
    # the times are hit exactly
    hits = [r[0] for r in log] + [tend]
    assert all(x in hits for x in targets)
    # a shortened step that is REJECTED does shrink: a proposal of 1 against a landing time at 0.5
    ctl = controller(tol, 1.0)
    e = ctl.propose(0.5)
    assert e == 0.5 and not ctl.update(e, C * e ** 3, 0.0) and not ctl.landed
    assert abs(ctl.eps - star) <= 1e-12 * star


def test_controller_special_values():
    ctl = controller(1e-6, 0.01)
    assert ctl.update(ctl.propose(), 0.0) and ctl.eps == 0.02                       # d = 0: grow
    ctl = controller(1e-6, 0.01, eps_max=0.015)
    assert ctl.update(ctl.propose(), 0.0) and ctl.eps == 0.015                      # capped
    assert ctl.update(ctl.propose(), 1e-30) and ctl.eps == 0.015
    assert controller(1e-6, 0.5, eps_max=0.1).propose() == 0.1
    for bad in (float('nan'), float('inf')):
        ctl = controller(1e-6, 0.01)
        assert not ctl.update(ctl.propose(), bad, 0.25) and ctl.eps == 0.005 and ctl.nreject == 1
        assert not ctl.update(ctl.propose(), bad, 0.25) and ctl.eps == 0.0025
        assert ctl.update(ctl.propose(), 1e-7, 0.25)                                # and recovers
    # max_reject rejections in a row pass, one more raises and names t, e and d
    ctl = controller(1e-6, 0.01, max_reject=3)
    for _ in range(3):
        assert not ctl.update(ctl.propose(), float('nan'), 0.75)
    with pytest.raises(RuntimeError) as ei:
        ctl.update(ctl.propose(), float('nan'), 0.75)
    msg = str(ei.value)
    assert 't = 0.75' in msg and 'e = 0.00125' in msg and 'd = nan' in msg
    # an accepted step in between starts the count again
    ctl = controller(1e-6, 0.01, max_reject=1)
    for _ in range(5):
        assert not ctl.update(ctl.propose(), 1.0)
        assert ctl.update(ctl.propose(), 1e-9)
    with pytest.raises(ValueError):
        controller(0.0)
    with pytest.raises(ValueError):
        controller(1e-6, eps0=0.0)


# ---------------------------------------------------------------------------- scales_from_flow
def scales(*a, **kw):
    from l2hmc.lattice.su3.pytorch.lattice import scales_from_flow
    return scales_from_flow(*a, **kw)


DT = 0.05
GRID = torch.arange(0, 21, dtype=torch.float64) * DT              # 0 .. 1


def energy(F):
    """E = F / t^2 on GRID (row 0, where F = 0, set to 0)"""
    E = F / torch.where(GRID > 0, GRID, torch.ones_like(GRID))[:, None] ** 2
    E[0] = 0.0
    return E


def test_scales_of_a_linear_t2E():
    a = torch.tensor([0.5, 0.9, 1.7], dtype=torch.float64)
    s = scales(GRID, energy(a * GRID[:, None]), 0.3)
    # F = a t and W = a t are linear: the interpolation bound (dt^2 / 8) |g''| / |g'| is zero, rounding remains
    assert (s['t0'] - 0.3 / a).abs().max() <= 1e-14
    assert (s['w0'] ** 2 - 0.3 / a).abs().max() <= 1e-14
    s = scales(GRID, energy(a * GRID[:, None]), target=0.2)
    assert (s['t0'] - 0.2 / a).abs().max() <= 1e-14 and (s['w0'] ** 2 - 0.2 / a).abs().max() <= 1e-14


def test_scales_of_a_quadratic_t2E():
    a = torch.tensor([1.7, 1.1, 0.4], dtype=torch.float64)
    s = scales(GRID, energy(a * GRID[:, None] ** 2), 0.3)
    t0 = torch.sqrt(0.3 / a)
    tstar = torch.sqrt(0.3 / (2 * a))
    # F = a t^2: (dt^2 / 8) 2a / (2a t0);  W = 2a t^2 (the central difference is exact): (dt^2 / 8) 4a / (4a t*)
    b0 = (DT ** 2 / 8) * (2 * a) / (2 * a * t0)
    bw = (DT ** 2 / 8) * (4 * a) / (4 * a * tstar)
    e0, ew = (s['t0'] - t0).abs(), (s['w0'] ** 2 - tstar).abs()
    print(f't0 error {e0.tolist()} bound {b0.tolist()}; t* error {ew.tolist()} bound {bw.tolist()}')
    assert (e0 <= b0).all() and (ew <= bw).all()
    assert (e0 > 0).all()                                         # (the bound is not met by an exact formula)


def test_scales_nan_first_crossing_and_cut_tables():
    a = torch.tensor([0.2, 1.7], dtype=torch.float64)             # chain 0 never reaches 0.3 on t <= 1
    s = scales(GRID, energy(a * GRID[:, None]), 0.3)
    assert math.isnan(float(s['t0'][0])) and math.isnan(float(s['w0'][0]))
    assert abs(float(s['t0'][1]) - 0.3 / 1.7) <= 1e-14
    # t0 bracketed but w0 not: F = a t^2 crosses 0.3 at t = 0.87, W = 2 a t^2 already at 0.61; cut the table at 0.5
    E = energy(torch.tensor([0.4], dtype=torch.float64) * GRID[:, None] ** 2)
    s = scales(GRID[:11], E[:11], 0.3)
    assert math.isnan(float(s['t0'][0])) and math.isnan(float(s['w0'][0]))
    s = scales(GRID[:15], E[:15], 0.3)
    assert math.isnan(float(s['t0'][0])) and not math.isnan(float(s['w0'][0]))
    # a non-monotone F: up through 0.3 between rows 3 and 4, down again, up again between rows 9 and 10; and one
    # that starts above the target, whose first UPWARD crossing is the second passage
    F = torch.tensor([[0.0, 0.1, 0.2, 0.28, 0.36, 0.4, 0.33, 0.25, 0.2, 0.29, 0.5, 0.6, 0.7],
                      [0.5, 0.45, 0.4, 0.35, 0.31, 0.29, 0.25, 0.2, 0.25, 0.29, 0.33, 0.4, 0.5]],
                     dtype=torch.float64).T.contiguous()
    g = GRID[1:14]                                                # a grid need not start at 0
    s = scales(g, F / g[:, None] ** 2, 0.3)
    assert abs(float(s['t0'][0]) - (float(g[3]) + DT * 0.02 / 0.08)) <= 1e-13
    assert abs(float(s['t0'][1]) - (float(g[9]) + DT * 0.01 / 0.04)) <= 1e-13
    # a crossing needs only the rows up to the one after it: the table cut behind both gives the same bits
    a = torch.tensor([1.7, 1.1], dtype=torch.float64)
    E = energy(a * GRID[:, None] ** 2)
    full = scales(GRID, E, 0.3)
    k = int(math.floor(float(full['t0'].max()) / DT)) + 2            # rows 0 .. the one after the last crossing
    cut = scales(GRID[:k], E[:k], 0.3)
    assert torch.equal(cut['t0'], full['t0']) and torch.equal(cut['w0'], full['w0'])
    assert torch.isnan(scales(GRID[:k - 1], E[:k - 1], 0.3)['t0']).any()
    # NaN in the data gives NaN, not an exception
    E[5, 0] = float('nan')
    assert scales(GRID, E, 0.3)['t0'].shape == (2,)


def test_scales_refuse_a_bad_grid():
    E = torch.ones((21, 2), dtype=torch.float64)
    with pytest.raises(ValueError):
        scales(GRID[:3], E[:3])
    bent = GRID.clone()
    bent[7] += 1e-3
    with pytest.raises(ValueError):
        scales(bent, E)
    with pytest.raises(ValueError):
        scales(GRID.flip(0), E)
    with pytest.raises(ValueError):
        scales(GRID, E[:20])


# ---------------------------------------------------------------------------- the restatement's own order
@pytest.mark.parametrize('scale', [0.6, 2.0])
def test_restated_estimate_is_third_order(scale):
    x = fr.rand_su3((2, 4, 2, 2, 2, 2), scale, torch.Generator().manual_seed(5))
    d = {eps: far.flow_step_err(x, eps)[1] for eps in (0.04, 0.02, 0.01)}
    for eps in (0.04, 0.02):
        r = d[eps] / d[eps / 2]
        print(f'scale {scale}: d({eps}) / d({eps / 2}) = {r.tolist()}')
        assert ((r >= 7.0) & (r <= 9.0)).all()
    # the step of the pair is the restated flow step itself
    assert torch.equal(far.flow_step_err(x, 0.02)[0], fr.flow_step(x, 0.02))
