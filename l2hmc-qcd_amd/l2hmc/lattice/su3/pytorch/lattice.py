"""``LatticeSU3`` -- API of src/l2hmc/lattice/su3/pytorch/lattice.py:39-349 on HIP kernels.

The reference builds ~18 lattice-sized temporaries per action call (roll / bmm / stack) and
gets the force by autograd; here ``action``, ``plaqs`` and the charges come from ONE pass of
``l2q_su3_plaq_reduce`` (576 B per chain-site) and the force from ``l2q_su3_force``
(explicit staples + TAH, 1152 B per chain-site).  c1 != 0 (Iwasaki / DBW2, lattice.py:83-112,
180-196) adds ``l2q_su3_rect_reduce`` / ``l2q_su3_rect_force_add`` for the 2x1 rectangles.
"""
from __future__ import annotations

import logging
from typing import NamedTuple, Optional

import numpy as np
import torch

import l2hmc.group.su3.pytorch.group as g
from l2hmc import DEVICE
from l2hmc import _autograd as AG
from l2hmc import _ops as ops
from l2hmc.configs import Charges
from l2hmc.lattice.lattice import Lattice
from l2hmc.lattice.su3.pytorch.wilson import (CloverTerm, WilsonFermions, _log_positive, effective_mass,  # noqa: F401
                                              pion_correlator)

log = logging.getLogger(__name__)
Tensor = torch.Tensor
PI = np.pi
TWO_PI = 2. * np.pi


def _beta(beta) -> float:
    return float(beta.item()) if isinstance(beta, torch.Tensor) else float(beta)


def pbc(tup: tuple[int], shape: tuple[int]) -> list:
    return np.mod(tup, shape).tolist()


def mat_adj(mat: np.ndarray) -> np.ndarray:
    return mat.conj().T


class PlaqSums:
    """Per-chain (sum Re tr P, sum Im tr P): what the sampler's own consumers (action, plaquette,
    charges) reduce the reference's ``wloops`` field to.  ``LatticeSU3.plaq_sums`` returns it from ONE
    pass of `l2q_su3_plaq_reduce`; ``wilson_loops`` returns the field itself as the reference does, and
    every ``_plaqs / _charges / ...`` helper below accepts either."""

    def __init__(self, sums: Tensor):
        self.re = sums[:, 0].contiguous()
        self.im = sums[:, 1].contiguous()


class Clover(NamedTuple):
    """Per-chain clover observables, [nb] float64 each: energy density ``E = -(1/V) sum_x sum_{mu<nu} tr F F``,
    topological charge ``Q = -(1/4 pi^2) sum_x tr(F01 F23 - F02 F13 + F03 F12)`` and the plaquette energy
    density ``Eplaq = 36 (1 - plaqs)``, from ONE pass of `l2q_su3_clover_reduce`."""
    E: Tensor
    Q: Tensor
    Eplaq: Tensor


class GaugeCondition(NamedTuple):
    """Per-chain gauge functional ``F = (1 / (3 |D| V)) sum_x sum_{mu in D} Re tr U_mu(x)`` and residual ``theta =
    (1 / (3 V)) sum_x tr Delta Delta^H`` of the gauge directions D, [nb] float64 each (`l2q_su3_gauge_condition`)."""
    F: Tensor
    theta: Tensor


# the overrelaxation parameter of `LatticeSU3.gauge_fix` when none is given: of {1.0, 1.3, 1.5, 1.7, 1.9} the one
# with the fewest sweeps to theta <= 1e-12 on thermalised 8^4 chains at beta = 6, in Landau and in Coulomb gauge
# (profiles/su3_gaugefix.md)
GAUGEFIX_OMEGA = 1.7


def _site_sum(w: Tensor) -> Tensor:
    """the reference's reduction of a trace field [nplanes, nb, T, X, Y, Z] to [nb] (lattice.py:209, 228)"""
    return w.sum(tuple(range(2, len(w.shape)))).sum(0)


def creutz_ratios(w: Tensor) -> Tensor:
    """chi(R, T) = -ln[W(R, T) W(R-1, T-1) / (W(R, T-1) W(R-1, T))] for R, T >= 2 from a table w[..., rmax, tmax] with
    w[..., R-1, T-1] = W(R, T): [..., rmax-1, tmax-1], entry [R-2, T-2].  An area law W = exp(-sigma R T - m (R + T) - c)
    gives sigma everywhere.  NaN where the argument of the logarithm is not positive; never raises."""
    w = torch.as_tensor(w)
    return -_log_positive(w[..., 1:, 1:] * w[..., :-1, :-1] / (w[..., 1:, :-1] * w[..., :-1, 1:]))


def static_potential(w: Tensor) -> Tensor:
    """V(R; T) = ln[W(R, T) / W(R, T+1)] from a table w[..., rmax, tmax]: [..., rmax, tmax-1], entry [R-1, T-1]; the
    static potential is its plateau at large T.  NaN where the ratio is not positive; never raises."""
    w = torch.as_tensor(w)
    return _log_positive(w[..., :, :-1] / w[..., :, 1:])


def _first_upward_crossing(t: Tensor, g: Tensor, target: float) -> Tensor:
    """[nb]: where g[k, nb] on the points t[k] first goes from below `target` to at or above it, linearly interpolated
    between the two points; NaN for a chain with no such pair"""
    nan = torch.full(g.shape[1:], float('nan'), dtype=g.dtype, device=g.device)
    if g.shape[0] < 2:
        return nan
    up = (g[:-1] < target) & (g[1:] >= target)
    k = up.to(torch.int8).argmax(0)[None]
    g0, g1 = g[:-1].gather(0, k)[0], g[1:].gather(0, k)[0]
    t0, t1 = t[:-1][k[0]], t[1:][k[0]]
    ok = up.any(0)
    den = torch.where(ok, g1 - g0, torch.ones_like(g0))
    return torch.where(ok, t0 + (t1 - t0) * ((target - g0) / den), nan)


def scales_from_flow(t: Tensor, E: Tensor, target: float = 0.3) -> dict[str, Tensor]:
    """The reference scales t0 and w0 (Luescher, arXiv:1006.4518; Borsanyi et al., arXiv:1203.4469) from the energy
    density E[k, nb] on a uniform grid t[k] of flow times, {'t0': [nb], 'w0': [nb]}, in lattice units.  With
    F = t^2 E: t0 is the first upward crossing of F through `target`, linearly interpolated between grid points;
    w0 = sqrt(t*) with t* the first upward crossing of W_k = t_k (F_{k+1} - F_{k-1}) / (2 dt) = t dF/dt at the
    interior points.  NaN where no crossing is bracketed; never raises on data.  A crossing depends only on the rows
    up to the one after it, so a table cut off behind both crossings gives the same bits as the whole one.  ValueError
    on a grid of fewer than four points or one that is not uniform."""
    t = torch.as_tensor(t, dtype=torch.float64)
    E = torch.as_tensor(E, dtype=torch.float64).to(t.device)
    if t.dim() != 1 or E.dim() != 2 or E.shape[0] != t.shape[0]:
        raise ValueError(f'scales_from_flow: need t [n] and E [n, nb], got {list(t.shape)} and {list(E.shape)}')
    if t.shape[0] < 4:
        raise ValueError(f'scales_from_flow: need at least four grid points, got {t.shape[0]}')
    dt = t[1] - t[0]
    if not bool(dt > 0) or not bool(((t[1:] - t[:-1] - dt).abs() <= 1e-9 * dt).all()):
        raise ValueError('scales_from_flow: the grid of flow times must be uniform and increasing')
    F = t[:, None] ** 2 * E
    W = t[1:-1, None] * ((F[2:] - F[:-2]) / (2.0 * dt))
    target = float(target)
    tstar = _first_upward_crossing(t[1:-1], W, target)
    return {'t0': _first_upward_crossing(t, F, target), 'w0': torch.sqrt(tstar)}


class LatticeSU3(Lattice, WilsonFermions):
    """4D lattice with SU(3) links: x.shape = [nb, 4, nt, nx, ny, nz, 3, 3] complex128."""
    dim = 4

    def __init__(self, nchains: int, shape: list[int], c1: float = 0.0) -> None:
        assert len(shape) == 4
        self.g = g.SU3()
        self.nt, self.nx, self.ny, self.nz = shape
        self.c1 = c1
        super().__init__(group=self.g, nchains=nchains, shape=list(shape))
        self.volume = self.nt * self.nx * self.ny * self.nz

    # ------------------------------------------------------------ native-layout core
    def pack(self, x: Tensor) -> Tensor:
        # (a tensor a transition returned still carries its native-layout original)
        return AG.su3_pack_cached(x.to(DEVICE))

    def unpack(self, xn: Tensor) -> Tensor:
        return ops.su3_unpack(xn, self._lattice_shape)

    def plaq_sums_n(self, xn: Tensor) -> Tensor:
        return ops.su3_plaq_sums_n(xn, self._lattice_shape)

    def rect_sums_n(self, xn: Tensor) -> Tensor:
        """[nb]: sum Re tr R over the 12 planar 2x1 loops per site (c1 != 0 actions)."""
        return ops.su3_rect_sums_n(xn, self._lattice_shape)

    def action_n(self, xn: Tensor, beta) -> Tensor:
        """-(1/3) [beta (1 - 8 c1) sum Re tr P + beta c1 sum Re tr R] (lattice.py:252-269)"""
        b = _beta(beta)
        if self.c1 == 0.0:
            return (-b / 3.0) * self.plaq_sums_n(xn)[:, 0]
        return (-b * (1.0 - 8.0 * self.c1) / 3.0) * self.plaq_sums_n(xn)[:, 0] \
            + (-b * self.c1 / 3.0) * self.rect_sums_n(xn)

    def grad_action_n(self, xn: Tensor, beta) -> Tensor:
        """(1/3) TAH(U (c_plaq A_plaq + c_rect A_rect)): staples of the plaquettes and, for
        c1 != 0, of the 18 rectangles through each link."""
        b = _beta(beta)
        if self.c1 == 0.0:
            return ops.su3_force_n(xn, b, self._lattice_shape)
        f = ops.su3_force_n(xn, b * (1.0 - 8.0 * self.c1), self._lattice_shape)
        return ops.su3_rect_force_add_n(xn, b * self.c1 / 3.0, f, self._lattice_shape)

    # ------------------------------------------------------------ Wilson flow and clover observables
    def _clover_of_sums(self, s: Tensor) -> Clover:
        return Clover(E=s[:, 0] / self.volume, Q=s[:, 1] / (4 * np.pi ** 2),
                      Eplaq=36.0 - (2.0 / self.volume) * s[:, 2])

    def clover_n(self, xn: Tensor) -> Clover:
        return self._clover_of_sums(ops.su3_clover_sums_n(xn, self._lattice_shape))

    def clover(self, x: Tensor) -> Clover:
        """Clover energy density, topological charge and plaquette energy density of x (reference layout)."""
        self._no_grad(x, 'clover')
        return self.clover_n(self.pack(x))

    def clover_autograd(self, x: Tensor, *, flow_time: float = 0.0, eps: float = 0.01) -> Clover:
        """`clover(x)`, differentiable where x requires a gradient (`l2q_su3_clover_bwd` behind it, the links as
        unconstrained complex matrices); the same kernel and the same numbers as `clover(x)` otherwise.  With
        `flow_time` > 0 the observables of x flowed to that time in steps of eps (`flow_autograd`)."""
        if float(flow_time) != 0.0:
            x = self.flow_autograd(x, flow_time, eps)
        if AG.wants_grad(x):
            return self._clover_of_sums(AG.SU3CloverSums.apply(x.to(DEVICE), self._lattice_shape))
        return self.clover_n(self.pack(x))

    def topological_charge(self, x: Tensor) -> Tensor:
        return self.clover(x).Q

    def energy_density(self, x: Tensor, kind: str = 'clover') -> Tensor:
        if kind not in ('clover', 'plaq'):
            raise ValueError(f"energy_density: kind must be 'clover' or 'plaq', got {kind!r}")
        c = self.clover(x)
        return c.E if kind == 'clover' else c.Eplaq

    @staticmethod
    def _no_grad(x: Tensor, what: str) -> None:
        if isinstance(x, torch.Tensor) and x.requires_grad:
            raise RuntimeError(f'LatticeSU3.{what}: no autograd through the Wilson flow / clover observables')

    @staticmethod
    def _flow_steps(t: float, eps: float) -> int:
        if not eps > 0 or t < 0:
            raise ValueError(f'flow: need eps > 0 and t >= 0, got t = {t}, eps = {eps}')
        n = round(t / eps)
        if abs(t / eps - n) > 1e-9:
            raise ValueError(f'flow: t / eps must be an integer, got t = {t}, eps = {eps}')
        return int(n)

    def _flow_iter(self, xn: Tensor, nsteps: int, eps: float):
        """yields the native field after 1, 2, ..., nsteps steps (a buffer that the step after next overwrites);
        three ping-pong fields and the generator field are allocated once, xn is never written"""
        bufs = [torch.empty_like(xn) for _ in range(2)]
        ws_x, ws_p = torch.empty_like(xn), torch.empty_like(xn)
        cur = xn
        for k in range(nsteps):
            out = bufs[k & 1]
            ops.su3_flow_step_n(cur, out, ws_p, ws_x, eps, self._lattice_shape)
            cur = out
            yield cur

    def flow_n(self, xn: Tensor, nsteps: int, eps: float = 0.01) -> Tensor:
        """`nsteps` third-order steps of size eps of the Wilson flow dV/dt = -TAH(V A) V (always the plaquette
        action, whatever c1) on a native field; returns a new field (xn itself for nsteps = 0)."""
        cur = xn
        for cur in self._flow_iter(xn, int(nsteps), float(eps)):
            pass
        return cur

    def flow(self, x: Tensor, t: float, eps: float = 0.01) -> Tensor:
        """x flowed to time t in round(t / eps) steps; reference layout in and out."""
        self._no_grad(x, 'flow')
        n = self._flow_steps(float(t), float(eps))
        return self.unpack(self.flow_n(self.pack(x), n, eps))

    def flow_autograd(self, x: Tensor, t: float, eps: float = 0.01) -> Tensor:
        """`flow(x, t, eps)`, differentiable where x requires a gradient (`AG.SU3Flow`: the reverse sweep of
        `l2q_su3_flow_step_bwd` behind it, the links as unconstrained complex matrices; round(t / eps) + 9 fields of
        memory); the same kernels and the same numbers as `flow` otherwise.  No step (t = 0) returns x itself."""
        n = self._flow_steps(float(t), float(eps))
        if n == 0:
            return x
        if AG.wants_grad(x):
            return AG.SU3Flow.apply(x.to(DEVICE), self._lattice_shape, n, float(eps))
        xn = self.flow_n(self.pack(x), n, eps)
        return AG.attach_native(self.unpack(xn), xn)

    def flow_observables(self, x: Tensor, t: float, eps: float = 0.01, every: int = 1) -> dict[str, Tensor]:
        """Clover observables along the flow: 't' [n+1], 'E', 'Eplaq', 'Q', 't2E' [n+1, nb], measured every
        `every` steps (row 0 = unflowed).  Packs once and stays in the native layout between steps."""
        self._no_grad(x, 'flow_observables')
        nsteps = self._flow_steps(float(t), float(eps))
        every = int(every)
        if every < 1 or nsteps % every != 0:
            raise ValueError(f'flow_observables: every = {every} must divide the {nsteps} steps')
        xn = self.pack(x)
        ts, rows = [0.0], [self.clover_n(xn)]
        for k, cur in enumerate(self._flow_iter(xn, nsteps, float(eps)), start=1):
            if k % every == 0:
                ts.append(k * float(eps))
                rows.append(self.clover_n(cur))
        tt = torch.tensor(ts, dtype=torch.float64, device=xn.device)
        out = {'t': tt}
        for name in Clover._fields:
            out[name] = torch.stack([getattr(r, name) for r in rows])
        out['t2E'] = tt[:, None] ** 2 * out['E']
        return out

    # ------------------------------------------------------------ adaptive-step flow, t0 and w0
    def _flow_adaptive_iter(self, xn: Tensor, ts, ctl: ops.FlowStepController, info: dict):
        """yields the native field at each of the increasing times ts (a buffer that the step after next overwrites):
        steps of `l2q_su3_flow_step_err` sized by ctl, the step before a time in ts shortened to land on it.  Six fields
        beside xn, allocated once (two ping-pong, W2, P1..P3); xn is never written, a rejected step is retried from
        its input.  One read of d [nb] from the device per step.  info collects the accepted steps."""
        bufs = [torch.empty_like(xn) for _ in range(2)]
        ws_x = torch.empty_like(xn)
        ws_p3 = torch.empty((3, *xn.shape), dtype=xn.dtype, device=xn.device)
        cur, t, k = xn, 0.0, 0
        for target in ts:
            while t < target:
                e = ctl.propose(target - t)
                out = bufs[k & 1]
                d = ops.su3_flow_step_err_n(cur, out, ws_p3, ws_x, e, self._lattice_shape).cpu()
                if ctl.update(e, float(d.max()), t):
                    info['eps'].append(e)
                    info['d'].append(d)
                    t = target if ctl.landed else t + e
                    cur = out
                    k += 1
            yield cur

    @staticmethod
    def _flow_times(ts, what: str) -> list[float]:
        ts = [float(t) for t in ts]
        if any(not b > a for a, b in zip([0.0] + ts[:-1], ts)) or not all(np.isfinite(ts)):
            raise ValueError(f'{what}: the flow times must be finite, positive and increasing, got {ts}')
        return ts

    @staticmethod
    def _flow_info(info: dict, ctl: ops.FlowStepController, nb: int) -> dict:
        n = len(info['eps'])
        return {'eps': torch.tensor(info['eps'], dtype=torch.float64),
                'd': torch.stack(info['d']) if n else torch.empty((0, nb), dtype=torch.float64),
                'nsteps': n, 'nreject': ctl.nreject}

    def flow_adaptive_n(self, xn: Tensor, t: float, tol: float = 1e-6, eps0: float = 0.01,
                        eps_max: Optional[float] = None):
        """The Wilson flow of `flow_n` to time t in third-order steps whose size follows the embedded second-order
        error estimate d = max over links of |W3 - W'|_F / 9 (`ops.FlowStepController`: a step is accepted iff
        d <= tol, the next one is e min(2, 0.95 (tol / d)^(1/3))), starting at eps0; lands on t exactly.
        -> (field, info): a new native field (xn itself for t = 0) and info = {'eps' [nsteps], 'd' [nsteps, nb] (host
        tensors, the accepted steps), 'nsteps', 'nreject'}.  ONE step size serves the whole batch, driven by its worst
        chain, so all chains stay at the same t; a chain's result therefore depends on its batch mates at the level
        of tol.  tol bounds the estimate of each step, not the error at t: at tol = 1e-6 the error of E was below that
        of `flow` at eps = 0.01 at t = 1 on a rough 4^4 field and twice it at t = 4 on thermalised 8^4 chains, in
        half the steps (profiles/su3_flow_adaptive.md).  Six fields of memory beside xn."""
        t = float(t)
        if not t >= 0 or not np.isfinite(t):
            raise ValueError(f'flow_adaptive: need a finite t >= 0, got {t}')
        ctl = ops.FlowStepController(tol, eps0, eps_max)
        info = {'eps': [], 'd': []}
        cur = xn
        for cur in self._flow_adaptive_iter(xn, [t] if t > 0 else [], ctl, info):
            pass
        return cur, self._flow_info(info, ctl, xn.shape[0])

    def flow_adaptive(self, x: Tensor, t: float, tol: float = 1e-6, eps0: float = 0.01,
                      eps_max: Optional[float] = None):
        """`flow_adaptive_n` in the reference layout: -> (x flowed to t, info).  Not differentiable: the
        differentiable flow (`flow_autograd`) stays fixed-step."""
        self._no_grad(x, 'flow_adaptive')
        xn, info = self.flow_adaptive_n(self.pack(x), t, tol, eps0, eps_max)
        return self.unpack(xn), info

    def flow_observables_adaptive(self, x: Tensor, ts, tol: float = 1e-6, eps0: float = 0.01,
                                  eps_max: Optional[float] = None) -> dict:
        """`flow_observables` on the adaptive flow: the observables at the increasing times ts, on each of which a step
        lands.  't' [n+1], 'E', 'Eplaq', 'Q', 't2E' [n+1, nb] with row 0 at t = 0, and the info of `flow_adaptive_n`
        ('eps', 'd', 'nsteps', 'nreject').  The step size is shared by the batch (see `flow_adaptive_n`)."""
        self._no_grad(x, 'flow_observables_adaptive')
        out, _ = self._flow_table(self.pack(x), self._flow_times(ts, 'flow_observables_adaptive'), tol, eps0, eps_max)
        return out

    def _flow_table(self, xn: Tensor, ts: list, tol: float, eps0: float, eps_max: Optional[float],
                    kind: Optional[str] = None, target: float = 0.3):
        """the table of `flow_observables_adaptive`; with `kind` the flow ends behind the first time at which
        `scales_from_flow` of the rows so far has t0 and w0 for every chain.  -> (table, those scales or None)"""
        ctl = ops.FlowStepController(tol, eps0, eps_max)
        info = {'eps': [], 'd': []}
        rows, scales = [self.clover_n(xn)], None
        for k, cur in enumerate(self._flow_adaptive_iter(xn, ts, ctl, info), start=1):
            rows.append(self.clover_n(cur))
            if kind is not None and k + 1 >= 4:
                tt = torch.tensor([0.0] + ts[:k], dtype=torch.float64, device=xn.device)
                s = scales_from_flow(tt, torch.stack([getattr(r, kind) for r in rows]), target)
                if not bool((torch.isnan(s['t0']) | torch.isnan(s['w0'])).any()):
                    scales = s
                    break
        tt = torch.tensor([0.0] + ts[:len(rows) - 1], dtype=torch.float64, device=xn.device)
        out = {'t': tt}
        for name in Clover._fields:
            out[name] = torch.stack([getattr(r, name) for r in rows])
        out['t2E'] = tt[:, None] ** 2 * out['E']
        out.update(self._flow_info(info, ctl, xn.shape[0]))
        return out, scales

    def flow_scales(self, x: Tensor, tmax: float, dt: float = 0.05, tol: float = 1e-6, kind: str = 'clover',
                    target: float = 0.3) -> dict:
        """t0 and w0 of every chain (`scales_from_flow`, lattice units): the adaptive flow measured on the grid
        k dt, k = 0 .. round(tmax / dt), stopped as soon as both crossings of every chain are bracketed, else at
        tmax.  kind = 'clover' or 'plaq' chooses the energy density.  -> {'t0', 'w0' [nb] (NaN: not reached before
        tmax), 't_reached', 'table' (that of `flow_observables_adaptive` up to t_reached)}.  The early stop does not
        change the answer: the same bits as `scales_from_flow` of the whole table to tmax on the same grid."""
        self._no_grad(x, 'flow_scales')
        if kind not in ('clover', 'plaq'):
            raise ValueError(f"flow_scales: kind must be 'clover' or 'plaq', got {kind!r}")
        tmax, dt = float(tmax), float(dt)
        n = round(tmax / dt) if dt > 0 else 0
        if n < 3 or abs(tmax / dt - n) > 1e-9:
            raise ValueError(f'flow_scales: tmax / dt must be an integer >= 3, got tmax = {tmax}, dt = {dt}')
        col = 'E' if kind == 'clover' else 'Eplaq'
        table, s = self._flow_table(self.pack(x), [k * dt for k in range(1, n + 1)], tol, 0.01, None, col, target)
        if s is None:
            s = scales_from_flow(table['t'], table[col], target)
        return {'t0': s['t0'], 'w0': s['w0'], 't_reached': float(table['t'][-1]), 'table': table}

    # ------------------------------------------------------------ Wilson loops R x T and Polyakov loops
    def wilson_loop_sums_n(self, xn: Tensor, rmax: int, tmax: int, xtn: Optional[Tensor] = None) -> Tensor:
        """[nb, rmax, tmax, 12] complex: entry [R-1, T-1, k] = sum over sites of tr W_{mu nu}(R, T), the loop with R links
        along mu and T links along nu, k = 3 mu + (nu if nu < mu else nu - 1).  The lines along mu grow by one link
        per R and the lines along nu by one link per T (`l2q_su3_line_extend`), in at most two fields beyond xn, which
        is never written; one `l2q_su3_loop_reduce` per (R, T).  With `xtn` (another native field, e.g. HYP-smeared)
        the T lines along nu are built from xtn and the R lines along mu from xn; None: both from xn."""
        self._no_grad(xn, 'wilson_loop_sums_n')
        rmax, tmax = int(rmax), int(tmax)
        if rmax < 1 or tmax < 1:
            raise ValueError(f'wilson_loop_sums_n: need rmax, tmax >= 1, got {rmax}, {tmax}')
        if xtn is None:
            xtn = xn
        else:
            self._no_grad(xtn, 'wilson_loop_sums_n')
            if xtn.shape != xn.shape or xtn.dtype != xn.dtype:
                raise ValueError(f'wilson_loop_sums_n: xtn must be shaped like xn {list(xn.shape)}, got '
                                 f'{list(xtn.shape)} {xtn.dtype}')
        L = self._lattice_shape
        out = torch.empty((xn.shape[0], rmax, tmax, 12), dtype=torch.complex128, device=xn.device)
        a, b_buf = xn, None
        for r in range(1, rmax + 1):
            if r > 1:       # a: lines of length r - 1 -> r (the first time into a new field, then in place)
                a = ops.su3_line_extend_n(a, xn, r - 1, L, out=None if a is xn else a)
            b = xtn
            for t in range(1, tmax + 1):
                if t > 1:
                    b_buf = torch.empty_like(xtn) if b_buf is None else b_buf
                    b = ops.su3_line_extend_n(b, xtn, t - 1, L, out=b_buf)
                out[:, r - 1, t - 1] = ops.su3_loop_sums_n(a, r, b, t, L)
        return out

    def _loop_extents(self, time_dir: Optional[int]) -> tuple[int, int]:
        """the smallest extents that the R lines and the T lines of `wilson_loop_table` run along"""
        L = [int(i) for i in self._lattice_shape]
        if time_dir is None:
            return min(L), min(L)
        time_dir = int(time_dir)
        if not 0 <= time_dir < 4:
            raise ValueError(f'wilson_loop_table: time_dir must be 0..3 or None, got {time_dir}')
        return min(n for d, n in enumerate(L) if d != time_dir), L[time_dir]

    def wilson_loop_table(self, x: Tensor, rmax: int, tmax: int, time_dir: Optional[int] = 0) -> Tensor:
        """W(R, T) [nb, rmax, tmax] real: the mean over sites and over the three pairs (mu != time_dir, nu = time_dir)
        of Re tr W_{mu nu}(R, T) / 3; with time_dir None the mean over all 12 ordered pairs.  Loops that would wrap
        around the lattice are refused: ValueError when rmax or tmax is below 1 or exceeds the smallest extent its
        lines run along.  Measured on smeared links by passing `flow(x, t)`, or, keeping the time direction sharp, by
        `wilson_loop_table_xt` / `smeared_loop_table`."""
        return self._loop_table(x, None, rmax, tmax, time_dir)

    def wilson_loop_table_xt(self, x: Tensor, xt: Tensor, rmax: int, tmax: int, time_dir: int = 0) -> Tensor:
        """`wilson_loop_table` with its two kinds of line from two fields: the R lines along mu != time_dir are built
        from x (e.g. `ape_smear(x)`), the T lines along time_dir from xt (e.g. `hyp_smear(x)`); `smeared_loop_table`
        does both.  xt = x gives the bits of `wilson_loop_table(x, ...)`.  Needs a time_dir (ValueError with None: over all 12
        ordered pairs every direction is both an R line and a T line)."""
        self._no_grad(x, 'wilson_loop_table_xt')
        self._no_grad(xt, 'wilson_loop_table_xt')
        if time_dir is None:
            raise ValueError('wilson_loop_table_xt: needs a time_dir: with all 12 ordered pairs every direction is '
                             'both an R line and a T line')
        if not isinstance(xt, torch.Tensor) or xt.shape != x.shape:
            raise ValueError(f'wilson_loop_table_xt: xt must be a tensor shaped like x {list(x.shape)}, got '
                             f'{list(getattr(xt, "shape", []))}')
        return self._loop_table(x, xt, rmax, tmax, time_dir)

    def _loop_table(self, x: Tensor, xt: Optional[Tensor], rmax: int, tmax: int, time_dir: Optional[int]) -> Tensor:
        """the table of `wilson_loop_table` (xt None) / `wilson_loop_table_xt`"""
        self._no_grad(x, 'wilson_loop_table')
        rmax, tmax = int(rmax), int(tmax)
        rlim, tlim = self._loop_extents(time_dir)
        if not (1 <= rmax <= rlim and 1 <= tmax <= tlim):
            raise ValueError(f'wilson_loop_table: need 1 <= rmax <= {rlim} and 1 <= tmax <= {tlim} on lattice '
                             f'{list(self._lattice_shape)} with time_dir = {time_dir}, got rmax = {rmax}, tmax = {tmax}')
        s = self.wilson_loop_sums_n(self.pack(x), rmax, tmax, None if xt is None else self.pack(xt)).real
        if time_dir is not None:
            td = int(time_dir)
            s = s[..., [3 * mu + (td if td < mu else td - 1) for mu in range(4) if mu != td]]
        return s.mean(-1) / (3.0 * self.volume)

    def polyakov_loops(self, x: Tensor, mu: int = 0) -> Tensor:
        """P(x_perp) = tr prod_k U_mu(x_perp, x_mu = k) / 3, [nb, *perp] complex: the lattice with direction mu removed"""
        self._no_grad(x, 'polyakov_loops')
        return ops.su3_polyakov_n(self.pack(x), mu, self._lattice_shape) / 3.0

    def polyakov(self, x: Tensor, mu: int = 0) -> Tensor:
        """[nb] complex: the mean of `polyakov_loops` over the perpendicular sites (the order parameter of the centre
        symmetry)"""
        p = self.polyakov_loops(x, mu)
        return p.reshape(p.shape[0], -1).mean(-1)

    def polyakov_correlator(self, x: Tensor, mu: int = 0) -> Tensor:
        """C(r) = (1 / V_perp) sum_y Re P(y) conj P(y + r), [nb, *perp] real, periodic in r; C(0) = mean |P|^2.  The sum
        over y is a circular correlation, taken by torch.fft on the device."""
        p = self.polyakov_loops(x, mu)
        dims = (1, 2, 3)
        f = torch.fft.fftn(p, dim=dims)
        vp = p[0].numel()
        return torch.fft.ifftn(f.real ** 2 + f.imag ** 2, dim=dims).real / vp

    def polyakov_metrics(self, x: Tensor, xinit: Optional[Tensor] = None) -> dict[str, Tensor]:
        """{'ploop': |polyakov(x, 0)|} and, with xinit, 'dploop' = | |polyakov(x, 0)| - |polyakov(xinit, 0)| | after it:
        the entries to append to `calc_metrics` when the Polyakov loop is monitored."""
        metrics = {'ploop': self.polyakov(x, 0).abs()}
        if xinit is not None:
            metrics['dploop'] = (metrics['ploop'] - self.polyakov(xinit, 0).abs()).abs()
        return metrics

    # ------------------------------------------------------------ APE and HYP link smearing
    def _smear_checks(self, x: Tensor, what: str, alphas, nsteps) -> tuple[list[float], int]:
        self._no_grad(x, what)
        try:
            al = [float(a) for a in alphas]
        except (TypeError, ValueError):
            al = [float('nan')]
        if not all(0.0 <= a <= 1.0 for a in al):
            raise ValueError(f'LatticeSU3.{what}: every alpha must be a number in [0, 1], got {alphas!r}')
        if isinstance(nsteps, bool) or int(nsteps) != nsteps or int(nsteps) < 0:
            raise ValueError(f'LatticeSU3.{what}: nsteps must be an integer >= 0, got {nsteps!r}')
        return al, int(nsteps)

    @staticmethod
    def _ape_dirmask(dirs: str, time_dir: int) -> int:
        """the APE directions as the 4-bit set of l2q.h: all four ('all'), all but time_dir ('spatial')"""
        if dirs not in ('spatial', 'all'):
            raise ValueError(f"LatticeSU3.ape_smear: dirs must be 'spatial' or 'all', got {dirs!r}")
        if isinstance(time_dir, bool) or int(time_dir) != time_dir or not 0 <= int(time_dir) < 4:
            raise ValueError(f'LatticeSU3.ape_smear: time_dir must be 0..3, got {time_dir!r}')
        return 15 if dirs == 'all' else 15 & ~(1 << int(time_dir))

    def ape_smear_n(self, xn: Tensor, alpha: float = 0.5, nsteps: int = 1, dirs: str = 'spatial',
                    time_dir: int = 0) -> Tensor:
        """`nsteps` APE smearing steps (Albanese et al.) of a native field,
            U'_mu = Proj[(1 - alpha) U_mu + (alpha / 2n) sum_{nu in D, nu != mu} (two staples of direction nu)],
        over the directions D: `dirs='spatial'` the three directions other than `time_dir`, with staples inside the
        slice (n = 2; the links along time_dir are copied and enter nothing, so slices do not mix); `dirs='all'` the 4D
        step (n = 3).  Proj is `l2q_su3_project_su`: the unitary (polar) factor with the determinant phase divided out,
        not the iterative max-Re-tr projection of some codes.  One `l2q_su3_ape_smear` per step, ping-pong between two
        fields; xn is never written.  Returns a new field (xn itself for nsteps = 0).  Any extents; no autograd."""
        (alpha,), nsteps = self._smear_checks(xn, 'ape_smear', [alpha], nsteps)
        mask = self._ape_dirmask(dirs, time_dir)
        bufs: list = [None, None]
        cur = xn
        for k in range(nsteps):
            if bufs[k & 1] is None:
                bufs[k & 1] = torch.empty_like(xn)
            cur = ops.su3_ape_smear_n(cur, alpha, mask, self._lattice_shape, out=bufs[k & 1])
        return cur

    def ape_smear(self, x: Tensor, alpha: float = 0.5, nsteps: int = 1, dirs: str = 'spatial',
                  time_dir: int = 0) -> Tensor:
        """`ape_smear_n` in the reference layout: a new tensor; x is never written."""
        self._smear_checks(x, 'ape_smear', [alpha], nsteps)
        self._ape_dirmask(dirs, time_dir)
        yn = self.ape_smear_n(self.pack(x), alpha, nsteps, dirs, time_dir)
        return AG.attach_native(self.unpack(yn), yn)

    def hyp_smear_n(self, xn: Tensor, alphas=(0.75, 0.6, 0.3), nsteps: int = 1) -> Tensor:
        """`nsteps` HYP smearing steps (Hasenfratz & Knechtli) of a native field with alphas = (alpha1, alpha2, alpha3):
        three nested levels of projected staple sums that stay inside the hypercubes attached to the link
        (`l2q_su3_hyp_level1/2/3`, definitions in include/l2q.h; the projection is that of `ape_smear_n`).  All four
        directions are smeared.  Workspace: the two decorated fields B1, B2 of 12 fields each, six link fields in size
        (3456 B per chain and site: 3.6 GB for 256 chains of 8^4), allocated once per call and reused across nsteps,
        plus the ping-pong result fields; xn is never written.  Returns a new field (xn itself for nsteps = 0).  Any
        extents; no autograd."""
        if not (isinstance(alphas, (tuple, list)) and len(alphas) == 3):
            raise ValueError(f'LatticeSU3.hyp_smear: alphas must be three numbers in [0, 1], got {alphas!r}')
        (a1, a2, a3), nsteps = self._smear_checks(xn, 'hyp_smear', alphas, nsteps)
        L = self._lattice_shape
        cur = xn
        if nsteps > 0:
            b1 = torch.empty((xn.shape[0], 4, 3, 9, xn.shape[-1]), dtype=xn.dtype, device=xn.device)
            b2 = torch.empty_like(b1)
            bufs: list = [None, None]
            for k in range(nsteps):
                if bufs[k & 1] is None:
                    bufs[k & 1] = torch.empty_like(xn)
                ops.su3_hyp_level1_n(cur, a3, L, out=b1)
                ops.su3_hyp_level2_n(cur, b1, a2, L, out=b2)
                cur = ops.su3_hyp_level3_n(cur, b2, a1, L, out=bufs[k & 1])
        return cur

    def hyp_smear(self, x: Tensor, alphas=(0.75, 0.6, 0.3), nsteps: int = 1) -> Tensor:
        """`hyp_smear_n` in the reference layout: a new tensor; x is never written."""
        if not (isinstance(alphas, (tuple, list)) and len(alphas) == 3):
            raise ValueError(f'LatticeSU3.hyp_smear: alphas must be three numbers in [0, 1], got {alphas!r}')
        self._smear_checks(x, 'hyp_smear', alphas, nsteps)
        yn = self.hyp_smear_n(self.pack(x), alphas, nsteps)
        return AG.attach_native(self.unpack(yn), yn)

    def smeared_loop_table(self, x: Tensor, rmax: int, tmax: int, time_dir: int = 0, ape_alpha: float = 0.5,
                           ape_steps: int = 10, hyp_alphas=(0.75, 0.6, 0.3)) -> Tensor:
        """W(R, T) [nb, rmax, tmax] for the static potential, the time direction kept sharp: the spatial lines from
        `ape_steps` spatial APE steps at `ape_alpha`, the temporal lines from one HYP step at `hyp_alphas`:
        `wilson_loop_table_xt(ape_smear(x, ape_alpha, ape_steps, 'spatial', time_dir), hyp_smear(x, hyp_alphas), rmax,
        tmax, time_dir)`.  ape_steps = 0 leaves the spatial lines thin, hyp_alphas None the temporal ones."""
        if time_dir is None:
            raise ValueError('smeared_loop_table: needs a time_dir (0..3)')
        xa = self.ape_smear(x, ape_alpha, ape_steps, 'spatial', time_dir) if int(ape_steps) != 0 else x
        xh = None if hyp_alphas is None else self.hyp_smear(x, hyp_alphas, 1)
        if xh is None:
            return self.wilson_loop_table(xa, rmax, tmax, time_dir)
        return self.wilson_loop_table_xt(xa, xh, rmax, tmax, time_dir)

    # ------------------------------------------------------------ heatbath and overrelaxation sweeps
    def _local_update_checks(self, xn: Tensor, what: str, nsweeps: int, nover: int = 0) -> None:
        if isinstance(xn, torch.Tensor) and xn.requires_grad:
            raise ValueError(f'LatticeSU3.{what}: no autograd through a local update')
        if any(int(n) % 2 for n in self._lattice_shape):
            raise ValueError(f'LatticeSU3.{what}: the checkerboard needs even extents, got {list(self._lattice_shape)}')
        if self.c1 != 0:
            raise ValueError(f'LatticeSU3.{what}: only the Wilson action (c1 = 0), got c1 = {self.c1}')
        if int(nsweeps) < 0 or int(nover) < 0:
            raise ValueError(f'LatticeSU3.{what}: sweep counts must be >= 0, got {nsweeps}, {nover}')

    def _heatbath_checks(self, x: Tensor, beta, nsweeps: int, nover: int, ntry: int) -> None:
        self._local_update_checks(x, 'heatbath', nsweeps, nover)
        b = _beta(beta)
        if not (b > 0 and np.isfinite(b)):
            raise ValueError(f'LatticeSU3.heatbath: beta must be positive and finite, got {b}')
        if not 1 <= int(ntry) <= 16:
            raise ValueError(f'LatticeSU3.heatbath: ntry must be 1..16, got {ntry}')

    def _overrelax_sweeps_(self, xn: Tensor, nsweeps: int) -> None:
        for _ in range(nsweeps):
            for mu in range(4):
                for parity in (0, 1):
                    ops.su3_overrelax_(xn, mu, parity, self._lattice_shape)

    def heatbath_n(self, xn: Tensor, beta, nsweeps: int = 1, nover: int = 0, ntry: int = 4,
                   generator: Optional[torch.Generator] = None, reunitarize: bool = True) -> tuple[Tensor, dict]:
        """`nsweeps` Cabibbo-Marinari heatbath sweeps of the Wilson action at `beta` on a native field, each followed by
        `nover` overrelaxation sweeps; returns (a new field, info); xn is never written.  A sweep is
        `for mu in 0..3: for parity in 0, 1:` one launch each (`l2q_su3_heatbath` / `l2q_su3_overrelax`).  Every
        heatbath launch draws `torch.rand((nb, 3, 4 * ntry + 2, V // 2), dtype=float64)`, in that order: on the device
        with generator None, on the host with a CPU torch.Generator (the parity mode: the same numbers on any machine).
        `ntry` (1..16) Kennedy-Pendleton proposals per SU(2) subgroup; a subgroup for which none is accepted is left as
        it is (still exact) and counted: info['fail_frac'] [nb] = failures / (3 * 4 V * nsweeps).  `reunitarize` projects
        the field on SU(3) once after each full sweep (the drift is rounding only, but accumulates)."""
        self._heatbath_checks(xn, beta, nsweeps, nover, ntry)
        b = _beta(beta)
        nsweeps, nover, ntry = int(nsweeps), int(nover), int(ntry)
        L = self._lattice_shape
        xn = xn.detach().clone()
        nb = xn.shape[0]
        shape = (nb, 3, 4 * ntry + 2, self.volume // 2)
        fails = torch.zeros(nb, dtype=torch.float64, device=xn.device)
        for _ in range(nsweeps):
            for mu in range(4):
                for parity in (0, 1):
                    if generator is None:
                        u = torch.rand(shape, dtype=torch.float64, device=xn.device)
                    else:
                        u = torch.rand(shape, dtype=torch.float64, generator=generator).to(xn.device)
                    fails += ops.su3_heatbath_(xn, b, mu, parity, u, ntry, L)
            self._overrelax_sweeps_(xn, nover)
            if reunitarize:
                xn = ops.su3_project_su_n(xn)
        return xn, {'fail_frac': fails / (3.0 * 4.0 * self.volume * max(nsweeps, 1))}

    def heatbath(self, x: Tensor, beta, nsweeps: int = 1, nover: int = 0, ntry: int = 4,
                 generator: Optional[torch.Generator] = None, reunitarize: bool = True) -> tuple[Tensor, dict]:
        """`heatbath_n` in the reference layout: (x_new, info); x is never written."""
        self._heatbath_checks(x, beta, nsweeps, nover, ntry)
        xn, info = self.heatbath_n(self.pack(x), beta, nsweeps, nover, ntry, generator, reunitarize)
        return AG.attach_native(self.unpack(xn), xn), info

    def overrelax_n(self, xn: Tensor, nsweeps: int = 1) -> Tensor:
        """`nsweeps` microcanonical overrelaxation sweeps (the heatbath's launch order) on a native field: a new field
        with the same Wilson action; xn is never written."""
        nsweeps = int(nsweeps)
        self._local_update_checks(xn, 'overrelax', nsweeps)
        xn = xn.detach().clone()
        self._overrelax_sweeps_(xn, nsweeps)
        return xn

    def overrelax(self, x: Tensor, nsweeps: int = 1) -> Tensor:
        self._local_update_checks(x, 'overrelax', nsweeps)
        xn = self.overrelax_n(self.pack(x), nsweeps)
        return AG.attach_native(self.unpack(xn), xn)

    # ------------------------------------------------------------ Landau and Coulomb gauge fixing
    @staticmethod
    def _gauge_dirmask(gauge: str, time_dir: int, what: str) -> int:
        """the gauge directions as the 4-bit set of l2q.h: all four (Landau), all but time_dir (Coulomb)"""
        if gauge not in ('landau', 'coulomb'):
            raise ValueError(f"LatticeSU3.{what}: gauge must be 'landau' or 'coulomb', got {gauge!r}")
        if isinstance(time_dir, bool) or int(time_dir) != time_dir or not 0 <= int(time_dir) < 4:
            raise ValueError(f'LatticeSU3.{what}: time_dir must be 0..3, got {time_dir!r}')
        return 15 if gauge == 'landau' else 15 & ~(1 << int(time_dir))

    def _gauge_fix_checks(self, x: Tensor, gauge, time_dir, omega, tol, max_sweeps, check_every) -> tuple[int, float]:
        if isinstance(x, torch.Tensor) and x.requires_grad:
            raise ValueError('LatticeSU3.gauge_fix: no autograd through gauge fixing')
        mask = self._gauge_dirmask(gauge, time_dir, 'gauge_fix')
        if any(int(n) % 2 for n in self._lattice_shape):
            raise ValueError('LatticeSU3.gauge_fix: the checkerboard needs even extents, got '
                             f'{list(self._lattice_shape)}')
        omega = GAUGEFIX_OMEGA if omega is None else float(omega)
        if not 1.0 <= omega < 2.0:
            raise ValueError(f'LatticeSU3.gauge_fix: omega must be in [1, 2), got {omega}')
        if not float(tol) > 0:
            raise ValueError(f'LatticeSU3.gauge_fix: tol must be positive, got {tol}')
        if int(check_every) < 1 or int(max_sweeps) < 0:
            raise ValueError(f'LatticeSU3.gauge_fix: need check_every >= 1 and max_sweeps >= 0, got {check_every}, '
                             f'{max_sweeps}')
        return mask, omega

    def _g_to_native(self, g: Tensor) -> Tensor:
        """g[nb, T, X, Y, Z, 3, 3] -> gn[nb, 9, V]"""
        nb = g.shape[0]
        g = g.to(DEVICE).to(torch.complex128)
        return ops.transpose(g.reshape(nb, self.volume, 9), nb, self.volume, 9).reshape(nb, 9, self.volume)

    def _g_from_native(self, gn: Tensor) -> Tensor:
        nb = gn.shape[0]
        return ops.transpose(gn, nb, 9, self.volume).reshape(nb, *self._lattice_shape, 3, 3)

    def gauge_fix_n(self, xn: Tensor, gauge: str = 'landau', time_dir: int = 0, omega: Optional[float] = None,
                    tol: float = 1e-12, max_sweeps: int = 10000, check_every: int = 10, reunitarize: bool = True,
                    return_transform: bool = False) -> tuple[Tensor, dict]:
        """Landau (`gauge='landau'`) or Coulomb (`'coulomb'`, all directions but `time_dir`) gauge fixing of a native
        field by overrelaxed Los Alamos sweeps (`l2q_su3_gaugefix_sweep`, parity 0 then parity 1): maximises the
        functional F until the residual theta <= tol (definitions: include/l2q.h).  Returns (a new field, info); xn is
        never written.  Every `check_every` sweeps one device read of theta[nb]; a chain with theta <= tol is frozen
        from then on, so its result and its sweep count do not depend on its batch mates.  The loop ends when every
        chain is frozen or after `max_sweeps` sweeps; a chain that did not get there shows in info['converged'], nothing
        raises.  A chain that satisfies tol at the start gets no sweep and comes back bit-identical (before
        `reunitarize`, one `l2q_su3_project_su` at the end).  omega in [1, 2), None = GAUGEFIX_OMEGA.
        info: 'theta', 'functional' (of the returned field), 'sweeps' (int64), 'converged' (bool), 'theta0',
        'functional0' (before the first sweep), each [nb]; with return_transform 'g' [nb, T, X, Y, Z, 3, 3], the
        transformation that `gauge_transform` applies (to the input: the result before `reunitarize`)."""
        mask, omega = self._gauge_fix_checks(xn, gauge, time_dir, omega, tol, max_sweeps, check_every)
        tol, max_sweeps, check_every = float(tol), int(max_sweeps), int(check_every)
        L = self._lattice_shape
        xn = xn.detach().clone()
        nb, dev = xn.shape[0], xn.device
        gn = None
        if return_transform:
            gn = torch.zeros((nb, 9, self.volume), dtype=torch.complex128, device=dev)
            gn[:, 0::4] = 1.0
        cond0 = ops.su3_gauge_condition_n(xn, mask, L).cpu()
        cond = cond0.clone()
        live = ~(cond[:, 1] <= tol)                         # (a theta that is not a number stays live, and unconverged)
        sweeps = torch.zeros(nb, dtype=torch.int64)
        done = 0
        while bool(live.any()) and done < max_sweeps:
            n = min(check_every, max_sweeps - done)
            active = live.to(torch.int32).to(dev)
            for _ in range(n):
                for parity in (0, 1):
                    ops.su3_gaugefix_sweep_(xn, parity, mask, omega, L, gn, active)
            done += n
            sweeps[live] += n
            cond = ops.su3_gauge_condition_n(xn, mask, L).cpu()     # frozen chains: untouched, the same bits again
            live = live & ~(cond[:, 1] <= tol)
        converged = ~live
        if reunitarize:
            xn = ops.su3_project_su_n(xn)
            cond = ops.su3_gauge_condition_n(xn, mask, L).cpu()
        info = {'theta': cond[:, 1].to(dev), 'functional': cond[:, 0].to(dev), 'sweeps': sweeps.to(dev),
                'converged': converged.to(dev), 'theta0': cond0[:, 1].to(dev), 'functional0': cond0[:, 0].to(dev)}
        if return_transform:
            info['g'] = self._g_from_native(gn)
        return xn, info

    def gauge_fix(self, x: Tensor, gauge: str = 'landau', time_dir: int = 0, omega: Optional[float] = None,
                  tol: float = 1e-12, max_sweeps: int = 10000, check_every: int = 10, reunitarize: bool = True,
                  return_transform: bool = False) -> tuple[Tensor, dict]:
        """`gauge_fix_n` in the reference layout: (x_fixed, info); x is never written."""
        self._gauge_fix_checks(x, gauge, time_dir, omega, tol, max_sweeps, check_every)
        xn, info = self.gauge_fix_n(self.pack(x), gauge, time_dir, omega, tol, max_sweeps, check_every, reunitarize,
                                    return_transform)
        return AG.attach_native(self.unpack(xn), xn), info

    def gauge_condition(self, x: Tensor, gauge: str = 'landau', time_dir: int = 0) -> GaugeCondition:
        """The gauge functional F and the residual theta of x, [nb] float64 each (`l2q_su3_gauge_condition`; any
        extents)."""
        if isinstance(x, torch.Tensor) and x.requires_grad:
            raise ValueError('LatticeSU3.gauge_condition: no autograd through the gauge condition')
        mask = self._gauge_dirmask(gauge, time_dir, 'gauge_condition')
        c = ops.su3_gauge_condition_n(self.pack(x), mask, self._lattice_shape)
        return GaugeCondition(F=c[:, 0].contiguous(), theta=c[:, 1].contiguous())

    def gauge_transform(self, x: Tensor, g: Tensor) -> Tensor:
        """U_mu(x) -> g(x) U_mu(x) g(x+mu)^H for g[nb, T, X, Y, Z, 3, 3] (`l2q_su3_gauge_apply`; any extents); a new
        tensor."""
        if any(isinstance(a, torch.Tensor) and a.requires_grad for a in (x, g)):
            raise ValueError('LatticeSU3.gauge_transform: no autograd through a gauge transformation')
        want = (x.shape[0], *[int(n) for n in self._lattice_shape], 3, 3)
        if tuple(g.shape) != want:
            raise ValueError(f'LatticeSU3.gauge_transform: g must be {list(want)}, got {list(g.shape)}')
        yn = ops.su3_gauge_apply_n(self.pack(x), self._g_to_native(g), self._lattice_shape)
        return AG.attach_native(self.unpack(yn), yn)

    # ------------------------------------------------------------ reference API
    def coeffs(self, beta: Tensor) -> dict[str, Tensor]:
        return {'plaq': beta * (1.0 - 8.0 * self.c1), 'rect': beta * self.c1}

    def wilson_loops(self, x: Tensor) -> Tensor:
        """tr P for the 6 planes (u > v) and every site: [6, nb, T, X, Y, Z] complex, the tensor the
        reference returns (lattice.py:242-244), from `l2q_su3_wilson_loops` (differentiable:
        `l2q_su3_wilson_loops_bwd`).  The sampler itself never materialises it (`plaq_sums`)."""
        if AG.wants_grad(x):
            return AG.SU3WilsonLoops.apply(x.to(DEVICE), self._lattice_shape)
        return ops.su3_wilson_loops_n(self.pack(x), self._lattice_shape)

    def plaq_sums(self, x: Tensor) -> PlaqSums:
        """the per-chain reductions of `wilson_loops(x)` in one fused pass (no field written)"""
        if AG.wants_grad(x):
            # differentiable route (loss.backward() of an autograd caller): l2q_su3_plaq_bwd behind it
            return PlaqSums(AG.SU3PlaqPlanes.apply(x.to(DEVICE), self._lattice_shape).sum(1))
        return PlaqSums(self.plaq_sums_n(self.pack(x)))

    def _wilson_loops(self, x: Tensor, needs_rect: bool = False) -> tuple[Tensor, Tensor]:
        """(plaquette traces [6, nb, T, X, Y, Z], rectangle traces [12, nb, T, X, Y, Z]) like the
        reference (lattice.py:157-199); without `needs_rect` the second is zeros (a broadcast view)."""
        ps = self.wilson_loops(x)
        if not needs_rect:
            return ps, torch.zeros((), dtype=ps.dtype, device=ps.device).expand(12, *ps.shape[1:])
        rects = []
        for u in range(1, self.dim):
            for v in range(u):
                rects.extend(self.g.trace(r) for r in self._rectangles(x, u, v))
        return ps, torch.stack(rects)

    def _plaquettes(self, x: Tensor) -> Tensor:
        return self._plaqs(self.plaq_sums(x))

    def plaqs(self, x: Optional[Tensor] = None, wloops=None) -> Tensor:
        return self._plaqs(self.plaq_sums(x) if wloops is None else wloops)

    def charges(self, x: Optional[Tensor] = None, wloops=None) -> Charges:
        return self._charges(self.plaq_sums(x) if wloops is None else wloops)

    def int_charges(self, x: Optional[Tensor] = None, wloops=None) -> Tensor:
        return self._int_charges(self.plaq_sums(x) if wloops is None else wloops)

    def sin_charges(self, x: Optional[Tensor] = None, wloops=None) -> Tensor:
        return self._sin_charges(self.plaq_sums(x) if wloops is None else wloops)

    # the helpers take the reference's trace field (a Tensor, lattice.py:208-240) or a PlaqSums
    @staticmethod
    def _re_sum(wloops) -> Tensor:
        return wloops.re if isinstance(wloops, PlaqSums) else _site_sum(wloops.real)

    @staticmethod
    def _im_sum(wloops) -> Tensor:
        return wloops.im if isinstance(wloops, PlaqSums) else _site_sum(wloops.imag)

    def _plaqs(self, wloops) -> Tensor:
        return self._re_sum(wloops) / (6 * 3 * self.volume)

    def _charges(self, wloops) -> Charges:
        return Charges(intQ=self._int_charges(wloops), sinQ=self._sin_charges(wloops))

    def _int_charges(self, wloops) -> Tensor:
        return self._im_sum(wloops) / (32 * (np.pi ** 2))

    def _sin_charges(self, wloops) -> Tensor:
        return self._im_sum(wloops) / (6 * 3 * self.volume)

    def kinetic_energy(self, v: Tensor) -> Tensor:
        return self.g.kinetic_energy(v)

    # ---- per-site plaquette matrices (observables / debugging helpers, lattice.py:93-155);
    # the sampler itself only ever needs the reductions above
    def _link_staple_op(self, link: Tensor, staple: Tensor) -> Tensor:
        return self.g.mul(link, staple)

    def _plaquette(self, x: Tensor, u: int, v: int) -> Tensor:
        """U_u(x) U_v(x+u) U_u(x+v)^H U_v(x)^H as a matrix field [nb, T, X, Y, Z, 3, 3]"""
        x = x.to(DEVICE).reshape(x.shape[0], *self._shape[1:])
        xu, xv = x[:, u], x[:, v]
        xuv = self.g.mul(xu, xv.roll(shifts=-1, dims=(u + 1)))
        xvu = self.g.mul(xv, xu.roll(shifts=-1, dims=(v + 1)))
        return self.g.mul(xuv, xvu, adjoint_b=True)

    def _trace_plaquette(self, x: Tensor, u: int, v: int) -> Tensor:
        return self.g.trace(self._plaquette(x, u, v))

    def _plaquette_field(self, x: Tensor, needs_rect: bool = False):
        """matrix fields of the 6 plaquettes (and the 12 rectangles), lattice.py:132-155"""
        plaqs = [self._plaquette(x, u, v) for u in range(1, self.dim) for v in range(u)]
        rects = None
        if needs_rect:
            rects = []
            for u in range(1, self.dim):
                for v in range(u):
                    rects.extend(self._rectangles(x, u, v))
            rects = torch.stack(rects)
        return torch.stack(plaqs), rects

    def _rectangles(self, x: Tensor, u: int, v: int) -> tuple[Tensor, Tensor]:
        """The two 2x1 loops of plane (u, v) as matrix fields (lattice.py:96-112): an
        observables / debugging helper, the sampler only needs rect_sums_n."""
        x = x.to(DEVICE).reshape(x.shape[0], *self._shape[1:])
        xu, xv = x[:, u], x[:, v]
        xuv = self.g.mul(xu, xv.roll(shifts=-1, dims=(u + 1)))
        xvu = self.g.mul(xv, xu.roll(shifts=-1, dims=(v + 1)))
        yu = xu.roll(-1, dims=v + 1)
        yv = xv.roll(-1, dims=u + 1)
        uu = self.g.mul(xv, xuv, adjoint_a=True)
        ur = self.g.mul(xu, xvu, adjoint_a=True)
        ul = self.g.mul(xuv, yu, adjoint_b=True)
        ud = self.g.mul(xvu, yv, adjoint_b=True)
        ul_ = ul.roll(-1, dims=u + 1)
        ud_ = ud.roll(-1, dims=v + 1)
        return self.g.mul(ur, ul_, adjoint_b=True), self.g.mul(uu, ud_, adjoint_b=True)

    def _action(self, wloops, beta: Tensor) -> Tensor:
        """The reference's unused opposite-sign variant (lattice.py:271-285): +coeff sum Re tr P / 3."""
        ps, rs = wloops if isinstance(wloops, tuple) else (wloops, None)
        c = self.coeffs(torch.as_tensor(_beta(beta)))
        action = c['plaq'] * self._re_sum(ps)
        if self.c1 != 0 and rs is not None:
            action = action + c['rect'] * (_site_sum(rs.real) if rs.dim() > 1 else rs)
        return action / 3.0

    def plaq_loss(self, acc: Tensor, x1=None, x2=None, wloops1=None, wloops2=None):
        log.error('TODO')                       # a stub in the reference as well (lattice.py:351-359)

    def charge_loss(self, acc: Tensor, x1=None, x2=None, wloops1=None, wloops2=None):
        log.error('TODO')                       # (lattice.py:361-369)

    def action(self, x: Tensor, beta: Tensor) -> Tensor:
        """-(1/3) (c_plaq sum Re tr P + c_rect sum Re tr R) (lattice.py:252-269)"""
        if AG.wants_grad(x):
            b = _beta(beta)
            s = (-b * (1.0 - 8.0 * self.c1) / 3.0) * AG.SU3PlaqPlanes.apply(
                x.to(DEVICE), self._lattice_shape)[:, :, 0].sum(1)
            if self.c1 != 0.0:
                s = s + (-b * self.c1 / 3.0) * AG.SU3RectSums.apply(x.to(DEVICE), self._lattice_shape)
            return s
        return self.action_n(self.pack(x), beta)

    def action_with_grad(self, x: Tensor, beta: Tensor) -> tuple[Tensor, Tensor]:
        xn = self.pack(x)
        return self.action_n(xn, beta), self.unpack(self.grad_action_n(xn, beta))

    def grad_action(self, x: Tensor, beta: Tensor) -> Tensor:
        """(beta/3) TAH(U * staples)  ==  projectTAH(autograd dS/dx @ x^H) (lattice.py:299-308)"""
        return self.unpack(self.grad_action_n(self.pack(x), beta))

    def calc_metrics(self, x: Tensor, beta: Optional[Tensor] = None,
                     xinit: Optional[Tensor] = None, flow_time: Optional[float] = None,
                     flow_eps: float = 0.01) -> dict[str, Tensor]:
        """The reference's metrics; with `flow_time` also the clover charge and t^2 E of x flowed to that time
        ('Qflow', 't2E', and 'dQflow' = |Qflow(x) - Qflow(xinit)| when xinit is given)."""
        w = self.plaq_sums(x)
        q = self._charges(w)
        metrics = {'plaqs': self._plaqs(w), 'sinQ': q.sinQ, 'intQ': q.intQ}
        if beta is not None:
            s, dsdx = self.action_with_grad(x, beta)
            metrics.update({'action': s, 'dsdx': dsdx})
            if xinit is not None:
                s_, dsdx_ = self.action_with_grad(xinit, beta)
                metrics.update({'daction': (s - s_).abs(), 'dsdx': (dsdx - dsdx_).abs()})
        if xinit is not None:
            w_ = self.plaq_sums(xinit)
            q_ = self._charges(w_)
            metrics.update({'dplaqs': (metrics['plaqs'] - self._plaqs(w_)).abs(),
                            'dQint': (q.intQ - q_.intQ).abs(),
                            'dQsin': (q.sinQ - q_.sinQ).abs()})
        if flow_time is not None:
            n = self._flow_steps(float(flow_time), float(flow_eps))
            c = self.clover_n(self.flow_n(self.pack(x), n, flow_eps))
            metrics.update({'Qflow': c.Q, 't2E': float(flow_time) ** 2 * c.E})
            if xinit is not None:
                c_ = self.clover_n(self.flow_n(self.pack(xinit), n, flow_eps))
                metrics['dQflow'] = (c.Q - c_.Q).abs()
        return metrics
