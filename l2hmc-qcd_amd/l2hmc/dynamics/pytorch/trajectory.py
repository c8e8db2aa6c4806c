"""The L2HMC trajectory (reference dynamics.py:956-1063) written once.

`run_trajectory` owns the bookkeeping -- the leapfrog loop, the momentum flip, the logdet sums, the per-step
metrics, the final Hamiltonian, the accept probability, the history -- and is told by a *stepper* how one
leapfrog step is taken: `SamplerStepper` (in place, `Dynamics._lf_n`) or `training.TapeStepper`
(functional, recorded for the reverse sweep).  A stepper has

    start(xn, vn) -> (x, v)                       the tensors the steps work on
    step(step, x, v, forward) -> (x, v, logdet)
    flip(v) -> v                                  the merged trajectory's v -> -v
    finish(x, v) -> logdet or None                a closing update that is still pending
    late (with ld1, ke)                           the metrics of a step arrive one call late (see `SamplerStepper`)
"""
from __future__ import annotations

import torch

Tensor = torch.Tensor

_WITH_FORCE = object()        # a potential energy that the next force launch delivers (SamplerStepper.energies)


class SamplerStepper:
    """In-place steps of the sampler and everything that is local to ONE of its trajectories:

    reuse    the force, the vec8 network inputs and the hidden activation are kept per distinct x
             (`valid`, `F`, `xv`, `fv`, `z` by network; `xv_pre`: vec8(x) emitted by the x-update that made x)
    defer    the closing v-update of a step runs together with the next step's opening one
             (`pending` = (step, forward, flip) of the update that has not run yet)
    late     ... under verbose=True: the mid-point pair kernel leaves the deferred update's logdet and the
             kinetic energy right after it in `ld1` / `ke`, so a step's metrics are complete one call late
    x_src, v_src   SU(3): the first step READS the trajectory's input from there and writes x / v, so the
             input is never copied
    energies ... with `defer`, where `Dynamics._kernel_energies` allows: the Hamiltonian's terms come out of the
             kernels that hold them.  `plaq` (beside `F`): sum Re tr P of the x the force was taken at, from the
             force launches whose potential is consumed (`want_pe`: the closing one; `late`: every one but the first);
             `ke_out`: the kinetic energy of the momentum the closing update wrote (None: that kernel does not
             emit it)"""
    __slots__ = ('dyn', 'beta', 'reuse', 'defer', 'late', 'lazy', 'x_src', 'v_src',
                 'valid', 'F', 'xv_pre', 'xv', 'fv', 'z',
                 'pending', 'ld1', 'ke', 'energies', 'want_pe', 'plaq', 'ke_out')

    def __init__(self, dyn, beta, merged: bool):
        verbose = dyn.config.verbose
        su3 = dyn.group == 'SU3' and dyn._networks_built
        self.dyn, self.beta = dyn, beta
        self.reuse = bool(dyn.reuse_v_inputs)
        # (the single-direction kernel neither pairs its v-updates nor reads its input in place)
        can_pair = merged and su3 and self.reuse and dyn.pair_v_updates
        self.late = bool(verbose and can_pair and dyn.pair_v_updates_verbose and dyn._can_pair_mid())
        self.defer = bool(can_pair and (not verbose or self.late))
        self.x_src = self.v_src = None
        self.valid = False
        self.F = self.xv_pre = self.xv = self.fv = None
        self.z = {}
        self.pending = self.ld1 = self.ke = None
        self.lazy = bool(merged and su3 and dyn.config.nleapfrog > 0)
        self.energies = self.want_pe = False
        self.plaq = self.ke_out = None

    def start(self, xn: Tensor, vn: Tensor):
        self.energies = bool(self.defer and self.lazy and self.dyn._kernel_energies(xn))
        if not self.lazy:
            return xn.clone(), vn.clone()
        self.x_src, self.v_src = xn, vn
        return torch.empty_like(xn), torch.empty_like(vn)

    def step(self, step: int, x: Tensor, v: Tensor, forward: bool):
        return x, v, self.dyn._lf_n(step, x, v, self.beta, forward, self)

    def flip(self, v: Tensor) -> Tensor:
        if self.pending is None:
            return self.dyn._flip_v_n(v)
        self.pending = (*self.pending[:2], True)        # the flip happens inside the paired kernel
        return v

    def finish(self, x: Tensor, v: Tensor):
        return self.dyn._flush_pending_n(self, x, v, self.beta)

    def potential(self, x: Tensor) -> Tensor:
        """of the x the last force was taken at (`energies`); the separate pass where no launch emitted it"""
        if self.plaq is None:
            return self.dyn._potential_n(x, self.beta)
        return self.dyn._potential_from_plaq(self.plaq, self.beta)

    def kinetic_out(self, v: Tensor) -> Tensor:
        """of the momentum `finish` left (`energies`)"""
        return self.dyn._kinetic_n(v) if self.ke_out is None else self.ke_out


def run_trajectory(dyn, stepper, xn: Tensor, vn: Tensor, beta, directions: tuple):
    """`directions` = (True, False): the merged forward + backward trajectory (dynamics.py:956-1029);
    (forward,): the single-direction one (:1031-1063), whose accept probability takes the reference's
    SWAPPED arguments.  Returns (x', v', history, H_init, H_final)."""
    merged = len(directions) == 2
    verbose, nlf = dyn.config.verbose, dyn.config.nleapfrog
    x, v = stepper.start(xn, vn)
    # SamplerStepper.energies: the potential of a step's x comes out of the force launch on it -- the next call's
    # (or `finish`'s) -- and the closing kinetic energy out of `finish`; the opening potential stays a pass
    energies = getattr(stepper, 'energies', False)
    # (every sum below is out of place: the history holds the earlier tensors)
    sumlogdet = dyn._zeros_nb(xn.shape[0])
    sldf = sldb = torch.zeros_like(sumlogdet) if merged else None
    history: dict = {}
    h = h_init = dyn._hamiltonian_n(xn, vn, beta)

    def add_sld(forward, logdet):
        nonlocal sldf, sldb
        if forward:
            sldf = sldf + logdet
        else:
            sldb = sldb + logdet

    def record(energy, idx=None, forward=True):
        m = {'energy': energy, 'logprob': energy - sumlogdet, 'logdet': sumlogdet}
        if merged:
            m.update({'sldf': sldf if forward else torch.zeros_like(sldb), 'sldb': sldb,
                      'sld': sumlogdet})
        if idx is not None:
            m.update({'xeps': dyn.xeps[idx], 'veps': dyn.veps[idx]})
        dyn.update_history(m, history)
        return energy

    if verbose:
        record(h_init, 0 if merged else None)
    # a step whose closing update has not run yet (stepper.late): its potential energy, step-size index, direction
    late_pe = late_idx = late_fwd = None
    for i, forward in enumerate(directions):
        if i > 0:
            v = stepper.flip(v)
        for step in range(nlf):
            x, v, logdet = stepper.step(step, x, v, forward)
            if late_pe is not None:                    # the previous step's closing update ran now
                sumlogdet = sumlogdet + stepper.ld1
                add_sld(late_fwd, stepper.ld1)
                if late_pe is _WITH_FORCE:             # ... on the force of that step's x (x_prev, no longer held)
                    late_pe = dyn._potential_from_plaq(stepper.plaq, beta)
                h = record(stepper.ke + late_pe, late_idx, late_fwd)
            sumlogdet = sumlogdet + logdet
            if not verbose:
                continue
            if merged:
                add_sld(forward, logdet)
            idx = step if (forward or not merged) else nlf - step - 1
            if stepper.late:
                late_pe = _WITH_FORCE if energies else dyn._potential_n(x, beta)
                late_idx, late_fwd = idx, forward
            else:
                h = record(dyn._hamiltonian_n(x, v, beta), idx, forward)
    last = stepper.finish(x, v)
    if last is not None:
        sumlogdet = sumlogdet + last
    if late_pe is not None:
        if last is not None:
            add_sld(late_fwd, last)
        if late_pe is _WITH_FORCE:
            h = record(stepper.kinetic_out(v) + stepper.potential(x), late_idx, late_fwd)
        else:
            h = record(dyn._kinetic_n(v) + late_pe, late_idx, late_fwd)
    if not verbose or nlf == 0:                        # (verbose: the last record's energy is H of the final state)
        h = stepper.kinetic_out(v) + stepper.potential(x) if energies else dyn._hamiltonian_n(x, v, beta)
    h_pair = (h_init, h) if merged else (h, h_init)        # single direction: the reference's swapped call
    acc = dyn._accept_prob_n(*h_pair, sumlogdet)
    history.update({'acc': acc, 'sumlogdet': sumlogdet})
    if verbose:
        history = dyn._stack_history(history)
    return x, v, history, h_init, h
