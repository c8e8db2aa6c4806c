"""The L2HMC trajectory (reference dynamics.py:956-1063) written once.

`run_trajectory` owns the bookkeeping -- the leapfrog loop, the momentum flip, the logdet sums, the per-step
metrics, the final Hamiltonian, the accept probability, the history -- and is told by a *stepper* how one
leapfrog step is taken: `SamplerStepper` (in place; it owns everything that is local to one trajectory of the
sampler, on top of the stateless `Dynamics._lf_n`) or `training.TapeStepper` (functional, recorded for the reverse
sweep).  A stepper has

    start(xn, vn) -> (x, v)                       the tensors the steps work on
    step(step, x, v, forward) -> (x, v, logdet)
    flip(v) -> v                                  the merged trajectory's v -> -v
    finish(x, v) -> logdet or None                a closing update that is still pending
    late (with ld1, ke)                           the metrics of a step arrive one call late (see `SamplerStepper`)
    energies (with plaq, potential(x), kinetic_out(v))   the Hamiltonian's terms come out of the steps' kernels (ditto)
"""
from __future__ import annotations

import torch

from l2hmc import _ops as ops

Tensor = torch.Tensor

_WITH_FORCE = object()        # a potential energy that the next force launch delivers (SamplerStepper.energies)
# (complement, first) of the two x half-updates of a leapfrog step, by direction (dynamics.py:1187-1228)
X_HALVES = {True: ((False, True), (True, False)), False: ((True, False), (False, True))}


class VInputs:
    """What is known about the CURRENT x for the v-updates taken at it: the force, the vec8 network inputs (fp64, or
    the int8 digit images of csrc/digits.hpp) and the hidden activation of every network that ran on them.  They
    depend only on x (and the network), and x does not change between the closing v-update of one leapfrog step and
    the opening v-update of the next (nor across the momentum flip), so an owner that says `x_changed` exactly when x
    did has them computed once per distinct x -- 9 instead of 16 evaluations in a merged nlf = 4 trajectory.  Same
    inputs, same deterministic kernels: bitwise identical results.  An owner that keeps nothing
    (`reuse_v_inputs = False`, the stateless `Dynamics._update_v_n`) says `x_changed` before every update.

    `plaq`: sum Re tr P of the x the LAST force was taken at when that launch was asked for it (`want_pe`), else
    None; it outlives `x_changed` (the late metrics read it after the x-update)."""
    __slots__ = ('dyn', 'beta', 'plaq', 'F', 'xv', 'fv', 'z', 'upper')

    def __init__(self, dyn, beta, upper: bool = True):
        """`upper`: F may be held as an `ops.UpperForce` where every consumer takes one (`_upper_ok`); an owner
        that hands F out (`Dynamics._v_inputs_n`) says False."""
        self.dyn, self.beta, self.plaq, self.upper = dyn, beta, None, upper
        self.x_changed()

    def x_changed(self, emitted=None) -> None:
        """`emitted`: vec8 of the NEW x (or its digit image), where the x-update that made it wrote that too."""
        self.F = self.fv = None
        self.xv, self.z = emitted, {}

    def _upper_ok(self, vnet, hs, xn: Tensor) -> bool:
        """The force of this x may keep only its six upper planes: its two readers are then the digit projection
        and the int8-sliced heads kernel of `vnet`, which both take that form.  The sampler only, SU(3) with the
        plain Wilson action, on the lattices whose force kernel has that output; not under injected draws (the
        launch-by-launch parity runs).  `dyn.upper_plane_force = False` keeps the full field everywhere."""
        dyn = self.dyn
        return bool(self.upper and dyn.upper_plane_force and hs is not None and dyn.group == 'SU3'
                    and dyn.potential_c1 == 0.0 and not dyn.training and dyn._inject is None and xn.is_cuda
                    and ops.heads_take_upper_force(hs) and dyn._digit_inputs(vnet, xn.shape[0], xn.shape[-1])
                    and ops.su3_force_upper_ok(xn.shape[0], dyn.latvolume))

    def get(self, vnet, xn: Tensor, want_pe: bool = False):
        """(force, hidden activation z, kernel weights) for the fused heads kernel; (force, None, None) where that
        kernel does not run.  `want_pe`: the potential of this x is consumed, so a force that is not held yet
        comes from the launch that also returns the plaquette sum.  The force is an `ops.UpperForce` where
        `_upper_ok`, else the full field."""
        dyn = self.dyn
        w = hs = None
        if dyn._can_fuse_heads(vnet):
            p = dyn._perms()
            w = vnet.kernel_weights(p['in'], p['out'])
            hs = w['heads_scaled']
            # int8 slice image of the head weights (csrc/heads_sliced.hip); lives in the version-keyed
            # weight cache, so it is rebuilt whenever a parameter changes.  Both knobs are consulted on
            # EVERY call (`use_sliced`), the image is built the first time they are both on.
            hs['use_sliced'] = bool(dyn._sliced_wanted(vnet) and ops.USE_SLICED_HEADS[0])
            if hs['use_sliced'] and 'sliced' not in hs:
                hs['sliced'] = ops.heads_sliced_build(hs)
        upper = self._upper_ok(vnet, hs, xn)
        if self.F is None or (isinstance(self.F, ops.UpperForce) and not upper):
            # (an upper-plane force held for another network of this x that this one cannot read: taken again as
            # the full field, the same bits; the projection and the plaquette sum of the first are kept)
            held = None if self.F is None else self.plaq
            if upper:
                self.F, self.plaq = ops.su3_force_upper_n(xn, float(self.beta), dyn.latvolume, want_pe)
            else:
                self.F, self.plaq = (ops.su3_force_action_n(xn, float(self.beta), dyn.latvolume) if want_pe
                                     else (dyn._force_n(xn, self.beta), None))
            if self.plaq is None:
                self.plaq = held
        fn = self.F
        if w is None:
            return fn, None, None
        z = self.z.get(id(vnet))
        if z is None:
            nb = xn.shape[0]
            digits = dyn._digit_inputs(vnet, nb, xn.shape[-1])
            project = ops.su3_projsu_digits_n if digits else (lambda a: ops.su3_projsu_vec8_n(a).reshape(nb, -1))
            xv, fv = self.xv, self.fv
            if fv is None:                       # the first network at this x: xv is what the x-update emitted
                if xv is None or isinstance(xv, ops.DigitImage) != digits:
                    xv = project(xn)             # (nothing emitted, or a knob changed since the x-update: x is at hand)
                fv = project(fn)
                self.xv, self.fv = xv, fv
            elif isinstance(xv, ops.DigitImage) and not digits:
                xv, fv = project(xn), project(fn)    # kept for another network of this x; this one takes fp64 inputs
            z = self.z[id(vnet)] = vnet.hidden_flat(xv, fv, w,
                                                    sliced_exp=ops.SLICED_INPUT_EXP if dyn.sliced_input else None)
        return fn, z, w

    def update_v(self, step: int, xn: Tensor, vn: Tensor, forward: bool, v_src=None, norm2=None, want_pe=False):
        """The v-update (dynamics.py:1266-1297) on these inputs, in place; returns logdet [nb].  `v_src`: the momentum
        is read from there and only written to vn (the heads kernel does that itself; the other path copies first).
        `norm2`: a list that receives sum |v'|^2 [nb] of the updated momentum when the kernel that runs emits it
        (ops.vnet_heads_vupdate_), and stays empty otherwise."""
        dyn = self.dyn
        nb, eps, vnet = xn.shape[0], dyn._eps('v', step), dyn._get_vnet(step)
        fn, z, w = self.get(vnet, xn, want_pe)
        if z is not None:
            # heads + momentum update in one kernel: s, t, q never reach HBM
            return ops.vnet_heads_vupdate_(z, w['heads_scaled'], (vnet.nw.s, vnet.nw.t, vnet.nw.q),
                                           vn.reshape(nb, -1), ops.flat_force(fn, nb), eps, forward,
                                           None if v_src is None else v_src.reshape(nb, -1), norm2=norm2)
        if v_src is not None:
            vn.copy_(v_src)
        s, t, q = dyn._vnet_n(step, xn, fn)
        return ops.v_update_(vn.reshape(nb, -1), fn.reshape(nb, -1), s, t, q, eps, forward)


class SamplerStepper:
    """In-place steps of the sampler and everything that is local to ONE of its trajectories:

    reuse    what the v-updates need of x is kept per distinct x (`inputs`, a `VInputs`)
    defer    the closing v-update of a step runs together with the next step's opening one (`v_slot`;
             `pending` = (step, forward) of the update that has not run yet, `flipped`: the momentum flip came after it)
    late     ... under verbose=True: the mid-point pair kernel leaves the deferred update's logdet and the
             kinetic energy right after it in `ld1` / `ke`, so a step's metrics are complete one call late
    x_src, v_src   SU(3): the first step READS the trajectory's input from there and writes x / v: it is never copied
    energies ... with `defer`, where `Dynamics._kernel_energies` allows: the Hamiltonian's terms come out of the
             kernels that hold them (`v_slot`).  `plaq`: sum Re tr P of the x the force was taken at; `ke_out`: the
             kinetic energy of the momentum the closing update wrote (None: that kernel does not emit it)"""
    __slots__ = ('dyn', 'beta', 'reuse', 'defer', 'late', 'lazy', 'x_src', 'v_src', 'inputs',
                 'pending', 'flipped', 'ld1', 'ke', 'energies', 'ke_out')

    def __init__(self, dyn, beta, merged: bool, xv=None):
        """`xv`: the vnet input of the trajectory's first x (or its digit image), where the entry emitted it"""
        verbose, su3 = dyn.config.verbose, dyn.group == 'SU3' and dyn._networks_built
        self.dyn, self.beta, self.inputs = dyn, beta, VInputs(dyn, beta)
        self.inputs.x_changed(xv)
        self.reuse = bool(dyn.reuse_v_inputs)
        # (the single-direction kernel neither pairs its v-updates nor reads its input in place)
        can_pair = merged and su3 and self.reuse and dyn.pair_v_updates
        self.late = bool(verbose and can_pair and dyn.pair_v_updates_verbose and dyn._can_pair_mid())
        self.defer = bool(can_pair and (not verbose or self.late))
        self.lazy = bool(merged and su3 and dyn.config.nleapfrog > 0)
        self.x_src = self.v_src = self.pending = self.ld1 = self.ke = self.ke_out = None
        self.energies = self.flipped = False

    plaq = property(lambda self: self.inputs.plaq)

    def start(self, xn: Tensor, vn: Tensor):
        self.energies = bool(self.defer and self.lazy and self.dyn._kernel_energies(xn))
        if not self.lazy:
            return xn.clone(), vn.clone()
        self.x_src, self.v_src = xn, vn
        return torch.empty_like(xn), torch.empty_like(vn)

    def step(self, step: int, x: Tensor, v: Tensor, forward: bool):
        """One generalised leapfrog step in place (dynamics.py:1187-1228): v-slot, x-update, and the closing v-update
        -- at once, or (`defer`) in the next v-slot, whose call then returns its logdet."""
        dyn = self.dyn
        st = step if forward else dyn.config.nleapfrog - step - 1
        m = dyn._native_masks()[st]
        ld = dyn._lf_fused_u1_n(st, x, v, m, self.beta, forward)
        if ld is not None:                              # (it holds its force: nothing of it is local to the trajectory)
            return x, v, ld
        x_src, v_src, self.x_src, self.v_src = self.x_src, self.v_src, None, None
        xr = x if x_src is None else x_src              # where this step reads x before its x-update
        ld = self.v_slot(self._take_pending(), (st, forward), xr, v, v_src)
        vnet = dyn._get_vnet(st)
        if dyn.group == 'SU3' and dyn.fuse_x_updates and self.reuse and dyn.fuse_x_vec8 and dyn._can_fuse_heads(vnet):
            # both half-updates in one kernel that also emits the next vnet input, vec8(x')
            nb, eps = x.shape[0], dyn._eps('x', st) * (1 if forward else -1)
            if dyn._digit_inputs(vnet, nb, x.shape[-1]):
                pre = ops.su3_expm_mul2_digits_n(xr, v, eps, m, not forward, out=x)[1]
            else:
                pre = ops.su3_expm_mul2_vec8_n(xr, v, eps, m, not forward, out=x)[1].reshape(nb, -1)
            self.inputs.x_changed(pre)
        else:
            ld = dyn._update_x_both_n(st, x, v, m, forward, ld, x_src)
            self.inputs.x_changed()
        if self.defer:
            self.pending = (st, forward)
            return x, v, ld
        return x, v, ld + self.v_slot((st, forward, False), None, x, v)

    def flip(self, v: Tensor) -> Tensor:
        if self.pending is None:
            return self.dyn._flip_v_n(v)
        self.flipped = True                             # the v-slot that runs the pending update flips after it
        return v

    def finish(self, x: Tensor, v: Tensor):
        return self.v_slot(self._take_pending(), None, x, v)

    def _take_pending(self):
        closing = None if self.pending is None else (*self.pending, self.flipped)
        self.pending, self.flipped = None, False
        return closing

    def _update_v(self, st: int, forward: bool, x: Tensor, v: Tensor, **kw) -> Tensor:
        if not self.reuse:
            self.inputs.x_changed()
        vnet = self.dyn._get_vnet(st)
        if self.dyn._fused_u1(vnet) is not None or self.dyn._half_fused(vnet):  # (U(1) kernels that take no kept force)
            return self.dyn._update_v_n(st, x, v, self.beta, forward)
        return self.inputs.update_v(st, x, v, forward, **kw)

    def v_slot(self, closing, opening, x: Tensor, v: Tensor, v_src=None):
        """Everything between two x-updates, at one x: the closing v-update `(step, forward, flip)` of one leapfrog
        step, the merged trajectory's v -> -v after it where `flip` (dynamics.py:1001), and the opening v-update
        `(step, forward)` of the next step; either may be None (the first step, whose opening update reads the
        momentum from `v_src`; `finish`, or a closing update that is not deferred).  Returns the sum of the logdets.
        Closing and opening on one network whose heads are fused (same x, same network => same s, t, q) take ONE
        evaluation of the heads, the pair kernel.  With `late` (per-step metrics, verbose=True) that is the mid-point
        kernel, which also returns the closing update's logdet and the kinetic energy of the momentum between the
        two updates: they are left in `ld1` / `ke`, and the return value is the OPENING update's logdet alone.
        `energies`: the force launch of a closing update leaves the potential of this x in `plaq` where that is
        consumed -- at the trajectory's last update, and under `late` at every one (the opening update of the first
        step has none: the potential of the trajectory's input stays a pass) -- and the last update leaves the
        kinetic energy of the final momentum in `ke_out` (the sign flip does not change it)."""
        dyn, nb = self.dyn, x.shape[0]
        st0, f0, flip = closing or (None, None, False)
        st1, f1 = opening or (None, None)
        want_pe = bool(self.energies and closing and (self.late or not opening))
        vnet = dyn._get_vnet(st1) if closing and opening else None
        if vnet is not None and dyn._get_vnet(st0) is vnet and dyn._can_fuse_heads(vnet):
            fn, z, w = self.inputs.get(vnet, x, want_pe)
            args = (z, w['heads_scaled'], (vnet.nw.s, vnet.nw.t, vnet.nw.q), v.reshape(nb, -1), ops.flat_force(fn, nb),
                    dyn._eps('v', st0), f0, flip, dyn._eps('v', st1), f1)
            if not self.late:
                return ops.vnet_heads_vupdate_pair_(*args)
            ld, self.ld1, vn2 = ops.vnet_heads_vupdate_pair_mid_(*args)
            self.ke = dyn._kinetic_from_norm2(vn2)
            return ld - self.ld1
        ld = None
        if closing:
            n2 = [] if (self.energies and not opening) else None
            ld = self._update_v(st0, f0, x, v, norm2=n2, want_pe=want_pe)
            if not opening:
                self.ke_out = dyn._kinetic_from_norm2(n2[0]) if n2 else None
            elif self.late:
                self.ld1, self.ke = ld, dyn._kinetic_n(v)
            if flip:
                dyn._flip_v_n(v)
        if opening:
            l1 = self._update_v(st1, f1, x, v, v_src=v_src)
            ld = l1 if (ld is None or self.late) else ld + l1
        return ld

    def potential(self, x: Tensor) -> Tensor:
        """of the x the last force was taken at (`energies`); the separate pass where no launch emitted it"""
        dyn, plaq = self.dyn, self.plaq
        return dyn._potential_n(x, self.beta) if plaq is None else dyn._potential_from_plaq(plaq, self.beta)

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
    energies = stepper.energies
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
