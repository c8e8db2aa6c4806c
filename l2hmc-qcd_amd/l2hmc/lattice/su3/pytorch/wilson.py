"""The host side of the Wilson fermions on `LatticeSU3` (kernels: csrc/su3_wilson.hip, csrc/su3_wilson_eo.hip,
csrc/su3_wilson_f32.hip, csrc/su3_wilson_force.hip, csrc/su3_wilson_clover.hip, csrc/su3_clover_force.hip): the mixin ``WilsonFermions`` with the
operator, the two solvers on one CG loop (``_CG``), their even-odd and mixed-precision forms (``_MixedSolve``: fp64 defect
correction around the same loop on fp32 fields), the clover-improved operator and its even-odd solve (``CloverTerm``,
``_CloverSchurOp``), the multi-shift CG (``_CG.multishift``, kernels: csrc/su3_spinor_mshift.hip) with the one-flavour
rational pseudofermion on it (``rational.py``), the propagator and the pseudofermions; ``pion_correlator`` / ``effective_mass``; and ``draw``, the
random-draw rule of the fermion layer."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from l2hmc import DEVICE
from l2hmc import _ops as ops

Tensor = torch.Tensor


def _log_positive(arg: Tensor) -> Tensor:
    """ln(arg) where arg is positive and finite, NaN elsewhere"""
    ok = (arg > 0) & torch.isfinite(arg)
    return torch.where(ok, torch.log(torch.where(ok, arg, torch.ones_like(arg))), torch.full_like(arg, float('nan')))


def pion_correlator(S: Tensor, t_source: int = 0) -> Tensor:
    """C(t) = sum_x sum_{spins, colours} |S(x, t_source + t)|^2 [nb, T] of a point-to-all propagator S[nb, T, X, Y, Z, 4,
    3, 4, 3] (`LatticeSU3.quark_propagator`), t counted from the source's time slice (periodically).  By gamma5-
    Hermiticity this is the pseudoscalar two-point function; it is positive."""
    S = torch.as_tensor(S)
    if S.dim() != 9 or tuple(S.shape[-4:]) != (4, 3, 4, 3):
        raise ValueError(f'pion_correlator: need S [nb, T, X, Y, Z, 4, 3, 4, 3], got {list(S.shape)}')
    c = (S.real ** 2 + S.imag ** 2).sum(tuple(range(2, 9)))
    return torch.roll(c, -int(t_source), 1)


def effective_mass(C: Tensor) -> Tensor:
    """m_eff(t) = ln[C(t) / C(t+1)] from C[..., T]: [..., T-1].  NaN where the ratio is not positive; never raises."""
    C = torch.as_tensor(C)
    return _log_positive(C[..., :-1] / C[..., 1:])


def draw(shape, generator: Optional[torch.Generator], device: torch.device, uniform: bool = False) -> Tensor:
    """float64 normals (or uniforms on [0, 1)) on `device`: drawn there with no generator or one of that device's type,
    else where the generator lives and moved -- a CPU generator gives the same numbers on any machine"""
    fn = torch.rand if uniform else torch.randn
    if generator is None or generator.device.type == device.type:
        return fn(shape, dtype=torch.float64, device=device, generator=generator)
    return fn(shape, dtype=torch.float64, generator=generator).to(device)


def ratio(live: Tensor, num: Tensor, den: Tensor) -> Tensor:
    """the CG's alpha and beta: num / den of the live systems with den > 0, 0 of the others, which freezes those"""
    ok = live & (den > 0)
    return torch.where(ok, num / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(den)).contiguous()


def _norm2(f: Tensor, other: Tensor, spare: Tensor, zero: Tensor, part: Optional[Tensor] = None, update=None) -> Tensor:
    """|f|^2 per system [nb, nrhs] by the update kernel at alpha = 0 (`zero`): it leaves spare (its x) and f (its r)
    as they are and |f|^2 in its partial sums; `other` is the p and q it reads.  `update`: the kernel wrapper, that of
    the complex128 fields unless given"""
    return ops.sum_parts((update or ops.su3_spinor_cg_update_)(spare, f, other, other, zero, part))


def _residual(r: Tensor, spare: Tensor, p: Tensor, ax: Tensor, bb: Tensor, part: Optional[Tensor] = None) -> Tensor:
    """the recomputed residual |b - A x| / sqrt(bb) per system, 0 where bb = 0: r holds b and becomes r - 1 * ax by the
    update kernel, spare and p serving as the update's other pair"""
    rr = ops.sum_parts(ops.su3_spinor_cg_update_(spare, r, p, ax, torch.ones_like(bb), part))
    return torch.sqrt(rr / torch.where(bb > 0, bb, torch.ones_like(bb)))


class _WilsonOp:
    """M on full fields [nb, nrhs, 12, V] as the operator of a `_CG`: apply(src, dst, dagger, norm) writes dst = M src
    (dagger: M^H src) and, with norm, returns the fused |dst|^2 [nb, nrhs]; `sites` is the site count of its fields."""

    def __init__(self, xn: Tensor, k: float, L, antiperiodic_t, like: Tensor):
        self.sites = like.shape[3]
        part = torch.empty((*like.shape[:2], ops.su3_wilson_norm_parts(L)), dtype=torch.float64, device=like.device)

        def apply(src, dst, dagger, norm=True):
            ops.su3_wilson_apply_n(xn, src, k, L, dagger, antiperiodic_t, out=dst, norm=part if norm else False)
            return ops.sum_parts(part) if norm else None
        self.apply = apply


class _SchurOp:
    """Mhat = 1 - kappa^2 H_eo H_oe on even half fields [nb, nrhs, 12, V/2] as the operator of a `_CG`: two
    `su3_wilson_hop_eo_n` through one scratch odd half field, the fused norm from the second.  The dagger bit on both
    hops gives Mhat^H.  dst must not be src."""

    def __init__(self, xn: Tensor, k: float, L, antiperiodic_t, like: Tensor):
        self.sites = like.shape[3]
        part = torch.empty((*like.shape[:2], -(-self.sites // 256)), dtype=torch.float64, device=like.device)
        odd = torch.empty_like(like)

        def apply(src, dst, dagger, norm=True):
            ops.su3_wilson_hop_eo_n(xn, src, L, 1, dagger, antiperiodic_t, out=odd)
            ops.su3_wilson_hop_eo_n(xn, odd, L, 0, dagger, antiperiodic_t, a=-k * k, aux=src, b=1.0, out=dst,
                                    norm=part if norm else False)
            return ops.sum_parts(part) if norm else None
        self.apply = apply


class _SchurOpF32:
    """`_SchurOp` in single precision: Mhat on complex64 even half fields, two `su3_wilson_hop_eo_f32_n` on the fp32,
    parity-ordered link copy x32 -- made here from xn, once per solve, unless given.  The fused norm stays float64."""

    def __init__(self, xn: Optional[Tensor], k: float, L, antiperiodic_t, like: Tensor, x32: Optional[Tensor] = None):
        self.sites = like.shape[3]
        self.x32 = x32 = ops.su3_links_demote_eo_n(xn, L) if x32 is None else x32
        part = torch.empty((*like.shape[:2], -(-self.sites // 256)), dtype=torch.float64, device=like.device)
        odd = torch.empty_like(like)

        def apply(src, dst, dagger, norm=True):
            ops.su3_wilson_hop_eo_f32_n(x32, src, L, 1, dagger, antiperiodic_t, out=odd)
            ops.su3_wilson_hop_eo_f32_n(x32, odd, L, 0, dagger, antiperiodic_t, a=-k * k, aux=src, b=1.0, out=dst,
                                        norm=part if norm else False)
            return ops.sum_parts(part) if norm else None
        self.apply = apply


class CloverTerm:
    """The clover term of one configuration, as `clover_term(_n)` builds it: `a` and `ainv`, the block fields [nb, 2
    parity, 2 chirality, 36, V/2] float64 of A and A^-1 (layout: include/l2q.h); `min_pivot` [nb], the smallest pivot of the
    L D L^H of any block of the chain (<= 0: A is not positive definite there and `ainv` is not usable); `logdet` [nb, 2],
    log det A per parity (NaN where a pivot is not positive); and the `kappa` and `c_sw` it was built with."""

    def __init__(self, a: Tensor, ainv: Tensor, min_pivot: Tensor, logdet: Tensor, kappa: float, c_sw: float):
        self.a, self.ainv, self.min_pivot, self.logdet, self.kappa, self.c_sw = a, ainv, min_pivot, logdet, kappa, c_sw


class _CloverSchurOp:
    """Mhat = A_ee - kappa^2 H_eo A_oo^-1 H_oe on even half fields as the operator of a `_CG`: two
    `su3_wilson_clover_hop_eo_n` through one scratch odd half field -- A_oo^-1 on the result of the first (cmode 2), A_ee
    on the aux of the second (cmode 1) -- the fused norm from the second.  A is Hermitian and commutes with gamma5, so
    the dagger bit on both hops gives Mhat^H.  dst must not be src."""

    def __init__(self, xn: Tensor, k: float, L, antiperiodic_t, like: Tensor, cl: CloverTerm):
        self.sites = like.shape[3]
        part = torch.empty((*like.shape[:2], -(-self.sites // 256)), dtype=torch.float64, device=like.device)
        odd = torch.empty_like(like)

        def apply(src, dst, dagger, norm=True):
            ops.su3_wilson_clover_hop_eo_n(xn, src, L, 1, cl.ainv, 2, dagger, antiperiodic_t, out=odd)
            ops.su3_wilson_clover_hop_eo_n(xn, odd, L, 0, cl.a, 1, dagger, antiperiodic_t, a=-k * k, aux=src, b=1.0,
                                           out=dst, norm=part if norm else False)
            return ops.sum_parts(part) if norm else None
        self.apply = apply


class _CG:
    """What the solvers share: a batched CG from x = 0 for every system (chain, rhs) of the field b [nb, nrhs, 12,
    sites] at once, on the operator `op` (`_WilsonOp` on full fields, `_SchurOp` on even half fields: its apply(src,
    dst, dagger, norm) and the site count of its fields).  It owns the argument checks, the workspace (x, r, q, z, the
    partial sums rpart of the updates), the loop with its look at |r|^2 <= tol^2 bb every check_every iterations (and
    after the last), and the recomputed residual; bb, the reference norm of the stopping test, is |b|^2 unless given (the
    even-odd solve gives |b|^2 of the full right-hand side).  `cgnr` and `normal` are the two loop bodies.  On complex64
    fields (the inner solves of `_MixedSolve`, on a `_SchurOpF32`) the same loops run on the fp32 update and xpay."""

    @staticmethod
    def check_args(what: str, tol, max_iter, check_every) -> None:
        if not (float(tol) > 0.0) or isinstance(max_iter, bool) or int(max_iter) != max_iter or int(max_iter) < 0 \
                or isinstance(check_every, bool) or int(check_every) != check_every or int(check_every) < 1:
            raise ValueError(f'LatticeSU3.{what}: need tol > 0, an integer max_iter >= 0 and check_every >= 1, got '
                             f'{tol!r}, {max_iter!r}, {check_every!r}')

    def __init__(self, what: str, b: Tensor, single: bool, op, tol, max_iter, check_every, bb: Optional[Tensor] = None):
        self.check_args(what, tol, max_iter, check_every)
        assert b.shape[3] == op.sites
        self.b, self.single, self.apply = b, single, op.apply
        self.tol2, self.max_iter, self.check_every = float(tol) ** 2, int(max_iter), int(check_every)
        f32 = b.dtype == torch.complex64
        self.update = ops.su3_spinor_cg_update_f32_ if f32 else ops.su3_spinor_cg_update_
        self.xpay = ops.su3_spinor_xpay_f32_ if f32 else ops.su3_spinor_xpay_
        self.x, self.r, self.q, self.z = torch.zeros_like(b), b.clone(), torch.empty_like(b), torch.empty_like(b)
        self.rpart = torch.empty((*b.shape[:2], -(-op.sites // 256)), dtype=torch.float64, device=b.device)
        self.zero = torch.zeros(b.shape[:2], dtype=torch.float64, device=b.device)
        self.bb0 = _norm2(self.r, b, self.x, self.zero, self.rpart, self.update)                          # |b|^2
        self.bb = self.bb0 if bb is None else bb

    def cgnr(self, final: bool = True) -> None:
        """A x = b by CG on A^H A with the true residual r = b - A x carried along; leaves x, and (final) A x in q"""
        psi, r, q, z, apply = self.x, self.r, self.q, self.z, self.apply
        zz = apply(r, z, True)
        self.p = p = z.clone()
        for active in self.iterations(lambda: ops.sum_parts(self.rpart)):      # |r|^2 is summed at a check only
            qq = apply(p, q, False)
            self.update(psi, r, p, q, ratio(active, zz, qq), self.rpart)
            zn = apply(r, z, True)
            self.xpay(p, z, ratio(active, zn, zz))
            zz = zn
        if final:
            apply(psi, q, False)

    def normal(self, final: bool = True) -> Optional[tuple[Tensor, Tensor]]:
        """A^H A X = b by CG: (Y = A X, |Y|^2 from the fused norm); leaves X in x and A^H A X in z.  Without final the
        loop only: X in x, nothing returned"""
        X, r, q, z, apply = self.x, self.r, self.q, self.z, self.apply
        self.p = p = self.b.clone()
        rr = self.bb0
        for active in self.iterations(lambda: rr):                             # |r|^2 is carried from every update
            qq = apply(p, q, False)
            apply(q, z, True, norm=False)
            rn = ops.sum_parts(self.update(X, r, p, z, ratio(active, rr, qq), self.rpart))
            self.xpay(p, r, ratio(active, rn, rr))
            rr = rn
        if not final:
            return None
        Y = torch.empty_like(X)
        action = apply(X, Y, False)
        apply(Y, z, True, norm=False)
        return Y, action

    def multishift(self, shifts: Tensor, freeze: bool = True) -> Tensor:
        """(A + sigma_k) x_k = b for A = op^H op and every shift sigma_k >= 0 of `shifts` [ns] at once, by multi-shift
        CG (Jegerlehner, hep-lat/9612014) from x_k = 0: the base system is the unshifted one, carried through p, r,
        alpha and beta (it has no x of its own); every shifted residual is zeta_k r.  Per iteration the two applies of
        `normal`, the residual step `l2q_su3_spinor_axmy_norm`, the zeta, a, b recurrences as [nb, nrhs, ns] tensor ops
        on the device, and the fused `l2q_su3_spinor_mshift_update`.  A system leaves at a check with |r|^2 <= tol^2 bb;
        at a check (freeze) a single shift with zeta_k^2 |r|^2 <= tol^2 bb has its `live` cleared and is frozen from then
        on.  Returns X [nb, nrhs, ns, 12, sites]; leaves `shift_iters` [nb, nrhs, ns], the check at which a shift froze
        (or its system left; max_iter if never)."""
        b, r, q, z, apply = self.b, self.r, self.q, self.z, self.apply
        nb, nrhs, ns = b.shape[0], b.shape[1], shifts.numel()
        sig = shifts.to(torch.float64).reshape(1, 1, ns)
        X = torch.zeros((nb, nrhs, ns, *b.shape[2:]), dtype=b.dtype, device=b.device)
        P = b[:, :, None].repeat(1, 1, ns, 1, 1)                     # a copy also at ns = 1
        self.p = p = b.clone()
        one = torch.ones((nb, nrhs, ns), dtype=torch.float64, device=b.device)
        zeta, zeta_old = one, one
        alpha_old, beta_old = torch.ones_like(self.zero), self.zero
        slive = torch.ones((nb, nrhs, ns), dtype=torch.bool, device=b.device)
        self.shift_iters = torch.full((nb, nrhs, ns), self.max_iter, dtype=torch.int64, device=b.device)
        state = {'rr': self.bb0, 'it': 0}

        def rnorm():                       # called once per check, before the systems that converged leave
            nonlocal slive
            bound = (self.tol2 * self.bb)[..., None]
            done = slive & self.active[..., None] & ((zeta * zeta * state['rr'][..., None] <= bound) if freeze
                                                     else (state['rr'] <= self.tol2 * self.bb)[..., None])
            self.shift_iters = torch.where(done, state['it'], self.shift_iters)
            slive = slive & ~done
            return state['rr']
        for active in self.iterations(rnorm):
            rr = state['rr']
            qq = apply(p, q, False)
            apply(q, z, True, norm=False)
            alpha = ratio(active, rr, qq)
            rn = ops.sum_parts(ops.su3_spinor_axmy_norm_(r, z, alpha, self.rpart))
            beta = ratio(active, rn, rr)
            al, bt, alo, bto = alpha[..., None], beta[..., None], alpha_old[..., None], beta_old[..., None]
            den = al * bto * (zeta_old - zeta) + zeta_old * alo * (1.0 + sig * al)
            lv = slive & (al > 0) & (den != 0)
            zn = torch.where(lv, zeta * zeta_old * alo / torch.where(lv, den, one), zeta)
            rat = torch.where(lv, zn / torch.where(lv, zeta, one), torch.zeros_like(one))
            ops.su3_spinor_mshift_update_(X, P, p, r, (al * rat).contiguous(), (bt * rat * rat).contiguous(),
                                          zn.contiguous(), beta, lv.to(torch.int32).contiguous())
            zeta_old, zeta = torch.where(lv, zeta, zeta_old), zn
            moved = alpha > 0
            alpha_old, beta_old = torch.where(moved, alpha, alpha_old), torch.where(moved, beta, beta_old)
            state['rr'], state['it'] = rn, state['it'] + 1
        self.shift_iters = torch.where(self.bb[..., None] <= self.tol2 * self.bb[..., None], 0, self.shift_iters)
        return X

    def iterations(self, rnorm):
        """`active` [nb, nrhs] once per iteration, for `ratio`.  At a check a system with rnorm() <= tol^2 |b|^2 leaves
        it and is frozen from then on, so its bits do not depend on the batch; `iters` is that check, max_iter if never."""
        self.active = ~(self.bb <= self.tol2 * self.bb)
        self.iters = torch.where(self.active, self.max_iter, 0)
        it = 0
        while it < self.max_iter and bool(self.active.any()):
            for _ in range(min(self.check_every, self.max_iter - it)):
                yield self.active
                it += 1
            now = self.active & (rnorm() <= self.tol2 * self.bb)
            self.iters = torch.where(now, it, self.iters)
            self.active = self.active & ~now

    def residual(self, spare: Tensor, p: Tensor, ax: Tensor) -> Tensor:
        """after the loop: the residual recomputed as r = b - 1 * ax from ax = A x in a scratch field, spare and p
        serving as the update's other pair"""
        self.r.copy_(self.b)
        return _residual(self.r, spare, p, ax, self.bb, self.rpart)

    def info(self, res: Tensor) -> dict:
        """the info every solver returns, `res` its recomputed residual; never raises on non-convergence"""
        return {'iters': self.iters, 'converged': ~self.active, 'residual': res}


# the mixed-precision solves: defaults and the margin of the relaxed inner target
MIXED_INNER_TOL = 1e-4       # chosen from the iteration and timing tables of profiles/su3_wilson_mixed.md
MIXED_MAX_INNER = 500
MIXED_MAX_OUTER = 30
MIXED_SAFETY = 0.5           # the last cycle aims at half of what the outer test still needs, so that the rounding of
                             # the fp32 correction (relative ~1e-7 of |r|) does not cost one more cycle


class _MixedSolve:
    """Defect correction on the even-odd Schur complement (Mhat: `form` 'cgnr', Mhat^H Mhat: 'normal'): the outer loop
    in fp64 on `op64` (a `_SchurOp`) recomputes the true residual r = b - A x, tests |r|^2 <= tol^2 bb per system,
    hands r / |r| of the live systems to an inner fp32 `_CG` from zero on `op32` (a `_SchurOpF32`) and adds x += |r| e.
    A system found converged gets the scale 0 and is frozen from then on: its inner right-hand side is zero, which the
    inner `_CG` leaves alone, and `su3_spinor_promote_axpy_` does not touch it, so a system's bits do not depend on the
    batch (as long as no system of the batch runs into max_iter: the budget left to a cycle is that of the system that
    has spent most).  The inner target per system is inner_tol relaxed to MIXED_SAFETY * tol sqrt(bb) / |r|, handed to
    the inner `_CG` through its bb argument (its test is |r_in|^2 <= inner_tol^2 bb_in, bb_in = (target / inner_tol)^2).
    Stops when nothing is live, when the summed inner iterations reach max_iter, or after max_outer cycles; never raises
    on non-convergence."""

    @staticmethod
    def check_args(what: str, inner_tol, max_inner, max_outer) -> None:
        ok = isinstance(inner_tol, (int, float, np.floating)) and not isinstance(inner_tol, bool) and 0.0 < inner_tol < 1.0
        for v, lo in ((max_inner, 1), (max_outer, 0)):
            ok = ok and not isinstance(v, bool) and isinstance(v, (int, np.integer)) and v >= lo
        if not ok:
            raise ValueError(f'LatticeSU3.{what}: need 0 < inner_tol < 1, an integer max_inner >= 1 and max_outer >= 0, '
                             f'got {inner_tol!r}, {max_inner!r}, {max_outer!r}')

    def __init__(self, what: str, form: str, b: Tensor, op64, op32, tol, max_iter, check_every, inner_tol, max_inner,
                 max_outer, bb: Optional[Tensor] = None):
        _CG.check_args(what, tol, max_iter, check_every)
        self.check_args(what, inner_tol, max_inner, max_outer)
        assert form in ('cgnr', 'normal') and b.shape[3] == op64.sites == op32.sites
        tol2, inner_tol = float(tol) ** 2, float(inner_tol)
        apply = op64.apply
        shape = b.shape[:2]
        self.x = x = torch.zeros_like(b)
        r, ax, spare = b.clone(), torch.empty_like(b), torch.zeros_like(b)
        mid = torch.empty_like(b) if form == 'normal' else None
        part = torch.empty((*shape, -(-op64.sites // 256)), dtype=torch.float64, device=b.device)
        zero = torch.zeros(shape, dtype=torch.float64, device=b.device)
        one = torch.ones_like(zero)
        r32 = torch.empty(b.shape, dtype=torch.complex64, device=b.device)
        rr = _norm2(r, b, spare, zero, part)                                                # |b|^2
        self.bb = bb = rr if bb is None else bb
        live = ~(bb <= tol2 * bb)
        self.iters = torch.zeros(shape, dtype=torch.int64, device=b.device)
        self.outer = torch.zeros_like(self.iters)
        cycles = 0
        while True:
            live = live & ~(rr <= tol2 * bb)
            spent = int(torch.where(live, self.iters, 0).max())
            if not bool(live.any()) or cycles >= int(max_outer) or spent >= int(max_iter):
                break
            rn = torch.sqrt(torch.where(live, rr, one))
            ops.su3_spinor_demote(r, torch.where(live, 1.0 / rn, zero).contiguous(), out=r32)
            target = torch.clamp(MIXED_SAFETY * float(tol) * torch.sqrt(bb) / rn, min=inner_tol)
            inner = _CG(what, r32, False, op32, inner_tol, min(int(max_inner), int(max_iter) - spent), check_every,
                        bb=torch.where(live, (target / inner_tol) ** 2, zero))
            inner.cgnr(final=False) if form == 'cgnr' else inner.normal(final=False)
            ops.su3_spinor_promote_axpy_(x, inner.x, torch.where(live, rn, zero).contiguous())
            self.iters = self.iters + torch.where(live, inner.iters, 0)
            self.outer = self.outer + live.to(torch.int64)
            cycles += 1
            if form == 'cgnr':                                                              # r = b - Mhat x
                apply(x, ax, False, norm=False)
            else:                                                                           # r = b - Mhat^H Mhat x
                apply(x, mid, False, norm=False)
                apply(mid, ax, True, norm=False)
            r.copy_(b)
            rr = ops.sum_parts(ops.su3_spinor_cg_update_(spare, r, ax, ax, one, part))
        self.live = live
        self.residual = torch.sqrt(rr / torch.where(bb > 0, bb, one))

    def info(self) -> dict:
        return {'iters': self.iters, 'outer': self.outer, 'converged': ~self.live, 'residual': self.residual}


class WilsonFermions:
    """The Wilson-fermion methods of ``LatticeSU3``, which inherits them.  Of the host class they use only
    ``_lattice_shape``, ``volume``, ``pack``, ``unpack`` and ``_no_grad``."""

    @staticmethod
    def gamma_matrices() -> Tensor:
        """[5, 4, 4] complex128 (CPU): gamma_0 (T), gamma_1, gamma_2, gamma_3 (x, y, z) and gamma5 = g0 g1 g2 g3 =
        diag(-1, -1, 1, 1), the Hermitian chiral basis of csrc/su3_wilson.hip: gamma_mu = [[0, B_mu], [B_mu^H, 0]] with
        B_0 = 1, B_k = -i sigma_k."""
        sig = torch.tensor([[[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]], dtype=torch.complex128)
        blocks = [torch.eye(2, dtype=torch.complex128)] + [-1j * s for s in sig]
        gam = torch.zeros((5, 4, 4), dtype=torch.complex128)
        for mu, b in enumerate(blocks):
            gam[mu, :2, 2:] = b
            gam[mu, 2:, :2] = b.conj().T
        gam[4] = gam[0] @ gam[1] @ gam[2] @ gam[3]
        return gam

    def _wilson_checks(self, what: str, kappa, *tensors) -> float:
        for t in tensors:
            self._no_grad(t, what)
        try:
            k = float(kappa)
        except (TypeError, ValueError):
            k = float('nan')
        if not np.isfinite(k):
            raise ValueError(f'LatticeSU3.{what}: kappa must be a finite number, got {kappa!r}')
        return k

    def _spinor_native(self, what: str, xn: Tensor, psin: Tensor, half: bool = False) -> tuple[Tensor, bool]:
        """psin as [nb, nrhs, 12, V] (half: a half field, V/2 sites) and whether it came without the nrhs axis"""
        sites, kind, v = (self.volume // 2, 'half', 'V/2') if half else (self.volume, 'spinor', 'V')
        single = psin.dim() == 3
        p = psin[:, None] if single else psin
        if p.dim() != 4 or tuple(p.shape[2:]) != (12, sites) or p.shape[0] != xn.shape[0]:
            raise ValueError(f'LatticeSU3.{what}: need a native {kind} field [nb, nrhs, 12, {v}] or [nb, 12, {v}] with '
                             f'nb = {xn.shape[0]}, {v} = {sites}, got {list(psin.shape)}')
        return p.to(torch.complex128).contiguous(), single

    def _spinor_reference(self, what: str, x: Tensor, psi: Tensor) -> tuple[Tensor, bool]:
        single = psi.dim() == 7
        p = psi[:, None] if single else psi
        if p.dim() != 8 or tuple(p.shape[2:]) != (*self._lattice_shape, 4, 3) or p.shape[0] != x.shape[0]:
            raise ValueError(f'LatticeSU3.{what}: need a spinor field [nb, nrhs, T, X, Y, Z, 4, 3] or one without the nrhs '
                             f'axis on this lattice, got {list(psi.shape)}')
        return ops.su3_spinor_pack(p.to(DEVICE)), single

    def wilson_dirac_n(self, xn: Tensor, psin: Tensor, kappa: float, dagger: bool = False,
                       antiperiodic_t: bool = True) -> Tensor:
        """M psi = psi - kappa H psi (dagger: M^H psi = gamma5 M gamma5 psi) of a native spinor field [nb, nrhs, 12, V]
        (or [nb, 12, V]) on the native links xn, thin or smeared,
            H psi(x) = sum_mu [(1 - gamma_mu) U_mu(x) psi(x+mu) + (1 + gamma_mu) U_mu(x-mu)^H psi(x-mu)],
        periodic except that with antiperiodic_t every hop across the t = T-1 -> 0 seam takes a factor -1.  One
        `l2q_su3_wilson_apply`; a new field, nothing is written.  Any extents; any gauge action; no autograd."""
        k = self._wilson_checks('wilson_dirac', kappa, xn, psin)
        p, single = self._spinor_native('wilson_dirac', xn, psin)
        out = ops.su3_wilson_apply_n(xn, p, k, self._lattice_shape, dagger, antiperiodic_t)
        return out[:, 0] if single else out

    def wilson_dirac(self, x: Tensor, psi: Tensor, kappa: float, dagger: bool = False,
                     antiperiodic_t: bool = True) -> Tensor:
        """`wilson_dirac_n` in the reference layout: psi[nb, nrhs, T, X, Y, Z, 4, 3] (spin, then colour), with or
        without the nrhs axis, which the result then lacks too."""
        k = self._wilson_checks('wilson_dirac', kappa, x, psi)
        p, single = self._spinor_reference('wilson_dirac', x, psi)
        out = ops.su3_spinor_unpack(ops.su3_wilson_apply_n(self.pack(x), p, k, self._lattice_shape, dagger,
                                                           antiperiodic_t), self._lattice_shape)
        return out[:, 0] if single else out

    def wilson_solve_n(self, xn: Tensor, bn: Tensor, kappa: float, tol: float = 1e-10, max_iter: int = 1000,
                       check_every: int = 10, antiperiodic_t: bool = True) -> tuple[Tensor, dict]:
        """M psi = b for every system (chain, rhs) of the native field bn at once, by CG on M^H M (CGNR) from psi = 0,
        with the true residual r = b - M psi carried along: per iteration two `l2q_su3_wilson_apply` (q = M p and
        z = M^H r, each with its fused norm), one `l2q_su3_spinor_cg_update` and one `l2q_su3_spinor_xpay`;
        alpha = |z|^2 / |M p|^2 and beta are formed per system on the device.  The host looks at |r|^2 <= tol^2 |b|^2
        every check_every iterations (and after the last); a system found converged takes alpha = beta = 0 from then
        on, so it no longer changes while the others go on, and a system's solution is the same bits whatever else is in
        the batch.  Returns (psi, info): info['iters'] (the check at which a system was found converged, max_iter if
        never), info['residual'] (|b - M psi| / |b| recomputed after the loop, 0 for b = 0), info['converged'], each
        [nb, nrhs].  Never raises on non-convergence; b = 0 gives psi = 0.  Workspace: six spinor fields.
        `wilson_solve_eo_n` is the same solve through the even-odd Schur complement."""
        k = self._wilson_checks('wilson_solve', kappa, xn, bn)
        _CG.check_args('wilson_solve', tol, max_iter, check_every)
        b, single = self._spinor_native('wilson_solve', xn, bn)
        op = _WilsonOp(xn, k, self._lattice_shape, antiperiodic_t, b)
        cg = _CG('wilson_solve', b, single, op, tol, max_iter, check_every)
        cg.cgnr()
        return (cg.x[:, 0] if single else cg.x), cg.info(cg.residual(cg.z, cg.p, cg.q))

    def wilson_solve_eo_n(self, xn: Tensor, bn: Tensor, kappa: float, tol: float = 1e-10, max_iter: int = 1000,
                          check_every: int = 10, antiperiodic_t: bool = True) -> tuple[Tensor, dict]:
        """`wilson_solve_n` with even-odd preconditioning (even extents): the same system M psi = b through its Schur
        complement on the even sites -- split b, form bhat_e = b_e + kappa H_eo b_o, the same CGNR loop on Mhat = 1 -
        kappa^2 H_eo H_oe from zero with the same stopping test |rhat|^2 <= tol^2 |b|^2 (|b|^2 of the full right-hand
        side: with psi_o reconstructed, b - M psi is rhat on the even sites and zero on the odd ones, so tol means what
        it means there), psi_o = b_o + kappa H_oe psi_e, merge.  Same arguments, same freezing, same independence of a
        system's bits from the batch, same info keys; info['residual'] is the full |b - M psi| / |b| recomputed with one
        `l2q_su3_wilson_apply` after the reconstruction.  b = 0 gives psi = 0.  `quark_propagator(_n)` takes it with
        even_odd=True."""
        k = self._wilson_checks('wilson_solve_eo', kappa, xn, bn)
        _CG.check_args('wilson_solve_eo', tol, max_iter, check_every)
        L = self._eo_lattice('wilson_solve_eo')
        b, single = self._spinor_native('wilson_solve_eo', xn, bn)
        be, bo = ops.su3_spinor_split_eo(b, L)
        zero = torch.zeros(b.shape[:2], dtype=torch.float64, device=b.device)
        spare = torch.zeros_like(be)
        bb = _norm2(be, bo, spare, zero) + _norm2(bo, be, spare, zero)                 # |b_e|^2 + |b_o|^2
        bhat = ops.su3_wilson_hop_eo_n(xn, bo, L, 0, False, antiperiodic_t, a=k, aux=be, b=1.0)
        cg = _CG('wilson_solve_eo', bhat, single, _SchurOp(xn, k, L, antiperiodic_t, bhat), tol, max_iter, check_every, bb=bb)
        cg.cgnr()
        psio = ops.su3_wilson_hop_eo_n(xn, cg.x, L, 1, False, antiperiodic_t, a=k, aux=bo, b=1.0)
        psi = ops.su3_spinor_merge_eo(cg.x, psio, L)
        mpsi = ops.su3_wilson_apply_n(xn, psi, k, L, False, antiperiodic_t)             # the residual of the full system
        return (psi[:, 0] if single else psi), cg.info(_residual(b.clone(), torch.zeros_like(b), mpsi, mpsi, bb))

    def wilson_solve(self, x: Tensor, b: Tensor, kappa: float, tol: float = 1e-10, max_iter: int = 1000,
                     check_every: int = 10, antiperiodic_t: bool = True) -> tuple[Tensor, dict]:
        """`wilson_solve_n` in the reference layout; x may be thin or smeared links, e.g.
        `wilson_solve(lat.hyp_smear(x), b, kappa)`."""
        self._wilson_checks('wilson_solve', kappa, x, b)
        bn, single = self._spinor_reference('wilson_solve', x, b)
        psin, info = self.wilson_solve_n(self.pack(x), bn, kappa, tol, max_iter, check_every, antiperiodic_t)
        psi = ops.su3_spinor_unpack(psin, self._lattice_shape)
        return (psi[:, 0] if single else psi), info

    def wilson_solve_eo(self, x: Tensor, b: Tensor, kappa: float, tol: float = 1e-10, max_iter: int = 1000,
                        check_every: int = 10, antiperiodic_t: bool = True) -> tuple[Tensor, dict]:
        """`wilson_solve_eo_n` in the reference layout"""
        self._wilson_checks('wilson_solve_eo', kappa, x, b)
        self._eo_lattice('wilson_solve_eo')
        bn, single = self._spinor_reference('wilson_solve_eo', x, b)
        psin, info = self.wilson_solve_eo_n(self.pack(x), bn, kappa, tol, max_iter, check_every, antiperiodic_t)
        psi = ops.su3_spinor_unpack(psin, self._lattice_shape)
        return (psi[:, 0] if single else psi), info

    # ------------------------------------------------------------ mixed-precision even-odd solves (defect correction)
    @staticmethod
    def _pop_mixed(what: str, solve_kwargs: dict, even_odd: bool) -> Optional[dict]:
        """the mixed-precision keywords popped from solve_kwargs: None without mixed=True, else the dict of inner_tol,
        max_inner, max_outer that were given.  ValueError: mixed without even_odd, or the others without mixed."""
        mixed = bool(solve_kwargs.pop('mixed', False))
        given = {k: solve_kwargs.pop(k) for k in ('inner_tol', 'max_inner', 'max_outer') if k in solve_kwargs}
        if mixed and not even_odd:
            raise ValueError(f'LatticeSU3.{what}: mixed=True needs even_odd=True: the mixed-precision solves are those '
                             f'of the even-odd Schur complement')
        if given and not mixed:
            raise ValueError(f'LatticeSU3.{what}: {sorted(given)} are keywords of the mixed-precision solves: pass '
                             f'mixed=True (with even_odd=True)')
        return given if mixed else None

    def wilson_solve_eo_mixed_n(self, xn: Tensor, bn: Tensor, kappa: float, tol: float = 1e-10, max_iter: int = 1000,
                                check_every: int = 10, antiperiodic_t: bool = True, inner_tol: float = MIXED_INNER_TOL,
                                max_inner: int = MIXED_MAX_INNER, max_outer: int = MIXED_MAX_OUTER) -> tuple[Tensor, dict]:
        """`wilson_solve_eo_n` in mixed precision, by defect correction: the outer loop recomputes the true residual
        rhat = bhat - Mhat psi_e with the fp64 kernels and stops on the test of `wilson_solve_eo_n`, |rhat|^2 <= tol^2
        |b|^2 (|b|^2 of the full right-hand side), so the answer meets the same double-precision test; each cycle solves
        Mhat e = rhat / |rhat| from zero by the same CGNR loop on the fp32 kernels (csrc/su3_wilson_f32.hip, on an fp32,
        parity-ordered copy of the links made once per solve) to the relative target max(inner_tol, 0.5 tol |b| /
        |rhat|), at most max_inner iterations, and adds psi_e += |rhat| e in fp64.  It stops when every system has
        converged, when a system's summed inner iterations reach max_iter, or after max_outer cycles; never raises on
        non-convergence; b = 0 gives psi = 0.  A converged system is frozen: its bits do not depend on the batch.
        info, each [nb, nrhs]: 'iters' (the summed inner iterations), 'outer' (cycles), 'converged', 'residual' (the
        last |rhat| / |b|, recomputed in fp64: with psi_o reconstructed it is |b - M psi| / |b|)."""
        k = self._wilson_checks('wilson_solve_eo_mixed', kappa, xn, bn)
        _CG.check_args('wilson_solve_eo_mixed', tol, max_iter, check_every)
        _MixedSolve.check_args('wilson_solve_eo_mixed', inner_tol, max_inner, max_outer)
        L = self._eo_lattice('wilson_solve_eo_mixed')
        b, single = self._spinor_native('wilson_solve_eo_mixed', xn, bn)
        be, bo = ops.su3_spinor_split_eo(b, L)
        zero = torch.zeros(b.shape[:2], dtype=torch.float64, device=b.device)
        spare = torch.zeros_like(be)
        bb = _norm2(be, bo, spare, zero) + _norm2(bo, be, spare, zero)                 # |b_e|^2 + |b_o|^2
        bhat = ops.su3_wilson_hop_eo_n(xn, bo, L, 0, False, antiperiodic_t, a=k, aux=be, b=1.0)
        like32 = torch.empty(bhat.shape, dtype=torch.complex64, device=bhat.device)
        ms = _MixedSolve('wilson_solve_eo_mixed', 'cgnr', bhat, _SchurOp(xn, k, L, antiperiodic_t, bhat),
                         _SchurOpF32(xn, k, L, antiperiodic_t, like32), tol, max_iter, check_every, inner_tol, max_inner,
                         max_outer, bb=bb)
        psio = ops.su3_wilson_hop_eo_n(xn, ms.x, L, 1, False, antiperiodic_t, a=k, aux=bo, b=1.0)
        psi = ops.su3_spinor_merge_eo(ms.x, psio, L)
        return (psi[:, 0] if single else psi), ms.info()

    def wilson_solve_eo_mixed(self, x: Tensor, b: Tensor, kappa: float, tol: float = 1e-10, max_iter: int = 1000,
                              check_every: int = 10, antiperiodic_t: bool = True, inner_tol: float = MIXED_INNER_TOL,
                              max_inner: int = MIXED_MAX_INNER, max_outer: int = MIXED_MAX_OUTER) -> tuple[Tensor, dict]:
        """`wilson_solve_eo_mixed_n` in the reference layout"""
        self._wilson_checks('wilson_solve_eo_mixed', kappa, x, b)
        self._eo_lattice('wilson_solve_eo_mixed')
        bn, single = self._spinor_reference('wilson_solve_eo_mixed', x, b)
        psin, info = self.wilson_solve_eo_mixed_n(self.pack(x), bn, kappa, tol, max_iter, check_every, antiperiodic_t,
                                                  inner_tol, max_inner, max_outer)
        psi = ops.su3_spinor_unpack(psin, self._lattice_shape)
        return (psi[:, 0] if single else psi), info

    def wilson_solve_schur_normal_mixed_n(self, xn: Tensor, phi_e: Tensor, kappa: float, tol: float = 1e-10,
                                          max_iter: int = 1000, check_every: int = 10, antiperiodic_t: bool = True,
                                          inner_tol: float = MIXED_INNER_TOL, max_inner: int = MIXED_MAX_INNER,
                                          max_outer: int = MIXED_MAX_OUTER) -> tuple[Tensor, Tensor, dict]:
        """`wilson_solve_schur_normal_n` in mixed precision, by the defect correction of `wilson_solve_eo_mixed_n` on
        Mhat^H Mhat: the outer loop recomputes r = phi_e - Mhat^H Mhat X_e in fp64 and stops on |r|^2 <= tol^2 |phi_e|^2,
        the inner cycles are the normal-equation CG on the fp32 kernels.  After the loop Y_e = Mhat X_e and |Y_e|^2 come
        from the fp64 operator with its fused norm, as there.  Returns (X_e, Y_e, info), info as in
        `wilson_solve_eo_mixed_n` plus 'action' = |Y_e|^2."""
        k = self._pf_checks('wilson_solve_schur_normal_mixed', kappa, xn, phi_e)
        _CG.check_args('wilson_solve_schur_normal_mixed', tol, max_iter, check_every)
        _MixedSolve.check_args('wilson_solve_schur_normal_mixed', inner_tol, max_inner, max_outer)
        L = self._eo_lattice('wilson_solve_schur_normal_mixed')
        b, single = self._spinor_native('wilson_solve_schur_normal_mixed', xn, phi_e, half=True)
        op = _SchurOp(xn, k, L, antiperiodic_t, b)
        like32 = torch.empty(b.shape, dtype=torch.complex64, device=b.device)
        ms = _MixedSolve('wilson_solve_schur_normal_mixed', 'normal', b, op, _SchurOpF32(xn, k, L, antiperiodic_t, like32),
                         tol, max_iter, check_every, inner_tol, max_inner, max_outer)
        X, Y = ms.x, torch.empty_like(ms.x)
        info = {**ms.info(), 'action': op.apply(X, Y, False)}
        return (X[:, 0], Y[:, 0], info) if single else (X, Y, info)

    def quark_propagator_n(self, xn: Tensor, kappa: float, source=(0, 0, 0, 0), **solve_kwargs) -> tuple[Tensor, dict]:
        """The point-to-all propagator from the site `source` = (t, x, y, z): the twelve unit sources (spin, colour) at
        that site solved as one nrhs = 12 batch of `wilson_solve_n`.  Returns (S, info), S[nb, 12, 12, V] native:
        source component 3 spin + colour, then sink component, then site.  even_odd=True among the keywords: by
        `wilson_solve_eo_n`; with mixed=True besides (and inner_tol, max_inner, max_outer): by `wilson_solve_eo_mixed_n`.
        c_sw among the keywords (and clover=, a prebuilt `CloverTerm`): the propagator of the clover-improved operator,
        by `wilson_clover_solve_n`, which is even-odd preconditioned: not with even_odd=False or mixed=True."""
        self._wilson_checks('quark_propagator', kappa, xn)
        improved = self._pop_clover('quark_propagator', solve_kwargs)
        even_odd = bool(solve_kwargs.pop('even_odd', False))
        mixed = self._pop_mixed('quark_propagator', solve_kwargs, even_odd)
        solve = self.wilson_solve_eo_n if even_odd else self.wilson_solve_n
        if improved is not None:
            self._clover_checks('quark_propagator', kappa, improved['c_sw'])

            def solve(xn, bn, kappa, **kw):
                return self.wilson_clover_solve_n(xn, bn, kappa, **improved, **kw)
        if even_odd:
            self._eo_lattice('quark_propagator')
        if mixed is not None:
            solve_kwargs.update(mixed)
            solve = self.wilson_solve_eo_mixed_n
        L = self._lattice_shape
        try:
            src = [int(c) for c in source]
            ok = len(src) == 4 and all(int(c) == c and 0 <= int(c) < n for c, n in zip(source, L))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f'LatticeSU3.quark_propagator: source must be a site (t, x, y, z) of {list(L)}, got {source!r}')
        s = ((src[0] * L[1] + src[1]) * L[2] + src[2]) * L[3] + src[3]
        bn = torch.zeros((xn.shape[0], 12, 12, self.volume), dtype=torch.complex128, device=xn.device)
        j = torch.arange(12, device=xn.device)
        bn[:, j, j, s] = 1.0
        return solve(xn, bn, kappa, **solve_kwargs)

    def quark_propagator(self, x: Tensor, kappa: float, source=(0, 0, 0, 0), **solve_kwargs) -> tuple[Tensor, dict]:
        """`quark_propagator_n` in the reference layout: S[nb, T, X, Y, Z, 4, 3, 4, 3] (sink spin, sink colour, source
        spin, source colour), for `pion_correlator`."""
        self._wilson_checks('quark_propagator', kappa, x)
        if self._pop_mixed('quark_propagator', dict(solve_kwargs), bool(solve_kwargs.get('even_odd', False))) is not None:
            self._eo_lattice('quark_propagator')                                    # raises before the pack
        sn, info = self.quark_propagator_n(self.pack(x), kappa, source, **solve_kwargs)
        S = ops.su3_spinor_unpack(sn, self._lattice_shape).movedim(1, -1).contiguous()
        return S.reshape(*S.shape[:-1], 4, 3), info

    # ------------------------------------------------------------ the clover term: the O(a)-improved operator
    @staticmethod
    def _pop_clover(what: str, solve_kwargs: dict) -> Optional[dict]:
        """the clover keywords c_sw and clover popped from solve_kwargs: None without c_sw, else the dict of them.
        ValueError: clover= without c_sw; c_sw with even_odd=False, mixed=True or a keyword of the mixed solves."""
        c_sw, clover = solve_kwargs.pop('c_sw', None), solve_kwargs.pop('clover', None)
        if c_sw is None:
            if clover is not None:
                raise ValueError(f'LatticeSU3.{what}: clover= goes with c_sw')
            return None
        mixed = [k for k in ('inner_tol', 'max_inner', 'max_outer') if k in solve_kwargs]
        if not solve_kwargs.get('even_odd', True) or solve_kwargs.get('mixed', False) or mixed:
            raise ValueError(f'LatticeSU3.{what}: c_sw goes with neither even_odd=False nor mixed=True: the clover solve is '
                             f'the even-odd preconditioned one, in double precision')
        solve_kwargs.pop('even_odd', None)
        solve_kwargs.pop('mixed', None)
        return {'c_sw': c_sw, 'clover': clover}

    def _clover_checks(self, what: str, kappa, c_sw, *tensors) -> tuple[float, float]:
        """(kappa, c_sw) as finite floats, after the checks of `_wilson_checks`, on a lattice with even extents"""
        k = self._wilson_checks(what, kappa, *tensors)
        try:
            c = float(c_sw)
        except (TypeError, ValueError):
            c = float('nan')
        if not np.isfinite(c):
            raise ValueError(f'LatticeSU3.{what}: c_sw must be a finite number, got {c_sw!r}')
        self._eo_lattice(what)
        return k, c

    def _clover_for(self, what: str, xn: Tensor, k: float, c: float, clover: Optional[CloverTerm],
                    inverse: bool = True) -> CloverTerm:
        """the clover term of xn: built here, or the prebuilt `clover` checked against kappa, c_sw and the batch.
        inverse: A^-1 is going to be used, so every chain needs min_pivot > 0 (ValueError naming the first that has not)"""
        if clover is None:
            clover = self.clover_term_n(xn, k, c)
        else:
            shape = (xn.shape[0], 2, 2, 36, self.volume // 2)
            ok = isinstance(clover, CloverTerm) and clover.kappa == k and clover.c_sw == c \
                and tuple(clover.a.shape) == shape and tuple(clover.ainv.shape) == shape and clover.a.device == xn.device
            if not ok:
                got = (f'kappa {clover.kappa!r}, c_sw {clover.c_sw!r}, blocks {list(clover.a.shape)}'
                       if isinstance(clover, CloverTerm) else repr(type(clover)))
                raise ValueError(f'LatticeSU3.{what}: clover= must be the `clover_term` of these links at kappa {k!r}, '
                                 f'c_sw {c!r} with blocks {list(shape)}, got {got}')
        if inverse:
            mp = clover.min_pivot.detach().cpu()
            bad = torch.nonzero(~(mp > 0)).reshape(-1)
            if bad.numel():
                i = int(bad[0])
                raise ValueError(f'LatticeSU3.{what}: the clover term of chain {i} is not positive definite at kappa '
                                 f'{k!r}, c_sw {c!r} (smallest L D L^H pivot {float(mp[i])!r}): A_oo^-1 and the Schur '
                                 f'complement do not exist there')
        return clover

    def clover_term_n(self, xn: Tensor, kappa: float, c_sw: float) -> CloverTerm:
        """The clover term A(x) = 1 + kappa c_sw i sum_{mu<nu} sigma_{mu nu} (x) Fhat_{mu nu}(x) of the native links xn and
        its inverse, as a `CloverTerm`: one `l2q_su3_clover_term` and one `l2q_su3_clover_invert`, once per
        configuration.  sigma_{mu nu} = (i/2) [gamma_mu, gamma_nu]; Fhat_{mu nu} = (Q_{mu nu} - Q_{mu nu}^H) / 8 of the
        four-leaf clover sum, NOT made traceless (Sheikholeslami-Wohlert; Luescher et al.: the definition for which
        published c_sw hold).  c_sw = 0 is legal and gives A = 1.  Even extents.  Never raises on a non-positive pivot:
        `min_pivot` reports it, and the entry points that need A^-1 raise."""
        k, c = self._clover_checks('clover_term', kappa, c_sw, xn)
        L = self._lattice_shape
        a = ops.su3_clover_term_n(xn, k * c, L)
        ainv, mp, ld = ops.su3_clover_invert_n(a, L)
        return CloverTerm(a, ainv, mp.amin((1, 2)), ops.sum_parts(ld), k, c)

    def clover_term(self, x: Tensor, kappa: float, c_sw: float) -> CloverTerm:
        """`clover_term_n` of links in the reference layout"""
        self._clover_checks('clover_term', kappa, c_sw, x)
        return self.clover_term_n(self.pack(x), kappa, c_sw)

    @staticmethod
    def _clover_dirac_halves(xn: Tensor, pe: Tensor, po: Tensor, k: float, L, dagger, antiperiodic_t,
                             cl: CloverTerm) -> tuple:
        """(M_sw psi)_e and (M_sw psi)_o from the halves of psi: A_pp psi_p - kappa H_pq psi_q, one kernel per parity"""
        return tuple(ops.su3_wilson_clover_hop_eo_n(xn, src, L, p, cl.a, 1, dagger, antiperiodic_t, a=-k, aux=aux, b=1.0)
                     for p, src, aux in ((0, po, pe), (1, pe, po)))

    def wilson_clover_dirac_n(self, xn: Tensor, psin: Tensor, kappa: float, c_sw: float, dagger: bool = False,
                              antiperiodic_t: bool = True, clover: Optional[CloverTerm] = None) -> Tensor:
        """M_sw psi = A psi - kappa H psi (dagger: M_sw^H psi = gamma5 M_sw gamma5 psi) of a native spinor field [nb,
        nrhs, 12, V] (or [nb, 12, V]): the clover-improved Wilson operator, H as in `wilson_dirac_n`, A as in
        `clover_term_n` (built here unless `clover` brings it).  Split, one `l2q_su3_wilson_clover_hop_eo` per parity,
        merge; a new field.  Even extents; no autograd."""
        k, c = self._clover_checks('wilson_clover_dirac', kappa, c_sw, xn, psin)
        L = self._lattice_shape
        p, single = self._spinor_native('wilson_clover_dirac', xn, psin)
        cl = self._clover_for('wilson_clover_dirac', xn, k, c, clover, inverse=False)
        pe, po = ops.su3_spinor_split_eo(p, L)
        out = ops.su3_spinor_merge_eo(*self._clover_dirac_halves(xn, pe, po, k, L, dagger, antiperiodic_t, cl), L)
        return out[:, 0] if single else out

    def wilson_clover_dirac(self, x: Tensor, psi: Tensor, kappa: float, c_sw: float, dagger: bool = False,
                            antiperiodic_t: bool = True, clover: Optional[CloverTerm] = None) -> Tensor:
        """`wilson_clover_dirac_n` in the reference layout"""
        self._clover_checks('wilson_clover_dirac', kappa, c_sw, x, psi)
        p, single = self._spinor_reference('wilson_clover_dirac', x, psi)
        out = ops.su3_spinor_unpack(self.wilson_clover_dirac_n(self.pack(x), p, kappa, c_sw, dagger, antiperiodic_t,
                                                               clover), self._lattice_shape)
        return out[:, 0] if single else out

    def wilson_clover_schur_n(self, xn: Tensor, psi_e: Tensor, kappa: float, c_sw: float, dagger: bool = False,
                              antiperiodic_t: bool = True, clover: Optional[CloverTerm] = None) -> Tensor:
        """Mhat psi_e = A_ee psi_e - kappa^2 H_eo A_oo^-1 H_oe psi_e (dagger: Mhat^H psi_e) of an even half field [nb,
        nrhs, 12, V/2] (or [nb, 12, V/2]): the asymmetric Schur complement of M_sw on the even sites.  Two
        `l2q_su3_wilson_clover_hop_eo`; a new field.  ValueError where a chain's A is not positive definite."""
        k, c = self._clover_checks('wilson_clover_schur', kappa, c_sw, xn, psi_e)
        L = self._lattice_shape
        p, single = self._spinor_native('wilson_clover_schur', xn, psi_e, half=True)
        cl = self._clover_for('wilson_clover_schur', xn, k, c, clover)
        out = torch.empty_like(p)
        _CloverSchurOp(xn, k, L, antiperiodic_t, p, cl).apply(p, out, dagger, norm=False)
        return out[:, 0] if single else out

    def wilson_clover_schur(self, x: Tensor, psi: Tensor, kappa: float, c_sw: float, dagger: bool = False,
                            antiperiodic_t: bool = True, clover: Optional[CloverTerm] = None) -> Tensor:
        """`wilson_clover_schur_n` in the reference layout: psi is a full-shape field of which only the even sites are
        read; the odd sites of the result are zero."""
        self._clover_checks('wilson_clover_schur', kappa, c_sw, x, psi)
        pe, single = self._half_reference('wilson_clover_schur', x, psi)
        out = self._half_to_reference(self.wilson_clover_schur_n(self.pack(x), pe, kappa, c_sw, dagger, antiperiodic_t,
                                                                 clover))
        return out[:, 0] if single else out

    def wilson_clover_solve_n(self, xn: Tensor, bn: Tensor, kappa: float, c_sw: float, tol: float = 1e-10,
                              max_iter: int = 1000, check_every: int = 10, antiperiodic_t: bool = True,
                              clover: Optional[CloverTerm] = None) -> tuple[Tensor, dict]:
        """M_sw psi = b for every system (chain, rhs) of the native field bn at once, through the asymmetric even-odd
        form: bhat_e = b_e + kappa H_eo A_oo^-1 b_o, the CGNR loop of `wilson_solve_eo_n` on Mhat = A_ee - kappa^2 H_eo
        A_oo^-1 H_oe from zero, psi_o = A_oo^-1 (b_o + kappa H_oe psi_e).  With psi_o reconstructed b - M_sw psi is rhat
        on the even sites and zero on the odd ones, so the stopping test stays |rhat|^2 <= tol^2 |b|^2 with |b|^2 of the
        full right-hand side, and tol means what it means everywhere else.  Same freezing, same independence of a
        system's bits from the batch, same info keys as `wilson_solve_eo_n`; info['residual'] is the full |b - M_sw psi|
        / |b| recomputed after the reconstruction.  Never raises on non-convergence; b = 0 gives psi = 0.  `clover`: the
        `clover_term_n` of these links at this kappa and c_sw, so that several solves on one configuration build A and
        A^-1 once.  ValueError where a chain's A is not positive definite (the message names chain and pivot)."""
        what = 'wilson_clover_solve'
        k, c = self._clover_checks(what, kappa, c_sw, xn, bn)
        _CG.check_args(what, tol, max_iter, check_every)
        L = self._lattice_shape
        b, single = self._spinor_native(what, xn, bn)
        cl = self._clover_for(what, xn, k, c, clover)
        be, bo = ops.su3_spinor_split_eo(b, L)
        zero = torch.zeros(b.shape[:2], dtype=torch.float64, device=b.device)
        spare = torch.zeros_like(be)
        bb = _norm2(be, bo, spare, zero) + _norm2(bo, be, spare, zero)                 # |b_e|^2 + |b_o|^2
        bhat = ops.su3_wilson_clover_hop_eo_n(xn, ops.su3_clover_apply_n(cl.ainv, bo, L, 1), L, 0, None, 0, False,
                                              antiperiodic_t, a=k, aux=be, b=1.0)
        cg = _CG(what, bhat, single, _CloverSchurOp(xn, k, L, antiperiodic_t, bhat, cl), tol, max_iter, check_every, bb=bb)
        cg.cgnr()
        psio = ops.su3_wilson_clover_hop_eo_n(xn, cg.x, L, 1, cl.ainv, 2, False, antiperiodic_t, a=k, aux=bo, b=1.0)
        psi = ops.su3_spinor_merge_eo(cg.x, psio, L)
        mpsi = ops.su3_spinor_merge_eo(*self._clover_dirac_halves(xn, cg.x, psio, k, L, False, antiperiodic_t, cl), L)
        return (psi[:, 0] if single else psi), cg.info(_residual(b.clone(), torch.zeros_like(b), mpsi, mpsi, bb))

    def wilson_clover_solve(self, x: Tensor, b: Tensor, kappa: float, c_sw: float, tol: float = 1e-10,
                            max_iter: int = 1000, check_every: int = 10, antiperiodic_t: bool = True,
                            clover: Optional[CloverTerm] = None) -> tuple[Tensor, dict]:
        """`wilson_clover_solve_n` in the reference layout"""
        self._clover_checks('wilson_clover_solve', kappa, c_sw, x, b)
        _CG.check_args('wilson_clover_solve', tol, max_iter, check_every)
        bn, single = self._spinor_reference('wilson_clover_solve', x, b)
        psin, info = self.wilson_clover_solve_n(self.pack(x), bn, kappa, c_sw, tol, max_iter, check_every,
                                                antiperiodic_t, clover)
        psi = ops.su3_spinor_unpack(psin, self._lattice_shape)
        return (psi[:, 0] if single else psi), info

    # ------------------------------------------------------------ dynamical Wilson fermions: pseudofermions
    def _pf_checks(self, what: str, kappa, *tensors) -> float:
        for t in tensors:
            if isinstance(t, torch.Tensor) and t.requires_grad:
                raise ValueError(f'LatticeSU3.{what}: no autograd through the pseudofermion action or the even-odd '
                                 f'operator; detach the fields')
        return self._wilson_checks(what, kappa, *tensors)

    @staticmethod
    def _sum_fields(a: Tensor) -> Tensor:
        """[nb, npf] -> [nb], the fields added in their order (a chain's bits do not depend on the batch)"""
        s = a[:, 0].clone()
        for r in range(1, a.shape[1]):
            s = s + a[:, r]
        return s

    def wilson_solve_normal_n(self, xn: Tensor, phin: Tensor, kappa: float, tol: float = 1e-10, max_iter: int = 1000,
                              check_every: int = 10, antiperiodic_t: bool = True) -> tuple[Tensor, Tensor, dict]:
        """M^H M X = phi for every system (chain, field) of the native field phin at once, by CG from X = 0, and
        Y = M X: what the pseudofermion action |Y|^2 and its force need.  Per iteration q = M p with its fused norm
        (<p, M^H M p> = |M p|^2), z = M^H q, one `l2q_su3_spinor_cg_update` (X += alpha p, r -= alpha z, |r|^2 fused)
        and one `l2q_su3_spinor_xpay` (p = r + beta p); alpha = |r|^2 / |M p|^2 and beta are formed per system on the
        device.  (X from two `wilson_solve_n` would cost twice the operator applications.)  The host looks at |r|^2 <=
        tol^2 |phi|^2 every check_every iterations; a system found converged takes alpha = beta = 0 from then on, so a
        system's bits do not depend on the batch.  Never raises on non-convergence; phi = 0 gives X = 0.  Returns (X,
        Y, info): info['iters'], info['converged'], info['residual'] (|phi - M^H M X| / |phi| recomputed) and
        info['action'] (|Y|^2 from the fused norm of the last apply), each [nb, npf].  Workspace: seven spinor fields."""
        k = self._pf_checks('wilson_solve_normal', kappa, xn, phin)
        _CG.check_args('wilson_solve_normal', tol, max_iter, check_every)
        b, single = self._spinor_native('wilson_solve_normal', xn, phin)
        op = _WilsonOp(xn, k, self._lattice_shape, antiperiodic_t, b)
        return self._solve_normal(_CG('wilson_solve_normal', b, single, op, tol, max_iter, check_every))

    @staticmethod
    def _solve_normal(cg: _CG) -> tuple[Tensor, Tensor, dict]:
        Y, action = cg.normal()
        X = cg.x
        info = {**cg.info(cg.residual(cg.q, cg.p, cg.z)), 'action': action}
        return (X[:, 0], Y[:, 0], info) if cg.single else (X, Y, info)

    # ------------------------------------------------------------ even-odd preconditioning: the Schur complement
    def _eo_lattice(self, what: str):
        """the lattice, or ValueError naming it if an extent is odd"""
        return ops._even_lattice(f'LatticeSU3.{what}', self._lattice_shape)

    def _half_reference(self, what: str, x: Tensor, psi: Tensor) -> tuple[Tensor, bool]:
        """the even half field of a full-shape field in the reference layout: its odd sites are not read"""
        pn, single = self._spinor_reference(what, x, psi)
        return ops.su3_spinor_split_eo(pn, self._lattice_shape)[0].contiguous(), single

    def _half_to_reference(self, he: Tensor) -> Tensor:
        """an even half field [nb, nrhs, 12, V/2] as a full-shape field in the reference layout, zero on the odd sites"""
        L = self._lattice_shape
        return ops.su3_spinor_unpack(ops.su3_spinor_merge_eo(he, torch.zeros_like(he), L), L)

    def wilson_schur_n(self, xn: Tensor, psi_e: Tensor, kappa: float, dagger: bool = False,
                       antiperiodic_t: bool = True) -> Tensor:
        """Mhat psi_e = psi_e - kappa^2 H_eo H_oe psi_e (dagger: Mhat^H psi_e) of an even half field [nb, nrhs, 12,
        V/2] (or [nb, 12, V/2]): the Schur complement of M = 1 - kappa H on the even sites, det M = det Mhat.  Two
        `l2q_su3_wilson_hop_eo`; a new field.  Even extents only."""
        k = self._pf_checks('wilson_schur', kappa, xn, psi_e)
        L = self._eo_lattice('wilson_schur')
        p, single = self._spinor_native('wilson_schur', xn, psi_e, half=True)
        out = torch.empty_like(p)
        _SchurOp(xn, k, L, antiperiodic_t, p).apply(p, out, dagger, norm=False)
        return out[:, 0] if single else out

    def wilson_schur(self, x: Tensor, psi: Tensor, kappa: float, dagger: bool = False,
                     antiperiodic_t: bool = True) -> Tensor:
        """`wilson_schur_n` in the reference layout: psi is a full-shape field of which only the even sites are read;
        the odd sites of the result are zero."""
        self._pf_checks('wilson_schur', kappa, x, psi)
        self._eo_lattice('wilson_schur')
        pe, single = self._half_reference('wilson_schur', x, psi)
        out = self._half_to_reference(self.wilson_schur_n(self.pack(x), pe, kappa, dagger, antiperiodic_t))
        return out[:, 0] if single else out

    def wilson_solve_schur_normal_n(self, xn: Tensor, phi_e: Tensor, kappa: float, tol: float = 1e-10,
                                    max_iter: int = 1000, check_every: int = 10,
                                    antiperiodic_t: bool = True) -> tuple[Tensor, Tensor, dict]:
        """Mhat^H Mhat X_e = phi_e for every system of the even half field phi_e at once, and Y_e = Mhat X_e:
        `wilson_solve_normal_n` on the Schur complement, the same loop on half fields.  Returns (X_e, Y_e, info), info
        as there with info['action'] = |Y_e|^2."""
        k = self._pf_checks('wilson_solve_schur_normal', kappa, xn, phi_e)
        _CG.check_args('wilson_solve_schur_normal', tol, max_iter, check_every)
        L = self._eo_lattice('wilson_solve_schur_normal')
        b, single = self._spinor_native('wilson_solve_schur_normal', xn, phi_e, half=True)
        op = _SchurOp(xn, k, L, antiperiodic_t, b)
        return self._solve_normal(_CG('wilson_solve_schur_normal', b, single, op, tol, max_iter, check_every))

    # ------------------------------------------------------------ multi-shift CG on the Schur complement
    @staticmethod
    def _shift_list(what: str, shifts) -> list:
        try:
            s = [float(v) for v in shifts]
        except (TypeError, ValueError):
            s = []
        if not s or not all(np.isfinite(v) and v >= 0.0 for v in s):
            raise ValueError(f'LatticeSU3.{what}: shifts must be a non-empty sequence of finite numbers >= 0, got '
                             f'{shifts!r}')
        return s

    def wilson_solve_multishift_n(self, xn: Tensor, phi_e: Tensor, kappa: float, shifts, tol: float = 1e-10,
                                  max_iter: int = 1000, check_every: int = 10, antiperiodic_t: bool = True,
                                  clover: Optional[CloverTerm] = None, freeze: bool = True) -> tuple[Tensor, dict]:
        """(Mhat^H Mhat + sigma_k) X_k = phi_e for every system of the even half field phi_e [nb, nrhs, 12, V/2] (or [nb,
        12, V/2]) and every shift sigma_k >= 0 at once, by multi-shift CG (`_CG.multishift`; Jegerlehner) on the even-odd
        Schur complement of M = 1 - kappa H; with clover= a `CloverTerm` of these links (its kappa must be this one) on
        that of the clover-improved operator.  One Krylov space for all shifts: per iteration the two operator applies of
        `wilson_solve_schur_normal_n`, one `l2q_su3_spinor_axmy_norm` and one fused `l2q_su3_spinor_mshift_update`, which
        reads the residual once for all shifts.  The stopping test is that of the unshifted system, |r|^2 <= tol^2
        |phi_e|^2, every check_every iterations; the shifted residuals are zeta_k r with |zeta_k| <= 1.  With freeze (the
        default) a single shift that meets the test alone stops being updated at that check.  A system's bits do not
        depend on the batch.  Returns (X [nb, nrhs, ns, 12, V/2], info): 'iters', 'converged' [nb, nrhs]; 'shift_iters'
        and 'residual' [nb, nrhs, ns], the latter |phi_e - (Mhat^H Mhat + sigma_k) X_k| / |phi_e| recomputed by one
        operator pass over all nrhs * ns systems.  Never raises on non-convergence; phi_e = 0 gives X = 0.  fp64 only."""
        what = 'wilson_solve_multishift'
        k = self._pf_checks(what, kappa, xn, phi_e)
        _CG.check_args(what, tol, max_iter, check_every)
        sig = self._shift_list(what, shifts)
        L = self._eo_lattice(what)
        b, single = self._spinor_native(what, xn, phi_e, half=True)
        if clover is not None:
            clover = self._clover_for(what, xn, k, getattr(clover, 'c_sw', None), clover)

        def make_op(like):
            if clover is None:
                return _SchurOp(xn, k, L, antiperiodic_t, like)
            return _CloverSchurOp(xn, k, L, antiperiodic_t, like, clover)
        cg = _CG(what, b, single, make_op(b), tol, max_iter, check_every)
        sg = torch.tensor(sig, dtype=torch.float64, device=b.device)
        X = cg.multishift(sg, freeze=bool(freeze))
        nb, nrhs, ns = X.shape[:3]
        Xw = X.view(nb, nrhs * ns, 12, X.shape[-1])
        R = b[:, :, None].repeat(1, 1, ns, 1, 1).view_as(Xw)           # a copy also at ns = 1: b is the caller's
        Q, Z = torch.empty_like(Xw), torch.empty_like(Xw)
        wide = make_op(Xw)
        wide.apply(Xw, Q, False, norm=False)
        wide.apply(Q, Z, True, norm=False)
        ops.su3_spinor_axmy_norm_(R, Z, torch.ones((nb, nrhs * ns), dtype=torch.float64, device=b.device))
        rr = ops.sum_parts(ops.su3_spinor_axmy_norm_(R, Xw, sg.repeat(nb, nrhs).contiguous())).view(nb, nrhs, ns)
        bb = cg.bb[..., None]
        res = torch.sqrt(rr / torch.where(bb > 0, bb, torch.ones_like(bb)))
        info = {'iters': cg.iters, 'converged': ~cg.active, 'shift_iters': cg.shift_iters, 'residual': res}
        if single:
            X, info = X[:, 0], {key: v[:, 0] for key, v in info.items()}
        return X, info

    def wilson_solve_multishift(self, x: Tensor, phi: Tensor, kappa: float, shifts, tol: float = 1e-10,
                                max_iter: int = 1000, check_every: int = 10, antiperiodic_t: bool = True,
                                clover: Optional[CloverTerm] = None, freeze: bool = True) -> tuple[Tensor, dict]:
        """`wilson_solve_multishift_n` in the reference layout: of the full-shape phi [nb, nrhs, T, X, Y, Z, 4, 3] (or
        without nrhs) only the even sites are read; X is [nb, nrhs, ns, T, X, Y, Z, 4, 3], zero on the odd sites."""
        what = 'wilson_solve_multishift'
        self._pf_checks(what, kappa, x, phi)
        _CG.check_args(what, tol, max_iter, check_every)
        self._shift_list(what, shifts)
        self._eo_lattice(what)
        pe, single = self._half_reference(what, x, phi)
        X, info = self.wilson_solve_multishift_n(self.pack(x), pe, kappa, shifts, tol, max_iter, check_every,
                                                 antiperiodic_t, clover, freeze)
        nb, nrhs, ns = X.shape[:3]
        out = self._half_to_reference(X.reshape(nb, nrhs * ns, 12, -1))
        out = out.reshape(nb, nrhs, ns, *out.shape[2:])
        if single:
            out, info = out[:, 0], {key: v[:, 0] for key, v in info.items()}
        return out, info

    # ------------------------------------------------------------ one flavour: the rational (RHMC) pseudofermion
    def _rat_checks(self, what: str, rat) -> None:
        from .rational import Rational
        if not isinstance(rat, Rational):
            raise ValueError(f'LatticeSU3.{what}: rat must be a `rational.Rational` (zolotarev_inv_sqrt), got '
                             f'{type(rat)!r}')

    def rhmc_pseudofermion_refresh_n(self, xn: Tensor, kappa: float, rat, npf: int = 1,
                                     generator: Optional[torch.Generator] = None, antiperiodic_t: bool = True,
                                     **solve_kwargs) -> tuple[Tensor, Tensor]:
        """The heatbath of the one-flavour action S_1 = phi_e^H R(Mhat^H Mhat) phi_e (`rhmc_pseudofermion_action_n`):
        eta_e drawn by the rule of `pseudofermion_refresh_eo_n` (same shape, same generator handling), and phi_e = C
        eta_e with C C^H = R^-1 (rational.py), Qhat = gamma5 Mhat: one multi-shift solve Z_k = (Mhat^H Mhat + nu_k^2)^-1
        eta, two `l2q_su3_spinor_lincomb` W = sum_k c_k Z_k and Vv = sum_k c_k nu_k Z_k, and phi_e = A^(-1/2) (eta + i
        gamma5 Mhat W + Vv); gamma5 = diag(-1, -1, 1, 1) is a sign on components 0..5.  Returns (phi_e [nb, npf, 12,
        V/2], S0 [nb]): S0 = |eta_e|^2 is S_1(phi_e) on these links exactly (to the solver's tolerance), without a
        further solve.  solve_kwargs: tol, max_iter, check_every of the solve."""
        what = 'rhmc_pseudofermion_refresh'
        k = self._pf_checks(what, kappa, xn)
        self._rat_checks(what, rat)
        if isinstance(npf, bool) or not isinstance(npf, (int, np.integer)) or int(npf) < 1:
            raise ValueError(f'LatticeSU3.{what}: npf must be an integer >= 1, got {npf!r}')
        L = self._eo_lattice(what)
        shape = (xn.shape[0], int(npf), 12, self.volume // 2, 2)
        eta = torch.view_as_complex(draw(shape, generator, xn.device) * float(np.sqrt(0.5))).contiguous()
        Zk, _ = self.wilson_solve_multishift_n(xn, eta, k, rat.nu ** 2, antiperiodic_t=antiperiodic_t, **solve_kwargs)
        coef = torch.tensor(np.stack([rat.c, rat.c * rat.nu]), dtype=torch.float64, device=xn.device)
        w = [c.repeat(shape[0], shape[1], 1).contiguous() for c in coef]
        W, Vv = ops.su3_spinor_lincomb(Zk, w[0]), ops.su3_spinor_lincomb(Zk, w[1])
        MW = torch.empty_like(W)
        _SchurOp(xn, k, L, antiperiodic_t, W).apply(W, MW, False, norm=False)
        g5 = torch.ones(12, dtype=torch.float64, device=xn.device)
        g5[:6] = -1.0
        phi = ((eta + 1j * g5[None, None, :, None] * MW + Vv) / float(np.sqrt(rat.A))).contiguous()
        zero = torch.zeros(shape[:2], dtype=torch.float64, device=xn.device)
        return phi, self._sum_fields(_norm2(eta, phi, torch.zeros_like(eta), zero))      # |eta|^2

    def rhmc_pseudofermion_refresh(self, x: Tensor, kappa: float, rat, npf: int = 1,
                                   generator: Optional[torch.Generator] = None, antiperiodic_t: bool = True,
                                   **solve_kwargs) -> tuple[Tensor, Tensor]:
        """`rhmc_pseudofermion_refresh_n` in the reference layout: the full shape phi[nb, npf, T, X, Y, Z, 4, 3], phi_e
        on the even sites and zero on the odd ones"""
        self._pf_checks('rhmc_pseudofermion_refresh', kappa, x)
        self._rat_checks('rhmc_pseudofermion_refresh', rat)
        self._eo_lattice('rhmc_pseudofermion_refresh')
        phi, s0 = self.rhmc_pseudofermion_refresh_n(self.pack(x), kappa, rat, npf, generator, antiperiodic_t,
                                                    **solve_kwargs)
        return self._half_to_reference(phi), s0

    def _rhmc_solve_n(self, what: str, xn: Tensor, phi_e: Tensor, kappa, rat, solve_kwargs):
        """(b [nb, npf, 12, V/2], X [nb, npf, n, 12, V/2], info) of the solve with the poles a_2k as shifts"""
        k = self._pf_checks(what, kappa, xn, phi_e)
        self._rat_checks(what, rat)
        self._eo_lattice(what)
        b = self._spinor_native(what, xn, phi_e, half=True)[0]
        X, info = self.wilson_solve_multishift_n(xn, b, k, rat.poles, **solve_kwargs)
        return k, b, X, info

    def rhmc_pseudofermion_action_n(self, xn: Tensor, phi_e: Tensor, kappa: float, rat,
                                    **solve_kwargs) -> tuple[Tensor, dict]:
        """The action of ONE flavour of Wilson quarks per pseudofermion field on the even-odd Schur complement,
            S_1 = sum_r phi_e,r^H R(Mhat^H Mhat) phi_e,r,   R(y) ~ y^(-1/2) on [rat.ra, rat.rb] (rational.py),
        which puts det R^-1 ~ |det Mhat| = |det M| into the ensemble, up to the relative error rat.delta of R; the
        spectrum of Mhat^H Mhat must lie inside [ra, rb] (`schur_spectrum_n`).  No reweighting by the error of R is
        done.  One `wilson_solve_multishift_n` with the poles a_2k as shifts (whose keywords the others are), and S = A
        (|phi|^2 + sum_k rho_k <phi, X_k>) with <phi, X_k> = |Mhat X_k|^2 + a_2k |X_k|^2 from fixed-order partial sums of
        norms (no cancellation: every term is positive), summed in the order of k, then of the fields.  Returns (S_1 [nb], info); info['action'] [nb, npf] is S per field."""
        k, b, X, info = self._rhmc_solve_n('rhmc_pseudofermion_action', xn, phi_e, kappa, rat, solve_kwargs)
        nb, npf, n = X.shape[:3]
        zero = torch.zeros((nb, npf), dtype=torch.float64, device=b.device)
        s = _norm2(b.clone(), b, torch.zeros_like(b), zero)
        # <phi, X_k> = <(Mhat^H Mhat + a_2k) X_k, X_k> = |Mhat X_k|^2 + a_2k |X_k|^2: two norms per (field, shift), the first
        # fused into one operator pass over the npf * n systems, the second from the residual kernel at alpha = 0
        Xw = X.view(nb, npf * n, 12, -1)
        Q = torch.empty_like(Xw)
        qq = _SchurOp(xn, k, self._lattice_shape, solve_kwargs.get('antiperiodic_t', True), Xw).apply(Xw, Q, False)
        xx = ops.sum_parts(ops.su3_spinor_axmy_norm_(Xw, Q, torch.zeros_like(qq)))
        dots = (qq + torch.tensor(np.tile(rat.poles, npf), dtype=torch.float64, device=b.device) * xx).view(nb, npf, n)
        for j in range(n):
            s = s + float(rat.rho[j]) * dots[:, :, j]
        info['action'] = float(rat.A) * s
        return self._sum_fields(info['action']), info

    def rhmc_pseudofermion_action(self, x: Tensor, phi: Tensor, kappa: float, rat, **solve_kwargs) -> tuple[Tensor, dict]:
        """`rhmc_pseudofermion_action_n` in the reference layout; only the even sites of phi are read"""
        self._pf_checks('rhmc_pseudofermion_action', kappa, x, phi)
        self._eo_lattice('rhmc_pseudofermion_action')
        pe = self._half_reference('rhmc_pseudofermion_action', x, phi)[0]
        return self.rhmc_pseudofermion_action_n(self.pack(x), pe, kappa, rat, **solve_kwargs)

    def rhmc_pseudofermion_force_n(self, xn: Tensor, phi_e: Tensor, kappa: float, rat,
                                   **solve_kwargs) -> tuple[Tensor, dict]:
        """The force of S_1 on the links, in the convention of `grad_action_n`: with X_k = (Mhat^H Mhat + a_2k)^-1 phi_e
        of the same solve as the action's, dS_1 = -A sum_k rho_k X_k^H d(Mhat^H Mhat) X_k, which is the two-flavour
        force of the fields X'_k = sqrt(A rho_k) X_k, Y'_k = Mhat X'_k taken as npf * n systems: the odd halves as in
        `_force_fields_n`, one `l2q_su3_wilson_force`, no new force kernel.  Returns (F [nb, 4, 9, V], info)."""
        k = self._pf_checks('rhmc_pseudofermion_force', kappa, xn, phi_e)
        X, Y, info = self._rhmc_force_fields_n(xn, phi_e, kappa, rat, **solve_kwargs)
        return ops.su3_wilson_force_n(xn, X, Y, k, self._lattice_shape, solve_kwargs.get('antiperiodic_t', True)), info

    def _rhmc_force_fields_n(self, xn: Tensor, phi_e: Tensor, kappa: float, rat, **solve_kwargs):
        """(X, Y, info): the full fields [nb, npf * n, 12, V] whose `l2q_su3_wilson_force` is the force of S_1"""
        what = 'rhmc_pseudofermion_force'
        k, b, X, info = self._rhmc_solve_n(what, xn, phi_e, kappa, rat, solve_kwargs)
        L = self._lattice_shape
        ap = solve_kwargs.get('antiperiodic_t', True)
        nb, npf, n = X.shape[:3]
        w = torch.tensor(np.sqrt(rat.A * rat.rho), dtype=torch.float64, device=b.device)
        Xe = (X * w[None, None, :, None, None]).view(nb, npf * n, 12, -1)
        Ye = torch.empty_like(Xe)
        _SchurOp(xn, k, L, ap, Xe).apply(Xe, Ye, False, norm=False)
        Xo = ops.su3_wilson_hop_eo_n(xn, Xe, L, 1, False, ap, a=k)
        Yo = ops.su3_wilson_hop_eo_n(xn, Ye, L, 1, True, ap, a=k)
        return ops.su3_spinor_merge_eo(Xe, Xo, L), ops.su3_spinor_merge_eo(Ye, Yo, L), info

    def rhmc_pseudofermion_force(self, x: Tensor, phi: Tensor, kappa: float, rat, **solve_kwargs) -> tuple[Tensor, dict]:
        """`rhmc_pseudofermion_force_n` in the reference layout: F[nb, 4, T, X, Y, Z, 3, 3]"""
        self._pf_checks('rhmc_pseudofermion_force', kappa, x, phi)
        self._eo_lattice('rhmc_pseudofermion_force')
        pe = self._half_reference('rhmc_pseudofermion_force', x, phi)[0]
        F, info = self.rhmc_pseudofermion_force_n(self.pack(x), pe, kappa, rat, **solve_kwargs)
        return self.unpack(F), info

    def schur_spectrum_n(self, xn: Tensor, kappa: float, iters: int = 30, generator: Optional[torch.Generator] = None,
                         antiperiodic_t: bool = True, **solve_kwargs) -> tuple[Tensor, Tensor]:
        """(lambda_min, lambda_max) estimates [nb] of Mhat^H Mhat on these links, for the choice of [ra, rb] of the
        rational approximation: lambda_max by `iters` steps of power iteration (a lower estimate of the largest
        eigenvalue), lambda_min by `iters` steps of inverse iteration on `wilson_solve_schur_normal_n` (an upper
        estimate of the smallest), both as Rayleigh quotients of one random start vector.  Leave a margin: the rigorous
        bound is lambda_max <= (1 + 64 kappa^2)^2, from ||H|| <= 8."""
        what = 'schur_spectrum'
        k = self._pf_checks(what, kappa, xn)
        if isinstance(iters, bool) or int(iters) != iters or int(iters) < 1:
            raise ValueError(f'LatticeSU3.{what}: iters must be an integer >= 1, got {iters!r}')
        L = self._eo_lattice(what)
        shape = (xn.shape[0], 1, 12, self.volume // 2, 2)
        v0 = torch.view_as_complex(draw(shape, generator, xn.device)).contiguous()
        op = _SchurOp(xn, k, L, antiperiodic_t, v0)
        zero = torch.zeros(shape[:2], dtype=torch.float64, device=xn.device)

        def normalised(f):
            return (f / torch.sqrt(_norm2(f.clone(), f, torch.zeros_like(f), zero))[..., None, None]).contiguous()
        v, q, z = normalised(v0), torch.empty_like(v0), torch.empty_like(v0)
        for _ in range(int(iters)):
            lmax = op.apply(v, q, False)                                    # <v, A v> = |Mhat v|^2 at |v| = 1
            op.apply(q, z, True, norm=False)
            v = normalised(z)
        u = normalised(v0)
        for _ in range(int(iters)):
            X, _, info = self.wilson_solve_schur_normal_n(xn, u, k, antiperiodic_t=antiperiodic_t, **solve_kwargs)
            u = normalised(X)
        lmin = op.apply(u, q, False)
        return lmin[:, 0], lmax[:, 0]

    def _force_fields_n(self, what: str, xn: Tensor, phin: Tensor, kappa: float, even_odd: bool,
                        **solve_kwargs) -> tuple[Tensor, Tensor, dict]:
        """(X, Y, info), X and Y the full fields whose `l2q_su3_wilson_force` is the force of the pseudofermion action:
        those of `wilson_solve_normal_n`, or with even_odd (and, with mixed=True among the keywords, by
        `wilson_solve_schur_normal_mixed_n`), phin the half field phi_e and the action phi_e^H (Mhat^H
        Mhat)^-1 phi_e: X_e, Y_e from `wilson_solve_schur_normal_n`, X_o = kappa H_oe X_e, Y_o = kappa (H^H)_oe Y_e.
        Exact: dS_f = 2 kappa Re[Y_e^H dH_eo X_o + Y_o^H dH_oe X_e], the full-lattice expression."""
        mixed = self._pop_mixed(what, solve_kwargs, even_odd)
        if not even_odd:
            return self.wilson_solve_normal_n(xn, phin, kappa, **solve_kwargs)
        L = self._eo_lattice(what)
        ap = solve_kwargs.get('antiperiodic_t', True)
        if mixed is None:
            Xe, Ye, info = self.wilson_solve_schur_normal_n(xn, phin, kappa, **solve_kwargs)
        else:
            Xe, Ye, info = self.wilson_solve_schur_normal_mixed_n(xn, phin, kappa, **solve_kwargs, **mixed)
        if Xe.dim() == 3:
            Xe, Ye = Xe[:, None].contiguous(), Ye[:, None].contiguous()
        Xo = ops.su3_wilson_hop_eo_n(xn, Xe, L, 1, False, ap, a=kappa)
        Yo = ops.su3_wilson_hop_eo_n(xn, Ye, L, 1, True, ap, a=kappa)
        return ops.su3_spinor_merge_eo(Xe, Xo, L), ops.su3_spinor_merge_eo(Ye, Yo, L), info

    def wilson_solve_normal(self, x: Tensor, phi: Tensor, kappa: float, tol: float = 1e-10, max_iter: int = 1000,
                            check_every: int = 10, antiperiodic_t: bool = True) -> tuple[Tensor, Tensor, dict]:
        """`wilson_solve_normal_n` in the reference layout"""
        self._pf_checks('wilson_solve_normal', kappa, x, phi)
        pn, single = self._spinor_reference('wilson_solve_normal', x, phi)
        X, Y, info = self.wilson_solve_normal_n(self.pack(x), pn, kappa, tol, max_iter, check_every, antiperiodic_t)
        X, Y = (ops.su3_spinor_unpack(f, self._lattice_shape) for f in (X, Y))
        return (X[:, 0], Y[:, 0], info) if single else (X, Y, info)

    def pseudofermion_refresh_n(self, xn: Tensor, kappa: float, npf: int = 1,
                                generator: Optional[torch.Generator] = None,
                                antiperiodic_t: bool = True) -> tuple[Tensor, Tensor]:
        """The pseudofermion heatbath: eta complex Gaussian with density exp(-eta^H eta) (variance 1/2 per real
        component; `torch.randn((nb, npf, 12, V, 2), dtype=float64)` on the device, or on the host with a CPU
        generator: the same numbers on any machine), phi = M^H eta, which is distributed as exp(-S_f).  Returns (phi
        [nb, npf, 12, V], S0 [nb]): S0 = |eta|^2 is S_f(phi) on these links without a solve."""
        return self._pf_refresh_n('pseudofermion_refresh', xn, kappa, npf, generator, antiperiodic_t, False)

    def pseudofermion_refresh_eo_n(self, xn: Tensor, kappa: float, npf: int = 1,
                                   generator: Optional[torch.Generator] = None,
                                   antiperiodic_t: bool = True) -> tuple[Tensor, Tensor]:
        """The heatbath of the even-odd pseudofermion action phi_e^H (Mhat^H Mhat)^-1 phi_e, which puts det(Mhat^H Mhat) =
        det(M^H M) into the ensemble: eta_e drawn by the rule of `pseudofermion_refresh_n` with the half shape (nb, npf,
        12, V/2, 2), phi_e = Mhat^H eta_e.  Returns (phi_e [nb, npf, 12, V/2], S0 [nb]), S0 = |eta_e|^2."""
        return self._pf_refresh_n('pseudofermion_refresh_eo', xn, kappa, npf, generator, antiperiodic_t, True)

    def _pf_refresh_n(self, what: str, xn: Tensor, kappa, npf, generator, antiperiodic_t, even_odd: bool,
                      cl: Optional[CloverTerm] = None):
        """cl (with even_odd): the clover term, and phi_e = Mhat^H eta_e on the Schur complement of M_sw"""
        k = self._pf_checks(what, kappa, xn)
        if isinstance(npf, bool) or not isinstance(npf, (int, np.integer)) or int(npf) < 1:
            raise ValueError(f'LatticeSU3.{what}: npf must be an integer >= 1, got {npf!r}')
        if even_odd:
            L = self._eo_lattice(what)
        shape = (xn.shape[0], int(npf), 12, self.volume // 2 if even_odd else self.volume, 2)
        eta = torch.view_as_complex(draw(shape, generator, xn.device) * float(np.sqrt(0.5))).contiguous()
        if even_odd:
            phi = torch.empty_like(eta)
            op = _SchurOp(xn, k, L, antiperiodic_t, eta) if cl is None else _CloverSchurOp(xn, k, L, antiperiodic_t, eta, cl)
            op.apply(eta, phi, True, norm=False)
        else:
            phi = ops.su3_wilson_apply_n(xn, eta, k, self._lattice_shape, True, antiperiodic_t)
        zero = torch.zeros(shape[:2], dtype=torch.float64, device=xn.device)
        return phi, self._sum_fields(_norm2(eta, phi, torch.zeros_like(eta), zero))      # |eta|^2

    def pseudofermion_refresh(self, x: Tensor, kappa: float, npf: int = 1, generator: Optional[torch.Generator] = None,
                              antiperiodic_t: bool = True) -> tuple[Tensor, Tensor]:
        """`pseudofermion_refresh_n` in the reference layout: phi[nb, npf, T, X, Y, Z, 4, 3]"""
        self._pf_checks('pseudofermion_refresh', kappa, x)
        phi, s0 = self.pseudofermion_refresh_n(self.pack(x), kappa, npf, generator, antiperiodic_t)
        return ops.su3_spinor_unpack(phi, self._lattice_shape), s0

    def pseudofermion_refresh_eo(self, x: Tensor, kappa: float, npf: int = 1,
                                 generator: Optional[torch.Generator] = None,
                                 antiperiodic_t: bool = True) -> tuple[Tensor, Tensor]:
        """`pseudofermion_refresh_eo_n` in the reference layout: the full shape phi[nb, npf, T, X, Y, Z, 4, 3], phi_e on
        the even sites and zero on the odd ones"""
        self._pf_checks('pseudofermion_refresh_eo', kappa, x)
        self._eo_lattice('pseudofermion_refresh_eo')
        phi, s0 = self.pseudofermion_refresh_eo_n(self.pack(x), kappa, npf, generator, antiperiodic_t)
        return self._half_to_reference(phi), s0

    def _pf_field(self, what: str, x: Tensor, phi: Tensor, even_odd: bool, native: bool) -> Tensor:
        """the checked native field of the action and the force: phi (native, or in the reference layout on the links
        x) as [nb, npf, 12, V], or with even_odd (even extents then) as the half field [nb, npf, 12, V/2]"""
        if even_odd:
            self._eo_lattice(what)
        if native:
            return self._spinor_native(what, x, phi, half=even_odd)[0]
        return (self._half_reference if even_odd else self._spinor_reference)(what, x, phi)[0]

    def pseudofermion_action_n(self, xn: Tensor, phin: Tensor, kappa: float, **solve_kwargs) -> tuple[Tensor, dict]:
        """S_f = sum_r phi_r^H (M^H M)^-1 phi_r = sum_r |Y_r|^2 per chain, by one `wilson_solve_normal_n` (whose
        keywords these are): (S_f [nb], info).  One more keyword, even_odd (default False): with True phin is the half
        field phi_e and S_f = sum_r |Y_e,r|^2 by one `wilson_solve_schur_normal_n`; with mixed=True besides (and its
        inner_tol, max_inner, max_outer) by one `wilson_solve_schur_normal_mixed_n`."""
        self._pf_checks('pseudofermion_action', kappa, xn, phin)
        even_odd = bool(solve_kwargs.pop('even_odd', False))
        mixed = self._pop_mixed('pseudofermion_action', solve_kwargs, even_odd)
        b = self._pf_field('pseudofermion_action', xn, phin, even_odd, native=True)
        solve = self.wilson_solve_schur_normal_n if even_odd else self.wilson_solve_normal_n
        if mixed is not None:
            solve_kwargs.update(mixed)
            solve = self.wilson_solve_schur_normal_mixed_n
        info = solve(xn, b, kappa, **solve_kwargs)[2]
        return self._sum_fields(info['action']), info

    def pseudofermion_action(self, x: Tensor, phi: Tensor, kappa: float, **solve_kwargs) -> tuple[Tensor, dict]:
        """`pseudofermion_action_n` in the reference layout; with even_odd only the even sites of phi are read"""
        self._pf_checks('pseudofermion_action', kappa, x, phi)
        even_odd = bool(solve_kwargs.pop('even_odd', False))
        self._pop_mixed('pseudofermion_action', dict(solve_kwargs), even_odd)       # raises early; the keys travel on
        pn = self._pf_field('pseudofermion_action', x, phi, even_odd, native=False)
        return self.pseudofermion_action_n(self.pack(x), pn, kappa, even_odd=even_odd, **solve_kwargs)

    def pseudofermion_force_n(self, xn: Tensor, phin: Tensor, kappa: float,
                              **solve_kwargs) -> tuple[Tensor, Tensor, dict]:
        """The force of S_f on the links, in the convention of `grad_action_n` (dS_f/dt = sum <p, F> under dU/dt =
        p U; the kick is p <- p - eps F): one `wilson_solve_normal_n` and one `l2q_su3_wilson_force` (see l2q.h).
        Returns (F [nb, 4, 9, V], S_f [nb], info).  even_odd=True among the keywords: phin is the half field phi_e and
        the force is that of phi_e^H (Mhat^H Mhat)^-1 phi_e: one `wilson_solve_schur_normal_n`, the odd halves X_o = kappa H_oe X_e and
        Y_o = kappa (H^H)_oe Y_e by one hop each, and the same `l2q_su3_wilson_force` on the merged fields (exact)."""
        k = self._pf_checks('pseudofermion_force', kappa, xn, phin)
        even_odd = bool(solve_kwargs.pop('even_odd', False))
        self._pop_mixed('pseudofermion_force', dict(solve_kwargs), even_odd)        # raises early; the keys travel on
        b = self._pf_field('pseudofermion_force', xn, phin, even_odd, native=True)
        X, Y, info = self._force_fields_n('pseudofermion_force', xn, b, k, even_odd, **solve_kwargs)
        F = ops.su3_wilson_force_n(xn, X, Y, k, self._lattice_shape, solve_kwargs.get('antiperiodic_t', True))
        return F, self._sum_fields(info['action']), info                           # (mixed=True: solves as the action's)

    def pseudofermion_force(self, x: Tensor, phi: Tensor, kappa: float, **solve_kwargs) -> tuple[Tensor, Tensor, dict]:
        """`pseudofermion_force_n` in the reference layout: F[nb, 4, T, X, Y, Z, 3, 3]; with even_odd only the even
        sites of phi are read"""
        self._pf_checks('pseudofermion_force', kappa, x, phi)
        even_odd = bool(solve_kwargs.pop('even_odd', False))
        self._pop_mixed('pseudofermion_force', dict(solve_kwargs), even_odd)
        pn = self._pf_field('pseudofermion_force', x, phi, even_odd, native=False)
        F, s, info = self.pseudofermion_force_n(self.pack(x), pn, kappa, even_odd=even_odd, **solve_kwargs)
        return self.unpack(F), s, info

    # ------------------------------------------------------------ dynamical clover quarks: pseudofermions
    def _clover_pf_checks(self, what: str, kappa, c_sw, *tensors) -> tuple[float, float]:
        """(kappa, c_sw) after the checks of `_pf_checks` and `_clover_checks`"""
        self._pf_checks(what, kappa, *tensors)
        return self._clover_checks(what, kappa, c_sw, *tensors)

    def wilson_clover_solve_schur_normal_n(self, xn: Tensor, phi_e: Tensor, kappa: float, c_sw: float, tol: float = 1e-10,
                                           max_iter: int = 1000, check_every: int = 10, antiperiodic_t: bool = True,
                                           clover: Optional[CloverTerm] = None) -> tuple[Tensor, Tensor, dict]:
        """Mhat^H Mhat X_e = phi_e for every system of the even half field phi_e at once, and Y_e = Mhat X_e, on the
        asymmetric Schur complement Mhat = A_ee - kappa^2 H_eo A_oo^-1 H_oe of the clover-improved operator:
        `wilson_solve_schur_normal_n` with `_CloverSchurOp`, the same loop.  Returns (X_e, Y_e, info), info as there with
        info['action'] = |Y_e|^2.  `clover` as in `wilson_clover_solve_n`.  ValueError where a chain's A is not positive
        definite.  Double precision only."""
        what = 'wilson_clover_solve_schur_normal'
        k, c = self._clover_pf_checks(what, kappa, c_sw, xn, phi_e)
        _CG.check_args(what, tol, max_iter, check_every)
        L = self._lattice_shape
        b, single = self._spinor_native(what, xn, phi_e, half=True)
        cl = self._clover_for(what, xn, k, c, clover)
        op = _CloverSchurOp(xn, k, L, antiperiodic_t, b, cl)
        return self._solve_normal(_CG(what, b, single, op, tol, max_iter, check_every))

    def wilson_clover_solve_schur_normal(self, x: Tensor, phi: Tensor, kappa: float, c_sw: float, tol: float = 1e-10,
                                         max_iter: int = 1000, check_every: int = 10, antiperiodic_t: bool = True,
                                         clover: Optional[CloverTerm] = None) -> tuple[Tensor, Tensor, dict]:
        """`wilson_clover_solve_schur_normal_n` in the reference layout: of the full-shape phi only the even sites are
        read; the odd sites of X_e and Y_e are zero"""
        self._clover_pf_checks('wilson_clover_solve_schur_normal', kappa, c_sw, x, phi)
        pe, single = self._half_reference('wilson_clover_solve_schur_normal', x, phi)
        X, Y, info = self.wilson_clover_solve_schur_normal_n(self.pack(x), pe, kappa, c_sw, tol, max_iter, check_every,
                                                             antiperiodic_t, clover)
        X, Y = (self._half_to_reference(f) for f in (X, Y))
        return (X[:, 0], Y[:, 0], info) if single else (X, Y, info)

    def clover_pseudofermion_refresh_n(self, xn: Tensor, kappa: float, c_sw: float, npf: int = 1,
                                       generator: Optional[torch.Generator] = None, antiperiodic_t: bool = True,
                                       clover: Optional[CloverTerm] = None) -> tuple[Tensor, Tensor]:
        """The heatbath of the pseudofermion part of the clover action (see `clover_pseudofermion_action_n`): eta_e drawn
        by the rule of `pseudofermion_refresh_eo_n`, phi_e = Mhat^H eta_e on the Schur complement of M_sw.  Returns (phi_e
        [nb, npf, 12, V/2], S0 [nb]), S0 = |eta_e|^2: the pseudofermion part of S_f on these links without a solve (the
        determinant part is not in it).  The clover term is built, and checked, before anything is drawn."""
        what = 'clover_pseudofermion_refresh'
        k, c = self._clover_pf_checks(what, kappa, c_sw, xn)
        cl = self._clover_for(what, xn, k, c, clover)
        return self._pf_refresh_n(what, xn, k, npf, generator, antiperiodic_t, True, cl)

    def clover_pseudofermion_refresh(self, x: Tensor, kappa: float, c_sw: float, npf: int = 1,
                                     generator: Optional[torch.Generator] = None, antiperiodic_t: bool = True,
                                     clover: Optional[CloverTerm] = None) -> tuple[Tensor, Tensor]:
        """`clover_pseudofermion_refresh_n` in the reference layout: the full shape phi[nb, npf, T, X, Y, Z, 4, 3], phi_e
        on the even sites and zero on the odd ones"""
        self._clover_pf_checks('clover_pseudofermion_refresh', kappa, c_sw, x)
        phi, s0 = self.clover_pseudofermion_refresh_n(self.pack(x), kappa, c_sw, npf, generator, antiperiodic_t, clover)
        return self._half_to_reference(phi), s0

    @staticmethod
    def _clover_logdet_part(cl: CloverTerm, npf: int) -> Tensor:
        """-2 npf log det A_oo [nb]"""
        return -2.0 * npf * cl.logdet[:, 1]

    def clover_pseudofermion_action_n(self, xn: Tensor, phi_e: Tensor, kappa: float, c_sw: float,
                                      clover: Optional[CloverTerm] = None, **solve_kwargs) -> tuple[Tensor, dict]:
        """The action of two flavours of clover-improved quarks per pseudofermion field, in the asymmetric even-odd form:
            S_f = sum_r phi_e,r^H (Mhat^H Mhat)^-1 phi_e,r - 2 npf log det A_oo,
        which puts det(M_sw^H M_sw)^npf = (det A_oo det Mhat)^(2 npf) into the ensemble.  One
        `wilson_clover_solve_schur_normal_n` (whose keywords the others are).  Returns (S_f [nb], info): the solve's info
        with info['action'] [nb, npf] the pseudofermion part per field and info['logdet'] [nb] the determinant part."""
        what = 'clover_pseudofermion_action'
        k, c = self._clover_pf_checks(what, kappa, c_sw, xn, phi_e)
        b = self._spinor_native(what, xn, phi_e, half=True)[0]
        cl = self._clover_for(what, xn, k, c, clover)
        info = self.wilson_clover_solve_schur_normal_n(xn, b, k, c, clover=cl, **solve_kwargs)[2]
        info['logdet'] = self._clover_logdet_part(cl, b.shape[1])
        return self._sum_fields(info['action']) + info['logdet'], info

    def clover_pseudofermion_action(self, x: Tensor, phi: Tensor, kappa: float, c_sw: float,
                                    clover: Optional[CloverTerm] = None, **solve_kwargs) -> tuple[Tensor, dict]:
        """`clover_pseudofermion_action_n` in the reference layout; only the even sites of phi are read"""
        self._clover_pf_checks('clover_pseudofermion_action', kappa, c_sw, x, phi)
        pe = self._half_reference('clover_pseudofermion_action', x, phi)[0]
        return self.clover_pseudofermion_action_n(self.pack(x), pe, kappa, c_sw, clover, **solve_kwargs)

    def _clover_force_fields_n(self, xn: Tensor, b: Tensor, k: float, c: float, cl: CloverTerm,
                               **solve_kwargs) -> tuple[Tensor, Tensor, dict]:
        """(X, Y, info): X_e, Y_e of `wilson_clover_solve_schur_normal_n` on the half field b [nb, npf, 12, V/2], completed
        by X_o = kappa A_oo^-1 H_oe X_e and Y_o = kappa A_oo^-1 (H^H)_oe Y_e (one hop each) and merged: the full fields
        whose `l2q_su3_wilson_force` plus `l2q_su3_clover_force` is the force of the clover action (see l2q.h)"""
        L = self._lattice_shape
        ap = solve_kwargs.get('antiperiodic_t', True)
        Xe, Ye, info = self.wilson_clover_solve_schur_normal_n(xn, b, k, c, clover=cl, **solve_kwargs)
        Xo = ops.su3_wilson_clover_hop_eo_n(xn, Xe, L, 1, cl.ainv, 2, False, ap, a=k)
        Yo = ops.su3_wilson_clover_hop_eo_n(xn, Ye, L, 1, cl.ainv, 2, True, ap, a=k)
        return ops.su3_spinor_merge_eo(Xe, Xo, L), ops.su3_spinor_merge_eo(Ye, Yo, L), info

    def clover_pseudofermion_force_n(self, xn: Tensor, phi_e: Tensor, kappa: float, c_sw: float,
                                     clover: Optional[CloverTerm] = None, **solve_kwargs) -> tuple[Tensor, Tensor, dict]:
        """The force of the S_f of `clover_pseudofermion_action_n` on the links, in the convention of `grad_action_n`
        (dS_f/dt = sum <p, F> under dU/dt = p U; the kick is p <- p - eps F): one solve, the two completion hops,
        `l2q_su3_wilson_force` for the hop part and `l2q_su3_clover_force` for the clover part of the pseudofermion term
        and the determinant term, into the same field.  Returns (F [nb, 4, 9, V], S_f [nb], info), info as the action's."""
        what = 'clover_pseudofermion_force'
        k, c = self._clover_pf_checks(what, kappa, c_sw, xn, phi_e)
        b = self._spinor_native(what, xn, phi_e, half=True)[0]
        cl = self._clover_for(what, xn, k, c, clover)
        L = self._lattice_shape
        X, Y, info = self._clover_force_fields_n(xn, b, k, c, cl, **solve_kwargs)
        F = ops.su3_wilson_force_n(xn, X, Y, k, L, solve_kwargs.get('antiperiodic_t', True))
        ops.su3_clover_force_n(xn, X, Y, cl.ainv, k * c, L, det_weight=b.shape[1], f_in=F, out=F)
        info['logdet'] = self._clover_logdet_part(cl, b.shape[1])
        return F, self._sum_fields(info['action']) + info['logdet'], info

    def clover_pseudofermion_force(self, x: Tensor, phi: Tensor, kappa: float, c_sw: float,
                                   clover: Optional[CloverTerm] = None, **solve_kwargs) -> tuple[Tensor, Tensor, dict]:
        """`clover_pseudofermion_force_n` in the reference layout: F[nb, 4, T, X, Y, Z, 3, 3]; only the even sites of phi
        are read"""
        self._clover_pf_checks('clover_pseudofermion_force', kappa, c_sw, x, phi)
        pe = self._half_reference('clover_pseudofermion_force', x, phi)[0]
        F, s, info = self.clover_pseudofermion_force_n(self.pack(x), pe, kappa, c_sw, clover, **solve_kwargs)
        return self.unpack(F), s, info
