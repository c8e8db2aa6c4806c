"""Functional wrappers over the C ABI (``include/l2q.h``): tensors in, tensors out.

SU(3) functions ending in ``_n`` take / return fields in the *native* layout
``xn[nb, 4, 9, V]`` complex128 (see l2q.h); ``su3_pack`` / ``su3_unpack`` convert from / to the
reference's public layout ``x[nb, 4, T, X, Y, Z, 3, 3]``.  Nothing here falls back to PyTorch
arithmetic: every function launches HIP kernels from libl2q.so or raises.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import native as N

C128 = torch.complex128

# bumped whenever parameters are modified by a kernel behind PyTorch's back (the fused Adam
# step on the flat arena does not touch Tensor._version): invalidates cached weight copies
PARAM_GENERATION = [0]


def _vol(lat: Sequence[int]) -> int:
    v = 1
    for n in lat:
        v *= int(n)
    return v


def _ws(nb: int, n_per_chain: int, device) -> torch.Tensor:
    return N.workspace(N.reduce_ws_bytes(nb, n_per_chain), device)


# ---------------------------------------------------------------------------- layout
def transpose(a: torch.Tensor, batch: int, rows: int, cols: int) -> torch.Tensor:
    """[batch, rows, cols] -> [batch, cols, rows] for 4/8/16-byte elements."""
    a = a.contiguous()
    out = torch.empty_like(a)
    N.call('l2q_transpose', a, out, batch, rows, cols, a.element_size())
    return out


def t2d(a: torch.Tensor) -> torch.Tensor:
    """[rows, cols] -> contiguous [cols, rows]."""
    r, c = a.shape
    return transpose(a, 1, r, c).reshape(c, r)


def su3_pack(x: torch.Tensor) -> torch.Tensor:
    """x[nb,4,T,X,Y,Z,3,3] (or any [nb, 4*V*9]-reshapeable) c128 -> xn[nb,4,9,V]."""
    nb = x.shape[0]
    x = x.to(C128).contiguous()
    V = x.numel() // (nb * 36)
    out = torch.empty((nb, 4, 9, V), dtype=C128, device=x.device)
    N.call('l2q_su3_pack', x, out, nb, V)
    return out


def su3_unpack(xn: torch.Tensor, lat: Sequence[int]) -> torch.Tensor:
    nb, _, _, V = xn.shape
    out = torch.empty((nb, 4, *[int(i) for i in lat], 3, 3), dtype=C128, device=xn.device)
    N.call('l2q_su3_unpack', xn.contiguous(), out, nb, V)
    return out


def su3_unpack_select(an: torch.Tensor, bn: torch.Tensor, mask: torch.Tensor,
                      lat: Sequence[int]) -> torch.Tensor:
    """reference-layout x_out[c] = mask[c] ? an[c] : bn[c] from two native fields in one pass"""
    nb, _, _, V = an.shape
    out = torch.empty((nb, 4, *[int(i) for i in lat], 3, 3), dtype=C128, device=an.device)
    N.call('l2q_su3_unpack_select', an.contiguous(), bn.contiguous(), mask.to(torch.float32).contiguous(),
           out, nb, V)
    return out


def pack_entries(a: torch.Tensor, V: int, ncomp: int = 9) -> torch.Tensor:
    """per-entry quantity [nb, 4*V*ncomp] in reference order -> native order [nb, 4*ncomp*V]."""
    nb = a.shape[0]
    return transpose(a.reshape(nb * 4, V, ncomp), nb * 4, V, ncomp).reshape(nb, -1)


def unpack_entries(a: torch.Tensor, V: int, ncomp: int = 9) -> torch.Tensor:
    nb = a.shape[0]
    return transpose(a.reshape(nb * 4, ncomp, V), nb * 4, ncomp, V).reshape(nb, -1)


def native_index(V: int, ncomp: int, device) -> torch.Tensor:
    """idx[j_native] = j_reference for per-entry (ncomp=9) or vec8 (ncomp=8) quantities."""
    return (torch.arange(4 * V * ncomp, device=device).reshape(4, V, ncomp)
            .permute(0, 2, 1).reshape(-1).contiguous())


# ---------------------------------------------------------------------------- SU(3)
def su3_plaq_sums_n(xn: torch.Tensor, lat: Sequence[int]) -> torch.Tensor:
    """[nb, 2]: (sum Re tr P, sum Im tr P) over sites and the 6 planes."""
    nb = xn.shape[0]
    T, X, Y, Z = (int(i) for i in lat)
    out = torch.empty((nb, 2), dtype=torch.float64, device=xn.device)
    ws = _ws(nb, T * X * Y * Z * 36, xn.device)
    N.call('l2q_su3_plaq_reduce', xn, nb, T, X, Y, Z, out, ws, ws.numel())
    return out


def su3_plaq_planes_n(xn: torch.Tensor, lat: Sequence[int]) -> torch.Tensor:
    """[nb, 6, 2]: per-plane (sum Re tr P, sum Im tr P)."""
    nb = xn.shape[0]
    T, X, Y, Z = (int(i) for i in lat)
    out = torch.empty((nb, 6, 2), dtype=torch.float64, device=xn.device)
    ws = N.workspace(N.reduce_ws_bytes(nb, T * X * Y * Z) * 4, xn.device)
    N.call('l2q_su3_plaq_planes', xn, nb, T, X, Y, Z, out, ws, ws.numel())
    return out


def su3_wilson_loops_n(xn: torch.Tensor, lat: Sequence[int]) -> torch.Tensor:
    """[6, nb, T, X, Y, Z] complex128: tr P per plane and site (the reference's `wilson_loops` tensor)."""
    nb = xn.shape[0]
    T, X, Y, Z = (int(i) for i in lat)
    out = torch.empty((6, nb, T, X, Y, Z), dtype=C128, device=xn.device)
    N.call('l2q_su3_wilson_loops', xn, nb, T, X, Y, Z, out)
    return out


def diff_norm2(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """per-chain sum |a - b|^2 (float64 / complex128 tensors of equal shape)."""
    nb = a.shape[0]
    a, b = a.contiguous(), b.contiguous()
    n = a.numel() // nb * (2 if a.is_complex() else 1)
    out = torch.empty(nb, dtype=torch.float64, device=a.device)
    ws = _ws(nb, n, a.device)
    N.call('l2q_diff_norm2_reduce', a, b, nb, n, out, ws, ws.numel())
    return out


def su3_force_n(xn: torch.Tensor, beta: float, lat: Sequence[int]) -> torch.Tensor:
    nb = xn.shape[0]
    T, X, Y, Z = (int(i) for i in lat)
    f = torch.empty_like(xn)
    N.call('l2q_su3_force', xn, float(beta), f, nb, T, X, Y, Z)
    return f


# The Hamiltonian's terms from the kernels that already hold them (l2q_su3_force_action, l2q_su3_assemble_tah_norm2,
# the sum |v_out|^2 request of the sliced heads kernel) instead of separate passes over the fields: [True] = the
# sampler asks for them where it can (dynamics.py: `Dynamics._kernel_energies`), [False] = the separate passes.
USE_KERNEL_ENERGIES = [True]


def su3_force_action_n(xn: torch.Tensor, beta: float, lat: Sequence[int]):
    """(F, plaq): su3_force_n and, from the same launch, plaq [nb] = sum Re tr P = su3_plaq_sums_n(xn)[:, 0] to
    rounding (include/l2q.h: l2q_su3_force_action)."""
    nb = xn.shape[0]
    T, X, Y, Z = (int(i) for i in lat)
    f = torch.empty_like(xn)
    plaq = torch.empty(nb, dtype=torch.float64, device=xn.device)
    ws = N.workspace(int(N.load().l2q_su3_force_action_ws_bytes(nb, T, X, Y, Z)), xn.device)
    N.call('l2q_su3_force_action', xn, float(beta), f, plaq, nb, T, X, Y, Z, ws, ws.numel())
    return f, plaq


class UpperForce:
    """An SU(3) force in upper-plane form (include/l2q.h: l2q_su3_force_upper): `buf` complex128 [nb, 4, 6, V], planes
    e = 0, 4, 8, 1, 2, 5 of the native [nb, 4, 9, V] field; the other three are their anti-Hermitian images.  Taken
    by su3_projsu_digits_n and by the int8-sliced heads kernel (`_sliced_call`), by nothing else."""
    __slots__ = ('buf',)

    def __init__(self, buf: torch.Tensor):
        self.buf = buf

    def full(self) -> torch.Tensor:
        """the native [nb, 4, 9, V] field (a zero keeps the sign the force kernel writes); for tests and tools"""
        u = self.buf
        low = torch.complex(torch.where(u.real == 0, u.real, -u.real), u.imag)
        return torch.stack([u[:, :, 0], u[:, :, 3], u[:, :, 4], low[:, :, 3], u[:, :, 1], u[:, :, 5],
                            low[:, :, 4], low[:, :, 5], u[:, :, 2]], dim=2)


def flat_force(f, nb: int):
    """the [nb, N] view of a force for the heads kernels; an UpperForce as it is"""
    return f if isinstance(f, UpperForce) else f.reshape(nb, -1)


def su3_force_upper_ok(nb: int, lat: Sequence[int]) -> bool:
    """The force kernel of this lattice has the upper-plane output and the sliced heads kernel can address it
    (csrc/heads_sliced.hip: a 32-bit row term, an exact tile -> plane multiply)."""
    V = int(lat[0]) * int(lat[1]) * int(lat[2]) * int(lat[3])
    return (V % 64 == 0 and nb * 192 * V < 2 ** 32 and 36 * (V // 16) ** 2 <= 2 ** 32
            and N.kernel_name('l2q_su3_force_upper', lat) != '')


def su3_force_upper_n(xn: torch.Tensor, beta: float, lat: Sequence[int], want_plaq: bool = False):
    """(UpperForce, plaq [nb] or None): su3_force_n / su3_force_action_n with the upper-plane output -- the same bits
    in the six planes that are stored, the same plaq.  Raises where su3_force_upper_ok says no."""
    nb, V = xn.shape[0], xn.shape[-1]
    T, X, Y, Z = (int(i) for i in lat)
    f = torch.empty((nb, 4, 6, V), dtype=xn.dtype, device=xn.device)
    if not want_plaq:
        N.call('l2q_su3_force_upper', xn, float(beta), f, nb, T, X, Y, Z)
        return UpperForce(f), None
    plaq = torch.empty(nb, dtype=torch.float64, device=xn.device)
    ws = N.workspace(int(N.load().l2q_su3_force_action_ws_bytes(nb, T, X, Y, Z)), xn.device)
    N.call('l2q_su3_force_action_upper', xn, float(beta), f, plaq, nb, T, X, Y, Z, ws, ws.numel())
    return UpperForce(f), plaq


def su3_force_kick_n(xn: torch.Tensor, beta: float, coef: float, vn: torch.Tensor,
                     lat: Sequence[int], v_src: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vn += coef * F(xn) in place; with v_src: vn = v_src + coef * F(xn) (vn only written)."""
    T, X, Y, Z = (int(i) for i in lat)
    if v_src is not None:
        assert v_src.shape == vn.shape and v_src.dtype == vn.dtype and v_src.is_contiguous()
        N.call('l2q_su3_force_kick_to', xn, float(beta), float(coef), v_src, vn, xn.shape[0], T, X, Y, Z)
        return vn
    N.call('l2q_su3_force_kick', xn, float(beta), float(coef), vn, xn.shape[0], T, X, Y, Z)
    return vn


def su3_expm_mul_n(xn: torch.Tensor, vn: torch.Tensor, eps: float,
                   mask_n: Optional[torch.Tensor] = None, complement: bool = False,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    nb, _, _, V = xn.shape
    out = torch.empty_like(xn) if out is None else out
    N.call('l2q_su3_expm_mul', xn, vn, float(eps), mask_n, int(complement), out, nb, V)
    return out


def su3_expm_mul2_n(xn: torch.Tensor, vn: torch.Tensor, eps: float, mask_n: torch.Tensor,
                    complement_first: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Both masked half-updates of one leapfrog step with one expm (== two calls to rounding)."""
    nb, _, _, V = xn.shape
    out = torch.empty_like(xn) if out is None else out
    N.call('l2q_su3_expm_mul2', xn, vn, float(eps), mask_n, int(complement_first), out, nb, V)
    return out


def su3_expm_mul2_vec8_n(xn: torch.Tensor, vn: torch.Tensor, eps: float, mask_n: torch.Tensor,
                         complement_first: bool, out: Optional[torch.Tensor] = None):
    """su3_expm_mul2_n + su3_projsu_vec8_n of its result in one pass: (x', vec8(x'))."""
    nb, _, _, V = xn.shape
    out = torch.empty_like(xn) if out is None else out
    vec = torch.empty((nb, 4, 8, V), dtype=torch.float64, device=xn.device)
    N.call('l2q_su3_expm_mul2_vec8', xn, vn, float(eps), mask_n, int(complement_first), out, vec,
           nb, V)
    return out, vec


def su3_project_su_n(xn: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(xn)
    nf, V = xn.numel() // (9 * xn.shape[-1]), xn.shape[-1]
    N.call('l2q_su3_project_su', xn, out, nf, V)
    return out


def su3_project_tah_n(xn: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(xn)
    nf, V = xn.numel() // (9 * xn.shape[-1]), xn.shape[-1]
    N.call('l2q_su3_project_tah', xn, out, nf, V)
    return out


def su3_project_u_n(xn: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(xn)
    nf, V = xn.numel() // (9 * xn.shape[-1]), xn.shape[-1]
    N.call('l2q_su3_project_u', xn, out, nf, V)
    return out


def su3_mul_n(an: torch.Tensor, bn: torch.Tensor, adjoint_a: bool = False,
              adjoint_b: bool = False) -> torch.Tensor:
    out = torch.empty_like(an)
    nf, V = an.numel() // (9 * an.shape[-1]), an.shape[-1]
    N.call('l2q_su3_mul', an, bn, int(adjoint_a), int(adjoint_b), out, nf, V)
    return out


def su3_projsu_vec8_n(xn: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[..., 9, V] c128 -> [..., 8, V] float64 (native vec8 order).  out: a contiguous float64 buffer of that
    many elements to write instead of a new tensor (the training tape's activation arena)."""
    V = xn.shape[-1]
    nf = xn.numel() // (9 * V)
    shape = (*xn.shape[:-2], 8, V)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=xn.device)
    elif out.numel() != nf * 8 * V or out.dtype != torch.float64 or not out.is_contiguous():
        raise N.L2QError('su3_projsu_vec8_n: bad output buffer')
    N.call('l2q_su3_projsu_vec8', xn, out, nf, V)
    return out.view(shape)


def su3_kinetic_n(vn: torch.Tensor) -> torch.Tensor:
    nb, _, _, V = vn.shape
    out = torch.empty(nb, dtype=torch.float64, device=vn.device)
    ws = _ws(nb, 36 * V, vn.device)
    N.call('l2q_su3_kinetic_reduce', vn, nb, V, out, ws, ws.numel())
    return out


def su3_assemble_tah_n(normals: torch.Tensor) -> torch.Tensor:
    """normals [8, ..., V] float64 -> vn [..., 9, V] (e.g. [8, nb, 4, V] -> [nb, 4, 9, V])."""
    V = normals.shape[-1]
    lead = tuple(normals.shape[1:-1])
    nf = 1
    for i in lead:
        nf *= int(i)
    out = torch.empty((*lead, 9, V), dtype=C128, device=normals.device)
    N.call('l2q_su3_assemble_tah', normals.contiguous(), out, nf, V)
    return out


def su3_assemble_tah_norm2_n(normals: torch.Tensor):
    """normals [8, nb, 4, V] float64 -> (vn [nb, 4, 9, V], norm2 [nb] = sum |vn|^2 per chain, from the same launch)."""
    _, nb, four, V = normals.shape
    assert four == 4
    out = torch.empty((nb, 4, 9, V), dtype=C128, device=normals.device)
    n2 = torch.empty(nb, dtype=torch.float64, device=normals.device)
    ws = _ws(nb, 4 * V, normals.device)
    N.call('l2q_su3_assemble_tah_norm2', normals.contiguous(), out, nb, V, n2, ws, ws.numel())
    return out, n2


def su3_check_su_n(xn: torch.Tensor) -> torch.Tensor:
    nb, _, _, V = xn.shape
    out = torch.empty((nb, 2), dtype=torch.float64, device=xn.device)
    ws = _ws(nb, 36 * V, xn.device)
    N.call('l2q_su3_check_su', xn, nb, V, out, ws, ws.numel())
    return out


def su3_clover_sums_n(xn: torch.Tensor, lat: Sequence[int]) -> torch.Tensor:
    """[nb, 3] raw clover sums over sites: (sum_{mu<nu} -tr F F, -tr(F01 F23 - F02 F13 + F03 F12),
    sum_{mu<nu} Re tr P); E = [:, 0] / V, Q = [:, 1] / (4 pi^2) (see l2q.h)."""
    nb = xn.shape[0]
    T, X, Y, Z = (int(i) for i in lat)
    out = torch.empty((nb, 3), dtype=torch.float64, device=xn.device)
    ws = _ws(nb, T * X * Y * Z * 36, xn.device)
    N.call('l2q_su3_clover_reduce', xn, nb, T, X, Y, Z, out, ws, ws.numel())
    return out


def su3_flow_stage_n(xn: torch.Tensor, pn: Optional[torch.Tensor], c: float, s: float, lat: Sequence[int],
                     p_out: Optional[torch.Tensor] = None, x_out: Optional[torch.Tensor] = None):
    """One low-storage stage of the Wilson flow: p_out = pn + c TAH(U A) (pn None = 0), x_out = exp(s p_out) xn.
    Returns (p_out, x_out); p_out may be pn itself, x_out is never xn."""
    T, X, Y, Z = (int(i) for i in lat)
    p_out = torch.empty_like(xn) if p_out is None else p_out
    x_out = torch.empty_like(xn) if x_out is None else x_out
    N.call('l2q_su3_flow_stage', xn, pn, float(c), float(s), p_out, x_out, xn.shape[0], T, X, Y, Z)
    return p_out, x_out


def su3_flow_step_n(xn: torch.Tensor, x_out: torch.Tensor, ws_p: torch.Tensor, ws_x: torch.Tensor, eps: float,
                    lat: Sequence[int]) -> torch.Tensor:
    """One third-order Wilson-flow step of size eps: xn (only read) -> x_out; ws_p, ws_x are scratch fields."""
    T, X, Y, Z = (int(i) for i in lat)
    N.call('l2q_su3_flow_step', xn, x_out, ws_p, ws_x, float(eps), xn.shape[0], T, X, Y, Z)
    return x_out


def su3_flow_step_err_n(xn: torch.Tensor, x_out: torch.Tensor, ws_p3: torch.Tensor, ws_x: torch.Tensor, eps: float,
                        lat: Sequence[int], d: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`su3_flow_step_n` with its embedded error estimate (`l2q_su3_flow_step_err`): xn (only read) -> x_out, and
    returns d [nb] float64 = max over the chain's links of |W3 - W'|_F / 9, W' the second-order result of the same
    force evaluations (+inf where a link is not finite).  ws_p3 is three scratch fields, [3, *xn.shape]; ws_x one."""
    nb = xn.shape[0]
    T, X, Y, Z = (int(i) for i in lat)
    if tuple(ws_p3.shape) != (3, *xn.shape) or not ws_p3.is_contiguous():
        raise ValueError(f'su3_flow_step_err_n: ws_p3 must be contiguous [3, {", ".join(map(str, xn.shape))}], got '
                         f'{list(ws_p3.shape)}')
    d = torch.empty(nb, dtype=torch.float64, device=xn.device) if d is None else d
    ws = N.workspace(int(N.load().l2q_su3_flow_step_err_ws_bytes(nb, T, X, Y, Z)), xn.device)
    N.call('l2q_su3_flow_step_err', xn, x_out, ws_p3, ws_x, float(eps), d, nb, T, X, Y, Z, ws, ws.numel())
    return d


class FlowStepController:
    """Step-size control of the adaptive Wilson flow (Fritzsch & Ramos, arXiv:1301.4388, App. D); pure Python, it
    never touches a tensor.  A step of size e whose error estimate is d (the largest over the batch) is accepted iff
    d <= tol; accepted or not, the next proposal is e min(grow, safety (tol / d)^(1/3)) (d = 0: e grow), at most
    eps_max where that is given.  A d that is not finite is a rejection that halves e.  More than max_reject
    rejections in a row raise RuntimeError.

        e = ctl.propose(remaining)      # the step to try: the proposal, shortened to `remaining` where it would pass it
        ok = ctl.update(e, d, t)        # judges it; ctl.landed tells whether an accepted step ended on the target

    A step shortened to land on a requested time carries forward the larger of its own proposal and the step size it
    was shortened from, so landing times do not shrink the step."""

    def __init__(self, tol: float, eps0: float = 0.01, eps_max: Optional[float] = None, safety: float = 0.95,
                 grow: float = 2.0, max_reject: int = 20):
        tol, eps0 = float(tol), float(eps0)
        if not (tol > 0 and math.isfinite(tol)) or not (eps0 > 0 and math.isfinite(eps0)):
            raise ValueError(f'FlowStepController: need finite tol > 0 and eps0 > 0, got {tol}, {eps0}')
        if eps_max is not None and not float(eps_max) > 0:
            raise ValueError(f'FlowStepController: need eps_max > 0, got {eps_max}')
        if not 0 < float(safety) <= 1 or not float(grow) > 1 or int(max_reject) < 0:
            raise ValueError(f'FlowStepController: need 0 < safety <= 1, grow > 1 and max_reject >= 0, got {safety}, '
                             f'{grow}, {max_reject}')
        self.tol, self.safety, self.grow, self.max_reject = tol, float(safety), float(grow), int(max_reject)
        self.eps_max = None if eps_max is None else float(eps_max)
        self.eps = self._cap(eps0)          # the next proposal
        self.landed = False                 # the step judged last was shortened to its landing time
        self.nreject = 0                    # all rejections
        self._run = 0                       # rejections in a row
        self._from = None                   # the proposal that the step in flight was shortened from

    def _cap(self, e: float) -> float:
        return e if self.eps_max is None else min(e, self.eps_max)

    def propose(self, remaining: Optional[float] = None) -> float:
        self._from = None
        if remaining is not None and self.eps >= remaining:
            self._from = self.eps
            return float(remaining)
        return self.eps

    def next_eps(self, e: float, d: float) -> float:
        """the proposal that follows a step of size e with estimate d"""
        if not math.isfinite(d):
            return 0.5 * e
        f = self.grow if d == 0.0 else min(self.grow, self.safety * (self.tol / d) ** (1.0 / 3.0))
        return self._cap(e * f)

    def update(self, e: float, d: float, t: float = float('nan')) -> bool:
        e, d = float(e), float(d)
        ok = math.isfinite(d) and d <= self.tol
        nxt = self.next_eps(e, d)
        self.landed = ok and self._from is not None
        if ok:
            self._run = 0
            self.eps = max(nxt, self._from) if self._from is not None else nxt
        else:
            self.nreject += 1
            self._run += 1
            self.eps = nxt
            if self._run > self.max_reject:
                raise RuntimeError(f'FlowStepController: {self._run} rejected steps in a row at t = {t}, e = {e}, '
                                   f'd = {d} (tol = {self.tol})')
        self._from = None
        return ok


def su3_flow_checkpoints_n(xn: torch.Tensor, nsteps: int, eps: float, lat: Sequence[int]):
    """`nsteps` Wilson-flow steps of size eps that keep the field entering each step: -> (flowed, checkpoints) with
    checkpoints[k] the native links entering step k (checkpoints[0] is xn itself, which is never written) -- what
    `su3_flow_bwd_n` reverses.  The same launches as a flow that keeps nothing, so the same bits; nsteps = 0 returns
    (xn, [])."""
    cps, cur = [], xn
    if int(nsteps) > 0:
        ws_p, ws_x = torch.empty_like(xn), torch.empty_like(xn)
        for _ in range(int(nsteps)):
            cps.append(cur)
            cur = su3_flow_step_n(cur, torch.empty_like(xn), ws_p, ws_x, eps, lat)
    return cur, cps


def su3_line_extend_n(lines: torch.Tensor, xn: torch.Tensor, n: int, lat: Sequence[int],
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out_mu(x) = lines_mu(x) U_mu(x + n mu) for all four mu (n >= 0, modulo the extent): lines of length n become
    lines of length n + 1.  out None = a new field; out may be `lines` itself (in place), never xn."""
    T, X, Y, Z = (int(i) for i in lat)
    out = torch.empty_like(xn) if out is None else out
    N.call('l2q_su3_line_extend', lines, xn, int(n), out, xn.shape[0], T, X, Y, Z)
    return out


def su3_loop_sums_n(a: torch.Tensor, r: int, b: torch.Tensor, t: int, lat: Sequence[int]) -> torch.Tensor:
    """[nb, 12] complex128: sum over sites of tr W_{mu nu}, W = a_mu(x) b_nu(x + r mu) a_mu(x + t nu)^H b_nu(x)^H,
    for the ordered pairs mu != nu at index 3 mu + (nu if nu < mu else nu - 1); a, b line fields of lengths r, t."""
    nb = a.shape[0]
    T, X, Y, Z = (int(i) for i in lat)
    out = torch.empty((nb, 12, 2), dtype=torch.float64, device=a.device)
    ws = N.workspace(N.reduce_ws_bytes(nb, T * X * Y * Z) * 6, a.device)
    N.call('l2q_su3_loop_reduce', a, int(r), b, int(t), out, nb, T, X, Y, Z, ws, ws.numel())
    return torch.view_as_complex(out)


def su3_polyakov_n(xn: torch.Tensor, mu: int, lat: Sequence[int]) -> torch.Tensor:
    """[nb, *perp] complex128: tr of the product of the links U_mu around direction mu, per site of the lattice
    with direction mu removed (not divided by 3)."""
    nb = xn.shape[0]
    lat = [int(i) for i in lat]
    mu = int(mu)
    if not 0 <= mu < 4:
        raise ValueError(f'su3_polyakov_n: mu must be 0..3, got {mu}')
    out = torch.empty((nb, *lat[:mu], *lat[mu + 1:]), dtype=C128, device=xn.device)
    N.call('l2q_su3_polyakov', xn, mu, out, nb, *lat)
    return out


def su3_heatbath_(xn: torch.Tensor, beta: float, mu: int, parity: int, u: torch.Tensor, ntry: int,
                  lat: Sequence[int]) -> torch.Tensor:
    """Cabibbo-Marinari / Kennedy-Pendleton heatbath of the links U_mu at the sites of one parity, IN PLACE in the
    native field xn, from the uniforms u[nb, 3, 4 ntry + 2, V/2] float64 (see l2q.h).  Returns [nb] float64: the
    number of (link, subgroup) updates of each chain for which none of the ntry proposals was accepted."""
    nb = xn.shape[0]
    T, X, Y, Z = (int(i) for i in lat)
    ntry = int(ntry)
    vh = T * X * Y * Z // 2
    if u.dtype != torch.float64 or tuple(u.shape) != (nb, 3, 4 * ntry + 2, vh):
        raise ValueError(f'su3_heatbath_: u must be float64 [{nb}, 3, {4 * ntry + 2}, {vh}], got {u.dtype} '
                         f'{list(u.shape)}')
    fails = torch.empty(nb, dtype=torch.float64, device=xn.device)
    ws = _ws(nb, max(vh, 1), xn.device)
    N.call('l2q_su3_heatbath', xn, float(beta), int(mu), int(parity), u, ntry, fails, nb, T, X, Y, Z, ws, ws.numel())
    return fails


def su3_overrelax_(xn: torch.Tensor, mu: int, parity: int, lat: Sequence[int]) -> torch.Tensor:
    """Microcanonical overrelaxation of the links U_mu at the sites of one parity, IN PLACE in the native field xn
    (the three SU(2) subgroups of each link reflected about their staple: the Wilson action is unchanged)."""
    T, X, Y, Z = (int(i) for i in lat)
    N.call('l2q_su3_overrelax', xn, int(mu), int(parity), xn.shape[0], T, X, Y, Z)
    return xn


def su3_gaugefix_sweep_(xn: torch.Tensor, parity: int, dirmask: int, omega: float, lat: Sequence[int],
                        gn: Optional[torch.Tensor] = None, active: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One overrelaxed Los Alamos gauge-fixing step at the sites of one parity, IN PLACE in the native field xn (every
    link is rewritten once; see l2q.h).  dirmask: the gauge directions as a 4-bit set.  gn [nb, 9, V] complex128, when
    given, accumulates the transformation in place; active int32 [nb], when given, freezes the chains that hold 0."""
    nb, V = xn.shape[0], xn.shape[-1]
    T, X, Y, Z = (int(i) for i in lat)
    if gn is not None and (gn.dtype != C128 or tuple(gn.shape) != (nb, 9, V)):
        raise ValueError(f'su3_gaugefix_sweep_: gn must be complex128 [{nb}, 9, {V}], got {gn.dtype} {list(gn.shape)}')
    if active is not None and (active.dtype != torch.int32 or tuple(active.shape) != (nb,)):
        raise ValueError(f'su3_gaugefix_sweep_: active must be int32 [{nb}], got {active.dtype} {list(active.shape)}')
    N.call('l2q_su3_gaugefix_sweep', xn, gn, active, int(dirmask), int(parity), float(omega), nb, T, X, Y, Z)
    return xn


def su3_gauge_condition_n(xn: torch.Tensor, dirmask: int, lat: Sequence[int]) -> torch.Tensor:
    """[nb, 2] float64: the gauge functional F and the residual theta of each chain for the directions in dirmask"""
    nb = xn.shape[0]
    T, X, Y, Z = (int(i) for i in lat)
    out = torch.empty((nb, 2), dtype=torch.float64, device=xn.device)
    ws = _ws(nb, T * X * Y * Z, xn.device)
    N.call('l2q_su3_gauge_condition', xn, int(dirmask), out, nb, T, X, Y, Z, ws, ws.numel())
    return out


def su3_gauge_apply_n(xn: torch.Tensor, gn: torch.Tensor, lat: Sequence[int]) -> torch.Tensor:
    """a new native field g(x) U_mu(x) g(x+mu)^H from gn [nb, 9, V] complex128"""
    nb, V = xn.shape[0], xn.shape[-1]
    T, X, Y, Z = (int(i) for i in lat)
    if gn.dtype != C128 or tuple(gn.shape) != (nb, 9, V):
        raise ValueError(f'su3_gauge_apply_n: gn must be complex128 [{nb}, 9, {V}], got {gn.dtype} {list(gn.shape)}')
    out = torch.empty_like(xn)
    N.call('l2q_su3_gauge_apply', xn, gn, out, nb, T, X, Y, Z)
    return out


def _smear_out(what: str, xn: torch.Tensor, out: Optional[torch.Tensor], decorated: bool) -> torch.Tensor:
    """the output of a smearing launch: a link field [nb, 4, 9, V] or a decorated field [nb, 4, 3, 9, V]"""
    nb, V = xn.shape[0], xn.shape[-1]
    want = (nb, 4, 3, 9, V) if decorated else (nb, 4, 9, V)
    if out is None:
        return torch.empty(want, dtype=C128, device=xn.device)
    if out.dtype != C128 or tuple(out.shape) != want or not out.is_contiguous():
        raise ValueError(f'{what}: out must be contiguous complex128 {list(want)}, got {out.dtype} {list(out.shape)}')
    return out


def _decorated_in(what: str, xn: torch.Tensor, bn: torch.Tensor) -> None:
    want = (xn.shape[0], 4, 3, 9, xn.shape[-1])
    if bn.dtype != C128 or tuple(bn.shape) != want or not bn.is_contiguous():
        raise ValueError(f'{what}: the decorated field must be contiguous complex128 {list(want)}, got {bn.dtype} '
                         f'{list(bn.shape)}')


def su3_ape_smear_n(xn: torch.Tensor, alpha: float, dirmask: int, lat: Sequence[int],
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One APE step of the native field xn over the directions in the 4-bit set dirmask (see l2q.h): the links of the
    other directions are copied.  Out of place: out None = a new field, never xn."""
    T, X, Y, Z = (int(i) for i in lat)
    out = _smear_out('su3_ape_smear_n', xn, out, False)
    N.call('l2q_su3_ape_smear', xn, float(alpha), int(dirmask), out, xn.shape[0], T, X, Y, Z)
    return out


def su3_hyp_level1_n(xn: torch.Tensor, alpha3: float, lat: Sequence[int],
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Level 1 of a HYP step: the decorated field B1 [nb, 4, 3, 9, V] from the thin links (see l2q.h)."""
    T, X, Y, Z = (int(i) for i in lat)
    out = _smear_out('su3_hyp_level1_n', xn, out, True)
    N.call('l2q_su3_hyp_level1', xn, float(alpha3), out, xn.shape[0], T, X, Y, Z)
    return out


def su3_hyp_level2_n(xn: torch.Tensor, b1: torch.Tensor, alpha2: float, lat: Sequence[int],
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Level 2 of a HYP step: the decorated field B2 from the thin links and B1; out is never b1."""
    T, X, Y, Z = (int(i) for i in lat)
    _decorated_in('su3_hyp_level2_n', xn, b1)
    out = _smear_out('su3_hyp_level2_n', xn, out, True)
    N.call('l2q_su3_hyp_level2', xn, b1, float(alpha2), out, xn.shape[0], T, X, Y, Z)
    return out


def su3_hyp_level3_n(xn: torch.Tensor, b2: torch.Tensor, alpha1: float, lat: Sequence[int],
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Level 3 of a HYP step: the smeared links from the thin links and B2; out is never xn."""
    T, X, Y, Z = (int(i) for i in lat)
    _decorated_in('su3_hyp_level3_n', xn, b2)
    out = _smear_out('su3_hyp_level3_n', xn, out, False)
    N.call('l2q_su3_hyp_level3', xn, b2, float(alpha1), out, xn.shape[0], T, X, Y, Z)
    return out


# ---------------------------------------------------------------------------- Wilson fermions
def su3_spinor_pack(psi: torch.Tensor) -> torch.Tensor:
    """psi[nb, nrhs, T, X, Y, Z, 4, 3] c128 -> psin[nb, nrhs, 12, V] (component 3 spin + colour); a new tensor"""
    if psi.dim() != 8 or tuple(psi.shape[-2:]) != (4, 3):
        raise ValueError(f'su3_spinor_pack: need [nb, nrhs, T, X, Y, Z, 4, 3], got {list(psi.shape)}')
    nb, nrhs = psi.shape[:2]
    return psi.to(C128).reshape(nb, nrhs, -1, 12).transpose(2, 3).contiguous()


def su3_spinor_unpack(psin: torch.Tensor, lat: Sequence[int]) -> torch.Tensor:
    nb, nrhs = psin.shape[:2]
    return psin.transpose(2, 3).contiguous().reshape(nb, nrhs, *[int(i) for i in lat], 4, 3)


def su3_wilson_norm_parts(lat: Sequence[int]) -> int:
    """partial sums per system that the spinor kernels leave on this lattice"""
    parts = int(N.load().l2q_su3_wilson_norm_parts(*(int(i) for i in lat)))
    if parts <= 0:
        raise N.L2QError(f'l2q_su3_wilson_norm_parts: bad extents {list(lat)}')
    return parts


def _spinor_check(what: str, name: str, t: torch.Tensor, shape) -> None:
    if t.dtype != C128 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f'{what}: {name} must be contiguous complex128 {list(shape)}, got {t.dtype} {list(t.shape)}')


def _norm_part(what: str, norm, nb: int, nrhs: int, parts, device) -> Optional[torch.Tensor]:
    """the `norm` argument of an operator entry as its partial-sum tensor [nb, nrhs, parts()]: None for False (parts is
    not asked then), a new tensor for True, or the tensor given, checked"""
    if not isinstance(norm, torch.Tensor) and not norm:
        return None
    want = [nb, nrhs, parts()]
    if not isinstance(norm, torch.Tensor):
        return torch.empty(want, dtype=torch.float64, device=device)
    if norm.dtype != torch.float64 or list(norm.shape) != want or not norm.is_contiguous():
        raise ValueError(f'{what}: norm must be contiguous float64 {want}, got {list(norm.shape)}')
    return norm


def su3_wilson_apply_n(xn: torch.Tensor, psin: torch.Tensor, kappa: float, lat: Sequence[int], dagger: bool = False,
                       antiperiodic_t: bool = True, out: Optional[torch.Tensor] = None, norm: bool = False):
    """M psi (dagger: M^H psi) of the native spinor field psin[nb, nrhs, 12, V] on the native links xn (see l2q.h).  Out
    of place: out None = a new field, never psin.  With norm=True returns (out, part), part[nb, nrhs, parts] the
    per-workgroup partial sums of |out|^2 of each system; norm may also be the tensor to write them to."""
    T, X, Y, Z = (int(i) for i in lat)
    if psin.dim() != 4 or psin.shape[0] != xn.shape[0] or psin.shape[2] != 12 or psin.shape[3] != xn.shape[-1]:
        raise ValueError(f'su3_wilson_apply_n: need psin [nb, nrhs, 12, V] on xn {list(xn.shape)}, got {list(psin.shape)}')
    _spinor_check('su3_wilson_apply_n', 'psin', psin, psin.shape)
    if out is None:
        out = torch.empty_like(psin)
    else:
        _spinor_check('su3_wilson_apply_n', 'out', out, psin.shape)
    nb, nrhs = psin.shape[:2]
    part = _norm_part('su3_wilson_apply_n', norm, nb, nrhs, lambda: su3_wilson_norm_parts(lat), psin.device)
    N.call('l2q_su3_wilson_apply', xn, psin, out, part, float(kappa), int(bool(dagger)) | (int(bool(antiperiodic_t)) << 1),
           nb, nrhs, T, X, Y, Z)
    return out if part is None else (out, part)


def su3_spinor_cg_update_(x: torch.Tensor, r: torch.Tensor, p: torch.Tensor, q: torch.Tensor, alpha: torch.Tensor,
                          part: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x += alpha_s p, r -= alpha_s q in place on native spinor fields [nb, nrhs, 12, V], alpha[nb, nrhs] float64 on the
    device; returns the partial sums [nb, nrhs, parts] of |r|^2 of the new r"""
    for name, t in (('x', x), ('r', r), ('p', p), ('q', q)):
        _spinor_check('su3_spinor_cg_update_', name, t, x.shape)
    nb, nrhs, _, V = x.shape
    if alpha.dtype != torch.float64 or alpha.numel() != nb * nrhs or not alpha.is_contiguous():
        raise ValueError(f'su3_spinor_cg_update_: alpha must be contiguous float64 [{nb}, {nrhs}]')
    parts = -(-V // 256)
    if part is None:
        part = torch.empty((nb, nrhs, parts), dtype=torch.float64, device=x.device)
    elif part.dtype != torch.float64 or tuple(part.shape) != (nb, nrhs, parts) or not part.is_contiguous():
        raise ValueError(f'su3_spinor_cg_update_: part must be contiguous float64 {[nb, nrhs, parts]}')
    N.call('l2q_su3_spinor_cg_update', x, r, p, q, alpha, part, nb * nrhs, V)
    return part


def su3_spinor_xpay_(p: torch.Tensor, z: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """p = z + beta_s p in place, beta[nb, nrhs] float64 on the device"""
    _spinor_check('su3_spinor_xpay_', 'p', p, p.shape)
    _spinor_check('su3_spinor_xpay_', 'z', z, p.shape)
    nb, nrhs, _, V = p.shape
    if beta.dtype != torch.float64 or beta.numel() != nb * nrhs or not beta.is_contiguous():
        raise ValueError(f'su3_spinor_xpay_: beta must be contiguous float64 [{nb}, {nrhs}]')
    N.call('l2q_su3_spinor_xpay', p, z, beta, nb * nrhs, V)
    return p


def _shift_coef(what: str, name: str, t: torch.Tensor, shape, dtype=torch.float64) -> None:
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f'{what}: {name} must be contiguous {dtype} {list(shape)}, got {t.dtype} {list(t.shape)}')


def su3_spinor_mshift_update_(x: torch.Tensor, ps: torch.Tensor, p: torch.Tensor, r: torch.Tensor, a: torch.Tensor,
                              b: torch.Tensor, zeta: torch.Tensor, beta: torch.Tensor, live: torch.Tensor) -> None:
    """The fused step of a multi-shift CG iteration, in place (see l2q.h): p = r + beta p on [nb, nrhs, 12, V], and for
    every live shift k  x_k += a_k p_k, p_k = zeta_k r + b_k p_k  on the shifted fields x, ps [nb, nrhs, ns, 12, V].
    a, b, zeta [nb, nrhs, ns] and beta [nb, nrhs] float64, live [nb, nrhs, ns] int32, all on the device."""
    what = 'su3_spinor_mshift_update_'
    if x.dim() != 5 or x.shape[2] < 1:
        raise ValueError(f'{what}: need shifted fields [nb, nrhs, ns, 12, V] with ns >= 1, got {list(x.shape)}')
    nb, nrhs, ns, _, V = x.shape
    _spinor_check(what, 'x', x, (nb, nrhs, ns, 12, V))
    _spinor_check(what, 'ps', ps, x.shape)
    _spinor_check(what, 'p', p, (nb, nrhs, 12, V))
    _spinor_check(what, 'r', r, (nb, nrhs, 12, V))
    for name, t in (('a', a), ('b', b), ('zeta', zeta)):
        _shift_coef(what, name, t, (nb, nrhs, ns))
    _shift_coef(what, 'beta', beta, (nb, nrhs))
    _shift_coef(what, 'live', live, (nb, nrhs, ns), torch.int32)
    N.call('l2q_su3_spinor_mshift_update', x, ps, p, r, a, b, zeta, beta, live, nb * nrhs, ns, V)


def su3_spinor_axmy_norm_(r: torch.Tensor, z: torch.Tensor, alpha: torch.Tensor,
                          part: Optional[torch.Tensor] = None) -> torch.Tensor:
    """r -= alpha_s z in place on native spinor fields [nb, nrhs, 12, V], alpha [nb, nrhs] float64 on the device;
    returns the partial sums [nb, nrhs, parts] of |r|^2 of the new r"""
    what = 'su3_spinor_axmy_norm_'
    if r.dim() != 4:
        raise ValueError(f'{what}: need fields [nb, nrhs, 12, V], got {list(r.shape)}')
    _spinor_check(what, 'r', r, r.shape)
    _spinor_check(what, 'z', z, r.shape)
    nb, nrhs, _, V = r.shape
    _shift_coef(what, 'alpha', alpha, (nb, nrhs))
    parts = -(-V // 256)
    if part is None:
        part = torch.empty((nb, nrhs, parts), dtype=torch.float64, device=r.device)
    else:
        _shift_coef(what, 'part', part, (nb, nrhs, parts))
    N.call('l2q_su3_spinor_axmy_norm', r, z, alpha, part, nb * nrhs, V)
    return part


def su3_spinor_lincomb(x: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = sum_k w_k x_k [nb, nrhs, 12, V] over the ns fields of a system of x [nb, nrhs, ns, 12, V], w [nb, nrhs, ns]
    float64 on the device; summed in the order of k.  out None = a new field."""
    what = 'su3_spinor_lincomb'
    if x.dim() != 5 or x.shape[2] < 1:
        raise ValueError(f'{what}: need shifted fields [nb, nrhs, ns, 12, V] with ns >= 1, got {list(x.shape)}')
    nb, nrhs, ns, _, V = x.shape
    _spinor_check(what, 'x', x, (nb, nrhs, ns, 12, V))
    _shift_coef(what, 'w', w, (nb, nrhs, ns))
    if out is None:
        out = torch.empty((nb, nrhs, 12, V), dtype=C128, device=x.device)
    else:
        _spinor_check(what, 'out', out, (nb, nrhs, 12, V))
    N.call('l2q_su3_spinor_lincomb', x, w, out, nb * nrhs, ns, V)
    return out


def su3_wilson_force_n(xn: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, kappa: float, lat: Sequence[int],
                       antiperiodic_t: bool = True, coef: float = 1.0, f_in: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = (f_in or 0) + coef F_f: the pseudofermion force of the native fields X = (M^H M)^-1 phi, Y = M X, both
    [nb, npf, 12, V], on the native links xn (see l2q.h).  coef = 1 and f_in None give the force; f_in = out = vn the
    kick in place; out None = a new field."""
    T, X_, Y_, Z = (int(i) for i in lat)
    if X.dim() != 4 or X.shape[0] != xn.shape[0] or X.shape[1] < 1 or X.shape[2] != 12 or X.shape[3] != xn.shape[-1]:
        raise ValueError(f'su3_wilson_force_n: need X [nb, npf, 12, V] on xn {list(xn.shape)}, got {list(X.shape)}')
    _spinor_check('su3_wilson_force_n', 'X', X, X.shape)
    _spinor_check('su3_wilson_force_n', 'Y', Y, X.shape)
    for name, t in (('xn', xn), ('f_in', f_in), ('out', out)):
        if t is not None and (t.dtype != C128 or tuple(t.shape) != (xn.shape[0], 4, 9, T * X_ * Y_ * Z)
                              or not t.is_contiguous()):
            raise ValueError(f'su3_wilson_force_n: {name} must be contiguous complex128 [nb, 4, 9, V] on {list(lat)}, '
                             f'got {t.dtype} {list(t.shape)}')
    if out is None:
        out = torch.empty_like(xn)
    N.call('l2q_su3_wilson_force', xn, X, Y, f_in, out, float(kappa), float(coef), int(bool(antiperiodic_t)) << 1,
           xn.shape[0], X.shape[1], T, X_, Y_, Z)
    return out


def _even_lattice(what: str, lat: Sequence[int]) -> tuple:
    L = tuple(int(i) for i in lat)
    if len(L) != 4 or any(e < 2 or e & 1 for e in L):
        raise ValueError(f'{what}: even-odd preconditioning needs even extents, got the lattice {list(L)}')
    return L


_EO_SITES: dict = {}


def su3_eo_sites(lat: Sequence[int], device) -> tuple[torch.Tensor, torch.Tensor]:
    """(even, odd): the sites of each parity (t + x + y + z) & 1 in lexicographic order, int64 [V/2] each, cached per
    (lattice, device); entry h of either is the site 2h or 2h + 1"""
    L = _even_lattice('su3_eo_sites', lat)
    key = (L, str(torch.device(device)))
    if key not in _EO_SITES:
        t, x, y, z = torch.meshgrid(*[torch.arange(e) for e in L], indexing='ij')
        par = ((t + x + y + z) & 1).reshape(-1)
        _EO_SITES[key] = tuple(torch.nonzero(par == p).reshape(-1).to(device) for p in (0, 1))
    return _EO_SITES[key]


def su3_spinor_split_eo(pn: torch.Tensor, lat: Sequence[int]) -> tuple[torch.Tensor, torch.Tensor]:
    """pn[nb, nrhs, 12, V] -> (even, odd) half fields [nb, nrhs, 12, V/2]: new tensors, by a gather"""
    L = _even_lattice('su3_spinor_split_eo', lat)
    if pn.dim() != 4 or pn.shape[2] != 12 or pn.shape[3] != L[0] * L[1] * L[2] * L[3]:
        raise ValueError(f'su3_spinor_split_eo: need pn [nb, nrhs, 12, V] on {list(L)}, got {list(pn.shape)}')
    e, o = su3_eo_sites(L, pn.device)
    return pn.index_select(3, e), pn.index_select(3, o)


def su3_spinor_merge_eo(even: torch.Tensor, odd: torch.Tensor, lat: Sequence[int]) -> torch.Tensor:
    """the inverse of `su3_spinor_split_eo`: a new full field [nb, nrhs, 12, V]"""
    L = _even_lattice('su3_spinor_merge_eo', lat)
    Vh = L[0] * L[1] * L[2] * L[3] // 2
    if even.dim() != 4 or tuple(even.shape[2:]) != (12, Vh) or odd.shape != even.shape or odd.dtype != even.dtype:
        raise ValueError(f'su3_spinor_merge_eo: need two half fields [nb, nrhs, 12, {Vh}] on {list(L)}, got '
                         f'{list(even.shape)} and {list(odd.shape)}')
    e, o = su3_eo_sites(L, even.device)
    pn = torch.empty((*even.shape[:3], 2 * Vh), dtype=even.dtype, device=even.device)
    pn.index_copy_(3, e, even)
    pn.index_copy_(3, o, odd)
    return pn


def su3_wilson_hop_eo_n(xn: torch.Tensor, src: torch.Tensor, lat: Sequence[int], parity: int, dagger: bool = False,
                        antiperiodic_t: bool = True, a: float = 1.0, aux: Optional[torch.Tensor] = None, b: float = 0.0,
                        out: Optional[torch.Tensor] = None, norm: bool = False):
    """out = b aux + a H src on the sites of `parity` (0 even, 1 odd): src[nb, nrhs, 12, V/2] a half field on the other
    parity, aux (None: no b term) and out half fields on this one, on the full native links xn (see l2q.h).  out None =
    a new field; out may be aux, never src.  norm as in `su3_wilson_apply_n`: True returns (out, part), part[nb, nrhs,
    ceil((V/2) / 256)] the partial sums of |out|^2; or the tensor to write them to."""
    T, X, Y, Z = _even_lattice('su3_wilson_hop_eo_n', lat)
    Vh = T * X * Y * Z // 2
    if parity not in (0, 1):
        raise ValueError(f'su3_wilson_hop_eo_n: parity must be 0 or 1, got {parity!r}')
    if src.dim() != 4 or src.shape[0] != xn.shape[0] or src.shape[2] != 12 or src.shape[3] != Vh \
            or xn.shape[-1] != 2 * Vh:
        raise ValueError(f'su3_wilson_hop_eo_n: need a half field src [nb, nrhs, 12, V/2] on xn {list(xn.shape)}, got '
                         f'{list(src.shape)}')
    _spinor_check('su3_wilson_hop_eo_n', 'src', src, src.shape)
    if aux is not None:
        _spinor_check('su3_wilson_hop_eo_n', 'aux', aux, src.shape)
    if out is None:
        out = torch.empty_like(src)
    else:
        _spinor_check('su3_wilson_hop_eo_n', 'out', out, src.shape)
    nb, nrhs = src.shape[:2]
    part = _norm_part('su3_wilson_hop_eo_n', norm, nb, nrhs, lambda: -(-Vh // 256), src.device)
    N.call('l2q_su3_wilson_hop_eo', xn, src, aux, out, part, float(a), float(b),
           int(bool(dagger)) | (int(bool(antiperiodic_t)) << 1), int(parity), nb, nrhs, T, X, Y, Z)
    return out if part is None else (out, part)


# the single-precision kernels of the mixed-precision even-odd solves (csrc/su3_wilson_f32.hip)
C64 = torch.complex64


def _spinor_check_f32(what: str, name: str, t: torch.Tensor, shape) -> None:
    if t.dtype != C64 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f'{what}: {name} must be contiguous complex64 {list(shape)}, got {t.dtype} {list(t.shape)}')


def _system_scalars(what: str, name: str, t: torch.Tensor, nb: int, nrhs: int) -> None:
    if t.dtype != torch.float64 or t.numel() != nb * nrhs or not t.is_contiguous():
        raise ValueError(f'{what}: {name} must be contiguous float64 [{nb}, {nrhs}]')


def su3_links_demote_eo_n(xn: torch.Tensor, lat: Sequence[int], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the fp32, parity-ordered copy of the native links xn[nb, 4, 9, V] complex128: x32[nb, 2, 4, 9, V/2] complex64,
    entry h of parity p the link at the site of that parity of the pair (2h, 2h + 1) (see l2q.h).  Even extents."""
    T, X, Y, Z = _even_lattice('su3_links_demote_eo_n', lat)
    V = T * X * Y * Z
    if xn.dtype != C128 or xn.dim() != 4 or tuple(xn.shape[1:]) != (4, 9, V) or not xn.is_contiguous():
        raise ValueError(f'su3_links_demote_eo_n: xn must be contiguous complex128 [nb, 4, 9, {V}], got {xn.dtype} '
                         f'{list(xn.shape)}')
    shape = (xn.shape[0], 2, 4, 9, V // 2)
    if out is None:
        out = torch.empty(shape, dtype=C64, device=xn.device)
    elif out.dtype != C64 or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f'su3_links_demote_eo_n: out must be contiguous complex64 {list(shape)}, got {out.dtype} '
                         f'{list(out.shape)}')
    N.call('l2q_su3_links_demote_eo', xn, out, xn.shape[0], T, X, Y, Z)
    return out


def su3_wilson_hop_eo_f32_n(x32: torch.Tensor, src: torch.Tensor, lat: Sequence[int], parity: int,
                            dagger: bool = False, antiperiodic_t: bool = True, a: float = 1.0,
                            aux: Optional[torch.Tensor] = None, b: float = 0.0, out: Optional[torch.Tensor] = None,
                            norm: bool = False):
    """`su3_wilson_hop_eo_n` in single precision: complex64 half fields [nb, nrhs, 12, V/2] on the link copy x32[nb, 2,
    4, 9, V/2] of `su3_links_demote_eo_n`.  The norm partials stay float64."""
    T, X, Y, Z = _even_lattice('su3_wilson_hop_eo_f32_n', lat)
    Vh = T * X * Y * Z // 2
    if parity not in (0, 1):
        raise ValueError(f'su3_wilson_hop_eo_f32_n: parity must be 0 or 1, got {parity!r}')
    if x32.dtype != C64 or x32.dim() != 5 or tuple(x32.shape[1:]) != (2, 4, 9, Vh) or not x32.is_contiguous():
        raise ValueError(f'su3_wilson_hop_eo_f32_n: x32 must be contiguous complex64 [nb, 2, 4, 9, {Vh}], got '
                         f'{x32.dtype} {list(x32.shape)}')
    if src.dim() != 4 or src.shape[0] != x32.shape[0] or src.shape[1] < 1 or src.shape[2] != 12 or src.shape[3] != Vh:
        raise ValueError(f'su3_wilson_hop_eo_f32_n: need a half field src [nb, nrhs, 12, V/2] on x32 {list(x32.shape)}, '
                         f'got {list(src.shape)}')
    _spinor_check_f32('su3_wilson_hop_eo_f32_n', 'src', src, src.shape)
    if aux is not None:
        _spinor_check_f32('su3_wilson_hop_eo_f32_n', 'aux', aux, src.shape)
    if out is None:
        out = torch.empty_like(src)
    else:
        _spinor_check_f32('su3_wilson_hop_eo_f32_n', 'out', out, src.shape)
    nb, nrhs = src.shape[:2]
    part = _norm_part('su3_wilson_hop_eo_f32_n', norm, nb, nrhs, lambda: -(-Vh // 256), src.device)
    N.call('l2q_su3_wilson_hop_eo_f32', x32, src, aux, out, part, float(a), float(b),
           int(bool(dagger)) | (int(bool(antiperiodic_t)) << 1), int(parity), nb, nrhs, T, X, Y, Z)
    return out if part is None else (out, part)


def su3_spinor_cg_update_f32_(x: torch.Tensor, r: torch.Tensor, p: torch.Tensor, q: torch.Tensor, alpha: torch.Tensor,
                              part: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`su3_spinor_cg_update_` on complex64 fields; alpha [nb, nrhs] and the partial sums of |r|^2 stay float64"""
    if x.dim() != 4 or x.shape[2] != 12:
        raise ValueError(f'su3_spinor_cg_update_f32_: need fields [nb, nrhs, 12, V], got {list(x.shape)}')
    for name, t in (('x', x), ('r', r), ('p', p), ('q', q)):
        _spinor_check_f32('su3_spinor_cg_update_f32_', name, t, x.shape)
    nb, nrhs, _, V = x.shape
    _system_scalars('su3_spinor_cg_update_f32_', 'alpha', alpha, nb, nrhs)
    parts = -(-V // 256)
    if part is None:
        part = torch.empty((nb, nrhs, parts), dtype=torch.float64, device=x.device)
    elif part.dtype != torch.float64 or tuple(part.shape) != (nb, nrhs, parts) or not part.is_contiguous():
        raise ValueError(f'su3_spinor_cg_update_f32_: part must be contiguous float64 {[nb, nrhs, parts]}')
    N.call('l2q_su3_spinor_cg_update_f32', x, r, p, q, alpha, part, nb * nrhs, V)
    return part


def su3_spinor_xpay_f32_(p: torch.Tensor, z: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """`su3_spinor_xpay_` on complex64 fields; beta [nb, nrhs] stays float64"""
    if p.dim() != 4 or p.shape[2] != 12:
        raise ValueError(f'su3_spinor_xpay_f32_: need fields [nb, nrhs, 12, V], got {list(p.shape)}')
    _spinor_check_f32('su3_spinor_xpay_f32_', 'p', p, p.shape)
    _spinor_check_f32('su3_spinor_xpay_f32_', 'z', z, p.shape)
    nb, nrhs, _, V = p.shape
    _system_scalars('su3_spinor_xpay_f32_', 'beta', beta, nb, nrhs)
    N.call('l2q_su3_spinor_xpay_f32', p, z, beta, nb * nrhs, V)
    return p


def su3_spinor_demote(f64: torch.Tensor, scale: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out32 = scale_s f64: a complex128 field [nb, nrhs, 12, V] times its system's float64 scale [nb, nrhs], rounded to
    complex64 once; out None = a new field"""
    if f64.dim() != 4 or f64.shape[2] != 12:
        raise ValueError(f'su3_spinor_demote: need a field [nb, nrhs, 12, V], got {list(f64.shape)}')
    _spinor_check('su3_spinor_demote', 'f64', f64, f64.shape)
    nb, nrhs, _, V = f64.shape
    _system_scalars('su3_spinor_demote', 'scale', scale, nb, nrhs)
    if out is None:
        out = torch.empty(f64.shape, dtype=C64, device=f64.device)
    else:
        _spinor_check_f32('su3_spinor_demote', 'out', out, f64.shape)
    N.call('l2q_su3_spinor_demote', f64, scale, out, nb * nrhs, V)
    return out


def su3_spinor_promote_axpy_(x64: torch.Tensor, e32: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """x64 += scale_s e32 in place, product and sum in float64; a system with scale_s = 0 keeps its bits"""
    if x64.dim() != 4 or x64.shape[2] != 12:
        raise ValueError(f'su3_spinor_promote_axpy_: need a field [nb, nrhs, 12, V], got {list(x64.shape)}')
    _spinor_check('su3_spinor_promote_axpy_', 'x64', x64, x64.shape)
    _spinor_check_f32('su3_spinor_promote_axpy_', 'e32', e32, x64.shape)
    nb, nrhs, _, V = x64.shape
    _system_scalars('su3_spinor_promote_axpy_', 'scale', scale, nb, nrhs)
    N.call('l2q_su3_spinor_promote_axpy', x64, e32, scale, nb * nrhs, V)
    return x64


# the clover term of the improved Wilson operator (csrc/su3_wilson_clover.hip)
def _clover_field_check(what: str, name: str, t: torch.Tensor, nb: int, Vh: int) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != (nb, 2, 2, 36, Vh) \
            or not t.is_contiguous():
        got = f'{t.dtype} {list(t.shape)}' if isinstance(t, torch.Tensor) else repr(t)
        raise ValueError(f'{what}: {name} must be a contiguous float64 block field [{nb}, 2, 2, 36, {Vh}], got {got}')


def su3_clover_term_n(xn: torch.Tensor, coef: float, lat: Sequence[int], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the block field cl[nb, 2 parity, 2 chirality, 36, V/2] float64 of the clover term A = 1 + coef i sum_{mu<nu}
    sigma_{mu nu} (x) Fhat_{mu nu}, coef = kappa c_sw, on the native links xn[nb, 4, 9, V] (see l2q.h).  Even extents."""
    T, X, Y, Z = _even_lattice('su3_clover_term_n', lat)
    V = T * X * Y * Z
    if xn.dtype != C128 or xn.dim() != 4 or tuple(xn.shape[1:]) != (4, 9, V) or not xn.is_contiguous():
        raise ValueError(f'su3_clover_term_n: xn must be contiguous complex128 [nb, 4, 9, {V}], got {xn.dtype} '
                         f'{list(xn.shape)}')
    if out is None:
        out = torch.empty((xn.shape[0], 2, 2, 36, V // 2), dtype=torch.float64, device=xn.device)
    else:
        _clover_field_check('su3_clover_term_n', 'out', out, xn.shape[0], V // 2)
    N.call('l2q_su3_clover_term', xn, out, float(coef), xn.shape[0], T, X, Y, Z)
    return out


def su3_clover_invert_n(cl: torch.Tensor, lat: Sequence[int], out: Optional[torch.Tensor] = None,
                        logdet: bool = True):
    """(clinv, minpiv_part, logdet_part): the inverse of every block of cl in the same layout, and per (chain, parity,
    workgroup) [nb, 2, ceil((V/2) / 256)] the smallest L D L^H pivot and (logdet; else None) the sum of log d_i.  A
    non-positive pivot is not an error here: the caller looks at minpiv_part."""
    T, X, Y, Z = _even_lattice('su3_clover_invert_n', lat)
    Vh = T * X * Y * Z // 2
    if not isinstance(cl, torch.Tensor) or cl.dim() != 5:
        raise ValueError(f'su3_clover_invert_n: cl must be a block field [nb, 2, 2, 36, {Vh}]')
    nb = cl.shape[0]
    _clover_field_check('su3_clover_invert_n', 'cl', cl, nb, Vh)
    if out is None:
        out = torch.empty_like(cl)
    else:
        _clover_field_check('su3_clover_invert_n', 'out', out, nb, Vh)
    minpiv = torch.empty((nb, 2, -(-Vh // 256)), dtype=torch.float64, device=cl.device)
    ld = torch.empty_like(minpiv) if logdet else None
    N.call('l2q_su3_clover_invert', cl, out, minpiv, ld, nb, T, X, Y, Z)
    return out, minpiv, ld


def su3_wilson_clover_hop_eo_n(xn: torch.Tensor, src: torch.Tensor, lat: Sequence[int], parity: int, c: Optional[torch.Tensor],
                               cmode: int, dagger: bool = False, antiperiodic_t: bool = True, a: float = 1.0,
                               aux: Optional[torch.Tensor] = None, b: float = 0.0, out: Optional[torch.Tensor] = None,
                               norm: bool = False):
    """`su3_wilson_hop_eo_n` with a block field c[nb, 2, 2, 36, V/2] (the clover term or its inverse), C its blocks at
    the output sites: cmode 0 (c None) out = b aux + a H src; 1 out = b (C aux) + a H src; 2 out = C (b aux + a H src)."""
    what = 'su3_wilson_clover_hop_eo_n'
    T, X, Y, Z = _even_lattice(what, lat)
    Vh = T * X * Y * Z // 2
    if parity not in (0, 1):
        raise ValueError(f'{what}: parity must be 0 or 1, got {parity!r}')
    if cmode not in (0, 1, 2) or isinstance(cmode, bool):
        raise ValueError(f'{what}: cmode must be 0, 1 or 2, got {cmode!r}')
    if (c is None) != (cmode == 0):
        raise ValueError(f'{what}: the block field c goes with cmode 1 and 2 and only with them, got cmode {cmode} and '
                         f'c {"None" if c is None else "given"}')
    if src.dim() != 4 or src.shape[0] != xn.shape[0] or src.shape[2] != 12 or src.shape[3] != Vh \
            or xn.shape[-1] != 2 * Vh:
        raise ValueError(f'{what}: need a half field src [nb, nrhs, 12, V/2] on xn {list(xn.shape)}, got '
                         f'{list(src.shape)}')
    _spinor_check(what, 'src', src, src.shape)
    if c is not None:
        _clover_field_check(what, 'c', c, src.shape[0], Vh)
    if aux is not None:
        _spinor_check(what, 'aux', aux, src.shape)
    if out is None:
        out = torch.empty_like(src)
    else:
        _spinor_check(what, 'out', out, src.shape)
    nb, nrhs = src.shape[:2]
    part = _norm_part(what, norm, nb, nrhs, lambda: -(-Vh // 256), src.device)
    N.call('l2q_su3_wilson_clover_hop_eo', xn, src, aux, c, out, part, float(a), float(b),
           int(bool(dagger)) | (int(bool(antiperiodic_t)) << 1), int(parity), int(cmode), nb, nrhs, T, X, Y, Z)
    return out if part is None else (out, part)


def su3_clover_apply_n(c: torch.Tensor, src: torch.Tensor, lat: Sequence[int], parity: int,
                       out: Optional[torch.Tensor] = None, norm: bool = False):
    """out = C src on the half field src[nb, nrhs, 12, V/2] of `parity`, C the blocks of that parity of the block field
    c; out None = a new field, out may be src.  norm as in `su3_wilson_hop_eo_n`."""
    what = 'su3_clover_apply_n'
    T, X, Y, Z = _even_lattice(what, lat)
    Vh = T * X * Y * Z // 2
    if parity not in (0, 1):
        raise ValueError(f'{what}: parity must be 0 or 1, got {parity!r}')
    if src.dim() != 4 or src.shape[2] != 12 or src.shape[3] != Vh:
        raise ValueError(f'{what}: need a half field src [nb, nrhs, 12, V/2] on {[T, X, Y, Z]}, got {list(src.shape)}')
    _spinor_check(what, 'src', src, src.shape)
    _clover_field_check(what, 'c', c, src.shape[0], Vh)
    if out is None:
        out = torch.empty_like(src)
    else:
        _spinor_check(what, 'out', out, src.shape)
    nb, nrhs = src.shape[:2]
    part = _norm_part(what, norm, nb, nrhs, lambda: -(-Vh // 256), src.device)
    N.call('l2q_su3_clover_apply', c, src, out, part, int(parity), nb, nrhs, T, X, Y, Z)
    return out if part is None else (out, part)


def su3_clover_force_n(xn: torch.Tensor, X: Optional[torch.Tensor], Y: Optional[torch.Tensor],
                       clinv: Optional[torch.Tensor], kc: float, lat: Sequence[int], det_weight: float = 0.0,
                       coef: float = 1.0, f_in: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = (f_in or 0) + coef F_sw: the clover part of the force of dynamical clover quarks (`l2q_su3_clover_force`, see
    l2q.h), kc = kappa c_sw.  X, Y [nb, npf, 12, V]: the completed solutions, or both None (the determinant term alone);
    clinv: the block field of A^-1, or None (the pseudofermion term alone); det_weight: npf of the action.  coef, f_in
    and out as in `su3_wilson_force_n`: f_in = out = vn is the kick in place."""
    what = 'su3_clover_force_n'
    T, X_, Y_, Z = _even_lattice(what, lat)
    V = T * X_ * Y_ * Z
    if (X is None) != (Y is None):
        raise ValueError(f'{what}: X and Y come together or not at all')
    if X is None and clinv is None:
        raise ValueError(f'{what}: need the fields X, Y, the blocks clinv, or both')
    for name, t in (('xn', xn), ('f_in', f_in), ('out', out)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != C128 or t.dim() != 4
                              or tuple(t.shape) != (xn.shape[0], 4, 9, V) or not t.is_contiguous()):
            raise ValueError(f'{what}: {name} must be contiguous complex128 [nb, 4, 9, V] on {list(lat)}, got '
                             f'{getattr(t, "dtype", type(t))} {list(getattr(t, "shape", []))}')
    nb, npf = xn.shape[0], 0
    if X is not None:
        if X.dim() != 4 or X.shape[0] != nb or X.shape[1] < 1 or X.shape[2] != 12 or X.shape[3] != V:
            raise ValueError(f'{what}: need X [nb, npf, 12, V] on xn {list(xn.shape)}, got {list(X.shape)}')
        _spinor_check(what, 'X', X, X.shape)
        _spinor_check(what, 'Y', Y, X.shape)
        npf = X.shape[1]
    if clinv is not None:
        _clover_field_check(what, 'clinv', clinv, nb, V // 2)
    if out is None:
        out = torch.empty_like(xn)
    ws = _ws(nb, 54 * V * 64, xn.device)       # 54 V doubles per chain; _ws counts 32 bytes per 256 items
    N.call('l2q_su3_clover_force', xn, X, Y, clinv, f_in, out, float(kc), float(coef), float(det_weight), nb, npf,
           T, X_, Y_, Z, ws, ws.numel())
    return out


def sum_parts(part: torch.Tensor) -> torch.Tensor:
    """[..., parts] -> [...] by a pairwise tree of element-wise additions: the bits of an entry depend on its own
    partials only, not on the batch around it (which a library reduction does not promise).  Always a new tensor."""
    if part.shape[-1] == 1:
        return part[..., 0].clone()
    while part.shape[-1] > 1:
        n = part.shape[-1]
        h = n // 2
        s = part[..., :h] + part[..., h:2 * h]
        part = torch.cat((s, part[..., 2 * h:]), -1) if n & 1 else s
    return part[..., 0]


# ---------------------------------------------------------------------------- shared
def v_update_(v: torch.Tensor, force: torch.Tensor, s: torch.Tensor, t: torch.Tensor,
              q: torch.Tensor, eps: float, forward: bool) -> torch.Tensor:
    """In-place generalised momentum update; returns logdet [nb]."""
    nb = v.shape[0]
    cplx = v.is_complex()
    n = v.numel() // nb
    real_dtype = s.dtype
    logdet = torch.empty(nb, dtype=real_dtype, device=v.device)
    ws = _ws(nb, n, v.device)
    N.call('l2q_v_update', v, force, s, t, q, float(eps), int(forward), int(cplx),
           s.element_size(), nb, n, logdet, ws, ws.numel())
    return logdet


def v_update(v: torch.Tensor, force: torch.Tensor, s: torch.Tensor, t: torch.Tensor,
             q: torch.Tensor, eps: float, forward: bool):
    """Out-of-place generalised momentum update: (v', logdet [nb]); v is not written."""
    nb = v.shape[0]
    n = v.numel() // nb
    out = torch.empty_like(v)
    logdet = torch.empty(nb, dtype=s.dtype, device=v.device)
    ws = _ws(nb, n, v.device)
    N.call('l2q_v_update_to', v, out, force, s, t, q, float(eps), int(forward), int(v.is_complex()),
           s.element_size(), nb, n, logdet, ws, ws.numel())
    return out, logdet


def accept(h_init: torch.Tensor, h_prop: torch.Tensor, sumlogdet: torch.Tensor,
           u: torch.Tensor):
    nb = h_init.shape[0]
    dt = h_init.dtype
    acc = torch.empty(nb, dtype=dt, device=h_init.device)
    mask = torch.empty(nb, dtype=torch.float32, device=h_init.device)
    N.call('l2q_accept', h_init.contiguous(), h_prop.to(dt).contiguous(),
           sumlogdet.to(dt).contiguous(), u.to(dt).contiguous(), acc, mask, nb,
           h_init.element_size())
    return acc, mask


def select_rows(a: torch.Tensor, b: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """out[c] = a[c] if mask[c] else b[c]."""
    nb = a.shape[0]
    a, b = a.contiguous(), b.contiguous()
    row_bytes = a.numel() // nb * a.element_size()
    out = torch.empty_like(a)
    N.call('l2q_select_rows', a, b, mask, out, nb, row_bytes)
    return out


def scale(x: torch.Tensor, alpha: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """alpha * x for float64 / complex128 tensors."""
    out = torch.empty_like(x) if out is None else out
    n = x.numel() * (2 if x.is_complex() else 1)
    N.call('l2q_scale_f64', x, float(alpha), out, n)
    return out


def axpy_(x: torch.Tensor, p: torch.Tensor, alpha: float) -> torch.Tensor:
    N.call('l2q_axpy', p, float(alpha), x, x.numel(), x.element_size())
    return x


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
         a2: Optional[torch.Tensor] = None, w2: Optional[torch.Tensor] = None,
         bias2: Optional[torch.Tensor] = None, coeff: Optional[torch.Tensor] = None,
         scale: float = 1.0, act: Optional[str] = None) -> torch.Tensor:
    """epi(a @ w.T (+ a2 @ w2.T) + bias (+ bias2)) on the MFMA GEMM (fp64 or fp32)."""
    m, k = a.shape
    n = w.shape[0]
    k2 = 0 if a2 is None else a2.shape[1]
    if w.shape[1] != k or (a2 is not None and (w2 is None or w2.shape != (n, k2))):
        raise N.L2QError(f'gemm: shape mismatch a{tuple(a.shape)} w{tuple(w.shape)}')
    for other in (w, bias, a2, w2, bias2, coeff):
        if other is not None and other.dtype != a.dtype:
            raise N.L2QError(f'gemm: dtype mismatch {other.dtype} vs {a.dtype}')
    out = torch.empty((m, n), dtype=a.dtype, device=a.device)
    ws = N.workspace(N.gemm_ws_bytes(m, n, k, k2), a.device)
    name = {torch.float64: 'l2q_gemm_f64', torch.float32: 'l2q_gemm_f32'}.get(a.dtype)
    if name is None:
        raise N.L2QError(f'gemm: unsupported dtype {a.dtype}')
    N.call(name, a, w, m, n, k, a2, w2, k2, bias, bias2, coeff, float(scale), N.ACT[act], out,
           ws, ws.numel())
    return out


# int8-sliced fp64 input layer (csrc/gemm_sliced.hip): [True] = use the digit images when the network
# offers them (LeapfrogLayer.kernel_weights builds them for fp64 SU(3) vnets whose shapes qualify)
USE_SLICED_INPUT = [True]
SLICED_INPUT_EXP = 2          # |su3_to_vec(projectSU(.))| < 2.31 < 2^2 for every entry of the vnet inputs


def gemm_sliced_ok(m: int, n: int, k: int, k2: int = 0) -> bool:
    """Shapes csrc/gemm_sliced.hip serves."""
    return m > 0 and m % 64 == 0 and n % 64 == 0 and k > 0 and k % 64 == 0 and k2 % 64 == 0


def gemm_sliced_pays(m: int, n: int, k: int, k2: int = 0) -> bool:
    """Shapes at which the int8-sliced layer is faster than the fp64 MFMA layer (measured at n = 256,
    tools/sweep_gemm_sliced.py, profiles/r04_gemm_sliced_sweep.txt): m (k + k2) >= 2^24, e.g. 256 chains
    with k + k2 >= 65 536 (the 8^4 lattice has 262 144); below it the fixed 64 x 64 tiles leave CUs idle."""
    return gemm_sliced_ok(m, n, k, k2) and m * n * (k + k2) >= 1 << 32


def gemm_sliced_build(w: torch.Tensor):
    """Digit image of one fp64 weight matrix [n, k] (include/l2q.h: l2q_gemm_sliced_build); None when
    the matrix does not qualify (dtype, shape, non-finite entry)."""
    import ctypes
    n, k = w.shape
    if w.dtype != torch.float64 or not w.is_cuda or n % 64 or k % 64:
        return None
    nbytes = int(N.load().l2q_gemm_sliced_bytes(n, k))
    buf = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    usable = ctypes.c_int(0)
    N.call('l2q_gemm_sliced_build', w.contiguous(), n, k, buf, nbytes, ctypes.byref(usable))
    return buf if usable.value else None


def _sliced_out_ws(name: str, ok: bool, m: int, n: int, k: int, k2: int, device, what: str):
    """(output, workspace) of a sliced input-layer call; refuses shapes csrc/gemm_sliced.hip does not serve."""
    if not ok or not gemm_sliced_ok(m, n, k, k2):
        raise N.L2QError(f'{name}: {what}')
    out = torch.empty((m, n), dtype=torch.float64, device=device)
    return out, N.workspace(int(N.load().l2q_gemm_sliced_ws_bytes(m, n, k, k2)), device)


def sliced_input_images(wx: torch.Tensor, wv: torch.Tensor, gate: str, gated: bool = True):
    """Digit images (ix, iv) of the input layer's two weight matrices, or None when they do not fit comfortably
    (memory gate `gate`; skipped with gated=False) or a matrix is refused.  The images take 7/8 of the weights' bytes
    again (2 x 235 MB per vnet at cfg-4, 2 x 3.8 GB at 16^4): built only while that leaves most of the free memory
    alone."""
    need = 2 * (wx.numel() + wv.numel()) * 8
    if gated and not mem_gate(gate, need, 0.25, wx.device):
        return None
    ix, iv = gemm_sliced_build(wx), gemm_sliced_build(wv)
    return (ix, iv) if ix is not None and iv is not None else None


def gemm_sliced(a: torch.Tensor, image: torch.Tensor, n: int, bias: Optional[torch.Tensor] = None, *,
                a_exp: int = SLICED_INPUT_EXP, a2: Optional[torch.Tensor] = None,
                image2: Optional[torch.Tensor] = None, a2_exp: int = SLICED_INPUT_EXP,
                bias2: Optional[torch.Tensor] = None, coeff: Optional[torch.Tensor] = None,
                scale: float = 1.0, act: Optional[str] = None) -> torch.Tensor:
    """epi(a @ W.T (+ a2 @ W2.T) + bias (+ bias2)) with W / W2 given as digit images and the fp64
    activations sliced on the fly: every |a| must be < 2^a_exp (else the output is NaN)."""
    m, k = a.shape
    k2 = 0 if a2 is None else a2.shape[1]
    out, ws = _sliced_out_ws('gemm_sliced', a.dtype == torch.float64 and not (a2 is not None and image2 is None),
                             m, n, k, k2, a.device, f'a{tuple(a.shape)} n {n} k2 {k2} {a.dtype}')
    N.call('l2q_gemm_sliced_f64', a, image, k, int(a_exp), a2, image2, k2, int(a2_exp), m, n, bias, bias2,
           coeff, float(scale), N.ACT[act], out, ws, ws.numel())
    return out


# activation digit images (csrc/digits.hpp, csrc/gemm_digits.hip): [True] = the sampler's x-update and projection
# write the vnet inputs as int8 digits and the sliced input layer takes both operands as images
USE_DIGIT_INPUTS = [True]


class DigitImage:
    """The digits of an fp64 operand [m, k] with every |entry| < 2^exp: `buf` uint8 [m, k / 64, 7, 64]."""
    __slots__ = ('buf', 'shape', 'exp')

    def __init__(self, buf: torch.Tensor, m: int, k: int, exp: int):
        self.buf, self.shape, self.exp = buf, (m, k), exp


def digits_ok(nb: int, V: int) -> bool:
    """Lattices whose vnet inputs [nb, 32 V] the producers can write as digit images."""
    return nb > 0 and V > 0 and V % 64 == 0


def _digit_buf(m: int, k: int, device) -> torch.Tensor:
    return torch.empty((m, k // 64, 7, 64), dtype=torch.uint8, device=device)


def gemm_digits_slice(a: torch.Tensor, a_exp: int = SLICED_INPUT_EXP) -> Optional[DigitImage]:
    """Digit image of fp64 a [m, k]; None when k % 64 != 0 (or not fp64)."""
    m, k = a.shape
    if a.dtype != torch.float64 or k % 64 or m <= 0:
        return None
    buf = _digit_buf(m, k, a.device)
    N.call('l2q_gemm_digits_slice', a.contiguous(), m, k, int(a_exp), buf, buf.numel())
    return DigitImage(buf, m, k, int(a_exp))


def su3_projsu_digits_n(xn, a_exp: int = SLICED_INPUT_EXP) -> Optional[DigitImage]:
    """su3_projsu_vec8_n(xn).reshape(nb, -1) as a digit image ([nb, 4, 9, V] links); None when the lattice does
    not qualify (digits_ok).  An UpperForce: the same bytes from its six planes."""
    if isinstance(xn, UpperForce):
        nb, _, _, V = xn.buf.shape
        buf = _digit_buf(nb, 32 * V, xn.buf.device)
        N.call('l2q_su3_projsu_digits_upper', xn.buf, buf, int(a_exp), nb * 4, V)
        return DigitImage(buf, nb, 32 * V, int(a_exp))
    nb, V = xn.shape[0], xn.shape[-1]
    if xn.dim() != 4 or xn.shape[1] != 4 or not digits_ok(nb, V):
        return None
    buf = _digit_buf(nb, 32 * V, xn.device)
    N.call('l2q_su3_projsu_digits', xn, buf, int(a_exp), nb * 4, V)
    return DigitImage(buf, nb, 32 * V, int(a_exp))


def su3_pack_digits(x: torch.Tensor, a_exp: int = SLICED_INPUT_EXP):
    """(su3_pack(x), su3_projsu_digits_n(su3_pack(x))) from one read of x: the same bits and bytes.  None when
    the lattice does not qualify (nothing is launched)."""
    nb = x.shape[0]
    x = x.to(C128).contiguous()
    V = x.numel() // (nb * 36)
    if not digits_ok(nb, V):
        return None
    out = torch.empty((nb, 4, 9, V), dtype=C128, device=x.device)
    buf = _digit_buf(nb, 32 * V, x.device)
    N.call('l2q_su3_pack_digits', x, out, buf, int(a_exp), nb, V)
    return out, DigitImage(buf, nb, 32 * V, int(a_exp))


def su3_expm_mul2_digits_n(xn: torch.Tensor, vn: torch.Tensor, eps: float, mask_n: torch.Tensor,
                           complement_first: bool, out: Optional[torch.Tensor] = None,
                           a_exp: int = SLICED_INPUT_EXP):
    """su3_expm_mul2_vec8_n with the vec8 of x' as a digit image: (x', image); None when the lattice does not
    qualify (nothing is launched)."""
    nb, _, _, V = xn.shape
    if not digits_ok(nb, V):
        return None
    out = torch.empty_like(xn) if out is None else out
    buf = _digit_buf(nb, 32 * V, xn.device)
    N.call('l2q_su3_expm_mul2_digits', xn, vn, float(eps), mask_n, int(complement_first), out, buf, int(a_exp),
           nb, V)
    return out, DigitImage(buf, nb, 32 * V, int(a_exp))


def gemm_digits(a: DigitImage, image: torch.Tensor, n: int, bias: Optional[torch.Tensor] = None, *,
                a2: Optional[DigitImage] = None, image2: Optional[torch.Tensor] = None,
                bias2: Optional[torch.Tensor] = None, coeff: Optional[torch.Tensor] = None,
                scale: float = 1.0, act: Optional[str] = None) -> torch.Tensor:
    """gemm_sliced with the activations given as digit images: the same bits."""
    m, k = a.shape
    k2 = 0 if a2 is None else a2.shape[1]
    out, ws = _sliced_out_ws('gemm_digits', not (a2 is not None and (image2 is None or a2.shape[0] != m)),
                             m, n, k, k2, a.buf.device, f'a{a.shape} n {n} k2 {k2}')
    N.call('l2q_gemm_digits_f64', a.buf, image, k, a.exp, None if a2 is None else a2.buf, image2, k2,
           0 if a2 is None else a2.exp, m, n, bias, bias2, coeff, float(scale), N.ACT[act], out, ws, ws.numel())
    return out


def gemm_ex(a: torch.Tensor, w: torch.Tensor, a_trans: bool = False, w_trans: bool = False,
            out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """C (+)= Aop @ Wop^T without transposed copies (include/l2q.h: l2q_gemm_ex).  a: [m, k], or
    [k, m] with a_trans; w: [n, k], or [k, n] with w_trans.  accumulate needs `out`."""
    (k, m) = a.shape if a_trans else a.shape[::-1]
    (kw, n) = w.shape if w_trans else w.shape[::-1]
    if k != kw or a.dtype != w.dtype or a.dtype not in (torch.float32, torch.float64):
        raise N.L2QError(f'gemm_ex: a{tuple(a.shape)} w{tuple(w.shape)} {a.dtype}/{w.dtype}')
    if out is None:
        if accumulate:
            raise N.L2QError('gemm_ex: accumulate needs an output tensor')
        out = torch.empty((m, n), dtype=a.dtype, device=a.device)
    elif out.numel() != m * n or out.dtype != a.dtype or not out.is_contiguous():
        raise N.L2QError('gemm_ex: bad output tensor')
    aligned = all(t.data_ptr() % 16 == 0 for t in (a, w) if t.device.type != 'cpu')
    if (a_trans or w_trans) and not (
            aligned and (gemm_ex_ok(m, a.dtype) if a_trans else gemm_ex_ok(k, a.dtype))
            and (gemm_ex_ok(n, a.dtype) if w_trans else gemm_ex_ok(k, a.dtype))):
        # rows that are not a multiple of 16 bytes: materialise the transposes instead
        y = gemm(t2d(a) if a_trans else a, t2d(w) if w_trans else w)
        if accumulate:
            return add_(out, y)
        out.copy_(y.reshape(out.shape))
        return out
    ws = N.workspace(N.gemm_ws_bytes(m, n, k, 0), a.device)
    N.call('l2q_gemm_ex', a.contiguous(), int(a_trans), w.contiguous(), int(w_trans), m, n, k,
           a.element_size(), int(accumulate), out, ws, ws.numel())
    return out


def gemm_ex_ok(rows: int, dtype: torch.dtype) -> bool:
    """A transposed operand's row length must be a multiple of 16 bytes."""
    return rows % (2 if dtype == torch.float64 else 4) == 0


HALF_TYPES = {torch.float16: 0, torch.bfloat16: 1}


def gemm_h(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
           a2: Optional[torch.Tensor] = None, w2: Optional[torch.Tensor] = None,
           bias2: Optional[torch.Tensor] = None, coeff: Optional[torch.Tensor] = None,
           scale: float = 1.0, act: Optional[str] = None,
           out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Half-precision layer (include/l2q.h: l2q_gemm_h).  w / w2: float16 or bfloat16 [n, k];
    a / a2: that type or float32 (rounded while staged); bias / bias2 / coeff float32;
    out_dtype: w.dtype (default) or float32 (required with coeff)."""
    m, k = a.shape
    n = w.shape[0]
    k2 = 0 if a2 is None else a2.shape[1]
    hd = w.dtype
    if hd not in HALF_TYPES:
        raise N.L2QError(f'gemm_h: weight dtype {hd} is not a 16-bit float')
    if w.shape[1] != k or (a2 is not None and (w2 is None or w2.shape != (n, k2))):
        raise N.L2QError(f'gemm_h: shape mismatch a{tuple(a.shape)} w{tuple(w.shape)}')
    if a.dtype not in (hd, torch.float32) or (a2 is not None and a2.dtype != a.dtype) or \
            (w2 is not None and w2.dtype != hd):
        raise N.L2QError(f'gemm_h: operand dtypes {a.dtype} / {hd}')
    for other in (bias, bias2, coeff):
        if other is not None and other.dtype != torch.float32:
            raise N.L2QError('gemm_h: bias / coeff must be float32')
    out_dtype = (torch.float32 if coeff is not None else hd) if out_dtype is None else out_dtype
    if out_dtype not in (hd, torch.float32):
        raise N.L2QError(f'gemm_h: output dtype {out_dtype}')
    out = torch.empty((m, n), dtype=out_dtype, device=a.device)
    ws = N.workspace(int(N.load().l2q_gemm_h_ws_bytes(m, n, k, k2)), a.device)
    N.call('l2q_gemm_h', HALF_TYPES[hd], a, int(a.dtype == torch.float32), w, m, n, k, a2, w2, k2,
           bias, bias2, coeff, float(scale), N.ACT[act], out, int(out_dtype == torch.float32),
           ws, ws.numel())
    return out


def gemm_h_u1x(x: torch.Tensor, mask: torch.Tensor, complement: bool, w: torch.Tensor,
               bias: torch.Tensor, a2: torch.Tensor, w2: torch.Tensor, bias2: torch.Tensor,
               act: Optional[str]) -> torch.Tensor:
    """Input layer of the half-precision U(1) xnet with the masked cos / sin formed in the tile
    loader (include/l2q.h: l2q_gemm_h_u1x).  x [nb, xdim] fp32 angles, w [n, 2 xdim] 16-bit,
    a2 = v [nb, k2] fp32, w2 [n, k2] 16-bit -> [nb, n] 16-bit."""
    m, xdim = x.shape
    n = w.shape[0]
    k2 = a2.shape[1]
    hd = w.dtype
    if w.shape[1] != 2 * xdim or w2.shape != (n, k2) or hd not in HALF_TYPES or \
            x.dtype != torch.float32 or a2.dtype != torch.float32:
        raise N.L2QError(f'gemm_h_u1x: x{tuple(x.shape)} w{tuple(w.shape)} w2{tuple(w2.shape)}')
    out = torch.empty((m, n), dtype=hd, device=x.device)
    ws = N.workspace(int(N.load().l2q_gemm_h_ws_bytes(m, n, 2 * xdim, k2)), x.device)
    N.call('l2q_gemm_h_u1x', HALF_TYPES[hd], x.contiguous(), mask.reshape(-1).contiguous(),
           int(complement), w, m, n, xdim, a2.contiguous(), w2, k2, bias, bias2, N.ACT[act], out,
           ws, ws.numel())
    return out


def u1_heads_update_h_(z: torch.Tensor, heads: dict, scale_t: float, a: torch.Tensor,
                       b: torch.Tensor, eps: float, forward: bool, *,
                       mask: Optional[torch.Tensor] = None, complement: bool = False,
                       use_ncp: bool = True, acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Half-precision heads + sub-update in one kernel (include/l2q.h: l2q_u1_heads_update_h).
    heads: {'s': (W16, b, cs), 't': (W16, b, None), 'q': (W16, b, cq)} with cs / cq the fp32
    per-entry scales nw * exp(coeff).  mask given: x-update (a = x, b = v), else v-update
    (a = v, b = force); a is updated in place.  Returns logdet [nb] fp32 (acc: added into it)."""
    m, k = z.shape
    ws_, bs, cs = heads['s']
    wt, bt, _ = heads['t']
    wq, bq, cq = heads['q']
    n = ws_.shape[0]
    if z.dtype not in HALF_TYPES or ws_.dtype != z.dtype:
        raise N.L2QError(f'u1_heads_update_h: dtypes {z.dtype} / {ws_.dtype}')
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.numel() != m * n:
        raise N.L2QError('u1_heads_update_h: the lattice operands are fp32 [nb, n]')
    logdet = acc if acc is not None else torch.empty(m, dtype=torch.float32, device=z.device)
    ws = N.workspace(int(N.load().l2q_u1_heads_update_h_ws_bytes(m, n)), z.device)
    N.call('l2q_u1_heads_update_h', HALF_TYPES[z.dtype], z, m, k, n, ws_, bs, cs, wt, bt,
           float(scale_t), wq, bq, cq, int(mask is not None), a, b, mask, int(complement),
           float(eps), int(forward), int(use_ncp), logdet, int(acc is not None), ws, ws.numel())
    return logdet


# int8-sliced heads (csrc/heads_sliced.hip): [True] = use the slice image when the network offers one
# (`heads['sliced']`, built by network.kernel_weights for fp64 heads with K = 256 outside training)
USE_SLICED_HEADS = [True]
SLICED_K = 256


SLICED_IMAGE_MAX_FREE_FRACTION = [0.25]     # heads_sliced_build: largest share of the free device memory


# ---- memory gates: ONE helper for every "take the faster path only while it fits comfortably" decision
# (ADVICE r04).  The int8-sliced and the fp64 kernels agree to rounding, not bit for bit, so a gate that
# silently flips with the allocator's state would make a run irreproducible from its seed and could put the
# ranks of a data-parallel job on different paths.  Every refusal is therefore RECORDED (MEM_GATE_LOG) and logged
# once per gate; `MEM_GATE_POLICY[0]` makes the choice explicit: 'auto' (default: gate on free + idle memory),
# 'always' (take the path, let the allocator fail loudly if it cannot), 'never' (the fp64 / un-deferred path).
# `mem_gate_signature()` is what a distributed job compares across ranks (Trainer does, and warns).
MEM_GATE_POLICY = ['auto']
MEM_GATE_LOG: dict = {}


def device_headroom(device) -> int:
    """bytes a new allocation can count on: free device memory + the caching allocator's idle blocks"""
    if not (isinstance(device, torch.device) and device.type == 'cuda'):
        return 1 << 62
    free, _total = torch.cuda.mem_get_info(device)
    return int(free + torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device))


# In a data-parallel job the ranks must take the SAME path (the overlapped gradient exchange launches
# one collective per finished parameter range, and which ranges exist depends on these gates -- ranks that
# disagree would issue mismatched all-reduces).  With torch.distributed initialised and more than one rank, an
# 'auto' decision is therefore made ONCE per (gate, size) by all ranks together -- the path is taken only if
# every rank can afford it (all-reduce MIN, before the first kernel that depends on it) -- and kept for the rest
# of the process.  Every rank reaches a gate in the same program order, so the collective matches up.
MEM_GATE_CONSENSUS = [True]
_MEM_GATE_AGREED: dict = {}


def _multi_rank() -> bool:
    import torch.distributed as dist
    return bool(MEM_GATE_CONSENSUS[0] and dist.is_available() and dist.is_initialized()
                and dist.get_world_size() > 1)


def _ranks_agree(ok: bool, device) -> bool:
    """all-reduce MIN of one rank-local yes / no"""
    import torch.distributed as dist
    backend = str(dist.get_backend())
    on_dev = 'nccl' in backend and isinstance(device, torch.device) and device.type == 'cuda'
    if not on_dev and 'gloo' not in backend:
        return ok                                     # (an RCCL-only group and a host-side decision: nothing to compare)
    t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=device if on_dev else 'cpu')
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return bool(int(t.item()))


def mem_gate(what: str, need_bytes: int, fraction: float, device) -> bool:
    """True: `need_bytes` may be taken for `what` (at most `fraction` of the headroom)."""
    pol = MEM_GATE_POLICY[0]
    if pol == 'always':
        ok = True
    elif pol == 'never':
        ok = False
    else:
        key = (what, int(need_bytes))
        if key in _MEM_GATE_AGREED:
            ok = _MEM_GATE_AGREED[key]
        else:
            ok = need_bytes <= fraction * device_headroom(device)
            if _multi_rank():
                ok = _MEM_GATE_AGREED[key] = _ranks_agree(ok, device)
    prev = MEM_GATE_LOG.get(what)
    MEM_GATE_LOG[what] = ok
    if not ok and prev is not False:
        import logging
        logging.getLogger('l2hmc').warning(
            'memory gate: %s not taken (%.2f GiB wanted, policy %s) -- the slower equivalent path runs; '
            'results agree with the faster one to rounding only', what, need_bytes / 2 ** 30, pol)
    return ok


def mem_gate_signature() -> tuple:
    return tuple(sorted(MEM_GATE_LOG.items()))


def heads_sliced_build(heads: dict):
    """int8 slice image of the three head weight matrices (include/l2q.h: l2q_heads_sliced_build).
    Returns the uint8 device buffer, or None when the weights do not qualify (dtype, K, dynamic range)."""
    import ctypes
    ws_, wt, wq = heads['s'][0], heads['t'][0], heads['q'][0]
    n, k = ws_.shape
    if ws_.dtype != torch.float64 or k != SLICED_K or not ws_.is_cuda:
        return None
    nbytes = int(N.load().l2q_heads_sliced_bytes(k, n))
    # the image lives NEXT TO the fp64 weights (+87 % of their size: 0.7 GB per vnet at 8^4, 11 GB at 16^4):
    # built only while it is a small part of what the device still has (free + the allocator's idle blocks)
    if not mem_gate('sliced heads image', nbytes, SLICED_IMAGE_MAX_FREE_FRACTION[0], ws_.device):
        return None
    buf = torch.empty(nbytes, dtype=torch.uint8, device=ws_.device)
    usable = ctypes.c_int(0)
    N.call('l2q_heads_sliced_build', ws_, wt, wq, k, n, buf, nbytes, ctypes.byref(usable))
    return buf if usable.value else None


def heads_sliced_build_into(ws_: torch.Tensor, wt: torch.Tensor, wq: torch.Tensor,
                            buf: Optional[torch.Tensor] = None):
    """The slice image of three [n, 256] fp64 weight matrices, written into `buf` when it has the right size
    (the training loop rebuilds the image every optimiser step: no allocation after the first).
    Returns (buffer, usable)."""
    import ctypes
    n, k = ws_.shape
    nbytes = int(N.load().l2q_heads_sliced_bytes(k, n))
    if buf is None or buf.numel() != nbytes or buf.device != ws_.device:
        if not mem_gate('sliced heads image (training tape)', nbytes, SLICED_IMAGE_MAX_FREE_FRACTION[0],
                        ws_.device):
            return None, False                       # (same memory gate as heads_sliced_build)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=ws_.device)
    usable = ctypes.c_int(0)
    N.call('l2q_heads_sliced_build', ws_, wt, wq, k, n, buf, nbytes, ctypes.byref(usable))
    return buf, bool(usable.value)


def vnet_heads_vupdate_sliced_tape(z: torch.Tensor, image: torch.Tensor, bs: torch.Tensor, cs: torch.Tensor,
                                   bt: torch.Tensor, scale_t: float, bq: torch.Tensor, cq: torch.Tensor,
                                   v: torch.Tensor, force: torch.Tensor, eps: float, forward: bool):
    """Forward pass of the training tape on the int8-sliced heads kernel (include/l2q.h:
    l2q_vnet_heads_vupdate_sliced_tape_f64): (v', logdet [nb], s, t, q); v is not written.
    cs / cq: per-entry scales nw.s exp(coeff_s) / nw.q exp(coeff_q)."""
    m, k = z.shape
    n = bs.numel()
    out = torch.empty_like(v)
    s = torch.empty((m, n), dtype=torch.float64, device=z.device)
    t = torch.empty_like(s)
    q = torch.empty_like(s)
    logdet = torch.empty(m, dtype=torch.float64, device=z.device)
    nbytes = int(N.load().l2q_vnet_heads_sliced_ws_bytes(m, n))
    ws = N.workspace(nbytes, z.device)
    N.call('l2q_vnet_heads_vupdate_sliced_tape_f64', z, m, k, n, image, bs, cs, bt, float(scale_t), bq, cq, v,
           out, force, int(v.is_complex()), float(eps), int(forward), s, t, q, logdet, ws, ws.numel())
    return out, logdet, s, t, q


def heads_sliced_zflag(reset: bool = True) -> int:
    """Number of activation rows handed to the sliced heads kernel since the last reset whose mean
    |entry| was below 2^-6 of their largest one (include/l2q.h: l2q_heads_sliced_zflag; synchronises).
    0 with tanh networks; > 0 means the sliced products of those rows carry the absolute bound
    2^-54 K max|z| max|w| instead of fp64's relative one -- `dyn.sliced_heads = False` selects fp64."""
    import ctypes
    count = ctypes.c_int(0)
    N.call('l2q_heads_sliced_zflag', int(reset), ctypes.byref(count))
    return int(count.value)


def _sliced_call(z, heads, scales, v, force, eps1, forward1, pair, flip, eps2, forward2, v_src=None,
                 mid=False, norm2=False):
    """out[0] = logdet; mid (pair): out[1] = the first update's logdet, out[2] = sum |v_mid|^2;
    norm2 (single update): out[2] = sum |v_out|^2"""
    m, k = z.shape
    _, bs, cs = heads['s']
    _, bt, _ = heads['t']
    wq, bq, cq = heads['q']
    n = wq.shape[0]
    assert not (norm2 and (pair or mid))
    out = torch.empty((3 if mid or norm2 else 1, m), dtype=torch.float64, device=z.device)
    nbytes = int(N.load().l2q_vnet_heads_sliced_ws_bytes(m, n))
    ws = N.workspace(nbytes, z.device)
    args = (z, m, k, n, heads['sliced'], bs, cs, float(scales[0]), bt, float(scales[1]), bq, cq, float(scales[2]),
            v_src, v, force.buf if isinstance(force, UpperForce) else force, int(v.is_complex()), float(eps1),
            int(forward1), int(pair), int(flip), float(eps2), int(forward2), out[0], out[1] if mid else None,
            out[2] if mid or norm2 else None, ws, ws.numel())
    if isinstance(force, UpperForce):
        N.call('l2q_vnet_heads_vupdate_sliced_upper_f64', *args, 1, force.buf.shape[-1])
    else:
        N.call('l2q_vnet_heads_vupdate_sliced_f64', *args)
    return out


def heads_take_upper_force(heads: dict) -> bool:
    """The heads + update of these weights run on the int8-sliced kernel (`_use_sliced` for an fp64 activation
    of their width), the one heads kernel that reads an UpperForce."""
    ws_ = heads['s'][0]
    return bool(USE_SLICED_HEADS[0] and heads.get('use_sliced', True) and heads.get('sliced') is not None
                and ws_.dtype == torch.float64 and ws_.shape[1] == SLICED_K
                and heads['s'][2] is not None and heads['q'][2] is not None)


def _full_force(force) -> None:
    if isinstance(force, UpperForce):
        raise N.L2QError('an upper-plane force reached a heads kernel that reads the full field')


def _use_sliced(z, heads) -> bool:
    # (the sliced kernel takes per-entry scales; a heads dict with scalar scales stays on the fp64 kernel)
    return (USE_SLICED_HEADS[0] and heads.get('use_sliced', True) and heads.get('sliced') is not None
            and z.dtype == torch.float64
            and z.shape[1] == SLICED_K and heads['s'][2] is not None and heads['q'][2] is not None)


def vnet_heads_vupdate_(z: torch.Tensor, heads: dict, scales, v: torch.Tensor,
                        force: torch.Tensor, eps: float, forward: bool,
                        v_src: Optional[torch.Tensor] = None, norm2: Optional[list] = None) -> torch.Tensor:
    """Fused (s, t, q) heads + generalised momentum update, v in place; returns logdet [nb].
    norm2: a list that receives sum |v_out|^2 [nb] when the kernel that runs can emit it (the int8-sliced one);
    left empty otherwise.
    heads: {'s': (W, b, colscale|None), 't': (W, b, None), 'q': (W, b, colscale|None)};
    scales = (nw.s, nw.t, nw.q) used where no per-column scale is given.
    v_src: read the momentum from there instead (v is then only written)."""
    m, k = z.shape
    ws_, bs, cs = heads['s']
    wt, bt, _ = heads['t']
    wq, bq, cq = heads['q']
    n = ws_.shape[0]
    if _use_sliced(z, heads):
        if v_src is not None:
            assert v_src.shape == v.shape and v_src.dtype == v.dtype and v_src.is_contiguous()
        out = _sliced_call(z, heads, scales, v, force, eps, forward, False, False, 0.0, False, v_src,
                           norm2=norm2 is not None)
        if norm2 is not None:
            norm2.append(out[2])
        return out[0]
    _full_force(force)
    logdet = torch.empty(m, dtype=torch.float64, device=z.device)
    nbytes = int(N.load().l2q_vnet_heads_ws_bytes(m, n))
    ws = N.workspace(nbytes, z.device)
    if v_src is not None:
        assert v_src.shape == v.shape and v_src.dtype == v.dtype and v_src.is_contiguous()
        N.call('l2q_vnet_heads_vupdate_to_f64', z, m, k, n, ws_, bs, cs, float(scales[0]), wt, bt,
               float(scales[1]), wq, bq, cq, float(scales[2]), v_src, v, force,
               int(v.is_complex()), float(eps), int(forward), logdet, ws, ws.numel())
        return logdet
    N.call('l2q_vnet_heads_vupdate_f64', z, m, k, n, ws_, bs, cs, float(scales[0]), wt, bt,
           float(scales[1]), wq, bq, cq, float(scales[2]), v, force, int(v.is_complex()),
           float(eps), int(forward), logdet, ws, ws.numel())
    return logdet


def vnet_heads_vupdate_pair_(z: torch.Tensor, heads: dict, scales, v: torch.Tensor,
                             force: torch.Tensor, eps1: float, forward1: bool, flip: bool,
                             eps2: float, forward2: bool) -> torch.Tensor:
    """Two consecutive v-updates on the same x from one evaluation of the heads (optionally
    with v -> -v in between); returns the summed logdet [nb]."""
    m, k = z.shape
    ws_, bs, cs = heads['s']
    wt, bt, _ = heads['t']
    wq, bq, cq = heads['q']
    n = ws_.shape[0]
    if _use_sliced(z, heads):
        return _sliced_call(z, heads, scales, v, force, eps1, forward1, True, flip, eps2, forward2)[0]
    _full_force(force)
    logdet = torch.empty(m, dtype=torch.float64, device=z.device)
    ws = N.workspace(int(N.load().l2q_vnet_heads_ws_bytes(m, n)), z.device)
    N.call('l2q_vnet_heads_vupdate_pair_f64', z, m, k, n, ws_, bs, cs, float(scales[0]), wt, bt,
           float(scales[1]), wq, bq, cq, float(scales[2]), v, force, int(v.is_complex()),
           float(eps1), int(forward1), int(flip), float(eps2), int(forward2), logdet, ws,
           ws.numel())
    return logdet


def vnet_heads_vupdate_pair_mid_(z: torch.Tensor, heads: dict, scales, v: torch.Tensor,
                                 force: torch.Tensor, eps1: float, forward1: bool, flip: bool,
                                 eps2: float, forward2: bool):
    """vnet_heads_vupdate_pair_ that also returns what per-step metrics need of the momentum between
    the two updates: (logdet_sum, logdet_first, sum |v_mid|^2), each [nb]
    (include/l2q.h: l2q_vnet_heads_vupdate_pair_mid_f64; needs K % 16 == 0)."""
    m, k = z.shape
    ws_, bs, cs = heads['s']
    wt, bt, _ = heads['t']
    wq, bq, cq = heads['q']
    n = ws_.shape[0]
    if _use_sliced(z, heads):
        out = _sliced_call(z, heads, scales, v, force, eps1, forward1, True, flip, eps2, forward2, mid=True)
        return out[0], out[1], out[2]
    _full_force(force)
    out = torch.empty((3, m), dtype=torch.float64, device=z.device)
    ws = N.workspace(int(N.load().l2q_vnet_heads_ws_bytes(m, n)), z.device)
    N.call('l2q_vnet_heads_vupdate_pair_mid_f64', z, m, k, n, ws_, bs, cs, float(scales[0]), wt, bt,
           float(scales[1]), wq, bq, cq, float(scales[2]), v, force, int(v.is_complex()),
           float(eps1), int(forward1), int(flip), float(eps2), int(forward2), out[0], out[1], out[2],
           ws, ws.numel())
    return out[0], out[1], out[2]


# ---------------------------------------------------------------------------- U(1)
def u1_plaq_sums(x: torch.Tensor, lat: Sequence[int]) -> torch.Tensor:
    """[nb, 3]: sum cos(theta), sum sin(theta), sum project_angle(theta)."""
    nb = x.shape[0]
    T, X = (int(i) for i in lat)
    out = torch.empty((nb, 3), dtype=x.dtype, device=x.device)
    N.call('l2q_u1_plaq_reduce', x, nb, T, X, x.element_size(), out)
    return out


def u1_wilson_loops(x: torch.Tensor, lat: Sequence[int]) -> torch.Tensor:
    """[nb, T, X]: the plaquette angles theta (the reference's `wilson_loops` tensor)."""
    T, X = (int(i) for i in lat)
    out = torch.empty((x.shape[0], T, X), dtype=x.dtype, device=x.device)
    N.call('l2q_u1_wilson_loops', x, x.shape[0], T, X, x.element_size(), out)
    return out


def u1_wilson_loops_bwd_(dx: torch.Tensor, g: torch.Tensor, lat: Sequence[int]) -> torch.Tensor:
    """dx [nb, 2, T, X] += adjoint of the plaquette-angle map applied to g [nb, T, X]."""
    T, X = (int(i) for i in lat)
    N.call('l2q_u1_wilson_loops_bwd', g.to(dx.dtype).contiguous(), dx.shape[0], T, X, dx.element_size(), dx)
    return dx


def u1_force(x: torch.Tensor, beta: float, lat: Sequence[int]) -> torch.Tensor:
    T, X = (int(i) for i in lat)
    f = torch.empty_like(x)
    N.call('l2q_u1_force', x, float(beta), f, None, 0.0, x.shape[0], T, X, x.element_size())
    return f


def u1_force_kick_(x: torch.Tensor, beta: float, coef: float, v: torch.Tensor,
                   lat: Sequence[int]) -> torch.Tensor:
    T, X = (int(i) for i in lat)
    N.call('l2q_u1_force', x, float(beta), None, v, float(coef), x.shape[0], T, X,
           x.element_size())
    return v


def u1_x_update_(x: torch.Tensor, v: torch.Tensor, s: torch.Tensor, t: torch.Tensor,
                 q: torch.Tensor, mask: torch.Tensor, complement: bool, eps: float,
                 forward: bool, use_ncp: bool = True) -> torch.Tensor:
    nb = x.shape[0]
    n = x.numel() // nb
    logdet = torch.empty(nb, dtype=x.dtype, device=x.device)
    N.call('l2q_u1_x_update', x, v, s, t, q, mask, int(complement), float(eps), int(forward),
           int(use_ncp), x.element_size(), nb, n, logdet)
    return logdet


def u1_wrap(x: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(x)
    N.call('l2q_u1_wrap', x, out, x.numel(), x.element_size())
    return out


def u1_kinetic(v: torch.Tensor) -> torch.Tensor:
    nb = v.shape[0]
    out = torch.empty(nb, dtype=v.dtype, device=v.device)
    N.call('l2q_u1_kinetic_reduce', v, nb, v.numel() // nb, v.element_size(), out)
    return out


def u1_masked_cos_sin(x: torch.Tensor, mask: torch.Tensor, complement: bool,
                      lat: Sequence[int]) -> torch.Tensor:
    """[nb, 4, T, X]: cat([cos(m x), sin(m x)], dim=1)."""
    nb = x.shape[0]
    n = x.numel() // nb
    out = torch.empty((nb, 4, *[int(i) for i in lat]), dtype=x.dtype, device=x.device)
    N.call('l2q_u1_masked_cos_sin', x, mask, int(complement), out, nb, n, x.element_size())
    return out


def conv2d_periodic(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, pool: int = 1,
                    act: Optional[str] = None) -> torch.Tensor:
    nb, cin, H, W = x.shape
    cout, _, k, _ = w.shape
    pool = max(int(pool), 1)
    Ho, Wo = (H + k - 1) // pool, (W + k - 1) // pool
    out = torch.empty((nb, cout, Ho, Wo), dtype=torch.float32, device=x.device)
    N.call('l2q_conv2d_periodic_f32', x.float().contiguous(), w.float().contiguous(),
           b.float().contiguous(), out, nb, cin, H, W, cout, k, pool, N.ACT[act])
    return out


_CONV_SUFFIX = {torch.float32: 'f32', torch.float64: 'f64'}


def _conv_suffix(where: str, x: torch.Tensor, *others: Optional[torch.Tensor]) -> str:
    """'f32' / 'f64': the conv kernels' entry point for x.dtype.  Every other operand must have
    x's dtype (no silent casts); any other dtype is refused."""
    sfx = _CONV_SUFFIX.get(x.dtype)
    if sfx is None:
        raise N.L2QError(f'{where}: the conv kernels take float32 or float64, got {x.dtype}')
    for t in others:
        if t is not None and t.dtype != x.dtype:
            raise N.L2QError(f'{where}: dtype mismatch {t.dtype} vs input {x.dtype}')
    return sfx


def conv2d_periodic_gemm(x: torch.Tensor, layout: str, w: torch.Tensor, b: torch.Tensor,
                         pool: int = 1, act: Optional[str] = None,
                         w_clast: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PeriodicPadding(k-1) -> Conv2d(k) -> [MaxPool2d(pool)] -> [act] as implicit GEMM on
    the f32 or f64 MFMA kernel (x.dtype; w, b, w_clast alike).  x: [nb, C, H, W] if
    layout == 'nchw' else [nb, H, W, C]; returns NHWC [nb, Ho, Wo, cout].  w_clast: the weight
    as [cout, k, k, C] (used for NHWC inputs: contiguous gathers); made on the fly when not
    supplied."""
    sfx = _conv_suffix('conv2d_periodic_gemm', x, w, b, w_clast)
    x = x.contiguous()
    if layout == 'nchw':
        nb, C, H, W = x.shape
        sn, sc, sh, sw = C * H * W, H * W, W, 1
    else:
        nb, H, W, C = x.shape
        sn, sc, sh, sw = H * W * C, 1, W * C, C
    cout, cin, k, _ = w.shape
    assert cin == C
    Ho, Wo, Kc = H + k - 1, W + k - 1, C * k * k
    pool = max(int(pool), 1)
    y = torch.empty((nb * Ho * Wo, cout), dtype=x.dtype, device=x.device)
    # im2col inside the GEMM's A-tile loader: no col matrix in HBM
    clast = layout != 'nchw'
    if clast:
        wk = (w.permute(0, 2, 3, 1) if w_clast is None else w_clast).reshape(cout, Kc).contiguous()
    else:
        wk = w.reshape(cout, Kc).contiguous()
    N.call('l2q_conv_gemm_periodic_' + sfx, x, sn, sc, sh, sw, nb, C, H, W, k, wk, int(clast),
           b.contiguous(), cout, N.ACT[None if pool > 1 else act], y)
    if pool == 1:
        return y.reshape(nb, Ho, Wo, cout)
    out = torch.empty((nb, Ho // pool, Wo // pool, cout), dtype=x.dtype, device=x.device)
    N.call('l2q_maxpool_act_nhwc_' + sfx, y, nb, Ho, Wo, cout, pool, N.ACT[act], out)
    return out


def nchw_to_nhwc_pad(x: torch.Tensor, cpad: int) -> torch.Tensor:
    """fp32 / fp64 [nb, C, H, W] -> [nb, H, W, cpad] of the same dtype, channels zero-padded."""
    sfx = _conv_suffix('nchw_to_nhwc_pad', x)
    nb, C, H, W = x.shape
    out = torch.empty((nb, H, W, cpad), dtype=x.dtype, device=x.device)
    N.call('l2q_nchw_to_nhwc_pad_' + sfx, x.contiguous(), nb, C, H, W, cpad, out)
    return out


def nchw_to_nhwc_pad_h(x: torch.Tensor, hd: torch.dtype, cpad: int = 8) -> torch.Tensor:
    """fp32 [nb, C, H, W] -> 16-bit [nb, H, W, cpad], channels zero-padded."""
    nb, C, H, W = x.shape
    out = torch.empty((nb, H, W, cpad), dtype=hd, device=x.device)
    N.call('l2q_nchw_to_nhwc_pad_h', HALF_TYPES[hd], x.contiguous(), nb, C, H, W, cpad, out)
    return out


FUSE_CONV_POOL_H = [True]      # switch for A/B and the equality test (same bits either way)


def conv2d_periodic_gemm_h(x: torch.Tensor, layout: str, w16: torch.Tensor, b: torch.Tensor,
                           pool: int = 1, act: Optional[str] = None) -> torch.Tensor:
    """Half-precision PeriodicPadding(k-1) -> Conv2d(k) -> [MaxPool2d] -> [act] (include/l2q.h:
    l2q_conv_gemm_periodic_h).  x: fp32 or 16-bit, [nb, C, H, W] ('nchw') or [nb, H, W, C]
    ('nhwc'); w16: 16-bit weight, [cout, C, k, k] for 'nchw' input, [cout, k, k, C] for 'nhwc'
    input; b fp32.  Returns NHWC 16-bit."""
    x = x.contiguous()
    hd = w16.dtype
    if layout == 'nchw':
        nb, C, H, W = x.shape
        sn, sc, sh, sw = C * H * W, H * W, W, 1
        cout, cin, k, _ = w16.shape
    else:
        nb, H, W, C = x.shape
        sn, sc, sh, sw = H * W * C, 1, W * C, C
        cout, k, _, cin = w16.shape
    if cin != C or hd not in HALF_TYPES or x.dtype not in (hd, torch.float32):
        raise N.L2QError(f'conv2d_periodic_gemm_h: x {tuple(x.shape)} {x.dtype}, w {tuple(w16.shape)} {hd}')
    Ho, Wo = H + k - 1, W + k - 1
    pool = max(int(pool), 1)
    if pool == 2 and FUSE_CONV_POOL_H[0] and Ho >= 2 and Wo >= 2:
        # conv + MaxPool2d(2) + activation in one kernel: the un-pooled image never reaches HBM
        out = torch.empty((nb, Ho // 2, Wo // 2, cout), dtype=hd, device=x.device)
        N.call('l2q_conv_pool_gemm_periodic_h', HALF_TYPES[hd], x, int(x.dtype == torch.float32), sn,
               sc, sh, sw, nb, C, H, W, k, w16.reshape(cout, -1).contiguous(), int(layout != 'nchw'),
               b.contiguous(), cout, N.ACT[act], out)
        return out
    y = torch.empty((nb * Ho * Wo, cout), dtype=hd, device=x.device)
    N.call('l2q_conv_gemm_periodic_h', HALF_TYPES[hd], x, int(x.dtype == torch.float32), sn, sc, sh,
           sw, nb, C, H, W, k, w16.reshape(cout, -1).contiguous(), int(layout != 'nchw'),
           b.contiguous(), cout, N.ACT[None if pool > 1 else act], y)
    if pool == 1:
        return y.reshape(nb, Ho, Wo, cout)
    out = torch.empty((nb, Ho // pool, Wo // pool, cout), dtype=hd, device=x.device)
    N.call('l2q_maxpool_act_nhwc_h', HALF_TYPES[hd], y, nb, Ho, Wo, cout, pool, N.ACT[act], out)
    return out


def _fused_net_args(fw: dict):
    """Network part of the fused-kernel argument list, marshalled once per weight version (the
    tensors stay referenced by `fw`; device pointers are passed as plain ints)."""
    args = fw.get('_args')
    if args is None:
        hs = fw['heads']
        # pre-convert to device pointers (plain ints) on the GPU; tensors otherwise, so that the
        # missing-GPU error still comes from native.call
        p = N.ptr if fw['wxT'].is_cuda else (lambda t: t)
        args = (p(fw['wxT']), p(fw['wvT']), p(fw['b0']), p(fw['hidden']), fw['units_c'], fw['nl'],
                p(hs['s'][0]), p(hs['s'][1]), p(hs['s'][2]), p(hs['t'][0]), p(hs['t'][1]),
                float(fw['scale_t']), p(hs['q'][0]), p(hs['q'][1]), p(hs['q'][2]),
                N.ACT[fw['act']])
        fw['_args'] = args
    return args


def u1_vstep_(x: torch.Tensor, v: torch.Tensor, beta: float, eps: float, forward: bool,
              lat: Sequence[int], fw: dict, acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused force + vnet + momentum update (v in place); returns logdet [nb] (added into
    `acc` when given).  fw: the 'fused_u1' entry of LeapfrogLayer.kernel_weights()."""
    T, X = (int(i) for i in lat)
    nb = x.shape[0]
    logdet = torch.empty(nb, dtype=torch.float32, device=x.device) if acc is None else acc
    N.call('l2q_u1_vstep_f32', x, v, float(beta), float(eps), int(forward), nb, T, X,
           *_fused_net_args(fw), int(acc is not None), logdet)
    return logdet


def u1_xstep_(x: torch.Tensor, v: torch.Tensor, mask: torch.Tensor, complement: bool, eps: float,
              forward: bool, use_ncp: bool, fw: dict,
              acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused masked cos/sin + xnet + position update (x in place); returns logdet [nb] (added
    into `acc` when given)."""
    nb = x.shape[0]
    n = x.numel() // nb
    logdet = torch.empty(nb, dtype=torch.float32, device=x.device) if acc is None else acc
    N.call('l2q_u1_xstep_f32', x, v, mask, int(complement), float(eps), int(forward),
           int(use_ncp), nb, n, *_fused_net_args(fw), int(acc is not None), logdet)
    return logdet


def u1_fused_max_n() -> int:
    return int(N.load().l2q_u1_fused_max_n())


# ---------------------------------------------------------------------------- training (VJPs)
def act_fwd(x: torch.Tensor, act: Optional[str]) -> torch.Tensor:
    """act(x) (new tensor)."""
    y = torch.empty_like(x)
    N.call('l2q_act_fwd', x.contiguous(), N.ACT[act], x.numel(), x.element_size(), y)
    return y


def act_bwd(dy: torch.Tensor, y: torch.Tensor, act: Optional[str],
            from_preact: bool = False) -> torch.Tensor:
    """dy * act'(z) in place on dy.  `y` is the activation OUTPUT for every activation whose
    derivative can be written in terms of it; swish needs the PRE-activation z, and the caller must
    say so (`from_preact=True`) -- a post-activation passed for swish would give a silently wrong
    gradient, so that combination raises."""
    if N.ACT[act] == 0:
        return dy
    if (act == 'swish') != bool(from_preact):
        raise ValueError("act_bwd: swish differentiates from the pre-activation (from_preact=True), "
                         "every other activation from its output")
    N.call('l2q_act_bwd', dy, y, N.ACT[act], dy.numel(), dy.element_size(), dy)
    return dy


def act_fwd_r16(x: torch.Tensor, act: Optional[str], half: torch.dtype) -> torch.Tensor:
    """r16(act(r16(x))) on fp32 containers (new tensor), r16 = round to `half` and back: autocast's two
    rounding points around an activation, rounded like the fused epilogue of gemm_h."""
    if x.dtype != torch.float32 or half not in HALF_TYPES:
        raise N.L2QError(f'act_fwd_r16: fp32 containers and a 16-bit type, got {x.dtype} / {half}')
    x = x.contiguous()
    y = torch.empty_like(x)
    N.call('l2q_act_fwd_r16', HALF_TYPES[half], x, N.ACT[act], x.numel(), y)
    return y


def act_bwd_sums(dy: torch.Tensor, y: torch.Tensor, act: Optional[str], bgrad: torch.Tensor,
                 from_preact: bool = False) -> torch.Tensor:
    """dz = dy * act'(z) over [m, n] (new tensor) and `bgrad += colsum(dz)` in one pass; `y` and
    `from_preact` as in act_bwd."""
    if (act == 'swish') != bool(from_preact):
        raise ValueError("act_bwd_sums: swish differentiates from the pre-activation (from_preact=True), "
                         "every other activation from its output")
    m, n = dy.shape
    if y.shape != dy.shape or y.dtype != dy.dtype or bgrad.dtype != dy.dtype or bgrad.numel() != n:
        raise N.L2QError(f'act_bwd_sums: dy {tuple(dy.shape)} {dy.dtype}, y {tuple(y.shape)} {y.dtype}, '
                         f'bgrad {tuple(bgrad.shape)} {bgrad.dtype}')
    dz = torch.empty_like(dy)
    ws = N.workspace(int(N.load().l2q_colsum_ws_bytes(m, n)), dy.device)
    N.call('l2q_act_bwd_sums', dy, y, N.ACT[act], m, n, dy.element_size(), dz, bgrad, ws, ws.numel())
    return dz


def mul(a: torch.Tensor, b: torch.Tensor, alpha: float = 1.0,
        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    out = torch.empty_like(a) if out is None else out
    N.call('l2q_mul', a, b, float(alpha), a.numel(), a.element_size(), out)
    return out


def axpy_rows_(y: torch.Tensor, a: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """y[c] += a[c] * x[c]"""
    nb = y.shape[0]
    N.call('l2q_axpy_rows', x, a.to(x.dtype).contiguous(), nb, y.numel() // nb, y.element_size(), y)
    return y


def add_(y: torch.Tensor, x: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
    """y += alpha * x (float32 / float64 / complex128 as pairs of doubles, any shape)."""
    if y.is_complex():
        N.call('l2q_axpy', torch.view_as_real(x), float(alpha), torch.view_as_real(y),
               2 * y.numel(), y.element_size() // 2)
        return y
    N.call('l2q_axpy', x, float(alpha), y, y.numel(), y.element_size())
    return y


def colsum_(out: torch.Tensor, a: torch.Tensor, b: Optional[torch.Tensor] = None,
            alpha: float = 1.0, accumulate: bool = True) -> torch.Tensor:
    """out[n] (+)= alpha * sum_m a[m, n] * (b[m, n] | 1)"""
    m, n = a.shape
    ws = N.workspace(int(N.load().l2q_colsum_ws_bytes(m, n)), a.device)
    N.call('l2q_colsum', a, b, m, n, float(alpha), int(accumulate), a.element_size(), out, ws,
           ws.numel())
    return out


def scaled_tanh_bwd(ds: torch.Tensor, s: Optional[torch.Tensor], coeff: Optional[torch.Tensor],
                    scale: float) -> torch.Tensor:
    m, n = ds.shape
    dpre = torch.empty_like(ds)
    N.call('l2q_scaled_tanh_bwd', ds, s, coeff, float(scale), m, n, ds.element_size(), dpre)
    return dpre


def scaled_tanh_bwd_sums(ds: torch.Tensor, s: Optional[torch.Tensor], coeff: Optional[torch.Tensor],
                         scale: float, bgrad: torch.Tensor, cgrad: Optional[torch.Tensor],
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """scaled_tanh_bwd + `bgrad += colsum(dpre)` + (with coeff) `cgrad += colsum(ds * s)` in one pass.
    out: where dpre goes (a contiguous [m, n] slice of the tape's cotangent arena)."""
    m, n = ds.shape
    dpre = torch.empty_like(ds) if out is None else out
    if dpre.shape != ds.shape or dpre.dtype != ds.dtype or not dpre.is_contiguous():
        raise N.L2QError('scaled_tanh_bwd_sums: bad output buffer')
    ws = N.workspace(2 * int(N.load().l2q_colsum_ws_bytes(m, n)), ds.device)
    N.call('l2q_scaled_tanh_bwd_sums', ds, s, coeff, float(scale), m, n, ds.element_size(), dpre, bgrad,
           cgrad, ws, ws.numel())
    return dpre


def bn_train_fwd(x: torch.Tensor, gamma, beta, eps: float, momentum: float, running_mean,
                 running_var):
    m, n = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(n, dtype=x.dtype, device=x.device)
    invstd = torch.empty(n, dtype=x.dtype, device=x.device)
    N.call('l2q_bn_train_fwd', x, gamma, beta, float(eps), float(momentum), running_mean,
           running_var, m, n, x.element_size(), y, mean, invstd)
    return y, mean, invstd


def bn_bwd(dy, x, mean, invstd, gamma, dgamma, dbeta) -> torch.Tensor:
    m, n = x.shape
    dx = torch.empty_like(x)
    N.call('l2q_bn_bwd', dy, x, mean, invstd, gamma, m, n, x.element_size(), dx, dgamma, dbeta)
    return dx


def u1_force_bwd_(dx: torch.Tensor, x: torch.Tensor, dF: torch.Tensor, beta: float,
                  lat: Sequence[int]) -> torch.Tensor:
    T, X = (int(i) for i in lat)
    N.call('l2q_u1_force_bwd', x, dF, float(beta), x.shape[0], T, X, x.element_size(), dx)
    return dx


def u1_plaq_bwd_(dx: torch.Tensor, x: torch.Tensor, gcos: Optional[torch.Tensor],
                 gsin: Optional[torch.Tensor], lat: Sequence[int]) -> torch.Tensor:
    T, X = (int(i) for i in lat)
    gcos = None if gcos is None else gcos.to(x.dtype).contiguous()
    gsin = None if gsin is None else gsin.to(x.dtype).contiguous()
    N.call('l2q_u1_plaq_bwd', x, gcos, gsin, x.shape[0], T, X, x.element_size(), dx)
    return dx


def u1_x_update_bwd(x, v, s, t, q, mask, complement: bool, eps: float, forward: bool,
                    use_ncp: bool, gx, gl, dv):
    """-> (dx, ds, dt, dq, deps[nb]); dv accumulated in place."""
    nb = x.shape[0]
    n = x.numel() // nb
    dx, ds, dt, dq = (torch.empty_like(s) for _ in range(4))
    deps = torch.empty(nb, dtype=x.dtype, device=x.device)
    N.call('l2q_u1_x_update_bwd', x, v, s, t, q, mask, int(complement), float(eps), int(forward),
           int(use_ncp), gx, gl, x.element_size(), nb, n, dx, dv, ds, dt, dq, deps)
    return dx, ds, dt, dq, deps


def v_update_bwd(v, force, s, t, q, eps: float, forward: bool, gv, gl):
    """-> (dv, dF, ds, dt, dq, deps[nb])"""
    nb = v.shape[0]
    n = v.numel() // nb
    dv, dF, ds, dt, dq = (torch.empty_like(s) for _ in range(5))
    deps = torch.empty(nb, dtype=v.dtype, device=v.device)
    N.call('l2q_v_update_bwd', v, force, s, t, q, float(eps), int(forward), gv, gl,
           v.element_size(), nb, n, dv, dF, ds, dt, dq, deps)
    return dv, dF, ds, dt, dq, deps


def u1_masked_cos_sin_bwd_(dx, x, mask, complement: bool, dout) -> torch.Tensor:
    nb = x.shape[0]
    N.call('l2q_u1_masked_cos_sin_bwd', x, mask, int(complement), dout, nb, x.numel() // nb,
           x.element_size(), dx)
    return dx


def conv2d_periodic_gemm_train(x: torch.Tensor, layout: str, w: torch.Tensor, b: torch.Tensor,
                               pool: int = 1, act: Optional[str] = None,
                               half: Optional[torch.dtype] = None):
    """conv2d_periodic_gemm that also returns what the backward pass needs.
    half = float16 | bfloat16: the layer as torch.autocast runs it in the reference's train step -- input,
    weight and bias rounded to that type, fp32 accumulation (products of 16-bit values are exact in fp32:
    the fp32 MFMA GEMM gives what the 16-bit one gives, to summation order), the convolution's output rounded,
    the activation's output rounded; everything stays in fp32 containers for the backward pass.
    half = None: fp32 or fp64 by x.dtype (w, b alike)."""
    sfx = _conv_suffix('conv2d_periodic_gemm_train', x, w, b)
    if half is not None and x.dtype != torch.float32:
        raise N.L2QError(f'conv2d_periodic_gemm_train: half={half} expects fp32 containers, got {x.dtype}')
    x = x.contiguous()
    if half is not None:
        r16 = lambda t: t.to(half).float()
        x, w, b = r16(x), r16(w), r16(b)
    if layout == 'nchw':
        nb, C, H, W = x.shape
        strides = (C * H * W, H * W, W, 1)
    else:
        nb, H, W, C = x.shape
        strides = (H * W * C, 1, W * C, C)
    cout, cin, k, _ = w.shape
    Ho, Wo, Kc = H + k - 1, W + k - 1, C * k * k
    # NHWC input: K columns in (i, j, ci) order, so that im2col, the GEMM and col2im all move
    # contiguous runs of channels (col2im was 35 % of the conv training step in (ci, i, j) order)
    clast = layout != 'nchw'
    col = torch.empty((nb * Ho * Wo, Kc), dtype=x.dtype, device=x.device)
    N.call('l2q_im2col_periodic_' + sfx, x, *strides, nb, C, H, W, k, int(clast), col)
    pool = max(int(pool), 1)
    wk = (w.permute(0, 2, 3, 1) if clast else w).reshape(cout, Kc).contiguous()
    pre = pool == 1 and act == 'swish'
    out = None
    if pre:
        # swish is not invertible: the tape keeps the pre-activation z (16-bit valued under `half`), the
        # activation runs as a pass of its own
        y = gemm(col, wk, b.contiguous(), act=None)
        if half is not None:
            y = act_fwd_r16(y, None, half)          # rounding point between the convolution and its activation
        out = act_fwd(y, act) if half is None else act_fwd_r16(y, act, half)
    elif half is not None and pool == 1 and act is not None:
        # rounding point between the convolution and its activation
        y = act_fwd(gemm(col, wk, b.contiguous(), act=None).to(half).float(), act).to(half).float()
    else:
        y = gemm(col, wk, b.contiguous(), act=None if pool > 1 else act)
        if half is not None:
            y = y.to(half).float()
    ctx = {'col': col, 'strides': strides, 'dims': (nb, C, H, W, k, cout), 'pool': pool,
           'act': act, 'y': y, 'pre': pre, 'clast': clast, 'wk': wk}
    if pool == 1:
        out = (out if pre else y).reshape(nb, Ho, Wo, cout)
    else:
        out = torch.empty((nb, Ho // pool, Wo // pool, cout), dtype=x.dtype, device=x.device)
        N.call('l2q_maxpool_act_nhwc_' + sfx, y, nb, Ho, Wo, cout, pool, N.ACT[act], out)
        if half is not None:
            out = out.to(half).float()
    ctx['out'] = out
    return out, ctx


def conv2d_periodic_gemm_bwd(ctx: dict, dout: torch.Tensor, w: torch.Tensor, dw: torch.Tensor,
                             db: torch.Tensor, need_dx: bool = True):
    """dw, db accumulated (+=); returns dx in the layout / strides of the forward input."""
    nb, C, H, W, k, cout = ctx['dims']
    Ho, Wo, Kc = H + k - 1, W + k - 1, C * k * k
    pool, act = ctx['pool'], ctx['act']
    sfx = _conv_suffix('conv2d_periodic_gemm_bwd', dout, ctx['y'], w, dw, db)
    dout = dout.contiguous()
    if pool > 1:
        # ctx['y'] is the pre-pool GEMM output: swish differentiates at its window maximum
        dy = torch.empty_like(ctx['y'])
        N.call('l2q_maxpool_act_nhwc_bwd_' + sfx, dout, ctx['out'], ctx['y'], nb, Ho, Wo, cout, pool,
               N.ACT[act], dy)
    elif act == 'swish':
        if not ctx.get('pre'):
            raise N.L2QError('conv2d_periodic_gemm_bwd: the swish tape must hold the pre-activation')
        # the activation's VJP and the bias gradient in one pass over (dout, z)
        dy = act_bwd_sums(dout.reshape(nb * Ho * Wo, cout), ctx['y'], act, db, from_preact=True)
    else:
        dy = act_bwd(dout.reshape(nb * Ho * Wo, cout).clone(), ctx['y'], act)
    dy = dy.reshape(nb * Ho * Wo, cout)
    if pool > 1 or act != 'swish':
        colsum_(db, dy)
    clast = ctx.get('clast', False)
    dwk = gemm(t2d(dy), t2d(ctx['col']))                             # dW = dy^T col, [cout, Kc]
    if clast:                                                        # (i, j, ci) -> (ci, i, j)
        dw.add_(dwk.reshape(cout, k, k, C).permute(0, 3, 1, 2))
    else:
        add_(dw, dwk.reshape(dw.shape))
    if not need_dx:
        return None
    dcol = gemm(dy, t2d(ctx['wk'] if 'wk' in ctx else w.reshape(cout, Kc)))    # [M, Kc]
    sn, sc, sh, sw = ctx['strides']
    shape = (nb, C, H, W) if sw == 1 else (nb, H, W, C)
    dx = torch.empty(shape, dtype=dout.dtype, device=dout.device)
    N.call('l2q_col2im_periodic_' + sfx, dcol, sn, sc, sh, sw, nb, C, H, W, k, int(clast), dx)
    return dx


def adam_step_(p, g, m, v, lr: float, beta1: float, beta2: float, eps: float, step: int,
               grad_scale: float = 1.0) -> None:
    N.call('l2q_adam', p, g, m, v, p.numel(), float(lr), float(beta1), float(beta2), float(eps),
           int(step), float(grad_scale), p.element_size())


def sumsq(a: torch.Tensor) -> torch.Tensor:
    out = torch.empty(1, dtype=torch.float64, device=a.device)
    ws = N.workspace(int(N.load().l2q_sumsq_ws_bytes(a.numel())), a.device)
    N.call('l2q_sumsq', a, a.numel(), a.element_size(), out, ws, ws.numel())
    return out


# ---------------------------------------------------------------------------- SU(3) training (VJPs)
def su3_expm_mul_bwd_n(xn, vn, eps: float, mask_n, complement: bool, gxnew, gv):
    """-> (gx, deps[nb]); gv accumulated in place.  eps: the signed step of the forward call."""
    nb, _, _, V = xn.shape
    gx = torch.empty_like(xn)
    deps = torch.empty(nb, dtype=torch.float64, device=xn.device)
    ws = N.workspace(nb * 4 * ((V + 255) // 256) * 8, xn.device)
    N.call('l2q_su3_expm_mul_bwd', xn, vn, float(eps), mask_n, int(complement), gxnew, gx, gv, deps,
           nb, V, ws, ws.numel())
    return gx, deps


def su3_expm_mul2_bwd_n(xn, vn, eps: float, mask_n, complement_first: bool, gxnew, gv):
    """VJP of su3_expm_mul2_n (both half-updates, one Frechet derivative): -> (gx, deps[nb]); gv += in place."""
    nb, _, _, V = xn.shape
    gx = torch.empty_like(xn)
    deps = torch.empty(nb, dtype=torch.float64, device=xn.device)
    ws = N.workspace(nb * 4 * ((V + 255) // 256) * 8, xn.device)
    N.call('l2q_su3_expm_mul2_bwd', xn, vn, float(eps), mask_n, int(complement_first), gxnew, gx, gv, deps,
           nb, V, ws, ws.numel())
    return gx, deps


def su3_projsu_vec8_bwd_(gm: torch.Tensor, mn: torch.Tensor, gvec: torch.Tensor) -> torch.Tensor:
    """gm += VJP of su3_projsu_vec8_n at mn for the cotangent gvec [..., 8, V]."""
    V = mn.shape[-1]
    nf = mn.numel() // (9 * V)
    N.call('l2q_su3_projsu_vec8_bwd', mn, gvec.contiguous(), gm, nf, V)
    return gm


def su3_force_bwd_(gx: torch.Tensor, xn: torch.Tensor, gf: torch.Tensor, beta: float,
                   lat: Sequence[int]) -> torch.Tensor:
    T, X, Y, Z = (int(i) for i in lat)
    N.call('l2q_su3_force_bwd', xn, gf, float(beta), gx, xn.shape[0], T, X, Y, Z)
    return gx


def su3_plaq_bwd_(gx: torch.Tensor, xn: torch.Tensor, w: torch.Tensor,
                  lat: Sequence[int]) -> torch.Tensor:
    """w [nb, 6, 2] float64: complex plane weights (re, im)."""
    T, X, Y, Z = (int(i) for i in lat)
    N.call('l2q_su3_plaq_bwd', xn, w.to(torch.float64).contiguous(), gx, xn.shape[0], T, X, Y, Z)
    return gx


def su3_wilson_loops_bwd_(gx: torch.Tensor, xn: torch.Tensor, w: torch.Tensor,
                          lat: Sequence[int]) -> torch.Tensor:
    """w [6, nb, T, X, Y, Z] complex128: the cotangent of `su3_wilson_loops_n`'s output."""
    T, X, Y, Z = (int(i) for i in lat)
    N.call('l2q_su3_wilson_loops_bwd', xn, w.to(C128).contiguous(), gx, xn.shape[0], T, X, Y, Z)
    return gx


def su3_clover_bwd_(gx: torch.Tensor, xn: torch.Tensor, w: torch.Tensor,
                    lat: Sequence[int]) -> torch.Tensor:
    """gx += VJP of `su3_clover_sums_n` at xn for the cotangent w [nb, 3] float64 (`l2q_su3_clover_bwd`).  The
    kernel's per-site field (54 doubles per (chain, site)) is a tensor of its own, not the shared reduction
    workspace: at a training shape it is hundreds of MB, which the allocator should get back."""
    nb = xn.shape[0]
    T, X, Y, Z = (int(i) for i in lat)
    ws = torch.empty(nb * 54 * T * X * Y * Z, dtype=torch.float64, device=xn.device)
    N.call('l2q_su3_clover_bwd', xn, w.to(torch.float64).contiguous(), gx, nb, T, X, Y, Z, ws,
           ws.numel() * ws.element_size())
    return gx


def su3_force_vjp_(gx: torch.Tensor, xn: torch.Tensor, gf: torch.Tensor, beta: float,
                   lat: Sequence[int]) -> torch.Tensor:
    """gx += the full VJP of `su3_force_n` at xn for the cotangent gf of the force, the staples differentiated too
    (`l2q_su3_force_vjp`; `su3_force_bwd_` holds them constant)."""
    T, X, Y, Z = (int(i) for i in lat)
    N.call('l2q_su3_force_vjp', xn, gf, float(beta), gx, xn.shape[0], T, X, Y, Z)
    return gx


def su3_flow_stage_bwd_n(xn: torch.Tensor, p_out: torch.Tensor, c: float, s: float, gx_out: torch.Tensor,
                         gp: torch.Tensor, lat: Sequence[int]) -> torch.Tensor:
    """Reverse of `su3_flow_stage_n` from its input links xn and its output p_out: returns the cotangent of xn for
    the cotangent gx_out of x_out; gp (in place) is the cotangent of p_out on entry and of pn on exit."""
    nb = xn.shape[0]
    T, X, Y, Z = (int(i) for i in lat)
    gx_in = torch.empty_like(xn)
    ws = N.workspace(int(N.load().l2q_su3_flow_stage_bwd_ws_bytes(nb, T, X, Y, Z)), xn.device)
    N.call('l2q_su3_flow_stage_bwd', xn, p_out, float(c), float(s), gx_out, gp, gx_in, nb, T, X, Y, Z, ws,
           ws.numel())
    return gx_in


def su3_flow_step_bwd_n(xn: torch.Tensor, eps: float, gx_out: torch.Tensor, lat: Sequence[int],
                        gx_in: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Reverse of one `su3_flow_step_n` of size eps that started from xn: the cotangent of xn for the cotangent
    gx_out of the step's result, into gx_in (a new field by default; may be gx_out itself).  ws: a uint8 tensor of
    `l2q_su3_flow_step_bwd_ws_bytes` (seven fields and a little), its own by default: like the field of
    `su3_clover_bwd_` it is too large for the shared reduction workspace."""
    nb = xn.shape[0]
    T, X, Y, Z = (int(i) for i in lat)
    gx_in = torch.empty_like(xn) if gx_in is None else gx_in
    if ws is None:
        ws = torch.empty(int(N.load().l2q_su3_flow_step_bwd_ws_bytes(nb, T, X, Y, Z)), dtype=torch.uint8,
                         device=xn.device)
    N.call('l2q_su3_flow_step_bwd', xn, float(eps), gx_out, gx_in, nb, T, X, Y, Z, ws, ws.numel())
    return gx_in


def su3_flow_bwd_n(checkpoints: Sequence[torch.Tensor], eps: float, g_out: torch.Tensor,
                   lat: Sequence[int]) -> torch.Tensor:
    """Reverse of a Wilson flow of len(checkpoints) steps of size eps: checkpoints[k] are the native links entering
    step k, g_out the cotangent of the flowed links (only read).  Returns the cotangent of checkpoints[0]; no
    checkpoint returns g_out itself.  One workspace and one cotangent field serve all steps."""
    if len(checkpoints) == 0:
        return g_out
    nb = g_out.shape[0]
    T, X, Y, Z = (int(i) for i in lat)
    ws = torch.empty(int(N.load().l2q_su3_flow_step_bwd_ws_bytes(nb, T, X, Y, Z)), dtype=torch.uint8,
                     device=g_out.device)
    g = torch.empty_like(g_out)
    src = g_out
    for xn in reversed(checkpoints):
        su3_flow_step_bwd_n(xn, eps, src, lat, gx_in=g, ws=ws)
        src = g
    return g


def su3_rect_sums_n(xn: torch.Tensor, lat: Sequence[int]) -> torch.Tensor:
    """[nb]: sum over sites and the 12 planar 2x1 loops of Re tr R (c1 != 0 actions)."""
    nb = xn.shape[0]
    T, X, Y, Z = (int(i) for i in lat)
    out = torch.empty(nb, dtype=torch.float64, device=xn.device)
    ws = _ws(nb, T * X * Y * Z * 36, xn.device)
    N.call('l2q_su3_rect_reduce', xn, nb, T, X, Y, Z, out, ws, ws.numel())
    return out


def su3_rect_force_add_n(xn: torch.Tensor, coef: float, fn: torch.Tensor,
                         lat: Sequence[int]) -> torch.Tensor:
    """fn += coef * TAH(U * rectangle staples) in place."""
    T, X, Y, Z = (int(i) for i in lat)
    N.call('l2q_su3_rect_force_add', xn, float(coef), fn, xn.shape[0], T, X, Y, Z)
    return fn


def su3_rect_bwd_(gx: torch.Tensor, xn: torch.Tensor, w: torch.Tensor,
                  lat: Sequence[int]) -> torch.Tensor:
    """gx += w[c] * d(sum_R Re tr R)/dx;  w [nb] float64."""
    T, X, Y, Z = (int(i) for i in lat)
    N.call('l2q_su3_rect_bwd', xn, w.to(torch.float64).contiguous(), gx, xn.shape[0], T, X, Y, Z)
    return gx


def v_update_bwd_c128(v, force, s, t, q, eps: float, forward: bool, gv, gl, acc=None):
    """complex momenta: -> (dv, dF, ds, dt, dq, deps[nb]).  acc = (aF, as, at, aq): cotangents added to
    (dF, ds, dt, dq) in the same pass (the v-update that shared this one's force and heads)."""
    nb = v.shape[0]
    n = v.numel() // nb
    dv, dF = torch.empty_like(v), torch.empty_like(v)
    ds, dt, dq = (torch.empty_like(s) for _ in range(3))
    deps = torch.empty(nb, dtype=torch.float64, device=v.device)
    ws = N.workspace(nb * ((n + 255) // 256) * 8, v.device)
    if acc is not None:
        aF, as_, at, aq = acc
        N.call('l2q_v_update_bwd_acc_c128', v, force, s, t, q, float(eps), int(forward), gv, gl, nb, n,
               aF, as_, at, aq, dv, dF, ds, dt, dq, deps, ws, ws.numel())
    else:
        N.call('l2q_v_update_bwd_c128', v, force, s, t, q, float(eps), int(forward), gv, gl, nb, n, dv,
               dF, ds, dt, dq, deps, ws, ws.numel())
    return dv, dF, ds, dt, dq, deps


def v_update_bwd_pair_c128(v1, v_mid, force, s, t, q, eps1: float, forward1: bool, eps2: float, forward2: bool,
                           flip: bool, gv, gl):
    """Two v-updates that share (force, s, t, q), reversed in one pass (include/l2q.h:
    l2q_v_update_bwd_pair_c128): -> (dv, dF, ds, dt, dq, deps1[nb], deps2[nb])."""
    nb = v1.shape[0]
    n = v1.numel() // nb
    dv, dF = torch.empty_like(v1), torch.empty_like(v1)
    ds, dt, dq = (torch.empty_like(s) for _ in range(3))
    deps1 = torch.empty(nb, dtype=torch.float64, device=v1.device)
    deps2 = torch.empty_like(deps1)
    ws = N.workspace(2 * nb * ((n + 255) // 256) * 8, v1.device)
    N.call('l2q_v_update_bwd_pair_c128', v1, v_mid, force, s, t, q, float(eps1), int(forward1), float(eps2),
           int(forward2), int(flip), gv, gl, nb, n, dv, dF, ds, dt, dq, deps1, deps2, ws, ws.numel())
    return dv, dF, ds, dt, dq, deps1, deps2


def diff_bwd_(gx: torch.Tensor, x: torch.Tensor, y: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """gx += 2 a[c] (x - y) over float64 / complex128 tensors of equal shape."""
    nb = x.shape[0]
    n = x.numel() // nb * (2 if x.is_complex() else 1)
    N.call('l2q_diff_bwd_f64', x, y, a.to(torch.float64).contiguous(), nb, n, gx)
    return gx
