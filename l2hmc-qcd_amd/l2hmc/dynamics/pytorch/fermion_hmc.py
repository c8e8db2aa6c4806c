"""HMC with two flavours of dynamical Wilson quarks (Duane et al. 1987; Gottlieb et al. 1987): the gauge action plus
the pseudofermion action S_f = sum_r phi_r^H (M^H M)^-1 phi_r, which puts det(M^H M)^npf into the ensemble.  Built from
the lattice's kernels: the gauge force kick, `l2q_su3_wilson_force` behind a CG on M^H M, the expm link update, the
kinetic-energy reduction and the accept step.  `WilsonCloverHMC`: the same with clover-improved sea quarks
(`l2q_su3_clover_force`, the log det A_oo term).  Plain leapfrog, every solve from zero (a chronological guess would break
reversibility at a finite solver tolerance).  Not wired into `Dynamics`, the trainer or the CLI; see INTEGRATION.md,
"Dynamical Wilson fermions", for what is deliberately left out."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from l2hmc import _ops as ops
from l2hmc.lattice.su3.pytorch.lattice import LatticeSU3
from l2hmc.lattice.su3.pytorch.wilson import MIXED_INNER_TOL, MIXED_MAX_INNER, MIXED_MAX_OUTER, _MixedSolve, draw

Tensor = torch.Tensor


class WilsonHMC:
    """One trajectory: momentum and pseudofermion refresh, `nleapfrog` leapfrog steps of size `eps` under the force of
    S_g(beta) + S_f(kappa), accept / reject per chain.  The solves of the molecular dynamics stop at `tol_md`, those
    of the Hamiltonian at `tol_h`; a solve that reaches `max_iter` is counted (metrics['unconverged']), not raised.
    `even_odd` is False here and True in `WilsonHMCEvenOdd`, which runs the same trajectory on the Schur complement."""

    even_odd = False

    def __init__(self, lattice: LatticeSU3, beta: float, kappa: float, eps: float, nleapfrog: int, npf: int = 1,
                 tol_md: float = 1e-8, tol_h: float = 1e-12, max_iter: int = 2000, antiperiodic_t: bool = True) -> None:
        if not isinstance(lattice, LatticeSU3):
            raise ValueError('WilsonHMC: needs a LatticeSU3')
        vals = dict(beta=beta, kappa=kappa, eps=eps, tol_md=tol_md, tol_h=tol_h)
        for name, v in vals.items():
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not np.isfinite(v):
                raise ValueError(f'WilsonHMC: {name} must be a finite number, got {v!r}')
        if not (tol_md > 0 and tol_h > 0):
            raise ValueError(f'WilsonHMC: tol_md and tol_h must be > 0, got {tol_md!r}, {tol_h!r}')
        for name, v, lo in (('nleapfrog', nleapfrog, 1), ('npf', npf, 1), ('max_iter', max_iter, 0)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
                raise ValueError(f'WilsonHMC: {name} must be an integer >= {lo}, got {v!r}')
        self.lattice = lattice
        self.beta, self.kappa, self.eps = float(beta), float(kappa), float(eps)
        self.nleapfrog, self.npf, self.max_iter = int(nleapfrog), int(npf), int(max_iter)
        self.tol_md, self.tol_h = float(tol_md), float(tol_h)
        self.antiperiodic_t = bool(antiperiodic_t)
        if self.even_odd:
            lattice._eo_lattice('WilsonHMCEvenOdd')

    # ------------------------------------------------------------ the pieces
    def _solve_kw(self, tol: float) -> dict:
        return dict(tol=tol, max_iter=self.max_iter, antiperiodic_t=self.antiperiodic_t)

    def _kick_(self, xn: Tensor, vn: Tensor, phin: Tensor, step: float, infos: list) -> None:
        """vn -= step * (F_g + F_f), in place: the gauge kick, then the fermion kick into the same momentum"""
        lat, L = self.lattice, self.lattice._lattice_shape
        if lat.c1 == 0:
            ops.su3_force_kick_n(xn, self.beta, -step, vn, L)
        else:
            ops.axpy_(vn, lat.grad_action_n(xn, self.beta), -step)
        X, Y, info = lat._force_fields_n('pseudofermion_force', xn, phin, self.kappa, self.even_odd,
                                         **self._solve_kw(self.tol_md))
        ops.su3_wilson_force_n(xn, X, Y, self.kappa, L, self.antiperiodic_t, coef=-step, f_in=vn, out=vn)
        infos.append(info)

    def leapfrog_n(self, xn: Tensor, vn: Tensor, phin: Tensor) -> tuple[Tensor, Tensor, dict]:
        """The deterministic part, no random numbers: half kick, `nleapfrog` link updates U <- exp(eps p) U with full
        kicks between them, half kick.  Returns (x', v', info); xn, vn are not written.  info: 'cg_iters' [solves, nb,
        npf] and 'unconverged', the number of systems that reached max_iter."""
        xn, vn = xn.detach(), vn.detach().clone()
        infos: list = []
        self._kick_(xn, vn, phin, 0.5 * self.eps, infos)
        for k in range(self.nleapfrog):
            xn = ops.su3_expm_mul_n(xn, vn, self.eps)
            self._kick_(xn, vn, phin, (1.0 if k + 1 < self.nleapfrog else 0.5) * self.eps, infos)
        iters = torch.stack([i['iters'] for i in infos])
        unconv = sum(int((~i['converged']).sum()) for i in infos)
        return xn, vn, {'cg_iters': iters, 'unconverged': unconv}

    def _refresh_n(self, xn: Tensor, generator: Optional[torch.Generator]) -> tuple[Tensor, Tensor]:
        """(phi, S_f(phi) on xn) of the pseudofermion heatbath"""
        lat = self.lattice
        refresh = lat.pseudofermion_refresh_eo_n if self.even_odd else lat.pseudofermion_refresh_n
        return refresh(xn, self.kappa, self.npf, generator, self.antiperiodic_t)

    def hamiltonian_n(self, xn: Tensor, vn: Tensor, phin: Tensor, info: Optional[dict] = None) -> Tensor:
        """H [nb] = kinetic + S_g + S_f, the solve at tol_h; `info`, if given, receives the solve's info"""
        sf, sinfo = self.lattice.pseudofermion_action_n(xn, phin, self.kappa, even_odd=self.even_odd,
                                                        **self._solve_kw(self.tol_h))
        if info is not None:
            info.update(sinfo)
        return ops.su3_kinetic_n(vn) + self.lattice.action_n(xn, self.beta) + sf

    # ------------------------------------------------------------ the trajectory
    def trajectory_n(self, xn: Tensor, generator: Optional[torch.Generator] = None) -> tuple[Tensor, dict]:
        """One trajectory on a native field: (x_out, metrics).  Draws, in this order: the momentum normals
        randn((8, nb, 4, V)), the pseudofermion noise (`pseudofermion_refresh_n`; with even_odd
        `pseudofermion_refresh_eo_n`: the half shape), the accept uniforms rand(nb)."""
        lat = self.lattice
        nb = xn.shape[0]
        xn = xn.detach().contiguous()
        vn = ops.su3_assemble_tah_n(draw((8, nb, 4, lat.volume), generator, xn.device))
        phin, s0 = self._refresh_n(xn, generator)
        h0 = ops.su3_kinetic_n(vn) + lat.action_n(xn, self.beta) + s0             # S_f(phi) = |eta|^2: no solve
        x1, v1, info = self.leapfrog_n(xn, vn, phin)
        hinfo: dict = {}
        h1 = self.hamiltonian_n(x1, v1, phin, hinfo)
        u = draw((nb,), generator, xn.device, uniform=True)
        acc, mask = ops.accept(h0, h1, torch.zeros_like(h0), u)
        xo = ops.select_rows(x1.reshape(nb, -1), xn.reshape(nb, -1), mask).reshape(xn.shape)
        it = info['cg_iters'].to(torch.float64)
        metrics = {'acc': acc, 'acc_mask': mask, 'dH': h1 - h0,
                   'plaq': lat.plaq_sums_n(xo)[:, 0] / (18.0 * lat.volume),
                   'cg_iters_md': {'mean': float(it.mean()), 'max': int(it.max())},
                   'cg_iters_h': {'mean': float(hinfo['iters'].to(torch.float64).mean()),
                                  'max': int(hinfo['iters'].max())},
                   'unconverged': info['unconverged'] + int((~hinfo['converged']).sum())}
        self._more_metrics(metrics, info, hinfo)
        return xo, metrics

    def _more_metrics(self, metrics: dict, info: dict, hinfo: dict) -> None:
        """what a subclass adds to the metrics of a trajectory from the infos of its leapfrog and its Hamiltonian"""

    def trajectory(self, x: Tensor, generator: Optional[torch.Generator] = None) -> tuple[Tensor, dict]:
        """`trajectory_n` in the reference layout x[nb, 4, T, X, Y, Z, 3, 3]: momentum refresh (the `assemble_tah`
        path), pseudofermion refresh, H0 (its S_f is the refresh's |eta|^2), leapfrog, H1, accept / reject per chain.
        metrics: 'acc', 'acc_mask', 'dH', 'plaq' [nb]; 'cg_iters_md', 'cg_iters_h' (mean and max per solve);
        'unconverged', the systems that hit max_iter -- the chain is still accepted or rejected on the H it got."""
        if x.requires_grad:
            raise ValueError('WilsonHMC.trajectory: no autograd through a trajectory; detach x')
        xo, metrics = self.trajectory_n(self.lattice.pack(x), generator)
        return self.lattice.unpack(xo), metrics

    def thermalize(self, x: Tensor, ntraj: int, generator: Optional[torch.Generator] = None) -> tuple[Tensor, list]:
        """`ntraj` trajectories in a row: (x, history), history the list of their metrics"""
        if x.requires_grad:
            raise ValueError('WilsonHMC.thermalize: no autograd through a trajectory; detach x')
        xn = self.lattice.pack(x)
        history = []
        for _ in range(int(ntraj)):
            xn, m = self.trajectory_n(xn, generator)
            history.append(m)
        return self.lattice.unpack(xn), history


class WilsonHMCEvenOdd(WilsonHMC):
    """`WilsonHMC` with even-odd preconditioning (even extents; same arguments, same draw order, same metrics): the
    pseudofermion lives on the even sites, S_f = sum_r phi_e,r^H (Mhat^H Mhat)^-1 phi_e,r on the Schur complement Mhat =
    1 - kappa^2 H_eo H_oe -- the same ensemble, det Mhat = det M.  The refresh, every solve of the molecular dynamics,
    the force and `hamiltonian_n` use the Schur forms; `phin` is a half field [nb, npf, 12, V/2] and the pseudofermion
    noise is drawn with that shape."""

    even_odd = True


class WilsonHMCMixed(WilsonHMCEvenOdd):
    """`WilsonHMCEvenOdd` with every solve in mixed precision (`wilson_solve_schur_normal_mixed_n`: fp32 inner CG, fp64
    defect correction to the same stopping test): the same trajectory, draw order and metrics.  `inner_tol` and
    `max_inner` are those of the mixed solves (None: their defaults); 'cg_iters_md' and 'cg_iters_h' count the summed
    inner iterations."""

    def __init__(self, *args, inner_tol: Optional[float] = None, max_inner: Optional[int] = None, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.mixed_kw = {k: v for k, v in (('inner_tol', inner_tol), ('max_inner', max_inner)) if v is not None}
        _MixedSolve.check_args('WilsonHMCMixed', self.mixed_kw.get('inner_tol', MIXED_INNER_TOL),
                               self.mixed_kw.get('max_inner', MIXED_MAX_INNER), MIXED_MAX_OUTER)

    def _solve_kw(self, tol: float) -> dict:
        return dict(super()._solve_kw(tol), mixed=True, **self.mixed_kw)


class WilsonCloverHMC(WilsonHMCEvenOdd):
    """`WilsonHMCEvenOdd` with O(a)-improved (Sheikholeslami-Wohlert) sea quarks at the clover coefficient `c_sw`, in the
    asymmetric even-odd form (Jansen & Liu 1997; same draw order, same metrics):
        S_f = sum_r phi_e,r^H (Mhat^H Mhat)^-1 phi_e,r - 2 npf log det A_oo,   Mhat = A_ee - kappa^2 H_eo A_oo^-1 H_oe,
    which puts det(M_sw^H M_sw)^npf into the ensemble.  One `clover_term_n` per kick and per Hamiltonian, shared by the
    solve, the completion hops and `l2q_su3_clover_force`; both fermion kicks go in place into the momentum.  The
    determinant term is part of `hamiltonian_n` and of H0.  A clover term that is not positive definite raises (the
    ValueError of `LatticeSU3.wilson_clover_solve_n`, naming chain and pivot).  Double precision only."""

    def __init__(self, lattice: LatticeSU3, beta: float, kappa: float, c_sw: float, eps: float, nleapfrog: int,
                 **kwargs) -> None:
        super().__init__(lattice, beta, kappa, eps, nleapfrog, **kwargs)
        if isinstance(c_sw, bool) or not isinstance(c_sw, (int, float, np.floating, np.integer)) or not np.isfinite(c_sw):
            raise ValueError(f'WilsonCloverHMC: c_sw must be a finite number, got {c_sw!r}')
        self.c_sw = float(c_sw)

    def _clover(self, xn: Tensor):
        """the clover term of xn, positive definite or ValueError"""
        lat = self.lattice
        return lat._clover_for('WilsonCloverHMC', xn, self.kappa, self.c_sw, lat.clover_term_n(xn, self.kappa, self.c_sw))

    def _kick_(self, xn: Tensor, vn: Tensor, phin: Tensor, step: float, infos: list) -> None:
        """vn -= step * (F_g + F_f), in place: the gauge kick, then the hop and the clover part of the fermion kick"""
        lat, L = self.lattice, self.lattice._lattice_shape
        if lat.c1 == 0:
            ops.su3_force_kick_n(xn, self.beta, -step, vn, L)
        else:
            ops.axpy_(vn, lat.grad_action_n(xn, self.beta), -step)
        cl = self._clover(xn)
        X, Y, info = lat._clover_force_fields_n(xn, phin, self.kappa, self.c_sw, cl, **self._solve_kw(self.tol_md))
        ops.su3_wilson_force_n(xn, X, Y, self.kappa, L, self.antiperiodic_t, coef=-step, f_in=vn, out=vn)
        ops.su3_clover_force_n(xn, X, Y, cl.ainv, self.kappa * self.c_sw, L, det_weight=self.npf, coef=-step, f_in=vn,
                               out=vn)
        infos.append(info)

    def hamiltonian_n(self, xn: Tensor, vn: Tensor, phin: Tensor, info: Optional[dict] = None) -> Tensor:
        """H [nb] = kinetic + S_g + S_f with its determinant term, the solve at tol_h"""
        sf, sinfo = self.lattice.clover_pseudofermion_action_n(xn, phin, self.kappa, self.c_sw, self._clover(xn),
                                                               **self._solve_kw(self.tol_h))
        if info is not None:
            info.update(sinfo)
        return ops.su3_kinetic_n(vn) + self.lattice.action_n(xn, self.beta) + sf

    def _refresh_n(self, xn: Tensor, generator: Optional[torch.Generator]) -> tuple[Tensor, Tensor]:
        """(phi_e, S_f(phi_e) on xn): the heatbath's |eta_e|^2 plus the determinant term -- one clover term, no solve"""
        lat = self.lattice
        cl = self._clover(xn)
        phin, s0 = lat.clover_pseudofermion_refresh_n(xn, self.kappa, self.c_sw, self.npf, generator, self.antiperiodic_t,
                                                      cl)
        return phin, s0 + lat._clover_logdet_part(cl, self.npf)


class WilsonRHMC(WilsonHMCEvenOdd):
    """HMC with ONE flavour of Wilson quarks at `kappa` by the rational action S_1 = sum_r phi_e,r^H R(Mhat^H Mhat) phi_e,r
    (`LatticeSU3.rhmc_pseudofermion_action_n`; `rat` = `rational.zolotarev_inv_sqrt(n, ra, rb)`, whose interval must hold
    the spectrum of Mhat^H Mhat along the trajectory: `LatticeSU3.schur_spectrum_n`), every solve a multi-shift CG.  With
    `kappa_light` it also carries the two-flavour even-odd pseudofermion of `WilsonHMCEvenOdd` at that hopping parameter:
    N_f = 2 + 1.  The ensemble weight of the one flavour is det R^-1, |det M| up to the relative error rat.delta of R; no
    reweighting is done.  Draw order of a trajectory: the momentum normals, the light pseudofermion noise (if any), then
    the strange one, then the accept uniforms.  The fermion kicks go in place into the momentum in the same order, light
    then strange.  `phin` is the pair (phi_light or None, phi_strange), each [nb, npf, 12, V/2].  Metrics: those of the
    parent -- 'cg_iters_md' and 'cg_iters_h' count the light solves where there are any, else the multi-shift ones --
    plus 'cg_iters_ms_md' and 'cg_iters_ms_h' for the multi-shift solves.  Double precision, plain Wilson only."""

    def __init__(self, lattice: LatticeSU3, beta: float, kappa: float, eps: float, nleapfrog: int, *, rat,
                 kappa_light: Optional[float] = None, **kwargs) -> None:
        super().__init__(lattice, beta, kappa, eps, nleapfrog, **kwargs)
        lattice._rat_checks('WilsonRHMC', rat)
        if kappa_light is not None and (isinstance(kappa_light, bool) or not np.isfinite(kappa_light)):
            raise ValueError(f'WilsonRHMC: kappa_light must be a finite number or None, got {kappa_light!r}')
        self.rat = rat
        self.kappa_light = None if kappa_light is None else float(kappa_light)

    def _kick_(self, xn: Tensor, vn: Tensor, phin, step: float, infos: list) -> None:
        """vn -= step * (F_g + F_light + F_strange), in place, in that order; infos receives the light solve's info (if
        any), then the multi-shift solve's"""
        lat, L = self.lattice, self.lattice._lattice_shape
        if lat.c1 == 0:
            ops.su3_force_kick_n(xn, self.beta, -step, vn, L)
        else:
            ops.axpy_(vn, lat.grad_action_n(xn, self.beta), -step)
        phi_l, phi_s = phin
        if phi_l is not None:
            X, Y, info = lat._force_fields_n('pseudofermion_force', xn, phi_l, self.kappa_light, True,
                                             **self._solve_kw(self.tol_md))
            ops.su3_wilson_force_n(xn, X, Y, self.kappa_light, L, self.antiperiodic_t, coef=-step, f_in=vn, out=vn)
            infos.append(info)
        X, Y, ms = lat._rhmc_force_fields_n(xn, phi_s, self.kappa, self.rat, **self._solve_kw(self.tol_md))
        ops.su3_wilson_force_n(xn, X, Y, self.kappa, L, self.antiperiodic_t, coef=-step, f_in=vn, out=vn)
        infos.append(ms)

    def leapfrog_n(self, xn: Tensor, vn: Tensor, phin) -> tuple[Tensor, Tensor, dict]:
        """`WilsonHMC.leapfrog_n`; info['unconverged'] counts the systems of every solve, light and multi-shift;
        info['cg_iters_ms'] [kicks, nb, npf] are the multi-shift solves' iterations and info['cg_iters'] the light
        solves' where there is a light field, else the same multi-shift ones"""
        x1, v1, info = super().leapfrog_n(xn, vn, phin)
        if phin[0] is not None:                      # the kicks appended light, multi-shift, light, ...
            info['cg_iters'], info['cg_iters_ms'] = info['cg_iters'][0::2], info['cg_iters'][1::2]
        else:
            info['cg_iters_ms'] = info['cg_iters']
        return x1, v1, info

    def _refresh_n(self, xn: Tensor, generator: Optional[torch.Generator]):
        """((phi_light or None, phi_strange), S_f on xn): the light heatbath first, then the strange one"""
        lat = self.lattice
        phi_l, s0 = None, 0.0
        if self.kappa_light is not None:
            phi_l, s0 = lat.pseudofermion_refresh_eo_n(xn, self.kappa_light, self.npf, generator, self.antiperiodic_t)
        phi_s, s1 = lat.rhmc_pseudofermion_refresh_n(xn, self.kappa, self.rat, self.npf, generator, self.antiperiodic_t,
                                                     tol=self.tol_h, max_iter=self.max_iter)
        return (phi_l, phi_s), s0 + s1

    def hamiltonian_n(self, xn: Tensor, vn: Tensor, phin, info: Optional[dict] = None) -> Tensor:
        """H [nb] = kinetic + S_g + S_light + S_1, the solves at tol_h; `info`, if given, receives the light solve's info
        (without a light field: the multi-shift solve's) and under 'multishift' the multi-shift solve's"""
        lat = self.lattice
        phi_l, phi_s = phin
        sf, ms = lat.rhmc_pseudofermion_action_n(xn, phi_s, self.kappa, self.rat, **self._solve_kw(self.tol_h))
        sinfo = ms
        if phi_l is not None:
            sl, sinfo = lat.pseudofermion_action_n(xn, phi_l, self.kappa_light, even_odd=True,
                                                   **self._solve_kw(self.tol_h))
            sf = sl + sf
        if info is not None:
            info.update(sinfo)
            info['multishift'] = ms
        return ops.su3_kinetic_n(vn) + lat.action_n(xn, self.beta) + sf

    def _more_metrics(self, metrics: dict, info: dict, hinfo: dict) -> None:
        ms = hinfo['multishift']
        for key, it in (('cg_iters_ms_md', info['cg_iters_ms']), ('cg_iters_ms_h', ms['iters'])):
            it = it.to(torch.float64)
            metrics[key] = {'mean': float(it.mean()), 'max': int(it.max())}
        if self.kappa_light is not None:             # the parent counted the light solve of the Hamiltonian only
            metrics['unconverged'] += int((~ms['converged']).sum())
