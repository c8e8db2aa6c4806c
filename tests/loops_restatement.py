"""Independent restatement of straight lines of SU(3) links, planar R x T Wilson loops and Polyakov loops: the
yardstick of tests/test_loops_host.py and tests/test_loops_gpu.py.  torch on the CPU, complex128, `torch.roll` and
`@`, written from the definitions and from nothing in the package: it must not import `l2hmc`, and nothing in it
may be tuned to the kernels.

Fields are x[nb, 4, T, X, Y, Z, 3, 3]; `sh(f, mu, n)` is the field f[nb, T, X, Y, Z, 3, 3] at x + n mu^.
  line:  L_mu(x, n) = U_mu(x) U_mu(x + mu) ... U_mu(x + (n-1) mu), a field shaped like the links
  loop:  W_{mu nu}(x) = A_mu(x) B_nu(x + r mu) A_mu(x + t nu)^H B_nu(x)^H for line fields A (length r), B (length t)
  Polyakov loop: P_mu(x_perp) = tr L_mu(x with x_mu = 0, N_mu)
"""
import torch

from flow_restatement import adj, flux_config, gauge_rotate, rand_su3, sh, tr  # noqa: F401

PAIRS = [(mu, nu) for mu in range(4) for nu in range(4) if nu != mu]


def pair_index(mu, nu):
    return 3 * mu + (nu if nu < mu else nu - 1)


def line(x, n):
    """the lines of length n >= 1 in all four directions"""
    out = []
    for mu in range(4):
        m = x[:, mu]
        for k in range(1, n):
            m = m @ sh(x[:, mu], mu, k)
        out.append(m)
    return torch.stack(out, 1)


def loop_traces(a, r, b, t):
    """tr W_{mu nu}(x) for the 12 ordered pairs: [12, nb, T, X, Y, Z], in the order of PAIRS"""
    return torch.stack([tr(a[:, mu] @ sh(b[:, nu], mu, r) @ adj(sh(a[:, mu], nu, t)) @ adj(b[:, nu]))
                        for mu, nu in PAIRS])


def loop_sums(a, r, b, t):
    """(sums [nb, 12] complex, S [nb, 12] = sum over sites of |tr W|, the scale for tolerances)"""
    w = loop_traces(a, r, b, t)
    nb = w.shape[1]
    return w.reshape(12, nb, -1).sum(-1).T.contiguous(), w.abs().reshape(12, nb, -1).sum(-1).T.contiguous()


def loop_table_sums(x, rmax, tmax):
    """(sums [nb, rmax, tmax, 12], S alike): entry [R-1, T-1] from the lines of lengths R and T"""
    lines = {n: line(x, n) for n in range(1, max(rmax, tmax) + 1)}
    rows = [[loop_sums(lines[r], r, lines[t], t) for t in range(1, tmax + 1)] for r in range(1, rmax + 1)]
    return (torch.stack([torch.stack([c[0] for c in row], 1) for row in rows], 1),
            torch.stack([torch.stack([c[1] for c in row], 1) for row in rows], 1))


def polyakov(x, mu):
    """tr of the line that closes around direction mu, per perpendicular site: [nb, *perp] (not divided by 3)"""
    n = x.shape[2 + mu]
    return tr(line(x, n)[:, mu].select(mu + 1, 0))


def polyakov_correlator(p):
    """C(r) = (1 / V_perp) sum_y Re P(y) conj P(y + r) for p[nb, n1, n2, n3], by one roll per displacement"""
    out = torch.empty(p.shape, dtype=torch.float64)
    vp = p[0].numel()
    for i in range(p.shape[1]):
        for j in range(p.shape[2]):
            for k in range(p.shape[3]):
                q = torch.roll(p, (-i, -j, -k), dims=(1, 2, 3))
                out[:, i, j, k] = (p * q.conj()).real.reshape(p.shape[0], -1).sum(-1) / vp
    return out
