"""Independent restatement of the Wilson flow and the clover observables on SU(3) links: the yardstick of
tests/test_flow_host.py and tests/test_flow_gpu.py.  torch on the CPU, complex128, `torch.roll` + `@` +
`torch.matrix_exp`, written from the definitions (Luescher, arXiv:1006.4518) and from nothing in the package:
it must not import `l2hmc`, and nothing in it may be tuned to the kernels.

Fields are x[nb, 4, T, X, Y, Z, 3, 3]; `sh(f, mu, n)` is the field f[nb, T, X, Y, Z, 3, 3] at x + n mu^.
"""
import math

import torch

C128 = torch.complex128
PLANES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def sh(f, mu, n=1):
    return torch.roll(f, -n, dims=mu + 1)


def adj(m):
    return m.conj().transpose(-1, -2)


def tr(m):
    return m.diagonal(dim1=-2, dim2=-1).sum(-1)


def tah(m):
    """(M - M^H)/2 - tr(M - M^H)/6"""
    a = 0.5 * (m - adj(m))
    eye = torch.eye(3, dtype=m.dtype)
    return a - (tr(a) / 3.0)[..., None, None] * eye


def staples(x):
    """A_mu(x) = sum over nu != mu of the up and the down staple"""
    out = []
    for mu in range(4):
        a = torch.zeros_like(x[:, mu])
        for nu in range(4):
            if nu == mu:
                continue
            um, un = x[:, mu], x[:, nu]
            a = a + sh(un, mu) @ adj(sh(um, nu)) @ adj(un)
            a = a + adj(sh(sh(un, mu), nu, -1)) @ adj(sh(um, nu, -1)) @ sh(un, nu, -1)
        out.append(a)
    return torch.stack(out, 1)


def flow_z(x):
    """generator of the flow, Z(V) = -TAH(V A)"""
    return -tah(x @ staples(x))


def flow_step(x, eps):
    """one step of the third-order scheme in its textbook three-Z form"""
    z0 = eps * flow_z(x)
    w1 = torch.matrix_exp(0.25 * z0) @ x
    z1 = eps * flow_z(w1)
    w2 = torch.matrix_exp((8.0 / 9.0) * z1 - (17.0 / 36.0) * z0) @ w1
    z2 = eps * flow_z(w2)
    return torch.matrix_exp(0.75 * z2 - (8.0 / 9.0) * z1 + (17.0 / 36.0) * z0) @ w2


def flow(x, eps, nsteps):
    for _ in range(nsteps):
        x = flow_step(x, eps)
    return x


def flow_stage(x, p_in, c, s):
    """P_out = P_in + c TAH(U A), X_out = exp(s P_out) X_in (p_in None = 0)"""
    p = -c * flow_z(x)
    if p_in is not None:
        p = p_in + p
    return p, torch.matrix_exp(s * p) @ x


def leaves(x, mu, nu):
    """the four plaquette leaves of the (mu, nu) plane that start and end at x, counter-clockwise"""
    um, un = x[:, mu], x[:, nu]
    um_m, un_n = sh(um, mu, -1), sh(un, nu, -1)
    l1 = um @ sh(un, mu) @ adj(sh(um, nu)) @ adj(un)
    l2 = un @ adj(sh(um_m, nu)) @ adj(sh(un, mu, -1)) @ um_m
    l3 = adj(um_m) @ adj(sh(sh(un, mu, -1), nu, -1)) @ sh(um_m, nu, -1) @ un_n
    l4 = adj(un_n) @ sh(um, nu, -1) @ sh(sh(un, mu), nu, -1) @ adj(um)
    return l1, l2, l3, l4


def field_strength(x, mu, nu):
    l1, l2, l3, l4 = leaves(x, mu, nu)
    return 0.25 * tah(l1 + l2 + l3 + l4)


def clover_sums(x):
    """raw per-chain sums over sites, and the sums of the absolute per-site terms next to them:
    (sums [nb, 3], abs_sums [nb, 3]) with the columns
      0: sum_{mu<nu} -tr F F     1: -tr(F01 F23 - F02 F13 + F03 F12)     2: sum_{mu<nu} Re tr P"""
    nb = x.shape[0]
    f = {pl: field_strength(x, *pl) for pl in PLANES}
    e_terms = [-tr(f[pl] @ f[pl]).real for pl in PLANES]
    q_terms = [-tr(f[(0, 1)] @ f[(2, 3)]).real, tr(f[(0, 2)] @ f[(1, 3)]).real, -tr(f[(0, 3)] @ f[(1, 2)]).real]
    p_terms = [tr(leaves(x, *pl)[0]).real for pl in PLANES]

    def red(terms, absolute):
        return sum((t.abs() if absolute else t).reshape(nb, -1).sum(-1) for t in terms)
    sums = torch.stack([red(t, False) for t in (e_terms, q_terms, p_terms)], 1)
    asums = torch.stack([red(t, True) for t in (e_terms, q_terms, p_terms)], 1)
    return sums, asums


def volume(x):
    return int(x.shape[2] * x.shape[3] * x.shape[4] * x.shape[5])


def clover_obs(x):
    """(E, Q) per chain: E = -(1/V) sum tr F F, Q = -(1/4 pi^2) sum tr(F01 F23 - F02 F13 + F03 F12)"""
    s, _ = clover_sums(x)
    return s[:, 0] / volume(x), s[:, 1] / (4.0 * math.pi ** 2)


def plaq_energy(x):
    """E_plaq = 2 sum_{mu<nu} (3 - Re tr P) averaged over the sites"""
    s, _ = clover_sums(x)
    return 36.0 - 2.0 * s[:, 2] / volume(x)


def flux_config(L, n01, n23):
    """uniform abelian fluxes n01, n23 along H = diag(1, -1, 0): for (a, b) = (0, 1) and (2, 3),
    U_b(x) = exp(i phi x_a H), U_a(x_a = L_a - 1) = exp(-i phi L_a x_b H), phi = 2 pi n / (L_a L_b)"""
    L = tuple(int(i) for i in L)
    h = torch.tensor([1.0, -1.0, 0.0], dtype=torch.float64)
    ang = torch.zeros((4, *L), dtype=torch.float64)
    for (a, b), n in (((0, 1), n01), ((2, 3), n23)):
        phi = 2.0 * math.pi * n / (L[a] * L[b])
        shape_a = [1, 1, 1, 1]; shape_a[a] = L[a]
        shape_b = [1, 1, 1, 1]; shape_b[b] = L[b]
        xa = torch.arange(L[a], dtype=torch.float64).reshape(shape_a)
        xb = torch.arange(L[b], dtype=torch.float64).reshape(shape_b)
        ang[b] = ang[b] + phi * xa
        ang[a] = ang[a] + torch.where(xa == L[a] - 1, -phi * L[a] * xb, torch.zeros(()).double())
    phase = torch.exp(1j * ang[..., None] * h)                     # [4, T, X, Y, Z, 3]
    return torch.diag_embed(phase).to(C128)[None]


def flux_closed_form(L, n01, n23):
    """(Q, E) of flux_config"""
    p01 = 2.0 * math.pi * n01 / (L[0] * L[1])
    p23 = 2.0 * math.pi * n23 / (L[2] * L[3])

    def sinc(p):
        return 1.0 if p == 0.0 else math.sin(p) / p
    return 2.0 * n01 * n23 * sinc(p01) * sinc(p23), 2.0 * (math.sin(p01) ** 2 + math.sin(p23) ** 2)


def rand_su3(shape, scale, generator):
    """exp(scale TAH(normal)) for a complex Gaussian of the given leading shape: unitary to rounding"""
    m = torch.complex(torch.randn((*shape, 3, 3), dtype=torch.float64, generator=generator),
                      torch.randn((*shape, 3, 3), dtype=torch.float64, generator=generator))
    return torch.matrix_exp(scale * tah(m))


def gauge_rotate(x, g):
    """U_mu(x) -> g(x) U_mu(x) g(x + mu)^H for g[nb, T, X, Y, Z, 3, 3]"""
    return torch.stack([g @ x[:, mu] @ adj(sh(g, mu)) for mu in range(4)], 1)
