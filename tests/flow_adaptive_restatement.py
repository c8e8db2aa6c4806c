"""Independent restatement of one Wilson-flow step with its embedded error estimate (Fritzsch & Ramos,
arXiv:1301.4388, App. D): the yardstick of tests/test_flow_adaptive_*.py.  torch on the CPU, on top of
tests/flow_restatement.py and nothing from the package: it must not import `l2hmc`, and nothing in it may be tuned to
the kernels.

The third-order step in its textbook three-Z form, and from the same Z0, Z1 the second-order result
W' = exp(-Z0 + 2 Z1) W0; d_c = max over mu, x of |W3 - W'|_F / 9 (9 = N^2).
"""
import torch

import flow_restatement as fr


def link_distance(a, b):
    """[nb]: max over the chain's links of |a - b|_F / 9 for fields [nb, 4, ..., 3, 3]"""
    n = torch.linalg.matrix_norm(a - b) / 9.0
    return n.reshape(n.shape[0], -1).amax(-1)


def flow_step_err(x, eps):
    """(W3, d [nb]) of one step of size eps"""
    z0 = eps * fr.flow_z(x)
    w1 = torch.matrix_exp(0.25 * z0) @ x
    z1 = eps * fr.flow_z(w1)
    w2 = torch.matrix_exp((8.0 / 9.0) * z1 - (17.0 / 36.0) * z0) @ w1
    z2 = eps * fr.flow_z(w2)
    w3 = torch.matrix_exp(0.75 * z2 - (8.0 / 9.0) * z1 + (17.0 / 36.0) * z0) @ w2
    wp = torch.matrix_exp(-z0 + 2.0 * z1) @ x
    return w3, link_distance(w3, wp)


def last_kernel(w0, w2, p1, p2, p3, eps):
    """what the step's last kernel makes of the fields it reads, in the low-storage generators P1 = G0,
    P2 = P1 - 32/17 G1, P3 = P2 + 27/17 G2 (G = -Z / eps): W3 = exp(-17 eps/36 P3) W2, W' = exp(eps/16 (17 P2 - P1)) W0
    -> (W3, d [nb]); fields [nb, 4, V, 3, 3]"""
    w3 = torch.matrix_exp((-17.0 * eps / 36.0) * p3) @ w2
    wp = torch.matrix_exp((eps / 16.0) * (17.0 * p2 - p1)) @ w0
    return w3, link_distance(w3, wp)


def rand_tah(shape, scale, generator):
    """scale TAH(normal): anti-Hermitian traceless matrices of the given leading shape"""
    m = torch.complex(torch.randn((*shape, 3, 3), dtype=torch.float64, generator=generator),
                      torch.randn((*shape, 3, 3), dtype=torch.float64, generator=generator))
    return scale * fr.tah(m)
