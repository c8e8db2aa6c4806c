"""The Hamiltonian's terms as by-products of the kernels that hold them: the plaquette sum out of the link force
kernel (l2q_su3_force_action), sum |v_out|^2 out of the single-update sliced heads kernel, sum |v|^2 out of the
momentum assembly (l2q_su3_assemble_tah_norm2).  In each case the primary output keeps its bits and the sum agrees
with the oracle / numpy; two runs give the same bits."""
import numpy as np
import pytest
import torch

from oracle import su3 as osu3

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from l2hmc import _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def err(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())


_CONFIGS = {}


def _config(L, nb, start):
    """(x, oracle sum Re tr P): hot = projectSU of Gaussian matrices; near = projectSU(1 + 0.05 Gaussian), where
    every plaquette has Re tr P ~ 3 -- all terms of one sign, the sums at their largest"""
    key = (L, nb, start)
    if key not in _CONFIGS:
        rng = np.random.default_rng(17)
        z = rng.normal(size=(nb, 4, *L, 3, 3)) + 1j * rng.normal(size=(nb, 4, *L, 3, 3))
        if start == 'near':
            z = 0.05 * z
            z[..., range(3), range(3)] += 1.0
        x = osu3.project_su(z)
        _CONFIGS[key] = (x, osu3.plaq_sums(x)[0])
    return _CONFIGS[key]


# (lattice, chains): the smallest lattice on the link kernel (in-LDS mask 0), odd T with uneven t-chunks, mask 6,
# mask 4, and a lattice the link kernel does not serve (the ordinary force, then the plaquette reduction)
FORCE_CASES = [((2, 4, 4, 12), 3), ((3, 4, 4, 12), 3), ((8, 8, 8, 8), 2), ((16, 16, 16, 16), 1), ((3, 5, 2, 7), 2)]


@pytest.mark.parametrize('start', ['hot', 'near'])
@pytest.mark.parametrize('L,nb', FORCE_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_force_action(ops, L, nb, start):
    """tolerance of the sum: what tests/test_kernels_gpu.py::test_su3_stencils_vs_oracle applies to
    l2q_su3_plaq_reduce against the same oracle (1e-10, absolute)"""
    from l2hmc import native
    x, re = _config(L, nb, start)
    xn = ops.su3_pack(dev(x))
    f0 = ops.su3_force_n(xn, 5.7, L)
    f, plaq = ops.su3_force_action_n(xn, 5.7, L)
    name = native.kernel_name('l2q_su3_force_action', L)
    assert ('su3_force_link_action_kernel' in name) == (L != (3, 5, 2, 7)), name
    assert torch.equal(f, f0)
    d = err(host(plaq), re)
    two = err(host(ops.su3_plaq_sums_n(xn, L))[:, 0], re)
    print(f'{L} {start}: |action sum - oracle| = {d:.3e} (plaq_reduce: {two:.3e}), |sum| = {np.abs(re).max():.6e}')
    f2, plaq2 = ops.su3_force_action_n(xn, 5.7, L)
    assert torch.equal(f2, f) and torch.equal(plaq2, plaq)
    assert d < 1e-10


def test_force_action_other_force_designs(ops):
    """force_tile 2 and 7 at 8^4: the entry point runs that force and the plaquette reduction"""
    from l2hmc import native
    L, nb = (8, 8, 8, 8), 2
    x, re = _config(L, nb, 'hot')
    xn = ops.su3_pack(dev(x))
    try:
        for ft in (2, 7):
            native.set_tuning('force_tile', ft)
            assert 'action' not in native.kernel_name('l2q_su3_force_action', L)
            f, plaq = ops.su3_force_action_n(xn, 5.7, L)
            assert torch.equal(f, ops.su3_force_n(xn, 5.7, L))
            assert torch.equal(plaq, ops.su3_plaq_sums_n(xn, L)[:, 0])
            assert err(host(plaq), re) < 1e-10
    finally:
        native.set_tuning('force_tile', 5)


def _heads(rng, n, k):
    scaled = {}
    for nm in 'stq':
        w = dev(rng.uniform(-1, 1, size=(n, k)) / 16)
        b = dev(0.1 * rng.normal(size=n))
        c = None if nm == 't' else dev(np.exp(0.3 * rng.normal(size=n)))
        scaled[nm] = (w, b, c)
    return scaled


# (M, N, complex): padding rows; a second row group that is mostly padding; real momenta with padding columns
# (N % 16 != 0); fewer 16-column tiles than column workers (the workers without a tile must report 0)
HEADS_CASES = [(3, 576, True), (65, 576, True), (16, 1000, False), (16, 48, True)]


@pytest.mark.parametrize('m,n,cplx', HEADS_CASES)
def test_heads_sliced_vnorm2_out(ops, m, n, cplx):
    """tolerance of the sum: that of the mid-point sum |v|^2 in tests/test_kernels_gpu.py (1e-12, relative to the
    largest sum)"""
    k = 256
    rng = np.random.default_rng(23)
    z = dev(np.tanh(rng.normal(size=(m, k))))
    sl = _heads(rng, n, k)
    sl['sliced'] = ops.heads_sliced_build(sl)
    assert sl['sliced'] is not None and ops.USE_SLICED_HEADS[0]
    nw = (0.9, 1.1, 0.8)
    if cplx:
        v = dev(rng.normal(size=(m, n)) + 1j * rng.normal(size=(m, n)))
        f = dev(rng.normal(size=(m, n)) + 1j * rng.normal(size=(m, n)))
    else:
        v = dev(rng.normal(size=(m, n)))
        f = dev(rng.normal(size=(m, n)))
    for fwd in (True, False):
        va = v.clone()
        la = ops.vnet_heads_vupdate_(z, sl, nw, va, f, 0.07, fwd)
        for src in (None, v.clone()):                      # in place, out of place
            vb = v.clone() if src is None else torch.full_like(v, float('nan'))
            got = []
            lb = ops.vnet_heads_vupdate_(z, sl, nw, vb, f, 0.07, fwd, v_src=src, norm2=got)
            assert torch.equal(vb, va) and torch.equal(lb, la)
            assert len(got) == 1 and got[0].shape == (m,)
            want = (np.abs(host(va)).astype(np.float64) ** 2).sum(1)
            d = err(host(got[0]), want)
            print(f'M {m} N {n} complex {cplx} forward {fwd}: |sum - numpy| = {d:.3e}, max sum {want.max():.6e}')
            assert d < 1e-12 * max(1.0, float(np.abs(want).max()))
            again = []
            vc = v.clone() if src is None else torch.full_like(v, float('nan'))
            ops.vnet_heads_vupdate_(z, sl, nw, vc, f, 0.07, fwd, v_src=src, norm2=again)
            assert torch.equal(again[0], got[0]) and torch.equal(vc, vb)
    # the fp64 heads kernel does not emit the sum: the list stays empty and the caller takes the separate pass
    fp = {nm: sl[nm] for nm in 'stq'}
    none = []
    ops.vnet_heads_vupdate_(z, fp, nw, v.clone(), f, 0.07, True, norm2=none)
    assert none == []


@pytest.mark.parametrize('nb,V', [(1, 1), (3, 255), (2, 257), (2, 1024), (5, 700)])
def test_assemble_tah_norm2(ops, nb, V):
    """block edges of the 256-site blocks (V = 1, 255, 257, whole blocks, several chains); the sum against numpy
    with the tolerance of the heads' sums (1e-12, relative to the largest sum)"""
    rng = np.random.default_rng(29)
    nrm = dev(rng.normal(size=(8, nb, 4, V)))
    v0 = ops.su3_assemble_tah_n(nrm)
    v, n2 = ops.su3_assemble_tah_norm2_n(nrm)
    assert torch.equal(v, v0)
    want = (np.abs(host(v0)) ** 2).reshape(nb, -1).sum(1)
    d = err(host(n2), want)
    print(f'nb {nb} V {V}: |sum - numpy| = {d:.3e}, max sum {want.max():.6e}')
    assert d < 1e-12 * max(1.0, float(want.max()))
    # the kinetic energy l2q_su3_kinetic_reduce gives for these momenta
    ke = host(ops.su3_kinetic_n(v0))
    assert err(0.5 * (host(n2) - 32.0 * V), ke) < 1e-12 * max(1.0, float(want.max()))     # (of the sum: ke cancels)
    v2, n22 = ops.su3_assemble_tah_norm2_n(nrm)
    assert torch.equal(v2, v) and torch.equal(n22, n2)
