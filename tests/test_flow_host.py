"""CPU tier of the Wilson flow / clover observables: (a) the yardstick tests/flow_restatement.py against facts
that do not depend on it (the numpy oracle's force, the closed forms of uniform abelian flux, gauge invariance,
the cold start) -- these validate the ruler the GPU tests measure with; (b) the drop-in boundary of the feature:
symbols, argument errors before any HIP call, kernel names, the Python surface."""
import inspect
import math

import numpy as np
import pytest
import torch

import flow_restatement as fr
from oracle import su3 as osu3


def hot(nb, L, seed):
    rng = np.random.default_rng(seed)
    return osu3.project_su(rng.normal(size=(nb, 4, *L, 3, 3)) + 1j * rng.normal(size=(nb, 4, *L, 3, 3)))


# ------------------------------------------------------------------ (a) the yardstick
def test_yardstick_generator_is_the_oracle_force():
    """Z = -TAH(U A) = -grad_action(beta = 3) of the numpy oracle"""
    for L in ((4, 4, 4, 6), (1, 3, 2, 5), (2, 2, 2, 2)):
        x = hot(2, L, 11)
        z = fr.flow_z(torch.from_numpy(x)).numpy()
        assert np.abs(z + osu3.grad_action(x, 3.0)).max() <= 1e-13, L


@pytest.mark.parametrize('n01,n23', [(1, 1), (2, -1), (1, 0)])
def test_yardstick_flux_closed_forms(n01, n23):
    """uniform abelian flux: Q = 2 n01 n23 sinc sinc, E = 2 (sin^2 + sin^2), and a fixed point of the flow"""
    L = (4, 6, 4, 8)
    x = fr.flux_config(L, n01, n23)
    e, q = fr.clover_obs(x)
    qc, ec = fr.flux_closed_form(L, n01, n23)
    assert abs(float(q[0]) - qc) <= 1e-12 and abs(float(e[0]) - ec) <= 1e-12
    assert float(fr.flow_z(x).abs().max()) <= 1e-14
    if (n01, n23) == (1, 1):
        assert abs(float(q[0]) - 1.9645515766969974) <= 1e-12
        assert abs(float(e[0]) - 0.21009506370427466) <= 1e-12
    # the links are unitary
    assert float((fr.adj(x) @ x - torch.eye(3, dtype=fr.C128)).abs().max()) <= 1e-14


def test_yardstick_gauge_invariance():
    L = (4, 6, 4, 8)
    gen = torch.Generator().manual_seed(5)
    for x in (torch.from_numpy(hot(1, L, 3)), fr.flux_config(L, 2, -1)):
        g = fr.rand_su3((1, *L), 3.0, gen)
        e0, q0 = fr.clover_obs(x)
        e1, q1 = fr.clover_obs(fr.gauge_rotate(x, g))
        assert float((e0 - e1).abs().max()) <= 1e-12 and float((q0 - q1).abs().max()) <= 1e-12
        assert float((fr.plaq_energy(x) - fr.plaq_energy(fr.gauge_rotate(x, g))).abs().max()) <= 1e-12


def test_yardstick_cold_start():
    L = (2, 3, 4, 2)
    x = torch.eye(3, dtype=fr.C128).expand(2, 4, *L, 3, 3).contiguous()
    e, q = fr.clover_obs(x)
    assert float(e.abs().max()) == 0.0 and float(q.abs().max()) == 0.0
    assert float(fr.plaq_energy(x).abs().max()) == 0.0
    assert float(fr.flow_z(x).abs().max()) == 0.0
    assert torch.equal(fr.flow_step(x, 0.05), x)


def test_yardstick_plaquette_sum_is_the_oracle():
    x = hot(2, (3, 2, 4, 5), 2)
    s, a = fr.clover_sums(torch.from_numpy(x))
    re, _ = osu3.plaq_sums(x)
    assert np.abs(s[:, 2].numpy() - re).max() <= 1e-11
    assert bool((a >= s.abs() - 1e-9).all())


# ------------------------------------------------------------------ (b) the boundary
def test_flow_symbols_and_argument_errors():
    from l2hmc import native
    lib = native.load()
    for name in ('l2q_su3_clover_reduce', 'l2q_su3_flow_stage', 'l2q_su3_flow_step'):
        assert hasattr(lib, name) and name in native.SIGNATURES
    # (addresses are never dereferenced: every check below comes before any HIP call)
    x, p, y, w, o = 4096, 8192, 12288, 16384, 20480

    def bad(rc, text):
        assert rc == -1 and text in lib.l2q_last_error(), (rc, lib.l2q_last_error())
    bad(lib.l2q_su3_clover_reduce(None, 1, 2, 2, 2, 2, o, w, 1 << 20, None), b'null pointer')
    bad(lib.l2q_su3_clover_reduce(x, 1, 2, 2, 2, 2, None, w, 1 << 20, None), b'null pointer')
    bad(lib.l2q_su3_clover_reduce(x, 1, 2, 2, 2, 2, o, None, 1 << 20, None), b'null pointer')
    bad(lib.l2q_su3_clover_reduce(x, 0, 2, 2, 2, 2, o, w, 1 << 20, None), b'size')
    bad(lib.l2q_su3_clover_reduce(x, 1, 2, 2, 0, 2, o, w, 1 << 20, None), b'size')
    bad(lib.l2q_su3_flow_stage(None, None, 1.0, 0.1, p, y, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(lib.l2q_su3_flow_stage(x, None, 1.0, 0.1, None, y, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(lib.l2q_su3_flow_stage(x, None, 1.0, 0.1, p, None, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(lib.l2q_su3_flow_stage(x, None, 1.0, 0.1, p, y, 1, 2, -2, 2, 2, None), b'size')
    bad(lib.l2q_su3_flow_stage(x, None, 1.0, 0.1, p, x, 1, 2, 2, 2, 2, None), b'alias')
    bad(lib.l2q_su3_flow_step(None, y, p, w, 0.1, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(lib.l2q_su3_flow_step(x, None, p, w, 0.1, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(lib.l2q_su3_flow_step(x, y, None, w, 0.1, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(lib.l2q_su3_flow_step(x, y, p, None, 0.1, 1, 2, 2, 2, 2, None), b'null pointer')
    bad(lib.l2q_su3_flow_step(x, y, p, w, 0.1, 0, 2, 2, 2, 2, None), b'size')
    bad(lib.l2q_su3_flow_step(x, x, p, w, 0.1, 1, 2, 2, 2, 2, None), b'different fields')
    bad(lib.l2q_su3_flow_step(x, y, p, y, 0.1, 1, 2, 2, 2, 2, None), b'different fields')
    bad(lib.l2q_su3_flow_step(x, y, p, x, 0.1, 1, 2, 2, 2, 2, None), b'different fields')


def test_flow_kernel_names():
    """host-side dispatch of the two new entries under the default tuning (no GPU work)"""
    from l2hmc import native
    expect = {
        (8, 8, 8, 8): ('su3_clover_slice_kernel', 'su3_force_link_kernel<1, 6> + su3_expm_mul_kernel<false, false>'),
        (16, 16, 16, 16): ('su3_clover_slice_kernel', 'su3_force_link_kernel<1, 4> + su3_expm_mul_kernel<false, false>'),
        (1, 3, 2, 5): ('su3_clover_kernel', 'su3_force_tile_kernel<true, 2> + su3_expm_mul_kernel<false, false>'),
    }
    for L, names in expect.items():
        got = (native.kernel_name('l2q_su3_clover_reduce', L), native.kernel_name('l2q_su3_flow_stage', L))
        assert got == names, (L, got)


def test_flow_python_surface():
    from l2hmc import _ops as ops
    from l2hmc.lattice.su3.pytorch import lattice as lsu3
    for name in ('su3_clover_sums_n', 'su3_flow_stage_n', 'su3_flow_step_n'):
        assert callable(getattr(ops, name))
    for name in ('clover', 'clover_n', 'topological_charge', 'energy_density', 'flow', 'flow_n', 'flow_observables'):
        assert callable(getattr(lsu3.LatticeSU3, name)), name
    assert lsu3.Clover._fields == ('E', 'Q', 'Eplaq')
    sig = inspect.signature(lsu3.LatticeSU3.calc_metrics)
    assert list(sig.parameters) == ['self', 'x', 'beta', 'xinit', 'flow_time', 'flow_eps']
    assert sig.parameters['flow_time'].default is None and sig.parameters['flow_eps'].default == 0.01
    assert inspect.signature(lsu3.LatticeSU3.flow).parameters['eps'].default == 0.01
    lat = lsu3.LatticeSU3(1, [2, 2, 2, 2])
    x = torch.zeros(1, 4, 2, 2, 2, 2, 3, 3, dtype=torch.complex128)
    with pytest.raises(ValueError):
        lat.flow(x, 0.105, eps=0.01)              # t / eps is no integer
    with pytest.raises(ValueError):
        lat.energy_density(x, kind='wilson')
    with pytest.raises(RuntimeError):
        lat.flow(x.clone().requires_grad_(True), 0.1)
    with pytest.raises(RuntimeError):
        lat.clover(x.clone().requires_grad_(True))
    assert lat._flow_steps(0.3, 0.01) == 30 and lat._flow_steps(1.0, 0.01) == 100 and lat._flow_steps(0.0, 0.01) == 0
    assert math.isclose(36.0, 2 * 6 * 3)
