"""CPU run of the kernels of csrc/su3_flow_adaptive.hip themselves: the file is compiled for the host with g++ against
the stand-in HIP header of tests/host_emu.py (every thread of a workgroup an OS thread), under
AddressSanitizer and UBSan as a stand-alone program run as a child process, and the step's last kernel (W3, and the
distance d to the embedded second-order result) is compared with tests/flow_adaptive_restatement.py.  Catches indexing,
reduction and out-of-bounds mistakes without a GPU: V = 16 and 30 are a partial wavefront, 210 a partial block, 256 one
whole block, 384 one and a half."""
import numpy as np
import pytest
import torch

import flow_adaptive_restatement as far
import flow_restatement as fr
import host_emu
from native_layout import pack, unpack

NB = 3
EPS = 0.02
SIZES = [16, 30, 210, 256, 384]


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = host_emu.build(tmp_path_factory.mktemp('flow_adaptive_emu'), 'flow_adaptive_emu')

    def run(V, fields):
        """fields: five x[nb, 4, V, 3, 3] (torch); returns W3 in the same shape (numpy) and d [nb]"""
        x, d = host_emu.run(exe, [NB, V, repr(EPS)], [pack(f) for f in fields], 2)
        return unpack(x.view(np.complex128).reshape(NB, 4, 9, V), (V,)), d
    return run


def fields(V, seed):
    """(W0, W2, P1, P2, P3): links and anti-Hermitian traceless generators of the size a flow step meets"""
    g = torch.Generator().manual_seed(seed)
    return [fr.rand_su3((NB, 4, V), 1.0, g), fr.rand_su3((NB, 4, V), 1.0, g), far.rand_tah((NB, 4, V), 2.0, g),
            far.rand_tah((NB, 4, V), 2.0, g), far.rand_tah((NB, 4, V), 2.0, g)]


def test_argument_errors_of_the_library():
    from l2hmc import native
    lib = native.load()
    L = (2, 2, 2, 2)
    field = 36 * 16 * 16                           # bytes of a field of one chain
    assert lib.l2q_su3_flow_step_err_ws_bytes(1, *L) == 4 * 8 and lib.l2q_su3_flow_step_err_ws_bytes(3, 4, 4, 4, 5) \
        == 3 * 4 * 2 * 8
    assert lib.l2q_su3_flow_step_err_ws_bytes(0, *L) == 0 and lib.l2q_su3_flow_step_err_ws_bytes(1, 2, 0, 2, 2) == 0
    mb = 1 << 20                                   # any non-null addresses: the checks come before every use of them
    ok = dict(x_in=mb, x_out=2 * mb, p3=4 * mb, ws_x=3 * mb, d=5 * mb, nb=1, Z=2, ws=6 * mb, ws_bytes=32)

    def call(**kw):
        a = {**ok, **kw}
        return lib.l2q_su3_flow_step_err(a['x_in'], a['x_out'], a['p3'], a['ws_x'], 0.01, a['d'], a['nb'], 2, 2, 2,
                                         a['Z'], a['ws'], a['ws_bytes'], None)
    for kw in (dict(x_in=None), dict(x_out=None), dict(p3=None), dict(ws_x=None), dict(d=None), dict(ws=None),
               dict(nb=0), dict(Z=0), dict(x_out=mb), dict(ws_x=mb), dict(ws_x=2 * mb),
               dict(x_in=4 * mb), dict(x_out=4 * mb + field), dict(ws_x=4 * mb + 3 * field - 16)):
        assert call(**kw) == -1, kw                                        # L2Q_EINVAL
    assert b'l2q_su3_flow_step_err' in lib.l2q_last_error()
    assert call(ws_bytes=31) == -2                                         # L2Q_ESHAPE
    assert b'workspace' in lib.l2q_last_error()


@pytest.mark.parametrize('V', SIZES)
def test_last_kernel_on_the_host(emu, V):
    f = fields(V, 100 + V)
    want_x, want_d = far.last_kernel(*f, EPS)
    got_x, got_d = emu(V, f)                                   # (the program itself fails if an input was written)
    ex = np.abs(got_x - want_x.numpy()).max()
    ed = np.abs(got_d - want_d.numpy()).max()
    print(f'V = {V}: |dW3| = {ex:.2e}, |dd| = {ed:.2e}, d = {want_d.tolist()}')
    assert ex <= 1e-13 and ed <= 1e-13
    assert (want_d > 1e-3).all()                               # the distance compared is far above the tolerance
    # one NaN in one link of one chain: that chain reports +inf, the others the same bits as before
    for which, chain, mu, site in ((2, 1, 3, V - 1), (0, 2, 0, 0), (1, 0, 2, V // 2), (4, 1, 1, V // 3)):
        bad = [t.clone() for t in f]
        bad[which][chain, mu, site, 1, 2] = complex(float('nan'), 0.0)
        _, d = emu(V, bad)
        assert d[chain] == np.inf, (which, d)
        others = [c for c in range(NB) if c != chain]
        assert np.array_equal(d[others], got_d[others]), (which, d, got_d)
