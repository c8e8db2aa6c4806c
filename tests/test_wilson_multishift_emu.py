"""CPU run of the kernels of csrc/su3_spinor_mshift.hip themselves: the file is compiled for the host with g++ against the
stand-in HIP header of tests/host_emu.py (every thread of a workgroup an OS thread), under AddressSanitizer and UBSan as
a stand-alone program run as a child process.  The fused multi-shift update, the residual step and the linear
combination are compared with their numpy restatements (tests/wilson_multishift_restatement.py) on 8, 24 and 320 sites,
ns 1 and 3, nb = nrhs = 2, under either block order.  Each output entry is a short chain of fma on operands of order one:
it is held to one rounding (2^-52) per operation of the sum of the sizes of its terms.  A shift that is not live keeps its
bits; the program itself refuses to finish when an input was written."""
import numpy as np
import pytest

import host_emu
import wilson_multishift_restatement as ms
import wilson_restatement as wr

NB = NRHS = 2
ULP = 2.0 ** -52


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = host_emu.build(tmp_path_factory.mktemp('spinor_mshift_emu'), 'spinor_mshift_emu')

    def run(V, ns, swz, f, c, live):
        fields = np.concatenate([f[k].reshape(-1) for k in ('x', 'ps', 'p', 'r', 'z')])
        coef = np.concatenate([c[k].reshape(-1) for k in ('a', 'b', 'zeta', 'beta', 'alpha', 'w')]
                              + [live.reshape(-1).astype(np.float64)])
        up, r2, part, lin = host_emu.run(exe, [NB * NRHS, ns, V, swz], [fields, coef], 4)
        n1, na = NB * NRHS * 12 * V, NB * NRHS * ns * 12 * V
        up = up.view(np.complex128)
        return (up[:na].reshape(f['x'].shape), up[na:2 * na].reshape(f['x'].shape), up[2 * na:].reshape(f['p'].shape),
                r2.view(np.complex128).reshape(f['r'].shape), part.reshape(NB, NRHS, -1),
                lin.view(np.complex128).reshape(f['p'].shape))
    return run


@pytest.mark.parametrize('ns', ms.KERNEL_NS)
@pytest.mark.parametrize('V', ms.KERNEL_SITES)
def test_mshift_kernels_on_the_host(emu, V, ns):
    f, c, live = ms.kernel_inputs(V, ns, NB, NRHS)
    xw, pw, bw = ms.mshift_update(f['x'], f['ps'], f['p'], f['r'], c['a'], c['b'], c['zeta'], c['beta'], live)
    rw, n2 = ms.axmy_norm(f['r'], f['z'], c['alpha'])
    lw = ms.lincomb(f['x'], c['w'])
    e = lambda v: np.abs(v)[..., None, None]                                  # noqa: E731
    first = None
    for swz in (0, 1):
        x, ps, p, r2, part, lin = got = emu(V, ns, swz, f, c, live)
        assert (np.abs(x - xw) <= ULP * (np.abs(f['x']) + e(c['a']) * np.abs(f['ps']))).all()
        assert (np.abs(ps - pw) <= 2 * ULP * (e(c['zeta']) * np.abs(f['r'])[:, :, None] + e(c['b']) * np.abs(f['ps']))).all()
        assert (np.abs(p - bw) <= ULP * (np.abs(f['r']) + e(c['beta']) * np.abs(f['p']))).all()
        assert (np.abs(r2 - rw) <= ULP * (np.abs(f['r']) + e(c['alpha']) * np.abs(f['z']))).all()
        size = sum(e(c['w'][:, :, k]) * np.abs(f['x'][:, :, k]) for k in range(ns))
        assert (np.abs(lin - lw) <= ns * ULP * size).all()
        assert part.shape[-1] == -(-V // 256)
        mine = (r2.real ** 2 + r2.imag ** 2).sum((-2, -1))                       # the partials against the kernel's own field
        assert (np.abs(part.sum(-1) - mine) <= wr.norm_bound(V) * mine).all()
        # a shift that is not live keeps its bits; a live one moved
        dead = live == 0
        assert dead.any() and np.array_equal(x[dead], f['x'][dead]) and np.array_equal(ps[dead], f['ps'][dead])
        alive = (live != 0) & (c['a'] != 0)
        assert not np.array_equal(x[alive], f['x'][alive])
        # all coefficients zero: x keeps its bits, p = r, p_k = 0, r' = r, the combination is zero
        assert np.array_equal(p[0, 0], f['r'][0, 0]) and np.array_equal(r2[0, 0], f['r'][0, 0]) and not lin[0, 0].any()
        assert np.array_equal(x[0, 0][live[0, 0] != 0], f['x'][0, 0][live[0, 0] != 0])
        assert not ps[0, 0][live[0, 0] != 0].any()
        if first is None:
            first = got
        else:                                                                    # the block order changes no bit
            assert all(np.array_equal(a, b) for a, b in zip(first, got))
