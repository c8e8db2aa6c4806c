"""CPU tier of the upper-plane force (include/l2q.h: l2q_su3_force_upper, l2q_su3_force_action_upper,
l2q_su3_projsu_digits_upper, l2q_vnet_heads_vupdate_sliced_upper_f64): the entries validate their arguments and
refuse, before any launch, the lattices and force_tile settings on which another force kernel runs; the kernel-name
query says which; and the plane selection of the force epilogue with the reconstruction the projection does
(csrc/su3_math.hpp: up_plane, m3_from_upper) give back an anti-Hermitian matrix bit for bit, signed zeros included,
in a host program built under AddressSanitizer + UBSan."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE = -1, -2


@pytest.fixture
def lib():
    from l2hmc import native
    return native.load()


def test_force_upper_arguments_and_refusals(lib):
    from l2hmc import native
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.c_void_p(p.value + 2048)
    for f in (lib.l2q_su3_force_upper,):
        assert f(None, 6.0, q, 1, 4, 4, 4, 4, None) == EINVAL and b'null pointer' in lib.l2q_last_error()
        assert f(p, 6.0, None, 1, 4, 4, 4, 4, None) == EINVAL
        assert f(p, 6.0, q, 0, 4, 4, 4, 4, None) == EINVAL
        assert f(p, 6.0, q, 1, 4, 4, 0, 4, None) == EINVAL
        assert f(p, 6.0, p, 1, 4, 4, 4, 4, None) == EINVAL and b'alias' in lib.l2q_last_error()
    g = lib.l2q_su3_force_action_upper
    big = 1 << 40
    assert g(None, 6.0, q, q, 1, 4, 4, 4, 4, q, big, None) == EINVAL
    assert g(p, 6.0, q, None, 1, 4, 4, 4, 4, q, big, None) == EINVAL
    assert g(p, 6.0, q, q, 1, 4, 4, 4, 4, None, big, None) == EINVAL
    assert g(p, 6.0, p, q, 1, 4, 4, 4, 4, q, big, None) == EINVAL
    assert g(p, 6.0, q, q, 1, 4, 4, 4, 4, q, 8, None) == ESHAPE and b'workspace' in lib.l2q_last_error()
    # lattices the thread-per-link kernel does not serve (odd V, a spatial volume that is no whole tile, one past its
    # size limit): refused with nothing launched, and the name query answers ''
    for L in ((3, 5, 2, 7), (1, 3, 2, 5), (4, 4, 4, 6), (8192, 8, 8, 8)):
        assert native.kernel_name('l2q_su3_force', L).startswith('su3_force_link') is False, L
        assert lib.l2q_su3_force_upper(p, 6.0, q, 1, *L, None) == ESHAPE, L
        assert b'upper-plane' in lib.l2q_last_error()
        assert g(p, 6.0, q, q, 1, *L, q, big, None) == ESHAPE, L
        assert native.kernel_name('l2q_su3_force_upper', L) == ''
        assert native.kernel_name('l2q_su3_force_action_upper', L) == ''
    # force_tile choosing another kernel on a lattice the link kernel serves
    L = (8, 8, 8, 8)
    try:
        for ft in (2, 7):
            assert native.set_tuning('force_tile', ft) >= 0
            assert lib.l2q_su3_force_upper(p, 6.0, q, 1, *L, None) == ESHAPE, ft
            assert g(p, 6.0, q, q, 1, *L, q, big, None) == ESHAPE, ft
            assert native.kernel_name('l2q_su3_force_upper', L) == ''
    finally:
        native.set_tuning('force_tile', 5)
    assert native.kernel_name('l2q_su3_force_upper', L) == 'su3_force_link_kernel<4, 6>'
    assert native.kernel_name('l2q_su3_force_action_upper', L) == 'su3_force_link_action_upper_kernel<6>'
    assert native.kernel_name('l2q_su3_force_upper', (4, 4, 4, 4)) == 'su3_force_link_kernel<4, 7>'
    assert native.kernel_name('l2q_su3_force_upper', (4, 4, 4, 8)) == 'su3_force_link_kernel<4, 6>'
    assert native.kernel_name('l2q_su3_force_upper', (2, 4, 4, 12)) == 'su3_force_link_kernel<4, 0>'
    assert native.kernel_name('l2q_su3_projsu_digits_upper', L) == 'su3_project_digits_upper_kernel'
    assert native.kernel_name('l2q_vnet_heads_vupdate_sliced_upper_f64', L) == 'heads_sliced_kernel'


def test_projection_and_heads_upper_arguments(lib):
    buf = (ctypes.c_char * 8192)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)     # (256-byte aligned, as the heads' buffers must be)
    f = lib.l2q_su3_projsu_digits_upper
    assert f(None, p, 2, 4, 64, None) == EINVAL and b'null pointer' in lib.l2q_last_error()
    assert f(p, None, 2, 4, 64, None) == EINVAL
    for V in (0, 16, 65, 100):
        assert f(p, p, 2, 4, V, None) == EINVAL, V
    assert f(p, p, 2, 3, 64, None) == EINVAL                      # whole chains
    assert f(p, p, 2000, 4, 64, None) == EINVAL                   # operand exponent
    assert f(ctypes.c_void_p(p.value), ctypes.c_void_p(p.value + 8), 2, 4, 64, None) == ESHAPE
    h = lib.l2q_vnet_heads_vupdate_sliced_upper_f64

    def heads(M=4, K=256, N=36 * 64, cplx=1, upper=1, V=64, ws_bytes=1 << 40, ptr=p):
        return h(ptr, M, K, N, ptr, ptr, ptr, 1.0, ptr, 1.0, ptr, ptr, 1.0, None, ptr, ptr, cplx, 0.1, 1, 0, 0, 0.0, 0,
                 ptr, None, None, ptr, ws_bytes, upper, V, None)
    assert heads(upper=2) == EINVAL and b'force_upper' in lib.l2q_last_error()
    assert heads(ptr=None) == EINVAL and b'null pointer' in lib.l2q_last_error()
    assert heads(K=128) == ESHAPE
    assert heads(ws_bytes=8) == ESHAPE and b'workspace' in lib.l2q_last_error()
    # an upper-plane force: complex, N = 36 V, V % 64 == 0, M 192 V < 2^32 -- refused before anything is launched
    for kw in (dict(cplx=0), dict(V=32, N=36 * 32), dict(V=128), dict(V=0), dict(N=36 * 64 + 16),
               dict(M=1 << 23, V=64, N=36 * 64)):
        assert heads(**kw) == ESHAPE, kw
        assert b'upper-plane' in lib.l2q_last_error(), (kw, lib.l2q_last_error())


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = tmp_path_factory.mktemp('upper_planes') / 'upper_planes_san'
    src = os.path.join(ROOT, 'tests', 'native_host', 'upper_planes', 'upper_planes.cpp')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'tests', 'native_host'), '-I', os.path.join(ROOT, 'l2hmc-qcd_amd', 'csrc'),
                    src, '-o', str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input='\n'.join(lines) + '\n', capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        assert r.stderr == '', r.stderr[-2000:]
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


def test_plane_selection_and_reconstruction_on_the_host(host):
    planes = [int(t) for t in host(['planes'])[0].split()]
    assert planes[:9] == [0, 3, 4, -1, 1, 5, -1, -1, 2]           # e = 3 i + j: diagonal first, then i < j
    assert planes[9:] == [0, 4, 8, 1, 2, 5]
    assert [planes[e] for e in planes[9:]] == list(range(6))      # up_plane inverts up_entry
    rng = np.random.default_rng(11)
    mats = [rng.normal(size=(3, 3)) + 1j * rng.normal(size=(3, 3)) for _ in range(64)]
    mats.append(np.zeros((3, 3), complex))                         # F = 0: every real part a zero
    mats.append(np.eye(3) * (0.3 + 0.2j))
    sym = rng.normal(size=(3, 3))
    mats.append((sym + sym.T) + 1j * rng.normal(size=(3, 3)))      # equal real parts across the diagonal: Re F = +0
    mats.append(-(sym + sym.T) + 0j)
    nan = rng.normal(size=(3, 3)) + 0j
    nan[0, 2] = complex(float('nan'), 1.0)
    mats.append(nan)
    lines = ['tah ' + ' '.join(f'{float(z.real)!r} {float(z.imag)!r}' for z in m.reshape(-1)) for m in mats]
    zeros = 0
    for m, ln in zip(mats, host(lines)):
        w = [int(t, 16) for t in ln.split()]
        full, rebuilt = w[:18], w[18:]
        assert len(rebuilt) == 18
        if not np.isnan(m).any():
            assert full == rebuilt, (m, full, rebuilt)             # bit for bit, signed zeros included
        else:
            isn = lambda b: (b & 0x7ff0000000000000) == 0x7ff0000000000000 and (b & 0xfffffffffffff) != 0
            assert all(a == b or (isn(a) and isn(b)) for a, b in zip(full, rebuilt))
        zeros += sum(1 for e in (1, 2, 5) if full[2 * e] in (0, 1 << 63))
    assert zeros >= 9                                              # the sign-of-zero case was exercised
