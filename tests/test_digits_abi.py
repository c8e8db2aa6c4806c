"""Argument checks of the digit-image entry points (include/l2q.h); no GPU needed."""
import ctypes


def test_digit_entry_points_reject_bad_arguments():
    from l2hmc import native
    lib = native.load()
    EINVAL = -1
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.cast(buf, ctypes.c_void_p)
    # null pointers
    assert lib.l2q_su3_projsu_digits(None, p, 2, 4, 64, None) == EINVAL
    assert b'null pointer' in lib.l2q_last_error()
    assert lib.l2q_su3_projsu_digits(p, None, 2, 4, 64, None) == EINVAL
    assert lib.l2q_su3_expm_mul2_digits(p, p, 0.1, p, 0, p, None, 2, 1, 64, None) == EINVAL
    assert lib.l2q_su3_expm_mul2_digits(None, p, 0.1, p, 0, p, p, 2, 1, 64, None) == EINVAL
    assert lib.l2q_su3_expm_mul2_digits(p, p, 0.1, None, 0, p, p, 2, 1, 64, None) == EINVAL
    assert lib.l2q_gemm_digits_slice(None, 64, 64, 2, p, 1 << 12, None) == EINVAL
    assert lib.l2q_gemm_digits_slice(p, 64, 64, 2, None, 1 << 12, None) == EINVAL
    assert lib.l2q_gemm_digits_f64(None, p, 64, 2, None, None, 0, 2, 64, 64, None, None, None, 1.0, 0, p, p, 1 << 20,
                                   None) == EINVAL
    assert lib.l2q_gemm_digits_f64(p, p, 64, 2, None, None, 64, 2, 64, 64, None, None, None, 1.0, 0, p, p, 1 << 20,
                                   None) == EINVAL                      # K2 without its operands
    # lattices the producers do not serve: V % 64 != 0, part of a chain
    for V in (48, 96, 65):
        assert lib.l2q_su3_projsu_digits(p, p, 2, 4, V, None) == EINVAL, V
        assert b'V % 64' in lib.l2q_last_error()
        assert lib.l2q_su3_expm_mul2_digits(p, p, 0.1, p, 0, p, p, 2, 1, V, None) == EINVAL, V
    assert lib.l2q_su3_projsu_digits(p, p, 2, 3, 64, None) == EINVAL
    assert lib.l2q_gemm_digits_slice(p, 64, 100, 2, p, 1 << 12, None) == EINVAL
    assert lib.l2q_gemm_digits_bytes(64, 100) == 0 and lib.l2q_gemm_digits_bytes(0, 64) == 0
    assert lib.l2q_gemm_digits_bytes(256, 131072) == 256 * 2048 * 7 * 64
    # the kernels behind the entry points
    for entry, kern in (('l2q_gemm_digits_f64', 'gemm_digits_kernel'), ('l2q_gemm_digits_slice', 'gd_slice_kernel'),
                        ('l2q_su3_projsu_digits', 'su3_project_digits_kernel'),
                        ('l2q_su3_expm_mul2_digits', 'su3_expm_mul_digits_kernel')):
        assert native.kernel_name(entry, (4, 4, 4, 4)) == kern
