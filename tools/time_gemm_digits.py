"""cfg-4 input layer (M 256, N 256, K 131072 + 131072) on fp64 activations sliced on the fly (gemm_sliced.hip)
against the same layer on activation digit images (gemm_digits.hip), and the kernels that write the two kinds of
activations: the projection and the x-update of an 8^4 lattice with 256 chains, the stand-alone slicer.
With a library built by tools/ab_build.sh <name> gemm_digits -DL2Q_GD_EXP=64 (L2Q_LIB_NAME=libl2q_<name>.so)
the kernel prints its clocks per slab; ONLY_GEMM=1 then keeps the output short."""
import os, sys
import torch
sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'l2hmc-qcd_amd'))
from l2hmc import _ops as ops


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


m, n = int(os.environ.get('M', 256)), int(os.environ.get('NN', 256))
L = [int(i) for i in os.environ.get('LAT', '8,8,8,8').split(',')]
V = L[0] * L[1] * L[2] * L[3]
k = 32 * V
only_gemm = bool(int(os.environ.get('ONLY_GEMM', '0')))
iters = 2 if only_gemm else 20
g = torch.Generator(device='cuda').manual_seed(1)
a = (torch.rand(m, k, dtype=torch.float64, device='cuda', generator=g) - 0.5) * 4.0
a2 = (torch.rand(m, k, dtype=torch.float64, device='cuda', generator=g) - 0.5) * 4.0
w = (torch.rand(n, k, dtype=torch.float64, device='cuda', generator=g) - 0.5) / k ** 0.5
w2 = (torch.rand(n, k, dtype=torch.float64, device='cuda', generator=g) - 0.5) / k ** 0.5
b = torch.zeros(n, dtype=torch.float64, device='cuda')
img, img2 = ops.gemm_sliced_build(w), ops.gemm_sliced_build(w2)
da, da2 = ops.gemm_digits_slice(a), ops.gemm_digits_slice(a2)
want = ops.gemm_sliced(a, img, n, b, a2=a2, image2=img2, bias2=b, act='tanh')
got = ops.gemm_digits(da, img, n, b, a2=da2, image2=img2, bias2=b, act='tanh')
print('digits == sliced:', bool(torch.equal(got, want)), flush=True)
for name, fn in (('sliced (fp64 A)', lambda: ops.gemm_sliced(a, img, n, b, a2=a2, image2=img2, bias2=b, act='tanh')),
                 ('digits (image A)', lambda: ops.gemm_digits(da, img, n, b, a2=da2, image2=img2, bias2=b, act='tanh'))):
    ms = timeit(fn, iters, 1 if only_gemm else 3)
    print(f'{name:18s} M {m} N {n} K 2x{k}: {ms:.4f} ms  {2.0 * m * n * 2 * k / ms / 1e9:.1f} fp64-equivalent TFLOP/s',
          flush=True)
if only_gemm:
    sys.exit(0)
print(f'slicer fp64 -> image [{m}][{k}]: {timeit(lambda: ops.gemm_digits_slice(a)):.4f} ms', flush=True)
xn = torch.randn(m, 4, 9, V, dtype=torch.complex128, device='cuda', generator=g) * 0.1
xn[:, :, 0] += 1.0; xn[:, :, 4] += 1.0; xn[:, :, 8] += 1.0
xn = ops.su3_project_su_n(xn)
vn = ops.su3_project_tah_n(torch.randn(m, 4, 9, V, dtype=torch.complex128, device='cuda', generator=g))
mask = (torch.rand(4, 1, V, device='cuda', generator=g) < 0.5).float().expand(4, 9, V).contiguous()
for rep in range(3):
    print(f'round {rep}: projection vec8 {timeit(lambda: ops.su3_projsu_vec8_n(xn)):.4f} ms, '
          f'digits {timeit(lambda: ops.su3_projsu_digits_n(xn)):.4f} ms; '
          f'x-update vec8 {timeit(lambda: ops.su3_expm_mul2_vec8_n(xn, vn, 0.05, mask, False)):.4f} ms, '
          f'digits {timeit(lambda: ops.su3_expm_mul2_digits_n(xn, vn, 0.05, mask, False)):.4f} ms', flush=True)
