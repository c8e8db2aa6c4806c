// su3_spinor_mshift.hip -- the BLAS-1 kernels of multi-shift CG (Jegerlehner, hep-lat/9612014) and of the rational
// heatbath on top of it (l2hmc/lattice/su3/pytorch/wilson.py: `_CG.multishift`, `rhmc_pseudofermion_refresh_n`).
//
// Shifted fields are f[system][shift][12][sites] complex128, a system one (chain, rhs) pair, sites V or V/2; a (system,
// shift) pair is then a system of every other spinor kernel.  The unshifted fields r, p, z, out are [system][12][sites].
// One workgroup handles one system and one block of kBlock sites, in the order and under the xcd_swizzle of
// su3_spinor_cg_update_kernel; one thread per site.  Every coefficient comes from a device array, one per system or
// per (system, shift); partial sums are the fixed tree of block_sum, so a system's bits do not depend on the batch.
//
// su3_spinor_mshift_update_kernel, the fused step of an iteration: with the new residual r,
//   p <- r + beta p;   for every shift k with live[system][k] != 0:  x_k += a_k p_k,  p_k <- zeta_k r + b_k p_k
// (the old p_k in the first).  Loop order: the thread loads the 12 components of r once and keeps them in registers (48
// VGPRs) across the shift loop; the shift loop is not unrolled, and inside it a shift goes in two passes of 6
// components, the 12 loads of x_k and p_k of a pass (16 B / lane each, coalesced planes) all issued before the first is
// used, which is what keeps a pure streaming kernel fed.  (All 24 at once, with their 24 64-bit addresses, take 252
// VGPRs and occupancy 2; capped at 168 or 128 VGPRs that form spills.)  live[system][k] is the same for the whole
// workgroup: a shift that is not live is neither read nor written.  Bytes per site: 3 fields (r read, p read and
// written) + 4 fields per live shift.  Compiler's resources for gfx950 (profiles/su3_wilson_multishift/
// kernel_resources.txt): 168 VGPRs, 0 AGPRs, no scratch, no LDS, occupancy 3 waves per SIMD, so 36 wave-loads of 1 KiB
// in flight per SIMD.
// su3_spinor_axmy_norm_kernel, the residual step: r -= alpha z, part[system][block] = the block's share of the new |r|^2.
// su3_spinor_lincomb_kernel: out = sum_k w_k x_k over the ns fields of a system, the shift loop not unrolled, the 12
// loads of a shift issued together; the sum runs in the order of k.
#include "su3_spinor.hpp"

namespace l2q {

__global__ __launch_bounds__(kBlock) void su3_spinor_mshift_update_kernel(
    double2* __restrict__ x, double2* __restrict__ ps, double2* __restrict__ p, const double2* __restrict__ r,
    const double* __restrict__ a, const double* __restrict__ b, const double* __restrict__ zeta,
    const double* __restrict__ beta, const int* __restrict__ live, int ns, int V, long nblk, int swz) {
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long sys = w / nblk, blk = w % nblk;
  const int s = (int)blk * kBlock + (int)threadIdx.x;
  if (s >= V) return;
  const long base = sys * 12L * V + s;
  double rr[12], ri[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const double2 v = r[base + (long)k * V];
    rr[k] = v.x; ri[k] = v.y;
  }
  {
    const double bt = beta[sys];
    double2 pv[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) pv[k] = p[base + (long)k * V];
#pragma unroll
    for (int k = 0; k < 12; ++k) p[base + (long)k * V] = make_double2(fma(bt, pv[k].x, rr[k]), fma(bt, pv[k].y, ri[k]));
  }
#pragma unroll 1
  for (int j = 0; j < ns; ++j) {
    const long c = sys * ns + j;
    if (live[c] == 0) continue;                       // workgroup-uniform: sys comes from blockIdx
    const double aj = a[c], bj = b[c], zj = zeta[c];
    const long bs = c * 12L * V + s;
#pragma unroll
    for (int h = 0; h < 12; h += 6) {                 // two passes of 6 components: 12 loads in flight, then 12 stores
      double2 xv[6], pv[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) { xv[k] = x[bs + (long)(h + k) * V]; pv[k] = ps[bs + (long)(h + k) * V]; }
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        x[bs + (long)(h + k) * V] = make_double2(fma(aj, pv[k].x, xv[k].x), fma(aj, pv[k].y, xv[k].y));
        ps[bs + (long)(h + k) * V] = make_double2(fma(bj, pv[k].x, zj * rr[h + k]), fma(bj, pv[k].y, zj * ri[h + k]));
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void su3_spinor_axmy_norm_kernel(double2* __restrict__ r,
                                                                      const double2* __restrict__ z,
                                                                      const double* __restrict__ alpha,
                                                                      double* __restrict__ part, int V, long nblk,
                                                                      int swz) {
  __shared__ double red[4];
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long sys = w / nblk, blk = w % nblk;
  const int s = (int)blk * kBlock + (int)threadIdx.x;
  const bool live = s < V;
  const double al = alpha[sys];
  const long base = sys * 12L * V;
  double n2 = 0.0;
  if (live) {
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const long i = base + (long)k * V + s;
      const double2 rv = r[i], zv = z[i];
      const double re = fma(-al, zv.x, rv.x), im = fma(-al, zv.y, rv.y);
      r[i] = make_double2(re, im);
      n2 = fma(re, re, n2); n2 = fma(im, im, n2);
    }
  }
  const double t = block_sum(n2, red);
  if (threadIdx.x == 0) part[sys * nblk + blk] = t;
}

__global__ __launch_bounds__(kBlock) void su3_spinor_lincomb_kernel(const double2* __restrict__ x,
                                                                    const double* __restrict__ wt,
                                                                    double2* __restrict__ out, int ns, int V,
                                                                    long nblk, int swz) {
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long sys = w / nblk, blk = w % nblk;
  const int s = (int)blk * kBlock + (int)threadIdx.x;
  if (s >= V) return;
  double ar[12], ai[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) { ar[k] = 0.0; ai[k] = 0.0; }
#pragma unroll 1
  for (int j = 0; j < ns; ++j) {
    const long c = sys * ns + j;
    const double wj = wt[c];
    const long bs = c * 12L * V + s;
    double2 xv[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) xv[k] = x[bs + (long)k * V];
#pragma unroll
    for (int k = 0; k < 12; ++k) { ar[k] = fma(wj, xv[k].x, ar[k]); ai[k] = fma(wj, xv[k].y, ai[k]); }
  }
  const long base = sys * 12L * V + s;
#pragma unroll
  for (int k = 0; k < 12; ++k) out[base + (long)k * V] = make_double2(ar[k], ai[k]);
}

// [lo, lo + n) and [f, f + m) share a byte
inline bool ranges_overlap(const void* lo, double n, const void* f, double m) {
  const double a = (double)(uintptr_t)lo, b = (double)(uintptr_t)f;      // addresses are exact in a double
  return b < a + n && a < b + m;
}

}  // namespace l2q

using namespace l2q;

extern "C" {

int l2q_su3_spinor_mshift_update(void* x, void* ps, void* p, const void* r, const double* a, const double* b,
                                 const double* zeta, const double* beta, const int* live, long nsys, long ns, long V,
                                 void* stream) {
  L2Q_REQUIRE(x && ps && p && r && a && b && zeta && beta && live, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(ns >= 1, L2Q_EINVAL, "ns must be >= 1");
  L2Q_REQUIRE(nsys > 0 && spinor_dims_ok(nsys * (double)ns < 2147483648.0 ? nsys * ns : 0, V), L2Q_EINVAL,
              "size: need nsys, ns, V > 0 and nsys * ns * 12 * V within an int");
  const double one = (double)nsys * 12.0 * (double)V * sizeof(double2), all = one * (double)ns;
  L2Q_REQUIRE(!ranges_overlap(x, all, r, one) && !ranges_overlap(ps, all, r, one) && !ranges_overlap(p, one, r, one),
              L2Q_EINVAL, "r must not alias p, an x_k or a p_k");
  L2Q_REQUIRE(!ranges_overlap(x, all, ps, all) && !ranges_overlap(x, all, p, one) && !ranges_overlap(ps, all, p, one),
              L2Q_EINVAL, "x, the p_k and p must not alias one another");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_spinor_mshift_update_kernel, dim3((unsigned)(nsys * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, (double2*)x, (double2*)ps, (double2*)p, (const double2*)r, a, b, zeta, beta,
                     live, (int)ns, (int)V, nblk, tuning().xcd_swizzle);
  return check_launch("l2q_su3_spinor_mshift_update");
}

int l2q_su3_spinor_axmy_norm(void* r, const void* z, const double* alpha, double* rr_part, long nsys, long V,
                             void* stream) {
  L2Q_REQUIRE(r && z && alpha && rr_part, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(r != z, L2Q_EINVAL, "r must not alias z");
  L2Q_REQUIRE(spinor_dims_ok(nsys, V), L2Q_EINVAL, "size: need nsys, V > 0 and nsys * 12 * V within an int");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_spinor_axmy_norm_kernel, dim3((unsigned)(nsys * nblk)), dim3(kBlock), 0, (hipStream_t)stream,
                     (double2*)r, (const double2*)z, alpha, rr_part, (int)V, nblk, tuning().xcd_swizzle);
  return check_launch("l2q_su3_spinor_axmy_norm");
}

int l2q_su3_spinor_lincomb(const void* x, const double* w, void* out, long nsys, long ns, long V, void* stream) {
  L2Q_REQUIRE(x && w && out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(ns >= 1, L2Q_EINVAL, "ns must be >= 1");
  L2Q_REQUIRE(nsys > 0 && spinor_dims_ok(nsys * (double)ns < 2147483648.0 ? nsys * ns : 0, V), L2Q_EINVAL,
              "size: need nsys, ns, V > 0 and nsys * ns * 12 * V within an int");
  const double one = (double)nsys * 12.0 * (double)V * sizeof(double2);
  L2Q_REQUIRE(!ranges_overlap(x, one * (double)ns, out, one), L2Q_EINVAL, "out must not alias an x_k");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_spinor_lincomb_kernel, dim3((unsigned)(nsys * nblk)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const double2*)x, w, (double2*)out, (int)ns, (int)V, nblk, tuning().xcd_swizzle);
  return check_launch("l2q_su3_spinor_lincomb");
}

}  // extern "C"
