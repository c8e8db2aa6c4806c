// su3_wilson_f32.hip -- the single-precision kernels of the mixed-precision even-odd Wilson solves (defect correction:
// the inner CG on Mhat runs on these, the outer loop recomputes the true residual with the fp64 kernels of
// su3_wilson_eo.hip and su3_wilson.hip; l2hmc/lattice/su3/pytorch/wilson.py).
//
// su3_links_demote_eo_kernel: the fp32, parity-ordered copy of the links, x32[chain][parity][4][9][V/2] float2, entry h
// of parity p the link at site checkerboard_site(h, p).  One thread per (chain, half-site) copies the 2 x 36 entries of
// its site pair (2h, 2h + 1); plain vector loads and stores.
// su3_wilson_hop_eo_f32_kernel: out = b aux + a H src on the sites of one parity, the body of su3_wilson_hop_eo_kernel in
// float on float2 half fields [nb][nrhs][12][V/2] -- one thread per (system, half-site), 8 B / lane plane loads, the
// direction loop not unrolled, workgroups in the order chain, site block, right-hand side, the same xcd_swizzle.  The
// forward link of a site is entry h of this parity's block of x32, the backward link entry sb >> 1 of the other
// parity's block: every link load is contiguous across lanes and uses whole cache lines.  The fused norm is summed in
// double: each thread adds its 24 squares in double, the block partial is the fixed tree of block_sum, so a system's
// partials are the same bits whatever else the launch holds.
// su3_spinor_cg_update_f32_kernel, su3_spinor_xpay_f32_kernel: the two BLAS-1 kernels of su3_wilson.hip on float2
// fields; alpha and beta stay double per system on the device and are rounded to float in the kernel, |r|^2 is summed
// in double.  su3_spinor_demote_kernel: out32 = scale_s in64 (the product in double, rounded once);
// su3_spinor_promote_axpy_kernel: x64 += scale_s e32 in double, a system with scale_s = 0 is not touched.
#include "su3_spinor_f32.hpp"
#include "su3_subgroup.hpp"

namespace l2q {

__global__ __launch_bounds__(kBlock) void su3_links_demote_eo_kernel(const double2* __restrict__ xn,
                                                                     float2* __restrict__ x32, int X, int Y, int Z,
                                                                     int V, long nblk) {
  const long c = blockIdx.x / nblk;
  const int h = (int)(blockIdx.x % nblk) * kBlock + (int)threadIdx.x;
  const int Vh = V / 2;
  if (h >= Vh) return;
  const double2* xc = xn + c * 36L * V;
  float2* oc = x32 + c * 72L * Vh;
#pragma unroll 1
  for (int p = 0; p < 2; ++p) {
    const int s = checkerboard_site(h, p, X, Y, Z);
#pragma unroll 4
    for (int e = 0; e < 36; ++e) {
      const double2 d = xc[(long)e * V + s];
      oc[((long)p * 36 + e) * Vh + h] = make_float2((float)d.x, (float)d.y);
    }
  }
}

// sgn: +1 for H, -1 for gamma5 H gamma5; apbc: the seam of direction 0 carries -1.  aux, part: may be null.
// The kernel has a barrier where part is given: threads past the last half-site run along on half-site 0 and write
// nothing.
__global__ __launch_bounds__(kBlock, 2) void su3_wilson_hop_eo_f32_kernel(const float2* __restrict__ x32,
                                                                          const float2* __restrict__ src,
                                                                          const float2* aux, float2* out,
                                                                          double* __restrict__ part, float a, float bc,
                                                                          float sgn, int apbc, int parity, int nrhs,
                                                                          int T, int X, int Y, int Z, long nblk,
                                                                          int swz) {
  __shared__ double red[4];
  const Dims d{T, X, Y, Z, T * X * Y * Z};
  const WilsonBlock b = wilson_block(xcd_swizzle(blockIdx.x, (long)gridDim.x, swz), nrhs, nblk);
  const int Vh = d.V / 2;
  const int h0 = b.blk * kBlock + (int)threadIdx.x;
  const bool live = h0 < Vh;
  const int hs = live ? h0 : 0;
  const int s = checkerboard_site(hs, parity, X, Y, Z);
  const float2* uf = x32 + (b.c * 2 + parity) * 36L * Vh;          // the links at the sites of this parity
  const float2* ub = x32 + (b.c * 2 + (1 - parity)) * 36L * Vh;    // ... and of the other one
  const float2* pc = src + b.sys * 12L * Vh;
  float ar[12], ai[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) { ar[k] = 0.0f; ai[k] = 0.0f; }
#pragma unroll 1
  for (int mu = 0; mu < 4; ++mu) {
    const int st = stride_of(d, mu), ext = extent_of(d, mu);
    const int cm = (s / st) % ext;
    const bool seam = apbc != 0 && mu == 0;
    HalfSpinorF h, chi;
    M3F u;
    {  // (1 - gamma_mu) U_mu(x) src(x+mu)
      const bool wrap = cm + 1 == ext;
      const int sf = wrap ? s - (ext - 1) * st : s + st;
      wilson_project_f32(h, pc, Vh, sf >> 1, mu, sgn, seam && wrap ? -1.0f : 1.0f);
      load_link_f32(u, uf + mu * 9L * Vh, Vh, hs);
      wilson_colour_mul_f32<false>(chi, u, h);
      wilson_reconstruct_f32(ar, ai, chi, mu, sgn);
    }
    {  // (1 + gamma_mu) U_mu(x-mu)^H src(x-mu)
      const bool wrap = cm == 0;
      const int sb = wrap ? s + (ext - 1) * st : s - st;
      wilson_project_f32(h, pc, Vh, sb >> 1, mu, -sgn, seam && wrap ? -1.0f : 1.0f);
      load_link_f32(u, ub + mu * 9L * Vh, Vh, sb >> 1);
      wilson_colour_mul_f32<true>(chi, u, h);
      wilson_reconstruct_f32(ar, ai, chi, mu, -sgn);
    }
  }
  const long off = b.sys * 12L * Vh;
  double n2 = 0.0;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    float re = a * ar[k], im = a * ai[k];
    if (aux != nullptr) {              // a kernel argument: wave-uniform
      const float2 p = aux[off + k * Vh + hs];
      re = fmaf(a, ar[k], bc * p.x); im = fmaf(a, ai[k], bc * p.y);
    }
    if (live) out[off + k * Vh + hs] = make_float2(re, im);
    n2 = fma((double)re, (double)re, n2); n2 = fma((double)im, (double)im, n2);
  }
  if (part != nullptr) {               // a kernel argument: the whole grid takes the barrier or none of it
    const double t = block_sum(live ? n2 : 0.0, red);
    if (threadIdx.x == 0) part[b.sys * nblk + b.blk] = t;
  }
}

// x += alpha_s p, r -= alpha_s q in float, part[system][nblk] = the block's share of |r|^2 (the new r) in double.
__global__ __launch_bounds__(kBlock) void su3_spinor_cg_update_f32_kernel(float2* __restrict__ x, float2* __restrict__ r,
                                                                          const float2* __restrict__ p,
                                                                          const float2* __restrict__ q,
                                                                          const double* __restrict__ alpha,
                                                                          double* __restrict__ part, int V, long nblk,
                                                                          int swz) {
  __shared__ double red[4];
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long sys = w / nblk, blk = w % nblk;
  const int s = (int)blk * kBlock + (int)threadIdx.x;
  const bool live = s < V;
  const float a = (float)alpha[sys];
  const long base = sys * 12L * V;
  double n2 = 0.0;
  if (live) {
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const long i = base + (long)k * V + s;
      const float2 xv = x[i], rv = r[i], pv = p[i], qv = q[i];
      x[i] = make_float2(fmaf(a, pv.x, xv.x), fmaf(a, pv.y, xv.y));
      const float re = fmaf(-a, qv.x, rv.x), im = fmaf(-a, qv.y, rv.y);
      r[i] = make_float2(re, im);
      n2 = fma((double)re, (double)re, n2); n2 = fma((double)im, (double)im, n2);
    }
  }
  const double t = block_sum(n2, red);
  if (threadIdx.x == 0) part[sys * nblk + blk] = t;
}

// p = z + beta_s p
__global__ __launch_bounds__(kBlock) void su3_spinor_xpay_f32_kernel(float2* __restrict__ p,
                                                                     const float2* __restrict__ z,
                                                                     const double* __restrict__ beta, int V, long nblk,
                                                                     int swz) {
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long sys = w / nblk, blk = w % nblk;
  const int s = (int)blk * kBlock + (int)threadIdx.x;
  if (s >= V) return;
  const float bt = (float)beta[sys];
  const long base = sys * 12L * V;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const long i = base + (long)k * V + s;
    const float2 pv = p[i], zv = z[i];
    p[i] = make_float2(fmaf(bt, pv.x, zv.x), fmaf(bt, pv.y, zv.y));
  }
}

// out32 = scale_s in64
__global__ __launch_bounds__(kBlock) void su3_spinor_demote_kernel(const double2* __restrict__ in,
                                                                   const double* __restrict__ scale,
                                                                   float2* __restrict__ out, int V, long nblk) {
  const long sys = blockIdx.x / nblk;
  const int s = (int)(blockIdx.x % nblk) * kBlock + (int)threadIdx.x;
  if (s >= V) return;
  const double sc = scale[sys];
  const long base = sys * 12L * V;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const long i = base + (long)k * V + s;
    const double2 v = in[i];
    out[i] = make_float2((float)(sc * v.x), (float)(sc * v.y));
  }
}

// x64 += scale_s e32, product and sum in double; scale_s = 0: the system is not touched
__global__ __launch_bounds__(kBlock) void su3_spinor_promote_axpy_kernel(double2* __restrict__ x,
                                                                         const float2* __restrict__ e,
                                                                         const double* __restrict__ scale, int V,
                                                                         long nblk) {
  const long sys = blockIdx.x / nblk;
  const int s = (int)(blockIdx.x % nblk) * kBlock + (int)threadIdx.x;
  const double sc = scale[sys];
  if (s >= V || sc == 0.0) return;
  const long base = sys * 12L * V;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const long i = base + (long)k * V + s;
    const float2 ev = e[i];
    const double2 xv = x[i];
    x[i] = make_double2(fma(sc, (double)ev.x, xv.x), fma(sc, (double)ev.y, xv.y));
  }
}

}  // namespace l2q

using namespace l2q;

extern "C" {

int l2q_su3_links_demote_eo(const void* xn, void* x32, int nb, int T, int X, int Y, int Z, void* stream) {
  L2Q_REQUIRE(xn && x32, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(x32 != xn, L2Q_EINVAL, "x32 must not alias xn");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(all_even(T, X, Y, Z), L2Q_ESHAPE, "a checkerboard update needs even extents");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V / 2, kBlock);
  hipLaunchKernelGGL(su3_links_demote_eo_kernel, dim3((unsigned)(nb * nblk)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const double2*)xn, (float2*)x32, X, Y, Z, d.V, nblk);
  return check_launch("l2q_su3_links_demote_eo");
}

int l2q_su3_wilson_hop_eo_f32(const void* x32, const void* src, const void* aux, void* out, double* norm_part, double a,
                              double b, int flags, int parity, int nb, int nrhs, int T, int X, int Y, int Z,
                              void* stream) {
  L2Q_REQUIRE(x32 && src && out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(out != src && out != x32, L2Q_EINVAL, "out must not alias src or x32");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z) && nrhs > 0, L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(spinor_dims_ok((long)nb * nrhs, (long)T * X * Y * Z), L2Q_EINVAL,
              "size: nb * nrhs * 12 * V does not fit an int");
  L2Q_REQUIRE(a - a == 0.0 && b - b == 0.0, L2Q_EINVAL, "the coefficients a and b must be finite");
  L2Q_REQUIRE(flags >= 0 && flags <= 3, L2Q_EINVAL, "flags must be 0..3 (bit 0 dagger, bit 1 antiperiodic in t)");
  L2Q_REQUIRE(parity == 0 || parity == 1, L2Q_EINVAL, "parity must be 0 (even) or 1 (odd)");
  L2Q_REQUIRE(all_even(T, X, Y, Z), L2Q_ESHAPE, "a checkerboard update needs even extents");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V / 2, kBlock);
  hipLaunchKernelGGL(su3_wilson_hop_eo_f32_kernel, dim3((unsigned)((long)nb * nrhs * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, (const float2*)x32, (const float2*)src, (const float2*)aux, (float2*)out,
                     norm_part, (float)a, (float)b, (flags & 1) ? -1.0f : 1.0f, (flags >> 1) & 1, parity, nrhs, T, X, Y,
                     Z, nblk, tuning().xcd_swizzle);
  return check_launch("l2q_su3_wilson_hop_eo_f32");
}

int l2q_su3_spinor_cg_update_f32(void* x, void* r, const void* p, const void* q, const double* alpha, double* rr_part,
                                 long nsys, long V, void* stream) {
  L2Q_REQUIRE(x && r && p && q && alpha && rr_part, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(x != r && x != p && x != q && r != p && r != q, L2Q_EINVAL, "x and r must not alias another field");
  L2Q_REQUIRE(spinor_dims_ok(nsys, V), L2Q_EINVAL, "size: need nsys, V > 0 and nsys * 12 * V within an int");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_spinor_cg_update_f32_kernel, dim3((unsigned)(nsys * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, (float2*)x, (float2*)r, (const float2*)p, (const float2*)q, alpha, rr_part,
                     (int)V, nblk, tuning().xcd_swizzle);
  return check_launch("l2q_su3_spinor_cg_update_f32");
}

int l2q_su3_spinor_xpay_f32(void* p, const void* z, const double* beta, long nsys, long V, void* stream) {
  L2Q_REQUIRE(p && z && beta, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(p != z, L2Q_EINVAL, "p must not alias z");
  L2Q_REQUIRE(spinor_dims_ok(nsys, V), L2Q_EINVAL, "size: need nsys, V > 0 and nsys * 12 * V within an int");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_spinor_xpay_f32_kernel, dim3((unsigned)(nsys * nblk)), dim3(kBlock), 0, (hipStream_t)stream,
                     (float2*)p, (const float2*)z, beta, (int)V, nblk, tuning().xcd_swizzle);
  return check_launch("l2q_su3_spinor_xpay_f32");
}

int l2q_su3_spinor_demote(const void* in64, const double* scale, void* out32, long nsys, long V, void* stream) {
  L2Q_REQUIRE(in64 && scale && out32, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(out32 != in64, L2Q_EINVAL, "out32 must not alias in64");
  L2Q_REQUIRE(spinor_dims_ok(nsys, V), L2Q_EINVAL, "size: need nsys, V > 0 and nsys * 12 * V within an int");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_spinor_demote_kernel, dim3((unsigned)(nsys * nblk)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const double2*)in64, scale, (float2*)out32, (int)V, nblk);
  return check_launch("l2q_su3_spinor_demote");
}

int l2q_su3_spinor_promote_axpy(void* x64, const void* e32, const double* scale, long nsys, long V, void* stream) {
  L2Q_REQUIRE(x64 && e32 && scale, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(x64 != e32, L2Q_EINVAL, "x64 must not alias e32");
  L2Q_REQUIRE(spinor_dims_ok(nsys, V), L2Q_EINVAL, "size: need nsys, V > 0 and nsys * 12 * V within an int");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_spinor_promote_axpy_kernel, dim3((unsigned)(nsys * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, (double2*)x64, (const float2*)e32, scale, (int)V, nblk);
  return check_launch("l2q_su3_spinor_promote_axpy");
}

}  // extern "C"
