// su3_wilson.hip -- the Wilson-Dirac operator on spinor fields and the two BLAS-1 kernels of a CG iteration around it.
// (Wilson 1974; the half-spinor form of the hopping term is that of every lattice code since.)
//
//   M psi = psi - kappa H psi,
//   H psi(x) = sum_mu [(1 - gamma_mu) U_mu(x) psi(x+mu) + (1 + gamma_mu) U_mu(x-mu)^H psi(x-mu)],
//   M^H = gamma5 M gamma5: the two projector signs swapped (flags bit 0).
// Boundary: periodic; flags bit 1 gives every hop across the t = T-1 -> 0 seam (direction 0), either way, a factor -1.
// With an extent of 1 or 2 the two neighbours coincide and both terms are added; with T = 1 both hops carry the sign.
//
// Gamma matrices: Hermitian, chiral, gamma_mu = [[0, B_mu], [B_mu^H, 0]] in 2 x 2 blocks with
//   B_0 = 1 (direction 0 is T),  B_k = -i sigma_k (k = 1, 2, 3 = x, y, z),  gamma5 = g0 g1 g2 g3 = diag(-1, -1, 1, 1).
// 1 - s gamma_mu has rank 2: with h = psi_u - s B psi_l (the upper two spin components), (1 - s gamma_mu) psi =
// (h, -s B^H h).  So a hop projects the neighbour to the half spinor h (6 complex), multiplies its two colour vectors
// by the link, adds the product chi to the upper half of the sum and -s B^H chi to the lower half: 1320 flops a site.
//
// Spinor fields are psi[chain][rhs][12][V] (component 3 spin + colour, the site index of the links); a system is one
// (chain, rhs) pair.  su3_wilson_kernel: one thread per (system, site); every operand a coalesced 16 B / lane plane
// load.  The direction loop is not unrolled (live: the sum 48 VGPRs, a half spinor 24, a link 36, a product 24), the
// neighbours come by division (site_hop's arithmetic), psi(x) itself is loaded after the loop.  A workgroup belongs to
// one system; with norm_part it leaves |out|^2 over its sites as one partial, part[system][site block], by the fixed
// tree of block_sum: a system's partials are the same bits whatever else the launch holds.
// Block order: chain, site block, right-hand side -- consecutive workgroups read the same links (profiles/su3_wilson.md).
// su3_spinor_cg_update_kernel, su3_spinor_xpay_kernel: one thread per (system, site), the 12 components in turn; the
// coefficients come from a device array, one per system.
// HalfSpinor, wilson_project, wilson_colour_mul, wilson_reconstruct, wilson_block and spinor_dims_ok: su3_spinor.hpp,
// shared with su3_wilson_eo.hip (the half-lattice hop) and su3_wilson_force.hip.
#include "su3_spinor.hpp"

namespace l2q {

// sgn: +1 for M, -1 for M^H; apbc: the seam of direction 0 carries -1.  part (may be null): [system][nblk].
// The kernel has a barrier where part is given: threads past the last site run along on site 0 and write nothing.
__global__ __launch_bounds__(kBlock, 2) void su3_wilson_kernel(const double2* __restrict__ xn,
                                                               const double2* __restrict__ psi,
                                                               double2* __restrict__ out, double* __restrict__ part,
                                                               double kappa, double sgn, int apbc, int nrhs, int T,
                                                               int X, int Y, int Z, long nblk, int swz) {
  __shared__ double red[4];
  const Dims d{T, X, Y, Z, T * X * Y * Z};
  const WilsonBlock b = wilson_block(xcd_swizzle(blockIdx.x, (long)gridDim.x, swz), nrhs, nblk);
  const int V = d.V;
  const int s0 = b.blk * kBlock + (int)threadIdx.x;
  const bool live = s0 < V;
  const int s = live ? s0 : 0;
  const double2* xc = xn + b.c * 36L * V;
  const double2* pc = psi + b.sys * 12L * V;
  double ar[12], ai[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) { ar[k] = 0.0; ai[k] = 0.0; }
#pragma unroll 1
  for (int mu = 0; mu < 4; ++mu) {
    const int st = stride_of(d, mu), ext = extent_of(d, mu);
    const double2* um = xc + mu * 9L * V;
    const int cm = (s / st) % ext;
    const bool seam = apbc != 0 && mu == 0;
    HalfSpinor h, chi;
    M3 u;
    {  // (1 - gamma_mu) U_mu(x) psi(x+mu)
      const bool wrap = cm + 1 == ext;
      wilson_project(h, pc, V, wrap ? s - (ext - 1) * st : s + st, mu, sgn, seam && wrap ? -1.0 : 1.0);
      load_link(u, um, V, s);
      wilson_colour_mul<false>(chi, u, h);
      wilson_reconstruct(ar, ai, chi, mu, sgn);
    }
    {  // (1 + gamma_mu) U_mu(x-mu)^H psi(x-mu)
      const bool wrap = cm == 0;
      const int sb = wrap ? s + (ext - 1) * st : s - st;
      wilson_project(h, pc, V, sb, mu, -sgn, seam && wrap ? -1.0 : 1.0);
      load_link(u, um, V, sb);
      wilson_colour_mul<true>(chi, u, h);
      wilson_reconstruct(ar, ai, chi, mu, -sgn);
    }
  }
  double2* oc = out + b.sys * 12L * V;
  double n2 = 0.0;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const double2 p = pc[k * V + s];
    const double re = fma(-kappa, ar[k], p.x), im = fma(-kappa, ai[k], p.y);
    if (live) oc[k * V + s] = make_double2(re, im);
    n2 = fma(re, re, n2); n2 = fma(im, im, n2);
  }
  if (part != nullptr) {             // a kernel argument: the whole grid takes the barrier or none of it
    const double t = block_sum(live ? n2 : 0.0, red);
    if (threadIdx.x == 0) part[b.sys * nblk + b.blk] = t;
  }
}

// x += alpha_s p, r -= alpha_s q, part[system][nblk] = the block's share of |r|^2 (the new r).  x, r are read and
// written by the same thread only.
__global__ __launch_bounds__(kBlock) void su3_spinor_cg_update_kernel(double2* __restrict__ x, double2* __restrict__ r,
                                                                      const double2* __restrict__ p,
                                                                      const double2* __restrict__ q,
                                                                      const double* __restrict__ alpha,
                                                                      double* __restrict__ part, int V, long nblk,
                                                                      int swz) {
  __shared__ double red[4];
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long sys = w / nblk, blk = w % nblk;
  const int s = (int)blk * kBlock + (int)threadIdx.x;
  const bool live = s < V;
  const double a = alpha[sys];
  const long base = sys * 12L * V;
  double n2 = 0.0;
  if (live) {
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const long i = base + (long)k * V + s;
      const double2 xv = x[i], rv = r[i], pv = p[i], qv = q[i];
      x[i] = make_double2(fma(a, pv.x, xv.x), fma(a, pv.y, xv.y));
      const double re = fma(-a, qv.x, rv.x), im = fma(-a, qv.y, rv.y);
      r[i] = make_double2(re, im);
      n2 = fma(re, re, n2); n2 = fma(im, im, n2);
    }
  }
  const double t = block_sum(n2, red);
  if (threadIdx.x == 0) part[sys * nblk + blk] = t;
}

// p = z + beta_s p
__global__ __launch_bounds__(kBlock) void su3_spinor_xpay_kernel(double2* __restrict__ p, const double2* __restrict__ z,
                                                                 const double* __restrict__ beta, int V, long nblk,
                                                                 int swz) {
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long sys = w / nblk, blk = w % nblk;
  const int s = (int)blk * kBlock + (int)threadIdx.x;
  if (s >= V) return;
  const double bt = beta[sys];
  const long base = sys * 12L * V;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const long i = base + (long)k * V + s;
    const double2 pv = p[i], zv = z[i];
    p[i] = make_double2(fma(bt, pv.x, zv.x), fma(bt, pv.y, zv.y));
  }
}

}  // namespace l2q

using namespace l2q;

extern "C" {

long l2q_su3_wilson_norm_parts(int T, int X, int Y, int Z) {
  if (T <= 0 || X <= 0 || Y <= 0 || Z <= 0 || (double)T * X * Y * Z * 36.0 >= 2.0e9) return 0;
  return cdiv((long)T * X * Y * Z, kBlock);
}

int l2q_su3_wilson_apply(const void* xn, const void* psi, void* out, double* norm_part, double kappa, int flags, int nb,
                         int nrhs, int T, int X, int Y, int Z, void* stream) {
  L2Q_REQUIRE(xn && psi && out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(out != psi && out != xn, L2Q_EINVAL, "out must not alias psi or xn");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z) && nrhs > 0, L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(spinor_dims_ok((long)nb * nrhs, (long)T * X * Y * Z), L2Q_EINVAL,
              "size: nb * nrhs * 12 * V does not fit an int");
  L2Q_REQUIRE(kappa - kappa == 0.0, L2Q_EINVAL, "kappa must be finite");
  L2Q_REQUIRE(flags >= 0 && flags <= 3, L2Q_EINVAL, "flags must be 0..3 (bit 0 dagger, bit 1 antiperiodic in t)");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V, kBlock);
  hipLaunchKernelGGL(su3_wilson_kernel, dim3((unsigned)((long)nb * nrhs * nblk)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const double2*)xn, (const double2*)psi, (double2*)out, norm_part, kappa,
                     (flags & 1) ? -1.0 : 1.0, (flags >> 1) & 1, nrhs, T, X, Y, Z, nblk, tuning().xcd_swizzle);
  return check_launch("l2q_su3_wilson_apply");
}

int l2q_su3_spinor_cg_update(void* x, void* r, const void* p, const void* q, const double* alpha, double* rr_part,
                             long nsys, long V, void* stream) {
  L2Q_REQUIRE(x && r && p && q && alpha && rr_part, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(x != r && x != p && x != q && r != p && r != q, L2Q_EINVAL, "x and r must not alias another field");
  L2Q_REQUIRE(spinor_dims_ok(nsys, V), L2Q_EINVAL, "size: need nsys, V > 0 and nsys * 12 * V within an int");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_spinor_cg_update_kernel, dim3((unsigned)(nsys * nblk)), dim3(kBlock), 0, (hipStream_t)stream,
                     (double2*)x, (double2*)r, (const double2*)p, (const double2*)q, alpha, rr_part, (int)V, nblk,
                     tuning().xcd_swizzle);
  return check_launch("l2q_su3_spinor_cg_update");
}

int l2q_su3_spinor_xpay(void* p, const void* z, const double* beta, long nsys, long V, void* stream) {
  L2Q_REQUIRE(p && z && beta, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(p != z, L2Q_EINVAL, "p must not alias z");
  L2Q_REQUIRE(spinor_dims_ok(nsys, V), L2Q_EINVAL, "size: need nsys, V > 0 and nsys * 12 * V within an int");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_spinor_xpay_kernel, dim3((unsigned)(nsys * nblk)), dim3(kBlock), 0, (hipStream_t)stream,
                     (double2*)p, (const double2*)z, beta, (int)V, nblk, tuning().xcd_swizzle);
  return check_launch("l2q_su3_spinor_xpay");
}

}  // extern "C"
