// su3_gaugefix.hip -- Landau and Coulomb gauge fixing by local maximisation (Los Alamos iteration with overrelaxation,
// Mandula & Ogilvie; SU(3) through its SU(2) subgroups as in Cabibbo-Marinari), on one checkerboard per launch.
//
//   D: the gauge directions, a 4-bit set (Landau: all four; Coulomb: all but the time direction).
//   F = (1 / (3 |D| V)) sum_x sum_{mu in D} Re tr U_mu(x)                   is maximised by g(x) in U -> g U g(x+mu)^H
//   A_mu(x) = (U - U^H) / (2i) - tr / 3,  Delta(x) = sum_{mu in D} [A_mu(x) - A_mu(x-mu)],
//   theta = (1 / (3 V)) sum_x tr Delta Delta^H                              vanishes at a maximum
//   Local step at x: K = sum_{mu in D} [U_mu(x) + U_mu(x-mu)^H], g = 1, W = K; for (i, j) = (0,1), (0,2), (1,2):
//     rh = r / |r| of W (su3_subgroup.hpp), a = conj(rh) = (cos phi, n sin phi), phi = atan2(|a_vec|, a0) in [0, pi],
//     a^omega = (cos(omega phi), n sin(omega phi)) (the identity where |r| is zero or not finite, or a_vec = 0),
//     g <- embed(a^omega) g, W <- embed(a^omega) W;
//   then for all four mu: U_mu(x) <- g U_mu(x), U_mu(x-mu) <- U_mu(x-mu) g^H.
//
// su3_gaugefix_kernel: one thread per (chain, half-site), the site decoding of su3_link_update_kernel.  With even
// extents each link has one end on each parity, so the threads of a launch rewrite every link exactly once and read
// only what they rewrite themselves: in place.  Two passes over the thread's eight links, neither loop unrolled: the
// first sums K (live: K and two links), the second, after the three subgroup steps, multiplies (live: g, the two links
// of a direction, one product).  The second pass reads the links again: the lines are the thread's own of a moment
// ago.  Loading the two links of a direction together is worth 0.22 ms of 1.03 ms per sweep at 8^4 x 256 chains (the
// steps of the loop are a chain of round trips); keeping the next direction's pair in flight as well, or four waves
// per SIMD at one link a time, is worth nothing more (profiles/su3_gaugefix.md).
// su3_gauge_condition_kernel: one thread per site, A being linear, Delta = A(sum_{mu in D} [U_mu(x) - U_mu(x-mu)]).
// su3_gauge_apply_kernel: one thread per (chain, mu, site) as su3_line_extend_kernel.
#include "su3_launch.hpp"
#include "su3_subgroup.hpp"

namespace l2q {

// one subgroup of the local step: g and W both take embed(a^omega) from the left
template <int I, int J>
__device__ __forceinline__ void gf_subgroup(M3& g, M3& w, double omega) {
  Quat rh;
  (void)su2_part_unit(rh, w.re[4 * I], w.im[4 * I], w.re[3 * I + J], w.im[3 * I + J], w.re[3 * J + I],
                      w.im[3 * J + I], w.re[4 * J], w.im[4 * J]);
  const Quat a = q_conj(rh);                           // (1, 0, 0, 0) where |r| is zero or not finite
  const double sv = sqrt(a.q1 * a.q1 + a.q2 * a.q2 + a.q3 * a.q3);
  if (!(sv > 0.0)) return;                             // a_vec = 0: the identity
  const double phi = omega * atan2(sv, a.q0);
  const double f = sin(phi) / sv;
  const Quat p{cos(phi), a.q1 * f, a.q2 * f, a.q3 * f};
  su2_embed_mul<I, J>(g, p);
  su2_embed_mul<I, J>(w, p);
}

// x: the field, read and written by the same thread only (not restrict: both go through it).  gn (may be null)
// G[chain][9][V]; active (may be null) [nb]: a chain with active[c] == 0 is left alone -- the whole block, which
// belongs to one chain.  The kernel has no barrier: threads past the last half-site leave at once.
__global__ __launch_bounds__(kBlock) void su3_gaugefix_kernel(double2* x, double2* gn, const int* __restrict__ active,
                                                              int dirmask, int parity, double omega, int T, int X,
                                                              int Y, int Z, long nblk, int swz) {
  const Dims d{T, X, Y, Z, T * X * Y * Z};
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long c = w / nblk, blk = w % nblk;
  if (active != nullptr && active[c] == 0) return;
  const int V = d.V, vh = V / 2;
  const int h = (int)blk * kBlock + threadIdx.x;
  if (h >= vh) return;
  const int s = checkerboard_site(h, parity, X, Y, Z);
  double2* f = x + c * 36L * V;
  M3 k;
  m3_zero(k);
#pragma unroll 1
  for (int mu = 0; mu < 4; ++mu) {
    if (((dirmask >> mu) & 1) == 0) continue;          // a kernel argument: wave-uniform
    const double2* fm = f + mu * 9 * V;
    M3 a;
    load_link(a, fm, V, s);
    m3_add(k, a);
    load_link_adj(a, fm, V, site_hop(s, stride_of(d, mu), extent_of(d, mu), -1));
    m3_add(k, a);
  }
  M3 g;
  m3_identity(g);
  gf_subgroup<0, 1>(g, k, omega);
  gf_subgroup<0, 2>(g, k, omega);
  gf_subgroup<1, 2>(g, k, omega);
#pragma unroll 1
  for (int mu = 0; mu < 4; ++mu) {
    double2* fm = f + mu * 9 * V;
    const int sm = site_hop(s, stride_of(d, mu), extent_of(d, mu), -1);
    // both links before either store: the compiler cannot know that a store through fm leaves the other link alone
    M3 u, v, o;
    load_link(u, fm, V, s);
    load_link(v, fm, V, sm);
    m3_mul_nn(o, g, u);
    store_link(fm, V, s, o);
    m3_mul_na(o, v, g);
    store_link(fm, V, sm, o);
  }
  if (gn != nullptr) {
    double2* fg = gn + c * 9L * V;
    M3 u, o;
    load_link(u, fg, V, s);
    m3_mul_nn(o, g, u);
    store_link(fg, V, s, o);
  }
}

// partial[c][blk][2]: the block's share of (F, theta), already scaled.  One thread per site.
__global__ __launch_bounds__(kBlock) void su3_gauge_condition_kernel(const double2* __restrict__ xn, int dirmask,
                                                                     double fscale, double tscale, int T, int X,
                                                                     int Y, int Z, long nblk, int swz,
                                                                     double* __restrict__ partial) {
  __shared__ double red[8];
  const Dims d{T, X, Y, Z, T * X * Y * Z};
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long c = w / nblk, blk = w % nblk;
  const int V = d.V;
  const int s0 = (int)blk * kBlock + threadIdx.x;
  const bool live = s0 < V;
  const int s = live ? s0 : 0;
  const double2* f = xn + c * 36L * V;
  M3 sum;
  m3_zero(sum);
  double fr = 0.0;
#pragma unroll 1
  for (int mu = 0; mu < 4; ++mu) {
    if (((dirmask >> mu) & 1) == 0) continue;
    const double2* fm = f + mu * 9 * V;
    M3 a;
    load_link(a, fm, V, s);
    fr += a.re[0] + a.re[4] + a.re[8];
    m3_add(sum, a);
    load_link(a, fm, V, site_hop(s, stride_of(d, mu), extent_of(d, mu), -1));
#pragma unroll
    for (int e = 0; e < 9; ++e) { sum.re[e] -= a.re[e]; sum.im[e] -= a.im[e]; }
  }
  // Delta = (S - S^H) / (2i) - tr / 3: Delta_ij = ((Im S_ij + Im S_ji) - i (Re S_ij - Re S_ji)) / 2
  const double tr3 = (sum.im[0] + sum.im[4] + sum.im[8]) / 3.0;
  double th = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double re = 0.5 * (sum.im[3 * i + j] + sum.im[3 * j + i]) - (i == j ? tr3 : 0.0);
      const double im = -0.5 * (sum.re[3 * i + j] - sum.re[3 * j + i]);
      th = fma(re, re, th); th = fma(im, im, th);
    }
  const double tf = block_sum(live ? fr : 0.0, red);
  const double tt = block_sum(live ? th : 0.0, red + 4);
  if (threadIdx.x == 0) {
    partial[(c * nblk + blk) * 2 + 0] = tf * fscale;
    partial[(c * nblk + blk) * 2 + 1] = tt * tscale;
  }
}

// out_mu(x) = G(x) U_mu(x) G(x+mu)^H; one thread per (chain, mu, site), mu from the block index
__global__ __launch_bounds__(kBlock) void su3_gauge_apply_kernel(const double2* __restrict__ xn,
                                                                 const double2* __restrict__ gn,
                                                                 double2* __restrict__ out, int T, int X, int Y,
                                                                 int Z, long nblk, int swz) {
  const Dims d{T, X, Y, Z, T * X * Y * Z};
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long fi = w / nblk, blk = w % nblk;             // fi = 4 chain + mu
  const int mu = (int)(fi & 3);
  const int s = (int)blk * kBlock + threadIdx.x;
  if (s >= d.V) return;
  const double2* fg = gn + (fi >> 2) * 9L * d.V;
  const long off = fi * 9L * d.V;
  M3 g, u, o;
  load_link(g, fg, d.V, s);
  load_link(u, xn + off, d.V, s);
  m3_mul_nn(o, g, u);
  load_link(g, fg, d.V, site_hop(s, stride_of(d, mu), extent_of(d, mu), +1));
  m3_mul_na(u, o, g);
  store_link(out + off, d.V, s, u);
}

}  // namespace l2q

using namespace l2q;

extern "C" {

int l2q_su3_gaugefix_sweep(void* xn, void* gn, const int* active, int dirmask, int parity, double omega, int nb,
                           int T, int X, int Y, int Z, void* stream) {
  L2Q_REQUIRE(xn, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(gn != xn, L2Q_EINVAL, "gn must not alias xn");
  L2Q_REQUIRE(parity == 0 || parity == 1, L2Q_EINVAL, "parity must be 0 or 1");
  L2Q_REQUIRE(dirmask_ok(dirmask), L2Q_EINVAL, "dirmask must be 1..15 with at least two directions");
  L2Q_REQUIRE(omega >= 1.0 && omega < 2.0, L2Q_EINVAL, "omega must be finite and in [1, 2)");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(all_even(T, X, Y, Z), L2Q_ESHAPE, "a checkerboard update needs even extents");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V / 2, kBlock);
  hipLaunchKernelGGL(su3_gaugefix_kernel, dim3((unsigned)(nb * nblk)), dim3(kBlock), 0, (hipStream_t)stream,
                     (double2*)xn, (double2*)gn, active, dirmask, parity, omega, T, X, Y, Z, nblk,
                     tuning().xcd_swizzle);
  return check_launch("l2q_su3_gaugefix_sweep");
}

int l2q_su3_gauge_condition(const void* xn, int dirmask, double* out, int nb, int T, int X, int Y, int Z, void* ws,
                            size_t ws_bytes, void* stream) {
  L2Q_REQUIRE(xn && out && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(dirmask_ok(dirmask), L2Q_EINVAL, "dirmask must be 1..15 with at least two directions");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V, kBlock);
  L2Q_REQUIRE(ws_bytes >= (size_t)nb * nblk * 2 * sizeof(double), L2Q_ESHAPE, "workspace too small");
  const int nd = dirmask_count(dirmask);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(su3_gauge_condition_kernel, dim3((unsigned)(nb * nblk)), dim3(kBlock), 0, st,
                     (const double2*)xn, dirmask, 1.0 / (3.0 * nd * d.V), 1.0 / (3.0 * d.V), T, X, Y, Z, nblk,
                     tuning().xcd_swizzle, (double*)ws);
  launch_finalize((const double*)ws, out, nb, nblk, 2, 1.0, 0.0, st);
  return check_launch("l2q_su3_gauge_condition");
}

int l2q_su3_gauge_apply(const void* xn, const void* gn, void* out, int nb, int T, int X, int Y, int Z,
                        void* stream) {
  L2Q_REQUIRE(xn && gn && out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(out != xn && out != gn, L2Q_EINVAL, "out must not alias xn or gn");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V, kBlock);
  hipLaunchKernelGGL(su3_gauge_apply_kernel, dim3((unsigned)(nb * 4L * nblk)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const double2*)xn, (const double2*)gn, (double2*)out, T, X, Y, Z, nblk, tuning().xcd_swizzle);
  return check_launch("l2q_su3_gauge_apply");
}

}  // extern "C"
