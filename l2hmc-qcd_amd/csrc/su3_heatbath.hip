// su3_heatbath.hip -- local updates of the Wilson action: Cabibbo-Marinari heatbath with Kennedy-Pendleton SU(2)
// sampling, and microcanonical overrelaxation, on one checkerboard of one direction per launch.
//
//   A = A_mu(x): the six staples in the convention of l2q_su3_force; the link's share of the action is
//   -(beta / 3) Re tr(U A).  For the SU(2) subgroups (i, j) = (0,1), (0,2), (1,2), with W = U A formed anew for each:
//     r = ( Re(W_ii + W_jj), Im(W_ij + W_ji), Re(W_ij - W_ji), Im(W_ii - W_jj) ) / 2,  k = |r|,  rh = r / k
//   A quaternion a is the block [[a0 + i a3, a2 + i a1], [-a2 + i a1, a0 - i a3]] at rows / columns i, j, so that
//   Re tr(embed(a) W) = const + 2 k (a rh)_0.
//     overrelaxation: a = conj(rh) conj(rh)                        (Re tr(U A) unchanged)
//     heatbath:       a = b conj(rh), b0 ~ sqrt(1 - b0^2) exp(alpha b0), alpha = 2 beta k / 3, direction uniform
//   and U <- embed(a) U.
//
// One thread per (chain, half-site): the launch writes U_mu at the sites of one parity and, with all extents even,
// reads besides them only links of other directions and mu-links of the other parity (the staples hold mu-links at
// x +- nu only), so the update is in place.  mu and parity are kernel arguments: wave-uniform.  The staple loop is
// not unrolled (live set: the sum, one product and two operands); the coordinates come by division as in
// su3_loops.hip.  The kernel holds no generator: the uniforms are an input, u[chain][subgroup][4 ntry + 2][V/2].
#include "su3_launch.hpp"
#include "su3_subgroup.hpp"

namespace l2q {

constexpr double kTwoPi = 6.283185307179586476925286766559;

// entry (R, C) of U A
template <int R, int C>
__device__ __forceinline__ void ua_entry(double& wr, double& wi, const M3& u, const M3& a) {
  double sr = 0.0, si = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double ur = u.re[3 * R + k], ui = u.im[3 * R + k];
    const double ar = a.re[3 * k + C], ai = a.im[3 * k + C];
    sr = fma(ur, ar, sr); sr = fma(-ui, ai, sr);
    si = fma(ur, ai, si); si = fma(ui, ar, si);
  }
  wr = sr; wi = si;
}

// Kennedy-Pendleton: the first of ntry proposals that is accepted gives b; false when none is.  ub: the uniforms of
// this (chain, subgroup, half-site), row stride vh.  The trip count is fixed and a try runs only while nothing is accepted.
__device__ __forceinline__ bool kp_sample(Quat& b, double alpha, const double* __restrict__ ub, long vh, int ntry) {
  bool done = false;
  double b0 = 1.0;
#pragma unroll 1
  for (int t = 0; t < ntry; ++t) {
    if (!done) {
      const double v1 = 1.0 - ub[(4 * t + 0) * vh], v2 = 1.0 - ub[(4 * t + 1) * vh];
      const double v3 = 1.0 - ub[(4 * t + 2) * vh], v4 = 1.0 - ub[(4 * t + 3) * vh];
      const double c = cos(kTwoPi * v2);
      const double delta = -(log(v1) + c * c * log(v3)) / alpha;
      if (v4 * v4 <= 1.0 - 0.5 * delta) { done = true; b0 = 1.0 - delta; }
    }
  }
  if (done) {
    const double v5 = 1.0 - ub[(4 * ntry + 0) * vh], v6 = 1.0 - ub[(4 * ntry + 1) * vh];
    const double ct = 1.0 - 2.0 * v5, phi = kTwoPi * v6;
    const double st = sqrt(fmax(0.0, 1.0 - ct * ct));
    const double n = sqrt(fmax(0.0, 1.0 - b0 * b0));
    b.q0 = b0; b.q1 = n * st * cos(phi); b.q2 = n * st * sin(phi); b.q3 = n * ct;
  }
  return done;
}

// one SU(2) subgroup of one link; returns 1 when the heatbath found no acceptable proposal (u then stays as it is)
template <bool HB, int I, int J>
__device__ __forceinline__ int subgroup_update(M3& u, const M3& a, double beta, const double* __restrict__ ub, long vh,
                                               int ntry) {
  double iir, iii, ijr, iji, jir, jii, jjr, jji;
  ua_entry<I, I>(iir, iii, u, a);
  ua_entry<I, J>(ijr, iji, u, a);
  ua_entry<J, I>(jir, jii, u, a);
  ua_entry<J, J>(jjr, jji, u, a);
  const double r0 = 0.5 * (iir + jjr), r1 = 0.5 * (iji + jii), r2 = 0.5 * (ijr - jir), r3 = 0.5 * (iii - jji);
  const double k = sqrt(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
  Quat rh{1.0, 0.0, 0.0, 0.0};
  if (k > 0.0 && k <= 1.7976931348623157e308) { rh.q0 = r0 / k; rh.q1 = r1 / k; rh.q2 = r2 / k; rh.q3 = r3 / k; }
  const Quat rc = q_conj(rh);
  Quat g;
  if (HB) {
    Quat b;
    if (!kp_sample(b, 2.0 * beta * k / 3.0, ub, vh, ntry)) return 1;
    g = q_mul(b, rc);
  } else {
    g = q_mul(rc, rc);
  }
  // rows I and J of embed(g) u
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double xr = u.re[3 * I + c], xi = u.im[3 * I + c], yr = u.re[3 * J + c], yi = u.im[3 * J + c];
    u.re[3 * I + c] = g.q0 * xr - g.q3 * xi + g.q2 * yr - g.q1 * yi;
    u.im[3 * I + c] = g.q0 * xi + g.q3 * xr + g.q2 * yi + g.q1 * yr;
    u.re[3 * J + c] = -g.q2 * xr - g.q1 * xi + g.q0 * yr + g.q3 * yi;
    u.im[3 * J + c] = -g.q2 * xi + g.q1 * xr + g.q0 * yi - g.q3 * yr;
  }
  return 0;
}

// xr and xw are the same field: read through xr, the thread's own link written through xw.  partial[c][blk] (HB with
// a failure count asked for): the block's number of (link, subgroup) failures.
template <bool HB>
__global__ __launch_bounds__(kBlock) void su3_link_update_kernel(const double2* xr, double2* xw, double beta, int mu,
                                                                 int parity, const double* __restrict__ u, int ntry,
                                                                 int T, int X, int Y, int Z, long nblk, int swz,
                                                                 double* __restrict__ partial) {
  __shared__ double red[4];
  const Dims d{T, X, Y, Z, T * X * Y * Z};
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long c = w / nblk, blk = w % nblk;
  const int V = d.V, vh = V / 2;
  const int h0 = (int)blk * kBlock + threadIdx.x;
  const bool live = h0 < vh;
  const int h = live ? h0 : 0;
  const int s = checkerboard_site(h, parity, X, Y, Z);
  const double2* f = xr + c * 36L * V;
  const int stm = stride_of(d, mu), em = extent_of(d, mu);
  const int s_pm = site_hop(s, stm, em, +1);
  M3 acc;
  m3_zero(acc);
#pragma unroll 1
  for (int j = 0; j < 3; ++j) {
    const int nu = j + (j >= mu ? 1 : 0);
    const int stn = stride_of(d, nu), en = extent_of(d, nu);
    const double2* fm = f + mu * 9 * V;
    const double2* fn = f + nu * 9 * V;
    M3 a, b, t;
    // up:   U_nu(x+mu) U_mu(x+nu)^H U_nu(x)^H
    load_link(a, fn, V, s_pm);
    load_link(b, fm, V, site_hop(s, stn, en, +1));
    m3_mul_na(t, a, b);
    load_link(a, fn, V, s);
    m3_mac_na(acc, t, a);
    // down: U_nu(x+mu-nu)^H U_mu(x-nu)^H U_nu(x-nu)
    const int s_mn = site_hop(s, stn, en, -1);
    load_link(a, fn, V, site_hop(s_pm, stn, en, -1));
    load_link(b, fm, V, s_mn);
    m3_mul_aa(t, a, b);
    load_link(a, fn, V, s_mn);
    m3_mac_nn(acc, t, a);
  }
  M3 uu;
  load_link(uu, f + mu * 9 * V, V, s);
  const double* ub = HB ? u + c * 3L * (4 * ntry + 2) * vh + h : nullptr;
  const long sg = (long)(4 * ntry + 2) * vh;
  int nf = 0;
  nf += subgroup_update<HB, 0, 1>(uu, acc, beta, ub, vh, ntry);
  nf += subgroup_update<HB, 0, 2>(uu, acc, beta, HB ? ub + sg : nullptr, vh, ntry);
  nf += subgroup_update<HB, 1, 2>(uu, acc, beta, HB ? ub + 2 * sg : nullptr, vh, ntry);
  if (live) store_link(xw + c * 36L * V + mu * 9 * V, V, s, uu);
  if (HB && partial != nullptr) {                      // a kernel argument: the whole block takes the same way
    const double tot = block_sum(live ? (double)nf : 0.0, red);
    if (threadIdx.x == 0) partial[c * nblk + blk] = tot;
  }
}

}  // namespace l2q

using namespace l2q;

extern "C" {

int l2q_su3_heatbath(void* xn, double beta, int mu, int parity, const double* u, int ntry, double* fails, int nb,
                     int T, int X, int Y, int Z, void* ws, size_t ws_bytes, void* stream) {
  L2Q_REQUIRE(xn && u, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(fails == nullptr || ws != nullptr, L2Q_EINVAL, "null pointer (failure counts need a workspace)");
  L2Q_REQUIRE(mu >= 0 && mu < 4, L2Q_EINVAL, "direction mu must be 0..3");
  L2Q_REQUIRE(parity == 0 || parity == 1, L2Q_EINVAL, "parity must be 0 or 1");
  L2Q_REQUIRE(ntry >= 1 && ntry <= 16, L2Q_EINVAL, "ntry must be 1..16");
  L2Q_REQUIRE(beta > 0.0 && beta <= 1.7976931348623157e308, L2Q_EINVAL, "beta must be positive and finite");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(all_even(T, X, Y, Z), L2Q_ESHAPE, "a checkerboard update needs even extents");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V / 2, kBlock);
  L2Q_REQUIRE(fails == nullptr || ws_bytes >= (size_t)nb * nblk * sizeof(double), L2Q_ESHAPE, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(su3_link_update_kernel<true>, dim3((unsigned)(nb * nblk)), dim3(kBlock), 0, st,
                     (const double2*)xn, (double2*)xn, beta, mu, parity, u, ntry, T, X, Y, Z, nblk,
                     tuning().xcd_swizzle, fails ? (double*)ws : nullptr);
  if (fails) launch_finalize((const double*)ws, fails, nb, nblk, 1, 1.0, 0.0, st);
  return check_launch("l2q_su3_heatbath");
}

int l2q_su3_overrelax(void* xn, int mu, int parity, int nb, int T, int X, int Y, int Z, void* stream) {
  L2Q_REQUIRE(xn, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(mu >= 0 && mu < 4, L2Q_EINVAL, "direction mu must be 0..3");
  L2Q_REQUIRE(parity == 0 || parity == 1, L2Q_EINVAL, "parity must be 0 or 1");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(all_even(T, X, Y, Z), L2Q_ESHAPE, "a checkerboard update needs even extents");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V / 2, kBlock);
  hipLaunchKernelGGL(su3_link_update_kernel<false>, dim3((unsigned)(nb * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, (const double2*)xn, (double2*)xn, 0.0, mu, parity, (const double*)nullptr, 0,
                     T, X, Y, Z, nblk, tuning().xcd_swizzle, (double*)nullptr);
  return check_launch("l2q_su3_overrelax");
}

}  // extern "C"
