// su3_clover_bwd.hip -- VJP of the clover sums of l2q_su3_clover_reduce (su3_flow.hip) with respect to the links.
//
// L = sum_c w[c][0] out[c][0] + w[c][1] out[c][1] + w[c][2] out[c][2] with out = (-sum tr F F,
// -sum tr(F01 F23 - F02 F13 + F03 F12), sum Re tr P).  F = TAH(Q) / 4 and TAH is an orthogonal projector, so per chain
//   dL = -1/4 sum_x sum_{mu<nu} Re tr(G_{mu nu}(x) dQ_{mu nu}(x)) + w2 sum Re tr dP,
//   G_{mu nu} = 2 w0 F_{mu nu} + w1 Fdual_{mu nu}      (anti-Hermitian, traceless; Fdual01 = F23, Fdual02 = -F13, ...)
// Q(x) is four leaves, each a plaquette walked from x; seen from a plaquette, each of its four corners c inserts
// G(c) into the loop at c.  A link U = U_mu(y) lies on six plaquettes (three nu, up and down).  Written as the loop
// that STARTS with the link, U A2 A3 A4 with the corners c1, c2, c3 after U, A2, A3 and c0 = y,
//   up:   A2 = U_nu(y+mu)       A3 = U_mu(y+nu)^H  A4 = U_nu(y)^H     c = y, y+mu, y+mu+nu, y+nu
//   down: A2 = U_nu(y+mu-nu)^H  A3 = U_mu(y-nu)^H  A4 = U_nu(y-nu)    c = y, y+mu, y+mu-nu, y-nu
// its terms are Re tr(U B), B = G1 S + A2 G2 A3 A4 + A2 A3 G3 A4 + S G0, S = A2 A3 A4 (the staple), and the
// cotangent of the link (dL = Re tr(g^H dU)) collects
//   g += (sigma (-1/4) B + w2 S)^H,    sigma = +1 where the loop runs counter-clockwise in its plane (mu < nu up,
//                                      mu > nu down), -1 where it is a leaf's adjoint: Re tr(G L^H) = -Re tr(G L).
// With extents 1 and 2 several of these operands are the same link; every geometric occurrence is its own term
// here, as it is in the forward.
//
// Two passes, both gathers, no atomics:
//   1. su3_clover_g_kernel: one thread per site, the forward's plane walk (clover_plane); writes -1/4 G as 6 planes
//      x 9 reals per site into the workspace, gw[c][plane][9][V], planes in the forward's order (01) (23) (02) (13)
//      (03) (12).
//   2. su3_clover_bwd_kernel: one thread per link, gx += the 6 x 4 inserted loops and the 6 staples.
// A thread's arithmetic depends on its chain, its link and the lattice only: a chain gives the same bits alone
// and in a batch, and from run to run.
#include "su3_clover.hpp"
#include "su3_launch.hpp"

namespace l2q {

constexpr int kCloverGReals = 6 * 9;      // reals of -1/4 G per site in the workspace

__device__ __forceinline__ void store_ah3(double* __restrict__ g, int V, int s, const AH3& a) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    g[i * V + s] = a.d[i]; g[(3 + i) * V + s] = a.re[i]; g[(6 + i) * V + s] = a.im[i];
  }
}

// the full matrix of an anti-Hermitian field stored as AH3 reals
__device__ __forceinline__ void load_ah3(M3& m, const double* __restrict__ g, int V, int s) {
  m.re[0] = 0.0; m.re[4] = 0.0; m.re[8] = 0.0;
  m.im[0] = g[s]; m.im[4] = g[V + s]; m.im[8] = g[2 * V + s];
  const double r0 = g[3 * V + s], r1 = g[4 * V + s], r2 = g[5 * V + s];
  const double i0 = g[6 * V + s], i1 = g[7 * V + s], i2 = g[8 * V + s];
  m.re[1] = r0; m.im[1] = i0; m.re[3] = -r0; m.im[3] = i0;
  m.re[2] = r1; m.im[2] = i1; m.re[6] = -r1; m.im[6] = i1;
  m.re[5] = r2; m.im[5] = i2; m.re[7] = -r2; m.im[7] = i2;
}

// a f + b g
__device__ __forceinline__ AH3 ah3_comb(double a, const AH3& f, double b, const AH3& g) {
  AH3 o;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    o.d[i] = a * f.d[i] + b * g.d[i]; o.re[i] = a * f.re[i] + b * g.re[i]; o.im[i] = a * f.im[i] + b * g.im[i];
  }
  return o;
}

// ------------------------------------------------------------------ pass 1: -1/4 G
// The walk of su3_clover_kernel: planes in dual pairs, the plane loop not unrolled, extents as scalar arguments.
__global__ __launch_bounds__(kBlock, 2) void su3_clover_g_kernel(const double2* __restrict__ xn,
                                                                const double* __restrict__ w, int T, int X, int Y,
                                                                int Z, long nblk, int swz, int lo,
                                                                double* __restrict__ gw) {
  const Dims d{T, X, Y, Z, T * X * Y * Z};
  const long wk = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long c = wk / nblk, blk = wk % nblk;
  const int s = (int)blk * kBlock + threadIdx.x;
  if (s >= d.V) return;
  const int V = d.V;
  const double2* xc = xn + c * 36L * V;
  double* gc = gw + c * (long)kCloverGReals * V;
  const double a0 = -0.5 * w[c * 3 + 0], a1 = -0.25 * w[c * 3 + 1];
  const bool go = s >= lo;
  const auto ld = [=](M3& m, int dir, int site) { load_link(m, xc + dir * 9 * V, V, site); };
  AH3 f = {};
  double sp = 0.0;
#pragma unroll 1
  for (int pl = 0; pl < 6; ++pl) {
    const int k = (pl >> 1) + 1;
    const int mu = (pl & 1) ? (k == 1 ? 2 : 1) : 0;
    const int nu = (pl & 1) ? (k == 3 ? 2 : 3) : k;
    const int cmu = (s / stride_of(d, mu)) % extent_of(d, mu), cnu = (s / stride_of(d, nu)) % extent_of(d, nu);
    CloverSites<int> st;
    st.o = s;
    st.pm = fwd(s, cmu, d, mu); st.mm = bwd(s, cmu, d, mu);
    st.pn = fwd(s, cnu, d, nu); st.mn = bwd(s, cnu, d, nu);
    st.mm_pn = fwd(st.mm, cnu, d, nu); st.mm_mn = bwd(st.mm, cnu, d, nu);
    st.pm_mn = bwd(st.pm, cnu, d, nu);
    AH3 g;
    clover_plane(g, sp, ld, st, mu, nu, go);
    if (pl & 1) {
      // f = F_{0k}, g = its dual plane's F; eps_{0 k a b} = +, -, +
      const double e1 = (k == 2) ? -a1 : a1;
      store_ah3(gc + (pl - 1) * 9L * V, V, s, ah3_comb(a0, f, e1, g));
      store_ah3(gc + pl * 9L * V, V, s, ah3_comb(a0, g, e1, f));
    }
    f = g;
  }
}

// ------------------------------------------------------------------ pass 2: one thread per link
// Operand loads are tied to the product before them with site_after (su3_links.hpp).  Without it hipcc starts all of
// a loop's operands (3 links, 4 G) ahead of the first product and spills 68 registers; the always-taken conditional
// of clover_plane does not stop it here.  With it one operand is in flight next to the live matrices: 210 registers,
// no spill.
// acc += sg (G1 S + A2 (G2 A3 A4 + A3 (G3 A4 + A4 G0))) + w2 S: eight products, at most four matrices live next to
// acc.  LDA2 / LDA3 / LDA4 load the three links of the staple (adjoint where the loop walks them backwards) once
// their second argument exists, gp is the plane of -1/4 G, c0..c3 the corners.
#define L2Q_CLOVER_BWD_LOOP(LDA2, LDA3, LDA4, c0, c1, c2, c3)                                \
  {                                                                                          \
    M3 a, g, wm, t34, xm;                                                                    \
    LDA4(a, 0.0); load_ah3(g, gp, V, c3); m3_mul_nn(wm, g, a);                               \
    load_ah3(g, gp, V, site_after(c0, wm.im[8])); m3_mac_nn(wm, a, g);                       \
    LDA3(g, wm.im[8]); m3_mul_nn(t34, g, a);                                                 \
    m3_mul_nn(xm, g, wm);                                                                    \
    load_ah3(g, gp, V, site_after(c2, xm.im[8])); m3_mac_nn(xm, g, t34);                     \
    LDA2(a, xm.im[8]); m3_mul_nn(wm, a, xm);                                                 \
    m3_mul_nn(g, a, t34);                                                                    \
    load_ah3(a, gp, V, site_after(c1, g.im[8])); m3_mac_nn(wm, a, g);                        \
    _Pragma("unroll") for (int e = 0; e < 9; ++e) {                                          \
      acc.re[e] += sg * wm.re[e] + w2 * g.re[e];                                             \
      acc.im[e] += sg * wm.im[e] + w2 * g.im[e];                                             \
    }                                                                                        \
  }

// The direction loop is not unrolled and the extents are scalar arguments (see su3_clover_kernel); mu comes from the
// block index, so it is wave-uniform.
__global__ __launch_bounds__(kBlock, 2) void su3_clover_bwd_kernel(const double2* __restrict__ xn,
                                                                  const double* __restrict__ w,
                                                                  const double* __restrict__ gw, int T, int X,
                                                                  int Y, int Z, long nblk, int swz, double2* gx) {
  const Dims d{T, X, Y, Z, T * X * Y * Z};
  const long wk = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const int mu = (int)(wk & 3);
  const long cb = wk >> 2;
  const long c = cb / nblk, blk = cb % nblk;
  const int s = (int)blk * kBlock + threadIdx.x;
  if (s >= d.V) return;
  const int V = d.V;
  const double2* xc = xn + c * 36L * V;
  const double2* fm = xc + mu * 9 * V;
  const double* gc = gw + c * (long)kCloverGReals * V;
  const double w2 = w[c * 3 + 2];
  const int s_pmu = fwd(s, (s / stride_of(d, mu)) % extent_of(d, mu), d, mu);
  M3 acc;
  m3_zero(acc);
#pragma unroll 1
  for (int j = 0; j < 3; ++j) {
    const int nu = j + (j >= mu ? 1 : 0);
    const double2* fn = xc + nu * 9 * V;
    // the plane of (mu, nu) in pass 1's order: (0, k) -> 2 (k - 1), the spatial plane dual to (0, k) -> 2 (k - 1) + 1
    const int lo_d = mu < nu ? mu : nu, hi_d = mu < nu ? nu : mu;
    const int pl = lo_d == 0 ? 2 * (hi_d - 1) : 2 * (6 - lo_d - hi_d) - 1;
    const double* gp = gc + pl * 9L * V;
    const int cnu = (s / stride_of(d, nu)) % extent_of(d, nu);
    const int s_pnu = fwd(s, cnu, d, nu), s_mnu = bwd(s, cnu, d, nu);
    const int s_pmu_pnu = fwd(s_pmu, cnu, d, nu), s_pmu_mnu = bwd(s_pmu, cnu, d, nu);
    double sg = mu < nu ? 1.0 : -1.0;
#define L2Q_UP_A2(m, dep) load_link(m, fn, V, site_after(s_pmu, dep))
#define L2Q_UP_A3(m, dep) load_link_adj(m, fm, V, site_after(s_pnu, dep))
#define L2Q_UP_A4(m, dep) load_link_adj(m, fn, V, site_after(s, dep))
    L2Q_CLOVER_BWD_LOOP(L2Q_UP_A2, L2Q_UP_A3, L2Q_UP_A4, s, s_pmu, s_pmu_pnu, s_pnu)
    sg = -sg;
#define L2Q_DN_A2(m, dep) load_link_adj(m, fn, V, site_after(s_pmu_mnu, dep))
#define L2Q_DN_A3(m, dep) load_link_adj(m, fm, V, site_after(s_mnu, dep))
#define L2Q_DN_A4(m, dep) load_link(m, fn, V, site_after(s_mnu, dep))
    L2Q_CLOVER_BWD_LOOP(L2Q_DN_A2, L2Q_DN_A3, L2Q_DN_A4, s, s_pmu, s_pmu_mnu, s_mnu)
  }
  // g += acc^H
  double2* o = gx + (c * 4 + mu) * 9L * V;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double2 r = o[(3 * i + k) * (long)V + s];
      r.x += acc.re[3 * k + i]; r.y -= acc.im[3 * k + i];
      o[(3 * i + k) * (long)V + s] = r;
    }
}

}  // namespace l2q

using namespace l2q;

extern "C" {

int l2q_su3_clover_bwd(const void* xn, const double* w, void* gx, int nb, int T, int X, int Y, int Z, void* ws,
                       size_t ws_bytes, void* stream) {
  L2Q_REQUIRE(xn && w && gx && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(gx != xn && ws != xn && ws != gx, L2Q_EINVAL, "xn, gx and ws must be three different buffers");
  const Dims d = make_dims(T, X, Y, Z);
  L2Q_REQUIRE(ws_bytes >= (size_t)nb * kCloverGReals * (size_t)d.V * sizeof(double), L2Q_ESHAPE,
              "workspace too small");
  const long nblk = cdiv(d.V, kBlock);
  hipStream_t st = (hipStream_t)stream;
  const int swz = tuning().xcd_swizzle;
  hipLaunchKernelGGL(su3_clover_g_kernel, dim3((unsigned)(nb * nblk)), dim3(kBlock), 0, st, (const double2*)xn, w, T,
                     X, Y, Z, nblk, swz, 0, (double*)ws);
  hipLaunchKernelGGL(su3_clover_bwd_kernel, dim3((unsigned)(nb * nblk * 4)), dim3(kBlock), 0, st, (const double2*)xn,
                     w, (const double*)ws, T, X, Y, Z, nblk, swz, (double2*)gx);
  return check_launch("l2q_su3_clover_bwd");
}

}  // extern "C"
