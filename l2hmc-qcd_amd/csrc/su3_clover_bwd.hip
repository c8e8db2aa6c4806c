// su3_clover_bwd.hip -- VJP of the clover sums of l2q_su3_clover_reduce (su3_flow.hip) with respect to the links.
//
// L = sum_c w[c][0] out[c][0] + w[c][1] out[c][1] + w[c][2] out[c][2] with out = (-sum tr F F,
// -sum tr(F01 F23 - F02 F13 + F03 F12), sum Re tr P).  F = TAH(Q) / 4 and TAH is an orthogonal projector, so per chain
//   dL = -1/4 sum_x sum_{mu<nu} Re tr(G_{mu nu}(x) dQ_{mu nu}(x)) + w2 sum Re tr dP,
//   G_{mu nu} = 2 w0 F_{mu nu} + w1 Fdual_{mu nu}      (anti-Hermitian, traceless; Fdual01 = F23, Fdual02 = -F13, ...)
// Q(x) is four leaves, each a plaquette walked from x; seen from a plaquette, each of its four corners c inserts
// G(c) into the loop at c.  The geometry of that insertion for one link (six plaquettes, four corners each, the sign
// of a leaf's adjoint) and its kernel loop are in su3_clover_insert.hpp, shared with the clover force of
// su3_clover_force.hip; here the cotangent of the link (dL = Re tr(g^H dU)) collects g += B^H, B = the inserted loops of
// -1/4 G plus w2 times the staples.
//
// Two passes, both gathers, no atomics:
//   1. su3_clover_g_kernel: one thread per site, the forward's plane walk (clover_plane); writes -1/4 G as 6 planes
//      x 9 reals per site into the workspace, gw[c][plane][9][V], planes in the forward's order (01) (23) (02) (13)
//      (03) (12).
//   2. su3_clover_bwd_kernel: one thread per link, gx += the 6 x 4 inserted loops and the 6 staples.
// A thread's arithmetic depends on its chain, its link and the lattice only: a chain gives the same bits alone
// and in a batch, and from run to run.
#include "su3_clover_insert.hpp"
#include "su3_launch.hpp"

namespace l2q {

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
// The insertion loop, its operand discipline and the plane order: clover_insert_link (su3_clover_insert.hpp), which
// the clover force of su3_clover_force.hip shares.
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
  const double* gc = gw + c * (long)kCloverGReals * V;
  M3 acc;
  clover_insert_link(acc, xc, gc, w[c * 3 + 2], d, s, mu);
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
