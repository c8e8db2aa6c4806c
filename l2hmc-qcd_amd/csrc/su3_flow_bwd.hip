// su3_flow_bwd.hip -- the reverse sweep of the Wilson flow (su3_flow.hip): the full VJP of the staple force, and on
// top of it the reverse of one flow stage and of one third-order flow step.
//
// l2q_su3_force_vjp.  F_l = (beta/3) TAH(U_l A_l(U)) with A the six staples, g_F its cotangent.  TAH is a
// self-adjoint projector under Re tr(a^H b), so with K_l = (beta/3) TAH(g_F,l) (anti-Hermitian, traceless)
//   L = sum_l Re tr(K_l^H U_l A_l) = -sum_l sum_{plaquettes through l} Re tr(K_l P),   P the plaquette walked from
// the base of l, starting with l.  A plaquette occurs four times, once for each of its links, walked in the sense in
// which that link runs forwards.  Seen from the link U = U_mu(y) and written as the loop U A2 A3 A4 that starts with
// it (the corners and the staples A2 A3 A4 of su3_clover_bwd.hip), every occurrence is this loop or its adjoint with
// one K inserted, and Re tr(K M^H) = -Re tr(K M) brings the adjoints back to it: a link walked forwards inserts +K at
// its base, a link walked backwards -K at its base.  With T = TAH(g_F):
//   up   (A2 = U_nu(y+mu), A3 = U_mu(y+nu)^H, A4 = U_nu(y)^H):
//        B = A2 A3 (A4 (T_mu(y) - T_nu(y)) - T_mu(y+nu) A4) + T_nu(y+mu) A2 A3 A4
//   down (A2 = U_nu(y+mu-nu)^H, A3 = U_mu(y-nu)^H, A4 = U_nu(y-nu)):
//        B = A2 (A3 ((T_nu(y-nu) - T_mu(y-nu)) A4 + A4 T_mu(y)) - T_nu(y+mu-nu) A3 A4)
// L = -(beta/3) sum Re tr(U B) over the six loops of the link, and its cotangent (dL = Re tr(g^H dU)) collects
//   g -= (beta/3) B^H.
// The terms A4 T_mu(y) alone are the staples-constant VJP of l2q_su3_force_bwd, (beta/3) T A^H.  With extents 1 and 2
// several operands are the same link; every geometric occurrence is its own term, as in the forward.
//
// One thread per link, a gather, no atomics: a thread's arithmetic depends on its chain, its link and the lattice
// only, so a chain gives the same bits alone and in a batch, and from run to run.
#include "su3_clover.hpp"
#include "su3_launch.hpp"

namespace l2q {

// sg TAH(g) of the cotangent g at site s, as a full matrix: anti-Hermitian, so the strict upper triangle and the
// imaginary diagonal determine it
__device__ __forceinline__ void fv_load_tah(M3& m, const double2* __restrict__ f, int V, int s, double sg) {
  const double h = 0.5 * sg;
  const double d0 = f[s].y, d1 = f[4 * V + s].y, d2 = f[8 * V + s].y;
  const double t3 = (d0 + d1 + d2) * (1.0 / 3.0);
  m.re[0] = 0.0; m.re[4] = 0.0; m.re[8] = 0.0;
  m.im[0] = sg * (d0 - t3); m.im[4] = sg * (d1 - t3); m.im[8] = sg * (d2 - t3);
#define L2Q_FV_OFF(U, L)                                                  \
  {                                                                       \
    const double2 a = f[U * V + s], b = f[L * V + s];                     \
    const double r = h * (a.x - b.x), i = h * (a.y + b.y);                \
    m.re[U] = r; m.im[U] = i; m.re[L] = -r; m.im[L] = i;                  \
  }
  L2Q_FV_OFF(1, 3) L2Q_FV_OFF(2, 6) L2Q_FV_OFF(5, 7)
#undef L2Q_FV_OFF
}

// The direction loop is not unrolled and the extents are scalar arguments (see su3_clover_kernel); mu comes from the
// block index, so it is wave-uniform.  Every operand load is tied to the product before it (site_after), the second
// of two insertions at one corner to the first: one operand in flight next to the live matrices, 234 registers, no
// spill.
__global__ __launch_bounds__(kBlock, 2) void su3_force_vjp_kernel(const double2* __restrict__ xn,
                                                                 const double2* __restrict__ gf, double coef, int T,
                                                                 int X, int Y, int Z, long nblk, int swz,
                                                                 double2* gx) {
  const Dims d{T, X, Y, Z, T * X * Y * Z};
  const long wk = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const int mu = (int)(wk & 3);
  const long cb = wk >> 2;
  const long c = cb / nblk, blk = cb % nblk;
  const int s = (int)blk * kBlock + threadIdx.x;
  if (s >= d.V) return;
  const int V = d.V;
  const double2* xc = xn + c * 36L * V;
  const double2* gc = gf + c * 36L * V;
  const double2* fm = xc + mu * 9 * V;
  const double2* tm = gc + mu * 9 * V;
  const int s_pmu = fwd(s, (s / stride_of(d, mu)) % extent_of(d, mu), d, mu);
  M3 acc;
  m3_zero(acc);
#pragma unroll 1
  for (int j = 0; j < 3; ++j) {
    const int nu = j + (j >= mu ? 1 : 0);
    const double2* fn = xc + nu * 9 * V;
    const double2* tn = gc + nu * 9 * V;
    const int cnu = (s / stride_of(d, nu)) % extent_of(d, nu);
    const int s_pnu = fwd(s, cnu, d, nu), s_mnu = bwd(s, cnu, d, nu);
    const int s_pmu_mnu = bwd(s_pmu, cnu, d, nu);
    {  // up: seven products, at most four matrices live next to acc
      M3 a, g, wm, t34, xm;
      load_link_adj(a, fn, V, s);                                                  // A4
      fv_load_tah(g, tm, V, s_pnu, -1.0); m3_mul_nn(wm, g, a);                   // -T_mu(y+nu) A4
      fv_load_tah(g, tm, V, site_after(s, wm.im[8]), 1.0);
      fv_load_tah(xm, tn, V, site_after(s, g.im[8]), -1.0);
      m3_add(g, xm); m3_mac_nn(wm, a, g);                                        // + A4 (T_mu(y) - T_nu(y))
      load_link_adj(g, fm, V, site_after(s_pnu, wm.im[8]));                          // A3
      m3_mul_nn(t34, g, a);
      m3_mul_nn(xm, g, wm);
      load_link(a, fn, V, site_after(s_pmu, xm.im[8]));                            // A2
      m3_mul_nn(wm, a, xm);
      m3_mul_nn(g, a, t34);                                                      // the staple
      fv_load_tah(a, tn, V, site_after(s_pmu, g.im[8]), 1.0); m3_mac_nn(wm, a, g); // + T_nu(y+mu) A2 A3 A4
      m3_add(acc, wm);
    }
    {  // down: six products
      M3 a, g, wm, t34, xm;
      load_link(a, fn, V, site_after(s_mnu, acc.im[8]));                           // A4
      fv_load_tah(g, tn, V, site_after(s_mnu, acc.im[8]), 1.0);
      fv_load_tah(xm, tm, V, site_after(s_mnu, g.im[8]), -1.0);
      m3_add(g, xm); m3_mul_nn(wm, g, a);                                        // (T_nu(y-nu) - T_mu(y-nu)) A4
      fv_load_tah(g, tm, V, site_after(s, wm.im[8]), 1.0); m3_mac_nn(wm, a, g);    // + A4 T_mu(y)
      load_link_adj(g, fm, V, site_after(s_mnu, wm.im[8]));                          // A3
      m3_mul_nn(t34, g, a);
      m3_mul_nn(xm, g, wm);
      fv_load_tah(g, tn, V, site_after(s_pmu_mnu, xm.im[8]), -1.0); m3_mac_nn(xm, g, t34);  // - T_nu(y+mu-nu) A3 A4
      load_link_adj(a, fn, V, site_after(s_pmu_mnu, xm.im[8]));                      // A2
      m3_mul_nn(wm, a, xm);
      m3_add(acc, wm);
    }
  }
  // g -= coef acc^H
  double2* o = gx + (c * 4 + mu) * 9L * V;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double2 r = o[(3 * i + k) * (long)V + s];
      r.x -= coef * acc.re[3 * k + i]; r.y += coef * acc.im[3 * k + i];
      o[(3 * i + k) * (long)V + s] = r;
    }
}

// bytes of one field of links
inline size_t fv_field_bytes(int nb, long V) { return (size_t)nb * 36 * (size_t)V * sizeof(double2); }
// bytes a stage's reverse needs: deps [nb] of l2q_su3_expm_mul_bwd (dropped) and that call's own workspace
inline size_t fv_stage_ws_bytes(int nb, long V) { return (size_t)nb * (1 + 4 * (size_t)cdiv(V, kBlock)) * sizeof(double); }

}  // namespace l2q

using namespace l2q;

extern "C" {

int l2q_su3_force_vjp(const void* xn, const void* gf, double beta, void* gx, int nb, int T, int X, int Y, int Z,
                      void* stream) {
  L2Q_REQUIRE(xn && gf && gx, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(gx != xn && gx != gf, L2Q_EINVAL, "gx must alias neither xn nor gf");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V, kBlock);
  hipLaunchKernelGGL(su3_force_vjp_kernel, dim3((unsigned)(nb * nblk * 4)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const double2*)xn, (const double2*)gf, beta / 3.0, T, X, Y, Z, nblk, tuning().xcd_swizzle,
                     (double2*)gx);
  return check_launch("l2q_su3_force_vjp");
}

size_t l2q_su3_flow_stage_bwd_ws_bytes(int nb, int T, int X, int Y, int Z) {
  if (!su3_dims_ok(nb, T, X, Y, Z)) return 0;
  return fv_stage_ws_bytes(nb, (long)T * X * Y * Z);
}

int l2q_su3_flow_stage_bwd(const void* x_in, const void* p_out, double c, double s, const void* gx_out, void* gp,
                           void* gx_in, int nb, int T, int X, int Y, int Z, void* ws, size_t ws_bytes,
                           void* stream) {
  L2Q_REQUIRE(x_in && p_out && gx_out && gp && gx_in && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(gx_in != x_in && gx_in != p_out && gx_in != gp && gx_in != gx_out, L2Q_EINVAL,
              "gx_in must alias no other field");
  L2Q_REQUIRE(gp != x_in && gp != p_out && gp != gx_out, L2Q_EINVAL, "gp must alias no other field");
  const long V = (long)T * X * Y * Z;
  L2Q_REQUIRE(ws_bytes >= fv_stage_ws_bytes(nb, V), L2Q_ESHAPE, "workspace too small");
  // X_out = exp(s P_out) X_in: gx_in = its cotangent of X_in, gp += its cotangent of P_out; dL/ds is dropped
  double* deps = (double*)ws;
  int rc = l2q_su3_expm_mul_bwd(x_in, p_out, s, nullptr, 0, gx_out, gx_in, gp, deps, nb, V, deps + nb,
                                ws_bytes - (size_t)nb * sizeof(double), stream);
  if (rc != L2Q_OK) return rc;
  // P_out = P_in + c TAH(U A): the force at beta = 3 c, its cotangent gp; P_in enters with weight 1, so gp stays
  return l2q_su3_force_vjp(x_in, gp, 3.0 * c, gx_in, nb, T, X, Y, Z, stream);
}

size_t l2q_su3_flow_step_bwd_ws_bytes(int nb, int T, int X, int Y, int Z) {
  if (!su3_dims_ok(nb, T, X, Y, Z)) return 0;
  const long V = (long)T * X * Y * Z;
  return 7 * fv_field_bytes(nb, V) + fv_stage_ws_bytes(nb, V);
}

int l2q_su3_flow_step_bwd(const void* x_in, double eps, const void* gx_out, void* gx_in, int nb, int T, int X,
                          int Y, int Z, void* ws, size_t ws_bytes, void* stream) {
  L2Q_REQUIRE(x_in && gx_out && gx_in && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(gx_in != x_in && gx_out != x_in, L2Q_EINVAL, "the cotangents must not alias x_in");
  L2Q_REQUIRE(ws != x_in && ws != gx_out && ws != gx_in, L2Q_EINVAL, "ws must alias no field");
  const long V = (long)T * X * Y * Z;
  const size_t fb = fv_field_bytes(nb, V);
  L2Q_REQUIRE(ws_bytes >= 7 * fb + fv_stage_ws_bytes(nb, V), L2Q_ESHAPE, "workspace too small");
  char* w = (char*)ws;
  void *x1 = w, *x2 = w + fb, *p1 = w + 2 * fb, *p2 = w + 3 * fb, *p3 = w + 4 * fb, *gp = w + 5 * fb, *ga = w + 6 * fb;
  void* gb = p3;                                // P3 is dead once stage 3 is reversed
  void* sws = w + 7 * fb;
  const size_t sws_bytes = ws_bytes - 7 * fb;
  hipStream_t st = (hipStream_t)stream;
  // the step again from x_in with the forward's own kernels (l2q_su3_flow_step), P1, P2, P3 kept apart; the links
  // after stage 3 are not needed, so its exponential is not taken
  const double c2 = -32.0 / 17.0, c3 = 27.0 / 17.0;
  const double s1 = -0.25 * eps, s2 = (17.0 / 36.0) * eps, s3 = -(17.0 / 36.0) * eps;
  int rc = l2q_su3_flow_stage(x_in, nullptr, 1.0, s1, p1, x1, nb, T, X, Y, Z, stream);
  if (rc != L2Q_OK) return rc;
  rc = l2q_su3_flow_stage(x1, p1, c2, s2, p2, x2, nb, T, X, Y, Z, stream);
  if (rc != L2Q_OK) return rc;
  rc = l2q_su3_force_kick_to(x2, 3.0, c3, p2, p3, nb, T, X, Y, Z, stream);
  if (rc != L2Q_OK) return rc;
  // stages 3 -> 1 with the cotangent of P starting at zero
  launch_zero(gp, fb, st);
  rc =l2q_su3_flow_stage_bwd(x2, p3, c3, s3, gx_out, gp, ga, nb, T, X, Y, Z, sws, sws_bytes, stream);
  if (rc != L2Q_OK) return rc;
  rc = l2q_su3_flow_stage_bwd(x1, p2, c2, s2, ga, gp, gb, nb, T, X, Y, Z, sws, sws_bytes, stream);
  if (rc != L2Q_OK) return rc;
  return l2q_su3_flow_stage_bwd(x_in, p1, 1.0, s1, gb, gp, gx_in, nb, T, X, Y, Z, sws, sws_bytes, stream);
}

}  // extern "C"
