// su3_clover_insert.hpp -- what the two thread-per-link gathers over a clover-shaped per-site field share: the VJP of
// the clover sums (su3_clover_bwd.hip) and the clover force of dynamical improved quarks (su3_clover_force.hip).
//
// Given an anti-Hermitian 3 x 3 field G_{mu nu}(x) per site and plane (need not be traceless), stored as 6 planes x 9
// reals per site in a workspace gw[c][plane][9][V], planes in the order (01) (23) (02) (13) (03) (12), with
//   dS = sum_x sum_{mu<nu} Re tr(G_{mu nu}(x) dQ_{mu nu}(x)),   Q the sum of the four clover leaves (su3_clover.hpp),
// `clover_insert_link` collects the B of one link with dS = sum Re tr(B_mu(y) dU_mu(y)).
// Q(x) is four leaves, each a plaquette walked from x; seen from a plaquette, each of its four corners c inserts
// G(c) into the loop at c.  A link U = U_mu(y) lies on six plaquettes (three nu, up and down).  Written as the loop
// that STARTS with the link, U A2 A3 A4 with the corners c1, c2, c3 after U, A2, A3 and c0 = y,
//   up:   A2 = U_nu(y+mu)       A3 = U_mu(y+nu)^H  A4 = U_nu(y)^H     c = y, y+mu, y+mu+nu, y+nu
//   down: A2 = U_nu(y+mu-nu)^H  A3 = U_mu(y-nu)^H  A4 = U_nu(y-nu)    c = y, y+mu, y+mu-nu, y-nu
// its terms are Re tr(U B'), B' = G1 S + A2 G2 A3 A4 + A2 A3 G3 A4 + S G0, S = A2 A3 A4 (the staple), and
//   B += sigma B' + w2 S,    sigma = +1 where the loop runs counter-clockwise in its plane (mu < nu up,
//                            mu > nu down), -1 where it is a leaf's adjoint: Re tr(G L^H) = -Re tr(G L).
// With extents 1 and 2 several of these operands are the same link; every geometric occurrence is its own term
// here, as it is in the forward.
#pragma once
#include "su3_clover.hpp"

namespace l2q {

constexpr int kCloverGReals = 6 * 9;      // reals of G per site in the workspace

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

// Operand loads are tied to the product before them with site_after (su3_links.hpp).  Without it hipcc starts all of
// a loop's operands (3 links, 4 G) ahead of the first product and spills 68 registers; the always-taken conditional
// of clover_plane does not stop it here.  With it one operand is in flight next to the live matrices: 210 registers,
// no spill.
// acc += sg (G1 S + A2 (G2 A3 A4 + A3 (G3 A4 + A4 G0))) + w2 S: eight products, at most four matrices live next to
// acc.  LDA2 / LDA3 / LDA4 load the three links of the staple (adjoint where the loop walks them backwards) once
// their second argument exists, gp is the plane of G, c0..c3 the corners.
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

// acc = B of link (mu, s): the 6 x 4 inserted loops and w2 times the 6 staples.  xc: the chain's links, gc: its G.  The
// direction loop is not unrolled; mu must be wave-uniform (the callers take it from the block index).
__device__ __forceinline__ void clover_insert_link(M3& acc, const double2* __restrict__ xc,
                                                   const double* __restrict__ gc, double w2, const Dims& d, int s,
                                                   int mu) {
  // the extents by value: a Dims indexed by the loop-variant direction is copied to scratch (su3_links.hpp, site_hop)
  const int V = d.V, T = d.T, X = d.X, Y = d.Y, Z = d.Z;
  const auto stride = [=](int dir) { return dir == 0 ? X * Y * Z : dir == 1 ? Y * Z : dir == 2 ? Z : 1; };
  const auto extent = [=](int dir) { return dir == 0 ? T : dir == 1 ? X : dir == 2 ? Y : Z; };
  const double2* fm = xc + mu * 9 * V;
  const int s_pmu = site_hop(s, stride(mu), extent(mu), 1);
  m3_zero(acc);
#pragma unroll 1
  for (int j = 0; j < 3; ++j) {
    const int nu = j + (j >= mu ? 1 : 0);
    const double2* fn = xc + nu * 9 * V;
    // the plane of (mu, nu) in the workspace's order: (0, k) -> 2 (k - 1), the spatial plane dual to (0, k) -> 2 (k - 1) + 1
    const int lo_d = mu < nu ? mu : nu, hi_d = mu < nu ? nu : mu;
    const int pl = lo_d == 0 ? 2 * (hi_d - 1) : 2 * (6 - lo_d - hi_d) - 1;
    const double* gp = gc + pl * 9L * V;
    const int sn = stride(nu), en = extent(nu);
    const int s_pnu = site_hop(s, sn, en, 1), s_mnu = site_hop(s, sn, en, -1);
    const int s_pmu_pnu = site_hop(s_pmu, sn, en, 1), s_pmu_mnu = site_hop(s_pmu, sn, en, -1);
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
#undef L2Q_UP_A2
#undef L2Q_UP_A3
#undef L2Q_UP_A4
#undef L2Q_DN_A2
#undef L2Q_DN_A3
#undef L2Q_DN_A4
  }
}

}  // namespace l2q
