// su3_clover.hpp -- the clover leaf of one plane, F_{mu nu}(x) = TAH(sum of the four leaves) / 4, shared by the
// clover sums (su3_flow.hip), their VJP (su3_clover_bwd.hip) and the clover term of the improved Wilson operator
// (su3_wilson_clover.hip), which takes the leaf sum Q without the TAH.  The leaves are listed in su3_flow.hip.
#pragma once
#include "su3_links.hpp"

namespace l2q {

// Each product of a leaf (one operand load + one 3x3 product) sits in a run-time conditional that is always
// taken (`go` compares a thread value with a kernel ARGUMENT, as in su3_expm_mul_kernel): hipcc cannot hoist the
// next operand's loads above it, so the live set stays at Q, two temporaries and one operand instead of all 16
// operands of a plane.
#define L2Q_CLOVER_STEP(...) if (go) { __VA_ARGS__ }

// anti-Hermitian 3x3 (traceless where TAH made it): i d[k] on the diagonal, (re, im)[0..2] = entries (0,1), (0,2), (1,2)
struct AH3 {
  double d[3], re[3], im[3];
};

// The eight sites a plane's leaves touch, as whatever handle the loader takes: x, x+mu, x+nu, x-mu, x-mu+nu,
// x-mu-nu, x-nu, x+mu-nu.
template <class S>
struct CloverSites {
  S o, pm, pn, mm, mm_pn, mm_mn, mn, pm_mn;
};

// q = Q_{mu nu}, the sum of the four leaves of plane (mu, nu); retr += Re tr L1.  ld(m, dir, site) loads U_dir(site).
// Each leaf is a chain of three products, so at most Q, two temporaries and one operand are live.
template <class Ld, class S>
__device__ __forceinline__ void clover_leaves(M3& q, double& retr, const Ld& ld, const CloverSites<S>& st, int mu,
                                              int nu, bool go) {
  M3 a, t, u;
  // L1
  L2Q_CLOVER_STEP(ld(a, mu, st.o); ld(u, nu, st.pm); m3_mul_nn(t, a, u);)
  L2Q_CLOVER_STEP(ld(a, mu, st.pn); m3_mul_na(u, t, a);)
  L2Q_CLOVER_STEP(ld(a, nu, st.o); m3_mul_na(q, u, a);)
  retr += q.re[0] + q.re[4] + q.re[8];
  // L2
  L2Q_CLOVER_STEP(ld(u, mu, st.mm_pn); m3_mul_na(t, a, u);)   // a = U_nu(x)
  L2Q_CLOVER_STEP(ld(a, nu, st.mm); m3_mul_na(u, t, a);)
  L2Q_CLOVER_STEP(ld(a, mu, st.mm); m3_mac_nn(q, u, a);)
  // L3
  L2Q_CLOVER_STEP(ld(u, nu, st.mm_mn); m3_mul_aa(t, a, u);)   // a = U_mu(x-mu)
  L2Q_CLOVER_STEP(ld(a, mu, st.mm_mn); m3_mul_nn(u, t, a);)
  L2Q_CLOVER_STEP(ld(a, nu, st.mn); m3_mac_nn(q, u, a);)
  // L4
  L2Q_CLOVER_STEP(ld(u, mu, st.mn); m3_mul_an(t, a, u);)      // a = U_nu(x-nu)
  L2Q_CLOVER_STEP(ld(a, nu, st.pm_mn); m3_mul_nn(u, t, a);)
  L2Q_CLOVER_STEP(ld(a, mu, st.o); m3_mac_na(q, u, a);)
}

// the anti-Hermitian part (Q - Q^H) / 8 with its trace: Fhat_{mu nu} of the Sheikholeslami-Wohlert term
__device__ __forceinline__ void clover_ah(AH3& f, const M3& q) {
  f.d[0] = 0.25 * q.im[0]; f.d[1] = 0.25 * q.im[4]; f.d[2] = 0.25 * q.im[8];
  f.re[0] = 0.125 * (q.re[1] - q.re[3]); f.im[0] = 0.125 * (q.im[1] + q.im[3]);
  f.re[1] = 0.125 * (q.re[2] - q.re[6]); f.im[1] = 0.125 * (q.im[2] + q.im[6]);
  f.re[2] = 0.125 * (q.re[5] - q.re[7]); f.im[2] = 0.125 * (q.im[5] + q.im[7]);
}

// F = TAH(sum of the four leaves of plane (mu, nu)) / 4; retr += Re tr L1
template <class Ld, class S>
__device__ __forceinline__ void clover_plane(AH3& f, double& retr, const Ld& ld, const CloverSites<S>& st, int mu,
                                             int nu, bool go) {
  M3 q;
  clover_leaves(q, retr, ld, st, mu, nu, go);
  // F = TAH(Q) / 4 kept as its 9 independent reals (anti-Hermitian, traceless)
  const double tr3 = (q.im[0] + q.im[4] + q.im[8]) * (1.0 / 3.0);
  f.d[0] = 0.25 * (q.im[0] - tr3); f.d[1] = 0.25 * (q.im[4] - tr3); f.d[2] = 0.25 * (q.im[8] - tr3);
  f.re[0] = 0.125 * (q.re[1] - q.re[3]); f.im[0] = 0.125 * (q.im[1] + q.im[3]);
  f.re[1] = 0.125 * (q.re[2] - q.re[6]); f.im[1] = 0.125 * (q.im[2] + q.im[6]);
  f.re[2] = 0.125 * (q.re[5] - q.re[7]); f.im[2] = 0.125 * (q.im[5] + q.im[7]);
}

// -tr(F G) = sum_ij F_ij conj(G_ij) for anti-Hermitian F, G (real)
__device__ __forceinline__ double clover_mtr(const AH3& f, const AH3& g) {
  double o = 0.0, r = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    r = fma(f.d[i], g.d[i], r);
    o = fma(f.re[i], g.re[i], o);
    o = fma(f.im[i], g.im[i], o);
  }
  return fma(2.0, o, r);
}

}  // namespace l2q
