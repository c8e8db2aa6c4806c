// su3_smear.hip -- APE and HYP link smearing: a sum of staples around a link, blended with the link and projected back
// to SU(3).  (APE: Albanese et al. 1987; HYP: Hasenfratz & Knechtli 2001.)
//
// Staples: for a side field A (links of direction nu) and a forward field B (links of direction mu), in the plaquette
// convention of su3_plaq_kernel and the force,
//     S_nu[A, B](x) = A(x) B(x+nu) A(x+mu)^H  +  A(x-nu)^H B(x-nu) A(x-nu+mu).
// Proj is m3_project_su: the unitary (polar) factor with the phase of its determinant divided out.
//
//   APE, directions D (a 4-bit set), n = |D| - 1:
//     mu in D:     U'_mu    = Proj[(1 - alpha) U_mu + (alpha / 2n) sum_{nu in D, nu != mu} S_nu[U_nu, U_mu]]
//     mu not in D: U'_mu    = U_mu, the same bits
//   HYP, eta = 6 - mu - nu - rho the fourth direction:
//     level 1:     B1[mu][eta] = Proj[(1 - alpha3) U_mu + (alpha3 / 2) S_eta[U_eta, U_mu]]
//     level 2:     B2[mu][nu]  = Proj[(1 - alpha2) U_mu
//                                     + (alpha2 / 4) sum_{rho != mu, nu} S_rho[B1[rho][eta], B1[mu][eta]]]
//     level 3:     V_mu        = Proj[(1 - alpha1) U_mu + (alpha1 / 6) sum_{nu != mu} S_nu[B2[nu][mu], B2[mu][nu]]]
//
// A decorated field holds the 12 fields F[mu][o], o != mu, of one level as dec[chain][mu][k][e][site], k = o - (o > mu)
// (the pair order of su3_loops.hip): three link fields in size.
//
// One kernel, su3_smear_kernel<LEVEL>: one thread per (chain, output field, site), the output field from the block
// index, so every direction below is wave-uniform and nothing is indexed dynamically in registers.  The levels differ
// only in which staple directions are summed (a 4-bit set) and where a direction's side and forward fields are
// (smear_fields).
// Every operand is a coalesced 16 B / lane plane load, the shifted ones re-read through L1 / L2 as in su3_loops.hip.
// The staple loop is not unrolled and the neighbours come by division (site_hop): live are the sum, one product and two
// operands; the link itself is loaded after the loop.  Left alone, the compiler hoists the plane addresses of the
// loop-invariant operands out of the loop (18 VGPRs per link) and issues all six loads of a direction at once, and
// spills at two waves per SIMD; so the site index of an iteration exists only once the sum of the one before does, and
// the second staple's pair only once the first staple is summed (site_after): three link loads in flight, no scratch
// (profiles/su3_smear.md).  All four entry points are out of place, so any extents do.
#include "su3_launch.hpp"

namespace l2q {

enum SmearLevel { kApe = 0, kHyp1 = 1, kHyp2 = 2, kHyp3 = 3 };

// the field F[a][o] of a chain's decorated field
__device__ __forceinline__ const double2* dec_field(const double2* dec, int V, int a, int o) {
  return dec + (a * 3 + (o - (o > a ? 1 : 0))) * 9L * V;
}

// the side field (direction rho) and the forward field (direction mu) of the staples of direction rho around the link
// of output field (mu, o); xc / dc: the chain's thin links and the previous level's decorated field
template <int LEVEL>
__device__ __forceinline__ void smear_fields(const double2*& side, const double2*& fwd, const double2* xc,
                                             const double2* dc, int V, int mu, int o, int rho) {
  if constexpr (LEVEL == kApe || LEVEL == kHyp1) {
    side = xc + rho * 9L * V;
    fwd = xc + mu * 9L * V;
  } else if constexpr (LEVEL == kHyp2) {
    const int eta = 6 - mu - o - rho;
    side = dec_field(dc, V, rho, eta);
    fwd = dec_field(dc, V, mu, eta);
  } else {
    side = dec_field(dc, V, rho, mu);
    fwd = dec_field(dc, V, mu, rho);
  }
}

// xn: the thin links; dec: the previous level's decorated field (levels 2 and 3; unused before); dirmask: the APE
// directions (unused by the HYP levels); out: a link field (APE, level 3) or a decorated field (levels 1, 2);
// cu = 1 - alpha, cs = alpha / (number of staples).  Two waves per SIMD: the four live matrices are 144 VGPRs, the
// plane addresses of the loads in flight most of the rest.
template <int LEVEL>
__global__ __launch_bounds__(kBlock, 2) void su3_smear_kernel(const double2* __restrict__ xn,
                                                              const double2* __restrict__ dec, int dirmask, double cu,
                                                              double cs, double2* __restrict__ out, int T, int X, int Y,
                                                              int Z, long nblk, int swz) {
  constexpr int NF = (LEVEL == kHyp1 || LEVEL == kHyp2) ? 12 : 4;      // output fields per chain
  const Dims d{T, X, Y, Z, T * X * Y * Z};
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  // Block order: chain, field, site block -- but level 2 takes chain, site block, field.  Each B1 field is read by four
  // of its output fields; with a chain's B1 at 7 MB per 8^4 against 4 MB of L2 per XCD, the field-major order fetches
  // it four times (7.3 GB instead of 2.4 GB per launch at 256 chains), the site-major one 1.2 times, 8 % faster.  The
  // other three read each input field's lines close together already and are 1 - 13 % slower site-major.
  constexpr bool kSiteMajor = LEVEL == kHyp2;
  const long c = w / (NF * nblk), rest = w % (NF * nblk);
  const long blk = kSiteMajor ? rest / NF : rest % nblk;
  const int f = (int)(kSiteMajor ? rest % NF : rest / nblk);
  const long fi = c * NF + f;                                           // the output field
  const int V = d.V;
  const int s = (int)blk * kBlock + threadIdx.x;
  if (s >= V) return;
  const int mu = NF == 12 ? f / 3 : f;
  const int k = NF == 12 ? f % 3 : 0;
  const int o = k + (k >= mu ? 1 : 0);                                  // the field's other direction (levels 1, 2)
  const double2* xc = xn + c * 36L * V;
  const double2* dc = (LEVEL == kHyp2 || LEVEL == kHyp3) ? dec + c * 108L * V : nullptr;
  const double2* um = xc + mu * 9L * V;
  double2* om = out + fi * 9L * V;
  // the staple directions
  int dirs;
  if constexpr (LEVEL == kApe) dirs = dirmask & ~(1 << mu);
  else if constexpr (LEVEL == kHyp1) dirs = 1 << o;
  else if constexpr (LEVEL == kHyp2) dirs = 15 & ~(1 << mu) & ~(1 << o);
  else dirs = 15 & ~(1 << mu);
  if (LEVEL == kApe && ((dirmask >> mu) & 1) == 0) {                    // wave-uniform
    M3 u;
    load_link(u, um, V, s);
    store_link(om, V, s, u);
    return;
  }
  const int s_mu = site_hop(s, stride_of(d, mu), extent_of(d, mu), +1);
  M3 acc;
  m3_zero(acc);
#pragma unroll 1
  for (int rho = 0; rho < 4; ++rho) {
    if (((dirs >> rho) & 1) == 0) continue;
    const double2 *side, *fwd;
    smear_fields<LEVEL>(side, fwd, xc, dc, V, mu, o, rho);
    const int st = stride_of(d, rho), ext = extent_of(d, rho);
    M3 a, b, p;
    const int sx = site_after(s, acc.im[8]), sx_mu = site_after(s_mu, acc.im[8]);
    // A(x) B(x+rho) A(x+mu)^H
    load_link(a, side, V, sx);
    load_link(b, fwd, V, site_hop(sx, st, ext, +1));
    m3_mul_nn(p, a, b);
    load_link(a, side, V, sx_mu);
    m3_mac_na(acc, p, a);
    // A(x-rho)^H B(x-rho) A(x-rho+mu)
    const int s_dn = site_after(site_hop(sx, st, ext, -1), acc.im[8]);
    load_link(a, side, V, s_dn);
    load_link(b, fwd, V, s_dn);
    m3_mul_an(p, a, b);
    load_link(a, side, V, site_hop(sx_mu, st, ext, -1));
    m3_mac_nn(acc, p, a);
  }
  M3 u, r;
  load_link(u, um, V, s);
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    u.re[e] = fma(cu, u.re[e], cs * acc.re[e]);
    u.im[e] = fma(cu, u.im[e], cs * acc.im[e]);
  }
  m3_project_su(r, u);
  store_link(om, V, s, r);
}

template <int LEVEL>
static int launch_smear(const char* name, const void* xn, const void* dec, int dirmask, double alpha, int nstaples,
                        void* out, int nb, int T, int X, int Y, int Z, void* stream) {
  constexpr int NF = (LEVEL == kHyp1 || LEVEL == kHyp2) ? 12 : 4;
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V, kBlock);
  hipLaunchKernelGGL(su3_smear_kernel<LEVEL>, dim3((unsigned)(nb * (long)NF * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, (const double2*)xn, (const double2*)dec, dirmask, 1.0 - alpha,
                     alpha / nstaples, (double2*)out, T, X, Y, Z, nblk, tuning().xcd_swizzle);
  return check_launch(name);
}

static bool smear_alpha_ok(double a) { return a >= 0.0 && a <= 1.0; }    // false for a NaN

}  // namespace l2q

using namespace l2q;

extern "C" {

int l2q_su3_ape_smear(const void* xn, double alpha, int dirmask, void* out, int nb, int T, int X, int Y, int Z,
                      void* stream) {
  L2Q_REQUIRE(xn && out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(out != xn, L2Q_EINVAL, "out must not alias xn");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(smear_alpha_ok(alpha), L2Q_EINVAL, "alpha must be finite and in [0, 1]");
  L2Q_REQUIRE(dirmask_ok(dirmask), L2Q_EINVAL, "dirmask must be 1..15 with at least two directions");
  return launch_smear<kApe>("l2q_su3_ape_smear", xn, nullptr, dirmask, alpha, 2 * (dirmask_count(dirmask) - 1), out, nb,
                            T, X, Y, Z, stream);
}

int l2q_su3_hyp_level1(const void* xn, double alpha3, void* b1, int nb, int T, int X, int Y, int Z, void* stream) {
  L2Q_REQUIRE(xn && b1, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(b1 != xn, L2Q_EINVAL, "b1 must not alias xn");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(smear_alpha_ok(alpha3), L2Q_EINVAL, "alpha3 must be finite and in [0, 1]");
  return launch_smear<kHyp1>("l2q_su3_hyp_level1", xn, nullptr, 0, alpha3, 2, b1, nb, T, X, Y, Z, stream);
}

int l2q_su3_hyp_level2(const void* xn, const void* b1, double alpha2, void* b2, int nb, int T, int X, int Y, int Z,
                       void* stream) {
  L2Q_REQUIRE(xn && b1 && b2, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(b2 != xn && b2 != b1, L2Q_EINVAL, "b2 must not alias xn or b1");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(smear_alpha_ok(alpha2), L2Q_EINVAL, "alpha2 must be finite and in [0, 1]");
  return launch_smear<kHyp2>("l2q_su3_hyp_level2", xn, b1, 0, alpha2, 4, b2, nb, T, X, Y, Z, stream);
}

int l2q_su3_hyp_level3(const void* xn, const void* b2, double alpha1, void* out, int nb, int T, int X, int Y, int Z,
                       void* stream) {
  L2Q_REQUIRE(xn && b2 && out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(out != xn && out != b2, L2Q_EINVAL, "out must not alias xn or b2");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(smear_alpha_ok(alpha1), L2Q_EINVAL, "alpha1 must be finite and in [0, 1]");
  return launch_smear<kHyp3>("l2q_su3_hyp_level3", xn, b2, 0, alpha1, 6, out, nb, T, X, Y, Z, stream);
}

}  // extern "C"
