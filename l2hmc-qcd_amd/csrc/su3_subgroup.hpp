// su3_subgroup.hpp -- what the checkerboard kernels of su3_heatbath.hip and su3_gaugefix.hip share: the site of a
// half-site index, and the quaternions that stand for the SU(2) subgroups of SU(3).
//   A quaternion a is the block [[a0 + i a3, a2 + i a1], [-a2 + i a1, a0 - i a3]] at rows / columns i, j of the
//   identity (embed(a)); for a 3 x 3 matrix W,
//     r = ( Re(W_ii + W_jj), Im(W_ij + W_ji), Re(W_ij - W_ji), Im(W_ii - W_jj) ) / 2
//   is the part of W that the subgroup sees: Re tr(embed(a) W) = const + 2 (a r)_0.
// su2_part_unit extracts r and su2_embed_mul forms embed(a) U; su3_gaugefix_kernel uses both.  su3_link_update_kernel
// deliberately keeps its own text of the same lines (subgroup_update): it fuses the extraction with its U A entries,
// and going through either function, alone or together, changes the instruction stream of both of its variants
// (profiles/site_kernels_single_source/).
#pragma once
#include "su3_links.hpp"

namespace l2q {

// The site of parity `parity` in the pair (2h, 2h + 1), which differ in z only (Z is even): one thread per half-site.
__device__ __forceinline__ int checkerboard_site(int h, int parity, int X, int Y, int Z) {
  int s = 2 * h;
  int q = s / Z;
  const int y = q % Y; q /= Y;
  const int x = q % X; q /= X;
  return s + ((parity - q - x - y) & 1);
}

struct Quat {
  double q0, q1, q2, q3;
};

// the product of the 2 x 2 matrices that a and b stand for
__device__ __forceinline__ Quat q_mul(const Quat& a, const Quat& b) {
  Quat c;
  c.q0 = a.q0 * b.q0 - a.q1 * b.q1 - a.q2 * b.q2 - a.q3 * b.q3;
  c.q1 = a.q0 * b.q1 + a.q1 * b.q0 - (a.q2 * b.q3 - a.q3 * b.q2);
  c.q2 = a.q0 * b.q2 + a.q2 * b.q0 - (a.q3 * b.q1 - a.q1 * b.q3);
  c.q3 = a.q0 * b.q3 + a.q3 * b.q0 - (a.q1 * b.q2 - a.q2 * b.q1);
  return c;
}

__device__ __forceinline__ Quat q_conj(const Quat& a) { return Quat{a.q0, -a.q1, -a.q2, -a.q3}; }

// k = |r| and rh = r / k of the subgroup part r of a matrix, from its four entries (ii, ij, ji, jj); rh = (1, 0, 0, 0)
// where k is zero or not finite
__device__ __forceinline__ double su2_part_unit(Quat& rh, double iir, double iii, double ijr, double iji, double jir,
                                                double jii, double jjr, double jji) {
  const double r0 = 0.5 * (iir + jjr), r1 = 0.5 * (iji + jii), r2 = 0.5 * (ijr - jir), r3 = 0.5 * (iii - jji);
  const double k = sqrt(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
  rh = Quat{1.0, 0.0, 0.0, 0.0};
  if (k > 0.0 && k <= 1.7976931348623157e308) { rh.q0 = r0 / k; rh.q1 = r1 / k; rh.q2 = r2 / k; rh.q3 = r3 / k; }
  return k;
}

// u <- embed(g) u: rows I and J
template <int I, int J>
__device__ __forceinline__ void su2_embed_mul(M3& u, const Quat& g) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double xr = u.re[3 * I + c], xi = u.im[3 * I + c], yr = u.re[3 * J + c], yi = u.im[3 * J + c];
    u.re[3 * I + c] = g.q0 * xr - g.q3 * xi + g.q2 * yr - g.q1 * yi;
    u.im[3 * I + c] = g.q0 * xi + g.q3 * xr + g.q2 * yi + g.q1 * yr;
    u.re[3 * J + c] = -g.q2 * xr - g.q1 * xi + g.q0 * yr + g.q3 * yi;
    u.im[3 * J + c] = -g.q2 * xi + g.q1 * xr + g.q0 * yi - g.q3 * yr;
  }
}

}  // namespace l2q
