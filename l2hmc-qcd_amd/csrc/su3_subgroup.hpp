// su3_subgroup.hpp -- what the checkerboard kernels of su3_heatbath.hip and su3_gaugefix.hip share: the periodic hop by
// division, and the quaternions that stand for the SU(2) subgroups of SU(3).
//   A quaternion a is the block [[a0 + i a3, a2 + i a1], [-a2 + i a1, a0 - i a3]] at rows / columns i, j of the
//   identity (embed(a)); for a 3 x 3 matrix W,
//     r = ( Re(W_ii + W_jj), Im(W_ij + W_ji), Re(W_ij - W_ji), Im(W_ii - W_jj) ) / 2
//   is the part of W that the subgroup sees: Re tr(embed(a) W) = const + 2 (a r)_0.
// (The extraction of r and the product embed(a) U are written out in each kernel: su3_link_update_kernel fuses them
// with its U A entries, and its fused multiply-adds are left exactly as they are.)
#pragma once
#include "su3_links.hpp"

namespace l2q {

// periodic neighbour of site s in a direction of stride st and extent ext; dir = +1 / -1
__device__ __forceinline__ int hb_hop(int s, int st, int ext, int dir) {
  const int c = (s / st) % ext;
  if (dir > 0) return c + 1 == ext ? s - (ext - 1) * st : s + st;
  return c == 0 ? s + (ext - 1) * st : s - st;
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

}  // namespace l2q
