// su3_spinor.hpp -- what the kernels over spinor fields share (su3_wilson.hip: the Wilson-Dirac operator;
// su3_wilson_eo.hip: its half-lattice hop; su3_wilson_force.hip: the pseudofermion force): the half spinor of a rank-2
// projector 1 -+ gamma_mu, its projection from a field in the layout psi[system][12][V], its product with a link, its
// reconstruction into the sum of a site, the workgroup order of the operator kernels, and the size check.
//
// Gamma matrices: Hermitian, chiral, gamma_mu = [[0, B_mu], [B_mu^H, 0]] in 2 x 2 blocks with
//   B_0 = 1 (direction 0 is T),  B_k = -i sigma_k (k = 1, 2, 3 = x, y, z),  gamma5 = g0 g1 g2 g3 = diag(-1, -1, 1, 1).
// 1 - s gamma_mu has rank 2: with h = psi_u - s B psi_l (the upper two spin components), (1 - s gamma_mu) psi =
// (h, -s B^H h).
#pragma once
#include "su3_launch.hpp"

namespace l2q {

struct HalfSpinor {
  double re[6], im[6];          // [3 spin + colour], spin 0, 1
};

// h = bs (psi_u - sg B_mu psi_l) of the spinor at site s of field f: the upper half of bs (1 - sg gamma_mu) psi.
// mu is wave-uniform (the loop counter), sg and bs are +-1.
__device__ __forceinline__ void wilson_project(HalfSpinor& h, const double2* __restrict__ f, int V, int s, int mu,
                                               double sg, double bs) {
  double ur[6], ui[6], lr[6], li[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double2 a = f[k * V + s], b = f[(6 + k) * V + s];
    ur[k] = a.x; ui[k] = a.y; lr[k] = b.x; li[k] = b.y;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double r0, i0, r1, i1;
    switch (mu) {
      case 0:            // B = 1: h0 = psi0 - sg psi2, h1 = psi1 - sg psi3
        r0 = fma(-sg, lr[c], ur[c]); i0 = fma(-sg, li[c], ui[c]);
        r1 = fma(-sg, lr[3 + c], ur[3 + c]); i1 = fma(-sg, li[3 + c], ui[3 + c]);
        break;
      case 1:            // B = -i sigma_1: h0 = psi0 + i sg psi3, h1 = psi1 + i sg psi2
        r0 = fma(-sg, li[3 + c], ur[c]); i0 = fma(sg, lr[3 + c], ui[c]);
        r1 = fma(-sg, li[c], ur[3 + c]); i1 = fma(sg, lr[c], ui[3 + c]);
        break;
      case 2:            // B = -i sigma_2: h0 = psi0 + sg psi3, h1 = psi1 - sg psi2
        r0 = fma(sg, lr[3 + c], ur[c]); i0 = fma(sg, li[3 + c], ui[c]);
        r1 = fma(-sg, lr[c], ur[3 + c]); i1 = fma(-sg, li[c], ui[3 + c]);
        break;
      default:           // B = -i sigma_3: h0 = psi0 + i sg psi2, h1 = psi1 - i sg psi3
        r0 = fma(-sg, li[c], ur[c]); i0 = fma(sg, lr[c], ui[c]);
        r1 = fma(sg, li[3 + c], ur[3 + c]); i1 = fma(-sg, lr[3 + c], ui[3 + c]);
        break;
    }
    h.re[c] = bs * r0; h.im[c] = bs * i0;
    h.re[3 + c] = bs * r1; h.im[3 + c] = bs * i1;
  }
}

// chi = U h (ADJ: U^H h) for both colour vectors of the half spinor
template <bool ADJ>
__device__ __forceinline__ void wilson_colour_mul(HalfSpinor& chi, const M3& u, const HalfSpinor& h) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double re = 0.0, im = 0.0;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double mr = ADJ ? u.re[3 * j + i] : u.re[3 * i + j];
        const double mi = ADJ ? -u.im[3 * j + i] : u.im[3 * i + j];
        const double hr = h.re[3 * a + j], hi = h.im[3 * a + j];
        re = fma(mr, hr, re); re = fma(-mi, hi, re);
        im = fma(mr, hi, im); im = fma(mi, hr, im);
      }
      chi.re[3 * a + i] = re; chi.im[3 * a + i] = im;
    }
}

// acc += (chi, -sg B_mu^H chi)
__device__ __forceinline__ void wilson_reconstruct(double (&ar)[12], double (&ai)[12], const HalfSpinor& chi, int mu,
                                                   double sg) {
#pragma unroll
  for (int k = 0; k < 6; ++k) { ar[k] += chi.re[k]; ai[k] += chi.im[k]; }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double r0 = chi.re[c], i0 = chi.im[c], r1 = chi.re[3 + c], i1 = chi.im[3 + c];
    switch (mu) {
      case 0:            // (-sg chi0, -sg chi1)
        ar[6 + c] = fma(-sg, r0, ar[6 + c]); ai[6 + c] = fma(-sg, i0, ai[6 + c]);
        ar[9 + c] = fma(-sg, r1, ar[9 + c]); ai[9 + c] = fma(-sg, i1, ai[9 + c]);
        break;
      case 1:            // (-i sg chi1, -i sg chi0)
        ar[6 + c] = fma(sg, i1, ar[6 + c]); ai[6 + c] = fma(-sg, r1, ai[6 + c]);
        ar[9 + c] = fma(sg, i0, ar[9 + c]); ai[9 + c] = fma(-sg, r0, ai[9 + c]);
        break;
      case 2:            // (-sg chi1, sg chi0)
        ar[6 + c] = fma(-sg, r1, ar[6 + c]); ai[6 + c] = fma(-sg, i1, ai[6 + c]);
        ar[9 + c] = fma(sg, r0, ar[9 + c]); ai[9 + c] = fma(sg, i0, ai[9 + c]);
        break;
      default:           // (-i sg chi0, i sg chi1)
        ar[6 + c] = fma(sg, i0, ar[6 + c]); ai[6 + c] = fma(-sg, r0, ai[6 + c]);
        ar[9 + c] = fma(-sg, i1, ar[9 + c]); ai[9 + c] = fma(sg, r1, ai[9 + c]);
        break;
    }
  }
}

// fout = (fin ? fin : 0) + cf TAH(w) at site s of one link's nine planes, the epilogue of the fermion forces
// (su3_wilson_force.hip, su3_clover_force.hip).  TAH(w) is stored exactly anti-Hermitian: the two planes of a transposed
// pair get one number and its negative, the diagonal no real part.  fin may be fout: an entry is read before it is
// written, by its own thread.
__device__ __forceinline__ void store_tah_axpy(const double2* fin, double2* fout, int V, int s, double cf,
                                               const M3& w) {
  const double tr3 = (w.im[0] + w.im[4] + w.im[8]) / 3.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int e = 4 * i;
    const double2 in = fin ? fin[e * V + s] : make_double2(0.0, 0.0);
    fout[e * V + s] = make_double2(in.x, fma(cf, w.im[e] - tr3, in.y));
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i + 1; j < 3; ++j) {
      const int e = 3 * i + j, et = 3 * j + i;
      const double ar = 0.5 * (w.re[e] - w.re[et]), ai = 0.5 * (w.im[e] + w.im[et]);
      const double2 in = fin ? fin[e * V + s] : make_double2(0.0, 0.0);
      const double2 it = fin ? fin[et * V + s] : make_double2(0.0, 0.0);
      fout[e * V + s] = make_double2(fma(cf, ar, in.x), fma(cf, ai, in.y));
      fout[et * V + s] = make_double2(fma(cf, -ar, it.x), fma(cf, ai, it.y));
    }
}

// the system and the site block of workgroup w: chain, site block, right-hand side (the fastest)
struct WilsonBlock {
  long c, sys;
  int blk;
};
__device__ __forceinline__ WilsonBlock wilson_block(long w, int nrhs, long nblk) {
  const long c = w / (nblk * nrhs), rest = w % (nblk * nrhs);
  return WilsonBlock{c, c * nrhs + rest % nrhs, (int)(rest / nrhs)};
}

// nsys systems of 12 V complex entries: positive sizes, and every entry's index fits an int (in double: no overflow)
inline bool spinor_dims_ok(long nsys, long V) {
  return nsys > 0 && V > 0 && (double)nsys * 12.0 * (double)V < 2147483648.0;
}

}  // namespace l2q
