// su3_spinor_f32.hpp -- the single-precision helpers of su3_wilson_f32.hip: the half spinor of a rank-2 projector
// 1 -+ gamma_mu in float, its projection from a float2 field psi[system][12][sites], its product with a float link,
// its reconstruction into the sum of a site.  The same gamma basis, projector signs and seam sign as su3_spinor.hpp,
// whose text this restates in float on purpose: the fp64 helpers are not templated, so the device code of the fp64
// kernels stays what it is (profiles/wilson_hop_single_source.md).  WilsonBlock, wilson_block and spinor_dims_ok come
// from su3_spinor.hpp.
#pragma once
#include "su3_spinor.hpp"

namespace l2q {

struct HalfSpinorF {
  float re[6], im[6];          // [3 spin + colour], spin 0, 1
};

struct M3F {
  float re[9], im[9];
};

// the link at entry h of a plane block u[9][n] of the parity-ordered fp32 copy
__device__ __forceinline__ void load_link_f32(M3F& m, const float2* __restrict__ u, int n, int h) {
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    const float2 d = u[e * n + h];
    m.re[e] = d.x; m.im[e] = d.y;
  }
}

// h = bs (psi_u - sg B_mu psi_l) of the spinor at entry s of field f: the upper half of bs (1 - sg gamma_mu) psi.
// mu is wave-uniform (the loop counter), sg and bs are +-1.
__device__ __forceinline__ void wilson_project_f32(HalfSpinorF& h, const float2* __restrict__ f, int V, int s, int mu,
                                                   float sg, float bs) {
  float ur[6], ui[6], lr[6], li[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float2 a = f[k * V + s], b = f[(6 + k) * V + s];
    ur[k] = a.x; ui[k] = a.y; lr[k] = b.x; li[k] = b.y;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float r0, i0, r1, i1;
    switch (mu) {
      case 0:            // B = 1: h0 = psi0 - sg psi2, h1 = psi1 - sg psi3
        r0 = fmaf(-sg, lr[c], ur[c]); i0 = fmaf(-sg, li[c], ui[c]);
        r1 = fmaf(-sg, lr[3 + c], ur[3 + c]); i1 = fmaf(-sg, li[3 + c], ui[3 + c]);
        break;
      case 1:            // B = -i sigma_1: h0 = psi0 + i sg psi3, h1 = psi1 + i sg psi2
        r0 = fmaf(-sg, li[3 + c], ur[c]); i0 = fmaf(sg, lr[3 + c], ui[c]);
        r1 = fmaf(-sg, li[c], ur[3 + c]); i1 = fmaf(sg, lr[c], ui[3 + c]);
        break;
      case 2:            // B = -i sigma_2: h0 = psi0 + sg psi3, h1 = psi1 - sg psi2
        r0 = fmaf(sg, lr[3 + c], ur[c]); i0 = fmaf(sg, li[3 + c], ui[c]);
        r1 = fmaf(-sg, lr[c], ur[3 + c]); i1 = fmaf(-sg, li[c], ui[3 + c]);
        break;
      default:           // B = -i sigma_3: h0 = psi0 + i sg psi2, h1 = psi1 - i sg psi3
        r0 = fmaf(-sg, li[c], ur[c]); i0 = fmaf(sg, lr[c], ui[c]);
        r1 = fmaf(sg, li[3 + c], ur[3 + c]); i1 = fmaf(-sg, lr[3 + c], ui[3 + c]);
        break;
    }
    h.re[c] = bs * r0; h.im[c] = bs * i0;
    h.re[3 + c] = bs * r1; h.im[3 + c] = bs * i1;
  }
}

// chi = U h (ADJ: U^H h) for both colour vectors of the half spinor
template <bool ADJ>
__device__ __forceinline__ void wilson_colour_mul_f32(HalfSpinorF& chi, const M3F& u, const HalfSpinorF& h) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      float re = 0.0f, im = 0.0f;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float mr = ADJ ? u.re[3 * j + i] : u.re[3 * i + j];
        const float mi = ADJ ? -u.im[3 * j + i] : u.im[3 * i + j];
        const float hr = h.re[3 * a + j], hi = h.im[3 * a + j];
        re = fmaf(mr, hr, re); re = fmaf(-mi, hi, re);
        im = fmaf(mr, hi, im); im = fmaf(mi, hr, im);
      }
      chi.re[3 * a + i] = re; chi.im[3 * a + i] = im;
    }
}

// acc += (chi, -sg B_mu^H chi)
__device__ __forceinline__ void wilson_reconstruct_f32(float (&ar)[12], float (&ai)[12], const HalfSpinorF& chi, int mu,
                                                       float sg) {
#pragma unroll
  for (int k = 0; k < 6; ++k) { ar[k] += chi.re[k]; ai[k] += chi.im[k]; }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float r0 = chi.re[c], i0 = chi.im[c], r1 = chi.re[3 + c], i1 = chi.im[3 + c];
    switch (mu) {
      case 0:            // (-sg chi0, -sg chi1)
        ar[6 + c] = fmaf(-sg, r0, ar[6 + c]); ai[6 + c] = fmaf(-sg, i0, ai[6 + c]);
        ar[9 + c] = fmaf(-sg, r1, ar[9 + c]); ai[9 + c] = fmaf(-sg, i1, ai[9 + c]);
        break;
      case 1:            // (-i sg chi1, -i sg chi0)
        ar[6 + c] = fmaf(sg, i1, ar[6 + c]); ai[6 + c] = fmaf(-sg, r1, ai[6 + c]);
        ar[9 + c] = fmaf(sg, i0, ar[9 + c]); ai[9 + c] = fmaf(-sg, r0, ai[9 + c]);
        break;
      case 2:            // (-sg chi1, sg chi0)
        ar[6 + c] = fmaf(-sg, r1, ar[6 + c]); ai[6 + c] = fmaf(-sg, i1, ai[6 + c]);
        ar[9 + c] = fmaf(sg, r0, ar[9 + c]); ai[9 + c] = fmaf(sg, i0, ai[9 + c]);
        break;
      default:           // (-i sg chi0, i sg chi1)
        ar[6 + c] = fmaf(sg, i0, ar[6 + c]); ai[6 + c] = fmaf(-sg, r0, ai[6 + c]);
        ar[9 + c] = fmaf(-sg, i1, ar[9 + c]); ai[9 + c] = fmaf(sg, r1, ai[9 + c]);
        break;
    }
  }
}

}  // namespace l2q
