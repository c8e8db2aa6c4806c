// su3_clover_block.hpp -- what the kernels of su3_wilson_clover.hip share: the block field of the clover term and the
// product of one of its Hermitian 6 x 6 blocks with the six components of one chirality.
//
// In the chiral gamma basis of su3_spinor.hpp the clover term A(x) = 1 + kappa c_sw i sum_{mu<nu} sigma_{mu nu} (x)
// Fhat_{mu nu}(x) is diag(A+, A-): two Hermitian 6 x 6 blocks, A+ on the spin components 0, 1 (gamma5 = -1), A- on 2, 3,
// row index 3 spin + colour within a chirality.  The block field is
//   cl[chain][parity][chirality][36][V/2] doubles,
// parity-ordered like the fp32 link copy (entry h of parity p belongs to checkerboard_site(h, p)); the 36 reals of a
// block are its 6 diagonal entries, then (re, im) of the 15 entries above the diagonal, row-major.  A lane's 36 loads
// are contiguous across lanes.
#pragma once
#include "su3_spinor.hpp"

namespace l2q {

constexpr int kCloverReals = 36;     // per block
// the position of entry (r, c), r < c, among the 15 entries above the diagonal
constexpr int clover_upper(int r, int c) { return r * 6 - r * (r + 1) / 2 + (c - r - 1); }

// block (chain, parity, chirality) of the field cl, at the lane's half-site
__device__ __forceinline__ const double* clover_block(const double* cl, long chain, int parity, int chi, int Vh, int h) {
  return cl + ((chain * 2 + parity) * 2 + chi) * (long)kCloverReals * Vh + h;
}

// o = C v: the Hermitian block at blk (stride Vh between its reals) times the six entries v of its chirality.  Every
// entry above the diagonal is loaded once and used for both triangles, so no more than the loads in flight are live.
__device__ __forceinline__ void clover_block_mul(double* __restrict__ orr, double* __restrict__ oi,
                                                 const double* __restrict__ blk, int Vh, const double* vr,
                                                 const double* vi) {
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const double dg = blk[r * Vh];
    orr[r] = dg * vr[r]; oi[r] = dg * vi[r];
  }
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r + 1; c < 6; ++c) {
      const int e = 6 + 2 * clover_upper(r, c);
      const double re = blk[e * Vh], im = blk[(e + 1) * Vh];
      orr[r] = fma(re, vr[c], orr[r]); orr[r] = fma(-im, vi[c], orr[r]);     // C_rc v_c
      oi[r] = fma(re, vi[c], oi[r]); oi[r] = fma(im, vr[c], oi[r]);
      orr[c] = fma(re, vr[r], orr[c]); orr[c] = fma(im, vi[r], orr[c]);      // conj(C_rc) v_r
      oi[c] = fma(re, vi[r], oi[c]); oi[c] = fma(-im, vr[r], oi[c]);
    }
}

// Smallest `v` over the 256 threads of a block, returned on thread 0: the fixed tree of block_sum.
__device__ __forceinline__ double block_min(double v, double* lds /* >= 4 doubles */) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off, 64));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  double r = v;
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
    for (int w = 1; w < nw; ++w) r = fmin(r, lds[w]);
  }
  return r;
}

}  // namespace l2q
