// digits.hpp -- the activation digit image of the int8-sliced input layer (gemm_digits.hip) and the code its
// producers (su3_kernels.hip, gemm_digits.hip) write it with.
//
// Code: the one of the whole sliced input layer (gd_digits below is its scalar definition, gs_slice16_impl of
// gemm_sliced.hip the staged four-wide form): a value v with |v| < 2^e is X = rint(v 2^(54 - e)), recoded in
// balanced base 256, X = sum_s d_s 256^(6-s), d_s in [-128, 127] -- the same magic-number sums, hence the same bytes
// as the on-the-fly slicer of gemm_sliced_kernel.
//
// Layout: image[row][K / 64][7 digit planes][64 B].  The 64 bytes of a plane hold the 64 k of a slab in the k-order
// of the weight images (gemm_sliced.hip, gs_build_kernel): 16-byte chunk g, byte b  <->  k = 8 (b >> 1) + 2 g + (b & 1),
// so that chunk g of a row is lane (row, g)'s piece of the MFMA operand fragment as it stands.  Dword 4 g + jh of a
// plane therefore holds k = 16 jh + 2 g + {0, 1, 8, 9}: in a producer wavefront (lane <-> k) these four lanes exchange
// their digits by DPP and transpose them with v_perm, a ds_bpermute puts the dwords in address order, and the
// wavefront stores the planes 0..3 as 256 contiguous bytes and the planes 4..6 as 192.
#pragma once
#include "l2q_common.hpp"

namespace l2q {

constexpr int GS_NS = 7;                        // int8 digits per value
constexpr int GS_BITS = 54;                     // fixed-point bits below the operand's exponent
constexpr double GS_MAGIC24 = 113336795588871485128704.0;   // 1.5 * 2^76: a sum with it has ulp 2^24
constexpr double GS_MAGIC = 6755399441055744.0;             // 1.5 * 2^52: ulp 1
constexpr int GD_SLAB = GS_NS * 64;             // bytes of one row's 64-k slab

// the "operand out of range" flag of the device (gemm_sliced.hip): raised by whoever slices, read and cleared by the
// layer's reduce kernel
int* gs_flag();

#ifdef __HIPCC__
// digits of one value: lo = digits 6, 5, 4 in bytes 0, 1, 2 (byte 3: not a digit), hi = digits 3, 2, 1, 0 in bytes
// 0..3; returns true for |x| >= lim or a NaN.  sc = 2^(54 - e), lim = 2^e.
__device__ __forceinline__ bool gd_digits(double x, double sc, double lim, unsigned& lo, unsigned& hi) {
  const double t1 = fma(x, sc, GS_MAGIC24);                   // low mantissa dword: H = rint(x sc 2^-24)
  double r = GS_MAGIC24 - t1;                                 // -H 2^24 exactly
  r = fma(x, sc, r);                                          // x sc - H 2^24, exact, |r| <= 2^23
  const double t2 = r + GS_MAGIC;                             // low mantissa dword: L = rint(r)
  const int Lb = (int)(unsigned)__double_as_longlong(t2) + 0x00808080;   // bit 24: the carry into H
  lo = (unsigned)Lb ^ 0x00808080u;
  hi = ((unsigned)__double_as_longlong(t1) + (unsigned)(Lb >> 24) + 0x80808080u) ^ 0x80808080u;
  return !(fabs(x) < lim);
}

// byte b (per lane) of the values that the four lanes k0 + {0, 1, 8, 9} hold (k0 = lane & ~9: this lane's group), in
// that order.  x0..x3 = the values of lanes k, k ^ 1, k ^ 8, k ^ 9 by DPP (neighbour swap inside a quad, rotation by
// 8 inside a row of 16); lane k is member i = (k & 1) + 2 (k >> 3 & 1) of its group and x_j belongs to member i ^ j.
__device__ __forceinline__ unsigned gd_group_bytes(unsigned v, unsigned b, unsigned i) {
  const unsigned x0 = v;
  const unsigned x1 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);    // quad_perm:[1,0,3,2]
  const unsigned x2 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);   // row_ror:8
  const unsigned x3 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)x2, 0xB1, 0xf, 0xf, false);
  // v_perm_b32(hi, lo, sel): selector 0..3 = byte of lo, 4..7 = byte of hi.  [even member, odd member] of a pair:
  const unsigned sel = (i & 1) ? (4 + b) | (b << 8) : b | ((4 + b) << 8);
  const unsigned pa = __builtin_amdgcn_perm(x1, x0, sel);        // the pair this lane is in
  const unsigned pb = __builtin_amdgcn_perm(x3, x2, sel);        // the other pair
  return __builtin_amdgcn_perm(pb, pa, (i & 2) ? 0x01000504u : 0x05040100u);
}
// One value per lane (lane <-> k, natural order) -> the slab's seven planes; called by whole wavefronts.
// `slab`: this row's 64-k slab of the image.  Lane k ends up with dword 4 (k >> 1 & 3) + (k >> 4) of plane i (from
// hi) and of plane 4 + i (from lo, i < 3); one ds_bpermute each puts them in address order, so that the wavefront
// stores 256 + 192 contiguous bytes with lane-linear addresses.
__device__ __forceinline__ void gd_store_slab(char* slab, int lane, unsigned lo, unsigned hi) {
  const unsigned i = (lane & 1) + ((lane >> 2) & 2);
  const unsigned h = gd_group_bytes(hi, 3 - i, i);               // plane i = digit i = byte 3 - i of hi
  const unsigned l = gd_group_bytes(lo, (2 - i) & 3, i);         // plane 4 + i = byte 2 - i of lo (i < 3)
  // lane L stores dword L & 15 = 4 g + jh of plane L >> 4 = p: held by lane 16 jh + 2 g + (p & 1) + 8 (p >> 1)
  const int d = lane & 15, p = lane >> 4;
  const int src = (16 * (d & 3) + 2 * (d >> 2) + (p & 1) + 8 * (p >> 1)) * 4;
  const unsigned hs = (unsigned)__builtin_amdgcn_ds_bpermute(src, (int)h);
  const unsigned ls = (unsigned)__builtin_amdgcn_ds_bpermute(src, (int)l);
  unsigned* dst = reinterpret_cast<unsigned*>(slab) + lane;
  dst[0] = hs;
  if (lane < 48) dst[64] = ls;                                  // planes 4..6: + 256 bytes
}
#endif

}  // namespace l2q
