// su3_kernels.hip -- 4D SU(3) lattice kernels for gfx950 (MI355X).
//
// Native field layout xn[chain][mu][e][site] complex128: lane <-> site, so every load of a
// matrix entry is one coalesced 16 B/lane wavefront load; the 3x3 algebra lives in
// registers (su3_math.hpp).  Stencil neighbours are re-read through L1/L2; the 1-D grids
// are XCD-swizzled so the blocks that share a chain's links share an XCD's L2.
#include "su3_launch.hpp"
#include "digits.hpp"
#include "half_common.hpp"

namespace l2q {

// ------------------------------------------------------------------ plaquette reduce
// sum over the 6 planes u > v of tr[ U_u(s) U_v(s+u) (U_v(s) U_u(s+v))^H ]
// (lattice/su3/pytorch/lattice.py:164-174).  The plane loop is deliberately NOT unrolled:
// it bounds the live ranges (<= 3 matrices) instead of letting the scheduler hoist 144 loads.
template <int OCC>
__global__ __launch_bounds__(kBlock, OCC) void su3_plaq_kernel(const double2* __restrict__ xn,
                                                               Dims d, long nblk, int swz,
                                                               double* __restrict__ partial) {
  __shared__ double lds[8];
  const long total = (long)gridDim.x;
  const long w = xcd_swizzle(blockIdx.x, total, swz);
  const long c = w / nblk, blk = w % nblk;
  const int s = (int)blk * kBlock + threadIdx.x;
  double sr = 0.0, si = 0.0;
  if (s < d.V) {
    const double2* xc = xn + c * 36L * d.V;
    const Site p = site_coords(s, d);
    const int V = d.V;
#pragma unroll 1
    for (int u = 1; u < 4; ++u) {
      const int s_pu = fwd(s, coord_of(p, u), d, u);
#pragma unroll 1
      for (int v = 0; v < u; ++v) {
        const int s_pv = fwd(s, coord_of(p, v), d, v);
        M3 a, b, yuv;
        load_link(a, xc + u * 9 * V, V, s);
        load_link(b, xc + v * 9 * V, V, s_pu);
        m3_mul_nn(yuv, a, b);
        load_link(a, xc + v * 9 * V, V, s);
        load_link(b, xc + u * 9 * V, V, s_pv);
        m3_trace_y_abh(sr, si, yuv, a, b);
      }
    }
  }
  const double br = block_sum(sr, lds);
  const double bi = block_sum(si, lds + 4);
  if (threadIdx.x == 0) {
    partial[(c * nblk + blk) * 2 + 0] = br;
    partial[(c * nblk + blk) * 2 + 1] = bi;
  }
}

// Per-plane variant for LatticeLoss._plaq_loss (loss/pytorch/loss.py:57-70 sums each of the 6
// planes separately): partial[c][blk][plane][re|im]; same site loop, one block reduction per
// plane.
__global__ __launch_bounds__(kBlock, 2) void su3_plaq_planes_kernel(const double2* __restrict__ xn,
                                                                    Dims d, long nblk,
                                                                    double* __restrict__ partial) {
  __shared__ double lds[8];
  const long c = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int s = (int)blk * kBlock + threadIdx.x;
  const bool live = s < d.V;
  const double2* xc = xn + c * 36L * d.V;
  const Site p = site_coords(live ? s : 0, d);
  const int V = d.V, ss = live ? s : 0;
  int plane = 0;
#pragma unroll 1
  for (int u = 1; u < 4; ++u) {
    const int s_pu = fwd(ss, coord_of(p, u), d, u);
#pragma unroll 1
    for (int v = 0; v < u; ++v, ++plane) {
      const int s_pv = fwd(ss, coord_of(p, v), d, v);
      double sr = 0.0, si = 0.0;
      M3 a, b, yuv;
      load_link(a, xc + u * 9 * V, V, ss);
      load_link(b, xc + v * 9 * V, V, s_pu);
      m3_mul_nn(yuv, a, b);
      load_link(a, xc + v * 9 * V, V, ss);
      load_link(b, xc + u * 9 * V, V, s_pv);
      m3_trace_y_abh(sr, si, yuv, a, b);
      if (!live) { sr = 0.0; si = 0.0; }
      const double br = block_sum(sr, lds);
      const double bi = block_sum(si, lds + 4);
      if (threadIdx.x == 0) {
        partial[((c * nblk + blk) * 6 + plane) * 2 + 0] = br;
        partial[((c * nblk + blk) * 6 + plane) * 2 + 1] = bi;
      }
    }
  }
}

// The trace FIELD itself, out[plane][chain][site] = tr P_plane(site) (complex): the tensor the reference's
// `LatticeSU3.wilson_loops` returns, [6, nb, T, X, Y, Z] (lattice/su3/pytorch/lattice.py:157-174, 242-244).
// The sampler never needs it (action / plaquette / charges are the per-chain sums above); callers that
// reduce the field themselves (loss/pytorch/loss.py:57-110) do.  864 B read + 96 B written per site.
__global__ __launch_bounds__(kBlock, 2) void su3_wloops_kernel(const double2* __restrict__ xn, Dims d,
                                                               long nblk, long nb,
                                                               double2* __restrict__ out) {
  const long c = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int s = (int)blk * kBlock + threadIdx.x;
  if (s >= d.V) return;
  const double2* xc = xn + c * 36L * d.V;
  const Site p = site_coords(s, d);
  const int V = d.V;
  int plane = 0;
#pragma unroll 1
  for (int u = 1; u < 4; ++u) {
    const int s_pu = fwd(s, coord_of(p, u), d, u);
#pragma unroll 1
    for (int v = 0; v < u; ++v, ++plane) {
      const int s_pv = fwd(s, coord_of(p, v), d, v);
      double sr = 0.0, si = 0.0;
      M3 a, b, yuv;
      load_link(a, xc + u * 9 * V, V, s);
      load_link(b, xc + v * 9 * V, V, s_pu);
      m3_mul_nn(yuv, a, b);
      load_link(a, xc + v * 9 * V, V, s);
      load_link(b, xc + u * 9 * V, V, s_pv);
      m3_trace_y_abh(sr, si, yuv, a, b);
      out[(plane * nb + c) * V + s] = make_double2(sr, si);
    }
  }
}

// per-chain sum |a - b|^2 over n doubles (complex fields pass 2n)
__global__ __launch_bounds__(kBlock) void diff_norm2_kernel(const double* __restrict__ a,
                                                            const double* __restrict__ b, long n,
                                                            long nblk, double* __restrict__ partial) {
  __shared__ double lds[4];
  const long c = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  double acc = 0.0;
  const long base = blk * (4L * kBlock);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long j = base + (long)k * kBlock + threadIdx.x;
    if (j < n) {
      const double dlt = a[c * n + j] - b[c * n + j];
      acc = fma(dlt, dlt, acc);
    }
  }
  const double r = block_sum(acc, lds);
  if (threadIdx.x == 0) partial[c * nblk + blk] = r;
}

// ------------------------------------------------------------------ plaquette, slice-resident
// One workgroup = 128 spatial sites of one chain, sweeping t.  LDS holds the 4 links of the
// CURRENT time slice for the tile ([4][9][128] complex = 72 KiB); the NEXT slice's links are
// prefetched into registers while the current slice is being computed and become the LDS
// tile of the next iteration.  Every link is therefore fetched from HBM exactly once per
// sweep (plus the x-halo of the tile): own links, +y/+z(/+x) neighbours come from LDS, the
// +t neighbours from the prefetch registers.  (The flat kernel moves 2.7x the algorithmic
// bytes through the fabric and is bound by that.)
constexpr int kSlice = 128;

__device__ __forceinline__ void lds_store_link(double2* tile, int rho, int li, const M3& m) {
#pragma unroll
  for (int e = 0; e < 9; ++e) tile[(rho * 9 + e) * kSlice + li] = make_double2(m.re[e], m.im[e]);
}

// link rho through a (base, stride) pair that points either into the LDS tile (stride 128)
// or into the global slice (stride V): one code path, flat addressing
struct SliceRef {
  const double2* base;   // entry e of link rho at base[(rho * 9 + e) * stride]
  int stride;
};

// own-site link: always in the tile -> plain ds_read_b128
__device__ __forceinline__ void slice_own(M3& m, const double2* tile, int rho, int li) {
  const double2* l = tile + rho * 9 * kSlice + li;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    const double2 dd = l[e * kSlice];
    m.re[e] = dd.x; m.im[e] = dd.y;
  }
}

// neighbour link: LDS when the (wave-uniform, loop-invariant) direction is known in-tile
template <bool LDS>
__device__ __forceinline__ void slice_nbr(M3& m, const SliceRef& r, const double2* tile, int lnb,
                                          int rho);
template <>
__device__ __forceinline__ void slice_nbr<true>(M3& m, const SliceRef&, const double2* tile,
                                                int lnb, int rho) {
  slice_own(m, tile, rho, lnb);
}

__device__ __forceinline__ void slice_link(M3& m, const SliceRef& r, int rho) {
  const double2* p = r.base + rho * 9 * r.stride;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    const double2 dd = p[e * r.stride];
    m.re[e] = dd.x; m.im[e] = dd.y;
  }
}

template <>
__device__ __forceinline__ void slice_nbr<false>(M3& m, const SliceRef& r, const double2*, int,
                                                 int rho) {
  slice_link(m, r, rho);
}

// YZ: +y and +z neighbours of every lane are inside the tile (e.g. the tile is a stack of
// whole (y,z) planes) -> plain LDS reads for them; +x stays on the generic flat path.
template <bool YZ>
__global__ __launch_bounds__(kSlice, 1) void su3_plaq_slice_kernel(
    const double2* __restrict__ xn, Dims d, int nsb, int tsplit, int swz,
    double* __restrict__ partial) {
  __shared__ double2 tile[4 * 9 * kSlice];
  __shared__ double red[8];
  const long w = xcd_swizzle(blockIdx.x, gridDim.x, swz);
  const int per_chain = nsb * tsplit;
  const long c = w / per_chain;
  const int r = (int)(w % per_chain);
  const int tc = r / nsb, sb = r % nsb;
  const int Vs = d.X * d.Y * d.Z, V = d.V;
  const int tile0 = sb * kSlice;
  const int li = threadIdx.x;
  const int sp = tile0 + li;                            // spatial site (Vs % 128 == 0)
  const int tlen = (d.T + tsplit - 1) / tsplit;
  const int t0 = tc * tlen, t1 = min(d.T, t0 + tlen);
  const double2* xc = xn + c * 36L * V;
  // periodic spatial neighbours (indices within a slice)
  int sn[4];
  {
    int q = sp;
    const int z = q % d.Z; q /= d.Z;
    const int y = q % d.Y; q /= d.Y;
    const int x = q;
    sn[0] = sp;
    sn[1] = (x + 1 == d.X) ? sp - (d.X - 1) * d.Y * d.Z : sp + d.Y * d.Z;
    sn[2] = (y + 1 == d.Y) ? sp - (d.Y - 1) * d.Z : sp + d.Z;
    sn[3] = (z + 1 == d.Z) ? sp - (d.Z - 1) : sp + 1;
  }
  bool in_tile[4];                                      // wave-uniform, loop-invariant
#pragma unroll
  for (int u = 0; u < 4; ++u) in_tile[u] = __all((unsigned)(sn[u] - tile0) < (unsigned)kSlice);
  M3 nxt[4];
#pragma unroll
  for (int rho = 0; rho < 4; ++rho) load_link(nxt[rho], xc + rho * 9 * V, V, t0 * Vs + sp);
  double sr = 0.0, si = 0.0;
#pragma unroll 1
  for (int t = t0; t < t1; ++t) {
    __syncthreads();                                    // previous slice fully consumed
#pragma unroll
    for (int rho = 0; rho < 4; ++rho) lds_store_link(tile, rho, li, nxt[rho]);
    __syncthreads();
    const int tn = (t + 1 == d.T) ? 0 : t + 1;
    // prefetch the next slice: U_1..U_3 now (needed by the temporal planes below), U_0 after
    // the spatial planes (only needed as next iteration's tile) to cap register pressure
#pragma unroll
    for (int rho = 1; rho < 4; ++rho) load_link(nxt[rho], xc + rho * 9 * V, V, tn * Vs + sp);
    const double2* xs = xc + (long)t * Vs;              // base of slice t (index by spatial site)
    SliceRef nb_[4];                                    // own site and +x, +y, +z neighbours
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      nb_[u].base = in_tile[u] ? (const double2*)(tile + (sn[u] - tile0)) : (xs + sn[u]);
      nb_[u].stride = in_tile[u] ? kSlice : V;
    }
    // spatial-spatial planes (u, v) = (2,1), (3,1), (3,2): everything in the current slice
    {
      M3 a, b, yuv;
      slice_own(a, tile, 2, li); slice_nbr<YZ>(b, nb_[2], tile, sn[2] - tile0, 1); m3_mul_nn(yuv, a, b);
      slice_own(a, tile, 1, li); slice_link(b, nb_[1], 2); m3_trace_y_abh(sr, si, yuv, a, b);
    }
    {
      M3 a, b, yuv;
      slice_own(a, tile, 3, li); slice_nbr<YZ>(b, nb_[3], tile, sn[3] - tile0, 1); m3_mul_nn(yuv, a, b);
      slice_own(a, tile, 1, li); slice_link(b, nb_[1], 3); m3_trace_y_abh(sr, si, yuv, a, b);
    }
    {
      M3 a, b, yuv;
      slice_own(a, tile, 3, li); slice_nbr<YZ>(b, nb_[3], tile, sn[3] - tile0, 2); m3_mul_nn(yuv, a, b);
      slice_own(a, tile, 2, li); slice_nbr<YZ>(b, nb_[2], tile, sn[2] - tile0, 3); m3_trace_y_abh(sr, si, yuv, a, b);
    }
    // temporal planes (u, 0): U_u(s) U_0(s+u) (U_0(s) U_u(s+t))^H, U_u(s+t) = prefetched link
    load_link(nxt[0], xc, V, tn * Vs + sp);
    {
      M3 a, b, yuv;
      slice_own(a, tile, 1, li); slice_link(b, nb_[1], 0); m3_mul_nn(yuv, a, b);
      slice_own(a, tile, 0, li); m3_trace_y_abh(sr, si, yuv, a, nxt[1]);
    }
    {
      M3 a, b, yuv;
      slice_own(a, tile, 2, li); slice_nbr<YZ>(b, nb_[2], tile, sn[2] - tile0, 0); m3_mul_nn(yuv, a, b);
      slice_own(a, tile, 0, li); m3_trace_y_abh(sr, si, yuv, a, nxt[2]);
    }
    {
      M3 a, b, yuv;
      slice_own(a, tile, 3, li); slice_nbr<YZ>(b, nb_[3], tile, sn[3] - tile0, 0); m3_mul_nn(yuv, a, b);
      slice_own(a, tile, 0, li); m3_trace_y_abh(sr, si, yuv, a, nxt[3]);
    }
  }
  // block reduction (2 waves)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { sr += __shfl_down(sr, off, 64); si += __shfl_down(si, off, 64); }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[(threadIdx.x >> 6) * 2] = sr; red[(threadIdx.x >> 6) * 2 + 1] = si; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[(c * per_chain + r) * 2 + 0] = red[0] + red[2];
    partial[(c * per_chain + r) * 2 + 1] = red[1] + red[3];
  }
}

// ------------------------------------------------------------------ per-link kernels
// out = keep (.) x + expm(eps v) @ ((1-keep) (.) x).  TWO: the two half-updates of one
// leapfrog step (keep = mask then keep = 1 - mask, or the reverse order when `complement`)
// applied back to back with ONE expm(eps v) and one pass over x -- both are local to a link.
// VEC8: additionally emit su3_to_vec(projectSU(x')) (the vnet input of the next v-update,
// group/su3/pytorch/group.py:138-147) while x' is in registers -- saves the pass that re-reads it.
#ifndef XU_OCC
#define XU_OCC 3        // wavefronts per SIMD the x-update is compiled for (A/B builds override)
#endif
// The eight vec8 values of link (f, s) -> their digits in the activation image of the int8-sliced input layer
// (digits.hpp; row = chain, k = ((mu 8 + a) V + s), V % 64 == 0: the 64 sites of a wavefront are one slab of the
// row).  Called by whole wavefronts.  Returns nonzero for a
// value outside (-lim, lim) or a NaN.
__device__ __forceinline__ int su3_vec8_to_digits(const double (&w)[8], char* img, long f, int s, int V, double dsc,
                                                  double dlim) {
  const int lane = threadIdx.x & 63;
  char* slab = img + ((f >> 2) * (V >> 1) + (f & 3) * 8L * (V >> 6) + (s >> 6)) * GD_SLAB;
  int bad = 0;
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    unsigned dl, dh;
    bad |= gd_digits(w[a], dsc, dlim, dl, dh);
    gd_store_slab(slab + a * (long)(V >> 6) * GD_SLAB, lane, dl, dh);
  }
  return bad;
}
// The 18 values of a matrix through an empty asm: what was computed before this point is complete here and
// nothing after it is moved in front.  The instantiations of su3_expm_mul_body must give each other's bits
// (links, vec8, digits of the same arguments), and m3_expm leaves its multiply-adds to the compiler, which
// fuses only inside a basic block: without the pin the optimiser moved part of the exponential's last sums
// into a later block in ONE instantiation (the digits one, after its tail changed) and its links differed in
// the last bit from the other two.
__device__ __forceinline__ void m3_pin(M3& m) {
#pragma unroll
  for (int i = 0; i < 9; ++i) asm volatile("" : "+v"(m.re[i]), "+v"(m.im[i]));
}
// VEC: 0 links only, 1 + vec8 as fp64 (out_vec), 2 + vec8 as digits (out_vec is the image; V % 64 == 0)
template <bool TWO, int VEC>
__device__ __forceinline__ void su3_expm_mul_body(const double2* xn, const double2* __restrict__ vn, double eps,
                                                  const float* __restrict__ mask, int complement, double2* out,
                                                  void* __restrict__ out_vec, int V, long f, int s, int lo,
                                                  double dsc, double dlim, int* flag) {
  const int mu = (int)(f & 3);
  // The three stages below sit in run-time conditionals that are always taken (`lo` = 0 is a kernel
  // ARGUMENT): hipcc then allocates each stage on its own instead of scheduling the exponential, the
  // masked products and the projection as one straight line with all their temporaries live
  // (218 VGPRs, two wavefronts per SIMD; capped at 168 it spilled 52).  Staged, with the masked copies of
  // x formed inside the product: 182 VGPRs uncapped, 168 with 10 spilled at three wavefronts per SIMD,
  // x-update 0.423 -> 0.402 ms at cfg-4 (the same staging at two wavefronts per SIMD: 0.443 ms).
  M3 x, e;
  load_link(e, vn + f * 9L * V, V, s);
  if (s >= lo) {
    M3 a;
#pragma unroll
    for (int i = 0; i < 9; ++i) { a.re[i] = e.re[i] * eps; a.im[i] = e.im[i] * eps; }
    m3_expm(e, a);
    m3_pin(e);
  }
  // (the link is requested only now: it would otherwise be live across the exponential; the other
  // wavefronts of the SIMD cover its latency)
  load_link(x, xn + f * 9L * V, V, s);
  if (mask != nullptr) {
    const float* mk = mask + mu * 9 * V;
    float keep[9];                           // 0 / 1 masks: exact in fp32, half the registers
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const float k = mk[i * V + s];
      keep[i] = complement ? 1.0f - k : k;
    }
    // m <- keep (.) m + e @ ((1 - keep) (.) m), IN PLACE and column by column: entry (i, j) of the
    // result needs column j of m only, so a column is read (masked copy formed on the fly), its
    // three results are formed and written back before the next column is touched -- the live set
    // is e, m, the masks and one column (no second and third copy of the link: that is what took
    // the staged kernel over the 168-register budget of three wavefronts per SIMD, 10 spilled).
    // Same products in the same order as the two-copy form: identical bits.
    auto half = [&](M3& m, bool flip) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        double cr[3], ci[3], ki[3];
#pragma unroll
        for (int kk = 0; kk < 3; ++kk) {
          const double kq = flip ? 1.0 - (double)keep[3 * kk + j] : (double)keep[3 * kk + j];
          cr[kk] = (1.0 - kq) * m.re[3 * kk + j]; ci[kk] = (1.0 - kq) * m.im[3 * kk + j];
          ki[kk] = kq;
        }
        double orr[3], oi[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          double sr = 0.0, si = 0.0;
#pragma unroll
          for (int kk = 0; kk < 3; ++kk) {
            const double ar = e.re[3 * i + kk], ai = e.im[3 * i + kk];
            sr = fma(ar, cr[kk], sr); sr = fma(-ai, ci[kk], sr);
            si = fma(ar, ci[kk], si); si = fma(ai, cr[kk], si);
          }
          orr[i] = fma(ki[i], m.re[3 * i + j], sr);
          oi[i] = fma(ki[i], m.im[3 * i + j], si);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) { m.re[3 * i + j] = orr[i]; m.im[3 * i + j] = oi[i]; }
      }
    };
    if (s >= lo) half(x, false);
    if (TWO) {
      if (s >= lo) half(x, true);
    }
  } else {
    if (s >= lo) {
      M3 r;
      m3_mul_nn(r, e, x);
      x = r;
    }
  }
  M3& r = x;
  m3_pin(r);
  store_link(out + f * 9L * V, V, s, r);
  if constexpr (VEC != 0) {
    if (s >= lo) {
      double w[8];
      m3_project_su_vec8(w, r);
      if constexpr (VEC == 1) {
#pragma unroll
        for (int a = 0; a < 8; ++a) static_cast<double*>(out_vec)[(f * 8 + a) * (long)V + s] = w[a];
      } else {
        if (su3_vec8_to_digits(w, static_cast<char*>(out_vec), f, s, V, dsc, dlim)) atomicOr(flag, 1);
      }
    }
  }
}
template <bool TWO, bool VEC8>
__global__ __launch_bounds__(kBlock, XU_OCC) void su3_expm_mul_kernel(const double2* xn,
                                                              const double2* __restrict__ vn,
                                                              double eps,
                                                              const float* __restrict__ mask,
                                                              int complement, double2* out,
                                                              double* __restrict__ out_vec,
                                                              int V, long nblk, int lo) {
  const long f = blockIdx.x / nblk, blk = blockIdx.x % nblk;     // f = chain*4 + mu
  const int s = (int)blk * kBlock + threadIdx.x;
  if (s >= V) return;
  su3_expm_mul_body<TWO, VEC8 ? 1 : 0>(xn, vn, eps, mask, complement, out, out_vec, V, f, s, lo, 0.0, 0.0, nullptr);
}
// the two half-updates + the digits of su3_to_vec(projectSU(x')) instead of its fp64 values
__global__ __launch_bounds__(kBlock, XU_OCC) void su3_expm_mul_digits_kernel(const double2* xn,
                                                                     const double2* __restrict__ vn, double eps,
                                                                     const float* __restrict__ mask, int complement,
                                                                     double2* out, char* __restrict__ image, int V,
                                                                     long nblk, int lo, double dsc, double dlim,
                                                                     int* flag) {
  const long f = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int s = (int)blk * kBlock + threadIdx.x;
  if (s >= V) return;                                           // (V % 64 == 0: whole wavefronts)
  su3_expm_mul_body<true, 2>(xn, vn, eps, mask, complement, out, image, V, f, s, lo, dsc, dlim, flag);
}

// MODE 0: projectSU -> links;  1: projectSU -> vec8;  2: projectTAH -> links;  3: projectU
template <int MODE>
__global__ __launch_bounds__(kBlock) void su3_project_kernel(const double2* in,
                                                             double2* out_links,
                                                             double* __restrict__ out_vec, int V,
                                                             long nblk) {
  const long f = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int s = (int)blk * kBlock + threadIdx.x;
  if (s >= V) return;
  M3 x, r;
  load_link(x, in + f * 9L * V, V, s);
  if constexpr (MODE == 1) {
    double v[8];
    m3_project_su_vec8(v, x);
#pragma unroll
    for (int a = 0; a < 8; ++a) out_vec[(f * 8 + a) * (long)V + s] = v[a];
  } else {
    if (MODE == 2) {
      m3_tah(r, x);
    } else if (MODE == 3) {
      m3_project_u(r, x);
    } else {
      m3_project_su(r, x);
    }
    store_link(out_links + f * 9L * V, V, s, r);
  }
}
// projectSU -> the digits of vec8 (V % 64 == 0: whole wavefronts)
__global__ __launch_bounds__(kBlock) void su3_project_digits_kernel(const double2* in, char* __restrict__ image, int V,
                                                                    long nblk, double dsc, double dlim, int* flag) {
  const long f = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int s = (int)blk * kBlock + threadIdx.x;
  if (s >= V) return;
  M3 x;
  load_link(x, in + f * 9L * V, V, s);
  double v[8];
  m3_project_su_vec8(v, x);
  if (su3_vec8_to_digits(v, image, f, s, V, dsc, dlim)) atomicOr(flag, 1);
}
// ... of an anti-Hermitian field given in upper-plane form ([f][6][V], su3_math.hpp: m3_from_upper): six loads, the
// other three entries rebuilt in registers; the bytes of su3_project_digits_kernel on the full field
__global__ __launch_bounds__(kBlock) void su3_project_digits_upper_kernel(const double2* in, char* __restrict__ image,
                                                                          int V, long nblk, double dsc, double dlim,
                                                                          int* flag) {
  const long f = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int s = (int)blk * kBlock + threadIdx.x;
  if (s >= V) return;
  double2 u[6];
#pragma unroll
  for (int p = 0; p < 6; ++p) u[p] = in[(f * 6L + p) * V + s];
  M3 x;
  m3_from_upper(x, u);
  double v[8];
  m3_project_su_vec8(v, x);
  if (su3_vec8_to_digits(v, image, f, s, V, dsc, dlim)) atomicOr(flag, 1);
}
// The trajectory's entry: reference layout x[f][site][9] -> the native planes (the bits of l2q_su3_pack) AND the
// digits of vec8(projectSU(x)) (the bytes of su3_project_digits_kernel on those planes) from one read of x.  The
// 64 links of a wavefront are 9216 contiguous bytes of x: read as nine lane-linear 16-byte loads, turned through
// LDS (each wavefront its own 576 entries), after which lane <-> site holds its link as the other kernels do.
// V % 64 == 0: whole wavefronts; one past the field (V % kBlock != 0) only waits at the barrier.
__global__ __launch_bounds__(kBlock) void su3_pack_digits_kernel(const double2* __restrict__ xref,
                                                                 double2* __restrict__ xn, char* __restrict__ image,
                                                                 int V, long nblk, double dsc, double dlim, int* flag) {
  __shared__ double2 tile[kBlock * 9];
  const long f = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int s = (int)blk * kBlock + threadIdx.x;
  const bool live = s < V;
  double2* t = tile + w * 576;
  if (live) {
    const double2* src = xref + (f * V + (s - lane)) * 9L;
#pragma unroll
    for (int k = 0; k < 9; ++k) t[lane + 64 * k] = src[lane + 64 * k];
  }
  __syncthreads();
  if (!live) return;
  M3 x;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    const double2 d = t[lane * 9 + e];
    x.re[e] = d.x; x.im[e] = d.y;
  }
  store_link(xn + f * 9L * V, V, s, x);
  double v[8];
  m3_project_su_vec8(v, x);
  if (su3_vec8_to_digits(v, image, f, s, V, dsc, dlim)) atomicOr(flag, 1);
}

// out = op(a) * op(b) per link, op = identity or adjoint   (SU3.mul, group.py:56-69)
__global__ __launch_bounds__(kBlock) void su3_mul_kernel(const double2* a, const double2* b,
                                                         int adj_a, int adj_b, double2* out, int V,
                                                         long nblk) {
  const long f = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int s = (int)blk * kBlock + threadIdx.x;
  if (s >= V) return;
  M3 x, y, r;
  load_link(x, a + f * 9L * V, V, s);
  load_link(y, b + f * 9L * V, V, s);
  if (adj_a && adj_b) m3_mul_aa(r, x, y);
  else if (adj_a) m3_mul_an(r, x, y);
  else if (adj_b) m3_mul_na(r, x, y);
  else m3_mul_nn(r, x, y);
  store_link(out + f * 9L * V, V, s, r);
}

// the momentum of link (field f, site s); returns the sum of |entry|^2 over its nine entries as stored
__device__ __forceinline__ double assemble_tah_link(const double* __restrict__ nrm, double2* __restrict__ vn,
                                                    long V, long nlinks, long f, long s) {
  const long l = f * V + s;
  const double h = 0.70710678118654757;          // sqrt(1/2)
  const double r3 = h * nrm[0 * nlinks + l];
  const double r8 = h * 0.57735026918962573 * nrm[1 * nlinks + l];
  const double r01 = h * nrm[2 * nlinks + l], r02 = h * nrm[3 * nlinks + l];
  const double r12 = h * nrm[4 * nlinks + l], i01 = h * nrm[5 * nlinks + l];
  const double i02 = h * nrm[6 * nlinks + l], i12 = h * nrm[7 * nlinks + l];
  double2* o = vn + f * 9 * V;
  const double2 m[9] = {make_double2(0.0, r8 + r3), make_double2(r01, i01),      make_double2(r02, i02),
                        make_double2(-r01, i01),    make_double2(0.0, r8 - r3),  make_double2(r12, i12),
                        make_double2(-r02, i02),    make_double2(-r12, i12),     make_double2(0.0, -2.0 * r8)};
  double acc = 0.0;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    o[e * V + s] = m[e];
    acc = fma(m[e].x, m[e].x, acc);
    acc = fma(m[e].y, m[e].y, acc);
  }
  return acc;
}

__global__ __launch_bounds__(kBlock) void su3_assemble_tah_kernel(const double* __restrict__ nrm,
                                                                  double2* __restrict__ vn, long V,
                                                                  long nblk, long nlinks) {
  const long f = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const long s = blk * kBlock + threadIdx.x;
  if (s >= V) return;
  (void)assemble_tah_link(nrm, vn, V, nlinks, f, s);
}

// the same with partial[f][blk] = the block's sum of |entry|^2: the four fields of a chain are adjacent, so a
// chain's partials are contiguous (l2q_su3_assemble_tah_norm2 sums them in a fixed order)
__global__ __launch_bounds__(kBlock) void su3_assemble_tah_norm2_kernel(const double* __restrict__ nrm,
                                                                        double2* __restrict__ vn, long V,
                                                                        long nblk, long nlinks,
                                                                        double* __restrict__ partial) {
  __shared__ double lds[4];
  const long f = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const long s = blk * kBlock + threadIdx.x;
  const double acc = s < V ? assemble_tah_link(nrm, vn, V, nlinks, f, s) : 0.0;
  const double r = block_sum(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// per-chain sum over all 36 V complex entries of |p|^2; the -8 per link and the 1/2 are
// applied in the finalize stage through `scale` and an offset there.
__global__ __launch_bounds__(kBlock) void su3_norm2_kernel(const double2* __restrict__ vn,
                                                           long n_per_chain, long nblk,
                                                           double* __restrict__ partial) {
  __shared__ double lds[4];
  const long c = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const double2* v = vn + c * n_per_chain;
  double acc = 0.0;
  // each block owns a contiguous run of 4 * kBlock entries
  const long base = blk * (4L * kBlock);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long j = base + (long)k * kBlock + threadIdx.x;
    if (j < n_per_chain) {
      const double2 d = v[j];
      acc = fma(d.x, d.x, acc);
      acc = fma(d.y, d.y, acc);
    }
  }
  const double r = block_sum(acc, lds);
  if (threadIdx.x == 0) partial[c * nblk + blk] = r;
}

__global__ __launch_bounds__(kBlock) void su3_check_kernel(const double2* __restrict__ xn, long V,
                                                           long nblk, double* __restrict__ psum,
                                                           double* __restrict__ pmax) {
  __shared__ double lds[8];
  const long c = blockIdx.x / nblk, blk = blockIdx.x % nblk;   // blk over 4 V links
  const long l = blk * kBlock + threadIdx.x;
  double dv = 0.0;
  const bool on = l < 4 * V;
  if (on) {
    const long mu = l / V, s = l % V;
    M3 x, t;
    load_link(x, xn + (c * 4 + mu) * 9L * V, (int)V, (int)s);
    m3_mul_an(t, x, x);
    t.re[0] -= 1.0; t.re[4] -= 1.0; t.re[8] -= 1.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) dv += t.re[i] * t.re[i] + t.im[i] * t.im[i];
    double dr, di;
    m3_det(dr, di, x);
    dv += (dr - 1.0) * (dr - 1.0) + di * di;
  }
  const double bs = block_sum(dv, lds);
  const double bm = block_max(dv, lds + 4);
  if (threadIdx.x == 0) { psum[c * nblk + blk] = bs; pmax[c * nblk + blk] = bm; }
}

__global__ void check_finalize_kernel(const double* __restrict__ psum,
                                      const double* __restrict__ pmax, long nblk, double nlinks,
                                      double* __restrict__ out) {
  __shared__ double lds[8];
  const long c = blockIdx.x;
  double s = 0.0, m = 0.0;
  for (long b = threadIdx.x; b < nblk; b += blockDim.x) {
    s += psum[c * nblk + b];
    m = fmax(m, pmax[c * nblk + b]);
  }
  const double ts = block_sum(s, lds);
  const double tm = block_max(m, lds + 4);
  if (threadIdx.x == 0) {
    out[c * 2 + 0] = sqrt(ts / nlinks / 20.0);
    out[c * 2 + 1] = sqrt(tm / 20.0);
  }
}

}  // namespace l2q

using namespace l2q;

// The plaquette sum: the slice-resident kernel where the spatial volume is whole tiles -- <true> where the tile is
// whole (y, z) planes (Y*Z | 128), which keeps +y, +z inside it -- else the flat kernel.
enum class PlaqKernel { SliceYZ, Slice, Flat };
constexpr int kPlaqOcc = 2;
static PlaqKernel pick_plaq(const Dims& d) {
  if ((d.X * d.Y * d.Z) % kSlice != 0) return PlaqKernel::Flat;
  return kSlice % (d.Y * d.Z) == 0 ? PlaqKernel::SliceYZ : PlaqKernel::Slice;
}

// What the entries that write a digit image (digits.hpp) check, in this order: their pointers, their shape (with its
// own text), the operand exponent and the image's alignment; then `flag` is the device address of the overflow flag.
static int digits_checks(const char* what, bool ptrs_ok, bool shape_ok, const char* shape_msg, int a_exp,
                         const void* image, int*& flag) {
  L2Q_REQUIRE_W(ptrs_ok, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE_W(shape_ok, L2Q_EINVAL, shape_msg);
  L2Q_REQUIRE_W(a_exp > -900 && a_exp < 900, L2Q_EINVAL, "bad operand exponent");
  L2Q_REQUIRE_W((reinterpret_cast<uintptr_t>(image) & 15) == 0, L2Q_ESHAPE, "the image must be 16-byte aligned");
  flag = gs_flag();
  L2Q_REQUIRE_W(flag, L2Q_EHIP, "device symbol gs_flag_dev not found");
  return L2Q_OK;
}

// l2q_su3_projsu_digits and l2q_su3_projsu_digits_upper: the same launch of either kernel
static int projsu_digits(const char* what, decltype(&su3_project_digits_kernel) kern, const void* in, void* image,
                         int a_exp, long nfields, long V, void* stream) {
  int* flag;
  const int rc = digits_checks(what, in && image, su3_field_ok(nfields, V) && V % 64 == 0 && nfields % 4 == 0,
                               "the digit image serves whole chains (4 fields each) with V % 64 == 0", a_exp, image, flag);
  if (rc != L2Q_OK) return rc;
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(kern, dim3((unsigned)(nfields * nblk)), dim3(kBlock), 0, (hipStream_t)stream, (const double2*)in,
                     (char*)image, (int)V, nblk, ldexp(1.0, GS_BITS - a_exp), ldexp(1.0, a_exp), flag);
  return check_launch(what);
}

extern "C" {

int l2q_kernel_name(const char* entry, int T, int X, int Y, int Z, char* buf, size_t buf_bytes) {
  L2Q_REQUIRE(entry && buf && buf_bytes > 0, L2Q_EINVAL, "null pointer");
  const Dims dd = strncmp(entry, "l2q_su3_", 8) ? Dims{} : make_dims(T, X, Y, Z);   // (other entries: not a lattice)
  buf[0] = 0;
  if (force_entry_kernel_name(entry, dd, buf, buf_bytes)) return L2Q_OK;      // the force entry points: su3_force.hip
  if (!strcmp(entry, "l2q_su3_plaq_reduce")) {
    const PlaqKernel pk = pick_plaq(dd);
    if (pk == PlaqKernel::Flat) snprintf(buf, buf_bytes, "su3_plaq_kernel<%d>", kPlaqOcc);
    else snprintf(buf, buf_bytes, "su3_plaq_slice_kernel<%s>", pk == PlaqKernel::SliceYZ ? "true" : "false");
  } else if (!strcmp(entry, "l2q_su3_projsu_digits_upper")) {
    snprintf(buf, buf_bytes, "su3_project_digits_upper_kernel");
  } else if (!strcmp(entry, "l2q_su3_clover_reduce")) {
    snprintf(buf, buf_bytes, "%s", clover_slice_applicable(dd) ? "su3_clover_slice_kernel" : "su3_clover_kernel");
  } else if (!strcmp(entry, "l2q_su3_flow_stage")) {
    // the kick of l2q_su3_force_kick_to (out of place: only the thread-per-link kernel has that form, the others
    // follow a copy), then the unmasked x-update
    char kick[128];
    (void)force_entry_kernel_name("l2q_su3_force_kick", dd, kick, sizeof(kick));
    snprintf(buf, buf_bytes, "%s + su3_expm_mul_kernel<false, false>", kick);
  } else if (!strcmp(entry, "l2q_vnet_heads_vupdate_sliced_f64") ||
             !strcmp(entry, "l2q_vnet_heads_vupdate_sliced_upper_f64")) {
    snprintf(buf, buf_bytes, "heads_sliced_kernel");
  } else if (!strncmp(entry, "l2q_vnet_heads_vupdate", 22)) {
    snprintf(buf, buf_bytes, "%s", heads_f64_kernel_name());
  } else if (!strcmp(entry, "l2q_gemm_h")) {
    snprintf(buf, buf_bytes, "%s", gemm_h_kernel_name(T, X, (long)Y));      // (T, X, Y) carry (M, N, K) here
  } else if (!strcmp(entry, "l2q_gemm_sliced_f64")) {
    snprintf(buf, buf_bytes, "gemm_sliced_kernel");
  } else if (!strcmp(entry, "l2q_gemm_digits_f64")) {
    snprintf(buf, buf_bytes, "gemm_digits_kernel");
  } else if (!strcmp(entry, "l2q_gemm_digits_slice")) {
    snprintf(buf, buf_bytes, "gd_slice_kernel");
  } else if (!strcmp(entry, "l2q_su3_expm_mul2_digits")) {
    snprintf(buf, buf_bytes, "su3_expm_mul_digits_kernel");
  } else if (!strcmp(entry, "l2q_su3_projsu_digits")) {
    snprintf(buf, buf_bytes, "su3_project_digits_kernel");
  } else if (!strcmp(entry, "l2q_su3_pack_digits")) {
    snprintf(buf, buf_bytes, "su3_pack_digits_kernel");
  } else if (!strcmp(entry, "l2q_gemm_f64")) {
    snprintf(buf, buf_bytes, "%s", gemm_f64_kernel_name());
  }
  return L2Q_OK;
}

size_t l2q_reduce_ws_bytes(int nb, long n_per_chain) {
  if (nb <= 0 || n_per_chain <= 0) return 0;
  // two partial arrays of up to 2 doubles per 256-item block
  return (size_t)nb * (size_t)cdiv(n_per_chain, kBlock) * 4 * sizeof(double) + 256;
}

int l2q_su3_plaq_reduce(const void* xn, int nb, int T, int X, int Y, int Z, double* out, void* ws,
                        size_t ws_bytes, void* stream) {
  L2Q_REQUIRE(xn && out && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  const Dims d = make_dims(T, X, Y, Z);
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)ws;
  const int swz = tuning().xcd_swizzle;
  const PlaqKernel pk = pick_plaq(d);
  if (pk != PlaqKernel::Flat) {
    const SliceGrid g = slice_grid(d, nb, kSlice, 1024);      // keep >= ~1024 workgroups
    L2Q_REQUIRE(ws_bytes >= (size_t)nb * g.per_chain * 2 * sizeof(double), L2Q_ESHAPE, "workspace too small");
    const auto kern = pk == PlaqKernel::SliceYZ ? su3_plaq_slice_kernel<true> : su3_plaq_slice_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)g.blocks), dim3(kSlice), 0, st, (const double2*)xn, d, g.nsb, g.tsplit, swz,
                       partial);
    launch_finalize(partial, out, nb, g.per_chain, 2, 1.0, 0.0, st);
    return check_launch("l2q_su3_plaq_reduce");
  }
  const long nblk = cdiv(d.V, kBlock);
  L2Q_REQUIRE(ws_bytes >= (size_t)nb * nblk * 2 * sizeof(double), L2Q_ESHAPE, "workspace too small");
  hipLaunchKernelGGL(su3_plaq_kernel<kPlaqOcc>, dim3((unsigned)(nb * nblk)), dim3(kBlock), 0, st,
                     (const double2*)xn, d, nblk, swz, partial);
  launch_finalize(partial, out, nb, nblk, 2, 1.0, 0.0, st);
  return check_launch("l2q_su3_plaq_reduce");
}

int l2q_su3_wilson_loops(const void* xn, int nb, int T, int X, int Y, int Z, void* out, void* stream) {
  L2Q_REQUIRE(xn && out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V, kBlock);
  hipLaunchKernelGGL(su3_wloops_kernel, dim3((unsigned)(nb * nblk)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const double2*)xn, d, nblk, (long)nb, (double2*)out);
  return check_launch("l2q_su3_wilson_loops");
}

int l2q_su3_plaq_planes(const void* xn, int nb, int T, int X, int Y, int Z, double* out, void* ws,
                        size_t ws_bytes, void* stream) {
  L2Q_REQUIRE(xn && out && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V, kBlock);
  L2Q_REQUIRE(ws_bytes >= (size_t)nb * nblk * 12 * sizeof(double), L2Q_ESHAPE, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(su3_plaq_planes_kernel, dim3((unsigned)(nb * nblk)), dim3(kBlock), 0, st,
                     (const double2*)xn, d, nblk, (double*)ws);
  launch_finalize((const double*)ws, out, nb, nblk, 12, 1.0, 0.0, st);
  return check_launch("l2q_su3_plaq_planes");
}

int l2q_diff_norm2_reduce(const double* a, const double* b, int nb, long n, double* out, void* ws,
                          size_t ws_bytes, void* stream) {
  L2Q_REQUIRE(a && b && out && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(nb > 0 && n > 0, L2Q_EINVAL, "non-positive size");
  const long nblk = cdiv(n, 4L * kBlock);
  L2Q_REQUIRE(ws_bytes >= (size_t)nb * nblk * sizeof(double), L2Q_ESHAPE, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(diff_norm2_kernel, dim3((unsigned)(nb * nblk)), dim3(kBlock), 0, st, a, b, n,
                     nblk, (double*)ws);
  launch_finalize((const double*)ws, out, nb, nblk, 1, 1.0, 0.0, st);
  return check_launch("l2q_diff_norm2_reduce");
}

int l2q_su3_expm_mul(const void* xn, const void* vn, double eps, const float* mask_n,
                     int complement, void* out, int nb, long V, void* stream) {
  L2Q_REQUIRE(xn && vn && out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_field_ok(nb, V), L2Q_EINVAL, "bad size");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL((su3_expm_mul_kernel<false, false>), dim3((unsigned)(nb * 4L * nblk)), dim3(kBlock),
                     0, (hipStream_t)stream, (const double2*)xn, (const double2*)vn, eps, mask_n,
                     complement, (double2*)out, (double*)nullptr, (int)V, nblk, 0);
  return check_launch("l2q_su3_expm_mul");
}

int l2q_su3_expm_mul2(const void* xn, const void* vn, double eps, const float* mask_n,
                      int complement_first, void* out, int nb, long V, void* stream) {
  L2Q_REQUIRE(xn && vn && out && mask_n, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_field_ok(nb, V), L2Q_EINVAL, "bad size");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL((su3_expm_mul_kernel<true, false>), dim3((unsigned)(nb * 4L * nblk)), dim3(kBlock),
                     0, (hipStream_t)stream, (const double2*)xn, (const double2*)vn, eps, mask_n,
                     complement_first, (double2*)out, (double*)nullptr, (int)V, nblk, 0);
  return check_launch("l2q_su3_expm_mul2");
}

int l2q_su3_expm_mul2_vec8(const void* xn, const void* vn, double eps, const float* mask_n,
                           int complement_first, void* out, double* vec, int nb, long V,
                           void* stream) {
  L2Q_REQUIRE(xn && vn && out && mask_n && vec, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_field_ok(nb, V), L2Q_EINVAL, "bad size");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL((su3_expm_mul_kernel<true, true>), dim3((unsigned)(nb * 4L * nblk)), dim3(kBlock),
                     0, (hipStream_t)stream, (const double2*)xn, (const double2*)vn, eps, mask_n,
                     complement_first, (double2*)out, vec, (int)V, nblk, 0);
  return check_launch("l2q_su3_expm_mul2_vec8");
}

int l2q_su3_expm_mul2_digits(const void* xn, const void* vn, double eps, const float* mask_n, int complement_first,
                             void* out, void* image, int a_exp, int nb, long V, void* stream) {
  int* flag;
  const int rc = digits_checks("l2q_su3_expm_mul2_digits", xn && vn && out && mask_n && image,
                               su3_field_ok(nb, V) && V % 64 == 0, "the digit image serves V % 64 == 0", a_exp, image, flag);
  if (rc != L2Q_OK) return rc;
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_expm_mul_digits_kernel, dim3((unsigned)(nb * 4L * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, (const double2*)xn, (const double2*)vn, eps, mask_n, complement_first,
                     (double2*)out, (char*)image, (int)V, nblk, 0, ldexp(1.0, GS_BITS - a_exp), ldexp(1.0, a_exp), flag);
  return check_launch("l2q_su3_expm_mul2_digits");
}

int l2q_su3_projsu_digits(const void* in, void* image, int a_exp, long nfields, long V, void* stream) {
  return projsu_digits("l2q_su3_projsu_digits", su3_project_digits_kernel, in, image, a_exp, nfields, V, stream);
}

int l2q_su3_projsu_digits_upper(const void* in, void* image, int a_exp, long nfields, long V, void* stream) {
  return projsu_digits("l2q_su3_projsu_digits_upper", su3_project_digits_upper_kernel, in, image, a_exp, nfields, V,
                       stream);
}

int l2q_su3_pack_digits(const void* x_ref, void* x_nat, void* image, int a_exp, int nb, long V, void* stream) {
  L2Q_REQUIRE(x_ref, L2Q_EINVAL, "null pointer: x_ref");
  L2Q_REQUIRE(x_nat, L2Q_EINVAL, "null pointer: x_nat");
  L2Q_REQUIRE(image, L2Q_EINVAL, "null pointer: image");
  L2Q_REQUIRE(x_ref != x_nat, L2Q_EINVAL, "x_nat must not alias x_ref");
  L2Q_REQUIRE(su3_field_ok(nb, V) && V % 64 == 0, L2Q_EINVAL, "V: the digit image serves V % 64 == 0");
  L2Q_REQUIRE(a_exp > -900 && a_exp < 900, L2Q_EINVAL, "a_exp: bad operand exponent");
  L2Q_REQUIRE((reinterpret_cast<uintptr_t>(x_ref) & 15) == 0, L2Q_ESHAPE, "x_ref must be 16-byte aligned");
  L2Q_REQUIRE((reinterpret_cast<uintptr_t>(x_nat) & 15) == 0, L2Q_ESHAPE, "x_nat must be 16-byte aligned");
  L2Q_REQUIRE((reinterpret_cast<uintptr_t>(image) & 15) == 0, L2Q_ESHAPE, "the image must be 16-byte aligned");
  const long nblk = cdiv(V, kBlock);
  L2Q_REQUIRE(nb * 4L * nblk <= 0x7fffffffL, L2Q_ESHAPE, "nb: grid too large");
  int* flag = gs_flag();
  L2Q_REQUIRE(flag, L2Q_EHIP, "device symbol gs_flag_dev not found");
  hipLaunchKernelGGL(su3_pack_digits_kernel, dim3((unsigned)(nb * 4L * nblk)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const double2*)x_ref, (double2*)x_nat, (char*)image, (int)V, nblk,
                     ldexp(1.0, GS_BITS - a_exp), ldexp(1.0, a_exp), flag);
  return check_launch("l2q_su3_pack_digits");
}

int l2q_su3_project_su(const void* in, void* out, long nfields, long V, void* stream) {
  L2Q_REQUIRE(in && out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_field_ok(nfields, V), L2Q_EINVAL, "bad size");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_project_kernel<0>, dim3((unsigned)(nfields * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, (const double2*)in, (double2*)out, (double*)nullptr, (int)V,
                     nblk);
  return check_launch("l2q_su3_project_su");
}

int l2q_su3_projsu_vec8(const void* in, double* vec, long nfields, long V, void* stream) {
  L2Q_REQUIRE(in && vec, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_field_ok(nfields, V), L2Q_EINVAL, "bad size");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_project_kernel<1>, dim3((unsigned)(nfields * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, (const double2*)in, (double2*)nullptr, vec, (int)V, nblk);
  return check_launch("l2q_su3_projsu_vec8");
}

int l2q_su3_project_tah(const void* in, void* out, long nfields, long V, void* stream) {
  L2Q_REQUIRE(in && out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_field_ok(nfields, V), L2Q_EINVAL, "bad size");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_project_kernel<2>, dim3((unsigned)(nfields * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, (const double2*)in, (double2*)out, (double*)nullptr, (int)V,
                     nblk);
  return check_launch("l2q_su3_project_tah");
}

int l2q_su3_project_u(const void* in, void* out, long nfields, long V, void* stream) {
  L2Q_REQUIRE(in && out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_field_ok(nfields, V), L2Q_EINVAL, "bad size");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_project_kernel<3>, dim3((unsigned)(nfields * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, (const double2*)in, (double2*)out, (double*)nullptr, (int)V,
                     nblk);
  return check_launch("l2q_su3_project_u");
}

int l2q_su3_mul(const void* a, const void* b, int adjoint_a, int adjoint_b, void* out,
                long nfields, long V, void* stream) {
  L2Q_REQUIRE(a && b && out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_field_ok(nfields, V), L2Q_EINVAL, "bad size");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_mul_kernel, dim3((unsigned)(nfields * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, (const double2*)a, (const double2*)b, adjoint_a, adjoint_b,
                     (double2*)out, (int)V, nblk);
  return check_launch("l2q_su3_mul");
}

int l2q_su3_kinetic_reduce(const void* vn, int nb, long V, double* out, void* ws, size_t ws_bytes,
                           void* stream) {
  L2Q_REQUIRE(vn && out && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_field_ok(nb, V), L2Q_EINVAL, "bad size");
  const long n = 36 * V;
  const long nblk = cdiv(n, 4L * kBlock);
  L2Q_REQUIRE(ws_bytes >= (size_t)nb * nblk * sizeof(double), L2Q_ESHAPE, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(su3_norm2_kernel, dim3((unsigned)(nb * nblk)), dim3(kBlock), 0, st,
                     (const double2*)vn, n, nblk, (double*)ws);
  // 0.5 * (sum |p|^2 - 8 * 4V)
  launch_finalize((const double*)ws, out, nb, nblk, 1, 0.5, -0.5 * 8.0 * 4.0 * (double)V, st);
  return check_launch("l2q_su3_kinetic_reduce");
}

int l2q_su3_assemble_tah(const double* normals, void* vn, long nfields, long V, void* stream) {
  L2Q_REQUIRE(normals && vn, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_field_ok(nfields, V), L2Q_EINVAL, "bad size");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_assemble_tah_kernel, dim3((unsigned)(nfields * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, normals, (double2*)vn, V, nblk, nfields * V);
  return check_launch("l2q_su3_assemble_tah");
}

int l2q_su3_assemble_tah_norm2(const double* normals, void* vn, int nb, long V, double* norm2, void* ws,
                               size_t ws_bytes, void* stream) {
  L2Q_REQUIRE(normals && vn && norm2 && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_field_ok(nb, V), L2Q_EINVAL, "bad size");
  const long nblk = cdiv(V, kBlock);
  L2Q_REQUIRE(ws_bytes >= (size_t)nb * 4 * nblk * sizeof(double), L2Q_ESHAPE, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(su3_assemble_tah_norm2_kernel, dim3((unsigned)(nb * 4L * nblk)), dim3(kBlock), 0, st, normals,
                     (double2*)vn, V, nblk, nb * 4L * V, (double*)ws);
  launch_finalize((const double*)ws, norm2, nb, 4 * nblk, 1, 1.0, 0.0, st);
  return check_launch("l2q_su3_assemble_tah_norm2");
}

int l2q_su3_check_su(const void* xn, int nb, long V, double* out, void* ws, size_t ws_bytes,
                     void* stream) {
  L2Q_REQUIRE(xn && out && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_field_ok(nb, V), L2Q_EINVAL, "bad size");
  const long nblk = cdiv(4 * V, kBlock);
  L2Q_REQUIRE(ws_bytes >= (size_t)nb * nblk * 2 * sizeof(double), L2Q_ESHAPE, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  double* psum = (double*)ws;
  double* pmax = psum + (size_t)nb * nblk;
  hipLaunchKernelGGL(su3_check_kernel, dim3((unsigned)(nb * nblk)), dim3(kBlock), 0, st,
                     (const double2*)xn, V, nblk, psum, pmax);
  hipLaunchKernelGGL(check_finalize_kernel, dim3(nb), dim3(kBlock), 0, st, psum, pmax, nblk,
                     4.0 * (double)V, out);
  return check_launch("l2q_su3_check_su");
}

}  // extern "C"
