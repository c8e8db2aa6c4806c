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

// ------------------------------------------------------------------ staple force, LDS tile
// KICK = false: fn[c][mu] = coef * TAH(U A);  KICK = true: vn[c][mu] += coef * TAH(U A)
// A_mu(s) = sum_{nu != mu} [ U_nu(s+mu) U_mu(s+nu)^H U_nu(s)^H
//                           + U_nu(s+mu-nu)^H U_mu(s-nu)^H U_nu(s-nu) ]
// One workgroup = 64 consecutive sites x 4 directions (wavefront w <-> mu = w).  The 4 own
// links of the 64 sites are staged once in LDS ([4][9][64] complex = 36 KiB); every operand
// whose site falls inside the tile (the site itself and, for 8^4 / 16^4 lattices, all +-y,
// +-z neighbours of a (y,z) plane) is then an LDS read instead of a 9 KiB trip to L2.
// For 8^4 that turns 42 of the 76 matrix loads per site into LDS reads (a flat thread-per-link
// kernel is L2-bandwidth-bound: 12 GB of L2->L1 traffic per launch at cfg-4).
struct TileRef {
  const double2* lds;    // [4][9][64]
  int s0;                // first site of the tile
};

// One code path for both sources: a generic (flat) pointer that is either the lane's slot in
// the LDS tile (stride 64) or the global plane (stride V), chosen wave-uniformly.
__device__ __forceinline__ void load_link_tiled(M3& m, const double2* __restrict__ xc,
                                                const TileRef& tr, int rho, int V, int s) {
  const int li = s - tr.s0;
  const bool in = __all((unsigned)li < 64u);
  const double2* base = in ? (tr.lds + rho * 9 * 64 + li) : (xc + rho * 9 * V + s);
  const int stride = in ? 64 : V;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    const double2 dd = base[e * stride];
    m.re[e] = dd.x; m.im[e] = dd.y;
  }
}

template <bool KICK, int OCC>
__global__ __launch_bounds__(kBlock, OCC) void su3_force_tile_kernel(
    const double2* __restrict__ xn, Dims d, long ntile, int swz, double coef,
    double2* __restrict__ out) {
  __shared__ double2 tile[4 * 9 * 64];
  const long w = xcd_swizzle(blockIdx.x, gridDim.x, swz);
  const long c = w / ntile, tb = w % ntile;
  const int mu = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int V = d.V;
  const int s0 = (int)tb * 64;
  const bool live = s0 + lane < V;
  const int s = live ? s0 + lane : V - 1;             // clamp: dead lanes still take part
  const double2* xc = xn + c * 36L * V;
  {
    const double2* g = xc + mu * 9 * V;
#pragma unroll
    for (int e = 0; e < 9; ++e) tile[(mu * 9 + e) * 64 + lane] = g[e * V + s];
  }
  __syncthreads();
  TileRef tr{tile, live ? s0 : -1000000};
  if (!__all(live)) tr.s0 = -1000000;                 // ragged last tile: global path only
  const Site p = site_coords(s, d);
  const int cmu = coord_of(p, mu);
  const int s_pmu = fwd(s, cmu, d, mu);
  M3 acc;
  m3_zero(acc);
#pragma unroll 1
  for (int nu = 0; nu < 4; ++nu) {
    if (nu == mu) continue;
    const int cnu = coord_of(p, nu);
    const int s_pnu = fwd(s, cnu, d, nu);
    const int s_mnu = bwd(s, cnu, d, nu);
    const int s_pmu_mnu = bwd(s_pmu, cnu, d, nu);
    M3 a, b, t;
    // up:   U_nu(s+mu) U_mu(s+nu)^H U_nu(s)^H
    load_link_tiled(a, xc, tr, nu, V, s_pmu);
    load_link_tiled(b, xc, tr, mu, V, s_pnu);
    m3_mul_na(t, a, b);
    load_link_tiled(a, xc, tr, nu, V, s);
    m3_mac_na(acc, t, a);
    // down: U_nu(s+mu-nu)^H U_mu(s-nu)^H U_nu(s-nu)
    load_link_tiled(a, xc, tr, nu, V, s_pmu_mnu);
    load_link_tiled(b, xc, tr, mu, V, s_mnu);
    m3_mul_aa(t, a, b);
    load_link_tiled(a, xc, tr, nu, V, s_mnu);
    m3_mac_nn(acc, t, a);
  }
  M3 u, ua, f;
  load_link_tiled(u, xc, tr, mu, V, s);
  m3_mul_nn(ua, u, acc);
  m3_tah(f, ua);
  if (!live) return;
  double2* o = out + (c * 4 + mu) * 9L * V;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    double2 r = make_double2(coef * f.re[e], coef * f.im[e]);
    if (KICK) {
      const double2 v = o[e * V + s];
      r.x += v.x; r.y += v.y;
    }
    o[e * V + s] = r;
  }
}

// ------------------------------------------------------------------ staple force, slice-resident
// One workgroup = 128 spatial sites x 4 directions (512 threads, wavefront pairs <-> mu),
// sweeping t.  LDS holds TWO time slices of the tile's links (current and next,
// 2 x [4][9][128] complex = 144 KiB); each thread prefetches its own link of the slice after
// next into registers.  The staples that reach back to slice t-1 (the down-staple of a
// spatial link in the t direction, built from slice t-1 links only) are computed one
// iteration early and carried in registers, so slice t-1 is never needed again.
// Per site and sweep the links are read from HBM once (+ the x-halo of the tile); ~17 of the
// 19 operands of a link come from LDS instead of L2 (a flat thread-per-link kernel issues 76 matrix loads
// per site to L2 and leaves the SIMDs idle 53 % of the time waiting for them).
// Register budget decides this kernel.  A workgroup is 64 sites x 4 directions = 4 wavefronts and
// is compiled for ONE wavefront per SIMD (__launch_bounds__(256, 1)): the unified register file
// then gives each wavefront 512 registers, and the ~70 values that do not fit the 256 VGPRs live
// in AGPRs (v_accvgpr moves) instead of scratch memory.  Measured on MI355X at cfg-4:
//   128-site tiles, 2 waves/SIMD (256 registers):  variant 0: 143 spilled VGPRs, 0.97 ms;
//     variant 1: 59 spills, 0.64 ms;  variant 2: 18 spills, 0.56-0.58 ms
//   64-site tiles, 1 wave/SIMD (256 VGPR + 72 AGPR, no scratch):  variant 0: 0.52 ms;
//     variant 1: 0.54 ms;  variant 2: 0.56 ms   (without the scheduling fences: 0.55 ms;
//     staple loops fully unrolled: 512 registers + 660 B scratch)
// 0: carried t-staple + register prefetch of the slice after next   1: no prefetch
// 2: no prefetch, t-staple re-read from slice t-1 through L2
// The plain force runs 128-site tiles with two links per thread at one wavefront per SIMD,
// variant 0 (same-box A/B: 0.51 ms; 64-site one-wave build 0.55 ms; 128-site two-wave variant 2
// 0.59 ms); the fused v += coef F variant (two more HBM streams) keeps the 128-site / two-wave /
// variant-2 build (0.73 ms vs 0.75-0.77 ms for the one-wave builds).
constexpr int kFSPlain = 128, kFSKick = 128, kLptPlain = 2;
// compiler-only fence: keeps hipcc from hoisting the next staple's operand loads above the
// current staple's arithmetic
#define L2Q_SCHED_FENCE() asm volatile("" ::: "memory")

// link rho of spatial site q in a slice: LDS copy if q is inside the tile (wave-uniform),
// else the global slice; one code path through a flat pointer
template <int kFS>
__device__ __forceinline__ void fs_get(M3& m, const double2* slot, const double2* __restrict__ gsl,
                                       int rho, int q, int tile0, int V) {
  const int li = q - tile0;
  const bool in = __all((unsigned)li < (unsigned)kFS);
  const double2* base = in ? (slot + rho * 9 * kFS + li) : (gsl + rho * 9 * V + q);
  const int stride = in ? kFS : V;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    const double2 dd = base[e * stride];
    m.re[e] = dd.x; m.im[e] = dd.y;
  }
}

template <int kFS>
__device__ __forceinline__ void fs_own(M3& m, const double2* slot, int rho, int lt) {
  const double2* l = slot + rho * 9 * kFS + lt;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    const double2 dd = l[e * kFS];
    m.re[e] = dd.x; m.im[e] = dd.y;
  }
}

template <int kFS>
__device__ __forceinline__ void fs_put(double2* slot, int rho, int lt, const M3& m) {
#pragma unroll
  for (int e = 0; e < 9; ++e) slot[(rho * 9 + e) * kFS + lt] = make_double2(m.re[e], m.im[e]);
}

// LPT: links (directions) per thread.  2: a workgroup of 2 kFS threads covers mu = g and g + 2
// one after the other -- the 128-site tile (half the x-halo of the 64-site one) at one wavefront
// per SIMD.
template <bool KICK, int kFS, int VARIANT, int LPT>
__global__ __launch_bounds__(4 * kFS / LPT, (kFS == 64 || LPT == 2) ? 1 : 2) void su3_force_slice_kernel(
    const double2* __restrict__ xn, Dims d, int nsb, int tsplit, int swz, double coef,
    double2* __restrict__ out) {
  extern __shared__ double2 fs_lds[];                   // [2][4][9][kFS]
  constexpr int kSlot = 4 * 9 * kFS;
  const long w = xcd_swizzle(blockIdx.x, gridDim.x, swz);
  const int per_chain = nsb * tsplit;
  const long c = w / per_chain;
  const int r = (int)(w % per_chain);
  const int tc = r / nsb, sb = r % nsb;
  const int Vs = d.X * d.Y * d.Z, V = d.V, T = d.T;
  const int tile0 = sb * kFS;
  const int lt = threadIdx.x & (kFS - 1), g = threadIdx.x / kFS;       // g (hence mu) is wave-uniform
  constexpr int MUSTEP = 4 / LPT;
  const int tlen = (T + tsplit - 1) / tsplit;
  const int t0 = tc * tlen, t1 = min(T, t0 + tlen);
  const double2* xc = xn + c * 36L * V;
  SPos p;
  p.q = tile0 + lt;
  {
    int q = p.q;
    p.z = q % d.Z; q /= d.Z;
    p.y = q % d.Y; q /= d.Y;
    p.x = q;
  }
  const int sp = p.q;
  // prologue: slices t0-1 and t0 of the tile -> slots 0, 1 (each thread its own link)
  {
    const int ta = (t0 - 1 + T) % T;
#pragma unroll 1
    for (int k = 0; k < 2 * LPT; ++k) {
      const int sl = (ta + (k & 1)) % T, mu = g + MUSTEP * (k >> 1);
      M3 tmp;
      load_link(tmp, xc + mu * 9 * V, V, sl * Vs + sp);
      fs_put<kFS>(fs_lds + (k & 1) * kSlot, mu, lt, tmp);
    }
  }
  __syncthreads();
  int slot_cur = 0;
  M3 dcarry_[LPT], pre_[LPT];
#pragma unroll
  for (int h = 0; h < LPT; ++h) m3_zero(dcarry_[h]);
  const int niter = (t1 - t0) + 1;
#pragma unroll 1
  for (int it = 0; it < niter; ++it) {
    const int tcur = (t0 - 1 + it + T) % T;
    const int tnext = (tcur + 1) % T;
    const double2* cur = fs_lds + slot_cur * kSlot;
    const double2* nxt = fs_lds + (slot_cur ^ 1) * kSlot;
    const double2* gcur = xc + (long)tcur * Vs;
    const double2* gnxt = xc + (long)tnext * Vs;
    const bool more = it + 1 < niter;
#pragma unroll
    for (int h = 0; h < LPT; ++h) {
    const int mu = g + MUSTEP * h;
    double2* oc = out + (c * 4 + mu) * 9L * V;
    SPos pmu = p;
    if (mu != 0) pmu = sp_move(p, mu, +1, d);
    if (it > 0) {
      M3 acc;
      if (mu == 0) {
        m3_zero(acc);
#pragma unroll 1
        for (int nu = 1; nu < 4; ++nu) {
          const SPos pp = sp_move(p, nu, +1, d), pm = sp_move(p, nu, -1, d);
          M3 a, b, t;
          // up:   U_nu(s+t) U_t(s+nu)^H U_nu(s)^H
          fs_own<kFS>(a, nxt, nu, lt);
          fs_get<kFS>(b, cur, gcur, 0, pp.q, tile0, V);
          m3_mul_na(t, a, b);
          fs_own<kFS>(a, cur, nu, lt);
          m3_mac_na(acc, t, a);
          L2Q_SCHED_FENCE();
          // down: U_nu(s+t-nu)^H U_t(s-nu)^H U_nu(s-nu)
          fs_get<kFS>(a, nxt, gnxt, nu, pm.q, tile0, V);
          fs_get<kFS>(b, cur, gcur, 0, pm.q, tile0, V);
          m3_mul_aa(t, a, b);
          fs_get<kFS>(a, cur, gcur, nu, pm.q, tile0, V);
          m3_mac_nn(acc, t, a);
          L2Q_SCHED_FENCE();
        }
      } else {
        if constexpr (VARIANT != 2) {
          acc = dcarry_[h];                                // down staple in the t direction
        } else {                                       // t-direction down staple from slice t-1 (L2)
          const double2* gprv = xc + (long)((tcur - 1 + T) % T) * Vs;
          M3 a, b, t;
          load_link(a, gprv, V, pmu.q);
          load_link(b, gprv + mu * 9 * V, V, sp);
          m3_mul_aa(t, a, b);
          load_link(a, gprv, V, sp);
          m3_mul_nn(acc, t, a);
          L2Q_SCHED_FENCE();
        }
        {
          M3 a, b, t;
          // up (nu = t): U_t(s+mu) U_mu(s+t)^H U_t(s)^H
          fs_get<kFS>(a, cur, gcur, 0, pmu.q, tile0, V);
          fs_own<kFS>(b, nxt, mu, lt);
          m3_mul_na(t, a, b);
          fs_own<kFS>(a, cur, 0, lt);
          m3_mac_na(acc, t, a);
          L2Q_SCHED_FENCE();
        }
#pragma unroll 1
        for (int nu = 1; nu < 4; ++nu) {
          if (nu == mu) continue;
          const SPos pp = sp_move(p, nu, +1, d), pm = sp_move(p, nu, -1, d);
          const SPos pmm = sp_move(pmu, nu, -1, d);
          M3 a, b, t;
          // up:   U_nu(s+mu) U_mu(s+nu)^H U_nu(s)^H
          fs_get<kFS>(a, cur, gcur, nu, pmu.q, tile0, V);
          fs_get<kFS>(b, cur, gcur, mu, pp.q, tile0, V);
          m3_mul_na(t, a, b);
          fs_own<kFS>(a, cur, nu, lt);
          m3_mac_na(acc, t, a);
          L2Q_SCHED_FENCE();
          // down: U_nu(s+mu-nu)^H U_mu(s-nu)^H U_nu(s-nu)
          fs_get<kFS>(a, cur, gcur, nu, pmm.q, tile0, V);
          fs_get<kFS>(b, cur, gcur, mu, pm.q, tile0, V);
          m3_mul_aa(t, a, b);
          fs_get<kFS>(a, cur, gcur, nu, pm.q, tile0, V);
          m3_mac_nn(acc, t, a);
          L2Q_SCHED_FENCE();
        }
      }
      M3 u, ua, f;
      fs_own<kFS>(u, cur, mu, lt);
      m3_mul_nn(ua, u, acc);
      m3_tah(f, ua);
      const int s = tcur * Vs + sp;
#pragma unroll
      for (int e = 0; e < 9; ++e) {
        double2 rr = make_double2(coef * f.re[e], coef * f.im[e]);
        if (KICK) {
          const double2 v = oc[e * V + s];
          rr.x += v.x; rr.y += v.y;
        }
        oc[e * V + s] = rr;
      }
      L2Q_SCHED_FENCE();
    }
    // prefetch this thread's link of the slice after next (hidden behind the carry staple,
    // the barrier and the partner wavefront's work)
    if constexpr (VARIANT == 0) {
      if (more) load_link(pre_[h], xc + mu * 9 * V, V, ((tnext + 1) % T) * Vs + sp);
    }
    if (VARIANT != 2 && mu != 0 && more) {
      // next iteration's t-direction down staple of link (tnext, sp, mu), all from slice tcur:
      //   U_t(tcur, sp+mu)^H U_mu(tcur, sp)^H U_t(tcur, sp)
      M3 a, b, t;
      fs_get<kFS>(a, cur, gcur, 0, pmu.q, tile0, V);
      fs_own<kFS>(b, cur, mu, lt);
      m3_mul_aa(t, a, b);
      fs_own<kFS>(a, cur, 0, lt);
      m3_mul_nn(dcarry_[h], t, a);
    }
    }
    __syncthreads();                                    // slice tcur fully consumed
    if (more) {
#pragma unroll
      for (int h = 0; h < LPT; ++h) {
        const int mu = g + MUSTEP * h;
        if constexpr (VARIANT != 0) load_link(pre_[h], xc + mu * 9 * V, V, ((tnext + 1) % T) * Vs + sp);
        fs_put<kFS>(fs_lds + slot_cur * kSlot, mu, lt, pre_[h]);
      }
    }
    slot_cur ^= 1;
    __syncthreads();
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

// out[c] = sums[c][0]: the real part of the (Re, Im) pairs l2q_su3_plaq_reduce writes
__global__ void su3_plaq_re_kernel(const double* __restrict__ sums, double* __restrict__ out, int nb) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < nb) out[c] = sums[2 * c];
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

// The slice-resident and LDS-tiled instantiations launch_force<KICK> runs; force_kernel_name prints the same constants.
template <bool KICK>
struct ForceInst {
  static constexpr int kFS = KICK ? kFSKick : kFSPlain, kVar = KICK ? 2 : 0, kLpt = KICK ? 1 : kLptPlain, kTileOcc = 2;
};

namespace l2q {
ForceKernel pick_force(const Dims& d, bool kick) {
  const int ft = tuning().force_tile;
  if (!kick && ft == 7 && force_plaq_applicable(d)) return ForceKernel::PlaqShare;
  if (ft >= 5 && force_link_applicable(d)) return ForceKernel::Link;
  return (d.X * d.Y * d.Z) % (kick ? kFSKick : kFSPlain) == 0 ? ForceKernel::Slice : ForceKernel::Tile;
}
}  // namespace l2q

template <bool KICK>
static void launch_force(const double2* xn, Dims d, int nb, double coef, double2* out, hipStream_t st) {
  using I = ForceInst<KICK>;
  switch (pick_force(d, KICK)) {
    case ForceKernel::PlaqShare: launch_force_plaq(xn, d, nb, coef, out, st); return;
    case ForceKernel::Link: launch_force_link(KICK, xn, d, nb, coef, out, st); return;
    case ForceKernel::Slice: {
      const int nsb = d.X * d.Y * d.Z / I::kFS;
      const int tsplit = t_chunks((long)nb * nsb, d.T, 512);       // >= ~2 resident rounds of 256 CUs
      const size_t lds = 2ul * 4 * 9 * I::kFS * sizeof(double2);
      static PerDeviceOnce attr_once;
      if (attr_once.first()) {
        (void)hipFuncSetAttribute((const void*)su3_force_slice_kernel<KICK, I::kFS, I::kVar, I::kLpt>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      }
      hipLaunchKernelGGL((su3_force_slice_kernel<KICK, I::kFS, I::kVar, I::kLpt>),
                         dim3((unsigned)((long)nb * nsb * tsplit)), dim3(4 * I::kFS / I::kLpt), lds, st, xn, d, nsb,
                         tsplit, tuning().xcd_swizzle, coef, out);
      return;
    }
    case ForceKernel::Tile: {
      const long ntile = cdiv(d.V, 64);
      hipLaunchKernelGGL((su3_force_tile_kernel<KICK, I::kTileOcc>), dim3((unsigned)(nb * ntile)), dim3(kBlock), 0,
                         st, xn, d, ntile, tuning().xcd_swizzle, coef, out);
    }
  }
}

template <bool KICK>
static void force_kernel_name(const Dims& d, char* buf, size_t n) {
  using I = ForceInst<KICK>;
  const char* k = KICK ? "true" : "false";
  switch (pick_force(d, KICK)) {
    case ForceKernel::PlaqShare: snprintf(buf, n, "su3_force_plaq_kernel"); break;
    case ForceKernel::Link: snprintf(buf, n, "su3_force_link_kernel<%d, %d>", KICK, force_link_inmask(d)); break;
    case ForceKernel::Slice:
      snprintf(buf, n, "su3_force_slice_kernel<%s, %d, %d, %d>", k, I::kFS, I::kVar, I::kLpt);
      break;
    case ForceKernel::Tile: snprintf(buf, n, "su3_force_tile_kernel<%s, %d>", k, I::kTileOcc);
  }
}

// The upper-plane force (l2q_su3_force_upper, l2q_su3_force_action_upper) is an output form of the thread-per-link
// kernel alone: where the ladder picks another kernel the entries refuse and the caller keeps the full field.
static bool force_upper_applicable(const Dims& d) { return pick_force(d, false) == ForceKernel::Link; }

// The plaquette sum: the slice-resident kernel where the spatial volume is whole tiles -- <true> where the tile is
// whole (y, z) planes (Y*Z | 128), which keeps +y, +z inside it -- else the flat kernel.
enum class PlaqKernel { SliceYZ, Slice, Flat };
constexpr int kPlaqOcc = 2;
static PlaqKernel pick_plaq(const Dims& d) {
  if ((d.X * d.Y * d.Z) % kSlice != 0) return PlaqKernel::Flat;
  return kSlice % (d.Y * d.Z) == 0 ? PlaqKernel::SliceYZ : PlaqKernel::Slice;
}

extern "C" {

int l2q_kernel_name(const char* entry, int T, int X, int Y, int Z, char* buf, size_t buf_bytes) {
  L2Q_REQUIRE(entry && buf && buf_bytes > 0, L2Q_EINVAL, "null pointer");
  const Dims dd = strncmp(entry, "l2q_su3_", 8) ? Dims{} : make_dims(T, X, Y, Z);   // (other entries: not a lattice)
  buf[0] = 0;
  if (!strcmp(entry, "l2q_su3_plaq_reduce")) {
    const PlaqKernel pk = pick_plaq(dd);
    if (pk == PlaqKernel::Flat) snprintf(buf, buf_bytes, "su3_plaq_kernel<%d>", kPlaqOcc);
    else snprintf(buf, buf_bytes, "su3_plaq_slice_kernel<%s>", pk == PlaqKernel::SliceYZ ? "true" : "false");
  } else if (!strcmp(entry, "l2q_su3_force")) {
    force_kernel_name<false>(dd, buf, buf_bytes);
  } else if (!strcmp(entry, "l2q_su3_force_kick")) {
    force_kernel_name<true>(dd, buf, buf_bytes);
  } else if (!strcmp(entry, "l2q_su3_force_action")) {
    if (pick_force(dd, false) == ForceKernel::Link) {
      snprintf(buf, buf_bytes, "su3_force_link_action_kernel<%d>", force_link_inmask(dd));
    } else {                          // the ordinary force, then the plaquette reduction
      char force[128], plaq[128];
      force_kernel_name<false>(dd, force, sizeof(force));
      (void)l2q_kernel_name("l2q_su3_plaq_reduce", T, X, Y, Z, plaq, sizeof(plaq));
      snprintf(buf, buf_bytes, "%s + %s", force, plaq);
    }
  } else if (!strcmp(entry, "l2q_su3_force_upper") || !strcmp(entry, "l2q_su3_force_action_upper")) {
    // (the thread-per-link kernel only; "": the entry refuses this lattice / force_tile)
    if (force_upper_applicable(dd)) {
      if (entry[14] == 'u') snprintf(buf, buf_bytes, "su3_force_link_kernel<4, %d>", force_link_inmask(dd));
      else snprintf(buf, buf_bytes, "su3_force_link_action_upper_kernel<%d>", force_link_inmask(dd));
    }
  } else if (!strcmp(entry, "l2q_su3_projsu_digits_upper")) {
    snprintf(buf, buf_bytes, "su3_project_digits_upper_kernel");
  } else if (!strcmp(entry, "l2q_su3_clover_reduce")) {
    snprintf(buf, buf_bytes, "%s", clover_slice_applicable(dd) ? "su3_clover_slice_kernel" : "su3_clover_kernel");
  } else if (!strcmp(entry, "l2q_su3_flow_stage")) {
    // the kick of l2q_su3_force_kick_to (out of place: only the thread-per-link kernel has that form, the others
    // follow a copy), then the unmasked x-update
    char kick[128];
    force_kernel_name<true>(dd, kick, sizeof(kick));
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
    const int nsb = X * Y * Z / kSlice;
    const int tsplit = t_chunks((long)nb * nsb, T, 1024);      // keep >= ~1024 workgroups
    const long per_chain = (long)nsb * tsplit;
    L2Q_REQUIRE(ws_bytes >= (size_t)nb * per_chain * 2 * sizeof(double), L2Q_ESHAPE, "workspace too small");
    if (pk == PlaqKernel::SliceYZ)
      hipLaunchKernelGGL(su3_plaq_slice_kernel<true>, dim3((unsigned)(nb * per_chain)), dim3(kSlice), 0, st,
                         (const double2*)xn, d, nsb, tsplit, swz, partial);
    else hipLaunchKernelGGL(su3_plaq_slice_kernel<false>, dim3((unsigned)(nb * per_chain)), dim3(kSlice), 0, st,
                            (const double2*)xn, d, nsb, tsplit, swz, partial);
    launch_finalize(partial, out, nb, per_chain, 2, 1.0, 0.0, st);
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

int l2q_su3_force(const void* xn, double beta, void* fn, int nb, int T, int X, int Y, int Z,
                  void* stream) {
  L2Q_REQUIRE(xn && fn, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(xn != fn, L2Q_EINVAL, "force output must not alias the gauge field");
  const Dims d = make_dims(T, X, Y, Z);
  launch_force<false>((const double2*)xn, d, nb, beta / 3.0, (double2*)fn, (hipStream_t)stream);
  return check_launch("l2q_su3_force");
}

size_t l2q_su3_force_action_ws_bytes(int nb, int T, int X, int Y, int Z) {
  if (!su3_dims_ok(nb, T, X, Y, Z)) return 0;
  // the link kernel's one partial per workgroup (at most V / 64 per chain), or, on the other route, the
  // plaquette reduction's (Re, Im) result in the first 256-byte multiple and its own workspace behind it
  return (((size_t)nb * 2 * sizeof(double) + 255) & ~(size_t)255) + l2q_reduce_ws_bytes(nb, 36L * T * X * Y * Z);
}

int l2q_su3_force_action(const void* xn, double beta, void* fn, double* plaq, int nb, int T, int X, int Y, int Z,
                         void* ws, size_t ws_bytes, void* stream) {
  L2Q_REQUIRE(xn && fn && plaq && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(xn != fn, L2Q_EINVAL, "force output must not alias the gauge field");
  L2Q_REQUIRE(ws_bytes >= l2q_su3_force_action_ws_bytes(nb, T, X, Y, Z), L2Q_ESHAPE, "workspace too small");
  const Dims d = make_dims(T, X, Y, Z);
  hipStream_t st = (hipStream_t)stream;
  if (pick_force(d, false) == ForceKernel::Link) {
    // sum over links of Re tr(U A) counts every plaquette once per link of it
    const long parts = force_link_action_parts(d, nb);
    launch_force_link_action((const double2*)xn, d, nb, beta / 3.0, (double2*)fn, (double*)ws, st);
    launch_finalize((const double*)ws, plaq, nb, parts, 1, 0.25, 0.0, st);
    return check_launch("l2q_su3_force_action");
  }
  // lattices (and force_tile settings) the link kernel does not serve: the two passes
  launch_force<false>((const double2*)xn, d, nb, beta / 3.0, (double2*)fn, st);
  const size_t head = ((size_t)nb * 2 * sizeof(double) + 255) & ~(size_t)255;
  const int rc = l2q_su3_plaq_reduce(xn, nb, T, X, Y, Z, (double*)ws, (char*)ws + head, ws_bytes - head, stream);
  if (rc != L2Q_OK) return rc;
  hipLaunchKernelGGL(su3_plaq_re_kernel, dim3((unsigned)cdiv(nb, kBlock)), dim3(kBlock), 0, st, (const double*)ws,
                     plaq, nb);
  return check_launch("l2q_su3_force_action");
}

int l2q_su3_force_upper(const void* xn, double beta, void* fu, int nb, int T, int X, int Y, int Z, void* stream) {
  L2Q_REQUIRE(xn && fu, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(xn != fu, L2Q_EINVAL, "force output must not alias the gauge field");
  const Dims d = make_dims(T, X, Y, Z);
  L2Q_REQUIRE(force_upper_applicable(d), L2Q_ESHAPE,
              "the upper-plane force is the thread-per-link kernel's: not on this lattice / force_tile");
  launch_force_link_upper((const double2*)xn, d, nb, beta / 3.0, (double2*)fu, (hipStream_t)stream);
  return check_launch("l2q_su3_force_upper");
}

int l2q_su3_force_action_upper(const void* xn, double beta, void* fu, double* plaq, int nb, int T, int X, int Y,
                               int Z, void* ws, size_t ws_bytes, void* stream) {
  L2Q_REQUIRE(xn && fu && plaq && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(xn != fu, L2Q_EINVAL, "force output must not alias the gauge field");
  L2Q_REQUIRE(ws_bytes >= l2q_su3_force_action_ws_bytes(nb, T, X, Y, Z), L2Q_ESHAPE, "workspace too small");
  const Dims d = make_dims(T, X, Y, Z);
  L2Q_REQUIRE(force_upper_applicable(d), L2Q_ESHAPE,
              "the upper-plane force is the thread-per-link kernel's: not on this lattice / force_tile");
  hipStream_t st = (hipStream_t)stream;
  launch_force_link_action((const double2*)xn, d, nb, beta / 3.0, (double2*)fu, (double*)ws, st, true);
  launch_finalize((const double*)ws, plaq, nb, force_link_action_parts(d, nb), 1, 0.25, 0.0, st);
  return check_launch("l2q_su3_force_action_upper");
}

int l2q_su3_force_kick(const void* xn, double beta, double coef, void* vn, int nb, int T, int X,
                       int Y, int Z, void* stream) {
  L2Q_REQUIRE(xn && vn, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  const Dims d = make_dims(T, X, Y, Z);
  launch_force<true>((const double2*)xn, d, nb, coef * beta / 3.0, (double2*)vn, (hipStream_t)stream);
  return check_launch("l2q_su3_force_kick");
}

int l2q_su3_force_kick_to(const void* xn, double beta, double coef, const void* v_in, void* v_out,
                          int nb, int T, int X, int Y, int Z, void* stream) {
  L2Q_REQUIRE(xn && v_in && v_out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  const Dims d = make_dims(T, X, Y, Z);
  hipStream_t st = (hipStream_t)stream;
  if (v_in != v_out && force_link_runs(d)) {
    launch_force_link(true, (const double2*)xn, d, nb, coef * beta / 3.0, (double2*)v_out, st,
                      (const double2*)v_in);
    return check_launch("l2q_su3_force_kick_to");
  }
  // the other kernels of the family update in place: copy first
  if (v_in != v_out)
    (void)hipMemcpyAsync(v_out, v_in, (size_t)nb * 36 * d.V * sizeof(double2), hipMemcpyDeviceToDevice, st);
  return l2q_su3_force_kick(xn, beta, coef, v_out, nb, T, X, Y, Z, stream);
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
  L2Q_REQUIRE(xn && vn && out && mask_n && image, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_field_ok(nb, V) && V % 64 == 0, L2Q_EINVAL, "the digit image serves V % 64 == 0");
  L2Q_REQUIRE(a_exp > -900 && a_exp < 900, L2Q_EINVAL, "bad operand exponent");
  L2Q_REQUIRE((reinterpret_cast<uintptr_t>(image) & 15) == 0, L2Q_ESHAPE, "the image must be 16-byte aligned");
  int* flag = gs_flag();
  L2Q_REQUIRE(flag, L2Q_EHIP, "device symbol gs_flag_dev not found");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_expm_mul_digits_kernel, dim3((unsigned)(nb * 4L * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, (const double2*)xn, (const double2*)vn, eps, mask_n, complement_first,
                     (double2*)out, (char*)image, (int)V, nblk, 0, ldexp(1.0, GS_BITS - a_exp), ldexp(1.0, a_exp), flag);
  return check_launch("l2q_su3_expm_mul2_digits");
}

int l2q_su3_projsu_digits(const void* in, void* image, int a_exp, long nfields, long V, void* stream) {
  L2Q_REQUIRE(in && image, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_field_ok(nfields, V) && V % 64 == 0 && nfields % 4 == 0, L2Q_EINVAL,
              "the digit image serves whole chains (4 fields each) with V % 64 == 0");
  L2Q_REQUIRE(a_exp > -900 && a_exp < 900, L2Q_EINVAL, "bad operand exponent");
  L2Q_REQUIRE((reinterpret_cast<uintptr_t>(image) & 15) == 0, L2Q_ESHAPE, "the image must be 16-byte aligned");
  int* flag = gs_flag();
  L2Q_REQUIRE(flag, L2Q_EHIP, "device symbol gs_flag_dev not found");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_project_digits_kernel, dim3((unsigned)(nfields * nblk)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const double2*)in, (char*)image, (int)V, nblk, ldexp(1.0, GS_BITS - a_exp), ldexp(1.0, a_exp),
                     flag);
  return check_launch("l2q_su3_projsu_digits");
}

int l2q_su3_projsu_digits_upper(const void* in, void* image, int a_exp, long nfields, long V, void* stream) {
  L2Q_REQUIRE(in && image, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_field_ok(nfields, V) && V % 64 == 0 && nfields % 4 == 0, L2Q_EINVAL,
              "the digit image serves whole chains (4 fields each) with V % 64 == 0");
  L2Q_REQUIRE(a_exp > -900 && a_exp < 900, L2Q_EINVAL, "bad operand exponent");
  L2Q_REQUIRE((reinterpret_cast<uintptr_t>(image) & 15) == 0, L2Q_ESHAPE, "the image must be 16-byte aligned");
  int* flag = gs_flag();
  L2Q_REQUIRE(flag, L2Q_EHIP, "device symbol gs_flag_dev not found");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_project_digits_upper_kernel, dim3((unsigned)(nfields * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, (const double2*)in, (char*)image, (int)V, nblk,
                     ldexp(1.0, GS_BITS - a_exp), ldexp(1.0, a_exp), flag);
  return check_launch("l2q_su3_projsu_digits_upper");
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
