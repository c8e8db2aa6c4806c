// su3_links.hpp -- link addressing in the native layout xn[chain][mu][e][site] and periodic
// neighbour arithmetic, shared by the SU(3) forward and training kernels.
#pragma once
#include "l2q_common.hpp"
#include "su3_math.hpp"

namespace l2q {

struct Dims {
  int T, X, Y, Z;
  int V;          // sites per chain (36 V complex entries per chain must fit an int)
};

__device__ __forceinline__ void load_link(M3& m, const double2* __restrict__ f, int V, int s) {
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    const double2 d = f[e * V + s];
    m.re[e] = d.x; m.im[e] = d.y;
  }
}

// U^H of the link at site s
__device__ __forceinline__ void load_link_adj(M3& m, const double2* __restrict__ f, int V, int s) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double2 d = f[(3 * j + i) * V + s];
      m.re[3 * i + j] = d.x; m.im[3 * i + j] = -d.y;
    }
}

// Site index that exists only once `dep` does: the loads it addresses cannot be issued before the product that made
// dep (the thread-per-link gathers of su3_clover_bwd.hip and su3_flow_bwd.hip keep one operand in flight this way).
__device__ __forceinline__ int site_after(int site, double dep) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(site) : "v"(dep));
#endif
  return site;
}

__device__ __forceinline__ void store_link(double2* __restrict__ f, int V, int s, const M3& m) {
#pragma unroll
  for (int e = 0; e < 9; ++e) f[e * V + s] = make_double2(m.re[e], m.im[e]);
}

struct Site {
  int t, x, y, z;
};

__device__ __forceinline__ Site site_coords(int s, const Dims& d) {
  Site r;
  r.z = s % d.Z; s /= d.Z;
  r.y = s % d.Y; s /= d.Y;
  r.x = s % d.X; s /= d.X;
  r.t = s;
  return r;
}

// mu is wave-uniform everywhere below (loop counters / blockIdx), so these selects are
// scalar and nothing is indexed dynamically in VGPR arrays.
__device__ __forceinline__ int coord_of(const Site& p, int mu) {
  return mu == 0 ? p.t : mu == 1 ? p.x : mu == 2 ? p.y : p.z;
}
__device__ __forceinline__ int stride_of(const Dims& d, int mu) {
  return mu == 0 ? d.X * d.Y * d.Z : mu == 1 ? d.Y * d.Z : mu == 2 ? d.Z : 1;
}
__device__ __forceinline__ int extent_of(const Dims& d, int mu) {
  return mu == 0 ? d.T : mu == 1 ? d.X : mu == 2 ? d.Y : d.Z;
}
// site index of the periodic forward / backward neighbour of s (coordinate cm in direction mu)
__device__ __forceinline__ int fwd(int s, int cm, const Dims& d, int mu) {
  const int st = stride_of(d, mu), n = extent_of(d, mu);
  return (cm + 1 == n) ? s - (n - 1) * st : s + st;
}
__device__ __forceinline__ int bwd(int s, int cm, const Dims& d, int mu) {
  const int st = stride_of(d, mu), n = extent_of(d, mu);
  return (cm == 0) ? s + (n - 1) * st : s - st;
}

// The flat site kernels keep no coordinates (a Site indexed by a loop-variant direction is copied to scratch): the
// coordinate comes by division.  Periodic neighbour of site s in a direction of stride st and extent ext; dir = +1 / -1
__device__ __forceinline__ int site_hop(int s, int st, int ext, int dir) {
  const int c = (s / st) % ext;
  if (dir > 0) return c + 1 == ext ? s - (ext - 1) * st : s + st;
  return c == 0 ? s + (ext - 1) * st : s - st;
}
// ... and site s moved n steps forward, 0 <= n < ext
__device__ __forceinline__ int site_shifted(int s, int st, int ext, int n) {
  const int c = (s / st) % ext;
  int c2 = c + n;
  if (c2 >= ext) c2 -= ext;
  return s + (c2 - c) * st;
}

// the slice-resident kernels sweep t and keep a thread's place inside a time slice
struct SPos {
  int q, x, y, z;        // spatial site index and coordinates
};

// one periodic hop in spatial direction dir (1, 2, 3 = x, y, z); dir and sgn are wave-uniform
__device__ __forceinline__ SPos sp_move(SPos p, int dir, int sgn, const Dims& d) {
  const int n = dir == 1 ? d.X : dir == 2 ? d.Y : d.Z;
  const int st = dir == 1 ? d.Y * d.Z : dir == 2 ? d.Z : 1;
  int c = dir == 1 ? p.x : dir == 2 ? p.y : p.z;
  if (sgn > 0) {
    if (c + 1 == n) { p.q -= (n - 1) * st; c = 0; } else { p.q += st; c += 1; }
  } else {
    if (c == 0) { p.q += (n - 1) * st; c = n - 1; } else { p.q -= st; c -= 1; }
  }
  if (dir == 1) p.x = c; else if (dir == 2) p.y = c; else p.z = c;
  return p;
}

}  // namespace l2q
