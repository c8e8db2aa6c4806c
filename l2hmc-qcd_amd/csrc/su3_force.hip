// su3_force.hip -- the SU(3) staple force: the LDS-tiled and the slice-resident kernel, the ladder that chooses
// between them and the kernels of su3_force_plaq.hip and su3_force_link.hip (pick_force), and the force entry points
// of the C ABI (gfx950).
#include "su3_launch.hpp"

namespace l2q {

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

// out[c] = sums[c][0]: the real part of the (Re, Im) pairs l2q_su3_plaq_reduce writes
__global__ void su3_plaq_re_kernel(const double* __restrict__ sums, double* __restrict__ out, int nb) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < nb) out[c] = sums[2 * c];
}

// ------------------------------------------------------------------ host side: the ladder and its names
// The slice-resident and LDS-tiled instantiations launch_force<KICK> runs; force_kernel_name prints the same constants.
template <bool KICK>
struct ForceInst {
  static constexpr int kFS = KICK ? kFSKick : kFSPlain, kVar = KICK ? 2 : 0, kLpt = KICK ? 1 : kLptPlain, kTileOcc = 2;
};

void set_dynamic_lds(const void* kern, size_t bytes) {
  (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

ForceKernel pick_force(const Dims& d, bool kick) {
  const int ft = tuning().force_tile;
  if (!kick && ft == 7 && force_plaq_applicable(d)) return ForceKernel::PlaqShare;
  if (ft >= 5 && force_link_applicable(d)) return ForceKernel::Link;
  return (d.X * d.Y * d.Z) % (kick ? kFSKick : kFSPlain) == 0 ? ForceKernel::Slice : ForceKernel::Tile;
}

template <bool KICK>
static void launch_force(const double2* xn, Dims d, int nb, double coef, double2* out, hipStream_t st) {
  using I = ForceInst<KICK>;
  switch (pick_force(d, KICK)) {
    case ForceKernel::PlaqShare: launch_force_plaq(xn, d, nb, coef, out, st); return;
    case ForceKernel::Link:
      launch_force_link(KICK ? LinkForm::Kick : LinkForm::Force, xn, d, nb, coef, nullptr, out, nullptr, st);
      return;
    case ForceKernel::Slice: {
      constexpr auto kern = su3_force_slice_kernel<KICK, I::kFS, I::kVar, I::kLpt>;
      const SliceGrid g = slice_grid(d, nb, I::kFS, 512);          // >= ~2 resident rounds of 256 CUs
      const size_t lds = 2ul * 4 * 9 * I::kFS * sizeof(double2);
      dynamic_lds_once<kern>(lds);
      hipLaunchKernelGGL(kern, dim3((unsigned)g.blocks), dim3(4 * I::kFS / I::kLpt), lds, st, xn, d, g.nsb, g.tsplit,
                         tuning().xcd_swizzle, coef, out);
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

bool force_entry_kernel_name(const char* entry, const Dims& d, char* buf, size_t n) {
  const auto is = [entry](const char* name) { return !strcmp(entry, name); };
  if (is("l2q_su3_force")) {
    force_kernel_name<false>(d, buf, n);
  } else if (is("l2q_su3_force_kick")) {
    force_kernel_name<true>(d, buf, n);
  } else if (is("l2q_su3_force_action")) {
    if (pick_force(d, false) == ForceKernel::Link) {
      snprintf(buf, n, "su3_force_link_action_kernel<%d>", force_link_inmask(d));
    } else {                          // the ordinary force, then the plaquette reduction
      char force[128], plaq[128];
      force_kernel_name<false>(d, force, sizeof(force));
      (void)l2q_kernel_name("l2q_su3_plaq_reduce", d.T, d.X, d.Y, d.Z, plaq, sizeof(plaq));
      snprintf(buf, n, "%s + %s", force, plaq);
    }
  } else if (is("l2q_su3_force_upper")) {        // ("": the entry refuses this lattice / force_tile)
    if (force_upper_applicable(d))
      snprintf(buf, n, "su3_force_link_kernel<%d, %d>", (int)LinkForm::Upper, force_link_inmask(d));
  } else if (is("l2q_su3_force_action_upper")) {
    if (force_upper_applicable(d)) snprintf(buf, n, "su3_force_link_action_upper_kernel<%d>", force_link_inmask(d));
  } else {
    return false;
  }
  return true;
}

}  // namespace l2q

using namespace l2q;

// l2q_su3_force and, with `upper`, l2q_su3_force_upper
static int force_entry(const char* what, bool upper, const void* xn, double beta, void* fn, int nb, int T, int X, int Y,
                       int Z, void* stream) {
  L2Q_REQUIRE_W(xn && fn, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE_W(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE_W(xn != fn, L2Q_EINVAL, "force output must not alias the gauge field");
  const Dims d = make_dims(T, X, Y, Z);
  hipStream_t st = (hipStream_t)stream;
  if (upper) {
    L2Q_REQUIRE_W(force_upper_applicable(d), L2Q_ESHAPE,
                  "the upper-plane force is the thread-per-link kernel's: not on this lattice / force_tile");
    launch_force_link(LinkForm::Upper, (const double2*)xn, d, nb, beta / 3.0, nullptr, (double2*)fn, nullptr, st);
  } else {
    launch_force<false>((const double2*)xn, d, nb, beta / 3.0, (double2*)fn, st);
  }
  return check_launch(what);
}

// l2q_su3_force_action and, with `upper`, l2q_su3_force_action_upper
static int force_action_entry(const char* what, bool upper, const void* xn, double beta, void* fn, double* plaq, int nb,
                              int T, int X, int Y, int Z, void* ws, size_t ws_bytes, void* stream) {
  L2Q_REQUIRE_W(xn && fn && plaq && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE_W(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE_W(xn != fn, L2Q_EINVAL, "force output must not alias the gauge field");
  L2Q_REQUIRE_W(ws_bytes >= l2q_su3_force_action_ws_bytes(nb, T, X, Y, Z), L2Q_ESHAPE, "workspace too small");
  const Dims d = make_dims(T, X, Y, Z);
  L2Q_REQUIRE_W(!upper || force_upper_applicable(d), L2Q_ESHAPE,
                "the upper-plane force is the thread-per-link kernel's: not on this lattice / force_tile");
  hipStream_t st = (hipStream_t)stream;
  if (pick_force(d, false) == ForceKernel::Link) {
    // sum over links of Re tr(U A) counts every plaquette once per link of it
    launch_force_link(upper ? LinkForm::UpperAction : LinkForm::ForceAction, (const double2*)xn, d, nb, beta / 3.0,
                      nullptr, (double2*)fn, (double*)ws, st);
    launch_finalize((const double*)ws, plaq, nb, force_link_action_parts(d, nb), 1, 0.25, 0.0, st);
    return check_launch(what);
  }
  // lattices (and force_tile settings) the link kernel does not serve: the two passes
  launch_force<false>((const double2*)xn, d, nb, beta / 3.0, (double2*)fn, st);
  const size_t head = ((size_t)nb * 2 * sizeof(double) + 255) & ~(size_t)255;
  const int rc = l2q_su3_plaq_reduce(xn, nb, T, X, Y, Z, (double*)ws, (char*)ws + head, ws_bytes - head, stream);
  if (rc != L2Q_OK) return rc;
  hipLaunchKernelGGL(su3_plaq_re_kernel, dim3((unsigned)cdiv(nb, kBlock)), dim3(kBlock), 0, st, (const double*)ws,
                     plaq, nb);
  return check_launch(what);
}

extern "C" {

int l2q_su3_force(const void* xn, double beta, void* fn, int nb, int T, int X, int Y, int Z,
                  void* stream) {
  return force_entry("l2q_su3_force", false, xn, beta, fn, nb, T, X, Y, Z, stream);
}

int l2q_su3_force_upper(const void* xn, double beta, void* fu, int nb, int T, int X, int Y, int Z, void* stream) {
  return force_entry("l2q_su3_force_upper", true, xn, beta, fu, nb, T, X, Y, Z, stream);
}

size_t l2q_su3_force_action_ws_bytes(int nb, int T, int X, int Y, int Z) {
  if (!su3_dims_ok(nb, T, X, Y, Z)) return 0;
  // the link kernel's one partial per workgroup (at most V / 64 per chain), or, on the other route, the
  // plaquette reduction's (Re, Im) result in the first 256-byte multiple and its own workspace behind it
  return (((size_t)nb * 2 * sizeof(double) + 255) & ~(size_t)255) + l2q_reduce_ws_bytes(nb, 36L * T * X * Y * Z);
}

int l2q_su3_force_action(const void* xn, double beta, void* fn, double* plaq, int nb, int T, int X, int Y, int Z,
                         void* ws, size_t ws_bytes, void* stream) {
  return force_action_entry("l2q_su3_force_action", false, xn, beta, fn, plaq, nb, T, X, Y, Z, ws, ws_bytes, stream);
}

int l2q_su3_force_action_upper(const void* xn, double beta, void* fu, double* plaq, int nb, int T, int X, int Y,
                               int Z, void* ws, size_t ws_bytes, void* stream) {
  return force_action_entry("l2q_su3_force_action_upper", true, xn, beta, fu, plaq, nb, T, X, Y, Z, ws, ws_bytes,
                            stream);
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
    launch_force_link(LinkForm::Kick, (const double2*)xn, d, nb, coef * beta / 3.0, (const double2*)v_in,
                      (double2*)v_out, nullptr, st);
    return check_launch("l2q_su3_force_kick_to");
  }
  // the other kernels of the family update in place: copy first
  if (v_in != v_out)
    (void)hipMemcpyAsync(v_out, v_in, (size_t)nb * 36 * d.V * sizeof(double2), hipMemcpyDeviceToDevice, st);
  return l2q_su3_force_kick(xn, beta, coef, v_out, nb, T, X, Y, Z, stream);
}

}  // extern "C"
