// su3_flow.hip -- Wilson (gradient) flow of the SU(3) links and the clover observables measured on
// the flowed field: energy density E, topological charge Q (Luescher, arXiv:1006.4518).
//
// Clover: for mu < nu, Q_{mu nu}(x) = the four plaquette leaves in the (mu, nu) plane that start and
// end at x, all counter-clockwise,
//   L1 = U_mu(x) U_nu(x+mu) U_mu(x+nu)^H U_nu(x)^H
//   L2 = U_nu(x) U_mu(x-mu+nu)^H U_nu(x-mu)^H U_mu(x-mu)
//   L3 = U_mu(x-mu)^H U_nu(x-mu-nu)^H U_mu(x-mu-nu) U_nu(x-nu)
//   L4 = U_nu(x-nu)^H U_mu(x-nu) U_nu(x+mu-nu) U_mu(x)^H
// F_{mu nu}(x) = TAH(Q_{mu nu}(x)) / 4 (anti-Hermitian, traceless).  Per chain the kernel sums
//   out[c][0] = sum_x sum_{mu<nu} -tr F F      out[c][1] = sum_x -tr(F01 F23 - F02 F13 + F03 F12)
//   out[c][2] = sum_x sum_{mu<nu} Re tr L1     (the plaquette sum: leaf 1 is the plaquette)
// The planes are walked as the pairs (01,23), (02,13), (03,12), so only two F are ever live.
//
// Flow: one low-storage stage is P_out = P_in + c TAH(U A), X_out = exp(s P_out) X_in with A the six
// staples of l2q_su3_force; here it is the force kick at beta = 3 into P_out followed by the unmasked
// expm_mul, out of place, so no neighbour ever sees a new link.
#include "su3_clover.hpp"
#include "su3_launch.hpp"

namespace l2q {

// Generic clover kernel: one thread per site, operands through L1/L2; any lattice (extents 1 and 2,
// odd sizes, V no multiple of the block).  The plane loop is NOT unrolled (live ranges, as su3_plaq_kernel).
__global__ __launch_bounds__(kBlock, 2) void su3_clover_kernel(const double2* __restrict__ xn, int T, int X, int Y,
                                                              int Z, long nblk, int swz, int lo,
                                                              double* __restrict__ partial) {
  // (the extents as scalar arguments: selected by a loop-variant direction out of a Dims ARGUMENT, hipcc copies
  // the struct to scratch and indexes it)
  const Dims d{T, X, Y, Z, T * X * Y * Z};
  __shared__ double lds[12];
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long c = w / nblk, blk = w % nblk;
  const int s = (int)blk * kBlock + threadIdx.x;
  double se = 0.0, sq = 0.0, sp = 0.0;
  if (s < d.V) {
    const double2* xc = xn + c * 36L * d.V;
    const int V = d.V;
    const bool go = s >= lo;
    const auto ld = [=](M3& m, int dir, int site) { load_link(m, xc + dir * 9 * V, V, site); };
    AH3 f = {};
#pragma unroll 1
    for (int pl = 0; pl < 6; ++pl) {
      // planes in the order (01), (23), (02), (13), (03), (12): each odd one is the dual of the one before it,
      // eps_{0 k a b} = +, -, +
      const int k = (pl >> 1) + 1;
      const int mu = (pl & 1) ? (k == 1 ? 2 : 1) : 0;
      const int nu = (pl & 1) ? (k == 3 ? 2 : 3) : k;
      // (coordinates by division: hipcc turns coord_of(p, mu) with a loop-variant mu into an indexed read of p
      // kept in scratch)
      const int cmu = (s / stride_of(d, mu)) % extent_of(d, mu), cnu = (s / stride_of(d, nu)) % extent_of(d, nu);
      CloverSites<int> st;
      st.o = s;
      st.pm = fwd(s, cmu, d, mu); st.mm = bwd(s, cmu, d, mu);
      st.pn = fwd(s, cnu, d, nu); st.mn = bwd(s, cnu, d, nu);
      st.mm_pn = fwd(st.mm, cnu, d, nu); st.mm_mn = bwd(st.mm, cnu, d, nu);
      st.pm_mn = bwd(st.pm, cnu, d, nu);
      AH3 g;
      clover_plane(g, sp, ld, st, mu, nu, go);
      se += clover_mtr(g, g);
      if (pl & 1) {
        const double fg = clover_mtr(f, g);
        sq += (k == 2) ? -fg : fg;
      }
      f = g;
    }
  }
  const double be = block_sum(se, lds);
  const double bq = block_sum(sq, lds + 4);
  const double bp = block_sum(sp, lds + 8);
  if (threadIdx.x == 0) {
    double* o = partial + (c * nblk + blk) * 3;
    o[0] = be; o[1] = bq; o[2] = bp;
  }
}

// ------------------------------------------------------------------ clover, slice-resident
// For lattices whose spatial volume is whole 64-site tiles (8^4, 16^4).  One workgroup = a 64-site spatial tile of
// one chain, sweeping t, with THREE time slices of the tile's links resident in LDS (t-1, t, t+1: 3 x [4][9][64]
// complex = 108 KiB, one workgroup per CU); the slice after next is prefetched into registers behind the
// arithmetic and replaces slice t-1 at the end of the iteration, so every link is fetched from HBM once per sweep
// (plus the halo of the tile).  Three wavefronts, one per plane pair: wavefront k takes the temporal plane
// (0, k+1) -- the only planes that reach into slices t-1 and t+1 -- and its dual spatial plane, so both F of a
// charge term live in one thread and nothing but the three block sums is exchanged.  An operand whose site lies
// in the tile (every own, +-t, +-y, +-z site of a (y, z)-plane tile) is an LDS read; the others (+-x) come from
// L2.  One wavefront per SIMD: the 512-register budget keeps the plane's temporaries out of scratch.
constexpr int kCT = 64;                       // sites per tile
constexpr int kCSlot = 4 * 9 * kCT;           // complex entries of one slice of the tile
constexpr int kCThreads = 192;
constexpr int kCPre = kCSlot / kCThreads;     // entries per thread when a slice is staged (12)

struct CSite {
  const double2* slot;   // the LDS copy of the tile's slice this site is in
  const double2* gsl;    // the chain's links at that time slice (index by spatial site)
  int q;                 // spatial site
};

__global__ __launch_bounds__(kCThreads, 1) void su3_clover_slice_kernel(const double2* __restrict__ xn, Dims d,
                                                                       int nsb, int tsplit, int swz, int lo,
                                                                       double* __restrict__ partial) {
  extern __shared__ double2 cl_lds[];                   // [3][4][9][kCT]
  __shared__ double red[9];
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const int per_chain = nsb * tsplit;
  const long c = w / per_chain;
  const int r = (int)(w % per_chain);
  const int tc = r / nsb, sb = r % nsb;
  const int Vs = d.X * d.Y * d.Z, V = d.V, T = d.T;
  const int tile0 = sb * kCT;
  const int lt = threadIdx.x & (kCT - 1), k = (threadIdx.x >> 6) + 1;      // k is wave-uniform
  const int tlen = (T + tsplit - 1) / tsplit;
  const int t0 = tc * tlen, t1 = min(T, t0 + tlen);
  const double2* xc = xn + c * 36L * V;
  const bool go = (int)threadIdx.x >= lo;
  // entry j of a slice of the tile: link and matrix entry j / 64, site tile0 + j % 64
  const auto stage_addr = [=](int t, int i) {
    const int j = i * kCThreads + (int)threadIdx.x;
    return xc + (long)(j >> 6) * V + (long)t * Vs + tile0 + (j & 63);
  };
  // prologue: slices t0-1, t0, t0+1 -> slots 0, 1, 2
#pragma unroll 1
  for (int sl = 0; sl < 3; ++sl) {
    const int t = (t0 - 1 + sl + 2 * T) % T;
#pragma unroll
    for (int i = 0; i < kCPre; ++i) cl_lds[sl * kCSlot + i * kCThreads + threadIdx.x] = *stage_addr(t, i);
  }
  __syncthreads();
  SPos p;
  p.q = tile0 + lt;
  {
    int q = p.q;
    p.z = q % d.Z; q /= d.Z;
    p.y = q % d.Y; q /= d.Y;
    p.x = q;
  }
  // the dual of plane (0, k): (a, b) = the two other spatial directions, eps_{0 k a b} = +, -, +
  const int a = k == 1 ? 2 : 1, b = k == 3 ? 2 : 3;
  const SPos pkp = sp_move(p, k, +1, d), pkm = sp_move(p, k, -1, d);
  const SPos pap = sp_move(p, a, +1, d), pam = sp_move(p, a, -1, d);
  const SPos pbp = sp_move(p, b, +1, d), pbm = sp_move(p, b, -1, d);
  const int q_am_bp = sp_move(pam, b, +1, d).q, q_am_bm = sp_move(pam, b, -1, d).q, q_ap_bm = sp_move(pap, b, -1, d).q;
  const auto ld = [=](M3& m, int dir, const CSite& s) {
    const int li = s.q - tile0;
    if (__all((unsigned)li < (unsigned)kCT)) {
      const double2* l = s.slot + dir * 9 * kCT + li;
#pragma unroll
      for (int e = 0; e < 9; ++e) {
        const double2 dd = l[e * kCT];
        m.re[e] = dd.x; m.im[e] = dd.y;
      }
      // (keeps the two sides apart: merged into one load through a selected flat pointer, every operand costs a
      // 64-bit address register pair and the LDS reads lose their immediate offsets)
      asm volatile("" ::: "memory");
    } else {
      load_link(m, s.gsl + dir * 9 * V, V, s.q);
    }
  };
  double se = 0.0, sq = 0.0, sp = 0.0;
  int sprev = 0;                                        // slot of slice t-1; t, t+1 follow cyclically
#pragma unroll 1
  for (int t = t0; t < t1; ++t) {
    const int tm = (t - 1 + T) % T, tp = (t + 1) % T;
    const bool more = t + 1 < t1;
    // The slice after next, 12 entries per thread, as named scalars (an array stays in scratch here); unconditional:
    // after the last slice it re-reads slice t, which is in cache.
#define L2Q_CPRE(OP) OP(0) OP(1) OP(2) OP(3) OP(4) OP(5) OP(6) OP(7) OP(8) OP(9) OP(10) OP(11)
    static_assert(kCPre == 12, "L2Q_CPRE lists 12 entries");
    const int tn = more ? (t + 2) % T : t;
#define L2Q_CPRE_LOAD(i) const double2 pre##i = *stage_addr(tn, i);
    L2Q_CPRE(L2Q_CPRE_LOAD)
    const double2* lprev = cl_lds + sprev * kCSlot;
    const double2* lcur = cl_lds + ((sprev + 1) % 3) * kCSlot;
    const double2* lnext = cl_lds + ((sprev + 2) % 3) * kCSlot;
    const double2* gprev = xc + (long)tm * Vs;
    const double2* gcur = xc + (long)t * Vs;
    const double2* gnext = xc + (long)tp * Vs;
    AH3 f, g;
    // an opaque zero added to every site index: the operand addresses then depend on a value of this iteration,
    // so hipcc cannot hoist ~200 loop-invariant address registers out of the t loop (it did, and spilled them)
    int z0 = 0, z1 = 0;
    asm volatile("" : "+v"(z0), "+v"(z1));
    {
      CloverSites<CSite> st;                            // temporal plane: mu = 0, nu = k
      st.o = {lcur, gcur, p.q + z0};
      st.pm = {lnext, gnext, p.q + z0};
      st.pn = {lcur, gcur, pkp.q + z0};
      st.mm = {lprev, gprev, p.q + z0};
      st.mm_pn = {lprev, gprev, pkp.q + z0};
      st.mm_mn = {lprev, gprev, pkm.q + z0};
      st.mn = {lcur, gcur, pkm.q + z0};
      st.pm_mn = {lnext, gnext, pkm.q + z0};
      clover_plane(f, sp, ld, st, 0, k, go);
    }
    {
      CloverSites<CSite> st;                            // its dual: mu = a, nu = b, all in slice t
      st.o = {lcur, gcur, p.q + z1};
      st.pm = {lcur, gcur, pap.q + z1};
      st.pn = {lcur, gcur, pbp.q + z1};
      st.mm = {lcur, gcur, pam.q + z1};
      st.mm_pn = {lcur, gcur, q_am_bp + z1};
      st.mm_mn = {lcur, gcur, q_am_bm + z1};
      st.mn = {lcur, gcur, pbm.q + z1};
      st.pm_mn = {lcur, gcur, q_ap_bm + z1};
      clover_plane(g, sp, ld, st, a, b, go);
    }
    se += clover_mtr(f, f) + clover_mtr(g, g);
    const double fg = clover_mtr(f, g);
    sq += (k == 2) ? -fg : fg;
    __syncthreads();                                    // slice t-1 fully consumed
#define L2Q_CPRE_PUT(i) cl_lds[sprev * kCSlot + i * kCThreads + threadIdx.x] = pre##i;
    L2Q_CPRE(L2Q_CPRE_PUT)
    sprev = (sprev + 1) % 3;
    __syncthreads();
  }
  // block reduction (3 waves), fixed order
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    se += __shfl_down(se, off, 64); sq += __shfl_down(sq, off, 64); sp += __shfl_down(sp, off, 64);
  }
  if (lt == 0) { red[(k - 1) * 3 + 0] = se; red[(k - 1) * 3 + 1] = sq; red[(k - 1) * 3 + 2] = sp; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = partial + (c * per_chain + r) * 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = red[j] + red[3 + j] + red[6 + j];
  }
}

bool clover_slice_applicable(const Dims& d) { return (d.X * d.Y * d.Z) % kCT == 0; }

}  // namespace l2q

using namespace l2q;

extern "C" {

int l2q_su3_clover_reduce(const void* xn, int nb, int T, int X, int Y, int Z, double* out, void* ws,
                          size_t ws_bytes, void* stream) {
  L2Q_REQUIRE(xn && out && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  const Dims d = make_dims(T, X, Y, Z);
  hipStream_t st = (hipStream_t)stream;
  const int swz = tuning().xcd_swizzle;
  if (clover_slice_applicable(d)) {
    const SliceGrid g = slice_grid(d, nb, kCT, 512);           // >= ~2 rounds of 256 CUs, one workgroup each
    L2Q_REQUIRE(ws_bytes >= (size_t)nb * g.per_chain * 3 * sizeof(double), L2Q_ESHAPE, "workspace too small");
    const size_t lds = 3ul * kCSlot * sizeof(double2);
    dynamic_lds_once<su3_clover_slice_kernel>(lds);
    hipLaunchKernelGGL(su3_clover_slice_kernel, dim3((unsigned)g.blocks), dim3(kCThreads), lds, st,
                       (const double2*)xn, d, g.nsb, g.tsplit, swz, 0, (double*)ws);
    launch_finalize((const double*)ws, out, nb, g.per_chain, 3, 1.0, 0.0, st);
    return check_launch("l2q_su3_clover_reduce");
  }
  const long nblk = cdiv(d.V, kBlock);
  L2Q_REQUIRE(ws_bytes >= (size_t)nb * nblk * 3 * sizeof(double), L2Q_ESHAPE, "workspace too small");
  hipLaunchKernelGGL(su3_clover_kernel, dim3((unsigned)(nb * nblk)), dim3(kBlock), 0, st, (const double2*)xn, T, X,
                     Y, Z, nblk, swz, 0, (double*)ws);
  launch_finalize((const double*)ws, out, nb, nblk, 3, 1.0, 0.0, st);
  return check_launch("l2q_su3_clover_reduce");
}

int l2q_su3_flow_stage(const void* x_in, const void* p_in, double c, double s, void* p_out, void* x_out,
                       int nb, int T, int X, int Y, int Z, void* stream) {
  L2Q_REQUIRE(x_in && p_out && x_out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(x_out != x_in, L2Q_EINVAL, "x_out must not alias x_in");
  L2Q_REQUIRE(p_out != x_in && p_out != x_out, L2Q_EINVAL, "p_out must not alias the links");
  // P_out = P_in + c TAH(U A): the force (kick) at beta = 3
  int rc = p_in ? l2q_su3_force_kick_to(x_in, 3.0, c, p_in, p_out, nb, T, X, Y, Z, stream)
                : l2q_su3_force(x_in, 3.0 * c, p_out, nb, T, X, Y, Z, stream);
  if (rc != L2Q_OK) return rc;
  // X_out = exp(s P_out) X_in
  return l2q_su3_expm_mul(x_in, p_out, s, nullptr, 0, x_out, nb, (long)T * X * Y * Z, stream);
}

int l2q_su3_flow_step(const void* x_in, void* x_out, void* ws_p, void* ws_x, double eps, int nb, int T, int X,
                      int Y, int Z, void* stream) {
  L2Q_REQUIRE(x_in && x_out && ws_p && ws_x, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(x_out != x_in && x_out != ws_x && x_in != ws_x, L2Q_EINVAL,
              "x_in, x_out and ws_x must be three different fields");
  L2Q_REQUIRE(ws_p != x_in && ws_p != x_out && ws_p != ws_x, L2Q_EINVAL, "ws_p must not alias the links");
  // W1 = exp(Z0/4) W0;  W2 = exp(8/9 Z1 - 17/36 Z0) W1;  W3 = exp(3/4 Z2 - 8/9 Z1 + 17/36 Z0) W2,  Zi = -eps G(Wi)
  int rc = l2q_su3_flow_stage(x_in, nullptr, 1.0, -0.25 * eps, ws_p, x_out, nb, T, X, Y, Z, stream);
  if (rc != L2Q_OK) return rc;
  rc = l2q_su3_flow_stage(x_out, ws_p, -32.0 / 17.0, (17.0 / 36.0) * eps, ws_p, ws_x, nb, T, X, Y, Z, stream);
  if (rc != L2Q_OK) return rc;
  return l2q_su3_flow_stage(ws_x, ws_p, 27.0 / 17.0, -(17.0 / 36.0) * eps, ws_p, x_out, nb, T, X, Y, Z, stream);
}

}  // extern "C"
