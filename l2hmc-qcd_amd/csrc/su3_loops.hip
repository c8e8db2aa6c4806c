// su3_loops.hip -- straight lines of SU(3) links and what closes them: planar R x T Wilson loops and Polyakov loops.
//
// Line:  L_mu(x, n) = U_mu(x) U_mu(x + mu) ... U_mu(x + (n-1) mu), periodic.  A field of lines has the shape and
//        the native layout xn[chain][mu][e][site] of a link field; L(., 1) is the links.  One more link:
//          L_mu(x, n + 1) = L_mu(x, n) U_mu(x + n mu)                                   (su3_line_extend_kernel)
// Loop:  for an ordered pair mu != nu, a line field A of length r and a line field B of length t,
//          W_{mu nu}(x) = A_mu(x) B_nu(x + r mu) A_mu(x + t nu)^H B_nu(x)^H             (su3_loop_reduce_kernel)
//        in the plaquette convention of su3_plaq_kernel: A = B = links, r = t = 1 is P_{mu nu}(x), with the same
//        two products per site, tr[(A_mu(x) B_nu(x + r mu)) (B_nu(x) A_mu(x + t nu))^H].
// Polyakov loop: P_mu(x_perp) = tr L_mu(x with x_mu = 0, N_mu)                         (su3_polyakov_kernel)
//
// The shifts r, t, n are run-time values, so nothing here keeps a halo: all three are flat kernels, lane <-> site,
// every operand a coalesced 16 B / lane load, the shifted ones re-read through L1 / L2.
#include "su3_launch.hpp"

namespace l2q {

// ------------------------------------------------------------------ one more link on every line
// One thread per (chain, mu, site); mu comes from the block index, so it is wave-uniform.  lin may be lout: a
// thread reads only its own entry of lin, and entry e of its result depends on entry e of what it read, so no
// store can pass the load of the value it replaces.  xn is read at another site and must not be lout.
__global__ __launch_bounds__(kBlock) void su3_line_extend_kernel(const double2* lin, const double2* __restrict__ xn,
                                                                 int n, double2* lout, int T, int X, int Y, int Z,
                                                                 long nblk, int swz) {
  const Dims d{T, X, Y, Z, T * X * Y * Z};
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long f = w / nblk, blk = w % nblk;              // f = 4 chain + mu
  const int mu = (int)(f & 3);
  const int s = (int)blk * kBlock + threadIdx.x;
  if (s >= d.V) return;
  const int ext = extent_of(d, mu);
  const int s2 = site_shifted(s, stride_of(d, mu), ext, n % ext);
  const long off = f * 9L * d.V;
  M3 a, u, o;
  load_link(a, lin + off, d.V, s);
  load_link(u, xn + off, d.V, s2);
  m3_mul_nn(o, a, u);
  store_link(lout + off, d.V, s, o);
}

// ------------------------------------------------------------------ loop sums
// partial[c][blk][k][re|im], k = 3 mu + (nu < mu ? nu : nu - 1), the sum over the block's sites of tr W_{mu nu}.
// One thread per site.  A_mu(x) is loaded once per mu and stays in registers for its three nu; B_nu(x) would
// serve three mu as well, but holding all four next to the pair's temporaries is 4 x 36 more registers than two
// wavefronts per SIMD leave, so it is re-read (an L1 / L2 hit: the same thread read it 3 pairs ago).  Neither
// loop is unrolled: as in su3_plaq_kernel that bounds the live set, here A_mu(x), the product and two operands.
// The extents are scalar arguments and the coordinates come by division (a Dims argument or a Site indexed by
// a loop-variant direction is copied to scratch, see su3_clover_kernel).  The 24 sums of a wavefront go through
// shuffles, the four wavefronts through LDS in a fixed order: one barrier per block.
__global__ __launch_bounds__(kBlock, 2) void su3_loop_reduce_kernel(const double2* __restrict__ a, int r,
                                                                    const double2* __restrict__ b, int t, int T,
                                                                    int X, int Y, int Z, long nblk, int swz,
                                                                    double* __restrict__ partial) {
  __shared__ double red[4][24];
  const Dims d{T, X, Y, Z, T * X * Y * Z};
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long c = w / nblk, blk = w % nblk;
  const int s0 = (int)blk * kBlock + threadIdx.x;
  const bool live = s0 < d.V;
  const int s = live ? s0 : 0, V = d.V;
  const double2* ac = a + c * 36L * V;
  const double2* bc = b + c * 36L * V;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1
  for (int mu = 0; mu < 4; ++mu) {
    const int emu = extent_of(d, mu);
    const int s_r = site_shifted(s, stride_of(d, mu), emu, r % emu);
    M3 am;
    load_link(am, ac + mu * 9 * V, V, s);
#pragma unroll 1
    for (int j = 0; j < 3; ++j) {
      const int nu = j + (j >= mu ? 1 : 0);
      const int enu = extent_of(d, nu);
      const int s_t = site_shifted(s, stride_of(d, nu), enu, t % enu);
      M3 p, q, y;
      load_link(p, bc + nu * 9 * V, V, s_r);
      m3_mul_nn(y, am, p);
      load_link(p, bc + nu * 9 * V, V, s);
      load_link(q, ac + mu * 9 * V, V, s_t);
      double sr = 0.0, si = 0.0;
      m3_trace_y_abh(sr, si, y, p, q);
      if (!live) { sr = 0.0; si = 0.0; }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        sr += __shfl_down(sr, off, 64); si += __shfl_down(si, off, 64);
      }
      if (lane == 0) { red[wave][(3 * mu + j) * 2 + 0] = sr; red[wave][(3 * mu + j) * 2 + 1] = si; }
    }
  }
  __syncthreads();
  if (threadIdx.x < 24) {
    const int i = threadIdx.x;
    partial[(c * nblk + blk) * 24 + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
  }
}

// ------------------------------------------------------------------ Polyakov loops
// One thread per (chain, perpendicular site): the perpendicular sites in the lattice's own order with direction
// mu removed, so adjacent lanes take adjacent sites of the fastest perpendicular direction (z; y for mu = 3, where
// a thread's own walk along z uses the rest of each cache line).  mu is a kernel argument.  Extent 1 gives tr U.
__global__ __launch_bounds__(kBlock) void su3_polyakov_kernel(const double2* __restrict__ xn, int mu, int T, int X,
                                                              int Y, int Z, long nblk, double2* __restrict__ out) {
  const Dims d{T, X, Y, Z, T * X * Y * Z};
  const long c = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int ext = extent_of(d, mu), st = stride_of(d, mu);
  const int Vp = d.V / ext;
  const int q = (int)blk * kBlock + threadIdx.x;
  if (q >= Vp) return;
  int rem = q, s = 0;                                   // the site with x_mu = 0 above perpendicular site q
  if (mu != 3) { s += rem % Z; rem /= Z; }
  if (mu != 2) { s += (rem % Y) * Z; rem /= Y; }
  if (mu != 1) { s += (rem % X) * Y * Z; rem /= X; }
  if (mu != 0) s += rem * X * Y * Z;
  const double2* f = xn + (c * 4 + mu) * 9L * d.V;
  M3 acc;
  load_link(acc, f, d.V, s);
#pragma unroll 1
  for (int k = 1; k < ext; ++k) {
    M3 u, p;
    load_link(u, f, d.V, s + k * st);
    m3_mul_nn(p, acc, u);
    acc = p;
  }
  out[c * Vp + q] = make_double2(acc.re[0] + acc.re[4] + acc.re[8], acc.im[0] + acc.im[4] + acc.im[8]);
}

}  // namespace l2q

using namespace l2q;

extern "C" {

int l2q_su3_line_extend(const void* lines_in, const void* xn, int n, void* lines_out, int nb, int T, int X, int Y,
                        int Z, void* stream) {
  L2Q_REQUIRE(lines_in && xn && lines_out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(n >= 0, L2Q_EINVAL, "negative shift n");
  L2Q_REQUIRE(lines_out != xn, L2Q_EINVAL, "lines_out must not alias xn");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V, kBlock);
  hipLaunchKernelGGL(su3_line_extend_kernel, dim3((unsigned)(nb * 4L * nblk)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const double2*)lines_in, (const double2*)xn, n, (double2*)lines_out, T, X, Y, Z, nblk,
                     tuning().xcd_swizzle);
  return check_launch("l2q_su3_line_extend");
}

int l2q_su3_loop_reduce(const void* a, int r, const void* b, int t, double* out, int nb, int T, int X, int Y, int Z,
                        void* ws, size_t ws_bytes, void* stream) {
  L2Q_REQUIRE(a && b && out && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(r >= 1 && t >= 1, L2Q_EINVAL, "line lengths r, t must be >= 1");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V, kBlock);
  L2Q_REQUIRE(ws_bytes >= (size_t)nb * nblk * 24 * sizeof(double), L2Q_ESHAPE, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(su3_loop_reduce_kernel, dim3((unsigned)(nb * nblk)), dim3(kBlock), 0, st, (const double2*)a, r,
                     (const double2*)b, t, T, X, Y, Z, nblk, tuning().xcd_swizzle, (double*)ws);
  launch_finalize((const double*)ws, out, nb, nblk, 24, 1.0, 0.0, st);
  return check_launch("l2q_su3_loop_reduce");
}

int l2q_su3_polyakov(const void* xn, int mu, void* out, int nb, int T, int X, int Y, int Z, void* stream) {
  L2Q_REQUIRE(xn && out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(mu >= 0 && mu < 4, L2Q_EINVAL, "direction mu must be 0..3");
  const Dims d = make_dims(T, X, Y, Z);
  const int ext = mu == 0 ? T : mu == 1 ? X : mu == 2 ? Y : Z;
  const long nblk = cdiv(d.V / ext, kBlock);
  hipLaunchKernelGGL(su3_polyakov_kernel, dim3((unsigned)(nb * nblk)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const double2*)xn, mu, T, X, Y, Z, nblk, (double2*)out);
  return check_launch("l2q_su3_polyakov");
}

}  // extern "C"
