// su3_wilson_force.hip -- the force of two flavours of Wilson pseudofermions on the links (Gottlieb et al. 1987):
// the derivative of S_f = sum_r phi_r^H (M^H M)^-1 phi_r in the project's convention dS/dt = sum <p, F> under
// dU/dt = p U, given the solutions X_r = (M^H M)^-1 phi_r and Y_r = M X_r.
//
//   W_mu(x) = U_mu(x) sum_r [(1 - gamma_mu) X'_r] Y_r(x)^H - sum_r X_r(x) [(1 + gamma_mu) Y'_r]^H U_mu(x)^H,
//   F_mu(x) = -2 kappa TAH(W_mu(x)),   X' = s X(x+mu), Y' = s Y(x+mu), s the seam sign of the operator,
// a b^H the colour outer product summed over spin.  TAH(-B) = TAH(B^H) folds the second term into the first, and
// 1 -+ gamma_mu = P has rank 2 with sum_spin (P a) b^H = sum_{a<2} h(a)_a h(b)_a^H for the half spinors h of
// su3_spinor.hpp (B_mu is unitary).  So W may be replaced by U_mu(x) C,
//   C = sum_r sum_{a<2} [h-(X')_a h-(Y)_a^H + h+(Y')_a h+(X)_a^H]:
// four projections and four rank-1 colour updates per pseudofermion, one 3 x 3 product per link.
//
// su3_wilson_force_kernel: one thread per (chain, site, mu), a workgroup one direction of 256 sites; every operand a
// coalesced 16 B / lane plane load.  Block order: chain, site block, direction -- the four workgroups that read the
// same X(x), Y(x) follow each other.  (One thread per (chain, site) looping over mu, the map of the operator, took
// 0.48 ms against 0.32 ms at 8^4 x 256, npf = 1: profiles/su3_wilson_force.md.)  The sum over r runs in its order inside the thread, every link is written by
// its thread alone, nothing is reduced: no atomics, no barrier, threads past the last site return.  The output is
// f_in + coef F entry by entry; F itself is anti-Hermitian by construction (the two planes of a transposed pair get
// one number and its negative, the diagonal no real part), so with an anti-Hermitian f_in -- or none -- plane (j, i)
// of the output is (-re, im) of plane (i, j) bit for bit.
#include "su3_spinor.hpp"

namespace l2q {

// The field index r as the compiler may not see through it: otherwise it turns the 48 plane addresses of the four
// projections into 48 pointers carried and stepped through the r loop (256 VGPRs and 42 spilled; 210 and none this way).
#if defined(__HIP_DEVICE_COMPILE__)
#define L2Q_WF_OPAQUE(x) asm volatile("" : "+s"(x));
#else
#define L2Q_WF_OPAQUE(x)
#endif

// c += sum_{a<2} p_a q_a^H: the colour outer product of two half spinors, summed over their two spin components
__device__ __forceinline__ void half_outer_acc(M3& c, const HalfSpinor& p, const HalfSpinor& q) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double pr = p.re[3 * a + i], pi = p.im[3 * a + i], qr = q.re[3 * a + j], qi = q.im[3 * a + j];
        double re = c.re[3 * i + j], im = c.im[3 * i + j];
        re = fma(pr, qr, re); re = fma(pi, qi, re);
        im = fma(pi, qr, im); im = fma(-pr, qi, im);
        c.re[3 * i + j] = re; c.im[3 * i + j] = im;
      }
}

// out = (fin ? fin : 0) + cf TAH(U_mu(s) C) at link (mu, s) of one chain; xs, ys: the chain's npf fields
__device__ __forceinline__ void wilson_force_link(const double2* __restrict__ um, const double2* __restrict__ xs,
                                                  const double2* __restrict__ ys, const double2* fin,
                                                  double2* fout, double cf, bool seam, int npf,
                                                  const Dims& d, int s, int mu) {
  const int V = d.V;
  const int st = stride_of(d, mu), ext = extent_of(d, mu);
  const bool wrap = (s / st) % ext + 1 == ext;
  const int sf = wrap ? s - (ext - 1) * st : s + st;
  const double bs = seam && wrap ? -1.0 : 1.0;
  M3 c;
  m3_zero(c);
#pragma unroll 1
  for (int r = 0; r < npf; ++r) {
    int ro = r;
    L2Q_WF_OPAQUE(ro)
    const double2* xr = xs + ro * 12L * V;
    const double2* yr = ys + ro * 12L * V;
    HalfSpinor p, q;
    wilson_project(p, xr, V, sf, mu, 1.0, bs);       // h-(X') h-(Y)^H
    wilson_project(q, yr, V, s, mu, 1.0, 1.0);
    half_outer_acc(c, p, q);
    wilson_project(p, yr, V, sf, mu, -1.0, bs);      // h+(Y') h+(X)^H
    wilson_project(q, xr, V, s, mu, -1.0, 1.0);
    half_outer_acc(c, p, q);
  }
  M3 u, w;
  load_link(u, um, V, s);
  m3_mul_nn(w, u, c);
  store_tah_axpy(fin, fout, V, s, cf, w);
}

// cf = -2 kappa coef; apbc: the seam of direction 0 carries -1; fin may be null or fout
__global__ __launch_bounds__(kBlock, 2) void su3_wilson_force_kernel(const double2* __restrict__ xn,
                                                                     const double2* __restrict__ xs,
                                                                     const double2* __restrict__ ys,
                                                                     const double2* fin, double2* fout, double cf,
                                                                     int apbc, int npf, int T, int X, int Y, int Z,
                                                                     long nblk, int swz) {
  const Dims d{T, X, Y, Z, T * X * Y * Z};
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long c = w / (4 * nblk), rest = w % (4 * nblk);
  const int mu = (int)(rest % 4);
  const int s = (int)(rest / 4) * kBlock + (int)threadIdx.x;
  if (s >= d.V) return;
  const long link = (c * 4 + mu) * 9L * d.V;
  wilson_force_link(xn + link, xs + c * npf * 12L * d.V, ys + c * npf * 12L * d.V, fin ? fin + link : nullptr,
                    fout + link, cf, apbc != 0 && mu == 0, npf, d, s, mu);
}

}  // namespace l2q

using namespace l2q;

extern "C" {

int l2q_su3_wilson_force(const void* xn, const void* X, const void* Y, const void* f_in, void* f_out, double kappa,
                         double coef, int flags, int nb, int npf, int T, int X_, int Y_, int Z, void* stream) {
  L2Q_REQUIRE(xn && X && Y && f_out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(f_out != xn && f_out != X && f_out != Y, L2Q_EINVAL, "f_out must not alias xn, X or Y");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X_, Y_, Z) && npf > 0, L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(spinor_dims_ok((long)nb * npf, (long)T * X_ * Y_ * Z), L2Q_EINVAL,
              "size: nb * npf * 12 * V does not fit an int");
  L2Q_REQUIRE(kappa - kappa == 0.0, L2Q_EINVAL, "kappa must be finite");
  L2Q_REQUIRE(coef - coef == 0.0, L2Q_EINVAL, "coef must be finite");
  L2Q_REQUIRE((flags & ~2) == 0, L2Q_EINVAL, "flags must be 0 or 2 (bit 1 antiperiodic in t)");
  const Dims d = make_dims(T, X_, Y_, Z);
  const long nblk = cdiv(d.V, kBlock);
  hipLaunchKernelGGL(su3_wilson_force_kernel, dim3((unsigned)((long)nb * 4 * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, (const double2*)xn, (const double2*)X, (const double2*)Y,
                     (const double2*)f_in, (double2*)f_out, -2.0 * kappa * coef, (flags >> 1) & 1, npf, T, X_, Y_, Z,
                     nblk, tuning().xcd_swizzle);
  return check_launch("l2q_su3_wilson_force");
}

}  // extern "C"
