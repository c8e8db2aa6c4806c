// su3_wilson_eo.hip -- the half-lattice hop of the Wilson-Dirac operator, the one kernel of even-odd preconditioning
// (DeGrand & Rossi 1990).  H couples sites of opposite parity only, so M psi = b reduces to the Schur system on the
// even sites,
//   Mhat psi_e = b_e + kappa H_eo b_o,   Mhat = 1 - kappa^2 H_eo H_oe,   psi_o = b_o + kappa H_oe psi_e,
// and every piece of it is
//   out(x) = b aux(x) + a (H src)(x)   for the sites x of one parity,
// src a half field on the other parity, aux (may be null: no b term) and out half fields on this one:
//   H_oe / H_eo alone: a = 1, b = 0, no aux;   the second half of Mhat: a = -kappa^2, b = 1, aux = psi_e;
//   the source b_e + kappa H_eo b_o and the reconstruction b_o + kappa H_oe psi_e: a = kappa, b = 1.
// H, the gamma basis, the seam sign and the flags are those of su3_wilson.hip; the dagger bit on both hops gives Mhat^H,
// since (H^H)_eo = gamma5 H_eo gamma5.
//
// A half field is psi_h[chain][rhs][12][V/2]: the sites of one parity in lexicographic order, half index h <-> site
// checkerboard_site(h, parity) (su3_subgroup.hpp).  All extents are even; with Z even the sites 2h and 2h + 1 differ in
// z only and have opposite parity, so the neighbour site s' of a site has the half index s' >> 1 in the other parity's
// field, and consecutive lanes load consecutive entries.  The links stay in the full native layout xn[chain][4][9][V]:
// a link load reads every second site of a plane, so it uses half of each cache line it touches (the load of the
// opposite direction uses the other half; a parity-ordered copy of the links would cure that; it is not built).
// su3_wilson_hop_eo_kernel: one thread per (system, half-site), the body of su3_wilson_kernel with the other
// addressing: the direction loop not unrolled, workgroups in the order chain, site block, right-hand side, the same
// xcd_swizzle, the same fixed-tree norm partials part[system][ceil((V/2) / 256)].  An extent of 2 is legal: the two
// neighbours coincide and both terms are added.  out may be aux (a thread reads, then writes, its own entries).
#include "su3_spinor.hpp"
#include "su3_subgroup.hpp"

namespace l2q {

// sgn: +1 for H, -1 for gamma5 H gamma5; apbc: the seam of direction 0 carries -1.  aux, part: may be null.
// The kernel has a barrier where part is given: threads past the last half-site run along on half-site 0 and write
// nothing.
__global__ __launch_bounds__(kBlock, 2) void su3_wilson_hop_eo_kernel(const double2* __restrict__ xn,
                                                                      const double2* __restrict__ src,
                                                                      const double2* aux, double2* out,
                                                                      double* __restrict__ part, double a, double bc,
                                                                      double sgn, int apbc, int parity, int nrhs, int T,
                                                                      int X, int Y, int Z, long nblk, int swz) {
  __shared__ double red[4];
  const Dims d{T, X, Y, Z, T * X * Y * Z};
  const WilsonBlock b = wilson_block(xcd_swizzle(blockIdx.x, (long)gridDim.x, swz), nrhs, nblk);
  const int V = d.V, Vh = V / 2;
  const int h0 = b.blk * kBlock + (int)threadIdx.x;
  const bool live = h0 < Vh;
  const int hs = live ? h0 : 0;
  const int s = checkerboard_site(hs, parity, X, Y, Z);
  const double2* xc = xn + b.c * 36L * V;
  const double2* pc = src + b.sys * 12L * Vh;
  double ar[12], ai[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) { ar[k] = 0.0; ai[k] = 0.0; }
#pragma unroll 1
  for (int mu = 0; mu < 4; ++mu) {
    const int st = stride_of(d, mu), ext = extent_of(d, mu);
    const double2* um = xc + mu * 9L * V;
    const int cm = (s / st) % ext;
    const bool seam = apbc != 0 && mu == 0;
    HalfSpinor h, chi;
    M3 u;
    {  // (1 - gamma_mu) U_mu(x) src(x+mu)
      const bool wrap = cm + 1 == ext;
      const int sf = wrap ? s - (ext - 1) * st : s + st;
      wilson_project(h, pc, Vh, sf >> 1, mu, sgn, seam && wrap ? -1.0 : 1.0);
      load_link(u, um, V, s);
      wilson_colour_mul<false>(chi, u, h);
      wilson_reconstruct(ar, ai, chi, mu, sgn);
    }
    {  // (1 + gamma_mu) U_mu(x-mu)^H src(x-mu)
      const bool wrap = cm == 0;
      const int sb = wrap ? s + (ext - 1) * st : s - st;
      wilson_project(h, pc, Vh, sb >> 1, mu, -sgn, seam && wrap ? -1.0 : 1.0);
      load_link(u, um, V, sb);
      wilson_colour_mul<true>(chi, u, h);
      wilson_reconstruct(ar, ai, chi, mu, -sgn);
    }
  }
  const long off = b.sys * 12L * Vh;
  double n2 = 0.0;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    double re = a * ar[k], im = a * ai[k];
    if (aux != nullptr) {              // a kernel argument: wave-uniform
      const double2 p = aux[off + k * Vh + hs];
      re = fma(a, ar[k], bc * p.x); im = fma(a, ai[k], bc * p.y);
    }
    if (live) out[off + k * Vh + hs] = make_double2(re, im);
    n2 = fma(re, re, n2); n2 = fma(im, im, n2);
  }
  if (part != nullptr) {               // a kernel argument: the whole grid takes the barrier or none of it
    const double t = block_sum(live ? n2 : 0.0, red);
    if (threadIdx.x == 0) part[b.sys * nblk + b.blk] = t;
  }
}

}  // namespace l2q

using namespace l2q;

extern "C" {

int l2q_su3_wilson_hop_eo(const void* xn, const void* src, const void* aux, void* out, double* norm_part, double a,
                          double b, int flags, int parity, int nb, int nrhs, int T, int X, int Y, int Z, void* stream) {
  L2Q_REQUIRE(xn && src && out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(out != src && out != xn, L2Q_EINVAL, "out must not alias src or xn");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z) && nrhs > 0, L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(spinor_dims_ok((long)nb * nrhs, (long)T * X * Y * Z), L2Q_EINVAL,
              "size: nb * nrhs * 12 * V does not fit an int");
  L2Q_REQUIRE(a - a == 0.0 && b - b == 0.0, L2Q_EINVAL, "the coefficients a and b must be finite");
  L2Q_REQUIRE(flags >= 0 && flags <= 3, L2Q_EINVAL, "flags must be 0..3 (bit 0 dagger, bit 1 antiperiodic in t)");
  L2Q_REQUIRE(parity == 0 || parity == 1, L2Q_EINVAL, "parity must be 0 (even) or 1 (odd)");
  L2Q_REQUIRE(all_even(T, X, Y, Z), L2Q_ESHAPE, "a checkerboard update needs even extents");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V / 2, kBlock);
  hipLaunchKernelGGL(su3_wilson_hop_eo_kernel, dim3((unsigned)((long)nb * nrhs * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, (const double2*)xn, (const double2*)src, (const double2*)aux, (double2*)out,
                     norm_part, a, b, (flags & 1) ? -1.0 : 1.0, (flags >> 1) & 1, parity, nrhs, T, X, Y, Z, nblk,
                     tuning().xcd_swizzle);
  return check_launch("l2q_su3_wilson_hop_eo");
}

}  // extern "C"
