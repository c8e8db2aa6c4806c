// su3_wilson_clover.hip -- the clover term of the O(a)-improved Wilson operator (Sheikholeslami & Wohlert 1985; Luescher,
// Sint, Sommer & Weisz 1996) and the kernels of its even-odd preconditioned solve.
//   M_sw = A - kappa H,   A(x) = 1 + kappa c_sw i sum_{mu<nu} sigma_{mu nu} (x) Fhat_{mu nu}(x),
//   sigma_{mu nu} = (i/2) [gamma_mu, gamma_nu],   Fhat_{mu nu} = (Q_{mu nu} - Q_{mu nu}^H) / 8,
// H the hop of su3_wilson.hip, Q_{mu nu} the sum of the four leaves of su3_clover.hpp; Fhat keeps its trace.  In the
// chiral basis A = diag(A+, A-) (su3_clover_block.hpp): with E_k = Fhat_{0k} and B = (Fhat_23, -Fhat_13, Fhat_12),
//   A+ = 1 - i kappa c_sw sum_k sigma_k (x) (E_k + B_k),   A- = 1 + i kappa c_sw sum_k sigma_k (x) (E_k - B_k).
// A is Hermitian and commutes with gamma5, so M_sw^H = gamma5 M_sw gamma5: the dagger bit of the hop still gives the
// adjoint.  The asymmetric even-odd form:
//   Mhat = A_ee - kappa^2 H_eo A_oo^-1 H_oe,   bhat_e = b_e + kappa H_eo A_oo^-1 b_o,
//   psi_o = A_oo^-1 (b_o + kappa H_oe psi_e).
// Four kernels:
//   su3_clover_term_kernel    one thread per site: the six Fhat through clover_leaves, a temporal plane with its dual as
//                             su3_clover_kernel walks them, E_k +- B_k folded into the two blocks as each pair completes:
//                             sigma_3 fills the two diagonal 3 x 3 spin blocks (stored at once), sigma_1 and sigma_2 the
//                             off-diagonal one (the pair k = 1 waits as two AH3 for k = 2).  Once per configuration.
//   su3_clover_invert_kernel  one thread per (chain, parity, half-site): both blocks inverted by an unpivoted, fully
//                             unrolled L D L^H in registers (no square roots), with the smallest pivot and sum log d_i
//                             of the workgroup by the fixed tree of the norm partials.
//   su3_wilson_clover_hop_eo_kernel<CMODE>   the hot kernel: the body of su3_wilson_hop_eo_kernel, then
//                             CMODE 0  out = b aux + a H src             (the hop itself)
//                             CMODE 1  out = b (C aux) + a H src
//                             CMODE 2  out = C (b aux + a H src)
//                             with C(x) the block pair of the field c at the output site.  Workgroups in the order chain,
//                             site block, right-hand side: the systems of a chain share a site's blocks in cache as
//                             they share its links.
//   su3_clover_apply_kernel   out = C src on a half field, the same 6 x 6 product.
#include "su3_clover.hpp"
#include "su3_clover_block.hpp"
#include "su3_subgroup.hpp"

namespace l2q {

// With X = i W (Hermitian; W anti-Hermitian as an AH3): X_ii = -d_i, X_ij = (-im_e, re_e) for i < j, e = i + j - 1.
// The sigma_3 part of a block, 1 + sc sigma_3 (x) X: the two diagonal 3 x 3 spin blocks, X and -X.
__device__ __forceinline__ void clover_store_sigma3(double* __restrict__ o, int Vh, const AH3& w, double sc) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    o[i * Vh] = fma(-sc, w.d[i], 1.0);
    o[(3 + i) * Vh] = fma(sc, w.d[i], 1.0);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i + 1; j < 3; ++j) {
      const int e = i + j - 1;
      const double xr = -sc * w.im[e], xi = sc * w.re[e];
      const int eu = 6 + 2 * clover_upper(i, j), el = 6 + 2 * clover_upper(3 + i, 3 + j);
      o[eu * Vh] = xr; o[(eu + 1) * Vh] = xi;
      o[el * Vh] = -xr; o[(el + 1) * Vh] = -xi;
    }
}

// The sigma_1 and sigma_2 part: the off-diagonal spin block (rows i, columns 3 + j) is sc (X1 - i X2), all nine entries.
__device__ __forceinline__ void clover_store_sigma12(double* __restrict__ o, int Vh, const AH3& w1, const AH3& w2,
                                                     double sc) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double x1r, x1i, x2r, x2i;
      if (i == j) {
        x1r = -w1.d[i]; x1i = 0.0; x2r = -w2.d[i]; x2i = 0.0;
      } else {
        const int e = i + j - 1;
        const double cj = i < j ? 1.0 : -1.0;                     // below the diagonal: the conjugate
        x1r = -w1.im[e]; x1i = cj * w1.re[e]; x2r = -w2.im[e]; x2i = cj * w2.re[e];
      }
      const int eo = 6 + 2 * clover_upper(i, 3 + j);
      o[eo * Vh] = sc * (x1r + x2i);
      o[(eo + 1) * Vh] = sc * (x1i - x2r);
    }
}

// One workgroup per SIMD set (launch bounds 1): next to the leaf code's Q, two temporaries and one operand the kernel
// carries E_k and the pair k = 1, 27 doubles; with the 256 registers of two workgroups it spills, with 512 it does not.
__global__ __launch_bounds__(kBlock, 1) void su3_clover_term_kernel(const double2* __restrict__ xn,
                                                                    double* __restrict__ cl, double coef, int T, int X,
                                                                    int Y, int Z, long nblk, int swz, int lo) {
  const int V = T * X * Y * Z, Vh = V / 2;
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long c = w / nblk, blk = w % nblk;
  const int s = (int)blk * kBlock + (int)threadIdx.x;
  if (s >= V) return;                                             // no barrier in this kernel
  const double2* xc = xn + c * 36L * V;
  const bool go = s >= lo;
  const auto ld = [=](M3& m, int dir, int site) { load_link(m, xc + dir * 9 * V, V, site); };
  const int par = (s + s / Z + s / (Y * Z) + s / (X * Y * Z)) & 1;     // (t + x + y + z) & 1: the extents are even
  double* up = cl + ((c * 2 + par) * 2) * (long)kCloverReals * Vh + (s >> 1);     // A+, then A-
  double* dn = up + (long)kCloverReals * Vh;
  AH3 e = {}, wp1 = {}, wm1 = {};
#pragma unroll 1
  for (int pl = 0; pl < 6; ++pl) {
    // planes in the order (01), (23), (02), (13), (03), (12): each odd one is the dual of the temporal plane before it,
    // eps_{0 k a b} = +, -, +.  One call of the leaf code in the loop body, as in su3_clover_kernel (live ranges).
    const int k = (pl >> 1) + 1;
    const int mu = (pl & 1) ? (k == 1 ? 2 : 1) : 0;
    const int nu = (pl & 1) ? (k == 3 ? 2 : 3) : k;
    // (coordinates by division, as in su3_clover_kernel)
    const int sm = mu == 0 ? X * Y * Z : mu == 1 ? Y * Z : Z, em = mu == 0 ? T : mu == 1 ? X : Y;      // mu <= 2
    const int sn = nu == 1 ? Y * Z : nu == 2 ? Z : 1, en = nu == 1 ? X : nu == 2 ? Y : Z;               // nu >= 1
    CloverSites<int> st;
    st.o = s;
    st.pm = site_hop(s, sm, em, 1); st.mm = site_hop(s, sm, em, -1);
    st.pn = site_hop(s, sn, en, 1); st.mn = site_hop(s, sn, en, -1);
    st.mm_pn = site_hop(st.mm, sn, en, 1); st.mm_mn = site_hop(st.mm, sn, en, -1);
    st.pm_mn = site_hop(st.pm, sn, en, -1);
    AH3 f;                                                        // Fhat_{mu nu}(s) = (Q - Q^H) / 8
    {
      M3 q;
      double retr = 0.0;
      clover_leaves(q, retr, ld, st, mu, nu, go);
      clover_ah(f, q);
    }
    if (!(pl & 1)) {                                              // pl, k: wave-uniform
      e = f;
      continue;
    }
    const double sg = k == 2 ? -1.0 : 1.0;
    AH3 wp, wm;                                                   // E_k + B_k, E_k - B_k
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      wp.d[i] = fma(sg, f.d[i], e.d[i]); wm.d[i] = fma(-sg, f.d[i], e.d[i]);
      wp.re[i] = fma(sg, f.re[i], e.re[i]); wm.re[i] = fma(-sg, f.re[i], e.re[i]);
      wp.im[i] = fma(sg, f.im[i], e.im[i]); wm.im[i] = fma(-sg, f.im[i], e.im[i]);
    }
    if (k == 3) {
      clover_store_sigma3(up, Vh, wp, -coef);
      clover_store_sigma3(dn, Vh, wm, coef);
    } else if (k == 1) {
      wp1 = wp; wm1 = wm;
    } else {
      clover_store_sigma12(up, Vh, wp1, wp, -coef);
      clover_store_sigma12(dn, Vh, wm1, wm, coef);
    }
  }
}

// One Hermitian 6 x 6 block inverted in registers: A = L D L^H without pivoting (L unit lower triangular, D real
// diagonal, no square roots), A^-1 = M^H D^-1 M with M = L^-1.  Every loop has constant bounds and is unrolled, so
// every array entry is a register.  minpiv takes the smallest d_i, logdet adds sum log d_i (NaN for d_i <= 0: the
// caller reads minpiv first).
__device__ __forceinline__ void clover_invert_block(const double* __restrict__ in, double* __restrict__ out, int Vh,
                                                    bool live, double& minpiv, double& logdet) {
  double dg[6], ur[15], ui[15];                                   // A: diagonal, entries above it
#pragma unroll
  for (int r = 0; r < 6; ++r) dg[r] = in[r * Vh];
#pragma unroll
  for (int e = 0; e < 15; ++e) { ur[e] = in[(6 + 2 * e) * Vh]; ui[e] = in[(7 + 2 * e) * Vh]; }
  double dd[6], inv[6], lr[15], li[15];                           // L_ij (i > j) at clover_upper(j, i)
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double dj = dg[j];
#pragma unroll
    for (int k = 0; k < j; ++k) {
      const int jk = clover_upper(k, j);
      dj = fma(-dd[k], fma(lr[jk], lr[jk], li[jk] * li[jk]), dj);
    }
    dd[j] = dj;
    inv[j] = 1.0 / dj;
    minpiv = fmin(minpiv, dj);
    logdet += log(dj);
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      const int ij = clover_upper(j, i);
      double sr = ur[ij], si = -ui[ij];                           // A_ij = conj(A_ji)
#pragma unroll
      for (int k = 0; k < j; ++k) {                               // - L_ik conj(L_jk) d_k
        const int ik = clover_upper(k, i), jk = clover_upper(k, j);
        const double tr = dd[k] * lr[jk], ti = -dd[k] * li[jk];
        sr = fma(-lr[ik], tr, sr); sr = fma(li[ik], ti, sr);
        si = fma(-lr[ik], ti, si); si = fma(-li[ik], tr, si);
      }
      lr[ij] = sr * inv[j]; li[ij] = si * inv[j];
    }
  }
  double mr[15], mi[15];                                          // M = L^-1: M_ij = -(L_ij + sum_{j<k<i} L_ik M_kj)
#pragma unroll
  for (int j = 0; j < 6; ++j)
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      const int ij = clover_upper(j, i);
      double sr = lr[ij], si = li[ij];
#pragma unroll
      for (int k = j + 1; k < i; ++k) {
        const int ik = clover_upper(k, i), kj = clover_upper(j, k);
        sr = fma(lr[ik], mr[kj], sr); sr = fma(-li[ik], mi[kj], sr);
        si = fma(lr[ik], mi[kj], si); si = fma(li[ik], mr[kj], si);
      }
      mr[ij] = -sr; mi[ij] = -si;
    }
  // (A^-1)_ij = sum_{k >= j} conj(M_ki) M_kj / d_k for i <= j, M_kk = 1
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = inv[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) {
      const int ki = clover_upper(i, k);
      s = fma(inv[k], fma(mr[ki], mr[ki], mi[ki] * mi[ki]), s);
    }
    if (live) out[i * Vh] = s;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i + 1; j < 6; ++j) {
      const int ji = clover_upper(i, j);
      double sr = inv[j] * mr[ji], si = -inv[j] * mi[ji];         // conj(M_ji) / d_j
#pragma unroll
      for (int k = j + 1; k < 6; ++k) {
        const int ki = clover_upper(i, k), kj = clover_upper(j, k);
        const double tr = inv[k] * mr[kj], ti = inv[k] * mi[kj];
        sr = fma(mr[ki], tr, sr); sr = fma(mi[ki], ti, sr);       // conj(M_ki) M_kj / d_k
        si = fma(mr[ki], ti, si); si = fma(-mi[ki], tr, si);
      }
      if (live) { out[(6 + 2 * ji) * Vh] = sr; out[(7 + 2 * ji) * Vh] = si; }
    }
}

// Workgroups: chain, parity, half-site block.  The kernel has barriers: threads past the last half-site run along on
// half-site 0 and write nothing.
__global__ __launch_bounds__(kBlock, 2) void su3_clover_invert_kernel(const double* __restrict__ cl,
                                                                      double* __restrict__ clinv,
                                                                      double* __restrict__ minpiv_part,
                                                                      double* __restrict__ logdet_part, int Vh,
                                                                      long nblk, int swz) {
  __shared__ double red[8];
  const long w = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long cp = w / nblk;                                       // 2 chain + parity
  const int blk = (int)(w % nblk);
  const int h0 = blk * kBlock + (int)threadIdx.x;
  const bool live = h0 < Vh;
  const int h = live ? h0 : 0;
  double mp = 1.7976931348623157e308, ls = 0.0;
#pragma unroll 1
  for (int chi = 0; chi < 2; ++chi) {
    const long off = (cp * 2 + chi) * (long)kCloverReals * Vh + h;
    clover_invert_block(cl + off, clinv + off, Vh, live, mp, ls);
  }
  const double bm = block_min(live ? mp : 1.7976931348623157e308, red);
  if (threadIdx.x == 0) minpiv_part[cp * nblk + blk] = bm;
  if (logdet_part != nullptr) {                                   // a kernel argument: the whole grid or none of it
    const double bl = block_sum(live ? ls : 0.0, red + 4);
    if (threadIdx.x == 0) logdet_part[cp * nblk + blk] = bl;
  }
}

// sgn, apbc, aux, part: as in su3_wilson_hop_eo_kernel, whose body this is up to the end of the direction loop.
template <int CMODE>
__global__ __launch_bounds__(kBlock, 2) void su3_wilson_clover_hop_eo_kernel(
    const double2* __restrict__ xn, const double2* __restrict__ src, const double2* aux, const double* __restrict__ cl,
    double2* out, double* __restrict__ part, double a, double bc, double sgn, int apbc, int parity, int nrhs, int T,
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
  double rr[12], ri[12];
  if (CMODE == 1) {                    // b (C aux) + a H src, one chirality at a time
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      double vr[6], vi[6], cr[6], ci[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) { cr[k] = 0.0; ci[k] = 0.0; }
      if (aux != nullptr) {            // a kernel argument: wave-uniform
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const double2 p = aux[off + (6 * ch + k) * Vh + hs];
          vr[k] = p.x; vi[k] = p.y;
        }
        clover_block_mul(cr, ci, clover_block(cl, b.c, parity, ch, Vh, hs), Vh, vr, vi);
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        rr[6 * ch + k] = aux != nullptr ? fma(a, ar[6 * ch + k], bc * cr[k]) : a * ar[6 * ch + k];
        ri[6 * ch + k] = aux != nullptr ? fma(a, ai[6 * ch + k], bc * ci[k]) : a * ai[6 * ch + k];
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      double re = a * ar[k], im = a * ai[k];
      if (aux != nullptr) {
        const double2 p = aux[off + k * Vh + hs];
        re = fma(a, ar[k], bc * p.x); im = fma(a, ai[k], bc * p.y);
      }
      if (CMODE == 2) { ar[k] = re; ai[k] = im; } else { rr[k] = re; ri[k] = im; }
    }
    if (CMODE == 2) {                  // C (b aux + a H src)
#pragma unroll
      for (int ch = 0; ch < 2; ++ch)
        clover_block_mul(rr + 6 * ch, ri + 6 * ch, clover_block(cl, b.c, parity, ch, Vh, hs), Vh, ar + 6 * ch,
                         ai + 6 * ch);
    }
  }
  double n2 = 0.0;
#pragma unroll
  for (int k = 0; k < 12; ++k) {       // every aux entry of this thread has been read: out may be aux
    if (live) out[off + k * Vh + hs] = make_double2(rr[k], ri[k]);
    n2 = fma(rr[k], rr[k], n2); n2 = fma(ri[k], ri[k], n2);
  }
  if (part != nullptr) {               // a kernel argument: the whole grid takes the barrier or none of it
    const double t = block_sum(live ? n2 : 0.0, red);
    if (threadIdx.x == 0) part[b.sys * nblk + b.blk] = t;
  }
}

// out = C src on the half field of `parity`; out may be src (a thread reads its twelve entries, then writes them)
__global__ __launch_bounds__(kBlock, 2) void su3_clover_apply_kernel(const double* __restrict__ cl, const double2* src,
                                                                     double2* out, double* __restrict__ part,
                                                                     int parity, int nrhs, int Vh, long nblk, int swz) {
  __shared__ double red[4];
  const WilsonBlock b = wilson_block(xcd_swizzle(blockIdx.x, (long)gridDim.x, swz), nrhs, nblk);
  const int h0 = b.blk * kBlock + (int)threadIdx.x;
  const bool live = h0 < Vh;
  const int hs = live ? h0 : 0;
  const long off = b.sys * 12L * Vh;
  double vr[12], vi[12], rr[12], ri[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const double2 p = src[off + k * Vh + hs];
    vr[k] = p.x; vi[k] = p.y;
  }
#pragma unroll
  for (int ch = 0; ch < 2; ++ch)
    clover_block_mul(rr + 6 * ch, ri + 6 * ch, clover_block(cl, b.c, parity, ch, Vh, hs), Vh, vr + 6 * ch, vi + 6 * ch);
  double n2 = 0.0;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    if (live) out[off + k * Vh + hs] = make_double2(rr[k], ri[k]);
    n2 = fma(rr[k], rr[k], n2); n2 = fma(ri[k], ri[k], n2);
  }
  if (part != nullptr) {
    const double t = block_sum(live ? n2 : 0.0, red);
    if (threadIdx.x == 0) part[b.sys * nblk + b.blk] = t;
  }
}

}  // namespace l2q

using namespace l2q;

extern "C" {

int l2q_su3_clover_term(const void* xn, void* cl, double coef, int nb, int T, int X, int Y, int Z, void* stream) {
  L2Q_REQUIRE(xn && cl, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(cl != xn, L2Q_EINVAL, "cl must not alias xn");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(coef - coef == 0.0, L2Q_EINVAL, "the coefficient coef = kappa c_sw must be finite");
  L2Q_REQUIRE(all_even(T, X, Y, Z), L2Q_ESHAPE, "the clover term needs even extents");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V, kBlock);
  hipLaunchKernelGGL(su3_clover_term_kernel, dim3((unsigned)(nb * nblk)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const double2*)xn, (double*)cl, coef, T, X, Y, Z, nblk, tuning().xcd_swizzle, 0);
  return check_launch("l2q_su3_clover_term");
}

int l2q_su3_clover_invert(const void* cl, void* clinv, double* minpiv_part, double* logdet_part, int nb, int T, int X,
                          int Y, int Z, void* stream) {
  L2Q_REQUIRE(cl && clinv && minpiv_part, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(clinv != cl && (const void*)minpiv_part != cl && (void*)minpiv_part != clinv &&
                  (logdet_part == nullptr || ((const void*)logdet_part != cl && (void*)logdet_part != clinv &&
                                              logdet_part != minpiv_part)),
              L2Q_EINVAL, "the outputs must not alias cl or each other");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(all_even(T, X, Y, Z), L2Q_ESHAPE, "the clover term needs even extents");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V / 2, kBlock);
  hipLaunchKernelGGL(su3_clover_invert_kernel, dim3((unsigned)(nb * 2 * nblk)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const double*)cl, (double*)clinv, minpiv_part, logdet_part, d.V / 2, nblk, tuning().xcd_swizzle);
  return check_launch("l2q_su3_clover_invert");
}

int l2q_su3_wilson_clover_hop_eo(const void* xn, const void* src, const void* aux, const void* c, void* out,
                                 double* norm_part, double a, double b, int flags, int parity, int cmode, int nb,
                                 int nrhs, int T, int X, int Y, int Z, void* stream) {
  L2Q_REQUIRE(xn && src && out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(cmode >= 0 && cmode <= 2, L2Q_EINVAL, "cmode must be 0 (no block), 1 (C on aux) or 2 (C on the result)");
  L2Q_REQUIRE((c != nullptr) == (cmode != 0), L2Q_EINVAL, "the block field c must be given with cmode 1 and 2, and only then");
  L2Q_REQUIRE(out != src && out != xn && out != c, L2Q_EINVAL, "out must not alias src, xn or c");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z) && nrhs > 0, L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(spinor_dims_ok((long)nb * nrhs, (long)T * X * Y * Z), L2Q_EINVAL,
              "size: nb * nrhs * 12 * V does not fit an int");
  L2Q_REQUIRE(a - a == 0.0 && b - b == 0.0, L2Q_EINVAL, "the coefficients a and b must be finite");
  L2Q_REQUIRE(flags >= 0 && flags <= 3, L2Q_EINVAL, "flags must be 0..3 (bit 0 dagger, bit 1 antiperiodic in t)");
  L2Q_REQUIRE(parity == 0 || parity == 1, L2Q_EINVAL, "parity must be 0 (even) or 1 (odd)");
  L2Q_REQUIRE(all_even(T, X, Y, Z), L2Q_ESHAPE, "a checkerboard update needs even extents");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V / 2, kBlock);
  const dim3 grid((unsigned)((long)nb * nrhs * nblk));
  const double sgn = (flags & 1) ? -1.0 : 1.0;
  const int apbc = (flags >> 1) & 1, swz = tuning().xcd_swizzle;
#define L2Q_CLOVER_HOP(M)                                                                                              \
  hipLaunchKernelGGL(su3_wilson_clover_hop_eo_kernel<M>, grid, dim3(kBlock), 0, (hipStream_t)stream,                   \
                     (const double2*)xn, (const double2*)src, (const double2*)aux, (const double*)c, (double2*)out,   \
                     norm_part, a, b, sgn, apbc, parity, nrhs, T, X, Y, Z, nblk, swz)
  if (cmode == 0) L2Q_CLOVER_HOP(0);
  else if (cmode == 1) L2Q_CLOVER_HOP(1);
  else L2Q_CLOVER_HOP(2);
#undef L2Q_CLOVER_HOP
  return check_launch("l2q_su3_wilson_clover_hop_eo");
}

int l2q_su3_clover_apply(const void* c, const void* src, void* out, double* norm_part, int parity, int nb, int nrhs,
                         int T, int X, int Y, int Z, void* stream) {
  L2Q_REQUIRE(c && src && out, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(out != c, L2Q_EINVAL, "out must not alias c");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z) && nrhs > 0, L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(spinor_dims_ok((long)nb * nrhs, (long)T * X * Y * Z), L2Q_EINVAL,
              "size: nb * nrhs * 12 * V does not fit an int");
  L2Q_REQUIRE(parity == 0 || parity == 1, L2Q_EINVAL, "parity must be 0 (even) or 1 (odd)");
  L2Q_REQUIRE(all_even(T, X, Y, Z), L2Q_ESHAPE, "a checkerboard update needs even extents");
  const Dims d = make_dims(T, X, Y, Z);
  const long nblk = cdiv(d.V / 2, kBlock);
  hipLaunchKernelGGL(su3_clover_apply_kernel, dim3((unsigned)((long)nb * nrhs * nblk)), dim3(kBlock), 0,
                     (hipStream_t)stream, (const double*)c, (const double2*)src, (double2*)out, norm_part, parity, nrhs,
                     d.V / 2, nblk, tuning().xcd_swizzle);
  return check_launch("l2q_su3_clover_apply");
}

}  // extern "C"
