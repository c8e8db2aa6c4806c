// su3_clover_force.hip -- the clover part of the force of two flavours of dynamical clover (Sheikholeslami-Wohlert)
// quarks on the links, in the asymmetric even-odd form (Jansen & Liu 1997):
//   S_f = sum_r phi_e,r^H (Mhat^H Mhat)^-1 phi_e,r - 2 npf log det A_oo,   Mhat = A_ee - kappa^2 H_eo A_oo^-1 H_oe.
// With X_e = (Mhat^H Mhat)^-1 phi_e, Y_e = Mhat X_e completed by X_o = kappa A_oo^-1 H_oe X_e, Y_o = kappa A_oo^-1
// (H^H)_oe Y_e,
//   dS_pf  = 2 kappa Re[Y^H dH X] - 2 Re sum_x Y(x)^H dA(x) X(x),     dS_det = -2 npf sum_{x odd} tr[A^-1(x) dA(x)],
//   dA(x)  = kappa c_sw i sum_{mu<nu} sigma_{mu nu} (x) dFhat_{mu nu}(x).
// The hop part is l2q_su3_wilson_force on (X, Y).  The rest, this file, is -2 kappa c_sw sum_x sum_{mu<nu} Re tr[dFhat_{mu
// nu}(x) Lambda_{mu nu}(x)] with (a b^H the colour outer product summed over spin)
//   Lambda_{mu nu}(x) = i sum_r (sigma_{mu nu} X_r)(x) Y_r(x)^H + [x odd] det_weight i tr_spin[sigma_{mu nu} A^-1(x)].
// Fhat = (Q - Q^H) / 8 keeps its trace, so Re tr(Lambda dFhat) = 1/4 Re tr(Lambda_AH dQ), Lambda_AH = (Lambda - Lambda^H)
// / 2 with its trace: dS = sum Re tr(G dQ), G = -(kappa c_sw / 2) Lambda_AH, the per-site field of su3_clover_insert.hpp.
//
// In the chiral basis sigma_{0k} = diag(-sigma_k, sigma_k) and sigma_{ij} = -eps_{ijk} diag(sigma_k, sigma_k).  Per
// chirality the Hermitian 6 x 6 matrix (index 3 spin + colour within the chirality, the layout of a clover block)
//   h = 2 det_weight A^-1 [x odd] + sum_r (X_r Y_r^H + Y_r X_r^H)
// holds all that enters: with U its upper right 3 x 3 block and h_ss its diagonal ones, the Hermitian colour matrices
//   S_1 = U + U^H,   S_2 = i (U - U^H),   S_3 = h_00 - h_11
// give i S_k = 2 AH(i sum sigma_k ...) and
//   G_{0k} = (kappa c_sw / 4) i (S_k[up] - S_k[dn]),   G_{dual k} = (kappa c_sw / 4) e_k i (S_k[up] + S_k[dn]),
// up the chirality of spin 0, 1, e = (+, -, +) for the planes (23), (13), (12).
//
// Two kernels, both gathers, no atomics:
//   1. su3_clover_force_g_kernel: one thread per (chain, site), site-local: npf * 384 B of spinors and, on odd sites, the
//      two blocks of A^-1 (2 x 288 B) in, 432 B of G out.  The sum over r runs in its order inside the thread.
//   2. su3_clover_force_link_kernel: one thread per link, clover_insert_link with no staple term, then
//      f_out = (f_in ? f_in : 0) + coef F, F = -TAH(U B) stored exactly anti-Hermitian (store_tah_axpy).
// A thread's arithmetic depends on its chain, its site or link and the lattice only: a chain gives the same bits alone
// and in a batch, and from run to run.
#include "su3_clover_block.hpp"
#include "su3_clover_insert.hpp"

namespace l2q {

// h += x y^H + y x^H for the six components (re, im) of one chirality of X and Y, in the 36 reals of a clover block
__device__ __forceinline__ void clover_herm_outer_acc(double* __restrict__ h, const double* xr, const double* xi,
                                                      const double* yr, const double* yi) {
#pragma unroll
  for (int i = 0; i < 6; ++i) h[i] = fma(2.0 * xr[i], yr[i], fma(2.0 * xi[i], yi[i], h[i]));
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i + 1; j < 6; ++j) {
      const int e = 6 + 2 * clover_upper(i, j);
      double re = h[e], im = h[e + 1];
      re = fma(xr[i], yr[j], re); re = fma(xi[i], yi[j], re); re = fma(yr[i], xr[j], re); re = fma(yi[i], xi[j], re);
      im = fma(xi[i], yr[j], im); im = fma(-xr[i], yi[j], im); im = fma(yi[i], xr[j], im); im = fma(-yr[i], xi[j], im);
      h[e] = re; h[e + 1] = im;
    }
}

// i S_k of the Hermitian 6 x 6 matrix h as an AH3 (d = the diagonal of S_k, (re, im) = (-Im, Re) of its entries above it)
template <int K>
__device__ __forceinline__ AH3 clover_sigma_part(const double* __restrict__ h) {
  AH3 o;
  if (K == 3) {
#pragma unroll
    for (int b = 0; b < 3; ++b) o.d[b] = h[b] - h[3 + b];
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int a = b + 1; a < 3; ++a) {
        const int e = b + a - 1, u = 6 + 2 * clover_upper(b, a), l = 6 + 2 * clover_upper(3 + b, 3 + a);
        o.re[e] = -(h[u + 1] - h[l + 1]); o.im[e] = h[u] - h[l];
      }
    return o;
  }
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const int u = 6 + 2 * clover_upper(b, 3 + b);
    o.d[b] = K == 1 ? 2.0 * h[u] : -2.0 * h[u + 1];
  }
#pragma unroll
  for (int b = 0; b < 3; ++b)
#pragma unroll
    for (int a = b + 1; a < 3; ++a) {
      const int e = b + a - 1, ba = 6 + 2 * clover_upper(b, 3 + a), ab = 6 + 2 * clover_upper(a, 3 + b);
      if (K == 1) {            // S = U_ba + conj(U_ab)
        o.re[e] = -(h[ba + 1] - h[ab + 1]); o.im[e] = h[ba] + h[ab];
      } else {                 // S = i (U_ba - conj(U_ab))
        o.re[e] = -(h[ba] - h[ab]); o.im[e] = -(h[ba + 1] + h[ab + 1]);
      }
    }
  return o;
}

// G_{0k} and its dual plane from the two chiralities
template <int K>
__device__ __forceinline__ void clover_force_g_store(double* __restrict__ gc, int V, int s, const double* hu,
                                                     const double* hd, double cf) {
  const AH3 su = clover_sigma_part<K>(hu), sd = clover_sigma_part<K>(hd);
  const double e = K == 2 ? -cf : cf;
  store_ah3(gc + (2 * (K - 1)) * 9L * V, V, s, ah3_comb(cf, su, -cf, sd));
  store_ah3(gc + (2 * (K - 1) + 1) * 9L * V, V, s, ah3_comb(e, su, e, sd));
}

// ------------------------------------------------------------------ pass 1: G
// cf = kappa c_sw / 4, dw2 = 2 det_weight; xs, ys null with npf = 0; clinv may be null
__global__ __launch_bounds__(kBlock, 2) void su3_clover_force_g_kernel(const double2* __restrict__ xs,
                                                                      const double2* __restrict__ ys,
                                                                      const double* __restrict__ clinv, double cf,
                                                                      double dw2, int npf, int V, int X, int Y, int Z,
                                                                      long nblk, int swz, double* __restrict__ gw) {
  const long wk = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const long c = wk / nblk, blk = wk % nblk;
  const int s = (int)blk * kBlock + (int)threadIdx.x;
  if (s >= V) return;                                             // no barrier in this kernel
  const int Vh = V / 2;
  const int par = (s + s / Z + s / (Y * Z) + s / (X * Y * Z)) & 1;     // (t + x + y + z) & 1: the extents are even
  double h[2][kCloverReals];
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    if (clinv != nullptr && par == 1) {
      const double* blkp = clover_block(clinv, c, 1, ch, Vh, s >> 1);
#pragma unroll
      for (int e = 0; e < kCloverReals; ++e) h[ch][e] = dw2 * blkp[e * Vh];
    } else {
#pragma unroll
      for (int e = 0; e < kCloverReals; ++e) h[ch][e] = 0.0;
    }
  }
#pragma unroll 1
  for (int r = 0; r < npf; ++r) {
    const double2* xr_ = xs + (c * npf + r) * 12L * V + s;
    const double2* yr_ = ys + (c * npf + r) * 12L * V + s;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      double xr[6], xi[6], yr[6], yi[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const double2 p = xr_[(6 * ch + k) * (long)V], q = yr_[(6 * ch + k) * (long)V];
        xr[k] = p.x; xi[k] = p.y; yr[k] = q.x; yi[k] = q.y;
      }
      clover_herm_outer_acc(h[ch], xr, xi, yr, yi);
    }
  }
  double* gc = gw + c * (long)kCloverGReals * V;
  clover_force_g_store<1>(gc, V, s, h[0], h[1], cf);
  clover_force_g_store<2>(gc, V, s, h[0], h[1], cf);
  clover_force_g_store<3>(gc, V, s, h[0], h[1], cf);
}

// ------------------------------------------------------------------ pass 2: one thread per link
// mu comes from the block index, so it is wave-uniform; cf = -coef; fin may be null or fout
__global__ __launch_bounds__(kBlock, 2) void su3_clover_force_link_kernel(const double2* __restrict__ xn,
                                                                         const double* __restrict__ gw,
                                                                         const double2* fin, double2* fout, double cf,
                                                                         int T, int X, int Y, int Z, long nblk,
                                                                         int swz) {
  const Dims d{T, X, Y, Z, T * X * Y * Z};
  const long wk = xcd_swizzle(blockIdx.x, (long)gridDim.x, swz);
  const int mu = (int)(wk & 3);
  const long cb = wk >> 2;
  const long c = cb / nblk, blk = cb % nblk;
  const int s = (int)blk * kBlock + (int)threadIdx.x;
  if (s >= d.V) return;
  const int V = d.V;
  const double2* xc = xn + c * 36L * V;
  M3 acc;
  clover_insert_link(acc, xc, gw + c * (long)kCloverGReals * V, 0.0, d, s, mu);
  M3 u, w;
  load_link(u, xc + mu * 9 * V, V, site_after(s, acc.im[8]));
  m3_mul_nn(w, u, acc);
  const long link = (c * 4 + mu) * 9L * V;
  store_tah_axpy(fin ? fin + link : nullptr, fout + link, V, s, cf, w);
}

}  // namespace l2q

using namespace l2q;

extern "C" {

int l2q_su3_clover_force(const void* xn, const void* X, const void* Y, const void* clinv, const void* f_in, void* f_out,
                         double kc, double coef, double det_weight, int nb, int npf, int T, int X_, int Y_, int Z, void* ws,
                         size_t ws_bytes, void* stream) {
  L2Q_REQUIRE(xn && f_out && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE((X != nullptr) == (npf > 0) && (Y != nullptr) == (npf > 0) && npf >= 0, L2Q_EINVAL,
              "X and Y go with npf > 0 and only with it (null pointer or npf)");
  L2Q_REQUIRE(npf > 0 || clinv != nullptr, L2Q_EINVAL,
              "both halves absent: need the fields X, Y (npf > 0), the blocks clinv, or both");
  L2Q_REQUIRE(f_out != xn && f_out != X && f_out != Y && f_out != clinv && f_out != ws, L2Q_EINVAL,
              "f_out must not alias xn, X, Y, clinv or ws");
  L2Q_REQUIRE(ws != xn && ws != X && ws != Y && ws != clinv && ws != f_in, L2Q_EINVAL,
              "ws must not alias xn, X, Y, clinv or f_in");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X_, Y_, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(npf == 0 || spinor_dims_ok((long)nb * npf, (long)T * X_ * Y_ * Z), L2Q_EINVAL,
              "size: nb * npf * 12 * V does not fit an int");
  L2Q_REQUIRE(kc - kc == 0.0 && coef - coef == 0.0 && det_weight - det_weight == 0.0, L2Q_EINVAL,
              "kc = kappa c_sw, coef and det_weight must be finite");
  const Dims d = make_dims(T, X_, Y_, Z);
  L2Q_REQUIRE(ws_bytes >= (size_t)nb * kCloverGReals * (size_t)d.V * sizeof(double), L2Q_EINVAL, "workspace too small");
  L2Q_REQUIRE(all_even(T, X_, Y_, Z), L2Q_ESHAPE, "the clover force needs even extents");
  const long nblk = cdiv(d.V, kBlock);
  hipStream_t st = (hipStream_t)stream;
  const int swz = tuning().xcd_swizzle;
  hipLaunchKernelGGL(su3_clover_force_g_kernel, dim3((unsigned)(nb * nblk)), dim3(kBlock), 0, st, (const double2*)X,
                     (const double2*)Y, (const double*)clinv, 0.25 * kc, 2.0 * det_weight, npf, d.V, X_, Y_, Z, nblk, swz,
                     (double*)ws);
  hipLaunchKernelGGL(su3_clover_force_link_kernel, dim3((unsigned)(nb * nblk * 4)), dim3(kBlock), 0, st,
                     (const double2*)xn, (const double*)ws, (const double2*)f_in, (double2*)f_out, -coef, T, X_, Y_, Z,
                     nblk, swz);
  return check_launch("l2q_su3_clover_force");
}

}  // extern "C"
