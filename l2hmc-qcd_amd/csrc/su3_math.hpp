// su3_math.hpp -- register-resident 3x3 complex fp64 algebra for gfx950 device code.
//
// Everything here is per-lane: one lane owns one 3x3 complex matrix (18 doubles = 36 VGPRs).
// Formulae follow the reference's PyTorch expressions so that results agree to rounding:
//   projectSU / eigs3x3 / rsqrtPHM3f : src/l2hmc/group/su3/pytorch/utils.py:227-346
//   projectTAH                        : src/l2hmc/group/su3/pytorch/group.py:92-103
//   su3_to_vec                        : src/l2hmc/group/su3/pytorch/utils.py:394-420
//   matrix_exp (torch library call)   : src/l2hmc/group/su3/pytorch/group.py:45-50
#pragma once
#include <hip/hip_runtime.h>

namespace l2q {

struct M3 {
  double re[9];
  double im[9];
};

__device__ __forceinline__ void m3_zero(M3& a) {
#pragma unroll
  for (int i = 0; i < 9; ++i) { a.re[i] = 0.0; a.im[i] = 0.0; }
}

__device__ __forceinline__ void m3_identity(M3& a) {
  m3_zero(a);
  a.re[0] = a.re[4] = a.re[8] = 1.0;
}

// C = A * B
__device__ __forceinline__ void m3_mul_nn(M3& c, const M3& a, const M3& b) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double ar = a.re[3 * i + k], ai = a.im[3 * i + k];
        const double br = b.re[3 * k + j], bi = b.im[3 * k + j];
        sr = fma(ar, br, sr); sr = fma(-ai, bi, sr);
        si = fma(ar, bi, si); si = fma(ai, br, si);
      }
      c.re[3 * i + j] = sr; c.im[3 * i + j] = si;
    }
}

// C = A * B^H
__device__ __forceinline__ void m3_mul_na(M3& c, const M3& a, const M3& b) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double ar = a.re[3 * i + k], ai = a.im[3 * i + k];
        const double br = b.re[3 * j + k], bi = -b.im[3 * j + k];
        sr = fma(ar, br, sr); sr = fma(-ai, bi, sr);
        si = fma(ar, bi, si); si = fma(ai, br, si);
      }
      c.re[3 * i + j] = sr; c.im[3 * i + j] = si;
    }
}

// C = A^H * B
__device__ __forceinline__ void m3_mul_an(M3& c, const M3& a, const M3& b) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double ar = a.re[3 * k + i], ai = -a.im[3 * k + i];
        const double br = b.re[3 * k + j], bi = b.im[3 * k + j];
        sr = fma(ar, br, sr); sr = fma(-ai, bi, sr);
        si = fma(ar, bi, si); si = fma(ai, br, si);
      }
      c.re[3 * i + j] = sr; c.im[3 * i + j] = si;
    }
}

// C = A^H * B^H
__device__ __forceinline__ void m3_mul_aa(M3& c, const M3& a, const M3& b) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double ar = a.re[3 * k + i], ai = -a.im[3 * k + i];
        const double br = b.re[3 * j + k], bi = -b.im[3 * j + k];
        sr = fma(ar, br, sr); sr = fma(-ai, bi, sr);
        si = fma(ar, bi, si); si = fma(ai, br, si);
      }
      c.re[3 * i + j] = sr; c.im[3 * i + j] = si;
    }
}

// acc += A * B^H
__device__ __forceinline__ void m3_mac_na(M3& c, const M3& a, const M3& b) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double sr = c.re[3 * i + j], si = c.im[3 * i + j];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double ar = a.re[3 * i + k], ai = a.im[3 * i + k];
        const double br = b.re[3 * j + k], bi = -b.im[3 * j + k];
        sr = fma(ar, br, sr); sr = fma(-ai, bi, sr);
        si = fma(ar, bi, si); si = fma(ai, br, si);
      }
      c.re[3 * i + j] = sr; c.im[3 * i + j] = si;
    }
}

// acc += A * B
__device__ __forceinline__ void m3_mac_nn(M3& c, const M3& a, const M3& b) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double sr = c.re[3 * i + j], si = c.im[3 * i + j];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double ar = a.re[3 * i + k], ai = a.im[3 * i + k];
        const double br = b.re[3 * k + j], bi = b.im[3 * k + j];
        sr = fma(ar, br, sr); sr = fma(-ai, bi, sr);
        si = fma(ar, bi, si); si = fma(ai, br, si);
      }
      c.re[3 * i + j] = sr; c.im[3 * i + j] = si;
    }
}

// tr( Y * (A * B)^H ) accumulated into (sr, si) without materialising A * B
__device__ __forceinline__ void m3_trace_y_abh(double& sr, double& si, const M3& y, const M3& a,
                                               const M3& b) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double pr = 0.0, pi = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double ar = a.re[3 * i + k], ai = a.im[3 * i + k];
        const double br = b.re[3 * k + j], bi = b.im[3 * k + j];
        pr = fma(ar, br, pr); pr = fma(-ai, bi, pr);
        pi = fma(ar, bi, pi); pi = fma(ai, br, pi);
      }
      const double yr = y.re[3 * i + j], yi = y.im[3 * i + j];
      sr = fma(yr, pr, sr); sr = fma(yi, pi, sr);
      si = fma(yi, pr, si); si = fma(-yr, pi, si);
    }
}

__device__ __forceinline__ void m3_add(M3& a, const M3& b) {
#pragma unroll
  for (int i = 0; i < 9; ++i) { a.re[i] += b.re[i]; a.im[i] += b.im[i]; }
}

// tr(A * B^H) = sum_ij A_ij conj(B_ij)
__device__ __forceinline__ void m3_trace_mul_na(double& tr, double& ti, const M3& a, const M3& b) {
  double sr = 0.0, si = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    sr = fma(a.re[i], b.re[i], sr); sr = fma(a.im[i], b.im[i], sr);
    si = fma(a.im[i], b.re[i], si); si = fma(-a.re[i], b.im[i], si);
  }
  tr = sr; ti = si;
}

__device__ __forceinline__ void cmul(double& cr, double& ci, double ar, double ai, double br,
                                     double bi) {
  cr = ar * br - ai * bi;
  ci = ar * bi + ai * br;
}

// det by cofactor expansion along the first row
__device__ __forceinline__ void m3_det(double& dr, double& di, const M3& m) {
  double t0r, t0i, t1r, t1i, ar, ai, br, bi;
  // m00 * (m11 m22 - m12 m21)
  cmul(ar, ai, m.re[4], m.im[4], m.re[8], m.im[8]);
  cmul(br, bi, m.re[5], m.im[5], m.re[7], m.im[7]);
  cmul(t0r, t0i, m.re[0], m.im[0], ar - br, ai - bi);
  // m01 * (m10 m22 - m12 m20)
  cmul(ar, ai, m.re[3], m.im[3], m.re[8], m.im[8]);
  cmul(br, bi, m.re[5], m.im[5], m.re[6], m.im[6]);
  cmul(t1r, t1i, m.re[1], m.im[1], ar - br, ai - bi);
  dr = t0r - t1r; di = t0i - t1i;
  // m02 * (m10 m21 - m11 m20)
  cmul(ar, ai, m.re[3], m.im[3], m.re[7], m.im[7]);
  cmul(br, bi, m.re[4], m.im[4], m.re[6], m.im[6]);
  cmul(t0r, t0i, m.re[2], m.im[2], ar - br, ai - bi);
  dr += t0r; di += t0i;
}

// R = (X - X^H)/2 - tr(X - X^H)/6 * I      (group.py:92-103)
__device__ __forceinline__ void m3_tah(M3& r, const M3& x) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      r.re[3 * i + j] = 0.5 * (x.re[3 * i + j] - x.re[3 * j + i]);
      r.im[3 * i + j] = 0.5 * (x.im[3 * i + j] + x.im[3 * j + i]);
    }
  const double dr = (r.re[0] + r.re[4] + r.re[8]) / 3.0;
  const double di = (r.im[0] + r.im[4] + r.im[8]) / 3.0;
  r.re[0] -= dr; r.re[4] -= dr; r.re[8] -= dr;
  r.im[0] -= di; r.im[4] -= di; r.im[8] -= di;
}

// Upper-plane form of an anti-Hermitian field (the force as its kernel stores it): of the nine planes only the
// diagonal and the i < j ones are kept, as six planes in the order e = 0, 4, 8, 1, 2, 5; plane (j, i) is
// (-re, im) of plane (i, j).  up_plane: entry e -> its plane, -1 for the three that are not stored.
__device__ __forceinline__ constexpr int up_entry(int p) { return p < 3 ? 4 * p : p == 3 ? 1 : p == 4 ? 2 : 5; }
__device__ __forceinline__ constexpr int up_plane(int e) {
  return e == 0 ? 0 : e == 4 ? 1 : e == 8 ? 2 : e == 1 ? 3 : e == 2 ? 4 : e == 5 ? 5 : -1;
}
// The full matrix from its six stored entries.  Where the two real parts of a transposed pair coincide the force
// kernel writes the SAME signed zero into both planes (0.5 * (a - a) on either side), so a zero keeps its sign.
__device__ __forceinline__ void m3_from_upper(M3& x, const double2 (&u)[6]) {
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    const int e = up_entry(p), et = 3 * (e % 3) + e / 3;
    x.re[e] = u[p].x; x.im[e] = u[p].y;
    if (et != e) { x.re[et] = u[p].x == 0.0 ? u[p].x : -u[p].x; x.im[et] = u[p].y; }
  }
}

// exp(A) for a general complex 3x3 A.  Scaling & squaring; the scaled exponential is summed
// through the Cayley-Hamilton recursion A^(n+1) = p0 A^(n-2) - p1 A^(n-1) + p2 A^n carried
// on the three scalar coefficients of {I, A, A^2}, so it costs one matmul (A^2), 20 scalar
// recursion steps and s squarings.
__device__ __forceinline__ void m3_expm(M3& out, const M3& ain) {
  double n2 = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) n2 += ain.re[i] * ain.re[i] + ain.im[i] * ain.im[i];
  const double nrm = sqrt(n2);                       // Frobenius >= spectral norm
  int s = 0;
  double scale = 1.0;
  if (nrm > 0.5) {
    int ex;
    (void)frexp(nrm, &ex);                           // nrm = f * 2^ex, f in [0.5, 1)
    s = ex + 1;                                      // nrm / 2^s in [0.25, 0.5)
    if (s > 60) s = 60;
    scale = ldexp(1.0, -s);
  }
  M3 a;
#pragma unroll
  for (int i = 0; i < 9; ++i) { a.re[i] = ain.re[i] * scale; a.im[i] = ain.im[i] * scale; }
  M3 a2;
  m3_mul_nn(a2, a, a);
  // characteristic polynomial  A^3 = p2 A^2 - p1 A + p0 I
  const double p2r = a.re[0] + a.re[4] + a.re[8], p2i = a.im[0] + a.im[4] + a.im[8];
  const double t2r = a2.re[0] + a2.re[4] + a2.re[8], t2i = a2.im[0] + a2.im[4] + a2.im[8];
  double sqr, sqi;
  cmul(sqr, sqi, p2r, p2i, p2r, p2i);
  const double p1r = 0.5 * (sqr - t2r), p1i = 0.5 * (sqi - t2i);
  double p0r, p0i;
  m3_det(p0r, p0i, a);
  // coefficients of A^n / n!  on {I, A, A^2}
  double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0, cr = 0.5, ci = 0.0;   // n = 2: A^2/2
  double f0r = 1.0, f0i = 0.0, f1r = 1.0, f1i = 0.0, f2r = 0.5, f2i = 0.0;
  // 1 / (n + 1) from a table of correctly rounded constants (scalar loads): written as a division the rolled
  // loop carries an IEEE fp64 division sequence per step (13 of its ~45 instructions), and fully unrolled the
  // kernels that inline this go from 158 to 168 VGPRs and spill
#ifndef L2Q_EXPM_DIV
#define L2Q_EXPM_DIV 0
#endif
  static constexpr double kInv[22] = {
      1.0 / 1, 1.0 / 2, 1.0 / 3, 1.0 / 4, 1.0 / 5, 1.0 / 6, 1.0 / 7, 1.0 / 8, 1.0 / 9, 1.0 / 10, 1.0 / 11,
      1.0 / 12, 1.0 / 13, 1.0 / 14, 1.0 / 15, 1.0 / 16, 1.0 / 17, 1.0 / 18, 1.0 / 19, 1.0 / 20, 1.0 / 21, 1.0 / 22};
  // Early exit, same bits as all 20 steps.  With |a|_F <= 0.5 the eigenvalues obey sum |l_i|^2 <= 1/4, hence
  // |p2| <= 0.87, |p1| <= 0.25, |p0| <= 0.025, and one step maps S = |a_n| + |b_n| + |c_n| (moduli) to
  //   S' <= (|c| |p0| + |a| + |c| |p1| + |b| + |c| |p2|) / (n + 1) <= 1.14 S / (n + 1) <= 0.29 S      (n + 1 >= 4
  // for every step after the first), the roundings of a step adding a few 2^-53 relative to the same sums of
  // moduli.  So once T = sum of the six |components| (>= S) satisfies 2^53 T <= |f| for each of the six real
  // sums f, every later term component t has |t| <= 0.29 T < 2^-54 |f|, less than half the gap from f to either
  // neighbour: f + t rounds to f, f never moves again and the induction carries to step 20.  A sum that is
  // exactly zero (a real matrix: all imaginary parts) is passed only by T == 0, after which all terms stay zero.
  // A NaN fails every comparison and runs all steps; so does the capped scaling (|a|_F may exceed 0.5 there,
  // `big` = +inf), and an infinite or NaN norm.
#ifndef L2Q_EXPM_EARLY_EXIT
#define L2Q_EXPM_EARLY_EXIT 1
#endif
#ifndef L2Q_EXPM_TEST_EVERY
#define L2Q_EXPM_TEST_EVERY 2
#endif
  const double big = nrm < 0x1p59 ? 0x1p53 : HUGE_VAL;
#ifdef L2Q_EXPM_COUNT_STEPS
  int steps = 0;
#endif
#pragma unroll 1
  for (int n = 2; n < 22; ++n) {
    const double inv = L2Q_EXPM_DIV ? 1.0 / (double)(n + 1) : kInv[n];
    double xr, xi, yr, yi, zr, zi;
    cmul(xr, xi, cr, ci, p0r, p0i);                  // c p0
    cmul(yr, yi, cr, ci, p1r, p1i);                  // c p1
    cmul(zr, zi, cr, ci, p2r, p2i);                  // c p2
    const double nar = xr * inv, nai = xi * inv;
    const double nbr = (ar - yr) * inv, nbi = (ai - yi) * inv;
    const double ncr = (br + zr) * inv, nci = (bi + zi) * inv;
    ar = nar; ai = nai; br = nbr; bi = nbi; cr = ncr; ci = nci;
    f0r += ar; f0i += ai; f1r += br; f1i += bi; f2r += cr; f2i += ci;
#ifdef L2Q_EXPM_COUNT_STEPS
    ++steps;
#endif
    // (tested after every second step, the first included -- a uniform branch on n skips the 12 instructions of
    // the test on the others: an exit one step late adds a term that moves no sum, by the argument above)
    if (L2Q_EXPM_EARLY_EXIT && (L2Q_EXPM_TEST_EVERY == 1 || (n & 1) == 0)) {
      const double tt = big * (((fabs(ar) + fabs(ai)) + (fabs(br) + fabs(bi))) + (fabs(cr) + fabs(ci)));
      if ((tt <= fabs(f0r)) & (tt <= fabs(f0i)) & (tt <= fabs(f1r)) & (tt <= fabs(f1i)) & (tt <= fabs(f2r)) &
          (tt <= fabs(f2i)))
        break;
    }
  }
#ifdef L2Q_EXPM_COUNT_STEPS
  L2Q_EXPM_COUNT_STEPS(steps);
#endif
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    double xr, xi, yr, yi;
    cmul(xr, xi, f1r, f1i, a.re[i], a.im[i]);
    cmul(yr, yi, f2r, f2i, a2.re[i], a2.im[i]);
    out.re[i] = xr + yr; out.im[i] = xi + yi;
  }
  out.re[0] += f0r; out.re[4] += f0r; out.re[8] += f0r;
  out.im[0] += f0i; out.im[4] += f0i; out.im[8] += f0i;
#pragma unroll 1
  for (int k = 0; k < s; ++k) {
    M3 t;
    m3_mul_nn(t, out, out);
    out = t;
  }
}

// The routines from here to m3_project_su_vec8 (the projection) are inlined into several kernels that must give each other's
// bits (the vec8 and the digit producers): every fused multiply-add in them is written out and the compiler is
// told not to form others, so that no kernel's schedule decides which product of a sum gets fused.
#if defined(__clang__)
#define L2Q_FP_AS_WRITTEN _Pragma("clang fp contract(off)")
#else
#define L2Q_FP_AS_WRITTEN
#endif

// The projection's transcendentals, reciprocals and roots on the ranges it calls them on (L2Q_RANGED_MATH 0: the
// library calls, divisions and square roots as before -- A/B builds).
#ifndef L2Q_RANGED_MATH
#define L2Q_RANGED_MATH 1
#endif

// hardware estimates of 1 / x and x^(-1/2) (v_rcp_f64, v_rsq_f64: 2^29 ulp = 2^-23 relative; 0 -> inf, inf -> 0).  The
// host build of the tests has no such instruction: the correctly rounded value cut to 24 bits stands in.
__device__ __forceinline__ double m_cut24(double y) {
  if (!(fabs(y) <= 1.7976931348623157e308) || y == 0.0) return y;
  int ex;
  const double f = frexp(y, &ex);
  return ldexp((double)(long)(f * 16777216.0), ex - 24);
}
__device__ __forceinline__ double m_rcp_est(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rcp(x);
#else
  return m_cut24(1.0 / x);
#endif
}
__device__ __forceinline__ double m_rsq_est(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rsq(x);
#else
  return m_cut24(1.0 / sqrt(x));
#endif
}

// 1 / x: three Newton steps on the estimate (relative error 2^-23 -> 2^-46 -> 2^-92, the third step is
// the residual correction of a division: the result is the correctly rounded reciprocal or its neighbour).
// x = 0, +-inf and NaN give what the division gives (the residual 1 - x y is NaN exactly there: 0 inf).
__device__ __forceinline__ double m_rcp(double x) {
  L2Q_FP_AS_WRITTEN
  const double y0 = m_rcp_est(x);
  const double e0 = fma(-x, y0, 1.0);
  double y = fma(e0, y0, y0);
  y = fma(fma(-x, y, 1.0), y, y);
  y = fma(fma(-x, y, 1.0), y, y);
  return e0 == e0 ? y : y0;
}

// g = sqrt(x), h = 1 / (2 sqrt(x)) for x >= 0: two coupled Newton steps on (x y, y / 2), y the estimate of
// x^(-1/2) (2^-23 -> 2^-45 -> 2^-89), then the residual correction x - g^2 of the root.  x = 0: g = 0,
// h = +inf, as sqrt and the division give (the estimate is inf there and 0 inf a NaN).
__device__ __forceinline__ void m_sqrt_hrsq(double& g, double& h, double x) {
  L2Q_FP_AS_WRITTEN
  const double y = m_rsq_est(x);
  double gg = x * y, hh = 0.5 * y;
  double r = fma(-gg, hh, 0.5);
  gg = fma(gg, r, gg); hh = fma(hh, r, hh);
  r = fma(-gg, hh, 0.5);
  gg = fma(gg, r, gg); hh = fma(hh, r, hh);
  gg = fma(fma(-gg, gg, x), hh, gg);
  const bool zero = x == 0.0;
  g = zero ? 0.0 : gg;
  h = zero ? HUGE_VAL : hh;
}
__device__ __forceinline__ double m_sqrt(double x) {
#if L2Q_RANGED_MATH
  double g, h;
  m_sqrt_hrsq(g, h, x);
  return g;
#else
  return sqrt(x);
#endif
}

// sin t and cos t for |t| <= pi / 3 (both call sites: a third of an acos, a third of an atan2).  Above pi / 4
// the argument is folded to u = pi / 2 - |t| in [pi / 6, pi / 4], held as uh + ul -- uh = pio2_hi - |t| is exact
// (Sterbenz), ul the low word of pi / 2, entering both series to first order as in fdlibm's kernels -- and the two
// series change places; no other reduction, no table, no integer work.  The series are the minimax polynomials of fdlibm's __kernel_sin / __kernel_cos on [-pi / 4, pi / 4]
// (error below 2^-58 and 2^-57 relative to sin and cos), cos summed as w + ((1 - w) - z / 2 + z^2 (...)) with
// w = 1 - z / 2 so that its leading terms round once: each result is within one ulp.
__device__ __forceinline__ void m_sincos_third(double t, double& s, double& c) {
  L2Q_FP_AS_WRITTEN
  const double a = fabs(t);
  const bool fold = a > 0.78539816339744828;
  const double u = fold ? 1.57079632679489655800e+00 - a : a;
  const double ul = fold ? 6.12323399573676603587e-17 : 0.0;
  const double z = u * u;
  double p = fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
  p = fma(z, p, 2.75573137070700676789e-06);
  p = fma(z, p, -1.98412698298579493134e-04);
  p = fma(z, p, 8.33333333332248946124e-03);
  p = fma(z, p, -1.66666666666666324348e-01);
  const double hz = 0.5 * z;
  const double w = 1.0 - hz;
  const double su = u + fma(ul, w, (z * u) * p);     // sin(uh + ul) = sin uh + ul cos uh
  double q = fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
  q = fma(z, q, -2.75573143513906633035e-07);
  q = fma(z, q, 2.48015872894767294178e-05);
  q = fma(z, q, -1.38888888888741095749e-03);
  q = fma(z, q, 4.16666666666666019037e-02);
  const double cu = w + fma(-u, ul, fma(z * z, q, (1.0 - w) - hz));   // cos(uh + ul) = cos uh - ul sin uh
  const double sa = fold ? cu : su;
  s = copysign(sa, t);
  c = fold ? su : cu;
}

// Closed-form eigenvalues of a 3x3 positive Hermitian matrix from (tr, tr(M^2), det).
// utils.py:227-283 (same clamps: +-3e38 on 1/q^1.5, acos argument to +-(1 - 1e-12)).
__device__ __forceinline__ void eigs3x3(double& e0, double& e1, double& e2, double tr, double p2,
                                        double det) {
  L2Q_FP_AS_WRITTEN
  const double tr3 = (1.0 / 3.0) * tr;
  const double p23 = (1.0 / 3.0) * p2;
  const double tr32 = tr3 * tr3;
  const double q = fabs(0.5 * (p23 - tr32));
  const double r = fma(0.25 * tr3, fma(5.0, tr32, -p2), -(0.5 * det));
#if L2Q_RANGED_MATH
  // sqrt(q) and 1 / (q sqrt(q)) from one reciprocal root: (2 h)^3 is within a few ulp of 1 / sq3, one Newton step on
  // sq3 itself takes it to the neighbourhood of the quotient (q = 0, a degenerate spectrum: +inf, clamped below)
  double sq, hq;
  m_sqrt_hrsq(sq, hq, q);
  const double sq3 = q * sq;
  const double iq = hq + hq;
  double isq3 = iq * iq * iq;
  const double eq = fma(-sq3, isq3, 1.0);
  isq3 = eq == eq ? fma(eq, isq3, isq3) : isq3;
#else
  const double sq = sqrt(q);
  const double sq3 = q * sq;
  double isq3 = 1.0 / sq3;
#endif
  isq3 = fmin(3e38, fmax(-3e38, isq3));
  double rsq3 = r * isq3;
  rsq3 = fmin(1.0, fmax(-1.0, rsq3));
  rsq3 = fmin(1.0 - 1e-12, fmax(-1.0 + 1e-12, rsq3));
  const double t = (1.0 / 3.0) * acos(rsq3);
  double st, ct;
#if L2Q_RANGED_MATH
  m_sincos_third(t, st, ct);                         // t in [0, pi / 3]
#else
  sincos(t, &st, &ct);
#endif
  const double sqc = sq * ct;
  const double sqs = 1.7320508075688772 * sq * st;
  const double ll = tr3 + sqc;
  e0 = fma(-2.0, sqc, tr3);
  e1 = ll + sqs;
  e2 = ll - sqs;
}

// A Hermitian 3x3 matrix held as what fixes it: the real diagonal and the upper triangle
// (o = 0: (0,1), 1: (0,2), 2: (1,2)); the lower triangle is the conjugate and is never formed.
struct H3 {
  double d[3];
  double re[3];
  double im[3];
};

// T = X^H X: the diagonal as column norms, the upper triangle with the sums of m3_mul_an
__device__ __forceinline__ void h3_gram(H3& t, const M3& x) {
  L2Q_FP_AS_WRITTEN
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { s = fma(x.re[3 * k + i], x.re[3 * k + i], s); s = fma(x.im[3 * k + i], x.im[3 * k + i], s); }
    t.d[i] = s;
  }
#pragma unroll
  for (int o = 0; o < 3; ++o) {
    const int i = o == 2 ? 1 : 0, j = o == 0 ? 1 : 2;
    double sr = 0.0, si = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double ar = x.re[3 * k + i], ai = -x.im[3 * k + i];
      const double br = x.re[3 * k + j], bi = x.im[3 * k + j];
      sr = fma(ar, br, sr); sr = fma(-ai, bi, sr);
      si = fma(ar, bi, si); si = fma(ai, br, si);
    }
    t.re[o] = sr; t.im[o] = si;
  }
}

// S = T T for Hermitian T (Hermitian again)
__device__ __forceinline__ void h3_square(H3& s, const H3& t) {
  L2Q_FP_AS_WRITTEN
  const double n01 = fma(t.re[0], t.re[0], t.im[0] * t.im[0]);
  const double n02 = fma(t.re[1], t.re[1], t.im[1] * t.im[1]);
  const double n12 = fma(t.re[2], t.re[2], t.im[2] * t.im[2]);
  s.d[0] = fma(t.d[0], t.d[0], n01 + n02);
  s.d[1] = fma(t.d[1], t.d[1], n01 + n12);
  s.d[2] = fma(t.d[2], t.d[2], n02 + n12);
  // (0,1) = (t00 + t11) t01 + t02 conj(t12)
  const double a01 = t.d[0] + t.d[1], a02 = t.d[0] + t.d[2], a12 = t.d[1] + t.d[2];
  s.re[0] = fma(a01, t.re[0], fma(t.re[1], t.re[2], t.im[1] * t.im[2]));
  s.im[0] = fma(a01, t.im[0], fma(t.im[1], t.re[2], -(t.re[1] * t.im[2])));
  // (0,2) = (t00 + t22) t02 + t01 t12
  s.re[1] = fma(a02, t.re[1], fma(t.re[0], t.re[2], -(t.im[0] * t.im[2])));
  s.im[1] = fma(a02, t.im[1], fma(t.re[0], t.im[2], t.im[0] * t.re[2]));
  // (1,2) = (t11 + t22) t12 + conj(t01) t02
  s.re[2] = fma(a12, t.re[2], fma(t.re[0], t.re[1], t.im[0] * t.im[1]));
  s.im[2] = fma(a12, t.im[2], fma(t.re[0], t.im[1], -(t.im[0] * t.re[1])));
}

// det of a Hermitian matrix (real): t00 t11 t22 + 2 Re(t01 t12 conj(t02)) - t00 |t12|^2 - t11 |t02|^2 - t22 |t01|^2
__device__ __forceinline__ double h3_det(const H3& t) {
  L2Q_FP_AS_WRITTEN
  const double n01 = fma(t.re[0], t.re[0], t.im[0] * t.im[0]);
  const double n02 = fma(t.re[1], t.re[1], t.im[1] * t.im[1]);
  const double n12 = fma(t.re[2], t.re[2], t.im[2] * t.im[2]);
  const double qr = fma(t.re[0], t.re[2], -(t.im[0] * t.im[2]));      // t01 t12
  const double qi = fma(t.re[0], t.im[2], t.im[0] * t.re[2]);
  const double tri = fma(qr, t.re[1], qi * t.im[1]);                  // Re(t01 t12 conj(t02))
  double det = t.d[0] * fma(t.d[1], t.d[2], -n12);
  det = fma(-t.d[1], n02, det);
  det = fma(-t.d[2], n01, det);
  return fma(2.0, tri, det);
}

// r = (x^H x)^(-1/2) as c0 + c1 t + c2 t^2, t = x^H x          utils.py:286-338
__device__ __forceinline__ void h3_rsqrt_gram(H3& r, const M3& x) {
  L2Q_FP_AS_WRITTEN
  H3 t, t2;
  h3_gram(t, x);
  h3_square(t2, t);
  const double tr = t.d[0] + t.d[1] + t.d[2];
  const double p2 = t2.d[0] + t2.d[1] + t2.d[2];
  const double det = h3_det(t);
  double e0, e1, e2;
  eigs3x3(e0, e1, e2, tr, p2, det);
  const double se0 = m_sqrt(fabs(e0)), se1 = m_sqrt(fabs(e1)), se2 = m_sqrt(fabs(e2));
  const double u = se0 + se1 + se2;
  const double w = se0 * se1 * se2;
  const double d = w * (se0 + se1) * (se0 + se2) * (se1 + se2);
  const double di = L2Q_RANGED_MATH ? m_rcp(d) : 1.0 / d;
  const double c0 = di * fma(e2 * se2, e0 + e1, fma(e1 * se1, e0 + e2, fma(e0 * se0, e1 + e2, w * u * u)));
  const double c1 = -fma(tr, u, w) * di;
  const double c2 = u * di;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    r.d[i] = fma(c2, t2.d[i], fma(c1, t.d[i], c0));
    r.re[i] = fma(c2, t2.re[i], c1 * t.re[i]);
    r.im[i] = fma(c2, t2.im[i], c1 * t.im[i]);
  }
}

// m3_det with its fused multiply-adds written out (m3_det itself is shared with m3_expm, whose bits are left as
// the compiler makes them)
__device__ __forceinline__ void m3_det_as_written(double& dr, double& di, const M3& m) {
  L2Q_FP_AS_WRITTEN
  auto mul = [](double& cr, double& ci, double ar, double ai, double br, double bi) {
    cr = fma(ar, br, -(ai * bi));
    ci = fma(ar, bi, ai * br);
  };
  double t0r, t0i, t1r, t1i, t2r, t2i, ar, ai, br, bi;
  mul(ar, ai, m.re[4], m.im[4], m.re[8], m.im[8]);
  mul(br, bi, m.re[5], m.im[5], m.re[7], m.im[7]);
  mul(t0r, t0i, m.re[0], m.im[0], ar - br, ai - bi);
  mul(ar, ai, m.re[3], m.im[3], m.re[8], m.im[8]);
  mul(br, bi, m.re[5], m.im[5], m.re[6], m.im[6]);
  mul(t1r, t1i, m.re[1], m.im[1], ar - br, ai - bi);
  mul(ar, ai, m.re[3], m.im[3], m.re[7], m.im[7]);
  mul(br, bi, m.re[4], m.im[4], m.re[6], m.im[6]);
  mul(t2r, t2i, m.re[2], m.im[2], ar - br, ai - bi);
  dr = (t0r - t1r) + t2r; di = (t0i - t1i) + t2i;
}

// entry (i, j) of X R, R Hermitian
__device__ __forceinline__ void m3_mul_h3_entry(double& sr, double& si, const M3& x, const H3& r, int i, int j) {
  L2Q_FP_AS_WRITTEN
  sr = x.re[3 * i + j] * r.d[j]; si = x.im[3 * i + j] * r.d[j];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k == j) continue;
    const int lo = k < j ? k : j, hi = k < j ? j : k, o = lo + hi - 1;
    const double br = r.re[o], bi = k < j ? r.im[o] : -r.im[o];    // r_kj: stored for k < j, its conjugate below
    const double ar = x.re[3 * i + k], ai = x.im[3 * i + k];
    sr = fma(ar, br, sr); sr = fma(-ai, bi, sr);
    si = fma(ar, bi, si); si = fma(ai, br, si);
  }
}

// m = x (x^H x)^(-1/2)                                 utils.py:286-338
__device__ __forceinline__ void m3_project_u(M3& m, const M3& x) {
  H3 r;
  h3_rsqrt_gram(r, x);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) m3_mul_h3_entry(m.re[3 * i + j], m.im[3 * i + j], x, r, i, j);
}

// out = projectU(x) * exp(-i arg(det)/3)                utils.py:341-346
__device__ __forceinline__ void m3_project_su(M3& out, const M3& x) {
  M3 m;
  m3_project_u(m, x);
  double detr, deti;
  m3_det(detr, deti, m);
  const double p = (-1.0 / 3.0) * atan2(deti, detr);
  double sp, cp;
#if L2Q_RANGED_MATH
  m_sincos_third(p, sp, cp);                         // |p| <= pi / 3
#else
  sincos(p, &sp, &cp);
#endif
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    out.re[i] = m.re[i] * cp - m.im[i] * sp;
    out.im[i] = m.re[i] * sp + m.im[i] * cp;
  }
}

// v = m3_to_vec8(m3_project_su(x)) to rounding, forming only what the eight components read: the strict upper
// triangle and the diagonal of x r (the rotated diagonal's imaginary part needs both parts of the unrotated
// one).  The phase is taken from det x: det(x r) = det x det r, and det r is real (r is Hermitian) and
// positive whenever c0 + c1 l + c2 l^2 > 0 at the three eigenvalues l of x^H x -- it approximates l^(-1/2)
// there, also at the clamps of eigs3x3 (a degenerate spectrum: q = 0 gives three equal e, the polynomial is
// then exact at that l).  It fails only where the closed form itself has lost the spectrum (condition numbers
// of 1e4 and beyond), where the full form is no better.
__device__ __forceinline__ void m3_project_su_vec8(double v[8], const M3& x) {
  L2Q_FP_AS_WRITTEN
  H3 r;
  h3_rsqrt_gram(r, x);
  double detr, deti;
  m3_det_as_written(detr, deti, x);
  const double p = (-1.0 / 3.0) * atan2(deti, detr);
  double sp, cp;
#if L2Q_RANGED_MATH
  m_sincos_third(p, sp, cp);                         // |p| <= pi / 3
#else
  sincos(p, &sp, &cp);
#endif
  double mr[3], mi[3], dr[3], dim[3];
#pragma unroll
  for (int o = 0; o < 3; ++o) m3_mul_h3_entry(mr[o], mi[o], x, r, o == 2 ? 1 : 0, o == 0 ? 1 : 2);
#pragma unroll
  for (int i = 0; i < 3; ++i) m3_mul_h3_entry(dr[i], dim[i], x, r, i, i);
  double ure[3], uim[3], di[3];
#pragma unroll
  for (int o = 0; o < 3; ++o) {
    ure[o] = fma(mr[o], cp, -(mi[o] * sp));
    uim[o] = fma(mr[o], sp, mi[o] * cp);
    di[o] = fma(dr[o], sp, dim[o] * cp);
  }
  v[0] = -2.0 * uim[0];
  v[1] = -2.0 * ure[0];
  v[2] = di[1] - di[0];
  v[3] = -2.0 * uim[1];
  v[4] = -2.0 * ure[1];
  v[5] = -2.0 * uim[2];
  v[6] = -2.0 * ure[2];
  v[7] = 0.57735026918962584 * (fma(2.0, di[2], -di[1]) - di[0]);
}

// 8 real adjoint components (utils.py:394-420)
__device__ __forceinline__ void m3_to_vec8(double v[8], const M3& x) {
  v[0] = -2.0 * x.im[1];
  v[1] = -2.0 * x.re[1];
  v[2] = x.im[4] - x.im[0];
  v[3] = -2.0 * x.im[2];
  v[4] = -2.0 * x.re[2];
  v[5] = -2.0 * x.im[5];
  v[6] = -2.0 * x.re[5];
  v[7] = 0.57735026918962584 * (2.0 * x.im[8] - x.im[4] - x.im[0]);
}

}  // namespace l2q
