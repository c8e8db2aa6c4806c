// TEST INFRASTRUCTURE: host driver that sets m3_expm and m3_project_su_vec8 of csrc/su3_math.hpp against the
// forms they replaced, which this file carries as its yardsticks (ref_expm: the 20-step coefficient loop run to
// its end; ref_project_su: the projection on full 3x3 products with the phase of det(x r)).
// stdin: one op per line; stdout: one line of numbers per op.
//   expm A(9 complex)            -> exp(A) from m3_expm (18), from ref_expm (18), steps the loop took (1)
//   rand norm count seed         -> `count` seeded Gaussian complex matrices scaled to |A|_F = norm:
//                                   entries compared, entries whose bits differ, entries off by more than 1 ulp,
//                                   mean steps of m3_expm
//   vec8 X(9 complex)            -> m3_project_su_vec8(X) (8), m3_to_vec8(ref_project_su(X)) (8)
#include <cstdint>
#include <cstdio>
#include <cstring>
static long g_steps = 0;
#define L2Q_EXPM_COUNT_STEPS(n) (g_steps += (n))
#include "su3_math.hpp"
using namespace l2q;

// ---- yardstick: m3_expm as it stood before the early exit (all 20 steps)
static void ref_expm(M3& out, const M3& ain) {
  double n2 = 0.0;
  for (int i = 0; i < 9; ++i) n2 += ain.re[i] * ain.re[i] + ain.im[i] * ain.im[i];
  const double nrm = sqrt(n2);
  int s = 0;
  double scale = 1.0;
  if (nrm > 0.5) {
    int ex;
    (void)frexp(nrm, &ex);
    s = ex + 1;
    if (s > 60) s = 60;
    scale = ldexp(1.0, -s);
  }
  M3 a;
  for (int i = 0; i < 9; ++i) { a.re[i] = ain.re[i] * scale; a.im[i] = ain.im[i] * scale; }
  M3 a2;
  m3_mul_nn(a2, a, a);
  const double p2r = a.re[0] + a.re[4] + a.re[8], p2i = a.im[0] + a.im[4] + a.im[8];
  const double t2r = a2.re[0] + a2.re[4] + a2.re[8], t2i = a2.im[0] + a2.im[4] + a2.im[8];
  double sqr, sqi;
  cmul(sqr, sqi, p2r, p2i, p2r, p2i);
  const double p1r = 0.5 * (sqr - t2r), p1i = 0.5 * (sqi - t2i);
  double p0r, p0i;
  m3_det(p0r, p0i, a);
  double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0, cr = 0.5, ci = 0.0;
  double f0r = 1.0, f0i = 0.0, f1r = 1.0, f1i = 0.0, f2r = 0.5, f2i = 0.0;
  static constexpr double kInv[22] = {
      1.0 / 1, 1.0 / 2, 1.0 / 3, 1.0 / 4, 1.0 / 5, 1.0 / 6, 1.0 / 7, 1.0 / 8, 1.0 / 9, 1.0 / 10, 1.0 / 11,
      1.0 / 12, 1.0 / 13, 1.0 / 14, 1.0 / 15, 1.0 / 16, 1.0 / 17, 1.0 / 18, 1.0 / 19, 1.0 / 20, 1.0 / 21, 1.0 / 22};
  for (int n = 2; n < 22; ++n) {
    const double inv = kInv[n];
    double xr, xi, yr, yi, zr, zi;
    cmul(xr, xi, cr, ci, p0r, p0i);                  // c p0
    cmul(yr, yi, cr, ci, p1r, p1i);                  // c p1
    cmul(zr, zi, cr, ci, p2r, p2i);                  // c p2
    const double nar = xr * inv, nai = xi * inv;
    const double nbr = (ar - yr) * inv, nbi = (ai - yi) * inv;
    const double ncr = (br + zr) * inv, nci = (bi + zi) * inv;
    ar = nar; ai = nai; br = nbr; bi = nbi; cr = ncr; ci = nci;
    f0r += ar; f0i += ai; f1r += br; f1i += bi; f2r += cr; f2i += ci;
  }
  for (int i = 0; i < 9; ++i) {
    double xr, xi, yr, yi;
    cmul(xr, xi, f1r, f1i, a.re[i], a.im[i]);
    cmul(yr, yi, f2r, f2i, a2.re[i], a2.im[i]);
    out.re[i] = xr + yr; out.im[i] = xi + yi;
  }
  out.re[0] += f0r; out.re[4] += f0r; out.re[8] += f0r;
  out.im[0] += f0i; out.im[4] += f0i; out.im[8] += f0i;
  for (int k = 0; k < s; ++k) {
    M3 t;
    m3_mul_nn(t, out, out);
    out = t;
  }
}

// ---- yardstick: the projection on full products, phase from det(x r)
static void ref_project_su(M3& out, const M3& x) {
  M3 t, t2;
  m3_mul_an(t, x, x);
  m3_mul_nn(t2, t, t);
  const double tr = t.re[0] + t.re[4] + t.re[8];
  const double p2 = t2.re[0] + t2.re[4] + t2.re[8];
  double detr, deti;
  m3_det(detr, deti, t);
  double e0, e1, e2;
  eigs3x3(e0, e1, e2, tr, p2, detr);
  const double se0 = sqrt(fabs(e0)), se1 = sqrt(fabs(e1)), se2 = sqrt(fabs(e2));
  const double u = se0 + se1 + se2;
  const double w = se0 * se1 * se2;
  const double d = w * (se0 + se1) * (se0 + se2) * (se1 + se2);
  const double di = 1.0 / d;
  const double c0 = di * (w * u * u + e0 * se0 * (e1 + e2) + e1 * se1 * (e0 + e2) + e2 * se2 * (e0 + e1));
  const double c1 = -(tr * u + w) * di;
  const double c2 = u * di;
  M3 r, m;
  for (int i = 0; i < 9; ++i) {
    r.re[i] = c1 * t.re[i] + c2 * t2.re[i];
    r.im[i] = c1 * t.im[i] + c2 * t2.im[i];
  }
  r.re[0] += c0; r.re[4] += c0; r.re[8] += c0;
  m3_mul_nn(m, x, r);
  m3_det(detr, deti, m);
  const double p = (-1.0 / 3.0) * atan2(deti, detr);
  const double sp = sin(p), cp = cos(p);
  for (int i = 0; i < 9; ++i) {
    out.re[i] = m.re[i] * cp - m.im[i] * sp;
    out.im[i] = m.re[i] * sp + m.im[i] * cp;
  }
}

static bool read_m3(M3& m) {
  for (int i = 0; i < 9; ++i)
    if (scanf("%lf %lf", &m.re[i], &m.im[i]) != 2) return false;
  return true;
}
static void print_m3(const M3& m) {
  for (int i = 0; i < 9; ++i) printf("%.17g %.17g ", m.re[i], m.im[i]);
}

// ordered integer image of a double: adjacent doubles differ by 1
static int64_t ordered(double x) {
  int64_t b;
  memcpy(&b, &x, 8);
  return b < 0 ? INT64_MIN - b : b;
}
// 0: same bits (or both NaN), 1: one ulp apart, 2: further
static int distance(double a, double b) {
  if (a != a || b != b) return (a != a && b != b) ? 0 : 2;
  uint64_t ba, bb;
  memcpy(&ba, &a, 8); memcpy(&bb, &b, 8);
  if (ba == bb) return 0;
  const int64_t oa = ordered(a), ob = ordered(b);
  const uint64_t d = oa > ob ? (uint64_t)oa - (uint64_t)ob : (uint64_t)ob - (uint64_t)oa;
  return d <= 1 ? 1 : 2;
}

// splitmix64 -> uniform (0, 1) -> Box-Muller
static uint64_t g_rng;
static double uniform() {
  uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return ((double)(z >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}
static double gauss() { return sqrt(-2.0 * log(uniform())) * cos(6.283185307179586 * uniform()); }

int main() {
  char op[32];
  while (scanf("%31s", op) == 1) {
    if (!strcmp(op, "expm")) {
      M3 a, e, r;
      if (!read_m3(a)) return 1;
      g_steps = 0;
      m3_expm(e, a);
      ref_expm(r, a);
      print_m3(e);
      print_m3(r);
      printf("%ld\n", g_steps);
    } else if (!strcmp(op, "rand")) {
      double norm;
      long count;
      unsigned long long seed;
      if (scanf("%lf %ld %llu", &norm, &count, &seed) != 3) return 1;
      g_rng = seed;
      g_steps = 0;
      long differ = 0, far = 0;
      for (long k = 0; k < count; ++k) {
        M3 a, e, r;
        double n2 = 0.0;
        for (int i = 0; i < 9; ++i) {
          a.re[i] = gauss(); a.im[i] = gauss();
          n2 += a.re[i] * a.re[i] + a.im[i] * a.im[i];
        }
        const double sc = norm / sqrt(n2);
        for (int i = 0; i < 9; ++i) { a.re[i] *= sc; a.im[i] *= sc; }
        m3_expm(e, a);
        ref_expm(r, a);
        for (int i = 0; i < 9; ++i) {
          const int dr = distance(e.re[i], r.re[i]), di = distance(e.im[i], r.im[i]);
          differ += (dr > 0) + (di > 0);
          far += (dr > 1) + (di > 1);
        }
      }
      printf("%ld %ld %ld %.6f\n", 18 * count, differ, far, (double)g_steps / (double)count);
    } else if (!strcmp(op, "vec8")) {
      M3 x, r;
      double v[8], w[8];
      if (!read_m3(x)) return 1;
      m3_project_su_vec8(v, x);
      ref_project_su(r, x);
      m3_to_vec8(w, r);
      for (int i = 0; i < 8; ++i) printf("%.17g ", v[i]);
      for (int i = 0; i < 8; ++i) printf("%.17g ", w[i]);
      printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
