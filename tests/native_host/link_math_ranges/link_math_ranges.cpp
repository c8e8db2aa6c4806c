// TEST INFRASTRUCTURE: host driver for the range-restricted routines of csrc/su3_math.hpp (m_sincos_third, m_rcp,
// m_sqrt_hrsq) against long double (64-bit mantissa: its own error is 2^-11 of an fp64 ulp).  Errors are in ulp
// of the TRUE value.  stdin: one op per line; stdout: one line of numbers per op.
//   sincos lo hi n   -> n equally spaced points of [lo, hi], both ends included: max error of sin, of cos, and
//                       the arguments where they occurred
//   sincos_at t      -> error of sin, of cos, sin, cos (the values, %.17g)
//   rcp lo hi n      -> n points x = +-lo (hi / lo)^(i / (n - 1)), both signs: max error of m_rcp, argument
//   rcp_at x         -> m_rcp(x), 1.0 / x
//   root lo hi n     -> same grid, positive: max error of g = sqrt(x), of h = 1 / (2 sqrt(x)), arguments
//   root_at x        -> g, h of m_sqrt_hrsq
#include <cmath>
#include <cstdio>
#include <cstring>
#include "su3_math.hpp"
using namespace l2q;

static double ulps(double got, long double want) {
  if (want == 0.0L) return got == 0.0 ? 0.0 : HUGE_VAL;
  int ex;
  (void)frexpl(want, &ex);                           // |want| in [2^(ex-1), 2^ex): ulp = 2^(ex-53)
  return (double)(fabsl((long double)got - want) / ldexpl(1.0L, ex - 53));
}

int main() {
  char op[32];
  while (scanf("%31s", op) == 1) {
    if (!strcmp(op, "sincos")) {
      double lo, hi;
      long n;
      if (scanf("%lf %lf %ld", &lo, &hi, &n) != 3 || n < 2) return 1;
      double ms = 0.0, mc = 0.0, as = lo, ac = lo;
      for (long i = 0; i < n; ++i) {
        const double t = i == n - 1 ? hi : lo + (hi - lo) * ((double)i / (double)(n - 1));
        double s, c;
        m_sincos_third(t, s, c);
        const double es = ulps(s, sinl((long double)t)), ec = ulps(c, cosl((long double)t));
        if (es > ms) { ms = es; as = t; }
        if (ec > mc) { mc = ec; ac = t; }
      }
      printf("%.6f %.6f %.17g %.17g\n", ms, mc, as, ac);
    } else if (!strcmp(op, "sincos_at")) {
      double t, s, c;
      if (scanf("%lf", &t) != 1) return 1;
      m_sincos_third(t, s, c);
      printf("%.6f %.6f %.17g %.17g\n", ulps(s, sinl((long double)t)), ulps(c, cosl((long double)t)), s, c);
    } else if (!strcmp(op, "rcp") || !strcmp(op, "root")) {
      double lo, hi;
      long n;
      if (scanf("%lf %lf %ld", &lo, &hi, &n) != 3 || n < 2) return 1;
      const bool rcp = op[1] == 'c';
      double m0 = 0.0, m1 = 0.0, a0 = lo, a1 = lo;
      for (long i = 0; i < n; ++i) {
        const double x = i == n - 1 ? hi : lo * pow(hi / lo, (double)i / (double)(n - 1));
        if (rcp) {
          for (int sg = 0; sg < 2; ++sg) {
            const double xs = sg ? -x : x;
            const double e = ulps(m_rcp(xs), 1.0L / (long double)xs);
            if (e > m0) { m0 = e; a0 = xs; }
          }
        } else {
          double g, h;
          m_sqrt_hrsq(g, h, x);
          const long double r = sqrtl((long double)x);
          const double eg = ulps(g, r), eh = ulps(h, 0.5L / r);
          if (eg > m0) { m0 = eg; a0 = x; }
          if (eh > m1) { m1 = eh; a1 = x; }
        }
      }
      printf("%.6f %.6f %.17g %.17g\n", m0, m1, a0, a1);
    } else if (!strcmp(op, "rcp_at")) {
      double x;
      if (scanf("%lf", &x) != 1) return 1;
      printf("%.17g %.17g\n", m_rcp(x), 1.0 / x);
    } else if (!strcmp(op, "root_at")) {
      double x, g, h;
      if (scanf("%lf", &x) != 1) return 1;
      m_sqrt_hrsq(g, h, x);
      printf("%.17g %.17g\n", g, h);
    } else {
      return 2;
    }
  }
  return 0;
}
