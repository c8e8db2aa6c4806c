// TEST INFRASTRUCTURE: csrc/su3_spinor_mshift.hip compiled for the host against the stand-in HIP header and the host side
// of tests/native_host/emu/ (every thread of a workgroup an OS thread).
//   spinor_mshift_emu nsys ns V xcd_swizzle in_fields in_coef out_update out_r out_part out_lin
// in_fields: x[nsys][ns][12][V], ps (the same shape), p[nsys][12][V], r, z, one after another (complex128 as pairs);
// in_coef: a, b, zeta [nsys * ns], beta, alpha [nsys], w [nsys * ns], live [nsys * ns] (doubles, != 0 is live).
//   out_update = x, ps, p after l2q_su3_spinor_mshift_update(x, ps, p, r, a, b, zeta, beta, live);
//   out_r, out_part = r2 and the partials [nsys][parts] after l2q_su3_spinor_axmy_norm(r2 = a copy of r, z, alpha);
//   out_lin = l2q_su3_spinor_lincomb(x (the input), w), its output pre-filled with -7.
// The program itself refuses (exit 4) an input that a kernel wrote: r in the update, z in the residual step, x and w in
// the linear combination, and the coefficient arrays everywhere.
#include "su3_spinor_mshift.hip"
#include "emu_host.hpp"
int main(int argc, char** argv) {
  if (argc != 11) { fprintf(stderr, "usage: see the head of spinor_mshift_emu.cpp\n"); return 2; }
  const long nsys = atol(argv[1]), ns = atol(argv[2]), V = atol(argv[3]);
  l2q::tuning().xcd_swizzle = atoi(argv[4]);
  const std::vector<double> f = rd(argv[5]), coef = rd(argv[6]);
  const size_t one = (size_t)nsys * 24 * V, all = one * ns, nc = (size_t)nsys * ns;
  if (f.size() != 2 * all + 3 * one || coef.size() != 5 * nc + 2 * (size_t)nsys) { fprintf(stderr, "bad field size\n"); return 3; }
  std::vector<double> x(f.begin(), f.begin() + all), ps(f.begin() + all, f.begin() + 2 * all);
  std::vector<double> p(f.begin() + 2 * all, f.begin() + 2 * all + one);
  const std::vector<double> r(f.begin() + 2 * all + one, f.begin() + 2 * all + 2 * one), z(f.begin() + 2 * all + 2 * one, f.end());
  const double *a = coef.data(), *b = a + nc, *zeta = b + nc, *beta = zeta + nc, *alpha = beta + nsys, *w = alpha + nsys;
  std::vector<int> live(nc);
  for (size_t i = 0; i < nc; ++i) live[i] = w[nc + i] != 0.0;
  const std::vector<double> x0 = x, r0 = r, z0 = z, c0 = coef;
  const std::vector<int> l0 = live;
  int rc = l2q_su3_spinor_mshift_update(x.data(), ps.data(), p.data(), r.data(), a, b, zeta, beta, live.data(), nsys, ns, V, nullptr);
  if (rc) return fail(rc);
  if (r != r0 || coef != c0 || live != l0) { fprintf(stderr, "the update wrote an input\n"); return 4; }
  const long parts = (V + 255) / 256;
  std::vector<double> r2 = r, part(nsys * parts, -7.0);
  rc = l2q_su3_spinor_axmy_norm(r2.data(), z.data(), alpha, part.data(), nsys, V, nullptr);
  if (rc) return fail(rc);
  if (z != z0 || coef != c0) { fprintf(stderr, "the residual step wrote an input\n"); return 4; }
  std::vector<double> lin(one, -7.0);
  rc = l2q_su3_spinor_lincomb(x0.data(), w, lin.data(), nsys, ns, V, nullptr);
  if (rc) return fail(rc);
  if (coef != c0) { fprintf(stderr, "the linear combination wrote an input\n"); return 4; }
  x.insert(x.end(), ps.begin(), ps.end());
  x.insert(x.end(), p.begin(), p.end());
  wr(argv[7], x);
  wr(argv[8], r2);
  wr(argv[9], part);
  wr(argv[10], lin);
  return 0;
}
