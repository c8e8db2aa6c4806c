// TEST INFRASTRUCTURE: csrc/su3_wilson.hip compiled for the host against the stand-in HIP header and the host side of
// tests/native_host/emu/ (every thread of a workgroup an OS thread; error text and tuning table of common.hip
// restated).
//   wilson_emu nb nrhs T X Y Z xcd_swizzle kappa in_x in_psi in_xrpq in_coef out_apply out_norm out_cg out_rr out_xpay
// reads a native-layout link field (raw float64) from in_x, a spinor field [nb][nrhs][12][V] from in_psi, the four
// spinor fields x, r, p, q of a CG update from in_xrpq and alpha[nb * nrhs], beta[nb * nrhs] from in_coef:
//   out_apply = l2q_su3_wilson_apply(in_x, in_psi, kappa, flags) for flags = 0, 1, 2, 3, one after another;
//   out_norm  = their norm partials [4][nb][nrhs][parts];
//   out_cg    = x, r after l2q_su3_spinor_cg_update(x, r, p, q, alpha);  out_rr = its partials [nb * nrhs][parts];
//   out_xpay  = p after l2q_su3_spinor_xpay(p, q, beta).
// Every output starts as -7 in every entry, so an entry that no thread wrote shows.
#include "su3_wilson.hip"
#include "emu_host.hpp"
int main(int argc, char** argv) {
  if (argc != 18) { fprintf(stderr, "usage: see the head of wilson_emu.cpp\n"); return 2; }
  const int nb = atoi(argv[1]), nrhs = atoi(argv[2]), T = atoi(argv[3]), X = atoi(argv[4]), Y = atoi(argv[5]), Z = atoi(argv[6]);
  l2q::tuning().xcd_swizzle = atoi(argv[7]);
  const double kappa = atof(argv[8]);
  const std::vector<double> x = rd(argv[9]), psi = rd(argv[10]), xrpq = rd(argv[11]), coef = rd(argv[12]);
  const long V = (long)T * X * Y * Z, nsys = (long)nb * nrhs;
  const size_t n = (size_t)nsys * 24 * V;
  if (x.size() != (size_t)nb * 72 * V || psi.size() != n || xrpq.size() != 4 * n || coef.size() != (size_t)2 * nsys) { fprintf(stderr, "bad field size\n"); return 3; }
  const long parts = l2q_su3_wilson_norm_parts(T, X, Y, Z);
  if (parts != (V + 255) / 256) { fprintf(stderr, "parts %ld\n", parts); return 3; }
  std::vector<double> oa, on;
  for (int flags = 0; flags < 4; ++flags) {
    std::vector<double> o(n, -7.0), np(nsys * parts, -7.0);
    const int rc = l2q_su3_wilson_apply(x.data(), psi.data(), o.data(), np.data(), kappa, flags, nb, nrhs, T, X, Y, Z, nullptr);
    if (rc) return fail(rc);
    // without the partials: the same field
    std::vector<double> o2(n, -7.0);
    const int rc2 = l2q_su3_wilson_apply(x.data(), psi.data(), o2.data(), nullptr, kappa, flags, nb, nrhs, T, X, Y, Z, nullptr);
    if (rc2) return fail(rc2);
    if (memcmp(o.data(), o2.data(), n * sizeof(double)) != 0) { fprintf(stderr, "the fused norm changed the field\n"); return 4; }
    oa.insert(oa.end(), o.begin(), o.end());
    on.insert(on.end(), np.begin(), np.end());
  }
  std::vector<double> cx(xrpq.begin(), xrpq.begin() + n), cr(xrpq.begin() + n, xrpq.begin() + 2 * n);
  std::vector<double> cp(xrpq.begin() + 2 * n, xrpq.begin() + 3 * n), cq(xrpq.begin() + 3 * n, xrpq.end());
  std::vector<double> rr(nsys * parts, -7.0);
  int rc = l2q_su3_spinor_cg_update(cx.data(), cr.data(), cp.data(), cq.data(), coef.data(), rr.data(), nsys, V, nullptr);
  if (rc) return fail(rc);
  rc = l2q_su3_spinor_xpay(cp.data(), cq.data(), coef.data() + nsys, nsys, V, nullptr);
  if (rc) return fail(rc);
  cx.insert(cx.end(), cr.begin(), cr.end());
  wr(argv[13], oa);
  wr(argv[14], on);
  wr(argv[15], cx);
  wr(argv[16], rr);
  wr(argv[17], cp);
  return 0;
}
