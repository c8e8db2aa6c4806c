// TEST INFRASTRUCTURE: csrc/su3_clover_force.hip compiled for the host against the stand-in HIP header and the host side
// of tests/native_host/emu/ (every thread of a workgroup an OS thread; error text and tuning table of common.hip
// restated).
//   wilson_clover_force_emu nb npf T X Y Z xcd_swizzle kc coef det_weight in_x in_X in_Y in_clinv in_v
//                           out_g out_force out_kick out_det out_pf
// reads the native-layout links, the fields X, Y [nb][npf][12][V], the block field of A^-1 [nb][2][2][36][V/2] and an
// anti-Hermitian link field v (raw float64), and runs l2q_su3_clover_force on a workspace of exactly the documented size:
//   out_force = the force (f_in null, coef 1) of both terms, out_g = the workspace it leaves;
//   out_kick  = v + coef F out of place; repeated in place (f_in == f_out): the same bits;
//   out_det   = the determinant term alone (X, Y null, npf 0);   out_pf = the pseudofermion term alone (clinv null).
// The force of chain 0 alone is the same bits; no input is written; a workspace one double short is refused.
// Every output starts as -7 in every entry, so an entry that no thread wrote shows.
#include "su3_clover_force.hip"
#include "emu_host.hpp"
int main(int argc, char** argv) {
  if (argc != 21) { fprintf(stderr, "usage: see the head of wilson_clover_force_emu.cpp\n"); return 2; }
  const int nb = atoi(argv[1]), npf = atoi(argv[2]), T = atoi(argv[3]), X = atoi(argv[4]), Y = atoi(argv[5]), Z = atoi(argv[6]);
  l2q::tuning().xcd_swizzle = atoi(argv[7]);
  const double kc = atof(argv[8]), coef = atof(argv[9]), dw = atof(argv[10]);
  const std::vector<double> x = rd(argv[11]), fx = rd(argv[12]), fy = rd(argv[13]), ci = rd(argv[14]), v = rd(argv[15]);
  const size_t V = (size_t)T * X * Y * Z, nl = (size_t)nb * 72 * V, ns = (size_t)nb * npf * 24 * V;
  if (x.size() != nl || v.size() != nl || fx.size() != ns || fy.size() != ns || ci.size() != (size_t)nb * 4 * 36 * (V / 2)) {
    fprintf(stderr, "bad field size\n");
    return 3;
  }
  const std::vector<double> x0 = x, fx0 = fx, fy0 = fy, ci0 = ci, v0 = v;
  const size_t nw = (size_t)nb * 54 * V;
  int rc;
  const auto run = [&](const double* px, const double* py, const double* pc, const double* fin, std::vector<double>& out,
                       std::vector<double>& ws, double cf, double w, int chains, int fields) {
    return l2q_su3_clover_force(x.data(), px, py, pc, fin, out.data(), kc, cf, w, chains, fields, T, X, Y, Z, ws.data(),
                                (size_t)chains * 54 * V * 8, nullptr);
  };
  std::vector<double> ws(nw, -7.0), force(nl, -7.0);
  if ((rc = run(fx.data(), fy.data(), ci.data(), nullptr, force, ws, 1.0, dw, nb, npf))) return fail(rc);
  wr(argv[16], ws);
  wr(argv[17], force);
  if (l2q_su3_clover_force(x.data(), fx.data(), fy.data(), ci.data(), nullptr, force.data(), kc, 1.0, dw, nb, npf, T, X, Y, Z,
                           ws.data(), nw * 8 - 8, nullptr) != L2Q_EINVAL) { fprintf(stderr, "short workspace accepted\n"); return 1; }
  {
    std::vector<double> w1(nw, -7.0), alone(nl / nb, -7.0);        // chain 0 alone
    if ((rc = run(fx.data(), fy.data(), ci.data(), nullptr, alone, w1, 1.0, dw, 1, npf))) return fail(rc);
    if (memcmp(alone.data(), force.data(), alone.size() * 8) != 0) { fprintf(stderr, "a chain alone gives other bits\n"); return 4; }
  }
  {
    std::vector<double> w1(nw, -7.0), kick(nl, -7.0), inplace(v);
    if ((rc = run(fx.data(), fy.data(), ci.data(), v.data(), kick, w1, coef, dw, nb, npf))) return fail(rc);
    if ((rc = run(fx.data(), fy.data(), ci.data(), inplace.data(), inplace, w1, coef, dw, nb, npf))) return fail(rc);
    if (memcmp(kick.data(), inplace.data(), nl * 8) != 0) { fprintf(stderr, "the kick in place gives other bits\n"); return 4; }
    wr(argv[18], kick);
  }
  {
    std::vector<double> w1(nw, -7.0), det(nl, -7.0), pf(nl, -7.0);
    if ((rc = run(nullptr, nullptr, ci.data(), nullptr, det, w1, 1.0, dw, nb, 0))) return fail(rc);
    std::fill(w1.begin(), w1.end(), -7.0);
    if ((rc = run(fx.data(), fy.data(), nullptr, nullptr, pf, w1, 1.0, dw, nb, npf))) return fail(rc);
    wr(argv[19], det);
    wr(argv[20], pf);
  }
  if (x != x0 || fx != fx0 || fy != fy0 || ci != ci0 || v != v0) { fprintf(stderr, "an input was written\n"); return 4; }
  return 0;
}
