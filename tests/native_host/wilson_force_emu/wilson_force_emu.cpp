// TEST INFRASTRUCTURE: csrc/su3_wilson_force.hip compiled for the host against the stand-in HIP header and the host
// side of tests/native_host/emu/ (every thread of a workgroup an OS thread; error text and tuning table of common.hip
// restated).
//   wilson_force_emu nb npf T X Y Z xcd_swizzle kappa coef in_x in_X in_Y in_v out_force out_kick out_inplace out_alone
// reads a native-layout link field (raw float64) from in_x, two spinor fields [nb][npf][12][V] from in_X and in_Y and a
// momentum field [nb][4][9][V] from in_v; for flags = 0 and 2 (periodic, antiperiodic in t), one after another:
//   out_force   = l2q_su3_wilson_force(f_in = null, coef = 1);
//   out_kick    = l2q_su3_wilson_force(f_in = v, coef) into a new field;
//   out_inplace = the same with f_in = f_out = a copy of v;
//   out_alone   = chain 0 on its own (nb = 1), f_in = null, coef = 1.
// Every output starts as -7 in every entry, so an entry that no thread wrote shows.
#include "su3_wilson_force.hip"
#include "emu_host.hpp"
int main(int argc, char** argv) {
  if (argc != 18) { fprintf(stderr, "usage: see the head of wilson_force_emu.cpp\n"); return 2; }
  const int nb = atoi(argv[1]), npf = atoi(argv[2]), T = atoi(argv[3]), X = atoi(argv[4]), Y = atoi(argv[5]), Z = atoi(argv[6]);
  l2q::tuning().xcd_swizzle = atoi(argv[7]);
  const double kappa = atof(argv[8]), coef = atof(argv[9]);
  const std::vector<double> x = rd(argv[10]), fx = rd(argv[11]), fy = rd(argv[12]), v = rd(argv[13]);
  const long V = (long)T * X * Y * Z;
  const size_t nl = (size_t)nb * 72 * V, ns = (size_t)nb * npf * 24 * V;
  if (x.size() != nl || v.size() != nl || fx.size() != ns || fy.size() != ns) { fprintf(stderr, "bad field size\n"); return 3; }
  std::vector<double> of, ok, oi, oa;
  for (int flags = 0; flags < 4; flags += 2) {
    std::vector<double> f(nl, -7.0), k(nl, -7.0), i(v), a(nl / nb, -7.0);
    int rc = l2q_su3_wilson_force(x.data(), fx.data(), fy.data(), nullptr, f.data(), kappa, 1.0, flags, nb, npf, T, X, Y, Z, nullptr);
    if (rc) return fail(rc);
    rc = l2q_su3_wilson_force(x.data(), fx.data(), fy.data(), v.data(), k.data(), kappa, coef, flags, nb, npf, T, X, Y, Z, nullptr);
    if (rc) return fail(rc);
    rc = l2q_su3_wilson_force(x.data(), fx.data(), fy.data(), i.data(), i.data(), kappa, coef, flags, nb, npf, T, X, Y, Z, nullptr);
    if (rc) return fail(rc);
    rc = l2q_su3_wilson_force(x.data(), fx.data(), fy.data(), nullptr, a.data(), kappa, 1.0, flags, 1, npf, T, X, Y, Z, nullptr);
    if (rc) return fail(rc);
    of.insert(of.end(), f.begin(), f.end());
    ok.insert(ok.end(), k.begin(), k.end());
    oi.insert(oi.end(), i.begin(), i.end());
    oa.insert(oa.end(), a.begin(), a.end());
  }
  wr(argv[14], of);
  wr(argv[15], ok);
  wr(argv[16], oi);
  wr(argv[17], oa);
  return 0;
}
