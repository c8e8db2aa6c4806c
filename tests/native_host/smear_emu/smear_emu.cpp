// TEST INFRASTRUCTURE: csrc/su3_smear.hip compiled for the host against the stand-in HIP header and the host side of
// tests/native_host/emu/ (every thread of a workgroup an OS thread; error text and tuning table of common.hip
// restated).
//   smear_emu nb T X Y Z xcd_swizzle masks alphas alpha1 alpha2 alpha3 in_x in_b1 in_b2 out_ape out_b1 out_b2 out_v
// reads a native-layout link field (raw float64) from in_x and two decorated fields [nb][4][3][9][V] from in_b1, in_b2:
//   out_ape = for each mask of the comma-separated list `masks` and the alpha at its place in the list `alphas`,
//             l2q_su3_ape_smear(in_x, alpha, mask), one after another;
//   out_b1  = l2q_su3_hyp_level1(in_x, alpha3);
//   out_b2  = l2q_su3_hyp_level2(in_x, in_b1, alpha2);
//   out_v   = l2q_su3_hyp_level3(in_x, in_b2, alpha1).
// Every output starts as -7 in every entry, so an entry that no thread wrote shows.
#include "su3_smear.hip"
#include "emu_host.hpp"
int main(int argc, char** argv) {
  if (argc != 19) { fprintf(stderr, "usage: see the head of smear_emu.cpp\n"); return 2; }
  const int nb = atoi(argv[1]), T = atoi(argv[2]), X = atoi(argv[3]), Y = atoi(argv[4]), Z = atoi(argv[5]);
  l2q::tuning().xcd_swizzle = atoi(argv[6]);
  std::vector<int> masks;
  for (char* tok = strtok(argv[7], ","); tok; tok = strtok(nullptr, ",")) masks.push_back(atoi(tok));
  std::vector<double> alphas;
  for (char* tok = strtok(argv[8], ","); tok; tok = strtok(nullptr, ",")) alphas.push_back(atof(tok));
  if (alphas.size() != masks.size()) { fprintf(stderr, "one alpha per mask\n"); return 2; }
  const double a1 = atof(argv[9]), a2 = atof(argv[10]), a3 = atof(argv[11]);
  const std::vector<double> x = rd(argv[12]), b1 = rd(argv[13]), b2 = rd(argv[14]);
  const long V = (long)T * X * Y * Z;
  if (x.size() != (size_t)nb * 72 * V || b1.size() != 3 * x.size() || b2.size() != 3 * x.size()) { fprintf(stderr, "bad field size\n"); return 3; }
  std::vector<double> oape;
  for (size_t i = 0; i < masks.size(); ++i) {
    std::vector<double> o(x.size(), -7.0);
    const int rc = l2q_su3_ape_smear(x.data(), alphas[i], masks[i], o.data(), nb, T, X, Y, Z, nullptr);
    if (rc) return fail(rc);
    oape.insert(oape.end(), o.begin(), o.end());
  }
  std::vector<double> o1(b1.size(), -7.0), o2(b1.size(), -7.0), ov(x.size(), -7.0);
  int rc = l2q_su3_hyp_level1(x.data(), a3, o1.data(), nb, T, X, Y, Z, nullptr);
  if (rc) return fail(rc);
  rc = l2q_su3_hyp_level2(x.data(), b1.data(), a2, o2.data(), nb, T, X, Y, Z, nullptr);
  if (rc) return fail(rc);
  rc = l2q_su3_hyp_level3(x.data(), b2.data(), a1, ov.data(), nb, T, X, Y, Z, nullptr);
  if (rc) return fail(rc);
  wr(argv[15], oape);
  wr(argv[16], o1);
  wr(argv[17], o2);
  wr(argv[18], ov);
  return 0;
}
