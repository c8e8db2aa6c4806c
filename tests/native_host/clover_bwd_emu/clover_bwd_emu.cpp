// TEST INFRASTRUCTURE: csrc/su3_clover_bwd.hip compiled for the host against the stand-in HIP header and the host side
// of tests/native_host/emu/ (every thread of a workgroup an OS thread; error text and tuning table of common.hip
// restated).
//   clover_bwd_emu nb T X Y Z xcd_swizzle xn w gx out
// reads the native-layout links xn, the weights w [nb][3] and the starting cotangent gx (raw float64), runs
// l2q_su3_clover_bwd on a workspace of exactly the documented size and writes gx to out.
#include "su3_clover_bwd.hip"
#include "emu_host.hpp"
int main(int argc, char** argv) {
  if (argc != 11) { fprintf(stderr, "usage: clover_bwd_emu nb T X Y Z xcd_swizzle xn w gx out\n"); return 2; }
  int nb = atoi(argv[1]), T = atoi(argv[2]), X = atoi(argv[3]), Y = atoi(argv[4]), Z = atoi(argv[5]);
  l2q::tuning().xcd_swizzle = atoi(argv[6]);
  auto xn = rd(argv[7]), w = rd(argv[8]), gx = rd(argv[9]);
  const size_t V = (size_t)T * X * Y * Z;
  if (xn.size() != nb * 72 * V || gx.size() != xn.size() || w.size() != (size_t)nb * 3) { fprintf(stderr, "bad input sizes\n"); return 2; }
  std::vector<double> ws(nb * 54 * V, -7.0);
  int rc = l2q_su3_clover_bwd(xn.data(), w.data(), gx.data(), nb, T, X, Y, Z, ws.data(), ws.size() * 8, nullptr);
  if (rc) return fail(rc);
  // a workspace one double short is refused
  if (l2q_su3_clover_bwd(xn.data(), w.data(), gx.data(), nb, T, X, Y, Z, ws.data(), ws.size() * 8 - 8, nullptr) != L2Q_ESHAPE) { fprintf(stderr, "short workspace accepted\n"); return 1; }
  wr(argv[10], gx);
  return 0;
}
