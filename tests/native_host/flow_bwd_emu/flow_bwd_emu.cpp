// TEST INFRASTRUCTURE: csrc/su3_flow_bwd.hip compiled for the host against the stand-in HIP header and the host side
// of tests/native_host/emu/ (every thread of a workgroup an OS thread; error text, tuning table and launch_zero of
// common.hip restated).  Only the kernel of l2q_su3_force_vjp is run here; the entry points the stage and the
// step reverse call in other files (forward stage, force kick, l2q_su3_expm_mul_bwd) are refused: their composition
// is the business of tests/test_flow_bwd_gpu.py.
//   flow_bwd_emu nb T X Y Z xcd_swizzle beta xn gf gx out
// reads the native-layout links xn, the cotangent gf of the force and the starting cotangent gx (raw float64), runs
// l2q_su3_force_vjp and writes gx to out.
#include "su3_flow_bwd.hip"
#include "emu_host.hpp"
extern "C" {
int l2q_su3_flow_stage(const void*, const void*, double, double, void*, void*, int, int, int, int, int, void*) { return L2Q_EINVAL; }
int l2q_su3_force_kick_to(const void*, double, double, const void*, void*, int, int, int, int, int, void*) { return L2Q_EINVAL; }
int l2q_su3_expm_mul_bwd(const void*, const void*, double, const float*, int, const void*, void*, void*, double*, int, long, void*, size_t, void*) { return L2Q_EINVAL; }
}
int main(int argc, char** argv) {
  if (argc != 12) { fprintf(stderr, "usage: flow_bwd_emu nb T X Y Z xcd_swizzle beta xn gf gx out\n"); return 2; }
  int nb = atoi(argv[1]), T = atoi(argv[2]), X = atoi(argv[3]), Y = atoi(argv[4]), Z = atoi(argv[5]);
  l2q::tuning().xcd_swizzle = atoi(argv[6]);
  const double beta = atof(argv[7]);
  auto xn = rd(argv[8]), gf = rd(argv[9]), gx = rd(argv[10]);
  const size_t V = (size_t)T * X * Y * Z;
  if (xn.size() != nb * 72 * V || gx.size() != xn.size() || gf.size() != xn.size()) { fprintf(stderr, "bad input sizes\n"); return 2; }
  int rc = l2q_su3_force_vjp(xn.data(), gf.data(), beta, gx.data(), nb, T, X, Y, Z, nullptr);
  if (rc) return fail(rc);
  // gx aliasing an input is refused
  if (l2q_su3_force_vjp(xn.data(), gf.data(), beta, gf.data(), nb, T, X, Y, Z, nullptr) != L2Q_EINVAL ||
      l2q_su3_force_vjp(xn.data(), gf.data(), beta, xn.data(), nb, T, X, Y, Z, nullptr) != L2Q_EINVAL) { fprintf(stderr, "aliased gx accepted\n"); return 1; }
  wr(argv[11], gx);
  return 0;
}
