// TEST INFRASTRUCTURE: csrc/su3_loops.hip compiled for the host against the stand-in HIP header and the host side of
// tests/native_host/emu/ (every thread of a workgroup an OS thread; error text, tuning table and the second reduction
// stage of common.hip restated).
//   loops_emu <extend|extend_alias|loops|polyakov> nb T X Y Z p1 p2 xcd_swizzle in_a in_b out
// reads native-layout fields (raw float64) from in_a, in_b and writes the entry point's output to out:
//   extend: lines_in = a, xn = b, n = p1;  loops: a, r = p1, b, t = p2;  polyakov: xn = a, mu = p1.
#include "su3_loops.hip"
#include "emu_host.hpp"
int main(int argc, char** argv) {
  std::string mode = argv[1];
  int nb = atoi(argv[2]), T = atoi(argv[3]), X = atoi(argv[4]), Y = atoi(argv[5]), Z = atoi(argv[6]), p1 = atoi(argv[7]), p2 = atoi(argv[8]);
  l2q::tuning().xcd_swizzle = atoi(argv[9]);
  auto a = rd(argv[10]), b = rd(argv[11]);
  long V = (long)T * X * Y * Z;
  int rc = 0;
  if (mode == "extend") { std::vector<double> o(a.size(), -7.0); rc = l2q_su3_line_extend(a.data(), b.data(), p1, o.data(), nb, T, X, Y, Z, nullptr); wr(argv[12], o); }
  else if (mode == "extend_alias") { rc = l2q_su3_line_extend(a.data(), b.data(), p1, a.data(), nb, T, X, Y, Z, nullptr); wr(argv[12], a); }
  else if (mode == "loops") { long nblk = (V + 255) / 256; std::vector<double> ws(nb * nblk * 24, -7.0), o(nb * 24, -7.0);
    rc = l2q_su3_loop_reduce(a.data(), p1, b.data(), p2, o.data(), nb, T, X, Y, Z, ws.data(), ws.size() * 8, nullptr); wr(argv[12], o); }
  else if (mode == "polyakov") { int ext = p1 == 0 ? T : p1 == 1 ? X : p1 == 2 ? Y : Z; std::vector<double> o(nb * (V / ext) * 2, -7.0);
    rc = l2q_su3_polyakov(a.data(), p1, o.data(), nb, T, X, Y, Z, nullptr); wr(argv[12], o); }
  if (rc) return fail(rc);
  return 0;
}
