// TEST INFRASTRUCTURE: csrc/su3_clover_bwd.hip compiled for the host against the stand-in HIP header next to this
// file, with the two things it takes from common.hip (error text, tuning table) restated plainly.
//   clover_bwd_emu nb T X Y Z xcd_swizzle xn w gx out
// reads the native-layout links xn, the weights w [nb][3] and the starting cotangent gx (raw float64), runs
// l2q_su3_clover_bwd on a workspace of exactly the documented size and writes gx to out.
#include <cstdarg>
#include <cstring>
#include <string>
#include "su3_clover_bwd.hip"
namespace l2q {
static char g_err[512];
void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
Tuning& tuning() { static Tuning t; return t; }
}
extern "C" const char* l2q_last_error() { return l2q::g_err; }
static std::vector<double> rd(const char* f) { FILE* p = fopen(f, "rb"); fseek(p, 0, SEEK_END); long n = ftell(p); fseek(p, 0, SEEK_SET); std::vector<double> v(n / 8); if (fread(v.data(), 8, v.size(), p) != v.size()) exit(3); fclose(p); return v; }
static void wr(const char* f, const std::vector<double>& v) { FILE* p = fopen(f, "wb"); fwrite(v.data(), 8, v.size(), p); fclose(p); }
int main(int argc, char** argv) {
  if (argc != 11) { fprintf(stderr, "usage: clover_bwd_emu nb T X Y Z xcd_swizzle xn w gx out\n"); return 2; }
  int nb = atoi(argv[1]), T = atoi(argv[2]), X = atoi(argv[3]), Y = atoi(argv[4]), Z = atoi(argv[5]);
  l2q::tuning().xcd_swizzle = atoi(argv[6]);
  auto xn = rd(argv[7]), w = rd(argv[8]), gx = rd(argv[9]);
  const size_t V = (size_t)T * X * Y * Z;
  if (xn.size() != nb * 72 * V || gx.size() != xn.size() || w.size() != (size_t)nb * 3) { fprintf(stderr, "bad input sizes\n"); return 2; }
  std::vector<double> ws(nb * 54 * V, -7.0);
  int rc = l2q_su3_clover_bwd(xn.data(), w.data(), gx.data(), nb, T, X, Y, Z, ws.data(), ws.size() * 8, nullptr);
  if (rc) { fprintf(stderr, "rc %d %s\n", rc, l2q_last_error()); return 1; }
  // a workspace one double short is refused
  if (l2q_su3_clover_bwd(xn.data(), w.data(), gx.data(), nb, T, X, Y, Z, ws.data(), ws.size() * 8 - 8, nullptr) != L2Q_ESHAPE) { fprintf(stderr, "short workspace accepted\n"); return 1; }
  wr(argv[10], gx);
  return 0;
}
