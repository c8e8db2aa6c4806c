// TEST INFRASTRUCTURE: csrc/su3_loops.hip compiled for the host against the stand-in HIP header next to this file, with
// the three things it takes from common.hip (error text, tuning table, the second reduction stage) restated plainly.
//   loops_emu <extend|extend_alias|loops|polyakov> nb T X Y Z p1 p2 xcd_swizzle in_a in_b out
// reads native-layout fields (raw float64) from in_a, in_b and writes the entry point's output to out:
//   extend: lines_in = a, xn = b, n = p1;  loops: a, r = p1, b, t = p2;  polyakov: xn = a, mu = p1.
#include <cstdarg>
#include <cstring>
#include <string>
#include "su3_loops.hip"
namespace l2q {
static char g_err[512];
void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
Tuning& tuning() { static Tuning t; return t; }
void launch_finalize(const double* partial, double* out, int nb, long nblk, int ncomp, double scale, double offset, hipStream_t) {
  for (int c = 0; c < nb; ++c) for (int k = 0; k < ncomp; ++k) { double s = 0; for (long b = 0; b < nblk; ++b) s += partial[(c * nblk + b) * ncomp + k]; out[c * ncomp + k] = scale * s + offset; }
}
}
extern "C" const char* l2q_last_error() { return l2q::g_err; }
static std::vector<double> rd(const char* f) { FILE* p = fopen(f, "rb"); fseek(p, 0, SEEK_END); long n = ftell(p); fseek(p, 0, SEEK_SET); std::vector<double> v(n / 8); if (fread(v.data(), 8, v.size(), p) != v.size()) exit(3); fclose(p); return v; }
static void wr(const char* f, const std::vector<double>& v) { FILE* p = fopen(f, "wb"); fwrite(v.data(), 8, v.size(), p); fclose(p); }
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
  if (rc) { fprintf(stderr, "rc %d %s\n", rc, l2q_last_error()); return 1; }
  return 0;
}
