// TEST INFRASTRUCTURE: csrc/su3_gaugefix.hip compiled for the host against the stand-in HIP header of
// tests/native_host/loops_emu/ (every thread of a workgroup an OS thread), with the three things it takes from
// common.hip (error text, tuning table, the second reduction stage) restated plainly.
//   gaugefix_emu what nb T X Y Z xcd_swizzle dirmask omega with_g with_active in_x in_g out_x out_g out_cond out_apply
// reads a native-layout field (raw float64) from in_x and a transformation G[nb][9][V] from in_g; `what` is a sum of
//   1: for parity 0, 1 one l2q_su3_gaugefix_sweep from in_x again; with_active = 1: the odd chains inactive (active =
//      1, 0, 1, ...), 0: no active array; with_g = 1: accumulating into a copy of in_g.  The two fields go to out_x and
//      the two G to out_g (with_g = 0: in_g unchanged);
//   2: out_cond = l2q_su3_gauge_condition of in_x, [nb][2];
//   4: out_apply = l2q_su3_gauge_apply of in_x with in_g.
#include <cstdarg>
#include <cstring>
#include <string>
#include "su3_gaugefix.hip"
namespace l2q {
static char g_err[512];
void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
Tuning& tuning() { static Tuning t; return t; }
void launch_finalize(const double* partial, double* out, int nb, long nblk, int ncomp, double scale, double offset, hipStream_t) {
  for (int c = 0; c < nb; ++c) for (int k = 0; k < ncomp; ++k) { double s = 0; for (long b = 0; b < nblk; ++b) s += partial[(c * nblk + b) * ncomp + k]; out[c * ncomp + k] = scale * s + offset; }
}
}
extern "C" const char* l2q_last_error() { return l2q::g_err; }
static std::vector<double> rd(const char* f) { FILE* p = fopen(f, "rb"); if (!p) exit(3); fseek(p, 0, SEEK_END); long n = ftell(p); fseek(p, 0, SEEK_SET); std::vector<double> v(n / 8); if (fread(v.data(), 8, v.size(), p) != v.size()) exit(3); fclose(p); return v; }
static void wr(const char* f, const std::vector<double>& v) { FILE* p = fopen(f, "wb"); fwrite(v.data(), 8, v.size(), p); fclose(p); }
static int fail(int rc) { fprintf(stderr, "rc %d %s\n", rc, l2q_last_error()); return 1; }
int main(int argc, char** argv) {
  if (argc != 18) { fprintf(stderr, "usage: see the head of gaugefix_emu.cpp\n"); return 2; }
  const int what = atoi(argv[1]);
  ++argv;
  const int nb = atoi(argv[1]), T = atoi(argv[2]), X = atoi(argv[3]), Y = atoi(argv[4]), Z = atoi(argv[5]);
  l2q::tuning().xcd_swizzle = atoi(argv[6]);
  const int dirmask = atoi(argv[7]);
  const double omega = atof(argv[8]);
  const bool with_g = atoi(argv[9]) != 0;
  const bool with_active = atoi(argv[10]) != 0;
  const std::vector<double> x = rd(argv[11]), g = rd(argv[12]);
  const long V = (long)T * X * Y * Z, nblk = (V + 255) / 256;
  if (x.size() != (size_t)nb * 72 * V || g.size() != (size_t)nb * 18 * V) { fprintf(stderr, "bad field size\n"); return 3; }
  std::vector<int> active(nb);
  for (int c = 0; c < nb; ++c) active[c] = c % 2 == 0;
  std::vector<double> ox, og;
  for (int parity = 0; parity < 2 && (what & 1); ++parity) {
    std::vector<double> f = x, h = g;
    const int rc = l2q_su3_gaugefix_sweep(f.data(), with_g ? h.data() : nullptr, with_active ? active.data() : nullptr, dirmask, parity, omega, nb, T, X, Y, Z, nullptr);
    if (rc) return fail(rc);
    ox.insert(ox.end(), f.begin(), f.end());
    og.insert(og.end(), h.begin(), h.end());
  }
  std::vector<double> cond(2 * nb, -7.0), ws(nb * nblk * 2, -7.0), ap(x.size(), -7.0);
  int rc = 0;
  if (what & 2) rc = l2q_su3_gauge_condition(x.data(), dirmask, cond.data(), nb, T, X, Y, Z, ws.data(), ws.size() * 8, nullptr);
  if (rc) return fail(rc);
  if (what & 4) rc = l2q_su3_gauge_apply(x.data(), g.data(), ap.data(), nb, T, X, Y, Z, nullptr);
  if (rc) return fail(rc);
  wr(argv[13], ox);
  wr(argv[14], og);
  wr(argv[15], cond);
  wr(argv[16], ap);
  return 0;
}
