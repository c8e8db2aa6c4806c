// TEST INFRASTRUCTURE: the host side that a driver of tests/native_host/*_emu/ needs around the csrc/su3_*.hip it
// compiles for the host: what that file takes from common.hip (error text, tuning table, the second reduction stage,
// the zeroing launch) restated plainly, and the raw float64 file I/O of the driver's main.  Included by a driver AFTER
// the .hip under test; a definition that the file does not call goes unused.
#pragma once
#include <cstdarg>
#include <cstring>
#include <string>
namespace l2q {
inline char g_err[512];
void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
Tuning& tuning() { static Tuning t; return t; }
void launch_finalize(const double* partial, double* out, int nb, long nblk, int ncomp, double scale, double offset, hipStream_t) {
  for (int c = 0; c < nb; ++c) for (int k = 0; k < ncomp; ++k) { double s = 0; for (long b = 0; b < nblk; ++b) s += partial[(c * nblk + b) * ncomp + k]; out[c * ncomp + k] = scale * s + offset; }
}
void launch_zero(void* p, size_t bytes, hipStream_t) { memset(p, 0, bytes); }
}
extern "C" const char* l2q_last_error() { return l2q::g_err; }
inline std::vector<double> rd(const char* f) { FILE* p = fopen(f, "rb"); if (!p) exit(3); fseek(p, 0, SEEK_END); long n = ftell(p); fseek(p, 0, SEEK_SET); std::vector<double> v(n / 8); if (fread(v.data(), 8, v.size(), p) != v.size()) exit(3); fclose(p); return v; }
inline void wr(const char* f, const std::vector<double>& v) { FILE* p = fopen(f, "wb"); fwrite(v.data(), 8, v.size(), p); fclose(p); }
inline int fail(int rc) { fprintf(stderr, "rc %d %s\n", rc, l2q_last_error()); return 1; }
