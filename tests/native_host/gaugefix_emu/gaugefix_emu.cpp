// TEST INFRASTRUCTURE: csrc/su3_gaugefix.hip compiled for the host against the stand-in HIP header and the host side of
// tests/native_host/emu/ (every thread of a workgroup an OS thread; error text, tuning table and the second reduction
// stage of common.hip restated).
//   gaugefix_emu what nb T X Y Z xcd_swizzle dirmask omega with_g with_active in_x in_g out_x out_g out_cond out_apply
// reads a native-layout field (raw float64) from in_x and a transformation G[nb][9][V] from in_g; `what` is a sum of
//   1: for parity 0, 1 one l2q_su3_gaugefix_sweep from in_x again; with_active = 1: the odd chains inactive (active =
//      1, 0, 1, ...), 0: no active array; with_g = 1: accumulating into a copy of in_g.  The two fields go to out_x and
//      the two G to out_g (with_g = 0: in_g unchanged);
//   2: out_cond = l2q_su3_gauge_condition of in_x, [nb][2];
//   4: out_apply = l2q_su3_gauge_apply of in_x with in_g.
#include "su3_gaugefix.hip"
#include "emu_host.hpp"
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
