// TEST INFRASTRUCTURE: csrc/su3_heatbath.hip compiled for the host against the stand-in HIP header and the host side of
// tests/native_host/emu/ (every thread of a workgroup an OS thread; error text, tuning table and the second reduction
// stage of common.hip restated).
//   heatbath_emu <hb|hb_nofails|or> nb T X Y Z xcd_swizzle beta ntry in_x in_u out_x out_fails
// reads a native-layout field (raw float64) from in_x and, for hb, the uniforms of the 8 launches (mu 0..3, parity
// 0, 1; u[8][nb][3][4 ntry + 2][V/2]) from in_u; every launch starts from in_x again.  Writes the 8 updated fields to
// out_x and the 8 x nb failure counts to out_fails.
#include "su3_heatbath.hip"
#include "emu_host.hpp"
int main(int argc, char** argv) {
  if (argc != 14) { fprintf(stderr, "usage: see the head of heatbath_emu.cpp\n"); return 2; }
  const std::string mode = argv[1];
  const int nb = atoi(argv[2]), T = atoi(argv[3]), X = atoi(argv[4]), Y = atoi(argv[5]), Z = atoi(argv[6]);
  l2q::tuning().xcd_swizzle = atoi(argv[7]);
  const double beta = atof(argv[8]);
  const int ntry = atoi(argv[9]);
  const std::vector<double> x = rd(argv[10]);
  const long V = (long)T * X * Y * Z, vh = V / 2, nblk = (vh + 255) / 256;
  const size_t per_u = (size_t)nb * 3 * (4 * ntry + 2) * vh;
  if (x.size() != (size_t)nb * 72 * V) { fprintf(stderr, "bad field size\n"); return 3; }
  std::vector<double> u;
  if (mode != "or") { u = rd(argv[11]); if (u.size() != 8 * per_u) { fprintf(stderr, "bad uniforms size\n"); return 3; } }
  std::vector<double> ox, of(8 * nb, -7.0);
  for (int mu = 0; mu < 4; ++mu)
    for (int parity = 0; parity < 2; ++parity) {
      const int l = 2 * mu + parity;
      std::vector<double> f = x, ws(nb * nblk, -7.0);
      int rc;
      if (mode == "or") rc = l2q_su3_overrelax(f.data(), mu, parity, nb, T, X, Y, Z, nullptr);
      else if (mode == "hb_nofails") rc = l2q_su3_heatbath(f.data(), beta, mu, parity, u.data() + l * per_u, ntry, nullptr, nb, T, X, Y, Z, nullptr, 0, nullptr);
      else rc = l2q_su3_heatbath(f.data(), beta, mu, parity, u.data() + l * per_u, ntry, of.data() + l * nb, nb, T, X, Y, Z, ws.data(), ws.size() * 8, nullptr);
      if (rc) return fail(rc);
      ox.insert(ox.end(), f.begin(), f.end());
    }
  wr(argv[12], ox);
  wr(argv[13], of);
  return 0;
}
