// TEST INFRASTRUCTURE: csrc/su3_wilson_eo.hip compiled for the host against the stand-in HIP header and the host side of
// tests/native_host/emu/ (every thread of a workgroup an OS thread; error text and tuning table of common.hip
// restated).
//   wilson_eo_emu nb nrhs T X Y Z xcd_swizzle kappa in_x in_src in_aux out_field out_norm
// reads a native-layout link field (raw float64) from in_x and, from in_src and in_aux each, the two half fields
// [parity][nb][nrhs][12][V/2] of a spinor field.  For parity = 0, 1, flags = 0, 1, 2, 3 and the four uses of the kernel
// (a, b, aux) = (1, 0, null), (-kappa^2, 1, aux), (kappa, 1, aux), (kappa, 1, aux), one after another:
//   out_field = l2q_su3_wilson_hop_eo(in_x, src of the other parity, aux of this parity, a, b, flags, parity),
//   out_norm  = its norm partials [nb][nrhs][parts].
// Every output starts as -7 in every entry, so an entry that no thread wrote shows.  Each call is repeated without the
// partials, and (with aux) with out == aux: the field must be the same bits.
#include "su3_wilson_eo.hip"
#include "emu_host.hpp"
int main(int argc, char** argv) {
  if (argc != 14) { fprintf(stderr, "usage: see the head of wilson_eo_emu.cpp\n"); return 2; }
  const int nb = atoi(argv[1]), nrhs = atoi(argv[2]), T = atoi(argv[3]), X = atoi(argv[4]), Y = atoi(argv[5]), Z = atoi(argv[6]);
  l2q::tuning().xcd_swizzle = atoi(argv[7]);
  const double kappa = atof(argv[8]);
  const std::vector<double> x = rd(argv[9]), src = rd(argv[10]), aux = rd(argv[11]);
  const long V = (long)T * X * Y * Z, Vh = V / 2, nsys = (long)nb * nrhs;
  const size_t n = (size_t)nsys * 24 * Vh;
  if (x.size() != (size_t)nb * 72 * V || src.size() != 2 * n || aux.size() != 2 * n) { fprintf(stderr, "bad field size\n"); return 3; }
  const long parts = (Vh + 255) / 256;
  const double as[4] = {1.0, -kappa * kappa, kappa, kappa}, bs[4] = {0.0, 1.0, 1.0, 1.0};
  std::vector<double> of, on;
  for (int parity = 0; parity < 2; ++parity)
    for (int flags = 0; flags < 4; ++flags)
      for (int use = 0; use < 4; ++use) {
        const double* s = src.data() + (1 - parity) * n;
        const double* a = use ? aux.data() + parity * n : nullptr;
        std::vector<double> o(n, -7.0), np(nsys * parts, -7.0);
        int rc = l2q_su3_wilson_hop_eo(x.data(), s, a, o.data(), np.data(), as[use], bs[use], flags, parity, nb, nrhs, T, X, Y, Z, nullptr);
        if (rc) return fail(rc);
        std::vector<double> o2(n, -7.0);                        // without the partials: the same field
        rc = l2q_su3_wilson_hop_eo(x.data(), s, a, o2.data(), nullptr, as[use], bs[use], flags, parity, nb, nrhs, T, X, Y, Z, nullptr);
        if (rc) return fail(rc);
        if (memcmp(o.data(), o2.data(), n * sizeof(double)) != 0) { fprintf(stderr, "the fused norm changed the field\n"); return 4; }
        if (a) {                                                // out == aux: the same field
          std::vector<double> o3(a, a + n);
          rc = l2q_su3_wilson_hop_eo(x.data(), s, o3.data(), o3.data(), nullptr, as[use], bs[use], flags, parity, nb, nrhs, T, X, Y, Z, nullptr);
          if (rc) return fail(rc);
          if (memcmp(o.data(), o3.data(), n * sizeof(double)) != 0) { fprintf(stderr, "out == aux changed the field\n"); return 4; }
        }
        of.insert(of.end(), o.begin(), o.end());
        on.insert(on.end(), np.begin(), np.end());
      }
  wr(argv[12], of);
  wr(argv[13], on);
  return 0;
}
