// TEST INFRASTRUCTURE: csrc/su3_wilson_clover.hip compiled for the host against the stand-in HIP header and the host side
// of tests/native_host/emu/ (every thread of a workgroup an OS thread; error text and tuning table of common.hip
// restated).
//   wilson_clover_emu nb nrhs T X Y Z xcd_swizzle kappa coef in_x in_src in_aux in_a in_ainv
//                     out_cl out_clinv out_parts out_field out_norm out_apply out_apply_norm
// reads a native-layout link field (raw float64) from in_x, from in_src and in_aux each the two half fields
// [parity][nb][nrhs][12][V/2] of a spinor field, and from in_a and in_ainv two block fields [nb][2][2][36][V/2].
//   out_cl     = l2q_su3_clover_term(in_x, coef)
//   out_clinv  = l2q_su3_clover_invert(in_a), out_parts = its smallest-pivot partials, then its log-det partials, each
//                [nb][2][parts]; the call is repeated without the log-det partials: the same bits
//   out_field  = for parity = 0, 1, flags = 0..3 and the six uses (cmode, block, a, b, aux) of the hop kernel
//                  (0, none, 1, 0, null), (0, none, kappa, 1, aux), (2, in_ainv, 1, 0, null), (1, in_a, -kappa^2, 1, aux),
//                  (2, in_ainv, kappa, 1, aux), (1, in_a, -kappa, 1, aux)
//                l2q_su3_wilson_clover_hop_eo(in_x, src of the other parity, aux of this parity, ...), out_norm its norm
//                partials [nb][nrhs][parts].  At flags 3 each call is repeated without the partials and (with aux) with out == aux.
//   out_apply  = for parity = 0, 1: l2q_su3_clover_apply(in_ainv, src of this parity), out_apply_norm its partials; repeated
//                in place.
// Every output starts as -7 in every entry, so an entry that no thread wrote shows.
#include "su3_wilson_clover.hip"
#include "emu_host.hpp"
int main(int argc, char** argv) {
  if (argc != 22) { fprintf(stderr, "usage: see the head of wilson_clover_emu.cpp\n"); return 2; }
  const int nb = atoi(argv[1]), nrhs = atoi(argv[2]), T = atoi(argv[3]), X = atoi(argv[4]), Y = atoi(argv[5]), Z = atoi(argv[6]);
  l2q::tuning().xcd_swizzle = atoi(argv[7]);
  const double kappa = atof(argv[8]), coef = atof(argv[9]);
  const std::vector<double> x = rd(argv[10]), src = rd(argv[11]), aux = rd(argv[12]), ca = rd(argv[13]), ci = rd(argv[14]);
  const long V = (long)T * X * Y * Z, Vh = V / 2, nsys = (long)nb * nrhs;
  const size_t n = (size_t)nsys * 24 * Vh, ncl = (size_t)nb * 4 * 36 * Vh;
  if (x.size() != (size_t)nb * 72 * V || src.size() != 2 * n || aux.size() != 2 * n || ca.size() != ncl || ci.size() != ncl) {
    fprintf(stderr, "bad field size\n");
    return 3;
  }
  const long parts = (Vh + 255) / 256;
  int rc;
  {
    std::vector<double> cl(ncl, -7.0);
    if ((rc = l2q_su3_clover_term(x.data(), cl.data(), coef, nb, T, X, Y, Z, nullptr))) return fail(rc);
    wr(argv[15], cl);
  }
  {
    std::vector<double> inv(ncl, -7.0), inv2(ncl, -7.0), pp(2 * nb * 2 * parts, -7.0), mp2(nb * 2 * parts, -7.0);
    if ((rc = l2q_su3_clover_invert(ca.data(), inv.data(), pp.data(), pp.data() + nb * 2 * parts, nb, T, X, Y, Z, nullptr))) return fail(rc);
    if ((rc = l2q_su3_clover_invert(ca.data(), inv2.data(), mp2.data(), nullptr, nb, T, X, Y, Z, nullptr))) return fail(rc);
    if (memcmp(inv.data(), inv2.data(), ncl * sizeof(double)) != 0 || memcmp(pp.data(), mp2.data(), mp2.size() * sizeof(double)) != 0) {
      fprintf(stderr, "the log-det partials changed the inverse\n");
      return 4;
    }
    wr(argv[16], inv);
    wr(argv[17], pp);
  }
  const int cmodes[6] = {0, 0, 2, 1, 2, 1};
  const double* blocks[6] = {nullptr, nullptr, ci.data(), ca.data(), ci.data(), ca.data()};
  const double as[6] = {1.0, kappa, 1.0, -kappa * kappa, kappa, -kappa}, bs[6] = {0.0, 1.0, 0.0, 1.0, 1.0, 1.0};
  const bool with_aux[6] = {false, true, false, true, true, true};
  std::vector<double> of, on;
  for (int parity = 0; parity < 2; ++parity)
    for (int flags = 0; flags < 4; ++flags)
      for (int use = 0; use < 6; ++use) {
        const double* s = src.data() + (1 - parity) * n;
        const double* a = with_aux[use] ? aux.data() + parity * n : nullptr;
        std::vector<double> o(n, -7.0), np(nsys * parts, -7.0);
        rc = l2q_su3_wilson_clover_hop_eo(x.data(), s, a, blocks[use], o.data(), np.data(), as[use], bs[use], flags, parity, cmodes[use], nb, nrhs, T, X, Y, Z, nullptr);
        if (rc) return fail(rc);
        if (flags != 3) { of.insert(of.end(), o.begin(), o.end()); on.insert(on.end(), np.begin(), np.end()); continue; }
        std::vector<double> o2(n, -7.0);                        // without the partials: the same field
        rc = l2q_su3_wilson_clover_hop_eo(x.data(), s, a, blocks[use], o2.data(), nullptr, as[use], bs[use], flags, parity, cmodes[use], nb, nrhs, T, X, Y, Z, nullptr);
        if (rc) return fail(rc);
        if (memcmp(o.data(), o2.data(), n * sizeof(double)) != 0) { fprintf(stderr, "the fused norm changed the field\n"); return 4; }
        if (a) {                                                // out == aux: the same field
          std::vector<double> o3(a, a + n);
          rc = l2q_su3_wilson_clover_hop_eo(x.data(), s, o3.data(), blocks[use], o3.data(), nullptr, as[use], bs[use], flags, parity, cmodes[use], nb, nrhs, T, X, Y, Z, nullptr);
          if (rc) return fail(rc);
          if (memcmp(o.data(), o3.data(), n * sizeof(double)) != 0) { fprintf(stderr, "out == aux changed the field\n"); return 4; }
        }
        of.insert(of.end(), o.begin(), o.end());
        on.insert(on.end(), np.begin(), np.end());
      }
  wr(argv[18], of);
  wr(argv[19], on);
  std::vector<double> af, an;
  for (int parity = 0; parity < 2; ++parity) {
    const double* s = src.data() + parity * n;
    std::vector<double> o(n, -7.0), np(nsys * parts, -7.0), o2(s, s + n);
    if ((rc = l2q_su3_clover_apply(ci.data(), s, o.data(), np.data(), parity, nb, nrhs, T, X, Y, Z, nullptr))) return fail(rc);
    if ((rc = l2q_su3_clover_apply(ci.data(), o2.data(), o2.data(), nullptr, parity, nb, nrhs, T, X, Y, Z, nullptr))) return fail(rc);
    if (memcmp(o.data(), o2.data(), n * sizeof(double)) != 0) { fprintf(stderr, "the apply in place changed the field\n"); return 4; }
    af.insert(af.end(), o.begin(), o.end());
    an.insert(an.end(), np.begin(), np.end());
  }
  wr(argv[20], af);
  wr(argv[21], an);
  return 0;
}
