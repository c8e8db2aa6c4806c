// TEST INFRASTRUCTURE: csrc/su3_wilson_f32.hip compiled for the host against the stand-in HIP header and the host side of
// tests/native_host/emu/ (every thread of a workgroup an OS thread; error text and tuning table of common.hip
// restated), float2 from hip_f32.hpp beside this file.
//   wilson_f32_emu nb nrhs T X Y Z xcd_swizzle kappa in_x in_src in_aux in_f64 in_scal
//                  out_links out_field out_norm out_blas32 out_blas64
// in_x: native links (raw float64); in_src, in_aux: the two half fields [parity][nb][nrhs][12][V/2] of a spinor field
// as float2; in_f64: one half field as double2; in_scal: alpha, beta, scale, [3][nb * nrhs] doubles.
// out_links = l2q_su3_links_demote_eo(in_x), which the hops then read.  For parity = 0, 1, flags = 0..3 and the four
// uses (a, b, aux) = (1, 0, null), (-kappa^2, 1, aux), (kappa, 1, aux), (kappa, 1, aux), one after another:
//   out_field = l2q_su3_wilson_hop_eo_f32(links, src of the other parity, aux of this parity, a, b, flags, parity),
//   out_norm  = its norm partials [nb][nrhs][parts].
// Every output starts as -7 in every entry, so an entry that no thread wrote shows.  Each call is repeated without the
// partials, and (with aux) with out == aux: the field must be the same bits.
// out_blas32: x, r after l2q_su3_spinor_cg_update_f32(x = src[0], r = src[1], p = aux[0], q = aux[1], alpha), then p
// after l2q_su3_spinor_xpay_f32(p = aux[0], z = aux[1], beta), then l2q_su3_spinor_demote(in_f64, scale);
// out_blas64: the update's partials [nb][nrhs][parts], then in_f64 after l2q_su3_spinor_promote_axpy(in_f64, src[0], scale).
#include "hip_f32.hpp"
#include "su3_wilson_f32.hip"
#include "emu_host.hpp"
static std::vector<float> rdf(const char* f) { const std::vector<double> d = rd(f); std::vector<float> v(2 * d.size()); memcpy(v.data(), d.data(), 8 * d.size()); return v; }
static void wrf(const char* f, const std::vector<float>& v) { FILE* p = fopen(f, "wb"); fwrite(v.data(), 4, v.size(), p); fclose(p); }
int main(int argc, char** argv) {
  if (argc != 19) { fprintf(stderr, "usage: see the head of wilson_f32_emu.cpp\n"); return 2; }
  const int nb = atoi(argv[1]), nrhs = atoi(argv[2]), T = atoi(argv[3]), X = atoi(argv[4]), Y = atoi(argv[5]), Z = atoi(argv[6]);
  l2q::tuning().xcd_swizzle = atoi(argv[7]);
  const double kappa = atof(argv[8]);
  const std::vector<double> x = rd(argv[9]), f64 = rd(argv[12]), scal = rd(argv[13]);
  const std::vector<float> src = rdf(argv[10]), aux = rdf(argv[11]);
  const long V = (long)T * X * Y * Z, Vh = V / 2, nsys = (long)nb * nrhs;
  const size_t n = (size_t)nsys * 24 * Vh;
  if (x.size() != (size_t)nb * 72 * V || src.size() != 2 * n || aux.size() != 2 * n || f64.size() != n ||
      scal.size() != (size_t)3 * nsys) { fprintf(stderr, "bad field size\n"); return 3; }
  const long parts = (Vh + 255) / 256;
  std::vector<float> links((size_t)nb * 72 * V, -7.0f);                  // [nb][2][4][9][V/2] float2
  int rc = l2q_su3_links_demote_eo(x.data(), links.data(), nb, T, X, Y, Z, nullptr);
  if (rc) return fail(rc);
  wrf(argv[14], links);
  const double as[4] = {1.0, -kappa * kappa, kappa, kappa}, bs[4] = {0.0, 1.0, 1.0, 1.0};
  std::vector<float> of;
  std::vector<double> on;
  for (int parity = 0; parity < 2; ++parity)
    for (int flags = 0; flags < 4; ++flags)
      for (int use = 0; use < 4; ++use) {
        const float* s = src.data() + (1 - parity) * n;
        const float* a = use ? aux.data() + parity * n : nullptr;
        std::vector<float> o(n, -7.0f);
        std::vector<double> np(nsys * parts, -7.0);
        rc = l2q_su3_wilson_hop_eo_f32(links.data(), s, a, o.data(), np.data(), as[use], bs[use], flags, parity, nb, nrhs, T, X, Y, Z, nullptr);
        if (rc) return fail(rc);
        std::vector<float> o2(n, -7.0f);                        // without the partials: the same field
        rc = l2q_su3_wilson_hop_eo_f32(links.data(), s, a, o2.data(), nullptr, as[use], bs[use], flags, parity, nb, nrhs, T, X, Y, Z, nullptr);
        if (rc) return fail(rc);
        if (memcmp(o.data(), o2.data(), n * sizeof(float)) != 0) { fprintf(stderr, "the fused norm changed the field\n"); return 4; }
        if (a) {                                                // out == aux: the same field
          std::vector<float> o3(a, a + n);
          rc = l2q_su3_wilson_hop_eo_f32(links.data(), s, o3.data(), o3.data(), nullptr, as[use], bs[use], flags, parity, nb, nrhs, T, X, Y, Z, nullptr);
          if (rc) return fail(rc);
          if (memcmp(o.data(), o3.data(), n * sizeof(float)) != 0) { fprintf(stderr, "out == aux changed the field\n"); return 4; }
        }
        of.insert(of.end(), o.begin(), o.end());
        on.insert(on.end(), np.begin(), np.end());
      }
  wrf(argv[15], of);
  wr(argv[16], on);
  // the BLAS-1 kernels, demote and promote
  const double *alpha = scal.data(), *beta = alpha + nsys, *scale = beta + nsys;
  std::vector<float> xs(src.begin(), src.begin() + n), rs(src.begin() + n, src.end()), ps(aux.begin(), aux.begin() + n);
  const float* qs = aux.data() + n;
  std::vector<double> part(nsys * parts, -7.0), x64(f64);
  std::vector<float> dem(n, -7.0f);
  rc = l2q_su3_spinor_cg_update_f32(xs.data(), rs.data(), ps.data(), qs, alpha, part.data(), nsys, Vh, nullptr);
  if (rc) return fail(rc);
  rc = l2q_su3_spinor_xpay_f32(ps.data(), qs, beta, nsys, Vh, nullptr);
  if (rc) return fail(rc);
  rc = l2q_su3_spinor_demote(f64.data(), scale, dem.data(), nsys, Vh, nullptr);
  if (rc) return fail(rc);
  rc = l2q_su3_spinor_promote_axpy(x64.data(), src.data(), scale, nsys, Vh, nullptr);
  if (rc) return fail(rc);
  std::vector<float> b32(xs);
  b32.insert(b32.end(), rs.begin(), rs.end());
  b32.insert(b32.end(), ps.begin(), ps.end());
  b32.insert(b32.end(), dem.begin(), dem.end());
  wrf(argv[17], b32);
  part.insert(part.end(), x64.begin(), x64.end());
  wr(argv[18], part);
  return 0;
}
