// TEST INFRASTRUCTURE: csrc/su3_flow_adaptive.hip compiled for the host against the stand-in HIP header and the host
// side of tests/native_host/emu/ (every thread of a workgroup an OS thread; the error text of common.hip restated, the
// rest of the host side unused).  Only the step's last kernel and its finalize are run here (l2q::launch_flow_step_err); the entry points
// that the whole step calls in other files (forward stage, force kick) are refused: their composition is the business
// of tests/test_flow_adaptive_gpu.py.
//   flow_adaptive_emu nb V eps w0 w2 p1 p2 p3 out_x out_d
// reads five native-layout fields [nb][4][9][V] complex (raw float64), writes W3 to out_x and d [nb] to out_d, and
// fails if an input changed, if the exact workspace was overrun, or if an aliased output or a short workspace passes.
#include "su3_flow_adaptive.hip"
#include "emu_host.hpp"
extern "C" {
int l2q_su3_flow_stage(const void*, const void*, double, double, void*, void*, int, int, int, int, int, void*) { return L2Q_EINVAL; }
int l2q_su3_force_kick_to(const void*, double, double, const void*, void*, int, int, int, int, int, void*) { return L2Q_EINVAL; }
}
int main(int argc, char** argv) {
  if (argc != 11) { fprintf(stderr, "usage: flow_adaptive_emu nb V eps w0 w2 p1 p2 p3 out_x out_d\n"); return 2; }
  const int nb = atoi(argv[1]);
  const long V = atol(argv[2]);
  const double eps = atof(argv[3]);
  std::vector<double> in[5];
  for (int i = 0; i < 5; ++i) {
    in[i] = rd(argv[4 + i]);
    if (in[i].size() != (size_t)nb * 72 * V) { fprintf(stderr, "bad field size\n"); return 3; }
  }
  const std::vector<double> w0 = in[0], w2 = in[1], p1 = in[2], p2 = in[3], p3 = in[4];
  std::vector<double> keep[5] = {w0, w2, p1, p2, p3};
  // the workspace at exactly the size asked for (AddressSanitizer sees one double too many), the outputs marked
  const size_t wsb = l2q::flow_step_err_ws_bytes(nb, V);
  if (wsb != (size_t)nb * 4 * ((V + 255) / 256) * 8) { fprintf(stderr, "workspace size %zu\n", wsb); return 1; }
  std::vector<double> ws(wsb / 8, -7.0), out((size_t)nb * 72 * V, -7.0), d(nb, -7.0);
  int rc = l2q::launch_flow_step_err(w0.data(), w2.data(), p1.data(), p2.data(), p3.data(), eps, out.data(), d.data(),
                                     nb, V, ws.data(), wsb, nullptr);
  if (rc) return fail(rc);
  const std::vector<double>* now[5] = {&w0, &w2, &p1, &p2, &p3};
  for (int i = 0; i < 5; ++i)
    if (memcmp(now[i]->data(), keep[i].data(), keep[i].size() * 8)) { fprintf(stderr, "input %d was written\n", i); return 1; }
  for (double v : ws) if (v == -7.0) { fprintf(stderr, "a partial was not written\n"); return 1; }
  // refused: an output that is an input, a workspace one byte short, a null pointer
  std::vector<double> o2 = out;
  for (int i = 0; i < 5; ++i)
    if (l2q::launch_flow_step_err(w0.data(), w2.data(), p1.data(), p2.data(), p3.data(), eps, (void*)now[i]->data(),
                                  d.data(), nb, V, ws.data(), wsb, nullptr) != L2Q_EINVAL) { fprintf(stderr, "aliased output accepted\n"); return 1; }
  if (l2q::launch_flow_step_err(w0.data(), w2.data(), p1.data(), p2.data(), p3.data(), eps, o2.data(), d.data(), nb, V,
                                ws.data(), wsb - 1, nullptr) != L2Q_ESHAPE) { fprintf(stderr, "short workspace accepted\n"); return 1; }
  if (l2q::launch_flow_step_err(w0.data(), w2.data(), p1.data(), p2.data(), p3.data(), eps, o2.data(), nullptr, nb, V,
                                ws.data(), wsb, nullptr) != L2Q_EINVAL) { fprintf(stderr, "null d accepted\n"); return 1; }
  wr(argv[9], out);
  wr(argv[10], d);
  return 0;
}
