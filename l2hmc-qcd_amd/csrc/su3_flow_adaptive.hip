// su3_flow_adaptive.hip -- one third-order Wilson-flow step together with the distance to the second-order
// result embedded in it: what a step-size controller needs (Fritzsch & Ramos, arXiv:1301.4388, App. D).
//
// Notation of l2q_su3_flow_step: G_i = TAH(W_i A(W_i)), Z_i = -eps G_i, and the low-storage generators kept
// apart, P1 = G0, P2 = P1 - 32/17 G1, P3 = P2 + 27/17 G2.  From the same force evaluations
//   W3 = exp(-17 eps/36 P3) W2                           (third order: the step itself)
//   W' = exp(-Z0 + 2 Z1) W0 = exp(eps/16 (17 P2 - P1)) W0     (second order)
//   d_c = max over mu, x of |W3 - W'|_F / 9              (9 = N^2)
// The last kernel of the step forms both products in registers, stores W3 only and reduces d: 864 B per link
// (W0, W2, P1, P2, P3 read, W3 written) against the 1296 B of two expm_mul launches and a distance pass.
#include <cfloat>

#include "su3_launch.hpp"

namespace l2q {

// Thread per link, indexed as su3_expm_mul_kernel: block = (f = chain * 4 + mu, 256 sites).  The two exponentials
// run one after the other, each in a run-time conditional that is always taken (`lo` = 0 is a kernel ARGUMENT, as
// in su3_expm_mul_body), so that hipcc allocates them one after the other: only the 18 values of W' live across the
// second.  A link whose distance is not finite (NaN or inf in any of the five inputs) reports +inf: fmax drops
// a NaN and would hide it.  partial[f * nblk + blk] = max over the block's links of |W3 - W'|_F^2.
__global__ __launch_bounds__(kBlock, 2) void su3_flow_step_err_kernel(
    const double2* __restrict__ w0, const double2* __restrict__ w2, const double2* __restrict__ p1,
    const double2* __restrict__ p2, const double2* __restrict__ p3, double s3, double sp, double2* __restrict__ out,
    int V, long nblk, int lo, double* __restrict__ partial) {
  __shared__ double lds[4];
  const long f = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int s = (int)blk * kBlock + threadIdx.x;
  double dv = 0.0;
  if (s < V) {
    const long base = f * 9L * V;
    M3 wp, e, x;
    load_link(e, p2 + base, V, s);
    load_link(x, p1 + base, V, s);
    if (s >= lo) {
      M3 a;
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        a.re[i] = (17.0 * e.re[i] - x.re[i]) * sp;
        a.im[i] = (17.0 * e.im[i] - x.im[i]) * sp;
      }
      m3_expm(e, a);
    }
    load_link(x, w0 + base, V, s);
    if (s >= lo) m3_mul_nn(wp, e, x);
    load_link(e, p3 + base, V, s);
    if (s >= lo) {
      M3 a;
#pragma unroll
      for (int i = 0; i < 9; ++i) { a.re[i] = e.re[i] * s3; a.im[i] = e.im[i] * s3; }
      m3_expm(e, a);
    }
    load_link(x, w2 + base, V, s);
    if (s >= lo) {
      M3 r;
      m3_mul_nn(r, e, x);
      store_link(out + base, V, s, r);
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const double dr = r.re[i] - wp.re[i], di = r.im[i] - wp.im[i];
        dv = fma(dr, dr, dv);
        dv = fma(di, di, dv);
      }
      if (!(dv <= DBL_MAX)) dv = HUGE_VAL;
    }
  }
  const double bm = block_max(dv, lds);
  if (threadIdx.x == 0) partial[f * nblk + blk] = bm;
}

// d[c] = sqrt(max of the chain's n partials) / 9; one block per chain (the pattern of check_finalize_kernel)
__global__ __launch_bounds__(kBlock) void su3_flow_err_finalize_kernel(const double* __restrict__ partial, long n,
                                                                       double* __restrict__ d) {
  __shared__ double lds[4];
  const long c = blockIdx.x;
  double m = 0.0;
  for (long b = threadIdx.x; b < n; b += blockDim.x) m = fmax(m, partial[c * n + b]);
  const double tm = block_max(m, lds);
  if (threadIdx.x == 0) d[c] = sqrt(tm) / 9.0;
}

size_t flow_step_err_ws_bytes(int nb, long V) { return (size_t)nb * 4 * cdiv(V, kBlock) * sizeof(double); }

// The last kernel of the step on fields of V sites per chain: eps is the step size, the five inputs are only read.
int launch_flow_step_err(const void* w0, const void* w2, const void* p1, const void* p2, const void* p3, double eps,
                         void* x_out, double* d, int nb, long V, void* ws, size_t ws_bytes, hipStream_t st) {
  const char* what = "l2q_su3_flow_step_err";
  L2Q_REQUIRE_W(w0 && w2 && p1 && p2 && p3 && x_out && d && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE_W(su3_field_ok(nb, V) && (double)V * 36.0 < 2.0e9, L2Q_EINVAL, "bad size");
  L2Q_REQUIRE_W(x_out != w0 && x_out != w2 && x_out != p1 && x_out != p2 && x_out != p3, L2Q_EINVAL,
                "x_out must not alias an input");
  L2Q_REQUIRE_W(ws_bytes >= flow_step_err_ws_bytes(nb, V), L2Q_ESHAPE, "workspace too small");
  const long nblk = cdiv(V, kBlock);
  hipLaunchKernelGGL(su3_flow_step_err_kernel, dim3((unsigned)(nb * 4L * nblk)), dim3(kBlock), 0, st,
                     (const double2*)w0, (const double2*)w2, (const double2*)p1, (const double2*)p2,
                     (const double2*)p3, -(17.0 / 36.0) * eps, eps / 16.0, (double2*)x_out, (int)V, nblk, 0,
                     (double*)ws);
  hipLaunchKernelGGL(su3_flow_err_finalize_kernel, dim3((unsigned)nb), dim3(kBlock), 0, st, (const double*)ws,
                     4 * nblk, d);
  return check_launch(what);
}

}  // namespace l2q

using namespace l2q;

extern "C" {

size_t l2q_su3_flow_step_err_ws_bytes(int nb, int T, int X, int Y, int Z) {
  if (!su3_dims_ok(nb, T, X, Y, Z)) return 0;
  return flow_step_err_ws_bytes(nb, (long)T * X * Y * Z);
}

int l2q_su3_flow_step_err(const void* x_in, void* x_out, void* ws_p3, void* ws_x, double eps, double* d, int nb,
                          int T, int X, int Y, int Z, void* ws, size_t ws_bytes, void* stream) {
  L2Q_REQUIRE(x_in && x_out && ws_p3 && ws_x && d && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(su3_dims_ok(nb, T, X, Y, Z), L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(x_out != x_in && x_out != ws_x && x_in != ws_x, L2Q_EINVAL,
              "x_in, x_out and ws_x must be three different fields");
  const long V = (long)T * X * Y * Z;
  const size_t field = (size_t)nb * 36 * V * sizeof(double2);
  char* p1 = (char*)ws_p3;
  char* p2 = p1 + field;
  char* p3 = p2 + field;
  const auto in_p = [=](const void* q) { return (const char*)q >= p1 && (const char*)q < p3 + field; };
  L2Q_REQUIRE(!in_p(x_in) && !in_p(x_out) && !in_p(ws_x), L2Q_EINVAL, "ws_p3 must not alias the links");
  L2Q_REQUIRE(ws_bytes >= flow_step_err_ws_bytes(nb, V), L2Q_ESHAPE, "workspace too small");
  // W1 = exp(-eps/4 P1) W0 -> x_out;  W2 = exp(17 eps/36 P2) W1 -> ws_x;  P3;  then W3 -> x_out and d from the kernel
  int rc = l2q_su3_flow_stage(x_in, nullptr, 1.0, -0.25 * eps, p1, x_out, nb, T, X, Y, Z, stream);
  if (rc != L2Q_OK) return rc;
  rc = l2q_su3_flow_stage(x_out, p1, -32.0 / 17.0, (17.0 / 36.0) * eps, p2, ws_x, nb, T, X, Y, Z, stream);
  if (rc != L2Q_OK) return rc;
  rc = l2q_su3_force_kick_to(ws_x, 3.0, 27.0 / 17.0, p2, p3, nb, T, X, Y, Z, stream);
  if (rc != L2Q_OK) return rc;
  return launch_flow_step_err(x_in, ws_x, p1, p2, p3, eps, x_out, d, nb, V, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
