// gemm_digits.hip -- the int8-sliced fp64 input layer of gemm_sliced.hip with BOTH operands given as digit images:
//     C[M][N] = epilogue( A[M][K] . W[N][K]^T + A2[M][K2] . W2[N][K2]^T + bias + bias2 ),
// W / W2 as the weight images of l2q_gemm_sliced_build, A / A2 as activation digit images (digits.hpp) written by
// the kernels that produce the activations (su3_kernels.hip: the projection and the x-update hold the eight values
// of a link in registers) or by l2q_gemm_digits_slice below.  gemm_sliced_kernel loads every 64-row strip of the fp64
// activations and recodes it in each of its N / 64 column-tile workgroups; here the digits are made once, cost 7 bytes
// per value instead of 8, and reach LDS by LDS-DMA like the weights.
//
// Same digits, the same slab loop and launcher (sliced_core.hpp: the same int32 sums over the same k-ranges, the same
// fp64 Horner combination) and the same reduce kernel as l2q_gemm_sliced_f64: the output has the same BITS
// (tests/test_gemm_digits_gpu.py).
//
// Kernel.  512 threads: four matrix wavefronts on a 64 x 64 tile (gs_slab_loop), and four loader wavefronts that only
// issue LDS-DMA: per slab each moves 7 of the 28 activation fragments (one slab ahead, two LDS stages) and 7 of the 28
// weight fragments (two slabs ahead, three stages); the matrix wavefronts issue no memory instruction in the loop.
// One barrier per slab; a loader waits vmcnt(7) in front of it (the weight pieces of the slab after next stay in
// flight).  An activation fragment is gathered by the DMA's per-lane source address: lane 4 r + c fetches the 16-byte
// chunk g = c ^ 2 (r >> 3) of row r's plane (four adjacent lanes = 64 contiguous bytes), and a matrix lane (r, g)
// reads slot 4 r + (g ^ 2 (r >> 3)): conflict-free for the 16-lane groups of ds_read_b128 by enumeration.
#include "sliced_core.hpp"

namespace l2q {

#ifndef L2Q_GD_EXP
#define L2Q_GD_EXP 0          // 64: print the shader clock per slab and the matrix wavefronts' barrier wait
#endif

// ---- fp64 [M][K] -> digit image ---------------------------------------------------------------------------
// thread <-> (row, slab, dword of a plane): four values, one dword of each of the seven planes
__global__ __launch_bounds__(256) void gd_slice_kernel(const double* __restrict__ A, long M, long K, double sc, double lim,
                                                        char* __restrict__ image, int* __restrict__ flag) {
  const long t = blockIdx.x * 256L + threadIdx.x;
  const long nslab = K / 64;
  int bad = 0;
  if (t < M * nslab * 16) {
    const int Q = (int)(t & 15), g = Q >> 2, jh = Q & 3;
    const long slab = (t >> 4) % nslab, row = (t >> 4) / nslab;
    const double* src = A + row * K + slab * 64 + 16 * jh + 2 * g;
    const double2 v0 = *reinterpret_cast<const double2*>(src), v1 = *reinterpret_cast<const double2*>(src + 8);
    const double x[4] = {v0.x, v0.y, v1.x, v1.y};
    unsigned lo[4], hi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bad |= gd_digits(x[i], sc, lim, lo[i], hi[i]);
    unsigned* dst = reinterpret_cast<unsigned*>(image + (row * nslab + slab) * GD_SLAB) + Q;
#pragma unroll
    for (int s = 0; s < GS_NS; ++s) {
      const int b = s < 4 ? 3 - s : 6 - s;                  // digit s: byte 3 - s of hi, or byte 6 - s of lo
      unsigned d = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) d |= (((s < 4 ? hi[i] : lo[i]) >> (8 * b)) & 0xffu) << (8 * i);
      dst[16 * s] = d;
    }
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

__global__ __launch_bounds__(512, 1) void gemm_digits_kernel(GsArgs a, int swz) {
  // two stages of activation digits (one slab ahead), three of weight digits (two slabs ahead)
  __shared__ __attribute__((aligned(1024))) char lds[GS_LDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const GsTile t = gs_tile(a, swz);
  const int nslab = t.nslab;

  if (wave < 4) {
    // ================================================================ matrix wavefronts
    const int wm = wave >> 1, wn = wave & 1;
    GsClock<(L2Q_GD_EXP & 64) != 0> clk;
    __builtin_amdgcn_s_setprio(3);
    // (activation fragment: lane (r, g) reads slot 4 r + (g ^ 2 (r >> 3)), see the loaders)
    const int fr = lane & 15, fg = lane >> 4;
    const char* abase = lds + (2 * wm) * (GS_NS * GS_FRAG) + (4 * fr + (fg ^ ((fr >> 3) * 2))) * 16;
    const char* bbase = lds + 2 * GS_OPER + (2 * wn) * (GS_NS * GS_FRAG) + lane * 16;
    double racc[4][4];
    auto barrier = []() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    gs_slab_loop<L2Q_GD_EXP & 64>(abase, bbase, nslab, racc, [&]() { clk.timed(barrier); }, [](int, int) {});
    clk.print(wave, lane, nslab);
    gs_store_part(a, t, wm, wn, lane, racc);
    return;
  }

  // ================================================================== loader wavefronts
  // Loader h moves row tile h of the activations (its seven planes) and the weight fragments h, h + 4, ..., h + 24.
  // Period p (between B(p - 1) and B(p)) issues A(p) into activation stage p & 1 and W(p + 1) into weight stage
  // (p + 1) % 3: both held slab p - 2, whose reads the matrix wavefronts retired (lgkmcnt(0)) in front of B(p - 1).
  // vmcnt counts in issue order: vmcnt(7) in front of B(p) leaves only the seven pieces of W(p + 1) in flight.
  const int h = wave - 4;
  const long aslabs = t.K / 64;
  const int lr = lane >> 2, lc = lane & 3;
  const char* asrc = (const char*)a.A[t.op] + (((long)t.tm * GS_T + h * 16 + lr) * aslabs + t.kbeg / 64) * GD_SLAB +
                     (lc ^ ((lr >> 3) * 2)) * 16;
  const char* bsrc = gs_wsrc(a, t, lane);
  const long bstep = gs_wstep(t);
  auto dma_a = [&](int q) {
#pragma unroll
    for (int s = 0; s < GS_NS; ++s)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(asrc + (long)q * GD_SLAB + s * 64),
                                       (gs_lds_ptr_t)(lds + (q & 1) * GS_OPER + (h * GS_NS + s) * GS_FRAG), 16, 0, 0);
  };
  auto dma_b = [&](int q) {
#pragma unroll
    for (int f = 0; f < GS_NS; ++f) {
      const int frag = h + 4 * f;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bsrc + (long)q * bstep + frag * GS_FRAG),
                                       (gs_lds_ptr_t)(lds + (2 + q % 3) * GS_OPER + frag * GS_FRAG), 16, 0, 0);
    }
  };
  if (nslab > 0) {
    dma_a(0);
    dma_b(0);
    for (int p = 0; p < nslab; ++p) {
      if (p > 0) dma_a(p);
      if (p + 1 < nslab) {
        dma_b(p + 1);
        asm volatile("s_waitcnt vmcnt(7)\n\ts_barrier" ::: "memory");          // B(p)
      } else {
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");          // B(nslab - 1): nothing stays in flight
      }
    }
  }
}

}  // namespace l2q

using namespace l2q;

extern "C" {

size_t l2q_gemm_digits_bytes(long M, long K) {
  if (M <= 0 || K <= 0 || K % 64 != 0) return 0;
  return (size_t)M * (size_t)(K / 64) * GD_SLAB;
}

int l2q_gemm_digits_slice(const double* A, long M, long K, int a_exp, void* image, size_t image_bytes, void* stream) {
  L2Q_REQUIRE(A && image, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(M > 0 && K > 0 && K % 64 == 0, L2Q_EINVAL, "the digit image serves K % 64 == 0");
  L2Q_REQUIRE(a_exp > -900 && a_exp < 900, L2Q_EINVAL, "bad operand exponent");
  L2Q_REQUIRE(image_bytes >= l2q_gemm_digits_bytes(M, K), L2Q_ESHAPE, "buffer too small");
  L2Q_REQUIRE((reinterpret_cast<uintptr_t>(A) & 15) == 0 && (reinterpret_cast<uintptr_t>(image) & 15) == 0, L2Q_ESHAPE,
              "A and the image must be 16-byte aligned");
  int* flag = gs_flag();
  L2Q_REQUIRE(flag, L2Q_EHIP, "device symbol gs_flag_dev not found");
  const long nthr = M * (K / 64) * 16;
  hipLaunchKernelGGL(gd_slice_kernel, dim3((unsigned)cdiv(nthr, 256)), dim3(256), 0, (hipStream_t)stream, A, M, K,
                     ldexp(1.0, GS_BITS - a_exp), ldexp(1.0, a_exp), (char*)image, flag);
  return check_launch("l2q_gemm_digits_slice");
}

int l2q_gemm_digits_f64(const void* A, const void* image, long K, int a_exp, const void* A2, const void* image2,
                        long K2, int a2_exp, int M, int N, const double* bias, const double* bias2,
                        const double* coeff, double scale, int act, double* C, void* ws, size_t ws_bytes,
                        void* stream) {
  return gs_launch("l2q_gemm_digits_f64", gemm_digits_kernel,
                   "activation images must be 16-byte aligned (weight images and workspace 256-byte)", A, image, K, a_exp,
                   A2, image2, K2, a2_exp, M, N, bias, bias2, coeff, scale, act, C, ws, ws_bytes, stream);
}

}  // extern "C"
