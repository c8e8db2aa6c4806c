// gemm_digits.hip -- the int8-sliced fp64 input layer of gemm_sliced.hip with BOTH operands given as digit images:
//     C[M][N] = epilogue( A[M][K] . W[N][K]^T + A2[M][K2] . W2[N][K2]^T + bias + bias2 ),
// W / W2 as the weight images of l2q_gemm_sliced_build, A / A2 as activation digit images (digits.hpp) written by
// the kernels that produce the activations (su3_kernels.hip: the projection and the x-update hold the eight values
// of a link in registers) or by l2q_gemm_digits_slice below.  gemm_sliced_kernel loads every 64-row strip of the fp64
// activations and recodes it in each of its N / 64 column-tile workgroups; here the digits are made once, cost 7 bytes
// per value instead of 8, and reach LDS by LDS-DMA like the weights.
//
// Same digits, same int32 sums over the same k-ranges (gs_klen, GD_RANGE), the same fp64 Horner combination and the
// same reduce kernel as l2q_gemm_sliced_f64: the output has the same BITS (tests/test_gemm_digits_gpu.py).
//
// Kernel.  As gemm_sliced_kernel: 512 threads, four matrix wavefronts on a 64 x 64 tile (28 ds_read_b128 and 112
// v_mfma_i32_16x16x64_i8 per 64-k slab, the reads asm with counted lgkmcnt), and four loader wavefronts that now only
// issue LDS-DMA: per slab each moves 7 of the 28 activation fragments (one slab ahead, two LDS stages) and 7 of the 28
// weight fragments (two slabs ahead, three stages); the matrix wavefronts issue no memory instruction in the loop.
// One barrier per slab; a loader waits vmcnt(7) in front of it (the weight pieces of the slab after next stay in
// flight).  An activation fragment is gathered by the DMA's per-lane source address: lane 4 r + c fetches the 16-byte
// chunk g = c ^ 2 (r >> 3) of row r's plane (four adjacent lanes = 64 contiguous bytes), and a matrix lane (r, g)
// reads slot 4 r + (g ^ 2 (r >> 3)): conflict-free for the 16-lane groups of ds_read_b128 by enumeration.
#include "digits.hpp"
#include "heads_common.hpp"

namespace l2q {

typedef int gd_v4i __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* gd_lds_ptr_t;

#ifndef L2Q_GD_EXP
#define L2Q_GD_EXP 0          // 64: print the shader clock per slab and the matrix wavefronts' barrier wait
#endif
constexpr int GD_FRAG = 1024;                  // one MFMA operand fragment: 64 lanes x 16 bytes
constexpr int GD_T = 64;                       // output tile (rows = columns)
constexpr int GD_OPER = 4 * GD_NS * GD_FRAG;   // one operand of a stage: 4 row tiles x 7 digits = 28 KB
constexpr int GD_RANGE = 16384;                // k per int32 accumulation (gemm_sliced.hip: GS_RANGE)

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
    for (int s = 0; s < GD_NS; ++s) {
      const int b = s < 4 ? 3 - s : 6 - s;                  // digit s: byte 3 - s of hi, or byte 6 - s of lo
      unsigned d = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) d |= (((s < 4 ? hi[i] : lo[i]) >> (8 * b)) & 0xffu) << (8 * i);
      dst[16 * s] = d;
    }
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

struct GdArgs {
  const char* A[2];         // activation digit images [M][K / 64][7][64]
  const char* img[2];       // digit images of the weights
  const double* wsc[2];     // [N] column scales
  long K[2];
  double post[2];           // 2^e_a
  int groups0;              // k-range groups of operand 0 (the rest belong to operand 1)
  long klen;                // k per group (a multiple of 64)
  int M, N;
  double* part;             // [groups][M][N]
};

// compile-time loop and LDS read / wait with literal operands (asm wants immediates)
template <int I> using gd_c = std::integral_constant<int, I>;
template <int I, int N, class F>
__device__ __forceinline__ void gd_for(F f) {
  if constexpr (I < N) {
    f(gd_c<I>());
    gd_for<I + 1, N>(f);
  }
}
template <int OFF>
__device__ __forceinline__ void gd_dsr(gd_v4i& d, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}
template <int N>
__device__ __forceinline__ void gd_wait(gd_v4i& a0, gd_v4i& a1, gd_v4i& b0, gd_v4i& b1) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a0), "+v"(a1), "+v"(b0), "+v"(b1) : "n"(N));
}

__global__ __launch_bounds__(512, 1) void gemm_digits_kernel(GdArgs a, int swz) {
  // two stages of activation digits (one slab ahead), three of weight digits (two slabs ahead), as gemm_sliced_kernel
  __shared__ __attribute__((aligned(1024))) char lds[5 * GD_OPER];           // 140 KB
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tn_count = a.N / GD_T;
  const int tiles = (a.M / GD_T) * tn_count;
  const long w = xcd_swizzle(blockIdx.x, gridDim.x, swz);
  const int grp = (int)(w / tiles), tile = (int)(w % tiles);
  const int tm = tile / tn_count, tn = tile % tn_count;
  const int op = grp < a.groups0 ? 0 : 1;
  const int gl = op ? grp - a.groups0 : grp;
  const long K = a.K[op];
  const long kbeg = (long)gl * a.klen;
  const long kend = kbeg + a.klen < K ? kbeg + a.klen : K;
  const int nslab = (int)((kend - kbeg) / 64);
  const int NT = a.N / 16;

  if (wave < 4) {
    // ================================================================ matrix wavefronts
    const int wm = wave >> 1, wn = wave & 1;
    unsigned long long t0c = 0, t0r = 0, twait = 0;
    if (L2Q_GD_EXP & 64) { t0c = __builtin_amdgcn_s_memtime(); t0r = __builtin_amdgcn_s_memrealtime(); }
    __builtin_amdgcn_s_setprio(3);
    gd_v4i acc[4][GD_NS];
    double racc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int g = 0; g < GD_NS; ++g) acc[t][g] = (gd_v4i){0, 0, 0, 0};
#pragma unroll
      for (int r = 0; r < 4; ++r) racc[t][r] = 0.0;
    }
    // (activation fragment: lane (r, g) reads slot 4 r + (g ^ 2 (r >> 3)), see the loaders)
    const int fr = lane & 15, fg = lane >> 4;
    const char* abase = lds + (2 * wm) * (GD_NS * GD_FRAG) + (4 * fr + (fg ^ ((fr >> 3) * 2))) * 16;
    const char* bbase = lds + 2 * GD_OPER + (2 * wn) * (GD_NS * GD_FRAG) + lane * 16;
    int p3 = 0;                                                // p % 3
    gd_v4i bf[2][GD_NS], af[2][2], afd[2][2];
    bool pending = false;                                      // rows 5, 6 of the previous slab not issued yet
    for (int p = 0; p < nslab; ++p) {
      unsigned long long tb = 0;
      if (L2Q_GD_EXP & 64) tb = __builtin_amdgcn_s_memtime();
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // B(p): the stages of slab p are complete
      if (L2Q_GD_EXP & 64) twait += __builtin_amdgcn_s_memtime() - tb;
      const int soa = (p & 1) * GD_OPER, sob = p3 * GD_OPER;
      p3 = p3 == 2 ? 0 : p3 + 1;
      // reads and MFMAs in the explicit order of gemm_sliced_kernel (LDS returns in order; a fragment is only
      // touched through its wait)
      const unsigned aaddr = (unsigned)(unsigned long)(gd_lds_ptr_t)(abase + soa);
      const unsigned baddr = (unsigned)(unsigned long)(gd_lds_ptr_t)(bbase + sob);
      auto rd_a = [&](auto sc, gd_v4i (&dst)[2]) {
        constexpr int S = decltype(sc)::value;
        gd_dsr<S * GD_FRAG>(dst[0], aaddr);
        gd_dsr<(GD_NS + S) * GD_FRAG>(dst[1], aaddr);
      };
      auto rd_b = [&](auto tc) {
        constexpr int T = decltype(tc)::value;
        gd_dsr<T * GD_FRAG>(bf[0][T], baddr);
        gd_dsr<(GD_NS + T) * GD_FRAG>(bf[1][T], baddr);
      };
      auto mm = [&](const gd_v4i (&a2)[2], int s, int t) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[2 * i + j][s + t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a2[i], bf[j][t], acc[2 * i + j][s + t], 0, 0, 0);
      };
      // the last two rows of a slab (12 MFMAs) are issued after the NEXT barrier, behind the first reads of the next
      // slab: they cover the barrier and the LDS latency
      auto tail = [&]() {
        mm(afd[0], 5, 0);
        mm(afd[0], 5, 1);
        mm(afd[1], 6, 0);
      };
      rd_a(gd_c<0>(), af[0]);
      rd_b(gd_c<6>());
      rd_b(gd_c<5>());
      rd_b(gd_c<4>());
      if (pending) {
        gd_wait<8>(afd[0][0], afd[0][1], afd[1][0], afd[1][1]);   // (complete since the barrier; orders the MFMAs)
        tail();
      }
      rd_b(gd_c<3>());
      gd_for<0, GD_NS>([&](auto uc) {                       // row 0: 7 groups of 4 MFMAs
        constexpr int T = GD_NS - 1 - decltype(uc)::value;
        // outstanding behind the fragments of group T: three more pairs (two for T = 1, one for T = 0)
        gd_wait<(T >= 2 ? 6 : T == 1 ? 4 : 2)>(af[0][0], af[0][1], bf[0][T], bf[1][T]);
        mm(af[0], 0, T);
        if constexpr (T >= 4) rd_b(gd_c<T - 4>());
        if constexpr (T == 3) rd_a(gd_c<1>(), af[1]);
      });
      gd_for<1, 5>([&](auto sc) {                           // rows 1..4: 24, 20, 16, 12 MFMAs
        constexpr int S = decltype(sc)::value;
        gd_wait<0>(af[S & 1][0], af[S & 1][1], bf[0][0], bf[1][0]);
        if constexpr (S < 4) rd_a(gd_c<S + 1>(), af[(S + 1) & 1]);
        if constexpr (S == 4) {
          rd_a(gd_c<5>(), afd[0]);
          rd_a(gd_c<6>(), afd[1]);
        }
#pragma unroll
        for (int t = 0; S + t < GD_NS; ++t) mm(af[S & 1], S, t);
      });
      pending = true;
      if (((p + 1) & (GD_RANGE / 64 - 1)) == 0 || p + 1 == nslab) {
        // end of an int32 range: the last rows now, then sum_g 256^(6-g) S_g in fp64, accumulate, clear
        gd_wait<0>(afd[0][0], afd[0][1], afd[1][0], afd[1][1]);
        tail();
        pending = false;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double x = (double)acc[t][0][r];
#pragma unroll
            for (int g = 1; g < GD_NS; ++g) x = fma(x, 256.0, (double)acc[t][g][r]);
            racc[t][r] += x;
          }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int g = 0; g < GD_NS; ++g) acc[t][g] = (gd_v4i){0, 0, 0, 0};
      }
    }
    if ((L2Q_GD_EXP & 64) && wave == 0 && lane == 0 && (blockIdx.x & 63) == 0) {
      const unsigned long long c = __builtin_amdgcn_s_memtime() - t0c, r = __builtin_amdgcn_s_memrealtime() - t0r;
      printf("block %d: %llu core clocks, %llu x 10 ns -> %.0f MHz, %.0f clocks per slab; matrix wavefront 0 at the barrier %.0f per slab\n",
             (int)blockIdx.x, c, r, (double)c / ((double)r * 0.01), (double)c / nslab, (double)twait / nslab);
    }
    // C/D layout of v_mfma_i32_16x16x64_i8: col = lane & 15, row = 4 (lane >> 4) + reg
    double* part = a.part + (long)grp * a.M * a.N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = tn * GD_T + (2 * wn + j) * 16 + (lane & 15);
        const double cs = a.wsc[op][n] * a.post[op];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = tm * GD_T + (2 * wm + i) * 16 + 4 * (lane >> 4) + r;
          part[(long)m * a.N + n] = racc[2 * i + j][r] * cs;
        }
      }
    return;
  }

  // ================================================================== loader wavefronts
  // Loader h moves row tile h of the activations (its seven planes) and the weight fragments h, h + 4, ..., h + 24.
  // Period p (between B(p - 1) and B(p)) issues A(p) into activation stage p & 1 and W(p + 1) into weight stage
  // (p + 1) % 3: both held slab p - 2, whose reads the matrix wavefronts retired (lgkmcnt(0)) in front of B(p - 1).
  // vmcnt counts in issue order: vmcnt(7) in front of B(p) leaves only the seven pieces of W(p + 1) in flight.
  const int h = wave - 4;
  const long aslabs = K / 64;
  const int lr = lane >> 2, lc = lane & 3;
  const char* asrc = a.A[op] + (((long)tm * GD_T + h * 16 + lr) * aslabs + kbeg / 64) * GD_SLAB + (lc ^ ((lr >> 3) * 2)) * 16;
  const char* bsrc = a.img[op] + ((kbeg / 64) * NT + tn * 4) * (long)(GD_NS * GD_FRAG) + lane * 16;
  const long bstep = (long)NT * (GD_NS * GD_FRAG);               // next k-slab of the weight image
  auto dma_a = [&](int q) {
#pragma unroll
    for (int s = 0; s < GD_NS; ++s)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(asrc + (long)q * GD_SLAB + s * 64),
                                       (gd_lds_ptr_t)(lds + (q & 1) * GD_OPER + (h * GD_NS + s) * GD_FRAG), 16, 0, 0);
  };
  auto dma_b = [&](int q) {
#pragma unroll
    for (int f = 0; f < GD_NS; ++f) {
      const int frag = h + 4 * f;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bsrc + (long)q * bstep + frag * GD_FRAG),
                                       (gd_lds_ptr_t)(lds + (2 + q % 3) * GD_OPER + frag * GD_FRAG), 16, 0, 0);
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
                     ldexp(1.0, GD_BITS - a_exp), ldexp(1.0, a_exp), (char*)image, flag);
  return check_launch("l2q_gemm_digits_slice");
}

int l2q_gemm_digits_f64(const void* A, const void* image, long K, int a_exp, const void* A2, const void* image2,
                        long K2, int a2_exp, int M, int N, const double* bias, const double* bias2,
                        const double* coeff, double scale, int act, double* C, void* ws, size_t ws_bytes,
                        void* stream) {
  L2Q_REQUIRE(A && image && C && ws, L2Q_EINVAL, "null pointer");
  L2Q_REQUIRE(K2 == 0 || (A2 && image2), L2Q_EINVAL, "second operand pair missing");
  L2Q_REQUIRE(M > 0 && N > 0 && K > 0 && K2 >= 0, L2Q_EINVAL, "non-positive size");
  L2Q_REQUIRE(M % GD_T == 0 && N % GD_T == 0 && K % 64 == 0 && K2 % 64 == 0, L2Q_ESHAPE,
              "the sliced layer serves M, N % 64 == 0 and K, K2 % 64 == 0");
  L2Q_REQUIRE(a_exp > -900 && a_exp < 900 && a2_exp > -900 && a2_exp < 900, L2Q_EINVAL, "bad operand exponent");
  L2Q_REQUIRE(act >= L2Q_ACT_NONE && act <= L2Q_ACT_SWISH, L2Q_EINVAL, "bad activation");
  L2Q_REQUIRE(ws_bytes >= l2q_gemm_sliced_ws_bytes(M, N, K, K2), L2Q_ESHAPE, "workspace too small");
  auto al = [](const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) == 0; };
  L2Q_REQUIRE(al(A, 15) && (!A2 || al(A2, 15)) && al(image, 255) && (!image2 || al(image2, 255)) && al(ws, 255),
              L2Q_ESHAPE, "activation images must be 16-byte aligned (weight images and workspace 256-byte)");
  hipStream_t st = (hipStream_t)stream;
  auto wimg_bytes = [&](long k) { return ((size_t)(k / 64) * (size_t)(N / 16) * GD_NS * GD_FRAG + 255) & ~(size_t)255; };
  GdArgs a;
  const long klen = gs_klen(M, N, K, K2);
  const int g0 = (int)cdiv(K, klen), g1 = K2 > 0 ? (int)cdiv(K2, klen) : 0;
  a.A[0] = (const char*)A; a.A[1] = (const char*)A2;
  a.img[0] = (const char*)image; a.img[1] = (const char*)image2;
  a.wsc[0] = (const double*)((const char*)image + wimg_bytes(K));
  a.wsc[1] = K2 > 0 ? (const double*)((const char*)image2 + wimg_bytes(K2)) : nullptr;
  a.K[0] = K; a.K[1] = K2;
  a.post[0] = ldexp(1.0, a_exp); a.post[1] = ldexp(1.0, a2_exp);
  a.groups0 = g0; a.klen = klen; a.M = M; a.N = N;
  const int groups = g0 + g1;
  a.part = (double*)ws;
  int* flag = gs_flag();
  L2Q_REQUIRE(flag, L2Q_EHIP, "device symbol gs_flag_dev not found");
  const int tiles = (M / GD_T) * (N / GD_T);
  hipLaunchKernelGGL(gemm_digits_kernel, dim3((unsigned)(groups * tiles)), dim3(512), 0, st, a, tuning().xcd_swizzle);
  gs_launch_reduce((const double*)ws, groups, (long)M * N, N, bias, bias2, coeff, scale, act, flag, C, st);
  return check_launch("l2q_gemm_digits_f64");
}

}  // extern "C"
