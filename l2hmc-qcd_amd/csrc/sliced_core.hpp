// sliced_core.hpp -- what the two kernels of the int8-sliced fp64 input layer share: gemm_sliced_kernel
// (gemm_sliced.hip: fp64 activations, sliced by helper wavefronts) and gemm_digits_kernel (gemm_digits.hip:
// activation digit images, fetched by loader wavefronts).  Both are 512-thread workgroups whose first four
// wavefronts are "matrix" wavefronts on a 64 x 64 output tile; they differ in how the digits of a slab reach LDS.
// Here, once: the argument block, the workgroup's place in the problem, the matrix wavefronts' slab loop and
// their store of the partial sums, and the host launcher.  One loop, hence one set of int32 sums over the same
// k-ranges and one fp64 Horner combination: the two kernels give the same BITS (tests/test_gemm_digits_gpu.py).
#pragma once
#include "digits.hpp"

namespace l2q {

typedef int gs_v4i __attribute__((ext_vector_type(4)));
typedef unsigned gs_v4u __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* gs_lds_ptr_t;

constexpr int GS_FRAG = 1024;                  // one MFMA operand fragment: 64 lanes x 16 bytes
constexpr int GS_T = 64;                       // output tile (rows = columns)
constexpr int GS_OPER = 4 * GS_NS * GS_FRAG;   // one operand of a stage: 4 row tiles x 7 digits = 28 KB
constexpr int GS_RANGE = 16384;                // k per int32 accumulation
constexpr int GS_LDS = 5 * GS_OPER;            // two activation stages, then three weight stages: 140 KB

struct GsArgs {
  const void* A[2];         // activations: fp64 [M][K] (gemm_sliced_kernel) or digit images (gemm_digits_kernel)
  const char* img[2];       // digit images of the weights
  const double* wsc[2];     // [N] column scales
  long K[2];
  double sc[2], lim[2], post[2];   // 2^(54 - e_a), 2^e_a, 2^e_a
  int groups0;              // k-range groups of operand 0 (the rest belong to operand 1)
  long klen;                // k per group (a multiple of 64)
  int M, N;
  double* part;             // [groups][M][N]
  int* flag;
};

// The launcher of both entry points (gemm_sliced.hip): validates, picks the k-grouping, launches `kernel` on
// (groups x tiles) workgroups and then the reduce kernel.  `what` names the entry point in error texts, `align_msg`
// is its wording of the alignment refusal.
typedef void (*gs_kernel_t)(GsArgs, int);
int gs_launch(const char* what, gs_kernel_t kernel, const char* align_msg, const void* A, const void* image, long K,
              int a_exp, const void* A2, const void* image2, long K2, int a2_exp, int M, int N, const double* bias,
              const double* bias2, const double* coeff, double scale, int act, double* C, void* ws, size_t ws_bytes,
              void* stream);

#ifdef __HIPCC__
// a workgroup owns (tile, k-range group): slabs [kbeg / 64, kbeg / 64 + nslab) of operand op
struct GsTile {
  int grp, tm, tn, op, nslab, NT;
  long K, kbeg;
};
__device__ __forceinline__ GsTile gs_tile(const GsArgs& a, int swz) {
  GsTile t;
  const int tn_count = a.N / GS_T;
  const int tiles = (a.M / GS_T) * tn_count;
  const long w = xcd_swizzle(blockIdx.x, gridDim.x, swz);
  t.grp = (int)(w / tiles);
  const int tile = (int)(w % tiles);
  t.tm = tile / tn_count; t.tn = tile % tn_count;
  t.op = t.grp < a.groups0 ? 0 : 1;
  const int gl = t.op ? t.grp - a.groups0 : t.grp;
  t.K = a.K[t.op];
  t.kbeg = (long)gl * a.klen;
  const long kend = t.kbeg + a.klen < t.K ? t.kbeg + a.klen : t.K;
  t.nslab = (int)((kend - t.kbeg) / 64);
  t.NT = a.N / 16;
  return t;
}
// first byte of the workgroup's weight fragments in the image, and the step to the next k-slab
__device__ __forceinline__ const char* gs_wsrc(const GsArgs& a, const GsTile& t, int lane) {
  return a.img[t.op] + ((t.kbeg / 64) * t.NT + t.tn * 4) * (long)(GS_NS * GS_FRAG) + lane * 16;
}
__device__ __forceinline__ long gs_wstep(const GsTile& t) { return (long)t.NT * (GS_NS * GS_FRAG); }

// compile-time loop and LDS read / wait with literal operands (asm wants immediates)
template <int I> using gs_c = std::integral_constant<int, I>;
template <int I, int N, class F>
__device__ __forceinline__ void gs_for(F f) {
  if constexpr (I < N) {
    f(gs_c<I>());
    gs_for<I + 1, N>(f);
  }
}
template <int OFF>
__device__ __forceinline__ void gs_dsr(gs_v4i& d, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}
template <int N>
__device__ __forceinline__ void gs_wait(gs_v4i& a0, gs_v4i& a1, gs_v4i& b0, gs_v4i& b1) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a0), "+v"(a1), "+v"(b0), "+v"(b1) : "n"(N));
}

// The slab loop of a matrix wavefront: racc[2 i + j][r] = sum over the workgroup's slabs of the products of its
// 2 x 2 MFMA tiles, int32 per k-range of GS_RANGE, fp64 across ranges.  Per 64-k slab: 28 ds_read_b128 and 112
// v_mfma_i32_16x16x64_i8 (pairs of digits s + t <= 6, accumulated by g = s + t).  abase / bbase: this lane's piece of
// the wavefront's first activation / weight fragment in stage 0; slab p is read from activation stage p & 1 and
// weight stage p % 3.  barrier() is B(p): behind it the stages of slab p are complete.  hook(p, f) runs after MFMA
// group f = 0..6 of row 0 (gemm_sliced_kernel issues its LDS-DMA there).  EXP: the timing experiments' bits.
template <int EXP, class Barrier, class Hook>
__device__ __forceinline__ void gs_slab_loop(const char* abase, const char* bbase, int nslab, double (&racc)[4][4],
                                             Barrier barrier, Hook hook) {
  gs_v4i acc[4][GS_NS];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int g = 0; g < GS_NS; ++g) acc[t][g] = (gs_v4i){0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) racc[t][r] = 0.0;
  }
  int p3 = 0;                                                  // p % 3
  gs_v4i bf[2][GS_NS], af[2][2], afd[2][2];
  bool pending = false;                                        // rows 5, 6 of the previous slab not issued yet
  for (int p = 0; p < nslab; ++p) {
    barrier();                                                 // B(p): the stages of slab p are complete
    const int soa = (p & 1) * GS_OPER, sob = p3 * GS_OPER;
    p3 = p3 == 2 ? 0 : p3 + 1;
    // Reads and MFMAs in an explicit order, the reads as asm with explicit lgkmcnt waits (LDS returns in
    // order): left to the compiler, all 18 reads of the first row are hoisted and waited for with
    // lgkmcnt(0) -- ~600 clocks of LDS time with four wavefronts reading -- before the first MFMA.  Row 0
    // starts on four reads and pulls the other weight fragments in two groups ahead; the activation
    // fragments of row s + 1 are read while row s runs.  A fragment is only touched through its wait.
    const unsigned aaddr = (unsigned)(unsigned long)(gs_lds_ptr_t)(abase + soa);
    const unsigned baddr = (unsigned)(unsigned long)(gs_lds_ptr_t)(bbase + sob);
    auto rd_a = [&](auto sc, gs_v4i (&dst)[2]) {
      constexpr int S = decltype(sc)::value;
      gs_dsr<S * GS_FRAG>(dst[0], aaddr);
      gs_dsr<(GS_NS + S) * GS_FRAG>(dst[1], aaddr);
    };
    auto rd_b = [&](auto tc) {
      constexpr int T = decltype(tc)::value;
      gs_dsr<T * GS_FRAG>(bf[0][T], baddr);
      gs_dsr<(GS_NS + T) * GS_FRAG>(bf[1][T], baddr);
    };
    auto mm = [&](const gs_v4i (&a2)[2], int s, int t) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (!(EXP & 2) || (i == 0 && j == 0))
            acc[2 * i + j][s + t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a2[i], bf[j][t], acc[2 * i + j][s + t], 0, 0, 0);
    };
    // The last two rows of a slab (12 MFMAs, fragments kept in afd and in the weight fragments 0 and 1) are
    // issued after the NEXT barrier, behind the first reads of the next slab: they cover the barrier and the
    // LDS latency, during which the matrix pipe would idle.  Row 0 runs t = 6 ... 0 so that its first weight
    // fragments go into registers the old slab no longer needs.
    auto tail = [&]() {
      mm(afd[0], 5, 0);
      mm(afd[0], 5, 1);
      mm(afd[1], 6, 0);
    };
    rd_a(gs_c<0>(), af[0]);
    rd_b(gs_c<6>());
    rd_b(gs_c<5>());
    rd_b(gs_c<4>());
    if (pending) {
      gs_wait<8>(afd[0][0], afd[0][1], afd[1][0], afd[1][1]);   // (complete since the barrier; orders the MFMAs)
      tail();
    }
    rd_b(gs_c<3>());
    gs_for<0, GS_NS>([&](auto uc) {                       // row 0: 7 groups of 4 MFMAs
      constexpr int T = GS_NS - 1 - decltype(uc)::value;
      // outstanding behind the fragments of group T: three more pairs (two for T = 1, one for T = 0)
      gs_wait<(T >= 2 ? 6 : T == 1 ? 4 : 2)>(af[0][0], af[0][1], bf[0][T], bf[1][T]);
      mm(af[0], 0, T);
      hook(p, GS_NS - 1 - T);
      if constexpr (T >= 4) rd_b(gs_c<T - 4>());
      if constexpr (T == 3) rd_a(gs_c<1>(), af[1]);
    });
    gs_for<1, 5>([&](auto sc) {                           // rows 1..4: 24, 20, 16, 12 MFMAs
      constexpr int S = decltype(sc)::value;
      gs_wait<0>(af[S & 1][0], af[S & 1][1], bf[0][0], bf[1][0]);
      if constexpr (S < 4) rd_a(gs_c<S + 1>(), af[(S + 1) & 1]);
      if constexpr (S == 4) {
        rd_a(gs_c<5>(), afd[0]);
        rd_a(gs_c<6>(), afd[1]);
      }
#pragma unroll
      for (int t = 0; S + t < GS_NS; ++t) mm(af[S & 1], S, t);
    });
    pending = true;
    if (((p + 1) & (GS_RANGE / 64 - 1)) == 0 || p + 1 == nslab) {
      // end of an int32 range: the last rows now, then sum_g 256^(6-g) S_g in fp64, accumulate, clear
      gs_wait<0>(afd[0][0], afd[0][1], afd[1][0], afd[1][1]);
      tail();
      pending = false;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double x = (double)acc[t][0][r];
#pragma unroll
          for (int g = 1; g < GS_NS; ++g) x = fma(x, 256.0, (double)acc[t][g][r]);
          racc[t][r] += x;
        }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int g = 0; g < GS_NS; ++g) acc[t][g] = (gs_v4i){0, 0, 0, 0};
    }
  }
}

// the partial sums of matrix wavefront (wm, wn) into part[grp][M][N], scaled by column.
// C/D layout of v_mfma_i32_16x16x64_i8: col = lane & 15, row = 4 (lane >> 4) + reg
__device__ __forceinline__ void gs_store_part(const GsArgs& a, const GsTile& t, int wm, int wn, int lane,
                                              const double (&racc)[4][4]) {
  double* part = a.part + (long)t.grp * a.M * a.N;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = t.tn * GS_T + (2 * wn + j) * 16 + (lane & 15);
      const double cs = a.wsc[t.op][n] * a.post[t.op];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = t.tm * GS_T + (2 * wm + i) * 16 + 4 * (lane >> 4) + r;
        part[(long)m * a.N + n] = racc[2 * i + j][r] * cs;
      }
    }
}

// timing experiment 64 (-DL2Q_GS_EXP=64, -DL2Q_GD_EXP=64; ON = that bit, nothing is emitted without it): the shader
// clock over the slab loop and the waits at its barriers (s_memtime counts core clocks, s_memrealtime 100 MHz),
// printed by matrix wavefront 0 of every 64th workgroup
template <bool ON>
struct GsClock {
  unsigned long long c0 = 0, r0 = 0, wait = 0;
  __device__ __forceinline__ GsClock() {
    if (ON) { c0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
  }
  template <class Barrier>
  __device__ __forceinline__ void timed(Barrier barrier) {
    unsigned long long tb = 0;
    if (ON) tb = __builtin_amdgcn_s_memtime();
    barrier();
    if (ON) wait += __builtin_amdgcn_s_memtime() - tb;
  }
  __device__ __forceinline__ void print(int wave, int lane, int nslab) const {
    if (!ON || wave != 0 || lane != 0 || (blockIdx.x & 63) != 0) return;
    const unsigned long long c = __builtin_amdgcn_s_memtime() - c0, r = __builtin_amdgcn_s_memrealtime() - r0;
    printf("block %d: %llu core clocks, %llu x 10 ns -> %.0f MHz, %.0f clocks per slab; matrix wavefront 0 at the barrier %.0f per slab\n",
           (int)blockIdx.x, c, r, (double)c / ((double)r * 0.01), (double)c / nslab, (double)wait / nslab);
  }
};
#endif

}  // namespace l2q
