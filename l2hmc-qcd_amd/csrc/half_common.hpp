// half_common.hpp -- shared by the half-precision layer kernels (gemm_f16*.hip, gemm_lt.hip, heads_kstream_f16.hip,
// conv_patch_f16.hip): MFMA wrappers for fp16 / bf16 operands, autocast rounding points of the epilogue, launch interface.
#pragma once
#include <type_traits>
#include "l2q_common.hpp"

namespace l2q {

typedef float v4f32 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int HBK = 64;            // K-slab: two MFMA K-steps of 32
constexpr int HLD = HBK + 8;       // row stride 144 B: conflict-free ds_read_b128 fragments

template <typename HT> struct MfmaH;
typedef float v16f32 __attribute__((ext_vector_type(16)));
template <> struct MfmaH<_Float16> {
  using vec_t = f16x8;
  static __device__ __forceinline__ v4f32 run(vec_t a, vec_t b, v4f32 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  // 32x32x16: A lane l holds row l & 31, k = 8 (l >> 5) .. +7; D col = l & 31,
  // row = (r & 3) + 8 (r >> 2) + 4 (l >> 5).  Half the LDS fragment reads per flop of 16x16x32.
  static __device__ __forceinline__ v16f32 run32(vec_t a, vec_t b, v16f32 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};
template <> struct MfmaH<__bf16> {
  using vec_t = bf16x8;
  static __device__ __forceinline__ v4f32 run(vec_t a, vec_t b, v4f32 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ v16f32 run32(vec_t a, vec_t b, v16f32 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};

template <typename HT> __device__ __forceinline__ float rnd(float x) { return (float)(HT)x; }

__device__ __forceinline__ float act_h(float z, int act) {
  switch (act) {
    case L2Q_ACT_TANH: return tanhf(z);
    case L2Q_ACT_RELU: return z > 0.f ? z : 0.f;
    case L2Q_ACT_LEAKY_RELU: return z > 0.f ? z : 0.01f * z;
    case L2Q_ACT_ELU: return z > 0.f ? z : expm1f(z);
    case L2Q_ACT_SWISH: return z / (1.f + expf(-z));
    default: return z;
  }
}

struct EpiH {
  const float* bias;
  const float* bias2;
  const float* coeff;
  float scale;
  int act;
};

// y = scale * exp(coeff[n]) * r16(act(r16(acc + bias)))   (see the header of this file)
template <typename HT>
__device__ __forceinline__ float epilogue_h(float acc, float cb, float cs, bool has_coeff, int act) {
  float y = rnd<HT>(acc + cb);
  if (act != L2Q_ACT_NONE) y = rnd<HT>(act_h(y, act));
  y *= cs;
  return has_coeff ? y : rnd<HT>(y);
}

// geometry of PeriodicPadding(k-1) -> Conv2d(k) as an implicit GEMM (gemm_f16.hip)
struct ConvGeomH {
  long sn, sc, sh, sw;
  int C, H, W, k, Ho, Wo, Kc;
  int clast;            // K order: 0 (ci, i, j) -- nn.Conv2d's flatten order, 1 (i, j, ci)
  long M;               // GEMM rows: output pixels, or (pool == 2) 4 x pooled pixels
  int pool = 1;         // 2: MaxPool2d(2) fused -- row m is window position m & 3 of pooled pixel m >> 2
  int Hp = 0, Wp = 0;   // pooled extent (Ho / 2, Wo / 2)
};

// ---- host side: the half-type check and switch that the entry points share, and the prototype of every function that
// one half-precision .hip defines and another one calls.  A _launch returns true when it has enqueued its kernel, false
// when the call is not its case (shape, alignment, workspace, a missing library: the caller goes on to its next route);
// a _shape is the part of that test the sizes alone decide.

// the check of every entry point that takes a half type: L2Q_REQUIRE(half_type_ok(half_type), L2Q_EINVAL, kBadHalf)
inline bool half_type_ok(int half_type) { return half_type == L2Q_HALF_F16 || half_type == L2Q_HALF_BF16; }
constexpr char kBadHalf[] = "bad half type";

// half_type -> element type: runs the statements (launches and assignments, no `return`) with HT = _Float16 or __bf16;
// and back.  The statements are pasted once per type, each paste in a block scope of its own: a `static` that a nested
// launch macro declares (the PerDeviceOnce of L2Q_CP, L2Q_HD) is one per element type because of that.
#define L2Q_WITH_HALF(half_type, ...)                                      \
  do {                                                                     \
    if ((half_type) == L2Q_HALF_F16) { using HT = _Float16; __VA_ARGS__; } \
    else { using HT = __bf16; __VA_ARGS__; }                               \
  } while (0)
template <typename HT>
constexpr int kHalfType = std::is_same<HT, _Float16>::value ? L2Q_HALF_F16 : L2Q_HALF_BF16;

struct HeadsHArgs;      // heads_h_common.hpp

// gemm_f16_small.hip: hidden layers on many chains (K, N <= 256)
bool gemm_h_small_shape(int M, int N, long K);
bool gemm_h_small_launch(int half_type, const void* A, const void* W, int M, int N, long K, const EpiH& epi, void* C,
                         int c_is_f32, hipStream_t st);
// gemm_lt.hip: hipBLASLt for plain layers with M, N, K in the thousands; _available: the library loaded
bool gemm_h_lt_shape(int M, int N, long K);
bool gemm_h_lt_available();
size_t gemm_h_lt_ws_bytes(int M, int N, long K);
bool gemm_h_lt_launch(int half_type, const void* A, const void* W, int M, int N, long K, const EpiH& epi, void* C,
                      int c_is_f32, void* ws, size_t ws_bytes, hipStream_t st);
// gemm_f16_dma.hip: big 16-bit x 16-bit layers, 256 x 256 tiles on LDS-DMA staging
bool gemm_h_dma_shape(int M, int N, long K);
bool gemm_h_dma_launch(int half_type, const void* A, const void* W, int M, int N, long K, const EpiH& epi, void* C,
                       int c_is_f32, hipStream_t st);
// gemm_f16_skinny.hip: the streaming kernel of the wide-K fp32-operand input layer (N <= 256).  _maybe: what M, N and
// K + K2 decide of its shape test; _launch leaves *splits_out partial sums in ws for the caller's split-K reduction
bool gemm_h_skinny_maybe(int M, int N, long Kt);
int gemm_h_skinny_splits(int M, int N, long raw1, long K2);
size_t gemm_h_skinny_ws_bytes(int M, int N, long K, long K2);
bool gemm_h_skinny_launch(int half_type, const float* A, const void* W, int M, int N, long K, const float* A2,
                          const void* W2, long K2, void* ws, size_t ws_bytes, hipStream_t st, const float* cs_mask,
                          int cs_compl, int* splits_out);
// heads_kstream_f16.hip: K-split stream kernel of the heads + update (tuning heads_h_stream >= 2)
bool heads_h_kstream_launch(int half_type, HeadsHArgs a, int xupd, int forward, int use_ncp, int swz, float* logdet,
                            int accumulate, hipStream_t st, bool any_length);
// conv_patch_f16.hip: LDS-patch kernel when the conv layer fits it
bool conv_patch_launch(int half_type, const void* in, const ConvGeomH& g, const void* w, const float* bias, int cout,
                       int act, void* out, hipStream_t st);
// gemm_f16.hip: what l2q_kernel_name (su3_kernels.hip) answers for "l2q_gemm_h"
const char* gemm_h_kernel_name(int M, int N, long K);

}  // namespace l2q
