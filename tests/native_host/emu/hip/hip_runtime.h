// TEST INFRASTRUCTURE: stand-in for <hip/hip_runtime.h> that RUNS the kernels of a csrc/su3_*.hip on the host (the
// drivers of tests/native_host/*_emu/, built by tests/host_emu.py): a launch executes the workgroups one after the
// other, every thread of a workgroup as an OS thread with real barriers, `__shfl_down` through a per-wavefront
// exchange, `__shared__` as a static.  Only what those files and the headers they include use is provided.  (The
// math-only stand-in of the link-math tests is tests/native_host/hip/hip_runtime.h.)
#pragma once
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <thread>
#include <vector>
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__ static
struct double2 { double x, y; };
static inline double2 make_double2(double x, double y) { return {x, y}; }
using std::fma; using std::sqrt; using std::cos; using std::sin; using std::atan2; using std::fabs; using std::acos; using std::frexp; using std::ldexp; using std::fmax; using std::fmin;
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
typedef void* hipStream_t;
typedef int hipError_t;
constexpr int hipSuccess = 0;
inline hipError_t hipGetDevice(int* d) { *d = 0; return 0; }
inline hipError_t hipGetLastError() { return 0; }
inline const char* hipGetErrorString(hipError_t) { return "ok"; }
inline thread_local dim3 threadIdx, blockIdx;
inline dim3 gridDim, blockDim;
inline std::barrier<>* g_block_bar;
inline std::barrier<>* g_wave_bar[16];
inline double g_xchg[1024];
inline void __syncthreads() { g_block_bar->arrive_and_wait(); }
inline double __shfl_down(double v, int off, int) {
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  g_xchg[t] = v;
  g_wave_bar[w]->arrive_and_wait();
  const double r = lane + off < 64 ? g_xchg[t + off] : v;
  g_wave_bar[w]->arrive_and_wait();
  return r;
}
template <class F>
void emu_launch(dim3 grid, dim3 block, F f) {
  gridDim = grid; blockDim = block;
  if (block.x % 64) { fprintf(stderr, "block not whole waves\n"); exit(2); }
  for (unsigned b = 0; b < grid.x; ++b) {
    std::barrier<> bb(block.x);
    g_block_bar = &bb;
    std::vector<std::unique_ptr<std::barrier<>>> wb;
    for (unsigned w = 0; w < block.x / 64; ++w) { wb.emplace_back(new std::barrier<>(64)); g_wave_bar[w] = wb.back().get(); }
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; ++t) th.emplace_back([&, t] { threadIdx = dim3(t); blockIdx = dim3(b); f(); });
    for (auto& x : th) x.join();
  }
}
#define hipLaunchKernelGGL(k, grid, block, lds, st, ...) emu_launch(grid, block, [&] { k(__VA_ARGS__); })
