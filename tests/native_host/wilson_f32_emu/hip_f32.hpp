// TEST INFRASTRUCTURE: what csrc/su3_wilson_f32.hip needs of <hip/hip_runtime.h> beyond the stand-in header
// tests/native_host/emu/hip/hip_runtime.h: the float2 vector type.  Included by wilson_f32_emu.cpp ahead of the kernel
// file; the stand-in header itself is shared by the other drivers and stays as it is.
#pragma once
#include <hip/hip_runtime.h>
struct float2 { float x, y; };
static inline float2 make_float2(float x, float y) { return {x, y}; }
