// Common helpers for the gfx950 (CDNA4) kernel library.
// Wavefront = 64; block sizes are multiples of 64 throughout.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdlib.h>

#include "launch_abi.h"

#define DEV_INLINE __device__ __forceinline__

// ---------------------------------------------------------------- vectors
typedef __attribute__((ext_vector_type(2))) float    f32x2;
typedef __attribute__((ext_vector_type(4))) float    f32x4;
typedef __attribute__((ext_vector_type(16))) float   f32x16;
typedef __attribute__((ext_vector_type(4))) short    s16x4;
typedef __attribute__((ext_vector_type(8))) short    s16x8;
typedef __attribute__((ext_vector_type(4))) int      i32x4;
typedef __attribute__((ext_vector_type(8))) __bf16   bf16x8;

using bf16 = __hip_bfloat16;

DEV_INLINE float bf2f(unsigned short u) {
  union { unsigned int i; float f; } v;
  v.i = (unsigned int)u << 16;
  return v.f;
}

DEV_INLINE unsigned short f2bf(float f) {
  union { float f; unsigned int i; } v;
  v.f = f;
  // round-to-nearest-even
  unsigned int lsb = (v.i >> 16) & 1;
  v.i += 0x7fffu + lsb;
  return (unsigned short)(v.i >> 16);
}

// -------------------------------------------------------------- activations
// act codes: 0 identity, 1 tanh, 2 sigmoid, 3 leaky-relu, 4 relu
DEV_INLINE float act_fwd(float x, int act, float slope) {
  switch (act) {
    case 1: return tanhf(x);
    case 2: return 1.0f / (1.0f + __expf(-x));
    case 3: return x > 0.0f ? x : slope * x;
    case 4: return x > 0.0f ? x : 0.0f;
    default: return x;
  }
}

// derivative expressed in terms of the OUTPUT y (valid for all five)
DEV_INLINE float act_bwd_from_y(float y, int act, float slope) {
  switch (act) {
    case 1: return 1.0f - y * y;
    case 2: return y * (1.0f - y);
    case 3: return y > 0.0f ? 1.0f : slope;
    case 4: return y > 0.0f ? 1.0f : 0.0f;
    default: return 1.0f;
  }
}

// ------------------------------------------------------------- reductions
DEV_INLINE float wave_reduce_sum(float v) {
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v += __shfl_down(v, off, 64);
  return v;  // valid in lane 0
}

DEV_INLINE float wave_reduce_max(float v) {
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_down(v, off, 64));
  return v;
}

constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }

// ------------------------------------------------- fast integer division
// device side of FastDiv (launch_abi.h)
DEV_INLINE unsigned fdiv(unsigned n, FastDiv f) {
  return (unsigned)(((unsigned long long)n * f.mul) >> f.shift);
}

DEV_INLINE unsigned fmod_(unsigned n, FastDiv f, unsigned q) {
  return n - q * (unsigned)f.d;
}

// ------------------------------------------------------- LDS-DMA staging
// one 16B global -> LDS copy per lane; the LDS destination is wave-uniform
// (lane-linear behind it), so swizzles go through the SOURCE address
#define GLDS16(gsrc, ldst)                                                    \
  __builtin_amdgcn_global_load_lds(                                          \
      (const __attribute__((address_space(1))) unsigned int*)(gsrc),          \
      (__attribute__((address_space(3))) unsigned int*)(ldst), 16, 0, 0)

// --------------------------------------------------------- XCD block remap
// Bijective XCD-aware remap of a linear block id over nwg blocks: hardware
// deals consecutive ids round-robin to the 8 XCDs; this hands each XCD a
// contiguous run of tiles instead (L2 locality), exact for any nwg.
// Callers read gridDim into a local before the call: evaluating it as an
// argument changes register allocation in gemm_tn_kshort<128, true>.
DEV_INLINE int xcd_remap(int bid, int nwg) {
  if (nwg >= 8) {
    int q = nwg / 8, r = nwg % 8;
    int xcd = bid % 8, idx = bid / 8;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  return bid;
}

// ------------------------------------------------- launcher env gates (host)
// Use as a function-local `static const int v = env_flag(...)`: the gate is
// read once, at the first launch that consults it.
// on/off gate: only a leading '0' turns a default-on gate off, only a
// leading '1' turns a default-off gate on
static inline int env_flag(const char* name, int dflt) {
  const char* e = getenv(name);
  return (e != nullptr && e[0] == (dflt ? '0' : '1')) ? !dflt : dflt;
}

// integer gate (atoi parse)
static inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e != nullptr ? atoi(e) : dflt;
}

#define HIP_CHECK_LAST()                                                     \
  do {                                                                       \
    hipError_t e = hipGetLastError();                                        \
    if (e != hipSuccess) {                                                   \
      printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__,      \
             __LINE__);                                                      \
    }                                                                        \
  } while (0)
