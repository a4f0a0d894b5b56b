// FP8 (OCP e4m3fn — gfx950 native, NOT the MI300X fnuz variant) conv path.
//
// Mixed-precision scheme: bf16 master activations/weights are quantized
// per-tensor (dynamic amax scaling) to e4m3, the conv forward runs on
// mfma_f32_16x16x32_fp8_fp8 with fp32 accumulation, and the epilogue
// de-scales + bias + activation back to bf16. Backward stays bf16.
//
// Same implicit-GEMM structure as the bf16 TN kernel: 128x128x64 tiles,
// double-buffered LDS staged by 16B global_load_lds with the im2col gather
// fused into the source address (zero-page redirect for OOB/pad).

#include "conv_gather.h"

typedef __attribute__((ext_vector_type(8))) float f32x8;

// ----------------------------------------------------------- quantization
// amax via atomicMax on the positive-float bit pattern
__global__ void amax_bf16(const s16x8* __restrict__ x, long n8,
                          unsigned* __restrict__ amax_bits) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  float m = 0.f;
  for (; i < n8; i += (long)gridDim.x * blockDim.x) {
    s16x8 v = x[i];
    #pragma unroll
    for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(bf2f((unsigned short)v[j])));
  }
  m = wave_reduce_max(m);
  if ((threadIdx.x & 63) == 0) {
    union { float f; unsigned u; } c;
    c.f = m;
    atomicMax(amax_bits, c.u);  // positive floats order like their bits
  }
}

// scale = 448/amax (e4m3 max normal 448); inv = 1/scale
__global__ void fp8_make_scale(const unsigned* __restrict__ amax_bits,
                               float* __restrict__ scale,
                               float* __restrict__ inv) {
  union { float f; unsigned u; } c;
  c.u = *amax_bits;
  float a = c.f;
  float s = (a > 1e-20f) ? 448.f / a : 1.f;
  *scale = s;
  *inv = 1.f / s;
}

// bf16 -> e4m3 with scale (device scalar), vectorized by 8
__global__ void quant_fp8(const s16x8* __restrict__ x,
                          unsigned long long* __restrict__ y, long n8,
                          const float* __restrict__ scale) {
  float s = *scale;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n8; i += (long)gridDim.x * blockDim.x) {
    s16x8 v = x[i];
    unsigned lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f((unsigned short)v[0]) * s,
                                         bf2f((unsigned short)v[1]) * s, lo,
                                         false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f((unsigned short)v[2]) * s,
                                         bf2f((unsigned short)v[3]) * s, lo,
                                         true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f((unsigned short)v[4]) * s,
                                         bf2f((unsigned short)v[5]) * s, hi,
                                         false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f((unsigned short)v[6]) * s,
                                         bf2f((unsigned short)v[7]) * s, hi,
                                         true);
    y[i] = ((unsigned long long)hi << 32) | lo;
  }
}

// bf16 -> e4m3 with the previous step's scale (delayed scaling), fused
// with this tensor's amax reduction so the standalone full-read amax
// pass disappears.  v_cvt_pk_fp8_f32 does NOT saturate — a scaled value
// past +-448 encodes as e4m3fn NaN (0x7f) and poisons the GEMM (measured:
// the second D forward of a GAN step overflowed its first-step scale) —
// so the scaled input is clamped to +-448 explicitly; the updated scale
// applies from the next step (TransformerEngine-style recipe).
__global__ void quant_fp8_delayed(const s16x8* __restrict__ x,
                                  unsigned long long* __restrict__ y, long n8,
                                  const float* __restrict__ scale,
                                  unsigned* __restrict__ amax_bits) {
  float s = *scale;
  float m = 0.f;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n8; i += (long)gridDim.x * blockDim.x) {
    s16x8 v = x[i];
    float f[8];
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      float raw = bf2f((unsigned short)v[j]);
      m = fmaxf(m, fabsf(raw));
      f[j] = fminf(fmaxf(raw * s, -448.f), 448.f);  // saturate, never NaN
    }
    unsigned lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    y[i] = ((unsigned long long)hi << 32) | lo;
  }
  m = wave_reduce_max(m);
  if ((threadIdx.x & 63) == 0) {
    union { float f; unsigned u; } c;
    c.f = m;
    atomicMax(amax_bits, c.u);
  }
}

// scale/inv for the NEXT step from the accumulated amax; resets amax
__global__ void fp8_roll_scale(unsigned* __restrict__ amax_bits,
                               float* __restrict__ scale,
                               float* __restrict__ inv) {
  union { float f; unsigned u; } c;
  c.u = *amax_bits;
  float a = c.f;
  float sc = (a > 1e-20f) ? 448.f / a : 1.f;
  *scale = sc;
  *inv = 1.f / sc;
  *amax_bits = 0;
}

// ------------------------------------------------------------ fp8 TN GEMM
// A gathered from an fp8 NHWC image (implicit conv) or plain [M][K];
// B plain fp8 [N][K]. LDS tiles [128 rows][128 k] fp8 = 16 KiB each.
// K depth is 128 to feed gfx950's DOUBLE-RATE fp8 MFMA
// (mfma_scale_f32_16x16x128_f8f6f4 with unit e8m0 scales — there is no
// non-scaled large-K fp8 form; the CDNA3-era 16x16x32_fp8 runs at the
// bf16 FLOP rate, i.e. half the 5 PF fp8 peak).
constexpr int F8_BM = 128, F8_BN = 128, F8_BK = 128;
constexpr int F8_TILE_B = F8_BM * F8_BK;  // bytes (1B/elem)
// Staged by conv_gather.h's tn_stage_rows / TnGatherStager at 1-byte
// elements: a 16B chunk is 16 fp8 channels.

typedef __attribute__((ext_vector_type(8))) int i32x8;

// fragment = 32 consecutive fp8 (lane's K window kq*32) as two XOR-swizzled
// 16B LDS reads; rows are 128B (8 slots of 16B)
DEV_INLINE i32x8 f8_frag32(const char* lds, int row, int kq) {
  int s0 = (2 * kq) ^ (row & 7);
  int s1 = (2 * kq + 1) ^ (row & 7);
  i32x4 lo = *(const i32x4*)(lds + row * 128 + s0 * 16);
  i32x4 hi = *(const i32x4*)(lds + row * 128 + s1 * 16);
  i32x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}

template <bool GATHER_A>
__global__ __launch_bounds__(256, 2) void gemm_tn_fp8_core(
    const unsigned char* __restrict__ A, const unsigned char* __restrict__ B,
    unsigned short* __restrict__ C, const float* __restrict__ bias,
    const float* __restrict__ inv_qa, const float* __restrict__ inv_qb,
    int M, int N, int K, long lda, long ldb, int act, float slope,
    ConvGather ga, const unsigned char* __restrict__ zp) {
  __shared__ __attribute__((aligned(128))) char lds[4 * F8_TILE_B];
  auto abuf = [&](int i) -> char* { return lds + (i ? 2 * F8_TILE_B : 0); };
  auto bbuf = [&](int i) -> char* {
    return lds + F8_TILE_B + (i ? 2 * F8_TILE_B : 0);
  };

  const int nwgx = gridDim.x;
  const int bidx = xcd_remap(blockIdx.x, nwgx);
  const int m0 = bidx * F8_BM;
  const int n0 = blockIdx.y * F8_BN;
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wr = wid >> 1, wc = wid & 1;
  const int fr = lane & 15, fq = lane >> 4;

  f32x4 acc[4][4];
  #pragma unroll
  for (int i = 0; i < 4; ++i)
    #pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int ntiles = K / F8_BK;
  TnGatherStager<256, unsigned char> gs;
  if (GATHER_A) {
    gs.init(ga, m0, M);
    gs.stage(A, ga, zp, 0, abuf(0));
  } else {
    tn_stage_rows<256, 4>(A, m0, M, lda, 0, abuf(0));
  }
  tn_stage_rows<256, 4>(B, n0, N, ldb, 0, bbuf(0));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    int cur = t & 1;
    if (t + 1 < ntiles) {
      if (GATHER_A)
        gs.stage(A, ga, zp, (t + 1) * F8_BK, abuf(cur ^ 1));
      else
        tn_stage_rows<256, 4>(A, m0, M, lda, (t + 1) * F8_BK, abuf(cur ^ 1));
      tn_stage_rows<256, 4>(B, n0, N, ldb, (t + 1) * F8_BK, bbuf(cur ^ 1));
    }
    const char* Al = abuf(cur);
    const char* Bl = bbuf(cur);
    {
      i32x8 a[4], b[4];
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        a[mi] = f8_frag32(Al, wr * 64 + mi * 16 + fr, fq);
      #pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        b[ni] = f8_frag32(Bl, wc * 64 + ni * 16 + fr, fq);
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          // cbsz=0/blgp=0: both operands e4m3 fp8; e8m0 scale byte 127
          // = x1.0 (per-tensor scaling stays in the epilogue de-scale)
          acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              a[mi], b[ni], acc[mi][ni], 0, 0, 0, 127, 0, 127);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // de-scale + bias + act, LDS-staged coalesced stores (N % 8 == 0 assumed
  // for the fast path; scalar fallback otherwise)
  float descale = (*inv_qa) * (*inv_qb);
  if ((N & 7) == 0) {
    unsigned short* ctile = (unsigned short*)lds;
    __syncthreads();
    #pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      #pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        int lc = wc * 64 + ni * 16 + fr;
        float bv = bias != nullptr ? bias[min(n0 + lc, N - 1)] : 0.f;
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          int lr = wr * 64 + mi * 16 + fq * 4 + r;
          ctile[lr * 128 + lc] =
              f2bf(act_fwd(acc[mi][ni][r] * descale + bv, act, slope));
        }
      }
    }
    __syncthreads();
    const int t = threadIdx.x;
    #pragma unroll
    for (int i = 0; i < 8; ++i) {
      int piece = i * 256 + t;
      int row = piece >> 4;
      int seg = piece & 15;
      int grow = m0 + row;
      int gcol = n0 + seg * 8;
      if (grow < M && gcol + 8 <= N) {
        long crow = grow;
        if (GATHER_A && ga.mode == 2) crow = scatter_row(ga, grow);
        *(s16x8*)(&C[crow * N + gcol]) =
            *(const s16x8*)(ctile + row * 128 + seg * 8);
      }
    }
    return;
  }
  #pragma unroll
  for (int mi = 0; mi < 4; ++mi)
    #pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      int col = n0 + wc * 64 + ni * 16 + fr;
      if (col >= N) continue;
      float bv = bias != nullptr ? bias[col] : 0.f;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m0 + wr * 64 + mi * 16 + fq * 4 + r;
        if (row >= M) continue;
        C[(long)row * N + col] =
            f2bf(act_fwd(acc[mi][ni][r] * descale + bv, act, slope));
      }
    }
}

extern "C" {

void launch_amax(const void* x, long n, unsigned* amax_bits, hipStream_t s) {
  long n8 = n / 8;
  int grid = (int)min((long)1024, n8 / 256 + 1);
  hipLaunchKernelGGL(amax_bf16, dim3(grid), dim3(256), 0, s, (const s16x8*)x,
                     n8, amax_bits);
}

void launch_fp8_make_scale(const unsigned* amax_bits, float* scale,
                           float* inv, hipStream_t s) {
  hipLaunchKernelGGL(fp8_make_scale, dim3(1), dim3(1), 0, s, amax_bits,
                     scale, inv);
}

void launch_quant_fp8(const void* x, void* y, long n, const float* scale,
                      hipStream_t s) {
  long n8 = n / 8;
  int grid = (int)min((long)2048, n8 / 256 + 1);
  hipLaunchKernelGGL(quant_fp8, dim3(grid), dim3(256), 0, s, (const s16x8*)x,
                     (unsigned long long*)y, n8, scale);
}

void launch_quant_fp8_delayed(const void* x, void* y, long n,
                              const float* scale, unsigned* amax_bits,
                              hipStream_t s) {
  long n8 = n / 8;
  int grid = (int)min((long)2048, n8 / 256 + 1);
  hipLaunchKernelGGL(quant_fp8_delayed, dim3(grid), dim3(256), 0, s,
                     (const s16x8*)x, (unsigned long long*)y, n8, scale,
                     amax_bits);
}

void launch_fp8_roll_scale(unsigned* amax_bits, float* scale, float* inv,
                           hipStream_t s) {
  hipLaunchKernelGGL(fp8_roll_scale, dim3(1), dim3(1), 0, s, amax_bits,
                     scale, inv);
}

void launch_gemm_tn_fp8(const void* A, const void* B, void* C,
                        const float* bias, const float* inv_qa,
                        const float* inv_qb, int M, int N, int K, long lda,
                        long ldb, int act, float slope, int gather,
                        ConvGather ga, const void* zp, hipStream_t s) {
  // 8-phase fp8 pipeline (gemm8p_fp8.hip) — default for large shapes
  if (gemm_tn_8p_fp8_eligible(M, N, K)) {
    launch_gemm_tn_8p_fp8(A, B, C, bias, inv_qa, inv_qb, M, N, K, lda, ldb,
                          act, slope, gather, ga, zp, s);
    return;
  }
  dim3 grid(ceil_div(M, F8_BM), ceil_div(N, F8_BN));
  if (gather)
    hipLaunchKernelGGL((gemm_tn_fp8_core<true>), grid, dim3(256), 0, s,
                       (const unsigned char*)A, (const unsigned char*)B,
                       (unsigned short*)C, bias, inv_qa, inv_qb, M, N, K, lda,
                       ldb, act, slope, ga, (const unsigned char*)zp);
  else
    hipLaunchKernelGGL((gemm_tn_fp8_core<false>), grid, dim3(256), 0, s,
                       (const unsigned char*)A, (const unsigned char*)B,
                       (unsigned short*)C, bias, inv_qa, inv_qb, M, N, K, lda,
                       ldb, act, slope, ga, (const unsigned char*)zp);
}

}  // extern "C"
