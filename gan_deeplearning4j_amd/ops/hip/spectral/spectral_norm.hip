// Spectral normalization of a bf16 weight matrix W [M, K] (row-major):
// one power iteration on persistent fp32 vectors u [M], v [K], then
// W_sn = W / sigma.  Semantics of torch.nn.utils.spectral_norm with
// n_power_iterations = 1, eps = 1e-12, dim = 0:
//
//   t = W^T u;  v = t / max(|t|, eps)
//   s = W v;    u' = s / max(|s|, eps)
//   sigma = u' . s;  W_sn = W * (1 / max(sigma, eps))
//
// (the max on the last division is the one deviation: a zero matrix gives
// zeros, not NaN).  Memory-bound family: every pass over W moves 16 B per
// lane when K % 8 == 0; otherwise (row byte stride not a multiple of 16)
// the same kernels fall back to per-element accesses of the same 8-column
// groups, so there is one code path and one reduction tree per shape.
//
// Capture safety: u, v, sigma and 1 / sigma are read from and written to
// device memory only; no scalar crosses to the host, no atomics.  Every
// reduction is fixed-order (per-thread serial, 6 shuffle steps, the block's
// waves in order, then per-block partials summed by sum_partials() in the
// consumer's prologue), so results are bit-reproducible run to run.
//
// Training forward, five launches on one stream:
//   sn_col_partial   tpart[c][k] = sum over row chunk c of W[m][k] u[m]
//   sn_col_finish    t[k] = sum_c tpart[c][k];  per-block partials of |t|^2
//   sn_row_pass      s[m] = sum_k W[m][k] (t[k] / max(|t|, eps))
//   sn_finalize      ONE block: writes v, u', sigma, 1/sigma and the copies
//   sn_scale         W_sn = bf16(W * (1 / sigma))
// Eval forward: sn_row_pass on the stored v, sn_sigma_eval, sn_scale;
// nothing but s, sig and W_sn is written.
// Backward: sn_dot_partial (<G, W_sn> partials), sn_bwd_apply.

#include "../common.h"
#include "spectral_abi.h"

#define SN_BLOCK 256
#define SN_WAVES (SN_BLOCK / 64)
#define SN_GRID_CAP 1024
#define SN_CHUNK_ROWS 16
#define SN_MAX_CHUNKS 64
#define SN_EPS 1e-12f

// 8 consecutive columns k0..k0+7 of one row; columns >= K read as 0
DEV_INLINE void load8(const unsigned short* __restrict__ row, long k0, long K,
                      int vec, float f[8]) {
  if (vec) {
    s16x8 p = *(const s16x8*)(row + k0);
    #pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = bf2f((unsigned short)p[j]);
  } else {
    #pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (k0 + j < K) ? bf2f(row[k0 + j]) : 0.f;
  }
}

DEV_INLINE void store8(unsigned short* __restrict__ row, long k0, long K,
                       int vec, const float f[8]) {
  if (vec) {
    s16x8 p;
    #pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = (short)f2bf(f[j]);
    *(s16x8*)(row + k0) = p;
  } else {
    #pragma unroll
    for (int j = 0; j < 8; ++j)
      if (k0 + j < K) row[k0 + j] = f2bf(f[j]);
  }
}

DEV_INLINE float sum8(const float a[8]) {
  return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

// sum over the block, the same value in every thread (waves added in order)
DEV_INLINE float block_sum(float v, float* lds) {
  v = wave_reduce_sum(v);
  __syncthreads();  // lds is reused between calls
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
  #pragma unroll
  for (int w = 0; w < SN_WAVES; ++w) r += lds[w];
  return r;
}

// fixed-order sum of n per-block partials; every wave computes the same
// bits (lane-strided serial sums, then the shuffle tree)
DEV_INLINE float sum_partials(const float* __restrict__ p, int n) {
  float a = 0.f;
  for (int i = threadIdx.x & 63; i < n; i += 64) a += p[i];
  a = wave_reduce_sum(a);
  return __shfl(a, 0, 64);
}

// ------------------------------------------------------------ column pass
// grid (col blocks, row chunks); a thread owns one 8-column group
__global__ void sn_col_partial(const unsigned short* __restrict__ W,
                               const float* __restrict__ u,
                               float* __restrict__ tpart, long M, long K,
                               long K8, long rpc, int vec) {
  long g = (long)blockIdx.x * SN_BLOCK + threadIdx.x;
  if (g >= K8) return;
  long m0 = (long)blockIdx.y * rpc;
  long m1 = m0 + rpc < M ? m0 + rpc : M;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (long m = m0; m < m1; ++m) {
    float um = u[m];
    float f[8];
    load8(W + m * K, g * 8, K, vec, f);
    #pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = fmaf(f[j], um, acc[j]);
  }
  float* out = tpart + (long)blockIdx.y * K;
  #pragma unroll
  for (int j = 0; j < 8; ++j)
    if (g * 8 + j < K) out[g * 8 + j] = acc[j];
}

// t[k] = chunks summed in order; nsq_part[block] = sum of t[k]^2
__global__ void sn_col_finish(const float* __restrict__ tpart,
                              float* __restrict__ t,
                              float* __restrict__ nsq_part, long K,
                              int nchunks) {
  __shared__ float lds[SN_WAVES];
  long k = (long)blockIdx.x * SN_BLOCK + threadIdx.x;
  float val = 0.f;
  if (k < K) {
    for (int c = 0; c < nchunks; ++c) val += tpart[(long)c * K + k];
    t[k] = val;
  }
  float tot = block_sum(val * val, lds);
  if (threadIdx.x == 0) nsq_part[blockIdx.x] = tot;
}

// --------------------------------------------------------------- row pass
// one wave per row.  NORMALISE: vin is the unnormalised t and every block
// derives |t| from the column pass's partials; else vin is the stored v.
template <bool NORMALISE>
__global__ void sn_row_pass(const unsigned short* __restrict__ W,
                            const float* __restrict__ vin,
                            const float* __restrict__ nsq_part, int nparts,
                            float* __restrict__ s, long M, long K, long K8,
                            int vec) {
  int lane = threadIdx.x & 63;
  float nrm = 1.f;
  if (NORMALISE) nrm = fmaxf(sqrtf(sum_partials(nsq_part, nparts)), SN_EPS);
  for (long m = (long)blockIdx.x * SN_WAVES + (threadIdx.x >> 6); m < M;
       m += (long)gridDim.x * SN_WAVES) {
    const unsigned short* row = W + m * K;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (long g = lane; g < K8; g += 64) {
      float f[8];
      load8(row, g * 8, K, vec, f);
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        long k = g * 8 + j;
        float vv = (k < K) ? vin[k] : 0.f;
        if (NORMALISE) vv = vv / nrm;
        acc[j] = fmaf(f[j], vv, acc[j]);
      }
    }
    float r = wave_reduce_sum(sum8(acc));
    if (lane == 0) s[m] = r;
  }
}

// --------------------------------------------------------------- finalize
// exactly one block writes the persistent state
__global__ void sn_finalize(const float* __restrict__ t,
                            const float* __restrict__ nsq_part, int nparts,
                            const float* __restrict__ s, float* __restrict__ u,
                            float* __restrict__ v, float* __restrict__ u_out,
                            float* __restrict__ v_out,
                            float* __restrict__ sig, long M, long K) {
  __shared__ float lds[SN_WAVES];
  float nrm = fmaxf(sqrtf(sum_partials(nsq_part, nparts)), SN_EPS);
  for (long k = threadIdx.x; k < K; k += SN_BLOCK) {
    float vv = t[k] / nrm;
    v[k] = vv;
    v_out[k] = vv;
  }
  float a = 0.f;
  for (long m = threadIdx.x; m < M; m += SN_BLOCK) a = fmaf(s[m], s[m], a);
  float sn = fmaxf(sqrtf(block_sum(a, lds)), SN_EPS);
  float b = 0.f;
  for (long m = threadIdx.x; m < M; m += SN_BLOCK) {
    float sm = s[m];
    float un = sm / sn;
    u[m] = un;
    u_out[m] = un;
    b = fmaf(un, sm, b);
  }
  float sigma = block_sum(b, lds);
  if (threadIdx.x == 0) {
    sig[0] = sigma;
    sig[1] = 1.0f / fmaxf(sigma, SN_EPS);
  }
}

__global__ void sn_sigma_eval(const float* __restrict__ s,
                              const float* __restrict__ u,
                              float* __restrict__ sig, long M) {
  __shared__ float lds[SN_WAVES];
  float b = 0.f;
  for (long m = threadIdx.x; m < M; m += SN_BLOCK) b = fmaf(u[m], s[m], b);
  float sigma = block_sum(b, lds);
  if (threadIdx.x == 0) {
    sig[0] = sigma;
    sig[1] = 1.0f / fmaxf(sigma, SN_EPS);
  }
}

// ------------------------------------------------- elementwise 2-D passes
// grid (column-group blocks, rows), both grid-strided
__global__ void sn_scale(const unsigned short* __restrict__ W,
                         const float* __restrict__ sig,
                         unsigned short* __restrict__ Wsn, long M, long K,
                         long K8, int vec) {
  float inv = sig[1];
  for (long m = blockIdx.y; m < M; m += gridDim.y)
    for (long g = (long)blockIdx.x * SN_BLOCK + threadIdx.x; g < K8;
         g += (long)gridDim.x * SN_BLOCK) {
      float f[8];
      load8(W + m * K, g * 8, K, vec, f);
      #pragma unroll
      for (int j = 0; j < 8; ++j) f[j] *= inv;
      store8(Wsn + m * K, g * 8, K, vec, f);
    }
}

// dot_part[block] = this block's share of <G, W_sn>
__global__ void sn_dot_partial(const unsigned short* __restrict__ G,
                               const unsigned short* __restrict__ Wsn,
                               float* __restrict__ dot_part, long M, long K,
                               long K8, int vec) {
  __shared__ float lds[SN_WAVES];
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (long m = blockIdx.y; m < M; m += gridDim.y)
    for (long g = (long)blockIdx.x * SN_BLOCK + threadIdx.x; g < K8;
         g += (long)gridDim.x * SN_BLOCK) {
      float a[8], b[8];
      load8(G + m * K, g * 8, K, vec, a);
      load8(Wsn + m * K, g * 8, K, vec, b);
      #pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(a[j], b[j], acc[j]);
    }
  float tot = block_sum(sum8(acc), lds);
  if (threadIdx.x == 0)
    dot_part[(long)blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

// dW = (G - dot * u[m] * v[k]) * (1 / sigma)
__global__ void sn_bwd_apply(const unsigned short* __restrict__ G,
                             const float* __restrict__ dot_part, int nparts,
                             const float* __restrict__ u,
                             const float* __restrict__ v,
                             const float* __restrict__ sig,
                             unsigned short* __restrict__ dW, long M, long K,
                             long K8, int vec) {
  float dot = sum_partials(dot_part, nparts);
  float inv = sig[1];
  for (long m = blockIdx.y; m < M; m += gridDim.y) {
    float c = dot * u[m];
    for (long g = (long)blockIdx.x * SN_BLOCK + threadIdx.x; g < K8;
         g += (long)gridDim.x * SN_BLOCK) {
      float f[8];
      load8(G + m * K, g * 8, K, vec, f);
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        long k = g * 8 + j;
        float vk = (k < K) ? v[k] : 0.f;
        f[j] = (f[j] - c * vk) * inv;
      }
      store8(dW + m * K, g * 8, K, vec, f);
    }
  }
}

// ------------------------------------------------------------- launchers
static long cdiv(long a, long b) { return (a + b - 1) / b; }

static int use_vec(long K, const void* a, const void* b = nullptr,
                   const void* c = nullptr) {
  unsigned long long bits = (unsigned long long)a | (unsigned long long)b |
                            (unsigned long long)c;
  return (K % 8 == 0 && (bits & 15ull) == 0) ? 1 : 0;
}

static dim3 grid2d(long M, long K8) {
  long gx = cdiv(K8, SN_BLOCK);
  if (gx > SN_GRID_CAP) gx = SN_GRID_CAP;
  long gy = SN_GRID_CAP / gx;
  if (gy > M) gy = M;
  if (gy < 1) gy = 1;
  return dim3((unsigned)gx, (unsigned)gy);
}

static int row_grid(long M) {
  long g = cdiv(M, SN_WAVES);
  if (g > SN_GRID_CAP) g = SN_GRID_CAP;
  return (int)g;
}

extern "C" {

int sn_block_size() { return SN_BLOCK; }
int sn_grid_cap() { return SN_GRID_CAP; }
int sn_chunk_rows() { return SN_CHUNK_ROWS; }
int sn_max_chunks() { return SN_MAX_CHUNKS; }

long sn_chunks(long M) {
  long c = cdiv(M, SN_CHUNK_ROWS);
  return c > SN_MAX_CHUNKS ? SN_MAX_CHUNKS : c;
}

long sn_col_blocks(long K) { return cdiv(K, SN_BLOCK); }

long sn_dot_blocks(long M, long K) {
  dim3 g = grid2d(M, cdiv(K, 8));
  return (long)g.x * g.y;
}

void launch_sn_forward(const void* W, void* Wsn, float* u, float* v,
                       float* u_out, float* v_out, float* sig, float* tpart,
                       float* t, float* nsq_part, float* s, long M, long K,
                       hipStream_t st) {
  long K8 = cdiv(K, 8);
  long nchunks = sn_chunks(M);
  long rpc = cdiv(M, nchunks);
  int nparts = (int)sn_col_blocks(K);
  int vec = use_vec(K, W, Wsn);
  const unsigned short* w = (const unsigned short*)W;
  hipLaunchKernelGGL(sn_col_partial,
                     dim3((unsigned)cdiv(K8, SN_BLOCK), (unsigned)nchunks),
                     dim3(SN_BLOCK), 0, st, w, (const float*)u, tpart, M, K,
                     K8, rpc, vec);
  hipLaunchKernelGGL(sn_col_finish, dim3((unsigned)nparts), dim3(SN_BLOCK), 0,
                     st, (const float*)tpart, t, nsq_part, K, (int)nchunks);
  hipLaunchKernelGGL(sn_row_pass<true>, dim3(row_grid(M)), dim3(SN_BLOCK), 0,
                     st, w, (const float*)t, (const float*)nsq_part, nparts,
                     s, M, K, K8, vec);
  hipLaunchKernelGGL(sn_finalize, dim3(1), dim3(SN_BLOCK), 0, st,
                     (const float*)t, (const float*)nsq_part, nparts,
                     (const float*)s, u, v, u_out, v_out, sig, M, K);
  hipLaunchKernelGGL(sn_scale, grid2d(M, K8), dim3(SN_BLOCK), 0, st, w,
                     (const float*)sig, (unsigned short*)Wsn, M, K, K8, vec);
}

void launch_sn_forward_eval(const void* W, void* Wsn, const float* u,
                            const float* v, float* sig, float* s, long M,
                            long K, hipStream_t st) {
  long K8 = cdiv(K, 8);
  int vec = use_vec(K, W, Wsn);
  const unsigned short* w = (const unsigned short*)W;
  hipLaunchKernelGGL(sn_row_pass<false>, dim3(row_grid(M)), dim3(SN_BLOCK), 0,
                     st, w, v, (const float*)nullptr, 0, s, M, K, K8, vec);
  hipLaunchKernelGGL(sn_sigma_eval, dim3(1), dim3(SN_BLOCK), 0, st,
                     (const float*)s, u, sig, M);
  hipLaunchKernelGGL(sn_scale, grid2d(M, K8), dim3(SN_BLOCK), 0, st, w,
                     (const float*)sig, (unsigned short*)Wsn, M, K, K8, vec);
}

void launch_sn_backward(const void* G, const void* Wsn, const float* u,
                        const float* v, const float* sig, float* dot_part,
                        void* dW, long M, long K, hipStream_t st) {
  long K8 = cdiv(K, 8);
  int vec = use_vec(K, G, Wsn, dW);
  dim3 grid = grid2d(M, K8);
  int nparts = (int)(grid.x * grid.y);
  hipLaunchKernelGGL(sn_dot_partial, grid, dim3(SN_BLOCK), 0, st,
                     (const unsigned short*)G, (const unsigned short*)Wsn,
                     dot_part, M, K, K8, vec);
  hipLaunchKernelGGL(sn_bwd_apply, grid, dim3(SN_BLOCK), 0, st,
                     (const unsigned short*)G, (const float*)dot_part, nparts,
                     u, v, sig, (unsigned short*)dW, M, K, K8, vec);
}

}  // extern "C"
