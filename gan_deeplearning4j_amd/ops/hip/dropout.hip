// Stochastic layers: inverted dropout fwd/bwd and additive Gaussian noise.
// Memory-bound family (same 16 B/lane geometry as elementwise.hip, G13/G11).
//
// Random stream: Philox4x32-10 (Random123 constants), counter-based, so the
// stream is a pure function of (block index, calls, seed). seed and calls
// are READ FROM DEVICE MEMORY (state = int64[2] = [seed, calls]), never
// passed as scalars: a captured hipGraph replays the same launch arguments
// forever, and the host bumps calls with a stream-ordered in-place add
// after the launch (part of the captured graph). The kernels only read the
// state, so blocks of one launch cannot race with the increment.
//
// Block i covers storage-order elements 8i..8i+7.
//   counter = (i lo, i hi, calls lo, calls hi), key = (seed lo, seed hi)
//   dropout: word j serves element 2j (low 16 bits) and 2j+1 (high 16 bits);
//            kept iff h < T, T = round(keep * 65536); y = bf16(x * 1/keep)
//   noise:   Philox blocks 2i and 2i+1; each block's words (w0,w1),(w2,w3)
//            are two Box-Muller pairs, u1 = (wa+1)*2^-32, u2 = wb*2^-32,
//            giving r*cos(2*pi*u2), r*sin(2*pi*u2), r = sqrt(-2 ln u1).

#include "common.h"

#define DROPOUT_BLOCK 256
#define DROPOUT_GRID_CAP 2048

#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

struct Philox4 {
  unsigned int w[4];
};

DEV_INLINE Philox4 philox4x32_10(unsigned int c0, unsigned int c1,
                                 unsigned int c2, unsigned int c3,
                                 unsigned int k0, unsigned int k1) {
  #pragma unroll
  for (int r = 0; r < 10; ++r) {
    unsigned int hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    unsigned int hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  Philox4 o;
  o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
  return o;
}

struct RngState {
  unsigned int k0, k1, t0, t1;
};

DEV_INLINE RngState load_state(const long long* __restrict__ state) {
  unsigned long long seed = (unsigned long long)state[0];
  unsigned long long calls = (unsigned long long)state[1];
  RngState s;
  s.k0 = (unsigned int)seed;
  s.k1 = (unsigned int)(seed >> 32);
  s.t0 = (unsigned int)calls;
  s.t1 = (unsigned int)(calls >> 32);
  return s;
}

DEV_INLINE Philox4 philox_block(unsigned long long blk, RngState s) {
  return philox4x32_10((unsigned int)blk, (unsigned int)(blk >> 32), s.t0,
                       s.t1, s.k0, s.k1);
}

// 16-bit uniform of element j (0..7) of a block
DEV_INLINE unsigned int drop_h(const Philox4& p, int j) {
  unsigned int w = p.w[j >> 1];
  return (j & 1) ? (w >> 16) : (w & 0xffffu);
}

// ------------------------------------------------------------ dropout fwd
__global__ void dropout_fwd_bf16(const s16x8* __restrict__ x,
                                 s16x8* __restrict__ y,
                                 unsigned char* __restrict__ mask,
                                 const long long* __restrict__ state,
                                 long n8, unsigned int thresh, float scale) {
  RngState st = load_state(state);
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n8; i += stride) {
    s16x8 v = x[i];
    Philox4 p = philox_block((unsigned long long)i, st);
    s16x8 o;
    unsigned int bits = 0;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      bool keep = drop_h(p, j) < thresh;
      bits |= (keep ? 1u : 0u) << j;
      o[j] = keep ? (short)f2bf(bf2f((unsigned short)v[j]) * scale) : (short)0;
    }
    y[i] = o;
    mask[i] = (unsigned char)bits;
  }
}

// partial last vector (n % 8 != 0): Philox block n/8, lanes 0..rem-1
__global__ void dropout_fwd_tail(const unsigned short* __restrict__ x,
                                 unsigned short* __restrict__ y,
                                 unsigned char* __restrict__ mask,
                                 const long long* __restrict__ state,
                                 long n8, long n, unsigned int thresh,
                                 float scale) {
  RngState st = load_state(state);
  Philox4 p = philox_block((unsigned long long)n8, st);
  int j = threadIdx.x;
  int rem = (int)(n - n8 * 8);
  if (j < rem) {
    bool keep = drop_h(p, j) < thresh;
    y[n8 * 8 + j] = keep ? f2bf(bf2f(x[n8 * 8 + j]) * scale)
                         : (unsigned short)0;
  }
  if (j == 0) {
    unsigned int bits = 0;
    for (int q = 0; q < rem; ++q)
      bits |= (drop_h(p, q) < thresh ? 1u : 0u) << q;
    mask[n8] = (unsigned char)bits;
  }
}

// ------------------------------------------------------------ dropout bwd
// dx = dy * scale * bit; the mask is the forward's, nothing is regenerated
__global__ void dropout_bwd_bf16(const s16x8* __restrict__ dy,
                                 const unsigned char* __restrict__ mask,
                                 s16x8* __restrict__ dx, long n8,
                                 float scale) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n8; i += stride) {
    s16x8 g = dy[i];
    unsigned int bits = mask[i];
    s16x8 o;
    #pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = ((bits >> j) & 1u)
                 ? (short)f2bf(bf2f((unsigned short)g[j]) * scale)
                 : (short)0;
    dx[i] = o;
  }
}

__global__ void dropout_bwd_tail(const unsigned short* __restrict__ dy,
                                 const unsigned char* __restrict__ mask,
                                 unsigned short* __restrict__ dx, long n8,
                                 long n, float scale) {
  int j = threadIdx.x;
  long i = n8 * 8 + j;
  if (j < 8 && i < n) {
    unsigned int bits = mask[n8];
    dx[i] = ((bits >> j) & 1u) ? f2bf(bf2f(dy[i]) * scale)
                               : (unsigned short)0;
  }
}

// ---------------------------------------------------------- gaussian noise
// One Box-Muller pair. -ln(u1) is evaluated so that neither end of (0,1]
// loses precision to the fp32 conversion of the 32-bit word: below 1/2 the
// word itself carries the relative precision, above it 1-u1 does.
DEV_INLINE void box_muller(unsigned int wa, unsigned int wb, float& n0,
                           float& n1) {
  float neg_ln;
  if (wa < 0x80000000u) {
    neg_ln = -logf(((float)wa + 1.0f) * 2.3283064365386963e-10f);
  } else {
    // u1 = 1 - m * 2^-32 with m = 2^32 - (wa + 1)
    float m = (float)(0xffffffffu - wa);
    neg_ln = -log1pf(-m * 2.3283064365386963e-10f);
  }
  float r = sqrtf(2.0f * neg_ln);
  float s, c;
  sincospif((float)wb * 4.656612873077393e-10f, &s, &c);  // 2*u2 = wb*2^-31
  n0 = r * c;
  n1 = r * s;
}

DEV_INLINE void normals8(unsigned long long blk, RngState st, float nrm[8]) {
  Philox4 a = philox_block(2ull * blk, st);
  Philox4 b = philox_block(2ull * blk + 1ull, st);
  box_muller(a.w[0], a.w[1], nrm[0], nrm[1]);
  box_muller(a.w[2], a.w[3], nrm[2], nrm[3]);
  box_muller(b.w[0], b.w[1], nrm[4], nrm[5]);
  box_muller(b.w[2], b.w[3], nrm[6], nrm[7]);
}

__global__ void gaussian_noise_fwd_bf16(const s16x8* __restrict__ x,
                                        s16x8* __restrict__ y,
                                        const long long* __restrict__ state,
                                        long n8, float stddev) {
  RngState st = load_state(state);
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n8; i += stride) {
    s16x8 v = x[i];
    float nrm[8];
    normals8((unsigned long long)i, st, nrm);
    s16x8 o;
    #pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = (short)f2bf(bf2f((unsigned short)v[j]) + stddev * nrm[j]);
    y[i] = o;
  }
}

__global__ void gaussian_noise_fwd_tail(const unsigned short* __restrict__ x,
                                        unsigned short* __restrict__ y,
                                        const long long* __restrict__ state,
                                        long n8, long n, float stddev) {
  RngState st = load_state(state);
  int j = threadIdx.x;
  long i = n8 * 8 + j;
  if (j < 8 && i < n) {
    float nrm[8];
    normals8((unsigned long long)n8, st, nrm);
    float mine = 0.f;
    #pragma unroll
    for (int q = 0; q < 8; ++q) mine = (q == j) ? nrm[q] : mine;
    y[i] = f2bf(bf2f(x[i]) + stddev * mine);
  }
}

// ------------------------------------------------------------- launchers
static int dropout_grid(long n8) {
  long g = (n8 + DROPOUT_BLOCK - 1) / DROPOUT_BLOCK;
  if (g > DROPOUT_GRID_CAP) g = DROPOUT_GRID_CAP;
  if (g < 1) g = 1;
  return (int)g;
}

extern "C" {

int dropout_grid_cap() { return DROPOUT_GRID_CAP; }
int dropout_block_size() { return DROPOUT_BLOCK; }

void launch_dropout_fwd(const void* x, void* y, void* mask,
                        const void* state, long n, unsigned int thresh,
                        float scale, hipStream_t s) {
  long n8 = n / 8;
  if (n8 > 0)
    hipLaunchKernelGGL(dropout_fwd_bf16, dim3(dropout_grid(n8)),
                       dim3(DROPOUT_BLOCK), 0, s, (const s16x8*)x, (s16x8*)y,
                       (unsigned char*)mask, (const long long*)state, n8,
                       thresh, scale);
  if (n % 8)
    hipLaunchKernelGGL(dropout_fwd_tail, dim3(1), dim3(64), 0, s,
                       (const unsigned short*)x, (unsigned short*)y,
                       (unsigned char*)mask, (const long long*)state, n8, n,
                       thresh, scale);
}

void launch_dropout_bwd(const void* dy, const void* mask, void* dx, long n,
                        float scale, hipStream_t s) {
  long n8 = n / 8;
  if (n8 > 0)
    hipLaunchKernelGGL(dropout_bwd_bf16, dim3(dropout_grid(n8)),
                       dim3(DROPOUT_BLOCK), 0, s, (const s16x8*)dy,
                       (const unsigned char*)mask, (s16x8*)dx, n8, scale);
  if (n % 8)
    hipLaunchKernelGGL(dropout_bwd_tail, dim3(1), dim3(64), 0, s,
                       (const unsigned short*)dy, (const unsigned char*)mask,
                       (unsigned short*)dx, n8, n, scale);
}

void launch_gaussian_noise_fwd(const void* x, void* y, const void* state,
                               long n, float stddev, hipStream_t s) {
  long n8 = n / 8;
  if (n8 > 0)
    hipLaunchKernelGGL(gaussian_noise_fwd_bf16, dim3(dropout_grid(n8)),
                       dim3(DROPOUT_BLOCK), 0, s, (const s16x8*)x, (s16x8*)y,
                       (const long long*)state, n8, stddev);
  if (n % 8)
    hipLaunchKernelGGL(gaussian_noise_fwd_tail, dim3(1), dim3(64), 0, s,
                       (const unsigned short*)x, (unsigned short*)y,
                       (const long long*)state, n8, n, stddev);
}

}  // extern "C"
