// bf16 MFMA GEMM kernels for gfx950 (CDNA4) — the conv/dense compute core.
//
// Two flavors cover every GEMM in the framework:
//
//  gemm_tn:  C[M][N] = act(A[M][K] . B[N][K]^T + bias)
//            both operands K-contiguous (TN form): conv/convT/dense forward
//            (A=im2col, B=weights) and data-grad (B=W^T).
//            128x128x64 tile, 4 waves, double-buffered LDS staged with
//            global_load_lds (16B), XOR-swizzled via the SOURCE address
//            (guide rule 21), mfma_f32_16x16x32_bf16 inner loop, LDS-staged
//            coalesced epilogue with fused bias+activation.
//            GATHER_A variant = implicit-GEMM convolution: the A operand is
//            gathered straight from the NHWC image (im2col fused into the
//            staging address computation; out-of-bounds/padded chunks are
//            redirected to a 16B zero page so global_load_lds stays
//            unconditional).
//
//  gemm_nt:  C[M][N] (fp32) += sum_k A[k][M] * B[k][N]
//            contraction over ROWS of both operands: weight-grad
//            (A=dOut, B=im2col). 128x128x64 tile, 8 waves, double-buffered
//            LDS staged with global_load_lds (operand rows land coalesced;
//            the stage for tile t+1 is issued before tile t's MFMAs),
//            fragments read by ds_read_b64_tr_b16 (hardware transpose),
//            split-K over blockIdx.z with fp32 atomics. Either operand may
//            be gathered from an NHWC image (implicit wgrad).  Fallback
//            of launch_gemm_nt: deep-K shapes with M, N >= 128 go to the
//            256-wide deep-pipelined core in gemm8p_nt.hip.
//
// K must be a multiple of 64 for gemm_tn (callers pad; gathered A pads by
// zero-page); gemm_nt handles arbitrary K by zero-fill.
//
// The gather address rule and the [row][8 slot] tile stagers are shared with
// fp8.hip and the 8-phase kernels: conv_gather.h.

#include "conv_gather.h"

// ---------------------------------------------------------------------------
// TN kernel
// ---------------------------------------------------------------------------
constexpr int TN_BM = 128, TN_BN = 128, TN_BK = 64;
constexpr int TN_TILE_B = TN_BM * TN_BK * 2;  // 16 KiB per operand tile

DEV_INLINE bf16x8 tn_frag(const char* lds, int row, int kslot) {
  int byte = row * 128 + ((kslot ^ (row & 7)) * 16);
  return *(const bf16x8*)(lds + byte);
}

template <bool GATHER_A>
__global__ __launch_bounds__(256, 2) void gemm_tn_core(
    const unsigned short* __restrict__ A, const unsigned short* __restrict__ B,
    unsigned short* __restrict__ C, float* __restrict__ Cf,
    const float* __restrict__ bias, int M, int N, int K, long lda, long ldb,
    int act, float slope, ConvGather ga,
    const unsigned short* __restrict__ zp,
    float* __restrict__ bn_part) {
  __shared__ __attribute__((aligned(128))) char lds[4 * TN_TILE_B];
  auto abuf = [&](int i) -> char* { return lds + (i ? 2 * TN_TILE_B : 0); };
  auto bbuf = [&](int i) -> char* {
    return lds + TN_TILE_B + (i ? 2 * TN_TILE_B : 0);
  };

  // XCD-aware swizzle (T1, bijective variant) over M-tiles
  const int nwgx = gridDim.x;
  const int bidx = xcd_remap(blockIdx.x, nwgx);
  const int m0 = bidx * TN_BM;
  const int n0 = blockIdx.y * TN_BN;

  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wr = wid >> 1, wc = wid & 1;
  const int fr = lane & 15, fq = lane >> 4;

  f32x4 acc[4][4];
  #pragma unroll
  for (int i = 0; i < 4; ++i)
    #pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int ntiles = K / TN_BK;
  TnGatherStager<256, unsigned short> gs;
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
        gs.stage(A, ga, zp, (t + 1) * TN_BK, abuf(cur ^ 1));
      else
        tn_stage_rows<256, 4>(A, m0, M, lda, (t + 1) * TN_BK, abuf(cur ^ 1));
      tn_stage_rows<256, 4>(B, n0, N, ldb, (t + 1) * TN_BK, bbuf(cur ^ 1));
    }
    const char* Al = abuf(cur);
    const char* Bl = bbuf(cur);
    #pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      bf16x8 a[4], b[4];
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        a[mi] = tn_frag(Al, wr * 64 + mi * 16 + fr, kc * 4 + fq);
      #pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        b[ni] = tn_frag(Bl, wc * 64 + ni * 16 + fr, kc * 4 + fq);
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // ---- epilogue: bias + activation, LDS-staged coalesced stores ------
  if (C != nullptr && (N & 7) == 0) {
    unsigned short* ctile = (unsigned short*)lds;  // [128][128] bf16
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
          ctile[lr * 128 + lc] = f2bf(act_fwd(acc[mi][ni][r] + bv, act,
                                              slope));
        }
      }
    }
    __syncthreads();
    const int t = threadIdx.x;
    #pragma unroll
    for (int i = 0; i < 8; ++i) {
      int piece = i * 256 + t;       // 2048 16B pieces = 128 rows x 16
      int row = piece >> 4;
      int seg = piece & 15;
      int grow = m0 + row;
      int gcol = n0 + seg * 8;
      if (grow < M && gcol < N) {
        long crow = grow;
        if (GATHER_A && ga.mode == 2) crow = scatter_row(ga, grow);
        s16x8 v = *(const s16x8*)(ctile + row * 128 + seg * 8);
        if (gcol + 8 <= N) {
          *(s16x8*)(&C[crow * N + gcol]) = v;
        } else {
          for (int j = 0; j < 8 && gcol + j < N; ++j)
            C[crow * N + gcol + j] = (unsigned short)v[j];
        }
      }
    }
    // optional fused BN-statistics: per-channel (tile-col) sum/sumsq of
    // the post-activation tile -> partials [gridDim.x][2N] (second pass =
    // bn_stats_sum2). Rows beyond M are masked out.
    if (bn_part != nullptr) {
      float* red = (float*)(lds + 2 * TN_TILE_B);  // past the 32KB ctile
      const int col = t & 127;
      const int rl = t >> 7;  // 2 row-lanes x 64 rows
      float s = 0.f, ss = 0.f;
      for (int row = rl; row < 128; row += 2) {
        if (m0 + row < M) {
          float v = bf2f(ctile[row * 128 + col]);
          s += v;
          ss += v * v;
        }
      }
      red[t] = s;
      red[256 + t] = ss;
      __syncthreads();
      if (rl == 0 && n0 + col < N) {
        s += red[128 + col];
        ss += red[256 + 128 + col];
        bn_part[(long)blockIdx.x * 2 * N + n0 + col] = s;
        bn_part[(long)blockIdx.x * 2 * N + N + n0 + col] = ss;
      }
    }
    return;
  }
  // fallback (fp32 out or N not a multiple of 8): direct predicated stores
  #pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    #pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      int col = n0 + wc * 64 + ni * 16 + fr;
      if (col >= N) continue;
      float bv = bias != nullptr ? bias[col] : 0.f;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m0 + wr * 64 + mi * 16 + fq * 4 + r;
        if (row >= M) continue;
        long crow = row;
        if (GATHER_A && ga.mode == 2) crow = scatter_row(ga, row);
        float v = act_fwd(acc[mi][ni][r] + bv, act, slope);
        if (C != nullptr)
          C[crow * N + col] = f2bf(v);
        else
          Cf[crow * N + col] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Single-shot TN for K in {64, 128} (the K-thin dcol/dense family):
// every K-tile is staged ONCE up front (no double-buffer loop, no
// per-tile vmcnt(0)+barrier drain pairs) and the block runs
// stage -> one wait -> MFMA -> epilogue.  Same 128x128 tile / 4 waves /
// 2 blocks per CU geometry as gemm_tn_core; these shapes are bound by
// the C-write stream + per-block overhead, so the win is structural
// overhead removal, not MFMA scheduling.
// ---------------------------------------------------------------------------
template <int KT, bool GATHER_A = false>  // KT = 64 or 128
__global__ __launch_bounds__(256, 2) void gemm_tn_kshort(
    const unsigned short* __restrict__ A, const unsigned short* __restrict__ B,
    unsigned short* __restrict__ C, const float* __restrict__ bias, int M,
    int N, long lda, long ldb, int act, float slope, int direct_epi,
    ConvGather ga, const unsigned short* __restrict__ zp) {
  constexpr int NT = KT / TN_BK;  // K-tiles
  __shared__ __attribute__((aligned(128))) char lds[2 * NT * TN_TILE_B];
  auto abuf = [&](int t) -> char* { return lds + t * TN_TILE_B; };
  auto bbuf = [&](int t) -> char* { return lds + (NT + t) * TN_TILE_B; };

  const int nwgx = gridDim.x;
  const int bidx = xcd_remap(blockIdx.x, nwgx);
  const int m0 = bidx * TN_BM;
  const int n0 = blockIdx.y * TN_BN;
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wr = wid >> 1, wc = wid & 1;
  const int fr = lane & 15, fq = lane >> 4;

  f32x4 acc[4][4];
  #pragma unroll
  for (int i = 0; i < 4; ++i)
    #pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  TnGatherStager<256, unsigned short> gs;
  if (GATHER_A) gs.init(ga, m0, M);
  #pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (GATHER_A)
      gs.stage(A, ga, zp, t * TN_BK, abuf(t));
    else
      tn_stage_rows<256, 4>(A, m0, M, lda, t * TN_BK, abuf(t));
    tn_stage_rows<256, 4>(B, n0, N, ldb, t * TN_BK, bbuf(t));
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  #pragma unroll
  for (int t = 0; t < NT; ++t) {
    const char* Al = abuf(t);
    const char* Bl = bbuf(t);
    #pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      bf16x8 a[4], b[4];
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        a[mi] = tn_frag(Al, wr * 64 + mi * 16 + fr, kc * 4 + fq);
      #pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        b[ni] = tn_frag(Bl, wc * 64 + ni * 16 + fr, kc * 4 + fq);
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
  }

  if ((N & 7) == 0 && direct_epi != 1) {
    unsigned short* ctile = (unsigned short*)lds;  // [128][128] bf16
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
          ctile[lr * 128 + lc] = f2bf(act_fwd(acc[mi][ni][r] + bv, act,
                                              slope));
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
        s16x8 v = *(const s16x8*)(ctile + row * 128 + seg * 8);
        if (direct_epi == 2)  // probe: nontemporal C stream
          __builtin_nontemporal_store(v, (s16x8*)(&C[crow * N + gcol]));
        else
          *(s16x8*)(&C[crow * N + gcol]) = v;
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
        long crow = row;
        if (GATHER_A && ga.mode == 2) crow = scatter_row(ga, row);
        C[crow * N + col] = f2bf(act_fwd(acc[mi][ni][r] + bv, act,
                                              slope));
      }
    }
}

// ---------------------------------------------------------------------------
// 256x128x64 TN variant (GDLJ_TN256): +37% arithmetic intensity per staged
// byte (2M MACs per 48 KiB vs 1M per 32 KiB) at the SAME 8-wave/CU
// occupancy — one 512-thread block per CU with 96 KiB dynamic LDS
// (2x32 KiB A + 2x16 KiB B double buffers; the 64 KiB epilogue ctile
// reuses the A region). No mode-2 scatter / fp32-out / bn_part here —
// the launcher falls back to the 128 tile for those.
// ---------------------------------------------------------------------------
constexpr int T2_BM = 256, T2_BN = 128, T2_BK = 64;
constexpr int T2_AT = T2_BM * T2_BK * 2;  // 32 KiB
constexpr int T2_BT = T2_BN * T2_BK * 2;  // 16 KiB

template <bool GATHER_A>
__global__ __launch_bounds__(512, 1) void gemm_tn_core256(
    const unsigned short* __restrict__ A, const unsigned short* __restrict__ B,
    unsigned short* __restrict__ C, const float* __restrict__ bias, int M,
    int N, int K, long lda, long ldb, int act, float slope, ConvGather ga,
    const unsigned short* __restrict__ zp) {
  extern __shared__ __attribute__((aligned(128))) char lds[];
  auto abuf = [&](int i) -> char* { return lds + (i ? T2_AT : 0); };
  auto bbuf = [&](int i) -> char* {
    return lds + 2 * T2_AT + (i ? T2_BT : 0);
  };

  const int nwgx = gridDim.x;
  const int bidx = xcd_remap(blockIdx.x, nwgx);
  const int m0 = bidx * T2_BM;
  const int n0 = blockIdx.y * T2_BN;

  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wr = wid >> 1, wc = wid & 1;  // 4(m) x 2(n) wave grid
  const int fr = lane & 15, fq = lane >> 4;

  f32x4 acc[4][4];
  #pragma unroll
  for (int i = 0; i < 4; ++i)
    #pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int ntiles = K / T2_BK;
  TnGatherStager<512, unsigned short> gs;
  if (GATHER_A) {
    gs.init(ga, m0, M);
    gs.stage(A, ga, zp, 0, abuf(0));
  } else {
    tn_stage_rows<512, 4>(A, m0, M, lda, 0, abuf(0));
  }
  tn_stage_rows<512, 2>(B, n0, N, ldb, 0, bbuf(0));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    int cur = t & 1;
    if (t + 1 < ntiles) {
      if (GATHER_A)
        gs.stage(A, ga, zp, (t + 1) * T2_BK, abuf(cur ^ 1));
      else
        tn_stage_rows<512, 4>(A, m0, M, lda, (t + 1) * T2_BK, abuf(cur ^ 1));
      tn_stage_rows<512, 2>(B, n0, N, ldb, (t + 1) * T2_BK, bbuf(cur ^ 1));
    }
    const char* Al = abuf(cur);
    const char* Bl = bbuf(cur);
    #pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      bf16x8 a[4], b[4];
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        a[mi] = tn_frag(Al, wr * 64 + mi * 16 + fr, kc * 4 + fq);
      #pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        b[ni] = tn_frag(Bl, wc * 64 + ni * 16 + fr, kc * 4 + fq);
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // epilogue: bias + act, LDS-staged coalesced stores (ctile 256x128 bf16
  // = 64 KiB in the A-buffer region)
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
          ctile[lr * 128 + lc] = f2bf(act_fwd(acc[mi][ni][r] + bv, act,
                                              slope));
        }
      }
    }
    __syncthreads();
    const int t = threadIdx.x;
    #pragma unroll
    for (int i = 0; i < 8; ++i) {
      int piece = i * 512 + t;       // 4096 16B pieces = 256 rows x 16
      int row = piece >> 4;
      int seg = piece & 15;
      int grow = m0 + row;
      int gcol = n0 + seg * 8;
      if (grow < M && gcol < N) {
        s16x8 v = *(const s16x8*)(ctile + row * 128 + seg * 8);
        if (gcol + 8 <= N) {
          *(s16x8*)(&C[(long)grow * N + gcol]) = v;
        } else {
          for (int j = 0; j < 8 && gcol + j < N; ++j)
            C[(long)grow * N + gcol + j] = (unsigned short)v[j];
        }
      }
    }
    return;
  }
  // N % 8 != 0 fallback: direct predicated stores
  #pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    #pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      int col = n0 + wc * 64 + ni * 16 + fr;
      if (col >= N) continue;
      float bv = bias != nullptr ? bias[col] : 0.f;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m0 + wr * 64 + mi * 16 + fq * 4 + r;
        if (row >= M) continue;
        C[(long)row * N + col] = f2bf(act_fwd(acc[mi][ni][r] + bv, act,
                                              slope));
      }
    }
  }
}

// ---------------------------------------------------------------------------
// NT kernel (weight grad): C[M][N] += sum_k A[k][M]*B[k][N], fp32 out.
//
// Contraction runs over operand ROWS, so rows stage straight into LDS with
// global_load_lds (fully coalesced) in a [kb][mb][4k][16m] window layout,
// and MFMA fragments come out via ds_read_b64_tr_b16 (gfx950 hardware
// transpose read: per 16-lane group, lane l receives column l of a [4][16]
// row-major window — verified by tools/probe_tr16.hip).
// ---------------------------------------------------------------------------
constexpr int NT_BM = 128, NT_BN = 128, NT_BK = 64;
constexpr int NT_TILE_E = NT_BM * NT_BK;     // elements per operand tile
constexpr int NT_THREADS = 512;              // 8 waves: 2(m) x 4(n)

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

// chunk c (16B = 8 elems) of the window-linear LDS image:
//   window w = c>>3 (64 elems: [4 rows k][16 cols m]), j = (c>>1)&3, h = c&1
//   w = kb*(BM/16) + mb
// source = operand row (k0 + kb*4 + j), cols (c0 + mb*16 + h*8 .. +8)
DEV_INLINE void nt_stage(const unsigned short* __restrict__ g, int k0, int K,
                         int c0, int L, long ldl,
                         const unsigned short* __restrict__ zp, char* lds) {
  const int t = threadIdx.x;
  const int wid = t >> 6;
  #pragma unroll
  for (int i = 0; i < 2; ++i) {
    int c = i * 512 + t;
    int w = c >> 3;
    int j = (c >> 1) & 3;
    int h = c & 1;
    int kb = w >> 3;
    int mb = w & 7;
    int row = k0 + kb * 4 + j;
    const unsigned short* src = zp;
    if (row < K) {
      int col = c0 + mb * 16 + h * 8;
      col = min(col, max(0, L - 8));  // M-edge clamp (rows >= M not stored)
      src = g + (long)row * ldl + col;
    }
    char* dst = lds + (i * 512 + wid * 64) * 16;
    GLDS16(src, dst);
  }
}

// gathered flavor: operand is the im2col of an NHWC image
// (contraction row = np; tile column = rsc coordinate).  The column-side
// k_decode (tap r,s + channel) is K-loop-invariant per thread — each
// thread stages the same two rsc coordinates every K-step — so it is
// hoisted into registers once (the row side np varies with k0 and is
// decoded per step).
struct NtGatherCols {
  int r[2], s[2], cc[2];
  bool in_rsc[2];

  DEV_INLINE void init(const ConvGather& g, int c0) {
    const int t = threadIdx.x;
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
      int c = i * 512 + t;
      int w = c >> 3;
      int h = c & 1;
      int mb = w & 7;
      int kk = c0 + mb * 16 + h * 8;
      in_rsc[i] = kk < g.rsc;
      if (in_rsc[i])
        k_decode(g, (unsigned)kk, r[i], s[i], cc[i]);
      else
        r[i] = s[i] = cc[i] = 0;
    }
  }
};

DEV_INLINE void nt_stage_gather(const unsigned short* __restrict__ img,
                                const ConvGather& g, const NtGatherCols& gc,
                                int k0, int K,
                                const unsigned short* __restrict__ zp,
                                char* lds) {
  const int t = threadIdx.x;
  const int wid = t >> 6;
  #pragma unroll
  for (int i = 0; i < 2; ++i) {
    int c = i * 512 + t;
    int w = c >> 3;
    int j = (c >> 1) & 3;
    int kb = w >> 3;
    int np = k0 + kb * 4 + j;
    const unsigned short* src = zp;
    if (np < K && gc.in_rsc[i]) {
      int n, ho, wo;
      np_decode(g, (unsigned)np, n, ho, wo);
      bool valid;
      const unsigned short* p = gather_addr(g, img, n, ho, wo, gc.r[i],
                                            gc.s[i], gc.cc[i], valid);
      if (valid) src = p;
    }
    char* dst = lds + (i * 512 + wid * 64) * 16;
    GLDS16(src, dst);
  }
}

// fragment: lane holds col m = (mb*16 + fr), k = kc*32 + fq*8 + (0..7)
DEV_INLINE bf16x8 nt_tr_frag(const unsigned short* lds, int kc, int mb) {
  const int l = threadIdx.x & 63;
  const int g = l >> 4;
  int kb = kc * 8 + 2 * g;
  const unsigned short* a0 = lds + ((kb * 8 + mb) * 64 + (l & 15) * 4);
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4*)a0);
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4*)(a0 + 512));
  bf16x8 r;
  #pragma unroll
  for (int j = 0; j < 4; ++j) {
    r[j] = lo[j];
    r[4 + j] = hi[j];
  }
  return r;
}

// GMODE: 0 = plain/plain, 1 = A gathered, 2 = B gathered
template <int GMODE>
__global__ __launch_bounds__(NT_THREADS, 2) void gemm_nt_core(
    const unsigned short* __restrict__ A, const unsigned short* __restrict__ B,
    float* __restrict__ C, int M, int N, int K, long lda, long ldb,
    int kchunks_per_block, int use_atomic, ConvGather gg,
    const unsigned short* __restrict__ zp) {
  __shared__ __attribute__((aligned(128))) unsigned short lds[4 * NT_TILE_E];
  auto albuf = [&](int i) -> unsigned short* {
    return lds + (i ? 2 * NT_TILE_E : 0);
  };
  auto blbuf = [&](int i) -> unsigned short* {
    return lds + NT_TILE_E + (i ? 2 * NT_TILE_E : 0);
  };

  const int m0 = blockIdx.x * NT_BM;
  const int n0 = blockIdx.y * NT_BN;
  // (static young-half wave priority measured NEUTRAL here — at 2
  // blocks/CU the SIMDs arbitrate across blocks, unlike the 1-block/CU
  // 8p template where it is +4.9-8.9%; tools/ab_gemm8p.py)
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wr = wid >> 2, wc = wid & 3;
  const int fr = lane & 15, fq = lane >> 4;

  f32x4 acc[4][2];
  #pragma unroll
  for (int i = 0; i < 4; ++i)
    #pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int kchunks = (K + NT_BK - 1) / NT_BK;
  int kt0 = blockIdx.z * kchunks_per_block;
  int kt1 = min(kt0 + kchunks_per_block, kchunks);
  if (kt0 >= kt1) return;

  NtGatherCols gca, gcb;
  if (GMODE == 1) gca.init(gg, m0);
  if (GMODE == 2) gcb.init(gg, n0);
  auto stage_a = [&](int kt, char* buf) {
    if (GMODE == 1)
      nt_stage_gather(A, gg, gca, kt * NT_BK, K, zp, buf);
    else
      nt_stage(A, kt * NT_BK, K, m0, M, lda, zp, buf);
  };
  auto stage_b = [&](int kt, char* buf) {
    if (GMODE == 2)
      nt_stage_gather(B, gg, gcb, kt * NT_BK, K, zp, buf);
    else
      nt_stage(B, kt * NT_BK, K, n0, N, ldb, zp, buf);
  };

  stage_a(kt0, (char*)albuf(0));
  stage_b(kt0, (char*)blbuf(0));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int kt = kt0; kt < kt1; ++kt) {
    int cur = (kt - kt0) & 1;
    if (kt + 1 < kt1) {
      stage_a(kt + 1, (char*)albuf(cur ^ 1));
      stage_b(kt + 1, (char*)blbuf(cur ^ 1));
    }
    const unsigned short* Al = albuf(cur);
    const unsigned short* Bl = blbuf(cur);
    #pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      bf16x8 a[4], b[2];
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        a[mi] = nt_tr_frag(Al, kc, wr * 4 + mi);
      #pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        b[ni] = nt_tr_frag(Bl, kc, wc * 2 + ni);
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  #pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    #pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      int col = n0 + wc * 32 + ni * 16 + fr;
      if (col >= N) continue;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m0 + wr * 64 + mi * 16 + fq * 4 + r;
        if (row >= M) continue;
        if (use_atomic)
          atomicAdd(&C[(long)row * N + col], acc[mi][ni][r]);
        else
          C[(long)row * N + col] = acc[mi][ni][r];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// K-short launch for K in {64, 128}: picks the compile-time KT instantiation
template <bool GATHER_A>
static int launch_kshort(const void* A, const void* B, void* C,
                         const float* bias, int M, int N, int K, long lda,
                         long ldb, int act, float slope, int direct_epi,
                         const ConvGather& ga, const void* zp, hipStream_t s) {
  dim3 grid(ceil_div(M, TN_BM), ceil_div(N, TN_BN));
  auto* kern = K == 64 ? gemm_tn_kshort<64, GATHER_A>
                       : gemm_tn_kshort<128, GATHER_A>;
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, (const unsigned short*)A,
                     (const unsigned short*)B, (unsigned short*)C, bias, M, N,
                     lda, ldb, act, slope, direct_epi, ga,
                     (const unsigned short*)zp);
  return (int)grid.x;
}

extern "C" {

// The 8-phase deep-pipelined 256x256 TN core (gemm8p.hip) is the default
// for large bf16 TN shapes; this file's 128-tile kernels remain the fallback
// (fp32 out, bn_part fusion, small N/K/M).

// env-gated 256-row TN tile (see gemm_tn_core256). Opted in with
// GDLJ_TN256=1; requires bf16 output, no bn_part, gather mode != 2,
// and enough rows to fill the chip at 1 block/CU.
static int t2_enabled() {
  static const int v = [] {
    int on = env_flag("GDLJ_TN256", 0);
    if (on) {
      (void)hipFuncSetAttribute(
          reinterpret_cast<const void*>(&gemm_tn_core256<false>),
          hipFuncAttributeMaxDynamicSharedMemorySize, 2 * T2_AT + 2 * T2_BT);
      (void)hipFuncSetAttribute(
          reinterpret_cast<const void*>(&gemm_tn_core256<true>),
          hipFuncAttributeMaxDynamicSharedMemorySize, 2 * T2_AT + 2 * T2_BT);
    }
    return on;
  }();
  return v;
}

static int kshort_enabled() {
  static const int v = env_flag("GDLJ_KSHORT", 1);
  return v;
}

int launch_gemm_tn(const void* A, const void* B, void* C_bf16, float* C_f32,
                   const float* bias, int M, int N, int K, long lda, long ldb,
                   int act, float slope, float* bn_part, hipStream_t s) {
  if (C_bf16 != nullptr && bn_part == nullptr && (K == 64 || K == 128) &&
      kshort_enabled()) {
    // probe: direct stores instead of the LDS-staged epilogue
    static const int depi = env_flag("GDLJ_KSHORT_EPI", 0);
    return launch_kshort<false>(A, B, C_bf16, bias, M, N, K, lda, ldb, act,
                                slope, depi, ConvGather{}, nullptr, s);
  }
  if (C_bf16 != nullptr && bn_part == nullptr &&
      gemm_tn_8p_eligible(M, N, K)) {
    ConvGather dummy{};
    return launch_gemm_tn_8p(A, B, C_bf16, bias, M, N, K, lda, ldb, act,
                             slope, 0, dummy, nullptr, s);
  }
  if (t2_enabled() && C_bf16 != nullptr && bn_part == nullptr &&
      M >= 8 * T2_BM) {
    dim3 grid(ceil_div(M, T2_BM), ceil_div(N, T2_BN));
    ConvGather dummy{};
    hipLaunchKernelGGL((gemm_tn_core256<false>), grid, dim3(512),
                       2 * T2_AT + 2 * T2_BT, s, (const unsigned short*)A,
                       (const unsigned short*)B, (unsigned short*)C_bf16,
                       bias, M, N, K, lda, ldb, act, slope, dummy, nullptr);
    return (int)grid.x;
  }
  dim3 grid(ceil_div(M, TN_BM), ceil_div(N, TN_BN));
  ConvGather dummy{};
  hipLaunchKernelGGL((gemm_tn_core<false>), grid, dim3(256), 0, s,
                     (const unsigned short*)A, (const unsigned short*)B,
                     (unsigned short*)C_bf16, C_f32, bias, M, N, K, lda, ldb,
                     act, slope, dummy, nullptr, bn_part);
  return (int)grid.x;
}

static int direct_conv_enabled() {
  static const int v = env_flag("GDLJ_DIRECT_CONV", 1);
  return v;
}

// implicit-GEMM conv forward / gathered-A TN: A is an NHWC image; M = the
// number of patch positions; K = kpad (zero page covers k >= rsc).  The
// small-C forward family goes to the LDS-image direct conv (conv_direct.hip).
int launch_gemm_tn_gather(const void* img, const void* B, void* C_bf16,
                          const float* bias, int M, int N, int K, long ldb,
                          int act, float slope, ConvGather ga,
                          const void* zero_page, float* bn_part,
                          hipStream_t s) {
  if (bn_part == nullptr && ga.mode == 0 && ldb == K &&
      direct_conv_enabled() &&
      launch_conv_direct_smallc(img, B, C_bf16, bias, zero_page, ga.N, ga.H,
                                ga.W, ga.C, ga.Ho, ga.Wo, ga.R, ga.S,
                                ga.stride, ga.pad, N, K, act, slope, s))
    return ceil_div(M, 128);
  if (bn_part == nullptr && (K == 64 || K == 128) && kshort_enabled())
    return launch_kshort<true>(img, B, C_bf16, bias, M, N, K, 0, ldb, act,
                               slope, 0, ga, zero_page, s);
  if (bn_part == nullptr && gemm_tn_8p_eligible(M, N, K)) {
    return launch_gemm_tn_8p(img, B, C_bf16, bias, M, N, K, 0, ldb, act,
                             slope, 1, ga, zero_page, s);
  }
  if (t2_enabled() && bn_part == nullptr && ga.mode != 2 && M >= 8 * T2_BM) {
    dim3 grid(ceil_div(M, T2_BM), ceil_div(N, T2_BN));
    hipLaunchKernelGGL((gemm_tn_core256<true>), grid, dim3(512),
                       2 * T2_AT + 2 * T2_BT, s, (const unsigned short*)img,
                       (const unsigned short*)B, (unsigned short*)C_bf16,
                       bias, M, N, K, 0, ldb, act, slope, ga,
                       (const unsigned short*)zero_page);
    return (int)grid.x;
  }
  dim3 grid(ceil_div(M, TN_BM), ceil_div(N, TN_BN));
  hipLaunchKernelGGL((gemm_tn_core<true>), grid, dim3(256), 0, s,
                     (const unsigned short*)img, (const unsigned short*)B,
                     (unsigned short*)C_bf16, nullptr, bias, M, N, K, 0, ldb,
                     act, slope, ga, (const unsigned short*)zero_page,
                     bn_part);
  return (int)grid.x;
}

void launch_gemm_nt(const void* A, const void* B, float* C, int M, int N,
                    int K, long lda, long ldb, int splitk, int gmode,
                    ConvGather gg, const void* zp, hipStream_t s) {
  // the deep-pipelined 256-wide core (gemm8p_nt.hip) takes the shapes it
  // wins on and re-derives split-K for its own tile count; gemm_nt_core
  // below is the fallback and the A/B arm (GDLJ_NT8P=0)
  if (launch_gemm_nt_8p(A, B, C, M, N, K, lda, ldb, splitk, gmode, gg, zp, s))
    return;
  int kchunks = (K + NT_BK - 1) / NT_BK;
  if (splitk > kchunks) splitk = kchunks;
  int per_block = (kchunks + splitk - 1) / splitk;
  dim3 grid(ceil_div(M, NT_BM), ceil_div(N, NT_BN), splitk);
  int ua = splitk > 1 ? 1 : 0;
  const unsigned short* z = (const unsigned short*)zp;
  if (gmode == 1)
    hipLaunchKernelGGL((gemm_nt_core<1>), grid, dim3(NT_THREADS), 0, s,
                       (const unsigned short*)A, (const unsigned short*)B, C,
                       M, N, K, lda, ldb, per_block, ua, gg, z);
  else if (gmode == 2)
    hipLaunchKernelGGL((gemm_nt_core<2>), grid, dim3(NT_THREADS), 0, s,
                       (const unsigned short*)A, (const unsigned short*)B, C,
                       M, N, K, lda, ldb, per_block, ua, gg, z);
  else
    hipLaunchKernelGGL((gemm_nt_core<0>), grid, dim3(NT_THREADS), 0, s,
                       (const unsigned short*)A, (const unsigned short*)B, C,
                       M, N, K, lda, ldb, per_block, ua, gg, z);
}

}  // extern "C"
