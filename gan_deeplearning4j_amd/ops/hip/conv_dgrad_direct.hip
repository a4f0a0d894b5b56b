// Direct strided conv dgrad for gfx950 — fuses the dcol GEMM + col2im
// round trip into one parity-decomposed kernel.
//
// The default strided dgrad materializes dcol[np][R*S*C8] (13.9 GB at
// the DCGAN-64 conv2 shape) and re-reads it in col2im.  Here each
// block owns a tile of dx pixels of ONE output-parity class
// (hi%stride, wi%stride) EXCLUSIVELY — so no atomics on dx, and every
// tap of the class's reduced tap set is valid for every pixel (no
// stride^2 MFMA waste, unlike a naive direct transposed conv).  The
// block stages the contributing dy region into LDS once (coalesced,
// zero-page halo cells absorb image borders), streams the transposed
// weight slices tap-by-tap (double-buffered, counted vmcnt), and
// accumulates complete per-pixel sums in MFMA registers.  Because the
// sums are complete, the epilogue also applies the producer's
// activation backward (col2im_dact's fusion) and emits its
// bias-gradient partials.  Each class pixel's C8-channel row is a
// whole 128-byte line, so the scattered stores stay line-coalesced.
//
// GEMM view per class tap (r,s): dx[px][c] += dy_rs[px][co] *
// Wt[(r*S+s)*C8 + c][co], Wt = the [R*S*C8][Ko8] transposed weight
// pack the dcol path already caches (gpu_ops "wt" cache).
//
// Tile: BM class-pixels x 64 c (BM 128 or 64), 4 waves; LDS = dy
// region + 32 KiB W double-buffer (ctile reuses the W area).
// Eligibility (launcher): stride == 2, Wc | BM, (Hc*Wc) % BM == 0,
// C8 % 64 == 0, Ko8 % 128 == 0 == ldw, region + 32 KiB <= 80 KiB
// (two blocks per CU).
// Covers conv2/conv3-class dgrads of the DCGAN family; everything
// else falls back to dcol+col2im (gemm.hip / im2col.hip).
//
// Three kernels run this arithmetic: conv_dgrad_direct (one-shot: a block
// per tile, class and c-tile), conv_dgrad_direct_p (persistent, class-fused,
// two blocks per CU; the launchers try it before the one-shot kernel, which
// stays as the fallback and A/B arm, GDLJ_DGRAD_PERSIST=0) and
// conv_dgrad_direct_w (one block per CU, for the 8x8 class grid, tried
// first; GDLJ_DGRAD_WIDE=0 skips it).  The arithmetic itself — geometry,
// region stager, slice body, ctile, epilogue piece, partial reduction — is
// in conv_dgrad_parts.h, once; the kernels below are the three pipelines
// around it.

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "common.h"
#include "conv_dgrad_parts.h"

// 64-row x 64-k staged sub-tile, same swizzled layout/frag read as the
// proven tn layout (conv_gather.h tn_stage_rows / gemm.hip tn_frag geometry).
DEV_INLINE void cdd_stage_w64(const unsigned short* __restrict__ g,
                              long ldk, int k0, char* lds) {
  const int t = threadIdx.x;
  const int wid = t >> 6;
  #pragma unroll
  for (int i = 0; i < 2; ++i) {
    int chunk = i * 256 + t;  // 512 chunks = row*8 + slot
    int row = chunk >> 3;
    int slot = chunk & 7;
    int gslot = slot ^ (row & 7);
    const unsigned short* src = g + (long)row * ldk + k0 + gslot * 8;
    char* dst = lds + (i * 256 + wid * 64) * 16;
    GLDS16(src, dst);
  }
}

// MI = pixel fragments per wave (BM = MI * 64).
//
// The same kernel serves the strided TRANSPOSED-conv forward (G side):
// y[ho,wo,co] = sum over parity-valid taps of x[(ho+p-r)/2][ci] *
// W[ci,co,r,s] is the identical gather; pass x as `dy`, the
// [R*S*Co8][Cin] "w2a" pack as `Wt`, bias_fwd + act for the fused
// epilogue, and stats_part ([kPartRows][2*C8]) for fused BN statistics.
//
// The region is the window of the block's own class only; Ko8 need not be
// a power of two here (stage_region<.., false>).
template <int MI>
__global__ __launch_bounds__(256, 2) void conv_dgrad_direct(
    const unsigned short* __restrict__ dy,   // [N][Ho][Wo][Ko8]
    const unsigned short* __restrict__ Wt,   // [R*S*C8][ldw], k = co
    unsigned short* __restrict__ dx,         // [N][H][W][C8]
    const unsigned short* __restrict__ y0,   // producer act out (or null)
    float* __restrict__ part,                // [kPartRows][C8] f32 (or null)
    const float* __restrict__ bias_fwd,      // convT fwd bias (or null)
    float* __restrict__ stats_part,          // [kPartRows][2*C8] f32 (or null)
    const unsigned short* __restrict__ zp,   // 16B zero page
    int Nb, int H, int W, int C8, int Ho, int Wo, int Ko8, long ldw,
    int R, int S, int pad, int act, float slope,
    int Hc, int Wc, int rgn_rows, int rgn_cols, FastDiv fWc) {
  using namespace cdd;
  constexpr int BM = MI * 64;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* rgn = lds;                                  // dy region
  const int rgn_b = rgn_rows * rgn_cols * Ko8 * 2;
  auto wbuf = [&](int i) -> char* { return lds + rgn_b + i * WSLICE_B; };

  // XCD-aware swizzle over class-pixel tiles
  const int nwgx = gridDim.x;
  const int bidx = xcd_remap(blockIdx.x, nwgx);
  const int np0 = bidx * BM;
  const int hwc = Hc * Wc;
  const int n = np0 / hwc;         // once per block: plain div is fine
  const int cp0 = np0 - n * hwc;
  const int hc0 = cp0 / Wc;        // Wc | BM => whole class-row start
  const int cy = blockIdx.y;       // c-tile: channels [cy*64, cy*64+64)
  const int cls = blockIdx.z;      // parity class
  const int qh = cls >> 1, qw = cls & 1;

  const int Rc = p_ntap(qh, pad, R), Sc = p_ntap(qw, pad, S);
  const int rb0 = p_boff(qh, pad), wb0 = p_boff(qw, pad);
  const int lo_h = p_lo(qh, pad, R);      // dy row of region row 0, - hc0
  const int lo_w = p_lo(qw, pad, S);      // dy col of region col 0

  stage_region<256, false>(dy, zp, rgn, n, 1, Nb, hc0 + lo_h, lo_w, rgn_rows,
                           rgn_cols, Ho, Wo, Ko8);

  const int wid = threadIdx.x >> 6;
  const int fr = threadIdx.x & 15;
  const LanePx<MI> px = lane_px<MI>(wid * (MI * 16), 1, hwc, 0, fWc, Wc);

  const int nj = Ko8 >> 7;           // 128-co chunks per tap
  const int nslice = Rc * Sc * nj;
  auto wsrc_for = [&](int sl) {
    int tapj = sl / nj, j = sl - tapj * nj;
    int rc_ = tapj / Sc, sc_ = tapj - rc_ * Sc;
    return w_slice_src(Wt, ldw, C8, S, pad, cls, cy, rc_, sc_, j);
  };

  // first W slice, then one wait covers region + slice 0
  cdd_stage_w64(wsrc_for(0), ldw, 0, wbuf(0));
  cdd_stage_w64(wsrc_for(0), ldw, 64, wbuf(0) + 8 * 1024);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  f32x4 acc[MI][4];
  zero_acc(acc);

  for (int sl = 0; sl < nslice; ++sl) {
    int tapj = sl / nj;
    int j = sl - tapj * nj;
    int rc_ = tapj / Sc, sc_ = tapj - rc_ * Sc;
    int cur = sl & 1;
    if (sl + 1 < nslice) {
      const unsigned short* ws = wsrc_for(sl + 1);
      cdd_stage_w64(ws, ldw, 0, wbuf(cur ^ 1));
      cdd_stage_w64(ws, ldw, 64, wbuf(cur ^ 1) + 8 * 1024);
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    slice_mfma<MI, 4, false>(acc, rgn, wbuf(cur), px, rb0 - rc_ - lo_h,
                             wb0 - sc_ - lo_w, rgn_cols, Ko8, j, 0);
    __syncthreads();  // all waves done with wbuf(cur) before restage
  }

  // ---- epilogue: ctile in the W-buffer area; dgrad mode applies the
  // producer act' downstream, convT-fwd mode applies bias+act here ----
  // This kernel keeps its own copy of the ctile transpose and the epilogue
  // piece, the same expressions as write_ctile / epilogue_piece: through
  // the shared ones (bias preloaded, pact / stats as arguments) it measured
  // 0.05 ms (0.6 %) slower per call at the conv2 shapes, a block being only
  // four to six slices long (profiles/dgrad_parts_refactor.md).
  unsigned short* ctile = (unsigned short*)wbuf(0);  // [BM][64]
  const int fq = (threadIdx.x & 63) >> 4;
  #pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    #pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      int lc = ni * 16 + fr;
      float bv = bias_fwd != nullptr ? bias_fwd[cy * 64 + lc] : 0.f;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        int lr = wid * (MI * 16) + mi * 16 + fq * 4 + r;
        float v = acc[mi][ni][r];
        if (bias_fwd != nullptr) v = act_fwd(v + bv, act, slope);
        ctile[lr * 64 + lc] = f2bf(v);
      }
    }
  }
  __syncthreads();
  const int t2 = threadIdx.x;
  const int seg = t2 & 7;            // fixed c-block per thread
  Partials<1> sums;
  sums.clear();
  #pragma unroll
  for (int i = 0; i < BM / 32; ++i) {
    int piece = i * 256 + t2;        // BM*8 pieces = BM rows x 8 segs
    int row = piece >> 3;
    int hl = (int)fdiv((unsigned)row, fWc);
    int wcl = row - hl * Wc;
    int hi = qh + 2 * (hc0 + hl);
    int wi = qw + 2 * wcl;
    long addr = (((long)n * H + hi) * W + wi) * C8 + cy * 64 + seg * 8;
    s16x8 v = *(const s16x8*)(ctile + row * 64 + seg * 8);
    if (y0 != nullptr) {
      s16x8 yv = *(const s16x8*)(y0 + addr);
      #pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        float d = bf2f((unsigned short)v[jj]) *
                  act_bwd_from_y(bf2f((unsigned short)yv[jj]), act, slope);
        v[jj] = (short)f2bf(d);
        sums.bsum[0][jj] += d;
      }
    }
    if (stats_part != nullptr) {
      #pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        float yv = bf2f((unsigned short)v[jj]);
        sums.ssum[0][jj] += yv;
        sums.ssq[0][jj] += yv * yv;
      }
    }
    *(s16x8*)(dx + addr) = v;
  }
  // all conditions are block-uniform, so the reductions' barriers are
  // safe; the region is dead after the MFMA loop
  flush_partials<32, 1>((float*)rgn, sums, y0 != nullptr ? part : nullptr,
                        stats_part, C8, cy * 64);
}

// ---------------------------------------------------------------------
// Persistent class-fused variant.
//
// A block walks a strided sequence of tiles (grid = CUs x 2, no
// inter-block communication).  A tile is one BM class-pixel tile times
// ALL of C8 and either all four parity classes or, where the full
// union region does not fit two blocks per CU, the two classes of one
// row parity (qsplit).  The union dy region of the tile's classes is
// staged ONCE and every class / 64-channel c-tile runs its tap set out
// of it, so the region is no longer re-staged per class and per c-tile.
//
// The W slices form one stream across classes, c-tiles and tiles: the
// slice after the last one of a (class, c-tile) is already in flight
// while the epilogue runs, and the epilogue's ctile is the W buffer the
// last slice just released (the prefetch targets the other one), so the
// double buffer never drains.  The next tile's region is issued right
// after the tile's last MFMA slice, under the last epilogue.
//
// Barriers are cdd::p_lds_barrier (LDS traffic only): __syncthreads()
// would drain the prefetched W slice / region at every barrier.
//
// Bias / BN-statistics partials stay in registers across all tiles and
// go through the LDS tree + atomics once per block; only the order of
// those fp32 partial sums differs from the one-shot kernel.
//
// PACT = y0 given (producer act-backward epilogue).
template <int MI, int NCT, bool PACT>
__global__ __launch_bounds__(256, 2) void conv_dgrad_direct_p(
    const unsigned short* __restrict__ dy,   // [N][Ho][Wo][Ko8]
    const unsigned short* __restrict__ Wt,   // [R*S*C8][ldw], k = co
    unsigned short* __restrict__ dx,         // [N][H][W][C8]
    const unsigned short* __restrict__ y0,   // producer act out (or null)
    float* __restrict__ part,                // [kPartRows][C8] f32 (or null)
    const float* __restrict__ bias_fwd,      // convT fwd bias (or null)
    float* __restrict__ stats_part,          // [kPartRows][2*C8] f32 (or null)
    const unsigned short* __restrict__ zp,   // 16B zero page
    int H, int W, int C8, int Ho, int Wo, int Ko8, long ldw,
    int R, int S, int pad, int act, float slope,
    int Hc, int Wc, int rgn_rows, int rgn_cols, FastDiv fWc,
    int ntiles, int qsplit) {
  using namespace cdd;
  constexpr int BM = MI * 64;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* rgn = lds;                                  // union dy region
  const int rgn_b = rgn_rows * rgn_cols * Ko8 * 2;
  auto wbuf = [&](int i) -> char* { return lds + rgn_b + i * WSLICE_B; };

  const int rows_c = BM / Wc;
  const int hwc = Hc * Wc;
  const int tpi = hwc / BM;                // pixel tiles per image
  const int nj = Ko8 >> 7;                 // 128-co chunks per tap

  // union column window over both column parities
  const int lo_w = p_union_lo(pad, S);
  // union row window: both row parities, or the tile's own one (qsplit)
  auto row_lo = [&](int tile) {
    return qsplit ? p_lo(tile & 1, pad, R) : p_union_lo(pad, R);
  };

  // a tile's region; Ko8 is a power of two (launcher); every tile lies
  // inside the batch
  auto stage_tile = [&](int tile) {
    int pt = qsplit ? (tile >> 1) : tile;
    int n = pt / tpi;
    int hc0 = (pt - n * tpi) * rows_c;
    stage_region<256, true>(dy, zp, rgn, n, 1, n + 1, hc0 + row_lo(tile),
                            lo_w, rgn_rows, rgn_cols, Ho, Wo, Ko8);
  };

  // W source of slice sl of (class cls, c-tile ct)
  auto wsrc_for = [&](int cls, int ct, int sl) {
    int Sc = p_ntap(cls & 1, pad, S);
    int tapj = sl / nj, j = sl - tapj * nj;
    int rc_ = tapj / Sc, sc_ = tapj - rc_ * Sc;
    return w_slice_src(Wt, ldw, C8, S, pad, cls, ct, rc_, sc_, j);
  };

  const int wid = threadIdx.x >> 6;
  const int fr = threadIdx.x & 15;
  const LanePx<MI> px = lane_px<MI>(wid * (MI * 16), 1, hwc, 0, fWc, Wc);

  const int t2 = threadIdx.x;
  const int seg = t2 & 7;            // fixed c-block per thread
  Partials<NCT> sums;
  sums.clear();

  // convT-forward bias of this lane's columns, loaded once: a global
  // load inside the epilogue would make the compiler drain the
  // in-flight prefetches to get at its value
  float biasv[NCT][4];
  #pragma unroll
  for (int k = 0; k < NCT; ++k)
    #pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      biasv[k][ni] =
          bias_fwd != nullptr ? bias_fwd[k * 64 + ni * 16 + fr] : 0.f;
      // consume the value here, ahead of every LDS-DMA load, so its
      // wait is placed now and not at the uses inside the tile loop
      asm volatile("" : "+v"(biasv[k][ni]));
    }

  // prologue: first region + first W slice; the first in-loop wait
  // covers both (loads complete in issue order)
  int tile = blockIdx.x;
  const int cls0 = qsplit ? (tile & 1) * 2 : 0;
  stage_tile(tile);
  cdd_stage_w64(wsrc_for(cls0, 0, 0), ldw, 0, wbuf(0));
  cdd_stage_w64(wsrc_for(cls0, 0, 0), ldw, 64, wbuf(0) + 8 * 1024);

  int g = 0;                         // running slice count -> W buffer
  for (; tile < ntiles; tile += gridDim.x) {
    const int pt = qsplit ? (tile >> 1) : tile;
    const int n = pt / tpi;
    const int hc0 = (pt - n * tpi) * rows_c;
    const int cb = qsplit ? (tile & 1) * 2 : 0;
    const int ce = qsplit ? cb + 2 : 4;
    const int ntile = tile + (int)gridDim.x;
    const bool has_next = ntile < ntiles;
    const int lo_h = row_lo(tile);

    for (int cls = cb; cls < ce; ++cls) {
      const int qh = cls >> 1, qw = cls & 1;
      const int Rc = p_ntap(qh, pad, R), Sc = p_ntap(qw, pad, S);
      const int rb0 = p_boff(qh, pad), wb0 = p_boff(qw, pad);
      const int nslice = Rc * Sc * nj;

      for (int ct = 0; ct < NCT; ++ct) {
        const bool last_ct = (cls + 1 == ce) && (ct + 1 == NCT);
        f32x4 acc[MI][4];
        zero_acc(acc);

        for (int sl = 0; sl < nslice; ++sl, ++g) {
          int tapj = sl / nj;
          int j = sl - tapj * nj;
          int rc_ = tapj / Sc, sc_ = tapj - rc_ * Sc;
          int cur = g & 1;
          // next slice of the stream: this (class, c-tile), else the
          // next c-tile, class or tile
          const unsigned short* ws = nullptr;
          if (sl + 1 < nslice) ws = wsrc_for(cls, ct, sl + 1);
          else if (ct + 1 < NCT) ws = wsrc_for(cls, ct + 1, 0);
          else if (cls + 1 < ce) ws = wsrc_for(cls + 1, 0, 0);
          else if (has_next)
            ws = wsrc_for(qsplit ? (ntile & 1) * 2 : 0, 0, 0);
          if (ws != nullptr) {
            cdd_stage_w64(ws, ldw, 0, wbuf(cur ^ 1));
            cdd_stage_w64(ws, ldw, 64, wbuf(cur ^ 1) + 8 * 1024);
            // Loads and stores retire in issue order.  Right after an
            // epilogue the newest operations are its BM/32 dx stores
            // and the 4 loads just issued; this slice's W and the
            // region are older, so the stores may stay outstanding.
            if (sl == 0 && g > 0)
              asm volatile("s_waitcnt vmcnt(%0)" ::"i"(4 + BM / 32)
                           : "memory");
            else
              asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
          } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          }
          p_lds_barrier();
          slice_mfma<MI, 4, false>(acc, rgn, wbuf(cur), px, rb0 - rc_ - lo_h,
                                   wb0 - sc_ - lo_w, rgn_cols, Ko8, j, 0);
          p_lds_barrier();  // all waves done with wbuf(cur) + region
        }

        // the tile's last MFMA slice is done: the region is dead, put
        // the next tile's region in flight under this epilogue
        if (last_ct && has_next) stage_tile(ntile);
        // keep the region loads ahead of the epilogue's stores (the
        // counted wait above relies on that order)
        asm volatile("" ::: "memory");

        // output addresses of this thread's pieces; the producer's
        // activation output is fetched now so that its latency runs
        // under the ctile transpose
        long eaddr[BM / 32];
        s16x8 yin[BM / 32];
        #pragma unroll
        for (int i = 0; i < BM / 32; ++i) {
          int row = (i * 256 + t2) >> 3;  // BM*8 pieces = BM rows x 8 segs
          ClassPx p = class_px(row, 1, hwc, fWc, Wc);
          int hi = qh + 2 * (hc0 + p.h);
          int wi = qw + 2 * p.w;
          eaddr[i] = (((long)n * H + hi) * W + wi) * C8 + ct * 64 + seg * 8;
          yin[i] = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
        if constexpr (PACT) {
          #pragma unroll
          for (int i = 0; i < BM / 32; ++i)
            yin[i] = *(const s16x8*)(y0 + eaddr[i]);
        }

        // ---- epilogue: ctile = the W buffer the last slice released
        // (the in-flight prefetch targets the other one) ----
        unsigned short* ctile = (unsigned short*)wbuf((g - 1) & 1);
        float bv[4];
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          bv[ni] = 0.f;
          #pragma unroll
          for (int k = 0; k < NCT; ++k)
            if (ct == k) bv[ni] = biasv[k][ni];
        }
        write_ctile<MI, 4>(ctile, acc, bv, bias_fwd != nullptr, act, slope,
                           wid * (MI * 16), 0);
        p_lds_barrier();
        if constexpr (PACT) {
          // take the wait for all fetched y0 pieces here, once; left to
          // the uses below, each one also waits for the previous store
          #pragma unroll
          for (int i = 0; i < BM / 32; ++i)
            asm volatile("" : "+v"(yin[i]));
        }
        #pragma unroll
        for (int i = 0; i < BM / 32; ++i) {
          int row = (i * 256 + t2) >> 3;
          epilogue_piece<NCT>(ctile + row * 64 + seg * 8, dx + eaddr[i], PACT,
                              yin[i], stats_part != nullptr, ct, act, slope,
                              sums);
        }
        p_lds_barrier();  // ctile reads done before it is restaged as W
      }
    }
  }

  // ---- once per block: LDS tree + atomics over the register partials
  // (region and W buffers are dead, nothing is in flight) ----
  flush_partials<32, NCT>((float*)rgn, sums, PACT ? part : nullptr,
                          stats_part, C8, 0);
}

// ---------------------------------------------------------------------
// Wide variant of the persistent kernel: ONE 8-wave block per CU.
//
// For the 8x8 class grid (conv3 dgrad / convT2 forward class).  A tile
// is BM = 128 class pixels = the class grids of TWO images, times all of
// C8 and all four parity classes out of one full-union region per image;
// there is no qsplit.  Twice the pixels per W slice halves the W bytes
// staged per output pixel, and the LDS of the whole CU pays for a third
// W buffer: the slice TWO ahead is issued before the current one is
// consumed, so a slice has two slice times to cross the L2.  (The
// 16x16 class grid, one image per BM = 256 tile, was built and measured
// slower than conv_dgrad_direct_p: profiles/dgrad_wide_ab.md.)
//
// The W stream is endless: the issue cursor walks (class, c-tile, slice)
// cyclically and does not look at the tile, so every iteration issues
// exactly two loads per thread and every counted wait is a constant.
// The two slices issued past the block's last tile land in free buffers
// and are drained before the block ends.
//
// A slice costs ONE barrier: wait for slice g, barrier, issue slice g+2
// into the buffer of slice g-1 (every wave has read it: its LDS reads
// are complete when it arrives at the barrier), fetch all fragments of
// slice g, then its MFMAs (slice_mfma's FETCH_AHEAD), which run into the
// next slice's scalar work and wait.
//
// Wait accounting (loads and stores retire in issue order).  Per thread
// a slice is 2 loads, an epilogue ST = BM/64 dx stores, and with PACT
// the y0 pieces of a (class, c-tile) are ST loads issued at its top,
// under its whole slice loop.  At the wait of slice g the only newer
// slice is g+1 (2); on the first slice after an epilogue also that
// epilogue's stores and this c-tile's y0 loads; on the first slice of a
// tile the region, which was issued after slice g+1 and must have
// landed too, so there only the stores and the y0 loads may stay
// outstanding.  A tile with an absent image (odd Nb) issues fewer
// stores / y0 loads in some waves: it takes the counts without them,
// which only waits for more.
// The PACT counts hold only while the compiler leaves the y0 loads at
// the top of the c-tile, ahead of its first slice wait: were they sunk
// to their use in the epilogue, that wait would let slice g itself stay
// outstanding.  The asm memory clobbers of the waits and barriers pin
// them today; after a compiler change re-check in the .s that the
// global_load_dwordx4 of y0 sit at the head of the c-tile loop
// (profiles/dgrad_wide_ab.md lists what to look at).
//
// Wave tile: 32 px x 32 c (4 pixel groups x 2 channel halves), 4 MFMA
// per kc against 4 ds_read_b128 (conv_dgrad_direct_p<1,..>: 4 against
// 5).  The fp32 bias / BN partials are summed in another order than in
// the other two kernels.
namespace cdd {
constexpr int W_NBUF = 3;
constexpr int W_THREADS = 512;
constexpr int W_BM = 128;                // class pixels per tile
constexpr int W_LDS_MAX = 160 * 1024;    // the whole LDS of a CU

// one [64c][128co] W slice by the 512-thread block: 2 loads per thread,
// same LDS image as two cdd_stage_w64 calls (k0 = 0, 64)
DEV_INLINE void w_stage_slice(const unsigned short* __restrict__ g, long ldk,
                              char* lds) {
  const int t = threadIdx.x;
  const int wid = t >> 6;
  const int row = t >> 3;
  const int gslot = (t & 7) ^ (row & 7);
  const unsigned short* src = g + (long)row * ldk + gslot * 8;
  GLDS16(src, lds + wid * 1024);
  GLDS16(src + 64, lds + 8 * 1024 + wid * 1024);
}

template <int N>
DEV_INLINE void w_wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
}  // namespace cdd

template <int NCT, bool PACT>
__global__ __launch_bounds__(512, 1) void conv_dgrad_direct_w(
    const unsigned short* __restrict__ dy,   // [N][Ho][Wo][Ko8]
    const unsigned short* __restrict__ Wt,   // [R*S*C8][ldw], k = co
    unsigned short* __restrict__ dx,         // [N][H][W][C8]
    const unsigned short* __restrict__ y0,   // producer act out (or null)
    float* __restrict__ part,                // [kPartRows][C8] f32 (or null)
    const float* __restrict__ bias_fwd,      // convT fwd bias (or null)
    float* __restrict__ stats_part,          // [kPartRows][2*C8] f32 (or null)
    const unsigned short* __restrict__ zp,   // 16B zero page
    int Nb, int H, int W, int C8, int Ho, int Wo, int Ko8, long ldw,
    int R, int S, int pad, int act, float slope,
    int Hc, int Wc, int rgn_rows, int rgn_cols, FastDiv fWc, int ntiles) {
  using namespace cdd;
  constexpr int MI = 2, NI = 2;       // wave tile: 32 px x 32 c
  constexpr int WC = 4 / NI;          // waves across the 64 channels
  constexpr int BM = W_BM;            // 4 pixel groups x 32 px
  constexpr int ST = BM / 64;         // dx stores per thread per epilogue
  constexpr int YL = PACT ? ST : 0;   // y0 loads per thread per c-tile
  static_assert((8 / WC) * MI * 16 == BM && BM * 64 * 2 == WSLICE_B,
                "wave tile; the ctile is one W buffer");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* rgn = lds;                    // union dy regions, one per image

  const int hwc = Hc * Wc;            // class pixels per image
  const int imgs = BM / hwc;          // 2 (launcher)
  const int rgn_img_b = rgn_rows * rgn_cols * Ko8 * 2;
  const int rgn_b = imgs * rgn_img_b;
  auto wbuf = [&](int i) -> char* { return lds + rgn_b + i * WSLICE_B; };
  const int nj = Ko8 >> 7;            // 128-co chunks per tap

  // union window over both parities, per axis
  const int lo_w = p_union_lo(pad, S);
  const int lo_h = p_union_lo(pad, R);

  // a tile's regions, an image past Nb all zero; Ko8 is a power of two
  // (launcher)
  auto stage_tile = [&](int tile) {
    stage_region<W_THREADS, true>(dy, zp, rgn, tile * imgs, imgs, Nb, lo_h,
                                  lo_w, rgn_rows, rgn_cols, Ho, Wo, Ko8);
  };

  // issue cursor of the endless W stream, in the consumer's order:
  // class, c-tile, tap row, tap column, 128-co chunk (counters, no
  // divisions: the slice loop's scalar work is on the critical path)
  int i_cls = 0, i_ct = 0, i_rc = 0, i_sc = 0, i_j = 0;
  auto issue_w = [&](int buf) {
    w_stage_slice(
        w_slice_src(Wt, ldw, C8, S, pad, i_cls, i_ct, i_rc, i_sc, i_j), ldw,
        wbuf(buf));
    if (++i_j == nj) {
      i_j = 0;
      if (++i_sc == p_ntap(i_cls & 1, pad, S)) {
        i_sc = 0;
        if (++i_rc == p_ntap(i_cls >> 1, pad, R)) {
          i_rc = 0;
          if (++i_ct == NCT) {
            i_ct = 0;
            i_cls = (i_cls + 1) & 3;
          }
        }
      }
    }
  };

  const int wid = threadIdx.x >> 6;
  const int fr = threadIdx.x & 15;
  const int pg = wid / WC;            // pixel group of this wave
  const int ch = wid - pg * WC;       // channel part of this wave
  const int wrow0 = pg * (MI * 16);   // first tile row of this wave
  const int wcol0 = ch * (NI * 16);   // first channel of this wave

  // a 16-pixel fragment never straddles two images: hwc is a multiple
  // of 16
  const LanePx<MI> px = lane_px<MI>(wrow0, imgs, hwc, rgn_img_b, fWc, Wc);

  const int t2 = threadIdx.x;
  const int seg = t2 & 7;             // fixed c-block per thread
  Partials<NCT> sums;
  sums.clear();

  // convT-forward bias of this lane's columns, loaded and consumed ahead
  // of every LDS-DMA load (see conv_dgrad_direct_p)
  float biasv[NCT][NI];
  #pragma unroll
  for (int k = 0; k < NCT; ++k)
    #pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      biasv[k][ni] = bias_fwd != nullptr
                         ? bias_fwd[k * 64 + wcol0 + ni * 16 + fr]
                         : 0.f;
      asm volatile("" : "+v"(biasv[k][ni]));
    }

  // this thread's epilogue pieces: piece e is row (e*512 + t2) >> 3 of
  // the tile (e = image of the pair), 8 channels at seg
  int erow[ST], eimg[ST], eoff[ST];
  #pragma unroll
  for (int e = 0; e < ST; ++e) {
    int row = (e * W_THREADS + t2) >> 3;
    ClassPx p = class_px(row, imgs, hwc, fWc, Wc);
    erow[e] = row;
    eimg[e] = p.img;
    eoff[e] = (2 * p.h * W + 2 * p.w) * C8 + seg * 8;
  }

  // prologue: first region + the first two W slices; the first in-loop
  // wait covers the region and slice 0
  int tile = blockIdx.x;
  stage_tile(tile);
  issue_w(0);
  issue_w(1);

  int cur = 0;                        // W buffer of the current slice
  bool first_slice = true;
  for (; tile < ntiles; tile += gridDim.x) {
    const int n0 = tile * imgs;
    const int ntile = tile + (int)gridDim.x;
    const bool has_next = ntile < ntiles;
    const bool tile_full = n0 + imgs <= Nb;

    for (int cls = 0; cls < 4; ++cls) {
      const int qh = cls >> 1, qw = cls & 1;
      const int Rc = p_ntap(qh, pad, R), Sc = p_ntap(qw, pad, S);
      const int rb0 = p_boff(qh, pad), wb0 = p_boff(qw, pad);

      for (int ct = 0; ct < NCT; ++ct) {
        const bool first_ct = cls == 0 && ct == 0;
        const bool last_ct = cls == 3 && ct + 1 == NCT;

        // output addresses of this thread's pieces; with PACT the
        // producer's activation output is fetched now, under the whole
        // slice loop of this c-tile
        long eaddr[ST];
        bool evalid[ST];
        s16x8 yin[ST];
        #pragma unroll
        for (int e = 0; e < ST; ++e) {
          int n = n0 + eimg[e];
          evalid[e] = n < Nb;
          eaddr[e] = ((long)n * H + qh) * W * C8 + (long)qw * C8 + eoff[e] +
                     ct * 64;
          yin[e] = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
        if constexpr (PACT) {
          #pragma unroll
          for (int e = 0; e < ST; ++e)
            if (evalid[e]) yin[e] = *(const s16x8*)(y0 + eaddr[e]);
        }

        f32x4 acc[MI][NI];
        zero_acc(acc);

        bool first_of_ct = true;
        for (int rc_ = 0; rc_ < Rc; ++rc_)
        for (int sc_ = 0; sc_ < Sc; ++sc_)
        for (int j = 0; j < nj; ++j) {
          // this slice has landed (counts: see the kernel's header)
          if (!first_of_ct) {
            w_wait_vm<2>();
          } else if (!tile_full) {
            if (first_ct && !first_slice) w_wait_vm<0>();
            else w_wait_vm<2>();
          } else if (first_slice) {
            w_wait_vm<2 + YL>();
          } else if (first_ct) {
            w_wait_vm<ST + YL>();
          } else {
            w_wait_vm<2 + ST + YL>();
          }
          first_slice = false;
          first_of_ct = false;
          // the one barrier of a slice: every wave's part of this slice
          // is in LDS, and every wave has finished reading the previous
          // slice, whose buffer takes the slice two ahead
          p_lds_barrier();
          issue_w(cur == 0 ? 2 : cur - 1);
          slice_mfma<MI, NI, true>(acc, rgn, wbuf(cur), px, rb0 - rc_ - lo_h,
                                   wb0 - sc_ - lo_w, rgn_cols, Ko8, j, wcol0);
          cur = cur == 2 ? 0 : cur + 1;
        }
        // every wave is done with the last slice's W buffer (the ctile)
        // and, on the tile's last c-tile, with the region
        p_lds_barrier();

        // the region is dead: put the next tile's region in flight under
        // this epilogue; with PACT after the y0 pieces are taken (below),
        // so that their wait does not cover it
        if constexpr (!PACT) {
          if (last_ct && has_next) stage_tile(ntile);
        }
        asm volatile("" ::: "memory");

        // ---- epilogue: ctile = the W buffer the last slice released
        // (slices g+1, g+2 sit in the other two) ----
        unsigned short* ctile =
            (unsigned short*)wbuf(cur == 0 ? 2 : cur - 1);
        float bv[NI];
        #pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
          bv[ni] = 0.f;
          #pragma unroll
          for (int k = 0; k < NCT; ++k)
            if (ct == k) bv[ni] = biasv[k][ni];
        }
        write_ctile<MI, NI>(ctile, acc, bv, bias_fwd != nullptr, act, slope,
                            wrow0, wcol0);
        p_lds_barrier();
        if constexpr (PACT) {
          // Take the wait for the y0 pieces here, once.  The compiler
          // cannot count the loads of the slice loop in between and
          // waits for vmcnt(0), i.e. also for the two prefetched slices;
          // loading y0 by inline asm with a counted wait here was tried,
          // but the compiler copies the destination registers ahead of
          // that wait.
          #pragma unroll
          for (int e = 0; e < ST; ++e) asm volatile("" : "+v"(yin[e]));
          if (last_ct && has_next) stage_tile(ntile);
          asm volatile("" ::: "memory");
        }
        #pragma unroll
        for (int e = 0; e < ST; ++e) {
          if (!evalid[e]) continue;
          epilogue_piece<NCT>(ctile + erow[e] * 64 + seg * 8, dx + eaddr[e],
                              PACT, yin[e], stats_part != nullptr, ct, act,
                              slope, sums);
        }
        // the ctile reads are complete before the next slice's barrier,
        // behind which the buffer is restaged
      }
    }
  }

  // ---- once per block: drain the two slices issued past the last
  // tile, then LDS tree + atomics over the register partials ----
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  flush_partials<W_THREADS / 8, NCT>((float*)rgn, sums,
                                     PACT ? part : nullptr, stats_part, C8,
                                     0);
}

// ---------------------------------------------------------------------
// Every instantiation that exists, once: O(MI) one-shot, P(MI, NCT, PACT)
// persistent, W(NCT, PACT) wide.  The dynamic-LDS opt-in and the three
// dispatches below are generated from it, so an instantiation cannot be
// launched without its opt-in.
#define CDD_INSTANCES(O, P, W)                                          \
  O(2) O(1)                                                             \
  P(2, 1, false) P(2, 2, false) P(1, 1, false) P(1, 2, false)           \
  P(2, 1, true) P(2, 2, true) P(1, 1, true) P(1, 2, true)               \
  W(1, false) W(2, false) W(1, true) W(2, true)
#define CDD_NONE(...)

namespace cdd {
// LDS of the 256-thread kernels: what their plans may use (two blocks per
// CU) and what the launch opts in to
constexpr int P_LDS_PLAN = 80 * 1024;
constexpr int P_LDS_MAX = 120 * 1024;

static void opt_in_lds(const void* fn, int bytes) {
  (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                            bytes);
}

// All of them on the first launch of any: set lazily per instantiation, the
// call could fall into a stream capture.
static void set_attrs_once() {
  static int attr_done = 0;
  if (attr_done) return;
#define CDD_ATTR_O(MI_) \
  opt_in_lds((const void*)&conv_dgrad_direct<MI_>, P_LDS_MAX);
#define CDD_ATTR_P(MI_, NCT_, PACT_) \
  opt_in_lds((const void*)&conv_dgrad_direct_p<MI_, NCT_, PACT_>, P_LDS_MAX);
#define CDD_ATTR_W(NCT_, PACT_) \
  opt_in_lds((const void*)&conv_dgrad_direct_w<NCT_, PACT_>, W_LDS_MAX);
  CDD_INSTANCES(CDD_ATTR_O, CDD_ATTR_P, CDD_ATTR_W)
#undef CDD_ATTR_O
#undef CDD_ATTR_P
#undef CDD_ATTR_W
  attr_done = 1;
}

// A plan asked for an instantiation the table does not have (the plans
// admit none): say so and launch nothing.
static void no_instance(const char* kernel, int mi, int nct) {
  fprintf(stderr, "%s: no instantiation for MI=%d NCT=%d, not launched\n",
          kernel, mi, nct);
}

// ---- plans.  Eligibility ({} is kind 0: not taken).
// What every direct kernel needs.  R,S >= 2 keeps every parity class's tap
// set non-empty (ntap >= 1).
static bool eligible(int H, int W, int C8, int Ko8, long ldw, int R, int S,
                     int stride) {
  if (stride != 2 || C8 % 64 != 0 || Ko8 % 128 != 0 || ldw != Ko8)
    return false;
  return R >= 2 && S >= 2 && R <= 8 && S <= 8 && !(H & 1) && !(W & 1);
}
// On top of it for the persistent kernels: C8 64 or 128 (register partials
// per c-tile) and Ko8 a power of two (shift/mask cell decode).
static bool eligible_persistent(int H, int W, int C8, int Ko8, long ldw,
                                int R, int S, int stride, int pad) {
  return eligible(H, W, C8, Ko8, ldw, R, S, stride) && C8 > 0 && C8 <= 128 &&
         (Ko8 & (Ko8 - 1)) == 0 && pad >= 0;
}
// a tile of bm class pixels is whole class rows of one image
static bool tile_fits(int Hc, int Wc, int bm) {
  return Wc <= bm && bm % Wc == 0 && (Hc * Wc) % bm == 0;
}
// The stager's chunk swizzle slot ^ (cc & (co_chunks - 1)) permutes the
// chunks of a cell if co_chunks is a power of two; otherwise a chunk can
// come from the next cell.  For the other Ko8 this admits only regions whose
// columns stay below the lowest set bit of co_chunks: a sufficient condition,
// not the exact one (with 48 chunks, mask 0b101111, columns 16..31 still
// permute and the first wrong column is 32), so a few geometries that
// computed correctly on the one-shot kernel go to dcol + col2im as well.
static bool swizzle_ok(int Ko8, int rgn_cols) {
  int co_chunks = Ko8 >> 3;
  return (co_chunks & (co_chunks - 1)) == 0 ||
         rgn_cols <= (co_chunks & -co_chunks);
}
// Region of a plan: the one-shot kernel stages the window of one class
// (the larger parity's on each axis), the persistent ones the union of the
// column parities and of the row parities (qsplit: one row parity).
struct Region { int rows, cols; };
static Region plan_region(DgradDirectPlan p, int H, int W, int R, int S,
                          int pad) {
  int Hc = H / 2, Wc = W / 2;
  int rows_c = p.wide ? Hc : p.bm / Wc;
  return {p_axis_extent(rows_c, pad, R, p.kind == 1 || p.qsplit != 0),
          p_axis_extent(Wc, pad, S, p.kind == 1)};
}
// Fills p.lds_bytes: `imgs` regions + nwbuf W buffers.  False where that
// exceeds `budget` or the region cannot be staged.
static bool plan_lds(DgradDirectPlan& p, int H, int W, int Ko8, int R, int S,
                     int pad, int imgs, int nwbuf, int budget) {
  Region g = plan_region(p, H, W, R, S, pad);
  p.lds_bytes = imgs * g.rows * g.cols * Ko8 * 2 + nwbuf * WSLICE_B;
  return p.lds_bytes <= budget && swizzle_ok(Ko8, g.cols);
}

// Persistent kernel: the union region + 32 KiB W double buffer within
// 80 KiB (two blocks per CU).  Full four-class fusion is preferred; where
// its region is too large the tile is split by row parity (two classes per
// staging).
static DgradDirectPlan plan_persistent(int H, int W, int C8, int Ko8,
                                       long ldw, int R, int S, int stride,
                                       int pad) {
  if (!eligible_persistent(H, W, C8, Ko8, ldw, R, S, stride, pad)) return {};
  for (int bm : {128, 64}) {
    if (!tile_fits(H / 2, W / 2, bm)) continue;
    for (int qsplit : {0, 1}) {
      DgradDirectPlan p{2, bm, qsplit, 0};
      if (plan_lds(p, H, W, Ko8, R, S, pad, 1, 2, P_LDS_PLAN)) return p;
    }
  }
  return {};
}

// Wide kernel: the persistent kernel's conditions; the 8x8 class grid, so
// that a tile is the class grids of two images; and the tile's full-union
// regions + three W buffers within the LDS of one CU.  Does not depend on
// the batch: an odd image count ends in a half tile.
static DgradDirectPlan plan_wide(int H, int W, int C8, int Ko8, long ldw,
                                 int R, int S, int stride, int pad) {
  if (!eligible_persistent(H, W, C8, Ko8, ldw, R, S, stride, pad)) return {};
  // the square 8x8 class grid only: the other grids of 64 pixels are
  // neither in the models nor tested
  if (H != 16 || W != 16) return {};
  DgradDirectPlan p{2, W_BM, 0, 0, 1};
  if (plan_lds(p, H, W, Ko8, R, S, pad, W_BM / 64, W_NBUF, W_LDS_MAX))
    return p;
  return {};
}

// One-shot kernel.  Capped at 2 blocks/CU (160 KiB LDS): 1-block/CU shapes
// measured slower than their dcol path (stage latency unhidden).
static DgradDirectPlan plan_oneshot(int H, int W, int C8, int Ko8, long ldw,
                                    int R, int S, int stride, int pad) {
  if (!eligible(H, W, C8, Ko8, ldw, R, S, stride)) return {};
  for (int bm : {128, 64}) {
    if (!tile_fits(H / 2, W / 2, bm)) continue;
    DgradDirectPlan p{1, bm, 0, 0};
    if (plan_lds(p, H, W, Ko8, R, S, pad, 1, 2, P_LDS_PLAN)) return p;
  }
  return {};
}

static int device_cus() {
  static int ncu = 0;
  if (ncu == 0) {
    int dev = 0, v = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess || v <= 0)
      v = 256;
    ncu = v;
  }
  return ncu;
}

// Grid of a persistent kernel: blocks_per_cu blocks on every CU (queried
// once), capped by the tile count and by GDLJ_DGRAD_PERSIST_BLOCKS (re-read
// per call; lets small problems make one block walk several tiles).
static long persistent_blocks(long ntiles, int blocks_per_cu) {
  long nblk = std::min<long>(ntiles, (long)device_cus() * blocks_per_cu);
  if (const char* e = getenv("GDLJ_DGRAD_PERSIST_BLOCKS")) {
    long cap = atol(e);
    if (cap > 0) nblk = std::min(nblk, cap);
  }
  return nblk;
}

// the kernels' leading pointer parameters
#define CDD_PTR_ARGS(a)                                                     \
  (const unsigned short*)a.dy, (const unsigned short*)a.Wt,                 \
      (unsigned short*)a.dx, (const unsigned short*)a.y0, a.part,           \
      a.bias_fwd, a.stats_part, (const unsigned short*)a.zp

static void launch_persistent(const DgradDirectArgs& a, DgradDirectPlan plan,
                              hipStream_t s) {
  const int lds_b = plan.lds_bytes, qsplit = plan.qsplit;
  const int Hc = a.H / 2, Wc = a.W / 2;
  const Region g = plan_region(plan, a.H, a.W, a.R, a.S, a.pad);
  set_attrs_once();
  long ntiles = (long)a.Nb * Hc * Wc / plan.bm * (qsplit ? 2 : 1);
  long nblk = persistent_blocks(ntiles, 2);
  if (nblk <= 0) return;
  const int mi = plan.bm / 64, nct = a.C8 / 64;
  const bool pact = a.y0 != nullptr;
#define CDD_LAUNCH_P(MI_, NCT_, PACT_)                                      \
  if (mi == MI_ && nct == NCT_ && pact == PACT_) {                          \
    hipLaunchKernelGGL((conv_dgrad_direct_p<MI_, NCT_, PACT_>),             \
                       dim3((unsigned)nblk), dim3(256), lds_b, s,           \
                       CDD_PTR_ARGS(a), a.H, a.W, a.C8, a.Ho, a.Wo, a.Ko8,  \
                       a.ldw, a.R, a.S, a.pad, a.act, a.slope, Hc, Wc,      \
                       g.rows, g.cols, make_fastdiv(Wc), (int)ntiles,       \
                       qsplit);                                             \
    return;                                                                 \
  }
  CDD_INSTANCES(CDD_NONE, CDD_LAUNCH_P, CDD_NONE)
#undef CDD_LAUNCH_P
  no_instance("conv_dgrad_direct_p", mi, nct);
}

// one block of 512 threads per CU
static void launch_wide(const DgradDirectArgs& a, DgradDirectPlan plan,
                        hipStream_t s) {
  const int lds_b = plan.lds_bytes;
  const int Hc = a.H / 2, Wc = a.W / 2;
  const int imgs = plan.bm / (Hc * Wc);
  const Region g = plan_region(plan, a.H, a.W, a.R, a.S, a.pad);
  set_attrs_once();
  long ntiles = ((long)a.Nb + imgs - 1) / imgs;
  long nblk = persistent_blocks(ntiles, 1);
  if (nblk <= 0) return;
  const int nct = a.C8 / 64;
  const bool pact = a.y0 != nullptr;
#define CDD_LAUNCH_W(NCT_, PACT_)                                           \
  if (nct == NCT_ && pact == PACT_) {                                       \
    hipLaunchKernelGGL((conv_dgrad_direct_w<NCT_, PACT_>),                  \
                       dim3((unsigned)nblk), dim3(W_THREADS), lds_b, s,     \
                       CDD_PTR_ARGS(a), a.Nb, a.H, a.W, a.C8, a.Ho, a.Wo,   \
                       a.Ko8, a.ldw, a.R, a.S, a.pad, a.act, a.slope, Hc,   \
                       Wc, g.rows, g.cols, make_fastdiv(Wc), (int)ntiles);  \
    return;                                                                 \
  }
  CDD_INSTANCES(CDD_NONE, CDD_NONE, CDD_LAUNCH_W)
#undef CDD_LAUNCH_W
  no_instance("conv_dgrad_direct_w", 2, nct);
}

static void launch_oneshot(const DgradDirectArgs& a, DgradDirectPlan plan,
                           hipStream_t s) {
  const int lds_b = plan.lds_bytes;
  const int Hc = a.H / 2, Wc = a.W / 2;
  const Region g = plan_region(plan, a.H, a.W, a.R, a.S, a.pad);
  set_attrs_once();
  dim3 grid((long)a.Nb * Hc * Wc / plan.bm, a.C8 / 64, 4);
  const int mi = plan.bm / 64;
#define CDD_LAUNCH_O(MI_)                                                   \
  if (mi == MI_) {                                                          \
    hipLaunchKernelGGL((conv_dgrad_direct<MI_>), grid, dim3(256), lds_b, s, \
                       CDD_PTR_ARGS(a), a.Nb, a.H, a.W, a.C8, a.Ho, a.Wo,   \
                       a.Ko8, a.ldw, a.R, a.S, a.pad, a.act, a.slope, Hc,   \
                       Wc, g.rows, g.cols, make_fastdiv(Wc));               \
    return;                                                                 \
  }
  CDD_INSTANCES(CDD_LAUNCH_O, CDD_NONE, CDD_NONE)
#undef CDD_LAUNCH_O
  no_instance("conv_dgrad_direct", mi, 0);
}
#undef CDD_PTR_ARGS
}  // namespace cdd

extern "C" {

// GDLJ_DGRAD_PERSIST=0 routes the direct dgrad / convT forward to the
// one-shot kernel instead of the persistent class-fused one (re-read
// per call, like the other gates).
// GDLJ_DGRAD_WIDE=0 sends the geometries of the wide kernel back to the
// two-blocks-per-CU persistent kernel (or, where that one does not take
// them, to the caller's fallback).  The result is the plan's allow mask:
// kDgradAllowPersist | kDgradAllowWide, or 0 for the one-shot kernel, each
// with kDgradAllowClassGemm or without.
int conv_dgrad_direct_allow() {
  auto off = [](const char* name) {
    const char* e = getenv(name);
    return e != nullptr && e[0] == '0' && e[1] == '\0';
  };
  // GDLJ_DGRAD_CLASSGEMM=0 leaves what no direct kernel takes to the caller's
  // fallback (dcol + col2im); it does not depend on the other two gates.
  // GDLJ_DGRAD_CLASSGEMM_FP32=1: one fp32 accumulation over all taps on the
  // 256-wide tile (faster and more accurate, but not the bits of dcol +
  // col2im, which the default reproduces)
  const char* f32 = getenv("GDLJ_DGRAD_CLASSGEMM_FP32");
  const int cls = off("GDLJ_DGRAD_CLASSGEMM") ? 0
                  : kDgradAllowClassGemm |
                        (f32 != nullptr && f32[0] == '1' ? kDgradClassFp32 : 0);
  if (off("GDLJ_DGRAD_PERSIST")) return cls;
  return cls | (off("GDLJ_DGRAD_WIDE")
                    ? kDgradAllowPersist
                    : kDgradAllowPersist | kDgradAllowWide);
}

DgradDirectPlan conv_dgrad_direct_plan(int Nb, int H, int W, int C8, int Ko8,
                                       long ldw, int R, int S, int stride,
                                       int pad, int allow) {
  if ((allow & kDgradAllowPersist) && (allow & kDgradAllowWide)) {
    DgradDirectPlan p = cdd::plan_wide(H, W, C8, Ko8, ldw, R, S, stride, pad);
    if (p.kind != 0) return p;
  }
  if (allow & kDgradAllowPersist) {
    DgradDirectPlan p =
        cdd::plan_persistent(H, W, C8, Ko8, ldw, R, S, stride, pad);
    if (p.kind != 0) return p;
  }
  DgradDirectPlan p = cdd::plan_oneshot(H, W, C8, Ko8, ldw, R, S, stride, pad);
  if (p.kind != 0) return p;
  // last resort: one gathered 8-phase GEMM per parity class (gemm8p.hip)
  if ((allow & kDgradAllowClassGemm) &&
      conv_dgrad_classgemm_eligible(Nb, H, W, C8, Ko8, ldw, R, S, stride, pad))
    return DgradDirectPlan{(allow & kDgradClassFp32) ? 4 : 3, 0, 0, 0, 0};
  return {};
}

void launch_conv_dgrad_direct(const DgradDirectArgs& a, DgradDirectPlan plan,
                              hipStream_t s) {
  if (plan.kind == 2 && plan.wide) cdd::launch_wide(a, plan, s);
  else if (plan.kind == 2) cdd::launch_persistent(a, plan, s);
  else if (plan.kind == 1) cdd::launch_oneshot(a, plan, s);
  else if (plan.kind >= 3)
    launch_conv_dgrad_classgemm(a, plan.kind == 4, s);
}

}  // extern "C"
