// Building blocks of the three direct dgrad / convT kernels of
// conv_dgrad_direct.hip (one-shot, persistent, wide).  Each piece of the
// arithmetic exists once, here: the kernels differ in their pipelines (waits,
// barriers, prefetch distance, tile walk), which stay spelled out in them.
// That per output element the accumulation sequence (tap, 128-co chunk, kc,
// one MFMA chain) and the epilogue expressions are the same in all three,
// hence dx / y bit-identical, follows from slice_mfma, write_ctile and
// epilogue_piece being the same code (the one-shot kernel keeps a copy of
// the last two for speed; the golden digests hold it to them).
//
//   p_tap0 / p_ntap / p_boff / p_lo   per-axis parity-class geometry (host
//                                     and device); p_axis_extent on the host
//   stage_region                      dy region -> LDS, swizzled, zero halo
//   class_px                          tile row -> (image, class row, class col)
//   w_slice_src                       W source of a slice of (class, c-tile)
//   slice_mfma                        fragment addressing + ds_read + MFMA
//   write_ctile                       acc -> bf16 ctile (+ bias + act forward)
//   epilogue_piece                    ctile row -> act backward, partials, store
//   reduce_and_add / flush_partials   LDS tree + atomics of the partials
#pragma once

#include <algorithm>

#include "common.h"

namespace cdd {
constexpr int WSLICE_B = 16 * 1024;      // one [64c][128co] slice (2 subs);
                                         // >= the bytes of a ctile

#define CDD_HD __host__ __device__ __forceinline__

// ---- per-axis parity-class geometry.  Output parity q of an axis takes
// the taps r = tap0 + 2*k, k < ntap; class pixel h reads dy rows
// h + boff - k, i.e. the window [h + lo, h + boff].
CDD_HD int p_tap0(int q, int pad) { return (q + pad) & 1; }
CDD_HD int p_ntap(int q, int pad, int R) {
  return (R - p_tap0(q, pad) + 1) >> 1;
}
CDD_HD int p_boff(int q, int pad) { return (q + pad - p_tap0(q, pad)) >> 1; }
CDD_HD int p_lo(int q, int pad, int R) {
  return p_boff(q, pad) - (p_ntap(q, pad, R) - 1);
}
// first dy offset of the union window over both parities
CDD_HD int p_union_lo(int pad, int R) {
  int a = p_lo(0, pad, R), b = p_lo(1, pad, R);
  return a < b ? a : b;
}
// Region extent along one axis for `len` class pixels: the union of both
// parities, or (qsplit) the larger single-parity window, ntap - 1 wide.
inline int p_axis_extent(int len, int pad, int R, bool qsplit) {
  if (qsplit)
    return len + std::max(p_ntap(0, pad, R), p_ntap(1, pad, R)) - 1;
  return len + std::max(p_boff(0, pad), p_boff(1, pad)) - p_union_lo(pad, R);
}

// Workgroup barrier for LDS traffic only.  __syncthreads() carries a
// release fence that drains vmcnt to 0, i.e. waits for the prefetched
// W slice / region at every barrier and serializes the pipeline
// (same finding as gemm8p.hip).  This one completes the wave's own LDS
// reads/writes and leaves the LDS-DMA loads in flight; their arrival
// is guarded by the counted vmcnt waits.
DEV_INLINE void p_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// ---- region stager: [imgs][rgn_rows][rgn_cols][Ko8] of images n0.. into
// LDS, region row 0 = dy row h0, column 0 = dy column lo_w.  Cells outside
// the image, and whole images at or past n_end, come from the zero page.
// Source-side chunk swizzle (slot = j ^ (cc & mask)): without it the
// A-fragment reads of 16 consecutive-cc pixels land 256B apart = same LDS
// bank (16-way conflict); the xor spreads them 8-wide.  It is a permutation
// of the cell's chunks under swizzle_ok (below).  POW2 = Ko8 is a power of
// two: shift/mask cell decode, no division by co_chunks.
template <int THREADS, bool POW2>
DEV_INLINE void stage_region(const unsigned short* __restrict__ dy,
                             const unsigned short* __restrict__ zp,
                             char* rgn, int n0, int imgs, int n_end, int h0,
                             int lo_w, int rgn_rows, int rgn_cols, int Ho,
                             int Wo, int Ko8) {
  const int co_chunks = Ko8 >> 3;
  const int cmask = co_chunks - 1;
  const int csh = 31 - __builtin_clz(co_chunks);
  const int cpi = rgn_rows * rgn_cols;          // region cells per image
  const int ncell = imgs * cpi * co_chunks;
  for (int cell = threadIdx.x; cell < ncell; cell += THREADS) {
    int rc_ = POW2 ? cell >> csh : cell / co_chunks;
    int slot = POW2 ? cell & cmask : cell - rc_ * co_chunks;
    int img = imgs > 1 && rc_ >= cpi ? 1 : 0;   // at most two images
    int rci = rc_ - img * cpi;
    int rr = rci / rgn_cols;
    int cc = rci - rr * rgn_cols;
    int j = slot ^ (cc & cmask);
    int hig = h0 + rr;
    int wig = lo_w + cc;
    int n = n0 + img;
    const unsigned short* src = zp;
    if (n < n_end && hig >= 0 && hig < Ho && wig >= 0 && wig < Wo)
      src = dy + (((long)n * Ho + hig) * Wo + wig) * Ko8 + j * 8;
    char* dst = rgn + (cell & ~63) * 16;
    GLDS16(src, dst);
  }
}

// ---- tile row -> class pixel.  A tile is `imgs` images' worth of rows,
// hwc class pixels each (imgs == 1: a part of one image's class grid).
struct ClassPx { int img, h, w; };
DEV_INLINE ClassPx class_px(int row, int imgs, int hwc, FastDiv fWc, int Wc) {
  ClassPx p;
  p.img = imgs > 1 && row >= hwc ? 1 : 0;
  int rem = row - p.img * hwc;
  p.h = (int)fdiv((unsigned)rem, fWc);          // class row within the tile
  p.w = rem - p.h * Wc;                         // class col (full width)
  return p;
}

// this lane's A-side class pixels: tile rows row0 + mi*16 + (lane & 15);
// a = byte offset of the pixel's image region (img_b each)
template <int MI>
struct LanePx { int a[MI], h[MI], w[MI]; };
template <int MI>
DEV_INLINE LanePx<MI> lane_px(int row0, int imgs, int hwc, int img_b,
                              FastDiv fWc, int Wc) {
  LanePx<MI> px;
  #pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    ClassPx p = class_px(row0 + mi * 16 + (threadIdx.x & 15), imgs, hwc, fWc,
                         Wc);
    px.a[mi] = p.img * img_b;
    px.h[mi] = p.h;
    px.w[mi] = p.w;
  }
  return px;
}

// ---- W source of slice (tap row rc, tap column sc, 128-co chunk j) of
// parity class cls, 64-channel c-tile ct
DEV_INLINE const unsigned short* w_slice_src(
    const unsigned short* __restrict__ Wt, long ldw, int C8, int S, int pad,
    int cls, int ct, int rc, int sc, int j) {
  int tap = (p_tap0(cls >> 1, pad) + 2 * rc) * S + p_tap0(cls & 1, pad) +
            2 * sc;
  return Wt + ((long)tap * C8 + ct * 64) * ldw + j * 128;
}

// fragment of a 64-row x 64-k staged W sub-tile (swizzled tn layout,
// conv_gather.h tn_stage_rows / gemm.hip tn_frag geometry)
DEV_INLINE bf16x8 cdd_wfrag(const char* lds, int row, int kslot) {
  int byte = row * 128 + ((kslot ^ (row & 7)) * 16);
  return *(const bf16x8*)(lds + byte);
}

// ---- one W slice against the region: acc[mi][ni] += A(px, co) * W(c, co)
// over the slice's 128 co, four kc steps of 16x16x32.  The lane's pixels
// read region cell (px.h + dr, px.w + dc), always in-grid (halo cells are
// zero); Wl is the slice's LDS image, wrow the wave's first channel row in
// it.  FETCH_AHEAD fetches all fragments of the slice ahead of its MFMAs:
// fetched per kc, every kc step exposes an LDS round trip that two waves
// per SIMD (the wide kernel) cannot cover.  No waits, barriers or loads
// from global memory in here.
template <int MI, int NI, bool FETCH_AHEAD>
DEV_INLINE void slice_mfma(f32x4 (&acc)[MI][NI], const char* rgn,
                           const char* Wl, const LanePx<MI>& px, int dr,
                           int dc, int rgn_cols, int Ko8, int j, int wrow) {
  const int fr = threadIdx.x & 15, fq = (threadIdx.x & 63) >> 4;
  const int cmask = (Ko8 >> 3) - 1;
  int abase[MI];
  int axor[MI];
  #pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    int rr = px.h[mi] + dr;
    int cc = px.w[mi] + dc;
    abase[mi] = px.a[mi] + (rr * rgn_cols + cc) * Ko8 * 2;
    axor[mi] = cc & cmask;
  }
  constexpr int KF = FETCH_AHEAD ? 4 : 1;       // kc steps fetched at once
  #pragma unroll
  for (int k0 = 0; k0 < 4; k0 += KF) {
    bf16x8 a[KF][MI], b[KF][NI];
    #pragma unroll
    for (int kf = 0; kf < KF; ++kf) {
      int kc = k0 + kf;
      int jc = j * 16 + kc * 4 + fq;            // 16B co-chunk within Ko8
      #pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        a[kf][mi] = *(const bf16x8*)(rgn + abase[mi] +
                                     ((jc ^ axor[mi]) << 4));
      int sub = kc >> 1, kslot = (kc & 1) * 4 + fq;
      #pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        b[kf][ni] = cdd_wfrag(Wl + sub * 8 * 1024, wrow + ni * 16 + fr,
                              kslot);
    }
    // keep the scheduler from sinking the reads back to their uses
    if constexpr (FETCH_AHEAD) __builtin_amdgcn_sched_barrier(0);
    #pragma unroll
    for (int kf = 0; kf < KF; ++kf)
      #pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        #pragma unroll
        for (int ni = 0; ni < NI; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[kf][mi], b[kf][ni], acc[mi][ni], 0, 0, 0);
  }
}

template <int MI, int NI>
DEV_INLINE void zero_acc(f32x4 (&acc)[MI][NI]) {
  #pragma unroll
  for (int i = 0; i < MI; ++i)
    #pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
}

// ---- acc -> bf16 ctile [BM][64]: the wave's MI*16 rows from row0, NI*16
// columns from col0.  fwd (convT forward) applies bias (bv: this lane's
// column of each ni) + activation here; dgrad applies the producer's act'
// in epilogue_piece.
template <int MI, int NI>
DEV_INLINE void write_ctile(unsigned short* ctile, const f32x4 (&acc)[MI][NI],
                            const float (&bv)[NI], bool fwd, int act,
                            float slope, int row0, int col0) {
  const int fr = threadIdx.x & 15, fq = (threadIdx.x & 63) >> 4;
  #pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    #pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      int lc = col0 + ni * 16 + fr;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        int lr = row0 + mi * 16 + fq * 4 + r;
        float v = acc[mi][ni][r];
        if (fwd) v = act_fwd(v + bv[ni], act, slope);
        ctile[lr * 64 + lc] = f2bf(v);
      }
    }
  }
}

// register partials of one thread: 8 channels at seg = threadIdx.x & 7 of
// each of the block's NCT c-tiles
template <int NCT>
struct Partials {
  float bsum[NCT][8], ssum[NCT][8], ssq[NCT][8];
  DEV_INLINE void clear() {
    #pragma unroll
    for (int k = 0; k < NCT; ++k)
      #pragma unroll
      for (int jj = 0; jj < 8; ++jj)
        bsum[k][jj] = ssum[k][jj] = ssq[k][jj] = 0.f;
  }
};

// ---- one epilogue piece: 8 channels of a ctile row.  pact: times the
// producer's act' from its output yv, rounded to bf16, summed into the bias
// partial; stats: BN sum / sum of squares of the bf16 values; then the 16 B
// store.  The partials of c-tile ct are selected by predicate so that they
// stay in registers.
template <int NCT>
DEV_INLINE void epilogue_piece(const unsigned short* crow,
                               unsigned short* out, bool pact, s16x8 yv,
                               bool stats, int ct, int act, float slope,
                               Partials<NCT>& p) {
  s16x8 v = *(const s16x8*)crow;
  if (pact) {
    #pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      float d = bf2f((unsigned short)v[jj]) *
                act_bwd_from_y(bf2f((unsigned short)yv[jj]), act, slope);
      v[jj] = (short)f2bf(d);
      #pragma unroll
      for (int k = 0; k < NCT; ++k)
        if (ct == k) p.bsum[k][jj] += d;
    }
  }
  if (stats) {
    #pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      float y = bf2f((unsigned short)v[jj]);
      #pragma unroll
      for (int k = 0; k < NCT; ++k)
        if (ct == k) {
          p.ssum[k][jj] += y;
          p.ssq[k][jj] += y * y;
        }
    }
  }
  *(s16x8*)out = v;
}

// ---- block-level seg reduction in LDS before the global atomics: naive
// per-lane atomics (2048 lane-ops per block, 32-way duplicate addresses)
// serialized across ALL concurrent blocks and cost ~12 ms/call at the
// DCGAN-64 conv2 shape.  ROWS = threads / 8 contributor rows per seg; red
// holds ROWS * 64 floats.  Block-uniform call sites only (barriers).
template <int ROWS>
DEV_INLINE void reduce_and_add(float* red, const float (&vec)[8],
                               float* dst) {
  const int seg = threadIdx.x & 7, rrow = threadIdx.x >> 3;
  #pragma unroll
  for (int jj = 0; jj < 8; ++jj) red[(rrow * 8 + seg) * 8 + jj] = vec[jj];
  __syncthreads();
  for (int off = ROWS / 2; off > 0; off >>= 1) {
    if (rrow < off) {
      #pragma unroll
      for (int jj = 0; jj < 8; ++jj)
        red[(rrow * 8 + seg) * 8 + jj] +=
            red[((rrow + off) * 8 + seg) * 8 + jj];
    }
    __syncthreads();
  }
  if (rrow == 0) {
    #pragma unroll
    for (int jj = 0; jj < 8; ++jj)
      atomicAdd(&dst[seg * 8 + jj], red[seg * 8 + jj]);
  }
  __syncthreads();  // red is reused by the next reduction
}

// Blocks add their partials into row blockIdx.x & (kPartRows - 1) of the
// bindings' [kPartRows][...] buffers (the one-shot grid can exceed kPartRows).
static_assert((kPartRows & (kPartRows - 1)) == 0,
              "kPartRows must be a power of two");

// all partials of the block: c-tile k covers channels c0 + k*64 ..
template <int ROWS, int NCT>
DEV_INLINE void flush_partials(float* red, const Partials<NCT>& p,
                               float* part, float* stats_part, int C8,
                               int c0) {
  const long prow = blockIdx.x & (kPartRows - 1);
  #pragma unroll
  for (int k = 0; k < NCT; ++k) {
    if (part != nullptr)
      reduce_and_add<ROWS>(red, p.bsum[k], part + prow * C8 + c0 + k * 64);
    if (stats_part != nullptr) {
      float* srow = stats_part + prow * 2 * C8;
      reduce_and_add<ROWS>(red, p.ssum[k], srow + c0 + k * 64);
      reduce_and_add<ROWS>(red, p.ssq[k], srow + C8 + c0 + k * 64);
    }
  }
}

#undef CDD_HD
}  // namespace cdd
