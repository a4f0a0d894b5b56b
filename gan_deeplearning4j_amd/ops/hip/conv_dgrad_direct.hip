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
// conv_dgrad_direct_p (below) is the persistent class-fused variant of
// the same arithmetic; the launchers try it first and keep this kernel
// as the fallback and A/B arm (GDLJ_DGRAD_PERSIST=0).
// conv_dgrad_direct_w (further below) is its one-block-per-CU variant for
// the 8x8 class grid, tried before it (GDLJ_DGRAD_WIDE=0 skips it).

#include <algorithm>
#include <cstdlib>

#include "common.h"

namespace cdd {
constexpr int BN = 64;
constexpr int WSLICE_B = 16 * 1024;      // one [64c][128co] slice (2 subs)
constexpr int WBUF_B = 2 * WSLICE_B;     // double buffer; >= ctile bytes
}  // namespace cdd

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

DEV_INLINE bf16x8 cdd_wfrag(const char* lds, int row, int kslot) {
  int byte = row * 128 + ((kslot ^ (row & 7)) * 16);
  return *(const bf16x8*)(lds + byte);
}

// Blocks add their partials into row blockIdx.x & (kPartRows - 1) of the
// bindings' [kPartRows][...] buffers (the one-shot grid can exceed kPartRows).
static_assert((kPartRows & (kPartRows - 1)) == 0,
              "kPartRows must be a power of two");

// MI = pixel fragments per wave (BM = MI * 64).
//
// The same kernel serves the strided TRANSPOSED-conv forward (G side):
// y[ho,wo,co] = sum over parity-valid taps of x[(ho+p-r)/2][ci] *
// W[ci,co,r,s] is the identical gather; pass x as `dy`, the
// [R*S*Co8][Cin] "w2a" pack as `Wt`, bias_fwd + act for the fused
// epilogue, and stats_part ([kPartRows][2*C8]) for fused BN statistics.
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
    int Hc, int Wc, int rows_c, int rgn_rows, int rgn_cols,
    FastDiv fWc) {
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
  const int qh = blockIdx.z >> 1;  // parity class
  const int qw = blockIdx.z & 1;

  // class tap set: r = r0 + 2*rc (rc < Rc), s = s0 + 2*sc (sc < Sc)
  const int r0 = (qh + pad) & 1;
  const int s0 = (qw + pad) & 1;
  const int Rc = (R - r0 + 1) >> 1;
  const int Sc = (S - s0 + 1) >> 1;
  const int rb0 = (qh + pad - r0) >> 1;   // dy row offset of tap rc=0
  const int wb0 = (qw + pad - s0) >> 1;
  const int lo_h = hc0 + rb0 - (Rc - 1);  // dy row of region row 0
  const int lo_w = wb0 - (Sc - 1);        // dy col of region col 0

  // ---- stage the dy region: [rgn_rows][rgn_cols][Ko8], zero halo ----
  // Source-side chunk swizzle (slot = j ^ (cc & mask)): without it the
  // A-fragment reads of 16 consecutive-cc pixels land 256B apart =
  // same LDS bank (16-way conflict); the xor spreads them 8-wide.
  const int co_chunks = Ko8 >> 3;
  const int cmask = co_chunks - 1;
  const int ncell = rgn_rows * rgn_cols * co_chunks;
  for (int cell = threadIdx.x; cell < ncell; cell += 256) {
    int rc_ = cell / co_chunks;
    int slot = cell - rc_ * co_chunks;
    int rr = rc_ / rgn_cols;
    int cc = rc_ - rr * rgn_cols;
    int j = slot ^ (cc & cmask);
    int hig = lo_h + rr;
    int wig = lo_w + cc;
    const unsigned short* src = zp;
    if (hig >= 0 && hig < Ho && wig >= 0 && wig < Wo)
      src = dy + (((long)n * Ho + hig) * Wo + wig) * Ko8 + j * 8;
    char* dst = rgn + (cell & ~63) * 16;
    GLDS16(src, dst);
  }

  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int fr = lane & 15, fq = lane >> 4;

  // this lane's A-side class pixels: px_l = wid*(MI*16) + mi*16 + fr
  int pxh[MI], pxw[MI];
  #pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    int pxl = wid * (MI * 16) + mi * 16 + fr;
    int hl = (int)fdiv((unsigned)pxl, fWc);
    pxh[mi] = hl;                    // class-row within tile
    pxw[mi] = pxl - hl * Wc;         // class-col (global: full width)
  }

  const int nj = Ko8 >> 7;           // 128-co chunks per tap
  const int nslice = Rc * Sc * nj;
  const unsigned short* wt_cy = Wt + (long)cy * 64 * ldw;
  auto wsrc_for = [&](int sl) {
    int tapj = sl / nj, j = sl - tapj * nj;
    int rc_ = tapj / Sc, sc_ = tapj - rc_ * Sc;
    int tap = (r0 + 2 * rc_) * S + (s0 + 2 * sc_);
    return wt_cy + (long)tap * C8 * ldw + j * 128;
  };

  // first W slice, then one wait covers region + slice 0
  cdd_stage_w64(wsrc_for(0), ldw, 0, wbuf(0));
  cdd_stage_w64(wsrc_for(0), ldw, 64, wbuf(0) + 8 * 1024);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  f32x4 acc[MI][4];
  #pragma unroll
  for (int i = 0; i < MI; ++i)
    #pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

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
    // region coordinates for this tap: rr = pxh + (Rc-1) - rc,
    // cc = pxw + (Sc-1) - sc  (always in-grid; halo cells are zero)
    long abase[MI];
    int axor[MI];
    #pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      int rr = pxh[mi] + (Rc - 1) - rc_;
      int cc = pxw[mi] + (Sc - 1) - sc_;
      abase[mi] = ((long)rr * rgn_cols + cc) * Ko8 * 2;
      axor[mi] = cc & cmask;
    }
    const char* Wl = wbuf(cur);
    #pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      int jc = j * 16 + kc * 4 + fq;       // 16B co-chunk within Ko8
      bf16x8 a[MI], b[4];
      #pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        a[mi] = *(const bf16x8*)(rgn + abase[mi] +
                                 ((jc ^ axor[mi]) << 4));
      int sub = kc >> 1, kslot = (kc & 1) * 4 + fq;
      #pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        b[ni] = cdd_wfrag(Wl + sub * 8 * 1024, ni * 16 + fr, kslot);
      #pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
    __syncthreads();  // all waves done with wbuf(cur) before restage
  }

  // ---- epilogue: ctile in the W-buffer area; dgrad mode applies the
  // producer act' downstream, convT-fwd mode applies bias+act here ----
  unsigned short* ctile = (unsigned short*)wbuf(0);  // [BM][64]
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
  float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float ssum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float ssq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
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
        bsum[jj] += d;
      }
    }
    if (stats_part != nullptr) {
      #pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        float yv = bf2f((unsigned short)v[jj]);
        ssum[jj] += yv;
        ssq[jj] += yv * yv;
      }
    }
    *(s16x8*)(dx + addr) = v;
  }
  // Block-level seg reductions in LDS before the global atomics: naive
  // per-lane atomics (2048 lane-ops per block, 32-way duplicate
  // addresses) serialized across ALL concurrent blocks and cost
  // ~12 ms/call at the DCGAN-64 conv2 shape.  All conditions are
  // block-uniform, so the inner barriers are safe.
  float* red = (float*)rgn;  // region is dead after the MFMA loop
  const int rrow = t2 >> 3;  // 32 contributor rows per seg
  auto reduce_and_add = [&](const float* vec, float* dst) {
    #pragma unroll
    for (int jj = 0; jj < 8; ++jj)
      red[(rrow * 8 + seg) * 8 + jj] = vec[jj];
    __syncthreads();
    for (int off = 16; off > 0; off >>= 1) {
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
  };
  if (y0 != nullptr && part != nullptr)
    reduce_and_add(
        bsum, part + (long)(blockIdx.x & (kPartRows - 1)) * C8 + cy * 64);
  if (stats_part != nullptr) {
    float* srow =
        stats_part + (long)(blockIdx.x & (kPartRows - 1)) * 2 * C8;
    reduce_and_add(ssum, srow + cy * 64);
    reduce_and_add(ssq, srow + C8 + cy * 64);
  }
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
// Bias / BN-statistics partials stay in registers across all tiles and
// go through the LDS tree + atomics once per block.  Per output element
// the accumulation sequence (taps, 128-co chunk, kc) and the epilogue
// expressions are those of conv_dgrad_direct, so dx / y are
// bit-identical; only the order of the fp32 partial sums differs.
namespace cdd {
// per-axis parity-class geometry: first tap, tap count, dy offset of
// tap 0 (class pixel h reads dy rows h + boff - k, k < ntap)
DEV_INLINE int p_tap0(int q, int pad) { return (q + pad) & 1; }
DEV_INLINE int p_ntap(int q, int pad, int R) {
  return (R - p_tap0(q, pad) + 1) >> 1;
}
DEV_INLINE int p_boff(int q, int pad) {
  return (q + pad - p_tap0(q, pad)) >> 1;
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
}  // namespace cdd

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
  const int tpi = (Hc * Wc) / BM;          // pixel tiles per image
  const int co_chunks = Ko8 >> 3;          // power of two (launcher)
  const int cmask = co_chunks - 1;
  const int csh = 31 - __builtin_clz(co_chunks);
  const int ncell = rgn_rows * rgn_cols * co_chunks;
  const int nj = Ko8 >> 7;                 // 128-co chunks per tap

  // union column window over both column parities
  const int lo_w = min(p_boff(0, pad) - (p_ntap(0, pad, S) - 1),
                       p_boff(1, pad) - (p_ntap(1, pad, S) - 1));
  // union row window: both row parities, or the tile's own one (qsplit)
  auto row_lo = [&](int tile) {
    int a = p_boff(0, pad) - (p_ntap(0, pad, R) - 1);
    int b = p_boff(1, pad) - (p_ntap(1, pad, R) - 1);
    return qsplit ? ((tile & 1) ? b : a) : min(a, b);
  };

  // ---- stage a tile's region: [rgn_rows][rgn_cols][Ko8], zero halo,
  // source-side chunk swizzle slot = j ^ (cc & cmask) as above ----
  auto stage_region = [&](int tile) {
    int pt = qsplit ? (tile >> 1) : tile;
    int n = pt / tpi;
    int hc0 = (pt - n * tpi) * rows_c;
    int h0 = hc0 + row_lo(tile);
    for (int cell = threadIdx.x; cell < ncell; cell += 256) {
      int rc_ = cell >> csh;
      int slot = cell & cmask;
      int rr = rc_ / rgn_cols;
      int cc = rc_ - rr * rgn_cols;
      int j = slot ^ (cc & cmask);
      int hig = h0 + rr;
      int wig = lo_w + cc;
      const unsigned short* src = zp;
      if (hig >= 0 && hig < Ho && wig >= 0 && wig < Wo)
        src = dy + (((long)n * Ho + hig) * Wo + wig) * Ko8 + j * 8;
      char* dst = rgn + (cell & ~63) * 16;
      GLDS16(src, dst);
    }
  };

  // W source of slice sl of (class cls, c-tile ct)
  auto wsrc_for = [&](int cls, int ct, int sl) {
    int qh = cls >> 1, qw = cls & 1;
    int r0 = p_tap0(qh, pad), s0 = p_tap0(qw, pad);
    int Sc = p_ntap(qw, pad, S);
    int tapj = sl / nj, j = sl - tapj * nj;
    int rc_ = tapj / Sc, sc_ = tapj - rc_ * Sc;
    int tap = (r0 + 2 * rc_) * S + (s0 + 2 * sc_);
    return Wt + ((long)tap * C8 + ct * 64) * ldw + j * 128;
  };

  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int fr = lane & 15, fq = lane >> 4;

  // this lane's A-side class pixels: px_l = wid*(MI*16) + mi*16 + fr
  int pxh[MI], pxw[MI];
  #pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    int pxl = wid * (MI * 16) + mi * 16 + fr;
    int hl = (int)fdiv((unsigned)pxl, fWc);
    pxh[mi] = hl;
    pxw[mi] = pxl - hl * Wc;
  }

  const int t2 = threadIdx.x;
  const int seg = t2 & 7;            // fixed c-block per thread
  float bsum[NCT][8], ssum[NCT][8], ssq[NCT][8];
  #pragma unroll
  for (int k = 0; k < NCT; ++k)
    #pragma unroll
    for (int jj = 0; jj < 8; ++jj)
      bsum[k][jj] = ssum[k][jj] = ssq[k][jj] = 0.f;

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
  stage_region(tile);
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
        #pragma unroll
        for (int i = 0; i < MI; ++i)
          #pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

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
          // region coordinates for this tap (always in-grid; halo
          // cells are zero)
          long abase[MI];
          int axor[MI];
          #pragma unroll
          for (int mi = 0; mi < MI; ++mi) {
            int rr = pxh[mi] + rb0 - rc_ - lo_h;
            int cc = pxw[mi] + wb0 - sc_ - lo_w;
            abase[mi] = ((long)rr * rgn_cols + cc) * Ko8 * 2;
            axor[mi] = cc & cmask;
          }
          const char* Wl = wbuf(cur);
          #pragma unroll
          for (int kc = 0; kc < 4; ++kc) {
            int jc = j * 16 + kc * 4 + fq;   // 16B co-chunk within Ko8
            bf16x8 a[MI], b[4];
            #pragma unroll
            for (int mi = 0; mi < MI; ++mi)
              a[mi] = *(const bf16x8*)(rgn + abase[mi] +
                                       ((jc ^ axor[mi]) << 4));
            int sub = kc >> 1, kslot = (kc & 1) * 4 + fq;
            #pragma unroll
            for (int ni = 0; ni < 4; ++ni)
              b[ni] = cdd_wfrag(Wl + sub * 8 * 1024, ni * 16 + fr, kslot);
            #pragma unroll
            for (int mi = 0; mi < MI; ++mi)
              #pragma unroll
              for (int ni = 0; ni < 4; ++ni)
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    a[mi], b[ni], acc[mi][ni], 0, 0, 0);
          }
          p_lds_barrier();  // all waves done with wbuf(cur) + region
        }

        // the tile's last MFMA slice is done: the region is dead, put
        // the next tile's region in flight under this epilogue
        if (last_ct && has_next) stage_region(ntile);
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
          int hl = (int)fdiv((unsigned)row, fWc);
          int wcl = row - hl * Wc;
          int hi = qh + 2 * (hc0 + hl);
          int wi = qw + 2 * wcl;
          eaddr[i] = (((long)n * H + hi) * W + wi) * C8 + ct * 64 + seg * 8;
        }
        if constexpr (PACT) {
          #pragma unroll
          for (int i = 0; i < BM / 32; ++i)
            yin[i] = *(const s16x8*)(y0 + eaddr[i]);
        }

        // ---- epilogue: ctile = the W buffer the last slice released
        // (the in-flight prefetch targets the other one) ----
        unsigned short* ctile = (unsigned short*)wbuf((g - 1) & 1);
        #pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          #pragma unroll
          for (int ni = 0; ni < 4; ++ni) {
            int lc = ni * 16 + fr;
            float bv = 0.f;
            #pragma unroll
            for (int k = 0; k < NCT; ++k)
              if (ct == k) bv = biasv[k][ni];
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
              int lr = wid * (MI * 16) + mi * 16 + fq * 4 + r;
              float v = acc[mi][ni][r];
              if (bias_fwd != nullptr) v = act_fwd(v + bv, act, slope);
              ctile[lr * 64 + lc] = f2bf(v);
            }
          }
        }
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
          const long addr = eaddr[i];
          s16x8 v = *(const s16x8*)(ctile + row * 64 + seg * 8);
          if constexpr (PACT) {
            const s16x8 yv = yin[i];
            #pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
              float d = bf2f((unsigned short)v[jj]) *
                        act_bwd_from_y(bf2f((unsigned short)yv[jj]), act,
                                       slope);
              v[jj] = (short)f2bf(d);
              #pragma unroll
              for (int k = 0; k < NCT; ++k)
                if (ct == k) bsum[k][jj] += d;
            }
          }
          if (stats_part != nullptr) {
            #pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
              float yv = bf2f((unsigned short)v[jj]);
              #pragma unroll
              for (int k = 0; k < NCT; ++k)
                if (ct == k) {
                  ssum[k][jj] += yv;
                  ssq[k][jj] += yv * yv;
                }
            }
          }
          *(s16x8*)(dx + addr) = v;
        }
        p_lds_barrier();  // ctile reads done before it is restaged as W
      }
    }
  }

  // ---- once per block: LDS tree + atomics over the register partials
  // (region and W buffers are dead, nothing is in flight) ----
  float* red = (float*)rgn;
  const int rrow = t2 >> 3;  // 32 contributor rows per seg
  auto reduce_and_add = [&](const float* vec, float* dst) {
    #pragma unroll
    for (int jj = 0; jj < 8; ++jj)
      red[(rrow * 8 + seg) * 8 + jj] = vec[jj];
    __syncthreads();
    for (int off = 16; off > 0; off >>= 1) {
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
  };
  #pragma unroll
  for (int k = 0; k < NCT; ++k) {
    if (PACT && part != nullptr)
      reduce_and_add(
          bsum[k], part + (long)(blockIdx.x & (kPartRows - 1)) * C8 + k * 64);
    if (stats_part != nullptr) {
      float* srow =
          stats_part + (long)(blockIdx.x & (kPartRows - 1)) * 2 * C8;
      reduce_and_add(ssum[k], srow + k * 64);
      reduce_and_add(ssq[k], srow + C8 + k * 64);
    }
  }
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
// slice g, then its MFMAs, which run into the next slice's scalar work
// and wait.
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
// 5).  Per output element the accumulation sequence
// (tap, 128-co chunk, kc, one MFMA chain) and the epilogue expressions
// are those of conv_dgrad_direct_p: dx / y are bit-identical to it; the
// fp32 bias / BN partials are summed in another order.
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
  const int cpi = rgn_rows * rgn_cols;          // region cells per image
  const int rgn_img_b = cpi * Ko8 * 2;
  const int rgn_b = imgs * rgn_img_b;
  auto wbuf = [&](int i) -> char* { return lds + rgn_b + i * WSLICE_B; };

  const int co_chunks = Ko8 >> 3;     // power of two (launcher)
  const int cmask = co_chunks - 1;
  const int csh = 31 - __builtin_clz(co_chunks);
  const int ncell = imgs * cpi * co_chunks;
  const int nj = Ko8 >> 7;            // 128-co chunks per tap

  // union window over both parities, per axis
  const int lo_w = min(p_boff(0, pad) - (p_ntap(0, pad, S) - 1),
                       p_boff(1, pad) - (p_ntap(1, pad, S) - 1));
  const int lo_h = min(p_boff(0, pad) - (p_ntap(0, pad, R) - 1),
                       p_boff(1, pad) - (p_ntap(1, pad, R) - 1));

  // ---- stage a tile's regions: [imgs][rgn_rows][rgn_cols][Ko8], zero
  // halo, an image past Nb all zero; source-side chunk swizzle ----
  auto stage_region = [&](int tile) {
    const int n0 = tile * imgs;
    for (int cell = threadIdx.x; cell < ncell; cell += W_THREADS) {
      int rc_ = cell >> csh;
      int slot = cell & cmask;
      int img = rc_ >= cpi ? 1 : 0;
      int rci = rc_ - img * cpi;
      int rr = rci / rgn_cols;
      int cc = rci - rr * rgn_cols;
      int j = slot ^ (cc & cmask);
      int hig = lo_h + rr;
      int wig = lo_w + cc;
      int n = n0 + img;
      const unsigned short* src = zp;
      if (n < Nb && hig >= 0 && hig < Ho && wig >= 0 && wig < Wo)
        src = dy + (((long)n * Ho + hig) * Wo + wig) * Ko8 + j * 8;
      char* dst = rgn + (cell & ~63) * 16;
      GLDS16(src, dst);
    }
  };

  // issue cursor of the endless W stream, in the consumer's order:
  // class, c-tile, tap row, tap column, 128-co chunk (counters, no
  // divisions: the slice loop's scalar work is on the critical path)
  int i_cls = 0, i_ct = 0, i_rc = 0, i_sc = 0, i_j = 0;
  auto issue_w = [&](int buf) {
    const int qh = i_cls >> 1, qw = i_cls & 1;
    const int tap = (p_tap0(qh, pad) + 2 * i_rc) * S + p_tap0(qw, pad) +
                    2 * i_sc;
    w_stage_slice(Wt + ((long)tap * C8 + i_ct * 64) * ldw + i_j * 128, ldw,
                  wbuf(buf));
    if (++i_j == nj) {
      i_j = 0;
      if (++i_sc == p_ntap(qw, pad, S)) {
        i_sc = 0;
        if (++i_rc == p_ntap(qh, pad, R)) {
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
  const int lane = threadIdx.x & 63;
  const int fr = lane & 15, fq = lane >> 4;
  const int pg = wid / WC;            // pixel group of this wave
  const int ch = wid - pg * WC;       // channel part of this wave
  const int wrow0 = pg * (MI * 16);   // first tile row of this wave

  // this lane's A-side class pixels (a 16-pixel fragment never
  // straddles two images: hwc is a multiple of 16)
  int pxa[MI], pxh[MI], pxw[MI];
  #pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    int pxl = wrow0 + mi * 16 + fr;
    int img = pxl >= hwc ? 1 : 0;
    int rem = pxl - img * hwc;
    int hl = (int)fdiv((unsigned)rem, fWc);
    pxa[mi] = img * rgn_img_b;
    pxh[mi] = hl;
    pxw[mi] = rem - hl * Wc;
  }

  const int t2 = threadIdx.x;
  const int seg = t2 & 7;             // fixed c-block per thread
  float bsum[NCT][8], ssum[NCT][8], ssq[NCT][8];
  #pragma unroll
  for (int k = 0; k < NCT; ++k)
    #pragma unroll
    for (int jj = 0; jj < 8; ++jj)
      bsum[k][jj] = ssum[k][jj] = ssq[k][jj] = 0.f;

  // convT-forward bias of this lane's columns, loaded and consumed ahead
  // of every LDS-DMA load (see conv_dgrad_direct_p)
  float biasv[NCT][NI];
  #pragma unroll
  for (int k = 0; k < NCT; ++k)
    #pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      biasv[k][ni] = bias_fwd != nullptr
                         ? bias_fwd[k * 64 + ch * (NI * 16) + ni * 16 + fr]
                         : 0.f;
      asm volatile("" : "+v"(biasv[k][ni]));
    }

  // this thread's epilogue pieces: piece e is row (e*512 + t2) >> 3 of
  // the tile (e = image of the pair), 8 channels at seg
  int erow[ST], eimg[ST], eoff[ST];
  #pragma unroll
  for (int e = 0; e < ST; ++e) {
    int row = (e * W_THREADS + t2) >> 3;
    int img = row >= hwc ? 1 : 0;
    int rem = row - img * hwc;
    int hl = (int)fdiv((unsigned)rem, fWc);
    erow[e] = row;
    eimg[e] = img;
    eoff[e] = (2 * hl * W + 2 * (rem - hl * Wc)) * C8 + seg * 8;
  }

  // prologue: first region + the first two W slices; the first in-loop
  // wait covers the region and slice 0
  int tile = blockIdx.x;
  stage_region(tile);
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
        }
        if constexpr (PACT) {
          #pragma unroll
          for (int e = 0; e < ST; ++e) {
            yin[e] = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (evalid[e]) yin[e] = *(const s16x8*)(y0 + eaddr[e]);
          }
        }

        f32x4 acc[MI][NI];
        #pragma unroll
        for (int i = 0; i < MI; ++i)
          #pragma unroll
          for (int j = 0; j < NI; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

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
          // region coordinates for this tap (always in-grid; halo
          // cells are zero)
          int abase[MI];
          int axor[MI];
          #pragma unroll
          for (int mi = 0; mi < MI; ++mi) {
            int rr = pxh[mi] + rb0 - rc_ - lo_h;
            int cc = pxw[mi] + wb0 - sc_ - lo_w;
            abase[mi] = pxa[mi] + (rr * rgn_cols + cc) * Ko8 * 2;
            axor[mi] = cc & cmask;
          }
          const char* Wl = wbuf(cur);
          // all fragments of the slice are fetched ahead of its MFMAs:
          // fetched per kc, every kc step exposes an LDS round trip that
          // two waves per SIMD cannot cover
          bf16x8 a[4][MI], b[4][NI];
          #pragma unroll
          for (int kc = 0; kc < 4; ++kc) {
            int jc = j * 16 + kc * 4 + fq;   // 16B co-chunk within Ko8
            #pragma unroll
            for (int mi = 0; mi < MI; ++mi)
              a[kc][mi] = *(const bf16x8*)(rgn + abase[mi] +
                                           ((jc ^ axor[mi]) << 4));
            int sub = kc >> 1, kslot = (kc & 1) * 4 + fq;
            #pragma unroll
            for (int ni = 0; ni < NI; ++ni)
              b[kc][ni] = cdd_wfrag(Wl + sub * 8 * 1024,
                                    ch * (NI * 16) + ni * 16 + fr, kslot);
          }
          // keep the scheduler from sinking the reads back to their uses
          __builtin_amdgcn_sched_barrier(0);
          #pragma unroll
          for (int kc = 0; kc < 4; ++kc)
            #pragma unroll
            for (int mi = 0; mi < MI; ++mi)
              #pragma unroll
              for (int ni = 0; ni < NI; ++ni)
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    a[kc][mi], b[kc][ni], acc[mi][ni], 0, 0, 0);
          cur = cur == 2 ? 0 : cur + 1;
        }
        // every wave is done with the last slice's W buffer (the ctile)
        // and, on the tile's last c-tile, with the region
        p_lds_barrier();

        // the region is dead: put the next tile's region in flight under
        // this epilogue; with PACT after the y0 pieces are taken (below),
        // so that their wait does not cover it
        if constexpr (!PACT) {
          if (last_ct && has_next) stage_region(ntile);
        }
        asm volatile("" ::: "memory");

        // ---- epilogue: ctile = the W buffer the last slice released
        // (slices g+1, g+2 sit in the other two) ----
        unsigned short* ctile =
            (unsigned short*)wbuf(cur == 0 ? 2 : cur - 1);
        #pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          #pragma unroll
          for (int ni = 0; ni < NI; ++ni) {
            int lc = ch * (NI * 16) + ni * 16 + fr;
            float bv = 0.f;
            #pragma unroll
            for (int k = 0; k < NCT; ++k)
              if (ct == k) bv = biasv[k][ni];
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
              int lr = wrow0 + mi * 16 + fq * 4 + r;
              float v = acc[mi][ni][r];
              if (bias_fwd != nullptr) v = act_fwd(v + bv, act, slope);
              ctile[lr * 64 + lc] = f2bf(v);
            }
          }
        }
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
          if (last_ct && has_next) stage_region(ntile);
          asm volatile("" ::: "memory");
        }
        #pragma unroll
        for (int e = 0; e < ST; ++e) {
          if (!evalid[e]) continue;
          const long addr = eaddr[e];
          s16x8 v = *(const s16x8*)(ctile + erow[e] * 64 + seg * 8);
          if constexpr (PACT) {
            const s16x8 yv = yin[e];
            #pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
              float d = bf2f((unsigned short)v[jj]) *
                        act_bwd_from_y(bf2f((unsigned short)yv[jj]), act,
                                       slope);
              v[jj] = (short)f2bf(d);
              #pragma unroll
              for (int k = 0; k < NCT; ++k)
                if (ct == k) bsum[k][jj] += d;
            }
          }
          if (stats_part != nullptr) {
            #pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
              float yv = bf2f((unsigned short)v[jj]);
              #pragma unroll
              for (int k = 0; k < NCT; ++k)
                if (ct == k) {
                  ssum[k][jj] += yv;
                  ssq[k][jj] += yv * yv;
                }
            }
          }
          *(s16x8*)(dx + addr) = v;
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
  float* red = (float*)rgn;
  const int rrow = t2 >> 3;  // 64 contributor rows per seg
  auto reduce_and_add = [&](const float* vec, float* dst) {
    #pragma unroll
    for (int jj = 0; jj < 8; ++jj)
      red[(rrow * 8 + seg) * 8 + jj] = vec[jj];
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) {
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
  };
  #pragma unroll
  for (int k = 0; k < NCT; ++k) {
    if (PACT && part != nullptr)
      reduce_and_add(
          bsum[k], part + (long)(blockIdx.x & (kPartRows - 1)) * C8 + k * 64);
    if (stats_part != nullptr) {
      float* srow =
          stats_part + (long)(blockIdx.x & (kPartRows - 1)) * 2 * C8;
      reduce_and_add(ssum[k], srow + k * 64);
      reduce_and_add(ssq[k], srow + C8 + k * 64);
    }
  }
}

// one-time dynamic-LDS opt-in for every instantiation of the kernels
static void cdd_set_attrs_once() {
  static int attr_done = 0;
  if (attr_done) return;
  const void* fns[] = {
      reinterpret_cast<const void*>(&conv_dgrad_direct<2>),
      reinterpret_cast<const void*>(&conv_dgrad_direct<1>),
      reinterpret_cast<const void*>(&conv_dgrad_direct_p<2, 1, false>),
      reinterpret_cast<const void*>(&conv_dgrad_direct_p<2, 2, false>),
      reinterpret_cast<const void*>(&conv_dgrad_direct_p<1, 1, false>),
      reinterpret_cast<const void*>(&conv_dgrad_direct_p<1, 2, false>),
      reinterpret_cast<const void*>(&conv_dgrad_direct_p<2, 1, true>),
      reinterpret_cast<const void*>(&conv_dgrad_direct_p<2, 2, true>),
      reinterpret_cast<const void*>(&conv_dgrad_direct_p<1, 1, true>),
      reinterpret_cast<const void*>(&conv_dgrad_direct_p<1, 2, true>),
  };
  for (const void* f : fns)
    (void)hipFuncSetAttribute(
        f, hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024);
  const void* wide_fns[] = {
      reinterpret_cast<const void*>(&conv_dgrad_direct_w<1, false>),
      reinterpret_cast<const void*>(&conv_dgrad_direct_w<2, false>),
      reinterpret_cast<const void*>(&conv_dgrad_direct_w<1, true>),
      reinterpret_cast<const void*>(&conv_dgrad_direct_w<2, true>),
  };
  for (const void* f : wide_fns)
    (void)hipFuncSetAttribute(
        f, hipFuncAttributeMaxDynamicSharedMemorySize, cdd::W_LDS_MAX);
  attr_done = 1;
}

namespace cdd {
// host mirror of the per-axis class geometry
inline void p_axis_window(int pad, int R, int q, int* lo, int* hi) {
  int t0 = (q + pad) & 1;
  int nt = (R - t0 + 1) >> 1;
  int bo = (q + pad - t0) >> 1;
  *lo = bo - (nt - 1);
  *hi = bo;
}
// region extent along one axis for `len` class pixels: the union of
// both parities, or (qsplit) the larger single-parity window
inline int p_axis_extent(int len, int pad, int R, bool qsplit) {
  int l0, h0, l1, h1;
  p_axis_window(pad, R, 0, &l0, &h0);
  p_axis_window(pad, R, 1, &l1, &h1);
  if (qsplit) return len + std::max(h0 - l0, h1 - l1);
  return len + std::max(h0, h1) - std::min(l0, l1);
}

// Persistent kernel eligibility ({} is kind 0: not taken).  On top of the
// one-shot kernel's conditions: C8 <= 128 (register partials per c-tile),
// Ko8 a power of two (shift/mask cell decode), and the union region +
// 32 KiB W double buffer within 80 KiB (two blocks per CU).  Full
// four-class fusion is preferred; where its region is too large the tile
// is split by row parity (two classes per staging).
static DgradDirectPlan plan_persistent(int H, int W, int C8, int Ko8,
                                       long ldw, int R, int S, int stride,
                                       int pad) {
  if (stride != 2 || (C8 != 64 && C8 != 128) || Ko8 % 128 != 0 ||
      (Ko8 & (Ko8 - 1)) != 0 || ldw != Ko8)
    return {};
  if (R < 2 || S < 2 || R > 8 || S > 8 || (H & 1) || (W & 1)) return {};
  if (pad < 0) return {};
  int Hc = H / 2, Wc = W / 2;
  for (int bm : {128, 64}) {
    if (Wc > bm || bm % Wc != 0 || (Hc * Wc) % bm != 0) continue;
    int rows_c = bm / Wc;
    for (int qsplit : {0, 1}) {
      int rgn_rows = p_axis_extent(rows_c, pad, R, qsplit != 0);
      int rgn_cols = p_axis_extent(Wc, pad, S, false);
      int lds_b = rgn_rows * rgn_cols * Ko8 * 2 + WBUF_B;
      if (lds_b > 80 * 1024) continue;
      return DgradDirectPlan{2, bm, qsplit, lds_b};
    }
  }
  return {};
}

// Wide kernel eligibility: the persistent kernel's conditions on strides,
// channels, taps and parity; the 8x8 class grid, so that a tile is the
// class grids of two images; and the tile's full-union regions +
// three W buffers within the LDS of one CU.  Does not depend on the
// batch: an odd image count ends in a half tile.
static DgradDirectPlan plan_wide(int H, int W, int C8, int Ko8, long ldw,
                                 int R, int S, int stride, int pad) {
  if (stride != 2 || (C8 != 64 && C8 != 128) || Ko8 % 128 != 0 ||
      (Ko8 & (Ko8 - 1)) != 0 || ldw != Ko8)
    return {};
  if (R < 2 || S < 2 || R > 8 || S > 8 || (H & 1) || (W & 1)) return {};
  if (pad < 0) return {};
  int Hc = H / 2, Wc = W / 2;
  const int bm = W_BM;
  // the square 8x8 class grid only: the other grids of 64 pixels are
  // neither in the models nor tested
  if (Hc != 8 || Wc != 8) return {};
  int rgn_rows = p_axis_extent(Hc, pad, R, false);
  int rgn_cols = p_axis_extent(Wc, pad, S, false);
  int lds_b = (bm / (Hc * Wc)) * rgn_rows * rgn_cols * Ko8 * 2 +
              W_NBUF * WSLICE_B;
  if (lds_b > W_LDS_MAX) return {};
  return DgradDirectPlan{2, bm, 0, lds_b, 1};
}

static DgradDirectPlan plan_oneshot(int H, int W, int C8, int Ko8, long ldw,
                                    int R, int S, int stride) {
  if (stride != 2 || C8 % 64 != 0 || Ko8 % 128 != 0 || ldw != Ko8)
    return {};
  // R,S >= 2 keeps every parity class's tap set non-empty (Rc,Sc >= 1)
  if (R < 2 || S < 2 || R > 8 || S > 8 || (H & 1) || (W & 1)) return {};
  int Hc = H / 2, Wc = W / 2;
  for (int bm : {128, 64}) {
    if (Wc > bm || bm % Wc != 0 || (Hc * Wc) % bm != 0) continue;
    int rows_c = bm / Wc;
    int rgn_rows = rows_c + ((R + 1) >> 1) - 1;
    int rgn_cols = Wc + ((S + 1) >> 1) - 1;
    // cap at 2 blocks/CU (160 KiB LDS): 1-block/CU shapes measured
    // slower than their dcol path (stage latency unhidden)
    int lds_b = rgn_rows * rgn_cols * Ko8 * 2 + WBUF_B;
    if (lds_b > 80 * 1024) continue;
    return DgradDirectPlan{1, bm, 0, lds_b};
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

// Grid = CUs x 2 blocks (queried once), capped by the tile count and by
// GDLJ_DGRAD_PERSIST_BLOCKS (re-read per call; lets small problems make
// one block walk several tiles).
static void launch_persistent(const DgradDirectArgs& a, DgradDirectPlan plan,
                              hipStream_t s) {
  const int bm = plan.bm, qsplit = plan.qsplit, lds_b = plan.lds_bytes;
  int Hc = a.H / 2, Wc = a.W / 2;
  int rows_c = bm / Wc;
  int rgn_rows = p_axis_extent(rows_c, a.pad, a.R, qsplit != 0);
  int rgn_cols = p_axis_extent(Wc, a.pad, a.S, false);
  cdd_set_attrs_once();
  long ntiles = (long)a.Nb * Hc * Wc / bm * (qsplit ? 2 : 1);
  long nblk = std::min<long>(ntiles, (long)device_cus() * 2);
  if (const char* e = getenv("GDLJ_DGRAD_PERSIST_BLOCKS")) {
    long cap = atol(e);
    if (cap > 0) nblk = std::min(nblk, cap);
  }
  if (nblk <= 0) return;
  dim3 grid((unsigned)nblk);
#define CDD_P_LAUNCH2(MI_, NCT_, PACT_)                                     \
  hipLaunchKernelGGL((conv_dgrad_direct_p<MI_, NCT_, PACT_>), grid,         \
                     dim3(256), lds_b, s, (const unsigned short*)a.dy,      \
                     (const unsigned short*)a.Wt, (unsigned short*)a.dx,    \
                     (const unsigned short*)a.y0, a.part, a.bias_fwd,       \
                     a.stats_part, (const unsigned short*)a.zp, a.H, a.W,   \
                     a.C8, a.Ho, a.Wo, a.Ko8, a.ldw, a.R, a.S, a.pad,       \
                     a.act, a.slope, Hc, Wc, rgn_rows, rgn_cols,            \
                     make_fastdiv(Wc), (int)ntiles, qsplit)
#define CDD_P_LAUNCH(MI_, NCT_)                                             \
  do {                                                                      \
    if (a.y0 != nullptr) CDD_P_LAUNCH2(MI_, NCT_, true);                    \
    else CDD_P_LAUNCH2(MI_, NCT_, false);                                   \
  } while (0)
  if (bm == 128 && a.C8 == 64) CDD_P_LAUNCH(2, 1);
  else if (bm == 128) CDD_P_LAUNCH(2, 2);
  else if (a.C8 == 64) CDD_P_LAUNCH(1, 1);
  else CDD_P_LAUNCH(1, 2);
#undef CDD_P_LAUNCH
#undef CDD_P_LAUNCH2
}

// Grid = CUs x 1 blocks of 512 threads, capped like launch_persistent.
static void launch_wide(const DgradDirectArgs& a, DgradDirectPlan plan,
                        hipStream_t s) {
  const int bm = plan.bm, lds_b = plan.lds_bytes;
  int Hc = a.H / 2, Wc = a.W / 2;
  int imgs = bm / (Hc * Wc);
  int rgn_rows = p_axis_extent(Hc, a.pad, a.R, false);
  int rgn_cols = p_axis_extent(Wc, a.pad, a.S, false);
  cdd_set_attrs_once();
  long ntiles = ((long)a.Nb + imgs - 1) / imgs;
  long nblk = std::min<long>(ntiles, (long)device_cus());
  if (const char* e = getenv("GDLJ_DGRAD_PERSIST_BLOCKS")) {
    long cap = atol(e);
    if (cap > 0) nblk = std::min(nblk, cap);
  }
  if (nblk <= 0) return;
  dim3 grid((unsigned)nblk);
#define CDD_W_LAUNCH2(NCT_, PACT_)                                          \
  hipLaunchKernelGGL((conv_dgrad_direct_w<NCT_, PACT_>), grid,              \
                     dim3(W_THREADS), lds_b, s,                             \
                     (const unsigned short*)a.dy,                           \
                     (const unsigned short*)a.Wt, (unsigned short*)a.dx,    \
                     (const unsigned short*)a.y0, a.part, a.bias_fwd,       \
                     a.stats_part, (const unsigned short*)a.zp, a.Nb, a.H,  \
                     a.W, a.C8, a.Ho, a.Wo, a.Ko8, a.ldw, a.R, a.S, a.pad,  \
                     a.act, a.slope, Hc, Wc, rgn_rows, rgn_cols,            \
                     make_fastdiv(Wc), (int)ntiles)
#define CDD_W_LAUNCH(NCT_)                                                  \
  do {                                                                      \
    if (a.y0 != nullptr) CDD_W_LAUNCH2(NCT_, true);                         \
    else CDD_W_LAUNCH2(NCT_, false);                                        \
  } while (0)
  if (a.C8 == 64) CDD_W_LAUNCH(1);
  else CDD_W_LAUNCH(2);
#undef CDD_W_LAUNCH
#undef CDD_W_LAUNCH2
}

static void launch_oneshot(const DgradDirectArgs& a, DgradDirectPlan plan,
                           hipStream_t s) {
  const int bm = plan.bm, lds_b = plan.lds_bytes;
  int Hc = a.H / 2, Wc = a.W / 2;
  int rows_c = bm / Wc;
  int rgn_rows = rows_c + ((a.R + 1) >> 1) - 1;
  int rgn_cols = Wc + ((a.S + 1) >> 1) - 1;
  cdd_set_attrs_once();
  dim3 grid((long)a.Nb * Hc * Wc / bm, a.C8 / 64, 4);
#define CDD_LAUNCH(MI_)                                                     \
  hipLaunchKernelGGL((conv_dgrad_direct<MI_>), grid, dim3(256), lds_b, s,   \
                     (const unsigned short*)a.dy,                           \
                     (const unsigned short*)a.Wt, (unsigned short*)a.dx,    \
                     (const unsigned short*)a.y0, a.part, a.bias_fwd,       \
                     a.stats_part, (const unsigned short*)a.zp, a.Nb, a.H,  \
                     a.W, a.C8, a.Ho, a.Wo, a.Ko8, a.ldw, a.R, a.S, a.pad,  \
                     a.act, a.slope, Hc, Wc, rows_c, rgn_rows, rgn_cols,    \
                     make_fastdiv(Wc))
  if (bm == 128) CDD_LAUNCH(2);
  else CDD_LAUNCH(1);
#undef CDD_LAUNCH
}
}  // namespace cdd

extern "C" {

// GDLJ_DGRAD_PERSIST=0 routes the direct dgrad / convT forward to the
// one-shot kernel instead of the persistent class-fused one (re-read
// per call, like the other gates).
// GDLJ_DGRAD_WIDE=0 sends the geometries of the wide kernel back to the
// two-blocks-per-CU persistent kernel (or, where that one does not take
// them, to the caller's fallback).  The result is the plan's allow mask:
// kDgradAllowPersist | kDgradAllowWide, or 0 for the one-shot kernel.
int conv_dgrad_direct_allow() {
  auto off = [](const char* name) {
    const char* e = getenv(name);
    return e != nullptr && e[0] == '0' && e[1] == '\0';
  };
  if (off("GDLJ_DGRAD_PERSIST")) return 0;
  return off("GDLJ_DGRAD_WIDE") ? kDgradAllowPersist
                                : kDgradAllowPersist | kDgradAllowWide;
}

DgradDirectPlan conv_dgrad_direct_plan(int H, int W, int C8, int Ko8,
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
  return cdd::plan_oneshot(H, W, C8, Ko8, ldw, R, S, stride);
}

void launch_conv_dgrad_direct(const DgradDirectArgs& a, DgradDirectPlan plan,
                              hipStream_t s) {
  if (plan.kind == 2 && plan.wide) cdd::launch_wide(a, plan, s);
  else if (plan.kind == 2) cdd::launch_persistent(a, plan, s);
  else if (plan.kind == 1) cdd::launch_oneshot(a, plan, s);
}

}  // extern "C"
