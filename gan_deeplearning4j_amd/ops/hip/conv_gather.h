// Implicit-GEMM gather: the one place that turns an im2col coordinate
// (row np, column k) into a source pointer into the NHWC image — or into the
// 16B zero page for padding / out-of-image taps, so global_load_lds stays
// unconditional.  ConvGather modes (launch_abi.h):
//   0  forward conv:        hi = ho*stride - pad + r
//   1  transposed (dgrad):  hi = (ho + pad - r) / stride, exact multiples only
//   2  parity class:        hi = ho + off_h - r, output rows scattered
// Every GEMM stager (gemm.hip, fp8.hip, gemm8p.hip, gemm8p_fp8.hip) owns only
// its chunk -> (row, k) mapping and its LDS destination; the address rule is
// here.  T is the image element type (unsigned short = bf16, unsigned char =
// fp8); pointer arithmetic is in elements.
#pragma once

#include "common.h"

// decode np -> (n, ho, wo)
DEV_INLINE void np_decode(const ConvGather& g, unsigned np, int& n, int& ho,
                          int& wo) {
  unsigned q1 = fdiv(np, g.fWo);
  wo = (int)(np - q1 * g.Wo);
  unsigned q2 = fdiv(q1, g.fHo);
  ho = (int)(q1 - q2 * g.Ho);
  n = (int)q2;
}

// decode k -> (r, s, c); caller checks k < rsc
DEV_INLINE void k_decode(const ConvGather& g, unsigned k, int& r, int& s,
                         int& c) {
  unsigned rs = fdiv(k, g.fC);
  c = (int)(k - rs * g.C);
  unsigned rr = fdiv(rs, g.fS);
  s = (int)(rs - rr * g.S);
  r = (int)rr;
}

// Row half of the rule, K-loop invariant: the n-plane element offset and the
// mode-adjusted spatial bases of im2col row np.
DEV_INLINE void gather_row_init(const ConvGather& g, int np, long& base,
                                int& h0, int& w0) {
  int n, ho, wo;
  np_decode(g, (unsigned)np, n, ho, wo);
  base = (long)n * g.H * g.W * g.C;
  if (g.mode == 0) {
    h0 = ho * g.stride - g.pad;
    w0 = wo * g.stride - g.pad;
  } else if (g.mode == 2) {
    h0 = ho + g.off_h;
    w0 = wo + g.off_w;
  } else {
    h0 = ho + g.pad;
    w0 = wo + g.pad;
  }
}

// Column half: source of the 16B chunk at im2col column k of a row prepared
// by gather_row_init; the zero page when k is K-padding or the tap is invalid.
template <typename T>
DEV_INLINE const T* gather_tap_src(const T* img, const ConvGather& g,
                                   const T* zp, long base, int h0, int w0,
                                   int k) {
  const T* src = zp;
  if (k < g.rsc) {
    int r, s, c;
    k_decode(g, (unsigned)k, r, s, c);
    int hi, wi;
    bool valid;
    if (g.mode == 0) {
      hi = h0 + r;
      wi = w0 + s;
      valid = hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
    } else if (g.mode == 2) {
      hi = h0 - r;
      wi = w0 - s;
      valid = hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
    } else {
      int hop = h0 - r;
      int wop = w0 - s;
      if (hop < 0 || wop < 0) {
        valid = false;
        hi = wi = 0;
      } else {
        unsigned qh = fdiv((unsigned)hop, g.fStride);
        unsigned qw = fdiv((unsigned)wop, g.fStride);
        valid = (hop == (int)(qh * g.stride)) &&
                (wop == (int)(qw * g.stride)) && (int)qh < g.H &&
                (int)qw < g.W;
        hi = (int)qh;
        wi = (int)qw;
      }
    }
    if (valid) src = img + base + (long)(hi * g.W + wi) * g.C + c;
  }
  return src;
}

// Un-hoisted form for the NT (wgrad) stager, whose row np changes every
// K-step: source address for grid position (ho,wo) + kernel offset (r,s),
// channel c; 'valid' false = use the zero page.  Same rule as the two halves
// above, kept separate because folding it into them changes generated code.
DEV_INLINE const unsigned short* gather_addr(
    const ConvGather& g, const unsigned short* img, int n, int ho, int wo,
    int r, int s, int c, bool& valid) {
  int hi, wi;
  if (g.mode == 0) {
    hi = ho * g.stride - g.pad + r;
    wi = wo * g.stride - g.pad + s;
    valid = hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
  } else if (g.mode == 2) {
    hi = ho + g.off_h - r;
    wi = wo + g.off_w - s;
    valid = hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
  } else {
    int hop = ho + g.pad - r;
    int wop = wo + g.pad - s;
    if (hop < 0 || wop < 0) {
      valid = false;
      hi = wi = 0;
    } else {
      unsigned qh = fdiv((unsigned)hop, g.fStride);
      unsigned qw = fdiv((unsigned)wop, g.fStride);
      valid = (hop == (int)(qh * g.stride)) &&
              (wop == (int)(qw * g.stride)) && (int)qh < g.H && (int)qw < g.W;
      hi = (int)qh;
      wi = (int)qw;
    }
  }
  return img + (((long)n * g.H + hi) * g.W + wi) * g.C + c;
}

// Mode-2 output scatter: GEMM row grow (a position of one parity class) ->
// row of the full-resolution [N][oH][oW] output.
DEV_INLINE long scatter_row(const ConvGather& ga, int grow) {
  int n, h2, w2;
  np_decode(ga, (unsigned)grow, n, h2, w2);
  return ((long)n * ga.oH + h2 * ga.stride + ga.oqh) * ga.oW +
         w2 * ga.stride + ga.oqw;
}

// ---------------------------------------------------------------------------
// Stagers for the 128-tile kernels' LDS image: [row][8 slots of 16 B], XOR
// swizzled through the SOURCE address (slot ^ (row & 7)) so the LDS
// destination stays wave-uniform + lane-linear.  A slot holds 16/sizeof(T)
// elements of k.  NTH = block thread count, ITERS = chunks per thread
// (rows staged = NTH * ITERS / 8).
// ---------------------------------------------------------------------------
template <int NTH, int ITERS, typename T>
DEV_INLINE void tn_stage_rows(const T* __restrict__ g, int row0, int nrows,
                              long ldk, int k0, char* lds) {
  constexpr int CE = 16 / (int)sizeof(T);
  const int t = threadIdx.x;
  const int wid = t >> 6;
  #pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    int chunk = i * NTH + t;         // = row*8 + slot
    int row = chunk >> 3;
    int slot = chunk & 7;
    int gslot = slot ^ (row & 7);    // inverse swizzle on the source
    int grow = min(row0 + row, nrows - 1);
    const T* src = g + (long)grow * ldk + k0 + gslot * CE;
    char* dst = lds + (i * NTH + wid * 64) * 16;
    GLDS16(src, dst);
  }
}

// Implicit-GEMM flavor: rows are im2col rows gathered from the NHWC image.
// Each thread stages the same 4 rows every K-step, so the row half is hoisted
// into registers once (init) and only the tap + channel part is decoded per
// chunk per step (stage).  fp8 chunks are 16 channels and must not straddle
// an (r,s) boundary: C % 16 == 0, enforced by the binding.
template <int NTH, typename T>
struct TnGatherStager {
  long base[4];        // (long)n * H*W*C element offset per chunk
  int h0[4], w0[4];    // mode-adjusted spatial bases per chunk

  DEV_INLINE void init(const ConvGather& g, int row0, int nrows) {
    const int t = threadIdx.x;
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
      int row = (i * NTH + t) >> 3;
      gather_row_init(g, min(row0 + row, nrows - 1), base[i], h0[i], w0[i]);
    }
  }

  DEV_INLINE void stage(const T* __restrict__ img, const ConvGather& g,
                        const T* __restrict__ zp, int k0, char* lds) const {
    constexpr int CE = 16 / (int)sizeof(T);
    const int t = threadIdx.x;
    const int wid = t >> 6;
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
      int chunk = i * NTH + t;
      int row = chunk >> 3;
      int slot = chunk & 7;
      int gslot = slot ^ (row & 7);
      const T* src = gather_tap_src(img, g, zp, base[i], h0[i], w0[i],
                                    k0 + gslot * CE);
      char* dst = lds + (i * NTH + wid * 64) * 16;
      GLDS16(src, dst);
    }
  }
};
