// Deep-pipelined bf16 MFMA NT (weight-grad) GEMM for gfx950 (CDNA4):
//   C[M][N] (fp32) (+)= sum_k A[k][M] * B[k][N]
// the contraction runs over operand ROWS; either operand may be the im2col
// of an NHWC image (implicit wgrad), exactly as in gemm_nt_core (gemm.hip),
// which stays as the fallback and the A/B arm (GDLJ_NT8P=0).
//
// What changes against gemm_nt_core is the schedule and the tile, not the
// arithmetic.  gemm_nt_core drains vmcnt(0) + __syncthreads() after every
// 64-row K-step and gives each wave a 64x32 panel (24 tr-reads per 16
// MFMAs).  Here the K-step is cut into the 4 phases of gemm8p.hip, each
//   { tr-reads of one quadrant's fragments | issue one staging region via
//     global_load_lds | raw s_barrier | s_waitcnt lgkmcnt(0) | MFMA
//     quadrant | raw s_barrier }
// with ONE counted s_waitcnt vmcnt per K-tile, so the LDS-DMA of the next
// two tiles stays in flight across barriers; no __syncthreads() in the loop.
//
// Tiles (BMT x BNT x 64), 8 waves, one block per CU:
//   256x256: waves 2(M) x 4(N), wave panel 128x64 (8x4 fragments, 128 acc
//            VGPRs), 48 tr-reads per 64 MFMAs; LDS 2 x 64 KiB; vmcnt(4).
//   128x256: waves 2 x 4, panel 64x64; LDS 2 x 48 KiB; vmcnt(3).  conv2-class
//            wgrad (M = Ko8 = 128).
//   256x128: waves 4 x 2, panel 64x64; LDS 2 x 48 KiB; vmcnt(3).  convT3-class
//            wgrad (N = Cin = 128).
//
// LDS image, per operand tile of width W: two HALVES of W/2 columns (the
// staging regions), each the window-linear [kb 0..15][mbl][4k][16m] image
// of gemm_nt_core (window = 128 B, kb = 4 contraction rows).  The fragment
// mapping is nt_tr_frag's: lane -> column mb*16 + fr, k = kc*32 + fq*8 +
// 0..7, kc ascending inside a K-tile — every C element therefore sees the
// same MFMA sequence as in gemm_nt_core and a splitk == 1 result is
// bit-equal to it.
// Bank rule (ds_read_b64_tr_b16: bank = (addr/4) % 64, conflicts per
// 32-lane half): the lane groups fq and fq+1 read kb and kb+2, a multiple
// of 256 B apart in the linear image, i.e. the same 128-B half of the bank
// row: 2-way.  So window mbl of row kb is stored at mbl ^ ((kb >> 1) & 1):
// groups fq and fq^1 then sit in opposite 128-B halves (conflict-free).  The
// XOR is applied to the glds SOURCE column (the LDS destination of
// global_load_lds stays wave-uniform + lane-linear) and to the read address.
//
// Staging schedule (as gemm8p.hip): regions R0/R2 = A half 0/1, R1/R3 = B
// half 0/1; phase p of tile t computes quadrant (mih,nih) = p1 (0,0)
// p2 (0,1) p3 (1,0) p4 (1,1) and issues
//   p1 -> R2(t+1)   p2 -> R3(t+1)   p3 -> R0(t+2)   p4 -> R1(t+2)
// The wave's half-mih fragments are columns mih*(BMT/2) + ..., so a region
// is dead as soon as its quadrant reads are done.  The counted wait at p4
// leaves exactly R0(t+2) + R1(t+2) in flight.  Tail tiles clamp to the
// block's last K-tile and restage identical data, so the glds count per
// phase is constant and the vmcnt immediate exact.
//
// The MFMA block, the fragment reads and the store loop are written out
// here, not shared with gemm_nt_core (docs/KERNELS.md, "Deliberately NOT
// shared").

#include "conv_gather.h"

namespace nt8 {

constexpr int BK = 64;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

// One operand tile of width W (256 or 128 columns).
template <int W>
struct Op {
  static constexpr int HALF_B = W * 64;   // bytes per half (W/2 cols x 64 k)
  static constexpr int KBROW_B = W * 4;   // bytes per kb row of a half
  static constexpr int TILE_B = W * 128;  // both halves
  static constexpr int NIT = W / 128;     // glds per thread per half

  // this thread's chunk of iteration i: kb row, column inside the half
  // (source-side XOR applied), contraction row inside the K-tile
  static DEV_INLINE int kb_of(int i) {
    const int wid = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    return W == 256 ? i * 8 + wid : wid * 2 + (lane >> 5);
  }
  static DEV_INLINE int colq() {
    const int wid = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    int pw = W == 256 ? (lane >> 3) : ((lane >> 3) & 3);
    int sw = W == 256 ? ((wid >> 1) & 1) : (wid & 1);  // (kb >> 1) & 1
    return ((pw ^ sw) << 4) + ((lane & 1) << 3);
  }
  static DEV_INLINE int rowq(int i) {
    const int lane = threadIdx.x & 63;
    return kb_of(i) * 4 + ((lane >> 1) & 3);
  }
  // wave-uniform LDS destination of iteration i inside a half
  static DEV_INLINE int dstq(int i) {
    const int wid = threadIdx.x >> 6;
    return (W == 256 ? i * 8 + wid : wid) << 10;
  }
};

// plain operand: rows are contraction rows, columns clamp at the L edge
// (columns >= L are never stored)
template <int W>
DEV_INLINE void stage_plain(const unsigned short* __restrict__ g, int k0,
                            int K, int c0, int L, long ldl,
                            const unsigned short* __restrict__ zp, int half,
                            char* op) {
  const int cq = c0 + half * (W / 2) + Op<W>::colq();
  #pragma unroll
  for (int i = 0; i < Op<W>::NIT; ++i) {
    int row = k0 + Op<W>::rowq(i);
    const unsigned short* src = zp;
    if (row < K) {
      int col = min(cq, max(0, L - 8));
      src = g + (long)row * ldl + col;
    }
    GLDS16(src, op + half * Op<W>::HALF_B + Op<W>::dstq(i));
  }
}

// gathered operand: the im2col of an NHWC image (contraction row = np,
// tile column = rsc coordinate).  The column-side k_decode is K-loop
// invariant (one coordinate per half) and hoisted; the row-side np_decode
// runs once per K-tile, at the half-0 stage, and is reused by the half-1
// stage of the same tile (the schedule always issues them in that order).
template <int W>
struct GatherOp {
  int r[2], s[2], cc[2];
  bool in_rsc[2];
  int n[Op<W>::NIT], ho[Op<W>::NIT], wo[Op<W>::NIT];

  DEV_INLINE void init(const ConvGather& g, int c0) {
    #pragma unroll
    for (int h = 0; h < 2; ++h) {
      int kk = c0 + h * (W / 2) + Op<W>::colq();
      in_rsc[h] = kk < g.rsc;
      if (in_rsc[h])
        k_decode(g, (unsigned)kk, r[h], s[h], cc[h]);
      else
        r[h] = s[h] = cc[h] = 0;
    }
  }

  DEV_INLINE void stage(const unsigned short* __restrict__ img,
                        const ConvGather& g, int k0, int K,
                        const unsigned short* __restrict__ zp, int half,
                        char* op) {
    #pragma unroll
    for (int i = 0; i < Op<W>::NIT; ++i) {
      int np = k0 + Op<W>::rowq(i);
      if (half == 0) np_decode(g, (unsigned)np, n[i], ho[i], wo[i]);
      const unsigned short* src = zp;
      if (np < K && in_rsc[half]) {
        bool valid;
        const unsigned short* p = gather_addr(g, img, n[i], ho[i], wo[i],
                                              r[half], s[half], cc[half],
                                              valid);
        if (valid) src = p;
      }
      GLDS16(src, op + half * Op<W>::HALF_B + Op<W>::dstq(i));
    }
  }
};

// fragment mbl (compile-time; relative to the wave's first window, which is
// even) of a half, K-half kc: lane holds column mbl*16 + fr, k = kc*32 +
// fq*8 + 0..7.  be / bo are the lane's byte addresses for even / odd mbl
// (the fq-parity XOR folded in).
// The __restrict__ qualifiers are load-bearing: the tr-read builtin carries
// no alias metadata of its own, and without any the compiler treats every
// outstanding global_load_lds as a possible writer of the address and puts
// s_waitcnt vmcnt(0) in front of each group of reads, which drains the
// pipeline every phase.  Inlining a __restrict__ parameter attaches scope
// metadata to the reads; the .s then holds only the counted waits.
template <int W>
DEV_INLINE bf16x8 tr_frag(const char* __restrict__ be,
                          const char* __restrict__ bo, int half, int mbl,
                          int kc) {
  const char* p = ((mbl & 1) ? bo : be) + half * Op<W>::HALF_B +
                  kc * 8 * Op<W>::KBROW_B + mbl * 128;
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4*)p);
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4*)(p + Op<W>::KBROW_B));
  bf16x8 v;
  #pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = lo[j];
    v[4 + j] = hi[j];
  }
  return v;
}

}  // namespace nt8

// GMODE: 0 = plain/plain, 1 = A gathered, 2 = B gathered
// (A third LDS stage for the narrow tiles - every region issued a full
// K-tile ahead, vmcnt(6) - measured 1-5% SLOWER than this schedule and was
// removed: profiles/wgrad_nt8p_ab.md.)
template <int GMODE, int BMT, int BNT>
__global__ __launch_bounds__(512, 1) void gemm_nt_8p(
    const unsigned short* __restrict__ A, const unsigned short* __restrict__ B,
    float* __restrict__ C, int M, int N, int K, long lda, long ldb,
    int kchunks_per_block, int use_atomic, int xcd, ConvGather gg,
    const unsigned short* __restrict__ zp) {
  using namespace nt8;
  using OA = Op<BMT>;
  using OB = Op<BNT>;
  constexpr int BUF = OA::TILE_B + OB::TILE_B;
  constexpr int MI = (BMT == 256 && BNT == 256) ? 8 : 4;  // M fragments/wave
  constexpr int MH = MI / 2;                              // per quadrant
  constexpr int WCN = BNT / 64;                           // waves along N
  constexpr int INFL = OA::NIT + OB::NIT;  // glds left in flight at p4
  static_assert((BMT / (MI * 16)) * WCN == 8, "8 waves");
  extern __shared__ __attribute__((aligned(16))) char lds[];

  // XCD-aware remap over the whole 3-D grid (K-split slowest): hardware
  // deals consecutive block ids round-robin to the 8 XCDs, which scatters
  // the blocks of one K-split - the ones that stage the same operand rows -
  // over all eight L2s.  The remap hands each XCD a contiguous run of ids,
  // i.e. whole K-splits, so an A panel is fetched into one L2 once per
  // split instead of once per XCD.
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (xcd) {
    const int gx = gridDim.x, gy = gridDim.y;
    const int nwg = gx * gy * (int)gridDim.z;
    const int bid = xcd_remap(bx + gx * (by + gy * bz), nwg);
    const int q = bid / gx;
    bx = bid - q * gx;
    bz = q / gy;
    by = q - bz * gy;
  }
  const int m0 = bx * BMT;
  const int n0 = by * BNT;

  const int kchunks = (K + BK - 1) / BK;
  const int kt0 = bz * kchunks_per_block;
  const int kt1 = min(kt0 + kchunks_per_block, kchunks);
  if (kt0 >= kt1) return;  // whole block; before any barrier

  // one-time priority for the younger dispatch half (as gemm_tn_8p)
  if (__builtin_amdgcn_readfirstlane(threadIdx.x) >= 256)
    __builtin_amdgcn_s_setprio(1);

  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wr = wid / WCN, wc = wid % WCN;
  const int fr = lane & 15, fq = lane >> 4;

  f32x4 acc[MI][4];
  #pragma unroll
  for (int i = 0; i < MI; ++i)
    #pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  auto abuf = [&](int tt) -> char* { return lds + (tt & 1) * BUF; };
  auto bbuf = [&](int tt) -> char* { return abuf(tt) + OA::TILE_B; };

  GatherOp<BMT> gca;
  GatherOp<BNT> gcb;
  if (GMODE == 1) gca.init(gg, m0);
  if (GMODE == 2) gcb.init(gg, n0);
  auto stage_a = [&](int tt, int half) {
    int tc = min(tt, kt1 - 1);
    if (GMODE == 1)
      gca.stage(A, gg, tc * BK, K, zp, half, abuf(tc));
    else
      stage_plain<BMT>(A, tc * BK, K, m0, M, lda, zp, half, abuf(tc));
  };
  auto stage_b = [&](int tt, int half) {
    int tc = min(tt, kt1 - 1);
    if (GMODE == 2)
      gcb.stage(B, gg, tc * BK, K, zp, half, bbuf(tc));
    else
      stage_plain<BNT>(B, tc * BK, K, n0, N, ldb, zp, half, bbuf(tc));
  };

#define NT8_VMWAIT()                                                         \
  do {                                                                       \
    if (INFL == 4)                                                           \
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");                       \
    else                                                                     \
      asm volatile("s_waitcnt vmcnt(3)" ::: "memory");                       \
  } while (0)

  // prologue: all of the first tile, then R0+R1 of the second; the wait
  // leaves that pair in flight (the steady-state queue)
  stage_a(kt0, 0);
  stage_b(kt0, 0);
  stage_a(kt0, 1);
  stage_b(kt0, 1);
  asm volatile("" ::: "memory");  // first tile's glds older than the pair
  stage_a(kt0 + 1, 0);
  stage_b(kt0 + 1, 0);
  NT8_VMWAIT();
  __builtin_amdgcn_s_barrier();

  // lane byte offsets of the tr-reads: kb = kc*8 + 2*fq (+1 for the high
  // half of k), column fr*4 elements inside the window row group; the
  // (kb >> 1) & 1 = fq & 1 window XOR becomes +-128 B for even / odd mbl
  const int sw = (fq & 1) * 128;
  // the wave's first window (wr*MH resp. wc*2, both even) rides in the base
  const int la = 2 * fq * OA::KBROW_B + fr * 8 + wr * MH * 128;
  const int lb = 2 * fq * OB::KBROW_B + fr * 8 + wc * 2 * 128;

  bf16x8 a[MH][2], blo[2][2], bhi[2][2];

#define NT8_QUAD(MIH, NIH, BREG)                                             \
  _Pragma("unroll") for (int kc = 0; kc < 2; ++kc)                           \
      _Pragma("unroll") for (int mi = 0; mi < MH; ++mi)                      \
      _Pragma("unroll") for (int ni = 0; ni < 2; ++ni)                       \
      acc[(MIH)*MH + mi][(NIH)*2 + ni] =                                     \
      __builtin_amdgcn_mfma_f32_16x16x32_bf16(                               \
          a[mi][kc], BREG[ni][kc], acc[(MIH)*MH + mi][(NIH)*2 + ni], 0, 0,   \
          0)

#define NT8_BAR_MFMA(MIH, NIH, BREG)                                         \
  __builtin_amdgcn_s_barrier();                                              \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                         \
  __builtin_amdgcn_sched_barrier(0);                                         \
  NT8_QUAD(MIH, NIH, BREG);                                                  \
  __builtin_amdgcn_s_barrier()

  for (int t = kt0; t < kt1; ++t) {
    const char* Ab = abuf(t);
    const char* Bb = bbuf(t);
    const char* ae = Ab + la + sw;
    const char* ao = Ab + la - sw;
    const char* be = Bb + lb + sw;
    const char* bo = Bb + lb - sw;

    // phase 1: A(half 0) + B(half 0) fragments; stage R2(t+1)
    #pragma unroll
    for (int mi = 0; mi < MH; ++mi) {
      a[mi][0] = tr_frag<BMT>(ae, ao, 0, mi, 0);
      a[mi][1] = tr_frag<BMT>(ae, ao, 0, mi, 1);
    }
    #pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      blo[ni][0] = tr_frag<BNT>(be, bo, 0, ni, 0);
      blo[ni][1] = tr_frag<BNT>(be, bo, 0, ni, 1);
    }
    stage_a(t + 1, 1);
    NT8_BAR_MFMA(0, 0, blo);

    // phase 2: B(half 1) fragments; stage R3(t+1)
    #pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      bhi[ni][0] = tr_frag<BNT>(be, bo, 1, ni, 0);
      bhi[ni][1] = tr_frag<BNT>(be, bo, 1, ni, 1);
    }
    stage_b(t + 1, 1);
    NT8_BAR_MFMA(0, 1, bhi);

    // phase 3: A(half 1) fragments; stage R0(t+2)
    #pragma unroll
    for (int mi = 0; mi < MH; ++mi) {
      a[mi][0] = tr_frag<BMT>(ae, ao, 1, mi, 0);
      a[mi][1] = tr_frag<BMT>(ae, ao, 1, mi, 1);
    }
    stage_a(t + 2, 0);
    NT8_BAR_MFMA(1, 0, blo);

    // phase 4: no reads; stage R1(t+2); the tile's single counted wait
    stage_b(t + 2, 0);
    NT8_VMWAIT();
    __builtin_amdgcn_s_barrier();
    NT8_QUAD(1, 1, bhi);
    __builtin_amdgcn_s_barrier();
  }
#undef NT8_BAR_MFMA
#undef NT8_QUAD
#undef NT8_VMWAIT

  // drain the clamped tail stages before the block may exit
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  #pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    #pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      int col = n0 + (ni >> 1) * (BNT / 2) + (wc * 2 + (ni & 1)) * 16 + fr;
      if (col >= N) continue;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m0 + (mi / MH) * (BMT / 2) + (wr * MH + mi % MH) * 16 +
                  fq * 4 + r;
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
extern "C" {

// GDLJ_NT8P=0 keeps every NT GEMM on gemm_nt_core (re-read per call).
static int nt8_enabled() {
  const char* e = getenv("GDLJ_NT8P");
  return !(e != nullptr && e[0] == '0' && e[1] == '\0');
}

static int nt8_ncu() {
  static const int v = [] {
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  return v;
}

// >64 KiB dynamic LDS needs an explicit opt-in per kernel
static void nt8_set_attrs() {
  static const int once = [] {
    #define NT8_SETATTR(G, BM_, BN_)                                         \
      (void)hipFuncSetAttribute(                                             \
          reinterpret_cast<const void*>(&gemm_nt_8p<G, BM_, BN_>),           \
          hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (BM_ + BN_) * 128)
    NT8_SETATTR(0, 256, 256);
    NT8_SETATTR(1, 256, 256);
    NT8_SETATTR(2, 256, 256);
    NT8_SETATTR(0, 128, 256);
    NT8_SETATTR(2, 128, 256);
    NT8_SETATTR(0, 256, 128);
    NT8_SETATTR(1, 256, 128);
    #undef NT8_SETATTR
    return 1;
  }();
  (void)once;
}

// Default floors (profiles/wgrad_nt8p_ab.md): the pipeline needs a deep
// contraction to amortize its two-tile prologue and one block per CU, so a
// shape is taken when it has >= kNt8MinK contraction rows and both C dims
// reach the narrow tile.  GDLJ_NT8P_MINK=<rows> (re-read per call) replaces
// the K floor and waives the M/N floor: a test / microbench override.
constexpr int kNt8MinK = 32768;

int launch_gemm_nt_8p(const void* A, const void* B, float* C, int M, int N,
                      int K, long lda, long ldb, int splitk, int gmode,
                      ConvGather gg, const void* zp, hipStream_t s) {
  if (!nt8_enabled()) return 0;
  if (const char* e = getenv("GDLJ_NT8P_MINK")) {
    if (K < atoi(e)) return 0;
  } else if (K < kNt8MinK || M < 128 || N < 128) {
    return 0;
  }
  // narrow side: a 128-wide tile where a 256-wide one would be half empty;
  // the gathered operand of an instantiated narrow tile is the wide side
  int bmt = 256, bnt = 256;
  if (M <= 128 && gmode != 1) bmt = 128;
  else if (N <= 128 && gmode != 2) bnt = 128;
  nt8_set_attrs();
  const int kchunks = (K + nt8::BK - 1) / nt8::BK;
  const int gm = ceil_div(M, bmt), gn = ceil_div(N, bnt);
  // split-K for this tile count: one block per CU; a caller that passed 1
  // gets plain stores into its uninitialised C, so it stays 1
  int sk = 1;
  if (splitk > 1) {
    sk = nt8_ncu() / (gm * gn);
    if (sk > kchunks) sk = kchunks;
    if (sk < 1) sk = 1;
  }
  const int per_block = (kchunks + sk - 1) / sk;
  const int ua = splitk > 1 ? 1 : 0;
  dim3 grid(gm, gn, sk);
  const int lds_b = 2 * (bmt + bnt) * 128;
  // GDLJ_NT8P_XCD=0: plain x/y/z block order (A/B arm of the XCD remap)
  const char* xe = getenv("GDLJ_NT8P_XCD");
  const int xcd = !(xe != nullptr && xe[0] == '0' && xe[1] == '\0');
  #define NT8_LAUNCH(G, BM_, BN_)                                            \
    hipLaunchKernelGGL((gemm_nt_8p<G, BM_, BN_>), grid, dim3(512), lds_b, s, \
                       (const unsigned short*)A, (const unsigned short*)B,   \
                       C, M, N, K, lda, ldb, per_block, ua, xcd, gg,         \
                       (const unsigned short*)zp)
  if (bmt == 128) {
    if (gmode == 2) NT8_LAUNCH(2, 128, 256);
    else NT8_LAUNCH(0, 128, 256);
  } else if (bnt == 128) {
    if (gmode == 1) NT8_LAUNCH(1, 256, 128);
    else NT8_LAUNCH(0, 256, 128);
  } else {
    if (gmode == 1) NT8_LAUNCH(1, 256, 256);
    else if (gmode == 2) NT8_LAUNCH(2, 256, 256);
    else NT8_LAUNCH(0, 256, 256);
  }
  #undef NT8_LAUNCH
  return 1;
}

}  // extern "C"
