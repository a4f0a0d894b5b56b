// Host/kernel launch ABI of the gfx950 kernel library: the one declaration
// of every struct passed by value from the bindings (ext.cpp) through the
// launchers into kernels, and of every extern "C" function that crosses a
// translation unit.  Plain host C++17: every .hip sees it through common.h
// and ext.cpp includes it, so a definition that disagrees with its prototype
// is a compile error ("conflicting types"), not a run-time mismatch.
// The structs stay at global scope with this field order: they appear in
// __global__ signatures, so moving them renames kernel symbols.
#pragma once

#include <hip/hip_runtime.h>

// Rows of every per-block partial-sum buffer the bindings allocate
// ([kPartRows][C] bias-grad, [kPartRows][2*C] BN sum/sumsq).  Launchers that
// fill one clamp grid.x to it; the direct dgrad kernels, whose grids may be
// larger, index it with blockIdx.x & (kPartRows - 1).
constexpr int kPartRows = 2048;

// ------------------------------------------------- fast integer division
// Granlund-Montgomery round-up magic; exact for 0 <= n < 2^30, 1 <= d < 2^16.
// mul is 64-bit: for power-of-two (and small) divisors ceil(2^(32+l)/d)
// exceeds 32 bits.  Device side: fdiv / fmod_ in common.h.
struct FastDiv {
  unsigned long long mul;
  int shift;  // = 32 + ceil(log2 d)
  int d;
};

inline FastDiv make_fastdiv(int d) {
  int l = 0;
  while ((1 << l) < d) ++l;
  FastDiv f;
  f.shift = 32 + l;
  f.mul = ((1ULL << (32 + l)) + (unsigned long long)d - 1) /
          (unsigned long long)d;
  f.d = d;
  return f;
}

// ------------------------------------------------------------ geometries
// Explicit im2col / col2im (im2col.hip).
struct ConvGeom {
  int N, H, W, C;       // image dims (the im2col SOURCE / col2im TARGET)
  int Ho, Wo;           // patch-grid dims
  int R, S;             // kernel
  int stride, pad;
  int kpad;             // padded K = round_up(R*S*C, 64)
};

// Max-pool (pool.hip).
struct PoolGeom {
  int N, H, W, C;   // input dims
  int Ho, Wo;       // output dims
  int k, stride;    // kernel, stride (square)
};

// Conv gather geometry for implicit-GEMM staging: maps an im2col
// coordinate (np, k) to an input-image address without materializing col.
// mode 0 (forward):    src pixel = grid_pos * stride - pad + (r,s)
// mode 1 (transposed): src pixel = (grid_pos + pad - (r,s)) / stride,
//                      valid only when divisible (conv dgrad / convT fwd)
// mode 2 (parity class of a stride-2 transposed conv): the GEMM covers one
//   (qh,qw) output-parity class; R,S are the per-class tap counts and
//   (r,s) taps map to src pixel (grid_pos + off - tap); output rows
//   scatter back to the full image via (oH,oW,oqh,oqw) in the epilogue.
//   Every tap is valid (no 4x zero-padding like mode 1 at stride 2).
struct ConvGather {
  int N, H, W, C;        // source image dims (NHWC)
  int Ho, Wo;            // patch grid (mode 2: the class grid)
  int R, S, stride, pad;
  int rsc;               // R*S*C (valid k range; >= rsc is zero padding)
  int mode;
  int off_h, off_w;      // mode 2: ho = hi2 + off - r2
  int oH, oW, oqh, oqw;  // mode 2: output scatter (full dims + class)
  FastDiv fC, fS, fWo, fHo, fStride;
};

// Modes 0/1 are complete as returned; mode 2 callers fill off_* / o*.
inline ConvGather make_conv_gather(int N, int H, int W, int C, int Ho, int Wo,
                                   int R, int S, int stride, int pad,
                                   int mode = 0) {
  ConvGather g;
  g.N = N; g.H = H; g.W = W; g.C = C; g.Ho = Ho; g.Wo = Wo;
  g.R = R; g.S = S; g.stride = stride; g.pad = pad;
  g.rsc = R * S * C;
  g.mode = mode;
  g.off_h = g.off_w = 0;
  g.oH = g.oW = g.oqh = g.oqw = 0;
  g.fC = make_fastdiv(C);
  g.fS = make_fastdiv(S);
  g.fWo = make_fastdiv(Wo);
  g.fHo = make_fastdiv(Ho);
  g.fStride = make_fastdiv(stride);
  return g;
}

// ------------------------------------------- direct dgrad plan / arguments
// Which direct strided dgrad kernel takes a geometry, and its tiling.
struct DgradDirectPlan {
  int kind;       // 0 ineligible, 1 one-shot kernel, 2 persistent kernels,
                  // 3 one gathered 8-phase GEMM per parity class (gemm8p.hip)
                  // with the taps rounded as dcol stores them, 4 the same
                  // with all taps accumulated in fp32
  int bm;         // class pixels per tile: 128 or 64 (wide: always 128)
  int qsplit;     // persistent only: 1 = tiles split by row parity
  int lds_bytes;  // dynamic LDS per block
  int wide;       // kind 2: 1 = wide kernel, one 8-wave block per CU
};

// allow mask of conv_dgrad_direct_plan (wide needs persist as well)
constexpr int kDgradAllowPersist = 1;
constexpr int kDgradAllowWide = 2;
constexpr int kDgradAllowClassGemm = 4;  // kind 3 / 4, the last resort
constexpr int kDgradClassFp32 = 8;       // kind 4 instead of kind 3

// Arguments of the direct dgrad launch, named for the conv data-grad.  The
// strided convT FORWARD runs the same kernel with the roles swapped: dy is
// the input x, Wt the "w2a" pack, dx the output y; H,W are then the OUTPUT
// dims and Ho,Wo the INPUT dims, C8 the padded output channels and Ko8 the
// padded input channels (the contraction).
struct DgradDirectArgs {
  const void* dy;         // [Nb][Ho][Wo][Ko8] bf16
  const void* Wt;         // [R*S*C8][ldw] bf16, k = co
  void* dx;               // [Nb][H][W][C8] bf16
  const void* y0;         // dgrad: producer act output (act bwd), or null
  float* part;            // dgrad: [kPartRows][C8] bias-grad partials, or null
  const float* bias_fwd;  // convT fwd: bias (non-null selects act forward)
  float* stats_part;      // convT fwd: [kPartRows][2*C8] BN partials, or null
  const void* zp;         // 16B zero page
  int Nb, H, W, C8, Ho, Wo, Ko8;
  long ldw;
  int R, S, pad, act;
  float slope;
};

// ----------------------------------------------------------- prototypes
// Grouped by defining file.  void* data is bf16 unless noted; lda/ldb/ldw
// are row pitches in elements.
extern "C" {

// gemm.hip -- launch_gemm_tn* return grid.x (= rows of bn_part written).
int launch_gemm_tn(const void* A, const void* B, void* C_bf16, float* C_f32,
                   const float* bias, int M, int N, int K, long lda, long ldb,
                   int act, float slope, float* bn_part, hipStream_t s);
int launch_gemm_tn_gather(const void* img, const void* B, void* C_bf16,
                          const float* bias, int M, int N, int K, long ldb,
                          int act, float slope, ConvGather ga,
                          const void* zero_page, float* bn_part,
                          hipStream_t s);
// gmode: 0 plain, 1 = A gathered, 2 = B gathered (through gg)
void launch_gemm_nt(const void* A, const void* B, float* C, int M, int N,
                    int K, long lda, long ldb, int splitk, int gmode,
                    ConvGather gg, const void* zp, hipStream_t s);

// gemm8p.hip
int gemm_tn_8p_eligible(int M, int N, int K);
int launch_gemm_tn_8p(const void* A, const void* B, void* C,
                      const float* bias, int M, int N, int K, long lda,
                      long ldb, int act, float slope, int gather,
                      ConvGather ga, const void* zp, hipStream_t s);
int launch_gemm_tn_8p_tweak(int tweak, const void* A, const void* B, void* C,
                            int M, int N, int K, long lda, long ldb,
                            hipStream_t s);
// Strided dgrad / convT forward as one gathered GEMM per parity class, B read
// in place from the [(r,s,c)][ko] pack (a.Wt).  _eligible: geometry, the 8p
// floors on rows and blocks per class (GDLJ_DGRAD_CLASSGEMM_MINM replaces
// them, read per call); Nb <= 0 is never eligible.  The launch uses a.bias_fwd
// / a.act as the epilogue (dgrad: bias_fwd null, identity) and ignores a.y0,
// a.part and a.stats_part.  fp32_taps = 0: 128-wide tile, every tap's sum
// rounded to bf16 before the taps add up, dx / y bit-equal to dcol GEMM +
// col2im; 1: 256-wide tile, one fp32 accumulation over all taps.
int conv_dgrad_classgemm_eligible(int Nb, int H, int W, int C8, int Ko8,
                                  long ldw, int R, int S, int stride,
                                  int pad);
void launch_conv_dgrad_classgemm(const DgradDirectArgs& a, int fp32_taps,
                                 hipStream_t s);

// gemm8p_nt.hip -- arguments as launch_gemm_nt; returns 1 and launches when
// the shape is eligible (GDLJ_NT8P, GDLJ_NT8P_MINK), else 0.
int launch_gemm_nt_8p(const void* A, const void* B, float* C, int M, int N,
                      int K, long lda, long ldb, int splitk, int gmode,
                      ConvGather gg, const void* zp, hipStream_t s);

// fp8.hip -- e4m3 data is unsigned char; amax_bits holds a float's bits.
void launch_amax(const void* x, long n, unsigned* amax_bits, hipStream_t s);
void launch_fp8_make_scale(const unsigned* amax_bits, float* scale,
                           float* inv, hipStream_t s);
void launch_quant_fp8(const void* x, void* y, long n, const float* scale,
                      hipStream_t s);
void launch_quant_fp8_delayed(const void* x, void* y, long n,
                              const float* scale, unsigned* amax_bits,
                              hipStream_t s);
void launch_fp8_roll_scale(unsigned* amax_bits, float* scale, float* inv,
                           hipStream_t s);
void launch_gemm_tn_fp8(const void* A, const void* B, void* C,
                        const float* bias, const float* inv_qa,
                        const float* inv_qb, int M, int N, int K, long lda,
                        long ldb, int act, float slope, int gather,
                        ConvGather ga, const void* zp, hipStream_t s);

// gemm8p_fp8.hip
int gemm_tn_8p_fp8_eligible(int M, int N, int K);
int launch_gemm_tn_8p_fp8(const void* A, const void* B, void* C,
                          const float* bias, const float* inv_qa,
                          const float* inv_qb, int M, int N, int K, long lda,
                          long ldb, int act, float slope, int gather,
                          ConvGather ga, const void* zp, hipStream_t s);

// conv_direct.hip -- returns 1 and launches when eligible, else 0.
int launch_conv_direct_smallc(const void* img, const void* Wp, void* C,
                              const float* bias, const void* zp, int Nb,
                              int H, int W, int C8, int Ho, int Wo, int R,
                              int S, int stride, int pad, int Kout, int kpad,
                              int act, float slope, hipStream_t s);

// conv_dgrad_direct.hip
// Allow mask from GDLJ_DGRAD_PERSIST / GDLJ_DGRAD_WIDE /
// GDLJ_DGRAD_CLASSGEMM / GDLJ_DGRAD_CLASSGEMM_FP32, read per call.
int conv_dgrad_direct_allow();
// Tries the wide, then the persistent kernel (as `allow` permits), then the
// one-shot one, and where all three refuse the class GEMMs (kind 3, or 4
// with kDgradClassFp32), whose floors depend on the batch Nb (0 = unknown:
// never).
DgradDirectPlan conv_dgrad_direct_plan(int Nb, int H, int W, int C8, int Ko8,
                                       long ldw, int R, int S, int stride,
                                       int pad, int allow);
void launch_conv_dgrad_direct(const DgradDirectArgs& a, DgradDirectPlan plan,
                              hipStream_t s);

// im2col.hip -- the int launchers return grid.x (= rows of part written).
int launch_col2im_stats(const void* dcol, void* din, ConvGeom g,
                        const float* bias, int act, float slope, float* part,
                        hipStream_t s);
int launch_col2im_dact(const void* dcol, void* din, ConvGeom g,
                       const void* y0, int act, float slope, float* part,
                       hipStream_t s);
void launch_im2col(const void* in, void* col, ConvGeom g, hipStream_t s);
void launch_col2im(const void* dcol, void* din, ConvGeom g, const float* bias,
                   int act, float slope, hipStream_t s);

// pool.hip -- argmax is one byte per output element.
void launch_maxpool_fwd(const void* in, void* out, void* argmax, PoolGeom g,
                        hipStream_t s);
void launch_maxpool_bwd(const void* dout, const void* argmax, void* din,
                        PoolGeom g, hipStream_t s);
void launch_upsample_fwd(const void* in, void* out, int n, int h, int w,
                         int c, int scale, hipStream_t s);
void launch_upsample_bwd(const void* dout, void* din, int n, int h, int w,
                         int c, int scale, hipStream_t s);

// elementwise.hip -- the int launchers return grid.x (= rows of scratch).
void launch_act_fwd(const void* x, void* y, long n, int act, float slope,
                    hipStream_t s);
void launch_act_bwd(const void* dy, const void* y, void* dx, long n, int act,
                    float slope, hipStream_t s);
int launch_act_bwd_bias(const void* dy, const void* y, void* dx,
                        float* scratch, long m, int n, int act, float slope,
                        hipStream_t s);
int launch_col_sum_part(const void* a, float* scratch, long m, int n,
                        hipStream_t s);
// out[n] = column sums of scratch[gx][n]
void launch_col_sum_sum2(const float* scratch, int gx, int n, float* out,
                         hipStream_t s);
void launch_col_sum(const void* a, float* out, long m, int n, hipStream_t s);
void launch_bce_fwd(const void* logits, const void* labels, float* loss_sum,
                    long n, hipStream_t s);
void launch_bce_bwd(const void* logits, const void* labels, void* dlogits,
                    float gscale, long n, hipStream_t s);
// probs is fp32 [rows][cols] (the backward subtracts the target from it);
// logits, onehot and dlogits are bf16.
void launch_softmax_xent_fwd(const void* logits, const void* onehot,
                             float* loss_sum, void* probs, int rows, int cols,
                             hipStream_t s);
void launch_softmax_xent_bwd(const void* probs, const void* onehot,
                             void* dlogits, float gscale, long n,
                             hipStream_t s);

// dropout.hip -- state is the device int64[2] {seed, calls}; mask is one
// byte per 8-element vector; thresh = round(keep * 65536).
int dropout_grid_cap();
int dropout_block_size();
void launch_dropout_fwd(const void* x, void* y, void* mask,
                        const void* state, long n, unsigned int thresh,
                        float scale, hipStream_t s);
void launch_dropout_bwd(const void* dy, const void* mask, void* dx, long n,
                        float scale, hipStream_t s);
void launch_gaussian_noise_fwd(const void* x, void* y, const void* state,
                               long n, float stddev, hipStream_t s);

// batchnorm.hip -- x is [m][c]; the int launchers return grid.x = gx, the
// rows written of scratch[gx][2c] / bias_part[gx][c].
void launch_bn_stats(const void* x, long m, int c, float* sum, float* sumsq,
                     hipStream_t s);
int launch_bn_stats_part(const void* x, long m, int c, float* scratch,
                         hipStream_t s);
void launch_bn_stats_sum2(const float* scratch, int gx, int c, float* sum,
                          float* sumsq, hipStream_t s);
void launch_bn_finalize(const float* sum, const float* sumsq, long m, int c,
                        float eps, float momentum, float* mean, float* istd,
                        float* running_mean, float* running_var,
                        hipStream_t s);
void launch_bn_apply(const void* x, void* y, long m, int c, const float* mean,
                     const float* istd, const float* gamma, const float* beta,
                     hipStream_t s);
void launch_bn_apply_eval(const void* x, void* y, long m, int c,
                          const float* rm, const float* rv, const float* gamma,
                          const float* beta, float eps, hipStream_t s);
void launch_bn_bwd_reduce(const void* x, const void* dy, long m, int c,
                          const float* mean, const float* istd, float* dgamma,
                          float* dbeta, hipStream_t s);
int launch_bn_bwd_reduce_part(const void* x, const void* dy, long m, int c,
                              const float* mean, const float* istd,
                              float* scratch, hipStream_t s);
void launch_bn_bwd_sum2(const float* scratch, int gx, int c, float* dgamma,
                        float* dbeta, hipStream_t s);
void launch_bn_bwd_apply(const void* x, const void* dy, void* dx, long m,
                         int c, const float* mean, const float* istd,
                         const float* gamma, const float* dgamma,
                         const float* dbeta, hipStream_t s);
int launch_bn_bwd_apply_act(const void* x, const void* dy, void* dx, long m,
                            int c, const float* mean, const float* istd,
                            const float* gamma, const float* dgamma,
                            const float* dbeta, int act, float slope,
                            float* bias_part, hipStream_t s);

// optim.hip -- t_dev: optional on-device int32 step count (else t is used).
void launch_fused_adam(void* param, const void* grad, float* master, float* m,
                       float* v, long n, int grad_is_bf16, int param_is_bf16,
                       float lr, float b1, float b2, float eps, float clip,
                       float l2, int t, const int* t_dev, hipStream_t s);
void launch_fused_rmsprop(void* param, const void* grad, float* master,
                          float* v, long n, int grad_is_bf16,
                          int param_is_bf16, float lr, float decay, float eps,
                          float clip, float l2, hipStream_t s);

}  // extern "C"
