/* mi355seg.h — C-ABI of libmi355seg.so (MI355X / gfx950 only).
 *
 * The reference (taintpro98/rnd-semantic-segmentation) has no FFI: its hot path is
 * Python calling torch ops.  This header DEFINES the boundary underneath the
 * reference's Python class surface.  Every entry point names the
 * reference call it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *  - plain pointers + sizes, no torch types.  All pointers are DEVICE pointers
 *    unless a parameter says "host".  The caller owns every buffer, including
 *    workspaces (query sizes with the *_workspace functions).
 *  - activations are NHWC ("channels_last") bf16: x[b][h][w][c]; a GEMM row m is
 *    the pixel (b,h,w).  Logits / losses / gradients of parameters are fp32.
 *  - master weights are fp32 in torch's OIHW layout; kernels consume bf16 packed
 *    copies produced by mi_pack_*.
 *  - every function enqueues on `stream` (a hipStream_t passed as void*) and
 *    never synchronises, allocates or frees: safe under HIP graph capture.
 *  - return 0 on success, a negative MI_E* code otherwise; mi_last_error()
 *    returns a thread-local message.  Nothing throws.  Re-entrant.
 */
#ifndef MI355SEG_H
#define MI355SEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355SEG_VERSION 100

#define MI_OK 0
#define MI_EINVAL (-22)   /* bad shape / alignment / null pointer */
#define MI_ENOMEM (-12)   /* workspace too small */
#define MI_EHIP (-5)      /* HIP launch error */

/* epilogue flags of mi_conv_gemm (applied in this order on the fp32 accumulator) */
#define MI_EPI_SCALE_BIAS 1  /* v = v*scale[n] + bias[n]      FrozenBatchNorm2d, reference core/components/layers.py:18-23 */
#define MI_EPI_RESIDUAL 2    /* v += res[m][n]                 `out += identity`, reference core/components/resnet.py:110 */
#define MI_EPI_RELU 4        /* v = max(v,0)                   resnet.py:95,99,111 */
#define MI_EPI_MASK 8        /* v = msk[m][n] > 0 ? v : 0      ReLU backward of the producer of msk */
#define MI_EPI_OUT_F32 16    /* store fp32 instead of bf16 */
#define MI_EPI_ZSPLIT 32     /* fp32 store to [n/zgw][M][zgw] (ASPP tap planes) */
#define MI_EPI_WRITE_MASK 64 /* also store sign bits of the result: bit n%16 of uint16 mask_out[m][n/16] = (v > 0)   (N % 16 == 0) */
#define MI_EPI_LEAKY 256     /* with MI_EPI_RELU: LeakyReLU(alpha); with MI_EPI_BITMASK: its backward (v *= alpha where the bit is 0) */
#define MI_EPI_STATS 512     /* (mi_conv_gemm_stats only) plain bf16 store + per-tile sums of (out - pilot), (out - pilot)^2 per channel */
#define MI_EPI_BITMASK 128   /* like MI_EPI_MASK but `msk` points at such packed bits: 1/16 of the bytes of the bf16 tensor */

/* gather modes */
#define MI_GATHER_FWD 0      /* src = out*stride + tap*dil - pad            (forward conv, wgrad) */
#define MI_GATHER_DGRAD 1    /* src = (out + pad - tap*dil)/stride if exact (data gradient)       */

int mi_version(void);
const char* mi_last_error(void);

/* ---- weight packing (fp32 OIHW master -> bf16 GEMM operand) ------------------------------- */
/* wp[t][o][i] = bf16(w[o][i][t]),  t = ky*k+kx.  Operand of the forward conv. */
int mi_pack_weight_fwd(const float* w_oihw, void* wp_bf16, int O, int I, int ksize, void* stream);
/* wp[t][i][o] = bf16(w[o][i][t] * (scale ? scale[o] : 1)).  Operand of the data gradient; the
 * FrozenBN scale of the conv's output channel is folded in (scale is a constant buffer). */
int mi_pack_weight_dgrad(const float* w_oihw, const float* scale_o, void* wp_bf16, int O, int I, int ksize, void* stream);

/* Every conv weight of a module in one launch.  table (device, int64[n_desc][8]) rows:
 * {w_off, scale_off or -1, wp_off, wpt_off or -1 (skip the dgrad pack), O, I, k*k, first_block}; offsets in elements
 * into wflat / sflat / wp / wpt; a block packs 32 output x 128 input channels, total_blocks = sum ceil(O/32) * ceil(I/128); k*k <= 9. */
int mi_pack_weights_multi(const float* wflat, const float* sflat, void* wp_bf16, void* wpt_bf16,
                          const int64_t* table_dev, int n_desc, int total_blocks, void* stream);

/* ---- implicit-GEMM convolution, MFMA bf16 -> fp32 accumulate ----------------------------------
 * Replaces nn.Conv2d forward and the data-gradient half of convolution_backward for every
 * conv of reference core/components/resnet.py:22-30 (conv3x3 with dilation, conv1x1) and, through
 * the fused epilogue, the FrozenBN / ReLU / residual that follow it (resnet.py:93-113).
 *   out[b][ho][wo][n] = epi( sum_{t,c} a[b][src_h(ho,t)][src_w(wo,t)][c] * wp[t][n][c] )
 * a: [B][Ha][Wa][Ca] bf16, wp: [k*k][N][Ca] bf16, out: [B][Ho][Wo][N] bf16 (or fp32).
 * Requirements: Ca % 32 == 0 (Ca % 64 != 0: stride-1 / same-size launches without a residual or mask tile only - the 32-channel main loop), N % 8 == 0, 16-byte aligned pointers; N % 16 == 0 with MI_EPI_BITMASK / MI_EPI_WRITE_MASK
 * (one uint16 of sign bits per 16 channels), and when N % 128 == 0 those packed-bit tensors must be 16-byte aligned too
 * (a tile row's 16 mask bytes move as one access).  Violations return MI_EINVAL. */
int mi_conv_gemm(const void* a, const void* wp, void* out,
                 int B, int Ha, int Wa, int Ca, int Ho, int Wo, int N,
                 int ksize, int stride, int pad, int dil, int gather_mode,
                 const float* scale, const float* bias, const void* res, const void* msk, void* mask_out,
                 int flags, int zgw, float alpha, void* stream);

/* The wide-tile main loop of mi_conv_gemm (csrc/igemm_pp.hip: 320|256 x 256 tile, 8 waves in two groups that alternate
 * between MFMA and LDS/DMA phases, 4-slot LDS ring) called explicitly.  Same contract and epilogue flags, restricted to
 * stride 1, Ha == Ho, Wa == Wo, Ca % 32 == 0.  mi_conv_gemm picks it by its own cost model; this entry point exists so that
 * the two main loops can be compared on one shape in one process.  mtg: 16-row MFMA tiles per wave (8 or 10 -> 256 or 320
 * tile rows), 0 = choose. */
/* which main loop mi_conv_gemm takes for a shape: 1 = igemm_pp_kernel (wide tile), 0 = igemm_nt_kernel (measurement tools): the `kernel` field of
 * mi_conv_gemm_plan for a padding of at most 32 rows.  A pure query: arguments mi_conv_gemm would refuse answer 0 and do not touch mi_last_error.  Since the
 * query became a view of the plan it answers 1 for every valid Ca % 64 != 0 launch (they run on igemm_pp_kernel whatever M is; the rule alone used to answer 0
 * for the small ones). */
int mi_conv_gemm_route(int B, int Ha, int Wa, int Ca, int Ho, int Wo, int N, int ksize, int stride, int flags);
/* The instantiation mi_conv_gemm / mi_conv_gemm_stats (pp_mtg = -1) or mi_conv_gemm_pp (pp_mtg = its mtg: 0, 8 or 10) launches for these arguments, from the
 * planning function the launches call, on the host (no GPU, no launch).  plan: int[MI_CPLAN_LEN] = {kernel (MI_CPLAN_*), tile height (igemm_nt_kernel: MT 4..6,
 * 32 * MT rows x 128 columns; igemm_pp_kernel: MTG 8 | 10, 32 * MTG rows x 256 columns), unit-stride gather, prefetched residual rows, staged epilogue,
 * compile-time epilogue flag set (-1: the generic epilogue that reads `flags`), K order (igemm_pp_kernel: 1 = channel-chunk-major), row tiles, column tiles,
 * rounds of the grid on the workgroup slots the tile picker assumed, those slots}. */
#define MI_CPLAN_NT 0         /* igemm_nt_kernel<MT, UNIT, PREF, 64, EPI, 2, STG> */
#define MI_CPLAN_PP 1         /* igemm_pp_kernel<MTG, EPI> */
#define MI_CPLAN_LEN 11
int mi_conv_gemm_plan(int B, int Ha, int Wa, int Ca, int Ho, int Wo, int N, int ksize, int stride, int pad, int dil, int flags, int pp_mtg, int* plan);
int mi_conv_gemm_pp(const void* a, const void* wp, void* out,
                    int B, int Ha, int Wa, int Ca, int Ho, int Wo, int N,
                    int ksize, int stride, int pad, int dil, int gather_mode,
                    const float* scale, const float* bias, const void* res, const void* msk, void* mask_out,
                    int flags, int zgw, float alpha, int mtg, void* stream);

/* ---- two chained 1x1 convolutions of the bottleneck sequence in one launch (csrc/chain.hip) --------------------------
 * forward (backward = 0): reference core/components/resnet.py:105-113 of block i followed by :93-95 of block i+1,
 *   mid = relu(scale1 * (a . w_first^T) + shift1 + res)   [M][N1] bf16, sign bits -> bits1_out [M][N1/8]
 *   out = relu(scale2 * (mid . w_second^T) + shift2)      [M][N2] bf16, sign bits -> bits2_out [M][N2/8]
 * i.e. mi_conv_gemm(a, w_first, flags 1|2|4|64) then mi_conv_gemm(mid, w_second, flags 1|4|64), with `mid` written once and
 * never read back.  backward = 1: the data gradients of the same two convs in the order backward meets them (conv1 of block i,
 * conv3 of block i-1; weights packed by mi_pack_weight_dgrad),
 *   mid = ((a . w_first^T) + res) where bit of bits1 else 0;   out = (mid . w_second^T) where bit of bits2 else 0
 * i.e. flags 2|128 then 128.  a [M][K1], w_first [N1][K1], res / mid [M][N1], w_second [N2][N1], out [M][N2], all bf16 and
 * 16-byte aligned; the sign-bit tensors as MI_EPI_WRITE_MASK / MI_EPI_BITMASK define them.  Built for K1 = 256, N1 = 1024, N2 = 256
 * (layer3); other sizes return MI_EINVAL.  grid: workgroups (0 = one per CU). */
int mi_conv_chain(const void* a, const void* w_first, const void* res, void* mid, const void* w_second, void* out,
                  long M, int K1, int N1, int N2,
                  const float* scale1, const float* shift1, const float* scale2, const float* shift2,
                  const void* bits1, const void* bits2, void* bits1_out, void* bits2_out,
                  int backward, int grid, void* stream);

/* ---- weight gradient (contraction over pixels), split-K with deterministic reduction ------------
 * Replaces the weight-gradient half of convolution_backward.
 *   dw[o][i][t] (+)= scale[o] * sum_m dy[m][o] * x[src(m,t)][i]
 * dy: [B][Ho][Wo][O] bf16, x: [B][Ha][Wa][I] bf16, dw: fp32 OIHW.  O % 8 == 0, I % 8 == 0.
 * out_map 0: OIHW as above (ncls ignored).  out_map 1 (ASPP): ksize must be 1 and row o = (br*9+tap)*ncls+cls of the
 * [O][I] product (O >= 36*ncls, 36*ncls <= MI_ASPP_KPAD: the column layout mi_aspp_im2col writes) is scattered to
 * dw[br][cls][i][tap] of the 4 stacked [ncls][I][3][3] tensors.  dw_elems = number of floats dw points at; the call
 * fails with MI_EINVAL instead of writing past it. */
size_t mi_conv_wgrad_workspace(int B, int Ho, int Wo, int O, int I, int ksize);
/* which kernel mi_conv_wgrad launches for a shape (measurement tools): 0 wgrad_tn_kernel (128 x 128 tile per tap), 1 wgrad_tn256_kernel
 * (opt-in), 2 wgrad_p3_kernel (opt-in), 3 wgrad_q3_kernel (3x3 stride 1: the three taps of a kernel row fused, 64 x 128 tile),
 * 4 wgrad_s4_kernel (1x1 stride 1: 32-pixel stages, three in flight) */
int mi_conv_wgrad_route(int B, int Ha, int Wa, int I, int Ho, int Wo, int O, int ksize, int stride, int pad, int dil, int out_map);
/* The launch mi_conv_wgrad (deferred = 0) or mi_conv_wgrad_partial (deferred = 1) makes for these arguments with a workspace of mi_conv_wgrad_workspace bytes,
 * from the planning function the launches call, on the host.  plan: int[MI_WPLAN_LEN] = {kernel (MI_WPLAN_*: mi_conv_wgrad_route's numbers), addressing mode
 * (wgrad_tn_kernel<MODE>: 0 general gather, 1 unit stride, 2 pointwise; wgrad_tn256_kernel<MODE>: 1 | 2; else 0), K splits S, K steps per split (q3: slabs of
 * 64 padded pixels), pixels per K step, o tiles, i tiles, deferred}. */
#define MI_WPLAN_TN 0
#define MI_WPLAN_TN256 1
#define MI_WPLAN_P3 2         /* experiment builds only */
#define MI_WPLAN_Q3 3
#define MI_WPLAN_S4 4
#define MI_WPLAN_LEN 8
int mi_conv_wgrad_plan(int B, int Ha, int Wa, int I, int Ho, int Wo, int O, int ksize, int stride, int pad, int dil, int out_map, int deferred, int* plan);
int mi_conv_wgrad(const void* dy, const void* x, float* dw,
                  int B, int Ha, int Wa, int I, int Ho, int Wo, int O,
                  int ksize, int stride, int pad, int dil,
                  const float* scale_o, int accumulate, int out_map, int ncls, size_t dw_elems,
                  void* workspace, size_t workspace_bytes, void* stream);

/* mi_conv_wgrad in two parts (round 5): _partial runs the main kernel only - the split-K slabs stay in `workspace`, which the caller keeps alive and
 * untouched until the reduction - and writes the reducer's arguments to `job` (mi_conv_wgrad_job_bytes() bytes of host memory); mi_conv_wgrad_reduce runs
 * the reducers of up to 8 consecutive job records as ONE launch (the three weight gradients of a bottleneck: one launch instead of three on the
 * weight-gradient stream).  Same fixed summation order per conv, hence the same bits as mi_conv_wgrad - with one exception: this form is the one that runs
 * BESIDE a data-gradient chain, and the fused-row 3x3 route plans its K split for that (448 instead of 512 workgroup slots, MI_WGRAD_Q3_SLOTS_BESIDE:
 * fewer, longer splits = another partition of the fp32 sums; deterministic, and within fp32 rounding of the one-call result). */
size_t mi_conv_wgrad_job_bytes(void);
int mi_conv_wgrad_partial(const void* dy, const void* x, float* dw,
                          int B, int Ha, int Wa, int I, int Ho, int Wo, int O,
                          int ksize, int stride, int pad, int dil,
                          const float* scale_o, int accumulate, int out_map, int ncls, size_t dw_elems,
                          void* workspace, size_t workspace_bytes, void* job, void* stream);
int mi_conv_wgrad_reduce(const void* jobs, int n, void* stream);

/* ---- ASPP head (reference core/models/classifiers/aspp/classifier.py:6-32) ---------------------
 * forward:  Z = X * Wall^T as ONE plain GEMM (mi_conv_gemm, ksize 1, MI_EPI_ZSPLIT, zgw 20) over all
 * 4 rates x 9 taps x 19 classes, then mi_aspp_col2im sums the 36 shifted planes (+ the 4 biases):
 *   low[b][h][w][n] = sum_r bias[r][n] + sum_{r,ky,kx} Z[r*9+ky*3+kx][b][h+(ky-1)d_r][w+(kx-1)d_r][n]
 * which is exactly out = conv_0(x); out += conv_i(x) (classifier.py:27-29) re-associated.
 * backward: mi_aspp_im2col builds G[m][(r*9+t)*19+n] = dlow[m - shift][n]; then dX = G * Wall (mi_conv_gemm),
 * dWall = G^T X (mi_conv_wgrad, out_map 1), dbias = column sums of dlow. */
#define MI_ASPP_NRATES 4
#define MI_ASPP_ZGW 20          /* classes padded 19 -> 20 per tap plane */
#define MI_ASPP_KPAD 704        /* 36*19 = 684 padded to a multiple of 64 */
/* wall[(g*20+n)][c] = bf16(w[r][n][c][tap]), g = r*9+tap; row n==19 of each plane is zero.  [720][C] */
int mi_aspp_pack_fwd(const float* w4 /*[4][K][C][3][3]*/, void* wall_bf16, int C, int K, void* stream);
/* wallT[c][g*K+n] = bf16(w[r][n][c][tap]); columns >= 36*K are zero.  [C][704] */
int mi_aspp_pack_dgrad(const float* w4, void* wallT_bf16, int C, int K, void* stream);
int mi_aspp_col2im(const float* z /*[36][M][20]*/, const float* bias4 /*[4][K]*/, float* low /*[B][H][W][K]*/,
                   int B, int H, int W, int K, const int* rates4 /*host*/, void* stream);
/* g[m][k] bf16, k = (r*9+t)*K+n, columns >= 36*K zero */
int mi_aspp_im2col(const float* dlow /*[B][H][W][K]*/, void* g_bf16 /*[M][704]*/,
                   int B, int H, int W, int K, const int* rates4 /*host*/, void* stream);
/* dbias4[r][n] (+)= sum_m dlow[m][n], r = 0..3 (every branch sees the same gradient); two-level fixed-order column sum,
 * workspace >= mi_colsum_workspace(M, K) bytes (csrc/colsum.hip) */
size_t mi_colsum_workspace(int M, int N);
int mi_aspp_bias_grad(const float* dlow, float* dbias4 /*[4][K]*/, int M, int K, int accumulate,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- bilinear upsample, align_corners=True (classifier.py:31, core/utils/utility.py:185) --------
 * low: [B][h][w][K] fp32 NHWC, up: [B][K][H][W] fp32 NCHW (the layout the reference returns). */
int mi_upsample_ac_fwd(const float* low, float* up, int B, int h, int w, int K, int H, int W, void* stream);
int mi_upsample_ac_bwd(const float* dup, float* dlow, int B, int h, int w, int K, int H, int W, void* stream);

/* ---- per-pixel softmax cross-entropy, ignore_index (core/trainers/aspp_trainer.py:61,91) --------
 * logits [B][K][H][W] fp32 NCHW, labels [B][H][W] int64.  loss_out is FOUR floats: [0] = mean over valid pixels
 * (nan if none), [1] = number of valid pixels, [2] = number of labels outside [0,K) that are not ignore_index (torch
 * raises a device assert for those; here they are left out of the loss and reported - a non-zero count means the
 * label map is wrong), [3] = scratch.  workspace: mi_ce_workspace bytes. */
size_t mi_ce_workspace(int B, int H, int W);
int mi_softmax_ce_fwd(const float* logits, const int64_t* labels, float* loss_out /*[4]*/,
                      int B, int K, int H, int W, int ignore_index, void* workspace, size_t workspace_bytes, void* stream);
/* dlogits = (softmax - onehot) * valid / n_valid * grad_scale, n_valid read from loss_out[1] on device */
int mi_softmax_ce_bwd(const float* logits, const int64_t* labels, const float* loss_out, float* dlogits,
                      int B, int K, int H, int W, int ignore_index, float grad_scale, void* stream);

/* ---- fused upsample + cross-entropy: never materialises the [B][K][H][W] tensor (training path) --
 * classifier(feat, size) + CrossEntropyLoss of reference aspp_trainer.py:89-91 in one call.
 * low [B][h][w][K] fp32 NHWC, labels [B][H][W] int64 (H >= h, W >= w, K <= 32).
 * loss_out (four floats, as mi_softmax_ce_fwd): [0] = mean loss over valid pixels, [1] = n_valid, [2] = out-of-range labels.
 * dlow (may be NULL: loss only) [B][h][w][K] = d loss / d low * grad_scale, already divided by n_valid.
 * Deterministic (fixed summation order, no atomics). */
size_t mi_upsample_ce_workspace(int B, int h, int w, int K, int H, int W);
int mi_upsample_ce(const float* low, const int64_t* labels, float* loss_out /*[4]*/, float* dlow,
                   int B, int h, int w, int K, int H, int W, int ignore_index, float grad_scale,
                   void* workspace, size_t workspace_bytes, void* stream);

/* The same with either bilinear convention: align_corners != 0 as above; 0: F.interpolate(..., size=, mode="bilinear") at its default
 * align_corners=False (source index max(in / out * (dst + 0.5) - 0.5, 0)) - the four deep-supervision heads of the GALD path
 * (core/models/classifiers/gcpacc/gcpa_cc2.py:78-81 + core/trainers/gald_trainer.py:66-84). */
int mi_upsample_ce_ex(const float* low, const int64_t* labels, float* loss_out /*[4]*/, float* dlow,
                      int B, int h, int w, int K, int H, int W, int ignore_index, float grad_scale, int align_corners,
                      void* workspace, size_t workspace_bytes, void* stream);

/* The same with torch.nn.CrossEntropyLoss's two other arguments, weight= (one factor per class) and label_smoothing=.  With z = bilinear(low),
 * p = softmax(z), y = label, valid = label not ignore_index and inside [0, K), s = label_smoothing, Wsum = sum_c w_c:
 *   S    = sum_valid w_y
 *   loss = [ (1-s) sum_valid w_y (-log p_y) + s/K sum_valid sum_c w_c (-log p_c) ] / S
 *   d loss / d z_k = valid [ (1-s) w_y (p_k - [k==y]) + s/K (p_k Wsum - w_k) ] / S
 * (the smoothing term counts every valid pixel, also one whose own class has weight 0; S == 0 gives a nan loss, as torch does).
 * class_weights: [K] fp32 in DEVICE memory, read on every call (a captured graph sees later values), or NULL = all 1.  0 <= label_smoothing <= 1.
 * loss_out: [0] = loss, [1] = S, [2] = out-of-range labels, [3] = scratch.  dlow may be NULL (loss only, same loss bits); an entry of dlow that
 * no valid pixel touches is exactly 0, also when S == 0.  Workspace, restrictions, launch count and determinism as mi_upsample_ce_ex; with
 * class_weights == NULL and label_smoothing == 0 the results are those of mi_upsample_ce_ex bit for bit. */
int mi_upsample_ce_w(const float* low, const int64_t* labels, const float* class_weights /*[K]*/, float* loss_out /*[4]*/, float* dlow,
                     int B, int h, int w, int K, int H, int W, int ignore_index, float label_smoothing, float grad_scale, int align_corners,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Focal loss (Lin et al., 2017) in the same head: FL = -w_y (1 - p_y)^gamma log p_y, the smooth counterpart of OHEM.  Operands, restrictions,
 * workspace (mi_upsample_ce_workspace), launch count and determinism as mi_upsample_ce_w.  With q = p_y, u = 1 - q, nll = -log q:
 *   S    = sum_valid w_y
 *   loss = sum_valid w_y u^gamma nll / S                                   (S == 0: nan)
 *   m    = u^gamma (1 + gamma q nll / u)                                   (nll / u taken as 1 where u == 0)
 *   d loss / d z_k = valid w_y m (p_k - [k==y]) / S
 * u is formed as the sum of the other classes' exponentials over the sum of all, so it keeps its relative precision on confident pixels, and the
 * gradient never forms u^(gamma-1): it is finite for every gamma in range.  0 <= gamma <= 8, finite.  gamma == 0 runs what mi_upsample_ce_w runs
 * at label_smoothing 0 and gives its bits (with class_weights == NULL those of mi_upsample_ce_ex).  There is no label smoothing here.
 * class_weights: [K] fp32 in DEVICE memory, read on every call, or NULL = all 1.  loss_out: [0] = loss, [1] = S, [2] = out-of-range labels,
 * [3] = scratch.  dlow may be NULL (loss only, same loss bits); an entry of dlow that no valid pixel touches is exactly 0, also when S == 0. */
int mi_upsample_ce_focal(const float* low, const int64_t* labels, const float* class_weights /*[K]*/, float* loss_out /*[4]*/, float* dlow,
                         int B, int h, int w, int K, int H, int W, int ignore_index, float gamma, float grad_scale, int align_corners,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- fused upsample + cross-entropy with online hard example mining (OHEM: the OhemCrossEntropy2d criterion GALDNet, CCNet, OCNet and HRNet-Seg
 * were published with) ----
 * Operands and restrictions as mi_upsample_ce_ex, and B H W < 2^24.  With z = bilinear(low) in either convention, p = softmax(z), y = label,
 * valid = label not ignore_index and inside [0, K), q_i = p_i[y_i] on valid pixels and n their count:
 *   k      = min(min_kept, n)                                       (min_kept >= 1)
 *   t      = max(thresh, k-th smallest q over the valid pixels)     (1-based; n == 0: t = thresh; 0 <= thresh <= 1)
 *   kept_i = valid_i and q_i <= t                                   (ties at t are all kept, so at least k pixels are kept)
 *   loss   = sum_kept (-log q_i) / n_kept                           (n_kept == 0, i.e. n == 0: nan, as the other heads)
 *   d loss / d z_c at pixel i = kept_i (p_i[c] - [c == y_i]) / n_kept;  d loss / d low = transposed bilinear of that, times grad_scale
 * The kept set is a constant of the backward pass: nothing differentiates through t.  min_kept counts full-resolution pixels of this one call
 * (one head, one batch, one rank).  min_kept >= n gives the plain cross-entropy over the valid pixels.
 * loss_out: [0] = loss, [1] = n_kept (an integer count, exact as a float below 2^24), [2] = out-of-range labels (left out and counted),
 * [3] = the threshold t that was used.  dlow may be NULL (loss only, same loss bits); an entry of dlow that no kept pixel touches is exactly 0,
 * also when n == 0.  prob (may be NULL): [B][H][W] fp32, receives q of every full-resolution pixel, 2.0 where the pixel is not valid.
 * t is the exact order statistic of the fp32 q the kernel computed (a three-level radix select on their bit patterns, histograms merged with
 * integer atomics); the pixels that receive gradient are exactly the n_kept that were counted, because both decisions read the same stored q.
 * No floating-point atomic, every sum in a fixed order: two calls give the same bits.  Nothing is read back between the launches (one memset,
 * 8 kernels for the loss, 2 more for dlow, one device copy for prob), so the call can be captured in a HIP graph; a replay reads low and
 * labels anew.  Refused before any launch: what mi_upsample_ce_ex refuses, B H W >= 2^24, thresh outside [0, 1], min_kept < 1, a short
 * workspace (MI_ENOMEM). */
size_t mi_upsample_ce_ohem_workspace(int B, int h, int w, int K, int H, int W);
int mi_upsample_ce_ohem(const float* low, const int64_t* labels, float* loss_out /*[4]*/, float* dlow, float* prob /*[B][H][W]*/,
                        int B, int h, int w, int K, int H, int W, int ignore_index, float thresh, int64_t min_kept, float grad_scale,
                        int align_corners, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fused upsample + generalized Dice loss (GeneralizedDiceLoss, reference core/utils/utility.py:399-447, label form) ----
 * Operands and restrictions as mi_upsample_ce_ex.  With p = softmax(bilinear(low)) and t = onehot(labels), both zero where the label is
 * ignore_index:  T_c = sum t, I_c = sum p t, P2_c = sum p^2, w_c = 1 / (T_c^2 + eps) | 1 / (T_c + eps) | 1 / (sqrt(T_c) + eps) by weight_type,
 * loss = 1 - 2 sum_c w_c I_c / (sum_c w_c (P2_c + T_c) + eps).  Labels outside [0, K) that are not ignore_index are left out and counted.
 * loss_out (four floats): [0] = loss, [1] = valid pixels, [2] = out-of-range labels, [3] = 0.
 * dlow (may be NULL: loss only) [B][h][w][K] = d loss / d low * grad_scale.  sums (may be NULL) [3K] fp32: T_c, I_c, P2_c (T_c exact below 2^24).
 * Launches: a reduction pass, a one-workgroup finalize that leaves the loss and the gradient's 2K coefficients in device memory, and - with dlow -
 * the gradient pass (two launches, along x then y), which recomputes the softmax from `low`.  Nothing is read back in between: the call can be
 * captured in a HIP graph.  Deterministic (fixed summation order, no floating-point atomics, T_c counted in integers). */
#define MI_GDL_SQUARE 0
#define MI_GDL_IDENTITY 1
#define MI_GDL_SQRT 2
size_t mi_upsample_gdl_workspace(int B, int h, int w, int K, int H, int W);
int mi_upsample_gdl(const float* low, const int64_t* labels, float* loss_out /*[4]*/, float* dlow, float* sums /*[3K]*/,
                    int B, int h, int w, int K, int H, int W, int ignore_index, int weight_type, float eps, float grad_scale,
                    int align_corners, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fused upsample + Lovasz-Softmax (Berman, Triki, Blaschko, CVPR 2018; classes = 'present', over the whole batch) on a 1024-cell order ----
 * Operands and restrictions as mi_upsample_ce_ex; bins must be 1024 and B H W < 2^31.  With p = softmax(bilinear(low)) and valid = label is not
 * ignore_index and lies in [0, K) (other labels are left out and counted), for every class c over the valid pixels i:
 *   e_i = 1 - p_i[c] where y_i == c (foreground), p_i[c] elsewhere (background);  cell_i = min(bins - 1, floor(e_i * bins))
 *   F[b], N[b] = foreground / background pixels in cell b;  G = sum_b F[b];  a_b, n_b = foreground / background pixels in strictly higher cells
 *   g_fg[b] = 1 / (G + n_b),  g_bg[b] = (G - a_b - F[b]) / ((G + n_b) (G + n_b + N[b]))
 *   loss_c = sum_i e_i g[cell_i];  loss = mean of loss_c over the classes with G > 0 (none, i.e. no valid pixel: nan, as the other heads)
 * This is the Lovasz gradient of the order "descending cell; inside a cell the foreground pixels first, then the background pixels with their Jaccard
 * increments averaged" - a subgradient of the Lovasz extension, so per class 0 <= exact (sorted) loss - loss_c <= 1 / bins.
 *   d loss / d z_k = p_k (s_k - sum_c s_c p_c),  s_c = -g_fg[cell] / C (foreground), +g_bg[cell] / C (background), 0 for a class that is not present,
 * C = number of present classes; the order is a constant of the backward pass.  d loss / d low = transposed bilinear of that, times grad_scale.
 * loss_out: [0] = loss, [1] = valid pixels, [2] = out-of-range labels, [3] = C.  dlow may be NULL (loss only, same loss bits); an entry of dlow
 * that no valid pixel touches is exactly 0.  hist (may be NULL) [K][bins][2] receives F and N, exact integers.  err (may be NULL; for tests and
 * diagnosis, never in training) [B][K][H][W] fp32 receives the kernel's own e of every (pixel, class), 2.0 where the pixel is not valid; the
 * foreground error is (sum of the other classes' exponentials) / (sum of all), not 1 - p.  Every pass forms e with the same device function, so
 * the cells the gradient looks up are the cells that were counted, and they are floor(err * 1024) exactly.
 * Launches: one memset, a counting pass (integer atomics only), a scan with one workgroup per class (coefficients formed in fp64), the loss /
 * x-gradient pass, a one-workgroup loss finalize, with dlow the y-gradient pass, with hist one device copy.  No floating-point atomic, every sum
 * in a fixed order: two calls give the same bits.  Nothing is read back in between, so the call can be captured in a HIP graph; a replay reads
 * low and labels anew.  Refused before any launch: what mi_upsample_ce_ex refuses, bins != 1024, B H W >= 2^31, a grad_scale that is not finite,
 * a short workspace (MI_ENOMEM). */
size_t mi_upsample_lovasz_workspace(int B, int h, int w, int K, int H, int W);
int mi_upsample_lovasz(const float* low, const int64_t* labels, float* loss_out /*[4]*/, float* dlow, uint32_t* hist /*[K][bins][2], may be NULL*/,
                       float* err /*[B][K][H][W], may be NULL*/, int B, int h, int w, int K, int H, int W, int ignore_index, int bins,
                       float grad_scale, int align_corners, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fused upsample + Tversky + binary cross-entropy (TverskyLoss / BinaryCrossEntropyLoss / CompoundLoss, reference
 * core/models/classifiers/attn/loss.py:7-27, 42-74) for one-channel logits ----
 * low [B][h][w] fp32 logits, mask [B][H][W] fp32 in [0, 1] (may be soft), H >= h, W >= w, either bilinear convention; h == H, w == W is the identity.
 * With z = bilinear(low), p = sigmoid(z), N = B H W:  TP = sum p y, FN = sum y (1 - p), FP = sum p (1 - y) over the whole batch,
 * tversky = 1 - (TP + eps) / (TP + alpha FN + (1 - alpha) FP + eps), bce = 1/N sum [max(z, 0) - z y + log1p(exp(-|z|))],
 * loss = w_tversky tversky + w_bce bce.  0 <= alpha <= 1, eps > 0.
 * loss_out (four floats): [0] = loss, [1] = tversky, [2] = bce, [3] = 0.  sums (may be NULL) [3] fp32: TP, FN, FP.
 * dlow (may be NULL: loss only, same loss bits) [B][h][w] = d loss / d low * grad_scale.
 * Launches: a reduction pass, a one-workgroup finalize that leaves the loss and the gradient's three coefficients in device memory, and - with dlow -
 * the gradient pass (two launches, along x then y), which recomputes z from `low`.  Nothing is read back in between: the call can be captured in a
 * HIP graph.  Deterministic (fixed summation order, no floating-point atomics). */
size_t mi_upsample_tversky_bce_workspace(int B, int h, int w, int H, int W);
int mi_upsample_tversky_bce(const float* low, const float* mask, float* loss_out /*[4]*/, float* dlow, float* sums /*[3]*/,
                            int B, int h, int w, int H, int W, float alpha, float eps, float w_tversky, float w_bce, float grad_scale,
                            int align_corners, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the same head with the boundary loss of Kervadec et al. (MIDL 2019; not in the reference) as a third term ----
 * phi [B][H][W] fp32: the signed distance map of the label (mi_signed_distance).  With S = sum p phi over the batch and N = B H W:
 * boundary = S / N, loss = w_tversky tversky + w_bce bce + w_boundary boundary, d loss / d z gains (w_boundary / N) phi p (1 - p).
 * w_boundary >= 0 and finite.  loss_out[3] = boundary (0 when w_boundary is 0: the term is off); sums (may be NULL) [4] fp32: TP, FN, FP, S.  Everything else - operands, launches, the fixed
 * summation orders (one more partial per workgroup, one more coefficient in device memory), capturability - as mi_upsample_tversky_bce, whose kernels
 * these are in another mode; one more 4-byte load per pixel in the reduction and in the gradient pass.  Refused before any launch: what
 * mi_upsample_tversky_bce refuses, a NULL phi, a negative or non-finite w_boundary. */
size_t mi_upsample_tversky_bce_sdf_workspace(int B, int h, int w, int H, int W);
int mi_upsample_tversky_bce_sdf(const float* low, const float* mask, const float* phi, float* loss_out /*[4]*/, float* dlow,
                                float* sums /*[4], may be NULL: TP, FN, FP, sum p*phi*/, int B, int h, int w, int H, int W, float alpha, float eps,
                                float w_tversky, float w_bce, float w_boundary, float grad_scale, int align_corners, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ---- inference tail: upsample to label size + softmax over classes (utility.py:185-186) ---------
 * probs [B][K][H][W] fp32; pred (optional, may be NULL) [B][H][W] uint8 argmax (first max wins). */
int mi_upsample_softmax(const float* low, float* probs, uint8_t* pred, int B, int h, int w, int K, int H, int W, void* stream);

/* ---- multi-scale, flip-averaged inference tail (multi_scale_inference, utility.py:193-209) in one kernel ---------
 * probs [K][H][W] fp32 = ((p_0 + p_1 + ... + p_{n-1}) / div_a) / div_b, where p_i = softmax_k(bilinear_align_corners(low_i -> H x W)),
 * read at column W-1-x when src[i].mirror is set (the reference's pred.flip(3)).  src is a HOST array of n sources, 1 <= n <= 16, copied by
 * value into the kernel arguments (no device table, no extra copy); each low is one image's [h][w][K] fp32 NHWC logits; K <= 32.
 * Arithmetic contract (the reference adds materialised fp32 tensors):
 *  - every p_i[k] is a rounded fp32 product before it is added: no fused multiply-add between the softmax and the sum;
 *  - the sum runs left to right in source order; the two divisions are true divisions in that order (output / len(scales) / 2);
 *    div_b == 1 skips the second;
 *  - a mirrored source is evaluated AT output column W-1-x with the same source-index arithmetic as an unmirrored one (not through an
 *    algebraically mirrored coordinate, which rounds differently);
 *  - the per-source interpolation + softmax is the device code of mi_upsample_softmax: n = 1, mirror = 0, div_a = div_b = 1 is bit-equal to it.
 * The only mandatory traffic is the one write of K*H*W*4 bytes (two floats per lane when W is even and probs is 8-byte aligned). */
typedef struct { const float* low; int h, w; int mirror; } MiProbSource;
int mi_upsample_softmax_multi(const MiProbSource* src, int n, float* probs, int K, int H, int W, float div_a, float div_b, void* stream);

/* ---- evaluation tail without the probability map: masks, pseudo-labels and scores in one kernel ---------
 * Per output pixel the K fp32 values are exactly those mi_upsample_softmax_multi writes (one shared device function; same sources, divisors
 * and arithmetic contract; n = 1, div_a = div_b = 1 is the single-scale tail).  Instead of storing them the kernel writes
 *   pred   [H][W] uint8: the LOWEST class index among their maxima (torch.max(dim) / numpy.argmax of the probability map - not the argmax of
 *          the logits: exp and the products can round two different logits to one probability);
 *   pseudo [H][W] uint8 or NULL: max >= threshold ? pred : 255;
 * and, when labels [H][W] int64 is given, ADDS to counts (int64, K*K + 3K cells, zeroed by the caller; two launches into one buffer add up)
 * the integers host/metrics.py derives from pred:
 *   counts[gt*K + pd]          confusion matrix, label gt != 255 and 0 <= gt < K            (confusion_matrix)
 *   counts[K*K + k]            area_intersection: pred == label == k, label != ignore_index (intersectionAndUnionGPU)
 *   counts[K*K + K + k]        area_output: pred == k where label != ignore_index
 *   counts[K*K + 2K + k]       area_target: label == k
 * The counts never depend on threshold.  Counting runs in a per-workgroup LDS table of 32-bit counters (a workgroup sees at most 512 pixels),
 * flushed with one 64-bit global atomic add per non-zero cell: integer sums, bit-reproducible.
 * Refused before launch: n outside 1..16, K outside 1..32, NULL pred, labels without counts or counts without labels, ignore_index inside
 * [0, K), threshold outside [0, 1], a zero divisor. */
int mi_upsample_predict_score(const MiProbSource* src, int n, int K, int H, int W, float div_a, float div_b, const int64_t* labels,
                              int ignore_index, float threshold, uint8_t* pred, uint8_t* pseudo, int64_t* counts, void* stream);

/* ---- the same tail with class-wise pseudo-label thresholds and the per-class confidence histogram they are taken from ---------
 * One kernel body with mi_upsample_predict_score (the extras are compiled out of that entry): the per-pixel values, pred, counts, the vector
 * paths and their alignment rules are those above.  What differs:
 *   class_threshold  HOST array of K floats or NULL, copied by value into the kernel arguments (as src is; no device table, no extra copy);
 *   pseudo [H][W] uint8 or NULL: max >= class_threshold[pred] ? pred : 255   (the same comparison; needs class_threshold);
 *   hist   DEVICE int64 [K][bins] or NULL, ADDED to (zeroed by the caller once per data set; launches into one buffer add up):
 *          hist[pred*bins + min(bins-1, int(max*bins))] += 1 for EVERY output pixel, whatever its label.  bins must be 1024: a power-of-two
 *          scale and a truncation are exact in fp32, so the bin is a function of the fp32 maximum alone (host/metrics.py confidence_bin).
 * From hist the host takes one threshold per class (host/metrics.py class_thresholds: the class's own confidence quantile, capped); a second
 * launch with that table and hist = NULL writes the masks.  The thresholds are bin edges j/1024, so max >= t is bin >= j.
 * Histogram in the kernel: two rounds of in-wave aggregation (the lanes holding the first waiting lane's cell retire, one lane carries their
 * number), then a per-workgroup LDS table of 128 lines of 16 neighbouring bins (32-bit counters; a workgroup sees at most 512 pixels),
 * open-addressed by line, flushed as 128-byte runs of 64-bit global atomic adds; a pixel that finds no line adds to hist directly.
 * Integer sums: bit-reproducible.  hist should be 128-byte aligned for the runs to be whole lines (any alignment is correct).
 * Refused before launch: everything mi_upsample_predict_score refuses (a threshold outside [0, 1] or NaN is any entry of the table), bins other
 * than 1024 (0 is accepted with hist == NULL), hist with bins == 0, pseudo without class_threshold. */
int mi_upsample_predict_score_cw(const MiProbSource* src, int n, int K, int H, int W, float div_a, float div_b, const int64_t* labels,
                                 int ignore_index, const float* class_threshold, uint8_t* pred, uint8_t* pseudo, int64_t* counts, int bins,
                                 int64_t* hist, void* stream);

/* ---- sliding-window evaluation tails (TEST.SLIDE): sources that each cover a rectangle of the output ---------
 * Crop-sized windows slid over the picture with an overlap, each evaluated as inference() evaluates a picture (utility.py:179-191), the
 * windows' probabilities averaged where they overlap.  win is a HOST array of n windows, 1 <= n <= MI_SLIDE_MAX_WINDOWS, copied by value into
 * the kernel arguments (as MiProbSource is: no device table, no extra copy; 64 descriptors stay far below the kernel-argument limit and allow
 * an 8 x 8 grid).  Every window has the same low map size h x w ([h][w][K] fp32 NHWC logits of the crop; low_mirror: those of the mirrored
 * crop, NULL without flip, on all windows or on none) and owns the output rectangle [y0, y0 + wh) x [x0, x0 + ww): label coordinates.
 * Arithmetic contract, per output pixel (y, x) and class k, fp32, no contraction:
 *  - for every window i IN ORDER that contains the pixel, local coordinates yl = y - y0_i, xl = x - x0_i:
 *      p  = softmax_k(bilinear_align_corners(low_i: h x w -> wh x ww)) at (yl, xl), the device code of mi_upsample_softmax (a rounded product);
 *      pm = the same on low_mirror_i at (yl, ww-1-xl): the mirrored source evaluated AT the mirrored output column;
 *      q  = (p + pm) / 2 with mirror maps, p without;   acc = acc + q, starting from 0;
 *  - result = acc / (float)cover, a true division by the number of windows that contain the pixel.
 *  - cover == 1 without mirror maps is bit-equal to mi_upsample_softmax on that window.
 * mi_upsample_softmax_slide writes probs [K][H][W]; mi_upsample_predict_score_slide derives pred, pseudo, counts and hist from the same K
 * values exactly as mi_upsample_predict_score(_cw) do from theirs (one kernel body, another value provider): class_threshold == NULL,
 * hist == NULL and bins == 0 is the plain entry with `threshold`; otherwise the class-wise entry's rules hold and `threshold` is not used.
 * Refused before launch: everything those entries refuse; n outside 1..64; wh < h or ww < w; a window that leaves [0,H) x [0,W); mirror maps
 * on some windows only; an output pixel that no window covers (it would be 0 / 0; checked on the host over the distinct window edges). */
#define MI_SLIDE_MAX_WINDOWS 64
typedef struct { const float* low; const float* low_mirror; int y0, x0; } MiSlideWindow;
int mi_upsample_softmax_slide(const MiSlideWindow* win, int n, int h, int w, int wh, int ww, float* probs, int K, int H, int W, void* stream);
int mi_upsample_predict_score_slide(const MiSlideWindow* win, int n, int h, int w, int wh, int ww, int K, int H, int W, const int64_t* labels,
                                    int ignore_index, float threshold, const float* class_threshold, uint8_t* pred, uint8_t* pseudo,
                                    int64_t* counts, int bins, int64_t* hist, void* stream);

/* ---- precision-recall and calibration histograms of the evaluation tails (TEST.CURVES) ---------
 * What a confidence is worth on a labelled picture, as integer histograms of the per-pixel values a_0 .. a_{K-1} of the tails above:
 * mi_upsample_curves takes those of mi_upsample_softmax_multi (same src, n, div_a, div_b), mi_upsample_curves_slide those of
 * mi_upsample_softmax_slide (same windows): the same device code (multi_probs / slide_probs), so the histograms are functions of exactly
 * the bits those entries write.  Only pixels whose label lies in [0, K) count - the confusion matrix's rule: 255, the ignore value and any
 * other value outside count nowhere.  For every counted pixel with label g:
 *   pr  DEVICE int64 [K][256][2] or NULL:  for every class k   pr[k][b][g == k] += 1,   b = min(255, max(0, int(a_k * 256)))
 *       (a power-of-two scale and a truncation, exact in fp32: the bin is a function of the fp32 value alone);
 *   cal DEVICE int64 [ece_bins][3] or NULL:  conf = max_k a_k, pred = the LOWEST index among the maxima,
 *       m = min(ece_bins-1, max(0, int(conf * (float)ece_bins)))  (an fp32 product, truncated):
 *       cal[m] += (1, pred == g, int(conf * 2^24))   - the last a fixed-point sum: the scale is exact, the integer sum has no order.
 * Both are ADDED to (zeroed by the caller once per data set; launches into one buffer add up); one of them may be NULL.  Integer sums:
 * bit-reproducible.  From pr the host reads per class the precision and recall at the 256 thresholds j/256, average precision, best F1 and
 * the threshold that reaches a target precision; from cal ECE, MCE, accuracy and mean confidence (host/metrics.py curves_summary).
 * Overflow: a picture adds at most H * W < 2^31 to a cell of pr and at most H * W * (2^24 + 1) to a cell of cal; 5 000 pictures of
 * 2 M pixels each adding at most 2^24 + 1 are 1.7 * 10^17 < 2^63 = 9.2 * 10^18.
 * Kernel: a dense per-workgroup LDS table (32-bit counters in the layout of pr, 64-bit calibration cells; dynamic, 2048 K + 24 ece_bins
 * bytes), the two cells nearly every pixel hits - (k, bin 0, negative) and (k, bin 255, positive) - aggregated in the wave by ballots, a grid
 * capped at 1024 workgroups that stride over the pixel tiles and flush once with 64-bit global adds.  One launch, capturable, no host
 * round trip.  Two pixels per lane when W is even and labels is 16-byte aligned.
 * Refused before launch: everything the corresponding predict-and-score entry refuses about its sources or windows (n, K > 32, a zero
 * divisor, a bad source; the window geometry and the cover check), NULL labels, pr and cal both NULL, ece_bins outside 1..64 when cal is
 * given, H * W >= 2^31 (the 32-bit counters of a workgroup could overflow). */
int mi_upsample_curves(const MiProbSource* src, int n, int K, int H, int W, float div_a, float div_b, const int64_t* labels, int ece_bins,
                       int64_t* pr, int64_t* cal, void* stream);
int mi_upsample_curves_slide(const MiSlideWindow* win, int n, int h, int w, int wh, int ww, int K, int H, int W, const int64_t* labels,
                             int ece_bins, int64_t* pr, int64_t* cal, void* stream);

/* ---- polyp evaluation tail: what Dice / IoU / F-beta / E-measure / S-measure / MAE need of PraNet's map, without the host ever seeing the map ----
 * low [B][h][w] fp32 (the res2 logits), labels [B][H][W] int64 (ground truth in {0, 1}).  Per output pixel, all in fp32:
 *   z = bilinear(low -> H x W), align_corners False, ATen's source index, each axis interpolated as a + lambda (b - a): a constant map stays constant
 *       bit for bit and h == H / w == W is the identity; either axis may shrink or grow (two taps, no antialiasing, as F.interpolate);
 *   p = 1 / (1 + exp(-z));   prob = (p - min) / (max - min + 1e-8), min / max of p over the WHOLE batch (pranet_tester.py:43);
 *   q = int(prob * 255) truncated (0..255);   g = (label == 1).
 * Outputs, all written (not added to) by every call:
 *   hist   [B][2][256] int64: hist[b][g][q] = pixels of image b with ground truth g whose quantised probability is q;
 *   sums   [B][MI_POLYP_SUMS] double: [quadrant LT, RT, LB, RB][sum prob, sum prob^2, sum prob g, sum prob^2 g, sum g] (20 values) over the
 *          quadrants [0:cy, 0:cx], [0:cy, cx:W], [cy:H, 0:cx], [cy:H, cx:W], then cx, cy, and the batch's min and max of p.
 *          cx = int(round_half_even(sum(col g) / G)) + 1, cy likewise with rows, in double; (0, 0) when G == 0;
 *   counts [B][MI_POLYP_COUNTS] int64: G = sum g, sum(col g), sum(row g), the number of labels that are neither 0 nor 1 (counted as background);
 *   prob   [B][H][W] fp32 or NULL;   pred [B][H][W] uint8 or NULL: prob > 1 - prob (PranetTester's mask; ties go to background).
 * hist, sums, counts and pred come from exactly the fp32 values prob receives, and are the same bits whether prob / pred are requested or NULL.
 * Bit-reproducible run to run: the histogram, the counts and min / max (on the bits of p >= 0) are integer atomics, which do not depend on
 * arrival order; the floating-point sums use none - a thread adds at most 32 doubles, a wave adds in a xor butterfly, a workgroup writes one
 * partial row into the workspace, and a last launch adds the rows of an image in a fixed order.  prob^2 is exact in double.
 * Four launches on `stream` (init, scan, score, finalize); workspace: mi_polyp_score_workspace bytes, 8-byte aligned, no initialisation needed.
 * Refused before any launch: a NULL low / labels / hist / sums / counts / workspace, a non-positive size, B > 65535, a side above 2^20 or more
 * than 2^40 pixels, a workspace that is too small. */
#define MI_POLYP_SUMS 24
#define MI_POLYP_COUNTS 4
size_t mi_polyp_score_workspace(int B, int h, int w, int H, int W);
int mi_polyp_score(const float* low, const int64_t* labels, int B, int h, int w, int H, int W, int64_t* hist, double* sums, int64_t* counts,
                   float* prob, uint8_t* pred, void* workspace, size_t workspace_bytes, void* stream);

/* ---- input side of multi-scale evaluation: F.interpolate(x, (Ho, Wo), mode='bilinear', align_corners=True) (utility.py:197) ----
 * x [B][C][H][W] fp32 NCHW (the loader's layout, what mi_stem_f32 consumes) -> out [B*(1+with_mirror)][C][Ho][Wo].  with_mirror != 0:
 * image b's horizontally mirrored copy (torch.flip(resized, [3]), utility.py:204: the mirror of the RESIZED image) is written as image B + b
 * in the same launch, bit-equal to the mirror of image b.  Ho == H && Wo == W reproduces the input bit for bit. */
int mi_image_resize_ac(const float* x, float* out, int B, int C, int H, int W, int Ho, int Wo, int with_mirror, void* stream);

/* ---- locally connected CRF refinement of a probability map (TEST.CRF; not in the reference: the third part of DeepLabV2 as published) ----
 * Mean field over a dilated window with Gaussian position and bilateral kernels and Potts compatibility (the form of ConvCRF).  Per image:
 * p [K][H][W] fp32 probabilities, I [3][H][W] the normalised input image at the same size, cs0..cs2 the factors that turn a difference of the
 * normalised image into a difference in 0..255 units.  eps = 1e-5; all arithmetic fp32.
 *   U_i[c]   = log(max(p_i[c], eps))
 *   offsets  o = (dy, dx) * dilation, dy, dx in [-(window/2), window/2], (dy, dx) != (0, 0), in row-major order
 *   in(i,o)  = 1 if pixel i + o lies inside the image, else 0
 *   gp(o)    = exp(-|o|^2 / (2 pos_xy^2));   gb(o) = exp(-|o|^2 / (2 bi_xy^2))
 *   gc(i,o)  = exp(-sum_ch (cs[ch] (I_{i+o}[ch] - I_i[ch]))^2 / (2 bi_rgb^2))
 *   Np_i     = sum_o in(i,o) gp(o);   Nb_i = sum_o in(i,o) gb(o)      (geometry only: never near zero because of colour)
 *   k(i,o)   = in(i,o) [pos_w gp(o) / Np_i + bi_w gb(o) gc(i,o) / Nb_i]      (a term whose N is 0 is 0)
 *   Q^0      = softmax_c(U);   Q^{t+1}_i = softmax_c(U_i[c] + sum_o k(i,o) Q^t_{i+o}[c]),  t = 0 .. iters-1
 * Outputs, each optional: out_probs = Q^{iters}; pred = the lowest class index among its maxima; conf = that maximum.  iters == 0: softmax(U).
 * What an output receives does not depend on which other outputs are requested, and two calls give the same bits (fixed neighbour order, no
 * atomics).  1 + iters launches on `stream`, nothing read back in between (capturable in a HIP graph); Q ping-pongs between the two halves of
 * the workspace (mi_crf_workspace bytes, 16-byte aligned, no initialisation needed; unused for iters == 0).  probs is read by every launch:
 * out_probs may alias neither it nor the image.
 * Refused before any launch (MI_EINVAL unless stated): a NULL probs / image, all three outputs NULL, K outside 1..32, window even or outside
 * 3..11, dilation outside 1..16, iters outside 0..32, a sigma that is not positive and finite, a weight that is negative or not finite,
 * B * H * W >= 2^31, a workspace that is too small (MI_ENOMEM). */
size_t mi_crf_workspace(int B, int K, int H, int W);
int mi_crf_refine(const float* probs /*[B][K][H][W]*/, const float* image /*[B][3][H][W]*/, float cs0, float cs1, float cs2,
                  float* out_probs /*[B][K][H][W] or NULL*/, uint8_t* pred /*[B][H][W] or NULL*/, float* conf /*[B][H][W] or NULL*/,
                  int B, int K, int H, int W, int iters, int window, int dilation,
                  float pos_w, float pos_xy, float bi_w, float bi_xy, float bi_rgb,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- Boundary IoU and trimap IoU of one picture (TEST.BOUNDARY; not in the reference: Cheng et al., CVPR 2021, and DeepLab's trimap plot) ----
 * pred [H][W] uint8, labels [H][W] int64, K classes, ignore_index outside [0, K), D the largest band width asked for.  Two class maps:
 *   G(p) = labels(p) where it lies in [0, K), else 255
 *   P(p) = 255 where labels(p) == ignore_index, else pred(p) where it is < K, else 255      (intersectionAndUnionGPU: output[target == ignore] = ignore)
 * For a map L and a pixel with L(p) < K, e_L(p) is the number of 3 x 3 erosions (outside the picture = background) p survives in the binary
 * mask L == L(p), capped at D: the largest r <= D whose (2r+1) x (2r+1) window around p lies inside the picture and is uniformly L(p).
 * Separably: a(y,x) = min(D, the largest r with L(y, x-r..x+r) inside the row and all equal to L(y,x)); radius r + 1 holds iff rows y +- (r+1)
 * exist, carry L(y,x) in column x, and the minimum of a over rows y-(r+1) .. y+(r+1) of column x is >= r + 1.  p lies in the boundary band of
 * width d of its class iff e_L(p) < d (mask - erode^d(mask)).
 * The call ADDS to hist, int64 [5][K][D+1] on the device (the caller zeroes it; calls into one buffer add up):
 *   hist[0][k][eG]           G == k             ground-truth band sizes, trimap target area
 *   hist[1][k][eP]           P == k             prediction band sizes
 *   hist[2][k][max(eG, eP)]  G == P == k        Boundary-IoU intersection
 *   hist[3][k][eG]           G == P == k        trimap intersection
 *   hist[4][k][eG]           P == k, G < K      trimap output area, by predicted class
 * With S_i[k] = sum of hist[i][k][0 .. d-1]: Boundary IoU at width d = S2 / (S0 + S1 - S2), trimap IoU = S3 / (S0 + S4 - S3).  Summed over
 * all D + 1 cells, hist[3], hist[4] and hist[0] are intersectionAndUnionGPU's area_intersection, area_output and area_target.
 * Integers only (no floating point, integer atomics): two calls give the same bits.  Two launches on `stream`, nothing read back (capturable
 * in a HIP graph).  The workspace (mi_boundary_score_workspace bytes, 4-byte aligned, no initialisation needed) holds one 32-bit word per pixel
 * between them; mi_boundary_score_workspace returns 0 for sizes the call refuses.
 * Refused before any launch (MI_EINVAL unless stated): a NULL pred / labels / hist / workspace, a non-positive size, H * W >= 2^31, K outside
 * 1..32, D outside 1..64, ignore_index inside [0, K), a workspace that is too small (MI_ENOMEM). */
size_t mi_boundary_score_workspace(int H, int W);
int mi_boundary_score(const uint8_t* pred /*[H][W]*/, const int64_t* labels /*[H][W]*/, int H, int W, int K, int ignore_index, int D,
                      int64_t* hist /*[5][K][D+1], added to*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---- surface-distance metrics of binary masks (TEST.SURFACE_METRICS; not in the reference: medpy's hd / hd95 / assd with connectivity 1, and
 * surface Dice) ----
 * pred [B][H][W] uint8, labels [B][H][W] int64; per image P = (pred == cls), G = (label == cls) on the H x W grid.
 *   Surface S(M): the pixels of M with at least one of their four neighbours outside M.  A neighbour outside the image counts as outside M, so
 *       foreground on the image frame is always surface: S(M) = M & ~binary_erosion(M, cross, border_value=0).
 *   Directed distances: for every s in S(P), d2(s) = min over t in S(G) of (sx - tx)^2 + (sy - ty)^2, an exact integer; likewise from S(G).
 *   HD = sqrt of the larger of the two directed maxima of d2.
 *   HD-q = numpy's linear-interpolation percentile of the CONCATENATION of the two directed distance lists (medpy's convention, not a
 *       per-direction percentile): rank r = q (n - 1) / 100 with n = |S(P)| + |S(G)|, value a[floor r] + frac(r) (a[floor r + 1] - a[floor r])
 *       on the sorted distances.
 *   ASSD = the mean of the two directed mean distances.
 *   NSD(tau) = (|{s in S(P): d <= tau}| + |{s in S(G): d <= tau}|) / n, decided on integers as d2 <= floor(tau^2).
 *   Both masks empty: every distance is 0 and NSD is 1.  Exactly one empty: the distances are undefined, NSD is 0.
 * q_num: the integer percentile q in 1..100.  tol2: T values floor(tau^2) in HOST memory (read before the first launch; NULL when T == 0).
 * Outputs, all written (not added to) by every call:
 *   ints [B][MI_SURFACE_INTS] int64: 0 |P|, 1 |G|, 2 |S(P)|, 3 |S(G)|, 4 max d2 from S(P), 5 max d2 from S(G), 6 d2[floor r] and
 *        7 d2[min(floor r + 1, n - 1)] of the sorted combined list, 8 floor r, 9 the remainder q (n - 1) mod 100 (frac(r) = remainder / 100),
 *        10 defined (1) / undefined (0), then 11 + 2 t + direction: the surface pixels of P (direction 0) / G (direction 1) with
 *        d2 <= tol2[t]; cells of t >= T are 0.  Fields 4..9 and the tolerance counts are 0 unless both masks have pixels.
 *   sums [B][2] double: the sums of sqrt((double) d2) over S(P) and over S(G).
 * Bit-reproducible run to run: everything but sums is integer arithmetic with integer atomics; sums uses no floating-point atomics - a thread
 * adds its pixels of a row in ascending x, a wave adds in a xor butterfly, one partial per row goes to the workspace, a last launch adds the
 * rows of an image in a fixed order.  Seven launches on `stream`, nothing read back in between (capturable in a HIP graph).  The workspace
 * (mi_surface_score_workspace bytes, 8-byte aligned, no initialisation needed) holds 5 bytes per pixel, 16 bytes per row and 64 KiB of histograms
 * per image; mi_surface_score_workspace returns 0 for sizes the call refuses.
 * Refused before any launch (MI_EINVAL unless stated): a NULL pred / labels / ints / sums / workspace (tol2 with T > 0), a non-positive size,
 * B > 65535, a side above 4096 (d2 < 2^25), cls outside 0..255, q_num outside 1..100, T outside 0..MI_SURFACE_MAX_TOL, a negative tol2, a
 * workspace that is too small (MI_ENOMEM). */
#define MI_SURFACE_MAX_TOL 8
#define MI_SURFACE_INTS 27
size_t mi_surface_score_workspace(int B, int H, int W);
int mi_surface_score(const uint8_t* pred /*[B][H][W]*/, const int64_t* labels /*[B][H][W]*/, int B, int H, int W, int cls, int q_num,
                     const int32_t* tol2 /*host [T]*/, int T, int64_t* ints /*[B][MI_SURFACE_INTS]*/, double* sums /*[B][2]*/, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---- exact signed Euclidean distance map of a batch of masks (SOLVER.BOUNDARY_WEIGHT; not in the reference: the level-set map of the boundary
 * loss, edt(~G) * ~G - (edt(G) - 1) * G with scipy.ndimage.distance_transform_edt) ----
 * mask [B][H][W] fp32; per image G = (mask >= thresh), a NaN is background.
 *   d2(q) for q outside G = min over t in G of |q - t|^2; for q in G = min over t outside G of |q - t|^2: an exact integer.  Pixels outside the
 *       image do not exist; they are neither foreground nor background.
 *   phi(q) = +sqrt(d2) outside G and -(sqrt(d2) - 1) inside G (+0 where d2 = 1), formed from sqrt((double) d2) in float64 and rounded to float32
 *       once: bit for bit the float32 cast of the line above.
 *   An image whose G is empty or the whole image has no contour: phi = 0 and d2 = 0 everywhere.
 * Outputs, all written by every call: phi [B][H][W] fp32; d2 (may be NULL) [B][H][W] int32; counts (may be NULL) [B][2] int32: foreground and
 * background pixels.  Bit-reproducible: integer arithmetic with integer atomics up to the final square root.  A memset and two launches on `stream`
 * (a column pass over the mask, a row pass with one workgroup per row), nothing read back (capturable in a HIP graph).  The workspace
 * (mi_signed_distance_workspace bytes, 4-byte aligned, no initialisation needed) holds 4 bytes per pixel and 4 per image;
 * mi_signed_distance_workspace returns 0 for sizes the call refuses.
 * Refused before any launch (MI_EINVAL unless stated): a NULL mask / phi / workspace, a non-positive size, B > 65535, a side above 4096
 * (d2 < 2^25), a thresh that is not finite, a workspace that is too small (MI_ENOMEM). */
size_t mi_signed_distance_workspace(int B, int H, int W);
int mi_signed_distance(const float* mask /*[B][H][W]*/, float thresh, float* phi /*[B][H][W]*/,
                       int32_t* d2 /*[B][H][W], may be NULL: tests and diagnosis*/,
                       int32_t* counts /*[B][2], may be NULL: foreground, background pixels*/, int B, int H, int W, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- connected components of a batch of binary masks (not in the reference: scipy.ndimage.label with the cross or the full 3 x 3 structure) ----
 * mask [B][H][W] uint8; per image the foreground is F = (mask == cls) on the H x W grid.
 *   Two foreground pixels are neighbours when they differ by one step along x or y (connectivity 4), or by at most one step along each
 *       (connectivity 8).  A component is a maximal set of foreground pixels joined by chains of neighbours.
 *   The first pixel of a component is its smallest linear index y * W + x.  Components are numbered 1..n per image in the raster order of their
 *       first pixels.
 * Outputs, all written by every call:
 *   labels [B][H][W] int32 (may be NULL): 0 on background, the component's number elsewhere.
 *   roots  [B][H][W] int32 (may be NULL): the linear index of the component's first pixel, -1 on background.
 *   counts [B] int32: n per image.
 * Bit-reproducible run to run: union-find on row runs whose roots are the smallest index of their component whatever the order of the merges;
 * integer atomics only, no floating point.  Six launches on `stream`, nothing read back in between (capturable in a HIP graph): rows, merge,
 * flatten, a scan of the rows' root counts, the numbers, the outputs.  No launch waits on another workgroup.  The workspace
 * (mi_label_components_workspace bytes, 8-byte aligned, no initialisation needed) holds 8 bytes and one bit per pixel and 4 bytes per row;
 * mi_label_components_workspace returns 0 for sizes the call refuses.
 * Refused before any launch (MI_EINVAL unless stated): a NULL mask / counts / workspace, labels and roots both NULL, a non-positive size,
 * B > 65535, a side above 4096, cls outside 0..255, a connectivity other than 4 or 8, a workspace that is too small (MI_ENOMEM). */
size_t mi_label_components_workspace(int B, int H, int W);
int mi_label_components(const uint8_t* mask /*[B][H][W]*/, int B, int H, int W, int cls, int connectivity, int32_t* labels /*[B][H][W], may be NULL*/,
                        int32_t* roots /*[B][H][W], may be NULL*/, int32_t* counts /*[B]*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---- lesion-wise detection counts and component filtering of binary masks (TEST.LESION_METRICS, TEST.MASK_MIN_AREA, TEST.MASK_KEEP_LARGEST;
 * not in the reference) ----
 * pred [B][H][W] uint8, labels [B][H][W] int64 (any value other than cls is background); per image P = (pred == cls), G = (label == cls), their
 * components as mi_label_components defines them at `connectivity`.
 *   Filter: P' = the union of the components of P with at least min_area pixels; with keep_largest only the largest of those stays, a tie goes to
 *       the component whose first pixel comes first in raster order.  An empty P stays empty.
 *   True positives: a component p of P' with hit(p) = |p & G| >= 1 and 1000 hit(p) >= overlap_permille |p| (64-bit integers); any other
 *       component of P' is a false positive.
 *   Detected lesions: a component g of G with hit'(g) = |g & P'| >= 1 and 1000 hit'(g) >= overlap_permille |g|; any other is missed.
 *       overlap_permille 0: any shared pixel counts.
 * Outputs, all written by every call:
 *   filtered [B][H][W] uint8 (may be NULL): cls on P', and (cls == 0 ? 1 : 0) elsewhere.
 *   ints [B][MI_LESION_INTS] int64: 0 |P|, 1 |P'|, 2 |G|, 3 components of P, 4 components of P', 5 components of G, 6 true-positive components
 *        of P', 7 detected components of G, 8 the largest component area of P, 9 of G, 10 |P' & G|, 11 components of P the filter removed
 *        (counted on its own: equal to field 3 minus field 4).
 * Bit-reproducible run to run: integer arithmetic with integer atomics, no floating point.  A memset and seven launches on `stream`, nothing
 * read back in between (capturable in a HIP graph): rows, merge and flatten over P and G as 2 B planes, then selection, hits, counts and the
 * output row.  No launch waits on another workgroup.  The workspace (mi_lesion_score_workspace bytes, 8-byte aligned, no initialisation needed)
 * holds 24 bytes and two bits per pixel, 8 bytes per row and 128 bytes per image; mi_lesion_score_workspace returns 0 for sizes the call refuses.
 * Refused before any launch (MI_EINVAL unless stated): a NULL pred / labels / ints / workspace, a non-positive size, B > 65535, a side above
 * 4096, cls outside 0..255, a connectivity other than 4 or 8, a negative min_area, keep_largest other than 0 / 1, overlap_permille outside
 * 0..1000, a workspace that is too small (MI_ENOMEM). */
#define MI_LESION_INTS 12
size_t mi_lesion_score_workspace(int B, int H, int W);
int mi_lesion_score(const uint8_t* pred /*[B][H][W]*/, const int64_t* labels /*[B][H][W]*/, int B, int H, int W, int cls, int connectivity, int min_area,
                    int keep_largest, int overlap_permille, uint8_t* filtered /*[B][H][W], may be NULL*/, int64_t* ints /*[B][MI_LESION_INTS]*/,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- optimiser: torch.optim.SGD(momentum, weight_decay) on flat fp32 buffers (aspp_trainer.py:25-26,94-95)
 * g' = g + wd*p; buf = mu*buf + g'; p -= lr*buf  (buf zero-initialised == torch's first-step buf = g'). */
int mi_sgd_step(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float weight_decay, void* stream);
/* the same update with hyper = {lr, momentum, weight_decay} read from DEVICE memory at run time: under HIP graph capture a
 * by-value argument is frozen into the graph, a pointer is not - the poly learning rate changes every step. */
int mi_sgd_step_dev(float* p, const float* g, float* buf, size_t n, const float* hyper /*[3], device*/, void* stream);
/* mi_sgd_step (mi_sgd_step_dev) over the whole flat store AND mi_pack_weights_multi of the updated weights, in one pass: every conv weight a row of
 * `table_dev` describes (mi_pack_weights_multi's table, n_desc, total_blocks) is updated tile by tile and both bf16 operands are written from the
 * registers / LDS that hold the new values; `gaps_dev` = n_gaps pairs [lo, hi) of element indices: what no row covers (other parameters, padding,
 * a tail), updated in the same launch.  Rows and gaps must partition [0, n).  p and buf get mi_sgd_step's bits, wp / wpt the bits
 * mi_pack_weights_multi writes from the stored p.  Buffers 16-byte aligned.  mi_sgd_pack_enabled: the MI_SGD_PACK switch (default 1). */
int mi_sgd_pack_enabled(void);
int mi_sgd_step_pack(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float weight_decay, const float* sflat, void* wp,
                     void* wpt, const int64_t* table_dev, int n_desc, int total_blocks, const int64_t* gaps_dev, int n_gaps, void* stream);
int mi_sgd_step_pack_dev(float* p, const float* g, float* buf, size_t n, const float* hyper /*[3], device*/, const float* sflat, void* wp, void* wpt,
                         const int64_t* table_dev, int n_desc, int total_blocks, const int64_t* gaps_dev, int n_gaps, void* stream);

/* ---- stem tail: FrozenBN + ReLU + 3x3/stride 2/pad 1 max-pool fused (resnet.py:138-141) ----------------------
 * y: conv1 output [B][Hc][Wc][C] bf16 NHWC; pool [B][Hp][Wp][C] bf16; idx one byte per pooled element: the winning
 * tap 0..8 (first maximum in scan order, like ATen) or 9 when the pooled value is 0 (no gradient through ReLU).
 * backward: dy[b][h][w][c] = scale[c] * sum of dpool over the windows whose idx points at (h,w).  C % 8 == 0. */
int mi_stem_pool_fwd(const void* y, const float* scale, const float* shift, void* pool, uint8_t* idx,
                     int B, int Hc, int Wc, int C, int Hp, int Wp, void* stream);
int mi_stem_pool_bwd(const void* dpool, const uint8_t* idx, const float* scale, void* dy,
                     int B, int Hc, int Wc, int C, int Hp, int Wp, void* stream);
/* Patch matrix of the stem conv (7x7, stride 2, pad 3, 3 input channels; resnet.py:137): col[m][k] bf16 [B*Ho*Wo][ncols], k = (c*7+ky)*7+kx for
 * k < 147, zero above (ncols a multiple of 8; 192 when the matrix also feeds the forward as a 1x1 mi_conv_gemm, 160 for the weight gradient
 * alone).  With it the stem conv is a plain GEMM and its weight gradient a 1x1 mi_conv_wgrad (deterministic), not the library's atomics. */
int mi_stem_im2col(const void* x_bf16_nhwc, void* col_bf16, int B, int H, int W, int Ho, int Wo, int ncols, void* stream);
/* The stem conv on raw image rows (csrc/stem_direct.hip): no patch matrix in forward or backward.
 * mi_stem_pack_image: x fp32 NCHW [B][3][H][W] (x_is_bf16_nhwc 0) or bf16 NHWC [B][H][W][3] (1) -> x4 bf16 [B][H][W][4], channel 3 = 0, in one pass
 *   (channels 0..2 are x rounded to nearest even, like x.to(bf16)).  x4 8-byte aligned.
 * mi_stem_conv_fwd: x4 and w fp32 [64][3][7][7] -> y [B][Ho][Wo][64] bf16 NHWC, the raw conv output.  The contraction runs in the order of
 *   mi_stem_im2col (192 columns) + mi_conv_gemm, which it replaces: y has the same bits.  wpack: 6*64*32 bf16 (24 KiB, 16-byte aligned) of scratch,
 *   rewritten by every call (the weights as [k / 32][o][k % 32], k the OIHW order).  O must be 64, (Ho, Wo) the 7x7/2/3 output size, every tensor
 *   within 2^31 elements; refused before any launch otherwise.
 * mi_stem_conv_wgrad: dy [B][Ho][Wo][64] bf16 NHWC and x4 -> dw fp32 [64][3][7][7].  Pixels are split over workgroups, each writes an fp32
 *   partial into `workspace` (mi_stem_conv_wgrad_workspace bytes, 16-byte aligned), and a reducer sums the partials in ascending split order: no
 *   float atomics, bit-reproducible.
 * mi_stem_conv_wgrad_pool: the same weight gradient from the POOLED gradient: dpool [B][Hp][Wp][64] bf16 NHWC, idx (the argmax bytes of
 *   mi_stem_pool_fwd, one per pooled element, 8-byte aligned) and the BatchNorm scale [64].  The launch builds each tile's dy in its staging exactly as
 *   mi_stem_pool_bwd computes it, so dw has the bits of mi_stem_pool_bwd + mi_stem_conv_wgrad, and dy is never written.  Same workspace.
 * mi_stem_pool_wgrad_enabled: the MI_STEM_POOL_WGRAD switch (default 1; 0: the host engine calls mi_stem_pool_bwd, then mi_stem_conv_wgrad).
 * mi_stem_direct_enabled: the MI_STEM_DIRECT switch (default 1; 0: the host engine takes the patch-matrix route, mi_stem_im2col + GEMM). */
int mi_stem_direct_enabled(void);
int mi_stem_pack_image(const void* x, int x_is_bf16_nhwc, void* x4, int B, int H, int W, void* stream);
int mi_stem_conv_fwd(const void* x4, const float* w, void* wpack, void* y, int B, int H, int W, int O, int Ho, int Wo, void* stream);
size_t mi_stem_conv_wgrad_workspace(int B, int Ho, int Wo);
int mi_stem_conv_wgrad(const void* dy, const void* x4, float* dw, int B, int H, int W, int O, int Ho, int Wo, void* workspace,
                       size_t workspace_bytes, void* stream);
int mi_stem_pool_wgrad_enabled(void);
int mi_stem_conv_wgrad_pool(const void* dpool, const uint8_t* idx, const float* scale, const void* x4, float* dw, int B, int H, int W, int O,
                            int Ho, int Wo, int Hp, int Wp, void* workspace, size_t workspace_bytes, void* stream);

/* ---- FADA adversarial step (reference core/combos/aspp_fada.py:80-127) ---------------------------
 * db[n] (+)= sum_m dy[m][n]  (conv bias gradient; dy bf16 [M][N], N % 8 == 0; fixed summation order) */
int mi_bias_grad_bf16(const void* dy_bf16, float* db, int M, int N, int accumulate,
                      void* workspace /* mi_colsum_workspace(M, N) */, size_t workspace_bytes, void* stream);
/* Fused  soft = clip(softmax(upsample(seg_low) * inv_temperature), clip);  pred = upsample(d_low)[:, :2K];
 *        loss = mean_pixels( -sum_c soft_c * log_softmax(pred)[c + domain*K] )
 * = soft_label_cross_entropy(model_D(fea, size), cat(soft, 0) or cat(0, soft)) of aspp_fada.py:104-121 with the soft labels
 * of :96-103, without materialising any [B,C,H,W] tensor.  seg_low [B][h][w][K], d_low [B][h][w][ldD] (first 2K channels
 * used), dd_low (may be NULL) = d loss / d d_low * grad_scale, same layout (padding channels zeroed).  loss_out[0] = loss,
 * loss_out[1] = pixel count.  K <= 32, 2K <= ldD. */
size_t mi_upsample_softce_workspace(int B, int h, int w, int K, int H, int W);
int mi_upsample_softce(const float* seg_low, float inv_temperature, float clip, const float* d_low, int ldD, int domain,
                       float* loss_out, float* dd_low, int B, int h, int w, int K, int H, int W, float grad_scale,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The same loss with the two operands on their own grids and conventions (GaldFada; reference core/combos/gald_fada.py:96-121): seg_low
 * [B][hs][ws][K] upsampled with seg_align_corners, d_low [B][hd][wd][ldD] with d_align_corners, both to H x W (H >= hs, hd; W >= ws, wd;
 * any ratio, integer or not).  Computed per high-resolution pixel, no [B,C,H,W] tensor, fixed summation orders (bitwise reproducible); LDS
 * per workgroup depends on K only.  K <= 32 (19: compile-time path), 2K <= ldD, domain 0 | 1; bad arguments return MI_EINVAL before any
 * launch.  loss_out[2], dd_low (may be NULL; padding channels zeroed) as mi_upsample_softce. */
size_t mi_upsample_softce_2grid_workspace(int B, int hd, int wd, int K, int H, int W);
int mi_upsample_softce_2grid(const float* seg_low, int hs, int ws, int seg_align_corners, float inv_temperature, float clip,
                             const float* d_low, int hd, int wd, int ldD, int d_align_corners, int domain, float grad_scale,
                             float* loss_out, float* dd_low, int B, int K, int H, int W, void* workspace, size_t workspace_bytes, void* stream);
/* torch.optim.Adam (no amsgrad, weight_decay 0; fada_adapter.py:24) on flat fp32 buffers; step >= 1 is this update's index */
int mi_adam_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1, float beta2,
                 float eps, int step, void* stream);
/* the same after clamping g to [-grad_clamp, grad_clamp] in place: clip_gradient (core/utils/utils.py:6-16) + Adam.step of pranet_trainer.py:59-60 */
int mi_adam_step_clamped(float* p, float* g, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1, float beta2,
                         float eps, int step, float grad_clamp, void* stream);

/* the same with hyper = {lr, beta1, beta2, eps, grad_clamp (<= 0: none), step} read from DEVICE memory at run time (HIP-graph replay: by-value
 * arguments are frozen into a captured graph; the step count and with it the bias corrections change on every replay) */
int mi_adam_step_dev(float* p, float* g, float* exp_avg, float* exp_avg_sq, size_t n, const float* hyper /*[6], device*/, void* stream);

/* ---- exact-fp32 evaluation path (test.py / ASPPTester; csrc/igemm_f32.hip) ---------------------------------------
 * The reference computes in fp32; BASELINE.json asks for argmax masks identical to it.  These entry points run the same
 * graph on fp32 NHWC activations with fp32 weights on the f32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain,
 * one rounding per product).  Forward only.
 * mi_pack_weight_f32: wp[t][o][i] = w[o][i][t] (no rounding; for ksize 1 the OIHW tensor itself is already this layout).
 * mi_conv_f32: out[b][ho][wo][n] = epi( sum_{t,c} a[b][ho*stride+ky*dil-pad][wo*stride+kx*dil-pad][c] * wp[t][n][c] ),
 *   a [B][Ha][Wa][Ca] fp32 (Ca % 16 == 0), out [B][Ho][Wo][N] fp32 (any N).  flags: MI_EPI_SCALE_BIAS (v*scale[n] then
 *   +bias[n], two rounded operations like layers.py:21-23; scale NULL = bias only, nn.Conv2d(bias=True) of classifier.py:12-20),
 *   MI_EPI_RESIDUAL (v += res[m][n]: `out += identity` resnet.py:110, or `out += conv_i(x)` classifier.py:28-29), MI_EPI_RELU.
 * mi_stem_f32: x [B][3][H][W] fp32 NCHW (the loader's layout) -> relu(bn(conv 7x7/2/3)) as [B][Hc][Wc][64] fp32 NHWC
 *   (resnet.py:137-139), w = conv1.weight [64][3][7][7], scale/shift = FrozenBN fold.
 * mi_maxpool_f32: 3x3 / stride 2 / pad 1 max-pool on fp32 NHWC (resnet.py:141), C % 4 == 0. */
int mi_pack_weight_f32(const float* w_oihw, float* wp, int O, int I, int ksize, void* stream);
int mi_conv_f32(const float* a, const float* wp, float* out, int B, int Ha, int Wa, int Ca, int Ho, int Wo, int N,
                int ksize, int stride, int pad, int dil, const float* scale, const float* bias, const float* res,
                int flags, void* stream);
int mi_stem_f32(const float* x_nchw, const float* w, const float* scale, const float* shift, float* y_nhwc,
                int B, int H, int W, void* stream);
int mi_maxpool_f32(const float* y_nhwc, float* pool_nhwc, int B, int Hc, int Wc, int C, void* stream);

/* ---- data-parallel gradient exchange over RCCL (csrc/comm.hip) ----------------------------------------------
 * For hosts that do not go through torch.distributed (the Python product does: host/ddp.py, backend "nccl" = RCCL).  One process
 * per GPU; rank 0 calls mi_comm_unique_id and passes the 128 bytes to the other ranks by its own means; every rank calls
 * mi_comm_init_rank; per step each bucket of the flat fp32 gradient buffer is averaged in place with mi_allreduce_bucket on a
 * side stream (order it after the bucket's weight-gradient launches with an event) and the optimizer stream waits for that
 * stream before mi_sgd_step.  librccl.so is resolved at the first call (dlopen; a copy already in the process is reused).
 * dtype: 0 = fp32, 1 = bf16; average != 0 divides by the number of ranks (ncclAvg). */
int mi_comm_unique_id(void* id128 /* host, 128 bytes out */);
int mi_comm_init_rank(void** comm /* out */, int nranks, const void* id128 /* host */, int rank);
int mi_comm_destroy(void* comm);
int mi_allreduce_bucket(void* ptr, size_t count, int dtype, int average, void* comm, void* stream);

/* ---- elementwise helpers ------------------------------------------------------------------------ */
/* y = msk > 0 ? x : 0 (bf16, n % 8 == 0): ReLU backward across an autograd boundary.  bits != 0: `msk` is the packed
 * sign-bit tensor written by MI_EPI_WRITE_MASK (same element order). */
int mi_relu_mask(const void* x_bf16, const void* msk, void* y_bf16, size_t n, int bits, void* stream);
/* The MI_HEAD_MASK switch (default 1): where the fused loss is the backbone output's only consumer (the source-only step), the host engine hands
 * the output's sign bits to the head's data gradient (MI_EPI_BITMASK epilogue) and skips the stand-alone mi_relu_mask pass over that gradient. */
int mi_head_mask_enabled(void);
/* FrozenBN fold: scale = w*rsqrt(var) (no eps), shift = b - mean*scale (layers.py:18-20) */
int mi_frozen_bn_fold(const float* w, const float* b, const float* mean, const float* var, float* scale, float* shift, int n, void* stream);

/* ---- trainable BatchNorm2d (MODEL.FREEZE_BN=False: feature_extractor.py:37-39 builds the backbone on torch.nn.BatchNorm2d) over NHWC
 * bf16 activations [M][C], C % 8 == 0, C <= 2048 for the reductions.  Reductions return RAW per-channel sums in a fixed order (bitwise
 * reproducible); the caller divides by the pixel count, after an all-reduce over ranks when the statistics are synchronised
 * (train_distill.py:53 converts to SyncBatchNorm).  workspace: mi_bn_workspace(M, C) bytes. */
size_t mi_bn_workspace(long M, int C);
/* out[c] = sum_m y[m][c] (mean == NULL) or sum_m (y[m][c] - mean[c])^2 (two-pass variance) */
int mi_bn_colsum(const void* y_bf16, const float* mean, long M, int C, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* one pass: s1[c] = sum_m (y[m][c] - pilot[c]), s2[c] = sum_m (y[m][c] - pilot[c])^2; mean = pilot + s1/N, var = s2/N - (s1/N)^2.  The pilot
 * must be the same on every rank that shares the statistics (the running mean is). */
int mi_bn_colsum2(const void* y_bf16, const float* pilot, long M, int C, float* s1, float* s2, void* workspace, size_t workspace_bytes, void* stream);
/* Conv forward (mi_conv_gemm's contract, plain bf16 store) that also returns what mi_bn_colsum2 would compute on its output: sums[0][n] = sum_m (out[m][n] -
 * pilot[n]), sums[1][n] = sum_m (out[m][n] - pilot[n])^2 over the bf16-rounded outputs, accumulated per row tile in the epilogue and added in a fixed
 * order (bitwise reproducible) - the statistics pass over the conv output of `bn(conv(x))` (resnet.py:93-109 with feature_extractor.py:37) costs no
 * extra read.  gamma != NULL: the last reduction launch also does mi_bn_finalize's work with count = B*Ho*Wo (gamma, beta, running_mean / running_var or
 * both NULL, num_batches_tracked or NULL, momentum, eps, out4 [4][N]) - the unsynchronised BatchNorm2d; gamma == out4 == NULL: sums only (the caller
 * all-reduces them and calls mi_bn_finalize).  workspace: mi_conv_gemm_stats_workspace(B*Ho*Wo, N) bytes. */
size_t mi_conv_gemm_stats_workspace(long M, int N);
int mi_conv_gemm_stats(const void* a, const void* wp, void* out, int B, int Ha, int Wa, int Ca, int Ho, int Wo, int N, int ksize, int stride, int pad,
                       int dil, const float* pilot, float* sums, void* workspace, size_t workspace_bytes, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps, float* out4, void* stream);
/* (s1, s2) of mi_bn_colsum2 over `count` pixels (all ranks) -> out4 = [mean | invstd | gamma * invstd | beta - mean * gamma * invstd] ([4][C] fp32), in
 * double; running_mean / running_var (both or neither) updated as torch.nn.BatchNorm2d does (momentum, unbiased variance), num_batches_tracked
 * (optional, int64 scalar) += 1.  pilot may alias running_mean (it is read first).  Replaces the host arithmetic between statistics and normalise pass
 * of resnet.py:84-113's BatchNorm2d in train(). */
int mi_bn_finalize(const float* s1, const float* s2, const float* pilot, double count, const float* gamma, const float* beta, float* running_mean,
                   float* running_var, long long* num_batches_tracked, float momentum, float eps, float* out4, int C, void* stream);
/* out = relu?((y - mean[c]) * scale[c] + beta[c] (+ res)), scale = gamma * rsqrt(var + eps); mask_out (optional, C % 16 == 0): the
 * packed sign bits of out in the layout of MI_EPI_WRITE_MASK */
int mi_bn_apply(const void* y_bf16, const float* mean, const float* scale, const float* beta, const void* res_bf16, void* out_bf16,
                void* mask_out, int relu, long M, int C, void* stream);
/* dbeta[c] = sum_m g[m][c], dgamma[c] = sum_m g[m][c] * (y[m][c] - mean[c]) * invstd[c]   (raw sums); relu_bits (optional, C % 16 == 0):
 * the packed sign bits of the layer's output - g counts only where the bit is set (ReLU backward without a separate pass) */
int mi_bn_bwd_colsums(const void* g_bf16, const void* y_bf16, const float* mean, const float* invstd, const void* relu_bits, long M, int C,
                      float* dbeta, float* dgamma, void* workspace, size_t workspace_bytes, void* stream);
/* dy = gamma * invstd * (g - dbeta * inv_count - xhat * dgamma * inv_count), xhat = (y - mean) * invstd; inv_count = 1 / (pixels over all
 * ranks that shared the statistics) */
int mi_bn_bwd_apply(const void* g_bf16, const void* y_bf16, const float* mean, const float* invstd, const float* gamma, const float* dbeta,
                    const float* dgamma, float inv_count, const void* relu_bits, void* dy_bf16, long M, int C, void* stream);

/* ---- PraNet path, first kernel: the structure loss of pranet_trainer.py:22-31 on one-channel maps pred / mask fp32
 * [B][H][W]: weit = 1 + 5 |avg_pool31(mask) - mask|, BCE-with-logits averaged over the whole batch (the reference's reduce='none' is read by
 * torch as the legacy reduce=True), weighted IoU per image.  out: float[1 + 2B] = {loss, N_0, D_0, ...} (N = inter + 1, D = union - inter + 1);
 * grad (optional) = grad_scale * d loss / d pred.  Fixed-order sums. */
size_t mi_structure_loss_workspace(int B, int H, int W);
int mi_structure_loss(const float* pred, const float* mask, int B, int H, int W, float* out, float* grad, float grad_scale,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- PraNet path, the network (csrc/gconv.hip, csrc/gnet.hip) ---------------------------------------------------
 * Operands are channel-slice VIEWS of NHWC tensors: a pointer to channel 0 of the slice in pixel 0 and `ld`, the elements per pixel
 * row of the tensor the slice lives in (ld >= channels).  torch.split / torch.cat of the Res2Net bottleneck (Res2Net_v1b.py:68-84),
 * of RFB_modified (PraNet_Res2Net.py:50-54) and of the partial decoder (:84-91) therefore never copy.  Any channel count; alignment
 * only selects the access width (16 / 4 / 2 bytes).  bf16 unless a parameter says fp32.
 *
 * mi_gconv: nn.Conv2d of every shape the path has (kh x kw taps, per-axis stride / padding / dilation, optional bias) and, with
 *   MI_GATHER_DGRAD on the transposed pack, its data gradient.  a [B][Ha][Wa][Ca], out [B][Ho][Wo][N] (the OUTPUT of the launch:
 *   in DGRAD mode that is the forward conv's input shape and a is the forward conv's output gradient).
 *   wp: [kh*kw][roundup(N,32)][roundup(Ca,32)] bf16 from mi_gconv_pack_multi (zero padded).
 *   stats (optional): float[ceil(M/128)][2][N], per 128-pixel tile the column sums and sums of squares of the bf16-rounded outputs -
 *   the first level of nn.BatchNorm2d's batch statistics (PraNet_Res2Net.py:13), finished by mi_gbn_finalize.
 *   out_f32: store fp32 (the one-channel side maps; N <= 32). */
size_t mi_gconv_pack_elems(int O, int I, int kh, int kw);
/* table (device, int64[n_desc][8]) rows: {w_off, wp_off, wpt_off or -1, O, I, kh*kw, first_block, 0}; w_off indexes wflat (fp32 OIHW
 * masters), wp_off / wpt_off the packed forward [t][Opad][Ipad] and data-gradient [t][Ipad][Opad] operands; a block packs 1024 elements,
 * total_blocks = sum ceil(kh*kw*Opad*Ipad / 1024). */
int mi_gconv_pack_multi(const float* wflat, void* wp_bf16, void* wpt_bf16, const int64_t* table_dev, int n_desc, int total_blocks, void* stream);
size_t mi_gconv_stats_elems(int B, int Ho, int Wo, int N);
int mi_gconv(const void* a, long lda, const void* wp, void* out, long ldo, int B, int Ha, int Wa, int Ca, int Ho, int Wo, int N,
             int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int mode, const float* bias, float* stats, int out_f32,
             void* stream);
/* The instance mi_gconv (bn_finalize = 0) or mi_gconv_bn (bn_finalize = 1) launches for these arguments, from the same planning function, on the host
 * (no GPU, no launch; a and out count for their alignment only and are never dereferenced).  route: int[MI_GROUTE_LEN] =
 * {kernel (MI_GROUTE_*), tile width BN, K chunk KC (0 for gconv3), AVEC, OVEC, OUTF32, GEN (general source map), KS (wave groups over K; 0 for gconv3), grid x, grid y}. */
#define MI_GROUTE_GCONV 0     /* gconv_kernel<BN, KC, AVEC, OVEC, OUTF32, GEN, KS> */
#define MI_GROUTE_GCONV3 1    /* gconv3_kernel<BN, AVEC, OVEC> (kernel-row window) */
#define MI_GROUTE_LEN 10
int mi_gconv_route(const void* a, long lda, const void* out, long ldo, int B, int Ha, int Wa, int Ca, int Ho, int Wo, int N, int kh, int kw, int sh, int sw,
                   int ph, int pw, int dh, int dw, int mode, int out_f32, int bn_finalize, int* route);
/* dw[o][i][ky][kx] (+)= sum_m dy[m][o] * x[src(m,ky,kx)][i], fp32 OIHW; split-K slabs summed in a fixed order. */
size_t mi_gconv_wgrad_workspace(int B, int Ho, int Wo, int O, int I, int kh, int kw);
int mi_gconv_wgrad(const void* dy, long ldy, const void* x, long ldx, float* dw, int B, int Ha, int Wa, int I, int Ho, int Wo, int O,
                   int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw_, int accumulate, void* workspace, size_t workspace_bytes, unsigned* tickets, int n_tickets,
                   void* stream);      /* tickets: NULL, or n_tickets zeroed words (left zero): with few K splits the slabs are then added inside the first launch (same bits) */
/* The weight gradients of many convs in one go (the tape of host/pranet.py queues them and flushes once per backward: nothing reads a weight gradient
 * before the optimizer; reference: the autograd of nn.Conv2d.weight, PraNet_Res2Net.py:7-20, hardnet_68.py:56-80).  Each job is mi_gconv_wgrad's argument
 * list; two jobs must not name the same dw.  table_dev: device scratch of mi_gconv_wgrad_multi_table_bytes(n) bytes; workspace: device scratch of
 * mi_gconv_wgrad_multi_workspace(jobs, n) bytes (fp32 split-K slabs of all jobs).  Launches: the table writers (descriptors travel as kernel arguments),
 * one main kernel per operand-alignment class, one reducer.  The K split per job is ~48 steps of 64 pixels (MI_GWM_STEPS) - not mi_gconv_wgrad's split, so the
 * fp32 summation order (not the result beyond rounding) differs from the one-conv call. */
typedef struct MiWgradJob {
    const void* dy; long ldy; const void* x; long ldx; float* dw;
    int B, Ha, Wa, I, Ho, Wo, O, kh, kw, sh, sw, ph, pw, dh, dw_, accumulate;
} MiWgradJob;
size_t mi_gconv_wgrad_multi_table_bytes(int n);
size_t mi_gconv_wgrad_multi_workspace(const MiWgradJob* jobs, int n);
int mi_gconv_wgrad_multi(const MiWgradJob* jobs, int n, void* table_dev, size_t table_bytes, void* workspace, size_t workspace_bytes, void* stream);
/* The weight-gradient instance mi_gconv_wgrad (multi = 0) or a job of mi_gconv_wgrad_multi (multi = 1) launches for these arguments, from the same planning
 * function, on the host (dy and x count for their alignment only).  route: int[MI_GWROUTE_LEN] = {fused (1: gwgrad3 kernel-row kernel, 0: per tap), YVEC, XVEC,
 * K splits S, output pixels per split, workgroups: of the main launch, or (multi) of this job within its class's launch}. */
#define MI_GWROUTE_LEN 6
int mi_gconv_wgrad_route(const void* dy, long ldy, const void* x, long ldx, int B, int Ha, int Wa, int I, int Ho, int Wo, int O, int kh, int kw, int sh, int sw,
                         int ph, int pw, int dh, int dw_, int multi, int* route);
/* nn.BatchNorm2d in train() from the conv's tile statistics: mean, invstd = rsqrt(biased var + eps), scale = gamma * invstd,
 * shift = beta - mean * scale, and the running-statistics update (momentum; unbiased variance), all per channel.  count = pixels. */
int mi_gbn_finalize(const float* partials, int tiles, int C, long count, const float* gamma, const float* beta, float* running_mean, float* running_var,
                    float momentum, float eps, float* mean_out, float* invstd_out, float* scale_out, float* shift_out, void* stream);
/* eval(): scale = gamma * rsqrt(running_var + eps), shift = beta - running_mean * scale */
int mi_gbn_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps, float* scale, float* shift, int C,
                void* stream);
/* out = act(y * scale[c] + shift[c] (+ add)); relu: 0 none, 1 ReLU, 2 ReLU6 (hardnet_68.py:78), any other code is refused; out bf16, or fp32 when
 * out_f32 */
int mi_gbn_apply(const void* y, long ldy, const float* scale, const float* shift, const void* add, long ldadd, void* out, long ldo, int out_f32, long M, int C,
                 int relu, void* stream);
/* mi_gbn_apply (bf16 output) with up to 4 extra destinations (round 5): channels [c0[k], c1[k]) of the result AS STORED (rounded to bf16), plus add2[k] when
 * that is not NULL, also go to the view dst[k] (ldd[k] elements per pixel row; add2[k] likewise a view of c1 - c0 channels).  Replaces the stand-alone copies of
 * a HarDBlock's gathers (reference hardnet_68.py:137-160), the pass-through group of a Res2Net bottleneck and its `sp = sp + spx[i]` (Res2Net_v1b.py:72-84)
 * with bit-identical results.  `out` may be NULL when only the extra destinations are wanted.  The arrays are HOST memory (read during the call). */
int mi_gbn_apply_multi(const void* y, long ldy, const float* scale, const float* shift, const void* add, long ldadd, void* out, long ldo, long M, int C, int relu,
                       int n_extra, const int* c0, const int* c1, void* const* dst, const long* ldd, const void* const* add2, const long* lda2, void* stream);
/* dbeta[c] (+)= sum_m g'[m][c], dgamma[c] (+)= sum_m g'[m][c] * (y[m][c] - mean[c]) * invstd[c]; g' = g where mask > 0 (mask: the layer's
 * ReLU output, or NULL); y NULL: dbeta only (a conv bias gradient).  g fp32 when g_f32; mask_f32 is a flag word: bit 0 = the mask is fp32,
 * bit 1 = the mask is a ReLU6 output (the gradient passes where 0 < mask < 6).  The same flags in mi_gbn_bwd_apply. */
size_t mi_gcolsum_workspace(long M, int C);
int mi_gbn_bwd_sums(const void* g, long ldg, int g_f32, const void* y, long ldy, const void* mask, long ldm, int mask_f32, const float* mean,
                    const float* invstd, long M, int C, float* dbeta, float* dgamma, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* dy = gamma * invstd * (g' - dbeta * inv_count - xhat * dgamma * inv_count) */
int mi_gbn_bwd_apply(const void* g, long ldg, int g_f32, const void* y, long ldy, const void* mask, long ldm, int mask_f32, const float* mean,
                     const float* invstd, const float* gamma, const float* dbeta, const float* dgamma, float inv_count, void* dy, long lddy, long M, int C,
                     void* stream);
/* out = a op b on views.  op: 0 add (sp + spx[i], Res2Net_v1b.py:72; x + crop, PraNet_Res2Net.py:140), 1 mul (partial decoder, :81-83),
 * 2 copy, 3 a where b > 0 else 0 (ReLU backward), 4 relu(a * b) (the gated products of FAM, gcpa_gald.py:88-101; bf16 only).
 * dtype: 0 bf16, 1 fp32, 2 copy fp32 -> bf16, 3 copy bf16 -> fp32. */
int mi_gbinary(int op, int dtype, const void* a, long lda, const void* b, long ldb, void* out, long ldo, long M, int C, void* stream);
/* AvgPool2d(k, stride, pad) with count_include_pad=True (include_pad != 0; Res2Net_v1b.py:40) or AvgPool2d(stride, stride, ceil_mode=True,
 * count_include_pad=False) (include_pad == 0; Res2Net_v1b.py:122-123).  backward != 0: x is d loss / d input (written), out is d loss / d output. */
int mi_gavgpool(const void* x, long ldx, void* out, long ldo, int B, int H, int W, int C, int Ho, int Wo, int k, int stride, int pad, int include_pad,
                int backward, void* stream);
/* MaxPool2d(k, stride, pad) on NHWC bf16 views (hardnet_68.py:213,233); idx: one byte per output element, the winning tap (first maximum in
 * scan order).  backward != 0: x is d loss / d input (written), out is d loss / d output, idx as written by the forward. */
int mi_gmaxpool(const void* x, long ldx, void* out, long ldo, uint8_t* idx, int B, int H, int W, int C, int Ho, int Wo, int k, int stride, int pad, int backward,
                void* stream);
/* CrossEntropyLoss(ignore_index) on NHWC fp32 logits [M][K] (view, K <= 32), labels int64 [M] (gald_trainer.py:66-84).  loss_out: four floats as
 * mi_softmax_ce_fwd (mean over valid pixels, n_valid, out-of-range labels, -).  dlogits (optional, same layout) = d loss / d logits * grad_scale. */
size_t mi_gce_workspace(long M);
int mi_gce(const float* logits, long ld, const int64_t* labels, long M, int K, int ignore_index, float* loss_out, float* dlogits, long ldd, float grad_scale,
           void* workspace, size_t workspace_bytes, void* stream);
/* F.interpolate / nn.Upsample, mode='bilinear' (PraNet_Res2Net.py:67,127-177): src = align_corners ? scale * dst : max(scale * (dst + 0.5) - 0.5, 0).
 * scale_h / scale_w as ATen computes them: align_corners: (in - 1) / (out - 1); otherwise 1 / scale_factor when the caller gave a
 * scale_factor, in / out when it gave a size.  backward != 0: x is d loss / d input (written), out is d loss / d output (gather form,
 * fixed summation order). */
int mi_gresize(const void* x, long ldx, void* out, long ldo, int f32, int B, int H, int W, int C, int Ho, int Wo, int align_corners, float scale_h, float scale_w,
               int backward, void* stream);
/* The kernel instance mi_gresize launches for these arguments, from the planning function the launch itself calls (no GPU, no launch; x and out count for
 * their alignment only and are never dereferenced).  route: int[MI_GRESIZE_ROUTE_LEN] = {kernel (MI_GRESIZE_*), f32, grid size in workgroups of 256}. */
#define MI_GRESIZE_FWD 0          /* gresize_fwd_kernel<T>: thread per output element */
#define MI_GRESIZE_FWD8 1         /* gresize_fwd8_kernel: bf16, thread per (output pixel, 8 channels) */
#define MI_GRESIZE_BWD_GATHER 2   /* gresize_bwd_kernel<T>: thread per source element */
#define MI_GRESIZE_BWD_WAVE 3     /* gresize_bwd_wave_kernel<T>: wave per source element */
#define MI_GRESIZE_BWD_PIX 4      /* gresize_bwd_pix_kernel<T>: wave per source pixel, lanes over the channels */
#define MI_GRESIZE_BWD8 5         /* gresize_bwd8_kernel: bf16, thread per (source pixel, 8 channels) */
#define MI_GRESIZE_ROUTE_LEN 3
int mi_gresize_route(const void* x, long ldx, const void* out, long ldo, int f32, int B, int H, int W, int C, int Ho, int Wo, int align_corners, float scale_h,
                     float scale_w, int backward, int* route);
/* reverse attention (PraNet_Res2Net.py:131-133): out[m][c] = (1 - sigmoid(gate[m])) * feat[m][c], gate fp32 [M]; backward: dfeat and dgate */
int mi_gra_fwd(const float* gate, const void* feat, long ldfeat, void* out, long ldo, long M, int C, void* stream);
int mi_gra_bwd(const float* gate, const void* feat, long ldfeat, const void* dy, long lddy, void* dfeat, long lddf, float* dgate, long M, int C, void* stream);

/* ---- GALD / GCPA path, first kernels (csrc/gald.hip) -----------------------------------------------------------------
 * Depthwise 3x3 convolution with bias on NHWC bf16 views: Conv2d(C, C, 3, groups=C, stride, padding) of LocalAttenModule
 * (core/models/classifiers/gcpacc/contextagg/GALDNet.py:127-141: stride 2, no padding).  w fp32 [C][3][3] (torch's [C,1,3,3]), bias fp32 [C] or NULL.
 * stats (optional): per-128-pixel-tile column sums / sums of squares of the rounded outputs, the layout mi_gbn_finalize takes. */
size_t mi_gdwconv_stats_elems(int B, int Ho, int Wo, int C);
int mi_gdwconv(const void* x, long ldx, const float* w, const float* bias, void* out, long ldo, int B, int H, int W, int C, int Ho, int Wo, int stride, int pad,
               float* stats, void* stream);
int mi_gdwconv_dgrad(const void* dy, long ldy, const float* w, void* dx, long lddx, int B, int H, int W, int C, int Ho, int Wo, int stride, int pad, void* stream);
size_t mi_gdwconv_wgrad_workspace(int B, int Ho, int Wo, int C);
int mi_gdwconv_wgrad(const void* dy, long ldy, const void* x, long ldx, float* dw, float* dbias, int B, int H, int W, int C, int Ho, int Wo, int stride, int pad,
                     int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* Criss-cross attention core (contextagg/ccnet.py:56-127) on the projected q, k [B][H][W][Cq] and v [B][H][W][C]: for every pixel the affinities
 * with its column (own position masked with -inf) and its row, ONE softmax over the H + W candidates (att, fp32 [B][H][W][H+W], kept for the
 * backward pass) and agg = sum_j att_j v_j.  The module's output is gamma * agg + x (mi_gbn_apply with scale = gamma).  H + W <= 512.
 * backward: dagg -> dq, dk, dv; de_ws: float[B*H*W*(H+W)] scratch. */
int mi_gcca_fwd(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, float* att, void* agg, long ldo, int B, int H, int W, int Cq, int C,
                void* stream);
int mi_gcca_bwd(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, const float* att, const void* dagg, long lddagg, float* de_ws, void* dq,
                long lddq, void* dk, long lddk, void* dv, long lddv, int B, int H, int W, int Cq, int C, void* stream);
/* Sigmoid gate of the local attention module (GALDNet.py:150-157).  dout == NULL: o1 = x + x * sigmoid(g).  Otherwise the backward:
 * o1 = d loss / d x = dout * (1 + s), o2 = d loss / d g = dout * x * s * (1 - s). */
int mi_ggate(const void* x, long ldx, const void* g, long ldg, const void* dout, long lddo, void* o1, long ld1, void* o2, long ld2, long M, int C, void* stream);

/* mi_gconv (forward, bf16 out, tile statistics) with BatchNorm2d's finalize done by the launch's last workgroup instead of a second launch
 * (mi_gbn_finalize's arithmetic and results: mean, invstd, scale, shift into fin_out[4][N], running statistics updated), for convs of at most
 * mi_gconv_bn_inlaunch_max_pixels() output pixels - the small maps of the deep stages, where the extra launch cost as much as the conv.
 * tickets: one zeroed 32-bit word per 32 output channels, owned by the caller, left zero by the launch (reusable on the same stream). */
int mi_gconv_bn_inlaunch_max_pixels(void);
int mi_gconv_bn(const void* a, long lda, const void* wp, void* out, long ldo, int B, int Ha, int Wa, int Ca, int Ho, int Wo, int N,
                int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, const float* bias, float* stats, unsigned* tickets, const float* gamma,
                const float* beta, float* running_mean, float* running_var, float momentum, float eps, float* fin_out, void* stream);

/* ---- the general family in the reference's precision (csrc/gf32.hip): evaluation forward of PraNet / GALD in fp32 ------------------------
 * Replaces the eval()-mode forward of core/testers/pranet_tester.py:36 (`self.model(x)`) and core/testers/gald_tester.py:56-57
 * (`self.encoder(x)`, `self.decoder(x, ...)`), whose masks the testers threshold: fp32 NHWC views (pointer to channel 0 + floats per pixel
 * row), weights read from the fp32 OIHW masters, fp32 accumulation on v_mfma_f32_16x16x4_f32 (exact fp32 products: BASELINE's 1e-3 / identical
 * argmax bar).  Forward only.
 * mi_gconv_f32: out = act(((conv(a, w) + bias) * scale + shift) + add): nn.Conv2d (any taps, per-axis stride / padding / dilation) + its bias,
 * BatchNorm2d in eval() as the affine of mi_gbn_fold (scale / shift NULL: none), the residual view (NULL: none), act 0 none | 1 ReLU | 2 ReLU6 -
 * the order of Res2Net_v1b.py:86-92 / PraNet_Res2Net.py:17-20,57-58 / hardnet_68.py:56-80. */
int mi_gconv_f32(const float* a, long lda, const float* w_oihw, const float* bias, const float* scale, const float* shift, const float* add, long ldadd, int act,
                 float* out, long ldo, int B, int Ha, int Wa, int Ca, int Ho, int Wo, int N, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                 void* stream);
/* mode 0: AvgPool2d(k, stride, pad), count_include_pad=True (Res2Net_v1b.py:40); 1: AvgPool2d(stride, stride, ceil_mode=True,
 * count_include_pad=False) (Res2Net_v1b.py:122-123); 2: MaxPool2d(k, stride, pad) (Res2Net_v1b.py:152, hardnet_68.py:213,233) */
int mi_gpool_f32(const float* x, long ldx, float* out, long ldo, int B, int H, int W, int C, int Ho, int Wo, int k, int stride, int pad, int mode, void* stream);
/* depthwise 3x3 + bias + eval()-BatchNorm affine + activation (GALDNet.py:127-141) */
int mi_gdwconv_f32(const float* x, long ldx, const float* w, const float* bias, const float* scale, const float* shift, int act, float* out, long ldo, int B, int H,
                   int W, int C, int Ho, int Wo, int stride, int pad, void* stream);
/* criss-cross attention core (ccnet.py:56-127), forward: out = sum_j softmax_j(q . k_j) v_j over the pixel's column (own position masked) and row */
int mi_gcca_f32(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, float* out, long ldo, int B, int H, int W, int Cq, int C, void* stream);
/* pointwise: op 0 out = act(a * scale[c] + shift[c] (+ b)) (gamma * agg + x of ccnet.py:127); 1 out = (1 - sigmoid(b[m])) * a, b one value per pixel
 * (PraNet_Res2Net.py:131-133); 2 out = a + a * sigmoid(b) (GALDNet.py:150-157); 3 out = relu(a * b) (gcpa_gald.py:88-101) */
int mi_gpoint_f32(int op, const float* a, long lda, const float* b, long ldb, const float* scale, const float* shift, int act, float* out, long ldo, long M, int C,
                  void* stream);

/* ---- the `aspp` input transform of a batch (csrc/augment.hip) ------------------------------------------------------------------------------
 * Replaces the per-image CPU transform of core/components/augment.py:87-120 / core/datasets/transform.py (ColorJitter, Resize | RandomScale +
 * RandomCrop(pad_if_needed), RandomHorizontalFlip, ToTensor, Normalize, through PIL) for decoded uint8 images; the results equal PIL's bit for
 * bit.  Everything random or derived is decided by the host (host/augment.py) and arrives as one MiAugSample per image; images of a batch may
 * differ in size.  A fixed number of launches per batch whatever B is.
 *
 * Byte buffers (img, jit, tmp): 4-byte aligned, readable / writable up to their size rounded up to a multiple of 16.
 *   jit: H*W*3 bytes (only when n_ops > 0).  tmp: (ry1 - ry0) * tstride bytes, tstride = 12 * ceil((cx1 - cx0) / 4) (only when sw != W).
 * Geometry: the image is resampled to sh x sw (PIL BICUBIC: horizontal pass, then vertical, each rounding to uint8; a pass whose size does not
 * change is skipped and its table pointers are NULL); output pixel (y, x) shows resampled pixel (y + off_y, xm + off_x), xm = flip ? out_w-1-x : x,
 * or the fill (image 0, label 255) outside - off_* = crop offset minus padding.  [cy0,cy1) x [cx0,cx1) is the part of the resampled image
 * the output shows, [ry0,ry1) x [rx0,rx1) the source rows / columns those need.  Tables: hcoef [hk][sw], vcoef [vk][sh] fixed point with 22
 * fraction bits, tap-major; hbound [sw][2], vbound [sh][2] = {first source index, taps}.  The label is gathered from the nearest source pixel
 * (PIL NEAREST) of a lab_sh x lab_sw resample with the same off / flip and mapped through lab_table.
 * ops: 1 brightness, 2 contrast, 3 saturation, 4 hue (torchvision ColorJitter on uint8 RGB), applied in order; factor[i] is the blend factor,
 * for hue the amount already as int(f * 255) mod 256 in hue_shift.  grey_sum must be 0 on entry (the contrast op's exact integer sum). */
typedef struct MiAugSample {
    const uint8_t* img;       /* [H][W][3] decoded RGB */
    const uint8_t* lab;       /* [H][W] label ids, NULL: no label */
    uint8_t* jit;
    uint8_t* tmp;
    const int32_t* hcoef;
    const int32_t* hbound;
    const int32_t* vcoef;
    const int32_t* vbound;
    unsigned long long grey_sum;
    int32_t H, W, sh, sw, hk, vk;
    int32_t off_y, off_x, flip;
    int32_t cy0, cy1, cx0, cx1, ry0, ry1, rx0, rx1, tstride;
    int32_t lab_sh, lab_sw;
    int32_t n_ops, op[4], hue_shift;
    float factor[4];
    int32_t to_bgr255;
    float mean[3], std[3];
    uint8_t lab_table[256];
} MiAugSample;
/* table_dev: the B records in device memory (written by the launches: grey_sum); table_host: the same records, read here to validate them and
 * to size the launches.  out_img [B][3][out_h][out_w] fp32, out_lab [B][lab_h][lab_w] fp32 (NULL when no sample has a label). */
int mi_augment_batch(void* table_dev, const void* table_host, int B, int out_h, int out_w, int lab_h, int lab_w, float* out_img, float* out_lab,
                     void* stream);

/* ---- the `pra` input transform of a batch (csrc/augment_pra.hip) ---------------------------------------------------------------------------
 * PraNet's polyp transform (the operations, probabilities and ranges of core/components/augment.py:55-85, the arithmetic defined on PIL; the
 * contract is in DESIGN.md) for decoded uint8 images and grey masks; the results equal PIL's bit for bit.  Everything random or derived is
 * decided by the host (host/pra_augment.py) and arrives as one MiPraSample per image; images of a batch may differ in size.  Four launches
 * per batch whatever B is: gather + colour -> win, horizontal pass -> tmp, vertical pass + normalise, mask.
 *
 * Geometry: sym = 4 * transpose + 2 * flip_rows + flip_cols names one of the eight symmetries of the square; pixel (y, x) of the transformed
 * frame (W x H when transposed, else H x W) is source pixel (fr(a), fc(b)), (a, b) = transpose ? (x, y) : (y, x), fr(a) = flip_rows ? H-1-a : a,
 * fc(b) = flip_cols ? W-1-b : b.  The window [y0, y0 + wh) x [x0, x0 + ww) of the transformed frame is what is resized to out_h x out_w.
 * Colour, per pixel of the window only: when hsv != 0, PIL rgb2hsv, H = (H + hue_shift) & 255, S = lut_s[S], V = lut_v[V], PIL hsv2rgb;
 * then, when bc != 0, every channel through lut_bc.  (The HSV round trip is lossy: it is skipped, not run with zero shifts.)
 * Resize: PIL BILINEAR - horizontal pass, then vertical, each rounding to uint8; a pass whose size does not change is skipped and its table
 * pointers are NULL.  Tables as for mi_augment_batch: hcoef [hk][out_w], vcoef [vk][out_h], 22 fraction bits, tap-major; hbound [out_w][2],
 * vbound [out_h][2] = {first index in the window, taps}; hk / vk must be 2 * ceil(max(in / out, 1)) + 1.
 * Mask: output (y, x) shows window pixel (ny[y], nx[x]) (PIL NEAREST, computed by the host) through mask_table, as float.
 * Byte buffers: 4-byte aligned, readable / writable up to their size rounded up to a multiple of 16.  win: wh * wstride bytes,
 * wstride = 12 * ceil(ww / 4); tmp: wh * tstride bytes, tstride = 12 * ceil(out_w / 4) (only when ww != out_w). */
typedef struct MiPraSample {
    const uint8_t* img;       /* [H][W][3] decoded RGB */
    const uint8_t* mask;      /* [H][W] grey levels, NULL: no mask */
    uint8_t* win;
    uint8_t* tmp;
    const int32_t* hcoef;
    const int32_t* hbound;
    const int32_t* vcoef;
    const int32_t* vbound;
    const int32_t* ny;        /* [out_h] */
    const int32_t* nx;        /* [out_w] */
    int32_t H, W, sym, y0, x0, wh, ww, hk, vk, wstride, tstride;
    int32_t hsv, hue_shift, bc;
    float mean[3], std[3];
    uint8_t lut_s[256], lut_v[256], lut_bc[256], mask_table[256];
} MiPraSample;
/* table_dev: the B records in device memory; table_host: the same records, read here to validate them and to size the launches.
 * out_img [B][3][out_h][out_w] fp32, out_mask [B][out_h][out_w] fp32 (NULL when no sample has a mask). */
int mi_augment_pra_batch(const void* table_dev, const void* table_host, int B, int out_h, int out_w, float* out_img, float* out_mask, void* stream);

/* ---- online self-training: mean teacher + ClassMix (DACS / DAFormer) on the device (csrc/classmix.hip; host/self_train.py AsppClassMix) ----------
 * The three entries are enqueue-only (no host read, no synchronisation; the memsets below are stream-ordered), use no floating-point atomics and
 * are bit-reproducible from run to run.  Bad arguments return MI_EINVAL before anything is enqueued.
 *
 * mi_label_classes: labels [B][H][W] int64 -> present [B] uint32, bit c of present[b] set iff class c in [0, K) occurs in image b.  Values outside
 * [0, K) - the ignore value included - set nothing.  present is zeroed by the entry (whatever it held).  OR within the thread, the wave, the
 * workgroup, then one integer atomic OR per workgroup.  K in 1..32 (K = 32 uses bit 31); two labels per load when H*W is even and labels is
 * 16-byte aligned.  Refused: NULL pointers, B outside 1..65535, H or W < 1, K outside 1..32. */
int mi_label_classes(const int64_t* labels, uint32_t* present, int B, int H, int W, int K, void* stream);

/* mi_classmix: the pseudo-label and mixing pass of one iteration, without the [B][K][H][W] probability map.
 *   src_img, tgt_img, mix_img  [B][3][H][W] fp32      src_lab, mix_lab  [B][H][W] int64      mask  [B][H][W] uint8 or NULL
 *   teacher_low  [B][h][w][K] fp32 NHWC: the teacher head's low-resolution logits of the target images
 *   present      [B] uint32 (mi_label_classes of src_lab)      priority  [B][K] uint8, every row a permutation of 0..K-1 drawn by the host
 *   counts       [B][2] int64, zeroed by the entry
 * chosen(b) = the ceil(n/2) classes of present[b] (bits below K) with the smallest priority[b][c], n their number; n = 0: the empty set.  Every
 * workgroup recomputes it from present and priority: no launch of its own, no round trip through the host.
 * Per pixel: M = src_lab in [0, K) and in chosen(b);  mix_img = M ? src_img : tgt_img (per channel; the other image is not read);
 * mix_lab = M ? src_lab : pseudo;  mask = M;  pseudo = (max_k p_k >= threshold) ? the LOWEST class index among the maxima : ignore_index, with
 * p_k exactly the K values of mi_upsample_predict_score for one source, no mirror, div_a = div_b = 1 (one shared device function: the labels
 * are bit-equal to that entry's pseudo output, 255 there = ignore_index here).  A pasted pixel does not read the teacher's logits.
 * counts[b][0] = pasted pixels, counts[b][1] = unpasted pixels whose pseudo-label was kept: 32-bit sums per workgroup, one 64-bit integer atomic
 * add per counter and workgroup.  mix_img may be a slice of a larger buffer; it must not overlap the inputs.
 * Two pixels per lane when W is even, the images are 8-byte, the labels 16-byte and mask 2-byte aligned.  Traffic per pixel: 8 (label) + 12 (the
 * image shown) read, 12 + 8 (+ 1 with mask) written, plus the low-resolution logits once per 64 pixels at 1/8 resolution.
 * Refused: NULL pointers (mask apart), B outside 1..65535, non-positive sizes, H < h, W < w, K outside 1..32, threshold outside [0, 1] or NaN,
 * ignore_index inside [0, K). */
int mi_classmix(const float* src_img, const float* tgt_img, const int64_t* src_lab, const float* teacher_low, const uint32_t* present,
                const uint8_t* priority, float threshold, int ignore_index, float* mix_img, int64_t* mix_lab, uint8_t* mask, int64_t* counts,
                int B, int h, int w, int K, int H, int W, void* stream);

/* mi_ema_update: teacher[i] = a * teacher[i] + b * student[i] for i < n over flat fp32 stores, a = hyper[0] read from DEVICE memory by the kernel
 * (a captured HIP graph replays with whatever the host wrote there), b the fp32 difference 1.0f - a; both products and the sum are rounded fp32
 * operations (a = 0 copies the student, a = 1 leaves the teacher).  16-byte accesses; any n and any 4-byte alignment of the two pointers: the
 * teacher's 16-byte boundaries hand out the ranges (a scalar head and tail of at most 3 elements each), the student is read at whatever
 * alignment it has.  Refused: NULL pointers, n = 0, a pointer that is not 4-byte aligned. */
int mi_ema_update(float* teacher, const float* student, size_t n, const float* hyper /*[1], device*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif
