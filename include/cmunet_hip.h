/*
 * cmunet_hip.h -- C-ABI of the MI355X (gfx950) CM-UNet hot-path library (libcmunet_hip.so).
 *
 * The reference (CamilleChallier/Contrastive-Masked-UNet) is 100 % Python: the arithmetic of its hot
 * path is dispatched by torch.nn modules into ATen/cuDNN.  There is no FFI in the reference; the
 * entry points below are what a binding for this path replaces, and each one cites the reference
 * call site whose ATen dispatch it stands for (paths relative to /root/reference).
 *
 * Conventions
 *   - plain C: device pointers, sizes, a dtype enum and a hipStream_t (passed as void*); no torch types.
 *   - every function returns 0 on success or a negative CMU_ERR_* code; cmu_last_error() returns a
 *     thread-local message.  Nothing is allocated or freed inside the library; workspaces are passed in
 *     and sized with the cmu_*_ws_bytes() queries.  No global mutable state; re-entrant.
 *   - activations are NHWC with an explicit pixel stride `ld` (elements), so a tensor may be a channel
 *     slice of a wider buffer (the concat-free decoder: UpBlock's torch.cat, Finetuning/model.py:80,
 *     never materialises).  dtype of activations/packed weights = `dt`; parameters, statistics,
 *     gradients of parameters and logits are fp32.
 *   - a "pending transform" (in_scale, in_shift, relu_from) is a training-mode BatchNorm+ReLU that the
 *     producer left un-applied: the consumer applies  v = x*scale[c]+shift[c]; if (c>=relu_from) v=max(v,0)
 *     (relu_from = -n < 0, the 3x3 conv / weight-gradient entries: the channels c < n are the activated ones instead --
 *     a concat view whose activated skip comes FIRST, cmu_conv1x1_nchw_fwd excepted)
 *     while staging its input tile (BatchNorm2d + ReLU of Finetuning/model.py:18-19,21-22 fused into the
 *     next conv / pool / convT load).  in_scale == NULL means identity.
 */
#ifndef CMUNET_HIP_H
#define CMUNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { CMU_F32 = 0, CMU_F16 = 1, CMU_BF16 = 2 } cmu_dtype;

#define CMU_OK 0
#define CMU_ERR_ARG (-1)      /* bad shape / alignment / null pointer */
#define CMU_ERR_UNSUPPORTED (-2)
#define CMU_ERR_WORKSPACE (-3)
#define CMU_ERR_LAUNCH (-4)   /* hipGetLastError() != hipSuccess after a launch */

const char* cmu_last_error(void);
/* name of the compute kernel the calling thread's last GEMM-shaped entry launched ("" if none): for profilers */
const char* cmu_last_kernel(void);
int cmu_version(void);
/* TEST HOOK -- the one piece of process-global mutable state in this library (every other entry is re-entrant and keeps no state
 * between calls: SURVEY section 8b).  Forces one of the library's dispatch knobs (every environment variable it reads: cmu_dispatch_knob_name
 * lists them, tools/README.md says what each does) or hands it back to the environment variable of the same name (value -1; the environment
 * is read once, never on the launch path).  On / off and opt-in knobs take 0 / 1, number knobs any value >= 0.  Documented as bit-identical
 * either way: "CMU_CONV_NARROW", "CMU_CONV_SLIM", "CMU_CONV_PERSIST_PART", "CMU_WGRAD_SQUARE", "CMU_WGRAD_WIDE_F32"; every other knob
 * ("CMU_CONV_V5", the 16x16x32 conv kernel against the 32x32x16 family, "CMU_CONV_V6", "CMU_CONV_WIDE", "CMU_CONV_PERSIST", ...) changes the
 * MFMA shape, the summation order or the split and is equal to rounding only.  The override applies to EVERY thread of the process from the
 * moment it is set: set it while no other thread is launching (the tests are single-threaded); stores and loads of the knob are atomic,
 * calls are serialised by a mutex, a launch in flight on another thread may see either value.  Product code never calls it.
 * Unknown name, or a value outside the knob's range: CMU_ERR_ARG. */
int cmu_set_dispatch_override(const char* name, int value);
/* host-only views of the knob table (no GPU call): the name of row `index` (NULL past the end); the value in effect (override, else
 * environment, else default) and the default of one knob (unknown name: CMU_ERR_ARG) */
const char* cmu_dispatch_knob_name(int index);
int cmu_get_dispatch_knob(const char* name, int* value, int* dflt);
/* element size in bytes of a cmu_dtype */
int cmu_dtype_size(int dt);

/* ---------------------------------------------------------------------------------------------
 * Weight packing (parameters stay in the reference's layouts; packed copies are per-step scratch)
 * ------------------------------------------------------------------------------------------- */
/* nn.Conv2d weight (Cout,Cin,3,3) fp32 -> [chunk][tap][CoutPad][KC] dt for cmu_conv3x3_fwd
 * (Finetuning/model.py:17,20).  transpose_flip=1 packs the data-gradient form
 * w'[tap'][c][n] = w[n][c][2-kh][2-kw] so that cmu_conv3x3_fwd computes dX from dY.            */
int64_t cmu_pack_conv3x3_elems(int Cin, int Cout, int dt, int transpose_flip);
int cmu_pack_conv3x3(const float* w, void* out, int Cin, int Cout, int dt, int transpose_flip, void* stream);
/* nn.ConvTranspose2d weight (Cin,Cout,2,2) fp32 (Finetuning/model.py:60).
 * mode 0: forward form  [chunk(Cin)][1][(ij*Cout+co)Pad][KC]
 * mode 1: data-grad form [chunk(4*Cout: ij*Cout+co)][1][CinPad][KC]                              */
int64_t cmu_pack_convT2x2_elems(int Cin, int Cout, int dt, int mode);
int cmu_pack_convT2x2(const float* w, void* out, int Cin, int Cout, int dt, int mode, void* stream);
/* Every pack of a training step in one launch.  descs_dev: device array of ndesc records of cmu_pack_desc_bytes() bytes
 * { const float* w; void* out; int32 Cin, Cout, mode, kind (0 conv3x3: mode = transpose_flip, 1 convT2x2); int64 total
 * (elements of the packed array); int64 block0 (first of its cmu_pack_desc_blocks(...) workgroups) }, block0 ascending from 0;
 * total_blocks = sum of the workgroup counts.  Same layouts as cmu_pack_conv3x3 / cmu_pack_convT2x2.               */
int cmu_pack_desc_bytes(void);
int64_t cmu_pack_desc_blocks(int kind, int Cin, int Cout, int dt, int mode);
int cmu_pack_batch(const void* descs_dev, int ndesc, int64_t total_blocks, int dt, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Forward
 * ------------------------------------------------------------------------------------------- */
/* (B,H,W) fp32 image -> NHWC 1-channel is the same memory; this entry is the first conv of the
 * network (Cin == 1): Conv2d(1,C,3,p=1) of model.py:96 (down_conv1) computed directly, with the
 * optional patch-mask multiply x*(1-mask) of UNet_encoder.py:156 / spark.py:93-94 fused into the load.
 * mask: uint8 (mask_per_sample ? B : 1, H, W) or NULL.  No bias (BatchNorm follows; see cmu_bn_finalize).
 * stats: [cmu_conv_ntiles][2][Cout] fp32 partial sums (sum, sum of squares) or NULL.               */
int cmu_conv3x3_c1_fwd(const float* x, const uint8_t* mask, int mask_per_sample, const float* w /*(Cout,1,3,3)*/,
                       void* y, int64_t ldy, float* stats, int B, int H, int W, int Cout, int dt, void* stream);

/* Conv2d(Cin,Cout,3,padding=1) as implicit GEMM on MFMA (model.py:17,20), bias-free, with the producer's
 * pending BN+ReLU applied on load and per-tile channel statistics of the raw output in the epilogue. */
int cmu_conv3x3_fwd(const void* x, int64_t ldx, const float* in_scale, const float* in_shift, int relu_from,
                    const void* wpacked, void* y, int64_t ldy, float* stats,
                    int B, int H, int W, int Cin, int Cout, int dt, void* stream);
/* number of spatial tiles (rows of the stats slab) for a (B,H,W) problem */
int cmu_conv_ntiles(int B, int H, int W);

/* BatchNorm2d training statistics (model.py:18,21; eps 1e-5, momentum 0.1): reduces the slab written by
 * a conv into batch mean / biased var, produces the pending transform scale=gamma*invstd,
 * shift=beta-mean*scale, saves mean/invstd for backward and updates running_mean (with the conv bias
 * added back) / running_var (unbiased).  training=0: scale/shift from the running statistics.
 * ws: cmu_bn_finalize_ws_bytes(C) bytes.                                                          */
int64_t cmu_bn_finalize_ws_bytes(int C);
int cmu_bn_finalize(const float* stats, int ntiles, int64_t count, const float* conv_bias, const float* gamma,
                    const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                    int training, float* scale, float* shift, float* save_mean, float* save_invstd,
                    int C, void* ws, void* stream);

/* BN+ReLU apply + MaxPool2d(2) (model.py:40,44): raw conv output -> activated pooled tensor. */
int cmu_bnrelu_maxpool_fwd(const void* y, int64_t ldy, const float* scale, const float* shift,
                           void* out, int64_t ldo, int B, int H, int W, int C, int dt, void* stream);

/* ConvTranspose2d(Cin,Cout,2,stride=2) (model.py:60,78) as GEMM M=B*H*W, N=4*Cout, K=Cin with the
 * pending transform on load, bias added, and a pixel-shuffle store into out (B,2H,2W,ldo) -- normally the
 * left half of the decoder's concat buffer.                                                        */
int cmu_convT2x2_fwd(const void* x, int64_t ldx, const float* in_scale, const float* in_shift, int relu_from,
                     const void* wpacked, const float* bias, void* out, int64_t ldo,
                     int B, int H, int W, int Cin, int Cout, int dt, void* stream);

/* Conv2d(C,K,1) head (model.py:108,130) with pending transform on load: logits (B,K,H,W) fp32 NCHW. */
int cmu_conv1x1_head_fwd(const void* x, int64_t ldx, const float* in_scale, const float* in_shift,
                         const float* w /*(K,C)*/, const float* bias, float* logits,
                         int B, int H, int W, int C, int K, int dt, void* stream);

/* Prediction head: the same Conv2d(C,K,1) + argmax / threshold (+ one class's probability) in one pass; no logits reach memory.
 * Per pixel: logit_k = exactly the bits cmu_conv1x1_head_fwd writes for the same x / transform / w / bias (same chunking, fmaf
 * order and lane butterfly).  K >= 2: label = the smallest k whose logit equals the maximum (torch.argmax on finite values);
 * K == 1: label = logit_0 > logit_threshold (the host passes log(t / (1 - t)) for a probability threshold t).  labels (B,H,W)
 * uint8 receives lut[label] (lut: max(K,2) device bytes), or the label itself when lut is NULL.  prob (B,H,W) f32 or NULL:
 * K >= 2: softmax probability of class prob_class, exp(l_pc - m) / sum_j exp(l_j - m) with m = max_j l_j; K == 1: sigmoid(logit_0)
 * (prob_class must be 0); fp32 with the accurate expf.  A NaN logit gives an unspecified label (one of the lut's values) and an
 * unspecified probability; it never traps.
 * Arguments as cmu_conv1x1_head_fwd: K in 1..8; C / (16 / sizeof(dt)) a power of two <= 64; x 16-byte aligned, ldx a multiple of
 * 16 / sizeof(dt) and >= C; scale / shift both set or both NULL.  labels and prob must be 4-byte aligned (labels are stored four
 * pixels per 32-bit word); 0 <= prob_class < max(K,1) when prob is given.  Every violation returns CMU_ERR_ARG, nothing is launched. */
int cmu_head_predict(const void* x, int64_t ldx, const float* in_scale, const float* in_shift,
                     const float* w /*(K,C)*/, const float* bias /*(K)*/, float logit_threshold, const uint8_t* lut,
                     uint8_t* labels, float* prob, int prob_class, int B, int H, int W, int C, int K, int dt, void* stream);

/* Tiled (sliding-window) prediction with flip / rotation ensembling: three streaming passes (csrc/tiled_predict.hip).
 * Geometry shared by the three: N images of one size (H,W); tiles TH x TW on the canvas max(H,TH) x max(W,TW), at the grid
 * ystarts (ny) x xstarts (nx) (int32 device arrays); A augmented copies per position; tile index
 * ((img * ny + iy) * nx + ix) * A + a.  Dihedral code of a copy: bit 0 flips W, bit 1 flips H, bit 2 transposes; the forward view
 * applies flip W, flip H, transpose in that order, the inverse view undoes them.  Transposing codes need TH == TW.
 *
 * cmu_extract_tiles: src (N,H,W) float32 (src_u8 = 0) or uint8 (1) -> out (N*ny*nx*A, TH, TW) float32: the forward view, under
 * codes[a] (A device bytes; NULL only with A == 1: code 0), of the window at (ystarts[iy], xstarts[ix]).  Window coordinates outside
 * the image are filled by pad_mode: 0 = zero, 1 = reflection without repeating the edge (period 2 (L - 1); L == 1: that pixel).  A
 * copy: exact.  The start arrays are read on the device: any value is safe (folded or zero-filled), a wrong one is a wrong tile.      */
int cmu_extract_tiles(const void* src, int src_u8, int N, int H, int W, const int* ystarts, int ny, const int* xstarts, int nx,
                      const uint8_t* codes, int A, int TH, int TW, int pad_mode, float* out, void* stream);
/* cmu_head_probs: the head of cmu_head_predict (the same logits bit for bit, the same softmax / sigmoid arithmetic) storing every
 * class's probability: probs (n, K', TH, TW) float32 with K' = K for K >= 2 and 1 (the sigmoid) for K == 1.  x holds n tiles of
 * TH x TW pixels in their augmented view; codes (n device bytes, or NULL: all 0) gives each tile's dihedral code, and the tile's
 * planes are stored in the un-augmented frame (the inverse view).  allow_transpose: 1 iff some code may have bit 2 set -- then
 * TH == TW is required (a transposing code met on a non-square tile with allow_transpose = 0 is read without its bit 2).
 * Other arguments and their rules as cmu_head_predict.  Every violation returns CMU_ERR_ARG, nothing is launched.                    */
int cmu_head_probs(const void* x, int64_t ldx, const float* in_scale, const float* in_shift, const float* w /*(K,C)*/,
                   const float* bias /*(K)*/, const uint8_t* codes, int allow_transpose, float* probs, int n, int TH, int TW, int C,
                   int K, int dt, void* stream);
/* cmu_blend_tiles: probs (N*ny*nx*A, K', TH, TW) -> labels (N,H,W) uint8 (+ prob (N,H,W) float32 or NULL).  Per pixel (y, x) the
 * covering tiles are visited in the fixed order iy, ix, a ascending; weight = wy[y - y0] * wx[x - x0] (fp32 windows of TH and TW
 * entries); num[k] = fmaf(weight, p[k], num[k]), den += weight.  K >= 2: label = the smallest k with the largest num[k]; K == 1:
 * label = num[0] / den > threshold (a PROBABILITY threshold, fp32 division).  labels receives lut[label] (max(K,2) device bytes) or
 * the label; prob receives num[prob_class] / den.  No atomics: the same bits on every call.  A pixel that no tile covers has
 * den = 0 (label 0 / lut[0], probability NaN): the caller checks coverage from the start arrays on the host.                        */
int cmu_blend_tiles(const float* probs, int N, int H, int W, const int* ystarts, int ny, const int* xstarts, int nx, int A, int TH,
                    int TW, int K, const float* wy, const float* wx, float threshold, const uint8_t* lut, uint8_t* labels,
                    float* prob, int prob_class, void* stream);

/* pending transform applied, NHWC dt -> NCHW fp32 (module boundary of DoubleConv/DownBlock/UpBlock). */
int cmu_apply_to_nchw(const void* y, int64_t ldy, const float* scale, const float* shift, int relu_from,
                      float* out, int B, int H, int W, int C, int dt, void* stream);
/* NCHW fp32 -> NHWC dt (module boundary, inputs with C > 1) and back for gradients. */
int cmu_nchw_to_nhwc(const float* x, void* out, int64_t ldo, int B, int H, int W, int C, int dt, void* stream);
int cmu_nhwc_to_nchw(const void* x, int64_t ldx, float* out, int B, int H, int W, int C, int dt, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward
 * ------------------------------------------------------------------------------------------- */
/* BatchNorm2d+ReLU backward, phase 1: per-channel sums of dz = dA*[y*scale+shift>0] and dz*xhat.
 * Produces dgamma, dbeta (fp32, overwritten) and coef[2][C] = (sum dz / N, sum dz*xhat / N).      */
int64_t cmu_bn_bwd_ws_bytes(int C);
int cmu_bn_bwd_reduce(const void* dA, int64_t ldd, const void* y, int64_t ldy, const float* scale, const float* shift,
                      const float* save_mean, const float* save_invstd, float* dgamma, float* dbeta, float* coef,
                      int B, int H, int W, int C, int dt, void* ws, void* stream);
/* finalisation of a slab written by a fused producer (cmu_maxpool_bwd / cmu_conv1x1_head_bwd with bn_ws):
 * dgamma, dbeta (nullable) and coef[2][C], summed in row order (bitwise reproducible).                          */
int cmu_bn_bwd_finalize(const void* bn_ws, int64_t count, float* dgamma, float* dbeta, float* coef, int C, void* stream);
/* Same phase-1 result from a per-tile slab [cmu_conv_ntiles][2][C] written by cmu_conv3x3_dgrad_bn /
 * cmu_convT2x2_dgrad_bn.  ws: cmu_bn_finalize_ws_bytes(C).                                                       */
int cmu_bn_bwd_finalize_tiles(const float* bstats, int ntiles, int64_t count, float* dgamma, float* dbeta, float* coef, int C,
                              void* ws, void* stream);
/* Data gradient of Conv2d 3x3 (autograd of model.py:17,20): cmu_conv3x3_fwd on dY with the flipped pack, plus -- in the
 * epilogue, from the stored dX and the raw output ``yraw`` of the conv+BN+ReLU layer that produced the conv's input --
 * that layer's BatchNorm+ReLU backward partial sums (replaces a separate cmu_bn_bwd_reduce pass over dX and yraw).
 * K = channels of dY, N = channels of dX.                                                                        */
int cmu_conv3x3_dgrad_bn(const void* dY, int64_t ldd, const void* wpacked_flip, void* dX, int64_t ldx, const void* yraw, int64_t ldy,
                         const float* scale, const float* shift, const float* save_mean, const float* save_invstd, float* bstats,
                         int B, int H, int W, int K, int N, int dt, void* stream);
/* phase 2: dY = scale * (dz - coef0 - xhat*coef1), written to dY (may alias dA). */
int cmu_bn_bwd_apply(const void* dA, int64_t ldd, const void* y, int64_t ldy, const float* scale, const float* shift,
                     const float* save_mean, const float* save_invstd, const float* coef, void* dY, int64_t ldo,
                     int B, int H, int W, int C, int dt, void* stream);

/* weight gradient of Conv2d 3x3 (autograd of model.py:17,20): dW (Cout,Cin,3,3) fp32, overwritten.
 * x is the layer's input with its pending transform (applied on load).  ws: cmu_conv3x3_wgrad_ws_bytes. */
int64_t cmu_conv3x3_wgrad_ws_bytes(int B, int H, int W, int Cin, int Cout, int dt);
int cmu_conv3x3_wgrad(const void* x, int64_t ldx, const float* in_scale, const float* in_shift, int relu_from,
                      const void* dY, int64_t ldd, float* dW, int B, int H, int W, int Cin, int Cout, int dt,
                      void* ws, void* stream);
/* first layer (Cin == 1): dW (Cout,1,3,3) from the fp32 image (+ optional mask) and dY. */
int64_t cmu_conv3x3_c1_wgrad_ws_bytes(int B, int H, int W, int Cout);
int cmu_conv3x3_c1_wgrad(const float* x, const uint8_t* mask, int mask_per_sample, const void* dY, int64_t ldd,
                         float* dW, int B, int H, int W, int Cout, int dt, void* ws, void* stream);
/* Same with the layer's BatchNorm+ReLU backward applied on the fly: dA is the gradient w.r.t. the activated output, yraw the
 * layer's raw conv output, coef the phase-1 coefficients (cmu_bn_bwd_finalize*).  The first layer has no data gradient, so
 * its dY never has to exist in memory (no cmu_bn_bwd_apply pass for it).                                               */
int cmu_conv3x3_c1_wgrad_bn(const float* x, const uint8_t* mask, int mask_per_sample, const void* dA, int64_t ldd,
                            const void* yraw, int64_t ldy, const float* scale, const float* shift, const float* save_mean,
                            const float* save_invstd, const float* coef, float* dW, int B, int H, int W, int Cout, int dt,
                            void* ws, void* stream);
/* Same, with the raw output recomputed from the image and the layer's forward weights w (Cout,1,3,3) instead of read: the bits
 * cmu_conv3x3_c1_fwd stored (same FMA order, rounded through the storage type), half the HBM traffic of the pass.           */
int cmu_conv3x3_c1_wgrad_bn_w(const float* x, const uint8_t* mask, int mask_per_sample, const void* dA, int64_t ldd,
                              const float* w, const float* scale, const float* shift, const float* save_mean,
                              const float* save_invstd, const float* coef, float* dW, int B, int H, int W, int Cout, int dt,
                              void* ws, void* stream);

/* MaxPool2d(2) backward fused with the skip-branch add: dA = unpool(dP) + dSkip (dSkip may be NULL).
 * The arg-max is recomputed from the raw output + transform (first max in row-major 2x2 order, as ATen). */
/* bn_ws != NULL additionally fuses phase 1 of this layer's BatchNorm backward: the partial sums of
 * dz and dz*xhat over the dA values just written go to the slab bn_ws (cmu_bn_bwd_ws_bytes(C) bytes; a device-side
 * header word holds the row count) -- follow with cmu_bn_bwd_finalize instead of cmu_bn_bwd_reduce.          */
int cmu_maxpool_bwd(const void* dP, int64_t ldp, const void* dSkip, int64_t lds, const void* y, int64_t ldy,
                    const float* scale, const float* shift, void* dA, int64_t lda,
                    const float* save_mean, const float* save_invstd, void* bn_ws,
                    int B, int H, int W, int C, int dt, void* stream);
/* cmu_maxpool_bwd2: the same with a second skip gradient dSkip2 (or NULL) added in fp32 inside the pass -- the skips of CM_UNet's online
 * encoder feed the pixel AND the feature decoder (cmunet.py:121-124 of the reference: autograd sums the two gradients).               */
int cmu_maxpool_bwd2(const void* dP, int64_t ldp, const void* dSkip, int64_t lds, const void* dSkip2, int64_t lds2, const void* y,
                     int64_t ldy, const float* scale, const float* shift, void* dA, int64_t lda,
                     const float* save_mean, const float* save_invstd, void* bn_ws,
                     int B, int H, int W, int C, int dt, void* stream);
/* Round 3 -- the pooled gradient never stored.  cmu_maxpool_bwd2 with dA == NULL (bn_ws required) leaves only the BatchNorm-backward
 * sums; after cmu_bn_bwd_finalize, cmu_maxpool_bwd_apply recomputes dA = unpool(dP) + dSkip (+ dSkip2), rounds it to the storage type
 * as the stored form would have been, and writes dY = scale * (gate * dA - coef[0] - xhat * coef[1]) -- bit-identical to
 * cmu_maxpool_bwd2 + cmu_bn_bwd_apply (the BatchNorm2d + ReLU + MaxPool2d backward of model.py:20-25,42-45), one tensor pass less. */
int cmu_maxpool_bwd_apply(const void* dP, int64_t ldp, const void* dSkip, int64_t lds, const void* dSkip2, int64_t lds2, const void* y,
                          int64_t ldy, const float* scale, const float* shift, const float* save_mean, const float* save_invstd,
                          const float* coef, void* dY, int64_t ldo, int B, int H, int W, int C, int dt, void* stream);

/* SparK's sparse encoder (Pretraining/Spark/encoder.py:20-36 + models/custom.py:152-182: conv * mask -> sparse BN -> ReLU -> MaxPool2d):
 * mask-aware pools, so that the activated + masked copy of a level's second conv output is never materialised.  A pool window lies in
 * one patch (patch side >= 2 px at every pooled level): cmu_bnrelu_maxpool_fwd_masked writes zero for masked windows without reading
 * y, cmu_maxpool_bwd_masked leaves their dA unwritten (the masked BatchNorm-backward passes that follow never read masked positions and
 * write zeros there).  active: (B,f,f) uint8; H = W = f << s, s >= 1.                                                          */
int cmu_bnrelu_maxpool_fwd_masked(const void* y, int64_t ldy, const float* scale, const float* shift, const uint8_t* active, int f,
                                  void* out, int64_t ldo, int B, int H, int W, int C, int dt, void* stream);
int cmu_maxpool_bwd_masked(const void* dP, int64_t ldp, const void* dSkip, int64_t lds, const void* y, int64_t ldy, const float* scale,
                           const float* shift, const uint8_t* active, int f, void* dA, int64_t lda, int B, int H, int W, int C, int dt,
                           void* stream);

/* ConvTranspose2d 2x2 s2 backward.  data: dX (B,H,W,Cin) from dOut (B,2H,2W,ldd) (GEMM K = 4*Cout).
 * weight: dW (Cin,Cout,2,2) and dbias (Cout) fp32, overwritten.                                    */
int cmu_convT2x2_dgrad(const void* dOut, int64_t ldd, const void* wpacked_dgrad, void* dX, int64_t ldx,
                       int B, int H, int W, int Cin, int Cout, int dt, void* stream);
/* cmu_convT2x2_dgrad + the BatchNorm+ReLU backward partial sums of the layer that produced the ConvTranspose's input
 * (see cmu_conv3x3_dgrad_bn).                                                                                     */
int cmu_convT2x2_dgrad_bn(const void* dOut, int64_t ldd, const void* wpacked_dgrad, void* dX, int64_t ldx, const void* yraw,
                          int64_t ldy, const float* scale, const float* shift, const float* save_mean, const float* save_invstd,
                          float* bstats, int B, int H, int W, int Cin, int Cout, int dt, void* stream);
int64_t cmu_convT2x2_wgrad_ws_bytes(int B, int H, int W, int Cin, int Cout, int dt);
int cmu_convT2x2_wgrad(const void* x, int64_t ldx, const float* in_scale, const float* in_shift, int relu_from,
                       const void* dOut, int64_t ldd, float* dW, float* dbias,
                       int B, int H, int W, int Cin, int Cout, int dt, void* ws, void* stream);

/* 1x1 head backward: dX (NHWC dt) = dLogits^T W ; dW (K,C), dbias (K) fp32 overwritten. */
int64_t cmu_conv1x1_head_bwd_ws_bytes(int B, int H, int W, int C, int K);
int cmu_conv1x1_head_bwd(const float* dlogits, const void* x, int64_t ldx, const float* in_scale, const float* in_shift,
                         const float* w, void* dX, int64_t ldo, float* dW, float* dbias,
                         const float* save_mean, const float* save_invstd, void* bn_ws /* optional, as cmu_maxpool_bwd */,
                         int B, int H, int W, int C, int K, int dt, void* ws, void* stream);
/* Second half of the fused form: cmu_conv1x1_head_bwd with dX = NULL and bn_ws set leaves only the parameter gradients and the
 * BatchNorm-backward partial sums of the layer that fed the head (the rank-K input gradient is never stored); after
 * cmu_bn_bwd_finalize this pass recomputes it per pixel from dlogits and writes that layer's dY = scale * (gate * dA - coef[0] -
 * xhat * coef[1]) -- the same bits as cmu_conv1x1_head_bwd (dX stored) + cmu_bn_bwd_apply, 3.2 instead of 5.4 GB at the bench size. */
int cmu_conv1x1_head_bn_apply(const float* dlogits, const void* x, int64_t ldx, const float* in_scale, const float* in_shift,
                              const float* w, const float* save_mean, const float* save_invstd, const float* coef, void* dY,
                              int64_t ldo, int B, int H, int W, int C, int K, int dt, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Losses / pretraining heads
 * ------------------------------------------------------------------------------------------- */
/* CM-UNet masked reconstruction (cmunet_head.py:62-70): target = per-row normalised image (unbiased var,
 * eps 1e-6), loss = sum((pred-target)^2*mask)/sum(mask), pred = logits[:,channel].  Writes loss (1 fp32)
 * and, if dlogits != NULL, d loss*loss_scale / d logits (B,K,H,W) (zero on the other channels).
 * mask uint8 (B,H,W).  ws: cmu_masked_mse_ws_bytes(B,H).                                            */
int64_t cmu_masked_mse_ws_bytes(int B, int H);
/* amp_state (nullable): a cmu_amp_* state whose current scale multiplies loss_scale in dlogits (loss stays unscaled).  */
int cmu_masked_mse_fwd_bwd(const float* logits, int K, int channel, const float* img, const uint8_t* mask,
                           float* loss, float* dlogits, float loss_scale, const void* amp_state, int B, int H, int W, void* ws,
                           void* stream);

/* Finetune criterion (train.py:455; metrics.py:135-180,503): softmax over 2 classes, CE with one-hot
 * (probability) targets averaged over B*H*W, Dice/IoU counters on softmax[:,1] > 0.5 (no gradient: A-4).
 * out[0]=ce, out[1]=dice_loss, out[2]=iou_loss, out[3..5]=tp, sum_pr, sum_gt.  y1h fp64 (B,2,H,W).
 * dlogits (nullable) = d ce / d logits * loss_scale.                                               */
int64_t cmu_softmax_ce_dice_ws_bytes(int B, int H, int W);
int cmu_softmax_ce_dice_fwd_bwd(const float* logits, const double* y1h, float* out, float* dlogits, float loss_scale,
                                int B, int H, int W, void* ws, void* stream);

/* Segmentation criterion for 2 <= K <= 8 classes (metrics.py:135-198,503 with any threshold / ignore_channels / beta / eps):
 * ONE pass over logits (B,K,H,W) fp32 and targets y of the same shape (fp64 if y_is_f64, else fp32; one-hot or any probabilities)
 * plus a fixed-order finalisation (no floating-point atomics: the same bits every run) writes table[1 + 5K] doubles:
 *   table[0]            ce       = mean over B*H*W of -sum_c w_c y_c log_softmax(l)_c  (class_w: K fp32 weights, NULL = ones; the
 *                                  divisor is the pixel count, as nn.CrossEntropyLoss(weight) has it for probability targets)
 *   table[1      + c]   tp_soft  = sum y_c p_c          table[1 +  K + c]   spr_soft = sum p_c
 *   table[1 + 2K + c]   tp_hard  = sum y_c [p_c > t]    table[1 + 3K + c]   spr_hard = sum [p_c > t]
 *   table[1 + 4K + c]   sgt      = sum y_c
 * with p = softmax(l, dim 1) in fp32 and t = threshold.  Every Dice / F-beta / IoU score, soft or thresholded at t, over any kept
 * channels is a few flops on these vectors.  The access width is chosen for the WHOLE tensor, there is no vector body with a
 * scalar tail: for K <= 4 a lane takes 4 consecutive pixels of every plane (16-byte logits loads, 2 x 16-byte fp64 target loads)
 * when H*W % 4 == 0 and logits, y (and dlogits, backward) are 16-byte aligned; for K > 4 it takes 2 (8-byte logits / dlogits
 * accesses, 16-byte fp64 target loads) when H*W % 2 == 0 and the same alignment holds; any other H*W or alignment sends every
 * pixel down the one-pixel-per-lane path (4-byte accesses): same results, lower rate.  ws: cmu_seg_stats_ws_bytes(K) bytes.    */
int64_t cmu_seg_stats_ws_bytes(int K);
int cmu_seg_stats_fwd(const float* logits, const void* y, int y_is_f64, const float* class_w, float threshold, double* table,
                      int B, int K, int H, int W, void* ws, void* stream);
/* Backward of cmu_seg_stats_fwd in one pass: with the upstream gradients of the final loss w.r.t. ce (g_ce, 1 double) and the
 * SOFT counters (g_tp[K], g_spr[K] doubles), all read from device memory (no host sync; a NULL pointer stands for zeros), and
 * G_c = g_tp[c] y_c + g_spr[c]:
 *   dlogits_j = g_ce / (B*H*W) * (p_j sum_c w_c y_c - w_j y_j) + p_j (G_j - sum_c p_c G_c)          (fp32, (B,K,H,W))
 * p is the forward's fp32 softmax; the combination runs in fp64.  The thresholded counters carry no gradient (SURVEY A-4).     */
int cmu_seg_stats_bwd(const float* logits, const void* y, int y_is_f64, const float* class_w, const double* g_ce,
                      const double* g_tp, const double* g_spr, float* dlogits, int B, int K, int H, int W, void* stream);

/* Element-wise losses of metrics.py:495-551 (nn.L1Loss / MSELoss / BCELoss / BCEWithLogitsLoss) as ONE streaming pass each way, with
 * the conventions of cmu_seg_stats_fwd / _bwd: x fp32, y fp64 if y_is_f64 else fp32, per-lane fp64 accumulation -> block partials in
 * ws -> a fixed-order finalisation (no floating-point atomics: the same bits every call), grid-stride loops under a block cap, 64-bit
 * indexing, no host synchronisation.  The tensor is viewed as (outer, C, inner), 1 <= C <= CMU_PWL_MAX_C; the optional per-channel
 * fp32 vectors chan_w[C] (a factor on the term) and chan_pw[C] (BCE_WITH_LOGITS's pos_weight; any other kind: CMU_ERR_ARG) are
 * indexed by (i / inner) % C, NULL = ones.  The forward writes out[0] = S = sum_i w_c term_i, the backward
 * dx_i = (float)(g[0] w_c dterm_i) with g one double read from DEVICE memory (NULL = zero); the caller applies 1/N for 'mean' as an
 * op on the device scalar, so that autograd hands it back in g.  With c = 1 + (pw_c - 1) y:
 *   kind                      term                                                      dterm
 *   CMU_PWL_L1                |x - y|                                                   sign(x - y), 0 at ties
 *   CMU_PWL_MSE               (x - y)^2                                                 2 (x - y)
 *   CMU_PWL_BCE               -[y max(log x, -100) + (1 - y) max(log(1 - x), -100)]      (x - y) / max(x (1 - x), 1e-12)
 *   CMU_PWL_BCE_WITH_LOGITS   (1 - y) x + c (log1p(e^-|x|) + max(-x, 0))                (1 - y) - c sigmoid(-x)
 * (torch's own clamps).  A BCE prediction outside [0, 1] gives a NaN sum, not an error (raising would need a host sync).  The
 * transcendental of a term is taken in fp32 on the fp32 prediction in a form that keeps its relative precision where it is tiny
 * (log1p(-x), e^-|x| / (1 + e^-|x|)); its combination with y, the weights and g runs in fp64, without cancellation for 0 <= y <= 1.
 * The access width is chosen for the WHOLE tensor: a lane takes 4 consecutive elements (16-byte accesses) when inner % 4 == 0 -- so
 * that the 4 share a channel -- and x, y (and dx, backward) are 16-byte aligned, one element otherwise.
 * ws: cmu_pointwise_loss_ws_bytes() bytes.                                                                                        */
#define CMU_PWL_L1 0
#define CMU_PWL_MSE 1
#define CMU_PWL_BCE 2
#define CMU_PWL_BCE_WITH_LOGITS 3
#define CMU_PWL_MAX_C 8
int64_t cmu_pointwise_loss_ws_bytes(void);
int cmu_pointwise_loss_fwd(int kind, const float* x, const void* y, int y_is_f64, const float* chan_w, const float* chan_pw,
                           double* out, int64_t outer, int C, int64_t inner, void* ws, void* stream);
int cmu_pointwise_loss_bwd(int kind, const float* x, const void* y, int y_is_f64, const float* chan_w, const float* chan_pw,
                           const double* g, float* dx, int64_t outer, int C, int64_t inner, void* stream);

/* Cross entropy / negative log-likelihood with CLASS-INDEX targets (nn.CrossEntropyLoss / nn.NLLLoss under metrics.py:511-543) of
 * x (B,K,H,W) fp32, 2 <= K <= 8, same conventions.  target_kind names what ``target`` holds:
 *   CMU_ICE_LABEL_*   one label plane (B,H,W) of int64 / int32 / uint8 / fp32 / fp64, truncated to an integer as .long() does
 *   CMU_ICE_ONEHOT_*  K planes (B,K,H,W) of fp32 / fp64; the label is the arg-max over the channels of keep_mask (bit c = channel c;
 *                     the first maximum wins, an all-zero pixel gives the first kept channel, as torch.argmax does)
 * x holds logits -- log p = log_softmax over ALL K channels, taken here -- or, with log_input != 0, log-probabilities used as they
 * are.  keep_mask (label targets: pass (1 << K) - 1) also selects the channels of the third sum.  class_w: K fp32 weights, NULL = ones.
 * A pixel whose label equals ignore_index adds nothing.  The forward writes table[3] doubles over the other pixels:
 *   table[0] = sum w_t (-log p_t)      table[1] = sum w_t      table[2] = sum over kept c of w_c (-log p_c)
 * from which torch's reductions follow on the device, with label smoothing e:  'mean' = (1 - e) T0 / T1 + (e / K) T2 / T1  (NaN when
 * every pixel is ignored, as in torch),  'sum' = (1 - e) T0 + (e / K) T2.  The backward takes g[2] = (d/dT0, d/dT2) from DEVICE memory
 * (NULL = zeros) and writes dx (B,K,H,W) fp32: g0 w_t (p_j - [j == t]) + g2 (p_j sum_kept w_c - [j kept] w_j) for logits,
 * -g0 w_t [j == t] - g2 [j kept] w_j for log_input; zeros at ignored pixels.
 * A label outside [0, K) that is not ignore_index is never used as an index: that pixel adds NaN to table[0] and gets a zero gradient
 * (torch asserts on the device there).  -log p_c = (max - l_c) + log1p(sum of the other e^(l - max)), the difference in fp64: a
 * confident pixel's tiny loss keeps its relative precision.  Pixels per lane: 4 (K <= 4) or 2 (K > 4) when H*W is a multiple of
 * that and x, target (and dx, backward) are 16-byte aligned, else 1 -- for the whole tensor.  ws: cmu_index_ce_ws_bytes() bytes.     */
#define CMU_ICE_LABEL_I64 0
#define CMU_ICE_LABEL_I32 1
#define CMU_ICE_LABEL_U8 2
#define CMU_ICE_LABEL_F32 3
#define CMU_ICE_LABEL_F64 4
#define CMU_ICE_ONEHOT_F32 5
#define CMU_ICE_ONEHOT_F64 6
int64_t cmu_index_ce_ws_bytes(void);
int cmu_index_ce_fwd(const float* x, const void* target, int target_kind, int log_input, int keep_mask, const float* class_w,
                     int64_t ignore_index, double* table, int B, int K, int H, int W, void* ws, void* stream);
int cmu_index_ce_bwd(const float* x, const void* target, int target_kind, int log_input, int keep_mask, const float* class_w,
                     int64_t ignore_index, const double* g, float* dx, int B, int K, int H, int W, void* stream);

/* CM-UNet in-batch InfoNCE (cmunet_head.py:72-88): pred (B,D) raw predictor output (L2-normalised inside),
 * keys (N,D) gathered, already normalised target projections; label i + B*rank; loss = ct_w*2*t*CE.
 * dpred (nullable) = d loss / d pred (B,D).  loss: 1 + B floats (loss[0] total, loss[1+b] per-row terms).     */
int cmu_infonce_inbatch_fwd_bwd(const float* pred, const float* keys, float* loss, float* dpred,
                                int B, int N, int D, int rank, float temperature, float ct_weight, void* stream);

/* MoCo-v2 InfoNCE + momentum-queue update in ONE launch (moco2_module.py:256-285, 160-175):
 * q_raw,k_raw (B,D) encoder outputs (normalised inside); queue (D,K) fp32; logits = [q.k, q@queue]/t,
 * CE with label 0 on the PRE-enqueue queue; then queue[:, ptr:ptr+Nk] = keys_all^T (keys_all (Nk,D),
 * the all-gathered normalised keys; may be NULL on one rank = normalised k_raw) and *ptr=(ptr+Nk)%K.
 * dq (nullable) = d loss / d q_raw.  k_norm_out (nullable, (B,D)) receives normalised keys.
 * One persistent launch of five phases with grid-wide barriers (row norms; logits = q . queue as a skinny MFMA GEMM; row
 * softmax + loss; gradient = p . queue^T as a second skinny GEMM split over K; dq, enqueue, pointer), every phase spread over
 * all workgroups, fixed-order sums.  K % 4 == 0.  ws: cmu_moco_ws_bytes(B, D, K) bytes, 16-byte aligned.                  */
int64_t cmu_moco_ws_bytes(int B, int D, int K);
int cmu_moco_infonce_enqueue(const float* q_raw, const float* k_raw, const float* keys_all, int Nk,
                             float* queue, int64_t* queue_ptr, float* loss, float* dq, float* k_norm_out,
                             int B, int D, int K, float temperature, void* ws, void* stream);
/* L2-normalise rows (F.normalize(dim=1), eps 1e-12) -- used before the key all-gather. */
int cmu_l2_normalize_rows(const float* x, float* out, int B, int D, void* stream);
/* The NON-fused MoCo API (moco2_module.py:224-285 ``forward`` / ``_compute_l_s``, :311-329 ``validation_step``; round 5: no ATen op left in
 * those paths).  All fp32, one workgroup per row, fixed-order sums.
 *   cmu_l2_normalize_rows_bwd: backward of F.normalize(x, dim=1) (:256, :259): dx = dy / n - x (x . dy) / n^3, n = |x| (dy / eps below the clamp)
 *   cmu_moco_logits_assemble:  logits (B, 1 + K) = [ q[b] . k[b] | lneg[b][:] ] * inv_t   (torch.cat([l_pos, l_neg], 1) / T, :258-267)
 *   cmu_moco_logits_split / _addpos: its backward -- dlneg (B, K) = dlogits[:, 1:] * inv_t (operand of dq = dlneg @ queue^T), then
 *                              dq[b] += dlogits[b][0] * inv_t * k[b]
 *   cmu_row_cross_entropy:     F.cross_entropy(logits (B, N), target int64 (B)) with mean reduction (:283, :324): loss[0], row_loss[B],
 *                              dlogits (optional) = (softmax - onehot) / B, rank (optional) [b] = number of logits strictly above the
 *                              target's (pl_bolts precision_at_k, metrics/aggregation.py:19-32: hit iff rank < k)
 *   cmu_scale_by_device_scalar: v[i] *= s[0], s on the device (the incoming gradient of a scalar loss) */
int cmu_l2_normalize_rows_bwd(const float* x, const float* dy, float* dx, int B, int D, void* stream);
int cmu_moco_logits_assemble(const float* q, const float* k, const float* lneg, float* logits, int B, int D, int K, float inv_t, void* stream);
int cmu_moco_logits_split(const float* dlogits, float* dlneg, int B, int K, float inv_t, void* stream);
int cmu_moco_logits_addpos(const float* dlogits, const float* k, float* dq, int B, int D, int K, float inv_t, void* stream);
int cmu_row_cross_entropy(const float* logits, const int64_t* target, float* loss, float* row_loss, float* dlogits, int* rank, int B, int N,
                          void* stream);
int cmu_scale_by_device_scalar(float* v, const float* s, int64_t n, void* stream);
/* SparK.patchify / unpatchify (Pretraining/Spark/spark.py:133-148), fp32: inverse 0: src (B, C, h*p, w*p) -> dst (B, h*w, p*p*C) with
 * dst[b][hy*w + wx][(py*p + px)*C + c] = src[b][c][hy*p + py][wx*p + px]; inverse 1: the other way round (src is the patch tensor). */
int cmu_patchify(const float* src, float* dst, int B, int C, int h, int w, int p, int inverse, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SparK sparse (masked) convolution support (Pretraining/Spark/encoder.py:12-56, spark.py:88-131).
 * `active` = (B,f,f) uint8 patch map; a (H,W) level with H = f << s looks up active[b][y>>s][x>>s].
 * ------------------------------------------------------------------------------------------- */
/* per-channel sum / sum-of-squares over the selected pixels (active, or non-active if invert): the statistics of
 * sp_bn_forward (encoder.py:26-36) and the mask-token gradient.  slab: [cmu_masked_stats_rows()][2][C] fp32,
 * fully written; feed it to cmu_bn_finalize with count = number of selected pixels.                       */
int cmu_masked_stats_rows(void);
int cmu_masked_channel_stats(const void* x, int64_t ldx, const uint8_t* active, int f, int invert, float* slab,
                             int B, int H, int W, int C, int dt, void* stream);
/* out = selected ? (relu ? max(x*scale+shift,0) : x*scale+shift) : fill[c]   (scale/shift/fill nullable = 1/0/0):
 * sparse BN apply + ReLU with zeros at masked positions, `x *= active` (encoder.py:20-23), densify with mask
 * tokens torch.where(active, feat, token) (spark.py:103-107), and their gradients.                         */
int cmu_mask_select(const void* x, int64_t ldx, const float* scale, const float* shift, int relu, const uint8_t* active,
                    int f, int invert, const float* fill, void* out, int64_t ldo, int B, int H, int W, int C, int dt,
                    void* stream);
/* BatchNorm backward restricted to the active positions (autograd of sp_bn_forward): count = number of active
 * pixels; masked positions contribute nothing and receive dY = 0.                                          */
int cmu_bn_bwd_reduce_masked(const void* dA, int64_t ldd, const void* y, int64_t ldy, const float* scale, const float* shift,
                             const float* save_mean, const float* save_invstd, float* dgamma, float* dbeta, float* coef,
                             const uint8_t* active, int f, int64_t count, int B, int H, int W, int C, int dt, void* ws,
                             void* stream);
int cmu_bn_bwd_apply_masked(const void* dA, int64_t ldd, const void* y, int64_t ldy, const float* scale, const float* shift,
                            const float* save_mean, const float* save_invstd, const float* coef, void* dY, int64_t ldo,
                            const uint8_t* active, int f, int B, int H, int W, int C, int dt, void* stream);
/* Tile skipping for the sparse encoder (K17; Spark/encoder.py:20-23 computes the dense op and multiplies by the mask --
 * here the masked tiles are never computed).  cmu_sparse_tile_list writes, in ascending order, the indices (dense numbering
 * (b * tilesY + ty) * tilesX + tx) of the tile_h x tile_w pixel tiles of a (B, H, W) level that overlap an active patch,
 * and their number to count[0] -- both on the device: the consumers read the count there, nothing synchronises with the host.
 * list: B * ceil(H / tile_h) * ceil(W / tile_w) ints.
 *   cmu_conv3x3_fwd_tiles   cmu_conv3x3_fwd (forward and, with the flipped pack, data gradient) over a 16 x 32 tile list;
 *                           y outside the listed tiles is left untouched (its consumers select by the mask).  Shapes the
 *                           persistent kernel serves (cmu_conv3x3_tiles_supported != 0): whole tiles, whole channel blocks.
 *   cmu_conv3x3_wgrad_tiles cmu_conv3x3_wgrad with the contraction restricted to a tile list (dY is zero elsewhere): 16 x 16 tiles
 *                           (tile_h 16, the first kernel) or 8 x 16 tiles (tile_h 8, the wide kernel: cmu_conv3x3_wgrad_tile_h).
 *
 * Gather form for the levels whose patches are smaller than a tile (every dense tile holds an active pixel there): the
 * convolution over the LIST of active pixels -- GEMM rows = active pixels (rows[r] = dense pixel index (b*H + y)*W + x, patch-
 * major, written with its count by cmu_sparse_pixel_list), K = 9 taps x Cin gathered per tap from the dense NHWC input (masked
 * neighbours hold zeros there), outputs scattered to y at the listed pixels, the rest of y untouched.  FLOPs = active fraction
 * of the dense launch.  Same packed weights as cmu_conv3x3_fwd (flipped pack: data gradient).
 *   cmu_conv3x3_rows_supported  Cout % 128 == 0, Cin a whole number of 128-byte steps, input tensor below 2 GiB
 *   cmu_sparse_pixel_list       rows[0 .. capacity) (entries past the end = -1), count[0] = min(active pixels, capacity): a capacity
 *                               below the number of active pixels keeps the first `capacity` rows; ws: cmu_sparse_pixel_list_ws_bytes(B, f)
 *   cmu_conv3x3_fwd_rows        max_rows: upper bound of *n_rows known to the host (sizes the grid; surplus workgroups exit)   */
int cmu_sparse_tile_list(const uint8_t* active, int f, int B, int H, int W, int tile_h, int tile_w, int* list, int* count, void* stream);
/* cmu_masked_channel_stats / cmu_bn_bwd_reduce_masked over the list of active pixels: only the listed pixels are visited. */
int cmu_rows_channel_stats(const void* x, int64_t ldx, const int* rows, const int* n_rows, float* slab, int B, int H, int W, int C, int dt,
                           void* stream);
int cmu_bn_bwd_reduce_rows(const void* dA, int64_t ldd, const void* y, int64_t ldy, const float* scale, const float* shift,
                           const float* save_mean, const float* save_invstd, float* dgamma, float* dbeta, float* coef, const int* rows,
                           const int* n_rows, int64_t max_rows, int64_t count, int B, int H, int W, int C, int dt, void* ws, void* stream);
int64_t cmu_sparse_pixel_list_ws_bytes(int B, int f);
int cmu_sparse_pixel_list(const uint8_t* active, int f, int B, int H, int W, int* rows, int64_t capacity, int* count, void* ws, void* stream);
/* Every list of a step in one launch each (the mask is known before the step starts): cmu_sparse_tile_lists builds n <=
 * cmu_sparse_tile_lists_max() tile lists (entry i: level side H[i] = f << s, tiles tile_h[i] x tile_w[i], lists[i] / counts[i] as in
 * cmu_sparse_tile_list -- element for element the same lists); cmu_sparse_pixel_lists expands ONE patch list (a tile list with tiles
 * of one patch, e.g. H = f and 1 x 1 tiles) into the pixel lists of n levels, exactly as cmu_sparse_pixel_list writes them.
 * H, tile_h, tile_w, lists, counts, rows, capacity are HOST arrays of length n.                                              */
int cmu_sparse_tile_lists_max(void);
int cmu_sparse_tile_lists(const uint8_t* active, int f, int B, int n, const int* H, const int* tile_h, const int* tile_w, int* const* lists,
                          int* const* counts, void* stream);
int cmu_sparse_pixel_lists(const int* patches, const int* patch_count, int f, int B, int n, const int* H, int* const* rows,
                           const int64_t* capacity, int* const* counts, void* stream);
/* Patch-organised forms of the sparse encoder's element-wise passes (csrc/sparse_elem.hip; Spark/encoder.py:12-56, spark.py:98-111):
 * the unit of work is a group of patch rows, the branch on the patch's bit is uniform per workgroup, masked patches cost no loads.
 * Outputs at active positions are bit-identical to the pixel-organised entries named beside them.
 *   cmu_cells_supported        square level with H = f << s and a power-of-two number (<= 256) of 16-byte chunks per pixel
 *   cmu_bn_bwd_apply_cells     = cmu_bn_bwd_apply_masked; ring = 1: zeros are written only to the one-pixel border frame of each masked
 *                              patch (enough when every consumer of dY is list-driven: they read active patches + a one-pixel halo;
 *                              the interior of masked patches stays unwritten)
 *   cmu_mask_select_cells      = cmu_mask_select(invert 0): relu?(x * scale + shift) in active patches, elsewhere zeros (ring as above) or fill[c]
 *                              (nullable; the densify step's mask tokens, spark.py:103-107)
 *   cmu_maxpool_bwd_cells      = cmu_maxpool_bwd_masked: active patches only, dA elsewhere unwritten (H / f >= 2)
 *   cmu_cells_channel_sum      out[c] = sum of x over the pixels of the active (invert 0) / masked (invert 1) patches -- the mask-token
 *                              gradient of spark.py:104-108; fixed-order fp32 partial sums, double final; ws: cmu_cells_channel_sum_ws_bytes(C) */
/* The first layer (Conv2d(1, Cout, 3, p=1), Finetuning/model.py:17) over a list of 16 x 16 tiles (cmu_sparse_tile_list numbering) for the
 * sparse encoder: cmu_conv3x3_c1_fwd_tiles computes the listed tiles only (y elsewhere untouched); stats, if given, is
 * [cmu_conv3x3_c1_fwd_tiles_rows(max_tiles)][2][Cout], fully written -- when the patches are multiples of 16 pixels these are the
 * sparse BatchNorm statistics.  cmu_conv3x3_c1_wgrad_bn_tiles = cmu_conv3x3_c1_wgrad_bn (yraw) / cmu_conv3x3_c1_wgrad_bn_w (w) with the
 * contraction restricted to the listed tiles: no masked BatchNorm-backward apply pass, no dY tensor.  max_tiles: host-side upper bound
 * of tile_count[0].  ws: cmu_conv3x3_c1_wgrad_ws_bytes.                                                                       */
int cmu_conv3x3_c1_fwd_tiles_rows(int64_t max_tiles);
int cmu_conv3x3_c1_fwd_tiles(const float* x, const uint8_t* mask, int mask_per_sample, const float* w, void* y, int64_t ldy, float* stats,
                             const int* tile_list, const int* tile_count, int64_t max_tiles, int B, int H, int W, int Cout, int dt,
                             void* stream);
int cmu_conv3x3_c1_wgrad_bn_tiles(const float* x, const uint8_t* mask, int mask_per_sample, const void* dA, int64_t ldd, const void* yraw,
                                  int64_t ldy, const float* w, const float* scale, const float* shift, const float* save_mean,
                                  const float* save_invstd, const float* coef, const int* tile_list, const int* tile_count,
                                  int64_t max_tiles, float* dW, int B, int H, int W, int Cout, int dt, void* ws, void* stream);
int cmu_cells_supported(int B, int H, int W, int f, int C, int dt);
int cmu_bn_bwd_apply_cells(const void* dA, int64_t ldd, const void* y, int64_t ldy, const float* scale, const float* shift,
                           const float* save_mean, const float* save_invstd, const float* coef, void* dY, int64_t ldo,
                           const uint8_t* active, int f, int ring, int B, int H, int W, int C, int dt, void* stream);
int cmu_mask_select_cells(const void* x, int64_t ldx, const float* scale, const float* shift, int relu, const uint8_t* active, int f,
                          int ring, const float* fill, void* out, int64_t ldo, int B, int H, int W, int C, int dt, void* stream);
int cmu_maxpool_bwd_cells(const void* dP, int64_t ldp, const void* dSkip, int64_t lds, const void* y, int64_t ldy, const float* scale,
                          const float* shift, const uint8_t* active, int f, void* dA, int64_t lda, int B, int H, int W, int C, int dt,
                          void* stream);
/*   cmu_cells_channel_stats    = cmu_masked_channel_stats(invert 0) / cmu_rows_channel_stats: slab [cmu_cells_stats_rows()][2][C], fully written
 *   cmu_bn_bwd_reduce_cells    = cmu_bn_bwd_reduce_masked / cmu_bn_bwd_reduce_rows (same sums in another fixed order); ws: cmu_bn_bwd_ws_bytes(C) */
int cmu_cells_stats_rows(void);
int cmu_cells_channel_stats(const void* x, int64_t ldx, const uint8_t* active, int f, float* slab, int B, int H, int W, int C, int dt,
                            void* stream);
int cmu_bn_bwd_reduce_cells(const void* dA, int64_t ldd, const void* y, int64_t ldy, const float* scale, const float* shift,
                            const float* save_mean, const float* save_invstd, float* dgamma, float* dbeta, float* coef,
                            const uint8_t* active, int f, int64_t count, int B, int H, int W, int C, int dt, void* ws, void* stream);
int64_t cmu_cells_channel_sum_ws_bytes(int C);
int cmu_cells_channel_sum(const void* x, int64_t ldx, const uint8_t* active, int f, int invert, float* out, void* ws, int B, int H, int W,
                          int C, int dt, void* stream);
int cmu_conv3x3_rows_supported(int B, int H, int W, int Cin, int Cout, int dt);
int cmu_conv3x3_fwd_rows(const void* x, int64_t ldx, const void* wpacked, void* y, int64_t ldy, const int* rows, const int* n_rows,
                         int64_t max_rows, int B, int H, int W, int Cin, int Cout, int dt, void* stream);
int cmu_conv3x3_tiles_supported(int B, int H, int W, int Cin, int Cout, int dt);
int cmu_conv3x3_fwd_tiles(const void* x, int64_t ldx, const float* in_scale, const float* in_shift, int relu_from,
                          const void* wpacked, void* y, int64_t ldy, const int* tile_list, const int* tile_count,
                          int B, int H, int W, int Cin, int Cout, int dt, void* stream);
/* tile height of the list cmu_conv3x3_wgrad_tiles wants for this shape: 8 (8 x 16 pixel tiles: the wide weight-gradient kernel
 * serves it) or 16 (16 x 16 tiles: the first kernel)                                                                       */
int cmu_conv3x3_wgrad_tile_h(int B, int H, int W, int Cin, int Cout, int dt);
int cmu_conv3x3_wgrad_tiles(const void* x, int64_t ldx, const float* in_scale, const float* in_shift, int relu_from,
                            const void* dY, int64_t ldd, float* dW, const int* tile_list, const int* tile_count, int tile_h,
                            int B, int H, int W, int Cin, int Cout, int dt, void* ws, void* stream);

/* SparK loss (spark.py:112-123): p x p patches, target patch normalised with its own mean / unbiased variance
 * (eps 1e-6), l2 = patch mean of (rec-target)^2, loss = sum over NON-active patches / (count + 1e-8).
 * rec, img (B,f*p,f*p) fp32; drec nullable.  ws: cmu_spark_loss_ws_bytes(B,f).                              */
int64_t cmu_spark_loss_ws_bytes(int B, int f);
int cmu_spark_loss_fwd_bwd(const float* rec, const float* img, const uint8_t* active, float* loss, float* drec,
                           float loss_scale, int B, int f, int p, void* ws, void* stream);

/* Global average pool of the activated latent (moco_data_module.py:65, x.mean([2,3])): out (B,C) fp32 from the
 * raw NHWC tensor + pending transform; backward broadcasts dout/(H*W) into dA (gradient w.r.t. the activation). */
int cmu_gap_fwd(const void* y, int64_t ldy, const float* in_scale, const float* in_shift, float* out,
                int B, int H, int W, int C, int dt, void* stream);
int cmu_gap_bwd(const float* dout, void* dA, int64_t ldd, int B, int H, int W, int C, int dt, void* stream);

/* EMA p_t = m*p_t + (1-m)*p_o over a flat fp32 arena (cmunet.py:78-92, moco2_module.py:153-158). */
int cmu_ema_update(float* target, const float* online, int64_t n, float momentum, void* stream);

/* Fused Adam/AdamW step over a flat fp32 arena (torch.optim.Adam, train.py:341; AdamW cmunet_config.py:79-83).
 * decoupled != 0: AdamW (p *= 1 - lr*wd) else L2 (g += wd*p).  wd_mask (nullable, uint8 per element):
 * weight decay applies where mask != 0 (bias / norm parameters are excluded, cmunet_config.py:84-91).
 * grad_scale multiplies the gradient first (loss-scale removal / DP mean).
 * amp_state (nullable, cmu_amp_*): the update is skipped when the state's found_inf flag is set, the gradient is divided
 * by the state's scale, and the step number of the bias corrections is the state's count of updates taken + 1 (``step``
 * is ignored) -- GradScaler.step / unscale_ without a host round trip.                               */
int cmu_adam_step(float* p, const float* g, float* m, float* v, const uint8_t* wd_mask, int64_t n,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled,
                  int64_t step, float grad_scale, const void* amp_state, void* stream);

/* cmu_adam_step + the EMA of the momentum networks in ONE pass over the arena: what the reference runs as AdamW.step
 * (cmunet_config.py:76-91) followed by MomentumUpdateHook.after_train_iter -> CM_UNet.momentum_update (cmunet.py:78-92,
 * momentum_update_hook.py:42-47).  Up to two ascending, disjoint element ranges [seg_lo[k], seg_hi[k]) of the online arena
 * (multiples of 4) have a target array seg_target[k] (16-byte aligned, hi - lo elements): after the element's AdamW update,
 * target = target*m + p_new*(1-m).  A step skipped by amp_state still runs the EMA with the unchanged parameters (the hook
 * runs behind a skipped optimiser step too).  n must be a multiple of 4, all arenas 16-byte aligned, wd_mask 4-byte aligned.
 * Bit-identical to cmu_adam_step followed by cmu_ema_update per segment.                                             */
int cmu_adam_ema_step(float* p, const float* g, float* m, float* v, const uint8_t* wd_mask, int64_t n,
                      float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled,
                      int64_t step, float grad_scale, const void* amp_state, int nseg, const int64_t* seg_lo,
                      const int64_t* seg_hi, float* const* seg_target, float ema_momentum, void* stream);

/* Dynamic loss scaling: AmpOptimWrapper(loss_scale='dynamic') of Pretraining/CM-UNet/configs/cmunet_config.py:76-78, i.e.
 * torch.cuda.amp.GradScaler(init_scale 2^16, growth 2, backoff 0.5, growth_interval 2000), with the state on the device
 * (cmu_amp_state_bytes() = 32 bytes: float scale, float found_inf, int32 growth_tracker, int32 good_steps,
 * int32 skipped_steps, pad): no host synchronisation per step.  Per step: the loss kernel scales its gradient by
 * state.scale; after the gradient exchange cmu_amp_check_finite raises found_inf if any gradient is inf / nan; the
 * optimiser kernel skips or unscales (see cmu_adam_step); cmu_amp_update halves the scale after a skipped step or doubles
 * it after growth_interval clean ones (keeping it when the product is not finite, as torch._amp_update_scale_ does), and
 * clears found_inf.                                                                                               */
int cmu_amp_state_bytes(void);
int cmu_amp_init(void* state, float init_scale, void* stream);
int cmu_amp_check_finite(const float* g, int64_t n, void* state, void* stream);
int cmu_amp_update(void* state, float growth_factor, float backoff_factor, int growth_interval, void* stream);

/* soft-clDice building blocks (Finetuning/metrics.py:401-492): soft skeleton of an fp32 (planes, H, W) stack by num_iter
 * rounds of min/max pooling (the reference uses 10), and the four sums sum(skel_pred*y_true), sum(skel_pred),
 * sum(skel_true*y_pred), sum(skel_true) -> out4 (device), from which clDice = 1 - 2*tprec*tsens/(tprec+tsens).        */
int cmu_softmax2_threshold(const float* logits /*(B,2,H,W)*/, float threshold, float* out /*(B,H,W) 0/1*/, int B, int H, int W, void* stream);
int64_t cmu_soft_skeleton_ws_bytes(int64_t n);
int cmu_soft_skeleton(const float* img, float* skel, int planes, int H, int W, int num_iter, void* ws, void* stream);
int64_t cmu_cldice_sums_ws_bytes(void);
int cmu_cldice_sums(const float* skel_pred, const float* y_true, const float* skel_true, const float* y_pred, int64_t n,
                    float* out4, void* ws, void* stream);

/* The differentiable soft-clDice (threshold=None; csrc/cldice_grad.hip).  Planes are fp32 (B*Kk, H, W): the Kk channels that bit k of
 * keep_mask keeps, in ascending order, image by image.
 *   cmu_softmax_planes      p_planes = softmax(logits, dim=1) of the kept channels (use_threshold: p > threshold as 0/1); t_planes =
 *                           the same channels of the f32 / f64 (B,K,H,W) target (target and t_planes may both be NULL).  2 <= K <= 8.
 *   cmu_softmax_planes_bwd  dlogits_k = p_k (G_k - sum_j p_j G_j) with G = g_planes on the kept channels and 0 elsewhere; p is
 *                           recomputed by the forward's instruction sequence (the same bits).
 *   cmu_soft_skeleton_save  the bits of cmu_soft_skeleton; `kept` (cmu_soft_skeleton_save_ws_bytes) receives the level images
 *                           img_1..img_{num_iter+1}, the running skeletons skel_0..skel_{num_iter-1} ((2 num_iter + 1) n floats) and
 *                           one selection-code byte per pixel for every dilate and every erode window (2 (num_iter + 1) n bytes).
 *   cmu_soft_skeleton_bwd   dimg = d/dimg of <g, soft_skeleton(img)> by one reverse sweep over the levels in gather form (no atomics:
 *                           the same bits on every call), PyTorch autograd's sub-gradients (first maximum / first minimum of a pooling
 *                           window, equal column and row minima share the gradient, relu'(0) = 0).  g = g_skel (may be NULL) plus,
 *                           with the device-resident fp64 g4 = dL/d(the four sums of cmu_cldice_sums), g4[0] y_true + g4[1]; dimg then
 *                           also gains g4[2] skel_true.  ws: cmu_soft_skeleton_bwd_ws_bytes(n).                                    */
int cmu_softmax_planes(const float* logits, const void* target, int target_is_f64, int keep_mask, int use_threshold, float threshold,
                       float* p_planes, float* t_planes, int B, int K, int H, int W, void* stream);
int cmu_softmax_planes_bwd(const float* logits, const float* g_planes, int keep_mask, float* dlogits, int B, int K, int H, int W,
                           void* stream);
int64_t cmu_soft_skeleton_save_ws_bytes(int64_t n, int num_iter);
int cmu_soft_skeleton_save(const float* img, float* skel, int planes, int H, int W, int num_iter, void* kept, void* stream);
int64_t cmu_soft_skeleton_bwd_ws_bytes(int64_t n);
int cmu_soft_skeleton_bwd(const float* img, const void* kept, const float* g_skel, const double* g4, const float* y_true,
                          const float* skel_true, float* dimg, int planes, int H, int W, int num_iter, void* ws, void* stream);

/* Geometry metrics of the finetuning driver (Finetuning/train.py:462-463: hausdorff, radius_arteries; metrics.py:224-395, where
 * scikit-image's find_contours / skeletonize and scipy KD-trees run on the host per image) as exact lattice geometry
 * (csrc/geometry.hip).  Masks are uint8 (B,H,W) 0/1.  The doubled lattice of an H x W mask has (2H-1) x (2W-1) points: pixel
 * centres at (even, even), crossings (midpoints of two 4-neighbour pixels that differ) at (even, odd) / (odd, even).
 *   cmu_argmax2_mask   mask = x[:,1] > x[:,0] for (B,2,H,W) f32 / f64 x (np.argmax: ties to channel 0); clear_border zeroes the
 *                      one-pixel image border (compute_radius_arteries, metrics.py:380-383).
 *   cmu_plane_mask     mask = x[:,channel] > 0 for (B,C,H,W) f32 / f64 x.
 *   cmu_contour_points wmap (B,2H-1,2W-1) uint8: the point multiset of find_contours(mask > 0) (fully_connected='low'):
 *                      1 = a crossing, 2 = the crossing that a closed contour repeats, 0 = none; counts (B,2) int32 =
 *                      (crossings, closed contours).  ws: cmu_contour_points_ws_bytes.
 *   cmu_lattice_nearest for every query point, the exact distance to the nearest point of `seeds` (a wmap; distances are
 *                      sqrt(integer)/2, bit-equal to a KD-tree's); out4 (B,4) fp64 = (sum w*d, sum w, max d, min d) over the
 *                      queries: query_pixels = 0 -> `queries` is a wmap (weights 1 / 2), 1 -> an H x W pixel mask (weight 1 at
 *                      (2r, 2c)).  W <= 512.  ws: cmu_lattice_nearest_ws_bytes.
 *   cmu_skeletonize    scikit-image 2-D skeletonize (Zhang, its own 256-entry table), one workgroup per image; H * ceil(W/32) * 32
 *                      <= 512 * 512.
 *   cmu_hausdorff_finish  per image: 0 if both point sets are empty, inf if one is, else max of the two directed means
 *                      (modified) / maxima (standard) (metrics.py:276-293).  Either output may be NULL.
 *   cmu_radius_finish  per image (2 min, 2 mean, 2 max) of the skeleton-to-contour distances; (0,0,0) without a contour, nan
 *                      when the skeleton is empty but the contour is not (the reference raises there).
 * No host synchronisation; everything is enqueued on `stream`.                                                           */
int cmu_argmax2_mask(const void* x, int is_f64, uint8_t* mask, int B, int H, int W, int clear_border, void* stream);
int cmu_plane_mask(const void* x, int is_f64, int C, int channel, uint8_t* mask, int B, int H, int W, int clear_border, void* stream);
int64_t cmu_contour_points_ws_bytes(int B, int H, int W);
int cmu_contour_points(const uint8_t* mask, uint8_t* wmap, int* counts, int B, int H, int W, void* ws, void* stream);
int64_t cmu_lattice_nearest_ws_bytes(int B, int H, int W);
int cmu_lattice_nearest(const uint8_t* seeds, const uint8_t* queries, int query_pixels, double* out4, int B, int H, int W,
                        void* ws, void* stream);
int cmu_skeletonize(const uint8_t* mask, uint8_t* skel, int B, int H, int W, void* stream);
int cmu_hausdorff_finish(const int* counts_a, const int* counts_b, const double* fwd4, const double* bwd4, double* out_modified,
                         double* out_standard, int B, void* stream);
int cmu_radius_finish(const int* counts, const double* near4, double* out3, int B, void* stream);

/* Fused SGD step over a flat fp32 arena (torch.optim.SGD; MoCo: moco2_module.py:339-344, momentum 0.9, weight decay 1e-4).
 * g' = g*grad_scale + wd*p (where wd_mask != 0 or wd_mask == NULL); buf = g' on step 1, else momentum*buf + (1-dampening)*g';
 * p -= lr * (nesterov ? g' + momentum*buf : buf); momentum == 0: p -= lr*g' (buf may be NULL).                        */
int cmu_sgd_step(float* p, const float* g, float* buf, const uint8_t* wd_mask, int64_t n, float lr, float momentum,
                 float dampening, float weight_decay, int nesterov, int64_t step, float grad_scale, void* stream);
/* cmu_sgd_step under a dynamic loss scaler (amp_state, cmu_amp_*): skipped when the scaler's found_inf is set, gradients unscaled by its
 * scale.  The first update (buf = g') is the first one the scaler lets through -- its good_steps == 0 -- whatever ``step`` says, as
 * torch.optim.SGD never runs behind a skipped step.                                                                              */
int cmu_sgd_step_amp(float* p, const float* g, float* buf, const uint8_t* wd_mask, int64_t n, float lr, float momentum, float dampening,
                     float weight_decay, int nesterov, int64_t step, float grad_scale, const void* amp_state, void* stream);

/* Fused LAMB step (Pretraining/Spark/utils/lamb.py:67-159) over a flat fp32 arena cut into blocks of at most
 * cmu_lamb_block_elems() elements that never straddle a parameter tensor: blk_start / blk_count / blk_tensor [nblocks]
 * (device), t_blk0 [ntensors+1] first block of each tensor, t_wd [ntensors] its weight decay (0 = excluded; such tensors
 * skip the trust ratio unless always_adapt).  u: scratch arena of the parameters' size; ws: cmu_lamb_ws_bytes.
 * Global gradient-norm clip (max_grad_norm <= 0: off), moments, per-tensor trust ratio, update -- no host sync.          */
int cmu_lamb_block_elems(void);
int64_t cmu_lamb_ws_bytes(int nblocks, int ntensors);
int cmu_lamb_step(float* p, const float* g, float* m, float* v, float* u, const int64_t* blk_start, const int* blk_count,
                  const int* blk_tensor, int nblocks, const int* t_blk0, const float* t_wd, int ntensors, float lr, float beta1,
                  float beta2, float eps, int bias_correction, int grad_averaging, float max_grad_norm, int trust_clip,
                  int always_adapt, int64_t step, float grad_scale, void* ws, void* stream);

/* ---- input pipeline on the device (Pretraining/CM-UNet/cmae/datasets/cmunet_dataset.py:60-88) -------------
 * cmu_resize_bicubic: Pillow-convention bicubic resize (mode 'F': Keys a = -0.5, antialiased support, double accumulation,
 * float32 store after each of the two passes, horizontal first) of a per-sample integer crop window to (Ho, Wo), then an
 * optional horizontal flip -- cmunet_dataset.py:74-75 (boxes == NULL: whole image) and RandomResizedCrop + RandomFlip of
 * configs/cmunet_config.py:49-50.  src (B,Hs,Ws) f32; boxes (B,4) int32 device (x0, y0, w, h) or NULL; flip (B) u8 device
 * or NULL; out (B,Ho,Wo) f32; ws: cmu_resize_bicubic_ws_bytes.  Bit-identical to Pillow 12.2 on finite inputs.             */
int64_t cmu_resize_bicubic_ws_bytes(int B, int Hs, int Ws, int Ho, int Wo);
int cmu_resize_bicubic(const float* src, int B, int Hs, int Ws, const int* boxes, const uint8_t* flip, float* out, int Ho, int Wo,
                       void* ws, void* stream);
/* cmu_resize_bicubic_u8: the same call on 8-bit images (PIL mode 'L', what Image.fromarray makes of a uint8 .npy:
 * Finetuning/dataset.py:44-46, Pretraining/Spark/utils/dataset.py:25-27, cmunet_dataset.py:74-75): Pillow's 8-bit resampler -- the
 * double coefficients as 22-bit fixed point (rounded half away from zero), int32 accumulation from 2^21, arithmetic shift, clip to
 * 0..255, a uint8 image between the passes.  src / out uint8, otherwise as cmu_resize_bicubic.  Bit-identical to Pillow 12.2.
 * cmu_resize_nearest_u8: Image.resize(size, NEAREST) of the label masks (Finetuning/dataset.py:47): source index int(x) of Pillow's
 * running double x = scale / 2, += scale per output index.  ws: cmu_resize_nearest_u8_ws_bytes (the two index tables).          */
int64_t cmu_resize_bicubic_u8_ws_bytes(int B, int Hs, int Ws, int Ho, int Wo);
int cmu_resize_bicubic_u8(const uint8_t* src, int B, int Hs, int Ws, const int* boxes, const uint8_t* flip, uint8_t* out, int Ho, int Wo,
                          void* ws, void* stream);
int64_t cmu_resize_nearest_u8_ws_bytes(int Ho, int Wo);
int cmu_resize_nearest_u8(const uint8_t* src, int B, int Hs, int Ws, uint8_t* out, int Ho, int Wo, void* ws, void* stream);
/* cmu_two_view: 'img' = src[b, :out, :out] (ShiftPixel(0), pipelines/processing.py:97-127); 'img_t' = src[b, dy:dy+out,
 * dx:dx+out] + (max of that crop / 10) * z evaluated in float64 and cast to float32 (GaussNoise,
 * pipelines/auto_augment.py:1136-1153).  shifts (B,2) int32 device (dy, dx); z = noise (B,out,out) f64 device, or, when
 * noise == NULL, the in-kernel generator: Philox4x32-10 with counter (element index, 0, 0) and key `seed`, Box-Muller on
 * its first two words (cmu_philox_normal returns the same draws).                                                        */
int cmu_two_view(const float* src, int B, int S, const int* shifts, const double* noise, uint64_t seed, float* img, float* img_t,
                 int out, void* stream);
int cmu_philox_normal(double* out, int64_t n, uint64_t offset, uint64_t seed, void* stream);
/* Random patch mask of backbones/UNet_encoder.py:106-139 on the device: mask (B,H,W) u8, 1 = masked; per sample a uniformly
 * random n_mask-subset of the (H/patch)*(W/patch) patches (<= 4096): patch p of sample b draws the first word of
 * Philox4x32-10(counter = offset + b*P + p, key = seed) and is masked iff (key, p) is among the n_mask smallest.            */
int cmu_random_patch_mask(uint8_t* mask, int B, int H, int W, int patch, int n_mask, uint64_t seed, uint64_t offset, void* stream);

/* ---- skinny (weight-streaming) GEMMs of the projector / predictor necks (nonlinear_neck.py:63-66, 95-101 with
 * cmunet_config.py:18-38: Linear(H*W -> 1536)) -- nn.Linear and its autograd, fp32, M <= 256 rows per GPU (the reference's batch
 * size, cmunet_config.py:55; moco2_module.py:91,262 for the queue logits), taken in groups of 32 rows (one 32-row MFMA tile):
 *   fwd    y (M,N) = x (M,K) . w (N,K)^T + bias (or NULL)      K % 8 == 0; ws: cmu_skinny_gemm_ws_bytes (split-K slab)
 *   dgrad  dx (M,K) = dy (M,N) . w (N,K)                        K % 4 == 0; ws: cmu_skinny_gemm_bwd_ws_bytes (dy transposed)
 *   wgrad  dw (N,K) = dy^T . x, dbias (N) = sum_m dy (or NULL)  K % 4 == 0
 * x, w, dx, dw 16-byte aligned, rows contiguous.  fwd / dgrad: one pass over the weights per group of 32 rows; wgrad: one
 * launch contracting over all rows; v_mfma_f32_32x32x2_f32.  M > 256 is an argument error (there is no library GEMM behind
 * these entries: the host side raises).                                                                                   */
int64_t cmu_skinny_gemm_ws_bytes(int M, int N, int64_t K);
int cmu_skinny_gemm_fwd(const float* x, const float* w, const float* bias, float* y, int M, int N, int64_t K, void* ws, void* stream);
int64_t cmu_skinny_gemm_bwd_ws_bytes(int M, int N);
int cmu_skinny_gemm_dgrad(const float* dy, const float* w, float* dx, int M, int N, int64_t K, void* ws, void* stream);
int cmu_skinny_gemm_wgrad(const float* dy, const float* x, float* dw, float* dbias, int M, int N, int64_t K, void* stream);

/* 16-bit-operand variants for the AMP configuration (cmunet_config.py:76-78: nn.Linear under autocast multiplies fp16
 * operands into fp32): x, w, dy, dx, dw stay fp32 in memory (the master weights of the optimiser), operands are rounded to
 * dt (CMU_F16 / CMU_BF16) in registers, accumulation fp32 -- v_mfma_f32_32x32x16.  Same contracts as above; fwd needs
 * K % 16 == 0; dgrad reads dy in place (no workspace).                                                                  */
int64_t cmu_skinny16_gemm_ws_bytes(int M, int N, int64_t K);
int cmu_skinny16_gemm_fwd(const float* x, const float* w, const float* bias, float* y, int M, int N, int64_t K, int dt, void* ws,
                          void* stream);
int cmu_skinny16_gemm_dgrad(const float* dy, const float* w, float* dx, int M, int N, int64_t K, int dt, void* stream);
int cmu_skinny16_gemm_wgrad(const float* dy, const float* x, float* dw, float* dbias, int M, int N, int64_t K, int dt, void* stream);

/* ---- BatchNorm1d (+ ReLU) of the necks' hidden layer (nonlinear_neck.py:58-60, 95-98: (Sync)BN eps 1e-6 then ReLU), rows M x
 * columns N fp32.  Statistics per column over the rows; on more than one rank the caller exchanges the column sums
 * (SyncBN):
 *   cmu_bn1d_colsums      sums[2][N] = (sum x, sum x^2)                       -> all-reduce -> cmu_bn1d_relu_fwd(sums, count)
 *   cmu_bn1d_relu_fwd     y = [relu](gamma * (x - mean) * invstd + beta); sums == NULL: statistics of the M rows (two-pass
 *                         variance, as F.batch_norm), else mean = sums[0]/count, var = sums[1]/count - mean^2; training:
 *                         running statistics updated (unbiased variance, momentum); training == 0: running statistics used.
 *                         save_mean / save_invstd (nullable) are written in both modes (eval: running_mean and
 *                         1/sqrt(running_var + eps): what cmu_bn1d_relu_bwd needs for the fixed affine map, with zero sums).
 *                         gamma / beta nullable (affine=False).
 *   cmu_bn1d_bwd_colsums  sums[2][N] = (sum dz, sum dz * xhat), dz = dy * [y > 0] when relu   -> all-reduce
 *   cmu_bn1d_relu_bwd     dx = gamma * invstd * (dz - S0/count - xhat * S1/count) with (S0, S1) = sums or, if NULL, the local
 *                         sums (count = M); dgamma / dbeta (nullable) = LOCAL sums (the gradient exchange averages them).   */
int cmu_bn1d_colsums(const float* x, float* sums, int M, int N, void* stream);
int cmu_bn1d_relu_fwd(const float* x, const float* sums, int64_t count, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, float momentum, float eps, int training, int relu, float* y, float* save_mean,
                      float* save_invstd, int M, int N, void* stream);
int cmu_bn1d_bwd_colsums(const float* dy, const float* x, const float* y, const float* save_mean, const float* save_invstd, int relu,
                         float* sums, int M, int N, void* stream);
int cmu_bn1d_relu_bwd(const float* dy, const float* x, const float* y, const float* save_mean, const float* save_invstd,
                      const float* gamma, int relu, const float* sums, int64_t count, float* dx, float* dgamma, float* dbeta, int M,
                      int N, void* stream);

/* Conv2d(K, N, 1) from an NHWC dt tensor with its pending transform to an NCHW fp32 tensor: the per-call `reduce_channels`
 * of the target latent (Pretraining/CM-UNet/cmae/models/algorithms/cmunet.py:128-131; the reference then re-views the NCHW
 * memory as a (B,1,H,W) image).  w (N,K) fp32 (rounded to dt in registers), bias (N) or NULL.  K a whole number of 32-byte
 * slices, H*W % 4 == 0.                                                                                                   */
int cmu_conv1x1_nchw_fwd(const void* x, int64_t ldx, const float* in_scale, const float* in_shift, int relu_from, const float* w,
                         const float* bias, float* out, int B, int H, int W, int K, int N, int dt, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Models Genesis / MAE baseline pretraining inputs (csrc/genesis.hip; Pretraining/Transformation_based/utils.py:69-253)
 * ------------------------------------------------------------------------------------------- */
/* One 112-byte record per image (layout: genesis.hip GenesisRec, mirrored by cmunet_amd/genesis.py REC_DTYPE) is the contract
 * between the randomness (this device sampler, or the host replay of the reference's own random / numpy streams) and the apply
 * kernels.  blocks: int16 (x0, y0, bx, by) x 10,000 per image; perms: uint8, (H/25)*(W/25) bytes per block.                  */
int cmu_genesis_rec_bytes(void);
/* row segments of the gather pass's LDS owner map (= min / max partials per image)                                          */
int cmu_genesis_segments(int H, int W);
/* Philox4x32-10 keyed by (seed, offset): batch selection (B distinct of N, uniform order) and, unless mae, the Genesis record
 * with the reference's laws (3-flip loop, local / non-linear / paint branches, truncated-geometric rectangle counts, uniform
 * Fisher-Yates per block).  42 <= H, W and (H/25)*(W/25) <= 256 for Genesis; B <= min(N, 1024).                              */
int cmu_genesis_sample(void* recs, int16_t* blocks, uint8_t* perms, int N, int B, int H, int W, int mae, double flip_rate,
                       double local_rate, double nonlinear_rate, double paint_rate, double inpaint_rate, uint64_t seed,
                       uint64_t offset, void* stream);
/* y = flip(src[rec.src]) (src (N,H,W) f32); x = local pixel shuffle of y (last covering block wins); minmax (B, segments, 2) f32 */
int cmu_genesis_gather_shuffle(const float* src, const void* recs, const int16_t* blocks, const uint8_t* perms, float* x, float* y,
                               float* minmax, int B, int H, int W, void* stream);
/* both sampled cubics of nonlinear_transformation (fp64, 100,000 points) and their sorted copies in ws, for any number of monotone
 * runs (up to 16: merged by rank; more -- a near-constant image, whose samples are rounding noise -- a general sort in place).  A rank
 * outside the table sets bit 1 of *err (device word, read at the next synchronisation); bit 0 is no longer raised.               */
int64_t cmu_genesis_bezier_ws_bytes(int B);
int cmu_genesis_bezier(const void* recs, const float* minmax, int B, int H, int W, void* ws, int* err, void* stream);
/* x <- np.interp(x, xs, ys) (fp64) where the record asks for it, then in- / out-painting; noise (B,H,W) f32 or NULL (Philox).  */
int cmu_genesis_intensity_paint(const void* recs, const void* ws, const float* noise, uint64_t seed, uint64_t offset, float* x, int B,
                                int H, int W, void* stream);
/* generate_pair_mae: y = src[rec.src], x = y * (1 - mask) with mask (H,W) uint8 shared by the batch                           */
int cmu_genesis_mae(const float* src, const void* recs, const uint8_t* mask, float* x, float* y, int B, int H, int W, void* stream);
/* ---------------------------------------------------------------------------------------------
 * Finetuning training augmentation (csrc/ft_augment.hip; Finetuning/dataset.py:134-165 get_training_augmentation, then the
 * SegmentationDataset resize + one-hot of dataset.py:44-55).  DESIGN.md 4.13 restates the rules.
 * ------------------------------------------------------------------------------------------- */
/* One record per image holds every random decision of its augmentation (mirrored by cmunet_amd/ft_augment.py REC_DTYPE; the
 * layout query below lets the host check it).  ops: bit 0 GaussNoise, 1 GaussianBlur, 2 RandomBrightnessContrast, 3 Downscale,
 * 4 OneOf; oneof: 0 HorizontalFlip, 1 VerticalFlip, 2 RandomRotate90 (np.rot90 by rot_k), 3 GaussNoise.                         */
typedef struct CmuFtAugRec {
    int32_t ops;
    int32_t y0, x0;         /* RandomCrop offset (row, column)                                                              */
    int32_t ksize;          /* GaussianBlur kernel size (odd)                                                               */
    double var_noise;       /* GaussNoise variance                                                                          */
    double var_oneof;       /* OneOf's GaussNoise variance                                                                  */
    double sigma;           /* GaussianBlur sigma                                                                           */
    double alpha, beta;     /* RandomBrightnessContrast: out = img * alpha + beta                                           */
    double scale;           /* Downscale factor                                                                             */
    int32_t oneof, rot_k;
} CmuFtAugRec;              /* 72 bytes */
/* out[0] = sizeof(CmuFtAugRec), out[1..12] = the fields' offsets in declaration order; returns the count (13)                */
int cmu_ftaug_rec_layout(int64_t* out, int n);
/* the largest GaussianBlur kernel size the photometric pass takes (its LDS halo is sized for it)                              */
int cmu_ftaug_max_ksize(void);
/* B records, Philox4x32-10 keyed by (seed, offset).  params (host, nparams = 19): p_noise, var lo, hi; p_blur, ksize lo, hi,
 * sigma lo, hi; p_brightness_contrast, brightness lo, hi, contrast lo, hi; p_downscale, scale lo, hi; p_oneof, var lo, hi.
 * crop <= H, W.  Every parameter is drawn whether or not its transform fires.                                                 */
int cmu_ftaug_sample(void* recs, int B, int H, int W, int crop, const double* params, int nparams, uint64_t seed, uint64_t offset,
                     void* stream);
/* P (B,S,S) f32 = brightness / contrast (float32, [0,1] clip if clip) of the separable Gaussian blur (float64 taps, reflect-101)
 * of GaussNoise (float64, clip if clip) of the S x S crop of src (B,H,W) f32.  noise: (2,B,S,S) float64 standard normals (plane 0
 * is read here) or NULL for Philox keyed by (seed, offset, image, pixel).                                                      */
int cmu_ftaug_photometric(const float* src, int B, int H, int W, const void* recs, const double* noise, uint64_t seed, uint64_t offset,
                          int clip, float* out, int S, void* stream);
/* the augmented image and mask before the resize: img_out = OneOf(Downscale(P)) (plane 1 of noise for OneOf's GaussNoise),
 * mask_out = OneOf's geometry of the crop of masks (B,H,W) uint8; both (B,S,S)                                                  */
int cmu_ftaug_apply(const float* aug, const uint8_t* masks, int B, int H, int W, const void* recs, const double* noise, uint64_t seed,
                    uint64_t offset, int clip, float* img_out, uint8_t* mask_out, int S, void* stream);
/* the same, composed into the Pillow bicubic resize to size x size (img_out (B,size,size) f32, bit-equal to cmu_resize_bicubic of
 * the materialised image) and the NEAREST resize + one-hot of the mask (onehot (B,ncls,size,size) float64, class_values a host
 * array of ncls <= 16 values).  ws: cmu_ftaug_resize_ws_bytes(B, S, size).                                                      */
int64_t cmu_ftaug_resize_ws_bytes(int B, int S, int size);
int cmu_ftaug_resize_onehot(const float* aug, const uint8_t* masks, int B, int H, int W, const void* recs, const double* noise,
                            uint64_t seed, uint64_t offset, int clip, const int* class_values, int ncls, float* img_out, double* onehot,
                            int S, int size, void* ws, void* stream);
/* ---------------------------------------------------------------------------------------------
 * MoCo-v2's two augmented views (csrc/moco_views.hip; Pretraining/MoCo/.../moco_data_module.py:119-132 tau_g, torchvision 0.14.0's
 * tensor path).  DESIGN.md 4.14 restates the rules.
 * ------------------------------------------------------------------------------------------- */
/* One record per (image, view) holds every random decision (mirrored by cmunet_amd/moco_views.py REC_DTYPE; records are laid out
 * (B, 2)).  ops: bit 0 RandomRotation, 1 GaussianBlur, 2 horizontal flip, 3 vertical flip, 4 GaussNoise.                          */
typedef struct CmuMocoViewRec {
    int32_t ops;
    int32_t top, left, height, width;   /* RandomResizedCrop's box (i, j, h, w)                                                 */
    int32_t pad;
    double angle;                       /* RandomRotation angle in degrees                                                      */
    double sigma;                       /* GaussianBlur sigma (both axes)                                                       */
} CmuMocoViewRec;                       /* 40 bytes */
/* out[0] = sizeof(CmuMocoViewRec), out[1..7] = the offsets of ops, top, left, height, width, angle, sigma; returns the count (8) */
int cmu_mocoviews_rec_layout(int64_t* out, int n);
/* the largest GaussianBlur kernel size (either axis) the geometry pass takes (its LDS halo is sized for it)                       */
int cmu_mocoviews_max_ksize(void);
/* 2 * B records, Philox4x32-10 keyed by (seed, offset).  params (host, nparams = 12): p_rotation, degrees; scale lo, hi, ratio lo,
 * hi; p_blur, sigma lo, hi; p_hflip; p_vflip; p_noise.  The crop's rejection loop (10 attempts, then the centred box) runs in the
 * kernel.  Every parameter is drawn whether or not its transform fires.                                                           */
int cmu_mocoviews_sample(void* recs, int B, int H, int W, const double* params, int nparams, uint64_t seed, uint64_t offset,
                         void* stream);
/* out (2,B,O,O) f32 = flips(blur(resize(crop(rotate(src (B,H,W) f32))))) of view v of image b at out[v][b]: rotation NEAREST about
 * the centre with zero fill, bilinear resize (antialias: ATen's triangle filter), kx x ky Gaussian blur with reflect padding.
 * vmax: 2 * B words, zeroed here and then merged with every view's maximum (order-preserving bits; cmu_mocoviews_max decodes).   */
int cmu_mocoviews_geometry(const float* src, int B, int H, int W, const void* recs, int kx, int ky, int antialias, float* out, int O,
                           void* vmax, void* stream);
/* out (B,2) f32 = the maxima that cmu_mocoviews_geometry left in vmax                                                            */
int cmu_mocoviews_max(const void* vmax, float* out, int B, void* stream);
/* GaussNoise on the views whose record asks for it: out += (max / 10) * z, float32; noise (2,B,O,O) f32 standard normals or NULL for
 * Philox keyed by (seed, offset, view, pixel).  Reads the maxima from vmax: no host round trip.                                   */
int cmu_mocoviews_noise(float* out, int B, int O, const void* recs, const void* vmax, const float* noise, uint64_t seed,
                        uint64_t offset, void* stream);
/* nn.MSELoss()(logits[:,0], y) over B*H*W into loss (1 fp32); dlogits (nullable) = d loss * loss_scale [* amp scale] / d logits
 * (zero on channels > 0).  Fixed-order reduction: same inputs, same bits.  ws: cmu_mse_ws_bytes().                           */
int64_t cmu_mse_ws_bytes(void);
int cmu_mse_fwd_bwd(const float* logits, int K, const float* y, float* loss, float* dlogits, float loss_scale, const void* amp_state,
                    int B, int H, int W, void* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Connected components of uint8 label maps and the clean-up of predicted masks (csrc/components.hip; no
 * reference counterpart: users of the reference call scipy.ndimage on the host).  Shapes: 1 <= B <= 65535, 1 <= H, W,
 * H * W < 2^31; B * H * W is indexed in 64 bits.  Every result is an integer: the same bits on every call.
 *
 * cmu_label_components: foreground = (src == cls) for cls in 0..255, (src != 0) for cls == -1, (src != c) for cls == -2 - c (the
 * complement of class c, c in 0..255: what hole filling labels).  connectivity 4 or 8.  labels (B,H,W) int32: 0 on background,
 * else 1 + the smallest row-major index y * W + x of the pixel's component within its image.  counts (B) int32: components per
 * image, or -1 if a find / union walk of that image overran its trip bound of H * W (a defect, never expected).  Block-based
 * union-find on 32 x 32 tiles; a fixed number of launches, no host synchronisation.  ws: cmu_label_components_ws_bytes.          */
int64_t cmu_label_components_ws_bytes(int B, int H, int W);
int cmu_label_components(const uint8_t* src, int cls, int connectivity, int32_t* labels, int32_t* counts, int B, int H, int W, void* ws,
                         void* stream);
/* sizes (B,H,W) int32: sizes[b, r] = pixels of the component labelled r + 1, 0 elsewhere (one atomic add per distinct label
 * of a wave's 64 consecutive pixels; integer adds: exact in any order).                                                            */
int cmu_component_sizes(const int32_t* labels, int32_t* sizes, int B, int H, int W, void* stream);
/* keep_roots (B,n) int32, 1 <= n <= 8: the labels of the n largest components of each image, largest first, ties to the smaller
 * label; unused slots -1.                                                                                                         */
int cmu_select_largest(const int32_t* sizes, int n, int32_t* keep_roots, int B, int H, int W, void* stream);
/* touches (B,H,W) uint8: touches[b, r] = 1 iff the component labelled r + 1 holds a pixel of the image's outer frame, else 0.   */
int cmu_border_components(const int32_t* labels, uint8_t* touches, int B, int H, int W, void* stream);
/* One streaming pass src (B,H,W) uint8 -> out (B,H,W) uint8 (another buffer).  With labels / sizes (both or neither; the labelling
 * of class cls): a labelled pixel whose component has fewer than min_size pixels, or -- keep_roots (B,n_keep) given -- whose label
 * is not listed for its image, receives removed_value.  With hole_labels / hole_touches (both or neither; the 4-connected labelling
 * of cls = -2 - class and its cmu_border_components flags): a pixel of a component that does not touch the frame receives cls.
 * class_values (n_values bytes, or NULL): out = class_values[v] for v < n_values.                                                  */
int cmu_filter_components(const uint8_t* src, int cls, const int32_t* labels, const int32_t* sizes, int min_size, const int32_t* keep_roots,
                          int n_keep, int removed_value, const int32_t* hole_labels, const uint8_t* hole_touches,
                          const uint8_t* class_values, int n_values, uint8_t* out, int B, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Exact Euclidean distance transform of uint8 maps, disk morphology and surface distances (csrc/edt.hip, csrc/edt_scan.h, DESIGN.md
 * section 4.23; no reference counterpart: users of the reference call scipy.ndimage on the host).  Shapes: 1 <= B <= 65535,
 * 1 <= H, W <= 4096 (2 * 4095^2 < 2^31); anything else is CMU_ERR_ARG.  Images of a batch are independent.  Every result but the fp64
 * sum is an integer; no atomics; the same bits on every call.  There is no workspace query: scratch is the explicit tensors named
 * below, every element of every output is written on every call and nothing is read before it is written.
 * Site rule: the codes of cmu_label_components (cls in 0..255: src == cls; -1: src != 0; -2 - c: src != c).
 *
 * The transform is two launches.  cmu_edt_columns: g (B,H,W) int32 = vertical distance to the nearest site of the pixel's own
 * column, 16384 where the column holds none.  border != 0: the sites are the rule's BORDER pixels instead: pixels of the rule's set with
 * a 4-neighbour outside the set or outside the image (mask & ~binary_erosion(mask, cross, border_value=0)).
 * cmu_edt_rows: from g, any of (NULL = not wanted, at least one)
 *   dist2 (B,H,W) int32    the squared Euclidean distance to the nearest site of the pixel's image; 0 on a site; -1 at EVERY pixel of an
 *                          image that holds no site at all (this library's rule: scipy's answer there is meaningless);
 *   dist  (B,H,W) float32  float32(sqrt(float64(dist2))), inf where dist2 == -1;
 *   out8  (B,H,W) uint8    with base (B,H,W) uint8: a site keeps base; any other pixel is a hit if dist2 <= t (greater == 0: it lies in
 *                          the dilation of the sites by the disk dy^2 + dx^2 <= t) or if dist2 > t (greater != 0: it survives the erosion
 *                          by that disk, the sites being the set's complement), -1 counting as infinitely far; a hit writes v_hit, a
 *                          miss v_miss, and a value of -1 means "keep base".  out8 may be base itself.                                    */
int cmu_edt_columns(const uint8_t* src, int cls, int border, int32_t* g, int B, int H, int W, void* stream);
int cmu_edt_rows(const int32_t* g, int32_t* dist2, float* dist, const uint8_t* base, uint8_t* out8, int greater, int t, int v_hit,
                 int v_miss, int B, int H, int W, void* stream);
/* border (B,H,W) uint8: 1 on the border pixels of the rule's set (as above), else 0.                                                     */
int cmu_surface_border(const uint8_t* src, int cls, uint8_t* border, int B, int H, int W, void* stream);
/* Over the border pixels of src's set, with dist2 the transform to ANOTHER set's border: sums (B,2) fp64 = (sum of sqrt(dist2), added
 * in a fixed order; sqrt(max dist2), 0 when n == 0); counts (B,3) int32 = (n border pixels, max dist2, number with dist2 <= tol2).
 * max is -1 when n == 0 and 2^31 - 1 when dist2 is -1 (the other border is empty: both sums are then inf).  masked (B,H,W) int32, or
 * NULL: dist2 on the border pixels, -2 elsewhere.  One workgroup per image.                                                             */
int cmu_surface_reduce(const uint8_t* src, int cls, const int32_t* dist2, int tol2, int32_t* masked, double* sums, int32_t* counts, int B,
                       int H, int W, void* stream);
/* Exact order statistics: values (B,n_ranks) int32 = the ranks[b][r]-th smallest (from 0) of the non-negative entries of masked_a and
 * masked_b of image b together, -1 if there are not that many (or the rank is negative); roots (B,n_ranks) fp64 = sqrt(value), inf
 * for -1.  n_ranks is 1 or 2; ranks (B,n_ranks) int32 lives on the device.  Bisection on the value, one counting pass per step, at
 * most 33 passes per rank; one workgroup per image.                                                                                     */
int cmu_surface_select(const int32_t* masked_a, const int32_t* masked_b, const int32_t* ranks, int n_ranks, int32_t* values, double* roots,
                       int B, int H, int W, void* stream);

/* ---- image preprocessing (csrc/preprocess.hip): the reference's data_processing/pre_processing.py -------------
 * Planes are contiguous (B,H,W), 1 <= B <= 65535, H, W >= 1, H * W < 2^31; x is uint8 (is_u8 = 1) or float32 (is_u8 = 0).  Every kernel is
 * deterministic (fixed summation order, no float atomics).  `stats` is (B,4) float64 per image: mean, population standard deviation
 * (numpy's np.std: sqrt(sum((x - mean)^2) / N)), min, max.
 * cmu_pre_stats: one workgroup per image, sums in float64; a uint8 image's sum is an exact integer, so its mean is one division.          */
int cmu_pre_stats(const void* x, int is_u8, double* stats, int B, int H, int W, void* stream);
/* out = float32((double(x) - stats[b][0]) / stats[b][1]); a zero deviation gives nan / inf as the division does.                         */
int cmu_pre_standardize(const void* x, int is_u8, const double* stats, float* out, int B, int H, int W, void* stream);
/* out = (x - lo) / float32(hi - lo) with lo = stats[b][2], hi = stats[b][3]: uint8 differences are exact integers, float32 ones a single
 * float32 subtraction; the quotient is one correctly rounded float32 division (hi == lo: nan where x == lo).                             */
int cmu_pre_minmax(const void* x, int is_u8, const double* stats, float* out, int B, int H, int W, void* stream);
/* every row divided by its Euclidean norm (float64 norm and quotient, then one cast); a zero row stays zero.                            */
int cmu_pre_row_normalize(const void* x, int is_u8, float* out, int B, int H, int W, void* stream);
/* The largest Gaussian radius (sigma) of the unsharp mask; the half-width of its kernel is lw = int(4 * radius + 0.5) <= 64.            */
#define CMU_PRE_MAX_RADIUS 16
#define CMU_PRE_MAX_LW 64
/* Unsharp mask in two passes.  f = float32(x) / scale_div (255 for skimage's uint8 -> [0,1] conversion, else 1).  weights: lw + 1 float32
 * on the device, w[k] the normalised Gaussian tap at distance k.  Borders are scipy's 'reflect' (d c b a | a b c d), repeated as needed.
 * cmu_pre_blur_rows: tmp = f blurred along W.  cmu_pre_unsharp_cols: blurred = tmp blurred along H, out = f + (f - blurred) * amount,
 * then with clip != 0 clipped to [0,1] -- or to [-1,1] for an image whose stats[b][2] (min) is negative (stats may be NULL: [0,1]).       */
int cmu_pre_blur_rows(const void* x, int is_u8, float scale_div, const float* weights, int lw, float* tmp, int B, int H, int W, void* stream);
int cmu_pre_unsharp_cols(const void* x, int is_u8, float scale_div, const float* tmp, const float* weights, int lw, float amount, int clip,
                         const double* stats, float* out, int B, int H, int W, void* stream);
/* dst (B,OH,OW) = src[:, y0:y0+OH, x0:x0+OW] for elements of elem_bytes = 1 or 4.                                                        */
int cmu_pre_crop(const void* src, int elem_bytes, void* dst, int B, int H, int W, int y0, int x0, int OH, int OW, void* stream);
/* out (B,HW) uint8 = 1 where any of the M masks (B,M,HW) uint8 is non-zero at the pixel, else 0.                                         */
int cmu_pre_integrate_masks(const uint8_t* masks, uint8_t* out, int B, int M, int64_t HW, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Choosing the operating point: probability histograms, threshold sweeps, ROC / PR and calibration (csrc/prob_hist.hip,
 * csrc/hist_curves.h; no reference counterpart: the reference fixes the threshold at 0.5).  Integers only up to
 * the scores: no floating-point atomics, the same bits on every call.  No workspace.
 *
 * cmu_prob_hist: ONE pass over src (B,K,H,W) fp32, 1 <= K <= CMU_HIST_MAX_K planes, and a target gives, per row (image or pool, plane)
 *   counts  (Bout,K,2,NB+1) int64    pixels of the row by ground truth (0, 1) and bin;
 *   conf    (Bout,K,NB+1)   uint64   the sum over the bin of floor(p * 2^32) (fixed point: order-free; feeds the calibration error);
 *   invalid (Bout,K)        int32    elements whose probability was NaN or outside [0, 1] (clamped as below).
 * from_logits = 1: src holds logits; p is the fp32 softmax over the K planes that cmu_seg_stats_fwd thresholds (the same bits), or for
 * K = 1 the sigmoid of cmu_head_predict.  from_logits = 0: src holds probabilities, one plane per row.
 * target_kind 0 / 1: fp32 / fp64 planes of src's shape, positive iff y > 0.5.  target_kind 2: a (B,H,W) uint8 label map; a pixel of
 * label c is positive for plane c only (a label >= K for none); with K = 1 the one plane is "foreground": label != 0.
 * NB: a power of two in 2..CMU_HIST_MAX_BINS.  bin = ceil(p * NB) in fp32 (the product is exact): bin b holds (b-1)/NB < p <= b/NB, bin
 * 0 holds p == 0, so "p > j/NB" is exactly "bin > j".  NaN and p < 0 count as 0 (-0.0 is 0), p > 1 and +inf as 1, each also in invalid.
 * pooled = 1: Bout = 1, every image adds into the same rows; else Bout = B <= 65535.  accumulate = 0: the entry zeroes the three outputs
 * on the stream first; accumulate = 1: it adds to what they hold (a validation set pools without a host sync).
 * 16-byte src loads (8-byte for K > 4) when H*W % 4 == 0 (% 2) and src and target are aligned (16 bytes; a label map: 4 / 2), one pixel
 * per lane otherwise -- decided for the whole tensor.  At most 2^32 pixels per workgroup (256 workgroups): CMU_ERR_ARG past that.       */
#define CMU_HIST_MAX_K 8
#define CMU_HIST_MAX_BINS 1024
int cmu_prob_hist(const float* src, int from_logits, const void* target, int target_kind, int64_t* counts, uint64_t* conf, int32_t* invalid,
                  int B, int K, int H, int W, int NB, int pooled, int accumulate, void* stream);
/* From rows histogram rows (counts (rows,2,NB+1), conf (rows,NB+1) or NULL), one workgroup per row:
 *   cum     (rows,4,NB+1) int64   tp, fp, fn, tn at threshold j/NB, j = 0..NB (tp[j] = positives in bins > j): the integers
 *                                 cmu_seg_stats_fwd counts at that threshold;
 *   scores  (rows,5,NB+1) fp64    F-beta ((1+b^2) tp + eps) / ((1+b^2) tp + b^2 fn + fp + eps), IoU (tp + eps) / (tp + fp + fn + eps),
 *                                 precision (tp + eps) / (tp + fp + eps), recall (tp + eps) / (tp + fn + eps), specificity
 *                                 (tn + eps) / (tn + fp + eps): Finetuning/metrics.py:135-198, each the Python expression's bits;
 *   summary (rows,6)      fp64    [0] AUROC = sum_b neg_b (pos_{>b} + pos_b / 2) / (P N) (the trapezoid rule over the NB + 2 points; NaN
 *                                 when P or N is 0); [1] average precision = sum (R_i - R_{i+1}) Prec_i over descending thresholds with
 *                                 the all-positive point, without eps (NaN when P is 0); [2] ECE = sum_b |pos_b - conf_b / 2^32| / (P + N);
 *                                 [3] MCE, the largest per-bin gap |pos_b - conf_b / 2^32| / (pos_b + neg_b); (both NaN without conf);
 *                                 [4] best_j, the first argmax over j = 1..NB-1 of the score select names (0 F-beta, 1 IoU, 2 Youden's
 *                                 J = recall + specificity - 1 without eps); [5] that score.                                          */
int cmu_hist_curves(const int64_t* counts, const uint64_t* conf, int rows, int NB, double eps, double beta, int select, int64_t* cum,
                    double* scores, double* summary, void* stream);
/* out[i] = prob[i] > threshold ? v_pos : v_neg for n float32 probabilities (NaN: v_neg); v_pos, v_neg in 0..255.  16 elements per lane
 * when n % 16 == 0 and both pointers are 16-byte aligned, else one.                                                                  */
int cmu_threshold_mask(const float* prob, float threshold, int v_pos, int v_neg, uint8_t* out, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Losses for thin, rare foregrounds: focal cross entropy, map-weighted softmax sums (boundary and Hausdorff-DT losses) and the distance
 * fields they take (csrc/map_loss.hip, csrc/map_loss_math.h; no reference counterpart).  x / logits (B,K,H,W)
 * fp32, 2 <= K <= 8.  The conventions of cmu_seg_stats_fwd / cmu_index_ce_fwd: p is the fp32 softmax those entries use (the same bits);
 * a lane takes 4 pixels (2 for K > 4) of every plane when H*W is a multiple of that and every tensor pointer of the call is 16-byte
 * aligned, else 1 -- for the whole tensor; per-lane fp64 sums -> block partials -> a fixed-order finalisation; no floating-point
 * atomics, the same bits on every call; upstream gradients g are read from device memory and NULL stands for zeros; no host sync.
 * There is no workspace query: `partials` is a caller's fp64 tensor of columns x 1024 doubles (the grid is capped at 1,024 blocks;
 * columns = 3 for cmu_focal_fwd, K for cmu_softmax_map_fwd).  It needs no initialisation: every element that is read was written by
 * the same call.  Every element of every output is written on every call.
 *
 * cmu_focal_fwd: target_kind is a CMU_ICE_* code, the target as cmu_index_ce_fwd takes it (the arg-max of one-hot planes runs over all
 * K channels).  class_w: K fp32 alpha_c or NULL (ones); gamma >= 0.  With t the pixel's label and q = 1 - p_t, formed as the sum of the
 * OTHER classes' exponentials over the total (never 1 - p_t):
 *   table[0] = sum alpha_t q^gamma (-log p_t)   -log p_t in the form of cmu_index_ce_fwd (with gamma = 0: its table[0], the same bits)
 *   table[1] = sum alpha_t                      over the same pixels
 *   table[2] = the number of pixels whose label is not ignore_index
 * q^gamma is exactly 1 for gamma = 0 (also at q = 0), a multiplication for gamma = 1 and 2, else one fp32 exp(gamma log q), 0 at q = 0.
 * A label outside [0, K) that is not ignore_index is never used as an index: it adds NaN to table[0] and gets a zero gradient.
 * cmu_focal_bwd: g = 1 double (d / d table[0]);  dx_j = g alpha_t (d_jt - p_j) (gamma p_t q^(gamma-1) log p_t - q^gamma), zero at
 * ignored pixels, evaluated without inf * 0 at q = 0 and without cancellation (both addends of an element have one sign).             */
int cmu_focal_fwd(const float* x, const void* target, int target_kind, const float* class_w, double gamma, int64_t ignore_index,
                  double* table, double* partials, int B, int K, int H, int W, void* stream);
int cmu_focal_bwd(const float* x, const void* target, int target_kind, const float* class_w, double gamma, int64_t ignore_index,
                  const double* g, float* dx, int B, int K, int H, int W, void* stream);
/* cmu_softmax_map_fwd: table[K] doubles over the classes of keep_mask (bit c = class c; the wmap / y planes of the others are not read
 * and their entries are 0).  wmap (B,K,H,W) fp32 or NULL (ones); y (B,K,H,W) fp32 / fp64 (y_is_f64), unused and nullable for kind 0.
 *   kind 0 (linear)    table[c] = sum wmap_c p_c
 *   kind 1 (squared)   table[c] = sum wmap_c (p_c - y_c)^2      the difference and the square in fp64; the difference is formed as
 *                      ((1 - y_c) e_c - y_c sum_{j != c} e_j) / sum_j e_j from the exponentials behind p, so that against a one-hot y a
 *                      confident pixel keeps its bits (p_c - 1 from the fp32 p would not)
 * cmu_softmax_map_bwd: g = K doubles; dlogits_j = p_j (G_j - sum_c p_c G_c) with G_c = g_c wmap_c (kind 0) or 2 g_c wmap_c (p_c - y_c)
 * (kind 1), G_c = 0 outside keep_mask; combined in fp64 as cmu_seg_stats_bwd does.  All K planes of dlogits are written.              */
int cmu_softmax_map_fwd(const float* logits, const float* wmap, const void* y, int y_is_f64, int keep_mask, int kind, double* table,
                        double* partials, int B, int K, int H, int W, void* stream);
int cmu_softmax_map_bwd(const float* logits, const float* wmap, const void* y, int y_is_f64, int keep_mask, int kind, const double* g,
                        float* dlogits, int B, int K, int H, int W, void* stream);
/* cmu_distance_field: one fp32 plane of a (B,K,H,W) map, written at field + b K H W + plane H W, from the (B,H,W) int32 dist2 maps of
 * cmu_edt_rows for a set S: d2_to = the transform to S (0 on S), d2_from = the transform to S's complement.  K >= 1.
 *   mode 0 (signed; Kervadec's one_hot2dist)   outside S: sqrt(d2_to); inside S: 1 - sqrt(d2_from); in fp64, rounded once.  alpha and
 *                                              the second pair are unused (NULL).
 *   mode 1 (unsigned, MONAI's distance_field to the power alpha, 0 < alpha <= 16)   (sqrt(d2_to) + sqrt(d2_from))^alpha, of which one
 *                                              root is 0: alpha = 2 is the integer d2 converted once, alpha = 1 its fp64 root rounded
 *                                              once, else one fp32 exp((alpha / 2) log d2), 0 at d2 = 0.  A second pair (d2_to_b,
 *                                              d2_from_b; both or neither) adds its own field: prediction plus target, one fp32 add.
 * This library's rule for an empty or a full S -- either map of the pair holds -1, at every pixel of that image --: the plane, or in
 * mode 1 that pair's addend, is 0 there.                                                                                              */
int cmu_distance_field(const int32_t* d2_to, const int32_t* d2_from, const int32_t* d2_to_b, const int32_t* d2_from_b, int mode,
                       double alpha, float* field, int plane, int B, int K, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A segmented key sort and the Lovasz-Softmax loss built on it (csrc/key_sort.hip, csrc/key_sort.h, csrc/lovasz.hip, DESIGN.md
 * section 4.26; no reference counterpart).  No floating-point atomics, no host sync, the same bits on every call.  There is no
 * workspace query: scratch is the explicit tensors named below, sized in closed form; none needs initialisation, and every element of
 * every output is written on every call.
 *
 * cmu_sort_u64: S segments of n keys each, at keys + s n, every segment sorted ascending on its own into out + s n.  scratch: S n
 * keys, needed when n > T = cmu_sort_tile_keys() (else it may be NULL); it may be `keys` itself, whose contents are then lost --
 * otherwise keys is left as it was.  out is neither of them.  One launch sorts tiles of T keys in LDS (a bitonic network), then
 * ceil(log2(ceil(n / T))) launches merge runs pairwise, partitioned by merge path; a tile never crosses a segment.  The launch count
 * depends on (S, n) alone.  S ceil(n / T) < 2^31.                                                                                      */
int cmu_sort_tile_keys(void);
int cmu_sort_u64(const uint64_t* keys, uint64_t* out, uint64_t* scratch, int64_t S, int64_t n, void* stream);
/* The Lovasz-Softmax loss (Berman et al., 2018) of logits x (B,K,H,W) fp32, 2 <= K <= 8, B <= 65535, over the classes of keep_mask
 * (bit c = class c; Kk of them).  A segment is the whole batch (per_image = 0: S = 1, n = B H W) or one image (S = B, n = H W);
 * n < 2^31.  Per kept class c and segment: e_i = 1 - p_c(i) where the label is c (foreground), else p_c(i); p is the fp32 softmax of
 * cmu_seg_stats_fwd / cmu_index_ce_fwd (the same bits) and 1 - p one fp32 subtraction.  The errors are taken in descending order,
 * equal ones by ascending pixel index (b, h, w) within the segment; with G the foreground count and F_r that among the first r,
 * J_r = 1 - (G - F_r) / (G + r - F_r), g_1 = J_1, g_r = J_r - J_(r-1) (integers, one fp64 quotient, formed without the difference's
 * cancellation), and the class's loss is sum_r e_(r) g_r in fp64.
 *
 * cmu_lovasz_keys: target_kind is a CMU_ICE_* code, the target as cmu_focal_fwd takes it (the arg-max of one-hot planes runs over all
 * K channels; one-hot targets have no ignore_index).  keys: S Kk n uint64, row (s, i-th kept class) at keys + (s Kk + i) n.  A key,
 * from the top: bit 63 "not valid" (the label is ignore_index or outside [0, K): such pixels sort behind every valid one), bits 62..32
 * the low 31 bits of the fp32 error inverted, bits 31..1 the pixel's index in its segment, bit 0 the foreground bit (0 in a key that
 * is not valid) -- below the index, so that it cannot influence the order.  counts: S (K + 1) + 1 int64 -- [s][0] valid pixels,
 * [s][1 + c] pixels of label c for every c < K, then the number of labels outside [0, K) that are not ignore_index (integer atomics
 * on a table the entry clears first: exact in any order).  Such a label is never used as an index.
 * cmu_lovasz_grad: sorted_keys = the rows of cmu_lovasz_keys after cmu_sort_u64(S Kk segments of n).  classes_all = 0: the classes
 * with G > 0 in the segment count ('present'); 1: all kept classes (a class with G = 0 has g = (1, 0, ..): its largest error).
 * coef_s = 1 / (S x the classes that count in s), 0 if none does.  With Tn = ceil(n / cmu_sort_tile_keys()):
 *   wmap     (B,K,H,W) fp32   d loss / d p_c(i) = -+ coef_s g_rank(i) (- on foreground), 0 at pixels that are not valid, at classes
 *                             that are not kept or do not count: the weight map of cmu_softmax_map_bwd(kind 0) with g = the incoming
 *                             gradient in each of its K slots;
 *   out      1 + 2 S + S K fp64   [0] the loss sum_s coef_s L_s; [1 + s] L_s, the sum of the losses of the classes that count in s;
 *                             [1 + S + s] coef_s; [1 + 2 S + s K + c] the loss of class c in s (0 if it does not count);
 *   tile_fg  S Kk Tn int64, partials  S Kk Tn fp64   scratch: foreground keys and sum e g per tile of a sorted row.
 * A label outside [0, K) anywhere makes out[0] NaN and the whole of wmap zero.  Sums: per-lane fp64 -> block partials -> fixed order. */
int cmu_lovasz_keys(const float* x, const void* target, int target_kind, int keep_mask, int per_image, int64_t ignore_index,
                    uint64_t* keys, int64_t* counts, int B, int K, int H, int W, void* stream);
int cmu_lovasz_grad(const uint64_t* sorted_keys, const int64_t* counts, int keep_mask, int per_image, int classes_all, float* wmap,
                    int64_t* tile_fg, double* partials, double* out, int B, int K, int H, int W, void* stream);

/* Measurement support (bench.py's roofline block; no reference counterpart): the 16-bit MFMA rate this chip SUSTAINS.
 * Every wave of a one-workgroup-per-CU grid issues iters x 8 back-to-back 32x32x16 MFMAs from registers (no LDS, no
 * memory) or -- lds_fed = 1 -- the same MFMAs fed from LDS at the persistent conv kernel's ratio (6 fragment reads of 1 KB
 * per 8 MFMAs, register double buffer); operands are generated in the kernel: pattern 0 = dense ~N(0,1), 1 = ReLU'd
 * (half zeros), 2 = all zeros.
 * The power management lowers the shader clock under this load by an amount that depends on the operand data
 * (csrc/probe.hip); *tflops and *clock_mhz (s_memtime / s_memrealtime of one wave) come back
 * after a synchronisation of the stream.  scratch64: 64 bytes of device memory.  Host-blocking; not for the hot path. */
int cmu_mfma_sustained_rate(int dt, int pattern, int lds_fed, int iters, void* scratch64, double* tflops, double* clock_mhz,
                            void* stream);
/* Diagnostic (tools/exchange_probe.py): a stand-in for a collective's reduction kernel -- `grid` workgroups of 256
 * threads compute out = a + b over n floats (n % 4 == 0) `passes` times on `stream`.  Launched on a side stream where a trainer announces a
 * gradient bucket (reference: DDP's bucketed all-reduce, Pretraining/Spark/main.py:102), it shows on ONE GPU whether such a kernel runs beside
 * the persistent conv kernels and what the backward pass loses.  Not used by the product path. */
int cmu_probe_stream_reduce(const float* a, const float* b, float* out, int64_t n, int grid, int passes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CMUNET_HIP_H */
