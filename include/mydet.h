/* mydet.h -- C ABI of libmydet_hip.so: the MI355X (gfx950) kernels behind the
 * single-stage detection inference hot path of duanzhiihao/myDetection.
 *
 * The reference has no FFI seam (it is pure Python over ATen/torchvision); its
 * seams are the Python plug-in factories models/registry.py:4-146 and
 * api/detection.py:19-205.  Each entry point below replaces the third-party native
 * op (ATen / torchvision) that a reference Python call site lands in; the call
 * site is cited per function.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *  - Plain pointers and sizes only.  All pointers are DEVICE pointers (HBM).
 *  - `stream` is a hipStream_t passed as void*; 0 = the null stream.
 *  - Every function only enqueues work on `stream`; it never allocates persistent
 *    memory, never synchronises, and is graph-capturable.  The caller owns all
 *    buffers, including scratch.
 *  - Return value: 0 on success, otherwise a hipError_t, or a negative MYDET_E_*
 *    code for argument errors detected on the host before any launch.
 *  - Activations are float32, channels-last ("NHWC"): element (b,y,x,c) of a
 *    tensor with pixel stride `ld` (in floats, ld >= C) lives at
 *    ((b*H + y)*W + x)*ld + c.  A pixel stride larger than C lets a kernel read
 *    or write a channel slice of a wider buffer (free concat / padding).
 */
#ifndef MYDET_H
#define MYDET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MYDET_ABI_VERSION 2      /* 2 (round 6): mydet_se_tail gained hpart_bytes; mydet_conv3x3_p3_f32 added */

#define MYDET_E_BADARG   (-1)   /* shape/stride/alignment precondition violated */
#define MYDET_E_UNSUPP   (-2)   /* valid request this build has no kernel for   */

/* activation codes for the conv epilogue */
#define MYDET_ACT_NONE   0
#define MYDET_ACT_LEAKY  1      /* LeakyReLU(0.1): models/modules.py:92        */
#define MYDET_ACT_SWISH  2      /* x*sigmoid(x):  models/modules.py:41-43      */

int mydet_abi_version(void);

/* Dense convolution as implicit GEMM on FP32 MFMA (v_mfma_f32_32x32x2_f32), with the
 * epilogue  y = act(acc*scale[n] + shift[n]) + residual  fused.
 * Replaces the conv2d -> batch_norm -> leaky_relu (-> add) ATen chain of
 *   ConvBnLeaky.forward  models/modules.py:94-95   (scale/shift = folded BN, eps 1e-5)
 *   DarkBlock.forward    models/modules.py:69-73   (residual != NULL)
 *   YOLOHead 1x1 convs   models/rpns.py:24-25      (scale NULL => 1, shift = bias)
 * x  : [B,H,W,Cin] pixel stride ldx.   Cin % 4 == 0, ldx % 4 == 0, 16-byte aligned.
 * w  : [Cout][KH][KW][Cin] contiguous (OHWI repack of the reference's OIHW weight).
 * y  : [B,Ho,Wo,Cout] pixel stride ldy.  residual: same shape, pixel stride ldr, or NULL.
 * Ho = (H + pad_t + pad_b - KH)/stride + 1 (likewise Wo); only pad_t/pad_l are
 * needed by the kernel, Ho/Wo are passed explicitly (asymmetric "SAME" pads allowed).
 * a_gate: NULL, or [B][Cin] per-image channel multipliers applied to x while it is staged
 *   (1x1 stride-1 convs without activation only): the squeeze-excite scale
 *   `torch.sigmoid(x_squeezed) * x` feeding `_project_conv`, external/efficientnet/model.py:83-85,
 *   without a pass over the expanded tensor.
 * workspace: NULL, or scratch (16-byte aligned) for the split-K tail: when the grid is a few full rounds of the
 *   chip plus a small remainder, the remainder tiles are cut along K, partial tiles go here and a fixup launch
 *   sums them in a fixed order (deterministic); 64 MiB covers every layer of the three models.
 * Also covers: MBConv expand/project convs (external/efficientnet/model.py:75,85), BiFPN
 * input projections (models/fpns.py:446-448), SeparableConv2d.pointwise (models/modules.py:20),
 * C6/C7 convs (models/backbones.py:183-200), dense cls_last conv (models/rpns.py:155-158).
 * Size limits (32-bit byte offsets; MYDET_E_UNSUPP beyond, nothing launched): the WHOLE output B*Ho*Wo*ldy*4, the whole
 * residual B*Ho*Wo*ldr*4 and the gate B*Cin*4 below 2^31 - 16 bytes (a 64-channel 320x320 output: up to batch 81); the input may be
 * larger -- only H*W*ldx*4 * (256 / (Ho*Wo) + 2), the images one tile can touch, must stay below 2^31 - 16; B*Ho*Wo <= 2^30.
 * The same limits hold for mydet_conv2d_igemm_b3_f32 and mydet_conv1x1_upcat_f32 (both of its inputs as windows).
 */
int mydet_conv2d_igemm_f32(const float *x, int64_t ldx, const float *w,
                           const float *scale, const float *shift,
                           const float *residual, int64_t ldr, const float *a_gate,
                           void *workspace, int64_t workspace_bytes,
                           float *y, int64_t ldy,
                           int B, int H, int W, int Cin, int Cout,
                           int KH, int KW, int stride, int pad_t, int pad_l,
                           int Ho, int Wo, int act, void *stream);

/* The same fused conv + epilogue for KH = KW = 3, stride 1, pad 1 (Ho = H, Wo = W) by Winograd F(2x2,3x3):
 * 16 transform-domain GEMMs on FP32 MFMA with the input/output transforms fused into staging and epilogue
 * (2.25x fewer multiplies; float32 throughout, only the association order of the sums differs from the direct
 * form).  Call sites replaced: the 3x3 ConvBnLeaky of Darknet53 / DarkBlock / YOLOBranch
 * (models/modules.py:69-73,94-95; models/backbones.py:14-41; models/fpns.py:38-47) and the dense 3x3 convs of
 * models/backbones.py:183-200, models/rpns.py:155-158.
 * u: weights in the transform domain, produced once per layer by mydet_wino_weights_f32 from the OHWI weight
 *    (mydet_wino_weights_floats(Cout, Cin) floats; 0 if the shape is unsupported).
 * workspace: NULL, or 16-byte aligned scratch (32 MiB suffices): grids of two or more resident rounds then run a
 *    stream-K schedule -- one round of persistent workgroups with equal shares of the K iterations; items whose K
 *    was cut leave partial outputs here and a fixup launch sums them in K order (deterministic).
 * Needs Cin % 8 == 0, Cout % 4 == 0, ldy % 4 == 0 (ldr % 4 == 0), 16-byte aligned pointers; otherwise
 * MYDET_E_UNSUPP and the caller uses mydet_conv2d_igemm_f32.
 * Size limit (32-bit byte offsets inside a workgroup's window; MYDET_E_UNSUPP beyond): input, output and residual may be of any
 * size, but H*W*max(ldx, ldy, ldr)*4 * (64 / (tiles per image) + 2) -- the images the 64 2x2-output tiles of one workgroup can
 * touch -- must stay below 2^31 - 16 bytes; B * tiles per image <= 2^30.
 */
int64_t mydet_wino_weights_floats(int Cout, int Cin);
int mydet_wino_weights_f32(const float *w_ohwi, int Cout, int Cin, float *u, void *stream);
int mydet_conv2d_wino_f32(const float *x, int64_t ldx, const float *u, const float *scale, const float *shift,
                          const float *residual, int64_t ldr, void *workspace, int64_t workspace_bytes, float *y,
                          int64_t ldy, int B, int H, int W, int Cin, int Cout, int act, void *stream);
/* Test hook (host only, no GPU call): the plan mydet_conv2d_wino_f32 uses for a layer on a chip of `cus` CUs with a workspace
 * of `workspace_bytes` (<= 0 = none: never stream-K).  It is the launcher's own arithmetic, not a copy: the launch takes its numbers
 * from the same function, with the device's CU count for `cus`, and both honour the once-per-process tuning values MYDET_WINO_NW /
 * MYDET_WINO_SK.  out[10] = {
 *   [0] NW: waves per workgroup, 4 (32 tiles of 2x2 outputs per item) or 8 (64 tiles); 8 from Cin = 128 up,
 *   [1] schedule: 0 plain (one workgroup per item, all of K), 1 stream-K (persistent workgroups),
 *   [2] items = tile blocks x 64-channel blocks,   [3] nk = Cin / 8 slab iterations per item,
 *   [4] nwg: persistent workgroups (0 when plain),  [5] whole items per workgroup before the tail (1 when plain),
 *   [6] tail items, cut along K: workgroup w owns the slab iterations [floor(w * T / nwg), floor((w + 1) * T / nwg)) of their
 *       item-major sequence, T = tail items * nk,   [7] skq, [8] skr: T = skq * nwg + skr,
 *   [9] 1 when the fixup launch (tail items x 8 workgroups) follows }.
 * Returns 0, MYDET_E_BADARG, or MYDET_E_UNSUPP for the shapes mydet_conv2d_wino_f32 does not take.  No reference counterpart. */
int mydet_wino_plan(int B, int H, int W, int Cin, int Cout, int64_t workspace_bytes, int cus, int32_t *out);

/* First-layer convolution (Cin == 3, 3x3) reading the image with arbitrary strides
 * (NCHW as handed over by api/detection.py:160-166, or channels-last) and writing NHWC.
 * Replaces netlist[0] of Darknet53 (models/backbones.py:14) and the EfficientNet stem.
 * Cout must be 32.  Strides sxb/sxc/sxh/sxw in floats.
 */
int mydet_conv2d_stem_f32(const float *x, int64_t sxb, int64_t sxc, int64_t sxh, int64_t sxw,
                          const float *w /* [Cout][3][3][3] OHWI */,
                          const float *scale, const float *shift,
                          float *y, int64_t ldy,
                          int B, int H, int W, int Cout, int stride, int pad_t, int pad_l,
                          int Ho, int Wo, int act, void *stream);

/* Depthwise K x K convolution (K = 3 or 5, stride 1 or 2), y = act(conv*scale + shift) (scale/shift NULL =>
 * plain conv).  Replaces `_depthwise_conv` + `_bn1` + swish (external/efficientnet/model.py:77) and
 * SeparableConv2d.depthwise (models/modules.py:12-13,19).  w: [K][K][C] (repack of [C,1,K,K]).
 * se_partial != NULL: the launch also writes per-image channel sums of y split over S pixel slices,
 * se_partial[B][S+1][C] (slices 0..S-1; slice S is scratch for mydet_se_gate_f32) -- the squeeze of the following squeeze-excite (adaptive_avg_pool2d,
 * external/efficientnet/model.py:81) without another pass over y; deterministic (no atomics).
 * S must be mydet_dwconv_slices(Ho, Wo, C, K, stride): the number of slices the kernel chosen for the layer writes
 * (one per 8 x 16 output tile for the LDS-tiled stride-1 kernel, which takes the layers of 32 channels and more).
 * Sizes: x and y are addressed with 64-bit offsets (no byte limit); with se_partial or an in-launch tail the grid has one row per
 * image and B <= 65535 (MYDET_E_BADARG beyond) -- mydet_channel_sums_f32 and mydet_se_gate_f32 likewise.
 */
/* Squeeze-excite tail inside the launch that produces the depthwise output (optional last argument of mydet_dwconv_f32,
 * mydet_mbconv_expand_dw_f32, mydet_stem_dw_f32; NULL = none).  The launch then also writes
 *     gate[b][c] = sigmoid(W2 . swish(W1 . mean_pixels(y[b]) + b1) + b2)[c]          (external/efficientnet/model.py:80-83)
 * -- what mydet_se_gate_f32 computes from se_partial in a launch of its own -- without that launch: every workgroup adds its
 * channels' share of W1 . sums while it holds them and publishes it (fire and forget); the last workgroup of an image waits
 * for the shares, sums them in a fixed order and runs the expand conv (csrc/se_tail.h).  Deterministic.
 *   w1 [Cse][C], b1 [Cse], w2t [Cse][C] (the expand conv TRANSPOSED), b2 [C], gate [B][C]  (all 16-byte aligned);
 *   hpart: the share buffer, 8-byte aligned, MYDET_SE_EPOCH_WORDS + 2 * B * groups * Cse 32-bit words (groups =
 *   mydet_dwconv_se_groups / mydet_mbconv_tiles of the layer): a header of MYDET_SE_EPOCH_WORDS words -- word 0 the launch
 *   counter, 1 when the buffer is made; word 1 the count of finished images, 0; word 2 the number of finishing workgroups that
 *   ever gave up waiting for a share and wrote a NaN gate (0 in a healthy run; never reset by the launches: a caller may poll it);
 *   the rest unused -- then (value, epoch) pairs, zero when the buffer is made.  hpart_bytes = the buffer's size: an entry point
 *   given a smaller one than its layer needs returns MYDET_E_BADARG and launches nothing.  After that only the launches touch it; ONE buffer serves every layer and batch size of a
 *   stream, but never two streams at a time.  Cse <= 96; MYDET_E_UNSUPP beyond.  se_partial may be NULL when the tail is given. */
#define MYDET_SE_EPOCH_WORDS 1024
typedef struct {
    const float *w1, *b1, *w2t, *b2;
    float *gate, *hpart;
    int Cse;
    int64_t hpart_bytes;      /* size of hpart: >= 4 * (MYDET_SE_EPOCH_WORDS + 2 * B * groups * Cse), checked by every entry point */
} mydet_se_tail;
int mydet_dwconv_slices(int Ho, int Wo, int C, int K, int stride);
/* workgroups per image of the kernel mydet_dwconv_f32 picks for the layer when it also emits the squeeze (sizes se->hpart) */
int mydet_dwconv_se_groups(int Ho, int Wo, int C, int K, int stride);
int mydet_dwconv_f32(const float *x, int64_t ldx, const float *w, const float *scale, const float *shift,
                     float *y, int64_t ldy, int B, int H, int W, int C, int K, int stride, int pad_t, int pad_l,
                     int Ho, int Wo, int act, float *se_partial, int S, const mydet_se_tail *se, void *stream);

/* Per-image channel sums of x split over S pixel slices: partial[B][S+1][C], slices 0..S-1 (standalone squeeze). */
int mydet_channel_sums_f32(const float *x, int64_t ldx, int B, int H, int W, int C, float *partial, int S,
                           void *stream);

/* Squeeze-excite gate from the partial sums partial[B][S+1][C]: mean = sum_{s<S} partial[b][s][:] / HW (stored
 * in slice S);
 * gate[b][c] = sigmoid(W2 . swish(W1 . mean + b1) + b2).  Replaces adaptive_avg_pool2d + _se_reduce + swish +
 * _se_expand + sigmoid (external/efficientnet/model.py:80-83).  w1 [Cse][C]; w2t [Cse][C] = _se_expand weight
 * transposed.
 */
int mydet_se_gate_f32(float *partial, int S, int B, int HW, int C, const float *w1, const float *b1, int Cse,
                      const float *w2t, const float *b2, float *gate, void *stream);

/* 3x3 stride-2 pad-1 max pool (-inf padding): nn.MaxPool2d(3, 2, 1) models/backbones.py:186,188,
 * tnf.max_pool2d models/fpns.py:405-416. */
int mydet_maxpool3s2_f32(const float *x, int64_t ldx, float *y, int64_t ldy, int B, int H, int W, int C,
                         int Ho, int Wo, void *stream);

/* BiFPN node input: y = swish(sum_i w_i * in_i), w = relu(weights) / (sum(relu(weights)) + 1e-4)
 * (LinearFusion.forward models/fpns.py:433-438, the part before spconv_bn).  n = 2 or 3 inputs of C
 * channels; mode_i: 0 = [B,H,W] map, 1 = [B,H/2,W/2] map read through nearest 2x upsampling
 * (upsample2x, models/fpns.py:442-444), 2 = [B,2H,2W] map read through max_pool2d(3,2,1). */
int mydet_bifpn_fuse_f32(int n, const float *in0, int64_t ld0, int mode0, const float *in1, int64_t ld1, int mode1,
                         const float *in2, int64_t ld2, int mode2, const float *weights, float *y, int64_t ldy,
                         int B, int H, int W, int C, void *stream);

/* y[b,yo,xo, 0:C1] = a[b, nearest(yo), nearest(xo), :]  ;  y[..., C1:C1+C2] = b[b,yo,xo,:]
 * Replaces F.interpolate(mode='nearest') + torch.cat((pre, x), 1) of
 * YOLOBranch.forward models/fpns.py:62-65.  C1, C2, strides multiples of 4.
 * If C2 == 0 / b == NULL it is a plain nearest resize.
 */
int mydet_upsample_concat_f32(const float *a, int64_t lda, int Ha, int Wa, int C1,
                              const float *b, int64_t ldb, int C2,
                              float *y, int64_t ldy, int B, int Ho, int Wo, void *stream);

/* The same concatenation consumed on the fly by the 1x1 ConvBnLeaky that follows it in YOLOBranch.forward
 * (models/fpns.py:62-66: `x = cat((upsample(pre), x), 1); x = self.cbl_0(x)`):
 *   y = LeakyReLU_0.1((conv1x1(cat((up2x_nearest(x_lo), x_hi), 1)) * scale + shift)
 * x_lo [B,H/2,W/2,ld_lo] (C_lo channels), x_hi [B,H,W,ld_hi] (C_hi channels), w [Cout][C_lo + C_hi] (OHWI, the
 * concatenation's channel order), y [B,H,W,ldy].  The concatenated tensor is never written; the sums run in the same k
 * order and tile shape as mydet_conv2d_igemm_f32 on the materialised tensor: bit-identical results.
 * workspace: as for mydet_conv2d_igemm_f32.  Needs H, W even, C_lo % 32 == 0, C_hi % 32 == 0, act == MYDET_ACT_LEAKY,
 * AND a shape that mydet_conv2d_igemm_f32 itself would run on its 64 x 64 x 32 tile (the only tile this entry point is
 * instantiated for: e.g. 64 < Cout, C_lo + C_hi <= 1024 or fewer than 1024 tiles of 128 x 128 -- YOLOv3's 768->256 and
 * 384->128 layers); otherwise MYDET_E_UNSUPP and the caller uses mydet_upsample_concat_f32 + mydet_conv2d_igemm_f32,
 * so the bit-identity above holds for every shape the call accepts. */
int mydet_conv1x1_upcat_f32(const float *x_lo, int64_t ld_lo, int C_lo, const float *x_hi, int64_t ld_hi, int C_hi,
                            const float *w, const float *scale, const float *shift, void *workspace,
                            int64_t workspace_bytes, float *y, int64_t ldy, int B, int H, int W, int Cout, int act,
                            void *stream);

/* The implicit GEMM of mydet_conv2d_igemm_f32 on the bfloat16 matrix instructions with float32-exact operands: every
 * float32 operand is cut into three bfloat16 pieces (a = a0 + a1 + a2 by round-to-nearest remainders, exact to 2^-27 |a|), a
 * product is the sum of the six piece products of weight >= 2^-18 (each exact in float32), accumulated in float32 by
 * v_mfma_f32_32x32x16_bf16: per product an error of 2^-26 |a b|, below the rounding of a float32 multiply-add -- the same
 * results as the float32 kernel to float32 round-off (tests hold both to 2e-5 * max|y| against float64) at 2.67 x its matrix
 * rate.  Same arguments as mydet_conv2d_igemm_f32 except: w_planes = the OHWI weight [Cout][K = KH*KW*Cin] as three bfloat16
 * planes in the kernels' slab-major, DMA-swizzled order (csrc/conv_igemm.hip: split_bf16_kernel; Cout padded to 256 rows),
 * made ONCE per layer by mydet_split_bf16_f32 into mydet_split_bf16_elems(Cout, K) uint16; a_gate (optional, 1x1 layers without an
 * activation: the squeeze-excite project convs) multiplies the activations per image and channel before they are split.  Cin % 16 == 0 (1x1 layers: Cin % 4 == 0, the
 * last 16-channel slab of the planes zero-filled by mydet_split_bf16_f32);
 * MYDET_E_UNSUPP otherwise (the caller then uses mydet_conv2d_igemm_f32).  Replaces the same reference lines.
 * Finite tensors only: an infinite operand, or a finite one of magnitude > 3.3962e38 (it rounds to a bfloat16 inf), yields NaN where
 * the float32 kernel and the reference yield inf (the split forms inf - inf); NaN propagates as NaN. */
int64_t mydet_split_bf16_elems(int Cout, int K);      /* uint16 elements of the operand below (0: K % 4 != 0) */
int mydet_split_bf16_f32(const float *w, int Cout, int K, uint16_t *planes, void *stream);
int mydet_conv2d_igemm_b3_f32(const float *x, int64_t ldx, const uint16_t *w_planes, const float *scale, const float *shift,
                              const float *residual, int64_t ldr, const float *a_gate, void *workspace, int64_t workspace_bytes, float *y,
                              int64_t ldy, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad_t,
                              int pad_l, int Ho, int Wo, int act, void *stream);
/* 3x3 convolution, pad 1, stride 1 or 2, on the bfloat16 matrix instructions with the float32-exact split operands of
 * mydet_conv2d_igemm_b3_f32 -- same w_planes, same six piece products, float32 accumulation -- but with the workgroup's INPUT
 * PATCH resident in LDS (csrc/conv_p3.hip): a workgroup owns 8 x 16 output pixels (stride 2: 16 x 8 / 32 x 4 for a remainder of 8 / 4
 * columns) x (64 | 128) output channels, loads and
 * splits the patch of a 16-channel slab once and the nine taps read their matrix operands out of it at tap offsets, instead of
 * gathering and splitting every input element once per tap (2.25 x at stride 2, 9 x at stride 1).  K order (slab, tap) instead of
 * (tap, slab): results equal the other kernels' to float32 round-off (tests: 2e-5 * max|y| against float64).
 *   y = act((conv3x3(x) * scale + shift)) + residual,  Ho = (H - 1) / stride + 1, Wo likewise;  act: MYDET_ACT_NONE | _LEAKY.
 * Cin % 16 == 0, ldx % 4 == 0; MYDET_E_UNSUPP otherwise (the caller then uses mydet_conv2d_igemm_b3_f32 / _igemm_f32).
 * Size limits (descriptors per image; MYDET_E_UNSUPP beyond): (H+1)*(W+1)*ldx*4 and Ho*Wo*max(ldy, ldr)*4 at most 2^31 - 16 bytes,
 * fewer than 2^31 workgroups; the batch may carry every tensor past 4 GiB.  mydet_conv_stem_p3_f32: the same for its output.
 * Replaces the ATen chain of models/modules.py:76-95 for the stride-2 ConvBnLeaky layers of models/backbones.py:14-30 and the
 * 32 -> 64 layer of the first DarkBlock (models/modules.py:56-73). */
int mydet_conv3x3_p3_f32(const float *x, int64_t ldx, const uint16_t *w_planes, const float *scale, const float *shift,
                         const float *residual, int64_t ldr, float *y, int64_t ldy, int B, int H, int W, int Cin, int Cout,
                         int stride, int act, void *stream);
/* Test and dispatch hook (host only, no GPU call): the tile plan mydet_conv3x3_p3_f32 launches for an Ho x Wo map of Cout output
 * channels.  out[8] = {channel tile BN (64 | 128), strip shape of the remainder columns (0 none, 1 = 16 x 8, 2 = 32 x 4 tiles),
 * tx_n, ty_n (8 x 16 tiles per image row / column), main_tiles = tx_n * ty_n, tiles_img (+ the strip tiles, which start at column
 * 16 * tx_n), channel tiles, dynamic LDS bytes of the kernel form}; workgroups = B * tiles_img * channel tiles.  It is the launcher's
 * own function, not a copy, and reads the same MYDET_P3_FORM / MYDET_P3_STRIP (once per process).  Returns 0, MYDET_E_BADARG or
 * (stride not 1 | 2) MYDET_E_UNSUPP.  No reference counterpart. */
int mydet_conv3x3_p3_plan(int Ho, int Wo, int Cout, int stride, int32_t *out);
/* The 3 -> 32 stem (3x3, stride 1; mydet_conv2d_stem_f32) and the 3x3 stride-2 pad-1 layer behind it (mydet_conv3x3_p3_f32) as ONE
 * launch (csrc/conv_stem_p3.hip): the workgroup of the second layer's 8 x 16-pixel x 64-channel tile computes the 17 x 33-pixel stem
 * patch it needs on the matrix instructions, straight into the LDS patch its nine taps read -- the 32-channel full-resolution map is
 * never written or read back.
 *   y = act1(conv3x3_s2_pad1(act0(conv3x3_s1(x) * scale0 + shift0)) * scale1 + shift1),  act: MYDET_ACT_NONE | _LEAKY.
 * x: logical [B,3,H,W] read through its element strides; stem output Hs x Ws with pad_t / pad_l as mydet_conv2d_stem_f32;
 * y [B,Ho,Wo,ldy], Ho = (Hs - 1) / 2 + 1, Wo likewise.  w0_planes = mydet_split_bf16_f32 of the stem's OHWI weight with every row's
 * K = 27 zero-padded to 32 (Cout 32, K 32); w1_planes = mydet_split_bf16_f32 of the second layer's [Cout][3][3][32] weight.
 * Both layers use the split-bf16 arithmetic of mydet_conv2d_igemm_b3_f32 (float32 round-off; tests: 2e-5 * max|y| against float64).
 * C0 == 32, stride0 == 1, stride1 == 2, Cout % 64 == 0; MYDET_E_UNSUPP otherwise (the caller then uses the two launches).
 * ldy % 4 == 0, ldy >= Cout, y and the planes 16-byte aligned; MYDET_E_BADARG otherwise.
 * Replaces netlist[0] and netlist[1] of models/backbones.py:14-30 (models/modules.py:76-95, twice). */
int mydet_conv_stem_p3_f32(const float *x, int64_t sxb, int64_t sxc, int64_t sxh, int64_t sxw, const uint16_t *w0_planes,
                           const float *scale0, const float *shift0, int act0, const uint16_t *w1_planes, const float *scale1,
                           const float *shift1, int act1, float *y, int64_t ldy, int B, int H, int W, int C0, int Cout,
                           int stride0, int pad_t, int pad_l, int Hs, int Ws, int stride1, void *stream);
int mydet_conv_stem_p3_lds_bytes(void);               /* dynamic LDS of that launch (one resident patch slab + the image patch) */
/* Test hook: the split-bf16 launcher reads MYDET_B3_WIDE / MYDET_B3_WAVES / MYDET_B3_HALF_TILES once per process; this reads them
 * again.  Returns the form bits (1 = wide 128 x 256 tiles from 192 output channels, 2 = 8-wave workgroups). */
int mydet_conv_b3_reload_tuning(void);

/* Test / tuning hook: workgroups per CU the runtime reports (hipOccupancyMaxActiveBlocksPerMultiprocessor) for the
 * base instance of conv_igemm tile configuration `cfg` (0, 1, 2, 3, 6, 8, 9); *assumed = the count the launch rule
 * computes its rounds with.  Returns the count or a negative MYDET_E_*.  No reference counterpart. */
int mydet_conv_igemm_occupancy(int cfg, int *assumed);

/* Test hook (host only, no GPU call): the plan mydet_conv2d_igemm_f32 uses for a layer on a chip of `cus` CUs.
 * cfg < 0: the rule's own choice (choose_cfg); otherwise that configuration.  out[7] = {cfg id, BM, BN, BK,
 * tiles in the main launch, tail tiles cut along K, cuts per tail tile (1 = no tail)}.  Returns 0 or MYDET_E_*.
 * taps = KH * KW; workspace_bytes <= 0 = no workspace (never a tail).  It is the launcher's own arithmetic, not a copy: the
 * tile table and the round / K-cut rule are the functions the launch calls.  (Not part of it: the 1x1 layers with at most 48
 * output channels and 65 536 rows or more, which mydet_conv2d_igemm_f32 hands to the skinny pointwise kernel first.)
 * No reference counterpart. */
int mydet_conv_igemm_plan(int cfg, int B, int Ho, int Wo, int Cin, int Cout, int taps,
                          int64_t workspace_bytes, int cus, int32_t *out);
/* Test hook (host only, no GPU call): the plan mydet_conv2d_igemm_b3_f32 uses for a layer on a chip of `cus` CUs, under the
 * MYDET_B3_* switches as last read.  out[7] = {form (0 default, 1 wide, 2 8-wave), BM, BN, waves along N, workgroups of the main
 * launch, tail tiles cut along K (0 = no tail), cuts per tail tile (1 = no tail)}.  taps = KH * KW; gated != 0: with a squeeze-excite
 * gate (the opt-in forms have no gated instance: the default form runs); workspace_bytes <= 0 = no workspace (never a tail).
 * It is the launcher's own arithmetic, not a copy: the form choice and the round / K-cut rule are the function the launch calls.
 * Returns 0, MYDET_E_BADARG, or MYDET_E_UNSUPP for the channel counts the entry point refuses (Cin % 16 with more than one tap,
 * Cin % 4, Cin % 16 under the wide form with Cout > 192).  No reference counterpart. */
int mydet_conv_b3_plan(int B, int Ho, int Wo, int Cin, int Cout, int taps, int gated, int64_t workspace_bytes, int cus,
                       int32_t *out);

/* Focus.forward of the Ultralytics backbone (external/ultralytics/common.py:79-86): 2x2 space-to-depth,
 *   y[b, yo, xo, g*C + c] = x[b, c, 2*yo + dy, 2*xo + dx],  g = 0:(dy 0, dx 0) 1:(dy 1, dx 0) 2:(dy 0, dx 1) 3:(dy 1, dx 1)
 * -- the channel order of torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1).
 * x: logical [B,C,H,W] read through its element strides (sb, sc, sh, sw), H and W even; y: channels-last
 * [B,H/2,W/2,ldy], ldy >= 4C, ldy % 4 == 0.  The 3x3 conv that follows is mydet_conv2d_igemm_f32 on 4C channels. */
int mydet_space_to_depth_f32(const float *x, int64_t sb, int64_t sc, int64_t sh, int64_t sw, float *y, int64_t ldy,
                             int B, int C, int H, int W, void *stream);

/* SPP.forward of the Ultralytics backbone (external/ultralytics/common.py:59-70), the part between its two convs:
 *   y[..., 0:C] = x,  y[..., C:2C] = maxpool_k0(x),  y[..., 2C:3C] = maxpool_k1(x),  y[..., 3C:4C] = maxpool_k2(x)
 * with nn.MaxPool2d(kernel_size=k, stride=1, padding=k//2) (-inf padding); k0 <= k1 <= k2 odd (5, 9, 13).
 * x [B,H,W,ldx], y [B,H,W,ldy], C % 4 == 0, ldy >= 4C. */
int mydet_spp_concat_f32(const float *x, int64_t ldx, float *y, int64_t ldy, int B, int H, int W, int C, int k0, int k1,
                         int k2, void *stream);

/* Box decode of one pyramid level: raw head logits -> (bbox cxcywh, class_idx, score)
 * for every candidate, written into the level's slice [n_off, n_off + A*H*W) of the
 * per-image candidate arrays (models/general.py:74-76 concatenates levels along dim 1).
 *   mode MYDET_DECODE_YOLO   YOLOLayer.forward        models/detlayers/yolov3.py:41-69
 *   mode MYDET_DECODE_RETINA RetinaLayer.forward      models/detlayers/retinanet.py:63-82
 *   mode MYDET_DECODE_FCOS   FCOS_ATSS_Layer.forward  models/detlayers/fcos2.py:222-251
 *   mode MYDET_DECODE_RAPID  RAPiDLayer.forward       models/detlayers/rapid.py:36-81 (inference branch)
 * box : [B,H,W,*] pixel stride ldbox; anchor a's 4 box logits (5 for RAPID) at a*box_astride + box_c0
 * cls : [B,H,W,*] pixel stride ldcls; anchor a's C class logits at a*cls_astride + cls_c0,
 *       its objectness/centerness logit (YOLO, FCOS) at a*cls_astride + conf_c0.
 *       (YOLO head: box == cls, astride 5+C, box_c0 0, conf_c0 4, cls_c0 5.  RAPID on a YOLO head: astride 6+C,
 *       conf_c0 5, cls_c0 6.)  1 <= C <= 128; RAPID also takes C == 0 (no class logit is read, class 0).
 * anchors_wh: HOST pointer (the one exception to "device pointers only") to A pairs (w,h)
 *       in pixels (A <= 16); the pairs travel as kernel arguments so the launch stays
 *       graph-capturable (YOLO, RETINA; ignored for FCOS, where A == 1).
 * Candidate order inside a level is (a, y, x), x fastest.  N = candidates per image.
 * Outputs: bbox [B,N,4] f32 ([B,N,5] for RAPID), class_idx [B,N] i64, score [B,N] f32.
 * ldbox, ldcls multiples of 4; 16-byte aligned bases.
 * RAPID (rotated boxes, bbox rows (cx, cy, w, h, deg)): cx, cy, w, h as YOLO; deg = ((s(t4)*2*pi - pi)/pi)*180 in
 *   float32 with pi the float32 constant, in (-180, 180); score = s(conf) when C == 0, else
 *   sqrt(s(conf) * max_c s(cls_c)) with class_idx the first argmax (torch.max).
 */
#define MYDET_DECODE_YOLO   0
#define MYDET_DECODE_RETINA 1
#define MYDET_DECODE_FCOS   2
#define MYDET_DECODE_RAPID  3
typedef struct mydet_decode_level {
    const float *box; int64_t ldbox;     /* device */
    const float *cls; int64_t ldcls;     /* device */
    const float *anchors_wh;             /* HOST, A pairs, or NULL (FCOS) */
    int H, W;
    float stride;
    int64_t n_off;                       /* first candidate of this level inside [0, N) */
} mydet_decode_level;
/* All pyramid levels in one launch (the per-level loop of models/general.py:69-72 + the torch.cat of :74-76);
 * `levels` is a HOST array of nlevels (<= 5) descriptors; the other arguments as for mydet_decode_f32. */
int mydet_decode_levels_f32(int mode, int nlevels, const mydet_decode_level *levels, int box_astride, int box_c0,
                            int cls_astride, int cls_c0, int conf_c0, int A, int C, int B, int img_h, int img_w,
                            float *bbox, int64_t *class_idx, float *score, int64_t N, void *stream);
/* The Ultralytics (YOLOv5) decode, DetectLayer.forward models/detlayers/uv5.py:42-91 (inference branch), every level in one
 * launch.  It has an entry point of its own because the `mode` argument above is closed: values above MYDET_DECODE_RAPID are
 * rejected by mydet_decode_f32 / mydet_decode_levels_f32.  Layout, anchors, candidate order, outputs and argument checks
 * are those of mydet_decode_levels_f32 with MYDET_DECODE_YOLO (1 <= C <= 128, anchors required, bbox [B,N,4]); the score
 * and class_idx are YOLO's bit for bit.  Only the box differs, in float32 in this operation order:
 *   s = sigmoid(t[0..3]);  cx = ((s0*2 - 0.5) + x) * stride, cy likewise with y;  w = ((s2*2) * (s2*2)) * anchor_w, h likewise.
 * Nothing is clamped: cx, cy >= -stride/2 and w, h <= 4 * anchor. */
int mydet_decode_uv5_levels_f32(int nlevels, const mydet_decode_level *levels, int box_astride, int box_c0,
                                int cls_astride, int cls_c0, int conf_c0, int A, int C, int B, int img_h, int img_w,
                                float *bbox, int64_t *class_idx, float *score, int64_t N, void *stream);
int mydet_decode_f32(int mode,
                     const float *box, int64_t ldbox, int box_astride, int box_c0,
                     const float *cls, int64_t ldcls, int cls_astride, int cls_c0, int conf_c0,
                     const float *anchors_wh, int A, int C,
                     int B, int H, int W, float stride, int img_h, int img_w,
                     float *bbox, int64_t *class_idx, float *score, int64_t N, int64_t n_off,
                     void *stream);

/* Batched confidence filter -> top-k -> class-aware greedy NMS, one image per workgroup.
 * Replaces ImageObjects.post_process / non_max_suppression (utils/structures.py:92-173)
 * and torchvision.ops.nms; the candidates never leave HBM.
 *   keep score >= conf_thres (float32 compare); if more than `topk` (<=512) pass, keep the
 *   topk highest (ties: lowest candidate index); per class ascending: greedy NMS on
 *   x1y1x2y2 = (cx-w/2, cy-h/2, cx+w/2, cy+h/2), suppress when (double)IoU > nms_thres;
 *   survivors ordered class ascending, score descending (ties: lowest index).
 *   Order of the scores: that of float32 `<`, from -inf to +inf, subnormals included (nothing is flushed).  -0.0 and +0.0
 *   are ONE score: they tie, and the lowest index wins, in the top-k and inside a class; out_score keeps each candidate's
 *   own bits.  A NaN score fails the filter for every conf_thres (a NaN conf_thres included) and is never selected.
 * In : bbox [B,N,4], class_idx [B,N] i64, score [B,N].   N < 2^20, class ids in [0, 2^12): an image in which a
 *      candidate that passes the filter / top-k carries a class id outside that range gets
 *      count = MYDET_COUNT_BAD_CLASS (-1) and all-zero rows instead of silently aliased classes.
 * Out: count [B] i32; out_bbox [B,topk,4]; out_class [B,topk] i64; out_score [B,topk];
 *      out_index [B,topk] i32 = candidate index in [0,N) of each survivor (rows >= count
 *      are zero-filled).
 * scratch: B*N*8 bytes.
 */
int mydet_postprocess_f32(const float *bbox, const int64_t *class_idx, const float *score,
                          int B, int64_t N, float conf_thres, double nms_thres, int topk,
                          int32_t *count, float *out_bbox, int64_t *out_class, float *out_score,
                          int32_t *out_index, void *scratch, void *stream);

/* Same post-processing (topk = 512), written as ONE fixed-size record per image -- the wire format of the
 * multi-GPU exchange (one all-gather of these records; no reference counterpart), so nothing is
 * packed or unpacked between the kernel and the collective.  A record is MYDET_REC_WORDS int32 words
 * (16 400 B, rows 16-byte aligned):
 *   [COUNT] count i32, 3 zero words | [BBOX] 512 x (cx,cy,w,h) f32 | [SCORE] 512 f32 |
 *   [CLASS] 512 i64 | [INDEX] 512 i32          (entries >= count are zero)
 * records: B * MYDET_REC_WORDS words, 16-byte aligned.  scratch: B*N*8 bytes.
 */
#define MYDET_COUNT_BAD_CLASS (-1)
#define MYDET_REC_TOPK   512
#define MYDET_REC_COUNT  0
#define MYDET_REC_BBOX   4
#define MYDET_REC_SCORE  (MYDET_REC_BBOX + 4 * MYDET_REC_TOPK)
#define MYDET_REC_CLASS  (MYDET_REC_SCORE + MYDET_REC_TOPK)
#define MYDET_REC_INDEX  (MYDET_REC_CLASS + 2 * MYDET_REC_TOPK)
#define MYDET_REC_WORDS  (MYDET_REC_INDEX + MYDET_REC_TOPK)
int mydet_postprocess_records_f32(const float *bbox, const int64_t *class_idx, const float *score,
                                  int B, int64_t N, float conf_thres, double nms_thres,
                                  int32_t *records, void *scratch, void *stream);

/* Rotated boxes (bb_format 'cxcywhd', rows (cx, cy, w, h, deg)): the same filter, top-k, sort and NMS, on columns 0-3
 * only -- the reference's non_max_suppression builds the axis-aligned x1y1x2y2 from them and calls torchvision.ops.nms
 * for 'cxcywhd' too (utils/structures.py:137-149; its rotated NMS is not on the inference path).  The angle travels
 * with its box.  For every input, count / class / score / index and box columns 0-3 equal those of the 4-column
 * entry points on bbox[..., 0:4] bit for bit, and each angle is bbox[b, index, 4].
 *   mydet_postprocess_rot_f32:         arguments as mydet_postprocess_f32, bbox [B,N,5], out_bbox [B,topk,5].
 *   mydet_postprocess_records_rot_f32: a ROTATED record per image, MYDET_REC_ROT_WORDS words (18 448 B): the
 *                                      4-column record (every field at its offset; BBOX stays a 512 x 4 plane, so
 *                                      mydet_bboxes_to_original_batched_f32 applies unchanged) + [ANGLE] 512 f32. */
#define MYDET_REC_ANGLE     MYDET_REC_WORDS
#define MYDET_REC_ROT_WORDS (MYDET_REC_WORDS + MYDET_REC_TOPK)
int mydet_postprocess_rot_f32(const float *bbox, const int64_t *class_idx, const float *score,
                              int B, int64_t N, float conf_thres, double nms_thres, int topk,
                              int32_t *count, float *out_bbox, int64_t *out_class, float *out_score,
                              int32_t *out_index, void *scratch, void *stream);
int mydet_postprocess_records_rot_f32(const float *bbox, const int64_t *class_idx, const float *score,
                                      int B, int64_t N, float conf_thres, double nms_thres,
                                      int32_t *records, void *scratch, void *stream);

/* Rotated-IoU NMS for 'cxcywhd' boxes (opt-in; the two entry points above are what the reference's inference path runs).
 * Arguments, argument checks, error codes, outputs and the record (MYDET_REC_ROT_WORDS words) are those of
 * mydet_postprocess_rot_f32 / mydet_postprocess_records_rot_f32; filter, top-k, class-aware greedy order and the tie order
 * (score descending, then candidate index ascending, as everywhere in this file) are unchanged.  Only the pair test differs:
 *   - the IoU of two boxes is the EXACT area of intersection of the two rotated rectangles over their union, in float32.
 *     The rectangles have the corners of the reference's xywha2vertex (utils/bbox_ops.py:137-172: angle clockwise in image
 *     coordinates, radians = deg * pi / 180 in float32, on deg reduced modulo 90 exactly).  The reference's iou_rle (utils/bbox_ops.py:52-100) counts the
 *     pixels of the rasterised rectangles instead; the exact area is a documented deviation (within 7.2e-4 of the
 *     reference's own 512^2 mask IoU on tests/golden/rot_iou.npz).
 *   - a box is suppressed when (double)IoU >= nms_thres -- `>=`, as nms_rotbb tests it (utils/bbox_ops.py:290), where
 *     the axis-aligned entry points use torchvision's `>`.  A pair of two zero-area boxes has no IoU (0/0) and is not
 *     suppressed.
 * mydet_rotated_iou_f32: the same IoU for every pair of two sets of rows (cx, cy, w, h, deg): a [Na,5], b [Nb,5] ->
 *   out [Na,Nb] (the exact-area counterpart of iou_rle).  Na or Nb == 0 is a no-op. */
int mydet_rotated_iou_f32(const float *a, int64_t Na, const float *b, int64_t Nb, float *out, void *stream);
int mydet_postprocess_rotnms_f32(const float *bbox, const int64_t *class_idx, const float *score,
                                 int B, int64_t N, float conf_thres, double nms_thres, int topk,
                                 int32_t *count, float *out_bbox, int64_t *out_class, float *out_score,
                                 int32_t *out_index, void *scratch, void *stream);
int mydet_postprocess_records_rotnms_f32(const float *bbox, const int64_t *class_idx, const float *score,
                                         int B, int64_t N, float conf_thres, double nms_thres,
                                         int32_t *records, void *scratch, void *stream);

/* NMS modes: class-agnostic suppression, Soft-NMS (Bodla et al. 2017) and box merging, inside the same one-workgroup-per-image
 * launch.  No reference counterpart (ImageObjects.post_process has the class-aware hard NMS only).
 * Filter, top-k, the NaN rule and the class-id check (MYDET_COUNT_BAD_CLASS) are those of mydet_postprocess_f32; call their
 * result the SELECTED list.  A mode is (kind, agnostic, sigma, min_score):
 *   Groups.  agnostic == 0: one group per class.  agnostic == 1: all selected boxes are one group.
 *   Order P inside a group: score descending, candidate index ascending (-0 and +0 tie), as everywhere in this file.
 *   Pair value o(i,j), for every kind: the axis-aligned float32 IoU of mydet_postprocess_f32 -- corners cx -/+ w/2, area
 *     (x2-x1)*(y2-y1), inter / (a_i + a_j - inter), no contraction; 0/0 is NaN and never suppresses or decays.  Boxes of width 5
 *     (cxcywhd) use columns 0-3 and the angle travels with its box, as in mydet_postprocess_rot_f32.
 *   MYDET_NMS_HARD           greedy in order P; j is suppressed when (double)o > nms_thres.  With agnostic == 0 this IS
 *                            mydet_postprocess_f32 (the same kernel instance, the same bits).
 *   MYDET_NMS_SOFT_LINEAR /  a working score t_j = s_j per box.  Per group, repeat: pick the remaining box with the largest t
 *   MYDET_NMS_SOFT_GAUSSIAN  (tie: lowest candidate index); stop the group -- the rest of it is dropped -- unless t >= min_score
 *                            (float32); emit the box with score t; then for every remaining k
 *                              linear:   if (double)o > nms_thres:  t_k = t_k * (1.0f - o)
 *                              gaussian: t_k = t_k * (float)exp(-((double)o * (double)o) / sigma)   (exp in double, rounded once;
 *                                        nms_thres is not used)
 *                            A NaN o leaves t_k unchanged; a t_k that becomes NaN (inf * 0) drops box k.
 *                            Requires conf_thres >= 0, min_score >= 0 and, for gaussian, sigma > 0: MYDET_E_BADARG otherwise.
 *   MYDET_NMS_MERGE          HARD first.  Then for every kept box i: its cluster is i itself plus every box j of its group with
 *                            (double)o(i,j) > nms_thres, kept or not.  In ascending position of P accumulate in float64
 *                            W += s_j, X1 += s_j*x1_j, likewise Y1, X2, Y2 (the float32 corners, widened); x1' = X1/W, ...;
 *                            the output row is ((float)((x1'+x2')*0.5), (float)((y1'+y2')*0.5), (float)(x2'-x1'), (float)(y2'-y1')).
 *                            Score, class and index are those of i.  Requires conf_thres > 0 (so W > 0): MYDET_E_BADARG
 *                            otherwise.  Box width 4 only: the _rot_ entry points return MYDET_E_UNSUPP (no mean of angles).
 * Output order for every kind: class ascending, and inside a class the order of selection -- order P for HARD and MERGE, the
 *   order of emission (non-increasing t) for the soft kinds.  Rows past the count are zero.  out_score holds t for the soft
 *   kinds, out_index the candidate index.  Outputs, records, scratch and every other argument rule are those of the entry point
 *   without _nms_.  A null mode, an unknown kind or an agnostic outside {0, 1} is MYDET_E_BADARG.  An error launches nothing.
 * Not provided: the exact rotated pair test (mydet_postprocess_rotnms_f32) together with a mode -- there is no such entry
 *   point, and mydet_merge_tile_records_nms_f32 returns MYDET_E_UNSUPP for rotated_nms with agnostic. */
#define MYDET_NMS_HARD          0
#define MYDET_NMS_SOFT_LINEAR   1
#define MYDET_NMS_SOFT_GAUSSIAN 2
#define MYDET_NMS_MERGE         3
typedef struct mydet_nms_mode {
    int kind;                         /* MYDET_NMS_* */
    int agnostic;                     /* 0 | 1 */
    double sigma;                     /* SOFT_GAUSSIAN only */
    float min_score;                  /* the soft kinds only */
    int reserved;                     /* 0 */
} mydet_nms_mode;
int mydet_postprocess_nms_f32(const float *bbox, const int64_t *class_idx, const float *score,
                              int B, int64_t N, float conf_thres, double nms_thres, int topk, const mydet_nms_mode *mode,
                              int32_t *count, float *out_bbox, int64_t *out_class, float *out_score,
                              int32_t *out_index, void *scratch, void *stream);
int mydet_postprocess_records_nms_f32(const float *bbox, const int64_t *class_idx, const float *score,
                                      int B, int64_t N, float conf_thres, double nms_thres, const mydet_nms_mode *mode,
                                      int32_t *records, void *scratch, void *stream);
int mydet_postprocess_rot_nms_f32(const float *bbox, const int64_t *class_idx, const float *score,
                                  int B, int64_t N, float conf_thres, double nms_thres, int topk, const mydet_nms_mode *mode,
                                  int32_t *count, float *out_bbox, int64_t *out_class, float *out_score,
                                  int32_t *out_index, void *scratch, void *stream);
int mydet_postprocess_records_rot_nms_f32(const float *bbox, const int64_t *class_idx, const float *score,
                                          int B, int64_t N, float conf_thres, double nms_thres, const mydet_nms_mode *mode,
                                          int32_t *records, void *scratch, void *stream);

/* Merge of tile records: tiled ("sliced") detection on large frames.  The detector ran on T windows of each of B frames
 * (overlapping tiles at native resolution, optionally the whole frame as one more window); this call turns the B x T
 * per-window records into B per-frame records with one more class-aware NMS in frame coordinates.  No reference counterpart.
 * In : the record of window t of frame b at tile_records + t*tile_stride_words + b*frame_stride_words: a record of
 *      MYDET_REC_WORDS (box_width 4) or MYDET_REC_ROT_WORDS (box_width 5) words whose boxes are in the window's own pixel
 *      coordinates (the state after mydet_bboxes_to_original_batched_f32).  Tile-major [T][B] and frame-major [B][T] buffers
 *      are both strides of this form.  origins: DEVICE int32 [T][2] = (x0, y0) of each window in the frame.
 * Candidates: frame b has T*512 of them.  Candidate t*512 + k, k < count[b,t], is slot k of that record with
 *      cx + (float)x0_t and cy + (float)y0_t (one float32 add each); w, h, angle, score and class unchanged.  Slots
 *      k >= count carry a NaN score and are never selected.  If any window of a frame has count == MYDET_COUNT_BAD_CLASS,
 *      so has the frame's record.
 * Out: records [B], wire layout, exactly what mydet_postprocess_records_f32 (box_width 4), mydet_postprocess_records_rot_f32
 *      (5) or, with rotated_nms != 0, mydet_postprocess_records_rotnms_f32 gives on those candidates with conf_thres = -inf:
 *      top-k 512 by (score descending, candidate index ascending) -- on a score tie the earlier window wins --, the
 *      class-aware greedy NMS, output order class ascending then score descending, every slot past the count zero.
 *      INDEX holds t*512 + k: window index >> 9 and slot index & 511 of every survivor.  records must not overlap
 *      tile_records.
 * metric: the pair test of the axis-aligned NMS.
 *      MYDET_MERGE_IOU  inter / (area_i + area_j - inter), the test of mydet_postprocess_f32.
 *      MYDET_MERGE_IOS  "intersection over smaller": inter / fminf(area_i, area_j) in float32, inter and the areas computed
 *                       in the same operation order as for the IoU; a box is suppressed when (double)value > nms_thres; two
 *                       boxes without area give 0/0 and are not suppressed.  It merges an object cut by a window seam: the
 *                       truncated box lies inside the whole one, so its IoU is small and its IoS about 1.
 *      MYDET_MERGE_IOS with rotated_nms is MYDET_E_UNSUPP.
 * scratch: mydet_merge_tile_records_scratch_bytes(B, T, box_width) bytes (the candidate arrays and the selection's key
 *      strip; 0 for arguments the merge rejects), 16-byte aligned; the call is two launches on `stream` (a gather of the
 *      candidates, then the post-process kernel itself) and stream-ordered.
 * MYDET_E_BADARG: B <= 0; T outside [1, MYDET_TILES_MAX]; box_width not 4 or 5; an unknown metric; rotated_nms with
 *      box_width 4; a null pointer; tile_records, records or scratch not 16-byte aligned; a stride that is negative or no
 *      multiple of 4 words; scratch_bytes too small. */
#define MYDET_TILES_MAX 64
#define MYDET_MERGE_IOU 0
#define MYDET_MERGE_IOS 1
int64_t mydet_merge_tile_records_scratch_bytes(int B, int T, int box_width);
int mydet_merge_tile_records_f32(const int32_t *tile_records, int64_t tile_stride_words, int64_t frame_stride_words,
                                 int B, int T, int box_width, const int32_t *origins, double nms_thres, int metric,
                                 int rotated_nms, int32_t *records, void *scratch, int64_t scratch_bytes, void *stream);
/* The same merge with `agnostic` (0 | 1; MYDET_E_BADARG otherwise): with 1 the merge's hard NMS has ONE group of all candidates
 * (NMS modes above: HARD with agnostic; output order class ascending, inside a class order P).  Both metrics apply.  agnostic
 * with rotated_nms is MYDET_E_UNSUPP.  agnostic == 0 is mydet_merge_tile_records_f32. */
int mydet_merge_tile_records_nms_f32(const int32_t *tile_records, int64_t tile_stride_words, int64_t frame_stride_words,
                                     int B, int T, int box_width, const int32_t *origins, double nms_thres, int metric,
                                     int rotated_nms, int agnostic, int32_t *records, void *scratch, int64_t scratch_bytes,
                                     void *stream);

/* Fusion of view records: test-time augmentation.  The detector ran on V views of each of B frames -- the frame mirrored by
 * flips[v] (MYDET_VIEW_HFLIP | MYDET_VIEW_VFLIP bits, mydet_frames_to_input_flip_f32 below), at any network input size -- and
 * this call turns the B x V per-view records into B per-frame records.  No reference counterpart; the view transform is the
 * reference's hflip / vflip label rule (utils/augmentation.py) read backwards.
 * In : the record of view v of frame b at view_records + v*view_stride_words + b*frame_stride_words, wire layout
 *      (MYDET_REC_WORDS or MYDET_REC_ROT_WORDS words), its boxes in the pixel coordinates of the MIRRORED frame (the state after
 *      mydet_bboxes_to_original_batched_f32).  Strides, alignment and the bad-class rule are those of
 *      mydet_merge_tile_records_f32.  flips: HOST int32 [V], read during the call (it travels in the kernel arguments).
 * Candidates: frame b has V*512.  Candidate v*512 + k, k < count[b,v], is slot k with
 *      cx' = (float)frame_w - cx  when HFLIP (one float32 subtraction),  cy' = (float)frame_h - cy  when VFLIP,
 *      angle' = -angle (box_width 5) when exactly ONE of the two bits is set, not wrapped; everything else unchanged.
 * mode (kind, metric, rotated_nms, agnostic, min_score):
 *   MYDET_FUSE_NMS  exactly what mydet_merge_tile_records_nms_f32 gives for these candidates with all origins zero (so cx' and
 *                   cy' also take its + (float)0: a -0 centre becomes +0), with its metric / rotated_nms / agnostic and its
 *                   MYDET_E_UNSUPP combinations; thres is its nms_thres.  Two launches: the merge's gather with the view
 *                   transform, then the post-process kernel itself.  With every flip 0 the output equals that call's on the same
 *                   buffer bit for bit.  min_score is not used.
 *   MYDET_FUSE_WBF  Weighted Boxes Fusion (Solovyev et al. 2021).  box_width 4 only (5 is MYDET_E_UNSUPP: no mean of angles, as
 *                   for MYDET_NMS_MERGE); metric must be MYDET_MERGE_IOU and rotated_nms 0 (MYDET_E_UNSUPP otherwise).
 *                   A candidate whose score is not > 0 is skipped.  The others are visited in order P (score descending,
 *                   candidate index ascending, -0 = +0).  Cluster j keeps, in creation order, float64 sums Wt, X1, Y1, X2, Y2, a
 *                   member count n, the class and candidate index of its first member, and its fused row
 *                     F_j = ((float)((x1'+x2')*0.5), (float)((y1'+y2')*0.5), (float)(x2'-x1'), (float)(y2'-y1')),  x1' = X1/Wt, ...
 *                   (the formula of MYDET_NMS_MERGE, also for a cluster of one).  For candidate c of class q: eligible are the
 *                   clusters of class q (agnostic: all); o_j is the axis-aligned float32 IoU of mydet_postprocess_f32 between
 *                   F_j and c's row (corners cx -/+ w/2 of both in float32); c joins the eligible cluster with the largest o_j
 *                   among those with (double)o_j > thres (tie: lowest j; NaN never matches):
 *                     Wt += s; X1 += s*x1; Y1 += s*y1; X2 += s*x2; Y2 += s*y2 (c's float32 corners and score widened to
 *                     double); n += 1; F_j recomputed.
 *                   Without a match c founds cluster number (clusters so far) if that is < 512, and is dropped otherwise (it
 *                   is among the lowest scores).  A cluster's score is f = (float)((Wt / n) * ((double)min(n, V) / (double)V));
 *                   clusters with f < min_score (float32) are dropped.  Rows: class ascending, f descending, creation index
 *                   ascending; each row is F_j, SCORE f, CLASS the first member's, INDEX the first member's v*512 + k; slots
 *                   past the count zero.  A view with count == MYDET_COUNT_BAD_CLASS, or a candidate with score > 0 and a class
 *                   outside [0, 4096), makes the frame's count MYDET_COUNT_BAD_CLASS.  Two launches: the gather, then one
 *                   workgroup per frame (sort of the <= 4096 keys and the cluster table in LDS, 66 KiB).
 *                   This is not the `ensemble-boxes` package bit for bit, on purpose: float32 IoU against the RUNNING fused box,
 *                   the tie rules above, the 512-cluster cap.
 * scratch: mydet_fuse_view_records_scratch_bytes(B, V, box_width, kind) bytes (0 for arguments the call rejects), 16-byte
 *      aligned.  records must not overlap view_records.  Stream-ordered.
 * MYDET_E_BADARG, nothing launched: V outside [1, MYDET_VIEWS_MAX]; a flip outside 0..3; frame_h or frame_w <= 0; a null mode or
 *      an unknown kind; min_score negative or NaN; and the pointer, alignment, stride, box_width, metric, agnostic and scratch
 *      rules of mydet_merge_tile_records_nms_f32.  `reserved` is ignored. */
#define MYDET_VIEWS_MAX 8
#define MYDET_FUSE_NMS 0
#define MYDET_FUSE_WBF 1
typedef struct mydet_fuse_mode {
    int kind;                         /* MYDET_FUSE_* */
    int metric;                       /* MYDET_MERGE_* */
    int rotated_nms, agnostic;        /* 0 | 1 */
    float min_score;                  /* WBF only */
    int reserved;
} mydet_fuse_mode;
int64_t mydet_fuse_view_records_scratch_bytes(int B, int V, int box_width, int kind);
int mydet_fuse_view_records_f32(const int32_t *view_records, int64_t view_stride_words, int64_t frame_stride_words,
                                int B, int V, int box_width, const int32_t *flips, int frame_h, int frame_w,
                                double thres, const mydet_fuse_mode *mode, int32_t *records,
                                void *scratch, int64_t scratch_bytes, void *stream);

/* Tracking of detections across video frames on the device: persistent identities and Kalman-filtered boxes from the detection
 * records of consecutive frames.  The state model is the reference's KFTracklet (utils/structures.py:445-529) over
 * RotBBoxKalmanFilter (utils/kalman_filter.py:77-142): constant velocity on (cx, cy, w, h, angle), diagonal P0 / Q / R with the
 * rows of cx, cy, w, h and of their velocities scaled by the box area w*h, the angle kept in [0, 180), a score with momentum.
 * Its 10 x 10 covariance stays five 2 x 2 blocks (pxx, pxv, pvv), which is how it is stored.  The reference has no loop around
 * that model; the association below is this library's.
 *
 * One launch advances S independent streams by F consecutive frames each (one workgroup per stream, the frames in order).
 * In : the record of frame f of stream s at records + s*stream_stride_words + f*frame_stride_words: a record of MYDET_REC_WORDS
 *      (box_width 4) or MYDET_REC_ROT_WORDS (box_width 5) words in frame coordinates (after
 *      mydet_bboxes_to_original_batched_f32).  A 4-wide record runs the same filter with angle 0.
 * Per frame, in this order (float32; csrc/track.hip is built with -ffp-contract=off and DESIGN.md section 4 has the operation order):
 *   predict   every live track: a = w*h of the state before the step; pxx += 2 pxv + pvv + q_x, pxv += pvv, pvv += q_v with
 *             q_x = q[i]*a, q_v = q[5+i]*a for i < 4 and q[4], q[9] for the angle; x += v; angle %= 180 (Python's %: in
 *             [0, 180)); from the second consecutive prediction on, score *= momentum; missed += 1.
 *   associate detections in (score descending, record slot ascending) order.  Each takes, among the live tracks of its own
 *             class that no earlier detection took, the one whose predicted box has the largest IoU with it, if that IoU is
 *             > match_thres; on equal IoU the lower track slot.  IoU: MYDET_TRACK_MATCH_IOU the axis-aligned IoU of
 *             mydet_postprocess_f32 on (cx, cy, w, h) (box i = the detection, j = the track); MYDET_TRACK_MATCH_ROTATED
 *             (box_width 5 only) the exact rotated IoU of mydet_rotated_iou_f32, a = the detection, b = the track.
 *   update    every matched track (KFTracklet.update): z4 = angle % 180, replaced by the nearest of z4, z4 - 180, z4 + 180 to the
 *             state angle (the first on a tie); a = w*h of the predicted state; per parameter y = z - x, inv = 1 / (pxx + r),
 *             r = r[i]*a (i < 4) or r[4]; kx = pxx*inv, kv = pxv*inv; x += kx*y, v += kv*y; pxx -= kx*pxx, pxv -= kx*pxv,
 *             pvv -= kv*pxv (old values on the right); angle %= 180; score = momentum*score + (1 - momentum)*detection score;
 *             missed = 0.
 *   retire    a live track with score < min_score, cx, cy, w or h < 0, cx > img_w, cy > img_h, w > img_w, h > img_h
 *             (KFTracklet.is_feasible), or missed >= max_missed.  Its slot becomes free (all zero) and its id is never used again.
 *   births    every unmatched detection with score >= new_thres, in the association order, into the lowest free slot (slots
 *             freed in this frame included) with the stream's next id (int64, from 1): x = the box with angle % 180, v = 0,
 *             pxx = p0[i]*a (i < 4) or p0[4], pvv = p0[5+i]*a or p0[9], pxv = 0, score = the detection's, missed = 0.  Without
 *             a free slot the detection is dropped and counted.
 * Out (dense, frame o = s*F + f): out_box [S*F][max_tracks][5], out_score, out_class i64, out_id i64 (0: a free slot),
 *      out_missed i32 (0: matched or born in this frame; k: k frames since; -1: a free slot) [S*F][max_tracks];
 *      out_count [S*F] the live tracks after the frame, out_dropped [S*F].  A frame whose record count is
 *      MYDET_COUNT_BAD_CLASS leaves the state as it is; its out_count is that sentinel, its slots are written as free.
 * params: HOST pointer; the struct travels as a kernel argument.  p0, q, r are VARIANCES (the reference's constants squared).
 * state: S * mydet_track_state_words(max_tracks) int32 words, 16-byte aligned, caller-owned, persistent between launches and
 *      initialised by mydet_track_reset.  Per stream, in words, MT = max_tracks:
 *        [0, 2) next id (int64)   [2] live tracks   [3, 8) zero
 *        [8, 8 + 2 MT) class (int64 [MT])           then id (int64 [MT]; 0 = free)
 *        then float planes [5][MT] each: x (cx, cy, w, h, angle), v, pxx, pxv, pvv
 *        then score [MT] f32, missed [MT] i32; zero padding to a multiple of 4 words.
 * MYDET_E_BADARG: S, F or max_tracks < 1; box_width not 4 or 5; an unknown params->match, or MATCH_ROTATED with box_width 4; a null
 *      pointer; records or state not 16-byte aligned; a stride that is negative or no multiple of 4 words; a misaligned
 *      output.  MYDET_E_UNSUPP: max_tracks > MYDET_TRACK_MAX_TRACKS.  mydet_track_state_words is 0 for such a max_tracks. */
#define MYDET_TRACK_MAX_TRACKS    512
#define MYDET_TRACK_STATE_HEADER  8      /* words before the planes */
#define MYDET_TRACK_SLOT_WORDS    31     /* words per track: 2 + 2 + 25 + 1 + 1 */
#define MYDET_TRACK_MATCH_IOU     0
#define MYDET_TRACK_MATCH_ROTATED 1
typedef struct mydet_track_params {
    float p0[10], q[10], r[5];           /* variances: initial covariance, process noise, measurement noise */
    float momentum, min_score, new_thres, match_thres;
    float img_h, img_w;
    int max_missed, match;
} mydet_track_params;
int64_t mydet_track_state_words(int max_tracks);
int mydet_track_reset(int32_t *state, int S, int max_tracks, void *stream);
int mydet_track_frames_f32(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S, int F,
                           int box_width, const mydet_track_params *params, int max_tracks, int32_t *state,
                           float *out_box, float *out_score, int64_t *out_class, int64_t *out_id, int32_t *out_missed,
                           int32_t *out_count, int32_t *out_dropped, void *stream);

/* Association modes of the tracker.  mydet_track_frames_assoc_f32 is mydet_track_frames_f32 with one more argument, `assoc` (HOST
 * pointer; the struct travels as a kernel argument); mydet_track_frames_f32 is it with {MYDET_TRACK_ASSIGN_GREEDY, bands 0}.
 * Predict, update, retire, births and every output are as documented above; only the "associate" step has modes, through two
 * independent settings.
 * Score bands (bands = 1; with bands = 0 there is one band and the three thresholds are not read):
 *   a detection with score >= high_thres is HIGH, one with low_thres <= score < high_thres is LOW, one below low_thres is
 *   ignored: neither matched nor born.  Births come only from unmatched HIGH detections with score >= new_thres, in the same
 *   order as before.  Stage 1 associates the HIGH detections with every live track at params->match_thres.  Stage 2 associates
 *   the LOW detections, at low_match_thres, with the live tracks that no stage-1 detection took AND whose missed == 1 after
 *   this frame's predict: the tracks matched or born in the previous frame (ByteTrack's rule).  A track matched in stage 2
 *   takes the normal update, score momentum included.
 * Assignment inside a stage:
 *   MYDET_TRACK_ASSIGN_GREEDY   the walk documented above.  With bands one walk in rank order is stage 1 and then stage 2 (every
 *             HIGH detection precedes every LOW one); the threshold and the eligibility change at the boundary.
 *   MYDET_TRACK_ASSIGN_OPTIMAL  rows: the stage's detections in rank order (score descending, record slot ascending); columns: the
 *             track slots 0 .. max_tracks-1 in order, then one dummy column per row.  With iou the float32 IoU of the greedy
 *             mode and q = (int)floorf(iou * 65536.0f): cost = 65536 - q for an eligible pair -- the track is live, not taken
 *             by an earlier stage, of the detection's class, passes the stage-2 missed rule, and iou > the stage's threshold (a
 *             NaN IoU is never eligible); cost = 131072 for an ineligible pair on a real column; cost = 65536 on a dummy
 *             column.  The result is the minimum-cost assignment as the shortest-augmenting-path method finds it (the solver
 *             of mydet_mot_clear_f64): rows inserted in ascending order, the next column the unused one of least reduced
 *             cost, the lowest column index on a tie.  A row that ends on a dummy column is unmatched.
 * MYDET_E_BADARG: as mydet_track_frames_f32, and a null assoc; an unknown assign; bands not 0 or 1; with bands a non-finite
 *      threshold or low_thres >= high_thres.  reserved is not read. */
#define MYDET_TRACK_ASSIGN_GREEDY  0
#define MYDET_TRACK_ASSIGN_OPTIMAL 1
typedef struct mydet_track_assoc {
    int assign;                          /* MYDET_TRACK_ASSIGN_GREEDY 0 | _OPTIMAL 1 */
    int bands;                           /* 0 | 1 */
    float high_thres, low_thres, low_match_thres;
    int reserved[3];
} mydet_track_assoc;
int mydet_track_frames_assoc_f32(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S, int F,
                                 int box_width, const mydet_track_params *params, int max_tracks, int32_t *state,
                                 float *out_box, float *out_score, int64_t *out_class, int64_t *out_id, int32_t *out_missed,
                                 int32_t *out_count, int32_t *out_dropped, const mydet_track_assoc *assoc, void *stream);

/* Counting tracks in zones and across lines on the device: one launch behind the tracker launch reads the tracker's dense outputs
 * (a track keeps its slot for life) and keeps, per stream, who is inside which polygon, who went through which directed line,
 * for how long, and where the anchors fell.  Every decision is an integer comparison; tests/_zones_ref.py restates the rules and
 * the kernel (csrc/zones.hip) equals it with ==.  The reference project counts people per frame only (draw_bboxes_on_np prints
 * `Count: N`); the rules below are this library's.
 *
 * Geometry: fixed point, 1/16 pixel.  q(v) = (int32) floorf(min(max(v * 16.0f, -1048576.0f), 1048576.0f)) in float32; the caller
 *   quantises polygon vertices and line end points with the same formula (mydet_zone_set holds the quantised values).  A track's
 *   anchor is (cx, cy) of its out_box (MYDET_ZONE_ANCHOR_CENTER) or (cx, cy + h / 2.0f) (MYDET_ZONE_ANCHOR_BOTTOM), in float32;
 *   a track whose anchor has a non-finite coordinate is unobserved in that frame; p = (q(x), q(y)) otherwise.  Frame sizes up to
 *   32768; cross products in int64.
 * Limits: at most MYDET_ZONES_MAX polygons of 3 .. MYDET_ZONE_MAX_VERTICES vertices and at most MYDET_ZONES_MAX directed lines A -> B.
 * Inside (even-odd, half-open): the edge (a, b) -- consecutive vertices, the last with the first -- toggles when
 *   (a.y > p.y) != (b.y > p.y) and, with d = b.y - a.y: (p.x - a.x) * d < (b.x - a.x) * (p.y - a.y) for d > 0, > for d < 0.
 *   A point on the shared edge of two adjacent polygons is inside exactly one of them.
 * Side of a line: side(p) = sign((B.x - A.x) * (p.y - A.y) - (B.y - A.y) * (p.x - A.x)).
 * Per stream, per frame, per track slot t, in this order (now = the stream's frame counter, kept in the state):
 *   1. bad-class frame (out_count < 0): the slot state stands; inside = 0, crossed = 0, dwell = -1 for every slot; the per-frame
 *      rows are written from the state; now still advances.
 *   2. close   if the state holds an id for t and the tracker's id of t differs (track gone, or slot reused): for every zone z
 *      whose bit is set lost[z] += 1, visits[z] += 1, dwell_sum[z] += now - entered[t][z], dwell_max[z] = max(dwell_max[z],
 *      now - entered[t][z]); then the slot state is cleared (all zero).
 *   3. observe when id != 0, the class passes the filter (n_classes == 0, or cls is one of classes[0 .. n_classes)), missed == 0
 *      (coasting = 1: missed >= 0) and the anchor is finite.  A live but unobserved track keeps its state and its dwell goes on.
 *      Observed, with p the quantised anchor: the slot adopts the id if its state is empty.  Every polygon z: outside -> inside
 *      gives entries[z] += 1, entered[t][z] = now, bit z set (a track born inside is an entry); inside -> outside gives
 *      exits[z] += 1, visits[z] += 1, now - entered[t][z] added to dwell_sum[z] and maxed into dwell_max[z], bit z cleared,
 *      entered[t][z] = 0.  Every line l, s = side(p): if s != 0 and a remembered side exists and differs from s, the segment test
 *      decides -- A and B must not lie strictly on the same side of the line through the previously observed anchor p' and p:
 *      sign(cross(p - p', A - p')) * sign(cross(p - p', B - p')) <= 0, cross(u, v) = u.x * v.y - u.y * v.x -- and if it passes
 *      pos[l] += 1 (s > 0) or neg[l] += 1 (s < 0) and bit 2l (pos) or 2l + 1 (neg) of the slot's `crossed` is set; a track that
 *      passes around a line's end is not counted.  Whenever s != 0 the remembered side becomes s; with s == 0 it stays (a track
 *      that sits on the line and goes back is not counted, one that continues is counted once).  Finally p' = p.
 *   4. outputs (frame o = s*F + f, Z = n_polygons, L = n_lines): out_inside i32 [S*F][MT] the zone bits of the slot, 0 unless
 *      the slot state's id equals the tracker's id; out_crossed i32 [S*F][MT] the frame's crossing bits; out_dwell i32
 *      [S*F][MT][Z] now - entered[t][z] where out_inside has bit z, else -1; out_occupancy i32 [S*F][Z] the slots whose state has
 *      bit z after the frame (unobserved live tracks included); cumulative after the frame out_zone_counts i32 [S*F][Z][4]
 *      (entries, exits, lost, visits) and out_line_counts i32 [S*F][L][2] (pos, neg).
 *   5. heat map (heat_h > 0): every observed anchor with missed == 0, 0 <= p.x < 16 img_w and 0 <= p.y < 16 img_h adds 1 to cell
 *      (p.y * heat_h / (16 img_h), p.x * heat_w / (16 img_w)) (integer division) of heat i32 [S][heat_h][heat_w], which
 *      accumulates across launches (the caller zeroes it).
 *   6. now += 1.
 * Two launches of F1 and F2 frames leave exactly the state and the outputs of one launch of F1 + F2 frames.
 * One workgroup per stream, thread = track slot, the frames in order.  In: the tracker's out_box [S*F][MT][5], out_id, out_class
 * (i64), out_missed, out_count of the SAME S, F and max_tracks.  zs: HOST pointer; the struct travels as a kernel argument.
 * state: S * mydet_zones_state_words(max_tracks) int32 words, 16-byte aligned, caller-owned, persistent between launches and
 *      initialised (all zero) by mydet_zones_reset.  Per stream, in words, MT = max_tracks:
 *        [0] now   [1, 4) zero   [4, 68) zone counts [16][4] (entries, exits, lost, visits)   [68, 100) line counts [16][2]
 *        [100, 116) dwell_max [16]   [116, 148) dwell_sum (int64 [16])
 *        [148, 148 + 2 MT) id (int64 [MT]; 0 = an empty slot)   then i32 planes [MT] each: inside (zone bits), sides (2 bits per
 *        line l at 2l: 0 none, 1 positive, 2 negative), px, py (the previously observed anchor)   then entered [16][MT];
 *        zero padding to a multiple of 4 words.
 * MYDET_E_BADARG: S, F or max_tracks < 1; a null pointer (out_dwell, out_occupancy, out_zone_counts may be null with no polygon,
 *      out_line_counts with no line, heat with heat_h == 0); a misaligned pointer; no polygon and no line; more than
 *      MYDET_ZONES_MAX of either; a vertex count outside 3 .. 16; a coordinate outside +-1048576; a polygon whose doubled area is 0;
 *      a line with A == B; n_classes outside 0 .. 16; anchor or coasting not 0 or 1; img_h or img_w outside 1 .. 32768; heat_h,
 *      heat_w not both 0 or both in 1 .. MYDET_ZONE_MAX_HEAT.  MYDET_E_UNSUPP: max_tracks > MYDET_TRACK_MAX_TRACKS
 *      (mydet_zones_state_words is 0 for such a max_tracks). */
#define MYDET_ZONES_MAX            16
#define MYDET_ZONE_MAX_VERTICES    16
#define MYDET_ZONE_MAX_CLASSES     16
#define MYDET_ZONE_MAX_HEAT        1024
#define MYDET_ZONE_MAX_FRAME       32768
#define MYDET_ZONE_COORD_MAX       1048576  /* |q(v)| <= this */
#define MYDET_ZONE_ANCHOR_CENTER   0
#define MYDET_ZONE_ANCHOR_BOTTOM   1
#define MYDET_ZONES_STATE_HEADER   148      /* words before the slot planes */
#define MYDET_ZONES_SLOT_WORDS     22       /* words per slot: 2 + 4 + 16 */
typedef struct mydet_zone_set {
    int n_polygons, n_lines, n_classes;
    int anchor;                          /* MYDET_ZONE_ANCHOR_* */
    int coasting;                        /* 0 | 1 */
    int img_h, img_w;
    int heat_h, heat_w;                  /* 0, 0: no heat map */
    int reserved[3];
    int n_vertices[MYDET_ZONES_MAX];
    int polygon[MYDET_ZONES_MAX][MYDET_ZONE_MAX_VERTICES][2];      /* quantised (x, y) */
    int line[MYDET_ZONES_MAX][4];        /* quantised A.x, A.y, B.x, B.y */
    int classes[MYDET_ZONE_MAX_CLASSES];
} mydet_zone_set;
int64_t mydet_zones_state_words(int max_tracks);
int mydet_zones_reset(int32_t *state, int S, int max_tracks, void *stream);
int mydet_zones_frames(const float *box, const int64_t *id, const int64_t *cls, const int32_t *missed, const int32_t *count,
                       int S, int F, int max_tracks, const mydet_zone_set *zs, int32_t *state, int32_t *heat,
                       int32_t *out_inside, int32_t *out_crossed, int32_t *out_dwell, int32_t *out_occupancy,
                       int32_t *out_zone_counts, int32_t *out_line_counts, void *stream);

/* Track trails: where each track's anchor was in its last frames, kept on the device by one launch behind the tracker launch
 * (csrc/overlay.hip), for the overlay painter below.  It has the shape of mydet_zones_frames: one workgroup per stream, thread =
 * track slot, the frames in order, the tracker's dense out_box / out_id / out_class / out_missed / out_count of the SAME S, F and
 * max_tracks as input; q(v) and the anchors are those of mydet_zones_frames.  tests/_overlay_ref.py restates the rules and the
 * kernel equals it with ==.
 * Per stream, per frame, per track slot t, in this order (L = max_points, 2 .. MYDET_TRAIL_MAX_POINTS):
 *   1. bad-class frame (out_count < 0): the state stands; the outputs come from the state.
 *   2. clear   if the state holds an id for t and the tracker's id of t differs: id = 0, fill = 0, head = 0, the ring all zero.
 *   3. push    when id != 0, missed == 0, the class passes the filter (n_classes == 0, or cls is one of classes[0 .. n_classes))
 *      and the anchor is finite: the slot adopts the id if its state is empty; ring[head] = p = (q(x), q(y)); head = (head + 1)
 *      mod L; fill = min(fill + 1, L).  (A coasting track pushes nothing: its trail ends at its last matched anchor.)
 *   4. outputs (frame o = s*F + f): out_points i32 [S*F][MT][L][2] the ring newest first -- entry k is ring[(head - 1 - k) mod L]
 *      for k < fill, zero beyond --; out_len i32 [S*F][MT] the fill, 0 unless the state's id equals the tracker's id; out_bbox i32
 *      [S*F][MT][4] (min x, min y, max x, max y) of those fill points, zeros with fill == 0.
 * Two launches of F1 and F2 frames leave exactly the state and the outputs of one launch of F1 + F2 frames.
 * ts: HOST pointer.  state: S * mydet_trails_state_words(max_tracks, max_points) int32 words, 16-byte aligned, caller-owned,
 *      persistent, initialised (all zero) by mydet_trails_reset.  Per stream, in words, MT = max_tracks:
 *        [0, 2 MT) id (int64 [MT]; 0 = an empty slot)   [2 MT, 3 MT) fill   [3 MT, 4 MT) head   then ring i32 [MT][L][2];
 *        zero padding to a multiple of 4 words.
 * MYDET_E_BADARG, with nothing launched: S, F or max_tracks < 1; a null or misaligned pointer; max_points outside
 *      2 .. MYDET_TRAIL_MAX_POINTS; anchor not MYDET_ZONE_ANCHOR_*; n_classes outside 0 .. MYDET_ZONE_MAX_CLASSES.
 *      MYDET_E_UNSUPP: max_tracks > MYDET_TRACK_MAX_TRACKS (mydet_trails_state_words is 0 for such a max_tracks, and for a
 *      max_points outside its range). */
#define MYDET_TRAIL_MAX_POINTS     32
typedef struct mydet_trail_set {
    int max_points;                      /* L */
    int anchor;                          /* MYDET_ZONE_ANCHOR_* */
    int n_classes, reserved;
    int classes[MYDET_ZONE_MAX_CLASSES];
} mydet_trail_set;
int64_t mydet_trails_state_words(int max_tracks, int max_points);
int mydet_trails_reset(int32_t *state, int S, int max_tracks, int max_points, void *stream);
int mydet_trails_frames(const float *box, const int64_t *id, const int64_t *cls, const int32_t *missed, const int32_t *count,
                        int S, int F, int max_tracks, const mydet_trail_set *ts, int32_t *state, int32_t *out_points,
                        int32_t *out_len, int32_t *out_bbox, void *stream);

/* Camera motion: one global integer shift (dx, dy) per frame, estimated from the frames themselves on the device
 * (csrc/motion.hip), for the tracker's predict step (mydet_track_frames_motion_f32 below).  On a pan, a shake or a drone every
 * box jumps together and the IoU with the constant-velocity prediction fails for all tracks at once; the information is in the
 * pixels, not in the boxes (BoT-SORT's camera-motion compensation; the reference project has nothing like it).  Everything
 * is an integer; tests/_motion_ref.py restates the rules and the kernels equal it with == on every output and on the state.
 *
 * The estimator runs per stream: frame f of stream s is frame o = s*F + f of the B = S*F frames of the call.  The previous frame of
 * frame f is frame f-1 of the call; for f = 0 it is the last frame of the previous call, of which the state keeps what is needed.
 * Luma L(y, x), 0 .. 255: RGB frames (77 R + 150 G + 29 B + 128) >> 8; 4:2:0 planes the Y sample as 8 bits (the 10-bit rule of
 *   mydet_yuv420_src: s8 = min(255, (v10 + 2) >> 2)); matrix, range and chroma play no part.
 * Reduced luma, k = `reduce` in {2, 4, 8} (0: the smallest k with max(H, W) <= 512 k, else 8 -- mydet_motion_default_reduce):
 *   hr = H / k, wr = W / k (integer division), r(i, j) = (sum of the k x k lumas at (i k, j k) + k*k/2) >> log2(k*k).  Rows and columns from
 *   hr k, wr k on are not read.
 * Blocks, R = `search` in MYDET_MOTION_MIN_SEARCH .. MYDET_MOTION_MAX_SEARCH reduced pixels: nby = (hr - 2R) / 16, nbx = (wr - 2R) / 16,
 *   nb = nby nbx; block b = by nbx + bx is 16 x 16 with its origin (y0, x0) = (R + 16 by, R + 16 bx) in the PREVIOUS reduced luma.
 * Coarse stage, per block: for every (dy, dx) in [-R, R]^2 the SAD of the previous block against the current reduced luma at
 *   (y0 + dy, x0 + dx).  The best candidate is the smallest (SAD, dy*dy + dx*dx, dy, dx), compared lexicographically: a tie
 *   goes to the smaller motion.  smin = its SAD, smax = the largest SAD of the block.  The block is VALID when
 *   smax - smin >= min_texture (a flat block fails) and 2 smin <= smax (a block whose content is gone fails).  With fewer
 *   than min_blocks valid blocks (0: max(2, ceil(nb / 8))) the frame's result is (0, 0, valid 0).  Otherwise D = the
 *   component-wise LOWER MEDIAN of (cdx, cdy) over the valid blocks: the element at index (n - 1) / 2 of the ascending sort.
 * Refine stage, at full resolution, valid blocks only: P = min(32, 8 k); the P x P patch of the previous luma has its origin at
 *   (py, px) = ((y0 + 8) k - P/2, (x0 + 8) k - P/2).  For every (ey, ex) in [-k, k]^2 the SAD against the current luma at
 *   (py + D.y k + ey, px + D.x k + ex); the best by (SAD, ey*ey + ex*ex, ey, ex); the block's vector is D k + e.  The geometry
 *   keeps every read inside the frame.
 * Result: (dx, dy) = the component-wise lower median of the block vectors, in whole pixels: content at p in the previous frame
 *   is at p + d in this one; valid = 1; n_valid = the number of valid blocks.  The first frame of a stream after a reset is
 *   (0, 0, 0, 0).  Not part of these rules: masking detections out, motion beyond R k; rotation, zoom and sub-pixel shifts are
 *   the similarity model's (mydet_motion_warp_frames_rgb_u8 below).
 * Out: out_shift int32 [S*F][4] = (dx, dy, valid, n_valid); out_blocks (may be NULL) int32 [S*F][nb][6] = (cdx, cdy, smin, smax,
 *   fdx, fdy), the block vector in (fdx, fdy); fields are zero where they are undefined (everything in a stream's first frame
 *   after a reset; fdx, fdy of an invalid block and of a frame without enough valid blocks).
 * state: S * mydet_motion_state_words(H, W, k, R) int32 words, 16-byte aligned, caller-owned, persistent, initialised (all zero)
 *   by mydet_motion_reset.  Per stream, with wrp = wr rounded up to a multiple of 4:
 *        [0] seen (0 | 1)   [1, 4) zero   then the reduced luma of the last frame, bytes [hr][wrp] (the padding columns zero)
 *        then its nb patches, bytes [nb][P][P]; zero padding to a multiple of 4 words.
 *   Two calls of F1 and F2 frames leave exactly the outputs and the state of one call of F1 + F2.
 * ws: device scratch of at least mydet_motion_workspace_bytes(S*F, H, W, k, R) bytes, 16-byte aligned, stream-ordered.
 * Frames are read in place: RGB packed pixels with any row and frame stride (as mydet_frames_to_input_f32); 4:2:0 through
 *   mydet_yuv420_src, every layout.  set: HOST pointer.
 * MYDET_E_BADARG, with nothing launched: B or S < 1 or B no multiple of S; a null or misaligned pointer; reduce not 0, 2, 4, 8;
 *   search out of range; H / k or W / k below 2R + 16; a negative min_texture or min_blocks; a workspace too small; a frame
 *   side above 32768; the source errors of the pixel format.  MYDET_E_UNSUPP: more than MYDET_MOTION_MAX_BLOCKS blocks
 *   (mydet_motion_state_words and _workspace_bytes are 0 for every refused geometry). */
#define MYDET_MOTION_MIN_SEARCH    4
#define MYDET_MOTION_MAX_SEARCH    16
#define MYDET_MOTION_MAX_BLOCKS    1024
#define MYDET_MOTION_STATE_HEADER  4        /* words before the reduced luma */
typedef struct mydet_motion_set {
    int reduce;                          /* k: 2 | 4 | 8, or 0 for the default of the frame size */
    int search;                          /* R, reduced pixels */
    int min_texture, min_blocks;         /* min_blocks 0: max(2, ceil(nb / 8)) */
    int reserved[4];                     /* read by mydet_motion_warp_frames_* only: [0] the model (MYDET_MOTION_MODEL_SIMILARITY), [1] the
                                            tolerance, [2] max_zoom, [3] max_rotation, Q16, 0 for the defaults; mydet_motion_frames_*
                                            ignore them, as they always did */
} mydet_motion_set;
int mydet_motion_default_reduce(int H, int W);
int64_t mydet_motion_state_words(int H, int W, int k, int R);
int64_t mydet_motion_workspace_bytes(int frames, int H, int W, int k, int R);
int mydet_motion_reset(int32_t *state, int S, int H, int W, int k, int R, void *stream);
int mydet_motion_frames_rgb_u8(const unsigned char *src, int B, int H, int W, int64_t src_img_bytes, int64_t src_row_bytes, int S,
                               const mydet_motion_set *set, int32_t *state, void *ws, int64_t ws_bytes, int32_t *out_shift,
                               int32_t *out_blocks, void *stream);
int mydet_motion_frames_yuv420(const struct mydet_yuv420_src *src, int B, int H, int W, int S, const mydet_motion_set *set, int32_t *state,
                               void *ws, int64_t ws_bytes, int32_t *out_shift, int32_t *out_blocks, void *stream);

/* Camera motion with rotation and zoom: a four-parameter similarity per frame, fitted to the block vectors of the estimator
 * above (csrc/motion.hip: motion_fit_kernel), for a camera that yaws, rolls, zooms, climbs or descends -- there the block
 * vectors left and right of the centre disagree and their median says little.  Everything is an integer; tests/_warp_ref.py
 * restates the rules and the kernels equal it with == on every output and on the state.
 *
 * The luma, the reduced luma, the blocks, the coarse stage, block validity, min_blocks, the state (layout, reset, the
 * two-calls-equal-one-call rule), the workspace, the frame sources and the errors are those of mydet_motion_frames_rgb_u8; a state
 * may pass between the two families.  Three things differ.
 * Refine stage: the window of a valid block sits at the block's OWN coarse vector c = (cdx, cdy) instead of the median D: for
 *   (ey, ex) in [-k, k]^2 the SAD at (py + c.y k + ey, px + c.x k + ex), the same tie rule, (fdx, fdy) = c k + e.  |c| <= R as
 *   |D| <= R, so the reads stay inside the frame: rows py + c.y k - k .. py + c.y k + k + P lie in [3k, (hr - 3) k], as P <= 8k
 *   and 16 nby <= hr - 2R; columns alike.
 * Fit, over the n valid blocks in ascending block index i.  Block i = by nbx + bx has the lattice point u_i = (bx, by), the
 *   centre p_i = ((R + 16 bx + 8) k, (R + 16 by + 8) k), the half-pixel offset q_i = 2 p_i - (W, H) from the frame centre
 *   c = (W/2, H/2), and the vector d_i = (fdx, fdy).  The model is p -> p + t + (M - I)(p - c), M - I = [[a, -b], [b, a]]; a, b,
 *   t = (tx, ty) are Q16.  Every division is a floor division; (M - I)(p_i - c) in Q16 is m_i = ((a q.x - b q.y) >> 1,
 *   (b q.x + a q.y) >> 1).
 *   Start: h = n / 2; pair i with j = i + (n - h) for i < h; with dp = p_j - p_i, dd = d_j - d_i the pair gives
 *     a_ij = ((dp . dd) << 16) / |dp|^2 and b_ij = ((dp.x dd.y - dp.y dd.x) << 16) / |dp|^2 (|dp|^2 > 0: blocks are distinct).
 *     a, b = the lower medians over the pairs; tx, ty = the lower medians over i of (d_i << 16) - m_i.  No pair (n < 2): invalid.
 *     A block with a foreign motion spoils the pair it is in, so the start tolerates foreign blocks up to a quarter of the
 *     valid ones (half of the pairs), not up to a half.
 *   Two rounds: the inliers are the blocks with |(d_i << 16) - t - m_i| <= tolerance in both components; m = their number;
 *     fewer than 3: invalid.  With the sums over the inliers Su = sum u, Sd = sum d, Sq = sum q:
 *       den = 16 k (m sum |u|^2 - |Su|^2)            (0: invalid; three distinct blocks never give it)
 *       a = ((m sum (u . d) - Su . Sd) << 16) / den,  b = ((m sum (u.x d.y - u.y d.x) - (Su.x Sd.y - Su.y Sd.x)) << 16) / den
 *       tx = ((Sd.x << 17) - (a Sq.x - b Sq.y)) / (2 m),  ty = ((Sd.y << 17) - (b Sq.x + a Sq.y)) / (2 m)
 *     -- the least squares on centred coordinates with numerators and denominator scaled by m^2 / (16 k), and the t that makes
 *     the model exact at the inliers' centroid.  n_inliers and the inlier mask are those of the second round.
 *   int64 holds every intermediate: with n <= 1024, |u| < 512, |d| <= 136, |q| <= 32768 and |a|, |b| < 2^21 (|dd| / |dp| <= 272 / 32)
 *     the largest are the least-squares numerator, below 2^55, and den, below 2^47.
 * Derived: s_q = isqrt((65536 + a)^2 + b^2) (the floor of the root); u = (b << 16) / (65536 + a); deg_q = Q16 degrees of atan(u / 2^16)
 *   = sign(u) ((|u| p) >> 24) with u2 = (u u) >> 16, p = c1 - ((u2 (c3 - ((u2 (c5 - ((u2 c7) >> 16))) >> 16))) >> 16) and
 *   c1, c3, c5, c7 = 961263669, 320421223, 192252734, 137323381 = round(180 / pi / (1, 3, 5, 7) 2^24): within 8 units (0.00013
 *   degrees) of the real arctangent of u / 2^16 on |u| <= 2^14; the floor of u is worth up to 58 more (0.001 degrees in all).  Invalid: |s_q - 65536| > max_zoom; 65536 + a <= 0; |u| > 2^14;
 *   |deg_q| > max_rotation; |tx| or |ty| >= 2^24 (256 pixels, beyond any block vector; below it the tracker's float32 takes t exactly).
 * Settings, the reserved words of mydet_motion_set: [0] = MYDET_MOTION_MODEL_SIMILARITY; [1] = tolerance, Q16 pixels, 0 for 2.0, at
 *   most 16.0; [2] = max_zoom, Q16, 0 for 1/8, at most 1/4; [3] = max_rotation, Q16 degrees, 0 for 7.0, at most 14.0.
 * Out: out_warp int32 [S*F][8] = (a, b, tx, ty, s_q, deg_q, valid, n_inliers), all zero where the frame is invalid (wherever
 *   mydet_motion_frames_rgb_u8 reports valid 0, and the invalid exits above); out_shift int32 [S*F][4] = ((tx + 32768) >> 16,
 *   (ty + 32768) >> 16, valid, n_valid), (0, 0, 0, n_valid) where invalid: the motion of the frame centre in whole pixels, for every
 *   reader of a shift; out_blocks (may be NULL) as above, with (fdx, fdy) = c k + e for every valid block of a frame with at least
 *   min_blocks valid blocks -- also where the fit then leaves by an invalid exit: the block vectors were made and stay written --
 *   and zero for an invalid block and a frame with fewer valid blocks; out_inliers (may be NULL) int32 [S*F][nb], 1 for an inlier of the
 *   second round of a valid frame.  A pure whole-pixel shift of the whole frame gives a = b = 0, s_q = 65536, deg_q = 0, t = shift << 16.
 * MYDET_E_BADARG: as mydet_motion_frames_rgb_u8, and reserved[0] not MYDET_MOTION_MODEL_SIMILARITY, a setting out of range, a null
 *   or misaligned out_warp, a misaligned out_inliers. */
#define MYDET_MOTION_MODEL_SHIFT       0
#define MYDET_MOTION_MODEL_SIMILARITY  1
int mydet_motion_warp_frames_rgb_u8(const unsigned char *src, int B, int H, int W, int64_t src_img_bytes, int64_t src_row_bytes, int S,
                                    const mydet_motion_set *set, int32_t *state, void *ws, int64_t ws_bytes, int32_t *out_shift,
                                    int32_t *out_warp, int32_t *out_blocks, int32_t *out_inliers, void *stream);
int mydet_motion_warp_frames_yuv420(const struct mydet_yuv420_src *src, int B, int H, int W, int S, const mydet_motion_set *set,
                                    int32_t *state, void *ws, int64_t ws_bytes, int32_t *out_shift, int32_t *out_warp, int32_t *out_blocks,
                                    int32_t *out_inliers, void *stream);

/* The tracker with camera motion: mydet_track_frames_assoc_f32 with one more argument, `shift` (DEVICE, int32 [S*F][4] = (dx, dy,
 * valid, n_valid): out_shift of the estimator above for the same S and F; 4-byte aligned).  mydet_track_frames_assoc_f32 and
 * mydet_track_frames_f32 are this entry point with shift = NULL and give the bits they always gave.
 * Rule: in a frame whose valid == 1, every live track takes x[0] = x[0] + (float)dx, x[1] = x[1] + (float)dy inside `predict`,
 * after x += v and before the frame's predicted box is taken: the association sees the moved prediction, a coasting track's
 * output moves with the camera, and the leave-the-frame rule of `retire` sees the moved box.  Velocities and covariances are
 * untouched; a bad-class frame leaves the state alone whatever its shift. */
int mydet_track_frames_motion_f32(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S, int F,
                                  int box_width, const mydet_track_params *params, int max_tracks, int32_t *state,
                                  float *out_box, float *out_score, int64_t *out_class, int64_t *out_id, int32_t *out_missed,
                                  int32_t *out_count, int32_t *out_dropped, const mydet_track_assoc *assoc, const int32_t *shift,
                                  void *stream);

/* The tracker with the similarity model: mydet_track_frames_motion_f32 with `warp` (DEVICE, int32 [S*F][8] = (a, b, tx, ty, s_q,
 * deg_q, valid, n_inliers): out_warp of mydet_motion_warp_frames_rgb_u8 for the same S and F; 4-byte aligned) in the place of shift.
 * Rule, float32 in this order (-ffp-contract=off), in a frame whose valid == 1, for every live track inside `predict`, after
 * x += v and where the shift applies:
 *   fa = (float)a * 2^-16, fb, ftx, fty alike (exact below 2^24);  ux = x[0] - img_w * 0.5f,  uy = x[1] - img_h * 0.5f
 *   x[0] = x[0] + ftx;  x[1] = x[1] + fty
 *   unless a == 0 and b == 0:   x[0] = x[0] + (fa * ux - fb * uy);  x[1] = x[1] + (fb * ux + fa * uy);
 *                               v[0] = v0 + (fa * v0 - fb * v1);    v[1] = v1 + (fb * v0 + fa * v1)     (v0, v1 the old v[0], v[1])
 *   unless s_q == 65536:        fs = (float)s_q * 2^-16;  x[2], x[3], v[2], v[3] each times fs
 *   box_width 5, unless deg_q == 0:   x[4] = x[4] + (float)deg_q * 2^-16, before the reduction to [0, 180)
 * A positive b turns the x axis towards y, the direction in which a record's angle counts.  Covariances are untouched (a
 * stated simplification).  The identity parts are skipped, so a row that is a pure whole-pixel shift (a = b = 0, s_q = 65536,
 * deg_q = 0, t a multiple of 65536) gives the bits of mydet_track_frames_motion_f32 with that shift; warp = NULL gives the bits
 * of mydet_track_frames_assoc_f32.  An invalid row and a bad-class frame leave the prediction, or the state, alone.
 * mydet_track_frames_appear_warp_f32 and mydet_track_frames_appear_optimal_warp_f32 (declared with their shift siblings' argument
 * lists, warp in the place of shift) are the same for the appearance entry points. */
int mydet_track_frames_warp_f32(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S, int F,
                                int box_width, const mydet_track_params *params, int max_tracks, int32_t *state,
                                float *out_box, float *out_score, int64_t *out_class, int64_t *out_id, int32_t *out_missed,
                                int32_t *out_count, int32_t *out_dropped, const mydet_track_assoc *assoc, const int32_t *warp,
                                void *stream);

/* Winograd F(4x4,3x3) form of the same 3x3 stride-1 pad-1 conv + BN + act (+ residual) as mydet_conv2d_wino_f32
 * (4x fewer multiplies than the direct form; used for the deep layers with chip-filling grids).  `u` = the
 * transform-domain weights made by mydet_wino4_weights_f32 from the OHWI weight (mydet_wino4_weights_floats(Cout, Cin)
 * floats; Cin % 4 == 0).  `ws` = device scratch of at least mydet_wino4_workspace_bytes(B, H, W, Cin, Cout) bytes
 * (36 floats per 4x4-output tile and input channel: the transform-domain input, written by a first launch and
 * streamed by the second, plus 64 MiB for the partial tiles of the K-cut tail: when the workgroup count is whole rounds
 * of the chip plus a small remainder, the remainder runs as K pieces that a fourth launch sums in K order -- deterministic);
 * stream-ordered, so one buffer serves every layer of a stream.
 * MYDET_E_UNSUPP (-2) for shapes it does not cover: the caller then uses mydet_conv2d_wino_f32 / _igemm_f32.
 * Size limit: as mydet_conv2d_wino_f32 with 32 tiles of 4x4 outputs per workgroup -- H*W*max(ldx, ldy, ldr)*4 * (32 / (tiles per
 * image) + 2) below 2^31 - 16 bytes; tensors and the workspace (about 2.25 x the input) may pass 4 GiB.
 * Replaces the same reference code as mydet_conv2d_igemm_f32 (models/modules.py:69-73,94-95). */
int64_t mydet_wino4_weights_floats(int Cout, int Cin);
int mydet_wino4_weights_f32(const float *w, int Cout, int Cin, float *u, void *stream);
int64_t mydet_wino4_workspace_bytes(int B, int H, int W, int Cin, int Cout);
/* Re-reads the MYDET_W4_TAIL* tuning variables (they are read once per process otherwise): tests and in-process sweeps. */
int mydet_wino4_reload_tuning(void);
int mydet_conv2d_wino4_f32(const float *x, int64_t ldx, const float *u, const float *scale, const float *shift,
                           const float *residual, int64_t ldr, float *ws, int64_t ws_bytes, float *y, int64_t ldy,
                           int B, int H, int W, int Cin, int Cout, int act, void *stream);
/* Test hook (host only, no GPU call): the K-cut tail plan mydet_conv2d_wino4_f32 uses on a chip that holds `slots` of its
 * workgroups (2 per CU).  Items are ids of 64-id blocks; out[0] = ids covered by the main launch, out[1] = groups, then per
 * group {first id, blocks, ids taken per block, cuts along K, scratch offset in KiB} (out: 17 ints).  Returns the number of
 * groups (0 = no tail) or a negative MYDET_E_*.  No reference counterpart. */
int mydet_wino4_tail_plan(int B, int H, int W, int Cin, int Cout, int slots, int32_t *out);

/* Bilinear resize of one 8-bit RGB image [H][W][3] -> [oh][ow][3] (rows src_row_bytes / dst_row_bytes apart, so the
 * result can land inside a padded batch buffer), bit-exact with PIL.Image.resize(size, BILINEAR), i.e. with the
 * reference's tvf.resize of a PIL image (utils/image_ops.py:22-35, :55-137; api/detection.py:177-205): Pillow's
 * two-pass 8-bit fixed-point filter.  bounds_* int32 [o][2] = (first tap, tap count), k* int32 [o][ks] = 22-bit
 * integer weights, both DEVICE arrays built by Pillow's rule (mydetection_amd/utils/image_ops.py:resample_tables);
 * NULL tables skip that pass (the size must then be unchanged). */
int mydet_resize_bilinear_u8(const unsigned char *src, int H, int W, int64_t src_row_bytes, unsigned char *dst, int oh,
                             int ow, int64_t dst_row_bytes, const int32_t *bounds_x, const int32_t *kx, int ksx,
                             const int32_t *bounds_y, const int32_t *ky, int ksy, void *stream);

/* Batched forms over per-image groups of K detection slots (e.g. the records of mydet_postprocess_records_f32):
 * bbox of image b at bbox + b*bbox_stride (floats), `count[b*count_stride]` slots valid.
 *   to_original: utils/structures.py:175-189 with one pad_info row (ori w, ori h, tl x, tl y, imw, imh) per image,
 *                pad_info DEVICE float [B][6] -- the per-image call of api/detection.py:173-174 for a whole batch.
 *   to_json:     the arithmetic of ImageObjects.to_json (utils/structures.py:243-256), which runs in Python floats:
 *                out[b][k] = { (double)cx - (double)w/2, (double)cy - (double)h/2, (double)w, (double)h, (double)score },
 *                out_cat[b][k] = cat_table[class] (class itself when cat_table is NULL; -1 outside the table);
 *                rows >= count are zero; count may be NULL (all K rows valid, e.g. B = 1 for one ImageObjects). */
int mydet_bboxes_to_original_batched_f32(float *bbox, int64_t bbox_stride, const int32_t *count, int64_t count_stride,
                                         int B, int K, const float *pad_info, void *stream);
int mydet_detections_to_json_f64(const float *bbox, int64_t bbox_stride, const float *score, int64_t score_stride,
                                 const int64_t *cls, int64_t cls_stride, const int32_t *count, int64_t count_stride,
                                 int B, int K, const int64_t *cat_table, int n_cat, double *out, int64_t *out_cat,
                                 void *stream);

/* Fused front half of an MBConv block (external/efficientnet/model.py:71-79): expand 1x1 + BN0 + swish -> depthwise
 * k x k stride s ("static SAME" pad of the EXPANDED map, utils.py:122-145) + BN1 + swish, plus the SE squeeze sums.
 * Replaces mydet_conv2d_igemm_f32 (expand) + mydet_dwconv_f32 for the shallow blocks; the 6x-wide expanded tensor
 * never reaches HBM.  x logical [B,Cin,H,W] (pixel stride ldx); w_expand [Cexp][Cin] and w_dw [K][K][Cexp] with the
 * per-channel BatchNorm scale already multiplied in; shift0 / shift1 = the folded BatchNorm shifts (they initialise
 * the accumulators); y logical [B,Cexp,Ho,Wo].  se_partial (optional): [B][S+1][Cexp] per-tile channel
 * sums of y with S == mydet_mbconv_tiles(Ho, Wo, stride) (slice S is scratch for mydet_se_gate_f32).
 * Instantiated for (K, stride, Cin) in {(3,2,16), (3,1,24), (5,2,24), (5,1,40), (3,2,40)}: MYDET_E_UNSUPP otherwise. */
int mydet_mbconv_tiles(int Ho, int Wo, int stride);
int mydet_mbconv_expand_dw_f32(const float *x, int64_t ldx, const float *w_expand, const float *shift0,
                               const float *w_dw, const float *shift1,
                               float *y, int64_t ldy, int B, int H, int W, int Cin, int Cexp, int K, int stride,
                               int pad_t, int pad_l, int Ho, int Wo, float *se_partial, int S, const mydet_se_tail *se,
                               void *stream);

/* EfficientNet stem fused with the depthwise conv of the first MBConv block (which has expand_ratio 1):
 *     y = swish(BN1(depthwise3x3_s1_pad1( swish(BN0(conv3x3_s2(image))) )))      + per-tile channel sums of y
 * Replaces _conv_stem -> _bn0 -> swish (external/efficientnet/model.py:133-140) and _depthwise_conv -> _bn1 -> swish +
 * the adaptive_avg_pool2d of block 0 (:76-80); the 32-channel stem output never reaches memory.
 * x: the image, logical [B,3,H,W], strides sxb/sxc/sxh/sxw in floats (as mydet_conv2d_stem_f32).  w_stem: OHWI [32][3][3][3]
 * with BN0's scale folded in, shift0 [32]; w_dw [3][3][32] with BN1's scale folded in, shift1 [32].  pad_t / pad_l: the
 * stem's "SAME" padding (top / left; bottom / right follow from Hs, Ws).  y [B,Hs,Ws,ldy].  se_partial (optional):
 * [B][S+1][32] with S == mydet_mbconv_tiles(Hs, Ws, 1).  C must be 32 (MYDET_E_UNSUPP otherwise). */
int mydet_stem_dw_f32(const float *x, int64_t sxb, int64_t sxc, int64_t sxh, int64_t sxw, const float *w_stem,
                      const float *shift0, const float *w_dw, const float *shift1, float *y, int64_t ldy, int B, int H, int W,
                      int C, int pad_t, int pad_l, int Hs, int Ws, float *se_partial, int S, const mydet_se_tail *se,
                      void *stream);

/* Fused separable-conv node of the 88-channel BiFPN / EfDetHead pyramid, several nodes per launch:
 *     y = act( pointwise1x1( depthwise3x3_pad1( pre(in...) ) ) * scale + shift )
 *   n_in == 1: pre = identity                 spconv3x3_bn_swish / last sepconv of a head tower, models/rpns.py:121-205
 *   n_in >= 2: pre = swish(sum_i w_i * in_i), w = relu(fuse_weights) / (sum + 1e-4)     LinearFusion, models/fpns.py:421-439;
 *              mode[i]: 0 same size, 1 half-size map read through nearest 2x, 2 double-size map read through
 *              max_pool2d(3,2,1) (the top-down / bottom-up paths of BiFPN5.forward, models/fpns.py:398-418)
 * Replaces mydet_bifpn_fuse_f32 + mydet_dwconv_f32 + mydet_conv2d_igemm_f32 for these nodes (SeparableConv2d,
 * models/modules.py:5-21, with the following BatchNorm folded into scale/shift).
 * in[i]: logical [B,C,h,w] channels-last, pixel stride ld[i].  w_dw [3][3][C].  w_pw_packed: the pointwise weight
 * W[Cout][C] in MFMA operand order with four k-steps of a lane side by side, ceil(Cout/16) x ceil(C/16) x 64 x 4 floats:
 *     packed[nb][kq][lane][e] = W[16*nb + (lane & 15)][4*(4*kq + e) + (lane >> 4)]   (rows >= Cout and k >= C are zero):
 *     a workgroup copies a block to LDS with 16-byte loads and every wave reads its operands from there.
 * scale may be NULL (no BatchNorm: y = conv + shift).  Cout % 4 == 0.  act: MYDET_ACT_NONE | MYDET_ACT_SWISH.
 * `nodes` is a HOST array of n (<= MYDET_SEPCONV_MAX_NODES) descriptors; all nodes share B and C (C == 88). */
#define MYDET_SEPCONV_MAX_NODES 10
typedef struct {
    const float *in[3];
    int64_t ld[3];
    int mode[3];
    int n_in;
    const float *fuse_weights;
    const float *w_dw;
    const float *w_pw_packed;
    const float *scale;
    const float *shift;
    float *y;
    int64_t ldy;
    int H, W, Cout, act;
} mydet_sepconv_node;
int mydet_sepconv_nodes_f32(int n, const mydet_sepconv_node *nodes, int B, int C, void *stream);

/* The LAST layers of the EfDetHead towers with RetinaLayer's decode in their epilogue: replaces the last
 * SeparableConv2d of class_nets / bbox_nets (models/rpns.py:121-197) + RetinaLayer.forward
 * (models/detlayers/retinanet.py:63-82) + the level concatenation of models/general.py:74-76, i.e.
 * mydet_sepconv_nodes_f32 + mydet_decode_levels_f32(MYDET_DECODE_RETINA) without the A*n_cls class logits per pixel ever
 * reaching memory.  Same results as that pair (same arithmetic, candidate order (a, y, x), first maximum on ties).
 *   kind 0 (class tower): node.Cout = A * cpad, cpad = 16 * ceil(n_cls / 16): w_pw_packed / shift hold anchor a's n_cls
 *           rows at [a * cpad, a * cpad + n_cls), zero rows after them; writes score (sigmoid of the anchor's largest
 *           logit) and class_idx.  n_cls in 65..96.
 *   kind 1 (box tower):   node.Cout = 4 * A (tx, ty, tw, th per anchor); anchors_wh = HOST pointer to A (w, h) pairs in
 *           pixels; writes bbox (cx, cy, w, h clamped to [1, max(img_h, img_w)]).
 * node.y / node.ldy are ignored, node.n_in == 1, node.act == MYDET_ACT_NONE.  n_off = first candidate of the node's
 * level inside [0, N).  bbox [B,N,4] f32, class_idx [B,N] i64, score [B,N] f32.  C == 88, A <= 12. */
typedef struct {
    mydet_sepconv_node node;
    int kind;
    float stride;
    const float *anchors_wh;
    int64_t n_off;
} mydet_sepconv_decode_node;
int mydet_sepconv_decode_retina_f32(int n, const mydet_sepconv_decode_node *nodes, int B, int C, int A, int n_cls,
                                    int img_h, int img_w, float *bbox, int64_t *class_idx, float *score, int64_t N,
                                    void *stream);

/* The lr_tb box layer of the EfficientDet + custom FCOS head (_LR_TB_last, models/rpns.py:208-229), every pyramid level
 * of a batch in one launch:
 *     dlr = depthwise3x3_pad1(x; W_lr0)   lr = conv(dlr; W_lr1 [2,C,1,3], pad (0,1)) + b_lr1
 *     dtb = depthwise3x3_pad1(x; W_tb0)   tb = conv(dtb; W_tb1 [2,C,3,1], pad (1,0)) + b_tb1
 *     y = (lr[0], tb[0], lr[1], tb[1]) per pixel
 * (the second conv pads the depthwise OUTPUT with zeros).  x: logical [B,C,H,W] channels-last with pixel stride ldx >= C
 * (4-byte aligned; 16-byte aligned with ldx % 4 == 0 takes vector loads).  y: [B,H,W,ldy], ldy % 4 == 0, 16-byte aligned:
 * one 16-byte store of (l, t, r, b) per pixel.  w: the level's weights packed as (30 C + 4) floats, 16-byte aligned:
 *     [0, 9C)    W_lr0 as [kh][kw][C]       [9C, 18C)  W_tb0 as [kh][kw][C]
 *     [18C, 24C) W_lr1 as [o][kw][C]        [24C, 30C) W_tb1 as [o][kh][C]
 *     [30C, 30C + 4) (b_lr1[0], b_tb1[0], b_lr1[1], b_tb1[1])
 * `levels` is a HOST array of n (<= MYDET_LR_TB_MAX_LEVELS) descriptors sharing B and C; C % 4 == 0, C <= MYDET_LR_TB_MAX_C.
 * Anything else returns MYDET_E_BADARG before any launch. */
#define MYDET_LR_TB_MAX_LEVELS 8
#define MYDET_LR_TB_MAX_C      128
typedef struct {
    const float *x;
    int64_t ldx;
    const float *w;
    float *y;
    int64_t ldy;
    int H, W;
} mydet_lr_tb_level;
int mydet_lr_tb_levels_f32(int n, const mydet_lr_tb_level *levels, int B, int C, void *stream);

/* Pairwise IoU [Na,Nb]; utils/bbox_ops.py:6-49 (xyxy != 0: corner format, else cxcywh). */
int mydet_bboxes_iou_f32(const float *a, int Na, const float *b, int Nb, int xyxy,
                         float *iou, void *stream);

/* Centre format -> corner format, utils/bbox_ops.py:309-316: n rows of `width` >= 4 floats; columns 0..3 of a row
 * become (cx - w/2, cy - h/2, cx + w/2, cy + h/2) with the reference's float32 operation order (bit-exact), columns
 * 4.. are copied.  Out of place (in == out is allowed: a thread reads its row before it writes it). */
int mydet_cxcywh_to_x1y1x2y2_f32(const float *cxcywh, float *x1y1x2y2, int64_t n, int width, void *stream);

/* In-place undo of resize/pad on cxcywh boxes; utils/structures.py:175-189. */
int mydet_bboxes_to_original_f32(float *bbox, int64_t n, float ori_w, float ori_h,
                                 float tl_x, float tl_y, float imw, float imh, void *stream);

/* Device-side image preparation (first stage before the path): uint8 [B,H,W,3] images ->
 * float32 [B,3,Hp,Wp]: zero-pad right/bottom (utils/image_ops.py:38-52), /255 (tvf.to_tensor,
 * api/detection.py:160), and, when norm != 0, (x - mean)/std per channel (utils/image_ops.py:177-180).
 * mean3/std3 are HOST pointers to 3 floats. */
int mydet_preprocess_u8_f32(const unsigned char *img, int B, int H, int W, float *out, int Hp, int Wp, int norm,
                            const float *mean3, const float *std3, void *stream);

/* Video frames -> network input in ONE launch: B uint8 frames [H][W][3] of one size (frame b at src + b*src_img_bytes,
 * rows src_row_bytes apart, so a crop of a larger buffer is read in place) -> float32 [B,3,Hp,Wp].  Inside the oh x ow
 * window at (top, left) the output is the Pillow-exact bilinear resize of the frame (mydet_resize_bilinear_u8: same
 * DEVICE tables, NULL tables = that axis keeps its size) put through the arithmetic of mydet_preprocess_u8_f32;
 * outside it, what that function gives for a zero pixel.  Bit-identical to the two calls it fuses; the uint8 image
 * between them exists only in LDS.  ksx / ksy above MYDET_FRAMES_MAX_TAPS (a downscale beyond 8x), a window that does
 * not fit Hp x Wp, and null or non-positive arguments are MYDET_E_BADARG.  mean3/std3 are HOST pointers to 3 floats. */
#define MYDET_FRAMES_MAX_TAPS 17
int mydet_frames_to_input_f32(const unsigned char *src, int B, int H, int W, int64_t src_img_bytes, int64_t src_row_bytes,
                              float *out, int Hp, int Wp, int oh, int ow, int top, int left,
                              const int32_t *bounds_x, const int32_t *kx, int ksx,
                              const int32_t *bounds_y, const int32_t *ky, int ksy,
                              int norm, const float *mean3, const float *std3, void *stream);

/* Mirrored views (test-time augmentation): mydet_frames_to_input_f32 with `flip`, a set of MYDET_VIEW_* bits.  The output is,
 * bit for bit, what mydet_frames_to_input_f32 writes for a source whose pixel (y, x) is pixel (H-1-y if VFLIP else y,
 * W-1-x if HFLIP else x) of `src`.  The frames are read in place through their strides -- the mirror is applied where a tap
 * is addressed, and no mirrored copy exists; the tables are those of the unmirrored geometry (the two have one size).
 * flip == 0 launches the kernel instance mydet_frames_to_input_f32 launches.  Any other bit is MYDET_E_BADARG; every other
 * argument rule is that of mydet_frames_to_input_f32.  Symbols added under ABI version 2. */
#define MYDET_VIEW_HFLIP 1
#define MYDET_VIEW_VFLIP 2
int mydet_frames_to_input_flip_f32(const unsigned char *src, int B, int H, int W, int64_t src_img_bytes, int64_t src_row_bytes,
                                   float *out, int Hp, int Wp, int oh, int ow, int top, int left,
                                   const int32_t *bounds_x, const int32_t *kx, int ksx,
                                   const int32_t *bounds_y, const int32_t *ky, int ksy,
                                   int norm, const float *mean3, const float *std3, int flip, void *stream);

/* NV12 video frames (what hardware decoders produce): per frame a Y plane [H][W] and an interleaved chroma plane of
 * ceil(H/2) rows of ceil(W/2) (U, V) byte pairs; odd H and W are legal.  Frame b of a plane is at ptr + b*img_bytes, its
 * rows row_bytes apart (y_row_bytes >= W, uv_row_bytes >= 2*ceil(W/2); the planes may be separate allocations or the two
 * parts of one decoder surface).  Conversion, 8-bit fixed point on signed 32-bit integers, >> an arithmetic shift,
 * clip8 a clamp to 0..255, chroma nearest-neighbour (pixel (y, x) uses the pair (y >> 1, x >> 1)):
 *     C = Y - 16 (limited range) or Y (full range),  D = U - 128,  E = V - 128
 *     R = clip8((cy*C         + crv*E + 128) >> 8)
 *     G = clip8((cy*C - cgu*D - cgv*E + 128) >> 8)
 *     B = clip8((cy*C + cbu*D         + 128) >> 8)
 * with round(256 * x) of the matrix (Kr, Kb = 0.299, 0.114 for BT.601, 0.2126, 0.0722 for BT.709; limited range scales
 * luma by 255/219 and chroma by 255/224):
 *     matrix, full_range     cy  crv  cgu  cgv  cbu
 *     0 (BT.601), 0         298  409  100  208  516
 *     1 (BT.709), 0         298  459   55  136  541
 *     0 (BT.601), 1         256  359   88  183  454
 *     1 (BT.709), 1         256  403   48  120  475
 * Another selector value, a pitch below the row's bytes, a negative frame stride and null or non-positive arguments are
 * MYDET_E_BADARG.  No reference counterpart.
 *
 * mydet_nv12_to_rgb_u8: the conversion alone, to packed uint8 RGB [B][H][W][3] (frame b at dst + b*dst_img_bytes, rows
 * dst_row_bytes >= 3*W apart). */
int mydet_nv12_to_rgb_u8(const unsigned char *y, int64_t y_img_bytes, int64_t y_row_bytes,
                         const unsigned char *uv, int64_t uv_img_bytes, int64_t uv_row_bytes, int B, int H, int W,
                         unsigned char *dst, int64_t dst_img_bytes, int64_t dst_row_bytes,
                         int matrix, int full_range, void *stream);

/* mydet_nv12_to_input_f32: NV12 frames -> float32 [B,3,Hp,Wp] in ONE launch: exactly what mydet_frames_to_input_f32 writes
 * for the RGB frames mydet_nv12_to_rgb_u8 gives, bit for bit, with no RGB image in memory (the converted source window of
 * a tile lives in LDS).  Geometry, tables, norm, mean3/std3 and their checks as for mydet_frames_to_input_f32, including
 * MYDET_FRAMES_MAX_TAPS. */
int mydet_nv12_to_input_f32(const unsigned char *y, int64_t y_img_bytes, int64_t y_row_bytes,
                            const unsigned char *uv, int64_t uv_img_bytes, int64_t uv_row_bytes, int B, int H, int W,
                            int matrix, int full_range,
                            float *out, int Hp, int Wp, int oh, int ow, int top, int left,
                            const int32_t *bounds_x, const int32_t *kx, int ksx,
                            const int32_t *bounds_y, const int32_t *ky, int ksy,
                            int norm, const float *mean3, const float *std3, void *stream);

/* The 4:2:0 family: one source descriptor for every layout a decoder gives.  Per frame a Y plane of H rows of W samples and
 * chroma at half resolution, ceil(H/2) rows for ceil(W/2) pixel pairs; odd H and W are legal for every layout.
 *     layout            bytes/sample  chroma                                        sample -> 8 bit
 *     MYDET_YUV420_NV12      1        plane[1]: (U, V) pairs, plane[2] NULL         as is
 *     MYDET_YUV420_NV21      1        plane[1]: (V, U) pairs, plane[2] NULL         as is
 *     MYDET_YUV420_I420      1        plane[1]: U, plane[2]: V, ceil(W/2) samples   as is
 *     MYDET_YUV420_P010      2, LE    plane[1]: (U, V) pairs, plane[2] NULL         v10 = word >> 6   (low six bits ignored)
 *     MYDET_YUV420_I010      2, LE    plane[1]: U, plane[2]: V                      v10 = word & 1023 (high six bits ignored)
 * YV12 is I420 with plane[1] and plane[2] exchanged by the caller.  A 10-bit sample becomes 8 bits by
 *     s8 = min(255, (v10 + 2) >> 2)                       for Y, U and V alike
 * (limited-range 64 / 512 / 940 become 16 / 128 / 235; the clamp is reached from v10 >= 1022).  From there the conversion
 * is the NV12 one above, unchanged: the same formula, the same four (matrix, full_range) rows of the one table, chroma
 * nearest-neighbour at (y >> 1, x >> 1).  So every layout gives the bits NV12 gives for the same 8-bit samples.
 *
 * Frame b of plane i is at plane[i] + b*img_bytes[i], its rows row_bytes[i] apart.  MYDET_E_BADARG, with nothing
 * launched: an unknown layout, matrix or range; a null src or plane[0] or plane[1]; plane[2] non-null for a semi-planar
 * layout or null for a planar one; a pitch below the row's bytes (Y: W*bps; interleaved chroma: 2*ceil(W/2)*bps; a planar
 * chroma plane: ceil(W/2)*bps); a negative frame stride; non-positive sizes; for the two 16-bit layouts any odd address,
 * pitch or frame stride.  `reserved` is ignored.  The kernels read a plane with wide loads when its address, pitch and
 * frame stride are multiples of: NV12 / NV21 4; I420 4 (Y), 2 (U, V); P010 8; I010 8 (Y), 4 (U, V) -- and sample by sample
 * otherwise, with the same result.  No reference counterpart. */
#define MYDET_YUV420_NV12 0
#define MYDET_YUV420_NV21 1
#define MYDET_YUV420_I420 2
#define MYDET_YUV420_P010 3
#define MYDET_YUV420_I010 4
typedef struct mydet_yuv420_src {
    const void *plane[3];            /* Y; interleaved chroma or U; V or NULL */
    int64_t img_bytes[3], row_bytes[3];
    int layout, matrix, full_range, reserved;
} mydet_yuv420_src;

/* mydet_yuv420_to_rgb_u8: mydet_nv12_to_rgb_u8 for any layout (dst as there). */
int mydet_yuv420_to_rgb_u8(const mydet_yuv420_src *src, int B, int H, int W,
                           unsigned char *dst, int64_t dst_img_bytes, int64_t dst_row_bytes, void *stream);

/* mydet_yuv420_to_input_f32: mydet_nv12_to_input_f32 for any layout, in ONE launch: the bits mydet_frames_to_input_f32
 * writes for the RGB frames mydet_yuv420_to_rgb_u8 gives.  Geometry, tables, norm, mean3/std3, their checks and
 * MYDET_FRAMES_MAX_TAPS as there.  The two mydet_nv12_* entry points are this pair with layout MYDET_YUV420_NV12. */
int mydet_yuv420_to_input_f32(const mydet_yuv420_src *src, int B, int H, int W,
                              float *out, int Hp, int Wp, int oh, int ow, int top, int left,
                              const int32_t *bounds_x, const int32_t *kx, int ksx,
                              const int32_t *bounds_y, const int32_t *ky, int ksy,
                              int norm, const float *mean3, const float *std3, void *stream);

/* mydet_yuv420_to_input_flip_f32: the mirrored views of mydet_frames_to_input_flip_f32 for every 4:2:0 layout.  The mirrored
 * source is the mirrored RGB image of mydet_yuv420_to_rgb_u8: luma AND chroma are fetched for the pixel's position in the
 * planes as they are (pixel (y, x) of the planes uses the pair (y >> 1, x >> 1)), so odd W and H stay legal and no
 * "mirrored plane" is defined -- for odd sizes the result is NOT what the unmirrored call gives on planes mirrored by the
 * caller, whose chroma pairing differs.  flip == 0 launches the instance mydet_yuv420_to_input_f32 launches; another bit
 * than MYDET_VIEW_HFLIP | MYDET_VIEW_VFLIP is MYDET_E_BADARG. */
int mydet_yuv420_to_input_flip_f32(const mydet_yuv420_src *src, int B, int H, int W,
                                   float *out, int Hp, int Wp, int oh, int ow, int top, int left,
                                   const int32_t *bounds_x, const int32_t *kx, int ksx,
                                   const int32_t *bounds_y, const int32_t *ky, int ksy,
                                   int norm, const float *mean3, const float *std3, int flip, void *stream);

/* Overlay renderer: outlines of axis-aligned and rotated boxes, optional translucent fills and text labels, painted IN PLACE
 * into uint8 RGB frames or into the planes of the 8-bit 4:2:0 layouts, one launch per batch (csrc/draw.hip).  It stands where
 * the reference's utils/visualization.py:draw_bboxes_on_np and ImageObjects.draw_on_np (utils/structures.py) stand, with their
 * intent and call shape -- not cv2's pixels: the raster rules are this library's own, and they are these.
 *
 * Geometry.  The centre of pixel (row i, column j) is (j + 0.5, i + 0.5).  A row of the list is (cx, cy, w, h) in frame pixels
 *   and an angle in degrees (0 without an angle plane).  With c = cos(angle), s = sin(angle), dx = j + 0.5 - cx, dy = i + 0.5 - cy:
 *       a = |dx*c + dy*s|,   b = |-dx*s + dy*c|
 *   (the reference's vertex convention, pts @ [[c, s], [-s, c]]: clockwise on screen).  angle == 0 uses c = 1, s = 0 exactly, with
 *   no trigonometric call; otherwise c, s = cosf, sinf of fmodf(angle, 360) * (pi / 180) in float32.  All arithmetic is float32
 *   and uncontracted.
 * Outline of thickness t (1..MYDET_DRAW_MAX_THICKNESS): painted iff a <= w/2 + t/2 and b <= h/2 + t/2 and not
 *   (a < w/2 - t/2 and b < h/2 - t/2): centred on the rectangle's edge, mitred corners; a box thinner than t is solid.  Opaque.
 * Fill (fill_alpha 1..255; 0 = none): every pixel with a <= w/2 and b <= h/2 becomes, per channel and in integers,
 *   (colour * alpha + old * (255 - alpha) + 127) / 255.
 * Label (label_flags; parts in the order class, score, id, one space between two parts; a part whose plane is NULL, or an empty name, is left out):
 *   class  names[cls] (ASCII, up to MYDET_DRAW_NAME_BYTES characters, NUL-terminated when shorter) when a names table is given
 *          and 0 <= cls < n_names, else the decimal class index ('-' first when negative), cut to MYDET_DRAW_NAME_BYTES characters
 *   score  d.dd of n = min(100, floor(score * 100 + 0.5)) in float32; NaN or a score <= 0 gives 0.00
 *   id     '#', then the decimal of id mod 10^10 (non-negative)
 *   -- at most MYDET_DRAW_MAX_GLYPHS glyphs, from a monospace cell atlas [96][ch][cw] of 0 / 1 bytes for ASCII 32..127 (another
 *   byte shows '?').  The rectangle is ch rows x n*cw columns; left column clamp(floor(cx - w/2 - t/2), 0, max(0, W - n*cw)), top
 *   row clamp(floor(cy - h/2 - t/2) - ch, 0, max(0, H - ch)); clipped to the frame.  Background: the box colour, opaque; text:
 *   white when 299 R + 587 G + 114 B < 150000, black otherwise.
 * Order.  Per frame rows count - 1 down to 0, for each row fill, outline, label: row 0 (a record's highest score) ends up on top.
 * Skipped: a row with a non-finite cx, cy, w, h or angle, or with w <= 0 or h <= 0; a frame with count <= 0 (that includes
 *   MYDET_COUNT_BAD_CLASS).  A count above K means K; a NULL count means K for every frame.  Everything is clipped to the frame:
 *   a box of any size or position is legal and nothing outside the H x W view is written (or read).
 * Colour, per row: palette[key mod n_palette] (non-negative mod) with key the class (MYDET_DRAW_COLOR_CLASS) or the id
 *   (MYDET_DRAW_COLOR_ID; 0 when that plane is NULL), or the fixed `color` (MYDET_DRAW_COLOR_FIXED).
 * 4:2:0 targets (NV12, NV21, I420; YV12 = I420 with the planes exchanged by the caller; odd H and W legal).  Luma is painted
 *   per pixel with Y of the colour.  A chroma sample covers its quad of luma pixels (2 x 2, fewer at odd edges) and receives, in
 *   paint order and once each, every operation (fill, outline, label) that hits any pixel of its quad; the operation's colour
 *   is its colour at the first pixel of the quad it hits, in raster order (this matters inside labels only); a fill blends U and
 *   V with the formula above.  RGB -> Y'CbCr is fixed point with 8 fraction bits, `>>` arithmetic, each result clamped to 0..255:
 *       Y = ((yr*R + yg*G + yb*B + 128) >> 8) + (16 limited | 0 full),  U = ((ur*R + ug*G + ub*B + 128) >> 8) + 128,  V likewise
 *     matrix, full_range     yr   yg  yb     ur   ug   ub     vr    vg   vb
 *     0 (BT.601), 0          66  129  25    -38  -74  112    112   -94  -18
 *     0 (BT.601), 1          77  150  29    -43  -85  128    128  -107  -21
 *     1 (BT.709), 0          47  157  16    -26  -86  112    112  -102  -10
 *     1 (BT.709), 1          54  183  18    -29  -99  128    128  -116  -12
 *   (within 1 code value of the float64 matrix rounded to nearest for all 2^24 colours; every grey gives U = V = 128).
 *   MYDET_YUV420_P010 / _I010 targets are not drawn: MYDET_E_BADARG.
 *
 * mydet_draw_list: DEVICE pointers with ELEMENT strides per frame and per row, so the planes of a detection record are read
 *   in place (box = the [B,512,4] plane, four floats of a row adjacent; angle, score, cls and id each their own plane) and a
 *   dense [B,K,5] array by the same struct (angle = box + 4 with the box strides).  angle, score, cls, id and count may be NULL.
 *   K <= MYDET_DRAW_MAX_BOXES rows per frame and launch.
 * mydet_draw_style: palette DEVICE uint8 [n_palette][3]; atlas DEVICE uint8 [96][ch][cw] (needed when label_flags != 0; ch in
 *   8..64, cw in 1..64); names DEVICE uint8 [n_names][MYDET_DRAW_NAME_BYTES] or NULL.
 * Frames of mydet_draw_boxes_rgb_u8 are [H][W][3], frame b at dst + b*dst_img_bytes, rows dst_row_bytes >= 3*W apart (as the
 *   source of mydet_frames_to_input_f32: a crop view is drawn in place).  mydet_draw_boxes_yuv420_u8 takes the plane descriptor
 *   of the input side and WRITES the planes.  Pixel groups are loaded and stored with dword accesses when address, pitch and
 *   frame stride are multiples of: RGB 4; NV12 / NV21 4 (both planes); I420 4 (Y), 2 (U, V: 16-bit accesses) -- and byte by byte
 *   otherwise, and in a row's partial last group, with the same result.  A tile (64 x 16 pixels RGB, 128 x 16 for 4:2:0) that no
 *   box or label reaches (the bounding box of a row's outer rectangle, less -- without a fill -- the tiles inside the outline's
 *   hole, and its label rectangle) is neither read nor written; in the others only pixel groups that some operation hit are stored.
 * MYDET_E_BADARG, with nothing launched: a null list, style, box plane or target; non-positive B, H, W; a pitch below the
 *   row's bytes; a negative stride; K outside 1..MYDET_DRAW_MAX_BOXES; thickness outside 1..MYDET_DRAW_MAX_THICKNESS; fill_alpha
 *   outside 0..255; an unknown colour mode or a palette mode without a palette; unknown label flags; labels without an atlas, ch
 *   outside 8..64 or cw outside 1..64; names with n_names < 1; an unknown layout, matrix or range, a 10-bit layout, plane[2]
 *   not matching the layout. */
#define MYDET_DRAW_MAX_BOXES     512
#define MYDET_DRAW_MAX_THICKNESS 64
#define MYDET_DRAW_MAX_GLYPHS    33
#define MYDET_DRAW_NAME_BYTES    16
#define MYDET_DRAW_COLOR_CLASS   0
#define MYDET_DRAW_COLOR_ID      1
#define MYDET_DRAW_COLOR_FIXED   2
#define MYDET_DRAW_LABEL_CLASS   1
#define MYDET_DRAW_LABEL_SCORE   2
#define MYDET_DRAW_LABEL_ID      4
typedef struct mydet_draw_list {
    const float *box;      int64_t box_frame_stride, box_row_stride;       /* (cx, cy, w, h) adjacent; strides in floats */
    const float *angle;    int64_t angle_frame_stride, angle_row_stride;   /* degrees, or NULL */
    const float *score;    int64_t score_frame_stride, score_row_stride;   /* or NULL */
    const int64_t *cls;    int64_t cls_frame_stride, cls_row_stride;       /* or NULL */
    const int64_t *id;     int64_t id_frame_stride, id_row_stride;         /* or NULL */
    const int32_t *count;  int64_t count_stride;                           /* rows to draw per frame, or NULL = K */
    int K, reserved;
} mydet_draw_list;
typedef struct mydet_draw_style {
    int thickness, fill_alpha, color_mode, label_flags;
    unsigned char color[4];                                                /* R, G, B of MYDET_DRAW_COLOR_FIXED; [3] ignored */
    int n_palette, ch, cw, n_names;
    const unsigned char *palette, *atlas, *names;
} mydet_draw_style;
int mydet_draw_boxes_rgb_u8(unsigned char *dst, int B, int H, int W, int64_t dst_img_bytes, int64_t dst_row_bytes,
                            const mydet_draw_list *list, const mydet_draw_style *style, void *stream);
int mydet_draw_boxes_yuv420_u8(const mydet_yuv420_src *planes, int B, int H, int W, const mydet_draw_list *list,
                               const mydet_draw_style *style, void *stream);

/* Counting overlay: the zones, the directed lines with a tick on their positive side, their running counters and the trails of
 * the tracks, painted IN PLACE into the frames the renderer above draws into, by one launch that runs before it (csrc/overlay.hip),
 * so that boxes and their labels stay on top.  The counters are read from the outputs of mydet_zones_frames on the device and
 * formatted by the kernel.  All geometry is in the zones' fixed point: q(v) as in mydet_zones_frames, |q| <= MYDET_ZONE_COORD_MAX,
 * frames at most MYDET_ZONE_MAX_FRAME on a side; the centre of pixel (row i, column j) is p = (16 j + 8, 16 i + 8).  Every
 * decision is an integer comparison; tests/_overlay_ref.py restates the rules with Python ints and the kernel equals it with ==.
 *
 * Zone fill.  Pixel (i, j) belongs to polygon z iff p is inside by the even-odd, half-open "Inside" rule of mydet_zones_frames,
 *   verbatim (two zones that share an edge paint disjoint pixel sets).  It blends with the renderer's formula (colour * alpha +
 *   old * (255 - alpha) + 127) / 255; alpha = zone_alpha when out_occupancy[o][z] == 0 in this frame, occupied_alpha otherwise
 *   (alpha 0 paints nothing); polygons in order z = 0 .. Z-1; colour palette[z mod n_palette].
 * Stroke (zone outlines, lines, direction ticks, trail segments).  A segment a -> b of thickness t (1..MYDET_DRAW_MAX_THICKNESS)
 *   paints every pixel whose centre lies within t/2 pixels of the segment (a capsule; a == b gives a dot), opaque.  In integers,
 *   with d = b - a, v = p - a, len2 = d.d, u = v.d and r = 8 t:   u <= 0: v.v <= r^2;   else u >= len2: (p-b).(p-b) <= r^2;   else
 *   cross(d, v)^2 <= r^2 * len2.  The components of d are at most 2^21 and those of v below 2^21, so |cross| < 2^43, len2 <= 2^43
 *   and r^2 * len2 <= 2^61 fit int64; cross^2 need not: the kernel first rejects |cross| >= 2^31, which is then certainly outside (r^2 * len2 < 2^62).
 * Direction tick of line A -> B, computed on the host with integers alone when the geometry is built: M = ((A + B) >> 1) per
 *   coordinate, n = (-(B.y - A.y), B.x - A.x) (the positive side of mydet_zones_frames), Lh = floor(sqrt(len2)), the tick goes
 *   from M to M + trunc(n * 16 * tick_px / Lh) per coordinate (truncated toward zero), tick_px = 4 * thickness: one more segment
 *   of the line's colour and thickness.  (Its end may pass MYDET_ZONE_COORD_MAX by 16 * tick_px <= 4096; the bounds above hold.)
 * Counter labels.  Zone z: its name, then for each requested part a space and its text -- MYDET_OVERLAY_COUNT_OCCUPANCY `N`,
 *   _ENTRIES `+E`, _VISITS `-V` (the finished visits: exits + lost) --; line l: `name +pos -neg`.  A number is the decimal of
 *   min(value, 999999) (a negative value, which the counters never are, shows 0); a name shows at most MYDET_DRAW_NAME_BYTES
 *   characters; a label has at most MYDET_OVERLAY_MAX_GLYPHS glyphs.  The label is the renderer's (same atlas; background the
 *   zone's or line's colour palette[z or l mod n_palette]; text colour by the renderer's rule) and is placed by the renderer's rule
 *   at an anchor point (x, y) in fixed point: left column clamp(x >> 4, 0, max(0, W - n*cw)), top row clamp((y >> 4) - ch, 0,
 *   max(0, H - ch)), ch rows x n*cw columns, clipped to the frame.  Zone: the vertex least in (y, x); line: M.  Values are those
 *   of out_occupancy, out_zone_counts and out_line_counts of frame o = s*F + f = the frame's index in the batch.
 * Trails (mydet_trails_frames).  In frame o every slot with out_len >= 2 whose track the call shows -- missed == 0, or with
 *   coasting missed >= 0 -- paints the segments between consecutive points with trail_thickness in palette[id mod n_palette]
 *   (non-negative mod: the renderer's MYDET_DRAW_COLOR_ID colour).
 * Paint order, per pixel: fills z ascending; zone outlines z ascending; lines l ascending, each followed by its tick; trails by
 *   slot ascending; labels of zones, then of lines.  The last opaque operation wins.
 * 4:2:0 targets follow the renderer's chroma rule unchanged: a chroma sample takes, in paint order and once each, every operation
 *   (a fill, a segment, a label) that hits a pixel of its quad, a label with its colour at the first pixel of the quad it hits.
 *   NV12, NV21, I420 (YV12 through exchanged planes); the 10-bit layouts are refused.
 * Skipping.  A tile no operation reaches is neither read nor written; in the others only pixel groups some operation hit are
 *   stored; nothing outside the H x W view is touched.
 *
 * mydet_overlay (HOST struct; it travels as a kernel argument, well below the 4 KB limit, because the static geometry --
 *   polygons, lines, ticks, anchors and names, 3.4 KB -- sits in a DEVICE buffer made once: mydet_overlay_geometry).  The
 *   kernel reads n_polygons and n_lines from the host struct and never more than MYDET_ZONE_MAX_VERTICES vertices.  flags says
 *   what is painted; the pointers a part does not need may be NULL: ZONES reads geometry and occupancy, LINES geometry, either
 *   with counters != 0 zone_counts (ZONES) / line_counts (LINES) and the style's atlas; TRAILS the trail outputs with id and
 *   missed [S*F][max_tracks] of the tracker.  style: palette, n_palette, atlas, ch, cw are read, the rest is ignored.
 * MYDET_E_BADARG, with nothing launched: a null overlay, style, palette or target, or a null pointer a painted part reads;
 *   n_palette < 1; non-positive B, H, W or H, W above MYDET_ZONE_MAX_FRAME; B != S * F; flags 0 or with unknown bits; unknown
 *   counter bits; an alpha outside 0..255; a thickness outside 1..MYDET_DRAW_MAX_THICKNESS; n_polygons or n_lines outside
 *   0..MYDET_ZONES_MAX; counters without an atlas, ch outside 8..64 or cw outside 1..64; max_tracks < 1; max_points outside
 *   2..MYDET_TRAIL_MAX_POINTS; coasting not 0 or 1; the target's rules of mydet_draw_boxes_*.  MYDET_E_UNSUPP: max_tracks >
 *   MYDET_TRACK_MAX_TRACKS, B or ceil(H / 16) above 65535. */
#define MYDET_OVERLAY_MAX_GLYPHS      40
#define MYDET_OVERLAY_ZONES           1
#define MYDET_OVERLAY_LINES           2
#define MYDET_OVERLAY_TRAILS          4
#define MYDET_OVERLAY_COUNT_OCCUPANCY 1
#define MYDET_OVERLAY_COUNT_ENTRIES   2
#define MYDET_OVERLAY_COUNT_VISITS    4
typedef struct mydet_overlay_geometry {
    int n_vertices[MYDET_ZONES_MAX];
    int polygon[MYDET_ZONES_MAX][MYDET_ZONE_MAX_VERTICES][2];      /* quantised (x, y), as in mydet_zone_set */
    int line[MYDET_ZONES_MAX][4];                                  /* A.x, A.y, B.x, B.y */
    int tick[MYDET_ZONES_MAX][4];                                  /* M.x, M.y, the tick's end */
    int anchor[2 * MYDET_ZONES_MAX][2];                            /* label anchors: zone z at z, line l at MYDET_ZONES_MAX + l */
    unsigned char name[2 * MYDET_ZONES_MAX][MYDET_DRAW_NAME_BYTES]; /* ASCII, NUL-terminated when shorter; same order */
} mydet_overlay_geometry;
typedef struct mydet_overlay {
    const mydet_overlay_geometry *geometry;                        /* DEVICE */
    int flags, counters;                                           /* MYDET_OVERLAY_*, MYDET_OVERLAY_COUNT_* */
    int n_polygons, n_lines;
    int zone_alpha, occupied_alpha, thickness, trail_thickness;
    int S, F, max_tracks, max_points;
    int coasting, reserved;
    const int32_t *occupancy, *zone_counts, *line_counts;          /* DEVICE: outputs of mydet_zones_frames of the same S, F */
    const int32_t *trail_points, *trail_len, *trail_bbox;          /* DEVICE: outputs of mydet_trails_frames */
    const int64_t *id;                                             /* DEVICE: the tracker's out_id */
    const int32_t *missed;                                         /* DEVICE: the tracker's out_missed */
} mydet_overlay;
int mydet_draw_overlay_rgb_u8(unsigned char *dst, int B, int H, int W, int64_t dst_img_bytes, int64_t dst_row_bytes,
                              const mydet_overlay *overlay, const mydet_draw_style *style, void *stream);
int mydet_draw_overlay_yuv420_u8(const mydet_yuv420_src *planes, int B, int H, int W, const mydet_overlay *overlay,
                                 const mydet_draw_style *style, void *stream);

/* Redaction: the detections of a list are hidden -- pixelated, blurred or painted over -- IN PLACE in uint8 RGB frames or in the
 * planes of the 8-bit 4:2:0 layouts, before a frame leaves the device for an encoder, a screen or a disk (csrc/redact.hip).  No
 * reference counterpart: the rules are this library's own, integer-exact, and they are these.
 *
 * List.  The renderer's mydet_draw_list, read in place: a record buffer's planes or a dense [B,K,5] array.  The renderer's skip
 *   rules hold unchanged: a row with a non-finite cx, cy, w, h or angle, or with w <= 0 or h <= 0, is skipped; a frame with
 *   count <= 0 is skipped; a count above K means K; a NULL count means K.  Nothing outside the H x W view is read or written.
 * Class filter.  n_classes == 0: every row is redacted.  n_classes in 1..MYDET_REDACT_MAX_CLASSES: only rows whose class is one
 *   of classes[0..n_classes) (the shape of mydet_zone_set's filter); the list then needs its cls plane.
 * Coverage.  The renderer's geometry: pixel centre (j + 0.5, i + 0.5); a, b, c and s exactly those of the overlay renderer
 *   above (csrc/box_rot.h; angle == 0 makes no trigonometric call); float32, uncontracted.  With ra = (w * 0.5f) * pad and
 *   rb = (h * 0.5f) * pad:
 *       MYDET_REDACT_BOX      covered iff a <= ra && b <= rb
 *       MYDET_REDACT_ELLIPSE  covered iff (a*rb)*(a*rb) + (b*ra)*(b*ra) <= (ra*rb)*(ra*rb)
 *   A pixel is redacted iff some row of its frame covers it.  Row order and overlaps do not matter: every new value is a function
 *   of the ORIGINAL frame and of the pixel's position only.
 * Cells.  The cell grid is anchored at the frame origin; cell = c is even, MYDET_REDACT_MIN_CELL..MYDET_REDACT_MAX_CELL.  Cell
 *   (I, J) holds rows [I*c, min(H, (I+1)*c)) and the matching columns; its mean, per channel and in integers, is
 *   (2*S + n) / (2*n) (round half up) with S the channel's sum and n the number of the cell's pixels inside the frame.
 * Modes.
 *   MYDET_REDACT_MOSAIC  a redacted pixel becomes the mean of its cell.
 *   MYDET_REDACT_SMOOTH  a redacted pixel becomes the bilinear interpolation of the cell means, each mean placed at its cell's
 *       nominal centre, all in integers: u = 2*j + 1 - c, J0 = floor(u / (2c)), fx = u - 2c*J0 (in [0, 2c)), Ja = clamp(J0, 0,
 *       nJ-1), Jb = clamp(J0+1, 0, nJ-1); v, I0, fy, Ia, Ib the same from i;
 *           value = ((2c-fy)*((2c-fx)*M[Ia][Ja] + fx*M[Ia][Jb]) + fy*((2c-fx)*M[Ib][Ja] + fx*M[Ib][Jb]) + 2c^2) / (4c^2)
 *       (fits int32 for c <= 64).  A strong blur whose cost does not depend on its radius.
 *   MYDET_REDACT_SOLID   a redacted pixel becomes `color`; in 4:2:0 the colour goes through the renderer's RGB -> Y'CbCr table above.
 * 4:2:0 targets (NV12, NV21, I420; YV12 = I420 with the planes exchanged by the caller; odd H and W legal; the 10-bit layouts are
 *   MYDET_E_BADARG).  Luma is redacted per pixel with the luma cell means.  A chroma sample is redacted iff any luma pixel of its
 *   quad is.  Chroma cells are c/2 x c/2 chroma samples anchored at the origin (c/2 may be odd); their means and the smooth
 *   formula use c/2 in place of c on the chroma sample grid of ceil(H/2) x ceil(W/2).
 * Launches.  The frames are written in place, a cell's mean must come from original pixels, and in `smooth` a pixel reads the
 *   means of cells that another workgroup repaints.  So the entry point issues two kernels on the stream: the first reads the
 *   frames and writes the mean of every cell the second may read (every cell that a non-skipped row's padded bounding box
 *   reaches, one cell further in `smooth`) into `workspace`, mydet_redact_workspace_bytes(B, H, W, cell) bytes (one dword per
 *   cell and frame; 4-byte aligned; its contents after the call are not part of the contract); the second reads the list and
 *   the workspace only and stores the redacted pixels.  MYDET_REDACT_SOLID issues the second alone and takes a NULL workspace.
 *   No host synchronisation, no allocation, no memset, no atomics on global memory: the pair can be captured in a graph and its
 *   result is deterministic.  A block of cells or a tile (64 x 16 pixels RGB, 128 x 16 for 4:2:0) that no padded box reaches is
 *   neither read nor written; in the others only covered pixels are stored -- with the renderer's dword accesses under the
 *   renderer's alignment conditions where a whole pixel group is covered, byte by byte otherwise, with the same result.
 * MYDET_E_BADARG, with nothing launched: what the renderer refuses for the list and the target; cell odd or outside
 *   MYDET_REDACT_MIN_CELL..MYDET_REDACT_MAX_CELL; pad not finite or <= 0; an unknown mode or shape; n_classes outside
 *   0..MYDET_REDACT_MAX_CLASSES; a class filter with a NULL cls plane; a NULL workspace when the mode needs one.
 *   mydet_redact_workspace_bytes returns MYDET_E_BADARG for non-positive B, H, W or such a cell.
 * MYDET_E_UNSUPP: B or ceil(H / 16) above 65535 (the renderer's grid limits), or H or W of 2^22 or more. */
#define MYDET_REDACT_MOSAIC      0
#define MYDET_REDACT_SMOOTH      1
#define MYDET_REDACT_SOLID       2
#define MYDET_REDACT_BOX         0
#define MYDET_REDACT_ELLIPSE     1
#define MYDET_REDACT_MIN_CELL    4
#define MYDET_REDACT_MAX_CELL    64
#define MYDET_REDACT_MAX_CLASSES 16
typedef struct mydet_redact_style {
    int mode, shape, cell;                   /* MYDET_REDACT_MOSAIC | _SMOOTH | _SOLID; MYDET_REDACT_BOX | _ELLIPSE; cell size */
    float pad;                               /* the box is scaled by this before it is covered */
    unsigned char color[4];                  /* R, G, B of MYDET_REDACT_SOLID; [3] ignored */
    int n_classes;
    int classes[MYDET_REDACT_MAX_CLASSES];
} mydet_redact_style;
int64_t mydet_redact_workspace_bytes(int B, int H, int W, int cell);
int mydet_redact_boxes_rgb_u8(unsigned char *dst, int B, int H, int W, int64_t img_bytes, int64_t row_bytes,
                              const mydet_draw_list *list, const mydet_redact_style *style, void *workspace, void *stream);
int mydet_redact_boxes_yuv420_u8(const mydet_yuv420_src *planes, int B, int H, int W,
                                 const mydet_draw_list *list, const mydet_redact_style *style, void *workspace, void *stream);

/* Object chips: the image of every box of a list, cut out of uint8 RGB frames or of 4:2:0 planes, turned upright and resampled
 * to one fixed size ch x cw, one launch per batch (csrc/crop.hip).  What attribute and re-identification classifiers, plate and
 * face recognisers and thumbnails take.  No reference counterpart: the sampling rules are this library's own, and they are these.
 *
 * Boxes.  The list is the renderer's mydet_draw_list, read in place: a record buffer's planes or a dense [B,K,5] array; a row is
 *   (cx, cy, w, h) in frame pixels and an angle in degrees (0 without an angle plane); score, cls and id are ignored.
 * Slots.  Frame b has n_b = min(count_b, K, M) chips (a NULL count plane: min(K, M); a count <= 0, which includes
 *   MYDET_COUNT_BAD_CLASS: 0).  The chip of row m < n_b is slot (b, m), at out + b*frame_stride + m*slot_stride (elements of the
 *   output type): MYDET_CROP_U8 chips are uint8 [ch][cw][3], MYDET_CROP_F32 chips are float32 [3][ch][cw].  Slots m >= n_b are NOT
 *   WRITTEN: their workgroups return before they touch memory.  A row m < n_b with a non-finite cx, cy, w, h or angle, or with
 *   w <= 0 or h <= 0, gets a chip of the `fill` colour, so the slot index always equals the row index.
 * Rotation.  angle == 0 uses c = 1, s = 0 with no trigonometric call.  With r = fmodf(angle, 360): r = +90 or -270 gives
 *   (c, s) = (0, 1), r = +-180 gives (-1, 0), r = +270 or -90 gives (0, -1), exactly; any other angle gives c, s = cosf, sinf of
 *   r * (pi / 180) in float32, as in the overlay renderer (which has no exact quarter turns).
 * Coordinates, all float32 and uncontracted, in the order written.  sx = (w * pad) / cw, sy = (h * pad) / ch (pad > 1 adds
 *   context around the box).  nx = clamp((int)ceilf(sx), 1, 4), ny likewise from sy: nx * ny sub-samples per chip pixel, so a
 *   downscale up to 4x does not alias; a larger one does (4 x 4 samples spread evenly over the pixel's footprint).  For chip pixel
 *   (row i, column j) and sub-sample (p, q), 0 <= p < ny, 0 <= q < nx:
 *       lx = ((float)j + ((float)q + 0.5f) / nx - 0.5f * cw) * sx
 *       ly = ((float)i + ((float)p + 0.5f) / ny - 0.5f * ch) * sy
 *       X  = cx + lx*c - ly*s
 *       Y  = cy + lx*s + ly*c
 *   the inverse of the renderer's a = dx*c + dy*s, b = -dx*s + dy*c: the chip's x axis runs along the box's w, so a rotated
 *   object comes out upright.  (X, Y) is a point of the frame in the renderer's convention: pixel (y, x) has its centre at
 *   (x + 0.5, y + 0.5).
 * Sample.  The point is quantised to 1/32 pixel: qx = (int)floorf((X - 0.5f) * 32 + 0.5f), x0 = qx >> 5 (arithmetic shift),
 *   fx = qx & 31; qy, y0, fy likewise from Y.  Bilinear, per channel, in integers, from the pixels p00 = (y0, x0), p01 = (y0, x0 + 1),
 *   p10 = (y0 + 1, x0), p11 = (y0 + 1, x0 + 1):
 *       top = p00*(32 - fx) + p01*fx,  bot = p10*(32 - fx) + p11*fx,  v = (top*(32 - fy) + bot*fy + 512) >> 10
 *   A tap outside the H x W view reads as the `fill` colour; nothing outside the view is addressed.  A point whose floorf value
 *   is NaN or beyond +-2^29 in either axis (no view reaches there: H, W <= 2^24, MYDET_E_UNSUPP beyond) has four fill taps.
 * Chip value, per channel: (sum of v over the nx*ny sub-samples + (n >> 1)) / n with n = nx*ny, an integer in 0..255.
 *   MYDET_CROP_F32 writes that value through the arithmetic of mydet_preprocess_u8_f32: x / 255, then with norm != 0
 *   (x - mean) / std per channel; mean3 / std3 are HOST pointers to 3 floats (read only when norm != 0).
 * 4:2:0 sources (mydet_crop_boxes_yuv420; all five layouts, the 10-bit ones included, YV12 as I420 with the planes exchanged):
 *   every tap is converted by the formula, the table and the 10-bit rule of mydet_yuv420_to_rgb_u8, chroma nearest at
 *   (y >> 1, x >> 1), so the chips are, bit for bit, the chips of the RGB frames that function gives -- which are never built.
 *   `fill` is an RGB colour here too.
 * Stores.  16 bytes per lane into each float plane, dwords of packed pixels for uint8, when cw % 4 == 0, the output address is
 *   a multiple of 16 (float) or 4 (uint8) and both strides are multiples of 4 elements; element by element otherwise, with the
 *   same result.
 * MYDET_E_BADARG, with nothing launched: a null list, out, box plane, source or output pointer; non-positive B, H, W; a source
 *   pitch below the row's bytes; a negative stride; slot_stride < 3*ch*cw; K outside 1..MYDET_DRAW_MAX_BOXES; M outside
 *   1..MYDET_CROP_MAX_SLOTS; ch or cw outside 1..MYDET_CROP_MAX_SIDE; pad not finite or <= 0; an unknown kind; norm != 0 with a
 *   null mean3 or std3; and what mydet_yuv420_src refuses on the input side (layout, matrix, range, planes, pitches, odd 16-bit
 *   addresses). */
#define MYDET_CROP_MAX_SIDE  256
#define MYDET_CROP_MAX_SLOTS 512
#define MYDET_CROP_U8        0
#define MYDET_CROP_F32       1
typedef struct mydet_crop_out {
    int ch, cw;                      /* chip rows, columns */
    int M;                           /* chip slots per frame */
    int kind;                        /* MYDET_CROP_U8 | MYDET_CROP_F32 */
    float pad;                       /* the box is scaled by this before it is cut out */
    unsigned char fill[4];           /* R, G, B of taps outside the view and of skipped rows; [3] ignored */
    int norm, reserved;
    const float *mean3, *std3;       /* HOST pointers, as in mydet_preprocess_u8_f32 */
    void *out;                       /* DEVICE: uint8 or float32 by `kind` */
    int64_t slot_stride, frame_stride;   /* elements between the chips of a frame / between frames */
} mydet_crop_out;
int mydet_crop_boxes_rgb(const unsigned char *src, int B, int H, int W, int64_t src_img_bytes, int64_t src_row_bytes,
                         const mydet_draw_list *list, const mydet_crop_out *out, void *stream);
int mydet_crop_boxes_yuv420(const mydet_yuv420_src *src, int B, int H, int W,
                            const mydet_draw_list *list, const mydet_crop_out *out, void *stream);

/* Appearance: a colour descriptor per box (csrc/appear.hip) and a tracker that matches by it too (csrc/track.hip), DeepSORT's and
 * BoT-SORT's appearance branch with a colour histogram in place of a ReID network (the library ships no weights).  The tracker
 * side takes ANY array of 128 uint16 bins per detection whose bins sum to at most 512 (not checked; S below is then <= 131072
 * and cannot overflow), so a learned embedding can be quantised into it.  No reference counterpart: the rules are this library's.
 *
 * Descriptor (mydet_appear_boxes_rgb_u8 / _yuv420).  Arguments as the crop entry points: the frames or a mydet_yuv420_src, B, H,
 *   W, and a mydet_draw_list read in place (box and angle planes, count; score, cls, id ignored).  Out: desc, uint16
 *   [B][K][128], frame b at desc + b*desc_frame_stride (elements).  EVERY row k < K of every frame is written: a row at or beyond
 *   the frame's count (NULL count: K; a negative count -- MYDET_COUNT_BAD_CLASS -- is 0) is 128 zeros.
 *   Geometry, float32 and uncontracted, in the order written.  (c, s) by the Rotation rule of the object chips above (angle 0
 *   without an angle plane).  32 rows x 16 columns of samples over the central 0.75 of the box:
 *       sx = w * 0.75f / 16,  sy = h * 0.75f / 32
 *       lx = ((float)j + 0.5f - 8.0f) * sx,  ly = ((float)i + 0.5f - 16.0f) * sy      (0 <= i < 32, 0 <= j < 16)
 *       X  = cx + lx*c - ly*s,  Y = cy + lx*s + ly*c
 *   Sampling.  A sample whose X or Y is NaN or has |.| > 2^29 is not counted (only a non-finite or absurd box has such samples).
 *   Every other sample reads the nearest pixel x = clamp((int)floorf(X), 0, W-1), y = clamp((int)floorf(Y), 0, H-1): a box
 *   outside the frame reads edge pixels, nothing outside the view is addressed.
 *   Bin of a sample with pixel (R, G, B): (i >> 4)*64 + (R >> 6)*16 + (G >> 6)*4 + (B >> 6) -- the upper and the lower half of
 *   the object each get a joint 4 x 4 x 4 colour histogram.  desc[b][k][bin] = the number of samples; a row sums to at most 512.
 *   4:2:0 sources: every layout of mydet_crop_boxes_yuv420, every tap converted as there, so the descriptors are bit for bit
 *   those of the RGB frames mydet_yuv420_to_rgb_u8 gives, which are never built.
 *   MYDET_E_BADARG, nothing launched: a null list, box plane, source or desc; non-positive B, H, W; a source pitch below the row's
 *   bytes; a negative stride; K outside 1..MYDET_DRAW_MAX_BOXES; desc not 4-byte aligned; desc_frame_stride odd or < K*128; and
 *   what mydet_yuv420_src refuses.  MYDET_E_UNSUPP: B > 65535, H or W > 2^24.
 *
 * Tracker (mydet_track_frames_appear_f32): mydet_track_frames_motion_f32 (shift may be NULL) with
 *   appear        HOST pointer to the settings below;
 *   desc          DEVICE uint16, the descriptors of frame o = s*F + f at desc + o*512*128, row = record slot; 16-byte aligned;
 *   appear_state  DEVICE int32, S * mydet_track_appear_state_words(max_tracks) words, 16-byte aligned, caller-owned, persistent,
 *                 all zero at the start.  Per stream, MT = max_tracks: has [MT] (1: the slot's track has a template), then
 *                 tmpl [128][MT] in units of 1/256 sample (bin-major), zero padding to a multiple of 4 words;
 *   out_sim, out_how   int32 [S*F][max_tracks].
 *   Similarity: S(j, d) = sum over the 128 bins of min(tmpl[b][j], 256 * desc[d][b]), an int32 in 0..MYDET_APPEAR_SIM_MAX.
 *   Per frame, beside the rules of mydet_track_frames_f32 and mydet_track_assoc (greedy; one band or two):
 *   gate      in the walk, a pair that passes every test of today's walk and iou > the threshold is offered only if gate == 0,
 *             or has[j] == 0, or S(j, d) >= gate.  The key stays IoU-major with the same tie rule.
 *   re-identification   after the walk, before the update, if reid > 0.  In rank order, every detection that is still unmatched and
 *             would be born (score >= new_thres; with bands also >= high_thres) is offered to every live track j that is
 *             unmatched, of its class, has[j] == 1, missed >= 2 after predict, and within reach: with m = max(x[2], x[3], z_w,
 *             z_h), fabsf(z_cx - x[0]) <= reach*m and fabsf(z_cy - x[1]) <= reach*m (float32; x the prediction after the
 *             camera shift), and S(j, d) >= reid.  The largest S wins, the lowest slot on a tie; the winner takes the detection
 *             exactly as a matched track does (update, score, missed = 0).
 *   template  a track matched in any stage to a detection with score >= update_thres: t += ((256*d - t) * alpha) >> 8 per bin
 *             (arithmetic shift, alpha in 1..256), or t = 256*d when has == 0, which sets has.  A birth writes t = 256*d,
 *             has = 1.  A retired slot clears both.  A bad-class frame leaves everything alone.
 *   out_how   -1 a free slot, 0 live and unmatched, 1 / 2 matched in the high / low band, 3 re-identified, 4 born.
 *   out_sim   S of the pair that matched, with the template as it was before the update (0 for has == 0), else -1.
 *   With gate == 0 and reid == 0 every other output and the tracker state are those of mydet_track_frames_motion_f32.
 *   MYDET_E_BADARG: as mydet_track_frames_motion_f32, and a null or misaligned appear, desc, appear_state, out_sim or out_how;
 *   gate or reid outside 0..MYDET_APPEAR_SIM_MAX; alpha outside 1..256; reach negative or not finite; update_thres NaN.
 *   MYDET_E_UNSUPP: MYDET_TRACK_ASSIGN_OPTIMAL (the solver forms its costs on the fly and would recompute S inside its inner
 *   loop: mydet_track_frames_appear_optimal_f32 below computes S ahead of the solve and fuses it into the cost).
 *   mydet_track_appear_state_words is 0 for a max_tracks the tracker refuses. */
#define MYDET_APPEAR_BINS    128
#define MYDET_APPEAR_SAMPLES 512
#define MYDET_APPEAR_SIM_MAX 131072      /* 256 * MYDET_APPEAR_SAMPLES */
typedef struct mydet_track_appear {
    int gate, reid;                      /* on the scale of S; 0 = off */
    int alpha;                           /* 1..256: the template moves by alpha/256 of the difference */
    float reach;                         /* re-identification: centre distance per axis, in units of the larger box side */
    float update_thres;                  /* the detection score from which a match moves the template */
    int reserved[3];
} mydet_track_appear;
int mydet_appear_boxes_rgb_u8(const unsigned char *src, int B, int H, int W, int64_t src_img_bytes, int64_t src_row_bytes,
                              const mydet_draw_list *list, uint16_t *desc, int64_t desc_frame_stride, void *stream);
int mydet_appear_boxes_yuv420(const mydet_yuv420_src *src, int B, int H, int W, const mydet_draw_list *list, uint16_t *desc,
                              int64_t desc_frame_stride, void *stream);
int64_t mydet_track_appear_state_words(int max_tracks);
int mydet_track_frames_appear_f32(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S, int F,
                                  int box_width, const mydet_track_params *params, int max_tracks, int32_t *state,
                                  float *out_box, float *out_score, int64_t *out_class, int64_t *out_id, int32_t *out_missed,
                                  int32_t *out_count, int32_t *out_dropped, const mydet_track_assoc *assoc, const int32_t *shift,
                                  const mydet_track_appear *appear, const uint16_t *desc, int32_t *appear_state,
                                  int32_t *out_sim, int32_t *out_how, void *stream);
/* ... with the similarity model: `warp` of mydet_track_frames_warp_f32 in the place of shift, the same rule */
int mydet_track_frames_appear_warp_f32(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S, int F,
                                       int box_width, const mydet_track_params *params, int max_tracks, int32_t *state,
                                       float *out_box, float *out_score, int64_t *out_class, int64_t *out_id, int32_t *out_missed,
                                       int32_t *out_count, int32_t *out_dropped, const mydet_track_assoc *assoc, const int32_t *warp,
                                       const mydet_track_appear *appear, const uint16_t *desc, int32_t *appear_state,
                                       int32_t *out_sim, int32_t *out_how, void *stream);

/* Appearance in the optimal assignment (mydet_track_frames_appear_optimal_f32): mydet_track_frames_appear_f32 with
 *   weight   0..256, the share of the appearance in the fused affinity below;
 *   sim_ws   DEVICE int32, S * mydet_track_appear_ws_words(max_tracks) words (512 * max_tracks per stream), 16-byte aligned,
 *            caller-owned; nothing is assumed about its content at the start.
 * It takes assoc->assign == MYDET_TRACK_ASSIGN_OPTIMAL only.  Every rule of mydet_track_frames_appear_f32 holds word for word --
 * predict with the camera shift, update, the template update at update_thres, retire, births, out_how, out_sim (S of the matched
 * pair with the template as it was before the update), bad-class frames -- except the associate step, which is the optimal one
 * of mydet_track_assoc: the same rows, columns, dummies, solver and tie rule, one band or two.  Only the cost of a real column
 * changes.  With q = (int)floorf(iou * 65536.0f), S = S(j, d) with the template before this frame's update, and a = S >> 1
 * (0..65536), for a pair (row i = detection d, column j), all in integers:
 *   eligible   as in mydet_track_assoc (the track is live, not taken by an earlier stage, of the detection's class, passes the
 *              stage-2 missed == 1 rule, iou > the stage's threshold), and it passes the gate: gate == 0, or has[j] == 0, or
 *              S >= gate;
 *   affinity   m = q when has[j] == 0, else m = ((256 - weight) * q + weight * a) >> 8;
 *   cost       65536 - m when eligible, 131072 when not, 65536 on a dummy column.
 * Re-identification (reid > 0) keeps its rule: the rank-order walk after the stages, the largest S wins, the lowest slot on a
 * tie, how = 3.  It runs behind the solve exactly as it runs behind the walk.
 * With weight == 0, gate == 0 and reid == 0 every tracker output and every word of the tracker state are those of
 * mydet_track_frames_motion_f32 with the same optimal assoc.
 * The workspace.  S is computed once per pair, by the whole workgroup, between predict and the solve; the solver's cost reads
 *   one word of it.  After a launch, for each stream whose last frame is not a bad-class frame, with n that frame's detections
 *   and MT = max_tracks: sim_ws[d * MT + j] == S(j, d), with the templates as they were before that frame's update, for every
 *   NEEDED pair (d < n, j): track j is live after predict, has[j] == 1, track j has the class of d, iou > the threshold of d's
 *   band, and for a low-band d missed == 1.  None of that depends on the solver's outcome.  Every other word may hold anything.
 * MYDET_E_BADARG: everything mydet_track_frames_appear_f32 answers so; weight outside 0..256; a null or misaligned sim_ws.
 * MYDET_E_UNSUPP: MYDET_TRACK_ASSIGN_GREEDY (the walk's key stays IoU-major), and max_tracks above MYDET_TRACK_MAX_TRACKS.
 * Nothing is launched and no buffer is touched on either.  mydet_track_appear_ws_words is 0 for a max_tracks the tracker refuses. */
int64_t mydet_track_appear_ws_words(int max_tracks);
int mydet_track_frames_appear_optimal_f32(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S, int F,
                                          int box_width, const mydet_track_params *params, int max_tracks, int32_t *state,
                                          float *out_box, float *out_score, int64_t *out_class, int64_t *out_id, int32_t *out_missed,
                                          int32_t *out_count, int32_t *out_dropped, const mydet_track_assoc *assoc, const int32_t *shift,
                                          const mydet_track_appear *appear, const uint16_t *desc, int32_t *appear_state,
                                          int32_t *out_sim, int32_t *out_how, int weight, int32_t *sim_ws, void *stream);
/* ... with the similarity model: `warp` of mydet_track_frames_warp_f32 in the place of shift, the same rule */
int mydet_track_frames_appear_optimal_warp_f32(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S,
                                               int F, int box_width, const mydet_track_params *params, int max_tracks, int32_t *state,
                                               float *out_box, float *out_score, int64_t *out_class, int64_t *out_id,
                                               int32_t *out_missed, int32_t *out_count, int32_t *out_dropped,
                                               const mydet_track_assoc *assoc, const int32_t *warp, const mydet_track_appear *appear,
                                               const uint16_t *desc, int32_t *appear_state, int32_t *out_sim, int32_t *out_how,
                                               int weight, int32_t *sim_ws, void *stream);

/* Key frames: the detector runs on every n-th frame only, and the boxes of a key frame are carried through the frames that follow
 * by matching their pixels (csrc/carry.hip), so that the tracker still gets one record per frame.  Everything after one conversion
 * of the box is integer arithmetic; tests/_carry_ref.py restates the rules and the kernels equal it with == on every output and
 * on every word of the state.  The reference project has nothing like it (DeepStream's `interval` with a visual tracker is the
 * deployed form of the idea).
 *
 * Frames: frame f of stream s is frame o = s*F + f of the B = S*F frames of the call.  `first` in [0, every) is the place of the
 * call's frame 0 inside its interval: frame f is a KEY frame when (first + f) % every == 0.  A stream has K = the number of key
 * frames among its F frames; key_records holds the detector's records of the key frames, stream-major: key k of stream s is row
 * s*K + k, rows key_stride_words apart, each a record of MYDET_REC_WORDS (box_width 4) or MYDET_REC_ROT_WORDS (box_width 5) words.
 * Luma L(y, x): that of the camera-motion estimator above, per source.  A coordinate outside the frame clamps to the edge.
 * Every slot (the 512 rows of a record) of every stream is carried on its own.
 *
 * 1. Key frame.  The frame's row of out_records is its key record, every word copied.  With COUNT outside 1 .. 512 (0, the
 *    bad-class marker) no slot is carried: every slot is EMPTY.  Otherwise slot j >= COUNT is EMPTY, and slot j < COUNT takes
 *    v16 = (int) floorf(v * 16.0f + 0.5f), float32 with separate multiply and add, of v = cx, cy, w, h.  It is NOT CARRIABLE
 *    when one of the four is not finite or |v| >= 2^26, or w16 <= 0 or h16 <= 0.  Else it is ALIVE with m = min(w16, h16),
 *    side = 3 m / 4 (box_width 5: m / 2, which lies inside the box at any angle), the cell size s = clamp((side + 255) / 256, 1, 16)
 *    pixels, X = cx16 >> 4, Y = cy16 >> 4 (arithmetic shifts), off = (0, 0), rel = (0, 0), and its template is taken from this
 *    frame:   coarse  C(i, j) = (sum of L over the s x s pixels at (Y - 8 s + i s, X - 8 s + j s) + s*s/2) / (s*s),  i, j in 0 .. 15;
 *             patch   P(i, j) = L(Y - 16 + i, X - 16 + j), i, j in 0 .. 31, for s >= 2 (zero bytes for s == 1).
 *    The template stays for the whole interval.
 * 2. In-between frame t, ALIVE slot.  (dx, dy) = the frame's shift when `shift` is given and its valid == 1, else (0, 0).
 *    c = clamp(off + rel + (dx, dy), -65536, 65536) per axis.  Coarse search: for every (i, j) in [-R, R]^2, R = `search`, the SAD of
 *    C against the 16 x 16 cell means of frame t, computed like C, whose grid starts at (Y - 8 s + c.y + i s, X - 8 s + c.x + j s).
 *    The best candidate is the smallest (SAD, i*i + j*j, i, j), compared lexicographically (the estimator's order); smin = its
 *    SAD, smax = the largest SAD.  smax - smin < min_texture: the slot is FLAT.  Else smin > 256 max_diff: it is LOST.  Else
 *    n = c + (j s, i s), and for s >= 2 the refine search: for every (ey, ex) in [-s, s]^2 the SAD of P against L of frame t at
 *    (Y - 16 + n.y + ey, X - 16 + n.x + ex); the best by (SAD, ey*ey + ex*ex, ey, ex); n = n + (ex, ey).  Then
 *    rel = (n - off) - (dx, dy), off = n.  With (X + off.x, Y + off.y) outside [0, W) x [0, H) the slot has LEFT.
 *    A FLAT, LOST or LEFT slot, like a NOT CARRIABLE one, stays what it is until the next key frame.
 * 3. The row of an in-between frame: the ALIVE slots in key order, compacted.  cx = cx + (float) off.x, cy = cy + (float) off.y,
 *    one float32 add each; w, h, angle, score and class are the key slot's; INDEX = the key slot; COUNT = their number; 3 zero
 *    words; entries from COUNT on are zero.
 * Out: out_how int32 [S*F][512]: 0 EMPTY, 1 in a key frame's row (slots below its COUNT in 1 .. 512), 2 carried, 3 FLAT, 4 LOST,
 *   5 LEFT, 6 NOT CARRIABLE; 3 .. 6 are repeated in every in-between frame until the next key frame.  out_offset int32
 *   [S*F][512][2] = off (x, y) where how == 2, else 0.  out_sad int32 [S*F][512][2] = (smin, smax) in the frame in which the slot was
 *   searched (how 2, and 3 .. 5 in the frame they were decided), else 0.
 * state: S * mydet_carry_state_words() int32 words, 16-byte aligned, caller-owned, persistent; mydet_carry_reset makes it all zero.
 *   Per stream 512 slots of MYDET_CARRY_SLOT_WORDS words:  [0] status (0 EMPTY, 2 ALIVE, 3 .. 6)  [1] s  [2] cx16  [3] cy16
 *   [4] off.x  [5] off.y  [6] rel.x  [7] rel.y  [8 .. 11] the key box (cx, cy, w, h) f32  [12] angle f32 (0 for box_width 4)  [13] score f32
 *   [14, 15] class i64  [16 .. 79] C, 256 bytes  [80 .. 335] P, 1024 bytes.  Every word but [0] is zero unless the slot is ALIVE.
 *   Two calls of F1 and F2 frames (first of the second = (first + F1) % every) leave exactly the outputs and the state of one call
 *   of F1 + F2 frames.  A workgroup is the only reader and writer of its slot's state.
 * ws: device scratch of S * 512 * 8 int32 words, stream-ordered (the key fields of the slots that a call carries in from the state).
 * shift: NULL, or DEVICE int32 [S*F][4] = (dx, dy, valid, n_valid), out_shift of the estimator above.
 * Frames are read in place: RGB packed pixels with any row and frame stride; 4:2:0 through mydet_yuv420_src, every layout.
 * Not part of the rules: scale, rotation or deformation of a carried box, sub-pixel offsets, a template update within an interval.
 * MYDET_E_BADARG, with nothing launched: B or S < 1, B no multiple of S, S > 65535; a null set; every outside 1 .. 16; search outside
 *   4 .. 16; min_texture outside [0, 2^24); max_diff outside 0 .. 255; first outside [0, every); box_width not 4 or 5; a null or
 *   misaligned pointer (state, out_records, key_records: 16 bytes; the others: 4; key_records may be NULL when K == 0, shift always);
 *   key_stride_words below the record's words or no multiple of 4; H or W outside 1 .. 32768; the source errors of the pixel format. */
#define MYDET_CARRY_SLOTS        512
#define MYDET_CARRY_SLOT_HEADER  16
#define MYDET_CARRY_SLOT_WORDS   336      /* header + 1280 template bytes */
#define MYDET_CARRY_MAX_EVERY    16
#define MYDET_CARRY_HOW_NONE     0
#define MYDET_CARRY_HOW_KEY      1
#define MYDET_CARRY_HOW_CARRIED  2
#define MYDET_CARRY_HOW_FLAT     3
#define MYDET_CARRY_HOW_LOST     4
#define MYDET_CARRY_HOW_LEFT     5
#define MYDET_CARRY_HOW_NOT      6
typedef struct mydet_carry_set {
    int every;                           /* a key frame every n-th frame, 1 .. 16 */
    int search;                          /* R: the coarse search range in cells, 4 .. 16 */
    int min_texture;                     /* the least SAD range over the candidates of a slot that is followed */
    int max_diff;                        /* the largest mean absolute cell difference of a match, 0 .. 255 */
    int reserved[4];
} mydet_carry_set;
int64_t mydet_carry_state_words(void);
int mydet_carry_reset(int32_t *state, int S, void *stream);
int mydet_carry_records_rgb_u8(const unsigned char *src, int B, int H, int W, int64_t src_img_bytes, int64_t src_row_bytes, int S,
                               const mydet_carry_set *set, int first, const int32_t *key_records, int64_t key_stride_words,
                               int box_width, int32_t *state, const int32_t *shift, int32_t *ws, int32_t *out_records,
                               int32_t *out_how, int32_t *out_offset, int32_t *out_sad, void *stream);
int mydet_carry_records_yuv420(const struct mydet_yuv420_src *src, int B, int H, int W, int S, const mydet_carry_set *set, int first,
                               const int32_t *key_records, int64_t key_stride_words, int box_width, int32_t *state,
                               const int32_t *shift, int32_t *ws, int32_t *out_records, int32_t *out_how, int32_t *out_offset,
                               int32_t *out_sad, void *stream);

/* Scoring detections against ground truth: COCO's bbox evaluation with useCats = 1, in three stream-ordered launches
 * (csrc/evalmatch.hip).  Replaces utils/evaluation/coco.py (coco_evaluate_bbox, myCOCOeval) and utils/evaluation/cepdof.py
 * (evaluate_json, CEPDOFeval) of the reference, which sit on pycocotools: its computeIoU, evaluateImg and accumulate.  The
 * summary (12 stats and the text) is host code.  Defaults: iouThrs = np.linspace(.5, .95, 10), recThrs = np.linspace(0, 1, 101),
 * maxDets = [1, 10, 100], areaRng = [[0, 1e10], [0, 32^2], [32^2, 96^2], [96^2, 1e10]]; every threshold array is computed by
 * numpy on the host and passed in as float64 through a HOST pointer, so the bits are numpy's.
 *
 * Packing (host side; mydetection_amd.ops.eval_pack).
 *   Images are indexed i in the order of the sorted unique image ids of the ground truth, categories k in the order of its sorted
 *   unique category ids.  A group is one (image, category) pair, g = k*I + i (category-major).  Detections whose image or
 *   category id is not in the ground truth are dropped.  Per group the detections are in (score descending, input order) order
 *   (a stable sort) and cut to maxDets[-1]; the ground truths keep annotation order.  Dense arrays, D detections, G ground truths:
 *     dt_start, gt_start  int32 [I*K + 1]          rows of group g: [start[g], start[g + 1])
 *     dt_score, dt_area   float64 [D];  gt_area float64 [G]
 *     gt_flags            uint8 [G]: bit 0 (MYDET_EVAL_GT_IGNORE) ignore, bit 1 (MYDET_EVAL_GT_CROWD) iscrowd
 *     boxes               float64 (x, y, w, h) rows, rotated == 0;  float32 (cx, cy, w, h, deg) rows, rotated == 1
 *     groups              int32 [n_groups]: the groups that hold a detection or a ground truth, ascending (the launches run
 *                         over these only: I*K may be 400 000 with most groups empty)
 *     pair_start          int64 [n_groups + 1]: listed group c owns IoU entries [pair_start[c], pair_start[c + 1]), Dg*Gg of them,
 *                         detection-major: entry pair_start[c] + d*Gg + j is (detection of rank d, ground truth j)
 *   Defaults.  coco: gt.ignore = iscrowd; dt.area = w*h if absent.  cepdof: gt.area = w*h if absent, gt.ignore = ignore or
 *   iscrowd, dt.area = w*h if absent, dt.category_id = 1 if absent.
 *   order int32 [D] is the per-category global order: category k's detections, order[cat_start[k] .. cat_start[k + 1]), sorted by
 *   (score descending, image index ascending, rank in group ascending); dt_rank int32 [D] is a detection's rank in its group.
 *
 * IoU (mydet_eval_ious_f64): one thread per pair, float64 [n_pairs] out; it is also what pycocotools keeps as `ious`.
 *   Axis-aligned, all float64 and uncontracted, in this order: da = dw*dh, ga = gw*gh; w = fmin(dx+dw, gx+gw) - fmax(dx, gx), if
 *   w <= 0 the IoU is 0; h likewise, if h <= 0 the IoU is 0; i = w*h; u = da for a crowd ground truth, else da + ga - i;
 *   iou = i/u.
 *   Rotated: the float32 IoU of mydet_rotated_iou_f32 (a = the detection, b = the ground truth) widened to float64.  Crowd flags
 *   do not change it (the reference passes iscrowd = 0 there).  This is the exact-area deviation from the reference's rasterised
 *   iou_rle, the same one as for the rotated NMS.
 *
 * Matching (mydet_eval_match_f64): per group, per area range a = (lo_a, hi_a) and per threshold t, independently.
 *   gtIg[j] = ignore[j] or area[j] < lo_a or area[j] > hi_a.  Ground truths are visited in (gtIg ascending, annotation order)
 *   order, detections in rank order.  For a detection, start with best = min(t, 1 - 1e-10) and m = none; for every ground truth
 *   j in that order: skip j if it is already matched at (a, t) and is not crowd; stop if m is set, gtIg[m] == 0 and gtIg[j] == 1;
 *   skip j if iou[d, j] < best; otherwise best = iou[d, j], m = j (an equal IoU moves the match to the later ground truth).  If m
 *   is set the detection is matched at (a, t), its ignore flag is gtIg[m], and m is marked matched.  Afterwards an unmatched
 *   detection is ignored if dt_area < lo_a or dt_area > hi_a.
 *   Outputs: dt_matched, dt_ignored uint32 [A][D], bit t = matched / ignored at (a, t); dt_gt (may be NULL) int32 [A][T][D], the
 *   matched ground-truth row (an index into the G rows) or -1.  Rows of detections are written for every listed group.
 *
 * Accumulating (mydet_eval_accumulate_f64): per (k, a, m), the detections of category k in `order` with rank < maxDets[m].
 *   npig = the number of ground truths of the category with gtIg == 0; if npig == 0, precision, recall and scores are -1.
 *   Otherwise, per t: tp and fp are the cumulative integer counts of (matched and not ignored) and (not matched and not
 *   ignored); in float64 rc = tp/npig and pr = tp/(fp + tp + 2^-52); pr[i] becomes max(pr[i:]); recall = rc[-1], or 0 without
 *   detections; for each recall threshold r, p is the first index with rc[p] >= recThrs[r], precision = pr[p] and score =
 *   dt_score[order[p]], both 0 when there is no such index.
 *   Outputs, every element written: precision [T,R,K,A,M], recall [T,K,A,M], scores [T,R,K,A,M], float64 -- the reference's
 *   eval['precision' | 'recall' | 'scores'].
 *
 * Every pointer of mydet_eval_set and every array argument below is a DEVICE pointer, except iou_thrs, area_rng ([A][2]: lo, hi),
 * max_dets and rec_thrs, which are HOST pointers read before the launch.
 * MYDET_E_BADARG, nothing launched -- all three: a null set; rotated not 0 | 1; I or K < 1 or I*K beyond int32; a negative
 *   count; D or G beyond int32; n_groups > I*K, or 0 with D > 0 or G > 0; max_dt > D, max_gt > G, n_pairs > D*G; a null dt_start or
 *   gt_start; null groups / pair_start with n_groups > 0; a null detection array with D > 0 or ground-truth array with G > 0; a
 *   null output that would be written.  match and accumulate: T, A (M, R) < 1; a null threshold array; a NaN IoU threshold; an
 *   area range with lo > hi or a NaN; maxDets not ascending or < 1; recThrs not ascending or NaN; null order, dt_rank or masks with
 *   D > 0; a null cat_start.
 * MYDET_E_UNSUPP, nothing launched: max_gt > MYDET_EVAL_MAX_GT (ground truths of one group); max_dt or maxDets[-1] >
 *   MYDET_EVAL_MAX_DT; T > MYDET_EVAL_MAX_THRS (the masks are 32 bits); A > MYDET_EVAL_MAX_AREAS; M > MYDET_EVAL_MAX_DETS;
 *   R > MYDET_EVAL_MAX_RECS.  A group whose table holds more ground truths than max_gt promised is left unwritten by the matcher.
 * No launch needs scratch memory or a workspace.  D == 0: ious and match return 0 at once; accumulate still writes its outputs. */
#define MYDET_EVAL_MAX_GT    1024
#define MYDET_EVAL_MAX_DT    1024
#define MYDET_EVAL_MAX_THRS  32
#define MYDET_EVAL_MAX_AREAS 8
#define MYDET_EVAL_MAX_DETS  8
#define MYDET_EVAL_MAX_RECS  128
#define MYDET_EVAL_GT_IGNORE 1
#define MYDET_EVAL_GT_CROWD  2
typedef struct mydet_eval_set {
    int rotated;                     /* 0: float64 (x, y, w, h) boxes; 1: float32 (cx, cy, w, h, deg) boxes */
    int I, K;                        /* images, categories */
    int n_groups;                    /* listed (non-empty) groups */
    int max_dt, max_gt;              /* the largest detection / ground-truth count of one group */
    int64_t D, G, n_pairs;           /* detections, ground truths, IoU entries (pair_start[n_groups]) */
    const int32_t *groups;
    const int32_t *dt_start, *gt_start;
    const int64_t *pair_start;
    const void *dt_box, *gt_box;
    const double *dt_score, *dt_area, *gt_area;
    const unsigned char *gt_flags;
} mydet_eval_set;
int mydet_eval_ious_f64(const mydet_eval_set *set, double *ious, void *stream);
int mydet_eval_match_f64(const mydet_eval_set *set, const double *ious, const double *iou_thrs, int T, const double *area_rng, int A,
                         uint32_t *dt_matched, uint32_t *dt_ignored, int32_t *dt_gt, void *stream);
int mydet_eval_accumulate_f64(const mydet_eval_set *set, const int32_t *order, const int32_t *cat_start, const int32_t *dt_rank,
                              const uint32_t *dt_matched, const uint32_t *dt_ignored, int T, const double *area_rng, int A,
                              const int32_t *max_dets, int M, const double *rec_thrs, int R, double *precision, double *recall,
                              double *scores, void *stream);

/* Scoring tracks against ground truth: the CLEAR MOT counts (Bernardin & Stiefelhagen, applied as py-motmetrics applies them) and
 * the identity counts behind IDF1 (Ristani et al.), in three stream-ordered launches (csrc/mot.hip) behind mydet_eval_ious_f64.
 * The reference has no tracking loop and no track scorer; its CEPDOF / COSSY annotations carry a person_id per box, and tracked
 * calls return ImageObjects.obj_ids: this is the scorer between them.  Agreement with py-motmetrics or TrackEval themselves is not
 * claimed; what is claimed, and tested with ==, is the rules below.
 *
 * Data model.  The packed arrays of mydet_eval_set are reused as they are: an "image" is a frame, all sequences laid end to end
 *   (I = the total number of frames); a group is a (frame, category) pair, g = k*I + f; dt_* are the tracker's boxes (the
 *   hypotheses) and gt_* the annotated ones.  mydet_eval_ious_f64 is called unchanged and gives `ious` (axis-aligned float64, or
 *   the exact rotated IoU).  gt_flags, the areas and the scores are not read here: every ground-truth row counts.
 *   mydet_mot_set adds (DEVICE pointers; the scalars are what the host knows about them):
 *     seq_start           int32 [S + 1], seq_start[0] = 0, seq_start[S] = I: sequence s is frames [seq_start[s], seq_start[s + 1])
 *     a UNIT is one (sequence, category), u = k*S + s, U = S*K units, independent of each other
 *     gt_id, dt_id        int32 [G], [D]: the dense identity index of every row inside its unit, 0 .. n - 1
 *     gt_id_start, dt_id_start   int32 [U + 1]: unit u owns identities [start[u], start[u + 1]) of the Gids = gt_id_start[U]
 *                         (Hids = dt_id_start[U]) global ones
 *     ov_start            int64 [U + 1]: unit u owns nG_u * nH_u entries of an overlap matrix from ov_start[u]; n_ov = ov_start[U]
 *   The packer (mydetection_amd.ops.mot_pack) guarantees that one identity appears at most once per frame on each side.
 *
 * Pair rules, every launch.  Rows are the ground truths of the group and columns its hypotheses, both in stored order.  A pair is
 *   eligible when iou[r, c] >= thr[t], compared in float64; a NaN IoU is never eligible; the threshold is not clamped.  Costs are
 *   integers so that no summation order can change a decision: q = (int64)floor(iou * 65536.0); an eligible pair costs 65536 - q,
 *   an ineligible one BIG = 1 << 27, which exceeds any sum of 1024 eligible costs -- so the minimum-cost assignment first has the
 *   most eligible pairs and then the least cost among those.  Sums are int64.
 *
 * The assignment routine (shared): the shortest-augmenting-path Hungarian method in its textbook u / v / p / way / minv form.
 *   Rows are inserted in ascending order.  Inside an augmentation the next column is the unused column of least minv; a tie goes
 *   to the lowest column index.  If there are more rows than columns the problem is transposed first (the routine's rows are then
 *   the columns).  One wavefront: lanes own columns, a row step is one wave minimum over (minv, column), costs are formed on the fly.
 *
 * mydet_mot_clear_f64: one wavefront per (unit, threshold) walks the unit's frames in order.  State per ground-truth identity o:
 *   last[o], the hypothesis identity of its most recent match (-1 at first; it persists over frames where o is unmatched or
 *   absent); whether o was ever matched; whether o was matched in the previous frame in which it was present.  Per frame:
 *   1. Keep.  Rows ascending: if last[o] >= 0, a column with that identity is in the frame, the pair is eligible and the column
 *      is free, they are matched.
 *   2. Assign.  The routine above on the remaining rows and columns, relative order kept; matches are the assigned pairs that are
 *      eligible.
 *   3. Count matches, rows ascending: TP += 1; SIOU += iou (float64, in this order); IDSW += 1 when last[o] >= 0 and differs from
 *      the column's identity; FRAG += 1 when o was matched before but not in its previous present frame; last[o] = the column's
 *      identity; matched[o] += 1.
 *   4. FN += the unmatched rows; FP += the unmatched columns; present[o] += 1 for every row.
 *   Outputs, every element written: counts int64 [U][T][5] = (TP, FP, FN, IDSW, FRAG); siou float64 [U][T]; present int32 [Gids];
 *   matched int32 [T][Gids]; gt_match (may be NULL) int32 [T][G], the matched hypothesis row (an index into the D rows) or -1.
 *
 * mydet_mot_id_overlap: n[o][h], per unit and threshold, is the number of frames in which both identities are present and their
 *   pair is eligible.  One thread per pair of `ious`; integer atomic adds into int32 matrices in caller scratch, [T][n_ov], which
 *   the call zeroes first (stream-ordered); the result does not depend on order.  mydet_mot_scratch_bytes(mot, T) sizes it.
 * mydet_mot_id_assign: IDTP[u][t] = the largest sum of n[o][h] over one-to-one pairings: the same routine with cost F_u - n, F_u
 *   the unit's frame count, the smaller side on the rows.  Only the optimum value is an output (int64 [U][T]); it is unique even
 *   when the pairing is not.  IDFN = nGT - IDTP and IDFP = nHyp - IDTP are the host's.
 *
 * iou_thrs is a HOST pointer, read before the launch.
 * MYDET_E_BADARG, nothing launched: every mydet_eval_set rule above; a null mot; S < 1 or S > I; a negative count; n_gt_ids > G,
 *   n_dt_ids > D, max_gt_ids > n_gt_ids, max_dt_ids > n_dt_ids, n_ov > n_gt_ids * n_dt_ids; a null seq_start, gt_id_start,
 *   dt_id_start or ov_start; a null gt_id with G > 0 or dt_id with D > 0; T < 1; a null or NaN threshold (clear, overlap); null ious
 *   with n_pairs > 0 (clear, overlap); a null output that would be written; scratch smaller than mydet_mot_scratch_bytes, or null
 *   when that is not 0.
 * MYDET_E_UNSUPP, nothing launched: max_gt > MYDET_EVAL_MAX_GT or max_dt > MYDET_EVAL_MAX_DT (rows of one group); max_gt_ids or
 *   max_dt_ids > MYDET_MOT_MAX_IDS (identities of one unit and side); T > MYDET_EVAL_MAX_THRS.  A frame or a unit whose tables
 *   hold more than was promised is left out by the kernels.
 * Both wavefront kernels keep their state in dynamic LDS: 65 KiB for the CLEAR kernel, above the 64 KiB a kernel gets without the
 *   opt-in and opted into once per device, and 32 KiB for the identity assignment.
 * MYDET_MOT_MAX_IDS is 1024 and not 2048 because of the assignment's worst case, a matrix of ties, in which every inserted row walks
 *   through the columns taken before it: measured on one MI355X (profiles/mot.md), the identity assignment of 2048 x 2048
 *   identities whose overlaps are all 0 or 1 took 9.05 s in one wavefront, that of 1024 x 1024 0.75 s; a 2048 x 2048 problem with
 *   spread overlaps took 32 ms. */
#define MYDET_MOT_MAX_IDS 1024
typedef struct mydet_mot_set {
    int S;                           /* sequences */
    int max_gt_ids, max_dt_ids;      /* the largest identity count of one unit, per side */
    int64_t n_gt_ids, n_dt_ids;      /* Gids = gt_id_start[U], Hids = dt_id_start[U] */
    int64_t n_ov;                    /* ov_start[U] */
    const int32_t *seq_start;
    const int32_t *gt_id, *dt_id;
    const int32_t *gt_id_start, *dt_id_start;
    const int64_t *ov_start;
} mydet_mot_set;
int mydet_mot_clear_f64(const mydet_eval_set *set, const mydet_mot_set *mot, const double *ious, const double *iou_thrs, int T,
                        int64_t *counts, double *siou, int32_t *present, int32_t *matched, int32_t *gt_match, void *stream);
int64_t mydet_mot_scratch_bytes(const mydet_mot_set *mot, int T);
int mydet_mot_id_overlap(const mydet_eval_set *set, const mydet_mot_set *mot, const double *ious, const double *iou_thrs, int T,
                         void *scratch, int64_t scratch_bytes, void *stream);
int mydet_mot_id_assign(const mydet_eval_set *set, const mydet_mot_set *mot, int T, const void *scratch, int64_t scratch_bytes,
                        int64_t *idtp, void *stream);

/* HOTA (Luiten et al., IJCV 2021): detection accuracy (DetA), association accuracy (AssA) and localisation (LocA) per localisation
 * threshold alpha, in three stream-ordered launches (csrc/hota.hip) behind mydet_eval_ious_f64.  The rules are those of TrackEval's
 * hota.py with three changes, made so that no order of evaluation can change a decision: the accumulations are in fixed point,
 * the costs are integers, and the tie rules are stated.  Agreement with TrackEval itself is not claimed; what is claimed, and tested
 * with ==, is the rules below.
 *
 * Data model: exactly that of mydet_mot_set above.  A unit u is one (sequence, category); a group is one frame of one category;
 *   rows are ground truths, columns are hypotheses; a group's IoU block is stored [column][row].  `ious` is the unchanged output of
 *   mydet_eval_ious_f64.  A NaN IoU counts as 0 everywhere below.  Pair values are IoUs, in [0, 1]; a pair whose alignment score
 *   (rule 1) or pair score (rule 2) leaves its range because they are not adds nothing and scores 0.
 *   alphas: a HOST array of T float64 values, each > 0, <= 1 and not NaN.
 *   A frame's assignment carries no state from frame to frame and does not depend on alpha: one assignment per group, every group
 *   of every sequence at once.
 *
 * 1. Alignment (mydet_hota_align_f64).  Per group, in float64, uncontracted: rowsum[r] = the sum of iou over the columns, added
 *    in ascending column order; colsum[c] = the sum of iou over the rows, added in ascending row order.  For a pair,
 *    den = rowsum[r] + colsum[c] - iou, in that order; s = iou / den when iou > 0, else 0.
 *    P[o][h] += (int64)floor(s * 2^30): an int64 atomic add into `pot`, int64 [n_ov], unit u's [nG_u][nH_u] block at ov_start[u]
 *    (o, h: the identities of the row and the column).  gt_count[o] and dt_count[h], int32 [Gids] and [Hids], are the numbers of
 *    frames an identity is present in.  The launch zeroes all three arrays first.  With at most 2^22 frames every integer below
 *    stays under 2^53.
 * 2. Pair score (mydet_hota_match).  A = (double)P / (double)((gt_count[o] + dt_count[h]) * 2^30 - P): one division of two exactly
 *    representable integers; 0 when P is 0.  q = (int32)floor(A * iou * 1048576.0), the product in that order.  score_q, int32
 *    [n_pairs] in the layout of `ious`, is an output.  q is formed once per pair, before the assignment runs.
 * 3. Match (mydet_hota_match).  Per group with both sides non-empty: the minimum-cost assignment with cost 1048576 - q, by the
 *    assignment routine above as it stands: all rows inserted in ascending order, a tie goes to the lowest column, the problem
 *    transposed when rows > columns.  The smaller side is fully assigned.  hota_match int32 [G]: the assigned hypothesis row (an
 *    index into the D rows) or -1; every element is written.
 * 4. Score (mydet_hota_score_f64), per unit and alpha.  A row with hota_match >= 0 and iou >= alpha (float64, no epsilon) is a TP
 *    of that alpha.  counts int64 [U][T][3] = (TP, FN, FP), FN = the unit's rows - TP and FP = the unit's columns - TP.  matches
 *    int32 [T][n_ov]: M[a][o][h] += 1 per TP (the launch zeroes it first).  loc_sum float64 [U][T]: the sum of the TPs' IoUs.
 *    ass_sum float64 [U][T][3], summed over the unit's pairs with M > 0: M * (M / max(1, gt_count + dt_count - M)),
 *    M * (M / max(1, gt_count)), M * (M / max(1, dt_count)): one int-to-double conversion per operand, one division and one
 *    multiplication a term.  The order of the two float64 sums is not part of the rules (the kernel adds per thread in index
 *    order and then by a fixed tree, so a result repeats from run to run); every term is >= 0, so any order is within
 *    (n - 1) * 2^-53 of the exact sum, relatively.
 * The host (mydetection_amd.ops.hota_summarize) sums units into sequence rows and one overall row, as the CLEAR rows are -- not
 *   TrackEval's averaging over classes -- and forms, per alpha, DetA = TP / (TP + FN + FP), DetRe, DetPr, AssA = ass_sum0 /
 *   max(1, TP), AssRe, AssPr, LocA = loc_sum / TP (1 without a TP) and HOTA = sqrt(DetA * AssA).
 *
 * What takes part.  A group with rows and columns that `groups` does not list, a group whose table holds more than the caps, and
 *   every group of a unit whose identity tables hold more than MYDET_MOT_MAX_IDS or reach past n_gt_ids, n_dt_ids or n_ov, is
 *   left out of all four rules: its rows and columns are counted nowhere and its rows keep hota_match -1.  A group with one empty
 *   side needs no listing, as in mydet_mot_clear_f64.
 * MYDET_E_BADARG and MYDET_E_UNSUPP, nothing launched: every rule of the mydet_mot_* launches above, in the same order; null ious
 *   or score_q with n_pairs > 0; a null array that would be read or written; T < 1, a null alphas or an alpha that is not > 0 and
 *   <= 1 (BADARG); T > MYDET_EVAL_MAX_THRS (UNSUPP); I > 2^22 frames (UNSUPP: seq_start is a device array, so the bound on a
 *   sequence is checked on the total).
 * mydet_hota_match keeps the solver's state in 32 KiB of dynamic LDS, which needs no opt-in.  No launch needs scratch memory. */
int mydet_hota_align_f64(const mydet_eval_set *set, const mydet_mot_set *mot, const double *ious, int64_t *pot, int32_t *gt_count,
                         int32_t *dt_count, void *stream);
int mydet_hota_match(const mydet_eval_set *set, const mydet_mot_set *mot, const double *ious, const int64_t *pot,
                     const int32_t *gt_count, const int32_t *dt_count, int32_t *score_q, int32_t *hota_match, void *stream);
int mydet_hota_score_f64(const mydet_eval_set *set, const mydet_mot_set *mot, const double *ious, const int32_t *hota_match,
                         const int32_t *gt_count, const int32_t *dt_count, const double *alphas, int T, int64_t *counts,
                         int32_t *matches, double *loc_sum, double *ass_sum, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MYDET_H */
