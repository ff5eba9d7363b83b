/*
 * dmvs.h -- C ABI of libdmvs_hip.so: the MI355X (gfx950) kernels behind the DiffMVS /
 * CasDiffMVS depth-estimation path.
 *
 * The reference (cvg/diffmvs) has no native layer at all: every entry point
 * below replaces a span of PyTorch ops inside models/module.py / models/update.py, cited
 * per function as  <file>:<lines>  relative to the reference repository root.
 *
 * Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is allocated, freed or
 *     retained by the library; no global state, no environment variables: every choice a caller can make is an argument
 *     or a descriptor field (the `tune` fields: 0 = the measured-best path; the other values exist for A/B measurements
 *     and for tests that pin a code path)  => re-entrant, graph-capturable;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing syncs;
 *   - the return value is 0 on success, a hipError_t otherwise, or DMVS_EINVAL for a
 *     descriptor the library cannot run (unsupported kernel size, channel tile, ...);
 *   - activations are fp32, planar NCHW / NCDHW unless a field says NHWC;
 *   - functions never throw.
 */
#ifndef DMVS_H
#define DMVS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): dmvs_conv2d_desc gained `arith` (round 3, without a bump) and `tune`; dmvs_conv3d_desc gained `tune`;
 * dmvs_featurenet_stem_f32 and dmvs_warp_corr_init_quad_f32 take a trailing `tune` argument; dmvs_conv3x3_pair16_f32 is gone;
 * the library no longer reads any environment variable; dmvs_conv2d_desc also gained `out_mul`, `out_mul_c0` (producer-side output
 * product, SepConvGRU's r * h) and `in0_cstride` (in0 as a channel slice) -- honoured by dmvs_conv2d_f32 only: the weight-gradient entry
 * points return DMVS_EINVAL when any of in0_cstride / gate_cstride / out_mul is set.  A caller built against version 1 passes shorter descriptors:
 * check dmvs_abi_version() == DMVS_ABI_VERSION before the first call. */
#define DMVS_ABI_VERSION 4
#define DMVS_EINVAL (-22)

/* activation codes for the fused epilogues */
enum { DMVS_ACT_NONE = 0, DMVS_ACT_RELU = 1, DMVS_ACT_SIGMOID = 2, DMVS_ACT_TANH = 3, DMVS_ACT_SILU = 4 };
/* how the logical input of a 2-D convolution is read from memory */
enum { DMVS_IN_PLAIN = 0, DMVS_IN_UPSAMPLE2 = 1 /* nearest x2, F.interpolate */, DMVS_IN_UNSHUFFLE2 = 2 /* einops 'b c (h p1) (w p2) -> b (c p1 p2) h w' */,
       DMVS_IN_ZEROINSERT2 = 3 /* logical (2y,2x) = physical (y,x), zero elsewhere: the input-gradient of a stride-2 conv as a stride-1 conv */ };
enum { DMVS_LAYOUT_NCHW = 0, DMVS_LAYOUT_NHWC = 1,
       /* channel-last output stored as 16-bit elements (round to nearest even): the reduced-precision FEATURE storage of
          BASELINE.json's bf16 / fp16 configurations; `out` then points at uint16 elements, strides / offsets count elements */
       DMVS_LAYOUT_NHWC_BF16 = 2, DMVS_LAYOUT_NHWC_F16 = 3 };
/* element type of the image-feature tensors handed to the quad warp kernels */
enum { DMVS_DTYPE_F32 = 0 /* fp32 in the NHWC-g4 channel order (see dmvs_getcost_quad_f32) */, DMVS_DTYPE_BF16 = 1, DMVS_DTYPE_F16 = 2 /* 16-bit, plain NHWC */,
       DMVS_DTYPE_F32_PLAIN = 3 /* fp32, plain NHWC: the training graph's features (its backward kernels read the same order) */ };

int dmvs_abi_version(void);

/* ---------------------------------------------------------------------------------------
 * 2-D convolution with everything around it fused.   Replaces, depending on the fields:
 *   module.Conv2d / ConvBnReLU / ConvBn (conv -> eval BN -> ReLU)      models/module.py:24-58, :279-301
 *   ResidualBlock's relu(x + y)                                        models/module.py:315-319
 *   FeatureNet's  nearest-x2(intra) + inner(conv)                      models/module.py:409-417
 *   ConditionEncoder convs, mask heads (0.25 * conv)                   models/update.py:289-297, :335-339,:473
 *   Unet init_conv / Downsample (pixel-unshuffle + 1x1) / Upsample     models/update.py:38-48, :186, :246
 *   WeightStandardizedConv2d (weights are pre-standardised by caller)  models/update.py:81-94
 *   SepConvGRU gates: z|r = sigmoid(conv[h,x]);  h' = (1-z)h + z*tanh(conv[r*h,x])
 *                                                                      models/module.py:164-177
 * Logical input = concat(in0 (* mul0), in1) along channels, read through `in_mode`.
 * Weight layout: [c0+c1][kh][kw][cout_pad] (cout fastest, zero padded to cout_pad, a
 * multiple of 8).  Epilogue, per output channel co:
 *   y = acc * scale[co] + shift[co]         (scale NULL = 1, shift NULL = 0; folded BN / bias)
 *   y += residual (read through res_mode)   if residual && !res_after_act
 *   y = act(y) * post_scale
 *   y += residual                           if residual &&  res_after_act
 *   y = (1 - gru_z) * gru_h + gru_z * y     if gru_z           (act must be TANH)
 *   y *= out_mul[co - out_mul_c0]           if out_mul && co >= out_mul_c0
 * Output is written at channel offset out_coffset of a tensor with out_cstride channels
 * (so that concatenations never have to be materialised), NCHW or NHWC.
 */
#define DMVS_ARITH_F32 0
#define DMVS_ARITH_BF16 1
#define DMVS_ARITH_SPLIT 2

/* dmvs_conv2d_desc.tune: 0 = the library's own choice (measured best on the MI355X); the bits force a code path for A/B runs.
 * Results do not depend on them (bit-identical kernels). */
#define DMVS_TUNE_TILE_WX(n) ((n) & 3)           /* 1 | 2: 16- / 32-pixel-wide workgroup tiles for the 3x3 / 5x5 layers           */
#define DMVS_TUNE_NO_WALK 0x4                     /* one tile per workgroup everywhere (no resident tile-walking workgroups)        */
#define DMVS_TUNE_PIECES4 0x8                     /* input halo staged in 4-byte LDS-DMA pieces even where 16-byte ones apply        */
#define DMVS_TUNE_TILE_MT(n) (((n) & 7) << 4)     /* A/B: 1 | 2 | 4 = tile height in units of 4 rows (4: plain 3x3 / 1xk families only; timed on the stride-2 / 5x5 / 7x7 ones in round 5: +-2 %, removed) */
#define DMVS_TUNE_1X1_TILED 0x200                 /* 1x1 layers on the LDS-tiled kernel instead of the 16-byte direct form                    */
#define DMVS_TUNE_NO_LEAN 0x100                   /* plain layers on the generic kernel (every fused path resolved at run time)     */
#define DMVS_TUNE_TALL(n) (((n) & 3) << 10)      /* 16 x 32-pixel tiles for the plain 3x3 layers: 0 = where measured better, 1 = never, 2 = wherever they apply (16 x 64 tiles: timed in round 5, 6-8 % slower, removed) */
#define DMVS_TUNE_STEM_EXACT 0x40000             /* dmvs_featurenet_stem_f32: conv0.1 in exact fp32 (0 = split-bf16 arithmetic with fp32 accuracy, the default) */
#define DMVS_TUNE_SPLIT_ALL 0x20000              /* DMVS_ARITH_SPLIT on every layer the form applies to, not only where it measured faster (A/B runs, tests) */
#define DMVS_TUNE_XCD_GROUP(n) (((n) & 7) << 14) /* tiled kernels, one tile per workgroup: which tiles share an XCD's L2.  0 = the library's choice, 1 = plain round robin, 2 | 3 | 4 = groups of 2 | 4 | 8 x-adjacent tiles, 5 = one tile row, 6 = two tile rows, 7 = one image (bit-identical results) */

typedef struct dmvs_conv2d_desc {
    const float* in0;       /* [B,c0,*,*] physical tensor                                   */
    const float* in1;       /* [B,c1,Hin,Win] or NULL; only with DMVS_IN_PLAIN               */
    const float* mul0;      /* [B,c0,Hin,Win] or NULL: in0 is multiplied element-wise       */
    const float* weight;    /* 16-byte aligned (staged in 16-byte pieces); DMVS_EINVAL otherwise */
    const float* scale;
    const float* shift;
    const float* residual;  /* [B,cout,*,*] or NULL                                         */
    const float* gru_z;     /* [B,cout,Hout,Wout] or NULL                                   */
    const float* gru_h;
    float* out;
    double* gn_stats;       /* [B,gn_groups,2] 8-byte slots or NULL (opaque: fixed-point integers, so that the accumulation
                               order of the workgroups cannot change the result -- zero-initialise, hand to
                               dmvs_groupnorm_apply_f32): += per-(b,group) sum and sum of squares of y
                               BEFORE the activation (GroupNorm statistics of the conv output, so
                               that Block.forward needs no separate reduction pass; the caller
                               zeroes the buffer).  gn_groups must be 4 and divide cout.       */
    const float* out_mul;   /* [B, cout - out_mul_c0, Hout, Wout] dense, or NULL: output channels co >= out_mul_c0 are multiplied by
                               out_mul[b, co - out_mul_c0] LAST (after activation, post-scale, residual).  SepConvGRU: the merged z|r
                               gate convolution writes [z | r * h] directly, so that the candidate convolution reads a plain input
                               instead of gating its staged tile (models/module.py:166-168)                                  */
    int32_t B, c0, c1;
    int32_t Hin, Win;       /* LOGICAL input size (after in_mode)                           */
    int32_t Hout, Wout;
    int32_t cout, cout_pad;
    int32_t kh, kw, stride, pad_h, pad_w;
    int32_t in_mode, act;
    int32_t res_mode;       /* DMVS_IN_PLAIN or DMVS_IN_UPSAMPLE2                           */
    int32_t res_after_act;
    int32_t out_layout, out_cstride, out_coffset;
    int32_t gn_groups;
    float post_scale;
    int32_t gate_cstride;   /* 0: mul0 / gru_z are dense [B,c0,..] / [B,cout,..] tensors.  > 0: both are channel slices (the pointers
                               include the channel offset) of tensors with this many channels per batch item -- SepConvGRU's z and
                               r gates computed by ONE convolution with 2x cout (models/module.py:164-177)              */
    int32_t arith;          /* DMVS_ARITH_F32 (0): exact fp32 products (v_mfma_f32_16x16x4_f32), the reference's precision.
                               DMVS_ARITH_BF16 (1): inputs and weights rounded to bf16 (nearest even) as they enter the matrix
                               cores, fp32 accumulation (v_mfma_f32_16x16x32_bf16) -- the reduced-precision configurations of
                               BASELINE.json (configs[2], [4]); tensors in memory stay fp32.  Honoured by stride-1 layers with
                               more than one tap, >= 24 input channels and an NCHW output (where it is faster); every other
                               layer computes in fp32 in either mode.
                               DMVS_ARITH_SPLIT (2): fp32 accuracy on the bf16 matrix cores -- every fp32 operand is split into three
                               bf16 values (hi + mid + lo = x to 2^-27) and a product is the sum of its six partial products down
                               to 2^-18 of it (the dropped ones are below 2^-26), fp32 accumulation.  Honoured by multi-tap layers with an NCHW
                               output on 16-byte aligned rows; the others compute in exact fp32.                           */
    int32_t tune;           /* DMVS_TUNE_* bits, 0 = automatic                                                              */
    int32_t out_mul_c0;     /* first output channel out_mul applies to                                                       */
    int32_t in0_cstride;    /* 0: in0 is a dense [B,c0,..] tensor.  > 0 (DMVS_IN_PLAIN only): in0 is a channel slice (the pointer includes
                               the channel offset) of a tensor with this many channels per batch item                         */
    const void* weight_split; /* ABI 4.  DMVS_ARITH_SPLIT only (else NULL): the layer's weights pre-split into bf16 triples in the matrix
                               cores' operand order, 16-byte aligned: [ceil(cin / 8)][ceil(kh*kw / 4)][3 planes: hi, mid, lo][4][cout_pad][8]
                               bf16 -- element (c, g, p, q, co, j) = part p of the weight of input channel 8c + j, tap 4g + q, output
                               channel co (zero beyond cin / kh*kw / cout); hi = bf16(w), mid = bf16(w - hi), lo = bf16(w - hi - mid),
                               round to nearest even.  A NULL pointer with DMVS_ARITH_SPLIT computes in exact fp32.               */
} dmvs_conv2d_desc;

/* Size limits (DMVS_EINVAL beyond them; the kernels address one batch item with 32-bit element offsets):
 *   (c0 + c1) * Hin * Win < 2^31,  max(cout, out_cstride) * Hout * Wout < 2^31,  Hout * Wout < 2^24,  out_cstride < 2^24. */
int dmvs_conv2d_f32(const dmvs_conv2d_desc* d, void* stream);

/* FeatureNet stem in one kernel: relu(bn1(conv3x3(relu(bn0(conv3x3(x)))))) with 3 -> 8 -> 8 channels, padding 1, at full
 * resolution (models/module.py:364-367 conv0, applied at :399); the 8-channel intermediate never leaves LDS.
 *   x [N,3,H,W], y [N,8,H,W] NCHW;  w0 [3][3][3][8], w1 [8][3][3][8] in the kernel weight layout of dmvs_conv2d_f32
 *   (cout_pad = 8); scale / shift [8] = folded eval BatchNorm (NULL = 1 / 0).  Agrees with the two dmvs_conv2d_f32
 *   launches it replaces to the last bits (different summation grouping of conv0.0's 27 products). */
/* tune: 0 = automatic (input halo in 16-byte LDS-DMA pieces when W % 4 == 0 and x is 16-byte aligned: 1094 -> 938 us per 96
 * images on the MI355X, profiles/r4_optins_ab.jsonl); DMVS_TUNE_PIECES4 = 4-byte pieces (bit-identical results). */
int dmvs_featurenet_stem_f32(const float* x, const float* w0, const float* scale0, const float* shift0, const float* w1,
                             const float* scale1, const float* shift1, float* y, int32_t N, int32_t H, int32_t W, int32_t tune,
                             void* stream);

/* The stem AND conv1.0 in one kernel: relu(bn2(conv5x5 stride 2 (relu(bn1(conv3x3(relu(bn0(conv3x3(x))))))))) with 3 -> 8 -> 8 -> 16 channels,
 * paddings 1, 1, 2 (models/module.py:364-371 conv0 + conv1[0], applied at :399-400); neither 8-channel full-resolution map leaves LDS (a
 * workgroup marches down a strip of 32 output columns with three row rings).  Inference only: nothing else reads conv0's output there.
 *   x [N,3,H,W], y [N,16,H/2,W/2] NCHW;  w0 [3][3][3][8], w1 [8][3][3][8], w2 [8][5][5][16] in the kernel weight layout of dmvs_conv2d_f32;
 *   scale / shift [8] / [8] / [16] = folded eval BatchNorm (NULL = 1 / 0).
 * Arithmetic: conv0.0 exact fp32, conv0.1 and conv1.0 DMVS_ARITH_SPLIT (bf16 triples, six partial products, fp32 accuracy) -- the entry point
 * has no exact-fp32 form: callers that want one launch dmvs_featurenet_stem_f32 + dmvs_conv2d_f32.  Every output depends only on its position
 * in the image (not on N, the grid or the strip a pixel falls into); launches are bit-reproducible.
 * DMVS_EINVAL unless H is even, W a multiple of 4, x 16-byte aligned and 3*H*W < 2^31.  tune: reserved, pass 0. */
int dmvs_featurenet_stem3_f32(const float* x, const float* w0, const float* scale0, const float* shift0, const float* w1,
                              const float* scale1, const float* shift1, const float* w2, const float* scale2, const float* shift2,
                              float* y, int32_t N, int32_t H, int32_t W, int32_t tune, void* stream);

/* FeatureNet conv1.1 + conv1.2 in one kernel: y = relu(bn2(conv3x3(relu(bn1(conv3x3(x)))))) with 16 -> 16 -> 16 channels, stride 1, padding 1
 * (models/module.py:368-371 conv1[1], conv1[2]); the 16-channel intermediate never leaves LDS (a workgroup marches down a strip of 80 output
 * columns with two row rings of bf16 triples; half of its waves run each layer).  Inference only: nothing else reads conv1.1's output there.
 *   x, y [N,16,H,W] NCHW;  wsplit1 / wsplit2 = the layers' weights as dmvs_conv2d_desc.weight_split lays them out (cout_pad = 16:
 *   [2 chunks][3 tap groups][3 planes][4][16][8] bf16); scale / shift [16] = folded eval BatchNorm (NULL = 1 / 0).
 * Arithmetic: DMVS_ARITH_SPLIT in both layers, the same matrix instructions on the same operands in the same order as two dmvs_conv2d_f32
 * launches with arith = DMVS_ARITH_SPLIT: the same bits.  Every output depends only on its position in the image (not on N, the grid or the
 * unit a pixel falls into).  DMVS_EINVAL unless W is a multiple of 4, x / y / the weights are 16-byte aligned and 16*H*W < 2^31.
 * tune: 0 = the grid of the occupancy query; 1 .. 65535 = that many workgroups (tests). */
int dmvs_featurenet_conv1_pair_f32(const float* x, const void* wsplit1, const float* scale1, const float* shift1, const void* wsplit2,
                                   const float* scale2, const float* shift2, float* y, int32_t N, int32_t H, int32_t W, int32_t tune,
                                   void* stream);

/* FeatureNet's FPN tail for stage 2 in one kernel: y = conv3x3(conv1x1(c2) + bias + nearest_up2(c3)) with 32 -> 64 -> 32 channels, the 3x3 with
 * zero padding and no bias / BN / activation (models/module.py:409-411 inner1, out2); the 64-channel sum never leaves LDS (a workgroup marches
 * down a strip of 32 output columns over a four-row ring of bf16 triples).  For networks without an out3: nothing else reads the sum there.
 *   c2 [N,32,H,W], c3 [N,64,H/2,W/2] NCHW;  y [N,H,W,32] channel-last;  w_inner [32][64] = the 1x1 layer's packed weights [cin][cout],
 *   b_inner [64] (NULL = 0);  wsplit_out = the 3x3 layer's weights as dmvs_conv2d_desc.weight_split lays them out (cout_pad = 32:
 *   [8 chunks][3 tap groups][3 planes][4][32][8] bf16; an output-channel permutation such as NHWC-g4 is a permutation of these weights).
 * Arithmetic: the 1x1 in exact fp32, the 3x3 in DMVS_ARITH_SPLIT, the same matrix instructions on the same operands in the same order as the two
 * dmvs_conv2d_f32 launches (residual = c3, res_mode = DMVS_IN_UPSAMPLE2; then out_layout = DMVS_LAYOUT_NHWC, arith = DMVS_ARITH_SPLIT): the
 * same bits.  Every output depends only on its position in the image (not on N, the grid or the unit a pixel falls into).
 * DMVS_EINVAL unless H is even, W a multiple of 8, c2 / c3 / y / wsplit_out are 16-byte aligned and 64*H*W < 2^31.
 * tune: 0 = the grid of the occupancy query; 1 .. 65535 = that many workgroups (tests). */
int dmvs_featurenet_fpn_tail_f32(const float* c2, const float* c3, const float* w_inner, const float* b_inner, const void* wsplit_out,
                                 float* y, int32_t N, int32_t H, int32_t W, int32_t tune, void* stream);

/* Weight (and bias) gradient of the convolution described by `d` (its input side: in0 / in1 / mul0 / in_mode / kh /
 * kw / stride / pad / cout / cout_pad / B / Hin / Win / Hout / Wout; epilogue fields are ignored; in0 / in1 / mul0 must be DENSE tensors:
 * DMVS_EINVAL when in0_cstride, gate_cstride or out_mul is set):
 *   gw[co][ci][ky][kx] = sum_{b,y,x} grad_out[b,co,y,x] * X[b,ci,y*stride+ky-pad,x*stride+kx-pad]     (torch layout)
 *   gb[co]             = sum_{b,y,x} grad_out[b,co,y,x]                                               (gb may be NULL)
 * grad_out [B,cout,Hout,Wout] NCHW.  Every element of gw / gb is written exactly once (no pre-zeroing) and the
 * summation order is fixed: workgroups store per-slot partial sums into `workspace` (caller-owned scratch of at
 * least dmvs_conv2d_wgrad_workspace_f32() bytes) and a second kernel folds the slots -- run-to-run reproducible
 * gradients.  The input gradient needs no entry point of its own: it is dmvs_conv2d_f32 on grad_out with the
 * spatially flipped, cin<->cout transposed weights (DMVS_IN_ZEROINSERT2 for stride 2).
 * d->tune: DMVS_TUNE_PIECES4 = 4-byte staging pieces (A/B; bit-identical); DMVS_TUNE_WGRAD_ACCUMULATE = the fold kernel ADDS its sums to gw /
 * gb instead of storing them (the caller's running gradient of a weight that several layers of a step share: one read-modify-write
 * per element instead of a store here + an add kernel elsewhere; the order of the additions is the order of the calls on the stream). */
#define DMVS_TUNE_WGRAD_ACCUMULATE 0x1000
int dmvs_conv2d_wgrad_workspace_f32(const dmvs_conv2d_desc* d, int64_t* bytes);
int dmvs_conv2d_wgrad_f32(const dmvs_conv2d_desc* d, const float* grad_out, float* gw, float* gb, float* workspace,
                          int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * 3-D convolution 3x3x3, padding 1 (module.Conv3d, models/module.py:66-102) and stride-2
 * transposed convolution with output_padding 1 (module.Deconv3d, :110-144, :436-437), with
 * eval-BN folded into scale/shift, optional ReLU and an optional post-activation residual
 * (CostRegNet_small skip adds, models/module.py:445-446).
 * Weight layout: [cin][27][cout_pad].  For transposed convs the caller passes the weight of
 * the equivalent gather form: w[ci][kd][kh][kw][co] = W_torch[ci][co][kd][kh][kw].
 */
typedef struct dmvs_conv3d_desc {
    const float* in;        /* [B,cin,Din,Hin,Win]                                          */
    const float* weight;    /* 16-byte aligned (staged in 16-byte pieces); DMVS_EINVAL otherwise */
    const float* scale;
    const float* shift;
    const float* residual;  /* [B,cout,Dout,Hout,Wout] or NULL, added after the activation  */
    float* out;             /* [B,cout,Dout,Hout,Wout]                                      */
    int32_t B, cin, cout, cout_pad;
    int32_t Din, Hin, Win;
    int32_t Dout, Hout, Wout;
    int32_t stride;         /* 1 or 2                                                       */
    int32_t transposed;     /* 0 | 1 (stride must be 2)                                     */
    int32_t act;
    int32_t tune;           /* 0 = automatic; DMVS_TUNE3D_* bits force a code path (A/B runs; bit-identical results except
                               DMVS_TUNE3D_S2_DIRECT, whose summation order is the direct kernel's)                        */
} dmvs_conv3d_desc;
#define DMVS_TUNE3D_PIECES4 0x1       /* stride-1 MFMA kernels: halo tile in 4-byte LDS-DMA pieces even where 16-byte ones apply  */
#define DMVS_TUNE3D_S2_DIRECT 0x2     /* stride-2 layers on the direct (VALU) kernels of round 1 instead of the matrix cores      */
#define DMVS_TUNE3D_NO_PAIR 0x4       /* A/B: the <= 8 -> <= 8 channel stride-1 layers on the generic / streamed kernels instead of the paired ones (two output depth
                                         slices per MFMA; bit-identical results; round 5: PixelViewWeight conv0 -5 %, CostRegNet conv1 1517 -> 983 us per 96 volumes) */
#define DMVS_TUNE3D_XCD_GROUP(n) (((n) & 7) << 4) /* tiled 3-D kernels: which tiles share an XCD's L2.  0 = groups of 4 x-adjacent tiles (the default), 1 = plain round robin, 2 | 3 | 4 = groups of 2 | 4 | 8 (bit-identical results) */

/* Size limit of the stride-1 layers (DMVS_EINVAL beyond): cin * Din*Hin*Win < 2^31 and cout * Dout*Hout*Wout < 2^31
 * (one batch item is addressed with 32-bit element offsets). */
int dmvs_conv3d_f32(const dmvs_conv3d_desc* d, void* stream);

/* Weight (and bias) gradient of the (non-transposed, stride 1|2) 3x3x3 convolution described by `d`:
 *   gw[co][ci][27] = sum_{b,voxel} grad_out[b,co,voxel] * in[b,ci,voxel*stride - 1 + tap]      (torch layout)
 *   gb[co]         = sum_{b,voxel} grad_out[b,co,voxel]                                          (gb may be NULL)
 * Written once, fixed summation order, via caller-owned `workspace` as for dmvs_conv2d_wgrad_f32.
 * The transposed layers use the same entry point with the roles of `in` and `grad_out` swapped.  Input gradients
 * need no entry point: stride 1 = dmvs_conv3d_f32 on flipped/transposed weights, stride 2 <-> transposed. */
int dmvs_conv3d_wgrad_workspace_f32(const dmvs_conv3d_desc* d, int64_t* bytes);
int dmvs_conv3d_wgrad_f32(const dmvs_conv3d_desc* d, const float* grad_out, float* gw, float* gb, float* workspace,
                          int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Camera composition.  For each batch item b and source view s = 1..S:
 *   P = (K_s E_s[:3,:4] | 0001) * inverse(K_0 E_0[:3,:4] | 0001)   models/module.py:188, :520-525
 * proj: [B,V,2,4,4] (V = S+1; [:, :, 0] extrinsic, [:, :, 1, :3, :3] intrinsic).
 * out:  [B,S,12]  = rot (row-major 3x3) followed by trans (3).  Computed in fp64 from the
 * fp32 inputs and rounded once.
 */
int dmvs_compose_proj_f32(const float* proj, float* out, int32_t B, int32_t V, void* stream);

/* ---------------------------------------------------------------------------------------
 * The two fused warp kernels ("quad per pixel", warp_quad.hip): any geometry in ONE launch.
 *
 * dmvs_warp_corr_init_quad_f32 -- plane-sweep group-wise correlation volumes for depth initialisation: differentiable_warping
 * (models/module.py:181-218) + the group-wise correlation of InitialCost.forward (:514-531) for ALL source views; the hypotheses
 * are uniform in normalised inverse depth (models/diffusion.py:187-192) and generated in-kernel:
 *   depth_d = 1 / clamp(1/dmax + (1/dmin - 1/dmax) * d/(D-1), 1e-6).
 *   ref  [B,H,W,C]   src  [S][B,Hs,Ws,C] channel-last, contiguous over S     rt [B,S,12] from dmvs_compose_proj_f32
 *   disp_min/disp_max [B] (= depth_values[:,0], depth_values[:,-1])           out [B,S,G,D,H,W], cor[g] = mean over the group's channels
 *   C in {16,32,48}, G = 4.
 *
 * dmvs_getcost_quad_f32 -- GetCost.forward (models/module.py:583-667): hypothesis generation (get_cur_depth_range_samples :250-277 +
 * disp_to_depth :220-227), S homography warps, group-wise correlation and view-weighted aggregation
 * sum_s w_s cor_s / (1e-8 + sum_s w_s).
 *   inv_depth  [B,1,H,W] normalised inverse depth      confidence [B,H,W] or NULL
 *   view_w     [B,S,H>>vw_shift,W>>vw_shift]  (nearest-upsampled on the fly, models/diffusion.py:219-221)
 *   out_cost   [B,G*n,H,W]  written at channel offset cost_coffset of a tensor with cost_cstride channels; out_samples [B,n,H,W] likewise
 *   n in {4,6}; interval = depth_interval * ratio (models/diffusion.py:246).
 *
 * (Round 1's LDS-window / per-pixel-gather forward kernels -- dmvs_getcost_f32, dmvs_getcost_gather_f32, dmvs_warp_corr_init_f32,
 * dmvs_warp_corr_init_gather_f32 -- were retired in round 4 / ABI 2: the training graph runs the quad kernels too, on
 * DMVS_DTYPE_F32_PLAIN features.  `worklist` remains for the BACKWARD's hybrid window / per-pixel launch, dmvs_getcost_bwd_f32.)
 */
#define DMVS_GETCOST_TILE 16
#define DMVS_GETCOST_MAX_WINDOW_VIEWS 16      /* more source views than this: dmvs_getcost_bwd_f32 takes the per-pixel path */
#define DMVS_GETCOST_WORKLIST_INTS(B, H, W) \
    (4 + 66 * (B) * (((H) + DMVS_GETCOST_TILE - 1) / DMVS_GETCOST_TILE) * (((W) + DMVS_GETCOST_TILE - 1) / DMVS_GETCOST_TILE))
typedef struct dmvs_getcost_desc {
    const float* ref;       /* [B,H,W,C] channel-last (16-bit elements behind the pointer for feat_dtype BF16 / F16) */
    const float* src;       /* [S][B,H,W,C] NHWC */
    const float* rt;        /* [B,S,12] */
    const float* inv_depth;
    const float* confidence;
    const float* view_w;
    const float* disp_min;  /* [B] */
    const float* disp_max;  /* [B] */
    float* out_cost;
    float* out_samples;
    int32_t* worklist;      /* dmvs_getcost_bwd_f32 only: scratch of DMVS_GETCOST_WORKLIST_INTS(B,H,W) ints (per-tile fit flags, the list of
                               tiles left to the per-pixel kernel, per-view window boxes), or NULL = per-pixel kernel everywhere */
    int32_t B, S, C, G, n, H, W;
    int32_t vw_shift;
    int32_t cost_cstride, cost_coffset, samp_cstride, samp_coffset;
    float interval, min_radius, max_radius;
    int32_t feat_dtype;     /* DMVS_DTYPE_*: element type / channel order of ref / src (the backward reads plain fp32 NHWC) */
    int32_t tune;           /* ABI 3.  dmvs_getcost_bwd_f32: DMVS_TUNE_BWD_* (0 = default); the forward ignores it */
} dmvs_getcost_desc;

/* ---------------------------------------------------------------------------------------
 * Feature layouts of the quad kernels.  feat_dtype = DMVS_DTYPE_F32: `ref` / `src` are read in the GROUP-INTERLEAVED channel-last layout
 * "NHWC-g4": a texel is C/16 units of 16 floats, unit j = [ch 4j..4j+3 of group 0 | of group 1 | of group 2 | of group 3]
 * (group g = channels g*C/4 .. (g+1)*C/4 - 1 of the reference's NCHW tensor), i.e.
 *     position p of a texel holds channel  c(p) = ((p / 4) % 4) * (C / 4) + (p / 16) * 4 + p % 4,
 * so that the 4 lanes of a pixel fetch 64 contiguous bytes and each receives channels of its own correlation group.
 * The inference engine has FeatureNet's output convolutions emit this layout directly (output-channel permutation of
 * their weights); diffmvs_amd.ops.g4_channels(C) is the permutation for callers that hold plain NHWC tensors.
 * Reduced-precision feature storage (BASELINE.json's bf16 / fp16 configurations): feat_dtype = DMVS_DTYPE_BF16 | _F16 reads ref /
 * src as 16-bit elements in PLAIN NHWC order (a group's C/4 channels are then contiguous already: 8 / 16 / 24 bytes per lane);
 * values are widened to fp32 on arrival, projection, hypotheses, correlation and accumulation stay fp32.
 * DMVS_DTYPE_F32_PLAIN: fp32 in plain NHWC order (what the training graph holds and its backward kernels read). */
/* tune (plane sweep): 0 = the source band of a 16 x 4 pixel tile is staged in LDS (warp_init_band_kernel);
 * DMVS_TUNE_SWEEP_GLOBAL = every texel from global memory (warp_init_quad_kernel, the round-2 form; bit-identical results). */
#define DMVS_TUNE_SWEEP_GLOBAL 0x1
int dmvs_getcost_quad_f32(const dmvs_getcost_desc* d, void* stream);
int dmvs_warp_corr_init_quad_f32(const void* ref, const void* src, const float* rt,
                                 const float* disp_min, const float* disp_max, float* out,
                                 int32_t B, int32_t S, int32_t C, int32_t G, int32_t D,
                                 int32_t H, int32_t W, int32_t Hs, int32_t Ws, int32_t feat_dtype, int32_t tune, void* stream);

/* Stand-alone differentiable_warping (models/module.py:181-218) in the reference's layouts:
 * src [B,C,Hs,Ws] NCHW, rt [B,12] (rot row-major, trans) = src_proj * inverse(ref_proj),
 * depth [B,D,H,W] metric -> out [B,C,D,H,W].  Not used by the model's fused path. */
int dmvs_warp_volume_f32(const float* src, const float* rt, const float* depth, float* out,
                         int32_t B, int32_t C, int32_t D, int32_t H, int32_t W, int32_t Hs, int32_t Ws,
                         void* stream);

/* ---------------------------------------------------------------------------------------
 * Training step: backward of the fused warp / correlation kernels w.r.t. the image features (the
 * reference builds the sampling grid under no_grad and detaches hypotheses and GetCost's view
 * weights: models/module.py:187, :573, models/update.py:442-445).
 *   gref [B,H,W,C] is WRITTEN; gsrc [S][B,Hs,Ws,C] is ACCUMULATED with fp32 atomics (caller zeroes it,
 *   or passes the running gradient of the source features).
 */
/* Channel -> lane mapping of the per-pixel scatter kernels.  Default: a lane owns CONSECUTIVE channels (16-byte loads; each atomic
 * instruction of a flush touches 4 bytes out of every 16 of the texel).  DMVS_TUNE_BWD_INTERLEAVED (dmvs_getcost_desc.tune) /
 * gather = DMVS_BWD_GATHER_INTERLEAVED: 16 lanes per pixel, lane = channel mod 16 -- an atomic instruction covers 64 contiguous bytes of the
 * texel, C*4/64 full requests per (pixel, tap) at the L2's atomic units instead of 4x as many quarter-filled ones.  Same sums in the same
 * per-lane order; the two mappings differ only in how atomics from different pixels interleave (last-bit differences, as between any two runs). */
#define DMVS_TUNE_BWD_INTERLEAVED 0x1
#define DMVS_BWD_GATHER_INTERLEAVED 2
/* gather != 0: per-pixel atomics kernel only (1: consecutive channels per lane, 2: interleaved); 0: LDS-window kernel for C = 48 (the model's stage 1) */
int dmvs_warp_corr_init_bwd_f32(const float* ref, const float* src, const float* rt,
                                const float* disp_min, const float* disp_max, const float* gcor,
                                float* gref, float* gsrc, int32_t B, int32_t S, int32_t C, int32_t G,
                                int32_t D, int32_t H, int32_t W, int32_t Hs, int32_t Ws, int32_t gather, void* stream);
/* gcost [B,G*n,H,W] contiguous; d->out_cost / out_samples / feat_dtype are ignored (features: plain fp32 NHWC).  With d->worklist the
 * LDS-window kernel takes the 16x16 tiles whose source footprints fit its windows (C = 32 | 16) and the per-pixel kernel the rest. */
int dmvs_getcost_bwd_f32(const dmvs_getcost_desc* d, const float* gcost, float* gref, float* gsrc, void* stream);
/* backward of dmvs_view_aggregate_f32 (InitialCost, where the view weights DO require grad, :539-548):
 * gcor [B,S,GD,HW], gw [B,S,HW] are written */
int dmvs_view_aggregate_bwd_f32(const float* cor, const float* w, const float* out, const float* gout,
                                float* gcor, float* gw, int32_t B, int32_t S, int32_t GD, int32_t HW,
                                void* stream);

/* view-weighted aggregation of the per-view volumes (models/module.py:539-548):
 * out[b,g,d,p] = sum_s w[b,s,p] cor[b,s,g,d,p] / (1e-8 + sum_s w[b,s,p]) */
int dmvs_view_aggregate_f32(const float* cor, const float* w, float* out,
                            int32_t B, int32_t S, int32_t GD, int32_t HW, void* stream);

/* PixelViewWeight tail (models/module.py:460-463): out[n,p] = max_d sigmoid(x[n,d,p]) */
int dmvs_sigmoid_max_d_f32(const float* x, float* out, int32_t N, int32_t D, int32_t HW, void* stream);

/* InitialCost epilogue (models/module.py:553-571): softmax over D, expectation index,
 * normalised depth index/(D-1), metric depth via disp_to_depth, photometric confidence =
 * sum of the 4 probabilities d-1..d+2 around floor(index).
 *   logits [B,D,HW] -> norm_depth [B,HW], depth [B,HW], conf [B,HW] */
int dmvs_depth_regress_f32(const float* logits, const float* disp_min, const float* disp_max,
                           float* norm_depth, float* depth, float* conf,
                           int32_t B, int32_t D, int32_t HW, void* stream);

/* upsample_depth (models/module.py:237-248) fused with disp_to_depth (:220-227):
 * convex combination of the 3x3 neighbourhood with softmax(mask) weights.
 *   inv [B,H,W], mask [B,9*r*r,H,W] -> out_inv [B,rH,rW] (may be NULL), out_depth [B,rH,rW] */
int dmvs_convex_upsample_f32(const float* inv, const float* mask, const float* disp_min,
                             const float* disp_max, float* out_inv, float* out_depth,
                             int32_t B, int32_t H, int32_t W, int32_t ratio, void* stream);

/* The mask head's last layer + upsample_depth in one launch (DiffMVS, ratio 4): logits = post_scale * (W x + bias) -- the 1x1 convolution
 * 64 -> 144 of models/update.py:335-339 with `mask = .25 * self.mask(context)` (:473) -- then upsample_depth (models/module.py:237-248)
 * and disp_to_depth (:220-227) exactly as dmvs_convex_upsample_f32; the 144-channel mask is never written to memory.  Results are those
 * of dmvs_conv2d_f32 followed by dmvs_convex_upsample_f32 bit for bit.
 *   x [B,64,H,W] (the ReLU output of the head's 3x3 layer), weight [64][1][144] (kernel layout), bias [144] or NULL, inv [B,H,W]
 *   -> out_inv [B,4H,4W] (may be NULL), out_depth [B,4H,4W] (may be NULL; not both).  cin must be 64 and cout_pad 144 (DMVS_EINVAL otherwise:
 *   other ratios / widths take the two entry points). */
int dmvs_mask_upsample4_f32(const float* x, const float* weight, const float* bias, float post_scale, const float* inv,
                            const float* disp_min, const float* disp_max, float* out_inv, float* out_depth,
                            int32_t B, int32_t cin, int32_t cout_pad, int32_t H, int32_t W, void* stream);

/* GroupNorm statistics + fused apply of Block.forward (models/update.py:124-133):
 *   y = silu( gn(x) * (scale+1) + shift ) [+ residual]
 * x [B,C,HW]; gamma,beta [C]; scale_shift [B,2C] (scale then shift) or NULL; residual or NULL.
 * stats: caller-provided scratch of B*groups*2 8-byte slots (opaque, see gn_stats above).  In-place (y == x) is allowed. */
int dmvs_groupnorm_silu_f32(const float* x, const float* gamma, const float* beta,
                            const float* scale_shift, const float* residual, float* y,
                            double* stats, int32_t B, int32_t C, int32_t HW, int32_t groups,
                            float eps, void* stream);

/* The apply half alone, for statistics that were accumulated by dmvs_conv2d_f32 (gn_stats). */
int dmvs_groupnorm_apply_f32(const float* x, const float* gamma, const float* beta,
                             const float* scale_shift, const float* residual, float* y,
                             const double* stats, int32_t B, int32_t C, int32_t HW, int32_t groups,
                             float eps, void* stream);

/* Refinement bookkeeping (models/update.py:479-483, :496-502):
 *   new = clamp(inv + delta_in (+ update), 0, 1);  delta_out = new - inv
 * update may be NULL (first step: delta_in = scale * noise).  `new` is written with channel
 * stride/offset so that it can land directly inside the Unet input tensor. */
int dmvs_delta_update_f32(const float* inv, const float* delta_in, const float* update,
                          float delta_in_scale, float* delta_out, float* new_inv,
                          float* new_inv2, int32_t new2_cstride, int32_t new2_coffset,
                          int32_t B, int32_t HW, void* stream);

/* element-wise helpers:  depth <-> normalised inverse depth (models/module.py:220-235),
 * activations on a channel slice, nearest upsampling by an integer factor. */
enum { DMVS_EW_DEPTH_TO_DISP = 0, DMVS_EW_DISP_TO_DEPTH = 1 };
int dmvs_depth_convert_f32(const float* in, const float* disp_min, const float* disp_max,
                           float* out, int32_t mode, int32_t B, int32_t HW, void* stream);
/* out[b, out_coffset + c, p] = act(in[b, in_coffset + c, p]) for c < C */
int dmvs_act_slice_f32(const float* in, float* out, int32_t act, int32_t B, int32_t C, int32_t HW,
                       int32_t in_cstride, int32_t in_coffset, int32_t out_cstride, int32_t out_coffset,
                       void* stream);
int dmvs_upsample_nearest_f32(const float* in, float* out, int32_t N, int32_t H, int32_t W,
                              int32_t factor, void* stream);
/* Backward of dmvs_groupnorm_silu_f32 without the residual (Block.forward in training, models/update.py:124-133):
 * `stats` [B*groups*2] doubles as left by the forward; dx [B,C,HW]; dgamma / dbeta [C]; dscale_shift [B,2C] (required when
 * scale_shift is given); `workspace`: caller scratch of dmvs_groupnorm_silu_bwd_workspace_f32() bytes.  No atomics. */
int dmvs_groupnorm_silu_bwd_workspace_f32(int32_t B, int32_t C, int32_t HW, int64_t* bytes);
int dmvs_groupnorm_silu_bwd_f32(const float* x, const float* dy, const float* gamma, const float* beta, const float* scale_shift,
                                const double* stats, float* dx, float* dgamma, float* dbeta, float* dscale_shift,
                                float* workspace, int64_t workspace_bytes, int32_t B, int32_t C, int32_t HW, int32_t groups,
                                float eps, void* stream);

/* ---------------------------------------------------------------------------------------
 * Training-mode BatchNorm (+ optional ReLU) on [B, C, S] fp32 (S = H*W or D*H*W).  Replaces nn.BatchNorm2d/3d in
 * train mode inside module.Conv2d / Conv3d / ConvBnReLU / ConvBn            models/module.py:24-58, :60-96, :279-301.
 *   fwd: mean/var over (rows of the view, S) per channel (biased var for the normalisation),
 *        y = act((x-mean)*rstd*gamma+beta); running_mean/var (may both be NULL) <- (1-momentum)*running +
 *        momentum*(mean | unbiased var), once per view in view order; save_mean / save_rstd [views][C] for the backward.
 *   bwd: dz = dy * [y > 0 if act == RELU];  per view dbeta_v = sum dz, dgamma_v = sum dz*xhat,
 *        dx = gamma*rstd*(dz - dbeta_v/N - xhat*dgamma_v/N), N = (B/views)*S;  dgamma / dbeta [C] = sums over views.
 * `views` (B % views == 0) batches that many independent BatchNorm calls: the reference runs FeatureNet once per image
 * of the view stack and PixelViewWeight once per source view (diffusion.py:156-157, module.py:533); row b belongs to
 * view b / (B/views) if view_major, else b % views.  act in {DMVS_ACT_NONE, DMVS_ACT_RELU}; x / y / dy / dx 16-byte
 * aligned; `workspace`: caller-owned scratch of dmvs_batchnorm_workspace_f32() bytes (per-chunk partial sums folded
 * in double, no atomics). */
int dmvs_batchnorm_workspace_f32(int32_t B, int32_t C, int32_t S, int32_t views, int64_t* bytes);
int dmvs_batchnorm_train_fwd_f32(const float* x, const float* gamma, const float* beta, float* running_mean,
                                 float* running_var, float* y, float* save_mean, float* save_rstd, float* workspace,
                                 int64_t workspace_bytes, int32_t B, int32_t C, int32_t S, int32_t views, int32_t view_major,
                                 float momentum, float eps, int32_t act, void* stream);
int dmvs_batchnorm_train_bwd_f32(const float* x, const float* dy, const float* gamma, const float* beta,
                                 const float* save_mean, const float* save_rstd, float* dx, float* dgamma, float* dbeta,
                                 float* workspace, int64_t workspace_bytes, int32_t B, int32_t C, int32_t S, int32_t views,
                                 int32_t view_major, int32_t act, void* stream);

/* ---------------------------------------------------------------------------------------
 * Depth-map fusion: geometric consistency of one reference depth map against S source depth maps (reference
 * filter.py:8-93 reproject_with_depth + check_geometric_consistency, :230-259 the dynamic variant).  Per reference pixel and
 * source view: reference depth -> source pixel -> source depth sampled like cv2.remap(INTER_LINEAR, constant 0 border,
 * 1/32-pixel coordinate quantisation) -> back into the reference view; level l accepts the pair when
 *     reprojection distance < pix_thres[l]  and  |depth_reproj - depth_ref| / depth_ref < rel_thres[l]
 *     (and, if use_range, range_min < depth_ref < range_max -- filter.py:89).
 *   depth_ref [H,W], depth_src [S,Hs,Ws] fp32
 *   mats [S][DMVS_GEO_MATS_FLOATS] fp32, per source view row-major: inv(K_ref) 3x3 | (E_src inv(E_ref))[:3,:4] |
 *        K_src 3x3 | inv(K_src) 3x3 | (E_ref inv(E_src))[:3,:4] | K_ref 3x3, composed by the caller in fp32 as the
 *        reference's np.linalg.inv / np.matmul on its fp32 camera files do
 *   level_counts [L,H,W] int32: number of source views accepted at level l;  depth_sum [H,W]: sum over the views accepted
 *        at the LAST level of the reprojected depth (filter.py:91, :257), accumulated in view order in fp32.
 * L = 1 is filter_depth (DTU / ETH3D), L = 11 - dh_view_num the Tanks&Temples dynamic check. */
#define DMVS_GEO_MATS_FLOATS 60
#define DMVS_GEO_MAX_LEVELS 12
int dmvs_geo_consistency_f32(const float* depth_ref, const float* depth_src, const float* mats, const double* pix_thres,
                             const float* rel_thres, int32_t L, int32_t use_range, float range_min, float range_max,
                             int32_t* level_counts, float* depth_sum, int32_t S, int32_t H, int32_t W, int32_t Hs, int32_t Ws,
                             void* stream);

/* ---------------------------------------------------------------------------------------
 * Training-step tail on one flat fp32 parameter bucket (the buffer RCCL all-reduces).  Replaces
 * torch.nn.utils.clip_grad_norm_(model.parameters(), 2.0) + AdamW.step()   train.py:200-203, :321-326.
 * dmvs_sumsq_f32: *out (a device double) = sum g[i]^2;  `g` must be 16-byte aligned.
 * dmvs_adamw_step_f32: g' = g * grad_scale (1/world_size of the data-parallel average), further scaled by
 *   min(1, max_norm / (grad_scale*sqrt(*sumsq) + 1e-6)) when sumsq != NULL; decoupled weight decay,
 *   bias correction with `step` (1-based), as torch.optim.AdamW(amsgrad=False). */
int dmvs_sumsq_f32(const float* g, int64_t n, double* out, void* stream);
int dmvs_adamw_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int32_t step, float grad_scale,
                        const double* sumsq, float max_norm, void* stream);
/* NCHW -> NHWC for features that did not come out of dmvs_conv2d_f32 channel-last */
int dmvs_nchw_to_nhwc_f32(const float* in, float* out, int32_t B, int32_t C, int32_t HW, void* stream);

/* ---------------------------------------------------------------------------------------
 * View selection of the COLMAP import (added under ABI 4, additive: no existing descriptor or arity changed).  Replaces
 * colmap_input.py:374-390 calc_score for every image pair at once.  Images are numbered by their position in images.bin.
 *   xyz [P,3] fp64: the points;  centres [N,3] fp64: camera centres -R^T t
 *   point -> image CSR built from the images' point3D_ids lists (entries of -1 dropped): offsets [P+1] int64, images [E] int32
 *        ascending and unique within a point, mult [E] int32 = how often that image lists the point
 *   pair_offsets [P+1] int64: exclusive prefix sum of L_p (L_p - 1) / 2, L_p = offsets[p+1] - offsets[p];  terms = pair_offsets[P]
 *   workspace: N (N - 1) / 2 uint64 (the fixed-point upper triangle), zeroed here;  score [N,N] fp64: symmetric, zero diagonal.
 * Pair (i, j), i < j, scores sum over points seen by both of mult_i * exp(-(th - theta0)^2 / (2 s^2)), s = sigma1 if th <= theta0
 * else sigma2, th = degrees(acos(dot(c_i - p, c_j - p) / |c_i - p| / |c_j - p|)) in fp64: the reference counts a point once per
 * entry in the LOWER-indexed image's list.  Two deviations from the reference: the cosine is clamped to [-1, 1] (the reference
 * gives NaN when it rounds past), and a point at a camera centre contributes 0 (the reference divides by zero).
 * Terms are summed as max(1, round(f 2^40)) (f > 0) in uint64 with integer atomics: the result is bitwise independent of launch order and shape.
 * The caller keeps every image's total multiplicity below DMVS_VIEW_SELECT_MAX_LIST (no overflow of the fixed point).
 * DMVS_EINVAL: N outside [1, DMVS_VIEW_SELECT_MAX_IMAGES], sigma <= 0, NULL operands. */
#define DMVS_VIEW_SELECT_MAX_IMAGES 16384
#define DMVS_VIEW_SELECT_MAX_LIST (1 << 23)
int dmvs_view_select_scores_f64(const double* xyz, const int64_t* offsets, const int32_t* images, const int32_t* mult,
                                const int64_t* pair_offsets, int64_t P, int64_t terms, const double* centres, int32_t N,
                                double theta0, double sigma1, double sigma2, uint64_t* workspace, double* score, void* stream);

/* ---------------------------------------------------------------------------------------
 * Point-cloud scoring (added under ABI 4, additive): the nearest-neighbour searches of the DTU / Tanks&Temples / ETH3D scorers and the
 * reduction of their distances (diffmvs_amd/cloud_eval.py builds the grid and the metrics).
 *
 * dmvs_cloud_nn_dist_f32: dist[i] = min(|query_i - nearest target|, max_dist), fp32 (differences, squares, root; no contraction).
 *   query [Q,3] fp32;  target [M,3] fp32 SORTED by cell key;  dist [Q] fp32;  work: NULL or [Q,2] int32 (rings walked, targets tested)
 *   the grid: origin (HOST, 3 doubles), cell side h, dims (HOST, 3 int32: cells along x, y, z, each >= 1).  A point's cell is
 *        floor(((double)p - origin) / h) per axis in fp64, clamped to the grid for queries;  key = (z << (bx + by)) | (y << bx) | x with
 *        bx / by = the number of bits that hold dims[0] - 1 / dims[1] - 1
 *   cell_keys [C] int64: the occupied cells, ascending and unique;  cell_start [C+1] int64: first target of each cell, cell_start[C] = M
 *   (all three device arrays; every target's cell lies inside dims).
 * One lane per query walks rings of slabs z = cz -+ r, the occupied rows of a slab and the occupied cells of a row outward, each found by
 * a binary search in cell_keys, and stops a direction when the gap to it cannot beat the best distance so far (csrc/cloud_eval.hip).  The
 * result is the minimum over all targets of the fp32 squared distance, whatever h is; M = 0 gives max_dist everywhere.
 * Worst case (2R + 1)^2 rows per query, R = ceil(max_dist / h): the caller keeps R small by raising h.
 * DMVS_EINVAL (before any launch): NULL operands, Q / M / C < 0, C > M, h or max_dist not finite or <= 0, a non-finite origin, dims < 1,
 * R > DMVS_CLOUD_MAX_RINGS, a grid whose key needs more than DMVS_CLOUD_MAX_KEY_BITS bits.
 *
 * dmvs_cloud_stats_f32: out [3 + T] uint64 (device, zeroed here) = { valid points, those with d < max_dist, their sum as fixed point
 *   (each term rint((double)d * scale)), then per threshold the valid points with d < thresholds[t] }.
 *   dist [N] fp32;  valid: NULL (all) or [N] uint8;  thresholds: HOST array of T <= DMVS_CLOUD_MAX_THRESHOLDS floats
 *   scale: a positive power of two with max_dist * scale * max(N, 1) < 2^62 (the sum cannot overflow; a term is rounded by at most 0.5 / scale)
 *   blocks: workgroups of the grid-stride launch, 0 = the library's choice (the result does not depend on it).
 * Wave shuffles, then one integer atomic per counter per workgroup: bitwise independent of launch order and shape.
 * DMVS_EINVAL: NULL operands, N < 0, T outside [0, 16], a NaN threshold, max_dist not finite or <= 0, scale not a power of two or beyond the bound. */
#define DMVS_CLOUD_MAX_RINGS 1024
#define DMVS_CLOUD_MAX_KEY_BITS 62
#define DMVS_CLOUD_MAX_THRESHOLDS 16
int dmvs_cloud_nn_dist_f32(const float* query, int64_t Q, const float* target, int64_t M, const int64_t* cell_keys,
                           const int64_t* cell_start, int64_t C, const double* origin, double h, const int32_t* dims,
                           float max_dist, float* dist, int32_t* work, void* stream);
int dmvs_cloud_stats_f32(const float* dist, const uint8_t* valid, int64_t N, float max_dist, const float* thresholds, int32_t T,
                         double scale, int32_t blocks, uint64_t* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Point-cloud registration and cropping (added under ABI 4, additive; diffmvs_amd/cloud_register.py runs ICP on them).
 *
 * `transform` (all three): a HOST pointer to a row-major 3x4 [sR | t], NULL = identity.  The moved point is
 *   p' = fp32(((m0 x + m1 y) + m2 z) + m3) per row: products and sums in fp64 in this order, no contraction, ONE rounding to fp32.
 *
 * dmvs_cloud_nn_index_f32: dmvs_cloud_nn_dist_f32 (same grid operands, same walk) that moves the query first and also says WHICH target
 *   is the nearest.  dist: NULL or [Q] fp32, bit-identical to dmvs_cloud_nn_dist_f32 called on q', for any cell size.
 *   index [Q] int32: the position in the SORTED target array of a target at distance dist[i] -- dist[i] is, bit for bit, the fp32
 *   distance (same operation order) between q'_i and target[index[i]] -- or -1 where dist[i] == max_dist (nothing closer than max_dist).
 *   Between exactly equidistant targets (equal fp32 squared distances) ANY one of them may be returned: which one depends on the walk
 *   order, hence on the cell size.  work as in dmvs_cloud_nn_dist_f32.
 *   DMVS_EINVAL: as dmvs_cloud_nn_dist_f32 (dist may be NULL, index may not), M >= 2^31, a non-finite transform entry.
 *
 * dmvs_cloud_pair_moments_f64: the sums one ICP step needs, over the pairs (source_i moved by `transform`, target[index[i]]).
 *   source [N,3] fp32;  target [M,3] fp32 (the sorted array `index` refers to);  index [N] int32;  valid: NULL (all) or [N] uint8.
 *   A pair is counted when index[i] >= 0, valid allows it, and the fp32 distance |q' - target| (the search's operation order) is <= max_corr.
 *   center_p, center_q: HOST, 3 doubles each.  With p = (double)q' - center_p, t = (double)target - center_q, out [DMVS_CLOUD_MOMENTS]
 *   int64 (device, zeroed here) =
 *     [0] pairs   [1..3] sum p   [4..6] sum t   [7..15] sum p_a t_b (row-major a, b)   [16] sum |p|^2   [17] sum |t|^2
 *     [18] sum |(double)q' - (double)target|^2   [19] pairs NOT summed because a |p_k| or |t_k| exceeded `bound` or index[i] >= M
 *   [1..6] are sums of rint(value * scale_linear), [7..18] of rint(value * scale_quadratic), signed 64-bit in two's complement; a sum of
 *   n terms is within n * 0.5 / scale of the exact sum.  Integer adds (lanes, wave shuffles, LDS, one atomic per counter per workgroup):
 *   bitwise independent of the launch shape, of `blocks` (0 = the library's choice) and of the order of the points.
 *   Resolution: centring bounds the coordinates by the clouds' half-extent B instead of their distance from the origin; the caller takes
 *   the largest powers of two with N B scale_linear < 2^62 and N max(3 B^2, max_corr^2) scale_quadratic < 2^62.  N = 10^7, B = 500 (a
 *   DTU scan centred on its box): scale_quadratic = 2^19, so the quadratic sums (order N B^2 / 3 ~ 10^12) carry at most 10 units
 *   (1e-11 relative) of rounding and the linear sums (2^29) at most 0.01 unit.
 *   DMVS_EINVAL: NULL operands, N or M < 0, M >= 2^31, max_corr / bound not finite or <= 0, non-finite centres or transform, a scale
 *   that is not a power of two, or one with N bound scale_linear >= 2^62 or N max(3 bound^2, (1.001 max_corr)^2) scale_quadratic >= 2^62.
 *
 * dmvs_cloud_crop_prism_f32: inside [N] uint8 = 1 where the (moved) point lies in the prism, the crop volume of a Tanks&Temples scene.
 *   polygon: DEVICE [K,2] fp64 (u, v) vertices, 3 <= K <= DMVS_CLOUD_MAX_POLYGON;  axis 0 / 1 / 2 = X / Y / Z: (u, v, w) = (1,2,0) /
 *   (0,2,1) / (0,1,2).  Inside: axis_min <= w <= axis_max (both ends included; infinite ends allowed) and (u, v) inside the polygon by the
 *   even-odd rule: edge (i, j = i - 1 cyclic) toggles when (v_i > v) != (v_j > v) and u < (u_j - u_i) * (v - v_i) / (v_j - v_i) + u_i,
 *   all in fp64 on the point's fp32 coordinates, in exactly this operation order, no contraction.  The mask is a `valid` of dmvs_cloud_stats_f32.
 *   DMVS_EINVAL: NULL operands, N < 0, K outside [3, DMVS_CLOUD_MAX_POLYGON], axis outside [0, 2], axis_min > axis_max or NaN, a non-finite transform. */
#define DMVS_CLOUD_MOMENTS 20
#define DMVS_CLOUD_MAX_POLYGON 256
int dmvs_cloud_nn_index_f32(const float* query, int64_t Q, const float* target, int64_t M, const int64_t* cell_keys,
                            const int64_t* cell_start, int64_t C, const double* origin, double h, const int32_t* dims,
                            float max_dist, const double* transform, float* dist, int32_t* index, int32_t* work, void* stream);
int dmvs_cloud_pair_moments_f64(const float* source, int64_t N, const double* transform, const float* target, int64_t M,
                                const int32_t* index, const uint8_t* valid, float max_corr, const double* center_p,
                                const double* center_q, double bound, double scale_linear, double scale_quadratic, int32_t blocks,
                                int64_t* out, void* stream);
int dmvs_cloud_crop_prism_f32(const float* points, int64_t N, const double* transform, const double* polygon, int32_t K,
                              int32_t axis, double axis_min, double axis_max, uint8_t* inside, void* stream);

/* ---------------------------------------------------------------------------------------
 * Point-cloud cleaning (added under ABI 4, additive; diffmvs_amd/cloud_clean.py builds the radius and the statistical outlier filters on it).
 *
 * dmvs_cloud_knn_f32: the k nearest targets of every query, over the grid operands and the walk of dmvs_cloud_nn_dist_f32.
 *   self_index: NULL or [Q] int32, the position in the SORTED target array that query i must not match (the query itself in a self
 *   search); -1 = none.  1 <= k <= DMVS_CLOUD_MAX_K.
 *   The candidates of query i are the targets p != self_index[i] with d2 = (dx dx + dy dy) + dz dz < md2, the fp32 squared distance of
 *   the nearest searches (same operation order, no contraction), md2 = max_dist * max_dist in fp32.  A duplicate of the query at
 *   another position is a candidate with d2 = 0.
 *   found [Q] int32 = min(k, number of candidates).
 *   d2_out: NULL or [Q,k] fp32 = the found[i] smallest candidate d2 in ascending order, padded with md2.  Ties at the k-th place have
 *     equal values, so this multiset -- and everything below -- is the same bits for any cell size and walk order.
 *   kth [Q] fp32 = sqrtf(d2_out[i, k-1]) where found[i] == k, else max_dist: "at least k others closer than r" is found == k at max_dist = r.
 *   mean [Q] fp32 = (float)(S / (double)found[i]), S = the sum of sqrt((double)d2_j) over the found entries in ascending order, fp64
 *     without contraction; max_dist where found[i] == 0.
 *   A non-finite query finds nothing (found = 0), as in the nearest searches.  work as in dmvs_cloud_nn_dist_f32.
 *   DMVS_EINVAL: as dmvs_cloud_nn_index_f32 (d2_out and self_index may be NULL; kth, mean and found may not), k outside [1, DMVS_CLOUD_MAX_K]. */
#define DMVS_CLOUD_MAX_K 32
int dmvs_cloud_knn_f32(const float* query, int64_t Q, const float* target, int64_t M, const int64_t* cell_keys,
                       const int64_t* cell_start, int64_t C, const double* origin, double h, const int32_t* dims,
                       float max_dist, const int32_t* self_index, int32_t k, float* d2_out, float* kth, float* mean,
                       int32_t* found, int32_t* work, void* stream);

/* ---------------------------------------------------------------------------------------
 * Depth-map scoring (added under ABI 4, additive): the per-pixel errors of utils.py:150-187 (AbsDepthError_metrics) and the "DTU abs-rel"
 * of BASELINE.json as integer and fixed-point sums per batch item (diffmvs_amd/depth_eval.py turns the rows into the metrics).
 *
 * dmvs_depth_stats_f32: est, gt [B, HW] fp32;  mask: NULL (every pixel) or [B, HW] fp32, a pixel is masked in where mask > 0.5
 *   (train.py:214-217).  out [B, DMVS_DEPTH_SLOTS + T] int64 (device, zeroed here), per item:
 *     [0] pixels masked in
 *     [1] pixels scored: masked in, est and gt finite, gt > 0, and band_lo <= |e| <= band_hi
 *     [2] pixels left out because est or gt is not finite or gt <= 0  (masked in and inside the band but not scored: [0] - [1] - [2])
 *     [3] TERMS of the three sums below that were clamped (|e| > big, |e| / gt > big, e^2 > big^2: up to three per scored pixel)
 *     [4] sum llrint(min(|e|, big) * scale)            [5] sum llrint(min(|e| / gt, big) * scale)
 *     [6] sum llrint(min(e^2, big^2) * scale_sq)       [7 + t] scored pixels with |e| < (double)thresholds[t]
 *   over the scored pixels, with e = (double)est - (double)gt; the difference, the quotient and the square are IEEE fp64 operations without
 *   contraction and llrint rounds half to even, so an fp64 restatement reproduces every integer.
 *   thresholds: HOST array of T <= DMVS_DEPTH_MAX_THRESHOLDS floats (not NaN).
 *   band_lo, band_hi: the `thres` band of AbsDepthError_metrics, 0 <= band_lo <= band_hi; (0, +inf) scores every valid pixel.
 *   big: finite, > 0.   scale: a positive power of two with big * scale * max(HW, 1) < 2^62 (no item's sum can overflow);
 *   scale_sq = scale / p, p the smallest power of two >= big, so that big^2 * scale_sq <= big * scale.
 *   blocks: workgroups PER ITEM of the grid-stride launch, 0 = the library's choice (the result does not depend on it).
 * Registers, wave shuffles, LDS, then one integer atomic per slot per workgroup: bitwise independent of launch order and grid shape.
 * Pixels are read 16 bytes at a time where est, gt and mask share one 16-byte phase (always the case for whole torch allocations), with a
 * scalar head and tail per item; otherwise one by one.  Same integers either way.
 * DMVS_EINVAL (before any launch): NULL est / gt / out with B * HW > 0, pointers not 4-byte aligned, B or HW < 0, B > 65535, T outside
 * [0, DMVS_DEPTH_MAX_THRESHOLDS], a NaN threshold, a band that is NaN / negative / empty, big or scale outside the above, blocks < 0. */
#define DMVS_DEPTH_MAX_THRESHOLDS 8
#define DMVS_DEPTH_SLOTS 7
int dmvs_depth_stats_f32(const float* est, const float* gt, const float* mask, int64_t B, int64_t HW, const float* thresholds, int32_t T,
                         double band_lo, double band_hi, double big, double scale, int32_t blocks, int64_t* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Ground-truth depth maps from a cloud (added under ABI 4, additive; diffmvs_amd/cloud_render.py): a scatter with a z-buffer, two passes
 * over the same walk.
 *
 * points [N,3] fp32 (device).  transform: as above (HOST 3x4 or NULL), applied first; the moved point is fp32.
 * views: HOST [V, DMVS_SPLAT_VIEW_DOUBLES] doubles per view: rows 0 and 1 of P = K E[:3] (4 + 4), row 2 of E (4), f = K[0][0], near, far.
 * Per (point (X, Y, Z) widened to fp64, view), IEEE fp64 in exactly this order, no contraction:
 *     x = ((P00 X + P01 Y) + P02 Z) + P03      y likewise with row 1      z = ((E20 X + E21 Y) + E22 Z) + E23
 *     slot 0 and no more if X, Y or Z is not finite;  slot 1 unless near < z <= far
 *     u = x / z, v = y / z (pixel centres at integer coordinates);  slot 2 if u or v is not finite
 *     r = fmin(fmax(radius * f / z, r_min), r_max)
 *     columns fmax(ceil(u - r), 0) .. fmin(floor(u + r), W - 1), rows likewise with v and H, clamped in fp64 and then converted;
 *     slot 2 ("off the image") if either range is empty;  otherwise slot 3 if radius * f / z > r_max (the radius was clamped), and
 *     z32 = (float)z goes to every pixel of the footprint:
 * dmvs_cloud_splat_zmin_f32: zbuf[view][row][col] = min(zbuf, z32).  zbuf [V,H,W] fp32 is the CALLER's, pre-filled with +inf.  One u32
 *   integer atomic-min on the bit pattern per pixel (z32 >= 0: the bits order like the values), behind a plain load that skips it when z32
 *   cannot lower the pixel (flags & DMVS_SPLAT_NO_PRETEST: always issue it; same result).
 *   counts [V, DMVS_SPLAT_SLOTS] int64 (device, zeroed here): the slots above, per view.
 *   work: NULL or [2] uint64 (device, zeroed here): footprint pixels visited, atomics issued (the second depends on timing with the pre-test).
 * dmvs_cloud_splat_sum_f32: the same walk over the FINISHED zbuf; for every footprint pixel with (double)z32 <= (double)zbuf * (1.0 + tau):
 *   sum[pixel] += llrint((double)z32 * scale) (uint64) and cnt[pixel] += 1 (int32); sum, cnt [V,H,W] (device, zeroed here).
 *   scale: a positive power of two with max(far) * scale * max(N, 1) < 2^62.
 *   The mean depth of a pixel is (float)(((double)sum / (double)cnt) / scale) where cnt > 0, the nearest one zbuf where it is finite.
 * blocks: workgroups of the grid-stride launch, 0 = the library's choice.  Views go DMVS_SPLAT_VIEW_CHUNK per launch as kernel arguments.
 * Integer min and integer adds only: every output is bitwise independent of blocks, of the launch order and of the order of the points.
 * N = 0 or V = 0: nothing is touched.  DMVS_EINVAL (before any launch): N, V, H, W or blocks < 0, N >= 2^31 (cnt and the slot counters of a workgroup are 32 bits), H W >= 2^31
 * or V H W > 2^40, NULL operands with work to do, points / zbuf / cnt not 4-byte or counts / work / sum not 8-byte aligned, a view with a
 * non-finite matrix entry, f < 0 or not finite, near <= 0, far <= near or far > FLT_MAX (NaN included), radius or r_min negative or not
 * finite, r_max < r_min or r_max > DMVS_SPLAT_MAX_RADIUS (a footprint is at most 33 x 33 pixels), a non-finite transform, unknown flags,
 * tau negative or not finite, a scale that is not a power of two or beyond the bound. */
#define DMVS_SPLAT_VIEW_CHUNK 8
#define DMVS_SPLAT_VIEW_DOUBLES 15
#define DMVS_SPLAT_SLOTS 4
#define DMVS_SPLAT_MAX_RADIUS 16
#define DMVS_SPLAT_NO_PRETEST 0x1
int dmvs_cloud_splat_zmin_f32(const float* points, int64_t N, const double* transform, const double* views, int64_t V, int32_t H, int32_t W,
                              double radius, double r_min, double r_max, int32_t flags, int32_t blocks, float* zbuf, int64_t* counts,
                              uint64_t* work, void* stream);
int dmvs_cloud_splat_sum_f32(const float* points, int64_t N, const double* transform, const double* views, int64_t V, int32_t H, int32_t W,
                             double radius, double r_min, double r_max, double tau, double scale, int32_t blocks, const float* zbuf,
                             uint64_t* sum, int32_t* cnt, void* stream);

/* ---------------------------------------------------------------------------------------
 * Oriented normals of a depth map (added under ABI 4, additive; diffmvs_amd/fusion.py): for a plane n.X = rho seen by a pinhole camera
 * 1 / depth is an affine function of the pixel, 1/d = (K^T)^-1 (n / rho) . (u, v, 1), so the plane through a pixel's neighbourhood is a
 * LINEAR least-squares fit in inverse depth on integer pixel offsets: an exact integer normal matrix, three fp64 sums, no eigen-solver.
 *
 * depth [B,H,W] fp32 (device);  valid: NULL or [B,H,W] uint8 (device);  cams: HOST [B, DMVS_NORMAL_CAM_DOUBLES] doubles per view:
 * K row-major (9) | inv(K) (9, formed by the caller) | R = E[:3,:3], world -> camera (9).  Views go DMVS_NORMAL_VIEW_CHUNK per launch as
 * kernel arguments.  out [B,H,W,4] fp32: the world normal x, y, z and the cosine between it and the ray back to the camera.
 * counts [B, DMVS_NORMAL_SLOTS] int64 (device, zeroed here).
 * Per pixel (y, x), pixel centres at integer coordinates, IEEE fp64 in exactly this order, no contraction:
 *   usable(j): (valid is NULL or valid[j] != 0) and depth[j] finite and > 0;  then w_j = 1.0 / (double)depth[j].
 *   The centre c is not usable: slot 0, four zeros.
 *   Support: the offsets dy = -r .. r (outer), dx = -r .. r (inner) that are inside the image, usable and have
 *     fabs(d_j) <= rel_jump * w_c  with  d_j = w_j - w_c  (the centre always is); any other tap is skipped.
 *   Integer sums over the support (exact): n, Sx = sum dx, Sy = sum dy, Sxx, Sxy, Syy.
 *   fp64 sums in walk order: Tw += d_j,  Tx += (double)dx * d_j,  Ty += (double)dy * d_j.
 *   Integer cofactors:  C00 = Syy n - Sy^2   C01 = -(Sxy n - Sx Sy)   C02 = Sxy Sy - Syy Sx
 *                       C11 = Sxx n - Sx^2   C12 = -(Sxx Sy - Sxy Sx)   C22 = Sxx Syy - Sxy^2     D = Sxx C00 + Sxy C01 + Sx C02
 *   n < min_pts or D == 0 (collinear support): slot 1, zeros.
 *   a = ((C00 Tx + C01 Ty) + C02 Tw) / D    b = ((C01 Tx + C11 Ty) + C12 Tw) / D    c = ((C02 Tx + C12 Ty) + C22 Tw) / D
 *     (the integers converted to double, exactly);   w_f = w_c + c;   c0 = (w_f - a x) - b y
 *   g_i = (K[0][i] a + K[1][i] b) + K[2][i] c0      len = sqrt((g0^2 + g1^2) + g2^2)
 *   ray_i = (Kinv[i][0] x + Kinv[i][1] y) + Kinv[i][2]      rl = sqrt((ray0^2 + ray1^2) + ray2^2)
 *   !(w_f > 0), len not finite or len == 0: slot 2, zeros.
 *   Otherwise slot 3:  n_cam = -g / len (it faces the camera: g . X_c = w_f d_c > 0),  N_i = (R[0][i] n0 + R[1][i] n1) + R[2][i] n2,
 *     cos = w_f / (len * rl);  the four values are rounded once to fp32.
 * One workgroup per image tile with its halo staged once in LDS as fp64 w (0 = not usable), one lane per pixel, one 16-byte store per
 * pixel, LDS slot counters and one u64 integer atomic per non-zero slot per workgroup: every output is bitwise independent of the tile
 * shape and of the launch order.  B = 0, H = 0 or W = 0: nothing is touched.
 * DMVS_EINVAL (before any launch): B, H or W < 0, H W >= 2^31 or B H W > 2^40, NULL depth / cams / out / counts with work to do, radius
 * outside 1 .. DMVS_NORMAL_MAX_RADIUS, min_pts outside 3 .. (2 radius + 1)^2, rel_jump negative or not finite, a non-finite cams entry,
 * depth not 4-byte, out not 16-byte or counts not 8-byte aligned. */
#define DMVS_NORMAL_MAX_RADIUS 4
#define DMVS_NORMAL_CAM_DOUBLES 27
#define DMVS_NORMAL_VIEW_CHUNK 8
#define DMVS_NORMAL_SLOTS 4
int dmvs_depth_normals_f32(const float* depth, const uint8_t* valid, const double* cams, int64_t B, int32_t H, int32_t W,
                           int32_t radius, double rel_jump, int32_t min_pts, float* out, int64_t* counts, void* stream);

/* ---------------------------------------------------------------------------------------
 * A surface from depth maps (added under ABI 4, additive; diffmvs_amd/mesh.py): a truncated signed distance volume averaged over all
 * views, and its zero set as a surface-nets mesh.  Integer sums and fp64 geometry in a fixed order: every output is bitwise independent
 * of the chunking and the order of the views, of the launch shape and of the run.
 *
 * The volume: dims (nx, ny, nz), nx ny nz < 2^31; origin: HOST, three doubles; h: the voxel side.  Voxel (i, j, k) samples the world
 * point  X = ox + (double)i * h,  Y = oy + (double)j * h,  Z = oz + (double)k * h.  S, Wt: [nz,ny,nx] int32 (device, x fastest);
 * C: NULL or [nz,ny,nx,4] uint32, the R, G, B sums and their count.  The caller zeroes them once; integration ADDS to them, so a scene
 * can be streamed through in several calls.
 *
 * dmvs_tsdf_integrate_f32: depth [V,H,W] fp32 (device); valid: NULL or [V,H,W] uint8; rgb: NULL or [V,H,W,3] uint8 (needs C);
 * views: HOST [V, DMVS_TSDF_VIEW_DOUBLES] doubles per view: rows 0 and 1 of P = K E[:3] (P00 .. P03, P10 .. P13), then row 2 of E
 * (world -> camera); they go DMVS_TSDF_VIEW_CHUNK per launch as kernel arguments.  Per (voxel, view), pixel centres at integer
 * coordinates, IEEE fp64 in exactly this order, no contraction:
 *   x = ((P00 X + P01 Y) + P02 Z) + P03     y likewise with row 1     z = ((E20 X + E21 Y) + E22 Z) + E23
 *   skip unless z > 0;   u = x / z,  v = y / z;   skip if u or v is not finite
 *   pu = rint(u), pv = rint(v) (ties to even);   skip unless 0 <= pu <= W - 1 and 0 <= pv <= H - 1 (tested in fp64, then converted)
 *   d = (double)depth[view][pv][pu];   skip unless (valid is NULL or valid[..] != 0) and d finite and d > 0
 *   sdf = d - z;   skip if sdf < -tau
 *   q = (int32)rint(fmin(sdf / tau, 1.0) * 16384.0);   S += q;   Wt += 1
 *   if rgb and sdf <= tau:   C += (r, g, b, 1)
 * One owner lane per voxel, plain read-modify-write, no atomics.  V <= DMVS_TSDF_MAX_VIEWS per call and over the life of a volume
 * (the caller's to keep) bounds |S| below 2^30 and the colour sums below 2^24.  A workgroup skips a (brick of voxels, view) pair only
 * when every voxel of the brick is provably behind the camera or off one side of the image (csrc/tsdf.hip has the argument): the
 * volume is bitwise the same with flags = DMVS_TSDF_NO_CULL, which is there for A/B runs and the tests.
 * V = 0, H W = 0 or an empty volume: nothing is touched.
 * DMVS_EINVAL (before any launch): a negative dim, nx ny nz >= 2^31, NULL origin, origin or h not finite, h <= 0, V < 0 or
 * V > DMVS_TSDF_MAX_VIEWS, H or W < 0, H W >= 2^31, tau not finite or <= 0, an unknown flag, rgb without C, NULL depth / views / S / Wt
 * with work to do, a non-finite views entry, depth / S / Wt not 4-byte or C not 16-byte aligned.
 *
 * Extraction (surface nets: no case table).  A voxel is OBSERVED iff Wt >= min_weight (min_weight >= 1), its value is
 * f = (double)S / (double)Wt, it is INSIDE iff S < 0.  Cell (i, j, k) of the (nx-1)(ny-1)(nz-1) cell grid has the corners c = 0 .. 7 at
 * the offsets (c & 1, c >> 1 & 1, c >> 2 & 1) and gets a VERTEX iff all 8 are observed and at least one of its 12 edges has ends of
 * different sign.  The edges are walked as the pairs (a, b), a < b, one bit apart, in lexicographic order: (0,1) (0,2) (0,4) (1,3)
 * (1,5) (2,3) (2,6) (3,7) (4,5) (4,6) (5,7) (6,7); a crossing edge contributes the point offset(a) + t e_axis, t = f_a / (f_a - f_b);
 * the three coordinates are summed in fp64 in that order and divided by the number of crossings; the vertex is
 * origin + ((double)cell + mean) * h per axis, rounded once to fp32.  Its colour, with n the sum of the eight corners' counts, is
 * (2 sum R + n) / (2 n) in integers, likewise G and B; 0 without C or with n = 0.  Vertices are numbered in ascending cell linear
 * index (x fastest).  Faces: for voxel (i, j, k) in ascending linear index and axis a = x, y, z in that order, the edge to the +a
 * neighbour, if that exists, both ends are observed and their signs differ, yields a quad over the cells at the offsets
 * (b, c) = (-1,-1), (0,-1), (0,0), (-1,0) along the cyclically next axes b, c -- only if all four are in the cell grid and have a
 * vertex; in that order if the voxel is inside, reversed otherwise (the normal points from inside to free space); the triangles are
 * (q0, q1, q2), (q0, q2, q3).
 *   dmvs_tsdf_flags_u8: cell [nz,ny,nx] uint8 = 1 where the cell whose lowest corner is the voxel has a vertex (0 on the upper
 *     faces), quad [nz,ny,nx] uint8: bit a set where the voxel's +a edge yields a quad.  Two launches (quad reads cell).
 *   The caller forms the INCLUSIVE running sums cell_cum, quad_cum [nz,ny,nx] int32 of cell and of popcount(quad), N = the number of
 *     vertices and Q = the number of quads (their last entries).
 *   dmvs_tsdf_vertices_f32: verts [N,3] fp32, rgb [N,3] uint8, vertex cell_cum - 1 of every flagged cell.
 *   dmvs_tsdf_faces_i32: faces [2 Q,3] int32, quads quad_cum - popcount(quad) .. quad_cum - 1 of every voxel, in axis order.
 * An empty volume, N = 0 or Q = 0: nothing is touched.  DMVS_EINVAL: the volume's cases above (origin and h where they are taken),
 * min_weight < 1, N < 0 or N > nx ny nz, Q < 0, Q > 3 nx ny nz or Q > DMVS_TSDF_MAX_QUADS, a NULL array other than C with work to do,
 * a misaligned int32 / fp32 array or C. */
#define DMVS_TSDF_VIEW_CHUNK 8
#define DMVS_TSDF_VIEW_DOUBLES 12
#define DMVS_TSDF_MAX_VIEWS 65535
#define DMVS_TSDF_MAX_QUADS 357913941 /* 6 Q int32 face entries below 2^31 */
#define DMVS_TSDF_NO_CULL 0x1
int dmvs_tsdf_integrate_f32(const float* depth, const uint8_t* valid, const uint8_t* rgb, const double* views, int64_t V, int32_t H, int32_t W,
                            int32_t nx, int32_t ny, int32_t nz, const double* origin, double h, double tau, int32_t flags, int32_t* S,
                            int32_t* Wt, uint32_t* C, void* stream);
int dmvs_tsdf_flags_u8(const int32_t* S, const int32_t* Wt, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight, uint8_t* cell,
                       uint8_t* quad, void* stream);
int dmvs_tsdf_vertices_f32(const int32_t* S, const int32_t* Wt, const uint32_t* C, int32_t nx, int32_t ny, int32_t nz, const double* origin,
                           double h, const uint8_t* cell, const int32_t* cell_cum, int64_t N, float* verts, uint8_t* rgb, void* stream);
int dmvs_tsdf_faces_i32(const int32_t* S, int32_t nx, int32_t ny, int32_t nz, const uint8_t* quad, const int32_t* quad_cum,
                        const int32_t* cell_cum, int64_t Q, int32_t* faces, void* stream);

/* ---------------------------------------------------------------------------------------
 * Triangle meshes into the views (added under ABI 4, additive; diffmvs_amd/mesh_render.py): a z-buffer rasteriser whose coverage is
 * exact integer arithmetic on vertices snapped to 1/256 pixel.  Integer min and integer adds only: zid and counts are bitwise
 * independent of blocks, of the queue, of the launch order and of the order of the faces.
 *
 * verts [N,3] fp32, faces [F,3] int32 (device).  transform: as above (HOST 3x4 or NULL), applied to a vertex first; the moved vertex
 * is fp32.  views: HOST [V, DMVS_RASTER_VIEW_DOUBLES] doubles per view: rows 0 and 1 of P = K E[:3] (4 + 4), E[:3] row-major (12,
 * world -> camera), near, far.  Views go DMVS_SPLAT_VIEW_CHUNK per launch as kernel arguments.
 *
 * dmvs_mesh_raster_fill_u64: zid[0 .. n) = all ones ("nothing drawn") on the stream.
 *
 * dmvs_mesh_raster_zid_u64: zid [V,H,W] uint64 is the CALLER's, pre-filled with all ones.  Every (face, view) is counted in exactly
 * one slot of counts [V, DMVS_RASTER_SLOTS] int64 (device, zeroed here).  IEEE fp64 in exactly this order, no contraction:
 *   1. per vertex (X, Y, Z) widened to fp64:  x = ((P00 X + P01 Y) + P02 Z) + P03,  y likewise with row 1,
 *      z = ((E20 X + E21 Y) + E22 Z) + E23,  u = x / z,  v = y / z  (pixel centres at integer coordinates)
 *   2. slot 0: a vertex index outside [0, N) or a (moved) coordinate that is not finite
 *   3. slot 1: some vertex has z <= near.  The face is NOT DRAWN -- there is no near clipping; the count tells the caller
 *   4. slot 2: all three vertices have z > far
 *   5. slot 3: some |u| or |v| is not <= 2^20 (the guard band; NaN included)
 *   6. sx = llrint(u * 256), sy = llrint(v * 256) as int64; everything about coverage is integer arithmetic from here (below 2^59)
 *   7. A = (sx1 - sx0)(sy2 - sy0) - (sy1 - sy0)(sx2 - sx0);  slot 4: A == 0;  slot 5: culled (flags & DMVS_RASTER_CULL_NEG and A < 0,
 *      or flags & DMVS_RASTER_CULL_POS and A > 0);  if A < 0, vertices 1 and 2 change places and A = -A (the face keeps its index)
 *   8. columns max(ceil(min sx / 256), 0) .. min(floor(max sx / 256), W - 1), rows likewise with sy and H;  slot 6: the box is empty;
 *      otherwise slot 7: drawn
 *   9. pixel (px, py) of the box is COVERED iff for k = 0, 1, 2, with a = k + 1, b = k + 2 (mod 3), dx = sxb - sxa, dy = syb - sya,
 *      e_k = dx (256 py - sya) - dy (256 px - sxa):   e_k > 0,  or  e_k == 0 and (dy > 0 or (dy == 0 and dx > 0)).
 *      Of the two directions of a shared edge exactly one owns its boundary: a pixel centre on it belongs to one of the two faces
 *  10. wq_k = ((double)e_k / (double)A) * (1.0 / z_k);  zp = 1.0 / ((wq_0 + wq_1) + wq_2);  skipped unless zp <= far;
 *      zid[pixel] = min(zid[pixel], (uint64)bits((float)zp) << 32 | face): one u64 integer atomic-min, behind a plain load that skips
 *      it when it cannot lower the pixel.  The depth is positive, so the bits order like the values; equal depths go to the smaller face
 *   work: NULL or [3] uint64 (device, zeroed here): covered pixels (exact), atomics issued (depends on timing), faces that fell back.
 *   A (face, view) whose box holds at most DMVS_RASTER_SMALL pixels is walked by the lane that projected it.  A larger one is appended
 *   to `queue` -- the caller's [1 + queue_cap] uint64 on the device, word 0 the counter, zeroed here per launch -- and walked by a whole
 *   wave in a second launch; with the queue full (or queue_cap = 0) the lane walks it itself and work[2] counts it.
 *   blocks: workgroups of the grid-stride launches, 0 = the library's choice.
 *
 * dmvs_mesh_raster_resolve_f32: per pixel of the FINISHED zid (same mesh, transform and views).  depth [V,H,W] fp32 = the high word
 * as a float, face [V,H,W] int32 = the low word; 0 and -1 where zid is all ones.
 *   normal: NULL or [V,H,W,3] fp32, from the winning face's (moved) vertices p0, p1, p2 in the order of the file, widened to fp64:
 *     a = p1 - p0, b = p2 - p0, c = (ay bz - az by, az bx - ax bz, ax by - ay bx), len = sqrt((cx^2 + cy^2) + cz^2), n = c / len;
 *     with nc_i = (Ei0 nx + Ei1 ny) + Ei2 nz and pc_i = ((Ei0 X0 + Ei1 Y0) + Ei2 Z0) + Ei3:  n = -n if (nc_0 pc_0 + nc_1 pc_1) + nc_2 pc_2 > 0
 *     (it faces the camera); rounded once to fp32.  Zeros where nothing was drawn or len is 0 or not finite.
 *   rgb: NULL or [V,H,W,3] uint8 from vrgb [N,3] uint8: steps 1 to 10 redone for that face and pixel, b_k = wq_k * zp, a channel is
 *     fmin(fmax(rint((b_0 c_0 + b_1 c_1) + b_2 c_2), 0), 255) with c_k the (swapped) vertices' values.  Zeros where nothing was drawn.
 *
 * F = 0 or V = 0: nothing but the zeroed counters is touched.  DMVS_EINVAL (before any launch): a negative size, N, F or H W >= 2^31,
 * V H W > 2^40, NULL operands with work to do, verts / faces / depth / face / normal not 4-byte or zid / counts / work / queue not
 * 8-byte aligned, a non-finite views entry, near <= 0, far <= near or far > FLT_MAX, both cull flags or an unknown one, blocks < 0,
 * queue_cap < 0 or >= 2^31, a NULL queue with queue_cap > 0, a non-finite transform, rgb without vrgb. */
#define DMVS_RASTER_VIEW_DOUBLES 22
#define DMVS_RASTER_SLOTS 8
#define DMVS_RASTER_SMALL 64
#define DMVS_RASTER_CULL_NEG 0x1
#define DMVS_RASTER_CULL_POS 0x2
int dmvs_mesh_raster_fill_u64(uint64_t* zid, int64_t n, void* stream);
int dmvs_mesh_raster_zid_u64(const float* verts, int64_t N, const int32_t* faces, int64_t F, const double* transform, const double* views,
                             int64_t V, int32_t H, int32_t W, int32_t flags, int32_t blocks, uint64_t* zid, int64_t* counts,
                             uint64_t* work, uint64_t* queue, int64_t queue_cap, void* stream);
int dmvs_mesh_raster_resolve_f32(const uint64_t* zid, const float* verts, int64_t N, const int32_t* faces, int64_t F, const double* transform,
                                 const double* views, int64_t V, int32_t H, int32_t W, const uint8_t* vrgb, float* depth, int32_t* face,
                                 float* normal, uint8_t* rgb, void* stream);

/* ---------------------------------------------------------------------------------------
 * Cleaning and scoring an extracted mesh (added under ABI 4, additive; diffmvs_amd/mesh_clean.py, diffmvs_amd/mesh_eval.py): connected
 * components, per-component face counts and areas, and points spread evenly by area.  Integer min, integer adds and fp64 in a fixed
 * order: every output is bitwise independent of blocks, of timing and of the run.
 *
 * verts [N,3] fp32, faces [F,3] int32 (device).  blocks: workgroups of the grid-stride launches, 0 = the library's choice.
 *
 * dmvs_mesh_label_round_i32: ONE round of labelling; two vertices are connected when a face names both.  label [N] int32 is the caller's,
 * filled with label[v] = v before the first round; state [2] int32 (device) is zeroed here on the stream.
 *   hook (first launch): a face with an index outside [0, N) is skipped and counted in state[1].  For every other face
 *     m = min over its vertices y of label[label[y]];  then for each of its vertices x, label[label[x]] and label[x] are lowered to m.
 *   shortcut (second launch): every label[v] is lowered to label[label[v]].
 *   "lowered": a u32 atomic-min behind a plain load, issued only when the loaded value is larger; every issued one adds 1 to state[0].
 *   Labels only fall, every value written is a vertex of the same component, and a stale load can only be too high: it costs a spurious
 *   count or one more round.  No launch relies on seeing another workgroup's writes of the same launch; nothing waits.  A round that
 *   leaves state[0] == 0 wrote nothing, so all it read was settled at a launch boundary: every face's labels are equal and
 *   label[label[v]] == label[v], hence label[v] is the SMALLEST VERTEX INDEX of v's component (v itself for a vertex no face names).
 *   That fixpoint is unique; the number of rounds to it is not part of the contract.  state[0] and state[1] are exact while a
 *   workgroup counts fewer than 2^31 / (workgroups of the round); beyond that they saturate (positive, below 2^31).
 *   A label outside [0, N) (never with labels made here) is not followed.
 *
 * dmvs_mesh_face_tally_i64: area_q [F] int64; comp_faces [N] int32 and comp_area [N] int64 are zeroed here.  Per face, its vertices
 * p0, p1, p2 widened to fp64, IEEE fp64 in exactly this order, no contraction:
 *   a = p1 - p0,  b = p2 - p0,  c = (ay bz - az by, az bx - ax bz, ax by - ay bx),  area = 0.5 * sqrt((cx^2 + cy^2) + cz^2)
 *   q = llrint(fmin(area * scale, cap)), or 0 where area is not finite;  area_q[f] = q
 *   A face with an index outside [0, N) gets area_q = 0 and is counted nowhere.  Every other face adds 1 to comp_faces[r] and q to
 *   comp_area[r], r = label[faces[f][0]] (a label outside [0, N): as an out-of-range face).  Integer atomics; a wave whose live lanes
 *   share one root adds them up first (shuffles, registers, then LDS per workgroup), so the order of the sums is free.  scale: a positive finite power of two; 0 <= cap < 2^62; the
 *   caller keeps F * cap < 2^62.
 *
 * dmvs_mesh_sample_f32: systematic sampling by area, one lane per sample k = 0 .. M - 1.  area_cum [F] int64: the caller's INCLUSIVE
 * running sum of area_q; the caller keeps M * a0 <= area_cum[F - 1].
 *   t = k * a0 + (a0 >> 1);  f = the smallest index with area_cum[f] > t (binary search; a face of zero area is never chosen)
 *   r1 = (double)(uint32)((uint32)k * 3242174889u) * 2^-32,  r2 = (double)(uint32)((uint32)k * 2447445414u) * 2^-32  (the R2 sequence)
 *   if r1 + r2 > 1.0:  r1 = 1 - r1,  r2 = 1 - r2
 *   per coordinate, a = p1 - p0, b = p2 - p0 in fp64:  points[k] = (float)((p0 + r1 * a) + r2 * b);  face_of[k] = f
 *   No such f, or a face with an index outside [0, N) (never with an area_cum made as above): points[k] = 0, face_of[k] = -1.
 *
 * F = 0 or N = 0 (and M = 0): nothing but the zeroed counters is touched.  DMVS_EINVAL (before any launch): a negative size, N or
 * F >= 2^31, NULL operands with work to do (state always), an int32 / fp32 array not 4-byte or an int64 array not 8-byte aligned,
 * blocks < 0, a scale that is not a positive finite power of two, cap not in [0, 2^62), a0 < 1, M < 0, M > 2^31 - 1, M a0 >= 2^63. */
int dmvs_mesh_label_round_i32(const int32_t* faces, int64_t F, int64_t N, int32_t* label, int32_t* state, int32_t blocks, void* stream);
int dmvs_mesh_face_tally_i64(const float* verts, int64_t N, const int32_t* faces, int64_t F, const int32_t* label, double scale, double cap,
                             int64_t* area_q, int32_t* comp_faces, int64_t* comp_area, int32_t blocks, void* stream);
int dmvs_mesh_sample_f32(const float* verts, int64_t N, const int32_t* faces, int64_t F, const int64_t* area_cum, int64_t a0, int64_t M,
                         float* points, int32_t* face_of, int32_t blocks, void* stream);

/* ---------------------------------------------------------------------------------------
 * Simplifying an extracted mesh (added under ABI 4, additive; diffmvs_amd/mesh_simplify.py): vertex clustering on a uniform lattice, each
 * cluster's vertex at the minimum of its faces' summed plane quadrics, regularised towards the mean of its vertices.  Integer sums and
 * IEEE fp64 in a fixed order without contraction: every output is bitwise independent of blocks, of timing and of the run.
 *
 * verts [N,3] fp32, rgb [N,3] uint8 or NULL, faces [F,3] int32, cluster [N] int32 (device): the caller's cluster of every vertex, a value
 * outside [0, K) = "none" (diffmvs_amd/mesh_simplify.py: the rank of the vertex's lattice key among the occupied keys, -1 for a vertex with
 * a non-finite coordinate).  origin [3] fp64 (HOST) and cell: the lattice.  blocks: workgroups of the grid-stride launches, 0 = the
 * library's choice.  The LOCAL coordinate of a vertex p, per axis i:
 *   t = (p_i - origin_i) / cell,  u_i = t - (floor(t) + 0.5)   in [-0.5, 0.5];  u_i = 0 where t is not finite (never with clusters made as above)
 *
 * dmvs_mesh_cluster_verts_i64: cnt [K] int32, pos_q [K,3] int64 and rgb_sum [K,3] int64 are zeroed here.  Per vertex with a cluster k:
 *   cnt[k] += 1,  pos_q[k][i] += llrint(u_i * 2^32),  rgb_sum[k][i] += rgb[v][i] (rgb NULL: rgb_sum may be NULL and is not touched).
 *
 * dmvs_mesh_cluster_quadrics_i64: quad_q [K,10] int64 and state [2] int64 are zeroed here.  A face with an index outside [0, N) or a vertex
 * without a cluster is BAD: state[0] += 1, nothing else.  Every other face, p0, p1, p2 widened to fp64, as dmvs_mesh_face_tally_i64 does:
 *   a = p1 - p0,  b = p2 - p0,  c = (ay bz - az by, az bx - ax bz, ax by - ay bx),  l = sqrt((cx^2 + cy^2) + cz^2)
 *   l zero or not finite: the face is FLAT, state[1] += 1, nothing else.   n = c / l,  w = fmin((0.5 * l) / (cell * cell), cap)
 *   for each corner j whose cluster k differs from the clusters of the corners before it, with u the LOCAL coordinate of THAT corner:
 *     d = -((nx ux + ny uy) + nz uz)      (the plane in the frame of the cell centre of the cluster it is added to)
 *     quad_q[k][0 .. 9] += llrint(T * scale),  T = (w nx) nx, (w nx) ny, (w nx) nz, (w ny) ny, (w ny) nz, (w nz) nz,
 *                                                  (w d) nx, (w d) ny, (w d) nz, (w d) d
 *   |T| <= cap.  scale: a positive finite power of two; 0 <= cap < 2^62; 3 F cap scale < 2^62 (checked), so no sum overflows.  Integer atomics;
 *   runs of neighbouring lanes of a wave that add to the same cluster are summed with shuffles first and go out as one lot (compiled with
 *   -DDMVS_MESH_QUADRIC_PLAIN every lane issues its own): the order of integer sums is free.
 *
 * dmvs_mesh_cluster_place_f32: one lane per cluster k.  cells [K,3] int64: the cluster's lattice cell.  mode: DMVS_SIMPLIFY_QUADRIC or
 * DMVS_SIMPLIFY_MEAN.  state [1] int64 is zeroed here.  out_rgb / rgb_sum may be NULL together.
 *   A = [[q0 q1 q2] [q1 q3 q4] [q2 q4 q5]] / scale,  b = (q6, q7, q8) / scale   (exact: scale is a power of two)
 *   m_i = ((double)pos_q[k][i] / 2^32) / (double)cnt[k]   (cnt 0: m = 0);  tr = (A00 + A11) + A22;  lam = reg * tr
 *   M = A + lam I (diagonal only);  r_i = lam * m_i - b_i
 *   c00 = M11 M22 - M12 M12,  c01 = M02 M12 - M01 M22,  c02 = M01 M12 - M02 M11,
 *   c11 = M00 M22 - M02 M02,  c12 = M01 M02 - M00 M12,  c22 = M00 M11 - M01 M01,   det = (M00 c00 + M01 c01) + M02 c02
 *   x0 = ((c00 r0 + c01 r1) + c02 r2) / det,  x1 = ((c01 r0 + c11 r1) + c12 r2) / det,  x2 = ((c02 r0 + c12 r1) + c22 r2) / det
 *   good = tr > 0 and det > 0 and x finite and max |x_i| <= 1.   mode MEAN, or not good: x = m; mode QUADRIC, tr > 0 and not good: state[0] += 1.
 *   out_verts[k][i] = (float)(origin_i + (((double)cells[k][i] + 0.5) + x_i) * cell)
 *   out_rgb[k][i] = (2 rgb_sum[k][i] + cnt[k]) / (2 cnt[k]) in integers (cnt 0: 0).
 *
 * dmvs_mesh_cluster_remap_i32: out_faces [F,3] int32, keep [F] uint8; state [3] int64 is zeroed here.  A BAD face (as above): out_faces =
 * (-1, -1, -1), keep = 0, state[2] += 1.  Every other face: its corners' clusters, rotated so that the smallest index comes first (the
 * orientation stays); keep = 1 where the three differ, else 0 and state[0] += 1 (degenerate).  With new_verts [K,3] fp32 (may be NULL: nothing
 * is counted), per kept face, corners in the face's INPUT order: c = the cross product above of the old positions, c' = the same formula on
 * new_verts of the corners' clusters; state[1] += 1 where (cx c'x + cy c'y) + cz c'z < 0 (flipped).
 *
 * F = 0, N = 0 or K = 0: nothing but the zeroed outputs is touched (remap: every face is BAD when N or K is 0).  DMVS_EINVAL (before any
 * launch): a negative size, N, F or K >= 2^31, NULL operands with work to do (origin and state always), an int32 / fp32 array not 4-byte
 * or an int64 array not 8-byte aligned, blocks < 0, a cell or reg that is not positive and finite, a non-finite origin, a scale that is
 * not a positive finite power of two, cap not in [0, 2^62), 3 F cap scale >= 2^62, an unknown mode. */
#define DMVS_SIMPLIFY_QUADRIC 0
#define DMVS_SIMPLIFY_MEAN 1
int dmvs_mesh_cluster_verts_i64(const float* verts, const uint8_t* rgb, int64_t N, const int32_t* cluster, int64_t K, const double* origin,
                                double cell, int32_t* cnt, int64_t* pos_q, int64_t* rgb_sum, int32_t blocks, void* stream);
int dmvs_mesh_cluster_quadrics_i64(const float* verts, int64_t N, const int32_t* faces, int64_t F, const int32_t* cluster, int64_t K,
                                   const double* origin, double cell, double scale, double cap, int64_t* quad_q, int64_t* state, int32_t blocks,
                                   void* stream);
int dmvs_mesh_cluster_place_f32(int64_t K, const int32_t* cnt, const int64_t* pos_q, const int64_t* rgb_sum, const int64_t* quad_q,
                                const int64_t* cells, const double* origin, double cell, double scale, double reg, int32_t mode, float* out_verts,
                                uint8_t* out_rgb, int64_t* state, void* stream);
int dmvs_mesh_cluster_remap_i32(const float* verts, int64_t N, const int32_t* faces, int64_t F, const int32_t* cluster, int64_t K,
                                const float* new_verts, int32_t* out_faces, uint8_t* keep, int64_t* state, int32_t blocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DMVS_H */
