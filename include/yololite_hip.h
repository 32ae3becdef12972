/*
 * yololite_hip.h -- C ABI of the MI355X-native (gfx950) YoloLite inference hot path.
 *
 * The reference (Lillthorin/YoloLite-Official-Repo) is pure Python and has no FFI / operator
 * registry; its hot path sits behind plain Python calls.  This header is the boundary a native
 * replacement introduces.  Every entry point cites the reference interface it replaces
 * (paths relative to the reference repository root).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types cross the boundary.
 *   - All *_dev pointers are device (HBM) pointers owned by the CALLER (e.g. torch tensors'
 *     data_ptr()); the context owns weights, activations and workspaces.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are asynchronous
 *     on that stream and never synchronise implicitly, except yl_forward_timed.
 *   - Every function returns YL_OK (0) or a negative yl_status; nothing throws across the ABI.
 *   - One context per device; a context is not thread-safe (one stream at a time).
 *   - Deterministic: results are bitwise repeatable run to run (no floating-point atomics).
 *   - Arithmetic is fp32 throughout (the reference CPU path is fp32).
 */
#ifndef YOLOLITE_HIP_H
#define YOLOLITE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YL_ABI_VERSION 7
#define YL_MAX_LEVELS 8

typedef struct yl_ctx yl_ctx;
typedef int32_t yl_status;

enum {
  YL_OK = 0,
  YL_ERR_INVALID = -1,      /* bad argument / inconsistent model description          */
  YL_ERR_HIP = -2,          /* a HIP runtime call failed (see yl_last_error)          */
  YL_ERR_NOMEM = -3,        /* device or host allocation failed                       */
  YL_ERR_STATE = -4,        /* call not valid for this context (e.g. no layers)       */
  YL_ERR_UNSUPPORTED = -5,  /* valid request the kernels do not implement             */
  YL_ERR_CAPACITY = -6      /* a caller-provided buffer is too small                  */
};

/* activations fused into conv epilogues (reference: nn.ReLU / nn.SiLU in model_v2.py:21,34,132,299;
 * timm ReLU / ReLU6 inside the backbones) */
enum {
  YL_ACT_NONE = 0, YL_ACT_RELU = 1, YL_ACT_RELU6 = 2, YL_ACT_SILU = 3,
  YL_ACT_GELU = 4,      /* erf form, x * 0.5 * (1 + erf(x / sqrt 2)): timm convnextv2 `GlobalResponseNormMlp` (ABI v5)   */
  YL_ACT_RELU_LAB = 5   /* ReLU followed by timm's LearnableAffineBlock (hgnetv2 `ConvBNAct(use_lab=True)`): two scalars,
                           lab_scale * relu(v) + lab_bias; valid as `act` of YL_OP_STEM / YL_OP_CONV / YL_OP_DW only (ABI v5) */
};

/* layer kinds of the forward program */
enum {
  YL_OP_STEM = 0,  /* dense kxk conv reading the NCHW fp32 network input (Cin<=4), writes NHWC   */
  YL_OP_CONV = 1,  /* dense kxk conv (groups=1) on NHWC, optional depthwise prologue, fused
                      bias/act/residual/nearest-upsample-add epilogue, optional head-layout store  */
  YL_OP_DW = 2,    /* stand-alone depthwise kxk conv on NHWC with bias/act                         */
  YL_OP_STEMBLOCK = 3, /* fused network entry: stem 3x3 s2 (w,b,act) -> dense 3x3 s2 pad 1 (w2,b2,act2, cout c2)
                         -> optional 1x1 (w3,b3,act3, cout c3), NCHW input to NHWC output; the stem's
                         full-resolution activation (the largest tensor of the network) never reaches HBM  */
  YL_OP_SE = 4,    /* squeeze-excite gate of timm's SqueezeExcite (efficientnetv2 `ir_..._se0.25` blocks behind
                      model_v2.py:94-100): in_slot [B,H,W,cin] -> out_slot [B,1,1,cin],
                      gate = sigmoid(w2 . act(w . mean_hw(x) + b) + b2); w = conv_reduce [cout][cin][1][1], b [cout],
                      w2 = conv_expand [cin][cout][1][1], b2 [cin] (cout = the reduced width, c2 must equal cin).
                      The spatial mean is a fixed-order two-pass sum (no floating-point atomics: bitwise repeatable).
                      The gate multiplies the INPUT of the conv that names it in `scale_slot`.                     */
  /* ---- ABI v5: the op kinds of timm's hgnetv2 (configs/models/edge_xl.yaml:4) and convnextv2 (configs/v2_models/yololite_l.yaml:4)
   * feature extractors behind model_v2.py:94-100,266-272.  Element-wise / reduction passes, HBM-bound. */
  YL_OP_POOL = 5,  /* max-pool k x k, stride, window origin (oy*stride - pad_t, ox*stride - pad_l) over the input EXTENDED WITH
                      ZEROS (timm hgnet StemV2: F.pad(x, (0,1,0,1)) then MaxPool2d(2, 1)); cin == cout                        */
  YL_OP_COPY = 6,  /* channel-slice copy: in_slot [B,H,W,cin] -> channels [out_ch_off, out_ch_off + cin) of out_slot
                      [B,H,W,C_total]; torch.cat(..., dim=1) = one copy per input (hgnet StemV2 / HighPerfGpuBlock)            */
  YL_OP_LN = 7,    /* LayerNorm over the channels of every pixel (timm LayerNorm2d / nn.LayerNorm on channels-last):
                      (x - mean) / sqrt(var + eps) * w + b, biased variance, w / b [cin]; cin == cout                         */
  YL_OP_GRN = 8,   /* gate of timm's GlobalResponseNorm: in_slot [B,H,W,cin] -> out_slot [B,1,1,cin],
                      g = sqrt(sum_hw x^2) (fixed-order two-pass sum), gate = 1 + w * g / (mean_c(g) + eps), w [cin].  With the
                      gate as `scale_slot` of the following 1x1 conv and GRN's bias folded into that conv's bias by the host
                      (W2 . beta), the conv computes fc2(x + (beta + w * (x * n))) without writing the normalised tensor      */
  YL_OP_NHWC4 = 9  /* the NCHW fp32 network input [B,3,S,S] -> NHWC [B,S,S,4] (channel 3 = 0) for stems the MFMA stem kernel
                      does not cover (convnext: 4x4 stride 4, 96 outputs -> a YL_OP_CONV with cin = 4 follows); in_slot ignored */
};

/*
 * One fused layer.  Weights are HOST pointers in PyTorch layout with BatchNorm already folded
 * (w' = w * gamma/sqrt(var+eps), b' = beta - mean*gamma/sqrt(var+eps)); yl_create repacks them into
 * the MFMA fragment order and uploads them.  Replaces the nn.Conv2d / nn.BatchNorm2d / activation /
 * F.interpolate(nearest)+add / view-cat-permute sequences of scripts/model/model_v2.py:15-53,
 * 179-192,337-350 and of the timm backbone (model_v2.py:94-100,266-272).
 */
typedef struct {
  int32_t op;                 /* YL_OP_*                                                         */
  int32_t in_slot;            /* input tensor slot (ignored for YL_OP_STEM: reads the net input)  */
  int32_t out_slot;           /* output tensor slot, or -1 when head_level >= 0                   */
  int32_t res_slot;           /* tensor added after bias+act (residual), -1 = none                */
  int32_t up_slot;            /* tensor nearest-upsampled to the output size and added, -1 = none */
  int32_t head_level;         /* >=0: store as detection level [B,A,S,S,5+C] (cout = A*(5+C))     */
  int32_t cin, cout;
  int32_t k, stride, pad_t, pad_l;
  int32_t act;                /* YL_ACT_* applied after bias                                      */
  int32_t in_shift;           /* YL_OP_CONV, k>1, no prologue: the conv reads its input nearest-upsampled by
                                 2^in_shift (F.interpolate(scale_factor=2) folded into the tap addressing)   */
  int32_t dw_k;               /* YL_OP_CONV: 0 = none, else depthwise kxk prologue on input.  YL_OP_STEMBLOCK (round 6): 3 = the
                               * second conv is DEPTHWISE 3x3 stride 1 pad 1 (w2 [c1][1][3][3], c2 == cout == 32) followed by
                               * the 1x1 w3 -- timm's EfficientNet-Lite entry conv_stem -> blocks.0.0 as one launch            */
  int32_t dw_stride, dw_pad_t, dw_pad_l, dw_act;
  const float* w;             /* CONV/STEM: [cout][cin][k][k]; DW: [cout][1][k][k]                */
  const float* b;             /* [cout] or NULL                                                   */
  const float* dw_w;          /* [cin][1][dw_k][dw_k] or NULL                                     */
  const float* dw_b;          /* [cin] or NULL                                                    */
  /* YL_OP_STEMBLOCK: second and optional third conv of the fused entry block.
   * YL_OP_CONV with c2 > 0: fused inverted-residual block -- in_slot has c2 channels, w2/b2/act2 is the 1x1
   * EXPANSION [cin][c2][1][1] applied first, then the depthwise prologue (dw_*, stride 1 or 2) on the cin expanded
   * channels, then the 1x1 projection (w,b,act,res_slot); the expanded tensor never reaches HBM.  With up_slot >= 0
   * (cin channels) the nearest-upsampled tensor is added to the EXPANSION's output before act2 -- the FPN pair
   * "lateral 1x1 (+bias) + upsample-add, then depthwise smooth block" (model_v2.py:359-361) as one launch.
   * YL_OP_CONV with c3 > 0 (k > 1, no depthwise prologue, cout <= 96, c3 <= 32): a 1x1 conv w3/b3/act3 [c3][cout][1][1]
   * chained behind this conv in the same launch; out_slot then has c3 channels and the cout-channel tensor never
   * reaches HBM.
   * 0 / NULL otherwise. */
  int32_t c2, act2;           /* STEMBLOCK: 3x3 stride-2 pad-1 conv [c2][cout][3][3]              */
  int32_t c3, act3;           /* 1x1 conv: [c3][c2][1][1]; c3 = 0 -> absent                       */
  const float* w2;
  const float* b2;
  const float* w3;
  const float* b3;
  int32_t scale_slot;         /* YL_OP_CONV, 1x1 stride 1, no depthwise prologue: slot [B,1,1,cin] (a YL_OP_SE output) whose
                                 values multiply the conv's input per image and input channel before the GEMM
                                 (x * gate, then conv_pwl: timm InvertedResidual.forward); -1 = none                 */
  int32_t reserved0;          /* 0                                                                                */
  /* ---- ABI v5 */
  float lab_scale, lab_bias;  /* act == YL_ACT_RELU_LAB: the two scalars of the LearnableAffineBlock                              */
  float eps;                  /* YL_OP_LN / YL_OP_GRN                                                                            */
  int32_t out_ch_off;         /* YL_OP_COPY: first channel of out_slot written; 0 otherwise                                      */
} yl_layer;

/*
 * Model + detection-head geometry.  Mirrors what build_model_from_meta() (tools/infer.py:34-77)
 * derives from a checkpoint's meta and what forward() returns (model_v2.py:352-383):
 * level l is a tensor [B, level_anchors[l], level_size[l], level_size[l], 5+num_classes],
 * last-dim order [tx,ty,tw,th,tobj,cls_0..cls_{C-1}] (model_v2.py:345-350).
 */
typedef struct {
  int32_t abi_version;        /* YL_ABI_VERSION                                                   */
  int32_t img_size;           /* square network input S (x is [B,3,S,S] NCHW fp32)                */
  int32_t in_channels;        /* 3                                                                */
  int32_t num_classes;        /* C                                                                */
  int32_t num_masks;          /* NM: mask coefficients appended to every level row (0 = detector);
                                 level rows are [tx,ty,tw,th,tobj, cls_0..C-1, mc_0..NM-1]                */
  int32_t proto_slot;         /* activation slot holding the mask prototypes [B,PH,PW,NM] (-1 = none)   */
  int32_t num_levels;         /* L <= YL_MAX_LEVELS                                               */
  int32_t level_size[YL_MAX_LEVELS];
  int32_t level_anchors[YL_MAX_LEVELS];
  int32_t num_slots;          /* activation tensors                                               */
  const int32_t* slot_h;      /* [num_slots]                                                      */
  const int32_t* slot_w;
  const int32_t* slot_c;
  int32_t num_layers;         /* 0 = post-processing-only context                                 */
  const yl_layer* layers;
} yl_model_desc;

/* post-processing pipelines */
enum {
  YL_POST_MAIN = 0,      /* tools/infer.py:460-493  torchvision-nms semantics, per-class cap        */
  YL_POST_FALLBACK = 1,  /* tools/infer.py:247-389  greedy nms (+1e-6), min-side>=2, global top-k   */
  YL_POST_EVAL = 2       /* scripts/helpers/helpers.py:87-153  torchvision-nms semantics, no cap    */
};
enum { YL_CENTER_V8 = 0, YL_CENTER_SIMPLE = 1 };              /* utils_ms.py:83-88   */
enum { YL_WH_SOFTPLUS = 0, YL_WH_V8 = 1, YL_WH_EXP = 2 };     /* utils_ms.py:91-99   */
enum { YL_NMS_TORCHVISION = 0, YL_NMS_GREEDY = 1 };           /* tools/infer.py:134-163 */

typedef struct {
  int32_t mode;               /* YL_POST_*                                                        */
  float conf_thr;             /* keep iff score > conf_thr (strict)                               */
  float iou_thr;
  int32_t per_class_cap;      /* keep[:cap] per class (300 in the reference's nms()); <=0 = none  */
  int32_t topk;               /* FALLBACK only: global top-k by score; <=0 = none                 */
  int32_t max_out;            /* rows per image available in dets_dev / keep_idx_dev              */
  int32_t center_mode;        /* YL_CENTER_*                                                      */
  int32_t wh_mode;            /* YL_WH_*                                                          */
  const float* backmap_dev;   /* optional [B][5] = padx,pady,scale,w0,h0 (tools/infer.py:508-516) */
  int32_t fallback_nms;       /* YL_POST_FALLBACK only: the primitive behind nms() (tools/infer.py:134-152).
                                 YL_NMS_TORCHVISION (0, default) = what nms() runs when torchvision imports (a normal
                                 reference install); YL_NMS_GREEDY = its pure-torch loop (IoU + 1e-6, keep <= thr),
                                 taken when the import fails -- the situation in which tools/infer.py itself reaches
                                 decode_anchorfree_like_train (utils_ms.py:4 imports torchvision too)            */
} yl_post_cfg;

/* ---- lifetime ---------------------------------------------------------------------------------
 * yl_create replaces build_model_from_meta + load_state_dict + .to(device).eval()
 * (tools/infer.py:34-102): it validates the layer program, packs and uploads the weights.        */
yl_status yl_create(const yl_model_desc* desc, int32_t device_id, yl_ctx** out);
/* A second context of the SAME model on the same device: shares the packed weights (immutable after yl_create, freed by
 * the last owner), copies the current options, and owns everything a call touches -- activation arenas, post-processing
 * workspace, internal streams, cached hipGraphs.  Contexts are independent (one call at a time per context, any number of
 * contexts at once): a serving host keeps ONE CONTEXT PER BATCH IN FLIGHT and issues yl_predict for batch i on context
 * i % K from its own stream, so that the launch chain of batch i+1 overlaps the latency-bound tail of batch i instead of
 * waiting behind the join of its chunks (K = 2, one internal stream each: +10 % images/s on edge_n 640x640 B=64 against
 * back-to-back calls on one context).  The reference has no counterpart (one model object, one call at
 * a time: tools/infer.py:435-516); this is the C form of serving.ServingPipeline.  ABI v4.                          */
yl_status yl_clone(const yl_ctx* src, yl_ctx** out);
/* Do kernels on HIP streams `a` and `b` of device `device_id` RUN CONCURRENTLY?  ROCm hands every stream one of
 * GPU_MAX_HW_QUEUES hardware queues when it is created, round-robin over the streams the PROCESS has created so far (idle and
 * destroyed ones included), and two streams on one queue serialise.  Measured on MI355X / ROCm 7.2 (round 6): the same
 * two-batches-in-flight loop runs at 46.3 k or at 39 k images/s, and back-to-back calls on a two-stream context at 42.5 k or
 * 27.9 k, depending only on how many streams had been created before -- so neither the library nor a host can pick "a second
 * stream" blindly.  The probe launches a CHAIN of eight dependent 25 us spin kernels (one wave each) on each stream, interleaved,
 * and reads the wall clock: *overlap = 1 when both chains finished in less than 1.5 chain times (a good pair: ~231 us, an
 * aliasing pair: ~465 us; lone kernels overlap on every pair and show nothing).  Both streams are synchronised by the call; not capturable.  The library uses
 * it for its own chunk streams (a candidate that does not overlap the caller's stream and its siblings is replaced); a serving
 * host uses it for its per-batch streams (serving.ServingPipeline does).  `a` / `b`: hipStream_t, NULL = the null stream.  */
yl_status yl_streams_overlap(int32_t device_id, void* a, void* b, int32_t* overlap);
void yl_destroy(yl_ctx* ctx);
const char* yl_strerror(yl_status s);
const char* yl_last_error(const yl_ctx* ctx);   /* detail of the last failure on this context     */
int32_t yl_abi_version(void);

/* ---- forward ----------------------------------------------------------------------------------
 * Replaces model(x) (model_v2.py:352-377 / :194-224): x_dev is [B,3,S,S] NCHW fp32; level_out_dev
 * holds num_levels device pointers, level l receiving the contiguous tensor [B,A_l,S_l,S_l,5+C].  */
yl_status yl_forward(yl_ctx* ctx, const float* x_dev, int32_t batch, float* const* level_out_dev,
                     void* stream);
/* Same, but records a HIP event pair around every layer on `stream`, synchronises, and returns the
 * per-layer durations (ms) in layer_ms[num_layers].  Measurement aid for bench.py (roofline).      */
yl_status yl_forward_timed(yl_ctx* ctx, const float* x_dev, int32_t batch, float* const* level_out_dev,
                           void* stream, float* layer_ms);
/* With option "time_split" 1, yl_predict runs as ONE chunk on the caller's stream (eagerly, or with option "graph" as two
 * replayed hipGraphs: conv layers | post-processing) with a HIP event
 * before the conv layers, between the last conv layer and the NMS, and after the NMS; this call waits for the last
 * event and returns the two intervals: infer_ms (backbone + neck + heads, decode fused into the head epilogues) and
 * post_ms (per-class NMS + back-map) -- the pre / infer / post split of the reference's timing harness
 * (export/infer_onnx.py:152-244, README.md:182-189).  Measurement aid: the split costs the chunk overlap. */
yl_status yl_last_timing(yl_ctx* ctx, float* infer_ms, float* post_ms);
/* Bytes of activation memory the context holds for the batch of its last forward / predict call (one arena per
 * batch chunk, tensors placed by liveness; see option "reuse_slots").  0 before the first call. */
int64_t yl_activation_bytes(const yl_ctx* ctx);
/* Copies activation slot `slot` (NHWC fp32, [B,h,w,c]) of the last forward to dst_dev (testing aid).  With option
 * "reuse_slots" on (default) only tensors that are outputs of the network (mask prototypes) are guaranteed to still
 * hold their values after the call; set the option to 0 to inspect intermediate tensors. */
yl_status yl_read_slot(yl_ctx* ctx, int32_t slot, int32_t batch, float* dst_dev, void* stream);
/* Options: "graph" (0/1: replay the whole call from a captured hipGraph), "streams" (1..4 internal
 * streams the batch is split over; default 2), "tile_m" (conv M-tile hint), "lanes" (0/1, default 0: neck/head
 * layers of the coarser levels run on a side stream next to the finest level's chain),
 * "nms_groups" (0..4, default 0 = auto: NMS workgroups per image, classes dealt to the groups by load; auto takes 4 at
 * evaluation thresholds (conf < 0.05: thousands of survivors per image) and 1 otherwise; main / eval modes),
 * "hybrid" (0/1, default 0: high-resolution layers run as full-batch launches, only the run of <= 1/16-resolution
 * layers is split into batch chunks over the internal streams), "batch_levels" (0/1, default 1: head trunks /
 * head outputs of all pyramid levels in one launch each),
 * "fuse_decode" (0/1, default 1: yl_predict decodes inside the head-output convs; the raw level tensors are
 * then NOT materialised; a model with mask coefficients gets ONLY the coefficient columns of its level rows written --
 * what yl_masks / yl_masks_image read -- by a second plain 1x1 launch per head ("fuse_head" 1, single-anchor levels,
 * 5+C <= 96; otherwise the whole raw rows as before)),
 * "fuse_head" (0/1, default 1: run-time launch fusion of layer pairs whose shapes are instantiated.  With "fuse_decode"
 * and "batch_levels", a head branch -- depthwise 3x3 -> 1x1 trunk of 96 or 64 channels feeding the 1x1 head output --
 * runs trunk, output conv and decode as ONE launch for all levels; a depthwise 3x3 -> 1x1 expand layer followed by the
 * 1x1 project conv that is its only consumer (48 -> 192 -> 48) runs as one launch in every call.  The intermediate
 * tensors are then never written (yl_read_slot of those slots returns stale data).  Same results bit for bit),
 * "time_split" (0/1, default 0: see yl_last_timing), "pre_norm" (0/1: see yl_preprocess),
 * "reuse_slots" (0/1, default 1: activation tensors share memory by liveness inside one arena per batch chunk;
 * 0 keeps every tensor of the forward pass),
 * "winograd" (0/1/2, default 1: dense 3x3 stride-1 pad-1 convolutions with >= 16 input and output channels as Winograd
 * F(2x2,3x3) -- 16 instead of 36 multiplications per 2x2 output tile; fp32.  1 = every such layer (the dense FPN smooth
 * blocks of the YOLOLiteMS neck, model_v2.py:125-127; the ConvBnAct / fused-MBConv expansions of the efficientnetv2
 * backbones), 2 = only the >= 64-channel layers on the LARGEST grid they occur on (the finest pyramid level's smooth
 * block), 0 = direct convolution everywhere.  Winograd rounds differently from the direct convolution (not bit-identical
 * to it); against the fp32 CPU oracle its score error is no larger than the direct path's -- measured over 4 weight seeds x
 * 32 images x 8400 candidates at 640x640 on yololite_m: max |score - oracle score| 1.4-1.7e-5 (0), 1.4-1.7e-5 (2),
 * 0.9-1.6e-5 (1); on the efficientnetv2 yololite_m: 1.0-1.3e-5 (0), 0.7-1.2e-5 (1) -- i.e. >= 5.9x inside the 1e-4 bar
 * (profiles/r04_winograd_margin*.json, tools/wino_margin.py)),
 * "split_k" (0/1, default 0: depthwise -> 1x1 layers with 49..64 outputs on grids of <= 20 x 20 pixels split their k-blocks
 * over the four waves of a workgroup (one tile per workgroup, partial sums joined in LDS in a fixed order).  A latency
 * option for small batches: edge_n batch-1 forward -9 %, batch-64 throughput -0.7 %.  Chosen per context, never by the
 * batch size, so results stay batch-invariant and bitwise repeatable within a setting; between the settings they differ
 * by fp32 rounding (another summation order of the same products).  The pip API (api.YoloLite) turns it on),
 * "mfma_bf16" (0/1, default 0: reduced-precision inference mode, never the parity path -- every conv rounds the lane's
 * operands (weights and activations) to bf16 in registers and issues v_mfma_f32_16x16x16_bf16 with fp32 accumulation;
 * tensors stay fp32 in HBM; raw logits within 3e-2 of the level maximum),
 * "mfma_f16" (0/1, default 0: the same with fp16 operands on v_mfma_f32_16x16x16_f16 -- 11 mantissa bits instead of 8:
 * raw logits within 4e-3 of the level maximum; exclusive with "mfma_bf16"),
 * "store_f16" (0/1, default 0, round 6: "mfma_f16" AND fp16 ACTIVATION TENSORS IN HBM -- the storage side of the reference's
 * fp16 autocast, scripts/helpers/evaluate.py:399,415.  Every activation tensor between two launches is fp16 (arenas are
 * planned at 2 bytes per element, loads widen, stores round to nearest even, arithmetic and accumulation fp32); the network
 * input, the detection level tensors, the mask prototypes and the squeeze-excite gates stay fp32, and so do the packed
 * weights (they are L2 / Infinity-Cache resident: 2.3 MB for edge_n).  MFMA tiles are the 16x16x16 fp16 ones of "mfma_f16".
 * Kernels that stage activations by raw LDS-DMA copies (window-in-LDS depthwise, Winograd) give way to their tap-load
 * predecessors in this mode; models with the hgnetv2 / convnextv2 element-wise ops are refused at the first forward
 * (YL_ERR_UNSUPPORTED); yl_read_slot hands out fp32 and refuses fp16 slots.  Raw logits within 8e-3 of the level maximum
 * (measured 3.7e-3 .. 5.9e-3 at 640x640); exclusive with the other two modes; never the parity path). */
yl_status yl_set_option(yl_ctx* ctx, const char* name, int32_t value);
/* Current value of an option (the library's default if it was never written; values are stored clamped to the
 * option's range, e.g. "streams" 1..4).  YL_ERR_INVALID for an unknown name.  Also "dev_select" (default 0): a word of
 * DEVELOPER kernel-selection switches for A/B runs and the bitwise kernel-equivalence tests -- per context, carried
 * with every launch; never needed in production (bit 0: stand-alone depthwise through the one-output-per-lane kernel,
 * 1: no weight-streaming 1x1 kernel, 2: no staged-patch 3x3 s2 kernel, 3: producer/consumer depthwise kernel on every
 * shape it supports (with "tile_m" 7), 4: no wave-autonomous depthwise kernel, 5-6: streamed depthwise->1x1 kernel
 * variant (0 default, 1 one n-group per item, 2 off), 7-8: streamed dense 3x3 waves per workgroup (0 auto, 1 four,
 * 2 eight, 3 off for 4-n-tile layers), 9: two m-tiles per wave in its 4-wave form, 10: depthwise -> 1x1 layers on
 * grids of <= 20 x 20 pixels with one wave per tile instead of the split-K form, 11: Winograd layers through the first
 * kernel form (every transform position in one wave), 12-13: item shape of the position-split Winograd kernel (0 auto),
 * 14: depthwise 3x3 -> wide 1x1 layers with the taps from L1/L2 instead of the window-in-LDS kernel, 15: that kernel on
 * every grid it supports, 16: the fused head launch with the taps from L1/L2 (yl_conv_dpp_kernel) instead of the
 * window-in-LDS form (yl_conv_dpw_kernel), 17: small-channel dense 3x3 layers without the window-in-LDS kernel
 * (yl_conv_k3w_kernel), 18: workspace poison for the isolation tests -- the activation arenas, pinned slots, squeeze-excite
 * scratch and level buffers are allocated filled with 0xFF bytes (a NaN in fp32 and fp16) instead of zeros and refilled
 * with them, on the call's stream, at the start of every yl_forward* / yl_predict call: no result may depend on them),
 * 19: a UIB projection and the next block's 1x1 expansion as two launches instead of one chained launch
 * (yl_conv_dwx_kernel), 20: the fused head launch without the objectness skip -- every 4x4 tile runs the whole head-output
 * GEMM and the class scan, also where no candidate's sigmoid(objectness) exceeds conf_thr (same results bit for bit),
 * 21: two plain 1x1 convs around a tensor nothing else reads as two launches instead of one (yl_conv_pwx_kernel).
 * Read-only: "chain_launches", the number of chained launches the context has enqueued; "pwx_launches", the number of
 * 1x1-pair launches (yl_conv_pwx_kernel) enqueued; "head_skip_launches", the number
 * of fused head launches enqueued in the objectness-skip form; "head_skipped_tiles", the tiles those launches skipped since
 * "head_skip_count" (0/1, default 0, settable) was first switched on -- the kernel counts only while it is 1, and reading the
 * count waits for the device. */
yl_status yl_get_option(const yl_ctx* ctx, const char* name, int32_t* value);
/* Host-side query, no device needed: would yl_create accept a fused inverted-residual block (yl_layer with c2 > 0:
 * 1x1 expand c_in -> c_mid, depthwise dw_k x dw_k stride dw_stride, 1x1 project c_mid -> c_out) producing an
 * out_h x out_w tensor?  Returns 1 (workgroup-level-halo kernel yl_ir_kernel), 2 (per-wave kernel yl_uib_kernel:
 * stride 1, in/out grids multiples of 4) or 0 (not instantiated: emit the block as separate layers).  The host
 * "compiler" (program.py) asks this instead of mirroring the kernels' shape tables.                                */
int32_t yl_query_fused_block(int32_t c_in, int32_t c_mid, int32_t c_out, int32_t dw_k, int32_t dw_stride, int32_t out_h,
                             int32_t out_w);
/* Host-side query (additive), no device needed: which form of yl_ir_kernel runs a fused block that yl_query_fused_block
 * reports as 1, on `batch` fp32 images per launch with an in_h x in_w block input, an up_h x up_w FPN addend of c_mid channels
 * (0 x 0: none) and the activation ids of the projection (act), the depthwise conv (dw_act) and the expansion (act2)?
 * 0: the kernel has no instantiation for the shape, 1: its first form (any activation, 64-bit addresses), 2: its second form
 * (all three activations none / ReLU / ReLU6 and every tensor within 32-bit byte offsets; same results bit for bit).
 * shape, if not NULL, receives the seven template arguments of the instantiation: input k-blocks, n-tile bucket, dw k,
 * dw stride, m-tiles per wave, wave rows, wave columns.  The launcher takes the same decision from the same function.     */
int32_t yl_query_ir_form(int32_t c_in, int32_t c_mid, int32_t c_out, int32_t dw_k, int32_t dw_stride, int32_t out_h, int32_t out_w,
                         int32_t batch, int32_t in_h, int32_t in_w, int32_t up_h, int32_t up_w, int32_t act, int32_t dw_act,
                         int32_t act2, int32_t* shape);
/* Host-side query (ABI v5): can a depthwise dw_k x dw_k (stride dw_stride) conv on c_in channels be the PROLOGUE of the 1x1
 * conv c_in -> c_out that follows it (yl_layer.dw_k > 0; timm `conv_dw` -> `conv_pwl`, DWConvBlock model_v2.py:23-39), output
 * out_h x out_w?  2: the streamed-tap kernel takes it (yl_conv_dws_kernel: >= 192 depthwise channels, 7..22 output n-tiles,
 * 4x4-tileable output -- tf_efficientnet_lite stages 4-6), 1: the generic depthwise-prologue kernels do (taps + bias of all
 * channels within 32 KiB of LDS), 0: no -- emit the depthwise conv as its own YL_OP_DW layer.                          */
int32_t yl_query_dw_prologue(int32_t c_in, int32_t c_out, int32_t dw_k, int32_t dw_stride, int32_t out_h, int32_t out_w);
/* Host-side query (additive to ABI v7), no device needed: which Winograd F(2x2,3x3) kernel form runs a dense 3x3 stride-1 pad-1 conv c_in -> c_out
 * with an out_h x out_w output on `batch` images per launch (in_shift 1: the input is read nearest-upsampled by 2) under
 * option "winograd" 1 and the given "dev_select" value (bit 11, bits 12-13)?  0: none (the direct kernels run it), 1: the
 * first form (yl_conv_wino_kernel: every transform position in one wave), 2: the position-split form
 * (yl_conv_wino2_kernel) with *mt m-tiles x *nt n-tiles per item (mt / nt may be NULL; they are 0 unless 2 is returned).
 * Only layers whose output grid equals their (virtual) input grid carry a Winograd image, so out_h x out_w is also the size
 * of the tensor the kernels read.  The launcher takes the same decision from the same function; the tests ask which
 * instantiation a case ran.                                                                                              */
int32_t yl_query_wino_form(int32_t c_in, int32_t c_out, int32_t out_h, int32_t out_w, int32_t batch, int32_t in_shift,
                           int32_t dev_select, int32_t* mt, int32_t* nt);
/* Host-side query (additive to ABI v7), no device needed: which kernel family runs ONE fp32 layer with a depthwise dw_k x dw_k
 * (stride dw_stride, leading pads dw_pad_t / dw_pad_l) conv on c_in channels -- op YL_OP_CONV: as the prologue of the 1x1 conv
 * c_in -> c_out (yl_layer.dw_k > 0, no c2 / c3, a launch of its own); op YL_OP_DW: stand-alone (c_out == c_in; the layer's k,
 * stride and pads are passed as dw_k, dw_stride, dw_pad_*) -- from an in_h x in_w input to an out_h x out_w output on `batch`
 * images per launch, with the activation id `act` of the 1x1 conv (of the depthwise conv for YL_OP_DW) and a residual or not,
 * (GELU and ReLU + affine run in a pass behind the kernel, with the residual: the kernel is asked for neither) under the option
 * values "tile_m", "dev_select" and "split_k"?  Returns a YL_DWF_* id, or YL_DWF_NONE where yl_create would
 * refuse the layer or no kernel runs it.  args, if not NULL, receives the template arguments of the instantiation (unused
 * entries 0):
 *   DWK        yl_conv_dwk_kernel<NT, GW, NW>                DWL         yl_conv_dwl_kernel<NTT>
 *   DWS        yl_conv_dws_kernel<NT, GW, DK, DS, NW>        DWT         yl_conv_dwt_kernel<NT, DK, DS, MT, WL, 1>
 *   DWT_SPLITK yl_conv_dwt_kernel<4, DK, DS, 1, false, 4>    DWC         yl_conv_dwc_kernel<DK, DS, NTW>
 *   DWH        yl_conv_dwh_kernel<NT, DK, DS>                MFMA        yl_conv_mfma_kernel<NT, MT, MODE>, then the k-steps of
 *   DW_TILE    yl_dw_tile_kernel<K, S>                                   1x1 weights resident in LDS (fewer than c_in / 16: they stream)
 *   DW         yl_dw_kernel
 * The launchers (yl_launch_conv_multi, yl_launch_dw) take the same decision from the same functions; the tests ask which
 * instantiation a case ran.  Launches that join the layer with a neighbour (the fused head and pair launches, the chained
 * projection) are decided before these and are not reported here.                                                        */
enum {
  YL_DWF_NONE = 0, YL_DWF_DWK = 1, YL_DWF_DWL = 2, YL_DWF_DWS = 3, YL_DWF_DWT = 4, YL_DWF_DWT_SPLITK = 5, YL_DWF_DWC = 6,
  YL_DWF_DWH = 7, YL_DWF_MFMA = 8, YL_DWF_DW_TILE = 9, YL_DWF_DW = 10
};
int32_t yl_query_dw_form(int32_t op, int32_t c_in, int32_t c_out, int32_t dw_k, int32_t dw_stride, int32_t dw_pad_t, int32_t dw_pad_l,
                         int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w, int32_t batch, int32_t act, int32_t has_res,
                         int32_t tile_m, int32_t dev_select, int32_t split_k, int32_t* args);

/* ---- pre-processing ----------------------------------------------------------------------------
 * Replaces letterbox() + cv2.cvtColor + /255 + (x-mean)/std + transpose of tools/infer.py:121-131,446-453
 * for a batch: `packed_u8_dev` holds the BGR uint8 HWC images back to back, `imgs_dev` one descriptor
 * per image (the caller computes the letterbox geometry exactly like the reference: scale=min(S/h,S/w),
 * nh,nw=int(round(.)), top=(S-nh)//2, left=(S-nw)//2).  x_dev receives [B,3,S,S] fp32.
 * Option "pre_norm" 1 switches the normalisation arithmetic to the evaluate path's (tools/evaluate.py:57-72 ->
 * scripts/data/augment.py:153-171: LongestMaxSize + PadIfNeeded give the SAME geometry -- scale S/max(h,w),
 * round-half-even sizes, floor-half padding, border 114 -- and A.Normalize computes (x - 255*mean) * (1/(255*std))
 * in float32 instead of (x/255 - mean)/std).                                                          */
typedef struct {
  int64_t offset;             /* byte offset of image b in packed_u8_dev                          */
  int32_t h0, w0;             /* source size                                                      */
  int32_t nh, nw;             /* resized size inside the letterbox                                */
  int32_t top, left;          /* padding                                                          */
} yl_pre_image;
yl_status yl_preprocess(yl_ctx* ctx, const uint8_t* packed_u8_dev, const yl_pre_image* imgs_dev, int32_t batch,
                        float* x_dev, void* stream);

/* ---- decode -----------------------------------------------------------------------------------
 * Replaces decode_preds_anchorfree (scripts/helpers/utils_ms.py:26-123): levels -> box [B,N,4]
 * xyxy pixels clamped to [0,S-1], obj [B,N,1] logits, cls [B,N,C] logits; N = sum A_l*S_l^2.        */
yl_status yl_decode(yl_ctx* ctx, const float* const* levels_dev, int32_t batch, int32_t center_mode,
                    int32_t wh_mode, float* box_dev, float* obj_dev, float* cls_dev, void* stream);

/* Forward + decode in ONE call: the exported "decoded" wire format of the reference (export/export_onnx.py:283-296:
 * boxes_xyxy [B,N,4], obj_logits [B,N,1], cls_logits [B,N,C]) straight from the network input; the raw level tensors
 * stay in the context's own buffers (not handed out).  Same arithmetic as yl_forward followed by yl_decode.       */
yl_status yl_forward_decoded(yl_ctx* ctx, const float* x_dev, int32_t batch, int32_t center_mode, int32_t wh_mode,
                             float* box_dev, float* obj_dev, float* cls_dev, void* stream);

/* ---- post-processing --------------------------------------------------------------------------
 * Replaces the score/threshold/per-class-NMS/(top-k)/(back-map) code of tools/infer.py:460-516
 * (MAIN), tools/infer.py:247-389 (FALLBACK) and helpers.py:87-136 (EVAL).
 * dets_dev  [B][max_out][6] = x1,y1,x2,y2,score,class   (class asc, score desc; FALLBACK after a
 *           fired top-k: score desc)
 * counts_dev[B] = number of detections produced (may exceed max_out: rows beyond it are dropped)
 * keep_idx_dev optional [B][max_out] candidate index n of every detection (NULL to skip).          */
yl_status yl_postprocess(yl_ctx* ctx, const float* const* levels_dev, int32_t batch,
                         const yl_post_cfg* cfg, float* dets_dev, int32_t* counts_dev,
                         int32_t* keep_idx_dev, void* stream);
/* forward + postprocess (YoloLite.predict hot loop).  With option "fuse_decode" (default) the raw head rows
 * never reach memory; set it to 0 to have the context's level buffers filled as by yl_forward.
 * keep_idx_dev: optional [B][max_out] candidate indices (needed by yl_masks), NULL to skip.          */
yl_status yl_predict(yl_ctx* ctx, const float* x_dev, int32_t batch, const yl_post_cfg* cfg,
                     float* dets_dev, int32_t* counts_dev, int32_t* keep_idx_dev, void* stream);

/* ---- multi-GPU exchange ----------------------------------------------------------------------
 * The reference is single-device; sharding the batch over GPUs needs exactly ONE exchange per step: an all-gather
 * of the packed per-rank result.  Every rank runs yl_predict on its shard with dets_dev / counts_dev pointing INTO
 * one flat buffer  local_dev = [ dets: b*max_out*6 floats | counts: b int32 ]  (row_floats = b*max_out*6 + b; equal
 * shards), then this call issues ncclAllGather(local_dev -> all_dev[world][row_floats]) on `stream` -- asynchronous,
 * no pack / unpack kernels.  `nccl_comm` is the caller's ncclComm_t (RCCL).  RCCL is resolved at run time from the
 * libraries already loaded in the process (YL_ERR_UNSUPPORTED if none is).  Python hosts use torch.distributed
 * instead (yololite_amd.dist.DetGatherer: same buffer layout). */
yl_status yl_allgather_dets(yl_ctx* ctx, void* nccl_comm, const float* local_dev, int64_t row_floats, float* all_dev,
                            void* stream);

/* ---- instance masks (BUILD-DEFINED: the reference repository contains no mask code; parity unpinned) --
 * For detection i of image b (candidate keep_idx[b][i] of the levels of the last yl_forward/yl_predict on
 * this context, box = its decoded box in network-input pixels):
 *     m(y,x) = sigmoid( sum_k mc_k * proto[b][y][x][k] )          proto = slot `proto_slot`, [PH,PW,NM]
 *     mask(y,x) = m(y,x) > thr  and  x1*PW/S <= x < x2*PW/S  and  y1*PH/S <= y < y2*PH/S
 * masks_dev: uint8 [B][max_out][PH][PW] (rows >= counts[b] are left untouched).                       */
yl_status yl_masks(yl_ctx* ctx, const float* const* levels_dev, int32_t batch, const int32_t* counts_dev,
                   const int32_t* keep_idx_dev, int32_t max_out, float thr, uint8_t* masks_dev, void* stream);
/* Masks at IMAGE resolution -- the form the pip API returns (README.md:38-42: results['masks']).  BUILD-DEFINED like
 * yl_masks.  For detection i of image b (row dets_dev[b][i] = x1,y1,x2,y2,.. as written by yl_predict / yl_postprocess,
 * i.e. ALREADY back-mapped when `backmap_dev` was given there; candidate keep_idx[b][i]) and every pixel (y,x) of the
 * output grid of image b (h_b x w_b = out_hw_dev[b]: the original image, or S x S without back-map):
 *     xs = (x + 0.5) * scale + padx,  ys = (y + 0.5) * scale + pady        letterbox coordinate of the pixel centre
 *                                                                          (scale 1, pad 0 without backmap_dev)
 *     u  = max(xs, 0) * (PW / S) - 0.5 clamped at 0,  v likewise           source index of a bilinear PW/S resize,
 *                                                                          align_corners = false, edges replicated
 *     m  = bilinear interpolation of sigmoid(mc . proto[b]) at (v, u)      4 prototype pixels
 *     mask(y,x) = m > thr  and  x1 <= x < x2  and  y1 <= y < y2
 * Output of image b starts at masks_dev + mask_off_dev[b] bytes: [min(counts[b], max_out)][h_b][row] with row = w_b
 * uint8 (packed = 0) or ceil(w_b / 32) uint32 words, bit k of word j = pixel 32 j + k (packed = 1).
 * max_h / max_w: the largest h_b / w_b of the batch.  The caller sizes masks_dev from the counts, or gives every
 * image a fixed capacity of max_out masks (mask_off_dev[b] = b * max_out * h * row: no host read of the counts, the
 * call stays asynchronous).  packed = 1 needs mask_off_dev[b] % 4 == 0; 16-byte aligned offsets give full-width
 * stores.  Limits: prototype width PW <= 1024 (img_size <= 4096), batch <= 8192 (YL_ERR_HIP / invalid value beyond).
 * Every byte of the [min(counts[b], max_out)][h_b][row] block of image b is written (zeros outside the boxes). */
yl_status yl_masks_image(yl_ctx* ctx, const float* const* levels_dev, int32_t batch, const float* dets_dev,
                         const int32_t* counts_dev, const int32_t* keep_idx_dev, int32_t max_out, float thr,
                         const float* backmap_dev, const int32_t* out_hw_dev, const int64_t* mask_off_dev, int32_t max_h,
                         int32_t max_w, int32_t packed, uint8_t* masks_dev, void* stream);
/* Replaces nms(boxes, scores, iou_th, max_det) (tools/infer.py:134-152): keep_dev[max_det] receives
 * the kept indices in score-descending order, count_dev[0] their number (<= max_det).              */
yl_status yl_nms(yl_ctx* ctx, const float* boxes_dev, const float* scores_dev, int32_t n, float iou_thr,
                 int32_t nms_impl, int32_t max_det, int32_t* keep_dev, int32_t* count_dev, void* stream);

/* ---- evaluate-path consumers ----------------------------------------------
 * The two O(detections x ground truths) matching loops of the reference's evaluation, as device
 * kernels.  They take no context (stateless; current HIP device); all pointers are device pointers.
 *
 * yl_eval_match replaces the greedy per-(image, category) matching of build_curves_from_coco
 * (scripts/data/p_r_f1.py:31-78 and :100-118).  Keys k = 0..num_keys-1 are the distinct
 * (image_id, category_id) pairs; detections of key k are rows det_off[k]..det_off[k+1]-1 of det_xywh,
 * ALREADY in score-descending stable order; ground truths likewise through gt_off.  Boxes are
 * [x,y,w,h] float64 exactly as the reference's python floats; IoU is evaluated in float64 with the
 * reference's operation order (iou_xywh, p_r_f1.py:31-41).  For every detection, in order: the
 * not-yet-matched ground truth with the largest IoU > 0 (first index on ties) is taken; if that IoU
 * >= iou_thr the detection is a true positive and the ground truth becomes matched.
 *   tp_dev[Nd]     1 = true positive, 0 = false positive
 *   match_dev[Nd]  index (within the key) of the matched ground truth, -1 if none   (may be NULL)
 *   gt_matched_dev[Ng]  scratch AND output: zeroed by the call, 1 where a ground truth was matched */
yl_status yl_eval_match(const double* det_xywh_dev, const int32_t* det_off_dev, const double* gt_xywh_dev,
                        const int32_t* gt_off_dev, int32_t num_keys, int32_t num_gt, double iou_thr,
                        uint8_t* tp_dev, int32_t* match_dev, uint8_t* gt_matched_dev, void* stream);
/* The 0..1 confidence sweep of build_curves_from_coco (p_r_f1.py:96-124): for every threshold
 * thr[s] (ascending float64, the reference uses np.linspace(0,1,steps)) the number of true / false
 * positives among the counted detections with score >= thr[s].  Because the greedy matching of a
 * score-descending list is prefix-stable, these are suffix sums of a histogram of the tp flags of ONE
 * matching pass (yl_eval_match) -- the reference re-runs the matching per threshold.
 *   counted_dev[n] 1 = detection takes part in the sweep (its key has ground truth), may be NULL = all
 *   tp_ge_dev[steps], fp_ge_dev[steps]  int32 outputs                                                   */
yl_status yl_eval_sweep(const double* score_dev, const uint8_t* tp_dev, const uint8_t* counted_dev, int32_t n,
                        const double* thr_dev, int32_t steps, int32_t* tp_ge_dev, int32_t* fp_ge_dev,
                        void* stream);
/* Replaces the matching loops of create_confusion_matrix (scripts/helpers/evaluate.py:96-153).
 * Images i = 0..num_images-1 are the images that HAVE ground truth; their detections (already
 * filtered by score >= score_thresh and in score-descending stable order) are rows
 * det_off[i]..det_off[i+1]-1; boxes are float32 [x1,y1,x2,y2] as produced by the reference's
 * xywh_to_xyxy (:23-25); IoU in float32 with iou_matrix's operation order (:27-57, union clipped at
 * 1e-6).  Class-agnostic: the best ground truth is the FIRST argmax over all ground truths of the
 * image; true positive iff its IoU >= iou_thr and it is unmatched (:128-140).
 *   cm_dev[(C+1)*(C+1)] int32, row = true class, column = predicted class, index C = background;
 *   zeroed by the call.                                                                               */
yl_status yl_eval_confusion(const float* det_xyxy_dev, const int32_t* det_cls_dev, const int32_t* det_off_dev,
                            const float* gt_xyxy_dev, const int32_t* gt_cls_dev, const int32_t* gt_off_dev,
                            int32_t num_images, int32_t num_gt, int32_t num_classes, float iou_thr,
                            int32_t* cm_dev, uint8_t* gt_matched_dev, void* stream);

/* ---- COCO bbox mAP (pycocotools 2.0 COCOeval, iouType="bbox"; the reference's _coco_eval_from_lists,
 * scripts/helpers/helpers.py:155-227).  evaluateImg + accumulate on the device; the host groups, sorts and
 * counts, and summarize() stays a numpy mean over the returned arrays.  Behaviour restated (boxes [x,y,w,h]
 * float64 exactly as given, finite):
 *   IoU = maskApi bbIou: w = fmin(dw+dx, gw+gx) - fmax(dx,gx) (0 if <= 0), h likewise, i = w*h,
 *         u = crowd ? dw*dh : (dw*dh + gw*gh) - i, iou = i/u
 *   gtIg(a) = crowd || area < lo || area > hi (both bounds inclusive; area = the annotation's field)
 *   per threshold t, detections in order: among the unmatched (or crowd) ground truths with IoU >=
 *   min(t, 1-1e-10), the non-ignored ones with the largest IoU, LAST index on ties; only if there is none,
 *   the same among the ignored ones.  dtm != 0 iff a ground truth with a nonzero id was taken;
 *   dtIg = gtIg[m] if one was taken, or (dtm == 0 and the detection's w*h is outside [lo, hi]). */
#define YL_COCO_GT_CROWD 1u       /* gt_flags: iscrowd                                        */
#define YL_COCO_GT_ID_NONZERO 2u  /* gt_flags: annotation id != 0 (pycocotools tests dtm != 0) */
#define YL_COCO_DT_MATCHED 1u     /* dt_flags: dtm != 0                                       */
#define YL_COCO_DT_IGNORED 2u     /* dt_flags: dtIgnore                                       */
/* evaluateImg for every key k = 0..num_keys-1 (an (image, category) pair with detections) and every
 * (area range a, threshold t).  Detections of key k are rows det_off[k]..det_off[k+1]-1 of det_xywh, sorted
 * by -score (stable) and already truncated to maxDets[-1]; its ground truths are rows gt_off[k].. in list
 * order, with gt_area and gt_flags (YL_COCO_GT_*).  area_rng[num_areas][2], iou_thrs[num_thrs] (<= 32) are
 * the COCOeval Params arrays as the host holds them.
 *   dt_flags_dev[num_areas][num_thrs][num_det]  YL_COCO_DT_* bits per detection
 *   gt_matched_dev[num_areas][num_gt]           uint32 scratch, zeroed by the call                          */
yl_status yl_eval_coco_match(const double* det_xywh_dev, const int32_t* det_off_dev, const double* gt_xywh_dev,
                             const double* gt_area_dev, const uint8_t* gt_flags_dev, const int32_t* gt_off_dev,
                             int32_t num_keys, int32_t num_det, int32_t num_gt, const double* area_rng_dev,
                             int32_t num_areas, const double* iou_thrs_dev, int32_t num_thrs, uint8_t* dt_flags_dev,
                             uint32_t* gt_matched_dev, void* stream);
/* accumulate for every (category k, area a, maxDet m, threshold t).  Entries cat_off[k]..cat_off[k+1]-1 of
 * order_dev are the detections (rows of yl_eval_coco_match) of category k in accumulate order: -score, then
 * image id, then rank within the key (a stable sort); rank_dev[i] is entry i's rank within its key, and an
 * entry counts for maxDets[m] iff rank < maxDets[m].  npig[k][a] = non-ignored ground truths.  With
 * tp/fp = prefix counts of (matched, not ignored) / (not matched, not ignored):
 *   rc = tp/npig, pr = tp/((fp+tp) + 2^-52), recall = rc[-1] (0 without detections),
 *   precision[r] = max{pr[i] : rc[i] >= rec_thrs[r]} (0 if none)   == the envelope + searchsorted of COCOeval
 *   precision_dev[num_thrs][num_rec][num_cats][num_areas][num_max_dets], recall_dev[num_thrs][num_cats][num_areas]
 *   [num_max_dets] float64, -1 where npig == 0.  rec_thrs ascending, num_rec <= 256.                       */
yl_status yl_eval_coco_accumulate(const int32_t* order_dev, const int32_t* rank_dev, const int32_t* cat_off_dev,
                                  const uint8_t* dt_flags_dev, int32_t num_det, const int32_t* npig_dev,
                                  int32_t num_cats, int32_t num_areas, int32_t num_thrs, const int32_t* max_dets_dev,
                                  int32_t num_max_dets, const double* rec_thrs_dev, int32_t num_rec,
                                  double* precision_dev, double* recall_dev, void* stream);

/* ---- the reference's LossAF (scripts/loss/loss.py:283-436), fp32: the forward, and its backward further down --
 * SimOTA-style assignment (centre mask AND level gate, orphan rescue, six-term cost, dynamic k from the topk_limit
 * largest IoUs, conflicts to the smallest cost / lowest box), then per image box = lambda_box * mean(1 - CIoU),
 * cls = lambda_cls * mean(cross-entropy with label smoothing) over the positives, obj = lambda_obj * (mean BCE of
 * the positives against clamp(IoU, 0, 1) + mean of the K = min(max(64, 3 * positives), negatives) largest BCE of
 * the rest against 0); images without boxes or without positives contribute the hard-negative term only.  The
 * batch result is the SUM over images; pos = images with positives / batch.  yl_loss_af itself keeps no state
 * for a backward pass (yl_loss_af_train does).
 * cfg carries the constructor's arguments as given (area_cells_min / area_cells_max BEFORE area_tol is applied).
 * topk_limit must be 1..YL_LOSS_MAX_TOPK; one anchor per cell only (the reference's anchor grid has no room for
 * more): YL_ERR_UNSUPPORTED otherwise.  The reference's focal / gamma / alpha arguments have no effect in its
 * forward and no field here. */
#define YL_LOSS_MAX_TOPK 64
typedef struct yl_loss_cfg {
  int32_t num_classes;        /* must equal the context's                                         */
  int32_t img_size;           /* must equal the context's                                         */
  int32_t center_mode;        /* YL_CENTER_*  (train-time decode, unclamped: LossAF._decode)      */
  int32_t wh_mode;            /* YL_WH_*                                                          */
  int32_t topk_limit;
  float lambda_box, lambda_obj, lambda_cls, assign_cls_weight, center_radius_cells, cls_smoothing, area_cells_min,
      area_cells_max, area_tol, size_prior_w, ar_prior_w, iou_cost_w, center_cost_w;
} yl_loss_cfg;
/* levels_dev: the raw level tensors as yl_forward writes them.  Ground truths of the batch as one flat list:
 * gt_xyxy_dev[num_gt][4] in network-input pixels, gt_label_dev[num_gt] in [0, num_classes), gt_off_dev[batch + 1]
 * ascending with gt_off[0] = 0 and gt_off[batch] = num_gt (image b owns rows gt_off[b] .. gt_off[b+1]-1; the three
 * may be NULL when num_gt == 0).  Outputs (device): per_image_dev[batch][3] = box, obj, cls of each image and
 * assign_dev[batch][N] = matched row of gt_* or -1 (either may be NULL), out4_dev[4] = box, obj, cls, pos.
 * Enqueues three kernels and one memset on `stream`; no synchronisation, no copy to the host.  Sums run in an
 * order fixed by the data: equal inputs give equal bits, and an image's parts do not depend on its batch. */
yl_status yl_loss_af(yl_ctx* ctx, const float* const* levels_dev, int32_t batch, const float* gt_xyxy_dev,
                     const int32_t* gt_label_dev, const int32_t* gt_off_dev, int32_t num_gt, const yl_loss_cfg* cfg,
                     float* per_image_dev, int32_t* assign_dev, float* out4_dev, void* stream);

/* ---- the loss's backward pass: d(box + obj + cls)/d(level tensors), in the level tensors' own layout ---------
 * Nothing of the assignment is differentiated in the reference (top-k indices, .int() and boolean masks carry no
 * gradient, the objectness target is detached), so the gradient is closed-form per anchor:
 *   positive, columns 0-3      lambda_box / npos * d(1 - CIoU)/d(x1,y1,x2,y2) chained through the train-time decode
 *                              (alpha of CIoU is a constant; an exp size outside its clamp [-10, 8] has derivative 0)
 *   positive, column 4         lambda_obj / npos * (sigmoid(x) - clamp(IoU, 0, 1))
 *   positive, columns 5..5+C-1 lambda_cls / npos * (softmax(z) - ((1 - e) * onehot + e / C));  +0 when C = 1
 *   selected negative, col 4   lambda_obj / K * sigmoid(x)
 *   every other element        +0.0 (unselected negatives, mask-coefficient columns)
 * all times grad_out.  The selected negatives are the K = min(max(64, 3 * npos), N - npos) largest BCE(x, 0) of the
 * non-positives, decided by the same fp32 term the forward's radix select saw.  TIES: of the entries whose term equals
 * the K-th largest bit for bit, the ones with the lowest anchor index are selected (torch.topk leaves that choice
 * unspecified).  KINKS follow torch: clamp passes the gradient at its boundary, binary max / min split it between
 * equal arguments.  The non-zero rows are evaluated in float64 from the fp32 logits and rounded once.
 *
 * yl_loss_af_train is yl_loss_af with two REQUIRED outputs that the backward needs: assign_dev[batch][N] and
 * sel_dev[batch][4] int32 = npos, K, the bits of the K-th largest negative term, and the tie cut (entries equal to the
 * K-th term are selected when their anchor index is below it).  Same numbers as yl_loss_af, bit for bit.
 * yl_loss_af_backward reads those two, the same levels / ground truths / cfg, and grad_out_dev (ONE float in device
 * memory, never read on the host) and writes grad_levels_dev[l], one tensor per level shaped like levels_dev[l]: every
 * element exactly once, none read.  One kernel on `stream`; no synchronisation, no atomics: equal inputs give equal
 * bits, and an image's rows do not depend on its batch. */
yl_status yl_loss_af_train(yl_ctx* ctx, const float* const* levels_dev, int32_t batch, const float* gt_xyxy_dev,
                           const int32_t* gt_label_dev, const int32_t* gt_off_dev, int32_t num_gt,
                           const yl_loss_cfg* cfg, float* per_image_dev, int32_t* assign_dev, int32_t* sel_dev,
                           float* out4_dev, void* stream);
yl_status yl_loss_af_backward(yl_ctx* ctx, const float* const* levels_dev, int32_t batch, const float* gt_xyxy_dev,
                              const int32_t* gt_label_dev, const int32_t* gt_off_dev, int32_t num_gt,
                              const yl_loss_cfg* cfg, const int32_t* assign_dev, const int32_t* sel_dev,
                              const float* grad_out_dev, float* const* grad_levels_dev, void* stream);

/* ---- Kalman-SORT tracker bank (reference tools/tracker.py:9-326) -------------
 * The reference's KalmanSortTracker follows ONE stream on the host.  A yl_tracker holds `num_streams`
 * independent trackers on the device (capacity `max_tracks` tracks each); yl_track_update advances all of
 * them by one frame from the packed detections of yl_predict / yl_postprocess without a host round trip:
 *   dets_dev   [S][max_out][6] = x1,y1,x2,y2,score,class      counts_dev [S] (clamped to max_out)
 * Semantics per stream = KalmanSortTracker.update(boxes, scores, classes) (tools/tracker.py:211-326):
 * predict, greedy IoU assignment (descending IoU, optional same-class mask, stop below iou_threshold),
 * Kalman update, new tracks for unmatched detections (ids from 1, detection order), drop tracks unseen
 * for more than max_age frames, report tracks updated this frame with hits >= min_hits, in list order.
 * Constructor defaults of the reference: iou_threshold 0.3, max_age 15, min_hits 2, match_by_class 1.
 * Outputs (device): out_id/out_cls [S][max_tracks] int32, out_box [S][max_tracks][4] xyxy,
 * out_score [S][max_tracks], out_count [S].  fp32 like the reference; the 7x7 / 4x4 products are not
 * summed in BLAS order, so boxes agree to rounding (tests: 1e-3 px), ids / classes / counts exactly.
 * Equal IoUs are taken in flat-index order (numpy's argsort leaves ties unspecified).
 * Tracks beyond max_tracks are not created; yl_track_stats reports how many were lost.                */
typedef struct yl_tracker yl_tracker;
yl_status yl_track_create(int32_t device, int32_t num_streams, int32_t max_tracks, float iou_threshold,
                          int32_t max_age, int32_t min_hits, int32_t match_by_class, yl_tracker** out);
void yl_track_destroy(yl_tracker* t);
/* reset() of the reference (tools/tracker.py:191-193) for one stream, or all with stream_index = -1 */
yl_status yl_track_reset(yl_tracker* t, int32_t stream_index, void* stream);
yl_status yl_track_update(yl_tracker* t, const float* dets_dev, const int32_t* counts_dev, int32_t max_out,
                          int32_t* out_id_dev, float* out_box_dev, int32_t* out_cls_dev, float* out_score_dev,
                          int32_t* out_count_dev, void* stream);
/* Grows the per-stream capacity to new_max_tracks (<= 4096), keeping every stream's state; synchronises the
 * device.  The output tensors of yl_track_update must then have the new row length.  No-op when not larger. */
yl_status yl_track_grow(yl_tracker* t, int32_t new_max_tracks);
/* synchronises the device; host arrays [num_streams] (either may be NULL) */
yl_status yl_track_stats(yl_tracker* t, int32_t* ntracks_host, int32_t* overflow_host);

/* ---- the training step's tail (reference tools/train.py:352-359 and ModelEMA.update, :45-57) -----------------
 * scaler.unscale_, clip_grad_norm_, scaler.step(AdamW | Adam | SGD), scaler.update and ema.update(model) for ALL
 * tensors of a model as three launches.  A yl_train handle needs no yl_ctx.  fp32, contiguous tensors on one device
 * only; every tensor may start at any 4-byte boundary (a pointer that does not: YL_ERR_UNSUPPORTED).
 *
 * One yl_train_segment per state_dict entry, in state_dict order:
 *   parameter          param / grad (may be NULL) / state0 / state1 / ema (NULL = no EMA), count elements, group
 *                      AdamW, Adam: state0 = exp_avg, state1 = exp_avg_sq.  SGD: state0 = momentum_buffer, state1 unused
 *   YL_TRAIN_SEG_EMA_ONLY  floating buffer (BatchNorm running statistics): param = the model's buffer (read only),
 *                      ema = the EMA's; no gradient, no state
 *   YL_TRAIN_SEG_BYTES     non-floating entry (num_batches_tracked): `count` BYTES are copied from param to ema
 * Update rules: torch 2.10's single-tensor implementations (torch/optim/adam.py, sgd.py; foreach=False, not
 * capturable, no amsgrad / maximize / dampening), with g = fp32(grad * inv_scale) * clip,
 * clip = min(1, max_norm / (norm + 1e-6)) or 1 when max_norm <= 0:
 *   AdamW  p *= 1 - lr*wd;  m += (g - m)(1 - b1);  v = v*b2 + (1 - b2) g*g;
 *          p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps)
 *   Adam   g += wd*p, then as AdamW without the decay
 *   SGD    g += wd*p;  buf = g on the tensor's first applied step, momentum*buf + g afterwards;
 *          p -= lr * (nesterov ? g + momentum*buf : buf)        (momentum 0: p -= lr*g, the buffer is not touched)
 *   EMA    ema = ema*d + value*(1 - d), value = the parameter just written, or the model's buffer
 * Everything after the fp32 unscale product is evaluated in float64 from the fp32 operands and rounded once per
 * stored value.  `step` is the TENSOR's own count (fp32, device memory), advanced only when that tensor has a
 * gradient in a step that is not skipped.  Gradients are READ ONLY: unlike torch, the unscaled and clipped values are
 * not written back into .grad.
 * Skipped step (amp and a non-finite gradient element): parameters, states and step counts keep their bits; the EMA
 * and the integer copies still run (the reference calls ema.update after scaler.step regardless); scale *= backoff,
 * tracker = 0.  Otherwise tracker += 1 and, when it reaches growth_interval, scale *= growth (kept if not finite, as
 * torch does), tracker = 0.  Without amp the scale is 1, stays 1, and nothing is skipped.
 * Deterministic: the norm is a float64 sum in an order fixed by the segment table, rounded once to fp32; no atomics;
 * equal inputs give equal bits. */
enum { YL_TRAIN_ADAMW = 0, YL_TRAIN_ADAM = 1, YL_TRAIN_SGD = 2 };
#define YL_TRAIN_SEG_EMA_ONLY 1u
#define YL_TRAIN_SEG_BYTES 2u
#define YL_TRAIN_MAX_GROUPS 8
#define YL_TRAIN_CHUNK_DEFAULT 4096
#define YL_TRAIN_STATE_WORDS 8
typedef struct yl_train yl_train;
typedef struct yl_train_segment {
  void* param;
  const void* grad;
  void* state0;
  void* state1;
  void* ema;
  int64_t count;
  int32_t group;       /* index into yl_train_hyper.lr / weight_decay, < YL_TRAIN_MAX_GROUPS */
  uint32_t flags;      /* YL_TRAIN_SEG_* */
} yl_train_segment;
typedef struct yl_train_chunk {
  int32_t seg;         /* row of the segment table */
  int32_t len;         /* 1..chunk_elems elements  */
  int64_t off;         /* first element            */
} yl_train_chunk;
typedef struct yl_train_cfg {
  int32_t kind;             /* YL_TRAIN_ADAMW / ADAM / SGD                                               */
  int32_t amp;              /* 0: scale fixed at 1, no skipping                                          */
  int32_t growth_interval;  /* torch.amp.GradScaler's arguments                                          */
  int32_t chunk_elems;      /* 0 = YL_TRAIN_CHUNK_DEFAULT; a multiple of 4                               */
  float init_scale;
  double growth_factor, backoff_factor;
} yl_train_cfg;
typedef struct yl_train_hyper {     /* passed by value on every step: the scheduler and the EMA warm-up stay on the host */
  double lr[YL_TRAIN_MAX_GROUPS], weight_decay[YL_TRAIN_MAX_GROUPS];
  double beta1, beta2, eps;         /* AdamW, Adam   */
  double momentum;                  /* SGD           */
  double ema_decay;                 /* d of this step */
  double max_norm;                  /* <= 0: no clipping (the norm is computed all the same) */
  int32_t nesterov;
  int32_t reserved0;
} yl_train_hyper;
/* The chunk list of a table whose rows hold counts_host[s] elements: rows in table order, each cut into pieces of at
 * most chunk_elems (a multiple of 4); every element lies in exactly one chunk.  A pure host function.  Returns the
 * number of chunks (out_host may be NULL to count), or a negative yl_status (YL_ERR_CAPACITY: more than `capacity`). */
int64_t yl_train_plan(const int64_t* counts_host, int32_t nseg, int32_t chunk_elems, yl_train_chunk* out_host,
                      int64_t capacity);
/* Uploads the segment table and its chunk list, allocates the per-chunk partial buffers and the per-tensor step counts
 * (zero).  state_dev: YL_TRAIN_STATE_WORDS 4-byte words of device memory, 8-byte aligned, owned by the caller and alive
 * as long as the handle, so that a framework can view them as its own tensors: word 0 = scale (fp32), 1 = growth
 * tracker (int32), 2 = norm of the last step (fp32), 3 = found_inf of the last step (int32), 4-7 private.  The call
 * initialises them (scale = init_scale) and synchronises the device. */
yl_status yl_train_create(int32_t device, const yl_train_cfg* cfg, const yl_train_segment* segments_host, int32_t nseg,
                          void* state_dev, yl_train** out);
void yl_train_destroy(yl_train* t);
/* grad_ptrs_host[nseg]: this step's gradient of every row (NULL = the tensor takes no part in this step, as a None
 * .grad in torch; ignored for EMA-only and byte rows).  When any differs from what the device holds, the column is
 * copied from pinned memory on `stream` (asynchronous; the call waits only if the copy of four uploads ago has not run
 * yet).  No change: no work. */
yl_status yl_train_set_grads(yl_train* t, const void* const* grad_ptrs_host, void* stream);
/* Enqueues three kernels on `stream`: gradient statistics (every gradient read once), one-workgroup reduce (norm,
 * found_inf, scaler update, step counts), apply (optimizer, EMA, integer copies; reads norm / found_inf / scale from
 * device memory).  No synchronisation, no copy to the host, no allocation. */
yl_status yl_train_step(yl_train* t, const yl_train_hyper* hyper, void* stream);
/* device pointer to the current scale (word 0 of state_dev), for loss * scale without a host round trip */
float* yl_train_scale_ptr(yl_train* t);
/* Synchronises the device.  Scale, tracker, norm and found_inf of the last step and steps_host[nseg] (any may be
 * NULL): for logging, checkpoints and tests. */
yl_status yl_train_read_state(yl_train* t, float* scale, int32_t* growth_tracker, float* norm, int32_t* found_inf,
                              float* steps_host);
/* Synchronises the device.  Resume: scale (> 0; ignored without amp), tracker, steps_host[nseg] (NULL = keep). */
yl_status yl_train_write_state(yl_train* t, float scale, int32_t growth_tracker, const float* steps_host);

/* ---- trainable detection heads (reference scripts/model/model_v2.py:23-53 make_head, :182-192 _forward_head) -----
 * Forward and backward of ONE level's head on the device: head_depth blocks of depthwise 3x3 (pad 1, no bias) -> 1x1
 * (no bias) -> BatchNorm2d -> ReLU, then the box / obj / cls 1x1 convolutions written straight as the level tensor
 * [B, A, S, S, 5 + C] (anchor-major channels).  A yl_head handle needs no yl_ctx and holds no parameter: every call
 * reads the caller's tensors in PyTorch layout (fp32, contiguous, any 4-byte boundary), so an optimizer may update them
 * in place between two calls.  The input x is NHWC [B, S, S, F], 16-byte aligned; F a multiple of 4 (anything else,
 * and num_masks != 0: YL_ERR_UNSUPPORTED).  fp32 storage and arithmetic; the GEMMs run on v_mfma_f32_16x16x4_f32
 * (or, see "Mixed precision" below, on the 16-bit MFMA).
 * BatchNorm: YL_HEAD_TRAIN normalises with the batch statistics (biased variance, eps 1e-5), updates running_mean /
 * running_var in place (momentum 0.1, unbiased variance) and adds 1 to num_batches_tracked; without it the running
 * statistics are used and nothing is updated.  YL_HEAD_SAVE keeps d, z, h of every block and the statistics in the
 * handle for ONE later yl_head_backward of the same (batch, size); a forward without it drops what is held, runs
 * every block in one block's buffers and allocates no more than those (saved_bytes / head_depth).
 * Deterministic: every sum over rows is written as per-tile partials and summed in tile order in float64 by a second
 * kernel; no floating-point atomics; equal inputs give equal bits.
 *
 * Mixed precision.  YL_HEAD_F16 / YL_HEAD_BF16 in the forward's flags (exclusive: both set is YL_ERR_INVALID, checked
 * before anything is enqueued or a held forward is dropped) run every 1x1 GEMM of the head -- per block z = d . W1^T,
 * dd = dz . W1, dW1 = dz^T . d; for the outputs y = h . Wout^T, dh = gy . Wout, dWout = gy^T . h -- with BOTH operands
 * rounded to that type, round to nearest even, on v_mfma_f32_16x16x16_{f16,bf16}: products exact, accumulation in fp32.
 * The rounding happens in registers, on the four values a lane has loaded; a value outside the matrices stays the zero
 * it was filled with.  Nothing is clamped: a finite fp32 value beyond fp16's range becomes +-inf and the gradients it
 * reaches are not finite.  Everything else (depthwise 3x3 and its gradients, BatchNorm statistics, BN + ReLU and their
 * backward, the bias added to y, the float64 column sum of the unrounded gy, the partials and their ordered float64 sum,
 * the saved d / z / h, parameters, gradients) is fp32 as without the bits; the launch counts and yl_head_plan's figures
 * are the same, and equal inputs give equal bits.  The handle records the mode with the held forward: yl_head_backward
 * runs in the mode of the forward it belongs to. */
#define YL_HEAD_MAX_DEPTH 4
#define YL_HEAD_TRAIN 1u
#define YL_HEAD_SAVE 2u
#define YL_HEAD_F16 0x100u
#define YL_HEAD_BF16 0x200u
#define YL_HEAD_SITE_OUT (-1)       /* yl_head_gemm's site: the output convolutions; 0 .. head_depth - 1: that trunk block's 1x1 */
#define YL_HEAD_PASS_FORWARD 0      /* block t: a = d  [B][S][S][F] -> out = z  [B][S][S][F];  outputs: a = h -> out = y (level tensor) */
#define YL_HEAD_PASS_DGRAD 1        /* block t: a = dz [B][S][S][F] -> out = dd [B][S][S][F];  outputs: a = gy (level tensor) -> out = dh */
#define YL_HEAD_PASS_WGRAD 2        /* block t: a = d, b = dz -> out = dW1 [F][F];  outputs: a = h, b = gy -> out = [4A + A + A C][F] */
typedef struct yl_head yl_head;
typedef struct yl_head_cfg {
  int32_t channels;       /* F = fpn_channels */
  int32_t num_classes;    /* C >= 1 */
  int32_t num_anchors;    /* A of this level */
  int32_t head_depth;     /* 1..YL_HEAD_MAX_DEPTH */
  int32_t num_masks;      /* must be 0: mask-coefficient heads are not implemented */
  int32_t reserved0;
} yl_head_cfg;
typedef struct yl_head_block {      /* trunk.t.block.{0,1,2} */
  float* dw;                        /* [F][1][3][3] */
  float* pw;                        /* [F][F][1][1] */
  float* gamma;                     /* [F] BatchNorm weight */
  float* beta;                      /* [F] BatchNorm bias */
  float* running_mean;              /* [F] (ignored in a gradient table) */
  float* running_var;               /* [F] (ignored in a gradient table) */
  int64_t* num_batches_tracked;     /* one int64, 8-byte aligned (ignored in a gradient table) */
} yl_head_block;
typedef struct yl_head_tensors {    /* the parameters of a head, or where their gradients go (NULL = not wanted) */
  yl_head_block block[YL_HEAD_MAX_DEPTH];
  float *box_w, *box_b;             /* out.box [4A][F][1][1], [4A] */
  float *obj_w, *obj_b;             /* out.obj [A][F][1][1], [A]  */
  float *cls_w, *cls_b;             /* out.cls [A*C][F][1][1], [A*C] */
} yl_head_tensors;
typedef struct yl_head_plan_info {
  int32_t rows;                       /* M = batch * size * size */
  int32_t stat_rows, stat_tiles;      /* row reductions (BN statistics, dgamma / dbeta, depthwise weight gradient) */
  int32_t gemm_rows, gemm_tiles;      /* X.W^T and dY.W: rows per workgroup */
  int32_t wgrad_rows, wgrad_splits;   /* dY^T.X of a trunk 1x1: rows per split (a multiple of 16), splits */
  int32_t ograd_rows, ograd_splits;   /* dY^T.X of the output convolutions */
  int32_t reserved0;
  int64_t saved_bytes;                /* activations and statistics kept between a YL_HEAD_SAVE forward and backward */
  int64_t workspace_bytes;            /* two gradient tensors and the partial sums */
} yl_head_plan_info;
/* How a (cfg, batch, size) is cut and what it holds.  A pure host function: tile t of a cut covers the rows
 * [t * rows_per_tile, min(M, (t + 1) * rows_per_tile)), every row exactly once. */
yl_status yl_head_plan(const yl_head_cfg* cfg, int32_t batch, int32_t size, yl_head_plan_info* out);
yl_status yl_head_create(int32_t device, const yl_head_cfg* cfg, yl_head** out);
void yl_head_destroy(yl_head* h);
/* Enqueues the forward on `stream`: per block 4 launches (5 with YL_HEAD_TRAIN), 1 for the outputs.  The handle's
 * buffers grow (synchronising the device) when (batch, size) needs more than they hold.  launches (may be NULL): the
 * number of kernels enqueued.  YL_HEAD_TRAIN with batch * size * size == 1: YL_ERR_INVALID. */
yl_status yl_head_forward(yl_head* h, const yl_head_tensors* params, const float* x_dev, int32_t batch, int32_t size,
                          uint32_t flags, float* y_dev, void* stream, int32_t* launches);
/* Enqueues the backward of the forward the handle holds (YL_ERR_STATE if there is none of this batch and size).
 * gy_dev: the gradient of the level tensor, [B, A, S, S, 5 + C].  Every non-NULL tensor of `grads` is OVERWRITTEN with
 * that parameter's gradient; dx_dev (NHWC, 16-byte aligned, or NULL) with the input's.  What nobody asked for is not
 * computed: the trunk is walked back only to the first block something is wanted of, and `launches` says how far. */
yl_status yl_head_backward(yl_head* h, const yl_head_tensors* params, const yl_head_tensors* grads, const float* x_dev,
                           const float* gy_dev, float* dx_dev, int32_t batch, int32_t size, void* stream,
                           int32_t* launches);
/* What the handle holds now (a host function; any out pointer may be NULL): the bytes of its two device buffers and
 * whether a forward is held for yl_head_backward. */
yl_status yl_head_held(const yl_head* h, int64_t* saved_bytes, int64_t* workspace_bytes, int32_t* forward_held);
/* One 1x1 GEMM of the head on its own, launched exactly as the module launches it: `site` is a trunk block or
 * YL_HEAD_SITE_OUT, `pass` a YL_HEAD_PASS_*, `mode` 0 (fp32), YL_HEAD_F16 or YL_HEAD_BF16 (anything else:
 * YL_ERR_INVALID, checked first).  The weights (and, for the outputs' forward, the biases) are read from `params`, a
 * whole parameter table, through the accessors the module uses; b_dev is read by WGRAD only.  FORWARD and DGRAD: 1
 * launch; WGRAD: 2 launches (partials, cut as yl_head_plan cuts this batch and size, and their ordered float64 sum).  The
 * outputs' WGRAD writes the rows of box_w, obj_w and cls_w one after the other.  [B][S][S][F] operands and results of
 * FORWARD and DGRAD are 16-byte aligned (else YL_ERR_UNSUPPORTED); the level tensor and WGRAD's operands and result
 * need 4 bytes.  Uses the handle's workspace; if that has to grow, a held forward is dropped as any growth drops it. */
yl_status yl_head_gemm(yl_head* h, int32_t site, int32_t pass, uint32_t mode, const yl_head_tensors* params,
                       const float* a_dev, const float* b_dev, float* out_dev, int32_t batch, int32_t size, void* stream,
                       int32_t* launches);

/* ---- trainable depthwise FPN neck (reference scripts/model/model_v2.py:285-294, :337-361, YOLOLiteMS_CPU) -------------
 * Forward and backward of the whole top-down neck on the device.  Levels go finest first (p3, p4, p5; with use_p2: p2
 * first) and are square; level L - 1 is the coarsest.  The forward runs coarsest first:
 *     t_k = Wlat_k . c_k + blat_k   (+ up(p_{k+1}) for k < L - 1; up = nearest, torch's index rule)
 *     p_k = block_{d-1}( ... block_0(t_k))      block = the heads' block (yl_head_block)
 * and the backward finest first: G_k = gp_k (+ up^T(gt_{k-1}) for k > 0), the blocks back to gt_k = dL/dt_k, then
 * dWlat_k = gt_k^T . c_k, dblat_k = colsum gt_k, dc_k = gt_k . Wlat_k.
 * Parameters are read in PyTorch layout from the caller's tensors on every call, at any 4-byte boundary; c / p / gp / dc
 * are NHWC fp32, 16-byte aligned.  channels % 4 != 0 or in_channels[k] % 4 != 0: YL_ERR_UNSUPPORTED.  The P6 path is not
 * implemented; the dense-3x3 + SiLU smooth blocks of YOLOLiteMS are yl_dneck_* below.  YL_HEAD_TRAIN / YL_HEAD_SAVE mean what they
 * mean for the heads; with YL_HEAD_SAVE the handle keeps, per level, t_k and every block's d, z, h and statistics
 * (the last block's h is a copy of p_k: the caller's tensor may change before the backward), without it every level
 * runs in one level's buffers.  Deterministic in the way of the heads: per-tile partials summed in tile order in
 * float64, no floating-point atomics; the transposed upsample is a gather over the contiguous pre-image of each cell. */
#define YL_NECK_MAX_DEPTH 4
#define YL_NECK_MAX_LEVELS 4
typedef struct yl_neck yl_neck;
typedef struct yl_neck_cfg {
  int32_t channels;                           /* F = fpn_channels */
  int32_t depth;                              /* blocks per smooth, 1..YL_NECK_MAX_DEPTH */
  int32_t num_levels;                         /* L, 1..YL_NECK_MAX_LEVELS */
  int32_t in_channels[YL_NECK_MAX_LEVELS];    /* Cin of each level's feature map, finest first */
  int32_t reserved0;
} yl_neck_cfg;
typedef struct yl_neck_level {
  float* lat_w;                               /* lateral{k}.weight [F][Cin][1][1] */
  float* lat_b;                               /* lateral{k}.bias [F] */
  yl_head_block block[YL_NECK_MAX_DEPTH];     /* smooth{k}.block.{4i, 4i+1, 4i+2} */
} yl_neck_level;
typedef struct yl_neck_tensors {              /* the parameters, or where their gradients go (NULL = not wanted) */
  yl_neck_level level[YL_NECK_MAX_LEVELS];
} yl_neck_tensors;
typedef struct yl_neck_level_plan {
  int32_t rows;                               /* M_k = batch * S_k * S_k */
  int32_t stat_tiles, gemm_tiles;             /* tiles of stat_rows / gemm_rows rows */
  int32_t wgrad_rows, wgrad_splits;           /* dz^T . d of a block's 1x1 (F x F): rows per split, splits */
  int32_t lgrad_rows, lgrad_splits;           /* gt^T . c of the lateral (Cin x F) */
  int32_t reserved0;
  int64_t saved_bytes;                        /* (1 + 3 depth) M_k F 4 + depth 2 F 4: t_k; d, z, h and statistics per block */
} yl_neck_level_plan;
typedef struct yl_neck_plan_info {
  int32_t stat_rows, gemm_rows;
  yl_neck_level_plan level[YL_NECK_MAX_LEVELS];
  int64_t saved_bytes;                        /* sum of the levels' saved_bytes (YL_HEAD_SAVE) */
  int64_t nosave_bytes;                       /* without YL_HEAD_SAVE: 4 Mmax F 4 + 2 F 4, t and ONE block of the largest level */
  int64_t workspace_bytes;                    /* 3 Mmax F 4 (two gradients in flight and gt) + the float64 partials of the
                                                 largest level, rounded up to 16 + 2 F 4 + the largest split partials */
  int64_t table_bytes;                        /* the nearest maps: per k < L - 1, (S_k + 2 S_{k+1}) int32 */
} yl_neck_plan_info;
/* A pure host function: tile t of a cut covers the rows [t * rows_per_tile, min(M, (t + 1) * rows_per_tile)). */
yl_status yl_neck_plan(const yl_neck_cfg* cfg, int32_t batch, const int32_t* sizes, yl_neck_plan_info* out);
/* torch's nearest rule for an axis of `in` cells read at `out`: src[o] = min((int)floorf(o * ((float)in / out)), in - 1),
 * and the pre-image of source cell i is the destination range [lo[i], hi[i]) (the map is monotone).  Host only. */
yl_status yl_neck_nearest_map(int32_t out, int32_t in, int32_t* src, int32_t* lo, int32_t* hi);
yl_status yl_neck_create(int32_t device, const yl_neck_cfg* cfg, yl_neck** out);
void yl_neck_destroy(yl_neck* h);
/* Enqueues the forward: per level 1 launch for the lateral (bias and upsample-add in its epilogue) and per block 4
 * launches (5 with YL_HEAD_TRAIN); with YL_HEAD_SAVE one device-to-device copy per level besides (not counted).
 * c_dev[k]: [B, S_k, S_k, Cin_k]; p_dev[k]: [B, S_k, S_k, F], written.  YL_HEAD_TRAIN with batch * S_k * S_k == 1 on any
 * level: YL_ERR_INVALID before any launch.  The nearest maps are computed on the host and uploaded when `sizes` change
 * (synchronising the device), as are the buffers when they must grow. */
yl_status yl_neck_forward(yl_neck* h, const yl_neck_tensors* params, const float* const* c_dev, int32_t batch,
                          const int32_t* sizes, uint32_t flags, float* const* p_dev, void* stream, int32_t* launches);
/* Enqueues the backward of the held forward (YL_ERR_STATE if there is none of this batch and these sizes).  gp_dev[k]:
 * the gradient of p_k.  Every non-NULL tensor of `grads` and every non-NULL dc_dev[k] is OVERWRITTEN.  What nobody
 * asked for is not run.  Level k is walked only if something of a level >= k is wanted (a parameter or dc), finest
 * first up to the coarsest such level K:
 *   1 launch for G_k when k > 0 (the gather of gt_{k-1} plus gp_k);
 *   the blocks, last first, as in yl_head_backward: per block [1 sums if train or gamma / beta wanted] + 1 (bn grads)
 *     + 1 (dz) + [2 if pw wanted] + 1 (dd) + [2 if dw wanted] + [1 input gradient], stopping at the last thing wanted;
 *     gt_k is wanted when something of the lateral k, dc_k or a level > k is;
 *   2 launches for dWlat_k, 2 for dblat_k, 1 for dc_k, each only where wanted. */
yl_status yl_neck_backward(yl_neck* h, const yl_neck_tensors* params, const yl_neck_tensors* grads,
                           const float* const* c_dev, const float* const* gp_dev, float* const* dc_dev, int32_t batch,
                           const int32_t* sizes, void* stream, int32_t* launches);
yl_status yl_neck_held(const yl_neck* h, int64_t* saved_bytes, int64_t* workspace_bytes, int32_t* forward_held);

/* ---- trainable dense FPN neck (reference scripts/model/model_v2.py:15-22 conv_block, :115-127, :194-203, YOLOLiteMS) ----
 * The neck above with the smooth blocks of arch YOLOLiteMS: block = dense 3x3 convolution (pad 1, stride 1, no bias,
 * weight [F][F][3][3]) -> BatchNorm2d -> SiLU.  Laterals, top-down chain, nearest maps (yl_neck_nearest_map), the
 * configuration (yl_neck_cfg, the same refusals), flags, layouts, alignment rules, BatchNorm numerics and the
 * determinism argument are those of yl_neck_*; the P6 path is not implemented.
 * The convolution is an implicit GEMM on v_mfma_f32_16x16x4_f32: a workgroup owns an 8 x 8 spatial tile of ONE image
 * times 64 output channels, stages the tile's 10 x 10 input window (zero outside the image) in LDS once per block of 16
 * input channels, and all nine taps read it there as shifted windows.  The weights are read from the caller's tensor on
 * every call and copied by a pack kernel into the handle's workspace as [tap][out][in] (forward) or, for the input
 * gradient, [8 - tap][in][out]: the input gradient is the same convolution kernel on dz.  The weight gradient cuts the
 * level's spatial tiles into w3grad_splits runs of w3grad_tiles tiles; a workgroup (64 in x 64 out channels, one run)
 * stages each tile's x window and dz tile once for all nine taps and writes fp32 partials [split][tap][out][in]; a
 * second kernel sums them in split order in float64 into [F][F][3][3].
 * With YL_HEAD_SAVE the handle keeps, per level, t_k and per block z, h and (mean, invstd): the block's input is t_k
 * or the previous h.
 *
 * Mixed precision.  YL_DNECK_F16 / YL_DNECK_BF16 in the forward's flags (exclusive: both set is YL_ERR_INVALID, checked
 * before the device is touched) run the three 3x3 GEMMs -- forward (x, W), input gradient (dz, W), weight gradient
 * (x, dz) -- with BOTH operands rounded to that type, round to nearest even, on v_mfma_f32_16x16x16_{f16,bf16}: products
 * exact, accumulation in fp32.  The pack kernel writes the 16-bit weight, the convolution converts the window and the
 * weight gradient the x window and the dz tile where they are written to LDS.  Nothing is clamped: a finite fp32 value
 * beyond fp16's range becomes +-inf and the gradients it reaches are not finite.  Everything else (laterals, the chain,
 * BatchNorm statistics, SiLU, the saved z / h / t, the partials and their ordered float64 sum, parameters, gradients)
 * is fp32 as without the bits, the launch counts and yl_dneck_plan's figures are the same, and equal inputs give equal
 * bits.  The backward runs in the mode of the forward it belongs to. */
#define YL_DNECK_F16 0x100u
#define YL_DNECK_BF16 0x200u
#define YL_DNECK_PASS_FORWARD 0     /* a = x  [B][S][S][F], b = W  [F][F][3][3] -> out = z  [B][S][S][F] */
#define YL_DNECK_PASS_DGRAD 1       /* a = dz [B][S][S][F], b = W  [F][F][3][3] -> out = dx [B][S][S][F] */
#define YL_DNECK_PASS_WGRAD 2       /* a = x  [B][S][S][F], b = dz [B][S][S][F] -> out = dW [F][F][3][3] */
typedef struct yl_dneck yl_dneck;
typedef struct yl_dneck_block {     /* smooth{k}.{3i} (w), smooth{k}.{3i+1} (BatchNorm) */
  float* w;                         /* [F][F][3][3] */
  float* gamma;                     /* [F] BatchNorm weight */
  float* beta;                      /* [F] BatchNorm bias */
  float* running_mean;              /* [F] (ignored in a gradient table) */
  float* running_var;               /* [F] (ignored in a gradient table) */
  int64_t* num_batches_tracked;     /* one int64, 8-byte aligned (ignored in a gradient table) */
} yl_dneck_block;
typedef struct yl_dneck_level {
  float* lat_w;                               /* lateral{k}.weight [F][Cin][1][1] */
  float* lat_b;                               /* lateral{k}.bias [F] */
  yl_dneck_block block[YL_NECK_MAX_DEPTH];
} yl_dneck_level;
typedef struct yl_dneck_tensors {             /* the parameters, or where their gradients go (NULL = not wanted) */
  yl_dneck_level level[YL_NECK_MAX_LEVELS];
} yl_dneck_tensors;
typedef struct yl_dneck_level_plan {
  int32_t rows;                               /* M_k = batch * S_k * S_k */
  int32_t stat_tiles, gemm_tiles;             /* tiles of stat_rows / gemm_rows rows */
  int32_t conv_tiles;                         /* batch * ceil(S_k / conv_tile)^2 spatial tiles, image-major then row-major */
  int32_t lgrad_rows, lgrad_splits;           /* gt^T . c of the lateral (Cin x F): rows per split, splits */
  int32_t w3grad_tiles, w3grad_splits;        /* the 3x3 weight gradient: spatial tiles per split, splits;
                                                 splits = ceil(conv_tiles / w3grad_tiles), w3grad_tiles =
                                                 ceil(conv_tiles / min(conv_tiles, 64, max(1, 512 / ceil(F / 64)^2))) */
  int64_t saved_bytes;                        /* (1 + 2 depth) M_k F 4 + depth 2 F 4: t_k; z, h and statistics per block */
} yl_dneck_level_plan;
typedef struct yl_dneck_plan_info {
  int32_t stat_rows, gemm_rows;
  int32_t conv_tile;                          /* edge of a spatial tile (8) */
  int32_t reserved0;
  yl_dneck_level_plan level[YL_NECK_MAX_LEVELS];
  int64_t saved_bytes;                        /* sum of the levels' saved_bytes (YL_HEAD_SAVE) */
  int64_t nosave_bytes;                       /* without YL_HEAD_SAVE: 3 Mmax F 4 + 2 F 4, t and ONE block of the largest level */
  int64_t workspace_bytes;                    /* 3 Mmax F 4 (two gradients in flight and gt)
                                                 + round16(max_k(stat_tiles_k) 2 F 8)  the float64 column partials
                                                 + 2 F 4                               the BatchNorm backward's coefficients
                                                 + 9 F F 4                             one packed 3x3 weight
                                                 + max_k round16(max(w3grad_splits_k 9 F F, lgrad_splits_k F Cin_k) 4) */
  int64_t table_bytes;                        /* the nearest maps: per k < L - 1, (S_k + 2 S_{k+1}) int32 */
} yl_dneck_plan_info;
/* A pure host function.  Row tile t covers the rows [t * rows_per_tile, min(M, (t + 1) * rows_per_tile)); split z of
 * the 3x3 weight gradient covers the spatial tiles [z * w3grad_tiles, min(conv_tiles, (z + 1) * w3grad_tiles)). */
yl_status yl_dneck_plan(const yl_neck_cfg* cfg, int32_t batch, const int32_t* sizes, yl_dneck_plan_info* out);
yl_status yl_dneck_create(int32_t device, const yl_neck_cfg* cfg, yl_dneck** out);
void yl_dneck_destroy(yl_dneck* h);
/* Enqueues the forward: per level 1 launch for the lateral (bias and upsample-add in its epilogue) and per block 4
 * launches (weight pack, convolution, BatchNorm statistics, BatchNorm + SiLU; 5 with YL_HEAD_TRAIN: the column sums);
 * with YL_HEAD_SAVE one device-to-device copy per level besides (not counted).  Arguments, refusals and the growth of
 * the buffers as in yl_neck_forward. */
yl_status yl_dneck_forward(yl_dneck* h, const yl_dneck_tensors* params, const float* const* c_dev, int32_t batch,
                           const int32_t* sizes, uint32_t flags, float* const* p_dev, void* stream, int32_t* launches);
/* Enqueues the backward of the held forward (YL_ERR_STATE if there is none of this batch and these sizes).  Every
 * non-NULL tensor of `grads` and every non-NULL dc_dev[k] is OVERWRITTEN.  What nobody asked for is not run.  Level k
 * is walked only if something of a level >= k is wanted (a parameter or dc), finest first up to the coarsest such
 * level K:
 *   1 launch for G_k when k > 0 (the gather of gt_{k-1} plus gp_k);
 *   the blocks, last first, back to the first thing wanted: per block [1 sums if train or gamma / beta wanted]
 *     + 1 (bn grads) + 1 (dz) + [2 if w wanted: partials, ordered sum] + [2 input gradient: weight pack, convolution];
 *     the input gradient of block 0 runs only if gt_k is needed, which it is when something of the lateral k, dc_k or
 *     a level > k is wanted;
 *   2 launches for dWlat_k, 2 for dblat_k, 1 for dc_k, each only where wanted. */
yl_status yl_dneck_backward(yl_dneck* h, const yl_dneck_tensors* params, const yl_dneck_tensors* grads,
                            const float* const* c_dev, const float* const* gp_dev, float* const* dc_dev, int32_t batch,
                            const int32_t* sizes, void* stream, int32_t* launches);
yl_status yl_dneck_held(const yl_dneck* h, int64_t* saved_bytes, int64_t* workspace_bytes, int32_t* forward_held);
/* One 3x3 GEMM of the neck on its own, launched exactly as the module launches it: `pass` is a YL_DNECK_PASS_*, `mode`
 * is 0 (fp32), YL_DNECK_F16 or YL_DNECK_BF16 (anything else: YL_ERR_INVALID); F is the handle's cfg.channels, `size` the
 * level's S.  FORWARD and DGRAD: 2 launches (weight pack, convolution); WGRAD: 2 launches (partials, cut as
 * yl_dneck_plan cuts a level of this batch and size, and their ordered float64 sum).  The three pointers are 16-byte
 * aligned (else YL_ERR_UNSUPPORTED).  Uses the handle's workspace (9 F F 4 + w3grad_splits 9 F F 4 bytes at most); if
 * that has to grow, a held forward is dropped as any growth drops it. */
yl_status yl_dneck_conv3x3(yl_dneck* h, int32_t pass, uint32_t mode, const float* a_dev, const float* b_dev,
                           float* out_dev, int32_t batch, int32_t size, void* stream, int32_t* launches);

/* ---- trainable backbone stage: a stack of MobileNetV4 UIB blocks (timm UniversalInvertedResidual) and 1x1 ConvBnAct ----
 * Forward and backward of up to YL_STAGE_MAX_BLOCKS blocks over square NHWC fp32 maps [B][S][S][C], fp32 throughout.
 * A block is a run of UNITS, each a bias-free convolution followed by BatchNorm2d:
 *     uir:  [dw_start: depthwise a x a, stride (k ? 1 : s), BN]   pw_exp: 1x1 cin -> mid, BN, ReLU
 *           [dw_mid:   depthwise k x k, stride s, BN, ReLU]        pw_proj: 1x1 mid -> cout, BN
 *           a, k in {0, 3, 5} (0: the unit is absent), s in {1, 2}; the block adds its input when cin == cout and s == 1
 *     cn:   1x1 cin -> cout, BN, ReLU   (held in the pw_exp entry of the tables; mid is ignored)
 * A depthwise k x k pads (k - 1) / 2 on every side: S_out = (S + 2 p - k) / s + 1, odd S under stride 2 included.  Every
 * channel count is a multiple of 4, block i's cin is block i - 1's cout, s == 2 needs a depthwise unit to carry it and
 * eps > 0: anything else is YL_ERR_INVALID from a host-side check before any device call.
 * A handle's VARIANT (yl_variant_stage_set, below) replaces ReLU by ReLU6 and the symmetric padding by TF-SAME's; a uir
 * block with a = 0 is then timm's InvertedResidual without squeeze-excite (conv_pw, conv_dw, conv_pwl), which is what
 * the EfficientNet-Lite stages are made of.  Squeeze-excite, SiLU and layer-scale do not exist here.
 * Parameters are read in PyTorch layout from the caller's tensors on every call, at any 4-byte boundary (depthwise
 * [C][1][k][k], 1x1 [out][in][1][1]); x / out / gy / dx are 16-byte aligned (else YL_ERR_UNSUPPORTED).
 * The depthwise passes: forward, one thread per output pixel x 4 channels, taps in (ky, kx) order, fp32 sum from zero;
 * input gradient as a gather, one thread per INPUT pixel x 4 channels summing, in (ky, kx) order, the taps whose
 * (i + p - ky) is a multiple of the stride; weight gradient as float64 partials per tile of stat_rows OUTPUT rows and
 * their sum in tile order (under TF-SAME p is the leading pad, see yl_variant_stage_set; tap order and sums are the same).
 * The 1x1 convolutions are the heads' GEMM (v_mfma_f32_16x16x4_f32) in all three passes.
 * BatchNorm numerics are the heads' with eps from the configuration: statistics in float64 partials per tile of
 * stat_rows rows summed in tile order, biased variance to normalise, unbiased for running_var, momentum 0.1,
 * num_batches_tracked += 1; without YL_HEAD_TRAIN the running statistics are used and nothing is updated.
 * Equal inputs give equal bits: no floating-point atomics. */
#define YL_STAGE_MAX_BLOCKS 16
#define YL_STAGE_UIR 0
#define YL_STAGE_CN 1
#define YL_STAGE_PASS_FORWARD 0     /* a = x  [B][S][S][C],    b = W  [C][1][k][k]   -> out = y  [B][So][So][C] */
#define YL_STAGE_PASS_DGRAD 1       /* a = dy [B][So][So][C],  b = W  [C][1][k][k]   -> out = dx [B][S][S][C]  */
#define YL_STAGE_PASS_WGRAD 2       /* a = x  [B][S][S][C],    b = dy [B][So][So][C] -> out = dW [C][1][k][k]  */
typedef struct yl_stage yl_stage;
typedef struct yl_stage_block_cfg {
  int32_t type;                     /* YL_STAGE_UIR / YL_STAGE_CN */
  int32_t a, k, s;                  /* uir: dw_start kernel, dw_mid kernel, stride; cn: 0, 1, 1 */
  int32_t mid;                      /* uir: the expanded width */
  int32_t cout;
  int32_t reserved0, reserved1;
} yl_stage_block_cfg;
typedef struct yl_stage_cfg {
  int32_t in_channels;              /* cin of block 0 */
  int32_t num_blocks;               /* 1..YL_STAGE_MAX_BLOCKS */
  double eps;                       /* of every BatchNorm */
  yl_stage_block_cfg block[YL_STAGE_MAX_BLOCKS];
} yl_stage_cfg;
typedef struct yl_stage_unit {      /* one convolution and its BatchNorm; an absent unit's entries are ignored */
  float* w;                         /* conv.weight */
  float* gamma;                     /* bn.weight */
  float* beta;                      /* bn.bias */
  float* running_mean;              /* (ignored in a gradient table) */
  float* running_var;               /* (ignored in a gradient table) */
  int64_t* num_batches_tracked;     /* one int64, 8-byte aligned (ignored in a gradient table) */
} yl_stage_unit;
typedef struct yl_stage_block {     /* cn: pw_exp holds conv / bn1 */
  yl_stage_unit dw_start, pw_exp, dw_mid, pw_proj;
} yl_stage_block;
typedef struct yl_stage_tensors {   /* the parameters, or where their gradients go (NULL = not wanted) */
  yl_stage_block block[YL_STAGE_MAX_BLOCKS];
} yl_stage_tensors;
typedef struct yl_stage_block_plan {
  int32_t size_in, size_mid, size_out;        /* S entering the block, behind dw_start (where pw_exp runs), leaving it */
  int32_t rows_mid, rows_out;                 /* batch * size_mid^2 (dw_start, pw_exp; cn), batch * size_out^2 (dw_mid, pw_proj) */
  int32_t stat_tiles_mid, stat_tiles_out;     /* tiles of stat_rows rows */
  int32_t exp_rows, exp_splits;               /* weight gradient of pw_exp / cn (cin x mid over rows_mid): rows per split, splits */
  int32_t proj_rows, proj_splits;             /* of pw_proj (mid x cout over rows_out); 0 for cn */
  int32_t units;                              /* 1..4 */
  int64_t saved_bytes;                        /* sum over the block's units of 2 M_u C_u 4 + 2 C_u 4: z, h and (mean, invstd);
                                                 M_u, C_u: rows and channels of the unit's OUTPUT */
} yl_stage_block_plan;
typedef struct yl_stage_plan_info {
  int32_t stat_rows, gemm_rows;
  yl_stage_block_plan block[YL_STAGE_MAX_BLOCKS];
  int64_t saved_bytes;              /* YL_HEAD_SAVE: M_0 C_0 4 (a copy of x) + the blocks' saved_bytes */
  int64_t nosave_bytes;             /* without: 4 Amax + 2 Cmax 4; Amax = max_u M_u C_u 4 (one z, three rotating h), Cmax = max_u C_u */
  int64_t workspace_bytes;          /* 3 max(Amax, M_0 C_0 4)                        three rotating gradients
                                       + max_u round16(tiles_u T_u C_u 8)           float64 partials; T_u = k^2 for a depthwise unit, 2 for a 1x1
                                       + 2 Cmax 4                                    the BatchNorm backward's coefficients
                                       + max over 1x1 units of round16(splits_u cin_u cout_u 4) */
} yl_stage_plan_info;
/* A pure host function: tile t of a cut covers the rows [t * rows_per_tile, min(M, (t + 1) * rows_per_tile)); the
 * splits are those the heads' weight gradient makes of an NP x NQ GEMM over M rows. */
yl_status yl_stage_plan(const yl_stage_cfg* cfg, int32_t batch, int32_t size, yl_stage_plan_info* out);
yl_status yl_stage_create(int32_t device, const yl_stage_cfg* cfg, yl_stage** out);
void yl_stage_destroy(yl_stage* h);
yl_status yl_stage_held(const yl_stage* h, int64_t* saved_bytes, int64_t* workspace_bytes, int32_t* forward_held);
/* Enqueues the forward: per unit 3 launches (convolution, BatchNorm statistics, BatchNorm [+ ReLU] [+ the block's
 * input]), 4 with YL_HEAD_TRAIN (the column sums); with YL_HEAD_SAVE two device-to-device copies besides (x in, the
 * last h out; not counted).  x_dev: [B][size][size][in_channels]; out_dev: [B][S_out][S_out][cout of the last block],
 * written.  `flags`: YL_HEAD_TRAIN, YL_HEAD_SAVE; any other bit (the precision bits among them) is YL_ERR_INVALID.
 * YL_HEAD_TRAIN with a unit of ONE output row: YL_ERR_INVALID before any launch.  One forward is held per handle. */
yl_status yl_stage_forward(yl_stage* h, const yl_stage_tensors* params, const float* x_dev, int32_t batch, int32_t size,
                           uint32_t flags, float* out_dev, void* stream, int32_t* launches);
/* Enqueues the backward of the held forward (YL_ERR_STATE if there is none).  gy_dev: the gradient of out.  Every
 * non-NULL tensor of `grads` and dx_dev (may be NULL) is OVERWRITTEN.  The units are walked last first down to the
 * first one something is wanted of (unit 0 with dx_dev); nothing upstream of it runs.  Per unit: [1 sums if train or
 * gamma / beta wanted] + 1 (bn grads) + 1 (dz) + [2 if w wanted: partials, ordered sum] + [1 input gradient, if the
 * walk goes on]; + 1 per residual block whose input gradient is computed (the add of the block output's gradient). */
yl_status yl_stage_backward(yl_stage* h, const yl_stage_tensors* params, const yl_stage_tensors* grads,
                            const float* gy_dev, float* dx_dev, void* stream, int32_t* launches);
/* ONE depthwise pass on its own, launched exactly as the module launches it, on the current device: `pass` is a
 * YL_STAGE_PASS_*, k in {3, 5}, stride in {1, 2}, `size` the FORWARD's input size S (So follows).  FORWARD and DGRAD: 1
 * launch; WGRAD: 2 (partials, ordered sum), with a temporary buffer for the partials that is freed before the call
 * returns, which waits for `stream`.  a_dev and out_dev of FORWARD / DGRAD and both operands of WGRAD are 16-byte
 * aligned (else YL_ERR_UNSUPPORTED); a weight may start at any 4-byte boundary. */
yl_status yl_stage_depthwise(const float* a_dev, const float* b_dev, float* out_dev, int32_t pass, int32_t k,
                             int32_t stride, int32_t batch, int32_t size, int32_t channels, void* stream,
                             int32_t* launches);
/* ---- The variant of a stage: what the EfficientNet-Lite family (tf_efficientnet_lite0..4) needs of it.
 * `act` is YL_STAGE_ACT_RELU (a new handle's) or YL_STAGE_ACT_RELU6: what every activated unit (pw_exp, dw_mid, cn) runs
 * behind its BatchNorm.  ReLU6 is h = min(max(y, 0), 6); its backward passes dh where 0 < h < 6, both strict (torch's
 * hardtanh_backward), read off the saved output as ReLU's mask is.
 * `same` is 0 (a new handle's: (k - 1) / 2 zeros on every side) or 1: TensorFlow's SAME padding of every depthwise unit.  For
 * odd k its output size is ceil(S / s), which is S_out above, so yl_stage_plan, the arenas and every tile count hold for both.
 * What differs is the pad in front of the first row and column: total = max((S_out - 1) s + k - S, 0), of which the leading
 * side gets total / 2 rounded down: (k - 1) / 2 - 1 when s == 2 and S is even, (k - 1) / 2 otherwise, so only strided
 * depthwise units over an even S change.  Forward: tap ky of output row i reads input row i s + ky - p; input gradient: input
 * row i gathers the taps whose (i + p - ky) is a multiple of s; the weight gradient reads the forward's rows.  Tap order,
 * fp32 sums from zero and float64 partials are those of the symmetric form, which runs the same kernels with p = (k - 1) / 2
 * and gives the bits it gave before the variant existed.
 * Any other value of either argument is YL_ERR_INVALID from a host-side check and changes nothing; with a forward held for
 * backward the setter is YL_ERR_STATE (the backward runs in the variant of its forward, and a forward stays held until
 * the next one): set the variant before the first forward, or behind a forward without YL_HEAD_SAVE.  _get: either
 * pointer may be NULL. */
#define YL_STAGE_ACT_RELU 0
#define YL_STAGE_ACT_RELU6 1
yl_status yl_variant_stage_set(yl_stage* h, int32_t act, int32_t same);
yl_status yl_variant_stage_get(const yl_stage* h, int32_t* act, int32_t* same);
/* yl_stage_depthwise (which is same = 0) with the padding chosen: same arguments, launches and alignment rules. */
yl_status yl_variant_stage_depthwise(const float* a_dev, const float* b_dev, float* out_dev, int32_t pass, int32_t k,
                                     int32_t stride, int32_t batch, int32_t size, int32_t channels, int32_t same,
                                     void* stream, int32_t* launches);

/* ---- trainable dense stem: a stack of dense convolutions, each followed by BatchNorm2d and ReLU --------------------------
 * Forward and backward of up to YL_STEM_MAX_UNITS units, fp32 throughout.  A unit is a bias-free dense k x k convolution,
 * k in {1, 3}, stride s in {1, 2}, padding (k - 1) / 2 on every side (S_out = (S + 2 p - k) / s + 1, odd S included), its
 * BatchNorm2d and a ReLU.  Activations are square NHWC maps [B][S][S][C] with C a multiple of 4; with input_nchw = 1 the
 * stack's input alone is planar [B][cin][S][S], cin in 1..4 (the image): forward and weight gradient read it, its own
 * gradient does not exist (dx_dev with input_nchw: YL_ERR_INVALID).  Every cout is a multiple of 4.  Residuals, other
 * activations and TF-SAME padding do not exist here.  Anything else is YL_ERR_INVALID from a host-side check before any
 * device call.  Parameters are read in PyTorch layout ([cout][cin][k][k]) from the caller's tensors on every call, at any
 * 4-byte boundary; x (NHWC) / out / gy / dx are 16-byte aligned (else YL_ERR_UNSUPPORTED), a planar x 4-byte aligned.
 * The 3x3 passes are implicit GEMMs on v_mfma_f32_16x16x4_f32 over spatial tiles of conv_tile x conv_tile pixels; the
 * GEMM's k index runs (tap, c) with c fastest and every tap's c padded to a multiple of 4; a weight pack kernel writes
 * that order once per call.  Input gradient under stride 2: four parity classes of input pixels, each a GEMM of its own
 * over 1, 2, 2, 4 taps (no zero insertion, no atomics).  Weight gradient: fp32 partials part[split][tap][n][c] over whole
 * spatial tiles, summed in split order in float64.  The 1x1 units are the heads' GEMM in all three passes (stride 2:
 * the rows read / write every second pixel; its input gradient zeroes dx first).  BatchNorm numerics are the stage's
 * (yl_stage_*), with one difference: a unit's statistics tiles hold stat_rows_u = stat_rows * ceil(ceil(M_u / stat_rows)
 * / stat_tiles_max) rows, so that no unit has more than stat_tiles_max tiles; partials are float64, summed in tile order.
 * Equal inputs give equal bits: no floating-point atomics. */
#define YL_STEM_MAX_UNITS 8
typedef struct yl_stem yl_stem;
typedef struct yl_stem_unit_cfg {
  int32_t k, s, cout, reserved0;
} yl_stem_unit_cfg;
typedef struct yl_stem_cfg {
  int32_t in_channels;              /* cin of unit 0 */
  int32_t num_units;                /* 1..YL_STEM_MAX_UNITS */
  int32_t input_nchw;               /* 1: x is planar [B][cin][S][S], cin in 1..4 */
  int32_t reserved0;
  double eps;                       /* of every BatchNorm */
  yl_stem_unit_cfg unit[YL_STEM_MAX_UNITS];
} yl_stem_cfg;
typedef struct yl_stem_tensors {    /* the parameters, or where their gradients go (NULL = not wanted) */
  yl_stage_unit unit[YL_STEM_MAX_UNITS];
} yl_stem_tensors;
typedef struct yl_stem_unit_plan {
  int32_t size_in, size_out;        /* S entering and leaving the unit */
  int32_t rows_out;                 /* M_u = batch * size_out^2 */
  int32_t stat_rows, stat_tiles;    /* stat_rows_u (above); ceil(M_u / stat_rows_u) <= stat_tiles_max */
  int32_t wgrad_rows, wgrad_splits; /* 1x1: rows per split and splits as the heads cut a cin x cout weight gradient over M_u
                                       rows.  3x3: spatial tiles per split and splits: with tiles = batch * ceil(size_out /
                                       conv_tile)^2, blocks = ceil(round4(cin) / 32) * ceil(cout / 64) and want =
                                       clamp(1024 / blocks, 1, tiles): wgrad_rows = ceil(tiles / want), splits = ceil(tiles / wgrad_rows) */
  int32_t conv_block;               /* 3x3: output channels per workgroup, 16 PT with the PT of {4, 3, 2} that minimises
                                       ceil(cout / (16 PT)) PT (ties: the larger PT); 1x1: 0 */
  int64_t saved_bytes;              /* 2 M_u C_u 4 + 2 C_u 4: z, h and (mean, invstd); C_u = cout */
} yl_stem_unit_plan;
typedef struct yl_stem_plan_info {
  int32_t stat_rows, gemm_rows, conv_tile, stat_tiles_max;
  yl_stem_unit_plan unit[YL_STEM_MAX_UNITS];
  int64_t saved_bytes;              /* YL_HEAD_SAVE: round16(M_0 C_0 4) (a copy of x) + the units' saved_bytes.  The edge_n
                                       stem at batch 64, 640 px keeps 2.67 GB: 2.36 GB of z and h, 0.84 GB each for unit 0's,
                                       and the 0.31 GB copy of x */
  int64_t nosave_bytes;             /* without: 3 Amax + 2 Cmax 4; Amax = max_u M_u C_u 4 (one z, two alternating h), Cmax = max_u C_u */
  int64_t workspace_bytes;          /* 2 Amax                                         two alternating gradients
                                       + max_u round16(stat_tiles_u 2 C_u 8)         float64 partials
                                       + 2 Cmax 4                                    the BatchNorm backward's coefficients
                                       + max over 3x3 units of round16(9 cout round4(cin) 4)      the packed weight
                                       + max_u round16(splits_u W_u 4), W_u = cin cout (1x1), 9 cout round4(cin) (3x3) */
} yl_stem_plan_info;
/* A pure host function.  YL_ERR_UNSUPPORTED: a shape beyond the kernels' index arithmetic (a 1x1 unit of more than
 * 65535 * gemm_rows rows among them). */
yl_status yl_stem_plan(const yl_stem_cfg* cfg, int32_t batch, int32_t size, yl_stem_plan_info* out);
yl_status yl_stem_create(int32_t device, const yl_stem_cfg* cfg, yl_stem** out);
void yl_stem_destroy(yl_stem* h);
yl_status yl_stem_held(const yl_stem* h, int64_t* saved_bytes, int64_t* workspace_bytes, int32_t* forward_held);
/* Enqueues the forward.  Launches per unit: convolution (3x3: 2, pack and convolution; 1x1: 1) + [1 column sums with
 * YL_HEAD_TRAIN] + 2 (BatchNorm statistics, BatchNorm + ReLU); with YL_HEAD_SAVE two device-to-device copies besides (x
 * in, the last h out; not counted).  x_dev: [B][size][size][in_channels], or planar with input_nchw; out_dev:
 * [B][S_out][S_out][cout of the last unit], written.  `flags`: YL_HEAD_TRAIN, YL_HEAD_SAVE; any other bit (the precision
 * bits among them) is YL_ERR_INVALID.  YL_HEAD_TRAIN with a unit of ONE output row: YL_ERR_INVALID before any launch.
 * One forward is held per handle. */
yl_status yl_stem_forward(yl_stem* h, const yl_stem_tensors* params, const float* x_dev, int32_t batch, int32_t size,
                          uint32_t flags, float* out_dev, void* stream, int32_t* launches);
/* Enqueues the backward of the held forward (YL_ERR_STATE if there is none).  Every non-NULL tensor of `grads` and
 * dx_dev (may be NULL; must be NULL with input_nchw) is OVERWRITTEN.  The units are walked last first down to the first
 * one something is wanted of (unit 0 with dx_dev); nothing upstream of it runs.  Per unit: [1 sums if train or gamma /
 * beta wanted] + 1 (bn grads) + 1 (dz) + [2 if w wanted: partials, ordered sum] + [the input gradient, if the walk goes
 * on: 1x1: 1 (stride 2: and a memset, not counted); 3x3 stride 1: 2 (pack, convolution); 3x3 stride 2: 1 + C (pack, one
 * convolution per parity class that has pixels: C = 4 if size_in >= 2, else 1)]. */
yl_status yl_stem_backward(yl_stem* h, const yl_stem_tensors* params, const yl_stem_tensors* grads, const float* gy_dev,
                           float* dx_dev, void* stream, int32_t* launches);
/* ONE convolution pass on its own, launched exactly as the module launches it, on the current device: `pass` is a
 * YL_STAGE_PASS_* (FORWARD: a = x, b = W -> y; DGRAD: a = dy, b = W -> dx; WGRAD: a = x, b = dy -> dW), W is
 * [cout][cin][k][k], `size` the FORWARD's input size S.  input_nchw: x is planar, cin in 1..4; DGRAD is then
 * YL_ERR_INVALID.  Launch counts as in yl_stem_forward / yl_stem_backward.  Packed weight and partials live in a temporary
 * buffer that is freed before the call returns, which waits for `stream`.  A weight and a planar x may start at any
 * 4-byte boundary, every other tensor is 16-byte aligned (else YL_ERR_UNSUPPORTED). */
yl_status yl_stem_conv(const float* a_dev, const float* b_dev, float* out_dev, int32_t pass, int32_t k, int32_t stride,
                       int32_t batch, int32_t size, int32_t cin, int32_t cout, int32_t input_nchw, void* stream,
                       int32_t* launches);

/* ---- Mixed precision of the trainable backbone (stage and stem): the operand type of every DENSE GEMM, i.e. the stem's
 * 3x3 convolution and every 1x1 of stage and stem, in all three passes.  `mode` is 0 (fp32), YL_HEAD_F16 or YL_HEAD_BF16;
 * anything else, both bits among it, is YL_ERR_INVALID and changes nothing.  In a 16-bit mode both operands of each such
 * GEMM are rounded to nearest even inside the launch that consumes them (the 3x3 weight in its pack launch), products are
 * exact and accumulation is fp32 (v_mfma_f32_16x16x16_f16 / _bf16_1k); nothing is clamped, so an fp16 overflow is inf.
 * Parameters, saved activations, partial sums and every returned gradient stay fp32; the depthwise convolutions,
 * BatchNorm, ReLU, the residual add and every float64 sum are the same in all three modes, and so are the launch counts.
 * The setter changes the mode of the NEXT forward: a held forward keeps its own, and its backward runs in it.  _get reports
 * the handle's mode and the held forward's (0 when none is held); either pointer may be NULL.  The forward's `flags` go on
 * refusing the precision bits. */
yl_status yl_amp_stage_set(yl_stage* h, uint32_t mode);
yl_status yl_amp_stem_set(yl_stem* h, uint32_t mode);
yl_status yl_amp_stage_get(const yl_stage* h, uint32_t* mode, uint32_t* held_mode);
yl_status yl_amp_stem_get(const yl_stem* h, uint32_t* mode, uint32_t* held_mode);
/* yl_stem_conv in the operand type `mode` (yl_stem_conv itself is mode 0): same arguments, launches and alignment rules;
 * the packed weight of a 16-bit 3x3 pass takes half the temporary buffer. */
yl_status yl_amp_stem_conv(const float* a_dev, const float* b_dev, float* out_dev, int32_t pass, int32_t k, int32_t stride,
                           int32_t batch, int32_t size, int32_t cin, int32_t cout, int32_t input_nchw, uint32_t mode,
                           void* stream, int32_t* launches);

/* ---- training-time augmentation (csrc/yl_aug.hip) ------------------------------------------------------------------
 * The training sibling of yl_preprocess: replaces the dataset's 4-image mosaic (scripts/data/dataset.py:124-175) and
 * get_base_transform (scripts/data/augment.py:54-101) for a batch, in one launch with one bilinear gather per output
 * pixel.  `packed_u8_dev` holds BGR uint8 HWC images back to back (the packing of yl_preprocess); x_dev receives
 * [B,3,S,S] fp32 planar RGB.  Output image b shows a FRAME of frame_w x frame_h pixels made of num_tiles tiles
 * (tiles_dev[first_tile ...]); a tile is one source image stretched over the rectangle [x0,x1) x [y0,y1) of the frame
 * (1 tile: the frame is the image; 4 tiles: the quadrants of the mosaic canvas).  Per output pixel (x, y), in this order:
 *   1. y - top outside [0,nh) or x - left outside [0,nw): raw 114 in every channel, straight to step 8 (letterbox pad);
 *   2. (u, v) = ((m0 x + m1 y) + m2, (m3 x + m4 y) + m5): frame coordinates with pixel centres at +0.5; the host composes
 *      letterbox^-1, affine^-1 and the un-flip in float64 and rounds to fp32 once;
 *   3. (u, v) outside [0,frame_w) x [0,frame_h): 114 (the affine's constant border), which does go through 6 and 7;
 *   4. the first tile whose rectangle holds (u, v): fx = (u - x0) * (w0 / (x1 - x0)) - 0.5 (fy alike), fp32 bilinear
 *      a + (b - a) * frac along x, then along y, of the four neighbours, indices clamped to the source's edge;
 *   5. BGR -> RGB, then channel c takes RGB channel perm[c];
 *   6. color_mode (one per image; every result clipped to [0,255]): YL_AUG_BRIGHTNESS_CONTRAST v = color[0] v + color[1] 255;
 *      YL_AUG_HSV_SHIFT RGB -> HSV in fp32, hue + color[0] OpenCV hue units (2 degrees each, wrapped), saturation +
 *      color[1] / 255, value + color[2] (0..255 scale), clipped, back to RGB; YL_AUG_RGB_SHIFT v_c += color[c];
 *      YL_AUG_NONE and YL_AUG_CHANNEL_SHUFFLE (whose work is perm) change nothing;
 *   7. noise_sigma > 0: v += noise_sigma * (sum of twelve uniforms in [0,1) - 6), the uniforms 24-bit words of an
 *      integer-only uint32 counter hash of (noise_seed, channel, y, x, k); clipped to [0,255].  The result depends on
 *      the descriptor alone: not on the batch, the image's slot in it, or the launch geometry;
 *   8. (v - mean 255) * (1 / (std 255)) in fp32, the evaluate path's arithmetic ("pre_norm" 1 of yl_preprocess).
 * Only IEEE-exact fp32 operations, each rounded where written.  Takes no context, like yl_stem_conv; enqueues one kernel on
 * `stream` and returns.  NULL pointers, batch <= 0, batch > 65535, size <= 0 or size > 262140: YL_ERR_INVALID before any
 * device call.  The descriptors live on the device and are not validated: a tile's offset / h0 / w0 must lie inside
 * packed_u8_dev, h0, w0 >= 1 and first_tile + num_tiles inside tiles_dev.                                             */
enum { YL_AUG_NONE = 0, YL_AUG_BRIGHTNESS_CONTRAST = 1, YL_AUG_HSV_SHIFT = 2, YL_AUG_RGB_SHIFT = 3,
       YL_AUG_CHANNEL_SHUFFLE = 4 };
typedef struct yl_aug_tile {
  int64_t offset;             /* byte offset of the source image in packed_u8_dev ([h0][w0][3] BGR)                    */
  int32_t h0, w0;             /* source size                                                                          */
  float x0, y0, x1, y1;       /* the tile's rectangle in frame pixels                                                 */
} yl_aug_tile;
typedef struct yl_aug_image {
  int32_t first_tile, num_tiles;
  int32_t frame_w, frame_h;
  int32_t nh, nw, top, left;  /* letterbox of the frame in the S x S output                                           */
  float m[6];                 /* output pixel index -> frame coordinates, row-major 2x3                               */
  int32_t perm[3];            /* channel permutation over RGB (identity 0,1,2)                                        */
  int32_t color_mode;         /* YL_AUG_*                                                                             */
  float color[4];
  float noise_sigma;          /* 0: no noise                                                                          */
  uint32_t noise_seed;
} yl_aug_image;
yl_status yl_augment(const uint8_t* packed_u8_dev, const yl_aug_tile* tiles_dev, const yl_aug_image* imgs_dev,
                     int32_t batch, int32_t size, float* x_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YOLOLITE_HIP_H */
