// C ABI (include/yololite_hip.h): context, weight packing, forward executor, post-processing driver.
#include "yl_internal.h"
#include "yl_program.h"

#include <dlfcn.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <chrono>
#include <string>
#include <vector>

namespace {

// a validated layer (yl_program.h; its host weight pointers are nulled after packing) with its weight images on the device
struct DevLayer : YlLayerInfo {
#define YL_X(name) float* name = nullptr;
  YL_LAYER_IMAGES(YL_X)
#undef YL_X
};

struct Slot {
  int h, w, c;
  size_t sz = 0;         // bytes per image
  size_t off = 0;        // byte offset of the slot inside a chunk arena, per image of the chunk (x chunk capacity)
  bool pinned = false;   // whole-batch contiguous allocation of its own (tensors the ABI hands out: mask prototypes)
  float* pin = nullptr;
};

// The model: everything yl_create derives from the description, and the packed weights on the device.  Immutable once
// yl_create returns and SHARED by the contexts of one model (yl_clone: one context per batch in flight of a serving
// pipeline); the last owner frees the device images.
struct Model : YlGeometry, YlTables {
  int device = 0;
  std::vector<DevLayer> layers;
  float* zeros = nullptr;                  // 1 KiB of zeros (padding source for the conv kernels)
  Model() = default;
  Model(const Model&) = delete;
  Model& operator=(const Model&) = delete;
  ~Model() {
    if (!zeros && layers.empty()) return;
    hipSetDevice(device);
    hipFree(zeros);
    for (DevLayer& L : layers) {
#define YL_X(name) hipFree(L.name);
      YL_LAYER_IMAGES(YL_X)
#undef YL_X
    }
  }
};

}  // namespace

#define YL_GRAPH_SLOTS 4
#define YL_NMS_GROUPS 4
struct yl_ctx {
  std::shared_ptr<const Model> m;          // never null in a context yl_create / yl_clone handed out
  std::vector<Slot> slots;                 // the model's slots (m->slot_dims) with this context's placement
  int cap_batch = 0;                       // images the pinned slots / level buffers are allocated for (capacity)
  int act_batch = 0;                       // batch of the last forward: what yl_masks* / yl_read_slot may address
  // Activation memory: ONE arena per batch chunk (chunks run concurrently on their own streams), slots placed by
  // liveness -- a slot's bytes are reused by later tensors once its last consumer (launch group) has run.  edge_n,
  // B = 64: 3.8 GB with one buffer per tensor -> a few hundred MB, so that a chunk's producer -> consumer pairs have
  // a chance to meet in the 256 MB Infinity Cache instead of HBM.  "reuse_slots" 0 keeps every tensor (debugging).
  char* arena[4] = {nullptr, nullptr, nullptr, nullptr};
  int arena_capi[4] = {0, 0, 0, 0};        // images arena i is allocated for (a single-chunk call grows arena 0 only)
  float* se_scratch[4] = {nullptr, nullptr, nullptr, nullptr};   // YL_OP_SE partial sums of a chunk: [capi][m->se_unit]
  int plan_n = 0;                          // the current job's batch is split into this many chunks
  int arena_n = 0, arena_cap = 0;          // allocated: arenas, images of the largest one (plan_n / plan_cap <= these)
  int plan_b0[5] = {0, 0, 0, 0, 0};        // chunk i covers images [plan_b0[i], plan_b0[i + 1])
  int plan_cap = 0;                        // images of the largest chunk
  size_t arena_unit = 0;                   // arena bytes per image of a chunk (peak of the live set)
  bool plan_reuse = false;
  int opt_reuse = 1;
  int opt_time_split = 0;    // yl_predict records HIP events around the conv layers and the NMS (one chunk; eager or two hipGraphs)
  hipEvent_t ev_t[3] = {nullptr, nullptr, nullptr};
  bool timing_valid = false;
  int opt_pre_norm = 0;      // yl_preprocess: 0 = tools/infer.py arithmetic, 1 = the evaluate path's A.Normalize
  float* level_buf[YL_MAX_LEVELS] = {nullptr};
  // post-processing workspace
  float4* ws_boxes = nullptr;
  float* ws_scores = nullptr;
  int* ws_cls = nullptr;
  int* ws_clsws = nullptr;
  int* ws_kept_list = nullptr;               // [B][YL_NMS_GROUPS][N] class-group split of the NMS kernel
  int* ws_done = nullptr;                    // [B][256 bytes] class -> NMS workgroup table
  unsigned long long* ws_gkeys = nullptr;
  int gP = 0;
  float* ws_tmp_dets = nullptr;
  int* ws_tmp_idx = nullptr;
  int post_cap_batch = 0;
  // validation-loss scratch (yl_loss_af), sized on first use
  unsigned long long* ws_loss_keys = nullptr;   // [B][N]
  float* ws_loss_neg = nullptr;                 // [B][N]
  float* ws_loss_pi = nullptr;                  // [B][3]
  int* ws_loss_pos = nullptr;                   // [B]
  int loss_cap_batch = 0;
  // standalone nms scratch
  int* ws_nms_clsws = nullptr;
  unsigned long long* ws_nms_gkeys = nullptr;
  int nms_gP = 0;
  // options
  int opt_graph = 0, opt_tile_m = 0, opt_streams = 2;
  int opt_nms_groups = 0;    // workgroups per image in the NMS kernel: 1..4, 0 = auto (by confidence threshold, see do_post)
  int opt_hybrid = 0;        // (off: measured -0.5 % at B=64) full-batch launches for the high-resolution layers, batch chunks on the internal streams only
                             // for the run of low-resolution (<= 1/16) layers, see plan_segments()
                             // (m->small_lo / small_hi: that run).  "hybrid" 2 (the reverse plan): the run of <= 1/32-resolution
                             // layers (m->tiny_lo / tiny_hi) goes out as FULL-batch launches between two chunked segments (half as
                             // many latency-bound launches)
  int opt_batch_levels = 1;  // runs of independent, identically shaped layers (FPN smooth / head trunk / head out of all
                             // levels) go out as ONE launch (YlConvMulti)
  int opt_winograd = 1;      // dense 3x3 stride-1 layers with >= 64 channels through Winograd F(2x2,3x3) (2.25x fewer MACs;
                             // NOT bit-identical to the direct convolution: fp32 rounding of the transforms); 2 = only the
                             // >= 64-channel layers on the LARGEST grid they occur on (the finest pyramid level's smooth block).
                             // 1 = every eligible layer (>= 16 channels in and out) -- the DEFAULT since round 4: measured score
                             // error vs the oracle over 4 weight seeds x 32 images x 8400 candidates 0.9-1.6e-5 (yololite_m) /
                             // 0.7-1.2e-5 (yololite_m v2), no worse than the direct convolution's 1.4-1.7e-5 / 1.0-1.3e-5
                             // (profiles/r04_winograd_margin*.json)
  int opt_fuse_decode = 1;   // yl_predict: decode in the head-output conv's epilogue (no raw level tensor, no decode kernel)
  int opt_fuse_head = 1;     // ... and the head trunk (depthwise 3x3 -> 1x1) in the same launch (yl_conv_dpp_kernel)
  int opt_split_k = 0; // depthwise -> 1x1 layers on <= 20x20 grids in the split-K form (yl_conv_dwt_kernel<.., SK = 4>): -9 % batch-1
                      // latency, -0.7 % throughput at B = 64 (measured, edge_n) -> off by default, the pip API turns it on
  int opt_dev = 0;    // developer kernel-selection word (YL_DEV_*, "dev_select"); rides in every YlConvP
  int chain_launches = 0;   // yl_conv_dwx_kernel launches enqueued so far (yl_get_option "chain_launches", read-only)
  int pwx_launches = 0;     // yl_conv_pwx_kernel launches enqueued so far (yl_get_option "pwx_launches", read-only)
  int head_skip_launches = 0;       // fused head launches enqueued in the objectness-skip form ("head_skip_launches", read-only)
  int opt_head_skip_count = 0;      // "head_skip_count": those launches count their skipped tiles into head_skip_cnt
  unsigned* head_skip_cnt = nullptr;   // device counter ("head_skipped_tiles", read-only), allocated when the option is first set
  int opt_bf16 = 0;   // reduced-precision MFMA mode: 1 = conv / stem-block launches use the bf16-MFMA builds, 2 = the fp16-MFMA
                      // builds (fp32 storage, fp32 accumulate either way); 0 = fp32 (the parity path)
  // batch chunks run on `opt_streams` internal streams (fork/join around every call): the
  // latency-bound low-resolution layers of one chunk overlap the bandwidth-bound layers of another
  hipStream_t work[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[4] = {nullptr, nullptr, nullptr, nullptr};
  // branch lanes inside a chunk: neck/head layers that only feed the heads of the coarser levels (smooth5,
  // head5, smooth4, head4, ...) run on a side stream next to the 80x80 chain (lateral3 -> smooth3 -> head3);
  // m->lane[i] is derived from the slot graph at yl_create.  Off by default ("lanes" option): measured no gain
  // (29.3 k img/s either way) -- the conv grids are occupancy-sized persistent grids, so a second kernel only
  // gets CUs at the tail of the first
  int opt_lanes = 0;
  hipStream_t side[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_la[4] = {nullptr, nullptr, nullptr, nullptr}, ev_lb[4] = {nullptr, nullptr, nullptr, nullptr};
  // hipGraph cache keyed on everything baked into the captured launches: up to YL_GRAPH_SLOTS jobs (a serving loop alternates
  // between a few input / output buffers, e.g. the two slots of the pipelined all-gather), least recently used evicted
  struct GraphEntry {
    std::vector<hipGraphExec_t> execs;   // one graph per (segment, chunk) piece, in launch order
    int n = 0;
    std::vector<unsigned char> key;
    unsigned long long stamp = 0;
  };
  std::vector<GraphEntry> graphs;
  unsigned long long graph_clock = 0;
  std::string err;
};

namespace {

// function attributes (dynamic-LDS opt-ins) are per DEVICE: one flag per device ordinal
bool g_inited[64] = {false};

yl_status fail(yl_ctx* c, yl_status s, const std::string& msg) {
  if (c) c->err = msg;
  return s;
}

#define HIPCHK(ctx, expr)                                                                        \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess) {                                                                      \
      char _b[512];                                                                              \
      snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,  \
               __LINE__);                                                                        \
      return fail(ctx, (_e == hipErrorOutOfMemory) ? YL_ERR_NOMEM : YL_ERR_HIP, _b);             \
    }                                                                                            \
  } while (0)

template <typename T>
yl_status upload(yl_ctx* c, const std::vector<T>& h, T** d) {
  *d = nullptr;
  if (h.empty()) return YL_OK;
  HIPCHK(c, hipMalloc((void**)d, h.size() * sizeof(T)));
  HIPCHK(c, hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return YL_OK;
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// a context's slots: the model's dimensions, nothing placed yet
void init_slots(yl_ctx* c) {
  c->slots.assign(c->m->slot_dims.size(), Slot());
  for (size_t i = 0; i < c->slots.size(); ++i) { c->slots[i].h = c->m->slot_dims[i].h; c->slots[i].w = c->m->slot_dims[i].w; c->slots[i].c = c->m->slot_dims[i].c; }
}

void drop_graph(yl_ctx* c);

void free_post_ws(yl_ctx* c) {
  drop_graph(c);                        // cached graphs have the workspace pointers baked in
  hipFree(c->ws_boxes); hipFree(c->ws_scores); hipFree(c->ws_cls); hipFree(c->ws_clsws);
  hipFree(c->ws_kept_list); hipFree(c->ws_done);
  c->ws_kept_list = nullptr; c->ws_done = nullptr;
  hipFree(c->ws_gkeys); hipFree(c->ws_tmp_dets); hipFree(c->ws_tmp_idx);
  c->ws_boxes = nullptr; c->ws_scores = nullptr; c->ws_cls = nullptr; c->ws_clsws = nullptr;
  c->ws_gkeys = nullptr; c->ws_tmp_dets = nullptr; c->ws_tmp_idx = nullptr;
  c->post_cap_batch = 0;
}

void drop_graph(yl_ctx* c) {
  for (auto& g : c->graphs)
    for (auto e : g.execs)
      if (e) hipGraphExecDestroy(e);
  c->graphs.clear();
}

void free_act(yl_ctx* c) {
  drop_graph(c);
  for (int i = 0; i < 4; ++i) {
    hipFree(c->arena[i]); c->arena[i] = nullptr; c->arena_capi[i] = 0;
    hipFree(c->se_scratch[i]); c->se_scratch[i] = nullptr;
  }
  for (auto& s : c->slots) { hipFree(s.pin); s.pin = nullptr; }
  for (int l = 0; l < YL_MAX_LEVELS; ++l) { hipFree(c->level_buf[l]); c->level_buf[l] = nullptr; }
  c->cap_batch = 0; c->plan_n = 0; c->arena_n = 0; c->arena_cap = 0; c->act_batch = 0;
}

int pow2ceil(int v) { int p = 64; while (p < v) p <<= 1; return p; }

// ---- what the next launch is.  One owner: run_layers emits what next_step says, plan_slots groups by it.

enum LaunchForm { F_LAYER, F_BATCHED, F_HEAD_RUN, F_DPQ_EXPAND, F_DPQ_PAIR, F_DWX_CHAIN, F_PW_PAIR, F_SPLIT_HEAD };
// first: the step's first program layer; width: members of the level-batched run (1..4); layers: program layers consumed
struct LaunchStep { LaunchForm form; size_t first; int width; int layers; };
constexpr unsigned form_bit(LaunchForm f) { return 1u << f; }

// layers [i, end) that go out as ONE launch (level-batched heads / smooth blocks): same kernel
// configuration, no residual / upsample operands, no dependency inside the run
size_t layer_group_end(const yl_ctx* c, size_t i, size_t lend) {
  auto same_shape = [&](size_t x, size_t y) {
    const yl_layer& a = c->m->layers[x].d; const yl_layer& e = c->m->layers[y].d;
    return a.op == YL_OP_CONV && e.op == YL_OP_CONV && a.cin == e.cin && a.cout == e.cout && a.k == e.k &&
           a.stride == e.stride && a.pad_t == e.pad_t && a.pad_l == e.pad_l && a.act == e.act &&
           !YL_ACT_POSTPASS(a.act) && a.in_shift == e.in_shift && a.dw_k == e.dw_k && a.dw_stride == e.dw_stride && a.dw_pad_t == e.dw_pad_t &&
           a.dw_pad_l == e.dw_pad_l && a.dw_act == e.dw_act && a.c2 == 0 && e.c2 == 0 && a.scale_slot < 0 && e.scale_slot < 0 && a.res_slot < 0 &&
           e.res_slot < 0 && a.up_slot < 0 && e.up_slot < 0 && (a.head_level >= 0) == (e.head_level >= 0) &&
           (a.cout + 15) / 16 <= 8;
  };
  size_t gend = i + 1;
  if (c->m->layers[i].d.op != YL_OP_CONV) return gend;
  while (gend < lend && gend - i < 4 && same_shape(i, gend)) {
    bool dep = false;
    for (size_t q = i; q < gend; ++q)
      if (c->m->layers[q].d.head_level < 0 && c->m->layers[q].d.out_slot == c->m->layers[gend].d.in_slot) dep = true;
    if (dep) break;
    ++gend;
  }
  return gend;
}

// The shape predicates know nothing of the options (allowed_forms).
// The first layer of a head run or a dpq pair: depthwise 3x3 stride 1 -> 1x1 on an unchanged grid, no other operand, written to
// a slot with a single reader (the caller checks that it is the step's second layer's input)
bool dw3_trunk(const yl_ctx* c, const DevLayer& T) {
  const yl_layer& t = T.d;
  return t.op == YL_OP_CONV && t.k == 1 && t.dw_k == 3 && t.dw_stride == 1 && t.c2 == 0 && t.c3 == 0 && t.head_level < 0 &&
         t.res_slot < 0 && t.up_slot < 0 && !t.in_shift && !YL_SMOOTH(t.act) && !YL_SMOOTH(t.dw_act) && t.out_slot >= 0 &&
         T.in_h == T.out_h && T.in_w == T.out_w && c->m->readers[t.out_slot] == 1;
}

// Head branches as ONE launch (yl_conv_dpp_kernel): the level-batched run [i, i + n) of head trunks (depthwise 3x3 -> 1x1)
// is followed by the run of their head-output convs in the same order, nothing else reads the trunk tensors, no mask
// coefficients and the shape is instantiated
bool head_run_fusable(const yl_ctx* c, size_t i, size_t n, size_t lend) {
  if (c->m->NM > 0 || i + 2 * n > lend) return false;
  for (size_t q = 0; q < n; ++q) {
    const DevLayer& T = c->m->layers[i + q];
    const DevLayer& O = c->m->layers[i + n + q];
    const yl_layer& t = T.d; const yl_layer& o = O.d;
    if (o.op != YL_OP_CONV || o.head_level < 0 || o.k != 1 || o.dw_k > 0 || o.c2 > 0 || o.c3 > 0 || o.in_slot != t.out_slot ||
        o.cin != t.cout || o.act != YL_ACT_NONE || o.res_slot >= 0 || o.up_slot >= 0 || o.in_shift)
      return false;
    if (!dw3_trunk(c, T) || !yl_dpp_supported(t.cin, t.cout, o.cout, T.out_h, T.out_w)) return false;
  }
  return true;
}

// depthwise 3x3 -> 1x1 expand -> 1x1 project (+residual) as ONE launch (yl_conv_dpq_kernel): layer i is the depthwise +
// expand conv, layer i + 1 the plain 1x1 that consumes it, nothing else reads the expanded tensor, shape instantiated
bool pair_fusable(const yl_ctx* c, size_t i, size_t lend) {
  if (i + 1 >= lend) return false;
  const DevLayer& T = c->m->layers[i];
  const yl_layer& t = T.d; const yl_layer& o = c->m->layers[i + 1].d;
  if (!dw3_trunk(c, T)) return false;
  if (o.op != YL_OP_CONV || o.head_level >= 0 || o.k != 1 || o.dw_k > 0 || o.c2 > 0 || o.c3 > 0 || o.in_slot != t.out_slot ||
      o.cin != t.cout || YL_SMOOTH(o.act) || o.up_slot >= 0 || o.in_shift || o.res_slot == t.out_slot ||
      o.scale_slot >= 0 || t.scale_slot >= 0)
    return false;
  return yl_dpq_supported(t.cin, t.cout, o.cout, T.out_h, T.out_w);
}

// wide depthwise 3x3 -> 1x1 layer (more than 96 outputs) on its own: yl_conv_dpq_kernel's expand-only form computes the
// depthwise part once per pixel
bool expand_fusable(const yl_ctx* c, size_t i) {
  const DevLayer& T = c->m->layers[i];
  const yl_layer& d = T.d;
  return d.op == YL_OP_CONV && d.dw_k == 3 && d.dw_stride == 1 && d.k == 1 && d.c2 == 0 && d.c3 == 0 && d.head_level < 0 &&
         d.res_slot < 0 && d.up_slot < 0 && !d.in_shift && d.cout > 96 && T.in_h == T.out_h &&
         yl_dpq_supported(d.cin, d.cout, 0, T.out_h, T.out_w);
}

// UIB projection -> the next block's expansion as ONE launch (yl_conv_dwx_kernel): layer i is a 1x1 conv with a stride-1
// depthwise prologue (optional residual) writing slot S, layer i + 1 a plain 1x1 conv (no prologue, residual, upsample,
// gate or head) reading S.  S is still written -- the next block reads it as its residual.
bool chain_fusable(const yl_ctx* c, size_t i, size_t lend) {
  if (i + 1 >= lend) return false;
  const DevLayer& T = c->m->layers[i];
  const DevLayer& O = c->m->layers[i + 1];
  const yl_layer& t = T.d; const yl_layer& o = O.d;
  if (t.op != YL_OP_CONV || t.k != 1 || t.stride != 1 || t.dw_k <= 0 || t.dw_stride != 1 || t.c2 > 0 || t.c3 > 0 ||
      t.head_level >= 0 || t.up_slot >= 0 || t.scale_slot >= 0 || t.in_shift || YL_SMOOTH(t.act) || t.out_slot < 0 ||
      (t.res_slot >= 0 && t.act != YL_ACT_NONE))
    return false;
  if (o.op != YL_OP_CONV || o.head_level >= 0 || o.k != 1 || o.stride != 1 || o.dw_k > 0 || o.c2 > 0 || o.c3 > 0 ||
      o.in_slot != t.out_slot || o.cin != t.cout || YL_SMOOTH(o.act) || o.res_slot >= 0 || o.up_slot >= 0 ||
      o.scale_slot >= 0 || o.in_shift || o.out_slot < 0)
    return false;
  return T.in_h == T.out_h && T.in_w == T.out_w && O.in_h == T.out_h && O.in_w == T.out_w && O.out_h == T.out_h &&
         O.out_w == T.out_w && yl_dwx_supported(t.cin, t.cout, t.dw_k, t.dw_stride, o.cout, T.out_h, T.out_w);
}

// Two plain 1x1 convs on one grid as ONE launch (yl_conv_pwx_kernel): layer i writes slot S (bias, ReLU-family activation or
// none, no other operand), layer i + 1 is its only reader (no residual, upsample addend, gate or head).  S is not written.
bool pwx_fusable(const yl_ctx* c, size_t i, size_t lend) {
  if (i + 1 >= lend) return false;
  const DevLayer& T = c->m->layers[i];
  const DevLayer& O = c->m->layers[i + 1];
  const yl_layer& t = T.d; const yl_layer& o = O.d;
  if (t.op != YL_OP_CONV || t.k != 1 || t.stride != 1 || t.dw_k > 0 || t.c2 > 0 || t.c3 > 0 || t.head_level >= 0 ||
      t.res_slot >= 0 || t.up_slot >= 0 || t.scale_slot >= 0 || t.in_shift || YL_SMOOTH(t.act) || t.out_slot < 0 ||
      c->m->readers[t.out_slot] != 1)
    return false;
  if (o.op != YL_OP_CONV || o.head_level >= 0 || o.k != 1 || o.stride != 1 || o.dw_k > 0 || o.c2 > 0 || o.c3 > 0 ||
      o.in_slot != t.out_slot || o.cin != t.cout || YL_SMOOTH(o.act) || o.res_slot >= 0 || o.up_slot >= 0 ||
      o.scale_slot >= 0 || o.in_shift || o.out_slot < 0)
    return false;
  return T.in_h == T.out_h && T.in_w == T.out_w && O.in_h == T.out_h && O.in_w == T.out_w && O.out_h == T.out_h &&
         O.out_w == T.out_w && yl_pwx_supported(t.cin, t.cout, o.cout);
}

// The forms the options allow a run_layers call (F_LAYER always is): the option tests, here and nowhere else.
// per_layer: per-layer timing or side lanes; fuse: yl_predict with decode in the head-output epilogue
unsigned allowed_forms(const yl_ctx* c, bool per_layer, bool fuse) {
  if (per_layer) return 0;
  unsigned f = c->opt_batch_levels ? form_bit(F_BATCHED) : 0;
  if (c->opt_fuse_head && !c->opt_bf16) f |= form_bit(F_DPQ_EXPAND) | form_bit(F_DPQ_PAIR) | (fuse ? form_bit(F_HEAD_RUN) : 0);
  if (c->opt_fuse_head && fuse) f |= form_bit(F_SPLIT_HEAD);
  // fp32 mode, split-K off (its form keeps the two launches), the automatic kernel choice, the depthwise -> 1x1 kernel and the
  // chaining not switched off
  if (!(c->opt_bf16 || c->opt_split_k || c->opt_tile_m || (c->opt_dev & (YL_DEV_CHAIN_OFF | YL_DEV_DWT_OFF)))) f |= form_bit(F_DWX_CHAIN);
  // the 1x1 pair: the same, its own switch
  if (!(c->opt_bf16 || c->opt_split_k || c->opt_tile_m || (c->opt_dev & YL_DEV_PWX_OFF))) f |= form_bit(F_PW_PAIR);
  return f;
}

// The launch that starts at layer i of [.., lend): the first of `forms` (form_bit set) that applies, in the order head run,
// expand-only dpq, dpq pair, dwx chain, 1x1 pair, split head, level-batched run, else the single layer.  Without F_BATCHED layer i is
// looked at on its own, as "batch_levels" 0 does.
LaunchStep next_step(const yl_ctx* c, size_t i, size_t lend, unsigned forms) {
  if (c->m->layers[i].d.op != YL_OP_CONV) return {F_LAYER, i, 1, 1};
  auto may = [&](LaunchForm f) { return (forms & form_bit(f)) != 0; };
  const size_t n = may(F_BATCHED) ? layer_group_end(c, i, lend) - i : 1;
  if (may(F_HEAD_RUN) && head_run_fusable(c, i, n, lend)) return {F_HEAD_RUN, i, (int)n, (int)(2 * n)};
  if (n == 1) {
    const bool pair = (may(F_DPQ_EXPAND) || may(F_DPQ_PAIR)) && pair_fusable(c, i, lend);
    if (may(F_DPQ_EXPAND) && !pair && expand_fusable(c, i)) return {F_DPQ_EXPAND, i, 1, 1};
    if (may(F_DPQ_PAIR) && pair) return {F_DPQ_PAIR, i, 1, 2};
    if (may(F_DWX_CHAIN) && chain_fusable(c, i, lend)) return {F_DWX_CHAIN, i, 1, 2};
    if (may(F_PW_PAIR) && pwx_fusable(c, i, lend)) return {F_PW_PAIR, i, 1, 2};
  }
  // head-output convs of a model with mask coefficients, every one packed as two weight images
  if (may(F_SPLIT_HEAD) && c->m->layers[i].d.head_level >= 0 &&
      std::all_of(c->m->layers.begin() + i, c->m->layers.begin() + i + n, [](const DevLayer& L) { return L.wp_det != nullptr; }))
    return {F_SPLIT_HEAD, i, (int)n, (int)n};
  return {n > 1 ? F_BATCHED : F_LAYER, i, (int)n, (int)n};
}

// Place the slots inside a chunk arena.  Liveness is tracked per LAUNCH GROUP (a level-batched run reads and writes
// all of its layers' tensors at once): slot s is live from the group that produces it to the group of its last
// consumer, inclusive; first-fit over the gaps of the live set.  reuse == false: every slot gets its own range.
void plan_slots(yl_ctx* c, bool reuse) {
  const size_t NL = c->m->layers.size(), NS = c->slots.size();
  std::vector<int> grp(NL, 0);
  int g = 0;
  // A group is whatever next_step could send out as one launch under ANY setting of the options (a fused launch writes its
  // last layer's output while other tiles still read its first layer's inputs): the level-batched run at i, plus one more
  // layer while the group's last member, on its own, can head a two-layer step.
  for (size_t i = 0; i < NL; ++g) {
    size_t e = i + (size_t)next_step(c, i, NL, form_bit(F_BATCHED)).width;
    // (again from the layer added: with the first pair's form off or refused, its second layer can head a pair of its own --
    // a dwx chain's expansion and the plain 1x1 behind it as yl_conv_pwx_kernel -- whose output must not lie over the first
    // layer's output, which that launch reads)
    while (next_step(c, e - 1, NL, form_bit(F_DPQ_PAIR) | form_bit(F_DWX_CHAIN) | form_bit(F_PW_PAIR)).layers == 2) e = e + 1;
    for (size_t q = i; q < e; ++q) grp[q] = g;
    i = e;
  }
  const int INF = 1 << 30;
  std::vector<int> def(NS, INF), last(NS, -1);
  for (size_t i = 0; i < NL; ++i) {
    const yl_layer& d = c->m->layers[i].d;
    if (d.head_level < 0 && d.out_slot >= 0 && grp[i] < def[d.out_slot]) def[d.out_slot] = grp[i];
    const int ins[4] = {(d.op == YL_OP_STEM || d.op == YL_OP_STEMBLOCK || d.op == YL_OP_NHWC4) ? -1 : d.in_slot, d.res_slot, d.up_slot, d.scale_slot};
    for (int k = 0; k < 4; ++k)
      if (ins[k] >= 0 && grp[i] > last[ins[k]]) last[ins[k]] = grp[i];
  }
  for (size_t s = 0; s < NS; ++s) {
    Slot& t = c->slots[s];
    t.pinned = (int)s == c->m->proto_slot;
    // fp16-storage mode ("store_f16"): activation tensors are fp16; the pinned prototypes (the mask kernels read them) and the
    // squeeze-excite gates (yl_se.hip writes them, the gated 1x1 convs read them: fp32 [B][C] vectors) stay fp32
    bool f32 = c->opt_bf16 != 3 || t.pinned;
    for (size_t i = 0; i < NL && !f32; ++i) f32 = c->m->layers[i].d.op == YL_OP_SE && c->m->layers[i].d.out_slot == (int)s;
    t.sz = (size_t)t.h * t.w * t.c * (f32 ? sizeof(float) : sizeof(_Float16));   // images of a slot are contiguous (a multiple of 8 B)
    if (last[s] < def[s]) last[s] = def[s] == INF ? -1 : def[s];     // produced, never consumed: live in its own group
  }
  struct Iv { size_t off, sz; int last; };
  std::vector<Iv> live;
  size_t peak = 0;
  std::vector<size_t> order;
  for (size_t s = 0; s < NS; ++s) if (!c->slots[s].pinned && def[s] != INF) order.push_back(s);
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return def[a] < def[b]; });
  size_t bump = 0;
  for (size_t s : order) {
    Slot& t = c->slots[s];
    const size_t need = (t.sz + 255) & ~(size_t)255;                  // placement granule: slot bases stay 256-B aligned
    if (!reuse) { t.off = bump; bump += need; peak = bump; continue; }
    live.erase(std::remove_if(live.begin(), live.end(), [&](const Iv& v) { return v.last < def[s]; }), live.end());
    std::sort(live.begin(), live.end(), [](const Iv& a, const Iv& b) { return a.off < b.off; });
    size_t at = 0;
    for (const Iv& v : live) {
      if (at + need <= v.off) break;
      if (v.off + v.sz > at) at = v.off + v.sz;
    }
    t.off = at;
    live.push_back({at, need, last[s]});
    if (at + need > peak) peak = at + need;
  }
  c->arena_unit = peak;
}

// bytes of detection level l for B images
size_t level_bytes(const yl_ctx* c, int l, int B) {
  return (size_t)B * c->m->level_A[l] * c->m->level_S[l] * c->m->level_S[l] * c->m->E * sizeof(float);
}

// number of batch chunks a job of B images is split into (submit / walk_plan)
int chunks_for(const yl_ctx* c, int B) {
  if (c->opt_time_split) return 1;          // the infer / post split is defined on ONE stream
  int n = c->opt_streams < 1 ? 1 : (c->opt_streams > 4 ? 4 : c->opt_streams);
  if (B < 4 * n) n = 1;
  return n;
}

// activations for a batch of B images processed as n chunks (the split walk_plan uses), one arena per chunk.
// The hybrid plan mixes full-batch and chunked segments and the side-lane option runs layers of one chunk
// concurrently: both get ONE arena with every tensor kept (any image range addressable, nothing reused).
yl_status ensure_act(yl_ctx* c, int B, int n) {
  const bool flat = c->opt_hybrid || c->opt_lanes;
  if (flat) n = 1;
  const bool reuse = c->opt_reuse && !flat;
  // the chunk split of THIS job
  int b0s[5] = {0, 0, 0, 0, 0}, cap = 0;
  {
    const int base = B / n, rem = B % n;
    int b0 = 0;
    for (int i = 0; i < n; ++i) {
      const int bn = base + (i < rem ? 1 : 0);
      b0s[i] = b0;
      b0 += bn;
      if (bn > cap) cap = bn;
    }
    b0s[n] = B;
  }
  // CAPACITY only grows: a smaller batch (a tail batch, alternating B = 4 / 16, a "time_split" toggle) re-plans its
  // chunk ranges inside the existing allocations -- no hipFree (a device sync), no dropped hipGraphs (their keys carry
  // the batch, so graphs of several batch sizes live side by side in the LRU), and the level buffers / prototypes of
  // the previous batch stay where yl_masks* reads them.  Slot addresses inside an arena scale with plan_cap
  // (slot_addr), i.e. a job's addresses are a function of (B, n) as long as the allocation does not move.
  // Per-arena capacity: a single-chunk call (time_split, per-layer timing) after a two-chunk run grows
  // arena 0 to the full batch and leaves the others at the chunk size -- not every arena at the full batch.
  bool grow = B > c->cap_batch || n > c->arena_n || reuse != c->plan_reuse || c->arena_n == 0;
  for (int i = 0; i < n && !grow; ++i) grow = cap > c->arena_capi[i];
  if (grow) {
    const int newB = B > c->cap_batch ? B : c->cap_batch, newn = n > c->arena_n ? n : c->arena_n;
    int capi[4], newcap = 0;
    for (int i = 0; i < 4; ++i) {
      capi[i] = i < newn ? c->arena_capi[i] : 0;
      if (i < n && cap > capi[i]) capi[i] = cap;
      if (capi[i] > newcap) newcap = capi[i];
    }
    free_act(c);                                             // also drops the cached graphs (addresses change)
    c->plan_reuse = reuse;
    plan_slots(c, reuse);
    // The arenas and pinned slots carry 256 spare bytes and start out as zeros (0xFF bytes under YL_DEV_POISON).  No kernel
    // needs either: the channel tail of a tensor's last k-block is masked in every conv kernel (those lanes load zeros, not the
    // next pixel's channels), so a result depends on nothing but its own image -- the isolation tests fill every byte here
    // with NaN and compare bitwise.
    const int fill = (c->opt_dev & YL_DEV_POISON) ? 0xFF : 0;
    for (int i = 0; i < newn; ++i) {
      if (c->arena_unit) {
        HIPCHK(c, hipMalloc((void**)&c->arena[i], c->arena_unit * (size_t)capi[i] + 256));
        HIPCHK(c, hipMemset(c->arena[i], fill, c->arena_unit * (size_t)capi[i] + 256));
      }
      if (c->m->se_unit) {
        HIPCHK(c, hipMalloc((void**)&c->se_scratch[i], c->m->se_unit * sizeof(float) * (size_t)capi[i]));
        if (fill) HIPCHK(c, hipMemset(c->se_scratch[i], fill, c->m->se_unit * sizeof(float) * (size_t)capi[i]));
      }
      c->arena_capi[i] = capi[i];
    }
    for (auto& s : c->slots)
      if (s.pinned) {
        HIPCHK(c, hipMalloc((void**)&s.pin, s.sz * (size_t)newB + 256));
        HIPCHK(c, hipMemset(s.pin, fill, s.sz * (size_t)newB + 256));
      }
    for (int l = 0; l < c->m->L; ++l) {
      HIPCHK(c, hipMalloc((void**)&c->level_buf[l], level_bytes(c, l, newB)));
      if (fill) HIPCHK(c, hipMemset(c->level_buf[l], fill, level_bytes(c, l, newB)));
    }
    c->cap_batch = newB; c->arena_n = newn; c->arena_cap = newcap;
  }
  c->plan_n = n; c->plan_cap = cap;
  for (int i = 0; i <= n; ++i) c->plan_b0[i] = b0s[i];
  c->act_batch = B;
  return YL_OK;
}

// YL_DEV_POISON: refill every activation buffer ensure_act allocated with 0xFF bytes on the call's stream, ahead of the call's
// first launch (the chunk streams and side lanes fork from `st` after this), so that no call sees what an earlier one wrote.
// Float / fp16 storage only: the post-processing workspaces (counts, indices, NMS keys) are never poisoned.
yl_status poison_act(yl_ctx* c, hipStream_t st) {
  if (!(c->opt_dev & YL_DEV_POISON)) return YL_OK;
  for (int i = 0; i < c->arena_n; ++i) {
    if (c->arena[i]) HIPCHK(c, hipMemsetAsync(c->arena[i], 0xFF, c->arena_unit * (size_t)c->arena_capi[i] + 256, st));
    if (c->se_scratch[i]) HIPCHK(c, hipMemsetAsync(c->se_scratch[i], 0xFF, c->m->se_unit * sizeof(float) * (size_t)c->arena_capi[i], st));
  }
  for (auto& s : c->slots)
    if (s.pinned && s.pin) HIPCHK(c, hipMemsetAsync(s.pin, 0xFF, s.sz * (size_t)c->cap_batch + 256, st));
  for (int l = 0; l < c->m->L; ++l)
    if (c->level_buf[l]) HIPCHK(c, hipMemsetAsync(c->level_buf[l], 0xFF, level_bytes(c, l, c->cap_batch), st));
  return YL_OK;
}

// the planned chunk (and with it the arena) that image b lives in
int chunk_of(const yl_ctx* c, int b) {
  int ch = 0;
  while (ch + 1 < c->plan_n && b >= c->plan_b0[ch + 1]) ++ch;
  return ch;
}

// image b of slot `sl` (b must lie in the planned chunk that contains it)
float* slot_addr(const yl_ctx* c, int sl, int b) {
  const Slot& t = c->slots[sl];
  if (t.pinned) return (float*)((char*)t.pin + (size_t)b * t.sz);
  const int ch = chunk_of(c, b);
  return (float*)(c->arena[ch] + t.off * (size_t)c->plan_cap + (size_t)(b - c->plan_b0[ch]) * t.sz);
}

// image b's part of its chunk's partial-sum scratch (squeeze-excite / GRN pooling)
float* se_partial(const yl_ctx* c, int b) {
  const int ch = chunk_of(c, b);
  return c->se_scratch[ch] + (size_t)(b - c->plan_b0[ch]) * c->m->se_unit;
}

yl_status ensure_post(yl_ctx* c, int B) {
  if (B <= c->post_cap_batch) return YL_OK;
  free_post_ws(c);
  const size_t n = (size_t)B * c->m->N;
  HIPCHK(c, hipMalloc((void**)&c->ws_boxes, n * sizeof(float4)));
  HIPCHK(c, hipMalloc((void**)&c->ws_scores, n * sizeof(float)));
  HIPCHK(c, hipMalloc((void**)&c->ws_cls, n * sizeof(int)));
  const int Cw = c->m->C > 0 ? c->m->C : 1;
  HIPCHK(c, hipMalloc((void**)&c->ws_clsws, (size_t)B * 4 * Cw * sizeof(int)));
  c->gP = pow2ceil(c->m->N);
  if (c->gP > YL_LDS_KEYS_MAX) HIPCHK(c, hipMalloc((void**)&c->ws_gkeys, (size_t)B * c->gP * 8));
  HIPCHK(c, hipMalloc((void**)&c->ws_tmp_dets, n * 6 * sizeof(float)));
  HIPCHK(c, hipMalloc((void**)&c->ws_tmp_idx, n * sizeof(int)));
  HIPCHK(c, hipMalloc((void**)&c->ws_kept_list, n * YL_NMS_GROUPS * sizeof(int)));
  HIPCHK(c, hipMalloc((void**)&c->ws_done, (size_t)B * 256));        // class -> NMS workgroup table per image
  c->post_cap_batch = B;
  return YL_OK;
}

void fill_levels(const yl_ctx* c, const float* const* ptrs, YlLevels& lv) {
  memset(&lv, 0, sizeof(lv));
  lv.L = c->m->L; lv.N = c->m->N; lv.E = c->m->E; lv.C = c->m->C;
  lv.hi = (float)(c->m->img_size - 1);
  for (int l = 0; l < c->m->L; ++l) {
    lv.ptr[l] = ptrs[l];
    lv.S[l] = c->m->level_S[l];
    lv.A[l] = c->m->level_A[l];
    lv.off[l] = c->m->level_off[l];
    lv.stride[l] = (float)((double)c->m->img_size / (double)c->m->level_S[l]);   // utils_ms.py:71
  }
  lv.off[c->m->L] = c->m->N;
}

// builds the kernel parameter block of layer i for batch B
void layer_params(const yl_ctx* c, const DevLayer& L, int b0, int B, const float* x, float* const* level_out,
                  YlConvP& p) {
  memset(&p, 0, sizeof(p));
  const yl_layer& d = L.d;
  p.wp = L.wp; p.bias = L.bias; p.dw_w = L.dw_w; p.dw_b = L.dw_b;
  // fp32 only: the committed Winograd error margins (profiles/r04_winograd_margin*.json) were measured with fp32 operands; with
  // 16-bit operands the transformed inputs and U = G g G^T would be rounded before the multiply
  p.wino = !c->opt_bf16 && (c->opt_winograd == 1 ||
            (c->opt_winograd == 2 && d.cin >= 64 && d.cout >= 64 && L.out_h * L.out_w >= c->m->wino_max_hw)) ? L.wino : nullptr;
  p.zeros = c->m->zeros;
  p.B = B; p.H = L.in_h; p.W = L.in_w; p.Cin = d.cin;
  p.OH = L.out_h; p.OW = L.out_w; p.N = d.cout;
  p.k = d.k; p.stride = d.stride; p.pad_t = d.pad_t; p.pad_l = d.pad_l; p.act = d.act;
  p.in_shift = d.in_shift;
  p.dw_k = d.dw_k; p.dw_stride = d.dw_stride; p.dw_pad_t = d.dw_pad_t; p.dw_pad_l = d.dw_pad_l; p.dw_act = d.dw_act;
  p.MH = L.out_h; p.MW = L.out_w;
  p.KB = cdiv(d.cin, 16);
  p.TK = d.k * d.k * p.KB;
  p.NTtot = cdiv(d.cout, 16);
  p.M = B * L.out_h * L.out_w;
  auto slot_ptr = [&](int sl) { return slot_addr(c, sl, b0); };
  p.x = (d.op == YL_OP_STEM || d.op == YL_OP_STEMBLOCK || d.op == YL_OP_NHWC4) ? x + (size_t)b0 * 3 * L.in_h * L.in_w : slot_ptr(d.in_slot);
  if (d.op == YL_OP_CONV && d.c2 > 0) {      // fused expand -> depthwise -> project
    p.w2p = L.w2p; p.b2 = L.b2; p.C1 = d.c2; p.act2 = d.act2;
  }
  if (d.op == YL_OP_CONV && d.c3 > 0) {      // dense k x k conv with a chained 1x1 conv (yl_conv_mfma_kernel epilogue)
    p.w3p = L.w3p; p.b3 = L.b3; p.C3 = d.c3; p.act3 = d.act3;
  }
  if (d.op == YL_OP_STEMBLOCK) {
    p.w2p = L.w2p; p.b2 = L.b2; p.w3p = L.w3p; p.b3 = L.b3;
    p.C1 = d.cout; p.C2 = d.c2; p.C3 = d.c3; p.act2 = d.act2; p.act3 = d.act3;
    p.SH = p.SW = (L.in_h + d.pad_t + (d.k - 1 - d.pad_t) - d.k) / d.stride + 1;
    p.tiles_x = cdiv(L.out_w, 8); p.tiles_y = cdiv(L.out_h, 8);
    p.ntiles = B * p.tiles_x * p.tiles_y;
    p.N = d.c3 > 0 ? d.c3 : d.c2;
  }
  if (d.res_slot >= 0) p.res = slot_ptr(d.res_slot);
  if (YL_ACT_POSTPASS(d.act)) { p.act = YL_ACT_NONE; p.res = nullptr; }     // applied by the activation pass (run_layers)
  if (d.scale_slot >= 0) p.scale = slot_ptr(d.scale_slot);
  p.dev = (unsigned)c->opt_dev | (c->opt_split_k ? 0u : YL_DEV_DWT_NOSPLIT);
  if (d.up_slot >= 0) {
    p.up = slot_ptr(d.up_slot);
    p.UH = c->slots[d.up_slot].h; p.UW = c->slots[d.up_slot].w;
  }
  p.out_f32 = (c->opt_bf16 == 3 && (d.head_level >= 0 || d.out_slot == c->m->proto_slot)) ? 1 : 0;
  if (d.head_level >= 0) {
    const int l = d.head_level;
    const int ss = c->m->level_S[l] * c->m->level_S[l];
    p.out_bstride = (long)c->m->level_A[l] * ss * c->m->E;
    p.out = level_out[l] + (size_t)b0 * p.out_bstride + (size_t)L.head_anchor * ss * c->m->E;
  } else {
    p.out = slot_ptr(d.out_slot);
    p.out_bstride = (long)L.out_h * L.out_w * ((d.op == YL_OP_CONV && d.c3 > 0) ? d.c3 : d.cout);
  }
}

// decode can be fused into the head-output convs when every one of them is a plain 1x1 conv whose 5+C(+masks)
// columns fit one block's n-tiles (<= 128)
bool can_fuse_decode(const yl_ctx* c) {
  if (!c->opt_fuse_decode) return false;
  bool any = false;
  for (const auto& L : c->m->layers) {
    if (L.d.head_level < 0) continue;
    if (L.d.op != YL_OP_CONV || L.d.k != 1 || L.d.dw_k > 0 || L.d.c2 > 0 || L.d.cout > 128 || L.d.cout != c->m->E ||
        L.d.act != YL_ACT_NONE || L.d.res_slot >= 0 || L.d.up_slot >= 0)
      return false;
    any = true;
  }
  return any;
}

// Launchers that exist once per precision mode, indexed by opt_bf16: 0 fp32, 1 bf16-MFMA, 2 fp16-MFMA, 3 fp16 storage.
// There is no bf16 / fp16-MFMA stem or depthwise launcher: those modes keep fp32 tensors and use the fp32 one.
struct ModeLaunchers {
  hipError_t (*conv)(const YlConvP&, int, hipStream_t);
  hipError_t (*conv_multi)(const YlConvP*, int, int, hipStream_t);
  hipError_t (*stem)(const YlConvP&, hipStream_t), (*dw)(const YlConvP&, hipStream_t);
  hipError_t (*stemblock)(const YlConvP&, hipStream_t), (*stemdw)(const YlConvP&, hipStream_t);
  hipError_t (*conv_init)(), (*convc_init)(), (*stemblock_init)();      // dynamic-LDS limits of the mode's kernels (yl_create)
};
// S: the mode's symbol suffix; SD: the suffix of its stem / depthwise launchers
#define YL_MODE_LAUNCHERS(S, SD)                                                                             \
  {yl_launch_conv##S, yl_launch_conv_multi##S, yl_launch_stem##SD, yl_launch_dw##SD, yl_launch_stemblock##S, \
   yl_launch_stemdw##S, yl_conv_init##S, yl_convc_init##S, yl_stemblock_init##S}
const ModeLaunchers kLaunch[4] = {YL_MODE_LAUNCHERS(, ), YL_MODE_LAUNCHERS(_bf16, ), YL_MODE_LAUNCHERS(_f16, ),
                                  YL_MODE_LAUNCHERS(_f16s, _f16s)};

yl_status launch_failed(yl_ctx* c, const LaunchStep& s, hipError_t e) {
  static const char* const what[] = {"", "batched ", "head ", "expand-only ", "fused ", "chained ", "split head "};   // by LaunchForm
  char b[256];
  snprintf(b, sizeof(b), "layers %zu..%zu %slaunch failed: %s", s.first, s.first + s.layers - 1, what[s.form], hipGetErrorString(e));
  return fail(c, YL_ERR_HIP, b);
}

// One run_layers call: what it was asked for and what it carries from launch to launch.
struct LayerRun {
  yl_ctx* c;
  const float* x; int b0, B; float* const* level_out;
  hipStream_t st; hipEvent_t* evs; int chunk; const yl_post_cfg* fuse; size_t lend;
  bool lanes = false;                        // two lanes (see yl_ctx::lane): lane-1 layers go to the chunk's side stream `sd`
  hipStream_t sd = nullptr;
  std::vector<unsigned char> prod;           // lane that produced each slot
  bool side_used = false;
  int pooled_slot = -1, pooled_P = 0;        // slot whose partial channel sums the last depthwise launch left

  // where the launch that computes head-output layer i decodes to (fuse != nullptr)
  void decode_targets(size_t i, YlConvP& p) const {
    const int l = c->m->layers[i].d.head_level, S = c->m->level_S[l];
    const size_t o = (size_t)b0 * c->m->N;
    p.dec_boxes = c->ws_boxes + o; p.dec_scores = c->ws_scores + o; p.dec_cls = c->ws_cls + o;
    p.dec_N = c->m->N; p.dec_off = c->m->level_off[l] + c->m->layers[i].head_anchor * S * S; p.dec_C = c->m->C;
    p.dec_mode = fuse->mode; p.dec_center = fuse->center_mode; p.dec_wh = fuse->wh_mode;
    p.dec_raw = c->m->NM > 0 ? 1 : 0;                          // mask coefficients are read from the raw rows
    p.dec_stride = (float)((double)c->m->img_size / (double)S);   // utils_ms.py:71, as fill_levels
    p.dec_hi = (float)(c->m->img_size - 1);
    p.dec_conf = fuse->conf_thr;
    p.dec_skip_cnt = c->opt_head_skip_count ? c->head_skip_cnt : nullptr;
  }
  void params(size_t i, YlConvP& p) const {
    layer_params(c, c->m->layers[i], b0, B, x, level_out, p);
    if (fuse && c->m->layers[i].d.head_level >= 0) decode_targets(i, p);
  }
};

// F_LAYER: layer i by its own launcher (+ the activation pass behind it), on its lane's stream
yl_status run_layer(LayerRun& r, size_t i) {
  yl_ctx* c = r.c;
  const DevLayer& L = c->m->layers[i];
  const yl_layer& d = L.d;
  const int b0 = r.b0, B = r.B;
  const ModeLaunchers& ml = kLaunch[c->opt_bf16];
  YlConvP p;
  r.params(i, p);
  const int ln = (r.lanes && c->m->lane[i]) ? 1 : 0;
  hipStream_t ls = ln ? r.sd : r.st;
  if (r.lanes) {
    // an event edge wherever a layer reads a slot produced on the other lane
    bool cross = false;
    const int ins[4] = {d.in_slot, d.res_slot, d.up_slot, d.scale_slot};
    for (int k = 0; k < 4; ++k)
      if (ins[k] >= 0 && d.op != YL_OP_STEM && d.op != YL_OP_STEMBLOCK && d.op != YL_OP_NHWC4 && r.prod[ins[k]] != ln) cross = true;
    if (ln == 1 && !r.side_used) cross = true;             // first side launch: order after everything enqueued so far
    if (cross) {
      hipEvent_t ev = ln ? c->ev_la[r.chunk] : c->ev_lb[r.chunk];
      HIPCHK(c, hipEventRecord(ev, ln ? r.st : r.sd));
      HIPCHK(c, hipStreamWaitEvent(ls, ev, 0));
    }
    if (ln) r.side_used = true;
    if (d.head_level < 0 && d.out_slot >= 0) r.prod[d.out_slot] = (unsigned char)ln;
  }
  hipError_t e;
  switch (d.op) {
    case YL_OP_SE: {
      YlSeP sp;
      sp.x = p.x; sp.gate = p.out;
      sp.w1 = L.wp; sp.b1 = L.bias; sp.w2 = L.w2p; sp.b2 = L.b2;
      sp.B = B; sp.HW = L.in_h * L.in_w; sp.C = d.cin; sp.RD = d.cout; sp.act = d.act;
      const bool pooled = r.pooled_slot == d.in_slot;      // the depthwise launch in front left the partial sums
      sp.P = pooled ? r.pooled_P : yl_se_parts(sp.HW, sp.C);
      sp.partial = se_partial(c, b0);
      if (c->opt_bf16 == 3 && !pooled) return fail(c, YL_ERR_UNSUPPORTED, "store_f16: squeeze-excite pooling needs the pooled depthwise launch in front of it");
      e = yl_launch_se(sp, pooled, ls);
      break;
    }
    case YL_OP_DW: {
      // feeding a squeeze-excite gate next (efficientnetv2 MBConv): pool in the same launch
      r.pooled_slot = -1;
      if (i + 1 < r.lend && c->m->layers[i + 1].d.op == YL_OP_SE && c->m->layers[i + 1].d.in_slot == d.out_slot && d.res_slot < 0 &&
          (!c->opt_bf16 || c->opt_bf16 == 3) && !(c->opt_dev & YL_DEV_DW_TILE_OFF)) {
        const int wpi = yl_dw_pool_wpi(d.k, d.stride, d.cin, d.cout, L.out_h, L.out_w);
        if (wpi > 0 && c->m->se_unit >= (size_t)wpi * d.cin) {
          p.pool = se_partial(c, b0);
          p.pool_wpi = wpi;
          r.pooled_slot = d.out_slot; r.pooled_P = wpi;
        }
      }
      e = ml.dw(p, ls);
      break;
    }
    case YL_OP_POOL: case YL_OP_COPY: case YL_OP_LN: case YL_OP_GRN: case YL_OP_NHWC4: {
      if (c->opt_bf16 == 3) return fail(c, YL_ERR_UNSUPPORTED, "store_f16: the element-wise ops of the hgnetv2 / convnextv2 backbones are fp32-storage only");
      YlOpP q;
      memset(&q, 0, sizeof(q));
      q.x = p.x; q.out = p.out; q.w = L.wp; q.b = L.bias;
      q.B = B; q.H = L.in_h; q.W = L.in_w; q.C = d.cin;
      q.OH = d.op == YL_OP_GRN ? L.in_h : L.out_h; q.OW = d.op == YL_OP_GRN ? L.in_w : L.out_w;
      q.k = d.k; q.stride = d.stride; q.pad_t = d.pad_t; q.pad_l = d.pad_l;
      q.ldo = d.op == YL_OP_COPY ? c->slots[d.out_slot].c : d.cin; q.ch_off = d.out_ch_off;
      q.eps = d.eps;
      if (d.op == YL_OP_GRN) {
        q.P = yl_grn_parts(L.in_h * L.in_w);
        q.partial = se_partial(c, b0);
      }
      e = yl_launch_op(d.op, q, ls);
      break;
    }
    case YL_OP_STEM: e = ml.stem(p, ls); break;
    case YL_OP_CONV:
      // small-channel dense 3x3 on large grids: window-in-LDS kernel (fp32 units only; "tile_m" 6 keeps the generic kernel)
      e = (!c->opt_bf16 && c->opt_tile_m != 6) ? yl_launch_conv_k3w(p, ls) : hipErrorNotSupported;
      if (e == hipErrorNotSupported) e = ml.conv(p, c->opt_tile_m, ls);
      break;
    case YL_OP_STEMBLOCK: e = d.dw_k == 3 ? ml.stemdw(p, ls) : ml.stemblock(p, ls); break;
    default: e = ml.dw(p, ls); break;
  }
  if (e == hipSuccess && YL_ACT_POSTPASS(d.act) && c->opt_bf16 == 3) return fail(c, YL_ERR_UNSUPPORTED, "store_f16: GELU / ReLU + affine passes are fp32-storage only");
  if (e == hipSuccess && YL_ACT_POSTPASS(d.act)) {
    // GELU / ReLU + learnable affine (+ the residual behind it): element-wise pass over the layer's output, in place
    YlOpP q;
    memset(&q, 0, sizeof(q));
    q.x = p.out; q.out = p.out;
    q.B = B; q.OH = L.out_h; q.OW = L.out_w; q.C = d.cout;
    q.act = d.act; q.lab_s = d.lab_scale; q.lab_b = d.lab_bias;
    if (d.res_slot >= 0) q.res = slot_addr(c, d.res_slot, b0);
    e = yl_launch_op(YL_OP_ACTPASS, q, ls);
  }
  if (e != hipSuccess) return launch_failed(c, {F_LAYER, i, 1, 1}, e);
  if (r.evs) HIPCHK(c, hipEventRecord(r.evs[i + 1], r.st));
  return YL_OK;
}

// Sends out one step.  *refused: the form's launcher answered hipErrorNotSupported and nothing was enqueued -- the fused
// forms only (their 32-bit byte-offset guards depend on the batch); from any other form that answer is an error
yl_status emit(LayerRun& r, const LaunchStep& s, bool* refused) {
  yl_ctx* c = r.c;
  const size_t i = s.first, n = (size_t)s.width;
  hipError_t e = hipSuccess;
  YlConvP ps[4];
  switch (s.form) {
    case F_LAYER: return run_layer(r, i);
    case F_HEAD_RUN:                          // trunks [i, i + n), their head-output convs [i + n, i + 2n)
      for (size_t q = 0; q < n; ++q) {
        const DevLayer& O = c->m->layers[i + n + q];            // the head-output conv: weights, bias, decode targets
        r.params(i + q, ps[q]);
        ps[q].w3p = O.wp; ps[q].b3 = O.bias; ps[q].C3 = O.d.cout;
        r.decode_targets(i + n + q, ps[q]);
      }
      {
        bool skip_form = false;
        e = yl_launch_conv_dpp(ps, (int)n, r.st, &skip_form);
        if (e == hipSuccess && skip_form) ++c->head_skip_launches;
      }
      break;
    case F_DPQ_EXPAND:
      r.params(i, ps[0]);
      ps[0].w3p = nullptr;
      e = yl_launch_conv_dpq(ps[0], r.st);
      break;
    case F_DPQ_PAIR: case F_DWX_CHAIN: {
      YlConvP& pt = ps[0]; YlConvP& po = ps[1];
      r.params(i, pt);
      r.params(i + 1, po);
      pt.w3p = po.wp; pt.b3 = po.bias; pt.C3 = po.N; pt.act3 = po.act;
      if (s.form == F_DPQ_PAIR) { pt.res = po.res; pt.out = po.out; }    // the expanded tensor is not written
      e = s.form == F_DPQ_PAIR ? yl_launch_conv_dpq(pt, r.st) : yl_launch_conv_dwx(pt, po.out, r.st);
      if (s.form == F_DWX_CHAIN && e == hipSuccess) ++c->chain_launches;
      break;
    }
    case F_PW_PAIR: {
      YlConvP& pt = ps[0]; YlConvP& po = ps[1];
      r.params(i, pt);
      r.params(i + 1, po);
      pt.w3p = po.wp; pt.b3 = po.bias; pt.C3 = po.N; pt.act3 = po.act;
      e = yl_launch_conv_pwx(pt, po.out, r.st);                          // the tensor between the two is not written
      if (e == hipSuccess) ++c->pwx_launches;
      break;
    }
    case F_SPLIT_HEAD: case F_BATCHED:
      for (size_t q = 0; q < n; ++q) {
        r.params(i + q, ps[q]);
        if (s.form == F_BATCHED) continue;
        // head-output conv of a model with mask coefficients under yl_predict: det rows through the decode epilogue (no raw
        // rows); the coefficient part rides along as the second weight image (yl_launch_conv_multi: one pass where it pays,
        // else a second plain 1x1 launch) and its columns go into the level rows behind the detection columns
        // (bit-identical values: same k order)
        const DevLayer& L = c->m->layers[i + q];
        YlConvP& a = ps[q];
        const int nd = 5 + c->m->C;
        a.wp = L.wp_det; a.bias = L.b_det; a.N = nd; a.NTtot = cdiv(nd, 16); a.dec_raw = 0;
        a.w3p = L.wp_mc; a.b3 = L.b_mc; a.C3 = c->m->NM;
        a.out += nd; a.ldo = c->m->E;
      }
      e = kLaunch[c->opt_bf16].conv_multi(ps, (int)n, c->opt_tile_m, r.st);
      break;
  }
  const unsigned fused = form_bit(F_HEAD_RUN) | form_bit(F_DPQ_EXPAND) | form_bit(F_DPQ_PAIR) | form_bit(F_DWX_CHAIN) | form_bit(F_PW_PAIR);
  *refused = e == hipErrorNotSupported && (fused & form_bit(s.form));
  if (e != hipSuccess && !*refused) return launch_failed(c, s, e);
  return YL_OK;
}

yl_status run_layers(yl_ctx* c, const float* x, int b0, int B, float* const* level_out, hipStream_t st,
                     hipEvent_t* evs /*nullable: num_layers+1 events*/, int chunk = 0,
                     const yl_post_cfg* fuse = nullptr /*non-null: head outputs decode in their epilogue*/,
                     int lo = 0, int hi = -1 /*layer range [lo, hi), -1 = to the end*/) {
  if (evs) HIPCHK(c, hipEventRecord(evs[0], st));
  LayerRun r{c, x, b0, B, level_out, st, evs, chunk, fuse, hi < 0 ? c->m->layers.size() : (size_t)hi};
  // side lanes: an event edge is inserted wherever a layer reads a slot produced on the other lane (run_layer), and the
  // side stream is joined at the end.  Per-layer timing (evs) keeps everything on one stream.
  r.lanes = !evs && c->opt_lanes && !c->m->lane.empty() && chunk >= 0 && chunk < 4;
  if (r.lanes) {
    if (!c->side[chunk]) HIPCHK(c, hipStreamCreateWithFlags(&c->side[chunk], hipStreamNonBlocking));
    if (!c->ev_la[chunk]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_la[chunk], hipEventDisableTiming));
    if (!c->ev_lb[chunk]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_lb[chunk], hipEventDisableTiming));
    r.sd = c->side[chunk];
  }
  r.prod.assign(c->slots.size(), 0);
  const unsigned allowed = allowed_forms(c, evs != nullptr || r.lanes, fuse != nullptr);
  for (size_t i = (size_t)lo; i < r.lend;) {
    LaunchStep step;
    for (unsigned forms = allowed;; forms &= ~form_bit(step.form)) {      // a refused form: ask again without it
      step = next_step(c, i, r.lend, forms);
      bool refused = false;
      const yl_status s = emit(r, step, &refused);
      if (s != YL_OK) return s;
      if (!refused) break;
    }
    i += (size_t)step.layers;
  }
  if (r.side_used) {                                          // join: decode / the caller see both lanes
    HIPCHK(c, hipEventRecord(c->ev_lb[chunk], r.sd));
    HIPCHK(c, hipStreamWaitEvent(st, c->ev_lb[chunk], 0));
  }
  return YL_OK;
}

yl_status check_cfg(yl_ctx* c, const yl_post_cfg* cfg) {
  if (!cfg) return fail(c, YL_ERR_INVALID, "cfg is NULL");
  if (cfg->mode < YL_POST_MAIN || cfg->mode > YL_POST_EVAL) return fail(c, YL_ERR_INVALID, "bad post mode");
  if (cfg->max_out <= 0) return fail(c, YL_ERR_INVALID, "max_out must be > 0");
  if (cfg->center_mode < 0 || cfg->center_mode > 1 || cfg->wh_mode < 0 || cfg->wh_mode > 2)
    return fail(c, YL_ERR_INVALID, "bad center/wh mode");
  if (cfg->fallback_nms != YL_NMS_TORCHVISION && cfg->fallback_nms != YL_NMS_GREEDY)
    return fail(c, YL_ERR_INVALID, "bad fallback_nms");
  return YL_OK;
}

// post-processing of images [b0, b0+B) of a batch (workspaces must already cover b0+B images)
yl_status do_post(yl_ctx* c, const float* const* levels_all, int b0, int B, const yl_post_cfg* cfg, float* dets,
                  int* counts, int* keep_idx, hipStream_t st, bool decoded = false /*NMS inputs already written*/) {
  const float* levels[YL_MAX_LEVELS];
  for (int l = 0; l < c->m->L; ++l)
    levels[l] = levels_all[l] + (size_t)b0 * c->m->level_A[l] * c->m->level_S[l] * c->m->level_S[l] * c->m->E;
  const size_t o = (size_t)b0 * c->m->N;
  YlLevels lv;
  fill_levels(c, levels, lv);
  YlDecodeP dp;
  dp.mode = cfg->mode; dp.center_mode = cfg->center_mode; dp.wh_mode = cfg->wh_mode;
  dp.boxes = c->ws_boxes + o; dp.scores = c->ws_scores + o; dp.cls = c->ws_cls + o;
  if (!decoded) HIPCHK(c, yl_launch_decode_score(lv, B, dp, st));
  YlNmsP np;
  memset(&np, 0, sizeof(np));
  np.boxes = c->ws_boxes + o; np.scores = c->ws_scores + o; np.cls = c->ws_cls + o;
  np.N = c->m->N; np.C = c->m->C > 0 ? c->m->C : 1;
  np.conf_thr = cfg->conf_thr; np.iou_thr = cfg->iou_thr;
  np.impl = (cfg->mode == YL_POST_FALLBACK && cfg->fallback_nms == YL_NMS_GREEDY) ? YL_NMS_GREEDY : YL_NMS_TORCHVISION;
  np.cap = (cfg->per_class_cap > 0) ? cfg->per_class_cap : INT_MAX;
  np.topk = (cfg->mode == YL_POST_FALLBACK && cfg->topk > 0) ? cfg->topk : 0;
  np.max_out = cfg->max_out;
  np.cls_ws = c->ws_clsws + (size_t)b0 * 4 * np.C;
  np.gkeys = c->ws_gkeys ? c->ws_gkeys + (size_t)b0 * c->gP : nullptr; np.gP = c->gP;
  np.lds_cap = c->gP < YL_LDS_KEYS_MAX ? c->gP : YL_LDS_KEYS_MAX;
  np.dets = dets + (size_t)b0 * cfg->max_out * 6; np.counts = counts + b0;
  np.keep_idx = keep_idx ? keep_idx + (size_t)b0 * cfg->max_out : nullptr;
  np.backmap = cfg->backmap_dev ? cfg->backmap_dev + (size_t)b0 * 5 : nullptr;
  np.tmp_dets = c->ws_tmp_dets + o * 6; np.tmp_idx = c->ws_tmp_idx + o;
  // several workgroups per image (classes split mod G) unless the fallback's global top-k needs the whole kept
  // set in one workgroup, or survivors could exceed the LDS key capacity
  // auto: the class-group split (histogram + assignment prologue, merge kernel) pays when an image has thousands of
  // survivors -- evaluation thresholds (conf 0.001: +2.7 % on a 2000-survivor workload) -- and costs 0.8 % at the
  // few hundred survivors of a detector operating point (conf 0.4, calibrated benchmark workload)
  const int groups = c->opt_nms_groups > 0 ? c->opt_nms_groups : (cfg->conf_thr < 0.05f ? YL_NMS_GROUPS : 1);
  np.G = (groups > 1 && np.topk == 0 && c->m->C > 1 && c->m->C <= 256 && c->m->N <= YL_LDS_KEYS_MAX) ? groups : 1;
  np.kept_list = c->ws_kept_list + o * YL_NMS_GROUPS;
  np.done = c->ws_done + (size_t)b0 * 64;                              // 256 bytes per image
  HIPCHK(c, yl_launch_nms(np, B, st));
  return YL_OK;
}

struct Job {
  const float* x = nullptr;          // nullptr: no forward (post-processing of caller levels only)
  int B = 0;
  float* outs[YL_MAX_LEVELS] = {nullptr};
  const yl_post_cfg* cfg = nullptr;  // nullptr: forward only
  float* dets = nullptr;
  int* counts = nullptr;
  int* keep_idx = nullptr;
};

// A job runs as a sequence of SEGMENTS: layer range [lo, hi), either as one full-batch piece on the caller's
// stream or as one piece per batch chunk on the internal streams (fork/join); the last segment carries the
// post-processing.  Plans:
//   plain    [0, L) chunked, post per chunk                      (1 segment; n == 1: a single piece)
//   hybrid   [0, lo) full | [lo, hi) chunked | [hi, L) full + post
// hybrid: the high-resolution layers (stem block, 160^2 / 80^2 stages, the 80^2 neck / heads) fill the machine on
// their own -- their grids are persistent and occupancy-sized, so a half-batch launch of another chunk cannot
// overlap them, it only queues behind them -- while the run of <= 1/16-resolution layers is latency-bound with a
// few hundred tiles: those runs of the two chunks interleave on two streams.
struct Seg { int lo, hi; bool chunked, post; };

int plan_segments(const yl_ctx* c, const Job& j, int n, Seg* segs) {
  const int L = (int)c->m->layers.size();
  if (!j.x) { segs[0] = {0, 0, n > 1, true}; return 1; }
  if (c->opt_time_split && j.cfg) {          // one chunk (chunks_for): conv layers | post-processing, an event between them
    segs[0] = {0, L, false, false};
    segs[1] = {L, L, false, true};
    return 2;
  }
  if (n > 1 && c->opt_hybrid == 2 && !c->opt_lanes && c->m->tiny_hi - c->m->tiny_lo >= 6) {
    int k = 0;
    if (c->m->tiny_lo > 0) segs[k++] = {0, c->m->tiny_lo, true, false};
    segs[k++] = {c->m->tiny_lo, c->m->tiny_hi, false, false};
    segs[k++] = {c->m->tiny_hi, L, true, j.cfg != nullptr};
    return k;
  }
  if (n > 1 && c->opt_hybrid == 1 && !c->opt_lanes && c->m->small_hi - c->m->small_lo >= 6) {
    int k = 0;
    if (c->m->small_lo > 0) segs[k++] = {0, c->m->small_lo, false, false};
    segs[k++] = {c->m->small_lo, c->m->small_hi, true, false};
    segs[k++] = {c->m->small_hi, L, false, j.cfg != nullptr};
    return k;
  }
  segs[0] = {0, L, n > 1, j.cfg != nullptr};
  return 1;
}

// one piece: layers [lo, hi) of images [b0, b0 + bn), then (last segment) post-processing of those images
yl_status run_piece(yl_ctx* c, const Job& j, const Seg& sg, int b0, int bn, hipStream_t st, int chunk) {
  yl_status s = YL_OK;
  const bool fused = j.x && j.cfg && can_fuse_decode(c);
  // ("time_split": the events are recorded by walk_plan AROUND the pieces -- conv layers | post-processing -- so that a
  // piece can also be a replayed hipGraph)
  if (j.x && sg.hi > sg.lo) s = run_layers(c, j.x, b0, bn, j.outs, st, nullptr, chunk, fused ? j.cfg : nullptr, sg.lo, sg.hi);
  if (s == YL_OK && sg.post && j.cfg) s = do_post(c, j.outs, b0, bn, j.cfg, j.dets, j.counts, j.keep_idx, st, fused);
  return s;
}

// ---- stream / hardware-queue aliasing probe (yl_streams_overlap, include/yololite_hip.h)
__global__ void yl_spin_kernel(long long ticks) {
  const long long t0 = wall_clock64();                       // 100 MHz constant clock
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

// 1 = kernel CHAINS on a and b overlap, 0 = they serialise, -1 = HIP error.  Two rounds, the better one counts (a busy device
// can only make a pair look serialised).  Measured (round 6): a good pair finishes two chains of 8 x 25 us in ~231 us, an aliasing
// pair in ~465 us; with ONE 200 us kernel per stream both kinds finish in ~224 us -- lone kernels do not show the aliasing.
int streams_overlap(hipStream_t a, hipStream_t b) {
  const long long ticks = 20000;                             // 200 us
  if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return -1;
  hipLaunchKernelGGL(yl_spin_kernel, dim3(1), dim3(64), 0, a, 100LL);   // code object load / first-launch cost off the clock
  hipLaunchKernelGGL(yl_spin_kernel, dim3(1), dim3(64), 0, b, 100LL);
  if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return -1;
  // CHAINS of dependent kernels, not one kernel per stream: two lone kernels overlap on any pair of streams; what a serving
  // loop needs is that the command processor keeps dispatching stream b's chain while stream a's next kernel waits for its
  // predecessor (two streams whose hardware queues share a pipe fail exactly there)
  const int links = 8;
  double best = 1e30;
  for (int r = 0; r < 2; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < links; ++i) {
      hipLaunchKernelGGL(yl_spin_kernel, dim3(1), dim3(64), 0, a, ticks / links);
      hipLaunchKernelGGL(yl_spin_kernel, dim3(1), dim3(64), 0, b, ticks / links);
    }
    if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return -1;
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (us < best) best = us;
  }
  return best < 1.5 * 200.0 ? 1 : 0;
}

// a new non-blocking stream whose kernels overlap those of every stream in `others` (up to 12 candidates: the hardware-queue
// assignment walks round-robin with the streams created; the rejected ones are destroyed afterwards -- destroying one right
// away would hand the same queue to the next candidate's successor).  Falls back to the last candidate.
yl_status make_overlapping_stream(yl_ctx* c, const hipStream_t* others, int n, hipStream_t* out) {
  std::vector<hipStream_t> rejected;
  hipStream_t s = nullptr;
  for (int attempt = 0; attempt < 12; ++attempt) {
    HIPCHK(c, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    bool ok = true;
    for (int i = 0; i < n && ok; ++i) ok = streams_overlap(others[i], s) != 0;
    if (ok || attempt == 11) break;
    rejected.push_back(s);
    s = nullptr;
  }
  for (hipStream_t r : rejected) hipStreamDestroy(r);
  *out = s;
  return YL_OK;
}

// Only the streams this job needs (round 6): n - 1 chunk streams, side streams only under the "lanes" option.  A context
// used to create all seven at its first call; ROCm hands streams to the GPU_MAX_HW_QUEUES hardware queues as they appear,
// and with two cloned contexts per serving pipeline (14 idle streams) the two LANE streams of the pipeline ended up
// sharing a queue: 38.6 k instead of 44.9 k images/s (edge_n B=64, two batches in flight).  A one-stream context now
// creates no stream at all.
yl_status ensure_streams(yl_ctx* c, int n, hipStream_t st) {
  for (int i = 0; i < 4 && i < n; ++i) {
    if (i > 0 && !c->work[i]) {
      // chunk stream i must run beside the caller's stream (chunk 0) and beside its siblings: probe, do not assume
      hipStream_t others[4] = {st, nullptr, nullptr, nullptr};
      int no = 1;
      for (int k = 1; k < i; ++k) others[no++] = c->work[k];
      hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        HIPCHK(c, hipStreamCreateWithFlags(&c->work[i], hipStreamNonBlocking));   // caller is capturing: no probe possible
      } else {
        yl_status ms = make_overlapping_stream(c, others, no, &c->work[i]);
        if (ms != YL_OK) return ms;
      }
    }
    if (i > 0 && !c->ev_join[i]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming));
    if (!c->opt_lanes) continue;
    if (!c->side[i]) HIPCHK(c, hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking));
    if (!c->ev_la[i]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_la[i], hipEventDisableTiming));
    if (!c->ev_lb[i]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_lb[i], hipEventDisableTiming));
  }
  if (!c->ev_fork) HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  return YL_OK;
}

// Walk the plan.  `piece(seg, chunk, b0, bn, stream)` either enqueues the piece's kernels (eager) or launches its
// captured graph; chunked segments are forked over the internal streams and joined back on `st`.
template <typename F>
yl_status walk_plan(yl_ctx* c, const Job& j, hipStream_t st, int n, const Seg* segs, int nseg, F&& piece) {
  const int base = j.B / n, rem = j.B % n;
  const bool timed = c->opt_time_split && j.x && j.cfg && nseg == 2 && c->ev_t[0];
  for (int g = 0; g < nseg; ++g) {
    if (!segs[g].chunked || n == 1) {
      if (timed) HIPCHK(c, hipEventRecord(c->ev_t[g], st));       // before the conv layers / between them and the NMS
      yl_status s = piece(g, 0, 0, j.B, st);
      if (s != YL_OK) return s;
      if (timed && g == 1) { HIPCHK(c, hipEventRecord(c->ev_t[2], st)); c->timing_valid = true; }
      continue;
    }
    HIPCHK(c, hipEventRecord(c->ev_fork, st));
    int b0 = 0;
    for (int i = 0; i < n; ++i) {
      const int bn = base + (i < rem ? 1 : 0);
      hipStream_t ws = (i == 0) ? st : c->work[i];
      if (i > 0) HIPCHK(c, hipStreamWaitEvent(ws, c->ev_fork, 0));
      yl_status s = piece(g, i, b0, bn, ws);
      if (s != YL_OK) return s;
      if (i > 0) {
        HIPCHK(c, hipEventRecord(c->ev_join[i], ws));
        HIPCHK(c, hipStreamWaitEvent(st, c->ev_join[i], 0));
      }
      b0 += bn;
    }
  }
  return YL_OK;
}

// run a job eagerly, or by replaying cached hipGraphs of exactly this job (one graph per piece: capturing several
// chunks plus side lanes into ONE graph -- 4 streams -- crashed hipGraphInstantiate on ROCm 7.2)
yl_status submit(yl_ctx* c, const Job& j, hipStream_t st, bool allow_graph = true) {
  const int n = chunks_for(c, j.B);
  Seg segs[3];
  const int nseg = plan_segments(c, j, n, segs);
  yl_status s = ensure_streams(c, n, st);
  if (s != YL_OK) return s;
  if (!c->opt_graph || !allow_graph)
    return walk_plan(c, j, st, n, segs, nseg, [&](int g, int i, int b0, int bn, hipStream_t ws) -> yl_status {
      return run_piece(c, j, segs[g], b0, bn, ws, i);
    });
  // every option that shapes the launch list is an int field of its own (no packed bit fields: "dev_select" uses the whole
  // YL_DEV_MASK, and a flag packed beside it once made time_split 0 and 1 share a key -- the replay then indexed the exec list
  // of another segment plan)
  const int opts[] = {c->opt_streams, c->opt_lanes, c->opt_bf16, c->opt_fuse_decode, c->opt_batch_levels, c->opt_hybrid,
                      c->opt_nms_groups, c->opt_winograd, c->opt_fuse_head, c->opt_tile_m, c->opt_dev, c->opt_time_split,
                      c->opt_split_k};
  std::vector<unsigned char> key(sizeof(Job) + sizeof(yl_post_cfg) + sizeof(opts), 0);
  memcpy(key.data(), &j, sizeof(Job));
  if (j.cfg) memcpy(key.data() + sizeof(Job), j.cfg, sizeof(yl_post_cfg));
  memcpy(key.data() + sizeof(Job) + sizeof(yl_post_cfg), opts, sizeof(opts));
  // the cfg POINTER is part of Job but not of the identity of the work: blank it in the key
  memset(key.data() + offsetof(Job, cfg), 0, sizeof(void*));
  yl_ctx::GraphEntry* ge = nullptr;
  for (auto& g : c->graphs)
    if (g.key == key) { ge = &g; break; }
  if (!ge) {
    yl_ctx::GraphEntry fresh;
    hipStream_t cs;
    HIPCHK(c, hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    hipError_t e = hipSuccess;
    // capture every piece in plan order (walk_plan's fork/join calls are NOT issued here: pieces are independent
    // captures on the scratch stream)
    const int base = j.B / n, rem = j.B % n;
    for (int g = 0; g < nseg && s == YL_OK && e == hipSuccess; ++g) {
      const int pieces = (segs[g].chunked && n > 1) ? n : 1;
      int b0 = 0;
      for (int i = 0; i < pieces && s == YL_OK && e == hipSuccess; ++i) {
        const int bn = pieces == 1 ? j.B : base + (i < rem ? 1 : 0);
        hipGraph_t gr = nullptr;
        hipGraphExec_t ex = nullptr;
        e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
        if (e != hipSuccess) break;
        s = run_piece(c, j, segs[g], b0, bn, cs, i);
        e = hipStreamEndCapture(cs, &gr);
        if (s == YL_OK && e == hipSuccess) e = hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0);
        if (gr) hipGraphDestroy(gr);
        fresh.execs.push_back(ex);
        b0 += bn;
      }
    }
    hipStreamDestroy(cs);
    if (s != YL_OK || e != hipSuccess) {
      for (auto ex : fresh.execs)
        if (ex) hipGraphExecDestroy(ex);
      if (s != YL_OK) return s;
      HIPCHK(c, e);
    }
    fresh.key = key;
    fresh.n = n;
    if (c->graphs.size() >= YL_GRAPH_SLOTS) {                 // evict the least recently used entry
      size_t v = 0;
      for (size_t i = 1; i < c->graphs.size(); ++i)
        if (c->graphs[i].stamp < c->graphs[v].stamp) v = i;
      for (auto ex : c->graphs[v].execs)
        if (ex) hipGraphExecDestroy(ex);
      c->graphs.erase(c->graphs.begin() + v);
    }
    c->graphs.push_back(fresh);
    ge = &c->graphs.back();
  }
  ge->stamp = ++c->graph_clock;
  size_t at = 0;
  std::vector<size_t> first(nseg);
  for (int g = 0; g < nseg; ++g) { first[g] = at; at += (segs[g].chunked && n > 1) ? n : 1; }
  return walk_plan(c, j, st, n, segs, nseg, [&](int g, int i, int, int, hipStream_t ws) -> yl_status {
    HIPCHK(c, hipGraphLaunch(ge->execs[first[g] + i], ws));
    return YL_OK;
  });
}

}  // namespace

// ================================================================================================
extern "C" {

int32_t yl_abi_version(void) { return YL_ABI_VERSION; }

const char* yl_strerror(yl_status s) {
  switch (s) {
    case YL_OK: return "ok";
    case YL_ERR_INVALID: return "invalid argument";
    case YL_ERR_HIP: return "HIP runtime error";
    case YL_ERR_NOMEM: return "out of memory";
    case YL_ERR_STATE: return "invalid state for this call";
    case YL_ERR_UNSUPPORTED: return "unsupported configuration";
    case YL_ERR_CAPACITY: return "output buffer too small";
    default: return "unknown yl_status";
  }
}

const char* yl_last_error(const yl_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

void yl_destroy(yl_ctx* c) {
  if (!c) return;
  hipSetDevice(c->m->device);
  free_act(c);
  free_post_ws(c);
  hipFree(c->ws_nms_clsws);
  hipFree(c->head_skip_cnt);
  hipFree(c->ws_loss_keys); hipFree(c->ws_loss_neg); hipFree(c->ws_loss_pi); hipFree(c->ws_loss_pos);
  for (int i = 0; i < 4; ++i) {
    if (c->work[i]) hipStreamDestroy(c->work[i]);
    if (c->ev_join[i]) hipEventDestroy(c->ev_join[i]);
    if (c->side[i]) hipStreamDestroy(c->side[i]);
    if (c->ev_la[i]) hipEventDestroy(c->ev_la[i]);
    if (c->ev_lb[i]) hipEventDestroy(c->ev_lb[i]);
  }
  if (c->ev_fork) hipEventDestroy(c->ev_fork);
  for (int i = 0; i < 3; ++i) if (c->ev_t[i]) hipEventDestroy(c->ev_t[i]);
  hipFree(c->ws_nms_gkeys);
  delete c;   // (the model and its device images go with the last context that shares them)
}

yl_status yl_clone(const yl_ctx* src, yl_ctx** out) {
  if (!src || !out) return YL_ERR_INVALID;
  *out = nullptr;
  if (hipSetDevice(src->m->device) != hipSuccess) return YL_ERR_HIP;
  yl_ctx* c = new (std::nothrow) yl_ctx();
  if (!c) return YL_ERR_NOMEM;
  *out = c;
  c->m = src->m;                           // the model, shared and immutable
  init_slots(c);
  // the options as they are now; activation arenas, workspaces, streams, events and cached graphs are the clone's own
  c->opt_reuse = src->opt_reuse; c->opt_pre_norm = src->opt_pre_norm; c->opt_graph = src->opt_graph; c->opt_tile_m = src->opt_tile_m;
  c->opt_streams = src->opt_streams; c->opt_nms_groups = src->opt_nms_groups; c->opt_hybrid = src->opt_hybrid;
  c->opt_batch_levels = src->opt_batch_levels; c->opt_winograd = src->opt_winograd; c->opt_fuse_decode = src->opt_fuse_decode;
  c->opt_fuse_head = src->opt_fuse_head; c->opt_split_k = src->opt_split_k; c->opt_dev = src->opt_dev; c->opt_bf16 = src->opt_bf16;
  c->opt_lanes = src->opt_lanes;
  return YL_OK;
}

yl_status yl_streams_overlap(int32_t device_id, void* a, void* b, int32_t* overlap) {
  if (!overlap) return YL_ERR_INVALID;
  *overlap = 0;
  if (hipSetDevice(device_id) != hipSuccess) return YL_ERR_HIP;
  const int r = streams_overlap((hipStream_t)a, (hipStream_t)b);
  if (r < 0) return YL_ERR_HIP;
  *overlap = r;
  return YL_OK;
}

// validate (host only, yl_program.cpp) -> touch the device -> pack and upload layer by layer
yl_status yl_create(const yl_model_desc* d, int32_t device_id, yl_ctx** out) {
  if (!d || !out) return YL_ERR_INVALID;
  *out = nullptr;
  yl_status s = yl_program_check_args(d);
  if (s != YL_OK) return s;
  YlProgram prog;
  std::string msg;
  s = yl_program_validate(d, &prog, &msg);
  if (s != YL_OK) {
    // handed out so that yl_last_error() can be read; caller destroys it.  No device has been touched: its model is empty
    yl_ctx* c = new (std::nothrow) yl_ctx();
    if (!c) return YL_ERR_NOMEM;
    *out = c;
    c->m = std::make_shared<Model>();
    return fail(c, s, msg);
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return YL_ERR_HIP;
  if (hipSetDevice(device_id) != hipSuccess) return YL_ERR_HIP;
  if (device_id >= 64) return YL_ERR_UNSUPPORTED;
  if (!g_inited[device_id]) {
    for (const ModeLaunchers& ml : kLaunch)
      if (ml.conv_init() != hipSuccess || ml.convc_init() != hipSuccess || ml.stemblock_init() != hipSuccess) return YL_ERR_HIP;
    if (yl_post_init() != hipSuccess || yl_dpp_init() != hipSuccess) return YL_ERR_HIP;     // (fp32-only units)
    g_inited[device_id] = true;
  }
  yl_ctx* c = new (std::nothrow) yl_ctx();
  if (!c) return YL_ERR_NOMEM;
  *out = c;   // handed out even on failure so that yl_last_error() can be read; caller destroys it
  // the context owns the model from before its first upload: whatever fails below, destroying the context frees every image
  const std::shared_ptr<Model> m = std::make_shared<Model>();
  c->m = m;
  m->device = device_id;
  static_cast<YlGeometry&>(*m) = prog;
  static_cast<YlTables&>(*m) = yl_program_tables(prog);
  init_slots(c);
  if (prog.layers.empty()) return YL_OK;
  HIPCHK(c, hipMalloc((void**)&m->zeros, 1024));
  HIPCHK(c, hipMemset(m->zeros, 0, 1024));
  m->layers.reserve(prog.layers.size());
  YlLayerImages im;
  for (size_t i = 0; i < prog.layers.size(); ++i) {
    yl_program_pack(prog, i, &im);
    m->layers.emplace_back();
    DevLayer& L = m->layers.back();
    static_cast<YlLayerInfo&>(L) = prog.layers[i];
    L.d.w = L.d.b = L.d.dw_w = L.d.dw_b = nullptr;      // the caller's arrays need not outlive this call
    L.d.w2 = L.d.b2 = L.d.w3 = L.d.b3 = nullptr;
#define YL_X(name) if ((s = upload(c, im.name, &L.name)) != YL_OK) return s;
    YL_LAYER_IMAGES(YL_X)
#undef YL_X
  }
  return YL_OK;
}

yl_status yl_set_option(yl_ctx* c, const char* name, int32_t value) {
  if (!c || !name) return YL_ERR_INVALID;
  if (!strcmp(name, "graph")) { c->opt_graph = value ? 1 : 0; drop_graph(c); return YL_OK; }
  if (!strcmp(name, "mfma_bf16")) { if (c->opt_bf16 == 3) free_act(c); c->opt_bf16 = value ? 1 : (c->opt_bf16 == 1 ? 0 : c->opt_bf16); drop_graph(c); return YL_OK; }
  if (!strcmp(name, "mfma_f16")) { if (c->opt_bf16 == 3) free_act(c); c->opt_bf16 = value ? 2 : (c->opt_bf16 == 2 ? 0 : c->opt_bf16); drop_graph(c); return YL_OK; }
  if (!strcmp(name, "store_f16")) {      // fp16 operands AND fp16 activation tensors in HBM (round 6): the arenas are re-planned
    const int nv = value ? 3 : (c->opt_bf16 == 3 ? 0 : c->opt_bf16);
    if ((nv == 3) != (c->opt_bf16 == 3)) free_act(c);
    c->opt_bf16 = nv; drop_graph(c); return YL_OK;
  }
  if (!strcmp(name, "nms_groups")) { c->opt_nms_groups = value < 0 ? 0 : (value > YL_NMS_GROUPS ? YL_NMS_GROUPS : value); drop_graph(c); return YL_OK; }
  if (!strcmp(name, "time_split")) {
    // (no drop_graph: the setting is part of the graph key -- a serving loop toggles it per call, api.YoloLite.predict)
    c->opt_time_split = value ? 1 : 0;
    for (int i = 0; i < 3 && value; ++i)
      if (!c->ev_t[i]) HIPCHK(c, hipEventCreate(&c->ev_t[i]));
    c->timing_valid = false;
    return YL_OK;
  }
  if (!strcmp(name, "pre_norm")) { c->opt_pre_norm = value ? 1 : 0; return YL_OK; }
  if (!strcmp(name, "reuse_slots")) { c->opt_reuse = value ? 1 : 0; drop_graph(c); return YL_OK; }
  if (!strcmp(name, "hybrid")) { c->opt_hybrid = value < 0 ? 0 : (value > 2 ? 2 : value); drop_graph(c); return YL_OK; }
  if (!strcmp(name, "batch_levels")) { c->opt_batch_levels = value ? 1 : 0; drop_graph(c); return YL_OK; }
  if (!strcmp(name, "fuse_decode")) { c->opt_fuse_decode = value ? 1 : 0; drop_graph(c); return YL_OK; }
  if (!strcmp(name, "fuse_head")) { c->opt_fuse_head = value ? 1 : 0; drop_graph(c); return YL_OK; }
  if (!strcmp(name, "winograd")) { c->opt_winograd = value < 0 ? 0 : (value > 2 ? 2 : value); drop_graph(c); return YL_OK; }
  if (!strcmp(name, "lanes")) { c->opt_lanes = value ? 1 : 0; drop_graph(c); return YL_OK; }
  if (!strcmp(name, "tile_m")) { c->opt_tile_m = value; drop_graph(c); return YL_OK; }
  if (!strcmp(name, "streams")) { c->opt_streams = value < 1 ? 1 : (value > 4 ? 4 : value); drop_graph(c); return YL_OK; }
  if (!strcmp(name, "split_k")) { c->opt_split_k = value ? 1 : 0; drop_graph(c); return YL_OK; }
  if (!strcmp(name, "dev_select")) { c->opt_dev = value & (int)YL_DEV_MASK; drop_graph(c); return YL_OK; }
  if (!strcmp(name, "head_skip_count")) {   // (the counter pointer rides in the launch parameters: cached graphs are dropped)
    if (value && !c->head_skip_cnt) {
      HIPCHK(c, hipSetDevice(c->m->device));
      HIPCHK(c, hipMalloc((void**)&c->head_skip_cnt, sizeof(unsigned)));
      HIPCHK(c, hipMemset(c->head_skip_cnt, 0, sizeof(unsigned)));
    }
    c->opt_head_skip_count = value ? 1 : 0; drop_graph(c); return YL_OK;
  }
  return fail(c, YL_ERR_INVALID, std::string("unknown option ") + name);
}

yl_status yl_get_option(const yl_ctx* c, const char* name, int32_t* value) {
  if (!c || !name || !value) return YL_ERR_INVALID;
  const struct { const char* n; int v; } tab[] = {
      {"graph", c->opt_graph}, {"mfma_bf16", c->opt_bf16 == 1}, {"mfma_f16", c->opt_bf16 == 2}, {"store_f16", c->opt_bf16 == 3}, {"nms_groups", c->opt_nms_groups}, {"time_split", c->opt_time_split},
      {"pre_norm", c->opt_pre_norm}, {"reuse_slots", c->opt_reuse}, {"hybrid", c->opt_hybrid}, {"batch_levels", c->opt_batch_levels},
      {"fuse_decode", c->opt_fuse_decode}, {"fuse_head", c->opt_fuse_head}, {"winograd", c->opt_winograd}, {"lanes", c->opt_lanes},
      {"tile_m", c->opt_tile_m}, {"streams", c->opt_streams}, {"dev_select", c->opt_dev}, {"split_k", c->opt_split_k},
      {"chain_launches", c->chain_launches}, {"pwx_launches", c->pwx_launches}, {"head_skip_launches", c->head_skip_launches},
      {"head_skip_count", c->opt_head_skip_count}};
  for (const auto& t : tab)
    if (!strcmp(name, t.n)) { *value = t.v; return YL_OK; }
  if (!strcmp(name, "head_skipped_tiles")) {   // tiles skipped since "head_skip_count" was first set (waits for the device)
    unsigned v = 0;
    if (c->head_skip_cnt &&
        (hipSetDevice(c->m->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
         hipMemcpy(&v, c->head_skip_cnt, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess))
      return YL_ERR_HIP;
    *value = (int32_t)(v & 0x7fffffffu);
    return YL_OK;
  }
  return YL_ERR_INVALID;
}

int32_t yl_query_fused_block(int32_t c_in, int32_t c_mid, int32_t c_out, int32_t dw_k, int32_t dw_stride, int32_t out_h,
                             int32_t out_w) {
  if (c_in < 1 || c_mid < 1 || c_out < 1 || out_h < 1 || out_w < 1) return 0;
  if (yl_ir_supported(c_in, c_mid, c_out, dw_k, dw_stride, out_h, out_w)) return 1;
  // per-wave kernel: stride 1 (input grid == output grid), grids multiples of 4 (the checks of yl_create)
  if (dw_stride == 1 && !(out_h & 3) && !(out_w & 3) && yl_uib_supported(c_in, c_mid, c_out, dw_k)) return 2;
  return 0;
}

int32_t yl_query_ir_form(int32_t c_in, int32_t c_mid, int32_t c_out, int32_t dw_k, int32_t dw_stride, int32_t out_h, int32_t out_w,
                         int32_t batch, int32_t in_h, int32_t in_w, int32_t up_h, int32_t up_w, int32_t act, int32_t dw_act,
                         int32_t act2, int32_t* shape) {
  if (c_in < 1 || c_mid < 1 || c_out < 1 || out_h < 1 || out_w < 1 || batch < 1 || in_h < 1 || in_w < 1 || up_h < 0 || up_w < 0) return 0;
  return yl_ir_form(c_in, c_mid, c_out, dw_k, dw_stride, out_h, out_w, batch, in_h, in_w, up_h, up_w, act, dw_act, act2, shape);
}

int32_t yl_query_dw_prologue(int32_t c_in, int32_t c_out, int32_t dw_k, int32_t dw_stride, int32_t out_h, int32_t out_w) {
  if (c_in < 1 || c_out < 1 || dw_k < 1 || dw_stride < 1 || out_h < 1 || out_w < 1) return 0;
  if (yl_dws_supported(c_in, c_out, dw_k, dw_stride, out_h, out_w)) return 2;
  if ((size_t)(dw_k * dw_k + 1) * c_in * sizeof(float) <= YL_DW_LDS_MAX) return 1;
  return 0;
}

int32_t yl_query_wino_form(int32_t c_in, int32_t c_out, int32_t out_h, int32_t out_w, int32_t batch, int32_t in_shift,
                           int32_t dev_select, int32_t* mt, int32_t* nt) {
  if (mt) *mt = 0;
  if (nt) *nt = 0;
  // the channel conditions under which a layer carries a Winograd image (yl_program.cpp), then the launcher's own decision
  if (c_in < 16 || c_out < 16 || (c_in & 3) || (c_out & 3)) return 0;
  const unsigned dev = (unsigned)dev_select;
  const YlWinoForm f = yl_wino_form(c_in, c_out, out_h, out_w, batch, in_shift, sizeof(float), (dev & YL_DEV_WINO_V1) != 0, YL_DEV_WINO_SHAPE(dev));
  if (f.form == 2) {
    if (mt) *mt = f.mt;
    if (nt) *nt = f.nt;
  }
  return f.form;
}

int32_t yl_query_dw_form(int32_t op, int32_t c_in, int32_t c_out, int32_t dw_k, int32_t dw_stride, int32_t dw_pad_t, int32_t dw_pad_l,
                         int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w, int32_t batch, int32_t act, int32_t has_res,
                         int32_t tile_m, int32_t dev_select, int32_t split_k, int32_t* args) {
  if (args) memset(args, 0, 6 * sizeof(int32_t));
  // what yl_create refuses (yl_program.cpp: validate_layer)
  if ((op != YL_OP_CONV && op != YL_OP_DW) || c_in < 1 || c_out < 1 || dw_k < 1 || dw_stride < 1 || in_h < 1 || in_w < 1 || out_h < 1 ||
      out_w < 1 || batch < 1 || (long)batch * out_h * out_w > 0x7fffffffL || (c_in & 3) || dw_pad_t < 0 || dw_pad_l < 0 ||
      dw_pad_t >= dw_k || dw_pad_l >= dw_k || (out_h - 1) * dw_stride - dw_pad_t >= in_h || (out_w - 1) * dw_stride - dw_pad_l >= in_w ||
      act < YL_ACT_NONE || act > YL_ACT_RELU_LAB)
    return YL_DWF_NONE;
  const bool conv_res_or_smooth = op == YL_OP_CONV && (has_res || YL_SMOOTH(act));   // (validate_layer asks the layer's own fields)
  if (YL_ACT_POSTPASS(act)) { act = YL_ACT_NONE; has_res = 0; }   // applied by the activation pass: the kernel sees neither (layer_params)
  static const float some = 0.0f;   // a residual the decision sees as a pointer that is set; nothing reads through it
  YlConvP p;
  memset(&p, 0, sizeof(p));
  p.B = batch; p.H = in_h; p.W = in_w; p.Cin = c_in; p.OH = out_h; p.OW = out_w; p.N = c_out;
  p.MH = out_h; p.MW = out_w; p.act = act;
  p.KB = cdiv(c_in, 16); p.NTtot = cdiv(c_out, 16); p.M = batch * out_h * out_w;
  p.res = has_res ? &some : nullptr;
  p.dev = ((unsigned)dev_select & YL_DEV_MASK) | (split_k ? 0u : YL_DEV_DWT_NOSPLIT);   // (layer_params)
  YlDwForm f;
  if (op == YL_OP_DW) {
    if (c_out != c_in) return YL_DWF_NONE;
    p.k = dw_k; p.stride = dw_stride; p.pad_t = dw_pad_t; p.pad_l = dw_pad_l; p.TK = dw_k * dw_k * p.KB;
    f = yl_dw_alone_form(p);
  } else {
    if (conv_res_or_smooth && (c_out & 3)) return YL_DWF_NONE;
    if ((size_t)(dw_k * dw_k + 1) * c_in * sizeof(float) > YL_DW_LDS_MAX && !yl_dws_supported(c_in, c_out, dw_k, dw_stride, out_h, out_w))
      return YL_DWF_NONE;
    p.k = 1; p.stride = 1; p.TK = p.KB;
    p.dw_k = dw_k; p.dw_stride = dw_stride; p.dw_pad_t = dw_pad_t; p.dw_pad_l = dw_pad_l;
    YlConvMulti m = {};
    m.n = 1;
    m.p[0] = p;
    f = yl_dw_form(m, 0, tile_m);
  }
  if (args)
    for (int i = 0; i < 6; ++i) args[i] = f.a[i];
  return f.family;
}

static yl_status forward_impl(yl_ctx* c, const float* x, int B, float* const* level_out, hipStream_t st,
                              float* layer_ms, const yl_post_cfg* cfg, float* dets, int* counts, int* keep_idx = nullptr) {
  if (!c) return YL_ERR_INVALID;
  if (c->m->layers.empty()) return fail(c, YL_ERR_STATE, "context was created without layers");
  if (!x || B < 1) return fail(c, YL_ERR_INVALID, "bad input");
  HIPCHK(c, hipSetDevice(c->m->device));
  yl_status s = ensure_act(c, B, layer_ms ? 1 : chunks_for(c, B));
  if (s != YL_OK) return s;
  if (cfg && (s = ensure_post(c, B)) != YL_OK) return s;
  if ((s = poison_act(c, st)) != YL_OK) return s;
  Job j;
  j.x = x; j.B = B; j.cfg = cfg; j.dets = dets; j.counts = counts; j.keep_idx = keep_idx;
  for (int l = 0; l < c->m->L; ++l) j.outs[l] = (level_out && level_out[l]) ? level_out[l] : c->level_buf[l];
  if (layer_ms) {        // measurement path: one stream, one chunk, an event pair around every launch
    std::vector<hipEvent_t> ev(c->m->layers.size() + 1);
    for (auto& e : ev) HIPCHK(c, hipEventCreate(&e));
    s = run_layers(c, x, 0, B, j.outs, st, ev.data());
    if (s == YL_OK) {
      HIPCHK(c, hipStreamSynchronize(st));
      for (size_t i = 0; i < c->m->layers.size(); ++i) hipEventElapsedTime(&layer_ms[i], ev[i], ev[i + 1]);
    }
    for (auto& e : ev) hipEventDestroy(e);
    return s;
  }
  return submit(c, j, st);
}

yl_status yl_forward(yl_ctx* c, const float* x, int32_t B, float* const* level_out, void* stream) {
  return forward_impl(c, x, B, level_out, (hipStream_t)stream, nullptr, nullptr, nullptr, nullptr);
}

yl_status yl_forward_timed(yl_ctx* c, const float* x, int32_t B, float* const* level_out, void* stream,
                           float* layer_ms) {
  if (!layer_ms) return YL_ERR_INVALID;
  return forward_impl(c, x, B, level_out, (hipStream_t)stream, layer_ms, nullptr, nullptr, nullptr);
}

yl_status yl_last_timing(yl_ctx* c, float* infer_ms, float* post_ms) {
  if (!c || !infer_ms || !post_ms) return YL_ERR_INVALID;
  if (!c->opt_time_split || !c->timing_valid) return fail(c, YL_ERR_STATE, "set option time_split and call yl_predict first");
  HIPCHK(c, hipEventSynchronize(c->ev_t[2]));
  HIPCHK(c, hipEventElapsedTime(infer_ms, c->ev_t[0], c->ev_t[1]));
  HIPCHK(c, hipEventElapsedTime(post_ms, c->ev_t[1], c->ev_t[2]));
  return YL_OK;
}

int64_t yl_activation_bytes(const yl_ctx* c) {
  if (!c || c->plan_n < 1) return 0;
  int64_t t = 0;
  for (int i = 0; i < c->arena_n; ++i) t += (int64_t)(c->arena_unit + c->m->se_unit * sizeof(float)) * c->arena_capi[i];
  for (const auto& s : c->slots)
    if (s.pinned) t += (int64_t)s.sz * c->cap_batch;
  return t;
}

yl_status yl_read_slot(yl_ctx* c, int32_t slot, int32_t B, float* dst, void* stream) {
  if (!c || !dst) return YL_ERR_INVALID;
  if (slot < 0 || slot >= (int)c->slots.size()) return fail(c, YL_ERR_INVALID, "bad slot");
  if (B > c->act_batch || c->plan_n < 1) return fail(c, YL_ERR_STATE, "no forward of >= B images has produced this slot");
  HIPCHK(c, hipSetDevice(c->m->device));
  const Slot& s = c->slots[slot];
  if (c->opt_bf16 == 3 && !s.pinned) return fail(c, YL_ERR_UNSUPPORTED, "store_f16: activation slots are fp16 (yl_read_slot hands out fp32)");
  // (with "reuse_slots" on, a tensor that is not an output of the network may have been overwritten by later layers)
  for (int i = 0; i < c->plan_n; ++i) {
    const int b0 = c->plan_b0[i], b1 = c->plan_b0[i + 1] < B ? c->plan_b0[i + 1] : B;
    if (b1 <= b0) break;
    HIPCHK(c, hipMemcpyAsync((char*)dst + (size_t)b0 * s.sz, slot_addr(c, slot, b0), (size_t)(b1 - b0) * s.sz,
                             hipMemcpyDeviceToDevice, (hipStream_t)stream));
  }
  return YL_OK;
}

yl_status yl_preprocess(yl_ctx* c, const uint8_t* packed, const yl_pre_image* imgs, int32_t B, float* x, void* stream) {
  if (!c || !packed || !imgs || !x || B < 1) return YL_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->m->device));
  static_assert(sizeof(yl_pre_image) == 32, "yl_pre_image layout");
  HIPCHK(c, yl_launch_preprocess(packed, imgs, B, c->m->img_size, x, c->opt_pre_norm, (hipStream_t)stream));
  return YL_OK;
}

yl_status yl_decode(yl_ctx* c, const float* const* levels, int32_t B, int32_t center_mode, int32_t wh_mode,
                    float* box, float* obj, float* cls, void* stream) {
  if (!c || !levels || !box || !obj || B < 1) return YL_ERR_INVALID;
  if (c->m->C > 0 && !cls) return fail(c, YL_ERR_INVALID, "cls_dev is NULL");
  if (center_mode < 0 || center_mode > 1 || wh_mode < 0 || wh_mode > 2) return fail(c, YL_ERR_INVALID, "bad mode");
  HIPCHK(c, hipSetDevice(c->m->device));
  YlLevels lv;
  fill_levels(c, levels, lv);
  HIPCHK(c, yl_launch_decode_only(lv, B, center_mode, wh_mode, box, obj, cls, (hipStream_t)stream));
  return YL_OK;
}

yl_status yl_forward_decoded(yl_ctx* c, const float* x, int32_t B, int32_t center_mode, int32_t wh_mode, float* box,
                             float* obj, float* cls, void* stream) {
  if (!c || !box || !obj) return YL_ERR_INVALID;
  if (c->m->C > 0 && !cls) return fail(c, YL_ERR_INVALID, "cls_dev is NULL");
  if (center_mode < 0 || center_mode > 1 || wh_mode < 0 || wh_mode > 2) return fail(c, YL_ERR_INVALID, "bad mode");
  // the raw levels go to the context's own buffers (two chunk streams, hipGraph: as yl_forward), the decode follows on
  // the caller's stream behind the join
  yl_status s = forward_impl(c, x, B, nullptr, (hipStream_t)stream, nullptr, nullptr, nullptr, nullptr);
  if (s != YL_OK) return s;
  YlLevels lv;
  fill_levels(c, c->level_buf, lv);
  HIPCHK(c, yl_launch_decode_only(lv, B, center_mode, wh_mode, box, obj, cls, (hipStream_t)stream));
  return YL_OK;
}

yl_status yl_postprocess(yl_ctx* c, const float* const* levels, int32_t B, const yl_post_cfg* cfg, float* dets,
                         int32_t* counts, int32_t* keep_idx, void* stream) {
  if (!c || !levels || !dets || !counts || B < 1) return YL_ERR_INVALID;
  yl_status s = check_cfg(c, cfg);
  if (s != YL_OK) return s;
  HIPCHK(c, hipSetDevice(c->m->device));
  if ((s = ensure_post(c, B)) != YL_OK) return s;
  Job j;
  j.B = B; j.cfg = cfg; j.dets = dets; j.counts = counts; j.keep_idx = keep_idx;
  for (int l = 0; l < c->m->L; ++l) j.outs[l] = const_cast<float*>(levels[l]);
  return submit(c, j, (hipStream_t)stream, false);
}

yl_status yl_predict(yl_ctx* c, const float* x, int32_t B, const yl_post_cfg* cfg, float* dets, int32_t* counts,
                     int32_t* keep_idx, void* stream) {
  if (!c || !dets || !counts) return YL_ERR_INVALID;
  yl_status s = check_cfg(c, cfg);
  if (s != YL_OK) return s;
  return forward_impl(c, x, B, nullptr, (hipStream_t)stream, nullptr, cfg, dets, counts, keep_idx);
}

yl_status yl_masks(yl_ctx* c, const float* const* levels, int32_t B, const int32_t* counts, const int32_t* keep_idx,
                   int32_t max_out, float thr, uint8_t* masks, void* stream) {
  if (!c || !counts || !keep_idx || !masks || B < 1 || max_out < 1) return YL_ERR_INVALID;
  if (c->m->NM <= 0 || c->m->proto_slot < 0) return fail(c, YL_ERR_STATE, "context has no mask branch");
  if (B > c->act_batch || B > c->post_cap_batch || !c->slots[c->m->proto_slot].pin)
    return fail(c, YL_ERR_STATE, "yl_masks needs a preceding yl_predict / yl_forward+yl_postprocess of this batch");
  HIPCHK(c, hipSetDevice(c->m->device));
  const float* lp[YL_MAX_LEVELS];
  for (int l = 0; l < c->m->L; ++l) lp[l] = (levels && levels[l]) ? levels[l] : c->level_buf[l];
  YlLevels lv;
  fill_levels(c, lp, lv);
  const Slot& ps = c->slots[c->m->proto_slot];
  HIPCHK(c, yl_launch_masks(lv, B, ps.pin, ps.h, ps.w, c->m->NM, c->m->img_size, c->ws_boxes, counts, keep_idx, max_out, thr,
                            masks, (hipStream_t)stream));
  return YL_OK;
}

yl_status yl_masks_image(yl_ctx* c, const float* const* levels, int32_t B, const float* dets, const int32_t* counts,
                         const int32_t* keep_idx, int32_t max_out, float thr, const float* backmap,
                         const int32_t* out_hw, const int64_t* mask_off, int32_t max_h, int32_t max_w, int32_t packed,
                         uint8_t* masks, void* stream) {
  if (!c || !dets || !counts || !keep_idx || !out_hw || !mask_off || !masks || B < 1 || max_out < 1 || max_h < 1 || max_w < 1)
    return YL_ERR_INVALID;
  if (c->m->NM <= 0 || c->m->proto_slot < 0) return fail(c, YL_ERR_STATE, "context has no mask branch");
  if (B > c->act_batch || !c->slots[c->m->proto_slot].pin)
    return fail(c, YL_ERR_STATE, "yl_masks_image needs a preceding yl_predict / yl_forward of this batch");
  HIPCHK(c, hipSetDevice(c->m->device));
  const float* lp[YL_MAX_LEVELS];
  for (int l = 0; l < c->m->L; ++l) lp[l] = (levels && levels[l]) ? levels[l] : c->level_buf[l];
  YlLevels lv;
  fill_levels(c, lp, lv);
  const Slot& ps = c->slots[c->m->proto_slot];
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  HIPCHK(c, yl_launch_masks_image(lv, B, ps.pin, ps.h, ps.w, c->m->NM, c->m->img_size, dets, counts, keep_idx, max_out, thr,
                                  backmap, out_hw, (const long long*)mask_off, max_h, max_w, packed ? 1 : 0, masks,
                                  (hipStream_t)stream));
  return YL_OK;
}

// the one exchange of the multi-GPU path, for hosts that do not go through torch.distributed.  RCCL is
// NOT a link-time dependency of this library: ncclAllGather is looked up among the libraries already loaded in the
// process, i.e. the RCCL that created the caller's communicator (PyTorch ships its own copy).
yl_status yl_allgather_dets(yl_ctx* c, void* comm, const float* local_dev, int64_t row_floats, float* all_dev, void* stream) {
  if (!c || !comm || !local_dev || !all_dev || row_floats <= 0) return c ? fail(c, YL_ERR_INVALID, "bad argument") : YL_ERR_INVALID;
  typedef int (*allgather_fn)(const void*, void*, size_t, int /*ncclDataType_t*/, void* /*ncclComm_t*/, hipStream_t);
  static allgather_fn fn = nullptr;
  if (!fn) fn = (allgather_fn)dlsym(RTLD_DEFAULT, "ncclAllGather");
  if (!fn) return fail(c, YL_ERR_UNSUPPORTED, "ncclAllGather not found: load RCCL (librccl.so) in this process first");
  HIPCHK(c, hipSetDevice(c->m->device));
  const int rc = fn(local_dev, all_dev, (size_t)row_floats, 7 /*ncclFloat32*/, comm, (hipStream_t)stream);
  if (rc != 0) {
    char b[96];
    snprintf(b, sizeof(b), "ncclAllGather failed with ncclResult_t %d", rc);
    return fail(c, YL_ERR_HIP, b);
  }
  return YL_OK;
}

yl_status yl_nms(yl_ctx* c, const float* boxes, const float* scores, int32_t n, float iou_thr, int32_t impl,
                 int32_t max_det, int32_t* keep, int32_t* count, void* stream) {
  if (!c || !boxes || !scores || !keep || !count || n < 0 || max_det < 1) return YL_ERR_INVALID;
  if (impl != YL_NMS_TORCHVISION && impl != YL_NMS_GREEDY) return fail(c, YL_ERR_INVALID, "bad nms_impl");
  if (n >= (1 << 20)) return fail(c, YL_ERR_UNSUPPORTED, "n must be < 2^20");
  HIPCHK(c, hipSetDevice(c->m->device));
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    HIPCHK(c, hipMemsetAsync(count, 0, sizeof(int), st));
    return YL_OK;
  }
  if (!c->ws_nms_clsws) HIPCHK(c, hipMalloc((void**)&c->ws_nms_clsws, 4 * sizeof(int)));
  const int P = pow2ceil(n);
  if (P > YL_LDS_KEYS_MAX && P > c->nms_gP) {
    hipFree(c->ws_nms_gkeys);
    c->ws_nms_gkeys = nullptr;
    HIPCHK(c, hipMalloc((void**)&c->ws_nms_gkeys, (size_t)P * 8));
    c->nms_gP = P;
  }
  // dets rows are not wanted here: reuse the top-k staging path's buffers? No -- a scratch dets
  // buffer of max_det rows is taken from the tmp area sized for n rows.
  float* scratch = nullptr;
  HIPCHK(c, hipMallocAsync((void**)&scratch, (size_t)max_det * 6 * sizeof(float), st));
  YlNmsP np;
  memset(&np, 0, sizeof(np));
  np.boxes = (const float4*)boxes; np.scores = scores; np.cls = nullptr;
  np.N = n; np.C = 1;
  np.conf_thr = -INFINITY; np.iou_thr = iou_thr; np.impl = impl;
  np.cap = max_det; np.topk = 0; np.max_out = max_det;
  np.cls_ws = c->ws_nms_clsws;
  np.gkeys = c->ws_nms_gkeys; np.gP = c->nms_gP;
  np.lds_cap = P < YL_LDS_KEYS_MAX ? P : YL_LDS_KEYS_MAX;
  np.dets = scratch; np.counts = count; np.keep_idx = keep; np.backmap = nullptr;
  hipError_t e = yl_launch_nms(np, 1, st);
  hipFreeAsync(scratch, st);
  HIPCHK(c, e);
  return YL_OK;
}

// argument checks shared by the three loss entries
static yl_status loss_check(yl_ctx* c, const float* const* levels, int32_t B, const float* gt_xyxy, const int32_t* gt_label,
                            const int32_t* gt_off, int32_t num_gt, const yl_loss_cfg* cfg) {
  if (!c || !levels || !cfg || B < 1 || num_gt < 0) return YL_ERR_INVALID;
  if (num_gt > 0 && (!gt_xyxy || !gt_label || !gt_off)) return fail(c, YL_ERR_INVALID, "ground-truth arrays are NULL");
  if (cfg->num_classes != c->m->C || cfg->img_size != c->m->img_size)
    return fail(c, YL_ERR_INVALID, "yl_loss_cfg num_classes / img_size differ from the context's");
  if (c->m->C < 1) return fail(c, YL_ERR_INVALID, "the loss needs at least one class");
  if (cfg->center_mode < 0 || cfg->center_mode > 1 || cfg->wh_mode < 0 || cfg->wh_mode > 2)
    return fail(c, YL_ERR_INVALID, "bad mode");
  for (int l = 0; l < c->m->L; ++l)
    if (c->m->level_A[l] != 1)
      return fail(c, YL_ERR_UNSUPPORTED, "LossAF is defined for one anchor per cell (the reference builds h*w anchors per level)");
  if (cfg->topk_limit < 1 || cfg->topk_limit > YL_LOSS_MAX_TOPK)
    return fail(c, YL_ERR_UNSUPPORTED, "topk_limit must be 1.." + std::to_string(YL_LOSS_MAX_TOPK));
  if (!(cfg->area_tol > 0.0f)) return fail(c, YL_ERR_INVALID, "area_tol must be positive");
  return YL_OK;
}

// yl_loss_af (sel == nullptr) and yl_loss_af_train
static yl_status loss_forward(yl_ctx* c, const float* const* levels, int32_t B, const float* gt_xyxy, const int32_t* gt_label,
                              const int32_t* gt_off, int32_t num_gt, const yl_loss_cfg* cfg, float* per_image,
                              int32_t* assign, int32_t* sel, float* out4, void* stream) {
  if (!out4) return YL_ERR_INVALID;
  const yl_status chk = loss_check(c, levels, B, gt_xyxy, gt_label, gt_off, num_gt, cfg);
  if (chk != YL_OK) return chk;
  HIPCHK(c, hipSetDevice(c->m->device));
  if (B > c->loss_cap_batch) {
    hipFree(c->ws_loss_keys); hipFree(c->ws_loss_neg); hipFree(c->ws_loss_pi); hipFree(c->ws_loss_pos);
    c->ws_loss_keys = nullptr; c->ws_loss_neg = nullptr; c->ws_loss_pi = nullptr; c->ws_loss_pos = nullptr;
    c->loss_cap_batch = 0;
    HIPCHK(c, hipMalloc((void**)&c->ws_loss_keys, (size_t)B * c->m->N * sizeof(unsigned long long)));
    HIPCHK(c, hipMalloc((void**)&c->ws_loss_neg, (size_t)B * c->m->N * sizeof(float)));
    HIPCHK(c, hipMalloc((void**)&c->ws_loss_pi, (size_t)B * 3 * sizeof(float)));
    HIPCHK(c, hipMalloc((void**)&c->ws_loss_pos, (size_t)B * sizeof(int)));
    c->loss_cap_batch = B;
  }
  YlLevels lv;
  fill_levels(c, levels, lv);
  YlLossP p;
  memset(&p, 0, sizeof(p));
  p.cfg = *cfg;
  // LossAF.__init__ folds area_tol into the bounds as Python floats; the comparison rounds them to fp32
  p.area_min = (float)((double)cfg->area_cells_min / (double)cfg->area_tol);
  p.area_max = (float)((double)cfg->area_cells_max * (double)cfg->area_tol);
  p.gt = gt_xyxy; p.label = gt_label; p.off = gt_off; p.T = num_gt; p.B = B;
  p.keys = c->ws_loss_keys; p.negv = c->ws_loss_neg;
  p.per_image = per_image ? per_image : c->ws_loss_pi;
  p.has_pos = c->ws_loss_pos; p.assign = assign; p.out4 = out4; p.sel = sel;
  HIPCHK(c, yl_launch_loss_af(lv, p, (hipStream_t)stream));
  return YL_OK;
}


yl_status yl_loss_af(yl_ctx* c, const float* const* levels, int32_t B, const float* gt_xyxy, const int32_t* gt_label,
                     const int32_t* gt_off, int32_t num_gt, const yl_loss_cfg* cfg, float* per_image, int32_t* assign,
                     float* out4, void* stream) {
  return loss_forward(c, levels, B, gt_xyxy, gt_label, gt_off, num_gt, cfg, per_image, assign, nullptr, out4, stream);
}

yl_status yl_loss_af_train(yl_ctx* c, const float* const* levels, int32_t B, const float* gt_xyxy,
                           const int32_t* gt_label, const int32_t* gt_off, int32_t num_gt, const yl_loss_cfg* cfg,
                           float* per_image, int32_t* assign, int32_t* sel, float* out4, void* stream) {
  if (!assign || !sel) return c ? fail(c, YL_ERR_INVALID, "yl_loss_af_train needs assign_dev and sel_dev") : YL_ERR_INVALID;
  return loss_forward(c, levels, B, gt_xyxy, gt_label, gt_off, num_gt, cfg, per_image, assign, sel, out4, stream);
}

yl_status yl_loss_af_backward(yl_ctx* c, const float* const* levels, int32_t B, const float* gt_xyxy,
                              const int32_t* gt_label, const int32_t* gt_off, int32_t num_gt, const yl_loss_cfg* cfg,
                              const int32_t* assign, const int32_t* sel, const float* grad_out,
                              float* const* grad_levels, void* stream) {
  const yl_status chk = loss_check(c, levels, B, gt_xyxy, gt_label, gt_off, num_gt, cfg);
  if (chk != YL_OK) return chk;
  if (!assign || !sel || !grad_out || !grad_levels) return fail(c, YL_ERR_INVALID, "yl_loss_af_backward: a NULL argument");
  for (int l = 0; l < c->m->L; ++l)
    if (!grad_levels[l]) return fail(c, YL_ERR_INVALID, "yl_loss_af_backward: a NULL gradient tensor");
  HIPCHK(c, hipSetDevice(c->m->device));
  YlLevels lv;
  fill_levels(c, levels, lv);
  YlLossGradP p;
  memset(&p, 0, sizeof(p));
  p.cfg = *cfg;
  p.gt = gt_xyxy; p.label = gt_label; p.assign = assign; p.sel = sel; p.gout = grad_out; p.B = B;
  for (int l = 0; l < c->m->L; ++l) p.out[l] = grad_levels[l];
  HIPCHK(c, yl_launch_loss_af_grad(lv, p, (hipStream_t)stream));
  return YL_OK;
}

}  // extern "C"
