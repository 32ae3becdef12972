// Trainable depthwise FPN neck (reference scripts/model/model_v2.py:285-294 lateral* / smooth*, :337-361 the top-down
// chain of YOLOLiteMS_CPU): forward and backward of all levels on NHWC fp32 rows, M_k = B * S_k * S_k rows per level.
//
//   forward, coarsest level first:   t_k = c_k . Wlat_k^T + blat_k  (+ up(p_{k+1}))      p_k = blocks(t_k)
//   backward, finest level first:    G_k = gp_k (+ up^T(gt_{k-1}))   gt_k = blocks^T(G_k)
//                                    dWlat_k = gt_k^T . c_k   dblat_k = colsum gt_k   dc_k = gt_k . Wlat_k
//
// The block (depthwise 3x3 -> 1x1 -> BatchNorm -> ReLU), its kernels and its launch sequences are the heads'
// (yl_block.h).  The lateral's epilogue, the transposed upsample as a gather, the lateral's gradients and the nearest
// maps on the device are shared with the dense neck (yl_fpn.h).
// The nearest maps follow torch (scale = (float)in / out in fp32, src = min((int)floorf(dst * scale), in - 1)); they are
// computed on the host and kept on the device as small int tables.
#include "yl_fpn.h"

struct yl_neck {
  Arena mem;                             // yl_block.h
  yl_neck_cfg cfg;
  MapTables maps;                        // yl_fpn.h
  int fB, fS[YL_NECK_MAX_LEVELS], fTrain;   // the forward whose activations are held (mem.fValid)
};

extern "C" {

yl_status yl_neck_nearest_map(int32_t out, int32_t in, int32_t* src, int32_t* lo, int32_t* hi) {
  if (out < 1 || in < 1 || !src) return YL_ERR_INVALID;
  const float scale = (float)in / (float)out;
  for (int o = 0; o < out; ++o) {
    int s = (int)floorf((float)o * scale);
    src[o] = s < in - 1 ? s : in - 1;
  }
  if (lo && hi) {
    int o = 0;
    for (int i = 0; i < in; ++i) {       // monotone: the cells that read i are consecutive
      lo[i] = o;
      while (o < out && src[o] == i) ++o;
      hi[i] = o;
    }
  }
  return YL_OK;
}

yl_status yl_neck_plan(const yl_neck_cfg* cfg, int32_t batch, const int32_t* sizes, yl_neck_plan_info* out) {
  if (!cfg_ok(cfg) || !out || !sizes || batch < 1) return YL_ERR_INVALID;
  for (int k = 0; k < cfg->num_levels; ++k)
    if (sizes[k] < 1) return YL_ERR_INVALID;
  if (!cfg_supported(cfg)) return YL_ERR_UNSUPPORTED;
  memset(out, 0, sizeof(*out));
  out->stat_rows = STAT_ROWS; out->gemm_rows = GEMM_ROWS;
  const int64_t F = cfg->channels;
  int64_t Mmax = 0, smax = 0, wmax = 0;
  for (int k = 0; k < cfg->num_levels; ++k) {
    const int64_t M = (int64_t)batch * sizes[k] * sizes[k], Cin = cfg->in_channels[k];
    if (!level_rows_ok(M, F, Cin)) return YL_ERR_UNSUPPORTED;
    yl_neck_level_plan& lp = out->level[k];
    lp.rows = (int32_t)M;
    lp.stat_tiles = ceil_div(M, STAT_ROWS); lp.gemm_tiles = ceil_div(M, GEMM_ROWS);
    split_plan((int)M, (int)F, (int)F, &lp.wgrad_rows, &lp.wgrad_splits);
    split_plan((int)M, (int)Cin, (int)F, &lp.lgrad_rows, &lp.lgrad_splits);
    lp.saved_bytes = (1 + 3 * (int64_t)cfg->depth) * M * F * 4 + cfg->depth * 2 * F * 4;
    out->saved_bytes += lp.saved_bytes;
    Mmax = M > Mmax ? M : Mmax;
    const int64_t sp = spart_bytes(lp.stat_tiles, F, F);
    smax = sp > smax ? sp : smax;
    int64_t wp = (int64_t)lp.wgrad_splits * F * F * 4;
    const int64_t lpb = (int64_t)lp.lgrad_splits * F * Cin * 4;
    wp = ((wp > lpb ? wp : lpb) + 15) & ~(int64_t)15;
    wmax = wp > wmax ? wp : wmax;
  }
  out->table_bytes = map_table_bytes(cfg->num_levels, sizes);
  out->nosave_bytes = 4 * Mmax * F * 4 + 2 * F * 4;
  out->workspace_bytes = 3 * Mmax * F * 4 + smax + 2 * F * 4 + wmax;
  return YL_OK;
}

void yl_neck_destroy(yl_neck* h) {
  if (!h) return;
  arena_release(h->mem);
  hipFree(h->maps.dev); (void)hipGetLastError();
  delete h;
}

yl_status yl_neck_held(const yl_neck* h, int64_t* saved_bytes, int64_t* workspace_bytes, int32_t* forward_held) {
  return arena_held(h ? &h->mem : nullptr, saved_bytes, workspace_bytes, forward_held);
}

yl_status yl_neck_create(int32_t device, const yl_neck_cfg* cfg, yl_neck** out) {
  if (!out || !cfg_ok(cfg)) return YL_ERR_INVALID;
  if (!cfg_supported(cfg)) return YL_ERR_UNSUPPORTED;
  if (hipSetDevice(device) != hipSuccess) return YL_ERR_HIP;
  yl_neck* h = new (std::nothrow) yl_neck();
  if (!h) return YL_ERR_NOMEM;
  h->mem.device = device; h->cfg = *cfg;
  *out = h;
  return YL_OK;
}

}  // extern "C"

namespace {

struct NeckBuffers {
  Buffers lv[YL_NECK_MAX_LEVELS];        // ga, gb, spart, coef, wpart are the same workspace in every level
  float* t[YL_NECK_MAX_LEVELS];
  float* gt;
  LevelMaps maps[YL_NECK_MAX_LEVELS];
};

// the handle's memory for (batch, sizes), cut as yl_neck_plan counts it; `save`: every level and block apart
yl_status ensure(yl_neck* h, int B, const int32_t* sizes, bool save, yl_neck_plan_info* pl, NeckBuffers* nb) {
  yl_status st = yl_neck_plan(&h->cfg, B, sizes, pl);
  if (st != YL_OK) return st;
  st = arena_reserve(h->mem, save ? pl->saved_bytes : pl->nosave_bytes, pl->workspace_bytes);
  if (st != YL_OK) return st;
  const int L = h->cfg.num_levels, D = h->cfg.depth;
  const size_t F = h->cfg.channels;
  st = maps_ensure(h->maps, L, sizes, pl->table_bytes, nb->maps);
  if (st != YL_OK) return st;
  size_t amax = 0, smax = 0;
  for (int k = 0; k < L; ++k) {
    const size_t a = (size_t)pl->level[k].rows * F * 4, sp = (size_t)spart_bytes(pl->level[k].stat_tiles, F, F);
    amax = a > amax ? a : amax;
    smax = sp > smax ? sp : smax;
  }
  char* w = h->mem.work;
  float* ga = (float*)w; w += amax;
  float* gb = (float*)w; w += amax;
  nb->gt = (float*)w; w += amax;
  double* spart = (double*)w; w += smax;
  float* coef = (float*)w; w += 2 * F * 4;
  float* wpart = (float*)w;
  char* p = h->mem.saved;
  for (int k = 0; k < L; ++k) {
    Buffers& bf = nb->lv[k];
    const size_t act = (size_t)pl->level[k].rows * F * 4;
    if (!save) p = h->mem.saved;         // every level in the same memory
    nb->t[k] = (float*)p; p += act;
    p = carve_blocks(p, save ? D : 1, act, F, &bf);
    bf.ga = ga; bf.gb = gb; bf.spart = spart; bf.coef = coef; bf.wpart = wpart;
  }
  return YL_OK;
}

bool params_ok(const yl_neck_cfg& c, const yl_neck_tensors* t) {
  if (!t) return false;
  uintptr_t any = 0;
  for (int k = 0; k < c.num_levels; ++k) {
    const yl_neck_level& l = t->level[k];
    if (!l.lat_w || !l.lat_b) return false;
    any |= (uintptr_t)l.lat_w | (uintptr_t)l.lat_b;
    if (!blocks_params_ok(l.block, c.depth, &any)) return false;
  }
  return !(any & 3u);
}

}  // namespace

extern "C" {

yl_status yl_neck_forward(yl_neck* h, const yl_neck_tensors* params, const float* const* c_dev, int32_t batch,
                          const int32_t* sizes, uint32_t flags, float* const* p_dev, void* stream, int32_t* launches) {
  if (!h || !c_dev || !p_dev || !sizes || !params_ok(h->cfg, params)) return YL_ERR_INVALID;
  const int L = h->cfg.num_levels, D = h->cfg.depth, F = h->cfg.channels;
  const bool train = flags & YL_HEAD_TRAIN, save = flags & YL_HEAD_SAVE;
  for (int k = 0; k < L; ++k) {
    if (!c_dev[k] || !p_dev[k] || sizes[k] < 1) return YL_ERR_INVALID;
    if (((uintptr_t)c_dev[k] & 15u) || ((uintptr_t)p_dev[k] & 15u)) return YL_ERR_UNSUPPORTED;
    if (train && (int64_t)batch * sizes[k] * sizes[k] < 2) return YL_ERR_INVALID;   // no variance of one value
  }
  yl_neck_plan_info pl;
  NeckBuffers nb;
  const yl_status st = ensure(h, batch, sizes, save, &pl, &nb);
  if (st != YL_OK) return st;
  hipStream_t s = (hipStream_t)stream;
  int nl = 0;
  h->mem.fValid = 0;
  for (int k = L - 1; k >= 0; --k) {
    const yl_neck_level& lv = params->level[k];
    const int M = pl.level[k].rows, Cin = h->cfg.in_channels[k], S = sizes[k];
    lateral_forward(s, lv.lat_w, lv.lat_b, c_dev[k], nb.t[k], k + 1 < L ? p_dev[k + 1] : nullptr, nb.maps[k].src, F, M, Cin, S,
                    k + 1 < L ? sizes[k + 1] : 0);
    ++nl;
    // with `save` the last block writes the handle's h and p_k is a copy of it; without, it writes p_k
    const float* last = blocks_forward<false>(s, lv.block, D, nb.t[k], nb.lv[k], save, train, 0, dims_of(pl.level[k], S, F),
                                              save ? nullptr : p_dev[k], &nl);
    if (save && hipMemcpyAsync(p_dev[k], last, (size_t)M * F * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return YL_ERR_HIP;
  }
  if (launches) *launches = nl;
  if (hipGetLastError() != hipSuccess) return YL_ERR_HIP;
  if (save) {
    h->fB = batch; h->fTrain = train ? 1 : 0; h->mem.fValid = 1;
    for (int k = 0; k < L; ++k) h->fS[k] = sizes[k];
  }
  return YL_OK;
}

yl_status yl_neck_backward(yl_neck* h, const yl_neck_tensors* params, const yl_neck_tensors* grads,
                           const float* const* c_dev, const float* const* gp_dev, float* const* dc_dev, int32_t batch,
                           const int32_t* sizes, void* stream, int32_t* launches) {
  if (!h || !grads || !c_dev || !gp_dev || !sizes || !params_ok(h->cfg, params)) return YL_ERR_INVALID;
  const int L = h->cfg.num_levels, D = h->cfg.depth, F = h->cfg.channels;
  uintptr_t gany = 0;
  int K = -1;                            // the coarsest level something is wanted of
  for (int k = 0; k < L; ++k) {
    if (!c_dev[k] || !gp_dev[k]) return YL_ERR_INVALID;
    float* dc = dc_dev ? dc_dev[k] : nullptr;
    if (((uintptr_t)c_dev[k] & 15u) || ((uintptr_t)gp_dev[k] & 15u) || ((uintptr_t)dc & 15u)) return YL_ERR_UNSUPPORTED;
    const yl_neck_level& g = grads->level[k];
    gany |= (uintptr_t)g.lat_w | (uintptr_t)g.lat_b;
    if (blocks_grads_wanted(g.block, D, &gany) || g.lat_w || g.lat_b || dc) K = k;
  }
  if (gany & 3u) return YL_ERR_UNSUPPORTED;            // before the first launch: nothing of the caller's is written
  if (!h->mem.fValid || h->fB != batch) return YL_ERR_STATE;
  for (int k = 0; k < L; ++k)
    if (h->fS[k] != sizes[k]) return YL_ERR_STATE;
  yl_neck_plan_info pl;
  NeckBuffers nb;
  const yl_status st = ensure(h, batch, sizes, true, &pl, &nb);
  if (st != YL_OK) return st;
  if (!h->mem.fValid) return YL_ERR_STATE;
  hipStream_t s = (hipStream_t)stream;
  const bool train = h->fTrain != 0;
  int nl = 0;
  for (int k = 0; k <= K; ++k) {
    const yl_neck_level& lv = params->level[k];
    const yl_neck_level& g = grads->level[k];
    const yl_neck_level_plan& lp = pl.level[k];
    const Buffers& bf = nb.lv[k];
    const int M = lp.rows, Cin = h->cfg.in_channels[k], S = sizes[k];
    float* dc = dc_dev ? dc_dev[k] : nullptr;
    const float* gin = gp_dev[k];
    if (k > 0) {                         // G_k = gp_k + up^T(gt_{k-1}): level k - 1 was walked down to its gt
      hipLaunchKernelGGL(yl_neck_upadd_bwd_kernel, dim3(ceil_div((long)M * (F >> 2), NT)), dim3(NT), 0, s,
                         (const float*)nb.gt, gp_dev[k], bf.ga, nb.maps[k - 1].lo, nb.maps[k - 1].hi, M, S, sizes[k - 1], F);
      ++nl;
      gin = bf.ga;
    }
    const bool lateral = g.lat_w || g.lat_b || dc;
    const bool need_gt = lateral || k < K;
    const int first = need_gt ? 0 : blocks_first_wanted(g.block, D);
    blocks_backward<false>(s, lv.block, g.block, D, first, gin, nb.t[k], need_gt ? nb.gt : nullptr, bf, train, 0,
                           dims_of(lp, S, F), &nl);
    lateral_backward(s, lv.lat_w, g.lat_w, g.lat_b, dc, c_dev[k], nb.gt, bf.wpart, bf.spart, F, Cin, M, S, lp.stat_tiles,
                     lp.lgrad_rows, lp.lgrad_splits, &nl);
  }
  if (launches) *launches = nl;
  return hipGetLastError() == hipSuccess ? YL_OK : YL_ERR_HIP;
}

}  // extern "C"
