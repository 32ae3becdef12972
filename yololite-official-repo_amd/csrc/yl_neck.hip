// Trainable depthwise FPN neck (reference scripts/model/model_v2.py:285-294 lateral* / smooth*, :337-361 the top-down
// chain of YOLOLiteMS_CPU): forward and backward of all levels on NHWC fp32 rows, M_k = B * S_k * S_k rows per level.
//
//   forward, coarsest level first:   t_k = c_k . Wlat_k^T + blat_k  (+ up(p_{k+1}))      p_k = blocks(t_k)
//   backward, finest level first:    G_k = gp_k (+ up^T(gt_{k-1}))   gt_k = blocks^T(G_k)
//                                    dWlat_k = gt_k^T . c_k   dblat_k = colsum gt_k   dc_k = gt_k . Wlat_k
//
// The block (depthwise 3x3 -> 1x1 -> BatchNorm -> ReLU), its kernels and its launch sequences are the heads'
// (yl_block.h).  New here:
//   * the lateral's epilogue: an output accessor of yl_head_gemm_kernel that adds the bias and the coarser level's p read
//     through the nearest map, and writes t_k;
//   * the transposed upsample as a gather: the nearest map is monotone, so the pre-image of a source cell is a
//     contiguous range of destination rows and of columns; one thread per (b, i, j, channel quad) sums its range in
//     row-major order and adds gp_k.  No atomics;
//   * the lateral's gradients from the GEMM forms of the heads (split GEMM + ordered sum for the weight, NP = Cin,
//     NQ = F; float64 column sums for the bias; one GEMM for dc).
// The nearest maps follow torch (scale = (float)in / out in fp32, src = min((int)floorf(dst * scale), in - 1)); they are
// computed on the host and kept on the device as small int tables.
#include <new>

#include "yl_block.h"

namespace {

// ---- t = acc + bias (+ p of the coarser level at the nearest source cell); rows of F floats, F % 4 == 0
struct OutLateral {
  float* t; const float* bias; const float* up;     // up == NULL: the coarsest level
  const int* src;                                   // [S]: source index of a destination index
  int F, S, Sc;
  __device__ __forceinline__ void store(int p, int q, f32x4 v, int NP, int NQ, int) const {
    if (q >= NQ || p >= NP) return;
    f32x4 o;
#pragma unroll
    for (int s = 0; s < 4; ++s) o[s] = v[s] + bias[p + s];
    if (up) {
      const int SS = S * S, b = q / SS, ij = q - b * SS, i = ij / S, j = ij - i * S;
      const long row = ((long)b * Sc + src[i]) * Sc + src[j];
      o = ld4(up + row * F + p) + o;
    }
    st4(t + (long)q * F + p, o);
  }
};

// G[b, i, j, :] = gp[b, i, j, :] + sum over ii in [lo[i], hi[i]), jj in [lo[j], hi[j]) of gt[b, ii, jj, :]
__global__ __launch_bounds__(NT) void yl_neck_upadd_bwd_kernel(const float* __restrict__ gt, const float* __restrict__ gp,
                                                              float* __restrict__ G, const int* __restrict__ lo,
                                                              const int* __restrict__ hi, int M, int S, int Sf, int F) {
  const int F4 = F >> 2;
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  if (idx >= (long)M * F4) return;
  const int m = (int)(idx / F4), c = (int)(idx - (long)m * F4) * 4;
  const int SS = S * S, b = m / SS, ij = m - b * SS, i = ij / S, j = ij - i * S;
  const int i0 = lo[i], i1 = hi[i], j0 = lo[j], j1 = hi[j];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int ii = i0; ii < i1; ++ii)
    for (int jj = j0; jj < j1; ++jj) acc = acc + ld4(gt + (((long)b * Sf + ii) * Sf + jj) * F + c);
  st4(G + (long)m * F + c, ld4(gp + (long)m * F + c) + acc);
}

// bias gradient: the column-sum partials of yl_head_ysum_kernel summed in tile order
__global__ __launch_bounds__(NT) void yl_neck_bsum_kernel(const double* __restrict__ part, int tiles, int n, float* __restrict__ out) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= n) return;
  double s = 0;
  for (int t = 0; t < tiles; ++t) s += part[(long)t * n + c];
  out[c] = (float)s;
}

bool cfg_ok(const yl_neck_cfg* c) {
  if (!c || c->channels < 4 || c->depth < 1 || c->depth > YL_NECK_MAX_DEPTH || c->num_levels < 1 ||
      c->num_levels > YL_NECK_MAX_LEVELS)
    return false;
  for (int k = 0; k < c->num_levels; ++k)
    if (c->in_channels[k] < 4) return false;
  return true;
}
bool cfg_supported(const yl_neck_cfg* c) {
  if (c->channels & 3) return false;
  for (int k = 0; k < c->num_levels; ++k)
    if (c->in_channels[k] & 3) return false;
  return true;
}

}  // namespace

struct yl_neck {
  Arena mem;                             // yl_block.h
  yl_neck_cfg cfg;
  int64_t table_cap;
  int* tables;
  int tS[YL_NECK_MAX_LEVELS];            // the sizes the tables on the device were made for (0: none)
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
    if (M > (int64_t)65535 * GEMM_ROWS || M * F >= ((int64_t)1 << 40) || M * Cin >= ((int64_t)1 << 40) || Cin > (1 << 20))
      return YL_ERR_UNSUPPORTED;
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
    if (k + 1 < cfg->num_levels) out->table_bytes += ((int64_t)sizes[k] + 2 * (int64_t)sizes[k + 1]) * 4;
  }
  out->nosave_bytes = 4 * Mmax * F * 4 + 2 * F * 4;
  out->workspace_bytes = 3 * Mmax * F * 4 + smax + 2 * F * 4 + wmax;
  return YL_OK;
}

void yl_neck_destroy(yl_neck* h) {
  if (!h) return;
  arena_release(h->mem);
  hipFree(h->tables); (void)hipGetLastError();
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

struct LevelMaps { const int *src, *lo, *hi; };      // of the pair (destination k, source k + 1)

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
  bool same = true;
  for (int k = 0; k < L; ++k) same = same && h->tS[k] == sizes[k];
  if (!same && L > 1) {                  // new maps: nothing that reads the old ones may still run
    if (hipDeviceSynchronize() != hipSuccess) return YL_ERR_HIP;
    for (int k = 0; k < L; ++k) h->tS[k] = 0;
    if (pl->table_bytes > h->table_cap) {
      hipFree(h->tables);
      h->tables = nullptr; h->table_cap = 0;
      if (hipMalloc((void**)&h->tables, (size_t)pl->table_bytes) != hipSuccess) { (void)hipGetLastError(); return YL_ERR_NOMEM; }
      h->table_cap = pl->table_bytes;
    }
    int32_t* host = new (std::nothrow) int32_t[(size_t)pl->table_bytes / 4];
    if (!host) return YL_ERR_NOMEM;
    int32_t* q = host;
    for (int k = 0; k + 1 < L; ++k) {
      yl_neck_nearest_map(sizes[k], sizes[k + 1], q, q + sizes[k], q + sizes[k] + sizes[k + 1]);
      q += sizes[k] + 2 * sizes[k + 1];
    }
    const hipError_t e = hipMemcpy(h->tables, host, (size_t)pl->table_bytes, hipMemcpyHostToDevice);
    delete[] host;
    if (e != hipSuccess) return YL_ERR_HIP;
    for (int k = 0; k < L; ++k) h->tS[k] = sizes[k];
  }
  const int* q = h->tables;
  for (int k = 0; k < YL_NECK_MAX_LEVELS; ++k) nb->maps[k] = LevelMaps{nullptr, nullptr, nullptr};
  for (int k = 0; k + 1 < L; ++k) {
    nb->maps[k] = LevelMaps{q, q + sizes[k], q + sizes[k] + sizes[k + 1]};
    q += sizes[k] + 2 * sizes[k + 1];
  }
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
    OutLateral ol;
    ol.t = nb.t[k]; ol.bias = lv.lat_b; ol.up = k + 1 < L ? p_dev[k + 1] : nullptr; ol.src = nb.maps[k].src;
    ol.F = F; ol.S = S; ol.Sc = k + 1 < L ? sizes[k + 1] : 0;
    launch_gemm(s, RowsScalar{lv.lat_w, Cin}, RowsVec{c_dev[k], Cin}, ol, F, M, Cin, Cin, 1);
    ++nl;
    // with `save` the last block writes the handle's h and p_k is a copy of it; without, it writes p_k
    const float* last = blocks_forward(s, lv.block, D, nb.t[k], nb.lv[k], save, train, dims_of(pl.level[k], S, F),
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
    blocks_backward(s, lv.block, g.block, D, first, gin, nb.t[k], need_gt ? nb.gt : nullptr, bf, train,
                    dims_of(lp, S, F), &nl);
    if (g.lat_w) {                       // dWlat[f][cin] = sum over rows of gt[m][f] * c[m][cin]
      launch_gemm(s, ColsScalar{c_dev[k], Cin}, ColsScalar{nb.gt, F}, OutPartial{bf.wpart, (long)F * Cin}, Cin, F, M,
                  lp.lgrad_rows, lp.lgrad_splits);
      HeadRows none;
      memset(&none, 0, sizeof(none));
      hipLaunchKernelGGL(yl_head_wsum_kernel, dim3(ceil_div((long)F * Cin, NT)), dim3(NT), 0, s, (const float*)bf.wpart,
                         lp.lgrad_splits, Cin, F, g.lat_w, none, 0);
      nl += 2;
    }
    if (g.lat_b) {
      const HeadGeom plain = {1, F, 0, S * S, F};   // column n of row m at m * F + n
      hipLaunchKernelGGL(yl_head_ysum_kernel, dim3(lp.stat_tiles, ceil_div(F, 64)), dim3(NT), 0, s, (const float*)nb.gt,
                         plain, bf.spart, M, F);
      hipLaunchKernelGGL(yl_neck_bsum_kernel, dim3(ceil_div(F, NT)), dim3(NT), 0, s, (const double*)bf.spart,
                         lp.stat_tiles, F, g.lat_b);
      nl += 2;
    }
    if (dc) {                            // dc = gt . Wlat
      launch_gemm(s, ColsScalar{lv.lat_w, Cin}, RowsVec{nb.gt, F}, OutRowsVec{dc, Cin}, Cin, M, F, F, 1);
      ++nl;
    }
  }
  if (launches) *launches = nl;
  return hipGetLastError() == hipSuccess ? YL_OK : YL_ERR_HIP;
}

}  // extern "C"
