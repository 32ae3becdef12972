// Trainable detection heads (reference scripts/model/model_v2.py:23-53 make_head / DWConvBlock, :182-192 _forward_head):
// forward and backward of ONE level's head on NHWC fp32 rows, M = B * S * S rows of F channels.
//
//   block t:  d = dw3x3(x)   z = d . W1^T   h = relu(gamma * (z - mean) * invstd + beta)     (d, z, h are kept for backward)
//   output :  y[b,a,i,j,:] = [Wbox[4a:4a+4]; Wobj[a]; Wcls[C*a:C*(a+1)]] . h + bias           (the level tensor itself)
//
// Parameters are read in PyTorch layout from the caller's tensors on every call (an optimizer updates them in place
// between two calls); there is no packed copy.  The caller's tensors may start at any 4-byte boundary, so they are read
// with scalar loads; the library's own activation buffers and the input are 16-byte aligned and read as float4.
//
// One GEMM kernel serves the three forms.  C[p][q] = sum_r P(p, r) * Q(q, r) on v_mfma_f32_16x16x4_f32: P is the A
// operand (lane (kq = lane >> 4, i = lane & 15) holds P(p0 + i, r0 + 4 kq + s) for step s), Q the B operand, and the lane
// ends with C[p0 + 4 kq .. + 3][q0 + i] -- four consecutive p, so p is the contiguous index of every output:
//   X . W^T        p = out channel, q = row,         r = in channel                         (z, y)
//   dY . W         p = in channel,  q = row,         r = out channel                        (dd, dh)
//   dY^T . X       p = in channel,  q = out channel, r = row, cut into `splits` row ranges  (weight gradients)
// The accessor structs below say where P(p, r), Q(q, r) and C live; the head output's rows are mapped through the three
// tensors box / obj / cls and the anchor-major level layout there.
//
// No floating-point atomics.  Every sum over rows (BN statistics, dgamma / dbeta, depthwise weight gradient, weight and
// bias gradients) is written as per-tile (per-split) partials and summed in tile order in float64 by a second kernel.
// Equal inputs give equal bits.
//
// Mixed precision.  YL_HEAD_F16 / YL_HEAD_BF16 in the forward's flags run the six 1x1 GEMMs (z, dd, dW1 per block; y, dh,
// dWout) with both operands rounded to that type as load4 returns them and one v_mfma_f32_16x16x16_* per p-tile and
// 16-wide k step (yl_head_gemm_kernel<.., P>, yl_block.h); the handle keeps the mode with the held forward (fMode) and the
// backward runs in it.  Everything else here is the fp32 code, whatever the mode.
#include <new>

#include "yl_block.h"

namespace {

bool cfg_ok(const yl_head_cfg* c) {
  return c && c->channels >= 4 && c->num_classes >= 1 && c->num_anchors >= 1 && c->head_depth >= 1 &&
         c->head_depth <= YL_HEAD_MAX_DEPTH;
}

}  // namespace

struct yl_head {
  Arena mem;                             // yl_block.h
  yl_head_cfg cfg;
  int fB, fS, fTrain;                    // the forward whose activations are held (mem.fValid)
  int fMode;                             // and the operand type of its 1x1 GEMMs (yl_head_gemm_kernel's P): the backward's too
};

extern "C" {

yl_status yl_head_plan(const yl_head_cfg* cfg, int32_t batch, int32_t size, yl_head_plan_info* out) {
  if (!cfg_ok(cfg) || !out || batch < 1 || size < 1) return YL_ERR_INVALID;
  if ((cfg->channels & 3) || cfg->num_masks != 0) return YL_ERR_UNSUPPORTED;
  const int64_t M = (int64_t)batch * size * size;
  const int64_t F = cfg->channels, NE = (int64_t)cfg->num_anchors * (5 + cfg->num_classes);
  if (M > (int64_t)65535 * GEMM_ROWS || M * F >= ((int64_t)1 << 40) || NE > (1 << 20)) return YL_ERR_UNSUPPORTED;
  memset(out, 0, sizeof(*out));
  out->rows = (int32_t)M;
  out->stat_rows = STAT_ROWS; out->stat_tiles = ceil_div(M, STAT_ROWS);
  out->gemm_rows = GEMM_ROWS; out->gemm_tiles = ceil_div(M, GEMM_ROWS);
  split_plan((int)M, (int)F, (int)F, &out->wgrad_rows, &out->wgrad_splits);
  split_plan((int)M, (int)F, (int)NE, &out->ograd_rows, &out->ograd_splits);
  const int64_t act = M * F * 4;
  out->saved_bytes = cfg->head_depth * (3 * act + 2 * F * 4);
  int64_t wpart = (int64_t)out->wgrad_splits * F * F * 4;
  const int64_t opart = (int64_t)out->ograd_splits * NE * F * 4;
  wpart = wpart > opart ? wpart : opart;
  wpart = (wpart + 15) & ~(int64_t)15;
  out->workspace_bytes = 2 * act + spart_bytes(out->stat_tiles, F, NE) + wpart + 2 * F * 4;
  return YL_OK;
}

void yl_head_destroy(yl_head* h) {
  if (!h) return;
  arena_release(h->mem);
  delete h;
}

yl_status yl_head_held(const yl_head* h, int64_t* saved_bytes, int64_t* workspace_bytes, int32_t* forward_held) {
  return arena_held(h ? &h->mem : nullptr, saved_bytes, workspace_bytes, forward_held);
}

yl_status yl_head_create(int32_t device, const yl_head_cfg* cfg, yl_head** out) {
  if (!out || !cfg_ok(cfg)) return YL_ERR_INVALID;
  if ((cfg->channels & 3) || cfg->num_masks != 0) return YL_ERR_UNSUPPORTED;
  if (hipSetDevice(device) != hipSuccess) return YL_ERR_HIP;
  yl_head* h = new (std::nothrow) yl_head();
  if (!h) return YL_ERR_NOMEM;
  h->mem.device = device; h->cfg = *cfg;
  *out = h;
  return YL_OK;
}

}  // extern "C"

namespace {

// the handle's memory for (batch, size) is cut as yl_head_plan counts it (Buffers: yl_block.h)
// `blocks`: how many blocks' activations the call keeps apart (head_depth with YL_HEAD_SAVE and in backward, else 1)
yl_status ensure(yl_head* h, int B, int S, int blocks, yl_head_plan_info* pl, Buffers* bf) {
  yl_status st = yl_head_plan(&h->cfg, B, S, pl);
  if (st != YL_OK) return st;
  st = arena_reserve(h->mem, pl->saved_bytes / h->cfg.head_depth * blocks, pl->workspace_bytes);
  if (st != YL_OK) return st;
  const size_t act = (size_t)pl->rows * h->cfg.channels * 4, F = h->cfg.channels;
  carve_blocks(h->mem.saved, blocks, act, F, bf);
  char* p = h->mem.work;
  bf->ga = (float*)p; p += act;
  bf->gb = (float*)p; p += act;
  const size_t NE = (size_t)h->cfg.num_anchors * (5 + h->cfg.num_classes);
  bf->spart = (double*)p; p += (size_t)spart_bytes(pl->stat_tiles, F, NE);
  bf->coef = (float*)p; p += 2 * F * 4;
  bf->wpart = (float*)p;
  return YL_OK;
}

HeadRows head_rows(const yl_head_cfg& c, const yl_head_tensors* t, int SS) {
  HeadRows w;
  w.box = t->box_w; w.obj = t->obj_w; w.cls = t->cls_w; w.box_b = t->box_b; w.obj_b = t->obj_b; w.cls_b = t->cls_b;
  w.g.A = c.num_anchors; w.g.E = 5 + c.num_classes; w.g.C = c.num_classes; w.g.SS = SS; w.g.F = c.channels;
  return w;
}

bool params_ok(const yl_head_cfg& c, const yl_head_tensors* t) {
  if (!t) return false;
  uintptr_t any = 0;
  if (!blocks_params_ok(t->block, c.head_depth, &any)) return false;
  if (!t->box_w || !t->box_b || !t->obj_w || !t->obj_b || !t->cls_w || !t->cls_b) return false;
  any |= (uintptr_t)t->box_w | (uintptr_t)t->box_b | (uintptr_t)t->obj_w | (uintptr_t)t->obj_b | (uintptr_t)t->cls_w |
         (uintptr_t)t->cls_b;
  return !(any & 3u);
}

// ---- the three GEMMs of the output convolutions in the mode `mode`, as yl_head_forward / _backward / _gemm launch them
// y = h . Wout^T + bias: 1 launch
void out_forward(int mode, hipStream_t s, const HeadRows& hw, const float* h_in, float* y, int M) {
  const int F = hw.g.F;
  launch_gemm_in<true>(mode, s, HeadWRows{hw}, RowsVec{h_in, F}, OutHeadY{y, hw}, hw.g.A * hw.g.E, M, F, F, 1);
}
// dh = gy . Wout: 1 launch
void out_dgrad(int mode, hipStream_t s, const HeadRows& hw, const float* gy, float* dh, int M) {
  const int F = hw.g.F, NE = hw.g.A * hw.g.E;
  launch_gemm_in<true>(mode, s, HeadWCols{hw}, HeadYRows{gy, hw.g}, OutRowsVec{dh, F}, F, M, NE, NE, 1);
}
// dWout = gy^T . h into the non-NULL weights of `gw`: the partials of the row splits and their ordered sum, 2 launches
void out_wgrad(int mode, hipStream_t s, const HeadGeom& g, const float* h_in, const float* gy, float* wpart, const HeadRows& gw,
               int M, int rows, int splits) {
  const int F = g.F, NE = g.A * g.E;
  launch_gemm_in<true>(mode, s, ColsScalar{h_in, F}, HeadYCols{gy, g}, OutPartial{wpart, (long)NE * F}, F, NE, M, rows, splits);
  hipLaunchKernelGGL(yl_head_wsum_kernel, dim3(ceil_div((long)NE * F, NT)), dim3(NT), 0, s, (const float*)wpart, splits, F,
                     NE, (float*)nullptr, gw, 1);
}

}  // namespace

extern "C" {

yl_status yl_head_forward(yl_head* h, const yl_head_tensors* params, const float* x_dev, int32_t batch, int32_t size,
                          uint32_t flags, float* y_dev, void* stream, int32_t* launches) {
  const int mode = mode_of(flags);       // both precision bits: refused here, before a held forward is touched
  if (!h || !x_dev || !y_dev || mode < 0 || !params_ok(h->cfg, params)) return YL_ERR_INVALID;
  if (((uintptr_t)x_dev & 15u) || ((uintptr_t)y_dev & 3u)) return YL_ERR_UNSUPPORTED;
  const bool train = flags & YL_HEAD_TRAIN, save = flags & YL_HEAD_SAVE;
  if (train && (int64_t)batch * size * size < 2) return YL_ERR_INVALID;   // no variance of one value
  yl_head_plan_info pl;
  Buffers bf;
  const yl_status st = ensure(h, batch, size, save ? h->cfg.head_depth : 1, &pl, &bf);
  if (st != YL_OK) return st;
  hipStream_t s = (hipStream_t)stream;
  const int M = pl.rows, F = h->cfg.channels, D = h->cfg.head_depth, S = size;
  const BlockDims dm = dims_of(pl, S, F);
  int nl = 0;
  h->mem.fValid = 0;
  const float* in = blocks_forward<true>(s, params->block, D, x_dev, bf, save, train, mode, dm, nullptr, &nl);
  const HeadRows hw = head_rows(h->cfg, params, S * S);
  out_forward(mode, s, hw, in, y_dev, M);
  ++nl;
  if (launches) *launches = nl;
  if (hipGetLastError() != hipSuccess) return YL_ERR_HIP;
  if (save) { h->fB = batch; h->fS = size; h->fTrain = train ? 1 : 0; h->fMode = mode; h->mem.fValid = 1; }
  return YL_OK;
}

yl_status yl_head_backward(yl_head* h, const yl_head_tensors* params, const yl_head_tensors* grads, const float* x_dev,
                           const float* gy_dev, float* dx_dev, int32_t batch, int32_t size, void* stream,
                           int32_t* launches) {
  if (!h || !grads || !x_dev || !gy_dev || !params_ok(h->cfg, params)) return YL_ERR_INVALID;
  if (((uintptr_t)x_dev & 15u) || ((uintptr_t)dx_dev & 15u) || ((uintptr_t)gy_dev & 3u)) return YL_ERR_UNSUPPORTED;
  if (!h->mem.fValid || h->fB != batch || h->fS != size) return YL_ERR_STATE;
  yl_head_plan_info pl;
  Buffers bf;
  uintptr_t gany = (uintptr_t)grads->box_w | (uintptr_t)grads->box_b | (uintptr_t)grads->obj_w | (uintptr_t)grads->obj_b |
                   (uintptr_t)grads->cls_w | (uintptr_t)grads->cls_b;
  blocks_grads_wanted(grads->block, h->cfg.head_depth, &gany);
  if (gany & 3u) return YL_ERR_UNSUPPORTED;            // before the first launch: nothing of the caller's is written
  const yl_status st = ensure(h, batch, size, h->cfg.head_depth, &pl, &bf);
  if (st != YL_OK) return st;
  if (!h->mem.fValid) return YL_ERR_STATE;
  hipStream_t s = (hipStream_t)stream;
  const int M = pl.rows, F = h->cfg.channels, D = h->cfg.head_depth, S = size, train = h->fTrain, mode = h->fMode;
  const BlockDims dm = dims_of(pl, S, F);
  int nl = 0;
  const HeadRows hw = head_rows(h->cfg, params, S * S);
  const int NE = hw.g.A * hw.g.E;
  // 1. the output convolutions: weights by one GEMM over the rows and one sum, biases by column sums of gy
  const HeadRows gw = head_rows(h->cfg, grads, S * S);
  if (grads->box_w || grads->obj_w || grads->cls_w) {
    out_wgrad(mode, s, hw.g, bf.h[D - 1], gy_dev, bf.wpart, gw, M, pl.ograd_rows, pl.ograd_splits);
    nl += 2;
  }
  if (grads->box_b || grads->obj_b || grads->cls_b) {
    hipLaunchKernelGGL(yl_head_ysum_kernel, dim3(pl.stat_tiles, ceil_div(NE, 64)), dim3(NT), 0, s, gy_dev, hw.g, bf.spart,
                       M, NE);
    hipLaunchKernelGGL(yl_head_bsum_kernel, dim3(ceil_div(NE, NT)), dim3(NT), 0, s, (const double*)bf.spart,
                       pl.stat_tiles, NE, gw);
    nl += 2;
  }
  // 2. the trunk, last block first, down to the first block something is wanted of
  int first = blocks_first_wanted(grads->block, D);
  if (dx_dev) first = 0;
  if (first < D) {
    out_dgrad(mode, s, hw, gy_dev, bf.ga, M);
    ++nl;
  }
  blocks_backward<true>(s, params->block, grads->block, D, first, bf.ga, x_dev, dx_dev, bf, train != 0, mode, dm, &nl);
  if (launches) *launches = nl;
  return hipGetLastError() == hipSuccess ? YL_OK : YL_ERR_HIP;
}

yl_status yl_head_gemm(yl_head* h, int32_t site, int32_t pass, uint32_t mode, const yl_head_tensors* params,
                       const float* a_dev, const float* b_dev, float* out_dev, int32_t batch, int32_t size, void* stream,
                       int32_t* launches) {
  if (mode != 0 && mode != YL_HEAD_F16 && mode != YL_HEAD_BF16) return YL_ERR_INVALID;
  if (!h || !a_dev || !out_dev || !params_ok(h->cfg, params)) return YL_ERR_INVALID;
  const bool out = site == YL_HEAD_SITE_OUT, wgrad = pass == YL_HEAD_PASS_WGRAD;
  if ((!out && (site < 0 || site >= h->cfg.head_depth)) || pass < YL_HEAD_PASS_FORWARD || pass > YL_HEAD_PASS_WGRAD ||
      (wgrad && !b_dev))
    return YL_ERR_INVALID;
  // what the kernels read and write as float4 (RowsVec, OutRowsVec); the level tensor and the weights are read by element
  const bool a_rows = !wgrad && !(out && pass == YL_HEAD_PASS_DGRAD), out_rows = !wgrad && !(out && pass == YL_HEAD_PASS_FORWARD);
  if (((uintptr_t)a_dev & (a_rows ? 15u : 3u)) || ((uintptr_t)b_dev & 3u) || ((uintptr_t)out_dev & (out_rows ? 15u : 3u)))
    return YL_ERR_UNSUPPORTED;
  yl_head_plan_info pl;
  Buffers bf;
  const yl_status st = ensure(h, batch, size, 0, &pl, &bf);   // the workspace only: nothing of a held forward is written
  if (st != YL_OK) return st;
  hipStream_t s = (hipStream_t)stream;
  const int M = pl.rows, F = h->cfg.channels, P = mode_of(mode);
  const HeadRows hw = head_rows(h->cfg, params, size * size);
  int nl = 1;
  if (!out) {
    const float* pw = params->block[site].pw;
    if (pass == YL_HEAD_PASS_FORWARD) {
      launch_gemm_in<true>(P, s, RowsScalar{pw, F}, RowsVec{a_dev, F}, OutRowsVec{out_dev, F}, F, M, F, F, 1);
    } else if (pass == YL_HEAD_PASS_DGRAD) {
      launch_gemm_in<true>(P, s, ColsScalar{pw, F}, RowsVec{a_dev, F}, OutRowsVec{out_dev, F}, F, M, F, F, 1);
    } else {
      HeadRows none;
      memset(&none, 0, sizeof(none));
      launch_gemm_in<true>(P, s, ColsScalar{a_dev, F}, ColsScalar{b_dev, F}, OutPartial{bf.wpart, (long)F * F}, F, F, M,
                           pl.wgrad_rows, pl.wgrad_splits);
      hipLaunchKernelGGL(yl_head_wsum_kernel, dim3(ceil_div((long)F * F, NT)), dim3(NT), 0, s, (const float*)bf.wpart,
                         pl.wgrad_splits, F, F, out_dev, none, 0);
      nl = 2;
    }
  } else if (pass == YL_HEAD_PASS_FORWARD) {
    out_forward(P, s, hw, a_dev, out_dev, M);
  } else if (pass == YL_HEAD_PASS_DGRAD) {
    out_dgrad(P, s, hw, a_dev, out_dev, M);
  } else {
    HeadRows gw = hw;                    // out_dev: the rows of box_w, obj_w, cls_w one after the other
    gw.box = out_dev; gw.obj = gw.box + (long)4 * hw.g.A * F; gw.cls = gw.obj + (long)hw.g.A * F;
    gw.box_b = gw.obj_b = gw.cls_b = nullptr;
    out_wgrad(P, s, hw.g, a_dev, b_dev, bf.wpart, gw, M, pl.ograd_rows, pl.ograd_splits);
    nl = 2;
  }
  if (launches) *launches = nl;
  return hipGetLastError() == hipSuccess ? YL_OK : YL_ERR_HIP;
}

}  // extern "C"
