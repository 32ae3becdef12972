// The reference's LossAF (scripts/loss/loss.py:283-436) on the device, fp32: the forward (validation loss and training
// criterion) and, further down, its backward.  Forward: three launches per batch, no host round trip, no floating-point
// atomics:
//   yl_loss_assign_kernel   one workgroup per ground-truth box: SimOTA candidate set, dynamic k, matches
//   yl_loss_reduce_kernel   one workgroup per image: positives (CIoU / cross-entropy / BCE), hard negatives
//   yl_loss_sum_kernel      one thread: the per-image parts added in image order
// Compiled with -ffp-contract=off: every + - * / is the IEEE fp32 operation torch performs, in its order, so the
// discrete choices (validity, dynamic k, the k smallest costs, conflicts) fall as they do in the reference.
//
// Assignment.  Of the [N anchors x G boxes] matrices of the reference only the VALID entries of a column matter:
// invalid IoUs are masked to 0 (they add nothing to the top-k sum) and invalid costs are 1e9 (never among the
// dynamic_k smallest: dynamic_k = max(int(sum of the k largest valid IoUs), 1) is at most the number of valid
// anchors, because every IoU is < 1 and orphan rescue guarantees one valid anchor -- torch's unspecified order
// among equal 1e9 entries is therefore never observed and not reproduced).  A workgroup walks its image's
// anchors level by level (a level outside the box's area gate is skipped whole), tests the centre mask on the
// decoded centre and appends the valid ones (anchor, cost, IoU) to a list in LDS.  The list is bounded: before
// it could overflow it is pruned to the entries that can still be selected (the topk_limit largest IoUs and the
// topk_limit smallest costs; top-k of a union = top-k of the parts' top-k).  Selection is by RANK -- entry e is
// among the k best iff fewer than k entries beat it under the total order (value, anchor index) -- so it does not
// depend on the order in which lanes appended.  Matches go into one 64-bit word per (image, anchor) with
// atomicMin on (order-preserving bits of cost) << 32 | box index: an integer minimum is independent of arrival
// order, it keeps the smallest cost and, on equal costs, the lowest box -- the reference's conflict argmin.
//
// Sums.  Every mean is accumulated in float64 in an order fixed by (anchor index, lane, wave) and rounded to fp32
// once; per-element terms are fp32.  Two runs on the same input are bitwise equal, and an image's parts do not
// depend on what else is in the batch.  The K largest negative-objectness terms are found by a 4 x 8-bit radix
// select on the float bits (all terms are >= 0): sum of the values above the K-th plus the K-th times its share.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "yl_internal.h"

namespace {

#define YL_LOSS_CAP 1024      // candidate list entries in LDS (>= 2 * YL_LOSS_MAX_TOPK + the 256 a tile can append)
#define YL_LOSS_RT 512        // threads of the reduce kernel
#define YL_LOSS_NOKEY 0xffffffffffffffffull

__device__ __forceinline__ float yl_sigm(float x) { return 1.0f / (1.0f + expf(-x)); }
// log_sigmoid form of BCEWithLogits: (1 - t) * x - (min(x, 0) - log1p(exp(-|x|)))
__device__ __forceinline__ float yl_bce(float x, float t) {
  return (1.0f - t) * x - (fminf(x, 0.0f) - log1pf(expf(-fabsf(x))));
}

struct YlAnchor {
  const float* row;
  float ax, ay, s;
};

__device__ __forceinline__ YlAnchor yl_anchor(const YlLevels& lv, int b, int n) {
  int l = 0;
  while (l + 1 < lv.L && n >= lv.off[l + 1]) ++l;
  const int S = lv.S[l], cell = n - lv.off[l];
  YlAnchor a;
  a.row = lv.ptr[l] + ((size_t)b * S * S + cell) * lv.E;
  a.ax = (float)(cell % S);
  a.ay = (float)(cell / S);
  a.s = lv.stride[l];
  return a;
}

// LossAF._decode (:258-276): train-time, unclamped
__device__ __forceinline__ void yl_loss_ctr(const YlAnchor& a, int cm, float& cx, float& cy) {
  const float sx = yl_sigm(a.row[0]), sy = yl_sigm(a.row[1]);
  if (cm == YL_CENTER_V8) {
    cx = (sx * 2.0f - 0.5f + a.ax) * a.s;
    cy = (sy * 2.0f - 0.5f + a.ay) * a.s;
  } else {
    cx = (sx + a.ax) * a.s;
    cy = (sy + a.ay) * a.s;
  }
}
__device__ __forceinline__ float yl_loss_side(float t, int wm, float s) {
  if (wm == YL_WH_V8) {
    const float q = yl_sigm(t) * 2.0f;
    return q * q * s;
  }
  if (wm == YL_WH_SOFTPLUS) return (t > 20.0f ? t : log1pf(expf(t))) * s;
  return expf(fminf(fmaxf(t, -10.0f), 8.0f)) * s;
}

struct YlGt {
  float x1, y1, x2, y2, cx, cy, w, h, area, larea, lar, rterm, cden, area2;
};
__device__ __forceinline__ YlGt yl_gt(const float* g) {
  YlGt q;
  q.x1 = g[0]; q.y1 = g[1]; q.x2 = g[2]; q.y2 = g[3];
  q.cx = (q.x1 + q.x2) * 0.5f;
  q.cy = (q.y1 + q.y2) * 0.5f;
  q.w = fmaxf(q.x2 - q.x1, 1.0f);
  q.h = fmaxf(q.y2 - q.y1, 1.0f);
  q.area = q.w * q.h;
  q.larea = logf(q.area);
  q.lar = logf(q.w / q.h);
  q.rterm = 0.10f * fmaxf(q.w, q.h);
  q.cden = q.w * q.w + q.h * q.h + 1e-6f;
  q.area2 = fmaxf(q.x2 - q.x1, 0.0f) * fmaxf(q.y2 - q.y1, 0.0f);
  return q;
}

// bbox_iou_matrix (:107)
__device__ __forceinline__ float yl_loss_iou(float x1, float y1, float x2, float y2, const YlGt& g) {
  const float iw = fmaxf(fminf(x2, g.x2) - fmaxf(x1, g.x1), 0.0f);
  const float ih = fmaxf(fminf(y2, g.y2) - fmaxf(y1, g.y1), 0.0f);
  const float inter = iw * ih;
  const float a1 = fmaxf(x2 - x1, 0.0f) * fmaxf(y2 - y1, 0.0f);
  return inter / (a1 + g.area2 - inter + 1e-7f);
}

// cost (:349-357) and IoU of a valid anchor; dist = squared centre distance already computed
__device__ __forceinline__ void yl_loss_cost(const YlAnchor& a, const yl_loss_cfg& c, const YlGt& g, int label, float cx,
                                             float cy, float dist, float& cost, float& iou) {
  const float w = yl_loss_side(a.row[2], c.wh_mode, a.s), h = yl_loss_side(a.row[3], c.wh_mode, a.s);
  iou = yl_loss_iou(cx - 0.5f * w, cy - 0.5f * h, cx + 0.5f * w, cy + 0.5f * h, g);
  const float cls_cost = 1.0f - yl_sigm(a.row[5 + label]);
  const float obj_cost = -yl_sigm(a.row[4]);
  const float dl = fabsf(logf(w * h) - g.larea);
  const float size_cost = dl / (1.0f + dl);
  const float da = fabsf(logf(w / h) - g.lar);
  const float ar_cost = da / (1.0f + da);
  const float cn = dist / g.cden;
  cost = c.iou_cost_w * (1.0f - iou) + c.assign_cls_weight * cls_cost + obj_cost + c.center_cost_w * cn +
         c.size_prior_w * size_cost + c.ar_prior_w * ar_cost;
}

// unsigned image of a float that sorts like the float (costs can be negative: obj_cost = -sigmoid).  A NaN cost
// (degenerate predictions: a zero or infinite side) sorts above every number, as in torch.topk.
__device__ __forceinline__ unsigned yl_ord(float f) {
  if (f != f) return 0xffffffffu;
  const unsigned u = __float_as_uint(f + 0.0f);          // -0 -> +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// e beats f under (larger IoU, lower anchor) / (smaller cost, lower anchor)
__device__ __forceinline__ int yl_rank_iou(const float* v, const int* idx, int n, int e) {
  const float ve = v[e];
  const int ie = idx[e];
  int r = 0;
  for (int f = 0; f < n; ++f) r += (v[f] > ve || (v[f] == ve && idx[f] < ie)) ? 1 : 0;
  return r;
}
__device__ __forceinline__ int yl_rank_cost(const float* v, const int* idx, int n, int e) {
  const unsigned ve = yl_ord(v[e]);
  const int ie = idx[e];
  int r = 0;
  for (int f = 0; f < n; ++f) {
    const unsigned vf = yl_ord(v[f]);
    r += (vf < ve || (vf == ve && idx[f] < ie)) ? 1 : 0;
  }
  return r;
}

__global__ __launch_bounds__(256) void yl_loss_assign_kernel(YlLevels lv, YlLossP p) {
  __shared__ int s_idx[YL_LOSS_CAP];
  __shared__ float s_cost[YL_LOSS_CAP];
  __shared__ float s_iou[YL_LOSS_CAP];
  __shared__ unsigned char s_keep[YL_LOSS_CAP];
  __shared__ float s_top[YL_LOSS_MAX_TOPK];
  __shared__ float s_rv[4];
  __shared__ int s_ri[4];
  __shared__ int s_n, s_total, s_dk;
  const int tid = threadIdx.x, t = blockIdx.x;
  const yl_loss_cfg& c = p.cfg;
  // image of box t: the last b with gt_off[b] <= t (images without boxes own no row)
  int lo = 0, hi = p.B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p.off[mid] <= t) lo = mid; else hi = mid - 1;
  }
  const int b = lo;
  const YlGt g = yl_gt(p.gt + 4 * (size_t)t);
  const int label = min(max(p.label[t], 0), lv.C - 1);
  const int kk = min(c.topk_limit, lv.N);
  if (tid == 0) { s_n = 0; s_total = 0; }
  if (tid < YL_LOSS_MAX_TOPK) s_top[tid] = 0.0f;

  for (int l = 0; l < lv.L; ++l) {
    const float s = lv.stride[l];
    const float cells = g.area / (s * s);
    if (!(cells >= p.area_min && cells <= p.area_max)) continue;           // level gate: the same for every lane
    const float r = fmaxf(c.center_radius_cells * s + g.rterm, 15.0f);
    const float r2 = r * r;
    const int S = lv.S[l], S2 = S * S;
    for (int base = 0; base < S2; base += 256) {
      __syncthreads();
      const int n = s_n;
      __syncthreads();                                   // every lane has read the count before any lane appends
      if (n + 256 > YL_LOSS_CAP) {
        // prune to the entries a later selection can still pick
        for (int e = tid; e < n; e += 256)
          s_keep[e] = (yl_rank_iou(s_iou, s_idx, n, e) < kk || yl_rank_cost(s_cost, s_idx, n, e) < kk) ? 1 : 0;
        __syncthreads();
        if (tid == 0) {
          int m = 0;
          for (int e = 0; e < n; ++e)
            if (s_keep[e]) { s_idx[m] = s_idx[e]; s_cost[m] = s_cost[e]; s_iou[m] = s_iou[e]; ++m; }
          s_n = m;
        }
        __syncthreads();
      }
      const int cell = base + tid;
      if (cell < S2) {
        YlAnchor a;
        a.row = lv.ptr[l] + ((size_t)b * S2 + cell) * lv.E;
        a.ax = (float)(cell % S); a.ay = (float)(cell / S); a.s = s;
        float cx, cy;
        yl_loss_ctr(a, c.center_mode, cx, cy);
        const float dx = cx - g.cx, dy = cy - g.cy;
        const float dist = dx * dx + dy * dy;
        if (dist <= r2) {
          float cost, iou;
          yl_loss_cost(a, c, g, label, cx, cy, dist, cost, iou);
          const int slot = atomicAdd(&s_n, 1);                             // < YL_LOSS_CAP by the check above
          s_idx[slot] = lv.off[l] + cell; s_cost[slot] = cost; s_iou[slot] = iou;
          atomicAdd(&s_total, 1);
        }
      }
    }
  }
  __syncthreads();
  if (s_total == 0) {
    // orphan rescue (:333-338): the anchor with the smallest centre distance over ALL levels, first index on ties
    float bd = INFINITY;
    int bi = 0x7fffffff;
    for (int n = tid; n < lv.N; n += 256) {
      const YlAnchor a = yl_anchor(lv, b, n);
      float cx, cy;
      yl_loss_ctr(a, c.center_mode, cx, cy);
      const float dx = cx - g.cx, dy = cy - g.cy;
      const float d = dx * dx + dy * dy;
      if (d < bd || (d == bd && n < bi)) { bd = d; bi = n; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float od = __shfl_xor(bd, m, 64);
      const int oi = __shfl_xor(bi, m, 64);
      if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    if ((tid & 63) == 0) { s_rv[tid >> 6] = bd; s_ri[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 4; ++w)
        if (s_rv[w] < bd || (s_rv[w] == bd && s_ri[w] < bi)) { bd = s_rv[w]; bi = s_ri[w]; }
      if (bi < lv.N) {                                                      // (every distance NaN: no match)
        const YlAnchor a = yl_anchor(lv, b, bi);
        float cx, cy, cost, iou;
        yl_loss_ctr(a, c.center_mode, cx, cy);
        yl_loss_cost(a, c, g, label, cx, cy, bd, cost, iou);
        s_idx[0] = bi; s_cost[0] = cost; s_iou[0] = iou;
        s_n = 1;
      }
    }
    __syncthreads();
  }
  const int n = s_n;
  // dynamic k (:362-364): the kk largest valid IoUs, summed in descending order as topk(...).sum() sees them
  for (int e = tid; e < n; e += 256) {
    const int r = yl_rank_iou(s_iou, s_idx, n, e);
    if (r < kk) s_top[r] = s_iou[e];
  }
  __syncthreads();
  if (tid == 0) {
    float sum = 0.0f;
    for (int i = 0; i < kk; ++i) sum += s_top[i];
    s_dk = (int)fminf(fmaxf(sum, 1.0f), (float)kk);                         // .int() truncates; clamp(min=1)
  }
  __syncthreads();
  const int dk = s_dk;
  for (int e = tid; e < n; e += 256)
    if (yl_rank_cost(s_cost, s_idx, n, e) < dk)
      atomicMin(p.keys + (size_t)b * lv.N + s_idx[e], ((unsigned long long)yl_ord(s_cost[e]) << 32) | (unsigned)t);
}

// bbox_ciou_flat (:130)
__device__ __forceinline__ float yl_loss_ciou(float px1, float py1, float px2, float py2, const YlGt& g) {
  const float eps = 1e-7f;
  const float pw = fmaxf(px2 - px1, eps), ph = fmaxf(py2 - py1, eps);
  const float tw = fmaxf(g.x2 - g.x1, eps), th = fmaxf(g.y2 - g.y1, eps);
  const float iw = fmaxf(fminf(px2, g.x2) - fmaxf(px1, g.x1), 0.0f);
  const float ih = fmaxf(fminf(py2, g.y2) - fmaxf(py1, g.y1), 0.0f);
  const float inter = iw * ih;
  const float iou = inter / (pw * ph + tw * th - inter + eps);
  const float dx = (px1 + px2) * 0.5f - (g.x1 + g.x2) * 0.5f, dy = (py1 + py2) * 0.5f - (g.y1 + g.y2) * 0.5f;
  const float cd = dx * dx + dy * dy;
  const float cw = fmaxf(px2, g.x2) - fminf(px1, g.x1), ch = fmaxf(py2, g.y2) - fminf(py1, g.y1);
  const float c2 = cw * cw + ch * ch + eps;
  const float d = atanf(tw / th) - atanf(pw / ph);
  const float v = 0.40528473456935108577551785283891f * (d * d);           // 4 / pi^2
  const float alpha = v / (v - iou + 1.0f + eps);
  return iou - cd / c2 - alpha * v;
}

// block sum in a fixed order: xor butterfly inside a wave (commutative pairs: every lane gets the same bits), then
// the waves in index order.  Every thread returns the total.
__device__ __forceinline__ double yl_block_sum(double v, double* s_w, int tid) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  __syncthreads();
  if ((tid & 63) == 0) s_w[tid >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < YL_LOSS_RT / 64; ++w) t += s_w[w];
  return t;
}
__device__ __forceinline__ int yl_block_isum(int v, int* s_w, int tid) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  __syncthreads();
  if ((tid & 63) == 0) s_w[tid >> 6] = v;
  __syncthreads();
  int t = 0;
  for (int w = 0; w < YL_LOSS_RT / 64; ++w) t += s_w[w];
  return t;
}

__global__ __launch_bounds__(YL_LOSS_RT) void yl_loss_reduce_kernel(YlLevels lv, YlLossP p) {
  __shared__ double s_wd[YL_LOSS_RT / 64];
  __shared__ int s_wi[YL_LOSS_RT / 64];
  __shared__ int s_hist[256];
  __shared__ unsigned s_prefix;
  __shared__ int s_need, s_cut;
  const int tid = threadIdx.x, b = blockIdx.x, N = lv.N;
  const yl_loss_cfg& c = p.cfg;
  const unsigned long long* keys = p.keys + (size_t)b * N;
  float* negv = p.negv + (size_t)b * N;
  double sb = 0.0, sc = 0.0, so = 0.0;
  int cnt = 0;
  for (int n = tid; n < N; n += YL_LOSS_RT) {
    const unsigned long long key = keys[n];
    const YlAnchor a = yl_anchor(lv, b, n);
    const float xo = a.row[4];
    if (key == YL_LOSS_NOKEY) {
      negv[n] = yl_bce(xo, 0.0f);
      if (p.assign) p.assign[(size_t)b * N + n] = -1;
      continue;
    }
    const int t = (int)(unsigned)(key & 0xffffffffull);
    negv[n] = -1.0f;                                     // not a negative (every real term is >= 0)
    if (p.assign) p.assign[(size_t)b * N + n] = t;
    const YlGt g = yl_gt(p.gt + 4 * (size_t)t);
    float cx, cy;
    yl_loss_ctr(a, c.center_mode, cx, cy);
    const float w = yl_loss_side(a.row[2], c.wh_mode, a.s), h = yl_loss_side(a.row[3], c.wh_mode, a.s);
    const float x1 = cx - 0.5f * w, y1 = cy - 0.5f * h, x2 = cx + 0.5f * w, y2 = cy + 0.5f * h;
    sb += (double)(1.0f - yl_loss_ciou(x1, y1, x2, y2, g));
    const float tgt = fminf(fmaxf(yl_loss_iou(x1, y1, x2, y2, g), 0.0f), 1.0f);
    so += (double)yl_bce(xo, tgt);
    if (lv.C > 1) {
      // CrossEntropyLoss(label_smoothing = e): (1 - e) * -logp[y] + e * mean_c(-logp[c])
      const int label = min(max(p.label[t], 0), lv.C - 1);
      const float* z = a.row + 5;
      float m = z[0];
      for (int k = 1; k < lv.C; ++k) m = fmaxf(m, z[k]);
      float se = 0.0f;
      for (int k = 0; k < lv.C; ++k) se += expf(z[k] - m);
      const float lse = logf(se);
      float sl = 0.0f;
      for (int k = 0; k < lv.C; ++k) sl += (z[k] - m) - lse;
      const float nll = -((z[label] - m) - lse);
      sc += (double)((1.0f - c.cls_smoothing) * nll + c.cls_smoothing * (-sl / (float)lv.C));
    }
    ++cnt;
  }
  sb = yl_block_sum(sb, s_wd, tid);
  sc = yl_block_sum(sc, s_wd, tid);
  so = yl_block_sum(so, s_wd, tid);
  const int npos = yl_block_isum(cnt, s_wi, tid);
  const int nneg = N - npos;
  const int K = min(max(64, 3 * npos), nneg);
  double negmean = 0.0;
  unsigned kthbits = 0u;
  int cut = 0;
  if (K > 0) {
    // the K-th largest term by radix select, most significant byte first; negv was written by this workgroup
    if (tid == 0) { s_prefix = 0u; s_need = K; }
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      if (tid < 256) s_hist[tid] = 0;
      __syncthreads();
      const unsigned prefix = s_prefix;
      const unsigned himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
      for (int n = tid; n < N; n += YL_LOSS_RT) {
        const unsigned u = __float_as_uint(negv[n]);
        if (!(u & 0x80000000u) && (u & himask) == prefix) atomicAdd(&s_hist[(u >> shift) & 255u], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int need = s_need, bin = 255;
        for (; bin > 0; --bin) {
          if (s_hist[bin] >= need) break;
          need -= s_hist[bin];
        }
        s_need = need;                                   // entries still to take from this bin
        s_prefix = prefix | ((unsigned)bin << shift);
      }
      __syncthreads();
    }
    const unsigned kth = s_prefix;                       // bits of the K-th largest term; s_need copies of it are taken
    kthbits = kth;
    double sg = 0.0;
    for (int n = tid; n < N; n += YL_LOSS_RT) {
      const unsigned u = __float_as_uint(negv[n]);
      if (!(u & 0x80000000u) && u > kth) sg += (double)negv[n];
    }
    sg = yl_block_sum(sg, s_wd, tid);
    negmean = (sg + (double)s_need * (double)__uint_as_float(kth)) / (double)K;
    if (p.sel) {
      // state for the backward only: which of the entries equal to the K-th term are the s_need selected ones -- the
      // lowest anchor indices.  One ordered pass: count per chunk of YL_LOSS_RT anchors; inside the chunk where the
      // running count reaches s_need, a ballot prefix finds the anchor that completes it.
      const int need = s_need;
      if (tid == 0) s_cut = N;
      int run = 0;
      for (int base = 0; base < N; base += YL_LOSS_RT) {
        const int n = base + tid;
        const int eq = (n < N && __float_as_uint(negv[n]) == kth) ? 1 : 0;
        const unsigned long long bal = __ballot(eq);
        const int below = __popcll(bal & ((1ull << (tid & 63)) - 1ull));
        const int cnt = yl_block_isum(eq, s_wi, tid);     // leaves the per-wave counts in s_wi
        if (run + cnt >= need) {                          // the same for every thread
          int before = run;
          for (int w = 0; w < (tid >> 6); ++w) before += s_wi[w];
          if (eq && before + below + 1 == need) s_cut = n + 1;
          break;
        }
        run += cnt;
      }
      __syncthreads();
      cut = s_cut;
    }
  }
  if (p.sel && tid == 0) {
    int* sel = p.sel + 4 * b;
    sel[0] = npos; sel[1] = K; sel[2] = (int)kthbits; sel[3] = cut;
  }
  if (tid == 0) {
    float box = 0.0f, obj, cls = 0.0f;
    if (npos > 0) {
      box = c.lambda_box * (float)(sb / (double)npos);
      if (lv.C > 1) cls = c.lambda_cls * (float)(sc / (double)npos);
      obj = c.lambda_obj * ((float)(so / (double)npos) + (float)negmean);
    } else {
      obj = c.lambda_obj * (float)negmean;
    }
    p.per_image[3 * b] = box; p.per_image[3 * b + 1] = obj; p.per_image[3 * b + 2] = cls;
    p.has_pos[b] = npos > 0 ? 1 : 0;
  }
}

__global__ void yl_loss_sum_kernel(YlLossP p) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float box = 0.0f, obj = 0.0f, cls = 0.0f;
  int np = 0;
  for (int b = 0; b < p.B; ++b) {
    box += p.per_image[3 * b]; obj += p.per_image[3 * b + 1]; cls += p.per_image[3 * b + 2];
    np += p.has_pos[b];
  }
  p.out4[0] = box; p.out4[1] = obj; p.out4[2] = cls;
  p.out4[3] = (float)((double)np / (double)p.B);
}

// ---- backward ------------------------------------------------------------------------------------------------
// d(box + obj + cls)/d(level tensors), closed-form per anchor from the forward's state (assign, sel): see the header
// for the semantics.  The gradient is as large as the level tensors and all but a few hundred rows per image are
// zero, so the kernel is a streaming write: a workgroup owns YL_LOSS_GR consecutive rows of one level tensor (a
// contiguous, 16-byte aligned range of YL_LOSS_GR * E floats) and
//   1. one thread per row reads assign / sel, decides a negative with the forward's own yl_bce bits, and puts the
//      row's columns 0-4 into LDS; a positive recomputes decode, IoU and the CIoU derivative from its logits;
//   2. one wave per positive row reduces the class logits to max + log-sum-exp;
//   3. all threads write the range once with 16-byte stores: columns 0-4 from LDS, the class columns of positives
//      from softmax, +0.0 everywhere else.  Nothing is read back, no element has two writers, no atomics.
// The few non-zero rows are evaluated in float64 from the fp32 logits (quantities of the ground truth alone stay
// fp32, as the reference's fp32 targets make them in its own float64 run) and rounded once.
#define YL_LOSS_GR 128        // rows per workgroup of the gradient kernel (64 / 128 / 256 measured: DESIGN 7c')
#define YL_LOSS_GT 256        // its threads

__device__ __forceinline__ double yl_dsigm(double x) { return 1.0 / (1.0 + exp(-x)); }
// derivative of max(a, b) with respect to a (of min(b, a) with respect to b): torch splits a tie
__device__ __forceinline__ double yl_dstep(double a, double b) { return a > b ? 1.0 : (a == b ? 0.5 : 0.0); }

// centre / side of the train-time decode with its derivative by the logit
__device__ __forceinline__ void yl_grad_ctr(double t, int cm, double a, double s, double& c, double& dc) {
  const double q = yl_dsigm(t);
  if (cm == YL_CENTER_V8) { c = (q * 2.0 - 0.5 + a) * s; dc = 2.0 * q * (1.0 - q) * s; }
  else { c = (q + a) * s; dc = q * (1.0 - q) * s; }
}
__device__ __forceinline__ void yl_grad_side(double t, int wm, double s, double& w, double& dw) {
  if (wm == YL_WH_V8) {
    const double q = yl_dsigm(t);
    w = (2.0 * q) * (2.0 * q) * s;
    dw = 2.0 * (2.0 * q) * 2.0 * q * (1.0 - q) * s;
  } else if (wm == YL_WH_SOFTPLUS) {
    w = (t > 20.0 ? t : log1p(exp(t))) * s;
    dw = (t > 20.0 ? 1.0 : yl_dsigm(t)) * s;
  } else {
    w = exp(fmin(fmax(t, -10.0), 8.0)) * s;
    dw = (t >= -10.0 && t <= 8.0) ? w : 0.0;              // clamp passes the gradient at its boundary, none outside
  }
}

// d(1 - CIoU)/d(x1, y1, x2, y2) of bbox_ciou_flat (:130); alpha is a constant (the reference's no_grad)
__device__ __forceinline__ void yl_ciou_grad(double x1, double y1, double x2, double y2, const YlGt& g, double* gr) {
  const double eps = 1e-7;
  const double gx1 = g.x1, gy1 = g.y1, gx2 = g.x2, gy2 = g.y2;
  const double wr = x2 - x1, hr = y2 - y1;
  const double pw = fmax(wr, eps), ph = fmax(hr, eps);
  const double mw = wr >= eps ? 1.0 : 0.0, mh = hr >= eps ? 1.0 : 0.0;
  const float twf = fmaxf(g.x2 - g.x1, 1e-7f), thf = fmaxf(g.y2 - g.y1, 1e-7f);
  const double tarea = (double)(twf * thf), tatan = (double)atanf(twf / thf);
  const double iwr = fmin(x2, gx2) - fmax(x1, gx1), ihr = fmin(y2, gy2) - fmax(y1, gy1);
  const double iw = fmax(iwr, 0.0), ih = fmax(ihr, 0.0);
  const double miw = iwr >= 0.0 ? 1.0 : 0.0, mih = ihr >= 0.0 ? 1.0 : 0.0;
  // derivatives by (x1, y1, x2, y2)
  const double d_iw[4] = {-miw * yl_dstep(x1, gx1), 0.0, miw * yl_dstep(gx2, x2), 0.0};
  const double d_ih[4] = {0.0, -mih * yl_dstep(y1, gy1), 0.0, mih * yl_dstep(gy2, y2)};
  const double d_pw[4] = {-mw, 0.0, mw, 0.0}, d_ph[4] = {0.0, -mh, 0.0, mh};
  const double inter = iw * ih;
  const double uni = pw * ph + tarea - inter + eps;
  const double iou = inter / uni;
  const double dx = (x1 + x2) * 0.5 - (double)g.cx, dy = (y1 + y2) * 0.5 - (double)g.cy;
  const double cd = dx * dx + dy * dy;
  const double d_cd[4] = {dx, dy, dx, dy};
  const double cw = fmax(x2, gx2) - fmin(x1, gx1), ch = fmax(y2, gy2) - fmin(y1, gy1);
  const double d_cw[4] = {-yl_dstep(gx1, x1), 0.0, yl_dstep(x2, gx2), 0.0};
  const double d_ch[4] = {0.0, -yl_dstep(gy1, y1), 0.0, yl_dstep(y2, gy2)};
  const double c2 = cw * cw + ch * ch + eps;
  const double k4 = 0.40528473456935108577551785283891;                   // 4 / pi^2
  const double d = tatan - atan(pw / ph);
  const double v = k4 * (d * d);
  const double alpha = v / (v - iou + 1.0 + eps);
  const double den = pw * pw + ph * ph;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double dinter = d_iw[k] * ih + iw * d_ih[k];
    const double duni = d_pw[k] * ph + pw * d_ph[k] - dinter;
    const double diou = (dinter * uni - inter * duni) / (uni * uni);
    const double dc2 = 2.0 * cw * d_cw[k] + 2.0 * ch * d_ch[k];
    const double dpen = (d_cd[k] * c2 - cd * dc2) / (c2 * c2);
    const double dd = (-ph * d_pw[k] + pw * d_ph[k]) / den;              // d(-atan(pw / ph))
    gr[k] = -(diou - dpen - alpha * (2.0 * k4 * d * dd));
  }
}

__global__ __launch_bounds__(YL_LOSS_GT) void yl_loss_grad_kernel(YlLevels lv, YlLossGradP p) {
  __shared__ float s_g[YL_LOSS_GR][5];        // columns 0-4 of the tile's rows
  __shared__ int s_label[YL_LOSS_GR];         // class of a positive row's box, -1 for every other row
  __shared__ double s_lse[YL_LOSS_GR];        // max + log-sum-exp of a positive row's class logits
  __shared__ double s_scale[YL_LOSS_GR];      // grad_out * lambda_cls / npos of a positive row
  const int tid = threadIdx.x, E = lv.E, C = lv.C;
  const yl_loss_cfg& c = p.cfg;
  // level and tile of this workgroup: tiles are numbered level by level
  int l = 0, tile = blockIdx.x;
  for (;;) {
    const int nt = (int)(((long long)p.B * lv.S[l] * lv.S[l] + YL_LOSS_GR - 1) / YL_LOSS_GR);
    if (tile < nt || l + 1 >= lv.L) break;
    tile -= nt; ++l;
  }
  const int S = lv.S[l], S2 = S * S;
  const long long rows = (long long)p.B * S2, row0 = (long long)tile * YL_LOSS_GR;
  const int nr = (int)(rows - row0 < YL_LOSS_GR ? rows - row0 : YL_LOSS_GR);
  if (nr <= 0) return;
  const float* in = lv.ptr[l] + row0 * E;
  float* out = p.out[l] + row0 * E;

  if (tid < nr) {
    const long long r = row0 + tid;
    const int b = (int)(r / S2), cell = (int)(r - (long long)b * S2), n = lv.off[l] + cell;
    const float* row = in + (size_t)tid * E;
    const int* sel = p.sel + 4 * b;
    const int npos = sel[0], K = sel[1], cut = sel[3];
    const unsigned kth = (unsigned)sel[2];
    const int t = p.assign[(size_t)b * lv.N + n];
    const float xo = row[4];                                                // both kinds of row need it: no load waits for `t`
    const double go = (double)p.gout[0];
    double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0, g4 = 0.0;
    int label = -1;
    if (t < 0) {
      const unsigned u = __float_as_uint(yl_bce(xo, 0.0f));                 // the bits the forward's radix select saw
      if (K > 0 && !(u & 0x80000000u) && (u > kth || (u == kth && n < cut)))
        g4 = go * (double)c.lambda_obj / (double)K * yl_dsigm((double)xo);
    } else {
      const YlGt g = yl_gt(p.gt + 4 * (size_t)t);
      const double s = (double)lv.stride[l];
      double cx, cy, w, h, dcx, dcy, dw, dh, gr[4];
      yl_grad_ctr((double)row[0], c.center_mode, (double)(cell % S), s, cx, dcx);
      yl_grad_ctr((double)row[1], c.center_mode, (double)(cell / S), s, cy, dcy);
      yl_grad_side((double)row[2], c.wh_mode, s, w, dw);
      yl_grad_side((double)row[3], c.wh_mode, s, h, dh);
      const double x1 = cx - 0.5 * w, y1 = cy - 0.5 * h, x2 = cx + 0.5 * w, y2 = cy + 0.5 * h;
      yl_ciou_grad(x1, y1, x2, y2, g, gr);
      const double sb = go * (double)c.lambda_box / (double)npos;
      g0 = sb * (gr[0] + gr[2]) * dcx;
      g1 = sb * (gr[1] + gr[3]) * dcy;
      g2 = sb * 0.5 * (gr[2] - gr[0]) * dw;
      g3 = sb * 0.5 * (gr[3] - gr[1]) * dh;
      // objectness against the detached clamp(IoU, 0, 1) of bbox_iou_matrix (:107)
      const double iw = fmax(fmin(x2, (double)g.x2) - fmax(x1, (double)g.x1), 0.0);
      const double ih = fmax(fmin(y2, (double)g.y2) - fmax(y1, (double)g.y1), 0.0);
      const double inter = iw * ih;
      const double a1 = fmax(x2 - x1, 0.0) * fmax(y2 - y1, 0.0);
      const double tgt = fmin(fmax(inter / (a1 + (double)g.area2 - inter + 1e-7), 0.0), 1.0);
      g4 = go * (double)c.lambda_obj / (double)npos * (yl_dsigm((double)xo) - tgt);
      if (C > 1) {
        label = min(max(p.label[t], 0), C - 1);
        s_scale[tid] = go * (double)c.lambda_cls / (double)npos;
      }
    }
    // x + 0.0f: a product that came out as -0.0 is stored as +0.0
    s_g[tid][0] = (float)g0 + 0.0f; s_g[tid][1] = (float)g1 + 0.0f; s_g[tid][2] = (float)g2 + 0.0f;
    s_g[tid][3] = (float)g3 + 0.0f; s_g[tid][4] = (float)g4 + 0.0f;
    s_label[tid] = label;
  }
  __syncthreads();
  // max + log-sum-exp of the positive rows' class logits: wave w takes rows w, w + 4, ...
  for (int r = tid >> 6; r < nr; r += YL_LOSS_GT / 64) {
    if (s_label[r] < 0) continue;                                           // the same for the whole wave
    const float* z = in + (size_t)r * E + 5;
    const int lane = tid & 63;
    double m = -INFINITY;
    for (int k = lane; k < C; k += 64) m = fmax(m, (double)z[k]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    double se = 0.0;
    for (int k = lane; k < C; k += 64) se += exp((double)z[k] - m);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) se += __shfl_xor(se, o, 64);         // commutative pairs: the same bits in every lane
    if (lane == 0) s_lse[r] = m + log(se);
  }
  __syncthreads();

  const int total = nr * E;                                                 // floats of this tile
  const double e = (double)c.cls_smoothing;
  const double tg_other = e / (double)C, tg_label = (1.0 - e) + e / (double)C;
  auto value = [&](int r, int col, int idx) -> float {
    if (col < 5) return s_g[r][col];
    const int label = s_label[r];
    if (label < 0 || col >= 5 + C) return 0.0f;
    const double pr = exp((double)in[idx] - s_lse[r]);
    return (float)(s_scale[r] * (pr - (col - 5 == label ? tg_label : tg_other))) + 0.0f;
  };
  const bool vec = (((uintptr_t)out) & 15u) == 0;                           // the tile's byte offset is a multiple of 256
  const int nvec = vec ? total >> 2 : 0;
  for (int i = tid; i < nvec; i += YL_LOSS_GT) {
    const int idx = 4 * i;
    int r = idx / E, col = idx - r * E;
    float q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      q[j] = value(r, col, idx + j);
      if (++col == E) { col = 0; ++r; }
    }
    *reinterpret_cast<float4*>(out + idx) = make_float4(q[0], q[1], q[2], q[3]);
  }
  for (int idx = 4 * nvec + tid; idx < total; idx += YL_LOSS_GT) {          // a last partial tile's tail (or an unaligned base)
    const int r = idx / E;
    out[idx] = value(r, idx - r * E, idx);
  }
}

}  // namespace

hipError_t yl_launch_loss_af(const YlLevels& lv, const YlLossP& p, hipStream_t st) {
  hipError_t e = hipMemsetAsync(p.keys, 0xff, (size_t)p.B * lv.N * sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  if (p.T > 0) hipLaunchKernelGGL(yl_loss_assign_kernel, dim3(p.T), dim3(256), 0, st, lv, p);
  hipLaunchKernelGGL(yl_loss_reduce_kernel, dim3(p.B), dim3(YL_LOSS_RT), 0, st, lv, p);
  hipLaunchKernelGGL(yl_loss_sum_kernel, dim3(1), dim3(64), 0, st, p);
  return hipGetLastError();
}

hipError_t yl_launch_loss_af_grad(const YlLevels& lv, const YlLossGradP& p, hipStream_t st) {
  long long tiles = 0;
  for (int l = 0; l < lv.L; ++l) tiles += ((long long)p.B * lv.S[l] * lv.S[l] + YL_LOSS_GR - 1) / YL_LOSS_GR;
  if (tiles <= 0 || tiles > 0x7fffffffll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(yl_loss_grad_kernel, dim3((unsigned)tiles), dim3(YL_LOSS_GT), 0, st, lv, p);
  return hipGetLastError();
}
