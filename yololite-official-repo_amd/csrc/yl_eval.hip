// Evaluate-path consumers on the device: the O(detections x ground truths)
// greedy matching loops of the reference's evaluation.
//   yl_eval_match      <- build_curves_from_coco     scripts/data/p_r_f1.py:31-78, :100-118  (float64)
//   yl_eval_sweep      <- its 0..1 confidence sweep  scripts/data/p_r_f1.py:96-124
//   yl_eval_confusion  <- create_confusion_matrix    scripts/helpers/evaluate.py:23-57, :96-153 (float32)
//   yl_eval_coco_match      <- COCOeval.evaluateImg  (pycocotools 2.0, iouType="bbox"; the reference calls it from
//   yl_eval_coco_accumulate <- COCOeval.accumulate    _coco_eval_from_lists, scripts/helpers/helpers.py:155-227) (float64)
// Compiled with -ffp-contract=off: every + - * / is the IEEE operation the reference's python / numpy
// arithmetic performs, in the same order, so the match decisions are bit-identical.
//
// Work decomposition: the matching of one key (image, category) -- or one image for the confusion
// matrix -- is inherently sequential over its score-ordered detections, and independent of every other
// key.  One 64-lane wave owns a key: detections in order, lanes across the ground truths (strided when
// there are more than 64), a butterfly reduction for (max IoU, first index).  The matched flag of a
// ground truth is written by the lane that will read it again (lane = index & 63): no fences.  The
// kernels are latency-bound integer/compare work on a few KB per key; they exist so the evaluation
// loop never leaves the device, not to fill the machine.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/yololite_hip.h"

namespace {

// ---- (max value, min index) butterfly over the 64 lanes; every lane ends with the result
template <typename T>
__device__ __forceinline__ void yl_wave_argmax(T& v, int& j) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const T ov = __shfl_xor(v, m, 64);
    const int oj = __shfl_xor(j, m, 64);
    if (ov > v || (ov == v && oj < j)) { v = ov; j = oj; }
  }
}

// iou_xywh, p_r_f1.py:31-41 (python floats = IEEE double)
__device__ __forceinline__ double yl_iou_xywh(double ax, double ay, double aw, double ah, double bx, double by,
                                              double bw, double bh) {
  const double ax2 = ax + aw, ay2 = ay + ah;
  const double bx2 = bx + bw, by2 = by + bh;
  const double ix1 = fmax(ax, bx), iy1 = fmax(ay, by);
  const double ix2 = fmin(ax2, bx2), iy2 = fmin(ay2, by2);
  const double iw = fmax(0.0, ix2 - ix1), ih = fmax(0.0, iy2 - iy1);
  const double inter = iw * ih;
  const double ua = fmax(0.0, aw * ah) + fmax(0.0, bw * bh) - inter;
  return ua > 0.0 ? inter / ua : 0.0;
}

__global__ __launch_bounds__(256) void yl_eval_match_kernel(const double* __restrict__ det,
                                                            const int* __restrict__ det_off,
                                                            const double* __restrict__ gt,
                                                            const int* __restrict__ gt_off, int num_keys, double thr,
                                                            uint8_t* __restrict__ tp, int* __restrict__ match,
                                                            uint8_t* gt_matched) {
  const int lane = threadIdx.x & 63;
  const int key = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (key >= num_keys) return;
  const int d0 = det_off[key], d1 = det_off[key + 1];
  const int g0 = gt_off[key], ng = gt_off[key + 1] - g0;
  for (int d = d0; d < d1; ++d) {
    const double ax = det[4 * (size_t)d], ay = det[4 * (size_t)d + 1];
    const double aw = det[4 * (size_t)d + 2], ah = det[4 * (size_t)d + 3];
    double best = 0.0;                 // p_r_f1.py:67 -- only an IoU strictly above 0 can be "best"
    int bj = 0x7fffffff;
    for (int j = lane; j < ng; j += 64) {
      if (gt_matched[g0 + j]) continue;
      const double* g = gt + 4 * (size_t)(g0 + j);
      const double v = yl_iou_xywh(ax, ay, aw, ah, g[0], g[1], g[2], g[3]);
      if (v > best) { best = v; bj = j; }       // strict: the first index keeps a tie (:72-73)
    }
    yl_wave_argmax(best, bj);
    const bool hit = bj != 0x7fffffff && best >= thr;          // :74
    if (hit && lane == (bj & 63)) gt_matched[g0 + bj] = 1;
    if (lane == 0) {
      tp[d] = hit ? 1 : 0;
      if (match) match[d] = hit ? bj : -1;
    }
  }
}

// histogram of the tp / fp flags over the threshold bins: bin(s) = largest k with thr[k] <= s
__global__ void yl_eval_hist_kernel(const double* __restrict__ score, const uint8_t* __restrict__ tp,
                                    const uint8_t* __restrict__ counted, int n, const double* __restrict__ thr,
                                    int steps, int* tp_hist, int* fp_hist) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (counted && !counted[i]) return;
  const double s = score[i];
  int lo = 0, hi = steps;              // first index with thr[idx] > s   (score >= thr, p_r_f1.py:104)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (thr[mid] <= s) lo = mid + 1; else hi = mid;
  }
  if (lo == 0) return;                 // below every threshold (or NaN): never counted
  atomicAdd(tp[i] ? &tp_hist[lo - 1] : &fp_hist[lo - 1], 1);
}

// in-place suffix sums of both histograms (steps is a few hundred: one block, serial tail is fine)
__global__ void yl_eval_suffix_kernel(int* tp_hist, int* fp_hist, int steps) {
  if (threadIdx.x == 0) {
    int a = 0;
    for (int k = steps - 1; k >= 0; --k) { a += tp_hist[k]; tp_hist[k] = a; }
  } else if (threadIdx.x == 64) {
    int a = 0;
    for (int k = steps - 1; k >= 0; --k) { a += fp_hist[k]; fp_hist[k] = a; }
  }
}

// iou_matrix, evaluate.py:27-57 (numpy float32)
__device__ __forceinline__ float yl_iou_xyxy_f32(const float* a, const float* b) {
  const float ix1 = fmaxf(a[0], b[0]), iy1 = fmaxf(a[1], b[1]);
  const float ix2 = fminf(a[2], b[2]), iy2 = fminf(a[3], b[3]);
  const float iw = fmaxf(ix2 - ix1, 0.0f), ih = fmaxf(iy2 - iy1, 0.0f);
  const float inter = iw * ih;
  const float area1 = (a[2] - a[0]) * (a[3] - a[1]);
  const float area2 = (b[2] - b[0]) * (b[3] - b[1]);
  float uni = area1 + area2 - inter;
  uni = fmaxf(uni, 1e-6f);
  return inter / uni;
}

__global__ __launch_bounds__(256) void yl_eval_confusion_kernel(const float* __restrict__ det,
                                                                const int* __restrict__ det_cls,
                                                                const int* __restrict__ det_off,
                                                                const float* __restrict__ gt,
                                                                const int* __restrict__ gt_cls,
                                                                const int* __restrict__ gt_off, int num_images,
                                                                int C, float thr, int* cm, uint8_t* gt_matched) {
  const int lane = threadIdx.x & 63;
  const int img = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (img >= num_images) return;
  const int d0 = det_off[img], d1 = det_off[img + 1];
  const int g0 = gt_off[img], ng = gt_off[img + 1] - g0;
  const int W = C + 1;
  for (int d = d0; d < d1; ++d) {
    float a[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = det[4 * (size_t)d + r];
    // np.argmax over the whole row (matched or not): first index of the maximum (:126-128)
    float best = -INFINITY;
    int bj = 0x7fffffff;
    for (int j = lane; j < ng; j += 64) {
      const float v = yl_iou_xyxy_f32(a, gt + 4 * (size_t)(g0 + j));
      if (v > best) { best = v; bj = j; }
    }
    yl_wave_argmax(best, bj);
    if (ng == 0) {                                                    // :119-123 (not reachable: images have GT)
      if (lane == 0) atomicAdd(&cm[C * W + det_cls[d]], 1);
      continue;
    }
    if (bj == 0x7fffffff) bj = 0;                                     // all-NaN row: argmax returns the first NaN
    const bool owner = lane == (bj & 63);
    int hit = 0;
    if (owner) {
      hit = (best >= thr && !gt_matched[g0 + bj]) ? 1 : 0;            // :130
      if (hit) {
        gt_matched[g0 + bj] = 1;
        atomicAdd(&cm[gt_cls[g0 + bj] * W + det_cls[d]], 1);          // true positive: (gt class, det class)
      } else {
        atomicAdd(&cm[C * W + det_cls[d]], 1);                        // false positive: (background, det class)
      }
    }
  }
  for (int j = lane; j < ng; j += 64)                                 // false negatives (:143-149)
    if (!gt_matched[g0 + j]) atomicAdd(&cm[gt_cls[g0 + j] * W + C], 1);
}

// ---- COCOeval, iouType="bbox" (pycocotools 2.0 cocoeval.py evaluateImg / accumulate, maskApi.c bbIou) -----------
// The reference's _coco_eval_from_lists (scripts/helpers/helpers.py:155-227) runs pycocotools' COCOeval; its
// behaviour is restated in include/yololite_hip.h and tests/_cocoeval_np.py.  Both kernels are exact: the match
// decisions are IEEE float64 compares of IoUs computed in bbIou's operation order, the accumulation divides
// integer counts once per element, so every parallel order gives pycocotools' bits.

constexpr int kYlCocoCache = 2;     // ground-truth strides per lane whose IoU is computed once per detection
constexpr int kYlCocoMaxR = 256;    // recall thresholds (default 101)

// maskApi.c bbIou: crowd ground truths divide by the detection's area
__device__ __forceinline__ double yl_bb_iou(double dx, double dy, double dw, double dh, double da,
                                            const double* __restrict__ g, bool crowd) {
  const double gx = g[0], gy = g[1], gw = g[2], gh = g[3];
  const double w = fmin(dw + dx, gw + gx) - fmax(dx, gx);
  if (w <= 0.0) return 0.0;
  const double h = fmin(dh + dy, gh + gy) - fmax(dy, gy);
  if (h <= 0.0) return 0.0;
  const double i = w * h;
  const double u = crowd ? da : (da + gw * gh) - i;
  return i / u;
}

// evaluateImg's scan over the ground truths (non-ignored first, stably) keeps the LAST maximum of the IoUs >= t
// among the non-ignored candidates, and only falls through to the ignored ones when there is none: the order is
// (group, IoU, index) with group 2 = not ignored, 1 = ignored, 0 = no candidate
__device__ __forceinline__ bool yl_coco_better(int g, double v, int j, int bg, double bv, int bj) {
  return g > bg || (g == bg && (v > bv || (v == bv && j > bj)));
}

__device__ __forceinline__ void yl_wave_coco_best(int& g, double& v, int& j) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const int og = __shfl_xor(g, m, 64);
    const double ov = __shfl_xor(v, m, 64);
    const int oj = __shfl_xor(j, m, 64);
    if (yl_coco_better(og, ov, oj, g, v, j)) { g = og; v = ov; j = oj; }
  }
}

// one block per key (image, category) and group of 4 area ranges; wave = area range, lanes across ground truths
__global__ __launch_bounds__(256) void yl_eval_coco_match_kernel(
    const double* __restrict__ det, const int* __restrict__ det_off, const double* __restrict__ gt,
    const double* __restrict__ gt_area, const uint8_t* __restrict__ gt_flags, const int* __restrict__ gt_off,
    int num_det, int num_gt, const double* __restrict__ area_rng, int A, const double* __restrict__ iou_thrs, int T,
    uint8_t* __restrict__ dt_flags, uint32_t* gt_matched) {
  const int lane = threadIdx.x & 63;
  const int a = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int key = blockIdx.x;
  if (a >= A) return;
  const int d0 = det_off[key], d1 = det_off[key + 1];
  const int g0 = gt_off[key], ng = gt_off[key + 1] - g0;
  const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
  // bit t = matched at iouThrs[t] in this area range; read and written only by lane (j & 63)
  uint32_t* gm = gt_matched + (size_t)a * num_gt + g0;
  // crowd (bit s) and _ignore (bit 8+s) of this lane's cached strides
  uint32_t cflag = 0;
#pragma unroll
  for (int s = 0; s < kYlCocoCache; ++s) {
    const int j = lane + 64 * s;
    if (j < ng) {
      const bool crowd = (gt_flags[g0 + j] & YL_COCO_GT_CROWD) != 0;
      const double ar = gt_area[g0 + j];
      if (crowd) cflag |= 1u << s;
      if (crowd || ar < lo || ar > hi) cflag |= 1u << (8 + s);
    }
  }
  for (int d = d0; d < d1; ++d) {
    const double dx = det[4 * (size_t)d], dy = det[4 * (size_t)d + 1];
    const double dw = det[4 * (size_t)d + 2], dh = det[4 * (size_t)d + 3];
    const double da = dw * dh;
    const bool d_out = da < lo || da > hi;
    if (ng == 0) {                                                       // unmatched at every threshold
      if (lane < T) dt_flags[((size_t)a * T + lane) * num_det + d] = d_out ? YL_COCO_DT_IGNORED : 0;
      continue;
    }
    double iou_c[kYlCocoCache];
#pragma unroll
    for (int s = 0; s < kYlCocoCache; ++s) {
      const int j = lane + 64 * s;
      iou_c[s] = j < ng ? yl_bb_iou(dx, dy, dw, dh, da, gt + 4 * (size_t)(g0 + j), (cflag >> s) & 1u) : 0.0;
    }
    uint8_t my_flag = 0;
    for (int t = 0; t < T; ++t) {
      const double tt = iou_thrs[t];
      const double thr = (1.0 - 1e-10) < tt ? (1.0 - 1e-10) : tt;       // min([t, 1-1e-10])
      const uint32_t bit = 1u << t;
      int bg = 0, bj = -1;
      double bv = 0.0;
#pragma unroll
      for (int s = 0; s < kYlCocoCache; ++s) {
        const int j = lane + 64 * s;
        if (j >= ng) break;
        const bool crowd = (cflag >> s) & 1u;
        if ((gm[j] & bit) && !crowd) continue;                           // matched, not crowd
        if (iou_c[s] < thr) continue;
        const int g = ((cflag >> (8 + s)) & 1u) ? 1 : 2;
        if (yl_coco_better(g, iou_c[s], j, bg, bv, bj)) { bg = g; bv = iou_c[s]; bj = j; }
      }
      for (int j = lane + 64 * kYlCocoCache; j < ng; j += 64) {        // crowded keys: IoU again per threshold
        const bool crowd = (gt_flags[g0 + j] & YL_COCO_GT_CROWD) != 0;
        if ((gm[j] & bit) && !crowd) continue;
        const double v = yl_bb_iou(dx, dy, dw, dh, da, gt + 4 * (size_t)(g0 + j), crowd);
        if (v < thr) continue;
        const double ar = gt_area[g0 + j];
        const int g = (crowd || ar < lo || ar > hi) ? 1 : 2;
        if (yl_coco_better(g, v, j, bg, bv, bj)) { bg = g; bv = v; bj = j; }
      }
      // most (detection, threshold) steps have no candidate or one: the butterfly only when two lanes compete
      const unsigned long long cand = __ballot(bg != 0);
      if (cand & (cand - 1)) {
        yl_wave_coco_best(bg, bv, bj);
      } else if (cand) {
        const int src = __ffsll(cand) - 1;
        bg = __shfl(bg, src, 64);
        bj = __shfl(bj, src, 64);
      } else {
        bg = 0;
      }
      const bool found = bg != 0;
      if (found && lane == (bj & 63)) gm[bj] |= bit;
      // dtm != 0: matched to a ground truth whose id is nonzero; dtIg = gtIg[m], or unmatched and outside the range
      const bool matched = found && (gt_flags[g0 + bj] & YL_COCO_GT_ID_NONZERO);
      const bool ignored = (found && bg == 1) || (!matched && d_out);
      if (lane == t) my_flag = (matched ? YL_COCO_DT_MATCHED : 0) | (ignored ? YL_COCO_DT_IGNORED : 0);
    }
    if (lane < T) dt_flags[((size_t)a * T + lane) * num_det + d] = my_flag;
  }
}

// one wave per (category k, area a, maxDet m, threshold t): a streaming pass over the category's detections in
// accumulate order with integer prefix counts (ballot + popcount), the max precision per recall bucket (the
// number of recThrs <= rc) in LDS, then a suffix max over the buckets:
//   q[r] = env[searchsorted(rc, recThrs[r], 'left')] = max{ pr[i] : rc[i] >= recThrs[r] }   (rc non-decreasing)
// Precisions are >= +0, so their bit patterns order like the values: a u64 max is the double max.
__global__ __launch_bounds__(256) void yl_eval_coco_accumulate_kernel(
    const int* __restrict__ order, const int* __restrict__ rank, const int* __restrict__ cat_off,
    const uint8_t* __restrict__ dt_flags, int num_det, const int* __restrict__ npig, int K, int A, int T,
    const int* __restrict__ max_dets, int M, const double* __restrict__ rec_thrs, int R,
    double* __restrict__ precision, double* __restrict__ recall) {
  __shared__ unsigned long long s_best[4][kYlCocoMaxR + 1];
  __shared__ double s_rec[kYlCocoMaxR];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int w = blockIdx.x * 4 + wv;                                     // ((k * A + a) * M + m) * T + t
  const int t = w % T, m = (w / T) % M, a = (w / (T * M)) % A, k = w / (T * M * A);
  const bool live = k < K;
  const int np = live ? npig[k * A + a] : 0;
  const size_t KAM = (size_t)K * A * M, pidx = ((size_t)k * A + a) * M + m;
  unsigned long long* best = s_best[wv];
  for (int r = threadIdx.x; r < R; r += 256) s_rec[r] = rec_thrs[r];
  for (int b = lane; b <= R; b += 64) best[b] = 0ull;
  __syncthreads();
  int tp = 0, fp = 0;
  if (live && np > 0) {
    const int e0 = cat_off[k], e1 = cat_off[k + 1];
    const int md = max_dets[m];
    const uint8_t* fl = dt_flags + ((size_t)a * T + t) * num_det;
    const double dnp = (double)np;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int base = e0; base < e1; base += 64) {
      const int i = base + lane;
      bool is_tp = false, is_fp = false;
      if (i < e1 && rank[i] < md) {
        const uint8_t f = fl[order[i]];
        if (!(f & YL_COCO_DT_IGNORED)) { is_tp = (f & YL_COCO_DT_MATCHED) != 0; is_fp = !is_tp; }
      }
      const unsigned long long btp = __ballot(is_tp), bfp = __ballot(is_fp);
      if (is_tp || is_fp) {
        const double ctp = (double)(tp + __popcll(btp & below) + (is_tp ? 1 : 0));
        const double cfp = (double)(fp + __popcll(bfp & below) + (is_fp ? 1 : 0));
        const double rc = ctp / dnp;
        const double pr = ctp / ((cfp + ctp) + 0x1p-52);                 // np.spacing(1)
        int lo = 0, hi = R;                                               // number of recThrs <= rc
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_rec[mid] <= rc) lo = mid + 1; else hi = mid;
        }
        atomicMax(&best[lo], (unsigned long long)__double_as_longlong(pr));
      }
      tp += __popcll(btp);
      fp += __popcll(bfp);
    }
  }
  __syncthreads();
  if (lane == 0)
    for (int b = R - 1; b >= 1; --b) best[b] = best[b] > best[b + 1] ? best[b] : best[b + 1];
  __syncthreads();
  if (!live) return;
  for (int r = lane; r < R; r += 64)
    precision[((size_t)t * R + r) * KAM + pidx] = np > 0 ? __longlong_as_double((long long)best[r + 1]) : -1.0;
  if (lane == 0) recall[(size_t)t * KAM + pidx] = np > 0 ? (double)tp / (double)np : -1.0;
}

inline yl_status yl_hip(hipError_t e) { return e == hipSuccess ? YL_OK : YL_ERR_HIP; }

}  // namespace

extern "C" {

yl_status yl_eval_match(const double* det_xywh_dev, const int32_t* det_off_dev, const double* gt_xywh_dev,
                        const int32_t* gt_off_dev, int32_t num_keys, int32_t num_gt, double iou_thr, uint8_t* tp_dev,
                        int32_t* match_dev, uint8_t* gt_matched_dev, void* stream) {
  if (num_keys < 0 || num_gt < 0) return YL_ERR_INVALID;
  if (num_keys == 0) return YL_OK;
  if (!det_off_dev || !gt_off_dev || !tp_dev || (num_gt > 0 && (!gt_xywh_dev || !gt_matched_dev)))
    return YL_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (num_gt > 0) {
    const hipError_t e = hipMemsetAsync(gt_matched_dev, 0, (size_t)num_gt, st);
    if (e != hipSuccess) return YL_ERR_HIP;
  }
  hipLaunchKernelGGL(yl_eval_match_kernel, dim3((num_keys + 3) / 4), dim3(256), 0, st, det_xywh_dev, det_off_dev,
                     gt_xywh_dev, gt_off_dev, num_keys, iou_thr, tp_dev, match_dev, gt_matched_dev);
  return yl_hip(hipGetLastError());
}

yl_status yl_eval_sweep(const double* score_dev, const uint8_t* tp_dev, const uint8_t* counted_dev, int32_t n,
                        const double* thr_dev, int32_t steps, int32_t* tp_ge_dev, int32_t* fp_ge_dev, void* stream) {
  if (n < 0 || steps <= 0 || !thr_dev || !tp_ge_dev || !fp_ge_dev) return YL_ERR_INVALID;
  if (n > 0 && (!score_dev || !tp_dev)) return YL_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(tp_ge_dev, 0, sizeof(int32_t) * (size_t)steps, st) != hipSuccess) return YL_ERR_HIP;
  if (hipMemsetAsync(fp_ge_dev, 0, sizeof(int32_t) * (size_t)steps, st) != hipSuccess) return YL_ERR_HIP;
  if (n > 0)
    hipLaunchKernelGGL(yl_eval_hist_kernel, dim3((n + 255) / 256), dim3(256), 0, st, score_dev, tp_dev, counted_dev, n,
                       thr_dev, steps, tp_ge_dev, fp_ge_dev);
  hipLaunchKernelGGL(yl_eval_suffix_kernel, dim3(1), dim3(128), 0, st, tp_ge_dev, fp_ge_dev, steps);
  return yl_hip(hipGetLastError());
}

yl_status yl_eval_confusion(const float* det_xyxy_dev, const int32_t* det_cls_dev, const int32_t* det_off_dev,
                            const float* gt_xyxy_dev, const int32_t* gt_cls_dev, const int32_t* gt_off_dev,
                            int32_t num_images, int32_t num_gt, int32_t num_classes, float iou_thr, int32_t* cm_dev,
                            uint8_t* gt_matched_dev, void* stream) {
  if (num_images < 0 || num_gt < 0 || num_classes <= 0 || !cm_dev) return YL_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const size_t W = (size_t)num_classes + 1;
  if (hipMemsetAsync(cm_dev, 0, sizeof(int32_t) * W * W, st) != hipSuccess) return YL_ERR_HIP;
  if (num_images == 0) return YL_OK;
  if (!det_off_dev || !gt_off_dev || (num_gt > 0 && (!gt_xyxy_dev || !gt_cls_dev || !gt_matched_dev)))
    return YL_ERR_INVALID;
  if (num_gt > 0 && hipMemsetAsync(gt_matched_dev, 0, (size_t)num_gt, st) != hipSuccess) return YL_ERR_HIP;
  hipLaunchKernelGGL(yl_eval_confusion_kernel, dim3((num_images + 3) / 4), dim3(256), 0, st, det_xyxy_dev,
                     det_cls_dev, det_off_dev, gt_xyxy_dev, gt_cls_dev, gt_off_dev, num_images, num_classes, iou_thr,
                     cm_dev, gt_matched_dev);
  return yl_hip(hipGetLastError());
}

yl_status yl_eval_coco_match(const double* det_xywh_dev, const int32_t* det_off_dev, const double* gt_xywh_dev,
                             const double* gt_area_dev, const uint8_t* gt_flags_dev, const int32_t* gt_off_dev,
                             int32_t num_keys, int32_t num_det, int32_t num_gt, const double* area_rng_dev,
                             int32_t num_areas, const double* iou_thrs_dev, int32_t num_thrs, uint8_t* dt_flags_dev,
                             uint32_t* gt_matched_dev, void* stream) {
  if (num_keys < 0 || num_det < 0 || num_gt < 0 || num_areas < 1 || num_thrs < 1 || num_thrs > 32)
    return YL_ERR_INVALID;
  if (num_keys == 0 || num_det == 0) return YL_OK;
  if (!det_xywh_dev || !det_off_dev || !gt_off_dev || !area_rng_dev || !iou_thrs_dev || !dt_flags_dev ||
      (num_gt > 0 && (!gt_xywh_dev || !gt_area_dev || !gt_flags_dev || !gt_matched_dev)))
    return YL_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (num_gt > 0 &&
      hipMemsetAsync(gt_matched_dev, 0, sizeof(uint32_t) * (size_t)num_gt * (size_t)num_areas, st) != hipSuccess)
    return YL_ERR_HIP;
  hipLaunchKernelGGL(yl_eval_coco_match_kernel, dim3(num_keys, (num_areas + 3) / 4), dim3(256), 0, st, det_xywh_dev,
                     det_off_dev, gt_xywh_dev, gt_area_dev, gt_flags_dev, gt_off_dev, num_det, num_gt, area_rng_dev,
                     num_areas, iou_thrs_dev, num_thrs, dt_flags_dev, gt_matched_dev);
  return yl_hip(hipGetLastError());
}

yl_status yl_eval_coco_accumulate(const int32_t* order_dev, const int32_t* rank_dev, const int32_t* cat_off_dev,
                                  const uint8_t* dt_flags_dev, int32_t num_det, const int32_t* npig_dev,
                                  int32_t num_cats, int32_t num_areas, int32_t num_thrs, const int32_t* max_dets_dev,
                                  int32_t num_max_dets, const double* rec_thrs_dev, int32_t num_rec,
                                  double* precision_dev, double* recall_dev, void* stream) {
  if (num_cats < 1 || num_areas < 1 || num_thrs < 1 || num_max_dets < 1 || num_rec < 1 || num_rec > kYlCocoMaxR ||
      num_det < 0)
    return YL_ERR_INVALID;
  if (!cat_off_dev || !npig_dev || !max_dets_dev || !rec_thrs_dev || !precision_dev || !recall_dev ||
      (num_det > 0 && (!order_dev || !rank_dev || !dt_flags_dev)))
    return YL_ERR_INVALID;
  const long long waves = (long long)num_cats * num_areas * num_max_dets * num_thrs;
  if (waves > 0x7fffffffll) return YL_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(yl_eval_coco_accumulate_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, order_dev,
                     rank_dev, cat_off_dev, dt_flags_dev, num_det, npig_dev, num_cats, num_areas, num_thrs,
                     max_dets_dev, num_max_dets, rec_thrs_dev, num_rec, precision_dev, recall_dev);
  return yl_hip(hipGetLastError());
}

}  // extern "C"
