// BatchNorm2d with and without ReLU on NHWC fp32 rows, eps from the configuration: what the trainable backbone stage
// (yl_stage.hip) and the trainable dense stem (yl_stem.hip) share.  Like yl_block.h, everything lives in an anonymous
// namespace: each translation unit that includes this header compiles the kernels it launches into its own code object.
// The kernels only: the walk over a stack's units that launches them, forward and backward, is yl_units.h.
#ifndef YL_BN_H
#define YL_BN_H
#include "yl_block.h"

namespace {

// ---- BatchNorm.  The column sums of yl_head_colstats_kernel (same StatP, same layout of workgroups, threads and
// partials) with the ReLU mask as a template argument: RELU = false has no mask, g = dh, and never reads P.h.
// The body is written once, as a macro over the rows of one tile (tile t covers [t * rows, min(M, (t + 1) * rows))): the
// stage's kernel has the constant STAT_ROWS in it and keeps the code it always had, the stem's takes the rows as an argument.
#define YL_COLSTATS_BODY(ROWS)                                                                                            \
  __shared__ double red[NT][8];                                                                                           \
  const int t = threadIdx.x, cq = t & (P.CQ - 1), rs = t / P.CQ, RS = NT / P.CQ;                                          \
  const int c = (blockIdx.y * P.CQ + cq) * 4, F = P.F;                                                                    \
  const bool on = c < F;                                                                                                  \
  const int m0 = blockIdx.x * (ROWS), m1 = m0 + (ROWS) < P.M ? m0 + (ROWS) : P.M;                                         \
  double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};                                                                      \
  if (on) {                                                                                                               \
    f32x4 mu = {0.f, 0.f, 0.f, 0.f}, is = mu;                                                                             \
    if (P.bwd) { mu = ld4(P.stats + c); is = ld4(P.stats + F + c); }                                                      \
    for (int m = m0 + rs; m < m1; m += RS) {                                                                              \
      const long o = (long)m * F + c;                                                                                     \
      const f32x4 a = ld4(P.a + o);                                                                                       \
      if (!P.bwd) {                                                                                                       \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) { s0[e] += (double)a[e]; s1[e] += (double)a[e] * (double)a[e]; }    \
      } else {                                                                                                            \
        const f32x4 zv = ld4(P.z + o);                                                                                    \
        f32x4 hv = {1.f, 1.f, 1.f, 1.f};                                                                                  \
        if (RELU) hv = ld4(P.h + o);                                                                                      \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                                   \
          const double g = hv[e] > 0.f ? (double)a[e] : 0.0;                                                              \
          const double xh = ((double)zv[e] - (double)mu[e]) * (double)is[e];                                              \
          s0[e] += g; s1[e] += g * xh;                                                                                    \
        }                                                                                                                 \
      }                                                                                                                   \
    }                                                                                                                     \
  }                                                                                                                       \
  _Pragma("unroll") for (int e = 0; e < 4; ++e) { red[t][e] = s0[e]; red[t][4 + e] = s1[e]; }                             \
  __syncthreads();                                                                                                        \
  if (rs == 0 && on) {                                                                                                    \
    for (int k = 1; k < RS; ++k)                                                                                          \
      _Pragma("unroll") for (int e = 0; e < 8; ++e) red[t][e] += red[k * P.CQ + cq][e];                                   \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                                       \
      P.part[((long)blockIdx.x * 2 + 0) * F + c + e] = red[t][e];                                                         \
      P.part[((long)blockIdx.x * 2 + 1) * F + c + e] = red[t][4 + e];                                                     \
    }                                                                                                                     \
  }
// tiles of STAT_ROWS rows (the stage)
template <bool RELU>
__global__ __launch_bounds__(NT) void yl_stage_colstats_kernel(StatP P) { YL_COLSTATS_BODY(STAT_ROWS) }
// tiles of `rows` rows, a multiple of STAT_ROWS (the stem, whose tile COUNT is bounded: yl_stem_plan)
template <bool RELU>
__global__ __launch_bounds__(NT) void yl_stem_colstats_kernel(StatP P, int rows) { YL_COLSTATS_BODY(rows) }
#undef YL_COLSTATS_BODY

// yl_head_bn_stats_kernel with eps from the configuration
__global__ __launch_bounds__(NT) void yl_stage_bn_stats_kernel(BnFwdP P, double eps) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= P.F) return;
  if (!P.train) {                        // eval: the running statistics
    P.stats[c] = P.rm[c];
    P.stats[P.F + c] = (float)(1.0 / sqrt((double)P.rv[c] + eps));
    return;
  }
  double s0 = 0, s1 = 0;
  for (int t = 0; t < P.tiles; ++t) { s0 += P.part[((long)t * 2) * P.F + c]; s1 += P.part[((long)t * 2 + 1) * P.F + c]; }
  const double mean = s0 / P.M;
  double var = s1 / P.M - mean * mean;
  var = var > 0 ? var : 0;
  P.stats[c] = (float)mean;
  P.stats[P.F + c] = (float)(1.0 / sqrt(var + eps));
  P.rm[c] = (float)((1.0 - BN_MOMENTUM) * (double)P.rm[c] + BN_MOMENTUM * mean);
  P.rv[c] = (float)((1.0 - BN_MOMENTUM) * (double)P.rv[c] + BN_MOMENTUM * (var * P.M / (P.M - 1)));
  if (c == 0) *P.nbt += 1;
}
// h = gamma * (z - mean) * invstd + beta, [relu], [+ res]: the residual is added to the ROUNDED BatchNorm output, as a
// separate add would (these units are compiled without contraction)
template <bool RELU>
__global__ __launch_bounds__(NT) void yl_stage_bn_kernel(const float* __restrict__ z, const float* __restrict__ stats,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const float* __restrict__ res, float* __restrict__ h, long n4, int F) {
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  if (idx >= n4) return;
  const int c = (int)((idx * 4) % F);
  const f32x4 v = ld4(z + idx * 4), mu = ld4(stats + c), is = ld4(stats + F + c);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    o[e] = (v[e] - mu[e]) * is[e] * gamma[c + e] + beta[c + e];
    if (RELU) o[e] = fmaxf(o[e], 0.f);
  }
  if (res) o = ld4(res + idx * 4) + o;
  st4(h + idx * 4, o);
}
// dz = gamma * invstd * (g - c0 - xhat * c1), g = dh [* (h > 0)].  dh and dz may be one buffer (each thread reads its four
// values before it writes them): neither is __restrict__
template <bool RELU>
__global__ __launch_bounds__(NT) void yl_stage_bn_bwd_kernel(const float* dh, const float* __restrict__ h,
                                                            const float* __restrict__ z, const float* __restrict__ stats,
                                                            const float* __restrict__ coef, const float* __restrict__ gamma,
                                                            float* dz, long n4, int F) {
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  if (idx >= n4) return;
  const int c = (int)((idx * 4) % F);
  const f32x4 g = ld4(dh + idx * 4), zv = ld4(z + idx * 4);
  f32x4 hv = {1.f, 1.f, 1.f, 1.f};
  if (RELU) hv = ld4(h + idx * 4);
  const f32x4 mu = ld4(stats + c), is = ld4(stats + F + c), c0 = ld4(coef + c), c1 = ld4(coef + F + c);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float ge = hv[e] > 0.f ? g[e] : 0.f;
    const float xh = (zv[e] - mu[e]) * is[e];
    o[e] = gamma[c + e] * is[e] * (ge - c0[e] - xh * c1[e]);
  }
  st4(dz + idx * 4, o);
}

inline int out_size(int S, int k, int st) { return (S + 2 * ((k - 1) / 2) - k) / st + 1; }
inline int64_t round16(int64_t v) { return (v + 15) & ~(int64_t)15; }

}  // namespace
#endif  // YL_BN_H
