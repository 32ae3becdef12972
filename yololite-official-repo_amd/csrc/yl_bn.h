// BatchNorm2d followed by nothing, ReLU, ReLU6 or SiLU on NHWC fp32 rows, forward and backward: the five kernels and the three
// launch sequences that every trainable module runs -- the heads' and the depthwise neck's blocks (yl_block.h), the dense
// neck (yl_dneck.hip), the backbone stage and the stem (yl_units.h) -- with the few primitives they are written in.  This
// is the bottom header of the training units.  Everything lives in an anonymous namespace: each translation unit that
// includes it compiles the instantiations IT launches into its own code object.
//
//   forward:   y = gamma * (z - mean) * invstd + beta    h = act(y) [+ res]
//   backward:  g = dh * act'(y)    dz = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat)),  xhat = (z - mean) * invstd
//
// The activation is a template argument; its part of the arithmetic is the two device functions act_apply and act_grad.
#ifndef YL_BN_H
#define YL_BN_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NT = 256;
constexpr int STAT_ROWS = 256;           // rows of one tile of the row reductions (the stem's tiles are a multiple of it)
constexpr double BN_EPS = 1e-5, BN_MOMENTUM = 0.1;

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }
inline int pick_cq(int F) {              // channel quads per workgroup of the row reductions: a power of two <= 64
  int cq = 1;
  while (cq < (F >> 2) && cq < 64) cq <<= 1;
  return cq;
}
inline int64_t round16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// ---- the activation's part.  y is computed in fp32 by bn_y everywhere; the SiLU factor is recomputed from it
constexpr int ACT_NONE = 0, ACT_RELU = 1, ACT_SILU = 2, ACT_RELU6 = 3;
constexpr bool act_reads_h(int act) { return act == ACT_RELU || act == ACT_RELU6; }
__device__ __forceinline__ float bn_y(float z, float mu, float is, float gamma, float beta) { return (z - mu) * is * gamma + beta; }
template <int ACT> __device__ __forceinline__ float act_apply(float y) {
  if constexpr (ACT == ACT_RELU) return fmaxf(y, 0.f);
  if constexpr (ACT == ACT_RELU6) return fminf(fmaxf(y, 0.f), 6.f);
  if constexpr (ACT == ACT_SILU) return y / (1.f + expf(-y));
  return y;
}
// g = dh * act'(y) in T (float, or double for the column sums): ReLU and ReLU6 read their mask off the output h and widen dh
// themselves (ReLU6: 0 < h < 6, both strict, torch's hardtanh_backward; h = 6 exactly where y >= 6);
// SiLU forms the product with d silu / dy = s * (1 + y * (1 - s)) in float and widens that.  h is read by ReLU / ReLU6 only, y by SiLU only
template <int ACT, class T> __device__ __forceinline__ T act_grad(float dh, float h, float y) {
  if constexpr (ACT == ACT_RELU) return h > 0.f ? (T)dh : (T)0;
  if constexpr (ACT == ACT_RELU6) return (h > 0.f && h < 6.f) ? (T)dh : (T)0;
  if constexpr (ACT == ACT_SILU) {
    const float sg = 1.f / (1.f + expf(-y));
    return (T)(dh * (sg * (1.f + y * (1.f - sg))));
  }
  return (T)dh;
}

// ---- column sums.  Workgroup (tile of `rows` rows, group of CQ channel quads); thread t: quad t % CQ, rows m0 + t / CQ,
// + 256 / CQ, ...; float64 sums per thread, summed over the row lanes in lane order by the thread of lane 0.
// Forward (bwd = 0, the same for every ACT): sum z, sum z^2.  Backward: sum g, sum g * xhat.
struct StatP {
  const float *a, *h, *z, *stats;        // forward: a = z.  backward: a = dh, h = the output (read by ReLU / ReLU6 only), z, stats
  double* part;                          // [tile][2][F]
  int M, F, CQ, bwd;
  int rows;                              // of one tile: a multiple of STAT_ROWS
  const float *gamma, *beta;             // backward, read by SiLU only
};
template <int ACT>
__global__ __launch_bounds__(NT) void yl_bn_colstats_kernel(StatP P) {
  __shared__ double red[NT][8];
  const int t = threadIdx.x, cq = t & (P.CQ - 1), rs = t / P.CQ, RS = NT / P.CQ;
  const int c = (blockIdx.y * P.CQ + cq) * 4, F = P.F;
  const bool on = c < F;
  const int m0 = blockIdx.x * P.rows, m1 = m0 + P.rows < P.M ? m0 + P.rows : P.M;
  double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
  if (on) {
    f32x4 mu = {0.f, 0.f, 0.f, 0.f}, is = mu;
    float ga[4] = {0.f, 0.f, 0.f, 0.f}, be[4] = {0.f, 0.f, 0.f, 0.f};
    if (P.bwd) {
      mu = ld4(P.stats + c); is = ld4(P.stats + F + c);
      if constexpr (ACT == ACT_SILU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { ga[e] = P.gamma[c + e]; be[e] = P.beta[c + e]; }
      }
    }
    for (int m = m0 + rs; m < m1; m += RS) {
      const long o = (long)m * F + c;
      const f32x4 a = ld4(P.a + o);
      if (!P.bwd) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { s0[e] += (double)a[e]; s1[e] += (double)a[e] * (double)a[e]; }
      } else {
        const f32x4 zv = ld4(P.z + o);
        f32x4 hv = {1.f, 1.f, 1.f, 1.f};
        if constexpr (act_reads_h(ACT)) hv = ld4(P.h + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float y = 0.f;
          if constexpr (ACT == ACT_SILU) y = bn_y(zv[e], mu[e], is[e], ga[e], be[e]);
          const double g = act_grad<ACT, double>(a[e], hv[e], y);
          const double xh = ((double)zv[e] - (double)mu[e]) * (double)is[e];
          s0[e] += g; s1[e] += g * xh;
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) { red[t][e] = s0[e]; red[t][4 + e] = s1[e]; }
  __syncthreads();
  if (rs == 0 && on) {
    for (int k = 1; k < RS; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) red[t][e] += red[k * P.CQ + cq][e];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      P.part[((long)blockIdx.x * 2 + 0) * F + c + e] = red[t][e];
      P.part[((long)blockIdx.x * 2 + 1) * F + c + e] = red[t][4 + e];
    }
  }
}

// ---- second stages: one thread per channel, the partials summed in tile order in float64
struct BnFwdP {
  const double* part; int tiles, M, F, train;
  float *rm, *rv; int64_t* nbt;          // running statistics (train: updated in place)
  float* stats;                          // [2][F]: mean, invstd of this call
};
__global__ __launch_bounds__(NT) void yl_bn_stats_kernel(BnFwdP P, double eps) {
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
struct BnBwdP {
  const double* part; int tiles, M, F, train;
  float *dgamma, *dbeta;                 // NULL: not wanted
  float* coef;                           // [2][F]: dbeta / M, dgamma / M (zero in eval mode)
};
__global__ __launch_bounds__(NT) void yl_bn_grads_kernel(BnBwdP P) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= P.F) return;
  double s0 = 0, s1 = 0;
  for (int t = 0; t < P.tiles; ++t) { s0 += P.part[((long)t * 2) * P.F + c]; s1 += P.part[((long)t * 2 + 1) * P.F + c]; }
  if (P.dbeta) P.dbeta[c] = (float)s0;
  if (P.dgamma) P.dgamma[c] = (float)s1;
  P.coef[c] = P.train ? (float)(s0 / P.M) : 0.f;
  P.coef[P.F + c] = P.train ? (float)(s1 / P.M) : 0.f;
}

// ---- element-wise.  h = act(y) [+ res]: the residual is added to the ROUNDED activation output, as a separate add would
// (these units are compiled without contraction)
template <int ACT>
__global__ __launch_bounds__(NT) void yl_bn_apply_kernel(const float* __restrict__ z, const float* __restrict__ stats,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const float* __restrict__ res, float* __restrict__ h, long n4, int F) {
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  if (idx >= n4) return;
  const int c = (int)((idx * 4) % F);
  const f32x4 v = ld4(z + idx * 4), mu = ld4(stats + c), is = ld4(stats + F + c);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = act_apply<ACT>(bn_y(v[e], mu[e], is[e], gamma[c + e], beta[c + e]));
  if (res) o = ld4(res + idx * 4) + o;
  st4(h + idx * 4, o);
}
// dz = gamma * invstd * (g - c0 - xhat * c1).  dh and dz may be one buffer (each thread reads its four values before it
// writes them): neither is __restrict__.  h is read by ReLU / ReLU6 only, beta by SiLU only
template <int ACT>
__global__ __launch_bounds__(NT) void yl_bn_bwd_kernel(const float* dh, const float* __restrict__ h, const float* __restrict__ z,
                                                      const float* __restrict__ stats, const float* __restrict__ coef,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float* dz, long n4, int F) {
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  if (idx >= n4) return;
  const int c = (int)((idx * 4) % F);
  const f32x4 g = ld4(dh + idx * 4), zv = ld4(z + idx * 4);
  f32x4 hv = {1.f, 1.f, 1.f, 1.f};
  if constexpr (act_reads_h(ACT)) hv = ld4(h + idx * 4);
  const f32x4 mu = ld4(stats + c), is = ld4(stats + F + c), c0 = ld4(coef + c), c1 = ld4(coef + F + c);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float y = 0.f;
    if constexpr (ACT == ACT_SILU) y = bn_y(zv[e], mu[e], is[e], gamma[c + e], beta[c + e]);
    const float ge = act_grad<ACT, float>(g[e], hv[e], y);
    const float xh = (zv[e] - mu[e]) * is[e];
    o[e] = gamma[c + e] * is[e] * (ge - c0[e] - xh * c1[e]);
  }
  st4(dz + idx * 4, o);
}

// ---- the launch sequences.  BnLayer: one BatchNorm of F channels over M rows; its row reductions run over `tiles` tiles
// of `rows` rows into `part`, its (mean, invstd) live in `stats`
struct BnLayer {
  int M, F, rows, tiles;
  const float *gamma, *beta;
  float *rm, *rv; int64_t* nbt;
  double eps;
  float* stats;
  double* part;
};

// forward: sums if training, stats, apply: h = act(bn(z)) [+ res].  -> launches enqueued
template <int ACT>
int bn_forward(hipStream_t s, const BnLayer& L, bool train, const float* z, const float* res, float* h) {
  if (train) {
    StatP sp;
    sp.a = z; sp.h = nullptr; sp.z = nullptr; sp.stats = nullptr; sp.part = L.part;
    sp.M = L.M; sp.F = L.F; sp.CQ = pick_cq(L.F); sp.bwd = 0; sp.rows = L.rows; sp.gamma = sp.beta = nullptr;
    hipLaunchKernelGGL(yl_bn_colstats_kernel<ACT>, dim3(L.tiles, ceil_div(L.F >> 2, sp.CQ)), dim3(NT), 0, s, sp);
  }
  BnFwdP bp;
  bp.part = L.part; bp.tiles = L.tiles; bp.M = L.M; bp.F = L.F; bp.train = train ? 1 : 0;
  bp.rm = L.rm; bp.rv = L.rv; bp.nbt = L.nbt; bp.stats = L.stats;
  hipLaunchKernelGGL(yl_bn_stats_kernel, dim3(ceil_div(L.F, NT)), dim3(NT), 0, s, bp, L.eps);
  const long n4 = (long)L.M * (L.F >> 2);
  hipLaunchKernelGGL(yl_bn_apply_kernel<ACT>, dim3(ceil_div(n4, NT)), dim3(NT), 0, s, z, (const float*)L.stats, L.gamma, L.beta,
                     res, h, n4, L.F);
  return train ? 3 : 2;
}
// backward, first part: sum g and sum g * xhat if the batch statistics or a gradient need them, then dgamma, dbeta (NULL:
// not wanted) and the two coefficients of the dz kernel.  -> launches enqueued
template <int ACT>
int bn_backward_sums(hipStream_t s, const BnLayer& L, bool train, const float* dh, const float* h, const float* z,
                     float* dgamma, float* dbeta, float* coef) {
  const bool sums = train || dgamma || dbeta;
  if (sums) {
    StatP sp;
    sp.a = dh; sp.h = h; sp.z = z; sp.stats = L.stats; sp.part = L.part;
    sp.M = L.M; sp.F = L.F; sp.CQ = pick_cq(L.F); sp.bwd = 1; sp.rows = L.rows; sp.gamma = L.gamma; sp.beta = L.beta;
    hipLaunchKernelGGL(yl_bn_colstats_kernel<ACT>, dim3(L.tiles, ceil_div(L.F >> 2, sp.CQ)), dim3(NT), 0, s, sp);
  }
  BnBwdP bp;
  bp.part = L.part; bp.tiles = sums ? L.tiles : 0; bp.M = L.M; bp.F = L.F; bp.train = train;
  bp.dgamma = dgamma; bp.dbeta = dbeta; bp.coef = coef;
  hipLaunchKernelGGL(yl_bn_grads_kernel, dim3(ceil_div(L.F, NT)), dim3(NT), 0, s, bp);
  return sums ? 2 : 1;
}
// backward, second part, if anything below needs it: dz (may be dh's buffer).  -> launches enqueued
template <int ACT>
int bn_backward_dz(hipStream_t s, const BnLayer& L, const float* dh, const float* h, const float* z, const float* coef, float* dz) {
  const long n4 = (long)L.M * (L.F >> 2);
  hipLaunchKernelGGL(yl_bn_bwd_kernel<ACT>, dim3(ceil_div(n4, NT)), dim3(NT), 0, s, dh, h, z, (const float*)L.stats, coef, L.gamma,
                     L.beta, dz, n4, L.F);
  return 1;
}

}  // namespace
#endif  // YL_BN_H
