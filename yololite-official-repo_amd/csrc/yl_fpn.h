// What the two trainable FPN necks share (yl_neck.hip: the depthwise neck of YOLOLiteMS_CPU; yl_dneck.hip: the dense
// 3x3 + SiLU neck of YOLOLiteMS): everything around the smooth blocks.
//   * the lateral's epilogue: an output accessor of yl_head_gemm_kernel that adds the bias and the coarser level's p read
//     through the nearest map, and writes t_k;
//   * the transposed upsample as a gather: the nearest map is monotone, so the pre-image of a source cell is a
//     contiguous range of destination rows and of columns; one thread per (b, i, j, channel quad) sums its range in
//     row-major order and adds gp_k.  No atomics;
//   * the lateral's gradients from the GEMM forms of the heads (split GEMM + ordered sum for the weight, NP = Cin,
//     NQ = F; float64 column sums for the bias; one GEMM for dc);
//   * the nearest maps on the device and the checks of yl_neck_cfg.
// Like yl_block.h, everything lives in an anonymous namespace: each unit compiles the kernels it launches.
#ifndef YL_FPN_H
#define YL_FPN_H
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

inline bool cfg_ok(const yl_neck_cfg* c) {
  if (!c || c->channels < 4 || c->depth < 1 || c->depth > YL_NECK_MAX_DEPTH || c->num_levels < 1 ||
      c->num_levels > YL_NECK_MAX_LEVELS)
    return false;
  for (int k = 0; k < c->num_levels; ++k)
    if (c->in_channels[k] < 4) return false;
  return true;
}
inline bool cfg_supported(const yl_neck_cfg* c) {
  if (c->channels & 3) return false;
  for (int k = 0; k < c->num_levels; ++k)
    if (c->in_channels[k] & 3) return false;
  return true;
}
// what the 32-bit row and offset arithmetic of the GEMMs and the row reductions carries
inline bool level_rows_ok(int64_t M, int64_t F, int64_t Cin) {
  return !(M > (int64_t)65535 * GEMM_ROWS || M * F >= ((int64_t)1 << 40) || M * Cin >= ((int64_t)1 << 40) || Cin > (1 << 20));
}

struct LevelMaps { const int *src, *lo, *hi; };      // of the pair (destination k, source k + 1)

// the nearest maps of a handle on the device, and the sizes they were made for (0: none)
struct MapTables {
  int64_t cap;
  int* dev;
  int S[YL_NECK_MAX_LEVELS];
};

inline int64_t map_table_bytes(int L, const int32_t* sizes) {
  int64_t n = 0;
  for (int k = 0; k + 1 < L; ++k) n += ((int64_t)sizes[k] + 2 * (int64_t)sizes[k + 1]) * 4;
  return n;
}

// the maps of `sizes` on the device (made on the host and uploaded when the sizes change) -> maps[k] of every pair
inline yl_status maps_ensure(MapTables& mt, int L, const int32_t* sizes, int64_t table_bytes, LevelMaps* maps) {
  bool same = true;
  for (int k = 0; k < L; ++k) same = same && mt.S[k] == sizes[k];
  if (!same && L > 1) {                  // new maps: nothing that reads the old ones may still run
    if (hipDeviceSynchronize() != hipSuccess) return YL_ERR_HIP;
    for (int k = 0; k < L; ++k) mt.S[k] = 0;
    if (table_bytes > mt.cap) {
      hipFree(mt.dev);
      mt.dev = nullptr; mt.cap = 0;
      if (hipMalloc((void**)&mt.dev, (size_t)table_bytes) != hipSuccess) { (void)hipGetLastError(); return YL_ERR_NOMEM; }
      mt.cap = table_bytes;
    }
    int32_t* host = new (std::nothrow) int32_t[(size_t)table_bytes / 4];
    if (!host) return YL_ERR_NOMEM;
    int32_t* q = host;
    for (int k = 0; k + 1 < L; ++k) {
      yl_neck_nearest_map(sizes[k], sizes[k + 1], q, q + sizes[k], q + sizes[k] + sizes[k + 1]);
      q += sizes[k] + 2 * sizes[k + 1];
    }
    const hipError_t e = hipMemcpy(mt.dev, host, (size_t)table_bytes, hipMemcpyHostToDevice);
    delete[] host;
    if (e != hipSuccess) return YL_ERR_HIP;
    for (int k = 0; k < L; ++k) mt.S[k] = sizes[k];
  }
  const int* q = mt.dev;
  for (int k = 0; k < YL_NECK_MAX_LEVELS; ++k) maps[k] = LevelMaps{nullptr, nullptr, nullptr};
  for (int k = 0; k + 1 < L; ++k) {
    maps[k] = LevelMaps{q, q + sizes[k], q + sizes[k] + sizes[k + 1]};
    q += sizes[k] + 2 * sizes[k + 1];
  }
  return YL_OK;
}

// t = c . Wlat^T + blat (+ up(p of the coarser level, Sc cells wide, through src)): 1 launch
inline void lateral_forward(hipStream_t s, const float* lat_w, const float* lat_b, const float* c, float* t, const float* up,
                            const int* src, int F, int M, int Cin, int S, int Sc) {
  OutLateral ol;
  ol.t = t; ol.bias = lat_b; ol.up = up; ol.src = src;
  ol.F = F; ol.S = S; ol.Sc = Sc;
  launch_gemm<0>(s, RowsScalar{lat_w, Cin}, RowsVec{c, Cin}, ol, F, M, Cin, Cin, 1);
}

// the lateral's three gradients from gt, each only where wanted: 2 launches for dWlat, 2 for dblat, 1 for dc
inline void lateral_backward(hipStream_t s, const float* lat_w, float* g_lat_w, float* g_lat_b, float* dc, const float* c,
                             const float* gt, float* wpart, double* spart, int F, int Cin, int M, int S, int stat_tiles,
                             int lgrad_rows, int lgrad_splits, int* launches) {
  int nl = 0;
  if (g_lat_w) {                         // dWlat[f][cin] = sum over rows of gt[m][f] * c[m][cin]
    launch_gemm<0>(s, ColsScalar{c, Cin}, ColsScalar{gt, F}, OutPartial{wpart, (long)F * Cin}, Cin, F, M, lgrad_rows, lgrad_splits);
    HeadRows none;
    memset(&none, 0, sizeof(none));
    hipLaunchKernelGGL(yl_head_wsum_kernel, dim3(ceil_div((long)F * Cin, NT)), dim3(NT), 0, s, (const float*)wpart,
                       lgrad_splits, Cin, F, g_lat_w, none, 0);
    nl += 2;
  }
  if (g_lat_b) {
    const HeadGeom plain = {1, F, 0, S * S, F};   // column n of row m at m * F + n
    hipLaunchKernelGGL(yl_head_ysum_kernel, dim3(stat_tiles, ceil_div(F, 64)), dim3(NT), 0, s, gt, plain, spart, M, F);
    hipLaunchKernelGGL(yl_neck_bsum_kernel, dim3(ceil_div(F, NT)), dim3(NT), 0, s, (const double*)spart, stat_tiles, F,
                       g_lat_b);
    nl += 2;
  }
  if (dc) {                              // dc = gt . Wlat
    launch_gemm<0>(s, ColsScalar{lat_w, Cin}, RowsVec{gt, F}, OutRowsVec{dc, Cin}, Cin, M, F, F, 1);
    ++nl;
  }
  *launches += nl;
}

}  // namespace
#endif  // YL_FPN_H
