// The DWConvBlock of the reference (scripts/model/model_v2.py:23-39) on NHWC fp32 rows, shared by the detection heads
// (yl_head.hip) and the FPN neck (yl_neck.hip): its kernels, the GEMM they share, the launch sequences of a run of
// blocks forward and backward, and the host side every trainable handle has: its device memory (Arena), the cut of a run
// of blocks out of it, and the checks of the parameter and gradient tables.  Everything lives in an anonymous namespace:
// each translation unit that includes this header compiles the kernels it launches into its own code object.
// BatchNorm + ReLU, kernels and launch sequences, is yl_bn.h's, and so are the primitives (f32x4, ld4 / st4, NT, ceil_div).
//
//   block t:  d = dw3x3(x)   z = d . W1^T   h = relu(gamma * (z - mean) * invstd + beta)     (d, z, h are kept for backward)
#ifndef YL_BLOCK_H
#define YL_BLOCK_H
#include <string.h>

#include "../../include/yololite_hip.h"
#include "yl_bn.h"

namespace {

constexpr int GEMM_ROWS = 64;            // q extent of one GEMM workgroup (four waves of 16)

// ---- the 16-bit MFMA operands: a lane's four k values as one 8-byte fragment (v_mfma_f32_16x16x16_f16 / _bf16, fp32
// accumulation).  __builtin_convertvector from f32x4 rounds to nearest even; nothing is clamped.
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 b16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 mfma16(h16x4 a, h16x4 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma16(b16x4 a, b16x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a), __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
}
// the operand type of a GEMM, P: 0 fp32, 1 fp16, 2 bf16 (the handles' fMode; mode_of() reads it off a call's flags)
template <int P> struct Frag16;
template <> struct Frag16<1> { typedef h16x4 T; };
template <> struct Frag16<2> { typedef b16x4 T; };

// ---- level geometry: column n = a * E + e of the head output <-> level tensor [B, A, S, S, E], parameter rows
struct HeadGeom { int A, E, C, SS, F; };
__device__ __forceinline__ long head_y_off(const HeadGeom& g, int m, int n) {
  if (g.A == 1) return (long)m * g.E + n;
  const int a = n / g.E, e = n - a * g.E;
  const int b = m / g.SS, ij = m - b * g.SS;
  return (((long)b * g.A + a) * g.SS + ij) * g.E + e;
}
struct HeadRows {                        // the three output convolutions as one matrix [A * E][F] (+ bias [A * E])
  float *box, *obj, *cls, *box_b, *obj_b, *cls_b;
  HeadGeom g;
  __device__ __forceinline__ long rowidx(int n, int& which) const {
    const int a = n / g.E, e = n - a * g.E;
    which = e < 4 ? 0 : (e == 4 ? 1 : 2);
    return e < 4 ? 4 * a + e : (e == 4 ? a : g.C * a + (e - 5));
  }
  __device__ __forceinline__ float* row(int n) const {
    int k; const long r = rowidx(n, k);
    return (k == 0 ? box : (k == 1 ? obj : cls)) + r * g.F;
  }
  __device__ __forceinline__ float* bias(int n) const {
    int k; const long r = rowidx(n, k);
    return (k == 0 ? box_b : (k == 1 ? obj_b : cls_b)) + r;
  }
};

// ---- operand accessors: load4(idx, r, NI, NR) = elements (idx, r .. r + 3), zero outside idx < NI, r + s < NR
struct RowsVec {                         // (idx, r) = p[idx * ld + r]; 16-byte aligned rows, ld % 4 == 0, NR % 4 == 0
  const float* p; int ld;
  __device__ __forceinline__ f32x4 load4(int idx, int r, int NI, int NR) const {
    if (idx < NI && r < NR) return ld4(p + (long)idx * ld + r);
    return (f32x4){0.f, 0.f, 0.f, 0.f};
  }
};
struct RowsScalar {                      // the same element, a caller's tensor at any 4-byte boundary
  const float* p; int ld;
  __device__ __forceinline__ f32x4 load4(int idx, int r, int NI, int NR) const {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (idx < NI) {
      const float* q = p + (long)idx * ld;
#pragma unroll
      for (int s = 0; s < 4; ++s) if (r + s < NR) v[s] = q[r + s];
    }
    return v;
  }
};
struct ColsScalar {                      // (idx, r) = p[r * ld + idx]
  const float* p; int ld;
  __device__ __forceinline__ f32x4 load4(int idx, int r, int NI, int NR) const {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (idx < NI) {
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (r + s < NR) v[s] = p[(long)(r + s) * ld + idx];
    }
    return v;
  }
};
struct HeadWRows {                       // (n, k) = Wout[n][k]
  HeadRows w;
  __device__ __forceinline__ f32x4 load4(int idx, int r, int NI, int NR) const {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (idx < NI) {
      const float* q = w.row(idx);
#pragma unroll
      for (int s = 0; s < 4; ++s) if (r + s < NR) v[s] = q[r + s];
    }
    return v;
  }
};
struct HeadWCols {                       // (k, n) = Wout[n][k]
  HeadRows w;
  __device__ __forceinline__ f32x4 load4(int idx, int r, int NI, int NR) const {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (idx < NI) {
#pragma unroll
      for (int s = 0; s < 4; ++s) if (r + s < NR) v[s] = w.row(r + s)[idx];
    }
    return v;
  }
};
struct HeadYRows {                       // (m, n) = level tensor element of row m, column n
  const float* y; HeadGeom g;
  __device__ __forceinline__ f32x4 load4(int idx, int r, int NI, int NR) const {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (idx < NI) {
#pragma unroll
      for (int s = 0; s < 4; ++s) if (r + s < NR) v[s] = y[head_y_off(g, idx, r + s)];
    }
    return v;
  }
};
struct HeadYCols {                       // (n, m)
  const float* y; HeadGeom g;
  __device__ __forceinline__ f32x4 load4(int idx, int r, int NI, int NR) const {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (idx < NI) {
#pragma unroll
      for (int s = 0; s < 4; ++s) if (r + s < NR) v[s] = y[head_y_off(g, r + s, idx)];
    }
    return v;
  }
};
// ---- output accessors: store(p, q, v, NP, NQ, split) writes C[p .. p + 3][q]
struct OutRowsVec {                      // c[q * ld + p], NP % 4 == 0
  float* c; int ld;
  __device__ __forceinline__ void store(int p, int q, f32x4 v, int NP, int NQ, int) const {
    if (q < NQ && p < NP) st4(c + (long)q * ld + p, v);
  }
};
struct OutHeadY {                        // the level tensor, bias added
  float* y; HeadRows w;
  __device__ __forceinline__ void store(int p, int q, f32x4 v, int NP, int NQ, int) const {
    if (q >= NQ) return;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (p + s < NP) y[head_y_off(w.g, q, p + s)] = v[s] + *w.bias(p + s);
  }
};
struct OutPartial {                      // part[split][q][p]
  float* part; long stride;
  __device__ __forceinline__ void store(int p, int q, f32x4 v, int NP, int NQ, int split) const {
    if (q >= NQ) return;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (p + s < NP) part[(long)split * stride + (long)q * NP + p + s] = v[s];
  }
};

// grid (ceil(NP / (16 PT)), ceil(NQ / 64), splits); r range of a split: [z * rsplit, min(NR, (z + 1) * rsplit))
// P != 0: both fragments are rounded to the 16-bit type as load4 returns them (the zero fill stays zero) and the lane's
// four r values, the k layout of v_mfma_f32_16x16x16_*, go through ONE MFMA per p-tile in the place of four; C/D is the same.
template <int PT, class PA, class QA, class CA, int P>
__global__ __launch_bounds__(NT) void yl_head_gemm_kernel(PA pa, QA qa, CA ca, int NP, int NQ, int NR, int rsplit) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4, i = lane & 15;
  const int p0 = blockIdx.x * (16 * PT), q0 = blockIdx.y * GEMM_ROWS + wave * 16;
  if (q0 >= NQ) return;                  // no barrier below
  const int rbeg = blockIdx.z * rsplit;
  const int rend = rbeg + rsplit < NR ? rbeg + rsplit : NR;
  f32x4 acc[PT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) acc[pt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int r0 = rbeg; r0 < rend; r0 += 16) {
    const int r = r0 + 4 * kq;
    const f32x4 qv = qa.load4(q0 + i, r, NQ, rend);
    f32x4 pv[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) pv[pt] = pa.load4(p0 + 16 * pt + i, r, NP, rend);
    if constexpr (P == 0) {
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int pt = 0; pt < PT; ++pt)
          acc[pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[pt][s], qv[s], acc[pt], 0, 0, 0);
    } else {
      typedef typename Frag16<P>::T H;
      const H qh = __builtin_convertvector(qv, H);
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) acc[pt] = mfma16(__builtin_convertvector(pv[pt], H), qh, acc[pt]);
    }
  }
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) ca.store(p0 + 16 * pt + 4 * kq, q0 + i, acc[pt], NP, NQ, blockIdx.z);
}

// ---- depthwise 3x3, pad 1, stride 1, weight [F][1][3][3]; FLIP: the transposed convolution (gradient of the input)
template <bool FLIP>
__global__ __launch_bounds__(NT) void yl_head_dw_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       float* __restrict__ out, int M, int S, int F) {
  const int F4 = F >> 2;
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  if (idx >= (long)M * F4) return;
  const int m = (int)(idx / F4), c = (int)(idx - (long)m * F4) * 4;
  const int SS = S * S, b = m / SS, ij = m - b * SS, i = ij / S, j = ij - i * S;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int yy = FLIP ? i - ky + 1 : i + ky - 1;
    if (yy < 0 || yy >= S) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int xx = FLIP ? j - kx + 1 : j + kx - 1;
      if (xx < 0 || xx >= S) continue;
      const f32x4 v = ld4(x + ((long)(b * S + yy) * S + xx) * F + c);
      const int t = ky * 3 + kx;
      const f32x4 wv = {w[(c + 0) * 9 + t], w[(c + 1) * 9 + t], w[(c + 2) * 9 + t], w[(c + 3) * 9 + t]};
      acc = acc + v * wv;
    }
  }
  st4(out + (long)m * F + c, acc);
}

// ---- depthwise weight gradient partials: part[tile][ky * 3 + kx][F] = sum over the tile's rows of dd[m][c] * x[m + tap][c].
// A row reduction in the tiling of yl_bn_colstats_kernel (yl_bn.h): workgroup (tile of STAT_ROWS rows, group of CQ channel
// quads); float64 sums per thread, summed over the row lanes in lane order by the thread of lane 0.
__global__ __launch_bounds__(NT) void yl_head_dw_wgrad_kernel(const float* __restrict__ dd, const float* __restrict__ x,
                                                             double* __restrict__ part, int M, int S, int F, int CQ) {
  __shared__ double red[NT][12];
  const int t = threadIdx.x, cq = t & (CQ - 1), rs = t / CQ, RS = NT / CQ;
  const int c = (blockIdx.y * CQ + cq) * 4;
  const bool on = c < F;
  const int SS = S * S;
  const int m0 = blockIdx.x * STAT_ROWS, m1 = m0 + STAT_ROWS < M ? m0 + STAT_ROWS : M;
  for (int ky = 0; ky < 3; ++ky) {
    double acc[3][4] = {};
    if (on)
      for (int m = m0 + rs; m < m1; m += RS) {
        const int b = m / SS, ij = m - b * SS, i = ij / S, j = ij - i * S, yy = i + ky - 1;
        if (yy < 0 || yy >= S) continue;
        const f32x4 g = ld4(dd + (long)m * F + c);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int xx = j + kx - 1;
          if (xx < 0 || xx >= S) continue;
          const f32x4 v = ld4(x + ((long)(b * S + yy) * S + xx) * F + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[kx][e] += (double)g[e] * (double)v[e];
        }
      }
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[t][kx * 4 + e] = acc[kx][e];
    __syncthreads();
    if (rs == 0 && on) {
      for (int k = 1; k < RS; ++k)
#pragma unroll
        for (int e = 0; e < 12; ++e) red[t][e] += red[k * CQ + cq][e];
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int e = 0; e < 4; ++e) part[((long)blockIdx.x * 9 + ky * 3 + kx) * F + c + e] = red[t][kx * 4 + e];
    }
    __syncthreads();
  }
}

// bias gradient partials: part[tile][NE] = sum over the tile's rows of gy(m, n); thread t: column t % 64, rows t / 64, + 4, ...
__global__ __launch_bounds__(NT) void yl_head_ysum_kernel(const float* __restrict__ gy, HeadGeom g, double* __restrict__ part,
                                                         int M, int NE) {
  __shared__ double red[NT];
  const int t = threadIdx.x, n = blockIdx.y * 64 + (t & 63), rs = t >> 6;
  const int m0 = blockIdx.x * STAT_ROWS, m1 = m0 + STAT_ROWS < M ? m0 + STAT_ROWS : M;
  double s = 0;
  if (n < NE)
    for (int m = m0 + rs; m < m1; m += NT / 64) s += (double)gy[head_y_off(g, m, n)];
  red[t] = s;
  __syncthreads();
  if (rs == 0 && n < NE) part[(long)blockIdx.x * NE + n] = ((red[t] + red[t + 64]) + red[t + 128]) + red[t + 192];
}

// ---- second stages: one thread per output element, the partials summed in tile order in float64
__global__ __launch_bounds__(NT) void yl_head_dw_wsum_kernel(const double* __restrict__ part, int tiles, int F,
                                                            float* __restrict__ out) {
  const int idx = blockIdx.x * NT + threadIdx.x;          // k * F + c
  if (idx >= 9 * F) return;
  const int k = idx / F, c = idx - k * F;
  double s = 0;
  for (int t = 0; t < tiles; ++t) s += part[((long)t * 9 + k) * F + c];
  out[c * 9 + k] = (float)s;
}
// weight-gradient partials [splits][NQ][NP] -> a plain matrix out[q * NP + p], or (head != 0) the weights of the three
// output convolutions: row q = column n of the head; a NULL tensor is not written
__global__ __launch_bounds__(NT) void yl_head_wsum_kernel(const float* __restrict__ part, int splits, int NP, int NQ,
                                                         float* __restrict__ out, HeadRows hw, int head) {
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  const long n = (long)NP * NQ;
  if (idx >= n) return;
  double s = 0;
  for (int z = 0; z < splits; ++z) s += (double)part[(long)z * n + idx];
  if (!head) { out[idx] = (float)s; return; }
  const int q = (int)(idx / NP), p = (int)(idx - (long)q * NP);
  int k; hw.rowidx(q, k);
  if (k == 0 ? hw.box != nullptr : (k == 1 ? hw.obj != nullptr : hw.cls != nullptr)) hw.row(q)[p] = (float)s;
}
__global__ __launch_bounds__(NT) void yl_head_bsum_kernel(const double* __restrict__ part, int tiles, int NE, HeadRows hw) {
  const int n = blockIdx.x * NT + threadIdx.x;
  if (n >= NE) return;
  double s = 0;
  for (int t = 0; t < tiles; ++t) s += part[(long)t * NE + n];
  int k; hw.rowidx(n, k);
  if (k == 0 ? hw.box_b != nullptr : (k == 1 ? hw.obj_b != nullptr : hw.cls_b != nullptr)) *hw.bias(n) = (float)s;
}

int pick_pt(int NP) {                    // p-tiles per wave: 4 (64 columns) or 6 (96), whichever pads NP less
  const int w4 = ceil_div(NP, 64) * 64, w6 = ceil_div(NP, 96) * 96;
  return w6 < w4 ? 6 : 4;
}
// rows per split and number of splits of a weight-gradient GEMM with NP x NQ outputs over M rows: about 1024 workgroups
void split_plan(int M, int NP, int NQ, int* rows, int* splits) {
  const int tiles = ceil_div(NP, 16 * pick_pt(NP)) * ceil_div(NQ, GEMM_ROWS);
  int want = 1024 / tiles;
  want = want < 8 ? 8 : (want > 128 ? 128 : want);
  const int most = ceil_div(M, 64);
  want = want < most ? want : most;
  *rows = ceil_div(ceil_div(M, want), 16) * 16;
  *splits = ceil_div(M, *rows);
}

template <int P, class PA, class QA, class CA>
void launch_gemm(hipStream_t s, PA pa, QA qa, CA ca, int NP, int NQ, int NR, int rsplit, int splits) {
  const int pt = pick_pt(NP);
  const dim3 grid(ceil_div(NP, 16 * pt), ceil_div(NQ, GEMM_ROWS), splits);
  if (pt == 6)
    hipLaunchKernelGGL((yl_head_gemm_kernel<6, PA, QA, CA, P>), grid, dim3(NT), 0, s, pa, qa, ca, NP, NQ, NR, rsplit);
  else
    hipLaunchKernelGGL((yl_head_gemm_kernel<4, PA, QA, CA, P>), grid, dim3(NT), 0, s, pa, qa, ca, NP, NQ, NR, rsplit);
}
// the same launch in a mode known at run time.  AMP = false (the necks, whose 1x1 GEMMs are fp32 only) instantiates
// nothing but P = 0, so their code objects hold no 16-bit kernel
template <bool AMP, class PA, class QA, class CA>
void launch_gemm_in(int mode, hipStream_t s, PA pa, QA qa, CA ca, int NP, int NQ, int NR, int rsplit, int splits) {
  if constexpr (AMP) {
    if (mode == 1) return launch_gemm<1>(s, pa, qa, ca, NP, NQ, NR, rsplit, splits);
    if (mode == 2) return launch_gemm<2>(s, pa, qa, ca, NP, NQ, NR, rsplit, splits);
  }
  launch_gemm<0>(s, pa, qa, ca, NP, NQ, NR, rsplit, splits);
}
// the precision bits of a forward's flags -> P; both: -1
static_assert(YL_HEAD_F16 == YL_DNECK_F16 && YL_HEAD_BF16 == YL_DNECK_BF16, "one mode_of for the heads and the dense neck");
inline int mode_of(uint32_t flags) {
  const bool f = flags & YL_HEAD_F16, b = flags & YL_HEAD_BF16;
  return f && b ? -1 : (f ? 1 : (b ? 2 : 0));
}

// the float64 partial sums of the row reductions, rounded up so that what follows them stays 16-byte aligned
int64_t spart_bytes(int64_t stat_tiles, int64_t F, int64_t NE) {
  return (stat_tiles * (9 * F > NE ? 9 * F : NE) * 8 + 15) & ~(int64_t)15;
}

// ---- a run of blocks.  Buffers: where the activations of each block and the gradients in flight live
struct Buffers {
  float *d[YL_HEAD_MAX_DEPTH], *z[YL_HEAD_MAX_DEPTH], *h[YL_HEAD_MAX_DEPTH], *stats[YL_HEAD_MAX_DEPTH];
  float *ga, *gb, *wpart, *coef;
  double* spart;
};
struct BlockDims { int M, S, F, stat_tiles, wgrad_rows, wgrad_splits; };
template <class Plan>                    // yl_head_plan_info, yl_neck_level_plan
BlockDims dims_of(const Plan& pl, int S, int F) { return {pl.rows, S, F, pl.stat_tiles, pl.wgrad_rows, pl.wgrad_splits}; }

// `blocks` blocks' d, z, h (`act` bytes each) and then their statistics, cut out of the saved buffer at `p`; the entries
// of the blocks beyond are NULL.  -> the cursor behind them
inline char* carve_blocks(char* p, int blocks, size_t act, size_t F, Buffers* bf) {
  for (int t = 0; t < YL_HEAD_MAX_DEPTH; ++t) bf->d[t] = bf->z[t] = bf->h[t] = bf->stats[t] = nullptr;
  for (int t = 0; t < blocks; ++t) {
    bf->d[t] = (float*)p; p += act;
    bf->z[t] = (float*)p; p += act;
    bf->h[t] = (float*)p; p += act;
  }
  for (int t = 0; t < blocks; ++t) { bf->stats[t] = (float*)p; p += 2 * F * 4; }
  return p;
}

// ---- the device memory of one handle: `saved` holds what a forward keeps for backward, `work` the gradients in flight
// and the partial sums.  One forward is held at a time (fValid); both buffers only ever grow.
struct Arena {
  int device;
  int64_t saved_cap, work_cap;           // bytes the two buffers hold
  char *saved, *work;
  int fValid;                            // a forward's activations are held in `saved`
};

// Both buffers hold at least the need afterwards.  Growing waits for everything enqueued, frees BOTH and drops the held
// forward (a backward that finds fValid cleared returns YL_ERR_STATE); a smaller need keeps what is there.
inline yl_status arena_reserve(Arena& a, int64_t need_saved, int64_t need_work) {
  if (hipSetDevice(a.device) != hipSuccess) return YL_ERR_HIP;
  if (need_saved <= a.saved_cap && need_work <= a.work_cap) return YL_OK;
  if (hipDeviceSynchronize() != hipSuccess) return YL_ERR_HIP;
  const int64_t sb = need_saved > a.saved_cap ? need_saved : a.saved_cap;
  const int64_t wb = need_work > a.work_cap ? need_work : a.work_cap;
  hipFree(a.saved); hipFree(a.work);
  a.saved = a.work = nullptr; a.saved_cap = a.work_cap = 0; a.fValid = 0;
  if (hipMalloc((void**)&a.saved, (size_t)sb) != hipSuccess || hipMalloc((void**)&a.work, (size_t)wb) != hipSuccess) {
    hipFree(a.saved); hipFree(a.work);
    a.saved = a.work = nullptr;
    (void)hipGetLastError();
    return YL_ERR_NOMEM;
  }
  a.saved_cap = sb; a.work_cap = wb;
  return YL_OK;
}

// for the destroy functions: leaves the device current and idle, so the owner may free what else it holds
inline void arena_release(Arena& a) {
  hipSetDevice(a.device); hipDeviceSynchronize();
  hipFree(a.saved); hipFree(a.work);
  (void)hipGetLastError();
}

inline yl_status arena_held(const Arena* a, int64_t* saved_bytes, int64_t* workspace_bytes, int32_t* forward_held) {
  if (!a) return YL_ERR_INVALID;
  if (saved_bytes) *saved_bytes = a->saved_cap;
  if (workspace_bytes) *workspace_bytes = a->work_cap;
  if (forward_held) *forward_held = a->fValid;
  return YL_OK;
}

// the parameter table of blocks 0 .. D - 1: every pointer given and num_batches_tracked (an int64) 8-byte aligned.
// The float pointers are ORed into *bits; the caller tests their 4-byte alignment together with its own.
inline bool blocks_params_ok(const yl_head_block* blocks, int D, uintptr_t* bits) {
  for (int t = 0; t < D; ++t) {
    const yl_head_block& b = blocks[t];
    if (!b.dw || !b.pw || !b.gamma || !b.beta || !b.running_mean || !b.running_var || !b.num_batches_tracked) return false;
    *bits |= (uintptr_t)b.dw | (uintptr_t)b.pw | (uintptr_t)b.gamma | (uintptr_t)b.beta | (uintptr_t)b.running_mean |
             (uintptr_t)b.running_var;
    if ((uintptr_t)b.num_batches_tracked & 7u) return false;
  }
  return true;
}

// the gradient table of the same blocks (NULL: not wanted): its pointers ORed into *bits.  -> is anything wanted
inline bool blocks_grads_wanted(const yl_head_block* grads, int D, uintptr_t* bits) {
  uintptr_t any = 0;
  for (int t = 0; t < D; ++t)
    any |= (uintptr_t)grads[t].dw | (uintptr_t)grads[t].pw | (uintptr_t)grads[t].gamma | (uintptr_t)grads[t].beta;
  *bits |= any;
  return any != 0;
}

// block t's BatchNorm over the run's rows; its statistics are those of slot k of the buffers
inline BnLayer bn_of(const yl_head_block& b, const BlockDims& dm, const Buffers& bf, int k) {
  return {dm.M, dm.F, STAT_ROWS, dm.stat_tiles, b.gamma, b.beta, b.running_mean, b.running_var, b.num_batches_tracked, BN_EPS,
          bf.stats[k], bf.spart};
}

// Blocks 0 .. D - 1 on `in`: per block 4 launches (5 with `train`).  `save` keeps every block's d, z, h apart; without it
// every block runs in the first block's buffers.  The last block's output goes to `last_out` if that is given.
// `mode`: the operand type of the 1x1 GEMM (0 with AMP = false).  -> where the last block's output is
template <bool AMP>
const float* blocks_forward(hipStream_t s, const yl_head_block* blocks, int D, const float* in, const Buffers& bf,
                            bool save, bool train, int mode, const BlockDims& dm, float* last_out, int* launches) {
  const int M = dm.M, S = dm.S, F = dm.F;
  const int eg = ceil_div((long)M * (F >> 2), NT);
  int nl = 0;
  for (int t = 0; t < D; ++t) {
    const int k = save ? t : 0;          // nothing is kept without `save`: every block runs in the first block's buffers
    const yl_head_block& b = blocks[t];
    float* hout = (t == D - 1 && last_out) ? last_out : bf.h[k];
    hipLaunchKernelGGL(yl_head_dw_kernel<false>, dim3(eg), dim3(NT), 0, s, in, (const float*)b.dw, bf.d[k], M, S, F);
    launch_gemm_in<AMP>(mode, s, RowsScalar{b.pw, F}, RowsVec{bf.d[k], F}, OutRowsVec{bf.z[k], F}, F, M, F, F, 1);
    nl += 2 + bn_forward<ACT_RELU>(s, bn_of(b, dm, bf, k), train, bf.z[k], nullptr, hout);
    in = hout;
  }
  *launches += nl;
  return in;
}

// the first block something of `grads` is wanted of (D: none)
inline int blocks_first_wanted(const yl_head_block* grads, int D) {
  int first = D;
  for (int t = D - 1; t >= 0; --t) {
    const yl_head_block& g = grads[t];
    if (g.dw || g.pw || g.gamma || g.beta) first = t;
  }
  return first;
}

// The blocks D - 1 .. first backward.  `gin`: the gradient of the last block's output (bf.ga, or a tensor that is only
// read).  x_in: the input of block 0.  dx (may be NULL): where the gradient of block 0's input goes; the caller passes
// first = 0 with it.  The walk stops at the last thing that is wanted.  `mode`: as in blocks_forward, of both 1x1 GEMMs.
template <bool AMP>
void blocks_backward(hipStream_t s, const yl_head_block* params, const yl_head_block* grads, int D, int first,
                     const float* gin, const float* x_in, float* dx, const Buffers& bf, bool train, int mode,
                     const BlockDims& dm, int* launches) {
  const int M = dm.M, S = dm.S, F = dm.F;
  const int eg = ceil_div((long)M * (F >> 2), NT), cq = pick_cq(F);
  HeadRows none;
  memset(&none, 0, sizeof(none));
  int nl = 0;
  for (int t = D - 1; t >= first; --t) {
    const yl_head_block& b = params[t];
    const yl_head_block& g = grads[t];
    const float* xin = t ? bf.h[t - 1] : x_in;
    const float* dh = t == D - 1 ? gin : bf.ga;
    const BnLayer bn = bn_of(b, dm, bf, t);
    // sum g, sum g * xhat: dbeta, dgamma, and the two means the batch statistics carry
    nl += bn_backward_sums<ACT_RELU>(s, bn, train, dh, bf.h[t], bf.z[t], g.gamma, g.beta, bf.coef);
    const bool below = t > first || g.dw || g.pw || (t == 0 && dx);   // anything that needs dz
    if (!below) break;
    nl += bn_backward_dz<ACT_RELU>(s, bn, dh, bf.h[t], bf.z[t], bf.coef, bf.ga);
    if (g.pw) {                          // dW1 = dz^T . d
      launch_gemm_in<AMP>(mode, s, ColsScalar{bf.d[t], F}, ColsScalar{bf.ga, F}, OutPartial{bf.wpart, (long)F * F}, F, F, M,
                          dm.wgrad_rows, dm.wgrad_splits);
      hipLaunchKernelGGL(yl_head_wsum_kernel, dim3(ceil_div((long)F * F, NT)), dim3(NT), 0, s, (const float*)bf.wpart,
                         dm.wgrad_splits, F, F, g.pw, none, 0);
      nl += 2;
    }
    const bool need_dx = t > first || (t == 0 && dx);
    if (!g.dw && !need_dx) break;
    launch_gemm_in<AMP>(mode, s, ColsScalar{b.pw, F}, RowsVec{bf.ga, F}, OutRowsVec{bf.gb, F}, F, M, F, F, 1);   // dd = dz . W1
    ++nl;
    if (g.dw) {
      hipLaunchKernelGGL(yl_head_dw_wgrad_kernel, dim3(dm.stat_tiles, ceil_div(F >> 2, cq)), dim3(NT), 0, s,
                         (const float*)bf.gb, xin, bf.spart, M, S, F, cq);
      hipLaunchKernelGGL(yl_head_dw_wsum_kernel, dim3(ceil_div(9 * F, NT)), dim3(NT), 0, s, (const double*)bf.spart,
                         dm.stat_tiles, F, g.dw);
      nl += 2;
    }
    if (need_dx) {                       // the gradient of the block's input: the next block's dh, or the caller's dx
      hipLaunchKernelGGL(yl_head_dw_kernel<true>, dim3(eg), dim3(NT), 0, s, (const float*)bf.gb, (const float*)b.dw,
                         t ? bf.ga : dx, M, S, F);
      ++nl;
    }
  }
  *launches += nl;
}

}  // namespace
#endif  // YL_BLOCK_H
