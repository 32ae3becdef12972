// Trainable dense FPN neck (reference scripts/model/model_v2.py:15-22 conv_block, :115-127 lateral* / smooth*, :194-203 the
// top-down chain of YOLOLiteMS): forward and backward of all levels on NHWC fp32 rows, M_k = B * S_k * S_k rows per level.
//
//   block:    z = conv3x3(x, W)   h = silu(y),  y = gamma * (z - mean) * invstd + beta        (z, h are kept for backward)
//   backward: g = dh * s(y) * (1 + y * (1 - s(y))), s = sigmoid, y recomputed from z and the statistics; then the
//             BatchNorm backward of yl_bn.h with g in place of the ReLU-masked gradient; dW = sum_m dz (x) x(m + tap);
//             dx = conv3x3(dz, W transposed in (n, c), taps flipped)
//
// Everything around the blocks (laterals, upsample-add and its transpose, lateral gradients, nearest maps) is yl_fpn.h,
// shared with yl_neck.hip.  BatchNorm + SiLU is the ACT_SILU instantiation of yl_bn.h's kernels and launch sequences.
// New here: the convolution (one kernel for forward and input gradient), its weight pack and its weight gradient
// (partials + ordered float64 sum).
//
// Convolution, implicit GEMM in the orientation of yl_head_gemm_kernel (weights: MFMA A operand, pixels: B operand, a lane
// ends with four consecutive output channels of one pixel).  Workgroup (spatial tile of CT x CT pixels of ONE image, block
// of CNB output channels); wave w owns tile rows 2w, 2w + 1.  Per k-block of CKB input channels the tile's (CT + 2)^2
// window is staged in LDS, CXS floats per pixel (CKB + 4: a lane's float4 of pixel i and of pixel i + 2 fall in
// different banks); a window pixel outside the image is written as zero, so no tap ever reads another image's rows or
// the previous row's last column.  Two LDS buffers: the next k-block's window is loaded into registers before the taps
// of this one are computed and written afterwards; one barrier per k-block.
//
// The three 3x3 GEMMs (forward, input gradient, weight gradient) also run with both operands rounded to fp16 or bf16 and
// fp32 accumulation (YL_DNECK_F16 / YL_DNECK_BF16): the same kernels, templated on the operand type (Opnd<P> below).
#include "yl_fpn.h"

namespace {

constexpr int CT = 8, CW = CT + 2;       // spatial tile edge; window edge
constexpr int CKB = 16, CXS = CKB + 4;   // input channels per k-block; LDS floats per window pixel
constexpr int CNB = 64;                  // output channels per workgroup: four 16-wide MFMA tiles
constexpr int CWIN = CW * CW;
constexpr int GB = 64, GXS = GB + 4;     // weight gradient: channels per block edge; LDS floats per pixel

// ---- the operand type of the three 3x3 GEMMs: P = 0 fp32 (v_mfma_f32_16x16x4_f32, everything above), P = 1 fp16,
// P = 2 bf16 (v_mfma_f32_16x16x16_*: the lane's four k values are one 8-byte fragment).  In the 16-bit modes both operands
// are rounded (nearest even) ONCE, where they are staged: the weight by the pack kernel, the window / the x window and the
// dz tile when they are written to LDS, which then holds halves.  Products are exact in fp32 and summed in fp32.
//   Convolution window: a pixel is 16 halves in a pitch of CHP = 24 (12 dwords), a window row starts every CHR = 320 halves
//   (160 dwords).  ds_read_b64 is served per 32-lane half, bank = dword % 64: the half's lanes are 16 pixels (8 columns of
//   two rows) x two 8-byte quads, 4 dwords per pixel, 64 in all.  Pixel (r, j) starts at dword 160 r + 12 j = 4 (8 r + 3 j)
//   mod 64, and 8 r + 3 j mod 16 takes sixteen values for r in {0, 1}, j in 0..7: no conflict (no single pitch does it: the
//   rows are 10 pixels apart and pixels p, p + 16 share a bank group for every multiple of 4 dwords).
//   Weight gradient: the MFMA's k index is the pixel, so LDS is [channel][pixel] and the four pixels of a fragment are
//   contiguous: dz [64][GDP = 72], x [3][64][GXP = 88], copy kx holds window columns kx .. kx + 7 of the ten rows, so a
//   tap's fragment is 8-byte aligned whatever kx.  A half-wave reads 16 channels x 4 dwords; 44 i and 36 i mod 64 are
//   sixteen multiples of 4: no conflict.  The staging writes (ds_write_b64: 16 consecutive lanes, bank = dword % 32) take
//   their 16 lanes over (channel quad parity, column half, row & 3): 16 q' + 2 h + 4 r mod 32, sixteen 2-dword slots.
constexpr int CHP = 24, CHR = 320;
constexpr int GXP = 88, GDP = 72;
// h16x4 / b16x4 / mfma16 and mode_of (flags -> Opnd<P>'s P; -1: both bits) are yl_block.h's, shared with the heads' GEMM

template <int P> struct Opnd;          // E: element in the packed weight and in LDS; Frag: a lane's four k values
template <> struct Opnd<0> {
  typedef float E; typedef f32x4 Frag;
  static constexpr int WIN = CWIN * CXS, XW = CWIN * GXS, DZ = CT * CT * GXS;
  static __device__ __forceinline__ int at(int pw) { return pw * CXS; }
  static __device__ __forceinline__ int at2(int py, int px) { return (py * CW + px) * CXS; }
  static __device__ __forceinline__ Frag get(const float* p) { return ld4(p); }
  static __device__ __forceinline__ void put(float* p, f32x4 v) { st4(p, v); }
  static __device__ __forceinline__ void mma(const Frag (&pv)[4], Frag qv, f32x4 (&acc)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) acc[pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[pt][s], qv[s], acc[pt], 0, 0, 0);
  }
};
template <class T, class T4> struct Opnd16 {
  typedef T E; typedef T4 Frag;
  static constexpr int WIN = CW * CHR, XW = 3 * GB * GXP, DZ = GB * GDP;
  static __device__ __forceinline__ int at(int pw) { return (pw / CW) * CHR + (pw % CW) * CHP; }
  static __device__ __forceinline__ int at2(int py, int px) { return py * CHR + px * CHP; }
  static __device__ __forceinline__ Frag get(const T* p) { return *reinterpret_cast<const T4*>(p); }
  static __device__ __forceinline__ void put(T* p, f32x4 v) { *reinterpret_cast<T4*>(p) = __builtin_convertvector(v, T4); }
  static __device__ __forceinline__ void mma(const Frag (&pv)[4], Frag qv, f32x4 (&acc)[4]) {
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) acc[pt] = mfma16(pv[pt], qv, acc[pt]);
  }
};
template <> struct Opnd<1> : Opnd16<_Float16, h16x4> {};
template <> struct Opnd<2> : Opnd16<__bf16, b16x4> {};

// w [F][F][3][3] (PyTorch: out, in, ky, kx) -> wp [tap][a][b]: T == 0: W[a][b][tap] (a = out, b = in);
// T == 1: W[b][a][8 - tap] (a = in, b = out), the weight of the transposed convolution
template <int P>
__global__ __launch_bounds__(NT) void yl_dneck_pack_kernel(const float* __restrict__ w, typename Opnd<P>::E* __restrict__ wp, int F, int T) {
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  const long FF = (long)F * F;
  if (idx >= 9 * FF) return;
  const int tap = (int)(idx / FF);
  const long ab = idx - tap * FF;
  const int a = (int)(ab / F), b = (int)(ab - (long)a * F);
  wp[idx] = (typename Opnd<P>::E)(T ? w[((long)b * F + a) * 9 + (8 - tap)] : w[((long)a * F + b) * 9 + tap]);
}

// out[b, i, j, n] = sum over taps (ky, kx) and c of wp[tap][n][c] * x[b, i + ky - 1, j + kx - 1, c], zero outside the image.
// grid (B * TX * TX, ceil(F / CNB)); TX = ceil(S / CT)
template <int P>
__global__ __launch_bounds__(NT) void yl_dneck_conv_kernel(const float* __restrict__ x, const typename Opnd<P>::E* __restrict__ wp,
                                                          float* __restrict__ out, int S, int F, int TX) {
  typedef Opnd<P> O;
  __shared__ __attribute__((aligned(16))) typename O::E win[2][O::WIN];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, kq = lane >> 4, i = lane & 15;
  const int b = blockIdx.x / (TX * TX), tr = blockIdx.x - b * TX * TX, ty0 = (tr / TX) * CT, tx0 = (tr % TX) * CT;
  const int n0 = blockIdx.y * CNB;
  // staging: item = window pixel * 4 + channel quad; this thread's items are t and t + NT
  long soff[2]; bool sok[2]; int sq[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int item = t + r * NT, pw = item >> 2;
    sq[r] = (item & 3) * 4;
    const int gy = ty0 - 1 + pw / CW, gx = tx0 - 1 + pw % CW;
    sok[r] = item < CWIN * 4 && gy >= 0 && gy < S && gx >= 0 && gx < S;
    soff[r] = sok[r] ? (((long)b * S + gy) * S + gx) * F + sq[r] : 0;
  }
  const int row = 2 * wave + (i >> 3), col = i & 7;
  const int nkb = (F + CKB - 1) / CKB;
  // acc sums one k-block (9 CKB products per output), tot the k-blocks: a single fp32 chain over all 9 F products
  // (2952 at F = 328, 4608 at F = 512) leaves the project's bar, 4 x the error of torch's fp32 CPU convolution
  f32x4 acc[4], tot[4], sv[2];
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) acc[pt] = tot[pt] = zero;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    sv[r] = (sok[r] && sq[r] < F) ? ld4(x + soff[r] + 0) : zero;
    if (t + r * NT < CWIN * 4) O::put(&win[0][O::at((t + r * NT) >> 2) + sq[r]], sv[r]);
  }
  __syncthreads();
  for (int kb = 0; kb < nkb; ++kb) {
    const int c0 = kb * CKB;
    const bool more = kb + 1 < nkb;
    if (more) {
#pragma unroll
      for (int r = 0; r < 2; ++r) sv[r] = (sok[r] && c0 + CKB + sq[r] < F) ? ld4(x + soff[r] + c0 + CKB) : zero;
    }
    const typename O::E* wb = win[kb & 1];
    const int c = c0 + 4 * kq;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - 3 * ky;
      const typename O::Frag qv = O::get(wb + O::at2(row + ky, col + kx) + 4 * kq);
      typename O::Frag pv[4];
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) {
        const int n = n0 + 16 * pt + i;
        pv[pt] = (n < F && c < F) ? O::get(wp + ((long)tap * F + n) * F + c) : typename O::Frag{};
      }
      O::mma(pv, qv, acc);
    }
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) { tot[pt] = tot[pt] + acc[pt]; acc[pt] = zero; }
    if (more) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
        if (t + r * NT < CWIN * 4) O::put(&win[(kb + 1) & 1][O::at((t + r * NT) >> 2) + sq[r]], sv[r]);
    }
    __syncthreads();
  }
  const int gy = ty0 + row, gx = tx0 + col;
  if (gy < S && gx < S) {
    float* o = out + (((long)b * S + gy) * S + gx) * F;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      const int n = n0 + 16 * pt + 4 * kq;
      if (n < F) st4(o + n, tot[pt]);
    }
  }
}

// Weight-gradient partials: part[split][tap][n][c] = sum over the split's spatial tiles and their pixels m of
// dz[m][n] * x[m + tap][c].  grid (ceil(F / GB) c blocks, ceil(F / GB) n blocks, splits); wave w owns n0 + 16 w .. + 15.
// Per tile the x window (zero outside the image) and the dz tile (zero outside the image) are staged once and all nine
// taps read them: 9 x 4 accumulators per lane.  The MFMA's k index is the pixel: pixel 16 step + 4 kq + s of the tile.
template <int P>
__global__ __launch_bounds__(NT) void yl_dneck_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dz,
                                                           float* __restrict__ part, int S, int F, int TX, int ntiles,
                                                           int tiles_per_split) {
  typedef Opnd<P> O;
  __shared__ __attribute__((aligned(16))) typename O::E xw[O::XW];
  __shared__ __attribute__((aligned(16))) typename O::E dzt[O::DZ];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, kq = lane >> 4, i = lane & 15;
  const int c0 = blockIdx.x * GB, n0 = blockIdx.y * GB;
  const int tbeg = blockIdx.z * tiles_per_split;
  const int tend = tbeg + tiles_per_split < ntiles ? tbeg + tiles_per_split : ntiles;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[9][4];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) acc[tap][pt] = zero;
  for (int tile = tbeg; tile < tend; ++tile) {
    const int b = tile / (TX * TX), tr = tile - b * TX * TX, ty0 = (tr / TX) * CT, tx0 = (tr % TX) * CT;
    __syncthreads();                     // the previous tile's reads are done
    if constexpr (P == 0) {
      for (int item = t; item < CWIN * (GB / 4); item += NT) {
        const int pw = item / (GB / 4), q = (item - pw * (GB / 4)) * 4;
        const int gy = ty0 - 1 + pw / CW, gx = tx0 - 1 + pw % CW;
        const bool ok = gy >= 0 && gy < S && gx >= 0 && gx < S && c0 + q < F;
        st4(&xw[pw * GXS + q], ok ? ld4(x + (((long)b * S + gy) * S + gx) * F + c0 + q) : zero);
      }
      for (int item = t; item < CT * CT * (GB / 4); item += NT) {
        const int pk = item / (GB / 4), q = (item - pk * (GB / 4)) * 4;
        const int gy = ty0 + (pk >> 3), gx = tx0 + (pk & 7);
        const bool ok = gy < S && gx < S && n0 + q < F;
        st4(&dzt[pk * GXS + q], ok ? ld4(dz + (((long)b * S + gy) * S + gx) * F + n0 + q) : zero);
      }
    } else {
      // item = (copy kx, window row r, column half hh, channel quad): four pixels of four channels, transposed to one
      // 8-byte fragment per channel.  Lane bits: quad parity, hh, r & 3, then the quad's other bits (conflict-free writes,
      // and a wave's loads are whole 128-byte runs of eight pixels)
      for (int item = t; item < 9 * 128; item += NT) {
        const int q = ((item & 1) | ((item >> 3) & 14)) * 4, hh = (item >> 1) & 1, rest = item >> 7, kx = rest / 3;
        const int r = ((item >> 2) & 3) + 4 * (rest - 3 * kx);
        if (r >= CW) continue;
        const int gy = ty0 - 1 + r;
        const bool rok = gy >= 0 && gy < S && c0 + q < F;
        f32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int gx = tx0 - 1 + kx + 4 * hh + j;
          v[j] = (rok && gx >= 0 && gx < S) ? ld4(x + (((long)b * S + gy) * S + gx) * F + c0 + q) : zero;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
          O::put(&xw[(kx * GB + q + e) * GXP + r * CT + 4 * hh], (f32x4){v[0][e], v[1][e], v[2][e], v[3][e]});
      }
      for (int item = t; item < CT * CT * 4; item += NT) {
        const int q = ((item & 1) | ((item >> 4) & 14)) * 4, hh = (item >> 1) & 1, r = (item >> 2) & 7;
        const int gy = ty0 + r;
        const bool rok = gy < S && n0 + q < F;
        f32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int gx = tx0 + 4 * hh + j;
          v[j] = (rok && gx < S) ? ld4(dz + (((long)b * S + gy) * S + gx) * F + n0 + q) : zero;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) O::put(&dzt[(q + e) * GDP + r * CT + 4 * hh], (f32x4){v[0][e], v[1][e], v[2][e], v[3][e]});
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int step = 0; step < 4; ++step) {
      if constexpr (P != 0) {            // pixels 16 step + 4 kq .. + 3 are one fragment; tap (ky, kx): copy kx, 8 ky further
        const typename O::Frag qv = O::get(&dzt[(16 * wave + i) * GDP + 16 * step + 4 * kq]);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int ky = tap / 3, kx = tap - 3 * ky;
          const typename O::E* xb = xw + (kx * GB + i) * GXP + 16 * step + 8 * ky + 4 * kq;
#pragma unroll
          for (int pt = 0; pt < 4; ++pt) acc[tap][pt] = mfma16(O::get(xb + 16 * pt * GXP), qv, acc[tap][pt]);
        }
      } else {
        const int prow = 2 * step + (kq >> 1), pcol = 4 * (kq & 1);   // pixel 16 step + 4 kq + s: (prow, pcol + s)
        float qv[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) qv[s] = dzt[(prow * CT + pcol + s) * GXS + 16 * wave + i];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int ky = tap / 3, kx = tap - 3 * ky;
          const float* xb = xw + ((prow + ky) * CW + pcol + kx) * GXS + i;
#pragma unroll
          for (int pt = 0; pt < 4; ++pt)
#pragma unroll
            for (int s = 0; s < 4; ++s)
              acc[tap][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[s * GXS + 16 * pt], qv[s], acc[tap][pt], 0, 0, 0);
        }
      }
    }
  }
  const int n = n0 + 16 * wave + i;
  if (n >= F) return;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      const int c = c0 + 16 * pt + 4 * kq;
      if (c < F) st4(part + (((long)blockIdx.z * 9 + tap) * F + n) * F + c, acc[tap][pt]);
    }
}

// the partials summed in split order in float64 -> dW in PyTorch layout [F][F][3][3]; one thread per element
__global__ __launch_bounds__(NT) void yl_dneck_wsum_kernel(const float* __restrict__ part, int splits, int F, float* __restrict__ out) {
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  const long FF = (long)F * F;
  if (idx >= 9 * FF) return;
  const long nc = idx / 9;
  const int tap = (int)(idx - nc * 9);
  double s = 0;
  for (int z = 0; z < splits; ++z) s += (double)part[((long)z * 9 + tap) * FF + nc];
  out[idx] = (float)s;
}

// the 3x3 weight gradient's cut of `tiles` spatial tiles into runs: about 512 workgroups; the partials are 9 F F floats per split
void w3_split(int64_t F, int64_t tiles, int32_t* tiles_per_split, int32_t* splits) {
  const int64_t blocks = (int64_t)ceil_div(F, GB) * ceil_div(F, GB);
  int64_t want = 512 / blocks;
  want = want < 1 ? 1 : (want > 64 ? 64 : want);
  want = want < tiles ? want : tiles;
  *tiles_per_split = ceil_div(tiles, want);
  *splits = ceil_div(tiles, *tiles_per_split);
}

}  // namespace

struct yl_dneck {
  Arena mem;                             // yl_block.h
  yl_neck_cfg cfg;
  MapTables maps;                        // yl_fpn.h
  int fB, fS[YL_NECK_MAX_LEVELS], fTrain;   // the forward whose activations are held (mem.fValid)
  int fMode;                             // and the operand type of its 3x3 GEMMs (Opnd<fMode>): the backward's too
};

extern "C" {

yl_status yl_dneck_plan(const yl_neck_cfg* cfg, int32_t batch, const int32_t* sizes, yl_dneck_plan_info* out) {
  if (!cfg_ok(cfg) || !out || !sizes || batch < 1) return YL_ERR_INVALID;
  for (int k = 0; k < cfg->num_levels; ++k)
    if (sizes[k] < 1) return YL_ERR_INVALID;
  if (!cfg_supported(cfg)) return YL_ERR_UNSUPPORTED;
  memset(out, 0, sizeof(*out));
  out->stat_rows = STAT_ROWS; out->gemm_rows = GEMM_ROWS; out->conv_tile = CT;
  const int64_t F = cfg->channels;
  int64_t Mmax = 0, smax = 0, wmax = 0;
  for (int k = 0; k < cfg->num_levels; ++k) {
    const int64_t M = (int64_t)batch * sizes[k] * sizes[k], Cin = cfg->in_channels[k];
    if (!level_rows_ok(M, F, Cin)) return YL_ERR_UNSUPPORTED;
    yl_dneck_level_plan& lp = out->level[k];
    lp.rows = (int32_t)M;
    lp.stat_tiles = ceil_div(M, STAT_ROWS); lp.gemm_tiles = ceil_div(M, GEMM_ROWS);
    const int64_t TX = ceil_div(sizes[k], CT), tiles = (int64_t)batch * TX * TX;
    lp.conv_tiles = (int32_t)tiles;
    split_plan((int)M, (int)Cin, (int)F, &lp.lgrad_rows, &lp.lgrad_splits);
    w3_split(F, tiles, &lp.w3grad_tiles, &lp.w3grad_splits);
    lp.saved_bytes = (1 + 2 * (int64_t)cfg->depth) * M * F * 4 + cfg->depth * 2 * F * 4;
    out->saved_bytes += lp.saved_bytes;
    Mmax = M > Mmax ? M : Mmax;
    const int64_t sp = round16((int64_t)lp.stat_tiles * 2 * F * 8);
    smax = sp > smax ? sp : smax;
    const int64_t w3 = (int64_t)lp.w3grad_splits * 9 * F * F * 4, lpb = (int64_t)lp.lgrad_splits * F * Cin * 4;
    const int64_t wp = round16(w3 > lpb ? w3 : lpb);
    wmax = wp > wmax ? wp : wmax;
  }
  out->table_bytes = map_table_bytes(cfg->num_levels, sizes);
  out->nosave_bytes = 3 * Mmax * F * 4 + 2 * F * 4;
  out->workspace_bytes = 3 * Mmax * F * 4 + smax + 2 * F * 4 + 9 * F * F * 4 + wmax;
  return YL_OK;
}

void yl_dneck_destroy(yl_dneck* h) {
  if (!h) return;
  arena_release(h->mem);
  hipFree(h->maps.dev); (void)hipGetLastError();
  delete h;
}

yl_status yl_dneck_held(const yl_dneck* h, int64_t* saved_bytes, int64_t* workspace_bytes, int32_t* forward_held) {
  return arena_held(h ? &h->mem : nullptr, saved_bytes, workspace_bytes, forward_held);
}

yl_status yl_dneck_create(int32_t device, const yl_neck_cfg* cfg, yl_dneck** out) {
  if (!out || !cfg_ok(cfg)) return YL_ERR_INVALID;
  if (!cfg_supported(cfg)) return YL_ERR_UNSUPPORTED;
  if (hipSetDevice(device) != hipSuccess) return YL_ERR_HIP;
  yl_dneck* h = new (std::nothrow) yl_dneck();
  if (!h) return YL_ERR_NOMEM;
  h->mem.device = device; h->cfg = *cfg;
  *out = h;
  return YL_OK;
}

}  // extern "C"

namespace {

struct DBuffers {
  float *t[YL_NECK_MAX_LEVELS];
  float *z[YL_NECK_MAX_LEVELS][YL_NECK_MAX_DEPTH], *h[YL_NECK_MAX_LEVELS][YL_NECK_MAX_DEPTH];
  float* stats[YL_NECK_MAX_LEVELS][YL_NECK_MAX_DEPTH];
  float *ga, *gb, *gt, *coef, *wpack, *wpart;
  double* spart;
  LevelMaps maps[YL_NECK_MAX_LEVELS];
};

// the handle's memory for (batch, sizes), cut as yl_dneck_plan counts it; `save`: every level and block apart
yl_status ensure(yl_dneck* h, int B, const int32_t* sizes, bool save, yl_dneck_plan_info* pl, DBuffers* nb) {
  yl_status st = yl_dneck_plan(&h->cfg, B, sizes, pl);
  if (st != YL_OK) return st;
  st = arena_reserve(h->mem, save ? pl->saved_bytes : pl->nosave_bytes, pl->workspace_bytes);
  if (st != YL_OK) return st;
  const int L = h->cfg.num_levels, D = h->cfg.depth;
  const size_t F = h->cfg.channels;
  st = maps_ensure(h->maps, L, sizes, pl->table_bytes, nb->maps);
  if (st != YL_OK) return st;
  size_t amax = 0, smax = 0;
  for (int k = 0; k < L; ++k) {
    const size_t a = (size_t)pl->level[k].rows * F * 4, sp = (size_t)round16((int64_t)pl->level[k].stat_tiles * 2 * F * 8);
    amax = a > amax ? a : amax;
    smax = sp > smax ? sp : smax;
  }
  char* w = h->mem.work;
  nb->ga = (float*)w; w += amax;
  nb->gb = (float*)w; w += amax;
  nb->gt = (float*)w; w += amax;
  nb->spart = (double*)w; w += smax;
  nb->coef = (float*)w; w += 2 * F * 4;
  nb->wpack = (float*)w; w += 9 * F * F * 4;
  nb->wpart = (float*)w;
  char* p = h->mem.saved;
  for (int k = 0; k < L; ++k) {
    const size_t act = (size_t)pl->level[k].rows * F * 4;
    if (!save) p = h->mem.saved;         // every level in the same memory
    nb->t[k] = (float*)p; p += act;
    const int blocks = save ? D : 1;
    for (int i = 0; i < YL_NECK_MAX_DEPTH; ++i) nb->z[k][i] = nb->h[k][i] = nb->stats[k][i] = nullptr;
    for (int i = 0; i < blocks; ++i) {
      nb->z[k][i] = (float*)p; p += act;
      nb->h[k][i] = (float*)p; p += act;
    }
    for (int i = 0; i < blocks; ++i) { nb->stats[k][i] = (float*)p; p += 2 * F * 4; }
  }
  return YL_OK;
}

bool params_ok(const yl_neck_cfg& c, const yl_dneck_tensors* t) {
  if (!t) return false;
  uintptr_t any = 0;
  for (int k = 0; k < c.num_levels; ++k) {
    const yl_dneck_level& l = t->level[k];
    if (!l.lat_w || !l.lat_b) return false;
    any |= (uintptr_t)l.lat_w | (uintptr_t)l.lat_b;
    for (int i = 0; i < c.depth; ++i) {
      const yl_dneck_block& b = l.block[i];
      if (!b.w || !b.gamma || !b.beta || !b.running_mean || !b.running_var || !b.num_batches_tracked) return false;
      any |= (uintptr_t)b.w | (uintptr_t)b.gamma | (uintptr_t)b.beta | (uintptr_t)b.running_mean | (uintptr_t)b.running_var;
      if ((uintptr_t)b.num_batches_tracked & 7u) return false;
    }
  }
  return !(any & 3u);
}

// pack + convolution of one level: 2 launches.  T: the transposed convolution (the gradient of the input).  The packed
// weight of Opnd<P> lies at the start of `wpack` (9 F F elements: the 16-bit ones take half of it)
template <int P>
void conv3x3_as(hipStream_t s, const float* w, float* wpack, const float* x, float* out, int B, int S, int F, int T) {
  typedef typename Opnd<P>::E E;
  const int TX = ceil_div(S, CT);
  hipLaunchKernelGGL(yl_dneck_pack_kernel<P>, dim3(ceil_div(9L * F * F, NT)), dim3(NT), 0, s, w, (E*)wpack, F, T);
  hipLaunchKernelGGL(yl_dneck_conv_kernel<P>, dim3(B * TX * TX, ceil_div(F, CNB)), dim3(NT), 0, s, x, (const E*)wpack, out, S, F, TX);
}
void conv3x3(int mode, hipStream_t s, const float* w, float* wpack, const float* x, float* out, int B, int S, int F, int T) {
  if (mode == 1) conv3x3_as<1>(s, w, wpack, x, out, B, S, F, T);
  else if (mode == 2) conv3x3_as<2>(s, w, wpack, x, out, B, S, F, T);
  else conv3x3_as<0>(s, w, wpack, x, out, B, S, F, T);
}

// partials + ordered sum of one block's weight gradient: 2 launches
template <int P>
void wgrad3x3_as(hipStream_t s, const float* x, const float* dz, float* wpart, float* dw, int S, int F, int tiles,
                 int tiles_per_split, int splits) {
  const int gbk = ceil_div(F, GB), TX = ceil_div(S, CT);
  hipLaunchKernelGGL(yl_dneck_wgrad_kernel<P>, dim3(gbk, gbk, splits), dim3(NT), 0, s, x, dz, wpart, S, F, TX, tiles, tiles_per_split);
  hipLaunchKernelGGL(yl_dneck_wsum_kernel, dim3(ceil_div(9L * F * F, NT)), dim3(NT), 0, s, (const float*)wpart, splits, F, dw);
}
void wgrad3x3(int mode, hipStream_t s, const float* x, const float* dz, float* wpart, float* dw, int S, int F, int tiles,
              int tiles_per_split, int splits) {
  if (mode == 1) wgrad3x3_as<1>(s, x, dz, wpart, dw, S, F, tiles, tiles_per_split, splits);
  else if (mode == 2) wgrad3x3_as<2>(s, x, dz, wpart, dw, S, F, tiles, tiles_per_split, splits);
  else wgrad3x3_as<0>(s, x, dz, wpart, dw, S, F, tiles, tiles_per_split, splits);
}

// a block's BatchNorm over the level's rows
BnLayer bn_of(const yl_dneck_block& b, const yl_dneck_level_plan& lp, int F, float* stats, double* spart) {
  return {lp.rows, F, STAT_ROWS, lp.stat_tiles, b.gamma, b.beta, b.running_mean, b.running_var, b.num_batches_tracked, BN_EPS, stats,
          spart};
}

// the first block something of `g` is wanted of (D: none)
int first_wanted(const yl_dneck_block* g, int D) {
  int first = D;
  for (int t = D - 1; t >= 0; --t)
    if (g[t].w || g[t].gamma || g[t].beta) first = t;
  return first;
}

}  // namespace

extern "C" {

yl_status yl_dneck_forward(yl_dneck* h, const yl_dneck_tensors* params, const float* const* c_dev, int32_t batch,
                           const int32_t* sizes, uint32_t flags, float* const* p_dev, void* stream, int32_t* launches) {
  const int mode = mode_of(flags);
  if (!h || !c_dev || !p_dev || !sizes || mode < 0 || !params_ok(h->cfg, params)) return YL_ERR_INVALID;
  const int L = h->cfg.num_levels, D = h->cfg.depth, F = h->cfg.channels;
  const bool train = flags & YL_HEAD_TRAIN, save = flags & YL_HEAD_SAVE;
  for (int k = 0; k < L; ++k) {
    if (!c_dev[k] || !p_dev[k] || sizes[k] < 1) return YL_ERR_INVALID;
    if (((uintptr_t)c_dev[k] & 15u) || ((uintptr_t)p_dev[k] & 15u)) return YL_ERR_UNSUPPORTED;
    if (train && (int64_t)batch * sizes[k] * sizes[k] < 2) return YL_ERR_INVALID;   // no variance of one value
  }
  yl_dneck_plan_info pl;
  DBuffers nb;
  const yl_status st = ensure(h, batch, sizes, save, &pl, &nb);
  if (st != YL_OK) return st;
  hipStream_t s = (hipStream_t)stream;
  int nl = 0;
  h->mem.fValid = 0;
  for (int k = L - 1; k >= 0; --k) {
    const yl_dneck_level& lv = params->level[k];
    const yl_dneck_level_plan& lp = pl.level[k];
    const int M = lp.rows, Cin = h->cfg.in_channels[k], S = sizes[k];
    lateral_forward(s, lv.lat_w, lv.lat_b, c_dev[k], nb.t[k], k + 1 < L ? p_dev[k + 1] : nullptr, nb.maps[k].src, F, M, Cin, S,
                    k + 1 < L ? sizes[k + 1] : 0);
    ++nl;
    const float* in = nb.t[k];
    for (int t = 0; t < D; ++t) {
      const int i = save ? t : 0;        // nothing is kept without `save`: every block runs in the first block's buffers
      const yl_dneck_block& b = lv.block[t];
      // with `save` the last block writes the handle's h and p_k is a copy of it; without, it writes p_k
      float* hout = (t == D - 1 && !save) ? p_dev[k] : nb.h[k][i];
      conv3x3(mode, s, b.w, nb.wpack, in, nb.z[k][i], batch, S, F, 0);
      nl += 2 + bn_forward<ACT_SILU>(s, bn_of(b, lp, F, nb.stats[k][i], nb.spart), train, nb.z[k][i], nullptr, hout);
      in = hout;
    }
    if (save && hipMemcpyAsync(p_dev[k], in, (size_t)M * F * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return YL_ERR_HIP;
  }
  if (launches) *launches = nl;
  if (hipGetLastError() != hipSuccess) return YL_ERR_HIP;
  if (save) {
    h->fB = batch; h->fTrain = train ? 1 : 0; h->fMode = mode; h->mem.fValid = 1;
    for (int k = 0; k < L; ++k) h->fS[k] = sizes[k];
  }
  return YL_OK;
}

yl_status yl_dneck_backward(yl_dneck* h, const yl_dneck_tensors* params, const yl_dneck_tensors* grads,
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
    const yl_dneck_level& g = grads->level[k];
    uintptr_t any = (uintptr_t)g.lat_w | (uintptr_t)g.lat_b;
    for (int t = 0; t < D; ++t) any |= (uintptr_t)g.block[t].w | (uintptr_t)g.block[t].gamma | (uintptr_t)g.block[t].beta;
    gany |= any;
    if (any || dc) K = k;
  }
  if (gany & 3u) return YL_ERR_UNSUPPORTED;            // before the first launch: nothing of the caller's is written
  if (!h->mem.fValid || h->fB != batch) return YL_ERR_STATE;
  for (int k = 0; k < L; ++k)
    if (h->fS[k] != sizes[k]) return YL_ERR_STATE;
  yl_dneck_plan_info pl;
  DBuffers nb;
  const yl_status st = ensure(h, batch, sizes, true, &pl, &nb);
  if (st != YL_OK) return st;
  if (!h->mem.fValid) return YL_ERR_STATE;
  hipStream_t s = (hipStream_t)stream;
  const bool train = h->fTrain != 0;
  int nl = 0;
  for (int k = 0; k <= K; ++k) {
    const yl_dneck_level& lv = params->level[k];
    const yl_dneck_level& g = grads->level[k];
    const yl_dneck_level_plan& lp = pl.level[k];
    const int M = lp.rows, Cin = h->cfg.in_channels[k], S = sizes[k];
    float* dc = dc_dev ? dc_dev[k] : nullptr;
    float *cur = nb.ga, *other = nb.gb;  // the two gradients in flight: dz of a block in `cur`, its input's in `other`
    const float* dh = gp_dev[k];
    if (k > 0) {                         // G_k = gp_k + up^T(gt_{k-1}): level k - 1 was walked down to its gt
      hipLaunchKernelGGL(yl_neck_upadd_bwd_kernel, dim3(ceil_div((long)M * (F >> 2), NT)), dim3(NT), 0, s,
                         (const float*)nb.gt, gp_dev[k], cur, nb.maps[k - 1].lo, nb.maps[k - 1].hi, M, S, sizes[k - 1], F);
      ++nl;
      dh = cur;
    }
    const bool lateral = g.lat_w || g.lat_b || dc;
    const bool need_gt = lateral || k < K;
    const int first = need_gt ? 0 : first_wanted(g.block, D);
    for (int t = D - 1; t >= first; --t) {
      const yl_dneck_block& b = lv.block[t];
      const yl_dneck_block& gb = g.block[t];
      const float* xin = t ? nb.h[k][t - 1] : nb.t[k];
      const BnLayer bn = bn_of(b, lp, F, nb.stats[k][t], nb.spart);
      // sum g, sum g * xhat: dbeta, dgamma, and the two means the batch statistics carry
      nl += bn_backward_sums<ACT_SILU>(s, bn, train, dh, nb.h[k][t], nb.z[k][t], gb.gamma, gb.beta, nb.coef);
      const bool need_dx = t > first || (t == 0 && need_gt);
      if (!gb.w && !need_dx) break;
      nl += bn_backward_dz<ACT_SILU>(s, bn, dh, nb.h[k][t], nb.z[k][t], nb.coef, cur);
      if (gb.w) {                        // dW[n][c][tap] = sum_m dz[m][n] * x[m + tap][c]
        wgrad3x3(h->fMode, s, xin, cur, nb.wpart, gb.w, S, F, lp.conv_tiles, lp.w3grad_tiles, lp.w3grad_splits);
        nl += 2;
      }
      if (!need_dx) break;
      float* dx = t ? other : nb.gt;     // the gradient of the block's input: the next block's dh, or gt_k
      conv3x3(h->fMode, s, b.w, nb.wpack, cur, dx, batch, S, F, 1);
      nl += 2;
      if (t) { dh = dx; float* sw = cur; cur = other; other = sw; }
    }
    if (lateral)
      lateral_backward(s, lv.lat_w, g.lat_w, g.lat_b, dc, c_dev[k], nb.gt, nb.wpart, nb.spart, F, Cin, M, S, lp.stat_tiles,
                       lp.lgrad_rows, lp.lgrad_splits, &nl);
  }
  if (launches) *launches = nl;
  return hipGetLastError() == hipSuccess ? YL_OK : YL_ERR_HIP;
}

yl_status yl_dneck_conv3x3(yl_dneck* h, int32_t pass, uint32_t mode, const float* a_dev, const float* b_dev,
                           float* out_dev, int32_t batch, int32_t size, void* stream, int32_t* launches) {
  if (!h || !a_dev || !b_dev || !out_dev || batch < 1 || size < 1) return YL_ERR_INVALID;
  if (pass != YL_DNECK_PASS_FORWARD && pass != YL_DNECK_PASS_DGRAD && pass != YL_DNECK_PASS_WGRAD) return YL_ERR_INVALID;
  if (mode != 0 && mode != YL_DNECK_F16 && mode != YL_DNECK_BF16) return YL_ERR_INVALID;
  if (((uintptr_t)a_dev | (uintptr_t)b_dev | (uintptr_t)out_dev) & 15u) return YL_ERR_UNSUPPORTED;
  const int64_t F = h->cfg.channels, TX = ceil_div(size, CT), tiles = (int64_t)batch * TX * TX;
  if (!level_rows_ok((int64_t)batch * size * size, F, F)) return YL_ERR_UNSUPPORTED;
  int32_t per = 0, splits = 0;
  w3_split(F, tiles, &per, &splits);
  const int64_t wp = 9 * F * F * 4;
  const yl_status st = arena_reserve(h->mem, 0, wp + round16((int64_t)splits * wp));
  if (st != YL_OK) return st;
  hipStream_t s = (hipStream_t)stream;
  float *wpack = (float*)h->mem.work, *wpart = (float*)(h->mem.work + wp);
  const int P = mode_of(mode);
  if (pass == YL_DNECK_PASS_WGRAD) wgrad3x3(P, s, a_dev, b_dev, wpart, out_dev, size, (int)F, (int)tiles, per, splits);
  else conv3x3(P, s, b_dev, wpack, a_dev, out_dev, batch, size, (int)F, pass == YL_DNECK_PASS_DGRAD);
  if (launches) *launches = 2;
  return hipGetLastError() == hipSuccess ? YL_OK : YL_ERR_HIP;
}

}  // extern "C"
