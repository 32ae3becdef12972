// Convolution kernels for gfx950 (MI355X / CDNA4), fp32 in / fp32 accumulate.
//
//   yl_conv_mfma_kernel  dense kxk conv (groups=1) as an implicit GEMM on v_mfma_f32_16x16x4_f32,
//                        NHWC, im2col-free.  Computes D[n][p] = sum_k W[n][k] * X[p][k] (weights are
//                        the MFMA A operand, activations the B operand) so that every lane ends up
//                        with 4 CONSECUTIVE output channels of one pixel -> one float4 store per
//                        16x16 tile, bias/act/residual/upsample-add applied in registers.
//                        Optional depthwise kxk prologue computed on the fly in the B-operand path
//                        (dw -> pw pairs of the reference's DWConvBlock / timm UIB never touch HBM
//                        between the two convs).
//   yl_stem_mfma_kernel  3x3 Cin=3 conv reading the NCHW network input (K=27 padded to 28), weights
//                        resident in registers as MFMA A fragments, writes NHWC.
//   yl_dw_kernel         stand-alone depthwise kxk, NHWC, float4 over channels.
//
// The k dimension of the MFMA is permuted: inside each block of 16 input channels lane l supplies
// channels 4*(l>>4)..4*(l>>4)+3 of pixel (l&15) from ONE float4 load and feeds them to 4 successive
// MFMAs; the host packs the weights in the matching order ([tap][kblock][ntile][lane][4]) so that
// the A fragments are a single conflict-free ds_read_b128 per 16x16x16 step.
//
// Replaces nn.Conv2d/BatchNorm2d(eval, folded)/ReLU/ReLU6/SiLU, F.interpolate(nearest)+add and the
// head's view/cat/permute of the reference (scripts/model/model_v2.py:15-53,179-192,337-350) and of
// the timm backbones it wraps (model_v2.py:94-100,266-272).
// Second compilation with -DYL_BF16=1 (csrc/build.py) produces the bf16-MFMA variant of this translation unit
// under distinct symbol names; yl_api.hip picks one per context (yl_set_option "mfma_bf16").
#include "yl_lp.h"
#if YL_BF16
#define yl_conv_mfma_kernel YL_LP_NAME(yl_conv_mfma_kernel)
#define yl_conv_dwh_kernel YL_LP_NAME(yl_conv_dwh_kernel)
#define yl_uib_kernel YL_LP_NAME(yl_uib_kernel)
#define yl_stem_mfma_kernel YL_LP_NAME(yl_stem_mfma_kernel)
#define yl_dw_kernel YL_LP_NAME(yl_dw_kernel)
#define yl_dw_tile_kernel YL_LP_NAME(yl_dw_tile_kernel)
#define yl_launch_conv YL_LP_NAME(yl_launch_conv)
#define yl_launch_conv_multi YL_LP_NAME(yl_launch_conv_multi)
#define yl_launch_stem YL_LP_NAME(yl_launch_stem)
#define yl_launch_dw YL_LP_NAME(yl_launch_dw)
#define yl_conv_init YL_LP_NAME(yl_conv_init)
#define yl_uib_supported YL_LP_NAME(yl_uib_supported)
#define yl_uib_lds_bytes YL_LP_NAME(yl_uib_lds_bytes)
#define yl_launch_conv_dwc YL_LP_NAME(yl_launch_conv_dwc)
#define yl_launch_conv_pwt YL_LP_NAME(yl_launch_conv_pwt)
#define yl_launch_conv_pwt_multi YL_LP_NAME(yl_launch_conv_pwt_multi)
#define yl_launch_conv_kxk YL_LP_NAME(yl_launch_conv_kxk)
#define yl_launch_conv_pws YL_LP_NAME(yl_launch_conv_pws)
#define yl_launch_conv_ir YL_LP_NAME(yl_launch_conv_ir)
#define yl_launch_conv_wino YL_LP_NAME(yl_launch_conv_wino)
#define yl_launch_conv_dwk YL_LP_NAME(yl_launch_conv_dwk)
#define yl_launch_conv_dws YL_LP_NAME(yl_launch_conv_dws)
#define yl_launch_conv_dwt YL_LP_NAME(yl_launch_conv_dwt)
#define yl_dwc_form YL_LP_NAME(yl_dwc_form)
#define yl_dwt_form YL_LP_NAME(yl_dwt_form)
#define yl_dwk_form YL_LP_NAME(yl_dwk_form)
#define yl_dws_form YL_LP_NAME(yl_dws_form)
#define yl_dw_form YL_LP_NAME(yl_dw_form)
#define yl_dw_alone_form YL_LP_NAME(yl_dw_alone_form)
#endif
#include <stdio.h>
#include <stdlib.h>
#include "yl_internal.h"
#include <math.h>

#include "yl_dev.h"
#include "yl_decode.h"
#include "yl_epi.h"

enum { YL_CM_PW = 0, YL_CM_KXK = 1, YL_CM_DWPRO = 2, YL_CM_DW3 = 3, YL_CM_DW5 = 5,
       YL_CM_PWSC = 6 /* 1x1 conv whose input is multiplied by a squeeze-excite gate [B][Cin] (YlConvP::scale) */ };

// ------------------------------------------------------------------------------------------------
// B-operand fetch: 4 consecutive input channels [c, c+4) of the lane's pixel for tap (ky,kx).
// Branch-free: addresses are clamped into the tensor and out-of-range values are zeroed by a select,
// so the hot loop stays straight-line code (loads issue early, MFMAs back to back).
// (YlPix and the float4 epilogues live in yl_epi.h, shared with yl_convc.hip.)
template <int MODE>
__device__ __forceinline__ f32x4 yl_fetch(const YlConvP& p, const YlPix& px, int ky, int kx, int c,
                                          const float* dwl /*LDS: [taps][Cin] weights then [Cin] bias*/) {
  const bool cin_ok = c < p.Cin;
  const int cs = cin_ok ? c : (p.Cin - 4);
  // out-of-range taps / channels load from a zero buffer: the select happens on the ADDRESS, so the
  // loaded registers are first touched by their consumer and the load latency stays hidden
  if (MODE == YL_CM_PW) {
    return yl_ld4(cin_ok ? p.x + px.lin * p.Cin + cs : p.zeros);
  } else if (MODE == YL_CM_PWSC) {
    // x * gate first (one fp32 rounding, as timm's `x * self.gate(x_se)`), then the GEMM
    return yl_ld4(cin_ok ? p.x + px.lin * p.Cin + cs : p.zeros) * yl_ld4(p.scale + (size_t)px.b * p.Cin + cs);
  } else if (MODE == YL_CM_KXK) {
    // p.H/p.W are the dims of the (virtually upsampled) tensor the conv sees; the stored tensor is
    // (H >> in_shift) x (W >> in_shift): nearest-neighbour upsampling folded into the addressing
    const int iy = px.oy * p.stride - p.pad_t + ky;
    const int ix = px.ox * p.stride - p.pad_l + kx;
    const bool in = cin_ok && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
    const int sh = p.in_shift;
    return yl_ld4(in ? p.x + (((size_t)px.b * (p.H >> sh) + (iy >> sh)) * (p.W >> sh) + (ix >> sh)) * p.Cin + cs
                     : p.zeros);
  } else {  // depthwise prologue feeding a 1x1 conv: value of the dw output at (oy,ox)
    // depthwise taps and bias come from LDS (staged once per block): the vector-memory pipe only
    // carries the activation taps
    f32x4 s = yl_ld4(dwl + p.dw_k * p.dw_k * p.Cin + cs);
    const int y0 = px.oy * p.dw_stride - p.dw_pad_t;
    const int x0 = px.ox * p.dw_stride - p.dw_pad_l;
    const yl_act_t* xb = p.x + (size_t)px.b * p.H * p.W * p.Cin + cs;
    const float* wb = dwl + cs;
    if (MODE == YL_CM_DW5) {
      // 5x5: one row of taps (5 loads) in flight at a time keeps the register footprint small
#pragma unroll 1
      for (int dy = 0; dy < 5; ++dy) {
        const int iy = y0 + dy;
        const bool yin = iy >= 0 && iy < p.H;
        const int iyc = min(max(iy, 0), p.H - 1);
        f32x4 v[5];
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) {
          const int ix = x0 + dx;
          const bool in = yin && ix >= 0 && ix < p.W;
          v[dx] = yl_ld4(in ? xb + ((size_t)iyc * p.W + ix) * p.Cin : p.zeros);
        }
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) {
          const f32x4 w = yl_ld4(wb + (dy * 5 + dx) * p.Cin);
          s.x = fmaf(v[dx].x, w.x, s.x); s.y = fmaf(v[dx].y, w.y, s.y);
          s.z = fmaf(v[dx].z, w.z, s.z); s.w = fmaf(v[dx].w, w.w, s.w);
        }
      }
    } else if (MODE == YL_CM_DW3) {
      // compile-time kernel size: every tap load is issued before the first use (memory-level parallelism)
      constexpr int DK = 3;
      f32x4 v[DK][DK];
#pragma unroll
      for (int dy = 0; dy < DK; ++dy) {
        const int iy = y0 + dy;
        const bool yin = iy >= 0 && iy < p.H;
        const int iyc = min(max(iy, 0), p.H - 1);
#pragma unroll
        for (int dx = 0; dx < DK; ++dx) {
          const int ix = x0 + dx;
          const bool in = yin && ix >= 0 && ix < p.W;
          v[dy][dx] = yl_ld4(in ? xb + ((size_t)iyc * p.W + ix) * p.Cin : p.zeros);
        }
      }
#pragma unroll
      for (int dy = 0; dy < DK; ++dy)
#pragma unroll
        for (int dx = 0; dx < DK; ++dx) {
          const f32x4 w = yl_ld4(wb + (dy * DK + dx) * p.Cin);
          s.x = fmaf(v[dy][dx].x, w.x, s.x); s.y = fmaf(v[dy][dx].y, w.y, s.y);
          s.z = fmaf(v[dy][dx].z, w.z, s.z); s.w = fmaf(v[dy][dx].w, w.w, s.w);
        }
    } else {
      for (int dy = 0; dy < p.dw_k; ++dy) {
        const int iy = y0 + dy;
        const bool yin = iy >= 0 && iy < p.H;
        const int iyc = min(max(iy, 0), p.H - 1);
        for (int dx = 0; dx < p.dw_k; ++dx) {
          const int ix = x0 + dx;
          const bool in = yin && ix >= 0 && ix < p.W;
          const f32x4 v = yl_ld4(in ? xb + ((size_t)iyc * p.W + ix) * p.Cin : p.zeros);
          const f32x4 w = yl_ld4(wb + (dy * p.dw_k + dx) * p.Cin);
          s.x = fmaf(v.x, w.x, s.x); s.y = fmaf(v.y, w.y, s.y);
          s.z = fmaf(v.z, w.z, s.z); s.w = fmaf(v.w, w.w, s.w);
        }
      }
    }
    const float dlo = yl_act_lo(p.dw_act), dhi = yl_act_hi(p.dw_act);
    s = yl_actc(s, p.dw_act, dlo, dhi);
    return yl_sel4(cin_ok, s);
  }
}

// N % 4 != 0 (the detection head: N = 5+C).  The MT*16 pixels of a wave's tile are consecutive rows of
// N floats, i.e. ONE contiguous, 16-byte aligned run of MT*16*N floats: the wave transposes its D
// fragments through a private LDS region and writes the run with coalesced float4 stores (4x fewer store
// instructions than per-element stores, full 128-B lines).  `stg` == nullptr or non-contiguous rows
// (A > 1 anchors: image pitch != OH*OW*N) fall back to per-element stores.
template <int NT, int MT>
__device__ __forceinline__ void yl_epi_scalar(const YlConvP& p, f32x4 (&acc)[MT][NT], const YlPix (&px)[MT], int nt0,
                                              int kq, float lo, float hi, float* stg, size_t lin0, int lane) {
  const int ohw = p.OH * p.OW;
  const bool contiguous = stg != nullptr && p.out_bstride == (long)ohw * p.N && gridDim.y == 1;
  if (contiguous) {
    const int pl = lane & 15;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = (nt0 + nt) * 16 + 4 * kq;
        f32x4 v = acc[mt][nt] + yl_ld4(p.bias + n);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float e = fminf(fmaxf(v[r], lo), hi);
          if (YL_SMOOTH(p.act)) e = yl_act1(v[r], p.act);
          if (n + r < p.N) stg[(mt * 16 + pl) * p.N + n + r] = e;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    long rows = (long)p.M - (long)lin0;                         // valid pixels of this tile
    if (rows > MT * 16) rows = MT * 16;
    const int total = (int)rows * p.N;                          // floats; the run starts 16-B aligned
    float* dst = reinterpret_cast<float*>(p.out) + lin0 * p.N;   // (rows with N & 3: detection-level rows, fp32 in every unit)
    const int n4 = total >> 2;
    for (int i = lane; i < n4; i += 64)
      *reinterpret_cast<f32x4*>(dst + 4 * i) = *reinterpret_cast<const f32x4*>(stg + 4 * i);
    for (int i = 4 * n4 + lane; i < total; i += 64) dst[i] = stg[i];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    return;
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    if (!px[mt].valid) continue;
    const int cell = px[mt].oy * p.OW + px[mt].ox;
    float* orow = reinterpret_cast<float*>(p.out) + (size_t)px[mt].b * p.out_bstride + (size_t)cell * p.N + 4 * kq;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = (nt0 + nt) * 16 + 4 * kq;
      f32x4 v = acc[mt][nt] + yl_ld4(p.bias + n);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float e = fminf(fmaxf(v[r], lo), hi);
        if (YL_SMOOTH(p.act)) e = yl_act1(v[r], p.act);
        if (n + r < p.N) orow[(nt0 + nt) * 16 + r] = e;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// grid.x: persistent over M tiles (4 waves x MT x 16 pixels each), grid.y: chunks of NT n-tiles.
// LDS: weight chunk [CH][NT][64] float4 (n-tiles beyond the layer's last one are zero-filled so the
// hot loop needs no tile predicate).
constexpr int YL_PW_SCHED = 24; // pin loads-before-MFMAs (A/B: 0 -> 29.33k, 12 -> 29.69k, 24 -> 29.75k img/s) in the 1x1/kxk loop (value = VALU ops in the address group)
// problem of this block in a level-batched launch (YlConvMulti) and the block's index / count inside it
#define YL_SELECT_PROBLEM(m)                                                        \
  int yl_k = 0;                                                                     \
  if ((m).n > 1 && (int)blockIdx.x >= (m).p[1].blk0) yl_k = 1;                     \
  if ((m).n > 2 && (int)blockIdx.x >= (m).p[2].blk0) yl_k = 2;                     \
  if ((m).n > 3 && (int)blockIdx.x >= (m).p[3].blk0) yl_k = 3;                     \
  const YlConvP& p = (m).p[yl_k];                                                   \
  const int bx = p.nblk ? (int)blockIdx.x - p.blk0 : (int)blockIdx.x;               \
  const int gx = p.nblk ? p.nblk : (int)gridDim.x;

constexpr int YL_PW_WAVES = 3;  // waves per SIMD the register budget is set for
// dynamic LDS of yl_conv_mfma_kernel, its regions in order and their floats: [CH][NT][64] float4 weight chunk | depthwise
// prologue: [dw_k*dw_k][Cin] taps, [Cin] bias | N % 4 != 0 (head rows): store staging per wave.  (Region sizes, which the kernel
// adds up as it walks the regions, not offsets: precomputed offsets hand the optimizer the same sums in another order -- and for
// the same reason functions of their arguments, not of a struct the kernel would fill from its parameters up front.)
struct YlMfmaLds {
  static constexpr size_t LIMIT = 128 * 1024;
  static constexpr size_t STREAM_CHUNK = 48 * 1024;               // weight chunk of a layer whose whole K does not fit
  static constexpr __host__ __device__ size_t chunk(int CH, int NT) { return (size_t)CH * NT * 256; }
  static constexpr __host__ __device__ size_t taps(int dw_k, int Cin) { return yl_taps_floats(dw_k, Cin); }   // (dw_k = 0: none)
  static constexpr __host__ __device__ size_t staging(int MT, int N) { return (N & 3) ? (size_t)4 * MT * 16 * N : 0; }
  static constexpr __host__ __device__ size_t bytes(int CH, int NT, int MT, int dw_k, int Cin, int N) {
    return (chunk(CH, NT) + (dw_k > 0 ? taps(dw_k, Cin) : 0) + staging(MT, N)) * 4;
  }
};

template <int NT, int MT, int MODE>
__global__ __launch_bounds__(256, (NT * MT <= 6 && MODE <= 1) ? YL_PW_WAVES : 3) void yl_conv_mfma_kernel(YlConvMulti mp) {
  YL_SELECT_PROBLEM(mp)
  extern __shared__ __attribute__((aligned(16))) float yl_wlds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, pl = lane & 15;
  const int nt0 = blockIdx.y * NT;
  const int ntc = (p.NTtot - nt0) < NT ? (p.NTtot - nt0) : NT;
  const int TK = p.TK, CH = p.CH;
  const bool single = (CH >= TK);
  f32x4* wl = reinterpret_cast<f32x4*>(yl_wlds);
  const f32x4* wg = reinterpret_cast<const f32x4*>(p.wp);
  const int ohw = p.OH * p.OW;
  const float lo = yl_act_lo(p.act), hi = yl_act_hi(p.act);

  auto load_chunk = [&](int c0, int c1) {          // asynchronous (yl_glds16): complete at the next barrier
    for (int t = c0 + wave; t < c1; t += 4) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        if (nt < ntc) yl_glds16(wg + ((size_t)t * p.NTtot + nt0 + nt) * 64 + lane, wl + ((t - c0) * NT + nt) * 64);
        else wl[((t - c0) * NT + nt) * 64 + lane] = (f32x4){0.f, 0.f, 0.f, 0.f};     // padding n-tiles of the last chunk
      }
    }
  };
  constexpr bool DWM = (MODE == YL_CM_DWPRO || MODE == YL_CM_DW3 || MODE == YL_CM_DW5);
  float* dwl = yl_wlds + YlMfmaLds::chunk(CH, NT);
  float* stg = nullptr;
  if (p.N & 3) stg = dwl + (DWM ? YlMfmaLds::taps(p.dw_k, p.Cin) : 0) + (size_t)wave * (MT * 16 * p.N);
  // residual / upsample-add without activation: the addends initialise the accumulators (loads issued
  // with the first activation fetch instead of after the last MFMA)
  const bool pre_add = (p.res || p.up) && p.act == YL_ACT_NONE && !(p.N & 3);
  if (DWM) {
    const int nw = p.dw_k * p.dw_k * p.Cin;
    yl_glds_floats(p.dw_w, dwl, nw, tid, 256);
    if (p.dw_b) yl_glds_floats(p.dw_b, dwl + nw, p.Cin, tid, 256);
    else for (int i = tid; i < p.Cin; i += 256) dwl[nw + i] = 0.0f;
  }
  if (single) load_chunk(0, TK);
  bool need_sync = single || DWM;     // first LDS read happens after the first activation loads are in flight

  for (int tile = bx; tile < p.ntiles; tile += gx) {
    YlPix px[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      px[mt] = yl_pix(((size_t)tile * 4 + wave) * (MT * 16) + mt * 16 + pl, p.M, ohw, p.OW);
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      // from zero, not from the bias: that would save 2 VALU ops per float4 but sums bias + conv instead of the reference's
      // conv + shift (on the ill-conditioned golden checkpoint one score moved by 1.2e-4)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    if (pre_add) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const size_t obase = px[mt].lin * p.N;
        size_t up_off = 0;
        if (p.up) {
          const int uy = (px[mt].oy * p.UH) / p.OH, ux = (px[mt].ox * p.UW) / p.OW;
          up_off = (((size_t)px[mt].b * p.UH + uy) * p.UW + ux) * p.N;
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const int n = (nt0 + nt) * 16 + 4 * kq;
          if (n < p.N) {
            if (p.res) acc[mt][nt] = yl_ld4(p.res + obase + n);
            if (p.up) acc[mt][nt] += yl_ld4(p.up + up_off + n);
          }
        }
      }
    }

    for (int c0 = 0; c0 < TK; c0 += CH) {
      const int c1 = (c0 + CH) < TK ? (c0 + CH) : TK;
      if (!single) {
        __syncthreads();
        load_chunk(c0, c1);
        __syncthreads();
      }
      // running (tap, kblock) counters for step c0
      int tap = c0 / p.KB, kb = c0 - tap * p.KB;
      int ky = tap / p.k, kx = tap - ky * p.k;
      f32x4 xq[MT];
      if (!DWM) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) xq[mt] = yl_fetch<MODE>(p, px[mt], ky, kx, kb * 16 + 4 * kq, dwl);
      }
      if (need_sync) {
        __syncthreads();
        need_sync = false;
      }
      for (int t = c0; t < c1; ++t) {
        int kb2 = kb + 1, ky2 = ky, kx2 = kx;
        if (kb2 == p.KB) { kb2 = 0; if (++kx2 == p.k) { kx2 = 0; ++ky2; } }
        if (t + 1 == c1) { kb2 = kb; ky2 = ky; kx2 = kx; }     // last step: harmless re-fetch
        f32x4 xn[MT];
        if (DWM) {
          // depthwise prologue: 9/25 tap loads + FMAs per step; latency is covered by the other
          // waves of the SIMD (register budget keeps >= 3 waves resident), not by a software prefetch
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) xq[mt] = yl_fetch<MODE>(p, px[mt], ky, kx, kb * 16 + 4 * kq, dwl);
        } else {
          // issue the next step's activation loads before this step's MFMAs
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) xn[mt] = yl_fetch<MODE>(p, px[mt], ky2, kx2, kb2 * 16 + 4 * kq, dwl);
        }
        const f32x4* wrow = wl + (size_t)(t - c0) * NT * 64 + lane;
        f32x4 wq[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wq[nt] = wrow[nt * 64];
        yl_mma_step<NT, MT>(wq, xq, acc);
        kb = kb2; ky = ky2; kx = kx2;
        if (!DWM) {
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) xq[mt] = xn[mt];
          // pin the order: next step's address math + loads FIRST, then the weight reads, then the MFMAs (left
          // alone the scheduler sinks the loads behind most of the MFMAs and waits for them at the end of the step)
          __builtin_amdgcn_sched_group_barrier(0x002, YL_PW_SCHED, 0);
          __builtin_amdgcn_sched_group_barrier(0x020, MT, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, NT, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, YL_MFMA_PER_BLOCK * NT * MT, 0);
        }
      }
    }

    if (MODE == YL_CM_KXK && p.w3p) {
      // Chained 1x1 conv (round 3: blocks.1.0 3x3 s2 16->48 -> blocks.1.1 1x1 48->32 of mobilenetv4_conv_small_050):
      // the epilogue of this conv leaves act(acc + bias) as 4 consecutive channels of the lane's pixel -- exactly the
      // B fragment of k-block `nt` of the next GEMM -- so the 48-channel tensor is never stored (79 MB written and
      // re-read at B = 64, one launch).  <= 2 n-tiles out; k-blocks beyond this conv's n-tiles meet zero weights.
      const f32x4* w3g = reinterpret_cast<const f32x4*>(p.w3p);      // [NTtot of this conv][NT3][64] float4
      const int NT3 = (p.C3 + 15) >> 4;
      const float lo3 = yl_act_lo(p.act3), hi3 = yl_act_hi(p.act3);
      f32x4 a3[MT][2];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) { a3[mt][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; a3[mt][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        if (nt < ntc) {
          f32x4 v[MT], w3[2];
          const f32x4 bq = yl_ld4(p.bias + (nt0 + nt) * 16 + 4 * kq);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) v[mt] = yl_clamp4(acc[mt][nt] + bq, lo, hi);
          w3[0] = w3g[((size_t)nt * NT3 + 0) * 64 + lane];
          w3[1] = w3g[((size_t)nt * NT3 + (NT3 > 1 ? 1 : 0)) * 64 + lane];
          yl_mma_step<2, MT>(w3, v, a3);
        }
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        if (!px[mt].valid) continue;
        yl_act_t* orow = p.out + px[mt].lin * p.C3;
#pragma unroll
        for (int nt3 = 0; nt3 < 2; ++nt3) {
          const int n = nt3 * 16 + 4 * kq;
          if (nt3 < NT3 && n < p.C3) yl_st4(orow + n, yl_clamp4(a3[mt][nt3] + yl_ld4(p.b3 + n), lo3, hi3));
        }
      }
      continue;
    }
    if (p.dec_boxes) yl_epi_decode<NT, MT>(p, acc, px, nt0, kq, lane);
    if (p.dec_boxes && !p.dec_raw) continue;
    if (p.N & 3) yl_epi_scalar<NT, MT>(p, acc, px, nt0, kq, lo, hi, stg, ((size_t)tile * 4 + wave) * (MT * 16), lane);
    else if (!pre_add && (p.res || p.up || YL_SMOOTH(p.act))) yl_epi_generic<NT, MT>(p, acc, px, nt0, kq);
    else yl_epi_fast<NT, MT>(p, acc, px, nt0, kq, lo, hi, true);
  }
}

// ------------------------------------------------------------------------------------------------
// depthwise (DK x DK, stride DS) -> 1x1 conv with the depthwise input staged through LDS.
// Each wave owns a 4x4 output-pixel tile (m-tile) end to end.  Per block of 16 input channels it
//   1. has the (3*DS+DK)^2-pixel x 16-channel halo patch in its private LDS region (coalesced float4
//      loads issued one k-step ahead, zero-filled outside the image),
//   2. forms its B fragment = act(bias + sum_taps w[tap] * patch[...]) from DK*DK conflict-free
//      ds_read_b128 (taps and bias also in LDS),
//   3. feeds 4 MFMA k-steps per n-tile,
// so the depthwise input is fetched from L2/HBM once per tile instead of DK*DK times and the hot loop
// has no bounds logic.  Requires OH % 4 == 0 and OW % 4 == 0 (else the DW3/DW5 global-tap modes run).
// Measured and not taken (edge_n B=64, profiles/README.md "Retired instruments"): raw buffer loads with the hardware range
// check instead of the address select -3.7 %; halo staging software-pipelined across tile boundaries +0.5 %, within noise.
constexpr __host__ __device__ int yl_dwh_hp(int dk, int ds) { return 3 * ds + dk; }                                  // halo edge in pixels
constexpr __host__ __device__ int yl_dwh_pitch(int dk, int ds) { return ((yl_dwh_hp(dk, ds) * 16 + 7) / 64) * 64 + 56; }   // see the kernel
// dynamic LDS of yl_conv_dwh_kernel, its regions in order and their floats (sizes, not offsets: see YlMfmaLds): [KB][NT][64]
// float4 weights (whole K) | [DK*DK][Cin] taps, [Cin] bias | one halo patch per wave
struct YlDwhLds {
  static constexpr size_t LIMIT = 144 * 1024;
  int NT, dk, ds, KB, Cin;
  constexpr __host__ __device__ size_t weights() const { return (size_t)KB * NT * 256; }
  constexpr __host__ __device__ size_t taps() const { return (size_t)(dk * dk + 1) * Cin; }
  constexpr __host__ __device__ size_t halos() const { return (size_t)4 * yl_dwh_hp(dk, ds) * yl_dwh_pitch(dk, ds); }
  constexpr __host__ __device__ size_t bytes() const { return (weights() + taps() + halos()) * 4; }
};

template <int NT, int DK, int DS>
__global__ __launch_bounds__(256, 3) void yl_conv_dwh_kernel(YlConvMulti mp) {
  YL_SELECT_PROBLEM(mp)
  constexpr int HP = yl_dwh_hp(DK, DS);
  // row pitch in floats, == 56 (mod 64): consecutive patch rows start 32 B "earlier" modulo the 256-B LDS
  // row, which makes the 16 lanes of every ds_read_b128 group (2 tile rows x 4 pixels x 2 channel quads)
  // hit 16 distinct 16-B slots -- conflict-free tap reads for stride 1
  constexpr int PITCHF = yl_dwh_pitch(DK, DS);
  constexpr int HF4 = HP * HP * 4;                        // float4 elements of one halo patch (16 ch)
  constexpr int NSLOT = (HF4 + 63) / 64;                  // staging float4 per lane
  constexpr int MT = 1;
  extern __shared__ __attribute__((aligned(16))) float yl_wlds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, pl = lane & 15;
  const int nt0 = blockIdx.y * NT;
  const int ntc = (p.NTtot - nt0) < NT ? (p.NTtot - nt0) : NT;
  const int KB = p.KB;
  const YlDwhLds L = {NT, DK, DS, KB, p.Cin};
  f32x4* wl = reinterpret_cast<f32x4*>(yl_wlds);          // (whole K: checked by the launcher)
  float* dwl = yl_wlds + L.weights();
  float* halo = dwl + L.taps() + wave * (HP * PITCHF);
  const f32x4* wg = reinterpret_cast<const f32x4*>(p.wp);
  const float lo = yl_act_lo(p.act), hi = yl_act_hi(p.act);
  const float dlo = yl_act_lo(p.dw_act), dhi = yl_act_hi(p.dw_act);


  const int tw = p.OW >> 2, th = p.OH >> 2;
  const int tiles_img = tw * th;
  const int ntiles = p.B * tiles_img;
  const int wstride = gx * 4;
  // lane constants: LDS offsets of the staging slots (halo pixel / channel quad) and the read base of the
  // lane's output pixel
  int s_lo[NSLOT];
  bool s_ok[NSLOT];
#pragma unroll
  for (int j = 0; j < NSLOT; ++j) {
    const int e = j * 64 + lane;
    s_ok[j] = e < HF4;
    const int hp = (s_ok[j] ? e : 0) >> 2, quad = e & 3;
    const int hr = hp / HP, hc = hp - hr * HP;
    s_lo[j] = hr * PITCHF + hc * 16 + quad * 4;
  }
  const int rbase = ((pl >> 2) * DS) * PITCHF + ((pl & 3) * DS) * 16 + 4 * kq;

  // residual add without activation: the addend initialises the accumulators (loads issued at tile start)
  const bool pre_add = p.res != nullptr && p.up == nullptr && p.act == YL_ACT_NONE;
  // The depthwise input is addressed by 32-bit byte offsets (the launcher guarantees the tensor is < 2 GiB); a slot outside
  // the image or in the channel tail carries OOB and reads the zero buffer instead (address select).
  constexpr unsigned OOB = 0x80000000u;
  unsigned goff[NSLOT];        // byte offsets of the lane's staging slots (channel block 0) for one tile
  auto tile_geom = [&](int tile) {
    const int b = tile / tiles_img;
    const int trem = tile - b * tiles_img;
    const int tyi = trem / tw, txi = trem - tyi * tw;
    const int iy0 = 4 * tyi * DS - p.dw_pad_t, ix0 = 4 * txi * DS - p.dw_pad_l;
#pragma unroll
    for (int j = 0; j < NSLOT; ++j) {
      const int e = j * 64 + lane;
      const int hp = (e < HF4 ? e : 0) >> 2;
      const int hr = hp / HP, hc = hp - hr * HP;
      const int iy = iy0 + hr, ix = ix0 + hc;
      const bool in = e < HF4 && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      goff[j] = in ? (unsigned)((((b * p.H + iy) * p.W + ix) * p.Cin + (lane & 3) * 4) * (int)sizeof(yl_act_t)) : OOB;
    }
  };
  auto stage_load = [&](int kb, f32x4 (&r)[NSLOT]) {
    const bool cok = kb * 16 + (lane & 3) * 4 < p.Cin;
#pragma unroll
    for (int j = 0; j < NSLOT; ++j) {
      const unsigned off = cok ? goff[j] + (unsigned)kb * (16u * (unsigned)sizeof(yl_act_t)) : OOB;
      r[j] = yl_ld4(off < OOB ? p.x + off / (unsigned)sizeof(yl_act_t) : p.zeros);
    }
  };
  auto stage_store = [&](const f32x4 (&r)[NSLOT]) {
#pragma unroll
    for (int j = 0; j < NSLOT; ++j)
      if (s_ok[j]) *reinterpret_cast<f32x4*>(halo + s_lo[j]) = r[j];
  };
  f32x4 stg[NSLOT];
  int tile = bx * 4 + wave;
  bool primed = false;
  if (tile < ntiles) {                  // the first tile's first halo stage is requested BEFORE the weight fill and
    tile_geom(tile);                    // the barrier: both fetches are in flight together
    stage_load(0, stg);
    primed = true;
  }
  for (int t = wave; t < KB; t += 4) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      f32x4 w = {0.f, 0.f, 0.f, 0.f};
      if (nt < ntc) yl_glds16(wg + ((size_t)t * p.NTtot + nt0 + nt) * 64 + lane, wl + (t * NT + nt) * 64);
      else wl[(t * NT + nt) * 64 + lane] = w;
    }
  }
  {
    const int nw = DK * DK * p.Cin;
    yl_glds_floats(p.dw_w, dwl, nw, tid, 256);
    if (p.dw_b) yl_glds_floats(p.dw_b, dwl + nw, p.Cin, tid, 256);
    else for (int i = tid; i < p.Cin; i += 256) dwl[nw + i] = 0.0f;
  }
  __syncthreads();
  for (; tile < ntiles; tile += wstride) {
    const int b = tile / tiles_img;
    const int trem = tile - b * tiles_img;
    const int tyi = trem / tw, txi = trem - tyi * tw;
    YlPix px[MT];
    px[0].b = b;
    px[0].oy = 4 * tyi + (pl >> 2);
    px[0].ox = 4 * txi + (pl & 3);
    px[0].valid = true;
    px[0].lin = ((size_t)b * p.OH + px[0].oy) * p.OW + px[0].ox;
    f32x4 acc[MT][NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = (nt0 + nt) * 16 + 4 * kq;
      acc[0][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};                       // (not the bias: see yl_conv_mfma_kernel)
      if (pre_add && n < p.N) acc[0][nt] = yl_ld4(p.res + px[0].lin * p.N + n);
    }
    if (!primed) {
      tile_geom(tile);
      stage_load(0, stg);
    }
    primed = false;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");          // previous tile's halo reads are complete
    stage_store(stg);
    for (int kb = 0; kb < KB; ++kb) {
      // next channel block of the tile: loads in flight under this step's taps and MFMAs
      const bool more = kb + 1 < KB;
      if (more) stage_load(kb + 1, stg);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");          // halo writes (all lanes) -> tap reads
      const int c = kb * 16 + 4 * kq;
      const int cs = c < p.Cin ? c : p.Cin - 4;
      f32x4 s = yl_ld4(dwl + DK * DK * p.Cin + cs);
      if (DK == 3) {
#pragma unroll
        for (int dy = 0; dy < DK; ++dy)
#pragma unroll
          for (int dx = 0; dx < DK; ++dx) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(halo + rbase + dy * PITCHF + dx * 16);
            const f32x4 w = yl_ld4(dwl + (dy * DK + dx) * p.Cin + cs);
            s.x = fmaf(v.x, w.x, s.x); s.y = fmaf(v.y, w.y, s.y);
            s.z = fmaf(v.z, w.z, s.z); s.w = fmaf(v.w, w.w, s.w);
          }
      } else {
#pragma unroll 1
        for (int dy = 0; dy < DK; ++dy) {                 // one tap row at a time bounds the register footprint
#pragma unroll
          for (int dx = 0; dx < DK; ++dx) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(halo + rbase + dy * PITCHF + dx * 16);
            const f32x4 w = yl_ld4(dwl + (dy * DK + dx) * p.Cin + cs);
            s.x = fmaf(v.x, w.x, s.x); s.y = fmaf(v.y, w.y, s.y);
            s.z = fmaf(v.z, w.z, s.z); s.w = fmaf(v.w, w.w, s.w);
          }
        }
      }
      // channel tail (c >= Cin): stage_load gave those lanes the out-of-range offset, so the halo holds zeros there (never the
      // next pixel's channels) and the packed 1x1 weights of those k slots are zero as well
      f32x4 xq[1];
      xq[0] = yl_actc(s, p.dw_act, dlo, dhi);
      const f32x4* wrow = wl + (size_t)kb * NT * 64 + lane;
      f32x4 wq[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) wq[nt] = wrow[nt * 64];
      yl_mma_step<NT, 1>(wq, xq, acc);
      if (more) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");        // this step's tap reads are complete
        stage_store(stg);
      }
    }
    if (!pre_add && (p.res || p.up || YL_SMOOTH(p.act))) yl_epi_generic<NT, MT>(p, acc, px, nt0, kq);
    else yl_epi_fast<NT, MT>(p, acc, px, nt0, kq, lo, hi, true);
  }
}

// ------------------------------------------------------------------------------------------------
// Whole inverted-residual block in ONE launch:  1x1 expand (+BN+act)  ->  depthwise DKxDK s1 (+BN+act)
// ->  1x1 project (+BN) (+residual).  The expanded tensor (2-6x the block's input) never exists in
// HBM: per 16-channel slab it is produced by a mini-GEMM on the wave's halo pixels (HM m-tiles of 16
// pixels: the 4x4 output tile grown by the depthwise reach), written to the wave's LDS patch in exactly
// the layout the depthwise stage reads (MFMA D fragment = 4 channels of one pixel), consumed by the
// tap FMAs, and fed to the projection GEMM.  Costs HM x the expansion FLOPs (2.25x for 3x3, 4x for 5x5)
// in exchange for one launch instead of two and no expanded-tensor traffic -- these blocks live at
// 40x40 / 20x20 where launches are latency-bound, not FLOP-bound.
// Projection weights: LDS.  Expansion weights: A fragments straight from L2 (prefetched one slab ahead).
constexpr __host__ __device__ int yl_uib_pitch(int dk) { return ((3 + dk) % 4 == 1 || (3 + dk) % 4 == 3) ? 3 + dk : 3 + dk + 1; }   // halo row pitch in pixels
// dynamic LDS of yl_uib_kernel, its regions in order and their floats (sizes, not offsets: see YlMfmaLds): [KB][NT][64] float4
// projection weights | [DK*DK][Cmid] taps, [Cmid] dw bias | [KB*16] expansion bias | one expanded halo slab per wave
struct YlUibLds {
  static constexpr size_t LIMIT = YlDwhLds::LIMIT;
  int NT, dk, KB, Cmid;
  constexpr __host__ __device__ size_t weights() const { return (size_t)KB * NT * 256; }
  constexpr __host__ __device__ size_t taps() const { return (size_t)(dk * dk + 1) * Cmid; }
  constexpr __host__ __device__ size_t bias2() const { return (size_t)KB * 16; }
  constexpr __host__ __device__ size_t halos() const { return (size_t)4 * (3 + dk) * yl_uib_pitch(dk) * 16; }
  constexpr __host__ __device__ size_t bytes() const { return (weights() + taps() + bias2() + halos()) * 4; }
};

template <int NT, int DK, int KBI /*ceil(C1/16)*/>
__global__ __launch_bounds__(256) void yl_uib_kernel(YlConvP p) {
  constexpr int HP = 3 + DK;                               // halo edge (stride 1)
  constexpr int PITCH = yl_uib_pitch(DK);
  constexpr int HM = (HP * HP + 15) / 16;                  // halo m-tiles (3 for 3x3, 4 for 5x5)
  constexpr int MT = 1;
  extern __shared__ __attribute__((aligned(16))) float yl_wlds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, pl = lane & 15;
  const int nt0 = 0;
  const int KB = p.KB;                                     // 16-channel slabs of the expanded tensor
  const YlUibLds L = {NT, DK, KB, p.Cin};
  f32x4* wl = reinterpret_cast<f32x4*>(yl_wlds);
  float* dwl = yl_wlds + L.weights();
  float* b2l = dwl + L.taps();
  float* halo = b2l + L.bias2() + wave * (HP * PITCH * 16);
  const f32x4* wg = reinterpret_cast<const f32x4*>(p.wp);
  const f32x4* w2g = reinterpret_cast<const f32x4*>(p.w2p);  // [KBI][KB][64] float4
  const float lo = yl_act_lo(p.act), hi = yl_act_hi(p.act);
  const float dlo = yl_act_lo(p.dw_act), dhi = yl_act_hi(p.dw_act);
  const float elo = yl_act_lo(p.act2), ehi = yl_act_hi(p.act2);

  for (int t = wave; t < KB; t += 4) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      f32x4 w = {0.f, 0.f, 0.f, 0.f};
      if (nt < p.NTtot) w = wg[((size_t)t * p.NTtot + nt) * 64 + lane];
      wl[(t * NT + nt) * 64 + lane] = w;
    }
  }
  {
    const int nw = DK * DK * p.Cin;
    yl_glds_floats(p.dw_w, dwl, nw, tid, 256);
    if (p.dw_b) yl_glds_floats(p.dw_b, dwl + nw, p.Cin, tid, 256);
    else for (int i = tid; i < p.Cin; i += 256) dwl[nw + i] = 0.0f;
    for (int i = tid; i < KB * 16; i += 256) b2l[i] = p.b2[i];
  }
  __syncthreads();

  const int tw = p.OW >> 2, th = p.OH >> 2;
  const int tiles_img = tw * th;
  const int ntiles = p.B * tiles_img;
  const int wstride = gridDim.x * 4;
  // lane constants: halo pixel of this lane in every halo m-tile
  int h_r[HM], h_c[HM], h_lo[HM];
  bool h_ok[HM];
#pragma unroll
  for (int m = 0; m < HM; ++m) {
    const int q = m * 16 + pl;
    h_ok[m] = q < HP * HP;
    const int qq = h_ok[m] ? q : 0;
    h_r[m] = qq / HP;
    h_c[m] = qq - h_r[m] * HP;
    h_lo[m] = (h_r[m] * PITCH + h_c[m]) * 16 + 4 * kq;
  }
  const int rbase = ((pl >> 2) * PITCH + (pl & 3)) * 16 + 4 * kq;
  const bool pre_add = p.res != nullptr && p.act == YL_ACT_NONE;

  for (int tile = blockIdx.x * 4 + wave; tile < ntiles; tile += wstride) {
    const int b = tile / tiles_img;
    const int trem = tile - b * tiles_img;
    const int tyi = trem / tw, txi = trem - tyi * tw;
    YlPix px[MT];
    px[0].b = b;
    px[0].oy = 4 * tyi + (pl >> 2);
    px[0].ox = 4 * txi + (pl & 3);
    px[0].valid = true;
    px[0].lin = ((size_t)b * p.OH + px[0].oy) * p.OW + px[0].ox;
    // block input at the lane's halo pixels: B fragments of the expansion GEMM, resident for the tile
    const int iy0 = 4 * tyi - p.dw_pad_t, ix0 = 4 * txi - p.dw_pad_l;
    f32x4 xin[HM][KBI];
    bool h_in[HM];
#pragma unroll
    for (int m = 0; m < HM; ++m) {
      const int iy = iy0 + h_r[m], ix = ix0 + h_c[m];
      h_in[m] = h_ok[m] && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      const yl_act_t* src = p.x + (((size_t)b * p.H + iy) * p.W + ix) * p.C1 + 4 * kq;
#pragma unroll
      for (int kbi = 0; kbi < KBI; ++kbi) {
        const bool ok = h_in[m] && (kbi * 16 + 4 * kq) < p.C1;
        xin[m][kbi] = yl_ld4(ok ? src + kbi * 16 : p.zeros);
      }
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      acc[0][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const int n = nt * 16 + 4 * kq;
      if (pre_add && n < p.N) acc[0][nt] = yl_ld4(p.res + px[0].lin * p.N + n);
    }
    f32x4 we[KBI], wn[KBI];
#pragma unroll
    for (int kbi = 0; kbi < KBI; ++kbi) wn[kbi] = w2g[((size_t)kbi * KB + 0) * 64 + lane];
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
      for (int kbi = 0; kbi < KBI; ++kbi) we[kbi] = wn[kbi];
      if (kb + 1 < KB) {
#pragma unroll
        for (int kbi = 0; kbi < KBI; ++kbi) wn[kbi] = w2g[((size_t)kbi * KB + kb + 1) * 64 + lane];
      }
      // expansion slab on the halo pixels
      const f32x4 eb = yl_ld4(b2l + kb * 16 + 4 * kq);
      f32x4 ex[HM];
#pragma unroll
      for (int m = 0; m < HM; ++m) {
        f32x4 e = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kbi = 0; kbi < KBI; ++kbi)
#pragma unroll
          for (int ss = 0; ss < 4; ++ss)
            e = __builtin_amdgcn_mfma_f32_16x16x4f32(we[kbi][ss], xin[m][kbi][ss], e, 0, 0, 0);
        e = yl_actc(e + eb, p.act2, elo, ehi);
        ex[m] = yl_sel4(h_in[m], e);                                  // the depthwise conv zero-pads the EXPANDED tensor
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");          // previous slab's tap reads are complete
#pragma unroll
      for (int m = 0; m < HM; ++m)
        if (h_ok[m]) *reinterpret_cast<f32x4*>(halo + h_lo[m]) = ex[m];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");          // slab visible to all lanes
      // depthwise on the slab
      const int c = kb * 16 + 4 * kq;
      const int cs = c < p.Cin ? c : p.Cin - 4;
      f32x4 s = yl_ld4(dwl + DK * DK * p.Cin + cs);
#pragma unroll
      for (int dy = 0; dy < DK; ++dy)
#pragma unroll
        for (int dx = 0; dx < DK; ++dx) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(halo + rbase + (dy * PITCH + dx) * 16);
          const f32x4 w = yl_ld4(dwl + (dy * DK + dx) * p.Cin + cs);
          s.x = fmaf(v.x, w.x, s.x); s.y = fmaf(v.y, w.y, s.y);
          s.z = fmaf(v.z, w.z, s.z); s.w = fmaf(v.w, w.w, s.w);
        }
      const f32x4 xq = yl_sel4(c < p.Cin, yl_actc(s, p.dw_act, dlo, dhi));
      // projection
      const f32x4* wrow = wl + (size_t)kb * NT * 64 + lane;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const f32x4 wq = wrow[nt * 64];
#pragma unroll
        for (int ss = 0; ss < 4; ++ss)
          acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wq[ss], xq[ss], acc[0][nt], 0, 0, 0);
      }
    }
    if (!pre_add && (p.res || YL_SMOOTH(p.act))) yl_epi_generic<NT, MT>(p, acc, px, nt0, kq);
    else yl_epi_fast<NT, MT>(p, acc, px, nt0, kq, lo, hi, true);
  }
}

// ------------------------------------------------------------------------------------------------
// stem: 3x3 conv on the NCHW network input (Cin = 3, K = 27 padded to 28 = 7 MFMA k-steps).
// Same transposed GEMM as above: A = weights (7*NT floats per lane, resident in registers for the whole
// kernel), B = one input scalar per lane per k-step gathered straight from the three input planes
// (lane = (pixel, k mod 4); k = c*9 + ky*3 + kx), D = 4 consecutive output channels per lane -> float4
// NHWC stores.  Persistent over tiles of 4 waves x MT x 16 pixels.
template <int NT, int MT>
__global__ __launch_bounds__(256) void yl_stem_mfma_kernel(YlConvP p) {
  constexpr int KS = 7;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, pl = lane & 15;
  float wa[KS][NT];
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) wa[s][nt] = p.wp[(s * NT + nt) * 64 + lane];
  int tky[KS], tkx[KS], tc[KS];
  bool tok[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int k = 4 * s + kq;
    tok[s] = k < 27;
    const int kc = tok[s] ? k : 26;
    tc[s] = kc / 9;
    const int r = kc - 9 * tc[s];
    tky[s] = r / 3;
    tkx[s] = r - 3 * tky[s];
  }
  const int ohw = p.OH * p.OW;
  const size_t plane = (size_t)p.H * p.W;
  const float lo = yl_act_lo(p.act), hi = yl_act_hi(p.act);
  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    float xv[MT][KS];
    size_t lins[MT];
    bool valid[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      size_t lin = ((size_t)tile * 4 + wave) * (MT * 16) + mt * 16 + pl;
      valid[mt] = lin < (size_t)p.M;
      if (!valid[mt]) lin = (size_t)p.M - 1;
      lins[mt] = lin;
      const int b = (int)(lin / ohw);
      const int rem = (int)(lin - (size_t)b * ohw);
      const int oy = rem / p.OW, ox = rem - oy * p.OW;
      const int y0 = oy * p.stride - p.pad_t, x0 = ox * p.stride - p.pad_l;
      const float* xb = reinterpret_cast<const float*>(p.x) + (size_t)b * 3 * plane;   // the fp32 NCHW network input
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int iy = y0 + tky[s], ix = x0 + tkx[s];
        const bool in = tok[s] && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        const int iyc = min(max(iy, 0), p.H - 1), ixc = min(max(ix, 0), p.W - 1);
        const float t = xb[tc[s] * plane + (size_t)iyc * p.W + ixc];
        xv[mt][s] = in ? t : 0.0f;
      }
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[s][nt], xv[mt][s], acc[mt][nt], 0, 0, 0);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      if (!valid[mt]) continue;
      yl_act_t* orow = p.out + lins[mt] * p.N;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = nt * 16 + 4 * kq;
        f32x4 v = acc[mt][nt] + yl_ld4(p.bias + n);
        if (YL_SMOOTH(p.act)) v = yl_act4(v, p.act);
        v.x = fminf(fmaxf(v.x, lo), hi); v.y = fminf(fmaxf(v.y, lo), hi);
        v.z = fminf(fmaxf(v.z, lo), hi); v.w = fminf(fmaxf(v.w, lo), hi);
        yl_st4(orow + n, v);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// stand-alone depthwise kxk: lane = (pixel, 4 channels); weights [tap][C].
__global__ __launch_bounds__(256) void yl_dw_kernel(YlConvP p) {
  const int cq = p.Cin >> 2;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)p.M * cq) return;
  const size_t lin = i / cq;
  const int c = (int)(i - lin * cq) * 4;
  const int ohw = p.OH * p.OW;
  const int b = (int)(lin / ohw);
  const int rem = (int)(lin - (size_t)b * ohw);
  const int oy = rem / p.OW, ox = rem - oy * p.OW;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (p.bias) s = yl_ld4(p.bias + c);
  const int y0 = oy * p.stride - p.pad_t, x0 = ox * p.stride - p.pad_l;
  const yl_act_t* xb = p.x + (size_t)b * p.H * p.W * p.Cin + c;
  for (int dy = 0; dy < p.k; ++dy) {
    const int iy = y0 + dy;
    if (iy < 0 || iy >= p.H) continue;
    for (int dx = 0; dx < p.k; ++dx) {
      const int ix = x0 + dx;
      if (ix < 0 || ix >= p.W) continue;
      const f32x4 v = yl_ld4(xb + ((size_t)iy * p.W + ix) * p.Cin);
      const f32x4 w = yl_ld4(p.wp + (dy * p.k + dx) * p.Cin + c);
      s.x = fmaf(v.x, w.x, s.x); s.y = fmaf(v.y, w.y, s.y);
      s.z = fmaf(v.z, w.z, s.z); s.w = fmaf(v.w, w.w, s.w);
    }
  }
  s = yl_act4(s, p.act);
  const size_t o = lin * p.N + c;
  if (p.res) s += yl_ld4(p.res + o);
  yl_st4(p.out + o, s);
}

// Register-tiled stand-alone depthwise K x K (stride S): a lane owns 4 channels of a 4 x 2 block of output pixels and
// streams the (3S+K) x (S+K) input window row by row through registers, so an input value is fetched once per
// 8 outputs x the window overlap (6 float4 loads per output at 5x5 stride 1) instead of once per tap (25): the
// one-output-per-lane kernel above is L2-bandwidth-bound (0.34 ms = 0.87 TB/s of HBM-side traffic for yololite_m's
// 720-channel 5x5 layers at 40x40, 11 TB/s out of L2).  Consecutive lanes = consecutive channel quads of the same
// pixels (coalesced 16-byte loads); a workgroup = 64 channel quads x 4 pixel blocks, persistent over the pixel
// blocks with its K*K x 256 tap weights (+ bias) in LDS.  Taps outside the image read the zero buffer and are
// accumulated in the same (dy, dx) order as yl_dw_kernel: bit-identical.
// POOL (squeeze-excite producer): waves are dealt to IMAGES -- wave gw = (b, r) walks the blocks r, r + WPI, ... of image
// b only -- and each lane also sums its 4 channels of the activated outputs it stores, in block / row / column order;
// the per-wave sums go to pool[b][r][C].  Same arithmetic per output: the tensor is bit-identical to the plain launch.
template <int K, int S, bool POOL = false>
__global__ __launch_bounds__(256, 2) void yl_dw_tile_kernel(YlConvP p) {
  constexpr int TX = 4, TY = 2;
  constexpr int COLS = (TX - 1) * S + K, ROWS = (TY - 1) * S + K;
  __shared__ __attribute__((aligned(16))) float wl[(K * K + 1) * 256];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // block coordinates below stay in SGPRs
  const int C = p.Cin;
  const int cbase = blockIdx.x * 256;
  for (int i = threadIdx.x; i < (K * K + 1) * 256; i += 256) {
    const int t = i >> 8, c = cbase + (i & 255);
    float v = 0.0f;
    if (c < C) v = t < K * K ? p.wp[t * C + c] : (p.bias ? p.bias[c] : 0.0f);
    wl[i] = v;
  }
  __syncthreads();
  const int c = cbase + lane * 4;
  if (c >= C) return;
  const int H = p.H, W = p.W, OH = p.OH, OW = p.OW;
  const int bxn = (OW + TX - 1) / TX, byn = (OH + TY - 1) / TY;
  const long nblk = (long)p.B * byn * bxn;
  const long zdelta = p.zeros - p.x;
  const float* wq = wl + lane * 4;
  const f32x4 bias = *reinterpret_cast<const f32x4*>(wq + K * K * 256);
  // plain: blocks of the whole batch dealt round-robin to the waves; POOL: wave (pb, pr) of image pb takes every
  // pool_wpi-th block of that image
  const int pgw = (int)blockIdx.y * 4 + wave;
  const int pb = POOL ? pgw / p.pool_wpi : 0, pr = POOL ? pgw - pb * p.pool_wpi : 0;
  if (POOL && pb >= p.B) return;
  const long blk_lo = POOL ? (long)pb * byn * bxn + pr : (long)blockIdx.y * 4 + wave;
  const long blk_hi = POOL ? (long)(pb + 1) * byn * bxn : nblk;
  const long blk_step = POOL ? (long)p.pool_wpi : (long)gridDim.y * 4;
  f32x4 psum = {0.f, 0.f, 0.f, 0.f};
  for (long blk = blk_lo; blk < blk_hi; blk += blk_step) {
    const int b = (int)(blk / (byn * bxn));
    const int r0 = (int)(blk - (long)b * byn * bxn);
    const int by = r0 / bxn, bx = r0 - by * bxn;
    const int oy0 = by * TY, ox0 = bx * TX;
    const int iy0 = oy0 * S - p.pad_t, ix0 = ox0 * S - p.pad_l;
    f32x4 acc[TY][TX];
#pragma unroll
    for (int t = 0; t < TY; ++t)
#pragma unroll
      for (int j = 0; j < TX; ++j) acc[t][j] = bias;
    // addresses: wave-uniform 64-bit base per (row, column) (SALU) + the lane's 32-bit channel offset; a tap outside
    // the image selects the zero buffer with offset 0
    const char* xb = reinterpret_cast<const char*>(p.x + (size_t)b * H * W * C);
    const unsigned coff = (unsigned)c * (unsigned)sizeof(yl_act_t);
    const long zoff = reinterpret_cast<const char*>(p.zeros) - xb;
    // window rows double-buffered in registers: row r + 1 is requested before the FMAs of row r (the scheduling
    // barriers keep the compiler from hoisting all ROWS x COLS loads to the top: 192 VGPRs and spills at 5x5)
    auto load_row = [&](int r, f32x4 (&row)[COLS]) {
      const int iy = iy0 + r;
      const bool yok = iy >= 0 && iy < H;
#pragma unroll
      for (int q = 0; q < COLS; ++q) {
        const int ix = ix0 + q;
        const bool ok = yok && ix >= 0 && ix < W;
        const long m = -(long)ok;                                     // branch-free select (uniform: SALU and/or)
        const long off = ((((long)iy * W + ix) * C * (long)sizeof(yl_act_t)) & m) | (zoff & ~m);
        row[q] = yl_ld4(reinterpret_cast<const yl_act_t*>(xb + off + (coff & (unsigned)m)));
      }
    };
    // 5x5: the 25 tap weights must be re-read from LDS per block (an opaque zero in their address stops the compiler
    // from hoisting 100 VGPRs of them out of the persistent loop); 3x3: the 9 hoisted weights stay in registers
    int wz = 0;
    if (K > 3) asm volatile("" : "+s"(wz));
    const float* wqb = wq + wz;
    f32x4 rows[2][COLS];
    load_row(0, rows[0]);
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      if (r + 1 < ROWS) load_row(r + 1, rows[(r + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < TY; ++t) {
        const int dy = r - t * S;
        if (dy < 0 || dy >= K) continue;
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(wqb + (dy * K + dx) * 256);
#pragma unroll
          for (int j = 0; j < TX; ++j) {
            const f32x4 v = rows[r & 1][j * S + dx];
            acc[t][j].x = fmaf(v.x, w.x, acc[t][j].x); acc[t][j].y = fmaf(v.y, w.y, acc[t][j].y);
            acc[t][j].z = fmaf(v.z, w.z, acc[t][j].z); acc[t][j].w = fmaf(v.w, w.w, acc[t][j].w);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // pin the accumulators here: without it LLVM sinks every output's 25-FMA chain into its guarded store block
    // below, which keeps the whole ROWS x COLS window (192 VGPRs at 5x5) alive until then
#pragma unroll
    for (int t = 0; t < TY; ++t)
#pragma unroll
      for (int j = 0; j < TX; ++j)
        asm volatile("" : "+v"(acc[t][j].x), "+v"(acc[t][j].y), "+v"(acc[t][j].z), "+v"(acc[t][j].w));
#pragma unroll
    for (int t = 0; t < TY; ++t) {
      const int oy = oy0 + t;
      if (oy >= OH) continue;
#pragma unroll
      for (int j = 0; j < TX; ++j) {
        const int ox = ox0 + j;
        if (ox >= OW) continue;
        f32x4 s4 = yl_act4(acc[t][j], p.act);
        const size_t o = (((size_t)b * OH + oy) * OW + ox) * p.N + c;
        if (p.res) s4 += yl_ld4(p.res + o);
        if (POOL) psum += s4;
        yl_st4(p.out + o, s4);
      }
    }
  }
  if (POOL) *reinterpret_cast<f32x4*>(p.pool + ((size_t)pb * p.pool_wpi + pr) * C + c) = psum;
}

// ------------------------------------------------------------------------------------------------
// The instantiations of the three kernel families of this unit, each written once; yl_conv_init, the occupancy query
// and the launch all go through these tables.
// n-tiles per workgroup of the persistent kernels: NT in {1, 2, 3, 4, 6, 8}, as the first index of their tables
#define YL_NT_LIST(X) {X(1), X(2), X(3), X(4), X(6), X(8)}
static int yl_nt_index(int NT) { return NT <= 4 ? NT - 1 : NT == 6 ? 4 : 5; }

// yl_conv_mfma_kernel<NT, MT, MODE>: every NT x MT in {1, 2} x the six modes, as [nt index][MT - 1][YL_CM_*] (no mode 4)
#define YL_MFMA_MODES(NT, MT)                                                                                            \
  {yl_conv_mfma_kernel<NT, MT, YL_CM_PW>, yl_conv_mfma_kernel<NT, MT, YL_CM_KXK>, yl_conv_mfma_kernel<NT, MT, YL_CM_DWPRO>, \
   yl_conv_mfma_kernel<NT, MT, YL_CM_DW3>, nullptr, yl_conv_mfma_kernel<NT, MT, YL_CM_DW5>, yl_conv_mfma_kernel<NT, MT, YL_CM_PWSC>}
#define YL_MFMA_MTS(NT) {YL_MFMA_MODES(NT, 1), YL_MFMA_MODES(NT, 2)}
static const YlMultiKernel yl_mfma_kernels[6][2][7] = YL_NT_LIST(YL_MFMA_MTS);

// yl_conv_dwh_kernel<NT, DK, DS>: every NT x depthwise 3x3 / 5x5 x stride 1 / 2, as [nt index][DK == 5][DS == 2]
#define YL_DWH_SHAPES(NT) \
  {{yl_conv_dwh_kernel<NT, 3, 1>, yl_conv_dwh_kernel<NT, 3, 2>}, {yl_conv_dwh_kernel<NT, 5, 1>, yl_conv_dwh_kernel<NT, 5, 2>}}
static const YlMultiKernel yl_dwh_kernels[6][2][2] = YL_NT_LIST(YL_DWH_SHAPES);

// yl_uib_kernel<NT, DK, KBI>: NT (projection n-tiles) x DK x KBI (input k-blocks)
#define YL_UIB_SHAPES(X)                                                           \
  X(1, 3, 1) X(2, 3, 1) X(1, 5, 1) X(2, 5, 2)          /* tiny test nets */            \
  X(3, 3, 3) X(4, 3, 4) X(4, 5, 4) X(3, 5, 3)          /* mobilenetv4_conv_small_050 */ \
  X(6, 3, 6) X(8, 3, 8) X(8, 5, 8) X(6, 5, 6)          /* mobilenetv4_conv_small */     \
  X(2, 3, 2) X(2, 5, 1)
static YlConvKernel yl_uib_kernel_of(int NT, int DK, int KBI) {
#define YL_UIB_PICK(A, B, C) if (NT == A && DK == B && KBI == C) return yl_uib_kernel<A, B, C>;
  YL_UIB_SHAPES(YL_UIB_PICK)
#undef YL_UIB_PICK
  return nullptr;
}

hipError_t yl_conv_init() {
  hipError_t e = yl_set_lds_cap(yl_mfma_kernels, YlMfmaLds::LIMIT);
  if (e == hipSuccess) e = yl_set_lds_cap(yl_dwh_kernels, YlDwhLds::LIMIT);
#define YL_UIB_CAP(A, B, C) if (e == hipSuccess) e = yl_set_lds_cap(yl_uib_kernel<A, B, C>, YlUibLds::LIMIT);
  YL_UIB_SHAPES(YL_UIB_CAP)
#undef YL_UIB_CAP
  return e;
}

// hipErrorInvalidValue: shape not instantiated (yl_uib_supported tells the host compiler beforehand)
static hipError_t yl_uib_go(const YlConvP& p, size_t lds, hipStream_t st, int NT, int DK, int KBI) {
  const YlConvKernel kern = yl_uib_kernel_of(NT, DK, KBI);
  if (!kern) return hipErrorInvalidValue;
  const long wtiles = (long)p.B * (p.OH >> 2) * (p.OW >> 2);
  int gx = yl_resident_blocks((const void*)kern, 256, lds, 4);
  if (gx > (wtiles + 3) / 4) gx = (int)((wtiles + 3) / 4);
  hipLaunchKernelGGL(kern, dim3(gx), dim3(256), lds, st, p);
  return hipGetLastError();
}

size_t yl_uib_lds_bytes(int Cmid, int NT, int dk) {
  return YlUibLds{NT, dk, (Cmid + 15) / 16, Cmid}.bytes();
}

bool yl_uib_supported(int c1, int cmid, int n, int dk) {
  const int nts[6] = {1, 2, 3, 4, 6, 8};
  const int ntt = (n + 15) / 16, kbi = (c1 + 15) / 16;
  int NT = 0;
  for (int i = 0; i < 6; ++i) if (nts[i] >= ntt) { NT = nts[i]; break; }
  if (!NT || (dk != 3 && dk != 5)) return false;
  if (yl_uib_lds_bytes(cmid, NT, dk) > YlUibLds::LIMIT) return false;
  return yl_uib_kernel_of(NT, dk, kbi) != nullptr;
}

// split `gx` blocks over the problems in proportion to their tile counts (every problem gets >= 1 block and
// never more blocks than tiles); n == 1 keeps the whole grid (nblk = 0)
static int yl_partition_blocks(YlConvMulti& m, const long* tiles, int gx) {
  if (m.n == 1) { m.p[0].blk0 = 0; m.p[0].nblk = 0; return gx; }
  long total = 0;
  for (int k = 0; k < m.n; ++k) total += tiles[k];
  int at = 0;
  for (int k = 0; k < m.n; ++k) {
    long nb = (tiles[k] * gx + total / 2) / total;
    if (nb < 1) nb = 1;
    if (nb > tiles[k]) nb = tiles[k];
    m.p[k].blk0 = at;
    m.p[k].nblk = (int)nb;
    at += (int)nb;
  }
  return at;
}

// n-tiles per workgroup of the kernels that chunk N over grid.y (yl_conv_mfma_kernel, yl_conv_dwh_kernel)
static int yl_pick_nt(int NTtot) {
  const int nts[6] = {1, 2, 3, 4, 6, 8};
  if (NTtot <= 8) {
    for (int i = 0; i < 6; ++i) if (nts[i] >= NTtot) return nts[i];
  }
  // smallest number of chunks, then the least padding
  int best = 8, bestc = (NTtot + 7) / 8;
  for (int i = 5; i >= 3; --i) {
    const int c = (NTtot + nts[i] - 1) / nts[i];
    if (c < bestc || (c == bestc && nts[i] < best)) { best = nts[i]; bestc = c; }
  }
  return best;
}

// yl_conv_mfma_kernel's weight chunk for the layer p at (NT, MT): CH k-steps resident in LDS, the whole K if it fits, else
// 48 KiB chunks stream; false: taps + store staging leave no room for one k-step
static bool yl_mfma_chunk(const YlConvP& p, int NT, int MT, int* CH) {
  const size_t step_bytes = YlMfmaLds::chunk(1, NT) * 4;               // one k-step of weights
  const size_t extra = YlMfmaLds::bytes(0, NT, MT, p.dw_k, p.Cin, p.N);   // taps + store staging (head rows)
  if (extra + step_bytes > YlMfmaLds::LIMIT) return false;
  const size_t budget = YlMfmaLds::LIMIT - extra;
  if ((size_t)p.TK * step_bytes <= budget) *CH = p.TK;                 // whole K resident
  else *CH = (int)((budget < YlMfmaLds::STREAM_CHUNK ? budget : YlMfmaLds::STREAM_CHUNK) / step_bytes);   // stream K in chunks
  return true;
}

// Which kernel runs the depthwise -> 1x1 launch m (yl_internal.h), in the order the families are asked:
YlDwForm yl_dw_form(const YlConvMulti& m, int big, int tile_hint) {
  const YlDwForm none = {YL_DWF_NONE, {0, 0, 0, 0, 0, 0}};
  const int n = m.n;
  const YlConvP& p = m.p[big];
  if (n < 1 || n > 4 || p.dw_k <= 0 || p.C1 > 0 || p.scale) return none;
  const int NT = yl_pick_nt(p.NTtot);
  const int gy = (p.NTtot + NT - 1) / NT;
  if (n > 1 && gy != 1) return none;
  // depthwise k x k -> 1x1 with >= 192 depthwise channels and 7..22 n-tiles (EfficientNet-Lite conv_dw -> conv_pwl): streamed 1x1
  // AND tap weights, halo patch through LDS (yl_convc.hip, round 5).  Not behind tile_hint: these layers carry more tap
  // weights than the 32 KB image of the other depthwise-prologue kernels, nothing else can run them
  // depthwise 3x3 -> wide 1x1 with 16 / 21 n-tiles (the 244- / 328-channel neck and head blocks): the input window through
  // LDS where the grid fills 8 x 8-pixel windows (yl_conv_dwl_kernel), else streamed weights with the taps from L1/L2
  // (yl_conv_dwk_kernel).  In front of yl_conv_dws_kernel, which also runs these shapes but slower (244 -> 244 @80x80 B = 32:
  // 0.45 ms against 0.36 for yl_conv_dwk_kernel -- it took them over unnoticed when it was written for the 528 - 1248-channel
  // 5x5 layers)
  if (n == 1 && p.dw_k == 3 && p.dw_stride == 1 && tile_hint != 6 && tile_hint != 3) {
    const YlDwForm f = yl_dwk_form(p);
    if (f.family) return f;
  }
  if (n == 1) {
    const YlDwForm f = yl_dws_form(p);
    if (f.family) return f;
  }
  // depthwise 3x3 -> wide 1x1 whose weight image is beyond LDS: streamed weights, taps from L1/L2 (yl_convc.hip)
  if (n == 1 && p.dw_k == 3 && tile_hint != 6 && tile_hint != 3) {
    const YlDwForm f = yl_dwk_form(p);
    if (f.family) return f;
  }
  // depthwise prologue with LDS-staged halo tiles (4x4 output pixels per wave)
  bool halo = (p.dw_k == 3 || p.dw_k == 5) && (p.dw_stride == 1 || p.dw_stride == 2) && (p.N & 3) == 0 && tile_hint != 3;
  for (int k = 0; k < n; ++k)
    halo = halo && (m.p[k].OH & 3) == 0 && (m.p[k].OW & 3) == 0 &&
           (size_t)m.p[k].B * m.p[k].H * m.p[k].W * m.p[k].Cin * 4 < ((size_t)1 << 31);
  if (halo && tile_hint != 6 && tile_hint != 7) {
    // wave-autonomous kernel (yl_convc.hip): one tile per wave, A fragments from L1/L2, ~15 KB of LDS per workgroup
    const YlDwForm f = yl_dwt_form(m);
    if (f.family) return f;
  }
  if (halo && tile_hint == 7) {
    // producer / consumer kernel (yl_convc.hip: 4 depthwise waves + 4 GEMM waves per workgroup, 1x1 weights resident
    // in registers).  OPT-IN (tile_hint 7): faster in isolation on the K >= 192 layers (28 vs 38 us, 44 vs 50 us at
    // 20x20, B = 64) but 0.5 % slower in the two-stream pipeline (31.10 k vs 31.27 k images/s): its workgroups
    // hold ~100-130 KB of LDS and 8 waves per CU, which keeps the other chunk's kernels off those CUs.
    const YlDwForm f = yl_dwc_form(m);
    if (f.family) return f;
  }
  if (halo && YlDwhLds{NT, p.dw_k, p.dw_stride, p.KB, p.Cin}.bytes() <= YlDwhLds::LIMIT)
    return {YL_DWF_DWH, {NT, p.dw_k, p.dw_stride, 0, 0, 0}};
  // yl_conv_mfma_kernel's depthwise-prologue modes: one m-tile per wave (register budget -> occupancy)
  int CH = 0;
  if (!yl_mfma_chunk(p, NT, 1, &CH)) return none;
  return {YL_DWF_MFMA, {NT, 1, p.dw_k == 3 ? YL_CM_DW3 : p.dw_k == 5 ? YL_CM_DW5 : YL_CM_DWPRO, CH, 0, 0}};
}

// choose (NT, MT, chunking) for a layer -- or for up to 4 layers of identical configuration that run as ONE
// launch (YlConvMulti) -- and launch.  tile_hint: 0 = auto, 1/2 = force MT.
hipError_t yl_launch_conv_multi(const YlConvP* ps, int n, int tile_hint, hipStream_t st) {
  if (n < 1 || n > 4) return hipErrorInvalidValue;
#if !YL_BF16
  if (n == 1 && ps[0].w3p && ps[0].k == 3 && ps[0].stride == 2 && tile_hint != 6 && !(ps[0].dev & YL_DEV_S2C_OFF)) {   // 3x3 s2 + chained 1x1, staged patch
    const hipError_t e = yl_launch_conv_s2c(ps[0], st);
    if (e != hipErrorNotSupported) return e;
  }
#endif
  if (ps[0].k == 1 && ps[0].dw_k == 0 && ps[0].dec_boxes && !ps[0].dec_raw && ps[0].w3p) {
    // head output of a segmentation model under yl_predict (yl_api.hip): 5 + C detection columns through the decode epilogue AND
    // the NM mask-coefficient columns (second weight image w3p / b3 / C3, stored plain into the level rows out / ldo).  Levels with
    // enough pixels: ONE pass over the input (yl_conv_pws_kernel's two-image form); the others as the two launches of round 4.
    YlConvP det[4], mc[4];
    int nr = 0;
    for (int k = 0; k < n; ++k) {
      const hipError_t e = tile_hint != 6 ? yl_launch_conv_pws(ps[k], st) : hipErrorNotSupported;
      if (e == hipSuccess) continue;
      if (e != hipErrorNotSupported) return e;
      det[nr] = ps[k]; det[nr].w3p = nullptr; det[nr].b3 = nullptr; det[nr].C3 = 0; det[nr].ldo = 0;
      mc[nr] = ps[k]; mc[nr].wp = ps[k].w3p; mc[nr].bias = ps[k].b3; mc[nr].N = ps[k].C3; mc[nr].NTtot = (ps[k].C3 + 15) / 16;
      mc[nr].w3p = nullptr; mc[nr].b3 = nullptr; mc[nr].C3 = 0;
      mc[nr].dec_boxes = nullptr; mc[nr].dec_scores = nullptr; mc[nr].dec_cls = nullptr; mc[nr].dec_raw = 0;
      ++nr;
    }
    if (nr == 0) return hipSuccess;
    const hipError_t e = yl_launch_conv_multi(det, nr, tile_hint, st);
    return e != hipSuccess ? e : yl_launch_conv_multi(mc, nr, tile_hint, st);
  }
  YlConvMulti m = {};
  m.n = n;
  int big = 0;
  for (int k = 0; k < n; ++k) {
    m.p[k] = ps[k];
    if (ps[k].M > ps[big].M) big = k;
    if (ps[k].NTtot != ps[0].NTtot || ps[k].KB != ps[0].KB || ps[k].TK != ps[0].TK || ps[k].dw_k != ps[0].dw_k ||
        ps[k].dw_stride != ps[0].dw_stride || ps[k].k != ps[0].k || ps[k].stride != ps[0].stride ||
        ps[k].N != ps[0].N || ps[k].Cin != ps[0].Cin || (ps[k].C1 > 0) != (ps[0].C1 > 0) ||
        (ps[k].scale != nullptr) != (ps[0].scale != nullptr))
      return hipErrorInvalidValue;
  }
  const YlConvP& p = m.p[big];                              // decisions follow the largest problem
  if (p.scale && (p.k != 1 || p.stride != 1 || p.dw_k > 0 || p.C1 > 0 || p.in_shift || p.w3p)) return hipErrorInvalidValue;
  const int NT = yl_pick_nt(p.NTtot);
  const int gy = (p.NTtot + NT - 1) / NT;
  if (n > 1 && gy != 1) return hipErrorInvalidValue;
  if (p.C1 > 0) {          // fused inverted-residual block (expand -> depthwise -> project)
    if (n == 1) {          // workgroup-level halo kernel for the shapes it is instantiated for (yl_convc.hip)
      const hipError_t ei = yl_launch_conv_ir(p, st);
      if (ei != hipErrorNotSupported) return ei;
    }
    if (n != 1 || gy != 1 || (p.OH & 3) || (p.OW & 3) || p.dw_stride != 1) return hipErrorInvalidValue;
    return yl_uib_go(p, yl_uib_lds_bytes(p.Cin, NT, p.dw_k), st, NT, p.dw_k, (p.C1 + 15) / 16);
  }
  // plain 1x1 layers (N % 4 == 0, single problem): wave-autonomous kernel (yl_convc.hip) -- every wave an independent
  // 16/32-pixel x <= 4 n-tile item with operands straight from L1/L2, thousands of waves at 8 per SIMD, no LDS
  // weight prologue, no barrier.  Measured against the persistent LDS kernel (edge_n, B = 64, eager, us): 48->96
  // @40x40 31 -> 26, 64->256 @20x20 28 -> 23, 64->480 @20x20 45 -> 35, 48->32 @80x80 40 -> 34, lateral3 32->96
  // @80x80 99 -> 81.  Same k order and epilogues: bit-identical results.  tile_hint 6 switches it off.
  if (n == 1 && p.dw_k == 0 && p.k == 1 && p.stride == 1 && tile_hint != 6) {
    // wide layers (K >= 80, >= 6 n-tiles): weight stream through LDS shared by the workgroup (yl_convc.hip, round 3)
    const hipError_t es = yl_launch_conv_pws(p, st);
    if (es != hipErrorNotSupported) return es;
  }
  if (n > 1 && p.dw_k == 0 && p.k == 1 && p.stride == 1 && tile_hint != 6 && p.dec_boxes && !p.dec_raw && p.NTtot == 6 && p.KB >= 5) {
    // head outputs with many input channels (yololite_m: 328 -> 85): the levels with enough pixels each through
    // yl_conv_pws_kernel's decode form (weights through LDS), the small ones together as before
    YlConvP rest[4];
    int nr = 0;
    for (int k = 0; k < n; ++k) {
      const hipError_t es = yl_launch_conv_pws(ps[k], st);
      if (es == hipErrorNotSupported) rest[nr++] = ps[k];
      else if (es != hipSuccess) return es;
    }
    if (nr == 0) return hipSuccess;
    if (nr < n) return yl_launch_conv_multi(rest, nr, tile_hint, st);
  }
  if (p.dw_k == 0 && p.k == 1 && p.stride == 1 && tile_hint != 6) {
    // (also the head-output layers of all levels in one launch when their decode runs in the epilogue)
    const hipError_t ep = yl_launch_conv_pwt_multi(ps, n, st);
    if (ep != hipErrorNotSupported) return ep;
  }
  // Winograd F(2x2,3x3) (option "winograd": the layer then carries p.wino)
  if (n == 1 && p.wino && tile_hint != 6) {
    const hipError_t ew = yl_launch_conv_wino(p, st);
    if (ew != hipErrorNotSupported) return ew;
  }
  // dense k x k with a weight image beyond LDS: double-buffered weight stream (yl_convc.hip); tile_hint 6 = off
  if (n == 1 && p.dw_k == 0 && p.k > 1 && tile_hint != 6) {
    const hipError_t ek = yl_launch_conv_kxk(p, st);
    if (ek != hipErrorNotSupported) return ek;
  }
  // depthwise k x k -> 1x1: the kernel yl_dw_form names (the families, their order and the tile_hint switches are there)
  const YlDwForm dwf = p.dw_k > 0 ? yl_dw_form(m, big, tile_hint) : YlDwForm{YL_DWF_NONE, {0, 0, 0, 0, 0, 0}};
  if (p.dw_k > 0) {
    switch (dwf.family) {
      case YL_DWF_DWK: case YL_DWF_DWL: return yl_launch_conv_dwk(p, dwf, st);
      case YL_DWF_DWS: return yl_launch_conv_dws(p, dwf, st);
      case YL_DWF_DWT: case YL_DWF_DWT_SPLITK: return yl_launch_conv_dwt(m, dwf, st);
      case YL_DWF_DWC: return yl_launch_conv_dwc(m, dwf, st);
      case YL_DWF_DWH: {
        const size_t lds = YlDwhLds{NT, p.dw_k, p.dw_stride, p.KB, p.Cin}.bytes();
        const YlMultiKernel kern = yl_dwh_kernels[yl_nt_index(NT)][p.dw_k == 5][p.dw_stride == 2];   // (halo: 3 / 5, 1 / 2)
        long tiles[4], wtotal = 0;
        for (int k = 0; k < n; ++k) {
          const long wt = (long)m.p[k].B * (m.p[k].OH >> 2) * (m.p[k].OW >> 2);
          tiles[k] = (wt + 3) / 4;                            // block-sized units (4 waves)
          wtotal += tiles[k];
        }
        int gx = yl_resident_blocks((const void*)kern, 256, lds, 4) / gy;
        if (gx < 8) gx = 8;
        gx &= ~7;
        if (gx > wtotal) gx = (int)wtotal;
        gx = yl_partition_blocks(m, tiles, gx);
        hipLaunchKernelGGL(kern, dim3(gx, gy), dim3(256), lds, st, m);
        return hipGetLastError();
      }
      case YL_DWF_MFMA: break;                                // below, with the other modes of yl_conv_mfma_kernel
      default: return hipErrorInvalidValue;
    }
  }
  long Mtot = 0;
  for (int k = 0; k < n; ++k) Mtot += m.p[k].M;
  int MT = 2;
  const long tiles2 = (Mtot + 127) / 128;
  if (tile_hint == 1 || (tile_hint == 0 && tiles2 * gy < 2 * YL_NUM_CU)) MT = 1;
  if (p.dw_k > 0) MT = 1;           // depthwise prologue: one m-tile per wave (register budget -> occupancy)
  // LDS weight chunk: whole K if it fits, else stream 48 KiB chunks (a depthwise layer: yl_dw_form's answer)
  int CH;
  if (p.dw_k > 0) CH = dwf.a[3];
  else if (!yl_mfma_chunk(p, NT, MT, &CH)) return hipErrorInvalidValue;
  const size_t lds = YlMfmaLds::bytes(CH, NT, MT, p.dw_k, p.Cin, p.N);
  const int mode = p.dw_k > 0 ? dwf.a[2] : ((p.k == 1 && p.stride == 1) ? (p.scale ? YL_CM_PWSC : YL_CM_PW) : YL_CM_KXK);
  long tiles[4], ttotal = 0;
  for (int k = 0; k < n; ++k) {
    m.p[k].CH = CH;
    m.p[k].ntiles = (int)(((long)m.p[k].M + 64 * MT - 1) / (64 * MT));
    tiles[k] = m.p[k].ntiles;
    ttotal += tiles[k];
  }
  const YlMultiKernel kern = yl_mfma_kernels[yl_nt_index(NT)][MT - 1][mode];
  int gx = yl_resident_blocks((const void*)kern, 256, lds, 4) / gy;
  if (gx < 8) gx = 8;
  gx &= ~7;                         // multiple of 8: N-chunks of one M tile land on the same XCD/L2
  if (gx > ttotal) gx = (int)ttotal;
  gx = yl_partition_blocks(m, tiles, gx);
  hipLaunchKernelGGL(kern, dim3(gx, gy), dim3(256), lds, st, m);
  return hipGetLastError();
}

hipError_t yl_launch_conv(const YlConvP& p, int tile_hint, hipStream_t st) {
  return yl_launch_conv_multi(&p, 1, tile_hint, st);
}

hipError_t yl_launch_stem(const YlConvP& p0, hipStream_t st) {
  YlConvP p = p0;
  constexpr int MT = 4;
  p.ntiles = (int)(((long)p.M + 64 * MT - 1) / (64 * MT));
  int gx = 8 * YL_NUM_CU;
  if (gx > p.ntiles) gx = p.ntiles;
  if (p.N == 32) hipLaunchKernelGGL((yl_stem_mfma_kernel<2, MT>), dim3(gx), dim3(256), 0, st, p);
  else if (p.N == 16) hipLaunchKernelGGL((yl_stem_mfma_kernel<1, MT>), dim3(gx), dim3(256), 0, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// waves per image of the pooling launch: ~4 blocks of 4x2 pixels per wave, at most 64 (the gate sums them serially)
#if !YL_BF16
int yl_dw_pool_wpi(int k, int stride, int cin, int n, int oh, int ow) {
  if ((k != 3 && k != 5) || (stride != 1 && stride != 2) || (cin & 3) || n != cin || oh < 1 || ow < 1) return 0;
  const long per = (long)((oh + 1) / 2) * ((ow + 3) / 4);
  long w = (per + 3) / 4;
  if (w > 64) w = 64;
  if (w < 1) w = 1;
  return (int)w;
}
#endif

template <int K, int S>
static hipError_t yl_launch_dw_tile(const YlConvP& p, hipStream_t st) {
  const int gx = (p.Cin + 255) / 256;
  if (p.pool) {
    const long waves = (long)p.B * p.pool_wpi;
    hipLaunchKernelGGL((yl_dw_tile_kernel<K, S, true>), dim3((unsigned)gx, (unsigned)((waves + 3) / 4)), dim3(256), 0, st, p);
    return hipGetLastError();
  }
  const long nblk = (long)p.B * ((p.OH + 1) / 2) * ((p.OW + 3) / 4);
  long gy = (long)8 * YL_NUM_CU / gx;                         // ~8 workgroups per CU in flight, persistent over the rest
  if (gy > (nblk + 3) / 4) gy = (nblk + 3) / 4;
  if (gy < 1) gy = 1;
  hipLaunchKernelGGL((yl_dw_tile_kernel<K, S>), dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, p);
  return hipGetLastError();
}

// Which kernel runs the stand-alone depthwise layer p (yl_internal.h)
YlDwForm yl_dw_alone_form(const YlConvP& p) {
  const bool tile_off = (p.dev & YL_DEV_DW_TILE_OFF) != 0 && !p.pool;   // developer A/B (yl_set_option "dev_select")
  if (p.pool && (p.res || p.pool_wpi != yl_dw_pool_wpi(p.k, p.stride, p.Cin, p.N, p.OH, p.OW) || p.pool_wpi < 1))
    return {YL_DWF_NONE, {0, 0, 0, 0, 0, 0}};
  if (!tile_off && (p.Cin & 3) == 0 && p.N == p.Cin && (p.k == 3 || p.k == 5) && (p.stride == 1 || p.stride == 2))
    return {YL_DWF_DW_TILE, {p.k, p.stride, 0, 0, 0, 0}};
  return {YL_DWF_DW, {0, 0, 0, 0, 0, 0}};
}

hipError_t yl_launch_dw(const YlConvP& p, hipStream_t st) {
  const YlDwForm f = yl_dw_alone_form(p);
  if (f.family == YL_DWF_NONE) return hipErrorInvalidValue;
  if (f.family == YL_DWF_DW_TILE) {
    if (f.a[0] == 3 && f.a[1] == 1) return yl_launch_dw_tile<3, 1>(p, st);
    if (f.a[0] == 3 && f.a[1] == 2) return yl_launch_dw_tile<3, 2>(p, st);
    if (f.a[0] == 5 && f.a[1] == 1) return yl_launch_dw_tile<5, 1>(p, st);
    if (f.a[0] == 5 && f.a[1] == 2) return yl_launch_dw_tile<5, 2>(p, st);
  }
  const size_t total = (size_t)p.M * (p.Cin >> 2);
  hipLaunchKernelGGL(yl_dw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p);
  return hipGetLastError();
}
