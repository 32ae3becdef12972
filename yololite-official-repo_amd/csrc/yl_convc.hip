// Block-cooperative depthwise -> 1x1 convolution for gfx950 (MI355X / CDNA4), fp32 in / fp32 accumulate.
//
// Same layer as yl_conv_dwh_kernel (yl_conv.hip): depthwise DK x DK (stride DS) + bias + act, then a 1x1 conv
// (dw -> pw pairs of the reference's DWConvBlock, model_v2.py:23-39, and of the timm UIB / inverted-residual
// blocks behind model_v2.py:94-100,266-272), the depthwise result never touching HBM.  Different decomposition,
// built for the layers whose pixel count cannot fill the chip (40x40 / 20x20 grids: a few hundred to a few
// thousand 16-pixel tiles per launch).  yl_conv_dwh_kernel gives every WAVE a 4x4-pixel tile end to end: the wave
// walks all K/16 channel blocks serially (halo fetch -> taps -> MFMAs for every n-tile), one wave per SIMD, and
// every block first copies the whole 1x1 weight matrix into LDS.  rocprofv3 (profiles/r01_pmc_summary.txt): such
// a wave lives 52 k cycles of which 7.5 k are MFMA issue -- the rest is waiting for memory with nothing else
// resident to run.
//
// Here the FOUR waves of a workgroup share one 4x4-pixel tile:
//   phase 1 (K split)  wave w takes channel blocks w, w+4, ...: stages the (3*DS+DK)^2 halo patch of 16 channels in
//                      its private LDS region (loads issued one block ahead, also across tiles), forms
//                      B = act(bias + sum_taps w*x) and writes the fragment to a block-shared LDS buffer;
//   barrier
//   phase 2 (N split)  wave w owns n-tiles [w*NTW, (w+1)*NTW): its 1x1 weights (MFMA A fragments, all K) were
//                      loaded ONCE per workgroup into REGISTERS -- no LDS weight image, no weight prologue per
//                      tile -- and it runs the k loop over the shared B fragments, then the epilogue.
// The serial chain per tile is 4x shorter, 4x as many waves are resident per tile, and because every output
// still sums its k blocks in ascending order the results are BIT-IDENTICAL to yl_conv_dwh_kernel / the generic
// conv kernel (tests/test_gpu_parity.py: test_convc_kernels_are_bitwise_the_kernels_they_replace).
//
// Limits (launcher falls back to yl_conv_dwh_kernel otherwise): OH, OW multiples of 4, N % 4 == 0,
// NTW = ceil(ceil(N/16)/4) <= 5 and ceil(Cin/16) <= KBMAX(NTW) (the register budget of the resident weights).
#include "yl_lp.h"
#if YL_BF16
#define yl_conv_dwc_kernel YL_LP_NAME(yl_conv_dwc_kernel)
#define yl_launch_conv_dwc YL_LP_NAME(yl_launch_conv_dwc)
#define yl_dwc_form YL_LP_NAME(yl_dwc_form)
#define yl_dwt_form YL_LP_NAME(yl_dwt_form)
#define yl_dwk_form YL_LP_NAME(yl_dwk_form)
#define yl_dws_form YL_LP_NAME(yl_dws_form)
#define yl_convc_init YL_LP_NAME(yl_convc_init)
#define yl_conv_pwt_kernel YL_LP_NAME(yl_conv_pwt_kernel)
#define yl_launch_conv_pwt YL_LP_NAME(yl_launch_conv_pwt)
#define yl_launch_conv_pwt_multi YL_LP_NAME(yl_launch_conv_pwt_multi)
#define yl_conv_dwt_kernel YL_LP_NAME(yl_conv_dwt_kernel)
#define yl_launch_conv_dwt YL_LP_NAME(yl_launch_conv_dwt)
#define yl_conv_dwk_kernel YL_LP_NAME(yl_conv_dwk_kernel)
#define yl_conv_dwl_kernel YL_LP_NAME(yl_conv_dwl_kernel)
#define yl_launch_conv_dwk YL_LP_NAME(yl_launch_conv_dwk)
#define yl_conv_dws_kernel YL_LP_NAME(yl_conv_dws_kernel)
#define yl_launch_conv_dws YL_LP_NAME(yl_launch_conv_dws)
#define yl_conv_wino_kernel YL_LP_NAME(yl_conv_wino_kernel)
#define yl_launch_conv_wino YL_LP_NAME(yl_launch_conv_wino)
#define yl_conv_kxk_kernel YL_LP_NAME(yl_conv_kxk_kernel)
#define yl_launch_conv_kxk YL_LP_NAME(yl_launch_conv_kxk)
#define yl_conv_pws_kernel YL_LP_NAME(yl_conv_pws_kernel)
#define yl_launch_conv_pws YL_LP_NAME(yl_launch_conv_pws)
#define yl_ir_kernel YL_LP_NAME(yl_ir_kernel)
#define yl_launch_conv_ir YL_LP_NAME(yl_launch_conv_ir)
#define yl_ir_supported YL_LP_NAME(yl_ir_supported)
#define yl_ir_form YL_LP_NAME(yl_ir_form)
#endif
#include <stdlib.h>
#include <type_traits>
#include "yl_internal.h"
#include "yl_dev.h"
#include "yl_epi.h"


template <int NTW>
struct YlDwcCfg {
  static constexpr int KBMAX = NTW == 1 ? 18 : NTW == 2 ? 9 : NTW == 3 ? 6 : 4;
};

#define YL_SELECT_PROBLEM_C(m)                                                      \
  int yl_k = 0;                                                                     \
  if ((m).n > 1 && (int)blockIdx.x >= (m).p[1].blk0) yl_k = 1;                     \
  if ((m).n > 2 && (int)blockIdx.x >= (m).p[2].blk0) yl_k = 2;                     \
  if ((m).n > 3 && (int)blockIdx.x >= (m).p[3].blk0) yl_k = 3;                     \
  const YlConvP& p = (m).p[yl_k];                                                   \
  const int bx = p.nblk ? (int)blockIdx.x - p.blk0 : (int)blockIdx.x;               \
  const int gx = p.nblk ? p.nblk : (int)gridDim.x;

// patch row pitch in floats (32 channels per pixel): HP pixels + padding chosen so that the 16 lanes of every
// ds_read_b128 service group -- (row py, pixel pair xh, channel half) combinations -- hit 16 distinct 16-byte slots
constexpr __host__ __device__ int yl_dwc_hp(int dk, int ds) { return 3 * ds + dk; }
constexpr __host__ __device__ int yl_dwc_pitch(int dk, int ds) {
  const int hp = yl_dwc_hp(dk, ds);
  return ds == 1 ? hp * 32 + ((hp * 128) % 256 == 128 ? 0 : 32) : hp * 32 + 16;
}
template <int DK, int DS>
struct YlDwcGeo {
  static constexpr int HP = yl_dwc_hp(DK, DS);
  static constexpr int PITCH = yl_dwc_pitch(DK, DS);
  static constexpr int HALF_F = HP * PITCH;                    // floats of one half patch (32 channels)
  static constexpr int RI = (HP + 7) / 8;                      // LDS-DMA instructions per patch row (8 pixels x 128 B each)
  static constexpr int NDMA = HP * RI;                         // instructions per half patch
};

// dynamic LDS of yl_conv_dwc_kernel, its regions in order and their floats: [2][KB][64] float4 B fragments | [DK*DK][Cin] taps,
// [Cin] bias | one half patch per producer wave that has a 64-channel group to stage (at most 4).  (Region sizes, which the kernel
// adds up as it walks the regions, not offsets: with the offsets precomputed the kernels came out with another schedule.)
struct YlDwcLds {
  static constexpr size_t LIMIT = 150 * 1024;
  int dk, ds, KB, Cin;
  constexpr __host__ __device__ size_t bfrag() const { return (size_t)2 * KB * 256; }
  constexpr __host__ __device__ size_t taps() const { return yl_taps_floats(dk, Cin); }
  constexpr __host__ __device__ size_t halo() const { return (size_t)((KB + 3) / 4 < 4 ? (KB + 3) / 4 : 4) * yl_dwc_hp(dk, ds) * yl_dwc_pitch(dk, ds); }
  constexpr __host__ __device__ size_t bytes() const { return (bfrag() + taps() + halo()) * 4; }
};

template <int DK, int DS, int NTW>
__global__ __launch_bounds__(512, 2) void yl_conv_dwc_kernel(YlConvMulti mp) {
  YL_SELECT_PROBLEM_C(mp)
  using G = YlDwcGeo<DK, DS>;
  constexpr int KBMAX = YlDwcCfg<NTW>::KBMAX;
  constexpr int HP = G::HP, PITCH = G::PITCH, NR = DS + DK;     // NR: patch columns a lane reads per tap row
  extern __shared__ __attribute__((aligned(16))) float yl_clds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool producer = wave < 4;
  const int KB = p.KB;
  const int NG = (KB + 3) >> 2;                                 // 64-channel groups
  const YlDwcLds L = {DK, DS, KB, p.Cin};
  f32x4* bbuf = reinterpret_cast<f32x4*>(yl_clds);
  float* dwl = yl_clds + L.bfrag();
  float* halo0 = dwl + L.taps();
  // every parameter the loops need, read ONCE: `p` points into the kernel-argument segment (problem selected at
  // run time), and the compiler re-reads such fields with s_load + s_waitcnt lgkmcnt(0) wherever it runs short of
  // SGPRs -- inside the tap / copy loops that was most of their time
  const int Cin = p.Cin, H = p.H, W = p.W, OH = p.OH, OW = p.OW, N = p.N, NTtot = p.NTtot, dw_act = p.dw_act;
  const int pad_t = p.dw_pad_t, pad_l = p.dw_pad_l;
  const yl_act_t* const xin = p.x;
  const long zdelta = p.zeros - p.x;                            // float offset of the zero buffer from the input tensor
  const int tw = OW >> 2, th = OH >> 2;
  const int tiles_img = tw * th;
  const int ntiles = p.B * tiles_img;
  // Tiles of this workgroup: t0, t0 + tstride, ... (nmine of them), tile = (image * th + tile row) * tw + tile column.
  // XCD-aware when the grid allows it (gx % 8 == 0 and, in a level-batched launch, the problem starts at a multiple
  // of 8): workgroup b runs on XCD b % 8 (observed dispatch order; a different placement changes speed only), and
  // XCD x owns the contiguous band [x*U/8, (x+1)*U/8) of the U = B * th tile rows -- whole images for B % 8 == 0, the
  // SAME images in every layer, so the halo overlap of neighbouring tiles and the producer layer's output are found
  // in this XCD's L2 instead of crossing the fabric from another XCD's.
  // (Neither yl_band_split nor yl_xcd_range: the bands are cut between tile ROWS, U of them, and dealt tile by tile.)
  int t0, tstride, nmine;
  if ((gx & 7) == 0 && ((int)blockIdx.x & 7) == (bx & 7)) {
    const int U = p.B * th, x = bx & 7, j = bx >> 3, nj = gx >> 3;
    const int r0 = (int)(((long)U * x) >> 3), r1 = (int)(((long)U * (x + 1)) >> 3);
    const int cnt = (r1 - r0) * tw;
    t0 = r0 * tw + j; tstride = nj;
    nmine = j < cnt ? (cnt - 1 - j) / nj + 1 : 0;
  } else {
    t0 = bx; tstride = gx;
    nmine = bx < ntiles ? (ntiles - 1 - bx) / gx + 1 : 0;
  }

  {                                                              // depthwise taps + bias -> LDS (asynchronous)
    const int nw = DK * DK * Cin;
    yl_glds_floats(p.dw_w, dwl, nw, tid, 512);
    if (p.dw_b) yl_glds_floats(p.dw_b, dwl + nw, Cin, tid, 512);
    else for (int i = tid; i < Cin; i += 512) dwl[nw + i] = 0.0f;
  }

  if (producer) {
    // =================================================================================== depthwise waves
    // lane = (output row py, pixel pair xh, 4 of the half group's 32 channels): 2 output pixels per lane, NR float4
    // patch reads + DK tap reads per tap row.  Steps of a tile: (group g = wave, wave + 4, ...) x (half 0, 1).
    const int py = lane >> 4, xh = (lane >> 3) & 1, c8 = lane & 7;
    float* hreg = halo0 + wave * G::HALF_F;
    const float dlo = yl_act_lo(dw_act), dhi = yl_act_hi(dw_act);
    // half patch (32 channels from c0) of a tile: HP rows x RI float4 per lane (lane = (pixel column lane >> 3 [+ 8q],
    // 4 channels)), fetched into registers one step ahead and written to the wave's LDS patch right before its taps.
    // (Asynchronous global->LDS copies were measured first: ~150-230 issue cycles per 1-KiB piece on the issuing wave,
    // 1200-1900 cycles per half patch -- more than the taps themselves; loads + ds_write_b128 cost a fraction.)
    // Pixels outside the image and channels beyond Cin come from a zero buffer (the depthwise zero padding).
    f32x4 stg[HP * G::RI];
    auto load_half = [&](int tile, int c0) {
      const int b = tile / tiles_img;
      const int trem = tile - b * tiles_img;
      const int tyi = trem / tw, txi = trem - tyi * tw;
      const int iy0 = 4 * tyi * DS - pad_t, ix0 = 4 * txi * DS - pad_l;
      const int cc = c0 + (lane & 7) * 4;
      const bool cok = cc < Cin;
      const long img = (long)b * H * W * Cin + cc;
      const long zoff = zdelta + (lane & 7) * 4;
      long coloff[G::RI];
      bool colok[G::RI];
#pragma unroll
      for (int q = 0; q < G::RI; ++q) {
        const int ix = ix0 + q * 8 + (lane >> 3);
        colok[q] = cok && ix >= 0 && ix < W && q * 8 + (lane >> 3) < HP;
        coloff[q] = img + (long)ix * Cin;
      }
#pragma unroll
      for (int r = 0; r < HP; ++r) {
        const int iy = iy0 + r;                                   // wave-uniform
        const bool rowok = iy >= 0 && iy < H;
        const long rowoff = (long)iy * W * Cin;
#pragma unroll
        for (int q = 0; q < G::RI; ++q) {
          const long off = (rowok && colok[q]) ? rowoff + coloff[q] : zoff;     // select, no branch
          stg[r * G::RI + q] = yl_ld4(xin + off);
        }
      }
    };
    auto store_half = [&](float* dst) {
#pragma unroll
      for (int r = 0; r < HP; ++r)
#pragma unroll
        for (int q = 0; q < G::RI; ++q)
          if (q * 8 + 7 < HP || q * 8 + (lane >> 3) < HP)
            *reinterpret_cast<f32x4*>(dst + r * PITCH + q * 256 + lane * 4) = stg[r * G::RI + q];
    };
    // step stream of this wave: s = 0, 1, ... over (tile index, group, half)
    const int gcount = NG > wave ? (NG - 1 - wave) / 4 + 1 : 0;   // groups of this wave per tile
    auto halves_of = [&](int g) { return (4 * g + 2 < KB) ? 2 : 1; };
    int st_it = 0, st_gi = 0, st_h = 0;                           // the step whose patch is requested NEXT
    auto step_valid = [&]() { return gcount > 0 && st_it < nmine; };
    auto step_c0 = [&]() { return (wave + 4 * st_gi) * 64 + st_h * 32; };
    auto step_advance = [&]() {
      if (++st_h >= halves_of(wave + 4 * st_gi)) { st_h = 0; if (++st_gi >= gcount) { st_gi = 0; ++st_it; } }
    };
    if (step_valid()) { load_half(t0 + st_it * tstride, step_c0()); step_advance(); }
    __syncthreads();                                              // taps are in LDS (drains the copy queue once)
    for (int it = 0; it <= nmine; ++it) {
      if (it < nmine) {
        f32x4* bb = bbuf + (size_t)(it & 1) * KB * 64;
        for (int gi = 0; gi < gcount; ++gi) {
          const int g = wave + 4 * gi;
          const int nh = halves_of(g);
          for (int h = 0; h < nh; ++h) {
            store_half(hreg);                                       // this step's patch: registers -> LDS (after the
                                                                    // previous step's tap reads, in LDS order)
            if (step_valid()) { load_half(t0 + st_it * tstride, step_c0()); step_advance(); }   // next step's patch: in flight under the taps
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // patch writes (all lanes) -> tap reads
            const float* hp_ = hreg;
            const int c = g * 64 + h * 32 + c8 * 4;
            const int cs = c < Cin ? c : Cin - 4;
            const float* tapw = dwl + cs;                            // tap t of this lane's 4 channels: tapw[t * Cin]
            f32x4 o[2];
            o[0] = o[1] = yl_ld4(tapw + DK * DK * Cin);
            const float* hrow = hp_ + (size_t)(py * DS) * PITCH + (2 * xh * DS) * 32 + c8 * 4;
            // tap rows: row dy+1 is read while row dy is multiplied (two rows of registers; unrolling all DK rows
            // spills for 5x5)
            f32x4 vn[NR], wn[DK];
#pragma unroll
            for (int x = 0; x < NR; ++x) vn[x] = *reinterpret_cast<const f32x4*>(hrow + x * 32);
#pragma unroll
            for (int dx = 0; dx < DK; ++dx) wn[dx] = yl_ld4(tapw + dx * Cin);
#pragma unroll 1
            for (int dy = 0; dy < DK; ++dy) {
              f32x4 v[NR], w[DK];
#pragma unroll
              for (int x = 0; x < NR; ++x) v[x] = vn[x];
#pragma unroll
              for (int dx = 0; dx < DK; ++dx) w[dx] = wn[dx];
              if (dy + 1 < DK) {
#pragma unroll
                for (int x = 0; x < NR; ++x) vn[x] = *reinterpret_cast<const f32x4*>(hrow + (dy + 1) * PITCH + x * 32);
#pragma unroll
                for (int dx = 0; dx < DK; ++dx) wn[dx] = yl_ld4(tapw + ((dy + 1) * DK + dx) * Cin);
              }
#pragma unroll
              for (int dx = 0; dx < DK; ++dx)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                  const f32x4 a = v[j * DS + dx];
                  o[j].x = fmaf(a.x, w[dx].x, o[j].x); o[j].y = fmaf(a.y, w[dx].y, o[j].y);
                  o[j].z = fmaf(a.z, w[dx].z, o[j].z); o[j].w = fmaf(a.w, w[dx].w, o[j].w);
                }
            }
            // B fragment of channel block kb: lane (kq = c8 & 3, pixel py*4 + 2*xh + j).  Blocks beyond KB (group
            // tail) are not stored; channels beyond Cin inside a block were loaded from the zero buffer (load_half) and
            // meet zero 1x1 weights.
            if (it == 2 && gi == 0) asm volatile("" :: "v"(o[0].x), "v"(o[1].x));   // (no-op anchor: see the GEMM waves)
            const int kb = 4 * g + 2 * h + (c8 >> 2);
            if (kb < KB) {
#pragma unroll
              for (int j = 0; j < 2; ++j)
                bb[kb * 64 + (c8 & 3) * 16 + py * 4 + 2 * xh + j] = yl_actc(o[j], dw_act, dlo, dhi);
            }
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");            // B fragments written; the patch copy stays in flight
      __builtin_amdgcn_s_barrier();
    }
  } else {
    // =================================================================================== GEMM waves
    const int cw = wave - 4;
    const int kq = lane >> 4, pl = lane & 15;
    const int nt0 = cw * NTW;
    const bool p2 = nt0 < NTtot;                                   // this wave owns output channels
    const yl_act_t* const resp = p.res;
    yl_act_t* const outp = p.out;
    const float lo = yl_act_lo(p.act), hi = yl_act_hi(p.act);
    f32x4 wreg[KBMAX][NTW], breg[NTW];
    {
      const f32x4* wg = reinterpret_cast<const f32x4*>(p.wp);
#pragma unroll
      for (int kb = 0; kb < KBMAX; ++kb)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
          const bool ok = kb < KB && nt0 + nt < NTtot;
          wreg[kb][nt] = ok ? wg[((size_t)kb * NTtot + nt0 + nt) * 64 + lane] : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) breg[nt] = yl_ld4(p.bias + (nt0 + nt) * 16 + 4 * kq);   // bias is padded
    }
    const bool pre_add = p.res != nullptr && p.up == nullptr && p.act == YL_ACT_NONE;
    const bool generic = !pre_add && (p.res || p.up || YL_SMOOTH(p.act));
    __syncthreads();
    for (int it = 0; it <= nmine; ++it) {
      if (it >= 1 && p2) {
        const int tile = t0 + (it - 1) * tstride;
        const f32x4* bb = bbuf + (size_t)((it - 1) & 1) * KB * 64;
        const int b = tile / tiles_img;
        const int trem = tile - b * tiles_img;
        const int tyi = trem / tw, txi = trem - tyi * tw;
        YlPix px[1];
        px[0].b = b;
        px[0].oy = 4 * tyi + (pl >> 2);
        px[0].ox = 4 * txi + (pl & 3);
        px[0].valid = true;
        px[0].lin = ((size_t)b * OH + px[0].oy) * OW + px[0].ox;
        f32x4 acc[1][NTW];
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
          const int n = (nt0 + nt) * 16 + 4 * kq;
          acc[0][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
          if (pre_add && n < N) acc[0][nt] = yl_ld4(resp + px[0].lin * N + n);
        }
        // (The empty asm statements of this kernel are no-ops left from a retired measurement.  Register allocation differs
        // without them; they stay until the kernel's code is next allowed to change.)
        if (it == 3) asm volatile("" :: "v"(acc[0][0].x));
        // B fragments are read PF channel blocks ahead of their MFMAs (one ds_read_b128 each; the depthwise waves
        // keep the LDS pipe busy, so a read issued one block ahead returned too late)
        constexpr int PF = KBMAX < 4 ? KBMAX : 4;
        f32x4 xr[PF];
#pragma unroll
        for (int i = 0; i < PF; ++i) xr[i] = bb[(i < KB ? i : 0) * 64 + lane];
#pragma unroll
        for (int kb = 0; kb < KBMAX; ++kb) {
          if (kb < KB) {
            f32x4 xq[1];
            xq[0] = xr[kb % PF];
            if (kb + PF < KBMAX) xr[kb % PF] = bb[(kb + PF < KB ? kb + PF : 0) * 64 + lane];
            yl_mma_step<NTW, 1>(wreg[kb], xq, acc);
          }
        }
        if (it == 3) asm volatile("" :: "v"(acc[0][0].x));
        if (generic) yl_epi_generic<NTW, 1>(p, acc, px, nt0, kq);
        else {                                                      // == yl_epi_fast with the bias from registers
          yl_act_t* orow = outp + px[0].lin * N;
#pragma unroll
          for (int nt = 0; nt < NTW; ++nt) {
            const int n = (nt0 + nt) * 16 + 4 * kq;
            const f32x4 v = yl_clamp4(acc[0][nt] + breg[nt], lo, hi);
            if (n < N) yl_st4(orow + n, v);
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");            // this tile's B-fragment reads are complete
      __builtin_amdgcn_s_barrier();
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Wave-autonomous 1x1 convolution for launches whose pixel count cannot fill the chip with 4-wave tiles
// (40x40 / 20x20 / 10x10 grids).  yl_conv_mfma_kernel (yl_conv.hip) is built for streaming many tiles per
// workgroup: persistent grid, weight image copied to LDS first, a wave walks all n-tiles of its pixels.  At
// M = 25 600 pixels that is 400 workgroups that spend their life in the weight prologue and one dependent tile:
// 25-47 us for layers whose MFMA time is 2-5 us.  Here every WAVE is an independent work item -- 16*MT pixels x
// NTW n-tiles -- with no LDS and no barrier: the A fragments (weights) and B fragments (activations) come straight
// from global memory (L1/L2-resident: the 4 waves of a workgroup share one pixel group, all workgroups share the
// weights), ~70 VGPRs, so 6-8 waves per SIMD cover each other's load latency and MFMA dependency chains, and the
// launch has thousands of waves instead of a few hundred.  Same k order, same epilogues as yl_conv_mfma_kernel:
// bit-identical results.
// SC: the input is multiplied by a squeeze-excite gate [B][Cin] (YlConvP::scale) in the B-operand path -- x * gate in one
// fp32 rounding, then the GEMM (timm: `x * gate` feeds conv_pwl).
template <int NTW, int MT, bool DEC, bool SC = false>
__global__ __launch_bounds__(256) void yl_conv_pwt_kernel(YlConvMulti mp, int nchunk) {
  YL_SELECT_PROBLEM_C(mp)                                   // level-batched launches: block ranges per problem
  (void)gx;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, pl = lane & 15;
  const int item = bx * 4 + wave;
  const int mg = item / nchunk, nc = item - mg * nchunk;
  const int nt0 = nc * NTW;
  const int Cin = p.Cin, N = p.N, NTtot = p.NTtot, KB = p.KB, M = p.M;
  if ((long)mg * (MT * 16) >= M) return;
  const yl_act_t* const xin = p.x;
  const f32x4* const wg = reinterpret_cast<const f32x4*>(p.wp);
  YlPix px[MT];
  const yl_act_t* xrow[MT];
  const float* srow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    // yl_pix written out: ohw is formed only where coordinates are wanted, and the kernels come out with another schedule
    // when the helper takes it as an argument
    size_t lin = (size_t)mg * (MT * 16) + mt * 16 + pl;
    px[mt].valid = lin < (size_t)M;
    if (!px[mt].valid) lin = (size_t)M - 1;
    px[mt].lin = lin;
    px[mt].b = 0; px[mt].oy = 0; px[mt].ox = 0;
    if (DEC || SC || p.up) {                                // only the upsample-add / decode epilogues / the gate need coordinates
      const int ohw = p.OH * p.OW;
      const int b = (int)(lin / ohw);
      const int rem = (int)(lin - (size_t)b * ohw);
      px[mt].b = b;
      px[mt].oy = rem / p.OW;
      px[mt].ox = rem - px[mt].oy * p.OW;
    }
    xrow[mt] = xin + lin * Cin + 4 * kq;
    srow[mt] = SC ? p.scale + (size_t)px[mt].b * Cin + 4 * kq : nullptr;
  }
  // n-tiles beyond the layer's last one (partial last chunk): read the last tile's weights, never stored
  int wofs[NTW];
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt) wofs[nt] = ((nt0 + nt < NTtot ? nt0 + nt : NTtot - 1) * 64 + lane);
  f32x4 acc[MT][NTW];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // residual / upsample-add without activation: the addends initialise the accumulators (as yl_conv_mfma_kernel)
  const bool pre_add = (p.res || p.up) && p.act == YL_ACT_NONE;
  if (pre_add) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const size_t obase = px[mt].lin * N;
      size_t up_off = 0;
      if (p.up) {
        const int uy = (px[mt].oy * p.UH) / p.OH, ux = (px[mt].ox * p.UW) / p.OW;
        up_off = (((size_t)px[mt].b * p.UH + uy) * p.UW + ux) * N;
      }
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) {
        const int n = (nt0 + nt) * 16 + 4 * kq;
        if (n < N) {
          if (p.res) acc[mt][nt] = yl_ld4(p.res + obase + n);
          if (p.up) acc[mt][nt] += yl_ld4(p.up + up_off + n);
        }
      }
    }
  }
  constexpr int UK = 2;
  const int cin4 = Cin - 4;
  for (int kb0 = 0; kb0 < KB; kb0 += UK) {
    f32x4 a[UK][NTW], bq[UK][MT];
#pragma unroll
    for (int u = 0; u < UK; ++u) {
      const int kb = kb0 + u < KB ? kb0 + u : KB - 1;       // odd KB: the tail step re-reads the last block, unused
      const int c = kb * 16 + 4 * kq;
      const bool cok = c < Cin;                              // channel tail of the last block: zero activations
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) a[u][nt] = wg[(size_t)kb * NTtot * 64 + wofs[nt]];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        bq[u][mt] = yl_ld4(cok ? xrow[mt] + kb * 16 : p.zeros);
        if (SC) bq[u][mt] *= yl_ld4(cok ? srow[mt] + kb * 16 : reinterpret_cast<const float*>(p.zeros));
      }
    }
    (void)cin4;
#pragma unroll
    for (int u = 0; u < UK; ++u)
      if (kb0 + u < KB) yl_mma_step<NTW, MT>(a[u], bq[u], acc);
  }
  const float lo = yl_act_lo(p.act), hi = yl_act_hi(p.act);
  if (DEC) { yl_epi_decode<NTW, MT, false, true>(p, acc, px, 0, kq, lane); return; }   // (nchunk == 1: nt0 == 0)
    // head output under yl_predict (one wave = whole rows)
  if (!pre_add && (p.res || p.up || YL_SMOOTH(p.act))) yl_epi_generic<NTW, MT>(p, acc, px, nt0, kq);
  else yl_epi_fast<NTW, MT>(p, acc, px, nt0, kq, lo, hi, true);
}

template <int NTW, int MT, bool DEC = false, bool SC = false>
static hipError_t pwt_go(YlConvMulti& m, int nchunk, hipStream_t st) {
  int at = 0;
  for (int k = 0; k < m.n; ++k) {
    const long groups = ((long)m.p[k].M + MT * 16 - 1) / (MT * 16);
    const long items = groups * nchunk;
    m.p[k].blk0 = at;
    m.p[k].nblk = (int)((items + 3) / 4);
    at += m.p[k].nblk;
  }
  if (m.n == 1) m.p[0].nblk = 0;                                 // single problem: the whole grid (YL_SELECT_PROBLEM_C)
  hipLaunchKernelGGL((yl_conv_pwt_kernel<NTW, MT, DEC, SC>), dim3((unsigned)at), dim3(256), 0, st, m, nchunk);
  return hipGetLastError();
}

// n <= 4 plain 1x1 stride-1 convs of identical configuration (one launch).  Either N % 4 == 0 (float4 epilogues),
// or head-output layers whose decode runs in the epilogue and whose raw rows are not wanted (yl_predict, no mask
// coefficients): then one wave holds whole rows (N <= 96).  hipErrorNotSupported otherwise.
hipError_t yl_launch_conv_pwt_multi(const YlConvP* ps, int n, hipStream_t st) {
  if (n < 1 || n > 4) return hipErrorNotSupported;
  YlConvMulti m = {};
  m.n = n;
  long Mtot = 0;
  for (int k = 0; k < n; ++k) {
    const YlConvP& p = ps[k];
    if (p.k != 1 || p.stride != 1 || p.dw_k > 0 || p.C1 > 0 || p.in_shift) return hipErrorNotSupported;
    if (p.scale && (n != 1 || p.dec_boxes)) return hipErrorNotSupported;      // gated input: single plain layer
    const bool dec = p.dec_boxes && !p.dec_raw;
    if ((p.N & 3) && !dec) return hipErrorNotSupported;
    if (p.dec_boxes && !dec) return hipErrorNotSupported;
    if (dec && p.NTtot > 6) return hipErrorNotSupported;
    if (p.NTtot != ps[0].NTtot || p.KB != ps[0].KB || (p.dec_boxes != nullptr) != (ps[0].dec_boxes != nullptr)) return hipErrorNotSupported;
    m.p[k] = p;
    Mtot += p.M;
  }
  const YlConvP& p = ps[0];
  const int NT = p.NTtot;
  const bool dec = p.dec_boxes != nullptr;
  // n-tiles per wave: as many as 4 (the activations are fetched once per wave), chunks of equal size; decode: the row
  int ntw = dec ? (NT <= 4 ? NT : 6) : (NT <= 4 ? NT : (NT % 4 == 0 ? 4 : (NT % 3 == 0 ? 3 : 4)));
  const int nchunk = dec ? 1 : (NT + ntw - 1) / ntw;
  const bool two = Mtot >= 65536;                               // two m-tiles per wave halve the weight traffic
  if (dec) {
    switch (ntw) {
      case 1: return pwt_go<1, 1, true>(m, nchunk, st);
      case 2: return pwt_go<2, 1, true>(m, nchunk, st);
      case 3: return pwt_go<3, 1, true>(m, nchunk, st);
      case 4: return pwt_go<4, 1, true>(m, nchunk, st);
      default: return two ? pwt_go<6, 2, true>(m, nchunk, st) : pwt_go<6, 1, true>(m, nchunk, st);
    }
  }
  if (p.scale) {
    switch (ntw) {
      case 1: return pwt_go<1, 1, false, true>(m, nchunk, st);
      case 2: return pwt_go<2, 1, false, true>(m, nchunk, st);
      case 3: return pwt_go<3, 1, false, true>(m, nchunk, st);
      default: return pwt_go<4, 1, false, true>(m, nchunk, st);
    }
  }
  switch (ntw) {
    case 1: return two ? pwt_go<1, 2>(m, nchunk, st) : pwt_go<1, 1>(m, nchunk, st);
    case 2: return two ? pwt_go<2, 2>(m, nchunk, st) : pwt_go<2, 1>(m, nchunk, st);
    case 3: return two ? pwt_go<3, 2>(m, nchunk, st) : pwt_go<3, 1>(m, nchunk, st);
    default: return two ? pwt_go<4, 2>(m, nchunk, st) : pwt_go<4, 1>(m, nchunk, st);
  }
}

hipError_t yl_launch_conv_pwt(const YlConvP& p, hipStream_t st) { return yl_launch_conv_pwt_multi(&p, 1, st); }

// Chained tail of yl_conv_dwx_kernel (see there): the projection's epilogue as yl_epi_fast (bias, clamp; every pixel of a
// tile is valid, N == 16 NT), whose stored values are, lane for lane, the B fragments of k-block nt of the next layer's
// 1x1 (channels 16 nt + 4 kq .. + 3 of pixel pl), then that 1x1 in chunks of CX n-tiles: k-blocks ascending, four k-steps
// each, accumulators from zero, + bias, clamp -- the arithmetic of yl_conv_pwt_kernel.  Its A fragments come from L1/L2
// through a buffer descriptor (lane offset in a VGPR, fragment offset as a constant), the next chunk's requested before
// the current chunk's MFMAs; the expanded rows are stored the same way.
template <int NT, int NX>
__device__ __forceinline__ void yl_dwx_tail(const YlConvP& p, const f32x4 (&acc)[NT], size_t lin, int kq, int lane, float lo,
                                            float hi, yl_act_t* const out3) {
#if !YL_BF16
  constexpr int CX = 2, NC = NX / CX;
  static_assert(NX % CX == 0, "chained n-tiles come in chunks of CX");
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w3p), 0, NT * NX * 1024, 0x00020000);
  const __amdgpu_buffer_rsrc_t ors =
      __builtin_amdgcn_make_buffer_rsrc(out3, 0, (int)((long)p.B * p.OH * p.OW * NX * 64), 0x00020000);
  f32x4 w[2][NT][CX];
  auto wload = [&](int c, f32x4 (&d)[NT][CX]) {
#pragma unroll
    for (int kb = 0; kb < NT; ++kb)
#pragma unroll
      for (int j = 0; j < CX; ++j)
        d[kb][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, lane * 16 + (c * CX + j) * 1024, kb * NX * 1024, 0));
  };
  wload(0, w[0]);                                                    // in flight under the projection's stores
  f32x4 hq[NT][1];
  const size_t orow = lin * (size_t)p.N;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = nt * 16 + 4 * kq;
    hq[nt][0] = yl_clamp4(acc[nt] + yl_ld4(p.bias + n), lo, hi);
    yl_out4(p, orow + n, hq[nt][0]);
  }
  const float lo3 = yl_act_lo(p.act3), hi3 = yl_act_hi(p.act3);
  const int ob = (int)lin * (NX * 64) + kq * 16;                    // byte offset of the lane's first expanded quad
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c + 1 < NC) wload(c + 1, w[(c + 1) & 1]);
    f32x4 a[1][CX];
#pragma unroll
    for (int j = 0; j < CX; ++j) a[0][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < NT; ++kb) yl_mma_step<CX, 1>(w[c & 1][kb], hq[kb], a);
#pragma unroll
    for (int j = 0; j < CX; ++j) {
      const f32x4 v = yl_clamp4(a[0][j] + yl_ld4(p.b3 + (c * CX + j) * 16 + 4 * kq), lo3, hi3);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), ors,
                                             ob + (c * CX + j) * 64, 0, 0);
    }
  }
#else
  (void)p; (void)acc; (void)lin; (void)kq; (void)lane; (void)lo; (void)hi; (void)out3;
#endif
}

// ------------------------------------------------------------------------------------------------
// Wave-autonomous depthwise -> 1x1 convolution: the depthwise counterpart of yl_conv_pwt_kernel and the successor of
// yl_conv_dwh_kernel (same per-wave algorithm: 4x4-pixel m-tiles, per 16-channel block the halo patch goes through
// the wave's private LDS region, B = act(bias + sum_taps w*x), NT x 4 MFMAs per m-tile; same k order and epilogues:
// bit-identical).  Persistent workgroups of four waves, one barrier (prologue), tiles dealt in XCD bands.  Two knobs:
//   WL   where the 1x1 A fragments come from.  false: straight from L1/L2 (requested before the taps of the block
//        they belong to) -- ~15 KB of LDS per workgroup, so K >= 192 layers keep 3-4 waves per SIMD where the LDS
//        weight image allowed one workgroup per CU (50 -> 36 us);  true: an LDS image filled once per workgroup,
//        the better choice when it is small (K = N = 96: 36 KB).
//   MT   m-tiles per wave: 2 = a 4x8-pixel tile, both m-tiles share the 6x10 / 8x12 halo patch, every A fragment
//        and every tap-weight read (LDS reads per pixel -35 %).
//   SK   split-K for grids of <= 20 x 20 pixels (round 4): such a layer has 25 tiles per image -- 800 wave tiles for a
//        32-image chunk on 1024 SIMDs, one wave walking 12-18 k-blocks serially while most of the chip idles (the 20x20
//        stage of edge_n: 4x off its byte / MFMA floor, and its launches cost their full duration in the two-stream step:
//        profiles/r04_skip_layers_edge_n_b64.txt).  SK = 4: the four waves of a workgroup share ONE tile, wave w takes the
//        k-blocks w, w + 4, ... (its own halo staging, no barrier in the loop); the partial accumulators meet in LDS (one
//        barrier per tile, buffers alternate) and wave w finishes n-tile w (+4): partials added in wave order 0..3, then
//        the usual epilogue.  Chosen by the LAYER SHAPE only (never by the batch): results stay batch-invariant and
//        bitwise repeatable, but are another fp32 summation order of the same products than SK = 1 / yl_conv_dwh_kernel.
//   NX   (yl_conv_dwx_kernel, fp32 unit only) n-tiles of the NEXT layer's plain 1x1, chained behind the epilogue: see there.
// halo patch of a 4 x 4 MT-pixel tile: rows, columns, row pitch in floats (see yl_conv_dwh_kernel)
constexpr __host__ __device__ int yl_dwt_hpy(int dk, int ds) { return 3 * ds + dk; }
constexpr __host__ __device__ int yl_dwt_hpx(int dk, int ds, int mt) { return (4 * mt - 1) * ds + dk; }
constexpr __host__ __device__ int yl_dwt_pitch(int dk, int ds, int mt) { return ((yl_dwt_hpx(dk, ds, mt) * 16 + 7) / 64) * 64 + 56; }
// dynamic LDS of yl_dwt_body (yl_conv_dwt_kernel, yl_conv_dwx_kernel), its regions in order and their floats: WL: [KB][NTtot][64]
// float4 1x1 weights | [DK*DK][Cin] taps, [Cin] bias | one halo patch per wave | SK > 1: [2][4][NT][64] float4 partial accumulators
// (region sizes, not offsets: see YlDwcLds)
struct YlDwtLds {
  static constexpr size_t LIMIT = 96 * 1024;
  int dk, ds, mt, sk, nt, KB, Cin;
  int NTl;                                                           // n-tiles of the weight image in LDS: NTtot (WL) or 0
  constexpr __host__ __device__ size_t weights() const { return (size_t)(KB * NTl) * 256; }
  constexpr __host__ __device__ size_t taps() const { return yl_taps_floats(dk, Cin); }
  constexpr __host__ __device__ int halos() const { return 4 * (yl_dwt_hpy(dk, ds) * yl_dwt_pitch(dk, ds, mt)); }
  constexpr __host__ __device__ size_t partials() const { return sk > 1 ? (size_t)2 * 4 * nt * 256 : 0; }
  constexpr __host__ __device__ size_t bytes() const { return (weights() + taps() + halos() + partials()) * 4; }
};

template <int NT, int DK, int DS, int MT, bool WL, int SK, int NX>
__device__ __forceinline__ void yl_dwt_body(const YlConvMulti& mp, yl_act_t* const out3) {
  YL_SELECT_PROBLEM_C(mp)
  constexpr int HPY = yl_dwt_hpy(DK, DS), HPX = yl_dwt_hpx(DK, DS, MT), PITCHF = yl_dwt_pitch(DK, DS, MT);
  constexpr int HF4 = HPY * HPX * 4;
  constexpr int NSLOT = (HF4 + 63) / 64;
  extern __shared__ __attribute__((aligned(16))) float yl_clds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, pl = lane & 15;
  const int Cin = p.Cin, H = p.H, W = p.W, OH = p.OH, OW = p.OW, N = p.N, NTtot = p.NTtot, KB = p.KB;
  const yl_act_t* const xin = p.x;
  // staging loads through a raw buffer descriptor (round 6, see yl_conv_dws_kernel): 32-bit byte offset per slot + scalar k-block
  // offset, zeros outside the image from the hardware range check.  The channel tail of the last k-block stages the next
  // pixel's channels (the tap weights are clamped to the last channels); its depthwise results are replaced by zeros before
  // the 1x1 (see the k-loop), so nothing past the pixel reaches the output
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<yl_act_t*>(p.x), 0, (int)((long)p.B * H * W * Cin * (long)sizeof(yl_act_t)), 0x00020000);
  constexpr unsigned OOB = 0x80000000u;
  const YlDwtLds L = {DK, DS, MT, SK, NT, KB, Cin, WL ? NTtot : 0};
  f32x4* wl = reinterpret_cast<f32x4*>(yl_clds);
  float* dwl = yl_clds + L.weights();
  float* halo = dwl + L.taps() + wave * (HPY * PITCHF);
  f32x4* red = reinterpret_cast<f32x4*>(dwl + L.taps() + L.halos());
  const f32x4* wg = reinterpret_cast<const f32x4*>(p.wp);
  const int twn = OW / (4 * MT), thn = OH >> 2;
  const int tiles_img = twn * thn;
  const int ntiles = p.B * tiles_img;
  // tile order: workgroup b runs on XCD b % 8; each XCD takes one contiguous band of tiles (halo rows of neighbouring
  // tiles then meet in the same L2), its workgroups' waves interleave inside the band
  int tile, tend, wstride;
  constexpr int WPT = SK > 1 ? 1 : 4;                                // tiles a workgroup works on at a time
  if ((gx & 7) == 0) {
    // yl_band_split's bands, written out: its slots are dealt WPT tiles and a wave at a time here, not item by item, next to
    // a branch for grids without bands -- through the helper the kernels came out with another control flow
    const int tpx = (ntiles + 7) >> 3;
    const int band0 = (bx & 7) * tpx;
    tend = (band0 + tpx) < ntiles ? (band0 + tpx) : ntiles;
    tile = band0 + (bx >> 3) * WPT + (SK > 1 ? 0 : wave);
    wstride = (gx >> 3) * WPT;
  } else {
    tile = bx * WPT + (SK > 1 ? 0 : wave); tend = ntiles; wstride = gx * WPT;
  }
  const int kb0 = SK > 1 ? wave : 0;                                 // SK: this wave's k-blocks kb0, kb0 + SK, ...
  unsigned sk_par = 0;
  // staging slots of this lane: halo pixel / channel quad -> LDS offset; global offsets per tile
  int s_lo[NSLOT];
  bool s_ok[NSLOT];
#pragma unroll
  for (int j = 0; j < NSLOT; ++j) {
    const int e = j * 64 + lane;
    s_ok[j] = e < HF4;
    const int hp = (s_ok[j] ? e : 0) >> 2, quad = e & 3;
    const int hr = hp / HPX, hc = hp - hr * HPX;
    s_lo[j] = hr * PITCHF + hc * 16 + quad * 4;
  }
  // (image, tile row, tile column) of the wave's current tile, advanced by the decomposition of wstride with two
  // carries: no integer division per tile (each one is ~25 VALU instructions, and fp32 VALU time is MFMA time)
  int tb = 0, tyi = 0, txi = 0;
  if (tile < tend) {
    tb = tile / tiles_img;
    const int trem = tile - tb * tiles_img;
    tyi = trem / twn; txi = trem - tyi * twn;
  }
  const int sdb = wstride / tiles_img, sdrem = wstride - sdb * tiles_img;
  const int sdy = sdrem / twn, sdx = sdrem - sdy * twn;
  unsigned goff[NSLOT];
  auto tile_geom = [&]() {
    const int b = tb;
    const int iy0 = 4 * tyi * DS - p.dw_pad_t, ix0 = 4 * MT * txi * DS - p.dw_pad_l;
#pragma unroll
    for (int j = 0; j < NSLOT; ++j) {
      const int e = j * 64 + lane;
      const int hp = (e < HF4 ? e : 0) >> 2;
      const int hr = hp / HPX, hc = hp - hr * HPX;
      const int iy = iy0 + hr, ix = ix0 + hc;
      const bool in = e < HF4 && iy >= 0 && iy < H && ix >= 0 && ix < W;
      goff[j] = in ? (unsigned)((((b * H + iy) * W + ix) * Cin + (lane & 3) * 4) * (int)sizeof(yl_act_t)) : OOB;
    }
  };
  auto stage_load = [&](int kb, f32x4 (&r)[NSLOT]) {
#pragma unroll
    for (int j = 0; j < NSLOT; ++j) {
#if YL_F16S
      r[j] = __builtin_convertvector(__builtin_bit_cast(yl_h16x4, __builtin_amdgcn_raw_buffer_load_b64(xrs, (int)goff[j], kb * 32, 0)), f32x4);
#else
      r[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, (int)goff[j], kb * 64, 0));
#endif
    }
  };
  auto stage_store = [&](const f32x4 (&r)[NSLOT]) {
#pragma unroll
    for (int j = 0; j < NSLOT; ++j)
      if (s_ok[j]) *reinterpret_cast<f32x4*>(halo + s_lo[j]) = r[j];
  };
  f32x4 stg[NSLOT];
  bool primed = false;
  if (tile < tend) {                       // first tile's first halo block: in flight together with the LDS fills
    tile_geom();
    stage_load(kb0, stg);
    primed = true;
  }
  if (WL) {
    for (int i = wave; i < KB * NTtot; i += 4) yl_glds16(wg + (size_t)i * 64 + lane, wl + (size_t)i * 64);
  }
  {
    const int nw = DK * DK * Cin;
    yl_glds_floats(p.dw_w, dwl, nw, tid, 256);
    if (p.dw_b) yl_glds_floats(p.dw_b, dwl + nw, Cin, tid, 256);
    else for (int i = tid; i < Cin; i += 256) dwl[nw + i] = 0.0f;
  }
  __syncthreads();                                                   // the only workgroup barrier
  const float lo = yl_act_lo(p.act), hi = yl_act_hi(p.act);
  const float dlo = yl_act_lo(p.dw_act), dhi = yl_act_hi(p.dw_act);
  const int dw_act = p.dw_act;
  const bool pre_add = p.res != nullptr && p.up == nullptr && p.act == YL_ACT_NONE;
  const int rbase = ((pl >> 2) * DS) * PITCHF + ((pl & 3) * DS) * 16 + 4 * kq;
  for (; tile < tend; tile += wstride) {
    const int b = tb;
    YlPix px[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      px[mt].b = b;
      px[mt].oy = 4 * tyi + (pl >> 2);
      px[mt].ox = 4 * MT * txi + 4 * mt + (pl & 3);
      px[mt].valid = true;
      px[mt].lin = ((size_t)b * OH + px[mt].oy) * OW + px[mt].ox;
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = nt * 16 + 4 * kq;
        acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (pre_add && n < N && (SK == 1 || wave == 0)) acc[mt][nt] = yl_ld4(p.res + px[mt].lin * N + n);
      }
    if (!primed) {
      tile_geom();
      stage_load(kb0, stg);
    }
    primed = false;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");          // previous tile's tap reads are complete
    stage_store(stg);
    // (Requesting the NEXT tile's first halo block under the last block of this one -- the pipelining that pays in
    // yl_conv_dpp_kernel -- was measured here: 37.54k vs 37.79k images/s on the headline step, slower.  So was chaining
    // the next block's plain 1x1 `pw_exp` behind this kernel's epilogue with both outputs written, for the five
    // `pw_proj` -> `pw_exp` pairs of edge_n's 20x20 stage: one-stream launch times at B = 64, 45.4 us chained against
    // 29.4 + 20.2 for the 5x5 pairs, 53.6 against 23.7 + 20.2 for the 3x3 pairs (one of them feeds 64 -> 480); headline
    // unchanged at 38.8k with five launches fewer per chunk -- not kept then.  Round 7: yl_conv_dwx_kernel, the four 64 -> 192 / 256
    // pairs only, the expansion's A fragments through a buffer descriptor with the next chunk in flight: 0.85x of the two launches.)
    for (int kb = kb0; kb < KB; kb += SK) {
      const bool more = kb + SK < KB;
      if (more) stage_load(kb + SK, stg);
      f32x4 wq[NT];
      if (!WL) {                                                     // A fragments from L1/L2: in flight under the taps
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wq[nt] = wg[((size_t)kb * NTtot + (nt < NTtot ? nt : NTtot - 1)) * 64 + lane];
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");        // halo writes (all lanes) -> tap reads
      const int c = kb * 16 + 4 * kq;
      const int cs = c < Cin ? c : Cin - 4;
      const float* tapw = dwl + cs;
      f32x4 xq[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) xq[mt] = yl_ld4(tapw + DK * DK * Cin);
      if (DK == 3) {
#pragma unroll
        for (int dy = 0; dy < DK; ++dy) {
#pragma unroll
          for (int dx = 0; dx < DK; ++dx) {
            const f32x4 w = yl_ld4(tapw + (dy * DK + dx) * Cin);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              const f32x4 v = *reinterpret_cast<const f32x4*>(halo + rbase + dy * PITCHF + (dx + 4 * mt * DS) * 16);
              xq[mt].x = fmaf(v.x, w.x, xq[mt].x); xq[mt].y = fmaf(v.y, w.y, xq[mt].y);
              xq[mt].z = fmaf(v.z, w.z, xq[mt].z); xq[mt].w = fmaf(v.w, w.w, xq[mt].w);
            }
          }
          if (MT > 1) __builtin_amdgcn_sched_barrier(0);             // one tap row in flight: bounds the live LDS reads
        }
      } else {
#pragma unroll 1
        for (int dy = 0; dy < DK; ++dy) {                            // one tap row at a time bounds the register footprint
#pragma unroll
          for (int dx = 0; dx < DK; ++dx) {
            const f32x4 w = yl_ld4(tapw + (dy * DK + dx) * Cin);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              const f32x4 v = *reinterpret_cast<const f32x4*>(halo + rbase + dy * PITCHF + (dx + 4 * mt * DS) * 16);
              xq[mt].x = fmaf(v.x, w.x, xq[mt].x); xq[mt].y = fmaf(v.y, w.y, xq[mt].y);
              xq[mt].z = fmaf(v.z, w.z, xq[mt].z); xq[mt].w = fmaf(v.w, w.w, xq[mt].w);
            }
          }
        }
      }
      // channel tail (c >= Cin): the staged halo holds the next pixel's channels there -- zeros into the MFMA (0 x inf / NaN
      // would be NaN against the zero 1x1 weights of those k slots)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) xq[mt] = yl_sel4(c < Cin, yl_actc(xq[mt], dw_act, dlo, dhi));
      if (WL) {
        const f32x4* wrow = wl + (size_t)kb * NTtot * 64 + lane;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wq[nt] = wrow[(nt < NTtot ? nt : NTtot - 1) * 64];
      }
      yl_mma_step<NT, MT>(wq, xq, acc);
      if (more) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // this block's tap reads are complete
        stage_store(stg);
      }
    }
    if (SK > 1) {
      // partial accumulators -> LDS (buffer = tile parity), ONE barrier per tile, wave w finishes the n-tiles w, w + SK
      f32x4* rb = red + (size_t)(sk_par & 1u) * (4 * NT * 64);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) rb[(wave * NT + nt) * 64 + lane] = acc[0][nt];
      __syncthreads();
      ++sk_par;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        if ((nt & (SK - 1)) != wave) continue;                       // wave-uniform
        f32x4 one[1][1];
        one[0][0] = ((rb[(0 * NT + nt) * 64 + lane] + rb[(1 * NT + nt) * 64 + lane]) + rb[(2 * NT + nt) * 64 + lane]) +
                    rb[(3 * NT + nt) * 64 + lane];
        const YlPix px1[1] = {px[0]};
        if (!pre_add && (p.res || p.up || YL_SMOOTH(p.act))) yl_epi_generic<1, 1>(p, one, px1, nt, kq);
        else yl_epi_fast<1, 1>(p, one, px1, nt, kq, lo, hi, true);
      }
    } else if constexpr (NX > 0) {
      yl_dwx_tail<NT, NX>(p, acc[0], px[0].lin, kq, lane, lo, hi, out3);
    } else {
      if (!pre_add && (p.res || p.up || YL_SMOOTH(p.act))) yl_epi_generic<NT, MT>(p, acc, px, 0, kq);
      else yl_epi_fast<NT, MT>(p, acc, px, 0, kq, lo, hi, true);
    }
    txi += sdx;
    if (txi >= twn) { txi -= twn; ++tyi; }
    tyi += sdy;
    if (tyi >= thn) { tyi -= thn; ++tb; }
    tb += sdb;
  }
}

template <int NT, int DK, int DS, int MT, bool WL, int SK = 1>
__global__ __launch_bounds__(256, MT == 2 ? 2 : 3) void yl_conv_dwt_kernel(YlConvMulti mp) {
  yl_dwt_body<NT, DK, DS, MT, WL, SK, 0>(mp, nullptr);
}

// The instantiations of yl_conv_dwt_kernel<NT, DK, DS, MT, WL, SK>, written once (yl_convc_init and the launcher read these
// tables).  One m-tile per wave (MT = 1: the 4x8-pixel tile of MT = 2 was measured slower, see yl_launch_conv_dwt); NT in
// {1, 2, 3, 4, 6} x depthwise 3x3 / 5x5 x stride 1 / 2 x 1x1 weights from L1/L2 or from an LDS image (WL), as
// [NT <= 4 ? NT - 1 : 4][DK == 5][DS == 2][WL]
#define YL_DWT_WLS(NT, DK, DS) {yl_conv_dwt_kernel<NT, DK, DS, 1, false>, yl_conv_dwt_kernel<NT, DK, DS, 1, true>}
#define YL_DWT_SHAPES(NT) {{YL_DWT_WLS(NT, 3, 1), YL_DWT_WLS(NT, 3, 2)}, {YL_DWT_WLS(NT, 5, 1), YL_DWT_WLS(NT, 5, 2)}}
static const YlMultiKernel dwt_kernels[5][2][2][2] = {YL_DWT_SHAPES(1), YL_DWT_SHAPES(2), YL_DWT_SHAPES(3), YL_DWT_SHAPES(4),
                                                      YL_DWT_SHAPES(6)};
// split-K form (see the kernel: NT = 4, one n-tile per wave, SK = 4, weights from L1/L2): stride-1 3x3 / 5x5 and stride-2
// 3x3 depthwise, as [DK == 5][DS == 2]
static const YlMultiKernel dwt_splitk_kernels[2][2] = {
    {yl_conv_dwt_kernel<4, 3, 1, 1, false, 4>, yl_conv_dwt_kernel<4, 3, 2, 1, false, 4>},
    {yl_conv_dwt_kernel<4, 5, 1, 1, false, 4>, nullptr}};

// dynamic LDS of yl_conv_dwt_kernel<NT, p.dw_k, p.dw_stride, 1, WL, SK> on the layer p
static size_t dwt_lds(const YlConvP& p, int NT, bool WL, int SK) {
  return YlDwtLds{p.dw_k, p.dw_stride, 1, SK, NT, p.KB, p.Cin, WL ? p.NTtot : 0}.bytes();
}

// NT, WL, SK: the template arguments of `kern` (DK and DS are the layer's); yl_dwt_form has held its LDS to the limit
static hipError_t dwt_go(YlConvMulti& m, hipStream_t st, YlMultiKernel kern, int NT, bool WL, int SK) {
  constexpr int MT = 1;
  const YlConvP& p = m.p[0];
  const size_t lds = dwt_lds(p, NT, WL, SK);
  const int res = yl_resident_blocks((const void*)kern, 256, lds, 8);
  long tiles[4];
  for (int k = 0; k < m.n; ++k)
    tiles[k] = (long)m.p[k].B * (m.p[k].OH >> 2) * (m.p[k].OW / (4 * MT)) * (SK > 1 ? 4 : 1);     // SK: a workgroup per tile
  // persistent workgroups: at most one wave per tile (four per workgroup)
  const int at = yl_multi_shares(m, tiles, res, 4);
  hipLaunchKernelGGL(kern, dim3((unsigned)at), dim3(256), lds, st, m);
  return hipGetLastError();
}

// depthwise (3x3 / 5x5, stride 1 / 2) -> 1x1 with N % 4 == 0, N <= 96 (all n-tiles in one wave), OH % 4 == 0,
// OW % 4 == 0.  Family 0 otherwise (yl_conv_dwh_kernel then runs the layer).
YlDwForm yl_dwt_form(const YlConvMulti& m) {
  const YlDwForm none = {YL_DWF_NONE, {0, 0, 0, 0, 0, 0}};
  const YlConvP& p = m.p[0];
  if (p.dw_k == 0 || (p.N & 3) || p.NTtot > 6 || p.dec_boxes || p.C1 > 0) return none;
  if ((p.dw_k != 3 && p.dw_k != 5) || (p.dw_stride != 1 && p.dw_stride != 2)) return none;
  // Per-layer measurements (edge_n, B = 64, us; dwh = yl_conv_dwh_kernel, <mt><wl> = this kernel):
  //   K=N=96 dw3 80x80:  dwh 143 | 10: 163 | 11: 137 | 20: 147 | 21: 141        K=96 N=48 dw3: dwh 32.9 | 11: 29.2
  //   K=256 N=64 dw5:    dwh 49.7 | 10: 35.1 | 11: 49.3 | 20: 34.9             K=32 N=96 dw5 s2: dwh 76 | 11: 70
  // -> one m-tile per wave (the 4x8 tile needs ~190 VGPRs: 2 waves per SIMD), LDS weight image while it is <= 36 KB.
  // ("dev_select" bit 4 disables the kernel: developer A/B)
  if (p.dev & YL_DEV_DWT_OFF) return none;
  const bool wl = p.KB * p.NTtot <= 36;
  for (int k = 0; k < m.n; ++k) {
    if ((m.p[k].OH & 3) || (m.p[k].OW & 3)) return none;
    if ((size_t)m.p[k].B * m.p[k].H * m.p[k].W * m.p[k].Cin * sizeof(yl_act_t) >= ((size_t)1 << 31)) return none;   // 32-bit byte offsets
  }
  const int nts[5] = {1, 2, 3, 4, 6};
  int NT = 6;
  for (int i = 0; i < 5; ++i) if (nts[i] >= p.NTtot) { NT = nts[i]; break; }
  const int dk5 = p.dw_k == 5, ds2 = p.dw_stride == 2;
  // split-K: chosen by the layer's SHAPE only (batch-invariant results); "dev_select" bit 10 keeps the one-wave-per-tile form
  if (m.n == 1 && NT == 4 && !wl && p.KB >= 8 && p.OH * p.OW <= 400 && !(p.dev & YL_DEV_DWT_NOSPLIT) && dwt_splitk_kernels[dk5][ds2] &&
      dwt_lds(p, 4, false, 4) <= YlDwtLds::LIMIT)
    return {YL_DWF_DWT_SPLITK, {4, p.dw_k, p.dw_stride, 1, 0, 4}};
  if (dwt_lds(p, NT, wl, 1) > YlDwtLds::LIMIT) return none;
  return {YL_DWF_DWT, {NT, p.dw_k, p.dw_stride, 1, wl, 1}};
}

hipError_t yl_launch_conv_dwt(YlConvMulti& m, const YlDwForm& f, hipStream_t st) {
  const int NT = f.a[0], dk5 = f.a[1] == 5, ds2 = f.a[2] == 2;
  if (f.family == YL_DWF_DWT_SPLITK) return dwt_go(m, st, dwt_splitk_kernels[dk5][ds2], 4, false, 4);
  if (f.family == YL_DWF_DWT) return dwt_go(m, st, dwt_kernels[NT <= 4 ? NT - 1 : 4][dk5][ds2][f.a[4]], NT, f.a[4] != 0, 1);
  return hipErrorNotSupported;
}

#if !YL_BF16
// ------------------------------------------------------------------------------------------------
// UIB projection (depthwise DK x DK stride 1 -> 1x1 -> 64 channels, + residual) with the NEXT block's expansion (plain 1x1
// 64 -> 16 NX, + ReLU) chained behind it in the same launch: edge_n's 20x20 stage, blocks.3.1-3.4 pw_proj + blocks.3.2-3.5
// pw_exp.  Two launches before (yl_conv_dwt_kernel<4, DK, 1, 1, false, 1> + yl_conv_pwt_kernel<4, 1>), each bound by
// latency and launch count, not by MFMA work or HBM.  The projection runs as in yl_conv_dwt_kernel (same
// body: one 4x4 tile per wave, halo through LDS, 1x1 A fragments from L1/L2) and stores its 64-channel output as before --
// the next block reads it as its residual; the accumulators of its epilogue are the B fragments of the expansion, which
// then runs from registers (yl_dwx_tail): no LDS transpose, no halo, no pixel computed twice.  Bit-identical to the two
// launches.  Only the shapes edge_n needs: Cin 192 / 256, N = 64, DK 3 / 5, NX = 12 / 16.
template <int DK, int NX>
__global__ __launch_bounds__(256, 3) void yl_conv_dwx_kernel(YlConvMulti mp, float* out3) {
  yl_dwt_body<4, DK, 1, 1, false, 1, NX>(mp, out3);
}

// instantiated: (depthwise k, n-tiles of the chained 1x1)
#define YL_DWX_SHAPES(X) X(5, 16) X(5, 12) X(3, 16) X(3, 12)
typedef void (*YlDwxKernel)(YlConvMulti, float*);
static YlDwxKernel dwx_kernel_of(int dk, int nx) {
#define YL_DWX_PICK(DK, NX) if (dk == DK && nx == NX) return yl_conv_dwx_kernel<DK, NX>;
  YL_DWX_SHAPES(YL_DWX_PICK)
#undef YL_DWX_PICK
  return nullptr;
}

static hipError_t dwx_go(YlConvMulti& m, float* out3, hipStream_t st, YlDwxKernel kern) {
  const YlConvP& p = m.p[0];
  const size_t lds = YlDwtLds{p.dw_k, 1, 1, 1, 4, p.KB, p.Cin, 0}.bytes();   // the body's <4, DK, 1, 1, false, 1>
  const int res = yl_resident_blocks((const void*)kern, 256, lds, 8);
  // persistent workgroups as dwt_go: a multiple of 8 (XCD bands), at most one wave per tile
  const long tiles = (long)p.B * (p.OH >> 2) * (p.OW >> 2);
  const int g = yl_multi_shares(m, &tiles, res, 4);
  hipLaunchKernelGGL(kern, dim3((unsigned)g), dim3(256), lds, st, m, out3);
  return hipGetLastError();
}

bool yl_dwx_supported(int cin, int cout, int dw_k, int dw_stride, int cout1, int oh, int ow) {
  return (cin == 192 || cin == 256) && cout == 64 && dw_stride == 1 && (cout1 & 15) == 0 && dwx_kernel_of(dw_k, cout1 / 16) &&
         (oh & 3) == 0 && (ow & 3) == 0;
}

// pd: the depthwise -> 1x1 projection layer with w3p / b3 / C3 / act3 of the plain 1x1 behind it, whose output is out3.
// hipErrorNotSupported for every other shape or configuration (the two launches then run).
hipError_t yl_launch_conv_dwx(const YlConvP& pd, float* out3, hipStream_t st) {
  const YlConvP& p = pd;
  if (p.k != 1 || p.stride != 1 || p.C1 > 0 || p.up || p.scale || p.dec_boxes || p.ldo || p.in_shift || !p.w3p || !out3 ||
      YL_SMOOTH(p.act) || YL_SMOOTH(p.act3) || (p.res && p.act != YL_ACT_NONE) || p.H != p.OH || p.W != p.OW ||
      !yl_dwx_supported(p.Cin, p.N, p.dw_k, p.dw_stride, p.C3, p.OH, p.OW))
    return hipErrorNotSupported;
  // the two-launch form these replace: yl_conv_dwt_kernel, one wave per tile (split-K off), A fragments from L1/L2
  if ((p.dev & (YL_DEV_DWT_OFF | YL_DEV_CHAIN_OFF)) || !(p.dev & YL_DEV_DWT_NOSPLIT) || p.KB * p.NTtot <= 36) return hipErrorNotSupported;
  if ((size_t)p.B * p.H * p.W * p.Cin * sizeof(float) >= ((size_t)1 << 31) ||
      (size_t)p.B * p.OH * p.OW * p.C3 * sizeof(float) >= ((size_t)1 << 31))
    return hipErrorNotSupported;                                     // 32-bit byte offsets
  YlConvMulti m = {};
  m.n = 1;
  m.p[0] = p;
  return dwx_go(m, out3, st, dwx_kernel_of(p.dw_k, p.C3 / 16));      // (instantiated: yl_dwx_supported above)
}

// ------------------------------------------------------------------------------------------------
// Two plain 1x1 convolutions as ONE launch, the tensor between them never written: L1 takes Cin <= 16 KB1 channels to Cmid
// (= 16 NTm, + bias, clamp), L2 takes Cmid to N <= 16 NT2 (+ bias, clamp or nothing).  edge_n's backbone tail: blocks.4.0.conv
// 64 -> 480 at 20x20 and lateral5 480 -> 96, the only reader of C5 -- 49 MB written and read again at B = 64 by two launches
// that are bound by latency, not by MFMA work.  The MFMA D layout of L1's mid n-tile c (lane (kq, pl): channels
// 16 c + 4 kq .. + 3 of pixel pl) is the B fragment of L2's k-block c, so per wave item of MT m-tiles: the KB1 B fragments of x
// are loaded once; for every mid n-tile c ascending: a = 0, k-blocks ascending into a, h = clamp(a + b1[c]), then the NT2 n-tiles
// of L2 take h as k-block c.  These are the k orders and epilogues of the two stand-alone launches (yl_conv_pws_kernel /
// yl_conv_pwt_kernel: channel blocks ascending, four k-steps each, bias added after the products): bit-identical results.  Cmid is
// never split between waves (that would be another fp32 summation order for L2).
// Weights: KB1 + NT2 pieces of 1 KiB per mid n-tile (W1[.][c] and W2[c][.]), the same stream for every item, double-buffered through
// LDS in chunks of CP mid n-tiles shared by the workgroup's NW waves -- the asynchronous copies of chunk c + 1 issued before the
// MFMAs of chunk c, ONE barrier per chunk, the pipeline running on across items (the recipe of yl_conv_pws_kernel).  L1's bias
// sits in LDS for the whole launch (an ordinary load inside the chunk loop would wait for the copies in flight).
// dynamic LDS of yl_conv_pwx_kernel, regions in order (floats): [2][CP][KB1 + NT2][64] float4 weight chunks | [Cmid] bias of L1
struct YlPwxLds {
  static constexpr size_t LIMIT = 64 * 1024;
  static constexpr int CP = 2;                               // mid n-tiles per weight chunk
  int KB1, NT2, Cmid;
  constexpr __host__ __device__ size_t weights() const { return (size_t)2 * CP * (KB1 + NT2) * 256; }
  constexpr __host__ __device__ size_t bytes() const { return (weights() + (size_t)Cmid) * 4; }
};

template <int KB1, int NT2, int NW, int MT>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 3 : 4) void yl_conv_pwx_kernel(YlConvP p) {
  constexpr int CP = YlPwxLds::CP, PC = KB1 + NT2;           // pieces of 1 KiB per mid n-tile
  extern __shared__ __attribute__((aligned(16))) float yl_clds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, pl = lane & 15;
  const int NTm = p.NTtot, Cin = p.Cin, M = p.M;
  const YlPwxLds L = {KB1, NT2, NTm * 16};
  const yl_act_t* const xin = p.x;
  f32x4* wl = reinterpret_cast<f32x4*>(yl_clds);             // [2][CP][PC][64] float4
  const float* b1l = yl_clds + L.weights();
  const f32x4* w1g = reinterpret_cast<const f32x4*>(p.wp);   // [KB1][NTm][64] float4
  const f32x4* w2g = reinterpret_cast<const f32x4*>(p.w3p);  // [NTm][NT2][64] float4
  const int NC = (NTm + CP - 1) / CP;                         // chunks per item
  // XCD x (workgroup b -> XCD b % 8) owns a contiguous band of the workgroup tiles (NW * MT m-tiles each), strided over its workgroups
  const YlBandSplit ws = yl_band_split((int)blockIdx.x, (int)gridDim.x, p.ntiles);   // gridDim.x % 8 == 0
  const int per = ws.per, slot = ws.slot, band0 = ws.band0, nmine = ws.nmine;
  const long total_chunks = (long)nmine * NC;
  // asynchronous copy of chunk `c` (mid n-tiles c*CP .. c*CP+CP-1, clamped) into buffer `buf`
  auto load_chunk = [&](int c, int buf) {
    for (int i = wave; i < CP * PC; i += NW) {
      const int j = i / PC, q = i - j * PC;
      int ct = c * CP + j;
      ct = ct < NTm ? ct : NTm - 1;
      const f32x4* src = q < KB1 ? w1g + ((size_t)q * NTm + ct) * 64 : w2g + ((size_t)ct * NT2 + (q - KB1)) * 64;   // (wave-uniform)
      yl_glds16(src + lane, wl + ((size_t)buf * CP * PC + i) * 64);
    }
  };
  if (total_chunks > 0) load_chunk(0, 0);
  yl_glds_floats(p.bias, yl_clds + L.weights(), NTm * 16, tid, NW * 64);
  long gchunk = 0;                                            // chunks consumed so far (buffer = gchunk & 1)
  __syncthreads();
  const float lo1 = yl_act_lo(p.act), hi1 = yl_act_hi(p.act);
  const float lo2 = yl_act_lo(p.act3), hi2 = yl_act_hi(p.act3);
  const int N2 = p.C3;
  yl_act_t* const outp = p.out;                               // L2's output
  f32x4 b2r[NT2];                                             // L2's bias (padded to whole n-tiles): read once, not per item
#pragma unroll
  for (int nt = 0; nt < NT2; ++nt) b2r[nt] = yl_ld4(p.b3 + nt * 16 + 4 * kq);

  for (int wi = 0; wi < nmine; ++wi) {
    const int tile = band0 + slot + wi * per;
    bool valid[MT];
    size_t pix[MT];                                           // linear pixel index (clamped)
    f32x4 xq[KB1][MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      // the last m-tiles may be partial or empty: their lanes read the last pixel and store nothing
      size_t lin = (((size_t)tile * NW + wave) * MT + mt) * 16 + pl;
      valid[mt] = lin < (size_t)M;
      if (!valid[mt]) lin = (size_t)M - 1;
      pix[mt] = lin;
      const yl_act_t* xrow = xin + lin * Cin + 4 * kq;
#pragma unroll
      for (int kb = 0; kb < KB1; ++kb)
        xq[kb][mt] = yl_ld4(kb * 16 + 4 * kq < Cin ? xrow + kb * 16 : p.zeros);   // channel tail of the last block: zeros
    }
    f32x4 acc[MT][NT2];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT2; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < NC; ++c) {
      const int buf = (int)(gchunk & 1);
      // next chunk of the stream (the same weights for every item) into the other buffer
      if (gchunk + 1 < total_chunks) load_chunk(c + 1 < NC ? c + 1 : 0, buf ^ 1);
      const f32x4* wb = wl + (size_t)buf * CP * PC * 64 + lane;
      f32x4 a[MT][CP];                                        // L1: CP mid n-tiles, independent accumulator chains
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < CP; ++j) a[mt][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < KB1; ++kb) {
        f32x4 wq[CP];
#pragma unroll
        for (int j = 0; j < CP; ++j) wq[j] = wb[(j * PC + kb) * 64];
        yl_mma_step<CP, MT>(wq, xq[kb], a);
      }
#pragma unroll
      for (int j = 0; j < CP; ++j) {
        const int ct = c * CP + j;
        if (ct < NTm) {                                       // (workgroup-uniform) odd NTm: the last chunk is half empty
          const f32x4 b1 = *reinterpret_cast<const f32x4*>(b1l + ct * 16 + 4 * kq);
          f32x4 h[MT], wq[NT2];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) h[mt] = yl_clamp4(a[mt][j] + b1, lo1, hi1);
#pragma unroll
          for (int nt = 0; nt < NT2; ++nt) wq[nt] = wb[(j * PC + KB1 + nt) * 64];
          yl_mma_step<NT2, MT>(wq, h, acc);
        }
      }
      __syncthreads();             // every wave is done with `buf`; the copies into the other buffer have landed
      ++gchunk;
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {                         // == yl_epi_fast with the bias from registers
      if (!valid[mt]) continue;
      yl_act_t* orow = outp + pix[mt] * N2;
#pragma unroll
      for (int nt = 0; nt < NT2; ++nt) {
        const int n = nt * 16 + 4 * kq;
        const f32x4 v = yl_clamp4(acc[mt][nt] + b2r[nt], lo2, hi2);
        if (n < N2) yl_st4(orow + n, v);
      }
    }
  }
}

// instantiated: (k-blocks of L1's input, n-tiles of L2's output, waves per workgroup, m-tiles per wave)
#define YL_PWX_SHAPES(X) X(4, 6, 4, 1)
static YlConvKernel pwx_kernel_of(int kb1, int nt2, int* nw, int* mt) {
#define YL_PWX_PICK(KB1, NT2, NW, MT) if (kb1 == KB1 && nt2 == NT2) { *nw = NW; *mt = MT; return yl_conv_pwx_kernel<KB1, NT2, NW, MT>; }
  YL_PWX_SHAPES(YL_PWX_PICK)
#undef YL_PWX_PICK
  return nullptr;
}

bool yl_pwx_supported(int cin, int cmid, int cout) {
  int nw, mt;
  return cin > 0 && (cin & 3) == 0 && cmid > 0 && (cmid & 15) == 0 && cout > 0 && (cout & 3) == 0 &&
         pwx_kernel_of((cin + 15) / 16, (cout + 15) / 16, &nw, &mt) &&
         YlPwxLds{(cin + 15) / 16, (cout + 15) / 16, cmid}.bytes() <= YlPwxLds::LIMIT;
}

// p1: the first plain 1x1 layer with w3p / b3 / C3 / act3 of the plain 1x1 behind it, whose output is out3; p1's own output is
// not written.  hipErrorNotSupported for every other shape or configuration (the two launches then run).
hipError_t yl_launch_conv_pwx(const YlConvP& p1, float* out3, hipStream_t st) {
  if (p1.k != 1 || p1.stride != 1 || p1.dw_k > 0 || p1.C1 > 0 || p1.res || p1.up || p1.scale || p1.dec_boxes || p1.ldo || p1.in_shift ||
      !p1.bias || !p1.w3p || !p1.b3 || !out3 || YL_SMOOTH(p1.act) || YL_SMOOTH(p1.act3) || p1.H != p1.OH || p1.W != p1.OW ||
      (p1.dev & YL_DEV_PWX_OFF) || !yl_pwx_supported(p1.Cin, p1.N, p1.C3))
    return hipErrorNotSupported;
  if ((size_t)p1.M * p1.Cin * sizeof(float) >= ((size_t)1 << 31) || (size_t)p1.M * p1.C3 * sizeof(float) >= ((size_t)1 << 31))
    return hipErrorNotSupported;                                     // byte offsets of the input and the output below 2^31
  int NW = 0, MT = 0;
  const YlConvKernel kern = pwx_kernel_of(p1.KB, (p1.C3 + 15) / 16, &NW, &MT);
  YlConvP p = p1;
  p.out = out3;
  p.ntiles = (int)(((long)p.M + 16 * NW * MT - 1) / (16 * NW * MT));
  const size_t lds = YlPwxLds{p.KB, (p.C3 + 15) / 16, p.N}.bytes();
  // Shape: 4 waves x 1 m-tile per wave (64 pixels per workgroup item; 94-118 VGPRs, 43 KB of LDS).  NOT MEASURED: the other
  // candidates (8 waves x 1, 4 waves x 2 m-tiles, A fragments straight from L1/L2 through a buffer descriptor) and the one-stream
  // launch time at B = 64 against the two launches (40.1 + 34.6 us, profiles/head_skip_kernel_stats_after.csv) have not been timed.
  const int gx = yl_band_grid(yl_resident_blocks((const void*)kern, NW * 64, lds, 8), p.ntiles);
  hipLaunchKernelGGL(kern, dim3(gx), dim3(NW * 64), lds, st, p);
  return hipGetLastError();
}
#endif

// ------------------------------------------------------------------------------------------------
// Dense k x k convolution whose weights do not fit LDS (yololite_m's FPN: 3x3, 328 -> 328 channels = 3.9 MB packed,
// 16.3 of the model's ~24 GMAC per image; model_v2.py:15-22,125-127) as an implicit GEMM with the weight stream
// DOUBLE-BUFFERED through LDS.  yl_conv_mfma_kernel streams the same weights in 48 KiB chunks between two
// workgroup barriers each (fill, then use): while a chunk is fetched the workgroup's four waves issue no MFMA,
// and with 21 n-tiles split 8 + 8 + 5 an eighth of the issued MFMAs multiplies zero padding -- 75 TFLOP/s = 0.48 of
// the fp32 MFMA peak.  Here: NT = 7 n-tiles per workgroup (21 = 3 x 7, no padding), chunks of CH k-steps in two LDS
// buffers, the asynchronous global->LDS copies of chunk c+1 issued before the MFMAs of chunk c (ONE barrier per
// chunk, which is also where the copies are waited for), the chunk pipeline running on across tile boundaries.
// Same transposed GEMM, k order and epilogues as yl_conv_mfma_kernel: bit-identical results.
// dynamic LDS of yl_conv_kxk_kernel: two buffers of one weight chunk = 3 taps x NT pieces of 1 KiB.  Layers whose whole weight
// image fits LIMIT are not this kernel's (yl_launch_conv_kxk)
struct YlKxkLds {
  static constexpr size_t LIMIT = 96 * 1024;
  static constexpr __host__ __device__ size_t bytes(int NT) { return (size_t)2 * 3 * NT * 1024; }   // [2][3][NT][64] float4 at 0
  static constexpr size_t image_bytes(int TK, int NT) { return (size_t)TK * NT * 1024; }   // the resident form (yl_conv_mfma_kernel)
};

template <int NT, int MT, int NW>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 3 : 4) void yl_conv_kxk_kernel(YlConvP p) {
  extern __shared__ __attribute__((aligned(16))) float yl_clds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, pl = lane & 15;
  const int TK = p.TK, KB = p.KB, K = p.k, NTtot = p.NTtot;
  const int Cin = p.Cin, H = p.H, W = p.W, stride = p.stride, pad_t = p.pad_t, pad_l = p.pad_l, sh = p.in_shift;
  const int ohw = p.OH * p.OW, OW = p.OW, M = p.M;
  const yl_act_t* const xin = p.x;
  const long zdelta = p.zeros - p.x;
  f32x4* wl = reinterpret_cast<f32x4*>(yl_clds);            // [2][3][NT][64] float4
  const f32x4* wg = reinterpret_cast<const f32x4*>(p.wp);
  const int NC = 3 * KB;                                     // chunks (3 taps each) per (m-tile, n-group) item
  const int G = NTtot / NT;                                  // n-groups of NT n-tiles (the launcher guarantees NTtot % NT == 0)
  // Work order.  A workgroup runs ALL its m-tiles for n-group 0, then for group 1, ...: at any time the workgroups
  // of an XCD stream the same 1/G of the weights (1.3 MB of yololite_m's 3.9 MB), which stays in that XCD's 4 MB L2;
  // with the groups spread over gridDim.y every XCD cycled through the whole image and FETCH_SIZE showed each pass
  // coming from HBM/MALL again (20x the algorithmic bytes).  The m-tiles of an XCD (workgroup b -> XCD b % 8) are
  // one contiguous band of the output, so the 3x3 halo rows of neighbouring tiles hit the same L2 as well.
  const int bx = blockIdx.x, gx = gridDim.x;                 // gx % 8 == 0
  const YlBandSplit ws = yl_band_split(bx, gx, p.ntiles, G);   // XCD bands, strided items
  const int per = ws.per, slot = ws.slot, band0 = ws.band0, bt = ws.bt, nmine = ws.nmine;
  const long total_chunks = (long)nmine * NC;

  // asynchronous copy of one chunk = the three taps (ky = cc, kx = 0..2) of channel block kb, n-group g, into buffer
  // `buf`: (tap, n-tile) pieces of 1 KiB dealt round-robin to the waves.  The packed image is tap-major (k-step
  // tap * KB + kb, shared with yl_conv_mfma_kernel); this kernel walks it channel-block-major, see below.
  auto load_chunk = [&](int g, int kb, int cc, int buf) {
    for (int i = wave; i < 3 * NT; i += NW) {
      const int j = i / NT, nt = i - j * NT;
      f32x4* dst = wl + ((size_t)buf * 3 * NT + i) * 64;
      yl_glds16(wg + ((size_t)((cc * 3 + j) * KB + kb) * NTtot + g * NT + nt) * 64 + lane, dst);
    }
  };
  if (total_chunks > 0) load_chunk(slot / bt, 0, 0, 0);
  long gchunk = 0;                                            // chunks consumed so far (buffer = gchunk & 1)
  __syncthreads();
  const bool pre_add = (p.res || p.up) && p.act == YL_ACT_NONE;
  const float lo = yl_act_lo(p.act), hi = yl_act_hi(p.act);

  for (int wi = 0; wi < nmine; ++wi) {
    const int item = slot + wi * per;
    const int g = item / bt;
    const int nt0 = g * NT;
    const int tile = band0 + item - g * bt;
    YlPix px[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      px[mt] = yl_pix(((size_t)tile * NW + wave) * (MT * 16) + mt * 16 + pl, M, ohw, OW);
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
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
    // K order: channel block outer, the nine taps inner.  The taps of one 16-channel block read a 3 x 18 pixel x 64 B
    // window per wave, which the 9 consecutive k-steps find in L1 / L2; tap-major (the order of yl_conv_mfma_kernel)
    // puts KB = 21 k-steps of other channels between two touches of a line, more than L1 and the XCD's L2 hold, and
    // FETCH_SIZE showed every tap of every pixel coming from HBM / MALL again: 7.5 GB per launch for a 269 MB input.
    // Per lane: nine tap pointers (the zero buffer where a tap falls outside the image, marked in `inb`).
    const yl_act_t* tp[MT][9];
    unsigned inb[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      inb[mt] = 0;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int iy = px[mt].oy * stride - pad_t + tap / 3, ix = px[mt].ox * stride - pad_l + tap % 3;
        const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
        const long off = in ? ((((long)px[mt].b * (H >> sh) + (iy >> sh)) * (W >> sh) + (ix >> sh)) * Cin + 4 * kq) : zdelta;
        tp[mt][tap] = xin + off;
        inb[mt] |= in ? (1u << tap) : 0u;
      }
    }
    auto fetch = [&](f32x4 (&dst)[MT], int kb, int tap) {
      const bool tail = kb * 16 + 4 * kq >= Cin;                  // channel tail of the last block: zeros
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const yl_act_t* q = tp[mt][tap] + (((inb[mt] >> tap) & 1u) ? kb * 16 : 0);
        dst[mt] = yl_ld4(tail ? xin + zdelta : q);
      }
    };
    f32x4 xq[MT];
    fetch(xq, 0, 0);
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
      for (int cc = 0; cc < 3; ++cc, ++gchunk) {
        const int buf = (int)(gchunk & 1);
        // next chunk of the stream (this item's, or the first one of the workgroup's next item) into the other buffer
        if (gchunk + 1 < total_chunks) {
          if (cc < 2) load_chunk(g, kb, cc + 1, buf ^ 1);
          else if (kb + 1 < KB) load_chunk(g, kb + 1, 0, buf ^ 1);
          else load_chunk((item + per) / bt, 0, 0, buf ^ 1);
        }
        const f32x4* wb = wl + (size_t)buf * 3 * NT * 64 + lane;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int tap = cc * 3 + j;
          f32x4 xn[MT];
          if (tap < 8) fetch(xn, kb, tap + 1);
          else if (kb + 1 < KB) fetch(xn, kb + 1, 0);
          else {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) xn[mt] = xq[mt];
          }
          f32x4 wq[NT];
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) wq[nt] = wb[(j * NT + nt) * 64];
          yl_mma_step<NT, MT>(wq, xq, acc);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) xq[mt] = xn[mt];
        }
        __syncthreads();           // every wave is done with `buf`; the copies into the other buffer have landed
      }
    }
    if (!pre_add && (p.res || p.up || YL_SMOOTH(p.act))) yl_epi_generic<NT, MT>(p, acc, px, nt0, kq);
    else yl_epi_fast<NT, MT>(p, acc, px, nt0, kq, lo, hi, true);
  }
}

// instantiated: (n-tiles per workgroup, m-tiles per wave, waves per workgroup)
#define YL_KXK_SHAPES(X) X(7, 1, 4) X(7, 2, 4) X(7, 1, 8) X(4, 1, 8) X(4, 2, 4)
static YlConvKernel kxk_kernel_of(int NT, int MT, int NW) {
#define YL_KXK_PICK(A, B, C) if (NT == A && MT == B && NW == C) return yl_conv_kxk_kernel<A, B, C>;
  YL_KXK_SHAPES(YL_KXK_PICK)
#undef YL_KXK_PICK
  return nullptr;
}

static hipError_t kxk_go(const YlConvP& p0, int NT, int MT, int NW, int gy, hipStream_t st) {
  const YlConvKernel kern = kxk_kernel_of(NT, MT, NW);
  if (!kern) return hipErrorNotSupported;
  YlConvP p = p0;
  p.ntiles = (int)(((long)p.M + 16 * NW * MT - 1) / (16 * NW * MT));
  const size_t lds = YlKxkLds::bytes(NT);
  const int gx = yl_band_grid(yl_resident_blocks((const void*)kern, NW * 64, lds, 4), (long)p.ntiles * gy);   // gy = n-groups: (m-tile, n-group) items
  hipLaunchKernelGGL(kern, dim3(gx), dim3(NW * 64), lds, st, p);
  return hipGetLastError();
}

// dense 3x3 layers with N % 4 == 0 whose weight image exceeds the LDS budget and whose n-tile count is a multiple of 7
// (yololite_m's 328-channel FPN) or exactly 4 (the 64-channel prototype branch of the seg head: two m-tiles per wave
// so that a weight fragment read feeds 8 MFMAs).  hipErrorNotSupported otherwise (yl_conv_mfma_kernel runs the layer).
hipError_t yl_launch_conv_kxk(const YlConvP& p, hipStream_t st) {
  if (p.k != 3 || p.dw_k > 0 || (p.N & 3) || p.dec_boxes || p.C1 > 0 || p.w3p) return hipErrorNotSupported;
  static const int nwtab[4] = {0, 4, 8, -1};                  // developer A/B ("dev_select" bits 7-9)
  const int NWsel = nwtab[YL_DEV_KXK_NW(p.dev)];
  const int MTsel = (p.dev & YL_DEV_KXK_MT2) ? 2 : 1;
  if (p.NTtot == 4) {
    if (YlKxkLds::image_bytes(p.TK, 4) <= YlKxkLds::LIMIT || NWsel < 0) return hipErrorNotSupported;
    return NWsel == 8 ? kxk_go(p, 4, 1, 8, 1, st) : kxk_go(p, 4, 2, 4, 1, st);
  }
  if (p.NTtot % 7 != 0) return hipErrorNotSupported;
  if (YlKxkLds::image_bytes(p.TK, 7) <= YlKxkLds::LIMIT) return hipErrorNotSupported;      // small enough to stay resident: other kernel
  // 8 waves per workgroup share each weight chunk (half the LDS-DMA issue work per MFMA: 107 -> 114 TFLOP/s on
  // yololite_m's 80x80 level) when there are enough 128-pixel items to keep the tail short; 4 otherwise
  const int gy = p.NTtot / 7;
  const bool eight = NWsel ? NWsel == 8 : ((long)p.M / 128) * gy >= 2 * 2 * YL_NUM_CU;
  return eight ? kxk_go(p, 7, 1, 8, gy, st) : kxk_go(p, 7, MTsel, 4, gy, st);
}

// ------------------------------------------------------------------------------------------------
// Plain 1x1 convolution with MANY channels on both sides (round 3): yololite_m's EfficientNet-Lite blocks at 40x40 /
// 20x20 -- conv_pw 120->720, 208->1248, conv_pwl 720->120, 1248->208, ... (model_v2.py:94-100: timm `ir` blocks) --
// 3.5 of the model's 18.6 ms at 45-63 TFLOP/s through yl_conv_pwt_kernel.  That kernel gives every wave 16 pixels x
// <= 4 n-tiles with BOTH operands straight from L1/L2: five 1-KiB fragment loads per 16 MFMAs, ~40 B/clk per CU at the
// MFMA rate -- it is bound by the vector-memory path, not by the matrix pipe.  Here, as in yl_conv_kxk_kernel: NT
// n-tiles (6..13, an exact divisor of the layer's n-tile count where one exists) per (m-tile, n-group) item, the
// weight stream double-buffered through LDS in chunks of two k-steps shared by the workgroup's NW waves (asynchronous
// copies of chunk c+1 under the MFMAs of chunk c, ONE barrier per chunk, the pipeline running on across items), the
// activation fragment of the next k-step requested before the MFMAs of this one; a wave reads its A fragments from
// LDS in groups of <= 7 (28 VGPRs).  Per 16 pixels and k-step: one L1/L2 load + NT LDS reads for 4 NT MFMAs.  Same k
// order (channel blocks ascending, four sub-steps each) and epilogues as yl_conv_pwt_kernel: bit-identical results.
// DEC (NT == 6, one n-group): the head output under yl_predict -- a wave holds whole rows of <= 96 logits and runs the decode
// epilogue of yl_conv_pwt_kernel on them (yololite_m's 328 -> 85 outputs: 21 k-blocks of weights through LDS once per 64 / 128 pixels
// instead of once per 32 through the vector-memory path).
// NT2 > 0 (with DEC): NT2 more n-tiles from a SECOND weight image (YlConvP::w3p / b3 / C3: the mask coefficients of a segmentation
// head, model_v2.py head output split into 5 + C detection columns and NM coefficient columns) ride in the same launch -- the wave's
// rows are read once instead of once per part; the extra columns are stored plain into the level rows (p.out, p.ldo).
// dynamic LDS of yl_conv_pws_kernel: two buffers of one weight chunk = CH k-steps x NTA pieces of 1 KiB, [2][CH][NTA][64] float4 at 0
struct YlPwsLds {
  static constexpr size_t LIMIT = 64 * 1024;
  static constexpr int CH = 2;                               // k-steps per weight chunk
  static constexpr __host__ __device__ size_t bytes(int NTA) { return (size_t)2 * CH * NTA * 1024; }
};

template <int NT, int NW, bool SC = false, bool DEC = false, int NT2 = 0>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 3 : 4) void yl_conv_pws_kernel(YlConvP p) {
  constexpr int CH = YlPwsLds::CH;
  constexpr int NTA = NT + NT2;                              // n-tiles a wave accumulates
  extern __shared__ __attribute__((aligned(16))) float yl_clds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, pl = lane & 15;
  const int KB = p.KB, NTtot = p.NTtot, Cin = p.Cin, M = p.M;
  const yl_act_t* const xin = p.x;
  f32x4* wl = reinterpret_cast<f32x4*>(yl_clds);            // [2][CH][NTA][64] float4
  const f32x4* wg = reinterpret_cast<const f32x4*>(p.wp);   // [KB][NTtot][64] float4
  const int NC = (KB + CH - 1) / CH;                         // chunks per item
  const int G = (NTtot + NT - 1) / NT;                       // n-groups (the last one may be partial: clamped reads, no stores)
  // work order as in yl_conv_kxk_kernel: XCD x (workgroup b -> XCD b % 8) owns a contiguous band of m-tiles and runs
  // its (n-group, m-tile) items group-major, so that at any time an XCD streams 1/G of the weights out of its own L2
  const int bx = blockIdx.x, gx = gridDim.x;                 // gx % 8 == 0
  const YlBandSplit ws = yl_band_split(bx, gx, p.ntiles, G);   // XCD bands, strided items
  const int per = ws.per, slot = ws.slot, band0 = ws.band0, bt = ws.bt, nmine = ws.nmine;
  const long total_chunks = (long)nmine * NC;
  // asynchronous copy of chunk `c` (k-steps c*CH .. c*CH+CH-1, clamped) of n-group g into buffer `buf`
  auto load_chunk = [&](int g, int c, int buf) {
    for (int i = wave; i < CH * NTA; i += NW) {
      const int j = i / NTA, nt = i - j * NTA;
      int kb = c * CH + j;
      kb = kb < KB ? kb : KB - 1;
      if (NT2 > 0 && nt >= NT) {                              // (wave-uniform) second image: [KB][NT2][64]
        yl_glds16(reinterpret_cast<const f32x4*>(p.w3p) + ((size_t)kb * NT2 + (nt - NT)) * 64 + lane, wl + ((size_t)buf * CH * NTA + i) * 64);
        continue;
      }
      int ntg = g * NT + nt;
      ntg = ntg < NTtot ? ntg : NTtot - 1;
      yl_glds16(wg + ((size_t)kb * NTtot + ntg) * 64 + lane, wl + ((size_t)buf * CH * NTA + i) * 64);
    }
  };
  if (total_chunks > 0) load_chunk(slot / bt, 0, 0);
  long gchunk = 0;                                            // chunks consumed so far (buffer = gchunk & 1)
  __syncthreads();
  const bool pre_add = (p.res || p.up) && p.act == YL_ACT_NONE;
  const float lo = yl_act_lo(p.act), hi = yl_act_hi(p.act);
  const int ohw = p.OH * p.OW;

  for (int wi = 0; wi < nmine; ++wi) {
    const int item = slot + wi * per;
    const int g = item / bt;
    const int nt0 = g * NT;
    const int tile = band0 + item - g * bt;
    YlPix px[1];
    {                                                        // (yl_pix written out, as in yl_conv_pwt_kernel)
      size_t lin = ((size_t)tile * NW + wave) * 16 + pl;
      px[0].valid = lin < (size_t)M;
      if (!px[0].valid) lin = (size_t)M - 1;
      px[0].lin = lin;
      px[0].b = 0; px[0].oy = 0; px[0].ox = 0;
      if (SC || DEC || p.up) {                               // only the upsample-add / decode epilogues / the gate need coordinates
        const int b = (int)(lin / ohw);
        const int rem = (int)(lin - (size_t)b * ohw);
        px[0].b = b;
        px[0].oy = rem / p.OW;
        px[0].ox = rem - px[0].oy * p.OW;
      }
    }
    const yl_act_t* xrow = xin + px[0].lin * Cin + 4 * kq;
    const float* srow = SC ? p.scale + (size_t)px[0].b * Cin + 4 * kq : nullptr;    // squeeze-excite gate of the pixel's image
    f32x4 acc[1][NTA];
#pragma unroll
    for (int nt = 0; nt < NTA; ++nt) acc[0][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (pre_add) {
      const size_t obase = px[0].lin * p.N;
      size_t up_off = 0;
      if (p.up) {
        const int uy = (px[0].oy * p.UH) / p.OH, ux = (px[0].ox * p.UW) / p.OW;
        up_off = (((size_t)px[0].b * p.UH + uy) * p.UW + ux) * p.N;
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = (nt0 + nt) * 16 + 4 * kq;
        if (n < p.N) {
          if (p.res) acc[0][nt] = yl_ld4(p.res + obase + n);
          if (p.up) acc[0][nt] += yl_ld4(p.up + up_off + n);
        }
      }
    }
    auto fetch = [&](int kb) {
      const bool ok = kb * 16 + 4 * kq < Cin;                 // channel tail of the last block: zeros
      f32x4 v = yl_ld4(ok ? xrow + kb * 16 : p.zeros);
      if (SC) v *= yl_ld4(ok ? srow + kb * 16 : reinterpret_cast<const float*>(p.zeros));     // x * gate (one rounding), then the GEMM
      return v;
    };
    // activation fragments PF k-steps ahead (a ring with compile-time slots: the chunk loop is unrolled by two).  One step ahead
    // was 1 KB in flight per wave -- 16-32 KB per CU, which at the ~2 us of a loaded HBM / MALL round trip is ~2 TB/s over the
    // chip: the 328 -> 85 head outputs and the 528 -> 88 projections sat on that, not on the matrix pipe.
    constexpr int PF = 4;
    f32x4 xr[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) xr[i] = fetch(i < KB ? i : KB - 1);
    auto chunk = [&](auto par, int c) {
      constexpr int P = decltype(par)::value;
      const int buf = (int)(gchunk & 1);
      // next chunk of the stream (this item's, or the first one of the workgroup's next item) into the other buffer
      if (gchunk + 1 < total_chunks) {
        if (c + 1 < NC) load_chunk(g, c + 1, buf ^ 1);
        else load_chunk((item + per) / bt, 0, buf ^ 1);
      }
      const f32x4* wb = wl + (size_t)buf * CH * NTA * 64 + lane;
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        constexpr int dummy = 0; (void)dummy;
        const int kb = c * CH + j;
        if (kb < KB) {                                         // (workgroup-uniform) odd KB: the last chunk is half empty
          const int slot = (P * CH + j) % PF;
          constexpr int H0 = NTA > 7 ? (NTA + 1) / 2 : NTA;    // A fragments in two groups: <= 28 VGPRs of them live
          constexpr int H1 = NTA - H0;
          f32x4 xs[1] = {xr[slot]};
          xr[slot] = fetch(kb + PF < KB ? kb + PF : KB - 1);
          {
            f32x4 wq[H0], a0[1][H0];
#pragma unroll
            for (int nt = 0; nt < H0; ++nt) { wq[nt] = wb[(j * NTA + nt) * 64]; a0[0][nt] = acc[0][nt]; }
            yl_mma_step<H0, 1>(wq, xs, a0);
#pragma unroll
            for (int nt = 0; nt < H0; ++nt) acc[0][nt] = a0[0][nt];
          }
          if (H1 > 0) {
            constexpr int H1s = H1 > 0 ? H1 : 1;
            f32x4 wq[H1s], a1[1][H1s];
#pragma unroll
            for (int nt = 0; nt < H1; ++nt) { wq[nt] = wb[(j * NTA + H0 + nt) * 64]; a1[0][nt] = acc[0][H0 + nt]; }
            yl_mma_step<H1s, 1>(wq, xs, a1);
#pragma unroll
            for (int nt = 0; nt < H1; ++nt) acc[0][H0 + nt] = a1[0][nt];
          }
        }
      }
      __syncthreads();             // every wave is done with `buf`; the copies into the other buffer have landed
      ++gchunk;
    };
    for (int c = 0; c < NC; c += 2) {
      chunk(std::integral_constant<int, 0>{}, c);
      if (c + 1 < NC) chunk(std::integral_constant<int, 1>{}, c + 1);
    }
    if (DEC) {                                                // (one n-group: nt0 == 0)
      if (NT2 > 0) {
        constexpr int N2 = NT2 > 0 ? NT2 : 1;
        f32x4 ad[1][NT], am[1][N2];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) ad[0][nt] = acc[0][nt];
#pragma unroll
        for (int nt = 0; nt < NT2; ++nt) am[0][nt] = acc[0][NT + nt];
        YlConvP pm = p;                                       // the second part: plain columns into the level rows
        pm.bias = p.b3; pm.N = p.C3;
        yl_epi_fast<N2, 1>(pm, am, px, 0, kq, lo, hi, true);
        yl_epi_decode<NT, 1, false, true>(p, ad, px, 0, kq, lane);
      } else {
        yl_epi_decode<NT, 1, false, true>(p, *reinterpret_cast<f32x4 (*)[1][NT]>(&acc), px, 0, kq, lane);
      }
      continue;
    }
    if (!pre_add && (p.res || p.up || YL_SMOOTH(p.act))) yl_epi_generic<NTA, 1>(p, acc, px, nt0, kq);
    else yl_epi_fast<NTA, 1>(p, acc, px, nt0, kq, lo, hi, true);
  }
}

// The instantiations of yl_conv_pws_kernel<NT, NW, SC, DEC, NT2>, written once: NT (n-tiles per item, the candidates of
// yl_launch_conv_pws in its order of preference) x 4 / 8 waves x plain / gated input (SC), as [candidate][NW == 8][SC] ...
#define YL_PWS_NTS(X) X(13) X(11) X(9) X(8) X(7) X(6)
#define YL_PWS_NT_VALUE(NT) NT,
#define YL_PWS_NT_KERNELS(NT) \
  {{yl_conv_pws_kernel<NT, 4>, yl_conv_pws_kernel<NT, 4, true>}, {yl_conv_pws_kernel<NT, 8>, yl_conv_pws_kernel<NT, 8, true>}},
static const int pws_nts[6] = {YL_PWS_NTS(YL_PWS_NT_VALUE)};
static const YlConvKernel pws_kernels[6][2][2] = {YL_PWS_NTS(YL_PWS_NT_KERNELS)};
// ... and the decode forms (NT = 6, one n-group), as [NW == 8][with the mask coefficients of the second weight image]
static const YlConvKernel pws_dec_kernels[2][2] = {{yl_conv_pws_kernel<6, 4, false, true>, yl_conv_pws_kernel<6, 4, false, true, 2>},
                                                   {yl_conv_pws_kernel<6, 8, false, true>, yl_conv_pws_kernel<6, 8, false, true, 2>}};

// cand: index into pws_nts
static hipError_t pws_go(const YlConvP& p0, hipStream_t st, int cand, bool eight) {
  const int NT = pws_nts[cand], NW = eight ? 8 : 4;
  YlConvP p = p0;
  p.ntiles = (int)(((long)p.M + 16 * NW - 1) / (16 * NW));
  const int gy = (p.NTtot + NT - 1) / NT;
  // the occupancy question is put to the plain kernel of the candidate, also for its gated and its decode form (same LDS, same
  // launch bounds); the form with the mask coefficients (+ 32 columns = 2 n-tiles from the second weight image) answers for itself
  YlConvKernel kern = pws_kernels[cand][eight][p.scale != nullptr], asked = pws_kernels[cand][eight][0];
  int NTA = NT;
  if (p.dec_boxes) {
    if (NT != 6 || p.scale) return hipErrorNotSupported;
    kern = pws_dec_kernels[eight][p.w3p != nullptr];
    if (p.w3p) { NTA = NT + 2; asked = kern; }
  }
  const size_t lds = YlPwsLds::bytes(NTA);
  const int gx = yl_band_grid(yl_resident_blocks((const void*)asked, NW * 64, lds, 8), (long)p.ntiles * gy);
  hipLaunchKernelGGL(kern, dim3(gx), dim3(NW * 64), lds, st, p);
  return hipGetLastError();
}

// plain 1x1 stride-1 layers (N % 4 == 0, no decode epilogue) with enough channels on both sides that the weight
// stream pays: K >= 80 and >= 6 n-tiles.  hipErrorNotSupported otherwise (yl_conv_pwt_kernel runs the layer).
hipError_t yl_launch_conv_pws(const YlConvP& p, hipStream_t st) {
  const bool dec = p.dec_boxes && !p.dec_raw;                  // head output under yl_predict: rows of <= 96 logits, one n-group
  if (p.k != 1 || p.stride != 1 || p.dw_k > 0 || p.C1 > 0 || p.in_shift || (p.dec_boxes && !dec)) return hipErrorNotSupported;
  if (dec ? (p.NTtot != 6 || p.scale || p.res || p.up || (p.w3p && (p.C3 != 32 || YL_SMOOTH(p.act)))) : ((p.N & 3) != 0 || p.w3p)) return hipErrorNotSupported;
  if ((p.dev & YL_DEV_PWS_OFF) || p.KB < 5 || p.NTtot < 6) return hipErrorNotSupported;     // (dev: A/B runs)
  // n-tiles per item, from {6..13}: the makespan of the launch in MFMA units -- (16-pixel x n-group) wave items dealt
  // to 1024 SIMDs, each NT x KB x 4 MFMAs long -- with a penalty when fewer than 1.5 waves per SIMD exist (one wave
  // alone cannot keep a matrix pipe busy); ties go to the larger NT (fewer passes over the activations).  E.g. 1248 ->
  // 208 at 20x20 x 32 images (13 n-tiles, 800 pixel tiles): NT = 7 in two groups (116 -> 90 us), not 13 in one.
  int NT = 0, cand = 0;
  double best = 1e30;
  long best_wi = 0;
  const long mt16 = ((long)p.M + 15) / 16;
  for (int i = dec ? 5 : 0; i < 6; ++i) {
    const long wi = mt16 * ((p.NTtot + pws_nts[i] - 1) / pws_nts[i]);
    const double sc = (double)((wi + 1023) / 1024) * pws_nts[i] * (wi < 1536 ? 1.25 : 1.0);
    if (sc < best) { best = sc; NT = pws_nts[i]; cand = i; best_wi = wi; }
  }
  if (best_wi < 1536) return hipErrorNotSupported;      // too few items for workgroup-shared weights: wave-autonomous kernel
  const int gy = (p.NTtot + NT - 1) / NT;
  const bool eight = ((long)p.M / 128) * gy >= 2 * 2 * YL_NUM_CU;          // enough 128-pixel items for 8-wave workgroups
  return pws_go(p, st, cand, eight);
}

// ------------------------------------------------------------------------------------------------
// Whole EfficientNet-style inverted-residual block in ONE launch (round 3):  1x1 expand (+BN+act) -> depthwise DK x DK,
// stride 1 or 2, TF-SAME or symmetric padding (+BN+act) -> 1x1 project (+BN) (+residual) -- timm's `ir` blocks behind
// model_v2.py:94-100.  Built for the EARLY blocks of yololite_m (tf_efficientnet_lite2: 16->96->24 at 320x320, 24->144->24 at
// 160x160, 48->288->48 at 80x80, ...), where the 6x expanded tensor is the largest tensor of the network (1.26 GB at B = 32)
// and the two-launch form (conv_pw, then depthwise + conv_pwl) spends its time writing and re-reading it at 3-4 TB/s:
// 2.7 of the model's 17.6 ms.  Here the expanded tensor exists only as one 16-channel SLAB of the workgroup's halo region
// in LDS.
//   workgroup tile  4*RBN x 4*MT*CBN output pixels, RBN x CBN waves (2 x 2, or 1 x 5 for 20 x 20 grids), wave w owns the
//                   4 x 4*MT block (w / CBN, w % CBN)
//   per slab kb     E: the halo region ((TH-1)*DS+DK rows x (TW-1)*DS+DK columns of expanded pixels, 16-pixel m-tiles
//                      dealt to the waves) = act(bias + Wexp[kb] . x) by MFMA from the block input held in registers
//                      for the whole tile, zero outside the image (the depthwise conv pads the EXPANDED tensor) -> LDS;
//                   barrier (ONE per slab: slabs and projection weights are double-buffered, the counters run on
//                      across tiles);
//                   D: B fragment of the lane's pixel = act(bias + sum of taps), taps and weights from LDS, in the tap
//                      order of yl_conv_dwt_kernel;  P: NT x 4 MFMAs per m-tile against the projection weights of
//                      the slab (asynchronous global -> LDS copy issued one slab ahead).
// The old yl_uib_kernel (yl_conv.hip, MobileNetV4 blocks) recomputes the expansion on a (3+DK)^2 halo per 4x4 tile and
// WAVE: 2.25-4x the expansion MFMAs; the workgroup-level halo here costs 1.2x (stride 2) to 1.9x (5x5 stride 1).  Same
// k orders (input channel blocks ascending; slabs = the projection's k blocks ascending; taps (dy,dx)) and epilogues as
// the two-launch form: bit-identical results.
// (Round 3, second half: a wave-autonomous form of the 48 -> 96 -> 48 blocks on an LDS-DMA-staged 6x6 input patch -- the
// recipe of yl_conv_s2c_kernel, no workgroup barrier, 288 MFMAs per 16 pixels instead of 198 -- was built and was
// bit-identical: 49.1 us per B = 64 launch against 46.2 us here, and 38.4k against 40.0k images/s on the two-stream
// headline (118 KB of LDS per CU also keeps the other chunk's kernels off the CU).  Not kept.  Likewise a START-depthwise
// form of this kernel for edge_n blocks.2.0 (dw5 -> 32->96 -> dw5 s2 -> 96->48 as one launch: the expansion's B fragments
// computed per halo pixel from 25 x 2 float4 taps read straight from L1/L2, bit-identical, the 157 MB expanded tensor
// never written): 35.4k against 40.0k images/s -- 300 dependent tap loads per lane and tile at two workgroups per CU;
// it would need the block input staged in LDS (68 KB per 8x8 tile).  Not kept.)
// expanded-halo slab of a workgroup tile of 4 RBN x 4 MT CBN output pixels: row pitch in floats (see yl_conv_dwh_kernel), floats
constexpr __host__ __device__ int yl_ir_pitch(int dk, int ds, int mt, int cbn) { return ((((4 * mt * cbn - 1) * ds + dk) * 16 + 7) / 64) * 64 + 56; }
constexpr __host__ __device__ int yl_ir_slab(int dk, int ds, int mt, int rbn, int cbn) { return ((4 * rbn - 1) * ds + dk) * yl_ir_pitch(dk, ds, mt, cbn); }
// dynamic LDS of yl_ir_kernel (offsets in floats): [2] slabs | [2][NT][64] float4 projection weights of a slab | [KB][DK*DK + 1][16]
// taps + dw bias of a slab's channels (zeros beyond Cmid; k-block-major, so that a lane's tap reads of a slab are ONE address +
// immediates) | [KB*16] expansion bias
struct YlIrLds {
  static constexpr size_t LIMIT = 150 * 1024;
  size_t wpl, dwl, b2l, bytes;
  constexpr __host__ __device__ YlIrLds(int dk, int ds, int mt, int rbn, int cbn, int nt, int KB)
      : wpl((size_t)2 * yl_ir_slab(dk, ds, mt, rbn, cbn)), dwl(wpl + (size_t)2 * nt * 256), b2l(dwl + (size_t)KB * (dk * dk + 1) * 16),
        bytes((b2l + (size_t)KB * 16) * 4) {}
};

// Two forms of one text.  CLAMP = false is the kernel as it was first written and takes every case.  CLAMP = true (the launcher
// picks it when act, act2 and dw_act are all clamp-type -- none / ReLU / ReLU6, !YL_SMOOTH -- and the block input, the FPN
// addend and the expansion weights lie within 32-bit byte offsets) is the same arithmetic with less beside the MFMAs:
//   - the activation is yl_clamp4 alone: exactly what yl_actc evaluates for a clamp-type id (yl_ir_act below), so no SiLU code
//     and no activation branch is compiled into the slab loop;
//   - the block input, the expansion weights and the FPN addend are read through raw buffer descriptors: a 32-bit byte offset per
//     lane, fixed per workgroup (weights) or per tile (halo pixels), + a scalar offset per slab -- no 64-bit vector address
//     arithmetic and no pointer select against p.zeros per slab.  A halo pixel outside the image carries an out-of-range offset
//     and reads zeros from the range check, as it read p.zeros; the channel tails carry one where a tail can be: the last input
//     k-block (once per tile), the last slab of the addend.  The projection weights' LDS-DMA requests stay global loads (32-bit
//     index arithmetic), waited for at the slab barrier as before.
// Same k order, tap order, fma chains and epilogues: the two forms are bit-identical (tests/test_ir_forms_gpu.py).
// Measured and NOT in the second form (one-stream medians at edge_n 640^2, B = 64, us: UIB 40x40 / lateral3 / lateral4; parent
// 47.1 / 170.4 / 60.3, the form above 43.4 / 163.4 / 57.2): the 3 x 3 tap loop unrolled to immediates, a row at a time where
// registers are tight, 54.4 / 171.1 / 125.4, with the taps as v_pk_fma_f32 by name 45.1 / 173.7 / 59.6; packed taps in the rolled
// loop with empty halo slots skipped and full m-tiles stored unmasked 46.0 / 182.6 / 61.1; the skip and the unmasked store alone
// 44.8 / 171.9 / 58.3; `up` decided once per slab instead of per m-tile: no difference.  The static vector-instruction count of
// the slab loop fell to a third in all of them -- it is not what these kernels wait for (profiles/README.md, ir_mix_*).
template <bool CLAMP>
__device__ __forceinline__ f32x4 yl_ir_act(f32x4 v, int act, float lo, float hi) {
  if constexpr (CLAMP) return yl_clamp4(v, lo, hi);      // == yl_actc(v, act, lo, hi) for !YL_SMOOTH(act): its second return
  else return yl_actc(v, act, lo, hi);
}
// waves per SIMD the kernel is compiled for.  The second form promises what the first form reaches: <3,6,3,1,1> asks for 2 and
// fits 3 (163 VGPRs)
constexpr int yl_ir_waves(int kbi, int nt, int dk, int ds, int mt, bool clamp) {
  return (dk == 3 && ds * mt <= 2 && kbi <= 3 && (nt <= 3 || (clamp && ds * mt == 1))) ? 3 : 2;
}
template <int KBI /*ceil(C1/16)*/, int NT, int DK, int DS, int MT, int RBN /*wave rows*/, int CBN /*wave columns*/, bool CLAMP>
__global__ __launch_bounds__(RBN * CBN * 64, yl_ir_waves(KBI, NT, DK, DS, MT, CLAMP)) void yl_ir_kernel(YlConvP p) {
  constexpr int NWV = RBN * CBN, NTH = NWV * 64;                   // waves / threads per workgroup
  constexpr int TH = 4 * RBN, TW = 4 * MT * CBN;                   // workgroup tile: every wave a 4 x 4 MT block
  constexpr int HH = (TH - 1) * DS + DK, HW = (TW - 1) * DS + DK, HN = HH * HW;
  constexpr int HMT = (HN + 15) / 16, HMW = (HMT + NWV - 1) / NWV; // halo m-tiles: all, per wave
  constexpr int PITCHF = yl_ir_pitch(DK, DS, MT, CBN), SLAB = yl_ir_slab(DK, DS, MT, RBN, CBN);
  extern __shared__ __attribute__((aligned(16))) float yl_clds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, pl = lane & 15;
  const int Cmid = p.Cin, KB = p.KB, NTtot = p.NTtot, C1 = p.C1, H = p.H, W = p.W, OH = p.OH, OW = p.OW, N = p.N;
  const YlIrLds L(DK, DS, MT, RBN, CBN, NT, KB);
  float* slab = yl_clds;
  f32x4* wpl = reinterpret_cast<f32x4*>(yl_clds + L.wpl);
  float* dwl = yl_clds + L.dwl;
  float* b2l = yl_clds + L.b2l;
  const f32x4* wg = reinterpret_cast<const f32x4*>(p.wp);          // projection [KB][NTtot][64]
  const f32x4* w2g = reinterpret_cast<const f32x4*>(p.w2p);        // expansion [KBI][KB][64]
  const yl_act_t* const xin = p.x;
  const yl_act_t* const up = p.up;                                     // FPN lateral + smooth pair: addend of the expansion
  {
    constexpr int T1 = DK * DK + 1;
    for (int i = tid; i < KB * T1 * 16; i += NTH) {
      const int kb = i / (T1 * 16), r = i - kb * (T1 * 16), t = r >> 4, ch = kb * 16 + (r & 15);
      dwl[i] = ch < Cmid ? (t < DK * DK ? p.dw_w[(size_t)t * Cmid + ch] : (p.dw_b ? p.dw_b[ch] : 0.0f)) : 0.0f;
    }
    for (int i = tid; i < KB * 16; i += NTH) b2l[i] = p.b2[i];
  }
  const float lo = yl_act_lo(p.act), hi = yl_act_hi(p.act);
  const float dlo = yl_act_lo(p.dw_act), dhi = yl_act_hi(p.dw_act);
  const float elo = yl_act_lo(p.act2), ehi = yl_act_hi(p.act2);
  const int dw_act = p.dw_act, act2 = p.act2;
  // lane constants: the lane's halo pixel in each of the wave's halo m-tiles (m = wave + 4 j)
  int h_r[HMW], h_c[HMW], h_lo[HMW];
  bool h_ok[HMW];
#pragma unroll
  for (int j = 0; j < HMW; ++j) {
    const int q = (wave + NWV * j) * 16 + pl;
    h_ok[j] = q < HN;
    const int qq = h_ok[j] ? q : 0;
    h_r[j] = qq / HW;
    h_c[j] = qq - h_r[j] * HW;
    h_lo[j] = h_r[j] * PITCHF + h_c[j] * 16 + 4 * kq;
  }
  const int rb = wave / CBN, cb = wave - rb * CBN;                  // the wave's 4 x 4 MT block of the tile
  const int rbase = ((4 * rb + (pl >> 2)) * DS) * PITCHF + ((cb * 4 * MT + (pl & 3)) * DS) * 16 + 4 * kq;
  const bool pre_add = p.res != nullptr && p.act == YL_ACT_NONE;
  const int twn = OW / TW, thn = OH / TH;
  const int tiles_img = twn * thn;
  const int ntiles = p.B * tiles_img;
  int tile, tend, tstride;
  if ((gridDim.x & 7) == 0) {                                      // XCD bands, see yl_conv_dwt_kernel
    const int tpx = (ntiles + 7) >> 3;                             // (written out for the same reason)
    const int band0 = (blockIdx.x & 7) * tpx;
    tend = (band0 + tpx) < ntiles ? (band0 + tpx) : ntiles;
    tile = band0 + (blockIdx.x >> 3);
    tstride = gridDim.x >> 3;
  } else {
    tile = blockIdx.x; tend = ntiles; tstride = gridDim.x;
  }
  auto load_proj = [&](int kb, int buf) {                           // projection weights of slab kb -> LDS (asynchronous)
    for (int nt = wave; nt < NT; nt += NWV) {
      if constexpr (CLAMP) yl_glds16(wg + (unsigned)((kb * NTtot + (nt < NTtot ? nt : NTtot - 1)) * 64) + (unsigned)lane, wpl + (buf * NT + nt) * 64);
      else yl_glds16(wg + ((size_t)kb * NTtot + (nt < NTtot ? nt : NTtot - 1)) * 64 + lane, wpl + ((size_t)buf * NT + nt) * 64);
    }
  };
  // second form: the block input, the FPN addend and the expansion weights through raw buffer descriptors (see yl_conv_dwk_kernel):
  // a 32-bit byte offset per lane + a scalar offset per slab; an offset of 2^31 is out of range and reads zeros
  constexpr int ESZ = (int)sizeof(yl_act_t);
  constexpr unsigned OOR = 0x80000000u;
  const int lane16 = lane * 16;
  __amdgpu_buffer_rsrc_t xrs, urs, wrs;
  if constexpr (CLAMP) {
    xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<yl_act_t*>(xin), 0, p.B * H * W * C1 * ESZ, 0x00020000);
    urs = __builtin_amdgcn_make_buffer_rsrc(const_cast<yl_act_t*>(up ? up : xin), 0, up ? p.B * p.UH * p.UW * Cmid * ESZ : 0, 0x00020000);
    wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<f32x4*>(w2g), 0, KBI * KB * 1024, 0x00020000);
  }
  auto bld4 = [&](__amdgpu_buffer_rsrc_t rs, unsigned voff, int soff) {   // four channels of an activation tensor
#if YL_F16S
    return __builtin_convertvector(__builtin_bit_cast(yl_h16x4, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)voff, soff, 0)), f32x4);
#else
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, soff, 0));
#endif
  };
  unsigned gs = 0;                                                  // slabs started by this workgroup (buffer = gs & 1)
  if (tile < tend) load_proj(0, 0);
  __syncthreads();

  // (wi is never read.  Without this second induction variable the compiler emits the loop differently; it stays until the
  // kernel's code is next allowed to change.)
  // (the first form only; the second has no such variable)
  for (int wi = 0; tile < tend; tile += tstride, wi += CLAMP ? 0 : 1) {
    const int b = tile / tiles_img;
    const int trem = tile - b * tiles_img;
    const int tyi = trem / twn, txi = trem - tyi * twn;
    const int iy0 = tyi * TH * DS - p.dw_pad_t, ix0 = txi * TW * DS - p.dw_pad_l;
    YlPix px[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      px[mt].b = b;
      px[mt].oy = tyi * TH + 4 * rb + (pl >> 2);
      px[mt].ox = txi * TW + cb * 4 * MT + 4 * mt + (pl & 3);
      px[mt].valid = true;
      px[mt].lin = ((size_t)b * OH + px[mt].oy) * OW + px[mt].ox;
    }
    // block input at the lane's halo pixels: B fragments of the expansion GEMM, resident for the tile
    f32x4 xh[HMW][KBI];
    bool h_in[HMW];
    long uoff[HMW];
    unsigned uo[HMW];                                                // second form: byte offset of the addend, out of range outside the image
#pragma unroll
    for (int j = 0; j < HMW; ++j) {
      const int iy = iy0 + h_r[j], ix = ix0 + h_c[j];
      h_in[j] = h_ok[j] && iy >= 0 && iy < H && ix >= 0 && ix < W;
      if constexpr (CLAMP) {
        uo[j] = OOR;
        if (up && h_in[j]) uo[j] = (unsigned)(((((b * p.UH + (iy * p.UH) / H) * p.UW + (ix * p.UW) / W) * Cmid) + 4 * kq) * ESZ);
        const unsigned xo = h_in[j] ? (unsigned)((((b * H + iy) * W + ix) * C1 + 4 * kq) * ESZ) : OOR;
#pragma unroll
        for (int kbi = 0; kbi < KBI; ++kbi)                          // only the last k-block can hold a channel tail
          xh[j][kbi] = bld4(xrs, ((kbi + 1 < KBI || (kbi * 16 + 4 * kq) < C1) ? xo : OOR) + kbi * 16 * ESZ, 0);
        continue;
      }
      uoff[j] = 0;
      if (up && h_in[j]) uoff[j] = ((((long)b * p.UH + (iy * p.UH) / H) * p.UW + (ix * p.UW) / W) * Cmid) + 4 * kq;
      const yl_act_t* src = xin + (((size_t)b * H + iy) * W + ix) * C1 + 4 * kq;
#pragma unroll
      for (int kbi = 0; kbi < KBI; ++kbi) {
        const bool ok = h_in[j] && (kbi * 16 + 4 * kq) < C1;
        xh[j][kbi] = yl_ld4(ok ? src + kbi * 16 : p.zeros);
      }
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int n = nt * 16 + 4 * kq;
        if (pre_add && n < N) acc[mt][nt] = yl_ld4(p.res + px[mt].lin * N + n);
      }
    f32x4 we[KBI], wn[KBI];
#pragma unroll
    for (int kbi = 0; kbi < KBI; ++kbi) {
      if constexpr (CLAMP) wn[kbi] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, lane16, kbi * KB * 1024, 0));
      else wn[kbi] = w2g[((size_t)kbi * KB + 0) * 64 + lane];
    }
    // FPN lateral: the addend of slab kb + 1 (the nearest-upsampled coarser level at the lane's halo pixels) is requested
    // one slab ahead like the expansion weights -- requested where it is used, every slab began with a wait for a
    // fragment-shaped load from L2 in front of its first MFMA (it initialises the accumulator)
    // (one register set: m-tile j's addend of slab kb + 1 is requested right behind the MFMAs that consumed slab kb's)
    f32x4 un[HMW];
    auto load_up = [&](int kb, int j) {
      if constexpr (CLAMP) {
        // only the last slab can hold a channel tail
        return bld4(urs, (kb + 1 < KB || kb * 16 + 4 * kq < Cmid) ? uo[j] : OOR, kb * 16 * ESZ);
      } else {
        return yl_ld4((h_in[j] && kb * 16 + 4 * kq < Cmid) ? up + uoff[j] + kb * 16 : p.zeros);
      }
    };
    if (up) {
#pragma unroll
      for (int j = 0; j < HMW; ++j) un[j] = load_up(0, j);
    }
    for (int kb = 0; kb < KB; ++kb, ++gs) {
      const int buf = (int)(gs & 1u);
#pragma unroll
      for (int kbi = 0; kbi < KBI; ++kbi) we[kbi] = wn[kbi];
      if (kb + 1 < KB) {
#pragma unroll
        for (int kbi = 0; kbi < KBI; ++kbi) {
          if constexpr (CLAMP) wn[kbi] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, lane16, (kbi * KB + kb + 1) * 1024, 0));
          else wn[kbi] = w2g[((size_t)kbi * KB + kb + 1) * 64 + lane];
        }
      }
      // ---- E: expansion slab on the wave's halo m-tiles -> LDS
      const f32x4 eb = yl_ld4(b2l + kb * 16 + 4 * kq);
      float* sb = slab + buf * SLAB;
#pragma unroll
      for (int j = 0; j < HMW; ++j) {
        f32x4 e[1][1] = {{{0.f, 0.f, 0.f, 0.f}}};
        if (up) e[0][0] = un[j];   // FPN lateral: the nearest-upsampled coarser level initialises the accumulator (the order
                                   // of the stand-alone lateral conv: (addend + products) + bias)
#pragma unroll
        for (int kbi = 0; kbi < KBI; ++kbi) {
          const f32x4 wq1[1] = {we[kbi]};
          const f32x4 xq1[1] = {xh[j][kbi]};
          yl_mma_step<1, 1>(wq1, xq1, e);
        }
        if (up && kb + 1 < KB) un[j] = load_up(kb + 1, j);
        const f32x4 v = yl_sel4(h_in[j], yl_ir_act<CLAMP>(e[0][0] + eb, act2, elo, ehi));   // zero padding of the EXPANDED tensor
        if (h_ok[j]) *reinterpret_cast<f32x4*>(sb + h_lo[j]) = v;
      }
      __syncthreads();                 // slab `buf` complete; the projection weights of this slab have landed
      if (kb + 1 < KB) load_proj(kb + 1, buf ^ 1);
      else if (tile + tstride < tend) load_proj(0, buf ^ 1);        // first slab of the workgroup's next tile
      // ---- D: depthwise on the slab -> B fragments
      const float* tapw = dwl + kb * ((DK * DK + 1) * 16) + 4 * kq;
      f32x4 xq[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) xq[mt] = yl_ld4(tapw + DK * DK * 16);
      auto tap_row = [&](int dy) {
#pragma unroll
        for (int dx = 0; dx < DK; ++dx) {
          const f32x4 w = yl_ld4(tapw + (dy * DK + dx) * 16);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(sb + rbase + dy * PITCHF + (dx + 4 * mt * DS) * 16);
            xq[mt].x = fmaf(v.x, w.x, xq[mt].x); xq[mt].y = fmaf(v.y, w.y, xq[mt].y);
            xq[mt].z = fmaf(v.z, w.z, xq[mt].z); xq[mt].w = fmaf(v.w, w.w, xq[mt].w);
          }
        }
      };
#pragma unroll 1
      for (int dy = 0; dy < DK; ++dy) tap_row(dy);                   // one tap row at a time bounds the register footprint
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) xq[mt] = yl_ir_act<CLAMP>(xq[mt], dw_act, dlo, dhi);
      // channel tail (c >= Cmid): the packed projection weights of those k slots are zero, no select needed.  The slab channels
      // there are computed from the block input with zero expansion weights and bias; that input is masked at C1 and the halo
      // stays inside the tile's image (h_in), so they can only carry this image's own non-finite values, never a neighbour's
      // ---- P: projection
      f32x4 wq[NT];
      const f32x4* wrow = wpl + (size_t)buf * NT * 64 + lane;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) wq[nt] = wrow[nt * 64];
      yl_mma_step<NT, MT>(wq, xq, acc);
    }
    if (!pre_add && (p.res || (!CLAMP && YL_SMOOTH(p.act)))) yl_epi_generic<NT, MT>(p, acc, px, 0, kq);
    else yl_epi_fast<NT, MT>(p, acc, px, 0, kq, lo, hi, true);
  }
}

template <int KBI, int NT, int DK, int DS, int MT, int RBN, int CBN, bool CLAMP>
static hipError_t ir_go(const YlConvP& p, hipStream_t st, bool second) {
  if (CLAMP && !second) return hipErrorNotSupported;                 // SiLU somewhere, or past 32-bit offsets: the first form runs
  const size_t lds = YlIrLds(DK, DS, MT, RBN, CBN, NT, p.KB).bytes;
  const long ntiles = (long)p.B * (p.OH / (4 * RBN)) * (p.OW / (4 * MT * CBN));
  int gx = yl_resident_blocks((const void*)yl_ir_kernel<KBI, NT, DK, DS, MT, RBN, CBN, CLAMP>, RBN * CBN * 64, lds, 8);
  if (gx > ntiles) gx = (int)ntiles;
  if (gx >= 8) gx &= ~7;
  hipLaunchKernelGGL((yl_ir_kernel<KBI, NT, DK, DS, MT, RBN, CBN, CLAMP>), dim3(gx), dim3(RBN * CBN * 64), lds, st, p);
  return hipGetLastError();
}

// instantiated shapes: (input k-blocks, projection n-tile bucket, dw k, dw stride, m-tiles per wave, wave rows, wave columns).
// Buckets: 2 = 1-2 n-tiles, 3 = 3, 4 = 4, 6 = 5-6.  Workgroup tile = 4*rows x 4*MT*columns output pixels: 2 x 2 waves for
// the grids that are multiples of 8 / 16.  (1 x 5 waves = 4 x 20 pixel tiles for the 20 x 20 stage of edge_n were built
// and measured: 320 workgroup tiles per B = 64 launch, 0.083-0.114 ms per block against 0.055-0.067 ms for the
// two-launch form -- not instantiated.)
#define YL_IR_SHAPES(X)                                                                                              \
  X(1, 2, 3, 2, 1, 2, 2) X(2, 2, 3, 1, 2, 2, 2) X(2, 3, 5, 2, 1, 2, 2) X(3, 3, 5, 1, 2, 2, 2) X(3, 6, 3, 2, 1, 2, 2)    \
  X(3, 3, 3, 1, 1, 2, 2) X(2, 6, 3, 1, 2, 2, 2) X(3, 6, 3, 1, 1, 2, 2)
#define YL_IR_BUCKET_LO(B) ((B) == 2 ? 0 : (B) == 3 ? 2 : (B) == 4 ? 3 : 4)

// fused inverted-residual block (p.C1 > 0).  hipErrorNotSupported: shape not instantiated (yl_uib_kernel or the
// two-launch form handles it -- yl_ir_supported tells the host compiler beforehand)
bool yl_ir_supported(int c1, int cmid, int n, int dk, int ds, int oh, int ow) {
  const int kbi = (c1 + 15) / 16, nt = (n + 15) / 16;
#define YL_IR_CHECK(A, B, C, D, E, R, S)                                                                             \
  if (kbi == A && nt <= B && nt > YL_IR_BUCKET_LO(B) && dk == C && ds == D && (oh % (4 * R)) == 0 &&                    \
      (ow % (4 * E * S)) == 0 && YlIrLds(C, D, E, R, S, B, (cmid + 15) / 16).bytes <= YlIrLds::LIMIT) return true;
  YL_IR_SHAPES(YL_IR_CHECK)
#undef YL_IR_CHECK
  return false;
}

// The one decision of yl_launch_conv_ir and yl_query_ir_form: 0 = no instantiation, 1 = the first form of the instantiation
// written to shape[7] (if given), 2 = its second form (CLAMP): all three activations clamp-type and the block input, the FPN
// addend (uh x uw x cmid per image; uh = 0: none) and both weight images within 32-bit byte offsets -- the kernel adds a
// lane's float4 and one k-block to an offset, hence the margin.  Anything else keeps the first form.
int yl_ir_form(int c1, int cmid, int n, int dk, int ds, int oh, int ow, int batch, int h, int w, int uh, int uw, int act,
               int dw_act, int act2, int* shape) {
  const int kbi = (c1 + 15) / 16, nt = (n + 15) / 16, KB = (cmid + 15) / 16;
  const size_t lim = ((size_t)1 << 31) - 4096, e = sizeof(yl_act_t);
  const bool second = !YL_SMOOTH(act) && !YL_SMOOTH(dw_act) && !YL_SMOOTH(act2) && batch > 0 && h > 0 && w > 0 && uh >= 0 && uw >= 0 &&
                      (size_t)batch * h * w * c1 * e < lim && (size_t)batch * uh * uw * cmid * e < lim &&
                      (size_t)kbi * KB * 1024 < lim && (size_t)KB * nt * 1024 < lim;
#define YL_IR_FORM(A, B, C, D, E, R, S)                                                                              \
  if (kbi == A && nt <= B && nt > YL_IR_BUCKET_LO(B) && dk == C && ds == D && (oh % (4 * R)) == 0 &&                    \
      (ow % (4 * E * S)) == 0 && YlIrLds(C, D, E, R, S, B, KB).bytes <= YlIrLds::LIMIT) {                                \
    const int sh[7] = {A, B, C, D, E, R, S};                                                                         \
    for (int i = 0; shape && i < 7; ++i) shape[i] = sh[i];                                                           \
    return second ? 2 : 1;                                                                                           \
  }
  YL_IR_SHAPES(YL_IR_FORM)
#undef YL_IR_FORM
  return 0;
}

hipError_t yl_launch_conv_ir(const YlConvP& p, hipStream_t st) {
  if (p.C1 <= 0 || p.k != 1 || p.dw_k == 0 || (p.N & 3)) return hipErrorNotSupported;
  const int kbi = (p.C1 + 15) / 16, nt = p.NTtot;
  const bool second = yl_ir_form(p.C1, p.Cin, p.N, p.dw_k, p.dw_stride, p.OH, p.OW, p.B, p.H, p.W, p.up ? p.UH : 0, p.up ? p.UW : 0,
                                 p.act, p.dw_act, p.act2, nullptr) == 2;
#define YL_IR_RUN(A, B, C, D, E, R, S)                                                                               \
  if (kbi == A && nt <= B && nt > YL_IR_BUCKET_LO(B) && p.dw_k == C && p.dw_stride == D && (p.OH % (4 * R)) == 0 &&     \
      (p.OW % (4 * E * S)) == 0 && YlIrLds(C, D, E, R, S, B, p.KB).bytes <= YlIrLds::LIMIT) {                               \
    const hipError_t e2 = ir_go<A, B, C, D, E, R, S, true>(p, st, second);                                           \
    return e2 != hipErrorNotSupported ? e2 : ir_go<A, B, C, D, E, R, S, false>(p, st, second);                        \
  }
  YL_IR_SHAPES(YL_IR_RUN)
#undef YL_IR_RUN
  return hipErrorNotSupported;
}

// ------------------------------------------------------------------------------------------------
// Depthwise 3x3 -> 1x1 convolution whose 1x1 weights do not fit LDS (edge_m's 244-channel and yololite_m's
// 328-channel neck / head blocks, model_v2.py:24-41: 240-430 KB packed).  yl_conv_dwh_kernel cannot hold the image and
// the layer fell to yl_conv_mfma_kernel's streamed mode (48 TFLOP/s: fill / use barriers, 21 n-tiles as 8 + 8 + 5).
// Same machinery as yl_conv_kxk_kernel: NT = 7 or 8 n-tiles per workgroup item, the weight stream double-buffered
// through LDS in chunks of three k-steps with one barrier per chunk, (n-group, m-tile) items dealt group-major in XCD
// bands.  The B operand of k-step kb is the depthwise result of the lane's pixel for 4 channels of block kb: nine
// float4 taps straight from L1/L2 (requested one k-step ahead), bias + 9 fma in the tap order of
// yl_conv_dwh_kernel, activation -- no halo patch in LDS.  Each n-group recomputes the depthwise part (36 fma per
// 28-32 MFMAs).  Same k order and epilogues as the kernels it replaces: bit-identical.
// GW = n-groups held by ONE wave (accumulators GW x NT x 4 VGPRs): 1 = every (n-group, m-tile) pair is its own item
// and the depthwise part is recomputed per group; GW = all groups = no recomputation, 2 waves per SIMD.
// dynamic LDS of yl_conv_dwk_kernel (offsets in floats): [2][S][GW][NT][64] float4 weight chunks | [9][Cin] taps, [Cin] bias
struct YlDwkLds {
  static constexpr size_t LIMIT = 96 * 1024;
  // k-steps per weight chunk (= per barrier): 3 when a wave holds one n-group; with all groups in one wave 2 where two
  // buffers of 2 x GW x NT KiB still leave two workgroups per CU (edge_m's 244 channels: 0.359 -> 0.341 ms), else 1
  static constexpr __host__ __device__ int steps(int NT, int GW) { return GW == 1 ? 3 : (GW * NT <= 16 ? 2 : 1); }
  size_t dwl, bytes;
  constexpr __host__ __device__ YlDwkLds(int NT, int GW, int Cin)
      : dwl((size_t)2 * steps(NT, GW) * GW * NT * 256), bytes((dwl + yl_taps_floats(3, Cin)) * 4) {}
};

template <int NT, int GW, int NW>
__global__ __launch_bounds__(NW * 64, GW == 1 ? 3 : 2) void yl_conv_dwk_kernel(YlConvP p) {
  constexpr int S = YlDwkLds::steps(NT, GW);
  constexpr int PCS = S * GW * NT;                           // 1 KiB pieces per chunk
  extern __shared__ __attribute__((aligned(16))) float yl_clds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, pl = lane & 15;
  const int KB = p.KB, NTtot = p.NTtot;
  const int Cin = p.Cin, H = p.H, W = p.W, DS = p.dw_stride, pad_t = p.dw_pad_t, pad_l = p.dw_pad_l;
  const int ohw = p.OH * p.OW, OW = p.OW, M = p.M;
  const yl_act_t* const xin = p.x;
  // tap loads through a raw buffer descriptor (round 6, see yl_conv_dws_kernel): a 32-bit byte offset per tap fixed for the item +
  // a scalar k-block offset (the loop carried a select, a conditional add and a 64-bit add per tap); taps outside the image carry
  // an out-of-range offset (zeros from the range check).  The channel tail of the last k-block loads the next pixel's channels
  // (no per-tap mask in the loop); its depthwise results are replaced by zeros before the 1x1
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<yl_act_t*>(xin), 0, (int)((long)p.B * H * W * Cin * (long)sizeof(yl_act_t)), 0x00020000);
  f32x4* wl = reinterpret_cast<f32x4*>(yl_clds);
  float* dwl = yl_clds + YlDwkLds(NT, GW, Cin).dwl;
  const f32x4* wg = reinterpret_cast<const f32x4*>(p.wp);
  const int NC = (KB + S - 1) / S;                           // chunks per item
  const int G = NTtot / (NT * GW);                           // item groups (1 when the wave holds every n-group)
  const int bx = blockIdx.x, gx = gridDim.x;                 // gx % 8 == 0
  const YlBandSplit ws = yl_band_split(bx, gx, p.ntiles, G);   // XCD bands, strided items
  const int per = ws.per, slot = ws.slot, band0 = ws.band0, bt = ws.bt, nmine = ws.nmine;
  const long total_chunks = (long)nmine * NC;
  auto load_chunk = [&](int g, int c, int buf) {
    for (int i = wave; i < PCS; i += NW) {
      const int j = i / (GW * NT), nt = i - j * (GW * NT);
      const int kb = c * S + j;
      if (kb < KB) yl_glds16(wg + ((size_t)kb * NTtot + g * (GW * NT) + nt) * 64 + lane, wl + ((size_t)buf * PCS + i) * 64);
    }
  };
  if (total_chunks > 0) load_chunk(slot / bt, 0, 0);
  {
    const int nw = 9 * Cin;
    yl_glds_floats(p.dw_w, dwl, nw, tid, NW * 64);
    if (p.dw_b) yl_glds_floats(p.dw_b, dwl + nw, Cin, tid, NW * 64);
    else for (int i = tid; i < Cin; i += NW * 64) dwl[nw + i] = 0.0f;
  }
  long gchunk = 0;
  __syncthreads();
  const bool pre_add = (p.res || p.up) && p.act == YL_ACT_NONE;
  const float lo = yl_act_lo(p.act), hi = yl_act_hi(p.act);
  const float dlo = yl_act_lo(p.dw_act), dhi = yl_act_hi(p.dw_act);
  const int dw_act = p.dw_act;

  for (int wi = 0; wi < nmine; ++wi) {
    const int item = slot + wi * per;
    const int g = item / bt;
    const int nt0 = g * (GW * NT);
    const int tile = band0 + item - g * bt;
    YlPix px[1];
    {
      px[0] = yl_pix(((size_t)tile * NW + wave) * 16 + pl, M, ohw, OW);
    }
    f32x4 acc[GW][1][NT];
#pragma unroll
    for (int gw = 0; gw < GW; ++gw)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[gw][0][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (pre_add) {
      const size_t obase = px[0].lin * p.N;
      size_t up_off = 0;
      if (p.up) {
        const int uy = (px[0].oy * p.UH) / p.OH, ux = (px[0].ox * p.UW) / p.OW;
        up_off = (((size_t)px[0].b * p.UH + uy) * p.UW + ux) * p.N;
      }
#pragma unroll
      for (int gw = 0; gw < GW; ++gw)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const int n = (nt0 + gw * NT + nt) * 16 + 4 * kq;
          if (n < p.N) {
            if (p.res) acc[gw][0][nt] = yl_ld4(p.res + obase + n);
            if (p.up) acc[gw][0][nt] += yl_ld4(p.up + up_off + n);
          }
        }
    }
    // nine tap pointers of the lane's pixel (the zero buffer where a tap falls outside the image, marked in `inb`)
    unsigned tp[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int iy = px[0].oy * DS - pad_t + tap / 3, ix = px[0].ox * DS - pad_l + tap % 3;
      const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
      tp[tap] = in ? (unsigned)((((px[0].b * H + iy) * W + ix) * Cin + 4 * kq) * (int)sizeof(yl_act_t)) : 0x80000000u;
    }
    auto fetch = [&](f32x4 (&dst)[9], int kb) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
#if YL_F16S
        dst[tap] = __builtin_convertvector(__builtin_bit_cast(yl_h16x4, __builtin_amdgcn_raw_buffer_load_b64(xrs, (int)tp[tap], kb * 32, 0)), f32x4);
#else
        dst[tap] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, (int)tp[tap], kb * 64, 0));
#endif
      }
    };
    f32x4 xt[9];
    fetch(xt, 0);
    for (int c = 0; c < NC; ++c, ++gchunk) {
      const int buf = (int)(gchunk & 1);
      if (gchunk + 1 < total_chunks) {
        if (c + 1 < NC) load_chunk(g, c + 1, buf ^ 1);
        else load_chunk((item + per) / bt, 0, buf ^ 1);
      }
      const f32x4* wb = wl + (size_t)buf * PCS * 64 + lane;
#pragma unroll
      for (int j = 0; j < S; ++j) {
        const int kb = c * S + j;
        if (kb < KB) {
          // depthwise result of block kb (tap order of yl_conv_dwh_kernel), then the next block's taps are requested
          const int cc = kb * 16 + 4 * kq;
          const int cs = cc < Cin ? cc : Cin - 4;
          const float* tapw = dwl + cs;
          f32x4 xq[1];
          xq[0] = yl_ld4(tapw + 9 * Cin);
#pragma unroll
          for (int tap = 0; tap < 9; ++tap) {
            const f32x4 w = yl_ld4(tapw + tap * Cin);
            xq[0].x = fmaf(xt[tap].x, w.x, xq[0].x); xq[0].y = fmaf(xt[tap].y, w.y, xq[0].y);
            xq[0].z = fmaf(xt[tap].z, w.z, xq[0].z); xq[0].w = fmaf(xt[tap].w, w.w, xq[0].w);
          }
          xq[0] = yl_sel4(cc < Cin, yl_actc(xq[0], dw_act, dlo, dhi));   // channel tail: zeros, not the next pixel's channels
          if (kb + 1 < KB) fetch(xt, kb + 1);
#pragma unroll
          for (int gw = 0; gw < GW; ++gw) {
            f32x4 wq[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) wq[nt] = wb[((j * GW + gw) * NT + nt) * 64];
            yl_mma_step<NT, 1>(wq, xq, acc[gw]);
          }
        }
      }
      __syncthreads();             // every wave is done with `buf`; the copies into the other buffer have landed
    }
#pragma unroll
    for (int gw = 0; gw < GW; ++gw) {
      if (!pre_add && (p.res || p.up || YL_SMOOTH(p.act))) yl_epi_generic<NT, 1>(p, acc[gw], px, nt0 + gw * NT, kq);
      else yl_epi_fast<NT, 1>(p, acc[gw], px, nt0 + gw * NT, kq, lo, hi, true);
    }
  }
}

// instantiated: (n-tiles per accumulator set, sets a wave holds, waves per workgroup)
#define YL_DWK_SHAPES(X) X(7, 1, 4) X(7, 3, 4) X(8, 1, 4) X(8, 2, 4)
static YlConvKernel dwk_kernel_of(int NT, int GW, int NW) {
#define YL_DWK_PICK(A, B, C) if (NT == A && GW == B && NW == C) return yl_conv_dwk_kernel<A, B, C>;
  YL_DWK_SHAPES(YL_DWK_PICK)
#undef YL_DWK_PICK
  return nullptr;
}

// yl_dwk_form has looked the instantiation up and held its LDS to the limit
static hipError_t dwk_go(const YlConvP& p0, hipStream_t st, int NT, int GW) {
  constexpr int NW = 4;
  const YlConvKernel kern = dwk_kernel_of(NT, GW, NW);
  if (!kern) return hipErrorNotSupported;
  YlConvP p = p0;
  p.ntiles = (int)(((long)p.M + 16 * NW - 1) / (16 * NW));
  const size_t lds = YlDwkLds(NT, GW, p.Cin).bytes;
  const int G = p.NTtot / (NT * GW);
  const int gx = yl_band_grid(yl_resident_blocks((const void*)kern, NW * 64, lds, 8), (long)p.ntiles * G);
  hipLaunchKernelGGL(kern, dim3(gx), dim3(NW * 64), lds, st, p);
  return hipGetLastError();
}

static YlConvKernel dwl_kernel_of(int NTT);
static hipError_t dwl_go(const YlConvP& p0, hipStream_t st, YlConvKernel kern);
static bool dwl_fits(int NTT, int KB);            // the window form's LDS within its limit

// depthwise 3x3 (stride 1 / 2) -> 1x1 with K >= 192, N % 4 == 0 and an n-tile count that is a multiple of 7 or 8,
// single problem.  Family 0 otherwise (yl_conv_mfma_kernel's streamed mode then runs the layer).
YlDwForm yl_dwk_form(const YlConvP& p) {
  const YlDwForm none = {YL_DWF_NONE, {0, 0, 0, 0, 0, 0}};
  if (p.dw_k != 3 || (p.N & 3) || p.dec_boxes || p.C1 > 0 || p.KB < 12 || p.NTtot <= 8) return none;
  if ((size_t)p.B * p.H * p.W * p.Cin * sizeof(yl_act_t) >= ((size_t)1 << 31)) return none;   // 32-bit byte offsets
  // developer A/B ("dev_select" bits 5-6): 2 = off, 1 = one n-group per item (depthwise recomputed per group),
  // 0 = default: a wave holds every n-group
  const int sel = YL_DEV_DWK(p.dev) == 2 ? 0 : (YL_DEV_DWK(p.dev) == 1 ? 1 : 2);
  if (sel == 0) return none;
  // window-in-LDS form (yl_conv_dwl_kernel): stride 1, pad 1, grids that fill the 8 x 8-pixel windows to >= 80 % (20 x 20: 69 %, slower than the tap-load kernel), >= 1.5 items
  // per CU (40 x 40 at B = 32: 0.116 -> 0.098 ms); "dev_select" bit 14 = off, bit 15 = on every grid (the bitwise test)
  // (the fp16-storage unit keeps the tap-load kernel: the windows are raw LDS-DMA copies of the tensor's bytes)
  if (!YL_F16S && !(p.dev & YL_DEV_DWL_OFF) && p.dw_stride == 1 && p.dw_pad_t == 1 && p.dw_pad_l == 1 && !p.scale &&
      (size_t)p.B * p.H * p.W * p.Cin < ((size_t)1 << 31)) {
    const long wins = (long)p.B * ((p.OW + 7) >> 3) * ((p.OH + 7) >> 3);
    if (((long)p.B * p.OH * p.OW * 10 >= wins * 64 * 8 && wins >= 3 * YL_NUM_CU) || (p.dev & YL_DEV_DWL_ALL)) {
      // (a window form beyond its LDS limit leaves the layer to the kernels behind this family, not to the tap-load form)
      if (dwl_kernel_of(p.NTtot)) return dwl_fits(p.NTtot, p.KB) ? YlDwForm{YL_DWF_DWL, {p.NTtot, 0, 0, 0, 0, 0}} : none;
    }
  }
  int NT = 0, GW = 1;
  if (p.NTtot == 21) { NT = 7; GW = sel == 2 ? 3 : 1; }
  else if (p.NTtot == 16) { NT = 8; GW = sel == 2 ? 2 : 1; }
  else if (p.NTtot % 7 == 0) NT = 7;
  else if (p.NTtot % 8 == 0) NT = 8;
  if (!NT || !dwk_kernel_of(NT, GW, 4) || YlDwkLds(NT, GW, p.Cin).bytes > YlDwkLds::LIMIT) return none;
  return {YL_DWF_DWK, {NT, GW, 4, 0, 0, 0}};
}

hipError_t yl_launch_conv_dwk(const YlConvP& p, const YlDwForm& f, hipStream_t st) {
  if (f.family == YL_DWF_DWL) return dwl_go(p, st, dwl_kernel_of(f.a[0]));
  if (f.family == YL_DWF_DWK) return dwk_go(p, st, f.a[0], f.a[1]);
  return hipErrorNotSupported;
}

// ------------------------------------------------------------------------------------------------
// Depthwise 3x3 (stride 1, pad 1) -> wide 1x1 with the INPUT WINDOW IN LDS (round 5): the layers of yl_conv_dwk_kernel
// on grids that fill 8 x 8-pixel windows.  yl_conv_dwk_kernel fetches nine float4 taps per lane and k-block straight
// from L1/L2 with the MFMA lane layout (lane = channel group * 16 + pixel): the four lanes of a quad sit on four
// different pixels, i.e. four cache lines, so a tap load keeps the texture addresser busy for 64 cycles and the nine of
// them for more cycles than the 64 MFMAs they feed (244 -> 244 @80x80: 55 TFLOP/s).  Here, with the machinery of
// yl_conv_wino2_kernel:
//   window   a workgroup item is TWO 8 x 8-pixel output windows (8 waves x one 4 x 4-pixel MFMA m-tile); their 10 x 10-pixel
//            input windows (64 B per pixel and k-block) land in LDS by asynchronous LDS-DMA copies whose quads read the 64
//            contiguous bytes of ONE pixel (2 copy instructions per wave and k-block; every input pixel once per item instead
//            of once per tap that touches it), double-buffered, requested a k-block ahead;
//   B        the lane's nine taps by ds_read_b128 from the window (slot = 4 P + (kq ^ 2 ((P >> 2) & 1)), P = y * 12 + x: a
//            lane group holds pixel rows {0,3} with one channel group and {1,2} with its neighbour -- conflict-free, see
//            yl_conv_wino2_kernel), tap weights + bias from LDS, the fmaf chain and activation of yl_conv_dwk_kernel;
//   A        the 1x1 weights of a k-block (all n-tiles: a wave accumulates every output channel of its 16 pixels, as in
//            yl_conv_dwk_kernel's GW = all form) shared by the 8 waves through LDS, TRIPLE-buffered;
//   barrier  ONE per k-block, in the middle of its MFMAs: behind it window(kb + 1) and weights(kb + 1) are complete, the
//            wave requests window(kb + 2) / weights(kb + 2) into the buffers of blocks kb / kb - 1, builds B(kb + 1) and goes
//            on with the second half of block kb's MFMAs -- the MFMA stream runs on across k-blocks.
// Same tap order, k order and epilogues as yl_conv_dwk_kernel: BIT-IDENTICAL to it ("dev_select" bit 14 keeps the old kernel).
// dynamic LDS of yl_conv_dwl_kernel (offsets in float4s): [3][NTP][64] weight pieces | [2 buffers][2 windows][RM] window slots |
// (floats) [KB][10][16]: taps 0..8 + bias of a k-block's channels (zeros beyond Cin)
struct YlDwlLds {
  static constexpr size_t LIMIT = 128 * 1024;
  static constexpr int RP = 12, RM = 512;                        // window row pitch in pixels, 16-byte slots per window
  int NTP;                                                       // weight pieces per buffer (8 waves x NTP / 8 copies)
  size_t Rl, dwl, bytes;
  constexpr __host__ __device__ YlDwlLds(int NTT, int KB)
      : NTP((NTT + 7) & ~7), Rl((size_t)3 * NTP * 64), dwl(Rl + 2 * 2 * RM), bytes(dwl * 16 + (size_t)KB * 160 * 4) {}
};

template <int NTT>
__global__ __launch_bounds__(512, 2) void yl_conv_dwl_kernel(YlConvP p) {
  constexpr YlDwlLds L(NTT, 0);                                  // (the offsets do not depend on KB)
  constexpr int RP = YlDwlLds::RP, RM = YlDwlLds::RM, NTP = L.NTP;
  // MFMA groups of <= 4 n-tiles, an even number of them (their A fragments alternate between two register sets across
  // k-blocks): 16 = 4 x 4, 21 = 3 x 4 + 3 x 3
  constexpr int NCH = NTT == 16 ? 4 : 6;
  static_assert(NTT == 16 || NTT == 21, "n-tile groups");
  auto c0of = [](int c) { return NTT == 16 ? 4 * c : (c <= 3 ? 4 * c : 12 + 3 * (c - 3)); };
  extern __shared__ __attribute__((aligned(16))) float yl_clds[];
  f32x4* const Wl = reinterpret_cast<f32x4*>(yl_clds);
  f32x4* const Rl = Wl + L.Rl;
  float* const dwl = reinterpret_cast<float*>(Wl + L.dwl);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, pl = lane & 15;
  const int KB = p.KB, NTtot = p.NTtot, Cin = p.Cin, H = p.H, W = p.W, OH = p.OH, OW = p.OW;
  const int WX = (OW + 7) >> 3, WY = (OH + 7) >> 3;
  const int wimg = WX * WY;
  const long WTOT = (long)p.B * wimg;                            // windows
  const yl_act_t* const xin = p.x;
  const int wgmax = KB * NTtot - 1;                              // last weight piece
  const int bx = blockIdx.x, gx = gridDim.x;                     // gx % 8 == 0
  const YlBandSplit ws = yl_band_split(bx, gx, p.ntiles);       // XCD bands, strided items (one n-group)
  const int per = ws.per, slot = ws.slot, band0 = ws.band0, band1 = ws.band1;
  // copy role of the lane: slot rs = wave * 64 + lane of both windows
  const int rs = wave * 64 + lane;
  const int rP = rs >> 2, rkq = (rs & 3) ^ (((rP >> 2) & 1) << 1);
  const int ry = rP / RP, rx = rP - ry * RP;
  const bool rpix = ry < 10 && rx < 10;
  // compute role: window wsel, 4 x 4-pixel block (qy, qx) of it, pixel (sy, sx) of the block
  const int wsel = wave >> 2, qy = (wave >> 1) & 1, qx = wave & 1;
  const int sy = pl >> 2, sx = pl & 3;
  int ts[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int P = (4 * qy + sy + tap / 3) * RP + 4 * qx + sx + tap % 3;
    ts[tap] = wsel * RM + 4 * P + (kq ^ (((P >> 2) & 1) << 1));
  }
  // the tap image k-block-major, so that a lane's ten tap / bias reads of a block are ONE address + immediates
  for (int i = tid; i < KB * 160; i += 512) {
    const int kb = i / 160, r = i - kb * 160, t = r >> 4, ch = kb * 16 + (r & 15);
    dwl[i] = ch < Cin ? (t < 9 ? p.dw_w[(size_t)t * Cin + ch] : (p.dw_b ? p.dw_b[ch] : 0.0f)) : 0.0f;
  }
  // Operand streams through raw buffer descriptors (as yl_conv_wino2_kernel, round 6): the lane's part of an address is a 32-bit
  // byte offset fixed for the item (window) or the launch (weights), the k-block part is scalar; lanes outside the image carry an
  // out-of-range offset and the copy writes zeros.  The channel tail of the last k-block copies the next pixel's first channels
  // (the next image's behind an image's last pixel); make_b hands zeros to the MFMA for those lanes (0 x inf / NaN would be NaN).
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<yl_act_t*>(xin), 0, (int)((long)p.B * H * W * Cin * (long)sizeof(yl_act_t)), 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(p.wp), 0, (int)((long)KB * NTtot * 1024), 0x00020000);
  constexpr unsigned OOB = 0x80000000u;
  const int lane16 = lane * 16;
  const int sh = KB & 1;                                         // window(kb) lives in buffer (kb + KB) & 1: see yl_conv_wino2_kernel
  const bool pre_add = (p.res || p.up) && p.act == YL_ACT_NONE;
  const float lo = yl_act_lo(p.act), hi = yl_act_hi(p.act);
  const float dlo = yl_act_lo(p.dw_act), dhi = yl_act_hi(p.dw_act);
  const int dw_act = p.dw_act;

  unsigned voff[2];
  auto issue_win = [&](int kb, int buf) {
#pragma unroll
    for (int w2 = 0; w2 < 2; ++w2)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(Rl + (buf * 2 + w2) * RM + wave * 64), 16,
                                               (int)voff[w2], kb * 16 * (int)sizeof(yl_act_t), 0, 0);
  };
  auto issue_wts = [&](int kb, int wb) {
#pragma unroll
    for (int j = 0; j < NTP / 8; ++j) {
      const int i = wave + 8 * j;                                // (pieces NTT..NTP-1: pad, any valid source)
      int src = kb * NTtot + (i < NTT ? i : 0);
      src = src < wgmax ? src : wgmax;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (__attribute__((address_space(3))) void*)(Wl + ((size_t)wb * NTP + i) * 64), 16,
                                               lane16, src * 1024, 0, 0);
    }
  };
  auto make_b = [&](int kb, int buf) {
    const float* tapw = dwl + kb * 160 + 4 * kq;
    const f32x4* const wb = Rl + buf * 2 * RM;
    f32x4 xq = yl_ld4(tapw + 9 * 16);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const f32x4 x = wb[ts[tap]];
      const f32x4 w = yl_ld4(tapw + tap * 16);
      xq.x = fmaf(x.x, w.x, xq.x); xq.y = fmaf(x.y, w.y, xq.y);
      xq.z = fmaf(x.z, w.z, xq.z); xq.w = fmaf(x.w, w.w, xq.w);
    }
    return yl_sel4(kb * 16 + 4 * kq < p.Cin, yl_actc(xq, dw_act, dlo, dhi));   // channel tail: zeros (see the window copy)
  };

  for (int item = band0 + slot; item < band1; item += per) {
    // the two windows of the item, the lane's output pixel, the lane's copy sources
    YlPix px[1];
    {
      const long wi = (long)item * 2 + wsel;
      const bool wv = wi < WTOT;
      const long wc = wv ? wi : WTOT - 1;
      const int b = (int)(wc / wimg);
      const int r = (int)(wc - (long)b * wimg);
      const int wy = r / WX, wx = r - wy * WX;
      int oy = 8 * wy + 4 * qy + sy, ox = 8 * wx + 4 * qx + sx;
      px[0].valid = wv && oy < OH && ox < OW;
      if (oy >= OH) oy = OH - 1;
      if (ox >= OW) ox = OW - 1;
      px[0].b = b; px[0].oy = oy; px[0].ox = ox;
      px[0].lin = ((size_t)b * OH + oy) * OW + ox;
    }
#pragma unroll
    for (int w2 = 0; w2 < 2; ++w2) {
      const long wi = (long)item * 2 + w2;
      const int b = (int)(wi / wimg);
      const int r = (int)(wi - (long)b * wimg);
      const int wy = r / WX, wx = r - wy * WX;
      const int gy = 8 * wy - 1 + ry, gxx = 8 * wx - 1 + rx;
      const bool in = rpix && wi < WTOT && gy >= 0 && gy < H && gxx >= 0 && gxx < W;
      voff[w2] = in ? (unsigned)((((b * H + gy) * W + gxx) * Cin + 4 * rkq) * (int)sizeof(yl_act_t)) : OOB;
    }
    f32x4 acc[1][NTT];
#pragma unroll
    for (int nt = 0; nt < NTT; ++nt) acc[0][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (pre_add) {
      const size_t obase = px[0].lin * p.N;
      size_t up_off = 0;
      if (p.up) {
        const int uy = (px[0].oy * p.UH) / p.OH, ux = (px[0].ox * p.UW) / p.OW;
        up_off = (((size_t)px[0].b * p.UH + uy) * p.UW + ux) * p.N;
      }
#pragma unroll
      for (int nt = 0; nt < NTT; ++nt) {
        const int n = nt * 16 + 4 * kq;
        if (n < p.N) {
          if (p.res) acc[0][nt] = yl_ld4(p.res + obase + n);
          if (p.up) acc[0][nt] += yl_ld4(p.up + up_off + n);
        }
      }
    }
    __syncthreads();                                              // the previous item's last weight reads are done
    issue_win(0, sh); issue_wts(0, 0);
    issue_win(1, sh ^ 1); issue_wts(1, 1);                        // (KB >= 12: the launcher)
    __builtin_amdgcn_s_waitcnt(0x0F70);                           // vmcnt(0)
    __syncthreads();
    f32x4 xq[1];
    xq[0] = make_b(0, sh);
    int wb = 0;
    f32x4 wq[2][4];                                               // A fragments of the current / the next MFMA group
    auto read_a = [&](int wbuf, int c, f32x4 (&dst)[4]) {
      const f32x4* const wl = Wl + (size_t)wbuf * NTP * 64 + lane;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (c0of(c) + i < c0of(c + 1)) dst[i] = wl[(c0of(c) + i) * 64];
    };
    read_a(0, 0, wq[0]);
    // One k-block.  Top: the barrier behind which window(kb + 1) / weights(kb + 1) are complete (requested a k-block ago)
    // and nobody reads window(kb) / weights(kb - 1) any more -- their buffers take the requests of block kb + 2.  Then the
    // MFMA groups; in front of group c the wave issues the LDS reads of what it needs one group later -- the A fragments of
    // group c + 1 (of block kb + 1's group 0 at the end: complete since this block's barrier) and three taps + tap weights
    // of B(kb + 1) -- and behind the group's MFMAs their arithmetic: no LDS round trip is waited for, the tap fma chain sits
    // between MFMA groups (a first version built B(kb + 1) in one piece between two halves of the block's MFMAs: both waves
    // of a SIMD waited there for 19 LDS reads with nothing to issue).  MODE 0 any block, 1 the second-to-last (no
    // requests), 2 the last (no next B): branch-free bodies.
    auto kblock = [&](int kb, auto par, auto mode) {
      constexpr int PAR = decltype(par)::value;                   // buffer of window(kb) (compile-time: LDS offsets are immediates)
      constexpr int MODE = decltype(mode)::value;
      const int wb1 = wb == 2 ? 0 : wb + 1;
      // the wave's own copies first: the compiler's wait-count pass does not carry the LDS-DMA requests of the previous
      // iteration across the loop's back edge (the barrier here came out with lgkmcnt(0) only, and two runs of edge_m at
      // B = 32 differed in a few bits)
      __builtin_amdgcn_s_waitcnt(0x0F70);                         // vmcnt(0)
      __syncthreads();
      if (MODE == 0) {
        issue_win(kb + 2, PAR);
        issue_wts(kb + 2, wb >= 1 ? wb - 1 : 2);                  // (wb + 2) % 3
      }
      const float* const tapw = dwl + (kb + 1) * 160 + 4 * kq;
      const f32x4* const win = Rl + (PAR ^ 1) * 2 * RM;
      f32x4 xn = xq[0];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        f32x4 tx[3], tw[3];
        if (c + 1 < NCH) read_a(wb, c + 1, wq[(c + 1) & 1]);
        else if (MODE < 2) read_a(wb1, 0, wq[0]);
        if (MODE < 2 && c < 3) {
          if (c == 0) xn = yl_ld4(tapw + 9 * 16);
#pragma unroll
          for (int t = 0; t < 3; ++t) { tx[t] = win[ts[3 * c + t]]; tw[t] = yl_ld4(tapw + (3 * c + t) * 16); }
        }
        __builtin_amdgcn_sched_barrier(0);
#if YL_BF16
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (c0of(c) + i < c0of(c + 1)) {
            const f32x4 w1[1] = {wq[c & 1][i]};
            yl_mma_step<1, 1>(w1, xq, *reinterpret_cast<f32x4 (*)[1][1]>(&acc[0][c0of(c) + i]));
          }
#else
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (c0of(c) + i < c0of(c + 1))
              acc[0][c0of(c) + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wq[c & 1][i][st], xq[0][st], acc[0][c0of(c) + i], 0, 0, 0);
#endif
        __builtin_amdgcn_sched_barrier(0);                        // (else the fma chain moves up to the group's first MFMA and waits there
        if (MODE < 2 && c < 3) {                                  //  for the reads issued a moment before)
#pragma unroll
          for (int t = 0; t < 3; ++t) xn = yl_pk_fma4(tx[t], tw[t], xn);     // two v_pk_fma_f32 by name: the same fma per component
                                                                             // (pinned packed form: +0.2 %, profiles/r06_pinned_pk_chains_ab.txt)
          if (c == 2) xn = yl_sel4((kb + 1) * 16 + 4 * kq < p.Cin, yl_actc(xn, dw_act, dlo, dhi));
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      xq[0] = xn;
      wb = wb1;
    };
    {
      using I0 = std::integral_constant<int, 0>;
      using I1 = std::integral_constant<int, 1>;
      using I2 = std::integral_constant<int, 2>;
      int kb = 0;
      if (sh) { kblock(0, I1{}, I0{}); kb = 1; }                  // odd KB: block 0 on its own, out of buffer 1
      for (; kb + 3 < KB; kb += 2) {
        kblock(kb, I0{}, I0{});
        kblock(kb + 1, I1{}, I0{});
      }
      kblock(KB - 2, I0{}, I1{});
      kblock(KB - 1, I1{}, I2{});
    }
    if (!pre_add && (p.res || p.up || YL_SMOOTH(p.act))) yl_epi_generic<NTT, 1>(p, acc, px, 0, kq);
    else yl_epi_fast<NTT, 1>(p, acc, px, 0, kq, lo, hi, true);
  }
}

// instantiated: n-tiles of the layer (244 / 328 output channels)
#define YL_DWL_SHAPES(X) X(16) X(21)
static YlConvKernel dwl_kernel_of(int NTT) {
#define YL_DWL_PICK(A) if (NTT == A) return yl_conv_dwl_kernel<A>;
  YL_DWL_SHAPES(YL_DWL_PICK)
#undef YL_DWL_PICK
  return nullptr;
}

static bool dwl_fits(int NTT, int KB) { return YlDwlLds(NTT, KB).bytes <= YlDwlLds::LIMIT; }

// yl_dwk_form has held the LDS to the limit and the tensor to 32-bit byte offsets
static hipError_t dwl_go(const YlConvP& p0, hipStream_t st, YlConvKernel kern) {
  YlConvP p = p0;
  const long WTOT = (long)p.B * ((p.OW + 7) >> 3) * ((p.OH + 7) >> 3);
  p.ntiles = (int)((WTOT + 1) / 2);
  const size_t lds = YlDwlLds(p.NTtot, p.KB).bytes;
  const int gx = yl_band_grid(yl_resident_blocks((const void*)kern, 512, lds, 8), p.ntiles);
  hipLaunchKernelGGL(kern, dim3(gx), dim3(512), lds, st, p);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Depthwise DK x DK (stride DS) -> 1x1 with MANY channels on the depthwise side (round 5): the `conv_dw` -> `conv_pwl` halves of
// timm's EfficientNet-Lite inverted-residual blocks behind model_v2.py:94-100 (yololite_m = tf_efficientnet_lite2 stages 4-6:
// 528 / 720 / 1248 channels, 5x5 stride 1 and 2, 3x3 at 1248 -> 352).  Neither fused kernel
// covered them -- yl_conv_dwt_kernel keeps the taps of ALL channels in LDS (26 x 1248 floats = 130 KB) and reads its 1x1
// weights per wave from L1/L2 (<= 6 n-tiles), yl_conv_dwk_kernel fetches nine taps per lane from L1/L2 (25 at 5x5: bound by
// the vector-memory path) -- so the depthwise conv ran as its own launch (yl_dw_tile_kernel: ten launches, ~0.8 ms of the
// 12 ms step at B = 32, the expanded tensor written and re-read).  This kernel joins the two recipes:
//   from yl_conv_dwk_kernel  the 1x1 weight stream double-buffered through LDS in chunks of S k-steps shared by the NW waves
//                            of a workgroup (asynchronous copies, one barrier per chunk), a wave holds EVERY n-tile of its
//                            pixels (GW x NT accumulator sets), items dealt in XCD bands;
//   from yl_conv_dwt_kernel  wave = one 4x4-pixel tile, the (3 DS + DK)^2 halo patch of a 16-channel block staged through the
//                            wave's private LDS region (4 / 8 / 3 coalesced float4 loads per lane, requested one k-step
//                            ahead), B = act(bias + sum_taps w * x) from conflict-free ds_read_b128;
//   new                      the tap weights + depthwise bias of a k-step (26 x 16 floats) ride in the weight chunk: LDS holds
//                            2 x S k-steps of them, whatever the channel count.
// Same tap order (dy, dx), k order and epilogues as yl_dw_tile_kernel + yl_conv_pws_kernel: the depthwise value of a channel is
// the same fmaf chain, the 1x1 sums its k blocks in ascending order -> bit-identical to the two launches it replaces.
// dynamic LDS of yl_conv_dws_kernel (offsets in float4s): [2][S][NTW][64] weight chunks | [2][S][TQP] taps: row t = tap t (t = TAPS:
// bias), 4 quads | (floats) one halo patch per wave
struct YlDwsLds {
  static constexpr size_t LIMIT = 96 * 1024;
  int S;                                                             // k-steps per chunk (= per barrier)
  int TQ, TQP;                                                       // float4s of taps + bias per k-step, padded to whole 64-lane copies
  int HP, PITCHF;                                                    // halo patch rows = columns, row pitch in floats (see yl_conv_dwh_kernel)
  size_t tl, halo, bytes;
  constexpr __host__ __device__ YlDwsLds(int NTW, int DK, int DS, int NW)
      : S(NTW <= 8 ? 2 : 1), TQ((DK * DK + 1) * 4), TQP(((TQ + 63) / 64) * 64), HP(3 * DS + DK), PITCHF(((HP * 16 + 7) / 64) * 64 + 56),
        tl((size_t)2 * S * NTW * 64), halo(tl + (size_t)2 * S * TQP), bytes(halo * 16 + (size_t)NW * HP * PITCHF * 4) {}
};

template <int NT, int GW, int DK, int DS, int NW>
__global__ __launch_bounds__(NW * 64, 2) void yl_conv_dws_kernel(YlConvP p) {
  constexpr int NTW = NT * GW;                                        // n-tiles a wave accumulates (all of the layer's)
  constexpr YlDwsLds L(NTW, DK, DS, NW);
  constexpr int S = L.S, TAPS = DK * DK, TQ = L.TQ, TQP = L.TQP, HP = L.HP, PITCHF = L.PITCHF;
  constexpr int HF4 = HP * HP * 4, NSLOT = (HF4 + 63) / 64;
  constexpr int PCS = S * NTW + S * (TQP / 64);                      // 1 KiB pieces per chunk: weights, then taps
  extern __shared__ __attribute__((aligned(16))) float yl_clds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, pl = lane & 15;
  const int KB = p.KB, NTtot = p.NTtot, Cin = p.Cin, H = p.H, W = p.W, OH = p.OH, OW = p.OW;
  const yl_act_t* const xin = p.x;
  // staging loads through a raw buffer descriptor (round 6, as yl_conv_wino2_kernel): a 32-bit byte offset per slot fixed for the
  // item + a scalar k-block offset -- the loop carried 8 64-bit adds and 16 selects per k-block for its four loads; slots outside
  // the image carry an out-of-range offset (the load returns zeros).  The channel tail of the last k-block stages the next
  // pixel's channels; its depthwise results are replaced by zeros before the 1x1 (0 x inf / NaN would be NaN)
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<yl_act_t*>(xin), 0, (int)((long)p.B * H * W * Cin * (long)sizeof(yl_act_t)), 0x00020000);
  constexpr unsigned OOB = 0x80000000u;
  f32x4* wl = reinterpret_cast<f32x4*>(yl_clds);
  f32x4* tl = wl + L.tl;
  float* halo = reinterpret_cast<float*>(wl + L.halo) + wave * (HP * PITCHF);
  const f32x4* wg = reinterpret_cast<const f32x4*>(p.wp);
  const int NC = (KB + S - 1) / S;
  const int twn = OW >> 2, tiles_img = twn * (OH >> 2);
  const long ntiles4 = (long)p.B * tiles_img;                        // 4x4 tiles; p.ntiles = items of NW tiles
  const int bx = blockIdx.x, gx = gridDim.x;                         // gx % 8 == 0
  const YlBandSplit ws = yl_band_split(bx, gx, p.ntiles);           // XCD bands, strided items (one n-group)
  const int per = ws.per, slot = ws.slot, band0 = ws.band0, nmine = ws.nmine;
  const long total_chunks = (long)nmine * NC;
  auto load_chunk = [&](int c, int buf) {
    for (int i = wave; i < PCS; i += NW) {
      if (i < S * NTW) {
        const int j = i / NTW, nt = i - j * NTW;
        const int kb = c * S + j;
        if (kb < KB) yl_glds16(wg + ((size_t)kb * NTtot + (nt < NTtot ? nt : NTtot - 1)) * 64 + lane, wl + ((size_t)buf * S * NTW + i) * 64);
      } else {
        const int i2 = i - S * NTW;
        const int j = i2 / (TQP / 64), r = i2 - j * (TQP / 64);
        const int kb = c * S + j;
        const int idx = r * 64 + lane, t = idx >> 2, ch = kb * 16 + (idx & 3) * 4;
        if (kb < KB && idx < TQ) {
          const float* src = (ch < Cin) ? (t < TAPS ? p.dw_w + (size_t)t * Cin + ch : (p.dw_b ? p.dw_b + ch : reinterpret_cast<const float*>(p.zeros))) : reinterpret_cast<const float*>(p.zeros);
          yl_glds16(src, tl + ((size_t)(buf * S + j) * TQP + r * 64));
        }
      }
    }
  };
  if (total_chunks > 0) load_chunk(0, 0);
  long gchunk = 0;
  // staging slots of this lane: halo pixel / channel quad -> LDS offset
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
  __syncthreads();
  const bool pre_add = (p.res || p.up) && p.act == YL_ACT_NONE;
  const float lo = yl_act_lo(p.act), hi = yl_act_hi(p.act);
  const float dlo = yl_act_lo(p.dw_act), dhi = yl_act_hi(p.dw_act);
  const int dw_act = p.dw_act;
  const int rbase = ((pl >> 2) * DS) * PITCHF + ((pl & 3) * DS) * 16 + 4 * kq;

  for (int wi = 0; wi < nmine; ++wi) {
    const int item = band0 + slot + wi * per;
    long t4 = (long)item * NW + wave;
    const bool tvalid = t4 < ntiles4;
    if (!tvalid) t4 = ntiles4 - 1;
    const int b = (int)(t4 / tiles_img);
    const int trem = (int)(t4 - (long)b * tiles_img);
    const int tyi = trem / twn, txi = trem - tyi * twn;
    YlPix px[1];
    px[0].b = b; px[0].oy = 4 * tyi + (pl >> 2); px[0].ox = 4 * txi + (pl & 3); px[0].valid = tvalid;
    px[0].lin = ((size_t)b * OH + px[0].oy) * OW + px[0].ox;
    f32x4 acc[GW][1][NT];
#pragma unroll
    for (int gw = 0; gw < GW; ++gw)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[gw][0][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (pre_add) {
      const size_t obase = px[0].lin * p.N;
      size_t up_off = 0;
      if (p.up) {
        const int uy = (px[0].oy * p.UH) / p.OH, ux = (px[0].ox * p.UW) / p.OW;
        up_off = (((size_t)px[0].b * p.UH + uy) * p.UW + ux) * p.N;
      }
#pragma unroll
      for (int gw = 0; gw < GW; ++gw)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const int n = (gw * NT + nt) * 16 + 4 * kq;
          if (n < p.N) {
            if (p.res) acc[gw][0][nt] = yl_ld4(p.res + obase + n);
            if (p.up) acc[gw][0][nt] += yl_ld4(p.up + up_off + n);
          }
        }
    }
    unsigned goff[NSLOT];
    {
      const int iy0 = 4 * tyi * DS - p.dw_pad_t, ix0 = 4 * txi * DS - p.dw_pad_l;
#pragma unroll
      for (int j = 0; j < NSLOT; ++j) {
        const int e = j * 64 + lane;
        const int hp = (e < HF4 ? e : 0) >> 2;
        const int hr = hp / HP, hc = hp - hr * HP;
        const int iy = iy0 + hr, ix = ix0 + hc;
        const bool in = e < HF4 && iy >= 0 && iy < H && ix >= 0 && ix < W;
        goff[j] = in ? (unsigned)((((b * H + iy) * W + ix) * Cin + (lane & 3) * 4) * (int)sizeof(yl_act_t)) : OOB;
      }
    }
    auto stage_load = [&](int kb, f32x4 (&r)[NSLOT]) {
#pragma unroll
      for (int j = 0; j < NSLOT; ++j) {
#if YL_F16S
        r[j] = __builtin_convertvector(__builtin_bit_cast(yl_h16x4, __builtin_amdgcn_raw_buffer_load_b64(xrs, (int)goff[j], kb * 32, 0)), f32x4);
#else
        r[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, (int)goff[j], kb * 64, 0));
#endif
      }
    };
    auto stage_store = [&](const f32x4 (&r)[NSLOT]) {
#pragma unroll
      for (int j = 0; j < NSLOT; ++j)
        if (s_ok[j]) *reinterpret_cast<f32x4*>(halo + s_lo[j]) = r[j];
    };
    f32x4 stg[NSLOT];
    stage_load(0, stg);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");          // previous item's tap reads are complete
    stage_store(stg);
    for (int c = 0; c < NC; ++c, ++gchunk) {
      const int buf = (int)(gchunk & 1);
      if (gchunk + 1 < total_chunks) load_chunk(c + 1 < NC ? c + 1 : 0, buf ^ 1);
#pragma unroll
      for (int j = 0; j < S; ++j) {
        const int kb = c * S + j;
        if (kb < KB) {
          const bool more = kb + 1 < KB;
          if (more) stage_load(kb + 1, stg);
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");    // halo writes (all lanes) -> tap reads
          const f32x4* tw = tl + (size_t)(buf * S + j) * TQP + kq;
          f32x4 xq[1];
          xq[0] = tw[TAPS * 4];
#pragma unroll 1
          for (int dy = 0; dy < DK; ++dy) {                          // one tap row at a time bounds the register footprint
#pragma unroll
            for (int dx = 0; dx < DK; ++dx) {
              const f32x4 w = tw[(dy * DK + dx) * 4];
              const f32x4 v = *reinterpret_cast<const f32x4*>(halo + rbase + dy * PITCHF + dx * 16);
              xq[0].x = fmaf(v.x, w.x, xq[0].x); xq[0].y = fmaf(v.y, w.y, xq[0].y);
              xq[0].z = fmaf(v.z, w.z, xq[0].z); xq[0].w = fmaf(v.w, w.w, xq[0].w);
            }
          }
          // channel tail (c >= Cin): the staged halo holds the next pixel's channels there -- zeros into the MFMA (0 x inf / NaN
          // would be NaN against the zero 1x1 weights of those k slots)
          xq[0] = yl_sel4(kb * 16 + 4 * kq < Cin, yl_actc(xq[0], dw_act, dlo, dhi));
          const f32x4* wb = wl + (size_t)(buf * S + j) * NTW * 64 + lane;
#pragma unroll
          for (int gw = 0; gw < GW; ++gw) {
            f32x4 wq[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) wq[nt] = wb[(gw * NT + nt) * 64];
            yl_mma_step<NT, 1>(wq, xq, acc[gw]);
          }
          if (more) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // this block's tap reads are complete
            stage_store(stg);
          }
        }
      }
      __syncthreads();             // every wave is done with `buf`; the copies into the other buffer have landed
    }
#pragma unroll
    for (int gw = 0; gw < GW; ++gw) {
      if (!pre_add && (p.res || p.up || YL_SMOOTH(p.act))) yl_epi_generic<NT, 1>(p, acc[gw], px, gw * NT, kq);
      else yl_epi_fast<NT, 1>(p, acc[gw], px, gw * NT, kq, lo, hi, true);
    }
  }
}

template <int NT, int GW, int DK, int DS, int NW>
static hipError_t dws_go(const YlConvP& p0, hipStream_t st) {
  YlConvP p = p0;
  const long t4 = (long)p.B * (p.OH >> 2) * (p.OW >> 2);
  p.ntiles = (int)((t4 + NW - 1) / NW);
  constexpr size_t lds = YlDwsLds(NT * GW, DK, DS, NW).bytes;
  static_assert(lds <= YlDwsLds::LIMIT, "yl_conv_dws_kernel: LDS of an instantiated shape");
  const int gx = yl_band_grid(yl_resident_blocks((const void*)yl_conv_dws_kernel<NT, GW, DK, DS, NW>, NW * 64, lds, 8), p.ntiles);
  hipLaunchKernelGGL((yl_conv_dws_kernel<NT, GW, DK, DS, NW>), dim3(gx), dim3(NW * 64), lds, st, p);
  return hipGetLastError();
}

// instantiated: (n-tiles per accumulator set, sets, depthwise k, stride): 8 n-tiles (N <= 128), 13 (N <= 208), 2 x 11 (N <= 352).
// Measured on yololite_m B = 32 (eager, ms; two launches -> this kernel): 528 -> 120 5x5 @40x40 0.191 -> 0.160, 720 -> 120 0.246 ->
// 0.217, 720 -> 208 5x5 s2 0.131 -> 0.127, 1248 -> 208 5x5 @20x20 0.168 -> 0.164, 1248 -> 352 3x3 (22 n-tiles) 0.188 -> 0.228.
// 45-50 TFLOP/s: the 25 tap + 25 tap-weight ds_read_b128 per k-step make it LDS-bound at two waves per SIMD (S = 1, 8 waves per
// workgroup and a fully unrolled tap loop were measured: 0.220 / 0.210 (but 0.233 at 13 n-tiles) / 0.226 against 0.217).  What
// counts is the step with two batches in flight, where launches and HBM traffic are the currency: 2.58 k images/s with the
// eleven stand-alone depthwise launches, 2.65 k with ten of them fused, 2.72 k with all eleven (the 22 n-tile layer included,
// although it is slower in isolation) -- 2.9 GB of expanded-tensor traffic fewer per step.
#define YL_DWS_SHAPES(X) X(8, 1, 5, 1) X(8, 1, 5, 2) X(13, 1, 5, 1) X(13, 1, 5, 2) X(8, 1, 3, 1) X(13, 1, 3, 1) X(11, 2, 3, 1) X(11, 2, 5, 1)

#if !YL_BF16
// depthwise -> 1x1 layers this kernel takes: >= 12 k-blocks (below that yl_conv_dwt / dwh / dwk_kernel and the 32 KB tap
// image are the better fit), 4x4-tileable output, N % 4 == 0, one of the instantiated (n-tiles, k, stride) shapes
bool yl_dws_supported(int cin, int n, int dk, int ds, int oh, int ow) {
  const int kb = (cin + 15) / 16, ntt = (n + 15) / 16;
  if (kb < 12 || (n & 3) || (cin & 3) || (oh & 3) || (ow & 3) || oh < 4 || ow < 4) return false;
#define YL_DWS_CHECK(A, G, K, S_) if (dk == K && ds == S_ && ntt <= A * G && ntt > (A * G == 8 ? 6 : A * G == 13 ? 8 : 13)) return true;
  YL_DWS_SHAPES(YL_DWS_CHECK)
#undef YL_DWS_CHECK
  return false;
}
#endif

// family 0: not a layer of this kernel (yl_dws_supported), or a configuration or tensor size it does not take
YlDwForm yl_dws_form(const YlConvP& p) {
  const YlDwForm none = {YL_DWF_NONE, {0, 0, 0, 0, 0, 0}};
  if ((size_t)p.B * p.H * p.W * p.Cin * sizeof(yl_act_t) >= ((size_t)1 << 31)) return none;   // 32-bit byte offsets
  if (p.dw_k == 0 || p.k != 1 || p.stride != 1 || p.dec_boxes || p.C1 > 0 || p.scale || p.in_shift || p.w3p ||
      !yl_dws_supported(p.Cin, p.N, p.dw_k, p.dw_stride, p.OH, p.OW) ||
      (size_t)p.B * p.H * p.W * p.Cin >= ((size_t)1 << 40))
    return none;
  const int ntt = p.NTtot;
#define YL_DWS_IS(A, G, K, S_) \
  if (p.dw_k == K && p.dw_stride == S_ && ntt <= A * G && ntt > (A * G == 8 ? 6 : A * G == 13 ? 8 : 13)) return {YL_DWF_DWS, {A, G, K, S_, 4, 0}};
  YL_DWS_SHAPES(YL_DWS_IS)
#undef YL_DWS_IS
  return none;
}

hipError_t yl_launch_conv_dws(const YlConvP& p, const YlDwForm& f, hipStream_t st) {
  if (f.family != YL_DWF_DWS) return hipErrorNotSupported;
#define YL_DWS_RUN(A, G, K, S_) if (f.a[0] == A && f.a[1] == G && f.a[2] == K && f.a[3] == S_) return dws_go<A, G, K, S_, 4>(p, st);
  YL_DWS_SHAPES(YL_DWS_RUN)
#undef YL_DWS_RUN
  return hipErrorNotSupported;
}

// ------------------------------------------------------------------------------------------------
// Dense 3x3 stride-1 convolution as Winograd F(2x2,3x3): Y = A^T [ sum_c (G g G^T) . (B^T d B) ] A -- 16 multiplications
// per 2x2 output tile and channel pair instead of 36 (2.25x fewer MFMAs; option "winograd": every eligible layer by
// default since round 4 -- the transforms round differently from the direct convolution, so the result is not
// bit-identical to it, but the score error against the fp32 oracle was measured equal: profiles/r04_winograd_margin*.json).
// One wave owns 16 Winograd tiles (lane pl = tile, 4 channels 4kq..4kq+3 of a 16-channel block) and 2 n-tiles, and
// holds ALL 16 transform positions' accumulators (16 x 2 x 4 = 128 VGPRs), so the loop is channel-block outer:
//   per k-block:  4x4 input patch of the lane's tile (16 float4 from L1/L2, zero buffer outside the image)
//                 column transform in place (16 float4 ops), then per position xi one row-transform op -> B operand,
//                 two A fragments of U_xi from the LDS chunk, 8 MFMAs
// The U image ([n-group][k-block][xi][2][64][4], pack_wino in yl_program.cpp) streams through LDS in 32 KiB chunks,
// double-buffered, one barrier per k-block, 8 waves (128 tiles = 512 output pixels) share a chunk; (n-group, m-tile)
// items group-major in XCD bands like yl_conv_kxk_kernel.  Output transform, bias, ReLU-family clamp and the four
// NHWC float4 stores per n-tile in the epilogue (ReLU-family clamp or SiLU).
// SH = 1 (round 4): the conv reads its input nearest-upsampled by 2 (yl_layer.in_shift, the prototype branch's second conv):
// p.H / p.W are the dims of the VIRTUAL tensor; the 4x4 patch of a tile maps onto a 3x3 block of stored pixels
// (rows / columns (2t-1+r) >> 1 = t-1, t, t, t+1).
// dynamic LDS of yl_conv_wino_kernel: two buffers of one k-block's U = 16 positions x NT pieces of 1 KiB, [2][16][NT][64] float4 at 0
struct YlWinoLds {
  static constexpr size_t LIMIT = 96 * 1024;
  static constexpr int NT = 2;                               // n-tiles per item
  static constexpr size_t bytes = (size_t)2 * 16 * NT * 1024;
};

template <int SH>
__global__ __launch_bounds__(512, 2) void yl_conv_wino_kernel(YlConvP p) {
  constexpr int NW = 8, NT = YlWinoLds::NT;
  extern __shared__ __attribute__((aligned(16))) float yl_clds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, pl = lane & 15;
  const int KB = p.KB, Cin = p.Cin, H = p.H, W = p.W, OH = p.OH, OW = p.OW, N = p.N;
  const int TW = (OW + 1) >> 1, TH = (OH + 1) >> 1;
  const int timg = TW * TH;
  const long T = (long)p.B * timg;                            // Winograd tiles
  const yl_act_t* const xin = p.x;
  const long zdelta = p.zeros - p.x;
  f32x4* wl = reinterpret_cast<f32x4*>(yl_clds);            // [2][16][NT][64] float4
  const f32x4* wg = reinterpret_cast<const f32x4*>(p.wino);
  const int G = (p.NTtot + NT - 1) / NT;
  const int bx = blockIdx.x, gx = gridDim.x;                 // gx % 8 == 0
  const YlBandSplit ws = yl_band_split(bx, gx, p.ntiles, G);   // XCD bands, strided items
  const int per = ws.per, slot = ws.slot, band0 = ws.band0, bt = ws.bt, nmine = ws.nmine;
  const long total_chunks = (long)nmine * KB;
  auto load_chunk = [&](int g, int kb, int buf) {
    for (int i = wave; i < 16 * NT; i += NW)
      yl_glds16(wg + (((size_t)g * KB + kb) * 16 * NT + i) * 64 + lane, wl + ((size_t)buf * 16 * NT + i) * 64);
  };
  // item -> (n-group g, m-tile): n-groups in blocks of GBS, inside a block m-tile-major with the GBS groups innermost,
  // so the workgroups of an XCD (consecutive items) read the SAME 128-tile input window for GBS n-groups at a time
  // and stream only GBS / G of the U image: both stay in the XCD's 4 MB L2 (group-major order re-read the input
  // from HBM / Infinity Cache once per n-group: 11 x 269 MB per launch at 80x80)
  constexpr int GBS = 4;
  const int nbf = G / GBS;
  auto item_g = [&](int item, int& mt) {
    int gb = item / (bt * GBS), cnt = GBS;
    if (gb >= nbf) { gb = nbf; cnt = G - nbf * GBS; }
    const int rem = item - gb * bt * GBS;
    mt = rem / cnt;
    return gb * GBS + (rem - mt * cnt);
  };
  int mt0 = 0;
  if (total_chunks > 0) load_chunk(item_g(slot, mt0), 0, 0);
  long gchunk = 0;
  __syncthreads();
  // Two wave groups half a k-block out of phase.  Wave w of a workgroup runs on SIMD w % 4, so waves 0-3 and 4-7 are
  // one wave per SIMD each: while group 0 waits for the patch of block n + 1 and transforms it (P1), group 1 issues
  // the MFMAs of block n (P2) on the same SIMDs, then the roles swap.  Every wave runs  P1; barrier; P2; barrier  and
  // group 1 starts one barrier late; chunk n + 1 is copied to LDS in the slot between the two groups' uses of the
  // buffer it replaces (each wave its share).  In phase, all eight waves waited for memory together: smooth3 2.59 ms;
  // out of phase 2.06 ms.  (Grouping by w & 1 or (w >> 1) & 1 puts both waves of a SIMD in one group: 3.27 ms.)
  const int grp = wave >> 2;
  if (grp == 1) __syncthreads();
  // SH == 0 (round 6): the patch loads go through a raw buffer descriptor whose base sits (W + 1) pixels IN FRONT of the tensor, so
  // that the lane's part of every address -- the patch origin, which may lie one row and one column outside the image -- is ONE
  // non-negative 32-bit byte offset for the tile and the element / k-block part is a scalar offset; elements outside the image
  // take an out-of-range offset (one select each; the loop carried a select pair, a compare and a 64-bit add per element: 85
  // vector instructions per k-block for 16 loads).  Lanes of the channel tail of the last k-block take the out-of-range offset
  // for every element (one select per k-block on the in-image mask): they would load the next pixel's channels, and U being
  // zero there (pack_wino) does not make 0 x inf / NaN zero.
  const int borg = (W + 1) * Cin * (int)sizeof(yl_act_t);
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(xin) - borg), 0, (int)((long)p.B * H * W * Cin * (long)sizeof(yl_act_t)) + borg, 0x00020000);
  const float lo = yl_act_lo(p.act), hi = yl_act_hi(p.act);

  for (int wi = 0; wi < nmine; ++wi) {
    const int item = slot + wi * per;
    int mtl = 0;
    const int g = item_g(item, mtl);
    const int mtile = band0 + mtl;
    long t = ((long)mtile * NW + wave) * 16 + pl;
    const bool tvalid = t < T;
    if (!tvalid) t = T - 1;
    const int b = (int)(t / timg);
    const int trem = (int)(t - (long)b * timg);
    const int ty = trem / TW, tx = trem - ty * TW;
    // patch offsets (floats from p.x; the launcher guarantees the tensor is < 2^31 floats): 16 pixels, rows 2ty-1 ..
    // 2ty+2, columns 2tx-1 .. 2tx+2; bit e of `inb` clear = outside the image (zero buffer)
    const int pbase = ((b * H + 2 * ty - 1) * W + 2 * tx - 1) * Cin + 4 * kq;   // patch origin (may lie outside: masked)
    int rowoff[4], coloff[4];                                    // SH: stored-tensor offsets of the patch rows / columns
    if (SH) {
      const int Hs = H >> SH, Ws = W >> SH;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        rowoff[r] = ((b * Hs + ((2 * ty - 1 + r) >> SH)) * Ws) * Cin + 4 * kq;
        coloff[r] = ((2 * tx - 1 + r) >> SH) * Cin;
      }
    }
    unsigned inb = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int iy = 2 * ty - 1 + r, ix = 2 * tx - 1 + q;
        inb |= (iy >= 0 && iy < H && ix >= 0 && ix < W) ? (1u << (r * 4 + q)) : 0u;
      }
    const int vbase = pbase * (int)sizeof(yl_act_t) + borg;       // >= 0: the patch origin seen from the descriptor's base
    auto load_row = [&](int kb, int r, f32x4 (&dst)[16]) {
      if (!SH && !YL_F16S) {
        const unsigned inbk = kb * 16 + 4 * kq < Cin ? inb : 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int e = r * 4 + q;
          dst[e] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, ((inbk >> e) & 1u) ? vbase : (int)0x80000000u,
                                                                                 ((r * W + q) * Cin + kb * 16) * (int)sizeof(yl_act_t), 0));
        }
        return;
      }
      const bool tail = kb * 16 + 4 * kq >= Cin;                  // channel tail of the last block: zeros
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = r * 4 + q;
        const int off = SH ? rowoff[r] + coloff[q] + kb * 16
                           : pbase + (r * W + q) * Cin + kb * 16;  // (r * W + q) * Cin + kb * 16: wave-uniform
        dst[e] = yl_ld4((((inb >> e) & 1u) && !tail) ? xin + off : xin + zdelta);
      }
    };
    f32x4 acc[16][1][NT];
#pragma unroll
    for (int xi = 0; xi < 16; ++xi)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[xi][0][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < KB; ++kb, ++gchunk) {
      const int buf = (int)(gchunk & 1);
      const bool more = gchunk + 1 < total_chunks;
      int gn = g, kn = kb + 1;
      if (kn == KB) { int mtn = 0; kn = 0; gn = more ? item_g(item + per, mtn) : g; }
      if (grp == 1 && more) load_chunk(gn, kn, buf ^ 1);
      f32x4 d[16];
#pragma unroll
      for (int r = 0; r < 4; ++r) load_row(kb, r, d);
      // column transform B^T d (rows of B^T: d0-d2, d1+d2, d2-d1, d1-d3), in place per column
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 d0 = d[q], d1 = d[4 + q], d2 = d[8 + q], d3 = d[12 + q];
        d[q] = d0 - d2; d[4 + q] = d1 + d2; d[8 + q] = d2 - d1; d[12 + q] = d1 - d3;
      }
      __syncthreads();
      if (grp == 0 && more) load_chunk(gn, kn, buf ^ 1);
      const f32x4* wb = wl + (size_t)buf * 16 * NT * 64 + lane;
      // A fragments of position xi + 1 are requested before the MFMAs of position xi (explicit double buffer, order
      // pinned with sched_barrier: left alone the compiler issued the two ds_read_b128 right in front of the MFMAs
      // that need them and every position waited out an LDS round trip)
      f32x4 wq[2][NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) wq[0][nt] = wb[nt * 64];
#pragma unroll
      for (int xi = 0; xi < 16; ++xi) {
        const int i = xi >> 2, j = xi & 3;
        const f32x4 t0 = d[i * 4], t1 = d[i * 4 + 1], t2 = d[i * 4 + 2], t3 = d[i * 4 + 3];
        f32x4 xq[1];
        xq[0] = j == 0 ? t0 - t2 : j == 1 ? t1 + t2 : j == 2 ? t2 - t1 : t1 - t3;
        if (xi + 1 < 16) {
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) wq[(xi + 1) & 1][nt] = wb[((xi + 1) * NT + nt) * 64];
        }
        __builtin_amdgcn_sched_barrier(0);                         // reads of position xi + 1 stay above ...
        yl_mma_step<NT, 1>(wq[xi & 1], xq, acc[xi]);
        __builtin_amdgcn_sched_barrier(0);                         // ... the MFMAs of position xi
      }
      if (kb + 1 < KB) __syncthreads();                            // (after the last block: behind the epilogue)
    }
    // output transform Y = A^T M A (A^T = [[1,1,1,0],[0,1,-1,-1]]), bias, clamp, store the 2x2 pixels
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = (g * NT + nt) * 16 + 4 * kq;
      f32x4 r0[4], r1[4];                                         // A^T M : two rows x four columns
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r0[j] = acc[j][0][nt] + acc[4 + j][0][nt] + acc[8 + j][0][nt];
        r1[j] = acc[4 + j][0][nt] - acc[8 + j][0][nt] - acc[12 + j][0][nt];
      }
      f32x4 y[2][2];
      y[0][0] = r0[0] + r0[1] + r0[2]; y[0][1] = r0[1] - r0[2] - r0[3];
      y[1][0] = r1[0] + r1[1] + r1[2]; y[1][1] = r1[1] - r1[2] - r1[3];
      if (tvalid && n < N) {
        const f32x4 bias = yl_ld4(p.bias + n);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int c2 = 0; c2 < 2; ++c2) {
            const int oy = 2 * ty + a, ox = 2 * tx + c2;
            if (oy < OH && ox < OW) {
              const size_t o = (((size_t)b * OH + oy) * OW + ox) * N + n;
              f32x4 v = yl_actc(y[a][c2] + bias, p.act, lo, hi);
              if (p.res) v += yl_ld4(p.res + o);                     // residual after the activation (yl_epi_generic's order)
              yl_st4(p.out + o, v);
            }
          }
      }
    }
    __syncthreads();               // closes the item's last P2 slot
  }
  if (grp == 0) __syncthreads();   // group 1's last slot
}

static const YlConvKernel wino_kernels[2] = {yl_conv_wino_kernel<0>, yl_conv_wino_kernel<1>};   // [input upsampled 2x (in_shift)]

static hipError_t wino_go(const YlConvP& p0, hipStream_t st) {
  YlConvP p = p0;
  const long T = (long)p.B * ((p.OH + 1) >> 1) * ((p.OW + 1) >> 1);
  p.ntiles = (int)((T + 127) / 128);
  const size_t lds = YlWinoLds::bytes;
  const int G = (p.NTtot + 1) / 2;
  const int gx = yl_band_grid(yl_resident_blocks((const void*)wino_kernels[0], 512, lds, 8), (long)p.ntiles * G);
  hipLaunchKernelGGL(wino_kernels[p.in_shift ? 1 : 0], dim3(gx), dim3(512), lds, st, p);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Winograd F(2x2,3x3), second form (round 5): the 16 transform positions are dealt to the WAVES -- wave w owns positions
// (i, j) = (w >> 1, 2 (w & 1) + {0, 1}) -- and every wave holds MT m-tiles x NT n-tiles of accumulators for its two
// positions.  yl_conv_wino_kernel gives each wave all 16 positions of 16 tiles x 2 n-tiles: per 128 MFMAs it fetches and
// transforms a 16 KB patch and reads 32 KB of U from LDS, the input is re-fetched and re-transformed once per 32 output
// channels (11 times at N = 328), and its two wave groups alternate between a memory phase and an MFMA phase with two
// barriers per k-block (MFMA pipe 56 % busy at 80 x 80).  Here a workgroup item is MT m-tiles (m-tile = 4 x 4 Winograd
// tiles = 8 x 8 output pixels of one image) x NT n-tiles; per 16-channel k-block:
//   window  the 10 x 10-pixel input window of each m-tile (64 B per pixel) lands in LDS by asynchronous LDS-DMA copies
//           (MT per wave, no VGPRs), double-buffered, requested a whole k-block ahead: every input pixel is fetched ONCE
//           per item -- not once per tile that touches it -- and once per NT n-tiles (7 times at N = 328, NT = 3)
//   B       a position (i, j) of B^T d B is a signed sum of FOUR window pixels (rows {0,2} {1,2} {2,1} {1,3} by i, columns
//           likewise by j), so a wave builds the B fragments of its two positions itself: per m-tile 6 ds_read_b128 (2 rows
//           x 3 columns), 3 row combinations X + s Y, 2 column combinations -- 10 packed VALU operations between the MFMAs.
//           No transformed image in LDS, no second barrier.  (A first version wrote V = B^T d B to LDS with all 512
//           threads and read it back as B fragments: two barriers per k-block, a 16-read / 8-write LDS round trip per
//           thread and a 160 KB footprint; in-kernel cycle stamps and ablation builds priced that round trip at 0.24 ms
//           of a 1.98 ms launch and the bare MFMA + barrier skeleton at 1.45 ms.)
//   A       NT 1-KB fragment loads of U_xi straight from L1/L2 per position, requested one position ahead -- U of a
//           position is used by one wave only, LDS would not share anything
//   MFMA    2 x MT x NT x 4 per wave and k-block; the memory requests sit BETWEEN them (issued back to back -- 8 waves x 7
//           instructions at one moment -- they filled the CU's vector-memory queue, and in-order issue kept every wave in
//           front of its MFMAs until its own requests were taken: 2300 of 11000 cycles per k-block)
// ONE barrier per k-block.  After the K loop the accumulators of one n-tile at a time go through LDS so that thread
// (m-tile, lane, output row) gathers the 12 positions of its row: output transform, bias, activation, residual, float4
// NHWC stores.  Same transform expressions (X - Y == X + (-1) Y in one rounding), k order (k-blocks ascending, the four
// MFMAs of a block in yl_mma_step's order per accumulator) and epilogue as yl_conv_wino_kernel: BIT-IDENTICAL to it
// (tests/test_gpu_parity.py).  Reads the same U image (pack_wino).
// Window layout (16-byte slots, 512 per m-tile and buffer, 480 used): pixel index P = R(y) * 12 + C(x) with R(y) =
// 5 (y & 1) + (y >> 1), C likewise -- even rows / columns first, so that tiles two pixels apart are neighbours --,
// slot = 4 P + (kq ^ 2 ((P >> 2) & 1)).  (a) the four lanes of a quad copy the 64 contiguous bytes of ONE pixel: a copy
// instruction touches 16 cache lines, not 64; (b) a ds_read_b128 lane group holds 8 tiles with channel group kq = a
// (tile rows {0,3}) and 8 with a ^ 1 (tile rows {1,2}) (MI355X_MICROARCH.md, LDS): P = ty4 * 12 + tx4 + const takes every
// residue mod 4 twice per set, the two with bit 2 of P different (36 = 9 * 4, 12 = 3 * 4), so the low slot bits are
// {a, a ^ 2} and {a ^ 1, a ^ 3}: sixteen distinct 16-byte bank groups, conflict-free.
// dynamic LDS of yl_conv_wino2_kernel (offsets in float4s): [2][MT][RM] windows | [16][MT][64] accumulator exchange of the epilogue.
// Every instantiation's limit is its exact size
struct YlWino2Lds {
  static constexpr int RP = 12, RM = 512;                       // window row pitch in pixels; slots per m-tile window (480 used: 8 full copy instructions)
  size_t Xl, bytes;
  constexpr __host__ __device__ YlWino2Lds(int MT) : Xl((size_t)2 * MT * RM), bytes((Xl + (size_t)16 * MT * 64) * 16) {}
};

template <int MT, int NT, int SH>
__global__ __launch_bounds__(512, 2) void yl_conv_wino2_kernel(YlConvP p) {
  constexpr int RP = YlWino2Lds::RP, RM = YlWino2Lds::RM;
  extern __shared__ __attribute__((aligned(16))) float yl_clds[];
  f32x4* const Rl = reinterpret_cast<f32x4*>(yl_clds);
  f32x4* const Xl = Rl + YlWino2Lds(MT).Xl;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, pl = lane & 15;                      // MFMA lane: 4 channels 4kq.. of tile pl
  const int ty4 = pl >> 2, tx4 = pl & 3;
  const int KB = p.KB, Cin = p.Cin, H = p.H, W = p.W, OH = p.OH, OW = p.OW, N = p.N;
  const int Hs = H >> SH, Ws = W >> SH;
  const int TW = (OW + 1) >> 1, TH = (OH + 1) >> 1;
  const int MX = (TW + 3) >> 2, MY = (TH + 3) >> 2;
  const int mimg = MX * MY;
  const long MTOT = (long)p.B * mimg;                           // m-tiles
  const yl_act_t* const xin = p.x;
  const int NG2 = (p.NTtot + 1) >> 1;                           // n-tile pairs of the U image
  const int G = (p.NTtot + NT - 1) / NT;
  const int bx = blockIdx.x, gx = gridDim.x;                    // gx % 8 == 0
  const YlBandSplit ws = yl_band_split(bx, gx, p.ntiles, G);   // XCD bands, strided items
  const int per = ws.per, slot = ws.slot, band0 = ws.band0, bt = ws.bt, nmine = ws.nmine;
  // item -> (n-group, m-block): as in yl_conv_wino_kernel (the workgroups of an XCD walk GBS n-groups of one input window)
  constexpr int GBS = 4;
  const int nbf = G / GBS;
  auto item_g = [&](int item, int& mt) {
    int gb = item / (bt * GBS), cnt = GBS;
    if (gb >= nbf) { gb = nbf; cnt = G - nbf * GBS; }
    const int rem = item - gb * bt * GBS;
    mt = rem / cnt;
    return gb * GBS + (rem - mt * cnt);
  };
  // copy role of the lane: slot rs = wave * 64 + lane of every m-tile's window
  const int rs = wave * 64 + lane;
  const int rP = rs >> 2, rkq = (rs & 3) ^ (((rP >> 2) & 1) << 1);
  const int rpr = rP / RP, rpc = rP - rpr * RP;
  const int ry = rpr < 5 ? 2 * rpr : 2 * (rpr - 5) + 1, rx = rpc < 5 ? 2 * rpc : 2 * (rpc - 5) + 1;
  const bool rpix = rpr < 10 && rpc < 10;                        // (slots 480..511 and the pad columns copy zeros)
  // position role of the wave: rows X + sr * Y, columns u0 - u1 and u1 + sc * u2
  const int pi = wave >> 1, pj = wave & 1;
  const int rowX = pi == 0 ? 0 : pi == 2 ? 2 : 1, rowY = pi == 2 ? 1 : pi == 3 ? 3 : 2;
  const float sr = pi == 1 ? 1.0f : -1.0f, sc = pj ? -1.0f : 1.0f;
  const f32x4 sr4 = (f32x4){sr, sr, sr, sr}, sc4 = (f32x4){sc, sc, sc, sc};
  const int col0 = pj ? 2 : 0, col1 = pj ? 1 : 2, col2 = pj ? 3 : 1;
  auto wslot = [&](int r, int c) {                               // the lane's slot of window pixel (2 ty4 + r, 2 tx4 + c)
    const int P = (ty4 + (r & 1) * 5 + (r >> 1)) * RP + tx4 + (c & 1) * 5 + (c >> 1);
    return 4 * P + (kq ^ (((P >> 2) & 1) << 1));
  };
  const int sX0 = wslot(rowX, col0), sX1 = wslot(rowX, col1), sX2 = wslot(rowX, col2);
  const int sY0 = wslot(rowY, col0), sY1 = wslot(rowY, col1), sY2 = wslot(rowY, col2);
  const float lo = yl_act_lo(p.act), hi = yl_act_hi(p.act);

  // Both operand streams go through raw buffer descriptors (round 6): the per-lane part of an address is ONE 32-bit byte
  // offset fixed for the whole item, the k-block part is a scalar offset -- no vector instruction in the loop computes an
  // address (the loop carried 14 64-bit adds and 8 selects for its ten requests).  Window lanes outside the image carry an
  // offset beyond num_records: the hardware range check makes the copy write zeros.  So do the lanes of the channel tail of
  // the last k-block (one select per copy): they would copy the first channels of the next pixel -- the next image's behind
  // an image's last pixel -- and U being zero there (pack_wino) does not make 0 x inf / NaN zero.
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<yl_act_t*>(xin), 0, (int)((long)p.B * Hs * Ws * Cin * (long)sizeof(yl_act_t)), 0x00020000);
  const __amdgpu_buffer_rsrc_t urs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(p.wino), 0, (int)((long)NG2 * KB * 16 * 2 * 1024), 0x00020000);
  constexpr unsigned OOB = 0x80000000u;
  const int lane16 = lane * 16;
  unsigned voff[MT];                                             // byte offset of the lane's window slot (k-block 0), OOB = zeros
  auto setup = [&](int mblock) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const long mi = (long)mblock * MT + mt;
      const int b = (int)(mi / mimg);
      const int r = (int)(mi - (long)b * mimg);
      const int my = r / MX, mx = r - my * MX;
      const int gy = 8 * my - 1 + ry, gxx = 8 * mx - 1 + rx;
      const bool in = rpix && mi < MTOT && gy >= 0 && gy < H && gxx >= 0 && gxx < W;
      voff[mt] = in ? (unsigned)((((b * Hs + (gy >> SH)) * Ws + (gxx >> SH)) * Cin + 4 * rkq) * (int)sizeof(yl_act_t)) : OOB;
    }
  };
  auto issue_raw = [&](int kb, int buf) {                        // branch-free: it is scheduled between MFMAs
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(Rl + (buf * MT + mt) * RM + wave * 64), 16,
                                               kb * 16 + 4 * rkq < Cin ? (int)voff[mt] : (int)OOB, kb * 16 * (int)sizeof(yl_act_t), 0, 0);
  };
  // Parity: the loop below is unrolled by two so that the window buffer and the U register set of a block are compile-time
  // (LDS read offsets become immediates, no register renaming at the block's end).  Block kb uses buffer / set
  // (kb + KB) & 1: the LAST block always sits in buffer 1, an odd KB starts with one single block out of buffer 1.
  const int sh = KB & 1;

  int mb0 = 0, g = 0;
  if (nmine > 0) { g = item_g(slot, mb0); setup(band0 + mb0); issue_raw(0, sh); }
  for (int wi = 0; wi < nmine; ++wi) {
    const int mblock = band0 + mb0;
    // U fragment of (n-tile g*NT + nt, k-block kb, position xi): pair-major image of pack_wino; scalar byte offset
    int ubs[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      int ntg = g * NT + nt;
      if (ntg >= 2 * NG2) ntg = 0;                                // beyond the image: any fragment (columns never stored)
      ubs[nt] = (((ntg >> 1) * KB * 32 + (ntg & 1)) * 64 + 2 * wave * 128) * 16;
    }
    auto load_u = [&](int kb, int ps, f32x4 (&dst)[NT]) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        dst[nt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(urs, lane16, ubs[nt] + (kb * 16 + ps) * 2048, 0));
    };
    f32x4 acc[2][MT][NT];
#pragma unroll
    for (int ps = 0; ps < 2; ++ps)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[ps][mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // B fragments of the wave's two positions for m-tile mt out of window buffer `buf`
    auto load_win = [&](int buf, int mt, f32x4 (&x)[3], f32x4 (&y)[3]) {
      const f32x4* const wb = Rl + (buf * MT + mt) * RM;
      x[0] = wb[sX0]; x[1] = wb[sX1]; x[2] = wb[sX2];
      y[0] = wb[sY0]; y[1] = wb[sY1]; y[2] = wb[sY2];
    };
    auto mma_mt = [&](const f32x4 (&a)[NT], const f32x4& b, f32x4 (&c)[NT]) {    // one m-tile: the 4 steps x NT n-tiles
#if YL_BF16
      const f32x4 bb[1] = {b};
      f32x4 cc[1][NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) cc[0][nt] = c[nt];
      yl_mma_step<NT, 1>(a, bb, cc);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) c[nt] = cc[0][nt];
#else
#pragma unroll
      for (int st = 0; st < 4; ++st)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) c[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nt][st], b[st], c[nt], 0, 0, 0);
#endif
    };
    // One k-block: MT x (window reads of the next m-tile, B fragments, 2 x NT x 4 MFMAs).  The block's ONE barrier sits in
    // front of the LAST m-tile's MFMAs: by then the wave has read all it needs of window(kb) and its copies of
    // window(kb + 1) (requested a k-block ago) have landed, so behind the barrier window(kb + 1) is complete and window(kb)'s
    // buffer is free -- the wave requests window(kb + 2) into it and the first m-tile's reads of block kb + 1, and only
    // then issues the last m-tile's 2 x NT x 4 MFMAs: barrier and LDS latency lie under them and the MFMA stream runs on
    // across k-blocks (with the barrier at the top of the block both waves of a SIMD met it with nothing to issue).
    // MODE 0: any block; 1: the second-to-last (nothing left to request); 2: the last (peeled like this so that the body
    // is branch-free: with conditional requests every merge waited for all outstanding loads).  The U fragments of block
    // kb + 1 are requested into the OTHER register set under the first two m-tiles -- requested behind the last use of this
    // block's set they had no time to arrive.  PAR = the block's window buffer and U set.
    f32x4 ua[2][2][NT];                                           // [set][position][n-tile]
    f32x4 x[2][3], y[2][3];
    auto kblock = [&](int kb, auto par, auto mode) {
      constexpr int PAR = decltype(par)::value;
      constexpr int MODE = decltype(mode)::value;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        if (mt + 1 < MT) load_win(PAR, mt + 1, x[(mt + 1) & 1], y[(mt + 1) & 1]);
        f32x4 b0, b1;
        yl_wino_b(x[mt & 1], y[mt & 1], sr4, sc4, b0, b1);       // (pinned packed form: +1.1 %, profiles/r06_pinned_pk_chains_ab.txt)
        if (mt == MT - 1 && MODE < 2) {
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_s_waitcnt(0x0070);                     // vmcnt(0) lgkmcnt(0): the wave's own window copies and reads (not left to the
          __syncthreads();                                        // compiler: LDS-DMA requests of the previous iteration are not carried over the back edge)
          if (MODE == 0) issue_raw(kb + 2, PAR);
          load_win(PAR ^ 1, 0, x[0], y[0]);
          __builtin_amdgcn_sched_barrier(0);
        }
        mma_mt(ua[PAR][0], b0, acc[0][mt]);
        if (MODE < 2 && mt == 0) load_u(kb + 1, 0, ua[PAR ^ 1][0]);
        mma_mt(ua[PAR][1], b1, acc[1][mt]);
        if (MODE < 2 && mt == (MT > 2 ? 1 : 0)) load_u(kb + 1, 1, ua[PAR ^ 1][1]);
        // m-tile by m-tile: left alone the scheduler gathered all window reads at the top (spills) and pushed the U
        // requests behind the last MFMA
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    int kb = 0;
    if (sh) {                                                     // odd KB: block 0 on its own, out of buffer / set 1
      load_u(0, 0, ua[1][0]);
      load_u(0, 1, ua[1][1]);
      __builtin_amdgcn_s_waitcnt(0x0F70);                         // vmcnt(0)
      __syncthreads();                                            // window(0) landed (requested under the previous epilogue)
      issue_raw(1, 0);
      load_win(1, 0, x[0], y[0]);
      kblock(0, I1{}, I0{});
      kb = 1;
    } else {
      load_u(0, 0, ua[0][0]);
      load_u(0, 1, ua[0][1]);
      __builtin_amdgcn_s_waitcnt(0x0F70);
      __syncthreads();
      issue_raw(1, 1);
      load_win(0, 0, x[0], y[0]);
    }
    for (; kb + 3 < KB; kb += 2) {
      kblock(kb, I0{}, I0{});
      kblock(kb + 1, I1{}, I0{});
    }
    kblock(KB - 2, I0{}, I1{});
    kblock(KB - 1, I1{}, I2{});
    // the item's coordinates for the epilogue, then the next item's window(0) request flies under the epilogue
    const int eg = g;
    const int emt = wave & (MT - 1), epart = wave / MT;            // output role: m-tile, row a (and column c2 when MT = 2)
    const long emi = (long)mblock * MT + emt;
    if (wi + 1 < nmine) { g = item_g(slot + (wi + 1) * per, mb0); setup(band0 + mb0); }
    const bool evalid = emi < MTOT;
    const int eb = (int)((evalid ? emi : 0) / mimg);
    const int er = (int)((evalid ? emi : 0) - (long)eb * mimg);
    const int emy = er / MX, emx = er - emy * MX;
    const int oa = epart & 1;
    const int oy = 2 * (4 * emy + ty4) + oa, ox0 = 2 * (4 * emx + tx4);
    __syncthreads();                                              // every wave is done with the windows
    if (wi + 1 < nmine) issue_raw(0, sh);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      if (nt > 0) __syncthreads();                                // the previous n-tile's exchange is read
#pragma unroll
      for (int ps = 0; ps < 2; ++ps)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) Xl[((size_t)(2 * wave + ps) * MT + mt) * 64 + lane] = acc[ps][mt][nt];
      __syncthreads();
      const f32x4* const mb = Xl + (size_t)emt * 64 + lane;
      f32x4 r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 m1 = mb[((4 + j) * MT) * 64], m2 = mb[((8 + j) * MT) * 64];
        if (oa == 0) r[j] = mb[(j * MT) * 64] + m1 + m2;
        else r[j] = m1 - m2 - mb[((12 + j) * MT) * 64];
      }
      f32x4 yy[2];
      yy[0] = r[0] + r[1] + r[2]; yy[1] = r[1] - r[2] - r[3];
      const int n = ((eg * NT + nt) * 16) + 4 * kq;
      if (evalid && n < N && oy < OH) {
        const f32x4 bias = yl_ld4(p.bias + n);
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) {
          if (MT == 2 && c2 != (epart >> 1)) continue;
          const int ox = ox0 + c2;
          if (ox < OW) {
            const size_t o = (((size_t)eb * OH + oy) * OW + ox) * N + n;
            f32x4 v = yl_actc(yy[c2] + bias, p.act, lo, hi);
            if (p.res) v += yl_ld4(p.res + o);
            yl_st4(p.out + o, v);
          }
        }
      }
    }
  }
}

// instantiated: YL_WINO2_SHAPES (yl_shapes.h: (m-tiles, n-tiles per item)), each for a plain and a 2x upsampled input (in_shift)
static YlConvKernel wino2_kernel_of(int MT, int NT, int in_shift) {
#define YL_WINO2_PICK(A, B) if (MT == A && NT == B) return in_shift ? yl_conv_wino2_kernel<A, B, 1> : yl_conv_wino2_kernel<A, B, 0>;
  YL_WINO2_SHAPES(YL_WINO2_PICK)
#undef YL_WINO2_PICK
  return nullptr;
}
static hipError_t wino2_go(const YlConvP& p0, hipStream_t st, int MT, int NT) {
  const size_t lds = YlWino2Lds(MT).bytes;
  YlConvP p = p0;
  const int TW = (p.OW + 1) >> 1, TH = (p.OH + 1) >> 1;
  const long MTOT = (long)p.B * ((TW + 3) >> 2) * ((TH + 3) >> 2);
  p.ntiles = (int)((MTOT + MT - 1) / MT);
  const int G = (p.NTtot + NT - 1) / NT;
  const int gx = yl_band_grid(yl_resident_blocks((const void*)wino2_kernel_of(MT, NT, 0), 512, lds, 8), (long)p.ntiles * G);
  hipLaunchKernelGGL(wino2_kernel_of(MT, NT, p.in_shift), dim3(gx), dim3(512), lds, st, p);
  return hipGetLastError();
}

// dense 3x3 stride-1 pad-1 layers that carry a Winograd image (yl_api.hip builds it for >= 64 channels, plain
// ReLU-family epilogue; layer_params hands it over only under option "winograd").
hipError_t yl_launch_conv_wino(const YlConvP& p, hipStream_t st) {
  if (!p.wino || p.k != 3 || p.stride != 1 || p.dw_k > 0 || p.up || p.dec_boxes || p.C1 > 0 || p.w3p || p.scale) return hipErrorNotSupported;
  // first form or second form with (m-tiles, n-tiles) per item: yl_wino_form (yl_shapes.h), which yl_query_wino_form reports
  const YlWinoForm f = yl_wino_form(p.Cin, p.N, p.OH, p.OW, p.B,   // (p.OH x p.OW is also the virtual input grid p.H x p.W: a layer carries p.wino only then, yl_program.cpp)
                                    p.in_shift, sizeof(yl_act_t), (p.dev & YL_DEV_WINO_V1) != 0, YL_DEV_WINO_SHAPE(p.dev));
  if (f.form == 0) return hipErrorNotSupported;
  return f.form == 2 ? wino2_go(p, st, f.mt, f.nt) : wino_go(p, st);
}

// ------------------------------------------------------------------------------------------------
namespace {

// yl_conv_dwc_kernel<DK, DS, NTW>: depthwise 3x3 / 5x5 x stride 1 / 2 x NTW (n-tiles per GEMM wave) 1..5, as [NTW - 1][DK == 5][DS == 2]
#define YL_DWC_SHAPES(NTW) \
  {{yl_conv_dwc_kernel<3, 1, NTW>, yl_conv_dwc_kernel<3, 2, NTW>}, {yl_conv_dwc_kernel<5, 1, NTW>, yl_conv_dwc_kernel<5, 2, NTW>}}
const YlMultiKernel dwc_kernels[5][2][2] = {YL_DWC_SHAPES(1), YL_DWC_SHAPES(2), YL_DWC_SHAPES(3), YL_DWC_SHAPES(4), YL_DWC_SHAPES(5)};

int kbmax_of(int ntw) { return ntw == 1 ? 18 : ntw == 2 ? 9 : ntw == 3 ? 6 : 4; }

}  // namespace

// dynamic-LDS limit of every instantiation of this unit: one walk per family over its list
hipError_t yl_convc_init() {
  hipError_t e = hipSuccess;
  const auto cap = [&e](const auto& kernels, size_t bytes) { if (e == hipSuccess) e = yl_set_lds_cap(kernels, bytes); };
#define YL_KXK_CAP(A, B, C) cap(yl_conv_kxk_kernel<A, B, C>, YlKxkLds::LIMIT);
  YL_KXK_SHAPES(YL_KXK_CAP)
#define YL_IR_CAP(A, B, C, D, E, R, S) cap(yl_ir_kernel<A, B, C, D, E, R, S, false>, YlIrLds::LIMIT); cap(yl_ir_kernel<A, B, C, D, E, R, S, true>, YlIrLds::LIMIT);
  YL_IR_SHAPES(YL_IR_CAP)
  cap(pws_kernels, YlPwsLds::LIMIT);
  cap(pws_dec_kernels, YlPwsLds::LIMIT);
  cap(dwt_kernels, YlDwtLds::LIMIT);
  cap(dwt_splitk_kernels, YlDwtLds::LIMIT);
  cap(wino_kernels, YlWinoLds::LIMIT);
#define YL_WINO2_CAP(A, B) cap(yl_conv_wino2_kernel<A, B, 1>, YlWino2Lds(A).bytes); cap(yl_conv_wino2_kernel<A, B, 0>, YlWino2Lds(A).bytes);
  YL_WINO2_SHAPES(YL_WINO2_CAP)
#define YL_DWK_CAP(A, B, C) cap(yl_conv_dwk_kernel<A, B, C>, YlDwkLds::LIMIT);
  YL_DWK_SHAPES(YL_DWK_CAP)
#define YL_DWL_CAP(A) cap(yl_conv_dwl_kernel<A>, YlDwlLds::LIMIT);
  YL_DWL_SHAPES(YL_DWL_CAP)
#define YL_DWS_CAP(A, G, K, S_) cap(yl_conv_dws_kernel<A, G, K, S_, 4>, YlDwsLds::LIMIT);
  YL_DWS_SHAPES(YL_DWS_CAP)
#if !YL_BF16
#define YL_DWX_CAP(A, B) cap(yl_conv_dwx_kernel<A, B>, YlDwtLds::LIMIT);
  YL_DWX_SHAPES(YL_DWX_CAP)
#define YL_PWX_CAP(A, B, C, D) cap(yl_conv_pwx_kernel<A, B, C, D>, YlPwxLds::LIMIT);
  YL_PWX_SHAPES(YL_PWX_CAP)
#undef YL_PWX_CAP
#endif
  cap(dwc_kernels, YlDwcLds::LIMIT);
  return e;
}

// n problems of identical configuration (m.p[0..n-1] filled like for yl_conv_dwh_kernel).  Family 0 when the shape is
// outside this kernel's limits (the caller then takes the halo kernel).
YlDwForm yl_dwc_form(const YlConvMulti& m) {
  const YlDwForm none = {YL_DWF_NONE, {0, 0, 0, 0, 0, 0}};
  const YlConvP& p = m.p[0];
  const int ntw = (p.NTtot + 3) / 4;
  if (ntw < 1 || ntw > 5 || p.KB > kbmax_of(ntw) || (p.N & 3)) return none;
  // Measured per layer (edge_n, B = 64, eager): the producer / consumer split pays where the depthwise phase is
  // long -- K >= 192 channels on a stride-1 depthwise (28 vs 38 us for 3x3, 44 vs 50 us for 5x5 at 20x20) -- and
  // loses on the short-K layers, where two or three of the four depthwise waves idle and the per-tile barrier costs
  // more than the weight prologue it replaces.  "dev_select" bit 3 lifts the restriction (A/B runs).
  const bool all = (p.dev & YL_DEV_DWC_ALL) != 0;       // "dev_select" bit 3: the bitwise-equivalence test
  if (!all && (p.KB < 12 || p.dw_stride != 1)) return none;
  if (!((p.dw_k == 3 || p.dw_k == 5) && (p.dw_stride == 1 || p.dw_stride == 2))) return none;
  if (YlDwcLds{p.dw_k, p.dw_stride, p.KB, p.Cin}.bytes() > YlDwcLds::LIMIT) return none;
  for (int k = 0; k < m.n; ++k)
    if ((m.p[k].OH & 3) || (m.p[k].OW & 3) || (size_t)m.p[k].B * m.p[k].H * m.p[k].W * m.p[k].Cin * 4 >= ((size_t)1 << 31))
      return none;
  return {YL_DWF_DWC, {p.dw_k, p.dw_stride, ntw, 0, 0, 0}};
}

hipError_t yl_launch_conv_dwc(YlConvMulti& m, const YlDwForm& f, hipStream_t st) {
  if (f.family != YL_DWF_DWC) return hipErrorNotSupported;
  const YlConvP& p = m.p[0];
  const size_t lds = YlDwcLds{p.dw_k, p.dw_stride, p.KB, p.Cin}.bytes();
  long tiles[4], total = 0;
  for (int k = 0; k < m.n; ++k) {
    tiles[k] = (long)m.p[k].B * (m.p[k].OH >> 2) * (m.p[k].OW >> 2);
    total += tiles[k];
  }
  const YlMultiKernel kern = dwc_kernels[f.a[2] - 1][f.a[0] == 5][f.a[1] == 2];
  const int res = yl_resident_blocks((const void*)kern, 512, lds, 4);
  // grid: a multiple of 8 workgroups (XCD-aware tile bands, see the kernel), at most what is co-resident and one per tile
  long gx = yl_band_grid(res, total);
  if (m.n == 1) { m.p[0].blk0 = 0; m.p[0].nblk = 0; }
  else {
    // shares of the grid, not of the co-resident count, rounded to nearest and without a per-tile cap: not yl_multi_shares'
    // rule (dwt, dwx), and other grids than it gives
    int at = 0;
    for (int k = 0; k < m.n; ++k) {
      long nb = ((tiles[k] * gx + total / 2) / total + 7) & ~7L;
      if (nb < 8) nb = 8;
      m.p[k].blk0 = at;
      m.p[k].nblk = (int)nb;
      at += (int)nb;
    }
    gx = at;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)gx), dim3(512), lds, st, m);
  return hipGetLastError();
}
