// Trainable dense stem: a stack of bias-free dense k x k convolutions (k in {1, 3}, stride in {1, 2}), each followed by
// BatchNorm2d and ReLU, forward and backward on NHWC fp32 rows (include/yololite_hip.h, yl_stem_*).  The stack's input
// may be the planar image [B][cin][S][S], cin in 1..4, which forward and weight gradient read and no gradient exists of.
//
//   unit u:  z = conv(x_u)   h = relu(bn(z))          x_u: the previous unit's h (the caller's x for unit 0)
//
// The walk over the units, forward and backward, with the handle, its memory and the table checks, is yl_units.h, shared
// with yl_stage.hip: a unit here is a block of its own without a residual, so two rotating buffers do.  BatchNorm, ReLU,
// the column sums and the BatchNorm backward are yl_bn.h's, the 1x1 units the heads' GEMM (yl_block.h: launch_gemm_in)
// with accessors of their own where the unit strides or reads the planar image.  Every dense GEMM, 3x3 and 1x1 in all three
// passes, runs in the handle's operand type (yl_amp_stem_set): fp32, or fp16 / bf16 operands rounded to nearest even with
// fp32 accumulation on v_mfma_f32_16x16x16_*; BatchNorm, ReLU and every float64 sum are the same in every mode.  Here are the stack's configuration and
// units (cfg_ok, make_units, wgrad3_plan), the policy that tells the walk what a unit's convolution launches, and what is
// new: the 3x3 convolution in three passes.
//
// ---- 3x3 forward and input gradient: ONE kernel, an implicit GEMM on v_mfma_f32_16x16x4_f32 in the orientation of
// yl_dneck_conv_kernel (weights: A operand, pixels: B operand; a lane ends with four consecutive output channels of one
// pixel: one 16-byte NHWC store).  The kernel gathers: output pixel (a, b) of a CLASS of destination pixels sums, over a
// tap table (ty, tx) in 0..nty-1 x 0..ntx-1, wp[tap][n][c] * src[ST a + o0 + ty][ST b + o0 + tx][c], zero outside src,
// and lands at dst[os a + poy][os b + pox]:
//   forward, stride s:        ST = s, o0 = -1, 3 x 3 taps (ky, kx) = (ty, tx), every output pixel (os = 1)
//   input gradient, stride 1: ST = 1, o0 = -1, 3 x 3 taps (ky, kx) = (2 - ty, 2 - tx), pack transposed (cin <-> cout)
//   input gradient, stride 2: no zero insertion and no atomics.  Input pixel (i, j) receives tap ky from output row
//     (i + 1 - ky) / 2 when that is even-numerator, so the pixels fall into four parity classes (pi, pj) = (i & 1, j & 1)
//     of (1 + pi) (1 + pj) = 1, 2, 2, 4 taps.  Class pixel a is input row 2 a + pi (os = 2, poy = pi); along y it reads
//     dz row a + ty with ky = 1 (pi = 0; one tap) or ky = 2 - 2 ty (pi = 1; ty = 0, 1): a stride-1 gather (ST = 1,
//     o0 = 0) over dz.  A row a + ty >= S_out lies outside src and is read as zero: the dropped taps of an odd S.
// The k index of the GEMM runs (tap, c), c fastest; each tap's c is padded to a multiple of 4 (cp), so the planar image of
// 3 channels has K = 9 x 4 = 36 of which 27 are not zero.  yl_stem_pack_kernel writes wp[tap][n][cp] once per call from the
// caller's PyTorch-layout tensor, which may start at any 4-byte boundary.
// Workgroup: a tile of T x T = 8 x 8 class pixels of ONE image x a block of 16 PT output channels, PT in {2, 3, 4} (the
// one that pads cout least; cout is 16..96 here: 32 -> one block of 32, 64 -> one of 64, 96 -> two of 48); wave w owns
// tile rows 2 w, 2 w + 1, lane (kq, i): pixel (2 w + (i >> 3), i & 7), k quad kq.
// LDS window: (ST (T - 1) + 3)^2 source pixels, 10 x 10 or 17 x 17, zeros for pixels outside the image.
//   NHWC source: per k-block of 16 channels, FOUR planes win[kq][pixel][4 floats], a plane PL pixels (PL % 16 == 0), a
//   window row RP stored pixels; under ST = 2 a row holds its even columns first and then its odd ones (column wx at
//   (wx & 1) 9 + (wx >> 1)), so the eight pixels of a lane row, two window columns apart, are consecutive for every tap.
//   Bank arithmetic of the tap read (ds_read_b128: four groups of 16 lanes, bank = dword % 64, i.e. 16 slots of 16 bytes;
//   group 0 is lanes 0-3, 12-15, 20-27 = (kq 0: i 0-3, 12-15) and (kq 1: i 4-11), the others alike): a lane's slot is
//   kq PL + q(i) + tap offset mod 16 with q(i) = ST RP (i >> 3) + (i & 7).  ST RP = 24 (ST = 1, RP = 24) or 40 (ST = 2,
//   RP = 20), both 8 mod 16, so q(i) takes all sixteen residues over i = 0..15 and a group's sixteen lanes hit sixteen
//   slots: no conflict, for every tap, at both strides.  (The stride-1 pitch without the parity split gives q = 2 (i & 7)
//   under stride 2: eight residues, 2-way.)
//   Planar source: one plane win[pixel][4] (channel c of the pixel, zero for c >= cin), staged plane by plane with
//   consecutive threads along x; a k step is FOUR TAPS (lane kq: tap 4 step + kq), 3 steps for 9 taps.  The lanes of a
//   group then read q(i) + their own tap's offset: by the code at most 2-way, not measured.
//
// ---- 3x3 weight gradient: dW[n][c][ky][kx] = sum_m dz[m][n] x[s m + tap - 1][c].  The pixel is the MFMA's k index.
// Workgroup (block of GC = 32 input channels, block of GN = 64 output channels, split); wave w owns n0 + 16 w .. + 15; per
// spatial tile of 8 x 8 OUTPUT pixels the x window [pixel][GXS = 36] and the dz tile [pixel][GDS = 68] are staged once
// and all nine taps read them (ds_read_b32, banks per 32-lane half: lanes i are consecutive channels, kq 0 and kq 1 are
// four stored pixels apart, 4 x 36 = 144 and 4 x 68 = 272, both 16 mod 32: no conflict; the parity split keeps "four class
// pixels" at four stored pixels under stride 2).  part[split][tap][n][cp] in fp32 over whole tiles, then an ordered float64
// sum in split order: equal inputs give equal bits.  The split count fills the chip (about 1024 workgroups).
#include "yl_units.h"

namespace {

constexpr int ST_T = 8;                  // spatial tile edge
constexpr int SKB = 16;                  // channels per k-block
constexpr int STAT_TILES_MAX = 1024;     // tiles of a unit's row reductions
constexpr int GC = 32, GXS = GC + 4, GN = 64, GDS = GN + 4;

template <int ST> struct Win {
  static constexpr int WE = ST * (ST_T - 1) + 3;           // window edge: 10 / 17
  static constexpr int WH = (WE + 1) / 2;                  // ST == 2: stored column of the first odd window column
  static constexpr int RP = ST == 1 ? 24 : 20;             // stored pixels per window row: ST * RP == 8 mod 16
  static constexpr int PL = (WE * RP + 15) / 16 * 16;      // pixels per plane
  static __device__ __forceinline__ int col(int wx) { return ST == 1 ? wx : (wx & 1) * WH + (wx >> 1); }
  static __device__ __forceinline__ int at(int wy, int wx) { return wy * RP + col(wx); }      // convolution window
  static __device__ __forceinline__ int gat(int wy, int wx) { return wy * WE + col(wx); }     // weight-gradient window
};
static_assert((1 * Win<1>::RP) % 16 == 8 && (2 * Win<2>::RP) % 16 == 8, "the lane rows are 8 slots apart");
static_assert(Win<1>::RP >= Win<1>::WE && Win<2>::RP >= Win<2>::WE, "a window row fits its pitch");

struct PackP { int ntap; int ky[9], kx[9]; };
// w [O][I][3][3] (PyTorch) -> wp[tap][a][b], b padded with zeros from Bn to Bp.  T == 0: W[a][b][tap] (a = out, b = in);
// T == 1: W[b][a][tap] (a = in, b = out); the tap table says which (ky, kx) a packed tap is
__global__ __launch_bounds__(NT) void yl_stem_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int A, int Bn,
                                                         int Bp, int T, PackP tp) {
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  const long AB = (long)A * Bp;
  if (idx >= tp.ntap * AB) return;
  const int tap = (int)(idx / AB);
  const long ab = idx - tap * AB;
  const int a = (int)(ab / Bp), b = (int)(ab - (long)a * Bp);
  float v = 0.f;
  if (b < Bn) {
    const long oi = T ? (long)b * A + a : (long)a * Bn + b;
    v = w[oi * 9 + tp.ky[tap] * 3 + tp.kx[tap]];
  }
  wp[idx] = v;
}
// ---- 16-bit modes (PR: 1 fp16, 2 bf16; yl_block.h: Frag16, mfma16).  Every staged value is rounded ONCE, to nearest even
// and without a clamp: the weight here, into a pack of 16-bit elements in the same [tap][a][b] order (half the bytes of the
// fp32 pack, in the same buffer), the window when it goes into LDS, where it stays a float that lies on the 16-bit grid, so
// the pitches and the bank arithmetic above hold as they are and the conversion in front of each MFMA is exact.
template <int PR> struct Elem16;
template <> struct Elem16<1> { typedef _Float16 T; };
template <> struct Elem16<2> { typedef __bf16 T; };
template <int PR> __device__ __forceinline__ f32x4 rne4(f32x4 v) {
  return __builtin_convertvector(__builtin_convertvector(v, typename Frag16<PR>::T), f32x4);
}
template <int PR> __device__ __forceinline__ float rne1(float v) { return (float)(typename Elem16<PR>::T)v; }
template <int PR> __device__ __forceinline__ typename Frag16<PR>::T ldh4(const void* base, long elem) {   // elem % 4 == 0
  return *reinterpret_cast<const typename Frag16<PR>::T*>(reinterpret_cast<const char*>(base) + elem * 2);
}
template <int PR>
__global__ __launch_bounds__(NT) void yl_stem_pack16_kernel(const float* __restrict__ w, typename Elem16<PR>::T* __restrict__ wp,
                                                           int A, int Bn, int Bp, int T, PackP tp) {
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  const long AB = (long)A * Bp;
  if (idx >= tp.ntap * AB) return;
  const int tap = (int)(idx / AB);
  const long ab = idx - tap * AB;
  const int a = (int)(ab / Bp), b = (int)(ab - (long)a * Bp);
  float v = 0.f;
  if (b < Bn) {
    const long oi = T ? (long)b * A + a : (long)a * Bn + b;
    v = w[oi * 9 + tp.ky[tap] * 3 + tp.kx[tap]];
  }
  wp[idx] = (typename Elem16<PR>::T)v;
}

struct ConvP {
  const float* src; const float* wp; float* dst;
  int Ss, Cs, Cp, N, Sd;                 // source edge, channels (planes), channels per packed tap; output channels, edge
  int TY, TXn;                           // tiles along y and x
  int ey, ex;                            // class pixels along y and x
  int os, poy, pox;                      // class pixel (a, b) -> destination pixel (os a + poy, os b + pox)
  int o0;                                // class pixel a, tap ty -> source row ST a + o0 + ty
  int nty, ntx;
};
// grid (B * TY * TXn, ceil(N / (16 PT))).  PR != 0: P.wp is the 16-bit pack, and the four 16x16x4 steps over a lane's four k
// values are ONE v_mfma_f32_16x16x16_* on the same four values (NHWC: 9 MFMAs per k-block and p-tile for 36; planar: one per
// k step of four taps); the accumulators, one per tap, and their pairwise sum are those of fp32
template <int ST, int PT, bool PLANAR, int PR = 0>
__global__ __launch_bounds__(NT) void yl_stem_conv_kernel(ConvP P) {
  typedef Win<ST> W;
  constexpr int WE = W::WE;
  __shared__ __attribute__((aligned(16))) float win[(PLANAR ? 1 : 4) * W::PL * 4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, kq = lane >> 4, i = lane & 15;
  const int tiles = P.TY * P.TXn;
  const int b = blockIdx.x / tiles, tr = blockIdx.x - b * tiles;
  const int ty0 = (tr / P.TXn) * ST_T, tx0 = (tr % P.TXn) * ST_T;
  const int n0 = blockIdx.y * (16 * PT);
  const int row = 2 * wave + (i >> 3), col = i & 7;
  const int sy0 = ty0 * ST + P.o0, sx0 = tx0 * ST + P.o0;  // the window's first source pixel
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  // NHWC: one accumulator per tap, summed pairwise at the end: a chain is the 4 ceil(Cs / 16) MFMAs of ONE tap, not of nine
  constexpr int NA = PLANAR ? 1 : 9;
  f32x4 acc[NA][PT];
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) acc[a][pt] = zero;
  if constexpr (PLANAR) {
    for (int item = t; item < 4 * WE * WE; item += NT) {   // plane by plane, consecutive threads along x
      const int c = item / (WE * WE), pw = item - c * (WE * WE), wy = pw / WE, wx = pw - wy * WE;
      const int gy = sy0 + wy, gx = sx0 + wx;
      float v = 0.f;
      if (c < P.Cs && gy >= 0 && gy < P.Ss && gx >= 0 && gx < P.Ss) v = P.src[(((long)b * P.Cs + c) * P.Ss + gy) * P.Ss + gx];
      if constexpr (PR != 0) v = rne1<PR>(v);
      win[W::at(wy, wx) * 4 + c] = v;
    }
    __syncthreads();
    const int ntap = P.nty * P.ntx;
    for (int t0 = 0; t0 < ntap; t0 += 4) {
      const int tap = t0 + kq;
      const bool on = tap < ntap;
      const int ty = on ? tap / P.ntx : 0, tx = on ? tap - ty * P.ntx : 0;
      const f32x4 qv = on ? ld4(&win[W::at(row * ST + ty, col * ST + tx) * 4]) : zero;
      if constexpr (PR == 0) {
        f32x4 pv[PT];
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) {
          const int n = n0 + 16 * pt + i;
          pv[pt] = (on && n < P.N) ? ld4(P.wp + ((long)tap * P.N + n) * 4) : zero;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int pt = 0; pt < PT; ++pt) acc[0][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[pt][s], qv[s], acc[0][pt], 0, 0, 0);
      } else {
        typedef typename Frag16<PR>::T H;
        const H zh = __builtin_convertvector(zero, H), qh = __builtin_convertvector(qv, H);
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) {
          const int n = n0 + 16 * pt + i;
          acc[0][pt] = mfma16((on && n < P.N) ? ldh4<PR>(P.wp, ((long)tap * P.N + n) * 4) : zh, qh, acc[0][pt]);
        }
      }
    }
  } else {
    const int nkb = (P.Cs + SKB - 1) / SKB;
    for (int kb = 0; kb < nkb; ++kb) {
      const int c0 = kb * SKB;
      if (kb) __syncthreads();           // the previous k-block's reads are done
      for (int item = t; item < 4 * WE * WE; item += NT) {
        const int pw = item >> 2, q = item & 3, wy = pw / WE, wx = pw - wy * WE;
        const int gy = sy0 + wy, gx = sx0 + wx;
        const bool ok = gy >= 0 && gy < P.Ss && gx >= 0 && gx < P.Ss && c0 + 4 * q < P.Cs;
        if constexpr (PR == 0)
          st4(&win[(q * W::PL + W::at(wy, wx)) * 4], ok ? ld4(P.src + (((long)b * P.Ss + gy) * P.Ss + gx) * P.Cs + c0 + 4 * q) : zero);
        else
          st4(&win[(q * W::PL + W::at(wy, wx)) * 4],
              ok ? rne4<PR>(ld4(P.src + (((long)b * P.Ss + gy) * P.Ss + gx) * P.Cs + c0 + 4 * q)) : zero);
      }
      __syncthreads();
      const int c = c0 + 4 * kq;
#pragma unroll
      for (int ty = 0; ty < 3; ++ty)
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
          if (ty >= P.nty || tx >= P.ntx) continue;        // uniform: the accumulators are indexed by constants
          const int tap = ty * P.ntx + tx;
          const f32x4 qv = ld4(&win[(kq * W::PL + W::at(row * ST + ty, col * ST + tx)) * 4]);
          if constexpr (PR == 0) {
            f32x4 pv[PT];
#pragma unroll
            for (int pt = 0; pt < PT; ++pt) {
              const int n = n0 + 16 * pt + i;
              pv[pt] = (n < P.N && c < P.Cp) ? ld4(P.wp + ((long)tap * P.N + n) * P.Cp + c) : zero;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
              for (int pt = 0; pt < PT; ++pt)
                acc[ty * 3 + tx][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[pt][s], qv[s], acc[ty * 3 + tx][pt], 0, 0, 0);
          } else {
            typedef typename Frag16<PR>::T H;
            const H zh = __builtin_convertvector(zero, H), qh = __builtin_convertvector(qv, H);
#pragma unroll
            for (int pt = 0; pt < PT; ++pt) {
              const int n = n0 + 16 * pt + i;
              acc[ty * 3 + tx][pt] = mfma16((n < P.N && c < P.Cp) ? ldh4<PR>(P.wp, ((long)tap * P.N + n) * P.Cp + c) : zh, qh,
                                            acc[ty * 3 + tx][pt]);
            }
          }
        }
    }
    if constexpr (!PLANAR) {             // ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)) + 8; a tap that does not exist is zero
#pragma unroll
      for (int pt = 0; pt < PT; ++pt)
        acc[0][pt] = (((acc[0][pt] + acc[1][pt]) + (acc[2][pt] + acc[3][pt])) + ((acc[4][pt] + acc[5][pt]) + (acc[6][pt] + acc[7][pt]))) +
                     acc[8 % NA][pt];
    }
  }
  const int ay = ty0 + row, ax = tx0 + col;
  if (ay < P.ey && ax < P.ex) {
    float* o = P.dst + (((long)b * P.Sd + ay * P.os + P.poy) * P.Sd + ax * P.os + P.pox) * P.N;
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const int n = n0 + 16 * pt + 4 * kq;
      if (n < P.N) st4(o + n, acc[0][pt]);
    }
  }
}

struct WgP {
  const float* x; const float* dz; float* part;
  int S, So, Cs, Cp, N, TX, ntiles, tps; // x edge, dz edge, x channels (planes), padded; dz channels; tiles per edge, in all, per split
};
// grid (ceil(Cp / GC), ceil(N / GN), splits); PTC c-tiles of 16 per lane (planar: 1, the image has at most 4 channels).
// PR != 0: x and dz are rounded as they are staged; kq selects four stored pixels, so the four K = 4 steps over them are ONE
// K = 16 MFMA per tap and c-tile.  The partials stay fp32
template <int ST, bool PLANAR, int PR = 0>
__global__ __launch_bounds__(NT) void yl_stem_wgrad_kernel(WgP P) {
  typedef Win<ST> W;
  constexpr int WE = W::WE, PTC = PLANAR ? 1 : GC / 16;
  __shared__ __attribute__((aligned(16))) float xw[WE * WE * GXS];
  __shared__ __attribute__((aligned(16))) float dzt[ST_T * ST_T * GDS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, kq = lane >> 4, i = lane & 15;
  const int c0 = blockIdx.x * GC, n0 = blockIdx.y * GN;
  const int tbeg = blockIdx.z * P.tps;
  const int tend = tbeg + P.tps < P.ntiles ? tbeg + P.tps : P.ntiles;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[9][PTC];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int pt = 0; pt < PTC; ++pt) acc[tap][pt] = zero;
  if constexpr (PLANAR) {                // channels 4 .. 15 of the window stay zero
    for (int item = t; item < WE * WE * (GXS / 4); item += NT) st4(&xw[item * 4], zero);
  }
  for (int tile = tbeg; tile < tend; ++tile) {
    const int b = tile / (P.TX * P.TX), tr = tile - b * P.TX * P.TX, ty0 = (tr / P.TX) * ST_T, tx0 = (tr % P.TX) * ST_T;
    const int sy0 = ty0 * ST - 1, sx0 = tx0 * ST - 1;
    __syncthreads();                     // the previous tile's reads (the zero fill) are done
    if constexpr (PLANAR) {
      for (int item = t; item < 4 * WE * WE; item += NT) {
        const int c = item / (WE * WE), pw = item - c * (WE * WE), wy = pw / WE, wx = pw - wy * WE;
        const int gy = sy0 + wy, gx = sx0 + wx;
        float v = 0.f;
        if (c < P.Cs && gy >= 0 && gy < P.S && gx >= 0 && gx < P.S) v = P.x[(((long)b * P.Cs + c) * P.S + gy) * P.S + gx];
        if constexpr (PR != 0) v = rne1<PR>(v);
        xw[W::gat(wy, wx) * GXS + c] = v;
      }
    } else {
      for (int item = t; item < WE * WE * (GC / 4); item += NT) {
        const int pw = item / (GC / 4), q = (item - pw * (GC / 4)) * 4, wy = pw / WE, wx = pw - wy * WE;
        const int gy = sy0 + wy, gx = sx0 + wx;
        const bool ok = gy >= 0 && gy < P.S && gx >= 0 && gx < P.S && c0 + q < P.Cs;
        if constexpr (PR == 0)
          st4(&xw[W::gat(wy, wx) * GXS + q], ok ? ld4(P.x + (((long)b * P.S + gy) * P.S + gx) * P.Cs + c0 + q) : zero);
        else
          st4(&xw[W::gat(wy, wx) * GXS + q], ok ? rne4<PR>(ld4(P.x + (((long)b * P.S + gy) * P.S + gx) * P.Cs + c0 + q)) : zero);
      }
    }
    for (int item = t; item < ST_T * ST_T * (GN / 4); item += NT) {
      const int pk = item / (GN / 4), q = (item - pk * (GN / 4)) * 4;
      const int gy = ty0 + (pk >> 3), gx = tx0 + (pk & 7);
      const bool ok = gy < P.So && gx < P.So && n0 + q < P.N;
      if constexpr (PR == 0)
        st4(&dzt[pk * GDS + q], ok ? ld4(P.dz + (((long)b * P.So + gy) * P.So + gx) * P.N + n0 + q) : zero);
      else
        st4(&dzt[pk * GDS + q], ok ? rne4<PR>(ld4(P.dz + (((long)b * P.So + gy) * P.So + gx) * P.N + n0 + q)) : zero);
    }
    __syncthreads();
#pragma unroll 1
    for (int step = 0; step < 4; ++step) {
      const int prow = 2 * step + (kq >> 1), pcol = 4 * (kq & 1);     // pixel 16 step + 4 kq + s: (prow, pcol + s)
      float qv[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) qv[s] = dzt[(prow * ST_T + pcol + s) * GDS + 16 * wave + i];
      if constexpr (PR == 0) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const float* xb = xw + W::gat(ST * prow + ky, ST * (pcol + s) + kx) * GXS + i;
#pragma unroll
            for (int pt = 0; pt < PTC; ++pt)
              acc[tap][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[16 * pt], qv[s], acc[tap][pt], 0, 0, 0);
          }
        }
      } else {
        typedef typename Frag16<PR>::T H;
        const f32x4 qf = {qv[0], qv[1], qv[2], qv[3]};
        const H qh = __builtin_convertvector(qf, H);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
          for (int pt = 0; pt < PTC; ++pt) {
            f32x4 xf;
#pragma unroll
            for (int s = 0; s < 4; ++s) xf[s] = xw[W::gat(ST * prow + ky, ST * (pcol + s) + kx) * GXS + i + 16 * pt];
            acc[tap][pt] = mfma16(__builtin_convertvector(xf, H), qh, acc[tap][pt]);
          }
        }
      }
    }
  }
  const int n = n0 + 16 * wave + i;
  if (n >= P.N) return;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int pt = 0; pt < PTC; ++pt) {
      const int c = c0 + 16 * pt + 4 * kq;
      if (c < P.Cp) st4(P.part + (((long)blockIdx.z * 9 + tap) * P.N + n) * P.Cp + c, acc[tap][pt]);
    }
}
// the partials summed in split order in float64 -> dW in PyTorch layout [N][Cs][3][3]; one thread per element
__global__ __launch_bounds__(NT) void yl_stem_wsum_kernel(const float* __restrict__ part, int splits, int N, int Cs, int Cp,
                                                         float* __restrict__ out) {
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  if (idx >= 9L * N * Cs) return;
  const long nc = idx / 9;
  const int tap = (int)(idx - nc * 9), n = (int)(nc / Cs), c = (int)(nc - (long)n * Cs);
  double s = 0;
  for (int z = 0; z < splits; ++z) s += (double)part[(((long)z * 9 + tap) * N + n) * Cp + c];
  out[idx] = (float)s;
}

// ---- the 1x1 units that stride or read the planar image: accessors of the heads' GEMM.  Row m of the unit's OUTPUT
// (b, i, j) reads / writes source pixel (b, st i, st j)
struct SrcGeom { int C, Sin, Sout, st, planar; };
__device__ __forceinline__ long src_off(const SrcGeom& g, int m, int c) {
  const int SS = g.Sout * g.Sout, b = m / SS, ij = m - b * SS, i = ij / g.Sout, j = ij - i * g.Sout;
  const int y = i * g.st, x = j * g.st;
  return g.planar ? (((long)b * g.C + c) * g.Sin + y) * g.Sin + x : (((long)b * g.Sin + y) * g.Sin + x) * g.C + c;
}
struct SrcRows {                         // (m, c)
  const float* p; SrcGeom g;
  __device__ __forceinline__ f32x4 load4(int idx, int r, int NI, int NR) const {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (idx < NI) {
#pragma unroll
      for (int s = 0; s < 4; ++s) if (r + s < NR) v[s] = p[src_off(g, idx, r + s)];
    }
    return v;
  }
};
struct SrcCols {                         // (c, m)
  const float* p; SrcGeom g;
  __device__ __forceinline__ f32x4 load4(int idx, int r, int NI, int NR) const {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (idx < NI) {
#pragma unroll
      for (int s = 0; s < 4; ++s) if (r + s < NR) v[s] = p[src_off(g, r + s, idx)];
    }
    return v;
  }
};
struct OutPix {                          // the input gradient of a strided 1x1: NHWC, the other pixels were zeroed
  float* c; SrcGeom g;
  __device__ __forceinline__ void store(int p, int q, f32x4 v, int NP, int NQ, int) const {
    if (q < NQ && p < NP) st4(c + src_off(g, q, p), v);
  }
};

int pick_conv_pt(int N) {                // 16 PT output channels per workgroup: the PT of {4, 3, 2} that pads N least
  int best = 4;
  for (int pt = 3; pt >= 2; --pt)
    if (ceil_div(N, 16 * pt) * pt < ceil_div(N, 16 * best) * best) best = pt;
  return best;
}

template <int ST, bool PLANAR, int PR>
void launch_conv_st(hipStream_t s, const ConvP& P, int B) {
  const int pt = pick_conv_pt(P.N);
  const dim3 grid(B * P.TY * P.TXn, ceil_div(P.N, 16 * pt)), blk(NT);
  if (pt == 2) hipLaunchKernelGGL((yl_stem_conv_kernel<ST, 2, PLANAR, PR>), grid, blk, 0, s, P);
  else if (pt == 3) hipLaunchKernelGGL((yl_stem_conv_kernel<ST, 3, PLANAR, PR>), grid, blk, 0, s, P);
  else hipLaunchKernelGGL((yl_stem_conv_kernel<ST, 4, PLANAR, PR>), grid, blk, 0, s, P);
}
template <int PR>
void launch_conv_in(hipStream_t s, const ConvP& P, int B, int st, bool planar) {
  if (st == 1 && !planar) launch_conv_st<1, false, PR>(s, P, B);
  else if (st == 1) launch_conv_st<1, true, PR>(s, P, B);
  else if (!planar) launch_conv_st<2, false, PR>(s, P, B);
  else launch_conv_st<2, true, PR>(s, P, B);
}
// `mode`: the operand type (0 fp32, 1 fp16, 2 bf16); P.wp is a pack launch_pack wrote in the same mode
void launch_conv(hipStream_t s, const ConvP& P, int B, int st, bool planar, int mode) {
  if (mode == 1) launch_conv_in<1>(s, P, B, st, planar);
  else if (mode == 2) launch_conv_in<2>(s, P, B, st, planar);
  else launch_conv_in<0>(s, P, B, st, planar);
}
void launch_pack(hipStream_t s, const float* w, float* wp, int A, int Bn, int Bp, int T, const PackP& tp, int mode) {
  const dim3 grid(ceil_div((long)tp.ntap * A * Bp, NT)), blk(NT);
  if (mode == 1) hipLaunchKernelGGL(yl_stem_pack16_kernel<1>, grid, blk, 0, s, w, (_Float16*)wp, A, Bn, Bp, T, tp);
  else if (mode == 2) hipLaunchKernelGGL(yl_stem_pack16_kernel<2>, grid, blk, 0, s, w, (__bf16*)wp, A, Bn, Bp, T, tp);
  else hipLaunchKernelGGL(yl_stem_pack_kernel, grid, blk, 0, s, w, wp, A, Bn, Bp, T, tp);
}
// packed tap `tap` of a pack of `per` elements a tap: 4 bytes an element in fp32, 2 in the 16-bit modes
inline const float* pack_tap(const float* wp, long tap, long per, int mode) {
  return (const float*)((const char*)wp + tap * per * (mode ? 2 : 4));
}

// 3x3 forward: 2 launches (pack, convolution).  wpack: 9 cout round4(cin) floats
int conv3_forward(hipStream_t s, const float* x, const float* w, float* wpack, float* z, int st, int B, int Sin, int Sout,
                  int cin, int cout, bool planar, int mode) {
  const int cp = round4(cin);
  PackP tp;
  tp.ntap = 9;
  for (int t = 0; t < 9; ++t) { tp.ky[t] = t / 3; tp.kx[t] = t % 3; }
  launch_pack(s, w, wpack, cout, cin, cp, 0, tp, mode);
  ConvP P;
  P.src = x; P.wp = wpack; P.dst = z;
  P.Ss = Sin; P.Cs = cin; P.Cp = cp; P.N = cout; P.Sd = Sout;
  P.TY = P.TXn = ceil_div(Sout, ST_T); P.ey = P.ex = Sout;
  P.os = 1; P.poy = P.pox = 0; P.o0 = -1; P.nty = P.ntx = 3;
  launch_conv(s, P, B, st, planar, mode);
  return 2;
}
// the parity classes of a stride-2 input gradient that have pixels: 4 if S >= 2, else 1
inline int dgrad_classes(int S) { return S >= 2 ? 4 : 1; }
// 3x3 input gradient: stride 1: 2 launches; stride 2: 1 + dgrad_classes(Sin).  wpack: 9 cin cout floats
int conv3_dgrad(hipStream_t s, const float* dz, const float* w, float* wpack, float* dx, int st, int B, int Sin, int Sout,
                int cin, int cout, int mode) {
  ConvP P;
  P.src = dz; P.dst = dx;
  P.Ss = Sout; P.Cs = cout; P.Cp = cout; P.N = cin; P.Sd = Sin;
  PackP tp;
  tp.ntap = 9;
  if (st == 1) {
    for (int t = 0; t < 9; ++t) { tp.ky[t] = 2 - t / 3; tp.kx[t] = 2 - t % 3; }
    launch_pack(s, w, wpack, cin, cout, cout, 1, tp, mode);
    P.wp = wpack;
    P.TY = P.TXn = ceil_div(Sin, ST_T); P.ey = P.ex = Sin;
    P.os = 1; P.poy = P.pox = 0; P.o0 = -1; P.nty = P.ntx = 3;
    launch_conv(s, P, B, 1, false, mode);
    return 2;
  }
  int o = 0, first[4];                   // the classes' taps, one after the other: 1 + 2 + 2 + 4 = 9
  for (int pi = 0; pi < 2; ++pi)
    for (int pj = 0; pj < 2; ++pj) {
      first[pi * 2 + pj] = o;
      for (int ty = 0; ty <= pi; ++ty)
        for (int tx = 0; tx <= pj; ++tx) { tp.ky[o] = pi ? 2 - 2 * ty : 1; tp.kx[o] = pj ? 2 - 2 * tx : 1; ++o; }
    }
  launch_pack(s, w, wpack, cin, cout, cout, 1, tp, mode);
  int nl = 1;
  for (int pi = 0; pi < 2; ++pi)
    for (int pj = 0; pj < 2; ++pj) {
      P.ey = (Sin - pi + 1) / 2; P.ex = (Sin - pj + 1) / 2;
      if (P.ey < 1 || P.ex < 1) continue;
      P.wp = pack_tap(wpack, first[pi * 2 + pj], (long)cin * cout, mode);
      P.TY = ceil_div(P.ey, ST_T); P.TXn = ceil_div(P.ex, ST_T);
      P.os = 2; P.poy = pi; P.pox = pj; P.o0 = 0; P.nty = 1 + pi; P.ntx = 1 + pj;
      launch_conv(s, P, B, 1, false, mode);
      ++nl;
    }
  return nl;
}
// the cut of a 3x3 weight gradient: whole spatial tiles per split, about 1024 workgroups in all
void wgrad3_plan(int B, int Sout, int cin, int cout, int* tps, int* splits) {
  const int ntiles = B * ceil_div(Sout, ST_T) * ceil_div(Sout, ST_T);
  const int blocks = ceil_div(round4(cin), GC) * ceil_div(cout, GN);
  int want = 1024 / blocks;
  want = want < 1 ? 1 : (want > ntiles ? ntiles : want);
  *tps = ceil_div(ntiles, want);
  *splits = ceil_div(ntiles, *tps);
}
template <int PR>
void launch_wgrad(hipStream_t s, dim3 grid, const WgP& P, int st, bool planar) {
  const dim3 blk(NT);
  if (st == 1 && !planar) hipLaunchKernelGGL((yl_stem_wgrad_kernel<1, false, PR>), grid, blk, 0, s, P);
  else if (st == 1) hipLaunchKernelGGL((yl_stem_wgrad_kernel<1, true, PR>), grid, blk, 0, s, P);
  else if (!planar) hipLaunchKernelGGL((yl_stem_wgrad_kernel<2, false, PR>), grid, blk, 0, s, P);
  else hipLaunchKernelGGL((yl_stem_wgrad_kernel<2, true, PR>), grid, blk, 0, s, P);
}
// 3x3 weight gradient: 2 launches (partials, ordered sum).  part: splits 9 cout round4(cin) floats
int conv3_wgrad(hipStream_t s, const float* x, const float* dz, float* part, float* dw, int st, int B, int Sin, int Sout,
                int cin, int cout, bool planar, int tps, int splits, int mode) {
  WgP P;
  P.x = x; P.dz = dz; P.part = part;
  P.S = Sin; P.So = Sout; P.Cs = cin; P.Cp = round4(cin); P.N = cout;
  P.TX = ceil_div(Sout, ST_T); P.ntiles = B * P.TX * P.TX; P.tps = tps;
  const dim3 grid(ceil_div(P.Cp, GC), ceil_div(cout, GN), splits), blk(NT);
  if (mode == 1) launch_wgrad<1>(s, grid, P, st, planar);
  else if (mode == 2) launch_wgrad<2>(s, grid, P, st, planar);
  else launch_wgrad<0>(s, grid, P, st, planar);
  hipLaunchKernelGGL(yl_stem_wsum_kernel, dim3(ceil_div(9L * cout * cin, NT)), blk, 0, s, (const float*)part, splits, cout, cin,
                     P.Cp, dw);
  return 2;
}

// ---- 1x1: the heads' GEMM.  Stride 1 on NHWC rows launches what yl_stage.hip launches
int conv1_forward(hipStream_t s, const float* x, const float* w, float* z, int st, int B, int Sin, int Sout, int cin, int cout,
                  bool planar, int mode) {
  const int M = B * Sout * Sout;
  if (st == 1 && !planar) launch_gemm_in<true>(mode, s, RowsScalar{w, cin}, RowsVec{x, cin}, OutRowsVec{z, cout}, cout, M, cin, cin, 1);
  else launch_gemm_in<true>(mode, s, RowsScalar{w, cin}, SrcRows{x, SrcGeom{cin, Sin, Sout, st, planar ? 1 : 0}}, OutRowsVec{z, cout}, cout, M,
                            cin, cin, 1);
  return 1;
}
// stride 2: dx is zeroed (a memset, not counted) and the rows land on its even pixels
int conv1_dgrad(hipStream_t s, const float* dz, const float* w, float* dx, int st, int B, int Sin, int Sout, int cin, int cout,
                int mode) {
  const int M = B * Sout * Sout;
  if (st == 1) {
    launch_gemm_in<true>(mode, s, ColsScalar{w, cin}, RowsVec{dz, cout}, OutRowsVec{dx, cin}, cin, M, cout, cout, 1);
  } else {
    hipMemsetAsync(dx, 0, (size_t)B * Sin * Sin * cin * 4, s);
    launch_gemm_in<true>(mode, s, ColsScalar{w, cin}, RowsVec{dz, cout}, OutPix{dx, SrcGeom{cin, Sin, Sout, st, 0}}, cin, M, cout, cout, 1);
  }
  return 1;
}
int conv1_wgrad(hipStream_t s, const float* x, const float* dz, float* part, float* dw, int st, int B, int Sin, int Sout, int cin,
                int cout, bool planar, int rows, int splits, int mode) {
  const int M = B * Sout * Sout;
  if (st == 1 && !planar)
    launch_gemm_in<true>(mode, s, ColsScalar{x, cin}, ColsScalar{dz, cout}, OutPartial{part, (long)cin * cout}, cin, cout, M, rows, splits);
  else
    launch_gemm_in<true>(mode, s, SrcCols{x, SrcGeom{cin, Sin, Sout, st, planar ? 1 : 0}}, ColsScalar{dz, cout},
                         OutPartial{part, (long)cin * cout}, cin, cout, M, rows, splits);
  HeadRows none;
  memset(&none, 0, sizeof(none));
  hipLaunchKernelGGL(yl_head_wsum_kernel, dim3(ceil_div((long)cin * cout, NT)), dim3(NT), 0, s, (const float*)part, splits, cin,
                     cout, dw, none, 0);
  return 2;
}

// ---- the stack as units (yl_units.h: Unit).  The row reductions run over at most STAT_TILES_MAX tiles of stat_rows rows
bool cfg_ok(const yl_stem_cfg* c) {
  if (!c || c->num_units < 1 || c->num_units > YL_STEM_MAX_UNITS || !(c->eps > 0)) return false;
  if (c->input_nchw != 0 && c->input_nchw != 1) return false;
  if (c->input_nchw) {
    if (c->in_channels < 1 || c->in_channels > 4) return false;
  } else if (c->in_channels < 4 || (c->in_channels & 3)) {
    return false;
  }
  for (int i = 0; i < c->num_units; ++i) {
    const yl_stem_unit_cfg& u = c->unit[i];
    if ((u.k != 1 && u.k != 3) || (u.s != 1 && u.s != 2) || u.cout < 4 || (u.cout & 3)) return false;
  }
  return true;
}

// the rows of one statistics tile: multiples of STAT_ROWS until at most STAT_TILES_MAX tiles cover M rows
inline int stat_rows_of(int64_t M) { return STAT_ROWS * ceil_div(ceil_div(M, STAT_ROWS), STAT_TILES_MAX); }

// every unit is a block of its own: ReLU, no residual
int make_units(const yl_stem_cfg& cfg, int B, int S, Unit* us) {
  int cin = cfg.in_channels;
  for (int i = 0; i < cfg.num_units; ++i) {
    const yl_stem_unit_cfg& c = cfg.unit[i];
    Unit& u = us[i];
    u.block = i; u.slot = 0; u.dw = 0; u.act = ACT_RELU; u.first = u.last = 1; u.res = 0;
    u.k = c.k; u.st = c.s; u.cin = cin; u.cout = c.cout; u.Sin = S; u.Sout = out_size(S, c.k, c.s);
    u.pb = pad_begin(c.k, c.s, S, 0);
    u.planar = i == 0 && cfg.input_nchw;
    u.Min = (int64_t)B * S * S; u.Mout = (int64_t)B * u.Sout * u.Sout;
    u.stat_rows = stat_rows_of(u.Mout); u.tiles = ceil_div(u.Mout, u.stat_rows);
    u.wrows = u.wsplits = 0;
    if (u.Mout < ((int64_t)1 << 31)) {
      if (u.k == 1) split_plan((int)u.Mout, cin, c.cout, &u.wrows, &u.wsplits);
      else wgrad3_plan(B, u.Sout, cin, c.cout, &u.wrows, &u.wsplits);
    }
    S = u.Sout; cin = c.cout;
  }
  return cfg.num_units;
}

// units and sizes of cfg at (B, S): what yl_stem_plan reports and the walk runs on
yl_status layout(const yl_stem_cfg& cfg, int B, int S, Unit* us, int* n, Sizes* z) {
  *n = make_units(cfg, B, S, us);
  const int64_t M0 = (int64_t)B * S * S, x0 = M0 * cfg.in_channels * 4;
  if (M0 >= ((int64_t)1 << 31) || x0 >= ((int64_t)1 << 42)) return YL_ERR_UNSUPPORTED;
  if (!unit_sizes(us, *n, 1 << 16, z)) return YL_ERR_UNSUPPORTED;
  for (int i = 0; i < *n; ++i)
    if (us[i].k == 1 && us[i].Mout > (int64_t)65535 * GEMM_ROWS) return YL_ERR_UNSUPPORTED;   // the GEMM's grid.y
  z->x0 = x0; z->xsave = round16(x0); z->gmax = z->amax;
  return YL_OK;
}

int resolve(const yl_stem_cfg& cfg, const yl_stem_tensors* t, const yl_stage_unit** tab) {
  for (int i = 0; i < cfg.num_units; ++i) tab[i] = &t->unit[i];
  return cfg.num_units;
}

// what yl_units.h's walk launches for this stack: the 3x3 convolution, or the heads' GEMM for a 1x1 unit
struct StemPolicy {
  static constexpr int ROT = 2;
  static constexpr bool MIXED = false;   // every unit has its ReLU and no block a residual
  static constexpr bool RELU6 = false;
  template <class H> static yl_status layout(const H& h, int B, int S, Unit* us, int* n, Sizes* z) { return ::layout(h.cfg, B, S, us, n, z); }
  static int conv_forward(hipStream_t s, const Unit& u, int B, const float* x, const float* w, float* z, const UnitBuffers& sb,
                          int mode) {
    return u.k == 3 ? conv3_forward(s, x, w, sb.wpack, z, u.st, B, u.Sin, u.Sout, u.cin, u.cout, u.planar, mode)
                    : conv1_forward(s, x, w, z, u.st, B, u.Sin, u.Sout, u.cin, u.cout, u.planar, mode);
  }
  static int conv_wgrad(hipStream_t s, const Unit& u, int B, const float* x, const float* dz, float* dw, const UnitBuffers& sb,
                        int mode) {
    return u.k == 3 ? conv3_wgrad(s, x, dz, sb.wpart, dw, u.st, B, u.Sin, u.Sout, u.cin, u.cout, u.planar, u.wrows, u.wsplits, mode)
                    : conv1_wgrad(s, x, dz, sb.wpart, dw, u.st, B, u.Sin, u.Sout, u.cin, u.cout, u.planar, u.wrows, u.wsplits, mode);
  }
  static int conv_dgrad(hipStream_t s, const Unit& u, int B, const float* dz, const float* w, float* dx, const UnitBuffers& sb,
                        int mode) {
    return u.k == 3 ? conv3_dgrad(s, dz, w, sb.wpack, dx, u.st, B, u.Sin, u.Sout, u.cin, u.cout, mode)
                    : conv1_dgrad(s, dz, w, dx, u.st, B, u.Sin, u.Sout, u.cin, u.cout, mode);
  }
};

}  // namespace

struct yl_stem : UnitStack<yl_stem_cfg> {};

extern "C" {

yl_status yl_stem_plan(const yl_stem_cfg* cfg, int32_t batch, int32_t size, yl_stem_plan_info* out) {
  if (!cfg_ok(cfg) || !out || batch < 1 || size < 1) return YL_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  out->stat_rows = STAT_ROWS; out->gemm_rows = GEMM_ROWS; out->conv_tile = ST_T; out->stat_tiles_max = STAT_TILES_MAX;
  Unit us[MAX_UNITS];
  Sizes z;
  int n;
  const yl_status st = layout(*cfg, batch, size, us, &n, &z);
  if (st != YL_OK) return st;
  for (int i = 0; i < n; ++i) {
    const Unit& u = us[i];
    yl_stem_unit_plan& p = out->unit[i];
    p.size_in = u.Sin; p.size_out = u.Sout; p.rows_out = (int32_t)u.Mout;
    p.stat_rows = u.stat_rows; p.stat_tiles = u.tiles; p.wgrad_rows = u.wrows; p.wgrad_splits = u.wsplits;
    p.conv_block = u.k == 3 ? 16 * pick_conv_pt(u.cout) : 0;
    p.saved_bytes = unit_saved_bytes(u);
  }
  const ArenaBytes b = arena_bytes(us, n, z, StemPolicy::ROT);
  out->saved_bytes = b.saved; out->nosave_bytes = b.nosave; out->workspace_bytes = b.work;
  return YL_OK;
}

yl_status yl_stem_create(int32_t device, const yl_stem_cfg* cfg, yl_stem** out) {
  return units_create(device, cfg, cfg_ok(cfg), out);
}

void yl_stem_destroy(yl_stem* h) { units_destroy(h); }

yl_status yl_stem_held(const yl_stem* h, int64_t* saved_bytes, int64_t* workspace_bytes, int32_t* forward_held) {
  return units_held(h, saved_bytes, workspace_bytes, forward_held);
}

yl_status yl_amp_stem_set(yl_stem* h, uint32_t mode) { return units_amp_set(h, mode); }

yl_status yl_amp_stem_get(const yl_stem* h, uint32_t* mode, uint32_t* held_mode) { return units_amp_get(h, mode, held_mode); }

yl_status yl_stem_forward(yl_stem* h, const yl_stem_tensors* params, const float* x_dev, int32_t batch, int32_t size,
                          uint32_t flags, float* out_dev, void* stream, int32_t* launches) {
  if (!h || !x_dev || !out_dev || batch < 1 || size < 1 || !params) return YL_ERR_INVALID;
  const yl_stage_unit* par[MAX_UNITS];
  const int n = resolve(h->cfg, params, par);
  return units_forward<StemPolicy>(h, par, n, x_dev, h->cfg.input_nchw ? 3u : 15u, batch, size, flags, out_dev, stream, launches);
}

yl_status yl_stem_backward(yl_stem* h, const yl_stem_tensors* params, const yl_stem_tensors* grads, const float* gy_dev,
                           float* dx_dev, void* stream, int32_t* launches) {
  if (!h || !grads || !gy_dev || !params) return YL_ERR_INVALID;
  if (dx_dev && h->cfg.input_nchw) return YL_ERR_INVALID;  // the planar image has no gradient
  const yl_stage_unit *par[MAX_UNITS], *grd[MAX_UNITS];
  const int n = resolve(h->cfg, params, par);
  resolve(h->cfg, grads, grd);
  return units_backward<StemPolicy>(h, par, grd, n, gy_dev, dx_dev, stream, launches);
}

yl_status yl_amp_stem_conv(const float* a_dev, const float* b_dev, float* out_dev, int32_t pass, int32_t k, int32_t stride,
                           int32_t batch, int32_t size, int32_t cin, int32_t cout, int32_t input_nchw, uint32_t mode_flag,
                           void* stream, int32_t* launches) {
  const int mode = mode_of_bits(mode_flag);
  if (mode < 0) return YL_ERR_INVALID;
  if (!a_dev || !b_dev || !out_dev || batch < 1 || size < 1 || cout < 4 || (cout & 3)) return YL_ERR_INVALID;
  if ((k != 1 && k != 3) || (stride != 1 && stride != 2)) return YL_ERR_INVALID;
  if (pass != YL_STAGE_PASS_FORWARD && pass != YL_STAGE_PASS_DGRAD && pass != YL_STAGE_PASS_WGRAD) return YL_ERR_INVALID;
  if (input_nchw != 0 && input_nchw != 1) return YL_ERR_INVALID;
  if (input_nchw ? (cin < 1 || cin > 4 || pass == YL_STAGE_PASS_DGRAD) : (cin < 4 || (cin & 3))) return YL_ERR_INVALID;
  const bool wg = pass == YL_STAGE_PASS_WGRAD, planar = input_nchw != 0;
  // the weight (b of FORWARD / DGRAD, out of WGRAD) and the planar image at any 4-byte boundary, every other tensor at 16
  if (((uintptr_t)a_dev & ((planar && pass != YL_STAGE_PASS_DGRAD) ? 3u : 15u)) || ((uintptr_t)b_dev & (wg ? 15u : 3u)) ||
      ((uintptr_t)out_dev & (wg ? 3u : 15u)))
    return YL_ERR_UNSUPPORTED;
  const int So = out_size(size, k, stride);
  const int64_t M = (int64_t)batch * size * size, Mo = (int64_t)batch * So * So;
  const int big = cin > cout ? cin : cout;
  if (M * big >= ((int64_t)1 << 40) || M >= ((int64_t)1 << 31) || big > (1 << 16)) return YL_ERR_UNSUPPORTED;
  if (k == 1 && Mo > (int64_t)65535 * GEMM_ROWS) return YL_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  int rows = 0, splits = 0;
  int64_t bytes = 16;
  if (wg) {
    if (k == 1) { split_plan((int)Mo, cin, cout, &rows, &splits); bytes = round16((int64_t)splits * cin * cout * 4); }
    else { wgrad3_plan(batch, So, cin, cout, &rows, &splits); bytes = round16((int64_t)splits * 9 * cout * round4(cin) * 4); }
  } else if (k == 3) {
    bytes = round16((int64_t)9 * cout * round4(cin) * 4);
  }
  float* tmp = nullptr;
  if (hipMalloc((void**)&tmp, (size_t)bytes) != hipSuccess) {
    (void)hipGetLastError();
    return YL_ERR_NOMEM;
  }
  int nl = 0;
  if (pass == YL_STAGE_PASS_FORWARD)
    nl = k == 3 ? conv3_forward(s, a_dev, b_dev, tmp, out_dev, stride, batch, size, So, cin, cout, planar, mode)
                : conv1_forward(s, a_dev, b_dev, out_dev, stride, batch, size, So, cin, cout, planar, mode);
  else if (pass == YL_STAGE_PASS_DGRAD)
    nl = k == 3 ? conv3_dgrad(s, a_dev, b_dev, tmp, out_dev, stride, batch, size, So, cin, cout, mode)
                : conv1_dgrad(s, a_dev, b_dev, out_dev, stride, batch, size, So, cin, cout, mode);
  else
    nl = k == 3 ? conv3_wgrad(s, a_dev, b_dev, tmp, out_dev, stride, batch, size, So, cin, cout, planar, rows, splits, mode)
                : conv1_wgrad(s, a_dev, b_dev, tmp, out_dev, stride, batch, size, So, cin, cout, planar, rows, splits, mode);
  const bool ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  hipFree(tmp);
  if (launches) *launches = nl;
  return ok ? YL_OK : YL_ERR_HIP;
}

yl_status yl_stem_conv(const float* a_dev, const float* b_dev, float* out_dev, int32_t pass, int32_t k, int32_t stride,
                       int32_t batch, int32_t size, int32_t cin, int32_t cout, int32_t input_nchw, void* stream,
                       int32_t* launches) {
  return yl_amp_stem_conv(a_dev, b_dev, out_dev, pass, k, stride, batch, size, cin, cout, input_nchw, 0u, stream, launches);
}

}  // extern "C"
