// Trainable backbone stage: a stack of MobileNetV4 UIB blocks (timm UniversalInvertedResidual) and 1x1 ConvBnAct blocks,
// forward and backward on NHWC fp32 rows (include/yololite_hip.h, yl_stage_*).
//
// The stack is flattened into UNITS, each a bias-free convolution and its BatchNorm:
//   unit u:  z = conv(x_u)   h = bn(z) [relu] [+ the block's input, behind the last unit of a residual block]
// x_u is the previous unit's h (the caller's x for unit 0).  A depthwise unit is k x k with stride 1 or 2; a 1x1 unit is
// the heads' GEMM (yl_block.h: launch_gemm<0> with its accessors) in all three passes.  With YL_HEAD_SAVE the handle keeps
// a copy of x and every unit's z, h and (mean, invstd).
// The backward walks the units last first.  Three gradient buffers rotate: a residual block's output gradient G stays in
// one of them until the block's input gradient exists and is then added to it; the other two carry dz and the unit's
// input gradient.  What yl_block.h has is used as it is (GEMM, weight-gradient sum, BatchNorm gradient sums, Arena); the
// kernels here are the ones it lacks: depthwise k x k with stride in three passes, BatchNorm with and without ReLU with
// eps from the configuration, and the add.
#include <new>

#include "yl_bn.h"

namespace {

// ---- depthwise K x K, pad (K - 1) / 2, stride ST, weight [C][1][K][K].  x: [B][Sx][Sx][C], y: [B][So][So][C].
// GRAD = false: y = conv(x); a thread owns one OUTPUT pixel x 4 channels.  GRAD = true: `src` is dy, `dst` is dx; a thread
// owns one INPUT pixel (i, j) x 4 channels and sums, ky then kx ascending, the taps whose (i + p - ky) is a multiple of ST
// (output row (i + p - ky) / ST): the transposed convolution as a gather.  fp32 sum from zero in tap order either way.
template <int K, int ST, bool GRAD>
__global__ __launch_bounds__(NT) void yl_stage_dw_kernel(const float* __restrict__ src, const float* __restrict__ w,
                                                        float* __restrict__ dst, int B, int Sx, int So, int C) {
  constexpr int P = (K - 1) / 2;
  const int C4 = C >> 2;
  const int T = GRAD ? Sx : So, R = GRAD ? So : Sx;         // extent of the pixels the threads own / of the map read
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  if (idx >= (long)B * T * T * C4) return;
  const int m = (int)(idx / C4), c = (int)(idx - (long)m * C4) * 4;
  const int TT = T * T, b = m / TT, ij = m - b * TT, i = ij / T, j = ij - i * T;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ky = 0; ky < K; ++ky) {
    int yy;
    if (!GRAD) {
      yy = i * ST + ky - P;
    } else {
      const int t = i + P - ky;
      if (t < 0 || (ST == 2 && (t & 1))) continue;
      yy = t / ST;
    }
    if (yy < 0 || yy >= R) continue;
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      int xx;
      if (!GRAD) {
        xx = j * ST + kx - P;
      } else {
        const int t = j + P - kx;
        if (t < 0 || (ST == 2 && (t & 1))) continue;
        xx = t / ST;
      }
      if (xx < 0 || xx >= R) continue;
      const f32x4 v = ld4(src + ((long)(b * R + yy) * R + xx) * C + c);
      const int t = ky * K + kx;
      const f32x4 wv = {w[(c + 0) * (K * K) + t], w[(c + 1) * (K * K) + t], w[(c + 2) * (K * K) + t], w[(c + 3) * (K * K) + t]};
      acc = acc + v * wv;
    }
  }
  st4(dst + (long)m * C + c, acc);
}

// depthwise weight gradient partials: part[tile][ky * K + kx][C] = sum over the tile's OUTPUT rows of dy[m][c] * x[tap][c].
// The workgroup and thread layout of the row reductions (yl_block.h); one ky row at a time, so K * 4 float64 sums per thread.
template <int K, int ST>
__global__ __launch_bounds__(NT) void yl_stage_dw_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                              double* __restrict__ part, int Mo, int Sx, int So, int C, int CQ) {
  constexpr int P = (K - 1) / 2;
  __shared__ double red[NT][K * 4];
  const int t = threadIdx.x, cq = t & (CQ - 1), rs = t / CQ, RS = NT / CQ;
  const int c = (blockIdx.y * CQ + cq) * 4;
  const bool on = c < C;
  const int SS = So * So;
  const int m0 = blockIdx.x * STAT_ROWS, m1 = m0 + STAT_ROWS < Mo ? m0 + STAT_ROWS : Mo;
  for (int ky = 0; ky < K; ++ky) {
    double acc[K][4] = {};
    if (on)
      for (int m = m0 + rs; m < m1; m += RS) {
        const int b = m / SS, ij = m - b * SS, i = ij / So, j = ij - i * So, yy = i * ST + ky - P;
        if (yy < 0 || yy >= Sx) continue;
        const f32x4 g = ld4(dy + (long)m * C + c);
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const int xx = j * ST + kx - P;
          if (xx < 0 || xx >= Sx) continue;
          const f32x4 v = ld4(x + ((long)(b * Sx + yy) * Sx + xx) * C + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[kx][e] += (double)g[e] * (double)v[e];
        }
      }
#pragma unroll
    for (int kx = 0; kx < K; ++kx)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[t][kx * 4 + e] = acc[kx][e];
    __syncthreads();
    if (rs == 0 && on) {
      for (int k = 1; k < RS; ++k)
#pragma unroll
        for (int e = 0; e < K * 4; ++e) red[t][e] += red[k * CQ + cq][e];
#pragma unroll
      for (int kx = 0; kx < K; ++kx)
#pragma unroll
        for (int e = 0; e < 4; ++e) part[((long)blockIdx.x * (K * K) + ky * K + kx) * C + c + e] = red[t][kx * 4 + e];
    }
    __syncthreads();
  }
}
__global__ __launch_bounds__(NT) void yl_stage_dw_wsum_kernel(const double* __restrict__ part, int tiles, int C, int KK,
                                                             float* __restrict__ out) {
  const int idx = blockIdx.x * NT + threadIdx.x;           // k * C + c
  if (idx >= KK * C) return;
  const int k = idx / C, c = idx - k * C;
  double s = 0;
  for (int t = 0; t < tiles; ++t) s += part[((long)t * KK + k) * C + c];
  out[c * KK + k] = (float)s;
}

// ---- BatchNorm: the column sums, the statistics, the normalisation and its backward are yl_bn.h, shared with yl_stem.hip
// the residual's backward: io += g
__global__ __launch_bounds__(NT) void yl_stage_add_kernel(float* io, const float* __restrict__ g, long n4) {
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  if (idx >= n4) return;
  st4(io + idx * 4, ld4(io + idx * 4) + ld4(g + idx * 4));
}

// ---- launches of one depthwise pass.  false: (k, stride) is not one of {3, 5} x {1, 2}
template <bool GRAD>
bool launch_dw(hipStream_t s, const float* src, const float* w, float* dst, int k, int st, int B, int Sx, int So, int C) {
  const long n = (long)B * (GRAD ? Sx : So) * (GRAD ? Sx : So) * (C >> 2);
  const dim3 grid(ceil_div(n, NT)), blk(NT);
  if (k == 3 && st == 1) hipLaunchKernelGGL((yl_stage_dw_kernel<3, 1, GRAD>), grid, blk, 0, s, src, w, dst, B, Sx, So, C);
  else if (k == 3 && st == 2) hipLaunchKernelGGL((yl_stage_dw_kernel<3, 2, GRAD>), grid, blk, 0, s, src, w, dst, B, Sx, So, C);
  else if (k == 5 && st == 1) hipLaunchKernelGGL((yl_stage_dw_kernel<5, 1, GRAD>), grid, blk, 0, s, src, w, dst, B, Sx, So, C);
  else if (k == 5 && st == 2) hipLaunchKernelGGL((yl_stage_dw_kernel<5, 2, GRAD>), grid, blk, 0, s, src, w, dst, B, Sx, So, C);
  else return false;
  return true;
}
// partials over `tiles` tiles of the B * So * So output rows, then their ordered sum into dw [C][1][k][k]: 2 launches
bool launch_dw_wgrad(hipStream_t s, const float* dy, const float* x, double* part, float* dw, int k, int st, int B, int Sx,
                     int So, int C, int tiles) {
  const int Mo = B * So * So, cq = pick_cq(C);
  const dim3 grid(tiles, ceil_div(C >> 2, cq)), blk(NT);
  if (k == 3 && st == 1) hipLaunchKernelGGL((yl_stage_dw_wgrad_kernel<3, 1>), grid, blk, 0, s, dy, x, part, Mo, Sx, So, C, cq);
  else if (k == 3 && st == 2) hipLaunchKernelGGL((yl_stage_dw_wgrad_kernel<3, 2>), grid, blk, 0, s, dy, x, part, Mo, Sx, So, C, cq);
  else if (k == 5 && st == 1) hipLaunchKernelGGL((yl_stage_dw_wgrad_kernel<5, 1>), grid, blk, 0, s, dy, x, part, Mo, Sx, So, C, cq);
  else if (k == 5 && st == 2) hipLaunchKernelGGL((yl_stage_dw_wgrad_kernel<5, 2>), grid, blk, 0, s, dy, x, part, Mo, Sx, So, C, cq);
  else return false;
  hipLaunchKernelGGL(yl_stage_dw_wsum_kernel, dim3(ceil_div((long)k * k * C, NT)), blk, 0, s, (const double*)part, tiles, C,
                     k * k, dw);
  return true;
}

// ---- the stack as units
struct Unit {
  int block, slot;                       // slot: 0 dw_start, 1 pw_exp (cn), 2 dw_mid, 3 pw_proj of yl_stage_block
  int dw, relu, k, st;                   // depthwise k x k of stride st, or (dw == 0) 1x1
  int cin, cout, Sin, Sout;
  int64_t Min, Mout;                     // rows of the unit's input and output
  int tiles, wrows, wsplits;             // tiles of STAT_ROWS output rows; the 1x1's weight-gradient cut
  int first, last, res;                  // first / last unit of its block; res: the block adds its input (set on both)
};
inline const yl_stage_unit& entry(const yl_stage_tensors* t, const Unit& u) {
  const yl_stage_block& b = t->block[u.block];
  return u.slot == 0 ? b.dw_start : (u.slot == 1 ? b.pw_exp : (u.slot == 2 ? b.dw_mid : b.pw_proj));
}

bool cfg_ok(const yl_stage_cfg* c) {
  if (!c || c->num_blocks < 1 || c->num_blocks > YL_STAGE_MAX_BLOCKS || !(c->eps > 0)) return false;
  if (c->in_channels < 4 || (c->in_channels & 3)) return false;
  for (int i = 0; i < c->num_blocks; ++i) {
    const yl_stage_block_cfg& b = c->block[i];
    if (b.cout < 4 || (b.cout & 3)) return false;
    if (b.type == YL_STAGE_CN) {
      if (b.a != 0 || b.k != 1 || b.s != 1) return false;
    } else if (b.type == YL_STAGE_UIR) {
      if ((b.a != 0 && b.a != 3 && b.a != 5) || (b.k != 0 && b.k != 3 && b.k != 5) || (b.s != 1 && b.s != 2)) return false;
      if (b.mid < 4 || (b.mid & 3)) return false;
      if (b.s == 2 && !b.a && !b.k) return false;          // no depthwise unit to carry the stride
    } else {
      return false;
    }
  }
  return true;
}

// the units of cfg at (B, S) -> their number; fills the per-block plan if `bp` is given.  cfg_ok(cfg) holds
int make_units(const yl_stage_cfg& cfg, int B, int S, Unit* us, yl_stage_block_plan* bp) {
  int n = 0, cin = cfg.in_channels;
  for (int i = 0; i < cfg.num_blocks; ++i) {
    const yl_stage_block_cfg& b = cfg.block[i];
    const bool cn = b.type == YL_STAGE_CN;
    const int mid = cn ? b.cout : b.mid;
    const int s0 = (b.a && !b.k) ? b.s : 1;
    const int Smid = (!cn && b.a) ? out_size(S, b.a, s0) : S;
    const int Sout = (!cn && b.k) ? out_size(Smid, b.k, b.s) : Smid;
    const int res = !cn && cin == b.cout && b.s == 1;
    const int n0 = n;
    auto add = [&](int slot, int dw, int relu, int k, int st, int ci, int co, int Si, int So) {
      Unit& u = us[n++];
      u.block = i; u.slot = slot; u.dw = dw; u.relu = relu; u.k = k; u.st = st; u.cin = ci; u.cout = co; u.Sin = Si; u.Sout = So;
      u.Min = (int64_t)B * Si * Si; u.Mout = (int64_t)B * So * So;
      u.tiles = ceil_div(u.Mout, STAT_ROWS);
      u.wrows = u.wsplits = 0;
      if (!dw && u.Mout < ((int64_t)1 << 31)) split_plan((int)u.Mout, ci, co, &u.wrows, &u.wsplits);
      u.first = u.last = 0; u.res = res;
    };
    if (!cn && b.a) add(0, 1, 0, b.a, s0, cin, cin, S, Smid);
    add(1, 0, 1, 1, 1, cin, mid, Smid, Smid);
    if (!cn && b.k) add(2, 1, 1, b.k, b.s, mid, mid, Smid, Sout);
    if (!cn) add(3, 0, 0, 1, 1, mid, b.cout, Sout, Sout);
    us[n0].first = 1; us[n - 1].last = 1;
    if (bp) {
      yl_stage_block_plan& p = bp[i];
      memset(&p, 0, sizeof(p));
      p.size_in = S; p.size_mid = Smid; p.size_out = Sout;
      p.rows_mid = (int32_t)((int64_t)B * Smid * Smid); p.rows_out = (int32_t)((int64_t)B * Sout * Sout);
      p.stat_tiles_mid = ceil_div((int64_t)B * Smid * Smid, STAT_ROWS); p.stat_tiles_out = ceil_div((int64_t)B * Sout * Sout, STAT_ROWS);
      p.units = n - n0;
      for (int u = n0; u < n; ++u) {
        p.saved_bytes += 2 * us[u].Mout * us[u].cout * 4 + 2 * (int64_t)us[u].cout * 4;
        if (us[u].slot == 1) { p.exp_rows = us[u].wrows; p.exp_splits = us[u].wsplits; }
        if (us[u].slot == 3) { p.proj_rows = us[u].wrows; p.proj_splits = us[u].wsplits; }
      }
    }
    S = Sout; cin = b.cout;
  }
  return n;
}

}  // namespace

struct yl_stage {
  Arena mem;                             // yl_block.h
  yl_stage_cfg cfg;
  int fB, fS, fTrain;                    // the forward whose activations are held (mem.fValid)
};

extern "C" {

yl_status yl_stage_plan(const yl_stage_cfg* cfg, int32_t batch, int32_t size, yl_stage_plan_info* out) {
  if (!cfg_ok(cfg) || !out || batch < 1 || size < 1) return YL_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  out->stat_rows = STAT_ROWS; out->gemm_rows = GEMM_ROWS;
  Unit us[4 * YL_STAGE_MAX_BLOCKS];
  const int64_t M0 = (int64_t)batch * size * size;
  if (M0 > (int64_t)65535 * GEMM_ROWS) return YL_ERR_UNSUPPORTED;      // the GEMM's grid.y; no unit has more rows than x
  const int n = make_units(*cfg, batch, size, us, out->block);
  int64_t amax = 0, cmax = 0, smax = 0, wmax = 0;
  for (int i = 0; i < n; ++i) {
    const Unit& u = us[i];
    if (u.Mout * u.cout >= ((int64_t)1 << 40) || u.cin > (1 << 20) || u.cout > (1 << 20)) return YL_ERR_UNSUPPORTED;
    const int64_t a = u.Mout * u.cout * 4;
    amax = a > amax ? a : amax;
    cmax = u.cout > cmax ? u.cout : cmax;
    const int64_t sp = round16((int64_t)u.tiles * (u.dw ? u.k * u.k : 2) * u.cout * 8);
    smax = sp > smax ? sp : smax;
    if (!u.dw) {
      const int64_t wp = round16((int64_t)u.wsplits * u.cin * u.cout * 4);
      wmax = wp > wmax ? wp : wmax;
    }
  }
  const int64_t x0 = M0 * cfg->in_channels * 4;
  if (x0 >= ((int64_t)1 << 42)) return YL_ERR_UNSUPPORTED;
  out->saved_bytes = x0;
  for (int i = 0; i < cfg->num_blocks; ++i) out->saved_bytes += out->block[i].saved_bytes;
  out->nosave_bytes = 4 * amax + 2 * cmax * 4;
  out->workspace_bytes = 3 * (amax > x0 ? amax : x0) + smax + 2 * cmax * 4 + wmax;
  return YL_OK;
}

yl_status yl_stage_create(int32_t device, const yl_stage_cfg* cfg, yl_stage** out) {
  if (!out || !cfg_ok(cfg)) return YL_ERR_INVALID;
  if (hipSetDevice(device) != hipSuccess) return YL_ERR_HIP;
  yl_stage* h = new (std::nothrow) yl_stage();
  if (!h) return YL_ERR_NOMEM;
  h->mem.device = device; h->cfg = *cfg;
  *out = h;
  return YL_OK;
}

void yl_stage_destroy(yl_stage* h) {
  if (!h) return;
  arena_release(h->mem);
  delete h;
}

yl_status yl_stage_held(const yl_stage* h, int64_t* saved_bytes, int64_t* workspace_bytes, int32_t* forward_held) {
  return arena_held(h ? &h->mem : nullptr, saved_bytes, workspace_bytes, forward_held);
}

}  // extern "C"

namespace {

struct StageBuffers {
  Unit us[4 * YL_STAGE_MAX_BLOCKS];
  int n;
  float* x;                              // save: the copy of the caller's x
  float *z[4 * YL_STAGE_MAX_BLOCKS], *h[4 * YL_STAGE_MAX_BLOCKS], *stats[4 * YL_STAGE_MAX_BLOCKS];   // save: per unit
  float *nz, *nh[3], *nstats;            // no save: one z, three rotating h, one (mean, invstd)
  float *g[3], *coef, *wpart;
  double* spart;
};

// the handle's memory for (B, S), cut as yl_stage_plan counts it
yl_status ensure(yl_stage* h, int B, int S, bool save, StageBuffers* sb) {
  yl_stage_plan_info pl;
  yl_status st = yl_stage_plan(&h->cfg, B, S, &pl);
  if (st != YL_OK) return st;
  st = arena_reserve(h->mem, save ? pl.saved_bytes : pl.nosave_bytes, pl.workspace_bytes);
  if (st != YL_OK) return st;
  sb->n = make_units(h->cfg, B, S, sb->us, nullptr);
  size_t amax = 0, cmax = 0, smax = 0;
  for (int i = 0; i < sb->n; ++i) {
    const Unit& u = sb->us[i];
    const size_t a = (size_t)u.Mout * u.cout * 4, sp = (size_t)round16((int64_t)u.tiles * (u.dw ? u.k * u.k : 2) * u.cout * 8);
    amax = a > amax ? a : amax;
    cmax = (size_t)u.cout > cmax ? (size_t)u.cout : cmax;
    smax = sp > smax ? sp : smax;
  }
  const size_t x0 = (size_t)B * S * S * h->cfg.in_channels * 4;
  const size_t gmax = amax > x0 ? amax : x0;
  char* w = h->mem.work;
  for (int i = 0; i < 3; ++i) { sb->g[i] = (float*)w; w += gmax; }
  sb->spart = (double*)w; w += smax;
  sb->coef = (float*)w; w += 2 * cmax * 4;
  sb->wpart = (float*)w;
  char* p = h->mem.saved;
  if (save) {
    sb->x = (float*)p; p += x0;
    for (int i = 0; i < sb->n; ++i) {
      const Unit& u = sb->us[i];
      const size_t a = (size_t)u.Mout * u.cout * 4;
      sb->z[i] = (float*)p; p += a;
      sb->h[i] = (float*)p; p += a;
      sb->stats[i] = (float*)p; p += 2 * (size_t)u.cout * 4;
    }
  } else {
    sb->nz = (float*)p; p += amax;
    for (int i = 0; i < 3; ++i) { sb->nh[i] = (float*)p; p += amax; }
    sb->nstats = (float*)p;
  }
  return YL_OK;
}

bool params_ok(const yl_stage* h, const yl_stage_tensors* t) {
  if (!t) return false;
  Unit us[4 * YL_STAGE_MAX_BLOCKS];
  const int n = make_units(h->cfg, 1, 1, us, nullptr);     // which units exist does not depend on the shape
  uintptr_t any = 0;
  for (int i = 0; i < n; ++i) {
    const yl_stage_unit& e = entry(t, us[i]);
    if (!e.w || !e.gamma || !e.beta || !e.running_mean || !e.running_var || !e.num_batches_tracked) return false;
    any |= (uintptr_t)e.w | (uintptr_t)e.gamma | (uintptr_t)e.beta | (uintptr_t)e.running_mean | (uintptr_t)e.running_var;
    if ((uintptr_t)e.num_batches_tracked & 7u) return false;
  }
  return !(any & 3u);
}

inline int pick(int a, int b) {          // a gradient buffer that is neither a nor b
  for (int i = 0; i < 3; ++i)
    if (i != a && i != b) return i;
  return 0;
}

}  // namespace

extern "C" {

yl_status yl_stage_forward(yl_stage* h, const yl_stage_tensors* params, const float* x_dev, int32_t batch, int32_t size,
                           uint32_t flags, float* out_dev, void* stream, int32_t* launches) {
  if (!h || !x_dev || !out_dev || batch < 1 || size < 1 || !params_ok(h, params)) return YL_ERR_INVALID;
  if (flags & ~(uint32_t)(YL_HEAD_TRAIN | YL_HEAD_SAVE)) return YL_ERR_INVALID;       // fp32 only: no precision bits
  if (((uintptr_t)x_dev & 15u) || ((uintptr_t)out_dev & 15u)) return YL_ERR_UNSUPPORTED;
  const bool train = flags & YL_HEAD_TRAIN, save = flags & YL_HEAD_SAVE;
  {
    Unit us[4 * YL_STAGE_MAX_BLOCKS];
    const int n = make_units(h->cfg, batch, size, us, nullptr);
    for (int i = 0; i < n; ++i)
      if (us[i].Mout < 1 || (train && us[i].Mout < 2)) return YL_ERR_INVALID;          // no variance of one value
  }
  StageBuffers sb;
  const yl_status st = ensure(h, batch, size, save, &sb);
  if (st != YL_OK) return st;
  hipStream_t s = (hipStream_t)stream;
  h->mem.fValid = 0;
  const size_t x0 = (size_t)batch * size * size * h->cfg.in_channels * 4;
  if (save && hipMemcpyAsync(sb.x, x_dev, x0, hipMemcpyDeviceToDevice, s) != hipSuccess) return YL_ERR_HIP;
  int nl = 0;
  const float* in = save ? sb.x : x_dev;
  const float* bin = in;                 // the input of the block the walk is in
  int in_i = -1, bin_i = -1;             // no save: which rotating buffer holds them (-1: none of the three)
  for (int i = 0; i < sb.n; ++i) {
    const Unit& u = sb.us[i];
    const yl_stage_unit& e = entry(params, u);
    if (u.first) { bin = in; bin_i = in_i; }
    float* z = save ? sb.z[i] : sb.nz;
    float* stats = save ? sb.stats[i] : sb.nstats;
    int out_i = -1;
    float* hout;
    if (save) hout = sb.h[i];
    else if (i == sb.n - 1) hout = out_dev;
    else { out_i = pick(in_i, bin_i); hout = sb.nh[out_i]; }
    const int M = (int)u.Mout, F = u.cout;
    if (u.dw) launch_dw<false>(s, in, e.w, z, u.k, u.st, batch, u.Sin, u.Sout, F);
    else launch_gemm<0>(s, RowsScalar{e.w, u.cin}, RowsVec{in, u.cin}, OutRowsVec{z, F}, F, M, u.cin, u.cin, 1);
    ++nl;
    if (train) {
      StatP sp;
      sp.a = z; sp.h = nullptr; sp.z = nullptr; sp.stats = nullptr; sp.part = sb.spart;
      sp.M = M; sp.F = F; sp.CQ = pick_cq(F); sp.bwd = 0;
      hipLaunchKernelGGL(yl_stage_colstats_kernel<false>, dim3(u.tiles, ceil_div(F >> 2, sp.CQ)), dim3(NT), 0, s, sp);
      ++nl;
    }
    BnFwdP bp;
    bp.part = sb.spart; bp.tiles = u.tiles; bp.M = M; bp.F = F; bp.train = train ? 1 : 0;
    bp.rm = e.running_mean; bp.rv = e.running_var; bp.nbt = e.num_batches_tracked; bp.stats = stats;
    hipLaunchKernelGGL(yl_stage_bn_stats_kernel, dim3(ceil_div(F, NT)), dim3(NT), 0, s, bp, h->cfg.eps);
    const long n4 = (long)M * (F >> 2);
    const float* res = (u.last && u.res) ? bin : nullptr;
    if (u.relu)
      hipLaunchKernelGGL(yl_stage_bn_kernel<true>, dim3(ceil_div(n4, NT)), dim3(NT), 0, s, (const float*)z, (const float*)stats,
                         (const float*)e.gamma, (const float*)e.beta, res, hout, n4, F);
    else
      hipLaunchKernelGGL(yl_stage_bn_kernel<false>, dim3(ceil_div(n4, NT)), dim3(NT), 0, s, (const float*)z, (const float*)stats,
                         (const float*)e.gamma, (const float*)e.beta, res, hout, n4, F);
    nl += 2;
    in = hout; in_i = out_i;
  }
  if (save) {
    const Unit& u = sb.us[sb.n - 1];
    if (hipMemcpyAsync(out_dev, in, (size_t)u.Mout * u.cout * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return YL_ERR_HIP;
  }
  if (launches) *launches = nl;
  if (hipGetLastError() != hipSuccess) return YL_ERR_HIP;
  if (save) { h->fB = batch; h->fS = size; h->fTrain = train ? 1 : 0; h->mem.fValid = 1; }
  return YL_OK;
}

yl_status yl_stage_backward(yl_stage* h, const yl_stage_tensors* params, const yl_stage_tensors* grads,
                            const float* gy_dev, float* dx_dev, void* stream, int32_t* launches) {
  if (!h || !grads || !gy_dev || !params_ok(h, params)) return YL_ERR_INVALID;
  if (((uintptr_t)gy_dev & 15u) || ((uintptr_t)dx_dev & 15u)) return YL_ERR_UNSUPPORTED;
  if (!h->mem.fValid) return YL_ERR_STATE;
  StageBuffers sb;
  const yl_status st = ensure(h, h->fB, h->fS, true, &sb);
  if (st != YL_OK) return st;
  if (!h->mem.fValid) return YL_ERR_STATE;
  uintptr_t gany = 0;
  int first = dx_dev ? 0 : sb.n;         // the first unit something is wanted of
  for (int i = sb.n - 1; i >= 0; --i) {
    const yl_stage_unit& g = entry(grads, sb.us[i]);
    const uintptr_t any = (uintptr_t)g.w | (uintptr_t)g.gamma | (uintptr_t)g.beta;
    gany |= any;
    if (any && i < first) first = i;
  }
  if (gany & 3u) return YL_ERR_UNSUPPORTED;                // before the first launch: nothing of the caller's is written
  hipStream_t s = (hipStream_t)stream;
  const bool train = h->fTrain != 0;
  const int B = h->fB;
  int nl = 0;
  const float* dh = gy_dev;
  int cur = -1;                          // the buffer dh is in (-1: the caller's gy)
  const float* G = nullptr;              // the output gradient of the residual block the walk is in
  int keep = -1;                         // the buffer G is in (-1: none of the three)
  for (int i = sb.n - 1; i >= first; --i) {
    const Unit& u = sb.us[i];
    const yl_stage_unit& e = entry(params, u);
    const yl_stage_unit& g = entry(grads, u);
    const float* xin = i ? sb.h[i - 1] : sb.x;
    const int M = (int)u.Mout, F = u.cout, cq = pick_cq(F);
    const long n4 = (long)M * (F >> 2);
    if (u.last && u.res) { G = dh; keep = cur; }
    const bool sums = train || g.gamma || g.beta;          // sum g, sum g * xhat: dbeta, dgamma and the batch statistics' two means
    if (sums) {
      StatP sp;
      sp.a = dh; sp.h = sb.h[i]; sp.z = sb.z[i]; sp.stats = sb.stats[i]; sp.part = sb.spart;
      sp.M = M; sp.F = F; sp.CQ = cq; sp.bwd = 1;
      const dim3 grid(u.tiles, ceil_div(F >> 2, cq));
      if (u.relu) hipLaunchKernelGGL(yl_stage_colstats_kernel<true>, grid, dim3(NT), 0, s, sp);
      else hipLaunchKernelGGL(yl_stage_colstats_kernel<false>, grid, dim3(NT), 0, s, sp);
      ++nl;
    }
    BnBwdP bp;
    bp.part = sb.spart; bp.tiles = sums ? u.tiles : 0; bp.M = M; bp.F = F; bp.train = train;
    bp.dgamma = g.gamma; bp.dbeta = g.beta; bp.coef = sb.coef;
    hipLaunchKernelGGL(yl_head_bn_grads_kernel, dim3(ceil_div(F, NT)), dim3(NT), 0, s, bp);
    ++nl;
    const bool need_dx = i > first || (i == 0 && dx_dev);
    if (!need_dx && !g.w) break;
    const int t = (cur >= 0 && cur != keep) ? cur : pick(keep, -1);      // dz: in place unless dh must survive
    float* dz = sb.g[t];
    if (u.relu)
      hipLaunchKernelGGL(yl_stage_bn_bwd_kernel<true>, dim3(ceil_div(n4, NT)), dim3(NT), 0, s, dh, (const float*)sb.h[i],
                         (const float*)sb.z[i], (const float*)sb.stats[i], (const float*)sb.coef, (const float*)e.gamma, dz, n4, F);
    else
      hipLaunchKernelGGL(yl_stage_bn_bwd_kernel<false>, dim3(ceil_div(n4, NT)), dim3(NT), 0, s, dh, (const float*)nullptr,
                         (const float*)sb.z[i], (const float*)sb.stats[i], (const float*)sb.coef, (const float*)e.gamma, dz, n4, F);
    ++nl;
    if (g.w) {
      if (u.dw) {
        launch_dw_wgrad(s, dz, xin, sb.spart, g.w, u.k, u.st, B, u.Sin, u.Sout, F, u.tiles);
      } else {                           // dW = dz^T . x
        launch_gemm<0>(s, ColsScalar{xin, u.cin}, ColsScalar{dz, F}, OutPartial{sb.wpart, (long)u.cin * F}, u.cin, F, M, u.wrows,
                       u.wsplits);
        HeadRows none;
        memset(&none, 0, sizeof(none));
        hipLaunchKernelGGL(yl_head_wsum_kernel, dim3(ceil_div((long)u.cin * F, NT)), dim3(NT), 0, s, (const float*)sb.wpart,
                           u.wsplits, u.cin, F, g.w, none, 0);
      }
      nl += 2;
    }
    if (!need_dx) break;
    const int d = pick(keep, t);
    float* dst = i ? sb.g[d] : dx_dev;
    if (u.dw) launch_dw<true>(s, dz, e.w, dst, u.k, u.st, B, u.Sin, u.Sout, F);
    else launch_gemm<0>(s, ColsScalar{e.w, u.cin}, RowsVec{dz, F}, OutRowsVec{dst, u.cin}, u.cin, M, F, F, 1);   // dx = dz . W
    ++nl;
    if (u.first && u.res) {              // the block's input also went straight to its output
      const long m4 = (long)u.Min * (u.cin >> 2);
      hipLaunchKernelGGL(yl_stage_add_kernel, dim3(ceil_div(m4, NT)), dim3(NT), 0, s, dst, G, m4);
      ++nl;
      G = nullptr; keep = -1;
    }
    dh = dst; cur = d;
  }
  if (launches) *launches = nl;
  return hipGetLastError() == hipSuccess ? YL_OK : YL_ERR_HIP;
}

yl_status yl_stage_depthwise(const float* a_dev, const float* b_dev, float* out_dev, int32_t pass, int32_t k,
                             int32_t stride, int32_t batch, int32_t size, int32_t channels, void* stream,
                             int32_t* launches) {
  if (!a_dev || !b_dev || !out_dev || batch < 1 || size < 1 || channels < 4 || (channels & 3)) return YL_ERR_INVALID;
  if ((k != 3 && k != 5) || (stride != 1 && stride != 2)) return YL_ERR_INVALID;
  if (pass != YL_STAGE_PASS_FORWARD && pass != YL_STAGE_PASS_DGRAD && pass != YL_STAGE_PASS_WGRAD) return YL_ERR_INVALID;
  const bool wg = pass == YL_STAGE_PASS_WGRAD;
  if (((uintptr_t)a_dev & 15u) || ((uintptr_t)(wg ? (const void*)b_dev : (const void*)out_dev) & 15u)) return YL_ERR_UNSUPPORTED;
  if (((uintptr_t)b_dev & 3u) || ((uintptr_t)out_dev & 3u)) return YL_ERR_UNSUPPORTED;
  const int So = out_size(size, k, stride);
  const int64_t M = (int64_t)batch * size * size, Mo = (int64_t)batch * So * So;
  if (M * channels >= ((int64_t)1 << 40) || M >= ((int64_t)1 << 31)) return YL_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (!wg) {
    if (pass == YL_STAGE_PASS_FORWARD) launch_dw<false>(s, a_dev, b_dev, out_dev, k, stride, batch, size, So, channels);
    else launch_dw<true>(s, a_dev, b_dev, out_dev, k, stride, batch, size, So, channels);
    if (launches) *launches = 1;
    return hipGetLastError() == hipSuccess ? YL_OK : YL_ERR_HIP;
  }
  const int tiles = ceil_div(Mo, STAT_ROWS);
  double* part = nullptr;
  if (hipMalloc((void**)&part, (size_t)round16((int64_t)tiles * k * k * channels * 8)) != hipSuccess) {
    (void)hipGetLastError();
    return YL_ERR_NOMEM;
  }
  launch_dw_wgrad(s, b_dev, a_dev, part, out_dev, k, stride, batch, size, So, channels, tiles);
  const bool ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  hipFree(part);
  if (launches) *launches = 2;
  return ok ? YL_OK : YL_ERR_HIP;
}

}  // extern "C"
