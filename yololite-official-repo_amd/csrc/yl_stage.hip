// Trainable backbone stage: a stack of MobileNetV4 UIB blocks (timm UniversalInvertedResidual) and 1x1 ConvBnAct blocks,
// forward and backward on NHWC fp32 rows (include/yololite_hip.h, yl_stage_*).  A uir block with a = 0 is, unit for unit,
// timm's InvertedResidual without squeeze-excite (conv_pw, conv_dw, conv_pwl): with the handle's variant
// (yl_variant_stage_set: ReLU6 for ReLU, TF-SAME padding) the same walk trains the EfficientNet-Lite stages.
//
// The stack is flattened into UNITS, each a bias-free convolution and its BatchNorm:
//   unit u:  z = conv(x_u)   h = bn(z) [relu] [+ the block's input, behind the last unit of a residual block]
// x_u is the previous unit's h (the caller's x for unit 0).  A depthwise unit is k x k with stride 1 or 2; a 1x1 unit is
// the heads' GEMM (yl_block.h: launch_gemm_in with its accessors) in all three passes, in the handle's operand type
// (yl_amp_stage_set: fp32, or fp16 / bf16 operands rounded to nearest even inside the GEMM, fp32 accumulation).  The
// depthwise units, BatchNorm, ReLU and the residual are fp32 in every mode.
// The walk over the units, forward and backward, with the handle, its memory and the table checks, is yl_units.h, shared
// with yl_stem.hip; here are what is this stack's own: its configuration and units (cfg_ok, make_units, the per-block
// plan), the policy that tells the walk what a unit's convolution launches (three rotating buffers; units without ReLU and
// residual blocks occur), and the kernels neither yl_block.h nor yl_bn.h has: depthwise k x k with stride in three passes,
// and the residual's add.
#include "yl_units.h"

namespace {

// ---- depthwise K x K, stride ST, weight [C][1][K][K].  x: [B][Sx][Sx][C], y: [B][So][So][C].  `pb` pixels of zeros stand
// in front of the first row and column (yl_units.h pad_begin: (K - 1) / 2, or TF-SAME's leading pad); behind the last ones as
// many as the taps reach.
// GRAD = false: y = conv(x); a thread owns one OUTPUT pixel x 4 channels.  GRAD = true: `src` is dy, `dst` is dx; a thread
// owns one INPUT pixel (i, j) x 4 channels and sums, ky then kx ascending, the taps whose (i + pb - ky) is a multiple of ST
// (output row (i + pb - ky) / ST): the transposed convolution as a gather.  fp32 sum from zero in tap order either way.
template <int K, int ST, bool GRAD>
__global__ __launch_bounds__(NT) void yl_stage_dw_kernel(const float* __restrict__ src, const float* __restrict__ w,
                                                        float* __restrict__ dst, int B, int Sx, int So, int C, int pb) {
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
      yy = i * ST + ky - pb;
    } else {
      const int t = i + pb - ky;
      if (t < 0 || (ST == 2 && (t & 1))) continue;
      yy = t / ST;
    }
    if (yy < 0 || yy >= R) continue;
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      int xx;
      if (!GRAD) {
        xx = j * ST + kx - pb;
      } else {
        const int t = j + pb - kx;
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
                                                              double* __restrict__ part, int Mo, int Sx, int So, int C, int CQ,
                                                              int pb) {
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
        const int b = m / SS, ij = m - b * SS, i = ij / So, j = ij - i * So, yy = i * ST + ky - pb;
        if (yy < 0 || yy >= Sx) continue;
        const f32x4 g = ld4(dy + (long)m * C + c);
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const int xx = j * ST + kx - pb;
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

// ---- BatchNorm: the column sums, the statistics, the normalisation and its backward are yl_bn.h, which every training unit runs
// the residual's backward: io += g
__global__ __launch_bounds__(NT) void yl_stage_add_kernel(float* io, const float* __restrict__ g, long n4) {
  const long idx = (long)blockIdx.x * NT + threadIdx.x;
  if (idx >= n4) return;
  st4(io + idx * 4, ld4(io + idx * 4) + ld4(g + idx * 4));
}

// ---- launches of one depthwise pass with the leading pad pb.  false: (k, stride) is not one of {3, 5} x {1, 2}
template <bool GRAD>
bool launch_dw(hipStream_t s, const float* src, const float* w, float* dst, int k, int st, int pb, int B, int Sx, int So, int C) {
  const long n = (long)B * (GRAD ? Sx : So) * (GRAD ? Sx : So) * (C >> 2);
  const dim3 grid(ceil_div(n, NT)), blk(NT);
  if (k == 3 && st == 1) hipLaunchKernelGGL((yl_stage_dw_kernel<3, 1, GRAD>), grid, blk, 0, s, src, w, dst, B, Sx, So, C, pb);
  else if (k == 3 && st == 2) hipLaunchKernelGGL((yl_stage_dw_kernel<3, 2, GRAD>), grid, blk, 0, s, src, w, dst, B, Sx, So, C, pb);
  else if (k == 5 && st == 1) hipLaunchKernelGGL((yl_stage_dw_kernel<5, 1, GRAD>), grid, blk, 0, s, src, w, dst, B, Sx, So, C, pb);
  else if (k == 5 && st == 2) hipLaunchKernelGGL((yl_stage_dw_kernel<5, 2, GRAD>), grid, blk, 0, s, src, w, dst, B, Sx, So, C, pb);
  else return false;
  return true;
}
// partials over `tiles` tiles of the B * So * So output rows, then their ordered sum into dw [C][1][k][k]: 2 launches
bool launch_dw_wgrad(hipStream_t s, const float* dy, const float* x, double* part, float* dw, int k, int st, int pb, int B, int Sx,
                     int So, int C, int tiles) {
  const int Mo = B * So * So, cq = pick_cq(C);
  const dim3 grid(tiles, ceil_div(C >> 2, cq)), blk(NT);
  if (k == 3 && st == 1) hipLaunchKernelGGL((yl_stage_dw_wgrad_kernel<3, 1>), grid, blk, 0, s, dy, x, part, Mo, Sx, So, C, cq, pb);
  else if (k == 3 && st == 2) hipLaunchKernelGGL((yl_stage_dw_wgrad_kernel<3, 2>), grid, blk, 0, s, dy, x, part, Mo, Sx, So, C, cq, pb);
  else if (k == 5 && st == 1) hipLaunchKernelGGL((yl_stage_dw_wgrad_kernel<5, 1>), grid, blk, 0, s, dy, x, part, Mo, Sx, So, C, cq, pb);
  else if (k == 5 && st == 2) hipLaunchKernelGGL((yl_stage_dw_wgrad_kernel<5, 2>), grid, blk, 0, s, dy, x, part, Mo, Sx, So, C, cq, pb);
  else return false;
  hipLaunchKernelGGL(yl_stage_dw_wsum_kernel, dim3(ceil_div((long)k * k * C, NT)), blk, 0, s, (const double*)part, tiles, C,
                     k * k, dw);
  return true;
}

// ---- the stack as units (yl_units.h: Unit)
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

// the handle's variant: what an activated unit runs behind its BatchNorm, and whether the depthwise units pad as TF-SAME.
// TF-SAME's output size is ceil(S / s), which for odd k is out_size's: sizes, arenas and tile counts do not depend on it
struct Variant { int act, same; };
constexpr Variant PLAIN = {ACT_RELU, 0};

// the units of cfg at (B, S) under the variant v -> their number; fills the per-block plan if `bp` is given.  cfg_ok(cfg) holds
int make_units(const yl_stage_cfg& cfg, Variant v, int B, int S, Unit* us, yl_stage_block_plan* bp) {
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
      u.block = i; u.slot = slot; u.dw = dw; u.planar = 0; u.act = relu ? v.act : ACT_NONE; u.k = k; u.st = st;
      u.pb = pad_begin(k, st, Si, v.same);
      u.cin = ci; u.cout = co; u.Sin = Si; u.Sout = So;
      u.Min = (int64_t)B * Si * Si; u.Mout = (int64_t)B * So * So;
      u.stat_rows = STAT_ROWS; u.tiles = ceil_div(u.Mout, STAT_ROWS);
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
        p.saved_bytes += unit_saved_bytes(us[u]);
        if (us[u].slot == 1) { p.exp_rows = us[u].wrows; p.exp_splits = us[u].wsplits; }
        if (us[u].slot == 3) { p.proj_rows = us[u].wrows; p.proj_splits = us[u].wsplits; }
      }
    }
    S = Sout; cin = b.cout;
  }
  return n;
}

// units, per-block plan (if `bp` is given) and sizes of cfg at (B, S): what yl_stage_plan reports and the walk runs on
yl_status layout(const yl_stage_cfg& cfg, Variant v, int B, int S, Unit* us, int* n, Sizes* z, yl_stage_block_plan* bp) {
  const int64_t M0 = (int64_t)B * S * S;
  const bool rows_ok = M0 <= (int64_t)65535 * GEMM_ROWS;   // the GEMM's grid.y; no unit has more rows than x
  *n = make_units(cfg, v, B, S, us, rows_ok ? bp : nullptr);
  if (!rows_ok) return YL_ERR_UNSUPPORTED;
  if (!unit_sizes(us, *n, 1 << 20, z)) return YL_ERR_UNSUPPORTED;
  z->x0 = z->xsave = M0 * cfg.in_channels * 4;
  if (z->x0 >= ((int64_t)1 << 42)) return YL_ERR_UNSUPPORTED;
  z->gmax = z->amax > z->x0 ? z->amax : z->x0;
  return YL_OK;
}

// the entries of a table in unit order -> their number (which units exist does not depend on the shape)
int resolve(const yl_stage_cfg& cfg, const yl_stage_tensors* t, const yl_stage_unit** tab) {
  Unit us[MAX_UNITS];
  const int n = make_units(cfg, PLAIN, 1, 1, us, nullptr);
  for (int i = 0; i < n; ++i) {
    const yl_stage_block& b = t->block[us[i].block];
    const int slot = us[i].slot;
    tab[i] = slot == 0 ? &b.dw_start : (slot == 1 ? &b.pw_exp : (slot == 2 ? &b.dw_mid : &b.pw_proj));
  }
  return n;
}

// what yl_units.h's walk launches for this stack: depthwise k x k, or the heads' GEMM for a 1x1 unit
struct StagePolicy {
  static constexpr int ROT = 3;
  static constexpr bool MIXED = true;
  static constexpr bool RELU6 = true;
  template <class H> static yl_status layout(const H& h, int B, int S, Unit* us, int* n, Sizes* z) {
    return ::layout(h.cfg, Variant{h.act, h.same}, B, S, us, n, z, nullptr);
  }
  static int conv_forward(hipStream_t s, const Unit& u, int B, const float* x, const float* w, float* z, const UnitBuffers&, int mode) {
    if (u.dw) launch_dw<false>(s, x, w, z, u.k, u.st, u.pb, B, u.Sin, u.Sout, u.cout);
    else launch_gemm_in<true>(mode, s, RowsScalar{w, u.cin}, RowsVec{x, u.cin}, OutRowsVec{z, u.cout}, u.cout, (int)u.Mout, u.cin, u.cin, 1);
    return 1;
  }
  static int conv_wgrad(hipStream_t s, const Unit& u, int B, const float* x, const float* dz, float* dw, const UnitBuffers& sb, int mode) {
    const int F = u.cout;
    if (u.dw) {
      launch_dw_wgrad(s, dz, x, sb.spart, dw, u.k, u.st, u.pb, B, u.Sin, u.Sout, F, u.tiles);
    } else {                             // dW = dz^T . x
      launch_gemm_in<true>(mode, s, ColsScalar{x, u.cin}, ColsScalar{dz, F}, OutPartial{sb.wpart, (long)u.cin * F}, u.cin, F,
                           (int)u.Mout, u.wrows, u.wsplits);
      HeadRows none;
      memset(&none, 0, sizeof(none));
      hipLaunchKernelGGL(yl_head_wsum_kernel, dim3(ceil_div((long)u.cin * F, NT)), dim3(NT), 0, s, (const float*)sb.wpart,
                         u.wsplits, u.cin, F, dw, none, 0);
    }
    return 2;
  }
  static int conv_dgrad(hipStream_t s, const Unit& u, int B, const float* dz, const float* w, float* dx, const UnitBuffers&, int mode) {
    const int F = u.cout;
    if (u.dw) launch_dw<true>(s, dz, w, dx, u.k, u.st, u.pb, B, u.Sin, u.Sout, F);
    else launch_gemm_in<true>(mode, s, ColsScalar{w, u.cin}, RowsVec{dz, F}, OutRowsVec{dx, u.cin}, u.cin, (int)u.Mout, F, F, 1);   // dx = dz . W
    return 1;
  }
  static void add(hipStream_t s, float* io, const float* g, long n4) {
    hipLaunchKernelGGL(yl_stage_add_kernel, dim3(ceil_div(n4, NT)), dim3(NT), 0, s, io, g, n4);
  }
};

}  // namespace

struct yl_stage : UnitStack<yl_stage_cfg> {};

extern "C" {

yl_status yl_stage_plan(const yl_stage_cfg* cfg, int32_t batch, int32_t size, yl_stage_plan_info* out) {
  if (!cfg_ok(cfg) || !out || batch < 1 || size < 1) return YL_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  out->stat_rows = STAT_ROWS; out->gemm_rows = GEMM_ROWS;
  Unit us[MAX_UNITS];
  Sizes z;
  int n;
  const yl_status st = layout(*cfg, PLAIN, batch, size, us, &n, &z, out->block);
  if (st != YL_OK) return st;
  const ArenaBytes b = arena_bytes(us, n, z, StagePolicy::ROT);
  out->saved_bytes = b.saved; out->nosave_bytes = b.nosave; out->workspace_bytes = b.work;
  return YL_OK;
}

yl_status yl_stage_create(int32_t device, const yl_stage_cfg* cfg, yl_stage** out) {
  return units_create(device, cfg, cfg_ok(cfg), out);
}

void yl_stage_destroy(yl_stage* h) { units_destroy(h); }

yl_status yl_stage_held(const yl_stage* h, int64_t* saved_bytes, int64_t* workspace_bytes, int32_t* forward_held) {
  return units_held(h, saved_bytes, workspace_bytes, forward_held);
}

yl_status yl_amp_stage_set(yl_stage* h, uint32_t mode) { return units_amp_set(h, mode); }

yl_status yl_amp_stage_get(const yl_stage* h, uint32_t* mode, uint32_t* held_mode) { return units_amp_get(h, mode, held_mode); }

yl_status yl_stage_forward(yl_stage* h, const yl_stage_tensors* params, const float* x_dev, int32_t batch, int32_t size,
                           uint32_t flags, float* out_dev, void* stream, int32_t* launches) {
  if (!h || !x_dev || !out_dev || batch < 1 || size < 1 || !params) return YL_ERR_INVALID;
  const yl_stage_unit* par[MAX_UNITS];
  const int n = resolve(h->cfg, params, par);
  return units_forward<StagePolicy>(h, par, n, x_dev, 15u, batch, size, flags, out_dev, stream, launches);
}

yl_status yl_stage_backward(yl_stage* h, const yl_stage_tensors* params, const yl_stage_tensors* grads,
                            const float* gy_dev, float* dx_dev, void* stream, int32_t* launches) {
  if (!h || !grads || !gy_dev || !params) return YL_ERR_INVALID;
  const yl_stage_unit *par[MAX_UNITS], *grd[MAX_UNITS];
  const int n = resolve(h->cfg, params, par);
  resolve(h->cfg, grads, grd);
  return units_backward<StagePolicy>(h, par, grd, n, gy_dev, dx_dev, stream, launches);
}

yl_status yl_variant_stage_set(yl_stage* h, int32_t act, int32_t same) {
  if (!h || (act != YL_STAGE_ACT_RELU && act != YL_STAGE_ACT_RELU6) || (same != 0 && same != 1)) return YL_ERR_INVALID;
  if (h->mem.fValid) return YL_ERR_STATE;                  // the held forward's backward runs in the variant of its forward
  h->act = act == YL_STAGE_ACT_RELU6 ? ACT_RELU6 : ACT_RELU;
  h->same = same;
  return YL_OK;
}

yl_status yl_variant_stage_get(const yl_stage* h, int32_t* act, int32_t* same) {
  if (!h) return YL_ERR_INVALID;
  if (act) *act = h->act == ACT_RELU6 ? YL_STAGE_ACT_RELU6 : YL_STAGE_ACT_RELU;
  if (same) *same = h->same;
  return YL_OK;
}

yl_status yl_stage_depthwise(const float* a_dev, const float* b_dev, float* out_dev, int32_t pass, int32_t k,
                             int32_t stride, int32_t batch, int32_t size, int32_t channels, void* stream,
                             int32_t* launches) {
  return yl_variant_stage_depthwise(a_dev, b_dev, out_dev, pass, k, stride, batch, size, channels, 0, stream, launches);
}

yl_status yl_variant_stage_depthwise(const float* a_dev, const float* b_dev, float* out_dev, int32_t pass, int32_t k,
                                     int32_t stride, int32_t batch, int32_t size, int32_t channels, int32_t same, void* stream,
                                     int32_t* launches) {
  if (same != 0 && same != 1) return YL_ERR_INVALID;
  if (!a_dev || !b_dev || !out_dev || batch < 1 || size < 1 || channels < 4 || (channels & 3)) return YL_ERR_INVALID;
  if ((k != 3 && k != 5) || (stride != 1 && stride != 2)) return YL_ERR_INVALID;
  if (pass != YL_STAGE_PASS_FORWARD && pass != YL_STAGE_PASS_DGRAD && pass != YL_STAGE_PASS_WGRAD) return YL_ERR_INVALID;
  const bool wg = pass == YL_STAGE_PASS_WGRAD;
  if (((uintptr_t)a_dev & 15u) || ((uintptr_t)(wg ? (const void*)b_dev : (const void*)out_dev) & 15u)) return YL_ERR_UNSUPPORTED;
  if (((uintptr_t)b_dev & 3u) || ((uintptr_t)out_dev & 3u)) return YL_ERR_UNSUPPORTED;
  const int So = out_size(size, k, stride), pb = pad_begin(k, stride, size, same);
  const int64_t M = (int64_t)batch * size * size, Mo = (int64_t)batch * So * So;
  if (M * channels >= ((int64_t)1 << 40) || M >= ((int64_t)1 << 31)) return YL_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (!wg) {
    if (pass == YL_STAGE_PASS_FORWARD) launch_dw<false>(s, a_dev, b_dev, out_dev, k, stride, pb, batch, size, So, channels);
    else launch_dw<true>(s, a_dev, b_dev, out_dev, k, stride, pb, batch, size, So, channels);
    if (launches) *launches = 1;
    return hipGetLastError() == hipSuccess ? YL_OK : YL_ERR_HIP;
  }
  const int tiles = ceil_div(Mo, STAT_ROWS);
  double* part = nullptr;
  if (hipMalloc((void**)&part, (size_t)round16((int64_t)tiles * k * k * channels * 8)) != hipSuccess) {
    (void)hipGetLastError();
    return YL_ERR_NOMEM;
  }
  launch_dw_wgrad(s, b_dev, a_dev, part, out_dev, k, stride, pb, batch, size, So, channels, tiles);
  const bool ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  hipFree(part);
  if (launches) *launches = 2;
  return ok ? YL_OK : YL_ERR_HIP;
}

}  // extern "C"
