// A stack of conv + BatchNorm UNITS on NHWC fp32 rows, forward and backward: the host code that the trainable backbone
// stage (yl_stage.hip) and the trainable dense stem (yl_stem.hip) share.  Like yl_block.h, everything lives in an
// anonymous namespace: each translation unit compiles the kernels IT launches into its own code object.
//
//   unit u:  z = conv(x_u)   h = bn(z) [relu] [+ the block's input, behind the last unit of a residual block]
//
// x_u is the previous unit's h (the caller's x for unit 0).  With YL_HEAD_SAVE the handle keeps a copy of x and every
// unit's z, h and (mean, invstd); without it one z and ROT rotating h.  The backward walks the units last first down to
// the first one something is wanted of.  ROT gradient buffers rotate: a residual block's output gradient G stays in one of
// them until the block's input gradient exists and is then added to it; the others carry dz (in place where dh may be
// overwritten) and the unit's input gradient.
// A stack without residual blocks is the special case in which every unit is a block of its own (first = last = 1,
// res = 0): bin follows in, G and keep are never set, pick() only ever answers 0 and 1 -- pick(-1, -1) = 0, pick(0, 0) = 1,
// pick(1, 1) = 0 in the forward, pick(-1, t) = 1 - t in the backward -- so two buffers do (ROT = 2, the stem) and the
// third is never touched.
// What a translation unit supplies is a POLICY P:
//   P::ROT                       rotating buffers: 3 with residual blocks, 2 without
//   P::MIXED                     units without ReLU and residual blocks can occur.  false keeps the ACT_NONE instantiations
//                                of yl_bn.h's kernels and the add out of the object
//   P::RELU6                     units with ReLU6 can occur (the stage's variant, yl_variant_stage_set).  false keeps the
//                                ACT_RELU6 instantiations out of the object
//   P::layout(h, B, S, us, &n, &z)     the units and sizes of the handle's cfg (and variant) at (B, S); a status.  us and n
//                                are filled either way
//   P::conv_forward / conv_wgrad / conv_dgrad(s, u, B, ..., sb, mode)   the unit's convolution passes in the dense GEMMs'
//                                operand type `mode` (a depthwise unit has none) -> launches enqueued
//   P::add(s, io, g, n4)         io += g (MIXED only)
#ifndef YL_UNITS_H
#define YL_UNITS_H
#include <new>
#include <type_traits>

#include "yl_block.h"

namespace {

constexpr int MAX_UNITS = 4 * YL_STAGE_MAX_BLOCKS;
static_assert(YL_STEM_MAX_UNITS <= MAX_UNITS, "one unit array serves both stacks");

struct Unit {
  int block, slot;                       // the stage's: slot 0 dw_start, 1 pw_exp (cn), 2 dw_mid, 3 pw_proj of yl_stage_block
  int dw, planar;                        // depthwise / dense; the input is the planar image (the stem's unit 0)
  int act, k, st;                        // the activation behind the BatchNorm (yl_bn.h: ACT_NONE, ACT_RELU, ACT_RELU6); k x k of stride st
  int pb;                                // the leading pad of the k x k window (pad_begin), rows and columns alike
  int cin, cout, Sin, Sout;
  int64_t Min, Mout;                     // rows of the unit's input and output
  int stat_rows, tiles;                  // the row reductions: `tiles` tiles of stat_rows rows
  int wrows, wsplits;                    // the weight gradient's cut: 1x1 rows per split, dense 3x3 spatial tiles per split
  int first, last, res;                  // first / last unit of its block; res: the block adds its input (set on both)
};

inline int round4(int v) { return (v + 3) & ~3; }
inline int out_size(int S, int k, int st) { return (S + 2 * ((k - 1) / 2) - k) / st + 1; }
// the pad in front of the first row and column of an odd k x k convolution of stride st over S pixels: (k - 1) / 2 on every
// side, or with `same` TF-SAME's: total = max((So - 1) st + k - S, 0) with So = ceil(S / st) = out_size(S, k, st), of which
// the leading side gets total / 2 rounded down: (k - 1) / 2 - 1 when st == 2 and S is even, (k - 1) / 2 otherwise
inline int pad_begin(int k, int st, int S, int same) {
  if (!same) return (k - 1) / 2;
  const int total = (out_size(S, k, st) - 1) * st + k - S;
  return total > 0 ? total / 2 : 0;
}

// bytes, but cmax: channels.  x0 (the caller's x), xsave (its saved copy) and gmax (one gradient buffer) are the
// translation unit's to set; the rest is unit_sizes'
struct Sizes { int64_t x0, xsave, gmax, amax, cmax, smax, pmax, wmax; };
// the maxima over the units: one activation, the channels, the partial sums of a row reduction (a depthwise weight
// gradient has k^2 per tile, everything else 2), a dense k x k unit's packed weight, a dense unit's weight-gradient partials.
// false: a shape the kernels' index arithmetic does not cover
inline bool unit_sizes(const Unit* us, int n, int chan_max, Sizes* z) {
  memset(z, 0, sizeof(*z));
  for (int i = 0; i < n; ++i) {
    const Unit& u = us[i];
    if (u.Mout * u.cout >= ((int64_t)1 << 40) || u.cin > chan_max || u.cout > chan_max) return false;
    const int64_t a = u.Mout * u.cout * 4;
    z->amax = a > z->amax ? a : z->amax;
    z->cmax = u.cout > z->cmax ? u.cout : z->cmax;
    const int64_t sp = round16((int64_t)u.tiles * (u.dw ? u.k * u.k : 2) * u.cout * 8);
    z->smax = sp > z->smax ? sp : z->smax;
    if (u.dw) continue;
    const int64_t wp = u.k == 1 ? round16((int64_t)u.wsplits * u.cin * u.cout * 4)
                                : round16((int64_t)u.wsplits * u.k * u.k * u.cout * round4(u.cin) * 4);
    z->wmax = wp > z->wmax ? wp : z->wmax;
    if (u.k > 1) {
      const int64_t pk = round16((int64_t)u.k * u.k * u.cout * round4(u.cin) * 4);
      z->pmax = pk > z->pmax ? pk : z->pmax;
    }
  }
  return true;
}
inline int64_t unit_saved_bytes(const Unit& u) { return 2 * u.Mout * u.cout * 4 + 2 * (int64_t)u.cout * 4; }   // z, h, (mean, invstd)
// what the two arenas hold with `rot` rotating buffers: both plans report these, and units_reserve cuts them
struct ArenaBytes { int64_t saved, nosave, work; };
inline ArenaBytes arena_bytes(const Unit* us, int n, const Sizes& z, int rot) {
  ArenaBytes b;
  b.saved = z.xsave;
  for (int i = 0; i < n; ++i) b.saved += unit_saved_bytes(us[i]);
  b.nosave = (1 + rot) * z.amax + 2 * z.cmax * 4;
  b.work = rot * z.gmax + z.smax + 2 * z.cmax * 4 + z.pmax + z.wmax;
  return b;
}

struct UnitBuffers {
  float* x;                              // save: the copy of the caller's x
  float *z[MAX_UNITS], *h[MAX_UNITS], *stats[MAX_UNITS];   // save: per unit
  float *nz, *nh[3], *nstats;            // no save: one z, `rot` rotating h, one (mean, invstd)
  float *g[3], *coef, *wpack, *wpart;    // `rot` rotating gradients, the BatchNorm backward's coefficients, pack, partials
  double* spart;
};
// the handle's memory for the units, cut as arena_bytes counts it
inline yl_status units_reserve(Arena& mem, const Unit* us, int n, const Sizes& z, int rot, bool save, UnitBuffers* sb) {
  const ArenaBytes b = arena_bytes(us, n, z, rot);
  const yl_status st = arena_reserve(mem, save ? b.saved : b.nosave, b.work);
  if (st != YL_OK) return st;
  char* w = mem.work;
  for (int i = 0; i < rot; ++i) { sb->g[i] = (float*)w; w += z.gmax; }
  sb->spart = (double*)w; w += z.smax;
  sb->coef = (float*)w; w += 2 * z.cmax * 4;
  sb->wpack = (float*)w; w += z.pmax;
  sb->wpart = (float*)w;
  char* p = mem.saved;
  if (save) {
    sb->x = (float*)p; p += z.xsave;
    for (int i = 0; i < n; ++i) {
      const size_t a = (size_t)us[i].Mout * us[i].cout * 4;
      sb->z[i] = (float*)p; p += a;
      sb->h[i] = (float*)p; p += a;
      sb->stats[i] = (float*)p; p += 2 * (size_t)us[i].cout * 4;
    }
  } else {
    sb->nz = (float*)p; p += z.amax;
    for (int i = 0; i < rot; ++i) { sb->nh[i] = (float*)p; p += z.amax; }
    sb->nstats = (float*)p;
  }
  return YL_OK;
}

// a parameter table, resolved to one entry per unit: every tensor there, 4-byte aligned, the counter 8-byte aligned
inline bool params_ok(const yl_stage_unit* const* tab, int n) {
  uintptr_t any = 0;
  for (int i = 0; i < n; ++i) {
    const yl_stage_unit& e = *tab[i];
    if (!e.w || !e.gamma || !e.beta || !e.running_mean || !e.running_var || !e.num_batches_tracked) return false;
    any |= (uintptr_t)e.w | (uintptr_t)e.gamma | (uintptr_t)e.beta | (uintptr_t)e.running_mean | (uintptr_t)e.running_var;
    if ((uintptr_t)e.num_batches_tracked & 7u) return false;
  }
  return !(any & 3u);
}
// a gradient table: -> the first unit something is wanted of (n: none); *bits: every wanted pointer or'ed
inline int first_wanted(const yl_stage_unit* const* tab, int n, bool want_dx, uintptr_t* bits) {
  int first = want_dx ? 0 : n;
  *bits = 0;
  for (int i = n - 1; i >= 0; --i) {
    const uintptr_t any = (uintptr_t)tab[i]->w | (uintptr_t)tab[i]->gamma | (uintptr_t)tab[i]->beta;
    *bits |= any;
    if (any && i < first) first = i;
  }
  return first;
}

inline int pick(int a, int b) {          // a rotating buffer that is neither a nor b
  for (int i = 0; i < 3; ++i)
    if (i != a && i != b) return i;
  return 0;
}

// ---- the handle: struct yl_stage / yl_stem derive from it
template <class Cfg> struct UnitStack {
  Arena mem;                             // yl_block.h
  Cfg cfg;
  int fB, fS, fTrain;                    // the forward whose activations are held (mem.fValid)
  int mode, fMode;                       // the dense GEMMs' operand type (yl_block.h: 0 fp32, 1 fp16, 2 bf16): of the next
                                         // forward (yl_amp_*_set) and of the held one, which its backward runs in
  int act = ACT_RELU, same = 0;          // the stage's variant (yl_variant_stage_set): the activation of every activated
                                         // unit, TF-SAME padding.  Not changed while a forward is held
};
// yl_amp_*_set / _get: the mode as the bits of the heads' flags (0, YL_HEAD_F16, YL_HEAD_BF16)
inline uint32_t mode_bits(int mode) { return mode == 1 ? YL_HEAD_F16 : (mode == 2 ? YL_HEAD_BF16 : 0u); }
inline int mode_of_bits(uint32_t bits) {                   // anything but the three values: -1
  return bits == 0 ? 0 : (bits == YL_HEAD_F16 ? 1 : (bits == YL_HEAD_BF16 ? 2 : -1));
}
template <class H> yl_status units_amp_set(H* h, uint32_t bits) {
  const int m = mode_of_bits(bits);
  if (!h || m < 0) return YL_ERR_INVALID;
  h->mode = m;                           // a held forward keeps fMode
  return YL_OK;
}
template <class H> yl_status units_amp_get(const H* h, uint32_t* mode, uint32_t* held_mode) {
  if (!h) return YL_ERR_INVALID;
  if (mode) *mode = mode_bits(h->mode);
  if (held_mode) *held_mode = h->mem.fValid ? mode_bits(h->fMode) : 0u;
  return YL_OK;
}
template <class H, class Cfg> yl_status units_create(int device, const Cfg* cfg, bool cfg_ok, H** out) {
  if (!out || !cfg_ok) return YL_ERR_INVALID;
  if (hipSetDevice(device) != hipSuccess) return YL_ERR_HIP;
  H* h = new (std::nothrow) H();
  if (!h) return YL_ERR_NOMEM;
  h->mem.device = device; h->cfg = *cfg;
  *out = h;
  return YL_OK;
}
template <class H> void units_destroy(H* h) {
  if (!h) return;
  arena_release(h->mem);
  delete h;
}
template <class H> yl_status units_held(const H* h, int64_t* saved_bytes, int64_t* workspace_bytes, int32_t* forward_held) {
  return arena_held(h ? &h->mem : nullptr, saved_bytes, workspace_bytes, forward_held);
}

// unit u's BatchNorm: its statistics in `stats`, the partial sums of its row reductions in the stack's spart
inline BnLayer bn_of(const Unit& u, const yl_stage_unit& e, double eps, float* stats, const UnitBuffers& sb) {
  return {(int)u.Mout, u.cout, u.stat_rows, u.tiles, e.gamma, e.beta, e.running_mean, e.running_var, e.num_batches_tracked, eps,
          stats, sb.spart};
}

// f(the unit's activation as a constant) -> what it returns: ACT_RELU, ACT_RELU6 where the policy has it, ACT_NONE where the
// policy has it; anything else runs nothing.  The BatchNorm instantiations a translation unit gets are the ones named here
template <class P, class F> inline int by_act(int act, F f) {
  if (act == ACT_RELU) return f(std::integral_constant<int, ACT_RELU>());
  if constexpr (P::RELU6) {
    if (act == ACT_RELU6) return f(std::integral_constant<int, ACT_RELU6>());
  }
  if constexpr (P::MIXED) return f(std::integral_constant<int, ACT_NONE>());
  return 0;
}

// ---- forward.  par: the parameters, one entry per unit (npar of them: which units exist does not depend on the shape);
// xmask: the alignment of x_dev.  The caller has checked its pointers and batch, size >= 1
template <class P, class H>
yl_status units_forward(H* h, const yl_stage_unit* const* par, int npar, const float* x_dev, unsigned xmask, int batch, int size,
                        uint32_t flags, float* out_dev, void* stream, int32_t* launches) {
  if (!params_ok(par, npar)) return YL_ERR_INVALID;
  if (flags & ~(uint32_t)(YL_HEAD_TRAIN | YL_HEAD_SAVE)) return YL_ERR_INVALID;       // no precision bits: yl_amp_*_set
  if (((uintptr_t)x_dev & xmask) || ((uintptr_t)out_dev & 15u)) return YL_ERR_UNSUPPORTED;
  const bool train = flags & YL_HEAD_TRAIN, save = flags & YL_HEAD_SAVE;
  Unit us[MAX_UNITS];
  Sizes sz;
  int n;
  const yl_status lst = P::layout(*h, batch, size, us, &n, &sz);
  for (int i = 0; i < n; ++i)
    if (us[i].Mout < 1 || (train && us[i].Mout < 2)) return YL_ERR_INVALID;            // no variance of one value
  if (lst != YL_OK) return lst;
  UnitBuffers sb;
  const yl_status st = units_reserve(h->mem, us, n, sz, P::ROT, save, &sb);
  if (st != YL_OK) return st;
  hipStream_t s = (hipStream_t)stream;
  const int mode = h->mode;
  h->mem.fValid = 0;
  if (save && hipMemcpyAsync(sb.x, x_dev, (size_t)sz.x0, hipMemcpyDeviceToDevice, s) != hipSuccess) return YL_ERR_HIP;
  int nl = 0;
  const float* in = save ? sb.x : x_dev;
  const float* bin = in;                 // the input of the block the walk is in
  int in_i = -1, bin_i = -1;             // no save: which rotating buffer holds them (-1: none of them)
  for (int i = 0; i < n; ++i) {
    const Unit& u = us[i];
    const yl_stage_unit& e = *par[i];
    if (u.first) { bin = in; bin_i = in_i; }
    float* z = save ? sb.z[i] : sb.nz;
    float* stats = save ? sb.stats[i] : sb.nstats;
    int out_i = -1;
    float* hout;
    if (save) hout = sb.h[i];
    else if (i == n - 1) hout = out_dev;
    else { out_i = pick(in_i, bin_i); hout = sb.nh[out_i]; }
    nl += P::conv_forward(s, u, batch, in, e.w, z, sb, mode);
    const BnLayer bn = bn_of(u, e, h->cfg.eps, stats, sb);
    const float* res = (u.last && u.res) ? bin : nullptr;
    nl += by_act<P>(u.act, [&](auto A) { return bn_forward<decltype(A)::value>(s, bn, train, z, res, hout); });
    in = hout; in_i = out_i;
  }
  if (save) {
    const Unit& u = us[n - 1];
    if (hipMemcpyAsync(out_dev, in, (size_t)u.Mout * u.cout * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return YL_ERR_HIP;
  }
  if (launches) *launches = nl;
  if (hipGetLastError() != hipSuccess) return YL_ERR_HIP;
  if (save) { h->fB = batch; h->fS = size; h->fTrain = train ? 1 : 0; h->fMode = mode; h->mem.fValid = 1; }
  return YL_OK;
}

// ---- backward of the held forward.  par, grd: parameters and where their gradients go, one entry per unit.  The caller
// has checked its pointers (dx_dev may be NULL)
template <class P, class H>
yl_status units_backward(H* h, const yl_stage_unit* const* par, const yl_stage_unit* const* grd, int npar, const float* gy_dev,
                         float* dx_dev, void* stream, int32_t* launches) {
  if (!params_ok(par, npar)) return YL_ERR_INVALID;
  if (((uintptr_t)gy_dev & 15u) || ((uintptr_t)dx_dev & 15u)) return YL_ERR_UNSUPPORTED;
  if (!h->mem.fValid) return YL_ERR_STATE;
  Unit us[MAX_UNITS];
  Sizes sz;
  int n;
  yl_status st = P::layout(*h, h->fB, h->fS, us, &n, &sz);
  if (st != YL_OK) return st;
  UnitBuffers sb;
  st = units_reserve(h->mem, us, n, sz, P::ROT, true, &sb);
  if (st != YL_OK) return st;
  if (!h->mem.fValid) return YL_ERR_STATE;
  uintptr_t gany;
  const int first = first_wanted(grd, n, dx_dev != nullptr, &gany);
  if (gany & 3u) return YL_ERR_UNSUPPORTED;                // before the first launch: nothing of the caller's is written
  hipStream_t s = (hipStream_t)stream;
  const bool train = h->fTrain != 0;
  const int B = h->fB, mode = h->fMode;  // the backward runs in the precision of its forward
  int nl = 0;
  const float* dh = gy_dev;
  int cur = -1;                          // the buffer dh is in (-1: the caller's gy)
  const float* G = nullptr;              // the output gradient of the residual block the walk is in
  int keep = -1;                         // the buffer G is in (-1: none of them)
  for (int i = n - 1; i >= first; --i) {
    const Unit& u = us[i];
    const yl_stage_unit& e = *par[i];
    const yl_stage_unit& g = *grd[i];
    const float* xin = i ? sb.h[i - 1] : sb.x;
    if (u.last && u.res) { G = dh; keep = cur; }
    const BnLayer bn = bn_of(u, e, h->cfg.eps, sb.stats[i], sb);
    // sum g, sum g * xhat: dbeta, dgamma and the batch statistics' two means
    nl += by_act<P>(u.act, [&](auto A) {
      return bn_backward_sums<decltype(A)::value>(s, bn, train, dh, sb.h[i], sb.z[i], g.gamma, g.beta, sb.coef);
    });
    const bool need_dx = i > first || (i == 0 && dx_dev);
    if (!need_dx && !g.w) break;
    const int t = (cur >= 0 && cur != keep) ? cur : pick(keep, -1);      // dz: in place unless dh must survive
    float* dz = sb.g[t];
    nl += by_act<P>(u.act, [&](auto A) { return bn_backward_dz<decltype(A)::value>(s, bn, dh, sb.h[i], sb.z[i], sb.coef, dz); });
    if (g.w) nl += P::conv_wgrad(s, u, B, xin, dz, g.w, sb, mode);
    if (!need_dx) break;
    const int d = pick(keep, t);
    float* dst = i ? sb.g[d] : dx_dev;
    nl += P::conv_dgrad(s, u, B, dz, e.w, dst, sb, mode);
    if constexpr (P::MIXED) {
      if (u.first && u.res) {            // the block's input also went straight to its output
        const long m4 = (long)u.Min * (u.cin >> 2);
        P::add(s, dst, G, m4);
        ++nl;
        G = nullptr; keep = -1;
      }
    }
    dh = dst; cur = d;
  }
  if (launches) *launches = nl;
  return hipGetLastError() == hipSuccess ? YL_OK : YL_ERR_HIP;
}

}  // namespace
#endif  // YL_UNITS_H
