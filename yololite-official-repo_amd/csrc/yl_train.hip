// The training step's tail on the device (reference tools/train.py:352-359): GradScaler.unscale_, clip_grad_norm_,
// GradScaler.step(AdamW | Adam | Nesterov SGD), GradScaler.update and ModelEMA.update as THREE launches, whatever
// the number of tensors.
//
// Every tensor of the step is one row of a segment table in device memory (parameter, two optimizer states, EMA
// entry, element count, parameter group, flags); the gradient pointers are a column of their own because
// zero_grad(set_to_none=True) gives every gradient a new address each step (yl_train_set_grads re-uploads that
// column only).  Work is cut into chunks (segment, offset, length) by yl_train_plan on the host; a chunk never
// crosses a tensor, and every kernel strides a capped grid over the chunk list.
//
//   1. yl_train_stats_kernel   reads every gradient once: per chunk the sum of squares of fp32(grad * inv_scale) in
//                              float64 and a non-finite flag, written to buffers indexed by chunk (no atomics)
//   2. yl_train_reduce_kernel  one workgroup: sums the partials in chunk order in float64, writes norm / found_inf,
//                              applies GradScaler.update to scale and tracker, and advances the step count of every
//                              tensor that has a gradient -- unless the step is skipped
//   3. yl_train_apply_kernel   per chunk: optimizer update of parameter and state from g = grad * inv_scale * clip
//                              (skipped as a whole on found_inf), then ema = ema * d + value * (1 - d) from the value
//                              just written; EMA-only entries read the model's buffer, integer entries are copied
//
// Arithmetic: the unscale is torch's fp32 multiply; everything after it is evaluated in float64 from the fp32
// operands and rounded once per stored value (parameter, each state, EMA entry).  Loads and stores are 16 bytes
// wide where the chunk's pointers share their offset within 16 bytes; a misaligned head and the tail are scalar.
// Which thread sums which element, and in which order, is fixed by the chunk list alone: equal inputs, equal bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <new>
#include <vector>

#include "../../include/yololite_hip.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_GRID = 2048;          // 256 CUs x 8 workgroups: the cap of a streaming grid
constexpr int RING = 4;                 // pinned staging buffers of the gradient-pointer column

struct Seg {                            // device row; the host's yl_train_segment without its gradient
  float* p; float* s0; float* s1; float* ema;
  int64_t n; int32_t group; uint32_t flags;
};

struct State {                          // YL_TRAIN_STATE_WORDS 4-byte words, in the caller's memory
  float scale; int32_t tracker; float norm; int32_t found_inf;
  float inv_scale; int32_t skip; double norm64;
};
static_assert(sizeof(State) == 4 * YL_TRAIN_STATE_WORDS, "state block layout");
static_assert(sizeof(yl_train_chunk) == 16, "chunk layout");

__device__ __forceinline__ double yl_block_sum(double v, double* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int m = NT / 2; m >= 1; m >>= 1) {
    if (tid < m) sh[tid] += sh[tid + m];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// elements before the first 16-byte boundary of `ptr` (at most len)
__device__ __forceinline__ int yl_head(const void* ptr, int len) {
  const int h = (int)(((16u - (unsigned)((uintptr_t)ptr & 15u)) & 15u) >> 2);
  return h < len ? h : len;
}

__global__ __launch_bounds__(NT) void yl_train_stats_kernel(const Seg* segs, const float* const* grads,
                                                            const yl_train_chunk* chunks, int nchunks,
                                                            const State* st, double* partial, int32_t* flags) {
  __shared__ double sh[NT];
  const int tid = threadIdx.x;
  const float inv = st->scale == 1.0f ? 1.0f : (float)(1.0 / (double)st->scale);
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const yl_train_chunk ck = chunks[c];
    const float* g = grads[ck.seg];
    if (!g || (segs[ck.seg].flags & (YL_TRAIN_SEG_EMA_ONLY | YL_TRAIN_SEG_BYTES))) {
      if (tid == 0) { partial[c] = 0.0; flags[c] = 0; }
      continue;
    }
    g += ck.off;
    const int len = ck.len;
    const int head = yl_head(g, len);
    const int nvec = (len - head) >> 2;
    double acc = 0.0;
    int bad = 0;
    auto take = [&](float x) {
      bad |= !isfinite(x);
      const float u = x * inv;                       // GradScaler.unscale_: an fp32 product
      acc += (double)u * (double)u;
    };
    for (int i = tid; i < head; i += NT) take(g[i]);
    const float4* gv = reinterpret_cast<const float4*>(g + head);
    for (int v = tid; v < nvec; v += NT) {
      const float4 x = gv[v];
      take(x.x); take(x.y); take(x.z); take(x.w);
    }
    for (int i = head + 4 * nvec + tid; i < len; i += NT) take(g[i]);
    const double s = yl_block_sum(acc, sh);
    const int anybad = __syncthreads_or(bad);
    if (tid == 0) { partial[c] = s; flags[c] = anybad; }
  }
}

struct ReduceP {
  const Seg* segs; const float* const* grads; float* steps; int nseg;
  const double* partial; const int32_t* flags; int nchunks;
  State* st; int amp; double growth, backoff; int interval;
};

__global__ __launch_bounds__(NT) void yl_train_reduce_kernel(ReduceP p) {
  __shared__ double sh[NT];
  const int tid = threadIdx.x;
  // thread t owns a contiguous run of chunks and adds them in order; the 256 runs are then added by a fixed tree
  const int per = (p.nchunks + NT - 1) / NT;
  const int b = tid * per, e = b + per < p.nchunks ? b + per : p.nchunks;
  double acc = 0.0;
  int bad = 0;
  for (int c = b; c < e; ++c) { acc += p.partial[c]; bad |= p.flags[c]; }
  const double total = yl_block_sum(acc, sh);
  const int found = __syncthreads_or(bad) ? 1 : 0;
  const int skip = (p.amp && found) ? 1 : 0;
  if (tid == 0) {
    State* st = p.st;
    const double nrm = sqrt(total);
    const float scale = st->scale;
    st->norm64 = nrm;
    st->norm = (float)nrm;
    st->found_inf = found;
    st->skip = skip;
    st->inv_scale = scale == 1.0f ? 1.0f : (float)(1.0 / (double)scale);
    if (p.amp) {                                     // GradScaler.update (torch's amp_update_scale kernel)
      if (found) {
        st->scale = (float)((double)scale * p.backoff);
        st->tracker = 0;
      } else {
        const int ok = st->tracker + 1;
        if (ok == p.interval) {
          const float ns = (float)((double)scale * p.growth);
          if (isfinite(ns)) st->scale = ns;
          st->tracker = 0;
        } else {
          st->tracker = ok;
        }
      }
    }
  }
  if (!skip)
    for (int s = tid; s < p.nseg; s += NT)
      if (p.grads[s] && !(p.segs[s].flags & (YL_TRAIN_SEG_EMA_ONLY | YL_TRAIN_SEG_BYTES))) p.steps[s] += 1.0f;
}

struct ApplyP {
  const Seg* segs; const float* const* grads; const float* steps;
  const yl_train_chunk* chunks; int nchunks;
  const State* st;
  int nesterov;
  double lr[YL_TRAIN_MAX_GROUPS], wd[YL_TRAIN_MAX_GROUPS];
  double beta1, beta2, eps, momentum, ema_d, max_norm;
};

struct ElemC {                          // what one chunk's elements share
  float inv;                            // unscale factor (fp32, as torch multiplies)
  double clip, lr, wd, decay;           // decay = 1 - lr * wd (AdamW)
  double omb1, b2, omb2, step_size, bc2_sqrt, eps;     // Adam family
  double mom; int first, nesterov;      // SGD
  double d, omd;                        // EMA
};

template <int W>
__device__ __forceinline__ void yl_ld(const float* p, float* o) {
  if constexpr (W == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {
    o[0] = *p;
  }
}
template <int W>
__device__ __forceinline__ void yl_st(float* p, const float* o) {
  if constexpr (W == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
    *p = o[0];
  }
}

// torch 2.10 _single_tensor_adam / _single_tensor_sgd on one element, float64 from fp32 operands
template <int KIND>
__device__ __forceinline__ void yl_update(float& pf, float gf, float& af, float& bf, const ElemC& c) {
  double p = (double)pf;
  double g = (double)(gf * c.inv) * c.clip;
  if constexpr (KIND == YL_TRAIN_SGD) {
    if (c.wd != 0.0) g += c.wd * p;
    double buf = g;
    if (c.mom != 0.0) {
      buf = c.first ? g : c.mom * (double)af + g;
      af = (float)buf;
      g = c.nesterov ? g + c.mom * buf : buf;
    }
    p -= c.lr * g;
  } else {
    if constexpr (KIND == YL_TRAIN_ADAMW) {
      if (c.wd != 0.0) p *= c.decay;
    } else {
      if (c.wd != 0.0) g += c.wd * p;
    }
    const double m = (double)af + (g - (double)af) * c.omb1;          // exp_avg.lerp_(grad, 1 - beta1)
    const double v = (double)bf * c.b2 + c.omb2 * (g * g);            // mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    af = (float)m;
    bf = (float)v;
    p -= c.step_size * (m / (sqrt(v) / c.bc2_sqrt + c.eps));
  }
  pf = (float)p;
}

template <int KIND, int W>
__device__ __forceinline__ void yl_apply_at(const Seg& s, const float* g, int64_t i, bool upd, const ElemC& c) {
  float p[W], a[W], b[W], e[W], gr[W];
  yl_ld<W>(s.p + i, p);
  if (upd) {
    yl_ld<W>(g + i, gr);
    if (KIND != YL_TRAIN_SGD || c.mom != 0.0) yl_ld<W>(s.s0 + i, a);
    if constexpr (KIND != YL_TRAIN_SGD) yl_ld<W>(s.s1 + i, b);
#pragma unroll
    for (int k = 0; k < W; ++k) yl_update<KIND>(p[k], gr[k], a[k], b[k], c);
    yl_st<W>(s.p + i, p);
    if (KIND != YL_TRAIN_SGD || c.mom != 0.0) yl_st<W>(s.s0 + i, a);
    if constexpr (KIND != YL_TRAIN_SGD) yl_st<W>(s.s1 + i, b);
  }
  if (s.ema) {
    yl_ld<W>(s.ema + i, e);
#pragma unroll
    for (int k = 0; k < W; ++k) e[k] = (float)((double)e[k] * c.d + (double)p[k] * c.omd);
    yl_st<W>(s.ema + i, e);
  }
}

template <int KIND>
__global__ __launch_bounds__(NT) void yl_train_apply_kernel(ApplyP P) {
  __shared__ ElemC shc;
  const int tid = threadIdx.x;
  const int skip = P.st->skip;
  for (int ci = blockIdx.x; ci < P.nchunks; ci += gridDim.x) {
    const yl_train_chunk ck = P.chunks[ci];
    const Seg s = P.segs[ck.seg];
    if (s.flags & YL_TRAIN_SEG_BYTES) {              // integer state_dict entry: v.copy_(msd[k])
      const unsigned char* src = reinterpret_cast<const unsigned char*>(s.p) + ck.off;
      unsigned char* dst = reinterpret_cast<unsigned char*>(s.ema) + ck.off;
      for (int i = tid; i < ck.len; i += NT) dst[i] = src[i];
      continue;
    }
    const float* g = (s.flags & YL_TRAIN_SEG_EMA_ONLY) ? nullptr : P.grads[ck.seg];
    const bool upd = g && !skip;
    if (!upd && !s.ema) continue;
    if (tid == 0) {
      ElemC c;
      memset(&c, 0, sizeof(c));
      c.inv = P.st->inv_scale;
      const double nrm = P.st->norm64;
      c.clip = 1.0;
      if (P.max_norm > 0.0) { const double q = P.max_norm / (nrm + 1e-6); c.clip = q < 1.0 ? q : 1.0; }
      c.lr = P.lr[s.group]; c.wd = P.wd[s.group];
      c.decay = 1.0 - c.lr * c.wd;
      c.eps = P.eps; c.mom = P.momentum; c.nesterov = P.nesterov;
      c.d = P.ema_d; c.omd = 1.0 - P.ema_d;
      if (upd) {
        const double step = (double)P.steps[ck.seg];                  // already advanced by the reduce launch
        c.first = step == 1.0;
        if (KIND != YL_TRAIN_SGD) {
          c.omb1 = 1.0 - P.beta1; c.b2 = P.beta2; c.omb2 = 1.0 - P.beta2;
          c.step_size = c.lr / (1.0 - pow(P.beta1, step));
          c.bc2_sqrt = sqrt(1.0 - pow(P.beta2, step));
        }
      }
      shc = c;
    }
    __syncthreads();
    const ElemC c = shc;
    const int64_t o = ck.off;
    const int len = ck.len;
    // one vector body needs every stream of this chunk at the same offset within 16 bytes
    const unsigned al = (unsigned)((uintptr_t)(s.p + o) & 15u);
    bool same = true;
    if (upd) {
      same = same && ((unsigned)((uintptr_t)(g + o) & 15u) == al);
      if (KIND != YL_TRAIN_SGD || c.mom != 0.0) same = same && ((unsigned)((uintptr_t)(s.s0 + o) & 15u) == al);
      if (KIND != YL_TRAIN_SGD) same = same && ((unsigned)((uintptr_t)(s.s1 + o) & 15u) == al);
    }
    if (s.ema) same = same && ((unsigned)((uintptr_t)(s.ema + o) & 15u) == al);
    const int head = same ? yl_head(s.p + o, len) : len;
    const int nvec = (len - head) >> 2;
    for (int i = tid; i < head; i += NT) yl_apply_at<KIND, 1>(s, g, o + i, upd, c);
    for (int v = tid; v < nvec; v += NT) yl_apply_at<KIND, 4>(s, g, o + head + 4 * v, upd, c);
    for (int i = head + 4 * nvec + tid; i < len; i += NT) yl_apply_at<KIND, 1>(s, g, o + i, upd, c);
    __syncthreads();                                 // shc is rewritten for the next chunk
  }
}

bool yl_is_float_seg(uint32_t flags) { return !(flags & YL_TRAIN_SEG_BYTES); }
bool yl_is_param_seg(uint32_t flags) { return !(flags & (YL_TRAIN_SEG_BYTES | YL_TRAIN_SEG_EMA_ONLY)); }

}  // namespace

struct yl_train {
  int device, kind, nseg, amp;
  int64_t nchunks;
  double growth, backoff;
  int interval;
  Seg* segs_dev;
  const float** grads_dev;
  yl_train_chunk* chunks_dev;
  double* partial_dev;
  int32_t* flags_dev;
  float* steps_dev;
  State* st;                            // the caller's state block
  std::vector<uint32_t> seg_flags;
  std::vector<const void*> grads_host;  // what the device column holds
  bool grads_sent;
  void* pinned[RING];
  hipEvent_t ev[RING];
  bool ev_used[RING];
  int ring;
};

extern "C" {

int64_t yl_train_plan(const int64_t* counts_host, int32_t nseg, int32_t chunk_elems, yl_train_chunk* out_host,
                      int64_t capacity) {
  if (!counts_host || nseg < 0 || chunk_elems < 4 || (chunk_elems & 3)) return YL_ERR_INVALID;
  int64_t n = 0;
  for (int32_t s = 0; s < nseg; ++s) {
    if (counts_host[s] < 0) return YL_ERR_INVALID;
    for (int64_t o = 0; o < counts_host[s]; o += chunk_elems, ++n) {
      if (!out_host) continue;
      if (n >= capacity) return YL_ERR_CAPACITY;
      const int64_t left = counts_host[s] - o;
      out_host[n].seg = s;
      out_host[n].len = (int32_t)(left < chunk_elems ? left : chunk_elems);
      out_host[n].off = o;
    }
  }
  return n;
}

void yl_train_destroy(yl_train* t) {
  if (!t) return;
  hipSetDevice(t->device);
  hipDeviceSynchronize();
  hipFree(t->segs_dev); hipFree((void*)t->grads_dev); hipFree(t->chunks_dev); hipFree(t->partial_dev);
  hipFree(t->flags_dev); hipFree(t->steps_dev);
  for (int k = 0; k < RING; ++k) {
    if (t->pinned[k]) hipHostFree(t->pinned[k]);
    if (t->ev[k]) hipEventDestroy(t->ev[k]);
  }
  (void)hipGetLastError();
  delete t;
}

yl_status yl_train_create(int32_t device, const yl_train_cfg* cfg, const yl_train_segment* segments_host, int32_t nseg,
                          void* state_dev, yl_train** out) {
  if (!out || !cfg || !segments_host || nseg <= 0 || !state_dev) return YL_ERR_INVALID;
  if (cfg->kind != YL_TRAIN_ADAMW && cfg->kind != YL_TRAIN_ADAM && cfg->kind != YL_TRAIN_SGD) return YL_ERR_INVALID;
  const int32_t chunk = cfg->chunk_elems ? cfg->chunk_elems : YL_TRAIN_CHUNK_DEFAULT;
  if (chunk < 4 || (chunk & 3) || ((uintptr_t)state_dev & 7u)) return YL_ERR_INVALID;
  if (cfg->amp && (!(cfg->init_scale > 0.0f) || cfg->growth_interval <= 0)) return YL_ERR_INVALID;
  std::vector<Seg> rows(nseg);
  std::vector<int64_t> counts(nseg);
  std::vector<const void*> grads(nseg, nullptr);
  std::vector<uint32_t> flags(nseg);
  for (int32_t s = 0; s < nseg; ++s) {
    const yl_train_segment& h = segments_host[s];
    if (h.count < 0 || (h.flags & ~(uint32_t)(YL_TRAIN_SEG_EMA_ONLY | YL_TRAIN_SEG_BYTES))) return YL_ERR_INVALID;
    if (h.count > 0 && !h.param) return YL_ERR_INVALID;
    if (h.group < 0 || h.group >= YL_TRAIN_MAX_GROUPS) return YL_ERR_UNSUPPORTED;
    if (!yl_is_param_seg(h.flags) && h.count > 0 && !h.ema) return YL_ERR_INVALID;
    if (yl_is_float_seg(h.flags)) {     // fp32 tensors start on a 4-byte boundary
      const uintptr_t any = (uintptr_t)h.param | (uintptr_t)h.grad | (uintptr_t)h.state0 | (uintptr_t)h.state1 |
                            (uintptr_t)h.ema;
      if (any & 3u) return YL_ERR_UNSUPPORTED;
    }
    if (yl_is_param_seg(h.flags) && h.count > 0) {
      if (!h.state0 || (cfg->kind != YL_TRAIN_SGD && !h.state1)) return YL_ERR_INVALID;
      grads[s] = h.grad;
    }
    rows[s].p = (float*)h.param; rows[s].s0 = (float*)h.state0; rows[s].s1 = (float*)h.state1;
    rows[s].ema = (float*)h.ema; rows[s].n = h.count; rows[s].group = h.group; rows[s].flags = h.flags;
    counts[s] = h.count;
    flags[s] = h.flags;
  }
  const int64_t nchunks = yl_train_plan(counts.data(), nseg, chunk, nullptr, 0);
  if (nchunks < 0) return (yl_status)nchunks;
  if (nchunks > (int64_t)1 << 30) return YL_ERR_UNSUPPORTED;
  std::vector<yl_train_chunk> chunks((size_t)nchunks);
  if (yl_train_plan(counts.data(), nseg, chunk, chunks.data(), nchunks) != nchunks) return YL_ERR_INVALID;
  if (hipSetDevice(device) != hipSuccess) return YL_ERR_HIP;
  yl_train* t = new (std::nothrow) yl_train();
  if (!t) return YL_ERR_NOMEM;
  t->device = device; t->kind = cfg->kind; t->nseg = nseg; t->amp = cfg->amp ? 1 : 0; t->nchunks = nchunks;
  t->growth = cfg->growth_factor; t->backoff = cfg->backoff_factor; t->interval = cfg->growth_interval;
  t->st = (State*)state_dev;
  t->seg_flags = flags;
  t->grads_host = grads;
  t->grads_sent = true;
  const size_t nc = (size_t)(nchunks > 0 ? nchunks : 1);
  bool ok = true;
  ok = ok && hipMalloc(&t->segs_dev, sizeof(Seg) * nseg) == hipSuccess;
  ok = ok && hipMalloc((void**)&t->grads_dev, sizeof(void*) * nseg) == hipSuccess;
  ok = ok && hipMalloc(&t->chunks_dev, sizeof(yl_train_chunk) * nc) == hipSuccess;
  ok = ok && hipMalloc(&t->partial_dev, sizeof(double) * nc) == hipSuccess;
  ok = ok && hipMalloc(&t->flags_dev, sizeof(int32_t) * nc) == hipSuccess;
  ok = ok && hipMalloc(&t->steps_dev, sizeof(float) * nseg) == hipSuccess;
  for (int k = 0; k < RING && ok; ++k) {
    ok = ok && hipHostMalloc(&t->pinned[k], sizeof(void*) * nseg, hipHostMallocDefault) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&t->ev[k], hipEventDisableTiming) == hipSuccess;
  }
  if (!ok) { yl_train_destroy(t); return YL_ERR_NOMEM; }
  State st0;
  memset(&st0, 0, sizeof(st0));
  st0.scale = cfg->amp ? cfg->init_scale : 1.0f;
  st0.inv_scale = 1.0f;
  ok = ok && hipMemcpy(t->segs_dev, rows.data(), sizeof(Seg) * nseg, hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipMemcpy((void*)t->grads_dev, grads.data(), sizeof(void*) * nseg, hipMemcpyHostToDevice) == hipSuccess;
  if (nchunks)
    ok = ok && hipMemcpy(t->chunks_dev, chunks.data(), sizeof(yl_train_chunk) * nc, hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipMemset(t->partial_dev, 0, sizeof(double) * nc) == hipSuccess;
  ok = ok && hipMemset(t->flags_dev, 0, sizeof(int32_t) * nc) == hipSuccess;
  ok = ok && hipMemset(t->steps_dev, 0, sizeof(float) * nseg) == hipSuccess;
  ok = ok && hipMemcpy(state_dev, &st0, sizeof(st0), hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipDeviceSynchronize() == hipSuccess;
  if (!ok) { yl_train_destroy(t); return YL_ERR_HIP; }
  *out = t;
  return YL_OK;
}

yl_status yl_train_set_grads(yl_train* t, const void* const* grad_ptrs_host, void* stream) {
  if (!t || !grad_ptrs_host) return YL_ERR_INVALID;
  bool changed = false;
  for (int s = 0; s < t->nseg; ++s) {
    const void* g = yl_is_param_seg(t->seg_flags[s]) ? grad_ptrs_host[s] : nullptr;
    if ((uintptr_t)g & 3u) return YL_ERR_UNSUPPORTED;
    changed = changed || g != t->grads_host[s];
  }
  if (!changed) return YL_OK;
  if (hipSetDevice(t->device) != hipSuccess) return YL_ERR_HIP;
  const int k = t->ring;
  // a staging buffer is rewritten only after the copy that last read it has run (RING steps ago: normally long done)
  if (t->ev_used[k] && hipEventSynchronize(t->ev[k]) != hipSuccess) return YL_ERR_HIP;
  const void** stage = (const void**)t->pinned[k];
  for (int s = 0; s < t->nseg; ++s) {
    stage[s] = yl_is_param_seg(t->seg_flags[s]) ? grad_ptrs_host[s] : nullptr;
    t->grads_host[s] = stage[s];
  }
  if (hipMemcpyAsync((void*)t->grads_dev, stage, sizeof(void*) * t->nseg, hipMemcpyHostToDevice,
                     (hipStream_t)stream) != hipSuccess)
    return YL_ERR_HIP;
  if (hipEventRecord(t->ev[k], (hipStream_t)stream) != hipSuccess) return YL_ERR_HIP;
  t->ev_used[k] = true;
  t->ring = (k + 1) % RING;
  return YL_OK;
}

yl_status yl_train_step(yl_train* t, const yl_train_hyper* h, void* stream) {
  if (!t || !h) return YL_ERR_INVALID;
  if (t->nchunks == 0) return YL_OK;
  if (hipSetDevice(t->device) != hipSuccess) return YL_ERR_HIP;
  hipStream_t s = (hipStream_t)stream;
  const int nchunks = (int)t->nchunks;
  const int grid = nchunks < MAX_GRID ? nchunks : MAX_GRID;
  hipLaunchKernelGGL(yl_train_stats_kernel, dim3(grid), dim3(NT), 0, s, t->segs_dev, t->grads_dev, t->chunks_dev,
                     nchunks, t->st, t->partial_dev, t->flags_dev);
  ReduceP r;
  r.segs = t->segs_dev; r.grads = t->grads_dev; r.steps = t->steps_dev; r.nseg = t->nseg;
  r.partial = t->partial_dev; r.flags = t->flags_dev; r.nchunks = nchunks;
  r.st = t->st; r.amp = t->amp; r.growth = t->growth; r.backoff = t->backoff; r.interval = t->interval;
  hipLaunchKernelGGL(yl_train_reduce_kernel, dim3(1), dim3(NT), 0, s, r);
  ApplyP a;
  a.segs = t->segs_dev; a.grads = t->grads_dev; a.steps = t->steps_dev; a.chunks = t->chunks_dev; a.nchunks = nchunks;
  a.st = t->st; a.nesterov = h->nesterov ? 1 : 0;
  for (int g = 0; g < YL_TRAIN_MAX_GROUPS; ++g) { a.lr[g] = h->lr[g]; a.wd[g] = h->weight_decay[g]; }
  a.beta1 = h->beta1; a.beta2 = h->beta2; a.eps = h->eps; a.momentum = h->momentum;
  a.ema_d = h->ema_decay; a.max_norm = h->max_norm;
  if (t->kind == YL_TRAIN_ADAMW)
    hipLaunchKernelGGL(yl_train_apply_kernel<YL_TRAIN_ADAMW>, dim3(grid), dim3(NT), 0, s, a);
  else if (t->kind == YL_TRAIN_ADAM)
    hipLaunchKernelGGL(yl_train_apply_kernel<YL_TRAIN_ADAM>, dim3(grid), dim3(NT), 0, s, a);
  else
    hipLaunchKernelGGL(yl_train_apply_kernel<YL_TRAIN_SGD>, dim3(grid), dim3(NT), 0, s, a);
  return hipGetLastError() == hipSuccess ? YL_OK : YL_ERR_HIP;
}

float* yl_train_scale_ptr(yl_train* t) { return t ? &t->st->scale : nullptr; }

yl_status yl_train_read_state(yl_train* t, float* scale, int32_t* growth_tracker, float* norm, int32_t* found_inf,
                              float* steps_host) {
  if (!t) return YL_ERR_INVALID;
  if (hipSetDevice(t->device) != hipSuccess) return YL_ERR_HIP;
  if (hipDeviceSynchronize() != hipSuccess) return YL_ERR_HIP;
  State st;
  if (hipMemcpy(&st, t->st, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess) return YL_ERR_HIP;
  if (scale) *scale = st.scale;
  if (growth_tracker) *growth_tracker = st.tracker;
  if (norm) *norm = st.norm;
  if (found_inf) *found_inf = st.found_inf;
  if (steps_host && hipMemcpy(steps_host, t->steps_dev, sizeof(float) * t->nseg, hipMemcpyDeviceToHost) != hipSuccess)
    return YL_ERR_HIP;
  return YL_OK;
}

yl_status yl_train_write_state(yl_train* t, float scale, int32_t growth_tracker, const float* steps_host) {
  if (!t || !(scale > 0.0f) || growth_tracker < 0) return YL_ERR_INVALID;
  if (steps_host)
    for (int s = 0; s < t->nseg; ++s)
      if (!(steps_host[s] >= 0.0f)) return YL_ERR_INVALID;
  if (hipSetDevice(t->device) != hipSuccess) return YL_ERR_HIP;
  if (hipDeviceSynchronize() != hipSuccess) return YL_ERR_HIP;
  State st;
  if (hipMemcpy(&st, t->st, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess) return YL_ERR_HIP;
  st.scale = t->amp ? scale : 1.0f;
  st.tracker = growth_tracker;
  if (hipMemcpy(t->st, &st, sizeof(st), hipMemcpyHostToDevice) != hipSuccess) return YL_ERR_HIP;
  if (steps_host && hipMemcpy(t->steps_dev, steps_host, sizeof(float) * t->nseg, hipMemcpyHostToDevice) != hipSuccess)
    return YL_ERR_HIP;
  return YL_OK;
}

}  // extern "C"
