// Host side of the layer program (yl_program.h): validate a yl_model_desc, pack a validated layer's weights into the
// images the kernels read, derive the executor's tables.  No HIP header, no device call.
#include "yl_program.h"

#include <stdio.h>
#include <string.h>

namespace {

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// MFMA fragment order: [tap][kblock][ntile][lane][s]  with
//   n = ntile*16 + (lane & 15),  c = kblock*16 + 4*(lane >> 4) + s     (see yl_conv.hip)
void pack_conv(const float* w, int cout, int cin, int k, std::vector<float>& out) {
  const int KB = cdiv(cin, 16), NT = cdiv(cout, 16), taps = k * k;
  out.assign((size_t)taps * KB * NT * 256, 0.0f);
  for (int tap = 0; tap < taps; ++tap)
    for (int kb = 0; kb < KB; ++kb)
      for (int nt = 0; nt < NT; ++nt)
        for (int lane = 0; lane < 64; ++lane)
          for (int s = 0; s < 4; ++s) {
            const int n = nt * 16 + (lane & 15);
            const int c = kb * 16 + 4 * (lane >> 4) + s;
            if (n < cout && c < cin)
              out[((((size_t)tap * KB + kb) * NT + nt) * 64 + lane) * 4 + s] =
                  w[((size_t)n * cin + c) * taps + tap];
          }
}

// Winograd F(2x2,3x3): U = G g G^T (4x4 per (cout, cin)), G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]], in the MFMA
// fragment order of pack_conv per transform position xi = 4i + j, grouped so that one (n-group of 2 n-tiles, k-block)
// chunk is 32 KiB contiguous: [ngroup][kblock][xi][nt 0..1][lane][s]   (yl_conv_wino_kernel)
void pack_wino(const float* w, int cout, int cin, std::vector<float>& out) {
  const int KB = cdiv(cin, 16), NG = cdiv(cdiv(cout, 16), 2);
  static const float G[4][3] = {{1.f, 0.f, 0.f}, {0.5f, 0.5f, 0.5f}, {0.5f, -0.5f, 0.5f}, {0.f, 0.f, 1.f}};
  out.assign((size_t)NG * KB * 16 * 2 * 256, 0.0f);
  for (int ng = 0; ng < NG; ++ng)
    for (int kb = 0; kb < KB; ++kb)
      for (int t = 0; t < 2; ++t)
        for (int lane = 0; lane < 64; ++lane)
          for (int s = 0; s < 4; ++s) {
            const int n = (ng * 2 + t) * 16 + (lane & 15);
            const int c = kb * 16 + 4 * (lane >> 4) + s;
            if (n >= cout || c >= cin) continue;
            const float* g = w + ((size_t)n * cin + c) * 9;
            float tmp[4][3];
            for (int i = 0; i < 4; ++i)
              for (int b = 0; b < 3; ++b) tmp[i][b] = G[i][0] * g[0 * 3 + b] + G[i][1] * g[1 * 3 + b] + G[i][2] * g[2 * 3 + b];
            for (int i = 0; i < 4; ++i)
              for (int j = 0; j < 4; ++j) {
                const float u = tmp[i][0] * G[j][0] + tmp[i][1] * G[j][1] + tmp[i][2] * G[j][2];
                out[(((((size_t)ng * KB + kb) * 16 + (i * 4 + j)) * 2 + t) * 64 + lane) * 4 + s] = u;
              }
          }
}

// depthwise [c][1][k][k] -> [tap][c]
void pack_dw(const float* w, int ch, int k, std::vector<float>& out) {
  out.assign((size_t)k * k * ch, 0.0f);
  for (int c = 0; c < ch; ++c)
    for (int t = 0; t < k * k; ++t) out[(size_t)t * ch + c] = w[(size_t)c * k * k + t];
}

// stem [cout][3][3][3] -> MFMA A fragments [kstep(7)][ntile][lane]: n = ntile*16 + (lane&15),
// k = 4*kstep + (lane>>4) with k = c*9 + ky*3 + kx (PyTorch OIHW flattening), zero for k >= 27
void pack_stem(const float* w, int cout, int cin, int k, std::vector<float>& out) {
  const int K = cin * k * k, KS = cdiv(K, 4), NT = cdiv(cout, 16);
  out.assign((size_t)KS * NT * 64, 0.0f);
  for (int s = 0; s < KS; ++s)
    for (int nt = 0; nt < NT; ++nt)
      for (int lane = 0; lane < 64; ++lane) {
        const int n = nt * 16 + (lane & 15), kk = 4 * s + (lane >> 4);
        if (n < cout && kk < K) out[((size_t)s * NT + nt) * 64 + lane] = w[(size_t)n * K + kk];
      }
}

// stem of the fused entry block (3 input channels, 3x3): K order by input rows, see yl_stemblock.hip
// bias (may be null): rides in the K = 27 -> 28 pad slot (s = 6, lane group 3) -- the kernel feeds 1.0 there, so the
// shift is the LAST product of every output's fma chain (the rounding of conv + shift)
void pack_stem_rows(const float* w, const float* bias, int cout, std::vector<float>& out) {
  const int KS = 7, NT = cdiv(cout, 16);
  out.assign((size_t)KS * NT * 64, 0.0f);
  for (int s = 0; s < KS; ++s)
    for (int nt = 0; nt < NT; ++nt)
      for (int lane = 0; lane < 64; ++lane) {
        const int n = nt * 16 + (lane & 15), kq = lane >> 4;
        int row, kx;
        if (s < 3) { row = 2 * kq; kx = s; }
        else if (s < 6) { row = 2 * kq + 1; kx = s - 3; }
        else if (kq < 3) { row = 8; kx = kq; }
        else {                                                       // pad slot: the bias
          if (n < cout && bias) out[((size_t)s * NT + nt) * 64 + lane] = bias[n];
          continue;
        }
        if (n < cout) out[((size_t)s * NT + nt) * 64 + lane] = w[(size_t)n * 27 + row * 3 + kx];
      }
}

// a status with its message: every check of the validation returns through one of these
struct Verdict {
  std::string* msg;
  yl_status operator()(yl_status s, const char* text) const { *msg = text; return s; }
};

// One layer of `d` against the geometry and slots in `p`; fills L (geometry, head anchor, which optional images it gets) and
// raises p.se_unit / p.wino_max_hw.  head_seen: head layers met so far, per level.
yl_status check_layer(const yl_model_desc* d, YlProgram& p, int i, std::vector<int>& head_seen, YlLayerInfo& L, Verdict fail) {
  const yl_layer& l = d->layers[i];
  const std::vector<YlSlotDim>& slots = p.slot_dims;
  L.d = l;
  char msg[256];
  auto bad = [&](const char* what) {
    snprintf(msg, sizeof(msg), "layer %d: %s", i, what);
    return fail(YL_ERR_INVALID, msg);
  };
  if (l.op < YL_OP_STEM || l.op > YL_OP_NHWC4) return bad("unknown op");
  if (l.reserved0 != 0) return bad("reserved0 must be 0");
  if (l.act < YL_ACT_NONE || l.act > YL_ACT_RELU_LAB || l.dw_act < 0 || l.dw_act > YL_ACT_SILU || l.act2 < 0 || l.act2 > YL_ACT_SILU ||
      l.act3 < 0 || l.act3 > YL_ACT_SILU)
    return bad("unknown activation (GELU / ReLU+affine are valid as `act` only)");
  if (YL_ACT_POSTPASS(l.act) && ((l.op != YL_OP_STEM && l.op != YL_OP_CONV && l.op != YL_OP_DW) || l.head_level >= 0 || l.up_slot >= 0 ||
                                 l.c2 > 0 || l.c3 > 0 || (l.cout & 3)))
    return bad("GELU / ReLU + learnable affine: plain STEM / CONV / DW layers with cout % 4 == 0 only");
  if (l.out_ch_off != 0 && l.op != YL_OP_COPY) return bad("out_ch_off is a YL_OP_COPY field");
  if (l.op >= YL_OP_POOL) {
    // element-wise / reduction ops (ABI v5): in_slot -> out_slot, no conv fields
    if (l.out_slot < 0 || l.out_slot >= d->num_slots) return bad("bad out_slot");
    if (l.op != YL_OP_NHWC4 && (l.in_slot < 0 || l.in_slot >= d->num_slots)) return bad("bad in_slot");
    if (l.res_slot >= 0 || l.up_slot >= 0 || l.scale_slot >= 0 || l.head_level >= 0 || l.dw_k || l.c2 || l.c3 || l.in_shift || l.act)
      return bad("element-wise op: plain layer fields only");
    const YlSlotDim& so = slots[l.out_slot];
    if (l.op == YL_OP_NHWC4) {
      if (so.h != d->img_size || so.w != d->img_size || so.c != 4 || l.cout != 4) return bad("NHWC4: out_slot must be [S,S,4]");
      L.in_h = L.in_w = d->img_size; L.out_h = L.out_w = d->img_size;
    } else {
      const YlSlotDim& si = slots[l.in_slot];
      if (si.c != l.cin || (l.cin & 3)) return bad("cin does not match the input slot / not a multiple of 4");
      L.in_h = si.h; L.in_w = si.w; L.out_h = so.h; L.out_w = so.w;
      if (l.op == YL_OP_POOL) {
        if (l.k < 1 || l.stride < 1 || l.cout != l.cin || so.c != l.cin || l.pad_t < 0 || l.pad_l < 0 || l.pad_t >= l.k || l.pad_l >= l.k ||
            (so.h - 1) * l.stride - l.pad_t >= si.h || (so.w - 1) * l.stride - l.pad_l >= si.w)
          return bad("pool: bad geometry");
      } else if (l.op == YL_OP_COPY) {
        if (so.h != si.h || so.w != si.w || l.out_ch_off < 0 || (l.out_ch_off & 3) || l.out_ch_off + l.cin > so.c)
          return bad("copy: channel slice outside the output slot");
      } else if (l.op == YL_OP_LN) {
        if (so.h != si.h || so.w != si.w || so.c != l.cin || l.cout != l.cin || !l.w || !l.b || !(l.eps > 0.0f)) return bad("layer norm: needs w, b [cin], eps > 0, same shape out");
      } else {     // GRN
        if (so.h != 1 || so.w != 1 || so.c != l.cin || !l.w || !(l.eps > 0.0f) || l.cin > 16384) return bad("GRN: out_slot must be [1,1,cin], needs w [cin], eps > 0");
        const size_t unit = (size_t)64 * l.cin;
        if (unit > p.se_unit) p.se_unit = unit;
        L.out_h = L.out_w = 1;
      }
    }
    return YL_OK;
  }
  if (!l.w) return bad("weights are NULL");
  if (l.k < 1 || l.stride < 1) return bad("bad kernel geometry");
  if (l.op == YL_OP_SE) {
    // squeeze-excite gate: in_slot [H,W,cin] -> out_slot [1,1,cin]; w/b = conv_reduce [cout][cin], w2/b2 = conv_expand [cin][cout]
    if (l.in_slot < 0 || l.in_slot >= d->num_slots || l.out_slot < 0 || l.out_slot >= d->num_slots) return bad("bad slot");
    const YlSlotDim& si = slots[l.in_slot]; const YlSlotDim& so = slots[l.out_slot];
    if (si.c != l.cin || so.c != l.cin || so.h != 1 || so.w != 1) return bad("squeeze-excite: out_slot must be [1,1,cin]");
    if (!l.w2 || !l.b || !l.b2 || l.c2 != l.cin || l.cout < 1 || l.cout > 256 || l.cin > 4096 || (l.cin & 3))
      return bad("squeeze-excite: needs w [cout][cin], b, w2 [cin][cout], b2, c2 == cin, cout <= 256, cin % 4 == 0 and <= 4096");
    if (l.k != 1 || l.stride != 1 || l.dw_k || l.c3 || l.res_slot >= 0 || l.up_slot >= 0 || l.scale_slot >= 0 || l.head_level >= 0 ||
        l.in_shift)
      return bad("squeeze-excite: plain layer fields only");
    L.in_h = si.h; L.in_w = si.w; L.out_h = L.out_w = 1;
    // scratch: partial sums of the stand-alone pool pass, or of the depthwise launch that produces the tensor (<= 64 each)
    const size_t unit = (size_t)64 * l.cin;
    if (unit > p.se_unit) p.se_unit = unit;
    return YL_OK;
  }
  if (l.scale_slot >= 0) {
    if (l.scale_slot >= d->num_slots || l.op != YL_OP_CONV || l.k != 1 || l.stride != 1 || l.dw_k || l.c2 || l.c3 || l.in_shift)
      return bad("scale_slot needs a plain 1x1 stride-1 conv");
    const YlSlotDim& g = slots[l.scale_slot];
    if (g.h != 1 || g.w != 1 || g.c != l.cin) return bad("scale_slot must be [1,1,cin]");
  }
  if (l.op == YL_OP_STEMBLOCK) {
    L.in_h = L.in_w = d->img_size;
    if (l.cin != 3 || l.k != 3) return fail(YL_ERR_UNSUPPORTED, "stem must be 3x3 with 3 input channels");
    if (!l.w2 || l.c2 < 1 || l.c3 < 0 || (l.c3 > 0 && !l.w3)) return bad("stem block needs w2 (and w3 when c3 > 0)");
    if (YL_SMOOTH(l.act) || YL_SMOOTH(l.act2) || YL_SMOOTH(l.act3))
      return fail(YL_ERR_UNSUPPORTED, "stem block: ReLU-family activations only");
    if (l.dw_k == 3) {       // second conv DEPTHWISE 3x3 stride 1 pad 1, then the 1x1: the EfficientNet-Lite entry (yl_stemdw_kernel)
      if (l.cout != 32 || l.c2 != 32 || l.c3 < 4 || l.c3 > 32 || (l.c3 & 3) || !l.w3 || l.dw_stride != 1 || l.dw_pad_t != 1 || l.dw_pad_l != 1)
        return fail(YL_ERR_UNSUPPORTED, "stem block with a depthwise second conv: 3 -> 32 -> dw3x3 s1 pad 1 -> 1x1 (4..32 outputs)");
    } else if (l.dw_k != 0) {
      return fail(YL_ERR_UNSUPPORTED, "stem block: dw_k must be 0 (dense 3x3 s2 second conv) or 3 (depthwise 3x3 s1)");
    } else if (!yl_stemblock_supported(l.cout, l.c2, l.c3))
      return fail(YL_ERR_UNSUPPORTED, "stem block: c1 in {16,32}, c2,c3 <= 32 and multiples of 4");
  } else if (l.op == YL_OP_STEM) {
    L.in_h = L.in_w = d->img_size;
    if (l.cin != 3 || l.k != 3) return fail(YL_ERR_UNSUPPORTED, "stem must be 3x3 with 3 input channels");
    if (l.cout != 16 && l.cout != 32) return fail(YL_ERR_UNSUPPORTED, "stem cout must be 16 or 32");
  } else {
    if (l.in_slot < 0 || l.in_slot >= d->num_slots) return bad("bad in_slot");
    L.in_h = slots[l.in_slot].h; L.in_w = slots[l.in_slot].w;
    if (l.in_shift != 0) {
      if (l.op != YL_OP_CONV || l.k < 2 || l.dw_k != 0 || l.in_shift < 0 || l.in_shift > 3)
        return bad("in_shift needs a kxk (k>1) conv without depthwise prologue");
      L.in_h <<= l.in_shift; L.in_w <<= l.in_shift;          // dims of the virtually upsampled input
    }
    const bool uib = (l.op == YL_OP_CONV && l.c2 > 0);
    if (slots[l.in_slot].c != (uib ? l.c2 : l.cin)) return bad("cin does not match the input slot");
    if (uib) {
      if (!l.w2 || l.dw_k == 0 || l.dw_stride < 1 || l.k != 1 || l.head_level >= 0)
        return bad("fused expand->depthwise->project block: needs w2, a depthwise prologue, 1x1 projection");
      // workgroup-level halo kernel (yl_ir_kernel: stride 1 / 2, TF-SAME pads) or the per-wave one (yl_uib_kernel)
      const bool ir = l.out_slot >= 0 && l.out_slot < d->num_slots &&
                      yl_ir_supported(l.c2, l.cin, l.cout, l.dw_k, l.dw_stride, slots[l.out_slot].h, slots[l.out_slot].w);
      if (!ir) {
        if (l.up_slot >= 0) return fail(YL_ERR_UNSUPPORTED, "fused block with an upsample-add: shape not instantiated");
        if (l.dw_stride != 1) return fail(YL_ERR_UNSUPPORTED, "fused inverted-residual block: stride-2 shape not instantiated");
        if (!yl_uib_supported(l.c2, l.cin, l.cout, l.dw_k))
          return fail(YL_ERR_UNSUPPORTED, "fused inverted-residual block: shape not instantiated / LDS budget exceeded");
        if ((slots[l.in_slot].h & 3) || (slots[l.in_slot].w & 3))
          return fail(YL_ERR_UNSUPPORTED, "fused inverted-residual block needs H,W multiples of 4");
      }
    }
  }
  // output geometry.  Sizes are declared by the host (slot / level dims); pad_t/pad_l are explicit
  // and the bottom/right padding is implied, so only reachability is checked here.
  if (l.op == YL_OP_CONV && l.dw_k > 0) {
    if (l.k != 1 || l.stride != 1) return fail(YL_ERR_UNSUPPORTED, "dw prologue needs a 1x1 stride-1 main conv");
    if (!l.dw_w) return bad("dw prologue weights are NULL");
    if (l.dw_stride < 1) return bad("bad dw_stride");
    if ((size_t)(l.dw_k * l.dw_k + 1) * l.cin * sizeof(float) > YL_DW_LDS_MAX) {
      // beyond the tap image of the generic depthwise-prologue kernels: only the streamed-tap kernel (yl_conv_dws_kernel) runs it
      const bool dws = l.out_slot >= 0 && l.out_slot < d->num_slots && l.c2 == 0 && l.c3 == 0 && l.scale_slot < 0 && l.head_level < 0 &&
                       yl_dws_supported(l.cin, l.cout, l.dw_k, l.dw_stride, slots[l.out_slot].h, slots[l.out_slot].w);
      if (!dws)
        return fail(YL_ERR_UNSUPPORTED, "dw prologue: taps+bias of all input channels must fit 32 KiB of LDS (or the layer must "
                                        "be one yl_query_dw_prologue reports as 2)");
    }
  }
  if (l.head_level >= 0) {
    if (l.op != YL_OP_CONV || l.head_level >= p.L) return bad("bad head_level");
    L.out_h = L.out_w = p.level_S[l.head_level];
    if (l.cout != p.E) return bad("head layers must have cout = 5+C+NM (one layer per anchor)");
    L.head_anchor = head_seen[l.head_level]++;
    if (L.head_anchor >= p.level_A[l.head_level]) return bad("more head layers than anchors for this level");
    if (l.res_slot >= 0 || l.up_slot >= 0) return bad("head layers take no residual/upsample input");
  } else {
    if (l.out_slot < 0 || l.out_slot >= d->num_slots) return bad("bad out_slot");
    L.out_h = slots[l.out_slot].h; L.out_w = slots[l.out_slot].w;
    const int oc = (l.op == YL_OP_STEMBLOCK) ? (l.c3 > 0 ? l.c3 : l.c2) : ((l.op == YL_OP_CONV && l.c3 > 0) ? l.c3 : l.cout);
    if (slots[l.out_slot].c != oc) return bad("cout does not match the output slot");
  }
  if (l.op == YL_OP_STEMBLOCK) {
    const int sh = (L.in_h + 2 * 0 + l.pad_t + (l.k - 1 - l.pad_t) - l.k) / l.stride + 1;   // symmetric / SAME stem
    if (L.out_h != (l.dw_k == 3 ? sh : (sh + 2 - 3) / 2 + 1) || L.out_w != L.out_h) return bad("stem block output size mismatch");
  } else {
    const bool pro = (l.op == YL_OP_CONV && l.dw_k > 0);
    const int st = pro ? l.dw_stride : l.stride, pt = pro ? l.dw_pad_t : l.pad_t, pl = pro ? l.dw_pad_l : l.pad_l;
    const int kk = pro ? l.dw_k : l.k;
    // the last window must start inside the tensor
    if ((L.out_h - 1) * st - pt >= L.in_h || (L.out_w - 1) * st - pl >= L.in_w || pt >= kk || pl >= kk ||
        L.out_h < 1 || L.out_w < 1)
      return bad("output size inconsistent with stride/padding");
  }
  if (l.res_slot >= 0) {
    if (l.res_slot >= d->num_slots) return bad("bad res_slot");
    const YlSlotDim& r = slots[l.res_slot];
    if (r.h != L.out_h || r.w != L.out_w || r.c != l.cout) return bad("residual shape mismatch");
  }
  if (l.up_slot >= 0) {
    if (l.up_slot >= d->num_slots || l.op != YL_OP_CONV) return bad("bad up_slot");
    // (fused block: the addend joins the EXPANDED tensor, cin channels)
    if (slots[l.up_slot].c != ((l.op == YL_OP_CONV && l.c2 > 0) ? l.cin : l.cout)) return bad("upsample source channel mismatch");
  }
  if (l.op == YL_OP_DW && l.cin != l.cout) return bad("depthwise needs cin == cout");
  if (l.op != YL_OP_STEM && l.op != YL_OP_STEMBLOCK && (l.cin & 3)) return fail(YL_ERR_UNSUPPORTED, "cin must be a multiple of 4");
  if ((l.res_slot >= 0 || l.up_slot >= 0 || YL_SMOOTH(l.act)) && (l.cout & 3) && l.op == YL_OP_CONV)
    return fail(YL_ERR_UNSUPPORTED, "residual/upsample/SiLU epilogue needs cout % 4 == 0");
  if (l.op != YL_OP_CONV) return YL_OK;
  // the optional images of a conv layer, and the chained 1x1 [c3][cout][1][1] (its k-blocks are this conv's 16-wide n-tiles)
  L.wino = l.k == 3 && l.stride == 1 && l.dw_k == 0 && l.c2 == 0 && l.c3 == 0 && l.pad_t == 1 && l.pad_l == 1 && l.in_shift <= 1 &&
           l.cin >= 16 && l.cout >= 16 && (l.cout & 3) == 0 && l.head_level < 0 && l.up_slot < 0 &&
           L.out_h == L.in_h && L.out_w == L.in_w;   // the output grid IS the (virtual) input grid: yl_wino_form sizes its 32-bit offsets by it
  if (L.wino && l.cin >= 64 && l.cout >= 64 && L.out_h * L.out_w > p.wino_max_hw) p.wino_max_hw = L.out_h * L.out_w;
  L.split_head = l.head_level >= 0 && p.NM > 0 && (p.NM & 3) == 0 && l.k == 1 && l.dw_k == 0 && l.c2 == 0 && l.c3 == 0 &&
                 5 + p.C <= 96 && l.cout == p.E && p.level_A[l.head_level] == 1;
  if (l.c3 > 0 && (!l.w3 || l.k < 2 || l.dw_k > 0 || l.c2 > 0 || l.head_level >= 0 || l.res_slot >= 0 || l.up_slot >= 0 || l.in_shift ||
                   (l.cout & 3) || (l.c3 & 3) || l.c3 > 32 || l.cout > 96 || YL_SMOOTH(l.act) || YL_SMOOTH(l.act3)))
    return fail(YL_ERR_UNSUPPORTED, "chained 1x1 conv: needs a plain dense k x k conv (<= 96 channels out), c3 <= 32, ReLU-family activations");
  return YL_OK;
}

// "conv weights + padded bias": the weights in MFMA fragment order, the bias (may be null) zero-padded to whole 16-wide
// n-tiles plus `extra` floats
void pad_bias(const float* b, int cout, int extra, std::vector<float>& bias) {
  bias.assign((size_t)cdiv(cout, 16) * 16 + extra, 0.0f);
  if (b) memcpy(bias.data(), b, cout * sizeof(float));
}
void pack_conv_bias(const float* w, const float* b, int cout, int cin, int k, int extra, std::vector<float>& wp, std::vector<float>& bias) {
  pack_conv(w, cout, cin, k, wp);
  pad_bias(b, cout, extra, bias);
}

}  // namespace

yl_status yl_program_check_args(const yl_model_desc* d) {
  if (d->abi_version != YL_ABI_VERSION) return YL_ERR_INVALID;
  if (d->num_levels < 1 || d->num_levels > YL_MAX_LEVELS) return YL_ERR_INVALID;
  if (d->num_classes < 0 || d->num_classes > 4096) return YL_ERR_UNSUPPORTED;
  return YL_OK;
}

yl_status yl_program_validate(const yl_model_desc* d, YlProgram* out, std::string* msg) {
  msg->clear();
  const yl_status a = yl_program_check_args(d);
  if (a != YL_OK) return a;
  const Verdict fail{msg};
  YlProgram& p = *out;
  p = YlProgram();
  p.img_size = d->img_size; p.in_ch = d->in_channels; p.C = d->num_classes; p.L = d->num_levels;
  p.NM = d->num_masks; p.proto_slot = d->proto_slot;
  if (p.NM < 0 || p.NM > 64) return fail(YL_ERR_UNSUPPORTED, "num_masks must be in [0,64]");
  p.E = 5 + p.C + p.NM;
  int off = 0;
  for (int l = 0; l < p.L; ++l) {
    p.level_S[l] = d->level_size[l]; p.level_A[l] = d->level_anchors[l];
    if (p.level_S[l] < 1 || p.level_A[l] < 1) return fail(YL_ERR_INVALID, "bad level geometry");
    p.level_off[l] = off;
    off += p.level_A[l] * p.level_S[l] * p.level_S[l];
  }
  p.level_off[p.L] = off;
  p.N = off;
  if (p.N >= (1 << 20)) return fail(YL_ERR_UNSUPPORTED, "more than 2^20 candidates per image");
  if (d->num_layers == 0) return YL_OK;   // a post-processing-only model: no slots, no layers
  if (d->in_channels != 3) return fail(YL_ERR_UNSUPPORTED, "network input must have 3 channels");
  if (!d->layers || !d->slot_h || !d->slot_w || !d->slot_c) return fail(YL_ERR_INVALID, "null layer/slot arrays");
  p.slot_dims.resize(d->num_slots);
  for (int i = 0; i < d->num_slots; ++i) {
    YlSlotDim& s = p.slot_dims[i];
    s.h = d->slot_h[i]; s.w = d->slot_w[i]; s.c = d->slot_c[i];
    if (s.h < 1 || s.w < 1 || s.c < 1 || (s.c & 3)) return fail(YL_ERR_UNSUPPORTED, "slot channels must be a positive multiple of 4");
  }
  std::vector<int> head_seen(p.L, 0);
  for (int i = 0; i < d->num_layers; ++i) {
    YlLayerInfo L;
    const yl_status s = check_layer(d, p, i, head_seen, L, fail);
    if (s != YL_OK) return s;
    p.layers.push_back(L);
  }
  for (int l = 0; l < p.L; ++l)
    if (head_seen[l] != p.level_A[l]) return fail(YL_ERR_INVALID, "every level needs one head layer per anchor");
  if (p.NM > 0) {
    if (p.proto_slot < 0 || p.proto_slot >= d->num_slots || p.slot_dims[p.proto_slot].c != p.NM)
      return fail(YL_ERR_INVALID, "num_masks > 0 needs proto_slot with num_masks channels");
  }
  return YL_OK;
}

void yl_program_pack(const YlProgram& p, size_t i, YlLayerImages* im) {
  const YlLayerInfo& L = p.layers[i];
  const yl_layer& l = L.d;
  *im = YlLayerImages();
  if (l.op == YL_OP_LN || l.op == YL_OP_GRN) {
    im->wp.assign(l.w, l.w + l.cin);
    if (l.op == YL_OP_LN) im->bias.assign(l.b, l.b + l.cin);
  } else if (l.op == YL_OP_SE) {
    im->wp.assign(l.w, l.w + (size_t)l.cout * l.cin);
    im->bias.assign(l.b, l.b + l.cout);
    im->w2p.resize((size_t)l.cin * l.cout);
    for (int cc = 0; cc < l.cin; ++cc)                       // conv_expand [cin][cout] -> [cout][cin]
      for (int j = 0; j < l.cout; ++j) im->w2p[(size_t)j * l.cin + cc] = l.w2[(size_t)cc * l.cout + j];
    im->b2.assign(l.b2, l.b2 + l.cin);
  } else if (l.op == YL_OP_STEM || l.op == YL_OP_STEMBLOCK) {
    if (l.op == YL_OP_STEMBLOCK) pack_stem_rows(l.w, l.b, l.cout, im->wp);
    else pack_stem(l.w, l.cout, l.cin, l.k, im->wp);
    im->bias.assign(l.cout, 0.0f);
    if (l.b) memcpy(im->bias.data(), l.b, l.cout * sizeof(float));
    if (l.op == YL_OP_STEMBLOCK) {
      if (l.dw_k == 3) {                                            // depthwise taps [c][1][3][3] -> tap-major [9][c]
        pack_dw(l.w2, l.c2, 3, im->w2p);
        pad_bias(l.b2, l.c2, 0, im->b2);
      } else
        pack_conv_bias(l.w2, l.b2, l.c2, l.cout, 3, 0, im->w2p, im->b2);
      // the 1x1 conv's k-blocks are the second conv's 16-wide n-tiles: pack with cin padded to that
      if (l.c3 > 0) pack_conv_bias(l.w3, l.b3, l.c3, l.c2, 1, 0, im->w3p, im->b3);
    }
  } else if (l.op == YL_OP_CONV) {
    pack_conv_bias(l.w, l.b, l.cout, l.cin, l.k, 128, im->wp, im->bias);
    if (L.wino) pack_wino(l.w, l.cout, l.cin, im->wino);
    if (L.split_head) {
      const int nd = 5 + p.C;
      pack_conv_bias(l.w, l.b, nd, l.cin, 1, 128, im->wp_det, im->b_det);
      pack_conv_bias(l.w + (size_t)nd * l.cin, l.b ? l.b + nd : nullptr, p.NM, l.cin, 1, 128, im->wp_mc, im->b_mc);
    }
    if (l.c3 > 0) pack_conv_bias(l.w3, l.b3, l.c3, l.cout, 1, 0, im->w3p, im->b3);   // chained 1x1
    if (l.c2 > 0) pack_conv_bias(l.w2, l.b2, l.cin, l.c2, 1, 0, im->w2p, im->b2);    // expansion conv of a fused block: [cin][c2][1][1]
    if (l.dw_k > 0) {
      pack_dw(l.dw_w, l.cin, l.dw_k, im->dw_w);
      if (l.dw_b) im->dw_b.assign(l.dw_b, l.dw_b + l.cin);
    }
  } else if (l.op == YL_OP_DW) {
    pack_dw(l.w, l.cout, l.k, im->wp);
    if (l.b) im->bias.assign(l.b, l.b + l.cout);
  }
}

namespace {

// the longest run of consecutive layers whose input AND output grids are <= 1/16 of the image (the 40x40 / 20x20
// stages of the backbone and the coarse part of the top-down pass): the part of the network that is chunked over
// the internal streams by the hybrid plan
void assign_small_run(const YlProgram& p, YlTables& t) {
  const int lim = p.img_size / 16;
  int best_lo = 0, best_hi = 0, lo = -1;
  const int n = (int)p.layers.size();
  for (int i = 0; i <= n; ++i) {
    const bool small = i < n && p.layers[i].d.op == YL_OP_CONV && p.layers[i].in_h <= lim && p.layers[i].out_h <= lim &&
                       p.layers[i].d.head_level < 0;
    if (small && lo < 0) lo = i;
    if (!small && lo >= 0) {
      if (i - lo > best_hi - best_lo) { best_lo = lo; best_hi = i; }
      lo = -1;
    }
  }
  t.small_lo = best_lo; t.small_hi = best_hi;
  const int lim2 = p.img_size / 32;
  best_lo = best_hi = 0; lo = -1;
  for (int i = 0; i <= n; ++i) {
    const bool small = i < n && (p.layers[i].d.op == YL_OP_CONV || p.layers[i].d.op == YL_OP_DW || p.layers[i].d.op == YL_OP_SE) &&
                       p.layers[i].in_h <= lim2 && p.layers[i].out_h <= lim2 && p.layers[i].d.head_level < 0;
    if (small && lo < 0) lo = i;
    if (!small && lo >= 0) {
      if (i - lo > best_hi - best_lo) { best_lo = lo; best_hi = i; }
      lo = -1;
    }
  }
  t.tiny_lo = best_lo; t.tiny_hi = best_hi;
}

// readers[s]: layer operands that read slot s -- the input (the stem-type ops read the caller's image instead), the
// residual and the upsampled operand (not scale_slot: gates are written by YL_OP_SE, never by a layer a fused step swallows)
void count_readers(const YlProgram& p, YlTables& t) {
  t.readers.assign(p.slot_dims.size(), 0);
  for (const YlLayerInfo& L : p.layers)
    for (int s : {(L.d.op == YL_OP_STEM || L.d.op == YL_OP_STEMBLOCK) ? -1 : L.d.in_slot, L.d.res_slot, L.d.up_slot})
      if (s >= 0 && (size_t)s < t.readers.size()) ++t.readers[s];   // (YL_OP_NHWC4's in_slot is not validated: unused)
}

// lane assignment from the slot graph: a layer goes to lane 1 iff everything it feeds ends in head outputs of
// levels >= 1 only (the finest level's chain, the backbone, the top-down laterals and the prototype branch stay
// on lane 0)
void assign_lanes(const YlProgram& p, YlTables& t) {
  const size_t n = p.layers.size();
  t.lane.assign(n, 0);
  std::vector<unsigned> reach(n, 0u);
  for (size_t ii = n; ii-- > 0;) {
    const yl_layer& d = p.layers[ii].d;
    unsigned r = 0;
    if (d.head_level >= 0) r |= 1u << (d.head_level > 30 ? 30 : d.head_level);
    if (d.out_slot >= 0 && d.out_slot == p.proto_slot) r |= 1u << 31;
    if (d.head_level < 0 && d.out_slot >= 0)
      for (size_t j = ii + 1; j < n; ++j) {
        const yl_layer& e = p.layers[j].d;
        if (e.in_slot == d.out_slot || e.res_slot == d.out_slot || e.up_slot == d.out_slot || e.scale_slot == d.out_slot) r |= reach[j];
      }
    reach[ii] = r;
  }
  bool any = false;
  for (size_t i = 0; i < n; ++i) {
    t.lane[i] = (reach[i] != 0 && (reach[i] & 1u) == 0 && (reach[i] >> 31) == 0) ? 1 : 0;
    any |= t.lane[i] != 0;
  }
  if (!any) t.lane.clear();
}

}  // namespace

YlTables yl_program_tables(const YlProgram& p) {
  YlTables t;
  assign_lanes(p, t);
  assign_small_run(p, t);
  count_readers(p, t);
  return t;
}
