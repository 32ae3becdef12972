// Layer properties the kernels, the executor and the host-side program validation (yl_program.cpp) agree on: the activation
// classes, and the shape predicates of the fused kernels ("is this layer one the kernel is instantiated for"), which are
// defined next to those kernels (yl_conv.hip, yl_convc.hip, yl_stemblock.hip).
// Also the one launch-form decision that a query of the C ABI reports: which Winograd kernel form runs a layer (yl_wino_form).
// Plain C++: no HIP header, so host-only code can include it (and links against the library for the predicates).
#pragma once

// activations that are not a clamp: SiLU runs in the conv kernels' generic epilogue (the fast clamp epilogues refuse it);
// GELU and ReLU + learnable affine (ABI v5: YL_ACT_POSTPASS) never reach a conv kernel -- the executor launches the layer with
// no activation (and no residual) and applies them in an element-wise pass over the output (yl_ops.hip: yl_act_kernel), so the
// hot kernels carry no code for them
#define YL_SMOOTH(a) ((a) >= YL_ACT_SILU)
#define YL_ACT_POSTPASS(a) ((a) >= YL_ACT_GELU)

#include <stddef.h>

#define YL_NUM_CU 256          // MI355X: 8 XCDs x 32 CUs

bool yl_stemblock_supported(int c1, int c2, int c3);
bool yl_uib_supported(int c1, int cmid, int n, int dk);
bool yl_ir_supported(int c1, int cmid, int n, int dk, int ds, int oh, int ow);
// which form of yl_ir_kernel runs a block yl_ir_supported accepts (0: none, 1: first, 2: second -- clamp-type activations, 32-bit
// offsets) and, in shape[7] if given, the instantiation; h x w input, uh x uw FPN addend (0: none).  fp32 tensors.
int yl_ir_form(int c1, int cmid, int n, int dk, int ds, int oh, int ow, int batch, int h, int w, int uh, int uw, int act,
               int dw_act, int act2, int* shape);
bool yl_dws_supported(int cin, int n, int dk, int ds, int oh, int ow);

// ---- Winograd F(2x2,3x3): which kernel form runs a dense 3x3 stride-1 pad-1 layer (yl_convc.hip) ----
// yl_conv_wino2_kernel<MT, NT, SH> is instantiated for these (m-tiles, n-tiles per item), each for a plain and a 2x upsampled
// input (in_shift)
#define YL_WINO2_SHAPES(X) X(4, 3) X(4, 4) X(2, 3) X(2, 4) X(2, 7)

struct YlWinoForm {
  int form;      // 0: not a Winograd shape, 1: yl_conv_wino_kernel (first form), 2: yl_conv_wino2_kernel<mt, nt>
  int mt, nt;    // form 2 only
};

// The one decision of yl_launch_conv_wino and yl_query_wino_form.  cin / n channels, oh x ow output (= the virtual input grid),
// elem: bytes per stored activation, v1: "dev_select" bit 11 (keep the first form), shape: "dev_select" bits 12-13 (0 auto,
// 1 (4,4), 2 (2,7), 3 two m-tiles).
inline YlWinoForm yl_wino_form(int cin, int n, int oh, int ow, int batch, int in_shift, size_t elem, bool v1, unsigned shape) {
  if (cin < 1 || n < 1 || oh < 1 || ow < 1 || batch < 1 || (n & 3) || in_shift < 0 || in_shift > 1 ||
      ((size_t)batch * (oh >> in_shift) * (ow >> in_shift) * cin + (size_t)(ow + 1) * cin) * elem >= ((size_t)1 << 31))
    return {0, 0, 0};                                       // (32-bit byte offsets: both forms read through buffer descriptors)
  const int KB = (cin + 15) / 16, NTtot = (n + 15) / 16;
  // second form (positions across the waves): K loops long enough to amortise the accumulator exchange, grids that fill
  // the 4 x 4-tile m-tiles; "dev_select" bit 11 keeps the first form (bitwise A/B), bits 12-13 pick a shape (A/B runs)
  // (second form: 32-bit byte offsets into the input tensor and the U image)
  const bool small = (size_t)batch * (oh >> in_shift) * (ow >> in_shift) * cin * elem < ((size_t)1 << 31) &&
                     (size_t)((NTtot + 1) / 2) * KB * 32768 < ((size_t)1 << 31);
  if (!v1 && KB >= 2 && NTtot >= 3 && small) {              // (KB >= 2: the peeled last two blocks)
    const int TW = (ow + 1) >> 1, TH = (oh + 1) >> 1;
    const int MX = (TW + 3) >> 2, MY = (TH + 3) >> 2;
    const long MTOT = (long)batch * MX * MY;
    if ((long)TW * TH * 100 >= (long)MX * MY * 16 * 65) {   // >= 65 % of the m-tiles' Winograd tiles exist (20 x 20: 69 %, 0.232 -> 0.205 ms)
      const int pad3 = (NTtot + 2) / 3 * 3, pad4 = (NTtot + 3) / 4 * 4;
      int nt = pad3 <= pad4 ? 3 : 4;
      // 4 m-tiles halve the U bytes per MFMA (80 x 80: 1.79 against 1.95 ms) when there are >= 3 items per CU; with 4
      // n-tiles that shape spills (2 x 4 x 4 accumulator quads + two U register sets)
      int mt = nt == 3 && (MTOT / 4) * ((NTtot + nt - 1) / nt) >= 3 * YL_NUM_CU ? 4 : 2;
      if (shape == 1) { mt = 4; nt = 4; } else if (shape == 2) { mt = 2; nt = 7; } else if (shape == 3) { mt = 2; }
#define YL_WINO2_HAS(A, B) if (mt == A && nt == B) return {2, mt, nt};
      YL_WINO2_SHAPES(YL_WINO2_HAS)
#undef YL_WINO2_HAS
    }
  }
  return {1, 0, 0};
}
