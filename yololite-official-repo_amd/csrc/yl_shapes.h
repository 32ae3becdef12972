// Layer properties the kernels, the executor and the host-side program validation (yl_program.cpp) agree on: the activation
// classes, and the shape predicates of the fused kernels ("is this layer one the kernel is instantiated for"), which are
// defined next to those kernels (yl_conv.hip, yl_convc.hip, yl_stemblock.hip).
// Plain C++: no HIP header, so host-only code can include it (and links against the library for the predicates).
#pragma once

// activations that are not a clamp: SiLU runs in the conv kernels' generic epilogue (the fast clamp epilogues refuse it);
// GELU and ReLU + learnable affine (ABI v5: YL_ACT_POSTPASS) never reach a conv kernel -- the executor launches the layer with
// no activation (and no residual) and applies them in an element-wise pass over the output (yl_ops.hip: yl_act_kernel), so the
// hot kernels carry no code for them
#define YL_SMOOTH(a) ((a) >= YL_ACT_SILU)
#define YL_ACT_POSTPASS(a) ((a) >= YL_ACT_GELU)

bool yl_stemblock_supported(int c1, int c2, int c3);
bool yl_uib_supported(int c1, int cmid, int n, int dk);
bool yl_ir_supported(int c1, int cmid, int n, int dk, int ds, int oh, int ow);
bool yl_dws_supported(int cin, int n, int dk, int ds, int oh, int ow);
