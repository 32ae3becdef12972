// Precision mode of a translation unit and the symbol suffix of the reduced-precision builds of the conv units (csrc/build.py
// compiles yl_conv.hip, yl_convc.hip and yl_stemblock.hip four times: fp32, -DYL_BF16=1 (bf16 operands), -DYL_BF16=1 -DYL_F16=1
// (fp16 operands) and -DYL_BF16=1 -DYL_F16=1 -DYL_F16S=1 (fp16 operands and fp16 activation tensors)).  A unit that a build
// line gives no mode macro is the fp32 one: all three are 0.
#pragma once
#ifndef YL_BF16
#define YL_BF16 0
#endif
#ifndef YL_F16
#define YL_F16 0
#endif
#ifndef YL_F16S
#define YL_F16S 0
#endif
#if YL_F16S
#define YL_LP_NAME(n) n##_f16s      /* fourth compilation: fp16 operands AND fp16 activation tensors in HBM */
#elif YL_F16
#define YL_LP_NAME(n) n##_f16
#else
#define YL_LP_NAME(n) n##_bf16
#endif
