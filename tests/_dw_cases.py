"""The depthwise k x k -> 1x1 layer cases (and the stand-alone depthwise ones): shapes, one-layer programs, the float64
reference, the fp32 yardstick and the bar.

A case is ONE yl_layer: `conv` -- a 1x1 conv c_in -> c_out with a depthwise k x k prologue (dw_k > 0: depthwise conv, bias,
activation, then the 1x1 conv, bias, activation, optional residual AFTER the activation) -- or `dw`, a stand-alone YL_OP_DW
layer (depthwise conv, bias, activation, optional residual), on a square G x G output grid.  tests/test_dw_layer_cpu.py holds
the yardstick and the bar to what they must be able to tell apart and takes the censuses; tests/test_dw_layer_gpu.py runs
every case under every form on the device and holds the layer's output to the float64 reference.

Which kernel a (case, form) runs is what the library says: `yl_query_dw_form`, host code built on the functions the
launchers themselves decide by (csrc/yl_conv.hip: yl_dw_form, yl_dw_alone_form; csrc/yl_convc.hip: yl_dwk_form, yl_dws_form,
yl_dwt_form, yl_dwc_form) -- nothing of the selection rules is written again here.  A form is a (tile_m, dev_select, split_k)
setting; a case runs under the default and under every candidate setting (CANDIDATES) for which the query names a family or
an instantiation it has not named for the case before.

Reference: torch conv2d in float64 on the CPU, groups = c_in, explicit zero padding -- (pad_t, pad_l) on the leading edges,
what the output size needs on the trailing ones -- bias, activation; then the 1x1 conv2d, bias, activation, residual.
Yardstick: the same calls in float32.  It restates the OPERATION, not a kernel's lane layout or summation order.
Bar: _train_cases.bar -- max(4 x the yardstick's own max-abs error against float64, 2 fp32 ulps at max |f64|), per case over
the whole output tensor.

Classes (the census of the zoo).  The class of a layer at a batch is ONE tuple: the kernel the query names under the default
options (family and template arguments; for yl_conv_mfma_kernel also whether the 1x1 weights stream in chunks), and
    KB       k-blocks of 16 depthwise channels: 1 | 2 | 3 | even (>= 4) | odd (>= 5)
    tail     c_in % 16 != 0: the last k-block has a channel tail
             (stand-alone depthwise: one | several 256-channel blocks of a workgroup, and c_in % 256 != 0)
    n-tile   c_out % 16 != 0: the last n-tile is partial
    grid     whole | partial units of the kernel's work split: 4 x 4-pixel tiles (dwt, dwh, dws, dwc: always whole), 8 x 8
             windows (dwl), 64-pixel items per image (dwk, mfma), 2 x 4-pixel blocks (dw_tile); `-` for yl_dw_kernel
    stride   1 | 2
    pad      sym (k // 2 on every edge) | tf<lead> (TensorFlow SAME: the leading pad, trailing what the size needs)
    acts     the activations the KERNEL applies on the depthwise and on the 1x1 site (GELU / ReLU + affine run in a pass of
             their own: the kernel sees none)
    res      residual in the epilogue
taken together.  A case's class is the one it has under the default options."""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from _train_cases import bar  # noqa: F401  (the project's rule; used by both test files)

ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SILU = 0, 1, 2, 3
ACT_NAME = {ACT_NONE: "none", ACT_RELU: "relu", ACT_RELU6: "relu6", ACT_SILU: "silu"}
OP_CONV, OP_DW = 1, 2                                   # YL_OP_CONV, YL_OP_DW (asserted against _lib in the CPU test)
FAMILY = {0: None, 1: "dwk", 2: "dwl", 3: "dws", 4: "dwt", 5: "dwt_splitk", 6: "dwc", 7: "dwh", 8: "mfma", 9: "dw_tile", 10: "dw"}
DWK, DWL, DWS, DWT, DWT_SPLITK, DWC, DWH, MFMA, DW_TILE, DW = range(1, 11)
CM_DWPRO, CM_DW3, CM_DW5 = 2, 3, 5                      # yl_conv_mfma_kernel's depthwise-prologue modes (csrc/yl_conv.hip)

# the layer's neighbours stay plain launches under every form: no 1x1 pair, no chained projection (dev_select bits 21, 19)
DEV_BASE = (1 << 21) | (1 << 19)
# (name, tile_m, dev_select bits, split_k): the settings a case is tried under; it RUNS under those that make the query name
# something new for it (forms())
CANDIDATES = (
    ("default", 0, 0, 0),
    ("dwt_off", 0, 1 << 4, 0),             # yl_conv_dwt_kernel off -> yl_conv_dwh_kernel
    ("split_k", 0, 0, 1),                  # the split-K form of yl_conv_dwt_kernel where the shape has one
    ("dwk_group", 0, 1 << 5, 0),           # yl_conv_dwk_kernel: one n-group per item
    ("dwk_off", 0, 2 << 5, 0),             # yl_conv_dwk_kernel off -> yl_conv_dws_kernel or the generic kernel's mode
    ("dwl_off", 0, 1 << 14, 0),            # the window-in-LDS kernel off -> yl_conv_dwk_kernel
    ("dwl_all", 0, 1 << 15, 0),            # the window-in-LDS kernel on every grid
    ("dwc", 7, 1 << 3, 0),                 # the producer / consumer kernel on every shape it supports
    ("tile6", 6, 0, 0),                    # yl_conv_dwh_kernel
    ("tile3", 3, 0, 0),                    # yl_conv_mfma_kernel's depthwise-prologue modes
    ("dw_tile_off", 0, 1 << 0, 0),         # stand-alone depthwise: yl_dw_kernel
)
# families documented as bit-identical to one another (csrc/yl_convc.hip: the kernels' header comments): same tap order, the
# 1x1 sums its k-blocks in ascending order, same epilogues.  yl_conv_dwt_kernel's split-K form sums in another order and
# yl_conv_dws_kernel equals the TWO LAUNCHES (yl_dw_tile_kernel + a plain 1x1 kernel), which the device test runs as well
BITWISE_GROUPS = ((DWK, DWL), (DWT, DWH, DWC))


def _case(tag, G, B, cin, cout, k, s, dw_act, act, op="conv", pad="sym", res=False, odd_in=False):
    """pad: "sym" = k // 2, "tf" = TensorFlow SAME.  odd_in: stride 2 on an input of 2 G - 1 pixels (else s G)"""
    assert op in ("conv", "dw") and pad in ("sym", "tf") and (op == "conv" or cin == cout)
    return dict(tag=tag, G=G, B=B, cin=cin, cout=cout, k=k, s=s, dw_act=dw_act, act=act, op=op, pad=pad, res=res, odd_in=odd_in)


N_, R_, R6, SI = ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SILU
CASES = [
    # ---- yl_conv_dwt_kernel<NT, DK, DS, 1, WL, SK>: N <= 96, grids that are multiples of 4
    # NT 1 / 2 / 3 / 4 / 6; N = 20 and 36: partial last n-tiles.  Grid 4: one tile on all four borders; B = 3: the three tiles
    # of a launch share a workgroup's four waves.  WL (KB * NTtot <= 36) true and false
    _case("t_nt1", 4, 3, 32, 16, 3, 1, R_, N_),
    _case("t_nt2_n20", 4, 3, 24, 20, 3, 1, R6, R6, res=True),                 # cin 24: 8-channel tail
    _case("t_nt3_n36", 8, 1, 48, 36, 5, 1, SI, SI),
    _case("t_nt4_wl", 8, 2, 96, 64, 3, 2, R_, N_, res=True),                  # KB 6 x 4 = 24: weights from LDS; residual in front (no activation)
    _case("t_nt6_n96", 12, 1, 96, 96, 3, 1, R_, R_),                          # KB 6 x 6 = 36: the last WL shape; an interior tile
    _case("t_nt6_nowl", 8, 1, 112, 96, 5, 2, R6, N_),                         # KB 7 x 6 = 42: weights from L1/L2
    _case("t_nt3_nowl", 4, 3, 208, 48, 3, 1, N_, SI, res=True),               # KB 13 x 3 = 39
    _case("t_tf3", 8, 2, 48, 32, 3, 2, R6, N_, pad="tf"),                     # TF-SAME on an even input: leading pad 0
    _case("t_sym3", 8, 2, 48, 32, 3, 2, R6, N_),                              # ... against the symmetric pad on the same shape
    _case("t_tf5", 4, 2, 40, 24, 5, 2, R6, R6, pad="tf"),                     # leading pad 1; 8-channel tail, N = 24
    _case("t_sym5", 4, 2, 40, 24, 5, 2, R6, R6),
    _case("t_odd_in", 4, 2, 32, 32, 3, 2, R_, R_, odd_in=True),               # stride 2 on a 7 x 7 input
    # split-K (NT 4, weights from L1/L2, KB >= 8, grid <= 20 x 20): KB even / odd, a channel tail in the last k-block
    _case("sk_k12", 4, 3, 192, 64, 3, 1, R_, N_, res=True),
    _case("sk_k13_tail", 20, 2, 200, 64, 5, 1, R_, N_, res=True),
    _case("sk_k16", 4, 2, 256, 64, 5, 1, R_, N_, res=True),
    _case("sk_s2_k18", 4, 3, 288, 64, 3, 2, R_, N_),
    _case("sk_s2_k11_tail", 20, 1, 172, 52, 3, 2, SI, R6),                    # odd KB, 12-channel tail, N = 52
    _case("sk_none_5s2", 4, 2, 160, 64, 5, 2, R_, N_),                        # 5x5 stride 2 has no split-K instantiation: the plain form
    # ---- above yl_conv_dwh_kernel's / every tap image's limits
    _case("h_nt8", 4, 2, 64, 256, 5, 1, N_, R_),                              # 16 n-tiles: dwt refuses, dwh<8> on two n-chunks
    _case("h_nt8_k8", 20, 1, 128, 512, 5, 1, N_, R_),
    _case("h_over", 4, 2, 256, 128, 3, 2, R_, N_),                            # 128 KiB of 1x1 weights + taps + halos: above dwh's LDS limit -> the mfma mode
    # yl_conv_dwc_kernel<DK, DS, NTW> (tile_m 7): NTW 1 and 5 at kbmax_of(NTW) = 18 / 4 k-blocks and one above, which falls through
    _case("c_ntw1_over", 4, 2, 304, 64, 3, 1, R_, N_, res=True),
    _case("c_ntw5", 4, 2, 64, 320, 3, 1, R_, R_),
    _case("c_ntw5_over", 4, 2, 80, 320, 5, 1, R_, R_),
    # ---- yl_conv_mfma_kernel's depthwise-prologue modes: odd grids (partial 64-pixel m-tiles, tiles across images), N % 4 != 0
    _case("m_odd5", 5, 3, 96, 96, 3, 1, R_, R_),
    _case("m_odd7_n50", 7, 2, 96, 50, 3, 1, R6, N_),                          # N % 4 != 0: the staged stores
    _case("m_odd13_5", 13, 1, 40, 24, 5, 1, SI, SI, res=True),
    _case("m_odd5_s2tf", 5, 2, 48, 32, 3, 2, R6, N_, pad="tf"),               # 10 x 10 input, leading pad 0
    _case("m_k7", 8, 1, 64, 64, 7, 1, R_, R_),                                # a depthwise size that is neither 3 nor 5
    _case("m_stream", 5, 1, 512, 128, 3, 1, R_, N_, res=True),                # K beyond the resident chunk: weights stream
    _case("m_k10_512", 10, 1, 128, 512, 5, 1, N_, R_),
    # ---- yl_conv_dwk_kernel<NT, GW, 4> / yl_conv_dwl_kernel<NTT>: 3x3, KB >= 12, more than 8 n-tiles
    _case("k_21", 8, 1, 192, 328, 3, 1, R_, R_),                              # NTtot 21: GW 3 / 1; 8-channel n-tail
    _case("k_16_tail", 12, 1, 244, 244, 3, 1, R_, R_),                        # NTtot 16: GW 2 / 1; 4-channel tails; 144 pixels: partial items
    _case("k_14_s2", 8, 2, 200, 224, 3, 2, R6, N_),                           # the % 7 rule; KB 13, 8-channel tail; stride 2
    _case("k_24_odd7", 7, 2, 192, 384, 3, 1, SI, SI),                         # the % 8 rule on an odd grid
    _case("k_16_b3", 12, 3, 244, 244, 3, 1, R_, R_),                          # B = 3: an item's two windows straddle images
    _case("k_21_g20", 20, 1, 328, 328, 3, 1, R_, R_),                         # partial windows on 20 x 20
    _case("k_21_tf", 8, 2, 192, 336, 3, 2, R6, N_, pad="tf"),
    # the window-in-LDS kernel by DEFAULT dispatch: >= 3 x 256 windows of 8 x 8 pixels at >= 80 % fill -- the smallest batch
    _case("l_default", 8, 768, 192, 256, 3, 1, R_, R_),
    # ---- yl_conv_dws_kernel<NT, GW, DK, DS, 4>: KB >= 12, 7..22 n-tiles, each instantiated shape at c_in 192
    _case("s_8_5_1", 4, 2, 192, 112, 5, 1, R6, N_),                           # 7 n-tiles: just above the bucket floor
    _case("s_8_5_2", 4, 2, 192, 128, 5, 2, R6, N_, pad="tf"),                 # the bucket's top
    _case("s_13_5_1", 8, 1, 192, 144, 5, 1, R6, N_, res=True),                # 9 n-tiles
    _case("s_13_5_2", 4, 2, 192, 208, 5, 2, R6, N_),
    _case("s_8_3_1", 4, 2, 200, 120, 3, 1, R6, N_),                           # channel tail
    _case("s_13_3_1", 8, 1, 192, 208, 3, 1, SI, SI),
    _case("s_22_3_1", 4, 2, 192, 224, 3, 1, R6, N_),                          # 14 n-tiles on the (11, 2) shape (dwk off)
    _case("s_22_5_1", 4, 2, 192, 352, 5, 1, R6, N_, res=True),
    _case("s_taps", 4, 1, 320, 112, 5, 1, R6, N_),                            # 26 x 320 floats of taps: beyond the 32 KiB image
    # ---- stand-alone depthwise: yl_dw_tile_kernel<K, S> (blocks of 2 x 4 pixels, 256 channels) / yl_dw_kernel
    _case("d_3_1_g1", 1, 3, 4, 4, 3, 1, R_, R_, op="dw"),
    _case("d_3_2_g2", 2, 2, 36, 36, 3, 2, R6, R6, op="dw"),
    _case("d_5_1_g5", 5, 2, 260, 260, 5, 1, R_, R_, op="dw", res=True),      # a second channel block of 256
    _case("d_5_2_g8", 8, 1, 36, 36, 5, 2, SI, SI, op="dw", pad="tf"),
    _case("d_3_2_tf", 5, 2, 36, 36, 3, 2, SI, SI, op="dw", pad="tf"),
    _case("d_3_1_none", 8, 1, 260, 260, 3, 1, N_, N_, op="dw", res=True),
    _case("d_7", 5, 2, 36, 36, 7, 1, N_, N_, op="dw"),                         # no tile kernel for 7 x 7: yl_dw_kernel
]


def _tables():
    """One case per instantiation of the tables that a hand-written case above does not name one by one.  What varies besides
    the template arguments -- activations, residual, padding rule, partial n-tiles, channel tails, batch -- is dealt round-robin,
    so that the families meet every such property on several instantiations.  Grid 4 (one tile, all four borders) or 8."""
    out = []
    acts = ((R_, N_), (R6, R6), (SI, N_), (N_, SI), (R6, R_), (R_, R6))
    n = 0

    def add(tag, cin, cout, k, s, G=None):
        nonlocal n
        dw_act, act = acts[n % len(acts)]
        tf = s == 2 and n % 2 == 0
        out.append(_case(tag, G or (4 if n % 3 else 8), 1 + n % 3, cin, cout, k, s, dw_act, act, pad="tf" if tf else "sym", res=n % 4 == 1))
        n += 1

    # dwt_kernels[NT][DK][DS][WL] (with yl_conv_dwh_kernel<NT, DK, DS>, yl_conv_dwc_kernel<DK, DS, NTW 1 | 2> and the generic
    # kernel's <NT, 1, DW3 | DW5> under the forced forms).  Weights from L1/L2 need KB x NTtot > 36; NT 1 gets there only with
    # 3x3 taps (592 channels; the tap image of a 5x5 layer ends at 315)
    for nt in (1, 2, 3, 4, 6):
        for k in (3, 5):
            for s in (1, 2):
                for wl in (True, False):
                    kb_taps = 32 * 1024 // ((k * k + 1) * 16 * 4)                 # k-blocks whose taps + bias fit the 32 KiB image
                    kb = min(36 // nt, kb_taps) if wl else (36 // nt + 1)
                    if kb > kb_taps:
                        continue
                    cin = 16 * kb - (4 if n % 5 == 2 else 0)                       # every fifth: a 12-channel tail
                    cout = 16 * nt - (12 if n % 4 == 3 else 0)                     # every fourth: 4 channels in the last n-tile
                    add("g_t%d_%d%d%s" % (nt, k, s, "l" if wl else "g"), cin, cout, k, s)
    # 8 n-tiles: yl_conv_dwh_kernel<8, DK, DS> by default (dwt refuses NTtot > 6; KB < 12: neither dwk nor dws)
    for k in (3, 5):
        for s in (1, 2):
            add("g_h8_%d%d" % (k, s), 64, 128 - (8 if s == 2 else 0), k, s)
    # yl_conv_dwc_kernel<DK, DS, NTW 3 | 4 | 5> (tile_m 7): 9..20 n-tiles at KB = 4 = kbmax_of(4) = kbmax_of(5)
    for ntw in (3, 4, 5):
        for k in (3, 5):
            for s in (1, 2):
                add("g_c%d_%d%d" % (ntw, k, s), 64 - (4 if ntw == 3 else 0), 64 * ntw - (8 if k == 5 else 0), k, s)
    # the generic kernel's mode for any other depthwise size (7x7): <NT, 1, DWPRO> for each NT, odd and even grids
    for i, nt in enumerate((1, 2, 3, 4, 6, 8)):
        add("g_p%d" % nt, 32 + 8 * (i % 2), 16 * nt - (6 if nt == 3 else 0), 7, 1 + i % 2, G=(5, 8, 7)[i % 3])
    return out


CASES += _tables()

# ---- the classes the MODEL_ZOO layers have beyond those above (test_dw_layer_cpu.py takes the census): each case is the zoo
# layer of its class with the fewest weights, on the smallest grid (from 4 x 4; stand-alone depthwise: from 1 x 1) and batch at
# which the library's answer and the class stay the same (the window-in-LDS kernel by default dispatch needs 768 windows).
# Not below 4 x 4: on a 1 x 1 grid the yardstick's maximum is taken over c_out values only and no longer stands for the
# operation's error (192 -> 64 5x5 on 1 x 1: yardstick 1.2 ulps of max |f64| where the same shapes on 4 x 4 and larger give 3 - 5,
# the generic kernel 9.1 ulps, inside its 4 - 15 ulps on every other case: 1.85 bars there, at most 0.71 elsewhere)
CASES += [
    _case("z00", 4, 1, 48, 192, 3, 1, N_, R_),   # dwh<6, 3, 1>
    _case("z01", 4, 1, 64, 192, 5, 1, N_, R_),   # dwh<6, 5, 1>
    _case("z02", 4, 1, 96, 384, 3, 1, N_, R_),   # dwh<8, 3, 1>
    _case("z03", 4, 1, 328, 328, 3, 1, N_, R_),   # dwk<7, 3, 4>
    _case("z04", 8, 1, 328, 328, 3, 1, N_, R_),   # dwk<7, 3, 4>
    _case("z05", 4, 1, 512, 512, 3, 1, N_, R_),   # dwk<8, 1, 4>
    _case("z06", 8, 1, 512, 512, 3, 1, N_, R_),   # dwk<8, 1, 4>
    _case("z07", 4, 1, 256, 256, 3, 1, N_, R_),   # dwk<8, 2, 4>
    _case("z08", 8, 1, 256, 256, 3, 1, N_, R_),   # dwk<8, 2, 4>
    _case("z09", 4, 1, 244, 244, 3, 1, N_, R_),   # dwk<8, 2, 4>
    _case("z10", 8, 1, 244, 244, 3, 1, N_, R_),   # dwk<8, 2, 4>
    _case("z11", 8, 768, 256, 256, 3, 1, N_, R_),   # dwl<16>
    _case("z12", 8, 768, 244, 244, 3, 1, N_, R_),   # dwl<16>
    _case("z13", 8, 768, 328, 328, 3, 1, N_, R_),   # dwl<21>
    _case("z14", 4, 1, 320, 320, 3, 1, N_, R_),   # dws<11, 2, 3, 1, 4>
    _case("z15", 4, 1, 1152, 320, 3, 1, R6, N_),   # dws<11, 2, 3, 1, 4>
    _case("z16", 4, 1, 1392, 232, 5, 1, R6, N_, res=True),   # dws<11, 2, 5, 1, 4>
    _case("z17", 4, 1, 192, 192, 3, 1, N_, R_),   # dws<13, 1, 3, 1, 4>
    _case("z18", 4, 1, 196, 196, 3, 1, N_, R_),   # dws<13, 1, 3, 1, 4>
    _case("z19", 4, 1, 672, 160, 5, 1, R6, N_),   # dws<13, 1, 5, 1, 4>
    _case("z20", 4, 1, 576, 136, 5, 1, R6, N_),   # dws<13, 1, 5, 1, 4>
    _case("z21", 4, 1, 816, 136, 5, 1, R6, N_, res=True),   # dws<13, 1, 5, 1, 4>
    _case("z22", 4, 1, 672, 192, 5, 2, R6, N_, pad="tf"),   # dws<13, 1, 5, 2, 4>
    _case("z23", 4, 1, 720, 208, 5, 2, R6, N_, pad="tf"),   # dws<13, 1, 5, 2, 4>
    _case("z24", 4, 1, 512, 128, 3, 1, R_, N_, res=True),   # dws<8, 1, 3, 1, 4>
    _case("z25", 4, 1, 672, 112, 3, 1, R6, N_, res=True),   # dws<8, 1, 3, 1, 4>
    _case("z26", 4, 1, 384, 128, 5, 1, R_, N_, res=True),   # dws<8, 1, 5, 1, 4>
    _case("z27", 4, 1, 672, 112, 5, 1, R6, N_, res=True),   # dws<8, 1, 5, 1, 4>
    _case("z28", 4, 1, 528, 120, 5, 1, R6, N_),   # dws<8, 1, 5, 1, 4>
    _case("z29", 4, 1, 720, 120, 5, 1, R6, N_, res=True),   # dws<8, 1, 5, 1, 4>
    _case("z30", 4, 1, 144, 32, 3, 2, R6, N_, pad="tf"),   # dwt<2, 3, 2, 1, true, 1>
    _case("z31", 4, 1, 96, 48, 3, 1, R_, N_, res=True),   # dwt<3, 3, 1, 1, true, 1>
    _case("z32", 4, 1, 288, 48, 5, 1, R6, N_, res=True),   # dwt<3, 5, 1, 1, false, 1>
    _case("z33", 4, 1, 240, 40, 5, 1, R6, N_, res=True),   # dwt<3, 5, 1, 1, false, 1>
    _case("z34", 4, 1, 96, 48, 5, 2, R_, N_),   # dwt<3, 5, 2, 1, true, 1>
    _case("z35", 4, 1, 192, 56, 5, 2, R6, N_, pad="tf"),   # dwt<4, 5, 2, 1, false, 1>
    _case("z36", 4, 1, 192, 96, 3, 1, R_, N_, res=True),   # dwt<6, 3, 1, 1, false, 1>
    _case("z37", 4, 1, 480, 80, 3, 1, R6, N_, res=True),   # dwt<6, 3, 1, 1, false, 1>
    _case("z38", 4, 1, 528, 88, 3, 1, R6, N_, res=True),   # dwt<6, 3, 1, 1, false, 1>
    _case("z39", 4, 1, 96, 96, 3, 1, N_, R_),   # dwt<6, 3, 1, 1, true, 1>
    _case("z40", 4, 1, 288, 96, 3, 2, R6, N_, pad="tf"),   # dwt<6, 3, 2, 1, false, 1>
    _case("z41", 4, 1, 288, 88, 3, 2, R6, N_, pad="tf"),   # dwt<6, 3, 2, 1, false, 1>
    _case("z42", 4, 1, 240, 80, 3, 2, R6, N_, pad="tf"),   # dwt<6, 3, 2, 1, false, 1>
    _case("z43", 4, 1, 32, 96, 5, 1, N_, R_),   # dwt<6, 5, 1, 1, true, 1>
    _case("z44", 4, 1, 192, 96, 5, 2, R_, N_),   # dwt<6, 5, 2, 1, false, 1>
    _case("z45", 5, 1, 256, 64, 3, 1, R_, N_, res=True),   # mfma<4, 1, 3> resident
    _case("z46", 5, 1, 288, 64, 3, 2, R_, N_),   # mfma<4, 1, 3> resident
    _case("z47", 5, 1, 192, 64, 5, 1, R_, N_, res=True),   # mfma<4, 1, 5> resident
    _case("z48", 5, 1, 96, 96, 3, 1, N_, R_),   # mfma<6, 1, 3> resident
    _case("z49", 5, 1, 196, 196, 3, 1, N_, R_),   # mfma<8, 1, 3> resident
    _case("z50", 5, 1, 320, 320, 3, 1, N_, R_),   # mfma<8, 1, 3> stream
    _case("z51", 4, 1, 336, 112, 3, 2, R6, N_, pad="tf"),   # mfma<8, 1, 3> stream
    _case("z52", 8, 1, 336, 112, 3, 2, R6, N_, pad="tf"),   # mfma<8, 1, 3> stream
    _case("z53", 1, 1, 768, 768, 7, 1, N_, N_, op="dw"),   # yl_dw
    _case("z54", 1, 1, 384, 384, 7, 1, N_, N_, op="dw"),   # yl_dw
    _case("z55", 1, 1, 1152, 1152, 3, 1, N_, R6, op="dw"),   # yl_dw_tile<3, 1>
    _case("z56", 4, 1, 1392, 1392, 3, 1, N_, R6, op="dw"),   # yl_dw_tile<3, 1>
    _case("z57", 4, 1, 256, 256, 3, 2, N_, N_, op="dw"),   # yl_dw_tile<3, 2>
    _case("z58", 4, 1, 64, 64, 3, 2, N_, N_, op="dw"),   # yl_dw_tile<3, 2>
    _case("z59", 1, 1, 512, 512, 3, 2, N_, N_, op="dw"),   # yl_dw_tile<3, 2>
    _case("z60", 4, 1, 512, 512, 3, 2, N_, N_, op="dw"),   # yl_dw_tile<3, 2>
    _case("z61", 1, 1, 128, 128, 5, 1, N_, N_, op="dw"),   # yl_dw_tile<5, 1>
    _case("z62", 4, 1, 64, 64, 5, 1, N_, N_, op="dw"),   # yl_dw_tile<5, 1>
    _case("z63", 1, 1, 512, 512, 5, 1, N_, R_, op="dw"),   # yl_dw_tile<5, 1>
    _case("z64", 1, 1, 384, 384, 5, 1, N_, R_, op="dw"),   # yl_dw_tile<5, 1>
    _case("z65", 1, 1, 1152, 1152, 5, 1, N_, R6, op="dw"),   # yl_dw_tile<5, 1>
    _case("z66", 4, 1, 336, 336, 5, 1, N_, R6, op="dw"),   # yl_dw_tile<5, 1>
    _case("z67", 1, 1, 672, 672, 5, 2, N_, R6, op="dw", pad="tf"),   # yl_dw_tile<5, 2>
    _case("z68", 4, 1, 816, 816, 5, 2, N_, R6, op="dw", pad="tf"),   # yl_dw_tile<5, 2>
]
BY_TAG = {c["tag"]: c for c in CASES}
TAGS = [c["tag"] for c in CASES]


def geometry(case):
    """(input grid, leading pad, trailing pad) of the depthwise conv: the trailing pad is what the output size needs"""
    G, k, s = case["G"], case["k"], case["s"]
    Gi = (2 * G - 1) if case["odd_in"] else s * G
    if case["pad"] == "sym":
        lead = k // 2
    else:                                                # TensorFlow SAME: total = max((G - 1) s + k - Gi, 0), the smaller half leads
        lead = max((G - 1) * s + k - Gi, 0) // 2
    trail = max((G - 1) * s + k - Gi - lead, 0)
    return Gi, lead, trail


# ---- what ran: the library's own answer

def query(op, cin, cout, k, s, pad_t, pad_l, in_hw, out_hw, B, act, res, tile_m=0, dev=0, split_k=0):
    """(family id, the six template arguments) of yl_query_dw_form"""
    from yololite_amd import _lib
    a = (C.c_int32 * 6)()
    f = _lib.load().yl_query_dw_form(op, cin, cout, k, s, pad_t, pad_l, in_hw, in_hw, out_hw, out_hw, B, act, int(bool(res)),
                                     tile_m, dev, split_k, a)
    return int(f), tuple(a)


def query_case(case, tile_m=0, dev=0, split_k=0, B=None):
    Gi, lead, _ = geometry(case)
    return query(OP_DW if case["op"] == "dw" else OP_CONV, case["cin"], case["cout"], case["k"], case["s"], lead, lead, Gi, case["G"],
                 case["B"] if B is None else B, case["act"], case["res"], tile_m, DEV_BASE | dev, split_k)


def kernel_name(q, kb=None):
    """the instantiation a query answer names; kb (k-blocks of the layer): yl_conv_mfma_kernel's weights `stream` in chunks or
    are `resident`, which the fourth argument (the k-steps of the chunk) says"""
    f, a = q
    if f == DWK:
        return "yl_conv_dwk_kernel<%d, %d, %d>" % a[:3]
    if f == DWL:
        return "yl_conv_dwl_kernel<%d>" % a[0]
    if f == DWS:
        return "yl_conv_dws_kernel<%d, %d, %d, %d, %d>" % a[:5]
    if f in (DWT, DWT_SPLITK):
        return "yl_conv_dwt_kernel<%d, %d, %d, %d, %s, %d>" % (a[0], a[1], a[2], a[3], "true" if a[4] else "false", a[5])
    if f == DWC:
        return "yl_conv_dwc_kernel<%d, %d, %d>" % a[:3]
    if f == DWH:
        return "yl_conv_dwh_kernel<%d, %d, %d>" % a[:3]
    if f == MFMA:
        return "yl_conv_mfma_kernel<%d, %d, %d>" % a[:3] + ("" if kb is None else (" stream" if a[3] < kb else " resident"))
    if f == DW_TILE:
        return "yl_dw_tile_kernel<%d, %d>" % a[:2]
    if f == DW:
        return "yl_dw_kernel"
    return None


def forms(case):
    """[(name, tile_m, dev, split_k, query answer)]: the default and every candidate setting under which the query names a
    family or instantiation not yet named for the case"""
    out, seen = [], set()
    for name, tile_m, dev, split_k in CANDIDATES:
        q = query_case(case, tile_m, dev, split_k)
        if q[0] and q not in seen:
            seen.add(q)
            out.append((name, tile_m, dev, split_k, q))
    return out


def klass(q, op, cin, cout, k, s, lead, oh, ow, dw_act, act, res):
    """the class tuple (see the module docstring) of a layer for which the query answered q"""
    f = q[0]
    kb = -(-cin // 16)
    if op == OP_DW:                                      # stand-alone: a workgroup's 256-channel blocks, not k-blocks
        kbs, tail = ("1 block" if cin <= 256 else "blocks"), ("tail" if cin % 256 else "no tail")
    else:
        kbs, tail = "KB " + (str(kb) if kb <= 3 else ("even" if kb % 2 == 0 else "odd")), ("tail" if cin % 16 else "no tail")
    if f in (DWT, DWT_SPLITK, DWH, DWS, DWC):
        grid = "whole"
    elif f == DWL:
        grid = "whole" if oh % 8 == 0 and ow % 8 == 0 else "partial"
    elif f in (DWK, MFMA):
        grid = "whole" if (oh * ow) % 64 == 0 else "partial"
    elif f == DW_TILE:
        grid = "whole" if oh % 2 == 0 and ow % 4 == 0 else "partial"
    else:
        grid = "-"
    seen = lambda a: ACT_NAME[a if a < 4 else ACT_NONE]  # GELU / ReLU + affine: applied by a pass behind the kernel
    return (kernel_name(q, kb), kbs, tail, "-" if op == OP_DW else ("partial n-tile" if cout % 16 else "full n-tiles"), grid + " grid", "stride %d" % s, "sym" if lead == k // 2 else "tf%d" % lead,
            "-" if op == OP_DW else seen(dw_act), seen(act), "residual" if res and act < 4 else "no residual")


def case_class(case):
    _, lead, _ = geometry(case)
    op = OP_DW if case["op"] == "dw" else OP_CONV
    return klass(query_case(case), op, case["cin"], case["cout"], case["k"], case["s"], lead, case["G"], case["G"], case["dw_act"],
                 case["act"], case["res"])


def case_classes():
    """class -> the tags of the cases that have it (under the default options)"""
    out = {}
    for c in CASES:
        out.setdefault(case_class(c), []).append(c["tag"])
    return out


# ---- weights, inputs, programs

def weights(case):
    """(dw_w [cin, 1, k, k], dw_b [cin], w [cout, cin, 1, 1] or None, b [cout] or None) fp32, seeded per case.  Gains 3 on the taps
    and 2 on the 1x1: on inputs of unit scale both sites reach beyond ReLU6's upper clamp"""
    rng = np.random.RandomState(11000 + 37 * TAGS.index(case["tag"]))
    k, cin, cout = case["k"], case["cin"], case["cout"]
    dw_w = (3.0 * rng.randn(cin, 1, k, k) / k).astype(np.float32)
    dw_b = (0.3 * rng.randn(cin)).astype(np.float32)
    if case["op"] == "dw":
        return dw_w, dw_b, None, None
    w = (2.0 * rng.randn(cout, cin, 1, 1) / np.sqrt(cin)).astype(np.float32)
    b = (0.3 * rng.randn(cout)).astype(np.float32)
    return dw_w, dw_b, w, b


def host_inputs(case, images=None):
    """signed fp32 inputs for the tests that have no device: (x [B, Gi, Gi, cin], res [B, G, G, cout] or None)"""
    rng = np.random.RandomState(13000 + TAGS.index(case["tag"]))
    B = case["B"] if images is None else min(images, case["B"])
    Gi, _, _ = geometry(case)
    x = rng.randn(B, Gi, Gi, case["cin"]).astype(np.float32)
    r = rng.randn(B, case["G"], case["G"], case["cout"]).astype(np.float32) if case["res"] else None
    return x, r


def is_head(case):
    return case["op"] == "conv" and case["cout"] % 4 != 0


def program(case, two_launches=False):
    """stem 3 -> 32 stride 2 -> feed (1x1 32 -> cin, NO activation: signed inputs) -> [the layer] -> 1x1 head output.
    Slots: 0 stem, 1 the layer's input, 2 its output, 3 the residual (a second feed of the output's shape: 1x1 from the stem at
    stride 1, 3x3 stride 2 at stride 2).  two_launches: the layer as a YL_OP_DW layer into a slot of its own and a plain 1x1 conv.
    A layer with c_out % 4 != 0 can only be a head output (slots hold multiples of 4 channels): it is the program's head
    layer itself, with c_out - 5 classes, and its output is the level tensor (is_head)."""
    from yololite_amd import _lib
    from yololite_amd.program import Layer, Program
    assert (_lib.OP_CONV, _lib.OP_DW) == (OP_CONV, OP_DW)
    G, cin, cout, k, s = case["G"], case["cin"], case["cout"], case["k"], case["s"]
    Gi, lead, _ = geometry(case)
    rng = np.random.RandomState(5000 + TAGS.index(case["tag"]))
    dw_w, dw_b, wl, bl = weights(case)

    def w(*shape):
        return (rng.randn(*shape) / np.sqrt(int(np.prod(shape[1:])))).astype(np.float32)

    def b(n):
        return (rng.randn(n) * 0.1).astype(np.float32)

    # (no ReLU in front of the layer: it would turn the NaN image of the isolation test into zeros)
    L = [Layer(_lib.OP_STEM, -1, 0, 3, 32, 3, 2, 1, 1, ACT_NONE, w(32, 3, 3, 3), b(32), name="stem"),
         Layer(_lib.OP_CONV, 0, 1, 32, cin, 1, 1, 0, 0, ACT_NONE, w(cin, 32, 1, 1), b(cin), name="feed")]
    slots = [(Gi, Gi, 32), (Gi, Gi, cin), (G, G, cout)]
    res_slot = -1
    if case["res"]:
        res_slot = 3
        slots.append((G, G, cout))
        if s == 1:
            L.append(Layer(_lib.OP_CONV, 0, 3, 32, cout, 1, 1, 0, 0, ACT_NONE, w(cout, 32, 1, 1), b(cout), name="resfeed"))
        else:
            L.append(Layer(_lib.OP_CONV, 0, 3, 32, cout, 3, 2, 1, 1, ACT_NONE, w(cout, 32, 3, 3), b(cout), name="resfeed"))
    if case["op"] == "dw":
        assert not two_launches
        L.append(Layer(_lib.OP_DW, 1, 2, cin, cout, k, s, lead, lead, case["act"], dw_w, dw_b, res_slot=res_slot, name="dw"))
    elif two_launches:
        mid = len(slots)
        slots.append((G, G, cin))
        L.append(Layer(_lib.OP_DW, 1, mid, cin, cin, k, s, lead, lead, case["dw_act"], dw_w, dw_b, name="dw"))
        L.append(Layer(_lib.OP_CONV, mid, 2, cin, cout, 1, 1, 0, 0, case["act"], wl, bl, res_slot=res_slot, name="pw"))
    elif is_head(case):
        assert not case["res"]
        L.append(Layer(_lib.OP_CONV, 1, -1, cin, cout, 1, 1, 0, 0, case["act"], wl, bl, dw_k=k, dw_stride=s, dw_pad_t=lead,
                       dw_pad_l=lead, dw_act=case["dw_act"], dw_w=dw_w, dw_b=dw_b, head_level=0, name="dwpw"))
        return Program(img_size=2 * Gi, num_classes=cout - 5, level_size=[G], level_anchors=[1], strides=[max(1, 2 * Gi // G)],
                       layers=L, slots=slots[:2])
    else:
        L.append(Layer(_lib.OP_CONV, 1, 2, cin, cout, 1, 1, 0, 0, case["act"], wl, bl, res_slot=res_slot, dw_k=k, dw_stride=s,
                       dw_pad_t=lead, dw_pad_l=lead, dw_act=case["dw_act"], dw_w=dw_w, dw_b=dw_b, name="dwpw"))
    L.append(Layer(_lib.OP_CONV, 2, -1, cout, 6, 1, 1, 0, 0, ACT_NONE, w(6, cout, 1, 1), b(6), head_level=0, name="out"))
    return Program(img_size=2 * Gi, num_classes=1, level_size=[G], level_anchors=[1], strides=[max(1, 2 * Gi // G)], layers=L,
                   slots=slots)


# ---- the operation, in float64 (the reference) or float32 (the yardstick)

def _act(y, act):
    if act == ACT_RELU:
        return torch.relu(y)
    if act == ACT_RELU6:
        return torch.clamp(y, 0.0, 6.0)
    if act == ACT_SILU:
        return y / (1.0 + torch.exp(-y))
    return y


def layer_op(case, x, res, dtype, lead=None, clamp6=True, res_first=False, dw_bias=True, keep_channels=None):
    """The layer on the NHWC input x (and NHWC residual) in torch `dtype` -> NHWC numpy.  The keyword arguments plant ONE
    mistake each, for the CPU test: another leading pad, ReLU6 without its upper clamp, the residual added in front of the
    activation, the depthwise bias dropped, only the first `keep_channels` depthwise channels entering the 1x1 sum."""
    G, k, s = case["G"], case["k"], case["s"]
    Gi, lead0, _ = geometry(case)
    lead = lead0 if lead is None else lead
    trail = max((G - 1) * s + k - Gi - lead, 0)
    dw_w, dw_b, w, b = weights(case)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)

    def act_of(y, a):
        return torch.relu(y) if (a == ACT_RELU6 and not clamp6) else _act(y, a)

    y = F.pad(t(x).permute(0, 3, 1, 2), (lead, trail, lead, trail))
    y = F.conv2d(y, t(dw_w), t(dw_b) if dw_bias else None, stride=s, groups=case["cin"])[:, :, :G, :G]
    r = None if res is None else t(res).permute(0, 3, 1, 2)
    if case["op"] == "dw":
        a = case["act"]
    else:
        y = act_of(y, case["dw_act"])
        if keep_channels is not None:
            y = y[:, :keep_channels]
            w = w[:, :keep_channels]
        y = F.conv2d(y, t(w), t(b))
        a = case["act"]
    if r is not None and res_first:
        y = act_of(y + r, a)
    else:
        y = act_of(y, a)
        if r is not None:
            y = y + r
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def reference(case, x, res):
    return layer_op(case, x, res, torch.float64)


def yardstick(case, x, res):
    return layer_op(case, x, res, torch.float32)


def blind_border(case, x, edge):
    """a planted mistake: the input with the LAST column (edge "col") or row ("row") that the windows reach read as zero -- the
    tap on that border dropped"""
    G, k, s = case["G"], case["k"], case["s"]
    Gi, lead, _ = geometry(case)
    last = min((G - 1) * s + k - 1 - lead, Gi - 1)       # the last input column / row the last output's window holds
    x0 = x.copy()
    if edge == "col":
        x0[:, :, last] = 0
    else:
        x0[:, last] = 0
    return x0


def row(ref, yard, got=None):
    """the figures of one comparison: max |f64|, the yardstick's error, the bar and (with a result) its error and ratio"""
    m64 = float(np.abs(ref).max())
    e32 = float(np.abs(yard.astype(np.float64) - ref).max())
    r = {"max_f64": m64, "err32": e32, "bar": bar(e32, m64)}
    if got is not None:
        r["device_error"] = float(np.abs(got.astype(np.float64) - ref).max())
        r["ratio"] = r["device_error"] / r["bar"]
    return r
