// The layer program on the host: validation of a yl_model_desc, weight packing and the tables derived from the program.
// No HIP: nothing here allocates on or calls the device, and the unit compiles with a plain C++17 host compiler
// (tests/host/ runs it under the sanitizers).  yl_create (yl_api.hip) is validate -> pack -> upload on top of it.
#pragma once
#include <stddef.h>
#include <string>
#include <vector>
#include "../../include/yololite_hip.h"
#include "yl_shapes.h"

#define YL_DW_LDS_MAX (32 * 1024)   // tap image (taps + bias of all input channels) of the generic depthwise-prologue kernels

struct YlSlotDim { int h = 0, w = 0, c = 0; };

// model geometry: what the executor needs to know about a validated description besides its layers
struct YlGeometry {
  int img_size = 0, in_ch = 3, C = 0, L = 0, N = 0, E = 0, NM = 0, proto_slot = -1;
  int level_S[YL_MAX_LEVELS] = {0}, level_A[YL_MAX_LEVELS] = {0};
  int level_off[YL_MAX_LEVELS + 1] = {0};   // candidate offset of level l inside [0, N)
  std::vector<YlSlotDim> slot_dims;
  size_t se_unit = 0;        // floats per image of the YL_OP_SE / YL_OP_GRN partial-sum scratch: max over those layers of P * C
  int wino_max_hw = 0;       // max out_h * out_w over the >= 64-channel layers that carry a Winograd weight image
};

struct YlLayerInfo {
  yl_layer d;                // the caller's description (its weight pointers are the caller's memory)
  int in_h = 0, in_w = 0, out_h = 0, out_w = 0;
  int head_anchor = -1;      // head layers: anchor index handled by this layer
  bool wino = false;         // dense 3x3 stride-1 conv that also gets a Winograd F(2x2,3x3) weight image
  bool split_head = false;   // head-output conv of a model with mask coefficients that also gets the det / mc image pair
};

struct YlProgram : YlGeometry {
  std::vector<YlLayerInfo> layers;
};

// The argument checks without a message: ABI version, level count, class range.
yl_status yl_program_check_args(const yl_model_desc* d);
// Checks `d` (non-null) completely: yl_program_check_args, model geometry, slots, every layer in program order, the head
// count per level and proto_slot.  YL_OK: *p describes the model.  Otherwise *msg says what is wrong (empty for the argument
// checks) and *p is unspecified.
yl_status yl_program_validate(const yl_model_desc* d, YlProgram* p, std::string* msg);

// One host vector per device weight image of a layer; an empty vector = the layer has no such image.
//   wp / bias       packed weights / padded bias (LN, GRN: weight / bias [cin]; SE: conv_reduce)
//   dw_w / dw_b     depthwise prologue [taps][cin] / [cin]
//   w2p / b2, w3p / b3   stem block: second / third conv; fused block: expansion; chained 1x1; SE: conv_expand (transposed)
//   wino            Winograd image (YlLayerInfo::wino)
//   wp_det / b_det, wp_mc / b_mc   (YlLayerInfo::split_head) the head-output conv as two images: rows [0, 5+C) -- decode fused in
//                   the epilogue, no raw rows -- and rows [5+C, 5+C+NM), whose columns land in the level rows the mask kernels read
#define YL_LAYER_IMAGES(X) X(wp) X(bias) X(dw_w) X(dw_b) X(w2p) X(b2) X(w3p) X(b3) X(wino) X(wp_det) X(b_det) X(wp_mc) X(b_mc)
struct YlLayerImages {
#define YL_X(name) std::vector<float> name;
  YL_LAYER_IMAGES(YL_X)
#undef YL_X
};
// packs layer i of a validated program (reads the caller's weight arrays at their declared extents)
void yl_program_pack(const YlProgram& p, size_t i, YlLayerImages* im);

// tables derived from the validated program
struct YlTables {
  std::vector<unsigned char> lane;   // per layer: branch lane (empty: every layer on lane 0)
  std::vector<int> readers;          // per slot: layer operands that read it -- 1 = a single consumer
  int small_lo = 0, small_hi = 0;    // the longest run of conv layers on <= 1/16-resolution grids: layers [small_lo, small_hi)
  int tiny_lo = 0, tiny_hi = 0;      // ... of conv / depthwise / SE layers on <= 1/32-resolution grids
};
YlTables yl_program_tables(const YlProgram& p);
