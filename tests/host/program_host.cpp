// Stand-alone check of the host unit csrc/yl_program.cpp: validates one small program that has a layer of every kind, packs
// every layer and checks each image's size against its formula; then hands the validator descriptions it must refuse.
// Built by tests/test_program_host_cpu.py with -fsanitize=address,undefined together with yl_program.cpp, and linked
// against the library only for the four shape predicates.  Every source array is a heap block of exactly its declared
// extent, so a packer that reads past one is caught.  Prints "ok" and exits 0, or says what failed and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <memory>
#include <string>
#include <vector>

#include "../../yololite-official-repo_amd/csrc/yl_program.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) { printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

std::vector<std::unique_ptr<float[]>> arrays;
const float* arr(size_t n) {           // exactly n floats on the heap
  arrays.emplace_back(new float[n]);
  for (size_t i = 0; i < n; ++i) arrays.back()[i] = 0.25f * (float)((i * 7 + arrays.size()) % 13) - 1.0f;
  return arrays.back().get();
}

size_t cdiv(size_t a, size_t b) { return (a + b - 1) / b; }

yl_layer plain(int op, int in_slot, int out_slot, int cin, int cout, int k, int pad) {
  yl_layer l = {};
  l.op = op; l.in_slot = in_slot; l.out_slot = out_slot; l.res_slot = l.up_slot = l.head_level = l.scale_slot = -1;
  l.cin = cin; l.cout = cout; l.k = k; l.stride = 1; l.pad_t = l.pad_l = pad; l.dw_stride = 1;
  return l;
}
yl_layer conv(int in_slot, int out_slot, int cin, int cout, int k) {
  yl_layer l = plain(YL_OP_CONV, in_slot, out_slot, cin, cout, k, k / 2);
  l.w = arr((size_t)cout * cin * k * k); l.b = arr(cout); l.act = YL_ACT_RELU;
  return l;
}

// slots: h, w, c
const int SH[] = {8, 8, 8, 8, 8, 8, 8, 8, 8, 1, 8, 8, 1, 8, 16, 16, 8, 4, 4, 8};
const int SW[] = {8, 8, 8, 8, 8, 8, 8, 8, 8, 1, 8, 8, 1, 8, 16, 16, 8, 4, 4, 8};
const int SC[] = {16, 4, 8, 24, 20, 8, 24, 40, 4, 8, 8, 8, 8, 12, 24, 24, 8, 8, 12, 8};
const int NSLOT = sizeof(SC) / sizeof(SC[0]);
const int C = 3, NM = 4, E = 5 + C + NM;

std::vector<yl_layer> layers() {
  std::vector<yl_layer> v;
  yl_layer l = plain(YL_OP_STEM, -1, 0, 3, 16, 3, 1);                           // 0: stem at 16 outputs
  l.stride = 2; l.w = arr(16 * 27); l.b = arr(16); l.act = YL_ACT_RELU;
  v.push_back(l);
  v.push_back(conv(0, 1, 16, 4, 1));                                             // 1
  v.push_back(conv(1, 2, 4, 8, 1));                                              // 2: cout 8, cin 4, 1x1
  v.push_back(conv(1, 3, 4, 24, 3));                                             // 3: cout 24, cin 4, 3x3
  v.push_back(conv(3, 4, 24, 20, 1));                                            // 4
  v.push_back(conv(4, 5, 20, 8, 3));                                             // 5: cout 8, cin 20, 3x3 (no Winograd image: cout < 16)
  v.push_back(conv(4, 6, 20, 24, 1));                                            // 6: cout 24, cin 20, 1x1
  v.push_back(conv(4, 7, 20, 40, 3));                                            // 7: Winograd, 3 n-tiles: the second n-group half empty
  l = plain(YL_OP_DW, 1, 8, 4, 4, 5, 2);                                         // 8: depthwise 5x5 on 4 channels
  l.w = arr(4 * 25); l.b = arr(4);
  v.push_back(l);
  l = plain(YL_OP_SE, 2, 9, 8, 4, 1, 0);                                         // 9: squeeze-excite 8 -> 4 -> 8
  l.c2 = 8; l.w = arr(4 * 8); l.b = arr(4); l.w2 = arr(8 * 4); l.b2 = arr(8); l.act = YL_ACT_SILU;
  v.push_back(l);
  l = conv(2, 10, 8, 8, 1); l.scale_slot = 9;                                    // 10: its consumer
  v.push_back(l);
  l = plain(YL_OP_LN, 2, 11, 8, 8, 1, 0); l.w = arr(8); l.b = arr(8); l.eps = 1e-6f;   // 11
  v.push_back(l);
  l = plain(YL_OP_GRN, 2, 12, 8, 8, 1, 0); l.w = arr(8); l.eps = 1e-6f;                // 12
  v.push_back(l);
  l = conv(1, 13, 4, 8, 3); l.c3 = 12; l.w3 = arr(12 * 8); l.b3 = arr(12); l.act3 = YL_ACT_RELU;   // 13: chained 1x1
  v.push_back(l);
  l = plain(YL_OP_CONV, 14, 15, 144, 24, 1, 0);                                  // 14: fused block 24 -> 144 -> dw 3x3 -> 24 on 16 x 16
  l.c2 = 24; l.w2 = arr(144 * 24); l.b2 = arr(144); l.act2 = YL_ACT_RELU6;
  l.dw_k = 3; l.dw_pad_t = l.dw_pad_l = 1; l.dw_w = arr(144 * 9); l.dw_b = arr(144); l.dw_act = YL_ACT_RELU6;
  l.w = arr(24 * 144); l.b = arr(24);
  v.push_back(l);
  l = conv(1, 16, 4, 8, 1);                                                      // 15: depthwise 3x3 prologue, with and ...
  l.dw_k = 3; l.dw_pad_t = l.dw_pad_l = 1; l.dw_w = arr(4 * 9); l.dw_b = arr(4);
  v.push_back(l);
  l = conv(1, 16, 4, 8, 1);                                                      // 16: ... without its bias, main conv without bias
  l.dw_k = 3; l.dw_pad_t = l.dw_pad_l = 1; l.dw_w = arr(4 * 9); l.b = nullptr;
  v.push_back(l);
  l = plain(YL_OP_STEMBLOCK, -1, 17, 3, 16, 3, 1);                               // 17: stem block rows with bias, no third conv
  l.stride = 2; l.w = arr(16 * 27); l.b = arr(16); l.act = YL_ACT_RELU;
  l.c2 = 8; l.w2 = arr(8 * 16 * 9); l.b2 = arr(8); l.act2 = YL_ACT_RELU;
  v.push_back(l);
  l = plain(YL_OP_STEMBLOCK, -1, 18, 3, 16, 3, 1);                               // 18: ... without bias, with the 1x1
  l.stride = 2; l.w = arr(16 * 27); l.act = YL_ACT_RELU;
  l.c2 = 8; l.w2 = arr(8 * 16 * 9); l.act2 = YL_ACT_RELU; l.c3 = 12; l.w3 = arr(12 * 8); l.b3 = arr(12);
  v.push_back(l);
  l = plain(YL_OP_STEMBLOCK, -1, 19, 3, 32, 3, 1);                               // 19: depthwise second conv
  l.stride = 2; l.w = arr(32 * 27); l.b = arr(32); l.act = YL_ACT_RELU6;
  l.c2 = 32; l.dw_k = 3; l.dw_pad_t = l.dw_pad_l = 1; l.w2 = arr(32 * 9); l.b2 = arr(32); l.act2 = YL_ACT_RELU6;
  l.c3 = 8; l.w3 = arr(8 * 32); l.b3 = arr(8);
  v.push_back(l);
  l = conv(2, -1, 8, E, 1); l.head_level = 0; l.act = YL_ACT_NONE;               // 20: head output, NM = 4, C = 3: the split form
  v.push_back(l);
  return v;
}

yl_model_desc model(const std::vector<yl_layer>& ls) {
  yl_model_desc d = {};
  d.abi_version = YL_ABI_VERSION; d.img_size = 16; d.in_channels = 3; d.num_classes = C; d.num_masks = NM; d.proto_slot = 1;
  d.num_levels = 1; d.level_size[0] = 8; d.level_anchors[0] = 1;
  d.num_slots = NSLOT; d.slot_h = SH; d.slot_w = SW; d.slot_c = SC;
  d.num_layers = (int)ls.size(); d.layers = ls.data();
  return d;
}

void check_images(const YlProgram& p, size_t i, const YlLayerImages& im) {
  const YlLayerInfo& L = p.layers[i];
  const yl_layer& l = L.d;
  const size_t cin = l.cin, cout = l.cout, taps = (size_t)l.k * l.k;
  size_t n_images = 0;
#define YL_X(name) n_images += !im.name.empty();
  YL_LAYER_IMAGES(YL_X)
#undef YL_X
  size_t expect = 0;          // images the layer must have
  auto conv_image = [](size_t co, size_t ci, size_t t) { return t * cdiv(ci, 16) * cdiv(co, 16) * 256; };
  switch (l.op) {
    case YL_OP_STEM:
      CHECK(im.wp.size() == 7 * cdiv(cout, 16) * 64 && im.bias.size() == cout);
      expect = 2;
      break;
    case YL_OP_STEMBLOCK:
      CHECK(im.wp.size() == 7 * cdiv(cout, 16) * 64 && im.bias.size() == cout);
      CHECK(im.w2p.size() == (l.dw_k == 3 ? (size_t)9 * l.c2 : conv_image(l.c2, cout, 9)) && im.b2.size() == cdiv(l.c2, 16) * 16);
      CHECK(l.c3 == 0 || (im.w3p.size() == conv_image(l.c3, l.c2, 1) && im.b3.size() == cdiv(l.c3, 16) * 16));
      CHECK(im.wp[(6 * cdiv(cout, 16) + 0) * 64 + 48] == (l.b ? l.b[0] : 0.0f));     // the bias rides in the K pad slot
      expect = l.c3 > 0 ? 6 : 4;
      break;
    case YL_OP_DW:
      CHECK(im.wp.size() == taps * cout && im.bias.size() == cout);
      CHECK(im.wp[1 * cout + 2] == l.w[2 * taps + 1]);                                  // [c][tap] -> [tap][c]
      expect = 2;
      break;
    case YL_OP_SE:
      CHECK(im.wp.size() == cout * cin && im.bias.size() == cout && im.w2p.size() == cin * cout && im.b2.size() == cin);
      CHECK(im.w2p[3 * cin + 5] == l.w2[5 * cout + 3]);                                 // conv_expand transposed
      expect = 4;
      break;
    case YL_OP_LN:
      CHECK(im.wp.size() == cin && im.bias.size() == cin);
      expect = 2;
      break;
    case YL_OP_GRN:
      CHECK(im.wp.size() == cin);
      expect = 1;
      break;
    case YL_OP_CONV: {
      CHECK(im.wp.size() == conv_image(cout, cin, taps) && im.bias.size() == cdiv(cout, 16) * 16 + 128);
      double src = 0, dst = 0;                   // the image is the weights in another order, zero padded
      for (size_t j = 0; j < cout * cin * taps; ++j) src += l.w[j];
      for (float x : im.wp) dst += x;
      CHECK(src == dst);
      CHECK(im.bias[cout - 1] == (l.b ? l.b[cout - 1] : 0.0f) && im.bias[cout] == 0.0f);
      expect = 2;
      CHECK(L.wino == (i == 7));
      if (L.wino) { CHECK(im.wino.size() == cdiv(cdiv(cout, 16), 2) * cdiv(cin, 16) * 16 * 2 * 256); ++expect; }
      CHECK(L.split_head == (l.head_level >= 0));
      if (L.split_head) {
        CHECK(im.wp_det.size() == conv_image(5 + C, cin, 1) && im.b_det.size() == cdiv(5 + C, 16) * 16 + 128);
        CHECK(im.wp_mc.size() == conv_image(NM, cin, 1) && im.b_mc.size() == cdiv(NM, 16) * 16 + 128);
        CHECK(im.b_det[5 + C - 1] == l.b[5 + C - 1] && im.b_det[5 + C] == 0.0f && im.b_mc[0] == l.b[5 + C] && im.b_mc[NM] == 0.0f);
        expect += 4;
      }
      if (l.c3 > 0) { CHECK(im.w3p.size() == conv_image(l.c3, cout, 1) && im.b3.size() == cdiv(l.c3, 16) * 16); expect += 2; }
      if (l.c2 > 0) { CHECK(im.w2p.size() == conv_image(cin, l.c2, 1) && im.b2.size() == cdiv(cin, 16) * 16); expect += 2; }
      if (l.dw_k > 0) {
        CHECK(im.dw_w.size() == (size_t)l.dw_k * l.dw_k * cin && im.dw_b.size() == (l.dw_b ? cin : 0));
        expect += l.dw_b ? 2 : 1;
      }
      break;
    }
    default:
      break;
  }
  if (n_images != expect) { printf("layer %zu: %zu images, expected %zu\n", i, n_images, expect); ++failures; }
}

// the validator must refuse `d` with a message, not crash
void refused(const char* what, const yl_model_desc& d) {
  YlProgram p;
  std::string msg;
  const yl_status s = yl_program_validate(&d, &p, &msg);
  if (s == YL_OK || msg.empty()) { printf("%s: not refused (status %d)\n", what, (int)s); ++failures; }
}

}  // namespace

int main() {
  const std::vector<yl_layer> ls = layers();
  const yl_model_desc d = model(ls);
  YlProgram p;
  std::string msg;
  const yl_status s = yl_program_validate(&d, &p, &msg);
  if (s != YL_OK) { printf("the valid program is refused: %d %s\n", (int)s, msg.c_str()); return 1; }
  CHECK(p.layers.size() == ls.size() && p.N == 64 && p.E == E && p.level_off[1] == 64);
  CHECK(p.se_unit == (size_t)64 * 8 && p.wino_max_hw == 0);
  CHECK(p.layers[20].head_anchor == 0 && p.layers[20].out_h == 8 && p.layers[14].in_h == 16 && p.layers[19].out_h == 8);
  YlLayerImages im;
  for (size_t i = 0; i < p.layers.size(); ++i) {
    yl_program_pack(p, i, &im);
    check_images(p, i, im);
  }
  const YlTables t = yl_program_tables(p);
  CHECK(t.readers.size() == (size_t)NSLOT && t.readers[1] == 6 && t.readers[0] == 1);
  CHECK(t.lane.empty() || t.lane.size() == ls.size());

  yl_model_desc e = d;
  e.layers = nullptr;
  refused("null layers", e);
  e = d; e.slot_c = nullptr;
  refused("null slot_c", e);
  struct { const char* what; size_t layer; int32_t yl_layer::*field; int32_t value; } const slots[] = {
      {"in_slot past the end", 2, &yl_layer::in_slot, NSLOT},   {"negative in_slot", 2, &yl_layer::in_slot, -1},
      {"out_slot past the end", 2, &yl_layer::out_slot, NSLOT}, {"negative out_slot", 8, &yl_layer::out_slot, -7},
      {"res_slot past the end", 2, &yl_layer::res_slot, 1 << 30}, {"up_slot past the end", 2, &yl_layer::up_slot, NSLOT},
      {"scale_slot past the end", 10, &yl_layer::scale_slot, NSLOT}, {"SE out_slot past the end", 9, &yl_layer::out_slot, NSLOT},
      {"LN in_slot past the end", 11, &yl_layer::in_slot, NSLOT}, {"GRN out_slot negative", 12, &yl_layer::out_slot, -1},
      {"fused block out_slot past the end", 14, &yl_layer::out_slot, NSLOT}, {"head_level past the end", 20, &yl_layer::head_level, 1},
  };
  for (const auto& c : slots) {
    std::vector<yl_layer> m = ls;
    m[c.layer].*c.field = c.value;
    refused(c.what, model(m));
  }
  for (size_t i : {(size_t)0, (size_t)2, (size_t)8, (size_t)9, (size_t)11, (size_t)12, (size_t)17}) {
    std::vector<yl_layer> m = ls;
    m[i].w = nullptr;
    refused("null w", model(m));
  }
  e = d; e.proto_slot = NSLOT;
  refused("proto_slot past the end", e);

  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
