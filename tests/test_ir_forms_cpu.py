"""Which form of yl_ir_kernel the launcher picks (yl_query_ir_form: host code of the library, the launcher's own decision), no
device: the second form needs clamp-type activations on all three sites and every tensor within 32-bit byte offsets; anything
else runs the first form, which is the kernel as it was."""
import ctypes as C

from yololite_amd import _lib

NONE, RELU, RELU6, SILU = (_lib.ACT[k] for k in ("none", "relu", "relu6", "silu"))
UIB = (48, 96, 48, 3, 1, 40, 40)          # edge_n's 40x40 UIB block: c_in, c_mid, c_out, dw_k, dw_stride, out_h, out_w
LAT3 = (32, 96, 96, 3, 1, 80, 80)         # lateral3 + smooth3


def _form(block, batch, in_hw, up_hw, acts):
    got = (C.c_int32 * 7)()
    f = _lib.load().yl_query_ir_form(*block, batch, in_hw, in_hw, up_hw, up_hw, *acts, got)
    return f, tuple(got)


def test_form_follows_the_three_activations():
    for acts in [(NONE, NONE, NONE), (RELU, RELU, RELU), (RELU6, RELU6, RELU6), (NONE, RELU6, RELU6), (RELU, NONE, NONE)]:
        assert _form(UIB, 64, 40, 0, acts) == (2, (3, 3, 3, 1, 1, 2, 2)), acts
    for acts in [(SILU, SILU, SILU), (SILU, RELU6, RELU6), (NONE, SILU, RELU6), (NONE, NONE, SILU)]:
        assert _form(UIB, 64, 40, 0, acts) == (1, (3, 3, 3, 1, 1, 2, 2)), acts
    assert _form(LAT3, 64, 80, 40, (RELU, NONE, NONE)) == (2, (2, 6, 3, 1, 2, 2, 2))
    assert _lib.load().yl_query_ir_form(*UIB, 64, 40, 40, 0, 0, NONE, NONE, NONE, None) == 2        # shape may be NULL


def test_shapes_without_an_instantiation_have_no_form():
    assert _form((48, 96, 48, 3, 1, 20, 20), 64, 20, 0, (NONE,) * 3)[0] == 0        # 20 x 20: no 8 x 8 tiles
    assert _form((48, 96, 48, 7, 1, 40, 40), 64, 40, 0, (NONE,) * 3)[0] == 0
    assert _form((0, 96, 48, 3, 1, 40, 40), 64, 40, 0, (NONE,) * 3)[0] == 0
    for block in (UIB, LAT3):
        assert (_lib.load().yl_query_fused_block(*block) == 1) == (_form(block, 1, block[5], 0, (NONE,) * 3)[0] != 0)


def test_tensors_past_32_bit_offsets_keep_the_first_form():
    """the block input of B images is B * 40 * 40 * 48 * 4 bytes: 2^31 lies between B = 6990 and 6991; the kernel adds a lane's
    float4 and a k-block to an offset, so the guard leaves a page of margin.  lateral3's block input (80 x 80 x 32) passes
    2^31 bytes between B = 2621 and 2622; the FPN addend is guarded on its own."""
    acts = (RELU6, RELU6, NONE)
    assert _form(UIB, 6990, 40, 0, acts)[0] == 2
    assert _form(UIB, 6991, 40, 0, acts)[0] == 1
    assert _form(UIB, 1 << 20, 40, 0, acts)[0] == 1
    assert _form(LAT3, 2600, 80, 40, acts)[0] == 2
    assert _form(LAT3, 2700, 80, 40, acts)[0] == 1          # 2700 * 80 * 80 * 32 * 4 > 2^31: the block input
    assert _form((32, 96, 96, 3, 1, 80, 80), 2600, 80, 80, acts)[0] == 1     # an addend of the full size: 2600 * 80 * 80 * 96 * 4
