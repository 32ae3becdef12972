"""Named yl_create cases: one field of a small valid program changed, and what yl_create must say about it.

Shared by tests/golden/make_create_fixtures.py (records status and message of every case at the commit BEFORE the
executor's validation moved to the host unit, on a GPU machine) and tests/test_create_errors_cpu.py (asserts them, with
or without a device).  Every distinct message text of yl_create's validation is produced by at least one case
(MESSAGE_TEXTS counts them); HIP failures are not validation and have no case.

Bases (3 classes, 64 x 64, seeded synthetic weights): edge_n; edge_n with the mask branch (num_masks / proto_slot / the
split head output); yololite_n for the fused inverted-residual block and the depthwise stem block; and, for the ops edge_n
does not have, the smallest zoo model with them: edge_xl (POOL, COPY), yololite_n_v2 (plain STEM, SE, scale_slot),
yololite_l_v2 (NHWC4, LN, GRN).

A case is (name, base, edit).  edit(prog) changes a private copy of the base Program (use `put`) and may return a
function that changes the filled yl_model_desc (fields no Program carries)."""
import copy
import ctypes
import dataclasses
import functools

from yololite_amd import _lib
from yololite_amd.model import model_desc
from yololite_amd.program import SynthStateDict, build_program, zoo_meta

MESSAGE_TEXTS = 63      # distinct message texts in yl_create's validation at the recording commit

BASES = {
    "edge_n": ("edge_n", {}),
    "edge_n_seg": ("edge_n", {"seg": True}),
    "yololite_n": ("yololite_n", {}),
    "edge_xl": ("edge_xl", {}),
    "yololite_n_v2": ("yololite_n_v2", {}),
    "yololite_l_v2": ("yololite_l_v2", {}),
}


@functools.lru_cache(maxsize=None)
def base_program(base):
    name, kw = BASES[base]
    return build_program(zoo_meta(name, num_classes=3, img_size=64, **kw), SynthStateDict(seed=1, num_classes=3))


def at(prog, name):
    """index of the layer called `name`"""
    return [l.name for l in prog.layers].index(name)


def first(prog, **fields):
    """index of the first layer whose fields have these values"""
    return next(i for i, l in enumerate(prog.layers) if all(getattr(l, k) == v for k, v in fields.items()))


def put(prog, i, **fields):
    prog.layers[i] = dataclasses.replace(prog.layers[i], **fields)


def slot(prog, s, h=None, w=None, c=None):
    o = prog.slots[s]
    prog.slots[s] = (o[0] if h is None else h, o[1] if w is None else w, o[2] if c is None else c)


def layer(name_or_fields, **fields):
    """edit: change fields of one layer, found by name or by field values"""
    def edit(prog):
        i = at(prog, name_or_fields) if isinstance(name_or_fields, str) else first(prog, **name_or_fields)
        put(prog, i, **fields)
    return edit


def desc(**fields):
    """edit: set fields of the descriptor (level_size / level_anchors: {index: value})"""
    def edit(prog):
        def on_desc(d):
            for k, v in fields.items():
                if isinstance(v, dict):
                    for i, x in v.items():
                        getattr(d, k)[i] = x
                else:
                    setattr(d, k, v)
        return on_desc
    return edit


def _null_layers(prog):
    def on_desc(d):
        d.layers = ctypes.POINTER(_lib.yl_layer)()
    return on_desc


def _reserved0(prog):
    def on_desc(d):
        d.layers[2].reserved0 = 1
    return on_desc


def _slot_channels(prog):
    slot(prog, 5, c=50)


def _stem_block_size(prog):
    slot(prog, prog.layers[0].out_slot, h=15, w=15)


def _no_head_for_last_level(prog):
    del prog.layers[-1]


def _proto_slot(value):
    def edit(prog):
        prog.proto_slot = value
    return edit


def _second_head_on_level0(prog):
    put(prog, at(prog, "head4.out[a=0]"), head_level=0)


def _conv_as_depthwise(prog):
    put(prog, at(prog, "backbone.blocks.2.1.pw_exp.conv"), op=2)       # 1x1 48 -> 96 declared YL_OP_DW


def _two_faulty_layers(prog):
    put(prog, 5, k=0)
    put(prog, 2, op=10)


# the fused inverted-residual block of yololite_n: 24 -> 144 -> depthwise 3x3 s1 -> 24 on 16 x 16, with a residual
_IR = "backbone.blocks.1.1.ir"


def _ir(**fields):
    return layer(_IR, **fields)


def _ir_odd_grid(prog):
    prog.slots += [(6, 6, 24), (6, 6, 24)]                 # the block on a 6 x 6 grid of its own
    put(prog, at(prog, _IR), in_slot=len(prog.slots) - 2, out_slot=len(prog.slots) - 1, res_slot=-1)


def _chained_with_residual(prog):
    i = at(prog, _K3)
    prog.slots.append((8, 8, prog.layers[i].cout))         # a residual of the k x k conv's own output shape
    put(prog, i, res_slot=len(prog.slots) - 1)


_PW = "backbone.blocks.2.1.pw_exp.conv"          # edge_n: plain 1x1 48 -> 96 on 4 x 4
_DWPW = "backbone.blocks.2.0.pw_exp.conv"        # edge_n: depthwise 5x5 -> 1x1 32 -> 96 on 8 x 8
_K3 = "backbone.blocks.1.0.conv+1.conv"          # edge_n: dense 3x3 s2 16 -> 48 with a chained 1x1 48 -> 32
_RES = "backbone.blocks.2.1.pw_proj.conv"        # edge_n: depthwise 3x3 -> 1x1 96 -> 48 with a residual
_HEAD = "head3.out[a=0]"
_SE = "backbone.blocks.3.0.se.gate"              # yololite_n_v2
_PWL = "backbone.blocks.3.0.conv_pwl"            # yololite_n_v2: the 1x1 conv that takes the gate

CASES = [
    # ---- the model
    ("num_masks_range", "edge_n", desc(num_masks=65)),
    ("level_geometry", "edge_n", desc(level_size={1: 0})),
    ("too_many_candidates", "edge_n", desc(level_size={0: 1024})),
    ("input_channels", "edge_n", desc(in_channels=4)),
    ("null_layers", "edge_n", _null_layers),
    ("slot_channels", "edge_n", _slot_channels),
    ("heads_per_level", "edge_n", _no_head_for_last_level),
    ("proto_slot_missing", "edge_n_seg", _proto_slot(-1)),
    ("proto_slot_channels", "edge_n_seg", _proto_slot(0)),
    ("num_masks_range_seg", "edge_n_seg", desc(num_masks=-1)),
    # ---- any layer
    ("unknown_op", "edge_n", layer(_PW, op=10)),
    ("reserved0", "edge_n", _reserved0),
    ("unknown_activation", "edge_n", layer(_PW, act=6)),
    ("unknown_act3", "edge_n", layer(_K3, act3=4)),
    ("postpass_on_head", "edge_n", layer(_HEAD, act=4)),
    ("out_ch_off_on_conv", "edge_n", layer(_PW, out_ch_off=4)),
    ("two_faulty_layers", "edge_n", _two_faulty_layers),
    # ---- element-wise ops
    ("pool_out_slot", "edge_xl", layer("backbone.stem.pool", out_slot=-1)),
    ("pool_in_slot", "edge_xl", layer("backbone.stem.pool", in_slot=999)),
    ("pool_conv_field", "edge_xl", layer("backbone.stem.pool", act=1)),
    ("pool_cin", "edge_xl", layer("backbone.stem.pool", cin=12)),
    ("pool_geometry", "edge_xl", layer("backbone.stem.pool", k=0)),
    ("copy_slice", "edge_xl", layer("backbone.stem.cat[1]", out_ch_off=20)),
    ("nhwc4_cout", "yololite_l_v2", layer("backbone.input.nhwc4", cout=8)),
    ("ln_eps", "yololite_l_v2", layer("backbone.stem_1", eps=0.0)),
    ("ln_no_bias", "yololite_l_v2", layer("backbone.stem_1", b=None)),
    ("grn_eps", "yololite_l_v2", layer("backbone.stages_0.blocks.0.mlp.grn", eps=0.0)),
    # ---- weights, kernel
    ("null_weights", "edge_n", layer(_PW, w=None)),
    ("kernel_geometry", "edge_n", layer(_PW, k=0)),
    # ---- squeeze-excite and its consumer
    ("se_slot", "yololite_n_v2", layer(_SE, out_slot=-1)),
    ("se_out_dims", "yololite_n_v2", lambda p: put(p, at(p, _SE), out_slot=p.layers[at(p, _SE)].in_slot)),
    ("se_no_b2", "yololite_n_v2", layer(_SE, b2=None)),
    ("se_conv_field", "yololite_n_v2", layer(_SE, k=3)),
    ("scale_slot_on_3x3", "yololite_n_v2", layer(_PWL, k=3)),
    ("scale_slot_dims", "yololite_n_v2", lambda p: put(p, at(p, _PWL), scale_slot=p.layers[at(p, _PWL)].in_slot)),
    # ---- stem, stem block
    ("stem_kernel", "yololite_n_v2", layer("backbone.conv_stem", k=5)),
    ("stem_cout", "yololite_n_v2", layer("backbone.conv_stem", cout=24)),
    ("stemblock_kernel", "edge_n", layer({"op": 3}, k=5)),
    ("stemblock_no_w2", "edge_n", layer({"op": 3}, w2=None)),
    ("stemblock_silu", "edge_n", layer({"op": 3}, act2=3)),
    ("stemblock_dw_k", "edge_n", layer({"op": 3}, dw_k=5)),
    ("stemblock_shape", "edge_n", layer({"op": 3}, c2=36)),
    ("stemblock_dw_shape", "yololite_n", layer({"op": 3}, c3=36)),
    ("stemblock_size", "edge_n", _stem_block_size),
    # ---- input side of a conv
    ("conv_in_slot", "edge_n", layer(_PW, in_slot=-1)),
    ("in_shift_on_1x1", "edge_n", layer(_PW, in_shift=1)),
    ("cin_mismatch", "edge_n", layer(_PW, cin=44)),
    # ---- fused inverted-residual block
    ("fused_no_w2", "yololite_n", _ir(w2=None)),
    ("fused_upsample", "yololite_n", _ir(dw_k=4, up_slot=0)),
    ("fused_stride2", "yololite_n", _ir(dw_k=4, dw_stride=2)),
    ("fused_shape", "yololite_n", _ir(dw_k=4)),
    ("fused_odd_grid", "yololite_n", _ir_odd_grid),
    ("fused_cin_mod4", "yololite_n", _ir(cin=142)),
    # ---- depthwise prologue
    ("dw_main_3x3", "edge_n", layer(_DWPW, k=3)),
    ("dw_null_weights", "edge_n", layer(_DWPW, dw_w=None)),
    ("dw_stride", "edge_n", layer(_DWPW, dw_stride=0)),
    ("dw_lds", "edge_n", layer("backbone.blocks.3.0.pw_proj.conv", dw_k=7)),
    # ---- head layers
    ("head_level", "edge_n", layer(_HEAD, head_level=3)),
    ("head_cout", "edge_n", layer(_HEAD, cout=12)),
    ("head_anchors", "edge_n", _second_head_on_level0),
    ("head_residual", "edge_n", layer(_HEAD, res_slot=0)),
    ("split_head_cout", "edge_n_seg", layer(_HEAD, cout=8)),
    ("split_head_residual", "edge_n_seg", layer(_HEAD, up_slot=0)),
    # ---- output side
    ("conv_out_slot", "edge_n", layer(_PW, out_slot=999)),
    ("cout_mismatch", "edge_n", layer(_PW, cout=44)),
    ("output_size", "edge_n", layer(_K3, pad_t=3)),
    ("res_slot_range", "edge_n", layer(_RES, res_slot=999)),
    ("res_shape", "edge_n", layer(_RES, res_slot=0)),
    ("up_slot_range", "edge_n", layer("lateral4", up_slot=999)),
    ("up_channels", "edge_n", layer("lateral4", up_slot=13)),
    ("depthwise_cin_cout", "edge_n", _conv_as_depthwise),
    ("silu_cout_mod4", "edge_n", layer(_K3, cout=46, act=3)),
    # ---- the check that used to run after the layer's first uploads
    ("chained_1x1_silu", "edge_n", layer(_K3, act3=3)),
    ("chained_1x1_residual", "edge_n", _chained_with_residual),
]


def build_case(base, edit=None):
    """(descriptor, keep) of a base program with `edit` applied; `keep` must outlive yl_create"""
    prog = copy.copy(base_program(base))
    prog.layers, prog.slots = list(prog.layers), list(prog.slots)
    on_desc = edit(prog) if edit else None
    d, keep = model_desc(prog.img_size, prog.num_classes, prog.level_size, prog.level_anchors, prog)
    if on_desc:
        on_desc(d)
    return d, keep


def create(lib, d, device=0):
    """yl_create -> (status, message, handle); the caller destroys a handle that is not null"""
    h = ctypes.c_void_p()
    st = lib.yl_create(ctypes.byref(d), device, ctypes.byref(h))
    return int(st), (lib.yl_last_error(h).decode() if h else ""), h
