"""Both forms of yl_ir_kernel (fused 1x1 expand -> depthwise -> 1x1 project, and the FPN lateral + smooth pair), each of the eight
instantiations on its own in a one-block network: the head output is bitwise the two-launch form's (the expansion as
yl_conv_pwt_kernel into a tensor in memory, then the depthwise -> 1x1 kernels: independent code), and the form that ran is the
one the library names (yl_query_ir_form, the launcher's own decision): the second form for none / ReLU / ReLU6 on all three
sites, the first form as soon as SiLU is among them.

Grids are the smallest at which the kernel can still go wrong.  Images are square here, so an instantiation with 8 x 16 tiles
(MT = 2) cannot be given a single tile: its smallest grid is 16 x 16 (two tiles, each on three borders), then 32 x 32 (4 x 2
tiles) and 48 x 48 (6 x 3: interior tiles); the 8 x 8-tile instantiations run 8 x 8 (one tile on all four borders), 16 x 16 and
24 x 24.  Every case runs B = 1 and B = 3: with fewer than 8 tiles (8 x 8 and 16 x 16 grids) the kernel deals its tiles
without XCD bands, otherwise in bands of a tile count that is no multiple of 8."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from yololite_amd import _lib
from yololite_amd.program import Layer, Program

from test_gpu_parity import DEV, _x

NONE, RELU, RELU6, SILU = (_lib.ACT[k] for k in ("none", "relu", "relu6", "silu"))
# instantiation -> channels (block input, expanded, output) that select it; the first five are yololite_m's blocks, then edge_n's
# 40x40 UIB block and its two lateral + smooth pairs
SHAPES = {
    (1, 2, 3, 2, 1, 2, 2): (16, 96, 24),
    (2, 2, 3, 1, 2, 2, 2): (24, 144, 24),
    (2, 3, 5, 2, 1, 2, 2): (24, 144, 48),
    (3, 3, 5, 1, 2, 2, 2): (48, 288, 48),
    (3, 6, 3, 2, 1, 2, 2): (48, 288, 88),
    (3, 3, 3, 1, 1, 2, 2): (48, 96, 48),
    (2, 6, 3, 1, 2, 2, 2): (32, 96, 96),
    (3, 6, 3, 1, 1, 2, 2): (48, 96, 96),
}
LATERAL = {(2, 6, 3, 1, 2, 2, 2), (3, 6, 3, 1, 1, 2, 2)}


def _programs(c1, cmid, n, dk, ds, G, acts, res, up):
    """stem -> 1x1 feed (32 -> c1) -> the block -> head, as (one fused layer, expansion and depthwise -> projection as two
    layers).  acts = (expansion, depthwise, projection); res: a skip tensor added to the projection; up: a coarser tensor of
    half the size added nearest-upsampled to the expansion (the FPN lateral).  G: output grid of the block"""
    rng = np.random.RandomState(c1 + 7 * cmid + 31 * n + dk + G)
    act2, dw_act, act = acts
    Gi = G * ds

    def w(*shape):
        return (rng.randn(*shape) / np.sqrt(int(np.prod(shape[1:])))).astype(np.float32)

    def b(c):
        return (rng.randn(c) * 0.1).astype(np.float32)

    slots = [(Gi, Gi, 32), (Gi, Gi, c1), (G, G, n)]
    pre = [Layer(_lib.OP_STEM, -1, 0, 3, 32, 3, 2, 1, 1, RELU, w(32, 3, 3, 3), b(32), name="stem"),
           Layer(_lib.OP_CONV, 0, 1, 32, c1, 1, 1, 0, 0, RELU, w(c1, 32, 1, 1), b(c1), name="feed")]
    res_slot = up_slot = -1
    if res:
        assert ds == 1
        res_slot = len(slots)
        slots.append((G, G, n))
        pre.append(Layer(_lib.OP_CONV, 0, res_slot, 32, n, 1, 1, 0, 0, NONE, w(n, 32, 1, 1), b(n), name="skip"))
    if up:
        up_slot = len(slots)
        slots.append((Gi // 2, Gi // 2, cmid))
        pre.append(Layer(_lib.OP_CONV, 0, up_slot, 32, cmid, 3, 2, 1, 1, RELU, w(cmid, 32, 3, 3), b(cmid), name="coarse"))
    w2, b2, dww, dwb, wp, bp = w(cmid, c1, 1, 1), b(cmid), w(cmid, 1, dk, dk), b(cmid), w(n, cmid, 1, 1), b(n)
    dwk = dict(dw_k=dk, dw_stride=ds, dw_pad_t=dk // 2, dw_pad_l=dk // 2, dw_act=dw_act, dw_w=dww, dw_b=dwb)
    head = Layer(_lib.OP_CONV, 2, -1, n, 6, 1, 1, 0, 0, NONE, w(6, n, 1, 1), b(6), head_level=0, name="out")
    fused = [Layer(_lib.OP_CONV, 1, 2, cmid, n, 1, 1, 0, 0, act, wp, bp, res_slot=res_slot, up_slot=up_slot, c2=c1, act2=act2,
                   w2=w2, b2=b2, name="block", **dwk)]
    mid = len(slots)
    two = [Layer(_lib.OP_CONV, 1, mid, c1, cmid, 1, 1, 0, 0, act2, w2, b2, up_slot=up_slot, name="expand"),
           Layer(_lib.OP_CONV, mid, 2, cmid, n, 1, 1, 0, 0, act, wp, bp, res_slot=res_slot, name="project", **dwk)]

    def prog(block, sl):
        return Program(img_size=2 * Gi, num_classes=1, level_size=[G], level_anchors=[1], strides=[2 * ds], layers=pre + block + [head],
                       slots=sl)
    return prog(fused, slots), prog(two, slots + [(Gi, Gi, cmid)])


def _ctx_of(p):
    from yololite_amd.model import HipContext
    ctx = HipContext(p.img_size, p.num_classes, p.level_size, p.level_anchors, p, 0)
    ctx.set_option("streams", 1)
    ctx.set_option("graph", 0)
    ctx.set_option("dev_select", _lib.DEV_PWX_OFF | _lib.DEV_CHAIN_OFF)      # the block's neighbours as plain launches in both
    return ctx


def _form(shape, c1, cmid, n, G, B, acts, up):
    dk, ds = shape[2], shape[3]
    got = (C.c_int32 * 7)()
    Gi = G * ds
    f = _lib.load().yl_query_ir_form(c1, cmid, n, dk, ds, G, G, B, Gi, Gi, Gi // 2 if up else 0, Gi // 2 if up else 0, acts[2], acts[1],
                                     acts[0], got)
    return f, tuple(got)


def _check(shape, chans, G, acts, res, up, want_form):
    c1, cmid, n = chans
    if up:
        # the stand-alone lateral conv adds the coarser level behind its activation, the fused block in front of the expansion's:
        # the two agree, and the program builder fuses, only where the expansion has none
        acts = (NONE,) + tuple(acts[1:])
    dk, ds = shape[2], shape[3]
    assert _lib.load().yl_query_fused_block(c1, cmid, n, dk, ds, G, G) == 1
    fused, two = (_ctx_of(p) for p in _programs(c1, cmid, n, dk, ds, G, acts, res, up))
    for B in (1, 3):
        assert _form(shape, c1, cmid, n, G, B, acts, up) == (want_form, shape)
        x = _x(B, 2 * G * ds, seed=17 + B).to(DEV)
        a = fused.forward(x)[0].clone()
        r = two.forward(x)[0].clone()
        torch.cuda.synchronize()
        assert torch.isfinite(a).all()
        assert torch.equal(a, r), (B, (a - r).abs().max().item())


@pytest.mark.parametrize("acts", [(RELU6, RELU6, RELU6), (NONE, NONE, NONE)], ids=["relu6", "none"])
@pytest.mark.parametrize("tiles", [1, 2, 3])
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "x".join(map(str, s[:5])))
def test_ir_second_form_is_bitwise_the_two_launches(shape, tiles, acts):
    """every instantiation at 1, 2 and 3 tile widths of grid; the lateral instantiations with the coarser level's addend"""
    G = tiles * 4 * shape[4] * shape[6]
    _check(shape, SHAPES[shape], G, acts, res=False, up=shape in LATERAL, want_form=2)


TAILS = [((3, 3, 3, 1, 1, 2, 2), (36, 40, 36)), ((2, 3, 5, 2, 1, 2, 2), (20, 40, 36)), ((2, 2, 3, 1, 2, 2, 2), (20, 40, 20)),
         ((1, 2, 3, 2, 1, 2, 2), (12, 40, 20)), ((3, 3, 5, 1, 2, 2, 2), (48, 288, 48)), ((3, 3, 3, 1, 1, 2, 2), (48, 96, 48))]
# a residual has the block's output grid and is made from its input grid here: stride-1 blocks only
TAIL_CASES = [(s, c, r) for s, c in TAILS for r in (False, True) if not (r and s[3] != 1)]


@pytest.mark.parametrize("acts", [(RELU6, RELU6, RELU6), (NONE, NONE, NONE), (RELU, RELU6, NONE)], ids=["relu6", "none", "mixed"])
@pytest.mark.parametrize("shape,chans,res", TAIL_CASES,
                         ids=["x".join(map(str, s[:5])) + "-" + "-".join(map(str, c)) + ("-res" if r else "") for s, c, r in TAIL_CASES])
def test_ir_second_form_channel_tails_and_residual(shape, chans, res, acts):
    """Cmid = 40 (a tail in the last slab), C1 = 36 / 20 / 12 (a tail inside the last input k-block), N = 36 / 20 (below the
    bucket's top), and full channels; with and without the residual: added in front of the accumulation when the projection
    has no activation, behind the activation otherwise.  Two tiles each way"""
    _check(shape, chans, 2 * 4 * shape[4] * shape[6], acts, res=res, up=False, want_form=2)


@pytest.mark.parametrize("acts", [(RELU6, RELU6, RELU6), (NONE, NONE, RELU)], ids=["relu6", "fpn"])
@pytest.mark.parametrize("up", [True, False])
@pytest.mark.parametrize("shape", sorted(LATERAL), ids=lambda s: "x".join(map(str, s[:5])))
def test_ir_second_form_lateral_with_channel_tail(shape, up, acts):
    """the lateral + smooth pair with 72 channels (a tail in the last slab of the addend; 5 of the bucket's 6 n-tiles), the
    addend half the size, and the same block without an addend"""
    _check(shape, (SHAPES[shape][0], 72, 72), 2 * 4 * shape[4] * shape[6], acts, res=False, up=up, want_form=2)


SILU_ACTS = {"silu": (SILU, SILU, SILU), "dw-silu": (RELU6, SILU, NONE), "proj-silu": (RELU6, RELU6, SILU)}
# the lateral + smooth pair only with SiLU on the depthwise conv: with a SiLU projection the kernel's generic epilogue would read
# the layer's `up` tensor as an addend of the OUTPUT (it is the 1x1 layers' epilogue), which the fused pair does not have
SILU_CASES = [(s, k) for s in [(3, 3, 3, 1, 1, 2, 2), (3, 3, 5, 1, 2, 2, 2)] for k in SILU_ACTS] + [((2, 6, 3, 1, 2, 2, 2), "dw-silu")]


@pytest.mark.parametrize("shape,acts", SILU_CASES, ids=["x".join(map(str, s[:5])) + "-" + k for s, k in SILU_CASES])
def test_ir_first_form_takes_silu(shape, acts):
    """SiLU on any of the three sites keeps the first form (one case per depthwise size with SiLU on all three)"""
    _check(shape, SHAPES[shape], 2 * 4 * shape[4] * shape[6], SILU_ACTS[acts], res=shape[3] == 1 and shape not in LATERAL,
           up=shape in LATERAL, want_form=1)
