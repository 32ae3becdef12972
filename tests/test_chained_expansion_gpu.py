"""The UIB projection with the next block's 1x1 expansion chained behind it (yl_conv_dwx_kernel, edge_n's 20x20 stage:
blocks.3.1-3.4 pw_proj + blocks.3.2-3.5 pw_exp) is bitwise the two launches it replaces ("dev_select" DEV_CHAIN_OFF), and
it does run: the context's read-only "chain_launches" count grows only when the chaining is on."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bench
from yololite_amd import _lib
from yololite_amd.program import synth_state_dict, zoo_meta

from test_gpu_parity import DEV, _hip_for, _x

CONF, IOU, MO = 0.05, 0.5, 300


def _both(ctx, run, base_dev=0):
    """run(ctx) with the chaining on, then off; returns (on, off, chained launches enqueued in each)"""
    out = []
    for dev in (base_dev, base_dev | _lib.DEV_CHAIN_OFF):
        ctx.set_option("dev_select", dev)
        n0 = ctx.get_option("chain_launches")
        r = run(ctx)
        torch.cuda.synchronize()
        out.append((r, ctx.get_option("chain_launches") - n0))
    ctx.set_option("dev_select", base_dev)
    return out[0][0], out[1][0], out[0][1], out[1][1]


def _forward_and_predict(model, x):
    def run(ctx):
        lv = [t.clone() for t in model(x)]
        d, c = ctx.predict(x, _lib.POST_MAIN, CONF, IOU, per_class_cap=300, max_out=MO)
        return lv, d.clone(), c.clone()
    return run


def _assert_same(a, b):
    (la, da, ca), (lb, db, cb) = a, b
    for l, (u, v) in enumerate(zip(la, lb)):
        assert torch.equal(u, v), f"level {l}"
    assert torch.equal(ca, cb)
    for i in range(ca.shape[0]):
        n = int(ca[i])
        assert torch.equal(da[i, :n], db[i, :n]), f"image {i}"


@pytest.mark.parametrize("S,B", [(640, 2), (640, 64), (384, 3), (320, 3)])
def test_edge_n_chained_expansion_is_bitwise_the_two_launches(S, B):
    """Raw levels of a forward and the predict rows, chaining on vs off.  At 640 / 384 the 20x20 / 12x12 stage runs the
    four chained launches per call; at 320 (10x10: partial 4x4 tiles) the kernel declines and the two launches run."""
    meta = zoo_meta("edge_n", 80, S)
    model = _hip_for(meta, synth_state_dict(meta, seed=2, head_noise=2.0))
    ctx = model._ctx_for(S)
    ctx.set_option("graph", 0)
    ctx.set_option("streams", 1)
    on, off, n_on, n_off = _both(ctx, _forward_and_predict(model, _x(B, S, seed=5).to(DEV)))
    _assert_same(on, off)
    assert n_off == 0
    if (S // 32) % 4 == 0:
        assert n_on == 8, n_on             # 4 pairs, forward + predict
    else:
        assert n_on == 0, n_on


def test_bench_schedule_chained_expansion_is_bitwise_the_two_launches():
    """The benchmark's own workload and schedule: serving.ServingPipeline with 2 lanes x 1 chunk stream x graph replay,
    chaining on vs off (the lanes are clones: they copy the option as it is when the pipeline is made)."""
    from yololite_amd.serving import ServingPipeline
    wl = bench.build_workload("edge_n", 640, 64, seed=1, dev=DEV)
    ctx, x = wl["ctx"], wl["x"]
    res = {}
    for dev in (0, _lib.DEV_CHAIN_OFF):
        ctx.set_option("dev_select", dev)
        pipe = ServingPipeline(ctx, lanes=2, streams_per_lane=1, graph=True)
        outs = [(torch.empty((64, bench.MAX_OUT, 6), device=DEV), torch.empty((64,), device=DEV, dtype=torch.int32))
                for _ in range(4)]
        got = []
        for i in range(4):
            r = pipe.submit(x, _lib.POST_MAIN, 0.4, 0.5, per_class_cap=300, max_out=bench.MAX_OUT, out=outs[i])
            if r is not None:
                got.append(tuple(t.clone() for t in r))
        got += [tuple(t.clone() for t in r) for r in pipe.flush()]
        torch.cuda.synchronize()
        res[dev] = (got, sum(c.get_option("chain_launches") for c in pipe.ctxs))
    ctx.set_option("dev_select", 0)
    (g_on, n_on), (g_off, n_off) = res[0], res[_lib.DEV_CHAIN_OFF]
    assert n_on >= 8 and n_off == 0, (n_on, n_off)
    assert len(g_on) == len(g_off) == 4
    for (d0, c0), (d1, c1) in zip(g_on, g_off):
        assert torch.equal(c0, c1)
        assert int(c0.min()) >= 20
        for b in range(64):
            assert torch.equal(d0[b, :int(c0[b])], d1[b, :int(c0[b])]), b


def _pair_program(dk, cx, res):
    """stem -> 1x1 feed (32 -> 256) -> [depthwise dk x dk -> 1x1 256 -> 64 (+ a 64-channel skip of the stem output)] ->
    [1x1 64 -> cx + ReLU] -> head: one chained pair on a 20x20 grid"""
    from yololite_amd.program import Layer, Program
    G = 20
    rng = np.random.RandomState(100 * dk + cx + res)

    def w(*shape):
        return (rng.randn(*shape) / np.sqrt(int(np.prod(shape[1:])))).astype(np.float32)

    def b(n):
        return (rng.randn(n) * 0.1).astype(np.float32)

    L = [Layer(_lib.OP_STEM, -1, 0, 3, 32, 3, 2, 1, 1, 0, w(32, 3, 3, 3), b(32), name="stem"),
         Layer(_lib.OP_CONV, 0, 1, 32, 256, 1, 1, 0, 0, 1, w(256, 32, 1, 1), b(256), name="feed"),
         Layer(_lib.OP_CONV, 0, 2, 32, 64, 1, 1, 0, 0, 0, w(64, 32, 1, 1), b(64), name="skip"),
         Layer(_lib.OP_CONV, 1, 3, 256, 64, 1, 1, 0, 0, 0, w(64, 256, 1, 1), b(64), dw_k=dk, dw_stride=1, dw_pad_t=dk // 2,
               dw_pad_l=dk // 2, dw_act=0, dw_w=w(256, 1, dk, dk), dw_b=b(256), res_slot=2 if res else -1, name="proj"),
         Layer(_lib.OP_CONV, 3, 4, 64, cx, 1, 1, 0, 0, 1, w(cx, 64, 1, 1), b(cx), name="exp"),
         Layer(_lib.OP_CONV, 4, -1, cx, 6, 1, 1, 0, 0, 0, w(6, cx, 1, 1), b(6), head_level=0, name="out")]
    return Program(img_size=2 * G, num_classes=1, level_size=[G], level_anchors=[1], strides=[2], layers=L,
                   slots=[(G, G, 32), (G, G, 256), (G, G, 64), (G, G, 64), (G, G, cx)])


@pytest.mark.parametrize("dk,cx,res", [(5, 256, False), (3, 192, False), (5, 192, True), (3, 256, True)])
def test_chained_pair_one_kernel_network(dk, cx, res):
    """Each instantiated shape on its own, with and without the projection's residual (edge_n's pairs all carry one):
    the head output bitwise the two launches', one chained launch per forward."""
    from yololite_amd.model import HipContext
    p = _pair_program(dk, cx, res)
    ctx = HipContext(p.img_size, p.num_classes, p.level_size, p.level_anchors, p, 0)
    ctx.set_option("streams", 1)
    ctx.set_option("graph", 0)
    x = _x(3, p.img_size, seed=17).to(DEV)
    on, off, n_on, n_off = _both(ctx, lambda c: c.forward(x)[0].clone())
    assert (n_on, n_off) == (1, 0)
    assert torch.isfinite(on).all()
    assert torch.equal(on, off)
