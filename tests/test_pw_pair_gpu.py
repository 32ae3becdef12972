"""Two plain 1x1 convs around a tensor nothing else reads run as ONE launch that never writes it (yl_conv_pwx_kernel; edge_n's
backbone tail: blocks.4.0.conv 64 -> 480 + lateral5 480 -> 96, C5 not written).  The launch is bitwise the two launches it
replaces ("dev_select" DEV_PWX_OFF), and it does run: the context's read-only "pwx_launches" count grows only with the form on."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bench
from yololite_amd import _lib
from yololite_amd.program import synth_state_dict, zoo_meta

from test_gpu_parity import DEV, _hip_for, _x
from test_chained_expansion_gpu import _assert_same, _forward_and_predict


def _both(ctx, run):
    """run(ctx) with the pair form on, then off; returns (on, off, pair launches enqueued in each)"""
    out = []
    for dev in (0, _lib.DEV_PWX_OFF):
        ctx.set_option("dev_select", dev)
        n0 = ctx.get_option("pwx_launches")
        r = run(ctx)
        torch.cuda.synchronize()
        out.append((r, ctx.get_option("pwx_launches") - n0))
    ctx.set_option("dev_select", 0)
    return out[0][0], out[1][0], out[0][1], out[1][1]


def _pair_program(G, second_reader=False):
    """stem -> 1x1 feed (32 -> 64) -> [1x1 64 -> 480 + ReLU] -> [1x1 480 -> 96, bias, no activation] -> head: one pair on a
    G x G grid.  second_reader: a further 1x1 reads the 480-channel tensor into a second head level."""
    from yololite_amd.program import Layer, Program
    rng = np.random.RandomState(1000 + G + (7 if second_reader else 0))

    def w(*shape):
        return (rng.randn(*shape) / np.sqrt(int(np.prod(shape[1:])))).astype(np.float32)

    def b(n):
        return (rng.randn(n) * 0.1).astype(np.float32)

    L = [Layer(_lib.OP_STEM, -1, 0, 3, 32, 3, 2, 1, 1, 0, w(32, 3, 3, 3), b(32), name="stem"),
         Layer(_lib.OP_CONV, 0, 1, 32, 64, 1, 1, 0, 0, 1, w(64, 32, 1, 1), b(64), name="feed"),
         Layer(_lib.OP_CONV, 1, 2, 64, 480, 1, 1, 0, 0, 1, w(480, 64, 1, 1), b(480), name="c5"),
         Layer(_lib.OP_CONV, 2, 3, 480, 96, 1, 1, 0, 0, 0, w(96, 480, 1, 1), b(96), name="lateral"),
         Layer(_lib.OP_CONV, 3, -1, 96, 6, 1, 1, 0, 0, 0, w(6, 96, 1, 1), b(6), head_level=0, name="out")]
    levels = 1
    if second_reader:
        L.append(Layer(_lib.OP_CONV, 2, -1, 480, 6, 1, 1, 0, 0, 0, w(6, 480, 1, 1), b(6), head_level=1, name="out2"))
        levels = 2
    return Program(img_size=2 * G, num_classes=1, level_size=[G] * levels, level_anchors=[1] * levels, strides=[2] * levels,
                   layers=L, slots=[(G, G, 32), (G, G, 64), (G, G, 480), (G, G, 96)])


def _ctx_of(p):
    from yololite_amd.model import HipContext
    ctx = HipContext(p.img_size, p.num_classes, p.level_size, p.level_anchors, p, 0)
    ctx.set_option("streams", 1)
    ctx.set_option("graph", 0)
    return ctx


@pytest.mark.parametrize("G,B", [(20, 3), (10, 3), (4, 1)])
def test_pw_pair_one_kernel_network(G, B):
    """1200 pixels = 75 full m-tiles; 300 pixels: the last m-tile is partial; 16 pixels: one m-tile, fewer items than
    workgroups.  The head output bitwise the two launches', one pair launch per forward."""
    p = _pair_program(G)
    ctx = _ctx_of(p)
    x = _x(B, p.img_size, seed=17).to(DEV)
    on, off, n_on, n_off = _both(ctx, lambda c: c.forward(x)[0].clone())
    assert (n_on, n_off) == (1, 0)
    assert torch.isfinite(on).all()
    assert torch.equal(on, off)


def test_pw_pair_is_not_taken_with_a_second_reader():
    """The 480-channel tensor has another reader: it must be written, so the two launches run whatever the switch says."""
    p = _pair_program(20, second_reader=True)
    ctx = _ctx_of(p)
    x = _x(3, p.img_size, seed=17).to(DEV)
    on, off, n_on, n_off = _both(ctx, lambda c: [t.clone() for t in c.forward(x)])
    assert (n_on, n_off) == (0, 0)
    assert len(on) == len(off) == 2
    for u, v in zip(on, off):
        assert torch.isfinite(u).all()
        assert torch.equal(u, v)


@pytest.mark.parametrize("S,B", [(640, 2), (320, 3), (384, 3)])
def test_edge_n_pw_pair_is_bitwise_the_two_launches(S, B):
    """Raw levels of a forward and the predict rows, pair form on vs off: 20x20, 10x10 (300 pixels: partial last m-tile) and
    12x12 grids; one pair launch per forward and one per predict."""
    meta = zoo_meta("edge_n", 80, S)
    model = _hip_for(meta, synth_state_dict(meta, seed=2, head_noise=2.0))
    ctx = model._ctx_for(S)
    ctx.set_option("graph", 0)
    ctx.set_option("streams", 1)
    on, off, n_on, n_off = _both(ctx, _forward_and_predict(model, _x(B, S, seed=5).to(DEV)))
    _assert_same(on, off)
    assert (n_on, n_off) == (2, 0)


def test_bench_schedule_pw_pair_is_bitwise_the_two_launches():
    """The benchmark's workload and schedule at a small batch: serving.ServingPipeline with 2 lanes x 1 chunk stream x graph
    replay, pair form on vs off (the lanes are clones: they copy the option as it is when the pipeline is made)."""
    from yololite_amd.serving import ServingPipeline
    B = 4
    wl = bench.build_workload("edge_n", 640, B, seed=1, dev=DEV)
    ctx, x = wl["ctx"], wl["x"]
    res = {}
    for dev in (0, _lib.DEV_PWX_OFF):
        ctx.set_option("dev_select", dev)
        pipe = ServingPipeline(ctx, lanes=2, streams_per_lane=1, graph=True)
        outs = [(torch.empty((B, bench.MAX_OUT, 6), device=DEV), torch.empty((B,), device=DEV, dtype=torch.int32))
                for _ in range(4)]
        got = []
        for i in range(4):
            r = pipe.submit(x, _lib.POST_MAIN, 0.4, 0.5, per_class_cap=300, max_out=bench.MAX_OUT, out=outs[i])
            if r is not None:
                got.append(tuple(t.clone() for t in r))
        got += [tuple(t.clone() for t in r) for r in pipe.flush()]
        torch.cuda.synchronize()
        res[dev] = (got, sum(c.get_option("pwx_launches") for c in pipe.ctxs))
    ctx.set_option("dev_select", 0)
    (g_on, n_on), (g_off, n_off) = res[0], res[_lib.DEV_PWX_OFF]
    assert n_on > 0 and n_off == 0, (n_on, n_off)
    assert len(g_on) == len(g_off) == 4
    for (d0, c0), (d1, c1) in zip(g_on, g_off):
        assert torch.equal(c0, c1)
        for b in range(B):
            assert torch.equal(d0[b, :int(c0[b])], d1[b, :int(c0[b])]), b
