"""The fused head launch's objectness skip (yl_conv_dpw_kernel<.., SKIP>): a 4x4 tile none of whose candidates has
sigmoid(objectness) > conf gets score -inf and neither class GEMM nor class scan.  The detections are bitwise those of the
full form ("dev_select" DEV_HEAD_SKIP_OFF) at every threshold and post mode, with poisoned workspaces, NaN images and in
the benchmark's schedule; the skip does happen (device counter "head_skipped_tiles" between two host-computed bounds) and
only in launches that decode for yl_predict ("head_skip_launches").

Model: edge_n with the benchmark's calibrated head at the test's size (bench.build_workload)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bench
from yololite_amd import _lib

from test_gpu_parity import DEV, _x

IOU = 0.5
CONFS = [0.001, 0.05, 0.4, 0.9]
SIZES = [(384, 3, 1), (256, 3, 2)]            # (S, B, seed): 384 -> grids 48 / 24 / 12 = 567 tiles per image set, not a multiple of 8
OFF = _lib.DEV_HEAD_SKIP_OFF


@functools.lru_cache(maxsize=None)
def _workload(S, B, seed):
    wl = bench.build_workload("edge_n", S, B, seed=seed, dev=DEV)
    ctx = wl["ctx"]
    ctx.set_option("graph", 0)
    ctx.set_option("streams", 1)
    return wl


def _predict(ctx, x, mode, conf):
    if mode == _lib.POST_FALLBACK:
        r = ctx.predict(x, mode, conf, 0.45, per_class_cap=300, topk=50, want_idx=True)
    elif mode == _lib.POST_EVAL:
        r = ctx.predict(x, mode, conf, 0.65, per_class_cap=0, want_idx=True)
    else:
        r = ctx.predict(x, mode, conf, IOU, per_class_cap=300, max_out=300, want_idx=True)
    torch.cuda.synchronize()
    return tuple(t.clone() for t in r)


def _same(a, b):
    (da, ca, ia), (db, cb, ib) = a, b
    assert torch.equal(ca, cb)
    for i in range(ca.shape[0]):
        n = min(int(ca[i]), da.shape[1])
        assert torch.equal(da[i, :n], db[i, :n]), f"image {i}"
        assert torch.equal(ia[i, :n], ib[i, :n]), f"image {i} indices"


def _on_off(ctx, run, base=0):
    out = []
    for dev in (base, base | OFF):
        ctx.set_option("dev_select", dev)
        out.append(run())
    ctx.set_option("dev_select", 0)
    return out


# ---------------------------------------------------------------------------------------------- 1: bitwise on / off
@pytest.mark.parametrize("S,B,seed", SIZES)
@pytest.mark.parametrize("mode,conf", [(_lib.POST_MAIN, c) for c in CONFS] + [(_lib.POST_EVAL, c) for c in CONFS] +
                         [(_lib.POST_FALLBACK, 0.4)])
def test_skip_form_is_bitwise_the_full_form(S, B, seed, mode, conf):
    wl = _workload(S, B, seed)
    on, off = _on_off(wl["ctx"], lambda: _predict(wl["ctx"], wl["x"], mode, conf))
    _same(on, off)
    if conf <= 0.4 and mode != _lib.POST_FALLBACK:
        assert int(on[1].sum()) > 0                                   # the comparison is not one of empty results


# ---------------------------------------------------------------------------------------------- 2: the skip happens
def _tile_bounds(levels, conf):
    """(tiles, lower, upper): 4x4 tiles of the raw levels whose 16 objectness sigmoids all lie < conf - 1e-4 / <= conf + 1e-4"""
    tiles = lo = hi = 0
    for lv in levels:
        o = lv[..., 4].double().cpu().numpy()                        # [B, A, S, S]
        sg = 1.0 / (1.0 + np.exp(-o))
        Bn, A, S, _ = sg.shape
        m = sg.reshape(Bn, A, S // 4, 4, S // 4, 4).max(axis=(3, 5))
        tiles += m.size
        lo += int((m < conf - 1e-4).sum())
        hi += int((m <= conf + 1e-4).sum())
    return tiles, lo, hi


@pytest.mark.parametrize("S,B,seed", SIZES)
def test_skipped_tiles_lie_between_the_host_bounds(S, B, seed):
    wl = _workload(S, B, seed)
    ctx, x, model = wl["ctx"], wl["x"], wl["model"]
    ctx.set_option("head_skip_count", 1)
    try:
        n0 = ctx.get_option("head_skip_launches")
        levels = [t.clone() for t in model(x)]                        # forward only
        ctx.forward_decoded(x)
        torch.cuda.synchronize()
        assert ctx.get_option("head_skip_launches") == n0            # neither uses the skip form
        for conf in CONFS:
            tiles, lo, hi = _tile_bounds(levels, conf)
            for dev in (0, OFF):
                ctx.set_option("dev_select", dev)
                l0, t0 = ctx.get_option("head_skip_launches"), ctx.get_option("head_skipped_tiles")
                _predict(ctx, x, _lib.POST_MAIN, conf)
                dl, dt = ctx.get_option("head_skip_launches") - l0, ctx.get_option("head_skipped_tiles") - t0
                print(f"S {S} conf {conf} dev {dev}: tiles {tiles} bounds [{lo}, {hi}] skipped {dt} skip-form launches {dl}")
                if dev == OFF:
                    assert (dl, dt) == (0, 0)
                    continue
                assert dl == 1                                        # the three levels are one head launch (streams 1: one chunk)
                assert lo <= dt <= hi, (conf, lo, dt, hi)
                if conf == 0.4:
                    assert 2 * lo >= tiles, (lo, tiles)
                if conf == 0.001:
                    assert dt == 0
    finally:
        ctx.set_option("dev_select", 0)
        ctx.set_option("head_skip_count", 0)


# ---------------------------------------------------------------------------------------------- 3: workspace independence
@pytest.mark.parametrize("S,B,seed", SIZES)
def test_poisoned_workspace_skip_equals_the_clean_run(S, B, seed):
    """Skipped tiles leave their boxes unwritten: with the workspaces refilled with NaN before every call (DEV_POISON), on
    both sides, and on a second call with other images, the rows are the clean run's."""
    wl = _workload(S, B, seed)
    ctx = wl["ctx"]
    for x in (wl["x"], _x(B, S, seed=77).to(DEV)):
        ctx.set_option("dev_select", 0)
        clean = _predict(ctx, x, _lib.POST_MAIN, 0.4)
        on, off = _on_off(ctx, lambda: _predict(ctx, x, _lib.POST_MAIN, 0.4), base=_lib.DEV_POISON)
        _same(on, clean)
        _same(off, clean)


# ---------------------------------------------------------------------------------------------- 4: the benchmark's schedule
def test_bench_schedule_skip_form_is_bitwise_the_full_form():
    """The benchmark's own workload and schedule: serving.ServingPipeline with 2 lanes x 1 chunk stream x graph replay
    (the lanes are clones: they copy the option as it is when the pipeline is made)."""
    from yololite_amd.serving import ServingPipeline
    wl = bench.build_workload("edge_n", 640, 64, seed=1, dev=DEV)
    ctx, x = wl["ctx"], wl["x"]
    res = {}
    for dev in (0, OFF):
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
        res[dev] = (got, sum(c.get_option("head_skip_launches") for c in pipe.ctxs))
    ctx.set_option("dev_select", 0)
    (g_on, n_on), (g_off, n_off) = res[0], res[OFF]
    assert n_on >= 2 and n_off == 0, (n_on, n_off)
    assert len(g_on) == len(g_off) == 4
    for (d0, c0), (d1, c1) in zip(g_on, g_off):
        assert torch.equal(c0, c1)
        assert int(c0.min()) >= 20
        for b in range(64):
            assert torch.equal(d0[b, :int(c0[b])], d1[b, :int(c0[b])]), b


# ---------------------------------------------------------------------------------------------- 5: conf <= 0 and NaN
@pytest.mark.parametrize("conf", [0.4, -1.0])
def test_nan_image_and_non_positive_threshold(conf):
    """Image 1 all NaN.  conf 0.4: wherever its objectness is NaN the tile is skipped (NaN compares false) and the full form's
    NaN score does not pass the NMS either; conf -1: nothing is skipped and every finite score passes."""
    S, B, seed = SIZES[0]
    wl = _workload(S, B, seed)
    x = wl["x"].clone()
    x[1] = float("nan")
    on, off = _on_off(wl["ctx"], lambda: _predict(wl["ctx"], x, _lib.POST_MAIN, conf))
    _same(on, off)
    assert int(on[1][0]) > 0 and int(on[1][2]) > 0
