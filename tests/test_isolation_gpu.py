"""Isolation: a call's results depend only on its own images and the options in force -- not on the other images of the
batch, not on what earlier calls left in the context's buffers, not on which cached graph is replayed.

The rest of the suite feeds finite images into zero-initialised arenas.  Here the workspace is filled with NaN before
every call ("dev_select" YL_DEV_POISON: 0xFF bytes, a NaN in fp32 and fp16) and batches carry NaN / inf images, and the
results must stay bitwise those of the clean run.  The poisoned workspace guards against a result that depends on bytes
no producer of this call wrote; it cannot see a channel-tail read (a lane of a tensor's last, partial 16-channel k-block
loading the next pixel's channels): the buffer-descriptor kernels' range check returns zeros past a tensor's end, and
inside a tensor every byte is written before its consumer runs -- no poisoned case failed on kernels without the tail
masks.  Tail reads are caught by the non-finite images, above all by the one-kernel networks of KERNEL_TARGETS (each
target layer has Cin % 16 == 8, or 4): removing any one kernel's tail mask fails its test.

Which configuration reaches which kernel: measured, `rocprofv3 --kernel-trace` of one forward + predict per configuration
and mode (tools/kernel_map.py; the *_bf16 / *_f16 / *_f16s builds of the same kernels in the other modes):

  edge_n 640              yl_stemblock, yl_conv_s2c, yl_conv_dpq, yl_conv_dwt, yl_conv_dwh, yl_ir, yl_conv_pwt, yl_conv_mfma,
                          yl_conv_dpw (fused head)
  edge_n 640 DPW_OFF      yl_conv_dpp
  edge_m + seg 320        yl_conv_dwk, yl_conv_dwt, yl_conv_dwh, yl_conv_wino2, yl_dw_tile, yl_conv_mfma, mask kernels
  yololite_m 256 / 224    yl_stemdw, yl_conv_dws (256), yl_conv_dwk, yl_conv_dwt, yl_ir, yl_conv_wino2, yl_dw_tile (224)
  yololite_m_v2 256       yl_stem_mfma, yl_conv_wino (Cin 56 expand convs), yl_conv_wino2, yl_conv_dwk, squeeze-excite
                          (yl_se_gate; yl_se_pool in the MFMA modes), yl_dw_tile
  yololite_m_v2 640 wino0 yl_conv_k3w (K3W_OFF: yl_conv_kxk)
  yololite_n 320          F = 196 neck (Cin % 16 == 4): yl_conv_dws, yl_conv_dwt, yl_ir, yl_conv_wino / wino2
  tiny 0..3 at 96         yl_stemblock / yl_stem_mfma, yl_conv_dwt, yl_conv_wino (tiny2, tiny3), yl_conv_pwt, yl_conv_mfma
  tiny4 (v2) at 96        yl_conv_wino, yl_dw_tile, yl_se_gate (yl_se_pool with bf16)
  tiny5 (hg), tiny6 (cnx) yl_ops.hip: yl_nhwc4, yl_pool, yl_copy, yl_act, yl_ln, yl_grn_sumsq / yl_grn_gate, yl_dw
  edge_n 320 tile_m 6     yl_conv_dwh, yl_conv_mfma (kxk / wino / wave-autonomous kernels off)
  edge_n 320 tile_m 7     yl_conv_dwc (DWC_ALL)
  edge_m 320 DWL_ALL      yl_conv_dwl;  DWL_OFF: yl_conv_dwk
  yololite_m WINO_V1      yl_conv_wino;  winograd 0: yl_conv_kxk
  yololite_m DW_TILE_OFF  the yololite_m 256 set (no stand-alone depthwise layer at 256: the switch selects nothing there)
yl_uib_kernel is not reached by any of these (the program builder prefers the other fused forms at these shapes); its
bitwise test is test_uib_and_lateral_fusion_through_the_ir_kernel_is_bitwise.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from yololite_amd import _lib
from yololite_amd.program import MODEL_ZOO, make_meta, synth_state_dict, zoo_meta
from yololite_amd.serving import ServingPipeline

from test_gpu_parity import DEV, TINY, _hip_for, _x

# ---------------------------------------------------------------------------------------------- configurations
# id -> (meta factory, input size, batch, context options)
CFG = {
    "edge_n_640": (lambda: zoo_meta("edge_n", 80, 640), 640, 3, {}),
    "edge_m_seg_320": (lambda: make_meta(num_classes=80, img_size=320, seg=True, **MODEL_ZOO["edge_m"]), 320, 2, {}),
    "yololite_m_256": (lambda: zoo_meta("yololite_m", 80, 256), 256, 2, {}),
    "yololite_m_224": (lambda: zoo_meta("yololite_m", 80, 224), 224, 2, {}),
    "yololite_m_v2_256": (lambda: zoo_meta("yololite_m_v2", 80, 256), 256, 2, {}),
    "yololite_m_v2_640_k3w": (lambda: zoo_meta("yololite_m_v2", 80, 640), 640, 1, {"winograd": 0}),
    "yololite_n_320_f196": (lambda: zoo_meta("yololite_n", 80, 320), 320, 3, {}),
    "edge_n_320_tile6": (lambda: zoo_meta("edge_n", 80, 320), 320, 3, {"tile_m": 6, "winograd": 0}),
    "edge_n_320_dwc": (lambda: zoo_meta("edge_n", 80, 320), 320, 3, {"tile_m": 7, "dev_select": _lib.DEV_DWC_ALL}),
    "edge_m_320_dwl_all": (lambda: zoo_meta("edge_m", 80, 320), 320, 2, {"dev_select": _lib.DEV_DWL_ALL}),
    "edge_m_320_dwl_off": (lambda: zoo_meta("edge_m", 80, 320), 320, 2, {"dev_select": _lib.DEV_DWL_OFF}),
    "yololite_m_256_wino_v1": (lambda: zoo_meta("yololite_m", 80, 256), 256, 2, {"dev_select": _lib.DEV_WINO_V1}),
    "yololite_m_256_wino0": (lambda: zoo_meta("yololite_m", 80, 256), 256, 2, {"winograd": 0}),
    "edge_n_320_dpw_off": (lambda: zoo_meta("edge_n", 80, 320), 320, 3, {"dev_select": _lib.DEV_DPW_OFF}),
    "yololite_m_v2_640_k3w_off": (lambda: zoo_meta("yololite_m_v2", 80, 640), 640, 1, {"winograd": 0, "dev_select": _lib.DEV_K3W_OFF}),
    "edge_n_640_dpw_off": (lambda: zoo_meta("edge_n", 80, 640), 640, 2, {"dev_select": _lib.DEV_DPW_OFF}),
    "yololite_m_256_dw_tile_off": (lambda: zoo_meta("yololite_m", 80, 256), 256, 2, {"dev_select": _lib.DEV_DW_TILE_OFF}),
}
for _i, _t in enumerate(TINY):
    CFG[f"tiny{_i}_{_t['backbone']}"] = ((lambda t=_t: make_meta(img_size=96, **t)), 96, 3, {})
MODEL_KW = {}                                       # model build options of a configuration (none at present)

MODES = {"fp32": {}, "store_f16": {"store_f16": 1}, "mfma_bf16": {"mfma_bf16": 1}, "mfma_f16": {"mfma_f16": 1}}
SCHED = {
    "eager": {"graph": 0, "streams": 1},
    "graph": {"graph": 1, "streams": 2},
    "hybrid": {"graph": 0, "streams": 2, "hybrid": 1},
    "lanes": {"graph": 0, "streams": 2, "lanes": 1},
    # one buffer per tensor ("reuse_slots" 0): another arena layout under the poison
    "noreuse": {"graph": 0, "streams": 1, "reuse_slots": 0},
}
_FP16_REFUSED = ("tiny5_oracle_tiny_hg", "tiny6_oracle_tiny_cnx")        # store_f16 refuses the hgnetv2 / convnextv2 ops

# every configuration in fp32 eager; the reduced-precision modes and the other schedules on a subset that still reaches
# every kernel family of each compilation (about 3 GPU-minutes for the whole file)
CASES = [(c, "fp32", "eager") for c in CFG] + [(c, "fp32", "noreuse") for c in CFG] + [
    ("edge_n_640", "store_f16", "graph"), ("edge_n_640", "mfma_bf16", "eager"),
    ("edge_m_seg_320", "store_f16", "eager"), ("edge_m_seg_320", "mfma_f16", "graph"), ("edge_m_seg_320", "fp32", "lanes"),
    ("yololite_m_256", "store_f16", "eager"), ("yololite_m_256", "mfma_bf16", "hybrid"), ("yololite_m_256", "fp32", "graph"),
    ("yololite_m_v2_256", "mfma_f16", "eager"), ("yololite_m_v2_256", "store_f16", "lanes"),
    ("yololite_n_320_f196", "store_f16", "eager"), ("yololite_n_320_f196", "mfma_f16", "hybrid"),
    ("tiny0_oracle_tiny", "store_f16", "eager"), ("tiny3_oracle_tiny_tf", "store_f16", "graph"),
    ("tiny4_oracle_tiny_v2", "mfma_bf16", "eager"), ("tiny1_oracle_tiny", "mfma_f16", "lanes"),
    ("edge_n_320_dwc", "store_f16", "noreuse"), ("yololite_m_256_wino_v1", "mfma_bf16", "noreuse"),
    ("edge_m_seg_320", "store_f16", "noreuse"), ("yololite_m_256", "mfma_f16", "noreuse"), ("edge_n_640", "mfma_f16", "noreuse"),
]
# the non-finite-image test needs images whose activations reach the channel tails: the same cases, fewer fp32 repeats
CASES_NF = [c for c in CASES if c[2] != "noreuse"]

_models = {}


def _model(cid):
    if cid not in _models:
        make, S, B, opts = CFG[cid]
        meta = make()
        sd = synth_state_dict(meta, seed=3, head_noise=2.0)
        _models[cid] = (_hip_for(meta, sd, **MODEL_KW.get(cid, {})), meta)
    return _models[cid][0]


def _configure(ctx, cid, mode, sched, poison=False):
    opts = {"graph": 0, "streams": 2, "hybrid": 0, "lanes": 0, "reuse_slots": 1, "tile_m": 0, "winograd": 1, "dev_select": 0,
            "store_f16": 0, "mfma_bf16": 0, "mfma_f16": 0}
    opts.update(CFG[cid][3])
    opts.update(MODES[mode])
    opts.update(SCHED[sched])
    if poison:
        opts["dev_select"] |= _lib.DEV_POISON
    for k in ("store_f16", "mfma_bf16", "mfma_f16"):        # at most one reduced-precision mode on: clear first
        if not opts[k]:
            ctx.set_option(k, 0)
    for k, v in opts.items():
        ctx.set_option(k, v)


def _skip_refused(cid, mode):
    if mode == "store_f16" and cid in _FP16_REFUSED:
        pytest.skip("store_f16 refuses the hgnetv2 / convnextv2 element-wise ops (tested in test_gpu_parity)")


def _run_all(m, ctx, x):
    """levels, prototypes (seg), detections + counts + kept indices, masks (seg) of one batch: cloned to the host."""
    out = m(x)
    seg = bool(ctx.NM)
    lv = [t.cpu() for t in (out[0] if seg else out)]
    pr = out[1].cpu() if seg else None
    d, c, idx = ctx.predict(x, _lib.POST_MAIN, 0.01, 0.5, per_class_cap=300, max_out=256, want_idx=True)
    mk = ctx.masks(c, idx, 256).cpu() if seg else None
    mi = [t.cpu() for t in ctx.masks_image(d, c, idx)] if seg else None
    return dict(levels=lv, proto=pr, dets=d.cpu(), counts=c.cpu(), masks=mk, masks_image=mi)


def _assert_rows_equal(a, b, rows, what):
    for l, (u, v) in enumerate(zip(a["levels"], b["levels"])):
        for r in rows:
            assert torch.equal(u[r[0]], v[r[1]]), f"{what}: level {l} image {r}"
    for r in rows:
        ca, cb = int(a["counts"][r[0]]), int(b["counts"][r[1]])
        assert ca == cb, f"{what}: counts of image {r}: {ca} != {cb}"
        n = min(ca, a["dets"].shape[1])
        assert torch.equal(a["dets"][r[0], :n], b["dets"][r[1], :n]), f"{what}: detections of image {r}"
        if a["proto"] is not None:
            assert torch.equal(a["proto"][r[0]], b["proto"][r[1]]), f"{what}: prototypes of image {r}"


def _assert_equal(a, b, what):
    B = a["counts"].shape[0]
    _assert_rows_equal(a, b, [(i, i) for i in range(B)], what)
    if a["masks"] is not None:
        assert torch.equal(a["masks"], b["masks"]), f"{what}: masks"
        for i, (u, v) in enumerate(zip(a["masks_image"], b["masks_image"])):
            assert torch.equal(u, v), f"{what}: masks_image of image {i}"


# ---------------------------------------------------------------------------------------------- item: graph key
@pytest.mark.parametrize("streams", [2, 1])
def test_time_split_toggle_never_replays_another_plans_graph(streams):
    """The cached-graph key holds every option in a field of its own.  It used to pack "time_split" into bit 16 of the
    "dev_select" word, where DEV_DPW_OFF lives: with that bit set, time_split 0 and 1 shared a key, and the call after a
    toggle replayed graphs captured for the other segment plan (one chunk + the event split against two chunks)."""
    S, B = 320, 8
    m = _model("edge_n_320_dpw_off")
    ctx = m._ctx_for(S)
    x = _x(B, S, seed=31).to(DEV)
    ctx.set_option("graph", 0); ctx.set_option("streams", streams); ctx.set_option("time_split", 0)
    ctx.set_option("dev_select", _lib.DEV_DPW_OFF)
    want = {}
    for ts in (0, 1):
        ctx.set_option("time_split", ts)
        d, c = ctx.predict(x, _lib.POST_MAIN, 0.02, 0.5, 300)
        want[ts] = (d.cpu(), c.cpu())
    assert int(want[0][1].min()) > 0
    ctx.set_option("time_split", 0)
    ctx.set_option("graph", 1)
    for ts in (0, 1, 0):
        ctx.set_option("time_split", ts)
        d, c = ctx.predict(x, _lib.POST_MAIN, 0.02, 0.5, 300)
        d, c = d.cpu(), c.cpu()
        assert torch.equal(c, want[ts][1]), ts
        for b in range(B):
            assert torch.equal(d[b, :int(c[b])], want[ts][0][b, :int(c[b])]), (ts, b)
        if ts:
            infer_ms, post_ms = ctx.last_timing()
            assert infer_ms > 0 and post_ms > 0
    for k, v in (("time_split", 0), ("graph", 0), ("streams", 2), ("dev_select", 0)):
        ctx.set_option(k, v)


# ---------------------------------------------------------------------------------------------- item: poisoned workspace
@pytest.mark.parametrize("cid,mode,sched", CASES)
def test_poisoned_workspace_is_bitwise_the_clean_run(cid, mode, sched):
    """Workspace filled with NaN before every call (YL_DEV_POISON) against the clean workspace: identical levels,
    detections (and prototypes / masks of seg models) -- no result depends on bytes this call did not write (stale
    arena, level-buffer or squeeze-excite contents).  Channel-tail reads are the business of the non-finite-image tests."""
    _skip_refused(cid, mode)
    m = _model(cid)
    _, S, B, _ = CFG[cid]
    ctx = m._ctx_for(S)
    x = _x(B, S, seed=7).to(DEV)
    _configure(ctx, cid, mode, sched)
    clean = _run_all(m, ctx, x)
    _configure(ctx, cid, mode, sched, poison=True)
    assert ctx.get_option("dev_select") & _lib.DEV_POISON
    dirty = _run_all(m, ctx, x)
    _configure(ctx, cid, "fp32", "eager")
    _assert_equal(clean, dirty, f"{cid} {mode} {sched}")
    for t in clean["levels"]:
        assert torch.isfinite(t).all(), f"{cid} {mode} {sched}: clean levels not finite"


def test_poisoned_workspace_through_serving_pipeline_lanes():
    """Two ServingPipeline lanes on cloned contexts (the clones copy "dev_select"): poisoned lanes hand back the rows
    of a clean plain call."""
    S, B = 320, 6
    m = _model("edge_n_320_dwc")
    ctx = m._ctx_for(S)
    _configure(ctx, "edge_n_320_dwc", "fp32", "eager")
    ctx.set_option("tile_m", 0); ctx.set_option("dev_select", 0)
    xs = [_x(B, S, seed=50 + i).to(DEV) for i in range(4)]
    want = [tuple(t.cpu() for t in ctx.predict(x, _lib.POST_MAIN, 0.02, 0.5, 300)) for x in xs]
    ctx.set_option("dev_select", _lib.DEV_POISON)
    pipe = ServingPipeline(ctx, lanes=2, streams_per_lane=1, graph=True)
    got = []
    for x in xs:
        r = pipe.submit(x, _lib.POST_MAIN, 0.02, 0.5, 300)
        if r is not None:
            got.append((r[0].cpu(), r[1].cpu()))
    got += [(d.cpu(), c.cpu()) for d, c in pipe.flush()]
    ctx.set_option("dev_select", 0)
    assert len(got) == len(xs)
    for (d0, c0), (d1, c1) in zip(want, got):
        assert torch.equal(c0, c1) and int(c0.min()) > 0
        for b in range(B):
            assert torch.equal(d0[b, :int(c0[b])], d1[b, :int(c1[b])])


# ---------------------------------------------------------------------------------------------- item: non-finite images
def _bad_batch(S, mode, seed=11, B=4, swap=False):
    """images 0 and 3 from _x; image 1 all NaN; image 2 all +inf (fp32) or 1e5 (finite in fp32, inf in fp16 storage) --
    images 1 and 2 the other way round with swap (a NaN image turns into zeros behind the first ReLU on the GPU, fmaxf,
    so the image right behind image 0 must also be the inf one).  Also the batch with images 1 and 2 clean."""
    x = _x(B, S, seed=seed)
    clean = x.clone()
    bad = x.clone()
    big = 1e5 if mode == "store_f16" else float("inf")
    bad[1] = big if swap else float("nan")
    bad[2] = float("nan") if swap else big
    return bad.to(DEV), clean.to(DEV)


def _forward_rows(m, ctx, x):
    r = _run_all(m, ctx, x)
    dec = ctx.forward_decoded(x)
    r["decoded"] = {k: v.cpu() for k, v in dec.items()}
    lv = [t.to(DEV) for t in r["levels"]]
    d, c = ctx.postprocess(lv, _lib.POST_MAIN, 0.01, 0.5, 300)
    r["post"] = (d.cpu(), c.cpu())
    return r


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("cid,mode,sched", CASES_NF)
def test_non_finite_image_does_not_reach_its_neighbours(cid, mode, sched, swap):
    """A batch of four whose images 1 and 2 are NaN / inf: images 0 and 3 come out bitwise as in the batch where 1 and 2
    are clean -- through forward, forward_decoded, predict and yl_postprocess on the levels.  (The poisoned images' own
    rows are not compared: the GPU's NaN handling in clamps is not torch's.)"""
    _skip_refused(cid, mode)
    m = _model(cid)
    S = CFG[cid][1]
    ctx = m._ctx_for(S)
    bad, clean = _bad_batch(S, mode, swap=swap)
    _configure(ctx, cid, mode, sched)
    want = _forward_rows(m, ctx, clean)
    got = _forward_rows(m, ctx, bad)
    _configure(ctx, cid, "fp32", "eager")
    what = f"{cid} {mode} {sched}"
    _assert_rows_equal(want, got, [(0, 0), (3, 3)], what)
    for k in want["decoded"]:
        for r in (0, 3):
            assert torch.equal(want["decoded"][k][r], got["decoded"][k][r]), f"{what}: forward_decoded {k} image {r}"
    for r in (0, 3):
        n = int(want["post"][1][r])
        assert int(got["post"][1][r]) == n, f"{what}: postprocess count of image {r}"
        assert torch.equal(want["post"][0][r, :n], got["post"][0][r, :n]), f"{what}: postprocess image {r}"


# ---------------------------------------------------------------------------------------------- item: earlier calls
@pytest.mark.parametrize("cid,sched", [("edge_n_640", "eager"), ("edge_n_640", "graph"), ("edge_m_seg_320", "graph"),
                                       ("yololite_m_256", "eager"), ("yololite_n_320_f196", "graph"),
                                       ("tiny4_oracle_tiny_v2", "eager"), ("tiny6_oracle_tiny_cnx", "graph")])
def test_earlier_calls_leave_no_trace(cid, sched):
    """A call with a NaN / inf batch of five, then a clean batch of three on the same context (re-planned chunks inside
    the existing allocation): bitwise the clean batch on a fresh context.  Eager launches and replayed graphs (the second
    clean call replays what the first captured)."""
    S = CFG[cid][1]
    m = _model(cid)
    ctx = m._ctx_for(S)
    _configure(ctx, cid, "fp32", sched)
    bad, _ = _bad_batch(S, "fp32", B=5)
    x = _x(3, S, seed=23).to(DEV)
    _run_all(m, ctx, bad)
    got = [_run_all(m, ctx, x) for _ in range(2)]
    _configure(ctx, cid, "fp32", "eager")
    make, _, _, _ = CFG[cid]
    meta = make()
    fresh = _hip_for(meta, synth_state_dict(meta, seed=3, head_noise=2.0), **MODEL_KW.get(cid, {}))
    fctx = fresh._ctx_for(S)
    _configure(fctx, cid, "fp32", sched)
    want = _run_all(fresh, fctx, x)
    for g in got:
        _assert_equal(want, g, f"{cid} {sched}")


def test_earlier_calls_leave_no_trace_in_serving_lanes():
    """ServingPipeline lanes: every lane first serves a NaN / inf batch, then clean batches -- the clean batches' rows
    equal a fresh context's."""
    S, B = 320, 5
    m = _model("edge_n_320_dpw_off")
    ctx = m._ctx_for(S)
    _configure(ctx, "edge_n_320_dpw_off", "fp32", "eager")
    ctx.set_option("dev_select", 0)
    bad, _ = _bad_batch(S, "fp32", B=B)
    xs = [_x(B, S, seed=60 + i).to(DEV) for i in range(3)]
    want = [tuple(t.cpu() for t in ctx.predict(x, _lib.POST_MAIN, 0.02, 0.5, 300)) for x in xs]
    pipe = ServingPipeline(ctx, lanes=2, streams_per_lane=1, graph=True)
    got = []
    for x in [bad, bad] + xs:
        r = pipe.submit(x, _lib.POST_MAIN, 0.02, 0.5, 300)
        if r is not None:
            got.append((r[0].cpu(), r[1].cpu()))
    got += [(d.cpu(), c.cpu()) for d, c in pipe.flush()]
    got = got[2:]
    assert len(got) == len(xs)
    for (d0, c0), (d1, c1) in zip(want, got):
        assert torch.equal(c0, c1) and int(c0.min()) > 0
        for b in range(B):
            assert torch.equal(d0[b, :int(c0[b])], d1[b, :int(c1[b])])


# ---------------------------------------------------------------------------------------------- item: one kernel at a time
# A whole network hides a channel-tail read behind its activations (a NaN image turns into zeros at the first ReLU on the
# GPU; an inf one into NaN and then zeros), so every kernel whose tail is masked also gets a network of its own:
#   stem 3x3 s2 (3 -> 32, no activation)  ->  1x1 (32 -> Cin, no activation)  ->  TARGET  ->  1x1 head output (level 0).
# Without activations a non-finite image stays non-finite up to the target layer's input: every pixel of image 1 --
# including the first, which image 0's last pixel reads through an unmasked tail -- is inf or NaN there.  Cin % 16 == 8
# (or 4) in every target.  The kernel each target runs on (`rocprofv3 --kernel-trace`, tools/kernel_map.py):
KERNEL_TARGETS = {
    # name: (target kind, Cin, Cout, dw_k, target grid, context options, kernel)
    "dwt": ("dw", 24, 32, 3, 20, {}, "yl_conv_dwt_kernel"),
    "dwh": ("dw", 24, 32, 3, 20, {"tile_m": 6}, "yl_conv_dwh_kernel"),
    "dwk": ("dw", 200, 384, 3, 40, {"dev_select": _lib.DEV_DWL_OFF}, "yl_conv_dwk_kernel"),
    "dwl": ("dw", 200, 256, 3, 40, {"dev_select": _lib.DEV_DWL_ALL}, "yl_conv_dwl_kernel"),     # 16 / 21 n-tiles only
    "dws": ("dw", 328, 128, 5, 40, {}, "yl_conv_dws_kernel"),
    "wino2": ("k3", 56, 64, 0, 40, {"winograd": 1}, "yl_conv_wino2_kernel"),
    "wino": ("k3", 56, 64, 0, 40, {"winograd": 1, "dev_select": _lib.DEV_WINO_V1}, "yl_conv_wino_kernel"),
    "f196": ("k1", 196, 64, 0, 20, {}, None),          # Cin % 16 == 4 through the plain 1x1 kernels
}


def _kernel_program(name):
    import numpy as np
    from yololite_amd.program import Layer, Program
    kind, cin, cout, dk, G, _, _ = KERNEL_TARGETS[name]
    S = 2 * G
    rng = np.random.RandomState(sum(map(ord, name)))

    def w(*shape):
        fan = int(np.prod(shape[1:]))
        return (rng.randn(*shape) / np.sqrt(fan)).astype(np.float32)

    def b(n):
        return (rng.randn(n) * 0.1).astype(np.float32)

    L = [Layer(_lib.OP_STEM, -1, 0, 3, 32, 3, 2, 1, 1, 0, w(32, 3, 3, 3), b(32), name="stem"),
         Layer(_lib.OP_CONV, 0, 1, 32, cin, 1, 1, 0, 0, 0, w(cin, 32, 1, 1), b(cin), name="feed")]
    if kind == "dw":
        L.append(Layer(_lib.OP_CONV, 1, 2, cin, cout, 1, 1, 0, 0, 0, w(cout, cin, 1, 1), b(cout), dw_k=dk, dw_stride=1,
                       dw_pad_t=dk // 2, dw_pad_l=dk // 2, dw_act=0, dw_w=w(cin, 1, dk, dk), dw_b=b(cin), name="target"))
    elif kind == "k3":
        L.append(Layer(_lib.OP_CONV, 1, 2, cin, cout, 3, 1, 1, 1, 0, w(cout, cin, 3, 3), b(cout), name="target"))
    else:
        L.append(Layer(_lib.OP_CONV, 1, 2, cin, cout, 1, 1, 0, 0, 0, w(cout, cin, 1, 1), b(cout), name="target"))
    L.append(Layer(_lib.OP_CONV, 2, -1, cout, 6, 1, 1, 0, 0, 0, w(6, cout, 1, 1), b(6), head_level=0, name="out"))
    return Program(img_size=S, num_classes=1, level_size=[G], level_anchors=[1], strides=[2], layers=L,
                   slots=[(G, G, 32), (G, G, cin), (G, G, cout)])


def _kernel_context(name, mode="fp32"):
    from yololite_amd.model import HipContext
    p = _kernel_program(name)
    ctx = HipContext(p.img_size, p.num_classes, p.level_size, p.level_anchors, p, 0)
    for k, v in {**KERNEL_TARGETS[name][5], **MODES[mode], "streams": 1}.items():
        ctx.set_option(k, v)
    return ctx, p.img_size


@pytest.mark.parametrize("bad", ["inf", "nan"])
@pytest.mark.parametrize("mode", ["fp32", "store_f16"])
@pytest.mark.parametrize("name", sorted(KERNEL_TARGETS))
def test_masked_channel_tail_kernel_keeps_images_apart(name, mode, bad):
    """Image 1 of three non-finite at the target layer's input: images 0 and 2 bitwise as in the clean batch.  Fails for
    the kernel of KERNEL_TARGETS[name] when its channel-tail mask is removed (image 0's last pixel turns NaN)."""
    ctx, S = _kernel_context(name, mode)
    x = _x(3, S, seed=17).to(DEV)
    y = x.clone()
    y[1] = float(bad) if mode == "fp32" else (1e5 if bad == "inf" else float("nan"))
    want = ctx.forward(x)[0].cpu()
    got = ctx.forward(y)[0].cpu()
    assert torch.isfinite(want).all()
    assert not torch.isfinite(got[1]).all(), "the non-finite image did not reach the head (test does not bite)"
    for r in (0, 2):
        assert torch.equal(want[r], got[r]), f"{name} {mode} {bad}: image {r}"


# ---------------------------------------------------------------------------------------------- item: non-finite logits
_NF_EDITS = [("obj+inf", [(4, float("inf"))]), ("obj-inf", [(4, float("-inf"))]), ("obj-nan", [(4, float("nan"))]),
             ("cls+inf", [(-1, float("inf"))]), ("cls-nan", [(-1, float("nan"))]), ("cls-all-inf", "allcls"),
             ("tw+inf", [(2, float("inf"))]), ("th-inf", [(3, float("-inf"))]), ("tx+inf", [(0, float("inf"))]),
             ("ty-inf", [(1, float("-inf"))])]


def _edit_levels(lv, edit):
    """set entries of the strongest candidate of image 0 and of one fixed cell of every level and image to non-finite
    values (a single row per edit site)"""
    out = [t.clone() for t in lv]
    t0 = out[0]
    sc = torch.sigmoid(t0[0, ..., 4]) * torch.sigmoid(t0[0, ..., 5:]).max(-1).values
    site = list(np.unravel_index(int(torch.argmax(sc)), sc.shape))
    sites = [(0, 0, (0,) + tuple(site))] + [(l, b, (b, 0, 1, 2)) for l in range(len(out)) for b in range(out[0].shape[0])]
    for l, _, idx in sites:
        row = out[l][idx]
        if edit == "allcls":
            row[5:] = float("-inf")
        else:
            for ch, v in edit:
                row[ch if ch >= 0 else 5 + min(1, row.shape[0] - 6)] = v     # -1: the second class (the only one if C == 1)
    return out


@pytest.mark.parametrize("edit", [e[0] for e in _NF_EDITS])
@pytest.mark.parametrize("tag", ["c3", "c3_lowconf", "c1"])
def test_non_finite_logits_match_the_oracle(golden_dir, tag, edit):
    """Golden levels with single non-finite logits (objectness / class / box, +-inf and NaN) through the four
    post-processing paths against the oracle, with the _match tolerances (assert_allclose: NaN only where the oracle has
    NaN); the decode under every centre / size mode."""
    import json, os
    import numpy as np
    import yololite_amd as ya
    from oracle import postproc as opost
    from test_gpu_parity import _match
    z = np.load(os.path.join(golden_dir, "pipelines.npz"))
    with open(os.path.join(golden_dir, "pipelines_cases.json")) as f:
        c = next(c for c in json.load(f) if c["tag"] == tag)
    lv = _edit_levels([torch.from_numpy(z[f"{tag}/level{j}"]) for j in range(3)], dict(_NF_EDITS)[edit])
    dl = [t.to(DEV) for t in lv]
    img, conf, iou = c["img"], c["conf"], c["iou"]
    for cm in ("v8", "simple"):
        for wm in ("softplus", "v8", "exp"):
            d = ya.decode_preds_anchorfree(dl, img, cm, wm)
            e = opost.decode_levels(lv, img, cm, wm)
            np.testing.assert_allclose(d["box"].cpu().numpy(), e["box"].numpy(), rtol=2e-6, atol=2e-5, err_msg=f"{cm} {wm}")
            np.testing.assert_array_equal(d["obj"].cpu().numpy(), e["obj"].numpy())
            np.testing.assert_array_equal(d["cls"].cpu().numpy(), e["cls"].numpy())
    exp = opost.pipeline_main(lv, img, conf, iou, 300)
    got = ya.infer_main_postprocess(dl, img, conf, iou, 300)
    for b in range(c["B"]):
        _match(got["boxes"][b], got["scores"][b], got["classes"][b], exp["boxes"][b], exp["scores"][b], exp["classes"][b])
    edets, _ = opost.pipeline_eval(lv, img, conf, iou)
    gdets = ya._decode_batch_to_coco_dets(dl, img, conf_th=conf, iou_th=iou, add_one=True)
    for g, e in zip(gdets, edets):
        assert [x["category_id"] for x in g] == [x["category_id"] for x in e]
        np.testing.assert_allclose([x["score"] for x in g], [x["score"] for x in e], atol=1e-5)
        np.testing.assert_allclose(np.asarray([x["bbox"] for x in g]).reshape(-1, 4),
                                   np.asarray([x["bbox"] for x in e]).reshape(-1, 4), atol=1e-3)
    exp = opost.pipeline_fallback(lv, img, conf, iou, topk=300, nms_impl="fallback")
    fb = ya.decode_anchorfree_like_train(dl, img, conf_th=conf, iou_th=iou, topk=300, nms_impl="greedy")
    for b in range(c["B"]):
        _match(fb["boxes"][b].cpu().numpy(), fb["scores"][b].cpu().numpy(), fb["classes"][b].cpu().numpy(),
               exp["boxes"][b], exp["scores"][b], exp["classes"][b])


@pytest.mark.parametrize("val", ["inf", "nan"])
@pytest.mark.parametrize("idx", [0, 1, 2])
def test_fused_decode_epilogue_equals_decode_kernel_on_non_finite_class_logits(idx, val):
    """test_fused_decode_epilogue_equals_decode_kernel with one level's class bias +inf or NaN (every candidate of that
    level has a non-finite class logit): the decode fused into the head-output conv (yl_epi.h) and the decode kernel on
    the levels of yl_forward give the same detections."""
    from yololite_amd import _lib as L
    meta = make_meta(img_size=96, **TINY[idx])
    sd = dict(synth_state_dict(meta, seed=20 + idx, head_noise=2.0))
    k = "head4.out.cls.bias"
    sd[k] = sd[k].copy()
    sd[k][-1] = float(val)
    m = _hip_for(meta, sd)
    ctx = m._ctx_for(96)
    x = _x(5, 96, seed=idx).to(DEV)
    outs = [o.clone() for o in m(x)]
    if val == "nan":
        # the plain head-output conv of yl_forward clamps its output with the activation bounds (-inf, inf) even without an
        # activation, and fmaxf(NaN, -inf) is -inf (the GPU's NaN handling in clamps is out of scope here): put the NaN
        # the fused epilogue sees back into the level the decode kernel reads
        C = TINY[idx]["num_classes"]
        outs[1][:, -1, ..., 5 + C - 1] = float("nan")          # (the last entry of the bias: the last anchor's last class)
    cases = [(L.POST_MAIN, 0.05, 0.5, 300, 0), (L.POST_FALLBACK, 0.05, 0.45, 300, 50), (L.POST_EVAL, 0.001, 0.65, 0, 0)]
    for mode, conf, iou, cap, topk in cases:
        d1, c1 = ctx.postprocess(outs, mode, conf, iou, cap, topk)
        d1, c1 = d1.cpu().numpy(), c1.cpu().numpy()
        for fuse in ((1, 0) if val == "inf" else (1,)):       # (fuse_decode 0 decodes the clamped level: see above)
            ctx.set_option("fuse_decode", fuse)
            d2, c2 = ctx.predict(x, mode, conf, iou, cap, topk)
            d2, c2 = d2.cpu().numpy(), c2.cpu().numpy()
            np.testing.assert_array_equal(c1, c2, err_msg=f"{mode} fuse {fuse}")
            for b in range(5):
                n = min(int(c1[b]), d1.shape[1])
                np.testing.assert_array_equal(d1[b, :n], d2[b, :n], err_msg=f"{mode} fuse {fuse} image {b}")
        ctx.set_option("fuse_decode", 1)
