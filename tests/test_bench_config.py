"""Parity tests of the BENCHMARKED configuration itself (bench.build_workload: the model, weights and inputs of
`python bench.py`) and of the other full-size BASELINE configs, run with `pytest -m gpu` on the MI355X box:

  config 2  edge_n 640x640 B=64, yl_predict + hipGraph + 2 streams + level-batched heads + fused decode
            == eager / 1 stream (bitwise), sampled images == oracle.pipeline_main(oracle forward) under the
            north_star tolerances (class ids equal, boxes equal after integer rounding, scores within 1e-4),
            nothing dropped by the packed-row capacity
  config 3  yololite_m 640x640 B=32        } determinism + batch invariance at full size (bitwise) and sampled
  config 4  edge_m + seg head 640x640 B=32 } images against the oracle
  config 1  edge_n 640x640 batch 1 through tools/infer.py (the CLI), detections == oracle flow

The oracle (CPU, fp32) runs only on the sampled images: ~0.1-3 s per image at these sizes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bench                                   # the benchmark's own workload builder
import yololite_amd as ya                      # noqa: F401
from yololite_amd import _lib
from oracle import model as omodel
from oracle import postproc as opost

DEV = "cuda:0"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _oracle(meta, sd):
    m = omodel.build_from_meta(meta).eval()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    return m


def _rows(dets, counts, b):
    k = int(counts[b])
    r = dets[b, :k].cpu().numpy()
    return r[:, :4], r[:, 4], r[:, 5].astype(np.int64)


def _assert_boxes_equal_after_rounding(got, exp):
    """north_star: box coordinates equal after integer rounding.  The only waiver: a coordinate that rounds differently
    while the RAW values agree to 1e-4 px (the value sits on a .5 boundary inside the fp32 drift of two summation
    orders) -- anything else is a failure."""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    assert got.shape == exp.shape
    bad = np.rint(got) != np.rint(exp)
    if bad.any():
        assert (np.abs(got[bad] - exp[bad]) < 1e-4).all(), (got[bad], exp[bad])
    np.testing.assert_allclose(got, exp, rtol=0, atol=1e-3)


def _align_score_ties(gb, eb, es, ec, band=1e-5):
    """Order inside a class is score-descending; two detections of one class whose ORACLE scores lie within `band`
    (the fp32 drift of the forward pass) may legitimately come out in the other order.  Returns the permutation of the
    oracle rows that undoes such swaps -- only rows of the same class within the band are ever exchanged; everything
    else stays where it is (and fails the comparison that follows if it differs)."""
    n = len(ec)
    perm = np.arange(n)
    close = lambda j, k: np.abs(np.asarray(gb[j], np.float64) - np.asarray(eb[k], np.float64)).max() < 0.5
    taken = set()
    for j in range(n):
        if close(j, j) and j not in taken:
            taken.add(j)
            continue
        cands = [k for k in range(max(0, j - 8), min(n, j + 9)) if k not in taken and ec[k] == ec[j] and
                 abs(float(es[k]) - float(es[j])) <= band and close(j, k)]
        if cands:
            perm[j] = cands[0]
            taken.add(cands[0])
    return perm if len(set(perm.tolist())) == n else np.arange(n)


def _assert_north_star(got, exp, b):
    gb, gs, gc = got
    assert gc.tolist() == exp["classes"][b].tolist(), "class ids / order differ"
    perm = _align_score_ties(gb, exp["boxes"][b], exp["scores"][b], exp["classes"][b])
    np.testing.assert_allclose(gs, exp["scores"][b][perm], rtol=0, atol=1e-4)
    _assert_boxes_equal_after_rounding(gb, exp["boxes"][b][perm])
    return int((perm != np.arange(len(perm))).sum())


def _score_tensor(levels, C=80):
    raw = torch.cat([l.reshape(l.shape[0], -1, l.shape[-1])[..., :5 + C] for l in levels], 1)
    return torch.sigmoid(raw[..., 4]) * torch.sigmoid(raw[..., 5:]).max(-1).values


def _safe_images(scores, boxes_unused, conf, cand, need=3):
    """images whose candidate scores all keep >= 2e-5 distance from `conf` (fp32 drift of the forward pass is ~1e-6
    relative: such an image cannot flip a threshold decision)"""
    ok = [b for b in cand if float((scores[b] - conf).abs().min()) > 2e-5]
    assert len(ok) >= need, "no sampled image is clear of the confidence threshold"
    return ok[:need]


def _iou64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    iw = max(min(a[2], b[2]) - max(a[0], b[0]), 0.0)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]), 0.0)
    inter = iw * ih
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def _assert_first_divergence_is_a_threshold_flip(got, exp_b, exp_s, exp_c, iou_thr, band=1e-5):
    """Two detection lists of ONE image (class ascending, score descending inside a class) that are not equal: locate
    the FIRST position where they differ.  Every kept box of that class with a higher score is then common to both
    lists, so the divergent detection D (present in one list, absent from the other) was decided by its largest IoU
    with those common boxes -- which must sit within `band` of the NMS threshold (one side computed > thr, the other
    <= thr inside the fp32 drift).  Anything else is a real disagreement."""
    gb, gs, gc = got
    n = min(len(gc), len(exp_c))
    # (boxes are not compared here: two near-tied scores of one class may swap places, see _align_score_ties)
    same = lambda j: int(gc[j]) == int(exp_c[j]) and abs(float(gs[j]) - float(exp_s[j])) <= 1e-4
    j = next((k for k in range(n) if not same(k)), n)
    assert j < max(len(gc), len(exp_c)), "lists are equal"
    cand = []                                       # (class, -score, box) of the entries at position j of both lists
    if j < len(gc):
        cand.append((int(gc[j]), -float(gs[j]), gb[j], "hip"))
    if j < len(exp_c):
        cand.append((int(exp_c[j]), -float(exp_s[j]), exp_b[j], "oracle"))
    cls, nscore, dbox, side = min(cand, key=lambda t: (t[0], t[1]))      # the one that sorts first is the extra detection
    # a third kind of decision inside the fp32 drift: the class arg-max of a candidate whose two best class logits are
    # nearly tied -- the SAME candidate (same box, same score to 1e-4) then sits in the other list under another class
    ob, os_, oc = (exp_b, exp_s, exp_c) if side == "hip" else (gb, gs, gc)
    twin = [k for k in range(len(oc)) if int(oc[k]) != cls and abs(float(os_[k]) + nscore) <= 1e-4 and
            np.abs(np.asarray(ob[k], np.float64) - np.asarray(dbox, np.float64)).max() <= 1e-2]
    if twin:
        return j, cls, f"class arg-max near-tie (the same candidate is class {int(oc[twin[0]])} on the other side)"
    # common kept boxes of that class in front of position j
    common = [exp_b[k] for k in range(j) if int(exp_c[k]) == cls]
    assert common, ("first divergence has no earlier kept box of its class to be suppressed by", j, cls, side)
    top = max(_iou64(dbox, k) for k in common)
    assert abs(top - iou_thr) <= band, (f"first differing detection (position {j}, class {cls}, extra on the {side} side): "
                                        f"deciding IoU {top:.7f} is not within {band} of the threshold {iou_thr}")
    return j, cls, top


def _assert_all_safe_images(dets, counts, exp, ref_scores, conf, images, min_safe_frac=0.9, exp_index=None, iou_thr=0.5,
                            what="", got_scores=None):
    """north_star on EVERY threshold-safe image of `images` (exp lists are indexed by position unless exp_index maps
    image -> position).  Safe = every candidate score of the oracle keeps clear of `conf` by more than the image's MEASURED
    score drift (1.5 x max |hip score - oracle score| over all its candidates when got_scores is given -- itself asserted
    <= 1e-4 by the callers -- and never less than 2e-5): no threshold decision can flip; at least `min_safe_frac` of the
    images must be safe.  Every safe image is held to class
    ids, 1e-4 scores and rounded boxes -- except that at most ONE image may differ in its detection list, and only if
    the first differing detection is PROVEN to be an NMS decision on the threshold (its deciding IoU within 1e-5 of
    iou_thr, _assert_first_divergence_is_a_threshold_flip) with the counts within +-2.  Prints how many images were
    held to the bar."""
    images = list(images)
    ix = lambda b: b if exp_index is None else exp_index[b]
    band = {b: 2e-5 if got_scores is None else max(2e-5, 1.5 * float((got_scores[ix(b)] - ref_scores[ix(b)]).abs().max()))
            for b in images}
    safe = [b for b in images if float((ref_scores[ix(b)] - conf).abs().min()) > band[b]]
    odd = []
    for b in safe:
        i = b if exp_index is None else exp_index[b]
        gb, gs, gc = _rows(dets, counts, b)
        if gc.tolist() != exp["classes"][i].tolist():
            assert abs(len(gc) - len(exp["classes"][i])) <= 2, (b, len(gc), len(exp["classes"][i]))
            flip = _assert_first_divergence_is_a_threshold_flip((gb, gs, gc), exp["boxes"][i], exp["scores"][i],
                                                                exp["classes"][i], iou_thr)
            odd.append((b, flip))
            continue
        _assert_north_star((gb, gs, gc), exp, i)
    print(f"[parity {what}] images held to class ids / 1e-4 scores / rounded boxes: {len(safe) - len(odd)} of {len(images)} "
          f"(threshold-safe {len(safe)}, largest safety band {max(band.values()):.2e}, list differs by a proven "
          f"IoU-threshold flip: {odd})")
    assert len(safe) >= min_safe_frac * len(images), (len(safe), len(images))
    assert len(odd) <= 1, odd
    return [b for b in safe if b not in [o[0] for o in odd]]


@pytest.mark.parametrize("seed", [1, 2])
def test_bench_configuration_edge_n_b64_parity(seed):
    """seed 1 is the benchmark's weight seed; seed 2 a second model (and input batch) held to the same bar"""
    wl = bench.build_workload("edge_n", 640, 64, seed=seed, dev=DEV, rank=seed - 1)
    ctx, x, meta, sd = wl["ctx"], wl["x"], wl["meta"], wl["sd"]
    mo = bench.MAX_OUT
    # ---- reference schedule: eager, one stream, per-level launches, decode kernel
    for k, v in (("graph", 0), ("streams", 1), ("batch_levels", 0), ("fuse_decode", 0)):
        ctx.set_option(k, v)
    d0, c0 = ctx.predict(x, _lib.POST_MAIN, 0.4, 0.5, per_class_cap=300, max_out=mo)
    d0, c0 = d0.clone(), c0.clone()
    cn = c0.cpu().numpy()
    assert cn.min() >= 50 and cn.max() <= mo, (cn.min(), cn.max())          # every image detects, nothing dropped
    ncls = [len(np.unique(_rows(d0, c0, b)[2])) for b in range(64)]
    assert np.mean(ncls) >= 40, np.mean(ncls)
    for g in (4, 2, 1):                                                      # NMS class-group split: same detections
        ctx.set_option("nms_groups", g)
        dg, cg = ctx.predict(x, _lib.POST_MAIN, 0.4, 0.5, per_class_cap=300, max_out=mo)
        assert torch.equal(cg, c0), g
        for b in range(64):
            assert torch.equal(dg[b, :cn[b]], d0[b, :cn[b]]), (g, b)
    ctx.set_option("nms_groups", 0)
    # ---- the bench schedule (bench.py defaults): hipGraph replay, 2 streams, level-batched heads, fused decode
    for k, v in (("graph", 1), ("streams", 2), ("batch_levels", 1), ("fuse_decode", 1)):
        ctx.set_option(k, v)
    for rep in range(3):                                                     # capture, then two replays
        d1, c1 = ctx.predict(x, _lib.POST_MAIN, 0.4, 0.5, per_class_cap=300, max_out=mo)
        assert torch.equal(c1, c0), rep
        for b in range(64):
            assert torch.equal(d1[b, :cn[b]], d0[b, :cn[b]]), (rep, b)
    # ---- ALL 64 images against the oracle end to end (oracle forward -> oracle pipeline): every image whose candidate
    # scores keep clear of the confidence threshold must give the oracle's class-id list, scores and rounded boxes
    orc = _oracle(meta, sd)
    with torch.no_grad():
        ref_lv = orc(x.cpu())
    ref_s = _score_tensor(ref_lv)
    exp = opost.pipeline_main(ref_lv, 640, 0.4, 0.5, 300)
    # raw head tensors: decoded scores within the 1e-4 bar everywhere (not only on survivors), all 64 images
    lv = wl["model"](x)
    got_s = _score_tensor([t.cpu() for t in lv])
    assert float((got_s - ref_s).abs().max()) <= 1e-4
    _assert_all_safe_images(d1, c1, exp, ref_s, 0.4, range(64), what=f"edge_n B=64 seed {seed}", got_scores=got_s)


@pytest.mark.parametrize("name,seg,B", [("edge_n", False, 64), ("yololite_m", False, 32), ("edge_m", True, 32),
                                        ("yololite_m_v2", False, 32)])
def test_bench_schedule_two_lanes_graph_full_size_parity(name, seg, B):
    """The schedule `python bench.py` times: serving.ServingPipeline with 2 lanes x 1 chunk stream x
    hipGraph replay -- un-chunked full-batch launches of two cloned contexts CO-RESIDENT on the chip, persistent grids of
    one lane next to the other lane's -- at the benchmark's full size, over 8 submissions of two different resident
    batches.  The submission order A B B A A B A B sends both batches through both lanes, as capture and as replay.
    Every handed-back result (rows, counts, and for the seg model the prototype indices and the image-resolution masks
    written on the lane) must be torch.equal to the eager one-stream call of the model's own context."""
    from yololite_amd.serving import ServingPipeline
    wl = bench.build_workload(name, 640, B, seed=1, seg=seg, dev=DEV)
    ctx, xa = wl["ctx"], wl["x"]
    xb = bench.synth_images(B, 640, seed=4321).to(DEV)
    mo = bench.MAX_OUT
    ctx.set_option("graph", 0); ctx.set_option("streams", 1)
    want = {}
    for key, x in (("a", xa), ("b", xb)):
        r = ctx.predict(x, _lib.POST_MAIN, 0.4, 0.5, per_class_cap=300, max_out=mo, want_idx=seg)
        r = tuple(t.clone() for t in r)
        masks = None
        if seg:
            masks = [m.clone() for m in ctx.masks_image(r[0], r[1], r[2], packed=True)]
        want[key] = (r, masks)
        assert int(r[1].min()) >= 20 and int(r[1].max()) <= mo
    assert not torch.equal(want["a"][0][1], want["b"][0][1])              # two different batches
    before = {k: ctx.get_option(k) for k in ("graph", "streams")}
    pipe = ServingPipeline(ctx, lanes=2, streams_per_lane=1, graph=True)
    assert {k: ctx.get_option(k) for k in before} == before              # the caller's context is left alone
    assert all(c.handle.value != ctx.handle.value for c in pipe.ctxs)
    order = "abbaabab"
    xs = {"a": xa, "b": xb}
    S_ = 640
    # one set of output buffers per SUBMISSION: a lane's buffers may be rewritten as soon as its result has been handed back,
    # and run() hands back and re-submits in one call (the serving loop consumes a result before it re-uses the lane)
    arenas = [torch.empty((B * mo * S_ * ((S_ + 31) // 32) * 4,), device=DEV, dtype=torch.uint8) if seg else None
              for _ in range(len(order))]
    outs = [(torch.empty((B, mo, 6), device=DEV), torch.empty((B,), device=DEV, dtype=torch.int32)) for _ in range(len(order))]

    def work_for(i, key):
        def work(c, k):
            r = c.predict(xs[key], _lib.POST_MAIN, 0.4, 0.5, per_class_cap=300, max_out=mo, out=outs[i], want_idx=seg)
            if seg:
                return tuple(r) + (c.masks_image(r[0], r[1], r[2], packed=True, arena=arenas[i]),)
            return tuple(r)
        return work

    def check(key, r):
        (d0, c0, *rest0), m0 = want[key]
        cn = c0.cpu().numpy()
        assert torch.equal(r[1], c0), key
        for b in range(B):
            assert torch.equal(r[0][b, :cn[b]], d0[b, :cn[b]]), (key, b)
        if seg:
            for b in range(B):
                assert torch.equal(r[2][b, :cn[b]], rest0[0][b, :cn[b]]), (key, b)
                got = r[3][b, :cn[b]].contiguous().view(torch.uint8).reshape(-1)       # arena view [B, max_out, h, row bytes]
                exp = m0[b].contiguous().view(torch.uint8).reshape(-1)                # list entry [Ni, h, ceil(w / 32)] words
                assert got.numel() == exp.numel() and torch.equal(got, exp), (key, b)

    handed = []
    for i, key in enumerate(order):
        r = pipe.run(work_for(i, key))
        if r is not None:
            # the hand-back is ordered on the current stream; compare before the lane's buffers are written again
            check(order[i - 2], r)
            handed.append(order[i - 2])
    for j, r in enumerate(pipe.flush()):
        check(order[len(order) - 2 + j], r)
        handed.append(order[len(order) - 2 + j])
    assert "".join(handed) == order


@pytest.mark.parametrize("name,seg,seed", [("yololite_m", False, 1), ("edge_m", True, 1), ("yololite_m", False, 2),
                                           ("edge_m", True, 2), ("yololite_m_v2", False, 1)])
def test_full_size_configs_3_and_4(name, seg, seed):
    """BASELINE configs 3 / 4 at 640x640 B=32 (two weight seeds each; plus the published efficientnetv2 yololite_m):
    bitwise determinism and batch invariance of the raw levels, the bench schedule against the eager one, ALL 32 images
    against the oracle (detections; masks of two images for config 4)."""
    wl = bench.build_workload(name, 640, 32, seed=seed, seg=seg, dev=DEV, rank=seed - 1)
    ctx, x, meta, sd, model = wl["ctx"], wl["x"], wl["meta"], wl["sd"], wl["model"]
    a = model(x)
    b = model(x)
    la, lb = (a[0], b[0]) if seg else (a, b)
    for u, v in zip(la, lb):
        assert torch.equal(u, v)
    if seg:
        assert torch.equal(a[1], b[1])
    for i in (0, 17, 31):
        one = model(x[i:i + 1])
        lo = one[0] if seg else one
        for u, v in zip(la, lo):
            assert torch.equal(u[i:i + 1], v), i
    mo = bench.MAX_OUT
    ctx.set_option("graph", 0); ctx.set_option("streams", 1)
    d0, c0, i0 = ctx.predict(x, _lib.POST_MAIN, 0.4, 0.5, per_class_cap=300, max_out=mo, want_idx=True)
    d0, c0, i0 = d0.clone(), c0.clone(), i0.clone()
    cn = c0.cpu().numpy()
    assert cn.min() >= 20 and cn.max() <= mo, (cn.min(), cn.max())
    ctx.set_option("graph", 1); ctx.set_option("streams", 2)
    for rep in range(2):
        d1, c1 = ctx.predict(x, _lib.POST_MAIN, 0.4, 0.5, per_class_cap=300, max_out=mo)
        assert torch.equal(c1, c0)
        for bb in range(32):
            assert torch.equal(d1[bb, :cn[bb]], d0[bb, :cn[bb]]), (rep, bb)
    orc = _oracle(meta, sd)
    cand = list(range(32))                                             # every image (the oracle forward costs ~1 s each)
    parts = []
    with torch.no_grad():
        for i0_ in range(0, 32, 4):                                    # 4 images at a time: host memory
            parts.append(orc(x[i0_:i0_ + 4].cpu()))
    if seg:
        ref_lv = [torch.cat([p[0][l] for p in parts]) for l in range(len(parts[0][0]))]
        ref_pr = torch.cat([p[1] for p in parts])
    else:
        ref_lv, ref_pr = [torch.cat([p[l] for p in parts]) for l in range(len(parts[0]))], None
    det_lv = [t[..., :85] for t in ref_lv]
    exp = opost.pipeline_main(det_lv, 640, 0.4, 0.5, 300)
    pos = {b: i for i, b in enumerate(cand)}
    got_s = _score_tensor([t[cand].cpu() for t in la])
    print(f"[parity {name} seed {seed}] max |score - oracle score| over all candidates: "
          f"{float((got_s - _score_tensor(det_lv)).abs().max()):.3e}")
    assert float((got_s - _score_tensor(det_lv)).abs().max()) <= 1e-4
    safe = _assert_all_safe_images(d1, c1, exp, _score_tensor(det_lv), 0.4, cand, exp_index=pos,
                                   what=f"{name}{'+seg' if seg else ''} B=32 seed {seed}", got_scores=got_s)
    sel = [pos[b] for b in safe][:2]
    # Winograd F(2x2,3x3): everything above ran the library default ("winograd" 1: every eligible dense 3x3 stride-1
    # layer -- yololite_m's six FPN convs, the fused-MBConv expansions of the efficientnetv2 backbone, the prototype
    # branch's first conv).  The other two settings are held to the SAME north_star bounds at full size -- all candidate
    # scores within 1e-4 of the oracle, sampled detections equal after rounding: 0 = direct convolution everywhere, 2 = only
    # the >= 64-channel layers of the finest level
    ctx.set_option("graph", 1); ctx.set_option("streams", 2)
    outs = {}
    for mode in (0, 2):
        ctx.set_option("winograd", mode)
        w = model(x)
        lw = w[0] if seg else w
        outs[mode] = (w[1].clone() if seg else None, [t.clone() for t in lw])
        err = float((_score_tensor([t[cand].cpu() for t in lw]) - _score_tensor(det_lv)).abs().max())
        print(f"[parity {name} seed {seed}] winograd {mode}: max |score - oracle score| {err:.3e}")
        assert err <= 1e-4
        dw_, cw_ = ctx.predict(x, _lib.POST_MAIN, 0.4, 0.5, per_class_cap=300, max_out=mo)
        # (round 5, VERDICT r04: the other Winograd settings used to be held to two sampled images) EVERY threshold-safe image
        _assert_all_safe_images(dw_, cw_, exp, _score_tensor(det_lv), 0.4, cand, exp_index=pos,
                                what=f"{name}{'+seg' if seg else ''} B=32 seed {seed} winograd {mode}",
                                got_scores=_score_tensor([t[cand].cpu() for t in lw]))
    if seg:                                                        # edge_m: only the prototype branch has eligible convs
        assert not torch.equal(outs[0][0], a[1]) and float((outs[0][0] - a[1]).abs().max()) <= 1e-4
        # (mode 2 = the >= 64-channel layer on the largest grid: the second prototype conv at 160x160 only)
        assert not torch.equal(outs[2][0], outs[0][0]) and float((outs[2][0] - a[1]).abs().max()) <= 1e-4
    else:                                                          # the options really select other kernels
        assert any(not torch.equal(u, v) for u, v in zip(la, outs[0][1]))
        assert any(not torch.equal(u, v) for u, v in zip(la, outs[2][1]))
    ctx.set_option("winograd", 1)
    if seg:
        # config 4: image-resolution masks (640 x 640 input grid, no back-map) of the sampled images vs the oracle's
        # restatement on the ORACLE's own levels / prototypes, mask IoU >= 0.999 (north_star); packed == unpacked
        ctx.set_option("graph", 0); ctx.set_option("streams", 1)
        d2, c2, i2 = ctx.predict(x, _lib.POST_MAIN, 0.4, 0.5, per_class_cap=300, max_out=mo, want_idx=True)
        mk = ctx.masks_image(d2, c2, i2)
        mp = ctx.masks_image(d2, c2, i2, packed=True)
        tot_i = tot_u = 0
        for i in sel:
            b = cand[i]
            n = min(int(c2[b]), 48)                                # the oracle materialises [n, 640, 640] floats
            keep = [i2[b, :n].cpu().numpy()]
            boxes = [d2[b, :n, :4].cpu().numpy()]
            exp = opost.masks_image_for([t[i:i + 1] for t in ref_lv], ref_pr[i:i + 1], 80, 640, keep, boxes, [(640, 640)])[0]
            got = mk[b][:n].cpu().numpy().astype(bool)
            inter, union = (got & exp.astype(bool)).sum(), (got | exp.astype(bool)).sum()
            tot_i += int(inter); tot_u += int(union)
            assert union == 0 or inter / union >= 0.999, (b, inter, union)
            words = mp[b][:n].cpu().numpy().view(np.uint32)
            bits = ((words[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(n, 640, -1)[..., :640].astype(bool)
            assert np.array_equal(bits, got)
        assert tot_u > 1000, tot_u
        # the asynchronous fixed-capacity form the benchmark uses (no host read of the counts): same bits
        arena = torch.empty((32 * mo * 640 * 80,), device=DEV, dtype=torch.uint8)
        va = ctx.masks_image(d2, c2, i2, packed=True, arena=arena)
        assert va.shape == (32, mo, 640, 20)
        for b in range(32):
            assert torch.equal(va[b, :int(c2[b])], mp[b]), b


def _match_detection_lists(got, exp, max_unmatched):
    """tolerant comparison of two detection lists of ONE image at evaluation thresholds (thousands of survivors: a
    handful of decisions sit inside the fp32 drift of the forward pass).  got / exp: (boxes [n,4], scores, classes).
    Every oracle detection is matched to a detection of the same class whose rounded box is equal; scores of matched
    pairs within 1e-4; at most `max_unmatched` detections on either side stay unmatched."""
    gb, gs, gc = got
    eb, es, ec = exp
    from collections import defaultdict
    idx = defaultdict(list)
    for j in range(len(gc)):
        idx[(int(gc[j]),) + tuple(np.rint(gb[j]).astype(np.int64).tolist())].append(j)
    un_e, used = 0, 0
    for i in range(len(ec)):
        key = (int(ec[i]),) + tuple(np.rint(eb[i]).astype(np.int64).tolist())
        c = [j for j in idx.get(key, []) if abs(float(gs[j]) - float(es[i])) <= 1e-4]
        if c:
            idx[key].remove(c[0]); used += 1
        else:
            un_e += 1
    un_g = len(gc) - used
    assert un_e <= max_unmatched and un_g <= max_unmatched, (len(ec), len(gc), un_e, un_g)


def test_eval_mode_on_real_levels_at_640():
    """the evaluation pipeline (conf 0.001 / iou 0.65, no cap: thousands of survivors per image) on a
    REAL model's levels at 640x640 -- (i) yl_predict(POST_EVAL) == the oracle pipeline run on the HIP forward's own
    levels: identical detection lists (every threshold / NMS decision), values to the last ulp of expf; (ii) == the oracle end to end (oracle forward) up to the handful of
    decisions inside the forward pass's fp32 drift."""
    wl = bench.build_workload("edge_n", 640, 8, seed=1, dev=DEV)
    ctx, x, meta, sd, model = wl["ctx"], wl["x"], wl["meta"], wl["sd"], wl["model"]
    lv = [t.cpu() for t in model(x)]
    dets, counts = ctx.predict(x, _lib.POST_EVAL, 0.001, 0.65, per_class_cap=0, topk=0, max_out=ctx.N)
    cn = counts.cpu().numpy()
    assert cn.min() >= 1000, cn                                    # thousands of survivors
    _, raw = opost.pipeline_eval(lv, 640, 0.001, 0.65)
    for b in range(8):
        gb, gs, gc = _rows(dets, counts, b)
        eb, es, ec = raw[b]
        assert gc.tolist() == ec.tolist(), b                       # same survivors, same NMS decisions, same order
        np.testing.assert_allclose(gs, es, rtol=0, atol=1e-6)      # expf of the device vs torch: ulp-level
        _match_detection_lists((gb, gs, gc), (eb, es, ec), max_unmatched=1)   # (ulp-level score ties may swap places)
    orc = _oracle(meta, sd)
    with torch.no_grad():
        ref_lv = orc(x.cpu())
    _, raw2 = opost.pipeline_eval(ref_lv, 640, 0.001, 0.65)
    for b in range(8):
        _match_detection_lists(_rows(dets, counts, b), raw2[b], max_unmatched=max(3, len(raw2[b][2]) // 200))


def test_cli_evaluate_end_to_end(tmp_path):
    """tools/evaluate.py end to end on edge_n @640 with 8 images of mixed sizes: detections.json ==
    oracle(preprocess_albumentations -> forward -> pipeline_eval, conf 0.001 / iou 0.65).  Two comparisons, as in
    test_eval_mode_on_real_levels_at_640: list-identical against the oracle pipeline on the HIP forward of the ORACLE's
    pre-processed tensor (pins pre-processing, decode, NMS, [cx,cy,w,h] conversion, category_id, image ids, order),
    tolerant against the oracle forward."""
    from PIL import Image
    from oracle import preproc as opre
    wl = bench.build_workload("edge_n", 640, 1, seed=1, dev=DEV)
    meta, sd, model = dict(wl["meta"]), wl["sd"], wl["model"]
    meta["names"] = [f"c{i}" for i in range(80)]
    ck = str(tmp_path / "edge_n.pt")
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}, "meta": meta}, ck)
    rng = np.random.RandomState(11)
    sizes = [(480, 640), (640, 640), (360, 500), (700, 420), (640, 480), (333, 777), (512, 512), (900, 1200)]
    (tmp_path / "imgs").mkdir()
    imgs = []
    for k, (h, w) in enumerate(sizes):
        im = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        Image.fromarray(im[..., ::-1]).save(str(tmp_path / "imgs" / f"im{k}.png"))     # files are RGB; arrays are BGR
        imgs.append(im)
    for flag in ([], ["--debug-levels"]):                                              # fused yl_predict and the two-call form
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "evaluate.py"), "--weights", ck, "--test_folder",
                            str(tmp_path / "imgs"), "--img_size", "640", "--batch_size", "3"] + flag,
                           cwd=str(tmp_path), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    with open(tmp_path / "runs" / "evaluate" / "1" / "detections.json") as f:
        dj = json.load(f)
    with open(tmp_path / "runs" / "evaluate" / "2" / "detections.json") as f:
        assert json.load(f) == dj                                                      # the two forms agree exactly
    orc = _oracle(meta, sd)
    tot = 0
    for k, im in enumerate(imgs):                                                      # sorted file order == k order
        xx, _ = opre.preprocess_albumentations(im, 640)
        xt = torch.from_numpy(xx[None])
        got = [d for d in dj if d["image_id"] == k]
        assert all(d["file_name"] == f"im{k}.png" for d in got)
        lv = [t.cpu() for t in model(xt.to(DEV))]
        exp, _ = opost.pipeline_eval(lv, 640, 0.001, 0.65)
        assert [d["category_id"] for d in got] == [d["category_id"] for d in exp[0]], k
        np.testing.assert_allclose([d["score"] for d in got], [d["score"] for d in exp[0]], rtol=0, atol=1e-6)
        # (two detections of one class whose scores differ by an ulp of expf may swap places: boxes are compared as a set)
        xyxy = lambda ds: np.asarray([[d["bbox"][0] - d["bbox"][2] / 2, d["bbox"][1] - d["bbox"][3] / 2,
                                       d["bbox"][0] + d["bbox"][2] / 2, d["bbox"][1] + d["bbox"][3] / 2] for d in ds], np.float64)
        _match_detection_lists((xyxy(got), np.asarray([d["score"] for d in got]), np.asarray([d["category_id"] for d in got])),
                               (xyxy(exp[0]), np.asarray([d["score"] for d in exp[0]]), np.asarray([d["category_id"] for d in exp[0]])),
                               max_unmatched=1)
        with torch.no_grad():
            _, raw2 = opost.pipeline_eval(orc(xt), 640, 0.001, 0.65)
        gb = np.asarray([[d["bbox"][0] - d["bbox"][2] / 2, d["bbox"][1] - d["bbox"][3] / 2,
                          d["bbox"][0] + d["bbox"][2] / 2, d["bbox"][1] + d["bbox"][3] / 2] for d in got], np.float64)
        _match_detection_lists((gb, np.asarray([d["score"] for d in got]), np.asarray([d["category_id"] - 1 for d in got])),
                               raw2[0], max_unmatched=max(3, len(got) // 200))
        tot += len(got)
    assert tot >= 8000, tot


def test_config1_edge_n_640_batch1_through_cli(tmp_path):
    """BASELINE config 1: edge_n 640x640, batch 1, the tools/infer.py flow (checkpoint file -> letterbox ->
    forward -> decode -> per-class NMS -> back-map -> JSON) against the oracle's restatement of the same flow."""
    from PIL import Image
    from oracle import preproc as opre
    wl = bench.build_workload("edge_n", 640, 1, seed=1, dev=DEV)
    meta, sd = dict(wl["meta"]), wl["sd"]
    meta["names"] = [f"c{i}" for i in range(80)]
    ck = str(tmp_path / "edge_n.pt")
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}, "meta": meta}, ck)
    rng = np.random.RandomState(3)
    imgs = {"frame_a": rng.randint(0, 256, size=(480, 640, 3)).astype(np.uint8),       # letterboxed (pad top/bottom)
            "frame_b": rng.randint(0, 256, size=(640, 640, 3)).astype(np.uint8)}       # identity resize
    (tmp_path / "imgs").mkdir()
    for n, im in imgs.items():
        Image.fromarray(im[..., ::-1]).save(str(tmp_path / "imgs" / f"{n}.png"))       # files are RGB; arrays are BGR
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "infer.py"), "--weights", ck, "--img_dir",
                        str(tmp_path / "imgs"), "--img_size", "640"], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    orc = _oracle(meta, sd)
    checked = 0
    for n, im in imgs.items():
        with open(tmp_path / "runs" / "infer" / "1" / "json" / f"{n}.json") as f:
            dets = json.load(f)["detections"]
        xx, (padx, pady, scale, w0, h0) = opre.preprocess(im, 640)
        with torch.no_grad():
            lv = orc(torch.from_numpy(xx[None]))
        if float((_score_tensor(lv) - 0.4).abs().min()) <= 2e-5:
            continue
        exp = opost.pipeline_main(lv, 640, 0.4, 0.5, 300)
        eb = opost.backmap(exp["boxes"][0], padx, pady, scale, w0, h0)
        assert len(dets) >= 20
        assert [d["class_id"] for d in dets] == exp["classes"][0].tolist()
        np.testing.assert_allclose([d["score"] for d in dets], exp["scores"][0], rtol=0, atol=1e-4)
        _assert_boxes_equal_after_rounding([d["bbox_xyxy"] for d in dets], eb)
        checked += 1
    assert checked >= 1


def test_plain_bench_run_times_its_steps_and_dumps_outputs(tmp_path):
    """A plain `bench.py` run (no --full) times exactly --steps steps in one block and reports the headline alone;
    --dump-outputs writes the last timed step's results, and a second run with the same arguments dumps the same arrays."""
    dumps = []
    for i in range(2):
        out = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2",
                            "--batch", "8", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert (d["metric"], d["unit"], d["higher_is_better"], d["dtype"]) == ("images/sec", "images/sec", True, "f32")
        assert d["steps"] == 6 and d["blocks"]["n"] == 1 and d["blocks"]["steps_each"] == 6
        assert d["value"] * d["ms_per_step"] == pytest.approx(8 * 1000.0, rel=1e-3)
        assert not {"roofline", "network", "one_batch_in_flight", "other_configs", "cpu_baseline", "gpu_batch1_flow"} & set(d)
        dets, counts = np.load(out / "dets.npy"), np.load(out / "counts.npy")
        assert dets.dtype == np.float32 and dets.shape == (8, bench.MAX_OUT, 6)
        assert counts.dtype == np.float64 and counts.shape == (8,) and counts.min() > 0
        assert not dets[np.arange(bench.MAX_OUT)[None, :] >= counts[:, None]].any()
        assert sum(f.stat().st_size for f in out.iterdir()) <= 64 << 20
        dumps.append((dets, counts))
    assert np.array_equal(dumps[0][0], dumps[1][0]) and np.array_equal(dumps[0][1], dumps[1][1])
