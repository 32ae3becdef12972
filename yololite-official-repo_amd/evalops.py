"""Evaluate-path consumers on the device behind the reference's own signatures.

    build_curves_from_coco(coco_images, coco_anns, coco_dets, out_dir, iou, steps)
        <- scripts/data/p_r_f1.py:6-162 (same summary dict)
    create_confusion_matrix(coco_anns, coco_dets, class_names, SAVE_PATH, ...)
        <- scripts/helpers/evaluate.py:59-238 (same *_stats.txt; returns the raw matrix as well;
           the heat-map PNG is not drawn)
    _coco_eval_from_lists(coco_images, coco_anns, coco_dets, iouType, num_classes) / coco_eval(...)
        <- scripts/helpers/helpers.py:155-227, pycocotools COCOeval (bbox): same dict; matching and
           accumulation in yl_eval_coco_match / yl_eval_coco_accumulate, summarize in numpy

The reference runs both as nested python loops over detections x ground truths -- and repeats the
P/R/F1 matching once per confidence step (201 times).  Here the host only groups and orders the rows
(numpy sort / unique); the matching runs in yl_eval_match / yl_eval_confusion, one wavefront per
(image, category) key or per image, and the 0..1 sweep is ONE matching pass plus a histogram
(yl_eval_sweep): greedy matching of a score-descending list is prefix-stable, so the per-threshold
re-matching of the reference yields exactly the prefix of the full pass.

No CPU fallback: the kernels live in libyololite_hip.so and a HIP device is required.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib


def _dev(device):
    if not torch.cuda.is_available():
        raise _lib.YoloLiteHipError("evalops needs a HIP device (no CPU fallback)")
    return torch.device(device if device is not None else "cuda:0")


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() > 0 else None


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# device time of the matching kernels (HIP events around every yl_eval_* launch), accumulated for the benchmark line:
# bench.py --workload eval reports how much of a step is kernels and how much host list -> array conversion
DEVICE_MS = {"total": 0.0, "launches": 0}


class _timed_launch:
    def __init__(self, dev, name=None):
        self.dev, self.name = dev, name          # name: also accumulated under DEVICE_MS[name]

    def __enter__(self):
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.e0.record(torch.cuda.current_stream(self.dev))
        return self

    def __exit__(self, *exc):
        self.e1.record(torch.cuda.current_stream(self.dev))
        self.e1.synchronize()
        DEVICE_MS["total"] += self.e0.elapsed_time(self.e1)
        DEVICE_MS["launches"] += 1
        if self.name:
            DEVICE_MS[self.name] = DEVICE_MS.get(self.name, 0.0) + self.e0.elapsed_time(self.e1)
        return False


def _offsets(sorted_keys, num_keys):
    off = np.zeros(num_keys + 1, dtype=np.int32)
    if len(sorted_keys):
        off[1:] = np.cumsum(np.bincount(sorted_keys, minlength=num_keys))
    return off


# ------------------------------------------------------------------------------ per-class matching
def match_per_class(det_img, det_cat, det_xywh, det_score, gt_img, gt_cat, gt_xywh, iou=0.5, device=None):
    """Greedy per-(image, category) matching of p_r_f1.py:58-78 for array inputs.
    Returns (tp uint8 [Nd] in the ORIGINAL detection order, has_gt bool [Nd], matched_gt bool [Ng])."""
    lib = _lib.load()
    dev = _dev(device)
    det_img = np.asarray(det_img, dtype=np.int64); det_cat = np.asarray(det_cat, dtype=np.int64)
    gt_img = np.asarray(gt_img, dtype=np.int64); gt_cat = np.asarray(gt_cat, dtype=np.int64)
    det_xywh = np.asarray(det_xywh, dtype=np.float64).reshape(-1, 4)
    gt_xywh = np.asarray(gt_xywh, dtype=np.float64).reshape(-1, 4)
    det_score = np.asarray(det_score, dtype=np.float64)
    nd, ng = len(det_img), len(gt_img)
    if nd == 0:
        return np.zeros(0, np.uint8), np.zeros(0, bool), np.zeros(ng, bool)
    pairs = np.concatenate([np.stack([det_img, det_cat], 1), np.stack([gt_img, gt_cat], 1)], 0)
    _, inv = np.unique(pairs, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    nk = int(inv.max()) + 1
    dkey, gkey = inv[:nd], inv[nd:]
    # key-major, score descending, original list order on ties (python's stable sorted(reverse=True))
    dorder = np.lexsort((np.arange(nd), -det_score, dkey))
    gorder = np.argsort(gkey, kind="stable")
    det_off = _offsets(dkey[dorder], nk)
    gt_off = _offsets(gkey[gorder], nk)

    t_det = _up(det_xywh[dorder], dev)
    t_doff, t_goff = _up(det_off, dev), _up(gt_off, dev)
    t_gt = _up(gt_xywh[gorder], dev) if ng else None
    t_tp = torch.empty(nd, dtype=torch.uint8, device=dev)
    t_gm = torch.empty(max(ng, 1), dtype=torch.uint8, device=dev)
    with _timed_launch(dev):
        _lib.check(lib.yl_eval_match(_ptr(t_det), _ptr(t_doff), _ptr(t_gt), _ptr(t_goff), nk, ng, float(iou),
                                     _ptr(t_tp), None, _ptr(t_gm), _stream(dev)), what="yl_eval_match")
    tp_sorted = t_tp.cpu().numpy()
    tp = np.empty(nd, np.uint8); tp[dorder] = tp_sorted
    has_gt = (gt_off[1:] - gt_off[:-1])[dkey] > 0
    gm = np.zeros(ng, bool)
    if ng:
        gm[gorder] = t_gm[:ng].cpu().numpy().astype(bool)
    return tp, has_gt, gm


def sweep_counts(score, tp, counted, thresholds, device=None):
    """TP / FP counts among `counted` detections with score >= thr, for every thr (p_r_f1.py:100-118)."""
    lib = _lib.load()
    dev = _dev(device)
    thr = np.asarray(thresholds, dtype=np.float64)
    steps = len(thr)
    n = len(score)
    t_thr = _up(thr, dev)
    t_tpg = torch.empty(steps, dtype=torch.int32, device=dev)
    t_fpg = torch.empty(steps, dtype=torch.int32, device=dev)
    t_s = _up(np.asarray(score, np.float64), dev) if n else None
    t_tp = _up(np.asarray(tp, np.uint8), dev) if n else None
    t_c = _up(np.asarray(counted, np.uint8), dev) if n else None
    with _timed_launch(dev):
        _lib.check(lib.yl_eval_sweep(_ptr(t_s), _ptr(t_tp), _ptr(t_c), n, _ptr(t_thr), steps, _ptr(t_tpg), _ptr(t_fpg),
                                     _stream(dev)), what="yl_eval_sweep")
    return t_tpg.cpu().numpy().astype(np.int64), t_fpg.cpu().numpy().astype(np.int64)


def build_curves_from_coco(coco_images, coco_anns, coco_dets, out_dir=None, iou=0.50, steps=201, device=None):
    """Drop-in for scripts/data/p_r_f1.py:6-162: same arguments, same summary dict (`out_dir` is
    accepted and, as in the reference, nothing is written by this function)."""
    total_gt = len(coco_anns)
    if len(coco_dets) == 0:                                                  # p_r_f1.py:80-89
        return {"iou": float(iou), "best_f1": 0.0, "best_conf": 0.0, "precision_at_best": 0.0,
                "recall_at_best": 0.0}
    d_img = np.array([int(d["image_id"]) for d in coco_dets], dtype=np.int64)
    d_cat = np.array([int(d["category_id"]) for d in coco_dets], dtype=np.int64)
    d_box = np.array([d["bbox"] for d in coco_dets], dtype=np.float64).reshape(-1, 4)
    d_sc = np.array([float(d.get("score", 0.0)) for d in coco_dets], dtype=np.float64)
    g_img = np.array([int(a["image_id"]) for a in coco_anns], dtype=np.int64)
    g_cat = np.array([int(a["category_id"]) for a in coco_anns], dtype=np.int64)
    g_box = np.array([a["bbox"] for a in coco_anns], dtype=np.float64).reshape(-1, 4)

    tp, has_gt, _ = match_per_class(d_img, d_cat, d_box, d_sc, g_img, g_cat, g_box, iou=iou, device=device)
    confs = np.linspace(0.0, 1.0, steps)
    tp_ge, fp_ge = sweep_counts(d_sc, tp, has_gt, confs, device=device)

    P_curve, R_curve, F1_curve = [], [], []
    for TP, FP in zip(tp_ge.tolist(), fp_ge.tolist()):                       # p_r_f1.py:120-124
        FN = total_gt - TP
        P = TP / (TP + FP) if (TP + FP) > 0 else 0.0
        R = TP / (TP + FN) if (TP + FN) > 0 else 0.0
        F1 = 2 * P * R / (P + R) if (P + R) > 0 else 0.0
        P_curve.append(P); R_curve.append(R); F1_curve.append(F1)
    P_curve = np.array(P_curve); R_curve = np.array(R_curve); F1_curve = np.array(F1_curve)
    best_idx = int(np.argmax(F1_curve))
    fixed_conf = 0.50
    idx = int(np.argmin(np.abs(confs - fixed_conf)))

    # score-ranked PR curve (p_r_f1.py:56-95; computed by the reference, not part of its summary)
    order = np.lexsort((np.arange(len(d_sc)), -d_sc))
    cum_tp = np.cumsum(tp[order].astype(np.float64))
    cum_fp = np.cumsum(1.0 - tp[order].astype(np.float64))
    return {
        "iou": float(iou), "best_f1": float(F1_curve[best_idx]), "best_conf": float(confs[best_idx]),
        "precision_at_best": float(P_curve[best_idx]), "recall_at_best": float(R_curve[best_idx]),
        "fixed_conf": fixed_conf, "precision_at_fixed_conf": float(P_curve[idx]),
        "recall_at_fixed_conf": float(R_curve[idx]), "f1_at_fixed_conf": float(F1_curve[idx]),
        "P_curve": P_curve, "R_curve": R_curve, "F1_curve": F1_curve, "confs": confs, "best_idx": best_idx,
        "recalls_rank": cum_tp / max(1, total_gt), "precisions_rank": cum_tp / np.maximum(1, cum_tp + cum_fp),
    }


# ------------------------------------------------------------------------------ confusion matrix
def confusion_matrix_counts(coco_anns, coco_dets, num_classes, iou_thresh=0.5, score_thresh=0.20, device=None):
    """Raw detection confusion matrix of evaluate.py:80-156: int64 [(C+1),(C+1)], row = true class,
    column = predicted class, last index = background.  category_id must be 1..C (KeyError otherwise,
    as in the reference)."""
    lib = _lib.load()
    dev = _dev(device)
    C = int(num_classes)

    def idx(cids):
        cids = np.asarray(cids, dtype=np.int64)
        bad = (cids < 1) | (cids > C)
        if bad.any():
            raise KeyError(int(cids[bad][0]))
        return (cids - 1).astype(np.int32)

    W = C + 1
    if len(coco_anns) == 0:
        return np.zeros((W, W), dtype=np.int64)
    g_img = np.array([a["image_id"] for a in coco_anns], dtype=np.int64)
    g_cls = idx([a["category_id"] for a in coco_anns])
    g_b = np.array([a["bbox"] for a in coco_anns], dtype=np.float64).reshape(-1, 4)
    img_ids, g_key = np.unique(g_img, return_inverse=True)                   # images WITH ground truth
    g_key = g_key.reshape(-1)
    ni = len(img_ids)
    gorder = np.argsort(g_key, kind="stable")

    def xyxy32(b):                                                           # evaluate.py:23-25
        return np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1).astype(np.float32)

    if len(coco_dets):
        d_img = np.array([d["image_id"] for d in coco_dets], dtype=np.int64)
        d_sc = np.array([d.get("score", 0.0) for d in coco_dets], dtype=np.float64)
        pos = np.searchsorted(img_ids, d_img)
        pos_c = np.minimum(pos, ni - 1)
        keep = (img_ids[pos_c] == d_img) & (d_sc >= score_thresh)            # :101-104
        sel = np.nonzero(keep)[0]
    else:
        sel = np.zeros(0, dtype=np.int64)
    if len(sel):
        d_key = pos_c[sel]
        d_cls = idx([coco_dets[i]["category_id"] for i in sel])
        d_b = np.array([coco_dets[i]["bbox"] for i in sel], dtype=np.float64).reshape(-1, 4)
        dorder = np.lexsort((np.arange(len(sel)), -d_sc[sel], d_key))        # :107 stable, score descending
        det_off = _offsets(d_key[dorder], ni)
        t_det, t_dcls = _up(xyxy32(d_b[dorder]), dev), _up(d_cls[dorder], dev)
    else:
        det_off = np.zeros(ni + 1, dtype=np.int32)
        t_det = t_dcls = None
    gt_off = _offsets(g_key[gorder], ni)
    t_gt, t_gcls = _up(xyxy32(g_b[gorder]), dev), _up(g_cls[gorder], dev)
    t_doff, t_goff = _up(det_off, dev), _up(gt_off, dev)
    t_cm = torch.empty(W * W, dtype=torch.int32, device=dev)
    t_gm = torch.empty(len(g_img), dtype=torch.uint8, device=dev)
    with _timed_launch(dev):
        _lib.check(lib.yl_eval_confusion(_ptr(t_det), _ptr(t_dcls), _ptr(t_doff), _ptr(t_gt), _ptr(t_gcls), _ptr(t_goff),
                                         ni, len(g_img), C, float(np.float32(iou_thresh)), _ptr(t_cm), _ptr(t_gm),
                                         _stream(dev)), what="yl_eval_confusion")
    return t_cm.cpu().numpy().reshape(W, W).astype(np.int64)


def confusion_stats(cm):
    """evaluate.py:158-200."""
    C = cm.shape[0] - 1
    tp = np.diag(cm)[:-1]
    fn = cm[:-1, C]
    fp = cm[C, :-1]
    prec = np.divide(tp, tp + fp, out=np.zeros_like(tp, dtype=float), where=(tp + fp) != 0)
    rec = np.divide(tp, tp + fn, out=np.zeros_like(tp, dtype=float), where=(tp + fn) != 0)
    return {"tp": tp, "fp": fp, "fn": fn, "precision": prec, "recall": rec,
            "total_fp": int(fp.sum()), "total_fn": int(fn.sum())}


def create_confusion_matrix(coco_anns, coco_dets, class_names, SAVE_PATH, filename="confusion_matrix.png",
                            title="Detection Confusion Matrix", iou_thresh=0.5, score_thresh=0.20, device=None):
    """Drop-in for scripts/helpers/evaluate.py:59-238: writes
    <SAVE_PATH>/confusion_matrices/<filename>_stats.txt exactly like the reference.  Returns the raw
    matrix (the reference returns None); the seaborn heat map is not drawn."""
    save_dir = os.path.join(SAVE_PATH, "confusion_matrices")
    os.makedirs(save_dir, exist_ok=True)
    cm = confusion_matrix_counts(coco_anns, coco_dets, len(class_names), iou_thresh, score_thresh, device=device)
    st = confusion_stats(cm)
    with open(os.path.join(save_dir, filename.replace(".png", "_stats.txt")), "w") as f:
        f.write(f"Total FP: {st['total_fp']}\n")
        f.write(f"Total FN: {st['total_fn']}\n\n")
        f.write("Class\tTP\tFP\tFN\tPrecision\tRecall\n")
        for i, cls in enumerate(class_names):
            f.write(f"{cls}\t{int(st['tp'][i])}\t{int(st['fp'][i])}\t{int(st['fn'][i])}\t"
                    f"{st['precision'][i]:.3f}\t{st['recall'][i]:.3f}\n")
    return cm


# ------------------------------------------------------------------------------ COCO bbox mAP
# pycocotools 2.0 COCOeval, iouType="bbox", default Params (the reference's _coco_eval_from_lists,
# scripts/helpers/helpers.py:155-227).  The host converts, filters, groups, sorts and counts; evaluateImg
# runs in yl_eval_coco_match and accumulate in yl_eval_coco_accumulate; summarize is the numpy mean below.
COCO_AREA_LBL = ["all", "small", "medium", "large"]


def coco_default_params(num_classes, img_ids):
    """COCOeval Params() for iouType="bbox" (the arrays are passed to the device as they are here:
    iouThrs[8] is 0.8999999999999999, not 0.9)."""
    return {"imgIds": [int(i) for i in np.unique(np.asarray(img_ids, dtype=np.int64))],
            "catIds": list(range(1, int(num_classes) + 1)),
            "iouThrs": np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True),
            "recThrs": np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True),
            "maxDets": [1, 10, 100],
            "areaRng": [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]],
            "areaRngLbl": list(COCO_AREA_LBL)}


def _coco_summary_specs(p):
    md = p["maxDets"]
    return [(1, None, "all", md[2]), (1, .5, "all", md[2]), (1, .75, "all", md[2]), (1, None, "small", md[2]),
            (1, None, "medium", md[2]), (1, None, "large", md[2]), (0, None, "all", md[0]), (0, None, "all", md[1]),
            (0, None, "all", md[2]), (0, None, "small", md[2]), (0, None, "medium", md[2]),
            (0, None, "large", md[2])]


def coco_summarize(precision, recall, p):
    """COCOeval.summarize() -> stats[12]: np.mean(s[s > -1]) (or -1) over the slices of _summarizeDets."""
    stats = np.zeros((12,))
    for n, (ap, thr, area, max_dets) in enumerate(_coco_summary_specs(p)):
        aind = [i for i, lbl in enumerate(p["areaRngLbl"]) if lbl == area]
        mind = [i for i, m in enumerate(p["maxDets"]) if m == max_dets]
        s = precision if ap == 1 else recall
        if thr is not None:
            s = s[np.where(thr == p["iouThrs"])[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        stats[n] = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
    return stats


def coco_summary_lines(stats, p=None):
    """The 12 lines COCOeval.summarize() prints."""
    p = p or coco_default_params(1, [])
    i_str = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}"
    lines = []
    for n, (ap, thr, area, max_dets) in enumerate(_coco_summary_specs(p)):
        iou = "{:0.2f}:{:0.2f}".format(p["iouThrs"][0], p["iouThrs"][-1]) if thr is None else "{:0.2f}".format(thr)
        lines.append(i_str.format("Average Precision" if ap == 1 else "Average Recall", "(AP)" if ap == 1 else "(AR)",
                                  iou, area, max_dets, stats[n]))
    return lines


def coco_per_class(precision, p):
    """Per-category AP (IoU .50:.95) and AP50 at area "all", maxDets 100, with summarize's mean rule."""
    m = p["maxDets"].index(100) if 100 in p["maxDets"] else len(p["maxDets"]) - 1
    t50 = np.where(.5 == p["iouThrs"])[0]
    out = []
    for k, cid in enumerate(p["catIds"]):
        s, s50 = precision[:, :, k, 0, m], precision[t50, :, k, 0, m]
        out.append({"category_id": int(cid),
                    "AP": float(np.mean(s[s > -1])) if (s > -1).any() else -1.0,
                    "AP50": float(np.mean(s50[s50 > -1])) if (s50 > -1).any() else -1.0})
    return out


def coco_eval(coco_images, coco_anns, coco_dets, num_classes=None, device=None):
    """COCO bbox evaluation (pycocotools 2.0 COCOeval evaluate + accumulate + summarize, default Params) of
    the reference's list-of-dicts inputs.  Returns {"stats": float64[12], "precision": [T,R,K,A,M],
    "recall": [T,K,A,M], "params": dict}.  `num_classes` defaults to the largest category id of the ground
    truths (or detections).  A detection on an image that is not in coco_images raises ValueError
    (pycocotools' loadRes asserts); ground truths and detections of other categories are dropped."""
    lib = _lib.load()
    dev = _dev(device)
    coco_images = coco_images or []
    if num_classes is None:
        src = coco_anns if len(coco_anns) else coco_dets
        num_classes = int(max(1, max((int(o["category_id"]) for o in src), default=1)))
    p = coco_default_params(num_classes, [int(im["id"]) for im in coco_images])
    img_ids = np.asarray(p["imgIds"], dtype=np.int64)
    K, A, T = len(p["catIds"]), len(p["areaRng"]), len(p["iouThrs"])
    R, M = len(p["recThrs"]), len(p["maxDets"])
    area_rng = np.asarray(p["areaRng"], dtype=np.float64)

    def img_index(ids):                                  # position in the sorted imgIds, -1 if absent
        pos = np.searchsorted(img_ids, ids)
        ok = pos < len(img_ids)
        ok[ok] = img_ids[pos[ok]] == ids[ok]
        return np.where(ok, pos, -1)

    # detections (loadRes: area = w*h, never crowd; ids 1..N only need to be nonzero)
    nd0 = len(coco_dets)
    d_img = np.array([int(d["image_id"]) for d in coco_dets], dtype=np.int64)
    d_cat = np.array([int(d["category_id"]) for d in coco_dets], dtype=np.int64)
    d_box = np.array([[float(v) for v in d["bbox"]] for d in coco_dets], dtype=np.float64).reshape(nd0, 4)
    d_sc = np.array([float(d["score"]) for d in coco_dets], dtype=np.float64)
    d_ii = img_index(d_img)
    if (d_ii < 0).any():
        raise ValueError(f"Results do not correspond to current coco set: image_id {int(d_img[d_ii < 0][0])} "
                         "is not in coco_images")
    # ground truths (area = the annotation's field, ignore = iscrowd)
    ng0 = len(coco_anns)
    g_img = np.array([int(a["image_id"]) for a in coco_anns], dtype=np.int64)
    g_cat = np.array([int(a["category_id"]) for a in coco_anns], dtype=np.int64)
    g_box = np.array([[float(v) for v in a["bbox"]] for a in coco_anns], dtype=np.float64).reshape(ng0, 4)
    g_area = np.array([float(a["area"]) for a in coco_anns], dtype=np.float64)
    g_crowd = np.array([bool(a.get("iscrowd", 0)) for a in coco_anns], dtype=bool)
    g_idnz = np.array([int(a["id"]) != 0 for a in coco_anns], dtype=bool)
    g_ii = img_index(g_img)
    for name, arr in (("detection bbox", d_box), ("detection score", d_sc), ("annotation bbox", g_box),
                      ("annotation area", g_area)):
        if not np.isfinite(arr).all():
            raise ValueError(f"coco_eval: non-finite {name}")

    dk = np.nonzero((d_cat >= 1) & (d_cat <= K))[0]
    gk = np.nonzero((g_ii >= 0) & (g_cat >= 1) & (g_cat <= K))[0]
    # detections key-major (category, image), -score stable within the key, truncated to maxDets[-1]
    dk = dk[np.lexsort((dk, -d_sc[dk], d_ii[dk], d_cat[dk]))]
    dkey = (d_cat[dk] - 1) * len(img_ids) + d_ii[dk]
    first = np.r_[True, dkey[1:] != dkey[:-1]] if len(dk) else np.zeros(0, bool)
    start = np.maximum.accumulate(np.where(first, np.arange(len(dk)), 0)) if len(dk) else np.zeros(0, np.int64)
    rank = np.arange(len(dk)) - start
    keep = rank < p["maxDets"][-1]
    dk, dkey, rank = dk[keep], dkey[keep], rank[keep]
    nd = len(dk)
    keys = np.unique(dkey)                               # keys with detections, sorted (category, image)
    nk = len(keys)
    det_off = np.zeros(nk + 1, dtype=np.int32)
    det_off[1:] = np.searchsorted(dkey, keys, side="right")
    # ground truths of those keys, list order within the key
    gkey = (g_cat[gk] - 1) * len(img_ids) + g_ii[gk]
    gsel = gk[np.isin(gkey, keys)]
    gsel_key = (g_cat[gsel] - 1) * len(img_ids) + g_ii[gsel]
    go = np.argsort(np.searchsorted(keys, gsel_key), kind="stable")
    gsel, gsel_key = gsel[go], gsel_key[go]
    ng = len(gsel)
    gt_off = np.zeros(nk + 1, dtype=np.int32)
    gt_off[1:] = np.searchsorted(gsel_key, keys, side="right")
    # npig[k][a]: non-ignored ground truths of category k in area range a
    npig = np.zeros((K, A), dtype=np.int32)
    for a in range(A):
        lo, hi = area_rng[a]
        ok = ~g_crowd[gk] & ~((g_area[gk] < lo) | (g_area[gk] > hi))
        npig[:, a] = np.bincount(g_cat[gk][ok] - 1, minlength=K)[:K]
    # accumulate order per category: -score, then image id, then rank (stable over the key-major rows)
    order = np.lexsort((np.arange(nd), -d_sc[dk], d_cat[dk])).astype(np.int32)
    cat_off = np.zeros(K + 1, dtype=np.int32)
    cat_off[1:] = np.cumsum(np.bincount(d_cat[dk] - 1, minlength=K)[:K])

    t_area, t_iou = _up(area_rng, dev), _up(p["iouThrs"].astype(np.float64), dev)
    t_flags = torch.empty(max(A * T * nd, 1), dtype=torch.uint8, device=dev)
    if nd:
        gflags = (g_crowd[gsel].astype(np.uint8) * 1) | (g_idnz[gsel].astype(np.uint8) * 2)
        t_det, t_doff, t_goff = _up(d_box[dk], dev), _up(det_off, dev), _up(gt_off, dev)
        t_gt = _up(g_box[gsel], dev) if ng else None
        t_garea = _up(g_area[gsel], dev) if ng else None
        t_gfl = _up(gflags, dev) if ng else None
        t_gm = torch.empty(max(A * ng, 1), dtype=torch.int32, device=dev)
        with _timed_launch(dev, "coco_match"):
            _lib.check(lib.yl_eval_coco_match(_ptr(t_det), _ptr(t_doff), _ptr(t_gt), _ptr(t_garea), _ptr(t_gfl),
                                              _ptr(t_goff), nk, nd, ng, _ptr(t_area), A, _ptr(t_iou), T,
                                              _ptr(t_flags), _ptr(t_gm), _stream(dev)), what="yl_eval_coco_match")
    t_order = _up(order, dev) if nd else None
    t_rank = _up(rank[order].astype(np.int32), dev) if nd else None
    t_coff, t_npig = _up(cat_off, dev), _up(npig, dev)
    t_md, t_rec = _up(np.asarray(p["maxDets"], np.int32), dev), _up(p["recThrs"].astype(np.float64), dev)
    t_prec = torch.empty(T * R * K * A * M, dtype=torch.float64, device=dev)
    t_recall = torch.empty(T * K * A * M, dtype=torch.float64, device=dev)
    with _timed_launch(dev, "coco_accumulate"):
        _lib.check(lib.yl_eval_coco_accumulate(_ptr(t_order), _ptr(t_rank), _ptr(t_coff), _ptr(t_flags) if nd else None,
                                               nd, _ptr(t_npig), K, A, T, _ptr(t_md), M, _ptr(t_rec), R,
                                               _ptr(t_prec), _ptr(t_recall), _stream(dev)),
                   what="yl_eval_coco_accumulate")
    precision = t_prec.cpu().numpy().reshape(T, R, K, A, M)
    recall = t_recall.cpu().numpy().reshape(T, K, A, M)
    return {"stats": coco_summarize(precision, recall, p), "precision": precision, "recall": recall, "params": p}


def _coco_eval_from_lists(coco_images, coco_anns, coco_dets, iouType="bbox", num_classes=None, device=None):
    """Drop-in for the reference's _coco_eval_from_lists (scripts/helpers/helpers.py:155-227): the same dict
    (AP, AP50, AP75, APS, APM, APL, AR = AR@100, ARS, ARM, ARL), the same 7-key zero dict when there are no
    detections, computed by coco_eval on the device instead of pycocotools."""
    if iouType != "bbox":
        raise ValueError(f"iouType {iouType!r} is not supported (bbox only)")
    if not coco_dets:
        return {"AP": 0.0, "AP50": 0.0, "AP75": 0.0, "APS": 0.0, "APM": 0.0, "APL": 0.0, "AR": 0.0}
    if num_classes is None:
        if len(coco_anns):
            num_classes = int(max(1, max(a["category_id"] for a in coco_anns)))
        else:
            num_classes = int(max(1, max((d["category_id"] for d in coco_dets), default=1)))
    s = coco_eval(coco_images, coco_anns, coco_dets, num_classes=num_classes, device=device)["stats"]
    return {"AP": float(s[0]), "AP50": float(s[1]), "AP75": float(s[2]), "APS": float(s[3]), "APM": float(s[4]),
            "APL": float(s[5]), "AR": float(s[8]), "ARS": float(s[9]), "ARM": float(s[10]), "ARL": float(s[11])}
