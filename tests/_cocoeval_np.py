"""Loop-for-loop numpy restatement of pycocotools 2.0 COCOeval (iouType="bbox", default Params), starting
from the list-of-dicts inputs of the reference's _coco_eval_from_lists (scripts/helpers/helpers.py:155-227):
COCO(gt) + loadRes(dets) -> evaluate() -> accumulate() -> summarize().

Test infrastructure only: the product (evalops.coco_eval, on the device) never imports it.  pycocotools
itself is not a dependency, so this file restates its behaviour; tests/test_coco_eval_cpu.py holds it to
hand-derived cases and tests/test_coco_eval_gpu.py holds the device path to it, bit for bit."""
from collections import defaultdict

import numpy as np

AREA_LBL = ["all", "small", "medium", "large"]


def default_params(num_classes, img_ids):
    return {"imgIds": list(np.unique(np.asarray(img_ids, dtype=np.int64))) if len(img_ids) else [],
            "catIds": list(range(1, int(num_classes) + 1)),
            "iouThrs": np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True),
            "recThrs": np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True),
            "maxDets": [1, 10, 100],
            "areaRng": [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]}


def bb_iou(d, g, iscrowd):
    """maskApi.c bbIou: o[d][g], float64, one rounding per operation."""
    o = np.zeros((len(d), len(g)))
    for gi, G in enumerate(g):
        ga = G[2] * G[3]
        crowd = bool(iscrowd[gi])
        for di, D in enumerate(d):
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if crowd else (da + ga) - i
            o[di, gi] = i / u
    return o


def _prepare(coco_images, coco_anns, coco_dets, p):
    img_set = set(int(im["id"]) for im in (coco_images or []))
    for d in coco_dets:                                     # loadRes: every result image must be a GT image
        if int(d["image_id"]) not in img_set:
            raise ValueError("Results do not correspond to current coco set")
    dts = []
    for n, d in enumerate(coco_dets):                       # loadRes (bbox): id, area, iscrowd
        bb = [float(v) for v in d["bbox"]]
        dts.append({"id": n + 1, "image_id": int(d["image_id"]), "category_id": int(d["category_id"]),
                    "bbox": bb, "score": float(d["score"]), "area": bb[2] * bb[3], "iscrowd": 0})
    cats = set(p["catIds"])
    imgs = set(int(i) for i in p["imgIds"])
    gts_k, dts_k = defaultdict(list), defaultdict(list)
    for a in coco_anns:
        if int(a["image_id"]) in imgs and int(a["category_id"]) in cats:
            g = {"id": int(a["id"]), "bbox": [float(v) for v in a["bbox"]], "area": float(a["area"]),
                 "iscrowd": int(bool(a.get("iscrowd", 0)))}
            g["ignore"] = g["iscrowd"]
            gts_k[int(a["image_id"]), int(a["category_id"])].append(g)
    for d in dts:
        if d["image_id"] in imgs and d["category_id"] in cats:
            dts_k[d["image_id"], d["category_id"]].append(d)
    return gts_k, dts_k


def _compute_iou(gt, dt, max_det):
    if len(gt) == 0 and len(dt) == 0:
        return []
    inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
    dt = [dt[i] for i in inds][:max_det]
    if len(dt) == 0 or len(gt) == 0:
        return []
    return bb_iou([d["bbox"] for d in dt], [g["bbox"] for g in gt], [g["iscrowd"] for g in gt])


def _evaluate_img(gt, dt, ious, a_rng, max_det, iou_thrs):
    if len(gt) == 0 and len(dt) == 0:
        return None
    gt_ig_l = [1 if (g["ignore"] or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0 for g in gt]
    gtind = np.argsort(gt_ig_l, kind="mergesort")
    gt = [gt[i] for i in gtind]
    dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
    dt = [dt[i] for i in dtind[0:max_det]]
    iscrowd = [int(o["iscrowd"]) for o in gt]
    ious = ious[:, gtind] if len(ious) > 0 else ious
    T, G, D = len(iou_thrs), len(gt), len(dt)
    gtm = np.zeros((T, G))
    dtm = np.zeros((T, D))
    gt_ig = np.array([gt_ig_l[i] for i in gtind])
    dt_ig = np.zeros((T, D))
    if not len(ious) == 0:
        for tind, t in enumerate(iou_thrs):
            for dind, d in enumerate(dt):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind, g in enumerate(gt):
                    if gtm[tind, gind] > 0 and not iscrowd[gind]:
                        continue
                    if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                        break
                    if ious[dind, gind] < iou:
                        continue
                    iou = ious[dind, gind]
                    m = gind
                if m == -1:
                    continue
                dt_ig[tind, dind] = gt_ig[m]
                dtm[tind, dind] = gt[m]["id"]
                gtm[tind, m] = d["id"]
    a = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dt]).reshape((1, len(dt)))
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
    return {"dtMatches": dtm, "dtScores": [d["score"] for d in dt], "gtIgnore": gt_ig, "dtIgnore": dt_ig}


def evaluate_accumulate(coco_images, coco_anns, coco_dets, num_classes):
    """-> (precision [T,R,K,A,M], recall [T,K,A,M], params)."""
    p = default_params(num_classes, [im["id"] for im in (coco_images or [])])
    gts_k, dts_k = _prepare(coco_images, coco_anns, coco_dets, p)
    max_det = p["maxDets"][-1]
    ious = {(i, c): _compute_iou(gts_k[i, c], dts_k[i, c], max_det) for i in p["imgIds"] for c in p["catIds"]}
    eval_imgs = [_evaluate_img(gts_k[i, c], dts_k[i, c], ious[i, c], a, max_det, p["iouThrs"])
                 for c in p["catIds"] for a in p["areaRng"] for i in p["imgIds"]]

    T, R = len(p["iouThrs"]), len(p["recThrs"])
    K, A, M = len(p["catIds"]), len(p["areaRng"]), len(p["maxDets"])
    I0 = len(p["imgIds"])
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k in range(K):
        for a in range(A):
            for m, md in enumerate(p["maxDets"]):
                E = [eval_imgs[k * A * I0 + a * I0 + i] for i in range(I0)]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([e["dtScores"][0:md] for e in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                dtm = np.concatenate([e["dtMatches"][:, 0:md] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtIgnore"][:, 0:md] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp, fp = np.array(tp), np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist(); q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, p["recThrs"], side="left")
                    try:
                        for ri, pi in enumerate(inds_r):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
    return precision, recall, p


def summarize(precision, recall, p):
    """COCOeval.summarize()._summarizeDets -> stats[12]."""
    def _s(ap=1, iou_thr=None, area="all", max_dets=100):
        aind = [i for i, lbl in enumerate(AREA_LBL) if lbl == area]
        mind = [i for i, md in enumerate(p["maxDets"]) if md == max_dets]
        if ap == 1:
            s = precision
            if iou_thr is not None:
                s = s[np.where(iou_thr == p["iouThrs"])[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = recall
            if iou_thr is not None:
                s = s[np.where(iou_thr == p["iouThrs"])[0]]
            s = s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    md = p["maxDets"]
    return np.array([_s(1), _s(1, iou_thr=.5, max_dets=md[2]), _s(1, iou_thr=.75, max_dets=md[2]),
                     _s(1, area="small", max_dets=md[2]), _s(1, area="medium", max_dets=md[2]),
                     _s(1, area="large", max_dets=md[2]), _s(0, max_dets=md[0]), _s(0, max_dets=md[1]),
                     _s(0, max_dets=md[2]), _s(0, area="small", max_dets=md[2]),
                     _s(0, area="medium", max_dets=md[2]), _s(0, area="large", max_dets=md[2])], dtype=np.float64)


def coco_eval_np(coco_images, coco_anns, coco_dets, num_classes):
    precision, recall, p = evaluate_accumulate(coco_images, coco_anns, coco_dets, num_classes)
    return {"stats": summarize(precision, recall, p), "precision": precision, "recall": recall, "params": p}


def coco_eval_from_lists_np(coco_images, coco_anns, coco_dets, num_classes=None):
    """The reference's _coco_eval_from_lists on top of the restatement (same dict, same early return)."""
    if not coco_dets:
        return {"AP": 0.0, "AP50": 0.0, "AP75": 0.0, "APS": 0.0, "APM": 0.0, "APL": 0.0, "AR": 0.0}
    if num_classes is None:
        if len(coco_anns):
            num_classes = int(max(1, max(a["category_id"] for a in coco_anns)))
        else:
            num_classes = int(max(1, max((d["category_id"] for d in coco_dets), default=1)))
    s = coco_eval_np(coco_images, coco_anns, coco_dets, num_classes)["stats"]
    return {"AP": float(s[0]), "AP50": float(s[1]), "AP75": float(s[2]), "APS": float(s[3]), "APM": float(s[4]),
            "APL": float(s[5]), "AR": float(s[8]), "ARS": float(s[9]), "ARM": float(s[10]), "ARL": float(s[11])}
