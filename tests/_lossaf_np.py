"""Plain numpy restatement of the reference's LossAF.forward (scripts/loss/loss.py:283-436), written from its
semantics: anchor grid, train-time decode, centre mask AND level gate, orphan rescue, the six-term cost, dynamic-k
SimOTA matching with the conflict pass, then CIoU / label-smoothed cross-entropy / BCE with hard negatives.

`dtype` selects the arithmetic (float64 by default; float32 gives the size of an fp32 implementation's own error).
Besides the loss it returns what the reference keeps to itself: the per-image parts and the assignment
(`assign[b, n]` = index of the box anchor n was matched to, counted over the whole batch, or -1).
tests/test_loss_af_cpu.py holds it to the fixtures the reference itself produced (tests/golden/loss_af.npz)."""
import math

import numpy as np

DEFAULTS = dict(lambda_box=5.0, lambda_obj=1.0, lambda_cls=0.5, assign_cls_weight=0.5, center_mode="v8",
                wh_mode="softplus", center_radius_cells=2.0, topk_limit=20, cls_smoothing=0.05, area_cells_min=4.0,
                area_cells_max=256.0, area_tol=1.25, size_prior_w=0.20, ar_prior_w=0.10, iou_cost_w=3.0,
                center_cost_w=0.5)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _softplus(x):
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def _bce_logits(x, t):
    # (1 - t) * x - log_sigmoid(x)
    return (1.0 - t) * x - (np.minimum(x, 0.0) - np.log1p(np.exp(-np.abs(x))))


def _seq_sum(v, dt):
    """sum along axis 0, first row first, in the working precision"""
    s = np.zeros(v.shape[1:], dt)
    for r in v:
        s = (s + r).astype(dt)
    return s


def _mean(v, dt):
    # float64 accumulation, one rounding: what a careful fp32 implementation can do
    return dt(np.sum(v.astype(np.float64)) / v.size)


def decode(levels, img_size, center_mode, wh_mode, dt):
    """levels: list of [B,1,h,w,E] -> flat rows [B,N,E], boxes [B,N,4], centres [B,N,2], sizes [B,N,2], strides [N]"""
    flat, anc, strd = [], [], []
    for p in levels:
        _, a, h, w, _ = p.shape
        assert a == 1, "one anchor per cell"
        flat.append(np.asarray(p, dt).reshape(p.shape[0], h * w, p.shape[-1]))
        sy, sx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        anc.append(np.stack([sx, sy], -1).reshape(-1, 2).astype(dt))
        strd.append(np.full((h * w,), np.float32(img_size / max(h, w)) if dt == np.float32 else img_size / max(h, w), dt))
    flat = np.concatenate(flat, 1)
    anc, strd = np.concatenate(anc, 0), np.concatenate(strd, 0)
    s = strd[None, :, None]
    sig = _sigmoid(flat[..., 0:2])
    if center_mode == "v8":
        xy = (sig * dt(2.0) - dt(0.5) + anc[None]) * s
    else:
        xy = (sig + anc[None]) * s
    t = flat[..., 2:4]
    if wh_mode == "v8":
        q = _sigmoid(t) * dt(2.0)
        wh = q * q * s
    elif wh_mode == "softplus":
        wh = _softplus(t) * s
    else:
        wh = np.exp(np.clip(t, -10.0, 8.0)) * s
    xyxy = np.concatenate([xy - dt(0.5) * wh, xy + dt(0.5) * wh], -1)
    return flat, xyxy.astype(dt), xy.astype(dt), wh.astype(dt), strd


def _iou_matrix(a, g32, dt):
    """g32: float32 target boxes.  Quantities of the targets alone are float32 whatever `dt` is: the reference casts its
    targets to float32, and torch only promotes where a prediction enters the expression."""
    a2 = (np.maximum(g32[:, 2] - g32[:, 0], 0) * np.maximum(g32[:, 3] - g32[:, 1], 0))[None].astype(dt)
    a, g = a[:, None, :], g32.astype(dt)[None, :, :]
    iw = np.maximum(np.minimum(a[..., 2], g[..., 2]) - np.maximum(a[..., 0], g[..., 0]), 0)
    ih = np.maximum(np.minimum(a[..., 3], g[..., 3]) - np.maximum(a[..., 1], g[..., 1]), 0)
    inter = iw * ih
    a1 = np.maximum(a[..., 2] - a[..., 0], 0) * np.maximum(a[..., 3] - a[..., 1], 0)
    return (inter / (a1 + a2 - inter + dt(1e-7))).astype(dt)


def _ciou(p, t32, dt):
    eps = dt(1e-7)
    f = np.float32
    pw, ph = np.maximum(p[:, 2] - p[:, 0], eps), np.maximum(p[:, 3] - p[:, 1], eps)
    tw32, th32 = np.maximum(t32[:, 2] - t32[:, 0], f(1e-7)), np.maximum(t32[:, 3] - t32[:, 1], f(1e-7))
    tarea, tatan = (tw32 * th32).astype(dt), np.arctan((tw32 / th32).astype(np.float64)).astype(f).astype(dt)
    tcx, tcy = ((t32[:, 0] + t32[:, 2]) * f(0.5)).astype(dt), ((t32[:, 1] + t32[:, 3]) * f(0.5)).astype(dt)
    t = t32.astype(dt)
    iw = np.maximum(np.minimum(p[:, 2], t[:, 2]) - np.maximum(p[:, 0], t[:, 0]), 0)
    ih = np.maximum(np.minimum(p[:, 3], t[:, 3]) - np.maximum(p[:, 1], t[:, 1]), 0)
    inter = iw * ih
    iou = inter / (pw * ph + tarea - inter + eps)
    dx = (p[:, 0] + p[:, 2]) * dt(0.5) - tcx
    dy = (p[:, 1] + p[:, 3]) * dt(0.5) - tcy
    cd = dx * dx + dy * dy
    cw = np.maximum(p[:, 2], t[:, 2]) - np.minimum(p[:, 0], t[:, 0])
    ch = np.maximum(p[:, 3], t[:, 3]) - np.minimum(p[:, 1], t[:, 1])
    c2 = cw * cw + ch * ch + eps
    d = tatan - np.arctan(pw / ph)
    v = dt(4 / (math.pi ** 2)) * (d * d)
    alpha = v / (v - iou + dt(1) + eps)
    return (iou - cd / c2 - alpha * v).astype(dt)


def _neg_term(neg, k, dt):
    k = min(k, neg.size)
    if k <= 0:
        return dt(0)
    return _mean(np.sort(neg)[::-1][:k], dt)


def loss_af(levels, gt_xyxy, gt_label, gt_off, num_classes, img_size, dtype=np.float64, keep_costs=False, **kw):
    """levels: list of [B,1,h,w,5+C(+...)] arrays; gt_xyxy [T,4] pixel boxes; gt_label [T]; gt_off [B+1].
    Returns dict(box, obj, cls, pos, per_image [B,3], assign [B,N] int32); with keep_costs also "costs": per image
    (cost [N,G], dynamic_k [G]) or None, for explaining a contested choice."""
    cfg = dict(DEFAULTS)
    cfg.update({k: v for k, v in kw.items() if k in DEFAULTS})
    dt = np.dtype(dtype).type
    C = int(num_classes)
    flat, xyxy, ctr, wh, strd = decode(levels, img_size, cfg["center_mode"], cfg["wh_mode"], dt)
    B, N, _ = flat.shape
    amin = dt(np.float32(cfg["area_cells_min"] / cfg["area_tol"]) if dt == np.float32 else cfg["area_cells_min"] / cfg["area_tol"])
    amax = dt(cfg["area_cells_max"] * cfg["area_tol"])
    gt_xyxy = np.asarray(gt_xyxy, np.float32).reshape(-1, 4)
    f = np.float32
    gt_label = np.asarray(gt_label, np.int64).reshape(-1)
    per_image = np.zeros((B, 3), dt)
    assign = np.full((B, N), -1, np.int32)
    n_pos_img = 0
    costs = []
    kk = min(int(cfg["topk_limit"]), N)
    for b in range(B):
        g0, g1 = int(gt_off[b]), int(gt_off[b + 1])
        obj_logit = flat[b, :, 4]
        costs.append(None)
        if g1 > g0:
            tg, lab = gt_xyxy[g0:g1], gt_label[g0:g1]
            iou = _iou_matrix(xyxy[b], tg, dt)
            gc = ((tg[:, :2] + tg[:, 2:]) * f(0.5)).astype(dt)
            gwh32 = np.maximum(tg[:, 2:] - tg[:, :2], f(1.0))
            gwh = gwh32.astype(dt)
            dxy = ctr[b][:, None, :] - gc[None]
            dist = (dxy[..., 0] * dxy[..., 0] + dxy[..., 1] * dxy[..., 1]).astype(dt)
            s = strd[:, None]
            r = np.maximum(dt(cfg["center_radius_cells"]) * s + (f(0.10) * gwh32.max(1)).astype(dt)[None], dt(15.0))
            garea32 = gwh32[:, 0] * gwh32[:, 1]
            garea = garea32.astype(dt)[None]
            cells = garea / (s * s)
            valid = (dist <= r * r) & (cells >= amin) & (cells <= amax)
            for j in np.nonzero(valid.sum(0) == 0)[0]:
                valid[int(np.argmin(dist[:, j])), j] = True          # orphan rescue: first index on ties
            cls_cost = dt(1.0) - _sigmoid(flat[b][:, 5:5 + C][:, lab])
            obj_cost = -_sigmoid(obj_logit)[:, None]
            parea = (wh[b, :, 0] * wh[b, :, 1])[:, None]
            dl = np.abs(np.log(parea) - np.log(garea32).astype(dt)[None])
            size_cost = dl / (dt(1.0) + dl)
            da = np.abs(np.log(wh[b, :, 0] / wh[b, :, 1])[:, None] - np.log(gwh32[:, 0] / gwh32[:, 1]).astype(dt)[None])
            ar_cost = da / (dt(1.0) + da)
            cn = dist / (gwh32[:, 0] * gwh32[:, 0] + gwh32[:, 1] * gwh32[:, 1] + f(1e-6)).astype(dt)[None]
            cost = (dt(cfg["iou_cost_w"]) * (dt(1.0) - iou) + dt(cfg["assign_cls_weight"]) * cls_cost + obj_cost +
                    dt(cfg["center_cost_w"]) * cn + dt(cfg["size_prior_w"]) * size_cost + dt(cfg["ar_prior_w"]) * ar_cost)
            cost = np.where(valid, cost, dt(1e9)).astype(dt)
            top = -np.sort(-np.where(valid, iou, dt(0)), axis=0)[:kk]        # descending, as topk returns them
            dyn = np.maximum(_seq_sum(top, dt).astype(np.int64), 1)
            order = np.argsort(cost, axis=0, kind="stable")[:kk]
            if keep_costs:
                costs[-1] = (cost, dyn)
            best = np.full((N,), np.inf)
            for j in range(g1 - g0):
                for n in order[:dyn[j], j]:
                    cj = np.inf if np.isnan(cost[n, j]) else cost[n, j]      # a NaN cost orders above every number
                    if assign[b, n] < 0 or cj < best[n]:                       # strict: the lowest box index keeps a tie
                        best[n], assign[b, n] = cj, g0 + j
        pos = np.nonzero(assign[b] >= 0)[0]
        if pos.size == 0:
            per_image[b, 1] = dt(cfg["lambda_obj"]) * _neg_term(_bce_logits(obj_logit, dt(0)), 64, dt)
            continue
        n_pos_img += 1
        m = assign[b, pos]
        per_image[b, 0] = dt(cfg["lambda_box"]) * _mean(dt(1.0) - _ciou(xyxy[b, pos], gt_xyxy[m], dt), dt)
        if C > 1:
            z = flat[b, pos, 5:5 + C]
            zs = z - z.max(1, keepdims=True)
            logp = zs - np.log(np.exp(zs).sum(1, keepdims=True))
            e = dt(cfg["cls_smoothing"])
            ce = (dt(1.0) - e) * -logp[np.arange(pos.size), gt_label[m]] + e * (-logp.sum(1) / dt(C))
            per_image[b, 2] = dt(cfg["lambda_cls"]) * _mean(ce.astype(dt), dt)
        tgt = np.clip(iou[pos, m - g0], 0, 1)
        pos_obj = _mean(_bce_logits(obj_logit[pos], tgt).astype(dt), dt)
        neg = _bce_logits(np.delete(obj_logit, pos), dt(0)).astype(dt)
        per_image[b, 1] = dt(cfg["lambda_obj"]) * dt(pos_obj + _neg_term(neg, max(64, 3 * pos.size), dt))
    tot = _seq_sum(per_image, dt)
    return {"box": float(tot[0]), "obj": float(tot[1]), "cls": float(tot[2]), "pos": n_pos_img / max(B, 1),
            "per_image": per_image, "assign": assign, **({"costs": costs} if keep_costs else {})}
