"""Plain numpy restatement of the gradient of the reference's LossAF (scripts/loss/loss.py:258-276, 284-436) with
respect to the level tensors, derived by hand -- no autograd.  Nothing of the assignment is differentiated (top-k
indices, .int() and boolean masks carry no gradient, the objectness target is detached), so the assignment is taken
from _lossaf_np.loss_af and the gradient is closed-form per anchor:

  positive, columns 0-3    lambda_box / npos * d(1 - CIoU)/d(x1,y1,x2,y2), chained through the train-time decode
                           (alpha of CIoU a constant; exp sizes outside the clamp [-10, 8] have derivative 0)
  positive, column 4       lambda_obj / npos * (sigmoid(x) - clamp(IoU, 0, 1))
  positive, columns 5..    lambda_cls / npos * (softmax(z) - ((1 - e) * onehot + e / C));  0 for C = 1
  selected negative, col 4 lambda_obj / K * sigmoid(x);  K = min(max(64, 3 * npos), N - npos), the K largest
                           BCE(x, 0) among the non-positives, equal terms in anchor order
  everything else          0

Kinks follow torch: clamp passes the gradient at its boundary, binary max / min split it between equal arguments.
`dtype` selects the arithmetic (float64, or float32 for the size of an fp32 implementation's own error); quantities
of the targets alone stay float32 as in _lossaf_np.  tests/test_loss_af_grad_cpu.py holds it to the reference's own
autograd (tests/golden/loss_af_grad.npz)."""
import math

import numpy as np

from _lossaf_np import DEFAULTS, _bce_logits, _sigmoid, decode, loss_af


def _step(a, b):
    """d max(a, b)/da = d min(b, a)/db ...: 1 where a > b, 1/2 where equal, else 0"""
    return np.where(a > b, 1.0, np.where(a == b, 0.5, 0.0)).astype(np.result_type(a, b))


def ciou_grad(p, t32, dt):
    """d(1 - CIoU)/d(px1, py1, px2, py2) of the rows of p [n,4] against the float32 boxes t32 [n,4]"""
    eps = dt(1e-7)
    f = np.float32
    one, zero = dt(1), dt(0)
    wr, hr = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    pw, ph = np.maximum(wr, eps), np.maximum(hr, eps)
    mw, mh = (wr >= eps).astype(dt), (hr >= eps).astype(dt)
    tw32, th32 = np.maximum(t32[:, 2] - t32[:, 0], f(1e-7)), np.maximum(t32[:, 3] - t32[:, 1], f(1e-7))
    tarea, tatan = (tw32 * th32).astype(dt), np.arctan((tw32 / th32).astype(np.float64)).astype(f).astype(dt)
    tcx, tcy = ((t32[:, 0] + t32[:, 2]) * f(0.5)).astype(dt), ((t32[:, 1] + t32[:, 3]) * f(0.5)).astype(dt)
    t = t32.astype(dt)
    iwr = np.minimum(p[:, 2], t[:, 2]) - np.maximum(p[:, 0], t[:, 0])
    ihr = np.minimum(p[:, 3], t[:, 3]) - np.maximum(p[:, 1], t[:, 1])
    iw, ih = np.maximum(iwr, 0), np.maximum(ihr, 0)
    miw, mih = (iwr >= 0).astype(dt), (ihr >= 0).astype(dt)
    z = np.zeros_like(pw)
    # derivatives with respect to (x1, y1, x2, y2), one list entry per coordinate
    d_iw = [-miw * _step(p[:, 0], t[:, 0]), z, miw * _step(t[:, 2], p[:, 2]), z]
    d_ih = [z, -mih * _step(p[:, 1], t[:, 1]), z, mih * _step(t[:, 3], p[:, 3])]
    d_pw, d_ph = [-mw, z, mw, z], [z, -mh, z, mh]
    inter = iw * ih
    uni = pw * ph + tarea - inter + eps
    iou = inter / uni
    dx = (p[:, 0] + p[:, 2]) * dt(0.5) - tcx
    dy = (p[:, 1] + p[:, 3]) * dt(0.5) - tcy
    cd = dx * dx + dy * dy
    d_cd = [dx, dy, dx, dy]
    cw = np.maximum(p[:, 2], t[:, 2]) - np.minimum(p[:, 0], t[:, 0])
    ch = np.maximum(p[:, 3], t[:, 3]) - np.minimum(p[:, 1], t[:, 1])
    d_cw = [-_step(t[:, 0], p[:, 0]), z, _step(p[:, 2], t[:, 2]), z]
    d_ch = [z, -_step(t[:, 1], p[:, 1]), z, _step(p[:, 3], t[:, 3])]
    c2 = cw * cw + ch * ch + eps
    d = tatan - np.arctan(pw / ph)
    k4 = dt(4 / (math.pi ** 2))
    v = k4 * (d * d)
    alpha = v / (v - iou + one + eps)
    den = pw * pw + ph * ph
    out = np.zeros((len(p), 4), dt)
    for k in range(4):
        dinter = d_iw[k] * ih + iw * d_ih[k]
        duni = d_pw[k] * ph + pw * d_ph[k] - dinter
        diou = (dinter * uni - inter * duni) / (uni * uni)
        dc2 = dt(2) * cw * d_cw[k] + dt(2) * ch * d_ch[k]
        dpen = (d_cd[k] * c2 - cd * dc2) / (c2 * c2)
        dd = (-ph * d_pw[k] + pw * d_ph[k]) / den                 # d(-atan(pw / ph))
        dv = dt(2) * k4 * d * dd
        out[:, k] = -(diou - dpen - alpha * dv)
    return out.astype(dt) + zero


def _iou_pairs(a, g32, dt):
    """bbox_iou_matrix on matched pairs: a [n,4] predictions, g32 [n,4] float32 boxes"""
    a2 = (np.maximum(g32[:, 2] - g32[:, 0], 0) * np.maximum(g32[:, 3] - g32[:, 1], 0)).astype(dt)
    g = g32.astype(dt)
    iw = np.maximum(np.minimum(a[:, 2], g[:, 2]) - np.maximum(a[:, 0], g[:, 0]), 0)
    ih = np.maximum(np.minimum(a[:, 3], g[:, 3]) - np.maximum(a[:, 1], g[:, 1]), 0)
    inter = iw * ih
    a1 = np.maximum(a[:, 2] - a[:, 0], 0) * np.maximum(a[:, 3] - a[:, 1], 0)
    return (inter / (a1 + a2 - inter + dt(1e-7))).astype(dt)


def select_negatives(obj_logit, pos, dt):
    """-> (indices of the selected hard negatives in anchor order, K).  Equal terms are taken in anchor order."""
    N = obj_logit.shape[0]
    neg_idx = np.setdiff1d(np.arange(N), pos)
    K = min(max(64, 3 * len(pos)), len(neg_idx))
    if K <= 0:
        return np.zeros((0,), np.int64), 0
    term = _bce_logits(obj_logit[neg_idx], dt(0)).astype(dt)
    order = np.argsort(-term, kind="stable")[:K]          # stable: the lowest anchor index first among equal terms
    return np.sort(neg_idx[order]), K


def loss_af_grad(levels, gt_xyxy, gt_label, gt_off, num_classes, img_size, dtype=np.float64, assign=None, **kw):
    """-> dict(grad [B,N,E] (the level tensors' gradients, flattened and concatenated as the reference's preds_flat),
    pos / neg: per image the positive anchors and the selected negatives, K [B], assign [B,N])"""
    cfg = dict(DEFAULTS)
    cfg.update({k: v for k, v in kw.items() if k in DEFAULTS})
    dt = np.dtype(dtype).type
    C = int(num_classes)
    if assign is None:
        assign = loss_af(levels, gt_xyxy, gt_label, gt_off, num_classes, img_size, dtype=dtype, **kw)["assign"]
    flat, xyxy, ctr, wh, strd = decode(levels, img_size, cfg["center_mode"], cfg["wh_mode"], dt)
    B, N, E = flat.shape
    gt_xyxy = np.asarray(gt_xyxy, np.float32).reshape(-1, 4)
    gt_label = np.asarray(gt_label, np.int64).reshape(-1)
    grad = np.zeros((B, N, E), dt)
    poss, negs, Ks = [], [], []
    for b in range(B):
        pos = np.nonzero(assign[b] >= 0)[0]
        neg, K = select_negatives(flat[b, :, 4], pos, dt)
        poss.append(pos); negs.append(neg); Ks.append(K)
        if K > 0:
            grad[b, neg, 4] = dt(cfg["lambda_obj"]) / dt(K) * _sigmoid(flat[b, neg, 4])
        if pos.size == 0:
            continue
        m = assign[b, pos]
        npos = dt(pos.size)
        s = strd[pos]
        # columns 0-3: CIoU through the decode
        gxy = ciou_grad(xyxy[b, pos], gt_xyxy[m], dt)
        g_ctr = np.stack([gxy[:, 0] + gxy[:, 2], gxy[:, 1] + gxy[:, 3]], 1)
        g_wh = dt(0.5) * np.stack([gxy[:, 2] - gxy[:, 0], gxy[:, 3] - gxy[:, 1]], 1)
        t = flat[b, pos, 0:4]
        sg = _sigmoid(t)
        dctr = (dt(2.0) if cfg["center_mode"] == "v8" else dt(1.0)) * sg[:, 0:2] * (dt(1) - sg[:, 0:2]) * s[:, None]
        if cfg["wh_mode"] == "v8":
            dwh = dt(2) * (sg[:, 2:4] * dt(2)) * dt(2) * sg[:, 2:4] * (dt(1) - sg[:, 2:4]) * s[:, None]
        elif cfg["wh_mode"] == "softplus":
            dwh = np.where(t[:, 2:4] > 20.0, dt(1), sg[:, 2:4]) * s[:, None]
        else:
            dwh = np.where((t[:, 2:4] >= -10.0) & (t[:, 2:4] <= 8.0), wh[b, pos], dt(0))
        sb = dt(cfg["lambda_box"]) / npos
        grad[b, pos, 0:2] = sb * g_ctr * dctr
        grad[b, pos, 2:4] = sb * g_wh * dwh
        # column 4
        tgt = np.clip(_iou_pairs(xyxy[b, pos], gt_xyxy[m], dt), 0, 1)
        grad[b, pos, 4] = dt(cfg["lambda_obj"]) / npos * (_sigmoid(flat[b, pos, 4]) - tgt)
        # classes
        if C > 1:
            z = flat[b, pos, 5:5 + C]
            zs = z - z.max(1, keepdims=True)
            ez = np.exp(zs)
            sm = ez / ez.sum(1, keepdims=True)
            e = dt(cfg["cls_smoothing"])
            tg = np.full_like(sm, e / dt(C))
            tg[np.arange(pos.size), gt_label[m]] += dt(1.0) - e
            grad[b, pos, 5:5 + C] = dt(cfg["lambda_cls"]) / npos * (sm - tg)
    return {"grad": grad, "pos": poss, "neg": negs, "K": np.asarray(Ks), "assign": assign}


def split_levels(flat_grad, levels):
    """[B,N,E] -> list of arrays shaped like the level tensors"""
    out, o = [], 0
    for l in levels:
        n = l.shape[2] * l.shape[3]
        out.append(flat_grad[:, o:o + n].reshape(l.shape))
        o += n
    return out
