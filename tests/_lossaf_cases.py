"""Inputs of the LossAF tests: level tensors as a function of a seed.

The fixture (tests/golden/loss_af_cases.json + loss_af.npz) stores targets, constructor arguments and the reference's
outputs; the level tensors themselves are regenerated here from the case's seed with numpy's frozen legacy generator
(RandomState: its stream is guaranteed not to change between numpy releases) and checked against the float64 sum the
generator recorded, so a drift would be noticed rather than compared.

The tensors are not plain noise: around every ground-truth centre the box channels are set to (noisy) encodings of
that box, so that IoUs are large enough for dynamic_k > 1 and neighbouring boxes contend for the same anchors."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _logit(p):
    return np.log(p / (1.0 - p))


def make_levels(seed, img_size, sizes, num_classes, batch, gt_xyxy, gt_off, center_mode="v8", wh_mode="softplus",
                scale=1.0, extra=0):
    """-> list of float32 [B,1,S,S,5+C+extra]; gt_xyxy [T,4] pixel boxes, gt_off [B+1]"""
    rs = np.random.RandomState(seed)
    E = 5 + num_classes + extra
    out = []
    for S in sizes:
        stride = img_size / S
        t = rs.standard_normal((batch, 1, S, S, E)) * scale
        t[..., 4] -= 2.0                                   # mostly background
        for b in range(batch):
            for g in range(int(gt_off[b]), int(gt_off[b + 1])):
                x1, y1, x2, y2 = [float(v) for v in gt_xyxy[g]]
                cx, cy, w, h = (x1 + x2) / 2, (y1 + y2) / 2, max(x2 - x1, 1.0), max(y2 - y1, 1.0)
                ix, iy = int(cx / stride), int(cy / stride)
                for yy in range(max(iy - 2, 0), min(iy + 3, S)):
                    for xx in range(max(ix - 2, 0), min(ix + 3, S)):
                        n = rs.standard_normal(5) * 0.3
                        ox, oy = cx / stride - xx, cy / stride - yy
                        if center_mode == "v8":
                            px, py = (ox + 0.5) / 2, (oy + 0.5) / 2
                        else:
                            px, py = ox, oy
                        t[b, 0, yy, xx, 0] = _logit(np.clip(px, 0.05, 0.95)) + n[0]
                        t[b, 0, yy, xx, 1] = _logit(np.clip(py, 0.05, 0.95)) + n[1]
                        for k, v in ((2, w / stride), (3, h / stride)):
                            if wh_mode == "v8":
                                e = _logit(np.clip(np.sqrt(v) / 2, 0.02, 0.98))
                            elif wh_mode == "softplus":
                                e = np.log(np.expm1(min(v, 30.0))) if v < 30 else v
                            else:
                                e = np.log(v)
                            t[b, 0, yy, xx, k] = e + n[k] * 0.5
                        t[b, 0, yy, xx, 4] += 2.0 + n[4]
        out.append(t.astype(np.float32))
    return out


def load_cases():
    with open(os.path.join(GOLDEN, "loss_af_cases.json")) as f:
        cases = json.load(f)
    return cases, np.load(os.path.join(GOLDEN, "loss_af.npz"))


def case_inputs(case, npz):
    """-> levels, gt_xyxy [T,4] float32 (as the reference converted the targets), gt_label [T], gt_off [B+1], kwargs"""
    n = case["name"]
    gt, off = npz[n + "/tgt_xyxy"], npz[n + "/gt_off"]
    kw = dict(case["kwargs"])
    levels = make_levels(case["seed"], case["img_size"], case["sizes"], case["num_classes"], case["batch"], gt, off,
                         kw.get("center_mode", "v8"), kw.get("wh_mode", "softplus"), case["scale"])
    chk = float(sum(np.sum(l, dtype=np.float64) for l in levels))
    assert chk == float(npz[n + "/levels_sum"]), "level tensors differ from the ones the fixture was made with"
    return levels, gt, npz[n + "/gt_label"], off, kw
