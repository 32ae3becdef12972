#!/usr/bin/env python3
"""Generate tests/golden/loss_af_cases.json + loss_af.npz by RUNNING THE REFERENCE's own LossAF
(scripts/loss/loss.py of the reference checkout, imported unmodified; pure torch, CPU) on seeded inputs.

    python tests/golden/make_loss_fixtures.py --reference /path/to/YoloLite-Official-Repo

Per case the archive holds the targets as the reference converted them (its own format sniffing), the float64 sum of
the level tensors (tests/_lossaf_cases.py regenerates the tensors from the seed), and the reference's outputs computed
twice: in fp32 and in fp64 (default dtype float64, double level tensors; the targets still pass through the
reference's fp32 cast).  Batch results and per-image parts (the reference called one image at a time).

Admission rule: a case goes in only if its fp32 and fp64 runs agree to 1e-5 relative on box, obj and cls -- the
assignment is discrete, and a case that sat on a near-tie would pin one implementation's rounding instead of the
semantics.  The generator asserts that for every case; none is dropped.  (No seed had to be changed so far.)"""
import argparse
import importlib.util
import json
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from _lossaf_cases import make_levels  # noqa: E402

OUT = os.environ.get("YL_FIXTURE_OUT") or HERE


def boxes_for(rs, img, n, lo=12, hi=0.5):
    c = rs.uniform(0.1 * img, 0.9 * img, (n, 2))
    wh = rs.uniform(lo, hi * img, (n, 2))
    b = np.concatenate([c - wh / 2, c + wh / 2], 1)
    return np.clip(b, 0, img - 1)


def to_fmt(b, fmt, img):
    b = np.asarray(b, np.float64).reshape(-1, 4)
    if fmt == "xyxy_px":
        return b
    if fmt == "xyxyn":
        return b / img
    c = np.concatenate([(b[:, :2] + b[:, 2:]) / 2, b[:, 2:] - b[:, :2]], 1)
    return c if fmt == "xywh_px" else c / img


def case(name, seed, img=256, sizes=None, C=3, counts=(3, 5), fmt="xyxy_px", key="boxes", scale=1.0, special=None, **kw):
    rs = np.random.RandomState(1000 + seed)
    sizes = sizes or [img // 8, img // 16, img // 32]
    targets = []
    for i, n in enumerate(counts):
        b = boxes_for(rs, img, n)
        if special:
            b = special(i, b, rs, img)
        targets.append({"key": key, "fmt": fmt, "boxes": to_fmt(b, fmt, img).tolist(),
                        "labels": rs.randint(0, C, len(b)).tolist()})
    return {"name": name, "seed": seed, "img_size": img, "sizes": sizes, "num_classes": C, "batch": len(counts),
            "scale": scale, "kwargs": kw, "targets": targets}


def sp_tiny(i, b, rs, img):          # 3 px box: below the finest level's gate at the default bounds -> orphan rescue
    if i == 0:
        b = np.concatenate([b, [[101.0, 57.0, 104.0, 60.0]]], 0)
    return b


def sp_huge(i, b, rs, img):          # nearly the whole image: above the coarsest level's gate
    if i == 1:
        b = np.concatenate([b, [[2.0, 3.0, img - 3.0, img - 2.0]]], 0)
    return b


def sp_overlap(i, b, rs, img):       # pairs shifted by a few pixels: they contend for the same anchors
    sh = rs.uniform(-6, 6, b.shape)
    return np.clip(np.concatenate([b, b + sh], 0), 0, img - 1)


def all_cases():
    cs = []
    s = 0
    for cm in ("v8", "simple"):
        for wm in ("softplus", "v8", "exp"):
            s += 1
            cs.append(case(f"modes_{cm}_{wm}", s, C=3, counts=(4, 0, 6), center_mode=cm, wh_mode=wm))
    cs.append(case("c1", 11, C=1, counts=(5, 3)))
    cs.append(case("c80", 12, C=80, counts=(6, 4)))
    cs.append(case("empty_batch", 13, C=3, counts=(0, 0)))
    cs.append(case("orphan_tiny", 14, C=3, counts=(3, 2), special=sp_tiny))
    cs.append(case("gate_huge", 15, sizes=[64, 32], C=3, counts=(2, 3), special=sp_huge))   # strides 4, 8: 251 px is above both gates
    cs.append(case("conflict", 16, C=3, counts=(6, 8), special=sp_overlap))
    cs.append(case("fmt_xywhn", 17, C=3, counts=(4, 3), fmt="xywhn", key="bboxes"))
    cs.append(case("fmt_xyxyn", 18, C=3, counts=(4, 3), fmt="xyxyn", key="xyxy"))
    cs.append(case("fmt_xywh_px", 19, C=3, counts=(4, 3), fmt="xywh_px"))
    cs.append(case("weights", 20, C=3, counts=(5, 7, 2), special=sp_overlap, lambda_box=2.5, lambda_obj=0.7, lambda_cls=1.0,
                   assign_cls_weight=1.0, center_radius_cells=3.5, topk_limit=7, cls_smoothing=0.1, area_cells_min=2.0,
                   area_cells_max=400.0, area_tol=1.1, size_prior_w=0.4, ar_prior_w=0.3, iou_cost_w=2.0,
                   center_cost_w=1.0))
    cs.append(case("p2_levels", 21, img=320, sizes=[80, 40, 20, 10], C=3, counts=(5, 4)))
    cs.append(case("p6_levels", 22, img=320, sizes=[40, 20, 10, 5], C=3, counts=(5, 4), scale=2.0))
    cs.append(case("crowded", 23, img=320, C=3, counts=(30, 18, 0, 25), scale=0.5))
    return cs


def run_reference(mod, c, levels, dtype):
    torch.set_default_dtype(dtype)
    try:
        preds = [torch.from_numpy(l).to(dtype) for l in levels]
        tg = [{t["key"]: torch.tensor(t["boxes"], dtype=torch.float32).reshape(-1, 4),
               "labels": torch.tensor(t["labels"], dtype=torch.int64)} for t in c["targets"]]
        crit = mod.LossAF(c["num_classes"], c["img_size"], **c["kwargs"])
        with torch.no_grad():
            _, d = crit(preds, tg)
            per = []
            for b in range(c["batch"]):
                crit1 = mod.LossAF(c["num_classes"], c["img_size"], **c["kwargs"])
                _, d1 = crit1([p[b:b + 1] for p in preds], tg[b:b + 1])
                per.append([d1["box"], d1["obj"], d1["cls"]])
        return np.array([d["box"], d["obj"], d["cls"], d["pos"]], np.float64), np.array(per, np.float64)
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_loss", os.path.join(a.reference, "scripts", "loss", "loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    arrays, cases = {}, all_cases()
    for c in cases:
        n = c["name"]
        conv = [mod._targets_to_xyxy_px({t["key"]: torch.tensor(t["boxes"], dtype=torch.float32).reshape(-1, 4)},
                                        c["img_size"], c["img_size"], torch.device("cpu")).numpy() for t in c["targets"]]
        off = np.concatenate([[0], np.cumsum([len(x) for x in conv])]).astype(np.int32)
        gt = np.concatenate(conv, 0).astype(np.float32).reshape(-1, 4)
        lab = np.concatenate([np.asarray(t["labels"], np.int32) for t in c["targets"]]).astype(np.int32)
        levels = make_levels(c["seed"], c["img_size"], c["sizes"], c["num_classes"], c["batch"], gt, off,
                             c["kwargs"].get("center_mode", "v8"), c["kwargs"].get("wh_mode", "softplus"), c["scale"])
        r32, p32 = run_reference(mod, c, levels, torch.float32)
        r64, p64 = run_reference(mod, c, levels, torch.float64)
        rel = np.abs(r32[:3] - r64[:3]) / np.maximum(np.abs(r64[:3]), 1e-30)
        rel[r64[:3] == r32[:3]] = 0.0
        assert rel.max() <= 1e-5 and r32[3] == r64[3], (n, r32, r64)      # admission rule: change the seed, say so above
        arrays.update({n + "/tgt_xyxy": gt, n + "/gt_label": lab, n + "/gt_off": off,
                       n + "/levels_sum": np.float64(sum(np.sum(l, dtype=np.float64) for l in levels)),
                       n + "/ref32": r32, n + "/ref64": r64, n + "/per32": p32, n + "/per64": p64})
        print(f"{n:22s} T={len(gt):3d} ref64={r64} rel32={rel.max():.2e}")
    np.savez_compressed(os.path.join(OUT, "loss_af.npz"), **arrays)
    with open(os.path.join(OUT, "loss_af_cases.json"), "w") as f:
        json.dump(cases, f, indent=1)


if __name__ == "__main__":
    main()
