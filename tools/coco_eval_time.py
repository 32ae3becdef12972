#!/usr/bin/env python3
"""Time evalops.coco_eval (COCO bbox mAP on the device) on a seeded COCO-val-sized synthetic set: 5000 images,
80 classes, about 7 ground truths per image, 100 and 300 detections per image.  Prints one JSON line:
device kernel ms per kernel (HIP events, evalops.DEVICE_MS), host ms (list -> array conversion, grouping,
sorting, copies, summarize) and the total; with --restatement also the numpy restatement of COCOeval
(tests/_cocoeval_np.py) on a subset of the images, for scale.

    python tools/coco_eval_time.py [--images 5000] [--dets 100,300] [--repeat 3] [--restatement 250] [--out F]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--dets", default="100,300")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--restatement", type=int, default=250, help="images for the numpy restatement (0 = skip)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    import yololite_amd  # noqa: F401
    from yololite_amd import evalops
    from _coco_cases import coco_like

    dev = torch.device("cuda:0")
    res = {"gpu": torch.cuda.get_device_name(0), "images": args.images, "classes": 80, "runs": []}
    im, an, dt, K = coco_like(1, 20)
    evalops.coco_eval(im, an, dt, num_classes=K, device=dev)                  # library load, allocator warm-up
    for dpi in (int(v) for v in args.dets.split(",")):
        images, anns, dets, K = coco_like(2024, args.images, det_per_img=dpi)
        rows = []
        for _ in range(args.repeat):
            evalops.DEVICE_MS.clear()
            evalops.DEVICE_MS.update(total=0.0, launches=0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = evalops.coco_eval(images, anns, dets, num_classes=K, device=dev)
            total = (time.perf_counter() - t0) * 1e3
            dm = dict(evalops.DEVICE_MS)
            rows.append({"total_ms": total, "device_ms": dm["total"], "host_ms": total - dm["total"],
                         "match_ms": dm.get("coco_match", 0.0), "accumulate_ms": dm.get("coco_accumulate", 0.0)})
        best = min(rows, key=lambda r: r["total_ms"])
        res["runs"].append({"dets_per_image": dpi, "ground_truths": len(anns), "detections": len(dets),
                            "AP": float(out["stats"][0]), "AP50": float(out["stats"][1]),
                            **{k: round(v, 3) for k, v in best.items()},
                            "device_ms_all_repeats": [round(r["device_ms"], 3) for r in rows]})
    if args.restatement:
        from _cocoeval_np import coco_eval_np
        images, anns, dets, K = coco_like(2024, args.restatement, det_per_img=100)
        t0 = time.perf_counter()
        coco_eval_np(images, anns, dets, K)
        ms = (time.perf_counter() - t0) * 1e3
        res["restatement"] = {"images": args.restatement, "dets_per_image": 100, "ms": round(ms, 1),
                              "ms_per_image": round(ms / args.restatement, 3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
