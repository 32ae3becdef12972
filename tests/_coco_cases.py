"""Inputs for the COCO bbox evaluation tests: the hand-derived cases A-H (tests/test_coco_eval_cpu.py holds the
restatement to their expected values, tests/test_coco_eval_gpu.py holds the device to the restatement) and
seeded random sets."""
import numpy as np

EPS1 = 1.0 / (1.0 + np.spacing(1))          # what a precision of "1" is in COCOeval: tp / (tp + eps)


def _img(*ids):
    return [{"id": i, "file_name": f"{i}.jpg", "width": 640, "height": 640} for i in ids]


def _gt(gid, img, box, cat=1, area=None, crowd=0):
    return {"id": gid, "image_id": img, "category_id": cat, "bbox": [float(v) for v in box],
            "area": float(box[2] * box[3] if area is None else area), "iscrowd": crowd}


def _dt(img, box, score, cat=1):
    return {"image_id": img, "category_id": cat, "bbox": [float(v) for v in box], "score": float(score)}


def analytic_cases():
    """name -> (images, anns, dets, num_classes, {stat index: expected})."""
    far = [[200.0 + 15 * i, 200.0, 10.0, 10.0] for i in range(10)]
    return {
        "A": (_img(1), [_gt(1, 1, [0, 0, 10, 10])], [_dt(1, [0, 0, 9, 8], .9)], 1,
              {0: .5 * EPS1, 1: EPS1, 2: 0.0, 3: .5 * EPS1, 4: -1, 5: -1, 6: .5, 7: .5, 8: .5}),
        "B": (_img(1), [_gt(1, 1, [0, 0, 10, 10]), _gt(2, 1, [5, 0, 10, 10])],
              [_dt(1, [2.5, 0, 10, 10], .9), _dt(1, [0, 0, 10, 10], .8)], 1,
              {1: EPS1, 2: 51 / 202, 6: .15, 7: .65}),
        "C": ([{"id": 2}, {"id": 1}], [_gt(1, 1, [0, 0, 10, 10]), _gt(2, 2, [0, 0, 10, 10])],
              [_dt(1, [300, 300, 10, 10], .5), _dt(2, [0, 0, 10, 10], .5)], 1, {1: 51 / 202}),
        "D": (_img(1), [_gt(1, 1, [0, 0, 32, 32])], [_dt(1, [0, 0, 32, 32], .7)], 1,
              {3: EPS1, 4: EPS1, 5: -1}),
        "E": (_img(1), [_gt(1, 1, [0, 0, 100, 100], area=500)], [_dt(1, [0, 0, 100, 100], .7)], 1,
              {0: EPS1, 3: EPS1, 4: -1, 5: -1}),
        "F": (_img(1), [_gt(1, 1, [0, 0, 10, 10]), _gt(2, 1, [100, 100, 50, 50], crowd=1)],
              [_dt(1, [110, 110, 10, 10], .95), _dt(1, [0, 0, 10, 10], .9), _dt(1, [130, 130, 10, 10], .8)], 1,
              {0: EPS1, 6: 0.0, 7: 1.0}),
        "G": (_img(1), [_gt(1, 1, [0, 0, 10, 10])],
              [_dt(1, b, .90 - .01 * i) for i, b in enumerate(far)] + [_dt(1, [0, 0, 10, 10], .5)], 1,
              {0: 1 / (11 + np.spacing(1)), 7: 0.0, 8: 1.0}),
        "H": (_img(1, 2), [_gt(1, 1, [0, 0, 10, 10], cat=1), _gt(2, 2, [50, 50, 20, 20], cat=2)],
              [_dt(1, [0, 0, 10, 10], .9, cat=1), _dt(2, [300, 300, 20, 20], .6, cat=3)], 3,
              {0: .5 * EPS1}),
    }


def random_coco(seed, n_img=30, n_cls=5, gt_per_img=(0, 12), det_per_img=(0, 60), crowd_p=0.08, id0=True,
                tie_p=0.3):
    """Crowds, areas straddling 32^2 / 96^2, exact score ties within and across images, more than 100
    detections in some keys, a ground truth with id 0, categories with ground truth only / detections only."""
    r = np.random.RandomState(seed)
    images = [{"id": int(i), "file_name": f"{i}.jpg", "width": 640, "height": 640}
              for i in r.permutation(np.arange(1, n_img + 1) * 3)]
    anns, dets = [], []
    gid = 0 if id0 else 1
    for im in images:
        img = im["id"]
        ng = r.randint(*gt_per_img)
        gts = []
        for _ in range(ng):
            side = float(np.float32(r.choice([r.uniform(4, 30), r.uniform(30, 34), r.uniform(34, 90),
                                              r.uniform(94, 98), r.uniform(98, 200)])))
            asp = float(np.float32(r.uniform(0.6, 1.6)))
            w, h = side * asp, side / asp
            x, y = float(np.float32(r.uniform(0, 500))), float(np.float32(r.uniform(0, 500)))
            cat = int(r.randint(1, n_cls))                     # category n_cls: detections only
            area = r.choice([w * h, 1024.0, 9216.0, w * h * float(np.float32(r.uniform(0.5, 1.2)))], p=[.7, .1, .1, .1])
            anns.append({"id": gid, "image_id": img, "category_id": cat, "bbox": [x, y, w, h], "area": float(area),
                         "iscrowd": int(r.rand() < crowd_p)})
            gts.append((cat, x, y, w, h))
            gid += 1
        nd = r.randint(*det_per_img)
        for k in range(nd):
            if gts and r.rand() < 0.7:
                cat, x, y, w, h = gts[r.randint(len(gts))]
                b = np.array([x, y, w, h]) * (1 + r.normal(0, 0.06, 4))
                if r.rand() < 0.1:
                    b = np.array([x, y, w, h])
                if r.rand() < 0.05:
                    cat = n_cls
            else:
                cat = int(r.randint(1, n_cls + 1))
                b = np.r_[r.uniform(0, 500, 2), r.uniform(4, 200, 2)]
            sc = round(r.rand(), 1) if r.rand() < tie_p else r.rand()
            dets.append({"image_id": img, "category_id": int(cat), "bbox": [float(np.float32(v)) for v in b],
                         "score": float(np.float32(sc))})
    # one image with a single key of > 100 detections
    img = images[0]["id"]
    x, y = 20.0, 20.0
    anns.append({"id": gid, "image_id": img, "category_id": 1, "bbox": [x, y, 40.0, 40.0], "area": 1600.0,
                 "iscrowd": 0})
    for k in range(130):
        b = [x + float(np.float32(r.normal(0, 3))), y + float(np.float32(r.normal(0, 3))), 40.0, 40.0]
        dets.append({"image_id": img, "category_id": 1, "bbox": b, "score": float(np.float32(round(r.rand(), 2)))})
    return images, anns, dets, n_cls + 1                        # category n_cls+1: neither (all -1)


def coco_like(seed, n_img, n_cls=80, gt_mean=7, det_per_img=100):
    """COCO-val-shaped synthetic set: Poisson(gt_mean) ground truths per image (about 1 % crowd), det_per_img
    detections per image (about 40 % near a ground truth of its class, the rest anywhere), COCO-like box sizes."""
    r = np.random.RandomState(seed)
    images = [{"id": int(i), "file_name": f"{i:012d}.jpg", "width": 640, "height": 480}
              for i in r.choice(np.arange(1, 10 * n_img), n_img, replace=False)]
    anns, dets = [], []
    for im in images:
        ng = r.poisson(gt_mean)
        side = np.exp(r.uniform(np.log(6), np.log(400), ng))
        asp = np.exp(r.uniform(-0.7, 0.7, ng))
        w, h = side * asp, side / asp
        x, y = r.uniform(0, 640, ng) - w / 2, r.uniform(0, 480, ng) - h / 2
        cat = r.randint(1, n_cls + 1, ng)
        crowd = r.rand(ng) < 0.01
        for k in range(ng):
            b = [float(np.float32(v)) for v in (x[k], y[k], w[k], h[k])]
            anns.append({"id": len(anns) + 1, "image_id": im["id"], "category_id": int(cat[k]), "bbox": b,
                         "area": float(np.float32(b[2] * b[3] * r.uniform(0.5, 0.9))), "iscrowd": int(crowd[k])})
        near = (r.rand(det_per_img) < 0.4) & (ng > 0)
        j = r.randint(0, max(ng, 1), det_per_img)
        for k in range(det_per_img):
            if near[k]:
                b = np.array([x[j[k]], y[j[k]], w[j[k]], h[j[k]]]) * (1 + r.normal(0, 0.1, 4))
                c = int(cat[j[k]])
            else:
                s = np.exp(r.uniform(np.log(6), np.log(400)))
                b = np.array([r.uniform(-20, 620), r.uniform(-20, 460), s, s * np.exp(r.uniform(-0.7, 0.7))])
                c = int(r.randint(1, n_cls + 1))
            dets.append({"image_id": im["id"], "category_id": c, "bbox": [float(np.float32(v)) for v in b],
                         "score": float(np.float32(r.beta(2, 5) + (0.3 if near[k] else 0.0)))})
    return images, anns, dets, n_cls
