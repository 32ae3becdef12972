"""COCO bbox evaluation without a GPU: the numpy restatement of pycocotools' COCOeval (tests/_cocoeval_np.py)
against hand-derived cases, and the call surface of the device path (exports, C ABI symbols, no CPU fallback)."""
import numpy as np
import pytest
import torch

import yololite_amd as ya
from yololite_amd import _lib, evalops
from _coco_cases import EPS1, analytic_cases
from _cocoeval_np import coco_eval_from_lists_np, coco_eval_np


@pytest.mark.parametrize("case", sorted(analytic_cases()))
def test_restatement_reproduces_analytic_case(case):
    images, anns, dets, K, want = analytic_cases()[case]
    stats = coco_eval_np(images, anns, dets, K)["stats"]
    for i, v in want.items():
        assert abs(stats[i] - v) <= 1e-12, (case, i, stats[i], v)


def test_no_ground_truth_gives_minus_one():
    images, _, dets, _, _ = analytic_cases()["A"]
    assert (coco_eval_np(images, [], dets, 1)["stats"] == -1).all()


def test_empty_detections_early_return():
    images, anns, _, _, _ = analytic_cases()["A"]
    want = {"AP": 0.0, "AP50": 0.0, "AP75": 0.0, "APS": 0.0, "APM": 0.0, "APL": 0.0, "AR": 0.0}
    assert coco_eval_from_lists_np(images, anns, []) == want
    assert ya._coco_eval_from_lists(images, anns, []) == want     # no device needed for the early return


def test_unknown_image_id_raises():
    images, anns, dets, K, _ = analytic_cases()["A"]
    with pytest.raises(ValueError):
        coco_eval_np(images, anns, dets + [dict(dets[0], image_id=99)], K)


def test_out_of_range_category_is_dropped():
    images, anns, dets, K, _ = analytic_cases()["B"]
    base = coco_eval_np(images, anns, dets, K)
    extra = dets + [dict(dets[1], category_id=7, score=.99)]
    extra_gt = anns + [dict(anns[0], id=9, category_id=0)]
    got = coco_eval_np(images, extra_gt, extra, K)
    assert np.array_equal(base["precision"], got["precision"]) and np.array_equal(base["stats"], got["stats"])


def test_detections_ranked_beyond_max_dets_do_not_count():
    """150 detections in one key: the exact match at rank 101 is cut by maxDets[-1]; at rank 100 it counts."""
    images, anns = analytic_cases()["A"][:2]
    def far(n, score):
        return [{"image_id": 1, "category_id": 1, "bbox": [300.0 + i, 300.0, 10.0, 10.0], "score": score}
                for i in range(n)]
    exact = {"image_id": 1, "category_id": 1, "bbox": [0.0, 0.0, 10.0, 10.0], "score": 0.5}
    cut = coco_eval_np(images, anns, far(100, 0.9) + [exact] + far(49, 0.1), 1)["stats"]
    assert cut[8] == 0.0 and cut[0] == 0.0
    kept = coco_eval_np(images, anns, far(49, 0.1) + [exact] + far(99, 0.9), 1)["stats"]
    assert kept[8] == 1.0 and abs(kept[0] - 1 / (100 + np.spacing(1))) <= 1e-12


def test_exact_ground_truth_at_area_boundaries():
    """An area of exactly 32^2 is small AND medium (both bounds inclusive)."""
    images, anns, dets, K, _ = analytic_cases()["D"]
    s = coco_eval_np(images, anns, dets, K)["stats"]
    assert s[3] == s[4] == EPS1 and s[9] == s[10] == 1.0


def test_coco_eval_is_exported():
    for name in ("coco_eval", "_coco_eval_from_lists", "coco_summary_lines"):
        assert callable(getattr(ya, name)) and name in ya.__all__
    names = [n for n, _, _ in _lib.SYMBOLS]
    assert "yl_eval_coco_match" in names and "yl_eval_coco_accumulate" in names


def test_coco_eval_without_device_raises(monkeypatch):
    """No CPU fallback: without a HIP device the device path refuses instead of computing elsewhere."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    images, anns, dets, K, _ = analytic_cases()["A"]
    with pytest.raises(ya.YoloLiteHipError):
        evalops.coco_eval(images, anns, dets, num_classes=K)
    with pytest.raises(ya.YoloLiteHipError):
        ya._coco_eval_from_lists(images, anns, dets, num_classes=K)


def test_non_bbox_iou_type_is_refused():
    images, anns, dets, K, _ = analytic_cases()["A"]
    with pytest.raises(ValueError):
        ya._coco_eval_from_lists(images, anns, dets, iouType="segm")


def test_summary_lines_format():
    stats = np.array([.5, 1, 0, .5, -1, -1, .5, .5, .5, .5, -1, -1])
    lines = ya.coco_summary_lines(stats)
    assert len(lines) == 12
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.500"
    assert lines[1] == " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 1.000"
    assert lines[4] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=medium | maxDets=100 ] = -1.000"
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.500"
