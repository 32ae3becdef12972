"""LossAF without a GPU: the fixtures the reference produced (tests/golden/make_loss_fixtures.py) pin the numpy
restatement (tests/_lossaf_np.py, which the GPU tests then use for the assignment and for inputs too large to commit)
and the Python restatement of the reference's target-format sniffing; the built library must export yl_loss_af."""
import ctypes
import os

import numpy as np
import pytest

from _lossaf_cases import case_inputs, load_cases
from _lossaf_np import loss_af

CASES, NPZ = load_cases()
NAMES = [c["name"] for c in CASES]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.where(a == b, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def test_fixture_covers_what_it_must():
    kw = [c["kwargs"] for c in CASES]
    assert {(k.get("center_mode", "v8"), k.get("wh_mode", "softplus")) for k in kw} >= {
        (a, b) for a in ("v8", "simple") for b in ("softplus", "v8", "exp")}
    assert {c["num_classes"] for c in CASES} >= {1, 3, 80}
    assert any(0 in np.diff(NPZ[n + "/gt_off"]) for n in NAMES)                       # an image without boxes
    assert {t["fmt"] for c in CASES for t in c["targets"]} == {"xyxy_px", "xywh_px", "xywhn", "xyxyn"}
    assert {t["key"] for c in CASES for t in c["targets"]} == {"boxes", "bboxes", "xyxy"}
    assert any(len(c["sizes"]) == 4 for c in CASES) and any("topk_limit" in k for k in kw)


@pytest.mark.parametrize("name", NAMES)
def test_admission_rule(name):
    """fp32 and fp64 runs of the reference agree to 1e-5 relative: no case sits on an assignment near-tie"""
    assert _rel(NPZ[name + "/ref32"][:3], NPZ[name + "/ref64"][:3]) <= 1e-5
    assert NPZ[name + "/ref32"][3] == NPZ[name + "/ref64"][3]


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_restatement_matches_reference_fp64(case):
    levels, gt, lab, off, kw = case_inputs(case, NPZ)
    r = loss_af(levels, gt, lab, off, case["num_classes"], case["img_size"], **kw)
    n = case["name"]
    ref = NPZ[n + "/ref64"]
    print(n, "rel", _rel([r["box"], r["obj"], r["cls"]], ref[:3]), "per-image", _rel(r["per_image"], NPZ[n + "/per64"]))
    assert _rel([r["box"], r["obj"], r["cls"]], ref[:3]) <= 1e-9
    assert r["pos"] == ref[3]
    assert _rel(r["per_image"], NPZ[n + "/per64"]) <= 1e-9
    a = r["assign"]
    assert a.shape == (case["batch"], sum(s * s for s in case["sizes"]))
    for b in range(case["batch"]):                       # matched rows belong to the image
        m = a[b][a[b] >= 0]
        assert ((m >= off[b]) & (m < off[b + 1])).all()


def test_special_cases_do_what_they_are_for():
    by = {c["name"]: c for c in CASES}

    def run(n):
        levels, gt, lab, off, kw = case_inputs(by[n], NPZ)
        return loss_af(levels, gt, lab, off, by[n]["num_classes"], by[n]["img_size"], **kw), gt, off
    r, gt, off = run("orphan_tiny")
    tiny = int(np.argmin((gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])))
    assert (r["assign"] == tiny).sum() == 1                                   # rescued: exactly one anchor
    r, gt, off = run("gate_huge")
    huge = int(np.argmax((gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])))
    assert (r["assign"] == huge).sum() == 1
    r, _, _ = run("c1")
    assert r["cls"] == 0.0


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_target_format_sniffing(case):
    from yololite_amd.lossops import pack_targets
    tg = [{t["key"]: np.asarray(t["boxes"], np.float32).reshape(-1, 4), "labels": np.asarray(t["labels"])}
          for t in case["targets"]]
    gt, lab, off = pack_targets(tg, case["img_size"], case["num_classes"])
    n = case["name"]
    assert np.array_equal(gt, NPZ[n + "/tgt_xyxy"]) and np.array_equal(lab, NPZ[n + "/gt_label"])
    assert np.array_equal(off, NPZ[n + "/gt_off"])


def test_library_exports_and_binds_loss_entry_point():
    from yololite_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "yl_loss_af")
    assert any(s[0] == "yl_loss_af" and len(s[2]) == 12 for s in _lib.SYMBOLS)
    assert ctypes.sizeof(_lib.yl_loss_cfg) == 18 * 4


def test_topk_limit_above_the_kernel_limit_is_refused():
    from yololite_amd import LossAF, YoloLiteHipError
    with pytest.raises(YoloLiteHipError):
        LossAF(3, 256, topk_limit=65)
