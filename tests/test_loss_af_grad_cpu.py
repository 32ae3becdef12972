"""LossAF's gradient without a GPU: the fixture the reference's own autograd produced
(tests/golden/make_loss_grad_fixtures.py -> loss_af_grad.npz) pins the hand-derived numpy restatement
(tests/_lossaf_grad_np.py), which the GPU tests then use for inputs the fixture does not hold; the restatement is also
checked against finite differences of the forward restatement, and the tie rule of the hard-negative selection against
its definition.  The built library must export the two new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest

from _lossaf_grad_cases import EXTRA, GROUPS, fixture_grad, grad_case_inputs, grad_cases, group_slices, load_grad_fixture
from _lossaf_grad_np import loss_af_grad, select_negatives
from _lossaf_np import loss_af

CASES, NPZ = grad_cases()
NAMES = [c["name"] for c in CASES]
Z = load_grad_fixture()
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _pairs(per_image):
    return np.array([(b, n) for b, idx in enumerate(per_image) for n in idx], np.int32).reshape(-1, 2)


def test_fixture_holds_every_case_and_its_admission():
    assert len(CASES) == 20 and NAMES[-1] == EXTRA
    for n in NAMES:
        assert float(Z[n + "/gap"]) > 1e-5                                    # no case on a selection tie
        assert len(Z[n + "/idx"]) == len(Z[n + "/g64"]) and np.all(Z[n + "/g64"] != 0)
    assert sum(len(Z[n + "/idx"]) for n in NAMES) > 40000


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_restatement_matches_reference_autograd_fp64(case):
    """sets exactly; values within 1e-9 of the column group's max|g64| (the bar of the forward restatement)"""
    n = case["name"]
    levels, gt, lab, off, kw = grad_case_inputs(case, NPZ)
    r = loss_af_grad(levels, gt, lab, off, case["num_classes"], case["img_size"], **kw)
    assert np.array_equal(_pairs(r["pos"]), Z[n + "/pos"])
    assert np.array_equal(_pairs(r["neg"]), Z[n + "/neg"])
    g = r["grad"]
    assert tuple(g.shape) == tuple(Z[n + "/shape"])
    ref = fixture_grad(Z, n, g.shape)
    rows = np.zeros(g.shape[:2], bool)
    for k in ("/pos", "/neg"):
        rows[Z[n + k][:, 0], Z[n + k][:, 1]] = True
    assert not g[~rows].any()                                                 # exactly zero outside the stored rows
    for k, sl in group_slices(case["num_classes"]).items():
        m = float(Z[n + "/max64"][GROUPS.index(k)])
        err = np.abs(g[..., sl] - ref[..., sl]).max() if g[..., sl].size else 0.0
        print(n, k, "error / max|g64|", err / m if m else err)
        assert err <= 1e-9 * m


def test_exp_clamp_case_does_what_it_is_for():
    case = CASES[NAMES.index(EXTRA)]
    levels, gt, lab, off, kw = grad_case_inputs(case, NPZ)
    flat = np.concatenate([l.reshape(l.shape[0], -1, l.shape[-1]) for l in levels], 1)
    pos = Z[EXTRA + "/pos"]
    out = (flat[pos[:, 0], pos[:, 1], 2] > 8.0) & (flat[pos[:, 0], pos[:, 1], 3] < -10.0)
    assert out.sum() == 1                                                     # the rescued anchor of the 3 px box
    b, n = pos[out][0]
    ref = fixture_grad(Z, EXTRA, tuple(Z[EXTRA + "/shape"]))
    assert ref[b, n, 2] == 0.0 and ref[b, n, 3] == 0.0 and ref[b, n, 0] != 0.0 and ref[b, n, 1] != 0.0
    g = loss_af_grad(levels, gt, lab, off, case["num_classes"], case["img_size"], **kw)["grad"]
    assert g[b, n, 2] == 0.0 and g[b, n, 3] == 0.0


def _flat(arrs):
    return np.concatenate([a.reshape(a.shape[0], -1, a.shape[-1]) for a in arrs], 1)


def _direction(levels, cols, seed=5):
    """seeded unit-normal direction that moves only the columns `cols` of every level tensor"""
    rs = np.random.RandomState(seed)
    d = [rs.standard_normal(l.shape) for l in levels]
    for dd in d:
        keep = np.zeros(dd.shape[-1], bool)
        keep[cols] = True
        dd[..., ~keep] = 0.0
    return d


@pytest.mark.parametrize("name", ["modes_v8_softplus", "weights"])
def test_directional_derivative_matches_central_difference(name):
    """<grad, d> against (f(x + h d) - f(x - h d)) / 2h of _lossaf_np.loss_af in fp64, h = 1e-6, d a seeded unit-normal
    direction over the objectness and class columns.  (The box columns are left to the next test: the reference detaches
    the objectness target and holds CIoU's alpha constant, both functions of the box columns, so along them the gradient
    autograd defines is NOT the derivative of the forward value.)  The assignment and the selected negatives are the
    same at x - h d, x and x + h d (asserted), so f is smooth along the segment.  The central difference's own error is
    truncation ~ h^2 times the third derivative (1e-12) plus the rounding of the two forward values, a few eps |f| each,
    divided by 2h.  Bound: |difference| <= 8 eps |f| / 2h + h^2 (about 1e-8 at |f| ~ 10; relative to |f| it is 9e-10).
    Measured |difference|: 3.3e-11 (modes_v8_softplus, derivative -0.22), 5.3e-10 (weights, derivative -0.0094)."""
    case = CASES[NAMES.index(name)]
    levels, gt, lab, off, kw = grad_case_inputs(case, NPZ)
    C, S = case["num_classes"], case["img_size"]
    lv = [l.astype(np.float64) for l in levels]
    d = _direction(lv, slice(4, 5 + C))
    h = 1e-6

    def f(sign):
        x = [l + sign * h * dd for l, dd in zip(lv, d)]
        r = loss_af(x, gt, lab, off, C, S, **kw)
        neg = loss_af_grad(x, gt, lab, off, C, S, assign=r["assign"], **kw)["neg"]
        return r["box"] + r["obj"] + r["cls"], r["assign"], neg
    r0 = loss_af_grad(lv, gt, lab, off, C, S, **kw)
    fp, ap_, np_ = f(+1.0)
    fm, am, nm = f(-1.0)
    assert np.array_equal(ap_, r0["assign"]) and np.array_equal(am, r0["assign"])
    assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(r0["neg"], np_, nm))
    want = (fp - fm) / (2 * h)
    got = float(np.sum(r0["grad"] * _flat(d)))
    tol = 8 * np.finfo(np.float64).eps * abs(fp + fm) / 2 / (2 * h) + h * h
    print(name, "directional derivative", got, "central difference", want, "difference", abs(got - want), "bound", tol)
    assert abs(got - want) <= tol


@pytest.mark.parametrize("name", ["modes_v8_softplus", "modes_simple_v8", "modes_v8_exp"])
def test_box_columns_match_central_difference_with_alpha_held(name):
    """the box columns 0-3 against a central difference of the box term with CIoU's alpha held at its value at x, as the
    reference's no_grad holds it: box(x') = lambda_box * sum over images of mean(1 - (ciou(x') + (alpha(x') - alpha(x))
    v(x'))), built from _lossaf_np's decode and _ciou; with alpha free it is loss_af's own box term (asserted).  Only the
    box term is differenced, so the detached objectness target does not enter.  The bound is the one above with the
    box term as f (about 2e-9).  Measured |difference|: 4.2e-11 (modes_v8_softplus), 7.7e-10 (modes_simple_v8), 3.6e-10
    (modes_v8_exp)."""
    import math
    from _lossaf_np import DEFAULTS, _ciou, decode
    case = CASES[NAMES.index(name)]
    levels, gt, lab, off, kw = grad_case_inputs(case, NPZ)
    C, S = case["num_classes"], case["img_size"]
    cfg = dict(DEFAULTS, **kw)
    lv = [l.astype(np.float64) for l in levels]
    r0 = loss_af(lv, gt, lab, off, C, S, **kw)
    asg = r0["assign"]
    gt32 = np.asarray(gt, np.float32)

    def alpha_v(p, t32):
        """alpha and v of bbox_ciou_flat, as _lossaf_np._ciou forms them"""
        f = np.float32
        pw, ph = np.maximum(p[:, 2] - p[:, 0], 1e-7), np.maximum(p[:, 3] - p[:, 1], 1e-7)
        tw, th = np.maximum(t32[:, 2] - t32[:, 0], f(1e-7)), np.maximum(t32[:, 3] - t32[:, 1], f(1e-7))
        d = np.arctan((tw / th).astype(np.float64)).astype(f).astype(np.float64) - np.arctan(pw / ph)
        v = 4 / math.pi ** 2 * (d * d)
        t = t32.astype(np.float64)
        iw = np.maximum(np.minimum(p[:, 2], t[:, 2]) - np.maximum(p[:, 0], t[:, 0]), 0)
        ih = np.maximum(np.minimum(p[:, 3], t[:, 3]) - np.maximum(p[:, 1], t[:, 1]), 0)
        iou = iw * ih / (pw * ph + (tw * th).astype(np.float64) - iw * ih + 1e-7)
        return v / (v - iou + 1 + 1e-7), v

    def box(x, alpha0=None):
        _, xyxy, _, _, _ = decode(x, S, cfg["center_mode"], cfg["wh_mode"], np.float64)
        tot, alphas = 0.0, []
        for b in range(asg.shape[0]):
            pos = np.nonzero(asg[b] >= 0)[0]
            alphas.append(None)
            if not pos.size:
                continue
            a, v = alpha_v(xyxy[b, pos], gt32[asg[b, pos]])
            alphas[-1] = a
            held = a if alpha0 is None else alpha0[b]
            tot += cfg["lambda_box"] * np.mean(1.0 - (_ciou(xyxy[b, pos], gt32[asg[b, pos]], np.float64) + (a - held) * v))
        return tot, alphas
    b0, alpha0 = box(lv)
    assert abs(b0 - r0["box"]) <= 1e-12 * abs(r0["box"])       # with alpha free: the forward restatement's box term
    d = _direction(lv, slice(0, 4))
    h = 1e-6
    want = (box([l + h * dd for l, dd in zip(lv, d)], alpha0)[0] - box([l - h * dd for l, dd in zip(lv, d)], alpha0)[0]) / (2 * h)
    g = loss_af_grad(lv, gt, lab, off, C, S, assign=asg, **kw)["grad"]
    got = float(np.sum(g[..., :4] * _flat(d)[..., :4]))
    tol = 8 * np.finfo(np.float64).eps * abs(b0) / (2 * h) + h * h
    print(name, "box directional derivative", got, "central difference", want, "difference", abs(got - want), "bound", tol)
    assert abs(got - want) <= tol


def test_tie_rule_selects_the_lowest_anchor_indices():
    """all-equal objectness logits on an empty image: every term equals the K-th, anchors 0..K-1 are selected"""
    x = np.full((1344,), -2.0)
    neg, K = select_negatives(x, np.zeros((0,), np.int64), np.float64)
    assert K == 64 and np.array_equal(neg, np.arange(64))
    # with positives in the way the selection skips them and K grows to 3 * npos
    pos = np.arange(0, 60, 2)
    neg, K = select_negatives(x, pos, np.float64)
    assert K == 90 and np.array_equal(neg, np.setdiff1d(np.arange(200), pos)[:90])
    # through the whole restatement: an image without boxes
    levels = [np.zeros((1, 1, 8, 8, 8), np.float32), np.zeros((1, 1, 4, 4, 8), np.float32)]
    r = loss_af_grad(levels, np.zeros((0, 4), np.float32), np.zeros((0,), np.int64), np.array([0, 0]), 3, 64)
    assert np.array_equal(r["neg"][0], np.arange(64))
    assert np.array_equal(np.flatnonzero(r["grad"][0, :, 4]), np.arange(64)) and not r["grad"][0, :, :4].any()
    assert np.allclose(r["grad"][0, :64, 4], 0.5 / 64, rtol=1e-15)


def test_library_exports_and_binds_the_backward_entry_points():
    from yololite_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "yololite_hip.h")) as f:
        header = f.read()
    for name, nargs in (("yl_loss_af_train", 13), ("yl_loss_af_backward", 13)):
        assert hasattr(lib, name)
        assert any(s[0] == name and len(s[2]) == nargs for s in _lib.SYMBOLS)
        m = re.search(r"yl_status\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m and len(m.group(1).split(",")) == nargs
    # the forward's entry and its configuration are as they were
    assert any(s[0] == "yl_loss_af" and len(s[2]) == 12 for s in _lib.SYMBOLS)
    assert ctypes.sizeof(_lib.yl_loss_cfg) == 18 * 4


def test_grad_keyword_constructs():
    from yololite_amd import LossAF
    assert LossAF(3, 256, grad=True).grad is True
    assert LossAF(3, 256).grad is False
