"""Inputs of the LossAF gradient tests: the 19 cases of tests/golden/loss_af_cases.json unchanged, plus one that the
forward fixture has no use for:

  orphan_exp_clamp   orphan_tiny's targets and seed with wh_mode="exp"; after make_levels the size logits of the 7 x 7
                     cells around the 3 px box on the finest level are set to 9.5 and -10.5, both outside the decode's
                     clamp [-10, 8].  The rescued anchor of that box is then a positive whose columns 2 and 3 have
                     derivative exactly 0.

The expected gradients (tests/golden/loss_af_grad.npz) come from the reference's own autograd, see
tests/golden/make_loss_grad_fixtures.py."""
import os

import numpy as np

from _lossaf_cases import GOLDEN, case_inputs, load_cases, make_levels

EXTRA = "orphan_exp_clamp"
GROUPS = ("box", "obj", "cls")


def group_slices(C):
    return {"box": slice(0, 4), "obj": slice(4, 5), "cls": slice(5, 5 + C)}


def grad_cases():
    """-> (cases, forward archive): the forward fixture's cases plus orphan_exp_clamp"""
    cases, npz = load_cases()
    base = next(c for c in cases if c["name"] == "orphan_tiny")
    extra = dict(base, name=EXTRA, kwargs=dict(base["kwargs"], wh_mode="exp"))
    return cases + [extra], npz


def grad_case_inputs(case, npz):
    """-> levels, gt_xyxy [T,4] float32, gt_label [T], gt_off [B+1], kwargs"""
    if case["name"] != EXTRA:
        return case_inputs(case, npz)
    gt, lab, off = npz["orphan_tiny/tgt_xyxy"], npz["orphan_tiny/gt_label"], npz["orphan_tiny/gt_off"]
    kw = dict(case["kwargs"])
    levels = make_levels(case["seed"], case["img_size"], case["sizes"], case["num_classes"], case["batch"], gt, off,
                         kw.get("center_mode", "v8"), kw["wh_mode"], case["scale"])
    levels[0][0, 0, 4:11, 9:16, 2] = 9.5
    levels[0][0, 0, 4:11, 9:16, 3] = -10.5
    return levels, gt, lab, off, kw


def load_grad_fixture():
    return np.load(os.path.join(GOLDEN, "loss_af_grad.npz"))


def fixture_grad(z, name, shape):
    """the reference's float64 gradient of a case as a dense [B,N,E] array (zero outside the stored entries)"""
    g = np.zeros(int(np.prod(shape)), np.float64)
    g[z[name + "/idx"]] = z[name + "/g64"]
    return g.reshape(shape)
