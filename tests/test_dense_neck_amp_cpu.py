"""tests/golden/dense_neck_amp.npz (the reference's YOLOLiteMS with rounded-operand smooth convolutions) against the
restatements, on the CPU: the reference's own fp32 arithmetic passes every bar, every bar can tell a rounded run from
an unrounded one, and tests/_dense_neck_amp_np.py reproduces the fixture."""
import functools

import numpy as np
import pytest
import torch

from _dense_neck_amp_cases import AMP_CASES as CASES, AMP_FIXTURE, AMP_PRECISIONS, amp_fixture_tensors, bar
from _dense_neck_amp_np import neck_all as neck_all_amp
from _dense_neck_cases import case_inputs, modes
from _dense_neck_np import neck_all

IDS = [c["name"] for c in CASES]


@functools.lru_cache(maxsize=None)
def _fixture():
    return np.load(AMP_FIXTURE)


def _at(v, idx):
    v = np.asarray(v, np.float64).reshape(-1)
    return v if idx is None else v[idx]


def _cells(case):
    return [(mode, precision) for mode in modes(case) for precision in AMP_PRECISIONS]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_restatement_reproduces_the_fixture(case):
    inputs = case_inputs(case)
    for mode, precision in _cells(case):
        got = neck_all_amp(inputs, case["depth"], mode == "train", precision)
        for li, d in enumerate(got):
            want = amp_fixture_tensors(_fixture(), case, mode, precision, li)
            assert set(d) == set(want)
            for n, (r64, idx, _, m64) in want.items():
                err = np.abs(_at(d[n], idx) - r64).max()
                assert err <= 1e-12 * max(m64, 1.0), (mode, precision, li, n, err)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_plain_fp32_run_of_the_rounded_restatement_is_inside_every_bar(case):
    inputs = case_inputs(case)
    for mode, precision in _cells(case):
        got = neck_all_amp(inputs, case["depth"], mode == "train", precision, dtype=torch.float32)
        for li, d in enumerate(got):
            for n, (r64, idx, flip, m64) in amp_fixture_tensors(_fixture(), case, mode, precision, li).items():
                if n.startswith("num_batches_tracked"):
                    assert int(d[n]) == int(r64[0])
                    continue
                err = np.abs(_at(d[n], idx) - r64).max()
                assert err <= bar(flip, m64), (mode, precision, li, n, err, bar(flip, m64))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_level_can_tell_the_unrounded_result_from_the_rounded_one(case):
    """per case, mode, precision and level, at least one of p, dc and the first block's weight gradient has the UNROUNDED
    float64 result outside its bar"""
    inputs = case_inputs(case)
    for mode, precision in _cells(case):
        plain = neck_all(inputs, case["depth"], mode == "train")
        for li, lv in enumerate(inputs):
            want = amp_fixture_tensors(_fixture(), case, mode, precision, li)
            outside = []
            for n in ("p", "dc", f"g.smooth{lv['k']}.0.weight"):
                r64, idx, flip, m64 = want[n]
                miss = np.abs(_at(plain[li][n], idx) - r64).max()
                outside.append(miss > bar(flip, m64))
            assert any(outside), (mode, precision, li)
