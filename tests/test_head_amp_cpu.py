"""tests/golden/head_amp.npz (the reference's make_head / _forward_head with rounded-operand 1x1 convolutions) against the
restatements, on the CPU: the reference's own fp32 arithmetic passes every bar, every bar can tell a rounded run from an
unrounded one, and tests/_head_amp_cases.py reproduces the fixture.  Also here, because it needs no device: every op-level
case of test_head_gemm_amp_gpu.py has its UNROUNDED float64 result outside its bar (the seeds were picked so)."""
import functools

import numpy as np
import pytest
import torch

from _head_amp_cases import (AMP_CASES, AMP_FIXTURE, PASSES, PRECISIONS, SITES, amp_fixture_tensors, amp_modes, bar,
                             head_all_amp, op_reference)
from _head_cases import CASES, case_inputs
from _head_np import head_all

IDS = [c["name"] for c in AMP_CASES]


@functools.lru_cache(maxsize=None)
def _fixture():
    return np.load(AMP_FIXTURE)


def _at(v, idx):
    v = np.asarray(v, np.float64).reshape(-1)
    return v if idx is None else v[idx]


def _cells(case):
    return [(mode, precision) for mode in amp_modes(case) for precision in PRECISIONS]


def test_the_fixture_is_small_enough_to_commit():
    import os
    assert os.path.getsize(AMP_FIXTURE) < (1 << 20)


@pytest.mark.parametrize("case", AMP_CASES, ids=IDS)
def test_the_restatement_reproduces_the_fixture(case):
    inputs = case_inputs(case)
    for mode, precision in _cells(case):
        for li, lv in enumerate(inputs):
            d = head_all_amp(case, lv, mode == "train", precision)
            want = amp_fixture_tensors(_fixture(), case, mode, precision, li)
            assert set(d) == set(want)
            for n, (r64, idx, _, m64) in want.items():
                err = np.abs(_at(d[n], idx) - r64).max()
                assert err <= 1e-12 * max(m64, 1.0), (mode, precision, li, n, err)


@pytest.mark.parametrize("case", AMP_CASES, ids=IDS)
def test_a_plain_fp32_run_of_the_rounded_restatement_is_inside_every_bar(case):
    inputs = case_inputs(case)
    for mode, precision in _cells(case):
        for li, lv in enumerate(inputs):
            d = head_all_amp(case, lv, mode == "train", precision, dtype=torch.float32)
            for n, (r64, idx, flip, m64) in amp_fixture_tensors(_fixture(), case, mode, precision, li).items():
                if n.startswith("num_batches_tracked"):
                    assert int(d[n]) == int(r64[0])
                    continue
                err = np.abs(_at(d[n], idx) - r64).max()
                assert err <= bar(flip, m64), (mode, precision, li, n, err, bar(flip, m64))


@pytest.mark.parametrize("case", AMP_CASES, ids=IDS)
def test_every_level_can_tell_the_unrounded_result_from_the_rounded_one(case):
    """per case, mode, precision and level, at least one of y, dx and block 0's 1x1 weight gradient has the UNROUNDED
    float64 result outside its bar"""
    inputs = case_inputs(case)
    for mode, precision in _cells(case):
        for li, lv in enumerate(inputs):
            plain = head_all(lv["params"], lv["buffers"], lv["x"], lv["gy"], lv["k"], case["A"], case["C"], case["depth"],
                             mode == "train")
            want = amp_fixture_tensors(_fixture(), case, mode, precision, li)
            outside = []
            for n in ("y", "dx", f"g.head{lv['k']}.trunk.0.block.1.weight"):
                r64, idx, flip, m64 = want[n]
                miss = np.abs(_at(plain[n], idx) - r64).max()
                outside.append(miss > bar(flip, m64))
            assert any(outside), (mode, precision, li)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_op_case_can_see_a_missing_rounding(case, precision):
    for li in range(len(case["sizes"])):
        for site in SITES:
            for pass_ in PASSES:
                ref = op_reference(case["name"], li, site, pass_, precision)
                miss = float((ref["unrounded"] - ref["r64"]).abs().max())
                assert miss > ref["bar"], (li, site, pass_, miss, ref["bar"])
