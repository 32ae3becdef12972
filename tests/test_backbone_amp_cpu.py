"""The backbone's 16-bit modes without a device: the `precision` interface of stemops / stageops (validation before any
device call, propagation through MobileNetV4Backbone, refusal when the parts differ), the C ABI's new symbols, the op
cells of test_stem_conv_amp_gpu.py (each must tell the rounded result from the unrounded one), and
tests/golden/backbone_amp.npz held to its generator's rules (_backbone_amp_cases.py)."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import yololite_amd as ya
from yololite_amd import _lib, stageops, stemops
from yololite_amd import _trainmod as tm
from yololite_amd.program import make_meta
from _backbone_amp_cases import (AMP_FIXTURE, AMP_SEEDS, AMP_STAGE, AMP_STEM, KS, PLANAR, PRECISIONS, SEED_STEP, SEEDS_PER_CASE,
                                 SHAPES, amp_cases, amp_fixture_tensors, amp_mod, amp_modes, cell, first_dense_weight, passes_of)
from _head_cases import bar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META = make_meta("YOLOLiteMS_CPU", "oracle_tiny", num_classes=3, img_size=64)
UNITS = [dict(k=3, s=2, c=8), dict(k=1, s=1, c=8)]
BLOCKS = [dict(type="uir", a=0, k=3, s=1, mid=16, c=8)]


def _stacks(precision="fp32"):
    return [ya.ConvStack(8, UNITS, precision=precision), ya.UIBStack(8, BLOCKS, precision=precision),
            ya.BackboneStem.from_meta(META, precision), stageops.BackboneMid.from_meta(META, precision),
            ya.BackboneTail.from_meta(META, precision=precision)]


def test_every_module_takes_and_reports_its_precision():
    for m in _stacks():
        assert m.precision == "fp32"
    for p in ("fp32", "fp16", "bf16"):
        for m in _stacks(p):
            assert m.precision == p, type(m)
            m.precision = "fp32"
            assert m.precision == "fp32"
            assert copy.deepcopy(_stacks(p)[0]).precision == p
    sd = ya.MobileNetV4Backbone.from_meta(META).state_dict()
    assert ya.BackboneStem.from_state_dict(META, sd, precision="bf16").precision == "bf16"
    assert stageops.BackboneMid.from_state_dict(META, sd, precision="bf16").precision == "bf16"
    assert ya.BackboneTail.from_state_dict(META, sd, precision="fp16").precision == "fp16"
    assert ya.MobileNetV4Backbone.from_state_dict(META, sd, precision="fp16").precision == "fp16"


def test_an_unknown_precision_is_a_value_error_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call")
    monkeypatch.setattr(_lib, "load", no_device)
    for bad in ("fp8", "half", None, 16, "FP16"):
        with pytest.raises(ValueError, match="precision"):
            ya.ConvStack(8, UNITS, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            ya.UIBStack(8, BLOCKS, precision=bad)
        for make in (ya.BackboneStem.from_meta, stageops.BackboneMid.from_meta, ya.MobileNetV4Backbone.from_meta):
            with pytest.raises(ValueError, match="precision"):
                make(META, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            ya.BackboneTail.from_meta(META, precision=bad)
        for m in _stacks() + [ya.MobileNetV4Backbone.from_meta(META)]:
            with pytest.raises(ValueError, match="precision"):
                m.precision = bad
            assert m.precision == "fp32"
    x = torch.zeros(1, 8, 8, 4)
    w = torch.zeros(4, 4, 3, 3)
    with pytest.raises(ValueError, match="precision"):
        stemops.conv(x, w, "forward", 3, 1, precision="fp8")
    with pytest.raises(ya.YoloLiteHipError):               # a known precision goes on to the usual refusal of CPU tensors
        stemops.conv(x, w, "forward", 3, 1, precision="fp16")


def test_the_backbone_sets_all_three_parts_and_refuses_to_name_a_mixture():
    bb = ya.MobileNetV4Backbone.from_meta(META, precision="bf16")
    assert (bb.stem.precision, bb.mid.precision, bb.tail.precision) == ("bf16",) * 3 and bb.precision == "bf16"
    bb.precision = "fp16"
    assert (bb.stem.precision, bb.mid.precision, bb.tail.precision) == ("fp16",) * 3
    bb.mid.precision = "fp32"
    with pytest.raises(ValueError, match="precision"):
        bb.precision
    bb.precision = "fp32"
    assert bb.precision == "fp32"
    parts = ya.MobileNetV4Backbone(bb.stem, bb.mid, bb.tail, precision="bf16")
    assert parts.precision == "bf16"
    bb.tail.precision = "fp16"
    assert ya.MobileNetV4Backbone(bb.stem, bb.mid, bb.tail).tail.precision == "fp16"      # None: the parts keep theirs


def test_the_header_declares_the_amp_symbols_and_the_library_has_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yololite_hip.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(yl_amp_[a-z_]+)\s*\(", text)))
    assert names == ["yl_amp_stage_get", "yl_amp_stage_set", "yl_amp_stem_conv", "yl_amp_stem_get", "yl_amp_stem_set"]
    lib = _lib.load()
    assert lib.yl_abi_version() == 7
    for n in names:
        assert hasattr(lib, n), n
    assert lib.yl_amp_stage_set(None, 0) == -1 and lib.yl_amp_stem_set(None, 0) == -1
    m = C.c_uint32()
    assert lib.yl_amp_stage_get(None, C.byref(m), C.byref(m)) == -1 and lib.yl_amp_stem_get(None, C.byref(m), C.byref(m)) == -1
    assert tm.PRECISIONS == {"fp32": 0, "fp16": _lib.YL_HEAD_F16, "bf16": _lib.YL_HEAD_BF16}


@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_op_cell_tells_the_rounded_result_from_the_unrounded_one(precision):
    for k, s in KS:
        for B, S, cin, cout, planar in SHAPES + PLANAR:
            x, w, dy, ref, seed = cell(k, s, B, S, cin, cout, planar, precision)
            assert seed is not None, (k, s, B, S, cin, cout, planar)
            for p in passes_of(planar):
                assert float((ref[p]["unrounded"] - ref[p]["r64"]).abs().max()) > ref[p]["bar"], (k, s, B, S, cin, cout, p)


def test_the_fixture_holds_every_case_the_cases_file_keeps_and_nothing_else():
    z = np.load(AMP_FIXTURE)
    want = {f"{c['name']}/{mode}/{p}/{part}" for c, p in amp_cases() for mode in amp_modes(c) for part in ("r64", "flip", "max64")}
    assert set(z.files) == want
    assert os.path.getsize(AMP_FIXTURE) < (1 << 20)
    for c in AMP_STEM + AMP_STAGE:
        for p in PRECISIONS:
            seed = AMP_SEEDS.get((c["name"], p))
            if seed is not None:                           # one of the twenty seeds of the case's list
                assert (seed - c["seed"]) % SEED_STEP == 0 and 0 <= (seed - c["seed"]) // SEED_STEP < SEEDS_PER_CASE
    kept = {p: {c["name"] for c, q in amp_cases() if q == p} for p in PRECISIONS}
    for p in PRECISIONS:                                   # what must remain for BOTH precisions
        assert kept[p] & {"planar3", "s2even", "s1"}, "a 3x3 stem case"
        assert "pw" in kept[p], "a 1x1 stem case"
        assert kept[p] & {"k3res"}, "a residual stage block"
    for c, p in amp_cases():
        for mode in amp_modes(c):
            for n, (r64, idx, flip, m64) in amp_fixture_tensors(z, c, mode, p).items():
                assert np.isfinite(r64).all() and flip >= 0 and m64 >= 0, (c["name"], mode, p, n)
                assert np.abs(r64).max() <= m64, (c["name"], mode, p, n)


def test_every_kept_case_tells_the_rounded_model_from_the_unrounded_one():
    """the cap: in at least one of y, dx and the first dense weight gradient the UNROUNDED float64 model (the restatement
    of _stem_cases / _stage_cases on the same seed) lies outside the fixture's bar"""
    z = np.load(AMP_FIXTURE)
    for c, p in amp_cases():
        m = amp_mod(c)
        inputs = m.case_inputs(c)
        for mode in amp_modes(c):
            un = m.stack_all(c, inputs, mode == "train", np.float64)
            want = amp_fixture_tensors(z, c, mode, p)
            told = []
            for n in ("y", "dx", first_dense_weight(c)):
                if n not in want:
                    continue
                r64, idx, flip, m64 = want[n]
                g = np.asarray(un[n], np.float64).reshape(-1)
                err = float(np.abs((g if idx is None else g[idx]) - r64).max())
                told.append(err > bar(flip, m64))
            assert any(told), (c["name"], mode, p)
