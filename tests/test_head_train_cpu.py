"""Host side of the trainable detection heads (yololite_amd.headops): the float64 restatement against the reference's
fixture, the module's names / shapes / initial values, the row planner and the refusals that need no device.  No HIP
compute here."""
import json

import numpy as np
import pytest
import torch

import yololite_amd as ya
from yololite_amd import headops
from _head_cases import CASES, E2E, FIXTURE, FIXTURE_WIDE, WIDE, case_inputs, fixture_tensors, level_names, modes
from _head_np import head_all


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def wide():
    return np.load(FIXTURE_WIDE)


@pytest.mark.parametrize("case", CASES + WIDE, ids=[c["name"] for c in CASES + WIDE])
def test_float64_restatement_reproduces_the_reference(case, fixture, wide):
    """tests/_head_np.py in float64 against the reference's own float64 run: every tensor to 1e-12 of its largest value"""
    for mode in modes(case):
        for li, lv in enumerate(case_inputs(case)):
            got = head_all(lv["params"], lv["buffers"], lv["x"], lv["gy"], lv["k"], case["A"], case["C"], case["depth"],
                           mode == "train")
            want = fixture_tensors(wide if case in WIDE else fixture, case, mode, li)
            assert set(got) == set(want)
            for n, (r64, idx, _, m64) in want.items():
                g = np.asarray(got[n], np.float64).reshape(-1)
                g = g if idx is None else g[idx]
                assert np.abs(g - r64).max() <= 1e-12 * max(m64, 1.0), (case["name"], mode, li, n)


def test_module_has_the_references_keys_shapes_and_dtypes(fixture):
    want = [(n, tuple(sh), dt) for n, sh, dt in json.loads(str(fixture["keys"]))]
    with torch.device("meta"):
        m = ya.DetectHeads(16, 3, (1, 1, 1), 2)
    got = [(n, tuple(v.shape), str(v.dtype)) for n, v in m.state_dict().items()]
    assert got == want
    assert [n for n, _ in m.named_parameters()] == [n for n, _, _ in want if "running" not in n and "tracked" not in n]


def test_state_dict_round_trip_and_from_state_dict():
    case = CASES[1]
    a = ya.DetectHeads(case["F"], case["C"], case["A"], case["depth"], level_names=level_names(case))
    sd = {}
    for lv in case_inputs(case):
        sd.update(lv["params"]); sd.update(lv["buffers"])
    a.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    out = a.state_dict()
    assert list(out) == list(ya.DetectHeads(case["F"], case["C"], case["A"], case["depth"],
                                            level_names=level_names(case)).state_dict())
    for k, v in sd.items():
        assert torch.equal(out[k], torch.as_tensor(v)), k
    meta = {"num_classes": case["C"], "num_anchors_per_level": (case["A"],) * 3,
            "config": {"model": {"fpn_channels": case["F"], "head_depth": case["depth"]},
                       "training": {"use_p2": False, "use_p6": False}}}
    full = dict(sd)
    for k, v in sd.items():                                 # a third level and a key of the trunk: a whole checkpoint
        if k.startswith("head4."):
            full["head5." + k[6:]] = v
    full["lateral3.weight"] = np.zeros((4, 4, 1, 1), np.float32)
    b = ya.DetectHeads.from_state_dict(meta, full)
    assert b.level_names == ("p3", "p4", "p5") and b.num_anchors_per_level == (case["A"],) * 3
    for k, v in full.items():
        if k.startswith("head"):
            assert torch.equal(b.state_dict()[k], torch.as_tensor(v)), k


@pytest.mark.parametrize("C", [1, 3, 80])
def test_initial_biases(C):
    m = ya.DetectHeads(8, C, 2, 1)
    for k in (3, 4, 5):
        o = getattr(m, f"head{k}")["out"]
        assert torch.equal(o["box"].bias, torch.zeros(8))
        assert torch.equal(o["obj"].bias, torch.full((2,), -np.log(99.0), dtype=torch.float32))
        assert torch.equal(o["cls"].bias, torch.full((2 * C,), -np.log(C) if C > 1 else 0.0, dtype=torch.float32))
        bn = getattr(m, f"head{k}")["trunk"][0].block[2]
        assert int(bn.num_batches_tracked) == 0 and torch.equal(bn.running_var, torch.ones(8))


@pytest.mark.parametrize("B,S", [(1, 1), (2, 2), (3, 5), (2, 24), (1, 17), (7, 13), (64, 80), (5, 9)])
@pytest.mark.parametrize("F,C,A", [(16, 1, 1), (96, 80, 1), (328, 80, 1), (20, 1, 2)])
def test_plan_covers_every_row_once(B, S, F, C, A):
    p = headops.plan(F, C, A, 2, B, S)
    M = B * S * S
    assert p["rows"] == M
    for rows, tiles in (("stat_rows", "stat_tiles"), ("gemm_rows", "gemm_tiles"), ("wgrad_rows", "wgrad_splits"),
                        ("ograd_rows", "ograd_splits")):
        r, t = p[rows], p[tiles]
        hit = np.zeros(M, np.int32)
        for i in range(t):
            assert i * r < M, f"{tiles}: tile {i} is empty"
            hit[i * r:min(M, (i + 1) * r)] += 1
        assert (hit == 1).all(), (rows, r, t)
    assert p["wgrad_rows"] % 16 == 0 and p["ograd_rows"] % 16 == 0
    assert p["saved_bytes"] == 2 * (3 * M * F * 4 + 2 * F * 4)
    assert p["workspace_bytes"] >= 2 * M * F * 4 + p["stat_tiles"] * 9 * F * 8 + p["wgrad_splits"] * F * F * 4


def test_plan_and_module_refuse_what_the_kernels_do_not_do():
    for F in (18, 2, 0, 97):
        with pytest.raises(ya.YoloLiteHipError, match="multiple of 4"):
            headops.plan(F, 3, 1, 1, 2, 8)
        with pytest.raises(ya.YoloLiteHipError, match="multiple of 4"):
            ya.DetectHeads(F, 3)
    with pytest.raises(ya.YoloLiteHipError, match="head_depth"):
        ya.DetectHeads(16, 3, 1, 5)
    lib = ya.load_library()
    cfg = headops._cfg(18, 3, 1, 1)
    out = headops._lib.yl_head_plan_info()
    import ctypes
    assert lib.yl_head_plan(ctypes.byref(cfg), 2, 8, ctypes.byref(out)) == -5        # the library refuses it as well


def test_cpu_tensors_and_masks_raise_without_loading_the_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device was asked for")
    m = ya.DetectHeads(16, 3)
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(headops._lib, "load", boom)
    feats = [torch.zeros(2, 16, s, s) for s in (8, 4, 2)]
    with pytest.raises(ya.YoloLiteHipError, match="HIP device"):
        m(feats)
    with pytest.raises(ya.YoloLiteHipError, match="HIP device"):
        m.eval()([f.permute(0, 2, 3, 1) for f in feats])
    with pytest.raises(ya.YoloLiteHipError, match="num_masks"):
        ya.DetectHeads(16, 3, num_masks=32)
    with pytest.raises(ya.YoloLiteHipError, match="num_masks"):
        ya.DetectHeads.from_meta({"num_classes": 3, "config": {"model": {"seg": True, "num_masks": 32}, "training": {}}})
    with pytest.raises(ValueError):
        m(feats[:2])
    with pytest.raises(ValueError):
        m([torch.zeros(2, 12, 8, 8)] * 3)


def test_the_cpu_loops_own_drop_is_a_fifth_of_the_first_loss(fixture):
    """the end-to-end test's yardstick (run once by the generator, tests/_head_np.py fit_reference)"""
    losses = fixture["e2e/losses"]
    assert len(losses) == E2E["steps"] + 1 and np.isfinite(losses).all()
    assert losses[0] - losses[-1] >= 0.2 * losses[0]


def test_a_shape_that_reads_both_ways_needs_a_layout(monkeypatch):
    """[B,F,F,F] is [B,F,S,S] and [B,S,S,F] at once (edge_n's p3 at 768 pixels is [B,96,96,96]): refused unless the
    caller says which, and a stated layout is held to the shape; all of it before a device is asked for"""
    def boom(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(headops._lib, "load", boom)
    m = ya.DetectHeads(8, 2, level_names=("p3",))
    with pytest.raises(ValueError, match="layout="):
        m([torch.zeros(2, 8, 8, 8)])
    for layout in ("nchw", "nhwc"):                        # said: the shape passes, the CPU tensor is what is refused
        with pytest.raises(ya.YoloLiteHipError, match="HIP device"):
            m([torch.zeros(2, 8, 8, 8)], layout=layout)
    with pytest.raises(ValueError, match="not \\[B,S,S,8\\]"):
        m([torch.zeros(2, 8, 4, 4)], layout="nhwc")
    with pytest.raises(ValueError, match="not \\[B,8,S,S\\]"):
        m([torch.zeros(2, 4, 4, 8)], layout="nchw")
    with pytest.raises(ValueError, match="layout must be"):
        m([torch.zeros(2, 4, 4, 8)], layout="hwc")


def test_plan_keeps_what_follows_the_partial_sums_16_byte_aligned():
    """85 columns of float64 partials over one tile are 680 bytes: the coefficients read as float4 come after them"""
    B, S, F, C = 1, 3, 4, 80
    p = headops.plan(F, C, 1, 1, B, S)
    assert p["stat_tiles"] == 1
    wpart = max(p["wgrad_splits"] * F * F * 4, p["ograd_splits"] * (5 + C) * F * 4)
    spart = p["workspace_bytes"] - 2 * B * S * S * F * 4 - 2 * F * 4 - (wpart + 15) // 16 * 16
    assert spart == 688
