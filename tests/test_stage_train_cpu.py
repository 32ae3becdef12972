"""Host side of the trainable backbone stage (yololite_amd.stageops): the numpy restatement against the oracle's fixture,
the byte plan, BackboneTail's names and shapes against the oracle backbone's, and the refusals that need no device.
No HIP compute here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import yololite_amd as ya
from yololite_amd import stageops
from yololite_amd.program import zoo_meta, make_meta
from _stage_cases import (CASES, FIXTURE, FIXTURE_WIDE, WIDE, bar, case_inputs, dw_dgrad, dw_forward, dw_wgrad, fixture_tensors, modes,
                          plan_restated, stack_all, units)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c["name"] for c in CASES]
ALL = CASES + WIDE
ALL_IDS = [c["name"] for c in ALL]


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def wide():
    return np.load(FIXTURE_WIDE)


@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_float64_restatement_reproduces_the_fixture(case, fixture, wide):
    """tests/_stage_cases.py stack_all in float64 against the oracle's float64 run: every tensor to 1e-12 of its
    largest value"""
    inputs = case_inputs(case)
    for mode in modes(case):
        got = stack_all(case, inputs, mode == "train")
        want = fixture_tensors(wide if case in WIDE else fixture, case, mode)
        assert set(got) == set(want)
        for n, (r64, idx, _, m64) in want.items():
            g = np.asarray(got[n], np.float64).reshape(-1)
            g = g if idx is None else g[idx]
            assert np.abs(g - r64).max() <= 1e-12 * max(m64, 1.0), (case["name"], mode, n)


@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_a_plain_fp32_run_of_the_restatement_passes_every_bar(case, fixture, wide):
    """the bars are not out of an fp32 implementation's reach: numpy's own fp32 arithmetic stays inside them"""
    inputs = case_inputs(case)
    for mode in modes(case):
        got = stack_all(case, inputs, mode == "train", np.float32)
        for n, (r64, idx, e32, m64) in fixture_tensors(wide if case in WIDE else fixture, case, mode).items():
            g = np.asarray(got[n]).reshape(-1)
            if "num_batches_tracked" in n:
                assert int(g[0]) == int(r64[0])
                continue
            g = g.astype(np.float64)
            err = np.abs((g if idx is None else g[idx]) - r64).max()
            assert err <= bar(e32, m64), (case["name"], mode, n, err, bar(e32, m64))


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("S", [1, 2, 5, 8, 9])
def test_the_restated_depthwise_passes_are_torchs(k, s, S):
    rs = np.random.RandomState(7 * k + s + 31 * S)
    x, w = rs.standard_normal((2, S, S, 4)), rs.standard_normal((4, 1, k, k))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.from_numpy(w).requires_grad_(True)
    y = torch.nn.functional.conv2d(xt, wt, None, s, (k - 1) // 2, 1, 4)
    dy = rs.standard_normal(tuple(y.permute(0, 2, 3, 1).shape))
    y.backward(torch.from_numpy(dy).permute(0, 3, 1, 2))
    assert np.abs(dw_forward(x, w, s) - y.detach().permute(0, 2, 3, 1).numpy()).max() <= 1e-12
    assert np.abs(dw_dgrad(dy, w, s, S) - xt.grad.permute(0, 2, 3, 1).numpy()).max() <= 1e-12
    assert np.abs(dw_wgrad(x, dy, k, s) - wt.grad.numpy()).max() <= 1e-12


@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_plan_counts_the_bytes_the_header_gives(case):
    for B, S in ((case["B"], case["S"]), (64, 40), (1, 7)):
        p = stageops.plan(case["cin"], case["blocks"], B, S)
        want = plan_restated(case, B, S, p["stat_rows"], p["gemm_rows"])
        assert [b["saved_bytes"] for b in p["blocks"]] == want["blocks"]
        for n in ("saved_bytes", "nosave_bytes", "workspace_bytes"):
            assert p[n] == want[n], (n, B, S)
        for b in p["blocks"]:
            assert b["rows_mid"] == B * b["size_mid"] ** 2 and b["rows_out"] == B * b["size_out"] ** 2
            for rows, splits, M in ((b["exp_rows"], b["exp_splits"], b["rows_mid"]), (b["proj_rows"], b["proj_splits"], b["rows_out"])):
                if splits:
                    assert rows % 16 == 0 and (splits - 1) * rows < M <= splits * rows


def _oracle_tail_keys(name):
    """the entries of the stages behind the C4 tap in the oracle's backbone of that name, under `backbone.`"""
    from oracle.backbones import FeatureBackbone
    bb = FeatureBackbone(name)
    first = bb._taps[-2] + 1
    return {"backbone." + k: tuple(v.shape) for k, v in bb.state_dict().items()
            if k.startswith("blocks.") and int(k.split(".")[1]) >= first}


@pytest.mark.parametrize("model", ["edge_n", "edge_m"])
def test_backbone_tail_has_timms_keys_and_shapes(model):
    meta = zoo_meta(model, num_classes=3, img_size=64)
    with torch.device("meta"):
        tail = ya.BackboneTail.from_meta(meta)
    got = {k: tuple(v.shape) for k, v in tail.state_dict().items()}
    want = _oracle_tail_keys(meta["backbone"])
    assert got == want
    stages = sorted({k.split(".")[2] for k in got})
    assert len(stages) == 2 and len({k.split(".")[3] for k in got if k.split(".")[2] == stages[0]}) == 6
    assert any(k.endswith(f"blocks.{stages[1]}.0.bn1.weight") for k in got)
    cmult = 0.5 if model == "edge_n" else 1.0
    assert (tail.in_channels, tail.out_channels) == (int(96 * cmult), int(960 * cmult))
    assert [n for n, _ in tail.named_parameters()] == [k for k in tail.state_dict() if "running" not in k and "tracked" not in k]


def test_the_tiny_tail_case_is_what_backbone_tail_makes_of_oracle_tiny():
    case = [c for c in CASES if c["name"] == "tiny_tail"][0]
    with torch.device("meta"):
        tail = ya.BackboneTail.from_meta(make_meta("YOLOLiteMS_CPU", "oracle_tiny", num_classes=3, img_size=64))
        mine = ya.UIBStack(case["cin"], case["blocks"], prefix=case["prefix"])
    assert tail.blocks_cfg == mine.blocks_cfg and tail.in_channels == case["cin"]
    assert list(tail.state_dict()) == list(mine.state_dict())
    assert {k: tuple(v.shape) for k, v in tail.state_dict().items()} == _oracle_tail_keys("oracle_tiny")
    assert [u["key"] for u in units(case)] == [
        "backbone.blocks.3.0.dw_start.", "backbone.blocks.3.0.pw_exp.", "backbone.blocks.3.0.dw_mid.", "backbone.blocks.3.0.pw_proj.",
        "backbone.blocks.3.1.pw_exp.", "backbone.blocks.3.1.dw_mid.", "backbone.blocks.3.1.pw_proj.", "backbone.blocks.4.0."]


def test_refusals_raise_before_the_library_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(stageops._lib, "load", boom)
    # backbones whose tail is made of other blocks, by name
    for bb in ("tf_efficientnet_lite0", "tf_efficientnetv2_b0", "hgnetv2_b0", "convnextv2_atto", "oracle_tiny_tf"):
        meta = make_meta("YOLOLiteMS_CPU", bb, num_classes=3, img_size=64)
        with pytest.raises(ya.YoloLiteHipError, match=f"{bb}.*not implemented"):
            ya.BackboneTail.from_meta(meta)
        with pytest.raises(ya.YoloLiteHipError, match="not implemented"):
            ya.BackboneTail.from_state_dict(meta, {})
    meta = zoo_meta("edge_n", num_classes=3, img_size=64)
    with pytest.raises(ya.YoloLiteHipError, match="start='c3'.*not implemented"):
        ya.BackboneTail.from_meta(meta, start="c3")
    uir = dict(type="uir", a=0, k=3, s=1, mid=16, c=8)
    # what the kernels do not have, by name
    for extra, word in ((dict(act="relu6"), "relu6"), (dict(act="silu"), "silu"), (dict(same=True), "TF-SAME"),
                        (dict(se=0.25), "squeeze-excite"), (dict(layer_scale=1e-5), "layer-scale")):
        with pytest.raises(ya.YoloLiteHipError, match=f"{word}.*not implemented"):
            ya.UIBStack(8, [dict(uir, **extra)])
    with pytest.raises(ya.YoloLiteHipError, match="type 'ir'.*not implemented"):
        ya.UIBStack(8, [dict(uir, type="ir")])
    # channel multiples
    for cin, blk in ((6, uir), (8, dict(uir, mid=18)), (8, dict(uir, c=10)), (8, dict(type="cn", k=1, s=1, c=30))):
        with pytest.raises(ya.YoloLiteHipError, match="multiple"):
            ya.UIBStack(cin, [blk])
        with pytest.raises(ya.YoloLiteHipError, match="multiple"):
            stageops.plan(cin, [blk], 2, 4)
    # more than 16 blocks, bad a / k / s
    with pytest.raises(ya.YoloLiteHipError, match="1..16 blocks"):
        ya.UIBStack(8, [uir] * 17)
    with pytest.raises(ya.YoloLiteHipError, match="1..16 blocks"):
        ya.UIBStack(8, [])
    for bad in (dict(a=7), dict(k=4), dict(a=1), dict(s=3), dict(s=0), dict(a=0, k=0, s=2)):
        with pytest.raises(ya.YoloLiteHipError, match="block 0"):
            ya.UIBStack(8, [dict(uir, **bad)])
    with pytest.raises(ya.YoloLiteHipError, match="cn block must be 1x1"):
        ya.UIBStack(8, [dict(type="cn", k=3, s=1, c=8)])
    # inputs: no CPU fallback, layouts, one value per channel in training
    m = ya.UIBStack(8, [dict(type="uir", a=5, k=5, s=2, mid=16, c=8)])
    with pytest.raises(ya.YoloLiteHipError, match="HIP device"):
        m(torch.zeros(2, 4, 4, 8), layout="nhwc")
    with pytest.raises(ValueError, match="layout="):
        ya.UIBStack(8, [uir])(torch.zeros(2, 8, 8, 8))
    with pytest.raises(ValueError):
        m(torch.zeros(2, 4, 4, 12))
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(torch.zeros(1, 2, 2, 8), layout="nhwc")              # S 2 -> 1 under stride 2: ONE output row
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(torch.zeros(1, 8, 1, 1), layout="nchw")
    with pytest.raises(ya.YoloLiteHipError, match="HIP device"):
        m.eval()(torch.zeros(1, 2, 2, 8), layout="nhwc")       # eval mode: only the device is missing
    with pytest.raises(ValueError, match="size="):
        stageops.depthwise(torch.zeros(1, 3, 3, 4), torch.zeros(4, 1, 3, 3), "dgrad", 3, 2)
    with pytest.raises(ya.YoloLiteHipError, match="HIP device"):
        stageops.depthwise(torch.zeros(1, 3, 3, 4), torch.zeros(4, 1, 3, 3), "forward", 3, 2)


def _raw_cfg(cin, blocks, eps=1e-5):
    c = stageops._lib.yl_stage_cfg()
    c.in_channels, c.num_blocks, c.eps = cin, len(blocks), eps
    for i, (t, a, k, s, mid, cout) in enumerate(blocks[:16]):
        b = c.block[i]
        b.type, b.a, b.k, b.s, b.mid, b.cout = t, a, k, s, mid, cout
    return c


def test_the_library_refuses_them_as_well():
    """YL_ERR_INVALID (-1) from yl_stage_plan and yl_stage_create, host-side checks in front of any device call (create
    with device -1 would otherwise fail with YL_ERR_HIP)"""
    lib = ya.load_library()
    out = stageops._lib.yl_stage_plan_info()
    h = ctypes.c_void_p()
    ok = (0, 0, 3, 1, 16, 8)
    bad = [_raw_cfg(6, [ok]), _raw_cfg(8, [(0, 0, 3, 1, 18, 8)]), _raw_cfg(8, [(0, 0, 3, 1, 16, 10)]), _raw_cfg(8, [(0, 7, 3, 1, 16, 8)]),
           _raw_cfg(8, [(0, 0, 4, 1, 16, 8)]), _raw_cfg(8, [(0, 0, 3, 3, 16, 8)]), _raw_cfg(8, [(0, 0, 0, 2, 16, 8)]),
           _raw_cfg(8, [(2, 0, 3, 1, 16, 8)]), _raw_cfg(8, [(1, 0, 3, 1, 0, 8)]), _raw_cfg(8, [ok], eps=0.0), _raw_cfg(8, [])]
    many = _raw_cfg(8, [ok] * 16)
    many.num_blocks = 17
    for c in bad + [many]:
        assert lib.yl_stage_plan(ctypes.byref(c), 2, 4, ctypes.byref(out)) == -1
        assert lib.yl_stage_create(-1, ctypes.byref(c), ctypes.byref(h)) == -1
    assert lib.yl_stage_plan(ctypes.byref(_raw_cfg(8, [ok])), 2, 4, ctypes.byref(out)) == 0
    assert lib.yl_stage_plan(ctypes.byref(_raw_cfg(8, [ok])), 0, 4, ctypes.byref(out)) == -1


def test_the_headers_new_symbols_resolve_in_the_built_library():
    text = open(os.path.join(ROOT, "include", "yololite_hip.h")).read()
    names = sorted(set(re.findall(r"\b(yl_stage_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert names == ["yl_stage_backward", "yl_stage_create", "yl_stage_depthwise", "yl_stage_destroy", "yl_stage_forward",
                     "yl_stage_held", "yl_stage_plan"]
    lib = ya.load_library()
    bound = {n for n, _, _ in stageops._lib.SYMBOLS}
    for n in names:
        assert n in bound and getattr(lib, n) is not None
    assert lib.yl_abi_version() == 7 and "#define YL_ABI_VERSION 7" in text
    assert ctypes.sizeof(stageops._lib.yl_stage_cfg) == 16 + 16 * 32
    assert ctypes.sizeof(stageops._lib.yl_stage_block) == 4 * 48
    assert ctypes.sizeof(stageops._lib.yl_stage_block_plan) == 12 * 4 + 8
