"""Host side of the trainable EfficientNet-Lite stages (yololite_amd.irops): the numpy restatement against the oracle's
fixture, TF-SAME's arithmetic against the oracle's Conv2dSame, the tail's and the mid's names and shapes against the oracle
backbones', the dispatch by family, and the refusals that need no device.  No HIP compute here."""
import math
import os
import re

import numpy as np
import pytest
import torch

import yololite_amd as ya
from yololite_amd import irops, stageops
from yololite_amd.program import make_meta, zoo_meta
import _stage_cases as sc
from _ir_cases import (CASES, FIXTURE, FIXTURE_WIDE, WIDE, as_uib, case_inputs, dw_dgrad, dw_forward, dw_wgrad,
                       fixture_tensors, modes, out_size, pad_begin, stack_all, units)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = CASES + WIDE
ALL_IDS = [c["name"] for c in ALL]
LITE = [f"tf_efficientnet_lite{i}" for i in range(5)]


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def wide():
    return np.load(FIXTURE_WIDE)


@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_float64_restatement_reproduces_the_fixture(case, fixture, wide):
    """tests/_ir_cases.py stack_all in float64 against the oracle's float64 run: every tensor to 1e-12 of its largest
    value (the rule of test_stage_train_cpu.py)"""
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
def test_every_relu6_unit_of_the_cases_reaches_both_kinks(case):
    """the generator's coverage condition, seen from the restatement: at least 2 % of every ReLU6 unit's outputs are
    clamped at 6 and at least 10 % at 0, so a ReLU6 that is really a ReLU differs from the fixture"""
    inputs = case_inputs(case)
    for mode in modes(case):
        pre = []
        stack_all(case, inputs, mode == "train", pre_act=pre)
        assert len(pre) == sum(u["act"] for u in units(case))
        for y in pre:
            assert (y >= 6).mean() >= 0.02 and (y <= 0).mean() >= 0.10, (case["name"], mode, (y >= 6).mean(), (y <= 0).mean())


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("s", [1, 2])
def test_pad_begin_and_output_size_are_conv2dsames(k, s):
    """irops.pad_begin (and the tests' own) against the arithmetic of oracle.backbones.Conv2dSame.forward, S in 1..12"""
    for S in range(1, 13):
        So = math.ceil(S / s)
        total = max((So - 1) * s + (k - 1) + 1 - S, 0)
        assert irops.pad_begin(k, s, S) == pad_begin(k, s, S) == total // 2, (k, s, S)
        assert irops.out_size(S, s) == out_size(S, s) == So == stageops._out_size(S, k, s), (k, s, S)
        assert irops.pad_begin(k, s, S, same=False) == (k - 1) // 2
        want = (k - 1) // 2 - 1 if (s == 2 and S % 2 == 0) else (k - 1) // 2
        assert irops.pad_begin(k, s, S) == want, (k, s, S)


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("S", [1, 2, 5, 6, 8, 9])
def test_the_restated_depthwise_passes_are_the_oracles(k, s, S):
    """under TF-SAME against oracle.backbones._conv(same=True) with autograd; with same=False against _stage_cases'"""
    from oracle.backbones import _conv
    rs = np.random.RandomState(7 * k + s + 31 * S)
    x, w = rs.standard_normal((2, S, S, 4)), rs.standard_normal((4, 1, k, k))
    conv = _conv(4, 4, k, s, groups=4, same=True).double()
    conv.weight.data = torch.from_numpy(w)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_(True)
    y = conv(xt)
    assert y.shape[-1] == out_size(S, s)
    dy = rs.standard_normal(tuple(y.permute(0, 2, 3, 1).shape))
    y.backward(torch.from_numpy(dy).permute(0, 3, 1, 2))
    assert np.abs(dw_forward(x, w, s) - y.detach().permute(0, 2, 3, 1).numpy()).max() <= 1e-12
    assert np.abs(dw_dgrad(dy, w, s, S) - xt.grad.permute(0, 2, 3, 1).numpy()).max() <= 1e-12
    assert np.abs(dw_wgrad(x, dy, k, s) - conv.weight.grad.numpy()).max() <= 1e-12
    assert np.array_equal(dw_forward(x, w, s, same=False), sc.dw_forward(x, w, s))
    assert np.array_equal(dw_dgrad(dy, w, s, S, same=False), sc.dw_dgrad(dy, w, s, S))
    assert np.array_equal(dw_wgrad(x, dy, k, s, same=False), sc.dw_wgrad(x, dy, k, s))


def _oracle_keys(name, part):
    """the entries of the stages behind the C4 tap ("tail") or between the C3 and the C4 tap ("mid") in the oracle's
    backbone of that name, under `backbone.`"""
    from oracle.backbones import FeatureBackbone
    bb = FeatureBackbone(name)
    lo, hi = (bb._taps[-2], bb._taps[-1]) if part == "tail" else (bb._taps[-3], bb._taps[-2])
    return {"backbone." + k: tuple(v.shape) for k, v in bb.state_dict().items()
            if k.startswith("blocks.") and lo < int(k.split(".")[1]) <= hi}


@pytest.mark.parametrize("name", LITE)
def test_lite_tail_and_mid_have_timms_keys_and_shapes(name):
    meta = make_meta("YOLOLiteMS", name, num_classes=3, img_size=64)
    for cls, part, stages in ((ya.EfficientNetLiteTail, "tail", ["5", "6"]), (ya.EfficientNetLiteMid, "mid", ["3", "4"])):
        with torch.device("meta"):
            m = cls.from_meta(meta)
        got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        want = _oracle_keys(name, part)
        assert got == want and list(m.state_dict()) == [k for k in want]
        assert sorted({k.split(".")[2] for k in got}) == stages
        assert (m.act, m.same, m.eps) == ("relu6", True, 1e-3)
        assert [n for n, _ in m.named_parameters()] == [k for k in m.state_dict() if "running" not in k and "tracked" not in k]
        assert len(m.blocks_cfg) <= 16
    if name == "tf_efficientnet_lite0":
        with torch.device("meta"):
            tail, mid = ya.EfficientNetLiteTail.from_meta(meta), ya.EfficientNetLiteMid.from_meta(meta)
        assert [d["name"] for d in tail.blocks_cfg] == ["5.0", "5.1", "5.2", "5.3", "6.0"]
        assert (tail.in_channels, tail.out_channels, mid.in_channels, mid.out_channels) == (112, 320, 40, 112)
        assert [(d["k"], d["s"], d["mid"], d["c"]) for d in tail.blocks_cfg][::4] == [(5, 2, 672, 192), (3, 1, 1152, 320)]
    if name == "tf_efficientnet_lite4":
        with torch.device("meta"):
            tail, mid = ya.EfficientNetLiteTail.from_meta(meta), ya.EfficientNetLiteMid.from_meta(meta)
        assert (len(tail.blocks_cfg), len(mid.blocks_cfg)) == (9, 12)
        assert max(d["mid"] for d in tail.blocks_cfg) == 1632


def test_tail_for_dispatches_by_family(monkeypatch):
    from yololite_amd.program import synth_state_dict
    lite, edge = zoo_meta("yololite_n", num_classes=3, img_size=64), zoo_meta("edge_n", num_classes=3, img_size=64)
    sd, sd_edge = synth_state_dict(lite), synth_state_dict(edge)          # (the program builder asks the library for shapes)

    def boom(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(stageops._lib, "load", boom)
    tail = irops.tail_for(lite, sd, precision="bf16")
    assert type(tail) is ya.EfficientNetLiteTail and tail.precision == "bf16"
    assert all(np.array_equal(v.numpy(), np.asarray(sd[k]).reshape(v.shape)) for k, v in tail.state_dict().items() if k in sd)
    assert type(irops.tail_for(edge, sd_edge)) is ya.BackboneTail
    for bb in ("tf_efficientnetv2_b0", "hgnetv2_b0", "oracle_tiny_tf"):
        with pytest.raises(ya.YoloLiteHipError, match=f"{bb}.*not implemented"):
            irops.tail_for(make_meta("YOLOLiteMS_CPU", bb, num_classes=3, img_size=64), {})
    with pytest.raises(KeyError, match="backbone tail"):
        irops.tail_for(zoo_meta("yololite_n", num_classes=3, img_size=64), {})


def test_refusals_raise_before_the_library_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(stageops._lib, "load", boom)
    ir = dict(type="ir", k=3, s=1, mid=48, c=8)
    assert ya.IRStack(8, [ir]).out_channels == 8
    # what the kernels do not have, by name
    for extra, word in ((dict(act="silu"), "silu"), (dict(act="relu"), "relu"), (dict(se=0.25), "squeeze-excite"),
                        (dict(layer_scale=1e-5), "layer-scale")):
        with pytest.raises(ya.YoloLiteHipError, match=f"{word}.*not implemented"):
            ya.IRStack(8, [dict(ir, **extra)])
    for act in ("silu", "hardswish", "gelu"):
        with pytest.raises(ya.YoloLiteHipError, match=f"{act}.*not implemented"):
            ya.IRStack(8, [ir], act=act)
    with pytest.raises(ValueError, match="same"):
        ya.IRStack(8, [ir], same="tf")
    for t in ("uir", "cn", "ds", "er"):
        with pytest.raises(ya.YoloLiteHipError, match=f"type '{t}'.*not implemented"):
            ya.IRStack(8, [dict(ir, type=t)])
    # channel multiples, block count, k and s
    for cin, blk in ((6, ir), (8, dict(ir, mid=50)), (8, dict(ir, c=10))):
        with pytest.raises(ya.YoloLiteHipError, match="multiple"):
            ya.IRStack(cin, [blk])
    with pytest.raises(ya.YoloLiteHipError, match="1..16 blocks"):
        ya.IRStack(8, [ir] * 17)
    with pytest.raises(ya.YoloLiteHipError, match="1..16 blocks"):
        ya.IRStack(8, [])
    for bad in (dict(k=0), dict(k=1), dict(k=4), dict(k=7), dict(s=0), dict(s=3)):
        with pytest.raises(ya.YoloLiteHipError, match="block 0"):
            ya.IRStack(8, [dict(ir, **bad)])
    with pytest.raises(ValueError, match="precision"):
        ya.IRStack(8, [ir], precision="fp8")
    # any backbone but the five lite ones, by name
    for bb in ("mobilenetv4_conv_small", "tf_efficientnetv2_b0", "hgnetv2_b0", "convnextv2_atto", "oracle_tiny_tf", "oracle_tiny"):
        meta = make_meta("YOLOLiteMS_CPU", bb, num_classes=3, img_size=64)
        for cls in (ya.EfficientNetLiteTail, ya.EfficientNetLiteMid):
            with pytest.raises(ya.YoloLiteHipError, match=f"{bb}.*not implemented"):
                cls.from_meta(meta)
            with pytest.raises(ya.YoloLiteHipError, match="not implemented"):
                cls.from_state_dict(meta, {})
    # inputs: no CPU fallback, one value per channel in training
    m = ya.IRStack(8, [dict(ir, s=2, c=16)])
    with pytest.raises(ya.YoloLiteHipError, match="HIP device"):
        m(torch.zeros(2, 4, 4, 8), layout="nhwc")
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(torch.zeros(1, 2, 2, 8), layout="nhwc")              # S 2 -> 1 under stride 2: ONE output row
    with pytest.raises(ya.YoloLiteHipError, match="HIP device"):
        stageops.depthwise(torch.zeros(1, 4, 4, 4), torch.zeros(4, 1, 3, 3), "forward", 3, 2, same=True)
    assert m.variant_state() == {"act": "relu6", "same": True}
    assert ya.IRStack(8, [ir], act="relu", same=False).variant_state() == {"act": "relu", "same": False}


def test_an_irstack_is_the_uibstack_of_its_a0_blocks_on_the_host():
    """units, sizes and plan are UIBStack's of the equivalent uir blocks; the state dicts map key for key"""
    case = [c for c in CASES if c["name"] == "lite_tiny_tail"][0]
    ucase, key = as_uib(case)
    with torch.device("meta"):
        ir = ya.IRStack(case["cin"], case["blocks"], prefix=case["prefix"])
        uib = ya.UIBStack(case["cin"], ucase["blocks"], eps=1e-3, prefix=case["prefix"])
    assert [key(k) for k in ir.state_dict()] == list(uib.state_dict())
    assert [tuple(v.shape) for v in ir.state_dict().values()] == [tuple(v.shape) for v in uib.state_dict().values()]
    assert ir._handle.unit_names == uib._handle.unit_names == [["pw_exp", "dw_mid", "pw_proj"]] * 3
    for S in (4, 7, 8):
        assert ir._unit_sizes(S) == uib._unit_sizes(S) and ir.out_size(S) == out_size(S, 2)
    assert [u["key"] + u["conv"] for u in units(case)][:3] == ["backbone.blocks.5.0.conv_pw", "backbone.blocks.5.0.conv_dw",
                                                               "backbone.blocks.5.0.conv_pwl"]


def test_the_header_declares_the_variant_symbols_and_the_library_has_them():
    """The stage's variant entry points carry the prefix yl_variant_, as the stage's mixed-precision ones carry yl_amp_:
    the header's yl_stage_* list is held name for name by test_stage_train_cpu.py"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yololite_hip.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(yl_variant_[a-z_]+)\s*\(", text)))
    assert names == ["yl_variant_stage_depthwise", "yl_variant_stage_get", "yl_variant_stage_set"]
    assert re.search(r"yl_variant_stage_set\(yl_stage\* h, int32_t act, int32_t same\)", text)
    assert "#define YL_STAGE_ACT_RELU 0" in text and "#define YL_STAGE_ACT_RELU6 1" in text and "#define YL_ABI_VERSION 7" in text
    lib = ya.load_library()
    bound = {n for n, _, _ in stageops._lib.SYMBOLS}
    for n in names:
        assert n in bound and hasattr(lib, n), n
    assert lib.yl_abi_version() == 7
    import ctypes as C
    a = C.c_int32()
    assert lib.yl_variant_stage_set(None, 0, 0) == -1 and lib.yl_variant_stage_get(None, C.byref(a), C.byref(a)) == -1
    assert lib.yl_variant_stage_depthwise(None, None, None, 0, 3, 1, 1, 4, 4, 2, None, None) == -1      # same = 2
    assert C.sizeof(stageops._lib.yl_stage_cfg) == 16 + 16 * 32
