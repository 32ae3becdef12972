"""Host side of the trainable dense stem and of the whole trainable backbone (yololite_amd.stemops, stageops.BackboneMid,
stageops.MobileNetV4Backbone): the numpy restatement against the oracle's fixture, the byte and launch plan, the names and
shapes against the oracle backbone's, and the refusals that need no device.  No HIP compute here."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import yololite_amd as ya
from yololite_amd import stageops, stemops
from yololite_amd.program import zoo_meta, make_meta
from _stem_cases import (CASES, FIXTURE, FIXTURE_WIDE, TINY, WIDE, bar, case_inputs, conv_dgrad, conv_forward, conv_wgrad, fixture_tensors, modes,
                         plan_restated, stack_all, tiny_all, tiny_inputs, tiny_tensor_shapes, units)

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


def _held(got, want, tol):
    assert set(want) <= set(got)
    for n, (r64, idx, e32, m64) in want.items():
        g = np.asarray(got[n]).reshape(-1)
        if "num_batches_tracked" in n:
            assert int(g[0]) == int(r64[0])
            continue
        g = g.astype(np.float64)
        err = np.abs((g if idx is None else g[idx]) - r64).max()
        assert err <= tol(e32, m64), (n, err, tol(e32, m64))


@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_float64_restatement_reproduces_the_fixture(case, fixture, wide):
    """tests/_stem_cases.py stack_all in float64 against the oracle's float64 run: every tensor to 1e-12 of its largest value"""
    inputs = case_inputs(case)
    for mode in modes(case):
        _held(stack_all(case, inputs, mode == "train"), fixture_tensors(wide if case in WIDE else fixture, case, mode),
              lambda e, m: 1e-12 * max(m, 1.0))


def test_the_whole_backbone_restated_reproduces_the_fixture(fixture):
    """stem, stage 2 and the tail chained with the gradient joins at C3 and C4, against the oracle_tiny FeatureBackbone"""
    want = fixture_tensors(fixture, TINY, "train", tiny_tensor_shapes())
    _held(tiny_all(tiny_inputs()), want, lambda e, m: 1e-11 * max(m, 1.0))


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("S", [1, 2, 5, 8, 9])
def test_the_restated_convolution_passes_are_torchs(k, s, S):
    rs = np.random.RandomState(7 * k + s + 31 * S)
    x, w = rs.standard_normal((2, S, S, 4)), rs.standard_normal((8, 4, k, k))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.from_numpy(w).requires_grad_(True)
    y = torch.nn.functional.conv2d(xt, wt, None, s, (k - 1) // 2)
    dy = rs.standard_normal(tuple(y.permute(0, 2, 3, 1).shape))
    y.backward(torch.from_numpy(dy).permute(0, 3, 1, 2))
    assert np.abs(conv_forward(x, w, s) - y.detach().permute(0, 2, 3, 1).numpy()).max() <= 1e-12
    assert np.abs(conv_dgrad(dy, w, s, S) - xt.grad.permute(0, 2, 3, 1).numpy()).max() <= 1e-12
    assert np.abs(conv_wgrad(x, dy, k, s) - wt.grad.numpy()).max() <= 1e-12


def _regenerates(tmp_path, committed, flags):
    env = dict(os.environ, YL_FIXTURE_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_stem_fixtures.py")] + flags, check=True, env=env,
                   stdout=subprocess.DEVNULL)
    new, old = np.load(tmp_path / os.path.basename(committed)), np.load(committed)
    assert sorted(new.files) == sorted(old.files)
    for n in old.files:
        a, b = new[n], old[n]
        assert a.shape == b.shape
        if n.endswith("/e32"):                             # the fp32 run's own error: to a factor, not to the bit, and
            big = old[n[:-3] + "max64"] > 1e-9             # not where the tensor is zero in exact arithmetic
            assert np.all(a[big] <= 4 * b[big] + 1e-30) and np.all(b[big] <= 4 * a[big] + 1e-30), n
        else:
            assert np.abs(a - b).max() <= 1e-9 * max(np.abs(b).max(), 1.0), n
    assert os.path.getsize(committed) < 600 * 1024


def test_the_recipe_regenerates_the_committed_fixture(tmp_path):
    _regenerates(tmp_path, FIXTURE, [])


def test_the_recipe_regenerates_the_committed_wide_fixture(tmp_path):
    _regenerates(tmp_path, FIXTURE_WIDE, ["--wide"])


def _layout(case):
    return "nchw" if case["planar"] else "nhwc"


@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_plan_counts_what_the_header_gives(case):
    for B, S in ((case["B"], case["S"]), (64, 40), (1, 7)):
        p = stemops.plan(case["cin"], case["units"], B, S, input_layout=_layout(case))
        assert (p["stat_rows"], p["gemm_rows"], p["conv_tile"], p["stat_tiles_max"]) == (256, 64, 8, 1024)
        want = plan_restated(case, B, S)
        assert p["units"] == want["units"]
        for n in ("saved_bytes", "nosave_bytes", "workspace_bytes"):
            assert p[n] == want[n], (n, B, S)
        for u in p["units"]:
            assert (u["stat_tiles"] - 1) * u["stat_rows"] < u["rows_out"] <= u["stat_tiles"] * u["stat_rows"]


def test_the_statistics_tile_count_is_bounded_at_the_real_stem_shape():
    """edge_n at batch 64, 640 px: 6 553 600 rows leave the stem unit; tiles of 256 rows would be 25 600"""
    meta = zoo_meta("edge_n", num_classes=3, img_size=640)
    units_, eps = stemops._stem_units(meta)
    p = stemops.plan(3, units_, 64, 640, eps=eps, input_layout="nchw")
    case = dict(B=64, S=640, cin=3, planar=True, units=units_)
    assert p["units"] == plan_restated(case)["units"]
    u0 = p["units"][0]
    assert (u0["rows_out"], u0["stat_rows"], u0["stat_tiles"]) == (64 * 320 * 320, 6400, 1024)
    assert all(u["stat_tiles"] <= 1024 and u["stat_rows"] % 256 == 0 for u in p["units"])
    assert [u["stat_rows"] for u in p["units"]] == [6400, 1792, 1792, 512, 512]
    # what the header says the handle keeps: 2.36 GB of z and h, 0.84 GB each for unit 0's, and a 0.31 GB copy of x
    assert u0["saved_bytes"] == 2 * 64 * 320 * 320 * 32 * 4 + 2 * 32 * 4
    x0 = 64 * 640 * 640 * 3 * 4
    assert abs(u0["saved_bytes"] / 2 - 0.84e9) < 0.005e9 and abs(p["saved_bytes"] - x0 - 2.36e9) < 0.01e9 and abs(x0 - 0.31e9) < 0.01e9
    # the weight gradient of the stem unit fills the chip: 1024 splits of 100 spatial tiles
    assert (u0["wgrad_rows"], u0["wgrad_splits"], u0["conv_block"]) == (100, 1024, 32)


def _oracle_keys(name, lo, hi, stem):
    """the entries of stages lo..hi (and conv_stem / bn1) of the oracle's backbone of that name, under `backbone.`"""
    from oracle.backbones import FeatureBackbone
    bb = FeatureBackbone(name)
    return {"backbone." + k: tuple(v.shape) for k, v in bb.state_dict().items()
            if (k.startswith("blocks.") and lo <= int(k.split(".")[1]) <= hi) or (stem and k.split(".")[0] in ("conv_stem", "bn1"))}


@pytest.mark.parametrize("model", ["edge_n", "edge_m"])
def test_the_backbone_has_timms_keys_and_shapes(model):
    meta = zoo_meta(model, num_classes=3, img_size=64)
    with torch.device("meta"):
        stem, mid = ya.BackboneStem.from_meta(meta), ya.BackboneMid.from_meta(meta)
        whole = ya.MobileNetV4Backbone.from_meta(meta)
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}   # noqa: E731
    assert shapes(stem) == _oracle_keys(meta["backbone"], 0, 1, True)
    assert list(stem.state_dict())[:2] == ["backbone.conv_stem.weight", "backbone.bn1.weight"]
    assert [(u["k"], u["s"]) for u in stem.units_cfg] == [(3, 2), (3, 2), (1, 1), (3, 2), (1, 1)]
    cm = 0.5 if model == "edge_n" else 1.0
    assert [u["c"] for u in stem.units_cfg] == [32, int(32 * cm), int(32 * cm), int(96 * cm), int(64 * cm)]   # the stem stays 32
    assert shapes(mid) == _oracle_keys(meta["backbone"], 2, 2, False)
    assert [(b["a"], b["k"], b["s"]) for b in mid.blocks_cfg] == [(5, 5, 2), (0, 3, 1), (0, 3, 1), (0, 3, 1), (0, 3, 1), (3, 0, 1)]
    assert (mid.in_channels, mid.out_channels) == (stem.out_channels, whole.tail.in_channels)
    assert shapes(whole) == _oracle_keys(meta["backbone"], 0, 4, True)
    assert sorted(n.split(".", 1)[1] for n, _ in whole.named_parameters()) == sorted(
        k for k in whole.state_dict() if "running" not in k and "tracked" not in k)


def test_the_tiny_cases_are_what_the_classes_make_of_oracle_tiny():
    case = [c for c in CASES if c["name"] == "stem_to_c3"][0]
    meta = make_meta("YOLOLiteMS_CPU", "oracle_tiny", num_classes=3, img_size=64)
    with torch.device("meta"):
        stem, mid = ya.BackboneStem.from_meta(meta), ya.BackboneMid.from_meta(meta)
        mine = ya.ConvStack(3, case["units"], prefix=case["prefix"], input_layout="nchw")
        mid2 = ya.UIBStack(TINY["mid"]["cin"], TINY["mid"]["blocks"], prefix="backbone.")
    assert stem.units_cfg == mine.units_cfg and list(stem.state_dict()) == list(mine.state_dict())
    assert {k: tuple(v.shape) for k, v in stem.state_dict().items()} == _oracle_keys("oracle_tiny", 0, 1, True)
    assert [u["conv"] for u in units(case)] == ["backbone.conv_stem", "backbone.blocks.0.0.conv", "backbone.blocks.1.0.conv",
                                                "backbone.blocks.1.1.conv"]
    assert mid.blocks_cfg == mid2.blocks_cfg and {k: tuple(v.shape) for k, v in mid.state_dict().items()} == _oracle_keys("oracle_tiny", 2, 2, False)


def test_refusals_raise_before_the_library_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(stemops._lib, "load", boom)
    # backbones whose first stages are made of other blocks, by name
    for bb in ("tf_efficientnet_lite0", "tf_efficientnetv2_b0", "hgnetv2_b0", "convnextv2_atto", "oracle_tiny_tf"):
        meta = make_meta("YOLOLiteMS_CPU", bb, num_classes=3, img_size=64)
        for cls in (ya.BackboneStem, ya.BackboneMid, ya.MobileNetV4Backbone):
            with pytest.raises(ya.YoloLiteHipError, match=f"{bb}.*not implemented"):
                cls.from_meta(meta)
            with pytest.raises(ya.YoloLiteHipError, match="not implemented"):
                cls.from_state_dict(meta, {})
    meta = zoo_meta("edge_n", num_classes=3, img_size=64)
    meta["config"] = dict(meta.get("config") or {})
    meta["config"]["training"] = dict(meta["config"].get("training") or {}, use_p2=True)
    with pytest.raises(ya.YoloLiteHipError, match="use_p2.*not implemented"):
        ya.BackboneStem.from_meta(meta)
    with pytest.raises(ya.YoloLiteHipError, match="start='c3'.*not implemented"):        # the tail keeps refusing it
        ya.BackboneTail.from_meta(zoo_meta("edge_n", num_classes=3, img_size=64), start="c3")
    with pytest.raises(ya.YoloLiteHipError, match="cn block must be 1x1"):               # and the stage a dense 3x3
        ya.UIBStack(8, [dict(type="cn", k=3, s=1, c=8)])
    u = dict(k=3, s=2, c=8)
    # what the kernels do not have, by name
    for extra, word in ((dict(act="relu6"), "relu6"), (dict(act="silu"), "silu"), (dict(same=True), "TF-SAME"),
                        (dict(skip=True), "_skip residual")):
        with pytest.raises(ya.YoloLiteHipError, match=f"{word}.*not implemented"):
            ya.ConvStack(8, [dict(u, **extra)])
    # channel multiples, the planar input's channels
    for cin, unit, layout in ((6, u, "nhwc"), (8, dict(u, c=10), "nhwc"), (3, u, "nhwc"), (5, u, "nchw"), (0, u, "nchw")):
        with pytest.raises(ya.YoloLiteHipError, match="multiple|1..4"):
            ya.ConvStack(cin, [unit], input_layout=layout)
        with pytest.raises(ya.YoloLiteHipError, match="multiple|1..4"):
            stemops.plan(cin, [unit], 2, 4, input_layout=layout)
    with pytest.raises(ya.YoloLiteHipError, match="1..8 units"):
        ya.ConvStack(8, [u] * 9)
    with pytest.raises(ya.YoloLiteHipError, match="1..8 units"):
        ya.ConvStack(8, [])
    for bad in (dict(k=5), dict(k=2), dict(k=0), dict(s=3), dict(s=0)):
        with pytest.raises(ya.YoloLiteHipError, match="unit 0"):
            ya.ConvStack(8, [dict(u, **bad)])
    with pytest.raises(ValueError, match="input_layout"):
        ya.ConvStack(8, [u], input_layout="chw")
    # inputs: the planar image has no gradient, no CPU fallback, shapes, one value per channel in training
    m = ya.ConvStack(3, [u], input_layout="nchw")
    with pytest.raises(ya.YoloLiteHipError, match="no gradient"):
        m(torch.zeros(2, 3, 4, 4, requires_grad=True))
    with pytest.raises(ya.YoloLiteHipError, match="HIP device"):
        m(torch.zeros(2, 3, 4, 4))
    with pytest.raises(ValueError):
        m(torch.zeros(2, 4, 4, 3))
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(torch.zeros(1, 3, 2, 2))                             # S 2 -> 1 under stride 2: ONE output row
    with pytest.raises(ya.YoloLiteHipError, match="HIP device"):
        m.eval()(torch.zeros(1, 3, 2, 2))                      # eval mode: only the device is missing
    n = ya.ConvStack(8, [u])
    with pytest.raises(ya.YoloLiteHipError, match="HIP device"):
        n(torch.zeros(2, 4, 4, 8))
    with pytest.raises(ValueError, match="size="):
        stemops.conv(torch.zeros(1, 2, 2, 8), torch.zeros(8, 4, 3, 3), "dgrad", 3, 2)
    with pytest.raises(ValueError, match="no gradient"):
        stemops.conv(torch.zeros(1, 2, 2, 8), torch.zeros(8, 3, 3, 3), "dgrad", 3, 1, layout="nchw")
    with pytest.raises(ValueError, match="k must be 1 or 3"):
        stemops.conv(torch.zeros(1, 3, 3, 4), torch.zeros(4, 4, 5, 5), "forward", 5, 1)
    with pytest.raises(ya.YoloLiteHipError, match="HIP device"):
        stemops.conv(torch.zeros(1, 3, 3, 4), torch.zeros(4, 4, 3, 3), "forward", 3, 2)


def _raw_cfg(cin, units_, eps=1e-5, nchw=0):
    c = stemops._lib.yl_stem_cfg()
    c.in_channels, c.num_units, c.input_nchw, c.eps = cin, len(units_), nchw, eps
    for i, (k, s, cout) in enumerate(units_[:8]):
        c.unit[i].k, c.unit[i].s, c.unit[i].cout = k, s, cout
    return c


def test_the_library_refuses_them_as_well():
    """YL_ERR_INVALID (-1) from yl_stem_plan and yl_stem_create, host-side checks in front of any device call (create
    with device -1 would otherwise fail with YL_ERR_HIP)"""
    lib = ya.load_library()
    out = stemops._lib.yl_stem_plan_info()
    h = ctypes.c_void_p()
    ok = (3, 2, 8)
    bad = [_raw_cfg(6, [ok]), _raw_cfg(3, [ok]), _raw_cfg(8, [(3, 2, 10)]), _raw_cfg(8, [(5, 2, 8)]), _raw_cfg(8, [(2, 1, 8)]),
           _raw_cfg(8, [(3, 3, 8)]), _raw_cfg(8, [(3, 0, 8)]), _raw_cfg(8, [ok], eps=0.0), _raw_cfg(8, []),
           _raw_cfg(5, [ok], nchw=1), _raw_cfg(0, [ok], nchw=1), _raw_cfg(8, [ok], nchw=2)]
    many = _raw_cfg(8, [ok] * 8)
    many.num_units = 9
    for c in bad + [many]:
        assert lib.yl_stem_plan(ctypes.byref(c), 2, 4, ctypes.byref(out)) == -1
        assert lib.yl_stem_create(-1, ctypes.byref(c), ctypes.byref(h)) == -1
    for good in (_raw_cfg(8, [ok]), _raw_cfg(3, [ok], nchw=1), _raw_cfg(4, [(1, 2, 4)])):
        assert lib.yl_stem_plan(ctypes.byref(good), 2, 4, ctypes.byref(out)) == 0
    assert lib.yl_stem_plan(ctypes.byref(_raw_cfg(8, [ok])), 0, 4, ctypes.byref(out)) == -1
    # one pass on its own: the same facts, and no gradient of the planar image
    n = ctypes.c_int32()
    one = ctypes.c_void_p(16)
    for args in ((0, 5, 1, 1, 4, 4, 4, 0), (0, 3, 3, 1, 4, 4, 4, 0), (0, 3, 1, 1, 4, 6, 4, 0), (0, 3, 1, 1, 4, 4, 10, 0),
                 (3, 3, 1, 1, 4, 4, 4, 0), (1, 3, 1, 1, 4, 3, 4, 1), (0, 3, 1, 1, 4, 5, 4, 1)):
        assert lib.yl_stem_conv(one, one, one, *args, None, ctypes.byref(n)) == -1, args


def test_the_headers_new_symbols_resolve_in_the_built_library():
    text = open(os.path.join(ROOT, "include", "yololite_hip.h")).read()
    names = sorted(set(re.findall(r"\b(yl_stem_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert names == ["yl_stem_backward", "yl_stem_conv", "yl_stem_create", "yl_stem_destroy", "yl_stem_forward", "yl_stem_held",
                     "yl_stem_plan"]
    lib = ya.load_library()
    bound = {n for n, _, _ in stemops._lib.SYMBOLS}
    for n in names:
        assert n in bound and getattr(lib, n) is not None
    assert lib.yl_abi_version() == 7 and "#define YL_ABI_VERSION 7" in text
    assert ctypes.sizeof(stemops._lib.yl_stem_cfg) == 24 + 8 * 16
    assert ctypes.sizeof(stemops._lib.yl_stem_tensors) == 8 * 48
    assert ctypes.sizeof(stemops._lib.yl_stem_unit_plan) == 8 * 4 + 8
    assert ctypes.sizeof(stemops._lib.yl_stem_plan_info) == 16 + 8 * 40 + 24
