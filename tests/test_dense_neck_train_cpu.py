"""Host side of the trainable dense FPN neck (yololite_amd.neckops.DetectNeckMS): the float64 restatement against the
reference's fixture, the module's names / shapes / dtypes, the planner and the refusals that need no device.  No HIP
compute here."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import yololite_amd as ya
from yololite_amd import neckops
from _dense_neck_cases import CASES, E2E, FIXTURE, FIXTURE_WIDE, KEYS, WIDE, case_inputs, fixture_tensors, level_names, modes
from _dense_neck_np import neck_all

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def wide():
    return np.load(FIXTURE_WIDE)


def test_the_fixture_is_a_committable_file():
    assert os.path.getsize(FIXTURE) < (1 << 20) and os.path.getsize(FIXTURE_WIDE) < (1 << 20)


@pytest.mark.parametrize("case", CASES + WIDE, ids=[c["name"] for c in CASES + WIDE])
def test_float64_restatement_reproduces_the_reference(case, fixture, wide):
    """tests/_dense_neck_np.py in float64 against the reference's own float64 run: every tensor to 1e-12 of its largest
    value.  One tensor's true value is zero (case tiny, g.lateral5.bias: at S = 1 the bias is a constant per channel in
    front of a train-mode BatchNorm; the fixture holds 5e-15): two float64 evaluations of a sum of O(10) terms that
    cancels differ by a few times 10 * 2^-52, so the bound has the floor 1e-13, which no tensor of O(0.1) or more feels"""
    inputs = case_inputs(case)
    for mode in modes(case):
        got = neck_all(inputs, case["depth"], mode == "train")
        for li in range(len(inputs)):
            want = fixture_tensors(wide if case in WIDE else fixture, case, mode, li)
            assert set(got[li]) == set(want)
            for n, (r64, idx, _, m64) in want.items():
                g = np.asarray(got[li][n], np.float64).reshape(-1)
                g = g if idx is None else g[idx]
                assert np.abs(g - r64).max() <= max(1e-12 * m64, 1e-13), (case["name"], mode, li, n)


def test_module_has_the_references_keys_shapes_dtypes_and_parameter_order(fixture):
    want = [(n, tuple(sh), dt) for n, sh, dt in json.loads(str(fixture["keys"]))]
    assert ("smooth3.3.weight", (16, 16, 3, 3), "torch.float32") in want and not any(".block." in n for n, _, _ in want)
    with torch.device("meta"):
        m = ya.DetectNeckMS(KEYS["Cin"], KEYS["F"], KEYS["depth"])
    got = [(n, tuple(v.shape), str(v.dtype)) for n, v in m.state_dict().items()]
    assert got == want
    assert [n for n, _ in m.named_parameters()] == [n for n, _, _ in want if "running" not in n and "tracked" not in n]
    with torch.device("meta"):
        m4 = ya.DetectNeckMS((8, 8, 8, 8), 16, 1, level_names=("p2", "p3", "p4", "p5"))
    assert [n.split(".")[0] for n, _ in m4.named_parameters()][:5] == ["lateral2", "lateral2", "smooth2", "smooth2", "smooth2"]


def test_from_meta_and_from_state_dict_read_the_program():
    from yololite_amd.program import build_program, synth_state_dict, zoo_meta
    meta = zoo_meta("yololite_n", num_classes=3, img_size=64)
    sd = synth_state_dict(meta)
    prog = build_program(meta, sd)
    a = ya.DetectNeckMS.from_meta(meta)
    b = ya.DetectNeckMS.from_state_dict(meta, sd)
    noarch = {k: v for k, v in meta.items() if k != "arch"}
    noarch["config"] = dict(meta["config"], model={k: v for k, v in meta["config"]["model"].items() if k != "arch"})
    c = ya.DetectNeckMS.from_state_dict(noarch, sd)           # a missing arch is YOLOLiteMS
    mcfg = meta["config"]["model"]
    assert a.level_names == b.level_names == c.level_names == ("p3", "p4", "p5")
    assert a.fpn_channels == int(mcfg["fpn_channels"] * mcfg.get("width_multiple", 1.0))
    assert a.depth == b.depth == max(1, round(2 * mcfg.get("depth_multiple", 1.0)))
    assert a.in_channels == b.in_channels == tuple(prog.slots[prog.feature_slots[c]][2] for c in ("c3", "c4", "c5"))
    for k, v in b.state_dict().items():
        if not k.endswith("num_batches_tracked") or k in sd:
            assert torch.equal(v, torch.as_tensor(sd[k]).reshape(v.shape).to(v.dtype)), k
    assert list(a.state_dict()) == list(b.state_dict()) == list(c.state_dict())
    assert all(k in sd for k in a.state_dict() if not k.endswith("num_batches_tracked"))
    assert type(neckops.neck_for(meta)) is ya.DetectNeckMS and type(ya.neck_for(meta, sd)) is ya.DetectNeckMS
    assert type(ya.neck_for(zoo_meta("edge_n", num_classes=3, img_size=64))) is ya.DetectNeck


def test_refusals_raise_before_the_library_is_touched(monkeypatch):
    from yololite_amd.program import zoo_meta

    def boom(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(neckops._lib, "load", boom)
    meta = zoo_meta("yololite_n", num_classes=3, img_size=64)
    with pytest.raises(ya.YoloLiteHipError, match="DetectNeck's"):
        ya.DetectNeckMS.from_meta(zoo_meta("edge_n", num_classes=3, img_size=64))
    with pytest.raises(ya.YoloLiteHipError, match="DetectNeck's"):
        ya.DetectNeckMS.from_state_dict(dict(meta, arch="YOLOLiteMS_CPU"), {})
    p6 = dict(meta, config=dict(meta["config"], training=dict(meta["config"]["training"], use_p6=True)))
    with pytest.raises(ya.YoloLiteHipError, match="P6.*not implemented"):
        ya.DetectNeckMS.from_meta(p6)
    with pytest.raises(ya.YoloLiteHipError, match="P6.*not implemented"):
        ya.DetectNeckMS.from_state_dict(p6, {})
    with pytest.raises(ya.YoloLiteHipError, match="P6.*not implemented"):
        ya.neck_for(p6)
    for F in (18, 2, 0, 97):
        with pytest.raises(ya.YoloLiteHipError, match="fpn_channels must be a multiple of 4"):
            ya.DetectNeckMS((8, 8, 8), F)
        with pytest.raises(ya.YoloLiteHipError, match="multiple of 4"):
            neckops.plan_ms((8, 8, 8), F, 1, 2, (8, 4, 2))
    with pytest.raises(ya.YoloLiteHipError, match="in_channels must be multiples of 4"):
        ya.DetectNeckMS((8, 10, 8), 16)
    with pytest.raises(ya.YoloLiteHipError, match="depth must be 1..4"):
        ya.DetectNeckMS((8, 8, 8), 16, 5)
    m = ya.DetectNeckMS((8, 12, 20), 16)
    with pytest.raises(ya.YoloLiteHipError, match="DetectNeckMS needs its inputs on a HIP device"):
        m([torch.zeros(2, s, s, c) for s, c in zip((8, 4, 2), (8, 12, 20))], layout="nhwc")
    with pytest.raises(ValueError):
        m([torch.zeros(2, 8, 8, 8)] * 2)
    with pytest.raises(ValueError, match="layout="):
        ya.DetectNeckMS((8,), 16, level_names=("p3",))([torch.zeros(2, 8, 8, 8)])


def test_the_library_refuses_them_as_well():
    lib = ya.load_library()
    out = neckops._lib.yl_dneck_plan_info()
    sz = (ctypes.c_int32 * 3)(8, 4, 2)
    assert lib.yl_dneck_plan(ctypes.byref(neckops._cfg((8, 8, 8), 18, 1)), 2, sz, ctypes.byref(out)) == -5
    assert lib.yl_dneck_plan(ctypes.byref(neckops._cfg((8, 10, 8), 16, 1)), 2, sz, ctypes.byref(out)) == -5
    assert lib.yl_dneck_plan(ctypes.byref(neckops._cfg((8, 8, 8), 16, 5)), 2, sz, ctypes.byref(out)) != 0
    assert lib.yl_dneck_plan(ctypes.byref(neckops._cfg((8, 8, 8), 16, 1)), 0, sz, ctypes.byref(out)) != 0
    assert lib.yl_dneck_plan(ctypes.byref(neckops._cfg((8, 8, 8), 16, 1)), 2, sz, ctypes.byref(out)) == 0


PLAN_SHAPES = [(B, sizes, F, cin, d)
               for B, sizes in [(1, (2, 1)), (2, (8, 4, 2)), (3, (5, 3, 2)), (2, (24, 12)), (64, (80, 40, 20)), (7, (13, 7, 4, 2))]
               for F, cin, d in [(16, 8, 1), (96, 480, 2), (20, 36, 4)]] + [(16, (80, 40, 20), 512, 352, 2)]


@pytest.mark.parametrize("B,sizes,F,cin,d", PLAN_SHAPES)
def test_plan_covers_every_row_and_tile_once_and_counts_the_bytes_its_docstring_gives(B, sizes, F, cin, d):
    cins = (cin,) * len(sizes)
    p = neckops.plan_ms(cins, F, d, B, sizes)
    T = p["conv_tile"]
    assert T == 8
    Ms = [B * S * S for S in sizes]
    blocks = ((F + 63) // 64) ** 2
    for lp, M, S in zip(p["levels"], Ms, sizes):
        assert lp["rows"] == M
        for r, t in ((p["stat_rows"], lp["stat_tiles"]), (p["gemm_rows"], lp["gemm_tiles"]),
                     (lp["lgrad_rows"], lp["lgrad_splits"])):
            hit = np.zeros(M, np.int32)
            for i in range(t):
                assert i * r < M, "an empty tile"
                hit[i * r:min(M, (i + 1) * r)] += 1
            assert (hit == 1).all(), (r, t)
        assert lp["lgrad_rows"] % 16 == 0
        # the spatial tiles cover every pixel of every image once, and the splits every tile once
        TX = -(-S // T)
        assert lp["conv_tiles"] == B * TX * TX
        pix = np.zeros((B, S, S), np.int32)
        tiles = np.zeros(lp["conv_tiles"], np.int32)
        for z in range(lp["w3grad_splits"]):
            assert z * lp["w3grad_tiles"] < lp["conv_tiles"], "an empty split"
            for t in range(z * lp["w3grad_tiles"], min(lp["conv_tiles"], (z + 1) * lp["w3grad_tiles"])):
                tiles[t] += 1
                b, tr = divmod(t, TX * TX)
                ty, tx = divmod(tr, TX)
                pix[b, ty * T:(ty + 1) * T, tx * T:(tx + 1) * T] += 1
        assert (tiles == 1).all() and (pix == 1).all()
        want = min(lp["conv_tiles"], 64, max(1, 512 // blocks))
        assert lp["w3grad_tiles"] == -(-lp["conv_tiles"] // want)
        assert lp["w3grad_splits"] == -(-lp["conv_tiles"] // lp["w3grad_tiles"])
        assert lp["saved_bytes"] == (1 + 2 * d) * M * F * 4 + d * 2 * F * 4
    Mmax = max(Ms)
    assert p["saved_bytes"] == sum(lp["saved_bytes"] for lp in p["levels"])
    assert p["nosave_bytes"] == 3 * Mmax * F * 4 + 2 * F * 4
    r16 = lambda v: (v + 15) // 16 * 16                                     # noqa: E731
    wpart = max(r16(max(lp["w3grad_splits"] * 9 * F * F, lp["lgrad_splits"] * F * ci) * 4) for lp, ci in zip(p["levels"], cins))
    assert p["workspace_bytes"] == 3 * Mmax * F * 4 + r16(max(lp["stat_tiles"] for lp in p["levels"]) * 2 * F * 8) + \
        2 * F * 4 + 9 * F * F * 4 + wpart
    assert p["table_bytes"] == sum((a + 2 * b) * 4 for a, b in zip(sizes[:-1], sizes[1:]))


def test_the_cases_reach_what_they_are_there_for():
    by = {c["name"]: c for c in CASES}
    rows = neckops.plan_ms(by["rows"]["Cin"], 16, 1, 2, by["rows"]["sizes"])["levels"][0]
    assert rows["conv_tiles"] == 18 and rows["w3grad_splits"] > 1
    assert -(-by["wide"]["F"] // 64) == 2 and -(-by["wide"]["F"] // 16) == 7 and by["wide"]["F"] % 16
    assert by["odd"]["F"] % 16 and by["tiny"]["sizes"][-1] == 1 and by["tiny"]["F"] < 16
    assert [level_names(c) for c in CASES if c["name"] in ("base", "wide", "l4")] == [
        ("p3", "p4", "p5"), ("p4", "p5"), ("p2", "p3", "p4", "p5")]


def test_the_headers_new_symbols_resolve_in_the_built_library():
    text = open(os.path.join(ROOT, "include", "yololite_hip.h")).read()
    names = sorted(set(re.findall(r"\b(yl_dneck_[a-z_]+)\s*\(", text)))
    assert names == ["yl_dneck_backward", "yl_dneck_create", "yl_dneck_destroy", "yl_dneck_forward", "yl_dneck_held",
                     "yl_dneck_plan"]
    lib = ya.load_library()
    bound = {n for n, _, _ in neckops._lib.SYMBOLS}
    for n in names:
        assert n in bound and getattr(lib, n) is not None
    assert ctypes.sizeof(neckops._lib.yl_dneck_block) == 48
    assert ctypes.sizeof(neckops._lib.yl_dneck_level) == 16 + 4 * 48
    assert ctypes.sizeof(neckops._lib.yl_dneck_level_plan) == 40
    assert ctypes.sizeof(neckops._lib.yl_dneck_plan_info) == 16 + 4 * 40 + 32


def test_the_cpu_loops_own_drop_is_a_fifth_of_the_first_loss(fixture):
    """the end-to-end test's yardstick (run once by the generator, tests/_dense_neck_np.py fit_reference)"""
    losses = fixture["e2e/losses"]
    assert len(losses) == E2E["steps"] + 1 and np.isfinite(losses).all()
    assert losses[0] - losses[-1] >= 0.2 * losses[0]
