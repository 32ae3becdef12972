"""Host side of the trainable FPN neck (yololite_amd.neckops): the float64 restatement against the reference's fixture,
the nearest map against F.interpolate, the module's names / shapes / dtypes, the row planner and the refusals that need
no device.  No HIP compute here."""
import ctypes
import json
import re
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import yololite_amd as ya
from yololite_amd import neckops
from _neck_cases import CASES, E2E, FIXTURE, FIXTURE_WIDE, KEYS, WIDE, case_inputs, fixture_tensors, level_names, modes
from _neck_np import nearest_src, neck_all

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def wide():
    return np.load(FIXTURE_WIDE)


@pytest.mark.parametrize("case", CASES + WIDE, ids=[c["name"] for c in CASES + WIDE])
def test_float64_restatement_reproduces_the_reference(case, fixture, wide):
    """tests/_neck_np.py in float64 against the reference's own float64 run: every tensor to 1e-12 of its largest value"""
    inputs = case_inputs(case)
    for mode in modes(case):
        got = neck_all(inputs, case["depth"], mode == "train")
        for li in range(len(inputs)):
            want = fixture_tensors(wide if case in WIDE else fixture, case, mode, li)
            assert set(got[li]) == set(want)
            for n, (r64, idx, _, m64) in want.items():
                g = np.asarray(got[li][n], np.float64).reshape(-1)
                g = g if idx is None else g[idx]
                assert np.abs(g - r64).max() <= 1e-12 * max(m64, 1.0), (case["name"], mode, li, n)


def test_nearest_map_is_torchs_and_its_ranges_partition_the_destination():
    for n_in in range(1, 41):
        for n_out in range(1, 81):
            want = TF.interpolate(torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in), size=(1, n_out),
                                  mode="nearest").view(-1).to(torch.int64).numpy()
            src, lo, hi = neckops.nearest_map(n_out, n_in)
            assert np.array_equal(src, want), (n_in, n_out)
            assert np.array_equal(nearest_src(n_out, n_in), want), (n_in, n_out)      # the restatement's own map
            assert lo[0] == 0 and hi[-1] == n_out and np.array_equal(lo[1:], hi[:-1]) and (lo <= hi).all()
            for i in range(n_in):
                assert (src[lo[i]:hi[i]] == i).all()


def test_the_maps_the_cases_name():
    assert neckops.nearest_map(5, 3)[0].tolist() == [0, 0, 1, 1, 2]
    assert neckops.nearest_map(3, 2)[0].tolist() == [0, 0, 1]
    assert neckops.nearest_map(8, 4)[0].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]


@pytest.mark.parametrize("B,sizes", [(1, (2, 1)), (2, (8, 4, 2)), (3, (5, 3, 2)), (2, (24, 12)), (64, (80, 40, 20)),
                                     (7, (13, 7, 4, 2))])
@pytest.mark.parametrize("F,cin,d", [(16, 8, 1), (96, 480, 2), (20, 36, 4)])
def test_plan_covers_every_row_once_and_counts_the_bytes_its_docstring_gives(B, sizes, F, cin, d):
    cins = (cin,) * len(sizes)
    p = neckops.plan(cins, F, d, B, sizes)
    Ms = [B * S * S for S in sizes]
    for lp, M, ci in zip(p["levels"], Ms, cins):
        assert lp["rows"] == M
        for r, t in ((p["stat_rows"], lp["stat_tiles"]), (p["gemm_rows"], lp["gemm_tiles"]),
                     (lp["wgrad_rows"], lp["wgrad_splits"]), (lp["lgrad_rows"], lp["lgrad_splits"])):
            hit = np.zeros(M, np.int32)
            for i in range(t):
                assert i * r < M, "an empty tile"
                hit[i * r:min(M, (i + 1) * r)] += 1
            assert (hit == 1).all(), (r, t)
        assert lp["wgrad_rows"] % 16 == 0 and lp["lgrad_rows"] % 16 == 0
        assert lp["saved_bytes"] == (1 + 3 * d) * M * F * 4 + d * 2 * F * 4
    Mmax = max(Ms)
    assert p["saved_bytes"] == sum(lp["saved_bytes"] for lp in p["levels"])
    assert p["nosave_bytes"] == 4 * Mmax * F * 4 + 2 * F * 4
    r16 = lambda v: (v + 15) // 16 * 16                                     # noqa: E731
    wpart = max(r16(max(lp["wgrad_splits"] * F * F, lp["lgrad_splits"] * F * ci) * 4) for lp, ci in zip(p["levels"], cins))
    assert p["workspace_bytes"] == 3 * Mmax * F * 4 + max(lp["stat_tiles"] for lp in p["levels"]) * 9 * F * 8 + \
        2 * F * 4 + wpart
    assert p["table_bytes"] == sum((a + 2 * b) * 4 for a, b in zip(sizes[:-1], sizes[1:]))


def test_module_has_the_references_keys_shapes_and_dtypes(fixture):
    want = [(n, tuple(sh), dt) for n, sh, dt in json.loads(str(fixture["keys"]))]
    with torch.device("meta"):
        m = ya.DetectNeck(KEYS["Cin"], KEYS["F"], KEYS["depth"])
    got = [(n, tuple(v.shape), str(v.dtype)) for n, v in m.state_dict().items()]
    assert got == want
    assert [n for n, _ in m.named_parameters()] == [n for n, _, _ in want if "running" not in n and "tracked" not in n]


def test_from_meta_and_from_state_dict_read_the_program():
    from yololite_amd.program import build_program, synth_state_dict, zoo_meta
    meta = zoo_meta("edge_n", num_classes=3, img_size=64)
    sd = synth_state_dict(meta)
    prog = build_program(meta, sd)
    a = ya.DetectNeck.from_meta(meta)
    b = ya.DetectNeck.from_state_dict(meta, sd)
    mcfg = meta["config"]["model"]
    assert a.level_names == b.level_names == ("p3", "p4", "p5")
    assert a.fpn_channels == int(mcfg["fpn_channels"] * mcfg.get("width_multiple", 1.0))
    assert a.depth == b.depth == max(1, round(2 * mcfg.get("depth_multiple", 1.0)))
    assert a.in_channels == b.in_channels == tuple(prog.slots[prog.feature_slots[c]][2] for c in ("c3", "c4", "c5"))
    for k, v in b.state_dict().items():
        if not k.endswith("num_batches_tracked") or k in sd:
            assert torch.equal(v, torch.as_tensor(sd[k]).reshape(v.shape).to(v.dtype)), k
    assert list(a.state_dict()) == list(b.state_dict())
    assert all(k in sd for k in a.state_dict() if not k.endswith("num_batches_tracked"))


def test_refusals_raise_before_the_library_is_touched(monkeypatch):
    from yololite_amd.program import zoo_meta

    def boom(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(neckops._lib, "load", boom)
    meta = zoo_meta("edge_n", num_classes=3, img_size=64)
    with pytest.raises(ya.YoloLiteHipError, match="not implemented"):
        ya.DetectNeck.from_meta(dict(meta, arch="YOLOLiteMS"))
    p6 = dict(meta, config=dict(meta["config"], training=dict(meta["config"]["training"], use_p6=True)))
    with pytest.raises(ya.YoloLiteHipError, match="P6.*not implemented"):
        ya.DetectNeck.from_meta(p6)
    with pytest.raises(ya.YoloLiteHipError, match="P6.*not implemented"):
        ya.DetectNeck.from_state_dict(p6, {})
    for F in (18, 2, 0, 97):
        with pytest.raises(ya.YoloLiteHipError, match="fpn_channels must be a multiple of 4"):
            ya.DetectNeck((8, 8, 8), F)
        with pytest.raises(ya.YoloLiteHipError, match="multiple of 4"):
            neckops.plan((8, 8, 8), F, 1, 2, (8, 4, 2))
    with pytest.raises(ya.YoloLiteHipError, match="in_channels must be multiples of 4"):
        ya.DetectNeck((8, 10, 8), 16)
    with pytest.raises(ya.YoloLiteHipError, match="depth must be 1..4"):
        ya.DetectNeck((8, 8, 8), 16, 5)
    m = ya.DetectNeck((8, 12, 20), 16)
    with pytest.raises(ya.YoloLiteHipError, match="HIP device"):
        m([torch.zeros(2, s, s, c) for s, c in zip((8, 4, 2), (8, 12, 20))], layout="nhwc")
    with pytest.raises(ValueError):
        m([torch.zeros(2, 8, 8, 8)] * 2)
    with pytest.raises(ValueError, match="layout="):
        ya.DetectNeck((8,), 16, level_names=("p3",))([torch.zeros(2, 8, 8, 8)])


def test_the_library_refuses_them_as_well():
    lib = ya.load_library()
    out = neckops._lib.yl_neck_plan_info()
    sz = (ctypes.c_int32 * 3)(8, 4, 2)
    assert lib.yl_neck_plan(ctypes.byref(neckops._cfg((8, 8, 8), 18, 1)), 2, sz, ctypes.byref(out)) == -5
    assert lib.yl_neck_plan(ctypes.byref(neckops._cfg((8, 10, 8), 16, 1)), 2, sz, ctypes.byref(out)) == -5
    assert lib.yl_neck_plan(ctypes.byref(neckops._cfg((8, 8, 8), 16, 5)), 2, sz, ctypes.byref(out)) != 0
    assert lib.yl_neck_plan(ctypes.byref(neckops._cfg((8, 8, 8), 16, 1)), 2, sz, ctypes.byref(out)) == 0


def test_the_headers_new_symbols_resolve_in_the_built_library():
    text = open(os.path.join(ROOT, "include", "yololite_hip.h")).read()
    names = sorted(set(re.findall(r"\b(yl_neck_[a-z_]+)\s*\(", text)))
    assert names == ["yl_neck_backward", "yl_neck_create", "yl_neck_destroy", "yl_neck_forward", "yl_neck_held",
                     "yl_neck_nearest_map", "yl_neck_plan"]
    lib = ya.load_library()
    bound = {n for n, _, _ in neckops._lib.SYMBOLS}
    for n in names:
        assert n in bound and getattr(lib, n) is not None
    assert ctypes.sizeof(neckops._lib.yl_neck_cfg) == 32
    assert ctypes.sizeof(neckops._lib.yl_neck_level) == 16 + 4 * 56


def test_the_cpu_loops_own_drop_is_a_fifth_of_the_first_loss(fixture):
    """the end-to-end test's yardstick (run once by the generator, tests/_neck_np.py fit_reference)"""
    losses = fixture["e2e/losses"]
    assert len(losses) == E2E["steps"] + 1 and np.isfinite(losses).all()
    assert losses[0] - losses[-1] >= 0.2 * losses[0]


def test_level_names_of_the_cases():
    assert [level_names(c) for c in CASES if c["name"] in ("base", "wide", "l4")] == [
        ("p3", "p4", "p5"), ("p4", "p5"), ("p2", "p3", "p4", "p5")]
