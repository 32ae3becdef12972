"""The launch forms the shipped models reach in training against the launch forms a test compares with a reference
(tests/_launch_classes.py).  Host functions only: no device.

The zoo side: every MODEL_ZOO entry at image sizes 640 and 320, B = 16 (the default --batch of tools/finetune_heads.py),
through every trainable module that accepts it (a module that answers "not implemented" for a backbone or an arch is
skipped for that entry).  The test side: the module-level parity cases (CASES and WIDE of the _*_cases.py files, and the
three parts of _stem_cases.TINY) and, for the GEMM's and the depthwise kernels' labels only, the op-level shapes of
test_head_gemm_fp32_gpu.py and test_stage_depthwise_gpu.py.  There is no allow-list: a label the zoo reaches and no test
does fails by name."""
import torch

import yololite_amd as ya
from yololite_amd import headops, neckops, stageops, stemops
from yololite_amd.program import MODEL_ZOO, zoo_meta
import _dense_neck_cases as dc
import _head_cases as hc
import _launch_classes as lc
import _neck_cases as nc
import _stage_cases as sc
import _stem_cases as tc

BATCH, IMG_SIZES = 16, (640, 320)
OP_SOURCES = ("gemm", "stage_dw_")                       # what an op-level shape may vouch for


def _or_none(make):
    try:
        with torch.device("meta"):
            return make()
    except ya.YoloLiteHipError as e:
        assert "not implemented" in str(e), e
        return None


def zoo_modules():
    """-> [(zoo name, image size, kind, arguments of the kind's label and plan functions)]"""
    out = []
    for name in MODEL_ZOO:
        meta = zoo_meta(name)
        heads = _or_none(lambda: ya.DetectHeads.from_meta(meta))
        neck = _or_none(lambda: ya.neck_for(meta))
        stem = _or_none(lambda: ya.BackboneStem.from_meta(meta))
        mid = _or_none(lambda: ya.BackboneMid.from_meta(meta))
        tail = _or_none(lambda: ya.BackboneTail.from_meta(meta))
        for img in IMG_SIZES:
            sizes = tuple(img // s for s in (8, 16, 32))
            if heads is not None:
                assert heads.level_names == ("p3", "p4", "p5")
                for A, S in zip(heads.num_anchors_per_level, sizes):
                    out.append((name, img, "heads", (heads.fpn_channels, heads.num_classes, A, heads.head_depth, BATCH, (S,))))
            if neck is not None:
                kind = "dense_neck" if isinstance(neck, ya.DetectNeckMS) else "neck"
                out.append((name, img, kind, (tuple(neck.in_channels), neck.fpn_channels, neck.depth, BATCH, sizes)))
            if stem is not None:
                units = [dict(k=d["k"], s=d["s"], c=d["c"]) for d in stem.units_cfg]
                out.append((name, img, "stem", (stem.in_channels, units, BATCH, img, True)))
            for m, S in ((mid, sizes[0]), (tail, sizes[1])):
                if m is not None:
                    out.append((name, img, "stage", (m.in_channels, _blocks(m.blocks_cfg), BATCH, S)))
    return out


def _blocks(cfg):
    return [{k: d[k] for k in ("type", "a", "k", "s", "mid", "c", "name") if k in d} for d in cfg]


def case_modules(wide=True):
    """the module-level parity cases in the same form"""
    out = []
    for c in hc.CASES + (hc.WIDE if wide else []):
        out.append((c["name"], None, "heads", (c["F"], c["C"], c["A"], c["depth"], c["B"], tuple(c["sizes"]))))
    for mod, kind in ((nc, "neck"), (dc, "dense_neck")):
        for c in mod.CASES + (mod.WIDE if wide else []):
            out.append((c["name"], None, kind, (tuple(c["Cin"]), c["F"], c["depth"], c["B"], tuple(c["sizes"]))))
    for c in sc.CASES + (sc.WIDE if wide else []) + [tc.TINY["mid"], tc.TINY["tail"]]:
        out.append((c["name"], None, "stage", (c["cin"], c["blocks"], c["B"], c["S"])))
    for c in tc.CASES + (tc.WIDE if wide else []) + [tc.TINY["stem"]]:
        out.append((c["name"], None, "stem", (c["cin"], c["units"], c["B"], c["S"], c["planar"])))
    return out


LABELS = dict(heads=lc.head_labels, neck=lc.neck_labels, dense_neck=lc.dense_neck_labels, stage=lc.stage_labels,
              stem=lc.stem_labels)


def op_labels(wide=True):
    out = set()
    for c in (hc.GEMM_OP_SHAPES if wide else []):
        out |= lc.head_gemm_op_labels(c["F"], c["C"], c["A"], c["B"], c["sizes"][0])
    for k, s in sc.DW_OP_KS:
        for B, S, C in sc.DW_OP_SHAPES + (sc.DW_OP_WIDE if wide else []):
            out |= lc.depthwise_op_labels(k, s, B, S, C)
    return {l for l in out if l[0].startswith(OP_SOURCES)}


def uncovered(wide=True):
    """{label: the first zoo (model, image size, module) that reaches it} of the labels no test reaches; wide = False: with
    the case lists as they were before the WIDE lists and the op-level additions"""
    covered = op_labels(wide)
    for _, _, kind, args in case_modules(wide):
        covered |= LABELS[kind](*args)
    out = {}
    for name, img, kind, args in zoo_modules():
        for l in LABELS[kind](*args):
            if l not in covered:
                out.setdefault(l, (name, img, kind))
    return out


def _same(got, want, who):
    for k, v in want.items():
        assert got[k] == v, (who, k, got[k], v)


def test_the_restatement_is_the_librarys():
    """row tiles, weight-gradient rows and split counts of every parity case and every zoo shape: _launch_classes.py
    against headops.plan, neckops.plan, neckops.plan_ms, stageops.plan and stemops.plan (pick_pt and pick_cq are not
    reported: they are restated from the header and covered through the splits)"""
    n = 0
    for name, img, kind, a in case_modules() + zoo_modules():
        who = (name, img, kind)
        if kind == "heads":
            F, C, A, depth, B, sizes = a
            for S in sizes:
                _same(headops.plan(F, C, A, depth, B, S), lc.head_plan(F, C, A, depth, B, S), who)
        elif kind in ("neck", "dense_neck"):
            lib = (neckops.plan if kind == "neck" else neckops.plan_ms)(*a)
            mine = (lc.neck_plan if kind == "neck" else lc.dense_neck_plan)(*a)
            assert lib["stat_rows"] == lc.STAT_ROWS and lib["gemm_rows"] == lc.GEMM_ROWS and len(lib["levels"]) == len(mine)
            if kind == "dense_neck":
                assert lib["conv_tile"] == lc.CT
            for li, (g, w) in enumerate(zip(lib["levels"], mine)):
                _same(g, w, who + (li,))
        elif kind == "stage":
            lib, mine = stageops.plan(*a), lc.stage_plan(*a)
            assert lib["stat_rows"] == lc.STAT_ROWS and lib["gemm_rows"] == lc.GEMM_ROWS and len(lib["blocks"]) == len(mine)
            for bi, (g, w) in enumerate(zip(lib["blocks"], mine)):
                _same(g, w, who + (bi,))
        else:
            cin, units, B, S, planar = a
            lib = stemops.plan(cin, units, B, S, input_layout="nchw" if planar else "nhwc")
            mine = lc.stem_units(cin, units, B, S, planar)
            assert lib["stat_rows"] == lc.STAT_ROWS and lib["conv_tile"] == lc.ST_T and lib["stat_tiles_max"] == lc.STAT_TILES_MAX
            assert len(lib["units"]) == len(mine)
            for ui, (g, w) in enumerate(zip(lib["units"], mine)):
                _same(g, {k: w[k] for k in ("stat_rows", "stat_tiles", "wgrad_rows", "wgrad_splits", "conv_block")}, who + (ui,))
                assert (g["size_in"], g["size_out"], g["rows_out"]) == (w["Sin"], w["Sout"], w["M"]), who
        n += 1
    assert n > 100
    # the bounds of split_plan the op-level shapes are there for, as the library cuts them
    for c in hc.GEMM_OP_SHAPES:
        rows, splits, bound = c["wgrad"]
        p = headops.plan(c["F"], c["C"], c["A"], c["depth"], c["B"], c["sizes"][0])
        assert (p["wgrad_rows"], p["wgrad_splits"]) == (rows, splits), (c["name"], p)
        assert lc.split_plan(p["rows"], c["F"], c["F"]) == (rows, splits, bound), c["name"]


def test_every_launch_form_the_zoo_reaches_is_reached_by_a_test():
    zoo = zoo_modules()
    kinds = {(name, kind) for name, _, kind, _ in zoo}
    assert {k for _, k in kinds} == set(LABELS)              # every kind of module is reached by some model
    assert {n for n, k in kinds if k == "heads"} == set(MODEL_ZOO)
    assert {n for n, k in kinds if k == "stem"} == {n for n, k in kinds if k == "stage"} == {"edge_n", "edge_s", "edge_m", "edge_l"}
    missing = uncovered()
    lines = [f"{' / '.join(l)}    (first: {who[0]} at {who[1]}, {who[2]})" for l, who in sorted(missing.items())]
    assert not missing, "launch forms of the zoo that no test compares with a reference:\n" + "\n".join(lines)
