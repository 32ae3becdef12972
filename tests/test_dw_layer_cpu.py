"""The depthwise -> 1x1 layer tests' own instruments, held on the CPU (tests/_dw_cases.py): the fp32 yardstick meets the bar,
planted mistakes do not, the cases reach every instantiation the library can name and every launch class the MODEL_ZOO
models reach, and the query refuses what the kernels refuse.  No device: what runs is yl_query_dw_form's answer (host code)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _dw_cases as dc

_CACHE = {}
HOST_IMAGES = 2


def _case_data(tag):
    """(x, res, float64 reference, yardstick row) of a case on its host inputs; computed once and left unchanged.  At most
    HOST_IMAGES images of a case: what is held here is the arithmetic on the case's channels, grid, padding, activations and
    residual, which no further image adds to (the batch decides the kernel, and the device tests run all of it)."""
    if tag not in _CACHE:
        c = dc.BY_TAG[tag]
        x, res = dc.host_inputs(c, HOST_IMAGES)
        ref = dc.reference(c, x, res)
        _CACHE[tag] = (x, res, ref, dc.row(ref, dc.yardstick(c, x, res)))
    return _CACHE[tag]


def _reaches_the_clamp(tag):
    """the case has a ReLU6 and, in float64, a value beyond 6 in front of one (a 1 x 1 grid under a 5 x 5 window sees one tap:
    its values stay below)"""
    c = dc.BY_TAG[tag]
    if dc.ACT_RELU6 not in ((c["act"],) if c["op"] == "dw" else (c["dw_act"], c["act"])):
        return False
    x, res, ref, _ = _case_data(tag)
    return bool(np.abs(dc.layer_op(c, x, res, torch.float64, clamp6=False) - ref).max() > 0)


def test_relu6_clamp_is_reached_in_every_family_that_has_the_activation():
    """the cases built to catch a missing upper clamp: every family has one, by the default form's kernel"""
    fam = {}
    for c in dc.CASES:
        if dc.ACT_RELU6 in ((c["act"],) if c["op"] == "dw" else (c["dw_act"], c["act"])) and c["B"] <= 3:
            fam.setdefault(dc.FAMILY[dc.query_case(c)[0]], []).append(_reaches_the_clamp(c["tag"]))
    assert set(fam) == {"dwk", "dws", "dwt", "dwh", "mfma", "dw_tile"}, sorted(fam)
    assert all(any(v) for v in fam.values()), {k: sum(v) for k, v in fam.items()}


def test_the_library_has_the_query_and_the_ids_are_the_headers():
    from yololite_amd import _lib
    assert hasattr(C.CDLL(_lib.LIB_PATH), "yl_query_dw_form") and _lib.load().yl_abi_version() == 7
    assert (_lib.OP_CONV, _lib.OP_DW) == (dc.OP_CONV, dc.OP_DW)
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "yololite_hip.h")).read()
    ids = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"YL_DWF_(\w+) = (\d+)", text)}
    assert ids == {(v or "none"): k for k, v in dc.FAMILY.items()}
    assert _lib.load().yl_query_dw_form(dc.OP_CONV, 96, 96, 3, 1, 1, 1, 8, 8, 8, 8, 1, 1, 0, 0, 0, 0, None) == dc.DWT   # args may be NULL


@pytest.mark.parametrize("tag", dc.TAGS)
def test_yardstick_meets_the_bar_and_planted_mistakes_do_not(tag):
    """The fp32 yardstick is within the bar of float64 (by the bar's construction: a quarter of it).  Each single mistake a
    kernel could make on this case exceeds the bar at least tenfold: the symmetric pad where TF-SAME is asked for (and the
    reverse), the tap on the last column / row dropped, the channel tail read as zero, one k-block left out of the 1x1 sum,
    the residual added in front of the activation, ReLU6 without its upper clamp, the depthwise bias dropped."""
    c = dc.BY_TAG[tag]
    x, res, ref, r = _case_data(tag)
    bar_ = r["bar"]
    assert np.isfinite(ref).all() and r["err32"] <= bar_
    Gi, lead, _ = dc.geometry(c)

    def err(y):
        return float(np.abs(y.astype(np.float64) - ref).max())

    f32 = torch.float32
    wrong = {"last column tap dropped": dc.layer_op(c, dc.blind_border(c, x, "col"), res, f32),
             "last row tap dropped": dc.layer_op(c, dc.blind_border(c, x, "row"), res, f32),
             "depthwise bias dropped": dc.layer_op(c, x, res, f32, dw_bias=False)}
    if c["s"] == 2 and not c["odd_in"]:
        other = c["k"] // 2 if c["pad"] == "tf" else (c["k"] - 2) // 2
        wrong["the other padding rule (leading pad %d for %d)" % (other, lead)] = dc.layer_op(c, x, res, f32, lead=other)
    if c["op"] == "conv":
        if c["cin"] % 16:
            wrong["channel tail read as zero"] = dc.layer_op(c, x, res, f32, keep_channels=c["cin"] - c["cin"] % 16)
        if c["cin"] > 16:
            wrong["last k-block left out of the sum"] = dc.layer_op(c, x, res, f32, keep_channels=(c["cin"] - 1) // 16 * 16)
    if res is not None and c["act"] != dc.ACT_NONE:
        wrong["residual before the activation"] = dc.layer_op(c, x, res, f32, res_first=True)
    if _reaches_the_clamp(tag):
        wrong["ReLU6 without its upper clamp"] = dc.layer_op(c, x, res, f32, clamp6=False)
    print(tag, "max|f64| %.3f yardstick %.3e bar %.3e" % (r["max_f64"], r["err32"], bar_))
    for what, y in wrong.items():
        e = err(y)
        print(tag, what, "%.3e = %.0f bars" % (e, e / bar_))
        assert e >= 10 * bar_, (what, e, bar_)


@pytest.mark.parametrize("tag", dc.TAGS)
def test_case_program_passes_the_host_side_validation(tag):
    """yl_create validates on the host before any device call: a case's one-layer program (and its two-launch twin where
    yl_conv_dws_kernel is among the forms) gets past it -- on a machine without a device the answer is the HIP error behind it"""
    from _create_cases import create
    from yololite_amd import _lib
    from yololite_amd.model import model_desc
    c = dc.BY_TAG[tag]
    twins = [False] + ([True] if c["op"] == "conv" and any(f[4][0] == dc.DWS for f in dc.forms(c)) else [])
    for two in twins:
        p = dc.program(c, two)
        d, keep = model_desc(p.img_size, p.num_classes, p.level_size, p.level_anchors, p, 0)
        st, msg, h = create(_lib.load(), d)
        if h:
            _lib.load().yl_destroy(h)
        assert st in (_lib.YL_OK, -2), (two, st, msg)     # YL_ERR_HIP: no device


def _sweep():
    """every (kernel name) the query names over a swept range of layer shapes, batches and option settings: the instantiation
    lists as the library itself reports them (csrc: dwt_kernels, dwt_splitk_kernels, YL_DWK_SHAPES, YL_DWL_SHAPES, YL_DWS_SHAPES,
    yl_dwh_kernels, dwc_kernels, yl_mfma_kernels' depthwise modes, yl_dw_tile_kernel) for layers yl_create accepts"""
    seen = set()
    cins = (16, 64, 96, 160, 192, 256, 304, 512, 608)
    couts = (16, 32, 48, 64, 96, 112, 128, 144, 208, 224, 256, 320, 336, 352, 384, 50)
    for k in (3, 5, 7):
        for s in (1, 2):
            for G, B in ((4, 1), (8, 1), (7, 1), (20, 1), (8, 768)):
                for cin in cins:
                    kb = -(-cin // 16)
                    for cout in couts:
                        for _, tile_m, dev, split_k in dc.CANDIDATES:
                            q = dc.query(dc.OP_CONV, cin, cout, k, s, k // 2, k // 2, s * G, G, B, dc.ACT_RELU, False, tile_m, dc.DEV_BASE | dev, split_k)
                            if q[0]:
                                seen.add(dc.kernel_name(q, kb).replace(" stream", "").replace(" resident", ""))
            for dev in (0, 1):
                q = dc.query(dc.OP_DW, 64, 64, k, s, k // 2, k // 2, s * 8, 8, 1, dc.ACT_RELU, False, 0, dc.DEV_BASE | dev, 0)
                seen.add(dc.kernel_name(q))
    return seen


def test_cases_reach_every_instantiation_the_library_names():
    """cases x forms reach every kernel instantiation that the query names anywhere in the swept range, family by family"""
    reached = {}
    for c in dc.CASES:
        fs = dc.forms(c)
        assert fs and fs[0][0] == "default", c["tag"]      # the library runs every case under its default options
        for name, _, _, _, q in fs:
            reached.setdefault(dc.kernel_name(q), []).append((c["tag"], name))
    swept = _sweep()
    by_family = {}
    for kname in swept:
        by_family.setdefault(kname.split("<")[0], set()).add(kname)
    # the sweep found every family, and as many instantiations of each as its table holds (for the tables that are dense).
    # Of dwt_kernels' 40, two cannot be selected by a layer yl_create accepts: NT 1 with the weights from L1/L2 needs KB > 36,
    # and a 5x5 layer's tap image holds 315 channels (KB <= 20)
    want = {"yl_conv_dwt_kernel": 5 * 2 * 2 * 2 - 2 + 3, "yl_conv_dwk_kernel": 4, "yl_conv_dwl_kernel": 2, "yl_conv_dws_kernel": 8,
            "yl_dw_tile_kernel": 4, "yl_dw_kernel": 1}
    for fam, n in want.items():
        assert len(by_family.get(fam, ())) == n, (fam, sorted(by_family.get(fam, ())))
    for fam in ("yl_conv_dwh_kernel", "yl_conv_dwc_kernel", "yl_conv_mfma_kernel"):
        assert by_family.get(fam), fam
    missing = sorted(swept - set(reached))
    assert not missing, missing


# images per launch: B = 1 and the benchmark's own batch (bench.py: 64 for the edge models, 32 for the others)
def _zoo_batches(name):
    return (1, 64 if name.startswith("edge") else 32)


def test_cases_reach_every_depthwise_launch_class_of_the_zoo():
    """Every class (kernel, KB kind, channel tail, partial last n-tile, grid, stride, padding rule, the two activations,
    residual -- one tuple) that a depthwise -> 1x1 layer (dw_k > 0, no expansion in front: c2 == 0) or a stand-alone depthwise
    layer of a MODEL_ZOO program reaches under the default options -- 320 and 640 px, B = 1 and the benchmark's batch -- is the
    default-form class of some case.  A stand-alone depthwise layer that feeds a squeeze-excite gate runs the pooling variant
    of its kernel, which the gate's own float64 test covers: not counted here."""
    from yololite_amd import _lib
    from yololite_amd.program import MODEL_ZOO, SynthStateDict, build_program, zoo_meta

    class Shapes(SynthStateDict):
        """the census reads shapes only: no random weights (BatchNorm variances 1, everything else 0)"""
        def make(self, key, shape):
            if key not in self:
                self[key] = (np.ones if key.endswith("running_var") else np.zeros)(shape, np.float32)

    have = dc.case_classes()
    missing = {}
    nlayers = 0
    for name in MODEL_ZOO:
        for S in (320, 640):
            prog = build_program(zoo_meta(name, 80, S), Shapes(1, 80, 0.5))
            for i, L in enumerate(prog.layers):
                alone = L.op == _lib.OP_DW
                if not (alone or (L.op == _lib.OP_CONV and L.dw_k > 0 and L.c2 == 0)):
                    continue
                if alone and i + 1 < len(prog.layers) and prog.layers[i + 1].op == _lib.OP_SE and prog.layers[i + 1].in_slot == L.out_slot:
                    continue
                ih, iw, _ = prog.slots[L.in_slot]
                oh, ow = (prog.level_size[L.head_level],) * 2 if L.head_level >= 0 else prog.slots[L.out_slot][:2]
                assert ih == iw and oh == ow
                k, s, pt, pl, dw_act = (L.k, L.stride, L.pad_t, L.pad_l, 0) if alone else (L.dw_k, L.dw_stride, L.dw_pad_t, L.dw_pad_l, L.dw_act)
                assert pt == pl
                nlayers += 1
                for B in _zoo_batches(name):
                    q = dc.query(L.op, L.cin, L.cout, k, s, pt, pl, ih, oh, B, L.act, L.res_slot >= 0)
                    assert q[0], (name, S, L.name)
                    cl = dc.klass(q, L.op, L.cin, L.cout, k, s, pt, oh, ow, dw_act, L.act, L.res_slot >= 0)
                    if cl not in have:
                        missing.setdefault(cl, "%s %d %s %d->%d k%d s%d @%d B=%d" % (name, S, L.name, L.cin, L.cout, k, s, oh, B))
    assert nlayers > 300, nlayers
    assert not missing, "%d classes\n" % len(missing) + "\n".join("%s: %s" % (k, v) for k, v in sorted(missing.items(), key=str))


def test_query_refuses_or_falls_through_where_a_kernel_refuses():
    """what each kernel refuses goes to the fall-through family, or to 0 where nothing runs the layer"""
    def q(cin, cout, k=3, s=1, G=8, B=1, tile_m=0, dev=0, split_k=0, res=False, act=dc.ACT_RELU, op=dc.OP_CONV, lead=None):
        return dc.query(op, cin, cout, k, s, k // 2 if lead is None else lead, k // 2 if lead is None else lead, s * G, G, B, act, res,
                        tile_m, dc.DEV_BASE | dev, split_k)[0]
    assert q(96, 96) == dc.DWT
    assert q(96, 50) == dc.MFMA                           # N % 4 != 0: dwt and dwh refuse
    assert q(96, 112) == dc.DWH                           # 7 n-tiles: dwt refuses, KB < 12: dws refuses
    assert q(96, 96, G=7) == dc.MFMA                      # a grid that is no multiple of 4: dwt, dwh
    assert q(96, 96, G=8, tile_m=7, dev=1 << 3) == dc.DWC and q(96, 96, G=7, tile_m=7, dev=1 << 3) == dc.MFMA
    assert q(304, 64, tile_m=7, dev=1 << 3) == dc.DWH     # KB 19 > kbmax_of(1): dwc refuses
    assert q(192, 336) == dc.DWK and q(176, 336) == dc.DWH        # KB 12 | 11: dwk and dws refuse
    assert q(192, 338) == dc.MFMA                         # N % 4 != 0: dwk and dws refuse
    assert q(192, 336, G=6) == dc.DWK and q(192, 336, G=6, dev=2 << 5) == dc.MFMA   # dws: a grid that is no multiple of 4
    assert q(192, 336, k=5) == dc.DWS and q(192, 336, k=5, G=6) == dc.MFMA
    assert q(192, 368) == dc.DWH                          # 23 n-tiles: no multiple of 7 or 8, beyond dws's 22
    assert q(192, 64, G=4, split_k=1) == dc.DWT_SPLITK and q(192, 64, G=24, split_k=1) == dc.DWT   # beyond 20 x 20
    assert q(192, 64, k=5, s=2, G=4, split_k=1) == dc.DWT          # no split-K instantiation for 5x5 stride 2
    # what yl_create refuses, and what no kernel runs
    assert q(98, 96) == 0                                 # c_in % 4
    assert q(96, 50, res=True) == 0 and q(96, 50, act=dc.ACT_SILU) == 0           # residual / SiLU epilogue: c_out % 4
    assert q(96, 96, lead=3) == 0                         # pad >= k
    assert q(512, 64, k=5) == 0                           # 26 x 512 floats of taps: beyond 32 KiB and not a dws shape
    assert q(320, 112, k=5, G=4) == dc.DWS               # ... unless it is one
    assert q(64, 64, op=dc.OP_DW) == dc.DW_TILE and q(64, 64, op=dc.OP_DW, dev=1) == dc.DW and q(64, 32, op=dc.OP_DW) == 0
    assert q(64, 64, k=7, op=dc.OP_DW) == dc.DW
