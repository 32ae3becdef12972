"""The depthwise k x k -> 1x1 kernels (yl_conv_dwk / dwl / dws / dwt (+ split-K) / dwc / dwh_kernel, the depthwise-prologue
modes of yl_conv_mfma_kernel) and the stand-alone depthwise kernels (yl_dw_tile_kernel, yl_dw_kernel) held PER LAYER to a
float64 reference at their edges: tests/_dw_cases.py has the cases, the one-layer programs, the reference, the fp32 yardstick
and the bar; tests/test_dw_layer_cpu.py holds those instruments themselves.  Every case runs under every form (a tile_m /
dev_select / split_k setting) for which the library names another kernel, and what ran is the library's own answer
(yl_query_dw_form).  The reference is computed from the layer's input as the device holds it (read back with read_slot), so
nothing in front of the layer enters the comparison.

The contexts run with streams 1, graph 0, reuse_slots 0 and fuse_head 0 (the expand-only form of the fused pair launch would
take a wide depthwise 3x3 layer away from the kernels named here); dev_select always carries the bits that keep the layer's
neighbours plain launches.

With YOLOLITE_DW_FIGURES=<path> the figures of every case that runs are merged into that JSON file
(profiles/dw_layer_parity.json is such a run)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _dw_cases as dc
from test_gpu_parity import DEV, _x

_RUN = {}
_WATCHED = ("dev_select", "tile_m", "split_k", "fuse_head", "streams", "graph", "reuse_slots")


class _Layer:
    """the one-layer program of a case on the device: forward, then the layer's input / residual / output read back"""

    def __init__(self, case, two_launches=False):
        from yololite_amd.model import HipContext
        self.case, self.p = case, dc.program(case, two_launches)
        self.ctx = HipContext(self.p.img_size, self.p.num_classes, self.p.level_size, self.p.level_anchors, self.p, 0)
        self.defaults = {k: self.ctx.get_option(k) for k in _WATCHED}
        for k, v in (("streams", 1), ("graph", 0), ("reuse_slots", 0), ("fuse_head", 0)):
            self.ctx.set_option(k, v)
        self.x = _x(case["B"], self.p.img_size, seed=300 + dc.TAGS.index(case["tag"])).to(DEV)

    def run(self, x=None, tile_m=0, dev=0, split_k=0, slots=(2,)):
        """forward under the given options -> the requested slots as numpy (1 input, 2 output, 3 residual)"""
        x = self.x if x is None else x
        ctx = self.ctx
        ctx.set_option("dev_select", dc.DEV_BASE | dev)
        ctx.set_option("tile_m", tile_m)
        ctx.set_option("split_k", split_k)
        try:
            levels = ctx.forward(x)
            G, E = self.case["G"], self.case["cout"]       # (a head-output case: its output is the level tensor [B, 1, G, G, E])
            out = [levels[0].reshape(x.shape[0], G, G, E).cpu().numpy() if (s == 2 and dc.is_head(self.case)) else
                   ctx.read_slot(s, x.shape[0], self.p.slots[s]).cpu().numpy() for s in slots]
            torch.cuda.synchronize()
        finally:
            for k in ("dev_select", "tile_m", "split_k"):
                ctx.set_option(k, self.defaults[k])
        return out if len(out) > 1 else out[0]

    def close(self):
        """the options back where the library had them; True when they are"""
        for k in _WATCHED:
            self.ctx.set_option(k, self.defaults[k])
        return {k: self.ctx.get_option(k) for k in _WATCHED} == self.defaults


def _layer(tag):
    """one live context at a time (the default-dispatch cases of the window kernel hold large tensors)"""
    if tag not in _RUN:
        _RUN.clear()
        _RUN[tag] = _Layer(dc.BY_TAG[tag])
    return _RUN[tag]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


_WHAT = ("per case: max |f64| of the layer output, the fp32 yardstick's max-abs error against float64 (err32), the bar "
         "(max(4 x err32, 2 fp32 ulps at max |f64|)) and, per form (the tile_m / dev_select / split_k setting named in "
         "tests/_dw_cases.py CANDIDATES; `two_launches`: the layer as YL_OP_DW + plain 1x1), the kernel yl_query_dw_form names, "
         "the device's max-abs error and error / bar")


def _dump(tag, record):
    """the case's figures into the file YOLOLITE_DW_FIGURES names; the other cases the file holds stay as they are"""
    path = os.environ.get("YOLOLITE_DW_FIGURES")
    if not path:
        return
    cases = {}
    if os.path.exists(path):
        with open(path) as f:
            cases = json.load(f).get("cases", {})
    cases[tag] = record
    with open(path, "w") as f:
        json.dump({"what": _WHAT, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.mark.parametrize("tag", dc.TAGS)
def test_depthwise_layer_matches_float64_under_every_form(tag):
    """Parity: under every form the output is finite and within the bar of the float64 reference; the input read back is signed
    and finite.  Forms whose kernels are documented as bit-identical (dwk = dwl; dwt = dwh = dwc) are bitwise equal; a layer that
    yl_conv_dws_kernel runs under some form is bitwise the two launches (YL_OP_DW, then the plain 1x1 conv), which are held to
    the bar as well.  The split-K form sums in another order and the generic kernel's modes are documented against no other
    kernel: the bar only.  The options are back at their defaults afterwards."""
    c = dc.BY_TAG[tag]
    L = _layer(tag)
    forms = dc.forms(c)
    assert forms and forms[0][0] == "default"
    slots = (1, 2, 3) if c["res"] else (1, 2)
    got = {}
    for i, (name, tile_m, dev, split_k, _) in enumerate(forms):
        if i == 0:
            first = L.run(tile_m=tile_m, dev=dev, split_k=split_k, slots=slots)
            xs, got[name] = first[0], first[1]
            res = first[2] if c["res"] else None
        else:
            got[name] = L.run(tile_m=tile_m, dev=dev, split_k=split_k)
    assert L.close()
    kernels = {name: q for name, _, _, _, q in forms}
    if c["op"] == "conv" and any(q[0] == dc.DWS for q in kernels.values()):
        T = _Layer(c, two_launches=True)
        got["two_launches"] = T.run()
        assert T.close()
        del T
    assert np.isfinite(xs).all() and (xs < 0).any() and (xs > 0).any()          # signed inputs
    ref = dc.reference(c, xs, res)
    y = dc.row(ref, dc.yardstick(c, xs, res))
    kb = -(-c["cin"] // 16)
    fig = {}
    for name, out in got.items():
        e = float(np.abs(out.astype(np.float64) - ref).max())
        fig[name] = {"kernel": dc.kernel_name(kernels[name], kb) if name in kernels else "yl_dw_tile_kernel / yl_dw_kernel + 1x1",
                     "device_error": e, "ratio": e / y["bar"]}
        print(tag, name, fig[name]["kernel"], "max|f64| %.3f yardstick %.3e device %.3e bar %.3e ratio %.3f" % (
            y["max_f64"], y["err32"], e, y["bar"], fig[name]["ratio"]))
    _dump(tag, dict(y, forms=fig))
    for name, out in got.items():
        assert np.isfinite(out).all(), name
        assert fig[name]["ratio"] <= 1.0, (name, fig[name], y)
    for group in dc.BITWISE_GROUPS:
        names = [n for n, q in kernels.items() if q[0] in group]
        for n in names[1:]:
            assert _same(got[n], got[names[0]]), (names[0], n, float(np.abs(got[n] - got[names[0]]).max()))
    if "two_launches" in got:
        for n, q in kernels.items():
            if q[0] == dc.DWS:
                assert _same(got[n], got["two_launches"]), (n, float(np.abs(got[n] - got["two_launches"]).max()))


# cases whose work items straddle images: three one-tile images to a workgroup's four waves (dwt, dwh, dwc; split-K: a workgroup
# per tile), 64-pixel m-tiles / items across 25-, 49- and 144-pixel images (mfma, dwk), two windows of an item from two images
# (dwl), 2 x 4-pixel blocks of a wave's four from two images (dw_tile)
BATCH_CASES = ["t_nt1", "t_nt2_n20", "t_nt3_nowl", "sk_k12", "sk_s2_k18", "m_odd5", "m_odd7_n50", "k_16_b3", "k_24_odd7", "d_3_1_g1",
               "d_5_1_g5"]


def _default_and_forced(c):
    """the default form and every form of another FAMILY (one each)"""
    out, fams = [], set()
    for f in dc.forms(c):
        if f[4][0] not in fams:
            fams.add(f[4][0])
            out.append(f)
    return out


@pytest.mark.parametrize("tag", BATCH_CASES)
def test_depthwise_layer_is_batch_invariant(tag):
    """Image b run alone is bitwise image b inside the batch, under the default form and under the forced forms of every other
    family the case reaches (the split-K form included: its choice depends on the layer's shape only)."""
    c = dc.BY_TAG[tag]
    assert c["B"] >= 2
    L = _layer(tag)
    forms = _default_and_forced(c)                       # (the odd-grid cases have the generic kernel's mode only)
    assert len(forms) >= (1 if tag.startswith("m_") else 2), forms
    for name, tile_m, dev, split_k, q in forms:
        assert dc.query_case(c, tile_m, dev, split_k, B=1) == q, name     # the same kernel runs the single image
        full = L.run(tile_m=tile_m, dev=dev, split_k=split_k)
        for i in range(c["B"]):
            one = L.run(x=L.x[i:i + 1].contiguous(), tile_m=tile_m, dev=dev, split_k=split_k)
            assert _same(one[0], full[i]), (name, i)
    assert L.close()


# channel tails (c_in % 16 != 0; stand-alone: c_in % 256 != 0) in a batch of two or three
TAIL_CASES = ["t_nt2_n20", "t_tf5", "sk_k13_tail", "k_16_b3", "k_14_s2", "s_8_3_1", "d_5_1_g5"]


@pytest.mark.parametrize("tag", TAIL_CASES)
def test_depthwise_layer_ignores_a_non_finite_neighbour(tag):
    """Channel tails: the tail lanes of an image's last pixel would read the next image's first channels, and a zero tap or 1x1
    weight does not make 0 x NaN zero.  One image of the batch replaced by NaN in the image tensor (it reaches the layer as NaN
    or inf): the other images' layer inputs and outputs are bitwise those of the clean run, under every form."""
    c = dc.BY_TAG[tag]
    assert c["B"] >= 2 and (c["cin"] % 16 or (c["op"] == "dw" and c["cin"] % 256))
    L = _layer(tag)
    for name, tile_m, dev, split_k, _ in dc.forms(c):
        xin, clean = L.run(tile_m=tile_m, dev=dev, split_k=split_k, slots=(1, 2))
        for j in range(c["B"]):
            x = L.x.clone()
            x[j] = float("nan")
            xs, out = L.run(x=x, tile_m=tile_m, dev=dev, split_k=split_k, slots=(1, 2))
            assert not np.isfinite(xs[j]).any(), (name, j)                      # the poison does reach the layer (NaN or inf: 0 x either is NaN)
            for i in range(c["B"]):
                if i != j:
                    assert _same(xs[i], xin[i]), (name, j, i, "input")
                    assert _same(out[i], clean[i]), (name, j, i, int(np.isnan(out[i]).sum()))
    assert L.close()
