"""The Winograd F(2x2,3x3) kernels (yl_conv_wino_kernel<SH>, yl_conv_wino2_kernel<MT, NT, SH>) held PER LAYER to a float64
reference at their edges: tests/_wino_cases.py has the cases, the one-layer programs, the reference, the fp32 yardsticks and
the bar; tests/test_wino_cpu.py holds those instruments themselves.  Every case runs under every kernel form ("dev_select"),
and what ran is the library's own answer (yl_query_wino_form).  The reference is computed from the layer's input as the
device holds it (read back with read_slot), so nothing in front of the layer enters the comparison.

With YOLOLITE_WINO_FIGURES=<path> the figures of every case that runs are merged into that JSON file
(profiles/wino_layer_parity.json is such a run)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _wino_cases as wc
from test_gpu_parity import DEV, _x

_RUN = {}
_WATCHED = ("winograd", "dev_select", "tile_m", "streams", "graph", "reuse_slots")


class _Layer:
    """the one-layer program of a case on the device: forward, then the layer's input / residual / output read back"""

    def __init__(self, case):
        from yololite_amd.model import HipContext
        self.case, self.p = case, wc.program(case)
        self.ctx = HipContext(self.p.img_size, self.p.num_classes, self.p.level_size, self.p.level_anchors, self.p, 0)
        self.defaults = {k: self.ctx.get_option(k) for k in _WATCHED}
        for k, v in (("streams", 1), ("graph", 0), ("reuse_slots", 0)):
            self.ctx.set_option(k, v)
        self.x = _x(case["B"], self.p.img_size, seed=100 + wc.TAGS.index(case["tag"])).to(DEV)

    def run(self, x=None, winograd=1, dev=0, tile_m=0, slots=(2,)):
        """forward under the given options -> the requested slots as numpy (1 input, 2 output, 3 residual)"""
        x = self.x if x is None else x
        ctx = self.ctx
        ctx.set_option("winograd", winograd)
        ctx.set_option("dev_select", dev)
        ctx.set_option("tile_m", tile_m)
        try:
            ctx.forward(x)
            out = [ctx.read_slot(s, x.shape[0], self.p.slots[s]).cpu().numpy() for s in slots]
            torch.cuda.synchronize()
        finally:
            ctx.set_option("winograd", self.defaults["winograd"])
            ctx.set_option("dev_select", self.defaults["dev_select"])
            ctx.set_option("tile_m", self.defaults["tile_m"])
        return out if len(out) > 1 else out[0]

    def close(self):
        """the options back where the library had them; True when they are"""
        for k in _WATCHED:
            self.ctx.set_option(k, self.defaults[k])
        return {k: self.ctx.get_option(k) for k in _WATCHED} == self.defaults


def _layer(tag):
    """one live context at a time (the (4,3) cases hold large tensors)"""
    if tag not in _RUN:
        _RUN.clear()
        _RUN[tag] = _Layer(wc.BY_TAG[tag])
    return _RUN[tag]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


_WHAT = ("per case: max |f64| of the layer output; `winograd`: the fp32 Winograd yardstick's max-abs error against float64, the "
         "bar (max(4 x yardstick error, 2 fp32 ulps at max |f64|)), the device's worst error over the forms and error / bar, and "
         "the kernel yl_query_wino_form names per form (v1 / auto / s1 / s2 / s3 = dev_select bit 11, 0, bits 12-13 = 1, 2, 3; "
         "the forms' outputs are bitwise equal); `direct`: the same against torch's fp32 conv2d for option winograd 0 under "
         "default dispatch and under tile_m 6")


def _dump(tag, record):
    """the case's figures into the file YOLOLITE_WINO_FIGURES names; the other cases the file holds stay as they are"""
    path = os.environ.get("YOLOLITE_WINO_FIGURES")
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


@pytest.mark.parametrize("tag", wc.TAGS)
def test_winograd_layer_matches_float64_under_every_form(tag):
    """Parity: every form's output within the Winograd bar of the float64 reference.  The forms are bitwise equal to each
    other.  The direct path (option "winograd" 0) differs from them in some bit and is within the direct bar, under default
    dispatch and under tile_m 6 (the generic kernel).  The options are back at their defaults afterwards."""
    c = wc.BY_TAG[tag]
    L = _layer(tag)
    slots = (1, 2, 3) if c["res"] else (1, 2)
    got = {}
    first = L.run(dev=wc.FORMS[0][1], slots=slots)
    xs, got[wc.FORMS[0][0]] = first[0], first[1]
    res = first[2] if c["res"] else None
    for form, dev in wc.FORMS[1:]:
        got[form] = L.run(dev=dev)
    direct = {"direct": L.run(winograd=0), "direct_tile6": L.run(winograd=0, tile_m=6)}
    assert L.close()
    assert np.isfinite(xs).all() and (xs < 0).any() and (xs > 0).any()          # signed inputs
    w, b = wc.weights(c)
    x = wc.upsample(xs, c["shift"])
    ref = wc.reference(x, w, b, c["act"], res)
    yw = wc.row(ref, wc.yard_wino(x, w, b, c["act"], res))
    yd = wc.row(ref, wc.yard_direct(x, w, b, c["act"], res))
    fig = {}
    for form, dev in wc.FORMS:
        q = wc.query_case(c, dev)
        e = float(np.abs(got[form].astype(np.float64) - ref).max())
        fig[form] = dict(yw, kernel=wc.kernel_name(q, c["shift"]), form=q[0], mt=q[1], nt=q[2], device_error=e, ratio=e / yw["bar"])
    for k, y in direct.items():
        e = float(np.abs(y.astype(np.float64) - ref).max())
        fig[k] = dict(yd, kernel="direct", device_error=e, ratio=e / yd["bar"])
    worst = {k: max(fig[f]["device_error"] for f in fs) for k, fs in (("winograd", [f for f, _ in wc.FORMS]), ("direct", list(direct)))}
    _dump(tag, {"max_f64": yw["max_f64"],
                "winograd": {"err32": yw["err32"], "bar": yw["bar"], "device_error": worst["winograd"], "ratio": worst["winograd"] / yw["bar"],
                             "forms": {f: fig[f]["kernel"] for f, _ in wc.FORMS}},
                "direct": {"err32": yd["err32"], "bar": yd["bar"],
                           "runs": {k: {"device_error": fig[k]["device_error"], "ratio": fig[k]["ratio"]} for k in direct}}})
    for k, r in fig.items():
        print(tag, k, r["kernel"], "max|f64| %.3f yardstick %.3e device %.3e bar %.3e ratio %.3f" % (
            r["max_f64"], r["err32"], r["device_error"], r["bar"], r["ratio"]))
    for form, _ in wc.FORMS:
        assert np.isfinite(got[form]).all(), form
        assert fig[form]["ratio"] <= 1.0, (form, fig[form])
    for form, _ in wc.FORMS[1:]:
        assert _same(got[form], got["v1"]), (form, float(np.abs(got[form] - got["v1"]).max()))
    for k, y in direct.items():
        assert not _same(y, got["auto"]), k                                     # the switch selects another kernel
        assert fig[k]["ratio"] <= 1.0, (k, fig[k])


@pytest.mark.parametrize("tag", ["k1", "k2tail", "k3odd"])
def test_winograd_layer_is_batch_invariant(tag):
    """Image b run alone is bitwise image b inside the batch, under the first form and under the launcher's own choice: in
    these cases a wave's 16 tiles (first form) or an item's m-tiles (second form) straddle images."""
    c = wc.BY_TAG[tag]
    L = _layer(tag)
    for form, dev in wc.FORMS[:2]:
        full = L.run(dev=dev)
        for i in range(c["B"]):
            one = L.run(x=L.x[i:i + 1].contiguous(), dev=dev)
            assert _same(one[0], full[i]), (form, i)
    assert L.close()


@pytest.mark.parametrize("tag", ["k2tail", "k3odd", "fpn328"])
def test_winograd_layer_ignores_a_non_finite_neighbour(tag):
    """Channel tails: the tail lanes of an image's last pixel would read the next image's first channels, and U being zero
    there does not make 0 x NaN zero.  One image of the batch replaced by NaN in the image tensor (it reaches the layer as NaN
    or inf): the other images' layer inputs and outputs are bitwise those of the clean run, under every form.
    With the tail guard of yl_conv_wino2_kernel's window copies switched off in a scratch build, k2tail fails here: the last
    pixel of the image in front of the poisoned one comes out non-finite under the launcher's own form."""
    c = wc.BY_TAG[tag]
    L = _layer(tag)
    for form, dev in wc.FORMS:
        xin, clean = L.run(dev=dev, slots=(1, 2))
        for j in range(c["B"]):
            x = L.x.clone()
            x[j] = float("nan")
            xs, out = L.run(x=x, dev=dev, slots=(1, 2))
            assert not np.isfinite(xs[j]).any(), (form, j)                      # the poison does reach the layer (NaN or inf: 0 x either is NaN)
            for i in range(c["B"]):
                if i != j:
                    assert _same(xs[i], xin[i]), (form, j, i, "input")
                    assert _same(out[i], clean[i]), (form, j, i, int(np.isnan(out[i]).sum()))
    assert L.close()
