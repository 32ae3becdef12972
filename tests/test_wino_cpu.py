"""The Winograd layer tests' own instruments, held on the CPU (tests/_wino_cases.py): the restatement of F(2x2,3x3) is the
convolution, the bar is one an honest fp32 kernel can meet and a wrong one cannot, and the cases reach every instantiation
and every launch class the MODEL_ZOO models reach.  No device: the kernel forms come from yl_query_wino_form (host code)."""
import numpy as np
import pytest

import _wino_cases as wc

_CACHE = {}
HOST_IMAGES = 4


def _case_data(tag):
    """(x as the conv sees it, w, b, res, float64 reference, Winograd yardstick row) of a case on its host inputs; computed once.
    At most HOST_IMAGES images of a case: what is held here is the arithmetic of the yardsticks on the case's channels, grid,
    activation and residual, which no image beyond the first few adds to (the batch decides the kernel form, and the device
    tests run all of it)."""
    if tag not in _CACHE:
        c = wc.BY_TAG[tag]
        xs, res = wc.host_inputs(c)
        xs, res = xs[:HOST_IMAGES], (None if res is None else res[:HOST_IMAGES])
        w, b = wc.weights(c)
        x = wc.upsample(xs, c["shift"])
        ref = wc.reference(x, w, b, c["act"], res)
        yard = wc.yard_wino(x, w, b, c["act"], res)
        _CACHE.clear()                                   # one case's tensors at a time (the (4,3) cases are large)
        _CACHE[tag] = (xs, x, w, b, res, ref, wc.row(ref, yard))
    return _CACHE[tag]


@pytest.mark.parametrize("tag", wc.TAGS)
def test_winograd_restatement_is_the_convolution_and_the_bar_tells_right_from_wrong(tag):
    """In float64 the restatement equals torch's float64 conv2d to 1e-12.  In fp32, the worst summation order a kernel could
    use (one channel at a time) stays within the bar; each single mistake a kernel could make exceeds it at least tenfold."""
    c = wc.BY_TAG[tag]
    xs, x, w, b, res, ref, r = _case_data(tag)
    act = c["act"]
    assert np.abs(wc.yard_wino(x, w, b, act, res, dt=np.float64) - ref).max() < 1e-12
    bar_ = r["bar"]

    def err(y):
        return float(np.abs(y.astype(np.float64) - ref).max())

    seq = err(wc.yard_wino(x, w, b, act, res, blk=1))
    print(tag, "max|f64| %.3f yardstick %.3e bar %.3e one-channel-at-a-time %.3e (%.2f of the bar)" % (r["max_f64"], r["err32"], bar_, seq, seq / bar_))
    assert seq <= bar_, (seq, bar_)
    wrong = {"last input channel dropped": wc.yard_wino(x[..., :-1], w[:, :-1], b, act, res),
             "right border column from the neighbour": wc.yard_wino(x, w, b, act, res, right_from_neighbour=True),
             "taps transposed": wc.yard_wino(x, np.ascontiguousarray(w.transpose(0, 1, 3, 2)), b, act, res)}
    if res is not None and act != wc.ACT_NONE:
        y = wc.wino_conv(x, w, np.float32)
        wrong["residual before the activation"] = wc.epilogue(y, b, act, res, np.float32, res_first=True)
    if c["shift"]:
        wrong["upsampled source index rounded up"] = wc.yard_wino(wc.upsample(xs, c["shift"], round_up=True), w, b, act, res)
    for what, y in wrong.items():
        e = err(y)
        print(tag, what, "%.3e = %.0f bars" % (e, e / bar_))
        assert e >= 10 * bar_, (what, e, bar_)


def test_cases_reach_every_winograd_instantiation():
    """cases x forms: both yl_conv_wino_kernel and all ten yl_conv_wino2_kernel instantiations, by the library's own answer"""
    seen = {}
    for c in wc.CASES:
        for form, dev in wc.FORMS:
            q = wc.query_case(c, dev)
            assert q[0] in (1, 2), (c["tag"], form, q)
            seen.setdefault(wc.kernel_name(q, c["shift"]), []).append((c["tag"], form))
    missing = [k for k in wc.ALL_KERNELS if k not in seen]
    assert not missing, missing
    assert set(seen) == set(wc.ALL_KERNELS), sorted(set(seen) - set(wc.ALL_KERNELS))
    # what each case is for
    auto = {c["tag"]: wc.query_case(c, 0) for c in wc.CASES}
    assert auto["k1"] == (1, 0, 0) and auto["sparse"] == (1, 0, 0) and auto["up_b"] == (1, 0, 0)
    assert auto["k2tail"] == (2, 2, 3) and auto["k3odd"] == (2, 2, 4) and auto["up_a"] == (2, 2, 4) and auto["up_c"] == (2, 2, 3)
    assert auto["big43"] == (2, 4, 3) and auto["big43up"] == (2, 4, 3)
    assert wc.query_case(wc.BY_TAG["k5wrap"], 2 << wc.SHAPE_SHIFT) == (2, 2, 7)
    assert wc.query_case(wc.BY_TAG["k2tail"], 1 << wc.SHAPE_SHIFT) == (2, 4, 4)
    assert wc.query_case(wc.BY_TAG["k8"], wc.DEV_WINO_V1) == (1, 0, 0)


def test_query_refuses_what_carries_no_winograd_image():
    assert wc.query(12, 64, 16, 1, 0, 0)[0] == 0          # cin < 16
    assert wc.query(64, 66, 16, 1, 0, 0)[0] == 0          # cout % 4
    assert wc.query(64, 64, 16, 1, 2, 0)[0] == 0          # in_shift > 1
    assert wc.query(512, 512, 160, 64, 0, 0)[0] == 0      # beyond 32-bit byte offsets
    from yololite_amd import _lib
    assert _lib.load().yl_query_wino_form(64, 64, 16, 16, 1, 0, 0, None, None) == 2   # mt / nt may be NULL


# images per launch: B = 1, the benchmark's batches (bench.py: 64 by default, 32 for the committed yololite_m / edge_m runs)
# and the chunks the executor's two streams cut them into
ZOO_BATCHES = (1, 16, 32, 64)


def test_cases_reach_every_winograd_launch_class_of_the_zoo():
    """Every class (instantiation, KB kind, channel tail, partial last n-tile, grid parity, m-tile fill, activation, residual --
    one tuple) that a Winograd-eligible layer of a MODEL_ZOO model reaches -- 320 and 640, with and without the mask branch,
    at the batches above -- is the class of some case."""
    import bench
    from yololite_amd.program import MODEL_ZOO, SynthStateDict, build_program, zoo_meta

    class Shapes(SynthStateDict):
        """the census reads shapes only: no random weights (BatchNorm variances 1, everything else 0)"""
        def make(self, key, shape):
            if key not in self:
                self[key] = (np.ones if key.endswith("running_var") else np.zeros)(shape, np.float32)

    have = wc.case_classes()
    missing = {}
    nlayers = 0
    for name in MODEL_ZOO:
        for S in (320, 640):
            for seg in (False, True):
                meta = zoo_meta(name, 80, S, **({"seg": True} if seg else {}))
                prog = build_program(meta, Shapes(1, 80, 0.5))
                for i in sorted(bench.wino_layers(prog, 1)):
                    L = prog.layers[i]
                    oh, ow, _ = prog.slots[L.out_slot]
                    assert oh == ow
                    nlayers += 1
                    for B in ZOO_BATCHES:
                        k = wc.kernel_name(wc.query(L.cin, L.cout, oh, B, L.in_shift, 0), L.in_shift)
                        assert k is not None, (name, S, L.name)
                        cl = wc.klass(k, L.cin, L.cout, oh, L.act, L.res_slot >= 0)
                        if cl not in have:
                            missing.setdefault(cl, "%s %d%s %s %d->%d @%d B=%d" % (name, S, " seg" if seg else "", L.name, L.cin, L.cout, oh, B))
    assert nlayers > 100, nlayers
    assert not missing, "\n".join("%s: %s" % (k, v) for k, v in sorted(missing.items(), key=str))
