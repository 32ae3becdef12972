"""The trainable backbone in precision "fp16" / "bf16" on the device: stemops.ConvStack and stageops.UIBStack against
tests/golden/backbone_amp.npz (the oracle modules with rounded-operand dense convolutions, _backbone_amp_cases.py), the
mode of a held forward, launch counts, the whole tiny backbone, and the refusals of yl_amp_*_set.  The worst error / bar
of every (case, mode, precision) goes to profiles/backbone_amp_parity.json under "module"."""
import ctypes as C

import numpy as np
import pytest
import torch

from yololite_amd import _lib
from _backbone_amp_cases import AMP_FIXTURE, PRECISIONS, amp_cases, amp_fixture_tensors, amp_kind, amp_mod, amp_modes, record
from _stage_cases import CASES as STAGE_CASES
from _stem_cases import CASES as STEM_CASES, TINY, tiny_inputs
from _stage_dev import run as stage_run, stack_of as stage_of
from _stem_dev import ratios, run as stem_run, run_tiny, stack_of as stem_of, tiny_backbone
from _train_dev import DEV, same

pytestmark = pytest.mark.gpu

YL_ERR_INVALID = -1                                        # include/yololite_hip.h, yl_status
BY_NAME = {c["name"]: c for c in STEM_CASES + STAGE_CASES}


def module_of(case, inputs, train, precision):
    m = (stem_of if amp_kind(case) == "stem" else stage_of)(case, inputs, train)
    m.precision = precision
    return m


def run(m, case, inputs):
    return stem_run(m, case, inputs) if amp_kind(case) == "stem" else stage_run(m, inputs)


@pytest.mark.parametrize("case,precision", amp_cases(), ids=[f"{c['name']}-{p}" for c, p in amp_cases()])
def test_fixture_parity(case, precision):
    z = np.load(AMP_FIXTURE)
    inputs = amp_mod(case).case_inputs(case)
    bad = []
    for mode in amp_modes(case):
        got = run(module_of(case, inputs, mode == "train", precision), case, inputs)
        rs = ratios(got, amp_fixture_tensors(z, case, mode, precision), (case["name"], mode, precision))
        worst = (0.0, "")
        for n, (err, b) in rs.items():
            print(f"{case['name']:8s} {mode:5s} {precision} {n:45s} err {err:.3e}  bar {b:.3e}  ratio {err / b if b else 0:.3f}")
            if b > 0:
                worst = max(worst, (round(err / b, 4), n))
            if not err <= b:
                bad.append((mode, n, err, b))
        record("module", f"{case['name']}/{mode}/{precision}", {"worst_ratio": worst[0], "at": worst[1]})
    assert not bad, bad


@pytest.mark.parametrize("name", ("s2even", "k3res"))
def test_a_backward_runs_in_the_precision_of_its_forward(name):
    """forward in fp16, then precision = "fp32", then backward: every gradient equals, bit for bit, that of a run left in
    fp16 (and not that of an fp32 run); yl_amp_*_get reports both modes"""
    case = BY_NAME[name]
    inputs = amp_mod(case).case_inputs(case)
    stay = run(module_of(case, inputs, True, "fp16"), case, inputs)
    plain = run(module_of(case, inputs, True, "fp32"), case, inputs)
    m = module_of(case, inputs, True, "fp16")
    assert m.amp_state() == {"precision": "fp32", "held": None}          # no handle yet: nothing was set
    x = torch.from_numpy(inputs["x"]).to(DEV).requires_grad_(True)
    y = m(x)
    assert m.amp_state() == {"precision": "fp16", "held": "fp16"}
    m.precision = "fp32"                                   # host side; the handle learns it in front of the next forward
    m._handle.amp_set("fp32")                              # and even told now, the held forward keeps its own mode
    assert m.amp_state() == {"precision": "fp32", "held": "fp16"}
    y.backward(torch.from_numpy(inputs["gy"]).to(DEV))
    got = {"y": y.detach().cpu(), "dx": x.grad.contiguous().cpu()}
    for n, q in m.named_parameters():
        got["g." + n] = q.grad.cpu()
    differs = False
    for n, v in got.items():
        assert torch.equal(v, stay[n]), n
        differs |= not torch.equal(v, plain[n])
    assert differs
    with torch.no_grad():                                  # the next forward is fp32: the plain run's y (eval statistics aside)
        m.eval()
        ref = module_of(case, inputs, False, "fp32")
        ref.load_state_dict(m.state_dict())
        assert torch.equal(m(x.detach()), ref(x.detach()))
    assert m.amp_state()["precision"] == "fp32"


@pytest.mark.parametrize("name", ("stem_to_c3", "a5k5s2"))
def test_launch_counts_are_equal_in_all_three_modes(name):
    case = BY_NAME[name]
    inputs = amp_mod(case).case_inputs(case)
    counts = []
    for precision in ("fp32", "fp16", "bf16"):
        m = module_of(case, inputs, True, precision)
        run(m, case, inputs)
        counts.append(m.last_launches)
    assert counts[0] == counts[1] == counts[2] and counts[0]["forward"] > 0 and counts[0]["backward"] > 0, counts


def test_the_whole_tiny_backbone_runs_in_each_precision():
    """wiring, not parity: through seventeen ReLUs the flip allowance cannot be predicted, and the short cases carry it"""
    inputs = tiny_inputs()
    assert TINY["B"] == 2 and TINY["S"] == 64
    base = run_tiny(tiny_backbone(inputs), inputs)
    for precision in PRECISIONS:
        m = tiny_backbone(inputs)
        m.precision = precision
        got = run_tiny(m, inputs)
        assert set(got) == set(base)
        for n, v in got.items():
            assert torch.isfinite(v.float()).all(), (precision, n)
        assert not torch.equal(got["y.c3"], base["y.c3"]), precision
        for part in (m.stem, m.mid, m.tail):
            assert part.amp_state() == {"precision": precision, "held": precision}
        again = tiny_backbone(inputs)
        again.precision = precision
        same(got, run_tiny(again, inputs))                 # equal inputs, equal bits


def test_the_setters_refuse_what_is_not_a_mode_and_a_held_forward_stays_held():
    for name in ("s2even", "k3res"):
        case = BY_NAME[name]
        inputs = amp_mod(case).case_inputs(case)
        m = module_of(case, inputs, True, "bf16")
        x = torch.from_numpy(inputs["x"]).to(DEV).requires_grad_(True)
        y = m(x)
        hd = m._handle
        setter = getattr(hd.lib, f"yl_amp_{hd.prefix[3:]}_set")
        for mode in (_lib.YL_HEAD_F16 | _lib.YL_HEAD_BF16, 0x400, 1, _lib.YL_HEAD_TRAIN):
            assert setter(hd.handle, mode) == YL_ERR_INVALID, (name, mode)
        assert m.amp_state() == {"precision": "bf16", "held": "bf16"} and m.held()["forward_held"] == 1
        mode, held = C.c_uint32(), C.c_uint32()
        getattr(hd.lib, f"yl_amp_{hd.prefix[3:]}_get")(hd.handle, C.byref(mode), C.byref(held))
        assert (mode.value, held.value) == (_lib.YL_HEAD_BF16, _lib.YL_HEAD_BF16)
        y.backward(torch.from_numpy(inputs["gy"]).to(DEV))  # and its backward still runs
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
