"""The precision interface of the trainable necks (yololite_amd.neckops): the argument and the property, what each value
does to the bits, the launch counts, the mode a backward runs in, the refusals, and the 20-step fit in the reduced modes."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import yololite_amd as ya
from yololite_amd import _lib, neckops
from _dense_neck_cases import CASES, E2E, case_inputs, head_inputs, level_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "dense_neck_amp_parity.json")
BY_NAME = {c["name"]: c for c in CASES}
gpu = pytest.mark.gpu


def test_precision_argument_and_property_exist_and_bad_values_raise():
    m = ya.DetectNeckMS((8, 12, 20), 16, 1)
    assert m.precision == "fp32"
    for p in ("fp16", "bf16", "fp32"):
        assert ya.DetectNeckMS((8, 12, 20), 16, 1, precision=p).precision == p
        m.precision = p
        assert m.precision == p
    for bad in ("fp8", "half", None, 16, "FP16"):
        with pytest.raises(ValueError, match="precision"):
            ya.DetectNeckMS((8, 12, 20), 16, 1, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            m.precision = bad
    assert m.precision == "fp32"                           # a refused value changes nothing


def test_the_depthwise_neck_refuses_a_reduced_precision_and_says_why():
    assert ya.DetectNeck((8, 12, 20), 16, 1).precision == "fp32"
    assert ya.DetectNeck((8, 12, 20), 16, 1, precision="fp32").precision == "fp32"
    for p in ("fp16", "bf16"):
        with pytest.raises(ya.YoloLiteHipError, match="no dense 3x3 GEMM"):
            ya.DetectNeck((8, 12, 20), 16, 1, precision=p)
    m = ya.DetectNeck((8, 12, 20), 16, 1)
    with pytest.raises(ya.YoloLiteHipError, match="DetectNeckMS"):
        m.precision = "bf16"
    with pytest.raises(ValueError, match="precision"):
        m.precision = "fp8"


def test_from_meta_from_state_dict_and_neck_for_carry_the_precision():
    from yololite_amd.program import synth_state_dict, zoo_meta
    meta = zoo_meta("yololite_n", num_classes=3, img_size=64)
    sd = synth_state_dict(meta)
    assert ya.DetectNeckMS.from_meta(meta, precision="bf16").precision == "bf16"
    assert ya.DetectNeckMS.from_state_dict(meta, sd, precision="fp16").precision == "fp16"
    assert ya.neck_for(meta, sd, precision="fp16").precision == "fp16"
    assert ya.neck_for(meta, precision="bf16").precision == "bf16"
    assert ya.neck_for(meta, sd).precision == "fp32"
    with pytest.raises(ValueError, match="precision"):
        ya.neck_for(meta, sd, precision="int8")
    cpu = zoo_meta("edge_n", num_classes=3, img_size=64)
    if (cpu.get("arch") or "").lower() == "yololitems_cpu":
        with pytest.raises(ya.YoloLiteHipError, match="no dense 3x3 GEMM"):
            ya.neck_for(cpu, precision="fp16")


# ---- on the device

def _load(m, inputs):
    sd = {}
    for lv in inputs:
        sd.update(lv["params"]); sd.update(lv["buffers"])
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return m


def _neck(case, inputs, **kw):
    from _train_dev import DEV
    m = ya.DetectNeckMS(case["Cin"], case["F"], case["depth"], level_names=level_names(case), **kw)
    return _load(m, inputs).to(DEV).train()


def _flat(outs):
    return {f"L{li}/{n}": v for li, d in enumerate(outs) for n, v in d.items()}


@gpu
@pytest.mark.parametrize("name", ["odd", "rows"])
def test_fp32_is_the_default_and_switching_back_restores_its_bits(name):
    from _dense_neck_dev import run
    from _train_dev import same
    case = BY_NAME[name]
    inputs = case_inputs(case)
    plain = _flat(run(_neck(case, inputs), inputs))
    same(plain, _flat(run(_neck(case, inputs, precision="fp32"), inputs)))
    m = _neck(case, inputs, precision="fp16")
    launches = {}
    half = _flat(run(m, inputs))
    launches["fp16"] = m.last_launches()
    assert any(not torch.equal(half[n], plain[n]) for n in plain if n.endswith(("/p", "/dc")))
    m.precision = "fp32"                                   # the same module and handle, back in fp32 ...
    _load(m, inputs)                                       # ... with the case's running statistics again (the fp16 step moved them)
    same(plain, _flat(run(m, inputs)))
    launches["fp32"] = m.last_launches()
    m3 = _neck(case, inputs, precision="bf16")
    b16 = _flat(run(m3, inputs))
    launches["bf16"] = m3.last_launches()
    assert any(not torch.equal(b16[n], half[n]) for n in plain if n.endswith("/p"))
    assert launches["fp16"] == launches["fp32"] == launches["bf16"], launches
    same(half, _flat(run(_neck(case, inputs, precision="fp16"), inputs)))      # equal inputs, equal bits


@gpu
def test_a_backward_runs_in_the_precision_of_its_forward():
    from _train_dev import DEV, same
    case = BY_NAME["odd"]
    inputs = case_inputs(case)

    def go(switch_to):
        m = _neck(case, inputs, precision="fp16")
        cs = [torch.from_numpy(lv["c"]).to(DEV).requires_grad_(True) for lv in inputs]
        ps = m(cs, layout="nhwc")
        if switch_to:
            m.precision = switch_to
        torch.autograd.backward(ps, [torch.from_numpy(lv["gp"]).to(DEV) for lv in inputs])
        out = {"g." + n: q.grad.cpu() for n, q in m.named_parameters()}
        out.update({f"dc{i}": c.grad.cpu() for i, c in enumerate(cs)})
        return out
    kept = go(None)
    same(kept, go("fp32"))
    same(kept, go("bf16"))


@gpu
def test_both_precision_bits_in_the_flags_are_refused():
    from _train_dev import DEV
    case = BY_NAME["base"]
    inputs = case_inputs(case)
    m = _neck(case, inputs)
    cs = [torch.from_numpy(lv["c"]).to(DEV) for lv in inputs]
    with torch.no_grad():
        m(cs, layout="nhwc")
    hd = m._handle
    hd.mode_bits = _lib.YL_DNECK_F16 | _lib.YL_DNECK_BF16
    ps = [p.detach() for p in m._param_list()]
    outs = [torch.empty((case["B"], S, S, case["F"]), device=DEV) for S in case["sizes"]]
    L = len(cs)
    args = (C.byref(hd.table(ps, m._stat_buffers())), neckops._ptrs(cs), case["B"], (C.c_int32 * L)(*case["sizes"]),
            _lib.YL_HEAD_TRAIN | hd.mode_bits, neckops._ptrs(outs))
    with pytest.raises(ya.YoloLiteHipError, match=r"yl_dneck_forward"):
        hd.launch("forward", torch.device(DEV), *args)
    n = C.c_int32()
    st = hd.lib.yl_dneck_conv3x3(hd.handle, 0, _lib.YL_DNECK_F16 | _lib.YL_DNECK_BF16, cs[0].data_ptr(), cs[0].data_ptr(),
                                 outs[0].data_ptr(), 1, 1, None, C.byref(n))
    assert st != _lib.YL_OK


@gpu
def test_twenty_steps_fit_one_batch_in_the_reduced_precisions():
    """E2E, 20 SGD steps of neck + heads: fp16 with a loss scale of 1024 through FusedTrainStep (unscale, found-inf skip and
    scale update on the device), bf16 unscaled.  The loss falls and every step is finite; L20 is compared with the fp32
    mode's of the same run: printed and recorded, not asserted (nobody has measured it)."""
    from _train_dev import DEV, targets
    inputs, hinputs = case_inputs(E2E), head_inputs(E2E)
    feats = [torch.from_numpy(lv["c"]).to(DEV) for lv in inputs]
    tg = targets(E2E)
    res = {}
    for precision in ("fp32", "fp16", "bf16"):
        neck = _neck(E2E, inputs, precision=precision)
        heads = ya.DetectHeads(E2E["F"], E2E["C"], E2E["A"], E2E["head_depth"])
        hsd = {}
        for lv in hinputs:
            hsd.update(lv["params"]); hsd.update(lv["buffers"])
        heads.load_state_dict({k: torch.as_tensor(v) for k, v in hsd.items()})
        heads.to(DEV).train()
        crit = ya.LossAF(E2E["C"], E2E["img_size"], grad=True)
        params = list(neck.parameters()) + list(heads.parameters())
        amp = precision == "fp16"
        kw = dict(scaler_kwargs={"init_scale": 1024.0}) if amp else {}
        fts = ya.FusedTrainStep(params, optimizer="sgd", amp=amp, lr=E2E["lr"], momentum=E2E["momentum"], nesterov=False,
                                weight_decay=0.0, **kw)
        losses = []
        for _ in range(E2E["steps"]):
            fts.zero_grad()
            loss, _ = crit(heads(neck(feats, layout="nhwc"), layout="nhwc"), tg)
            fts.scale(loss).backward()                     # loss * scale in fp16 mode, the identity otherwise
            assert torch.isfinite(loss).all()
            assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
            fts.step()
            losses.append(float(loss.detach()))
        with torch.no_grad():
            losses.append(float(crit(heads(neck(feats, layout="nhwc"), layout="nhwc"), tg)[0]))
        assert np.isfinite(losses).all()
        res[precision] = losses
        print(f"{precision}: L0 {losses[0]:.6f}  L20 {losses[-1]:.6f}")
    for precision in ("fp16", "bf16"):
        L0, L20 = res[precision][0], res[precision][-1]
        assert L20 < L0, (precision, L0, L20)
        print(f"{precision}: L20 - L20(fp32) = {L20 - res['fp32'][-1]:+.3e}")
    try:
        table = json.load(open(PARITY)) if os.path.exists(PARITY) else {}
        table["e2e"] = {p: {"L0": v[0], "L20": v[-1], "L20_minus_fp32": v[-1] - res["fp32"][-1]} for p, v in res.items()}
        with open(PARITY, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass
