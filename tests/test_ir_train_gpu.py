"""Trainable EfficientNet-Lite stages on the device (yololite_amd.irops.IRStack / EfficientNetLiteTail, the ReLU6 and
TF-SAME variant of csrc/yl_stage.hip) against the oracle's fixture, the depthwise op on its own under TF-SAME, UIBStack bit
for bit where the two coincide, and a short fit through neck, heads and loss.

Fixture parity, per case, mode and tensor: the bar is max(4 x the oracle's own fp32 error, 2 fp32 ulps at the tensor's
largest magnitude), the rule of the head tests; the worst device error / bar of each case is written to
profiles/ir_train_parity.json."""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch

import yololite_amd as ya
from yololite_amd import stageops
from _ir_cases import (CASES, WIDE, as_uib, bar, case_inputs, dw_dgrad, dw_forward, dw_wgrad, fixture_path, fixture_tensors,
                       modes, stack_all)
from _neck_cases import E2E
from _stage_cases import DW_OP_KS, DW_OP_SHAPES
from _stage_dev import run as _run
from _train_dev import DEV, same as _same, targets as _targets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "ir_train_parity.json")
BY_NAME = {c["name"]: c for c in CASES + WIDE}


def _stack(case, inputs, train=True, **kw):
    m = ya.IRStack(case["cin"], case["blocks"], prefix=case.get("prefix", ""), **kw)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in {**inputs["params"], **inputs["buffers"]}.items()})
    return m.to(DEV).train(train)


def _parity_ratios(case, mode, z):
    """{tensor: (error, bar)} of one case and mode against the fixture `z`"""
    inputs = case_inputs(case)
    got = _run(_stack(case, inputs, mode == "train"), inputs)
    want = fixture_tensors(z, case, mode)
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    out = {}
    for n, (r64, idx, e32, m64) in want.items():
        g = got[n].numpy().reshape(-1)
        if n.endswith("num_batches_tracked"):
            assert int(g[0]) == int(r64[0]), (case["name"], mode, n)
            continue
        g = g.astype(np.float64)
        out[n] = (float(np.abs((g if idx is None else g[idx]) - r64).max()), bar(e32, m64))
    return out


@pytest.mark.parametrize("case", CASES + WIDE, ids=[c["name"] for c in CASES + WIDE])
def test_fixture_parity(case):
    z = np.load(fixture_path(case))
    bad, worst = [], {}
    for mode in modes(case):
        for n, (err, b) in _parity_ratios(case, mode, z).items():
            print(f"{case['name']:14s} {mode:5s} {n:50s} err {err:.3e}  bar {b:.3e}  ratio {err / b:.3f}")
            if err / b > worst.get(mode, (0.0,))[0]:
                worst[mode] = (err / b, n)
            if not err <= b:
                bad.append((mode, n, err, b))
    try:                                                   # the figures of this run, beside the others' (best effort)
        table = json.load(open(PARITY)) if os.path.exists(PARITY) else {}
        table[case["name"]] = {m: {"worst_ratio": round(r, 4), "tensor": t} for m, (r, t) in worst.items()}
        with open(PARITY, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass
    assert not bad, bad


@pytest.mark.parametrize("name", [c["name"] for c in WIDE])
def test_sampled_tensors_agree_with_the_restatement_everywhere(name):
    """the fixture stores tensors above 8192 elements at a sample (only the wide cases have any); here every element of
    those is held to the float64 restatement (which test_ir_train_cpu.py ties to the fixture), under the fixture's bar"""
    case = BY_NAME[name]
    want = fixture_tensors(np.load(fixture_path(case)), case, "train")
    sampled = [n for n, v in want.items() if v[1] is not None]
    assert sampled                                         # every wide case has a 1x1 weight above the threshold
    inputs = case_inputs(case)
    got = _run(_stack(case, inputs), inputs)
    ref = stack_all(case, inputs, True)
    for n in sampled:
        _, _, e32, m64 = want[n]
        err = np.abs(got[n].numpy().astype(np.float64) - ref[n]).max()
        print(f"{name} {n} err {err:.3e} bar {bar(e32, m64):.3e}")
        assert err <= bar(e32, m64), (n, err, bar(e32, m64))


# ---- the depthwise op alone under TF-SAME
DW_SHAPES = [(B, S, C) for B, S, C in DW_OP_SHAPES if S % 2 == 0] + [(1, 6, 260)]
PASSES = ("forward", "dgrad", "wgrad")


@functools.lru_cache(maxsize=None)
def cell(k, s, B, S, C):
    """inputs (fp32, NHWC), the float64 restatement under TF-SAME, and the error of the oracle's own fp32 convolution
    (oracle.backbones._conv(same=True), torch autograd on the CPU) against it: computed once, shared, never written to"""
    from oracle.backbones import _conv
    rs = np.random.RandomState(1000 * k + 100 * s + 10 * S + C + B)
    So = -(-S // s)
    x = rs.standard_normal((B, S, S, C)).astype(np.float32)
    w = (rs.standard_normal((C, 1, k, k)) / k).astype(np.float32)
    dy = rs.standard_normal((B, So, So, C)).astype(np.float32)
    x64, w64, dy64 = x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64)
    r64 = {"forward": dw_forward(x64, w64, s), "dgrad": dw_dgrad(dy64, w64, s, S), "wgrad": dw_wgrad(x64, dy64, k, s)}
    conv = _conv(C, C, k, s, groups=C, same=True)
    conv.weight.data = torch.from_numpy(w)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_(True)
    y = conv(xt)
    y.backward(torch.from_numpy(dy).permute(0, 3, 1, 2))
    r32 = {"forward": y.detach().permute(0, 2, 3, 1).numpy(), "dgrad": xt.grad.permute(0, 2, 3, 1).numpy(), "wgrad": conv.weight.grad.numpy()}
    bars = {p: bar(np.abs(r32[p].astype(np.float64) - r64[p]).max(), np.abs(r64[p]).max()) for p in PASSES}
    return x, w, dy, r64, bars


def device_pass(pass_, k, s, x, w, dy, same):
    t = lambda a: torch.from_numpy(a).to(DEV)              # noqa: E731
    if pass_ == "forward":
        return stageops.depthwise(t(x), t(w), "forward", k, s, same=same)
    if pass_ == "dgrad":
        return stageops.depthwise(t(dy), t(w), "dgrad", k, s, size=x.shape[1], same=same)
    return stageops.depthwise(t(x), t(dy), "wgrad", k, s, same=same)


@pytest.mark.parametrize("pass_", PASSES)
@pytest.mark.parametrize("k,s", DW_OP_KS)
def test_the_depthwise_op_under_tf_same_against_the_float64_restatement(k, s, pass_):
    bad = []
    for B, S, C in DW_SHAPES:
        x, w, dy, r64, bars = cell(k, s, B, S, C)
        got = device_pass(pass_, k, s, x, w, dy, True).cpu().numpy()
        assert got.shape == r64[pass_].shape
        err = np.abs(got.astype(np.float64) - r64[pass_]).max()
        print(f"k{k} s{s} {pass_:7s} B{B} S{S:2d} C{C:3d}  err {err:.3e}  bar {bars[pass_]:.3e}")
        if not err <= bars[pass_]:
            bad.append((B, S, C, err, bars[pass_]))
    assert not bad, bad


@pytest.mark.parametrize("pass_", PASSES)
def test_same_and_symmetric_padding_give_equal_bits_where_they_coincide(pass_):
    """stride 1, or an odd S under stride 2: the two leading pads are equal and so are the bits; an even S under stride 2
    moves the window by one pixel and the results differ"""
    for k, s in DW_OP_KS:
        for B, S, C in DW_OP_SHAPES + [(1, 6, 260)]:
            rs = np.random.RandomState(17 * k + s + 5 * S + C + B)
            So = -(-S // s)
            x = rs.standard_normal((B, S, S, C)).astype(np.float32)
            w = rs.standard_normal((C, 1, k, k)).astype(np.float32)
            dy = rs.standard_normal((B, So, So, C)).astype(np.float32)
            a, b = device_pass(pass_, k, s, x, w, dy, True), device_pass(pass_, k, s, x, w, dy, False)
            if s == 1 or S % 2 == 1:
                assert torch.equal(a, b), (k, s, B, S, C)
            else:
                assert not torch.equal(a, b), (k, s, B, S, C)


# ---- the walk, tied to UIBStack

@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
def test_relu_and_symmetric_padding_give_uibstacks_bits(precision):
    """IRStack(act="relu", same=False) against UIBStack of the equivalent a = 0 blocks on the same weights: y, dx, every
    gradient and every buffer, bit for bit, in every precision of the 1x1 GEMMs"""
    for name in ("k3s2", "k5s2", "k3res", "ragged", "rows", "lite_tiny_tail"):
        case = BY_NAME[name]
        inputs = case_inputs(case)
        ucase, key = as_uib(case)
        uib = ya.UIBStack(case["cin"], ucase["blocks"], eps=1e-3, prefix=case.get("prefix", ""), precision=precision)
        uib.load_state_dict({key(k): torch.as_tensor(v) for k, v in {**inputs["params"], **inputs["buffers"]}.items()})
        want = _run(uib.to(DEV).train(), inputs)
        m = _stack(case, inputs, act="relu", same=False, precision=precision)
        got = _run(m, inputs)
        assert m.variant_state() == {"act": "relu", "same": False} and m.amp_state()["precision"] == precision
        assert m.last_launches == uib.last_launches
        pre = {"y": "y", "dx": "dx"}
        pre.update({n: n[:2] + key(n[2:]) for n in got if n[:2] in ("b.", "g.")})
        assert sorted(pre.values()) == sorted(want)
        for n in got:
            assert torch.equal(got[n], want[pre[n]]), (name, precision, n)
        # and the variant is not a no-op: the default IRStack differs on the same weights
        other = _run(_stack(case, inputs, precision=precision), inputs)
        assert not torch.equal(other["y"], got["y"]), name


def test_relu6_really_clamps_and_its_gradient_is_zero_at_the_clamp():
    """with bn2's gamma 0 and beta 7 EVERY value in front of the second ReLU6 exceeds 6: the block's output does not
    depend on x, and nothing passes the clamp backwards: dx and bn2's own gradients are exactly zero"""
    case = BY_NAME["k3s2"]
    inputs = case_inputs(case)
    m = _stack(case, inputs).eval()
    with torch.no_grad():
        bn2 = m.get_submodule("blocks.0.0.bn2")
        bn2.weight.zero_()
        bn2.bias.fill_(7.0)
    got = _run(m, inputs)
    assert torch.equal(got["y"], _run(m, dict(inputs, x=inputs["x"] * 2 + 1))["y"])
    assert float(got["dx"].abs().max()) == 0.0 and float(got["g.blocks.0.0.bn2.bias"].abs().max()) == 0.0
    assert float(got["g.blocks.0.0.bn3.bias"].abs().max()) > 0.0


# ---- the behaviours the stack shares with UIBStack

def test_two_runs_give_the_same_bits_in_both_input_layouts():
    for case in (BY_NAME["k3s2"], BY_NAME["rows"], BY_NAME["lite_tiny_tail"]):
        inputs = case_inputs(case)
        first = _run(_stack(case, inputs), inputs)
        for layout in ("nhwc", "nchw"):
            _same(first, _run(_stack(case, inputs), inputs, layout=layout))


def test_gradients_nobody_asked_for_are_not_computed():
    """the launch counts are those include/yololite_hip.h documents for the stage: a unit's forward is 4 launches in train
    mode and 3 in eval mode; its backward 1 (sums) + 1 (bn grads) + 1 (dz) + 2 (weight gradient) + 1 (input gradient), and
    a residual block's add is 1"""
    case = BY_NAME["k3res"]                                # conv_pw, conv_dw, conv_pwl; residual
    inputs = case_inputs(case)
    m = _stack(case, inputs)
    full = _run(m, inputs)
    assert m.last_launches == {"forward": 3 * 4, "backward": 3 * 6 + 1}
    m = _stack(case, inputs)                               # the input does not require grad: no input gradient, no add
    nodx = _run(m, inputs, x_grad=False)
    assert m.last_launches["backward"] == 3 * 6 - 1 and "dx" not in nodx
    _same({n: v for n, v in full.items() if n != "dx"}, nodx)
    case = BY_NAME["lite_tiny_tail"]                       # 5.0, 5.1 (residual), 6.0: three units each
    inputs = case_inputs(case)
    m = _stack(case, inputs)
    full = _run(m, inputs)
    assert m.last_launches == {"forward": 9 * 4, "backward": 9 * 6 + 1}
    # a frozen first block, and an input that does not require grad: nothing upstream of block 5.1 runs
    m = _stack(case, inputs)
    for n, p in m.named_parameters():
        p.requires_grad_(not n.startswith("backbone.blocks.5.0."))
    part = _run(m, inputs, x_grad=False)
    assert m.last_launches["backward"] == 6 * 6 - 1        # block 5.1's input gradient and its add are not run
    for n, p in m.named_parameters():
        assert (p.grad is None) == n.startswith("backbone.blocks.5.0."), n
    _same({n: v for n, v in full.items() if n in part}, part)
    m = _stack(case, inputs)                               # only the last BatchNorm: two launches
    for n, p in m.named_parameters():
        p.requires_grad_(n.startswith("backbone.blocks.6.0.bn3."))
    bn = _run(m, inputs, x_grad=False)
    assert m.last_launches["backward"] == 2
    _same({n: v for n, v in full.items() if n in bn}, bn)
    m.eval()                                               # eval mode, no graph: 3 launches per unit
    with torch.no_grad():
        y = m(torch.from_numpy(inputs["x"]).to(DEV), layout="nhwc")
    assert y.grad_fn is None and m.last_launches["forward"] == 9 * 3


def test_the_variant_is_refused_while_a_forward_is_held_and_deepcopy_keeps_it():
    case = BY_NAME["k3s2"]
    inputs = case_inputs(case)
    m = _stack(case, inputs)
    want = _run(_stack(case, inputs), inputs)
    x = torch.from_numpy(inputs["x"]).to(DEV).requires_grad_(True)
    y = m(x, layout="nhwc")
    assert m.held()["forward_held"] == 1 and m.variant_state() == {"act": "relu6", "same": True}
    with pytest.raises(ya.YoloLiteHipError, match="yl_variant_stage_set"):
        m._handle.variant_set("relu", False)
    assert m.variant_state() == {"act": "relu6", "same": True}
    lib = stageops._lib.load()
    for act, same in ((2, 0), (-1, 1), (0, 2), (1, -1)):   # host-side checks: YL_ERR_INVALID, nothing changes
        assert lib.yl_variant_stage_set(m._handle.handle, act, same) == -1
    twin = copy.deepcopy(m)
    assert twin._handle is not m._handle and twin._handle.handle is None and twin._handle.variant == ("relu6", True)
    twin(torch.from_numpy(inputs["x"]).to(DEV), layout="nhwc")             # a forward of the copy does not touch m's
    assert twin.variant_state() == {"act": "relu6", "same": True}
    y.backward(torch.from_numpy(inputs["gy"]).to(DEV))
    assert torch.equal(x.grad.cpu(), want["dx"])
    with torch.no_grad():                                  # a forward without a graph holds nothing: the variant may change
        m(x.detach(), layout="nhwc")
    m._handle.variant_set("relu", False)
    assert m.variant_state() == {"act": "relu", "same": False}


# ---- through the model

def _yololite_n():
    from yololite_amd.program import synth_state_dict, zoo_meta
    meta = zoo_meta("yololite_n", num_classes=3, img_size=64)
    sd = synth_state_dict(meta)
    model = ya.build_model_from_meta(meta)
    model.load_state_dict(sd)
    model.to(DEV)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(DEV)
    return meta, sd, model, x


def _restated(stack, x):
    """the float64 restatement of the eval-mode stack on x, and the bar an fp32 evaluation gets against it:
    max(4 x the fp32 restatement's error, 2 fp32 ulps at the largest value)"""
    blocks = [dict(type="ir", k=d["k"], s=d["s"], mid=d["mid"], c=d["c"], name=d["name"]) for d in stack.blocks_cfg]
    case = dict(name="part", B=int(x.shape[0]), S=int(x.shape[1]), cin=stack.in_channels, prefix="backbone.", blocks=blocks)
    sd = {k: v.detach().cpu().numpy() for k, v in stack.state_dict().items()}
    So = stack.out_size(case["S"])
    inputs = dict(params={k: v for k, v in sd.items() if "running_" not in k and "tracked" not in k},
                  buffers={k: v for k, v in sd.items() if "running_" in k or "tracked" in k}, x=x.cpu().numpy(),
                  gy=np.zeros((case["B"], So, So, stack.out_channels), np.float32))
    r64 = stack_all(case, inputs, False)["y"]
    r32 = stack_all(case, inputs, False, np.float32)["y"]
    return r64, bar(np.abs(r32.astype(np.float64) - r64).max(), np.abs(r64).max())


def _check_against_executor(model, mid, tail, x):
    """the stacks in eval mode on the executor's own inputs: each within its bar of the float64 restatement, and within
    2 bars of what the executor gives (the rule of test_dense_neck_train_gpu.py for this model family)"""
    c3, c4, c5 = model.features(x)
    for what, stack, inp, theirs in (("c4", mid, c3, c4), ("c5", tail, c4, c5)):
        if stack is None:
            continue
        with torch.no_grad():
            ours = stack.eval()(inp, layout="nhwc")
        r64, b = _restated(stack, inp)
        eo = np.abs(ours.cpu().numpy().astype(np.float64) - r64).max()
        ee = np.abs(theirs.cpu().numpy().astype(np.float64) - r64).max()
        diff = float((ours - theirs).abs().max())
        print(f"{what}: stack err {eo:.3e}  executor err {ee:.3e}  bar {b:.3e}  diff {diff:.3e}")
        assert ours.shape == theirs.shape
        assert eo <= b and diff <= 2 * b, (what, eo, diff, b)


def test_eval_tail_and_mid_agree_with_the_executor():
    meta, sd, model, x = _yololite_n()
    before = [f.clone() for f in model.features(x)]
    tail = ya.tail_for(meta, sd).to(DEV)
    mid = ya.EfficientNetLiteMid.from_state_dict(meta, sd).to(DEV)
    assert type(tail) is ya.EfficientNetLiteTail
    assert (mid.in_channels, mid.out_channels, tail.in_channels, tail.out_channels) == (40, 112, 112, 320)
    assert [tuple(f.shape) for f in before] == [(2, 8, 8, 40), (2, 4, 4, 112), (2, 2, 2, 320)]
    _check_against_executor(model, mid, tail, x)
    for a, b in zip(before, model.features(x)):            # the executor's own contexts behave as before
        assert torch.equal(a, b)


def test_six_steps_through_neck_heads_and_loss_and_the_checkpoint_round_trip():
    """tail_for + neck_for + DetectHeads through LossAF(grad=True) and FusedTrainStep on a synthetic yololite_n at 64 px,
    the tail's parameters a group of their own (SGD with momentum 0.9 at the rates of the edge_n test overshoots on this
    model from the second step on: 12.3, 10.5, 11.9, 13.2, ...): the loss falls, every step is finite, and the merged checkpoint in a
    fresh model gives the C5 that tail.eval() gives: what tools/finetune_heads.py writes is what tools/infer.py runs"""
    meta, sd, model, x = _yololite_n()
    tail = ya.tail_for(meta, sd).to(DEV).train()
    neck = ya.neck_for(meta, sd).to(DEV).train()
    heads = ya.DetectHeads.from_state_dict(meta, sd).to(DEV).train()
    assert type(tail) is ya.EfficientNetLiteTail and type(neck) is ya.DetectNeckMS
    crit = ya.LossAF(3, 64, grad=True)
    rest = list(neck.parameters()) + list(heads.parameters())
    # the optimizer, rate and clip that tools/finetune_heads.py runs by default; the tail at half the rate
    fts = ya.FusedTrainStep([{"params": rest}, {"params": list(tail.parameters()), "lr": 5e-4}], optimizer="adamw", grad_clip=10.0,
                            amp=False, lr=1e-3)
    tg = _targets(dict(E2E, B=2))
    c3, c4, _ = model.features(x)
    start = {n: p.detach().clone() for n, p in tail.named_parameters()}
    losses = []
    for _ in range(6):
        fts.zero_grad()
        c5 = tail(c4, layout="nhwc")
        loss = crit(heads(neck([c3, c4, c5], layout="nhwc"), layout="nhwc"), tg)[0]
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in tail.parameters())
        fts.step()
        losses.append(float(loss.detach()))
    print("losses", losses)
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert not [n for n, p in tail.named_parameters() if torch.equal(p, start[n])]      # every tail parameter has moved
    merged = dict(sd)
    for mod in (tail, neck, heads):
        merged.update({k: v.detach().cpu().numpy() for k, v in mod.state_dict().items()})
    assert set(sd) <= set(merged)
    changed = [k for k in sd if not np.array_equal(np.asarray(sd[k]), merged[k])]
    assert any(k.startswith("backbone.blocks.5.") for k in changed) and any(k.startswith("backbone.blocks.6.") for k in changed)
    assert all(k.startswith(("backbone.blocks.5.", "backbone.blocks.6.", "lateral", "smooth", "head")) for k in changed)
    m2 = ya.build_model_from_meta(copy.deepcopy(meta))
    m2.load_state_dict(merged)
    m2.to(DEV)
    _check_against_executor(m2, None, tail, x)
