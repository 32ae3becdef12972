"""Trainable dense stem and whole backbone on the device (yololite_amd.stemops.ConvStack / BackboneStem,
stageops.BackboneMid / MobileNetV4Backbone, csrc/yl_stem.hip) against the oracle's fixture, the executor, and a short fit
through neck, heads and loss.

Fixture parity, per case, mode and tensor: the bar is max(4 x the oracle's own fp32 error, 2 fp32 ulps at the tensor's
largest magnitude), the rule of the head tests; the worst device error / bar of each case is written to
profiles/stem_train_parity.json."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import yololite_amd as ya
from _neck_cases import E2E
from _stem_cases import (CASES, FIXTURE, TINY, WIDE, backward_launches, bar, case_inputs, fixture_path, fixture_tensors, forward_launches,
                         modes, stack_all, tiny_inputs, tiny_tensor_shapes)
from _stem_dev import parity_ratios, ratios, restated_features, run as _run, run_tiny, stack_of as _stack, tiny_backbone
from _train_dev import DEV, edge_n as _edge_n, same as _same, targets as _targets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "stem_train_parity.json")
BY_NAME = {c["name"]: c for c in CASES}


def _judge(name, per_mode):
    bad, worst = [], {}
    for mode, table in per_mode.items():
        for n, (err, b) in table.items():
            print(f"{name:14s} {mode:5s} {n:50s} err {err:.3e}  bar {b:.3e}  ratio {err / b:.3f}")
            if err / b > worst.get(mode, (0.0,))[0]:
                worst[mode] = (err / b, n)
            if not err <= b:
                bad.append((mode, n, err, b))
    try:                                                   # the figures of this run, beside the others' (best effort)
        table = json.load(open(PARITY)) if os.path.exists(PARITY) else {}
        table[name] = {m: {"worst_ratio": round(r, 4), "tensor": t} for m, (r, t) in worst.items()}
        with open(PARITY, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass
    assert not bad, bad


@pytest.mark.parametrize("case", CASES + WIDE, ids=[c["name"] for c in CASES + WIDE])
def test_fixture_parity(case):
    z = np.load(fixture_path(case))
    _judge(case["name"], {mode: parity_ratios(case, mode, z) for mode in modes(case)})


@pytest.mark.parametrize("case", WIDE, ids=[c["name"] for c in WIDE])
def test_sampled_tensors_agree_with_the_restatement_everywhere(case):
    """the fixture stores tensors above 8192 elements at a sample (only the wide cases have any); here every element of
    those is held to the float64 restatement (which test_stem_train_cpu.py ties to the fixture), under the fixture's bar"""
    want = fixture_tensors(np.load(fixture_path(case)), case, "train")
    sampled = [n for n, v in want.items() if v[1] is not None]
    assert sampled
    inputs = case_inputs(case)
    got = _run(_stack(case, inputs), case, inputs)
    ref = stack_all(case, inputs, True)
    for n in sampled:
        _, _, e32, m64 = want[n]
        err = np.abs(got[n].numpy().astype(np.float64) - np.asarray(ref[n])).max()
        assert err <= bar(e32, m64), (n, err, bar(e32, m64))


def test_the_whole_tiny_backbone_against_the_fixture():
    """image -> [c3, c4, c5] with independent gradients into all three maps: pins the gradient joins at C3 and C4"""
    inputs = tiny_inputs()
    got = run_tiny(tiny_backbone(inputs), inputs)
    want = fixture_tensors(np.load(FIXTURE), TINY, "train", tiny_tensor_shapes())
    _judge(TINY["name"], {"train": ratios(got, want, TINY["name"])})


def test_two_steps_give_equal_bits():
    for case in (BY_NAME["planar3"], BY_NAME["rows"], BY_NAME["stem_to_c3"]):
        inputs = case_inputs(case)
        _same(_run(_stack(case, inputs), case, inputs), _run(_stack(case, inputs), case, inputs))
    inputs = tiny_inputs()
    _same(run_tiny(tiny_backbone(inputs), inputs), run_tiny(tiny_backbone(inputs), inputs))


def test_launch_counts_are_the_headers_and_gradients_nobody_asked_for_are_not_computed():
    for case in CASES:
        inputs = case_inputs(case)
        m = _stack(case, inputs)
        _run(m, case, inputs)
        assert m.last_launches == {"forward": forward_launches(case, True), "backward": backward_launches(case, True, not case["planar"])}, case["name"]
    # a planar input: unit 0 has no input-gradient launch (3x3 stride 2 at S 9 would be 1 + 4)
    case = BY_NAME["planar3"]
    inputs = case_inputs(case)
    m = _stack(case, inputs)
    _run(m, case, inputs)
    assert m.last_launches == {"forward": 5, "backward": 1 + 1 + 1 + 2}
    # the same unit on an NHWC input that wants its gradient: pack + four parity classes more
    case = BY_NAME["s2even"]
    inputs = case_inputs(case)
    m = _stack(case, inputs)
    full = _run(m, case, inputs)
    assert m.last_launches == {"forward": 5, "backward": 5 + 1 + 4}
    m = _stack(case, inputs)
    nodx = _run(m, case, inputs, x_grad=False)
    assert m.last_launches["backward"] == 5 and "dx" not in nodx
    _same({n: v for n, v in full.items() if n != "dx"}, nodx)
    # four units; the first two frozen: nothing upstream of blocks.1.0 runs
    case = BY_NAME["stem_to_c3"]                           # 3x3 s2 (planar), 3x3 s2, 3x3 s2, 1x1
    inputs = case_inputs(case)
    m = _stack(case, inputs)
    full = _run(m, case, inputs)
    assert m.last_launches == {"forward": 3 * 5 + 4, "backward": (5 + 1) + (5 + 5) + (5 + 5) + 5}
    m = _stack(case, inputs)
    for n, p in m.named_parameters():
        p.requires_grad_(n.startswith("backbone.blocks.1."))
    part = _run(m, case, inputs)
    assert m.last_launches["backward"] == (5 + 1) + 5 == backward_launches(case, True, False, [False, False, True, True])
    for n, p in m.named_parameters():
        assert (p.grad is None) == (not n.startswith("backbone.blocks.1.")), n
    _same({n: v for n, v in full.items() if n in part}, part)
    # only the last unit's BatchNorm: two launches
    m = _stack(case, inputs)
    for n, p in m.named_parameters():
        p.requires_grad_(n.startswith("backbone.blocks.1.1.bn1."))
    bn = _run(m, case, inputs)
    assert m.last_launches["backward"] == 2
    _same({n: v for n, v in full.items() if n in bn}, bn)
    # eval mode, no graph: one launch per unit less
    m.eval()
    with torch.no_grad():
        y = m(torch.from_numpy(inputs["x"]).to(DEV).permute(0, 3, 1, 2).contiguous())
    assert y.grad_fn is None and m.last_launches["forward"] == forward_launches(case, False) == 3 * 4 + 3


def test_a_frozen_stem_runs_nothing_upstream_of_the_first_wanted_gradient():
    inputs = tiny_inputs()
    m = tiny_backbone(inputs)
    full = run_tiny(m, inputs)
    m = tiny_backbone(inputs)
    m.stem.requires_grad_(False)
    part = run_tiny(m, inputs)
    assert m.stem.last_launches["backward"] == 0 and m.mid.last_launches["backward"] > 0
    assert all(p.grad is None for p in m.stem.parameters())
    _same({n: v for n, v in full.items() if n in part}, part)
    # eval() as well: the stem's BatchNorms use and keep their running statistics
    m = tiny_backbone(inputs)
    m.stem.requires_grad_(False).eval()
    before = {k: v.clone() for k, v in m.stem.state_dict().items()}
    run_tiny(m, inputs)
    assert all(torch.equal(v, before[k]) for k, v in m.stem.state_dict().items())
    assert m.stem.last_launches == {"forward": 3 * 4 + 3, "backward": 0}


def test_no_grad_saves_nothing_and_the_handle_holds_what_the_plan_says():
    case = BY_NAME["stem_to_c3"]
    inputs = case_inputs(case)
    m = _stack(case, inputs)
    x = torch.from_numpy(inputs["x"]).to(DEV).permute(0, 3, 1, 2).contiguous()
    plan = ya.stemops.plan(case["cin"], case["units"], case["B"], case["S"], input_layout="nchw")
    with torch.no_grad():
        quiet = m(x)
    h = m.held()
    assert h["forward_held"] == 0 and h["saved_bytes"] == plan["nosave_bytes"] < plan["saved_bytes"], (h, plan)
    y = m(x)
    assert m.held() == dict(saved_bytes=plan["saved_bytes"], workspace_bytes=plan["workspace_bytes"], forward_held=1)
    assert torch.equal(quiet, y)


def test_a_second_forward_and_a_one_row_training_unit_are_refused():
    case = BY_NAME["s2to1"]
    inputs = case_inputs(case)
    m = _stack(case, inputs)
    x = torch.from_numpy(inputs["x"]).to(DEV)
    y1 = m(x)
    m(x)
    with pytest.raises(ya.YoloLiteHipError, match="another forward"):
        y1.sum().backward()
    with pytest.raises(ValueError, match="more than 1 value"):
        m(x[:1])                                           # B 1, S 2 -> 1: one output row
    # and by the library itself, before any launch
    hd, lib = m._handle, ya.stemops._lib
    table = hd.table([p.detach() for p in m._param_list()], m._stat_buffers())
    out, n = torch.empty(1, 1, 1, 8, device=DEV), ctypes.c_int32()
    nbt = int(m.state_dict()["units.0.bn1.num_batches_tracked"])
    with pytest.raises(ya.YoloLiteHipError, match="yl_stem_forward"):
        hd.call("forward", ctypes.byref(table), x.data_ptr(), 1, 2, lib.YL_HEAD_TRAIN, out.data_ptr(),
                torch.cuda.current_stream().cuda_stream, ctypes.byref(n))
    for bits in (lib.YL_HEAD_F16, lib.YL_HEAD_BF16, 4):    # fp32 only: the precision bits are refused
        with pytest.raises(ya.YoloLiteHipError, match="yl_stem_forward"):
            hd.call("forward", ctypes.byref(table), x.data_ptr(), 2, 2, lib.YL_HEAD_TRAIN | bits, out.data_ptr(),
                    torch.cuda.current_stream().cuda_stream, ctypes.byref(n))
    assert int(m.state_dict()["units.0.bn1.num_batches_tracked"]) == nbt
    m.eval()
    assert m(x[:1]).shape == (1, 1, 1, 8)


def _check_against_executor(model, backbone, x):
    feats = model.features(x)
    with torch.no_grad():
        ours = backbone.eval()(x)
    for name, o, e, (r64, b) in zip(("c3", "c4", "c5"), ours, feats, restated_features(backbone, x)):
        eo = np.abs(o.cpu().numpy().astype(np.float64) - r64).max()
        ee = np.abs(e.cpu().numpy().astype(np.float64) - r64).max()
        print(f"{name}: backbone err {eo:.3e}  executor err {ee:.3e}  bar {b:.3e}")
        assert o.shape == e.shape
        assert eo <= b and ee <= b, (name, eo, ee, b)


def test_eval_backbone_agrees_with_the_executor():
    meta, sd, model, x = _edge_n()
    before = [f.clone() for f in model.features(x)]
    bb = ya.MobileNetV4Backbone.from_state_dict(meta, sd).to(DEV)
    _check_against_executor(model, bb, x)
    for a, b in zip(before, model.features(x)):            # the executor's own contexts behave as before
        assert torch.equal(a, b)


def test_six_steps_of_backbone_neck_heads_and_loss_and_the_checkpoint_round_trip():
    """backbone + DetectNeck + DetectHeads through LossAF(grad=True) and FusedTrainStep, the backbone's parameters a group
    of their own: the loss falls, every step is finite, and the merged checkpoint in a fresh model gives the maps that
    backbone.eval() gives: what tools/finetune_heads.py --train-backbone writes is what tools/infer.py runs"""
    meta, sd, model, x = _edge_n()
    bb = ya.MobileNetV4Backbone.from_state_dict(meta, sd).to(DEV).train()
    neck = ya.DetectNeck.from_state_dict(meta, sd).to(DEV).train()
    heads = ya.DetectHeads.from_state_dict(meta, sd).to(DEV).train()
    crit = ya.LossAF(3, 64, grad=True)
    rest = list(neck.parameters()) + list(heads.parameters())
    fts = ya.FusedTrainStep([{"params": rest}, {"params": list(bb.parameters()), "lr": 0.005}], optimizer="sgd", amp=False,
                            lr=0.01, momentum=0.9)
    tg = _targets(dict(E2E, B=2))
    start = {n: p.detach().clone() for n, p in bb.named_parameters()}
    losses = []
    for _ in range(6):
        fts.zero_grad()
        loss = crit(heads(neck(bb(x), layout="nhwc"), layout="nhwc"), tg)[0]
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in bb.parameters())
        fts.step()
        losses.append(float(loss.detach()))
    print("losses", losses)
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    # every convolution of the backbone has moved (a BatchNorm bias in front of a train-mode BatchNorm has a gradient that
    # is zero in exact arithmetic: it may stay where it was)
    assert not [n for n, p in bb.named_parameters() if p.dim() == 4 and torch.equal(p, start[n])]
    merged = dict(sd)
    for mod in (bb, neck, heads):
        merged.update({k: v.detach().cpu().numpy() for k, v in mod.state_dict().items()})
    assert set(sd) <= set(merged)
    changed = [k for k in sd if not np.array_equal(np.asarray(sd[k]), merged[k])]
    assert any(k.startswith("backbone.conv_stem") for k in changed) and any(k.startswith("backbone.blocks.2.") for k in changed)
    m2 = ya.build_model_from_meta(copy.deepcopy(meta))
    m2.load_state_dict(merged)
    m2.to(DEV)
    _check_against_executor(m2, bb, x)
