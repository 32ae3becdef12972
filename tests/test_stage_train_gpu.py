"""Trainable backbone stage on the device (yololite_amd.stageops.UIBStack / BackboneTail, csrc/yl_stage.hip) against the
oracle's fixture, the executor, and a short fit through neck, heads and loss.

Fixture parity, per case, mode and tensor: the bar is max(4 x the oracle's own fp32 error, 2 fp32 ulps at the tensor's
largest magnitude), the rule of the head tests; the worst device error / bar of each case is written to
profiles/stage_train_parity.json."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import yololite_amd as ya
from _neck_cases import E2E
from _stage_cases import CASES, WIDE, bar, case_inputs, fixture_path, fixture_tensors, modes, stack_all
from _stage_dev import parity_ratios, run as _run, stack_of as _stack
from _train_dev import DEV, edge_n as _edge_n, same as _same, targets as _targets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "stage_train_parity.json")
BY_NAME = {c["name"]: c for c in CASES + WIDE}


@pytest.mark.parametrize("case", CASES + WIDE, ids=[c["name"] for c in CASES + WIDE])
def test_fixture_parity(case):
    z = np.load(fixture_path(case))
    bad, worst = [], {}
    for mode in modes(case):
        for n, (err, b) in parity_ratios(case, mode, z).items():
            print(f"{case['name']:10s} {mode:5s} {n:50s} err {err:.3e}  bar {b:.3e}  ratio {err / b:.3f}")
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
    those is held to the float64 restatement (which test_stage_train_cpu.py ties to the fixture), under the fixture's bar"""
    case = BY_NAME[name]
    want = fixture_tensors(np.load(fixture_path(case)), case, "train")
    sampled = [n for n, v in want.items() if v[1] is not None]
    if not sampled:
        return                                             # nothing of this case is stored sampled
    inputs = case_inputs(case)
    got = _run(_stack(case, inputs), inputs)
    ref = stack_all(case, inputs, True)
    for n in sampled:
        _, _, e32, m64 = want[n]
        err = np.abs(got[n].numpy().astype(np.float64) - ref[n]).max()
        assert err <= bar(e32, m64), (n, err, bar(e32, m64))


def test_two_runs_give_the_same_bits_in_both_input_layouts():
    for case in (BY_NAME["a5k5s2"], BY_NAME["rows"], BY_NAME["tiny_tail"]):
        inputs = case_inputs(case)
        first = _run(_stack(case, inputs), inputs)
        for layout in ("nhwc", "nchw"):
            _same(first, _run(_stack(case, inputs), inputs, layout=layout))


def test_gradients_nobody_asked_for_are_not_computed():
    """the launch counts are those include/yololite_hip.h documents: a unit's forward is 4 launches in train mode and 3
    in eval mode; its backward 1 (sums) + 1 (bn grads) + 1 (dz) + 2 (weight gradient) + 1 (input gradient), and a
    residual block's add is 1"""
    case = BY_NAME["k3res"]                                # pw_exp, dw_mid, pw_proj; residual
    inputs = case_inputs(case)
    m = _stack(case, inputs)
    full = _run(m, inputs)
    assert m.last_launches == {"forward": 3 * 4, "backward": 3 * 6 + 1}
    # the input does not require grad: unit 0's input gradient and the residual's add are not run
    m = _stack(case, inputs)
    nodx = _run(m, inputs, x_grad=False)
    assert m.last_launches["backward"] == 3 * 6 - 1
    assert "dx" not in nodx
    _same({n: v for n, v in full.items() if n != "dx"}, nodx)
    # a frozen first block, and an input that does not require grad: nothing upstream of block 3.1 runs
    case = BY_NAME["tiny_tail"]                            # 3.0: four units; 3.1: three, residual; 4.0: one
    inputs = case_inputs(case)
    m = _stack(case, inputs)
    full = _run(m, inputs)
    assert m.last_launches == {"forward": 8 * 4, "backward": 8 * 6 + 1}
    m = _stack(case, inputs)
    for n, p in m.named_parameters():
        p.requires_grad_(not n.startswith("backbone.blocks.3.0."))
    part = _run(m, inputs, x_grad=False)
    assert m.last_launches["backward"] == 3 * 6 + 5
    for n, p in m.named_parameters():
        assert (p.grad is None) == n.startswith("backbone.blocks.3.0."), n
    assert any(n.startswith("g.backbone.blocks.3.1.") for n in part) and any(n.startswith("g.backbone.blocks.4.0.") for n in part)
    _same({n: v for n, v in full.items() if n in part}, part)
    # only the last block's BatchNorm: two launches
    m = _stack(case, inputs)
    for n, p in m.named_parameters():
        p.requires_grad_(n.startswith("backbone.blocks.4.0.bn1."))
    bn = _run(m, inputs, x_grad=False)
    assert m.last_launches["backward"] == 2
    _same({n: v for n, v in full.items() if n in bn}, bn)
    assert sorted(n for n in bn if n.startswith("g.")) == ["g.backbone.blocks.4.0.bn1.bias", "g.backbone.blocks.4.0.bn1.weight"]
    # everything frozen, the input wanted: the whole walk for dx alone (sums, bn grads, dz, input gradient) and the add
    m = _stack(case, inputs)
    for p in m.parameters():
        p.requires_grad_(False)
    dx = _run(m, inputs)
    assert m.last_launches["backward"] == 8 * 4 + 1
    assert torch.equal(dx["dx"], full["dx"])
    # eval mode, no graph: 3 launches per unit
    m.eval()
    with torch.no_grad():
        y = m(torch.from_numpy(inputs["x"]).to(DEV), layout="nhwc")
    assert y.grad_fn is None and m.last_launches["forward"] == 8 * 3


def test_no_grad_saves_nothing_and_the_handle_holds_what_the_plan_says():
    case = BY_NAME["tiny_tail"]
    inputs = case_inputs(case)
    m = _stack(case, inputs)
    x = torch.from_numpy(inputs["x"]).to(DEV)
    plan = ya.stageops.plan(case["cin"], case["blocks"], case["B"], case["S"])
    with torch.no_grad():
        quiet = m(x, layout="nhwc")
    h = m.held()
    assert h["forward_held"] == 0 and h["saved_bytes"] == plan["nosave_bytes"] < plan["saved_bytes"], (h, plan)
    y = m(x, layout="nhwc")
    assert m.held() == dict(saved_bytes=plan["saved_bytes"], workspace_bytes=plan["workspace_bytes"], forward_held=1)
    assert torch.equal(quiet, y)                           # the same y either way (the statistics are the batch's)
    assert int(m.state_dict()["backbone.blocks.4.0.bn1.num_batches_tracked"]) == 3 + 7 + 2


def test_a_second_forward_makes_the_stale_backward_raise_and_single_value_batches_raise():
    case = BY_NAME["s2to1"]
    inputs = case_inputs(case)
    m = _stack(case, inputs)
    x = torch.from_numpy(inputs["x"]).to(DEV)
    y1 = m(x, layout="nhwc")
    m(x, layout="nhwc")
    with pytest.raises(ya.YoloLiteHipError, match="another forward"):
        y1.sum().backward()
    with pytest.raises(ValueError, match="more than 1 value"):
        m(x[:1], layout="nhwc")                            # B 1, S 2 -> 1: one output row
    m.eval()
    assert m(x[:1], layout="nhwc").shape == (1, 1, 1, 8)


def test_the_precision_bits_of_the_flags_are_refused_and_a_held_forward_stays_held():
    """this stack is fp32: yl_stage_forward refuses YL_HEAD_F16 / YL_HEAD_BF16 before anything is enqueued"""
    import ctypes
    case = BY_NAME["k3res"]
    inputs = case_inputs(case)
    m = _stack(case, inputs)
    x = torch.from_numpy(inputs["x"]).to(DEV).requires_grad_(True)
    y = m(x, layout="nhwc")
    hd, lib = m._handle, ya.stageops._lib
    table = hd.table([p.detach() for p in m._param_list()], m._stat_buffers())
    out, n = torch.empty_like(y), ctypes.c_int32()
    nbt = int(m.state_dict()["blocks.0.0.pw_exp.bn.num_batches_tracked"])
    for bits in (lib.YL_HEAD_F16, lib.YL_HEAD_BF16, lib.YL_HEAD_F16 | lib.YL_HEAD_BF16, 4):
        with pytest.raises(ya.YoloLiteHipError, match="yl_stage_forward"):
            hd.call("forward", ctypes.byref(table), x.data_ptr(), case["B"], case["S"], lib.YL_HEAD_TRAIN | lib.YL_HEAD_SAVE | bits,
                    out.data_ptr(), torch.cuda.current_stream().cuda_stream, ctypes.byref(n))
    assert int(m.state_dict()["blocks.0.0.pw_exp.bn.num_batches_tracked"]) == nbt and m.held()["forward_held"] == 1
    y.backward(torch.from_numpy(inputs["gy"]).to(DEV))
    assert torch.equal(x.grad.cpu(), _run(_stack(case, inputs), inputs)["dx"])


def test_deepcopy_gives_a_handle_of_its_own():
    case = BY_NAME["k3res"]
    inputs = case_inputs(case)
    m = _stack(case, inputs)
    want = _run(_stack(case, inputs), inputs)
    x = torch.from_numpy(inputs["x"]).to(DEV).requires_grad_(True)
    y = m(x, layout="nhwc")
    twin = copy.deepcopy(m)
    assert twin._handle is not m._handle and twin._handle.handle is None
    twin(torch.from_numpy(inputs["x"]).to(DEV), layout="nhwc")             # a forward of the copy does not touch m's
    y.backward(torch.from_numpy(inputs["gy"]).to(DEV))
    assert torch.equal(x.grad.cpu(), want["dx"])
    for n, p in m.named_parameters():
        assert torch.equal(p.grad.cpu(), want["g." + n]), n
    assert all(p.grad is None for p in twin.parameters())


def _tail_case(tail, B, S):
    blocks = [{k: d[k] for k in ("type", "a", "k", "s", "mid", "c", "name")} for d in tail.blocks_cfg]
    return dict(name="tail", B=B, S=S, cin=tail.in_channels, prefix="backbone.", blocks=blocks)


def _restated_c5(tail, c4):
    """the float64 restatement of the eval-mode tail on c4, and the bar an fp32 evaluation gets against it:
    max(4 x the fp32 restatement's error, 2 fp32 ulps at the largest value)"""
    case = _tail_case(tail, int(c4.shape[0]), int(c4.shape[1]))
    sd = {k: v.detach().cpu().numpy() for k, v in tail.state_dict().items()}
    So = tail.out_size(case["S"])
    inputs = dict(params={k: v for k, v in sd.items() if "running_" not in k and "tracked" not in k},
                  buffers={k: v for k, v in sd.items() if "running_" in k or "tracked" in k}, x=c4.cpu().numpy(),
                  gy=np.zeros((case["B"], So, So, tail.out_channels), np.float32))
    r64 = stack_all(case, inputs, False)["y"]
    r32 = stack_all(case, inputs, False, np.float32)["y"]
    return r64, bar(np.abs(r32.astype(np.float64) - r64).max(), np.abs(r64).max())


def _check_against_executor(model, tail, x):
    c3, c4, c5 = model.features(x)
    with torch.no_grad():
        ours = tail.eval()(c4, layout="nhwc")
    r64, b = _restated_c5(tail, c4)
    eo = np.abs(ours.cpu().numpy().astype(np.float64) - r64).max()
    ee = np.abs(c5.cpu().numpy().astype(np.float64) - r64).max()
    print(f"c5: tail err {eo:.3e}  executor err {ee:.3e}  bar {b:.3e}  diff {float((ours - c5).abs().max()):.3e}")
    assert ours.shape == c5.shape
    assert eo <= b and ee <= b, (eo, ee, b)
    return c3, c4, ours


def test_eval_tail_agrees_with_the_executor():
    meta, sd, model, x = _edge_n()
    before = [f.clone() for f in model.features(x)]
    tail = ya.BackboneTail.from_state_dict(meta, sd).to(DEV)
    assert (tail.in_channels, tail.out_channels) == (48, 480)
    _check_against_executor(model, tail, x)
    for a, b in zip(before, model.features(x)):            # the executor's own contexts behave as before
        assert torch.equal(a, b)


def test_six_steps_through_neck_heads_and_loss_and_the_checkpoint_round_trip():
    """tail + DetectNeck + DetectHeads through LossAF(grad=True) and FusedTrainStep, the tail's parameters a group of
    their own: the loss falls, every step is finite, and the merged checkpoint in a fresh model gives the C5 that
    tail.eval() gives: what tools/finetune_heads.py writes is what tools/infer.py runs"""
    meta, sd, model, x = _edge_n()
    tail = ya.BackboneTail.from_state_dict(meta, sd).to(DEV).train()
    neck = ya.DetectNeck.from_state_dict(meta, sd).to(DEV).train()
    heads = ya.DetectHeads.from_state_dict(meta, sd).to(DEV).train()
    crit = ya.LossAF(3, 64, grad=True)
    rest = list(neck.parameters()) + list(heads.parameters())
    fts = ya.FusedTrainStep([{"params": rest}, {"params": list(tail.parameters()), "lr": 0.005}], optimizer="sgd", amp=False,
                            lr=0.01, momentum=0.9)
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
    assert any(k.startswith("backbone.blocks.3.") for k in changed) and any(k.startswith("backbone.blocks.4.") for k in changed)
    assert all(k.startswith(("backbone.blocks.3.", "backbone.blocks.4.", "lateral", "smooth", "head")) for k in changed)
    m2 = ya.build_model_from_meta(copy.deepcopy(meta))
    m2.load_state_dict(merged)
    m2.to(DEV)
    _check_against_executor(m2, tail, x)
