"""Trainable detection heads on the device (yololite_amd.headops.DetectHeads, csrc/yl_head.hip) against the reference's
fixture, the executor, and the CPU float64 training loop.

Fixture parity, per case, level and tensor (figures of one run on an MI355X, device error / bar, the worst tensor of
each case): see profiles/head_train_parity.json.  The bar is max(4 x the reference's own fp32 error, 2 fp32 ulps at
the tensor's largest magnitude), the rule of the loss and train-step tests."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import yololite_amd as ya
from _head_cases import CASES, E2E, FIXTURE, WIDE, bar, case_inputs, fixture_path, fixture_tensors, modes
from _head_dev import heads_of as _heads, parity_ratios, run as _run
from _head_np import head_forward
from _train_dev import DEV, edge_n as _edge_n, same as _same, targets as _targets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "head_train_parity.json")


@pytest.mark.parametrize("case", CASES + WIDE, ids=[c["name"] for c in CASES + WIDE])
def test_fixture_parity(case):
    z = np.load(fixture_path(case))
    bad, rows = [], []
    for mode in modes(case):
        for (li, n), (err, b) in parity_ratios(case, mode, z).items():
            print(f"{case['name']:5s} {mode:5s} L{li} {n:40s} err {err:.3e}  bar {b:.3e}  ratio {err / b:.3f}")
            rows.append(dict(case=case["name"], mode=mode, level=li, tensor=n, error=err, bar=b, ratio=round(err / b, 4)))
            if not err <= b:
                bad.append((mode, li, n, err, b))
    if case in WIDE:                                       # the figures of this run, beside the others' rows (best effort)
        try:
            table = [r for r in json.load(open(PARITY)) if r["case"] != case["name"]] if os.path.exists(PARITY) else []
            with open(PARITY, "w") as f:
                json.dump(table + rows, f, indent=1)
                f.write("\n")
        except OSError:
            pass
    assert not bad, bad


def test_large_tensors_agree_with_the_restatement_everywhere():
    """the fixture stores the 1x1 weight gradients of the F = 244 case at a sample of their elements; here every element
    is held to the float64 restatement (which test_head_train_cpu.py ties to the fixture), under the fixture's bar"""
    _everywhere("f244")


@pytest.mark.parametrize("name", [c["name"] for c in WIDE])
def test_large_tensors_of_the_wide_cases_agree_with_the_restatement_everywhere(name):
    """and so do the wide cases': every tensor their fixture stores sampled (the 1x1 weight gradients)"""
    _everywhere(name)


def _everywhere(name):
    from _head_np import head_all
    case = [c for c in CASES + WIDE if c["name"] == name][0]
    z = np.load(fixture_path(case))
    assert any(v[1] is not None for li in range(len(case["sizes"])) for v in fixture_tensors(z, case, "train", li).values())
    inputs = case_inputs(case)
    got = _run(_heads(case, inputs), inputs)
    for li, (lv, d) in enumerate(zip(inputs, got)):
        ref = head_all(lv["params"], lv["buffers"], lv["x"], lv["gy"], lv["k"], case["A"], case["C"], case["depth"], True)
        for n, (_, idx, e32, m64) in fixture_tensors(z, case, "train", li).items():
            if idx is not None:
                err = np.abs(d[n].numpy().astype(np.float64) - ref[n]).max()
                assert err <= bar(e32, m64), (li, n, err, bar(e32, m64))


def test_two_runs_give_the_same_bits_in_every_input_layout():
    for case in (CASES[1], CASES[4]):
        inputs = case_inputs(case)
        first = _run(_heads(case, inputs), inputs)
        for layout in ("nhwc", "nchw", "channels_last"):
            again = _run(_heads(case, inputs), inputs, layout=layout)
            for a, b in zip(first, again):
                _same(a, b)


def test_gradients_nobody_asked_for_are_not_computed():
    case = CASES[0]
    inputs = case_inputs(case)
    m = _heads(case, inputs)
    full = _run(m, inputs)
    assert [l["forward"] for l in m.last_launches()] == [6, 6, 6]        # depth 1, train: 5 + the outputs
    assert [l["backward"] for l in m.last_launches()] == [14, 14, 14]
    # the input does not require grad: no dx, one launch less, the same parameter gradients
    m = _heads(case, inputs)
    nodx = _run(m, inputs, x_grad=False)
    assert [l["backward"] for l in m.last_launches()] == [13, 13, 13]
    for a, b in zip(full, nodx):
        assert "dx" not in b
        _same({n: v for n, v in a.items() if n != "dx"}, b)
    # a frozen trunk: the four launches of the output convolutions only (weights: GEMM + sum, biases: column sums + sum)
    m = _heads(case, inputs)
    for n, p in m.named_parameters():
        p.requires_grad_(".out." in n)
    out = _run(m, inputs, x_grad=False)
    assert [l["backward"] for l in m.last_launches()] == [4, 4, 4]
    for n, p in m.named_parameters():
        assert (p.grad is None) == (".out." not in n), n
    for a, b in zip(full, out):
        _same({n: v for n, v in a.items() if n in b}, b)
    # BatchNorm's weight and bias only: up to the statistics of the block, no further
    m = _heads(case, inputs)
    for n, p in m.named_parameters():
        p.requires_grad_(".block.2." in n)
    out = _run(m, inputs, x_grad=False)
    assert [l["backward"] for l in m.last_launches()] == [3, 3, 3]
    for a, b in zip(full, out):
        assert sorted(n for n in b if n.startswith("g.")) == sorted(n for n in a if ".block.2." in n)
        _same({n: v for n, v in a.items() if n in b}, b)
    # eval mode: 4 launches per block
    m.eval()
    with torch.no_grad():
        ys = m([torch.from_numpy(lv["x"]).to(DEV) for lv in inputs])
    assert all(y.grad_fn is None and not y.requires_grad for y in ys)
    assert [l["forward"] for l in m.last_launches()] == [5, 5, 5]


def test_no_grad_saves_nothing_and_holds_one_blocks_buffers():
    """a module whose parameters require grad, in train mode, two blocks deep: under no_grad the handle keeps no forward
    for backward and has allocated one block's activations; the first recorded forward grows it to the plan's"""
    case = CASES[1]
    inputs = case_inputs(case)
    m = _heads(case, inputs)
    assert all(p.requires_grad for p in m.parameters()) and m.training and case["depth"] == 2
    xs = [torch.from_numpy(lv["x"]).to(DEV) for lv in inputs]
    plans = [ya.headops.plan(case["F"], case["C"], case["A"], case["depth"], case["B"], S) for S in case["sizes"]]
    with torch.no_grad():
        quiet = m(xs)
    assert all(y.grad_fn is None and not y.requires_grad for y in quiet)
    for h, p in zip(m.held(), plans):
        assert h["forward_held"] == 0 and h["saved_bytes"] == p["saved_bytes"] // 2, (h, p)
    bn = m.head3["trunk"][1].block[2]
    assert int(bn.num_batches_tracked) == 4 + 1            # train mode all the same: the running statistics moved
    ys = m(xs)
    for h, p in zip(m.held(), plans):
        assert h["forward_held"] == 1 and h["saved_bytes"] == p["saved_bytes"], (h, p)
    with torch.no_grad():                                  # and a later no_grad forward drops what was held
        m(xs)
    assert [h["forward_held"] for h in m.held()] == [0, 0]
    with pytest.raises(ya.YoloLiteHipError, match="another forward"):
        ys[0].sum().backward()


def test_the_handles_memory_grows_never_shrinks_and_is_cut_the_same_inside_a_larger_buffer():
    """the handle's memory through S = 4, 8, 4 (two blocks, so a block offset exists; two sizes, so the second S = 4
    step is cut out of a buffer made for S = 8): what it holds is the plan's, growth drops the held forward, nothing
    shrinks, and the step in the larger buffer gives the bits of a fresh module that ran only that step"""
    small = dict(name="arena", F=8, C=2, A=1, depth=2, B=2, sizes=(4,), seed=909)
    ins, inb = case_inputs(small), case_inputs(dict(small, sizes=(8,)))
    p4, p8 = (ya.headops.plan(8, 2, 1, 2, 2, S) for S in (4, 8))
    assert p8["saved_bytes"] > p4["saved_bytes"] and p8["workspace_bytes"] > p4["workspace_bytes"]
    m = _heads(small, ins)
    x4, x8 = torch.from_numpy(ins[0]["x"]).to(DEV), torch.from_numpy(inb[0]["x"]).to(DEV)
    y1 = m([x4], layout="nhwc")
    assert m.held() == [dict(saved_bytes=p4["saved_bytes"], workspace_bytes=p4["workspace_bytes"], forward_held=1)]
    m([x8], layout="nhwc")
    grown = dict(saved_bytes=p8["saved_bytes"], workspace_bytes=p8["workspace_bytes"], forward_held=1)
    assert m.held() == [grown]
    with pytest.raises(ya.YoloLiteHipError, match="another forward"):
        y1[0].sum().backward()
    m.zero_grad(set_to_none=True)
    x = x4.clone().requires_grad_(True)
    y = m([x], layout="nhwc")[0]
    assert m.held() == [grown]
    y.backward(torch.from_numpy(ins[0]["gy"]).to(DEV))
    fresh = _run(_heads(small, ins), ins)[0]
    assert torch.equal(y.detach().cpu(), fresh["y"]) and torch.equal(x.grad.cpu(), fresh["dx"])
    grads = {"g." + n: p.grad.cpu() for n, p in m.named_parameters()}
    _same(grads, {n: v for n, v in fresh.items() if n.startswith("g.")})


def test_a_cube_shaped_map_goes_by_the_layout_it_is_given():
    """S == F: [B,8,8,8] reads as NCHW and as NHWC.  Without a layout it is refused; with one the result is that of the
    float64 restatement on the map so read, and the other reading gives another result."""
    case = dict(name="cube", F=8, C=2, A=1, depth=1, B=2, sizes=(8,), seed=808)
    inputs = case_inputs(case)
    lv = inputs[0]
    m = _heads(case, inputs, train=False)
    x = torch.from_numpy(lv["x"]).to(DEV)                   # NHWC
    with pytest.raises(ValueError, match="layout="):
        m([x])
    with torch.no_grad():
        y = m([x], layout="nhwc")[0]
        y_cl = m([x.permute(0, 3, 1, 2)], layout="nchw")[0]           # the same map, NCHW shape over the same memory
        y_t = m([x], layout="nchw")[0]                               # another map: x's axes read as [B,F,S,S]
    args = (lv["params"], lv["buffers"], lv["x"], lv["k"], 1, 2, 1, False)
    with torch.no_grad():
        r64 = head_forward(*args, dtype=torch.float64)[0].numpy()
        r32 = head_forward(*args, dtype=torch.float32)[0].numpy()
    b = bar(np.abs(r32.astype(np.float64) - r64).max(), np.abs(r64).max())
    err = np.abs(y.cpu().numpy().astype(np.float64) - r64).max()
    print(f"cube: err {err:.3e}  bar {b:.3e}")
    assert err <= b
    assert torch.equal(y, y_cl)
    assert (y - y_t).abs().max().item() > 1e-2
    feats = [x.clone().requires_grad_(True)]
    m.train()
    m(feats, layout="nhwc")[0].sum().backward()
    assert feats[0].grad.shape == x.shape


def test_a_second_forward_replaces_the_held_one_and_single_value_batches_raise():
    case = CASES[0]
    inputs = case_inputs(case)
    m = _heads(case, inputs)
    xs = [torch.from_numpy(lv["x"]).to(DEV) for lv in inputs]
    y1 = m(xs)
    m(xs)
    with pytest.raises(ya.YoloLiteHipError, match="another forward"):
        y1[0].sum().backward()
    with pytest.raises(ValueError, match="more than 1 value"):
        m([x[:1, :1, :1] for x in xs])
    m.eval()
    assert m([x[:1, :1, :1] for x in xs])[0].shape == (1, 1, 1, 1, 8)


def _levels_bars(heads, feats):
    """the float64 restatement of the eval-mode heads on `feats`, and the bar an fp32 evaluation gets against it:
    max(4 x the CPU fp32 restatement's error, 2 fp32 ulps at the largest value)"""
    sd = {k: v.detach().cpu().numpy() for k, v in heads.state_dict().items()}
    out = []
    for n, A, f in zip(heads.level_names, heads.num_anchors_per_level, feats):
        k = int(n[1:])
        args = (sd, sd, f.cpu().numpy(), k, A, heads.num_classes, heads.head_depth, False)
        with torch.no_grad():
            r64 = head_forward(*args, dtype=torch.float64)[0].numpy()
            r32 = head_forward(*args, dtype=torch.float32)[0].numpy()
        out.append((r64, bar(np.abs(r32.astype(np.float64) - r64).max(), np.abs(r64).max())))
    return out


def _check_against_executor(model, heads, x):
    feats = model.pyramid(x)
    with torch.no_grad():
        ours = heads.eval()(feats)
    theirs = model(x)
    for li, (o, t, (r64, b)) in enumerate(zip(ours, theirs, _levels_bars(heads, feats))):
        eo = np.abs(o.cpu().numpy().astype(np.float64) - r64).max()
        et = np.abs(t.cpu().numpy().astype(np.float64) - r64).max()
        diff = (o - t).abs().max().item()
        print(f"L{li}: heads err {eo:.3e}  executor err {et:.3e}  diff {diff:.3e}  bar {b:.3e}")
        assert o.shape == t.shape and diff <= 2 * b, (li, diff, b)


def test_eval_heads_agree_with_the_executor():
    meta, sd, model, x = _edge_n()
    before = [o.clone() for o in model(x)]
    feats = model.pyramid(x)
    assert [tuple(f.shape) for f in feats] == [(2, s, s, 96) for s in (8, 4, 2)]
    _check_against_executor(model, ya.DetectHeads.from_state_dict(meta, sd).to(DEV), x)
    for a, b in zip(before, model(x)):                      # the executor's own contexts behave as before
        assert torch.equal(a, b)


def test_twenty_steps_fit_one_batch_as_the_float64_loop_does():
    ref = np.load(FIXTURE)["e2e/losses"]
    L0_ref, L20_ref = float(ref[0]), float(ref[-1])
    inputs = case_inputs(E2E)
    heads = _heads(E2E, inputs)
    start = {n: p.detach().clone() for n, p in heads.named_parameters()}
    feats = [torch.from_numpy(lv["x"]).to(DEV) for lv in inputs]
    crit = ya.LossAF(E2E["C"], E2E["img_size"], grad=True)
    fts = ya.FusedTrainStep(list(heads.parameters()), optimizer="sgd", amp=False, lr=E2E["lr"], momentum=E2E["momentum"],
                            nesterov=False, weight_decay=0.0)
    tg = _targets(E2E)
    losses = []
    for _ in range(E2E["steps"]):
        fts.zero_grad()
        loss, _ = crit(heads(feats), tg)
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in heads.parameters())
        fts.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(crit(heads(feats), tg)[0]))
    L0, L20 = losses[0], losses[-1]
    print(f"L0 {L0:.6f} (float64 loop {L0_ref:.6f})  L20 {L20:.6f} (float64 loop {L20_ref:.6f})")
    assert L0_ref - L20_ref >= 0.2 * L0_ref
    # every level's trunk and objectness row see a gradient (the negatives); box and class rows only where a level has
    # positive anchors
    same = [n for n, p in heads.named_parameters() if torch.equal(p, start[n])]
    assert not [n for n in same if ".trunk." in n or ".out.obj." in n], same
    assert any(".out.box." in n and n not in same for n in start) and any(".out.cls." in n and n not in same for n in start)
    assert L20 <= L0 - 0.5 * (L0 - L20_ref)
    bn = heads.head3["trunk"][0].block[2]
    assert int(bn.num_batches_tracked) == 3 + E2E["steps"] + 1


def test_trained_heads_round_trip_through_a_checkpoint():
    meta, sd, model, x = _edge_n()
    heads = ya.DetectHeads.from_state_dict(meta, sd).to(DEV).train()
    crit = ya.LossAF(3, 64, grad=True)
    fts = ya.FusedTrainStep(list(heads.parameters()), optimizer="sgd", amp=False, lr=0.01)
    tg = _targets(dict(E2E, B=2))
    feats = model.pyramid(x)
    for _ in range(2):
        fts.zero_grad()
        crit(heads(feats), tg)[0].backward()
        fts.step()
    merged = dict(sd)
    merged.update({k: v.detach().cpu().numpy() for k, v in heads.state_dict().items()})
    assert set(sd) <= set(merged)
    changed = [k for k in sd if not np.array_equal(np.asarray(sd[k]), merged[k])]
    assert changed and all(k.startswith("head") for k in changed)
    assert any("running_mean" in k for k in changed) and any(".out.cls.weight" in k for k in changed)
    m2 = ya.build_model_from_meta(copy.deepcopy(meta))
    m2.load_state_dict(merged)
    m2.to(DEV)
    _check_against_executor(m2, heads, x)
