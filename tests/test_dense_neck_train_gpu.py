"""Trainable dense FPN neck on the device (yololite_amd.neckops.DetectNeckMS, csrc/yl_dneck.hip) against the reference's
fixture, the executor, and the CPU float64 training loop.

Fixture parity, per case, level and tensor: the bar is max(4 x the reference's own fp32 error, 2 fp32 ulps at the
tensor's largest magnitude), the rule of the head tests; the worst device error / bar of each case is written to
profiles/dense_neck_train_parity.json."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import yololite_amd as ya
from yololite_amd.program import synth_state_dict, zoo_meta
from _head_np import head_forward
from _dense_neck_cases import CASES, E2E, FIXTURE, WIDE, bar, case_inputs, fixture_path, fixture_tensors, head_inputs, modes
from _dense_neck_dev import neck_of as _neck, parity_ratios, run as _run
from _dense_neck_np import neck_all, neck_forward
from _train_dev import DEV, same as _same, targets as _targets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "dense_neck_train_parity.json")
BY_NAME = {c["name"]: c for c in CASES + WIDE}


@pytest.mark.parametrize("case", CASES + WIDE, ids=[c["name"] for c in CASES + WIDE])
def test_fixture_parity(case):
    z = np.load(fixture_path(case))
    bad, worst = [], {}
    for mode in modes(case):
        for (li, n), (err, b) in parity_ratios(case, mode, z).items():
            print(f"{case['name']:6s} {mode:5s} L{li} {n:32s} err {err:.3e}  bar {b:.3e}  ratio {err / b:.3f}")
            if err / b > worst.get(mode, (0.0,))[0]:
                worst[mode] = (err / b, f"L{li} {n}")
            if not err <= b:
                bad.append((mode, li, n, err, b))
    try:                                                   # the figures of this run, beside the others' (best effort)
        table = json.load(open(PARITY)) if os.path.exists(PARITY) else {}
        table[case["name"]] = {m: {"worst_ratio": round(r, 4), "tensor": t} for m, (r, t) in worst.items()}
        with open(PARITY, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass
    assert not bad, bad


@pytest.mark.parametrize("name", [c["name"] for c in CASES + WIDE])
def test_sampled_tensors_agree_with_the_restatement_everywhere(name):
    """the fixture stores tensors above 8192 elements at a sample; here every element of those is held to the float64
    restatement (which test_dense_neck_train_cpu.py ties to the fixture), under the fixture's bar"""
    case = BY_NAME[name]
    z = np.load(fixture_path(case))
    sampled = [(li, n) for li in range(len(case["sizes"])) for n, v in fixture_tensors(z, case, "train", li).items()
               if v[1] is not None]
    if not sampled:
        return                                             # nothing of this case is stored sampled
    inputs = case_inputs(case)
    got = _run(_neck(case, inputs), inputs)
    ref = neck_all(inputs, case["depth"], True)
    for li, n in sampled:
        _, _, e32, m64 = fixture_tensors(z, case, "train", li)[n]
        err = np.abs(got[li][n].numpy().astype(np.float64) - ref[li][n]).max()
        assert err <= bar(e32, m64), (li, n, err, bar(e32, m64))


def test_two_runs_give_the_same_bits_in_all_three_input_layouts():
    for case in (BY_NAME["odd"], BY_NAME["rows"]):
        inputs = case_inputs(case)
        first = _run(_neck(case, inputs), inputs)
        for layout in ("nhwc", "nchw", "channels_last"):
            again = _run(_neck(case, inputs), inputs, layout=layout)
            for a, b in zip(first, again):
                _same(a, b)


def test_an_image_never_reads_its_neighbour():
    """Image seam: two eval-mode forward + backward passes of case rows (nine spatial tiles per image at the fine level)
    whose batches share image 0 and differ in image 1.  In eval mode nothing but a convolution window that crosses the
    image boundary (or wraps a row) can carry image 1 into image 0: p and dc of image 0 are bit-identical."""
    case = BY_NAME["rows"]
    inputs = case_inputs(case)
    rs = np.random.RandomState(99)
    cs2, gp2 = [], []
    for lv in inputs:
        c, g = lv["c"].copy(), lv["gp"].copy()
        c[1] = 100.0 * rs.standard_normal(c[1].shape).astype(np.float32)
        g[1] = 100.0 * rs.standard_normal(g[1].shape).astype(np.float32)
        cs2.append(c); gp2.append(g)
    a = _run(_neck(case, inputs, train=False), inputs)
    b = _run(_neck(case, inputs, train=False), inputs, cs=cs2, gps=gp2)
    for li, (x, y) in enumerate(zip(a, b)):
        for n in ("p", "dc"):
            assert torch.equal(x[n][0], y[n][0]), (li, n)
            assert not torch.equal(x[n][1], y[n][1]), (li, n)


def test_gradients_nobody_asked_for_are_not_computed():
    """the launch counts are those include/yololite_hip.h documents.  depth 1: a forward block is 4 launches (pack,
    convolution, statistics, BatchNorm + SiLU; 5 in train mode); backward in train mode, a block walked for its input
    gradient alone is 5 (sums, bn grads, dz, pack, convolution), with all its parameters 7 (5 without the input
    gradient); a lateral is 2 + 2 + 1; the gather of a level below the finest is 1"""
    case = BY_NAME["base"]
    inputs = case_inputs(case)
    m = _neck(case, inputs)
    full = _run(m, inputs)
    assert m.last_launches() == {"forward": 3 * (1 + 5), "backward": (7 + 5) + 2 * (1 + 7 + 5)}
    # no feature map requires grad: three dc launches less, the same parameter gradients
    m = _neck(case, inputs)
    nodc = _run(m, inputs, c_grad=False)
    assert m.last_launches()["backward"] == (7 + 4) + 2 * (1 + 7 + 4)
    for a, b in zip(full, nodc):
        assert "dc" not in b
        _same({n: v for n, v in a.items() if n != "dc"}, b)
    # only smooth5's parameters: every level's chain is walked, no lateral launch runs, block 0 of p5 has no input gradient
    m = _neck(case, inputs)
    for n, p in m.named_parameters():
        p.requires_grad_(n.startswith("smooth5."))
    out = _run(m, inputs, c_grad=False)
    assert m.last_launches()["backward"] == 5 + (1 + 5) + (1 + 5)
    for n, p in m.named_parameters():
        assert (p.grad is None) == (not n.startswith("smooth5.")), n
    for a, b in zip(full, out):
        _same({n: v for n, v in a.items() if n in b}, b)
    assert sorted(n for n in out[2] if n.startswith("g.")) == sorted(n for n in full[2] if n.startswith("g.smooth5."))
    # only lateral3: levels 4 and 5 run nothing
    m = _neck(case, inputs)
    for n, p in m.named_parameters():
        p.requires_grad_(n.startswith("lateral3."))
    out = _run(m, inputs, c_grad=False)
    assert m.last_launches()["backward"] == 5 + 2 + 2
    for n, p in m.named_parameters():
        assert (p.grad is None) == (not n.startswith("lateral3.")), n
    _same({n: v for n, v in full[0].items() if n in out[0]}, out[0])
    assert {"g.lateral3.weight", "g.lateral3.bias"} <= set(out[0])
    # dc only for the maps that require grad: c4 alone, all parameters frozen
    m = _neck(case, inputs)
    for p in m.parameters():
        p.requires_grad_(False)
    out = _run(m, inputs, c_grad=[False, True, False])
    assert m.last_launches()["backward"] == 5 + (1 + 5 + 1)
    assert ["dc" in d for d in out] == [False, True, False]
    assert torch.equal(out[1]["dc"], full[1]["dc"])
    # eval mode: 4 launches per block
    m.eval()
    with torch.no_grad():
        ps = m([torch.from_numpy(lv["c"]).to(DEV) for lv in inputs], layout="nhwc")
    assert all(p.grad_fn is None and not p.requires_grad for p in ps)
    assert m.last_launches()["forward"] == 3 * (1 + 4)


def test_no_grad_saves_nothing_and_holds_one_blocks_buffers():
    case = BY_NAME["odd"]
    inputs = case_inputs(case)
    m = _neck(case, inputs)
    assert all(p.requires_grad for p in m.parameters()) and m.training and case["depth"] == 2
    cs = [torch.from_numpy(lv["c"]).to(DEV) for lv in inputs]
    plan = ya.neckops.plan_ms(case["Cin"], case["F"], case["depth"], case["B"], case["sizes"])
    with torch.no_grad():
        quiet = m(cs)
    assert all(p.grad_fn is None and not p.requires_grad for p in quiet)
    h = m.held()
    assert h["forward_held"] == 0 and h["saved_bytes"] == plan["nosave_bytes"] < plan["saved_bytes"], (h, plan)
    bn = m.smooth3[4]
    assert int(bn.num_batches_tracked) == 4 + 1            # train mode all the same: the running statistics moved
    ps = m(cs)
    h = m.held()
    assert h["forward_held"] == 1 and h["saved_bytes"] == plan["saved_bytes"], (h, plan)
    assert h["workspace_bytes"] == plan["workspace_bytes"]
    for a, b in zip(quiet, ps):                            # the same p either way (the statistics are the batch's)
        assert torch.equal(a, b)
    with torch.no_grad():                                  # a later no_grad forward drops what was held
        m(cs)
    assert m.held()["forward_held"] == 0
    with pytest.raises(ya.YoloLiteHipError, match="another forward"):
        ps[0].sum().backward()


def test_the_handles_memory_grows_never_shrinks_and_is_cut_the_same_inside_a_larger_buffer():
    """the handle's memory through the sizes (4, 2), (8, 4), (4, 2) (two blocks, so a block offset exists): what it holds
    is the plan's, growth drops the held forward, nothing shrinks, and the step in the larger buffers gives the bits of
    a fresh module that ran only that step"""
    small = dict(name="arena", B=2, F=8, Cin=(8, 8), depth=2, sizes=(4, 2), seed=929)
    big = dict(small, sizes=(8, 4))
    ins, inb = case_inputs(small), case_inputs(big)
    plan, plan_big = (ya.neckops.plan_ms((8, 8), 8, 2, 2, c["sizes"]) for c in (small, big))
    assert plan_big["saved_bytes"] > plan["saved_bytes"] and plan_big["workspace_bytes"] > plan["workspace_bytes"]
    m = _neck(small, ins)
    cs, cb = ([torch.from_numpy(lv["c"]).to(DEV) for lv in i] for i in (ins, inb))
    p1 = m(cs, layout="nhwc")
    assert m.held() == dict(saved_bytes=plan["saved_bytes"], workspace_bytes=plan["workspace_bytes"], forward_held=1)
    m(cb, layout="nhwc")
    grown = dict(saved_bytes=plan_big["saved_bytes"], workspace_bytes=plan_big["workspace_bytes"], forward_held=1)
    assert m.held() == grown
    with pytest.raises(ya.YoloLiteHipError, match="another forward"):
        p1[0].sum().backward()
    m.zero_grad(set_to_none=True)
    cs = [c.clone().requires_grad_(True) for c in cs]
    ps = m(cs, layout="nhwc")
    assert m.held() == grown
    torch.autograd.backward(ps, [torch.from_numpy(lv["gp"]).to(DEV) for lv in ins])
    fresh = _run(_neck(small, ins), ins)
    grads = {"g." + n: q.grad.cpu() for n, q in m.named_parameters()}
    for lv, c, p, f in zip(ins, cs, ps, fresh):
        assert torch.equal(p.detach().cpu(), f["p"]) and torch.equal(c.grad.cpu(), f["dc"])
        own = {n: v for n, v in grads.items() if n.startswith((f"g.lateral{lv['k']}.", f"g.smooth{lv['k']}."))}
        _same(own, {n: v for n, v in f.items() if n.startswith("g.")})
    assert sum(n.startswith("g.") for f in fresh for n in f) == len(grads)


def test_a_second_forward_replaces_the_held_one_and_single_value_batches_raise():
    case = BY_NAME["base"]
    inputs = case_inputs(case)
    m = _neck(case, inputs)
    cs = [torch.from_numpy(lv["c"]).to(DEV) for lv in inputs]
    p1 = m(cs, layout="nhwc")
    m(cs, layout="nhwc")
    with pytest.raises(ya.YoloLiteHipError, match="another forward"):
        p1[0].sum().backward()
    with pytest.raises(ValueError, match="more than 1 value"):
        m([c[:1, :1, :1] for c in cs], layout="nhwc")
    m.eval()
    assert m([c[:1, :1, :1] for c in cs], layout="nhwc")[0].shape == (1, 1, 1, 16)


def _yololite_n(**options):
    meta = zoo_meta("yololite_n", num_classes=3, img_size=64)
    sd = synth_state_dict(meta)
    model = ya.build_model_from_meta(meta)
    model.load_state_dict(sd)
    model.to(DEV)
    if options:
        model.set_context_options(**options)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(DEV)
    return meta, sd, model, x


def _restated(neck, heads, feats):
    """the float64 restatement of eval-mode neck and heads on `feats`, and the bars an fp32 evaluation gets against
    it: per p level and per head level, max(4 x the CPU fp32 restatement's error, 2 fp32 ulps at the largest value)"""
    sd = {k: v.detach().cpu().numpy() for k, v in list(neck.state_dict().items()) + list(heads.state_dict().items())}
    cs = [f.cpu().numpy() for f in feats]
    ks = [int(n[1:]) for n in neck.level_names]
    res = {}
    with torch.no_grad():
        for dt in (torch.float64, torch.float32):
            ps = neck_forward(sd, sd, cs, ks, neck.depth, False, dt)[0]
            ys = [head_forward(sd, sd, p, k, A, heads.num_classes, heads.head_depth, False, dt)[0]
                  for p, k, A in zip(ps, ks, heads.num_anchors_per_level)]
            res[dt] = ([p.contiguous().numpy() for p in ps], [y.numpy() for y in ys])
    out = []
    for which in (0, 1):
        out.append([(r64, bar(np.abs(r32.astype(np.float64) - r64).max(), np.abs(r64).max()))
                    for r64, r32 in zip(res[torch.float64][which], res[torch.float32][which])])
    return out


def _check_against_executor(model, neck, heads, x, check=True, tag=""):
    """the rule of test_neck_train_gpu.py: the difference to the executor is at most 2 x the bar an fp32 CPU
    restatement earns against float64.  check=False: print only"""
    feats = model.features(x)
    with torch.no_grad():
        ps = neck.eval()(feats, layout="nhwc")
        ours = heads.eval()(ps, layout="nhwc")
    theirs, pyr = model(x), model.pyramid(x)
    pbars, ybars = _restated(neck, heads, feats)
    for what, mine, other, bars in (("p", ps, pyr, pbars), ("y", ours, theirs, ybars)):
        for li, (o, t, (r64, b)) in enumerate(zip(mine, other, bars)):
            eo = np.abs(o.cpu().numpy().astype(np.float64) - r64).max()
            diff = (o - t).abs().max().item()
            print(f"{tag}{what} L{li}: device err {eo:.3e}  diff to the executor {diff:.3e}  bar {b:.3e}")
            assert o.shape == t.shape
            if check:
                assert diff <= 2 * b, (what, li, diff, b)


def test_eval_neck_and_heads_agree_with_the_executor():
    """yololite_n at 64 x 64, B = 2.  The executor runs with option winograd 0, so both sides sum the same products; the
    difference under its default Winograd setting is printed, not asserted"""
    meta, sd, model, x = _yololite_n(winograd=0)
    before = [o.clone() for o in model(x)]
    feats = model.features(x)
    neck = ya.DetectNeckMS.from_state_dict(meta, sd).to(DEV)
    heads = ya.DetectHeads.from_state_dict(meta, sd).to(DEV)
    assert [tuple(f.shape) for f in feats] == [(2, s, s, c) for s, c in zip((8, 4, 2), neck.in_channels)]
    _check_against_executor(model, neck, heads, x)
    for a, b in zip(before, model(x)):                      # the executor's own contexts behave as before
        assert torch.equal(a, b)
    _, _, default, _ = _yololite_n()
    _check_against_executor(default, neck, heads, x, check=False, tag="default winograd: ")


def test_twenty_steps_fit_one_batch_as_the_float64_loop_does():
    ref = np.load(FIXTURE)["e2e/losses"]
    L0_ref, L20_ref = float(ref[0]), float(ref[-1])
    inputs, hinputs = case_inputs(E2E), head_inputs(E2E)
    neck = _neck(E2E, inputs)
    heads = ya.DetectHeads(E2E["F"], E2E["C"], E2E["A"], E2E["head_depth"])
    hsd = {}
    for lv in hinputs:
        hsd.update(lv["params"]); hsd.update(lv["buffers"])
    heads.load_state_dict({k: torch.as_tensor(v) for k, v in hsd.items()})
    heads.to(DEV).train()
    start = {n: p.detach().clone() for n, p in neck.named_parameters()}
    feats = [torch.from_numpy(lv["c"]).to(DEV) for lv in inputs]
    crit = ya.LossAF(E2E["C"], E2E["img_size"], grad=True)
    params = list(neck.parameters()) + list(heads.parameters())
    fts = ya.FusedTrainStep(params, optimizer="sgd", amp=False, lr=E2E["lr"], momentum=E2E["momentum"], nesterov=False,
                            weight_decay=0.0)
    tg = _targets(E2E)
    losses = []
    for _ in range(E2E["steps"]):
        fts.zero_grad()
        loss, _ = crit(heads(neck(feats, layout="nhwc"), layout="nhwc"), tg)
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
        fts.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(crit(heads(neck(feats, layout="nhwc"), layout="nhwc"), tg)[0]))
    L0, L20 = losses[0], losses[-1]
    print(f"L0 {L0:.6f} (float64 loop {L0_ref:.6f})  L20 {L20:.6f} (float64 loop {L20_ref:.6f})")
    assert L0_ref - L20_ref >= 0.2 * L0_ref
    assert L20 <= L0 - 0.5 * (L0 - L20_ref)
    same = [n for n, p in neck.named_parameters() if torch.equal(p, start[n])]
    assert not same, same                                  # every lateral and every smooth parameter has moved
    assert int(neck.smooth3[1].num_batches_tracked) == 3 + E2E["steps"] + 1


def test_trained_neck_and_heads_round_trip_through_a_checkpoint():
    meta, sd, model, x = _yololite_n(winograd=0)
    neck = ya.neck_for(meta, sd).to(DEV).train()
    assert type(neck) is ya.DetectNeckMS
    heads = ya.DetectHeads.from_state_dict(meta, sd).to(DEV).train()
    crit = ya.LossAF(3, 64, grad=True)
    fts = ya.FusedTrainStep(list(neck.parameters()) + list(heads.parameters()), optimizer="sgd", amp=False, lr=0.01)
    tg = _targets(dict(E2E, B=2))
    feats = model.features(x)
    for _ in range(2):
        fts.zero_grad()
        crit(heads(neck(feats, layout="nhwc"), layout="nhwc"), tg)[0].backward()
        fts.step()
    merged = dict(sd)
    for mod in (neck, heads):
        merged.update({k: v.detach().cpu().numpy() for k, v in mod.state_dict().items()})
    assert set(sd) <= set(merged)
    changed = [k for k in sd if not np.array_equal(np.asarray(sd[k]), merged[k])]
    assert changed and all(k.startswith(("lateral", "smooth", "head")) for k in changed)
    assert any(k.startswith("lateral") for k in changed) and any(k.startswith("smooth") for k in changed)
    m2 = ya.build_model_from_meta(copy.deepcopy(meta))
    m2.load_state_dict(merged)
    m2.to(DEV)
    m2.set_context_options(winograd=0)
    _check_against_executor(m2, neck, heads, x)
