"""LossAF's backward on the device (yl_loss_af_train / yl_loss_af_backward behind lossops.LossAF(grad=True) and torch
autograd) against the reference's own autograd (tests/golden/loss_af_grad.npz: its fp64 gradient, and its fp32 error
as the yardstick) and against the numpy restatement held to it (tests/_lossaf_grad_np.py).

Tolerance, per case and column group (box 0-3, obj 4, cls 5..): max|g_dev - g64| <= 4 x the reference's own fp32 error
e32 of that case and group, with a floor of 2 fp32 ulps at the group's max|g64| -- the forward test's rule.  Outside the
positives' and selected negatives' rows, and outside their columns, the gradient must be +0.0 exactly.  Measured on
MI355X (profiles/loss_af_grad_parity.json): every case inside the bar; the largest device error relative to the bar is
0.18 (c80 / cls: 4.5e-10 against a reference fp32 error of 6.1e-10, bar 2.5e-9)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import yololite_amd as ya
from _lossaf_cases import make_levels
from _lossaf_grad_cases import GROUPS, fixture_grad, grad_case_inputs, grad_cases, group_slices, load_grad_fixture
from _lossaf_grad_np import loss_af_grad
from _lossaf_np import loss_af

CASES, NPZ = grad_cases()
NAMES = [c["name"] for c in CASES]
Z = load_grad_fixture()


def _targets(gt, lab, off):
    return [{"boxes": gt[off[b]:off[b + 1]], "labels": lab[off[b]:off[b + 1]]} for b in range(len(off) - 1)]


def _flat(grads):
    return np.concatenate([g.reshape(g.shape[0], -1, g.shape[-1]) for g in grads], 1)


def _backward(crit, levels, tg, scale=None):
    """-> loss, dict, gradient [B,N,E] (numpy) of fresh leaf tensors made from `levels` (numpy or torch, on the host)"""
    dl = [torch.as_tensor(l).cuda().requires_grad_(True) for l in levels]
    loss, d = crit(dl, tg)
    assert loss.shape == (1,) and loss.dtype == torch.float32 and loss.grad_fn is not None
    (loss if scale is None else scale * loss).backward()
    assert all(p.grad.shape == p.shape and p.grad.dtype == p.dtype for p in dl)
    return loss, d, _flat([p.grad.float().cpu().numpy() for p in dl])


@functools.lru_cache(maxsize=None)
def _case_run(name):
    case = CASES[NAMES.index(name)]
    levels, gt, lab, off, kw = grad_case_inputs(case, NPZ)
    crit = ya.LossAF(case["num_classes"], case["img_size"], grad=True, **kw)
    tg = _targets(gt, lab, off)
    loss, d, g = _backward(crit, levels, tg)
    g.setflags(write=False)
    return case, levels, tg, kw, loss, d, g


def _is_pos_zero(a):
    return bool(np.all(a == 0) and not np.signbit(a).any())


def _bar(e32, m64):
    return max(4.0 * float(e32), 2.0 * float(np.spacing(np.float32(abs(m64)))))


def _check_against(g, ref, pos, neg, C, e32, m64, what):
    """sets exact, +0.0 outside them, values inside the 4 x e32 bar; -> {group: (error, bar)}"""
    rows_p = np.zeros(g.shape[:2], bool)
    rows_n = np.zeros(g.shape[:2], bool)
    rows_p[pos[:, 0], pos[:, 1]] = True
    rows_n[neg[:, 0], neg[:, 1]] = True
    assert _is_pos_zero(g[~(rows_p | rows_n)]), what + ": a row outside the positives and selected negatives is not +0.0"
    assert _is_pos_zero(g[rows_n][:, :4]) and _is_pos_zero(g[rows_n][:, 5:]), what + ": a negative's other columns"
    assert _is_pos_zero(g[rows_p][:, 5 + C:]), what + ": columns past the classes"
    assert (g[rows_n][:, 4] != 0).all(), what + ": a selected negative has no gradient"
    out = {}
    for k, sl in group_slices(C).items():
        i = GROUPS.index(k)
        err = float(np.abs(g[..., sl].astype(np.float64) - ref[..., sl]).max()) if g[..., sl].size else 0.0
        out[k] = (err, _bar(e32[i], m64[i]))
        print(what, k, "device error", err, "bar", out[k][1], "ratio", err / out[k][1] if out[k][1] else 0.0,
              "e32", float(e32[i]), "max|g64|", float(m64[i]))
    for k, (err, bar) in out.items():
        assert err <= bar, (what, k, err, bar)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_fixture_case(name):
    case, levels, tg, kw, loss, d, g = _case_run(name)
    assert tuple(g.shape) == tuple(Z[name + "/shape"])
    crit = ya.LossAF(case["num_classes"], case["img_size"], **kw)
    asg = crit.assign([torch.from_numpy(l).cuda() for l in levels], tg).cpu().numpy()
    assert np.array_equal(np.argwhere(asg >= 0).astype(np.int32), Z[name + "/pos"])
    _check_against(g, fixture_grad(Z, name, g.shape), Z[name + "/pos"], Z[name + "/neg"], case["num_classes"],
                   Z[name + "/e32"], Z[name + "/max64"], name)


@pytest.mark.parametrize("name", ["modes_v8_softplus", "c80", "empty_batch", "crowded"])
def test_loss_values_are_the_plain_forwards(name):
    case, levels, tg, kw, loss, d, _ = _case_run(name)
    plain = ya.LossAF(case["num_classes"], case["img_size"], **kw)
    dl = [torch.from_numpy(l).cuda() for l in levels]
    loss0, d0 = plain(dl, tg)
    assert d == d0 and torch.equal(loss.detach(), loss0) and loss0.grad_fn is None
    # grad=True without an input that requires grad, or under no_grad: today's forward
    crit = ya.LossAF(case["num_classes"], case["img_size"], grad=True, **kw)
    loss1, d1 = crit(dl, tg)
    assert d1 == d0 and torch.equal(loss1, loss0) and loss1.grad_fn is None
    with torch.no_grad():
        loss2, d2 = crit([l.clone().requires_grad_(True) for l in dl], tg)
    assert d2 == d0 and torch.equal(loss2, loss0) and loss2.grad_fn is None
    with pytest.raises(ya.YoloLiteHipError, match="requires grad"):
        crit([l.clone().requires_grad_(True) for l in dl],
             [dict(t, boxes=torch.tensor(np.asarray(t["boxes"]), requires_grad=True)) for t in tg])


def test_autograd_plumbing():
    case, levels, tg, kw, loss, d, g = _case_run("modes_v8_softplus")
    C, S = case["num_classes"], case["img_size"]
    crit = ya.LossAF(C, S, grad=True, **kw)
    # a scaled loss: the scale reaches the kernel as grad_output, the product is rounded once
    _, _, g3 = _backward(crit, levels, tg, scale=3.0)
    want = 3.0 * g.astype(np.float64)
    assert (np.abs(g3 - want) <= 2 * np.spacing(np.abs(want).astype(np.float32))).all() and _is_pos_zero(g3[g == 0])
    # a second backward accumulates into the same .grad
    dl = [torch.from_numpy(l).cuda().requires_grad_(True) for l in levels]
    for _ in range(2):
        crit(dl, tg)[0].backward()
    assert np.array_equal(_flat([p.grad.cpu().numpy() for p in dl]), g + g)
    # inputs that are views of differently laid out tensors receive the gradient in the base's layout
    bases = [torch.from_numpy(l).cuda().permute(0, 1, 4, 2, 3).contiguous().requires_grad_(True) for l in levels]
    views = [b.permute(0, 1, 3, 4, 2) for b in bases]
    assert not views[0].is_contiguous()
    crit(views, tg)[0].backward()
    assert np.array_equal(_flat([b.grad.permute(0, 1, 3, 4, 2).cpu().numpy() for b in bases]), g)
    # fp16 inputs: fp32 arithmetic on the upcast values, the gradient comes back in fp16
    l16 = [torch.from_numpy(l).half() for l in levels]
    _, d32, g32 = _backward(crit, [l.float() for l in l16], tg)
    dl16 = [l.cuda().requires_grad_(True) for l in l16]
    loss16, d16 = crit(dl16, tg)
    loss16.backward()
    assert d16 == d32 and all(p.grad.dtype == torch.float16 for p in dl16)
    assert np.array_equal(_flat([p.grad.cpu().numpy() for p in dl16]), g32.astype(np.float16))
    # an input edited in place between forward and backward is caught by its version counter
    dl = [torch.from_numpy(l).cuda().requires_grad_(True) for l in levels]
    loss_e, _ = crit(dl, tg)
    with torch.no_grad():
        dl[1].mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss_e.backward()


@pytest.mark.parametrize("name", ["crowded", "weights", "c80"])
def test_determinism_and_batch_independence(name):
    case, levels, tg, kw, loss, d, g = _case_run(name)
    crit = ya.LossAF(case["num_classes"], case["img_size"], grad=True, **kw)
    assert np.array_equal(_backward(crit, levels, tg)[2], g)                         # run to run
    for b in range(case["batch"]):                                                    # an image alone
        one = _backward(crit, [l[b:b + 1] for l in levels], tg[b:b + 1])[2]
        assert np.array_equal(one[0], g[b]), b
    rev = _backward(crit, [np.ascontiguousarray(l[::-1]) for l in levels], tg[::-1])[2]
    assert np.array_equal(rev[::-1], g)


def test_seg_layout_mask_columns_are_zero():
    case = CASES[NAMES.index("modes_v8_softplus")]
    _, gt, lab, off, kw = grad_case_inputs(case, NPZ)
    C, S = case["num_classes"], case["img_size"]
    lv8 = make_levels(case["seed"], S, case["sizes"], C, case["batch"], gt, off, extra=8)
    tg = _targets(gt, lab, off)
    g8 = _backward(ya.LossAF(C, S, grad=True, **kw), lv8, tg)[2]
    g0 = _backward(ya.LossAF(C, S, grad=True, **kw), [np.ascontiguousarray(l[..., :5 + C]) for l in lv8], tg)[2]
    assert g8.shape[-1] == 5 + C + 8 and _is_pos_zero(g8[..., 5 + C:])
    assert np.array_equal(g8[..., :5 + C], g0) and np.abs(g0[..., 5:]).max() > 0


def test_ties_select_the_lowest_anchor_indices():
    """all-equal objectness logits (a freshly initialised head): one empty image, one with boxes"""
    case = CASES[NAMES.index("modes_v8_softplus")]
    levels, gt, lab, off, kw = grad_case_inputs(case, NPZ)
    C, S = case["num_classes"], case["img_size"]
    levels = [l[1:3].copy() for l in levels]                       # image 1 has no boxes, image 2 has six
    assert off[2] == off[1] and off[3] > off[2]
    tg = _targets(gt, lab, off)[1:3]
    x = np.float32(-2.0)
    for l in levels:
        l[..., 4] = x
    kw = dict(kw, lambda_obj=0.7)
    g = _backward(ya.LossAF(C, S, grad=True, **kw), levels, tg)[2]
    asg = ya.LossAF(C, S, **kw).assign([torch.from_numpy(l).cuda() for l in levels], tg).cpu().numpy()
    N = asg.shape[1]
    assert (asg[0] < 0).all() and (asg[1] >= 0).sum() > 0
    term = np.float32(0.7) * (1.0 / (1.0 + np.exp(-np.float64(x))))
    for b in range(2):
        pos = asg[b] >= 0
        K = min(max(64, 3 * int(pos.sum())), N - int(pos.sum()))
        want = np.flatnonzero(~pos)[:K]
        got = np.flatnonzero((g[b, :, 4] != 0) & ~pos)
        assert np.array_equal(got, want), (b, K, got[:5], want[:5])
        s = g[b, want, 4].astype(np.float64).sum()
        print("image", b, "K", K, "sum", s, "lambda_obj * sigmoid", term)
        assert abs(s - term) <= K * np.spacing(np.float32(term / K))


def test_every_anchor_valid_bounded_candidate_list():
    """crowded with a radius and area gate that admit every anchor (the candidate list in LDS is pruned on the way),
    against the numpy restatement: sets exact, values by the 4 x rule with e32 from the restatement's own fp32 run"""
    case = CASES[NAMES.index("crowded")]
    levels, gt, lab, off, kw = grad_case_inputs(case, NPZ)
    kw = dict(kw, center_radius_cells=1000.0, area_cells_min=1e-6, area_cells_max=1e12)
    C, S = case["num_classes"], case["img_size"]
    a64 = loss_af(levels, gt, lab, off, C, S, **kw)["assign"]
    a32 = loss_af(levels, gt, lab, off, C, S, dtype=np.float32, **kw)["assign"]
    assert np.array_equal(a32, a64)                                # the input has no near-tie of its own
    r64 = loss_af_grad(levels, gt, lab, off, C, S, assign=a64, **kw)
    r32 = loss_af_grad(levels, gt, lab, off, C, S, dtype=np.float32, assign=a32, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(r32["neg"], r64["neg"]))
    sl = group_slices(C)
    e32 = [np.abs(r32["grad"][..., sl[k]].astype(np.float64) - r64["grad"][..., sl[k]]).max() for k in GROUPS]
    m64 = [np.abs(r64["grad"][..., sl[k]]).max() for k in GROUPS]
    tg = _targets(gt, lab, off)
    g = _backward(ya.LossAF(C, S, grad=True, **kw), levels, tg)[2]
    asg = ya.LossAF(C, S, **kw).assign([torch.from_numpy(l).cuda() for l in levels], tg).cpu().numpy()
    assert np.array_equal(asg, a64)
    pairs = lambda per: np.array([(b, n) for b, idx in enumerate(per) for n in idx], np.int32).reshape(-1, 2)
    _check_against(g, r64["grad"], pairs(r64["pos"]), pairs(r64["neg"]), C, e32, m64, "crowded_all_valid")
