"""LossAF on the device (yl_loss_af through ctypes, lossops.LossAF / HipContext.loss_af) against the reference's own
numbers (tests/golden/loss_af.npz, produced by running the reference in fp32 and in fp64) and against the numpy
restatement held to them (tests/_lossaf_np.py).

Tolerance (per component, against the fp64 reference): 4 x the reference's own fp32 error on the case, with a floor of
B + 2 fp32 ulps at the value (the batch result is an fp32 sum of B per-image fp32 means).  The assignment is compared
exactly.  Measured on MI355X (profiles/loss_af_parity.json): every case inside the bar; the largest device error relative
to 4 x err32 is 0.90 (conflict / box: 1.6e-7 against a reference fp32 error of 4.6e-8, floor 4.8e-7)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import yololite_amd as ya
from _lossaf_cases import case_inputs, load_cases, make_levels
from _lossaf_np import loss_af

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CASES, NPZ = load_cases()
NAMES = [c["name"] for c in CASES]
KEYS = ("box", "obj", "cls")


def _tol(ref64, err32, B):
    ref64, err32 = np.asarray(ref64, np.float64), np.asarray(err32, np.float64)
    return np.maximum(4.0 * err32, (B + 2) * np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64))


def _targets(gt, lab, off):
    return [{"boxes": gt[off[b]:off[b + 1]], "labels": lab[off[b]:off[b + 1]]} for b in range(len(off) - 1)]


def _dev(levels):
    return [torch.from_numpy(l).cuda() for l in levels]


def _margin(levels, gt, lab, off, C, S, kw, b, n, t_dev, t_ref):
    """the fp64 margins of a contested choice: for the device's and the restatement's box of anchor n of image b, the
    anchor's cost and the selection boundary of that box's column (its dynamic_k-th and next smallest costs)"""
    r = loss_af(levels, gt, lab, off, C, S, keep_costs=True, **kw)
    cost, dyn = r["costs"][b]
    out = [f"image {b} anchor {n}: device box {t_dev}, restatement box {t_ref}"]
    for t in (t_dev, t_ref):
        if t >= 0:
            j = int(t - off[b])
            col = np.sort(cost[:, j])
            k = int(dyn[j])
            out.append(f"box {t}: cost[anchor] {cost[n, j]!r}, dynamic_k {k}, k-th smallest {col[k - 1]!r}, next {col[k]!r}")
    return "; ".join(out)


def _check(crit, levels, gt, lab, off, want, err32, B, what):
    dl, tg = _dev(levels), _targets(gt, lab, off)
    loss, d = crit(dl, tg)
    got = np.array([d[k] for k in KEYS], np.float64)
    ref = np.array([want[k] for k in KEYS], np.float64)
    tol = _tol(ref, err32, B)
    print(what, "device error", np.abs(got - ref), "allowed", tol, "err32", err32)
    asg = crit.assign(dl, tg).cpu().numpy()
    bad = np.argwhere(asg != want["assign"])
    assert len(bad) == 0, f"{what}: {len(bad)} anchors assigned differently, first: " + \
        _margin(levels, gt, lab, off, crit.nc, crit.img_size, want["kw"], int(bad[0][0]), int(bad[0][1]),
                int(asg[tuple(bad[0])]), int(want["assign"][tuple(bad[0])]))
    assert (np.abs(got - ref) <= tol).all(), (what, got, ref, np.abs(got - ref), tol)
    assert abs(d["pos"] - want["pos"]) <= 1e-6
    assert float(loss.cpu()[0]) == float(np.float32(np.float32(np.float32(d["box"]) + np.float32(d["obj"])) + np.float32(d["cls"])))
    return got, ref


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_fixture_case(case):
    levels, gt, lab, off, kw = case_inputs(case, NPZ)
    n, B = case["name"], case["batch"]
    r64 = loss_af(levels, gt, lab, off, case["num_classes"], case["img_size"], **kw)
    ref64, ref32 = NPZ[n + "/ref64"], NPZ[n + "/ref32"]
    want = {"box": ref64[0], "obj": ref64[1], "cls": ref64[2], "pos": ref64[3], "assign": r64["assign"], "kw": kw}
    crit = ya.LossAF(case["num_classes"], case["img_size"], **kw)
    got, ref = _check(crit, levels, gt, lab, off, want, np.abs(ref32[:3] - ref64[:3]), B, n)
    # the raw targets in their own format and key go through the package's sniffing to the same numbers
    raw = [{t["key"]: torch.tensor(t["boxes"], dtype=torch.float32).reshape(-1, 4), "labels": torch.tensor(t["labels"])}
           for t in case["targets"]]
    _, d2 = crit(_dev(levels), raw)
    assert [d2[k] for k in KEYS] == [float(np.float32(v)) for v in got]


@pytest.mark.parametrize("name", ["crowded", "modes_v8_softplus", "weights", "c80"])
def test_order_and_batch_independence(name):
    case = CASES[NAMES.index(name)]
    levels, gt, lab, off, kw = case_inputs(case, NPZ)
    dl, tg = _dev(levels), _targets(gt, lab, off)
    crit = ya.LossAF(case["num_classes"], case["img_size"], **kw)
    _, d = crit(dl, tg)
    per = crit.per_image(dl, tg).cpu().numpy()
    s = np.zeros(3, np.float32)
    for row in per:                                       # image order, fp32
        s = (s + row).astype(np.float32)
    assert [float(v) for v in s] == [d[k] for k in KEYS]
    _, d2 = crit(dl, tg)
    assert d2 == d and np.array_equal(crit.per_image(dl, tg).cpu().numpy(), per)          # run to run
    assert torch.equal(crit.assign(dl, tg), crit.assign(dl, tg))
    for b in range(case["batch"]):                        # an image alone == the image in its batch
        one = crit.per_image([l[b:b + 1].contiguous() for l in dl], tg[b:b + 1]).cpu().numpy()
        assert np.array_equal(one[0], per[b]), (b, one, per[b])
    rev = crit.per_image([l.flip(0).contiguous() for l in dl], tg[::-1]).cpu().numpy()
    assert np.array_equal(rev[::-1], per)


def test_full_size_edge_n_640_batch_64():
    """levels from the real forward, 0-60 seeded boxes per image, against the restatement (fp64; err32 from its fp32 run)"""
    from yololite_amd.program import synth_state_dict, zoo_meta
    S, B, C = 640, 64, 80
    meta = zoo_meta("edge_n", num_classes=C, img_size=S)
    model = ya.build_model_from_meta(meta)
    model.load_state_dict(synth_state_dict(meta, seed=2, head_noise=2.0))
    model.to("cuda:0")
    x = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(5))
    outs = model(x.cuda())
    rs = np.random.RandomState(77)
    bx, lb, off = [], [], [0]
    for b in range(B):
        n = int(rs.randint(0, 61))
        c = rs.uniform(20, S - 20, (n, 2))
        wh = np.exp(rs.uniform(np.log(6), np.log(400), (n, 2)))
        bx.append(np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, S - 1))
        lb.append(rs.randint(0, C, n)); off.append(off[-1] + n)
    gt = np.concatenate(bx).astype(np.float32); lab = np.concatenate(lb).astype(np.int32); off = np.asarray(off, np.int32)
    levels = [o.cpu().numpy() for o in outs]
    r64 = loss_af(levels, gt, lab, off, C, S)
    r32 = loss_af(levels, gt, lab, off, C, S, dtype=np.float32)
    err32 = np.abs(np.array([r32[k] - r64[k] for k in KEYS]))
    r64["kw"] = {}
    crit = ya.LossAF(C, S, ctx=model._ctx_for(S))
    _check(crit, levels, gt, lab, off, r64, err32, B, "edge_n_640_b64")
    per = crit.per_image(outs, _targets(gt, lab, off)).cpu().numpy().astype(np.float64)
    ptol = np.maximum(4 * np.abs(r32["per_image"] - r64["per_image"]), 3 * np.spacing(np.abs(r64["per_image"]).astype(np.float32)))
    print("per-image worst error / allowed", np.max(np.abs(per - r64["per_image"]) / ptol))
    assert (np.abs(per - r64["per_image"]) <= ptol).all()


@pytest.mark.parametrize("name,topk", [("crowded", 20), ("p2_levels", 64), ("c80", 5)])
def test_every_anchor_valid_prunes_the_candidate_list(name, topk):
    """a radius and area gate that admit every anchor of every level: far more candidates per box than the kernel's LDS
    list holds, so it is pruned on the way (several times on the P2 level set) -- same assignment, same numbers"""
    case = CASES[NAMES.index(name)]
    levels, gt, lab, off, kw = case_inputs(case, NPZ)
    kw = dict(kw, center_radius_cells=1000.0, area_cells_min=1e-6, area_cells_max=1e12, topk_limit=topk)
    C, S = case["num_classes"], case["img_size"]
    r64 = loss_af(levels, gt, lab, off, C, S, **kw)
    r32 = loss_af(levels, gt, lab, off, C, S, dtype=np.float32, **kw)
    assert np.array_equal(r32["assign"], r64["assign"])            # the input has no near-tie of its own
    r64["kw"] = kw
    _check(ya.LossAF(C, S, **kw), levels, gt, lab, off, r64, np.abs(np.array([r32[k] - r64[k] for k in KEYS])),
           case["batch"], name + "_all_valid")


def test_refusals_and_optional_outputs():
    case = CASES[NAMES.index("modes_v8_softplus")]
    levels, gt, lab, off, kw = case_inputs(case, NPZ)
    dl, tg = _dev(levels), _targets(gt, lab, off)
    crit = ya.LossAF(case["num_classes"], case["img_size"], **kw)
    g = [l.clone().requires_grad_(True) for l in dl]
    with pytest.raises(ya.YoloLiteHipError, match="forward only"):
        crit(g, tg)
    two = ya.LossAF(case["num_classes"], case["img_size"])
    with pytest.raises(ya.YoloLiteHipError, match="one anchor per cell"):
        two([torch.cat([l, l], 1) for l in dl], tg)
    # NULL optional outputs, straight at the context
    ctx = crit._context(dl)
    d = torch.from_numpy(np.concatenate([gt.reshape(-1).view(np.int32), lab, off])).cuda()
    T = len(lab)
    a = (d[:4 * T].view(torch.float32).view(T, 4), d[4 * T:5 * T], d[5 * T:])
    o1, p1, a1 = ctx.loss_af(dl, *a, crit.cfg)
    o2, p2, a2 = ctx.loss_af(dl, *a, crit.cfg, want_per_image=True, want_assign=True)
    assert p1 is None and a1 is None and p2.shape == (3, 3) and a2.shape == (3, ctx.N) and torch.equal(o1, o2)
    # T = 0: only the hard-negative term of every image
    e = CASES[NAMES.index("empty_batch")]
    levels, gt, lab, off, kw = case_inputs(e, NPZ)
    _, dd = ya.LossAF(e["num_classes"], e["img_size"])(_dev(levels), [{"boxes": np.zeros((0, 4)), "labels": []}, {"labels": []}])
    assert dd["box"] == 0.0 and dd["cls"] == 0.0 and dd["pos"] == 0.0 and dd["obj"] > 0.0


def test_cli_val_loss(tmp_path, golden_dir):
    """tools/evaluate.py --val-loss on a labelled folder == the restatement on the same levels and labels, accumulated as
    the reference's validation loop does; without the flag the summary has no such key and is otherwise the same."""
    from PIL import Image
    from yololite_amd.program import synth_state_dict, zoo_meta
    img = np.load(os.path.join(golden_dir, "infer_main.npz"))["img_sq"]         # the golden image, S x S
    S = int(img.shape[0])
    # a seeded edge_n whose heads give ordinary logits (the golden checkpoint's are in the hundreds: every predicted
    # side under- or overflows in fp32, which says nothing about the loss)
    meta = zoo_meta("edge_n", num_classes=3, img_size=S)
    meta = dict(meta, config=dict(meta.get("config") or {}, loss={"lambda_box": 4.0, "topk_limit": 10}))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth_state_dict(meta, seed=2, head_noise=2.0).items()}
    ck = str(tmp_path / "tiny.pt")
    torch.save({"state_dict": sd, "meta": meta}, ck)
    ds = tmp_path / "ds"
    (ds / "images").mkdir(parents=True); (ds / "labels").mkdir()
    labels = ["0 0.5 0.5 0.4 0.4\n1 0.25 0.3 0.2 0.2\n", "2 0.6 0.6 0.5 0.3\n", "0 0.3 0.7 0.1 0.1\n1 0.5 0.5 0.9 0.9\n"]
    for n, lab in enumerate(labels):
        Image.fromarray(np.roll(img, 7 * n, axis=1)[..., ::-1]).save(str(ds / "images" / f"im{n}.png"))
        (ds / "labels" / f"im{n}.txt").write_text(lab)
    outs = {}
    for flag in ("--val-loss", None):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "evaluate.py"), "--weights", ck, "--test_folder",
                            str(ds), "--batch_size", "2"] + ([flag] if flag else []), cwd=str(tmp_path),
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[flag] = json.loads(r.stdout.splitlines()[0])
    plain, withl = outs[None], outs["--val-loss"]
    assert "val_loss" not in plain
    vl = withl.pop("val_loss")
    drop = lambda d: {k: v for k, v in d.items() if not k.endswith("_ms_per_img")}
    assert drop(plain) == drop(withl)
    assert json.loads((tmp_path / "runs" / "evaluate" / "1" / "val_loss.json").read_text()) == vl
    # the same computation here: the CLI's pre-processing and forward, the restatement for the loss
    from tools.infer import imread_bgr
    model, names, _ = ya.load_model_names_imgsize_from_ckpt(ck, torch.device("cuda:0"))
    ctx = model._ctx_for(S)
    paths = sorted(str(p) for p in (ds / "images").glob("*"))
    kw = dict(lambda_box=4.0, topk_limit=10, lambda_cls=1.0)
    vb = vo = vc = 0.0
    e32 = np.zeros(3)
    for i in range(0, 3, 2):
        chunk = paths[i:i + 2]
        x, bms = ya.preprocess_batch(ctx, [imread_bgr(p) for p in chunk], letterbox=True, norm="albumentations")
        levels = [o.cpu().numpy() for o in ctx.forward(x)]
        bx, lb, off = [], [], [0]
        for j, p in enumerate(chunk):
            rows = np.loadtxt(str(ds / "labels" / (os.path.splitext(os.path.basename(p))[0] + ".txt")), ndmin=2)
            padx, pady, scale, w0, h0 = bms[j]
            for r_ in rows:
                bx.append([(r_[1] - r_[3] / 2) * w0 * scale + padx, (r_[2] - r_[4] / 2) * h0 * scale + pady,
                           (r_[1] + r_[3] / 2) * w0 * scale + padx, (r_[2] + r_[4] / 2) * h0 * scale + pady])
                lb.append(int(r_[0]))
            off.append(len(bx))
        a = (np.asarray(bx, np.float32), np.asarray(lb), np.asarray(off))
        r64 = loss_af(levels, *a, len(names), S, **kw)
        r32 = loss_af(levels, *a, len(names), S, dtype=np.float32, **kw)
        vb += r64["box"] / len(chunk); vo += r64["obj"] / len(chunk); vc += r64["cls"] / len(chunk)
        e32 += np.abs([r32[k] - r64[k] for k in KEYS]) / len(chunk)
    want = np.array([vb, vo, vc]) / 2
    got = np.array([vl[k] for k in KEYS])
    tol = _tol(want, e32 / 2, 2)
    print("cli val_loss", vl, "restatement", want, "allowed", tol)
    assert (np.abs(got - want) <= tol).all()
    assert abs(vl["total"] - got.sum()) <= 1e-12 and 0.0 <= vl["pos"] <= 1.0
