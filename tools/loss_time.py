#!/usr/bin/env python3
"""Time the validation loss on the device (yl_loss_af through lossops.LossAF): edge_n at 640, batch 64, level tensors
from the real forward on seeded images, 8 / 40 / 128 seeded boxes per image.  Warm, median of --repeat runs:
  device_ms  HIP events around the call on the context (one memset + three kernels)
  wall_ms    LossAF(preds, targets) as a user calls it: target sniffing and packing on the host, one upload, the
             kernels, and the copy of the four floats back
With --grad the loss's backward is timed as well, per box count:
  train_device_ms     yl_loss_af_train: the forward that keeps the backward's state (assign, sel)
  backward_device_ms  yl_loss_af_backward: one kernel that writes every level gradient once, 10 calls queued back to
                      back per sample; backward_write_GBps is the gradient tensors' bytes over that time (one write of
                      them is the kernel's floor)
  grad_wall_ms        LossAF(grad=True)(preds, targets)[0].backward() as a training loop calls it
and with --grad-parity F the gradient fixture's cases (tests/golden/loss_af_grad.npz) are run and, per case and column
group, the device error against the reference's fp64 gradient, the bar (4 x the reference's fp32 error, floor 2 ulps)
and their ratio are written to F.
Prints one JSON line.  With --parity F the fixture cases of tests/golden/loss_af.npz are run as well and their
device errors against the reference's fp64 numbers written to F (per case: ref64, err32, device error).

    python tools/loss_time.py [--boxes 8,40,128] [--batch 64] [--repeat 30] [--out F] [--parity F] [--grad]
                              [--grad-parity F]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def seeded_boxes(rs, n, S, C):
    import numpy as np
    c = rs.uniform(20, S - 20, (n, 2))
    wh = np.exp(rs.uniform(np.log(8), np.log(300), (n, 2)))
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, S - 1).astype(np.float32), rs.randint(0, C, n)


BACK_TO_BACK = 10


def time_grad(ctx, outs, dev_args, targets, crit, repeat):
    import numpy as np
    import torch
    one = torch.ones(1, device=outs[0].device)
    nbytes = sum(o.numel() * 4 for o in outs)
    leaves = [o.detach().clone().requires_grad_(True) for o in outs]
    for _ in range(3):
        crit(leaves, targets)[0].backward()
    tr_ms, bw_ms, wall_ms = [], [], []
    for _ in range(repeat):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        e[0].record()
        _, asg, sel = ctx.loss_af_train(outs, *dev_args, crit.cfg)
        e[1].record()
        torch.cuda.synchronize()
        e[2].record()
        for _ in range(BACK_TO_BACK):                          # queued faster than they run: launch latency is hidden
            ctx.loss_af_backward(outs, *dev_args, crit.cfg, asg, sel, one)
        e[3].record()
        torch.cuda.synchronize()
        tr_ms.append(e[0].elapsed_time(e[1])); bw_ms.append(e[2].elapsed_time(e[3]) / BACK_TO_BACK)
        for l in leaves:
            l.grad = None
        t0 = time.perf_counter()
        crit(leaves, targets)[0].backward()
        torch.cuda.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
    bw = float(np.median(bw_ms))
    return {"train_device_ms": round(float(np.median(tr_ms)), 4), "train_device_ms_min": round(float(np.min(tr_ms)), 4),
            "backward_device_ms": round(bw, 4), "backward_device_ms_min": round(float(np.min(bw_ms)), 4),
            "grad_bytes": nbytes, "backward_write_GBps": round(nbytes / (bw * 1e-3) / 1e9, 1),
            "grad_wall_ms": round(float(np.median(wall_ms)), 4)}


def grad_parity(path):
    import numpy as np
    import torch
    import yololite_amd as ya
    from _lossaf_grad_cases import GROUPS, fixture_grad, grad_case_inputs, grad_cases, group_slices, load_grad_fixture
    cases, npz = grad_cases()
    z = load_grad_fixture()
    rows = []
    for c in cases:
        n = c["name"]
        levels, gt, lab, off, kw = grad_case_inputs(c, npz)
        tg = [{"boxes": gt[off[b]:off[b + 1]], "labels": lab[off[b]:off[b + 1]]} for b in range(c["batch"])]
        dl = [torch.from_numpy(l).cuda().requires_grad_(True) for l in levels]
        ya.LossAF(c["num_classes"], c["img_size"], grad=True, **kw)(dl, tg)[0].backward()
        g = np.concatenate([p.grad.cpu().numpy().reshape(p.shape[0], -1, p.shape[-1]) for p in dl], 1).astype(np.float64)
        ref = fixture_grad(z, n, g.shape)
        row = {"case": n, "batch": c["batch"]}
        for i, (k, sl) in enumerate(group_slices(c["num_classes"]).items()):
            assert k == GROUPS[i]
            e32, m64 = float(z[n + "/e32"][i]), float(z[n + "/max64"][i])
            bar = max(4.0 * e32, 2.0 * float(np.spacing(np.float32(m64))))
            err = float(np.abs(g[..., sl] - ref[..., sl]).max()) if g[..., sl].size else 0.0
            row[k] = {"max_g64": m64, "err32": e32, "device_error": err, "bar": bar, "ratio": err / bar if bar else 0.0}
        rows.append(row)
    with open(path, "w") as f:
        json.dump(rows, f, indent=1)
    return max(r[k]["ratio"] for r in rows for k in GROUPS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", default="8,40,128")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--out", default="")
    ap.add_argument("--parity", default="")
    ap.add_argument("--grad", action="store_true")
    ap.add_argument("--grad-parity", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    import yololite_amd as ya
    from yololite_amd.program import synth_state_dict, zoo_meta

    S, B, C = 640, args.batch, 80
    meta = zoo_meta("edge_n", num_classes=C, img_size=S)
    model = ya.build_model_from_meta(meta)
    model.load_state_dict(synth_state_dict(meta, seed=2, head_noise=2.0))
    model.to("cuda:0")
    ctx = model._ctx_for(S)
    outs = model(torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(5)).cuda())
    crit = ya.LossAF(C, S, ctx=ctx)
    res = {"gpu": torch.cuda.get_device_name(0), "model": "edge_n", "img_size": S, "batch": B, "anchors": ctx.N,
           "repeat": args.repeat, "runs": []}
    for nb in (int(v) for v in args.boxes.split(",")):
        rs = np.random.RandomState(100 + nb)
        targets = []
        for _ in range(B):
            bx, lb = seeded_boxes(rs, nb, S, C)
            targets.append({"boxes": bx, "labels": lb})
        from yololite_amd.lossops import pack_targets
        gt, lab, off = pack_targets(targets, S, C)
        d = torch.from_numpy(np.concatenate([gt.reshape(-1).view(np.int32), lab, off])).cuda()
        T = len(lab)
        dev_args = (d[:4 * T].view(torch.float32).view(T, 4), d[4 * T:5 * T], d[5 * T:])
        for _ in range(3):
            crit(outs, targets)
        dev_ms, wall_ms = [], []
        for _ in range(args.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            ctx.loss_af(outs, *dev_args, crit.cfg)
            e1.record()
            torch.cuda.synchronize()
            dev_ms.append(e0.elapsed_time(e1))
            t0 = time.perf_counter()
            _, dd = crit(outs, targets)
            wall_ms.append((time.perf_counter() - t0) * 1e3)
        res["runs"].append({"boxes_per_image": nb, "boxes": T, "device_ms": round(float(np.median(dev_ms)), 4),
                            "device_ms_min": round(float(np.min(dev_ms)), 4), "wall_ms": round(float(np.median(wall_ms)), 4),
                            "device_us_per_image": round(float(np.median(dev_ms)) * 1e3 / B, 3),
                            "loss": {k: dd[k] for k in ("box", "obj", "cls", "pos")}})
        if args.grad:
            res["runs"][-1].update(time_grad(ctx, outs, dev_args, targets, ya.LossAF(C, S, ctx=ctx, grad=True), args.repeat))
    if args.parity:
        from _lossaf_cases import case_inputs, load_cases
        cases, z = load_cases()
        rows = []
        for c in cases:
            levels, gt, lab, off, kw = case_inputs(c, z)
            tg = [{"boxes": gt[off[b]:off[b + 1]], "labels": lab[off[b]:off[b + 1]]} for b in range(c["batch"])]
            _, dd = ya.LossAF(c["num_classes"], c["img_size"], **kw)([torch.from_numpy(l).cuda() for l in levels], tg)
            r64, r32 = z[c["name"] + "/ref64"], z[c["name"] + "/ref32"]
            rows.append({"case": c["name"], "batch": c["batch"], "ref64": [float(v) for v in r64[:3]],
                         "err32": [float(abs(a - b)) for a, b in zip(r32[:3], r64[:3])],
                         "device_error": [float(abs(dd[k] - r)) for k, r in zip(("box", "obj", "cls"), r64[:3])]})
        with open(args.parity, "w") as f:
            json.dump(rows, f, indent=1)
    if args.grad_parity:
        res["grad_parity_worst_ratio"] = round(grad_parity(args.grad_parity), 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
