#!/usr/bin/env python3
"""Generate tests/golden/loss_af_grad.npz by RUNNING THE REFERENCE's own LossAF (scripts/loss/loss.py of the reference
checkout, imported unmodified; pure torch, CPU) with level tensors that require grad, and calling backward().

    python tests/golden/make_loss_grad_fixtures.py --reference /path/to/YoloLite-Official-Repo

The inputs are the 19 cases of loss_af_cases.json (regenerated from their seeds by tests/_lossaf_cases.py) plus
orphan_exp_clamp (tests/_lossaf_grad_cases.py).  Every case runs in fp32 and in fp64; the gradients of the level
tensors are flattened and concatenated to [B, N, E] as the reference's own preds_flat.  Per case the archive holds
  pos, neg    [k,2] int32 (image, anchor): the positive anchors (a non-zero gradient outside column 4) and the selected
              hard negatives (column 4 only)
  idx, g64    the non-zero entries of the fp64 gradient: flat index into [B, N, E] and value -- all of them lie in the
              rows of pos and neg; every other entry of the gradient is exactly 0
  e32, max64  per column group (box 0-3, obj 4, cls 5..): the reference's own fp32 error max|g32 - g64| and max|g64|
  gap         the smallest relative gap, over the images, between the K-th and (K+1)-th hard-negative term

Admission rule, asserted for every case (none is dropped): the loss agrees to 1e-5 relative between fp32 and fp64 (the
forward fixture's rule), both precisions have the same positives and the same selected negatives, and gap > 1e-5 --
torch.topk's choice among equal terms is unspecified, so a case on a tie would pin an accident."""
import argparse
import importlib.util
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from _lossaf_grad_cases import GROUPS, grad_case_inputs, grad_cases, group_slices  # noqa: E402

OUT = os.environ.get("YL_FIXTURE_OUT") or HERE


def run_reference(mod, c, levels, gt, lab, off, kw, dtype):
    torch.set_default_dtype(dtype)
    try:
        preds = [torch.from_numpy(l).to(dtype).requires_grad_(True) for l in levels]
        tg = [{"boxes": torch.from_numpy(gt[off[b]:off[b + 1]]).reshape(-1, 4),
               "labels": torch.from_numpy(lab[off[b]:off[b + 1]].astype(np.int64))} for b in range(c["batch"])]
        crit = mod.LossAF(c["num_classes"], c["img_size"], **kw)
        loss, d = crit(preds, tg)
        loss.backward()
        g = np.concatenate([p.grad.numpy().reshape(p.shape[0], -1, p.shape[-1]) for p in preds], 1)
        return np.array([d["box"], d["obj"], d["cls"]], np.float64), g
    finally:
        torch.set_default_dtype(torch.float32)


def sets(g):
    other = np.ones(g.shape[-1], bool)
    other[4] = False
    pos = (g[..., other] != 0).any(-1)
    neg = (g[..., 4] != 0) & ~pos
    return pos, neg


def negative_gap(levels, pos):
    """smallest relative gap between the K-th and (K+1)-th largest BCE(x, 0) of the non-positives, over the images"""
    x = np.concatenate([l.reshape(l.shape[0], -1, l.shape[-1])[..., 4] for l in levels], 1).astype(np.float64)
    gap = np.inf
    for b in range(x.shape[0]):
        v = np.sort(np.maximum(x[b][~pos[b]], 0) + np.log1p(np.exp(-np.abs(x[b][~pos[b]]))))[::-1]
        K = min(max(64, 3 * int(pos[b].sum())), v.size)
        if 0 < K < v.size:
            gap = min(gap, (v[K - 1] - v[K]) / v[K - 1])
    return gap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_loss", os.path.join(a.reference, "scripts", "loss", "loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cases, npz = grad_cases()
    arrays, nnz = {}, 0
    for c in cases:
        n = c["name"]
        levels, gt, lab, off, kw = grad_case_inputs(c, npz)
        l32, g32 = run_reference(mod, c, levels, gt, lab, off, kw, torch.float32)
        l64, g64 = run_reference(mod, c, levels, gt, lab, off, kw, torch.float64)
        rel = np.abs(l32 - l64) / np.maximum(np.abs(l64), 1e-30)
        rel[l32 == l64] = 0.0
        p32, n32 = sets(g32)
        p64, n64 = sets(g64)
        gap = negative_gap(levels, p64)
        # admission rule: change the seed, say so above
        assert rel.max() <= 1e-5, (n, l32, l64)
        assert np.array_equal(p32, p64) and np.array_equal(n32, n64), (n, "sets differ between fp32 and fp64")
        assert gap > 1e-5, (n, gap)
        rows = p64 | n64
        assert not g64[~rows].any() and not g32[~rows].any()
        idx = np.flatnonzero(g64)
        sl = group_slices(c["num_classes"])
        e32 = np.array([np.abs(g32[..., sl[k]].astype(np.float64) - g64[..., sl[k]]).max() if g64[..., sl[k]].size else 0.0
                        for k in GROUPS])
        m64 = np.array([np.abs(g64[..., sl[k]]).max() if g64[..., sl[k]].size else 0.0 for k in GROUPS])
        arrays.update({n + "/pos": np.argwhere(p64).astype(np.int32), n + "/neg": np.argwhere(n64).astype(np.int32),
                       n + "/idx": idx.astype(np.int32), n + "/g64": g64.reshape(-1)[idx], n + "/e32": e32,
                       n + "/max64": m64, n + "/gap": np.float64(gap), n + "/shape": np.asarray(g64.shape, np.int32)})
        nnz += idx.size
        print(f"{n:22s} pos={int(p64.sum()):4d} neg={int(n64.sum()):4d} nnz={idx.size:6d} gap={gap:.1e} "
              f"e32/max64={e32 / np.maximum(m64, 1e-300)}")
    print("non-zero entries:", nnz)
    np.savez_compressed(os.path.join(OUT, "loss_af_grad.npz"), **arrays)


if __name__ == "__main__":
    main()
