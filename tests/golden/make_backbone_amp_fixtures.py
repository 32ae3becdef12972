#!/usr/bin/env python3
"""Generate tests/golden/backbone_amp.npz from the oracle/backbones.py modules (ConvBnAct, UniversalInvertedResidual; pure
torch, CPU, torch autograd) as make_stem_fixtures.py and make_stage_fixtures.py run them, with one change: every DENSE
convolution (bias-free nn.Conv2d with groups == 1: the stem's 3x3 and every 1x1) computes
tests/_backbone_amp_cases.RoundedConv (x, W and dz rounded to fp16 / bf16, nearest even; the products of the rounded
values in the run's dtype).  The depthwise convolutions, BatchNorm, ReLU and the residual add are the oracle's, unmodified.

    python tests/golden/make_backbone_amp_fixtures.py [--search]

Layout, flip allowance and admission rule are written down in tests/_backbone_amp_cases.py.  --search prints, per case
and precision, the first admitted seed of case seed + 101 j, j < 20 (the AMP_SEEDS table), and writes nothing."""
import argparse
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from _backbone_amp_cases import (AMP_FIXTURE, AMP_STAGE, AMP_STEM, FLIP_RUNS, FLIP_SEED, PRECISIONS, ROUND_LOG, SEED_STEP,  # noqa: E402
                                 SEEDS_PER_CASE, amp_cases, amp_kind, amp_mod, amp_modes, round_to, rounded_dense_convs)
import make_stage_fixtures as stage_gen  # noqa: E402
import make_stem_fixtures as stem_gen  # noqa: E402

OUT = os.environ.get("YL_FIXTURE_OUT") or HERE
torch.set_num_threads(1)                                   # the fp32 runs' sums in one order, whatever the machine's cores


def run(case, inputs, train, dtype, precision, jitter=None):
    """-> ({tensor name: array}, [BatchNorm output in front of each ReLU]) of the rounded model"""
    gen = stem_gen if amp_kind(case) == "stem" else stage_gen
    with rounded_dense_convs(precision, jitter):
        return gen.run_oracle(case, inputs, train, dtype)


def case_run(case, mode, precision):
    """-> (r64, flips, why): why is None if the case is admitted at its seed"""
    inputs = amp_mod(case).case_inputs(case)
    train = mode == "train"
    ROUND_LOG["inputs"] = []
    r64, bn64 = run(case, inputs, train, torch.float64, precision)
    t64, ROUND_LOG["inputs"] = ROUND_LOG["inputs"], []
    runs = [run(case, inputs, train, torch.float32, precision)]
    t32, ROUND_LOG["inputs"] = ROUND_LOG["inputs"], None
    flips = {n: 0.0 for n in r64}
    ROUND_LOG["flips"] = 0
    for j in range(FLIP_RUNS):
        r32, bn32 = run(case, inputs, train, torch.float32, precision, torch.Generator().manual_seed(FLIP_SEED + j))
        runs.append((r32, bn32))
        for n in r64:
            flips[n] = max(flips[n], float(np.abs(np.asarray(r32[n], np.float64) - r64[n]).max()))
    why = None
    if ROUND_LOG["flips"] == 0:                            # the midpoint rule: the allowance holds no flip, so none may be near
        assert len(t64) == len(t32)
        for i, (a64, a32) in enumerate(zip(t64, t32)):
            d = (a32.double() - a64).abs()                     # per element: its own fp32 error, or the tensor's relative one
            e = 4.0 * torch.maximum(d, a64.abs() * float(d.max() / a64.abs().max().clamp_min(1e-300)))
            near = int((round_to(a64 + e, precision) != round_to(a64 - e, precision)).sum())
            if near:
                why = ("rounding input", i, near, "elements within 4 fp32 errors of a midpoint and no flip in the allowance")
    for t, b64 in enumerate(bn64):
        margin = np.abs(b64).min()
        dev = max(np.abs(bn32[t].astype(np.float64) - b64).max() for _, bn32 in runs)
        if any(not np.array_equal(bn32[t] > 0, b64 > 0) for _, bn32 in runs):
            why = (t, "ReLU masks differ")
        elif not (margin >= 1e-5 and margin >= 64 * dev):
            why = (t, float(margin), float(dev))
    return r64, flips, why


def search():
    for case in AMP_STEM + AMP_STAGE:
        for precision in PRECISIONS:
            found = None
            for j in range(SEEDS_PER_CASE):
                c = dict(case, seed=case["seed"] + SEED_STEP * j)
                if all(case_run(c, mode, precision)[2] is None for mode in amp_modes(c)):
                    found = c["seed"]
                    break
            print(f'    ("{case["name"]}", "{precision}"): {found},', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--search", action="store_true")
    if ap.parse_args().search:
        return search()
    arrays = {}
    for case, precision in amp_cases():
        m = amp_mod(case)
        shapes = m.tensor_shapes(case)
        for mode in amp_modes(case):
            r64, flips, why = case_run(case, mode, precision)
            assert why is None, (case["name"], mode, precision, why)      # admission rule: the next seed in AMP_SEEDS
            key = f"{case['name']}/{mode}/{precision}"
            vals, fl, m64s = [], [], []
            assert set(shapes) == set(r64), sorted(set(shapes) ^ set(r64))
            for n, shape in shapes.items():
                v64 = np.asarray(r64[n])
                assert v64.shape == tuple(shape), (n, v64.shape, shape)
                fl.append(flips[n])
                m64s.append(np.abs(v64).max())
                flat = v64.reshape(-1).astype(np.float64)
                idx = m.stored_indices(key, n, shape)
                vals.append(flat if idx is None else flat[idx])
            arrays[key + "/r64"] = np.concatenate(vals)
            arrays[key + "/flip"] = np.asarray(fl, np.float64)
            arrays[key + "/max64"] = np.asarray(m64s, np.float64)
            worst = max(f / max(mx, 1e-300) for f, mx in zip(fl, m64s))
            print(f"{case['name']:8s} {mode:5s} {precision} seed {case['seed']}  worst flip/max64={worst:.1e}")
    path = os.path.join(OUT, os.path.basename(AMP_FIXTURE))
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
