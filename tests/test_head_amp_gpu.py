"""DetectHeads in precision "fp16" / "bf16" on the device against tests/golden/head_amp.npz: a2c1, c80 and base in train
mode plus eval for `base`, forward and backward, y, dx, the running statistics and every parameter gradient.

What this test is for is wiring: every one of the six GEMMs rounds, the right operands are used, everything else is the
fp32 code and the backward runs in the forward's mode.  (The kernel's arithmetic is held to the tight bar of
test_head_gemm_amp_gpu.py.)  The bar is max(4 x flip, 2 fp32 ulps): `flip` is what an ulp of difference in a computed
operand does to the reference itself once a rounding flips (tests/_head_amp_cases.py).  The worst error / bar of every
case is written to profiles/head_amp_parity.json under "module"."""
import json
import os

import numpy as np
import pytest

from _head_amp_cases import AMP_CASES, AMP_FIXTURE, PRECISIONS, amp_fixture_tensors, amp_modes, bar
from _head_cases import case_inputs
from _head_dev import heads_of, run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "head_amp_parity.json")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", AMP_CASES, ids=[c["name"] for c in AMP_CASES])
def test_fixture_parity(case, precision):
    z = np.load(AMP_FIXTURE)
    inputs = case_inputs(case)
    bad, worst = [], {}
    for mode in amp_modes(case):
        m = heads_of(case, inputs, mode == "train")
        m.precision = precision
        got = run(m, inputs)
        for li, d in enumerate(got):
            want = amp_fixture_tensors(z, case, mode, precision, li)
            assert set(d) == set(want), sorted(set(d) ^ set(want))
            for n, (r64, idx, flip, m64) in want.items():
                g = d[n].numpy().reshape(-1)
                if n.startswith("num_batches_tracked"):
                    assert int(g[0]) == int(r64[0]), (mode, li, n)
                    continue
                g = g.astype(np.float64)
                b = bar(flip, m64)
                err = float(np.abs((g if idx is None else g[idx]) - r64).max())
                print(f"{case['name']:5s} {mode:5s} {precision} L{li} {n:36s} err {err:.3e}  bar {b:.3e}  ratio {err / b:.3f}")
                if err / b > worst.get(mode, (0.0,))[0]:
                    worst[mode] = (err / b, f"L{li} {n}")
                if not err <= b:
                    bad.append((mode, li, n, err, b))
    try:                                                   # the figures of this run, beside the others' (best effort)
        table = json.load(open(PARITY)) if os.path.exists(PARITY) else {}
        table.setdefault("module", {})[f"{case['name']}/{precision}"] = {
            mo: {"worst_ratio": round(r, 4), "tensor": t} for mo, (r, t) in worst.items()}
        with open(PARITY, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass
    assert not bad, bad
