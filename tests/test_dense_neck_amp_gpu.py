"""DetectNeckMS in precision "fp16" / "bf16" on the device against tests/golden/dense_neck_amp.npz: the six dense-neck
cases' inputs, train mode plus eval for `base`, forward and backward.

What this test is for is wiring: every pass rounds, the right operands are used, and the backward runs in the forward's
mode.  (The kernels' arithmetic is held to the tight bar of test_dense_conv3x3_amp_gpu.py.)  The bar is max(4 x flip, 2
fp32 ulps): `flip` is what an ulp of difference in a computed operand does to the reference itself once a rounding flips
(tests/_dense_neck_amp_cases.py).  Tensors the fixture stores sampled are held to the float64 restatement everywhere
(test_dense_neck_amp_cpu.py ties it to the fixture).  The worst error / bar of every case is written to
profiles/dense_neck_amp_parity.json under "module"."""
import json
import os

import numpy as np
import pytest

from _dense_neck_amp_cases import AMP_CASES as CASES, AMP_FIXTURE, AMP_PRECISIONS, amp_fixture_tensors, bar
from _dense_neck_amp_np import neck_all as neck_all_amp
from _dense_neck_cases import case_inputs, modes
from _dense_neck_dev import neck_of, run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "dense_neck_amp_parity.json")


@pytest.mark.parametrize("precision", AMP_PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_parity(case, precision):
    z = np.load(AMP_FIXTURE)
    inputs = case_inputs(case)
    bad, worst = [], {}
    for mode in modes(case):
        m = neck_of(case, inputs, mode == "train")
        m.precision = precision
        got = run(m, inputs)
        full = None
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
                if idx is not None:                        # stored sampled: everywhere against the restatement
                    full = full or neck_all_amp(inputs, case["depth"], mode == "train", precision)
                    r64 = np.asarray(full[li][n], np.float64).reshape(-1)
                err = float(np.abs(g - r64).max())
                print(f"{case['name']:6s} {mode:5s} {precision} L{li} {n:32s} err {err:.3e}  bar {b:.3e}  ratio {err / b:.3f}")
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
