"""What the backbone-stage GPU tests and tools/tail_train_time.py share: a UIBStack with a case's weights, one forward +
backward of it, and the device error and bar of every fixture tensor."""
import numpy as np
import torch

import yololite_amd as ya
from _stage_cases import bar, case_inputs, fixture_tensors
from _train_dev import DEV, collect


def stack_of(case, inputs, train=True):
    m = ya.UIBStack(case["cin"], case["blocks"], prefix=case.get("prefix", ""))
    m.load_state_dict({k: torch.as_tensor(v) for k, v in {**inputs["params"], **inputs["buffers"]}.items()})
    return m.to(DEV).train(train)


def run(m, inputs, x_grad=True, layout="nhwc"):
    """forward + backward with the case's gy -> {fixture tensor name: cpu tensor}"""
    m.zero_grad(set_to_none=True)
    x = torch.from_numpy(inputs["x"]).to(DEV)
    if layout == "nchw":                                   # contiguous NCHW memory
        x = x.permute(0, 3, 1, 2).contiguous()
    x.requires_grad_(x_grad)
    y = m(x, layout=layout)
    if y.requires_grad:
        y.backward(torch.from_numpy(inputs["gy"]).to(DEV))
    d = {"y": y.detach().cpu()}
    if x.grad is not None:
        d["dx"] = (x.grad if layout == "nhwc" else x.grad.permute(0, 2, 3, 1)).contiguous().cpu()
    return collect(m, d)


def parity_ratios(case, mode, z):
    """{tensor: (error, bar)} of one case and mode against the fixture `z`"""
    inputs = case_inputs(case)
    got = run(stack_of(case, inputs, mode == "train"), inputs)
    want = fixture_tensors(z, case, mode)
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    out = {}
    for n, (r64, idx, e32, m64) in want.items():
        g = got[n].numpy().reshape(-1)
        if n.endswith("num_batches_tracked"):
            assert int(g[0]) == int(r64[0]), (case["name"], mode, n)
            continue
        g = g.astype(np.float64)
        out[n] = (float(np.abs((g if idx is None else g[idx]) - r64).max()), bar(e32, m64))
    return out
