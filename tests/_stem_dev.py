"""What the dense-stem GPU tests and tools/backbone_train_time.py share: a ConvStack with a case's weights, one forward +
backward of it, the whole oracle_tiny backbone on the device, and the float64 restatement of an eval-mode backbone."""
import numpy as np
import torch

import yololite_amd as ya
import _stage_cases as sc
from _stem_cases import bar, case_inputs, fixture_tensors, sizes, stack_all
from _train_dev import DEV, collect


def stack_of(case, inputs, train=True):
    m = ya.ConvStack(case["cin"], case["units"], prefix=case.get("prefix", ""), input_layout="nchw" if case["planar"] else "nhwc")
    m.load_state_dict({k: torch.as_tensor(v) for k, v in {**inputs["params"], **inputs["buffers"]}.items()})
    return m.to(DEV).train(train)


def run(m, case, inputs, x_grad=True):
    """forward + backward with the case's gy -> {fixture tensor name: cpu tensor}"""
    m.zero_grad(set_to_none=True)
    x = torch.from_numpy(inputs["x"]).to(DEV)
    if case["planar"]:
        x = x.permute(0, 3, 1, 2).contiguous()
    else:
        x.requires_grad_(x_grad)
    y = m(x)
    if y.requires_grad:
        y.backward(torch.from_numpy(inputs["gy"]).to(DEV))
    d = {"y": y.detach().cpu()}
    if x.grad is not None:
        d["dx"] = x.grad.contiguous().cpu()
    return collect(m, d)


def ratios(got, want, what):
    """{tensor: (error, bar)} of device results against fixture tensors"""
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    out = {}
    for n, (r64, idx, e32, m64) in want.items():
        g = got[n].numpy().reshape(-1)
        if n.endswith("num_batches_tracked"):
            assert int(g[0]) == int(r64[0]), (what, n)
            continue
        g = g.astype(np.float64)
        out[n] = (float(np.abs((g if idx is None else g[idx]) - r64).max()), bar(e32, m64))
    return out


def parity_ratios(case, mode, z):
    inputs = case_inputs(case)
    return ratios(run(stack_of(case, inputs, mode == "train"), case, inputs), fixture_tensors(z, case, mode), (case["name"], mode))


def tiny_backbone(inputs):
    """MobileNetV4Backbone of oracle_tiny with the composite case's weights, in train mode"""
    from yololite_amd.program import make_meta
    meta = make_meta("YOLOLiteMS_CPU", "oracle_tiny", num_classes=3, img_size=64)
    return ya.MobileNetV4Backbone.from_state_dict(meta, {**inputs["params"], **inputs["buffers"]}).to(DEV).train()


def run_tiny(m, inputs):
    """loss = sum_k <c_k, g_k> -> {fixture tensor name: cpu tensor}"""
    m.zero_grad(set_to_none=True)
    x = torch.from_numpy(inputs["x"]).to(DEV).permute(0, 3, 1, 2).contiguous()
    cs = m(x)
    loss = sum((c * torch.from_numpy(inputs[g]).to(DEV)).sum() for c, g in zip(cs, ("g3", "g4", "g5")))
    loss.backward()
    d = {"y.c3": cs[0].detach().cpu(), "y.c4": cs[1].detach().cpu(), "y.c5": cs[2].detach().cpu()}
    for part in (m.stem, m.mid, m.tail):
        collect(part, d)
    return d


def restated_features(backbone, x_nchw):
    """the float64 restatement of the eval-mode backbone on the image -> [(r64, bar)] for c3, c4, c5: the bar an fp32
    evaluation gets against it is max(4 x the fp32 restatement's error, 2 fp32 ulps at the largest value)"""
    sd = {k: v.detach().cpu().numpy() for k, v in backbone.state_dict().items()}
    params = {k: v for k, v in sd.items() if "running_" not in k and "tracked" not in k}
    buffers = {k: v for k, v in sd.items() if "running_" in k or "tracked" in k}
    B, S = int(x_nchw.shape[0]), int(x_nchw.shape[2])
    stem, mid, tail = backbone.stem, backbone.mid, backbone.tail
    scase = dict(name="stem", B=B, S=S, cin=3, planar=True, prefix="backbone.",
                 units=[dict(k=u["k"], s=u["s"], c=u["c"], conv=u["conv"], bn=u["bn"]) for u in stem.units_cfg])

    def ucase(m, S_):
        blocks = [{k: d[k] for k in ("type", "a", "k", "s", "mid", "c", "name")} for d in m.blocks_cfg]
        return dict(name="s", B=B, S=S_, cin=m.in_channels, prefix="backbone.", blocks=blocks)

    xh = x_nchw.cpu().numpy().transpose(0, 2, 3, 1)
    ins = lambda x: dict(params=params, buffers=buffers, x=x)   # noqa: E731
    res = {}
    for dt in (np.float64, np.float32):
        c3 = _forward_only(stack_all, scase, ins(xh), dt)
        c4 = _forward_only(sc.stack_all, ucase(mid, c3.shape[1]), ins(c3), dt)
        c5 = _forward_only(sc.stack_all, ucase(tail, c4.shape[1]), ins(c4), dt)
        res[dt] = (c3, c4, c5)
    return [(r64, bar(np.abs(r32.astype(np.float64) - r64).max(), np.abs(r64).max())) for r64, r32 in zip(res[np.float64], res[np.float32])]


def _forward_only(stack, case, inputs, dt):
    """y of an eval-mode stack: the restatement runs forward and backward, so it gets a zero gy of the right shape"""
    So = (sizes(case) if "units" in case else sc.sizes(case))[-1]
    cout = case["units"][-1]["c"] if "units" in case else case["blocks"][-1]["c"]
    inputs = dict(inputs, gy=np.zeros((case["B"], So, So, cout), np.float32))
    return stack(case, inputs, False, dt)["y"]
