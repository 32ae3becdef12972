"""Inputs, CPU yardstick and device runner of the fused training step's tests (tests/test_train_step_gpu.py) and of
tools/train_step_time.py --parity.

The model: ten parameters of COUNTS elements in three groups with different lr (two of them views into a larger buffer
at storage offsets of 1 and 2 elements), two floating EMA-only buffers of 24 and 257 elements (the second a view at an
offset of 3 elements in the model AND the EMA, so that a 16-byte body with a scalar head runs), one int64 scalar.
The yardstick is the reference's sequence (tools/train.py:352-359) with torch's own pieces on the CPU, in float64 or
float32, from the same fp32 start values and gradients."""
import math

import numpy as np
import torch

COUNTS = [1, 3, 4, 5, 255, 256, 257, 1023, 4097, 70001]
GROUP_OF = [0, 0, 0, 0, 1, 1, 1, 2, 2, 2]
LR = {"adamw": (1e-3, 2e-3, 5e-4), "adam": (1e-3, 2e-3, 5e-4), "sgd": (1e-2, 2e-2, 5e-3)}
WD = 1e-2
EMA_ONLY = [24, 257]
VIEW_OFFSET = {8: 1, 9: 2}          # parameter index -> storage offset (elements): 4- and 8-byte alignment
NONE_PARAM, NONE_STEPS = 5, (1, 2)  # parameter 5 has no gradient in steps 2 and 3
EMA_DECAY, TOTAL_UPDATES = 0.999, 100
NSTEPS = 5
KINDS = ("adamw", "adam", "sgd")
QUANTITIES = {"adamw": ("param", "exp_avg", "exp_avg_sq", "ema"), "adam": ("param", "exp_avg", "exp_avg_sq", "ema"),
              "sgd": ("param", "momentum_buffer", "ema")}


def inputs(seed=0):
    rs = np.random.RandomState(1000 + seed)
    p0 = [rs.randn(n).astype(np.float32) for n in COUNTS]
    grads = [[(0.1 * rs.randn(n)).astype(np.float32) for n in COUNTS] for _ in range(NSTEPS)]
    ema0 = [(p + 0.05 * rs.randn(len(p))).astype(np.float32) for p in p0]
    buf = [[(1.0 + 0.1 * t + rs.rand(n)).astype(np.float32) for n in EMA_ONLY] for t in range(NSTEPS)]
    ebuf0 = [rs.rand(n).astype(np.float32) for n in EMA_ONLY]
    return {"p0": p0, "grads": grads, "ema0": ema0, "buf": buf, "ebuf0": ebuf0}


def ema_d(updates):
    return EMA_DECAY * (1 - math.exp(-updates / max(100, TOTAL_UPDATES // 5)))


def _grad_at(inp, t, i, none_steps, poison):
    if i == NONE_PARAM and t in none_steps:
        return None
    g = inp["grads"][t][i]
    for (pt, pi, pe, val) in poison:
        if pt == t and pi == i:
            g = g.copy()
            g[pe] = val
    return g


def run_torch(kind, dtype, nsteps, grad_clip=0.0, none_steps=NONE_STEPS, growth_interval=2000, poison=(), seed=0):
    """the yardstick on the CPU in `dtype`; poison = [(step, parameter, element, value)]"""
    inp = inputs(seed)
    params = [torch.nn.Parameter(torch.from_numpy(p).to(dtype)) for p in inp["p0"]]
    groups = [{"params": [p for p, g in zip(params, GROUP_OF) if g == k], "lr": LR[kind][k], "weight_decay": WD}
              for k in range(3)]
    if kind == "sgd":
        opt = torch.optim.SGD(groups, momentum=0.9, nesterov=True, foreach=False)
    else:
        opt = (torch.optim.AdamW if kind == "adamw" else torch.optim.Adam)(groups, foreach=False)
    scaler = torch.amp.GradScaler("cpu", growth_interval=growth_interval)
    scaler.scale(torch.zeros(1))
    ema = [torch.from_numpy(e).to(dtype) for e in inp["ema0"]]
    ebuf = [torch.from_numpy(e).to(dtype) for e in inp["ebuf0"]]
    eint = torch.zeros((), dtype=torch.int64)
    norms, found, updates = [], [], 0
    for t in range(nsteps):
        scale = scaler.get_scale()
        for i, p in enumerate(params):
            g = _grad_at(inp, t, i, none_steps, poison)
            p.grad = None if g is None else torch.from_numpy(g).to(dtype) * scale
        scaler.unscale_(opt)
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, grad_clip if grad_clip > 0 else float("inf"),
                                                          foreach=False)))
        scaler.step(opt)
        scaler.update()
        found.append(scaler.get_scale() < scale)
        updates += 1
        d = ema_d(updates)
        with torch.no_grad():
            for v, m in zip(ema, params):
                v.mul_(d).add_(m.detach(), alpha=1 - d)
            for v, m in zip(ebuf, inp["buf"][t]):
                v.mul_(d).add_(torch.from_numpy(m).to(dtype), alpha=1 - d)
            eint.copy_(torch.tensor(t + 1))
    names = QUANTITIES[kind][1:-1]
    out = {"param": [p.detach().numpy().astype(np.float64) for p in params],
           "ema": [v.numpy().astype(np.float64) for v in ema + ebuf], "int": int(eint), "norms": norms, "found": found,
           "scale": scaler.get_scale(), "tracker": int(scaler._growth_tracker),
           "steps": [float(opt.state[p]["step"]) if "step" in opt.state.get(p, {}) else None for p in params]}
    for n in names:
        out[n] = [opt.state[p][n].numpy().astype(np.float64) if n in opt.state.get(p, {}) and
                  opt.state[p][n] is not None else np.zeros(len(q), np.float64) for p, q in zip(params, inp["p0"])]
    return out


def build_fused(kind, grad_clip=0.0, growth_interval=2000, seed=0, chunk_elems=1024):
    """-> FusedTrainStep, parameters, model dict, EMA dict (all on cuda:0)"""
    import yololite_amd as ya
    inp = inputs(seed)
    dev = "cuda:0"
    params = []
    for i, p in enumerate(inp["p0"]):
        o = VIEW_OFFSET.get(i, 0)
        base = torch.zeros(len(p) + o + 3, device=dev)
        v = base[o:o + len(p)]
        v.copy_(torch.from_numpy(p))
        params.append(torch.nn.Parameter(v))
        assert params[-1].data_ptr() == base.data_ptr() + 4 * o
    model = {f"p{i}": p.detach() for i, p in enumerate(params)}
    ema = {f"p{i}": torch.from_numpy(e).to(dev) for i, e in enumerate(inp["ema0"])}
    for j, n in enumerate(EMA_ONLY):
        o = 3 if j == 1 else 0
        model[f"b{j}"] = torch.zeros(n + o, device=dev)[o:]
        ema[f"b{j}"] = torch.zeros(n + o, device=dev)[o:]
        ema[f"b{j}"].copy_(torch.from_numpy(inp["ebuf0"][j]))
    model["n"] = torch.zeros((), dtype=torch.int64, device=dev)
    ema["n"] = torch.zeros((), dtype=torch.int64, device=dev)
    groups = [{"params": [p for p, g in zip(params, GROUP_OF) if g == k], "lr": LR[kind][k], "weight_decay": WD}
              for k in range(3)]
    fts = ya.FusedTrainStep(groups, optimizer=kind, grad_clip=grad_clip, amp=True,
                            scaler_kwargs={"growth_interval": growth_interval}, ema_model=ema, model=model,
                            ema_decay=EMA_DECAY, total_updates=TOTAL_UPDATES, chunk_elems=chunk_elems)
    return fts, params, model, ema


def snapshot(fts, params, ema, norms, found):
    st = fts.read_state()
    sd = fts.state_dict()
    out = {"param": [p.detach().cpu().numpy() for p in params],
           "ema": [ema[k].cpu().numpy() for k in ema if k != "n"], "int": int(ema["n"].cpu()),
           "norms": norms, "found": found, "scale": st["scale"], "tracker": st["_growth_tracker"],
           "steps": [s if s > 0 else None for s in st["steps"]]}
    for n in QUANTITIES[fts.optimizer][1:-1]:
        out[n] = [sd["state"][i][n].cpu().numpy() if i in sd["state"] else np.zeros(len(p), np.float32)
                  for i, p in enumerate(out["param"])]
    return out


def run_fused(kind, nsteps, grad_clip=0.0, none_steps=NONE_STEPS, growth_interval=2000, poison=(), seed=0,
              chunk_elems=1024, set_to_none=True, after_step=None):
    """the same steps through FusedTrainStep.  set_to_none: new gradient tensors every step (zero_grad(True)), else the
    first step's tensors are kept and overwritten (a None gradient is None either way).  The gradient of parameter 9
    is a view at an offset of one element: the statistics kernel's scalar head."""
    inp = inputs(seed)
    fts, params, model, ema = build_fused(kind, grad_clip, growth_interval, seed, chunk_elems)
    norms, found, kept = [], [], {}
    scale = 65536.0
    for t in range(nsteps):
        fts.zero_grad(set_to_none=True)
        for i, p in enumerate(params):
            g = _grad_at(inp, t, i, none_steps, poison)
            if g is None:
                continue
            o = 1 if i == 9 else 0
            if set_to_none or i not in kept:
                kept[i] = torch.empty(len(g) + o, device="cuda:0")[o:]
            kept[i].copy_(torch.from_numpy(g * np.float32(scale)))
            p.grad = kept[i]
        for j in range(len(EMA_ONLY)):
            model[f"b{j}"].copy_(torch.from_numpy(inp["buf"][t][j]))
        model["n"].fill_(t + 1)
        norms.append(fts.step().clone())
        st = fts.read_state()
        found.append(st["found_inf"])
        scale = st["scale"]
        if after_step is not None:
            after_step(t, fts, params, ema)
    return snapshot(fts, params, ema, [float(n.cpu()) for n in norms], found)


def cat(x):
    return np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in x])


def bar(err32, max64):
    """the project's rule: 4 x the reference's own fp32 error, floor 2 fp32 ulps at the quantity's max|f64|"""
    return max(4.0 * err32, 2.0 * float(np.spacing(np.float32(max64))))


def parity_rows(kind, nsteps, dev, r64=None, r32=None, **kw):
    r64 = r64 or run_torch(kind, torch.float64, nsteps, **kw)
    r32 = r32 or run_torch(kind, torch.float32, nsteps, **kw)
    rows = {}
    for q in QUANTITIES[kind]:
        c = cat(r64[q])
        e32 = float(np.abs(cat(r32[q]) - c).max())
        err = float(np.abs(cat(dev[q]) - c).max())
        m64 = float(np.abs(c).max())
        b = bar(e32, m64)
        rows[q] = {"max_f64": m64, "err32": e32, "device_error": err, "bar": b, "ratio": err / b}
    return rows
