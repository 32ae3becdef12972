"""The fused training step on the device (csrc/yl_train.hip behind yololite_amd.FusedTrainStep) against the reference's
sequence of torch calls (tools/train.py:352-359: GradScaler, clip_grad_norm_, torch.optim.{AdamW, Adam, SGD} with
foreach=False, the EMA loop) run on the CPU in float64 and float32 from the same fp32 start values and gradients.

Tolerance, per optimizer and per quantity (parameter, each state, EMA): max|dev - f64| <= 4 x max|cpu32 - f64|, with a
floor of 2 fp32 ulps at that quantity's max|f64| (the rule of the loss tests).  Measured on an MI355X after the
five-step trajectory (profiles/train_step_parity.json): worst device error / bar = 0.29 (sgd, EMA after one step; 0.25 after five); the device
evaluates each update in float64 from the fp32 operands and rounds once per stored value, so it sits well inside the
CPU's own fp32 error.

Inputs (tests/_train_cases.py): ten parameters of 1 .. 70 001 elements in three groups with different lr, two of them
views at storage offsets of 1 and 2 elements, two floating EMA-only entries, one int64 scalar; chunks of 1024
elements, so the largest tensor spans 69 chunks."""
import functools

import numpy as np
import pytest
import torch

import yololite_amd as ya
import _train_cases as tc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ref(kind, dtype, nsteps, grad_clip=0.0, growth_interval=2000, poison=()):
    return tc.run_torch(kind, dtype, nsteps, grad_clip=grad_clip, growth_interval=growth_interval, poison=poison)


@functools.lru_cache(maxsize=None)
def _dev(kind, nsteps, grad_clip=0.0, growth_interval=2000, poison=(), chunk_elems=1024, set_to_none=True):
    return tc.run_fused(kind, nsteps, grad_clip=grad_clip, growth_interval=growth_interval, poison=poison,
                        chunk_elems=chunk_elems, set_to_none=set_to_none)


def _expected_steps(nsteps, skipped=()):
    out = []
    for i in range(len(tc.COUNTS)):
        n = sum(1 for t in range(nsteps) if t not in skipped and not (i == tc.NONE_PARAM and t in tc.NONE_STEPS))
        out.append(float(n) if n else None)
    return out


def _check_parity(kind, nsteps, dev, **kw):
    r64, r32 = _ref(kind, torch.float64, nsteps, **kw), _ref(kind, torch.float32, nsteps, **kw)
    rows = tc.parity_rows(kind, nsteps, dev, r64, r32)
    for q, r in rows.items():
        print(f"{kind} steps={nsteps} {q}: device_error {r['device_error']:.3e} err32 {r['err32']:.3e} "
              f"bar {r['bar']:.3e} ratio {r['ratio']:.3f}")
    for q, r in rows.items():
        assert r["device_error"] <= r["bar"], (kind, nsteps, q, r)
    return r64


def _same_bits(a, b, keys):
    for k in keys:
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(np.asarray(x).view(np.int32), np.asarray(y).view(np.int32)), k


def _all_keys(kind):
    return tc.QUANTITIES[kind]


@pytest.mark.parametrize("nsteps", [1, tc.NSTEPS])
@pytest.mark.parametrize("kind", tc.KINDS)
def test_step_parity(kind, nsteps):
    dev = _dev(kind, nsteps)
    r64 = _check_parity(kind, nsteps, dev)
    # parameter 5 has no gradient in steps 2 and 3: its count lags as torch's does (torch's SGD keeps none: counted)
    assert dev["steps"] == _expected_steps(nsteps)
    if kind != "sgd":
        assert dev["steps"] == r64["steps"]
    assert dev["int"] == r64["int"] == nsteps
    assert dev["found"] == [False] * nsteps and dev["scale"] == 65536.0 and dev["tracker"] == nsteps
    for n, m in zip(dev["norms"], r64["norms"]):
        assert abs(n - m) <= 2 * np.spacing(np.float32(m)), (n, m)


@pytest.mark.parametrize("kind", tc.KINDS)
def test_clip(kind):
    """norm ~ 27.6: max_norm 1000 leaves the gradients alone (bit for bit the no-clip run), max_norm 1 scales them"""
    free, above, below = _dev(kind, 2), _dev(kind, 2, grad_clip=1000.0), _dev(kind, 2, grad_clip=1.0)
    _same_bits(free, above, _all_keys(kind))
    assert free["norms"] == above["norms"]
    for run, clip in ((below, 1.0), (above, 1000.0)):
        r64 = _check_parity(kind, 2, run, grad_clip=clip)
        for n, m in zip(run["norms"], r64["norms"]):        # the returned norm is the one BEFORE clipping
            assert abs(n - m) <= 2 * np.spacing(np.float32(m)), (n, m)
    assert any(not np.array_equal(a, b) for a, b in zip(free["param"], below["param"])), "the coefficient was not applied"


POISONS = [(0, 0, float("inf")), (0, 0, float("nan")), (9, 70000, float("inf")), (9, 70000, float("nan"))]


@pytest.mark.parametrize("pi,pe,val", POISONS)
def test_skipped_step(pi, pe, val):
    """a non-finite element in step 2 of 3 (first element of the first tensor; last element of the 70 001-element tensor,
    which the scalar tail reads): parameters, states and step counts keep their bits, the scale is halved, the EMA
    moves, and the clean step after it matches the yardstick that skipped the same step"""
    kind = "adamw"
    poison = ((1, pi, pe, val),)
    seen = {}

    def after(t, fts, params, ema):
        seen[t] = tc.snapshot(fts, params, ema, [], [])

    dev = tc.run_fused(kind, 3, poison=poison, after_step=after)
    before, skipped = seen[0], seen[1]
    _same_bits(before, skipped, ("param", "exp_avg", "exp_avg_sq"))
    assert skipped["steps"] == before["steps"] == [1.0] * len(tc.COUNTS)
    assert before["scale"] == 65536.0 and skipped["scale"] == 32768.0 and skipped["tracker"] == 0
    assert dev["found"] == [False, True, False]
    assert not np.isfinite(dev["norms"][1])
    assert all(not np.array_equal(a, b) for a, b in zip(before["ema"], skipped["ema"])), "the EMA did not move"
    assert skipped["int"] == 2
    r64 = _check_parity(kind, 3, dev, poison=poison)
    assert dev["steps"] == r64["steps"] and dev["scale"] == r64["scale"] == 32768.0
    assert dev["tracker"] == r64["tracker"] == 1


def test_scale_growth():
    dev = _dev("sgd", 3, growth_interval=3)
    r64 = _ref("sgd", torch.float64, 3, growth_interval=3)
    assert dev["scale"] == r64["scale"] == 131072.0 and dev["tracker"] == r64["tracker"] == 0
    _check_parity("sgd", 3, dev, growth_interval=3)


@pytest.mark.parametrize("kind", tc.KINDS)
def test_determinism(kind):
    a = _dev(kind, tc.NSTEPS)
    b = tc.run_fused(kind, tc.NSTEPS)
    _same_bits(a, b, _all_keys(kind))
    assert np.array_equal(np.float32(a["norms"]).view(np.int32), np.float32(b["norms"]).view(np.int32))
    assert a["steps"] == b["steps"]


@pytest.mark.parametrize("kind", tc.KINDS)
def test_gradient_pointers(kind):
    """new gradient tensors every step (zero_grad(set_to_none=True)) against gradients kept in place; default chunks"""
    fresh = _dev(kind, tc.NSTEPS, chunk_elems=None, set_to_none=True)
    kept = _dev(kind, tc.NSTEPS, chunk_elems=None, set_to_none=False)
    _same_bits(fresh, kept, _all_keys(kind))
    assert fresh["norms"] == kept["norms"] and fresh["steps"] == kept["steps"]
    _same_bits(fresh, _dev(kind, tc.NSTEPS), _all_keys(kind))       # the chunk size does not enter the element updates


def test_state_dict_resume():
    """two steps, state_dict into a fresh object, three more: bit for bit the five-step run"""
    kind = "adamw"
    inp = tc.inputs()
    whole = _dev(kind, tc.NSTEPS)
    box = {}

    def after(t, fts, params, ema):
        if t == 1:
            box["sd"] = fts.state_dict()
            box["p"] = [p.detach().clone() for p in params]
            box["ema"] = {k: v.clone() for k, v in ema.items()}

    tc.run_fused(kind, 2, after_step=after)
    fts, params, model, ema = tc.build_fused(kind)
    with torch.no_grad():
        for p, q in zip(params, box["p"]):
            p.copy_(q)
        for k in ema:
            ema[k].copy_(box["ema"][k])
    fts.load_state_dict(box["sd"])
    assert fts.updates == 2 and fts.get_scale() == 65536.0
    norms = []
    for t in range(2, tc.NSTEPS):
        fts.zero_grad()
        for i, p in enumerate(params):
            g = tc._grad_at(inp, t, i, tc.NONE_STEPS, ())
            if g is not None:
                p.grad = torch.from_numpy(g * np.float32(65536.0)).cuda()
        for j in range(len(tc.EMA_ONLY)):
            model[f"b{j}"].copy_(torch.from_numpy(inp["buf"][t][j]))
        model["n"].fill_(t + 1)
        norms.append(float(fts.step().cpu()))
    got = tc.snapshot(fts, params, ema, norms, [])
    _same_bits(whole, got, _all_keys(kind))
    assert got["steps"] == whole["steps"] and got["norms"] == whole["norms"][2:]


def test_refusals_on_the_device():
    p = torch.nn.Parameter(torch.zeros(8, device="cuda:0"))
    with pytest.raises(ya.YoloLiteHipError):
        ya.FusedTrainStep([p], model={"p": p.detach()}, ema_model={"p": torch.zeros(8)})      # EMA on the CPU
    fts = ya.FusedTrainStep([p], amp=False)
    p.grad = torch.zeros(16, device="cuda:0")[::2]
    with pytest.raises(ya.YoloLiteHipError):
        fts.step()
    p.grad = torch.ones(8, device="cuda:0")
    n = fts.step()
    assert abs(float(n) - 8 ** 0.5) < 1e-6 and fts.get_scale() == 1.0
    assert fts.scale(n) is n


def test_with_the_criterion():
    """the level tensors of the loss's smallest gradient case are the parameters: fts.scale(loss).backward();
    fts.step() against torch.optim.AdamW + clip_grad_norm_ applied on the device to the same gradients; the CPU
    float64 run of that update is the centre, the CPU float32 run gives the bar"""
    from _lossaf_grad_cases import grad_case_inputs, grad_cases
    cases, npz = grad_cases()
    case = min(cases, key=lambda c: c["batch"] * sum(s * s for s in c["sizes"]))
    levels, gt, lab, off, kw = grad_case_inputs(case, npz)
    tg = [{"boxes": gt[off[b]:off[b + 1]], "labels": lab[off[b]:off[b + 1]]} for b in range(case["batch"])]
    crit = ya.LossAF(case["num_classes"], case["img_size"], grad=True, **kw)
    clip, lr, wd = 0.1, 1e-3, 1e-2       # the case's gradient norm is 0.307: the coefficient is applied

    params = [torch.nn.Parameter(torch.from_numpy(l).cuda()) for l in levels]
    fts = ya.FusedTrainStep(params, optimizer="adamw", grad_clip=clip, lr=lr, weight_decay=wd)
    fts.zero_grad()
    loss, _ = crit(params, tg)
    fts.scale(loss).backward()
    scaled = [p.grad.detach().clone() for p in params]
    norm = float(fts.step().cpu())
    got = {"param": [p.detach().cpu().numpy() for p in params]}
    sd = fts.state_dict()
    for n in ("exp_avg", "exp_avg_sq"):
        got[n] = [sd["state"][i][n].cpu().numpy() for i in range(len(params))]

    def torch_update(device, dtype):
        ps = [torch.nn.Parameter(torch.from_numpy(l).to(device=device, dtype=dtype)) for l in levels]
        opt = torch.optim.AdamW(ps, lr=lr, weight_decay=wd, foreach=False)
        for p, g in zip(ps, scaled):
            p.grad = g.to(device=device, dtype=dtype) / 65536.0
        nrm = torch.nn.utils.clip_grad_norm_(ps, clip, foreach=False)
        opt.step()
        out = {"param": [p.detach().cpu().numpy().astype(np.float64) for p in ps]}
        for n in ("exp_avg", "exp_avg_sq"):
            out[n] = [opt.state[p][n].cpu().numpy().astype(np.float64) for p in ps]
        return out, float(nrm)

    (r64, n64), (r32, _), (rdev, ndev) = (torch_update("cpu", torch.float64), torch_update("cpu", torch.float32),
                                          torch_update("cuda:0", torch.float32))
    assert n64 > clip, "the case does not clip"
    assert abs(norm - n64) <= 2 * np.spacing(np.float32(n64)) and abs(ndev - n64) <= 1e-5 * n64
    for q in ("param", "exp_avg", "exp_avg_sq"):
        c = tc.cat(r64[q])
        m64 = float(np.abs(c).max())
        e32, edev = float(np.abs(tc.cat(r32[q]) - c).max()), float(np.abs(tc.cat(rdev[q]) - c).max())
        err = float(np.abs(tc.cat(got[q]) - c).max())
        print(f"criterion {q}: device_error {err:.3e} torch fp32 error cpu {e32:.3e} device {edev:.3e} "
              f"bars {tc.bar(e32, m64):.3e} {tc.bar(edev, m64):.3e}")
        assert err <= tc.bar(e32, m64) and err <= tc.bar(edev, m64), q
