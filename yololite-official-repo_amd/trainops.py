"""The training step's tail on the device: what the reference's loop does between backward() and the next forward.

    fts = FusedTrainStep(param_groups, optimizer="adamw", grad_clip=..., amp=True, ema_model=ema, model=model,
                         ema_decay=0.995, total_updates=...)
    fts.zero_grad(set_to_none=True)
    fts.scale(loss).backward()
    norm = fts.step()
        <- tools/train.py:347-359: scaler.scale / unscale_ / clip_grad_norm_ / scaler.step(optimizer) /
           scaler.update() / ema.update(model), and ModelEMA (:29-57)

One call of step() is three kernels (csrc/yl_train.hip) whatever the number of tensors: gradient statistics, a
one-workgroup reduce that also updates the loss scale and the per-tensor step counts, and one pass that applies the
optimizer (torch 2.10's single-tensor AdamW / Adam / SGD rules), the EMA and the integer-buffer copies.  Norm,
found_inf and scale stay in device memory; step() neither synchronises nor copies to the host.

Differences from the torch sequence, all deliberate:
  * gradients are read only -- the unscaled and clipped values are NOT written back into .grad (nothing in the
    reference's loop reads them afterwards);
  * the norm is computed in every step, also with grad_clip == 0 (step() returns it);
  * step() returns a view of the state block: the next step() overwrites it (clone it to keep it).
The learning-rate schedule and the EMA's warm-up stay on the host: `param_groups[i]["lr"]` / `["weight_decay"]` are
read on every call, as a torch scheduler leaves them.  fp32, contiguous tensors on one HIP device only; anything else
is refused.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

KINDS = {"adamw": _lib.YL_TRAIN_ADAMW, "adam": _lib.YL_TRAIN_ADAM, "sgd": _lib.YL_TRAIN_SGD}
_STATE_KEYS = {"adamw": ("exp_avg", "exp_avg_sq"), "adam": ("exp_avg", "exp_avg_sq"), "sgd": ("momentum_buffer",)}
_SCALER_DEFAULTS = {"init_scale": 65536.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000}


def plan_chunks(counts: Sequence[int], chunk_elems: int = _lib.YL_TRAIN_CHUNK_DEFAULT) -> List[Tuple[int, int, int]]:
    """The chunk list the kernels stride over: [(segment, offset, length)] in table order (yl_train_plan, a host
    function of the library -- no device needed)."""
    lib = _lib.load()
    n = len(counts)
    arr = (C.c_int64 * max(n, 1))(*[int(c) for c in counts])
    total = lib.yl_train_plan(arr, n, int(chunk_elems), None, 0)
    if total < 0:
        _lib.check(int(total), what="yl_train_plan")
    out = (_lib.yl_train_chunk * max(int(total), 1))()
    got = lib.yl_train_plan(arr, n, int(chunk_elems), out, total)
    if got != total:
        _lib.check(int(got) if got < 0 else -1, what="yl_train_plan")
    return [(out[i].seg, out[i].off, out[i].len) for i in range(int(total))]


def ema_warmup_limit(total_updates: int) -> int:
    return max(100, int(total_updates) // 5)


def ema_decay_at(updates: int, decay: float, total_updates: int) -> float:
    """ModelEMA's d after `updates` calls (tools/train.py:35,49), in double precision"""
    return float(decay) * (1.0 - math.exp(-int(updates) / ema_warmup_limit(total_updates)))


def _check_tensor(t, what: str, dtype=torch.float32):
    """dtype and layout first (host-side facts), the device last"""
    if not torch.is_tensor(t):
        raise _lib.YoloLiteHipError(f"{what}: not a tensor")
    if dtype is not None and t.dtype != dtype:
        raise _lib.YoloLiteHipError(f"{what}: dtype {t.dtype} is not supported (fp32 only)")
    if not t.is_contiguous():
        raise _lib.YoloLiteHipError(f"{what}: non-contiguous tensors are not supported")


def _normalise_groups(param_groups, defaults: dict) -> List[dict]:
    groups = list(param_groups)
    if not groups:
        raise ValueError("FusedTrainStep got an empty parameter list")
    if not isinstance(groups[0], dict):
        groups = [{"params": groups}]
    out = []
    for g in groups:
        g = dict(g)
        ps = g["params"]
        g["params"] = [ps] if torch.is_tensor(ps) else list(ps)
        for k, v in defaults.items():
            g.setdefault(k, v)
        out.append(g)
    return out


def build_state_dict(optimizer: str, param_groups: Sequence[dict], steps: Sequence[float],
                     state0: Sequence[torch.Tensor], state1: Sequence[Optional[torch.Tensor]], scale: float,
                     growth_tracker: int, ema_updates: int) -> dict:
    """torch's optimizer / GradScaler key names around the fused step's state (plain data in, plain dict out).
    `param_groups[i]["params"]` are parameter indices; a parameter that never stepped has no state entry, as in torch."""
    names = _STATE_KEYS[optimizer]
    state = {}
    for i, st in enumerate(steps):
        if float(st) <= 0:
            continue
        e = {"step": torch.tensor(float(st), dtype=torch.float32), names[0]: state0[i].detach().clone()}
        if len(names) > 1:
            e[names[1]] = state1[i].detach().clone()
        state[i] = e
    return {"optimizer": optimizer, "state": state,
            "param_groups": [{k: (list(v) if k == "params" else v) for k, v in g.items()} for g in param_groups],
            "scaler": {"scale": float(scale), "_growth_tracker": int(growth_tracker)},
            "ema_updates": int(ema_updates)}


def parse_state_dict(sd: dict, optimizer: str, nparams: int):
    """-> steps [nparams] float32, {index: (state0, state1 | None)}, group options, scale, tracker, ema_updates"""
    if sd.get("optimizer") != optimizer:
        raise ValueError(f"state_dict is of optimizer {sd.get('optimizer')!r}, this step runs {optimizer!r}")
    names = _STATE_KEYS[optimizer]
    steps = np.zeros((nparams,), np.float32)
    tensors = {}
    for i, e in sd["state"].items():
        i = int(i)
        if not 0 <= i < nparams:
            raise ValueError(f"state_dict names parameter {i}, there are {nparams}")
        steps[i] = float(e["step"])
        tensors[i] = (e[names[0]], e[names[1]] if len(names) > 1 else None)
    opts = [{k: v for k, v in g.items() if k != "params"} for g in sd["param_groups"]]
    return steps, tensors, opts, float(sd["scaler"]["scale"]), int(sd["scaler"]["_growth_tracker"]), int(sd["ema_updates"])


class FusedTrainStep:
    """See the module docstring.  `param_groups`: as given to torch.optim (tensors, or dicts with "params" and optional
    "lr" / "weight_decay").  `model` / `ema_model`: two modules (or two name -> tensor mappings) whose state_dict()s are
    paired entry by entry: parameters of `param_groups`, other floating entries (EMA only: BatchNorm running statistics,
    frozen parameters) and integer entries (copied).  Without them there is no EMA."""

    def __init__(self, param_groups, optimizer: str = "adamw", grad_clip: float = 0.0, amp: bool = True,
                 scaler_kwargs: Optional[dict] = None, ema_model=None, model=None, ema_decay: float = 0.999,
                 total_updates: int = 0, lr: float = 1e-3, weight_decay: Optional[float] = None,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, momentum: float = 0.9,
                 nesterov: bool = True, chunk_elems: Optional[int] = None):
        if optimizer not in KINDS:
            raise ValueError(f"optimizer must be one of {sorted(KINDS)}")
        self.optimizer = optimizer
        wd = (1e-2 if optimizer == "adamw" else 0.0) if weight_decay is None else float(weight_decay)
        self.param_groups = _normalise_groups(param_groups, {"lr": float(lr), "weight_decay": wd})
        if len(self.param_groups) > _lib.YL_TRAIN_MAX_GROUPS:
            raise _lib.YoloLiteHipError(f"at most {_lib.YL_TRAIN_MAX_GROUPS} parameter groups")
        self.grad_clip, self.amp = float(grad_clip), bool(amp)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.momentum, self.nesterov = float(momentum), bool(nesterov)
        self.ema_decay, self.total_updates, self.updates = float(ema_decay), int(total_updates), 0
        sk = dict(_SCALER_DEFAULTS, **(scaler_kwargs or {}))
        unknown = set(sk) - set(_SCALER_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown scaler_kwargs {sorted(unknown)}")
        if (model is None) != (ema_model is None):
            raise ValueError("give both `model` and `ema_model`, or neither")

        # ---- host-side checks first: nothing below this block has touched a device yet
        self.params: List[torch.Tensor] = []
        self._group_of: List[int] = []
        seen = set()
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                _check_tensor(p, f"parameter {len(self.params)} (group {gi})")
                if id(p) in seen:
                    raise ValueError("a parameter appears in more than one group")
                seen.add(id(p))
                if p.numel():
                    self.params.append(p)
                    self._group_of.append(gi)
        pairs = []          # (key, model tensor, ema tensor)
        if model is not None:
            msd = model.state_dict() if hasattr(model, "state_dict") else dict(model)
            esd = ema_model.state_dict() if hasattr(ema_model, "state_dict") else dict(ema_model)
            for k, v in esd.items():
                if k not in msd:
                    raise _lib.YoloLiteHipError(f"EMA entry {k!r} has no counterpart in the model")
                m = msd[k]
                if m.shape != v.shape or m.dtype != v.dtype:
                    raise _lib.YoloLiteHipError(f"EMA entry {k!r}: {tuple(v.shape)} {v.dtype} vs the model's "
                                                f"{tuple(m.shape)} {m.dtype}")
                fl = v.dtype.is_floating_point
                _check_tensor(v, f"EMA entry {k!r}", torch.float32 if fl else None)
                _check_tensor(m, f"model entry {k!r}", torch.float32 if fl else None)
                if v.numel():
                    pairs.append((k, m, v))
        every = self.params + [t for _, m, v in pairs for t in (m, v)]
        if not every:
            raise ValueError("FusedTrainStep got no elements to update")
        if not torch.cuda.is_available() or any(not t.is_cuda for t in every):
            raise _lib.YoloLiteHipError("FusedTrainStep needs its tensors on a HIP device (no CPU fallback)")
        self.device = every[0].device
        if any(t.device != self.device for t in every):
            raise _lib.YoloLiteHipError("FusedTrainStep: all tensors must live on one device")

        # ---- the segment table: state_dict entries in order, then parameters the state_dict does not hold
        self.lib = _lib.load()
        two = optimizer != "sgd"
        self._state0 = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self._state1 = [torch.zeros_like(p, memory_format=torch.contiguous_format) if two else None for p in self.params]
        by_ptr = {(p.data_ptr(), p.numel()): i for i, p in enumerate(self.params)}
        rows = []           # (param index | None, param/src, ema | None, count, flags)
        placed = set()
        for k, m, v in pairs:
            i = by_ptr.get((m.data_ptr(), m.numel())) if v.dtype.is_floating_point else None
            if i is not None and i in placed:
                raise _lib.YoloLiteHipError(f"entry {k!r} shares its storage with another entry (tied parameters "
                                            "are not supported)")
            if i is not None:
                placed.add(i)
                rows.append((i, self.params[i], v, v.numel(), 0))
            elif v.dtype.is_floating_point:
                rows.append((None, m, v, v.numel(), _lib.YL_TRAIN_SEG_EMA_ONLY))
            else:
                rows.append((None, m, v, v.numel() * v.element_size(), _lib.YL_TRAIN_SEG_BYTES))
        for i, p in enumerate(self.params):
            if i not in placed:
                rows.append((i, p, None, p.numel(), 0))
        self._keep = [(m, v) for _, m, v in pairs]
        self._nseg = len(rows)
        self._seg_of_param = [0] * len(self.params)
        self._param_rows: List[Tuple[int, torch.Tensor]] = []       # (segment, parameter) of every trainable row
        segs = (_lib.yl_train_segment * self._nseg)()
        for s, (i, src, ema, count, flags) in enumerate(rows):
            segs[s].param = src.data_ptr()
            segs[s].ema = ema.data_ptr() if ema is not None else None
            segs[s].count, segs[s].flags = int(count), int(flags)
            if i is not None:
                segs[s].state0 = self._state0[i].data_ptr()
                segs[s].state1 = self._state1[i].data_ptr() if two else None
                segs[s].group = self._group_of[i]
                self._seg_of_param[i] = s
                self._param_rows.append((s, src))
        cfg = _lib.yl_train_cfg()
        cfg.kind, cfg.amp = KINDS[optimizer], int(self.amp)
        cfg.growth_interval, cfg.chunk_elems = int(sk["growth_interval"]), int(chunk_elems or 0)
        cfg.init_scale = float(sk["init_scale"])
        cfg.growth_factor, cfg.backoff_factor = float(sk["growth_factor"]), float(sk["backoff_factor"])
        self._state = torch.zeros(_lib.YL_TRAIN_STATE_WORDS, dtype=torch.float32, device=self.device)
        h = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _lib.check(self.lib.yl_train_create(idx, C.byref(cfg), segs, self._nseg, self._state.data_ptr(), C.byref(h)),
                   what="yl_train_create (fp32 tensors at 4-byte boundaries only)")
        self._h = h
        self._scale = self._state[0]
        self._norm = self._state[2]
        self._grads = (C.c_void_p * self._nseg)()
        self._hyper = _lib.yl_train_hyper()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self.lib.yl_train_destroy(h)
            self._h = None

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    # ---- the five replaced lines
    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        """loss * scale, the scale read from device memory (GradScaler.scale); the identity without amp"""
        return loss * self._scale if self.amp else loss

    def zero_grad(self, set_to_none: bool = True):
        if set_to_none:
            for p in self.params:
                p.grad = None
        else:
            gs = [p.grad for p in self.params if p.grad is not None]
            if gs:
                torch._foreach_zero_(gs)

    def step(self) -> torch.Tensor:
        """unscale, clip, optimizer step, scaler update and EMA update.  Returns the total gradient norm (before
        clipping, after unscaling) as a 0-dim device tensor that the next call overwrites."""
        grads, dev, f32 = self._grads, self.device, torch.float32
        for s, p in self._param_rows:
            g = p.grad
            if g is None:
                grads[s] = None
                continue
            if g.dtype is not f32 or not g.is_contiguous() or g.device != dev or g.shape != p.shape:
                raise _lib.YoloLiteHipError("FusedTrainStep.step: a gradient is not a contiguous fp32 tensor of its "
                                            "parameter's shape and device")
            grads[s] = g.data_ptr()
        stream = self._stream()
        _lib.check(self.lib.yl_train_set_grads(self._h, grads, stream), what="yl_train_set_grads")
        self.updates += 1
        h = self._hyper
        for gi, g in enumerate(self.param_groups):
            h.lr[gi], h.weight_decay[gi] = float(g["lr"]), float(g["weight_decay"])
        h.beta1, h.beta2, h.eps = self.betas[0], self.betas[1], self.eps
        h.momentum, h.nesterov = self.momentum, int(self.nesterov)
        h.ema_decay = ema_decay_at(self.updates, self.ema_decay, self.total_updates)
        h.max_norm = self.grad_clip
        _lib.check(self.lib.yl_train_step(self._h, C.byref(h), stream), what="yl_train_step")
        return self._norm

    # ---- state
    def _read(self):
        sc, nm = C.c_float(), C.c_float()
        tr, fi = C.c_int32(), C.c_int32()
        steps = np.zeros((self._nseg,), np.float32)
        _lib.check(self.lib.yl_train_read_state(self._h, C.byref(sc), C.byref(tr), C.byref(nm), C.byref(fi),
                                                steps.ctypes.data_as(C.POINTER(C.c_float))), what="yl_train_read_state")
        return sc.value, tr.value, nm.value, fi.value, steps

    def get_scale(self) -> float:
        """the current loss scale; synchronises -- for logging only"""
        return self._read()[0]

    def read_state(self) -> dict:
        """scale, growth tracker, norm and found_inf of the last step and every parameter's step count; synchronises"""
        sc, tr, nm, fi, steps = self._read()
        return {"scale": sc, "_growth_tracker": tr, "norm": nm, "found_inf": bool(fi),
                "steps": [float(steps[s]) for s in self._seg_of_param]}

    def state_dict(self) -> dict:
        sc, tr, _, _, steps = self._read()
        index = {id(p): i for i, p in enumerate(self.params)}
        groups = [dict(g, params=[index[id(p)] for p in g["params"] if id(p) in index]) for g in self.param_groups]
        return build_state_dict(self.optimizer, groups, [steps[s] for s in self._seg_of_param], self._state0,
                                self._state1, sc, tr, self.updates)

    def load_state_dict(self, sd: dict):
        steps, tensors, opts, scale, tracker, updates = parse_state_dict(sd, self.optimizer, len(self.params))
        if len(opts) != len(self.param_groups):
            raise ValueError(f"state_dict has {len(opts)} parameter groups, this step has {len(self.param_groups)}")
        for i in range(len(self.params)):
            a, b = tensors.get(i, (None, None))
            for dst, src in ((self._state0[i], a), (self._state1[i], b)):
                if dst is None:
                    continue
                if src is None:
                    dst.zero_()
                else:
                    dst.copy_(src.to(dtype=torch.float32).reshape(dst.shape))
        seg_steps = np.zeros((self._nseg,), np.float32)
        for i, s in enumerate(self._seg_of_param):
            seg_steps[s] = steps[i]
        _lib.check(self.lib.yl_train_write_state(self._h, scale, tracker,
                                                 seg_steps.ctypes.data_as(C.POINTER(C.c_float))),
                   what="yl_train_write_state")
        for g, o in zip(self.param_groups, opts):
            g.update(o)
        self.updates = updates
