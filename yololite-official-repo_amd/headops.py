"""Trainable detection heads on the device: the reference's make_head / _forward_head with a backward pass.

    heads = DetectHeads(fpn_channels, num_classes, num_anchors_per_level, head_depth)     # or .from_state_dict(meta, sd)
    levels = heads(model.pyramid(x), layout="nhwc")     # [B,A,S,S,5+C] per level, as model(x) returns them
    loss, _ = LossAF(..., grad=True)(levels, targets)
    loss.backward()                            # .grad of every head parameter that requires grad
        <- scripts/model/model_v2.py:23-53 (DWConvBlock, make_head), :7-14 (init_detect_bias), :182-192 (_forward_head)

The module's parameters and buffers carry the reference's names and shapes (`head3.trunk.0.block.0.weight`, ...,
`head3.out.cls.bias`), so state_dict() merges into a reference checkpoint, load_state_dict() takes one and
FusedTrainStep takes parameters().  Every level runs through one torch.autograd.Function whose forward and backward
are yl_head_forward / yl_head_backward (csrc/yl_head.hip); the kernels read the parameters where torch keeps them.
train() / eval() select the BatchNorm mode.  Gradients nobody asked for are not computed (`last_launches` says what
ran).  One forward per level is held for backward at a time: a second forward before backward() replaces it, and the
stale backward raises.  fp32 on one HIP device; no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import torch
from torch import nn

from . import _lib

def plan(fpn_channels: int, num_classes: int, num_anchors: int, head_depth: int, batch: int, size: int,
         num_masks: int = 0) -> Dict[str, int]:
    """yl_head_plan: how one level's rows are cut and what the handle holds for it (a host function; no device)."""
    if int(fpn_channels) % 4 or int(fpn_channels) < 4:
        raise _lib.YoloLiteHipError(f"fpn_channels must be a multiple of 4, got {fpn_channels}")
    if int(num_masks):
        raise _lib.YoloLiteHipError("mask-coefficient heads (num_masks > 0) are not implemented")
    if not 1 <= int(head_depth) <= _lib.YL_HEAD_MAX_DEPTH:
        raise _lib.YoloLiteHipError(f"head_depth must be 1..{_lib.YL_HEAD_MAX_DEPTH}")
    cfg = _cfg(fpn_channels, num_classes, num_anchors, head_depth)
    out = _lib.yl_head_plan_info()
    _lib.check(_lib.load().yl_head_plan(C.byref(cfg), int(batch), int(size), C.byref(out)), what="yl_head_plan")
    return {n: int(getattr(out, n)) for n, _ in out._fields_ if n != "reserved0"}


def _cfg(F, nc, A, depth):
    c = _lib.yl_head_cfg()
    c.channels, c.num_classes, c.num_anchors, c.head_depth, c.num_masks = int(F), int(nc), int(A), int(depth), 0
    return c


def _make_head(A: int, depth: int, nc: int, F: int) -> nn.ModuleDict:
    """Containers only: the layers hold the parameters under the reference's names; their own forward is never called."""
    def block():
        m = nn.Module()
        m.block = nn.Sequential(nn.Conv2d(F, F, 3, padding=1, groups=F, bias=False), nn.Conv2d(F, F, 1, bias=False),
                                nn.BatchNorm2d(F), nn.ReLU(inplace=True))
        return m
    return nn.ModuleDict({"trunk": nn.Sequential(*[block() for _ in range(depth)]),
                          "out": nn.ModuleDict({"box": nn.Conv2d(F, A * 4, 1), "obj": nn.Conv2d(F, A, 1),
                                                "cls": nn.Conv2d(F, A * nc, 1)})})


def init_detect_bias(head: nn.ModuleDict, num_classes: int, p_obj: float = 0.01):
    with torch.no_grad():
        head["out"]["obj"].bias.fill_(-math.log((1 - p_obj) / p_obj))
        head["out"]["cls"].bias.fill_(-math.log(num_classes) if num_classes > 1 else 0.0)
        head["out"]["box"].bias.zero_()


class _Level:
    """One level's handle and the order its tensors go to the library in"""

    def __init__(self, F: int, nc: int, A: int, depth: int):
        self.F, self.nc, self.A, self.depth = F, nc, A, depth
        self.handle, self.lib, self.device = None, None, None
        self.generation = 0
        self.last_launches = {"forward": 0, "backward": 0}

    def held(self) -> Dict[str, int]:
        """yl_head_held: bytes the handle holds now and whether a forward is held for backward"""
        if self.handle is None:
            return {"saved_bytes": 0, "workspace_bytes": 0, "forward_held": 0}
        sb, wb, fv = C.c_int64(), C.c_int64(), C.c_int32()
        _lib.check(self.lib.yl_head_held(self.handle, C.byref(sb), C.byref(wb), C.byref(fv)), what="yl_head_held")
        return {"saved_bytes": int(sb.value), "workspace_bytes": int(wb.value), "forward_held": int(fv.value)}

    def __deepcopy__(self, memo):                          # a copied module (an EMA) gets a handle of its own
        return _Level(self.F, self.nc, self.A, self.depth)

    def __reduce__(self):
        return _Level, (self.F, self.nc, self.A, self.depth)

    @staticmethod
    def params(head: nn.ModuleDict) -> List[torch.Tensor]:
        """block t: dw, pw, gamma, beta (4 each), then box_w, box_b, obj_w, obj_b, cls_w, cls_b"""
        out = []
        for blk in head["trunk"]:
            s = blk.block
            out += [s[0].weight, s[1].weight, s[2].weight, s[2].bias]
        o = head["out"]
        return out + [o["box"].weight, o["box"].bias, o["obj"].weight, o["obj"].bias, o["cls"].weight, o["cls"].bias]

    @staticmethod
    def buffers(head: nn.ModuleDict):
        return [(blk.block[2].running_mean, blk.block[2].running_var, blk.block[2].num_batches_tracked)
                for blk in head["trunk"]]

    def table(self, tensors: Sequence[Optional[torch.Tensor]], buffers=None):
        """yl_head_tensors from a list in params() order (None = NULL)"""
        t = _lib.yl_head_tensors()
        ptr = lambda v: v.data_ptr() if v is not None else None       # noqa: E731
        for k in range(self.depth):
            b = t.block[k]
            b.dw, b.pw, b.gamma, b.beta = (ptr(v) for v in tensors[4 * k:4 * k + 4])
            if buffers is not None:
                b.running_mean, b.running_var, b.num_batches_tracked = (ptr(v) for v in buffers[k])
        o = 4 * self.depth
        t.box_w, t.box_b, t.obj_w, t.obj_b, t.cls_w, t.cls_b = (ptr(v) for v in tensors[o:o + 6])
        return t

    def ensure(self, device: torch.device):
        if self.handle is not None and self.device == device:
            return
        self.close()
        self.lib = _lib.load()
        h = C.c_void_p()
        cfg = _cfg(self.F, self.nc, self.A, self.depth)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        _lib.check(self.lib.yl_head_create(idx, C.byref(cfg), C.byref(h)), what="yl_head_create")
        self.handle, self.device = h, device

    def close(self):
        if self.handle:
            self.lib.yl_head_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _aligned(t: torch.Tensor) -> torch.Tensor:
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


class _HeadFunction(torch.autograd.Function):
    """level tensor = head(x NHWC, parameters): yl_head_forward / yl_head_backward"""

    @staticmethod
    def forward(fctx, lv: _Level, bufs, train: bool, grad_mode: bool, x, *params):
        B, S = int(x.shape[0]), int(x.shape[1])
        # needs_input_grad reports requires_grad whatever the grad mode, and inside a Function's forward the mode is
        # always off: the caller says whether a graph is being recorded.  Without one nothing is saved.
        save = grad_mode and any(fctx.needs_input_grad)
        xd = _aligned(x.detach())
        ps = [p.detach() for p in params]
        for p in ps:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != x.device:
                raise _lib.YoloLiteHipError("DetectHeads: parameters must be contiguous fp32 tensors on the input's device")
        y = torch.empty((B, lv.A, S, S, 5 + lv.nc), device=x.device, dtype=torch.float32)
        n = C.c_int32()
        flags = (_lib.YL_HEAD_TRAIN if train else 0) | (_lib.YL_HEAD_SAVE if save else 0)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(lv.lib.yl_head_forward(lv.handle, C.byref(lv.table(ps, bufs)), xd.data_ptr(), B, S, flags,
                                          y.data_ptr(), stream, C.byref(n)), what="yl_head_forward")
        lv.generation += 1
        lv.last_launches["forward"] = int(n.value)
        if save:
            fctx.save_for_backward(xd, *params)
            fctx.lv, fctx.bufs, fctx.generation, fctx.shape = lv, bufs, lv.generation, (B, S)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, gy):
        lv = fctx.lv
        if fctx.generation != lv.generation:
            raise _lib.YoloLiteHipError("DetectHeads: this level ran another forward since the one backward() belongs to "
                                        "(one forward per level is held at a time)")
        xd, *params = fctx.saved_tensors
        B, S = fctx.shape
        need = fctx.needs_input_grad
        gy = gy.to(dtype=torch.float32).contiguous()
        grads = [torch.empty_like(p, memory_format=torch.contiguous_format) if need[5 + i] else None
                 for i, p in enumerate(params)]
        dx = torch.empty_like(xd) if need[4] else None
        n = C.c_int32()
        stream = torch.cuda.current_stream(xd.device).cuda_stream
        ps = [p.detach() for p in params]
        _lib.check(lv.lib.yl_head_backward(lv.handle, C.byref(lv.table(ps, fctx.bufs)), C.byref(lv.table(grads)),
                                           xd.data_ptr(), gy.data_ptr(), dx.data_ptr() if dx is not None else None,
                                           B, S, stream, C.byref(n)), what="yl_head_backward")
        lv.last_launches["backward"] = int(n.value)
        return (None, None, None, None, dx) + tuple(grads)


class DetectHeads(nn.Module):
    """See the module docstring.  `num_anchors_per_level`: one int per level (or one int for all)."""

    def __init__(self, fpn_channels: int, num_classes: int, num_anchors_per_level=1, head_depth: int = 1,
                 level_names: Sequence[str] = ("p3", "p4", "p5"), num_masks: int = 0):
        super().__init__()
        F, nc, depth = int(fpn_channels), int(num_classes), int(head_depth)
        if int(num_masks):
            raise _lib.YoloLiteHipError("mask-coefficient heads (num_masks > 0) are not implemented")
        if F < 4 or F % 4:
            raise _lib.YoloLiteHipError(f"fpn_channels must be a multiple of 4, got {F}")
        if not 1 <= depth <= _lib.YL_HEAD_MAX_DEPTH:
            raise _lib.YoloLiteHipError(f"head_depth must be 1..{_lib.YL_HEAD_MAX_DEPTH}, got {depth}")
        if nc < 1:
            raise _lib.YoloLiteHipError("num_classes must be at least 1")
        self.level_names = tuple(level_names)
        apl = num_anchors_per_level
        apl = (int(apl),) * len(self.level_names) if isinstance(apl, int) else tuple(int(a) for a in apl)
        if len(apl) != len(self.level_names) or min(apl) < 1:
            raise ValueError(f"{len(self.level_names)} levels but anchors {apl}")
        self.fpn_channels, self.num_classes, self.head_depth, self.num_anchors_per_level = F, nc, depth, apl
        self._levels: List[_Level] = []
        for n, A in zip(self.level_names, apl):
            head = _make_head(A, depth, nc, F)
            init_detect_bias(head, nc)
            setattr(self, "head" + n[1:], head)
            self._levels.append(_Level(F, nc, A, depth))

    @classmethod
    def from_meta(cls, meta: dict, num_classes: Optional[int] = None) -> "DetectHeads":
        """freshly initialised heads of the model `meta` describes (program.build_program reads the same keys)"""
        cfg = meta.get("config", {}) or {}
        mcfg, tcfg = cfg.get("model", {}) or {}, cfg.get("training", {}) or {}
        if mcfg.get("seg"):
            raise _lib.YoloLiteHipError("mask-coefficient heads (num_masks > 0) are not implemented")
        nc = int(num_classes or meta.get("num_classes") or mcfg.get("num_classes") or 80)
        F = int(int(mcfg.get("fpn_channels", 128)) * float(mcfg.get("width_multiple", 1.0)))
        names = (["p2"] if tcfg.get("use_p2") else []) + ["p3", "p4", "p5"] + (["p6"] if tcfg.get("use_p6") else [])
        apl = tuple(meta.get("num_anchors_per_level") or (1, 1, 1))
        if len(apl) >= 3:
            amap = dict(p2=apl[0], p3=apl[0], p4=apl[1], p5=apl[2], p6=apl[2])
        else:
            amap = dict.fromkeys(("p2", "p3", "p4", "p5", "p6"), apl[0] if apl else 1)
        return cls(F, nc, tuple(int(amap[n]) for n in names), int(mcfg.get("head_depth", 1)), level_names=names)

    @classmethod
    def from_state_dict(cls, meta: dict, sd: dict) -> "DetectHeads":
        """the heads of a checkpoint: built from its meta, filled with its `head*.` entries (tensors or numpy arrays)"""
        m = cls.from_meta(meta)
        own = m.state_dict()
        missing = [k for k in own if k not in sd and not k.endswith("num_batches_tracked")]
        if missing:
            raise KeyError(f"checkpoint lacks head entries: {missing[:4]}")
        m.load_state_dict({k: torch.as_tensor(sd[k]).reshape(v.shape).to(v.dtype) for k, v in own.items() if k in sd},
                          strict=False)
        return m

    def last_launches(self) -> List[Dict[str, int]]:
        """kernels enqueued by the last forward / backward of every level"""
        return [dict(lv.last_launches) for lv in self._levels]

    def held(self) -> List[Dict[str, int]]:
        """per level: the bytes its handle holds on the device and whether a forward is held for backward"""
        return [lv.held() for lv in self._levels]

    def forward(self, feats: Sequence[torch.Tensor], layout: Optional[str] = None) -> List[torch.Tensor]:
        """`layout`: "nchw" ([B,F,S,S], any strides) or "nhwc" ([B,S,S,F]) for every map; None reads it off each map's
        shape and refuses the one shape that is both ([B,F,F,F])."""
        feats = list(feats)
        if layout not in (None, "nchw", "nhwc"):
            raise ValueError(f"layout must be 'nchw', 'nhwc' or None, got {layout!r}")
        if len(feats) != len(self._levels):
            raise ValueError(f"expected {len(self._levels)} feature maps, got {len(feats)}")
        F = self.fpn_channels
        xs = []
        for f in feats:                                    # host-side facts first, the device last
            if not torch.is_tensor(f) or f.dim() != 4:
                raise ValueError("feature maps must be 4-d tensors [B,F,S,S] or [B,S,S,F]")
            nchw = f.shape[1] == F and f.shape[2] == f.shape[3]
            nhwc = f.shape[3] == F and f.shape[1] == f.shape[2]
            if layout is None and nchw and nhwc:
                raise ValueError(f"feature map {tuple(f.shape)} reads as [B,{F},S,S] and as [B,S,S,{F}]: "
                                 "pass layout='nchw' or layout='nhwc'")
            if not (nchw if layout == "nchw" else nhwc if layout == "nhwc" else nchw or nhwc):
                want = {None: f"neither [B,{F},S,S] nor [B,S,S,{F}]", "nchw": f"not [B,{F},S,S]", "nhwc": f"not [B,S,S,{F}]"}
                raise ValueError(f"feature map {tuple(f.shape)} is {want[layout]}")
            if layout == "nchw" or (layout is None and nchw):
                f = f.permute(0, 2, 3, 1)                  # NCHW -> an NHWC view (channels-last memory: already contiguous)
            if not f.is_cuda:
                raise _lib.YoloLiteHipError("DetectHeads needs its inputs on a HIP device (no CPU fallback)")
            if self.training and f.shape[0] * f.shape[1] * f.shape[2] == 1:
                raise ValueError("Expected more than 1 value per channel when training, got input size "
                                 f"{[int(f.shape[0]), F, 1, 1]}")
            xs.append(f)
        outs = []
        for lv, n, f in zip(self._levels, self.level_names, xs):
            head = getattr(self, "head" + n[1:])
            params = lv.params(head)
            if any(p.device != f.device for p in params):
                raise _lib.YoloLiteHipError("DetectHeads: parameters and inputs must live on one HIP device")
            lv.ensure(f.device)
            x = f.float().contiguous()                     # autograd carries the gradient back through cast and copy
            outs.append(_HeadFunction.apply(lv, lv.buffers(head), self.training, torch.is_grad_enabled(), x, *params))
        return outs
