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
from . import _trainmod as tm


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
    return nn.ModuleDict({"trunk": nn.Sequential(*[tm.dw_block(F, 1) for _ in range(depth)]),
                          "out": nn.ModuleDict({"box": nn.Conv2d(F, A * 4, 1), "obj": nn.Conv2d(F, A, 1),
                                                "cls": nn.Conv2d(F, A * nc, 1)})})


def init_detect_bias(head: nn.ModuleDict, num_classes: int, p_obj: float = 0.01):
    with torch.no_grad():
        head["out"]["obj"].bias.fill_(-math.log((1 - p_obj) / p_obj))
        head["out"]["cls"].bias.fill_(-math.log(num_classes) if num_classes > 1 else 0.0)
        head["out"]["box"].bias.zero_()


class _Level(tm.DeviceHandle):
    """One level's handle (see _trainmod.DeviceHandle) and the order its tensors go to the library in"""

    def __init__(self, F: int, nc: int, A: int, depth: int):
        super().__init__("yl_head", _cfg, F, nc, A, depth)
        self.nc, self.A, self.depth = nc, A, depth

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
        for k in range(self.depth):
            tm.fill_block(t.block[k], tensors[4 * k:4 * k + 4], buffers[k] if buffers is not None else None)
        o = 4 * self.depth
        t.box_w, t.box_b, t.obj_w, t.obj_b, t.cls_w, t.cls_b = (tm.ptr(v) for v in tensors[o:o + 6])
        return t


class _HeadFunction(torch.autograd.Function):
    """level tensor = head(x NHWC, parameters): yl_head_forward / yl_head_backward"""

    @staticmethod
    def forward(fctx, lv: _Level, bufs, train: bool, grad_mode: bool, x, *params):
        B, S = int(x.shape[0]), int(x.shape[1])
        save = tm.saving(fctx, grad_mode)
        xd = tm.aligned(x.detach())
        ps = tm.detached_params("DetectHeads", params, x.device)
        y = torch.empty((B, lv.A, S, S, 5 + lv.nc), device=x.device, dtype=torch.float32)
        lv.launch("forward", x.device, C.byref(lv.table(ps, bufs)), xd.data_ptr(), B, S, tm.flags(train, save), y.data_ptr())
        if save:
            fctx.save_for_backward(xd, *params)
            fctx.lv, fctx.bufs, fctx.generation, fctx.shape = lv, bufs, lv.generation, (B, S)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, gy):
        lv = fctx.lv
        lv.check_generation(fctx.generation, "DetectHeads: this level", "one forward per level")
        xd, *params = fctx.saved_tensors
        B, S = fctx.shape
        gy = gy.to(dtype=torch.float32).contiguous()
        dx, *grads = tm.grads_like([xd, *params], fctx.needs_input_grad[4:])
        ps = [p.detach() for p in params]
        lv.launch("backward", xd.device, C.byref(lv.table(ps, fctx.bufs)), C.byref(lv.table(grads)), xd.data_ptr(),
                  gy.data_ptr(), tm.ptr(dx), B, S)
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
        F, names, mcfg, _ = tm.meta_fpn(meta)
        if mcfg.get("seg"):
            raise _lib.YoloLiteHipError("mask-coefficient heads (num_masks > 0) are not implemented")
        nc = int(num_classes or meta.get("num_classes") or mcfg.get("num_classes") or 80)
        apl = tuple(meta.get("num_anchors_per_level") or (1, 1, 1))
        if len(apl) >= 3:
            amap = dict(p2=apl[0], p3=apl[0], p4=apl[1], p5=apl[2], p6=apl[2])
        else:
            amap = dict.fromkeys(("p2", "p3", "p4", "p5", "p6"), apl[0] if apl else 1)
        return cls(F, nc, tuple(int(amap[n]) for n in names), int(mcfg.get("head_depth", 1)), level_names=names)

    @classmethod
    def from_state_dict(cls, meta: dict, sd: dict) -> "DetectHeads":
        """the heads of a checkpoint: built from its meta, filled with its `head*.` entries (tensors or numpy arrays)"""
        return tm.fill_from_state_dict(cls.from_meta(meta), sd, "head")

    def last_launches(self) -> List[Dict[str, int]]:
        """kernels enqueued by the last forward / backward of every level"""
        return [dict(lv.last_launches) for lv in self._levels]

    def held(self) -> List[Dict[str, int]]:
        """per level: the bytes its handle holds on the device and whether a forward is held for backward"""
        return [lv.held() for lv in self._levels]

    def forward(self, feats: Sequence[torch.Tensor], layout: Optional[str] = None) -> List[torch.Tensor]:
        """`layout`: "nchw" ([B,F,S,S], any strides) or "nhwc" ([B,S,S,F]) for every map; None reads it off each map's
        shape and refuses the one shape that is both ([B,F,F,F])."""
        feats = tm.check_layout(layout, feats, len(self._levels))
        xs = [tm.as_nhwc(f, self.fpn_channels, layout, "DetectHeads", self.training) for f in feats]
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
