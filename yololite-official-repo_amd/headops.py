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
stale backward raises.  One HIP device; no CPU fallback.

Mixed precision (the reference's AMP, tools/train.py:284-357): DetectHeads(..., precision="fp16" | "bf16"), or
`heads.precision = ...` at any time, runs every 1x1 GEMM of the heads -- the trunk blocks' z = d . W1^T, dd = dz . W1,
dW1 = dz^T . d and the outputs' y = h . Wout^T, dh = gy . Wout, dWout = gy^T . h -- with both operands rounded to that
type (nearest even) and fp32 accumulation on the 16-bit MFMA.  Parameters, gradients, the saved activations, the
depthwise 3x3, BatchNorm, the bias and every ordered float64 sum stay fp32; the launch counts are the same.  Nothing is
clamped: a value beyond fp16's range becomes inf and the gradients it reaches are not finite, which is what
FusedTrainStep's loss-scale logic looks for.  A backward runs in the precision of the forward it belongs to.
head_gemm() runs one of those GEMMs on its own (yl_head_gemm).
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
        self.F, self.nc, self.A, self.depth = F, nc, A, depth
        self.mode_bits = 0                                 # yl_head_forward's precision bits: the module sets them per call

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
        lv.launch("forward", x.device, C.byref(lv.table(ps, bufs)), xd.data_ptr(), B, S,
                  tm.flags(train, save) | lv.mode_bits, y.data_ptr())
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
                 level_names: Sequence[str] = ("p3", "p4", "p5"), num_masks: int = 0, precision: str = "fp32"):
        super().__init__()
        tm.check_precision(precision)
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
        self.precision = precision

    @property
    def precision(self) -> str:
        """"fp32", "fp16" or "bf16": the operand type of the 1x1 GEMMs of the forwards to come (and of their backwards)"""
        return self._precision

    @precision.setter
    def precision(self, value: str):
        self._precision = tm.check_precision(value)

    @classmethod
    def from_meta(cls, meta: dict, num_classes: Optional[int] = None, precision: str = "fp32") -> "DetectHeads":
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
        return cls(F, nc, tuple(int(amap[n]) for n in names), int(mcfg.get("head_depth", 1)), level_names=names,
                   precision=precision)

    @classmethod
    def from_state_dict(cls, meta: dict, sd: dict, precision: str = "fp32") -> "DetectHeads":
        """the heads of a checkpoint: built from its meta, filled with its `head*.` entries (tensors or numpy arrays)"""
        return tm.fill_from_state_dict(cls.from_meta(meta, precision=precision), sd, "head")

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
            lv.mode_bits = tm.PRECISIONS[self._precision]
            x = f.float().contiguous()                     # autograd carries the gradient back through cast and copy
            outs.append(_HeadFunction.apply(lv, lv.buffers(head), self.training, torch.is_grad_enabled(), x, *params))
        return outs


PASSES = {"forward": _lib.YL_HEAD_PASS_FORWARD, "dgrad": _lib.YL_HEAD_PASS_DGRAD, "wgrad": _lib.YL_HEAD_PASS_WGRAD}


def head_gemm(heads: DetectHeads, level: int, site, pass_: str, a: torch.Tensor, b: Optional[torch.Tensor] = None,
              precision: Optional[str] = None):
    """One 1x1 GEMM of level `level` (an index into heads.level_names) on its own, launched as the module launches it
    (yl_head_gemm), with that level's weights read where torch keeps them.  `site`: a trunk block's index or "out", the
    three output convolutions.  fp32 tensors on the heads' HIP device:
        site t, "forward":  a = d  [B,S,S,F]                 -> z  [B,S,S,F]          = d . W1^T
        site t, "dgrad":    a = dz [B,S,S,F]                 -> dd [B,S,S,F]          = dz . W1
        site t, "wgrad":    a = d  [B,S,S,F], b = dz [B,S,S,F] -> dW1 [F,F,1,1]        = dz^T . d
        "out",  "forward":  a = h  [B,S,S,F]                 -> y  [B,A,S,S,5+C]      = h . Wout^T + bias
        "out",  "dgrad":    a = gy [B,A,S,S,5+C]             -> dh [B,S,S,F]          = gy . Wout
        "out",  "wgrad":    a = h  [B,S,S,F], b = gy [B,A,S,S,5+C] -> (dbox_w, dobj_w, dcls_w)
    `precision`: both operands are rounded to it (nearest even), fp32 accumulation; None: the heads' own.  Uses the
    level's handle: if its workspace has to grow for the call, a forward it holds for backward is dropped and that
    backward raises."""
    if not isinstance(heads, DetectHeads):
        raise ValueError("`heads` must be a DetectHeads")
    if isinstance(level, bool) or not isinstance(level, int) or not 0 <= level < len(heads._levels):
        raise ValueError(f"level must be an index 0..{len(heads._levels) - 1}, got {level!r}")
    out_site = isinstance(site, str) and site == "out"
    if not out_site and (isinstance(site, bool) or not isinstance(site, int) or not 0 <= site < heads.head_depth):
        raise ValueError(f"site must be a block index 0..{heads.head_depth - 1} or 'out', got {site!r}")
    if not isinstance(pass_, str) or pass_ not in PASSES:
        raise ValueError(f"pass_ must be one of {sorted(PASSES)}, got {pass_!r}")
    precision = tm.check_precision(heads.precision if precision is None else precision)
    lv, F = heads._levels[level], heads.fpn_channels
    E = 5 + lv.nc
    level_in = out_site and pass_ == "dgrad"               # `a` is the level tensor
    if not torch.is_tensor(a) or a.dim() != (5 if level_in else 4):
        raise ValueError("the first operand must be " + ("[B,A,S,S,5+C]" if level_in else "[B,S,S,F]"))
    B, S = int(a.shape[0]), int(a.shape[2])
    rows, lvl = (B, S, S, F), (B, lv.A, S, S, E)
    if tuple(a.shape) != (lvl if level_in else rows) or B < 1 or S < 1:
        raise ValueError(f"the first operand of {pass_!r} must be {lvl if level_in else rows}, got {tuple(a.shape)}")
    if pass_ == "wgrad":
        want = lvl if out_site else rows
        if not torch.is_tensor(b) or tuple(b.shape) != want:
            raise ValueError(f"the second operand of 'wgrad' must be {want}")
    elif b is not None:
        raise ValueError(f"{pass_!r} takes one operand")
    if not a.is_cuda or (b is not None and b.device != a.device):
        raise _lib.YoloLiteHipError("head_gemm needs its operands on one HIP device (no CPU fallback)")
    head = getattr(heads, "head" + heads.level_names[level][1:])
    ps = tm.detached_params("DetectHeads", lv.params(head), a.device)
    lv.ensure(a.device)
    ad = tm.aligned(a.detach().float().contiguous())
    bd = tm.aligned(b.detach().float().contiguous()) if b is not None else None
    NE = lv.A * E
    if pass_ == "wgrad":
        out = torch.empty((NE, F) if out_site else (F, F, 1, 1), device=a.device, dtype=torch.float32)
    else:
        out = torch.empty(lvl if out_site and pass_ == "forward" else rows, device=a.device, dtype=torch.float32)
    n = C.c_int32()
    lv.call("gemm", _lib.YL_HEAD_SITE_OUT if out_site else site, PASSES[pass_], tm.PRECISIONS[precision],
            C.byref(lv.table(ps, lv.buffers(head))), ad.data_ptr(), tm.ptr(bd), out.data_ptr(), B, S,
            torch.cuda.current_stream(a.device).cuda_stream, C.byref(n))
    if out_site and pass_ == "wgrad":                      # the rows of box_w, obj_w, cls_w one after the other
        A, nc = lv.A, lv.nc
        return (out[:4 * A].reshape(4 * A, F, 1, 1), out[4 * A:5 * A].reshape(A, F, 1, 1),
                out[5 * A:].reshape(A * nc, F, 1, 1))
    return out
