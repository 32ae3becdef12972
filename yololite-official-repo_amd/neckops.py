"""Trainable FPN necks on the device: the laterals, the top-down upsample-add chain and the smooth blocks of the
reference's two architectures, with a backward pass.

    DetectNeck      arch YOLOLiteMS_CPU: smooth block = depthwise 3x3 -> 1x1 -> BatchNorm -> ReLU   (csrc/yl_neck.hip)
    DetectNeckMS    arch YOLOLiteMS (the default arch): dense 3x3 -> BatchNorm -> SiLU              (csrc/yl_dneck.hip)
    neck_for(meta, sd=None, precision="fp32")   the right class's instance for a model's meta (from_state_dict with `sd`,
                                                else from_meta)
    conv3x3(x, w_or_dz, pass_, precision)       one 3x3 GEMM of DetectNeckMS on its own (yl_dneck_conv3x3)

    neck = DetectNeck(in_channels, fpn_channels, depth)          # or .from_meta(meta) / .from_state_dict(meta, sd)
    ps = neck(model.features(x))                                 # NHWC [B,S,S,F] per level, finest first
    levels = heads(ps, layout="nhwc")
    loss.backward()                 # .grad of every neck parameter that requires grad, and of the feature maps' if they do
        <- scripts/model/model_v2.py:23-39 (DWConvBlock), :285-294 (lateral*, smooth*), :337-361 (_upsample_add, forward)

The parameters and buffers carry the reference's names and shapes (`lateral3.weight`, `smooth3.block.0.weight`, ...,
`smooth5.block.{4i+2}.running_var`), so state_dict() merges into a reference checkpoint and FusedTrainStep takes
parameters().  The whole neck is ONE torch.autograd.Function (yl_neck_forward / yl_neck_backward, csrc/yl_neck.hip): the
top-down chain is internal to it and autograd hands it the gradient of every p_k.  train() / eval() select the BatchNorm
mode.  Gradients nobody asked for are not computed (`last_launches` says what ran).  One forward is held for backward
at a time: a second forward before backward() replaces it, and the stale backward raises.  fp32 on one HIP device; no
CPU fallback.  Not implemented, and refused: the P6 path (`use_p6`); DetectNeck refuses arch YOLOLiteMS and DetectNeckMS
refuses arch YOLOLiteMS_CPU, each naming the other.

DetectNeckMS is the same module around the other block (model_v2.py:15-22 conv_block, :115-127, :194-203): its entries are
`lateral{k}.weight/bias`, `smooth{k}.{3i}.weight` [F,F,3,3] and `smooth{k}.{3i+1}.weight/bias/running_mean/running_var/
num_batches_tracked` (conv_block is a plain nn.Sequential: no `.block.` level), one autograd.Function over
yl_dneck_forward / yl_dneck_backward.  The 3x3 convolution runs forward, input gradient and weight gradient on fp32 MFMA.

Mixed precision (the reference's AMP, tools/train.py:284-357): DetectNeckMS(..., precision="fp16" | "bf16"), or
`neck.precision = ...` at any time, runs the three 3x3 GEMMs with both operands rounded to that type (nearest even) and fp32
accumulation on 16-bit MFMA; everything else, the parameters and every returned gradient stay fp32.  Nothing is clamped:
an operand beyond fp16's range becomes inf and the gradients are not finite, which is what FusedTrainStep's found-inf /
loss-scale logic looks for.  A backward runs in the precision of the forward it belongs to.  DetectNeck refuses it: the
depthwise neck has no dense 3x3 GEMM, and its 1x1 is the heads' fp32 GEMM.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib
from . import _trainmod as tm


PRECISIONS = tm.PRECISIONS                                 # -> yl_dneck_forward's flag bits (YL_DNECK_F16 / _BF16)
_check_precision = tm.check_precision


def _check_dims(in_channels, F, depth):
    in_channels = tuple(int(c) for c in in_channels)
    if int(F) < 4 or int(F) % 4:
        raise _lib.YoloLiteHipError(f"fpn_channels must be a multiple of 4, got {F}")
    if any(c < 4 or c % 4 for c in in_channels):
        raise _lib.YoloLiteHipError(f"in_channels must be multiples of 4, got {in_channels}")
    if not 1 <= int(depth) <= _lib.YL_NECK_MAX_DEPTH:
        raise _lib.YoloLiteHipError(f"depth must be 1..{_lib.YL_NECK_MAX_DEPTH}, got {depth}")
    if not 1 <= len(in_channels) <= _lib.YL_NECK_MAX_LEVELS:
        raise _lib.YoloLiteHipError(f"1..{_lib.YL_NECK_MAX_LEVELS} levels, got {len(in_channels)}")
    return in_channels


def _cfg(in_channels, F, depth):
    c = _lib.yl_neck_cfg()
    c.channels, c.depth, c.num_levels = int(F), int(depth), len(in_channels)
    for k, ci in enumerate(in_channels):
        c.in_channels[k] = int(ci)
    return c


def plan(in_channels: Sequence[int], fpn_channels: int, depth: int, batch: int, sizes: Sequence[int]) -> Dict:
    """yl_neck_plan (a host function; no device): how every level's rows are cut and what the handle holds.
    -> {"stat_rows", "gemm_rows", "levels": [{rows, stat_tiles, gemm_tiles, wgrad_rows, wgrad_splits, lgrad_rows,
    lgrad_splits, saved_bytes}], "saved_bytes", "nosave_bytes", "workspace_bytes", "table_bytes"} with, for F channels,
    depth d, M_k = batch * S_k^2 rows and Mmax the largest M_k:
        levels[k].saved_bytes = (1 + 3 d) M_k F 4 + d 2 F 4              t_k; d, z, h and (mean, invstd) per block
        saved_bytes           = sum of the levels'
        nosave_bytes          = 4 Mmax F 4 + 2 F 4                        t and one block of the largest level
        workspace_bytes       = 3 Mmax F 4 + max_k(stat_tiles_k) 9 F 8 + 2 F 4
                                + max_k round16(max(wgrad_splits_k F F, lgrad_splits_k F Cin_k) 4)
        table_bytes           = sum over k < L - 1 of (S_k + 2 S_{k+1}) 4"""
    in_channels = _check_dims(in_channels, fpn_channels, depth)
    if len(sizes) != len(in_channels):
        raise ValueError(f"{len(in_channels)} levels but sizes {tuple(sizes)}")
    cfg = _cfg(in_channels, fpn_channels, depth)
    out = _lib.yl_neck_plan_info()
    sz = (C.c_int32 * len(sizes))(*[int(s) for s in sizes])
    _lib.check(_lib.load().yl_neck_plan(C.byref(cfg), int(batch), sz, C.byref(out)), what="yl_neck_plan")
    lv = [{n: int(getattr(out.level[k], n)) for n, _ in out.level[k]._fields_ if n != "reserved0"}
          for k in range(len(sizes))]
    return {"stat_rows": int(out.stat_rows), "gemm_rows": int(out.gemm_rows), "levels": lv,
            "saved_bytes": int(out.saved_bytes), "nosave_bytes": int(out.nosave_bytes),
            "workspace_bytes": int(out.workspace_bytes), "table_bytes": int(out.table_bytes)}


def nearest_map(out_size: int, in_size: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The host tables the kernels read: src[out_size] (the source index of every destination index under
    F.interpolate(mode="nearest")), and lo[in_size], hi[in_size]: source cell i is read by the destinations [lo, hi)."""
    out_size, in_size = int(out_size), int(in_size)
    if out_size < 1 or in_size < 1:
        raise ValueError("sizes must be positive")
    src = (C.c_int32 * out_size)()
    lo, hi = (C.c_int32 * in_size)(), (C.c_int32 * in_size)()
    _lib.check(_lib.load().yl_neck_nearest_map(out_size, in_size, src, lo, hi), what="yl_neck_nearest_map")
    return np.asarray(list(src), np.int64), np.asarray(list(lo), np.int64), np.asarray(list(hi), np.int64)


class _Handle(tm.DeviceHandle):
    """The neck's handle (see _trainmod.DeviceHandle) and the order its tensors go to the library in"""
    who = "DetectNeck"

    def __init__(self, in_channels, F: int, depth: int):
        super().__init__("yl_neck", _cfg, tuple(in_channels), F, depth)
        self.F, self.depth, self.L = F, depth, len(in_channels)
        self.mode_bits = 0

    @property
    def per_level(self) -> int:
        return 2 + 4 * self.depth

    def table(self, tensors: Sequence[Optional[torch.Tensor]], buffers=None):
        """yl_neck_tensors from a list in DetectNeck._param_list() order (None = NULL)"""
        t = _lib.yl_neck_tensors()
        n = self.per_level
        for k in range(self.L):
            lv, ts = t.level[k], tensors[k * n:(k + 1) * n]
            lv.lat_w, lv.lat_b = tm.ptr(ts[0]), tm.ptr(ts[1])
            for i in range(self.depth):
                tm.fill_block(lv.block[i], ts[2 + 4 * i:6 + 4 * i], buffers[k][i] if buffers is not None else None)
        return t


class _HandleMS(tm.DeviceHandle):
    """The dense neck's handle: yl_dneck_*, per level lateral weight, bias, then per block w, gamma, beta"""
    who = "DetectNeckMS"

    def __init__(self, in_channels, F: int, depth: int):
        super().__init__("yl_dneck", _cfg, tuple(in_channels), F, depth)
        self.F, self.depth, self.L = F, depth, len(in_channels)
        self.mode_bits = 0                                 # YL_DNECK_F16 / YL_DNECK_BF16 of the next forward

    @property
    def per_level(self) -> int:
        return 2 + 3 * self.depth

    def table(self, tensors: Sequence[Optional[torch.Tensor]], buffers=None):
        """yl_dneck_tensors from a list in DetectNeckMS._param_list() order (None = NULL)"""
        t = _lib.yl_dneck_tensors()
        n = self.per_level
        for k in range(self.L):
            lv, ts = t.level[k], tensors[k * n:(k + 1) * n]
            lv.lat_w, lv.lat_b = tm.ptr(ts[0]), tm.ptr(ts[1])
            for i in range(self.depth):
                b = lv.block[i]
                b.w, b.gamma, b.beta = (tm.ptr(v) for v in ts[2 + 3 * i:5 + 3 * i])
                if buffers is not None:
                    b.running_mean, b.running_var, b.num_batches_tracked = (tm.ptr(v) for v in buffers[k][i])
        return t


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[tm.ptr(t) for t in ts])


class _NeckFunction(torch.autograd.Function):
    """(p_0, ..., p_{L-1}) = neck(c_0, ..., c_{L-1} NHWC, parameters): <prefix>_forward / <prefix>_backward of the handle
    (yl_neck_* or yl_dneck_*: the two share their signatures)"""

    @staticmethod
    def forward(fctx, hd: _Handle, bufs, train: bool, grad_mode: bool, *args):
        L = hd.L
        cs, params = args[:L], args[L:]
        B = int(cs[0].shape[0])
        sizes = [int(c.shape[1]) for c in cs]
        save = tm.saving(fctx, grad_mode)
        cd = [tm.aligned(c.detach()) for c in cs]
        dev = cs[0].device
        ps = tm.detached_params(hd.who, params, dev)
        outs = [torch.empty((B, S, S, hd.F), device=dev, dtype=torch.float32) for S in sizes]
        hd.launch("forward", dev, C.byref(hd.table(ps, bufs)), _ptrs(cd), B, (C.c_int32 * L)(*sizes),
                  tm.flags(train, save) | hd.mode_bits, _ptrs(outs))
        if save:
            fctx.save_for_backward(*cd, *params)
            fctx.hd, fctx.bufs, fctx.generation, fctx.shape = hd, bufs, hd.generation, (B, sizes)
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, *gps):
        hd = fctx.hd
        hd.check_generation(fctx.generation, hd.who + ": the neck", "one forward")
        L = hd.L
        saved = fctx.saved_tensors
        cd, params = saved[:L], saved[L:]
        B, sizes = fctx.shape
        gps = [tm.aligned(g.to(dtype=torch.float32).contiguous()) for g in gps]
        grads = tm.grads_like(saved, fctx.needs_input_grad[4:])
        ps = [p.detach() for p in params]
        hd.launch("backward", cd[0].device, C.byref(hd.table(ps, fctx.bufs)), C.byref(hd.table(grads[L:])), _ptrs(cd),
                  _ptrs(gps), _ptrs(grads[:L]), B, (C.c_int32 * L)(*sizes))
        return (None, None, None, None) + tuple(grads)


def conv_block(F: int, n: int) -> nn.Module:
    """Container only (the reference's conv_block(F, F, n)): the layers hold the parameters; their forward is never called."""
    layers = []
    for _ in range(n):
        layers += [nn.Conv2d(F, F, 3, padding=1, bias=False), nn.BatchNorm2d(F), nn.SiLU(inplace=True)]
    return nn.Sequential(*layers)


def _meta_arch(meta: dict, mcfg: dict) -> str:
    return (meta.get("arch") or mcfg.get("arch") or "YOLOLiteMS").lower()


class _NeckBase(nn.Module):
    """What the two necks share: the reference constructor's order of registration, the reading of meta and checkpoint,
    and forward().  A subclass gives _who, _handle_cls, _smooth(F, depth), _meta_dims(meta), _param_list(), _bn(level
    name, block)."""

    def __init__(self, in_channels: Sequence[int], fpn_channels: int, depth: int = 1,
                 level_names: Sequence[str] = ("p3", "p4", "p5"), precision: str = "fp32"):
        super().__init__()
        in_channels = _check_dims(in_channels, fpn_channels, depth)
        self._check_precision(precision)
        self.level_names = tuple(level_names)
        if len(self.level_names) != len(in_channels):
            raise ValueError(f"{len(self.level_names)} levels but in_channels {in_channels}")
        F = int(fpn_channels)
        self.in_channels, self.fpn_channels, self.depth = in_channels, F, int(depth)
        rest = [(n, ci) for n, ci in zip(self.level_names, in_channels) if n != "p2"]
        if "p2" in self.level_names:                       # the reference's order of registration (model_v2.py:286-294)
            self.lateral2 = nn.Conv2d(in_channels[self.level_names.index("p2")], F, 1)
            self.smooth2 = self._smooth(F, self.depth)
        for n, ci in rest:
            setattr(self, "lateral" + n[1:], nn.Conv2d(ci, F, 1))
        for n, ci in rest:
            setattr(self, "smooth" + n[1:], self._smooth(F, self.depth))
        self._handle = self._handle_cls(in_channels, F, self.depth)
        self.precision = precision

    @classmethod
    def _check_precision(cls, precision) -> str:
        """the operand types this neck's GEMMs run in: a subclass without a reduced mode refuses the others"""
        return _check_precision(precision)

    @property
    def precision(self) -> str:
        """"fp32", "fp16" or "bf16": the operand type of the 3x3 GEMMs of the next forward (and of its backward)"""
        return self._precision

    @precision.setter
    def precision(self, value: str):
        self._precision = self._check_precision(value)

    @classmethod
    def from_meta(cls, meta: dict, precision: str = "fp32"):
        """a freshly initialised neck of the model `meta` describes; the input channels are those of the feature maps of
        the program build_program makes for it"""
        from .program import build_program, synth_state_dict
        F, d, names = cls._meta_dims(meta)
        prog = build_program(meta, synth_state_dict(meta))
        cin = [int(prog.slots[prog.feature_slots["c" + n[1:]]][2]) for n in names]
        return cls(cin, F, d, level_names=names, precision=precision)

    @classmethod
    def from_state_dict(cls, meta: dict, sd: dict, precision: str = "fp32"):
        """the neck of a checkpoint: built from its meta, filled with its `lateral*.` / `smooth*.` entries"""
        F, d, names = cls._meta_dims(meta)
        missing = [f"lateral{n[1:]}.weight" for n in names if f"lateral{n[1:]}.weight" not in sd]
        if missing:
            raise KeyError(f"checkpoint lacks neck entries: {missing[:4]}")
        cin = [int(np.shape(sd[f"lateral{n[1:]}.weight"])[1]) for n in names]
        return tm.fill_from_state_dict(cls(cin, F, d, level_names=names, precision=precision), sd, "neck")

    def _stat_buffers(self):
        out = []
        for n in self.level_names:
            bns = [self._bn(n, i) for i in range(self.depth)]
            out.append([(bn.running_mean, bn.running_var, bn.num_batches_tracked) for bn in bns])
        return out

    def last_launches(self) -> Dict[str, int]:
        """kernels enqueued by the last forward / backward"""
        return dict(self._handle.last_launches)

    def held(self) -> Dict[str, int]:
        """the bytes the handle holds on the device and whether a forward is held for backward"""
        return self._handle.held()

    def forward(self, feats: Sequence[torch.Tensor], layout: Optional[str] = None) -> List[torch.Tensor]:
        """`feats`: the backbone's maps, finest first, "nchw" ([B,Cin,S,S], any strides) or "nhwc" ([B,S,S,Cin]); None
        reads the layout off each map's shape and refuses a shape that is both.  -> NHWC [B,S,S,F] per level, finest
        first: what DetectHeads(..., layout="nhwc") takes."""
        feats = tm.check_layout(layout, feats, len(self.level_names))
        xs = [tm.as_nhwc(f, ci, layout, self._who, self.training, name="Cin", bn_channels=self.fpn_channels)
              for f, ci in zip(feats, self.in_channels)]
        if len({int(f.shape[0]) for f in xs}) != 1 or len({f.device for f in xs}) != 1:
            raise ValueError("the feature maps must share one batch size and one device")
        params = self._param_list()
        if any(p.device != xs[0].device for p in params):
            raise _lib.YoloLiteHipError(f"{self._who}: parameters and inputs must live on one HIP device")
        self._handle.ensure(xs[0].device)
        self._handle.mode_bits = PRECISIONS[self._precision]
        xs = [f.float().contiguous() for f in xs]          # autograd carries the gradient back through cast and copy
        return list(_NeckFunction.apply(self._handle, self._stat_buffers(), self.training, torch.is_grad_enabled(), *xs, *params))


class DetectNeck(_NeckBase):
    """See the module docstring.  `in_channels`: the channels of the feature maps, finest level first."""
    _who, _handle_cls = "DetectNeck", _Handle

    @classmethod
    def _check_precision(cls, precision) -> str:
        if _check_precision(precision) != "fp32":
            raise _lib.YoloLiteHipError(f"DetectNeck: precision {precision!r} is not implemented: the depthwise neck has no dense "
                                        "3x3 GEMM to run on 16-bit MFMA (its 3x3 is depthwise, its 1x1 is the heads' fp32 "
                                        "GEMM); only DetectNeckMS has the reduced modes")
        return precision

    @staticmethod
    def _smooth(F: int, depth: int) -> nn.Module:
        return tm.dw_block(F, depth)

    @staticmethod
    def _meta_dims(meta: dict):
        F, names, mcfg, tcfg = tm.meta_fpn(meta)
        arch = _meta_arch(meta, mcfg)
        if arch != "yololitems_cpu":
            raise _lib.YoloLiteHipError(f"DetectNeck: the dense-3x3 + SiLU smooth blocks of arch {arch!r} are not implemented "
                                        "(only YOLOLiteMS_CPU's depthwise neck is)")
        if tcfg.get("use_p6"):
            raise _lib.YoloLiteHipError("DetectNeck: the P6 path (use_p6) is not implemented")
        return F, max(1, round(2 * float(mcfg.get("depth_multiple", 1.0)))), names

    def _param_list(self) -> List[torch.Tensor]:
        """per level: lateral weight, bias, then per block dw, pw, gamma, beta"""
        out = []
        for n in self.level_names:
            lat, s = getattr(self, "lateral" + n[1:]), getattr(self, "smooth" + n[1:]).block
            out += [lat.weight, lat.bias]
            for i in range(self.depth):
                out += [s[4 * i].weight, s[4 * i + 1].weight, s[4 * i + 2].weight, s[4 * i + 2].bias]
        return out

    def _bn(self, name: str, i: int) -> nn.Module:
        return getattr(self, "smooth" + name[1:]).block[4 * i + 2]


class DetectNeckMS(_NeckBase):
    """The dense 3x3 + SiLU neck of arch YOLOLiteMS; see the module docstring.  `in_channels`: the channels of the
    feature maps, finest level first."""
    _who, _handle_cls = "DetectNeckMS", _HandleMS

    @staticmethod
    def _smooth(F: int, depth: int) -> nn.Module:
        return conv_block(F, depth)

    @staticmethod
    def _meta_dims(meta: dict):
        F, names, mcfg, tcfg = tm.meta_fpn(meta)
        arch = _meta_arch(meta, mcfg)
        if arch == "yololitems_cpu":
            raise _lib.YoloLiteHipError("DetectNeckMS: the depthwise smooth blocks of arch 'yololitems_cpu' are DetectNeck's "
                                        "(this class is the dense-3x3 + SiLU neck of YOLOLiteMS)")
        if arch != "yololitems":
            raise _lib.YoloLiteHipError(f"DetectNeckMS: arch {arch!r} is not implemented (only YOLOLiteMS's dense neck is)")
        if tcfg.get("use_p6"):
            raise _lib.YoloLiteHipError("DetectNeckMS: the P6 path (use_p6) is not implemented")
        return F, max(1, round(2 * float(mcfg.get("depth_multiple", 1.0)))), names

    def _param_list(self) -> List[torch.Tensor]:
        """per level: lateral weight, bias, then per block w, gamma, beta"""
        out = []
        for n in self.level_names:
            lat, s = getattr(self, "lateral" + n[1:]), getattr(self, "smooth" + n[1:])
            out += [lat.weight, lat.bias]
            for i in range(self.depth):
                out += [s[3 * i].weight, s[3 * i + 1].weight, s[3 * i + 1].bias]
        return out

    def _bn(self, name: str, i: int) -> nn.Module:
        return getattr(self, "smooth" + name[1:])[3 * i + 1]


def plan_ms(in_channels: Sequence[int], fpn_channels: int, depth: int, batch: int, sizes: Sequence[int]) -> Dict:
    """yl_dneck_plan (a host function; no device): how every level of DetectNeckMS is cut and what the handle holds.
    -> {"stat_rows", "gemm_rows", "conv_tile", "levels": [{rows, stat_tiles, gemm_tiles, conv_tiles, lgrad_rows,
    lgrad_splits, w3grad_tiles, w3grad_splits, saved_bytes}], "saved_bytes", "nosave_bytes", "workspace_bytes",
    "table_bytes"} with, for F channels, depth d, M_k = batch * S_k^2 rows, Mmax the largest M_k and T = conv_tile:
        levels[k].conv_tiles    = batch * ceil(S_k / T)^2                  spatial tiles, image-major then row-major
        levels[k].w3grad_tiles  = ceil(conv_tiles / min(conv_tiles, 64, max(1, 512 // ceil(F / 64)^2)))
        levels[k].w3grad_splits = ceil(conv_tiles / w3grad_tiles)          split z: tiles [z w3grad_tiles, ...)
        levels[k].saved_bytes   = (1 + 2 d) M_k F 4 + d 2 F 4              t_k; z, h and (mean, invstd) per block
        saved_bytes             = sum of the levels'
        nosave_bytes            = 3 Mmax F 4 + 2 F 4                        t and one block of the largest level
        workspace_bytes         = 3 Mmax F 4 + round16(max_k(stat_tiles_k) 2 F 8) + 2 F 4 + 9 F F 4
                                  + max_k round16(max(w3grad_splits_k 9 F F, lgrad_splits_k F Cin_k) 4)
        table_bytes             = sum over k < L - 1 of (S_k + 2 S_{k+1}) 4"""
    in_channels = _check_dims(in_channels, fpn_channels, depth)
    if len(sizes) != len(in_channels):
        raise ValueError(f"{len(in_channels)} levels but sizes {tuple(sizes)}")
    cfg = _cfg(in_channels, fpn_channels, depth)
    out = _lib.yl_dneck_plan_info()
    sz = (C.c_int32 * len(sizes))(*[int(s) for s in sizes])
    _lib.check(_lib.load().yl_dneck_plan(C.byref(cfg), int(batch), sz, C.byref(out)), what="yl_dneck_plan")
    lv = [{n: int(getattr(out.level[k], n)) for n, _ in out.level[k]._fields_} for k in range(len(sizes))]
    return {"stat_rows": int(out.stat_rows), "gemm_rows": int(out.gemm_rows), "conv_tile": int(out.conv_tile), "levels": lv,
            "saved_bytes": int(out.saved_bytes), "nosave_bytes": int(out.nosave_bytes),
            "workspace_bytes": int(out.workspace_bytes), "table_bytes": int(out.table_bytes)}


def neck_for(meta: dict, sd: Optional[dict] = None, precision: str = "fp32"):
    """the trainable neck of the model `meta` describes: DetectNeck for arch YOLOLiteMS_CPU, DetectNeckMS for YOLOLiteMS
    (and a meta without `arch`); filled from the checkpoint `sd` if that is given, freshly initialised otherwise.
    `precision`: DetectNeckMS's operand type; DetectNeck refuses anything but "fp32"."""
    mcfg = (meta.get("config", {}) or {}).get("model", {}) or {}
    cls = DetectNeck if _meta_arch(meta, mcfg) == "yololitems_cpu" else DetectNeckMS
    return cls.from_state_dict(meta, sd, precision) if sd is not None else cls.from_meta(meta, precision)


PASSES = {"forward": _lib.YL_DNECK_PASS_FORWARD, "dgrad": _lib.YL_DNECK_PASS_DGRAD, "wgrad": _lib.YL_DNECK_PASS_WGRAD}


def conv3x3(x_nhwc: torch.Tensor, w_or_dz: torch.Tensor, pass_: str, precision: str = "fp32",
            neck: Optional[DetectNeckMS] = None) -> torch.Tensor:
    """One 3x3 GEMM of DetectNeckMS on its own (yl_dneck_conv3x3: pack + convolution, or partials + ordered sum, launched as
    the module launches them), fp32 tensors on one HIP device:
        "forward":  x  [B,S,S,F], W  [F,F,3,3] -> z  [B,S,S,F]      (pad 1, stride 1, no bias)
        "dgrad":    dz [B,S,S,F], W  [F,F,3,3] -> dx [B,S,S,F]      the gradient of forward's x
        "wgrad":    x  [B,S,S,F], dz [B,S,S,F] -> dW [F,F,3,3]      the gradient of forward's W
    `precision`: both operands are rounded to it (nearest even), fp32 accumulation.  `neck`: a DetectNeckMS of F channels
    whose handle (and workspace) is used (if the workspace has to grow for it, a forward that neck holds for backward is
    dropped and that backward raises); without one a handle is made for the call."""
    if pass_ not in PASSES:
        raise ValueError(f"pass_ must be one of {sorted(PASSES)}, got {pass_!r}")
    _check_precision(precision)
    if not (torch.is_tensor(x_nhwc) and x_nhwc.dim() == 4 and x_nhwc.shape[1] == x_nhwc.shape[2]):
        raise ValueError("the first operand must be [B,S,S,F]")
    B, S, _, F = (int(v) for v in x_nhwc.shape)
    want = (B, S, S, F) if pass_ == "wgrad" else (F, F, 3, 3)
    if not torch.is_tensor(w_or_dz) or tuple(w_or_dz.shape) != want:
        raise ValueError(f"the second operand of {pass_!r} must be {want}")
    if not x_nhwc.is_cuda or w_or_dz.device != x_nhwc.device:
        raise _lib.YoloLiteHipError("conv3x3 needs both operands on one HIP device (no CPU fallback)")
    if neck is not None and (not isinstance(neck, DetectNeckMS) or neck.fpn_channels != F):
        raise ValueError(f"`neck` must be a DetectNeckMS of {F} channels")
    hd = neck._handle if neck is not None else _HandleMS(_check_dims((F,), F, 1), F, 1)
    hd.ensure(x_nhwc.device)
    a = tm.aligned(x_nhwc.detach().float().contiguous())
    b = tm.aligned(w_or_dz.detach().float().contiguous())
    out = torch.empty((F, F, 3, 3) if pass_ == "wgrad" else (B, S, S, F), device=a.device, dtype=torch.float32)
    n = C.c_int32()
    hd.call("conv3x3", PASSES[pass_], PRECISIONS[precision], a.data_ptr(), b.data_ptr(), out.data_ptr(), B, S,
            torch.cuda.current_stream(a.device).cuda_stream, C.byref(n))
    return out
