"""Trainable depthwise FPN neck on the device: the laterals, the top-down upsample-add chain and the smooth blocks of
the reference's YOLOLiteMS_CPU, with a backward pass.

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
CPU fallback.  Not implemented, and refused: the P6 path (`use_p6`) and the dense-3x3 + SiLU smooth blocks of arch
YOLOLiteMS.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib


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


def _dw_block(F: int, n: int) -> nn.Module:
    """Container only (the reference's DWConvBlock(F, F, n)): the layers hold the parameters; their forward is never called."""
    m = nn.Module()
    layers = []
    for _ in range(n):
        layers += [nn.Conv2d(F, F, 3, padding=1, groups=F, bias=False), nn.Conv2d(F, F, 1, bias=False),
                   nn.BatchNorm2d(F), nn.ReLU(inplace=True)]
    m.block = nn.Sequential(*layers)
    return m


class _Handle:
    """The neck's handle and the order its tensors go to the library in"""

    def __init__(self, in_channels, F: int, depth: int):
        self.in_channels, self.F, self.depth = tuple(in_channels), F, depth
        self.L = len(self.in_channels)
        self.handle, self.lib, self.device = None, None, None
        self.generation = 0
        self.last_launches = {"forward": 0, "backward": 0}

    def held(self) -> Dict[str, int]:
        if self.handle is None:
            return {"saved_bytes": 0, "workspace_bytes": 0, "forward_held": 0}
        sb, wb, fv = C.c_int64(), C.c_int64(), C.c_int32()
        _lib.check(self.lib.yl_neck_held(self.handle, C.byref(sb), C.byref(wb), C.byref(fv)), what="yl_neck_held")
        return {"saved_bytes": int(sb.value), "workspace_bytes": int(wb.value), "forward_held": int(fv.value)}

    def __deepcopy__(self, memo):                          # a copied module (an EMA) gets a handle of its own
        return _Handle(self.in_channels, self.F, self.depth)

    def __reduce__(self):
        return _Handle, (self.in_channels, self.F, self.depth)

    @property
    def per_level(self) -> int:
        return 2 + 4 * self.depth

    def table(self, tensors: Sequence[Optional[torch.Tensor]], buffers=None):
        """yl_neck_tensors from a list in DetectNeck._param_list() order (None = NULL)"""
        t = _lib.yl_neck_tensors()
        ptr = lambda v: v.data_ptr() if v is not None else None       # noqa: E731
        n = self.per_level
        for k in range(self.L):
            lv, ts = t.level[k], tensors[k * n:(k + 1) * n]
            lv.lat_w, lv.lat_b = ptr(ts[0]), ptr(ts[1])
            for i in range(self.depth):
                b = lv.block[i]
                b.dw, b.pw, b.gamma, b.beta = (ptr(v) for v in ts[2 + 4 * i:6 + 4 * i])
                if buffers is not None:
                    b.running_mean, b.running_var, b.num_batches_tracked = (ptr(v) for v in buffers[k][i])
        return t

    def ensure(self, device: torch.device):
        if self.handle is not None and self.device == device:
            return
        self.close()
        self.lib = _lib.load()
        h = C.c_void_p()
        cfg = _cfg(self.in_channels, self.F, self.depth)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        _lib.check(self.lib.yl_neck_create(idx, C.byref(cfg), C.byref(h)), what="yl_neck_create")
        self.handle, self.device = h, device

    def close(self):
        if self.handle:
            self.lib.yl_neck_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _aligned(t: torch.Tensor) -> torch.Tensor:
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])


class _NeckFunction(torch.autograd.Function):
    """(p_0, ..., p_{L-1}) = neck(c_0, ..., c_{L-1} NHWC, parameters): yl_neck_forward / yl_neck_backward"""

    @staticmethod
    def forward(fctx, hd: _Handle, bufs, train: bool, grad_mode: bool, *args):
        L = hd.L
        cs, params = args[:L], args[L:]
        B = int(cs[0].shape[0])
        sizes = [int(c.shape[1]) for c in cs]
        # as in DetectHeads: inside a Function's forward the grad mode is always off, so the caller says whether a graph
        # is being recorded.  Without one nothing is saved.
        save = grad_mode and any(fctx.needs_input_grad)
        cd = [_aligned(c.detach()) for c in cs]
        ps = [p.detach() for p in params]
        dev = cs[0].device
        for p in ps:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise _lib.YoloLiteHipError("DetectNeck: parameters must be contiguous fp32 tensors on the input's device")
        outs = [torch.empty((B, S, S, hd.F), device=dev, dtype=torch.float32) for S in sizes]
        n = C.c_int32()
        flags = (_lib.YL_HEAD_TRAIN if train else 0) | (_lib.YL_HEAD_SAVE if save else 0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        sz = (C.c_int32 * L)(*sizes)
        _lib.check(hd.lib.yl_neck_forward(hd.handle, C.byref(hd.table(ps, bufs)), _ptrs(cd), B, sz, flags, _ptrs(outs),
                                          stream, C.byref(n)), what="yl_neck_forward")
        hd.generation += 1
        hd.last_launches["forward"] = int(n.value)
        if save:
            fctx.save_for_backward(*cd, *params)
            fctx.hd, fctx.bufs, fctx.generation, fctx.shape = hd, bufs, hd.generation, (B, sizes)
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, *gps):
        hd = fctx.hd
        if fctx.generation != hd.generation:
            raise _lib.YoloLiteHipError("DetectNeck: the neck ran another forward since the one backward() belongs to "
                                        "(one forward is held at a time)")
        L = hd.L
        saved = fctx.saved_tensors
        cd, params = saved[:L], saved[L:]
        B, sizes = fctx.shape
        need = fctx.needs_input_grad[4:]
        gps = [_aligned(g.to(dtype=torch.float32).contiguous()) for g in gps]
        dcs = [torch.empty_like(c) if need[k] else None for k, c in enumerate(cd)]
        grads = [torch.empty_like(p, memory_format=torch.contiguous_format) if need[L + i] else None
                 for i, p in enumerate(params)]
        n = C.c_int32()
        stream = torch.cuda.current_stream(cd[0].device).cuda_stream
        ps = [p.detach() for p in params]
        sz = (C.c_int32 * L)(*sizes)
        _lib.check(hd.lib.yl_neck_backward(hd.handle, C.byref(hd.table(ps, fctx.bufs)), C.byref(hd.table(grads)),
                                           _ptrs(cd), _ptrs(gps), _ptrs(dcs), B, sz, stream, C.byref(n)),
                   what="yl_neck_backward")
        hd.last_launches["backward"] = int(n.value)
        return (None, None, None, None) + tuple(dcs) + tuple(grads)


class DetectNeck(nn.Module):
    """See the module docstring.  `in_channels`: the channels of the feature maps, finest level first."""

    def __init__(self, in_channels: Sequence[int], fpn_channels: int, depth: int = 1,
                 level_names: Sequence[str] = ("p3", "p4", "p5")):
        super().__init__()
        in_channels = _check_dims(in_channels, fpn_channels, depth)
        self.level_names = tuple(level_names)
        if len(self.level_names) != len(in_channels):
            raise ValueError(f"{len(self.level_names)} levels but in_channels {in_channels}")
        F = int(fpn_channels)
        self.in_channels, self.fpn_channels, self.depth = in_channels, F, int(depth)
        rest = [(n, ci) for n, ci in zip(self.level_names, in_channels) if n != "p2"]
        if "p2" in self.level_names:                       # the reference's order of registration (model_v2.py:286-294)
            self.lateral2 = nn.Conv2d(in_channels[self.level_names.index("p2")], F, 1)
            self.smooth2 = _dw_block(F, self.depth)
        for n, ci in rest:
            setattr(self, "lateral" + n[1:], nn.Conv2d(ci, F, 1))
        for n, ci in rest:
            setattr(self, "smooth" + n[1:], _dw_block(F, self.depth))
        self._handle = _Handle(in_channels, F, self.depth)

    @staticmethod
    def _meta_dims(meta: dict):
        cfg = meta.get("config", {}) or {}
        mcfg, tcfg = cfg.get("model", {}) or {}, cfg.get("training", {}) or {}
        arch = (meta.get("arch") or mcfg.get("arch") or "YOLOLiteMS").lower()
        if arch != "yololitems_cpu":
            raise _lib.YoloLiteHipError(f"DetectNeck: the dense-3x3 + SiLU smooth blocks of arch {arch!r} are not implemented "
                                        "(only YOLOLiteMS_CPU's depthwise neck is)")
        if tcfg.get("use_p6"):
            raise _lib.YoloLiteHipError("DetectNeck: the P6 path (use_p6) is not implemented")
        F = int(int(mcfg.get("fpn_channels", 128)) * float(mcfg.get("width_multiple", 1.0)))
        d = max(1, round(2 * float(mcfg.get("depth_multiple", 1.0))))
        names = (["p2"] if tcfg.get("use_p2") else []) + ["p3", "p4", "p5"]
        return F, d, names

    @classmethod
    def from_meta(cls, meta: dict) -> "DetectNeck":
        """a freshly initialised neck of the model `meta` describes; the input channels are those of the feature maps of
        the program build_program makes for it"""
        from .program import build_program, synth_state_dict
        F, d, names = cls._meta_dims(meta)
        prog = build_program(meta, synth_state_dict(meta))
        cin = [int(prog.slots[prog.feature_slots["c" + n[1:]]][2]) for n in names]
        return cls(cin, F, d, level_names=names)

    @classmethod
    def from_state_dict(cls, meta: dict, sd: dict) -> "DetectNeck":
        """the neck of a checkpoint: built from its meta, filled with its `lateral*.` / `smooth*.` entries"""
        F, d, names = cls._meta_dims(meta)
        missing = [f"lateral{n[1:]}.weight" for n in names if f"lateral{n[1:]}.weight" not in sd]
        if missing:
            raise KeyError(f"checkpoint lacks neck entries: {missing[:4]}")
        cin = [int(np.shape(sd[f"lateral{n[1:]}.weight"])[1]) for n in names]
        m = cls(cin, F, d, level_names=names)
        own = m.state_dict()
        missing = [k for k in own if k not in sd and not k.endswith("num_batches_tracked")]
        if missing:
            raise KeyError(f"checkpoint lacks neck entries: {missing[:4]}")
        m.load_state_dict({k: torch.as_tensor(np.asarray(sd[k]) if not torch.is_tensor(sd[k]) else sd[k])
                           .reshape(v.shape).to(v.dtype) for k, v in own.items() if k in sd}, strict=False)
        return m

    def _param_list(self) -> List[torch.Tensor]:
        """per level: lateral weight, bias, then per block dw, pw, gamma, beta"""
        out = []
        for n in self.level_names:
            lat, s = getattr(self, "lateral" + n[1:]), getattr(self, "smooth" + n[1:]).block
            out += [lat.weight, lat.bias]
            for i in range(self.depth):
                out += [s[4 * i].weight, s[4 * i + 1].weight, s[4 * i + 2].weight, s[4 * i + 2].bias]
        return out

    def _stat_buffers(self):
        out = []
        for n in self.level_names:
            s = getattr(self, "smooth" + n[1:]).block
            out.append([(s[4 * i + 2].running_mean, s[4 * i + 2].running_var, s[4 * i + 2].num_batches_tracked)
                        for i in range(self.depth)])
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
        feats = list(feats)
        if layout not in (None, "nchw", "nhwc"):
            raise ValueError(f"layout must be 'nchw', 'nhwc' or None, got {layout!r}")
        if len(feats) != len(self.level_names):
            raise ValueError(f"expected {len(self.level_names)} feature maps, got {len(feats)}")
        xs = []
        for f, ci in zip(feats, self.in_channels):         # host-side facts first, the device last
            if not torch.is_tensor(f) or f.dim() != 4:
                raise ValueError("feature maps must be 4-d tensors [B,Cin,S,S] or [B,S,S,Cin]")
            nchw = f.shape[1] == ci and f.shape[2] == f.shape[3]
            nhwc = f.shape[3] == ci and f.shape[1] == f.shape[2]
            if layout is None and nchw and nhwc:
                raise ValueError(f"feature map {tuple(f.shape)} reads as [B,{ci},S,S] and as [B,S,S,{ci}]: "
                                 "pass layout='nchw' or layout='nhwc'")
            if not (nchw if layout == "nchw" else nhwc if layout == "nhwc" else nchw or nhwc):
                want = {None: f"neither [B,{ci},S,S] nor [B,S,S,{ci}]", "nchw": f"not [B,{ci},S,S]",
                        "nhwc": f"not [B,S,S,{ci}]"}
                raise ValueError(f"feature map {tuple(f.shape)} is {want[layout]}")
            if layout == "nchw" or (layout is None and nchw):
                f = f.permute(0, 2, 3, 1)
            if not f.is_cuda:
                raise _lib.YoloLiteHipError("DetectNeck needs its inputs on a HIP device (no CPU fallback)")
            if self.training and f.shape[0] * f.shape[1] * f.shape[2] == 1:
                raise ValueError("Expected more than 1 value per channel when training, got input size "
                                 f"{[int(f.shape[0]), self.fpn_channels, 1, 1]}")
            xs.append(f)
        if len({int(f.shape[0]) for f in xs}) != 1 or len({f.device for f in xs}) != 1:
            raise ValueError("the feature maps must share one batch size and one device")
        params = self._param_list()
        if any(p.device != xs[0].device for p in params):
            raise _lib.YoloLiteHipError("DetectNeck: parameters and inputs must live on one HIP device")
        self._handle.ensure(xs[0].device)
        xs = [f.float().contiguous() for f in xs]          # autograd carries the gradient back through cast and copy
        return list(_NeckFunction.apply(self._handle, self._stat_buffers(), self.training, torch.is_grad_enabled(), *xs, *params))
