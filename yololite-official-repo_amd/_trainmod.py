"""What the trainable modules on the device share (headops.DetectHeads, neckops.DetectNeck / DetectNeckMS,
stageops.UIBStack, stemops.ConvStack): the handle of one library
object, the depthwise block's container and its entry in the library's tables, the reading of feature maps, checkpoints
and meta, the parts of an autograd.Function that do not depend on the module, and the Function and module base of the
conv + BatchNorm unit stacks (backbone stage and dense stem).

One handle holds ONE forward for backward at a time (csrc/yl_block.h, Arena): every forward bumps the handle's
generation, and a backward whose generation is no longer the handle's raises.  The handle's memory only grows.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch
from torch import nn

from . import _lib


class DeviceHandle:
    """A `<prefix>_create`d library object (prefix "yl_head", "yl_neck", "yl_dneck") of the config `cfg(*args)`, made on first use
    and again when the device changes.  A subclass adds table(): the order its tensors go to the library in."""

    def __init__(self, prefix: str, cfg, *args):
        self.prefix, self.cfg, self.args = prefix, cfg, args
        self.handle, self.lib, self.device = None, None, None
        self.generation = 0
        self.last_launches = {"forward": 0, "backward": 0}

    def __deepcopy__(self, memo):                          # a copied module (an EMA) gets a handle of its own
        return type(self)(*self.args)

    def __reduce__(self):
        return type(self), self.args

    def call(self, name: str, *args):
        what = f"{self.prefix}_{name}"
        _lib.check(getattr(self.lib, what)(self.handle, *args), what=what)

    def held(self) -> Dict[str, int]:
        """<prefix>_held: bytes the handle holds now and whether a forward is held for backward"""
        if self.handle is None:
            return {"saved_bytes": 0, "workspace_bytes": 0, "forward_held": 0}
        sb, wb, fv = C.c_int64(), C.c_int64(), C.c_int32()
        self.call("held", C.byref(sb), C.byref(wb), C.byref(fv))
        return {"saved_bytes": int(sb.value), "workspace_bytes": int(wb.value), "forward_held": int(fv.value)}

    def ensure(self, device: torch.device):
        if self.handle is not None and self.device == device:
            return
        self.close()
        self.lib = _lib.load()
        h = C.c_void_p()
        idx = device.index if device.index is not None else torch.cuda.current_device()
        what = self.prefix + "_create"
        _lib.check(getattr(self.lib, what)(idx, C.byref(self.cfg(*self.args)), C.byref(h)), what=what)
        self.handle, self.device = h, device

    def close(self):
        if self.handle:
            getattr(self.lib, self.prefix + "_destroy")(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def launch(self, name: str, device: torch.device, *args):
        """<prefix>_forward / _backward(handle, *args, stream, &launches) on torch's current stream of `device`.  A
        forward that went through is a new generation: what an earlier one held for backward is gone."""
        n = C.c_int32()
        self.call(name, *args, torch.cuda.current_stream(device).cuda_stream, C.byref(n))
        if name == "forward":
            self.generation += 1
        self.last_launches[name] = int(n.value)

    def check_generation(self, generation: int, subject: str, rule: str):
        if generation != self.generation:
            raise _lib.YoloLiteHipError(f"{subject} ran another forward since the one backward() belongs to "
                                        f"({rule} is held at a time)")


# the operand type of a module's GEMMs -> the precision bits of its forward's flags (YL_HEAD_F16 / _BF16 and
# YL_DNECK_F16 / _BF16 are the same bits)
PRECISIONS = {"fp32": 0, "fp16": _lib.YL_HEAD_F16, "bf16": _lib.YL_HEAD_BF16}


def check_precision(precision) -> str:
    if not isinstance(precision, str) or precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
    return precision


PRECISION_OF = {v: k for k, v in PRECISIONS.items()}


def dw_block(F: int, n: int) -> nn.Module:
    """Container only (the reference's DWConvBlock(F, F, n)): the layers hold the parameters; their forward is never called."""
    m = nn.Module()
    layers = []
    for _ in range(n):
        layers += [nn.Conv2d(F, F, 3, padding=1, groups=F, bias=False), nn.Conv2d(F, F, 1, bias=False),
                   nn.BatchNorm2d(F), nn.ReLU(inplace=True)]
    m.block = nn.Sequential(*layers)
    return m


def ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def fill_block(b, params4: Sequence[Optional[torch.Tensor]], buffers3=None):
    """one yl_head_block: dw, pw, gamma, beta (None = NULL) and, for a parameter table, the BatchNorm's three buffers"""
    b.dw, b.pw, b.gamma, b.beta = (ptr(v) for v in params4)
    if buffers3 is not None:
        b.running_mean, b.running_var, b.num_batches_tracked = (ptr(v) for v in buffers3)


def aligned(t: torch.Tensor) -> torch.Tensor:
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def as_nhwc(f, channels: int, layout: Optional[str], who: str, training: bool, *, name: str = "F",
            bn_channels: Optional[int] = None) -> torch.Tensor:
    """One feature map as an NHWC view.  `layout`: "nchw" ([B,C,S,S], any strides), "nhwc" ([B,S,S,C]) or None, which
    reads it off the shape and refuses the one shape that is both.  Host-side facts first, the device last; then what
    BatchNorm refuses in training (`bn_channels`: of the map the first BatchNorm sees)."""
    c = channels
    if not torch.is_tensor(f) or f.dim() != 4:
        raise ValueError(f"feature maps must be 4-d tensors [B,{name},S,S] or [B,S,S,{name}]")
    nchw = f.shape[1] == c and f.shape[2] == f.shape[3]
    nhwc = f.shape[3] == c and f.shape[1] == f.shape[2]
    if layout is None and nchw and nhwc:
        raise ValueError(f"feature map {tuple(f.shape)} reads as [B,{c},S,S] and as [B,S,S,{c}]: "
                         "pass layout='nchw' or layout='nhwc'")
    if not (nchw if layout == "nchw" else nhwc if layout == "nhwc" else nchw or nhwc):
        want = {None: f"neither [B,{c},S,S] nor [B,S,S,{c}]", "nchw": f"not [B,{c},S,S]", "nhwc": f"not [B,S,S,{c}]"}
        raise ValueError(f"feature map {tuple(f.shape)} is {want[layout]}")
    if layout == "nchw" or (layout is None and nchw):
        f = f.permute(0, 2, 3, 1)                          # NCHW -> an NHWC view (channels-last memory: already contiguous)
    if not f.is_cuda:
        raise _lib.YoloLiteHipError(f"{who} needs its inputs on a HIP device (no CPU fallback)")
    if training and f.shape[0] * f.shape[1] * f.shape[2] == 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size "
                         f"{[int(f.shape[0]), c if bn_channels is None else bn_channels, 1, 1]}")
    return f


def check_layout(layout: Optional[str], feats, levels: int) -> list:
    """the arguments of a module's forward: -> the feature maps as a list"""
    feats = list(feats)
    if layout not in (None, "nchw", "nhwc"):
        raise ValueError(f"layout must be 'nchw', 'nhwc' or None, got {layout!r}")
    if len(feats) != levels:
        raise ValueError(f"expected {levels} feature maps, got {len(feats)}")
    return feats


def fill_from_state_dict(module: nn.Module, sd: dict, what: str) -> nn.Module:
    """fills `module` with the checkpoint's entries of its own keys (tensors or numpy arrays, any shape of the right
    size); only num_batches_tracked may be absent"""
    own = module.state_dict()
    missing = [k for k in own if k not in sd and not k.endswith("num_batches_tracked")]
    if missing:
        raise KeyError(f"checkpoint lacks {what} entries: {missing[:4]}")
    module.load_state_dict({k: torch.as_tensor(sd[k]).reshape(v.shape).to(v.dtype) for k, v in own.items() if k in sd},
                           strict=False)
    return module


def meta_fpn(meta: dict):
    """-> (fpn channels, level names finest first, model config, training config) of the model `meta` describes
    (program.build_program reads the same keys)"""
    cfg = meta.get("config", {}) or {}
    mcfg, tcfg = cfg.get("model", {}) or {}, cfg.get("training", {}) or {}
    F = int(int(mcfg.get("fpn_channels", 128)) * float(mcfg.get("width_multiple", 1.0)))
    names = (["p2"] if tcfg.get("use_p2") else []) + ["p3", "p4", "p5"] + (["p6"] if tcfg.get("use_p6") else [])
    return F, names, mcfg, tcfg


# ---- the parts of an autograd.Function's forward and backward that are the same for every module

def saving(fctx, grad_mode: bool) -> bool:
    """needs_input_grad reports requires_grad whatever the grad mode, and inside a Function's forward the mode is always
    off: the caller says whether a graph is being recorded.  Without one nothing is saved."""
    return grad_mode and any(fctx.needs_input_grad)


def detached_params(who: str, params: Sequence[torch.Tensor], device: torch.device) -> List[torch.Tensor]:
    ps = [p.detach() for p in params]
    for p in ps:
        if p.dtype != torch.float32 or not p.is_contiguous() or p.device != device:
            raise _lib.YoloLiteHipError(f"{who}: parameters must be contiguous fp32 tensors on the input's device")
    return ps


def flags(train: bool, save: bool) -> int:
    return (_lib.YL_HEAD_TRAIN if train else 0) | (_lib.YL_HEAD_SAVE if save else 0)


def grads_like(tensors: Sequence[torch.Tensor], need: Sequence[bool]) -> List[Optional[torch.Tensor]]:
    """an uninitialised contiguous gradient for every tensor whose entry of `need` (a slice of needs_input_grad) is set"""
    return [torch.empty_like(t, memory_format=torch.contiguous_format) if n else None for t, n in zip(tensors, need)]


# ---- a stack of conv + BatchNorm units (csrc/yl_units.h): stageops.UIBStack and stemops.ConvStack

class UnitStackHandle(DeviceHandle):
    """The handle of a unit stack (prefix "yl_stage", "yl_stem"): its dense GEMMs' operand type goes through
    yl_amp_<stage|stem>_set / _get, not through the forward's flags"""

    def _amp(self, name: str, *args):
        what = f"yl_amp_{self.prefix[3:]}_{name}"
        _lib.check(getattr(self.lib, what)(self.handle, *args), what=what)

    def amp_set(self, precision: str):
        """the mode of the NEXT forward; a held forward keeps its own"""
        self._amp("set", PRECISIONS[precision])

    def amp_get(self) -> Dict[str, Optional[str]]:
        """{"precision": the handle's mode, "held": the held forward's, None without one}"""
        if self.handle is None:
            return {"precision": "fp32", "held": None}
        m, hm = C.c_uint32(), C.c_uint32()
        self._amp("get", C.byref(m), C.byref(hm))
        return {"precision": PRECISION_OF[int(m.value)], "held": PRECISION_OF[int(hm.value)] if self.held()["forward_held"] else None}


class UnitStackFunction(torch.autograd.Function):
    """y = stack(x, parameters): <prefix>_forward / <prefix>_backward of the handle `hd`.  x: NHWC [B,S,S,C], or with
    `nchw` the planar image [B,C,S,S], which has no gradient"""
    ARGS = 6                                               # what stands in front of x

    @staticmethod
    def forward(fctx, hd: DeviceHandle, bufs, train: bool, grad_mode: bool, out_shape, nchw: bool, x, *params):
        save = saving(fctx, grad_mode)
        xd = x.detach() if nchw else aligned(x.detach())
        dev = x.device
        ps = detached_params(hd.who, params, dev)
        B, S = int(x.shape[0]), int(x.shape[2])            # S stands third in either layout
        out = torch.empty(out_shape, device=dev, dtype=torch.float32)
        hd.launch("forward", dev, C.byref(hd.table(ps, bufs)), xd.data_ptr(), B, S, flags(train, save), out.data_ptr())
        if save:
            fctx.save_for_backward(xd, *params)
            fctx.hd, fctx.bufs, fctx.generation, fctx.nchw = hd, bufs, hd.generation, nchw
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, gy):
        hd = fctx.hd
        hd.check_generation(fctx.generation, hd.who + ": the stack", "one forward")
        saved = fctx.saved_tensors
        gy = aligned(gy.to(dtype=torch.float32).contiguous())
        need = list(fctx.needs_input_grad[UnitStackFunction.ARGS:])
        if fctx.nchw:
            need[0] = False
        grads = grads_like(saved, need)
        ps = [p.detach() for p in saved[1:]]
        hd.launch("backward", saved[0].device, C.byref(hd.table(ps, fctx.bufs)), C.byref(hd.table(grads[1:])), gy.data_ptr(),
                  ptr(grads[0]))
        return (None,) * UnitStackFunction.ARGS + tuple(grads)


class UnitStack(nn.Module):
    """What the unit stacks share.  A subclass fills _convs, _bns (one layer each per unit, in running order) and _handle,
    and gives _unit_sizes(S): the size of the map every unit writes.  `.precision` ("fp32", "fp16", "bf16") is the operand
    type of the stack's dense GEMMs from the next forward on; a backward runs in the precision of its forward."""
    _precision = "fp32"

    @property
    def precision(self) -> str:
        return self._precision

    @precision.setter
    def precision(self, value):
        self._precision = check_precision(value)           # host side only: the handle learns it in front of a forward

    def amp_state(self) -> Dict[str, Optional[str]]:
        """yl_amp_*_get: {"precision": the mode the handle was last given, "held": that of the forward held for backward}"""
        return self._handle.amp_get()

    def _param_list(self) -> List[torch.Tensor]:
        """per unit in running order: conv weight, BatchNorm weight, BatchNorm bias"""
        out = []
        for cv, bn in zip(self._convs, self._bns):
            out += [cv.weight, bn.weight, bn.bias]
        return out

    def _stat_buffers(self):
        return [(bn.running_mean, bn.running_var, bn.num_batches_tracked) for bn in self._bns]

    @property
    def last_launches(self) -> Dict[str, int]:
        """kernels enqueued by the last forward / backward"""
        return dict(self._handle.last_launches)

    def held(self) -> Dict[str, int]:
        """the bytes the handle holds on the device and whether a forward is held for backward"""
        return self._handle.held()

    def _check_rows(self, B: int, S: int) -> List[int]:
        """-> the size of every unit's output; in training no BatchNorm may see ONE value per channel"""
        sizes = self._unit_sizes(S)
        if self.training:
            for So, bn in zip(sizes, self._bns):
                if B * So * So == 1:
                    raise ValueError("Expected more than 1 value per channel when training, got input size "
                                     f"{[B, bn.num_features, So, So]}")
        return sizes

    def _run_stack(self, x: torch.Tensor, B: int, sizes: List[int], nchw: bool) -> torch.Tensor:
        """forward()'s tail, once x's shape is checked and it is on a device: -> NHWC [B,S_out,S_out,C_out]"""
        params = self._param_list()
        if any(p.device != x.device for p in params):
            raise _lib.YoloLiteHipError(f"{self._who}: parameters and inputs must live on one HIP device")
        self._handle.ensure(x.device)
        self._handle.amp_set(self._precision)
        x = x.float().contiguous()                         # autograd carries the gradient back through cast and copy
        shape = (B, sizes[-1], sizes[-1], self.out_channels)
        return UnitStackFunction.apply(self._handle, self._stat_buffers(), self.training, torch.is_grad_enabled(), shape, nchw,
                                       x, *params)
