"""A trainable dense stem on the device: a stack of dense `conv -> BatchNorm -> ReLU` units with a backward pass
(csrc/yl_stem.hip), the part of a MobileNetV4 backbone between the image and its C3 tap.

    ConvStack(in_channels, units, eps=1e-5, prefix="", input_layout="nhwc", precision="fp32")    any such stack
    BackboneStem.from_meta(meta) / .from_state_dict(meta, sd)    conv_stem, stage 0 and stage 1: image -> C3
    conv(a, b, pass_, k, stride, size=None, layout="nhwc", precision=None)   one convolution pass on its own (yl_stem_conv,
                                                                 with a precision yl_amp_stem_conv)
    plan(in_channels, units, batch, size, input_layout="nhwc")   yl_stem_plan: what the handle holds

    c3 = stem(x)                                           # x: the image [B,3,S,S]; c3: NHWC [B,S/8,S/8,C3]

`units` is a list of dicts {"k": 3, "s": 2, "c": 32}: a bias-free dense k x k convolution (k 1 or 3, stride 1 or 2,
padding (k - 1) / 2), BatchNorm2d, ReLU.  Optional "conv" / "bn": the dotted names of the two layers under `prefix`
(default "units.{i}.conv" / "units.{i}.bn1"), so that state_dict() carries a checkpoint's own names
(`backbone.conv_stem.weight`, `backbone.bn1.*`, `backbone.blocks.0.0.conv.weight`, `backbone.blocks.0.0.bn1.*`, ...).
input_layout="nchw": the stack's input is the planar image [B,cin,S,S] with cin in 1..4, read as it is; it has no
gradient here, and a tensor that requires one is refused.  With "nhwc" x is [B,S,S,cin] (cin a multiple of 4) and its
gradient is computed when asked for.  The output is NHWC.

The whole stack is ONE torch.autograd.Function (_trainmod.UnitStackFunction, which the backbone stage shares) over
yl_stem_forward / yl_stem_backward.  train() / eval() select the
BatchNorm mode.  Gradients nobody asked for are not computed, and nothing upstream of the first one wanted runs
(`last_launches` says what ran).  One forward is held for backward at a time.  fp32 tensors on one HIP device; no CPU
fallback.  precision="fp16" / "bf16" (constructor, from_meta / from_state_dict, or the settable `.precision`) runs every
dense GEMM, the 3x3 and the 1x1 convolutions of all three passes, on 16-bit MFMA: operands rounded to nearest even inside
the launch that reads them, fp32 accumulation, nothing clamped (an fp16 overflow is inf).  Parameters, saved activations
and gradients stay fp32, BatchNorm and ReLU too, and the launch counts are those of fp32.  A backward runs in the
precision of its forward.
ReLU only: the `_skip` residual, other activations and TF-SAME padding are refused by name, as are the backbone
families whose first stages are built from other blocks.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch
from torch import nn

from . import _lib
from . import _trainmod as tm
from .stageops import _nest, _out_size

PASSES = {"forward": _lib.YL_STAGE_PASS_FORWARD, "dgrad": _lib.YL_STAGE_PASS_DGRAD, "wgrad": _lib.YL_STAGE_PASS_WGRAD}


def _check_units(in_channels, units, eps, input_layout) -> List[dict]:
    """host-side facts only: -> the units as dicts with every field present (cin among them)"""
    if input_layout not in ("nhwc", "nchw"):
        raise ValueError(f"input_layout must be 'nhwc' or 'nchw', got {input_layout!r}")
    cin = int(in_channels)
    if input_layout == "nchw":
        if not 1 <= cin <= 4:
            raise _lib.YoloLiteHipError(f"a planar (nchw) input has 1..4 channels, got {cin}")
    elif cin < 4 or cin % 4:
        raise _lib.YoloLiteHipError(f"in_channels must be a multiple of 4 (or input_layout='nchw' with 1..4), got {cin}")
    units = list(units)
    if not 1 <= len(units) <= _lib.YL_STEM_MAX_UNITS:
        raise _lib.YoloLiteHipError(f"1..{_lib.YL_STEM_MAX_UNITS} units, got {len(units)}")
    if not float(eps) > 0:
        raise _lib.YoloLiteHipError(f"eps must be positive, got {eps}")
    out = []
    for i, u in enumerate(units):
        u = dict(u)
        act = str(u.get("act", "relu")).lower()
        if act != "relu":
            raise _lib.YoloLiteHipError(f"unit {i}: activation {act!r} is not implemented (ReLU only)")
        if u.get("same"):
            raise _lib.YoloLiteHipError(f"unit {i}: TF-SAME padding is not implemented (symmetric padding (k - 1) / 2 only)")
        if u.get("skip"):
            raise _lib.YoloLiteHipError(f"unit {i}: the _skip residual is not implemented")
        k, s, c = int(u.get("k", 0)), int(u.get("s", 1)), int(u.get("c", 0))
        if k not in (1, 3):
            raise _lib.YoloLiteHipError(f"unit {i}: k must be 1 or 3, got {k}")
        if s not in (1, 2):
            raise _lib.YoloLiteHipError(f"unit {i}: s must be 1 or 2, got {s}")
        if c < 4 or c % 4:
            raise _lib.YoloLiteHipError(f"unit {i}: channels must be multiples of 4, got c = {c}")
        out.append(dict(k=k, s=s, c=c, cin=cin, conv=str(u.get("conv", f"units.{i}.conv")), bn=str(u.get("bn", f"units.{i}.bn1"))))
        cin = c
    names = [d["conv"] for d in out] + [d["bn"] for d in out]
    if len(set(names)) != len(names):
        raise ValueError("layer names must differ")
    return out


def _sizes(units: List[dict], S: int) -> List[int]:
    out = []
    for d in units:
        S = _out_size(S, d["k"], d["s"])
        out.append(S)
    return out


def _cfg(in_channels, units, eps, nchw):
    c = _lib.yl_stem_cfg()
    c.in_channels, c.num_units, c.input_nchw, c.eps = int(in_channels), len(units), int(bool(nchw)), float(eps)
    for i, d in enumerate(units):
        c.unit[i].k, c.unit[i].s, c.unit[i].cout = d["k"], d["s"], d["c"]
    return c


def plan(in_channels: int, units: Sequence[dict], batch: int, size: int, eps: float = 1e-5, input_layout: str = "nhwc") -> Dict:
    """yl_stem_plan (a host function; no device).  -> {"stat_rows", "gemm_rows", "conv_tile", "stat_tiles_max", "units":
    [{size_in, size_out, rows_out, stat_rows, stat_tiles, wgrad_rows, wgrad_splits, conv_block, saved_bytes}],
    "saved_bytes", "nosave_bytes", "workspace_bytes"}; the formulas are in include/yololite_hip.h (yl_stem_plan_info)."""
    units = _check_units(in_channels, units, eps, input_layout)
    cfg = _cfg(in_channels, units, eps, input_layout == "nchw")
    out = _lib.yl_stem_plan_info()
    _lib.check(_lib.load().yl_stem_plan(C.byref(cfg), int(batch), int(size), C.byref(out)), what="yl_stem_plan")
    us = [{n: int(getattr(out.unit[i], n)) for n, _ in out.unit[i]._fields_} for i in range(len(units))]
    return {"stat_rows": int(out.stat_rows), "gemm_rows": int(out.gemm_rows), "conv_tile": int(out.conv_tile),
            "stat_tiles_max": int(out.stat_tiles_max), "units": us, "saved_bytes": int(out.saved_bytes),
            "nosave_bytes": int(out.nosave_bytes), "workspace_bytes": int(out.workspace_bytes)}


class _Handle(tm.UnitStackHandle):
    """The stack's handle (see _trainmod.UnitStackHandle) and the order its tensors go to the library in"""
    who = "ConvStack"

    def __init__(self, in_channels: int, units: List[dict], eps: float, nchw: bool):
        super().__init__("yl_stem", _cfg, in_channels, [dict(d) for d in units], eps, nchw)
        self.n = len(units)

    def table(self, tensors: Sequence[Optional[torch.Tensor]], buffers=None):
        """yl_stem_tensors from a list in ConvStack._param_list() order: per unit w, gamma, beta (None = NULL)"""
        t = _lib.yl_stem_tensors()
        for i in range(self.n):
            e = t.unit[i]
            e.w, e.gamma, e.beta = (tm.ptr(v) for v in tensors[3 * i:3 * i + 3])
            if buffers is not None:
                e.running_mean, e.running_var, e.num_batches_tracked = (tm.ptr(v) for v in buffers[i])
        return t


class _StemHandle(_Handle):
    who = "BackboneStem"


class ConvStack(tm.UnitStack):
    """See the module docstring."""
    _who, _handle_cls = "ConvStack", _Handle

    def __init__(self, in_channels: int, units: Sequence[dict], eps: float = 1e-5, prefix: str = "", input_layout: str = "nhwc",
                 precision: str = "fp32"):
        super().__init__()
        self.precision = precision
        self.units_cfg = _check_units(in_channels, units, eps, input_layout)
        self.in_channels, self.eps, self.prefix = int(in_channels), float(eps), str(prefix)
        self.input_layout = input_layout
        self.out_channels = self.units_cfg[-1]["c"]
        self._convs, self._bns = [], []
        for d in self.units_cfg:                           # containers only: the layers hold the parameters
            cv = nn.Conv2d(d["cin"], d["c"], d["k"], d["s"], padding=d["k"] // 2, bias=False)
            bn = nn.BatchNorm2d(d["c"], eps=self.eps)
            _nest(self, self.prefix + d["conv"], cv)
            _nest(self, self.prefix + d["bn"], bn)
            self._convs.append(cv); self._bns.append(bn)
        self._handle = self._handle_cls(self.in_channels, self.units_cfg, self.eps, input_layout == "nchw")

    def out_size(self, size: int) -> int:
        return _sizes(self.units_cfg, int(size))[-1]

    def _unit_sizes(self, S: int) -> List[int]:
        return _sizes(self.units_cfg, S)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """`x`: [B,cin,S,S] with input_layout "nchw", [B,S,S,cin] with "nhwc".  -> NHWC [B,S_out,S_out,C_out]."""
        nchw = self.input_layout == "nchw"
        c = self.in_channels
        if not torch.is_tensor(x) or x.dim() != 4:
            raise ValueError(f"the input must be a 4-d tensor {'[B,%d,S,S]' % c if nchw else '[B,S,S,%d]' % c}")
        ok = (x.shape[1] == c and x.shape[2] == x.shape[3]) if nchw else (x.shape[3] == c and x.shape[1] == x.shape[2])
        if not ok:
            raise ValueError(f"input {tuple(x.shape)} is not {'[B,%d,S,S]' % c if nchw else '[B,S,S,%d]' % c}")
        if nchw and x.requires_grad:
            raise _lib.YoloLiteHipError(f"{self._who}: the planar (nchw) input has no gradient here: pass a tensor that "
                                        "does not require one (x.detach())")
        B, S = int(x.shape[0]), int(x.shape[2])
        sizes = self._check_rows(B, S)
        if not x.is_cuda:
            raise _lib.YoloLiteHipError(f"{self._who} needs its inputs on a HIP device (no CPU fallback)")
        return self._run_stack(x, B, sizes, nchw)


def _stem_units(meta: dict):
    """-> (units with the checkpoint's layer names, eps) of the part of the backbone `meta` names between the image and
    its C3 tap: conv_stem and the stages up to the third-last tap, read from program.BACKBONES with program._backbone's
    channel arithmetic (the stem is fixed below 1.0x).  Host-side facts only; refuses by name."""
    import math
    from .program import BACKBONES, CONVNEXT, HGNET, _make_divisible, _parse
    who = "BackboneStem"
    cfg = meta.get("config", {}) or {}
    mcfg, tcfg = cfg.get("model", {}) or {}, cfg.get("training", {}) or {}
    name = meta.get("backbone") or mcfg.get("backbone") or "resnet18"
    if name in HGNET or name in CONVNEXT or name not in BACKBONES:
        raise _lib.YoloLiteHipError(f"{who}: backbone {name!r} is not implemented (its first stages are not made of dense "
                                    "conv-BN-ReLU blocks; only the mobilenetv4_conv_small family's are)")
    if tcfg.get("use_p2"):
        raise _lib.YoloLiteHipError(f"{who}: use_p2 (a C2 tap inside the stem) is not implemented")
    spec = BACKBONES[name]
    arch, rlim = spec["arch"], spec.get("round_limit", 0.9)
    if spec["act"] != "relu":
        raise _lib.YoloLiteHipError(f"{who}: backbone {name!r} is not implemented: activation {spec['act']!r} (ReLU only)")
    if spec["same"]:
        raise _lib.YoloLiteHipError(f"{who}: backbone {name!r} is not implemented: TF-SAME padding")
    ns = len(arch)
    taps = [si for si in range(ns) if si + 1 == ns or _parse(arch[si + 1][0])["s"] > 1]
    if len(taps) < 3:
        raise _lib.YoloLiteHipError(f"{who}: backbone {name!r} has no C3 tap")
    units = [dict(k=3, s=2, c=int(spec["stem"]), conv="conv_stem", bn="bn1")]
    for si in range(taps[-3] + 1):
        bi = 0
        for bstr in arch[si]:
            d = _parse(bstr)
            rep = d["r"]
            if spec["dmult"] != 1.0 and not (spec["fix_first_last"] and si in (0, ns - 1)):
                rep = int(math.ceil(rep * spec["dmult"]))
            cout = _make_divisible(d["c"] * spec["cmult"], 8, rlim)
            for r in range(rep):
                if d["type"] != "cn" or d.get("se") or d.get("skip") or d["k"] not in (1, 3):
                    raise _lib.YoloLiteHipError(f"{who}: backbone {name!r} is not implemented: block {bstr!r} of its first "
                                                "stages is not a plain dense 1x1 / 3x3 conv-BN-ReLU block")
                units.append(dict(k=d["k"], s=d["s"] if r == 0 else 1, c=cout, conv=f"blocks.{si}.{bi}.conv",
                                  bn=f"blocks.{si}.{bi}.bn1"))
                bi += 1
    if len(units) > _lib.YL_STEM_MAX_UNITS:
        raise _lib.YoloLiteHipError(f"{who}: backbone {name!r} is not implemented: {len(units)} units before its C3 tap")
    return units, float(spec["eps"])


class BackboneStem(ConvStack):
    """Image -> C3 of a mobilenetv4_conv_small[_050] backbone (`backbone.conv_stem`, `backbone.bn1`, `backbone.blocks.0.*`,
    `backbone.blocks.1.*`) under the checkpoint's key names.  stem(x [B,3,S,S]) -> c3 NHWC."""
    _who, _handle_cls = "BackboneStem", _StemHandle

    @classmethod
    def from_meta(cls, meta: dict, precision: str = "fp32"):
        tm.check_precision(precision)
        units, eps = _stem_units(meta)
        return cls(3, units, eps=eps, prefix="backbone.", input_layout="nchw", precision=precision)

    @classmethod
    def from_state_dict(cls, meta: dict, sd: dict, precision: str = "fp32"):
        return tm.fill_from_state_dict(cls.from_meta(meta, precision), sd, "backbone stem")


def conv(a: torch.Tensor, b: torch.Tensor, pass_: str, k: int, stride: int, size: Optional[int] = None,
         layout: str = "nhwc", precision: Optional[str] = None) -> torch.Tensor:
    """One convolution pass of the stack on its own (yl_stem_conv, launched as the module launches it), fp32 tensors on
    one HIP device, pad (k - 1) / 2, So = (S + 2 pad - k) / stride + 1:
        "forward":  x  [B,S,S,cin],     W  [cout,cin,k,k]    -> y  [B,So,So,cout]
        "dgrad":    dy [B,So,So,cout],  W  [cout,cin,k,k]    -> dx [B,S,S,cin]       the gradient of forward's x
        "wgrad":    x  [B,S,S,cin],     dy [B,So,So,cout]    -> dW [cout,cin,k,k]    the gradient of forward's W
    layout="nchw": x is the planar image [B,cin,S,S], cin in 1..4 ("forward" and "wgrad" only).  `size`: S of "dgrad",
    which So does not determine under stride 2 (stride 1: S = So).  The weight may start at any 4-byte boundary.
    `precision`: None is yl_stem_conv (fp32); "fp32", "fp16", "bf16" go through yl_amp_stem_conv: both operands rounded to
    nearest even inside the launches, fp32 accumulation, an fp32 result."""
    if precision is not None:
        tm.check_precision(precision)
    if pass_ not in PASSES:
        raise ValueError(f"pass_ must be one of {sorted(PASSES)}, got {pass_!r}")
    if layout not in ("nhwc", "nchw"):
        raise ValueError(f"layout must be 'nhwc' or 'nchw', got {layout!r}")
    k, stride = int(k), int(stride)
    if k not in (1, 3) or stride not in (1, 2):
        raise ValueError(f"k must be 1 or 3 and stride 1 or 2, got k = {k}, stride = {stride}")
    nchw = layout == "nchw"
    if nchw and pass_ == "dgrad":
        raise ValueError("the planar (nchw) input has no gradient: dgrad needs layout='nhwc'")
    if not (torch.is_tensor(a) and a.dim() == 4 and torch.is_tensor(b) and b.dim() == 4):
        raise ValueError("both operands must be 4-d tensors")
    if nchw:
        if a.shape[2] != a.shape[3]:
            raise ValueError("the first operand must be [B,cin,S,S]")
        B, Ca, S1 = int(a.shape[0]), int(a.shape[1]), int(a.shape[2])
    else:
        if a.shape[1] != a.shape[2]:
            raise ValueError("the first operand must be [B,S,S,C]")
        B, S1, Ca = int(a.shape[0]), int(a.shape[1]), int(a.shape[3])
    if pass_ == "dgrad":
        cout, cin = Ca, int(b.shape[1])
        if size is None:
            if stride != 1:
                raise ValueError("dgrad under stride 2 needs size=, the forward's input size")
            size = S1
        S = int(size)
        if _out_size(S, k, stride) != S1:
            raise ValueError(f"size {S} does not give dy's {S1} under k = {k}, stride = {stride}")
    else:
        S, cin = S1, Ca
        cout = int(b.shape[3]) if pass_ == "wgrad" else int(b.shape[0])
    So = _out_size(S, k, stride)
    if (not 1 <= cin <= 4) if nchw else (cin < 4 or cin % 4):
        raise ValueError(f"cin must be a multiple of 4 (1..4 with layout='nchw'), got {cin}")
    if cout < 4 or cout % 4:
        raise ValueError(f"cout must be a multiple of 4, got {cout}")
    want = (B, So, So, cout) if pass_ == "wgrad" else (cout, cin, k, k)
    if tuple(b.shape) != want:
        raise ValueError(f"the second operand of {pass_!r} must be {want}")
    if not a.is_cuda or b.device != a.device:
        raise _lib.YoloLiteHipError("conv needs both operands on one HIP device (no CPU fallback)")
    lib = _lib.load()
    a = a.detach().float().contiguous()
    if not nchw:
        a = tm.aligned(a)
    b = b.detach().float().contiguous()
    if pass_ == "wgrad":
        b = tm.aligned(b)
    shape = {"forward": (B, So, So, cout), "dgrad": (B, S, S, cin), "wgrad": (cout, cin, k, k)}[pass_]
    out = torch.empty(shape, device=a.device, dtype=torch.float32)
    n = C.c_int32()
    with torch.cuda.device(a.device):
        stream = torch.cuda.current_stream(a.device).cuda_stream
        if precision is None:
            _lib.check(lib.yl_stem_conv(a.data_ptr(), b.data_ptr(), out.data_ptr(), PASSES[pass_], k, stride, B, S, cin, cout,
                                        int(nchw), stream, C.byref(n)), what="yl_stem_conv")
        else:
            _lib.check(lib.yl_amp_stem_conv(a.data_ptr(), b.data_ptr(), out.data_ptr(), PASSES[pass_], k, stride, B, S, cin,
                                            cout, int(nchw), tm.PRECISIONS[precision], stream, C.byref(n)),
                       what="yl_amp_stem_conv")
    conv.last_launches = int(n.value)
    return out


conv.last_launches = 0
