"""A trainable backbone stage on the device: a stack of MobileNetV4 UIB blocks (timm's UniversalInvertedResidual) and
1x1 ConvBnAct blocks, with a backward pass (csrc/yl_stage.hip).

    UIBStack(in_channels, blocks, eps=1e-5, prefix="", precision="fp32")     any such stack
    BackboneTail.from_meta(meta) / .from_state_dict(meta, sd)   the backbone's last stage: its C4 tap -> its C5 tap
    BackboneMid.from_meta(meta) / .from_state_dict(meta, sd)    the stage between its C3 and its C4 tap
    MobileNetV4Backbone.from_meta(meta) / .from_state_dict(meta, sd)   image -> [c3, c4, c5]: stemops.BackboneStem, mid, tail
    depthwise(x, w_or_dy, pass_, k, stride, same=False)    one depthwise pass on its own (yl_stage_depthwise)
    plan(in_channels, blocks, batch, size)                 yl_stage_plan: what the handle holds

    c3, c4, _ = model.features(x)                          # NHWC; the executor's frozen stages 0..3
    c5 = tail(c4)                                          # NHWC [B,S/2,S/2,C5]
    ps = neck([c3, c4, c5], layout="nhwc")
    loss.backward()                                        # .grad of the tail's parameters, and of c4 if it requires grad

`blocks` is a list of dicts in the arch-string fields: {"type": "uir", "a": 5, "k": 5, "s": 2, "mid": 288, "c": 96} or
{"type": "cn", "k": 1, "s": 1, "c": 960}; an optional "name" ("4.0") is the block's place `blocks.{i}.{j}` in the key
names (default "0.{index}").  A uir block is  [dw_start: depthwise a x a, BN]  pw_exp: 1x1, BN, ReLU  [dw_mid: depthwise
k x k stride s, BN, ReLU]  pw_proj: 1x1, BN,  plus its input when cin == c and s == 1; dw_start carries the stride when
k == 0.  Parameters and buffers carry timm's names and shapes under `prefix`
(`blocks.{i}.{j}.dw_start.conv.weight` [C,1,a,a], `...dw_start.bn.weight/bias/running_mean/running_var/
num_batches_tracked`, `pw_exp.*`, `dw_mid.*`, `pw_proj.*`; `conv.weight`, `bn1.*` for cn blocks), so state_dict() merges
into a checkpoint and FusedTrainStep takes parameters().

The whole stack is ONE torch.autograd.Function (_trainmod.UnitStackFunction, which the dense stem shares) over
yl_stage_forward / yl_stage_backward.  train() / eval() select the
BatchNorm mode.  Gradients nobody asked for are not computed, and nothing upstream of the first one wanted runs
(`last_launches` says what ran).  One forward is held for backward at a time: a second forward before backward()
replaces it, and the stale backward raises.  fp32 tensors on one HIP device; no CPU fallback.  precision="fp16" / "bf16"
(constructor, from_meta / from_state_dict, or the settable `.precision`; MobileNetV4Backbone sets all three parts) runs the
1x1 GEMMs (pw_exp, pw_proj, cn) of all three passes on 16-bit MFMA: operands rounded to nearest even inside the GEMM, fp32
accumulation, nothing clamped.  Parameters, saved activations and gradients stay fp32, and so do the depthwise
convolutions, BatchNorm, ReLU and the residual: unlike torch.autocast, which also runs the depthwise convolutions in 16
bits.  A backward runs in the precision of its forward.  ReLU only: relu6, silu, TF-SAME
padding, squeeze-excite and layer-scale are refused by name, as are the backbone families built from other blocks
(ReLU6, TF-SAME and timm's `ir` block, i.e. the EfficientNet-Lite stages, are irops.IRStack's).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch
from torch import nn

from . import _lib
from . import _trainmod as tm

UNITS = ("dw_start", "pw_exp", "dw_mid", "pw_proj")
_NOT_HERE = ("se", "layer_scale", "ls")


def _out_size(S: int, k: int, s: int) -> int:
    return (S + 2 * ((k - 1) // 2) - k) // s + 1


def _check_blocks(in_channels, blocks, eps) -> List[dict]:
    """host-side facts only: -> the blocks as dicts with every field present (cin among them)"""
    if int(in_channels) < 4 or int(in_channels) % 4:
        raise _lib.YoloLiteHipError(f"in_channels must be a multiple of 4, got {in_channels}")
    blocks = list(blocks)
    if not 1 <= len(blocks) <= _lib.YL_STAGE_MAX_BLOCKS:
        raise _lib.YoloLiteHipError(f"1..{_lib.YL_STAGE_MAX_BLOCKS} blocks, got {len(blocks)}")
    if not float(eps) > 0:
        raise _lib.YoloLiteHipError(f"eps must be positive, got {eps}")
    out, cin = [], int(in_channels)
    for i, b in enumerate(blocks):
        b = dict(b)
        act = str(b.get("act", "relu")).lower()
        if act != "relu":
            raise _lib.YoloLiteHipError(f"block {i}: activation {act!r} is not implemented (ReLU only)")
        if b.get("same"):
            raise _lib.YoloLiteHipError(f"block {i}: TF-SAME padding is not implemented (symmetric padding (k - 1) / 2 only)")
        for n in _NOT_HERE:
            if b.get(n):
                what = "squeeze-excite (se)" if n == "se" else "layer-scale"
                raise _lib.YoloLiteHipError(f"block {i}: {what} is not implemented")
        t = b.get("type")
        c = int(b.get("c", 0))
        if c < 4 or c % 4:
            raise _lib.YoloLiteHipError(f"block {i}: channels must be multiples of 4, got c = {c}")
        if t == "cn":
            if int(b.get("k", 1)) != 1 or int(b.get("s", 1)) != 1:
                raise _lib.YoloLiteHipError(f"block {i}: a cn block must be 1x1 with stride 1, got k = {b.get('k')}, s = {b.get('s')}")
            d = dict(type="cn", a=0, k=1, s=1, mid=0, c=c)
        elif t == "uir":
            a, k, s, mid = (int(b.get(n, 0)) for n in ("a", "k", "s", "mid"))
            if a not in (0, 3, 5) or k not in (0, 3, 5):
                raise _lib.YoloLiteHipError(f"block {i}: a and k must be 0, 3 or 5, got a = {a}, k = {k}")
            if s not in (1, 2):
                raise _lib.YoloLiteHipError(f"block {i}: s must be 1 or 2, got {s}")
            if s == 2 and not a and not k:
                raise _lib.YoloLiteHipError(f"block {i}: s = 2 needs a depthwise convolution to carry it (a = k = 0)")
            if mid < 4 or mid % 4:
                raise _lib.YoloLiteHipError(f"block {i}: channels must be multiples of 4, got mid = {mid}")
            d = dict(type="uir", a=a, k=k, s=s, mid=mid, c=c)
        else:
            raise _lib.YoloLiteHipError(f"block {i}: type {t!r} is not implemented (only 'uir' and 1x1 'cn' blocks are)")
        d["cin"] = cin
        d["name"] = str(b.get("name", f"0.{i}"))
        out.append(d)
        cin = c
    if len({d["name"] for d in out}) != len(out):
        raise ValueError("block names must differ")
    return out


def _units(d: dict) -> List[str]:
    """the units a block has, in the order they run"""
    if d["type"] == "cn":
        return ["pw_exp"]
    return [u for u in UNITS if not (u == "dw_start" and not d["a"]) and not (u == "dw_mid" and not d["k"])]


def _sizes(blocks: List[dict], S: int) -> List[int]:
    """the size of the map every unit of every block writes, in running order"""
    out = []
    for d in blocks:
        for u in _units(d):
            if u == "dw_start":
                S = _out_size(S, d["a"], d["s"] if not d["k"] else 1)
            elif u == "dw_mid":
                S = _out_size(S, d["k"], d["s"])
            out.append(S)
    return out


def _cfg(in_channels, blocks, eps):
    c = _lib.yl_stage_cfg()
    c.in_channels, c.num_blocks, c.eps = int(in_channels), len(blocks), float(eps)
    for i, d in enumerate(blocks):
        b = c.block[i]
        b.type = _lib.YL_STAGE_CN if d["type"] == "cn" else _lib.YL_STAGE_UIR
        b.a, b.k, b.s, b.mid, b.cout = d["a"], d["k"], d["s"], d["mid"], d["c"]
    return c


def plan(in_channels: int, blocks: Sequence[dict], batch: int, size: int, eps: float = 1e-5) -> Dict:
    """yl_stage_plan (a host function; no device): how every block's rows are cut and what the handle holds.
    -> {"stat_rows", "gemm_rows", "blocks": [{size_in, size_mid, size_out, rows_mid, rows_out, stat_tiles_mid,
    stat_tiles_out, exp_rows, exp_splits, proj_rows, proj_splits, units, saved_bytes}], "saved_bytes", "nosave_bytes",
    "workspace_bytes"} with, per unit u (a convolution and its BatchNorm), M_u = batch * S_u^2 rows and C_u channels of
    its OUTPUT, M_0 C_0 those of x:
        blocks[i].saved_bytes = sum over its units of 2 M_u C_u 4 + 2 C_u 4          z, h and (mean, invstd)
        saved_bytes           = M_0 C_0 4 + sum of the blocks'                       and a copy of x
        nosave_bytes          = 4 Amax + 2 Cmax 4,  Amax = max_u M_u C_u 4, Cmax = max_u C_u
        workspace_bytes       = 3 max(Amax, M_0 C_0 4) + max_u round16(tiles_u T_u C_u 8) + 2 Cmax 4
                                + max over the 1x1 units of round16(splits_u cin_u cout_u 4)
    tiles_u = ceil(M_u / stat_rows); T_u = k^2 for a depthwise unit, 2 for a 1x1; splits_u as the heads cut an
    NP x NQ weight gradient over M rows."""
    blocks = _check_blocks(in_channels, blocks, eps)
    cfg = _cfg(in_channels, blocks, eps)
    out = _lib.yl_stage_plan_info()
    _lib.check(_lib.load().yl_stage_plan(C.byref(cfg), int(batch), int(size), C.byref(out)), what="yl_stage_plan")
    bl = [{n: int(getattr(out.block[i], n)) for n, _ in out.block[i]._fields_} for i in range(len(blocks))]
    return {"stat_rows": int(out.stat_rows), "gemm_rows": int(out.gemm_rows), "blocks": bl,
            "saved_bytes": int(out.saved_bytes), "nosave_bytes": int(out.nosave_bytes),
            "workspace_bytes": int(out.workspace_bytes)}


class _Handle(tm.UnitStackHandle):
    """The stack's handle (see _trainmod.UnitStackHandle) and the order its tensors go to the library in"""
    who = "UIBStack"

    def __init__(self, in_channels: int, blocks: List[dict], eps: float):
        super().__init__("yl_stage", _cfg, in_channels, [dict(d) for d in blocks], eps)
        self.unit_names = [_units(d) for d in blocks]

    def table(self, tensors: Sequence[Optional[torch.Tensor]], buffers=None):
        """yl_stage_tensors from a list in UIBStack._param_list() order: per unit w, gamma, beta (None = NULL)"""
        t = _lib.yl_stage_tensors()
        o = 0
        for i, names in enumerate(self.unit_names):
            for u in names:
                e = getattr(t.block[i], u)
                e.w, e.gamma, e.beta = (tm.ptr(v) for v in tensors[3 * o:3 * o + 3])
                if buffers is not None:
                    e.running_mean, e.running_var, e.num_batches_tracked = (tm.ptr(v) for v in buffers[o])
                o += 1
        return t


class _TailHandle(_Handle):
    who = "BackboneTail"


def _conv_bn(cin: int, cout: int, k: int, s: int, groups: int, eps: float, names=("conv", "bn")) -> nn.Module:
    """Container only (timm's ConvNormAct / ConvBnAct): the layers hold the parameters; their forward is never called."""
    m = nn.Module()
    setattr(m, names[0], nn.Conv2d(cin, cout, k, s, padding=k // 2, groups=groups, bias=False))
    setattr(m, names[1], nn.BatchNorm2d(cout, eps=eps))
    return m


def _nest(root: nn.Module, path: str, module: nn.Module):
    """register `module` under the dotted `path` below `root`, through plain containers made on the way"""
    parts = [p for p in path.split(".") if p]
    for p in parts[:-1]:
        if not hasattr(root, p):
            root.add_module(p, nn.Module())
        root = getattr(root, p)
    root.add_module(parts[-1], module)


class UIBStack(tm.UnitStack):
    """See the module docstring."""
    _who, _handle_cls = "UIBStack", _Handle

    def __init__(self, in_channels: int, blocks: Sequence[dict], eps: float = 1e-5, prefix: str = "", precision: str = "fp32"):
        super().__init__()
        self._setup(in_channels, _check_blocks(in_channels, blocks, eps), eps, prefix, precision)

    def _setup(self, in_channels: int, blocks_cfg: List[dict], eps: float, prefix: str, precision: str):
        """the constructor behind the checks (irops.IRStack shares it): the blocks' containers under their key names, the
        units' layers in running order, the handle"""
        self.precision = precision
        self.blocks_cfg = blocks_cfg
        self.in_channels, self.eps, self.prefix = int(in_channels), float(eps), str(prefix)
        self.out_channels = self.blocks_cfg[-1]["c"]
        self._convs, self._bns = [], []
        for d in self.blocks_cfg:
            _nest(self, f"{self.prefix}blocks.{d['name']}", self._block_module(d))
        self._handle = self._make_handle()

    def _make_handle(self):
        return self._handle_cls(self.in_channels, self.blocks_cfg, self.eps)

    def _block_module(self, d: dict) -> nn.Module:
        """the container of one block under timm's names; appends its units' layers to _convs / _bns in running order"""
        cin, mid, c = d["cin"], d["mid"], d["c"]
        if d["type"] == "cn":
            blk = _conv_bn(cin, c, 1, 1, 1, self.eps, names=("conv", "bn1"))
            self._convs.append(blk.conv); self._bns.append(blk.bn1)
            return blk
        blk = nn.Module()
        for u in _units(d):
            if u == "dw_start":
                m = _conv_bn(cin, cin, d["a"], d["s"] if not d["k"] else 1, cin, self.eps)
            elif u == "pw_exp":
                m = _conv_bn(cin, mid, 1, 1, 1, self.eps)
            elif u == "dw_mid":
                m = _conv_bn(mid, mid, d["k"], d["s"], mid, self.eps)
            else:
                m = _conv_bn(mid, c, 1, 1, 1, self.eps)
            blk.add_module(u, m)
            self._convs.append(m.conv); self._bns.append(m.bn)
        return blk

    def out_size(self, size: int) -> int:
        return _sizes(self.blocks_cfg, int(size))[-1]

    def _unit_sizes(self, S: int) -> List[int]:
        return _sizes(self.blocks_cfg, S)

    def forward(self, x: torch.Tensor, layout: Optional[str] = None) -> torch.Tensor:
        """`x`: "nchw" ([B,Cin,S,S], any strides) or "nhwc" ([B,S,S,Cin]); None reads the layout off the shape and
        refuses a shape that is both.  -> NHWC [B,S_out,S_out,C_out]."""
        if layout not in (None, "nchw", "nhwc"):
            raise ValueError(f"layout must be 'nchw', 'nhwc' or None, got {layout!r}")
        try:
            x = tm.as_nhwc(x, self.in_channels, layout, self._who, False, name="Cin")
        except _lib.YoloLiteHipError:                      # the shape is right (B first, S third in either layout), the device
            self._check_rows(int(x.shape[0]), int(x.shape[2]))   # is not: what BatchNorm refuses comes first all the same
            raise
        B, S = int(x.shape[0]), int(x.shape[1])
        return self._run_stack(x, B, self._check_rows(B, S), False)


def _arch_walk(spec: dict):
    """-> (taps, blocks): the stages of a program.BACKBONES entry a feature is tapped behind, and every block of the
    backbone in running order as (stage, index in the stage, arch string, its fields, stride, cin, cout), with
    program._backbone's channel and depth arithmetic (cmult, dmult, fix_first_last, _make_divisible)"""
    import math
    from .program import _make_divisible, _parse
    arch, rlim = spec["arch"], spec.get("round_limit", 0.9)
    ns = len(arch)
    taps = [si for si in range(ns) if si + 1 == ns or _parse(arch[si + 1][0])["s"] > 1]
    out, cin = [], spec["stem"]
    for si, stage in enumerate(arch):
        bi = 0
        for bstr in stage:
            d = _parse(bstr)
            rep = d["r"]
            if spec["dmult"] != 1.0 and not (spec["fix_first_last"] and si in (0, ns - 1)):
                rep = int(math.ceil(rep * spec["dmult"]))
            cout = _make_divisible(d["c"] * spec["cmult"], 8, rlim)
            for r in range(rep):
                out.append((si, bi, bstr, d, d["s"] if r == 0 else 1, cin, cout))
                cin = cout
                bi += 1
    return taps, out


def _meta_backbone(meta: dict) -> str:
    mcfg = (meta.get("config", {}) or {}).get("model", {}) or {}
    return meta.get("backbone") or mcfg.get("backbone") or "resnet18"


def _tail_blocks(meta: dict, start: str = "c4"):
    """-> (cin at the C4 tap, blocks with their names "si.bi", eps) of the backbone `meta` names, read from
    program.BACKBONES with program._backbone's channel arithmetic.  Host-side facts only; refuses by name."""
    from .program import BACKBONES, CONVNEXT, HGNET, _make_divisible
    if start != "c4":
        raise _lib.YoloLiteHipError(f"BackboneTail: start={start!r} is not implemented (only the C4 tap -> C5 tail is; "
                                    "stages 0..3 stay the executor's)")
    name = _meta_backbone(meta)
    if name in HGNET or name in CONVNEXT or name not in BACKBONES:
        raise _lib.YoloLiteHipError(f"BackboneTail: backbone {name!r} is not implemented (its tail is not made of uir / 1x1 cn "
                                    "blocks; only the mobilenetv4_conv_small family's is)")
    spec = BACKBONES[name]
    if spec["act"] != "relu":
        raise _lib.YoloLiteHipError(f"BackboneTail: backbone {name!r} is not implemented: activation {spec['act']!r} (ReLU only; "
                                    "the EfficientNet-Lite family: see EfficientNetLiteTail)")
    if spec["same"]:
        raise _lib.YoloLiteHipError(f"BackboneTail: backbone {name!r} is not implemented: TF-SAME padding")
    taps, walk = _arch_walk(spec)
    if len(taps) < 2:
        raise _lib.YoloLiteHipError(f"BackboneTail: backbone {name!r} has no C4 tap")
    c4, blocks = None, []
    for si, bi, bstr, d, s, cin, cout in walk:
        if si > taps[-2]:
            if d["type"] not in ("uir", "cn") or d.get("se") or d.get("skip"):
                raise _lib.YoloLiteHipError(f"BackboneTail: backbone {name!r} is not implemented: block {bstr!r} of its "
                                            "tail is not a uir or 1x1 cn block")
            blocks.append(dict(type=d["type"], a=d.get("a", 0), k=d["k"], s=s, c=cout, name=f"{si}.{bi}",
                               mid=_make_divisible(cin * d["e"], 8) if d["type"] == "uir" else 0))
        elif si == taps[-2]:
            c4 = cout
    return c4, blocks, float(spec["eps"])


class BackboneTail(UIBStack):
    """The stack from the backbone's C4 tap to its C5 tap (mobilenetv4_conv_small[_050]: `backbone.blocks.3.*`, six UIB
    blocks of which the first strides, and `backbone.blocks.4.0`, the 1x1 ConvBnAct), under the checkpoint's key names: state_dict() merges into a
    checkpoint.  tail(c4) -> c5, both NHWC."""
    _who, _handle_cls = "BackboneTail", _TailHandle

    @classmethod
    def from_meta(cls, meta: dict, start: str = "c4", precision: str = "fp32"):
        """a freshly initialised tail of the model `meta` describes"""
        tm.check_precision(precision)
        cin, blocks, eps = _tail_blocks(meta, start)
        return cls(cin, blocks, eps=eps, prefix="backbone.", precision=precision)

    @classmethod
    def from_state_dict(cls, meta: dict, sd: dict, start: str = "c4", precision: str = "fp32"):
        """the tail of a checkpoint: built from its meta, filled with its `backbone.blocks.{si}.{bi}.` entries"""
        return tm.fill_from_state_dict(cls.from_meta(meta, start, precision), sd, "backbone tail")


def _mid_blocks(meta: dict):
    """-> (cin at the C3 tap, blocks with their names "si.bi", eps) of the stages between the C3 and the C4 tap of the
    backbone `meta` names (mobilenetv4_conv_small[_050]: stage 2, six uir blocks).  Host-side facts only; refuses by name."""
    from .program import BACKBONES, CONVNEXT, HGNET, _make_divisible
    who = "BackboneMid"
    name = _meta_backbone(meta)
    if name in HGNET or name in CONVNEXT or name not in BACKBONES:
        raise _lib.YoloLiteHipError(f"{who}: backbone {name!r} is not implemented (its C3 -> C4 stage is not made of uir / 1x1 cn "
                                    "blocks; only the mobilenetv4_conv_small family's is)")
    spec = BACKBONES[name]
    if spec["act"] != "relu":
        raise _lib.YoloLiteHipError(f"{who}: backbone {name!r} is not implemented: activation {spec['act']!r} (ReLU only; "
                                    "the EfficientNet-Lite family: see EfficientNetLiteMid)")
    if spec["same"]:
        raise _lib.YoloLiteHipError(f"{who}: backbone {name!r} is not implemented: TF-SAME padding")
    taps, walk = _arch_walk(spec)
    if len(taps) < 3:
        raise _lib.YoloLiteHipError(f"{who}: backbone {name!r} has no C3 tap")
    c3, blocks = None, []
    for si, bi, bstr, d, s, cin, cout in walk:
        if taps[-3] < si <= taps[-2]:
            if d["type"] not in ("uir", "cn") or d.get("se") or d.get("skip"):
                raise _lib.YoloLiteHipError(f"{who}: backbone {name!r} is not implemented: block {bstr!r} of its C3 -> C4 "
                                            "stage is not a uir or 1x1 cn block")
            blocks.append(dict(type=d["type"], a=d.get("a", 0), k=d["k"], s=s, c=cout, name=f"{si}.{bi}",
                               mid=_make_divisible(cin * d["e"], 8) if d["type"] == "uir" else 0))
        elif si == taps[-3]:
            c3 = cout
    return c3, blocks, float(spec["eps"])


class _MidHandle(_Handle):
    who = "BackboneMid"


class BackboneMid(UIBStack):
    """The stack from the backbone's C3 tap to its C4 tap (mobilenetv4_conv_small[_050]: `backbone.blocks.2.*`, six UIB
    blocks of which the first strides) under the checkpoint's key names.  mid(c3) -> c4, both NHWC."""
    _who, _handle_cls = "BackboneMid", _MidHandle

    @classmethod
    def from_meta(cls, meta: dict, precision: str = "fp32"):
        tm.check_precision(precision)
        cin, blocks, eps = _mid_blocks(meta)
        return cls(cin, blocks, eps=eps, prefix="backbone.", precision=precision)

    @classmethod
    def from_state_dict(cls, meta: dict, sd: dict, precision: str = "fp32"):
        return tm.fill_from_state_dict(cls.from_meta(meta, precision), sd, "backbone C3 -> C4 stage")


class MobileNetV4Backbone(nn.Module):
    """The whole mobilenetv4_conv_small[_050] backbone with every parameter trainable: .stem (stemops.BackboneStem, image ->
    C3), .mid (BackboneMid, C3 -> C4), .tail (BackboneTail, C4 -> C5).  backbone(x [B,3,S,S]) -> [c3, c4, c5] NHWC,
    smallest stride first: what neck(cs, layout="nhwc") takes.  torch sums the two gradients that arrive at C3 and at C4.
    Freezing is torch's own: backbone.stem.requires_grad_(False).eval(); nothing upstream of the first wanted gradient
    runs.  state_dict() / load_state_dict() speak the checkpoint's key names (`backbone.conv_stem.weight`, ...).
    `precision` (None: the parts keep theirs) and the settable `.precision` set the operand type of every dense GEMM of all
    three parts; reading `.precision` while the parts differ raises."""

    def __init__(self, stem: nn.Module, mid: nn.Module, tail: nn.Module, precision: Optional[str] = None):
        super().__init__()
        if precision is not None:
            tm.check_precision(precision)
        self.stem, self.mid, self.tail = stem, mid, tail
        if precision is not None:
            self.precision = precision

    @property
    def precision(self) -> str:
        ps = [p.precision for p in (self.stem, self.mid, self.tail)]
        if len(set(ps)) != 1:
            raise ValueError(f"the backbone's parts differ in precision: stem {ps[0]!r}, mid {ps[1]!r}, tail {ps[2]!r}")
        return ps[0]

    @precision.setter
    def precision(self, value):
        tm.check_precision(value)
        for p in (self.stem, self.mid, self.tail):
            p.precision = value

    @classmethod
    def from_meta(cls, meta: dict, precision: str = "fp32"):
        from .stemops import BackboneStem
        tm.check_precision(precision)
        return cls(BackboneStem.from_meta(meta, precision), BackboneMid.from_meta(meta, precision),
                   BackboneTail.from_meta(meta, precision=precision))

    @classmethod
    def from_state_dict(cls, meta: dict, sd: dict, precision: str = "fp32"):
        m = cls.from_meta(meta, precision)
        m.load_state_dict(sd)
        return m

    def state_dict(self, *args, **kwargs):                 # the three parts' own keys, which are the checkpoint's
        out = self.stem.state_dict()
        out.update(self.mid.state_dict())
        out.update(self.tail.state_dict())
        return out

    def load_state_dict(self, sd, strict: bool = True):
        for part, what in ((self.stem, "backbone stem"), (self.mid, "backbone C3 -> C4 stage"), (self.tail, "backbone tail")):
            tm.fill_from_state_dict(part, sd, what)
        return self

    def forward(self, x: torch.Tensor) -> List[torch.Tensor]:
        c3 = self.stem(x)
        c4 = self.mid(c3, layout="nhwc")
        c5 = self.tail(c4, layout="nhwc")
        return [c3, c4, c5]


PASSES = {"forward": _lib.YL_STAGE_PASS_FORWARD, "dgrad": _lib.YL_STAGE_PASS_DGRAD, "wgrad": _lib.YL_STAGE_PASS_WGRAD}


def depthwise(x: torch.Tensor, w_or_dy: torch.Tensor, pass_: str, k: int, stride: int, size: Optional[int] = None,
              same: bool = False) -> torch.Tensor:
    """One depthwise pass of the stack on its own (yl_stage_depthwise, launched as the module launches it), fp32 NHWC
    tensors on one HIP device, pad (k - 1) / 2, So = (S + 2 pad - k) / stride + 1; with `same` TF-SAME padding
    (yl_variant_stage_depthwise): the same So, the leading pad irops.pad_begin(k, stride, S):
        "forward":  x  [B,S,S,C],   W  [C,1,k,k]    -> y  [B,So,So,C]
        "dgrad":    dy [B,So,So,C], W  [C,1,k,k]    -> dx [B,S,S,C]      the gradient of forward's x
        "wgrad":    x  [B,S,S,C],   dy [B,So,So,C]  -> dW [C,1,k,k]      the gradient of forward's W
    `size`: S of "dgrad", which So does not determine under stride 2 (stride 1: S = So).  The weight may start at any
    4-byte boundary (a view into a larger tensor is taken as it is)."""
    if pass_ not in PASSES:
        raise ValueError(f"pass_ must be one of {sorted(PASSES)}, got {pass_!r}")
    k, stride = int(k), int(stride)
    if k not in (3, 5) or stride not in (1, 2):
        raise ValueError(f"k must be 3 or 5 and stride 1 or 2, got k = {k}, stride = {stride}")
    if not (torch.is_tensor(x) and x.dim() == 4 and x.shape[1] == x.shape[2]):
        raise ValueError("the first operand must be [B,S,S,C]")
    B, S1, _, Cn = (int(v) for v in x.shape)
    if Cn < 4 or Cn % 4:
        raise ValueError(f"channels must be a multiple of 4, got {Cn}")
    if pass_ == "dgrad":
        if size is None:
            if stride != 1:
                raise ValueError("dgrad under stride 2 needs size=, the forward's input size")
            size = S1
        S = int(size)
        if _out_size(S, k, stride) != S1:
            raise ValueError(f"size {S} does not give dy's {S1} under k = {k}, stride = {stride}")
    else:
        S = S1
    So = _out_size(S, k, stride)
    want = (B, So, So, Cn) if pass_ == "wgrad" else (Cn, 1, k, k)
    if not torch.is_tensor(w_or_dy) or tuple(w_or_dy.shape) != want:
        raise ValueError(f"the second operand of {pass_!r} must be {want}")
    if not x.is_cuda or w_or_dy.device != x.device:
        raise _lib.YoloLiteHipError("depthwise needs both operands on one HIP device (no CPU fallback)")
    lib = _lib.load()
    a = tm.aligned(x.detach().float().contiguous())
    b = w_or_dy.detach().float().contiguous()
    if pass_ == "wgrad":
        b = tm.aligned(b)
    shape = {"forward": (B, So, So, Cn), "dgrad": (B, S, S, Cn), "wgrad": (Cn, 1, k, k)}[pass_]
    out = torch.empty(shape, device=a.device, dtype=torch.float32)
    n = C.c_int32()
    with torch.cuda.device(a.device):
        stream = torch.cuda.current_stream(a.device).cuda_stream
        if same:
            _lib.check(lib.yl_variant_stage_depthwise(a.data_ptr(), b.data_ptr(), out.data_ptr(), PASSES[pass_], k, stride, B, S,
                                                      Cn, 1, stream, C.byref(n)), what="yl_variant_stage_depthwise")
        else:
            _lib.check(lib.yl_stage_depthwise(a.data_ptr(), b.data_ptr(), out.data_ptr(), PASSES[pass_], k, stride, B, S, Cn,
                                              stream, C.byref(n)), what="yl_stage_depthwise")
    return out
