"""The trainable stages of the EfficientNet-Lite backbones (tf_efficientnet_lite0..4, the backbones of yololite_n .. xl) on
the device: stacks of timm's InvertedResidual blocks under ReLU6 and TF-SAME padding, with a backward pass.

    IRStack(in_channels, blocks, eps=1e-3, act="relu6", same=True, prefix="", precision="fp32")    any such stack
    EfficientNetLiteTail.from_meta(meta) / .from_state_dict(meta, sd)   the C4 tap -> the C5 tap: arch stages 5 and 6
    EfficientNetLiteMid.from_meta(meta) / .from_state_dict(meta, sd)    the C3 tap -> the C4 tap: arch stages 3 and 4
    tail_for(meta, sd, precision="fp32")                    BackboneTail or EfficientNetLiteTail, by the backbone's family
    pad_begin(k, s, S, same=True) / out_size(S, s)          TF-SAME's leading pad and output size
    plan(in_channels, blocks, batch, size)                  yl_stage_plan: what the handle holds

`blocks` is a list of dicts {"type": "ir", "k": 3 | 5, "s": 1 | 2, "mid": 480, "c": 112, "name": "5.0"}: conv_pw 1x1
cin -> mid, bn1, act; conv_dw depthwise k x k stride s, bn2, act; conv_pwl 1x1 mid -> c, bn3; plus the block's input when
cin == c and s == 1.  Parameters and buffers carry timm's names and shapes under `prefix`
(`blocks.{i}.{j}.conv_pw.weight` [mid,cin,1,1], `bn1.weight/bias/running_mean/running_var/num_batches_tracked`,
`conv_dw.weight` [mid,1,k,k], `bn2.*`, `conv_pwl.weight` [c,mid,1,1], `bn3.*`), so state_dict() merges into a checkpoint
and FusedTrainStep takes parameters().

Unit for unit an `ir` block without squeeze-excite is a `uir` block with a = 0, so an IRStack IS a stageops.UIBStack over
the same library handle (yl_stage_*), whose variant (yl_variant_stage_set) it sets once: `act` "relu6" or "relu", `same`
True (TF-SAME: So = ceil(S / s), leading pad pad_begin) or False ((k - 1) / 2 on every side).  Everything else is
UIBStack's: ONE autograd.Function, train() / eval(), `last_launches` and the per-unit launch counts, gradients nobody asked
for are not computed, one forward held for backward at a time, NHWC / NCHW input, `precision` "fp16" / "bf16" for the 1x1
GEMMs.  IRStack(act="relu", same=False) computes, bit for bit, what UIBStack computes of the equivalent a = 0 blocks.

Refused by name, from host-side checks before the library is loaded: squeeze-excite, SiLU and any other activation;
uir / cn / ds / er blocks inside an IRStack; channels that are not multiples of 4; more than YL_STAGE_MAX_BLOCKS blocks; k
outside {3, 5}, s outside {1, 2}; any backbone but the five lite ones.  The family's stem (a dense 3x3 under TF-SAME) and
its stages 0 .. 2 (stage 0 is a `ds` block, whose 1x1 has no activation) stay the executor's: model.features(x).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Sequence

from torch import nn

from . import _lib
from . import _trainmod as tm
from . import stageops

ACTS = {"relu": _lib.YL_STAGE_ACT_RELU, "relu6": _lib.YL_STAGE_ACT_RELU6}
ACT_OF = {v: k for k, v in ACTS.items()}
LITE = tuple(f"tf_efficientnet_lite{i}" for i in range(5))


def out_size(S: int, s: int) -> int:
    """TF-SAME: ceil(S / s).  For odd k this is stageops' (S + 2 ((k - 1) / 2) - k) / s + 1"""
    return -(-int(S) // int(s))


def pad_begin(k: int, s: int, S: int, same: bool = True) -> int:
    """the zeros in front of the first row and column (csrc/yl_units.h pad_begin, the one place the library decides it):
    (k - 1) / 2, or under TF-SAME total / 2 rounded down of total = max((So - 1) s + k - S, 0)"""
    if not same:
        return (k - 1) // 2
    return max((out_size(S, s) - 1) * s + k - S, 0) // 2


def _check_blocks(in_channels, blocks, eps, act, same) -> List[dict]:
    """host-side facts only: -> the blocks in stageops' form (a uir block with a = 0 each; "type" stays "ir")"""
    act = str(act).lower()
    if act not in ACTS:
        raise _lib.YoloLiteHipError(f"IRStack: activation {act!r} is not implemented (relu6 and relu only)")
    if not isinstance(same, (bool, int)) or same not in (False, True):
        raise ValueError(f"same must be False or True, got {same!r}")
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
        t = b.get("type")
        if t != "ir":
            raise _lib.YoloLiteHipError(f"block {i}: type {t!r} is not implemented in an IRStack (only 'ir' blocks are; uir and "
                                        "1x1 cn blocks: see UIBStack)")
        bact = str(b.get("act", act)).lower()
        if bact != act:
            raise _lib.YoloLiteHipError(f"block {i}: activation {bact!r} is not implemented (the stack's {act!r} only)")
        if b.get("se"):
            raise _lib.YoloLiteHipError(f"block {i}: squeeze-excite (se) is not implemented")
        for n in ("layer_scale", "ls"):
            if b.get(n):
                raise _lib.YoloLiteHipError(f"block {i}: layer-scale is not implemented")
        k, s, mid, c = (int(b.get(n, 0)) for n in ("k", "s", "mid", "c"))
        if k not in (3, 5):
            raise _lib.YoloLiteHipError(f"block {i}: k must be 3 or 5, got {k}")
        if s not in (1, 2):
            raise _lib.YoloLiteHipError(f"block {i}: s must be 1 or 2, got {s}")
        for n, v in (("mid", mid), ("c", c)):
            if v < 4 or v % 4:
                raise _lib.YoloLiteHipError(f"block {i}: channels must be multiples of 4, got {n} = {v}")
        out.append(dict(type="ir", a=0, k=k, s=s, mid=mid, c=c, cin=cin, name=str(b.get("name", f"0.{i}"))))
        cin = c
    if len({d["name"] for d in out}) != len(out):
        raise ValueError("block names must differ")
    return out


def plan(in_channels: int, blocks: Sequence[dict], batch: int, size: int, eps: float = 1e-3) -> Dict:
    """yl_stage_plan of the stack: stageops.plan of the equivalent a = 0 blocks (the variant changes no size)"""
    cfg = _check_blocks(in_channels, blocks, eps, "relu6", True)
    return stageops.plan(in_channels, [dict(d, type="uir") for d in cfg], batch, size, eps)


class _Handle(stageops._Handle):
    """stageops' handle with the variant it is given when the library object is made (yl_variant_stage_set)"""
    who = "IRStack"

    def __init__(self, in_channels: int, blocks: List[dict], eps: float, act: str = "relu6", same: bool = True):
        super().__init__(in_channels, blocks, eps)
        self.variant = (str(act), bool(same))

    def __deepcopy__(self, memo):
        return type(self)(*self.args, *self.variant)

    def __reduce__(self):
        return type(self), tuple(self.args) + self.variant

    def ensure(self, device):
        fresh = self.handle is None or self.device != device
        super().ensure(device)
        if fresh:
            self.variant_set(*self.variant)

    def variant_set(self, act: str, same: bool):
        """yl_variant_stage_set: refused (YL_ERR_STATE) while a forward is held for backward"""
        _lib.check(self.lib.yl_variant_stage_set(self.handle, ACTS[act], int(bool(same))), what="yl_variant_stage_set")

    def variant_get(self) -> Dict[str, object]:
        if self.handle is None:
            return {"act": self.variant[0], "same": self.variant[1]}
        a, s = C.c_int32(), C.c_int32()
        _lib.check(self.lib.yl_variant_stage_get(self.handle, C.byref(a), C.byref(s)), what="yl_variant_stage_get")
        return {"act": ACT_OF[int(a.value)], "same": bool(s.value)}


class _TailHandle(_Handle):
    who = "EfficientNetLiteTail"


class _MidHandle(_Handle):
    who = "EfficientNetLiteMid"


class IRStack(stageops.UIBStack):
    """See the module docstring."""
    _who, _handle_cls = "IRStack", _Handle

    def __init__(self, in_channels: int, blocks: Sequence[dict], eps: float = 1e-3, act: str = "relu6", same: bool = True,
                 prefix: str = "", precision: str = "fp32"):
        nn.Module.__init__(self)
        cfg = _check_blocks(in_channels, blocks, eps, act, same)
        self.act, self.same = str(act).lower(), bool(same)
        self._setup(in_channels, cfg, eps, prefix, precision)

    def _make_handle(self):
        return self._handle_cls(self.in_channels, self.blocks_cfg, self.eps, self.act, self.same)

    def _block_module(self, d: dict) -> nn.Module:
        """Container only (timm's InvertedResidual): the layers hold the parameters; their forward is never called."""
        cin, mid, c, k = d["cin"], d["mid"], d["c"], d["k"]
        blk = nn.Module()
        blk.conv_pw, blk.bn1 = nn.Conv2d(cin, mid, 1, bias=False), nn.BatchNorm2d(mid, eps=self.eps)
        blk.conv_dw = nn.Conv2d(mid, mid, k, d["s"], padding=k // 2, groups=mid, bias=False)
        blk.bn2 = nn.BatchNorm2d(mid, eps=self.eps)
        blk.conv_pwl, blk.bn3 = nn.Conv2d(mid, c, 1, bias=False), nn.BatchNorm2d(c, eps=self.eps)
        self._convs += [blk.conv_pw, blk.conv_dw, blk.conv_pwl]
        self._bns += [blk.bn1, blk.bn2, blk.bn3]
        return blk

    def variant_state(self) -> Dict[str, object]:
        """yl_variant_stage_get: {"act", "same"} of the library object (of the module while there is none yet)"""
        return self._handle.variant_get()


def is_lite(meta: dict) -> bool:
    return stageops._meta_backbone(meta) in LITE


def _lite_blocks(meta: dict, who: str, part: str):
    """-> (cin at the tap the part starts from, blocks with their names "si.bi", eps, act, same) of the lite backbone
    `meta` names: part "tail" is what lies behind the C4 tap, "mid" what lies between the C3 and the C4 tap.  Read from
    program.BACKBONES with stageops._arch_walk's arithmetic.  Host-side facts only; refuses by name."""
    from .program import BACKBONES, _make_divisible
    name = stageops._meta_backbone(meta)
    if name not in LITE or name not in BACKBONES:
        raise _lib.YoloLiteHipError(f"{who}: backbone {name!r} is not implemented (only the tf_efficientnet_lite0..4 family's "
                                    "stages are made of ir blocks under relu6 and TF-SAME; mobilenetv4_conv_small: see "
                                    "BackboneTail / BackboneMid)")
    spec = BACKBONES[name]
    taps, walk = stageops._arch_walk(spec)
    lo, hi = (taps[-2], taps[-1]) if part == "tail" else (taps[-3], taps[-2])
    cin0, blocks = None, []
    for si, bi, bstr, d, s, cin, cout in walk:
        if lo < si <= hi:
            if d["type"] != "ir" or d.get("se") or d.get("skip"):
                raise _lib.YoloLiteHipError(f"{who}: backbone {name!r} is not implemented: block {bstr!r} is not an ir block "
                                            "without squeeze-excite")
            blocks.append(dict(type="ir", k=d["k"], s=s, c=cout, name=f"{si}.{bi}", mid=_make_divisible(cin * d["e"], 8)))
        elif si == lo:
            cin0 = cout
    return cin0, blocks, float(spec["eps"]), spec["act"], bool(spec["same"])


class _LitePart(IRStack):
    _part = ""

    @classmethod
    def from_meta(cls, meta: dict, precision: str = "fp32"):
        """a freshly initialised part of the model `meta` describes"""
        tm.check_precision(precision)
        cin, blocks, eps, act, same = _lite_blocks(meta, cls._who, cls._part)
        return cls(cin, blocks, eps=eps, act=act, same=same, prefix="backbone.", precision=precision)

    @classmethod
    def from_state_dict(cls, meta: dict, sd: dict, precision: str = "fp32"):
        """the part of a checkpoint: built from its meta, filled with its `backbone.blocks.{si}.{bi}.` entries"""
        return tm.fill_from_state_dict(cls.from_meta(meta, precision), sd, cls._what)


class EfficientNetLiteTail(_LitePart):
    """The stack from a lite backbone's C4 tap to its C5 tap (lite0: `backbone.blocks.5.0..3`, of which the first strides,
    and `backbone.blocks.6.0`) under the checkpoint's key names: state_dict() merges into a checkpoint.  tail(c4) -> c5,
    both NHWC."""
    _who, _handle_cls, _part, _what = "EfficientNetLiteTail", _TailHandle, "tail", "backbone tail"


class EfficientNetLiteMid(_LitePart):
    """The stack from a lite backbone's C3 tap to its C4 tap (lite0: `backbone.blocks.3.0..2`, of which the first strides,
    and `backbone.blocks.4.0..2`) under the checkpoint's key names.  mid(c3) -> c4, both NHWC."""
    _who, _handle_cls, _part, _what = "EfficientNetLiteMid", _MidHandle, "mid", "backbone C3 -> C4 stage"


def tail_for(meta: dict, sd: dict, precision: str = "fp32"):
    """the trainable C4 -> C5 tail of a checkpoint, by the backbone's family: stageops.BackboneTail (mobilenetv4_conv_small)
    or EfficientNetLiteTail (tf_efficientnet_lite0..4); any other backbone raises BackboneTail's refusal"""
    if is_lite(meta):
        return EfficientNetLiteTail.from_state_dict(meta, sd, precision)
    return stageops.BackboneTail.from_state_dict(meta, sd, precision=precision)
