"""The reference's loss on the device behind its own class surface: validation loss and training criterion.

    LossAF(num_classes, img_size, **kwargs)(preds, targets) -> (loss, {"box", "obj", "cls", "pos"})
        <- scripts/loss/loss.py:180-436 (same constructor arguments and defaults, same return)

The assignment and the three terms run in yl_loss_af (csrc/yl_loss.hip) on the raw level tensors `model(x)` returns.
By default the class is forward only: an input that requires grad is refused rather than silently detached.  With
`grad=True` such a call goes through torch autograd instead: the forward keeps the assignment and the hard-negative
selection (yl_loss_af_train), and `loss.backward()` runs yl_loss_af_backward, one kernel that writes the gradient of
every level tensor (the network's own backward is not part of this package).  The host's part is the reference's
target-format sniffing (_targets_to_xyxy_px: normalised xywh / normalised xyxy / pixel xyxy / pixel xywh, told apart
by value range) and packing the batch's boxes into one flat list.  No CPU fallback: a HIP device is required.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib


def targets_to_xyxy_px(tgt: dict, W: int, H: int) -> np.ndarray:
    """The reference's _targets_to_xyxy_px (loss.py:157-190) in float32 numpy: -> [n,4] pixel xyxy."""
    boxes = None
    for k in ("boxes", "bboxes", "xyxy"):
        if k in tgt and tgt[k] is not None:
            boxes = tgt[k]
            break
    if boxes is None:
        return np.zeros((0, 4), np.float32)
    if isinstance(boxes, torch.Tensor):
        boxes = boxes.detach().cpu().numpy()
    b = np.asarray(boxes, dtype=np.float32)
    if b.size == 0:
        return b.reshape(0, 4)
    f = np.float32

    def xywh_to_xyxy(bt):
        return np.stack([bt[:, 0] - bt[:, 2] * f(0.5), bt[:, 1] - bt[:, 3] * f(0.5),
                         bt[:, 0] + bt[:, 2] * f(0.5), bt[:, 1] + bt[:, 3] * f(0.5)], 1)

    b_min, b_max = float(b.min()), float(b.max())
    if -1e-3 <= b_min <= 1.01 and -1e-3 <= b_max <= 1.01:
        mean_wh = float((b[:, 2] + b[:, 3]).mean(dtype=np.float32))
        if mean_wh <= 2.01:      # normalised xywh
            return xywh_to_xyxy(np.stack([b[:, 0] * f(W), b[:, 1] * f(H), b[:, 2] * f(W), b[:, 3] * f(H)], 1))
        return np.stack([b[:, 0] * f(W), b[:, 1] * f(H), b[:, 2] * f(W), b[:, 3] * f(H)], 1)   # normalised xyxy
    likely_xyxy = float(((b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])).astype(np.float32).mean()) > 0.8
    return b if likely_xyxy else xywh_to_xyxy(b)


def pack_targets(targets: Sequence[dict], img_size: int, num_classes: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """list of target dicts -> (gt_xyxy [T,4] float32, gt_label [T] int32, gt_off [B+1] int32)"""
    bx, lb, off = [], [], [0]
    for i, t in enumerate(targets):
        b = targets_to_xyxy_px(t, img_size, img_size)
        l = t.get("labels")
        l = np.zeros((0,), np.int64) if l is None else (l.detach().cpu().numpy() if isinstance(l, torch.Tensor) else np.asarray(l))
        l = l.reshape(-1).astype(np.int64)
        if len(l) != len(b):
            raise ValueError(f"target {i}: {len(b)} boxes but {len(l)} labels")
        if len(l) and (l.min() < 0 or l.max() >= num_classes):
            raise ValueError(f"target {i}: labels must lie in [0, {num_classes})")
        bx.append(b); lb.append(l); off.append(off[-1] + len(b))
    gt = np.concatenate(bx, 0).astype(np.float32).reshape(-1, 4) if bx else np.zeros((0, 4), np.float32)
    lab = np.concatenate(lb).astype(np.int32) if lb else np.zeros((0,), np.int32)
    return np.ascontiguousarray(gt), np.ascontiguousarray(lab), np.asarray(off, np.int32)


class _LossAFFunction(torch.autograd.Function):
    """loss = box + obj + cls as a function of the level tensors; targets, cfg and context ride along undifferentiated"""

    @staticmethod
    def forward(fctx, ctx, cfg, gt, lab, off, *levels):
        lv = [l.detach() for l in levels]
        out4, asg, sel = ctx.loss_af_train(lv, gt, lab, off, cfg)
        fctx.save_for_backward(asg, sel, gt, lab, off, *levels)       # version counters catch an edit in between
        fctx.yl, fctx.cfg = ctx, cfg
        fctx.mark_non_differentiable(out4)
        return (out4[0] + out4[1] + out4[2]).reshape(1), out4

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, grad_loss, _grad_out4):
        asg, sel, gt, lab, off, *levels = fctx.saved_tensors
        g = grad_loss.to(dtype=torch.float32).reshape(1).contiguous()
        grads = fctx.yl.loss_af_backward(levels, gt, lab, off, fctx.cfg, asg, sel, g)
        return (None, None, None, None, None) + tuple(gr.view(l.shape) for gr, l in zip(grads, levels))


class LossAF:
    """The reference's LossAF.  `grad=False` (default): forward only.  `grad=True`: a call whose level tensors require
    grad returns a loss with a grad_fn (see the module docstring); every other call behaves as with grad=False.  `focal`,
    `gamma` and `alpha` are accepted and ignored, as the reference's forward ignores them.  `ctx`: the HipContext the
    level tensors came from (tools/evaluate.py passes the one it holds); without it a context with no layers is made
    from the shapes of the first call's tensors."""

    def __init__(self, num_classes: int, img_size: int, lambda_box: float = 5.0, lambda_obj: float = 1.0,
                 lambda_cls: float = 0.5, assign_cls_weight: float = 0.5, center_mode: str = "v8",
                 wh_mode: str = "softplus", center_radius_cells: float = 2.0, topk_limit: int = 20, focal: bool = False,
                 gamma: float = 2.0, alpha: float = 0.25, cls_smoothing: float = 0.05, area_cells_min: float = 4.0,
                 area_cells_max: float = 256.0, area_tol: float = 1.25, size_prior_w: float = 0.20,
                 ar_prior_w: float = 0.10, iou_cost_w: float = 3.0, center_cost_w: float = 0.5, ctx=None,
                 grad: bool = False):
        self.nc, self.img_size = int(num_classes), int(img_size)
        self.grad = bool(grad)
        self.topk_limit = int(topk_limit)
        if not 1 <= self.topk_limit <= _lib.YL_LOSS_MAX_TOPK:
            raise _lib.YoloLiteHipError(f"topk_limit must be 1..{_lib.YL_LOSS_MAX_TOPK} (the kernel does not truncate)")
        c = _lib.yl_loss_cfg()
        c.num_classes, c.img_size, c.topk_limit = self.nc, self.img_size, self.topk_limit
        # the reference: "v8" or anything else for the centre; "v8", "softplus" or anything else (exp) for the size
        c.center_mode = _lib.CENTER["v8"] if center_mode == "v8" else _lib.CENTER["simple"]
        c.wh_mode = _lib.WH[wh_mode] if wh_mode in ("v8", "softplus") else _lib.WH["exp"]
        c.lambda_box, c.lambda_obj, c.lambda_cls = float(lambda_box), float(lambda_obj), float(lambda_cls)
        c.assign_cls_weight, c.center_radius_cells = float(assign_cls_weight), float(center_radius_cells)
        c.cls_smoothing, c.area_tol = float(cls_smoothing), float(area_tol)
        c.area_cells_min, c.area_cells_max = float(area_cells_min), float(area_cells_max)
        c.size_prior_w, c.ar_prior_w = float(size_prior_w), float(ar_prior_w)
        c.iou_cost_w, c.center_cost_w = float(iou_cost_w), float(center_cost_w)
        self.cfg, self.ctx = c, ctx

    def _context(self, preds):
        if self.ctx is None:
            from .model import HipContext
            p0 = preds[0]
            E = int(p0.shape[-1])
            if any(p.dim() != 5 or p.shape[2] != p.shape[3] for p in preds) or E < 5 + self.nc:
                raise ValueError("preds must be level tensors [B,A,S,S,5+num_classes(+masks)]")
            dev = p0.device.index if p0.device.type == "cuda" else 0
            self.ctx = HipContext(self.img_size, self.nc, [int(p.shape[2]) for p in preds],
                                  [int(p.shape[1]) for p in preds], device=dev or 0, num_masks=E - 5 - self.nc)
        return self.ctx

    def _wants_grad(self, preds):
        return torch.is_grad_enabled() and any(torch.is_tensor(p) and p.requires_grad for p in preds)

    def _pack(self, preds, targets):
        """-> context, device tensors gt [T,4] float32, labels [T] int32, offsets [B+1] int32 (one upload per batch)"""
        for t in targets:
            if any(torch.is_tensor(v) and v.requires_grad for v in t.values()):
                raise _lib.YoloLiteHipError("LossAF is forward only (no backward pass): a target requires grad")
        if len(targets) != preds[0].shape[0]:
            raise ValueError(f"{preds[0].shape[0]} images but {len(targets)} targets")
        ctx = self._context(preds)
        gt, lab, off = pack_targets(targets, self.img_size, self.nc)
        packed = np.concatenate([gt.reshape(-1).view(np.int32), lab, off])
        d = torch.from_numpy(packed).to(ctx.device, non_blocking=True)
        T = len(lab)
        return ctx, d[:4 * T].view(torch.float32).view(T, 4), d[4 * T:5 * T], d[5 * T:]

    def _run(self, preds, targets, per=False, asg=False):
        preds = list(preds)
        if not self.grad and any(torch.is_tensor(p) and p.requires_grad for p in preds):
            raise _lib.YoloLiteHipError("LossAF is forward only (no backward pass): an input requires grad; "
                                        "call it under torch.no_grad() on detached tensors")
        ctx, gt, lab, off = self._pack(preds, targets)
        return ctx.loss_af([p.detach() for p in preds], gt, lab, off, self.cfg, want_per_image=per, want_assign=asg)

    def _run_grad(self, preds, targets):
        ctx, gt, lab, off = self._pack(preds, targets)
        # fp32 arithmetic on contiguous tensors of the context's layout; autograd carries the gradient back through
        # the cast and the copy, into the input's own dtype and strides
        lv = []
        for p, s, a in zip(preds, ctx.level_size, ctx.level_anchors):
            if tuple(p.shape) not in ((p.shape[0], a, s, s, ctx.E), (p.shape[0], s, s, ctx.E)):
                raise ValueError(f"level shape {tuple(p.shape)} != {(p.shape[0], a, s, s, ctx.E)}")
            lv.append(p.float().contiguous())
        return _LossAFFunction.apply(ctx, self.cfg, gt, lab, off, *lv)

    def __call__(self, preds, targets) -> Tuple[torch.Tensor, Dict[str, float]]:
        preds = list(preds)
        if self.grad and self._wants_grad(preds):
            loss, out4 = self._run_grad(preds, targets)
        else:
            out4, _, _ = self._run(preds, targets)
            loss = (out4[0] + out4[1] + out4[2]).reshape(1)
        h = out4.detach().cpu()
        return loss, {"box": float(h[0]), "obj": float(h[1]), "cls": float(h[2]), "pos": float(h[3])}

    forward = __call__

    def assign(self, preds, targets) -> torch.Tensor:
        """[B,N] int32: the row (over the whole batch's boxes, in order) anchor n was matched to, or -1"""
        return self._run(preds, targets, asg=True)[2]

    def per_image(self, preds, targets) -> torch.Tensor:
        """[B,3] float32: box, obj, cls of every image (the batch result is their sum in image order)"""
        return self._run(preds, targets, per=True)[1]
