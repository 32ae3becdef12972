#!/usr/bin/env python3
"""Fit the detection heads of a checkpoint to a label set, everything on the device and without a torch model:

    backbone + FPN frozen in the executor (YOLOLiteHIP.pyramid) -> DetectHeads (forward + backward, csrc/yl_head.hip)
    -> LossAF(grad=True) -> FusedTrainStep (clip, optimizer, EMA off)

    python tools/finetune_heads.py --weights in.pt --data DIR --out out.pt [--num-classes N] [--names a,b,c]
                                   [--epochs 10] [--batch 16] [--lr 1e-3] [--optimizer adamw] [--grad-clip 10]
                                   [--train-neck [--amp fp16|bf16] [--train-tail [--lr-tail 1e-4] [--train-mid]]] [--amp-heads fp16|bf16]
                                   [--train-neck --train-backbone [--lr-backbone 1e-4]]
                                   [--amp-backbone fp16|bf16]
                                   [--augment [--mosaic-p 0.2] [--aug-seed 0]]
    python tools/finetune_heads.py --synthetic edge_n --out out.pt [--num-classes 3] [--img-size 128] [--steps 20]
                                   [--augment [--mosaic-p 0.2] [--aug-seed 0]]

DIR is a YOLO-txt dataset: DIR/images/*.{jpg,jpeg,png,bmp} and DIR/labels/<stem>.txt with lines
`class cx cy w h` (normalised to the image).  Images are read with PIL, letterboxed by the library's preprocess path
(yl_preprocess), the boxes follow the same geometry.  No augmentation unless --augment is given (below).  With --num-classes other than the
checkpoint's the heads start freshly initialised (torch's defaults plus the reference's init_detect_bias); otherwise
they start from the checkpoint.  --synthetic NAME takes a zoo model with seeded synthetic weights and one random batch
instead of --weights / --data.  The output is a checkpoint {"state_dict", "meta"}: the input's state_dict with the
`head*.` entries replaced, meta.num_classes / names updated -- tools/infer.py runs it.

With --train-neck (models without P6) the FPN neck is trained as well: the executor stops being the pyramid's source and
gives the backbone's feature maps (YOLOLiteHIP.features); neckops.neck_for picks the neck of the model's arch --
DetectNeck (csrc/yl_neck.hip) for YOLOLiteMS_CPU, DetectNeckMS (csrc/yl_dneck.hip, dense 3x3 + SiLU) for YOLOLiteMS,
e.g. --synthetic yololite_n -- which starts from the checkpoint's `lateral*.` / `smooth*.` entries; its parameters join
the heads' in the one FusedTrainStep, and its state_dict is merged into the output as well.

--amp fp16 | bf16 (with --train-neck and a YOLOLiteMS model; the reference's AMP, tools/train.py:284-357): DetectNeckMS runs
its three 3x3 GEMMs in that precision (operands rounded, fp32 accumulation; parameters and gradients stay fp32).  With
fp16 the loss is multiplied by FusedTrainStep's loss scale before backward() and the step unscales, skips a step whose
gradients are not finite and updates the scale, all on the device; with bf16 the scale is fixed at 1.  The laterals
and the loss stay fp32.

With --train-tail (needs --train-neck; the mobilenetv4_conv_small backbones, i.e. edge_n / edge_s / edge_m / edge_l) the
backbone's last stage is trained as well: stageops.BackboneTail (csrc/yl_stage.hip) holds the UIB blocks and the 1x1
ConvBnAct between the C4 and the C5 tap, starts from the checkpoint's `backbone.blocks.*` entries, and runs
`c3, c4, _ = model.features(x); c5 = tail(c4); neck([c3, c4, c5])`; stages 0..3 stay frozen in the executor.  The tail's
parameters are a FusedTrainStep group of their own with the rate --lr-tail (default: --lr), and its state_dict is merged
into the output.  The tail is fp32; --amp / --amp-heads go with it: nothing in the code ties the precision of the
neck's or the heads' GEMMs to the tail's, and the loss scale reaches its gradients through the chain like any others.

For the EfficientNet-Lite backbones (tf_efficientnet_lite0..4: yololite_n / s / m / l / xl) --train-tail picks
irops.EfficientNetLiteTail through irops.tail_for (timm's `ir` blocks under ReLU6 and TF-SAME padding, arch stages 5 and 6),
e.g. --synthetic yololite_n --train-neck --train-tail.  --train-mid (needs --train-tail; this family only) trains the
C3 -> C4 stage as well (irops.EfficientNetLiteMid, arch stages 3 and 4): `c3 = model.features(x)[0]; c4 = mid(c3);
c5 = tail(c4)`, torch sums the two gradients that meet at C4; its parameters are a group of their own with --lr-tail.
--train-backbone is refused for this family: its stem is a dense 3x3 under TF-SAME and its stage 0 a `ds` block whose
1x1 has no activation, neither of which the trainable modules have; stages 0..2 stay frozen in the executor.

With --train-backbone (needs --train-neck, implies --train-tail; the mobilenetv4_conv_small backbones) the WHOLE backbone is trained:
stageops.MobileNetV4Backbone holds the stem (stemops.BackboneStem, csrc/yl_stem.hip: image -> C3), the C3 -> C4 stage
(stageops.BackboneMid) and the tail, starts from the checkpoint's `backbone.*` entries, and the step runs
`neck(backbone(x))`: the executor is out of the loop.  The backbone's parameters are a FusedTrainStep group of their own
with the rate --lr-backbone (default: --lr), and its state_dict is merged into the output.  The backbone is fp32.

--amp-heads fp16 | bf16 (with or without --train-neck): DetectHeads runs every 1x1 GEMM of the heads in that precision, on
the same terms.  --amp-backbone fp16 | bf16 (needs --train-backbone or --train-tail) does the same for the trainable
backbone: every dense GEMM of MobileNetV4Backbone (the stem's 3x3 and every 1x1 convolution) or of BackboneTail, on the
same terms; its depthwise convolutions and BatchNorm stay fp32.  The loss scale is on when any of --amp, --amp-heads and
--amp-backbone is fp16.

--augment: batches go through augment.TrainAugmenter (csrc/yl_aug.hip) instead of yl_preprocess: the reference's
training-time transforms (scripts/data/augment.py:54-101: flips, affine, one colour operation, noise, letterbox, normalise)
and its 4-image mosaic (scripts/data/dataset.py:124-175) with their probabilities and ranges, one kernel launch per batch,
the boxes transformed and filtered on the host; augment.py's docstring lists what differs from Albumentations / cv2.  With
--data the three extra images of a mosaic are drawn from the dataset, and the schedule of tools/train.py:326-331 holds
(mosaic off from 70 % of the epochs, everything off after 90 %).  With --synthetic the one batch is seeded random uint8
images of mixed sizes, augmented anew at every step.  --mosaic-p sets the mosaic's probability (default: the reference's
0.2), --aug-seed the generator's seed.  The images are normalised with the evaluate path's arithmetic (A.Normalize), which
is what the reference trains on.
"""
import argparse
import copy
import glob
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import yololite_amd as ya  # noqa: E402
from yololite_amd.program import synth_state_dict, zoo_meta  # noqa: E402

EXTS = (".jpg", ".jpeg", ".png", ".bmp")


def read_dataset(root):
    """-> [(image path, labels [n] int64, boxes [n,4] normalised cx cy w h)]"""
    items = []
    for p in sorted(glob.glob(os.path.join(root, "images", "*"))):
        if not p.lower().endswith(EXTS):
            continue
        lab = os.path.join(root, "labels", os.path.splitext(os.path.basename(p))[0] + ".txt")
        rows = []
        if os.path.exists(lab):
            with open(lab) as f:
                rows = [[float(v) for v in ln.split()[:5]] for ln in f if len(ln.split()) >= 5]
        a = np.asarray(rows, np.float64).reshape(-1, 5)
        items.append((p, a[:, 0].astype(np.int64), a[:, 1:5]))
    if not items:
        raise SystemExit(f"no images under {os.path.join(root, 'images')}")
    return items


def load_batch(ctx, items, img_size):
    """-> x [B,3,S,S] on the device, targets (pixel xyxy in the letterboxed image)"""
    from PIL import Image
    images, targets = [], []
    for path, labels, boxes in items:
        rgb = np.asarray(Image.open(path).convert("RGB"))
        images.append(np.ascontiguousarray(rgb[:, :, ::-1]))          # the preprocess path takes BGR, as cv2 reads it
        h, w = rgb.shape[:2]
        scale, nh, nw, top, left = ya.letterbox_geometry(h, w, img_size)
        cx, cy, bw, bh = (boxes[:, i] for i in range(4))
        xyxy = np.stack([(cx - bw / 2) * w * scale + left, (cy - bh / 2) * h * scale + top,
                         (cx + bw / 2) * w * scale + left, (cy + bh / 2) * h * scale + top], 1)
        targets.append({"boxes": torch.from_numpy(xyxy.astype(np.float32)).reshape(-1, 4),
                        "labels": torch.from_numpy(labels)})
    x, _ = ya.preprocess_batch(ctx, images, letterbox=True, norm="infer")
    return x, targets


def load_item(item):
    """-> (BGR uint8 image, {"boxes": xyxy in the image's pixels, "labels"}): what TrainAugmenter takes"""
    from PIL import Image
    path, labels, boxes = item
    rgb = np.asarray(Image.open(path).convert("RGB"))
    h, w = rgb.shape[:2]
    cx, cy, bw, bh = (boxes[:, i] for i in range(4))
    xyxy = np.stack([(cx - bw / 2) * w, (cy - bh / 2) * h, (cx + bw / 2) * w, (cy + bh / 2) * h], 1).reshape(-1, 4)
    return np.ascontiguousarray(rgb[:, :, ::-1]), {"boxes": xyxy, "labels": labels}


def synthetic_images(img_size, batch, num_classes, seed=0):
    """--synthetic --augment: seeded random uint8 images of mixed sizes with 1..3 boxes each, in source pixels"""
    rs = np.random.RandomState(seed)
    images, targets = [], []
    for _ in range(batch):
        h, w = (int(v) for v in rs.randint(img_size // 2, 2 * img_size + 1, 2))
        images.append(rs.randint(0, 256, (h, w, 3)).astype(np.uint8))
        n = int(rs.randint(1, 4))
        c = rs.uniform(0.25, 0.75, (n, 2)) * (w, h)
        wh = rs.uniform(0.15, 0.45, (n, 2)) * (w, h)
        targets.append({"boxes": np.concatenate([c - wh / 2, c + wh / 2], 1), "labels": rs.randint(0, num_classes, n).astype(np.int64)})
    return images, targets


def synthetic_batch(img_size, batch, num_classes, device, seed=0):
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.standard_normal((batch, 3, img_size, img_size)).astype(np.float32)).to(device)
    targets = []
    for _ in range(batch):
        n = int(rs.randint(1, 4))
        c = rs.uniform(0.25, 0.75, (n, 2)) * img_size
        wh = rs.uniform(0.15, 0.45, (n, 2)) * img_size
        targets.append({"boxes": torch.from_numpy(np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)),
                        "labels": torch.from_numpy(rs.randint(0, num_classes, n).astype(np.int64))})
    return x, targets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", default="")
    ap.add_argument("--data", default="")
    ap.add_argument("--synthetic", default="", help="zoo model name: synthetic weights and one random batch")
    ap.add_argument("--out", required=True)
    ap.add_argument("--num-classes", type=int, default=0)
    ap.add_argument("--names", default="")
    ap.add_argument("--img-size", type=int, default=0)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20, help="--synthetic: steps on the one batch")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--optimizer", default="adamw", choices=("adamw", "adam", "sgd"))
    ap.add_argument("--grad-clip", type=float, default=10.0)
    ap.add_argument("--train-neck", action="store_true", help="train the FPN neck (laterals, smooth blocks) as well")
    ap.add_argument("--train-tail", action="store_true",
                    help="with --train-neck: train the backbone's last stage (C4 tap -> C5 tap) as well")
    ap.add_argument("--lr-tail", type=float, default=0.0, help="learning rate of the tail's (and the mid's) parameters (default: --lr)")
    ap.add_argument("--train-mid", action="store_true",
                    help="with --train-tail, EfficientNet-Lite backbones: train the C3 tap -> C4 tap stage as well")
    ap.add_argument("--train-backbone", action="store_true",
                    help="with --train-neck: train the whole backbone (image -> C3, C4, C5); implies --train-tail")
    ap.add_argument("--lr-backbone", type=float, default=0.0, help="learning rate of the backbone's parameters (default: --lr)")
    ap.add_argument("--amp", default="", choices=("", "fp16", "bf16"),
                    help="with --train-neck, YOLOLiteMS models: the dense neck's 3x3 GEMMs in this precision")
    ap.add_argument("--amp-heads", default="", choices=("", "fp16", "bf16"),
                    help="the heads' 1x1 GEMMs in this precision (independent of --train-neck)")
    ap.add_argument("--amp-backbone", default="", choices=("", "fp16", "bf16"),
                    help="with --train-backbone or --train-tail: the backbone's dense GEMMs (3x3 stem, every 1x1) in this precision")
    ap.add_argument("--augment", action="store_true",
                    help="training-time augmentation on the device (flips, affine, colour, noise, mosaic) instead of the plain letterbox")
    ap.add_argument("--mosaic-p", type=float, default=-1.0, help="with --augment: probability of the 4-image mosaic (default 0.2)")
    ap.add_argument("--aug-seed", type=int, default=0, help="with --augment: seed of the augmentation's generator")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if (a.mosaic_p >= 0 or a.aug_seed) and not a.augment:
        raise SystemExit("--mosaic-p / --aug-seed set the augmentation: they need --augment")
    if bool(a.synthetic) == bool(a.weights):
        raise SystemExit("give either --weights (with --data) or --synthetic NAME")
    if a.amp_backbone and not (a.train_backbone or a.train_tail):
        raise SystemExit("--amp-backbone sets the precision of the trainable backbone: it needs --train-backbone or --train-tail")
    if a.amp and not a.train_neck:
        raise SystemExit("--amp sets the precision of the trainable dense neck: it needs --train-neck")
    if a.train_tail and not a.train_neck:
        raise SystemExit("--train-tail feeds the tail's C5 to the trainable neck: it needs --train-neck")
    if a.train_mid and not a.train_tail:
        raise SystemExit("--train-mid feeds the stage's C4 to the trainable tail: it needs --train-tail")
    if a.train_backbone and not a.train_neck:
        raise SystemExit("--train-backbone feeds the backbone's maps to the trainable neck: it needs --train-neck")
    if a.synthetic:
        meta = zoo_meta(a.synthetic, num_classes=a.num_classes or 3, img_size=a.img_size or 128)
        sd = synth_state_dict(meta, seed=1)
    else:
        if not a.data:
            raise SystemExit("--weights needs --data")
        ckpt = torch.load(a.weights, map_location="cpu", weights_only=False)
        meta, sd = copy.deepcopy(ckpt["meta"] or {}), dict(ckpt["state_dict"])
    img_size = int(a.img_size or meta.get("img_size", 640))
    old_nc = int(meta.get("num_classes") or meta["config"]["model"].get("num_classes") or 80)
    nc = int(a.num_classes or old_nc)

    model = ya.build_model_from_meta(meta)
    model.load_state_dict(sd)
    model.to(a.device)
    if nc == old_nc:
        heads = ya.DetectHeads.from_state_dict(meta, sd, precision=a.amp_heads or "fp32")
    else:
        heads = ya.DetectHeads.from_meta(meta, num_classes=nc, precision=a.amp_heads or "fp32")
        print(f"[finetune_heads] {old_nc} -> {nc} classes: heads freshly initialised")
    heads.to(a.device).train()
    # DetectNeck (arch YOLOLiteMS_CPU) refuses a reduced precision and says why
    neck = ya.neck_for(meta, sd, precision=a.amp or "fp32").to(a.device).train() if a.train_neck else None
    lite = ya.irops.is_lite(meta)
    if lite and a.train_backbone:
        raise SystemExit("--train-backbone is not implemented for the EfficientNet-Lite backbones: the stem is a dense 3x3 under "
                         "TF-SAME padding and stage 0 a `ds` block whose 1x1 has no activation; --train-tail [--train-mid] "
                         "trains stages 3..6")
    if a.train_mid and not lite:
        raise SystemExit("--train-mid is the EfficientNet-Lite backbones' (yololite_n .. xl); the mobilenetv4_conv_small "
                         "backbones train their C3 -> C4 stage with --train-backbone")
    # tail_for picks the tail of the backbone's family and refuses, by name, a backbone whose last stage neither has
    bprec = a.amp_backbone or "fp32"
    tail = ya.tail_for(meta, sd, precision=bprec).to(a.device).train() if a.train_tail and not a.train_backbone else None
    mid = ya.EfficientNetLiteMid.from_state_dict(meta, sd, precision=bprec).to(a.device).train() if a.train_mid else None
    # MobileNetV4Backbone (stem, C3 -> C4 stage and the tail in one) refuses the other backbone families by name as well
    backbone = ya.MobileNetV4Backbone.from_state_dict(meta, sd, precision=bprec).to(a.device).train() if a.train_backbone else None
    crit = ya.LossAF(nc, img_size, grad=True)
    params = (list(neck.parameters()) if neck is not None else []) + list(heads.parameters())
    if tail is not None:                                   # a group of its own: its rate is --lr-tail
        params = [{"params": params}, {"params": list(tail.parameters()), "lr": a.lr_tail or a.lr}]
    if mid is not None:                                    # likewise, at the tail's rate
        params.append({"params": list(mid.parameters()), "lr": a.lr_tail or a.lr})
    if backbone is not None:                               # likewise: --lr-backbone
        params = [{"params": params}, {"params": list(backbone.parameters()), "lr": a.lr_backbone or a.lr}]
    # fp16: dynamic loss scale (unscale, found-inf skip, growth / backoff in the step); bf16 has fp32's range: scale 1
    fts = ya.FusedTrainStep(params, optimizer=a.optimizer, grad_clip=a.grad_clip, amp="fp16" in (a.amp, a.amp_heads, a.amp_backbone), lr=a.lr)

    def step(x, targets):
        # frozen trunk: plain tensors, nothing to backpropagate into
        if neck is None:
            feats = model.pyramid(x)
        elif backbone is not None:                         # image -> [c3, c4, c5], every stage trainable: no executor
            feats = neck(backbone(x), layout="nhwc")
        else:
            cs = model.features(x)
            if mid is not None:                            # the executor's C4 and C5 are replaced: C4 feeds the neck and the tail
                c4 = mid(cs[-3], layout="nhwc")
                cs = cs[:-2] + [c4, tail(c4, layout="nhwc")]
            elif tail is not None:                         # the executor's C5 is replaced by the trainable tail's
                cs = cs[:-2] + [cs[-2], tail(cs[-2], layout="nhwc")]
            feats = neck(cs, layout="nhwc")
        fts.zero_grad()
        loss, parts = crit(heads(feats, layout="nhwc"), targets)
        fts.scale(loss).backward()                         # the identity unless one of the --amp options is fp16
        norm = fts.step()
        return float(loss), parts, float(norm)

    augmenter = None
    if a.augment:
        cfg = ya.AugmentConfig() if a.mosaic_p < 0 else ya.AugmentConfig(mosaic_p=a.mosaic_p)
        augmenter = ya.TrainAugmenter(cfg, img_size, seed=a.aug_seed, device=a.device)

    if a.synthetic:
        if augmenter is not None:
            images, src_targets = synthetic_images(img_size, min(a.batch, 8), nc)
        else:
            x, targets = synthetic_batch(img_size, min(a.batch, 8), nc, a.device)
        for i in range(a.steps):
            if augmenter is not None:                      # the same sources, drawn anew: mosaics take their extras from the batch
                x, targets = augmenter(images, src_targets, dataset_len=len(images), fetch=lambda j: (images[j], src_targets[j]))
            loss, parts, norm = step(x, targets)
            print(f"step {i:3d}  loss {loss:.4f}  box {parts['box']:.4f} obj {parts['obj']:.4f} cls {parts['cls']:.4f}  "
                  f"|g| {norm:.3f}")
    else:
        items = read_dataset(a.data)
        ctx = model._ctx_for(img_size)
        for ep in range(a.epochs):
            order = np.random.RandomState(ep).permutation(len(items))
            tot, n = 0.0, 0
            if augmenter is not None:
                augmenter.epoch_schedule(ep, a.epochs)
            for i in range(0, len(order), a.batch):
                if augmenter is not None:
                    loaded = [load_item(items[j]) for j in order[i:i + a.batch]]
                    x, targets = augmenter([im for im, _ in loaded], [t for _, t in loaded], dataset_len=len(items),
                                           fetch=lambda j: load_item(items[j]))
                else:
                    x, targets = load_batch(ctx, [items[j] for j in order[i:i + a.batch]], img_size)
                if x.shape[0] * (img_size // 32) ** 2 < 2:
                    continue                               # BatchNorm needs more than one value per channel
                loss, _, _ = step(x, targets)
                tot, n = tot + loss, n + 1
            print(f"epoch {ep:3d}  mean loss {tot / max(n, 1):.4f}  ({n} batches)")

    out_sd = dict(sd)
    for mod in [m for m in (backbone, mid, tail, neck) if m is not None] + [heads]:
        for k, v in mod.state_dict().items():
            out_sd[k] = v.detach().cpu()
    out_sd = {k: (torch.as_tensor(v) if not torch.is_tensor(v) else v) for k, v in out_sd.items()}
    meta = copy.deepcopy(meta)
    meta["num_classes"] = nc
    meta.setdefault("config", {}).setdefault("model", {})["num_classes"] = nc
    names = [s for s in a.names.split(",") if s]
    if names and len(names) != nc:
        raise SystemExit(f"--names has {len(names)} entries for {nc} classes")
    if names or nc != old_nc or not meta.get("names"):
        meta["names"] = names or [str(i) for i in range(nc)]
    torch.save({"state_dict": out_sd, "meta": meta}, a.out)
    print(f"[finetune_heads] wrote {a.out}")


if __name__ == "__main__":
    main()
