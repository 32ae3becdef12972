"""Training-time augmentation on the device: uint8 BGR HWC images of any sizes -> warped, colour-jittered, noised,
letterboxed and normalised [B,3,S,S] fp32 RGB with one H2D copy of the packed bytes, one of the descriptors and ONE
kernel (yl_augment, csrc/yl_aug.hip); the boxes follow on the host in float64.

Stands in for what the reference runs on CPU workers through Albumentations and cv2: the dataset's 4-image mosaic
(scripts/data/dataset.py:124-175, drawn with p = 0.2 at :232-248) and get_base_transform (scripts/data/augment.py:54-101:
HorizontalFlip 0.3, VerticalFlip 0.3, Affine 0.2 (rotate +-20, shear +-10 along x, scale 0.85..1.15, translate 0.05..0.1
of the frame), OneOf 0.4 of the colour operations, GaussNoise var 5..20 with 0.15, LongestMaxSize + PadIfNeeded 114,
Normalize), with the schedule of tools/train.py:326-331.  The host draws explicit per-image values (ImageParams), folds
every geometric step into one inverse 2x3 map per image (compose) and the kernel interpolates each output pixel once.

The OneOf of the colour operations is drawn with EQUAL weights over four modes: brightness_contrast, hsv_shift,
rgb_shift, channel_shuffle (A.ColorJitter, the reference's fifth, is left out: its contrast term needs the image's
mean, a second pass over the image).

Deviations from the reference.  Neither Albumentations nor cv2 is there to pin against, and the reference's own make_*
wrappers show that their output differs between versions: this is the same family of transforms with the same
probabilities and ranges, not a bit-copy.
  * One interpolation instead of up to three (mosaic resize, affine, LongestMaxSize), and float pixels are not rounded
    to uint8 between the steps.
  * Edge-clamped sampling inside the frame; cv2 blends with the border value there.  Each mosaic tile replicates its own
    edge, tiles do not bleed into each other.
  * Noise is added at output resolution (the reference adds it before the letterbox resize), and it is the sum of twelve
    hashed uniforms, not a drawn normal.
  * ColorJitter, MotionBlur and cutmix_focus_small are absent.
  * The box filter thresholds (min_visibility, min_area) use >=.
"""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .preprocess import letterbox_geometry

COLOR_MODES = {"none": 0, "brightness_contrast": 1, "hsv_shift": 2, "rgb_shift": 3, "channel_shuffle": 4}
ONE_OF = ("brightness_contrast", "hsv_shift", "rgb_shift", "channel_shuffle")      # equal weights

TILE_DESC = np.dtype([("offset", "<i8"), ("h0", "<i4"), ("w0", "<i4"), ("x0", "<f4"), ("y0", "<f4"), ("x1", "<f4"),
                      ("y1", "<f4")])
IMAGE_DESC = np.dtype([("first_tile", "<i4"), ("num_tiles", "<i4"), ("frame_w", "<i4"), ("frame_h", "<i4"),
                       ("nh", "<i4"), ("nw", "<i4"), ("top", "<i4"), ("left", "<i4"), ("m", "<f4", (6,)),
                       ("perm", "<i4", (3,)), ("color_mode", "<i4"), ("color", "<f4", (4,)), ("noise_sigma", "<f4"),
                       ("noise_seed", "<u4")])
assert TILE_DESC.itemsize == 32 and IMAGE_DESC.itemsize == 96


@dataclass
class AugmentConfig:
    """The reference's numbers (scripts/data/augment.py:54-101, scripts/data/dataset.py:240)."""
    hflip_p: float = 0.3
    vflip_p: float = 0.3
    affine_p: float = 0.2
    rotate: Tuple[float, float] = (-20.0, 20.0)            # degrees
    shear: Tuple[float, float] = (-10.0, 10.0)             # degrees, along x only
    scale: Tuple[float, float] = (0.85, 1.15)
    translate: Tuple[float, float] = (0.05, 0.1)           # of the frame, per axis
    color_p: float = 0.4
    brightness: float = 0.2                                # beta in [-b, b]
    contrast: float = 0.2                                  # alpha in [1 - c, 1 + c]
    hue_shift: float = 5.0                                 # OpenCV hue units (2 degrees each)
    sat_shift: float = 15.0                                # of 255
    val_shift: float = 15.0                                # of 255
    rgb_shift: float = 20.0                                # Albumentations' default
    noise_p: float = 0.15
    noise_var: Tuple[float, float] = (5.0, 20.0)
    mosaic_p: float = 0.2
    min_visibility: float = 0.25
    min_area: float = 16.0

    @classmethod
    def off(cls) -> "AugmentConfig":
        return cls(hflip_p=0.0, vflip_p=0.0, affine_p=0.0, color_p=0.0, noise_p=0.0, mosaic_p=0.0,
                   min_visibility=0.0, min_area=0.0)


@dataclass
class ImageParams:
    """Explicit values of one output image; the default is the identity (plain letterbox)."""
    hflip: bool = False
    vflip: bool = False
    affine: Optional[np.ndarray] = None                    # 2x3 float64 forward matrix in frame pixels (centres at +0.5)
    # (rotate deg, shear deg, scale, tx, ty as fractions of the frame): what sample_params draws, since the frame's size is
    # only known in compose(), which makes `affine` of it (affine_matrix) when `affine` itself is None
    affine_draw: Optional[Tuple[float, float, float, float, float]] = None
    color: Tuple[str, Tuple[float, ...]] = ("none", ())
    perm: Tuple[int, int, int] = (0, 1, 2)
    noise: Tuple[float, int] = (0.0, 0)                    # (sigma in gray levels, seed)
    mosaic: Optional[Tuple[int, int, int]] = None          # the three extra source indices (quadrants 1..3)


def affine_matrix(rotate_deg: float, shear_deg: float, scale: float, tx: float, ty: float, frame_w: float,
                  frame_h: float) -> np.ndarray:
    """Forward 2x3 matrix about the frame centre: scale, shear along x, rotate, then translate by (tx fw, ty fh)."""
    th, sh = math.radians(rotate_deg), math.radians(shear_deg)
    cx, cy = frame_w / 2.0, frame_h / 2.0
    R = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    Sh = np.array([[1.0, math.tan(sh)], [0.0, 1.0]])
    L = R @ Sh * scale
    t = np.array([cx + tx * frame_w, cy + ty * frame_h]) - L @ np.array([cx, cy])
    return np.concatenate([L, t[:, None]], 1)


def sample_params(cfg: AugmentConfig, n: int, dataset_len: int, rng: np.random.Generator) -> List[ImageParams]:
    """n draws from `rng`; the same seed gives the same list.  Mosaic indices are drawn from range(dataset_len) (with
    dataset_len <= 0 no mosaic is drawn)."""
    out = []
    for _ in range(n):
        p = ImageParams()
        if dataset_len > 0 and rng.random() < cfg.mosaic_p:
            p.mosaic = tuple(int(v) for v in rng.integers(0, dataset_len, 3))
        p.hflip = bool(rng.random() < cfg.hflip_p)
        p.vflip = bool(rng.random() < cfg.vflip_p)
        if rng.random() < cfg.affine_p:
            p.affine_draw = (float(rng.uniform(*cfg.rotate)), float(rng.uniform(*cfg.shear)),
                             float(rng.uniform(*cfg.scale)), float(rng.uniform(*cfg.translate)),
                             float(rng.uniform(*cfg.translate)))
        if rng.random() < cfg.color_p:
            mode = ONE_OF[int(rng.integers(0, len(ONE_OF)))]
            if mode == "brightness_contrast":
                vals = (float(rng.uniform(1.0 - cfg.contrast, 1.0 + cfg.contrast)),
                        float(rng.uniform(-cfg.brightness, cfg.brightness)))
            elif mode == "hsv_shift":
                vals = (float(rng.uniform(-cfg.hue_shift, cfg.hue_shift)), float(rng.uniform(-cfg.sat_shift, cfg.sat_shift)),
                        float(rng.uniform(-cfg.val_shift, cfg.val_shift)))
            elif mode == "rgb_shift":
                vals = tuple(float(v) for v in rng.uniform(-cfg.rgb_shift, cfg.rgb_shift, 3))
            else:
                vals = ()
                p.perm = tuple(int(v) for v in rng.permutation(3))
            p.color = (mode, vals)
        if rng.random() < cfg.noise_p:
            p.noise = (math.sqrt(float(rng.uniform(*cfg.noise_var))), int(rng.integers(0, 2 ** 32)))
        out.append(p)
    return out


def _check_params(params: Sequence[ImageParams], nsrc: int):
    if len(params) > nsrc:
        raise ValueError(f"{len(params)} ImageParams for {nsrc} source images")
    for i, p in enumerate(params):
        if p.mosaic is not None:
            if len(p.mosaic) != 3 or any(not 0 <= int(j) < nsrc for j in p.mosaic):
                raise ValueError(f"image {i}: mosaic index out of range: {tuple(p.mosaic)} with {nsrc} source images")
        if p.color[0] not in COLOR_MODES:
            raise ValueError(f"image {i}: unknown color mode {p.color[0]!r}")
        if sorted(int(c) for c in p.perm) != [0, 1, 2]:
            raise ValueError(f"image {i}: perm {tuple(p.perm)} is not a permutation of (0, 1, 2)")


def compose(params: Sequence[ImageParams], sizes: Sequence[Tuple[int, int]], S: int) -> List[dict]:
    """sizes: (h, w) of every source image; params[i] describes output image i, whose first (or only) tile is source i and
    whose mosaic indices point into `sizes`.  -> one dict per output image, everything float64:
      tiles      [(source index, x0, y0, x1, y1)]: the rectangles of the frame
      frame      (frame_w, frame_h)
      letterbox  (scale, nh, nw, top, left) of preprocess.letterbox_geometry(frame_h, frame_w, S)
      forward    3x3: frame coordinates -> frame coordinates after the flips and the affine (what the boxes go through)
      M          2x3: output pixel INDEX -> frame coordinates (pixel centres at +0.5) = un-flip . affine^-1 . letterbox^-1"""
    if S <= 0:
        raise ValueError(f"img_size must be positive, got {S}")
    _check_params(params, len(sizes))
    out = []
    for i, p in enumerate(params):
        if p.mosaic is None:
            h, w = sizes[i]
            fw, fh = int(w), int(h)
            tiles = [(i, 0.0, 0.0, float(fw), float(fh))]
        else:
            s = float(S)                                   # scripts/data/dataset.py:128-132: (y, x) offsets (0,0) (0,s) (s,0) (s,s)
            fw = fh = 2 * S
            src = (i,) + tuple(int(j) for j in p.mosaic)
            tiles = [(src[k], ox, oy, ox + s, oy + s) for k, (oy, ox) in enumerate(((0.0, 0.0), (0.0, s), (s, 0.0), (s, s)))]
        scale, nh, nw, top, left = letterbox_geometry(fh, fw, S)
        F = np.eye(3)
        if p.hflip:
            F = np.array([[-1.0, 0, fw], [0, 1.0, 0], [0, 0, 1.0]]) @ F
        if p.vflip:
            F = np.array([[1.0, 0, 0], [0, -1.0, fh], [0, 0, 1.0]]) @ F
        A = p.affine
        if A is None and p.affine_draw is not None:
            A = affine_matrix(*p.affine_draw, fw, fh)
        A3, Ainv = np.eye(3), np.eye(3)
        if A is not None:
            A = np.asarray(A, np.float64).reshape(2, 3)
            det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
            if not np.isfinite(A).all() or det == 0.0:
                raise ValueError(f"image {i}: affine is singular or not finite")
            A3[:2] = A
            Li = np.array([[A[1, 1], -A[0, 1]], [-A[1, 0], A[0, 0]]]) / det      # exact for the exact rotations
            Ainv[:2, :2] = Li
            Ainv[:2, 2] = -(Li @ A[:, 2])
        # letterbox^-1 of the pixel index: centre x + 0.5 -> (x + 0.5 - left) * fw / nw, per axis so that the nw x nh window
        # shows exactly the frame (the resize of LongestMaxSize maps it the same way)
        sx, sy = fw / nw, fh / nh
        Linv = np.array([[sx, 0, (0.5 - left) * sx], [0, sy, (0.5 - top) * sy], [0, 0, 1.0]])
        M = (F @ Ainv @ Linv)[:2]                          # a flip is its own inverse
        out.append({"tiles": tiles, "frame": (fw, fh), "letterbox": (scale, nh, nw, top, left), "forward": A3 @ F, "M": M})
    return out


def descriptors(params: Sequence[ImageParams], composed: Sequence[dict], sizes: Sequence[Tuple[int, int]],
                offsets: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """The two tables yl_augment reads (TILE_DESC, IMAGE_DESC): float64 values rounded to fp32 once, here."""
    tiles = np.zeros(sum(len(c["tiles"]) for c in composed), TILE_DESC)
    imgs = np.zeros(len(composed), IMAGE_DESC)
    t = 0
    for i, (p, c) in enumerate(zip(params, composed)):
        d = imgs[i]
        d["first_tile"], d["num_tiles"] = t, len(c["tiles"])
        for src, x0, y0, x1, y1 in c["tiles"]:
            tiles[t] = (offsets[src], sizes[src][0], sizes[src][1], x0, y0, x1, y1)
            t += 1
        d["frame_w"], d["frame_h"] = c["frame"]
        _, d["nh"], d["nw"], d["top"], d["left"] = c["letterbox"]
        d["m"] = c["M"].reshape(6).astype(np.float32)
        d["perm"] = p.perm
        d["color_mode"] = COLOR_MODES[p.color[0]]
        vals = tuple(p.color[1])
        need = {"none": 0, "brightness_contrast": 2, "hsv_shift": 3, "rgb_shift": 3, "channel_shuffle": 0}[p.color[0]]
        if len(vals) != need:
            raise ValueError(f"image {i}: color mode {p.color[0]!r} takes {need} values, got {len(vals)}")
        d["color"] = np.asarray(vals + (0.0,) * (4 - len(vals)), np.float32)
        d["noise_sigma"] = np.float32(p.noise[0])
        d["noise_seed"] = int(p.noise[1]) & 0xFFFFFFFF
    return tiles, imgs


def _as_np(v, dtype):
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return np.asarray(v, dtype)


def transform_boxes(params: Sequence[ImageParams], boxes_xyxy_px: Sequence, labels: Sequence,
                    sizes: Sequence[Tuple[int, int]], S: int, cfg: Optional[AugmentConfig] = None) -> List[dict]:
    """boxes_xyxy_px[j] / labels[j]: the boxes of SOURCE image j in its own pixels ([n,4] xyxy, [n]).  Float64 on the host:
    per box (1) into its tile: scale by the tile's size over the source's, offset by the tile's origin, clip to the tile
    (dataset.py:149-161); (2) flips; (3) the four corners through the affine, enclosing axis-aligned box; (4) visibility =
    area clipped to the frame / area before; (5) times the letterbox scale plus (left, top); (6) kept when visibility >=
    min_visibility, output area >= min_area px^2 and both sides > 0.  -> [{"boxes": float32 [m,4] xyxy in output pixels,
    "labels": int64 [m]}] as torch tensors: the targets LossAF takes.  cfg gives the two thresholds (default: AugmentConfig())."""
    import torch
    cfg = cfg or AugmentConfig()
    out = []
    for p, c in zip(params, compose(params, sizes, S)):
        fw, fh = c["frame"]
        scale, _, _, top, left = c["letterbox"]
        keep_b, keep_l = [], []
        for src, x0, y0, x1, y1 in c["tiles"]:
            b = _as_np(boxes_xyxy_px[src], np.float64).reshape(-1, 4)
            lab = _as_np(labels[src], np.int64).reshape(-1)
            if not len(b):
                continue
            h, w = sizes[src]
            b = b * np.array([(x1 - x0) / w, (y1 - y0) / h] * 2) + np.array([x0, y0, x0, y0])
            b = np.stack([b[:, 0].clip(x0, x1), b[:, 1].clip(y0, y1), b[:, 2].clip(x0, x1), b[:, 3].clip(y0, y1)], 1)
            corners = np.stack([b[:, [0, 1]], b[:, [2, 1]], b[:, [2, 3]], b[:, [0, 3]]], 1)          # [n,4,2]
            corners = corners @ c["forward"][:2, :2].T + c["forward"][:2, 2]
            lo, hi = corners.min(1), corners.max(1)
            area = (hi[:, 0] - lo[:, 0]) * (hi[:, 1] - lo[:, 1])
            lo_c = np.stack([lo[:, 0].clip(0, fw), lo[:, 1].clip(0, fh)], 1)
            hi_c = np.stack([hi[:, 0].clip(0, fw), hi[:, 1].clip(0, fh)], 1)
            area_c = (hi_c[:, 0] - lo_c[:, 0]) * (hi_c[:, 1] - lo_c[:, 1])
            vis = np.divide(area_c, area, out=np.zeros_like(area), where=area > 0)
            o = np.concatenate([lo_c, hi_c], 1) * scale + np.array([left, top, left, top])
            ow, oh = o[:, 2] - o[:, 0], o[:, 3] - o[:, 1]
            keep = (vis >= cfg.min_visibility) & (ow * oh >= cfg.min_area) & (ow > 0) & (oh > 0)
            keep_b.append(o[keep])
            keep_l.append(lab[keep])
        bb = np.concatenate(keep_b, 0) if keep_b else np.zeros((0, 4))
        ll = np.concatenate(keep_l, 0) if keep_l else np.zeros((0,), np.int64)
        out.append({"boxes": torch.from_numpy(bb.astype(np.float32)).reshape(-1, 4),
                    "labels": torch.from_numpy(ll.astype(np.int64))})
    return out


def pack_images(images: Sequence[np.ndarray]) -> Tuple[np.ndarray, List[int], List[Tuple[int, int]]]:
    """The packing of preprocess_batch: images back to back, 16-byte aligned starts.  -> (bytes, offsets, (h, w) sizes)."""
    offsets, sizes, off = [], [], 0
    for i, im in enumerate(images):
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8:
            raise ValueError(f"image {i}: images must be uint8 arrays, got {getattr(im, 'dtype', type(im).__name__)}")
        if im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
            raise ValueError(f"image {i}: images must be HxWx3 (BGR), got shape {tuple(im.shape)}")
        offsets.append(off)
        sizes.append((int(im.shape[0]), int(im.shape[1])))
        off += (im.size + 15) & ~15
    packed = np.zeros(off, np.uint8)
    for o, im in zip(offsets, images):
        packed[o:o + im.size] = np.ascontiguousarray(im).reshape(-1)
    return packed, offsets, sizes


def augment_batch(images: Sequence[np.ndarray], targets: Optional[Sequence[dict]], params: Sequence[ImageParams],
                  img_size: int, device, extra_images: Sequence[np.ndarray] = (),
                  extra_targets: Optional[Sequence[dict]] = None, cfg: Optional[AugmentConfig] = None):
    """images: BGR uint8 HWC arrays of any sizes, one per entry of `params`; extra_images: further sources that only mosaic
    indices reach (source index len(images) + k).  targets / extra_targets: per source {"boxes": [n,4] xyxy in the
    source's pixels, "labels": [n]}, or None for no boxes.  -> (x [B,3,S,S] fp32 on `device`, targets in output pixels
    as transform_boxes returns them).  One H2D copy of the packed bytes, one of both descriptor tables, one launch on
    the current stream."""
    import torch
    from . import _lib
    S = int(img_size)
    if S <= 0:
        raise ValueError(f"img_size must be positive, got {img_size}")
    if len(params) != len(images) or not len(images):
        raise ValueError(f"{len(params)} ImageParams for {len(images)} images (need one each, at least one)")
    sources = list(images) + list(extra_images)
    packed, offsets, sizes = pack_images(sources)
    composed = compose(params, sizes, S)
    tiles, imgs = descriptors(params, composed, sizes, offsets)
    empty = {"boxes": np.zeros((0, 4)), "labels": np.zeros((0,), np.int64)}
    tg = list(targets) if targets is not None else [empty] * len(images)
    tg += list(extra_targets) if extra_targets is not None else [empty] * len(extra_images)
    if len(tg) != len(sources):
        raise ValueError(f"{len(tg)} targets for {len(sources)} source images")
    out_targets = transform_boxes(params, [t["boxes"] for t in tg], [t["labels"] for t in tg], sizes, S, cfg)

    lib = _lib.load()
    dev = torch.device(device)
    table = np.concatenate([tiles.view(np.uint8).reshape(-1), imgs.view(np.uint8).reshape(-1)])   # both 16-byte multiples
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        p_dev = torch.from_numpy(packed).to(dev, non_blocking=False)
        d_dev = torch.from_numpy(table).to(dev)
        x = torch.empty((len(images), 3, S, S), device=dev, dtype=torch.float32)
        _lib.check(lib.yl_augment(p_dev.data_ptr(), d_dev.data_ptr(), d_dev.data_ptr() + tiles.nbytes, len(images), S,
                                  x.data_ptr(), int(stream.cuda_stream)), None, "yl_augment")
        x.record_stream(stream)
        stream.synchronize()                               # p_dev / d_dev may be freed after return
    return x, out_targets


class TrainAugmenter:
    """sample_params + augment_batch with one seeded generator.  epoch_schedule follows tools/train.py:326-331: the
    mosaic is off from epoch int(0.7 epochs) on, everything (the box filter's thresholds included: get_val_transform has
    none) after epoch int(0.9 epochs)."""

    def __init__(self, cfg: Optional[AugmentConfig] = None, img_size: int = 640, seed: int = 0, device="cuda:0"):
        if img_size <= 0:
            raise ValueError(f"img_size must be positive, got {img_size}")
        self.base = cfg or AugmentConfig()
        self.cfg = self.base
        self.img_size = int(img_size)
        self.device = device
        self.rng = np.random.default_rng(seed)

    def epoch_schedule(self, epoch: int, epochs: int) -> AugmentConfig:
        if epoch > int(epochs * 0.9):
            self.cfg = AugmentConfig.off()
        elif epoch >= int(epochs * 0.7):
            self.cfg = dataclasses.replace(self.base, mosaic_p=0.0)
        else:
            self.cfg = self.base
        return self.cfg

    def __call__(self, images: Sequence[np.ndarray], targets: Optional[Sequence[dict]], dataset_len: int = 0, fetch=None):
        """fetch(j) -> (image, target) loads dataset item j for a mosaic; without it (or with dataset_len 0) no mosaic is
        drawn.  -> (x, targets) of augment_batch."""
        params = sample_params(self.cfg, len(images), dataset_len if fetch is not None else 0, self.rng)
        extra_images, extra_targets = [], []
        for p in params:
            if p.mosaic is not None:
                idx = []
                for j in p.mosaic:
                    im, tg = fetch(j)
                    idx.append(len(images) + len(extra_images))
                    extra_images.append(im)
                    extra_targets.append(tg)
                p.mosaic = tuple(idx)
        return augment_batch(images, targets, params, self.img_size, self.device, extra_images, extra_targets, self.cfg)
