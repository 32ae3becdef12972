"""Case tables shared by test_augment_cpu.py and test_augment_gpu.py: the five source images, the ImageParams of every
case, and the references (computed once per case and size, then only read)."""
import functools
import math

import numpy as np

from yololite_amd import augment as aug
from yololite_amd.augment import ImageParams as P

from _augment_np import render32, render64

SIZES = (96, 64)                       # 96 = 1.5 blocks of 64 pixels: the x-edge guard works; 64: every source is resized
SOURCE_HW = ((96, 96), (37, 53), (195, 203), (1, 7), (120, 80))
B = len(SOURCE_HW)

# fp32 statement against float64, in gray levels (divide by 255 std for normalised units): about 3 ulp of a coordinate
# <= 256 (9e-5 px) times the steepest slope, 255 gray levels per px
BAR_GRAY = 0.025
BOUNDARY_PX = 1e-3                     # pixels nearer than this to a frame / tile boundary are not compared ...
EXCLUDED_SHARE = 0.005                 # ... and may be at most this share of an image
# HSV: render32 against render64 (colorsys) measured, at worst over HSV_CASES at both sizes, 0.0078 gray levels for the
# shift alone and 0.0202 behind mosaic + affine ("everything", image 0: the hue is ill-conditioned where max - min is
# small, so the coordinate's error reaches the output through a steeper function); 4x headroom on the larger
HSV_MEASURED_GRAY = 0.0202
BAR_HSV_GRAY = 4 * HSV_MEASURED_GRAY


@functools.lru_cache(maxsize=None)
def sources():
    rs = np.random.RandomState(11)
    return tuple(rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SOURCE_HW)


FULL_AFFINE = (20.0, 10.0, 0.85, 0.1, 0.1)
ROT = math.sqrt(20.0)


def _each(**kw):
    return [P(**kw) for _ in range(B)]


def _everything():
    return [
        P(hflip=True, vflip=True, affine_draw=FULL_AFFINE, color=("hsv_shift", (5.0, -15.0, 15.0)), noise=(ROT, 7), mosaic=(1, 2, 4)),
        P(vflip=True, affine_draw=(-20.0, -10.0, 1.15, 0.05, 0.1), color=("brightness_contrast", (1.2, -0.2)), noise=(math.sqrt(5.0), 8)),
        P(hflip=True, affine_draw=(13.0, -7.0, 0.9, 0.07, 0.06), color=("rgb_shift", (20.0, -20.0, 5.5)), noise=(3.0, 0xFFFFFFFF), mosaic=(3, 0, 1)),
        P(affine_draw=FULL_AFFINE, color=("channel_shuffle", ()), perm=(1, 2, 0), noise=(4.0, 9)),
        P(hflip=True, color=("hsv_shift", (-5.0, 15.0, -15.0)), affine_draw=(-5.0, 10.0, 1.0, 0.1, 0.05)),
    ]


CASES = {
    "identity": lambda: _each(),
    "hflip": lambda: _each(hflip=True),
    "vflip": lambda: _each(vflip=True),
    "both_flips": lambda: _each(hflip=True, vflip=True),
    "affine_full": lambda: _each(affine_draw=FULL_AFFINE),
    "affine_other_end": lambda: _each(affine_draw=(-20.0, -10.0, 1.15, 0.05, 0.05)),
    "bc_low": lambda: _each(color=("brightness_contrast", (0.8, -0.2))),
    "bc_high": lambda: _each(color=("brightness_contrast", (1.2, 0.2))),
    "hsv_low": lambda: _each(color=("hsv_shift", (-5.0, -15.0, -15.0))),
    "hsv_high": lambda: _each(color=("hsv_shift", (5.0, 15.0, 15.0))),
    "hsv_wrap": lambda: _each(color=("hsv_shift", (170.0, 0.0, 0.0))),        # 340 degrees: most hues pass 360
    "rgb_low": lambda: _each(color=("rgb_shift", (-20.0, -20.0, -20.0))),
    "rgb_high": lambda: _each(color=("rgb_shift", (20.0, 20.0, 20.0))),
    "shuffle": lambda: _each(color=("channel_shuffle", ()), perm=(2, 0, 1)),
    "noise": lambda: [P(noise=(ROT if i % 2 else math.sqrt(5.0), 100 + i)) for i in range(B)],
    "mosaic": lambda: [P(mosaic=((i + 1) % B, (i + 2) % B, (i + 3) % B)) for i in range(B)],
    "mosaic_affine": lambda: [P(mosaic=((i + 1) % B, (i + 2) % B, (i + 3) % B), affine_draw=FULL_AFFINE) for i in range(B)],
    "everything": _everything,
}
HSV_CASES = ("hsv_low", "hsv_high", "hsv_wrap", "everything")


def tables(params, S, images=None):
    """-> (packed bytes, tile table, image table, composed) exactly as augment_batch builds them"""
    packed, offsets, sizes = aug.pack_images(list(images if images is not None else sources()))
    composed = aug.compose(params, sizes, S)
    tiles, imgs = aug.descriptors(params, composed, sizes, offsets)
    return packed, tiles, imgs, composed


@functools.lru_cache(maxsize=None)
def reference32(name, S):
    packed, tiles, imgs, _ = tables(CASES[name](), S)
    out = render32(packed, tiles, imgs, S)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference64(name, S):
    params = CASES[name]()
    _, _, _, composed = tables(params, S)
    out, dist = render64(params, composed, sources(), S)
    out.setflags(write=False)
    dist.setflags(write=False)
    return out, dist
