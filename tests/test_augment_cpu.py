"""Training-time augmentation, host side (yololite_amd.augment, csrc/yl_aug.hip's contract): the fp32 statement of the
kernel against an independent float64 one, the boxes against hand-derived cases, the random draws, the schedule, the
refusals and the C ABI.  No device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import yololite_amd as ya
from yololite_amd import _lib, augment as aug
from yololite_amd.augment import AugmentConfig, ImageParams as P

import _augment_cases as C
from _augment_np import STD, render32
from oracle.preproc import preprocess_albumentations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_IDS = [(n, S) for n in C.CASES for S in C.SIZES]


@pytest.mark.parametrize("name,S", CASE_IDS, ids=[f"{n}-{S}" for n, S in CASE_IDS])
def test_fp32_statement_stays_within_the_bar_of_the_float64_one(name, S):
    """render32 (what the kernel is held to, bit for bit) against render64 on every pixel farther than BOUNDARY_PX from a
    frame / tile boundary: BAR_GRAY gray levels (3 ulp of a coordinate <= 256 times 255 gray levels per px; a probe on
    noise images measured 0.0045, these cases at most 0.012), the HSV cases BAR_HSV_GRAY (measured 0.0202, see the case
    table); the excluded pixels are at most EXCLUDED_SHARE of an image (measured: at most 0.033 %)"""
    r64, dist = C.reference64(name, S)
    gray = np.abs(C.reference32(name, S).astype(np.float64) - r64) * (255.0 * STD.astype(np.float64))[None, :, None, None]
    ok = dist > C.BOUNDARY_PX
    bar = C.BAR_HSV_GRAY if name in C.HSV_CASES else C.BAR_GRAY
    for b in range(C.B):
        share = 1.0 - ok[b].mean()
        worst = (gray[b] * ok[b][None]).max()
        print(f"{name} S={S} image {b}: worst {worst:.5f} gray levels (bar {bar}), excluded {share:.5f}")
        assert share <= C.EXCLUDED_SHARE, (b, share)
        assert worst <= bar, (b, worst)


def test_restatement_agrees_with_the_oracle_and_with_numpy_flips_and_rotations():
    """render32 itself, tied to things it does not contain: the evaluate path's oracle where nothing is resized, numpy's
    flip and rot90 for the exact maps"""
    src = C.sources()[0]                                   # 96 x 96 at S = 96: no resize
    ident = C.reference32("identity", 96)[0]
    np.testing.assert_array_equal(ident, preprocess_albumentations(src, 96)[0])
    np.testing.assert_array_equal(C.reference32("hflip", 96)[0], ident[:, :, ::-1])
    np.testing.assert_array_equal(C.reference32("vflip", 96)[0], ident[:, ::-1, :])
    for k, A in ((-1, [[0, -1, 96], [1, 0, 0]]), (1, [[0, 1, 0], [-1, 0, 96]])):
        packed, tiles, imgs, _ = C.tables([P(affine=np.array(A, np.float64))], 96, images=[src])
        np.testing.assert_array_equal(render32(packed, tiles, imgs, 96)[0], np.rot90(ident, k, axes=(1, 2)))
    for S in C.SIZES:                                      # resized: the letterbox kernel's fixed point and uint8 rounding
        for b, im in enumerate(C.sources()):
            d = np.abs(C.reference32("identity", S)[b].astype(np.float64) - preprocess_albumentations(im, S)[0])
            assert (d * (255.0 * STD.astype(np.float64))[:, None, None]).max() <= 1.5, (S, b)


# ---- boxes ---------------------------------------------------------------------------------------------------------

def _boxes(params, boxes, sizes, S, labels=None, cfg=None):
    labels = labels if labels is not None else [np.arange(len(b)) for b in boxes]
    return aug.transform_boxes(params, boxes, labels, sizes, S, cfg)


def test_identity_boxes_are_the_letterboxed_ones():
    sizes = [(120, 80), (37, 53)]
    boxes = [np.array([[10.0, 20.0, 50.0, 100.0], [0.0, 0.0, 80.0, 120.0]]), np.array([[5.5, 6.25, 30.0, 20.0]])]
    got = _boxes([P(), P()], boxes, sizes, 96)
    for (h, w), b, g in zip(sizes, boxes, got):
        scale, _, _, top, left = ya.letterbox_geometry(h, w, 96)
        want = (b * scale + np.array([left, top, left, top])).astype(np.float32)       # tools/finetune_heads.py load_batch
        np.testing.assert_array_equal(g["boxes"].numpy(), want)
        assert g["boxes"].dtype.is_floating_point and g["boxes"].numpy().dtype == np.float32
        assert g["labels"].numpy().dtype == np.int64 and g["labels"].tolist() == list(range(len(b)))


def test_flipped_and_rotated_boxes():
    sizes, b = [(100, 200)], [np.array([[10.0, 20.0, 50.0, 60.0]])]                  # S = 200: scale 1, top 50, left 0
    off = np.array([0, 50, 0, 50], np.float32)
    np.testing.assert_array_equal(_boxes([P(hflip=True)], b, sizes, 200)[0]["boxes"].numpy(), np.float32([[150, 20, 190, 60]]) + off)
    np.testing.assert_array_equal(_boxes([P(vflip=True)], b, sizes, 200)[0]["boxes"].numpy(), np.float32([[10, 40, 50, 80]]) + off)
    np.testing.assert_array_equal(_boxes([P(hflip=True, vflip=True)], b, sizes, 200)[0]["boxes"].numpy(),
                                  np.float32([[150, 40, 190, 80]]) + off)
    # 90 degrees about the centre of a 100 x 100 frame: (x, y) -> (100 - y, x); S = 50 halves everything
    rot = P(affine=np.array([[0.0, -1.0, 100.0], [1.0, 0.0, 0.0]]))
    got = _boxes([rot], [np.array([[10.0, 20.0, 50.0, 40.0]])], [(100, 100)], 50)[0]["boxes"].numpy()
    np.testing.assert_array_equal(got, np.float32([[30, 5, 40, 25]]))
    # the flip comes first: (10, 20, 50, 40) -> (50, 20, 90, 40), then the rotation -> (60, 50, 80, 90)
    rot.hflip = True
    got = _boxes([rot], [np.array([[10.0, 20.0, 50.0, 40.0]])], [(100, 100)], 50)[0]["boxes"].numpy()
    np.testing.assert_array_equal(got, np.float32([[30, 25, 40, 45]]))


def test_visibility_and_area_thresholds():
    sizes, S = [(100, 100)], 100
    box = [np.array([[0.0, 0.0, 40.0, 40.0]])]
    shift = lambda dx: P(affine=np.array([[1.0, 0.0, dx], [0.0, 1.0, 0.0]]))
    at = lambda v: AugmentConfig(min_visibility=v)
    # a little more than three quarters out: 9.8 of 40 px remain, visibility 0.245
    assert len(_boxes([shift(-30.2)], box, sizes, S, cfg=at(0.25))[0]["boxes"]) == 0
    kept = _boxes([shift(-30.2)], box, sizes, S, cfg=at(0.24))[0]
    np.testing.assert_allclose(kept["boxes"].numpy(), [[0, 0, 9.8, 40]], rtol=0, atol=1e-5)
    assert kept["labels"].tolist() == [0]
    # exactly three quarters out: visibility 0.25 exactly, and the threshold is >=
    assert len(_boxes([shift(-30.0)], box, sizes, S, cfg=at(0.25))[0]["boxes"]) == 1
    assert len(_boxes([shift(-40.0)], box, sizes, S, cfg=at(0.0))[0]["boxes"]) == 0      # gone: no side left
    # area: 3.975 x 4 = 15.9 px^2 is dropped, 4 x 4 = 16 kept (>=)
    small = [np.array([[10.0, 10.0, 13.975, 14.0], [20.0, 20.0, 24.0, 24.0]])]
    got = _boxes([P()], small, sizes, S)[0]
    assert got["labels"].tolist() == [1]
    np.testing.assert_array_equal(got["boxes"].numpy(), np.float32([[20, 20, 24, 24]]))
    assert len(_boxes([P()], small, sizes, S, cfg=AugmentConfig(min_area=15.8))[0]["boxes"]) == 2


def test_mosaic_boxes_land_in_their_quadrants_and_empty_targets_stay_empty():
    S = 50                                                 # canvas 100 x 100 shown at scale 0.5
    sizes = [(100, 200), (50, 50), (25, 50), (10, 20)]
    boxes = [np.array([[20.0, 10.0, 120.0, 60.0]]), np.array([[0.0, 0.0, 50.0, 50.0]]), np.array([[10.0, 5.0, 30.0, 20.0]]),
             np.zeros((0, 4))]
    labels = [np.array([3]), np.array([1]), np.array([4]), np.zeros((0,), np.int64)]
    got = aug.transform_boxes([P(mosaic=(1, 2, 3))], boxes, labels, sizes, S)[0]
    want = np.float32([[5, 5, 30, 30],                     # (0,0): x * 50/200, y * 50/100
                       [50, 0, 100, 50],                   # (0,s): the top-right quadrant, whole
                       [10, 60, 30, 90]]) * np.float32(0.5)  # (s,0): bottom-left, x * 1, y * 2, + 50
    np.testing.assert_array_equal(got["boxes"].numpy(), want)
    assert got["labels"].tolist() == [3, 1, 4]
    # the fourth quadrant (s,s) and a box that leaves its tile: clipped to the tile, not bleeding into the neighbour
    boxes[3] = np.array([[10.0, 5.0, 40.0, 10.0]])
    labels[3] = np.array([7])
    got = aug.transform_boxes([P(mosaic=(1, 2, 3))], boxes, labels, sizes, S)[0]
    np.testing.assert_array_equal(got["boxes"].numpy()[3], np.float32([75, 75, 100, 100]) * np.float32(0.5))
    empty = aug.transform_boxes([P()], [np.zeros((0, 4))], [np.zeros((0,), np.int64)], [(10, 20)], 64)[0]
    assert tuple(empty["boxes"].shape) == (0, 4) and tuple(empty["labels"].shape) == (0,)
    assert empty["boxes"].numpy().dtype == np.float32 and empty["labels"].numpy().dtype == np.int64


# ---- random draws and schedule -----------------------------------------------------------------------------------

def test_sample_params_is_deterministic_by_seed():
    cfg = AugmentConfig()
    a = aug.sample_params(cfg, 200, 50, np.random.default_rng(3))
    b = aug.sample_params(cfg, 200, 50, np.random.default_rng(3))
    c = aug.sample_params(cfg, 200, 50, np.random.default_rng(4))
    assert a == b and a != c


def test_sampled_values_lie_in_their_ranges_and_probabilities_hold():
    cfg, n = AugmentConfig(), 20000
    ps = aug.sample_params(cfg, n, 37, np.random.default_rng(0))

    def near(count, p, total=n):
        sigma = math.sqrt(p * (1 - p) / total)
        assert abs(count / total - p) <= 4 * sigma, (count / total, p, sigma)

    near(sum(p.hflip for p in ps), cfg.hflip_p)
    near(sum(p.vflip for p in ps), cfg.vflip_p)
    near(sum(p.affine_draw is not None for p in ps), cfg.affine_p)
    near(sum(p.color[0] != "none" for p in ps), cfg.color_p)
    near(sum(p.noise[0] > 0 for p in ps), cfg.noise_p)
    near(sum(p.mosaic is not None for p in ps), cfg.mosaic_p)
    coloured = [p for p in ps if p.color[0] != "none"]
    for mode in aug.ONE_OF:                                # the OneOf: equal weights over four modes
        near(sum(p.color[0] == mode for p in coloured), 0.25, len(coloured))
    for p in ps:
        assert p.affine is None
        if p.affine_draw is not None:
            rot, shear, scale, tx, ty = p.affine_draw
            assert -20 <= rot <= 20 and -10 <= shear <= 10 and 0.85 <= scale <= 1.15
            assert 0.05 <= tx <= 0.1 and 0.05 <= ty <= 0.1
        mode, v = p.color
        if mode == "brightness_contrast":
            assert 0.8 <= v[0] <= 1.2 and -0.2 <= v[1] <= 0.2
        elif mode == "hsv_shift":
            assert abs(v[0]) <= 5 and abs(v[1]) <= 15 and abs(v[2]) <= 15
        elif mode == "rgb_shift":
            assert len(v) == 3 and all(abs(t) <= 20 for t in v)
        assert sorted(p.perm) == [0, 1, 2] and (mode == "channel_shuffle" or p.perm == (0, 1, 2))
        if p.noise[0] > 0:
            assert 5.0 - 1e-9 <= p.noise[0] ** 2 <= 20.0 + 1e-9 and 0 <= p.noise[1] < 2 ** 32
        if p.mosaic is not None:
            assert len(p.mosaic) == 3 and all(0 <= j < 37 for j in p.mosaic)
    assert all(p == P() for p in aug.sample_params(AugmentConfig.off(), 500, 37, np.random.default_rng(1)))
    assert all(p.mosaic is None for p in aug.sample_params(cfg, 500, 0, np.random.default_rng(1)))


def test_sampled_affine_moves_the_centre_by_the_translation_and_keeps_the_angles():
    A = aug.affine_matrix(20.0, 10.0, 0.85, 0.1, 0.05, 200, 100)
    np.testing.assert_allclose(A @ np.array([100.0, 50.0, 1.0]), [100 + 20, 50 + 5], atol=1e-12)
    ex = A[:, :2] @ np.array([1.0, 0.0])                   # the x axis: scaled and rotated, the shear leaves it alone
    np.testing.assert_allclose([np.hypot(*ex), math.degrees(math.atan2(ex[1], ex[0]))], [0.85, 20.0], atol=1e-12)
    np.testing.assert_allclose(np.linalg.det(A[:, :2]), 0.85 ** 2, atol=1e-12)


def test_schedule_switches_the_mosaic_off_at_70_percent_and_everything_after_90():
    t = ya.TrainAugmenter(AugmentConfig(), 64, seed=0)
    assert t.epoch_schedule(0, 100) == AugmentConfig() and t.epoch_schedule(69, 100).mosaic_p == 0.2
    at70 = t.epoch_schedule(70, 100)
    assert at70.mosaic_p == 0.0 and at70.hflip_p == 0.3 and at70.color_p == 0.4 and at70.min_visibility == 0.25
    assert t.epoch_schedule(90, 100) == at70               # tools/train.py:328 compares with >
    assert t.epoch_schedule(91, 100) == AugmentConfig.off() and t.cfg == AugmentConfig.off()
    assert t.epoch_schedule(6, 10).mosaic_p == 0.2 and t.epoch_schedule(7, 10).mosaic_p == 0.0
    off = AugmentConfig.off()
    assert (off.hflip_p, off.vflip_p, off.affine_p, off.color_p, off.noise_p, off.mosaic_p) == (0,) * 6


# ---- geometry, refusals, ABI -------------------------------------------------------------------------------------

def test_compose_takes_the_letterbox_from_letterbox_geometry_and_maps_centres():
    c = aug.compose([P(), P(mosaic=(0, 0, 0))], [(37, 53), (20, 10)], 96)
    assert c[0]["letterbox"] == ya.letterbox_geometry(37, 53, 96) and c[0]["frame"] == (53, 37)
    _, nh, nw, top, left = c[0]["letterbox"]
    np.testing.assert_allclose(c[0]["M"] @ np.array([left, top, 1.0]), [0.5 * 53 / nw, 0.5 * 37 / nh], atol=1e-12)
    assert c[1]["frame"] == (192, 192) and c[1]["letterbox"] == ya.letterbox_geometry(192, 192, 96)
    assert [t[1:] for t in c[1]["tiles"]] == [(0, 0, 96, 96), (96, 0, 192, 96), (0, 96, 96, 192), (96, 96, 192, 192)]
    assert c[0]["M"].dtype == np.float64


def test_refusals_name_what_is_wrong():
    im = np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(ValueError, match="uint8"):
        ya.augment_batch([im.astype(np.float32)], None, [P()], 64, "cuda:0")
    with pytest.raises(ValueError, match="HxWx3"):
        ya.augment_batch([im[:, :, 0]], None, [P()], 64, "cuda:0")
    with pytest.raises(ValueError, match="HxWx3"):
        ya.augment_batch([np.zeros((4, 5, 4), np.uint8)], None, [P()], 64, "cuda:0")
    with pytest.raises(ValueError, match="mosaic index out of range"):
        ya.augment_batch([im], None, [P(mosaic=(0, 1, 0))], 64, "cuda:0")
    with pytest.raises(ValueError, match="mosaic index out of range"):
        ya.augment_batch([im], None, [P(mosaic=(0, -1, 0))], 64, "cuda:0", extra_images=[im])
    with pytest.raises(ValueError, match="img_size"):
        ya.augment_batch([im], None, [P()], 0, "cuda:0")
    with pytest.raises(ValueError, match="img_size"):
        ya.TrainAugmenter(AugmentConfig(), -1)
    with pytest.raises(ValueError, match="singular"):
        aug.compose([P(affine=np.zeros((2, 3)))], [(4, 5)], 64)


def test_abi_declares_and_exports_yl_augment_and_it_refuses_null():
    header = open(os.path.join(ROOT, "include", "yololite_hip.h")).read()
    assert re.search(r"yl_status\s+yl_augment\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert "yl_augment" in [n for n, _, _ in _lib.SYMBOLS]
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "yl_augment") and lib.yl_abi_version() == 7
    one = ctypes.c_void_p(16)                              # never dereferenced: every call below is refused on the host
    assert lib.yl_augment(None, None, None, 1, 64, None, None) == -1
    for args in ((None, one, one, 1, 64, one), (one, None, one, 1, 64, one), (one, one, None, 1, 64, one),
                 (one, one, one, 1, 64, None), (one, one, one, 0, 64, one), (one, one, one, -3, 64, one),
                 (one, one, one, 1, 0, one), (one, one, one, 1, -64, one), (one, one, one, 65536, 64, one)):
        assert lib.yl_augment(*args, None) == -1, args
    assert aug.TILE_DESC.itemsize == 32 and aug.IMAGE_DESC.itemsize == 96
