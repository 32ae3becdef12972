"""Training-time augmentation on the device (yl_augment, csrc/yl_aug.hip, through yololite_amd.augment): bit equality
with the numpy float32 restatement on every case of the shared table, anchors that do not rest on that restatement
(the evaluate path's oracle, torch.flip, torch.rot90, channel indexing), independence of batch, slot and stream, and
one training step behind TrainAugmenter."""
import numpy as np
import pytest
import torch

import yololite_amd as ya
from yololite_amd.augment import AugmentConfig, ImageParams as P

import _augment_cases as C
from _augment_np import MEAN, STD
from _train_dev import DEV, edge_n as _edge_n
from oracle.preproc import preprocess_albumentations

pytestmark = pytest.mark.gpu

CASE_IDS = [(n, S) for n in C.CASES for S in C.SIZES]
GRAY = (255.0 * STD.astype(np.float64))[:, None, None]    # normalised units -> gray levels


def _run(params, S, images=None, extra=()):
    x, _ = ya.augment_batch(list(images if images is not None else C.sources()), None, params, S, DEV, extra_images=extra)
    assert x.dtype == torch.float32 and tuple(x.shape) == (len(params), 3, S, S) and x.device == torch.device(DEV)
    return x


@pytest.mark.parametrize("name,S", CASE_IDS, ids=[f"{n}-{S}" for n, S in CASE_IDS])
def test_kernel_equals_the_float32_restatement_bit_for_bit(name, S):
    np.testing.assert_array_equal(_run(C.CASES[name](), S).cpu().numpy(), C.reference32(name, S))


def test_identity_is_the_evaluate_paths_preprocessing():
    """no resize (96 x 96 at S = 96): bit-equal to oracle.preproc.preprocess_albumentations.  Resized sources: within 1.5
    gray levels of it, which is the fixed-point rounding of the letterbox kernel (11-bit coefficients, two truncating
    shifts) plus its final rounding to uint8; this kernel keeps the float"""
    for S in C.SIZES:
        got = _run(C.CASES["identity"](), S).cpu().numpy()
        for b, im in enumerate(C.sources()):
            want = preprocess_albumentations(im, S)[0]
            if im.shape[:2] == (S, S):
                np.testing.assert_array_equal(got[b], want)
            d = (np.abs(got[b].astype(np.float64) - want) * GRAY).max()
            print(f"S={S} source {im.shape[:2]}: {d:.4f} gray levels from the evaluate path")
            assert d <= 1.5, (S, b, d)
    assert C.sources()[0].shape[:2] == (96, 96)            # the bit-equal branch did run


def test_flips_rotation_and_shuffle_against_torch():
    src = [C.sources()[0]]                                 # square, no resize at S = 96: every map below is exact
    ident = _run([P()], 96, src)[0]
    assert torch.equal(_run([P(hflip=True)], 96, src)[0], torch.flip(ident, dims=[2]))
    assert torch.equal(_run([P(vflip=True)], 96, src)[0], torch.flip(ident, dims=[1]))
    assert torch.equal(_run([P(hflip=True, vflip=True)], 96, src)[0], torch.flip(ident, dims=[1, 2]))
    # forward (x, y) -> (96 - y, x) turns the picture clockwise on the screen (y points down): torch.rot90 with k = -1
    cw = P(affine=np.array([[0.0, -1.0, 96.0], [1.0, 0.0, 0.0]]))
    ccw = P(affine=np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 96.0]]))
    assert torch.equal(_run([cw], 96, src)[0], torch.rot90(ident, -1, dims=(1, 2)))
    assert torch.equal(_run([ccw], 96, src)[0], torch.rot90(ident, 1, dims=(1, 2)))
    # channel shuffle: channel c shows RGB channel perm[c] of the de-normalised identity output
    mean = torch.tensor(MEAN, dtype=torch.float64, device=DEV)[:, None, None] * 255.0
    std = torch.tensor(STD, dtype=torch.float64, device=DEV)[:, None, None] * 255.0
    for S in C.SIZES:
        raw = _run(C.CASES["identity"](), S).double() * std + mean
        for perm in ((2, 0, 1), (1, 0, 2)):
            got = _run([P(color=("channel_shuffle", ()), perm=perm) for _ in range(C.B)], S).double() * std + mean
            assert (got - raw[:, list(perm)]).abs().max().item() <= 1e-4


def _independent_case(order):
    """the images of `order`, each with the values it has in every arrangement; mosaics reach the five sources as extras"""
    src = C.sources()
    n = len(order)
    per_image = C.CASES["everything"]()
    per_image[3].mosaic = (2, 4, 0)                        # overwritten below; marks a second mosaic image
    params = []
    for i in order:
        p = per_image[i]
        q = P(hflip=p.hflip, vflip=p.vflip, affine_draw=p.affine_draw, color=p.color, perm=p.perm, noise=p.noise)
        if p.mosaic is not None:
            q.mosaic = tuple(n + (i + k) % C.B for k in (1, 2, 3))
        params.append(q)
    return [src[i] for i in order], params, list(src)


@pytest.mark.parametrize("S", C.SIZES)
def test_an_image_does_not_depend_on_batch_slot_or_stream(S):
    alone = []
    for i in range(C.B):
        images, params, extra = _independent_case([i])
        alone.append(_run(params, S, images, extra)[0])
    for order in ([0, 1, 2, 3, 4], [4, 2, 0, 3, 1], [3, 3, 1]):
        images, params, extra = _independent_case(order)
        got = _run(params, S, images, extra)
        side = torch.cuda.Stream(DEV)
        with torch.cuda.stream(side):
            other = _run(params, S, images, extra)
        side.synchronize()
        for slot, i in enumerate(order):
            assert torch.equal(got[slot], alone[i]), (order, slot)
            assert torch.equal(other[slot], alone[i]), (order, slot, "side stream")


def test_train_augmenter_feeds_a_training_step():
    """TrainAugmenter -> MobileNetV4Backbone -> DetectNeck -> DetectHeads -> LossAF(grad=True) at S = 64: the loss is
    finite and backward() fills every gradient; the same seed gives the same batch"""
    meta, sd, _, _ = _edge_n()
    rs = np.random.RandomState(2)
    data = []
    for h, w in ((48, 64), (64, 40), (33, 57), (64, 64), (20, 90), (70, 70)):
        im = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        boxes = np.array([[0.1 * w, 0.1 * h, 0.6 * w, 0.7 * h], [0.4 * w, 0.3 * h, 0.95 * w, 0.9 * h]])
        data.append((im, {"boxes": boxes, "labels": np.array([len(data) % 3, 2])}))
    cfg = AugmentConfig(hflip_p=0.5, vflip_p=0.5, affine_p=0.5, color_p=0.8, noise_p=0.5, mosaic_p=0.5)

    def batch(seed):
        t = ya.TrainAugmenter(cfg, 64, seed=seed, device=DEV)
        assert t.epoch_schedule(0, 10) == cfg
        return t([d[0] for d in data[:4]], [d[1] for d in data[:4]], dataset_len=len(data), fetch=lambda j: data[j])

    x, targets = batch(5)
    x2, targets2 = batch(5)
    assert torch.equal(x, x2) and all(torch.equal(a["boxes"], b["boxes"]) for a, b in zip(targets, targets2))
    assert not torch.equal(x, batch(6)[0])
    assert tuple(x.shape) == (4, 3, 64, 64) and torch.isfinite(x).all()
    assert len(targets) == 4 and sum(len(t["boxes"]) for t in targets) > 0
    for t in targets:
        assert t["boxes"].dtype == torch.float32 and t["labels"].dtype == torch.int64 and len(t["boxes"]) == len(t["labels"])
        assert (t["boxes"] >= 0).all() and (t["boxes"] <= 64).all()

    bb = ya.MobileNetV4Backbone.from_state_dict(meta, sd).to(DEV).train()
    neck = ya.DetectNeck.from_state_dict(meta, sd).to(DEV).train()
    heads = ya.DetectHeads.from_state_dict(meta, sd).to(DEV).train()
    crit = ya.LossAF(3, 64, grad=True)
    loss = crit(heads(neck(bb(x), layout="nhwc"), layout="nhwc"), targets)[0]
    assert torch.isfinite(loss).all()
    loss.backward()
    for mod in (bb, neck, heads):
        missing = [n for n, p in mod.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
        assert not missing, missing
