#!/usr/bin/env python3
"""Time the training-time augmentation kernel (yl_augment, csrc/yl_aug.hip) beside the letterbox kernel it is the sibling
of (yl_preprocess, csrc/yl_pre.hip: the same output bytes from the same four taps, so it is the floor): batch 64 of
seeded 1280 x 720 uint8 images to 640 x 640, everything resident on the device, HIP events around blocks of launches
queued back to back.  Configurations:
  identity     plain letterbox through yl_augment
  mix          every image flipped, warped (rotate, shear, scale, translate), colour-jittered (the four modes in turn)
               and noised
  mosaic       every image a 4-image mosaic, nothing else
  mosaic_mix   both
  only_affine, only_color, only_noise   the parts of mix alone
Per configuration: the median and the minimum over the blocks, the spread (max - min) / median of the blocks, the ratio
to yl_preprocess's median and the bytes written per second.  Prints one JSON line.

    python tools/augment_time.py [--batch 64] [--img-size 640] [--src 720x1280] [--blocks 7] [--steps 20] [--out F]"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--img-size", type=int, default=640)
    ap.add_argument("--src", default="720x1280", help="source size HxW")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20, help="launches per block")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch
    import yololite_amd as ya
    from yololite_amd import _lib, augment as aug, preprocess as pre
    from yololite_amd.augment import ImageParams as P
    from yololite_amd.program import synth_state_dict, zoo_meta

    B, S = a.batch, a.img_size
    h, w = (int(v) for v in a.src.split("x"))
    dev = torch.device(a.device)
    rs = np.random.RandomState(0)
    images = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(B)]
    packed, offsets, sizes = aug.pack_images(images)
    p_dev = torch.from_numpy(packed).to(dev)
    x = torch.empty((B, 3, S, S), device=dev, dtype=torch.float32)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev)
    sp = int(stream.cuda_stream)

    def measure(launch):
        for _ in range(3):
            launch()
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(a.blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.steps):
                launch()
            e1.record(stream)
            torch.cuda.synchronize(dev)
            ms.append(e0.elapsed_time(e1) / a.steps)
        med = float(np.median(ms))
        return {"device_ms": round(med, 4), "device_ms_min": round(float(np.min(ms)), 4),
                "spread": round((max(ms) - min(ms)) / med, 4), "write_GBps": round(x.numel() * 4 / (med * 1e-3) / 1e9, 1),
                "device_ms_blocks": [round(v, 4) for v in ms]}

    # the floor: yl_preprocess with the evaluate path's normalisation (the arithmetic yl_augment ends with)
    meta = zoo_meta("edge_n", num_classes=80, img_size=S)
    model = ya.build_model_from_meta(meta)
    model.load_state_dict(synth_state_dict(meta))
    model.to(dev)
    ctx = model._ctx_for(S)
    ctx.set_option("pre_norm", 1)
    desc = np.zeros(B, pre._DESC)
    for i, (off, (ih, iw)) in enumerate(zip(offsets, sizes)):
        _, nh, nw, top, left = pre.letterbox_geometry(ih, iw, S)
        desc[i] = (off, ih, iw, nh, nw, top, left)
    d_dev = torch.from_numpy(desc.view(np.uint8).reshape(-1)).to(dev)

    def launch_pre():
        _lib.check(ctx.lib.yl_preprocess(ctx.handle, p_dev.data_ptr(), d_dev.data_ptr(), B, x.data_ptr(), sp), ctx.handle,
                   "yl_preprocess")

    result = {"tool": "augment", "gpu": torch.cuda.get_device_name(dev), "batch": B, "img_size": S, "source": [h, w],
              "steps_per_block": a.steps, "blocks": a.blocks, "output_bytes": x.numel() * 4,
              "yl_preprocess": measure(launch_pre)}
    floor = result["yl_preprocess"]["device_ms"]

    modes = ("brightness_contrast", "hsv_shift", "rgb_shift", "channel_shuffle")
    values = {"brightness_contrast": (1.2, -0.2), "hsv_shift": (5.0, -15.0, 15.0), "rgb_shift": (20.0, -20.0, 10.0),
              "channel_shuffle": ()}

    def mix(i, mosaic=None):
        m = modes[i % 4]
        return P(hflip=bool(i & 1), vflip=bool(i & 2), affine_draw=(20.0 - 40.0 * (i % 5) / 4, 10.0 - 20.0 * (i % 3) / 2,
                                                                   0.85 + 0.3 * (i % 7) / 6, 0.05 + 0.05 * (i % 2), 0.1),
                 color=(m, values[m]), perm=(2, 0, 1) if m == "channel_shuffle" else (0, 1, 2),
                 noise=(float(np.sqrt(5.0 + 15.0 * (i % 4) / 3)), 1000 + i), mosaic=mosaic)

    others = lambda i: ((i + 1) % B, (i + B // 2) % B, (i + B - 1) % B)
    configs = {"identity": [P() for _ in range(B)], "mix": [mix(i) for i in range(B)],
               "mosaic": [P(mosaic=others(i)) for i in range(B)], "mosaic_mix": [mix(i, others(i)) for i in range(B)],
               # the parts of "mix" alone: which of them carries its time
               "only_affine": [P(affine_draw=mix(i).affine_draw) for i in range(B)],
               "only_color": [P(color=mix(i).color, perm=mix(i).perm) for i in range(B)],
               "only_noise": [P(noise=mix(i).noise) for i in range(B)]}
    for name, params in configs.items():
        tiles, imgs = aug.descriptors(params, aug.compose(params, sizes, S), sizes, offsets)
        table = torch.from_numpy(np.concatenate([tiles.view(np.uint8).reshape(-1), imgs.view(np.uint8).reshape(-1)])).to(dev)
        t_ptr, i_ptr = table.data_ptr(), table.data_ptr() + tiles.nbytes

        def launch_aug():
            _lib.check(lib.yl_augment(p_dev.data_ptr(), t_ptr, i_ptr, B, S, x.data_ptr(), sp), None, "yl_augment")

        r = measure(launch_aug)
        r["ratio_to_yl_preprocess"] = round(r["device_ms"] / floor, 3)
        result["yl_augment_" + name] = r
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
