"""The oracle (oracle/) against the golden vectors produced by the reference's own code
(tests/golden/make_fixtures.py).  CPU only."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import model as omodel
from oracle import postproc as opost

torch.set_num_threads(1)


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


# --------------------------------------------------------------------------- neck + head + layout
def _cases(golden_dir):
    with open(os.path.join(golden_dir, "neck_head_cases.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("idx", range(4))
def test_neck_head_matches_reference(golden_dir, idx):
    z = _load(golden_dir, "neck_head.npz")
    c = _cases(golden_dir)[idx]
    tag = c["tag"]
    arch = c["cls"]
    m = omodel.DetectorOracle(arch=arch, backbone="oracle_tiny", **c["kw"]).eval()
    sd = {k[len(tag) + 4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(tag + "/sd/")}
    m.load_state_dict(sd, strict=True)            # identical key set to the reference class
    x = torch.from_numpy(z[f"{tag}/x"])
    with torch.no_grad():
        outs = m(x)
        m.export_concat = True
        cat = m(x)
    assert list(z[f"{tag}/strides"]) == m.get_strides()
    assert tuple(z[f"{tag}/anchors"]) == m.get_num_anchors_per_level()
    for j, o in enumerate(outs):
        ref = z[f"{tag}/out{j}"]
        assert o.shape == ref.shape
        assert o.is_contiguous()
        np.testing.assert_allclose(o.numpy(), ref, rtol=0, atol=1e-6)
    np.testing.assert_allclose(cat.numpy(), z[f"{tag}/concat"], rtol=0, atol=1e-6)


# --------------------------------------------------------------------------- decode
def test_decode_zero_logits_known_answer(golden_dir):
    z = _load(golden_dir, "decode.npz")
    d = opost.decode_levels([torch.zeros(1, 1, s, s, 8) for s in (80, 40, 20)], 640)
    assert d["box"].shape == (1, 8400, 4)
    np.testing.assert_array_equal(d["box"][0, :3].numpy(), z["zero/box_first"])
    np.testing.assert_array_equal(d["box"][0, -3:].numpy(), z["zero/box_last"])
    # SURVEY 8(a) a8 known answer: P3 cell (0,0)
    np.testing.assert_allclose(d["box"][0, 0].numpy(), [1.2274113, 1.2274113, 6.7725887, 6.7725887], atol=1e-6)


@pytest.mark.parametrize("cm", ["v8", "simple"])
@pytest.mark.parametrize("wm", ["softplus", "v8", "exp"])
def test_decode_random_bit_exact(golden_dir, cm, wm):
    z = _load(golden_dir, "decode.npz")
    lv = [torch.from_numpy(z[f"rand/level{j}"]) for j in range(3)]
    d = opost.decode_levels(lv, 128, center_mode=cm, wh_mode=wm)
    for k in ("box", "obj", "cls"):
        np.testing.assert_array_equal(d[k].numpy(), z[f"rand/{cm}_{wm}/{k}"])


def test_decode_multi_anchor_c1(golden_dir):
    z = _load(golden_dir, "decode.npz")
    d = opost.decode_levels([torch.from_numpy(z[f"a2/level{j}"]) for j in range(2)], 96)
    for k in ("box", "obj", "cls"):
        np.testing.assert_array_equal(d[k].numpy(), z[f"a2/{k}"])


# --------------------------------------------------------------------------- pipelines
def _pipe_cases(golden_dir):
    with open(os.path.join(golden_dir, "pipelines_cases.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("idx", range(6))
def test_eval_pipeline_matches_reference(golden_dir, idx):
    z = _load(golden_dir, "pipelines.npz")
    c = _pipe_cases(golden_dir)[idx]
    lv = [torch.from_numpy(z[f"{c['tag']}/level{j}"]) for j in range(3)]
    dets, _ = opost.pipeline_eval(lv, c["img"], conf_th=c["conf"], iou_th=c["iou"], add_one=True)
    for b, dl in enumerate(dets):
        bbox = np.asarray([d["bbox"] for d in dl], np.float64).reshape(-1, 4)
        np.testing.assert_array_equal(bbox, z[f"{c['tag']}/eval/{b}/bbox"])
        np.testing.assert_array_equal(np.asarray([d["score"] for d in dl]), z[f"{c['tag']}/eval/{b}/score"])
        np.testing.assert_array_equal(np.asarray([d["category_id"] for d in dl], np.int64), z[f"{c['tag']}/eval/{b}/cat"])


@pytest.mark.parametrize("idx", range(6))
def test_fallback_pipeline_matches_reference(golden_dir, idx):
    z = _load(golden_dir, "pipelines.npz")
    c = _pipe_cases(golden_dir)[idx]
    lv = [torch.from_numpy(z[f"{c['tag']}/level{j}"]) for j in range(3)]
    out = opost.pipeline_fallback(lv, c["img"], conf_th=c["conf"], iou_th=c["iou"], topk=300)
    for b in range(c["B"]):
        rb, rs, rc = (z[f"{c['tag']}/fallback/{b}/{k}"] for k in ("boxes", "scores", "classes"))
        assert out["boxes"][b].shape == rb.shape, (c["tag"], b)
        if c["tag"] == "c3" and b == 0:
            # this image holds deliberate exact score ties; torch.argsort(descending) is not stable, so
            # compare as sets of (class, score, box) rows
            a = np.concatenate([out["classes"][b][:, None], out["scores"][b][:, None], out["boxes"][b]], 1)
            r = np.concatenate([rc[:, None], rs[:, None], rb], 1)
            assert sorted(map(tuple, a.tolist())) == sorted(map(tuple, r.tolist()))
        else:
            np.testing.assert_array_equal(out["boxes"][b], rb)
            np.testing.assert_array_equal(out["scores"][b], rs)
            np.testing.assert_array_equal(out["classes"][b], rc)


def test_nms_wrapper_cap_and_greedy(golden_dir):
    z = _load(golden_dir, "pipelines.npz")
    bx, sc = z["nms/boxes"], z["nms/scores"]
    np.testing.assert_array_equal(opost.nms(bx, sc, 0.9, 300, "torchvision"), z["nms/keep_tv_cap300_iou09"])
    np.testing.assert_array_equal(opost.nms(bx, sc, 0.5, 20, "torchvision"), z["nms/keep_tv_cap20_iou05"])
    np.testing.assert_array_equal(opost.nms(bx, sc, 0.5, 300, "fallback"), z["nms/keep_greedy_iou05"])
    np.testing.assert_array_equal(opost.nms(bx, sc, 0.3, 300, "fallback"), z["nms/keep_greedy_iou03"])


def test_tv_restatement_agrees_with_reference_greedy_on_tiefree_input(golden_dir):
    """Cross-check of the (unpinned) torchvision.ops.nms restatement: on inputs with no score ties and
    no IoU within 1e-4 of the threshold it must keep exactly what the reference's own pure-torch NMS
    (pinned above) keeps -- the two differ only by the 1e-6 in the denominator."""
    z = _load(golden_dir, "pipelines.npz")
    bx, sc = z["nms/boxes"], z["nms/scores"]
    assert np.unique(sc).size == sc.size
    for thr in (0.3, 0.5):
        np.testing.assert_array_equal(opost.nms_torchvision(bx, sc, thr), opost.nms_greedy_fallback(bx, sc, thr))


# --------------------------------------------------------------------------- whole tools/infer.py flow
@pytest.mark.parametrize("name", ["sq", "wide"])
def test_infer_main_flow(golden_dir, name):
    """Reference main() (letterbox -> normalise -> forward -> decode -> score -> per-class NMS (cap 300)
    -> back-map -> JSON) on a tiny seeded checkpoint vs. the oracle restatement of the same flow."""
    z = _load(golden_dir, "infer_main.npz")
    with open(os.path.join(golden_dir, "infer_main_meta.json")) as f:
        meta = json.load(f)
    m = omodel.build_from_meta(meta).eval()
    m.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}, strict=True)
    img0 = z[f"img_{name}"]
    S = meta["img_size"]
    h, w = img0.shape[:2]
    scale = min(S / h, S / w)
    nh, nw = int(round(h * scale)), int(round(w * scale))
    assert (nh, nw) == (h, w)                       # fixtures avoid cv2.resize interpolation
    top, left = (S - nh) // 2, (S - nw) // 2
    lb = np.full((S, S, 3), 114, np.uint8)
    lb[top:top + nh, left:left + nw] = img0
    im = lb[..., ::-1].astype(np.float32) / 255.0
    im = (im - np.array([0.485, 0.456, 0.406], np.float32)) / np.array([0.229, 0.224, 0.225], np.float32)
    x = torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1))[None])
    with torch.no_grad():
        lv = m(x)
    out = opost.pipeline_main(lv, S, conf=0.4, iou=0.5, per_class_cap=300)
    boxes = opost.backmap(out["boxes"][0], left, top, scale, w, h)
    assert boxes.shape[0] == z[f"{name}/bbox_xyxy"].shape[0] > 20
    np.testing.assert_array_equal(out["classes"][0], z[f"{name}/class_id"])
    np.testing.assert_array_equal(out["scores"][0].astype(np.float64), z[f"{name}/score"])
    np.testing.assert_array_equal(boxes.astype(np.float64), z[f"{name}/bbox_xyxy"])


# --------------------------------------------------------------------------- checksums
def test_param_count_checksum():
    """edge_n at C=3: 0.5524 M parameters (published 0.553 M, reference BENCHMARK.md:353);
    edge_m: 2.949 M (published 2.950 M, BENCHMARK.md:355)."""
    n = sum(p.numel() for p in omodel.DetectorOracle(num_classes=3, **omodel.MODEL_ZOO["edge_n"]).parameters())
    assert n == 552408
    n = sum(p.numel() for p in omodel.DetectorOracle(num_classes=3, **omodel.MODEL_ZOO["edge_m"]).parameters())
    assert abs(n - 2.950e6) < 0.002e6
    # edge_s: 2 359 736 against the published 2.359 M (BENCHMARK.md:354) -- a fifth reference-held checksum of the
    # mobilenetv4_conv_small restatement (1.0x widths) with F = int(256 * 0.75) = 192, d = round(1.8) = 2, head_depth 2
    n = sum(p.numel() for p in omodel.DetectorOracle(num_classes=3, **omodel.MODEL_ZOO["edge_s"]).parameters())
    assert n == 2359736 and abs(n - 2.359e6) < 0.001e6


def test_every_buildable_reference_yaml_has_a_zoo_entry_in_oracle_and_program():
    """/root/reference/configs/models/*.yaml and configs/v2_models/*.yaml, restated as data: the values below are those of the
    14 yaml files; every one whose backbone is restated must build in the oracle AND in the host compiler, with the same
    parameter count (the program consumes every tensor of the oracle's state_dict except num_batches_tracked)."""
    from yololite_amd.program import MODEL_ZOO as PZ, build_program, synth_state_dict, zoo_meta
    yamls = {   # name: (arch, backbone, depth_multiple, width_multiple, fpn_channels, head_depth)
        "edge_n": ("YOLOLiteMS_CPU", "mobilenetv4_conv_small_050", 0.65, 0.60, 160, 1),
        "edge_s": ("YOLOLiteMS_CPU", "mobilenetv4_conv_small", 0.90, 0.75, 256, 2),
        "edge_m": ("YOLOLiteMS_CPU", "mobilenetv4_conv_small", 0.95, 0.85, 288, 2),
        "edge_l": ("YOLOLiteMS_CPU", "mobilenetv4_conv_small", 1.05, 1.00, 320, 3),
        "edge_xl": ("YOLOLiteMS_CPU", "hgnetv2_b0", 1.0, 1.0, 256, 3),
        "yololite_n": ("YOLOLiteMS", "tf_efficientnet_lite0", 1.0, 1.0, 196, 1),
        "yololite_s": ("YOLOLiteMS", "tf_efficientnet_lite1", 1.0, 1.0, 256, 1),
        "yololite_m": ("YOLOLiteMS", "tf_efficientnet_lite2", 1.0, 1.0, 328, 2),
        "yololite_l": ("YOLOLiteMS", "tf_efficientnet_lite3", 1.0, 1.0, 512, 3),
        "yololite_xl": ("YOLOLiteMS", "tf_efficientnet_lite4", 1.5, 1.0, 512, 3),
        "yololite_n_v2": ("YOLOLiteMS", "tf_efficientnetv2_b0", 1.0, 1.0, 196, 1),
        "yololite_s_v2": ("YOLOLiteMS", "tf_efficientnetv2_b1", 1.0, 1.0, 256, 2),
        "yololite_m_v2": ("YOLOLiteMS", "tf_efficientnetv2_b2", 1.0, 1.0, 328, 2),
        "yololite_l_v2": ("YOLOLiteMS", "convnextv2_tiny", 1.0, 1.0, 512, 3),
    }
    from oracle import backbones as ob
    for name, (arch, bb, dm, wm, fpn, hd) in yamls.items():
        want = dict(arch=arch, backbone=bb, depth_multiple=dm, width_multiple=wm, fpn_channels=fpn, head_depth=hd)
        assert name in PZ, f"{name}: all 14 model yamls build since round 5"
        assert PZ[name] == want and omodel.MODEL_ZOO[name] == want, name
        meta = zoo_meta(name, 3, 256)
        sd = synth_state_dict(meta)
        prog = build_program(meta, sd)
        o = omodel.DetectorOracle(num_classes=3, **omodel.MODEL_ZOO[name])
        osd = {k: v for k, v in o.state_dict().items() if not k.endswith("num_batches_tracked")}
        unused = sorted(k for k in osd if k not in prog.used_keys and not k.startswith(("p6_", "smooth6", "head6")))
        assert not unused, (name, unused[:5])
        for k in prog.used_keys:
            assert tuple(sd[k].shape) == tuple(osd[k].shape), (name, k)


def test_param_checksums_of_the_published_models():
    """The efficientnetv2 family (configs/v2_models/*.yaml) has TWO reference-held checksums: yololite_n 8.923 M and
    yololite_m 17.916 M parameters (BENCHMARK.md:356-357, nc = 3 like dataset.yaml:7).  The restated tf_efficientnetv2_b0 /
    b2 backbones + the reference's neck / heads reproduce both within 0.05 %; the feature-extractor parts alone also
    reproduce timm's published totals (7.14 / 8.14 / 10.10 / 14.36 M for b0-b3) once the classifier-only conv_head +
    fc are added back."""
    from oracle import backbones as ob
    for name, pub in (("yololite_n_v2", 8.923e6), ("yololite_m_v2", 17.916e6)):
        n = sum(p.numel() for p in omodel.DetectorOracle(num_classes=3, **omodel.MODEL_ZOO[name]).parameters())
        assert abs(n - pub) / pub < 5e-4, (name, n)
    for name, last, feat, pub in (("tf_efficientnetv2_b0", 192, 1280, 7.14e6), ("tf_efficientnetv2_b1", 192, 1280, 8.14e6),
                                  ("tf_efficientnetv2_b2", 208, 1408, 10.10e6), ("tf_efficientnetv2_b3", 232, 1536, 14.36e6)):
        m = ob.create_model(name)
        assert m.feature_info[-1]["num_chs"] == last and [i["reduction"] for i in m.feature_info] == [2, 4, 8, 16, 32]
        n = sum(p.numel() for p in m.parameters()) + last * feat + 2 * feat + feat * 1000 + 1000
        assert abs(n - pub) / pub < 1e-3, (name, n)


def test_param_checksums_of_hgnetv2_and_convnextv2():
    """configs/models/edge_xl.yaml (hgnetv2_b0) and configs/v2_models/yololite_l.yaml (convnextv2_tiny) have no reference-held
    number; the checksum of these two restatements is timm's published classifier totals -- hgnetv2_b0 6.0 M (PaddleClas
    PP-HGNetV2-B0: 6.00 M), convnextv2_tiny 28.64 M, nano 15.62 M, atto 3.71 M -- feature extractor + the classifier-only
    parts (hgnet: 1x1 conv 1024 -> 2048 without bias + LAB + fc; convnext: LayerNorm + fc)."""
    from oracle import backbones as ob
    m = ob.create_model("hgnetv2_b0")
    assert [(f["num_chs"], f["reduction"]) for f in m.feature_info] == [(64, 4), (256, 8), (512, 16), (1024, 32)]
    n = sum(p.numel() for p in m.parameters()) + 1024 * 2048 + 2 + 2048 * 1000 + 1000
    assert abs(n - 6.00e6) / 6.00e6 < 1e-3, n
    for name, last, pub in (("convnextv2_tiny", 768, 28.64e6), ("convnextv2_nano", 640, 15.62e6), ("convnextv2_atto", 320, 3.71e6)):
        m = ob.create_model(name)
        assert m.feature_info[-1] == dict(num_chs=last, reduction=32, module="stages.3")
        n = sum(p.numel() for p in m.parameters()) + 2 * last + last * 1000 + 1000
        assert abs(n - pub) / pub < 1e-3, (name, n)


def test_published_macs_of_the_v2_models():
    """BENCHMARK.md:356-357 publishes 11.473 / 27.239 GMAC for yololite_n / yololite_m (v2).  A thop-style profiler
    matches module TYPES exactly and therefore skips timm's Conv2dSame (the strided TF-SAME convs: stem, the first
    fused-MBConv of stages 1 and 2, two strided depthwise convs); conv MACs of this build's program minus those five
    layers agree with the published figures to 0.3 % (the rest: BatchNorm / activation terms the profiler adds)."""
    from yololite_amd.program import build_program, synth_state_dict, zoo_meta
    for name, pub in (("yololite_n_v2", 11.473e9), ("yololite_m_v2", 27.239e9)):
        meta = zoo_meta(name, 3, 640)
        p = build_program(meta, synth_state_dict(meta))
        same = sum(l.macs for l in p.layers if (l.stride == 2 or l.dw_stride == 2) and l.op in (0, 1, 2))
        assert abs((p.macs - same) - pub) / pub < 3e-3, (name, p.macs, same)


def test_preproc_oracle_matches_reference_flow_on_identity_resize(golden_dir):
    """oracle/preproc.py letterbox + normalise equals the reference flow captured in the main() fixture for
    the same-size images (the only resize the cv2 stub allowed); the bilinear path itself is unpinned."""
    from oracle import preproc as opre
    z = _load(golden_dir, "infer_main.npz")
    for name in ("sq", "wide"):
        img0 = z[f"img_{name}"]
        x, (padx, pady, scale, w0, h0) = opre.preprocess(img0, 96)
        S = 96
        h, w = img0.shape[:2]
        sc = min(S / h, S / w)
        nh, nw = int(round(h * sc)), int(round(w * sc))
        top, left = (S - nh) // 2, (S - nw) // 2
        lb = np.full((S, S, 3), 114, np.uint8)
        lb[top:top + nh, left:left + nw] = img0
        im = (lb[..., ::-1].astype(np.float32) / 255.0 - opre.MEAN) / opre.STD
        np.testing.assert_array_equal(x, im.transpose(2, 0, 1))
        assert (padx, pady, scale, w0, h0) == (left, top, sc, w, h)
    # fixed-point bilinear sanity: constant images stay constant, identity resize is exact
    c = np.full((17, 29, 3), 200, np.uint8)
    assert (opre.resize_linear_u8(c, 64, 40) == 200).all()


# --------------------------------------------------------------------------- evaluate-path consumers (f3)
from oracle import evalcons as oeval   # noqa: E402


def _eval_fix(golden_dir):
    with open(os.path.join(golden_dir, "eval_consumers.json")) as f:
        return json.load(f)


from _evalcheck import assert_curves_equal   # noqa: E402


@pytest.mark.parametrize("case", ["mixed", "ties", "crowded", "no_dets"])
def test_eval_curves_oracle_matches_reference(golden_dir, case):
    fx = _eval_fix(golden_dir)[case]
    for tag, want in fx["curves"].items():
        iou, steps = tag.split("_")
        got = oeval.build_curves_from_coco(fx["images"], fx["anns"], fx["dets"], None, iou=float(iou),
                                           steps=int(steps))
        assert_curves_equal(got, want)


@pytest.mark.parametrize("case", ["mixed", "ties", "crowded", "no_dets"])
def test_eval_confusion_oracle_matches_reference(golden_dir, case):
    fx = _eval_fix(golden_dir)[case]
    for rec in fx["confusion"].values():
        cm = oeval.confusion_matrix_counts(fx["anns"], fx["dets"], fx["num_classes"], rec["iou_thresh"],
                                           rec["score_thresh"])
        assert np.array_equal(cm, np.asarray(rec["cm"]))
        st = oeval.confusion_stats(cm)
        assert f"Total FP: {st['total_fp']}\n" in rec["stats_txt"]
        assert f"Total FN: {st['total_fn']}\n" in rec["stats_txt"]


# --------------------------------------------------------------------------- Kalman-SORT tracker (f4)
from oracle import tracker as otrack   # noqa: E402
from _evalcheck import check_tracker_sequence   # noqa: E402


@pytest.mark.parametrize("case", ["default", "crowd", "anyclass", "gaps"])
def test_tracker_oracle_matches_reference(golden_dir, case):
    with open(os.path.join(golden_dir, "tracker.json")) as f:
        rec = json.load(f)[case]
    check_tracker_sequence(otrack.SortOracle, rec, box_tol=0.0)       # same numpy calls: bit-exact here
