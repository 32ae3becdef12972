"""yololite-official-repo_amd -- MI355X-native (gfx950) YoloLite inference hot path.

backbone -> FPN -> heads -> anchor-free decode -> class-wise NMS as hand-written HIP kernels
behind a C ABI (include/yololite_hip.h, libyololite_hip.so); this package is the Python host
side mirroring the reference's call surface.  Importable as `yololite_amd` (see yololite_amd.py
at the repository root: the directory name contains a hyphen).
"""
from ._lib import YoloLiteHipError, load as load_library  # noqa: F401
from .model import (HipContext, YOLOLiteHIP, build_model_from_meta,  # noqa: F401
                    load_model_names_imgsize_from_ckpt)
from .postprocess import (_decode_batch_to_coco_dets, decode_anchorfree_like_train,  # noqa: F401
                          decode_preds_anchorfree, infer_main_postprocess, nms, predict_coco_dets, predict_main)
from .preprocess import letterbox_geometry, preprocess_batch  # noqa: F401
from .augment import (AugmentConfig, ImageParams, TrainAugmenter, augment_batch, compose,  # noqa: F401
                      sample_params, transform_boxes)
from .program import BACKBONES, Program, build_program  # noqa: F401
from .evalops import (_coco_eval_from_lists, build_curves_from_coco, coco_eval,  # noqa: F401
                      coco_summary_lines, create_confusion_matrix)
from .lossops import LossAF, targets_to_xyxy_px  # noqa: F401
from .trainops import FusedTrainStep  # noqa: F401
from .headops import DetectHeads  # noqa: F401
from .neckops import DetectNeck, DetectNeckMS, neck_for  # noqa: F401
from .stageops import BackboneMid, BackboneTail, MobileNetV4Backbone, UIBStack  # noqa: F401
from .stemops import BackboneStem, ConvStack  # noqa: F401
from .irops import EfficientNetLiteMid, EfficientNetLiteTail, IRStack, tail_for  # noqa: F401
from .tracker import KalmanSortTracker, TrackerBank  # noqa: F401
from .serving import ServingPipeline  # noqa: F401

__all__ = ["YoloLiteHipError", "load_library", "HipContext", "YOLOLiteHIP", "build_model_from_meta",
           "load_model_names_imgsize_from_ckpt", "decode_preds_anchorfree", "_decode_batch_to_coco_dets",
           "decode_anchorfree_like_train", "infer_main_postprocess", "nms", "predict_main", "predict_coco_dets", "build_program", "Program", "BACKBONES",
           "preprocess_batch", "letterbox_geometry", "build_curves_from_coco", "create_confusion_matrix",
           "coco_eval", "_coco_eval_from_lists", "coco_summary_lines", "LossAF", "targets_to_xyxy_px", "FusedTrainStep", "DetectHeads", "DetectNeck", "DetectNeckMS", "neck_for", "UIBStack", "BackboneTail", "BackboneMid", "MobileNetV4Backbone", "ConvStack", "BackboneStem",
           "IRStack", "EfficientNetLiteTail", "EfficientNetLiteMid", "tail_for",
           "KalmanSortTracker", "TrackerBank", "ServingPipeline",
           "AugmentConfig", "ImageParams", "TrainAugmenter", "augment_batch", "compose", "sample_params", "transform_boxes"]
