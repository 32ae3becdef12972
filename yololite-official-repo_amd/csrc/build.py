#!/usr/bin/env python3
"""Build libyololite_hip.so (gfx950) in-tree with hipcc.  No cmake, no torch extension machinery:
twenty translation units (one of them, yl_program.cpp, plain host C++; three of them compiled four times: fp32, bf16-MFMA, fp16-MFMA and fp16-storage builds), one shared
library with a plain C ABI (include/yololite_hip.h).

    python yololite-official-repo_amd/csrc/build.py [--force | --asan]
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "libyololite_hip.so")
OBJ = os.path.join(HERE, "_obj")
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-value"]
UNITS = [   # (source, extra flags, object name)
    ("yl_api.hip", [], "yl_api.o"),
    # host side of the layer program (validation, weight packing, derived tables): no HIP header, no device code
    ("yl_program.cpp", [], "yl_program.o"),
    ("yl_conv.hip", [], "yl_conv.o"),
    ("yl_stemblock.hip", [], "yl_stemblock.o"),
    ("yl_convc.hip", [], "yl_convc.o"),
    ("yl_dpp.hip", [], "yl_dpp.o"),
    ("yl_se.hip", [], "yl_se.o"),
    # element-wise / reduction ops of the hgnetv2 / convnextv2 backbones: one rounding per operation (LayerNorm, GRN)
    ("yl_ops.hip", ["-ffp-contract=off"], "yl_ops.o"),
    ("yl_convc.hip", ["-DYL_BF16=1"], "yl_convc_bf16.o"),
    # bf16-MFMA inference mode: the same two units compiled again under distinct symbol names (yl_dev.h)
    ("yl_conv.hip", ["-DYL_BF16=1"], "yl_conv_bf16.o"),
    ("yl_stemblock.hip", ["-DYL_BF16=1"], "yl_stemblock_bf16.o"),
    # fp16-MFMA inference mode (the reference's fp16 autocast, scripts/helpers/evaluate.py:399,415): a third compilation
    ("yl_convc.hip", ["-DYL_BF16=1", "-DYL_F16=1"], "yl_convc_f16.o"),
    ("yl_conv.hip", ["-DYL_BF16=1", "-DYL_F16=1"], "yl_conv_f16.o"),
    ("yl_stemblock.hip", ["-DYL_BF16=1", "-DYL_F16=1"], "yl_stemblock_f16.o"),
    # fp16-STORAGE mode (option "store_f16", round 6): fp16 operands and fp16 activation tensors in HBM -- a fourth compilation
    ("yl_convc.hip", ["-DYL_BF16=1", "-DYL_F16=1", "-DYL_F16S=1"], "yl_convc_f16s.o"),
    ("yl_conv.hip", ["-DYL_BF16=1", "-DYL_F16=1", "-DYL_F16S=1"], "yl_conv_f16s.o"),
    ("yl_stemblock.hip", ["-DYL_BF16=1", "-DYL_F16=1", "-DYL_F16S=1"], "yl_stemblock_f16s.o"),
    # reference-exact fp32 arithmetic in decode/NMS: no fused multiply-add contraction
    ("yl_post.hip", ["-ffp-contract=off"], "yl_post.o"),
    ("yl_pre.hip", ["-ffp-contract=off"], "yl_pre.o"),
    # training-time augmentation (warp, colour, noise, mosaic): IEEE-exact fp32 held bit for bit to a numpy restatement
    ("yl_aug.hip", ["-ffp-contract=off"], "yl_aug.o"),
    # evaluation consumers: python-float / numpy-float32 exact IoU arithmetic
    ("yl_eval.hip", ["-ffp-contract=off"], "yl_eval.o"),
    # tracker: float32 scalar arithmetic of the reference's bbox conversions / IoU, op by op
    ("yl_track.hip", ["-ffp-contract=off"], "yl_track.o"),
    # validation loss (LossAF forward): torch's fp32 operations one by one, so the discrete assignment falls the same way
    ("yl_loss.hip", ["-ffp-contract=off"], "yl_loss.o"),
    # training step tail (unscale, clip, optimizer, EMA): every product and sum rounded where it is written
    ("yl_train.hip", ["-ffp-contract=off"], "yl_train.o"),
    # trainable detection heads (forward and backward): one rounding per written operation outside the MFMAs
    ("yl_head.hip", ["-ffp-contract=off"], "yl_head.o"),
    # trainable FPN neck: the heads' block (yl_block.h), the laterals and the top-down chain, forward and backward
    ("yl_neck.hip", ["-ffp-contract=off"], "yl_neck.o"),
    # trainable dense FPN neck (YOLOLiteMS): dense 3x3 convolution with all three passes, BatchNorm + SiLU; the chain is yl_fpn.h
    ("yl_dneck.hip", ["-ffp-contract=off"], "yl_dneck.o"),
    # trainable backbone stage (MobileNetV4 UIB blocks): depthwise k x k with stride in three passes and the residual's add;
    # the 1x1 convolutions are the heads' GEMM (yl_block.h).  The walk over its conv + BatchNorm units, forward and backward,
    # is yl_units.h, shared with yl_stem.hip; BatchNorm is yl_bn.h, the bottom header of all five training units
    ("yl_stage.hip", ["-ffp-contract=off"], "yl_stage.o"),
    # trainable dense stem (image -> C3): dense 3x3 convolution with stride in three passes on fp32 (or fp16 / bf16) MFMA, strided 1x1 units on
    # the heads' GEMM; the unit walk is yl_units.h (the one yl_stage.hip runs) and BatchNorm + ReLU is yl_bn.h
    ("yl_stem.hip", ["-ffp-contract=off"], "yl_stem.o"),
]
DEPS = ["yl_internal.h", "yl_shapes.h", "yl_program.h", "yl_dev.h", "yl_lp.h", "yl_epi.h", "yl_decode.h", "yl_block.h", "yl_bn.h", "yl_units.h", "yl_fpn.h", os.path.join("..", "..", "include", "yololite_hip.h")]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.sep not in c or os.path.exists(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stale(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def build_asan(verbose=True):
    """AddressSanitizer build of the HOST side: libyololite_hip_asan.so next to the normal library --
    every translation unit compiled with -fsanitize=address on the host pass only (-fno-gpu-sanitize: the gfx950 code
    objects are the production ones).  Run the host-logic / symbol tests under it with
        LD_PRELOAD=$(/opt/rocm/lib/llvm/bin/clang -print-file-name=libclang_rt.asan-x86_64.so) \
        ASAN_OPTIONS=detect_leaks=0 YOLOLITE_HIP_LIB=.../libyololite_hip_asan.so python -m pytest tests -m "not gpu"
    (round 3: 11 host tests clean).  Meant for the host logic on a CPU box: with the HIP runtime live under the ASAN
    interceptors the -m gpu suite crawls (4 tests in 20 minutes on the MI355X box) -- do not spend GPU time on it.
    Delete the library afterwards (28 MB; it would travel with every gpurun snapshot)."""
    hipcc = _hipcc()
    obj = os.path.join(HERE, "_obj_asan")
    os.makedirs(obj, exist_ok=True)
    out = os.path.join(os.path.dirname(HERE), "libyololite_hip_asan.so")
    san = ["-fsanitize=address", "-fno-gpu-sanitize", "-shared-libsan", "-fno-omit-frame-pointer", "-g"]
    cmds = [[hipcc] + COMMON + extra + san + ["-c", os.path.join(HERE, src), "-o", os.path.join(obj, oname)]
            for src, extra, oname in UNITS]

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    with ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(run, cmds))
    run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-fsanitize=address", "-fno-gpu-sanitize", "-shared-libsan",
         "-o", out] + [os.path.join(obj, oname) for _, _, oname in UNITS])
    return out


def build(force=False, verbose=True):
    os.makedirs(OBJ, exist_ok=True)
    hipcc = _hipcc()
    deps = [os.path.join(HERE, d) for d in DEPS] + [os.path.abspath(__file__)]
    jobs = []
    for src, extra, oname in UNITS:
        s = os.path.join(HERE, src)
        o = os.path.join(OBJ, oname)
        if force or _stale(o, [s] + deps):
            jobs.append([hipcc] + COMMON + extra + ["-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    with ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(run, jobs))
    objs = [os.path.join(OBJ, oname) for _, _, oname in UNITS]
    if force or jobs or _stale(OUT, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs)
    return OUT


if __name__ == "__main__":
    print(build_asan() if "--asan" in sys.argv else build(force="--force" in sys.argv))
