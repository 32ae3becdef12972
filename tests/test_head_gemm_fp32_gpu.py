"""The six 1x1 GEMMs of DetectHeads in precision "fp32" (yololite_amd.headops.head_gemm over yl_head_gemm,
yl_head_gemm_kernel<.., 0> of csrc/yl_block.h) at the row counts where split_plan's other bounds decide, against
torch.matmul in float64 on the CPU.

The module-level cases have few rows, so the weight gradient's split count is always the `most` bound, ceil(M / 64).
_head_cases.GEMM_OP_SHAPES holds the two shapes at which the cap of 128 splits and the unclamped 1024 / tiles decide; the
launch census (test_launch_classes_cpu.py) reads them too.  The bar is the project's rule, max(4 x e32, 2 fp32 ulps at
the tensor's maximum), e32 = the error of torch's fp32 CPU product of the same operands, as in test_head_gemm_amp_gpu.py."""
import functools

import pytest
import torch

from yololite_amd import headops
from _head_amp_cases import PASSES, SITES, cat_rows, gemm_pass, level_weights, op_operands
from _head_cases import GEMM_OP_SHAPES, bar, case_inputs
from _head_dev import heads_of
from _launch_classes import split_plan
from _train_dev import DEV

pytestmark = pytest.mark.gpu

BY_NAME = {c["name"]: c for c in GEMM_OP_SHAPES}


@functools.lru_cache(maxsize=None)
def _heads(name):
    """one module per shape with the shape's weights, shared; no test writes to it"""
    return heads_of(BY_NAME[name], case_inputs(BY_NAME[name]))


@functools.lru_cache(maxsize=None)
def _weights(name):
    return level_weights(BY_NAME[name], 0)


@pytest.mark.parametrize("name", list(BY_NAME))
def test_the_shapes_reach_the_bounds_they_are_here_for(name):
    case = BY_NAME[name]
    rows, splits, bound = case["wgrad"]
    p = headops.plan(case["F"], case["C"], case["A"], case["depth"], case["B"], case["sizes"][0])
    assert (p["wgrad_rows"], p["wgrad_splits"]) == (rows, splits), p
    assert split_plan(p["rows"], case["F"], case["F"]) == (rows, splits, bound)


@pytest.mark.parametrize("pass_", PASSES)
@pytest.mark.parametrize("site", SITES, ids=[str(s) for s in SITES])
@pytest.mark.parametrize("name", list(BY_NAME))
def test_fp32_gemm_against_the_float64_product(name, site, pass_):
    case = BY_NAME[name]
    a, b = op_operands(case, 0, site, pass_)
    w = _weights(name)
    W, bias, A = (w["Wout"] if site == "out" else w["W1"]), w["bout"], case["A"]
    d = lambda t: None if t is None else t.double()     # noqa: E731
    r64 = gemm_pass(site, pass_, d(a), d(b), d(W), d(bias), A)
    r32 = gemm_pass(site, pass_, a, b, W, bias, A)
    bound = bar(float((r32.double() - r64).abs().max()), float(r64.abs().max()))
    got = headops.head_gemm(_heads(name), 0, site, pass_, a.to(DEV), None if b is None else b.to(DEV), precision="fp32")
    if site == "out" and pass_ == "wgrad":                   # the reference's form: ONE matrix in the level's channel order
        got = cat_rows(*[g.cpu() for g in got], case["A"], case["C"]).reshape(-1, case["F"])
    got = got.cpu()
    assert got.shape == r64.shape and got.dtype == torch.float32
    err = float((got.double() - r64).abs().max())
    print(f"{name:6s} {site!s:3s} {pass_:8s} err {err:.3e}  bar {bound:.3e}  ratio {err / bound:.3f}")
    assert err <= bound, (err, bound)
