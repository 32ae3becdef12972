"""The depthwise k x k passes of the backbone stage on their own (yololite_amd.stageops.depthwise -> yl_stage_depthwise,
csrc/yl_stage.hip) against torch's CPU convolution in float64.

Every cell of k in {3, 5} x stride in {1, 2} x {forward, dgrad, wgrad} x S in {1, 2, 5, 8, 9} x C in {4, 20} x B in {1, 3},
plus B 3 / S 10 (300 rows under stride 1: two tiles of the weight gradient's partials) and the shapes of
_stage_cases.DW_OP_WIDE (C 260 and 512: a second channel group of the weight gradient, one quad of it and all of it
switched on; B 2 / S 32 and B 3 / S 20: several row tiles under either stride, the last full and ragged), is held to
max(4 x e32, 2 fp32 ulps of the tensor's largest magnitude), e32 the error of torch's own fp32 CPU convolution on the
same fp32-valued inputs."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from yololite_amd import stageops
from _head_cases import bar
from _stage_cases import DW_OP_KS, DW_OP_SHAPES, DW_OP_WIDE
from _train_dev import DEV

pytestmark = pytest.mark.gpu

KS = DW_OP_KS
SHAPES = DW_OP_SHAPES + DW_OP_WIDE                         # data of _stage_cases.py: the launch census reads them too
PASSES = ("forward", "dgrad", "wgrad")


@functools.lru_cache(maxsize=None)
def cell(k, s, B, S, C):
    """inputs (fp32, NHWC) and torch's CPU results in float64 and fp32: computed once, shared, never written to"""
    rs = np.random.RandomState(1000 * k + 100 * s + 10 * S + C + B)
    So = (S + 2 * ((k - 1) // 2) - k) // s + 1
    x = rs.standard_normal((B, S, S, C)).astype(np.float32)
    w = (rs.standard_normal((C, 1, k, k)) / k).astype(np.float32)
    dy = rs.standard_normal((B, So, So, C)).astype(np.float32)
    res = {}
    for dt in (torch.float64, torch.float32):
        xt = torch.from_numpy(x).to(dt).permute(0, 3, 1, 2).requires_grad_(True)
        wt = torch.from_numpy(w).to(dt).requires_grad_(True)
        y = TF.conv2d(xt, wt, None, s, (k - 1) // 2, 1, C)
        y.backward(torch.from_numpy(dy).to(dt).permute(0, 3, 1, 2))
        res[dt] = {"forward": y.detach().permute(0, 2, 3, 1).contiguous().numpy(),
                   "dgrad": xt.grad.permute(0, 2, 3, 1).contiguous().numpy(), "wgrad": wt.grad.numpy()}
    return x, w, dy, res[torch.float64], res[torch.float32]


def device_pass(pass_, k, s, x, w, dy):
    t = lambda a: torch.from_numpy(a).to(DEV)              # noqa: E731
    if pass_ == "forward":
        return stageops.depthwise(t(x), t(w), "forward", k, s)
    if pass_ == "dgrad":
        return stageops.depthwise(t(dy), t(w), "dgrad", k, s, size=x.shape[1])
    return stageops.depthwise(t(x), t(dy), "wgrad", k, s)


@pytest.mark.parametrize("pass_", PASSES)
@pytest.mark.parametrize("k,s", KS)
def test_every_cell_against_the_float64_convolution(k, s, pass_):
    bad = []
    for B, S, C in SHAPES:
        x, w, dy, r64, r32 = cell(k, s, B, S, C)
        got = device_pass(pass_, k, s, x, w, dy).cpu().numpy()
        assert got.shape == r64[pass_].shape
        err = np.abs(got.astype(np.float64) - r64[pass_]).max()
        b = bar(np.abs(r32[pass_].astype(np.float64) - r64[pass_]).max(), np.abs(r64[pass_]).max())
        print(f"k{k} s{s} {pass_:7s} B{B} S{S:2d} C{C:3d}  err {err:.3e}  bar {b:.3e}")
        if not err <= b:
            bad.append((B, S, C, err, b))
    assert not bad, bad


@pytest.mark.parametrize("k,s", KS)
def test_a_one_hot_centre_tap_reproduces_x_bit_for_bit(k, s):
    """any slip of the padding or of an offset moves or drops a value"""
    for B, S, C in ((1, 1, 4), (3, 5, 20), (1, 8, 4), (3, 9, 4), (1, 2, 20)):
        x = torch.from_numpy(cell(k, s, B, S, C)[0]).to(DEV)
        w = torch.zeros(C, 1, k, k, device=DEV)
        w[:, 0, k // 2, k // 2] = 1.0
        y = stageops.depthwise(x, w, "forward", k, s)
        assert torch.equal(y, x[:, ::s, ::s].contiguous()), (B, S, C)
        # and the transposed pass puts dy back where it came from, zeros elsewhere
        dx = stageops.depthwise(y, w, "dgrad", k, s, size=S)
        want = torch.zeros_like(x)
        want[:, ::s, ::s] = x[:, ::s, ::s]
        assert torch.equal(dx, want), (B, S, C)


@pytest.mark.parametrize("pass_", PASSES)
def test_two_calls_give_equal_bits(pass_):
    for k, s in KS:
        for B, S, C in ((3, 9, 20), (3, 10, 20)):
            x, w, dy, _, _ = cell(k, s, B, S, C)
            assert torch.equal(device_pass(pass_, k, s, x, w, dy), device_pass(pass_, k, s, x, w, dy))


@pytest.mark.parametrize("k,s", KS)
def test_image_0_does_not_change_by_a_bit_when_image_1_does(k, s):
    x, w, dy, _, _ = cell(k, s, 3, 9, 20)
    x2, dy2 = x.copy(), dy.copy()
    x2[1:] = x2[1:] * 3 + 1
    dy2[1:] = dy2[1:] * 3 + 1
    for pass_ in ("forward", "dgrad"):
        a, b = device_pass(pass_, k, s, x, w, dy), device_pass(pass_, k, s, x2, w, dy2)
        assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])


@pytest.mark.parametrize("k,s", KS)
def test_weights_four_bytes_past_a_16_byte_boundary_give_the_bits_of_aligned_ones(k, s):
    x, w, dy, _, _ = cell(k, s, 3, 9, 20)
    wd = torch.from_numpy(w).to(DEV)
    buf = torch.zeros(w.size + 1, device=DEV)
    assert buf.data_ptr() % 16 == 0
    off = buf[1:].view(w.shape)
    off.copy_(wd)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    xd, dyd = torch.from_numpy(x).to(DEV), torch.from_numpy(dy).to(DEV)
    assert torch.equal(stageops.depthwise(xd, off, "forward", k, s), stageops.depthwise(xd, wd, "forward", k, s))
    assert torch.equal(stageops.depthwise(dyd, off, "dgrad", k, s, size=9), stageops.depthwise(dyd, wd, "dgrad", k, s, size=9))
