"""The dense convolution passes of the trainable stem on their own (yololite_amd.stemops.conv -> yl_stem_conv,
csrc/yl_stem.hip) against torch's CPU conv2d in float64.

Every cell of k in {1, 3} x stride in {1, 2} x {forward, dgrad, wgrad} x S in {1, 2, 5, 8, 9, 17} x (cin, cout) in
{(4, 4), (8, 12), (20, 36)} x B in {1, 3}; the planar cin 3 image for forward and wgrad; S = 7 (with 8, 9 and 17 of the
grid: T - 1, T, T + 1 and 2 T + 1 for the kernels' spatial tile edge T = 8); and channel counts just below and just above
the kernels' channel blocks (28 / 36 around the weight gradient's 32 input channels, 60 / 68 around the 64 output
channels of the widest convolution block and of the weight gradient).  Each is held to max(4 x e32, 2 fp32 ulps of the
tensor's largest magnitude), e32 the error of torch's own fp32 CPU convolution on the same fp32-valued inputs."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from yololite_amd import stemops
from _head_cases import bar
from _train_dev import DEV

pytestmark = pytest.mark.gpu

T = 8                                                      # yl_stem_plan's conv_tile
KS = [(k, s) for k in (1, 3) for s in (1, 2)]
CHANNELS = [(4, 4), (8, 12), (20, 36)]
SHAPES = [(B, S, ci, co, False) for S in (1, 2, 5, T, T + 1, 2 * T + 1) for ci, co in CHANNELS for B in (1, 3)]
SHAPES += [(B, T - 1, ci, co, False) for ci, co in CHANNELS for B in (1, 3)]
SHAPES += [(1, T + 1, 28, 60, False), (1, T + 1, 36, 68, False)]
PLANAR = [(B, S, 3, co, True) for S in (1, 2, 5, T - 1, T, T + 1, 2 * T + 1) for co in (8, 32) for B in (1, 3)]
PASSES = ("forward", "dgrad", "wgrad")


def test_the_tile_edge_is_the_plans():
    assert stemops.plan(4, [dict(k=3, s=2, c=8)], 1, 9)["conv_tile"] == T


@functools.lru_cache(maxsize=None)
def cell(k, s, B, S, cin, cout):
    """inputs (fp32; x NHWC) and torch's CPU results in float64 and fp32: computed once, shared, never written to"""
    rs = np.random.RandomState(100000 * k + 10000 * s + 100 * S + 7 * cin + cout + B)
    So = (S + 2 * ((k - 1) // 2) - k) // s + 1
    x = rs.standard_normal((B, S, S, cin)).astype(np.float32)
    w = (rs.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
    dy = rs.standard_normal((B, So, So, cout)).astype(np.float32)
    res = {}
    for dt in (torch.float64, torch.float32):
        xt = torch.from_numpy(x).to(dt).permute(0, 3, 1, 2).requires_grad_(True)
        wt = torch.from_numpy(w).to(dt).requires_grad_(True)
        y = TF.conv2d(xt, wt, None, s, (k - 1) // 2)
        y.backward(torch.from_numpy(dy).to(dt).permute(0, 3, 1, 2))
        res[dt] = {"forward": y.detach().permute(0, 2, 3, 1).contiguous().numpy(),
                   "dgrad": xt.grad.permute(0, 2, 3, 1).contiguous().numpy(), "wgrad": wt.grad.numpy()}
    return x, w, dy, res[torch.float64], res[torch.float32]


def device_pass(pass_, k, s, x, w, dy, planar=False):
    t = lambda a: torch.from_numpy(a).to(DEV)              # noqa: E731
    xd = t(np.ascontiguousarray(x.transpose(0, 3, 1, 2))) if planar else t(x)
    layout = "nchw" if planar else "nhwc"
    if pass_ == "forward":
        return stemops.conv(xd, t(w), "forward", k, s, layout=layout)
    if pass_ == "dgrad":
        return stemops.conv(t(dy), t(w), "dgrad", k, s, size=x.shape[1])
    return stemops.conv(xd, t(dy), "wgrad", k, s, layout=layout)


def held(k, s, pass_, shapes):
    bad = []
    for B, S, cin, cout, planar in shapes:
        x, w, dy, r64, r32 = cell(k, s, B, S, cin, cout)
        got = device_pass(pass_, k, s, x, w, dy, planar).cpu().numpy()
        assert got.shape == r64[pass_].shape
        err = np.abs(got.astype(np.float64) - r64[pass_]).max()
        b = bar(np.abs(r32[pass_].astype(np.float64) - r64[pass_]).max(), np.abs(r64[pass_]).max())
        print(f"k{k} s{s} {pass_:7s} B{B} S{S:2d} {cin:2d}->{cout:2d} {'planar' if planar else 'nhwc  '}  err {err:.3e}  bar {b:.3e}")
        if not err <= b:
            bad.append((B, S, cin, cout, planar, err, b))
    assert not bad, bad


@pytest.mark.parametrize("pass_", PASSES)
@pytest.mark.parametrize("k,s", KS)
def test_every_cell_against_the_float64_convolution(k, s, pass_):
    held(k, s, pass_, SHAPES)


@pytest.mark.parametrize("pass_", ("forward", "wgrad"))
@pytest.mark.parametrize("k,s", KS)
def test_the_planar_image_against_the_float64_convolution(k, s, pass_):
    held(k, s, pass_, PLANAR)


@pytest.mark.parametrize("k,s", KS)
def test_a_one_hot_centre_tap_reproduces_x_bit_for_bit(k, s):
    """W[n][c] = delta_nc at the centre tap: any slip of the padding, of an offset or of the parity gather moves or
    drops a value"""
    for B, S, C in ((1, 1, 4), (3, 5, 20), (1, 8, 4), (3, 9, 12), (1, 2, 20), (1, 17, 36)):
        x = torch.from_numpy(cell(k, s, B, S, C, C)[0]).to(DEV)
        w = torch.zeros(C, C, k, k, device=DEV)
        w[torch.arange(C), torch.arange(C), k // 2, k // 2] = 1.0
        y = stemops.conv(x, w, "forward", k, s)
        assert torch.equal(y, x[:, ::s, ::s].contiguous()), (B, S, C)
        # and the transposed pass puts dy back where it came from, zeros elsewhere
        dx = stemops.conv(y, w, "dgrad", k, s, size=S)
        want = torch.zeros_like(x)
        want[:, ::s, ::s] = x[:, ::s, ::s]
        assert torch.equal(dx, want), (B, S, C)


@pytest.mark.parametrize("pass_", PASSES)
def test_two_calls_give_equal_bits(pass_):
    for k, s in KS:
        for B, S, cin, cout in ((3, 9, 20, 36), (3, 17, 8, 12)):
            x, w, dy, _, _ = cell(k, s, B, S, cin, cout)
            assert torch.equal(device_pass(pass_, k, s, x, w, dy), device_pass(pass_, k, s, x, w, dy))


@pytest.mark.parametrize("k,s", KS)
def test_image_0_does_not_change_by_a_bit_when_image_1_does(k, s):
    x, w, dy, _, _ = cell(k, s, 3, 9, 20, 36)
    x2, dy2 = x.copy(), dy.copy()
    x2[1:] = x2[1:] * 3 + 1
    dy2[1:] = dy2[1:] * 3 + 1
    for pass_ in ("forward", "dgrad"):
        a, b = device_pass(pass_, k, s, x, w, dy), device_pass(pass_, k, s, x2, w, dy2)
        assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])


@pytest.mark.parametrize("k,s", KS)
def test_weights_four_bytes_past_a_16_byte_boundary_give_the_bits_of_aligned_ones(k, s):
    x, w, dy, _, _ = cell(k, s, 3, 9, 20, 36)
    wd = torch.from_numpy(w).to(DEV)
    buf = torch.zeros(w.size + 1, device=DEV)
    assert buf.data_ptr() % 16 == 0
    off = buf[1:].view(w.shape)
    off.copy_(wd)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    xd, dyd = torch.from_numpy(x).to(DEV), torch.from_numpy(dy).to(DEV)
    assert torch.equal(stemops.conv(xd, off, "forward", k, s), stemops.conv(xd, wd, "forward", k, s))
    assert torch.equal(stemops.conv(dyd, off, "dgrad", k, s, size=9), stemops.conv(dyd, wd, "dgrad", k, s, size=9))
