"""The Winograd F(2x2,3x3) layer cases: shapes, one-layer programs, the float64 reference, the fp32 yardsticks and the bar.

A case is ONE dense 3x3 stride-1 pad-1 conv layer (bias, activation, optional residual after the activation, optional input
read nearest-upsampled by 2: `in_shift`) on a square G x G output grid.  tests/test_wino_cpu.py holds the yardsticks and the
bar to what they must be able to tell apart and takes the two censuses; tests/test_wino_gpu.py runs every case under every
kernel form ("dev_select") on the device and holds the layer's output to the float64 reference.

Which kernel a (case, form) runs is what the library says: `yl_query_wino_form`, the host function the launcher itself
calls (csrc/yl_shapes.h: yl_wino_form) -- nothing of the selection rule is written again here.

Reference: torch.nn.functional.conv2d in float64 on the CPU; activation and residual in float64, residual after the activation.
Yardsticks (plain numpy / torch on the CPU, restating the OPERATION, not a kernel's lane layout):
    direct    torch's fp32 conv2d, bias, activation, residual
    winograd  F(2x2,3x3) in float32: U = G g G^T, V = B^T d B, M = sum_c U . V in ascending 16-channel blocks,
              Y = A^T M A; G, B^T, A^T as in pack_wino (csrc/yl_program.cpp) and the kernel comment (csrc/yl_convc.hip);
              every transform stage is rounded once; SiLU is x / (1 + exp(-x))
Bar: _train_cases.bar -- max(4 x the yardstick's own max-abs error against float64, 2 fp32 ulps at max |f64|), per case over
the whole output tensor.

Classes (the census of the zoo).  The class of a layer at a batch is ONE tuple: the instantiation the library's query names
under the default dev_select (it carries in_shift), and
    KB         k-blocks of 16 input channels: 1 | 2 | 3 | even (>= 4) | odd (>= 5) -- the K loop's peeled forms
    tail       cin % 16 != 0: the last k-block has a channel tail
    n-tile     cout % 16 != 0: the last n-tile is partial
    grid       odd | even output grid
    fill       < 100 % of the 4 x 4-tile m-tiles' Winograd tiles exist
    act        the activation the KERNEL applies (GELU / ReLU + affine run in a pass of their own: the kernel sees none)
    res        residual in the epilogue
taken together.  A case's class is the one it has under the default dev_select; the forced forms run it through further
instantiations but do not count for the census."""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from _train_cases import bar  # noqa: F401  (the project's rule; used by both test files)

ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SILU = 0, 1, 2, 3

# dev_select values every case runs under: the first form, the launcher's own choice, and the three forced item shapes
DEV_WINO_V1, SHAPE_SHIFT = 1 << 11, 12
FORMS = (("v1", DEV_WINO_V1), ("auto", 0), ("s1", 1 << SHAPE_SHIFT), ("s2", 2 << SHAPE_SHIFT), ("s3", 3 << SHAPE_SHIFT))


def _case(tag, G, B, cin, cout, act, res=False, shift=0, seed=0):
    return dict(tag=tag, G=G, B=B, cin=cin, cout=cout, act=act, res=res, shift=shift, seed=seed)


CASES = [
    # KB 1 and one n-tile: the first form only.  9 tiles per image: a wave's 16 tiles straddle images; T = 27: one partial
    # 128-tile m-tile, fewer items than workgroups
    _case("k1", 5, 3, 16, 16, ACT_RELU),
    # KB 2: the second form at its minimum (only the two peeled blocks); 4-channel tail on both sides; MTOT = 3 against MT 2 and 4
    _case("k2tail", 7, 3, 20, 36, ACT_NONE),
    # odd KB (one block out of buffer 1) and an 8-channel tail; 77 % m-tile fill, odd edges
    _case("k3odd", 13, 2, 40, 52, ACT_SILU, res=True),
    # 56 % fill: the rule sends a second-form shape to the first form
    _case("sparse", 11, 2, 64, 64, ACT_RELU6),
    # KB 5, NTtot 9: under shape (2,7) the second item's n-tiles lie beyond the U image; first form: 5 n-groups, a partial group block
    _case("k5wrap", 20, 1, 72, 144, ACT_RELU, res=True),
    # even KB, NTtot 5
    _case("k8", 16, 2, 128, 80, ACT_SILU),
    # yololite_m's FPN width: KB 21 with a tail, NTtot 21
    _case("fpn328", 8, 5, 328, 328, ACT_RELU),
    # second form, upsampled input
    _case("up_a", 16, 3, 64, 64, ACT_SILU, shift=1),
    # first form, upsampled input; stored grid 5: odd
    _case("up_b", 10, 2, 24, 32, ACT_RELU, shift=1),
    # stored grid 7, KB 3, residual
    _case("up_c", 14, 3, 48, 48, ACT_NONE, res=True, shift=1),
    # (1024 / 4) * 3 = 768 items: the launcher's own choice is (4,3), the shape the benchmark runs
    _case("big43", 32, 64, 32, 144, ACT_RELU),
    _case("big43up", 32, 64, 32, 144, ACT_RELU, shift=1),
    # ---- the classes the MODEL_ZOO layers have (test_wino_cpu.py takes the census): SiLU on even grids, mostly.  Each case is the
    # smallest shape of its class; the (4,3) ones need >= 768 items (m-tiles / 4 x n-groups), which is what their batch is for
    # second form (2,3): efficientnetv2's conv_exp 48 -> 192 and 56 -> 224 @40, the 196-wide FPN @40 and @20 (69 % fill)
    _case("m23_k3", 8, 1, 48, 48, ACT_SILU),
    _case("m23_even_tail", 8, 1, 52, 48, ACT_SILU),
    _case("m23_odd_tail_n", 8, 1, 68, 36, ACT_SILU),
    _case("m23_odd_tail_n_fill", 14, 1, 68, 36, ACT_SILU),
    # second form (2,4): 32 -> 128 @80, the prototype branch (96 -> 64, 244 -> 64, 196 -> 64 @40), the 256-wide FPN @20
    _case("m24_k2", 8, 1, 32, 64, ACT_SILU),
    _case("m24_even", 8, 1, 64, 64, ACT_SILU),
    _case("m24_even_fill", 14, 1, 64, 64, ACT_SILU),
    _case("m24_even_tail", 8, 1, 52, 64, ACT_SILU),
    _case("m24_odd_tail", 8, 1, 72, 64, ACT_SILU),
    # second form (4,3) at the benchmark's batches: conv_exp 48 -> 192 and 56 -> 224 @40, the 196-wide FPN @40, and
    # yololite_m's own 328 -> 328 @20 at B = 64 (odd KB, channel tail, partial last n-tile, partial m-tiles, SiLU)
    _case("m43_k3", 8, 1024, 48, 144, ACT_SILU),
    _case("m43_even_tail", 8, 1024, 52, 144, ACT_SILU),
    _case("m43_odd_tail_n", 8, 3072, 68, 36, ACT_SILU),
    _case("m43_odd_tail_n_fill", 14, 768, 68, 36, ACT_SILU),
    # first form: hgnetv2's 16 -> 16, 32 -> 32, 64 -> 32 (ReLU + affine in a pass of its own: the kernel applies nothing),
    # efficientnetv2's 16 -> 16 with a residual and 32 -> 16, the 256- and 196-wide FPN @10 (39 % fill)
    _case("v1_k1_none", 8, 1, 16, 16, ACT_NONE),
    _case("v1_k1_res", 8, 1, 16, 16, ACT_SILU, res=True),
    _case("v1_k2_none", 8, 1, 32, 32, ACT_NONE),
    _case("v1_k2", 8, 1, 32, 16, ACT_SILU),
    _case("v1_even_none", 8, 1, 64, 32, ACT_NONE),
    _case("v1_even_fill", 10, 1, 64, 64, ACT_SILU),
    _case("v1_odd_tail_n_fill", 10, 1, 68, 36, ACT_SILU),
]
BY_TAG = {c["tag"]: c for c in CASES}
TAGS = [c["tag"] for c in CASES]

# ---- what ran: the library's own answer

def query(cin, cout, G, B, shift, dev):
    """(form, mt, nt) of yl_query_wino_form: 0 not Winograd, 1 first form, 2 second form with (mt, nt)"""
    from yololite_amd import _lib
    mt, nt = C.c_int32(), C.c_int32()
    f = _lib.load().yl_query_wino_form(cin, cout, G, G, B, shift, dev, C.byref(mt), C.byref(nt))
    return int(f), int(mt.value), int(nt.value)


def query_case(case, dev, B=None):
    return query(case["cin"], case["cout"], case["G"], case["B"] if B is None else B, case["shift"], dev)


def kernel_name(q, shift):
    """the instantiation a query answer names"""
    f, mt, nt = q
    if f == 1:
        return "yl_conv_wino_kernel<%d>" % shift
    if f == 2:
        return "yl_conv_wino2_kernel<%d, %d, %d>" % (mt, nt, shift)
    return None


ALL_KERNELS = ["yl_conv_wino_kernel<%d>" % s for s in (0, 1)] + \
              ["yl_conv_wino2_kernel<%d, %d, %d>" % (m, n, s) for m, n in ((4, 3), (4, 4), (2, 3), (2, 4), (2, 7)) for s in (0, 1)]


def klass(kernel, cin, cout, G, act, res):
    """the class tuple (see the module docstring) of a layer that `kernel` runs"""
    kb = -(-cin // 16)
    t = (G + 1) // 2
    kact = act if act < 4 else ACT_NONE                  # GELU / ReLU + affine: applied by a pass behind the kernel
    return (kernel, "KB " + (str(kb) if kb <= 3 else ("even" if kb % 2 == 0 else "odd")), "tail" if cin % 16 else "no tail",
            "partial n-tile" if cout % 16 else "full n-tiles", "odd grid" if G % 2 else "even grid",
            "fill < 100 %" if t * t < (-(-t // 4)) ** 2 * 16 else "fill 100 %",
            {ACT_NONE: "none", ACT_RELU: "relu", ACT_RELU6: "relu6", ACT_SILU: "silu"}[kact],
            "residual" if res and act < 4 else "no residual")


def case_classes():
    """class -> the tags of the cases that have it (under the default dev_select)"""
    out = {}
    for c in CASES:
        k = kernel_name(query_case(c, 0), c["shift"])
        out.setdefault(klass(k, c["cin"], c["cout"], c["G"], c["act"], c["res"]), []).append(c["tag"])
    return out


# ---- weights, inputs, programs

def weights(case):
    """(w [cout, cin, 3, 3], b [cout]) fp32: randn / sqrt(9 cin), 0.1 randn, seeded per case"""
    rng = np.random.RandomState(7000 + 31 * TAGS.index(case["tag"]) + case["seed"])
    w = (rng.randn(case["cout"], case["cin"], 3, 3) / np.sqrt(9 * case["cin"])).astype(np.float32)
    b = (0.1 * rng.randn(case["cout"])).astype(np.float32)
    return w, b


def host_inputs(case):
    """signed fp32 inputs for the tests that have no device: (x [B, Gs, Gs, cin] stored grid, res [B, G, G, cout] or None)"""
    rng = np.random.RandomState(9000 + TAGS.index(case["tag"]))
    Gs = case["G"] >> case["shift"]
    x = rng.randn(case["B"], Gs, Gs, case["cin"]).astype(np.float32)
    r = rng.randn(case["B"], case["G"], case["G"], case["cout"]).astype(np.float32) if case["res"] else None
    return x, r


def program(case):
    """stem 3 -> 32 stride 2 -> feed (32 -> cin, no activation: signed inputs) -> [the 3x3 layer] -> 1x1 head output.
    Slots: 0 stem, 1 the layer's input, 2 its output, 3 the residual (a second feed of the output's shape).
    in_shift: the image side is G, so the stem's grid is the stored grid G / 2; with a residual the image side is 2 G, the
    residual feed reads the stem's G x G grid and the layer's input is a 3x3 stride-2 feed on G / 2."""
    from yololite_amd import _lib
    from yololite_amd.program import Layer, Program
    G, cin, cout, sh = case["G"], case["cin"], case["cout"], case["shift"]
    rng = np.random.RandomState(5000 + TAGS.index(case["tag"]))
    wl, bl = weights(case)

    def w(*shape):
        return (rng.randn(*shape) / np.sqrt(int(np.prod(shape[1:])))).astype(np.float32)

    def b(n):
        return (rng.randn(n) * 0.1).astype(np.float32)

    Gs = G >> sh
    down = bool(sh and case["res"])                      # the stem runs on G x G and a strided feed makes the stored grid
    Gstem = G if (down or not sh) else Gs
    # (no ReLU in front of the layer: it would turn the NaN image of the isolation test into zeros)
    L = [_lib_layer(Layer, _lib.OP_STEM, -1, 0, 3, 32, 3, 2, 1, ACT_NONE, w(32, 3, 3, 3), b(32), "stem")]
    if down:
        L.append(_lib_layer(Layer, _lib.OP_CONV, 0, 1, 32, cin, 3, 2, 1, ACT_NONE, w(cin, 32, 3, 3), b(cin), "feed"))
    else:
        L.append(_lib_layer(Layer, _lib.OP_CONV, 0, 1, 32, cin, 1, 1, 0, ACT_NONE, w(cin, 32, 1, 1), b(cin), "feed"))
    slots = [(Gstem, Gstem, 32), (Gs, Gs, cin), (G, G, cout)]
    if case["res"]:
        L.append(_lib_layer(Layer, _lib.OP_CONV, 0, 3, 32, cout, 1, 1, 0, ACT_NONE, w(cout, 32, 1, 1), b(cout), "resfeed"))
        slots.append((G, G, cout))
    lay = Layer(_lib.OP_CONV, 1, 2, cin, cout, 3, 1, 1, 1, case["act"], wl, bl, in_shift=sh, res_slot=3 if case["res"] else -1,
                name="wino")
    L.append(lay)
    L.append(Layer(_lib.OP_CONV, 2, -1, cout, 6, 1, 1, 0, 0, ACT_NONE, w(6, cout, 1, 1), b(6), head_level=0, name="out"))
    return Program(img_size=2 * Gstem, num_classes=1, level_size=[G], level_anchors=[1], strides=[2 * Gstem // G],
                   layers=L, slots=slots)


def _lib_layer(Layer, op, i, o, cin, cout, k, s, pad, act, w, b, name):
    return Layer(op, i, o, cin, cout, k, s, pad, pad, act, w, b, name=name)


# ---- the operation, in any precision

def upsample(x, shift, round_up=False):
    """[B, Gs, Gs, C] stored -> the tensor the conv sees: pixel i reads stored pixel i >> shift (round_up: the WRONG index
    (i + 1) >> shift, clipped -- a mistake the bar must catch)"""
    if not shift:
        return x
    if not round_up:
        return x.repeat(2, axis=1).repeat(2, axis=2)
    n = x.shape[1]
    idx = np.minimum((np.arange(2 * n) + 1) >> 1, n - 1)
    return x[:, idx][:, :, idx]


def act_np(y, act, dt):
    if act == ACT_RELU:
        return np.maximum(y, dt(0))
    if act == ACT_RELU6:
        return np.minimum(np.maximum(y, dt(0)), dt(6))
    if act == ACT_SILU:
        return (y / (dt(1) + np.exp(-y).astype(dt)).astype(dt)).astype(dt)
    return y


def epilogue(y, b, act, res, dt, res_first=False):
    """bias, activation, residual AFTER the activation, each rounded once (res_first: the wrong order)"""
    y = (y + b.astype(dt)).astype(dt)
    if res is not None and res_first:
        return act_np((y + res.astype(dt)).astype(dt), act, dt)
    y = act_np(y, act, dt)
    return y if res is None else (y + res.astype(dt)).astype(dt)


def reference(x, w, b, act, res):
    """float64: torch conv2d on the (already upsampled) NHWC input -> NHWC output"""
    y = F.conv2d(torch.from_numpy(np.ascontiguousarray(x)).double().permute(0, 3, 1, 2), torch.from_numpy(w).double(), padding=1)
    y = y.permute(0, 2, 3, 1).contiguous().numpy()
    return epilogue(y, b, act, res, np.float64)


def yard_direct(x, w, b, act, res):
    """torch's fp32 conv2d, then the fp32 epilogue"""
    y = F.conv2d(torch.from_numpy(np.ascontiguousarray(x)).float().permute(0, 3, 1, 2), torch.from_numpy(w).float(), padding=1)
    return epilogue(y.permute(0, 2, 3, 1).contiguous().numpy(), b, act, res, np.float32)


_G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
_BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]])
_AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]])


def wino_conv(x, w, dt, blk=16, right_from_neighbour=False):
    """F(2x2,3x3) of the NHWC input x with taps w [N, C, 3, 3] in precision dt -> [B, H, W, N] (no bias).
    One rounding per transform stage (G g, (G g) G^T; B^T d, (B^T d) B; A^T M, (A^T M) A); the channel sum in ascending
    blocks of `blk` channels, each block's partial sum rounded and added to the running sum.
    right_from_neighbour: the column right of the image repeats the last column instead of zero (a mistake)."""
    B, H, W, Cn = x.shape
    N = w.shape[0]
    TH, TW = (H + 1) // 2, (W + 1) // 2
    xp = np.zeros((B, 2 * TH + 2, 2 * TW + 2, Cn), dt)
    xp[:, 1:H + 1, 1:W + 1] = x
    if right_from_neighbour:
        xp[:, 1:H + 1, W + 1] = x[:, :, W - 1]
    g, bt, at = _G.astype(dt), _BT.astype(dt), _AT.astype(dt)
    U = np.einsum("ir,ncrq->nciq", g, w.astype(dt)).astype(dt)
    U = np.einsum("jq,nciq->ncij", g, U).astype(dt)
    d = np.stack([np.stack([xp[:, r:r + 2 * TH:2, q:q + 2 * TW:2] for q in range(4)]) for r in range(4)])   # [r][q][B][TH][TW][C]
    V = np.einsum("ir,rqbyxc->iqbyxc", bt, d).astype(dt)
    V = np.einsum("jq,iqbyxc->ijbyxc", bt, V).astype(dt)
    M = np.zeros((4, 4, B, TH, TW, N), dt)
    for i in range(4):
        for j in range(4):
            v = V[i, j].reshape(-1, Cn)
            acc = np.zeros((v.shape[0], N), dt)
            for k0 in range(0, Cn, blk):
                acc = (acc + (v[:, k0:k0 + blk] @ U[:, k0:k0 + blk, i, j].T).astype(dt)).astype(dt)
            M[i, j] = acc.reshape(B, TH, TW, N)
    R = np.einsum("ai,ijbyxn->ajbyxn", at, M).astype(dt)
    Y = np.einsum("cj,ajbyxn->acbyxn", at, R).astype(dt)
    y = np.zeros((B, 2 * TH, 2 * TW, N), dt)
    for a in range(2):
        for c in range(2):
            y[:, a::2, c::2] = Y[a, c]
    return y[:, :H, :W]


def yard_wino(x, w, b, act, res, dt=np.float32, blk=16, **kw):
    return epilogue(wino_conv(x.astype(dt), w, dt, blk, **kw), b, act, res, dt)


def row(ref, yard, got=None):
    """the figures of one comparison: max |f64|, the yardstick's error, the bar and (with a result) its error and ratio"""
    m64 = float(np.abs(ref).max())
    e32 = float(np.abs(yard.astype(np.float64) - ref).max())
    r = {"max_f64": m64, "err32": e32, "bar": bar(e32, m64)}
    if got is not None:
        r["device_error"] = float(np.abs(got.astype(np.float64) - ref).max())
        r["ratio"] = r["device_error"] / r["bar"]
    return r
