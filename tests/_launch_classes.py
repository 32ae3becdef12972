"""Which form every launch of the trainable modules takes, as a function of the module's configuration and (B, sizes):
the few host functions of csrc/ that decide a launch's grid and template, written again in Python, and on top of them a
map from a module at a shape to a set of labels (kernel source, pass, axis, value).  No device, no library.

tests/test_launch_classes_cpu.py holds the restated plans to what the library's own plan functions report, and takes the
census: every label a MODEL_ZOO model reaches in training must be reached by a parity case (`CASES` / `WIDE` of the
_*_cases.py files) or, for the GEMM and the depthwise kernels, by an op-level test shape.

Restated (re-derive when the C++ changes):
    csrc/yl_bn.h       pick_cq, STAT_ROWS = 256, NT = 256; the launches of bn_forward / bn_backward_sums, which every walk
                       below goes through with its activation
    csrc/yl_block.h    pick_pt, split_plan, GEMM_ROWS = 64; the launches of blocks_forward / blocks_backward
    csrc/yl_head.hip   the three output GEMMs, column sums over 64 columns per workgroup
    csrc/yl_fpn.h      the lateral's three GEMMs and its bias sums
    csrc/yl_dneck.hip  CT = 8, CNB = 64, GB = 64, CKB = 16 (32 in the 16x16x32 forms), w3_split
    csrc/yl_stage.hip  make_units, the depthwise weight gradient per (k, stride)
    csrc/yl_stem.hip   pick_conv_pt, ST_T = 8, GC = 32, GN = 64, wgrad3_plan, stat_rows_of
    csrc/yl_units.h    the walk: which activation a unit's BatchNorm runs with
The axes are independent: a label says one thing about one launch, never a combination."""
NT = 256
STAT_ROWS = 256
GEMM_ROWS = 64
STAT_TILES_MAX = 1024
CT, CNB, GB = 8, 64, 64
ST_T, GC, GN = 8, 32, 64


def cdiv(a, b):
    return -(-a // b)


def r16(v):
    return (v + 15) // 16 * 16


# ---- csrc/yl_bn.h

def pick_cq(F):
    """channel quads per workgroup of the row reductions: a power of two <= 64"""
    cq = 1
    while cq < (F >> 2) and cq < 64:
        cq <<= 1
    return cq


# ---- csrc/yl_block.h

def pick_pt(NP):
    """p-tiles per wave: 4 (64 columns) or 6 (96), whichever pads NP less"""
    return 6 if cdiv(NP, 96) * 96 < cdiv(NP, 64) * 64 else 4


def split_plan(M, NP, NQ, gemm_rows=GEMM_ROWS):
    """-> (rows per split, splits, which bound decided: "most" | "free" | "cap128" | "floor8")"""
    tiles = cdiv(NP, 16 * pick_pt(NP)) * cdiv(NQ, gemm_rows)
    want = 1024 // tiles
    bound = "floor8" if want < 8 else ("cap128" if want > 128 else "free")
    want = min(max(want, 8), 128)
    most = cdiv(M, 64)
    if most < want:
        want, bound = most, "most"
    rows = cdiv(cdiv(M, want), 16) * 16
    return rows, cdiv(M, rows), bound


# ---- csrc/yl_stem.hip

def pick_conv_pt(N):
    """16 PT output channels per workgroup: the PT of {4, 3, 2} that pads N least"""
    best = 4
    for pt in (3, 2):
        if cdiv(N, 16 * pt) * pt < cdiv(N, 16 * best) * best:
            best = pt
    return best


def stat_rows_of(M):
    return STAT_ROWS * cdiv(cdiv(M, STAT_ROWS), STAT_TILES_MAX)


def wgrad3_plan(B, Sout, cin, cout):
    """-> (tiles per split, splits) of the stem's 3x3 weight gradient"""
    ntiles = B * cdiv(Sout, ST_T) ** 2
    blocks = cdiv((cin + 3) // 4 * 4, GC) * cdiv(cout, GN)
    want = min(max(1024 // blocks, 1), ntiles)
    tps = cdiv(ntiles, want)
    return tps, cdiv(ntiles, tps)


# ---- csrc/yl_dneck.hip

def w3_split(F, tiles):
    """-> (tiles per split, splits) of the dense neck's 3x3 weight gradient"""
    want = min(max(512 // cdiv(F, GB) ** 2, 1), 64, tiles)
    tps = cdiv(tiles, want)
    return tps, cdiv(tiles, tps)


# ---- labels

def _three(n, full):
    return "1" if n == 1 else (">=2 last full" if full else ">=2 last ragged")


def gemm(src, pass_, NP, NQ, NR, splits=1, bound=None):
    """yl_head_gemm_kernel through launch_gemm: grid (p-tiles, q groups of 64, splits); r in steps of 16"""
    pt = pick_pt(NP)
    out = {("pt", str(pt)), ("p-tiles", "1" if cdiv(NP, 16 * pt) == 1 else ">=2"),
           ("NP % (16 pt)", "0" if NP % (16 * pt) == 0 else "ragged"), ("q groups", "1" if cdiv(NQ, 64) == 1 else ">=2"),
           ("NQ % 64", "0" if NQ % 64 == 0 else "ragged"), ("NR % 16", "0" if NR % 16 == 0 else "ragged"),
           ("splits", "1" if splits == 1 else ">=2")}
    if bound is not None:
        out.add(("split bound", bound))
    return {(src, pass_, a, v) for a, v in out}


def wgrad_gemm(src, NP, NQ, M):
    _, splits, bound = split_plan(M, NP, NQ)
    return gemm(src, "wgrad", NP, NQ, M, splits, bound)


def rows(src, pass_, M, C, stat_rows=STAT_ROWS):
    """a row reduction: grid (row tiles, groups of pick_cq(C) channel quads)"""
    q, cq = C >> 2, pick_cq(C)
    return {(src, pass_, "channel groups", _three(cdiv(q, cq), q % cq == 0)),
            (src, pass_, "row tiles", _three(cdiv(M, stat_rows), M % stat_rows == 0))}


def colsums(src, M, N):
    """yl_head_ysum_kernel: grid (row tiles, groups of 64 columns)"""
    return {(src, "bwd", "column groups", _three(cdiv(N, 64), N % 64 == 0)),
            (src, "bwd", "row tiles", _three(cdiv(M, STAT_ROWS), M % STAT_ROWS == 0))}


def per_channel(src, n):
    """one thread per output element, NT to a workgroup"""
    return {(src, "-", "workgroups", "1" if cdiv(n, NT) == 1 else ">=2")}


def batchnorm(act, M, F, stat_rows=STAT_ROWS):
    """bn_forward + bn_backward_sums of csrc/yl_bn.h over M rows of F channels: the column sums of both passes and the two
    second stages.  The activation is a template argument that the cut into tiles and groups does not depend on: an axis
    of its own"""
    out = rows("bn_colstats", "fwd", M, F, stat_rows) | rows("bn_colstats", "bwd", M, F, stat_rows)
    out.add(("bn_colstats", "bwd", "act", act))
    return out | per_channel("bn_stats", F) | per_channel("bn_grads", F)


def _blocks(M, F):
    """a run of DWConvBlocks of yl_block.h at M rows: blocks_forward + blocks_backward with every gradient wanted"""
    out = gemm("gemm", "forward", F, M, F) | gemm("gemm", "dgrad", F, M, F) | wgrad_gemm("gemm", F, F, M)
    out |= batchnorm("relu", M, F) | rows("head_dw_wgrad", "bwd", M, F) | per_channel("head_dw_wsum", 9 * F)
    out |= per_channel("head_wsum", F * F)
    return out


def head_plan(F, C, A, depth, B, S):
    M, NE = B * S * S, A * (5 + C)
    w, o = split_plan(M, F, F), split_plan(M, F, NE)
    return dict(rows=M, stat_tiles=cdiv(M, STAT_ROWS), gemm_tiles=cdiv(M, GEMM_ROWS), wgrad_rows=w[0], wgrad_splits=w[1],
                ograd_rows=o[0], ograd_splits=o[1])


def head_labels(F, C, A, depth, B, sizes):
    out = set()
    for S in sizes:
        M, NE = B * S * S, A * (5 + C)
        out |= _blocks(M, F)
        out |= gemm("gemm.head_out", "forward", NE, M, F) | gemm("gemm.head_out", "dgrad", F, M, NE)
        out |= wgrad_gemm("gemm.head_out", F, NE, M)
        out |= colsums("head_ysum", M, NE) | per_channel("head_bsum", NE) | per_channel("head_wsum", NE * F)
    return out


def _lateral(M, Cin, F):
    out = gemm("gemm", "forward", F, M, Cin) | gemm("gemm", "dgrad", Cin, M, F) | wgrad_gemm("gemm", Cin, F, M)
    return out | colsums("head_ysum", M, F) | per_channel("neck_bsum", F) | per_channel("head_wsum", F * Cin)


def neck_plan(Cin, F, depth, B, sizes):
    out = []
    for ci, S in zip(Cin, sizes):
        M = B * S * S
        w, l = split_plan(M, F, F), split_plan(M, ci, F)
        out.append(dict(rows=M, stat_tiles=cdiv(M, STAT_ROWS), gemm_tiles=cdiv(M, GEMM_ROWS), wgrad_rows=w[0],
                        wgrad_splits=w[1], lgrad_rows=l[0], lgrad_splits=l[1]))
    return out


def neck_labels(Cin, F, depth, B, sizes):
    out = set()
    for ci, S in zip(Cin, sizes):
        out |= _lateral(B * S * S, ci, F) | _blocks(B * S * S, F)
    return out


def dense_neck_plan(Cin, F, depth, B, sizes):
    out = []
    for ci, S in zip(Cin, sizes):
        M, tiles = B * S * S, B * cdiv(S, CT) ** 2
        l, w3 = split_plan(M, ci, F), w3_split(F, tiles)
        out.append(dict(rows=M, stat_tiles=cdiv(M, STAT_ROWS), gemm_tiles=cdiv(M, GEMM_ROWS), conv_tiles=tiles,
                        lgrad_rows=l[0], lgrad_splits=l[1], w3grad_tiles=w3[0], w3grad_splits=w3[1]))
    return out


def _cblocks(n, ragged):
    return ("1" if n == 1 else ("2" if n == 2 else ">=3")), ("ragged" if ragged else "full")


def dense_conv(pass_, F):
    """yl_dneck_conv_kernel: CNB output channels per workgroup, k-blocks of 16 (fp32, 16x16x16) or 32 input channels"""
    n, last = _cblocks(cdiv(F, CNB), F % CNB)
    return {("dneck_conv", pass_, "channel blocks", n), ("dneck_conv", pass_, "last channel block", last),
            ("dneck_conv", pass_, "last k-block of 16", "ragged" if F % 16 else "full"),
            ("dneck_conv", pass_, "last k-block of 32", "ragged" if F % 32 else "full")}


def dense_wgrad(F, S, B):
    """yl_dneck_wgrad_kernel: grid (GB-blocks of x channels, GB-blocks of dz channels, runs of spatial tiles); its k index
    is the pixel, so the k-block that can be ragged is the spatial tile"""
    n, last = _cblocks(cdiv(F, GB), F % GB)
    splits = w3_split(F, B * cdiv(S, CT) ** 2)[1]
    return {("dneck_wgrad", "wgrad", "channel blocks", n), ("dneck_wgrad", "wgrad", "last channel block", last),
            ("dneck_wgrad", "wgrad", "last k-block", "ragged" if S % CT else "full"),
            ("dneck_wgrad", "wgrad", "splits", "1" if splits == 1 else ">=2")}


def dense_neck_labels(Cin, F, depth, B, sizes):
    out = set()
    for ci, S in zip(Cin, sizes):
        M = B * S * S
        out |= _lateral(M, ci, F)
        out |= dense_conv("forward", F) | dense_conv("dgrad", F) | dense_wgrad(F, S, B)
        out |= batchnorm("silu", M, F)
        out |= per_channel("dneck_pack", 9 * F * F) | per_channel("dneck_wsum", 9 * F * F)
    return out


def dense_conv_op_labels(F, S, B):
    """neckops.conv3x3 at one shape: the three passes as the module launches them"""
    return dense_conv("forward", F) | dense_conv("dgrad", F) | dense_wgrad(F, S, B)


def stage_units(cin, blocks, B, S):
    """make_units of csrc/yl_stage.hip -> [dict(block, slot, dw, relu, k, s, cin, cout, M, rows, splits)]"""
    import _stage_cases as sc
    case = dict(cin=cin, blocks=[dict(b, name=b.get("name", str(i))) for i, b in enumerate(blocks)], S=S)
    out = []
    block = -1
    for u, So in zip(sc.units(case), sc.sizes(case)[1:]):
        if u["first"]:
            block += 1
        slot = {"dw_start": 0, "pw_exp": 1, "dw_mid": 2, "pw_proj": 3}.get(u["key"].split(".")[-2], 1)    # a cn block's unit: 1
        M = B * So * So
        r, s = (0, 0) if u["dw"] else split_plan(M, u["cin"], u["cout"])[:2]
        out.append(dict(block=block, slot=slot, dw=u["dw"], relu=u["relu"], k=u["k"], s=u["s"], cin=u["cin"], cout=u["cout"], M=M,
                        rows=r, splits=s))
    return out


def stage_plan(cin, blocks, B, S):
    """per block: stat_tiles_mid / _out, exp_rows / _splits, proj_rows / _splits as yl_stage_plan reports them"""
    out = []
    for u in stage_units(cin, blocks, B, S):
        if len(out) <= u["block"]:
            out.append(dict(exp_rows=0, exp_splits=0, proj_rows=0, proj_splits=0))
        p = out[-1]
        if u["slot"] == 1:
            p.update(exp_rows=u["rows"], exp_splits=u["splits"], stat_tiles_mid=cdiv(u["M"], STAT_ROWS))
        if u["slot"] == 3:
            p.update(proj_rows=u["rows"], proj_splits=u["splits"])
        p["stat_tiles_out"] = cdiv(u["M"], STAT_ROWS)
    return out


def dw_labels(k, s, Mo, C):
    """yl_stage_dw_wgrad_kernel<k, s> and the ordered sum behind it at Mo OUTPUT rows"""
    return rows(f"stage_dw_wgrad.k{k}s{s}", "wgrad", Mo, C) | per_channel("stage_dw_wsum", k * k * C)


def _unit_tail(u, stat_rows=STAT_ROWS):
    """what yl_units.h's walk launches around a unit's convolution (the stem's row reductions take more rows per tile)"""
    return batchnorm("relu" if u["relu"] else "none", u["M"], u["cout"], stat_rows)


def stage_labels(cin, blocks, B, S):
    out = set()
    for u in stage_units(cin, blocks, B, S):
        out |= _unit_tail(u)
        if u["dw"]:
            out |= dw_labels(u["k"], u["s"], u["M"], u["cout"])
        else:
            out |= gemm("gemm", "forward", u["cout"], u["M"], u["cin"]) | gemm("gemm", "dgrad", u["cin"], u["M"], u["cout"])
            out |= wgrad_gemm("gemm", u["cin"], u["cout"], u["M"]) | per_channel("head_wsum", u["cin"] * u["cout"])
    return out


def stem_units(cin, units, B, S, planar):
    import _stage_cases as sc
    out = []
    for i, u in enumerate(units):
        So = sc.out_size(S, u["k"], u["s"])
        M = B * So * So
        sr = stat_rows_of(M)
        r, s = split_plan(M, cin, u["c"])[:2] if u["k"] == 1 else wgrad3_plan(B, So, cin, u["c"])
        out.append(dict(k=u["k"], s=u["s"], cin=cin, cout=u["c"], relu=True, Sin=S, Sout=So, M=M, planar=planar and i == 0,
                        stat_rows=sr, stat_tiles=cdiv(M, sr), wgrad_rows=r, wgrad_splits=s,
                        conv_block=16 * pick_conv_pt(u["c"]) if u["k"] == 3 else 0))
        S, cin = So, u["c"]
    return out


def stem_labels(cin, units, B, S, planar):
    out = set()
    for u in stem_units(cin, units, B, S, planar):
        out |= _unit_tail(u, u["stat_rows"])
        if u["k"] == 3:
            # forward; the input gradient runs the same kernel on dz (stride 1: flipped taps, cin outputs; stride 2: its four
            # parity classes, stride-1 launches of cin outputs); the planar image has none
            fwd = f"stem_conv<{u['s']}, {'planar' if u['planar'] else 'nhwc'}>"
            convs = [(fwd, "forward", u["cout"])] + ([] if u["planar"] else [("stem_conv<1, nhwc>", "dgrad", u["cin"])])
            for src, pass_, N in convs:
                pt = pick_conv_pt(N)
                out |= {(src, pass_, "PT", str(pt)), (src, pass_, "channel blocks", "1" if cdiv(N, 16 * pt) == 1 else ">=2")}
            Cp = (u["cin"] + 3) // 4 * 4
            out |= {("stem_wgrad", "wgrad", "x channel blocks", "1" if cdiv(Cp, GC) == 1 else ">=2"),
                    ("stem_wgrad", "wgrad", "dz channel blocks", "1" if cdiv(u["cout"], GN) == 1 else ">=2"),
                    ("stem_wgrad", "wgrad", "splits", "1" if u["wgrad_splits"] == 1 else ">=2")}
            out |= per_channel("stem_wsum", 9 * u["cout"] * u["cin"])
        else:
            src = "gemm" if u["s"] == 1 and not u["planar"] else "gemm.stem_src"
            out |= gemm(src, "forward", u["cout"], u["M"], u["cin"]) | wgrad_gemm(src, u["cin"], u["cout"], u["M"])
            if not u["planar"]:
                out |= gemm(src, "dgrad", u["cin"], u["M"], u["cout"])
            out |= per_channel("head_wsum", u["cin"] * u["cout"])
    return out


# ---- op-level test shapes (the GEMM's and the depthwise kernels' labels only)

def head_gemm_op_labels(F, C, A, B, S):
    """headops.head_gemm, sites 0 and "out", the three passes, as the module launches them"""
    M, NE = B * S * S, A * (5 + C)
    out = gemm("gemm", "forward", F, M, F) | gemm("gemm", "dgrad", F, M, F) | wgrad_gemm("gemm", F, F, M)
    out |= gemm("gemm.head_out", "forward", NE, M, F) | gemm("gemm.head_out", "dgrad", F, M, NE) | wgrad_gemm("gemm.head_out", F, NE, M)
    return out


def depthwise_op_labels(k, s, B, S, C):
    import _stage_cases as sc
    So = sc.out_size(S, k, s)
    return dw_labels(k, s, B * So * So, C)
