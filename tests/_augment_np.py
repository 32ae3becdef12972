"""Two independent restatements of what yl_augment (csrc/yl_aug.hip, the contract in include/yololite_hip.h) computes.

render32: numpy float32 / uint32, operation by operation, from the two fp32 descriptor tables the kernel itself reads:
the bit-exact target.  render64: float64 from the float64 matrix and rectangles of yololite_amd.augment.compose, HSV
through Python's colorsys, the same counter hash for the noise; it also gives each pixel's distance, in frame pixels,
to the nearest frame or tile boundary under the float64 map (where a one-ulp difference of the coordinate changes
which side a pixel falls on, the two may differ by any amount)."""
import colorsys

import numpy as np

F = np.float32
U = np.uint32
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)


def mix(h):
    h = h ^ (h >> U(16)); h = h * U(0x7feb352d)
    h = h ^ (h >> U(15)); h = h * U(0x846ca68b)
    return h ^ (h >> U(16))


def noise_sums(seed, S):
    """[3,S,S] uint32: the sum of the twelve 24-bit uniforms of (seed, channel, y, x)"""
    ys, xs = np.meshgrid(np.arange(S, dtype=U), np.arange(S, dtype=U), indexing="ij")
    out = np.zeros((3, S, S), U)
    for ch in range(3):
        key = mix(U(seed) ^ mix(ys * U(0x9E3779B1) + U(ch)))
        key = mix(key ^ (xs * U(0x85EBCA77)))
        for k in range(12):
            out[ch] += mix(key + U((k * 0xC2B2AE3D) & 0xFFFFFFFF)) >> U(8)
    return out


def _clip255(v):
    return np.minimum(np.maximum(v, F(0)), F(255))


def _hsv32(c, dh, ds, dv):
    r, g, b = c
    v = np.maximum(np.maximum(r, g), b)
    mn = np.minimum(np.minimum(r, g), b)
    d = v - mn
    pos = d > 0
    sd, sv = np.where(pos, d, F(1)), np.where(pos, v, F(1))
    s = np.where(pos, d / sv, F(0))
    h = np.where(v == r, F(60) * ((g - b) / sd),
                 np.where(v == g, F(120) + F(60) * ((b - r) / sd), F(240) + F(60) * ((r - g) / sd)))
    h = np.where(h < 0, h + F(360), h)
    h = np.where(pos, h, F(0))
    h = h + F(2) * F(dh)
    h = np.where(h < 0, h + F(360), h)
    h = np.where(h >= F(360), h - F(360), h)
    s = np.minimum(np.maximum(s + F(ds) / F(255), F(0)), F(1))
    v = _clip255(v + F(dv))
    hp = h / F(60)
    fi = np.floor(hp)
    f = hp - fi
    p = v * (F(1) - s)
    q = v * (F(1) - s * f)
    t = v * (F(1) - s * (F(1) - f))
    i = fi.astype(np.int32)
    sel = lambda a0, a1, a2, a3, a4, a5: np.where(i == 0, a0, np.where(i == 1, a1, np.where(i == 2, a2, np.where(
        i == 3, a3, np.where(i == 4, a4, a5)))))
    return np.stack([sel(v, q, p, p, t, v), sel(t, v, v, q, p, p), sel(p, p, t, v, v, q)])


def render32(packed, tiles, imgs, S):
    """packed: the uint8 buffer; tiles / imgs: augment.TILE_DESC / IMAGE_DESC arrays.  -> [B,3,S,S] float32"""
    out = np.empty((len(imgs), 3, S, S), F)
    ys, xs = np.meshgrid(np.arange(S, dtype=np.int32), np.arange(S, dtype=np.int32), indexing="ij")
    xf, yf = xs.astype(F), ys.astype(F)
    for bi, im in enumerate(imgs):
        ry, rx = ys - im["top"], xs - im["left"]
        inside = (ry >= 0) & (ry < im["nh"]) & (rx >= 0) & (rx < im["nw"])
        m = im["m"]
        u = (m[0] * xf + m[1] * yf) + m[2]
        v = (m[3] * xf + m[4] * yf) + m[5]
        assert u.dtype == F and v.dtype == F
        todo = inside & (u >= 0) & (u < F(im["frame_w"])) & (v >= 0) & (v < F(im["frame_h"]))
        c = np.full((3, S, S), 114, F)
        for t in tiles[im["first_tile"]:im["first_tile"] + im["num_tiles"]]:
            sel = todo & (u >= t["x0"]) & (u < t["x1"]) & (v >= t["y0"]) & (v < t["y1"])
            todo = todo & ~sel
            h0, w0 = int(t["h0"]), int(t["w0"])
            src = packed[int(t["offset"]):int(t["offset"]) + h0 * w0 * 3].reshape(h0, w0, 3).astype(F)
            sx, sy = F(w0) / (t["x1"] - t["x0"]), F(h0) / (t["y1"] - t["y0"])
            fx = np.where(sel, (u - t["x0"]) * sx - F(0.5), F(0))
            fy = np.where(sel, (v - t["y0"]) * sy - F(0.5), F(0))
            flx, fly = np.floor(fx), np.floor(fy)
            ax, ay = fx - flx, fy - fly
            ix, iy = flx.astype(np.int32), fly.astype(np.int32)
            x0, x1 = np.clip(ix, 0, w0 - 1), np.clip(ix + 1, 0, w0 - 1)
            y0, y1 = np.clip(iy, 0, h0 - 1), np.clip(iy + 1, 0, h0 - 1)
            bgr = []
            for ch in range(3):
                p00, p01, p10, p11 = src[y0, x0, ch], src[y0, x1, ch], src[y1, x0, ch], src[y1, x1, ch]
                a = p00 + (p01 - p00) * ax
                b = p10 + (p11 - p10) * ax
                bgr.append(a + (b - a) * ay)
            rgb = bgr[::-1]
            for ch in range(3):
                c[ch] = np.where(sel, rgb[int(im["perm"][ch])], c[ch])
        mode, col = int(im["color_mode"]), im["color"]
        if mode == 1:
            beta = col[1] * F(255)
            c = np.where(inside, _clip255(col[0] * c + beta), c)
        elif mode == 2:
            c = np.where(inside, _clip255(_hsv32(c, col[0], col[1], col[2])), c)
        elif mode == 3:
            c = np.where(inside, _clip255(c + col[:3, None, None]), c)
        if im["noise_sigma"] > 0:
            n = noise_sums(int(im["noise_seed"]), S).astype(F) * F(1.0 / 16777216.0) - F(6)
            c = np.where(inside, _clip255(c + im["noise_sigma"] * n), c)
        assert c.dtype == F
        m255 = MEAN * F(255)
        d = F(1) / (STD * F(255))
        out[bi] = (c - m255[:, None, None]) * d[:, None, None]
    return out


def _hsv64(c, dh, ds, dv):
    out = np.empty_like(c)
    flat, oflat = c.reshape(3, -1), out.reshape(3, -1)
    for k in range(flat.shape[1]):
        h, s, v = colorsys.rgb_to_hsv(flat[0, k] / 255.0, flat[1, k] / 255.0, flat[2, k] / 255.0)
        h = (h + 2.0 * dh / 360.0) % 1.0
        s = min(max(s + ds / 255.0, 0.0), 1.0)
        v = min(max(v + dv / 255.0, 0.0), 1.0)
        oflat[:, k] = colorsys.hsv_to_rgb(h, s, v)
    return out * 255.0


def render64(params, composed, images, S):
    """params: ImageParams; composed: augment.compose's dicts; images: every source image (uint8 HWC BGR).
    -> ([B,3,S,S] float64, [B,S,S] float64 distance to the nearest frame / tile boundary, inf on the letterbox pad)"""
    out = np.empty((len(params), 3, S, S))
    dist = np.full((len(params), S, S), np.inf)
    ys, xs = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    for bi, (p, cpo) in enumerate(zip(params, composed)):
        _, nh, nw, top, left = cpo["letterbox"]
        fw, fh = cpo["frame"]
        inside = (ys >= top) & (ys < top + nh) & (xs >= left) & (xs < left + nw)
        M = cpo["M"]
        u = M[0, 0] * xs + M[0, 1] * ys + M[0, 2]
        v = M[1, 0] * xs + M[1, 1] * ys + M[1, 2]
        dd = np.minimum(np.minimum(np.abs(u), np.abs(u - fw)), np.minimum(np.abs(v), np.abs(v - fh)))
        inframe = inside & (u >= 0) & (u < fw) & (v >= 0) & (v < fh)
        c = np.full((3, S, S), 114.0)
        for si, x0, y0, x1, y1 in cpo["tiles"]:
            dd = np.minimum(dd, np.minimum(np.minimum(np.abs(u - x0), np.abs(u - x1)),
                                           np.minimum(np.abs(v - y0), np.abs(v - y1))))
            sel = inframe & (u >= x0) & (u < x1) & (v >= y0) & (v < y1)
            src = images[si].astype(np.float64)
            h0, w0 = src.shape[:2]
            fx = np.where(sel, (u - x0) * (w0 / (x1 - x0)) - 0.5, 0.0)
            fy = np.where(sel, (v - y0) * (h0 / (y1 - y0)) - 0.5, 0.0)
            ix, iy = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
            ax, ay = fx - ix, fy - iy
            xa, xb = np.clip(ix, 0, w0 - 1), np.clip(ix + 1, 0, w0 - 1)
            ya, yb = np.clip(iy, 0, h0 - 1), np.clip(iy + 1, 0, h0 - 1)
            val = ((src[ya, xa] * (1 - ax)[..., None] + src[ya, xb] * ax[..., None]) * (1 - ay)[..., None]
                   + (src[yb, xa] * (1 - ax)[..., None] + src[yb, xb] * ax[..., None]) * ay[..., None])     # [S,S,3] BGR
            rgb = val[..., ::-1].transpose(2, 0, 1)
            c = np.where(sel, rgb[list(p.perm)], c)
        dist[bi] = np.where(inside, dd, np.inf)
        mode, vals = p.color
        if mode == "brightness_contrast":
            c = np.where(inside, np.clip(vals[0] * c + vals[1] * 255.0, 0, 255), c)
        elif mode == "hsv_shift":
            c = np.where(inside, np.clip(_hsv64(c, *vals), 0, 255), c)
        elif mode == "rgb_shift":
            c = np.where(inside, np.clip(c + np.asarray(vals, np.float64)[:, None, None], 0, 255), c)
        if p.noise[0] > 0:
            n = noise_sums(int(p.noise[1]) & 0xFFFFFFFF, S).astype(np.float64) / 16777216.0 - 6.0
            c = np.where(inside, np.clip(c + p.noise[0] * n, 0, 255), c)
        mean, std = MEAN.astype(np.float64), STD.astype(np.float64)
        out[bi] = (c - mean[:, None, None] * 255.0) / (std[:, None, None] * 255.0)
    return out, dist
