"""The NumPy reference of draw_heatmaps: an independent painter written from the rule's text, not from csrc/draw_heat_arith.h (nothing
here reads that file, the library or centerpose_amd), and the seeded cases the CPU and GPU tests share.

The rule.  maps float32 [N, C, h, w], palette P: C (B, G, R) triples, opacity a in 1..256, invert.
1. Colour map per image and cell: m_k = max over c of float32(v_c * P[c][k]), from 0 and by '>': NaN never wins, negatives give 0;
   cm_k = min(255, int(m_k)).  invert: P -> 255 - P, then cm -> 255 - cm.
2. Position per frame pixel (x, y) with T (six doubles): mx = T0 x + T1 y + T2 left to right in double, clamped to [0, w - 1];
   X = int(mx * 256 + 0.5); ix = X >> 8, fx = X & 255, ix1 = min(ix + 1, w - 1); my with T3..T5 and h alike.
3. Sample per component, integer: t0 = a (256 - fx) + b fx on row iy, t1 on row iy1; f = (t0 (256 - fy) + t1 fy + 32768) >> 16.
4. Blend p' = (p (256 - a) + f a + 128) >> 8 on the three colour bytes.
5. 4:2:0 YUV: (B, G, R) -> (Y, U, V) by the limited-range forward forms; luma per pixel; a chroma sample with the (U, V) of the rounded
   mean (sum + (n >> 1)) // n of the fore colours of its n in-frame pixels."""
import numpy as np

import draw_ref

FORWARD = {"bt601": ((66, 129, 25), (-38, -74, 112), (112, -94, -18)), "bt709": ((47, 157, 16), (-26, -87, 112), (112, -102, -10))}


def forward_yuv(bgr, matrix):
    """int64 [..., 3] (B, G, R) -> int64 [..., 3] (Y, U, V); vectorised."""
    bgr = np.asarray(bgr, np.int64)
    b, g, r = bgr[..., 0], bgr[..., 1], bgr[..., 2]
    out = [((kr * r + kg * g + kb * b + 128) >> 8) + off for (kr, kg, kb), off in zip(FORWARD[matrix], (16, 128, 128))]
    return np.stack(out, axis=-1)


def colormap(maps, palette, invert):
    """maps float32 [C, h, w] -> int64 [h, w, 3]."""
    maps = np.asarray(maps, np.float32)
    P = np.asarray(palette, np.int64)[:maps.shape[0]]
    if invert:
        P = 255 - P
    h, w = maps.shape[1:]
    cm = np.zeros((h, w, 3), np.int64)
    with np.errstate(all="ignore"):
        for k in range(3):
            m = np.zeros((h, w), np.float32)
            for c in range(maps.shape[0]):
                t = maps[c] * np.float32(P[c, k])
                m = np.where(t > m, t, m)
            level = np.where(m >= np.float32(255.0), np.float32(255.0), m)          # +inf included; m is never NaN
            cm[..., k] = np.trunc(level).astype(np.int64)
    return 255 - cm if invert else cm


def _axis(t0, t1, t2, X, Y, n):
    m = np.float64(t0) * X + np.float64(t1) * Y
    m = m + np.float64(t2)
    with np.errstate(all="ignore"):
        m = np.where(m > 0.0, m, 0.0)
        m = np.where(m < float(n - 1), m, float(n - 1))
    q = np.floor(m * 256.0 + 0.5).astype(np.int64)              # m >= 0: floor is the truncation
    i0 = q >> 8
    return i0, np.minimum(i0 + 1, n - 1), q & 255


def fore(cm, T, H, W):
    """The sampled colour map of an H x W frame: int64 [H, W, 3] (B, G, R)."""
    h, w = cm.shape[:2]
    Y, X = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        ix, ix1, fx = _axis(T[0], T[1], T[2], X, Y, w)
        iy, iy1, fy = _axis(T[3], T[4], T[5], X, Y, h)
    fx, fy = fx[..., None], fy[..., None]
    t0 = cm[iy, ix] * (256 - fx) + cm[iy, ix1] * fx
    t1 = cm[iy1, ix] * (256 - fx) + cm[iy1, ix1] * fx
    return (t0 * (256 - fy) + t1 * fy + 32768) >> 16


def blend(p, f, a):
    return ((p.astype(np.int64) * (256 - a) + f * a + 128) >> 8).astype(np.uint8)


def reference(form, maps, T, palette, opacity, invert, matrix="bt601"):
    """The buffer of `form` after maps [C, h, w] have been blended over it with the frame -> map matrix T (a copy)."""
    buf = form["buf"].copy()
    views = draw_ref.numpy_views(buf, form)
    H, W = draw_ref.frame_size(form)
    f = fore(colormap(maps, palette, invert), np.asarray(T, np.float64).reshape(6), H, W)
    if form["color"] in ("bgr", "rgb"):
        hwc = views[0] if form["layout"] == "hwc" else views[0].transpose(1, 2, 0)
        for k in range(3):
            ch = k if form["color"] == "bgr" else 2 - k
            hwc[..., ch] = blend(hwc[..., ch], f[..., k], opacity)
        return buf
    y, u, v = draw_ref.yuv_planes(views, form["color"])
    y[...] = blend(y, forward_yuv(f, matrix)[..., 0], opacity)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    total = np.zeros((2 * ch, 2 * cw, 3), np.int64)
    count = np.zeros((2 * ch, 2 * cw), np.int64)
    total[:H, :W], count[:H, :W] = f, 1
    total = total.reshape(ch, 2, cw, 2, 3).sum(axis=(1, 3))
    n = count.reshape(ch, 2, cw, 2).sum(axis=(1, 3))[..., None]
    uv = forward_yuv((total + (n >> 1)) // n, matrix)
    u[...] = blend(u, uv[..., 1], opacity)
    v[...] = blend(v, uv[..., 2], opacity)
    return buf


# ------------------------------------------------------------------------------------------------------------------ shared cases
SPECIAL = np.array([0.0, 1.0, 1.5, -0.3, np.nan, np.inf, 0.25, 0.999], np.float32)


def fuzz_maps(seed, N, C, h, w):
    """float32 [N, C, h, w]: sparse blobs in [0, 1) with the special values (exact 0, exact 1.0, 1.5, -0.3, NaN, +inf) sprinkled in."""
    r = np.random.RandomState(seed)
    m = (r.uniform(0, 1, (N, C, h, w)) ** 3).astype(np.float32)
    where = r.uniform(0, 1, m.shape) < 0.12
    m[where] = SPECIAL[r.randint(0, len(SPECIAL), int(where.sum()))]
    return m


def fuzz_palette(seed, C):
    r = np.random.RandomState(seed)
    pal = r.randint(0, 256, (C, 3))
    pal[r.randint(0, C)] = (255, 0, 255)
    return [tuple(int(v) for v in c) for c in pal]


def fit_matrix(H, W, h, w):
    """The matrix a pre-process gives a frame that fills its map: map coordinate = pixel * (map side / frame side), plus a small shift
    so that fractions of every kind occur and both borders are crossed."""
    return [w / W * 1.07, 0.0, -0.21, 0.0, h / H * 1.05, -0.13]


OUTSIDE = [0.5, 0.0, 1.0e6, 0.0, 0.5, -1.0e6]                  # the whole frame right of and above the map: its corner cell everywhere

# (C, opacity, invert) of the styles every form is painted with
STYLES = [(1, 179, False), (17, 179, False), (17, 1, True), (1, 256, True), (17, 256, False)]
SIZES = [(37, 53), (70, 90), (16, 16), (1, 1)]
MAP_SIZES = [(8, 12), (5, 7)]
