"""The NumPy reference of YUV device frames beyond 8-bit 4:2:0 limited range: P010 / P016, planar 4:2:2 and 4:4:4, grey, packed
YUYV / UYVY, the full-range and BT.2020 matrices (csrc/yuv_source.h restates it for the host and the device; nothing here reads that
file or the library).  Integer-only, int64, arithmetic shifts.

8-bit samples (tests/yuv_ref.py's rule, restated):   y = max(Y - YOFF, 0) * CY;  u = U - 128;  v = V - 128;  (... + 2^19) >> 20
16-bit samples, the container value as stored:       y = max(Y - 256 * YOFF, 0) * CY;  u = U - 32768;  v = V - 32768;  (... + 2^27) >> 28
    R = clamp(y + CVR*v), G = clamp(y + CVG*v + CUG*u), B = clamp(y + CUB*u)
The chroma of pixel (r, c) is the sample (r >> sy, c >> sx): (sx, sy) = (1, 1) for 4:2:0, (1, 0) for 4:2:2, (0, 0) for 4:4:4; a grey
frame has U = V = 128.  A matrix is (CY, CVR, CVG, CUG, CUB, YOFF), every entry round(k * 2^20), k in double from (Kr, Kb)."""
import numpy as np


def closed_form(kr, kb, full):
    kg = 1.0 - kr - kb
    l, c, yoff = (1.0, 1.0, 0) if full else (255.0 / 219.0, 255.0 / 224.0, 16)
    ks = (l, 2.0 * (1.0 - kr) * c, -2.0 * kr * (1.0 - kr) / kg * c, -2.0 * kb * (1.0 - kb) / kg * c, 2.0 * (1.0 - kb) * c)
    return tuple(int(round(k * (1 << 20))) for k in ks) + (yoff,)


LUMA = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
NEW_COEF = {"bt601-full": closed_form(*LUMA["bt601"], True), "bt709-full": closed_form(*LUMA["bt709"], True),
            "bt2020-limited": closed_form(*LUMA["bt2020"], False), "bt2020-full": closed_form(*LUMA["bt2020"], True)}
# the two rows that were there before: cv2's three-decimal constants, not the closed form
COEF = dict(NEW_COEF, **{"bt601": (1220542, 1673527, -852492, -409993, 2116026, 16), "bt709": (1220542, 1880097, -558891, -223347, 2214593, 16)})

COLORS = ("p010", "p016", "i422", "i444", "i400", "yuyv", "uyvy")
SHIFTS = {"nv12": (1, 1), "nv21": (1, 1), "i420": (1, 1), "p010": (1, 1), "p016": (1, 1), "i422": (1, 0), "yuyv": (1, 0), "uyvy": (1, 0),
          "i444": (0, 0)}


def _convert(y, u, v, coef, yoff_scale, mid, shift):
    cy, cvr, cvg, cug, cub, yoff = (int(c) for c in coef)
    y = np.maximum(np.asarray(y).astype(np.int64) - yoff_scale * yoff, 0) * cy
    u = np.asarray(u).astype(np.int64) - mid
    v = np.asarray(v).astype(np.int64) - mid
    half = 1 << (shift - 1)
    r = (y + cvr * v + half) >> shift
    g = (y + cvg * v + cug * u + half) >> shift
    b = (y + cub * u + half) >> shift
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def to_bgr8(y, u, v, coef):
    """uint8 arrays of one shape -> uint8 [..., 3] in B, G, R order."""
    return _convert(y, u, v, coef, 1, 128, 20)


def to_bgr16(y, u, v, coef):
    """uint16 arrays of one shape (container values, low bits and all) -> uint8 [..., 3] in B, G, R order."""
    return _convert(y, u, v, coef, 256, 32768, 28)


def samples(planes, color):
    """Host planes of one frame -> (y, u, v) arrays, the chroma as stored (not up-sampled); u = v = None for grey.
    planes: (y, uv [.., .., 2]) for nv12 / p010 / p016 (uv[..., 0] is U) and nv21 (V first), (y, u, v) for i420 / i422 / i444, (y,) for
    i400, (packed [H, W, 2],) for yuyv / uyvy."""
    if color in ("nv12", "p010", "p016"):
        return np.asarray(planes[0]), planes[1][..., 0], planes[1][..., 1]
    if color == "nv21":
        return np.asarray(planes[0]), planes[1][..., 1], planes[1][..., 0]
    if color in ("i420", "i422", "i444"):
        return tuple(np.asarray(p) for p in planes)
    if color == "i400":
        return np.asarray(planes[0]), None, None
    p, lum = np.asarray(planes[0]), ("yuyv", "uyvy").index(color)
    return p[:, :, lum], p[:, 0::2, 1 - lum], p[:, 1::2, 1 - lum]


def frame_to_bgr(planes, color, matrix):
    """Host planes of one frame -> the HxWx3 BGR array it converts to: index arithmetic for the chroma, then the rule per pixel."""
    y, u, v = samples(planes, color)
    H, W = y.shape
    wide = y.dtype.itemsize == 2
    assert wide == (color in ("p010", "p016")) and y.dtype in (np.uint8, np.uint16)
    if u is None:
        u = v = np.full((H, W), 128, np.uint8)
    else:
        sx, sy = SHIFTS[color]
        assert u.shape == v.shape == (((H - 1) >> sy) + 1, ((W - 1) >> sx) + 1) and u.dtype == v.dtype == y.dtype
        r, c = np.arange(H) >> sy, np.arange(W) >> sx
        u, v = u[r][:, c], v[r][:, c]
    return (to_bgr16 if wide else to_bgr8)(y, u, v, COEF[matrix])


def random_planes(seed, color, h, w):
    """Random host planes of one frame of the given colour (the forms `samples` takes), every bit of every sample random."""
    rs = np.random.RandomState(seed)
    dt = np.uint16 if color in ("p010", "p016") else np.uint8
    rnd = lambda *shape: rs.randint(0, 1 << (8 * np.dtype(dt).itemsize), size=shape).astype(dt)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if color in ("nv12", "nv21", "p010", "p016"):
        return rnd(h, w), rnd(ch, cw, 2)
    if color == "i420":
        return rnd(h, w), rnd(ch, cw), rnd(ch, cw)
    if color == "i422":
        return rnd(h, w), rnd(h, cw), rnd(h, cw)
    if color == "i444":
        return rnd(h, w), rnd(h, w), rnd(h, w)
    if color == "i400":
        return (rnd(h, w),)
    assert color in ("yuyv", "uyvy") and w % 2 == 0
    return (rnd(h, w, 2),)
