"""The NumPy reference of the YUV -> BGR conversion that device frames in NV12 / NV21 / I420 go through (csrc/yuv_arith.h restates it
for the host and the device; nothing here reads that file or the library).  Integer-only, int64 here so that no intermediate can wrap:

    y = max(Y - YOFF, 0) * CY;  u = U - 128;  v = V - 128
    R = clamp((y + CVR*v         + 2^19) >> 20, 0, 255)
    G = clamp((y + CVG*v + CUG*u + 2^19) >> 20, 0, 255)
    B = clamp((y + CUB*u         + 2^19) >> 20, 0, 255)

with coef = (CY, CVR, CVG, CUG, CUB, YOFF), every entry round(k * 2^20), and the chroma of pixel (r, c) the sample (r >> 1, c >> 1)."""
import numpy as np

COEF = {"bt601": (1220542, 1673527, -852492, -409993, 2116026, 16),       # 1.164, 1.596, -0.813, -0.391, 2.018 (limited range)
        "bt709": (1220542, 1880097, -558891, -223347, 2214593, 16)}       # 1.164, 1.793, -0.533, -0.213, 2.112 (limited range)

# (Y, U, V) -> (B, G, R) under "bt601", worked by hand
ANCHORS = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((81, 90, 240), (0, 0, 254)), ((145, 54, 34), (1, 255, 0)),
           ((41, 240, 110), (255, 0, 0))]


def to_bgr(y, u, v, coef):
    """uint8 arrays of one shape -> uint8 [..., 3] in B, G, R order."""
    cy, cvr, cvg, cug, cub, yoff = (int(c) for c in coef)
    y = np.maximum(np.asarray(y).astype(np.int64) - yoff, 0) * cy
    u = np.asarray(u).astype(np.int64) - 128
    v = np.asarray(v).astype(np.int64) - 128
    half = 1 << 19
    r = (y + cvr * v + half) >> 20                            # numpy's >> on signed integers is arithmetic
    g = (y + cvg * v + cug * u + half) >> 20
    b = (y + cub * u + half) >> 20
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def frame_to_bgr(planes, color, matrix="bt601"):
    """Host uint8 planes of one 4:2:0 frame -> the HxWx3 BGR array it converts to.  planes: (y [H,W], uv [ceil(H/2),ceil(W/2),2]) for
    "nv12" (uv[..., 0] is U) / "nv21" (uv[..., 0] is V), (y, u, v) for "i420".  Chroma is up-sampled by index >> 1."""
    y = np.asarray(planes[0])
    if color == "nv12":
        u, v = planes[1][..., 0], planes[1][..., 1]
    elif color == "nv21":
        v, u = planes[1][..., 0], planes[1][..., 1]
    else:
        assert color == "i420"
        u, v = planes[1], planes[2]
    H, W = y.shape
    assert u.shape == v.shape == ((H + 1) // 2, (W + 1) // 2)
    r, c = np.arange(H) >> 1, np.arange(W) >> 1
    return to_bgr(y, np.asarray(u)[r][:, c], np.asarray(v)[r][:, c], COEF[matrix])
