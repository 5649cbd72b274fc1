"""The independent reference of the 3-D face stage (nothing here reads csrc/face_arith.h or the library):

* the selection, crop and restore rules in NumPy float32 -- `square`, `select`, `crop`, `restore` -- and the restore in float64;
* PRNet as a functional torch statement -- `net`, from the layer list of demo/face/resfcn256.py (every BatchNorm has eps 1e-3);
* the seeded inputs of the recorded maps (`make_input`) and the hand-built selection cases.

The rule restates PRN.process (demo/face/prnet.py:83-117) in closed form; skimage (estimate_transform, warp) is not available to this
project, so the crop is NOT pinned to a recording of it.  Box (left, right, top, bottom): the min / max of the five face joints
(floats 5..14 of a row) or a given (x1, y1, x2, y2, score) read as left = x1, right = x2, top = y1, bottom = y2;
old_size = ((right - left) + bottom - top) / 2, size = int(old_size * expand), cx = right - (right - left) / 2, cy alike,
x0 = cx - size / 2, y0 = cy - size / 2; selected iff score > vis_thresh, every coordinate finite and min_size <= size <= 32768.
Crop pixel (u, v): x = x0 + u * (size / 255), y = y0 + v * (size / 255); bilinear over (floor, floor + 1), a neighbour outside the
frame contributing 0; / 255; channels R, G, B.  Restore: P = out * 281.6; x = P_x * (size / 255) + x0, y alike, z = P_z * (size / 255).
All float32, one rounding per operation."""
import numpy as np
import torch
import torch.nn.functional as F

import draw_ref
import reid_ref

RES, NKPT, MAX_SIZE = 256, 68, 32768
BN_EPS = 1e-3
f32 = np.float32


# ---- selection ---------------------------------------------------------------------------------------------------------------------
def square(left, right, top, bottom, expand=1.6, min_size=1):
    """-> (x0, y0, size) float32 or None."""
    left, right, top, bottom = f32(left), f32(right), f32(top), f32(bottom)
    if not np.isfinite([left, right, top, bottom]).all():
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        w, h = f32(right - left), f32(bottom - top)
        old = f32(f32(f32(w + bottom) - top) / f32(2))
        fs = f32(old * f32(expand))
        if not (fs >= f32(min_size) and fs < f32(MAX_SIZE + 1)):
            return None
        size = int(fs)
        cx, cy = f32(right - f32(w / f32(2))), f32(bottom - f32(h / f32(2)))
        half = f32(f32(size) / f32(2))
        return f32(cx - half), f32(cy - half), f32(size)


def candidate(c, boxes, vis_thresh, expand=1.6, min_size=1):
    c = np.asarray(c, f32)
    if not (c[4] > f32(vis_thresh)):
        return None
    if boxes:
        return square(c[0], c[2], c[1], c[3], expand, min_size)
    xs, ys = c[5:15:2], c[6:15:2]
    if not np.isfinite(c[5:15]).all():
        return None
    return square(xs.min(), xs.max(), ys.min(), ys.max(), expand, min_size)


def select(cand, boxes, vis_thresh, cap, expand=1.6, min_size=1):
    """cand [N, M, 56 or 5] -> (slots int32 [cap], counts int32 [N], xform float32 [cap, 3])."""
    N, M = cand.shape[:2]
    q = cap // N
    slots, counts, xform = np.full(cap, -1, np.int32), np.zeros(N, np.int32), np.zeros((cap, 3), f32)
    for n in range(N):
        c = 0
        for m in range(M):
            t = candidate(cand[n, m], boxes, vis_thresh, expand, min_size)
            if t is None:
                continue
            if c < q:
                slots[n * q + c] = n * M + m
                xform[n * q + c] = t
            c += 1
        counts[n] = c
    return slots, counts, xform


# ---- crop --------------------------------------------------------------------------------------------------------------------------
def _axis(origin, size, n):
    """-> (first neighbour, its validity, the second's validity, weight of the second) for the 256 output positions."""
    step = f32(f32(size) / f32(255))
    x = (f32(origin) + np.arange(RES, dtype=f32) * step).astype(f32)
    ok = (x > f32(-1)) & (x < f32(n))
    fl = np.floor(np.where(ok, x, f32(0))).astype(f32)
    i = fl.astype(np.int64)
    f = np.where(ok, (x - fl).astype(f32), f32(0)).astype(f32)
    return i, ok & (i >= 0), ok & (i + 1 < n), f


def crop(bgr, t):
    """bgr uint8 [H, W, 3], t = (x0, y0, size) -> float32 [3, 256, 256] in R, G, B order."""
    H, W = bgr.shape[:2]
    ix, x_in0, x_in1, a = _axis(t[0], t[2], W)
    iy, y_in0, y_in1, b = _axis(t[1], t[2], H)
    img = bgr[..., ::-1].astype(f32)

    def tap(yy, y_ok, xx, x_ok):
        v = img[np.clip(yy, 0, H - 1)][:, np.clip(xx, 0, W - 1)]
        return np.where((y_ok[:, None] & x_ok[None, :])[..., None], v, f32(0)).astype(f32)
    a3, b3 = a[None, :, None], b[:, None, None]
    one = f32(1)
    top = (tap(iy, y_in0, ix, x_in0) * (one - a3) + tap(iy, y_in0, ix + 1, x_in1) * a3).astype(f32)
    bot = (tap(iy + 1, y_in1, ix, x_in0) * (one - a3) + tap(iy + 1, y_in1, ix + 1, x_in1) * a3).astype(f32)
    v = ((top * (one - b3) + bot * b3).astype(f32) / f32(255)).astype(f32)
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def crops(pictures, slots, xform, M):
    """pictures: N B, G, R arrays -> float32 [cap, 3, 256, 256], zeros in unused slots."""
    out = np.zeros((len(slots), 3, RES, RES), f32)
    for s, idx in enumerate(slots):
        if idx >= 0:
            out[s] = crop(pictures[int(idx) // M], xform[s])
    return out


def crop_scipy(bgr, t):
    """The same sampling by scipy.ndimage.map_coordinates(order=1, mode='grid-constant') in float64 -> [3, 256, 256]."""
    from scipy import ndimage
    step = np.float64(t[2]) / 255.0
    xs, ys = np.float64(t[0]) + np.arange(RES) * step, np.float64(t[1]) + np.arange(RES) * step
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    return np.stack([ndimage.map_coordinates(bgr[..., 2 - k].astype(np.float64) / 255.0, [yy, xx], order=1, mode="grid-constant", cval=0.0)
                     for k in range(3)])


# ---- restore -----------------------------------------------------------------------------------------------------------------------
def restore(net, slots, xform, uv, dtype=f32):
    """net [cap, 3, 256, 256] -> (pos [cap, 256, 256, 3], landmarks [cap, 68, 3]) in `dtype` (float32: the rule, one rounding per
    operation; float64: prnet.py:106-126 evaluated exactly on the float32 inputs)."""
    cap = net.shape[0]
    pos = np.zeros((cap, RES, RES, 3), dtype)
    for s in range(cap):
        if slots[s] < 0:
            continue
        x0, y0, size = (dtype(v) for v in xform[s])
        step = dtype(size / dtype(255))
        gain = dtype(f32(256) * f32(1.1)) if dtype is f32 else dtype(256 * 1.1)
        P = (net[s].astype(dtype) * gain).astype(dtype)
        pos[s, ..., 0] = (P[0] * step).astype(dtype) + x0
        pos[s, ..., 1] = (P[1] * step).astype(dtype) + y0
        pos[s, ..., 2] = (P[2] * step).astype(dtype)
    return pos, np.ascontiguousarray(pos[:, uv[1], uv[0], :])


# ---- the net -----------------------------------------------------------------------------------------------------------------------
def _bn(x, sd, p):
    g, b, m, v = (sd[p + s].to(x.dtype) for s in (".weight", ".bias", ".running_mean", ".running_var"))
    return (x - m.view(1, -1, 1, 1)) / torch.sqrt(v.view(1, -1, 1, 1) + BN_EPS) * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def _same4(x, w, stride):
    """padding_same_conv2d(k4): stride 1 pads (1, 2), stride 2 pads (1, 1)."""
    return F.conv2d(F.pad(x, (1, 2, 1, 2)) if stride == 1 else F.pad(x, (1, 1, 1, 1)), w, None, stride)


def _tconv1(x, w):
    """ConstantPad2d((2, 1, 2, 1)) + ConvTranspose2d(k4, s1, p3)."""
    return F.conv_transpose2d(F.pad(x, (2, 1, 2, 1)), w, None, 1, 3)


def net(sd, x, taps=None):
    """x [B, 3, H, W] -> [B, 3, H, W] after the sigmoid, in x.dtype.  taps: a dict that receives the activation after every layer
    (NCHW), keyed by the conv's parameter name."""
    w = lambda k: sd[k + ".weight"].to(x.dtype)
    note = (lambda k, t: taps.__setitem__(k, t)) if taps is not None else (lambda k, t: None)
    x = F.relu(_bn(_same4(x, w("input_conv.1"), 1), sd, "input_conv.2"))
    note("input_conv.1", x)
    for i, stride in enumerate((2, 1, 2, 1, 2, 1, 2, 1, 2, 1), start=1):
        p = "down_conv_%d" % i
        c2, c3 = (3, 6) if stride == 2 else (4, 7)
        h = F.relu(_bn(F.conv2d(x, w(p + ".main.0")), sd, p + ".main.1"))
        note(p + ".main.0", h)
        h = F.relu(_bn(_same4(h, w("%s.main.%d" % (p, c2)), stride), sd, "%s.main.%d" % (p, c2 + 1)))
        note("%s.main.%d" % (p, c2), h)
        h = F.conv2d(h, w("%s.main.%d" % (p, c3)))
        sc = F.conv2d(x, w(p + ".shortcut"), None, stride) if stride == 2 else x
        x = F.relu(_bn(sc + h, sd, p + ".activate.0"))
        note("%s.main.%d" % (p, c3), x)
    x = F.relu(_bn(_tconv1(x, w("center_conv.1")), sd, "center_conv.2"))
    note("center_conv.1", x)
    for i, n in ((5, 2), (4, 2), (3, 2), (2, 1), (1, 1)):
        p = "up_conv_%d.main." % i
        x = F.relu(_bn(F.conv_transpose2d(x, w(p + "0"), None, 2, 1), sd, p + "1"))
        note(p + "0", x)
        for j in range(n):
            x = F.relu(_bn(_tconv1(x, w(p + str(4 * j + 4))), sd, p + str(4 * j + 5)))
            note(p + str(4 * j + 4), x)
    x = F.relu(_bn(_tconv1(x, w("output_conv.1")), sd, "output_conv.2"))
    note("output_conv.1", x)
    x = F.relu(_bn(_tconv1(x, w("output_conv.5")), sd, "output_conv.6"))
    note("output_conv.5", x)
    x = torch.sigmoid(_bn(_tconv1(x, w("output_conv.9")), sd, "output_conv.10"))
    note("output_conv.9", x)
    return x


def make_input(seed, H, W):
    """A seeded picture-like input float32 [3, H, W] in 0..1: smooth waves of a few periods, some rectangles and a little noise (what
    tools/make_prnet_golden.py records the module on; never stored)."""
    r = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64) / H, np.arange(W, dtype=np.float64) / W, indexing="ij")
    img = np.zeros((3, H, W))
    for c in range(3):
        for _ in range(4):
            fy, fx, ph, amp = r.uniform(0.5, 4), r.uniform(0.5, 4), r.uniform(0, 2 * np.pi), r.uniform(0.1, 0.3)
            img[c] += amp * np.cos(2 * np.pi * (fy * yy + fx * xx) + ph)
    for _ in range(6):
        y0, x0 = r.randint(0, H - 4), r.randint(0, W - 4)
        h, w = r.randint(2, max(3, H // 3)), r.randint(2, max(3, W // 3))
        img[:, y0:y0 + h, x0:x0 + w] += r.uniform(-0.5, 0.5, (3, 1, 1))
    img = 0.5 + img + r.uniform(-0.05, 0.05, img.shape)
    return np.clip(img, 0, 1).astype(f32)


# ---- hand-built selection cases ----------------------------------------------------------------------------------------------------
VIS = 0.3


def joints_row(left, right, top, bottom, score=1.0):
    """A detection row whose five face joints span exactly (left, right, top, bottom)."""
    r = np.zeros(56, f32)
    r[4] = score
    mx, my = (f32(left) + f32(right)) / f32(2), (f32(top) + f32(bottom)) / f32(2)
    pts = [(mx, my), (left, top), (right, bottom), (left, bottom), (right, top)]
    if left == right and top == bottom:
        pts = [(left, top)] * 5
    r[5:15] = np.asarray(pts, f32).reshape(-1)
    r[0:4] = (left, top, right, bottom)
    return r


def box_of(left, right, top, bottom, score=1.0):
    return np.asarray([left, top, right, bottom, score], f32)


def select_cases(boxes):
    """cand [3, 7, 56 | 5]: frame 0 -- selected, score at the threshold (not), one float above it (selected), NaN score (not), a NaN
    joint (not), size 0 (not), size exactly 1 (selected); frame 1 -- size above 32768 (not), size 32768 (selected), an infinite
    coordinate (not), four more selected (a capacity overflow); frame 2 -- nothing selected."""
    mk = (lambda l, r, t, b, s=1.0: box_of(l, r, t, b, s)) if boxes else joints_row
    above = float(np.nextafter(f32(VIS), f32(1)))
    nanj = mk(10, 50, 10, 50)
    nanj[1 if boxes else 8] = np.nan
    infc = mk(10, 50, 10, 50)
    infc[2 if boxes else 9] = np.inf
    f0 = [mk(10, 50, 20, 60), mk(10, 50, 20, 60, VIS), mk(12.5, 50.25, 20, 61, above), mk(10, 50, 20, 60, float("nan")), nanj,
          mk(30, 30, 40, 40), mk(30, 30.625, 40, 40.625)]                 # old_size 0.625 * 1.6 = 1.0
    f1 = [mk(0, 20481, 0, 20481), mk(0, 20480, 0, 20480), infc, mk(-5, 30, -8, 40), mk(100, 140, 90, 150), mk(3, 9, 3, 9), mk(60, 90, 10, 45)]
    f2 = [mk(10, 50, 20, 60, 0.0), mk(10, 50, 20, 60, -1.0)] + [mk(30, 30, 40, 40)] * 5
    return np.stack([np.stack(f) for f in (f0, f1, f2)]).astype(f32)


# ---- crop cases --------------------------------------------------------------------------------------------------------------------
def crop_boxes(H, W):
    """(left, right, top, bottom): inside, straddling each border, wholly outside, size 1, larger than the frame, a fractional centre."""
    return [(10, 30, 8, 24), (-14, 10, 6, 26), (W - 12, W + 9, 5, 20), (12, 30, -9, 7), (9, 31, H - 8, H + 11), (W + 40, W + 70, 5, 30),
            (20, 20.625, 11, 11.625), (-30, W + 25, -20, H + 40), (10.3, 31.45, 7.7, 25.15)]


def crop_cases():
    """[(name, forms, matrix)]: the forms of tests/draw_ref.py on odd 37 x 53 frames."""
    H, W = 37, 53
    b, y = draw_ref.bgr_forms(1200, H, W), draw_ref.yuv_forms(1230, H, W)
    return [("hwc bgr + hwc rgb4", [b[0], b[1]], "bt601"), ("bgra padded + chw rgb", [b[2], b[3]], "bt601"),
            ("chw bgr4 padded + roi rgb", [b[4], b[5]], "bt601"), ("nv12 pitched odd + nv21 pitched", [reid_ref.nv12_pitched_odd(1240, H, W), y[1]], "bt601"),
            ("i420 + i420 interleaved views, bt709", [y[2], y[3]], "bt709")]


def case_candidates(forms):
    """boxes [N, 9, 5] over the frames of a case and the capacity that leaves one slot unused"""
    H, W = draw_ref.frame_size(forms[0])
    boxes = np.stack([np.stack([box_of(*b) for b in crop_boxes(H, W)]) for _ in forms]).astype(np.float32)
    return boxes, len(forms) * 10



SELECT_EXPECT = {        # cap -> slots (n * 7 + m)
    6: [0, 2, 8, 10, -1, -1],                 # q = 2: frame 0 drops row 6, frame 1 drops rows 4, 5, 6; counts stay uncapped
    3: [0, 8, -1],
    7: [0, 2, 8, 10, -1, -1, -1],             # cap % N != 0: the slot beyond N * q is unused
    21: [0, 2, 6, -1, -1, -1, -1, 8, 10, 11, 12, 13, -1, -1, -1, -1, -1, -1, -1, -1, -1],
}
SELECT_COUNTS = [3, 5, 0]
