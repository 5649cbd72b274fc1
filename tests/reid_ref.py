"""The independent reference of the re-id stage (nothing here reads csrc/reid_arith.h or the library):

* the box, slot and crop rules in NumPy -- `box`, `select`, `crop`, `crops`;
* the re-id net as a functional torch statement in float64 -- `net`, from the layer list of demo/tracking/model.py (Net(reid=True):
  3x3 stem conv + BN + ReLU + 3x3/s2 max-pool, four stages of two BasicBlocks, AvgPool2d((8, 4)), x / ||x||_2);
* the forms (buffers + views) the crop tests run on and their B, G, R pictures.

Box: coordinates clamped to +-2^30 and truncated toward zero; w = x2 - x1, h = y2 - y1; X1 = max(x1, 0), Y1 = max(y1, 0),
X2 = min(X1 + w, W - 1), Y2 = min(Y1 + h, H - 1); crop = rows Y1..Y2-1, columns X1..X2-1; selected iff score > vis_thresh, no NaN
coordinate and a non-empty crop.  Resize: fx = (o + 0.5) * (n / N) - 0.5 in double, s = floor(fx), f = float32(fx - s); s < 0 -> tap 0
alone; s >= n - 1 -> tap n - 1 alone; blend horizontal then vertical in double with the float32 weights (1 - f, f), rounded to float32;
then (v * scale - mean[k]) / std[k] in float32."""
import numpy as np
import torch
import torch.nn.functional as F

import draw_ref
import yuv_ref

OUT_H, OUT_W, DIM = 128, 64, 512
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
LIM = 2 ** 30


# ---- box and slots -----------------------------------------------------------------------------------------------------------------
def box(row, H, W, vis_thresh):
    """-> (X1, Y1, X2, Y2) of the crop (exclusive ends) or None when the row gets no embedding."""
    if not (np.float32(row[4]) > np.float32(vis_thresh)):
        return None
    c = np.asarray(row[:4], np.float64)
    if np.isnan(c).any():
        return None
    x1, y1, x2, y2 = (int(v) for v in np.trunc(np.clip(c, -LIM, LIM)))
    w, h = x2 - x1, y2 - y1
    X1, Y1 = max(x1, 0), max(y1, 0)
    X2, Y2 = min(X1 + w, W - 1), min(Y1 + h, H - 1)
    if X2 <= X1 or Y2 <= Y1:
        return None
    return X1, Y1, X2, Y2


def select(rows, sizes, vis_thresh, cap):
    """rows [N, M, 56], sizes [(H, W)] * N -> (slots int32 [cap], counts int32 [N])."""
    N, M = rows.shape[:2]
    q = cap // N
    slots, counts = np.full(cap, -1, np.int32), np.zeros(N, np.int32)
    for n in range(N):
        c = 0
        for m in range(M):
            if box(rows[n, m], sizes[n][0], sizes[n][1], vis_thresh) is None:
                continue
            if c < q:
                slots[n * q + c] = n * M + m
            c += 1
        counts[n] = c
    return slots, counts


# ---- crop --------------------------------------------------------------------------------------------------------------------------
def taps(n, N):
    o = np.arange(N, dtype=np.float64)
    fx = (o + 0.5) * (np.float64(n) / np.float64(N)) - 0.5
    s = np.floor(fx)
    f = (fx - s).astype(np.float32)
    s = s.astype(np.int64)
    lo = s < 0
    s = np.where(lo, 0, s)
    hi = s >= n - 1                                           # (a one-pixel axis: tap 0 is also the last tap)
    s = np.where(hi, n - 1, s)
    f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    return s, np.where(hi, s, s + 1), f


def crop(bgr, b, scale=1.0, mean=MEAN, std=STD, channel_order="bgr"):
    """bgr uint8 [H, W, 3], b = box(...) -> float32 [3, 128, 64]."""
    X1, Y1, X2, Y2 = b
    patch = bgr[Y1:Y2, X1:X2].astype(np.float64)
    x0, x1, fx = taps(X2 - X1, OUT_W)
    y0, y1, fy = taps(Y2 - Y1, OUT_H)
    ax0, ax1 = (np.float32(1) - fx).astype(np.float64)[None, :, None], fx.astype(np.float64)[None, :, None]
    ay0, ay1 = (np.float32(1) - fy).astype(np.float64)[:, None, None], fy.astype(np.float64)[:, None, None]
    top = patch[y0][:, x0] * ax0 + patch[y0][:, x1] * ax1
    bot = patch[y1][:, x0] * ax0 + patch[y1][:, x1] * ax1
    v = (top * ay0 + bot * ay1).astype(np.float32)
    if channel_order == "rgb":
        v = v[..., ::-1]
    out = np.empty((3, OUT_H, OUT_W), np.float32)
    for k in range(3):
        out[k] = (v[..., k] * np.float32(scale) - np.float32(mean[k])) / np.float32(std[k])
    return out


def crops(pictures, rows, vis_thresh, cap, **norm):
    """pictures: N B, G, R arrays; rows [N, M, 56] -> (x float32 [cap, 3, 128, 64] with zeros in unused slots, slots, counts)."""
    N, M = rows.shape[:2]
    slots, counts = select(rows, [p.shape[:2] for p in pictures], vis_thresh, cap)
    x = np.zeros((cap, 3, OUT_H, OUT_W), np.float32)
    for s, idx in enumerate(slots):
        if idx >= 0:
            n, m = divmod(int(idx), M)
            x[s] = crop(pictures[n], box(rows[n, m], pictures[n].shape[0], pictures[n].shape[1], vis_thresh), **norm)
    return x, slots, counts


# ---- forms -------------------------------------------------------------------------------------------------------------------------
def picture(form, matrix="bt601", buf=None):
    """The H x W x 3 B, G, R picture a form of tests/draw_ref.py (a buffer and the views of its planes) shows."""
    views = draw_ref.numpy_views(form["buf"] if buf is None else buf, form)
    if form["color"] in ("bgr", "rgb"):
        v = views[0] if form["layout"] == "hwc" else views[0].transpose(1, 2, 0)
        v = v[..., :3]
        return np.ascontiguousarray(v if form["color"] == "bgr" else v[..., ::-1])
    y, u, v = draw_ref.yuv_planes(views, form["color"])
    r, c = np.arange(y.shape[0]) >> 1, np.arange(y.shape[1]) >> 1
    return yuv_ref.to_bgr(y, u[r][:, c], v[r][:, c], yuv_ref.COEF[matrix])


def nv12_pitched_odd(seed, H, W):
    """NV12 planes with odd H and W and both pitches wider than the picture."""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    return draw_ref._form(seed, "nv12 planes, pitched, odd", "hwc", "nv12",
                          [(0, (H, W), (W + 11, 1)), (H * (W + 11) + 5, (ch, cw, 2), (2 * cw + 10, 2, 1))])


def row(x1, y1, x2, y2, score=1.0):
    r = np.zeros(56, np.float32)
    r[:5] = (x1, y1, x2, y2, score)
    return r


def _rows(per_frame, M):
    out = np.zeros((len(per_frame), M, 56), np.float32)
    for n, rs in enumerate(per_frame):
        for m, r in enumerate(rs):
            out[n, m] = r
    return out


def crop_cases():
    """[(name, forms, rows [N, M, 56], matrix, norm kwargs)]: every frame layout, both matrices, enlarging and shrinking crops, boxes
    off every edge, unused slots; frames of at most 240 x 320, to be run at cap = 4 and VIS."""
    H, W = 37, 53
    b = draw_ref.bgr_forms(900, H, W)
    y = draw_ref.yuv_forms(930, H, W)
    ye = draw_ref.yuv_forms(960, 64, 64)
    small = [row(10, 7, 15.9, 10.2), row(-6.5, -3, 20, 30, 0.31), row(3, 3, 9, 9, 0.3)]              # 5 x 3 pixels; off the top left; score == VIS
    edges = [row(40, 20, 70, 60), row(0, 0, 52, 36), row(20.5, 30.2, 21.9, 99)]                      # off the bottom right; the whole frame; one column
    big = draw_ref._form(990, "hwc bgr 240 x 320", "hwc", "bgr", [(0, (320, 240, 3), (720, 3, 1))])
    return [
        ("bgr + rgb4: enlarging, unused slot", [b[0], b[1]], _rows([small, edges[:1]], 3), "bt601", {}),
        ("chw rgb, chw bgr4 padded, roi rgb, bgra padded", [b[3], b[4], b[5], b[2]], _rows([edges[1:2], edges[2:], small[1:2], edges[:1]], 1), "bt601", {}),
        ("shrinking 200 x 300 of 240 x 320", [big], _rows([[row(20, 10, 220, 310), row(0, 0, 1e9, 1e9), row(-50, 100, 130, 200)]], 3), "bt601", {}),
        ("nv12 pitched odd + nv21 pitched, bt601", [nv12_pitched_odd(940, H, W), y[1]], _rows([small, edges], 3), "bt601", {}),
        ("i420 + i420 interleaved views, bt709", [y[2], y[3]], _rows([edges, small], 3), "bt709", {}),
        ("nv12 surface pitched + nv21 surface, bt709", [ye[4], ye[5]], _rows([[row(1, 1, 63, 63), row(30, 31, 64, 64)], [row(0, 0, 6, 4)]], 2), "bt709", {}),
        ("rgb order, scale 1/255", [b[0], b[1]], _rows([small, edges[:1]], 3), "bt601", dict(channel_order="rgb", scale=1.0 / 255.0)),
    ]


VIS, CAP = 0.3, 4


def slot_rows():
    """N = 3, M = 7 on 100 x 200 frames: frame 0 selects rows 0, 2, 3, 5; frame 1 none; frame 2 row 6."""
    sel, thr, nan, empty = row(10, 10, 50, 50), row(10, 10, 50, 50, 0.3), row(10, 10, 50, 50, float("nan")), row(250, 10, 300, 50)
    f0 = [sel, thr, row(-10, 20, 30, 60), row(20.5, 30.2, 21.9, 99), nan, row(180, 10, 230, 50, 0.31), empty]
    f1 = [thr, nan, empty, row(50, 10, 50, 40), row(10, float("nan"), 50, 50), row(10, 10, 50, 50, -1.0), row(10, 10, 50, 50, 0.0)]
    f2 = [empty] * 6 + [sel]
    return np.stack([np.stack(f) for f in (f0, f1, f2)]).astype(np.float32)


SLOT_CASES = [(6, [0, 2, -1, -1, 20, -1]),         # q = 2: rows 3 and 5 of frame 0 are dropped, counts stay uncapped
              (3, [0, -1, 20]),                    # N == cap: q = 1
              (7, [0, 2, -1, -1, 20, -1, -1]),     # cap % N != 0: the slot beyond N * q is unused
              (13, [0, 2, 3, 5, -1, -1, -1, -1, 20, -1, -1, -1, -1])]


# ---- the net -----------------------------------------------------------------------------------------------------------------------
def _bn(x, sd, p, eps=1e-5):
    g, b, m, v = (sd[p + s].to(x.dtype) for s in (".weight", ".bias", ".running_mean", ".running_var"))
    return (x - m.view(1, -1, 1, 1)) / torch.sqrt(v.view(1, -1, 1, 1) + eps) * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def net(sd, x, taps=None):
    """x [B, 3, 128, 64] -> unit-norm features [B, 512], in x.dtype (float64 for the reference).  taps: a dict that receives the
    activation after every layer (NCHW), keyed by the conv's parameter name."""
    w = lambda k: sd[k].to(x.dtype)
    note = (lambda k, t: taps.__setitem__(k, t)) if taps is not None else (lambda k, t: None)
    x = F.relu(_bn(F.conv2d(x, w("conv.0.weight"), w("conv.0.bias"), 1, 1), sd, "conv.1"))
    note("conv.0", x)
    x = F.max_pool2d(x, 3, 2, 1)
    note("maxpool", x)
    for li, down in zip(range(1, 5), (False, True, True, True)):
        for b in range(2):
            q = "layer%d.%d" % (li, b)
            s = 2 if down and b == 0 else 1
            y = F.relu(_bn(F.conv2d(x, w(q + ".conv1.weight"), None, s, 1), sd, q + ".bn1"))
            note(q + ".conv1", y)
            y = _bn(F.conv2d(y, w(q + ".conv2.weight"), None, 1, 1), sd, q + ".bn2")
            if s == 2:
                x = _bn(F.conv2d(x, w(q + ".downsample.0.weight"), None, 2, 0), sd, q + ".downsample.1")
                note(q + ".downsample.0", x)
            x = F.relu(x + y)
            note(q + ".conv2", x)
    assert tuple(x.shape[1:]) == (DIM, 8, 4)
    x = x.mean((2, 3))
    return x / x.norm(p=2, dim=1, keepdim=True)


def normalise(crops_u8, dtype=torch.float64):
    """uint8 [n, 128, 64, 3] B, G, R crops -> the net's input under the reference's defaults, computed in `dtype`."""
    x = torch.from_numpy(np.asarray(crops_u8).astype(np.float64)).permute(0, 3, 1, 2).to(dtype)
    return (x - torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1)
