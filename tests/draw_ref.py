"""The NumPy reference of draw_results: a sequential painter written from the rule, not from csrc/draw_arith.h (nothing here reads that
file or the library), and the seeded cases the CPU and GPU tests share.

The rule.  Rows are float32 [M, 56]: box 0:4, score 4, joints 5:39 as (x, y), joint scores 39:56.  A row is live iff score > vis_thresh.
A non-finite coordinate kills its primitive, any other is clamped to [-16384, 16383] and truncated toward zero.  Per live row, in this
order: the box (four live coordinates), the 18 LIMBS (both joint scores > 0, four live coordinates), the 17 joints (score > 0, two live
coordinates).  With k = R^2 + R: a joint at P covers p iff |p - P|^2 <= k; a limb P -> Q with a = p - P, d = Q - P, L2 = d.d, t = a.d
covers p iff (L2 == 0 or t <= 0) and a.a <= k, or t >= L2 and |p - Q|^2 <= k, or 0 < t < L2 and (a x d)^2 <= k * L2; a box of thickness
T with sorted corners covers the pixels of the closed rectangle that are less than T from one of its sides.  Later paint wins."""
import numpy as np

LIMBS = [(0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (4, 6), (5, 6), (5, 7), (7, 9), (6, 8), (8, 10), (5, 11), (6, 12), (11, 12), (11, 13), (13, 15),
         (12, 14), (14, 16)]


def coord(v):
    """One float32 coordinate -> int, or None when it is not finite."""
    v = float(np.float32(v))
    if not np.isfinite(v):
        return None
    return int(np.trunc(min(max(v, -16384.0), 16383.0)))


def _disc(X, Y, px, py, k):
    return (X - px) ** 2 + (Y - py) ** 2 <= k


def joint_mask(X, Y, P, R):
    return _disc(X, Y, P[0], P[1], R * R + R)


def limb_mask(X, Y, P, Q, R):
    k = R * R + R
    ax, ay = X - P[0], Y - P[1]
    dx, dy = Q[0] - P[0], Q[1] - P[1]
    L2 = dx * dx + dy * dy
    t = ax * dx + ay * dy
    near_p = _disc(X, Y, P[0], P[1], k)
    if L2 == 0:
        return near_p
    near_q = _disc(X, Y, Q[0], Q[1], k)
    cross = ax * dy - ay * dx
    return np.where(t <= 0, near_p, np.where(t >= L2, near_q, cross * cross <= k * L2))


def box_mask(X, Y, c, T):
    x0, x1 = min(c[0], c[2]), max(c[0], c[2])
    y0, y1 = min(c[1], c[3]), max(c[1], c[3])
    inside = (X >= x0) & (X <= x1) & (Y >= y0) & (Y <= y1)
    return inside & ((X - x0 < T) | (x1 - X < T) | (Y - y0 < T) | (y1 - Y < T))


def winners(rows, H, W, vis_thresh, thickness, limb_radius, joint_radius):
    """int64 [H, W]: the paint index (row * 36 + primitive; 0 box, 1..18 limbs, 19..35 joints) of the last primitive that covers each
    pixel, -1 where none does.  Sequential: every primitive in paint order overwrites what it covers."""
    rows = np.asarray(rows, np.float32).reshape(-1, 56)
    Y, X = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    win = np.full((H, W), -1, np.int64)
    vis = np.float32(vis_thresh)
    for m, row in enumerate(rows):
        if not (row[4] > vis):                                 # NaN compares false
            continue
        if thickness > 0:
            c = [coord(v) for v in row[0:4]]
            if None not in c:
                win[box_mask(X, Y, c, thickness)] = m * 36
        pts = [(coord(row[5 + 2 * j]), coord(row[6 + 2 * j])) for j in range(17)]
        ok = [bool(row[39 + j] > 0) and None not in pts[j] for j in range(17)]
        if limb_radius >= 1:
            for i, (a, b) in enumerate(LIMBS):
                if ok[a] and ok[b]:
                    win[limb_mask(X, Y, pts[a], pts[b], limb_radius)] = m * 36 + 1 + i
        if joint_radius >= 0:
            for j in range(17):
                if ok[j]:
                    win[joint_mask(X, Y, pts[j], joint_radius)] = m * 36 + 19 + j
    return win


def paint_bgr(view, layout, color, win, palette):
    """view: a writable uint8 array [H,W,C] ("hwc") or [C,H,W] ("chw"), C = 3 or 4, first three channels in `color` order; palette: 36
    (B, G, R).  Covered pixels get the three bytes of their winner, nothing else is touched."""
    hwc = view if layout == "hwc" else view.transpose(1, 2, 0)
    pal = np.asarray(palette, np.uint8)
    ys, xs = np.nonzero(win >= 0)
    prim = win[ys, xs] % 36
    for k in range(3):                                         # k: B, G, R
        hwc[ys, xs, k if color == "bgr" else 2 - k] = pal[prim, k]


def paint_yuv(y, u, v, win, palette_yuv):
    """y [H,W], u / v [ceil(H/2),ceil(W/2)]: writable uint8 views of the planes; palette_yuv: 36 (Y, U, V).  Luma per covered pixel; a
    chroma sample is written iff one of its (up to four) luma pixels is covered, with the colour of the highest paint index among them."""
    pal = np.asarray(palette_yuv, np.uint8)
    H, W = win.shape
    ys, xs = np.nonzero(win >= 0)
    y[ys, xs] = pal[win[ys, xs] % 36, 0]
    padded = np.full((2 * ((H + 1) // 2), 2 * ((W + 1) // 2)), -1, np.int64)
    padded[:H, :W] = win
    top = padded.reshape((H + 1) // 2, 2, (W + 1) // 2, 2).max(axis=(1, 3))
    cy, cx = np.nonzero(top >= 0)
    u[cy, cx] = pal[top[cy, cx] % 36, 1]
    v[cy, cx] = pal[top[cy, cx] % 36, 2]


FORWARD = {"bt601": ((66, 129, 25), (-38, -74, 112), (112, -94, -18)), "bt709": ((47, 157, 16), (-26, -87, 112), (112, -102, -10))}


def bgr_to_yuv(colors, matrix="bt601"):
    """(B, G, R) -> (Y, U, V): Y = ((66R + 129G + 25B + 128) >> 8) + 16 and so on, the usual limited-range 8-bit forms."""
    out = []
    for b, g, r in colors:
        rgb = np.array([r, g, b], np.int64)
        out.append(tuple(int((np.dot(np.array(w, np.int64), rgb) + 128) >> 8) + off for w, off in zip(FORWARD[matrix], (16, 128, 128))))
    return out


# ------------------------------------------------------------------------------------------------------------------ shared cases
# A frame "form" is a flat host buffer of random bytes (the guard bytes, the padding and the alpha channel are simply the bytes no view
# element or no painted channel addresses) and the views of its planes as (byte offset, shape, strides): the host painter addresses the
# buffer by descriptor, the device test rebuilds the same views with torch.as_strided, the reference paints numpy as_strided views of a
# copy.  Whole buffers are compared, so a byte written anywhere it should not be is found.
SIZES = [(1, 1), (7, 5), (37, 53), (64, 64)]
GUARD = 64


def _rand(seed, n):
    return np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8)


def _span(shape, strides):
    return sum((n - 1) * s for n, s in zip(shape, strides)) + 1


def _form(seed, name, layout, color, views):
    """views: [(offset from the end of the front guard, shape, strides)]"""
    size = max(off + _span(sh, st) for off, sh, st in views) + 2 * GUARD
    return dict(name=name, layout=layout, color=color, buf=_rand(seed, size), views=[(off + GUARD, tuple(sh), tuple(st)) for off, sh, st in views])


def bgr_forms(seed, H, W):
    P = 4 * W + 13                                             # a padded row
    return [
        _form(seed, "hwc bgr", "hwc", "bgr", [(0, (H, W, 3), (3 * W, 3, 1))]),
        _form(seed + 1, "hwc rgb, 4 channels", "hwc", "rgb", [(0, (H, W, 4), (4 * W, 4, 1))]),
        _form(seed + 2, "hwc bgra, padded rows", "hwc", "bgr", [(0, (H, W, 4), (P, 4, 1))]),
        _form(seed + 3, "chw rgb", "chw", "rgb", [(0, (3, H, W), (H * W, W, 1))]),
        _form(seed + 4, "chw bgr, 4 planes, padded rows and planes", "chw", "bgr", [(0, (4, H, W), (H * (W + 5) + 9, W + 5, 1))]),
        _form(seed + 5, "roi of a larger hwc rgb frame", "hwc", "rgb", [((3 * (W + 11) + 4) * 3, (H, W, 3), ((W + 11) * 3, 3, 1))]),
    ]


def yuv_forms(seed, H, W):
    ch, cw = (H + 1) // 2, (W + 1) // 2
    ysz = H * W
    forms = [
        _form(seed, "nv12 planes", "hwc", "nv12", [(0, (H, W), (W, 1)), (ysz + 7, (ch, cw, 2), (2 * cw, 2, 1))]),
        _form(seed + 1, "nv21 planes, pitched", "hwc", "nv21", [(0, (H, W), (W + 9, 1)), (H * (W + 9) + 3, (ch, cw, 2), (2 * cw + 6, 2, 1))]),
        _form(seed + 2, "i420 planes", "hwc", "i420", [(0, (H, W), (W, 1)), (ysz + 5, (ch, cw), (cw, 1)), (ysz + 5 + ch * cw + 5, (ch, cw), (cw, 1))]),
        _form(seed + 3, "i420, chroma planes as views of one interleaved plane", "hwc", "i420",
              [(0, (H, W), (W + 3, 1)), (H * (W + 3) + 2, (ch, cw), (2 * cw, 2)), (H * (W + 3) + 3, (ch, cw), (2 * cw, 2))]),
    ]
    if H % 2 == 0 and W % 2 == 0:
        forms.append(_form(seed + 4, "nv12 surface, pitched", "hwc", "nv12", [(0, (H * 3 // 2, W), (W + 16, 1))]))
        forms.append(_form(seed + 5, "nv21 surface", "hwc", "nv21", [(0, (H * 3 // 2, W), (W, 1))]))
    return forms


def numpy_views(buf, form):
    return [np.lib.stride_tricks.as_strided(buf[off:], shape, strides) for off, shape, strides in form["views"]]


def yuv_planes(views, color):
    """The numpy views of a form -> (y [H,W], u, v [ceil(H/2),ceil(W/2)]) views, by what the colour name means."""
    if len(views) == 1:                                        # a surface [H*3/2, W]: luma rows, then interleaved chroma rows
        s = views[0]
        H, W = s.shape[0] * 2 // 3, s.shape[1]
        uv = np.lib.stride_tricks.as_strided(s[H:], (H // 2, W // 2, 2), (s.strides[0], 2 * s.strides[1], s.strides[1]))
        views = [s[:H], uv]
    if color == "i420":
        return views[0], views[1], views[2]
    first, second = views[1][..., 0], views[1][..., 1]
    return (views[0], first, second) if color == "nv12" else (views[0], second, first)


def frame_size(form):
    shape = form["views"][0][1]
    if form["color"] in ("bgr", "rgb"):
        return (shape[0], shape[1]) if form["layout"] == "hwc" else (shape[1], shape[2])
    return (shape[0] * 2 // 3 if len(form["views"]) == 1 else shape[0]), shape[1]


def reference(form, rows, vis_thresh, thickness, limb_radius, joint_radius, palette, matrix="bt601"):
    """The buffer of `form` after the reference has painted `rows` onto it (a copy; palette: 36 (B, G, R))."""
    buf = form["buf"].copy()
    views = numpy_views(buf, form)
    H, W = frame_size(form)
    win = winners(rows, H, W, vis_thresh, thickness, limb_radius, joint_radius)
    if form["color"] in ("bgr", "rgb"):
        paint_bgr(views[0], form["layout"], form["color"], win, palette)
    else:
        y, u, v = yuv_planes(views, form["color"])
        paint_yuv(y, u, v, win, bgr_to_yuv(palette, matrix))
    return buf


VIS = 0.3
_SPECIAL = [1e9, -1e9, np.nan, np.inf, -np.inf, 16383.9, -16384.9, 20000.0, -20000.0]
_SCORES = [1.0, 0.5, 1e-30, 0.0, -0.0, -1.0, np.nan]


def fuzz_rows(seed, M, H, W, dense=False):
    """float32 [M, 56].  Boxes and joints in and around the frame, some far outside on every side, some coordinates +-1e9 / NaN / +-inf;
    row scores above, exactly at and below VIS and NaN; joint scores > 0, 0, -0.0, negative and NaN.  dense: every row live."""
    r = np.random.RandomState(seed)
    rows = np.zeros((M, 56), np.float32)
    for m in range(M):
        far = r.randint(0, 6)                                  # 0..3: this row lies off one side of the frame
        ox = {0: -3.0 * W - 40, 1: 3.0 * W + 40}.get(far, 0.0)
        oy = {2: -3.0 * H - 40, 3: 3.0 * H + 40}.get(far, 0.0)
        if far < 4 and r.rand() < 0.5:                         # ... but reaches back into it
            ox, oy = ox / 3, oy / 3
        cx, cy = r.uniform(-4, W + 4) + ox, r.uniform(-4, H + 4) + oy
        w, h = r.uniform(0, W + 6), r.uniform(0, H + 6)
        box = [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2]
        if r.rand() < 0.3:
            box = [box[2], box[3], box[0], box[1]]             # reversed corners
        rows[m, 0:4] = box
        rows[m, 4] = 1.0 if dense else [0.9, 0.31, VIS, 0.1, np.nan, 0.9][r.randint(0, 6)]
        rows[m, 5:39:2] = cx + r.uniform(-w / 2 - 3, w / 2 + 3, 17)
        rows[m, 6:39:2] = cy + r.uniform(-h / 2 - 3, h / 2 + 3, 17)
        rows[m, 39:56] = np.where(r.rand(17) < 0.7, r.uniform(0.01, 1, 17), np.array(_SCORES, np.float32)[r.randint(0, len(_SCORES), 17)])
        for _ in range(r.randint(0, 4)):                       # special coordinates
            rows[m, r.choice([0, 1, 2, 3] + list(range(5, 39)))] = _SPECIAL[r.randint(0, len(_SPECIAL))]
    return rows


def fuzz_style(seed):
    """(thickness, limb_radius, joint_radius, 36 (B, G, R)): the default radii first, then random ones, the degenerate values included."""
    r = np.random.RandomState(seed)
    palette = [tuple(int(v) for v in c) for c in r.randint(0, 256, (36, 3))]
    if seed % 3 == 0:
        return 2, 1, 2, palette
    return int(r.choice([0, 1, 2, 3, 5, 64])), int(r.choice([-1, 1, 2, 3, 4])), int(r.choice([-1, 0, 1, 2, 3, 6])), palette
