"""The NumPy reference of the overlay painters (draw_results with score labels and translucent primitives): a sequential painter written
from the rule, not from csrc/draw_overlay_arith.h (nothing here reads csrc/ or the library).  The coverage masks, the frame forms and
the row fuzzers come from tests/draw_ref.py, the font from tests/draw_tracks_ref.py (the hand-drawn tests/golden/draw_font_5x7.txt).

The rule.  Per live row, in this order: the box, the 18 limbs, the 17 joints (tests/draw_ref.py), then -- when label_scale s >= 1 and
the row's four box coordinates are alive, whatever the box thickness -- the label bar, the closed rectangle [x0, x0 + 6 s n - s + 3] x
[y0 - 7 s - 5, y0 - 1] over the box's sorted corner (x0, y0), and the label text: character i's font cell (r, u) that is set fills the
s x s pixels at (x0 + 2 + 6 s i + s u, y0 - 7 s - 3 + s r).  The text is prefix + '%.1f' % score (scores with |s| < 999.95).  Every
primitive blends every byte it covers, p' = (p (256 - a) + c a + 128) >> 8 in int64, with a the opacity of its class (box, limbs,
joints; bar and text 256), one primitive after the other.  The bar takes the box's colour, the text its own.  YUV: luma per covered
pixel, a chroma sample once per primitive that covers any in-frame pixel of its 2 x 2 block."""
import numpy as np

import draw_ref
import draw_tracks_ref as tref


def score_text(score):
    return "%.1f" % float(np.float32(score))


def text_mask(H, W, x0, y0, text, s):
    """bool [H, W]: the pixels of `text` written with its first cell's top-left corner at (x0, y0), clipped to the frame."""
    m = np.zeros((H, W), bool)
    for i, ch in enumerate(text):
        for r in range(7):
            for u in range(5):
                if tref.FONT[ch][r, u]:
                    cx, cy = x0 + 6 * s * i + s * u, y0 + s * r
                    xa, xb, ya, yb = max(cx, 0), min(cx + s, W), max(cy, 0), min(cy + s, H)
                    if xa < xb and ya < yb:
                        m[ya:yb, xa:xb] = True
    return m


def primitives(rows, H, W, vis_thresh, thickness, limb_radius, joint_radius, label_scale=0, prefix=""):
    """Yields (row, primitive, bool [H, W] mask, info) in paint order for every primitive that exists; info: for the bar its rectangle
    (x0, y0, x1, y1) before clipping, else None."""
    rows = np.asarray(rows, np.float32).reshape(-1, 56)
    Y, X = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    vis = np.float32(vis_thresh)
    for m, row in enumerate(rows):
        if not (row[4] > vis):
            continue
        c = [draw_ref.coord(v) for v in row[0:4]]
        if thickness > 0 and None not in c:
            yield m, 0, draw_ref.box_mask(X, Y, c, thickness), None
        pts = [(draw_ref.coord(row[5 + 2 * j]), draw_ref.coord(row[6 + 2 * j])) for j in range(17)]
        ok = [bool(row[39 + j] > 0) and None not in pts[j] for j in range(17)]
        if limb_radius >= 1:
            for i, (a, b) in enumerate(draw_ref.LIMBS):
                if ok[a] and ok[b]:
                    yield m, 1 + i, draw_ref.limb_mask(X, Y, pts[a], pts[b], limb_radius), None
        if joint_radius >= 0:
            for j in range(17):
                if ok[j]:
                    yield m, 19 + j, draw_ref.joint_mask(X, Y, pts[j], joint_radius), None
        if label_scale >= 1 and None not in c:
            s, text = label_scale, prefix + score_text(row[4])
            x0, y0 = min(c[0], c[2]), min(c[1], c[3])
            bar = (x0, y0 - 7 * s - 5, x0 + 6 * s * len(text) - s + 3, y0 - 1)
            yield m, 36, (X >= bar[0]) & (X <= bar[2]) & (Y >= bar[1]) & (Y <= bar[3]), bar
            yield m, 37, text_mask(H, W, x0 + 2, y0 - 7 * s - 3, text, s), None


def _blend(arr, mask, c, a):
    """arr: a writable uint8 view; the bytes under `mask` blended with c at opacity a, in int64."""
    p = arr[mask].astype(np.int64)
    arr[mask] = ((p * (256 - a) + int(c) * a + 128) >> 8).astype(np.uint8)


def reference(form, rows, vis_thresh, thickness, limb_radius, joint_radius, palette, opacity=(256, 256, 256), label_scale=0, prefix="PERSON",
              text_color=(0, 0, 0), ids=None, id_palette=None, matrix="bt601", stats=None, prims=None):
    """The buffer of `form` after the reference has painted `rows` onto it (a copy).  palette: 36 (B, G, R); ids / id_palette: a row
    whose id is >= 0 takes id_palette[id % P] for its pose, its box and its bar.  stats (a dict): what the picture exercised.
    prims: list(primitives(...)) of these very arguments, for a caller that paints them several times in other colours."""
    buf = form["buf"].copy()
    views = draw_ref.numpy_views(buf, form)
    H, W = draw_ref.frame_size(form)
    yuv = form["color"] not in ("bgr", "rgb")
    conv = (lambda col: draw_ref.bgr_to_yuv([tuple(int(v) for v in col)], matrix)[0]) if yuv else (lambda col: tuple(int(v) for v in col))
    if yuv:
        y, u, v = draw_ref.yuv_planes(views, form["color"])
        ch, cw = (H + 1) // 2, (W + 1) // 2
    else:
        hwc = views[0] if form["layout"] == "hwc" else views[0].transpose(1, 2, 0)
    blends = np.zeros((H, W), np.int64)                          # how many translucent primitives were blended into each pixel
    st = dict(max_blends=0, partial_chroma=0, label_pixels=0, clipped_top=0, clipped_right=0, painted=0)
    if prims is None:
        prims = primitives(rows, H, W, vis_thresh, thickness, limb_radius, joint_radius, label_scale, prefix)
    for m, l, mask, bar in prims:
        a = 256 if l >= 36 else opacity[0 if l == 0 else (1 if l <= 18 else 2)]
        if l == 37:
            col = text_color
        elif ids is not None and int(ids[m]) >= 0:
            col = id_palette[int(ids[m]) % len(id_palette)]
        else:
            col = palette[0 if l == 36 else l]
        col = conv(col)
        if bar is not None and mask.any():
            st["clipped_top"] += int(bar[1] < 0)
            st["clipped_right"] += int(bar[2] > W - 1)
        if l >= 36:
            st["label_pixels"] += int(mask.sum())
        if a < 256:
            blends[mask] += 1
        st["painted"] += int(mask.sum())
        if yuv:
            _blend(y, mask, col[0], a)
            padded = np.zeros((2 * ch, 2 * cw), bool)
            padded[:H, :W] = mask
            blocks = padded.reshape(ch, 2, cw, 2)
            cm = blocks.any(axis=(1, 3))
            inframe = np.zeros((2 * ch, 2 * cw), bool)
            inframe[:H, :W] = True
            st["partial_chroma"] += int((cm & (blocks.sum(axis=(1, 3)) < inframe.reshape(ch, 2, cw, 2).sum(axis=(1, 3)))).sum())
            _blend(u, cm, col[1], a)
            _blend(v, cm, col[2], a)
        else:
            for k in range(3):                                 # k: B, G, R
                _blend(hwc[..., k if form["color"] == "bgr" else 2 - k], mask, col[k], a)
    st["max_blends"] = int(blends.max()) if blends.size else 0
    if stats is not None:
        for k, val in st.items():
            stats[k] = max(stats.get(k, 0), val) if k == "max_blends" else stats.get(k, 0) + val
    return buf


# ------------------------------------------------------------------------------------------------------------------ shared cases
# (label_scale, opacity (box, limbs, joints), prefix): labels only at s = 1, 2 and 8; opacities only; both together
STYLES = [(1, (256, 256, 256), "PERSON"), (2, (256, 256, 256), "P"), (8, (256, 256, 256), ""),
          (0, (128, 51, 256), "PERSON"), (0, (1, 255, 128), "PERSON"), (0, (255, 255, 255), "PERSON"),
          (2, (128, 51, 256), "PERSON"), (1, (1, 255, 128), "ID_7:# -.")]


def text_color(seed):
    return tuple(int(v) for v in np.random.RandomState(seed + 77).randint(0, 256, 3))


def wide_score_rows(seed, M, H, W):
    """fuzz_rows, every row with a score of its own in (-999.9, 999.9): live under a threshold of -1000, signs and three digits drawn."""
    rows = draw_ref.fuzz_rows(seed, M, H, W, dense=True)
    r = np.random.RandomState(seed + 5)
    rows[:, 4] = np.where(r.rand(M) < 0.5, r.uniform(-999.9, 999.9, M), r.uniform(-1.2, 1.2, M)).astype(np.float32)
    rows[0, 4] = -0.0
    return rows
