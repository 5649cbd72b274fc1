"""The NumPy reference of draw_tracks and of the identity-coloured draw_results: sequential painters written from the rule, not from
csrc/draw_text_arith.h (nothing here reads that file or the library), with their own copy of the font, read from the hand-drawn
tests/golden/draw_font_5x7.txt; and the seeded cases the CPU and GPU tests share.  The pose primitives come from tests/draw_ref.py.

The rule.  An item is a box with sorted integer corners, a colour, a text colour and a label of 0..16 characters.  With thickness T and
font scale s, in this order per item: the box (draw_ref.box_mask); if s > 0 and the label is not empty the bar, the closed rectangle
[x0, x0 + 6 s n - s + 3] x [y0, y0 + 7 s + 4]; then the text: character i's cell (r, u) that is set in the font fills the s x s pixels
at (x0 + 2 + 6 s i + s u, y0 + 2 + s r).  Items ascending; later paint wins."""
import os

import numpy as np

import draw_ref

CHARSET = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ #-.:_"         # the glyph order of cp_draw_track_item (include/centerpose_hip.h)
FONT_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "draw_font_5x7.txt")


def load_font(path=FONT_FILE):
    """{character: bool [7, 5]} from the ASCII-art file: a line [c], then seven rows of '#' and '.'."""
    font, cur = {}, None
    for line in open(path).read().split("\n"):
        if len(line) == 3 and line[0] == "[" and line[2] == "]":
            cur = line[1]
            assert cur not in font, cur
            font[cur] = []
        elif cur is not None and len(line) == 5 and set(line) <= {"#", "."}:
            font[cur].append([c == "#" for c in line])
    assert all(len(v) == 7 for v in font.values())
    return {c: np.array(v, bool) for c, v in font.items()}


FONT = load_font()
SIZES = [(1, 1), (7, 5), (37, 53), (64, 96)]


def glyph_rows(ch):
    """The seven row bytes of a character, bit 4 the leftmost column: what cp_draw_glyph_rows returns."""
    return [int(sum(int(b) << (4 - u) for u, b in enumerate(row))) for row in FONT[ch]]


def item(x0, y0, x1, y1, text="", color=(10, 200, 30), text_color=(255, 255, 255)):
    return dict(x0=min(x0, x1), y0=min(y0, y1), x1=max(x0, x1), y1=max(y0, y1), text=text, color=tuple(color), text_color=tuple(text_color))


def item_winners(items, H, W, T, s):
    """int64 [H, W]: the paint index (item * 3 + primitive; 0 box, 1 bar, 2 text) of the last primitive that covers each pixel, -1 where
    none does.  Sequential: every primitive in paint order overwrites what it covers; the text is blitted cell by cell."""
    Y, X = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    win = np.full((H, W), -1, np.int64)
    for k, it in enumerate(items):
        x0, y0 = it["x0"], it["y0"]
        if T > 0:
            win[draw_ref.box_mask(X, Y, (x0, y0, it["x1"], it["y1"]), T)] = 3 * k
        n = len(it["text"])
        if s <= 0 or n == 0:
            continue
        win[(X >= x0) & (X <= x0 + 6 * s * n - s + 3) & (Y >= y0) & (Y <= y0 + 7 * s + 4)] = 3 * k + 1
        for i, ch in enumerate(it["text"]):
            for r in range(7):
                for u in range(5):
                    if FONT[ch][r, u]:
                        cx, cy = x0 + 2 + 6 * s * i + s * u, y0 + 2 + s * r
                        xa, xb, ya, yb = max(cx, 0), min(cx + s, W), max(cy, 0), min(cy + s, H)
                        if xa < xb and ya < yb:
                            win[ya:yb, xa:xb] = 3 * k + 2
    return win


def item_colors(items):
    """(B, G, R) per paint index: uint8 [3 K, 3]."""
    out = []
    for it in items:
        out += [it["color"], it["color"], it["text_color"]]
    return np.array(out, np.uint8).reshape(-1, 3)


def row_colors(M, palette, ids=None, id_palette=None):
    """(B, G, R) per paint index of M detection rows (row * 36 + primitive): the style's palette, or id_palette[id % P] for a row
    whose id is >= 0."""
    out = np.tile(np.asarray(palette, np.uint8).reshape(1, 36, 3), (M, 1, 1))
    if ids is not None:
        for m, i in enumerate(ids):
            if int(i) >= 0:
                out[m, :] = id_palette[int(i) % len(id_palette)]
    return out.reshape(-1, 3)


def paint_bgr(view, layout, color, win, colors):
    hwc = view if layout == "hwc" else view.transpose(1, 2, 0)
    ys, xs = np.nonzero(win >= 0)
    for k in range(3):
        hwc[ys, xs, k if color == "bgr" else 2 - k] = colors[win[ys, xs], k]


def paint_yuv(y, u, v, win, colors_yuv):
    H, W = win.shape
    ys, xs = np.nonzero(win >= 0)
    y[ys, xs] = colors_yuv[win[ys, xs], 0]
    padded = np.full((2 * ((H + 1) // 2), 2 * ((W + 1) // 2)), -1, np.int64)
    padded[:H, :W] = win
    top = padded.reshape((H + 1) // 2, 2, (W + 1) // 2, 2).max(axis=(1, 3))
    cy, cx = np.nonzero(top >= 0)
    u[cy, cx] = colors_yuv[top[cy, cx], 1]
    v[cy, cx] = colors_yuv[top[cy, cx], 2]


def paint(buf, form, win, colors, matrix="bt601"):
    """Paint `buf` (a form's buffer or a copy), in place, with the winners `win` and (B, G, R) `colors` per paint index."""
    views = draw_ref.numpy_views(buf, form)
    if form["color"] in ("bgr", "rgb"):
        paint_bgr(views[0], form["layout"], form["color"], win, colors)
    elif len(colors):
        y, u, v = draw_ref.yuv_planes(views, form["color"])
        paint_yuv(y, u, v, win, np.array(draw_ref.bgr_to_yuv([tuple(int(c) for c in col) for col in colors], matrix), np.uint8).reshape(-1, 3))
    return buf


def reference(form, items, T, s, matrix="bt601", buf=None):
    """The buffer of `form` (or `buf`, painted in place) after the reference has painted `items` onto it."""
    buf = form["buf"].copy() if buf is None else buf
    H, W = draw_ref.frame_size(form)
    return paint(buf, form, item_winners(items, H, W, T, s), item_colors(items), matrix)


def reference_rows(form, rows, vis, T, RL, RJ, palette, ids=None, id_palette=None, matrix="bt601", buf=None):
    """The same for detection rows in identity colours."""
    buf = form["buf"].copy() if buf is None else buf
    H, W = draw_ref.frame_size(form)
    rows = np.asarray(rows, np.float32).reshape(-1, 56)
    return paint(buf, form, draw_ref.winners(rows, H, W, vis, T, RL, RJ), row_colors(len(rows), palette, ids, id_palette), matrix)


# ------------------------------------------------------------------------------------------------------------------ shared cases
def fuzz_label(r, n):
    return "".join(CHARSET[i] for i in r.randint(0, len(CHARSET), n))


def fuzz_items(seed, K, H, W):
    """K items: boxes in and around the frame, some far outside on every side, some degenerate (x0 = x1, y0 = y1), some at the clamp
    limits; labels of 0, 1, 16 and other lengths over the whole character set."""
    r = np.random.RandomState(seed)
    items = []
    for k in range(K):
        far = r.randint(0, 8)
        ox = {0: -3 * W - 900, 1: 3 * W + 900}.get(far, 0)
        oy = {2: -3 * H - 900, 3: 3 * H + 900}.get(far, 0)
        if far < 4 and r.rand() < 0.5:                         # ... but its bar or box reaches back into the frame
            ox, oy = ox // 40, oy // 40
        x0, y0 = int(r.randint(-8, W + 4)) + ox, int(r.randint(-8, H + 4)) + oy
        w, h = int(r.randint(0, W + 8)), int(r.randint(0, H + 8))
        if far == 4:
            w = 0
        if far == 5:
            h = 0
        if far == 6 and k % 5 == 0:
            x0, y0, w, h = -16384, -16384, 32767, 32767        # the clamp limits: a box around everything
        n = [0, 1, 16, int(r.randint(2, 16))][r.randint(0, 4)]
        items.append(item(x0, y0, min(x0 + w, 16383), min(y0 + h, 16383), fuzz_label(r, n), tuple(int(v) for v in r.randint(0, 256, 3)),
                          tuple(int(v) for v in r.randint(0, 256, 3))))
    return items


STYLES = [(3, 2), (0, 1), (64, 8), (1, 0), (2, 1), (5, 3)]     # (T, s): the defaults, T = 0 and 64, s = 0, 1, 2, 3 and 8


def fuzz_ids(seed, M):
    """int32 [M]: about half the rows matched (ids up to 2^31 - 1), the rest -1 or another negative value."""
    r = np.random.RandomState(seed)
    ids = r.randint(0, 200, M).astype(np.int64)
    ids[r.rand(M) < 0.15] = 2 ** 31 - 1
    ids[r.rand(M) < 0.5] = -1
    ids[r.rand(M) < 0.1] = -7
    return ids.astype(np.int32)


def fuzz_id_palette(seed, P):
    r = np.random.RandomState(seed)
    return [tuple(int(v) for v in c) for c in r.randint(0, 256, (P, 3))]
