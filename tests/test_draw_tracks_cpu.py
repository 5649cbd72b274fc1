"""CPU: draw_tracks, the identity-coloured draw_results and the per-row track ids without a device -- the font against the hand-drawn
ASCII-art file, the HOST painters (cp_draw_tracks_*_host, cp_draw_rows_ids_*_host: the statements of csrc/draw_text_arith.h and
csrc/draw_arith.h the kernels compile) against hand-written pixel sets and, byte for byte over whole buffers, against the independent
NumPy painter of tests/draw_tracks_ref.py; cp_track_row_ids_host against a NumPy scatter; every refusal that needs no device."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import draw_ref
import draw_tracks_ref as tref
import draw_tracks_util as tu
import draw_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p
SYMBOLS = ["cp_draw_rows_ids_frames_u8", "cp_draw_rows_ids_yuv_frames_u8", "cp_draw_rows_ids_frames_host", "cp_draw_rows_ids_yuv_frames_host",
           "cp_draw_tracks_frames_u8", "cp_draw_tracks_yuv_frames_u8", "cp_draw_tracks_frames_host", "cp_draw_tracks_yuv_frames_host",
           "cp_sizeof_draw_track_item", "cp_draw_glyph_rows", "cp_track_row_ids", "cp_track_row_ids_host"]


@functools.lru_cache(maxsize=None)
def _L():
    return draw_util.lib_built()


def _err():
    return _L().cp_last_error().decode()


# ---------------------------------------------------------------- 1. symbols, the structs, the font
def test_symbols_and_structs():
    from centerpose_amd import _lib, detector, draw
    L = _L()
    header = open(os.path.join(ROOT, "include", "centerpose_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in SYMBOLS:
        assert "int %s(" % sym in header, sym
        assert " T %s\n" % sym in nm, sym
    assert L.cp_sizeof_draw_track_item() == detector.TRACK_ITEM.itemsize == 44
    body = re.search(r"typedef struct cp_draw_track_item \{(.*?)\} cp_draw_track_item;", header, re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"(?:unsigned char|int) ([^;]+);", body) for f in re.sub(r"\[\d+\]", "", decl).split(",")]
    assert fields == list(detector.TRACK_ITEM.names)
    assert draw.DRAW_ID_PALETTE.itemsize == 260 and draw.CHARSET == tref.CHARSET


def test_font_equals_the_ascii_art_file():
    L = _L()
    assert sorted(tref.FONT) == sorted(tref.CHARSET) and len(tref.CHARSET) == 42
    seen = {}
    for i, ch in enumerate(tref.CHARSET):
        rows = (ctypes.c_ubyte * 7)()
        assert L.cp_draw_glyph_rows(ord(ch), rows) == i, ch
        assert list(rows) == tref.glyph_rows(ch), ch
        assert all(v < 32 for v in rows)
        assert tuple(rows) not in seen, (ch, seen.get(tuple(rows)))          # all glyphs are distinct
        seen[tuple(rows)] = ch
    sentinel = (ctypes.c_ubyte * 7)(*[0xEE] * 7)
    for code in range(-2, 300):
        if 0 <= code < 256 and chr(code) in tref.CHARSET:
            continue
        assert L.cp_draw_glyph_rows(code, sentinel) == -1, code               # lower case included: the caller folds it
    assert list(sentinel) == [0xEE] * 7
    assert L.cp_draw_glyph_rows(ord("A"), None) == -1


# ---------------------------------------------------------------- 2. hand-written pixel sets
def _index_map(items, H, W, T, s):
    """The host painter on a zeroed H x W BGR frame, item k painting (k + 1, 0, 0) and its text (k + 1, 1, 0) -> {(x, y): (k, is text)}."""
    form = dict(name="plain", layout="hwc", color="bgr", buf=np.zeros(H * W * 3, np.uint8), views=[(0, (H, W, 3), (3 * W, 3, 1))])
    items = [dict(it, color=(k + 1, 0, 0), text_color=(k + 1, 1, 0)) for k, it in enumerate(items)]
    got, = tu.host_paint_tracks(_L(), [form], [items], T, s)
    assert np.array_equal(got, tref.reference(form, items, T, s))
    img = got.reshape(H, W, 3)
    assert not img[..., 2].any()
    return {(x, y): (int(img[y, x, 0]) - 1, bool(img[y, x, 1])) for y in range(H) for x in range(W) if img[y, x, 0]}


ONE = {(2, 0), (1, 1), (2, 1), (2, 2), (2, 3), (2, 4), (2, 5), (1, 6), (2, 6), (3, 6)}       # the cells (u, r) of the glyph "1"


def test_one_glyph_at_scale_1_and_3():
    got = _index_map([tref.item(3, 4, 30, 30, "1")], 24, 24, 0, 1)
    text = {p for p, (k, t) in got.items() if t}
    assert text == {(3 + 2 + u, 4 + 2 + r) for u, r in ONE}
    bar = {p for p, (k, t) in got.items() if not t}
    assert bar == {(x, y) for x in range(3, 3 + 5 + 3 + 1) for y in range(4, 4 + 7 + 4 + 1)} - text      # tw = 5, th = 7
    got = _index_map([tref.item(0, 0, 0, 0, "-")], 30, 30, 0, 3)
    text = {p for p, (k, t) in got.items() if t}
    assert text == {(x, y) for x in range(2, 17) for y in range(11, 14)}        # row 3 of "-": five columns of 3 pixels, 3 pixels high
    assert {p for p in got} == {(x, y) for x in range(0, 19) for y in range(0, 26)}          # tw = 15, th = 21: the bar [0, 18] x [0, 25]


def test_bar_of_two_characters_and_the_box_under_it():
    got = _index_map([tref.item(4, 2, 40, 29, "  ")], 32, 48, 2, 2)             # two spaces: a bar without text
    assert not any(t for _, t in got.values())
    bar = {(x, y) for x in range(4, 4 + 22 + 3 + 1) for y in range(2, 2 + 14 + 4 + 1)}       # tw = 6 * 2 * 2 - 2 = 22, th = 14
    box = {(x, y) for x in range(4, 41) for y in range(2, 30) if x - 4 < 2 or 40 - x < 2 or y - 2 < 2 or 29 - y < 2}
    assert set(got) == bar | box and not bar <= box
    # s = 0: no bar and no text; no characters: the same
    assert set(_index_map([tref.item(4, 2, 40, 29, "AB")], 32, 48, 2, 0)) == box
    assert set(_index_map([tref.item(4, 2, 40, 29, "")], 32, 48, 2, 2)) == box
    # a later item paints over an earlier one's label
    got = _index_map([tref.item(4, 2, 40, 29, "8"), tref.item(6, 4, 6, 4, "")], 32, 48, 1, 1)
    assert got[(6, 4)] == (1, False) and got[(5, 4)] == (0, False) and got[(4 + 2 + 1, 2 + 2)] == (0, True)


@pytest.mark.parametrize("x0,y0", [(-4, 5), (5, -5), (16, 5), (5, 12), (-6, -7), (17, 14)])
def test_label_cut_by_each_frame_edge(x0, y0):
    H, W = 20, 22
    got = _index_map([tref.item(x0, y0, x0 + 1, y0 + 1, "1")], H, W, 0, 1)
    inside = lambda p: 0 <= p[0] < W and 0 <= p[1] < H
    text = {(x0 + 2 + u, y0 + 2 + r) for u, r in ONE}
    bar = {(x, y) for x in range(x0, x0 + 9) for y in range(y0, y0 + 12)}
    assert {p for p, (k, t) in got.items() if t} == set(filter(inside, text))
    assert set(got) == set(filter(inside, bar)) and 0 < len(got) < len(bar)


# ---------------------------------------------------------------- 3. host painters == NumPy, whole buffers
def _forms(kind, seed, H, W):
    return (draw_ref.bgr_forms if kind == "bgr" else draw_ref.yuv_forms)(seed, H, W)


@pytest.mark.parametrize("kind", ["bgr", "yuv"])
@pytest.mark.parametrize("sz", range(len(tref.SIZES)))
def test_host_painter_equals_numpy(kind, sz):
    L = _L()
    H, W = tref.SIZES[sz]
    painted = 0
    for f, form in enumerate(_forms(kind, 100 * sz + 20, H, W)):
        for trial, (T, s) in enumerate(tref.STYLES):
            seed = 2000 * sz + 20 * f + trial + (700 if kind == "yuv" else 0)
            items = tref.fuzz_items(seed, 14, H, W)
            matrix = "bt709" if trial % 3 == 2 else "bt601"
            want = tref.reference(form, items, T, s, matrix)
            host, = tu.host_paint_tracks(L, [form], [items], T, s, matrix)
            assert np.array_equal(host, want), (form["name"], seed, np.nonzero(host != want)[0][:8])
            G = draw_ref.GUARD
            assert np.array_equal(host[:G], form["buf"][:G]) and np.array_equal(host[-G:], form["buf"][-G:])
            painted += int((want != form["buf"]).sum())
    assert painted > 0


@pytest.mark.parametrize("kind", ["bgr", "yuv"])
def test_host_painter_300_overlapping_items_and_counts_per_frame(kind):
    L = _L()
    forms = [_forms(kind, 400 + n, 37, 53)[n % 3] for n in (0, 3, 6)]       # one form three times: a call has one layout / colour
    per_frame = [tref.fuzz_items(31, 300, 37, 53), [], tref.fuzz_items(32, 5, 37, 53)]
    want = [tref.reference(f, it, 2, 1) for f, it in zip(forms, per_frame)]
    host = tu.host_paint_tracks(L, forms, per_frame, 2, 1)
    for n in range(3):
        assert np.array_equal(host[n], want[n]), n
    assert np.array_equal(host[1], forms[1]["buf"]) and not np.array_equal(host[0], forms[0]["buf"])
    win = tref.item_winners(per_frame[0], 37, 53, 2, 1) // 3
    assert (win >= 256).any() and ((win >= 0) & (win < 256)).any()             # winners from both chunks of the device walk
    # N = 0 and no items at all succeed
    assert L.cp_draw_tracks_frames_host(None, 0, None, None, 4, 2, 1) == 0
    assert L.cp_draw_tracks_frames_host(None, 3, None, None, 0, 2, 1) == 0


# ---------------------------------------------------------------- 4. identity-coloured rows
@pytest.mark.parametrize("kind", ["bgr", "yuv"])
@pytest.mark.parametrize("sz", [1, 2, 3])
def test_rows_ids_host_painter(kind, sz):
    L = _L()
    H, W = tref.SIZES[sz]
    differs = 0
    for f, form in enumerate(_forms(kind, 100 * sz + 30, H, W)):
        seed = 3000 * sz + 10 * f + (500 if kind == "yuv" else 0)
        rows = draw_ref.fuzz_rows(seed, 12, H, W)
        T, RL, RJ, pal = draw_ref.fuzz_style(seed)
        matrix = "bt709" if f % 2 else "bt601"
        plain, = draw_util.host_paint(L, [form], rows, draw_ref.VIS, T, RL, RJ, pal, matrix)
        idpal = tref.fuzz_id_palette(seed, [1, 7, 64][f % 3])
        none, = tu.host_paint_rows_ids(L, [form], rows, np.full(12, -1, np.int32), idpal, draw_ref.VIS, T, RL, RJ, pal, matrix)
        assert np.array_equal(none, plain), form["name"]                       # all ids -1: today's picture, byte for byte
        ids = tref.fuzz_ids(seed, 12)
        want = tref.reference_rows(form, rows, draw_ref.VIS, T, RL, RJ, pal, ids, idpal, matrix)
        got, = tu.host_paint_rows_ids(L, [form], rows, ids, idpal, draw_ref.VIS, T, RL, RJ, pal, matrix)
        assert np.array_equal(got, want), (form["name"], seed)
        differs += int(not np.array_equal(got, plain))
    assert differs > 0


# ---------------------------------------------------------------- 5. per-row track ids
@pytest.mark.parametrize("S,q,M,capacity", [(1, 1, 1, 1), (2, 4, 9, 8), (3, 5, 7, 17), (2, 6, 4, 13), (1, 3, 0, 3)])
def test_row_ids_host_twin(S, q, M, capacity):
    slots, slot_ids, want = tu.row_ids_case(5 + S + q, S, q, M, capacity)
    rc, got = tu.host_row_ids(_L(), slots, slot_ids, capacity, S, q, M)
    assert rc == 0, _err()
    assert np.array_equal(got, want)
    if M > 2:
        assert (want >= 0).any() and (want == -1).any()


def test_row_ids_refusals():
    L = _L()
    for fn, tail in ((L.cp_track_row_ids, (None,)), (L.cp_track_row_ids_host, ())):
        assert fn(None, VP(64), 8, 2, 4, 9, VP(64), *tail) == 1 and "null" in _err()
        assert fn(VP(64), None, 8, 2, 4, 9, VP(64), *tail) == 1 and "null" in _err()
        assert fn(VP(64), VP(64), 8, 2, 4, 9, None, *tail) == 1 and "null" in _err()
        assert fn(VP(64), VP(64), 7, 2, 4, 9, VP(64), *tail) == 1 and "capacity" in _err()
        assert fn(VP(64), VP(64), 8, 0, 4, 9, VP(64), *tail) == 1 and "S = 0" in _err()
        assert fn(VP(64), VP(64), 8, 2, 0, 9, VP(64), *tail) == 1 and "q = 0" in _err()
        assert fn(VP(64), VP(64), 8, 2, 4, -1, VP(64), *tail) == 1 and "negative" in _err()
        assert fn(VP(64), VP(64), 8, 2, 4, (1 << 23) + 1, VP(64), *tail) == 1 and "2^24" in _err()
    for bad in (-2, 18):                                                      # slot values outside [-1, S * M): the host twin refuses
        slots = np.array([0, bad, 3, -1], np.int32)
        rc, got = tu.host_row_ids(L, slots, np.zeros(4, np.int32), 4, 2, 2, 9)
        assert rc == 1 and "outside" in _err() and (got == -99).all()


# ---------------------------------------------------------------- 6. refusals through ctypes; the frames are never touched
def _good_call(yuv=False):
    """(forms, bufs, table, items, counts): one valid 7 x 5 frame with two items; the tables are real, the frame is never written."""
    form = _forms("yuv" if yuv else "bgr", 60, 7, 5)[0]
    buf = form["buf"].copy()
    table = draw_util.table_of([form], [buf.ctypes.data])
    items, counts = tu.item_table([[tref.item(0, 0, 4, 4, "A1"), tref.item(1, 1, 3, 3, "")]], yuv)
    return form, buf, table, items, counts


@pytest.mark.parametrize("yuv", [False, True])
def test_draw_tracks_refusals(yuv):
    L = _L()
    form, buf, table, items, counts = _good_call(yuv)
    host = L.cp_draw_tracks_yuv_frames_host if yuv else L.cp_draw_tracks_frames_host
    dev = L.cp_draw_tracks_yuv_frames_u8 if yuv else L.cp_draw_tracks_frames_u8
    t, i, c = (a.ctypes.data_as(VP) for a in (table, items, counts))

    def both(word, N=1, Kmax=2, T=2, s=1, t=t, i=i, c=c):
        assert host(t, N, i, c, Kmax, T, s) == 1 and word in _err(), (word, _err())
        assert dev(VP(256), t, N, VP(256), i, VP(256), c, Kmax, T, s, None) == 1 and word in _err(), (word, _err())

    both("frames per call", N=-1)
    both("frames per call", N=65536)
    both("negative item count", Kmax=-1)
    both("too many", N=4097, Kmax=4096)
    both("box_thickness", T=-1)
    both("box_thickness", T=65)
    both("font_scale", s=-1)
    both("font_scale", s=9)
    both("null", t=None)
    both("null", i=None)
    both("null", c=None)
    assert dev(None, t, 1, VP(256), i, VP(256), c, 2, 2, 1, None) == 1 and "null" in _err()
    assert dev(VP(256), t, 1, None, i, VP(256), c, 2, 2, 1, None) == 1 and "null" in _err()
    assert dev(VP(256), t, 1, VP(256), i, None, c, 2, 2, 1, None) == 1 and "null" in _err()
    assert dev(VP(256), t, 1, VP(258), i, VP(256), c, 2, 2, 1, None) == 1 and "aligned" in _err()
    for field, value, word in (("nchars", 17, "characters"), ("nchars", -1, "characters"), ("x0", 5, "sorted"), ("y1", 16384, "sorted"),
                               ("x0", -16385, "sorted")):
        keep = items[0, 0][field]
        items[0, 0][field] = value
        both(word)
        items[0, 0][field] = keep
    items[0, 0]["glyph"][1] = 42
    both("glyph index")
    items[0, 0]["glyph"][1] = 1
    items[0, 1]["glyph"][0] = 200                                              # behind nchars = 0: not read, not refused
    for bad in (-1, 3):
        counts[0] = bad
        both("outside 0..Kmax")
    counts[0] = 2
    good = table[0]["W"]
    table[0]["W"] = 0
    both("bad size")
    table[0]["W"] = good
    assert np.array_equal(buf, form["buf"])                                   # nothing was painted by any refused call
    assert host(t, 1, i, c, 2, 2, 1) == 0 and not np.array_equal(buf, form["buf"])
    # N = 0, Kmax = 0, and no items at all: the device launcher succeeds without a device, for it launches nothing
    assert dev(None, None, 0, None, None, None, None, 2, 2, 1, None) == 0
    assert dev(None, None, 1, None, None, None, None, 0, 2, 1, None) == 0
    counts[0] = 0
    assert dev(VP(256), t, 1, VP(256), i, VP(256), c, 2, 2, 1, None) == 0


@pytest.mark.parametrize("yuv", [False, True])
def test_rows_ids_refusals(yuv):
    L = _L()
    form = _forms("yuv" if yuv else "bgr", 61, 7, 5)[0]
    buf = form["buf"].copy()
    table = draw_util.table_of([form], [buf.ctypes.data])
    rows = np.zeros((1, 2, 56), np.float32)
    rows[:, :, 0:5] = (0, 0, 4, 4, 1.0)
    ids = np.array([[3, -1]], np.int32)
    st = draw_util.style_struct(2, 1, 2, [(255, 255, 255)] * 36)
    idp = tu.id_palette_struct([(1, 2, 3)])
    host = L.cp_draw_rows_ids_yuv_frames_host if yuv else L.cp_draw_rows_ids_frames_host
    dev = L.cp_draw_rows_ids_yuv_frames_u8 if yuv else L.cp_draw_rows_ids_frames_u8
    t, r, s_, i, p = (a.ctypes.data_as(VP) for a in (table, rows, st, ids, idp))
    nbytes = ctypes.c_size_t(1 << 20)

    def both(word, i=i, p=p, M=2):
        assert host(t, 1, r, M, ctypes.c_float(0.3), s_, i, p) == 1 and word in _err(), (word, _err())
        assert dev(VP(256), t, 1, VP(256), M, ctypes.c_float(0.3), s_, VP(256), nbytes, VP(256) if i else None, p, None) == 1 and word in _err()

    both("row_ids", i=None)
    both("id palette", p=None)
    for count in (0, 65, -1):
        idp["count"] = count
        both("id colours")
    idp["count"] = 1
    both("negative row count", M=-1)                                          # and the checks of the plain entry points still hold
    assert np.array_equal(buf, form["buf"])
    assert host(t, 1, r, 2, ctypes.c_float(0.3), s_, i, p) == 0 and not np.array_equal(buf, form["buf"])


# ---------------------------------------------------------------- 7. the Python side
def test_track_style_palette_and_items():
    from centerpose_amd import detector, draw
    from centerpose_amd._lib import CenterposeHipError
    st = detector.TrackStyle()
    assert (st.box_thickness, st.font_scale, st.prefix, st.text_color) == (3, 2, "ID ", (255, 255, 255))
    pal = detector.TRACK_PALETTE
    assert st.palette == pal and 16 <= len(pal) <= 64 and len(set(pal)) == len(pal)
    assert all(len(c) == 3 and all(0 <= v <= 255 for v in c) for c in pal)
    for a in range(len(pal)):                                                 # clearly distinct: no two colours close in every channel
        for b in range(a):
            assert max(abs(x - y) for x, y in zip(pal[a], pal[b])) >= 40, (a, b)
    tracks = [np.array([[30, 20, 10, 5, 7], [-40000, 3, 50000, 9, 25]], np.int64), np.zeros((0, 5), np.int64)]
    items, counts = draw.track_items(tracks, detector.TrackStyle(prefix="id "))
    assert items.shape == (2, 2) and counts.tolist() == [2, 0]
    a, b = items[0]
    assert (a["x0"], a["y0"], a["x1"], a["y1"]) == (10, 5, 30, 20) and (b["x0"], b["x1"]) == (-16384, 16383)      # sorted, clamped
    assert a["nchars"] == 4 and a["glyph"][:4].tolist() == [tref.CHARSET.index(c) for c in "ID 7"]                # lower case folded
    assert tuple(a["color"][:3]) == pal[7] and tuple(b["color"][:3]) == pal[25 % len(pal)] and tuple(a["text_color"][:3]) == (255, 255, 255)
    yuv, _ = draw.track_items(tracks, detector.TrackStyle(), "bt601")
    assert tuple(yuv[0, 0]["color"][:3]) == draw_ref.bgr_to_yuv([pal[7]])[0]
    with pytest.raises(ValueError, match="at most 16"):
        draw.track_items([np.array([[0, 0, 5, 5, 10 ** 14]], np.int64)], detector.TrackStyle())
    draw.track_items([np.array([[0, 0, 5, 5, 10 ** 12]], np.int64)], detector.TrackStyle())            # "ID " + 13 digits: 16 characters
    with pytest.raises(ValueError, match="does not have"):
        detector.TrackStyle(prefix="N° ")
    with pytest.raises(ValueError, match="does not have"):
        draw.label_glyphs("A+B")
    for bad in (dict(box_thickness=65), dict(font_scale=9), dict(font_scale=-1), dict(palette=[]), dict(palette=[(0, 0, 0)] * 65),
                dict(text_color=(0, 0, 256))):
        with pytest.raises(CenterposeHipError):
            detector.TrackStyle(**bad)


def _detector():
    from centerpose_amd import config, detector
    det = object.__new__(detector.MultiPoseDetector)
    det.cfg = config.get_cfg("dla_34")
    det.scales = det.cfg.TEST.TEST_SCALES
    det.model = type("Model", (), {"process": None, "device": "cpu"})()
    return det


def test_python_refusals_without_a_device():
    from centerpose_amd import frames, track
    from centerpose_amd._lib import CenterposeHipError
    det = _detector()
    none = [np.zeros((0, 5), np.int64)]
    with pytest.raises(ValueError, match="needs track="):
        det.run_batch([np.zeros((8, 8, 3), np.uint8)], draw="tracks")
    with pytest.raises(ValueError, match="needs track="):
        det.run_batch([], draw="tracks")
    with pytest.raises(ValueError, match="tracks"):
        det.run_batch([], draw="boxes")
    with pytest.raises(CenterposeHipError, match="host arrays"):
        det.draw_tracks([np.zeros((8, 8, 3), np.uint8)], none)
    with pytest.raises(CenterposeHipError, match="cpu"):
        det.draw_tracks([torch.zeros((8, 8, 3), dtype=torch.uint8)], none)
    t = torch.zeros((8, 8, 3), dtype=torch.uint8)
    with pytest.raises(CenterposeHipError, match="given twice"):               # the writability rule draw_tracks applies
        frames.FrameIO.check_writable([t, t], [t, t], "bgr")
    with pytest.raises(CenterposeHipError, match="same byte"):
        frames.FrameIO.check_writable([t[:, :1].expand(8, 8, 3)], [t[:, :1].expand(8, 8, 3)], "bgr")
    trk = track.DeepSortTracker(4, streams=2, device=None)
    with pytest.raises(CenterposeHipError, match="without a device"):
        trk.row_ids(None, 5)
