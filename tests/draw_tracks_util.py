"""What the draw_tracks tests share on the library's side: the item table for the items of tests/draw_tracks_ref.py and the calls of
the HOST painters (cp_draw_tracks_*_host, cp_draw_rows_ids_*_host) on copies of the forms' buffers."""
import ctypes

import numpy as np

import draw_ref
import draw_tracks_ref as tref
import draw_util

VP = ctypes.c_void_p


def item_table(per_frame, yuv=False, matrix="bt601", Kmax=None):
    """per_frame: a list of item lists -> (TRACK_ITEM [N, Kmax], counts int32 [N]); colours as (Y, U, V) for YUV frames."""
    from centerpose_amd import detector
    N = len(per_frame)
    Kmax = max([len(p) for p in per_frame] + [0]) if Kmax is None else Kmax
    items = np.zeros((N, Kmax), detector.TRACK_ITEM)
    items["color"][..., 3] = 0xA5                               # never stored anywhere
    items["text_color"][..., 3] = 0x5A
    counts = np.array([len(p) for p in per_frame], np.int32)
    conv = (lambda c: draw_ref.bgr_to_yuv([c], matrix)[0]) if yuv else (lambda c: c)
    for n, frame_items in enumerate(per_frame):
        for k, it in enumerate(frame_items):
            rec = items[n, k]
            rec["x0"], rec["y0"], rec["x1"], rec["y1"] = it["x0"], it["y0"], it["x1"], it["y1"]
            rec["color"][:3], rec["text_color"][:3] = conv(it["color"]), conv(it["text_color"])
            rec["nchars"] = len(it["text"])
            rec["glyph"][:len(it["text"])] = [tref.CHARSET.index(c) for c in it["text"]]
            rec["glyph"][len(it["text"]):] = 0xFF              # behind nchars: never read
    return items, counts


def is_yuv(form):
    return form["color"] not in ("bgr", "rgb")


def host_paint_tracks(L, forms, per_frame, T, s, matrix="bt601", bufs=None):
    """The host painter over copies of the forms' buffers (or over `bufs`, in place) -> the painted buffers."""
    yuv = is_yuv(forms[0])
    bufs = [f["buf"].copy() for f in forms] if bufs is None else bufs
    table = draw_util.table_of(forms, [b.ctypes.data for b in bufs])
    items, counts = item_table(per_frame, yuv, matrix)
    fn = L.cp_draw_tracks_yuv_frames_host if yuv else L.cp_draw_tracks_frames_host
    rc = fn(table.ctypes.data_as(VP), len(forms), items.ctypes.data_as(VP), counts.ctypes.data_as(VP), items.shape[1], T, s)
    assert rc == 0, L.cp_last_error()
    return bufs


def id_palette_struct(colors, yuv=False, matrix="bt601"):
    rec = np.zeros(1, np.dtype([("count", "<i4"), ("colors", "u1", (64, 4))]))
    rec["count"] = len(colors)
    rec["colors"][0, :len(colors), :3] = np.asarray(draw_ref.bgr_to_yuv(colors, matrix) if yuv else colors, np.uint8)
    rec["colors"][0, :, 3] = 0xA5
    rec["colors"][0, len(colors):, :3] = 0x11                   # behind count: never stored
    return rec


def host_paint_rows_ids(L, forms, rows, ids, id_palette, vis, T, RL, RJ, palette, matrix="bt601", bufs=None):
    """cp_draw_rows_ids_*_host over copies of the forms' buffers (or `bufs`, in place).  rows [N, M, 56], ids int32 [N, M]."""
    yuv = is_yuv(forms[0])
    bufs = [f["buf"].copy() for f in forms] if bufs is None else bufs
    table = draw_util.table_of(forms, [b.ctypes.data for b in bufs])
    rows = np.ascontiguousarray(rows, np.float32).reshape(len(forms), -1, 56)
    ids = np.ascontiguousarray(ids, np.int32).reshape(len(forms), -1)
    st = draw_util.style_struct(T, RL, RJ, draw_ref.bgr_to_yuv(palette, matrix) if yuv else palette)
    idp = id_palette_struct(id_palette, yuv, matrix)
    fn = L.cp_draw_rows_ids_yuv_frames_host if yuv else L.cp_draw_rows_ids_frames_host
    rc = fn(table.ctypes.data_as(VP), len(forms), rows.ctypes.data_as(VP), rows.shape[1], ctypes.c_float(vis), st.ctypes.data_as(VP),
            ids.ctypes.data_as(VP), idp.ctypes.data_as(VP))
    assert rc == 0, L.cp_last_error()
    return bufs


def host_row_ids(L, slots, slot_ids, capacity, S, q, M):
    """cp_track_row_ids_host -> (rc, int32 [S, M] that started as a sentinel)."""
    slots, slot_ids = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(slot_ids, np.int32)
    out = np.full((S, M), -99, np.int32)
    rc = L.cp_track_row_ids_host(slots.ctypes.data_as(VP), slot_ids.ctypes.data_as(VP), capacity, S, q, M, out.ctypes.data_as(VP))
    return rc, out


def row_ids_case(seed, S, q, M, capacity):
    """(slots int32 [capacity], slot_ids int32 [S * q], want int32 [S, M]): distinct rows per stream, unused slots, unmatched slots."""
    r = np.random.RandomState(seed)
    slots = np.full(capacity, -1, np.int32)
    slots[S * q:] = r.randint(0, max(S * M, 1), capacity - S * q)      # behind S * q: never read
    slot_ids = np.full(S * q, -1, np.int32)
    want = np.full((S, M), -1, np.int32)
    for s_ in range(S):
        picks = r.permutation(M)[:min(q, M)]
        for j, m in enumerate(picks):
            if r.rand() < 0.25:
                continue                                       # an unused slot
            slots[s_ * q + j] = s_ * M + m
            if r.rand() < 0.7:
                slot_ids[s_ * q + j] = int(r.randint(0, 2 ** 31 - 1))
                want[s_, m] = slot_ids[s_ * q + j]
        for j in range(len(picks), q):                         # q > M: the slots beyond the rows are unused, some with a stale id
            slot_ids[s_ * q + j] = int(r.randint(-1, 50))
    return slots, slot_ids, want
