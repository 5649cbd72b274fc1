"""What the overlay tests share on the library's side: the cp_draw_overlay record from raw values and the call of the HOST painters
(cp_draw_overlay_frames_host / cp_draw_overlay_yuv_frames_host) on copies of the forms' buffers."""
import ctypes

import numpy as np

import draw_overlay_ref as oref
import draw_ref
import draw_tracks_ref as tref
import draw_tracks_util
import draw_util

VP = ctypes.c_void_p


def lib(build=True):
    L = draw_util.lib_built() if build else draw_util.lib_loaded()
    L.cp_draw_overlay_scratch_bytes.restype = ctypes.c_size_t
    return L


def overlay_struct(opacity=(256, 256, 256), label_scale=0, prefix="", text_color3=(0, 0, 0), nprefix=None):
    """One DRAW_OVERLAY record from raw values (no range check: refusals are the library's to make)."""
    from centerpose_amd import draw
    rec = np.zeros(1, draw.DRAW_OVERLAY)
    rec["opacity"][0] = opacity
    rec["label_scale"] = label_scale
    rec["prefix"][0, :] = 0xFF                                  # behind nprefix: never read
    glyphs = [tref.CHARSET.index(c) for c in prefix] if isinstance(prefix, str) else list(prefix)
    rec["prefix"][0, :len(glyphs)] = glyphs
    rec["nprefix"] = len(glyphs) if nprefix is None else nprefix
    rec["text_color"][0, :3] = text_color3
    rec["text_color"][0, 3] = 0x5A                              # never stored anywhere
    return rec


def host_paint(L, forms, rows, vis, T, RL, RJ, palette, opacity=(256, 256, 256), label_scale=0, prefix="PERSON", text_color=(0, 0, 0), ids=None,
               id_palette=None, matrix="bt601"):
    """The overlay host painter over copies of the forms' buffers -> the painted buffers.  rows [N, M, 56]; ids int32 [N, M] or None;
    colours (B, G, R), converted for YUV forms by the reference's formulas."""
    yuv = draw_tracks_util.is_yuv(forms[0])
    conv = (lambda cols: draw_ref.bgr_to_yuv(cols, matrix)) if yuv else (lambda cols: cols)
    bufs = [f["buf"].copy() for f in forms]
    table = draw_util.table_of(forms, [b.ctypes.data for b in bufs])
    rows = np.ascontiguousarray(rows, np.float32).reshape(len(forms), -1, 56)
    st = draw_util.style_struct(T, RL, RJ, conv(palette))
    ov = overlay_struct(opacity, label_scale, prefix, conv([text_color])[0])
    ids_p = idp_p = None
    if ids is not None:
        ids = np.ascontiguousarray(ids, np.int32).reshape(len(forms), -1)
        idp = draw_tracks_util.id_palette_struct(id_palette, yuv, matrix)
        ids_p, idp_p = ids.ctypes.data_as(VP), idp.ctypes.data_as(VP)
    fn = L.cp_draw_overlay_yuv_frames_host if yuv else L.cp_draw_overlay_frames_host
    rc = fn(table.ctypes.data_as(VP), len(forms), rows.ctypes.data_as(VP), rows.shape[1], ctypes.c_float(vis), st.ctypes.data_as(VP), ids_p, idp_p,
            ov.ctypes.data_as(VP))
    assert rc == 0, L.cp_last_error()
    return bufs


def case_inputs(kind, s, f, k):
    """What style k of oref.STYLES paints on form f of size s: (rows, vis, (T, RL, RJ, palette), ids, id_palette, text colour).
    Every third style takes scores of both signs and up to three digits."""
    H, W = draw_ref.SIZES[s]
    seed = 1000 * s + 10 * f + k + (500 if kind == "yuv" else 0)
    rows, vis = (oref.wide_score_rows(seed, 12, H, W), -1000.0) if k % 3 == 2 else (draw_ref.fuzz_rows(seed, 12, H, W), draw_ref.VIS)
    return rows, vis, draw_ref.fuzz_style(seed), tref.fuzz_ids(seed + 1, 12), tref.fuzz_id_palette(seed + 2, 1 + seed % 64), oref.text_color(seed)
