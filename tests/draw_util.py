"""What the draw_results tests share on the library's side: descriptor tables for the forms of tests/draw_ref.py and the call of the
HOST painters (cp_draw_rows_frames_host / cp_draw_rows_yuv_frames_host) on a copy of a form's buffer."""
import ctypes

import numpy as np

import draw_ref


def lib_built():
    import __graft_entry__ as g
    g.build()
    from centerpose_amd import _lib
    L = _lib.lib()
    L.cp_draw_scratch_bytes.restype = ctypes.c_size_t
    return L


def lib_loaded():
    """The library as it was built, without building (GPU tests)."""
    from centerpose_amd import _lib
    L = _lib.lib()
    L.cp_draw_scratch_bytes.restype = ctypes.c_size_t
    return L


def style_struct(thickness, limb_radius, joint_radius, palette3):
    """One DRAW_STYLE record from raw values (no range check: refusals are the library's to make); palette3: 36 triples."""
    from centerpose_amd import detector
    rec = np.zeros(1, detector.DRAW_STYLE)
    rec["box_thickness"], rec["limb_radius"], rec["joint_radius"] = thickness, limb_radius, joint_radius
    rec["palette"][0, :, :3] = np.asarray(palette3, np.uint8)
    rec["palette"][0, :, 3] = 0xA5                              # never stored anywhere
    return rec


def describe(form, address):
    """One descriptor record (FRAME_DESC or YUV_FRAME_DESC) for `form` with its buffer at `address`, by the detector's pure geometry
    functions -- what BaseDetector._frame / _yuv_frame do with a tensor's shape, strides and data pointer."""
    from centerpose_amd import detector
    views = form["views"]
    if form["color"] in ("bgr", "rgb"):
        off, shape, strides = views[0]
        H, W, row, pix, ch = detector.frame_geometry(shape, strides, form["layout"], form["color"])
        d = np.zeros(1, detector.FRAME_DESC)
        d["base"], d["row_stride"], d["pix_stride"], d["ch_off"] = address + off, row, pix, ch
    else:
        H, W, y_row, y_pix, u_off, v_off, c_row, c_pix = detector.yuv_frame_geometry([v[1] for v in views], [v[2] for v in views], form["color"])
        d = np.zeros(1, detector.YUV_FRAME_DESC)
        u_plane, v_plane = (views[0][0], views[0][0]) if len(views) == 1 else (views[1][0], views[-1][0])
        d["y_base"], d["y_row"], d["y_pix"] = address + views[0][0], y_row, y_pix
        d["u_base"], d["v_base"], d["c_row"], d["c_pix"] = address + u_plane + u_off, address + v_plane + v_off, c_row, c_pix
    d["H"], d["W"], d["NH"], d["NW"], d["mid_off"] = H, W, H, W, -1
    return d


def table_of(forms, addresses):
    return np.ascontiguousarray(np.concatenate([describe(f, a) for f, a in zip(forms, addresses)]))


def host_paint(L, forms, rows, vis_thresh, thickness, limb_radius, joint_radius, palette, matrix="bt601"):
    """The host painter over copies of the forms' buffers (all BGR / RGB forms or all YUV forms) -> the painted buffers.  rows:
    float32 [N, M, 56]; palette: 36 (B, G, R), converted for YUV forms by the reference's formulas."""
    yuv = forms[0]["color"] not in ("bgr", "rgb")
    bufs = [f["buf"].copy() for f in forms]
    table = table_of(forms, [b.ctypes.data for b in bufs])
    rows = np.ascontiguousarray(rows, np.float32).reshape(len(forms), -1, 56)
    st = style_struct(thickness, limb_radius, joint_radius, draw_ref.bgr_to_yuv(palette, matrix) if yuv else palette)
    fn = L.cp_draw_rows_yuv_frames_host if yuv else L.cp_draw_rows_frames_host
    rc = fn(table.ctypes.data_as(ctypes.c_void_p), len(forms), rows.ctypes.data_as(ctypes.c_void_p), rows.shape[1], ctypes.c_float(vis_thresh),
            st.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, L.cp_last_error()
    return bufs
