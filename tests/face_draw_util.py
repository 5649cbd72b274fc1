"""What the face-overlay tests share on the library's side: the style record and the call of the HOST painters
(cp_face_draw_frames_host / cp_face_draw_yuv_frames_host) on copies of the forms' buffers."""
import numpy as np

import draw_ref
import draw_util
import face_draw_ref as fdr


def style_struct(style, yuv, matrix="bt601"):
    from centerpose_amd import draw
    rec = np.zeros(1, draw.FACE_STYLE)
    for k in ("landmarks", "vertices", "pose_box"):
        rec[k] = int(style[k])
    for k in ("landmark_radius", "line_radius", "box_radius", "vertex_radius", "vertex_step"):
        rec[k] = style[k]
    colors = [style["landmark_color"], style["line_color"], style["vertex_color"], style["box_color"]]
    rec["colors"][0, :, :3] = np.asarray(draw_ref.bgr_to_yuv(colors, matrix) if yuv else colors, np.uint8)
    rec["colors"][0, :, 3] = 0xA5                              # never stored anywhere
    return rec


def host_paint(L, forms, faces, style, matrix="bt601", with_pose=True, with_pos=True):
    """-> (rc, the painted copies of the forms' buffers)"""
    yuv = forms[0]["color"] not in ("bgr", "rgb")
    bufs = [f["buf"].copy() for f in forms]
    table = draw_util.table_of(forms, [b.ctypes.data for b in bufs])
    a = {k: np.ascontiguousarray(v) for k, v in faces.items()}
    st = style_struct(style, yuv, matrix)
    fn = L.cp_face_draw_yuv_frames_host if yuv else L.cp_face_draw_frames_host
    rc = fn(table.ctypes.data, len(forms), a["slots"].ctypes.data, len(a["slots"]), a["landmarks"].ctypes.data,
            a["box"].ctypes.data if with_pose else None, a["valid"].ctypes.data if with_pose else None,
            a["pos"].ctypes.data if with_pos else None, a["face_ind"].ctypes.data if with_pos else None, len(a["face_ind"]), st.ctypes.data)
    return rc, bufs


def forms_of(H, W, seed=900):
    return draw_ref.bgr_forms(seed, H, W), draw_ref.yuv_forms(seed + 50, H, W)
