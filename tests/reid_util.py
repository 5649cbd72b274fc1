"""What the re-id tests share on the library's side: the norm record and the calls of the HOST twins (cp_reid_select_rows_host /
cp_reid_crop_frames_host / cp_reid_crop_yuv_frames_host) over the forms of tests/draw_ref.py, addressed by descriptor."""
import ctypes

import numpy as np

import draw_util
import yuv_ref

GUARD = 257          # floats behind the crop buffer that no call may touch
VP = ctypes.c_void_p


def norm_struct(scale=1.0, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), channel_order="bgr"):
    from centerpose_amd import reid
    rec = np.zeros(1, reid.REID_NORM)
    rec["scale"], rec["mean"], rec["std"], rec["rgb"] = scale, mean, std, ("bgr", "rgb").index(channel_order)
    return rec


def is_yuv(forms):
    return forms[0]["color"] not in ("bgr", "rgb")


def host_select(L, forms, rows, vis_thresh, cap, table=None):
    """-> (rc, slots [cap], counts [N]); the arrays start as a sentinel so that an unwritten entry shows."""
    N, M = rows.shape[:2]
    table = draw_util.table_of(forms, [f["buf"].ctypes.data for f in forms]) if table is None else table
    rows = np.ascontiguousarray(rows, np.float32)
    slots, counts = np.full(max(cap, 1), -7, np.int32), np.full(max(N, 1), -7, np.int32)
    rc = L.cp_reid_select_rows_host(table.ctypes.data_as(VP), int(is_yuv(forms)), N, rows.ctypes.data_as(VP), M, ctypes.c_float(vis_thresh), cap,
                                    slots.ctypes.data_as(VP), counts.ctypes.data_as(VP))
    return rc, slots, counts


def host_crop(L, forms, rows, vis_thresh, slots, cap, matrix="bt601", **norm):
    """-> (rc, out float32 [cap * 3 * 128 * 64 + GUARD], NaN-filled before the call)."""
    N, M = rows.shape[:2]
    table = draw_util.table_of(forms, [f["buf"].ctypes.data for f in forms])
    rows = np.ascontiguousarray(rows, np.float32)
    slots = np.ascontiguousarray(slots, np.int32)
    out = np.full(cap * 3 * 128 * 64 + GUARD, np.nan, np.float32)
    nm = norm_struct(**norm)
    if is_yuv(forms):
        coef = (ctypes.c_int * 6)(*yuv_ref.COEF[matrix])
        rc = L.cp_reid_crop_yuv_frames_host(table.ctypes.data_as(VP), N, coef, rows.ctypes.data_as(VP), M, ctypes.c_float(vis_thresh),
                                            slots.ctypes.data_as(VP), cap, nm.ctypes.data_as(VP), out.ctypes.data_as(VP))
    else:
        rc = L.cp_reid_crop_frames_host(table.ctypes.data_as(VP), N, rows.ctypes.data_as(VP), M, ctypes.c_float(vis_thresh),
                                        slots.ctypes.data_as(VP), cap, nm.ctypes.data_as(VP), out.ctypes.data_as(VP))
    return rc, out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
