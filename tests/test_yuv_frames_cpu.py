"""CPU: the host side of device frames in NV12 / NV21 / I420 -- the one copy of the YUV -> BGR arithmetic (csrc/yuv_arith.h, through
cp_yuv_to_bgr_host) against the NumPy reference of tests/yuv_ref.py on hand anchors and on all 2^24 triples, the descriptor struct and
the new C-ABI symbols, the pure function that turns plane shapes and strides into the addressing fields of cp_yuv_frame_desc, and
the argument checks that come before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import yuv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_built():
    import __graft_entry__ as g
    g.build()
    from centerpose_amd import _lib
    return _lib.lib()


def _detector(arch="dla_34", **overrides):
    """A MultiPoseDetector without a model or a device (what is tested here stops before any launch)."""
    from centerpose_amd import config, detector
    det = object.__new__(detector.MultiPoseDetector)
    det.cfg = config.get_cfg(arch, **overrides)
    det.scales = det.cfg.TEST.TEST_SCALES
    det.num_classes = 1
    det.model = type("Model", (), {"process": None})()
    det.mean = np.array(det.cfg.DATASET.MEAN, dtype=np.float32).reshape(1, 1, 3)
    det.std = np.array(det.cfg.DATASET.STD, dtype=np.float32).reshape(1, 1, 3)
    return det


def _host_convert(L, y, u, v, coef):
    y, u, v = (np.ascontiguousarray(a, np.uint8).reshape(-1) for a in (y, u, v))
    out = np.empty((y.size, 3), np.uint8)
    rc = L.cp_yuv_to_bgr_host(y.ctypes.data_as(ctypes.c_void_p), u.ctypes.data_as(ctypes.c_void_p), v.ctypes.data_as(ctypes.c_void_p),
                              ctypes.c_size_t(y.size), (ctypes.c_int * 6)(*coef), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, L.cp_last_error()
    return out


# ---------------------------------------------------------------- 1. hand anchors
def test_hand_anchors_through_the_reference_and_the_library():
    L = _lib_built()
    from centerpose_amd import detector
    assert detector.YUV_MATRICES == yuv_ref.COEF
    assert len(yuv_ref.ANCHORS) == 5
    yuv = np.array([a for a, _ in yuv_ref.ANCHORS], np.uint8)
    want = np.array([b for _, b in yuv_ref.ANCHORS], np.uint8)
    assert np.array_equal(yuv_ref.to_bgr(yuv[:, 0], yuv[:, 1], yuv[:, 2], yuv_ref.COEF["bt601"]), want)
    assert np.array_equal(_host_convert(L, yuv[:, 0], yuv[:, 1], yuv[:, 2], yuv_ref.COEF["bt601"]), want)
    # every shipped entry is round(k * 2^20) of the published limited-range coefficients
    for name, ks in (("bt601", (1.164, 1.596, -0.813, -0.391, 2.018)), ("bt709", (1.164, 1.793, -0.533, -0.213, 2.112))):
        assert yuv_ref.COEF[name] == tuple(int(round(k * (1 << 20))) for k in ks) + (16,), name


# ---------------------------------------------------------------- 2. all 2^24 triples
@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_library_equals_reference_on_all_triples(matrix):
    L = _lib_built()
    coef = yuv_ref.COEF[matrix]
    u, v = (a.reshape(-1).astype(np.uint8) for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    clamped = np.zeros(2, np.int64)
    for lo in range(0, 256, 32):                              # 32 luma values x 65536 chroma pairs per slice
        y = np.repeat(np.arange(lo, lo + 32, dtype=np.uint8), u.size)
        uu, vv = np.tile(u, 32), np.tile(v, 32)
        want = yuv_ref.to_bgr(y, uu, vv, coef)
        got = _host_convert(L, y, uu, vv, coef)
        bad = np.nonzero((got != want).any(1))[0]
        assert bad.size == 0, (matrix, int(y[bad[0]]), int(uu[bad[0]]), int(vv[bad[0]]), got[bad[0]], want[bad[0]])
        clamped += (int((want == 0).sum()), int((want == 255).sum()))
    # both clamps are exercised, each on well over a tenth of the 3 * 2^24 channels
    assert clamped.min() > 3 * (1 << 24) // 10, clamped


# ---------------------------------------------------------------- 3. descriptor and symbols
def test_yuv_frame_desc_size_fields_and_symbols():
    L = _lib_built()
    from centerpose_amd import detector
    hdr = open(os.path.join(ROOT, "include", "centerpose_hip.h")).read()
    assert L.cp_sizeof_yuv_frame_desc() == detector.YUV_FRAME_DESC.itemsize == 136
    assert detector.YUV_FRAME_DESC.itemsize % 8 == 0                                      # the table upload packs 8-byte items
    assert re.search(r"typedef struct cp_yuv_frame_desc \{\s*/\* 136 bytes \*/", hdr)
    for sym in ("cp_sizeof_yuv_frame_desc", "cp_preprocess_yuv_frames_u8_f32", "cp_yuv_to_bgr_host"):
        assert re.search(r"\b%s\s*\(" % sym, hdr) and hasattr(L, sym), sym
    assert L.cp_abi_version() == 4
    body = re.search(r"typedef struct cp_yuv_frame_desc \{(.*?)\} cp_yuv_frame_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"[\[\]\d\*\s]", "", f) for decl in re.findall(r"(?:const unsigned char\*|long long|int|double) ([^;]+);", body)
              for f in decl.split(",")]
    assert fields == list(detector.YUV_FRAME_DESC.names)
    assert fields[:7] == ["y_base", "y_row", "y_pix", "u_base", "v_base", "c_row", "c_pix"]
    # the fields shared with cp_frame_desc keep their order and (from mid_off on) their relative offsets
    shared = ["mid_off", "H", "W", "NH", "NW", "mi", "slot"]
    assert fields[7:14] == shared
    off = lambda dt, n: dt.fields[n][1] - dt.fields["mid_off"][1]
    assert all(off(detector.YUV_FRAME_DESC, n) == off(detector.FRAME_DESC, n) for n in shared)


# ---------------------------------------------------------------- 4. yuv_frame_geometry
def _geom(planes, color, with_dtypes=True):
    from centerpose_amd import detector
    planes = planes if isinstance(planes, (tuple, list)) else [planes]
    return detector.yuv_frame_geometry([t.shape for t in planes], [t.stride() for t in planes], color,
                                       [t.dtype for t in planes] if with_dtypes else None)


def _u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def test_geometry_of_contiguous_planes():
    H, W = 36, 52
    for color, (u_off, v_off) in (("nv12", (0, 1)), ("nv21", (1, 0))):
        got = _geom((_u8(H, W), _u8(H // 2, W // 2, 2)), color)
        assert got == (H, W, W, 1, u_off, v_off, W, 2), color
        assert abs(got[4] - got[5]) == 1                                                  # the bases differ by exactly one byte
    assert _geom((_u8(H, W), _u8(H // 2, W // 2), _u8(H // 2, W // 2)), "i420") == (H, W, W, 1, 0, 0, W // 2, 1)
    assert _geom((_u8(H, W), _u8(H // 2, W // 2, 2)), "nv12", with_dtypes=False)[0:2] == (H, W)


def test_geometry_of_a_pitched_surface_and_the_views_it_stands_for():
    H, W, pitch = 36, 52, 64
    alloc = torch.arange(H * 3 // 2 * pitch, dtype=torch.int64).remainder(251).to(torch.uint8).view(H * 3 // 2, pitch)
    surface = alloc[:, :W]
    assert surface.stride() == (pitch, 1)
    got = _geom(surface, "nv12")
    assert got == (H, W, pitch, 1, H * pitch, H * pitch + 1, pitch, 2)                    # chroma base: H * pitch bytes in
    assert _geom(surface, "nv21") == (H, W, pitch, 1, H * pitch + 1, H * pitch, pitch, 2)
    # the same numbers as the two plane views the library says it splits the surface into
    y, uv = surface[:H], surface[H:].unflatten(1, (W // 2, 2))
    assert _geom((y, uv), "nv12") == (H, W, pitch, 1, 0, 1, pitch, 2)
    assert uv.storage_offset() - y.storage_offset() == H * pitch
    # the rule itself, on bytes: U(r, c) and V(r, c) are found where the fields say
    flat = alloc.reshape(-1)
    for r, c in ((0, 0), (H - 1, W - 1), (11, 17), (12, 18)):
        assert int(flat[got[4] + (r >> 1) * got[6] + (c >> 1) * got[7]]) == int(uv[r >> 1, c >> 1, 0])
        assert int(flat[got[5] + (r >> 1) * got[6] + (c >> 1) * got[7]]) == int(uv[r >> 1, c >> 1, 1])
        assert int(flat[r * got[2] + c * got[3]]) == int(y[r, c])


def test_geometry_of_crops_odd_sizes_and_expanded_planes():
    big_y, big_uv = _u8(64, 80), _u8(32, 40, 2)
    y, uv = big_y[6:42, 8:60], big_uv[3:21, 4:30]                                         # an even-origin crop: 36 x 52 at (6, 8)
    assert _geom((y, uv), "nv12") == (36, 52, 80, 1, 0, 1, 80, 2)
    assert (y.storage_offset(), uv.storage_offset()) == (6 * 80 + 8, (3 * 40 + 4) * 2)
    # odd H / W: the chroma planes hold (H + 1) / 2 x (W + 1) / 2 samples
    assert _geom((_u8(37, 53), _u8(19, 27, 2)), "nv21") == (37, 53, 53, 1, 1, 0, 54, 2)
    assert _geom((_u8(37, 53), _u8(19, 27), _u8(19, 27)), "i420") == (37, 53, 53, 1, 0, 0, 27, 1)
    assert _geom((_u8(1, 9), _u8(1, 5, 2)), "nv12") == (1, 9, 9, 1, 0, 1, 10, 2)
    assert _geom((_u8(9, 1), _u8(5, 1), _u8(5, 1)), "i420") == (9, 1, 1, 1, 0, 0, 1, 1)
    # one chroma pair expanded over the frame (grey-world chroma): strides of 0
    assert _geom((_u8(36, 52), _u8(1, 1, 2).expand(18, 26, 2)), "nv12") == (36, 52, 52, 1, 0, 1, 0, 0)
    one = _u8(1, 1).expand(18, 26)
    assert _geom((_u8(36, 52), one, one), "i420") == (36, 52, 52, 1, 0, 0, 0, 0)
    assert _geom((_u8(1, 52).expand(36, 52), _u8(18, 26, 2)), "nv12")[2:4] == (0, 1)


def test_geometry_refusals():
    from centerpose_amd import detector
    from centerpose_amd._lib import CenterposeHipError
    g = detector.yuv_frame_geometry
    cases = [
        ("uv plane", lambda: _geom((_u8(36, 52), _u8(18, 26)), "nv12")),                             # a 2-D uv plane
        ("uv plane", lambda: _geom((_u8(36, 52), _u8(18, 25, 2)), "nv12")),
        ("uv plane", lambda: _geom((_u8(37, 53), _u8(18, 26, 2)), "nv21")),                          # floor instead of ceil
        ("u and v planes", lambda: _geom((_u8(36, 52), _u8(18, 26), _u8(18, 27)), "i420")),
        ("y plane", lambda: _geom((_u8(36, 52, 1), _u8(18, 26, 2)), "nv12")),
        ("got 3 tensors", lambda: _geom((_u8(36, 52), _u8(18, 26), _u8(18, 26)), "nv12")),
        ("got 2 tensors", lambda: _geom((_u8(36, 52), _u8(18, 26, 2)), "i420")),
        ("three planes", lambda: _geom(_u8(54, 52), "i420")),
        ("no pixels", lambda: _geom((_u8(0, 52), _u8(0, 26, 2)), "nv12")),
        ("uint8", lambda: _geom((_u8(36, 52), _u8(18, 26, 2).float()), "nv12")),
        ("uint8", lambda: g([(36, 52), (18, 26, 2)], [(52, 1), (52, 2, 1)], "nv12", [np.uint8, np.int16])),
        ("equal strides", lambda: _geom((_u8(36, 52), _u8(18, 26), _u8(18, 32)[:, :26]), "i420")),
        ("negative strides", lambda: g([(36, 52), (18, 26, 2)], [(52, 1), (-52, 2, 1)], "nv12")),
        ("negative strides", lambda: g([(54, 52)], [(52, -1)], "nv12")),
        ("even H and W", lambda: _geom(_u8(55, 52), "nv12")),                                        # rows not H * 3 / 2 of an even H
        ("even H and W", lambda: _geom(_u8(56, 52), "nv12")),
        ("even H and W", lambda: _geom(_u8(54, 51), "nv21")),                                        # W odd
        ("2-D tensor", lambda: _geom(_u8(54, 52, 1), "nv12")),
        ("unknown color", lambda: _geom((_u8(36, 52), _u8(18, 26, 2)), "yuv")),
        ("not planes", lambda: _geom((_u8(36, 52), _u8(18, 26, 2)), "bgr")),
    ]
    for match, call in cases:
        with pytest.raises(CenterposeHipError, match=match):
            call()
    with pytest.raises(CenterposeHipError, match="planes"):
        detector.frame_geometry((36, 52, 3), (156, 3, 1), "hwc", "nv12")


def test_refusals_of_the_entry_points_that_need_no_device():
    from centerpose_amd._lib import CenterposeHipError
    det = _detector()
    y, uv = _u8(8, 8), _u8(4, 4, 2)
    host = (np.zeros((8, 8), np.uint8), np.zeros((4, 4, 2), np.uint8))
    bgr = np.zeros((8, 8, 3), np.uint8)
    calls = lambda frame, **kw: (lambda: det.pre_process(frame, 1, **kw), lambda: det.pre_process_batch([frame], 1, **kw),
                                 lambda: det.run_batch([frame], **kw), lambda: det.run(frame, **kw))
    for match, frame, kw in [
        ("layout", (y, uv), dict(color="nv12", layout="chw")),                 # a layout other than the default with a YUV colour
        ("matrix", bgr, dict(matrix="bt709")),                                 # a matrix with BGR / RGB
        ("matrix", bgr, dict(color="rgb", matrix="bt709")),
        ("unknown matrix", (y, uv), dict(color="nv12", matrix="bt2020")),
        ("unknown matrix", bgr, dict(matrix="jpeg")),
        ("device", host, dict(color="nv12")),                                  # host planes
        ("device", host[0], dict(color="nv21")),                               # a host surface
        ("device", bgr, dict(color="i420")),
        ("cpu", (y, uv), dict(color="nv12")),                                  # planes that are tensors, but not on a GPU
        ("cpu", _u8(12, 8), dict(color="nv12")),
        ("unknown color", (y, uv), dict(color="yuv")),
        ("unknown color", (y, uv), dict(color="gray")),
        ("unknown color", (y, uv), dict(color="yv12")),
    ]:
        for call in calls(frame, **kw):
            with pytest.raises(CenterposeHipError, match=match):
                call()
    with pytest.raises(CenterposeHipError, match="mixed"):
        det.run_batch([host[0], (y, uv)], color="nv12")                        # host arrays and device frames in one call
    with pytest.raises(CenterposeHipError, match="mixed"):
        det.pre_process_batch([(y, host[1])], 1, color="nv12")                 # ... and in one frame
    with pytest.raises(CenterposeHipError, match="list of frames"):
        det.run_batch(torch.zeros((2, 12, 8), dtype=torch.uint8), color="nv12")
    assert det.run_batch([], color="nv12", matrix="bt709") == []


def test_yuv_table_addresses_the_planes_in_place():
    """The YUV_FRAME_DESC table of a mixed list: bases and strides are the planes' own, the geometry, matrix and scratch layout are
    those of the staging table for the same sizes."""
    _lib_built()                                               # cp_invert_warp is host code of the library
    from centerpose_amd import detector
    det = _detector("res_50")
    assert det.cfg.TEST.FIX_RES and det.cfg.TEST.FLIP_TEST
    frames = [(1000, 36, 52, 64, 1, 1000 + 36 * 64, 1001 + 36 * 64, 64, 2), (5000, 37, 53, 53, 1, 9000, 9500, 27, 1)]
    shapes = [f[1:3] for f in frames]
    for scale in (1, 0.5):
        table, scratch, inp_h, inp_w, metas = det._pre_table(shapes, None, [0, 1], scale, frames, True)
        ref, rscratch, rh, rw, rmetas = det._pre_table(shapes, [0, 0], [0, 1], scale)
        assert table.dtype == detector.YUV_FRAME_DESC and (scratch, inp_h, inp_w) == (rscratch, rh, rw)
        for name in ("mid_off", "H", "W", "NH", "NW", "mi", "slot"):
            assert np.array_equal(table[name], ref[name]), name
        for n, f in enumerate(frames):
            d = table[n]
            assert tuple(int(d[k]) for k in ("y_base", "H", "W", "y_row", "y_pix", "u_base", "v_base", "c_row", "c_pix")) == f


# ---------------------------------------------------------------- 5. argument checks before any launch
def _desc(**kw):
    from centerpose_amd import detector
    t = np.zeros(1, detector.YUV_FRAME_DESC)
    d = t[0]
    d["y_base"], d["y_row"], d["y_pix"], d["u_base"], d["v_base"], d["c_row"], d["c_pix"], d["mid_off"] = 4096, 8, 1, 8192, 8193, 8, 2, -1
    d["H"], d["W"], d["NH"], d["NW"], d["mi"], d["slot"] = 4, 8, 4, 8, (1, 0, 0, 0, 1, 0), 0
    for k, v in kw.items():
        d[k] = v
    return t


def _call(L, table, N=1, coef=yuv_ref.COEF["bt601"], scratch=None, scratch_bytes=0, out=4096, out_batch=1, flip=0):
    """cp_preprocess_yuv_frames_u8_f32 with addresses that are never dereferenced: only calls whose argument check fails are made."""
    mean = (ctypes.c_float * 3)(0.4, 0.4, 0.4)
    std = (ctypes.c_float * 3)(0.3, 0.3, 0.3)
    coef = (ctypes.c_int * 6)(*coef) if coef is not None else None
    return L.cp_preprocess_yuv_frames_u8_f32(ctypes.c_void_p(4096), table.ctypes.data_as(ctypes.c_void_p), N, coef, ctypes.c_void_p(scratch),
                                             ctypes.c_size_t(scratch_bytes), ctypes.c_void_p(out), out_batch, 8, 8, mean, std, flip, None)


@pytest.mark.parametrize("fields,message", [
    (dict(y_base=0), b"null base"),
    (dict(u_base=0), b"null base"),
    (dict(v_base=0), b"null base"),
    (dict(y_row=-8), b"negative stride"),
    (dict(y_pix=-1), b"negative stride"),
    (dict(c_row=-8), b"negative stride"),
    (dict(c_pix=-2), b"negative stride"),
    (dict(H=0), b"bad size"),
    (dict(W=-8), b"bad size"),
    (dict(H=1 << 15, W=1 << 14, NH=1 << 15, NW=1 << 14), b"bad size"),            # 2^29 pixels
    (dict(y_row=1 << 61), b"2^62"),                                              # 3 * 2^61 >= 2^62
    (dict(c_row=1 << 62), b"2^62"),                                              # the chroma plane alone: one chroma row down
    (dict(H=2, NH=2, NW=4, c_row=1 << 62), b"needs a scratch offset"),           # ... a 2-row frame never leaves chroma row 0: next check
    (dict(NH=2, NW=4), b"needs a scratch offset"),                               # a resize without a place for it
    (dict(NH=2, NW=4, mid_off=0), b"outside the scratch buffer"),
    (dict(slot=1), b"output slot"),
])
def test_argument_checks_come_before_any_launch(fields, message):
    """No device here: a call that got past its argument checks would fail to launch, with another message."""
    L = _lib_built()
    L.cp_last_error.restype = ctypes.c_char_p
    assert _call(L, _desc(**fields)) == 1
    assert message in L.cp_last_error(), L.cp_last_error()


def test_argument_checks_of_the_call_itself():
    L = _lib_built()
    L.cp_last_error.restype = ctypes.c_char_p
    assert _call(L, _desc(), N=65536) == 1 and b"65535" in L.cp_last_error()
    assert _call(L, _desc(), N=0) == 1
    assert _call(L, _desc(), out=None) == 1
    assert _call(L, _desc(), coef=None) == 1 and b"null coef" in L.cp_last_error()
    assert _call(L, _desc(), flip=1) == 1 and b"output slot" in L.cp_last_error()          # the twin needs slot + 1
    assert _call(L, _desc(NH=2, NW=4, mid_off=0), scratch=4096, scratch_bytes=23) == 1 and b"outside the scratch" in L.cp_last_error()


BT601 = yuv_ref.COEF["bt601"]


@pytest.mark.parametrize("coef,message", [
    ((0,) + BT601[1:], b"CY must be positive"),
    ((-1220542,) + BT601[1:], b"CY must be positive"),
    (BT601[:5] + (-1,), b"YOFF"),
    (BT601[:5] + (256,), b"YOFF"),
    ((1 << 23,) + BT601[1:], b"overflow"),                                       # 255 * 2^23 alone is 2^31 - 2^23: the rest tips it
    (BT601[:1] + (-(1 << 24),) + BT601[2:], b"overflow"),                        # |CVR|: 128 * 2^24 = 2^31
    (BT601[:2] + (-(1 << 23), -(1 << 23)) + BT601[4:], b"overflow"),             # |CVG| + |CUG| counts as one term
    (BT601[:4] + (1 << 24, 16), b"overflow"),                                    # |CUB|
    (BT601[:4] + (-2147483648, 16), b"overflow"),                                # INT_MIN has no int32 absolute value
])
def test_coef_that_could_overflow_is_refused_before_any_launch(coef, message):
    L = _lib_built()
    L.cp_last_error.restype = ctypes.c_char_p
    assert _call(L, _desc(), coef=coef) == 1
    assert message in L.cp_last_error(), L.cp_last_error()
    y = np.zeros(1, np.uint8)
    out = np.zeros(3, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.cp_yuv_to_bgr_host(p(y), p(y), p(y), ctypes.c_size_t(1), (ctypes.c_int * 6)(*coef), p(out)) == 1
    assert message in L.cp_last_error()


def test_the_overflow_bound_is_the_stated_one():
    """The largest matrix the condition admits is accepted (the call then fails later, at the descriptor), one more is refused."""
    L = _lib_built()
    L.cp_last_error.restype = ctypes.c_char_p
    cy = 1220542
    room = ((1 << 31) - 1 - 255 * cy - (1 << 19)) // 128                          # 255*CY + 2^19 + 128*room < 2^31
    assert 255 * cy + (1 << 19) + 128 * room < (1 << 31) <= 255 * cy + (1 << 19) + 128 * (room + 1)
    bad_desc = _desc(y_base=0)
    for coef in ((cy, room, 0, 0, 0, 16), (cy, 0, -(room // 2), room - room // 2, 0, 16), (cy, 0, 0, 0, -room, 0)):
        assert _call(L, bad_desc, coef=coef) == 1 and b"null base" in L.cp_last_error(), coef
    for coef in ((cy, room + 1, 0, 0, 0, 16), (cy, 0, -(room // 2) - 1, room - room // 2, 0, 16), (cy, 0, 0, 0, -room - 1, 255)):
        assert _call(L, bad_desc, coef=coef) == 1 and b"overflow" in L.cp_last_error(), coef
