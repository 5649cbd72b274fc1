"""CPU: the host side of YUV device frames beyond 8-bit 4:2:0 limited range (P010 / P016, i422, i444, i400, yuyv / uyvy; the full-range
and BT.2020 matrices) -- the matrix rows against the closed form, the 16-bit conversion rule (csrc/yuv_source.h through
cp_yuv16_to_bgr_host) against the 8-bit one on all 2^24 triples and against the NumPy reference of tests/yuv_surface_ref.py on random
16-bit triples, the geometry and descriptor tables of every new form, the re-id host twins on such frames, and every refusal that
needs no device.  Every comparison is bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import draw_ref
import draw_util
import reid_ref
import reid_util
import yuv_ref
import yuv_surface_ref as ysr

VP = ctypes.c_void_p
ISSUE_ROWS = {"bt601-full": (1048576, 1470104, -748826, -360853, 1858077, 0), "bt709-full": (1048576, 1651297, -490864, -196424, 1945738, 0),
              "bt2020-limited": (1220945, 1760217, -682019, -196426, 2245811, 16), "bt2020-full": (1048576, 1546230, -599107, -172546, 1972791, 0)}
MATRICES = ["bt601", "bt709"] + sorted(ISSUE_ROWS)


@functools.lru_cache(maxsize=None)
def _lib_built():
    L = draw_util.lib_built()                                 # builds once per run of this file
    L.cp_last_error.restype = ctypes.c_char_p
    return L


def _convert(L, fn, y, u, v, coef):
    dt = np.uint16 if fn == "cp_yuv16_to_bgr_host" else np.uint8
    y, u, v = (np.ascontiguousarray(a, dt).reshape(-1) for a in (y, u, v))
    out = np.empty((y.size, 3), np.uint8)
    rc = getattr(L, fn)(y.ctypes.data_as(VP), u.ctypes.data_as(VP), v.ctypes.data_as(VP), ctypes.c_size_t(y.size), (ctypes.c_int * 6)(*coef),
                        out.ctypes.data_as(VP))
    assert rc == 0, L.cp_last_error()
    return out


# ---------------------------------------------------------------- 1. matrices
def test_matrix_rows_equal_the_closed_form():
    from centerpose_amd import detector, frames
    assert ysr.NEW_COEF == ISSUE_ROWS
    assert frames.SURFACE_MATRICES == ISSUE_ROWS and detector.SURFACE_MATRICES is frames.SURFACE_MATRICES
    assert detector.YUV_MATRICES == yuv_ref.COEF                      # the two old names keep cv2's three-decimal rows ...
    assert ysr.closed_form(0.299, 0.114, False) != yuv_ref.COEF["bt601"]      # ... which are not the closed form
    for name in MATRICES:
        assert frames.yuv_coef(name) == ysr.COEF[name], name
    # every row satisfies the overflow condition of csrc/yuv_arith.h: the host conversion takes it
    L = _lib_built()
    for name, row in ISSUE_ROWS.items():
        cy, cvr, cvg, cug, cub, yoff = row
        assert 255 * cy + (1 << 19) + 128 * max(abs(cvr), abs(cvg) + abs(cug), abs(cub)) < 1 << 31, name
        _convert(L, "cp_yuv_to_bgr_host", [16], [128], [128], row)


def test_hand_anchors_of_the_16_bit_rule():
    L = _lib_built()
    # 10-bit studio black and white, ten bits in the MSBs; the low six bits count
    y, c = np.array([64 << 6, 940 << 6, (64 << 6) | 63], np.uint16), np.full(3, 512 << 6, np.uint16)
    for name in ("bt601", "bt709", "bt2020-limited"):
        want = ysr.to_bgr16(y, c, c, ysr.COEF[name])
        assert want[:2].tolist() == [[0, 0, 0], [255, 255, 255]], name
        assert np.array_equal(_convert(L, "cp_yuv16_to_bgr_host", y, c, c, ysr.COEF[name]), want)
    # full range: Y alone is the grey level, rounded from 16 to 8 bits
    full = ysr.to_bgr16(np.array([0, 65535, 32768 + 127, 32768 + 128], np.uint16), np.full(4, 32768, np.uint16), np.full(4, 32768, np.uint16),
                        ysr.COEF["bt601-full"])
    assert full[:, 0].tolist() == [0, 255, 128, 129]
    # the low bits of a P010 sample change the result somewhere
    y, u, v = (np.random.RandomState(k).randint(0, 1024, 4096).astype(np.uint16) << 6 for k in range(3))
    assert (ysr.to_bgr16(y | 63, u | 63, v | 63, ysr.COEF["bt709"]) != ysr.to_bgr16(y, u, v, ysr.COEF["bt709"])).any()


@pytest.mark.parametrize("matrix", MATRICES)
def test_16_bit_rule_on_x_shl_8_equals_the_8_bit_rule_on_all_triples(matrix):
    L = _lib_built()
    coef = ysr.COEF[matrix]
    u, v = (a.reshape(-1).astype(np.uint8) for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    for lo in range(0, 256, 32):                              # 32 luma values x 65536 chroma pairs per slice: all 2^24 triples
        y = np.repeat(np.arange(lo, lo + 32, dtype=np.uint8), u.size)
        uu, vv = np.tile(u, 32), np.tile(v, 32)
        want = _convert(L, "cp_yuv_to_bgr_host", y, uu, vv, coef)
        got = _convert(L, "cp_yuv16_to_bgr_host", y.astype(np.uint16) << 8, uu.astype(np.uint16) << 8, vv.astype(np.uint16) << 8, coef)
        bad = np.nonzero((got != want).any(1))[0]
        assert bad.size == 0, (matrix, int(y[bad[0]]), int(uu[bad[0]]), int(vv[bad[0]]), got[bad[0]], want[bad[0]])
        if lo == 96:                                          # the 8-bit rule itself, for the new rows, against NumPy
            assert np.array_equal(want, ysr.to_bgr8(y, uu, vv, coef))


@pytest.mark.parametrize("matrix", MATRICES)
def test_16_bit_rule_on_random_triples_equals_the_reference(matrix):
    L = _lib_built()
    rs = np.random.RandomState(MATRICES.index(matrix))
    y, u, v = (rs.randint(0, 1 << 16, size=1 << 22).astype(np.uint16) for _ in range(3))
    assert (y & 63).any() and (u & 63).any() and (v & 63).any()                           # low bits set
    y[:4], u[:4], v[:4] = (0, 65535, 0, 65535), (0, 0, 65535, 65535), (65535, 0, 0, 65535)
    want = ysr.to_bgr16(y, u, v, ysr.COEF[matrix])
    got = _convert(L, "cp_yuv16_to_bgr_host", y, u, v, ysr.COEF[matrix])
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, (matrix, int(y[bad[0]]), int(u[bad[0]]), int(v[bad[0]]), got[bad[0]], want[bad[0]])
    assert (want == 0).any() and (want == 255).any() and ((want > 0) & (want < 255)).any()


def test_symbols_and_the_header():
    import os
    import re
    L = _lib_built()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "centerpose_hip.h")).read()
    assert re.search(r"\bcp_yuv16_to_bgr_host\s*\(", hdr) and hasattr(L, "cp_yuv16_to_bgr_host")
    assert "preprocess_yuv_surfaces_kernel<vec4|scalar>" in hdr and "reid_crop_kernel<surfaces>" in hdr
    assert L.cp_sizeof_yuv_frame_desc() == 136 and L.cp_abi_version() == 4


# ---------------------------------------------------------------- 2. geometry and tables
def _z(dtype, *shape):
    return torch.zeros(shape, dtype=dtype)


def _geom(planes, color, with_dtypes=True):
    from centerpose_amd import frames
    planes = planes if isinstance(planes, (tuple, list)) else [planes]
    return frames.yuv_surface_geometry([t.shape for t in planes], [t.stride() for t in planes], color, [t.dtype for t in planes] if with_dtypes else None)


U8, I16, U16 = torch.uint8, torch.int16, torch.uint16


def test_geometry_of_every_new_form():
    H, W = 36, 52
    for color in ("p010", "p016"):
        for dt in (U16, I16):
            # planes: the nv12 numbers in BYTES, format word 4
            assert _geom((_z(dt, H, W), _z(dt, H // 2, W // 2, 2)), color) == (H, W, 0, 2 * W, 2, 0, 2, 2 * W, 4, 4), (color, dt)
            # a pitched surface: 64 samples = 128 bytes per row
            surface = _z(dt, H * 3 // 2, 64)[:, :W]
            assert _geom(surface, color) == (H, W, 0, 128, 2, H * 128, H * 128 + 2, 128, 4, 4)
        # odd sizes, a crop at an even origin, expanded chroma
        assert _geom((_z(I16, 37, 53), _z(I16, 19, 27, 2)), color) == (37, 53, 0, 106, 2, 0, 2, 108, 4, 4)
        big_y, big_uv = _z(U16, 64, 80), _z(U16, 32, 40, 2)
        assert _geom((big_y[6:42, 8:60], big_uv[3:21, 4:30]), color) == (H, W, 0, 160, 2, 0, 2, 160, 4, 4)
        assert _geom((_z(U16, H, W), _z(U16, 1, 1, 2).expand(18, 26, 2)), color) == (H, W, 0, 2 * W, 2, 0, 2, 0, 0, 4)
    assert _geom((_z(U8, H, W), _z(U8, H, 26), _z(U8, H, 26)), "i422") == (H, W, 0, W, 1, 0, 0, 26, 1, 2)
    assert _geom((_z(U8, 37, 53), _z(U8, 37, 27), _z(U8, 37, 27)), "i422") == (37, 53, 0, 53, 1, 0, 0, 27, 1, 2)
    assert _geom((_z(U8, H, W), _z(U8, H, W), _z(U8, H, W)), "i444") == (H, W, 0, W, 1, 0, 0, W, 1, 3)
    assert _geom((_z(U8, 1, 9), _z(U8, 1, 9), _z(U8, 1, 9)), "i444") == (1, 9, 0, 9, 1, 0, 0, 9, 1, 3)
    packed444 = _z(U8, H, W, 3)                                                          # planes as strided views of a packed buffer
    assert _geom((packed444[..., 0], packed444[..., 1], packed444[..., 2]), "i444") == (H, W, 0, 3 * W, 3, 0, 0, 3 * W, 3, 3)
    assert _geom(_z(U8, H, W), "i400") == _geom((_z(U8, H, W),), "i400") == (H, W, 0, W, 1, None, None, 0, 0, 8)
    assert _geom(_z(U8, 64, 80)[5:42, 7:60], "i400") == (37, 53, 0, 80, 1, None, None, 0, 0, 8)
    # packed 4:2:2: only addresses.  Y at element 0 / 1, U and V at the other element of the even and of the odd pixel
    assert _geom(_z(U8, H, W, 2), "yuyv") == (H, W, 0, 2 * W, 2, 1, 3, 2 * W, 4, 2)
    assert _geom(_z(U8, H, W, 2), "uyvy") == (H, W, 1, 2 * W, 2, 0, 2, 2 * W, 4, 2)
    assert _geom(_z(U8, 64, 80, 2)[6:42, 8:60], "yuyv") == (H, W, 0, 160, 2, 1, 3, 160, 4, 2)           # cropped at an even column
    assert _geom(_z(U8, 9, 2, 2), "uyvy") == (9, 2, 1, 4, 2, 0, 2, 4, 4, 2)
    # the old colours through the same function: their numbers, format word 0
    assert _geom((_z(U8, H, W), _z(U8, 18, 26, 2)), "nv21") == (H, W, 0, W, 1, 1, 0, W, 2, 0)
    assert _geom((_z(U8, H, W), _z(U8, 18, 26), _z(U8, 18, 26)), "i420") == (H, W, 0, W, 1, 0, 0, 26, 1, 0)
    assert _geom((_z(U16, H, W), _z(U16, 18, 26, 2)), "p010", with_dtypes=False)[:2] == (H, W)


def test_the_rule_on_bytes_finds_every_sample():
    """The fields, applied to the raw bytes of a buffer, find the samples the reference's index arithmetic finds."""
    for color, (h, w) in (("p010", (6, 10)), ("i422", (5, 7)), ("i444", (5, 7)), ("yuyv", (5, 8)), ("uyvy", (5, 8))):
        planes = ysr.random_planes(3, color, h, w)
        y, u, v = ysr.samples(planes, color)
        tensors = [torch.from_numpy(p) if p.dtype == np.uint8 else torch.from_numpy(p.view(np.int16)) for p in planes]
        H, W, y_off, y_row, y_pix, u_off, v_off, c_row, c_pix, fmt = _geom(tensors, color)
        raw = [p.reshape(-1).view(np.uint8) for p in planes]
        b = 2 if fmt & 4 else 1
        get = lambda buf, off: int(buf[off]) | (int(buf[off + 1]) << 8) if b == 2 else int(buf[off])
        sx, sy = 0 if fmt & 1 else 1, 0 if fmt & 2 else 1
        assert (sx, sy) == ysr.SHIFTS[color]
        for r in range(h):
            for c in range(w):
                assert get(raw[0], y_off + r * y_row + c * y_pix) == int(y[r, c])
                assert get(raw[1 if len(raw) > 1 else 0], u_off + (r >> sy) * c_row + (c >> sx) * c_pix) == int(u[r >> sy, c >> sx])
                assert get(raw[-1], v_off + (r >> sy) * c_row + (c >> sx) * c_pix) == int(v[r >> sy, c >> sx])


class _OnGpu(torch.Tensor):
    """A host tensor that says it lies on cuda:0: FrameIO reads its shape, strides and data pointer, never its bytes."""
    is_cuda, device = True, torch.device("cuda", 0)


def _on_gpu(dtype, *shape):
    return torch.zeros(shape, dtype=dtype).as_subclass(_OnGpu)


def test_descriptor_tables_carry_the_tensors_own_addresses_and_the_format_word():
    from centerpose_amd import frames
    io = frames.FrameIO(torch.device("cuda", 0))
    H, W = 36, 52
    y16, uv16 = _on_gpu(I16, 64, 80)[6:42, 8:60], _on_gpu(I16, 32, 40, 2)[3:21, 4:30]
    surface = _on_gpu(U16, 54, 64)[:, :W]
    p8 = [_on_gpu(U8, H, W) for _ in range(3)]
    c422 = [_on_gpu(U8, H, 26) for _ in range(2)]
    packed = _on_gpu(U8, 64, 80, 2)[6:42, 8:60]
    cases = [("p010", (y16, uv16), (y16.data_ptr(), H, W, 160, 2, uv16.data_ptr(), uv16.data_ptr() + 2, 160, 4, 4)),
             ("p016", surface, (surface.data_ptr(), H, W, 128, 2, surface.data_ptr() + H * 128, surface.data_ptr() + H * 128 + 2, 128, 4, 4)),
             ("i422", (p8[0], c422[0], c422[1]), (p8[0].data_ptr(), H, W, W, 1, c422[0].data_ptr(), c422[1].data_ptr(), 26, 1, 2)),
             ("i444", tuple(p8), (p8[0].data_ptr(), H, W, W, 1, p8[1].data_ptr(), p8[2].data_ptr(), W, 1, 3)),
             ("i400", p8[0], (p8[0].data_ptr(), H, W, W, 1, 0, 0, 0, 0, 8)),
             ("i400", (p8[1],), (p8[1].data_ptr(), H, W, W, 1, 0, 0, 0, 0, 8)),
             ("yuyv", packed, (packed.data_ptr(), H, W, 160, 2, packed.data_ptr() + 1, packed.data_ptr() + 3, 160, 4, 2)),
             ("uyvy", packed, (packed.data_ptr() + 1, H, W, 160, 2, packed.data_ptr(), packed.data_ptr() + 2, 160, 4, 2))]
    for color, frame, want in cases:
        f = io.yuv_frame(frame, color)
        assert isinstance(f, frames.YuvSurface) and tuple(f) == want and f.fmt == want[9], color
        images, descs = io.batch_input([frame, frame], "hwc", color, "bt2020-full")
        assert descs == [f, f]
        t = frames.identity_table(descs, True)
        assert t.dtype == frames.YUV_FRAME_DESC and t.itemsize == 136
        for d in t:
            got = tuple(int(d[k]) for k in ("y_base", "H", "W", "y_row", "y_pix", "u_base", "v_base", "c_row", "c_pix", "pad"))
            assert got == want, color
            assert (int(d["NH"]), int(d["NW"]), int(d["mid_off"]), int(d["slot"])) == (H, W, -1, 0) and not d["mi"].any()
    # the old colours: the nine-field tuple they always gave, format word 0, the same table bytes as a hand-written row
    y, uv = _on_gpu(U8, H, W), _on_gpu(U8, 18, 26, 2)
    for color, (uo, vo) in (("nv12", (0, 1)), ("nv21", (1, 0))):
        f = io.yuv_frame((y, uv), color)
        assert type(f) is frames.YuvFrame and len(f) == 9 and tuple(f) == (y.data_ptr(), H, W, W, 1, uv.data_ptr() + uo, uv.data_ptr() + vo, W, 2)
        t = frames.identity_table([f], True)
        assert int(t["pad"][0]) == 0
        hand = np.zeros(1, frames.YUV_FRAME_DESC)
        d = hand[0]
        d["y_base"], d["H"], d["W"], d["y_row"], d["y_pix"], d["u_base"], d["v_base"], d["c_row"], d["c_pix"] = tuple(f)
        d["NH"], d["NW"], d["mid_off"] = H, W, -1
        assert t.tobytes() == hand.tobytes()
    f = io.yuv_frame((y, uv[..., 0], uv[..., 1]), "i420")
    assert type(f) is frames.YuvFrame and int(frames.identity_table([f], True)["pad"][0]) == 0


def test_pre_table_keeps_the_format_word():
    _lib_built()
    from centerpose_amd import config, detector, frames
    det = object.__new__(detector.MultiPoseDetector)
    det.cfg = config.get_cfg("res_50")
    f = frames.YuvSurface(8192, 36, 52, 128, 2, 16384, 16386, 128, 4, 4)
    g = frames.YuvSurface(4096, 37, 53, 53, 1, 0, 0, 0, 0, 8)
    table, scratch, _, _, _ = det._pre_table([(36, 52), (37, 53)], None, [0, 1], 0.5, [f, g], True)
    assert table["pad"].tolist() == [4, 8] and table["y_base"].tolist() == [8192, 4096] and table["NH"].tolist() == [18, 18]
    assert table["u_base"].tolist() == [16384, 0] and (table["mid_off"] >= 0).all() and scratch > 0


# ---------------------------------------------------------------- 3. the re-id host twins on the new colours
def _host_table(frames_np, colors):
    """YUV_FRAME_DESC rows that address host NumPy planes in place, by the library's pure geometry function."""
    from centerpose_amd import frames
    rows = []
    for planes, color in zip(frames_np, colors):
        H, W, y_off, y_row, y_pix, u_off, v_off, c_row, c_pix, fmt = frames.yuv_surface_geometry(
            [p.shape for p in planes], [tuple(s // p.itemsize for s in p.strides) for p in planes], color, [p.dtype for p in planes])
        u_plane, v_plane = (planes[0], planes[0]) if len(planes) == 1 else (planes[1], planes[-1])
        u_base, v_base = (0, 0) if u_off is None else (u_plane.ctypes.data + u_off, v_plane.ctypes.data + v_off)
        rows.append(frames.YuvSurface(planes[0].ctypes.data + y_off, H, W, y_row, y_pix, u_base, v_base, c_row, c_pix, fmt))
    return frames.identity_table(rows, True)


def _pitched(p, pad):
    """The same samples as a view of a wider allocation whose padding holds other values."""
    big = np.full(p.shape[:1] + (p.shape[1] + pad,) + p.shape[2:], 0xA5, p.dtype)
    big[:, :p.shape[1]] = p
    return big[:, :p.shape[1]]


REID_FRAMES = [("p010", 37, 53, "bt2020-limited"), ("i422", 37, 53, "bt601-full"), ("i444", 37, 53, "bt709-full"), ("i400", 37, 53, "bt601-full"),
               ("yuyv", 37, 54, "bt601-full"), ("uyvy", 64, 64, "bt709"), ("p016", 64, 64, "bt2020-full")]


@pytest.mark.parametrize("color,H,W,matrix", REID_FRAMES, ids=[c[0] for c in REID_FRAMES])
def test_reid_host_twins_on_the_new_colours_equal_the_reference(color, H, W, matrix):
    L = _lib_built()
    R = reid_ref.row
    # two frames of one colour in one call: contiguous, and pitched rows with foreign padding
    a, b = ysr.random_planes(700, color, H, W), tuple(_pitched(p, 5) for p in ysr.random_planes(710, color, H, W))
    frames_np, colors = [a, b], [color, color]
    rows = np.zeros((2, 3, 56), np.float32)
    rows[0] = [R(10, 7, 15.9, 10.2), R(-6.5, -3, 20, 30, 0.31), R(3, 3, 9, 9, 0.3)]          # enlarging; off the top left; score == VIS
    rows[1] = [R(W - 13, H - 17, W + 20, H + 30), R(0, 0, W - 1, H - 1), R(20.5, 30.2, 21.9, 99)]      # off the bottom right; the whole frame
    pictures = [ysr.frame_to_bgr(p, color, matrix) for p in frames_np]
    cap, vis = 6, reid_ref.VIS
    want_x, want_slots, want_counts = reid_ref.crops(pictures, rows, vis, cap)
    assert (want_slots >= 0).sum() >= 4
    table = _host_table(frames_np, colors)
    assert (table["pad"] != 0).all()
    before = [[p.base.copy() if p.base is not None else p.copy() for p in f] for f in frames_np]
    rc, slots, counts = reid_util.host_select(L, [dict(color=color)] * 2, rows, vis, cap, table=table)
    assert rc == 0 and np.array_equal(slots, want_slots) and np.array_equal(counts, want_counts)
    out = np.full(cap * 3 * 128 * 64 + reid_util.GUARD, np.nan, np.float32)
    nm = reid_util.norm_struct()
    rc = L.cp_reid_crop_yuv_frames_host(table.ctypes.data_as(VP), 2, (ctypes.c_int * 6)(*ysr.COEF[matrix]), rows.ctypes.data_as(VP), 3,
                                        ctypes.c_float(vis), slots.ctypes.data_as(VP), cap, nm.ctypes.data_as(VP), out.ctypes.data_as(VP))
    assert rc == 0, L.cp_last_error()
    n = cap * 3 * 128 * 64
    assert np.isnan(out[n:]).all() and not np.isnan(out[:n]).any()
    assert reid_util.same_bits(out[:n].reshape(cap, 3, 128, 64), want_x)
    after = [[p.base if p.base is not None else p for p in f] for f in frames_np]
    assert all(np.array_equal(x, y) for fa, fb in zip(after, before) for x, y in zip(fa, fb))           # frames are only read


# ---------------------------------------------------------------- 4. refusals that need no device
def test_geometry_refusals():
    from centerpose_amd import frames
    from centerpose_amd._lib import CenterposeHipError
    H, W = 36, 52
    g = frames.yuv_surface_geometry
    cases = [
        # wrong dtype per colour
        ("uint16 or int16", lambda: _geom((_z(U8, H, W), _z(U8, 18, 26, 2)), "p010")),
        ("uint16 or int16", lambda: _geom(_z(torch.int32, 54, W), "p016")),
        ("uint16 or int16", lambda: g([(H, W), (18, 26, 2)], [(W, 1), (W, 2, 1)], "p010", [np.uint16, np.float32])),
        ("uint8", lambda: _geom((_z(I16, H, W), _z(I16, H, 26), _z(I16, H, 26)), "i422")),
        ("uint8", lambda: _geom((_z(U8, H, W), _z(U8, H, W), _z(U16, H, W)), "i444")),
        ("uint8", lambda: _geom(_z(I16, H, W), "i400")),
        ("uint8", lambda: _geom(_z(U16, H, W, 2), "yuyv")),
        ("uint8", lambda: _geom(_z(torch.float32, H, W, 2), "uyvy")),
        # mixed dtypes
        ("same dtype", lambda: _geom((_z(U16, H, W), _z(I16, 18, 26, 2)), "p010")),
        ("same dtype", lambda: _geom((_z(I16, H, W), _z(U16, 18, 26, 2)), "p016")),
        # odd W for packed forms, other shapes
        ("even W", lambda: _geom(_z(U8, H, 51, 2), "yuyv")),
        ("even W", lambda: _geom(_z(U8, 1, 9, 2), "uyvy")),
        (r"\[H,W,2\]", lambda: _geom(_z(U8, H, W), "yuyv")),
        (r"\[H,W,2\]", lambda: _geom(_z(U8, H, W, 3), "uyvy")),
        ("one tensor", lambda: _geom((_z(U8, H, W, 2), _z(U8, H, W, 2)), "yuyv")),
        # odd surface sizes
        ("even H and W", lambda: _geom(_z(U16, 55, W), "p010")),
        ("even H and W", lambda: _geom(_z(I16, 54, 51), "p010")),
        ("even H and W", lambda: _geom(_z(I16, 56, W), "p016")),
        ("uv plane", lambda: _geom((_z(U16, 37, 53), _z(U16, 18, 26, 2)), "p010")),                  # floor instead of ceil
        ("got 3 tensors", lambda: _geom((_z(U16, H, W), _z(U16, 18, 26), _z(U16, 18, 26)), "p010")),
        # planes of the wrong shape, unequal chroma strides
        ("u and v planes", lambda: _geom((_z(U8, H, W), _z(U8, 18, 26), _z(U8, 18, 26)), "i422")),   # 4:2:0 planes
        ("u and v planes", lambda: _geom((_z(U8, H, W), _z(U8, H, 26), _z(U8, H, 26)), "i444")),
        ("u and v planes", lambda: _geom((_z(U8, 37, 53), _z(U8, 37, 26), _z(U8, 37, 26)), "i422")),
        ("equal strides", lambda: _geom((_z(U8, H, W), _z(U8, H, 26), _z(U8, H, 32)[:, :26]), "i422")),
        ("equal strides", lambda: _geom((_z(U8, H, W), _z(U8, H, W), _z(U8, H, 2 * W)[:, ::2]), "i444")),
        (r"\(y, u, v\)", lambda: _geom((_z(U8, H, W), _z(U8, H, W, 2)), "i444")),
        ("one tensor", lambda: _geom((_z(U8, H, W), _z(U8, H, W)), "i400")),
        ("2-D", lambda: _geom(_z(U8, H, W, 1), "i400")),
        ("no pixels", lambda: _geom(_z(U8, 0, W), "i400")),
        ("negative strides", lambda: g([(H, W, 2)], [(2 * W, -2, 1)], "yuyv")),
        ("negative strides", lambda: g([(H, W), (18, 26, 2)], [(W, 1), (-W, 2, 1)], "p010")),
        # names
        ("unknown color", lambda: _geom(_z(U8, H, W), "gray")),
        ("unknown color", lambda: _geom(_z(U8, H, W), "nv16")),
        ("not planes", lambda: _geom(_z(U8, H, W, 3), "rgb")),
        ("format word", lambda: frames.yuv_frame_geometry([(H, W)], [(W, 1)], "i400")),              # the 8-tuple has no room for it
    ]
    for match, call in cases:
        with pytest.raises(CenterposeHipError, match=match):
            call()
    # the old colours keep their texts: an int16 plane under nv12 is still "uint8"
    with pytest.raises(CenterposeHipError, match="must be uint8"):
        _geom((_z(I16, H, W), _z(I16, 18, 26, 2)), "nv12")
    with pytest.raises(CenterposeHipError, match="must be uint8"):
        frames.yuv_frame_geometry([(54, W)], [(W, 1)], "nv21", [torch.int16])
    with pytest.raises(CenterposeHipError, match="planes"):
        frames.frame_geometry((H, W, 2), (2 * W, 2, 1), "hwc", "yuyv")


def _detector():
    from centerpose_amd import config, detector
    det = object.__new__(detector.MultiPoseDetector)
    det.cfg = config.get_cfg("dla_34")
    det.scales = det.cfg.TEST.TEST_SCALES
    det.num_classes = 1
    det.model = type("Model", (), {"process": None, "device": "cuda:0"})()
    return det


def test_entry_points_take_the_names_and_refuse_the_rest():
    from centerpose_amd import reid, frames
    from centerpose_amd._lib import CenterposeHipError
    det = _detector()
    y16, uv16 = _z(I16, 8, 8), _z(I16, 4, 4, 2)
    y, uv = _z(U8, 8, 8), _z(U8, 4, 4, 2)
    calls = lambda frame, **kw: (lambda: det.pre_process(frame, 1, **kw), lambda: det.pre_process_batch([frame], 1, **kw),
                                 lambda: det.run_batch([frame], **kw), lambda: det.run(frame, **kw))
    for match, frame, kw in [
        ("cpu", (y16, uv16), dict(color="p010")),                          # the names are known: the call gets as far as the tensors
        ("cpu", _z(U16, 12, 8), dict(color="p016", matrix="bt2020-limited")),
        ("cpu", (y, y, y), dict(color="i444", matrix="bt601-full")),
        ("cpu", y, dict(color="i400", matrix="bt709-full")),
        ("cpu", _z(U8, 8, 8, 2), dict(color="yuyv", matrix="bt2020-full")),
        ("cpu", (y, uv), dict(color="nv12", matrix="bt601-full")),         # a new matrix with an old colour
        ("unknown matrix", (y, uv), dict(color="nv12", matrix="bt2020")),
        ("unknown matrix", (y16, uv16), dict(color="p010", matrix="bt2020")),
        ("unknown matrix", (y, uv), dict(color="nv12", matrix="jpeg")),
        ("unknown matrix", (y, uv), dict(color="nv12", matrix="bt601-limited")),
        ("unknown color", (y, uv), dict(color="yuv")), ("unknown color", y, dict(color="gray")), ("unknown color", (y, uv), dict(color="yv12")),
        ("unknown color", (y, uv), dict(color="p012")), ("unknown color", (y, uv), dict(color="nv16")),
        ("layout", (y16, uv16), dict(color="p010", layout="chw")),
        ("matrix", np.zeros((8, 8, 3), np.uint8), dict(matrix="bt601-full")),        # a matrix with BGR
        ("device", (np.zeros((8, 8), np.uint16), np.zeros((4, 4, 2), np.uint16)), dict(color="p010")),      # host YUV arrays are not taken
        ("device", np.zeros((8, 8), np.uint8), dict(color="i400")),
    ]:
        for call in calls(frame, **kw):
            with pytest.raises(CenterposeHipError, match=match):
                call()
    assert det.run_batch([], color="p010", matrix="bt2020-limited") == []
    with pytest.raises(CenterposeHipError, match="list of frames"):
        det.run_batch(_z(U8, 2, 8, 8), color="i400")
    ext = object.__new__(reid.ReidExtractor)
    ext.device = torch.device("cuda", 0)
    ext._io = frames.FrameIO(ext.device)
    with pytest.raises(CenterposeHipError, match="cpu"):
        ext.embed([(y16, uv16)], torch.zeros((1, 1, 56)), color="p010", matrix="bt2020-full")
    with pytest.raises(CenterposeHipError, match="unknown matrix"):
        ext.embed([(y16, uv16)], torch.zeros((1, 1, 56)), color="p010", matrix="bt2020")


def test_drawing_refuses_the_new_colours_and_matrices_before_it_looks_at_a_frame():
    from centerpose_amd._lib import CenterposeHipError
    det = _detector()
    rows = torch.zeros((1, 1, 56))
    y, uv = _on_gpu(U8, 8, 8), _on_gpu(U8, 4, 4, 2)
    new_frames = {"p010": (_on_gpu(I16, 8, 8), _on_gpu(I16, 4, 4, 2)), "p016": _on_gpu(U16, 12, 8), "i422": (y, _on_gpu(U8, 8, 4), _on_gpu(U8, 8, 4)),
                  "i444": (y, y, y), "i400": y, "yuyv": _on_gpu(U8, 8, 8, 2), "uyvy": _on_gpu(U8, 8, 8, 2)}
    assert set(new_frames) == set(ysr.COLORS)
    tracks = [np.array([[1, 1, 5, 5, 3]])]
    for color, frame in new_frames.items():
        for call in (lambda: det.draw_results([frame], rows, color=color), lambda: det.draw_tracks([frame], tracks, color=color),
                     lambda: det.run_batch([frame], color=color, draw=True), lambda: det.run_batch([frame], color=color, draw=True, return_device=True)):
            with pytest.raises(CenterposeHipError, match="color='%s' frames cannot be drawn on" % color):
                call()
    for matrix in ISSUE_ROWS:
        for call in (lambda: det.draw_results([(y, uv)], rows, color="nv12", matrix=matrix), lambda: det.draw_tracks([(y, uv)], tracks, color="nv12", matrix=matrix),
                     lambda: det.run_batch([(y, uv)], color="nv12", matrix=matrix, draw=True)):
            with pytest.raises(CenterposeHipError, match="matrix='%s' is not taken for drawing" % matrix):
                call()
    # unknown names are still unknown first, and draw="tracks" without a tracker is still its own error
    with pytest.raises(CenterposeHipError, match="unknown matrix"):
        det.draw_results([(y, uv)], rows, color="nv12", matrix="bt2020")
    with pytest.raises(CenterposeHipError, match="unknown color"):
        det.draw_tracks([y], tracks, color="gray")


# ---------------------------------------------------------------- 5. the C ABI through host tables
def _desc(**kw):
    from centerpose_amd import frames
    t = np.zeros(1, frames.YUV_FRAME_DESC)
    d = t[0]
    d["y_base"], d["y_row"], d["y_pix"], d["u_base"], d["v_base"], d["c_row"], d["c_pix"], d["mid_off"] = 4096, 16, 2, 8192, 8194, 16, 4, -1
    d["H"], d["W"], d["NH"], d["NW"], d["mi"], d["slot"], d["pad"] = 4, 8, 4, 8, (1, 0, 0, 0, 1, 0), 0, 4
    for k, v in kw.items():
        d[k] = v
    return t


BAD_FORMATS = [(dict(pad=16), b"outside 0..15"), (dict(pad=-1), b"outside 0..15"), (dict(pad=255), b"outside 0..15"), (dict(pad=1 << 30), b"outside 0..15"),
               (dict(pad=9), b"grey"), (dict(pad=10), b"grey"), (dict(pad=11), b"grey"), (dict(pad=15), b"grey"),
               (dict(y_base=4097), b"even luma"), (dict(y_row=17), b"even luma"), (dict(y_pix=1), b"even luma"),
               (dict(u_base=8193), b"even chroma"), (dict(v_base=8195), b"even chroma"), (dict(c_row=15), b"even chroma"), (dict(c_pix=3), b"even chroma"),
               (dict(pad=12, y_base=4097), b"even luma"),                                      # 16-bit grey: the luma still counts
               (dict(u_base=0), b"null base"), (dict(pad=6, v_base=0), b"null base"), (dict(pad=8, y_base=0), b"null base"),
               (dict(c_row=-16), b"negative stride"), (dict(pad=7, c_row=1 << 62), b"2^62"),    # 4:4:4: chroma row 3 is addressed
               (dict(pad=2, H=2, NH=2, c_row=1 << 62), b"2^62")]                               # 4:2:2: a 2-row frame reaches chroma row 1


@pytest.mark.parametrize("fields,message", BAD_FORMATS)
def test_format_refusals_of_the_pre_process_come_before_any_launch(fields, message):
    """No device here: a call that got past its argument checks would fail to launch, with another message."""
    L = _lib_built()
    table = _desc(**fields)
    mean, std = (ctypes.c_float * 3)(0.4, 0.4, 0.4), (ctypes.c_float * 3)(0.3, 0.3, 0.3)
    rc = L.cp_preprocess_yuv_frames_u8_f32(VP(4096), table.ctypes.data_as(VP), 1, (ctypes.c_int * 6)(*ysr.COEF["bt601"]), None, ctypes.c_size_t(0),
                                           VP(4096), 1, 8, 8, mean, std, 0, None)
    assert rc == 1 and message in L.cp_last_error(), L.cp_last_error()
    assert b"pad" in L.cp_last_error()


@pytest.mark.parametrize("fields,message", BAD_FORMATS)
def test_format_refusals_of_the_reid_host_twins_touch_nothing(fields, message):
    L = _lib_built()
    table = _desc(**fields)
    rows = reid_ref.row(1, 1, 7, 3).reshape(1, 1, 56)
    out = np.full(3 * 128 * 64, np.nan, np.float32)
    slots, nm = np.zeros(1, np.int32), reid_util.norm_struct()
    rc = L.cp_reid_crop_yuv_frames_host(table.ctypes.data_as(VP), 1, (ctypes.c_int * 6)(*ysr.COEF["bt601"]), rows.ctypes.data_as(VP), 1, ctypes.c_float(0.3),
                                        slots.ctypes.data_as(VP), 1, nm.ctypes.data_as(VP), out.ctypes.data_as(VP))
    assert rc == 1 and message in L.cp_last_error() and np.isnan(out).all(), L.cp_last_error()
    # the selection reads H and W only: it refuses the words no crop would take, and nothing else of these
    rc, got_slots, counts = reid_util.host_select(L, [dict(color="p010")], rows, 0.3, 1, table=table)
    word_is_bad = message in (b"outside 0..15", b"grey")
    assert rc == (1 if word_is_bad else 0), L.cp_last_error()
    if word_is_bad:
        assert message in L.cp_last_error() and (got_slots == -7).all() and (counts == -7).all()


def test_a_grey_frame_may_have_null_chroma_bases_and_16_bit_444_is_valid():
    """Through the re-id host twin, which runs on the CPU: format words 8 and 12 with null chroma, and word 7 that Python names no
    colour for, against the reference on the same samples."""
    L = _lib_built()
    from centerpose_amd import frames
    H, W = 9, 7
    rs = np.random.RandomState(5)
    y8 = rs.randint(0, 256, (H, W)).astype(np.uint8)
    y16, u16, v16 = (rs.randint(0, 1 << 16, (H, W)).astype(np.uint16) for _ in range(3))
    grey16 = ysr.to_bgr16(y16, np.full((H, W), 32768), np.full((H, W), 32768), ysr.COEF["bt601-full"])
    cases = [(frames.YuvSurface(y8.ctypes.data, H, W, W, 1, 0, 0, 0, 0, 8), ysr.frame_to_bgr((y8,), "i400", "bt601-full")),
             (frames.YuvSurface(y16.ctypes.data, H, W, 2 * W, 2, 0, 0, 0, 0, 12), grey16),
             (frames.YuvSurface(y16.ctypes.data, H, W, 2 * W, 2, u16.ctypes.data, v16.ctypes.data, 2 * W, 2, 7), ysr.to_bgr16(y16, u16, v16, ysr.COEF["bt601-full"]))]
    rows = reid_ref.row(0, 0, W, H).reshape(1, 1, 56)                    # clamps to the whole frame but its last row and column
    for f, picture in cases:
        table = frames.identity_table([f], True)
        want, slots, _ = reid_ref.crops([picture], rows, 0.3, 1)
        out = np.full(3 * 128 * 64, np.nan, np.float32)
        nm = reid_util.norm_struct()
        rc = L.cp_reid_crop_yuv_frames_host(table.ctypes.data_as(VP), 1, (ctypes.c_int * 6)(*ysr.COEF["bt601-full"]), rows.ctypes.data_as(VP), 1,
                                            ctypes.c_float(0.3), slots.ctypes.data_as(VP), 1, nm.ctypes.data_as(VP), out.ctypes.data_as(VP))
        assert rc == 0, L.cp_last_error()
        assert slots.tolist() == [0] and reid_util.same_bits(out.reshape(1, 3, 128, 64), want), f.fmt


def test_the_host_painters_refuse_a_non_zero_format_word():
    L = _lib_built()
    from centerpose_amd import draw
    form = draw_ref.yuv_forms(3, 20, 24)[0]
    rows = np.zeros((1, 1, 56), np.float32)
    rows[0, 0, :5] = (2, 2, 15, 15, 1.0)
    st = draw_util.style_struct(2, 2, 2, [(10, 20, 30)] * 36)
    items, counts = draw.track_items([np.array([[2, 2, 15, 15, 3]])], draw.TrackStyle(), "bt601")
    idp = np.zeros(1, draw.DRAW_ID_PALETTE)
    idp["count"], ids = 1, np.zeros(1, np.int32)
    for word in (1, 2, 3, 4, 8, 15, 16, -1):
        buf = form["buf"].copy()
        table = draw_util.table_of([form], [buf.ctypes.data])
        table["pad"] = word
        calls = [lambda: L.cp_draw_rows_yuv_frames_host(table.ctypes.data_as(VP), 1, rows.ctypes.data_as(VP), 1, ctypes.c_float(0.3), st.ctypes.data_as(VP)),
                 lambda: L.cp_draw_rows_ids_yuv_frames_host(table.ctypes.data_as(VP), 1, rows.ctypes.data_as(VP), 1, ctypes.c_float(0.3), st.ctypes.data_as(VP),
                                                            ids.ctypes.data_as(VP), idp.ctypes.data_as(VP)),
                 lambda: L.cp_draw_tracks_yuv_frames_host(table.ctypes.data_as(VP), 1, items.ctypes.data_as(VP), counts.ctypes.data_as(VP), items.shape[1], 2, 1)]
        for call in calls:
            assert call() == 1 and b"pad = %d" % word in L.cp_last_error(), (word, L.cp_last_error())
            assert np.array_equal(buf, form["buf"])
    buf = form["buf"].copy()
    table = draw_util.table_of([form], [buf.ctypes.data])
    assert int(table["pad"][0]) == 0
    assert L.cp_draw_rows_yuv_frames_host(table.ctypes.data_as(VP), 1, rows.ctypes.data_as(VP), 1, ctypes.c_float(0.3), st.ctypes.data_as(VP)) == 0
    assert not np.array_equal(buf, form["buf"])                          # the same call with word 0 paints
