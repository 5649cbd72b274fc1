"""CPU: draw_results without a device -- the C-ABI symbols and the style struct, the HOST painters (cp_draw_rows_frames_host /
cp_draw_rows_yuv_frames_host, the statements of csrc/draw_arith.h the kernels compile) against hand-written pixel sets and, byte for
byte over whole buffers, against the independent NumPy painter of tests/draw_ref.py; the palette conversion, the writability rule and
every refusal that needs no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import draw_ref
import draw_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHITE = [(255, 255, 255)] * 36


def _detector():
    from centerpose_amd import config, detector
    det = object.__new__(detector.MultiPoseDetector)
    det.cfg = config.get_cfg("dla_34")
    det.scales = det.cfg.TEST.TEST_SCALES
    det.model = type("Model", (), {"process": None, "device": "cpu"})()
    return det


# ---------------------------------------------------------------- 1. symbols and the struct
def test_symbols_abi_and_style_struct():
    L = draw_util.lib_built()
    from centerpose_amd import detector
    hdr = open(os.path.join(ROOT, "include", "centerpose_hip.h")).read()
    for sym in ("cp_sizeof_draw_style", "cp_draw_scratch_bytes", "cp_draw_rows_frames_u8", "cp_draw_rows_yuv_frames_u8",
                "cp_draw_rows_frames_host", "cp_draw_rows_yuv_frames_host"):
        assert re.search(r"\b%s\s*\(" % sym, hdr) and hasattr(L, sym), sym
    assert L.cp_abi_version() == 4
    assert L.cp_sizeof_draw_style() == detector.DRAW_STYLE.itemsize == 156
    body = re.search(r"typedef struct cp_draw_style \{(.*?)\} cp_draw_style;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"[\[\]\d\s]", "", f) for f in re.findall(r"(?:unsigned char|int) ([^;]+);", body)]
    assert fields == list(detector.DRAW_STYLE.names)
    assert detector.DRAW_STYLE.fields["palette"][0].shape == (36, 4) and detector.DRAW_STYLE.fields["palette"][1] == 12
    assert L.cp_draw_scratch_bytes(0, 5) == 0 and L.cp_draw_scratch_bytes(3, 0) == 0
    assert L.cp_draw_scratch_bytes(2, 3) == 6 * L.cp_draw_scratch_bytes(1, 1) > 0
    assert tuple(detector.DRAW_LIMBS) == tuple(draw_ref.LIMBS)


def test_default_style_and_palette():
    from centerpose_amd import detector
    st = detector.DrawStyle()
    assert (st.box_thickness, st.limb_radius, st.joint_radius) == (2, 1, 2)
    pal = st.palette()
    assert len(pal) == 36 and set(pal) == {detector.DRAW_LEFT, detector.DRAW_RIGHT, detector.DRAW_MID}
    assert pal[0] == detector.DRAW_MID and pal[19] == detector.DRAW_MID                     # the box, the nose
    assert pal[19 + 5] == detector.DRAW_LEFT and pal[19 + 6] == detector.DRAW_RIGHT         # the shoulders
    assert pal[1 + 6] == detector.DRAW_MID and pal[1 + 13] == detector.DRAW_MID             # shoulder to shoulder, hip to hip
    assert pal[1 + 0] == detector.DRAW_LEFT and pal[1 + 1] == detector.DRAW_RIGHT           # nose to the left / right eye
    rec = st.struct()
    assert rec["palette"][0, :, :3].tolist() == [list(c) for c in pal] and not rec["palette"][0, :, 3].any()
    for bad in (dict(box_thickness=65), dict(box_thickness=-1), dict(limb_radius=0), dict(limb_radius=-2), dict(joint_radius=-2),
                dict(joint_radius=65), dict(box_color=(0, 0, 256)), dict(limb_colors=[(0, 0, 0)] * 17)):
        with pytest.raises(detector._lib.CenterposeHipError):
            detector.DrawStyle(**bad)


# ---------------------------------------------------------------- 2. hand anchors
def _painted(L, H, W, row, thickness=0, limb_radius=-1, joint_radius=-1):
    """The set of (x, y) the host painter paints for one row on an H x W packed frame of zeros."""
    form = dict(name="anchor", layout="hwc", color="bgr", buf=np.zeros(H * W * 3, np.uint8), views=[(0, (H, W, 3), (3 * W, 3, 1))])
    buf, = draw_util.host_paint(L, [form], row, 0.0, thickness, limb_radius, joint_radius, WHITE)
    img = buf.reshape(H, W, 3)
    assert ((img == 0) | (img == 255)).all() and (img[..., 0] == img[..., 1]).all() and (img[..., 1] == img[..., 2]).all()
    return {(int(x), int(y)) for y, x in zip(*np.nonzero(img[..., 0]))}


def _row(box=(np.nan,) * 4, joints=()):
    row = np.zeros(56, np.float32)
    row[0:4], row[4] = box, 1.0
    for j, (x, y) in joints:
        row[5 + 2 * j], row[6 + 2 * j], row[39 + j] = x, y, 1.0
    return row


DISCS = {1: ["xxx", "xxx", "xxx"],
         2: [".xxx.", "xxxxx", "xxxxx", "xxxxx", ".xxx."],
         3: ["..xxx..", ".xxxxx.", "xxxxxxx", "xxxxxxx", "xxxxxxx", ".xxxxx.", "..xxx.."]}


def _disc_pixels(R, cx, cy):
    if R == 0:
        return {(cx, cy)}
    return {(cx - R + i, cy - R + j) for j, line in enumerate(DISCS[R]) for i, ch in enumerate(line) if ch == "x"}


@pytest.mark.parametrize("R,count", [(0, 1), (1, 9), (2, 21), (3, 37)])
def test_joint_radii_by_hand(R, count):
    L = draw_util.lib_built()
    want = _disc_pixels(R, 8, 6)
    assert len(want) == count
    assert _painted(L, 13, 17, _row(joints=[(4, (8.9, 6.2))]), joint_radius=R) == want       # truncation toward zero: (8, 6)
    # the same disc from a degenerate limb (P == Q) of that radius
    if R >= 1:
        assert _painted(L, 13, 17, _row(joints=[(0, (8, 6)), (1, (8.5, 6.5))]), limb_radius=R) == want
    # clipped by the frame's corner
    assert _painted(L, 13, 17, _row(joints=[(16, (0, 0))]), joint_radius=R) == {p for p in _disc_pixels(R, 0, 0) if p[0] >= 0 and p[1] >= 0}


def test_limbs_by_hand():
    L = draw_util.lib_built()
    # horizontal, radius 1: k = 2, the body is |dy| <= 1 between the ends, the caps add nothing beyond x = 2 - 1 and 9 + 1
    got = _painted(L, 9, 14, _row(joints=[(5, (2, 4)), (7, (9, 4))]), limb_radius=1)
    assert got == {(x, y) for x in range(1, 11) for y in (3, 4, 5)}
    # the diagonal (2,2) -> (5,5), radius 1: cross^2 = 9 (x - y)^2 <= 2 * 18 means |x - y| <= 2 inside the ends
    got = _painted(L, 9, 9, _row(joints=[(11, (2, 2)), (13, (5, 5))]), limb_radius=1)
    want = set()
    for x in range(9):
        for y in range(9):
            t = (x - 2) * 3 + (y - 2) * 3
            if t <= 0:
                ok = (x - 2) ** 2 + (y - 2) ** 2 <= 2
            elif t >= 18:
                ok = (x - 5) ** 2 + (y - 5) ** 2 <= 2
            else:
                ok = abs(x - y) <= 2
            if ok:
                want.add((x, y))
    assert got == want and (1, 1) in want and (6, 6) in want and (0, 0) not in want and (3, 5) in want and (2, 5) not in want
    # a limb needs both joints: one score at 0 and nothing is drawn
    row = _row(joints=[(5, (2, 4)), (7, (9, 4))])
    row[39 + 7] = 0.0
    assert _painted(L, 9, 14, row, limb_radius=1) == set()


def test_boxes_by_hand():
    L = draw_util.lib_built()
    ring = {(x, y) for x in range(2, 10) for y in range(3, 8) if x in (2, 9) or y in (3, 7)}
    assert _painted(L, 10, 12, _row(box=(2, 3, 9, 7)), thickness=1) == ring
    assert _painted(L, 10, 12, _row(box=(9.7, 7.2, 2.1, 3.9)), thickness=1) == ring            # reversed corners, truncated
    full = {(x, y) for x in range(2, 10) for y in range(3, 8)}
    assert _painted(L, 10, 12, _row(box=(2, 3, 9, 7)), thickness=2) == full - {(x, 5) for x in range(4, 8)}
    assert _painted(L, 10, 12, _row(box=(2, 3, 9, 7)), thickness=3) == full                    # thickness >= half the box fills it
    assert _painted(L, 10, 12, _row(box=(2, 3, 9, 7)), thickness=64) == full
    assert _painted(L, 10, 12, _row(box=(4, 4, 4, 4)), thickness=1) == {(4, 4)}                # a 1 x 1 box
    assert _painted(L, 10, 12, _row(box=(4, 4, 4, 4)), thickness=0) == set()
    assert _painted(L, 10, 12, _row(box=(-1e9, -50, 1e9, 2)), thickness=1) == {(x, 2) for x in range(12)}      # clamped far outside
    assert _painted(L, 10, 12, _row(box=(2, 3, np.inf, 7)), thickness=1) == set()


def test_liveness_and_order_by_hand():
    L = draw_util.lib_built()
    form = dict(name="order", layout="hwc", color="bgr", buf=np.zeros(6 * 6 * 3, np.uint8), views=[(0, (6, 6, 3), (18, 3, 1))])
    rows = np.stack([_row(box=(0, 0, 5, 5), joints=[(0, (1, 1))]), _row(box=(1, 1, 1, 1)), _row(box=(2, 2, 2, 2)), _row(box=(3, 3, 3, 3))])
    rows[2, 4], rows[3, 4] = 0.5, np.nan                        # exactly at the threshold, and NaN: neither is drawn
    pal = [(10 + i, 0, 0) for i in range(36)]
    buf, = draw_util.host_paint(L, [form], rows, 0.5, 1, -1, 0, pal)
    img = buf.reshape(6, 6, 3)[..., 0]
    assert img[1, 1] == 10                                     # row 1's box over row 0's joint: the later row wins
    assert img[0, 0] == 10 and img[3, 3] == 0 and img[2, 2] == 0
    rows[1, 4] = 0.0
    buf, = draw_util.host_paint(L, [form], rows, 0.5, 1, -1, 0, pal)
    assert buf.reshape(6, 6, 3)[1, 1, 0] == 10 + 19            # the joint over its own row's box


# ---------------------------------------------------------------- 3. seeded fuzz: host painter == NumPy reference, whole buffers
def _fuzz_cases():
    cases = []
    for s, (H, W) in enumerate(draw_ref.SIZES):
        for f in range(6):
            cases.append(("bgr", s, f))
        for f in range(6 if H % 2 == 0 and W % 2 == 0 else 4):
            cases.append(("yuv", s, f))
    return cases


@pytest.mark.parametrize("kind,s,f", _fuzz_cases())
def test_host_painter_equals_numpy_reference(kind, s, f):
    L = draw_util.lib_built()
    H, W = draw_ref.SIZES[s]
    form = (draw_ref.bgr_forms if kind == "bgr" else draw_ref.yuv_forms)(100 * s + 10, H, W)[f]
    assert draw_ref.frame_size(form) == (H, W)
    painted = 0
    for trial in range(3):
        seed = 1000 * s + 10 * f + trial + (500 if kind == "yuv" else 0)
        rows = draw_ref.fuzz_rows(seed, 12, H, W)
        T, RL, RJ, pal = draw_ref.fuzz_style(seed)
        matrix = "bt709" if trial == 2 else "bt601"
        want = draw_ref.reference(form, rows, draw_ref.VIS, T, RL, RJ, pal, matrix)
        got, = draw_util.host_paint(L, [form], rows, draw_ref.VIS, T, RL, RJ, pal, matrix)
        assert np.array_equal(got, want), (form["name"], seed, np.nonzero(got != want)[0][:8])
        # the guard bytes on either side of the views, explicitly
        G = draw_ref.GUARD
        assert np.array_equal(got[:G], form["buf"][:G]) and np.array_equal(got[-G:], form["buf"][-G:])
        painted += int((want != form["buf"]).sum())
    assert painted > 0, "nothing was painted: the case shows nothing"


@pytest.mark.parametrize("kind", ["bgr", "yuv"])
def test_dense_300_rows_on_16x16(kind):
    L = draw_util.lib_built()
    form = (draw_ref.bgr_forms if kind == "bgr" else draw_ref.yuv_forms)(77, 16, 16)[2]
    rows = draw_ref.fuzz_rows(4242, 300, 16, 16, dense=True)
    assert (rows[:, 4] > draw_ref.VIS).all()
    T, RL, RJ, pal = draw_ref.fuzz_style(3)
    want = draw_ref.reference(form, rows, draw_ref.VIS, T, RL, RJ, pal)
    got, = draw_util.host_paint(L, [form], rows, draw_ref.VIS, T, RL, RJ, pal)
    assert np.array_equal(got, want)
    win = draw_ref.winners(rows, 16, 16, draw_ref.VIS, T, RL, RJ)
    assert (win >= 0).mean() > 0.9 and len(np.unique(win // 36)) > 8      # nearly every pixel covered, by many different rows


def test_alpha_and_padding_untouched():
    L = draw_util.lib_built()
    H, W = 7, 5
    form = draw_ref.bgr_forms(5, H, W)[2]                      # bgra with padded rows
    row = np.zeros(56, np.float32)
    row[0:5] = (-5, -5, 50, 50, 1.0)
    got, = draw_util.host_paint(L, [form], row, 0.3, 64, 1, 2, WHITE)       # the box fills the frame
    view, = draw_ref.numpy_views(got, form)
    orig, = draw_ref.numpy_views(form["buf"], form)
    assert (view[..., :3] == 255).all() and np.array_equal(view[..., 3], orig[..., 3])
    changed = np.nonzero(got != form["buf"])[0]
    assert len(changed) <= H * W * 3 and set(changed) <= {form["views"][0][0] + y * (4 * W + 13) + 4 * x + k for y in range(H) for x in range(W)
                                                          for k in range(3)}


# ---------------------------------------------------------------- 4. palette conversion
def test_palette_conversion_against_the_stated_formulas():
    from centerpose_amd import detector
    colors = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (1, 2, 3), (200, 100, 50)] + detector.DrawStyle().palette()
    for b, g, r in colors:
        y, u, v = detector.palette_to_yuv([(b, g, r)], "bt601")[0]
        assert y == ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
        assert u == ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128
        assert v == ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128
        y, u, v = detector.palette_to_yuv([(b, g, r)], "bt709")[0]
        assert y == ((47 * r + 157 * g + 16 * b + 128) >> 8) + 16
        assert u == ((-26 * r - 87 * g + 112 * b + 128) >> 8) + 128
        assert v == ((112 * r - 102 * g - 10 * b + 128) >> 8) + 128
    assert detector.palette_to_yuv([(0, 0, 0), (255, 255, 255), (255, 0, 0)]) == [(16, 128, 128), (235, 128, 128), (41, 240, 110)]
    assert detector.palette_to_yuv(colors, "bt709") == draw_ref.bgr_to_yuv(colors, "bt709")
    rec = detector.DrawStyle().struct("bt601")
    assert rec["palette"][0, :, :3].tolist() == [list(c) for c in detector.palette_to_yuv(detector.DrawStyle().palette())]
    with pytest.raises(detector._lib.CenterposeHipError, match="unknown matrix"):
        detector.palette_to_yuv(colors, "bt2020")


# ---------------------------------------------------------------- 5. which views may be written
def test_frame_writable():
    from centerpose_amd import detector
    w = detector.frame_writable
    t = torch.zeros((9, 5, 3), dtype=torch.uint8)
    big = torch.zeros((20, 30, 4), dtype=torch.uint8)
    ok = [t, t.permute(2, 0, 1), big[3:12, 4:9], big[3:12, 4:9, :3], big[::2, ::3], torch.zeros((4, 3, 9, 5), dtype=torch.uint8),
          torch.zeros((4, 9, 5, 3), dtype=torch.uint8).permute(0, 3, 1, 2), t[:1], t[:, :1], torch.zeros((12, 8), dtype=torch.uint8)[:, :6]]
    for v in ok:
        assert w(v.shape, v.stride()), (tuple(v.shape), v.stride())
    bad = [torch.zeros((9, 1, 3), dtype=torch.uint8).expand(9, 5, 3), torch.zeros((1, 1, 1), dtype=torch.uint8).expand(9, 5, 3),
           torch.zeros((1, 9, 5, 3), dtype=torch.uint8).expand(4, 9, 5, 3),
           torch.as_strided(torch.zeros(200, dtype=torch.uint8), (9, 5, 3), (10, 3, 1)),        # rows of 15 bytes every 10
           torch.as_strided(torch.zeros(200, dtype=torch.uint8), (9, 5, 3), (15, 2, 1))]        # pixels of 3 bytes every 2
    for v in bad:
        assert not w(v.shape, v.stride()), (tuple(v.shape), v.stride())
    assert not w((9, 5, 3), (15, -3, 1)) and not w((0, 5, 3), (15, 3, 1))
    assert detector.byte_range(1000, (9, 5, 3), (15, 3, 1)) == (1000, 1000 + 135)


def test_refusals_without_a_device():
    from centerpose_amd._lib import CenterposeHipError
    det = _detector()
    rows = torch.zeros((1, 2, 56))
    with pytest.raises(CenterposeHipError, match="host arrays"):
        det.draw_results([np.zeros((8, 8, 3), np.uint8)], rows)
    with pytest.raises(CenterposeHipError, match="host arrays"):
        det.run_batch([np.zeros((8, 8, 3), np.uint8)], draw=True)
    with pytest.raises(CenterposeHipError, match="cpu"):
        det.draw_results([torch.zeros((8, 8, 3), dtype=torch.uint8)], rows)
    with pytest.raises(CenterposeHipError, match="unknown color"):
        det.draw_results([np.zeros((8, 8, 3), np.uint8)], rows, color="gray")
    assert det.run_batch([], draw=True) == []


# ---------------------------------------------------------------- 6. argument checks through ctypes: nothing is dereferenced
def _bgr_desc(**kw):
    from centerpose_amd import detector
    t = np.zeros(1, detector.FRAME_DESC)
    d = t[0]
    d["base"], d["row_stride"], d["pix_stride"], d["ch_off"], d["mid_off"], d["H"], d["W"] = 4096, 24, 3, (0, 1, 2), -1, 4, 8
    for k, v in kw.items():
        d[k] = v
    return t


def _yuv_desc(**kw):
    from centerpose_amd import detector
    t = np.zeros(1, detector.YUV_FRAME_DESC)
    d = t[0]
    d["y_base"], d["y_row"], d["y_pix"], d["u_base"], d["v_base"], d["c_row"], d["c_pix"] = 4096, 8, 1, 8192, 8193, 8, 2
    d["mid_off"], d["H"], d["W"] = -1, 4, 8
    for k, v in kw.items():
        d[k] = v
    return t


def _call(L, table, yuv=False, host=False, N=1, M=2, vis=0.3, style=(2, 1, 2), rows=4096, scratch=4096, scratch_bytes=1 << 20, dev_table=4096,
          null_style=False):
    st = draw_util.style_struct(style[0], style[1], style[2], WHITE)
    sp = None if null_style else st.ctypes.data_as(ctypes.c_void_p)
    tp = table.ctypes.data_as(ctypes.c_void_p) if table is not None else None
    if host:
        fn = L.cp_draw_rows_yuv_frames_host if yuv else L.cp_draw_rows_frames_host
        return fn(tp, N, ctypes.c_void_p(rows), M, ctypes.c_float(vis), sp)
    fn = L.cp_draw_rows_yuv_frames_u8 if yuv else L.cp_draw_rows_frames_u8
    return fn(ctypes.c_void_p(dev_table), tp, N, ctypes.c_void_p(rows), M, ctypes.c_float(vis), sp, ctypes.c_void_p(scratch),
              ctypes.c_size_t(scratch_bytes), None)


BAD_BGR = [(dict(base=0), b"null base"), (dict(H=0), b"bad size"), (dict(W=16385), b"bad size"), (dict(row_stride=-24), b"negative"),
           (dict(pix_stride=-3), b"negative"), (dict(ch_off=(0, -1, 2)), b"negative"), (dict(pix_stride=0), b"stride of 0"),
           (dict(row_stride=0), b"stride of 0"), (dict(ch_off=(0, 1, 1)), b"one offset"), (dict(row_stride=1 << 61), b"2^62")]
BAD_YUV = [(dict(y_base=0), b"null base"), (dict(u_base=0), b"null base"), (dict(v_base=0), b"null base"), (dict(H=16385), b"bad size"),
           (dict(W=0), b"bad size"), (dict(y_row=-8), b"negative"), (dict(c_pix=-2), b"negative"), (dict(y_pix=0), b"stride of 0"),
           (dict(c_row=0), b"stride of 0"), (dict(c_pix=0), b"stride of 0"), (dict(v_base=8192), b"one address"), (dict(y_row=1 << 61), b"2^62")]


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("yuv,fields,message", [(False, f, m) for f, m in BAD_BGR] + [(True, f, m) for f, m in BAD_YUV])
def test_descriptor_checks_come_before_any_launch(host, yuv, fields, message):
    """No device here: a device call that got past its checks would fail to launch, with another message; a host call that got
    past them would dereference address 4096."""
    L = draw_util.lib_built()
    table = (_yuv_desc if yuv else _bgr_desc)(**fields)
    assert _call(L, table, yuv=yuv, host=host) == 1
    assert message in L.cp_last_error(), L.cp_last_error()


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("yuv", [False, True])
def test_checks_of_the_call_itself(host, yuv):
    L = draw_util.lib_built()
    table = (_yuv_desc if yuv else _bgr_desc)()
    call = lambda **kw: _call(L, table, yuv=yuv, host=host, **kw)
    err = L.cp_last_error
    assert call(N=65536) == 1 and b"65535" in err()
    assert call(N=-1) == 1 and b"65535" in err()
    assert call(M=-1) == 1 and b"negative row count" in err()
    for vis in (np.nan, np.inf, -np.inf):
        assert call(vis=vis) == 1 and b"vis_thresh" in err()
    for style, msg in (((65, 1, 2), b"box_thickness"), ((-1, 1, 2), b"box_thickness"), ((2, 0, 2), b"limb_radius"), ((2, -2, 2), b"limb_radius"),
                       ((2, 65, 2), b"limb_radius"), ((2, 1, -2), b"joint_radius"), ((2, 1, 65), b"joint_radius")):
        assert call(style=style) == 1 and msg in err(), style
    assert call(null_style=True) == 1 and b"null style" in err()
    assert call(rows=None) == 1 and b"null pointer" in err()
    assert _call(L, None, yuv=yuv, host=host) == 1 and b"null pointer" in err()
    if not host:
        assert call(scratch=None) == 1 and b"null pointer" in err()
        assert call(dev_table=None) == 1 and b"null pointer" in err()
        assert call(scratch=4104) == 1 and b"aligned" in err()
        assert call(scratch_bytes=L.cp_draw_scratch_bytes(1, 2) - 1) == 1 and b"cp_draw_scratch_bytes" in err()
    # nothing to paint: a success that looks at nothing else (the addresses are still not real)
    assert call(N=0) == 0 and call(M=0) == 0
    assert _call(L, None, yuv=yuv, host=host, N=0, rows=None, scratch=None, scratch_bytes=0) == 0
    assert call(N=0, style=(2, 0, 2)) == 1                     # ... but a bad style is still a bad style
