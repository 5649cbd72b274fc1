"""CPU: the overlay painters without a device -- the score rule (cp_draw_score_label) against Python's '%.1f', the HOST painters
(cp_draw_overlay_frames_host / cp_draw_overlay_yuv_frames_host, the statements of csrc/draw_overlay_arith.h the kernels compile) byte
for byte over whole buffers against the independent NumPy painter of tests/draw_overlay_ref.py, their identity with the plain host
painters when nothing leaves the defaults, every refusal that needs no device, and DrawStyle's new keywords."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import draw_overlay_ref as oref
import draw_overlay_util as outil
import draw_ref
import draw_tracks_ref as tref
import draw_tracks_util
import draw_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p


# ---------------------------------------------------------------- 1. symbols and the struct
def test_symbols_and_overlay_struct():
    L = outil.lib()
    from centerpose_amd import draw
    hdr = open(os.path.join(ROOT, "include", "centerpose_hip.h")).read()
    for sym in ("cp_sizeof_draw_overlay", "cp_draw_overlay_scratch_bytes", "cp_draw_score_label", "cp_draw_overlay_frames_u8",
                "cp_draw_overlay_yuv_frames_u8", "cp_draw_overlay_frames_host", "cp_draw_overlay_yuv_frames_host"):
        assert re.search(r"\b%s\s*\(" % sym, hdr) and hasattr(L, sym), sym
    assert L.cp_sizeof_draw_overlay() == draw.DRAW_OVERLAY.itemsize == 36
    body = re.search(r"typedef struct cp_draw_overlay \{(.*?)\} cp_draw_overlay;", hdr, re.S).group(1)
    fields = [re.sub(r"[\[\]\d\s]", "", f) for f in re.findall(r"(?:unsigned char|int) ([^;]+);", body)]
    assert fields == list(draw.DRAW_OVERLAY.names)
    # the existing records keep their sizes
    assert L.cp_sizeof_draw_style() == 156 and L.cp_sizeof_draw_track_item() == 44
    assert L.cp_draw_overlay_scratch_bytes(0, 5) == 0 and L.cp_draw_overlay_scratch_bytes(3, 0) == 0
    assert L.cp_draw_overlay_scratch_bytes(2, 3) == 6 * L.cp_draw_overlay_scratch_bytes(1, 1) > L.cp_draw_scratch_bytes(2, 3)


# ---------------------------------------------------------------- 2. the score rule
def _label(L, values):
    """cp_draw_score_label per float32 value -> the texts ("nan" for -1)."""
    fn = L.cp_draw_score_label
    fn.argtypes, fn.restype = [ctypes.c_float, ctypes.POINTER(ctypes.c_ubyte)], ctypes.c_int
    out, g = [], (ctypes.c_ubyte * 8)()
    for v in values:
        for i in range(8):
            g[i] = 0xEE
        n = fn(ctypes.c_float(v), g)
        assert n == -1 or (3 <= n <= 6 and all(g[i] == 0xEE for i in range(n, 8))), (v, n)
        out.append("nan" if n < 0 else "".join(tref.CHARSET[g[i]] for i in range(n)))
    return out


def _mismatches(L, values):
    values = np.asarray(values, np.float32)
    got = _label(L, values.tolist())
    want = ["%.1f" % float(v) for v in values]
    return [(float(v), g, w) for v, g, w in zip(values, got, want) if g != w]


def test_score_label_equals_percent_1f():
    L = outil.lib()
    r = np.random.RandomState(20241)
    assert _mismatches(L, r.uniform(0, 1.2, 200000)) == []
    assert _mismatches(L, r.uniform(-999.9, 999.9, 200000)) == []
    # every tenths boundary (2k + 1) / 20 with its +-3 ulp neighbours, both signs
    edge = []
    for k in range(41):
        v = np.float32((2 * k + 1) / 20.0)
        for _ in range(3):
            v = np.nextafter(v, np.float32(-np.inf), dtype=np.float32)
        for _ in range(7):
            edge += [v, -v]
            v = np.nextafter(v, np.float32(np.inf), dtype=np.float32)
    assert len(edge) == 41 * 14 and _mismatches(L, edge) == []
    # exact ties go to the even tenth
    assert _label(L, [0.0, -0.0, 1e-30, -1e-30, 1e-45, 0.25, 0.75, 2.25, -2.75, 100.25, 999.94, -999.94, 9.96875]) == \
        ["0.0", "-0.0", "0.0", "-0.0", "0.0", "0.2", "0.8", "2.2", "-2.8", "100.2", "999.9", "-999.9", "10.0"]
    # random bit patterns: '%.1f' wherever it stays below the cap, 999.9 above, -1 for NaN
    bits = r.randint(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32)
    vals = bits.view(np.float32)
    got = _label(L, vals.tolist())
    bad = []
    for v, b, g in zip(vals, bits, got):
        if np.isnan(v):
            want = "nan"
        elif abs(float(v)) < 999.95:
            want = "%.1f" % float(v)
        else:
            want = ("-" if b >> 31 else "") + "999.9"
        if g != want:
            bad.append((hex(int(b)), g, want))
    assert bad == [] and sum(np.isnan(vals)) > 0 and sum(np.abs(vals) < 999.95) > 5000
    assert _label(L, [np.inf, -np.inf, 1e9, -3e38, 999.95, 1000.0, 8388608.0]) == ["999.9", "-999.9", "999.9", "-999.9", "999.9", "999.9", "999.9"]
    assert L.cp_draw_score_label(ctypes.c_float(np.nan), None) == -1


# ---------------------------------------------------------------- 3. host painter == NumPy reference, whole buffers
def _cases():
    cases = []
    for s, (H, W) in enumerate(draw_ref.SIZES):
        for f in range(6):
            cases.append(("bgr", s, f))
        for f in range(6 if H % 2 == 0 and W % 2 == 0 else 4):
            cases.append(("yuv", s, f))
    return cases


@pytest.mark.parametrize("kind,s,f", _cases())
def test_host_painter_equals_numpy_reference(kind, s, f):
    L = outil.lib()
    H, W = draw_ref.SIZES[s]
    form = (draw_ref.bgr_forms if kind == "bgr" else draw_ref.yuv_forms)(100 * s + 10, H, W)[f]
    painted = 0
    for k, (scale, opacity, prefix) in enumerate(oref.STYLES):
        rows, vis, (T, RL, RJ, pal), ids, idpal, tc = outil.case_inputs(kind, s, f, k)
        prims = list(oref.primitives(rows, H, W, vis, T, RL, RJ, scale, prefix))      # the masks once, the colours four times
        for with_ids in (False, True):
            for matrix in (("bt601", "bt709") if kind == "yuv" else ("bt601",)):
                kw = dict(opacity=opacity, label_scale=scale, prefix=prefix, text_color=tc, matrix=matrix)
                if with_ids:
                    kw.update(ids=ids, id_palette=idpal)
                want = oref.reference(form, rows, vis, T, RL, RJ, pal, prims=prims, **kw)
                got, = outil.host_paint(L, [form], rows, vis, T, RL, RJ, pal, **kw)
                assert np.array_equal(got, want), (form["name"], k, with_ids, matrix, np.nonzero(got != want)[0][:8])
                G = draw_ref.GUARD
                assert np.array_equal(got[:G], form["buf"][:G]) and np.array_equal(got[-G:], form["buf"][-G:])
                painted += int((want != form["buf"]).sum())
    assert painted > 0, "nothing was painted: the case shows nothing"


@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("kind", ["bgr", "yuv"])
def test_the_cases_are_not_vacuous(kind, s):
    """On the REFERENCE's output, per size from (7, 5) up: what the byte equality above is worth."""
    H, W = draw_ref.SIZES[s]
    forms = (draw_ref.bgr_forms if kind == "bgr" else draw_ref.yuv_forms)(100 * s + 10, H, W)
    stats = {}
    for f, form in enumerate(forms):
        for k, (scale, opacity, prefix) in enumerate(oref.STYLES):
            rows, vis, (T, RL, RJ, pal), ids, idpal, tc = outil.case_inputs(kind, s, f, k)
            oref.reference(form, rows, vis, T, RL, RJ, pal, opacity=opacity, label_scale=scale, prefix=prefix, text_color=tc, stats=stats)
    assert stats["max_blends"] >= 2, stats                      # some pixel is blended at least twice
    assert stats["label_pixels"] > 0, stats                     # some label pixel is painted
    assert stats["clipped_top"] > 0 and stats["clipped_right"] > 0, stats
    if kind == "yuv":
        assert stats["partial_chroma"] > 0, stats               # some chroma sample has only part of its block covered


def test_label_by_hand():
    """One row on a black frame: the bar sits on the box, in the box's colour; the text is PERSON0.9, cell by cell from the font file."""
    L = outil.lib()
    H, W = 24, 70
    form = dict(name="hand", layout="hwc", color="bgr", buf=np.zeros(H * W * 3, np.uint8), views=[(0, (H, W, 3), (3 * W, 3, 1))])
    row = np.zeros((1, 56), np.float32)
    row[0, 0:5] = (3.7, 12.2, 60, 20, 0.87)
    pal = [(10 + i, 20, 30) for i in range(36)]
    got, = outil.host_paint(L, [form], row, 0.3, 1, -1, -1, pal, label_scale=1, prefix="PERSON", text_color=(200, 201, 202))
    img = got.reshape(H, W, 3)
    text = "PERSON0.9"
    x1 = 3 + 6 * len(text) - 1 + 3
    bar = np.zeros((H, W), bool)
    bar[12 - 7 - 5:12, 3:x1 + 1] = True                         # rows 0..11, columns 3..59
    glyphs = np.zeros((H, W), bool)
    for i, ch in enumerate(text):
        glyphs[2:9, 5 + 6 * i:5 + 6 * i + 5] = tref.FONT[ch]
    assert (img[glyphs] == (200, 201, 202)).all() and (img[bar & ~glyphs] == (10, 20, 30)).all()
    box = np.zeros((H, W), bool)
    box[12:21, 3:61] = True
    box[13:20, 4:60] = False
    assert (img[box] == (10, 20, 30)).all() and not img[~(bar | box)].any()
    # thickness 0: no box, the label stays; a dead box coordinate: no label either
    got0, = outil.host_paint(L, [form], row, 0.3, 0, -1, -1, pal, label_scale=1, prefix="PERSON", text_color=(200, 201, 202))
    assert np.array_equal(got0.reshape(H, W, 3)[bar], img[bar]) and not got0.reshape(H, W, 3)[~bar].any()
    row[0, 2] = np.inf
    gotn, = outil.host_paint(L, [form], row, 0.3, 1, -1, -1, pal, label_scale=1, prefix="PERSON", text_color=(200, 201, 202))
    assert not gotn.any()


def test_blend_by_hand():
    """Two translucent joints over one pixel: blended twice, in paint order, with the stated rounding."""
    L = outil.lib()
    form = dict(name="hand", layout="hwc", color="bgr", buf=np.full(3 * 3 * 3, 100, np.uint8), views=[(0, (3, 3, 3), (9, 3, 1))])
    row = np.zeros((1, 56), np.float32)
    row[0, 0:5] = (np.nan, 0, 0, 0, 1.0)
    row[0, 5:9], row[0, 39:41] = (1, 1, 1, 1), 1.0              # joints 0 and 1 at (1, 1)
    pal = [(0, 0, 0)] * 19 + [(255, 7, 100), (0, 255, 100)] + [(0, 0, 0)] * 15
    got, = outil.host_paint(L, [form], row, 0.3, 2, -1, 0, pal, opacity=(256, 256, 51))
    once = [(100 * 205 + c * 51 + 128) >> 8 for c in (255, 7, 100)]
    twice = [(p * 205 + c * 51 + 128) >> 8 for p, c in zip(once, (0, 255, 100))]
    img = got.reshape(3, 3, 3)
    assert img[1, 1].tolist() == twice and twice[2] == 100 and (np.delete(img.reshape(9, 3), 4, 0) == 100).all()


# ---------------------------------------------------------------- 4. nothing leaves the defaults: the plain host painters
@pytest.mark.parametrize("kind", ["bgr", "yuv"])
def test_identity_with_the_plain_host_painters(kind):
    L = outil.lib()
    for s, (H, W) in enumerate(draw_ref.SIZES):
        for f, form in enumerate((draw_ref.bgr_forms if kind == "bgr" else draw_ref.yuv_forms)(100 * s + 10, H, W)):
            seed = 1000 * s + 10 * f
            rows = draw_ref.fuzz_rows(seed, 12, H, W)
            T, RL, RJ, pal = draw_ref.fuzz_style(seed)
            ids, idpal = tref.fuzz_ids(seed + 1, 12), tref.fuzz_id_palette(seed + 2, 5)
            plain, = draw_util.host_paint(L, [form], rows, draw_ref.VIS, T, RL, RJ, pal)
            got, = outil.host_paint(L, [form], rows, draw_ref.VIS, T, RL, RJ, pal, label_scale=0, prefix="PERSON", text_color=(1, 2, 3))
            assert np.array_equal(got, plain), (form["name"], seed)
            plain, = draw_tracks_util.host_paint_rows_ids(L, [form], rows, ids, idpal, draw_ref.VIS, T, RL, RJ, pal)
            got, = outil.host_paint(L, [form], rows, draw_ref.VIS, T, RL, RJ, pal, ids=ids, id_palette=idpal)
            assert np.array_equal(got, plain), (form["name"], seed, "ids")


# ---------------------------------------------------------------- 5. argument checks through ctypes: nothing is dereferenced
def _call(L, yuv=False, host=False, N=1, M=2, style=(2, 1, 2), ov=None, null_overlay=False, row_ids=None, idp=None, table_fields=None,
          scratch=4096, scratch_bytes=1 << 20, vis=0.3):
    from centerpose_amd import detector
    if yuv:
        table = np.zeros(1, detector.YUV_FRAME_DESC)
        d = table[0]
        d["y_base"], d["y_row"], d["y_pix"], d["u_base"], d["v_base"], d["c_row"], d["c_pix"] = 4096, 8, 1, 8192, 8193, 8, 2
    else:
        table = np.zeros(1, detector.FRAME_DESC)
        d = table[0]
        d["base"], d["row_stride"], d["pix_stride"], d["ch_off"] = 4096, 24, 3, (0, 1, 2)
    d["mid_off"], d["H"], d["W"] = -1, 4, 8
    for key, val in (table_fields or {}).items():
        d[key] = val
    st = draw_util.style_struct(style[0], style[1], style[2], [(255, 255, 255)] * 36)
    ov = outil.overlay_struct(**(ov or {}))
    op = None if null_overlay else ov.ctypes.data_as(VP)
    tp, sp, vf = table.ctypes.data_as(VP), st.ctypes.data_as(VP), ctypes.c_float(vis)
    ids_p = VP(row_ids) if row_ids else None
    idp_p = idp.ctypes.data_as(VP) if idp is not None else None
    if host:
        fn = L.cp_draw_overlay_yuv_frames_host if yuv else L.cp_draw_overlay_frames_host
        return fn(tp, N, VP(4096), M, vf, sp, ids_p, idp_p, op)
    fn = L.cp_draw_overlay_yuv_frames_u8 if yuv else L.cp_draw_overlay_frames_u8
    return fn(VP(4096), tp, N, VP(4096), M, vf, sp, VP(scratch) if scratch else None, ctypes.c_size_t(scratch_bytes), ids_p, idp_p, op, None)


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("yuv", [False, True])
def test_refusals_come_before_any_launch(host, yuv):
    """No device here: a device call that got past its checks would fail to launch, with another message; a host call that got past
    them would dereference address 4096."""
    L = outil.lib()
    err = L.cp_last_error
    call = lambda **kw: _call(L, yuv=yuv, host=host, **kw)
    for op in ((0, 256, 256), (256, 257, 256), (256, 256, -1), (256, 0, 256)):
        assert call(ov=dict(opacity=op)) == 1 and b"opacity" in err(), op
    for scale in (-1, 9):
        assert call(ov=dict(label_scale=scale)) == 1 and b"label_scale" in err()
    assert call(ov=dict(nprefix=10)) == 1 and b"prefix" in err()
    assert call(ov=dict(nprefix=-1)) == 1 and b"prefix" in err()
    assert call(ov=dict(prefix=[1, 2, 42], label_scale=1)) == 1 and b"glyph" in err()
    assert call(ov=dict(prefix=[255])) == 1 and b"glyph" in err()
    assert call(null_overlay=True) == 1 and b"null overlay" in err()
    idp = draw_tracks_util.id_palette_struct([(1, 2, 3)])
    assert call(row_ids=4096) == 1 and b"together" in err()
    assert call(idp=idp) == 1 and b"together" in err()
    idp["count"] = 65
    assert call(row_ids=4096, idp=idp) == 1 and b"id colours" in err()
    # everything cp_draw_rows_ids_* checks
    assert call(N=65536) == 1 and b"65535" in err()
    assert call(M=-1) == 1 and b"negative row count" in err()
    assert call(vis=np.nan) == 1 and b"vis_thresh" in err()
    for style, msg in (((65, 1, 2), b"box_thickness"), ((2, 0, 2), b"limb_radius"), ((2, 1, 65), b"joint_radius")):
        assert call(style=style) == 1 and msg in err(), style
    assert call(table_fields=dict(H=0)) == 1 and b"bad size" in err()
    assert call(table_fields=dict(W=16385)) == 1 and b"bad size" in err()
    assert call(table_fields=dict(y_base=0) if yuv else dict(base=0)) == 1 and b"null base" in err()
    if not host:
        assert call(scratch=None) == 1 and b"null pointer" in err()
        assert call(scratch=4104) == 1 and b"aligned" in err()
        assert call(scratch_bytes=L.cp_draw_overlay_scratch_bytes(1, 2) - 1) == 1 and b"cp_draw_overlay_scratch_bytes" in err()
    # nothing to paint: a success that looks at nothing behind the call's own arguments ...
    assert call(N=0) == 0 and call(M=0) == 0
    assert call(N=0, ov=dict(opacity=(0, 256, 256))) == 1       # ... but a bad overlay is still a bad overlay


# ---------------------------------------------------------------- 6. DrawStyle
def test_draw_style_keywords():
    from centerpose_amd import detector, draw
    from centerpose_amd._lib import CenterposeHipError
    st = detector.DrawStyle()
    assert not st.needs_overlay()
    assert (st.labels, st.label_prefix, st.label_scale, st.label_text_color) == (False, "person", 1, (0, 0, 0))
    assert (st.box_opacity, st.limb_opacity, st.joint_opacity) == (256, 256, 256)
    assert not detector.DrawStyle(label_prefix="id", label_scale=3, label_text_color=(9, 9, 9)).needs_overlay()     # labels stay off
    for kw in (dict(labels=True), dict(box_opacity=255), dict(limb_opacity=128), dict(joint_opacity=1)):
        assert detector.DrawStyle(**kw).needs_overlay(), kw
    rec = detector.DrawStyle(labels=True, limb_opacity=128, label_scale=2, label_text_color=(1, 2, 3)).overlay_struct()
    assert rec.dtype == draw.DRAW_OVERLAY and rec["opacity"][0].tolist() == [256, 128, 256] and int(rec["label_scale"][0]) == 2
    assert int(rec["nprefix"][0]) == 6 and "".join(tref.CHARSET[g] for g in rec["prefix"][0, :6]) == "PERSON"      # lower case folded
    assert rec["text_color"][0].tolist() == [1, 2, 3, 0]
    assert int(detector.DrawStyle(label_scale=2).overlay_struct()["label_scale"][0]) == 0                          # labels=False: scale 0
    rec = detector.DrawStyle(labels=True, label_prefix="", label_text_color=(255, 0, 0)).overlay_struct("bt601")
    assert int(rec["nprefix"][0]) == 0 and rec["text_color"][0, :3].tolist() == list(detector.palette_to_yuv([(255, 0, 0)], "bt601")[0])
    for bad in (dict(label_scale=0), dict(label_scale=9), dict(box_opacity=0), dict(limb_opacity=257), dict(joint_opacity=-1),
                dict(label_prefix="0123456789"), dict(label_prefix="person!"), dict(label_text_color=(0, 0, 256)), dict(label_text_color=(0, 0))):
        with pytest.raises(CenterposeHipError):
            detector.DrawStyle(**bad)
    # the plain record is what it was
    assert detector.DrawStyle(labels=True, limb_opacity=3).struct().tobytes() == detector.DrawStyle().struct().tobytes()


def test_run_batch_draw_style_refusals_without_a_device():
    from centerpose_amd import config, detector
    from centerpose_amd._lib import CenterposeHipError
    det = object.__new__(detector.MultiPoseDetector)
    det.cfg = config.get_cfg("dla_34")
    det.scales = det.cfg.TEST.TEST_SCALES
    det.model = type("Model", (), {"process": None, "device": "cpu"})()
    with pytest.raises(CenterposeHipError, match="DrawStyle"):
        det.run_batch([], draw=True, draw_style=dict(labels=True))
    with pytest.raises(ValueError, match="draw_style"):
        det.run_batch([], draw_style=detector.DrawStyle(labels=True))
    with pytest.raises(CenterposeHipError, match="host arrays"):
        det.run_batch([np.zeros((8, 8, 3), np.uint8)], draw=True, draw_style=detector.DrawStyle(labels=True))
    with pytest.raises(CenterposeHipError, match="host arrays"):
        det.draw_results([np.zeros((8, 8, 3), np.uint8)], torch.zeros((1, 2, 56)), style=detector.DrawStyle(limb_opacity=128))
    assert det.run_batch([], draw=True, draw_style=detector.DrawStyle(labels=True)) == []
