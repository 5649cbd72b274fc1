"""CPU: the heat-map overlay without a device -- the symbols and the style record, the forward colour form (cp_bgr_to_yuv_host) on every
colour, the HOST painters (cp_draw_heat_frames_host / cp_draw_heat_yuv_frames_host, the statements of csrc/draw_heat_arith.h the
kernels compile) byte for byte over whole buffers against the independent NumPy painter of tests/draw_heat_ref.py, three properties of
the rule, and every refusal that needs no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import draw_heat_ref as href
import draw_heat_util as hutil
import draw_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, LL = ctypes.c_void_p, ctypes.c_longlong


# ---------------------------------------------------------------- 1. symbols and the struct
def test_symbols_and_style_struct():
    L = hutil.lib()
    from centerpose_amd import detector, draw
    hdr = open(os.path.join(ROOT, "include", "centerpose_hip.h")).read()
    for sym in ("cp_sizeof_draw_heat_style", "cp_draw_heat_scratch_bytes", "cp_draw_heat_frames_u8", "cp_draw_heat_yuv_frames_u8",
                "cp_draw_heat_frames_host", "cp_draw_heat_yuv_frames_host", "cp_bgr_to_yuv_host"):
        assert re.search(r"\b%s\s*\(" % sym, hdr) and hasattr(L, sym), sym
    assert L.cp_sizeof_draw_heat_style() == draw.DRAW_HEAT_STYLE.itemsize == 140
    body = re.search(r"typedef struct cp_draw_heat_style \{(.*?)\} cp_draw_heat_style;", hdr, re.S).group(1)
    fields = [re.sub(r"[\[\]\d\s]", "", f) for f in re.findall(r"(?:unsigned char|int) ([^;]+);", body)]
    assert fields == ["channels", "opacity", "invert", "palette"] == list(draw.DRAW_HEAT_STYLE.names)
    # the existing records keep their sizes
    assert L.cp_sizeof_draw_style() == 156 and L.cp_sizeof_draw_track_item() == 44 and L.cp_sizeof_draw_overlay() == 36
    sb = L.cp_draw_heat_scratch_bytes
    assert sb(0, 5, 7) == 0 and sb(3, 0, 7) == 0 and sb(3, 5, 0) == 0
    assert sb(1, 5, 7) == 5 * 7 * 4 and sb(6, 5, 7) == 6 * sb(1, 5, 7) and sb(2, 8, 12) == 2 * sb(1, 8, 12)
    assert detector.HeatmapStyle is draw.HeatmapStyle and callable(detector.BaseDetector.draw_heatmaps)


# ---------------------------------------------------------------- 2. the forward form
def _forward(L, bgr, matrix):
    bgr = np.ascontiguousarray(bgr, np.uint8).reshape(-1, 3)
    out = np.full_like(bgr, 0xEE)
    assert L.cp_bgr_to_yuv_host(VP(bgr.ctypes.data), LL(len(bgr)), hutil.MATRIX_IDS[matrix], VP(out.ctypes.data)) == 0, L.cp_last_error()
    return out


@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_forward_form_on_every_colour(matrix):
    L = hutil.lib()
    g, r = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    kr, kg, kb = (np.array(row, np.int64) for row in zip(*href.FORWARD[matrix]))          # the weights of R, of G, of B for (Y, U, V)
    for b in range(256):
        bgr = np.stack([np.full_like(g, b), g, r], axis=-1).reshape(-1, 3)
        want = ((bgr[:, 2:3] * kr + bgr[:, 1:2] * kg + bgr[:, 0:1] * kb + 128) >> 8) + np.array([16, 128, 128])
        assert want.min() >= 0 and want.max() <= 255
        got = _forward(L, bgr, matrix)
        assert np.array_equal(got, want.astype(np.uint8)), b


@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_forward_form_equals_palette_to_yuv(matrix):
    L = hutil.lib()
    from centerpose_amd import draw
    corners = [(b, g, r) for b in (0, 255) for g in (0, 255) for r in (0, 255)]
    colors = corners + [tuple(int(v) for v in c) for c in np.random.RandomState(5).randint(0, 256, (4000, 3))]
    assert _forward(L, colors, matrix).tolist() == [list(c) for c in draw.palette_to_yuv(colors, matrix)]
    assert L.cp_bgr_to_yuv_host(None, LL(0), 0, None) == 0
    assert L.cp_bgr_to_yuv_host(None, LL(1), 0, None) == 1 and L.cp_bgr_to_yuv_host(VP(4096), LL(1), 2, VP(4096)) == 1


# ---------------------------------------------------------------- 3. host painters == the NumPy painter, whole buffers
@pytest.mark.parametrize("kind", ["bgr", "yuv"])
def test_host_painter_equals_numpy_painter(kind):
    L = hutil.lib()
    cases = hutil.cases(kind)
    seen = {"forms": set(), "odd": 0, "views": set(), "outside": 0, "painted": 0}
    for name, form, maps, T, pal, opacity, invert, matrix in cases:
        host, = hutil.host_paint(L, [form], maps, [T], pal, opacity, invert, matrix)
        want = href.reference(form, maps[0], T, pal, opacity, invert, matrix)
        assert np.array_equal(host, want), (name, np.nonzero(host != want)[0][:8])
        G = draw_ref.GUARD
        assert np.array_equal(host[:G], form["buf"][:G]) and np.array_equal(host[-G:], form["buf"][-G:]), name
        seen["painted"] += int((host != form["buf"]).sum())
        seen["forms"].add(form["name"])
        seen["views"].add(maps.strides)
        seen["odd"] += draw_ref.frame_size(form)[0] % 2
        seen["outside"] += T is href.OUTSIDE
    assert len(seen["forms"]) >= (7 if kind == "bgr" else 6) and seen["odd"] and seen["outside"] and seen["painted"] > 100000 and len(seen["views"]) >= 6
    assert {(c[5], c[6]) for c in cases} >= {(1, True), (179, False), (256, False), (256, True)}


@pytest.mark.parametrize("kind", ["bgr", "yuv"])
def test_two_frames_of_different_sizes_in_one_call(kind):
    L = hutil.lib()
    sizes = [(37, 53), (1, 1)] if kind == "bgr" else [(37, 53), (16, 16)]
    pick = [0, 0] if kind == "bgr" else [1, 1]                  # packed BGR; NV21 planes with a pitch
    forms = [hutil.forms_of(kind, 400 + 10 * n, H, W)[p] for n, ((H, W), p) in enumerate(zip(sizes, pick))]
    maps = href.fuzz_maps(77, 4, 17, 8, 12)[0::2]               # a [0::2] batch view: entries 0 and 2
    pal = href.fuzz_palette(3, 17)
    Ts = [href.fit_matrix(H, W, 8, 12) for H, W in sizes]
    host = hutil.host_paint(L, forms, maps, Ts, pal, 179, False, "bt709")
    for n in range(2):
        want = href.reference(forms[n], maps[n], Ts[n], pal, 179, False, "bt709")
        assert np.array_equal(host[n], want), n
    swapped = href.reference(forms[0], maps[1], Ts[0], pal, 179, False, "bt709")
    assert not np.array_equal(host[0], swapped)                 # each frame got its own map


# ---------------------------------------------------------------- 4. properties of the rule
def _packed(seed, H, W):
    return draw_ref.bgr_forms(seed, H, W)[0]


def test_opacity_256_writes_the_sampled_colour_map():
    L = hutil.lib()
    H, W, h, w = 37, 53, 8, 12
    form, maps, pal, T = _packed(1, H, W), href.fuzz_maps(2, 1, 17, h, w), href.fuzz_palette(3, 17), href.fit_matrix(H, W, h, w)
    host, = hutil.host_paint(L, [form], maps, [T], pal, 256, False)
    fore = href.fore(href.colormap(maps[0], pal, False), np.array(T), H, W)
    view, = draw_ref.numpy_views(host, form)
    assert np.array_equal(view, fore.astype(np.uint8))
    other, = hutil.host_paint(L, [dict(form, buf=255 - form["buf"])], maps, [T], pal, 256, False)
    assert np.array_equal(draw_ref.numpy_views(other, form)[0], view)          # whatever the frame held


def test_silent_map_blends_towards_black():
    L = hutil.lib()
    H, W = 16, 16
    form = _packed(4, H, W)
    for a in (1, 179, 256):
        host, = hutil.host_paint(L, [form], np.zeros((1, 17, 5, 7), np.float32), [href.fit_matrix(H, W, 5, 7)], href.fuzz_palette(5, 17), a, False)
        p = draw_ref.numpy_views(form["buf"].copy(), form)[0].astype(np.int64)
        assert np.array_equal(draw_ref.numpy_views(host, form)[0], (p * (256 - a) + 0 * a + 128) >> 8), a


def test_identity_matrix_on_an_equally_sized_map_gives_each_cell_its_own_colour():
    L = hutil.lib()
    H, W = 8, 12
    form, maps, pal = _packed(6, H, W), href.fuzz_maps(7, 1, 17, H, W), href.fuzz_palette(8, 17)
    host, = hutil.host_paint(L, [form], maps, [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]], pal, 256, True)
    assert np.array_equal(draw_ref.numpy_views(host, form)[0], href.colormap(maps[0], pal, True).astype(np.uint8))


# ---------------------------------------------------------------- 5. refusals that need no device
def _call(L, yuv=False, host=True, N=1, C=2, h=4, w=6, strides=(48, 24, 6, 1), style=(2, 179, 0), null_style=False, matrix=0, mi=None,
          table_fields=None, scratch=8192, scratch_bytes=1 << 20, maps=4096):
    """One call with addresses nothing may be read from or written to: 4096 for the frame and the maps."""
    from centerpose_amd import detector
    if yuv:
        table = np.zeros(max(N, 1), detector.YUV_FRAME_DESC)
        d = table[0]
        d["y_base"], d["y_row"], d["y_pix"], d["u_base"], d["v_base"], d["c_row"], d["c_pix"] = 4096, 8, 1, 8192, 8193, 8, 2
    else:
        table = np.zeros(max(N, 1), detector.FRAME_DESC)
        d = table[0]
        d["base"], d["row_stride"], d["pix_stride"], d["ch_off"] = 4096, 24, 3, (0, 1, 2)
    d["mid_off"], d["H"], d["W"] = -1, 4, 8
    d["mi"] = (1, 0, 0, 0, 1, 0) if mi is None else mi
    for key, val in (table_fields or {}).items():
        d[key] = val
    st = hutil.style_struct(style[0], style[1], style[2], [(255, 255, 255)] * 32)
    sp = None if null_style else st.ctypes.data_as(VP)
    head = (table.ctypes.data_as(VP), N, VP(maps) if maps else None, *(LL(s) for s in strides), C, h, w, sp)
    tail = (matrix,) if yuv else ()
    if host:
        return (L.cp_draw_heat_yuv_frames_host if yuv else L.cp_draw_heat_frames_host)(*head, *tail)
    fn = L.cp_draw_heat_yuv_frames_u8 if yuv else L.cp_draw_heat_frames_u8
    return fn(VP(4096), *head, *tail, VP(scratch) if scratch else None, ctypes.c_size_t(scratch_bytes), None)


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("yuv", [False, True])
def test_refusals_come_before_any_launch(host, yuv):
    """No device here: a device call that got past its checks would fail to launch, with another message; a host call that got past
    them would dereference address 4096."""
    L = hutil.lib()
    err = L.cp_last_error
    call = lambda **kw: _call(L, yuv=yuv, host=host, **kw)
    for C in (0, 33, -1):
        assert call(C=C, style=(32, 179, 0)) == 1 and b"map channels" in err(), C
    assert call(C=3) == 1 and b"colours" in err()               # a style of two colours
    assert call(style=(33, 179, 0)) == 1 and b"colours" in err()
    for a in (0, 257, -5):
        assert call(style=(2, a, 0)) == 1 and b"opacity" in err(), a
    assert call(style=(2, 179, 2)) == 1 and b"invert" in err()
    assert call(null_style=True) == 1 and b"null style" in err()
    for i in range(4):
        s = [48, 24, 6, 1]
        s[i] = -1
        assert call(strides=s) == 1 and b"negative map stride" in err(), i
    assert call(h=0) == 1 and b"bad map size" in err()
    assert call(w=16385) == 1 and b"bad map size" in err()
    assert call(N=65536) == 1 and b"65535" in err()
    assert call(N=-1) == 1
    assert call(maps=None) == 1 and b"null pointer" in err()
    for bad in (np.nan, np.inf, -np.inf):
        for i in range(6):
            mi = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
            mi[i] = bad
            assert call(mi=mi) == 1 and b"not finite" in err(), (bad, i)
    assert call(table_fields=dict(H=0)) == 1 and b"bad size" in err()
    assert call(table_fields=dict(W=16385)) == 1 and b"bad size" in err()
    assert call(table_fields=dict(y_base=0) if yuv else dict(base=0)) == 1 and b"null base" in err()
    if yuv:
        assert call(matrix=2) == 1 and b"matrix id" in err()
        assert call(table_fields=dict(pad=4)) == 1 and b"can be drawn on" in err()
    if not host:
        assert call(scratch=None) == 1 and b"null pointer" in err()
        assert call(scratch=8200) == 1 and b"aligned" in err()
        assert call(scratch_bytes=L.cp_draw_heat_scratch_bytes(1, 4, 6) - 1) == 1 and b"cp_draw_heat_scratch_bytes" in err()
    # nothing to paint: a success that looks at nothing behind the call's own arguments ...
    assert call(N=0) == 0 and call(N=0, maps=None) == 0
    assert call(N=0, style=(2, 0, 0)) == 1                      # ... but a bad style is still a bad style


def test_heatmap_style():
    from centerpose_amd import detector, draw
    from centerpose_amd._lib import CenterposeHipError
    st = detector.HeatmapStyle()
    assert (st.colors, st.opacity, st.invert) == (None, 179, False)
    assert st.palette(1) == [(255, 255, 255)]
    assert st.palette(17) == list(detector.TRACK_PALETTE[:17])
    assert st.palette(30) == list(detector.TRACK_PALETTE) + list(detector.TRACK_PALETTE[:6])          # cycling past its length
    rec = detector.HeatmapStyle(colors=[(1, 2, 3), (4, 5, 6), (7, 8, 9)], opacity=128, invert=True).struct(2)
    assert rec.dtype == draw.DRAW_HEAT_STYLE and (int(rec["channels"][0]), int(rec["opacity"][0]), int(rec["invert"][0])) == (2, 128, 1)
    assert rec["palette"][0, :3].tolist() == [[1, 2, 3, 0], [4, 5, 6, 0], [0, 0, 0, 0]]
    for bad in (dict(opacity=0), dict(opacity=257), dict(colors=[(0, 0, 256)]), dict(colors=[(0, 0)]), dict(colors=[(1, 2, 3)] * 33)):
        with pytest.raises(CenterposeHipError):
            detector.HeatmapStyle(**bad)
    with pytest.raises(CenterposeHipError, match="colours for 3"):
        detector.HeatmapStyle(colors=[(1, 2, 3)] * 2).struct(3)                 # fewer than C colours
    for C in (0, 33):
        with pytest.raises(CenterposeHipError, match="map channels"):
            detector.HeatmapStyle().struct(C)
        with pytest.raises(CenterposeHipError, match="map channels"):
            detector.HeatmapStyle(colors=[(1, 2, 3)] * 32).palette(C)


def _meta(out_h=4, out_w=6, s=24.0):
    return {"c": np.array([12.0, 8.0], np.float32), "s": s, "out_height": out_h, "out_width": out_w}


def test_metas_and_matrix_refusals_without_a_device():
    from centerpose_amd import detector, draw, frames
    from centerpose_amd._lib import CenterposeHipError
    from centerpose_amd.post_process import get_affine_transform
    fr = [frames.Frame(4096, 16, 24, 72, 3, (0, 1, 2))]
    geometry = lambda H, W: (H // 2, W // 2)
    table = draw.heat_table(fr, False, [_meta()], geometry, 4, 6)
    want = np.array(get_affine_transform(_meta()["c"], 24.0, 0, (6, 4)), np.float64)
    want[:, 0] *= 12 / 24
    want[:, 1] *= 8 / 16
    assert table.dtype == detector.FRAME_DESC and np.array_equal(table[0]["mi"], want.reshape(6))
    assert (int(table[0]["H"]), int(table[0]["W"]), int(table[0]["NH"]), int(table[0]["mid_off"])) == (16, 24, 16, -1)
    with pytest.raises(CenterposeHipError, match="2 entries for 1 frames"):
        draw.heat_table(fr, False, [_meta(), _meta()], geometry, 4, 6)
    with pytest.raises(CenterposeHipError, match="0 entries for 1 frames"):
        draw.heat_table(fr, False, [], geometry, 4, 6)
    with pytest.raises(CenterposeHipError, match="5 x 6 map with maps of 4 x 6"):
        draw.heat_table(fr, False, [_meta(out_h=5)], geometry, 4, 6)
    for bad in (dict(s=np.nan), dict(s=1e-320), dict(c=np.array([np.inf, 8.0], np.float32))):      # k = out_w / s; t = centre - k c
        with np.errstate(all="ignore"), pytest.raises(CenterposeHipError, match="not finite"):
            draw.heat_table(fr, False, [dict(_meta(), **bad)], geometry, 4, 6)
    # the maps' own checks, in the order they are made, as far as a host tensor gets
    dev = torch.device("cuda", 0)
    for maps, match in ((np.zeros((1, 2, 4, 6), np.float32), "CUDA float32 tensor"), (torch.zeros((2, 4)), r"\[N, C, h, w\]"),
                        (torch.zeros((1, 2, 0, 6)), r"\[N, C, h, w\]"), (torch.zeros((1, 2, 4, 6)), "maps on cpu")):
        with pytest.raises(CenterposeHipError, match=match):
            draw.check_heat_maps(maps, 1, dev)


def test_draw_heatmaps_refuses_host_frames_without_a_device():
    from centerpose_amd import config, detector
    from centerpose_amd._lib import CenterposeHipError
    det = object.__new__(detector.MultiPoseDetector)
    det.cfg = config.get_cfg("dla_34")
    det.scales = det.cfg.TEST.TEST_SCALES
    det.model = type("Model", (), {"process": None, "device": "cpu"})()
    maps = torch.zeros((1, 17, 4, 6))
    with pytest.raises(CenterposeHipError, match="host arrays"):
        det.draw_heatmaps([np.zeros((8, 8, 3), np.uint8)], maps, [_meta()])
    with pytest.raises(CenterposeHipError, match="cannot be drawn on"):
        det.draw_heatmaps([], maps, [], color="p010")
    with pytest.raises(CenterposeHipError, match="not taken for drawing"):
        det.draw_heatmaps([], maps, [], color="nv12", matrix="bt601-full")
