"""GPU: the heat-map overlay (csrc/draw_heat.hip) through cp_draw_heat_frames_u8 / cp_draw_heat_yuv_frames_u8 and through
MultiPoseDetector.draw_heatmaps.  Every comparison is of whole buffers, byte for byte: device result == host painter
(cp_draw_heat_*_host), which tests/test_draw_heat_cpu.py pins to the NumPy painter of tests/draw_heat_ref.py on these very cases -- so the
guard bytes, the padding and a fourth channel are compared with everything else."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import draw_heat_ref as href
import draw_heat_util as hutil
import draw_ref

pytestmark = pytest.mark.gpu
VP, LL = ctypes.c_void_p, ctypes.c_longlong
PACKED, GENERAL, YUV = b"draw_heat_blend_kernel<bgr_packed>", b"draw_heat_blend_kernel<bgr>", b"draw_heat_blend_kernel<yuv>"


def _L():
    return hutil.lib(build=False)


@functools.lru_cache(maxsize=None)
def _det():
    """A dla_34 with random weights, FLIP_TEST on, the network input following the frame."""
    from centerpose_amd import config, detector
    return detector.MultiPoseDetector(config.get_cfg("dla_34", TEST__FIX_RES=False, TEST__FLIP_TEST=True))


def _on_device(form):
    dev = torch.from_numpy(form["buf"].copy()).cuda()
    views = [torch.as_strided(dev, shape, strides, off) for off, shape, strides in form["views"]]
    return dev, (views[0] if len(views) == 1 else tuple(views))


def _maps_on_device(maps):
    """A float32 NumPy view [N, C, h, w] -> the same view (shape, element strides) of a device copy of the memory it lies in."""
    base = maps
    while base.base is not None:
        base = base.base
    dev = torch.from_numpy(np.ascontiguousarray(base).reshape(-1)).cuda()
    off = (maps.ctypes.data - base.ctypes.data) // 4
    return torch.as_strided(dev, maps.shape, [s // 4 for s in maps.strides], off)


def _capi(L, forms, maps, matrices, palette, opacity, invert, matrix="bt601"):
    """cp_draw_heat_*_u8 over device copies of the forms' buffers -> the buffers back on the host."""
    yuv = hutil.is_yuv(forms[0])
    devs = [torch.from_numpy(f["buf"].copy()).cuda() for f in forms]
    table = hutil.table_of(forms, [d.data_ptr() for d in devs], matrices)
    table_dev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).cuda()
    m = _maps_on_device(maps)
    N, C, h, w = maps.shape
    st = hutil.style_struct(C, opacity, invert, palette)
    nbytes = int(L.cp_draw_heat_scratch_bytes(N, h, w))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    fn = L.cp_draw_heat_yuv_frames_u8 if yuv else L.cp_draw_heat_frames_u8
    rc = fn(VP(table_dev.data_ptr()), table.ctypes.data_as(VP), N, VP(m.data_ptr()), *(LL(s) for s in m.stride()), C, h, w, st.ctypes.data_as(VP),
            *((hutil.MATRIX_IDS[matrix],) if yuv else ()), VP(scratch.data_ptr()), ctypes.c_size_t(nbytes),
            VP(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.cp_last_error()
    torch.cuda.synchronize()
    return [d.cpu().numpy() for d in devs]


def _meta(H, W, h, w):
    """The meta of an H x W frame whose longer side fills an h x w map (what a pre-process with these sizes would hand out)."""
    return {"c": np.array([W / 2.0, H / 2.0], np.float32), "s": max(H, W) * 1.0, "out_height": h, "out_width": w}


def _matrix_of(det, meta, H, W):
    from centerpose_amd import draw
    new_h, new_w = det.input_geometry(H, W, 1)[0:2]
    return draw.heat_transform(meta, H, W, new_h, new_w)


def _style(palette, opacity, invert):
    from centerpose_amd import detector
    return detector.HeatmapStyle(colors=palette, opacity=opacity, invert=invert)


# ---------------------------------------------------------------- 1. the cases of the CPU test through the C entry points
@pytest.mark.parametrize("kind", ["bgr", "yuv"])
def test_device_equals_host_painter(kind):
    L = _L()
    names = set()
    for name, form, maps, T, pal, opacity, invert, matrix in hutil.cases(kind):
        host, = hutil.host_paint(L, [form], maps, [T], pal, opacity, invert, matrix)
        got, = _capi(L, [form], maps, [T], pal, opacity, invert, matrix)
        assert np.array_equal(got, host), (name, np.nonzero(got != host)[0][:8])
        G = draw_ref.GUARD
        assert np.array_equal(got[:G], form["buf"][:G]) and np.array_equal(got[-G:], form["buf"][-G:]), name
        names.add(L.cp_last_kernel())
        packed = form["layout"] == "hwc" and form["views"][0][1][-1] == 3
        assert L.cp_last_kernel() == (YUV if kind == "yuv" else PACKED if packed else GENERAL), name
    assert names == ({YUV} if kind == "yuv" else {PACKED, GENERAL})


# ---------------------------------------------------------------- 2. the same pictures through det.draw_heatmaps
@pytest.mark.parametrize("kind", ["bgr", "yuv"])
def test_draw_heatmaps_equals_host_painter(kind):
    L, det = _L(), _det()
    for s, (H, W) in enumerate(href.SIZES):
        for f, form in enumerate(hutil.forms_of(kind, 500 + 10 * s, H, W)):
            C, opacity, invert = href.STYLES[(s + f) % len(href.STYLES)]
            h, w = href.MAP_SIZES[(s + f) % 2]
            maps, pal = href.fuzz_maps(60 + 7 * s + f, 2, C, h, w)[0::2], href.fuzz_palette(s + f, C)
            meta = _meta(H, W, h, w)
            T = _matrix_of(det, meta, H, W)
            matrix = ("bt601", "bt709")[f % 2] if kind == "yuv" else "bt601"
            host, = hutil.host_paint(L, [form], maps, [T], pal, opacity, invert, matrix)
            dev, frame = _on_device(form)
            kw = dict(matrix=matrix) if kind == "yuv" else {}
            out = det.draw_heatmaps([frame], _maps_on_device(maps), [meta], 1, form["layout"], form["color"], style=_style(pal, opacity, invert),
                                    **kw)
            assert isinstance(out, list) and out[0] is frame
            got = dev.cpu().numpy()
            assert np.array_equal(got, host), (form["name"], H, W, np.nonzero(got != host)[0][:8])
            assert (got != form["buf"]).any() or opacity == 1
    # one frame, maps [C, h, w], a meta instead of a list, the default style: white for C = 1
    form = hutil.forms_of(kind, 900, 16, 16)[0]
    maps, meta = href.fuzz_maps(9, 1, 1, 5, 7), _meta(16, 16, 5, 7)
    host, = hutil.host_paint(L, [form], maps, [_matrix_of(det, meta, 16, 16)], [(255, 255, 255)], 179, False)
    dev, frame = _on_device(form)
    det.draw_heatmaps([frame], _maps_on_device(maps)[0], meta, layout=form["layout"], color=form["color"])
    assert np.array_equal(dev.cpu().numpy(), host)


# ---------------------------------------------------------------- 3. which instantiation runs
def _packed_at(offset, H=37, W=53, seed=21):
    """A packed hwc BGR frame whose first byte lies `offset` bytes into a buffer (allocations are at least 4-byte aligned): with rows of
    3 * 53 = 159 bytes every row starts at another address modulo 4."""
    form = draw_ref._form(seed + offset, "packed bgr at byte %d" % offset, "hwc", "bgr", [(offset, (H, W, 3), (3 * W, 3, 1))])
    draw_ref.numpy_views(form["buf"], form)[0][...] = np.random.RandomState(seed).randint(0, 256, (H, W, 3))     # the pixels: the seed's
    return form


def test_last_kernel_names_and_the_two_instantiations_agree():
    L, det = _L(), _det()
    H, W, h, w = 37, 53, 8, 12
    maps, pal, meta = href.fuzz_maps(31, 1, 17, h, w), href.fuzz_palette(32, 17), _meta(H, W, h, w)
    T = _matrix_of(det, meta, H, W)
    style = _style(pal, 179, False)
    pictures = []
    for offset in (0, 1, 2, 3):
        form = _packed_at(offset)
        dev, frame = _on_device(form)
        assert frame.data_ptr() % 4 == offset
        det.draw_heatmaps([frame], _maps_on_device(maps), [meta], style=style)
        assert L.cp_last_kernel() == PACKED, offset
        host, = hutil.host_paint(L, [form], maps, [T], pal, 179, False)
        got = dev.cpu().numpy()
        assert np.array_equal(got, host), (offset, np.nonzero(got != host)[0][:8])
        pictures.append(frame.cpu().numpy())
    assert all(np.array_equal(p, pictures[0]) for p in pictures)       # the same pixels wherever they lie
    # the same pixels behind a pixel stride of 4, and as planes: the general instantiation, the same picture
    pixels = draw_ref.numpy_views(_packed_at(0)["buf"], _packed_at(0))[0]
    wide = torch.full((H, W, 4), 0xC3, dtype=torch.uint8, device="cuda")
    wide[..., :3] = torch.from_numpy(pixels.copy()).cuda()
    det.draw_heatmaps([wide[..., :3]], _maps_on_device(maps), [meta], style=style)
    assert L.cp_last_kernel() == GENERAL
    assert np.array_equal(wide[..., :3].cpu().numpy(), pictures[0]) and bool((wide[..., 3] == 0xC3).all())
    planes = torch.from_numpy(np.ascontiguousarray(pixels.transpose(2, 0, 1))).cuda()
    det.draw_heatmaps([planes], _maps_on_device(maps), [meta], layout="chw", style=style)
    assert L.cp_last_kernel() == GENERAL
    assert np.array_equal(planes.cpu().numpy().transpose(1, 2, 0), pictures[0])


def test_mixed_batch_runs_the_general_instantiation():
    """One packed frame and one pitched 4-channel frame in one call: the launcher picks one instantiation per call, <bgr>."""
    L = _L()
    forms = [draw_ref.bgr_forms(41, 37, 53)[0], draw_ref.bgr_forms(42, 16, 16)[2]]
    assert {f["color"] for f in forms} == {"bgr"} and forms[1]["views"][0][1][-1] == 4
    maps, pal = href.fuzz_maps(43, 2, 17, 5, 7), href.fuzz_palette(44, 17)
    Ts = [href.fit_matrix(37, 53, 5, 7), href.fit_matrix(16, 16, 5, 7)]
    host = hutil.host_paint(L, forms, maps, Ts, pal, 179, True)
    got = _capi(L, forms, maps, Ts, pal, 179, True)
    assert L.cp_last_kernel() == GENERAL
    for n in range(2):
        assert np.array_equal(got[n], host[n]), n
    got = _capi(L, [forms[0], _packed_at(3, 16, 16, 45)], maps, Ts, pal, 179, True)       # two packed frames of two sizes: <bgr_packed>
    assert L.cp_last_kernel() == PACKED
    host = hutil.host_paint(L, [forms[0], _packed_at(3, 16, 16, 45)], maps, Ts, pal, 179, True)
    assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1])


# ---------------------------------------------------------------- 4. stream discipline
def test_side_stream_and_no_synchronisation(monkeypatch):
    L, det = _L(), _det()
    H, W, h, w = 70, 90, 8, 12
    form = draw_ref.bgr_forms(51, H, W)[0]
    maps, pal, meta = href.fuzz_maps(52, 1, 17, h, w), href.fuzz_palette(53, 17), _meta(H, W, h, w)
    host, = hutil.host_paint(L, [form], maps, [_matrix_of(det, meta, H, W)], pal, 179, False)
    dev, frame = _on_device(form)
    m = _maps_on_device(maps)
    det.draw_heatmaps([_on_device(form)[1]], m, [meta])         # the detector's staging buffers exist from here on
    ballast = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    forbidden = []
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", lambda self, *a, **k: forbidden.append("cpu") or self)
        mp.setattr(torch.cuda, "synchronize", lambda *a, **k: forbidden.append("synchronize"))
        mp.setattr(torch.cuda.Stream, "synchronize", lambda *a, **k: forbidden.append("stream.synchronize"))
        with torch.cuda.stream(side):
            for _ in range(20):                                 # 40 GiB of memory traffic in front of the call: some ten milliseconds
                ballast.add_(1.0)
            det.draw_heatmaps([frame], m, [meta], style=_style(pal, 179, False))
            pending = not torch.cuda.current_stream().query()   # the call came back with its stream still busy: nothing waited
        idle = torch.cuda.current_stream().query()              # the default stream got no work
    assert forbidden == [] and pending and idle
    side.synchronize()
    assert np.array_equal(dev.cpu().numpy(), host)


# ---------------------------------------------------------------- 5. refusals leave the frames alone
def test_python_refusals_paint_nothing():
    from centerpose_amd._lib import CenterposeHipError
    det = _det()
    base = torch.full((8, 8, 3), 7, dtype=torch.uint8, device="cuda")
    y = torch.full((12, 8), 7, dtype=torch.uint8, device="cuda")
    nv12 = (y[:8], y[8:].unflatten(1, (4, 2)))
    maps = torch.full((1, 17, 2, 2), 0.5, device="cuda")
    meta = _meta(8, 8, 2, 2)
    two = torch.cat([maps, maps])
    cases = [("same byte", lambda: det.draw_heatmaps([torch.full((8, 1, 3), 7, dtype=torch.uint8, device="cuda").expand(8, 8, 3)], maps, [meta])),
             ("same byte", lambda: det.draw_heatmaps([torch.as_strided(base, (4, 4, 3), (6, 3, 1))], maps, [meta])),
             ("given twice", lambda: det.draw_heatmaps([base, base], two, [meta, meta])),
             ("host arrays", lambda: det.draw_heatmaps([np.zeros((8, 8, 3), np.uint8)], maps, [meta])),
             ("cannot be drawn on", lambda: det.draw_heatmaps([y], maps, [meta], color="p010")),
             ("cannot be drawn on", lambda: det.draw_heatmaps([y], maps, [meta], color="i400")),
             ("not taken for drawing", lambda: det.draw_heatmaps([nv12], maps, [meta], color="nv12", matrix="bt601-full")),
             ("maps on cpu", lambda: det.draw_heatmaps([base], maps.cpu(), [meta])),
             ("float32", lambda: det.draw_heatmaps([base], maps.half(), [meta])),
             ("2 images for 1 frames", lambda: det.draw_heatmaps([base], two, [meta])),
             ("map channels", lambda: det.draw_heatmaps([base], torch.zeros((1, 33, 2, 2), device="cuda"), [meta])),
             ("map channels", lambda: det.draw_heatmaps([base], torch.zeros((1, 0, 2, 2), device="cuda"), [meta])),
             ("2 entries for 1 frames", lambda: det.draw_heatmaps([base], maps, [meta, meta])),
             ("map with maps of", lambda: det.draw_heatmaps([base], maps, [_meta(8, 8, 3, 2)])),
             ("HeatmapStyle", lambda: det.draw_heatmaps([base], maps, [meta], style=dict(opacity=128))),
             ("colours for 17", lambda: det.draw_heatmaps([base], maps, [meta], style=_style([(1, 2, 3)], 128, False)))]
    for match, call in cases:
        with pytest.raises(CenterposeHipError, match=match):
            call()
    torch.cuda.synchronize()
    assert int(base.min()) == int(base.max()) == 7 and int(y.min()) == int(y.max()) == 7
    det.draw_heatmaps([base], maps, [meta])                     # ... and the accepted calls do paint
    det.draw_heatmaps([nv12], maps, [meta], color="nv12")
    assert int(base.max()) != 7 and int(y[:8].max()) != 7


# ---------------------------------------------------------------- 6. end to end on the network's own maps
@pytest.mark.parametrize("kind", ["bgr", "nv12"])
def test_end_to_end_on_the_joint_heat_maps(kind):
    L, det = _L(), _det()
    H, W = 64, 96
    r = np.random.RandomState(71)
    if kind == "bgr":
        forms = [dict(name="bgr", layout="hwc", color="bgr", buf=r.randint(0, 256, H * W * 3).astype(np.uint8), views=[(0, (H, W, 3), (3 * W, 3, 1))])
                 for _ in range(2)]
    else:
        forms = [dict(name="nv12 surface", layout="hwc", color="nv12", buf=r.randint(0, 256, H * 3 // 2 * W).astype(np.uint8),
                      views=[(0, (H * 3 // 2, W), (W, 1))]) for _ in range(2)]
    frames = [torch.from_numpy(f["buf"].copy()).cuda().reshape(f["views"][0][1]) for f in forms]
    x, metas = det.pre_process_batch(frames, 1, color=kind)
    outputs, dets = det.process(x)
    plain_outputs, plain_dets = [o.clone() for o in outputs], dets.clone()
    hm_hp = outputs[4][0::2]                                    # the images of the flip-test batch, not their twins
    assert tuple(hm_hp.shape) == (2, 17, metas[0]["out_height"], metas[0]["out_width"]) and not hm_hp.is_contiguous()
    assert det.draw_heatmaps(frames, hm_hp, metas, color=kind) is frames
    assert L.cp_last_kernel() == (PACKED if kind == "bgr" else YUV)
    maps_host = np.ascontiguousarray(hm_hp.cpu().numpy())
    Ts = [_matrix_of(det, m, H, W) for m in metas]
    from centerpose_amd import detector
    host = hutil.host_paint(L, forms, maps_host, Ts, detector.TRACK_PALETTE[:17], 179, False)
    for n in range(2):
        got = frames[n].cpu().numpy().reshape(-1)
        assert np.array_equal(got, host[n]), (n, np.nonzero(got != host[n])[0][:8])
        assert not np.array_equal(got, forms[n]["buf"])
    # the drawing call changed nothing the network handed out, and the next run gives the same again
    assert all(torch.equal(a, b) for a, b in zip(outputs, plain_outputs)) and torch.equal(dets, plain_dets)
    outputs2, dets2 = det.process(x)
    assert all(torch.equal(a, b) for a, b in zip(outputs2, plain_outputs)) and torch.equal(dets2, plain_dets)
