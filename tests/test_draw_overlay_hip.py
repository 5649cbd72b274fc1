"""GPU: the overlay painters (csrc/draw_overlay.hip) through MultiPoseDetector.draw_results(style=DrawStyle(labels=..., *_opacity=...))
and run_batch(draw=..., draw_style=...).  Every comparison is of whole buffers, byte for byte: device result == host painter
(cp_draw_overlay_*_host), which tests/test_draw_overlay_cpu.py pins to the NumPy painter of tests/draw_overlay_ref.py on these very
cases -- so the guard bytes, the padding and a fourth channel are compared with everything else."""
import functools
import os

import numpy as np
import pytest
import torch

import draw_overlay_ref as oref
import draw_overlay_util as outil
import draw_ref
import draw_tracks_ref as tref
import draw_tracks_util as tu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _L():
    return outil.lib(build=False)


@functools.lru_cache(maxsize=None)
def _det():
    """A dla_34 with random weights whose default threshold lets every detection through (a sigmoid score is > 0)."""
    from centerpose_amd import config, detector
    return detector.MultiPoseDetector(config.get_cfg("dla_34", TEST__FIX_RES=False, TEST__VIS_THRESH=0.0))


def _style(T, RL, RJ, pal, opacity=(256, 256, 256), label_scale=0, prefix="PERSON", text_color=(0, 0, 0)):
    from centerpose_amd import detector
    return detector.DrawStyle(T, RL, RJ, box_color=pal[0], limb_colors=pal[1:19], joint_colors=pal[19:], labels=label_scale > 0,
                              label_prefix=prefix.lower(), label_scale=max(label_scale, 1), label_text_color=text_color, box_opacity=opacity[0],
                              limb_opacity=opacity[1], joint_opacity=opacity[2])


def _forms(kind, seed, H, W):
    return (draw_ref.bgr_forms if kind == "bgr" else draw_ref.yuv_forms)(seed, H, W)


def _on_device(form):
    dev = torch.from_numpy(form["buf"].copy()).cuda()
    views = [torch.as_strided(dev, shape, strides, off) for off, shape, strides in form["views"]]
    return dev, (views[0] if len(views) == 1 else tuple(views))


def _draw(forms, rows, vis, T, RL, RJ, pal, opacity=(256, 256, 256), label_scale=0, prefix="PERSON", text_color=(0, 0, 0), ids=None,
          id_palette=None, matrix="bt601"):
    """det.draw_results of the forms (one layout / colour) with rows [N,M,56] -> the buffers back on the host."""
    devs, frames = zip(*[_on_device(f) for f in forms])
    N = len(forms)
    rows = torch.from_numpy(np.ascontiguousarray(rows, np.float32).reshape(N, -1, 56)).cuda()
    kw = dict(matrix=matrix) if tu.is_yuv(forms[0]) else {}
    if ids is not None:
        kw.update(row_ids=torch.from_numpy(np.ascontiguousarray(ids, np.int32).reshape(N, -1)).cuda(), id_palette=id_palette)
    out = _det().draw_results(list(frames), rows, forms[0]["layout"], forms[0]["color"], vis_thresh=vis,
                              style=_style(T, RL, RJ, pal, opacity, label_scale, prefix, text_color), **kw)
    assert isinstance(out, list) and all(a is b for a, b in zip(out, frames))
    return [d.cpu().numpy() for d in devs]


# ---------------------------------------------------------------- 1. the cases of the CPU test: forms, sizes, styles, ids, matrices
@pytest.mark.parametrize("kind", ["bgr", "yuv"])
@pytest.mark.parametrize("s", range(len(draw_ref.SIZES)))
def test_device_equals_host_painter(kind, s):
    L = _L()
    H, W = draw_ref.SIZES[s]
    painted = 0
    for f, form in enumerate(_forms(kind, 100 * s + 10, H, W)):
        for k, (scale, opacity, prefix) in enumerate(oref.STYLES):
            rows, vis, (T, RL, RJ, pal), ids, idpal, tc = outil.case_inputs(kind, s, f, k)
            for with_ids in (False, True):
                for matrix in (("bt601", "bt709") if kind == "yuv" else ("bt601",)):
                    kw = dict(opacity=opacity, label_scale=scale, prefix=prefix, text_color=tc, matrix=matrix)
                    if with_ids:
                        kw.update(ids=ids, id_palette=idpal)
                    host, = outil.host_paint(L, [form], rows, vis, T, RL, RJ, pal, **kw)
                    got, = _draw([form], rows, vis, T, RL, RJ, pal, **kw)
                    assert np.array_equal(got, host), (form["name"], k, with_ids, matrix, np.nonzero(got != host)[0][:8])
                    G = draw_ref.GUARD
                    assert np.array_equal(got[:G], form["buf"][:G]) and np.array_equal(got[-G:], form["buf"][-G:])
                    painted += int((host != form["buf"]).sum())
    assert painted > 0
    assert L.cp_last_kernel() == (b"draw_overlay_kernel<bgr>" if kind == "bgr" else b"draw_overlay_kernel<yuv>")


# ---------------------------------------------------------------- 2. more rows than one chunk of the rasteriser, several tiles
@pytest.mark.parametrize("kind", ["bgr", "yuv"])
@pytest.mark.parametrize("k", [0, 3, 6])                        # labels only, opacities only, both
def test_300_rows_on_64x96(kind, k):
    L = _L()
    H, W = 64, 96
    scale, opacity, prefix = oref.STYLES[k]
    form = _forms(kind, 77, H, W)[2]
    rows = draw_ref.fuzz_rows(4242 + k, 300, H, W, dense=True)
    rows[:, 4] = np.random.RandomState(k).uniform(0.31, 1.2, 300).astype(np.float32)
    T, RL, RJ, pal = draw_ref.fuzz_style(3)
    ids, idpal = tref.fuzz_ids(5, 300), tref.fuzz_id_palette(6, 24)
    for with_ids in (False, True):
        kw = dict(opacity=opacity, label_scale=scale, prefix=prefix, text_color=(250, 250, 250))
        if with_ids:
            kw.update(ids=ids, id_palette=idpal)
        host, = outil.host_paint(L, [form], rows, draw_ref.VIS, T, RL, RJ, pal, **kw)
        got, = _draw([form], rows, draw_ref.VIS, T, RL, RJ, pal, **kw)
        assert np.array_equal(got, host), (with_ids, np.nonzero(got != host)[0][:8])
    # the late rows dead but two: what is seen comes from both chunks of 256 rows
    rows[258:, 4] = 0.0
    kw = dict(opacity=opacity, label_scale=scale, prefix=prefix)
    host, = outil.host_paint(L, [form], rows, draw_ref.VIS, T, RL, RJ, pal, **kw)
    got, = _draw([form], rows, draw_ref.VIS, T, RL, RJ, pal, **kw)
    assert np.array_equal(got, host)
    early, = outil.host_paint(L, [form], rows[:256], draw_ref.VIS, T, RL, RJ, pal, **kw)
    late = rows.copy()
    late[:256, 4] = 0.0
    late, = outil.host_paint(L, [form], late, draw_ref.VIS, T, RL, RJ, pal, **kw)
    assert not np.array_equal(host, early) and not np.array_equal(host, late)


# ---------------------------------------------------------------- 3. frames of different sizes in one call
@pytest.mark.parametrize("kind", ["bgr", "yuv"])
def test_three_sizes_in_one_call_each_frame_its_own_rows(kind):
    L = _L()
    sizes = [(1, 1), (37, 53), (64, 64)]
    pick = [0, 2, 0] if kind == "bgr" else [0, 0, 4]           # packed / bgra with padded rows / packed; planes / planes / a pitched surface
    forms = [_forms(kind, 300 + 10 * n, H, W)[p] for n, ((H, W), p) in enumerate(zip(sizes, pick))]
    assert len({(f["layout"], f["color"]) for f in forms}) == 1
    rows = np.stack([draw_ref.fuzz_rows(900 + n, 20, H, W) for n, (H, W) in enumerate(sizes)])
    rows[0, :, 4] = 1.0
    rows[0, :, 0:4] = (0, 0, 0, 0)                              # the 1 x 1 frame is painted for sure
    T, RL, RJ, pal = draw_ref.fuzz_style(9)
    ids = np.stack([tref.fuzz_ids(40 + n, 20) for n in range(3)])
    kw = dict(opacity=(128, 51, 255), label_scale=1, prefix="PERSON", text_color=(9, 8, 7), ids=ids, id_palette=tref.fuzz_id_palette(3, 7))
    host = outil.host_paint(L, forms, rows, draw_ref.VIS, T, RL, RJ, pal, **kw)
    got = _draw(forms, rows, draw_ref.VIS, T, RL, RJ, pal, **kw)
    for n in range(3):
        assert np.array_equal(got[n], host[n]), n
        assert (host[n] != forms[n]["buf"]).any(), n
    # a frame painted with another frame's rows looks different: the rows were not mixed up
    other = outil.host_paint(L, [forms[1]], rows[2], draw_ref.VIS, T, RL, RJ, pal, **dict(kw, ids=ids[2]))
    assert not np.array_equal(host[1], other[0])


# ---------------------------------------------------------------- 4. the default style keeps its kernels
@pytest.mark.parametrize("kind", ["bgr", "yuv"])
def test_last_kernel_names(kind):
    L = _L()
    form = _forms(kind, 5, 37, 53)[0]
    rows = draw_ref.fuzz_rows(11, 12, 37, 53, dense=True)
    T, RL, RJ, pal = draw_ref.fuzz_style(3)
    plain, = _draw([form], rows, draw_ref.VIS, T, RL, RJ, pal)
    assert L.cp_last_kernel() == (b"draw_raster_kernel<bgr>" if kind == "bgr" else b"draw_raster_kernel<yuv>")
    assert np.array_equal(plain, draw_ref.reference(form, rows, draw_ref.VIS, T, RL, RJ, pal))
    ids = tref.fuzz_ids(3, 12)
    _draw([form], rows, draw_ref.VIS, T, RL, RJ, pal, ids=ids, id_palette=tref.fuzz_id_palette(3, 7))
    assert L.cp_last_kernel() == (b"draw_raster_kernel<bgr,ids>" if kind == "bgr" else b"draw_raster_kernel<yuv,ids>")
    for kw in (dict(label_scale=1), dict(opacity=(256, 128, 256)), dict(opacity=(255, 256, 256), ids=ids, id_palette=tref.fuzz_id_palette(3, 7))):
        got, = _draw([form], rows, draw_ref.VIS, T, RL, RJ, pal, **kw)
        assert L.cp_last_kernel() == (b"draw_overlay_kernel<bgr>" if kind == "bgr" else b"draw_overlay_kernel<yuv>"), kw
        assert not np.array_equal(got, plain), kw


# ---------------------------------------------------------------- 5. refusals leave the frames alone
def test_python_refusals_paint_nothing():
    from centerpose_amd import detector
    from centerpose_amd._lib import CenterposeHipError
    det = _det()
    style = detector.DrawStyle(labels=True, limb_opacity=128)
    base = torch.full((8, 8, 3), 7, dtype=torch.uint8, device="cuda")
    y = torch.full((12, 8), 7, dtype=torch.uint8, device="cuda")
    rows = torch.zeros((1, 3, 56), device="cuda")
    rows[:, :, 0:5] = torch.tensor([1.0, 4.0, 6.0, 6.0, 1.0], device="cuda")
    two = torch.cat([rows, rows])
    cases = [(CenterposeHipError, "same byte", lambda: det.draw_results([torch.full((8, 1, 3), 7, dtype=torch.uint8, device="cuda").expand(8, 8, 3)],
                                                                      rows, style=style)),
             (CenterposeHipError, "same byte", lambda: det.draw_results([torch.as_strided(base, (4, 4, 3), (6, 3, 1))], rows, style=style)),
             (CenterposeHipError, "given twice", lambda: det.draw_results([base, base], two, style=style)),
             (CenterposeHipError, "given twice", lambda: det.run_batch([base, base], draw=True, draw_style=style)),
             (CenterposeHipError, "share bytes", lambda: det.draw_results([(y[:8], y[4:8].unflatten(1, (4, 2)))], rows, color="nv12", style=style)),
             (CenterposeHipError, "host arrays", lambda: det.draw_results([np.zeros((8, 8, 3), np.uint8)], rows, style=style)),
             (CenterposeHipError, "host arrays", lambda: det.run_batch([np.zeros((96, 128, 3), np.uint8)], draw=True, draw_style=style)),
             (CenterposeHipError, "unknown matrix", lambda: det.draw_results([(y[:8], y[8:].unflatten(1, (4, 2)))], rows, color="nv12",
                                                                           matrix="bt2020", style=style)),
             (CenterposeHipError, "cannot be drawn on", lambda: det.draw_results([y], rows, color="i400", style=style)),
             (CenterposeHipError, "not taken for drawing", lambda: det.run_batch([(y[:8], y[8:].unflatten(1, (4, 2)))], color="nv12",
                                                                                  matrix="bt601-full", draw=True, draw_style=style)),
             (CenterposeHipError, "DrawStyle", lambda: det.run_batch([base], draw=True, draw_style=dict(labels=True))),
             (ValueError, "draw_style", lambda: det.run_batch([base], draw_style=style)),
             (CenterposeHipError, "id_palette", lambda: det.draw_results([base], rows, style=style, id_palette=[(1, 2, 3)]))]
    for exc, match, call in cases:
        with pytest.raises(exc, match=match):
            call()
    torch.cuda.synchronize()
    assert int(base.min()) == int(base.max()) == 7 and int(y.min()) == int(y.max()) == 7
    det.draw_results([base], rows, vis_thresh=0.5, style=style)    # ... and the accepted call does paint: the bar above the box
    assert int(base[4, 1, 0]) != 7 and int(base[0, 1, 0]) != 7 and int(base[7, 7, 0]) == 7


# ---------------------------------------------------------------- 6. run_batch(draw=True, draw_style=...)
def _batch_frames(kind, sizes):
    """Fresh device frames of the given sizes from fixed host bytes as forms: packed BGR, or NV12 surfaces [H * 3 / 2, W]."""
    forms = []
    for i, (h, w) in enumerate(sizes):
        r = np.random.RandomState(800 + i)
        if kind == "bgr":
            forms.append(dict(name="bgr", layout="hwc", color="bgr", buf=r.randint(0, 256, h * w * 3).astype(np.uint8),
                              views=[(0, (h, w, 3), (3 * w, 3, 1))]))
        else:
            forms.append(dict(name="nv12 surface", layout="hwc", color="nv12", buf=r.randint(0, 256, h * 3 // 2 * w).astype(np.uint8),
                              views=[(0, (h * 3 // 2, w), (w, 1))]))
    return forms


def _device_frames(forms):
    return [torch.from_numpy(f["buf"].copy()).cuda().reshape(f["views"][0][1]) for f in forms]


def _host_overlay(L, forms, rows_h, style, ids=None, id_palette=None, vis=0.0):
    """The overlay host painter with a DrawStyle's values, one frame at a time (the frames differ in size) -> the painted buffers."""
    out = []
    for n, form in enumerate(forms):
        kw = dict(opacity=(style.box_opacity, style.limb_opacity, style.joint_opacity), label_scale=style.label_scale if style.labels else 0,
                  prefix=style.label_prefix.upper(), text_color=style.label_text_color)
        if ids is not None:
            kw.update(ids=ids[n], id_palette=id_palette)
        out += outil.host_paint(L, [form], rows_h[n], vis, style.box_thickness, style.limb_radius, style.joint_radius, style.palette(), **kw)
    return out


@pytest.mark.parametrize("kind", ["bgr", "nv12"])
def test_run_batch_draw_style(kind, monkeypatch):
    from centerpose_amd import detector
    L, det = _L(), _det()
    sizes = [(96, 128), (200, 264), (96, 128)]
    kw = dict(color=kind)
    forms = _batch_frames(kind, sizes)
    style = detector.DrawStyle(labels=True, limb_opacity=128)
    rows = det.run_batch(_device_frames(forms), return_device=True, draw=True, **kw)
    listed = det.run_batch(_device_frames(forms), **kw)
    assert bool((rows[:, :, 4] > 0).any(1).all())              # every frame has live rows under this detector's threshold

    drawn = _device_frames(forms)
    forbidden = []
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "cpu", lambda self, *a, **k: forbidden.append("cpu") or self)
        m.setattr(torch.cuda, "synchronize", lambda *a, **k: forbidden.append("synchronize"))
        m.setattr(torch.cuda.Stream, "synchronize", lambda *a, **k: forbidden.append("stream.synchronize"))
        rows_drawn = det.run_batch(drawn, return_device=True, draw=True, draw_style=style, **kw)
    assert forbidden == []
    assert L.cp_last_kernel() == (b"draw_overlay_kernel<bgr>" if kind == "bgr" else b"draw_overlay_kernel<yuv>")
    assert torch.equal(rows_drawn, rows)                       # what it returns without draw_style, bit for bit
    host = _host_overlay(L, forms, rows.cpu().numpy(), style)
    for n in range(3):
        got = drawn[n].cpu().numpy().reshape(-1)
        assert np.array_equal(got, host[n]), (n, np.nonzero(got != host[n])[0][:8])
        assert not np.array_equal(got, forms[n]["buf"])
    # the same picture from draw_results with the rows, and a different one from the default style
    by_hand = _device_frames(forms)
    assert det.draw_results(by_hand, rows, style=style, **kw) is by_hand
    assert all(torch.equal(a, b) for a, b in zip(by_hand, drawn))
    default = _device_frames(forms)
    det.run_batch(default, draw=True, **kw)
    assert L.cp_last_kernel() == (b"draw_raster_kernel<bgr>" if kind == "bgr" else b"draw_raster_kernel<yuv>")
    assert all(not torch.equal(a, b) for a, b in zip(default, drawn))
    again = _device_frames(forms)
    assert det.run_batch(again, draw=True, draw_style=style, **kw) == listed       # the list form: same return value, same picture
    assert all(torch.equal(a, b) for a, b in zip(again, drawn))


@functools.lru_cache(maxsize=None)
def _sd():
    from centerpose_amd import synth
    g = np.load(os.path.join(ROOT, "tests", "golden", "reid_features.npz"))
    return synth.make_state_dict("reid", seed=int(g["seed"]))


@pytest.mark.parametrize("kind", ["bgr", "nv12"])
def test_run_batch_draw_tracks_with_a_style(kind):
    from centerpose_amd import detector, reid, track
    L, det = _L(), _det()
    ex = reid.ReidExtractor(_sd(), capacity=8)
    trk, twin = track.DeepSortTracker(8, streams=2, n_init=1), track.DeepSortTracker(8, streams=2, n_init=1)
    forms = _batch_frames(kind, [(64, 96), (64, 96)])
    kw = dict(color=kind)
    style, ts = detector.DrawStyle(labels=True, limb_opacity=128, label_scale=2, label_text_color=(255, 255, 255)), detector.TrackStyle()
    matched = 0
    for call in range(3):
        want_rows, want_res, want_tracks = det.run_batch(_device_frames(forms), return_device=True, embed=ex, track=twin, draw="tracks", **kw)
        want_feats, want_slots = want_res.features.clone(), want_res.slots.clone()
        drawn = _device_frames(forms)
        rows, res, tracks = det.run_batch(drawn, return_device=True, embed=ex, track=trk, draw="tracks", draw_style=style, **kw)
        assert torch.equal(rows, want_rows) and torch.equal(res.features, want_feats) and torch.equal(res.slots, want_slots)
        assert len(tracks) == 2 and all(np.array_equal(a, b) for a, b in zip(tracks, want_tracks))
        M = int(rows.shape[1])
        ids = trk.row_ids(res, M).cpu().numpy()
        per_frame = [[tref.item(int(t[0]), int(t[1]), int(t[2]), int(t[3]), "ID %d" % t[4], detector.TRACK_PALETTE[int(t[4]) % 24], (255, 255, 255))
                      for t in tr] for tr in tracks]
        host = _host_overlay(L, forms, rows.cpu().numpy(), style, ids, detector.TRACK_PALETTE)
        host = tu.host_paint_tracks(L, forms, per_frame, ts.box_thickness, ts.font_scale, bufs=host)
        for n in range(2):
            got = drawn[n].cpu().numpy().reshape(-1)
            assert np.array_equal(got, host[n]), (call, n, np.nonzero(got != host[n])[0][:8])
        matched += int((ids >= 0).sum())
    assert matched > 0                                          # later calls painted identity colours under the labels
