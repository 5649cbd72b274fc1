"""GPU: draw_tracks (csrc/draw_tracks.hip), the identity-coloured draw_results, DeepSortTracker.row_ids and run_batch(draw="tracks").
Every picture is compared as a whole buffer, byte for byte: device result == host painter == the NumPy painter of
tests/draw_tracks_ref.py, so the guard bytes, the padding and a fourth channel are compared with everything else."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import draw_ref
import draw_tracks_ref as tref
import draw_tracks_util as tu
import draw_util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p


def _L():
    return draw_util.lib_loaded()


@functools.lru_cache(maxsize=None)
def _det():
    """A dla_34 with random weights whose default threshold lets every detection through (a sigmoid score is > 0)."""
    from centerpose_amd import config, detector
    return detector.MultiPoseDetector(config.get_cfg("dla_34", TEST__FIX_RES=False, TEST__VIS_THRESH=0.0))


def _forms(kind, seed, H, W):
    return (draw_ref.bgr_forms if kind == "bgr" else draw_ref.yuv_forms)(seed, H, W)


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _on_device(form):
    dev = torch.from_numpy(form["buf"].copy()).cuda()
    views = [torch.as_strided(dev, shape, strides, off) for off, shape, strides in form["views"]]
    return dev, (views[0] if len(views) == 1 else tuple(views))


def dev_paint_tracks(forms, per_frame, T, s, matrix="bt601", devs=None, expect=0):
    """cp_draw_tracks_*_u8 through ctypes over device copies of the forms' buffers -> the buffers back on the host."""
    from centerpose_amd import _lib
    L, yuv = _L(), tu.is_yuv(forms[0])
    devs = [torch.from_numpy(f["buf"].copy()).cuda() for f in forms] if devs is None else devs
    table = draw_util.table_of(forms, [d.data_ptr() for d in devs])
    items, counts = tu.item_table(per_frame, yuv, matrix)
    t_dev, i_dev, c_dev = _up(table), _up(items), _up(counts)
    fn = L.cp_draw_tracks_yuv_frames_u8 if yuv else L.cp_draw_tracks_frames_u8
    rc = fn(VP(t_dev.data_ptr()), table.ctypes.data_as(VP), len(forms), VP(i_dev.data_ptr()), items.ctypes.data_as(VP), VP(c_dev.data_ptr()),
            counts.ctypes.data_as(VP), items.shape[1], T, s, _lib.stream())
    assert rc == expect, L.cp_last_error()
    return [d.cpu().numpy() for d in devs]


# ---------------------------------------------------------------- 1. the fuzz cases of the CPU test
@pytest.mark.parametrize("kind", ["bgr", "yuv"])
@pytest.mark.parametrize("sz", range(len(tref.SIZES)))
def test_device_equals_host_painter_equals_numpy(kind, sz):
    L = _L()
    H, W = tref.SIZES[sz]
    painted = 0
    for f, form in enumerate(_forms(kind, 100 * sz + 20, H, W)):
        for trial, (T, s) in enumerate(tref.STYLES):
            seed = 2000 * sz + 20 * f + trial + (700 if kind == "yuv" else 0)
            items = tref.fuzz_items(seed, 14, H, W)
            matrix = "bt709" if trial % 3 == 2 else "bt601"
            want = tref.reference(form, items, T, s, matrix)
            host, = tu.host_paint_tracks(L, [form], [items], T, s, matrix)
            got, = dev_paint_tracks([form], [items], T, s, matrix)
            assert np.array_equal(host, want), (form["name"], seed)
            assert np.array_equal(got, want), (form["name"], seed, T, s, np.nonzero(got != want)[0][:8])
            painted += int((want != form["buf"]).sum())
    assert painted > 0
    assert L.cp_last_kernel() == (b"draw_tracks_kernel<bgr>" if kind == "bgr" else b"draw_tracks_kernel<yuv>")


# ---------------------------------------------------------------- 2. mixed sizes and plane forms in one launch, counts per frame
@pytest.mark.parametrize("kind", ["bgr", "yuv"])
def test_mixed_sizes_in_one_launch_each_frame_its_own_items(kind):
    L = _L()
    sizes = [(1, 1), (37, 53), (64, 96), (7, 5)]
    pick = [0, 2, 0, 2] if kind == "bgr" else [0, 0, 4, 0]      # packed / bgra with padded rows; planes / a pitched surface
    forms = [_forms(kind, 300 + 10 * n, H, W)[p] for n, ((H, W), p) in enumerate(zip(sizes, pick))]
    assert len({(f["layout"], f["color"]) for f in forms}) == 1
    per_frame = [[tref.item(0, 0, 0, 0, "")], tref.fuzz_items(51, 9, 37, 53), tref.fuzz_items(52, 20, 64, 96), []]
    want = [tref.reference(f, it, 3, 2) for f, it in zip(forms, per_frame)]
    host = tu.host_paint_tracks(L, forms, per_frame, 3, 2)
    got = dev_paint_tracks(forms, per_frame, 3, 2)
    for n in range(4):
        assert np.array_equal(host[n], want[n]) and np.array_equal(got[n], want[n]), n
    assert all((want[n] != forms[n]["buf"]).any() for n in range(3)) and np.array_equal(want[3], forms[3]["buf"])
    assert not np.array_equal(want[2], tref.reference(forms[2], per_frame[1], 3, 2))       # the items were not mixed up


# ---------------------------------------------------------------- 3. more items than one chunk
@pytest.mark.parametrize("kind", ["bgr", "yuv"])
def test_300_overlapping_items(kind):
    form = _forms(kind, 77, 37, 53)[2]
    items = tref.fuzz_items(31, 300, 37, 53)
    win = tref.item_winners(items, 37, 53, 2, 1) // 3
    assert (win >= 256).any() and ((win >= 0) & (win < 256)).any()             # the winners come from both chunks of 256 items
    got, = dev_paint_tracks([form], [items], 2, 1)
    assert np.array_equal(got, tref.reference(form, items, 2, 1))


# ---------------------------------------------------------------- 4. the Python entry point: labels, colours, nothing to paint
@pytest.mark.parametrize("kind", ["bgr", "yuv"])
def test_draw_tracks_through_the_detector(kind):
    from centerpose_amd import detector
    det = _det()
    H, W = 64, 96
    forms = [_forms(kind, 500 + n, H, W)[1 if kind == "bgr" else 4] for n in range(2)]       # rgb with 4 channels; a pitched nv12 surface
    palette = tref.fuzz_id_palette(3, 5)
    style = detector.TrackStyle(2, 1, "t:", (250, 240, 1), palette)
    tracks = [np.array([[5, 6, 60, 50, 3], [40, 20, 95, 63, 12345678901234], [-30, -20, 20, 30, 7]], np.int64),
              np.array([[70, 40, 20, 10, 4]], np.int64)]
    per_frame = [[tref.item(int(t[0]), int(t[1]), int(t[2]), int(t[3]), "T:%d" % t[4], palette[int(t[4]) % 5], (250, 240, 1)) for t in tr]
                 for tr in tracks]
    assert max(len(it["text"]) for it in per_frame[0]) == 16
    matrix = "bt709" if kind == "yuv" else "bt601"
    devs, frames = zip(*[_on_device(f) for f in forms])
    kw = dict(matrix=matrix) if kind == "yuv" else {}
    out = det.draw_tracks(list(frames), tracks, forms[0]["layout"], forms[0]["color"], style=style, **kw)
    assert isinstance(out, list) and all(a is b for a, b in zip(out, frames))
    for n in range(2):
        want = tref.reference(forms[n], per_frame[n], 2, 1, matrix)
        assert np.array_equal(devs[n].cpu().numpy(), want), n
        assert (want != forms[n]["buf"]).any()
    # no frames, no tracks, and a frame without tracks: nothing is painted
    assert det.draw_tracks([], []) == []
    dev, frame = _on_device(forms[0])
    det.draw_tracks([frame], [np.zeros((0, 5), np.int64)], forms[0]["layout"], forms[0]["color"], **kw)
    assert np.array_equal(dev.cpu().numpy(), forms[0]["buf"])


# ---------------------------------------------------------------- 5. refusals leave the frames alone
def test_python_refusals_paint_nothing():
    from centerpose_amd import detector
    from centerpose_amd._lib import CenterposeHipError
    det = _det()
    base = torch.full((16, 16, 3), 7, dtype=torch.uint8, device="cuda")
    other = torch.full((16, 16, 3), 7, dtype=torch.uint8, device="cuda")
    one = [np.array([[1, 1, 12, 12, 5]], np.int64)]
    cases = [(CenterposeHipError, "given twice", lambda: det.draw_tracks([base, base], one * 2)),
             (CenterposeHipError, "same byte", lambda: det.draw_tracks([base[:, :1].expand(16, 16, 3)], one)),
             (CenterposeHipError, "host arrays", lambda: det.draw_tracks([np.zeros((8, 8, 3), np.uint8)], one)),
             (CenterposeHipError, "1 arrays for 2 frames", lambda: det.draw_tracks([base, other], one)),
             (CenterposeHipError, "TrackStyle", lambda: det.draw_tracks([base], one, style=detector.DrawStyle())),
             (CenterposeHipError, "integer arrays", lambda: det.draw_tracks([base], [np.zeros((1, 5), np.float32)])),
             (ValueError, "at most 16", lambda: det.draw_tracks([base, other], one + [np.array([[1, 1, 9, 9, 10 ** 15]], np.int64)])),
             (ValueError, "needs track=", lambda: det.run_batch([base], draw="tracks")),
             (CenterposeHipError, "row_ids", lambda: det.draw_results([base], torch.zeros((1, 2, 56), device="cuda"),
                                                                        row_ids=torch.zeros((1, 2), dtype=torch.int64, device="cuda"))),
             (CenterposeHipError, "row_ids", lambda: det.draw_results([base], torch.zeros((1, 2, 56), device="cuda"),
                                                                        row_ids=np.zeros((1, 2), np.int32))),
             (CenterposeHipError, "row_ids", lambda: det.draw_results([base], torch.zeros((1, 2, 56), device="cuda"), id_palette=[(1, 2, 3)]))]
    for exc, match, call in cases:
        with pytest.raises(exc, match=match):
            call()
    torch.cuda.synchronize()
    assert int(base.min()) == int(base.max()) == 7 and int(other.min()) == int(other.max()) == 7
    det.draw_tracks([base], one)                               # ... and the accepted call does paint
    assert int(base[1, 1, 0]) != 7 and int(base[0, 0, 0]) == 7


@pytest.mark.parametrize("yuv", [False, True])
def test_bad_second_frame_through_ctypes_launches_nothing(yuv):
    forms = [_forms("yuv" if yuv else "bgr", 50 + n, 7, 5)[0] for n in range(2)]
    devs = [torch.from_numpy(f["buf"].copy()).cuda() for f in forms]
    good = [tref.item(0, 0, 4, 6, "A")]
    bad = [dict(tref.item(0, 0, 4, 6, "A"), x1=-3)]              # unsorted corners in the SECOND frame's item
    dev_paint_tracks(forms, [good, bad], 2, 1, devs=devs, expect=1)
    assert b"sorted" in _L().cp_last_error()
    torch.cuda.synchronize()
    assert all(np.array_equal(d.cpu().numpy(), f["buf"]) for d, f in zip(devs, forms))
    dev_paint_tracks(forms, [good, good], 2, 1, devs=devs)
    assert all(not np.array_equal(d.cpu().numpy(), f["buf"]) for d, f in zip(devs, forms))


# ---------------------------------------------------------------- 6. per-row track ids
@pytest.mark.parametrize("S,q,M,capacity", [(1, 1, 1, 1), (2, 4, 9, 8), (3, 5, 7, 17), (2, 6, 4, 13), (3, 300, 700, 900)])
def test_row_ids_device_equals_host_twin(S, q, M, capacity):
    from centerpose_amd import _lib
    L = _L()
    slots, slot_ids, want = tu.row_ids_case(5 + S + q, S, q, M, capacity)
    rc, host = tu.host_row_ids(L, slots, slot_ids, capacity, S, q, M)
    assert rc == 0 and np.array_equal(host, want)
    s_dev, i_dev = torch.from_numpy(slots).cuda(), torch.from_numpy(slot_ids).cuda()
    out = torch.full((S * M + 8,), -99, dtype=torch.int32, device="cuda")
    assert L.cp_track_row_ids(VP(s_dev.data_ptr()), VP(i_dev.data_ptr()), capacity, S, q, M, VP(out.data_ptr()), _lib.stream()) == 0
    got = out.cpu().numpy()
    assert np.array_equal(got[:S * M].reshape(S, M), want) and (got[S * M:] == -99).all()
    # a slot outside [0, S * M) is skipped on the device, never written through
    slots[0] = S * M + 3
    out.fill_(-99)
    assert L.cp_track_row_ids(VP(torch.from_numpy(slots).cuda().data_ptr()), VP(i_dev.data_ptr()), capacity, S, q, M, VP(out.data_ptr()),
                              _lib.stream()) == 0
    assert (out.cpu().numpy()[S * M:] == -99).all()


def test_tracker_row_ids():
    from centerpose_amd import reid, track
    trk = track.DeepSortTracker(8, streams=2)
    M = 6
    slots = np.array([3, 0, -1, 5, 6 + 2, -1, 6 + 4, 6 + 1], np.int32)
    trk.assignments[:] = [[11, -1, 7, 2 ** 31 - 1], [5, 9, -1, 6]]
    res = reid.ReidResult(torch.zeros((8, 512), device="cuda"), torch.from_numpy(slots).cuda(), torch.zeros((2,), dtype=torch.int32, device="cuda"))
    got = trk.row_ids(res, M)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (2, M)
    want = np.full((2, M), -1, np.int32)
    want[0, 3], want[0, 5], want[1, 2], want[1, 1] = 11, 2 ** 31 - 1, 5, 6
    assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError, match="int32"):
        trk.row_ids(reid.ReidResult(res.features, res.slots[:6], res.counts), M)
    with pytest.raises(ValueError, match="ReidResult"):
        trk.row_ids(res.slots, M)


# ---------------------------------------------------------------- 7. poses in identity colours
def _style(T, RL, RJ, pal):
    from centerpose_amd import detector
    return detector.DrawStyle(T, RL, RJ, box_color=pal[0], limb_colors=pal[1:19], joint_colors=pal[19:])


@pytest.mark.parametrize("kind", ["bgr", "yuv"])
@pytest.mark.parametrize("sz", [1, 2, 3])
def test_rows_in_identity_colours(kind, sz):
    L, det = _L(), _det()
    H, W = tref.SIZES[sz]
    differs = 0
    for f, form in enumerate(_forms(kind, 100 * sz + 30, H, W)):
        seed = 3000 * sz + 10 * f + (500 if kind == "yuv" else 0)
        rows = draw_ref.fuzz_rows(seed, 12, H, W)
        T, RL, RJ, pal = draw_ref.fuzz_style(seed)
        matrix = "bt709" if f % 2 else "bt601"
        idpal = tref.fuzz_id_palette(seed, [1, 7, 64][f % 3])
        ids = tref.fuzz_ids(seed, 12)
        want = tref.reference_rows(form, rows, draw_ref.VIS, T, RL, RJ, pal, ids, idpal, matrix)
        host, = tu.host_paint_rows_ids(L, [form], rows, ids, idpal, draw_ref.VIS, T, RL, RJ, pal, matrix)
        kw = dict(matrix=matrix) if kind == "yuv" else {}
        plain = None
        for use in (ids, np.full(12, -1, np.int32), None):
            dev, frame = _on_device(form)
            row_ids = None if use is None else torch.from_numpy(use.reshape(1, 12)).cuda()
            det.draw_results([frame], torch.from_numpy(rows).cuda().reshape(1, 12, 56), form["layout"], form["color"], vis_thresh=draw_ref.VIS,
                             style=_style(T, RL, RJ, pal), row_ids=row_ids, id_palette=idpal if use is not None else None, **kw)
            got = dev.cpu().numpy()
            if use is ids:
                assert np.array_equal(host, want) and np.array_equal(got, want), (form["name"], seed)
                assert L.cp_last_kernel() == (b"draw_raster_kernel<bgr,ids>" if kind == "bgr" else b"draw_raster_kernel<yuv,ids>")
            elif use is not None:
                plain = got
            else:
                assert np.array_equal(got, plain), form["name"]                 # all ids -1 == no ids at all, byte for byte
                assert np.array_equal(got, draw_ref.reference(form, rows, draw_ref.VIS, T, RL, RJ, pal, matrix))
                differs += int(not np.array_equal(got, want))
    assert differs > 0


# ---------------------------------------------------------------- 8. run_batch(draw="tracks")
@functools.lru_cache(maxsize=None)
def _sd():
    from centerpose_amd import synth
    g = np.load(os.path.join(ROOT, "tests", "golden", "reid_features.npz"))
    return synth.make_state_dict("reid", seed=int(g["seed"]))


def _image(seed, H, W):
    """A B, G, R picture with large-scale structure, uint8 [H, W, 3]."""
    r = np.random.RandomState(seed)
    grid = torch.from_numpy(r.uniform(0, 255, (1, 3, 5, 6)))
    up = torch.nn.functional.interpolate(grid, size=(H, W), mode="bilinear", align_corners=False)[0].numpy()
    return np.clip(np.rint(up + r.uniform(-20, 20, up.shape)), 0, 255).astype(np.uint8).transpose(1, 2, 0).copy()


def _host_frames(kind, H, W):
    """Two frames as flat host buffers with their forms: packed BGR, or an NV12 surface [H * 3 / 2, W]."""
    forms = []
    for n in range(2):
        if kind == "bgr":
            buf = _image(31 + n, H, W).reshape(-1)
            forms.append(dict(name="bgr", layout="hwc", color="bgr", buf=buf, views=[(0, (H, W, 3), (3 * W, 3, 1))]))
        else:
            img = _image(31 + n, H, W)
            buf = np.concatenate([img[:, :, 1].reshape(-1), np.full(H // 2 * W, 128, np.uint8) + (img[::2, :, 0].reshape(-1) >> 3)])
            forms.append(dict(name="nv12 surface", layout="hwc", color="nv12", buf=buf, views=[(0, (H * 3 // 2, W), (W, 1))]))
    return forms


def _device_frames(forms):
    out = []
    for f in forms:
        (off, shape, strides), = f["views"]
        out.append(torch.from_numpy(f["buf"].copy()).cuda().reshape(shape))
    return out


@pytest.mark.parametrize("kind", ["bgr", "nv12"])
def test_run_batch_draw_tracks(kind, monkeypatch):
    from centerpose_amd import detector, reid, track
    L, det = _L(), _det()
    H, W = 64, 96
    ex = reid.ReidExtractor(_sd(), capacity=8)
    trk, twin = track.DeepSortTracker(8, streams=2, n_init=1), track.DeepSortTracker(8, streams=2, n_init=1)
    forms = _host_frames(kind, H, W)
    kw = dict(color=kind)
    st, ts = detector.DrawStyle(), detector.TrackStyle()
    labels = matched = 0
    for call in range(3):
        plain = _device_frames(forms)
        want_rows, want_res, want_tracks = det.run_batch(plain, return_device=True, embed=ex, track=twin, **kw)
        want_feats, want_slots = want_res.features.clone(), want_res.slots.clone()
        assert all(np.array_equal(p.cpu().numpy().reshape(-1), f["buf"]) for p, f in zip(plain, forms))      # draw=False paints nothing
        drawn = _device_frames(forms)
        calls = []
        real_cpu = torch.Tensor.cpu
        with monkeypatch.context() as m:
            m.setattr(torch.Tensor, "cpu", lambda self, *a, **k: calls.append("cpu") or real_cpu(self, *a, **k))
            m.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.append("synchronize"))
            m.setattr(torch.cuda.Stream, "synchronize", lambda *a, **k: calls.append("stream.synchronize"))
            rows, res, tracks = det.run_batch(drawn, return_device=True, embed=ex, track=trk, draw="tracks", **kw)
        assert calls == ["cpu"]                                                # the tracker's own download and nothing else
        assert torch.equal(rows, want_rows) and torch.equal(res.features, want_feats) and torch.equal(res.slots, want_slots)
        assert len(tracks) == 2 and all(a.dtype == np.int64 and np.array_equal(a, b) for a, b in zip(tracks, want_tracks))
        assert np.array_equal(trk.assignments, twin.assignments)
        # the picture: the host painters and the NumPy painter fed the downloaded rows, ids and tracks
        M = int(rows.shape[1])
        ids = trk.row_ids(res, M).cpu().numpy()
        slots = res.slots.cpu().numpy()
        want_ids = np.full(2 * M, -1, np.int32)
        for j, v in enumerate(slots):
            if v >= 0 and trk.assignments.reshape(-1)[j] >= 0:
                want_ids[v] = trk.assignments.reshape(-1)[j]
        assert np.array_equal(ids.reshape(-1), want_ids)
        rows_h = rows.cpu().numpy()
        per_frame = [[tref.item(int(t[0]), int(t[1]), int(t[2]), int(t[3]), "ID %d" % t[4], detector.TRACK_PALETTE[int(t[4]) % 24], (255, 255, 255))
                      for t in tr] for tr in tracks]
        host = tu.host_paint_rows_ids(L, forms, rows_h, ids, detector.TRACK_PALETTE, 0.0, st.box_thickness, st.limb_radius, st.joint_radius,
                                      st.palette())
        host = tu.host_paint_tracks(L, forms, per_frame, ts.box_thickness, ts.font_scale, bufs=host)
        for n in range(2):
            ref = tref.reference_rows(forms[n], rows_h[n], 0.0, st.box_thickness, st.limb_radius, st.joint_radius, st.palette(), ids[n],
                                      detector.TRACK_PALETTE)
            ref = tref.reference(forms[n], per_frame[n], ts.box_thickness, ts.font_scale, buf=ref)
            got = drawn[n].cpu().numpy().reshape(-1)
            assert np.array_equal(host[n], ref), (call, n)
            assert np.array_equal(got, ref), (call, n, np.nonzero(got != ref)[0][:8])
            assert not np.array_equal(got, forms[n]["buf"])
        labels += sum(len(t) for t in tracks)
        matched += int((ids >= 0).sum())
        if call == 0:
            assert matched == 0 and labels == 0                                # the first call starts tracks: nothing is matched yet
    assert labels > 0 and matched > 0                                          # later calls painted identities and labels
    # the list form returns what it returns without draw, and paints the same picture as the device form would
    listed = det.run_batch(_device_frames(forms), embed=ex, track=trk, draw="tracks", **kw)
    assert listed[0] == det.run_batch(_device_frames(forms), **kw) and len(listed) == 3
