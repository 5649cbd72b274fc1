"""GPU: draw_results (csrc/draw_results.hip) through MultiPoseDetector.draw_results and run_batch(draw=True).  Every comparison is of
whole buffers, byte for byte: device result == host painter (cp_draw_rows_*_host) == the NumPy painter of tests/draw_ref.py, so the
guard bytes, the padding and a fourth channel are compared with everything else."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import draw_ref
import draw_util

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _det():
    """A dla_34 with random weights whose default threshold lets every detection through (a sigmoid score is > 0)."""
    from centerpose_amd import config, detector
    return detector.MultiPoseDetector(config.get_cfg("dla_34", TEST__VIS_THRESH=0.0))


def _style(T, RL, RJ, pal):
    from centerpose_amd import detector
    return detector.DrawStyle(T, RL, RJ, box_color=pal[0], limb_colors=pal[1:19], joint_colors=pal[19:])


def _on_device(form):
    """The form's buffer on the device and its frame as the detector takes it: a tensor view, or a tuple of plane views."""
    dev = torch.from_numpy(form["buf"].copy()).cuda()
    views = [torch.as_strided(dev, shape, strides, off) for off, shape, strides in form["views"]]
    return dev, (views[0] if len(views) == 1 else tuple(views))


def _draw(forms, rows, T, RL, RJ, pal, matrix="bt601", vis=draw_ref.VIS):
    """det.draw_results of the forms (one layout / colour) with rows [N,M,56] -> the buffers back on the host."""
    devs, frames = zip(*[_on_device(f) for f in forms])
    rows = torch.from_numpy(np.ascontiguousarray(rows, np.float32).reshape(len(forms), -1, 56)).cuda()
    kw = dict(matrix=matrix) if forms[0]["color"] not in ("bgr", "rgb") else {}
    out = _det().draw_results(list(frames), rows, forms[0]["layout"], forms[0]["color"], vis_thresh=vis, style=_style(T, RL, RJ, pal), **kw)
    assert isinstance(out, list) and all(a is b for a, b in zip(out, frames))
    return [d.cpu().numpy() for d in devs]


def _forms(kind, seed, H, W):
    return (draw_ref.bgr_forms if kind == "bgr" else draw_ref.yuv_forms)(seed, H, W)


# ---------------------------------------------------------------- 1. the fuzz cases of the CPU test
@pytest.mark.parametrize("kind", ["bgr", "yuv"])
@pytest.mark.parametrize("s", range(len(draw_ref.SIZES)))
def test_device_equals_host_painter_equals_numpy(kind, s):
    L = draw_util.lib_loaded()
    H, W = draw_ref.SIZES[s]
    painted = 0
    for f, form in enumerate(_forms(kind, 100 * s + 10, H, W)):
        for trial in range(3):
            seed = 1000 * s + 10 * f + trial + (500 if kind == "yuv" else 0)
            rows = draw_ref.fuzz_rows(seed, 12, H, W)
            T, RL, RJ, pal = draw_ref.fuzz_style(seed)
            matrix = "bt709" if trial == 2 else "bt601"
            want = draw_ref.reference(form, rows, draw_ref.VIS, T, RL, RJ, pal, matrix)
            host, = draw_util.host_paint(L, [form], rows, draw_ref.VIS, T, RL, RJ, pal, matrix)
            got, = _draw([form], rows, T, RL, RJ, pal, matrix)
            assert np.array_equal(host, want), (form["name"], seed)
            assert np.array_equal(got, want), (form["name"], seed, np.nonzero(got != want)[0][:8])
            G = draw_ref.GUARD
            assert np.array_equal(got[:G], form["buf"][:G]) and np.array_equal(got[-G:], form["buf"][-G:])
            painted += int((want != form["buf"]).sum())
    assert painted > 0
    assert L.cp_last_kernel() == (b"draw_raster_kernel<bgr>" if kind == "bgr" else b"draw_raster_kernel<yuv>")


# ---------------------------------------------------------------- 2. mixed sizes and plane forms in one launch
@pytest.mark.parametrize("kind", ["bgr", "yuv"])
def test_mixed_sizes_in_one_launch_each_frame_its_own_rows(kind):
    L = draw_util.lib_loaded()
    sizes = [(1, 1), (37, 53), (64, 64)]
    pick = [0, 2, 0] if kind == "bgr" else [0, 0, 4]           # packed / bgra with padded rows / packed; planes / planes / a pitched surface
    forms = [_forms(kind, 300 + 10 * n, H, W)[p] for n, ((H, W), p) in enumerate(zip(sizes, pick))]
    assert len({(f["layout"], f["color"]) for f in forms}) == 1
    rows = np.stack([draw_ref.fuzz_rows(900 + n, 20, H, W) for n, (H, W) in enumerate(sizes)])
    rows[0, :, 4] = 1.0
    rows[0, :, 0:4] = (0, 0, 0, 0)                              # the 1 x 1 frame is painted for sure
    T, RL, RJ, pal = draw_ref.fuzz_style(9)
    want = [draw_ref.reference(f, rows[n], draw_ref.VIS, T, RL, RJ, pal) for n, f in enumerate(forms)]
    host = draw_util.host_paint(L, forms, rows, draw_ref.VIS, T, RL, RJ, pal)
    got = _draw(forms, rows, T, RL, RJ, pal)
    for n in range(3):
        assert np.array_equal(host[n], want[n]) and np.array_equal(got[n], want[n]), n
        assert (want[n] != forms[n]["buf"]).any(), n
    # a frame painted with another frame's rows looks different: the rows were not mixed up
    assert not np.array_equal(want[1], draw_ref.reference(forms[1], rows[2], draw_ref.VIS, T, RL, RJ, pal))


# ---------------------------------------------------------------- 3. more rows than one chunk of the rasteriser, all live
@pytest.mark.parametrize("kind", ["bgr", "yuv"])
def test_dense_300_rows(kind):
    form = _forms(kind, 77, 16, 16)[2]
    rows = draw_ref.fuzz_rows(4242, 300, 16, 16, dense=True)
    T, RL, RJ, pal = draw_ref.fuzz_style(3)
    want = draw_ref.reference(form, rows, draw_ref.VIS, T, RL, RJ, pal)
    got, = _draw([form], rows, T, RL, RJ, pal)
    assert np.array_equal(got, want)
    # the late rows dead but two: the winners come from both chunks of 256 rows
    rows[258:, 4] = 0.0
    win = draw_ref.winners(rows, 16, 16, draw_ref.VIS, T, RL, RJ) // 36
    assert (win >= 256).any() and ((win >= 0) & (win < 256)).any()
    want = draw_ref.reference(form, rows, draw_ref.VIS, T, RL, RJ, pal)
    got, = _draw([form], rows, T, RL, RJ, pal)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- 4. nothing to paint; two calls in a row
def test_no_frames_and_no_rows():
    det = _det()
    assert det.draw_results([], torch.zeros((0, 5, 56), device="cuda")) == []
    form = draw_ref.bgr_forms(5, 7, 5)[0]
    dev, frame = _on_device(form)
    assert det.draw_results([frame], torch.zeros((1, 0, 56), device="cuda"))[0] is frame
    dead = torch.zeros((1, 4, 56), device="cuda")              # scores of 0 under the default threshold of this detector: 0 > 0 is false
    det.draw_results([frame], dead)
    det.draw_results(frame.unsqueeze(0), dead[0])              # one 4-D tensor, rows [M,56] for its one frame
    assert np.array_equal(dev.cpu().numpy(), form["buf"])


@pytest.mark.parametrize("kind", ["bgr", "yuv"])
def test_two_calls_equal_one_painter_over_both_row_sets(kind):
    det = _det()
    form = _forms(kind, 41, 37, 53)[1]
    a, b = draw_ref.fuzz_rows(71, 12, 37, 53, dense=True), draw_ref.fuzz_rows(72, 12, 37, 53, dense=True)
    T, RL, RJ, pal = draw_ref.fuzz_style(6)
    dev, frame = _on_device(form)
    for rows in (a, b):
        det.draw_results([frame], torch.from_numpy(rows).cuda(), form["layout"], form["color"], vis_thresh=draw_ref.VIS, style=_style(T, RL, RJ, pal))
    want = draw_ref.reference(form, np.concatenate([a, b]), draw_ref.VIS, T, RL, RJ, pal)
    assert np.array_equal(dev.cpu().numpy(), want)
    assert not np.array_equal(want, draw_ref.reference(form, np.concatenate([b, a]), draw_ref.VIS, T, RL, RJ, pal))


# ---------------------------------------------------------------- 5. refusals leave the frames alone
def test_python_refusals_paint_nothing():
    from centerpose_amd._lib import CenterposeHipError
    det = _det()
    base = torch.full((8, 8, 3), 7, dtype=torch.uint8, device="cuda")
    other = torch.full((8, 8, 3), 7, dtype=torch.uint8, device="cuda")
    y = torch.full((12, 8), 7, dtype=torch.uint8, device="cuda")
    rows = torch.zeros((1, 3, 56), device="cuda")
    rows[:, :, 0:5] = torch.tensor([1.0, 1.0, 6.0, 6.0, 1.0], device="cuda")
    two = torch.cat([rows, rows])
    cases = [("same byte", lambda: det.draw_results([torch.full((8, 1, 3), 7, dtype=torch.uint8, device="cuda").expand(8, 8, 3)], rows)),
             ("same byte", lambda: det.draw_results([torch.as_strided(base, (4, 4, 3), (6, 3, 1))], rows)),
             ("same byte", lambda: det.draw_results(base.unsqueeze(0).expand(2, 8, 8, 3), two)),
             ("given twice", lambda: det.draw_results([base, base], two)),
             ("given twice", lambda: det.run_batch([base, base], draw=True)),
             ("share bytes", lambda: det.draw_results([(y[:8], y[4:8].unflatten(1, (4, 2)))], rows, color="nv12")),
             ("host arrays", lambda: det.draw_results([np.zeros((8, 8, 3), np.uint8)], rows)),
             ("host arrays", lambda: det.run_batch([np.zeros((96, 128, 3), np.uint8)], draw=True)),
             ("CUDA float32 tensor", lambda: det.draw_results([base], rows.cpu().numpy())),
             ("cpu", lambda: det.draw_results([base], rows.cpu())),
             ("float32", lambda: det.draw_results([base], rows.double())),
             ("56", lambda: det.draw_results([base], rows[:, :, :55])),
             ("56", lambda: det.draw_results([base], rows.unsqueeze(0))),
             ("2 blocks for 1 frames", lambda: det.draw_results([base], two)),
             ("1 blocks for 2 frames", lambda: det.draw_results([base, other], rows)),
             ("DrawStyle", lambda: det.draw_results([base], rows, style=dict(box_thickness=2))),
             ("unknown matrix", lambda: det.draw_results([(y[:8], y[8:].unflatten(1, (4, 2)))], rows, color="nv12", matrix="bt2020"))]
    for match, call in cases:
        with pytest.raises(CenterposeHipError, match=match):
            call()
    torch.cuda.synchronize()
    assert int(base.min()) == int(base.max()) == 7 and int(other.min()) == int(other.max()) == 7 and int(y.min()) == int(y.max()) == 7
    det.draw_results([base], rows, vis_thresh=0.5)             # ... and the accepted call does paint
    assert int(base[1, 1, 0]) != 7 and int(base[0, 0, 0]) == 7


@pytest.mark.parametrize("yuv", [False, True])
def test_bad_second_descriptor_through_ctypes_launches_nothing(yuv):
    from centerpose_amd import _lib
    L = draw_util.lib_loaded()
    forms = [_forms("yuv" if yuv else "bgr", 50 + n, 7, 5)[0] for n in range(2)]
    devs = [torch.from_numpy(f["buf"].copy()).cuda() for f in forms]
    table = draw_util.table_of(forms, [d.data_ptr() for d in devs])
    rows = np.zeros((2, 2, 56), np.float32)
    rows[:, :, 0:5] = (0, 0, 4, 6, 1.0)
    rows_dev = torch.from_numpy(rows).cuda()
    nbytes = L.cp_draw_scratch_bytes(2, 2)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = draw_util.style_struct(2, 1, 2, [(255, 255, 255)] * 36)
    fn = L.cp_draw_rows_yuv_frames_u8 if yuv else L.cp_draw_rows_frames_u8

    def call(n_bytes=nbytes):
        dev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).cuda()
        rc = fn(ctypes.c_void_p(dev.data_ptr()), table.ctypes.data_as(ctypes.c_void_p), 2, ctypes.c_void_p(rows_dev.data_ptr()), 2,
                ctypes.c_float(0.3), st.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(scratch.data_ptr()), ctypes.c_size_t(n_bytes), _lib.stream())
        torch.cuda.synchronize()
        return rc

    assert call(nbytes - 1) == 1 and b"cp_draw_scratch_bytes" in L.cp_last_error()
    good = table[1]["W"]
    table[1]["W"] = 0                                          # the SECOND descriptor is bad: the first must not have been painted either
    assert call() == 1 and b"bad size" in L.cp_last_error()
    assert all(np.array_equal(d.cpu().numpy(), f["buf"]) for d, f in zip(devs, forms))
    table[1]["W"] = good
    assert call() == 0
    assert all(not np.array_equal(d.cpu().numpy(), f["buf"]) for d, f in zip(devs, forms))


# ---------------------------------------------------------------- 6. run_batch(draw=True)
def _batch_frames(kind, sizes):
    """Fresh device frames of the given sizes from fixed host bytes: BGR (every second one BGRA) or NV12 (surfaces and plane tuples)."""
    frames = []
    for i, (h, w) in enumerate(sizes):
        r = np.random.RandomState(800 + i)
        if kind == "bgr":
            frames.append(torch.from_numpy(r.randint(0, 256, (h, w, 4 if i % 2 else 3)).astype(np.uint8)).cuda())
        elif i % 2:
            frames.append((torch.from_numpy(r.randint(0, 256, (h, w)).astype(np.uint8)).cuda(),
                           torch.from_numpy(r.randint(0, 256, (h // 2, w // 2, 2)).astype(np.uint8)).cuda()))
        else:
            frames.append(torch.from_numpy(r.randint(0, 256, (h * 3 // 2, w + 32)).astype(np.uint8)).cuda()[:, :w])      # a pitched surface
    return frames


def _same(a, b):
    return all(torch.equal(p, q) for x, y in zip(a, b) for p, q in zip(x if isinstance(x, tuple) else (x,), y if isinstance(y, tuple) else (y,)))


@pytest.mark.parametrize("kind", ["bgr", "nv12"])
def test_run_batch_draw(kind, monkeypatch):
    det = _det()
    sizes = [(96, 128), (200, 264), (96, 128)]
    assert len(det._batch_groups(sizes)) == 2
    kw = dict(color=kind)
    original = _batch_frames(kind, sizes)
    plain = _batch_frames(kind, sizes)
    rows = det.run_batch(plain, return_device=True, **kw)
    listed = det.run_batch(plain, **kw)
    assert _same(plain, original)
    assert bool((rows[:, :, 4] > 0).any(1).all())              # every frame has live rows under this detector's threshold

    drawn = _batch_frames(kind, sizes)
    forbidden = []
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "cpu", lambda self, *a, **k: forbidden.append("cpu") or self)
        m.setattr(torch.cuda, "synchronize", lambda *a, **k: forbidden.append("synchronize"))
        m.setattr(torch.cuda.Stream, "synchronize", lambda *a, **k: forbidden.append("stream.synchronize"))
        rows_drawn = det.run_batch(drawn, return_device=True, draw=True, **kw)
    assert forbidden == []
    assert torch.equal(rows_drawn, rows)                       # bit-equal: the painting comes after the frames were read
    assert all(not _same([d], [o]) for d, o in zip(drawn, original))       # every frame was painted

    by_hand = _batch_frames(kind, sizes)
    assert det.draw_results(by_hand, rows, **kw) is by_hand
    assert _same(drawn, by_hand)

    again = _batch_frames(kind, sizes)
    assert det.run_batch(again, draw=True, **kw) == listed     # the list form: same return value, same picture
    assert _same(again, drawn)

    if kind == "bgr":                                          # the small BGR frame against the NumPy painter as well
        from centerpose_amd import detector
        st = detector.DrawStyle()
        win = draw_ref.winners(rows[0].cpu().numpy(), 96, 128, 0.0, st.box_thickness, st.limb_radius, st.joint_radius)
        want = original[0].cpu().numpy().copy()
        draw_ref.paint_bgr(want, "hwc", "bgr", win, st.palette())
        assert np.array_equal(drawn[0].cpu().numpy(), want)
