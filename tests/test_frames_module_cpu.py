"""CPU: the device-frame layer as a module of its own (centerpose_amd/frames.py) -- what importing it and its users pulls in, the one
identity descriptor table against values written out by hand, `_pre_table` on top of the same rows, the rows check with every
caller's exact texts, and the names detector.py keeps handing out."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fresh(code):
    """`code` in a new interpreter started in the repository root -> its stdout."""
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout.split()


def test_importing_frames_pulls_in_none_of_its_users():
    out = _fresh("import sys, centerpose_amd.frames\n"
                 "print(*[m for m in ('detector', 'engine', 'reid', 'track', 'draw') if 'centerpose_amd.' + m in sys.modules])")
    assert out == []


def test_reid_and_track_define_no_detector_subclass():
    out = _fresh("import centerpose_amd.reid, centerpose_amd.track\n"
                 "from centerpose_amd.detector import BaseDetector\n"
                 "def subs(c):\n"
                 "    return [s for d in c.__subclasses__() for s in [d] + subs(d)]\n"
                 "print(*sorted(c.__name__ for c in subs(BaseDetector)))")
    assert out == ["MultiPoseDetector"]


def _two_frames():
    """(a 4 x 6 RGBA crop of a 10 x 12 image at 4096, a 4 x 6 NV12 surface with 8-byte rows at 8192), described as FrameIO would."""
    from centerpose_amd import frames
    crop = torch.zeros((10, 12, 4), dtype=torch.uint8)[3:7, 2:8]
    packed = frames.Frame(4096 + crop.storage_offset(), *frames.frame_geometry(crop.shape, crop.stride(), "hwc", "rgb"))
    surface = torch.zeros((6, 8), dtype=torch.uint8)[:, :6]
    H, W, y_row, y_pix, u_off, v_off, c_row, c_pix = frames.yuv_frame_geometry([surface.shape], [surface.stride()], "nv12")
    return packed, frames.YuvFrame(8192, H, W, y_row, y_pix, 8192 + u_off, 8192 + v_off, c_row, c_pix)


def test_identity_table_field_by_field():
    from centerpose_amd import frames
    packed, planes = _two_frames()
    assert (packed.H, packed.W, packed.ch_off) == (4, 6, (2, 1, 0)) and packed[1:3] == (4, 6) and len(packed) == 6 and len(planes) == 9
    t = frames.identity_table([packed], False)
    assert t.dtype == frames.FRAME_DESC and t.shape == (1,) and t.flags["C_CONTIGUOUS"]
    want = dict(base=4096 + (3 * 12 + 2) * 4, row_stride=48, pix_stride=4, ch_off=[2, 1, 0], mid_off=-1, H=4, W=6, NH=4, NW=6, mi=[0.0] * 6,
                slot=0, pad=0)
    assert set(want) == set(t.dtype.names)
    for name, v in want.items():
        assert t[name][0].tolist() == v, name
    t = frames.identity_table([planes, planes], True)
    assert t.dtype == frames.YUV_FRAME_DESC and t.shape == (2,) and t.flags["C_CONTIGUOUS"]
    want = dict(y_base=8192, y_row=8, y_pix=1, u_base=8192 + 32, v_base=8192 + 33, c_row=8, c_pix=2, mid_off=-1, H=4, W=6, NH=4, NW=6,
                mi=[0.0] * 6, slot=0, pad=0)
    assert set(want) == set(t.dtype.names)
    for name, v in want.items():
        assert t[name][0].tolist() == v and t[name][1].tolist() == v, name
    # plain tuples in the same order (what the CPU tests build by hand) give the same rows; no frames, no rows
    assert frames.identity_table([tuple(packed)], False).tobytes() == frames.identity_table([packed], False).tobytes()
    assert frames.identity_table([], True).shape == (0,)


def test_pre_table_fills_its_addresses_through_the_identity_table():
    import __graft_entry__ as g
    g.build()                                              # cp_invert_warp is host code of the library
    from centerpose_amd import config, detector, frames
    det = object.__new__(detector.MultiPoseDetector)
    det.cfg = config.get_cfg("res_50")
    assert det.cfg.TEST.FIX_RES
    for yuv, f in enumerate(_two_frames()):
        ident = frames.identity_table([f, f], bool(yuv))
        table, scratch, _, _, _ = det._pre_table([(4, 6)] * 2, None, [1, 0], 0.5, [f, f], bool(yuv))
        assert table.dtype == ident.dtype and scratch == 2 * 2 * 3 * 3
        assert table["NH"].tolist() == [2, 2] and table["NW"].tolist() == [3, 3] and table["mid_off"].tolist() == [0, 18]
        assert table["slot"].tolist() == [0, 2] and table["mi"].any()
        address = ("y_base", "y_row", "y_pix", "u_base", "v_base", "c_row", "c_pix") if yuv else ("base", "row_stride", "pix_stride", "ch_off")
        for name in address + ("H", "W"):
            assert np.array_equal(table[name], ident[name]), name


class _OnGpu(torch.Tensor):
    """A host tensor that says it lies on cuda:0: the checks below stop before anything would read it."""
    is_cuda, device = True, torch.device("cuda", 0)


def _on_gpu(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype).as_subclass(_OnGpu)


def _callers():
    """(name, call(rows) with two frames / streams expected on cuda:0, error type of a wrong block count) for the three users."""
    from centerpose_amd import detector, frames, reid, track
    det = object.__new__(detector.MultiPoseDetector)
    det.model = type("Model", (), {"device": "cuda:0"})()
    ext = object.__new__(reid.ReidExtractor)
    ext.device = torch.device("cuda", 0)
    ext._io = frames.FrameIO(ext.device)
    trk = track.DeepSortTracker(4, streams=2, device=None)
    trk.device = torch.device("cuda", 0)
    res = reid.ReidResult(_on_gpu(4, 512), _on_gpu(4, dtype=torch.int32), _on_gpu(2, dtype=torch.int32))
    # two frames that fail in FrameIO.frame would hide the rows check: draw and embed get rows for the empty list, i.e. 0 frames
    return [("draw", lambda rows: det.draw_results([], rows), 0), ("reid", lambda rows: ext.embed([], rows), 0),
            ("track", lambda rows: trk._check(rows, res, [(64, 48)] * 2), 2)]


def test_rows_check_gives_every_caller_its_own_texts():
    from centerpose_amd._lib import CenterposeHipError
    plan, gallery = "the re-id plan is on cuda:0; there is no CPU fallback", "the gallery is on cuda:0; there is no CPU fallback"
    full = "rows must be a CUDA float32 tensor [N, M, 56] on the device (got ndarray): there is no CPU fallback"
    cases = {
        "numpy": (lambda n: np.zeros((n, 3, 56), np.float32),
                  dict(draw=full, reid=full, track="rows must be a CUDA tensor on the device (got ndarray): there is no CPU fallback")),
        "rank": (lambda n: _on_gpu(n, 3, 56, 1),
                 dict(draw="rows must be [N, M, 56] (or [M, 56] for one frame), got shape (%d, 3, 56, 1)",
                      reid="rows must be [N, M, 56] (or [M, 56] for one frame), got shape (%d, 3, 56, 1)",
                      track="rows must be [N, M, 56] (or [M, 56] for one stream), got shape (%d, 3, 56, 1)")),
        "not 56": (lambda n: _on_gpu(n, 3, 55),
                   dict(draw="rows must be [N, M, 56] (or [M, 56] for one frame), got shape (%d, 3, 55)",
                        reid="rows must be [N, M, 56] (or [M, 56] for one frame), got shape (%d, 3, 55)",
                        track="rows must be [N, M, 56] (or [M, 56] for one stream), got shape (%d, 3, 55)")),
        "float64": (lambda n: _on_gpu(n, 3, 56, dtype=torch.float64),
                    dict(draw="rows must be float32 (got torch.float64)", reid="rows must be float32 (got torch.float64)",
                         track="rows must be torch.float32 (got torch.float64)")),
        "cpu": (lambda n: torch.zeros((n, 3, 56)),
                dict(draw="rows on cpu: they must be on the model's GPU; there is no CPU fallback", reid="rows on cpu, " + plan,
                     track="rows on cpu, " + gallery)),
        "other gpu": (lambda n: _other_gpu(n),
                      dict(draw="rows on cuda:1, the model is on cuda:0", reid="rows on cuda:1, " + plan, track="rows on cuda:1, " + gallery)),
    }
    for what, (make, texts) in cases.items():
        for name, call, n in _callers():
            with pytest.raises(CenterposeHipError) as e:
                call(make(n))
            want = texts[name]
            assert str(e.value) == (want % n if "%d" in want else want), (what, name)
    # a block count other than the frame count: the tracker's is a ValueError with its own text
    for name, call, n in _callers():
        with pytest.raises(ValueError if name == "track" else CenterposeHipError) as e:
            call(_on_gpu(n + 1, 3, 56))
        assert str(e.value) == ("rows hold 3 frames, the tracker has 2 streams: frame n of a call belongs to stream n" if name == "track" else
                                "rows hold 1 blocks for 0 frames"), name
        assert not (name != "track" and isinstance(e.value, ValueError))
    # [M, 56] is one block
    from centerpose_amd import frames
    assert tuple(frames.check_rows(_on_gpu(3, 56), 1, torch.device("cuda", 0), "the model is on %s").shape) == (1, 3, 56)


def _other_gpu(n):
    t = _on_gpu(n, 3, 56)
    t.device = torch.device("cuda", 1)
    return t


def test_detector_hands_out_the_same_objects():
    from centerpose_amd import detector, draw, frames
    for name in ("frame_geometry", "yuv_frame_geometry", "frame_writable", "byte_range", "PRE_DESC", "FRAME_DESC", "YUV_FRAME_DESC",
                 "YUV_MATRICES", "YUV_COLORS"):
        assert getattr(detector, name) is getattr(frames, name), name
    for name in ("DrawStyle", "palette_to_yuv", "DRAW_STYLE", "DRAW_LIMBS", "DRAW_LEFT", "DRAW_RIGHT", "DRAW_MID"):
        assert getattr(detector, name) is getattr(draw, name), name
