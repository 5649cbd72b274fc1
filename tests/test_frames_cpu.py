"""CPU: the host side of device-resident frames -- the descriptor struct and the new C-ABI symbols, the pure function that turns a
tensor's shape and strides into the addressing rule of cp_frame_desc (base + y * row_stride + x * pix_stride + ch_off[k]), the
descriptor table built from it, and the input validation that needs no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import prepost_np as pp

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


def test_frame_desc_size_and_symbols():
    L = _lib_built()
    from centerpose_amd import detector
    assert L.cp_sizeof_frame_desc() == detector.FRAME_DESC.itemsize == 128
    hdr = open(os.path.join(ROOT, "include", "centerpose_hip.h")).read()
    for sym in ("cp_sizeof_frame_desc", "cp_preprocess_frames_u8_f32"):
        assert re.search(r"\b%s\s*\(" % sym, hdr) and hasattr(L, sym)
    assert L.cp_abi_version() == 4
    # the header's struct declares the fields in the binder's order
    body = re.search(r"typedef struct cp_frame_desc \{(.*?)\} cp_frame_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"[\[\]\d\*\s]", "", f) for decl in re.findall(r"(?:const unsigned char\*|long long|int|double) ([^;]+);", body)
              for f in decl.split(",")]
    assert fields == list(detector.FRAME_DESC.names)


def _desc(**kw):
    from centerpose_amd import detector
    t = np.zeros(1, detector.FRAME_DESC)
    d = t[0]
    d["base"], d["row_stride"], d["pix_stride"], d["ch_off"], d["mid_off"] = 4096, 24, 3, (0, 1, 2), -1
    d["H"], d["W"], d["NH"], d["NW"], d["mi"], d["slot"] = 4, 8, 4, 8, (1, 0, 0, 0, 1, 0), 0
    for k, v in kw.items():
        d[k] = v
    return t


def _call(L, table, N=1, scratch=None, scratch_bytes=0, out=4096, out_batch=1, flip=0):
    """cp_preprocess_frames_u8_f32 with addresses that are never dereferenced: only calls whose argument check fails are made here."""
    mean = (ctypes.c_float * 3)(0.4, 0.4, 0.4)
    std = (ctypes.c_float * 3)(0.3, 0.3, 0.3)
    return L.cp_preprocess_frames_u8_f32(ctypes.c_void_p(4096), table.ctypes.data_as(ctypes.c_void_p), N, ctypes.c_void_p(scratch),
                                         ctypes.c_size_t(scratch_bytes), ctypes.c_void_p(out), out_batch, 8, 8, mean, std, flip, None)


@pytest.mark.parametrize("fields,message", [
    (dict(base=0), b"null base"),
    (dict(row_stride=-24), b"negative"),
    (dict(pix_stride=-1), b"negative"),
    (dict(ch_off=(0, -1, 2)), b"negative"),
    (dict(H=0), b"bad size"),
    (dict(H=1 << 15, W=1 << 14, NH=1 << 15, NW=1 << 14), b"bad size"),            # 2^29 pixels
    (dict(row_stride=1 << 61), b"2^62"),                                         # 3 * 2^61 >= 2^62
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
    assert _call(L, _desc(), flip=1) == 1 and b"output slot" in L.cp_last_error()          # the twin needs slot + 1


# the six forms of the bit-exactness test, as CPU tensors: (tensor view, layout, color) -> hand-written (H, W, row, pix, ch_off, offset)
def _forms():
    H, W = 37, 53
    big = torch.zeros((64, 80, 3), dtype=torch.uint8)
    clip = torch.zeros((4, H, W, 3), dtype=torch.uint8)
    return [
        ("contiguous bgr", torch.zeros((H, W, 3), dtype=torch.uint8), "hwc", "bgr", (H, W, 3 * W, 3, (0, 1, 2)), 0),
        ("crop view", big[5:42, 7:60], "hwc", "bgr", (H, W, 3 * 80, 3, (0, 1, 2)), (5 * 80 + 7) * 3),
        ("bgra", torch.zeros((H, W, 4), dtype=torch.uint8), "hwc", "bgr", (H, W, 4 * W, 4, (0, 1, 2)), 0),
        ("planar rgb", torch.zeros((3, H, W), dtype=torch.uint8), "chw", "rgb", (H, W, W, 1, (2 * H * W, H * W, 0)), 0),
        ("clip frame 2", clip.unbind(0)[2], "hwc", "bgr", (H, W, 3 * W, 3, (0, 1, 2)), 2 * H * W * 3),
        ("expanded along W", torch.zeros((H, 1, 3), dtype=torch.uint8).expand(H, W, 3), "hwc", "bgr", (H, W, 3, 0, (0, 1, 2)), 0),
    ]


@pytest.mark.parametrize("n", range(6))
def test_frame_geometry_of_the_six_forms(n):
    from centerpose_amd import detector
    name, t, layout, color, want, offset = _forms()[n]
    assert detector.frame_geometry(t.shape, t.stride(), layout, color) == want, name
    assert t.storage_offset() == offset, name
    # the rule itself: a marked byte is found where the rule says channel k of pixel (y, x) lies
    if 0 not in t.stride():
        H, W, row, pix, ch = want
        flat = torch.zeros(t.untyped_storage().nbytes(), dtype=torch.uint8)
        for k, (y, x) in enumerate(((0, 0), (H - 1, W - 1), (11, 17))):
            flat[offset + y * row + x * pix + ch[k]] = 100 + k
        view = torch.as_strided(flat, t.shape, t.stride(), offset)
        hwc = view if layout == "hwc" else view.permute(1, 2, 0)
        if color == "rgb":
            hwc = hwc.flip(2) if hwc.shape[2] == 3 else torch.cat([hwc[..., :3].flip(2), hwc[..., 3:]], 2)
        for k, (y, x) in enumerate(((0, 0), (H - 1, W - 1), (11, 17))):
            assert int(hwc[y, x, k]) == 100 + k, (name, k)


def test_frame_geometry_more_forms_and_refusals():
    from centerpose_amd import detector
    from centerpose_amd._lib import CenterposeHipError
    g = detector.frame_geometry
    assert g((9, 5, 4), (20, 4, 1), "hwc", "rgb") == (9, 5, 20, 4, (2, 1, 0))            # RGBA
    assert g((4, 9, 5), (64, 6, 1), "chw", "bgr") == (9, 5, 6, 1, (0, 64, 128))          # planar BGRA, padded rows
    assert g((9, 5, 3), (0, 0, 0)) == (9, 5, 0, 0, (0, 0, 0))                            # one pixel expanded to a frame
    for bad in (dict(layout="nhwc"), dict(color="yuv")):
        with pytest.raises(CenterposeHipError, match="unknown"):
            g((9, 5, 3), (15, 3, 1), **bad)
    with pytest.raises(CenterposeHipError, match="3 or 4 channels"):
        g((9, 5, 2), (10, 2, 1))
    with pytest.raises(CenterposeHipError, match="3 or 4 channels"):
        g((9, 5, 3), (15, 3, 1), "chw")                                                  # [9,5,3] read as CHW has 9 channels
    with pytest.raises(CenterposeHipError, match="3-D"):
        g((2, 9, 5, 3), (135, 15, 3, 1))
    with pytest.raises(CenterposeHipError, match="no pixels"):
        g((0, 5, 3), (15, 3, 1))


def test_frame_table_addresses_the_frames_in_place():
    """The FRAME_DESC table of a mixed list: base / strides / ch_off are the frames' own, the geometry, matrix and scratch layout are
    those of the staging table for the same sizes."""
    _lib_built()                                               # cp_invert_warp is host code of the library
    from centerpose_amd import detector
    det = _detector("res_50")
    assert det.cfg.TEST.FIX_RES and det.cfg.TEST.FLIP_TEST
    forms = _forms()
    frames = [(1000 * (n + 1),) + detector.frame_geometry(t.shape, t.stride(), layout, color) for n, (_, t, layout, color, _, _) in enumerate(forms)]
    shapes = [f[1:3] for f in frames]
    idx = list(range(len(frames)))
    for scale in (1, 0.5):
        table, scratch, inp_h, inp_w, metas = det._pre_table(shapes, None, idx, scale, frames)
        ref, rscratch, rh, rw, rmetas = det._pre_table(shapes, [0] * len(idx), idx, scale)
        assert table.dtype == detector.FRAME_DESC and ref.dtype == detector.PRE_DESC
        assert (scratch, inp_h, inp_w) == (rscratch, rh, rw) and len(metas) == len(rmetas) == len(idx)
        for name in ("mid_off", "H", "W", "NH", "NW", "mi", "slot"):
            assert np.array_equal(table[name], ref[name]), name
        for n, (_, _, _, _, want, _) in enumerate(forms):
            d = table[n]
            assert (int(d["base"]), int(d["row_stride"]), int(d["pix_stride"]), tuple(int(v) for v in d["ch_off"])) == (1000 * (n + 1),) + want[2:]
            _, rmeta = pp.pre_process(np.zeros(shapes[n] + (3,), np.uint8), scale, det.cfg.DATASET.MEAN, det.cfg.DATASET.STD,
                                      fix_res=True, flip_test=True)
            assert all(np.array_equal(np.asarray(metas[n][k]), np.asarray(rmeta[k])) for k in rmeta)


def test_cpu_tensor_raises_and_names_the_device():
    from centerpose_amd._lib import CenterposeHipError
    det = _detector()
    t = torch.zeros((8, 8, 3), dtype=torch.uint8)
    for call in (lambda: det.pre_process(t, 1), lambda: det.pre_process_batch([t], 1), lambda: det.run_batch([t]),
                 lambda: det.run_batch(torch.zeros((2, 8, 8, 3), dtype=torch.uint8)), lambda: det.run(t)):
        with pytest.raises(CenterposeHipError, match="cpu"):
            call()


def test_numpy_input_takes_the_default_layout_only():
    from centerpose_amd._lib import CenterposeHipError
    det = _detector()
    im = np.zeros((8, 8, 3), np.uint8)
    for kw in (dict(layout="chw"), dict(color="rgb")):
        with pytest.raises(CenterposeHipError, match="device"):
            det.run_batch([im], **kw)
        with pytest.raises(CenterposeHipError, match="device"):
            det.pre_process_batch([im], 1, **kw)
        with pytest.raises(CenterposeHipError, match="device"):
            det.pre_process(im, 1, **kw)
    with pytest.raises(CenterposeHipError, match="unknown layout"):
        det.run_batch([im], layout="nchw")
    with pytest.raises(CenterposeHipError, match="unknown color"):
        det.pre_process(im, 1, color="gray")


def test_mixed_wrong_rank_and_empty_input():
    from centerpose_amd._lib import CenterposeHipError
    det = _detector()
    t = torch.zeros((8, 8, 3), dtype=torch.uint8)
    with pytest.raises(CenterposeHipError, match="mixed"):
        det.run_batch([np.zeros((8, 8, 3), np.uint8), t])
    with pytest.raises(CenterposeHipError, match="4-D"):
        det.run_batch(t)                                       # one 3-D tensor is not a batch
    with pytest.raises(CenterposeHipError, match="3-D"):
        det.pre_process(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), 1)
    assert det.run_batch([]) == [] and det.run_batch([], layout="chw", color="rgb") == []
