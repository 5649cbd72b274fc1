"""GPU: device frames in NV12 / NV21 / I420 (csrc/yuv_frames.hip) through pre_process / pre_process_batch / run / run_batch.  Every
comparison is bit for bit against oracle.prepost_np.pre_process of the HxWx3 BGR array that tests/yuv_ref.py converts the frame to, and
against the staging path on that array: every addressing mode under both store kernels, the second matrix, mixed sizes and plane forms
in one launch, the sources read in place and left alone, run_batch against run_batch of the converted host arrays, and the refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import yuv_ref
from oracle import prepost_np as pp

pytestmark = pytest.mark.gpu

SIZES = [(37, 53), (64, 80), (2, 2), (1, 9), (9, 1)]
FIX = dict(TEST__FIX_RES=True, MODEL__INPUT_H=48, MODEL__INPUT_W=64)
GEOMETRIES = {"vec4": (FIX, b"preprocess_yuv_frames_kernel<vec4>"),
              "scalar": (dict(TEST__FIX_RES=True, MODEL__INPUT_H=48, MODEL__INPUT_W=62), b"preprocess_yuv_frames_kernel<scalar>"),
              "padded": (dict(TEST__FIX_RES=False), b"preprocess_yuv_frames_kernel<vec4>")}


def _scales(h, w):
    return (1, 2) if min(h, w) == 1 else (1, 0.5, 2)           # a one-pixel side has no pixels at 0.5


def _bytes(seed, *shape):
    return (np.random.RandomState(seed).rand(*shape) * 256).astype(np.uint8)


def _planes(seed, h, w):
    """Random host planes of one frame: y [h,w], u and v [ceil(h/2),ceil(w/2)]."""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return _bytes(seed, h, w), _bytes(seed + 1, ch, cw), _bytes(seed + 2, ch, cw)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _cached_det(arch, over):
    from centerpose_amd import config, detector
    return detector.MultiPoseDetector(config.get_cfg(arch, **dict(over)))


def _det(arch="dla_34", **over):
    return _cached_det(arch, tuple(sorted(over.items())))


def _last_kernel():
    from centerpose_amd import _lib
    return _lib.lib().cp_last_kernel()


_ORACLE = {}


def _oracle(det, host, scale):
    """oracle.prepost_np.pre_process of a host HxWx3 BGR array under det's configuration, computed once per (array, scale, config)."""
    cfg = det.cfg
    key = (host.tobytes(), host.shape, scale, cfg.TEST.FIX_RES, cfg.TEST.FLIP_TEST, cfg.MODEL.INPUT_H, cfg.MODEL.INPUT_W)
    if key not in _ORACLE:
        _ORACLE[key] = pp.pre_process(host, scale, cfg.DATASET.MEAN, cfg.DATASET.STD, fix_res=cfg.TEST.FIX_RES, flip_test=cfg.TEST.FLIP_TEST,
                                      input_h=cfg.MODEL.INPUT_H, input_w=cfg.MODEL.INPUT_W, pad=cfg.MODEL.PAD, down_ratio=cfg.MODEL.DOWN_RATIO)
    return _ORACLE[key]


def _at_odd_address(a):
    """The host array as a contiguous device tensor whose first byte lies at an odd address."""
    storage = torch.zeros((a.size + 1,), dtype=torch.uint8, device="cuda")
    t = storage[1:].view(a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert t.data_ptr() % 2 == 1
    return t


def _surface(y, u, v, color, pitch):
    """The decoder's layout on the device: [h*3/2, w] with the given row pitch, luma rows, then interleaved chroma rows."""
    h, w = y.shape
    uv = np.stack([u, v] if color == "nv12" else [v, u], -1).reshape(h // 2, w)
    alloc = torch.from_numpy(_bytes(7, h * 3 // 2, pitch)).cuda()             # the padding holds random bytes, not zeros
    alloc[:, :w] = _cuda(np.concatenate([y, uv], 0))
    return alloc, alloc[:, :w]


def _forms(seed, h, w):
    """The addressing modes for one frame size: [(name, what is given to the detector, color, host planes as yuv_ref takes them)].
    All forms but the expanded one hold the same samples, so they share one converted BGR array and one oracle result."""
    y, u, v = _planes(seed, h, w)
    ch, cw = u.shape
    uv, vu = np.stack([u, v], -1), np.stack([v, u], -1)
    forms = [("nv12 planes", (_cuda(y), _cuda(uv)), "nv12", (y, uv)),
             ("nv21 planes", (_cuda(y), _cuda(vu)), "nv21", (y, vu)),
             ("i420 planes", (_cuda(y), _cuda(u), _cuda(v)), "i420", (y, u, v))]
    if h % 2 == 0 and w % 2 == 0:
        forms.append(("nv12 surface, pitch w + 48", _surface(y, u, v, "nv12", w + 48)[1], "nv12", (y, uv)))
        forms.append(("nv21 surface, odd pitch", _surface(y, u, v, "nv21", w + 47)[1], "nv21", (y, vu)))
    # an even-origin crop of a larger frame: y and uv views (and u, v views) with the samples pasted where the crop lies
    big_y, big_uv = _bytes(seed + 3, h + 22, w + 28), _bytes(seed + 4, ch + 11, cw + 14, 2)
    big_y[6:6 + h, 8:8 + w], big_uv[3:3 + ch, 4:4 + cw] = y, uv
    by, buv = _cuda(big_y), _cuda(big_uv)
    forms.append(("nv12 crop at (6, 8)", (by[6:6 + h, 8:8 + w], buv[3:3 + ch, 4:4 + cw]), "nv12", (y, uv)))
    forms.append(("i420 crop, planes as strided views of one uv plane", (by[6:6 + h, 8:8 + w], buv[3:3 + ch, 4:4 + cw, 0], buv[3:3 + ch, 4:4 + cw, 1]),
                  "i420", (y, u, v)))
    # planes at odd byte addresses: nothing may assume an aligned plane, an interleaved uv plane included
    forms.append(("i420 at odd addresses", (_at_odd_address(y), _at_odd_address(u), _at_odd_address(v)), "i420", (y, u, v)))
    forms.append(("nv12, y at an odd address", (_at_odd_address(y), _cuda(uv)), "nv12", (y, uv)))
    forms.append(("nv21, uv at an odd address", (_cuda(y), _at_odd_address(vu)), "nv21", (y, vu)))
    # one chroma pair for the whole frame: strides of 0
    pair = _bytes(seed + 5, 1, 1, 2)
    forms.append(("nv12, expanded chroma", (_cuda(y), _cuda(pair).expand(ch, cw, 2)), "nv12", (y, np.broadcast_to(pair, (ch, cw, 2)))))
    forms.append(("i420, expanded chroma", (_cuda(y), _cuda(pair[:, :, 0]).expand(ch, cw), _cuda(pair[:, :, 1]).expand(ch, cw)), "i420",
                  (y, np.broadcast_to(pair[:, :, 0], (ch, cw)), np.broadcast_to(pair[:, :, 1], (ch, cw)))))
    return forms


def _same_meta(a, b):
    return set(a) == set(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in b)


def _check_forms(det, forms, scale, kernel, matrix="bt601"):
    nb = 2 if det.cfg.TEST.FLIP_TEST else 1
    staged = {}
    for name, given, color, planes in forms:
        what = (name, tuple(planes[0].shape), scale)
        host = yuv_ref.frame_to_bgr(planes, color, matrix)
        x, metas = det.pre_process_batch([given], scale, color=color, matrix=matrix)
        assert _last_kernel() == kernel, what
        assert x.is_cuda and x.dtype == torch.float32 and x.shape[0] == nb and len(metas) == 1, what
        got = x.cpu().numpy()
        ref, rmeta = _oracle(det, host, scale)
        assert np.array_equal(got, ref), what
        key = host.tobytes()
        if key not in staged:
            s, smetas = det.pre_process_batch([host], scale)
            staged[key] = (s.cpu().numpy(), smetas[0])
        assert np.array_equal(got, staged[key][0]), what
        assert _same_meta(metas[0], rmeta) and _same_meta(metas[0], staged[key][1]), what


# ---------------------------------------------------------------- 1. every addressing mode, both store kernels, bit for bit
@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("geometry", ["vec4", "scalar", "padded"])
def test_every_addressing_mode_bit_exact(geometry, flip):
    over, kernel = GEOMETRIES[geometry]
    det = _det(TEST__FLIP_TEST=flip, **over)
    if geometry == "padded":
        assert det.input_geometry(37, 53, 1)[2:4] == (64, 64)
    for i, (h, w) in enumerate(SIZES):
        forms = _forms(100 + 10 * i, h, w)
        assert len(forms) == (12 if h % 2 == 0 and w % 2 == 0 else 10)
        for scale in _scales(h, w):
            _check_forms(det, forms, scale, kernel)


# ---------------------------------------------------------------- 2. the second matrix
def test_bt709_is_used_and_differs_from_bt601():
    det = _det(TEST__FLIP_TEST=True, **FIX)
    forms = _forms(200, 37, 53)[:3]
    for scale in (1, 0.5, 2):
        _check_forms(det, forms, scale, b"preprocess_yuv_frames_kernel<vec4>", matrix="bt709")
    _, given, color, planes = forms[0]
    assert not np.array_equal(yuv_ref.frame_to_bgr(planes, color, "bt709"), yuv_ref.frame_to_bgr(planes, color, "bt601"))
    a = det.pre_process_batch([given], 1, color=color, matrix="bt709")[0]
    b = det.pre_process_batch([given], 1, color=color)[0]
    assert not torch.equal(a, b)
    assert torch.equal(b, det.pre_process_batch([given], 1, color=color, matrix="bt601")[0])


# ---------------------------------------------------------------- 3. mixed sizes and plane forms in one launch
@pytest.mark.parametrize("flip", [True, False])
def test_mixed_sizes_and_forms_in_one_launch(flip):
    det = _det(TEST__FLIP_TEST=flip, **FIX)
    nb = 2 if flip else 1
    samples = [_planes(300, 37, 53), _planes(310, 64, 80), _planes(320, 1, 9)]
    uvs = [np.stack([u, v], -1) for _, u, v in samples]
    hosts = [yuv_ref.frame_to_bgr((s[0], uv), "nv12") for s, uv in zip(samples, uvs)]
    # one list, one color word per call: plane tensors, a pitched surface, planes at odd addresses
    frames = [(_cuda(samples[0][0]), _cuda(uvs[0])), _surface(*samples[1], "nv12", 128)[1], (_at_odd_address(samples[2][0]), _at_odd_address(uvs[2]))]
    assert frames[1].stride() == (128, 1) and tuple(frames[1].shape) == (96, 80)
    for scale in (0.5, 1, 2):
        n = 2 if scale == 0.5 else 3                         # (1,9) has no pixels at 0.5
        x, metas = det.pre_process_batch(frames[:n], scale, color="nv12")
        got = x.cpu().numpy()
        assert got.shape == (nb * n, 3, 48, 64)
        for k in range(n):
            ref, rmeta = _oracle(det, hosts[k], scale)
            assert np.array_equal(got[nb * k:nb * k + nb], ref), (scale, k)
            assert _same_meta(metas[k], rmeta)
        assert np.array_equal(got, det.pre_process_batch(hosts[:n], scale)[0].cpu().numpy()), scale
    # i420 frames of two sizes in one list, the first as a YV12 file lays them out: v before u in memory, passed as (y, u, v)
    yv12 = _cuda(np.concatenate([samples[0][2].reshape(-1), samples[0][1].reshape(-1)]))
    n_c = samples[0][1].size
    planar = [(_cuda(samples[0][0]), yv12[n_c:].view(19, 27), yv12[:n_c].view(19, 27)), tuple(_cuda(p) for p in samples[1])]
    got = det.pre_process_batch(planar, 2, color="i420")[0].cpu().numpy()
    for k in range(2):
        assert np.array_equal(got[nb * k:nb * k + nb], _oracle(det, hosts[k], 2)[0]), k
    from centerpose_amd._lib import CenterposeHipError
    with pytest.raises(CenterposeHipError, match="no pixels"):
        det.pre_process_batch(frames, 0.5, color="nv12")


# ---------------------------------------------------------------- 4. read in place, left alone
def test_sources_left_alone():
    det = _det(TEST__FLIP_TEST=True, **FIX)
    y, u, v = _planes(400, 64, 80)
    alloc, surface = _surface(y, u, v, "nv12", 128)
    cy, cu, cv = _planes(410, 37, 53)
    cuv = np.stack([cu, cv], -1)
    big_y, big_uv = _bytes(420, 64, 80), _bytes(421, 32, 40, 2)
    big_y[6:43, 8:61], big_uv[3:22, 4:31] = cy, cuv
    by, buv = _cuda(big_y), _cuda(big_uv)
    frames = [surface, (by[6:43, 8:61], buv[3:22, 4:31])]
    before = [alloc.clone(), by.clone(), buv.clone()]
    hosts = [yuv_ref.frame_to_bgr((y, np.stack([u, v], -1)), "nv12"), yuv_ref.frame_to_bgr((cy, cuv), "nv12")]
    for scale in (1, 0.5, 2):
        x, _ = det.pre_process_batch(frames, scale, color="nv12")
        got = x.cpu().numpy()
        for k in range(2):
            assert np.array_equal(got[2 * k:2 * k + 2], _oracle(det, hosts[k], scale)[0]), (scale, k)
    torch.cuda.synchronize()
    assert torch.equal(alloc, before[0])                                          # the pitch padding included
    assert torch.equal(by, before[1]) and torch.equal(buv, before[2])             # the crop's surroundings included
    assert frames[0].data_ptr() == alloc.data_ptr() and frames[1][0].data_ptr() == by.data_ptr() + 6 * 80 + 8
    assert frames[1][1].data_ptr() == buv.data_ptr() + (3 * 40 + 4) * 2


# ---------------------------------------------------------------- 5. pre_process / run of one frame; run_batch
def _nv12_surface_and_host(seed, h, w, pitch):
    y, u, v = _planes(seed, h, w)
    return _surface(y, u, v, "nv12", pitch)[1], (y, u, v), yuv_ref.frame_to_bgr((y, np.stack([u, v], -1)), "nv12")


def test_pre_process_and_run_of_one_frame():
    det = _det("dla_34")
    surface, (y, u, v), host = _nv12_surface_and_host(500, 96, 128, 256)
    i420 = (_cuda(y), _cuda(u), _cuda(v))
    want, wmeta = det.pre_process(host, 1)
    for frame, color in ((surface, "nv12"), ((surface[:96], surface[96:].unflatten(1, (64, 2))), "nv12"), (i420, "i420")):
        x, meta = det.pre_process(frame, 1, color=color)
        assert _last_kernel() == b"preprocess_yuv_frames_kernel<vec4>"
        assert torch.equal(x, want) and _same_meta(meta, wmeta)
    want = det.run(host)
    got = det.run(surface, color="nv12")
    assert got["results"] == want["results"] and set(got) == set(want)
    assert det.run(i420, color="i420", matrix="bt601")["results"] == want["results"]
    host709 = yuv_ref.frame_to_bgr((y, u, v), "i420", "bt709")
    assert det.run(list(i420), color="i420", matrix="bt709")["results"] == det.run(host709)["results"]


@pytest.mark.parametrize("arch,sizes,groups", [("dla_34", [(200, 264), (96, 128), (200, 264), (96, 128)], 2),
                                               ("hrnet", [(120, 160), (96, 128)], 2)])
def test_run_batch_yuv_frames_equal_converted_host_arrays(arch, sizes, groups):
    det = _det(arch)
    assert len(det._batch_groups(sizes)) == groups
    if arch == "hrnet":
        assert len(det.scales) == 2
    frames, hosts = [], []
    for i, (h, w) in enumerate(sizes):
        surface, (y, u, v), host = _nv12_surface_and_host(610 + 10 * i, h, w, w + 64)
        frames.append(surface if i % 2 == 0 else (_cuda(y), _cuda(np.stack([u, v], -1))))      # surfaces and plane tuples in one call
        hosts.append(host)
    want = det.run_batch(hosts)
    plans = len(det.model._engines)
    got = det.run_batch(frames, color="nv12")
    assert len(det.model._engines) == plans
    assert got == want and len(got) == len(sizes)
    S, K = len(det.scales), det.cfg.TEST.TOPK
    rows = det.run_batch(frames, color="nv12", return_device=True)
    assert rows.is_cuda and rows.dtype == torch.float32 and tuple(rows.shape) == (len(sizes), S * K, 56)
    rows = rows.cpu().numpy()
    for n in range(len(sizes)):
        assert np.array_equal(rows[n], np.array(want[n][1], np.float32)), n
    assert len(det.model._engines) == plans
    if arch == "dla_34":
        want = det.run_batch(hosts, dets_only=True)
        plans = len(det.model._engines)
        assert det.run_batch(frames, dets_only=True, color="nv12") == want
        assert len(det.model._engines) == plans


# ---------------------------------------------------------------- 6. refusals
def test_refusals(monkeypatch):
    from centerpose_amd._lib import CenterposeHipError
    det = _det(TEST__FLIP_TEST=True, **FIX)
    y = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
    uv = torch.zeros((4, 4, 2), dtype=torch.uint8, device="cuda")
    u = torch.zeros((4, 4), dtype=torch.uint8, device="cuda")
    surface = torch.zeros((12, 8), dtype=torch.uint8, device="cuda")
    bgr = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    cases = [("cpu", (y, uv.cpu()), dict(color="nv12")),
             ("uint8", (y, uv.float()), dict(color="nv12")),
             ("uint8", surface.short(), dict(color="nv21")),
             ("uv plane", (y, u), dict(color="nv12")),
             ("u and v planes", (y, u, uv[:, :, 0].unsqueeze(2)), dict(color="i420")),
             ("equal strides", (y, u, uv[:, :, 0]), dict(color="i420")),
             ("got 3 tensors", (y, u, u), dict(color="nv21")),
             ("three planes", surface, dict(color="i420")),
             ("even H and W", surface[:11], dict(color="nv12")),
             ("even H and W", surface[:, :7], dict(color="nv12")),
             ("mixed", (y, np.zeros((4, 4, 2), np.uint8)), dict(color="nv12")),
             ("device", (np.zeros((8, 8), np.uint8), np.zeros((4, 4, 2), np.uint8)), dict(color="nv12")),
             ("layout", (y, uv), dict(color="nv12", layout="chw")),
             ("unknown matrix", (y, uv), dict(color="nv12", matrix="bt2020")),
             ("matrix", bgr, dict(matrix="bt709")),
             ("matrix", bgr, dict(color="rgb", matrix="bt709")),
             ("unknown color", (y, uv), dict(color="yuv")),
             ("unknown color", bgr, dict(color="gray"))]
    for match, frame, kw in cases:
        with pytest.raises(CenterposeHipError, match=match):
            det.pre_process_batch([frame], 1, **kw)
        with pytest.raises(CenterposeHipError, match=match):
            det.run_batch([frame], **kw)
        with pytest.raises(CenterposeHipError, match=match):
            det.pre_process(frame, 1, **kw)
        with pytest.raises(CenterposeHipError, match=match):
            det.run(frame, **kw)
    with pytest.raises(CenterposeHipError, match="mixed"):
        det.run_batch([np.zeros((12, 8), np.uint8), surface], color="nv12")
    with pytest.raises(CenterposeHipError, match="list of frames"):
        det.run_batch(surface.unsqueeze(0), color="nv12")
    # planes on another device than the model: the model is said to live on a second card
    assert y.device == det._model_device()
    monkeypatch.setattr(det, "_model_device", lambda: torch.device("cuda", y.device.index + 1))
    for call in (lambda: det.pre_process((y, uv), 1, color="nv12"), lambda: det.pre_process_batch([surface], 1, color="nv21"),
                 lambda: det.run_batch([(y, u, u)], color="i420"), lambda: det.run((y, uv), color="nv12")):
        with pytest.raises(CenterposeHipError, match="the model is on cuda:%d" % (y.device.index + 1)):
            call()


BAD_SECOND = [(dict(y_base=0), None, b"null base"), (dict(u_base=0), None, b"null base"), (dict(v_base=0), None, b"null base"),
              (dict(y_row=-8), None, b"negative stride"), (dict(c_pix=-2), None, b"negative stride"),
              ({}, (0,) + yuv_ref.COEF["bt601"][1:], b"CY must be positive"), ({}, yuv_ref.COEF["bt601"][:4] + (1 << 24, 16), b"overflow")]


@pytest.mark.parametrize("fields,coef,message", BAD_SECOND)
def test_bad_descriptor_or_coef_through_ctypes_launches_nothing(fields, coef, message):
    from centerpose_amd import _lib, detector
    L = _lib.lib()
    y = torch.full((8, 8), 200, dtype=torch.uint8, device="cuda")
    uv = torch.full((4, 4, 2), 128, dtype=torch.uint8, device="cuda")
    out = torch.full((2, 3, 8, 8), -7.0, device="cuda")
    table = np.zeros(2, detector.YUV_FRAME_DESC)
    for n in range(2):
        d = table[n]
        d["y_base"], d["y_row"], d["y_pix"], d["u_base"], d["v_base"], d["c_row"], d["c_pix"] = y.data_ptr(), 8, 1, uv.data_ptr(), uv.data_ptr() + 1, 8, 2
        d["mid_off"], d["H"], d["W"], d["NH"], d["NW"], d["mi"], d["slot"] = -1, 8, 8, 8, 8, (1, 0, 0, 0, 1, 0), n
    mean, std = (ctypes.c_float * 3)(0.4, 0.4, 0.4), (ctypes.c_float * 3)(0.3, 0.3, 0.3)

    def call(coef):
        dev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).cuda()
        rc = L.cp_preprocess_yuv_frames_u8_f32(ctypes.c_void_p(dev.data_ptr()), table.ctypes.data_as(ctypes.c_void_p), 2, (ctypes.c_int * 6)(*coef),
                                               None, ctypes.c_size_t(0), ctypes.c_void_p(out.data_ptr()), 2, 8, 8, mean, std, 0, _lib.stream())
        torch.cuda.synchronize()
        return rc

    good = dict((k, table[0][k]) for k in fields)
    for k, val in fields.items():
        table[1][k] = val                                    # the SECOND descriptor is bad: the first must not have been launched either
    assert call(coef or yuv_ref.COEF["bt601"]) == 1 and message in L.cp_last_error()
    assert bool((out == -7.0).all())
    for k in fields:
        table[1][k] = good[k]
    assert call(yuv_ref.COEF["bt601"]) == 0                  # the same call with the descriptor / matrix mended runs
    # (200, 128, 128) -> ((200 - 16) * 1220542 + 2^19) >> 20 = 214 in all three channels
    assert yuv_ref.to_bgr(200, 128, 128, yuv_ref.COEF["bt601"]).tolist() == [214, 214, 214]
    want = np.float32((np.float64(214) / 255.0 - np.float64(np.float32(0.4))) / np.float64(np.float32(0.3)))
    assert bool((out == float(want)).all())
