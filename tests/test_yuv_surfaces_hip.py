"""GPU: device frames in P010 / P016, i422, i444, i400 and packed yuyv / uyvy, and the full-range / BT.2020 matrices, through
pre_process_batch / run_batch / ReidExtractor.embed (csrc/yuv_source.h in csrc/yuv_frames.hip and csrc/reid_crops.hip).  Every
comparison is bit for bit: against oracle.prepost_np.pre_process of the HxWx3 BGR array that tests/yuv_surface_ref.py converts the frame
to, and against the staging path on that array -- every addressing form of every colour under both store kernels, 16-bit against
8-bit, the matrices, mixed sizes and forms in one launch with the sources left alone, run_batch and embed against the converted
arrays, one 16-bit 4:4:4 table through the C ABI, and the refusals that must launch nothing.  Conventions of test_yuv_frames_hip.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import reid_ref
import reid_util
import yuv_ref
import yuv_surface_ref as ysr
from oracle import prepost_np as pp

pytestmark = pytest.mark.gpu

SIZES = [(37, 53), (64, 80), (2, 2), (1, 9), (9, 1)]
FIX = dict(TEST__FIX_RES=True, MODEL__INPUT_H=48, MODEL__INPUT_W=64)
GEOMETRIES = {"vec4": (FIX, b"preprocess_yuv_surfaces_kernel<vec4>"),
              "scalar": (dict(TEST__FIX_RES=True, MODEL__INPUT_H=48, MODEL__INPUT_W=62), b"preprocess_yuv_surfaces_kernel<scalar>"),
              "padded": (dict(TEST__FIX_RES=False), b"preprocess_yuv_surfaces_kernel<vec4>")}
VP = ctypes.c_void_p


def _scales(h, w):
    return (1, 2) if min(h, w) == 1 else (1, 0.5, 2)           # a one-pixel side has no pixels at 0.5


def _junk(seed, dtype, *shape):
    return np.random.RandomState(seed).randint(0, 1 << (8 * np.dtype(dtype).itemsize), size=shape).astype(dtype)


def _cuda(a, uint16=True):
    """A host array as a contiguous device tensor; 16-bit samples as torch.uint16 or, the same bits, torch.int16."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        t = torch.from_numpy(a.view(np.int16)).cuda()
        return t.view(torch.uint16) if uint16 else t
    return torch.from_numpy(a).cuda()


def _offset(a, uint16=True):
    """The same, with the first sample one sample past an allocation's start: an odd address for bytes, 2 mod 4 for 16-bit samples."""
    a = np.ascontiguousarray(a)
    wide = a.dtype == np.uint16
    storage = torch.zeros((a.size + 1,), dtype=torch.int16 if wide else torch.uint8, device="cuda")
    t = storage[1:].view(a.shape)
    t.copy_(torch.from_numpy(a.view(np.int16) if wide else a))
    assert t.data_ptr() % 4 == 2 if wide else t.data_ptr() % 2 == 1
    return t.view(torch.uint16) if wide and uint16 else t


def _within(seed, a, top, left, pad_h, pad_w):
    """-> (the larger random device tensor, its view that holds `a` at (top, left)): pitched rows, crops."""
    big = _junk(seed, a.dtype, a.shape[0] + pad_h, a.shape[1] + pad_w, *a.shape[2:])
    big[top:top + a.shape[0], left:left + a.shape[1]] = a
    t = _cuda(big)
    return t, t[top:top + a.shape[0], left:left + a.shape[1]]


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


def _forms(seed, h, w):
    """Every addressing form of every new colour for one frame size: [(name, what is given to the detector, color, host planes as
    yuv_surface_ref takes them)].  The packed colours need an even W: they run at w rounded up."""
    forms = []
    # ---- p010 / p016: the forms of nv12 with 16-bit samples
    y, uv = ysr.random_planes(seed, "p010", h, w)
    ch, cw = uv.shape[:2]
    forms += [("p010 planes, uint16", (_cuda(y), _cuda(uv)), "p010", (y, uv)),
              ("p016 planes, an int16-typed view", (_cuda(y, False), _cuda(uv, False)), "p016", (y, uv)),
              ("p010 planes at 2 mod 4", (_offset(y), _offset(uv)), "p010", (y, uv)),
              ("p016, int16 uv at 2 mod 4", (_cuda(y, False), _offset(uv, False)), "p016", (y, uv)),
              ("p010 crop at (6, 8)", (_within(seed + 1, y, 6, 8, 22, 28)[1], _within(seed + 2, uv, 3, 4, 11, 14)[1]), "p010", (y, uv))]
    pair = _junk(seed + 3, np.uint16, 1, 1, 2)
    forms.append(("p010, expanded chroma", (_cuda(y), _cuda(pair).expand(ch, cw, 2)), "p010", (y, np.broadcast_to(pair, (ch, cw, 2)))))
    if h % 2 == 0 and w % 2 == 0:
        surface = np.concatenate([y, uv.reshape(h // 2, w)], 0)
        forms.append(("p010 surface, pitch w + 48 samples", _within(seed + 4, surface, 0, 0, 0, 48)[1], "p010", (y, uv)))
        forms.append(("p016 surface, pitch w + 47 samples: every other row at 2 mod 4", _within(seed + 5, surface, 0, 0, 0, 47)[1], "p016", (y, uv)))
    # ---- i422 / i444: three byte planes
    for color in ("i422", "i444"):
        y, u, v = ysr.random_planes(seed + 10, color, h, w)
        cw = u.shape[1]
        forms += [("%s planes" % color, (_cuda(y), _cuda(u), _cuda(v)), color, (y, u, v)),
                  ("%s at odd addresses" % color, (_offset(y), _offset(u), _offset(v)), color, (y, u, v)),
                  ("%s, pitched planes" % color, (_within(seed + 11, y, 0, 0, 0, 48)[1], _within(seed + 12, u, 0, 0, 0, 23)[1], _within(seed + 13, v, 0, 0, 0, 23)[1]),
                   color, (y, u, v))]
        one = _junk(seed + 14, np.uint8, 1, 1, 2)
        forms.append(("%s, expanded chroma" % color, (_cuda(y), _cuda(one[:, :, 0]).expand(h, cw), _cuda(one[:, :, 1]).expand(h, cw)), color,
                      (y, np.broadcast_to(one[:, :, 0], (h, cw)), np.broadcast_to(one[:, :, 1], (h, cw)))))
    y, u, v = ysr.random_planes(seed + 10, "i422", h, w)
    cw = u.shape[1]                                            # a crop at an even column (any row): the chroma phase is kept
    forms.append(("i422 crop at (5, 8)", (_within(seed + 15, y, 5, 8, 9, 28)[1], _within(seed + 16, u, 5, 4, 9, 14)[1], _within(seed + 17, v, 5, 4, 9, 14)[1]),
                  "i422", (y, u, v)))
    y, u, v = ysr.random_planes(seed + 10, "i444", h, w)
    packed = _cuda(np.stack([y, u, v], -1))                    # the planes as strided views of one packed [H,W,3] buffer, at any origin
    forms.append(("i444 as views of a packed buffer", (packed[..., 0], packed[..., 1], packed[..., 2]), "i444", (y, u, v)))
    forms.append(("i444 crop at (5, 7)", tuple(_within(seed + 18 + k, p, 5, 7, 9, 13)[1] for k, p in enumerate((y, u, v))), "i444", (y, u, v)))
    # ---- i400: one plane
    forms += [("i400 plane", _cuda(y), "i400", (y,)), ("i400 1-tuple at an odd address", (_offset(y),), "i400", (y,)),
              ("i400 crop at (5, 7) of a pitched frame", _within(seed + 21, y, 5, 7, 9, 13)[1], "i400", (y,))]
    # ---- yuyv / uyvy: one packed tensor
    we = w + w % 2
    for color in ("yuyv", "uyvy"):
        p, = ysr.random_planes(seed + 30, color, h, we)
        forms += [("%s packed" % color, _cuda(p), color, (p,)), ("%s at an odd address" % color, _offset(p), color, (p,)),
                  ("%s cropped at column 8 of a pitched frame" % color, _within(seed + 31, p, 3, 8, 5, 22)[1], color, (p,))]
    return forms


def _same_meta(a, b):
    return set(a) == set(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in b)


def _check_forms(det, forms, scale, kernel, matrix="bt601"):
    nb = 2 if det.cfg.TEST.FLIP_TEST else 1
    staged = {}
    for name, given, color, planes in forms:
        what = (name, tuple(planes[0].shape), scale, matrix)
        host = ysr.frame_to_bgr(planes, color, matrix)
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


# ---------------------------------------------------------------- 1. every addressing form of every new colour, bit for bit
@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("geometry", ["vec4", "scalar", "padded"])
def test_every_addressing_form_bit_exact(geometry, flip):
    over, kernel = GEOMETRIES[geometry]
    det = _det(TEST__FLIP_TEST=flip, **over)
    for i, (h, w) in enumerate(SIZES):
        forms = _forms(100 + 40 * i, h, w)
        assert len(forms) == (28 if h % 2 == 0 and w % 2 == 0 else 26)
        assert {f[2] for f in forms} == set(ysr.COLORS)
        for scale in _scales(h, w):
            _check_forms(det, forms, scale, kernel)


def test_forms_lie_where_their_names_say():
    forms = dict((f[0], f[1]) for f in _forms(100, 64, 80))
    assert forms["p010 planes, uint16"][0].dtype == torch.uint16 and forms["p016 planes, an int16-typed view"][1].dtype == torch.int16
    assert all(t.data_ptr() % 4 == 2 for t in forms["p010 planes at 2 mod 4"])
    s = forms["p016 surface, pitch w + 47 samples: every other row at 2 mod 4"]
    assert s.stride() == (127, 1) and (s.data_ptr() + 65 * 127 * 2) % 4 == 2 and tuple(s.shape) == (96, 80)      # chroma row 1
    assert all(t.data_ptr() % 2 == 1 for t in forms["i422 at odd addresses"]) and forms["yuyv at an odd address"].data_ptr() % 2 == 1
    assert forms["i444, expanded chroma"][1].stride() == (0, 0) and forms["p010, expanded chroma"][1].stride() == (0, 0, 1)
    c = forms["yuyv cropped at column 8 of a pitched frame"]
    assert c.stride() == (204, 2, 1) and c.storage_offset() == 3 * 204 + 16


# ---------------------------------------------------------------- 2. 16-bit against 8-bit
@pytest.mark.parametrize("matrix", ["bt601", "bt709-full"])
def test_p016_holding_x_shl_8_equals_nv12_holding_x(matrix):
    det = _det(TEST__FLIP_TEST=True, **FIX)
    for h, w in ((37, 53), (64, 80)):
        y, uv = ysr.random_planes(250, "nv12", h, w)
        wide = (y.astype(np.uint16) << 8, uv.astype(np.uint16) << 8)
        for scale in (1, 0.5, 2):
            a = det.pre_process_batch([(_cuda(wide[0]), _cuda(wide[1]))], scale, color="p016", matrix=matrix)[0]
            assert _last_kernel() == b"preprocess_yuv_surfaces_kernel<vec4>"
            b = det.pre_process_batch([(_cuda(y), _cuda(uv))], scale, color="nv12", matrix=matrix)[0]
            assert _last_kernel() == b"preprocess_yuv_frames_kernel<vec4>"              # format word 0: the kernels it always ran
            assert torch.equal(a, b), (h, w, scale)


# ---------------------------------------------------------------- 3. the matrices
SIBLING = {"bt601-full": "bt601", "bt709-full": "bt709", "bt2020-limited": "bt601", "bt2020-full": "bt2020-limited"}


@pytest.mark.parametrize("matrix", sorted(SIBLING))
def test_each_new_matrix_is_used_and_differs_from_its_sibling(matrix):
    det = _det(TEST__FLIP_TEST=True, **FIX)
    forms = [f for f in _forms(200, 37, 53) if f[0] in ("p010 planes, uint16", "i444 planes", "i400 plane", "yuyv packed")]
    assert len(forms) == 4
    # one old colour under the new matrix: format word 0, so the kernels that were there, with the new coefficients
    y, uv = ysr.random_planes(260, "nv12", 37, 53)
    for scale in (1, 0.5, 2):
        _check_forms(det, forms, scale, b"preprocess_yuv_surfaces_kernel<vec4>", matrix=matrix)
        _check_forms(det, [("nv12 planes", (_cuda(y), _cuda(uv)), "nv12", (y, uv))], scale, b"preprocess_yuv_frames_kernel<vec4>", matrix=matrix)
    for _, given, color, planes in forms + [("nv12 planes", (_cuda(y), _cuda(uv)), "nv12", (y, uv))]:
        assert not np.array_equal(ysr.frame_to_bgr(planes, color, matrix), ysr.frame_to_bgr(planes, color, SIBLING[matrix])), color
        a = det.pre_process_batch([given], 1, color=color, matrix=matrix)[0]
        b = det.pre_process_batch([given], 1, color=color, matrix=SIBLING[matrix])[0]
        assert not torch.equal(a, b), color
    # the old names compute what they computed: tests/yuv_ref.py's array
    assert np.array_equal(ysr.frame_to_bgr((y, uv), "nv12", "bt601"), yuv_ref.frame_to_bgr((y, uv), "nv12", "bt601"))


# ---------------------------------------------------------------- 4. mixed sizes and forms in one launch; sources left alone
@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("color", ["p010", "i422", "yuyv"])
def test_mixed_sizes_and_forms_of_one_colour_in_one_launch(color, flip):
    det = _det(TEST__FLIP_TEST=flip, **FIX)
    nb = 2 if flip else 1
    sizes = [(37, 54), (64, 80), (1, 10)] if color == "yuyv" else [(37, 53), (64, 80), (1, 9)]
    planes = [ysr.random_planes(300 + 10 * k, color, h, w) for k, (h, w) in enumerate(sizes)]
    hosts = [ysr.frame_to_bgr(p, color, "bt601-full") for p in planes]
    owners = []
    if color == "p010":
        y, uv = planes[1]
        alloc, surface = _within(330, np.concatenate([y, uv.reshape(32, 80)], 0), 0, 0, 0, 48)
        big_y, crop_y = _within(331, planes[0][0], 6, 8, 22, 28)
        big_uv, crop_uv = _within(332, planes[0][1], 3, 4, 11, 14)
        frames = [(crop_y, crop_uv), surface, (_offset(planes[2][0], False), _offset(planes[2][1], False))]       # a crop, a pitched surface, int16 at 2 mod 4
        owners = [alloc, big_y, big_uv]
    elif color == "i422":
        bigs = [_within(340 + k, p, 5, 8 if k == 0 else 4, 9, 28 if k == 0 else 14) for k, p in enumerate(planes[0])]
        pitched = [_within(345 + k, p, 0, 0, 0, 48 if k == 0 else 23) for k, p in enumerate(planes[1])]
        frames = [tuple(b[1] for b in bigs), tuple(p[1] for p in pitched), tuple(_offset(p) for p in planes[2])]
        owners = [b[0] for b in bigs] + [p[0] for p in pitched]
    else:
        big, crop = _within(350, planes[0][0], 3, 8, 5, 22)
        alloc, pitched = _within(351, planes[1][0], 0, 0, 0, 24)
        frames = [crop, pitched, _offset(planes[2][0])]
        owners = [big, alloc]
    before = [t.view(torch.uint8).clone() for t in owners]
    for scale in (0.5, 1, 2):
        n = 2 if scale == 0.5 else 3                         # a one-row frame has no pixels at 0.5
        x, metas = det.pre_process_batch(frames[:n], scale, color=color, matrix="bt601-full")
        assert _last_kernel() == b"preprocess_yuv_surfaces_kernel<vec4>"
        got = x.cpu().numpy()
        assert got.shape == (nb * n, 3, 48, 64)
        for k in range(n):
            ref, rmeta = _oracle(det, hosts[k], scale)
            assert np.array_equal(got[nb * k:nb * k + nb], ref), (scale, k)
            assert _same_meta(metas[k], rmeta)
        assert np.array_equal(got, det.pre_process_batch(hosts[:n], scale)[0].cpu().numpy()), scale
    torch.cuda.synchronize()
    for t, b in zip(owners, before):                          # the sources, padding and surroundings included, are byte-identical
        assert torch.equal(t.view(torch.uint8), b)
    from centerpose_amd._lib import CenterposeHipError
    with pytest.raises(CenterposeHipError, match="no pixels"):
        det.pre_process_batch(frames, 0.5, color=color)


# ---------------------------------------------------------------- 5. run_batch
def _structured(seed, h, w):
    """A frame with large-scale structure as 8-bit (y, u, v) planes at full resolution."""
    r = np.random.RandomState(seed)
    grid = torch.from_numpy(r.uniform(0, 255, (1, 3, 5, 6)))
    up = torch.nn.functional.interpolate(grid, size=(h, w), mode="bilinear", align_corners=False)[0].numpy()
    return np.clip(np.rint(up + r.uniform(-20, 20, up.shape)), 0, 255).astype(np.uint8)


def _p010_surface(seed, h, w, pitch):
    """A P010 surface [h*3/2, w] on the device with `pitch` samples per row -> (the surface view, its host planes)."""
    yuv = _structured(seed, h, w)
    low = _junk(seed + 1, np.uint16, h * 3 // 2, w) & 63                                 # whatever the low six bits hold counts
    y = (yuv[0].astype(np.uint16) << 8) | low[:h]
    uv = (np.stack([yuv[1][::2, ::2], yuv[2][::2, ::2]], -1).astype(np.uint16) << 8) | low[h:].reshape(h // 2, w // 2, 2)
    return _within(seed + 2, np.concatenate([y, uv.reshape(h // 2, w)], 0), 0, 0, 0, pitch - w)[1], (y, uv)


def _yuyv_frame(seed, h, w):
    yuv = _structured(seed, h, w)
    p = np.empty((h, w, 2), np.uint8)
    p[:, :, 0], p[:, 0::2, 1], p[:, 1::2, 1] = yuv[0], yuv[1][:, 0::2], yuv[2][:, 0::2]
    return _within(seed + 2, p, 2, 4, 6, 12)[1], (p,)


@pytest.mark.parametrize("color,matrix", [("p010", "bt2020-limited"), ("yuyv", "bt601-full")])
def test_run_batch_equals_run_batch_of_the_converted_host_arrays(color, matrix):
    det = _det("dla_34")
    sizes = [(200, 264), (96, 128), (200, 264)]
    assert len(det._batch_groups(sizes)) == 2
    made = [_p010_surface(610 + 10 * i, h, w, w + 32) if color == "p010" else _yuyv_frame(610 + 10 * i, h, w) for i, (h, w) in enumerate(sizes)]
    frames = [m[0] for m in made]
    if color == "p010":                                       # surfaces and plane tuples in one call
        y, uv = made[1][1]
        frames[1] = (_cuda(y, False), _cuda(uv, False))
    hosts = [ysr.frame_to_bgr(m[1], color, matrix) for m in made]
    want = det.run_batch(hosts)
    plans = len(det.model._engines)
    got = det.run_batch(frames, color=color, matrix=matrix)
    assert got == want and len(got) == len(sizes)
    S, K = len(det.scales), det.cfg.TEST.TOPK
    rows = det.run_batch(frames, color=color, matrix=matrix, return_device=True)
    assert rows.is_cuda and rows.dtype == torch.float32 and tuple(rows.shape) == (len(sizes), S * K, 56)
    rows = rows.cpu().numpy()
    for n in range(len(sizes)):
        assert np.array_equal(rows[n], np.array(want[n][1], np.float32)), n
    assert len(det.model._engines) == plans
    want = det.run_batch(hosts, dets_only=True)
    plans = len(det.model._engines)
    assert det.run_batch(frames, dets_only=True, color=color, matrix=matrix) == want
    rows = det.run_batch(frames, dets_only=True, color=color, matrix=matrix, return_device=True).cpu().numpy()
    for n in range(len(sizes)):
        assert np.array_equal(rows[n], np.array(want[n][1], np.float32)), n
    assert len(det.model._engines) == plans                   # no plan per colour
    # one frame through pre_process and run
    one = det.run(frames[0], color=color, matrix=matrix)
    assert one["results"] == det.run(hosts[0])["results"]


# ---------------------------------------------------------------- 6. embed
@functools.lru_cache(maxsize=None)
def _ex(cap=8):
    from centerpose_amd import reid, synth
    return reid.ReidExtractor(synth.make_state_dict("reid", seed=1), capacity=cap)


def _rows2():
    rows = np.zeros((2, 4, 56), np.float32)
    for n in range(2):
        rows[n, 0] = reid_ref.row(5, 8, 60, 90)
        rows[n, 1] = reid_ref.row(40, 2, 100, 80, 0.2)         # below the threshold
        rows[n, 2] = reid_ref.row(-10, 30, 50, 140)
        rows[n, 3] = reid_ref.row(70, 20, 127, 95, 0.9)
    return rows


def _host_table(frames_np, color):
    """YUV_FRAME_DESC rows that address host NumPy planes in place, by the library's pure geometry function."""
    from centerpose_amd import frames
    rows = []
    for planes in frames_np:
        H, W, y_off, y_row, y_pix, u_off, v_off, c_row, c_pix, fmt = frames.yuv_surface_geometry(
            [p.shape for p in planes], [tuple(s // p.itemsize for s in p.strides) for p in planes], color, [p.dtype for p in planes])
        u_plane, v_plane = (planes[0], planes[0]) if len(planes) == 1 else (planes[1], planes[-1])
        rows.append(frames.YuvSurface(planes[0].ctypes.data + y_off, H, W, y_row, y_pix, u_plane.ctypes.data + u_off, v_plane.ctypes.data + v_off,
                                      c_row, c_pix, fmt))
    return frames.identity_table(rows, True)


@pytest.mark.parametrize("color,matrix", [("p010", "bt2020-full"), ("i444", "bt601-full"), ("yuyv", "bt709")])
def test_embed_crops_equal_the_host_twin_and_features_those_of_the_converted_frames(color, matrix):
    from centerpose_amd import _lib
    ex = _ex()
    H, W = 96, 128
    host_planes, given = [], []
    for n in range(2):
        yuv = _structured(20 + n, H, W)
        if color == "p010":
            low = _junk(30 + n, np.uint16, H * 3 // 2, W) & 63
            planes = ((yuv[0].astype(np.uint16) << 8) | low[:H],
                      (np.stack([yuv[1][::2, ::2], yuv[2][::2, ::2]], -1).astype(np.uint16) << 8) | low[H:].reshape(H // 2, W // 2, 2))
            frame = _within(40 + n, np.concatenate([planes[0], planes[1].reshape(H // 2, W)], 0), 0, 0, 0, 31)[1] if n else (_cuda(planes[0]), _offset(planes[1]))
        elif color == "i444":
            planes = tuple(np.ascontiguousarray(p) for p in yuv)
            frame = tuple(_offset(p) for p in planes) if n else tuple(_cuda(p) for p in planes)
        else:
            planes = (np.stack([yuv[0], np.where(np.arange(W) % 2 == 0, yuv[1], yuv[2])], -1),)
            frame = _within(40 + n, planes[0], 3, 8, 5, 22)[1] if n else _cuda(planes[0])
        host_planes.append(planes)
        given.append(frame)
    rows = _rows2()
    dev_rows = torch.from_numpy(rows).cuda()
    a = ex.embed(given, dev_rows, color=color, matrix=matrix)
    crops = ex.engine.input.cpu().numpy().copy()
    L = _lib.lib()
    table = _host_table(host_planes, color)
    out = np.full(8 * 3 * 128 * 64 + reid_util.GUARD, np.nan, np.float32)
    nm = reid_util.norm_struct(scale=float(ex.norm["scale"][0]), mean=tuple(ex.norm["mean"][0]), std=tuple(ex.norm["std"][0]),
                               channel_order=("bgr", "rgb")[int(ex.norm["rgb"][0])])
    slots = a.slots.cpu().numpy().astype(np.int32)
    rc = L.cp_reid_crop_yuv_frames_host(table.ctypes.data_as(VP), 2, (ctypes.c_int * 6)(*ysr.COEF[matrix]), rows.ctypes.data_as(VP), 4, ctypes.c_float(0.3),
                                        slots.ctypes.data_as(VP), 8, nm.ctypes.data_as(VP), out.ctypes.data_as(VP))
    assert rc == 0, L.cp_last_error()
    assert slots.tolist() == [0, 2, 3, -1, 4, 6, 7, -1] and a.counts.cpu().tolist() == [3, 3]
    assert reid_util.same_bits(crops, out[:8 * 3 * 128 * 64].reshape(8, 3, 128, 64))
    converted = [ysr.frame_to_bgr(p, color, matrix) for p in host_planes]
    b = ex.embed([torch.from_numpy(c).cuda() for c in converted], dev_rows)
    assert torch.equal(a.features, b.features) and torch.equal(a.slots, b.slots) and torch.equal(a.counts, b.counts)
    assert reid_util.same_bits(ex.engine.input.cpu().numpy(), crops)


def test_crop_launcher_names_the_general_instantiation_only_for_a_non_zero_word():
    from centerpose_amd import _lib, frames
    L = _lib.lib()
    y, uv = ysr.random_planes(800, "p010", 36, 52)
    y8, uv8 = ysr.random_planes(801, "nv12", 36, 52)
    io = frames.FrameIO(torch.device("cuda", torch.cuda.current_device()))
    keep = [(_cuda(y), _cuda(uv)), (_cuda(y8), _cuda(uv8))]
    rows = torch.from_numpy(np.stack([np.stack([reid_ref.row(3, 3, 40, 30)])])).cuda()
    nm = reid_util.norm_struct()
    for (frame, color), kernel in zip(((keep[0], "p010"), (keep[1], "nv12")), (b"reid_crop_kernel<surfaces>", b"reid_crop_kernel<yuv>")):
        table = frames.identity_table([io.yuv_frame(frame, color)], True)
        dev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).cuda()
        slots = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = torch.full((1, 3, 128, 64), float("nan"), device="cuda")
        rc = L.cp_reid_crop_yuv_frames_f32(VP(dev.data_ptr()), table.ctypes.data_as(VP), 1, (ctypes.c_int * 6)(*ysr.COEF["bt709"]), VP(rows.data_ptr()), 1,
                                           ctypes.c_float(0.3), VP(slots.data_ptr()), 1, nm.ctypes.data_as(VP), VP(out.data_ptr()), _lib.stream())
        torch.cuda.synchronize()
        assert rc == 0 and L.cp_last_kernel() == kernel, L.cp_last_error()
        planes = (y, uv) if color == "p010" else (y8, uv8)
        want, _, _ = reid_ref.crops([ysr.frame_to_bgr(planes, color, "bt709")], rows.cpu().numpy(), 0.3, 1)
        assert reid_util.same_bits(out.cpu().numpy(), want)


# ---------------------------------------------------------------- 7. the C ABI directly: 16-bit 4:4:4, which Python names no colour for
def test_a_16_bit_444_table_through_the_c_abi():
    from centerpose_amd import _lib
    L = _lib.lib()
    det = _det(TEST__FLIP_TEST=False, **FIX)
    H, W = 37, 53
    y, u, v = (_junk(900 + k, np.uint16, H, W) for k in range(3))
    host = ysr.to_bgr16(y, u, v, ysr.COEF["bt2020-full"])
    keep = [_offset(y, False), _offset(u, False), _cuda(v, False)]
    frame = (keep[0].data_ptr(), H, W, 2 * W, 2, keep[1].data_ptr(), keep[2].data_ptr(), 2 * W, 2, 7)           # y and u at 2 mod 4
    for scale in (1, 0.5):
        table, scratch_bytes, inp_h, inp_w, _ = det._pre_table([(H, W)], None, [0], scale, [frame], True)
        assert table["pad"].tolist() == [7]
        dev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).cuda()
        scratch = torch.empty(max(scratch_bytes, 1), dtype=torch.uint8, device="cuda")
        out = torch.full((1, 3, inp_h, inp_w), float("nan"), device="cuda")
        mean, std = (ctypes.c_float * 3)(*det.cfg.DATASET.MEAN), (ctypes.c_float * 3)(*det.cfg.DATASET.STD)
        rc = L.cp_preprocess_yuv_frames_u8_f32(VP(dev.data_ptr()), table.ctypes.data_as(VP), 1, (ctypes.c_int * 6)(*ysr.COEF["bt2020-full"]),
                                               VP(scratch.data_ptr()), ctypes.c_size_t(scratch_bytes), VP(out.data_ptr()), 1, inp_h, inp_w, mean, std, 0,
                                               _lib.stream())
        torch.cuda.synchronize()
        assert rc == 0 and L.cp_last_kernel() == b"preprocess_yuv_surfaces_kernel<vec4>", L.cp_last_error()
        assert np.array_equal(out.cpu().numpy(), _oracle(det, host, scale)[0]), scale


# ---------------------------------------------------------------- 8. refusals that launch nothing
def test_draw_refusals_launch_nothing_and_leave_the_frames_alone():
    from centerpose_amd import _lib
    from centerpose_amd._lib import CenterposeHipError
    L = _lib.lib()
    det = _det("dla_34")
    y, uv = ysr.random_planes(950, "p010", 96, 128)
    p, = ysr.random_planes(951, "yuyv", 96, 128)
    y8, uv8 = ysr.random_planes(952, "nv12", 96, 128)
    wide, packed, nv12 = (_cuda(y, False), _cuda(uv, False)), _cuda(p), (_cuda(y8), _cuda(uv8))
    rows = torch.zeros((1, 2, 56), device="cuda")
    rows[0, 0, :5] = torch.tensor([10.0, 10.0, 90.0, 80.0, 1.0])
    tracks = [np.array([[10, 10, 90, 80, 3]])]
    x = det.pre_process_batch([nv12], 1, color="nv12")[0]                                # the last launch before the refusals
    torch.cuda.synchronize()
    marker = L.cp_last_kernel()
    before = [t.clone() for t in wide + (packed,) + nv12]
    calls = [("cannot be drawn on", lambda: det.draw_results([wide], rows, color="p010")),
             ("cannot be drawn on", lambda: det.draw_tracks([packed], tracks, color="yuyv")),
             ("cannot be drawn on", lambda: det.run_batch([wide], color="p016", draw=True)),
             ("cannot be drawn on", lambda: det.run_batch([packed], color="yuyv", draw=True, return_device=True)),
             ("not taken for drawing", lambda: det.draw_results([nv12], rows, color="nv12", matrix="bt601-full")),
             ("not taken for drawing", lambda: det.draw_tracks([nv12], tracks, color="nv12", matrix="bt2020-limited")),
             ("not taken for drawing", lambda: det.run_batch([nv12], color="nv12", matrix="bt709-full", draw=True))]
    for match, call in calls:
        with pytest.raises(CenterposeHipError, match=match):
            call()
        assert L.cp_last_kernel() == marker
    torch.cuda.synchronize()
    for t, b in zip(wide + (packed,) + nv12, before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8))
    # the C entry points name the field: a draw table with a non-zero format word
    from centerpose_amd import draw, frames
    io = frames.FrameIO(torch.device("cuda", torch.cuda.current_device()))
    table = frames.identity_table([io.yuv_frame(nv12, "nv12")], True)
    table["pad"] = 4
    dev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).cuda()
    st = draw.DrawStyle().struct("bt601")
    L.cp_draw_scratch_bytes.restype = ctypes.c_size_t
    scratch = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    rc = L.cp_draw_rows_yuv_frames_u8(VP(dev.data_ptr()), table.ctypes.data_as(VP), 1, VP(rows.data_ptr()), 2, ctypes.c_float(0.3), st.ctypes.data_as(VP),
                                      VP(scratch.data_ptr()), ctypes.c_size_t(scratch.numel()), _lib.stream())
    torch.cuda.synchronize()
    assert rc == 1 and b"pad = 4" in L.cp_last_error() and L.cp_last_kernel() == marker
    assert torch.equal(nv12[0], before[3]) and torch.equal(nv12[1], before[4])


def test_16_bit_misalignment_launches_nothing():
    from centerpose_amd import _lib, detector
    from centerpose_amd._lib import CenterposeHipError
    L = _lib.lib()
    det = _det(TEST__FLIP_TEST=True, **FIX)
    y, uv = ysr.random_planes(960, "p010", 8, 8)
    ty, tuv = _cuda(y, False), _cuda(uv, False)
    before = [ty.clone(), tuv.clone()]
    out = torch.full((2, 3, 8, 8), -7.0, device="cuda")
    table = np.zeros(2, detector.YUV_FRAME_DESC)
    for n in range(2):
        d = table[n]
        d["y_base"], d["y_row"], d["y_pix"], d["u_base"], d["v_base"], d["c_row"], d["c_pix"] = ty.data_ptr(), 16, 2, tuv.data_ptr(), tuv.data_ptr() + 2, 16, 4
        d["mid_off"], d["H"], d["W"], d["NH"], d["NW"], d["mi"], d["slot"], d["pad"] = -1, 8, 8, 8, 8, (1, 0, 0, 0, 1, 0), n, 4
    mean, std = (ctypes.c_float * 3)(0.4, 0.4, 0.4), (ctypes.c_float * 3)(0.3, 0.3, 0.3)

    def call():
        dev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).cuda()
        rc = L.cp_preprocess_yuv_frames_u8_f32(VP(dev.data_ptr()), table.ctypes.data_as(VP), 2, (ctypes.c_int * 6)(*ysr.COEF["bt601"]), None,
                                               ctypes.c_size_t(0), VP(out.data_ptr()), 2, 8, 8, mean, std, 0, _lib.stream())
        torch.cuda.synchronize()
        return rc

    # the SECOND descriptor is bad: the first must not have been launched either
    for field, value, message in (("y_base", ty.data_ptr() + 1, b"even luma"), ("v_base", tuv.data_ptr() + 1, b"even chroma"), ("c_row", 15, b"even chroma"),
                                  ("y_row", 17, b"even luma"), ("pad", 16, b"outside 0..15"), ("pad", 12 | 1, b"grey")):
        good = table[1][field]
        table[1][field] = value
        assert call() == 1 and message in L.cp_last_error(), (field, L.cp_last_error())
        assert bool((out == -7.0).all())
        table[1][field] = good
    assert call() == 0 and L.cp_last_kernel() == b"preprocess_yuv_surfaces_kernel<vec4>"
    want = ysr.frame_to_bgr((y, uv), "p010", "bt601").astype(np.float64).transpose(2, 0, 1)
    want = ((want / 255.0 - np.float64(np.float32(0.4))) / np.float64(np.float32(0.3))).astype(np.float32)
    got = out.cpu().numpy()
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
    assert torch.equal(ty, before[0]) and torch.equal(tuv, before[1])
    # through Python an odd address cannot arise from a 16-bit tensor, but a wrong dtype can: refused before any launch
    marker = L.cp_last_kernel()
    with pytest.raises(CenterposeHipError, match="uint16 or int16"):
        det.pre_process_batch([(ty.view(torch.uint8), tuv.view(torch.uint8))], 1, color="p010")
    with pytest.raises(CenterposeHipError, match="same dtype"):
        det.pre_process_batch([(ty, tuv.view(torch.uint16))], 1, color="p010")
    with pytest.raises(CenterposeHipError, match="must be uint8"):
        det.pre_process_batch([(ty, tuv)], 1, color="nv12")
    assert L.cp_last_kernel() == marker
