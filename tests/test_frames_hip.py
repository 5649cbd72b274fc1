"""GPU: frames that are already on the device (csrc/frame_sources.hip) through pre_process / pre_process_batch / run / run_batch --
every addressing mode bit for bit against the oracle on the equivalent host HxWx3 BGR array and against the staging path, the
sources read in place and left alone, run_batch on device frames against run_batch on host arrays, the device-resident result, and the
refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import prepost_np as pp

pytestmark = pytest.mark.gpu

SIZES = [(37, 53), (64, 80), (1, 9), (9, 1)]
FIX = dict(TEST__FIX_RES=True, MODEL__INPUT_H=48, MODEL__INPUT_W=64)


def _scales(h, w):
    return (1, 2) if min(h, w) == 1 else (1, 0.5, 2)           # a one-pixel side has no pixels at 0.5


def _bytes(seed, *shape):
    return (np.random.RandomState(seed).rand(*shape) * 256).astype(np.uint8)


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
    """The addressing modes for one frame size: [(name, what is given to the detector, layout, color, [equivalent host BGR arrays])]."""
    bgr = _bytes(seed, h, w, 3)
    forms = [("contiguous bgr", torch.from_numpy(bgr).cuda(), "hwc", "bgr", [bgr])]
    if (h, w) == (37, 53):
        big = _bytes(seed + 1, 64, 80, 3)
        forms.append(("crop view", torch.from_numpy(big).cuda()[5:42, 7:60], "hwc", "bgr", [big[5:42, 7:60].copy()]))
    bgra = np.concatenate([bgr, _bytes(seed + 2, h, w, 1)], 2)
    forms.append(("bgra", torch.from_numpy(bgra).cuda(), "hwc", "bgr", [bgr]))
    planar = np.ascontiguousarray(bgr[:, :, ::-1].transpose(2, 0, 1))
    forms.append(("planar rgb", torch.from_numpy(planar).cuda(), "chw", "rgb", [bgr]))
    clip = _bytes(seed + 3, 3, h, w, 3)
    forms.append(("clip", torch.from_numpy(clip).cuda(), "hwc", "bgr", [clip[n] for n in range(3)]))
    col = _bytes(seed + 4, h, 1, 3)
    forms.append(("expanded along W", torch.from_numpy(col).cuda().expand(h, w, 3), "hwc", "bgr", [np.broadcast_to(col, (h, w, 3)).copy()]))
    return forms


def _same_meta(a, b):
    return set(a) == set(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in b)


def _check_forms(det, forms, scale, kernel):
    nb = 2 if det.cfg.TEST.FLIP_TEST else 1
    for name, given, layout, color, hosts in forms:
        what = (name, tuple(hosts[0].shape), scale)
        frames = given if given.dim() == 4 else [given]
        x, metas = det.pre_process_batch(frames, scale, layout=layout, color=color)
        assert _last_kernel() == kernel, what
        assert x.is_cuda and x.dtype == torch.float32 and x.shape[0] == nb * len(hosts) and len(metas) == len(hosts), what
        got = x.cpu().numpy()
        staged, smetas = det.pre_process_batch(hosts, scale)
        assert np.array_equal(got, staged.cpu().numpy()), what
        for n, host in enumerate(hosts):
            ref, rmeta = _oracle(det, host, scale)
            assert np.array_equal(got[nb * n:nb * n + nb], ref), what + (n,)
            assert _same_meta(metas[n], rmeta) and _same_meta(metas[n], smetas[n]), what


# ---------------------------------------------------------------- 1. every addressing mode, bit for bit
@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("fix_res", [True, False])
def test_every_addressing_mode_bit_exact(fix_res, flip):
    det = _det(TEST__FLIP_TEST=flip, **(FIX if fix_res else dict(TEST__FIX_RES=False)))
    if not fix_res:
        assert det.input_geometry(37, 53, 1)[2:4] == (64, 64)
    for i, (h, w) in enumerate(SIZES):
        forms = _forms(100 + 10 * i, h, w)
        assert len(forms) == (6 if (h, w) == (37, 53) else 5)
        for scale in _scales(h, w):
            _check_forms(det, forms, scale, b"preprocess_frames_kernel<vec4>")


# ---------------------------------------------------------------- 2. the scalar store path
@pytest.mark.parametrize("flip", [True, False])
def test_scalar_store_path(flip):
    det = _det(TEST__FLIP_TEST=flip, TEST__FIX_RES=True, MODEL__INPUT_H=48, MODEL__INPUT_W=62)
    for i, (h, w) in enumerate(SIZES):
        forms = _forms(200 + 10 * i, h, w)
        for scale in _scales(h, w):
            _check_forms(det, forms, scale, b"preprocess_frames_kernel<scalar>")


# ---------------------------------------------------------------- 3. mixed sizes and layouts in one launch
@pytest.mark.parametrize("flip", [True, False])
def test_mixed_sizes_and_layouts_in_one_launch(flip):
    det = _det(TEST__FLIP_TEST=flip, **FIX)
    nb = 2 if flip else 1
    big = _bytes(300, 64, 80, 3)
    a = _bytes(301, 64, 80, 3)
    b = _bytes(302, 1, 9, 3)
    hosts = [big[5:42, 7:60].copy(), a, b]
    # one list, one layout word per call: the crop, a BGRA frame and a padded-row frame, all "hwc" / "bgr"
    padded = torch.zeros((1, 16, 4), dtype=torch.uint8, device="cuda")
    padded[:, :9, :3] = torch.from_numpy(b).cuda()
    frames = [torch.from_numpy(big).cuda()[5:42, 7:60],
              torch.from_numpy(np.concatenate([a, _bytes(303, 64, 80, 1)], 2)).cuda(),
              padded[:, :9]]
    assert [f.stride() for f in frames] == [(240, 3, 1), (320, 4, 1), (64, 4, 1)]
    for scale in (0.5, 1, 2):
        n = 2 if scale == 0.5 else 3                         # (1,9) has no pixels at 0.5
        x, metas = det.pre_process_batch(frames[:n], scale)
        got = x.cpu().numpy()
        assert got.shape == (nb * n, 3, 48, 64)
        for k in range(n):
            ref, rmeta = _oracle(det, hosts[k], scale)
            assert np.array_equal(got[nb * k:nb * k + nb], ref), (scale, k)
            assert _same_meta(metas[k], rmeta)
    # planar RGB frames of two sizes in one list
    planar = [torch.from_numpy(np.ascontiguousarray(h[:, :, ::-1].transpose(2, 0, 1))).cuda() for h in hosts[:2]]
    got = det.pre_process_batch(planar, 2, layout="chw", color="rgb")[0].cpu().numpy()
    for k in range(2):
        assert np.array_equal(got[nb * k:nb * k + nb], _oracle(det, hosts[k], 2)[0]), k
    from centerpose_amd._lib import CenterposeHipError
    with pytest.raises(CenterposeHipError, match="no pixels"):
        det.pre_process_batch(frames, 0.5)


# ---------------------------------------------------------------- 4. read in place, left alone, any byte address
def test_sources_left_alone_and_odd_byte_address():
    det = _det(TEST__FLIP_TEST=True, **FIX)
    host = _bytes(400, 37, 53, 3)
    storage = torch.zeros((37 * 53 * 3 + 1,), dtype=torch.uint8, device="cuda")
    odd = storage[1:].view(37, 53, 3)
    odd.copy_(torch.from_numpy(host))
    assert odd.data_ptr() % 2 == 1 and odd.data_ptr() == storage.data_ptr() + 1
    big = torch.from_numpy(_bytes(401, 64, 80, 3)).cuda()
    frames = [odd, big[5:42, 7:60]]
    before = [storage.clone(), big.clone()]
    for scale in (1, 0.5, 2):
        x, _ = det.pre_process_batch(frames, scale)
        got = x.cpu().numpy()
        assert np.array_equal(got[0:2], _oracle(det, host, scale)[0]), scale
        assert np.array_equal(got[2:4], _oracle(det, big.cpu().numpy()[5:42, 7:60].copy(), scale)[0]), scale
    assert torch.equal(storage, before[0]) and torch.equal(big, before[1])        # the crop's surroundings included
    assert frames[1].data_ptr() == big.data_ptr() + (5 * 80 + 7) * 3


# ---------------------------------------------------------------- 5. pre_process / run of one tensor
def test_pre_process_and_run_of_one_tensor():
    det = _det("dla_34")
    host = _bytes(500, 96, 128, 3)
    rgb_planar = torch.from_numpy(np.ascontiguousarray(host[:, :, ::-1].transpose(2, 0, 1))).cuda()
    for frame, kw in ((torch.from_numpy(host).cuda(), {}), (rgb_planar, dict(layout="chw", color="rgb"))):
        x, meta = det.pre_process(frame, 1, **kw)
        assert _last_kernel() == b"preprocess_frames_kernel<vec4>"
        want, wmeta = det.pre_process(host, 1)
        assert torch.equal(x, want) and _same_meta(meta, wmeta)
    want = det.run(host)
    got = det.run(torch.from_numpy(host).cuda())
    assert got["results"] == want["results"] and set(got) == set(want)
    assert det.run(rgb_planar, layout="chw", color="rgb")["results"] == want["results"]


# ---------------------------------------------------------------- 6. / 7. run_batch: device frames == host arrays; the device result
def _device_frames(hosts):
    """The host BGR arrays as device frames, every other one with an alpha channel of random bytes."""
    out = []
    for n, h in enumerate(hosts):
        if n % 2:
            h = np.concatenate([h, _bytes(600 + n, h.shape[0], h.shape[1], 1)], 2)
        out.append(torch.from_numpy(h).cuda())
    return out


@pytest.mark.parametrize("arch,sizes,groups", [("dla_34", [(200, 264), (96, 128), (200, 264), (96, 128)], 2),
                                               ("hrnet", [(120, 160), (96, 128)], 2)])
def test_run_batch_device_frames_equal_host_arrays(arch, sizes, groups):
    det = _det(arch)
    assert len(det._batch_groups(sizes)) == groups
    hosts = [_bytes(610 + i, h, w, 3) for i, (h, w) in enumerate(sizes)]
    frames = _device_frames(hosts)
    want = det.run_batch(hosts)
    plans = len(det.model._engines)
    got = det.run_batch(frames)
    assert len(det.model._engines) == plans
    assert got == want and len(got) == len(sizes)
    assert all(torch.equal(f.cpu(), torch.from_numpy(h if f.shape[2] == 3 else np.concatenate([h, f.cpu().numpy()[:, :, 3:]], 2)))
               for f, h in zip(frames, hosts))
    # 7. the rows as one device tensor, in input order (two groups: reordered on the device)
    S, K = len(det.scales), det.cfg.TEST.TOPK
    for given in (frames, hosts):
        rows = det.run_batch(given, return_device=True)
        assert rows.is_cuda and rows.dtype == torch.float32 and tuple(rows.shape) == (len(sizes), S * K, 56)
        rows = rows.cpu().numpy()
        for n in range(len(sizes)):
            assert np.array_equal(rows[n], np.array(want[n][1], np.float32)), n
    assert len(det.model._engines) == plans
    if arch == "dla_34":
        want = det.run_batch(hosts, dets_only=True)
        plans = len(det.model._engines)
        assert det.run_batch(frames, dets_only=True) == want
        assert len(det.model._engines) == plans


def test_run_batch_of_one_clip_tensor_planar():
    """One 4-D [N,C,H,W] RGB tensor (a data loader's batch): one group, no reordering."""
    det = _det("dla_34")
    hosts = [_bytes(700 + i, 96, 128, 3) for i in range(3)]
    clip = torch.from_numpy(np.stack([np.ascontiguousarray(h[:, :, ::-1].transpose(2, 0, 1)) for h in hosts])).cuda()
    want = det.run_batch(hosts)
    assert det.run_batch(clip, layout="chw", color="rgb") == want
    rows = det.run_batch(clip, layout="chw", color="rgb", return_device=True)
    assert rows.is_cuda and np.array_equal(rows.cpu().numpy(), np.array([w[1] for w in want], np.float32))


# ---------------------------------------------------------------- 8. refusals
def test_refusals(monkeypatch):
    from centerpose_amd._lib import CenterposeHipError
    det = _det(TEST__FLIP_TEST=True, **FIX)
    good = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    cases = [("cpu", [torch.zeros((8, 8, 3), dtype=torch.uint8)], {}),
             ("uint8", [good.float()], {}),
             ("3 or 4 channels", [torch.zeros((8, 8, 2), dtype=torch.uint8, device="cuda")], {}),
             ("3 or 4 channels", [good], dict(layout="chw")),
             ("mixed", [good, np.zeros((8, 8, 3), np.uint8)], {}),
             ("unknown layout", [good], dict(layout="nhwc")),
             ("unknown color", [good], dict(color="yuv"))]
    for match, frames, kw in cases:
        with pytest.raises(CenterposeHipError, match=match):
            det.pre_process_batch(frames, 1, **kw)
        with pytest.raises(CenterposeHipError, match=match):
            det.run_batch(frames, **kw)
        if len(frames) == 1:
            with pytest.raises(CenterposeHipError, match=match):
                det.pre_process(frames[0], 1, **kw)
    # a tensor on another device than the model: the model is said to live on a second card
    assert good.device == det._model_device()
    monkeypatch.setattr(det, "_model_device", lambda: torch.device("cuda", good.device.index + 1))
    for call in (lambda: det.pre_process(good, 1), lambda: det.pre_process_batch([good], 1), lambda: det.run_batch([good]), lambda: det.run(good)):
        with pytest.raises(CenterposeHipError, match="the model is on cuda:%d" % (good.device.index + 1)):
            call()


@pytest.mark.parametrize("fields,message", [(dict(base=0), b"null base"), (dict(row_stride=-24), b"negative"), (dict(pix_stride=-3), b"negative")])
def test_bad_descriptor_through_ctypes_launches_nothing(fields, message):
    from centerpose_amd import _lib, detector
    L = _lib.lib()
    frame = torch.full((8, 8, 3), 200, dtype=torch.uint8, device="cuda")
    out = torch.full((2, 3, 8, 8), -7.0, device="cuda")
    table = np.zeros(2, detector.FRAME_DESC)
    for n in range(2):
        d = table[n]
        d["base"], d["row_stride"], d["pix_stride"], d["ch_off"], d["mid_off"] = frame.data_ptr(), 24, 3, (0, 1, 2), -1
        d["H"], d["W"], d["NH"], d["NW"], d["mi"], d["slot"] = 8, 8, 8, 8, (1, 0, 0, 0, 1, 0), n
    mean, std = (ctypes.c_float * 3)(0.4, 0.4, 0.4), (ctypes.c_float * 3)(0.3, 0.3, 0.3)

    def call():
        dev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).cuda()
        rc = L.cp_preprocess_frames_u8_f32(ctypes.c_void_p(dev.data_ptr()), table.ctypes.data_as(ctypes.c_void_p), 2, None, ctypes.c_size_t(0),
                                           ctypes.c_void_p(out.data_ptr()), 2, 8, 8, mean, std, 0, _lib.stream())
        torch.cuda.synchronize()
        return rc

    for k, v in fields.items():
        table[1][k] = v                                      # the SECOND descriptor is bad: the first must not have been launched either
    assert call() == 1 and message in L.cp_last_error()
    assert bool((out == -7.0).all())
    for k in fields:
        table[1][k] = table[0][k]
    assert call() == 0                                       # the same call with the descriptor mended runs
    want = np.float32((np.float64(200) / 255.0 - np.float64(np.float32(0.4))) / np.float64(np.float32(0.3)))
    assert bool((out == float(want)).all())
