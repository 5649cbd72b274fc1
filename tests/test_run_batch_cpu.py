"""CPU: run_batch's host side -- grouping by network input shape, the staging layout and the descriptor table of a mixed-size list, one
`process` per (group, scale), the pair-by-pair route of the gated-head configuration, input validation -- with recording stand-ins
for the device code; and the new C-ABI symbols."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import prepost_np as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 100


def _img(seed, h, w):
    return (np.random.RandomState(seed).rand(h, w, 3) * 255).astype(np.uint8)


class _FakeStaging:
    """_Staging without a device: `upload` returns a host copy of what was staged."""

    def __init__(self, log, name):
        self.log, self.name, self.buf = log, name, None

    def host(self, nbytes):
        self.buf = np.zeros(nbytes, np.uint8)
        return self.buf

    def upload(self, nbytes):
        self.log.append(("upload", self.name, int(nbytes)))
        return torch.from_numpy(self.buf[:nbytes].copy())


def _detector(monkeypatch, arch="dla_34", **overrides):
    """A MultiPoseDetector without a model or a device: the launches record their arguments; `process` returns dets whose element
    [n, :, 0] is the image's first pixel, so that the order of the results can be followed."""
    import __graft_entry__ as g
    g.build()                                              # cp_invert_warp is host code of the library
    from centerpose_amd import config, detector
    det = object.__new__(detector.MultiPoseDetector)
    det.cfg = config.get_cfg(arch, **overrides)
    det.scales = det.cfg.TEST.TEST_SCALES
    det.num_classes = 1
    det.model = type("Model", (), {"process": None})()     # "has the one-replay process()"; never called: det.process is a stand-in
    det.mean = np.array(det.cfg.DATASET.MEAN, dtype=np.float32).reshape(1, 1, 3)
    det.std = np.array(det.cfg.DATASET.STD, dtype=np.float32).reshape(1, 1, 3)
    log = []
    det._io.buffers.update(images=_FakeStaging(log, "images"), table=_FakeStaging(log, "table"))
    nb = 2 if det.cfg.TEST.FLIP_TEST else 1

    def launch_pre(staging, table_dev, table, scratch_bytes, inp_h, inp_w):
        assert np.array_equal(table_dev.numpy(), np.ascontiguousarray(table).view(np.uint8).reshape(-1))
        log.append(("pre", table.copy(), scratch_bytes, inp_h, inp_w))
        x = torch.zeros((nb * len(table), 3, 2, 2))
        for j, d in enumerate(table):
            x[nb * j:nb * j + nb] = float(staging[int(d["src_off"])])
        return x

    def process(images, return_time=False, dets_only=False):
        log.append(("process", tuple(images.shape)))
        return ["outs"], images[::nb, 0, 0, 0].reshape(-1, 1, 1).repeat(1, K, 56).clone()

    def launch_post(dets, inv_dev, scale):
        log.append(("post", tuple(dets.shape), inv_dev.numpy().copy(), scale))
        return dets + 0

    def merge(detections):
        log.append(("merge", [tuple(d.shape) for d in detections]))
        return torch.cat(list(detections), 1)

    monkeypatch.setattr(det, "_launch_pre", launch_pre, raising=False)
    monkeypatch.setattr(det, "process", process, raising=False)
    monkeypatch.setattr(det, "_launch_post", launch_post, raising=False)
    monkeypatch.setattr(det, "merge_outputs_batch", merge, raising=False)
    return det, log


SIZES = [(96, 128), (217, 333), (96, 128), (100, 130), (217, 333)]        # (100, 130) pads to the input shape of (96, 128)


def test_new_symbols_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from centerpose_amd import _lib, detector
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "centerpose_hip.h")).read()
    for sym in ("cp_preprocess_batch_u8_f32", "cp_post_merge_batch_f32", "cp_invert_warp", "cp_sizeof_pre_desc", "cp_post_merge_max_rows"):
        assert re.search(r"\b%s\s*\(" % sym, hdr) and hasattr(L, sym)
    assert L.cp_sizeof_pre_desc() == detector.PRE_DESC.itemsize == 88
    assert L.cp_post_merge_max_rows() == 512
    assert L.cp_abi_version() == 4
    # the argument checks come before any launch: no device is needed to see them
    assert L.cp_post_merge_batch_f32(5, None, None, None, 1, 1, None, None, 0) != 0
    assert b"scales" in L.cp_last_error()


def test_invert_warp_is_the_per_image_inversion():
    from centerpose_amd import detector
    from centerpose_amd.post_process import get_affine_transform
    for c, s, out in (([320, 240], 640.0, [512, 512]), ([100.5, 77], [672, 512], [672, 512]), ([160, 120], [320., 256.], [128, 96])):
        M = get_affine_transform(np.array(c, np.float32), s, 0, out)
        assert np.array_equal(detector.invert_warp(M).reshape(2, 3), pp.invert_affine(np.asarray(M, np.float64)))


def test_groups_by_input_shape_and_results_in_input_order(monkeypatch):
    det, log = _detector(monkeypatch, "dla_34")
    assert not det.cfg.TEST.FIX_RES and det.cfg.TEST.FLIP_TEST
    assert det._batch_groups(SIZES) == [[0, 2, 3], [1, 4]]
    images = [_img(i, h, w) for i, (h, w) in enumerate(SIZES)]
    for i, im in enumerate(images):
        im[0, 0, 0] = 10 * (i + 1)
    res = det.run_batch(images)
    assert [r[1][0][0] for r in res] == [10.0, 20.0, 30.0, 40.0, 50.0]
    assert all(set(r) == {1} and len(r[1]) == K and len(r[1][0]) == 56 for r in res)
    # one upload of the images and one of the tables; one process per (group, scale)
    assert [e[:2] for e in log if e[0] == "upload"] == [("upload", "images"), ("upload", "table")]
    assert log[0][2] == sum(h * w * 3 for h, w in SIZES)
    assert [e[1] for e in log if e[0] == "process"] == [(6, 3, 2, 2), (4, 3, 2, 2)]
    assert [e[0] for e in log if e[0] != "upload"] == ["pre", "process", "post", "merge"] * 2
    # FIX_RES: every size in one group
    det, log = _detector(monkeypatch, "dla_34", TEST__FIX_RES=True)
    assert det._batch_groups(SIZES) == [[0, 1, 2, 3, 4]]
    det.run_batch(images)
    assert [e[1] for e in log if e[0] == "process"] == [(10, 3, 2, 2)]


def test_descriptor_table_of_a_mixed_size_list(monkeypatch):
    from centerpose_amd import detector
    from centerpose_amd.post_process import get_affine_transform
    det, log = _detector(monkeypatch, "hrnet")
    assert det.scales == [1, 2] and det.cfg.TEST.FLIP_TEST
    images = [_img(i, h, w) for i, (h, w) in enumerate(SIZES)]
    det.run_batch(images)
    offsets = np.cumsum([0] + [h * w * 3 for h, w in SIZES])
    pres = [e for e in log if e[0] == "pre"]
    posts = [e for e in log if e[0] == "post"]
    assert len(pres) == len(posts) == 4 and [e[1] for e in log if e[0] == "merge"] == [[(3, K, 56)] * 2, [(2, K, 56)] * 2]
    expect = [([0, 2, 3], 1), ([0, 2, 3], 2), ([1, 4], 1), ([1, 4], 2)]
    for (_, table, scratch, inp_h, inp_w), (_, dshape, inv, pscale), (idx, scale) in zip(pres, posts, expect):
        assert table.dtype == detector.PRE_DESC and len(table) == len(idx) and pscale == scale
        mid = 0
        for j, i in enumerate(idx):
            h, w = SIZES[i]
            # what pre_process computes for this image
            new_h, new_w, ih, iw, c, s = det.input_geometry(h, w, scale)
            ref, rmeta = pp.pre_process(images[i], scale, det.cfg.DATASET.MEAN, det.cfg.DATASET.STD, fix_res=False, flip_test=True)
            assert (inp_h, inp_w) == (ih, iw) == ref.shape[2:]
            d = table[j]
            assert (d["src_off"], d["H"], d["W"], d["NH"], d["NW"], d["slot"]) == (offsets[i], h, w, new_h, new_w, 2 * j)
            M = np.asarray(get_affine_transform(c, s, 0, [iw, ih]), np.float64)
            assert np.array_equal(d["mi"].reshape(2, 3), pp.invert_affine(M))
            if scale == 1:
                assert d["mid_off"] == -1
            else:
                assert d["mid_off"] == mid
                mid += new_h * new_w * 3
            want_inv = get_affine_transform(rmeta["c"], rmeta["s"], 0, (rmeta["out_width"], rmeta["out_height"]), inv=1)
            assert np.array_equal(inv[0, j], np.asarray(want_inv, np.float64).reshape(6))
        assert scratch == mid and dshape == (len(idx), K, 56)


def test_pre_process_batch_table_and_metas(monkeypatch):
    det, log = _detector(monkeypatch, "res_50")
    assert det.cfg.TEST.FIX_RES
    images = [_img(i, h, w) for i, (h, w) in enumerate(SIZES)]
    x, metas = det.pre_process_batch(images, 0.5)
    assert x.shape[0] == 10 and len(metas) == 5
    table = [e for e in log if e[0] == "pre"][0][1]
    assert table["slot"].tolist() == [0, 2, 4, 6, 8] and (table["mid_off"] >= 0).all()
    for im, m in zip(images, metas):
        _, rmeta = pp.pre_process(im, 0.5, det.cfg.DATASET.MEAN, det.cfg.DATASET.STD, fix_res=True, flip_test=True)
        assert set(m) == set(rmeta) and all(np.array_equal(np.asarray(m[k]), np.asarray(rmeta[k])) for k in rmeta)
    from centerpose_amd._lib import CenterposeHipError
    det, _ = _detector(monkeypatch, "dla_34")
    with pytest.raises(CenterposeHipError, match="input shape"):
        det.pre_process_batch(images, 1)


def test_gated_head_goes_pair_by_pair(monkeypatch):
    det, log = _detector(monkeypatch, "dla_34", LOSS__REG_OFFSET=False, TEST__FIX_RES=True)
    assert det.cfg.TEST.FLIP_TEST and not det._flip_replay_path()
    images = [_img(i, h, w) for i, (h, w) in enumerate(SIZES[:3])]
    for i, im in enumerate(images):
        im[0, 0, 0] = 10 * (i + 1)
    res = det.run_batch(images)
    assert [e[1] for e in log if e[0] == "process"] == [(2, 3, 2, 2)] * 3
    assert [e[0] for e in log if e[0] != "upload"] == ["pre", "process", "process", "process", "post", "merge"]
    assert [r[1][0][0] for r in res] == [10.0, 20.0, 30.0]
    # FLIP_TEST off with a gated head: the two-stage path takes any batch
    det, log = _detector(monkeypatch, "dla_34", LOSS__REG_OFFSET=False, TEST__FIX_RES=True, TEST__FLIP_TEST=False)
    det.run_batch(images)
    assert [e[1] for e in log if e[0] == "process"] == [(3, 3, 2, 2)]


def test_empty_list_and_bad_images(monkeypatch):
    from centerpose_amd._lib import CenterposeHipError
    det, log = _detector(monkeypatch, "dla_34")
    assert det.run_batch([]) == [] and log == []
    for bad in (np.zeros((10, 10, 3), np.float32), np.zeros((10, 10), np.uint8), np.zeros((10, 10, 4), np.uint8), "image.jpg"):
        with pytest.raises(CenterposeHipError):
            det.run_batch([_img(0, 8, 8), bad])
        with pytest.raises(CenterposeHipError):
            det.pre_process_batch([bad], 1)
    assert log == []


def test_merge_outputs_batch_routing(monkeypatch):
    from centerpose_amd import config, detector
    calls = []
    monkeypatch.setattr(detector, "post_merge_batch", lambda dets, **kw: (calls.append((len(dets), kw)) or "merged", None))
    det = object.__new__(detector.MultiPoseDetector)
    rows = torch.zeros((2, K, 56))
    det.cfg = config.get_cfg("res_50")                      # no NMS, one scale: the rows as they are, no launch
    assert det.merge_outputs_batch([rows]) is rows and calls == []
    det.cfg = config.get_cfg("dla_34")                      # TEST.NMS
    assert det.merge_outputs_batch([rows]) == "merged" and calls.pop() == (1, dict(nms=True, Nt=0.5, method=2))
    det.cfg = config.get_cfg("hrnet")                       # two scales
    assert det.merge_outputs_batch([rows, rows]) == "merged" and calls.pop() == (2, dict(nms=True, Nt=0.5, method=2))
