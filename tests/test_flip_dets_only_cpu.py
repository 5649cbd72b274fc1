"""CPU: detections-only inference under the flip test, host side -- the launch-function id of cp_head_points_pairs_f32 shared by ops.py
and the C plan runtime, its argument marshalling, the new C-ABI symbol, the argument checks of Engine(flip_dets_only=True) and the
routing of MultiPoseDetector.process_dets / run_batch(dets_only=True) (recording stand-ins for the device code)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 100


def test_points_pairs_fn_id_matches_the_plan_runtime_enum():
    from centerpose_amd import ops
    src = open(os.path.join(ROOT, "centerpose_amd", "csrc", "plan_runtime.cpp")).read()
    body = re.search(r"enum \{ (FN_CONV = 1.*?)\};", src, re.S).group(1)
    enum = {n: int(v) for n, v in re.findall(r"(FN_[A-Z0-9]+) = (\d+)", body)}
    assert ops.FN_IDS["cp_head_points_pairs_f32"] == enum["FN_POINTSPAIRS"] == 21
    assert len(re.findall(r"case FN_POINTSPAIRS:", src)) == 2


def test_points_pairs_symbol_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from centerpose_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "centerpose_hip.h")).read()
    assert re.search(r"\bcp_head_points_pairs_f32\s*\(", hdr) and hasattr(L, "cp_head_points_pairs_f32")
    assert L.cp_abi_version() == 4


def test_points_pairs_marshal_order():
    from centerpose_amd import ops
    ptrs = [ctypes.c_void_p(100 + i) for i in range(8)]
    ints = [64, 2, 16, 16, 64, 17, 100, 256]
    args = ops.marshal("cp_head_points_pairs_f32", None, ptrs, ints)
    # cp_head_points_pairs_f32(feat, featLd, ws_inds, perm, w1, b1, w2, b2, out, N, H, W, C, J, K, hc, stream)
    assert args[0] is ptrs[0] and args[1] == 64 and args[2:9] == ptrs[1:] and args[9:] == ints[1:] and len(args) == 16


def test_engine_flip_dets_only_argument_checks():
    from centerpose_amd import engine
    with pytest.raises(ValueError, match="even batch"):
        engine.Engine("dla_34", {}, 3, 128, 128, decode_k=100, flip_dets_only=True)
    with pytest.raises(ValueError, match="decode_k"):
        engine.Engine("dla_34", {}, 4, 128, 128, flip_dets_only=True)
    with pytest.raises(ValueError):
        engine.Engine("dla_34", {}, 4, 128, 128, decode_k=100, flip_dets_only=True, flip_test=True)
    with pytest.raises(ValueError):
        engine.Engine("dla_34", {}, 4, 128, 128, decode_k=100, flip_dets_only=True, dets_only=True)


class _RecordingModel:
    """model stand-in: `process` (the one-replay path) and `__call__` (the two-stage path's forward) record their calls."""

    def __init__(self, flip):
        self.calls, self.flip = [], flip

    def process(self, x, K=100, **kw):
        self.calls.append(("process", tuple(x.shape), K, kw))
        return ["outs"], torch.zeros((x.shape[0] // 2 if self.flip else x.shape[0], K, 56))

    def __call__(self, x):
        self.calls.append(("forward", tuple(x.shape)))
        return [torch.zeros((x.shape[0], c, 4, 4)) for c in (1, 2, 34, 2, 17, 2)]


def _detector(**overrides):
    from centerpose_amd import config, detector
    det = object.__new__(detector.MultiPoseDetector)
    det.cfg = config.get_cfg("dla_34", **overrides)
    det.model = _RecordingModel(det.cfg.TEST.FLIP_TEST)
    return det


def test_process_dets_under_flip_test_takes_the_new_plan():
    det = _detector()
    assert det.cfg.TEST.FLIP_TEST and det.cfg.TEST.TOPK == 100
    dets = det.process_dets(torch.zeros((4, 3, 16, 16)))
    assert det.model.calls == [("process", (4, 3, 16, 16), 100, {"flip_dets_only": True})]
    assert torch.is_tensor(dets) and dets.shape == (2, 100, 56)


def test_process_dets_without_flip_test_takes_the_dets_only_plan():
    det = _detector(TEST__FLIP_TEST=False)
    dets = det.process_dets(torch.zeros((3, 3, 16, 16)))
    assert det.model.calls == [("process", (3, 3, 16, 16), 100, {"dets_only": True})]
    assert dets.shape == (3, 100, 56)


@pytest.mark.parametrize("B", [1, 3, 5])
def test_process_dets_odd_batch_raises(B):
    det = _detector()
    with pytest.raises(ValueError, match="pairs"):
        det.process_dets(torch.zeros((B, 3, 16, 16)))
    assert det.model.calls == []


@pytest.mark.parametrize("flip", [True, False])
def test_process_dets_gated_head_raises(flip):
    det = _detector(TEST__FLIP_TEST=flip, LOSS__REG_OFFSET=False)
    with pytest.raises(ValueError):
        det.process_dets(torch.zeros((2, 3, 16, 16)))
    assert det.model.calls == []


def test_process_refusal_points_at_process_dets():
    det = _detector()
    with pytest.raises(ValueError, match="FLIP_TEST") as e:
        det.process(torch.zeros((2, 3, 16, 16)), dets_only=True)
    assert "process_dets" in str(e.value) and "run_batch" in str(e.value)
    assert det.model.calls == []


def test_engine_for_flip_dets_only_has_its_own_key_and_keeps_the_forward_plan(monkeypatch):
    from centerpose_amd import config, engine, model
    cfg = config.get_cfg("dla_34")
    m = model.create_model(cfg.MODEL.NAME, cfg.MODEL.HEAD_CONV, cfg)
    built = []

    class FakeEngine:
        def __init__(self, arch, sd, B, H, W, **kw):
            self.key = (B, H, W, kw.get("decode_k"), kw.get("flip_test", False), kw.get("flip_dets_only", False), kw.get("dets_only", False))
            built.append(self.key)

        def __call__(self, x):
            return self.key

    monkeypatch.setattr(engine, "Engine", FakeEngine)
    x = torch.zeros((2, 3, 8, 8))
    assert m(x) == (2, 8, 8, None, False, False, False)
    a = m.engine_for(2, 8, 8, decode_k=100, flip_dets_only=True)
    assert a.key == (2, 8, 8, 100, False, True, False)
    assert (2, 8, 8) in m._engines and len(m._engines) == 2          # the forward-only plan of the shape stays
    assert m(x) == (2, 8, 8, None, False, False, False) and len(built) == 2
    assert m.engine_for(2, 8, 8, decode_k=100, flip_dets_only=True) is a and len(built) == 2
    # its key is neither the flip-test plan's nor the detections-only plan's
    m.engine_for(2, 8, 8, decode_k=100, flip_test=True)
    m.engine_for(2, 8, 8, decode_k=100, dets_only=True)
    assert len(built) == 4 and m.engine_for(2, 8, 8, decode_k=100, flip_dets_only=True) is a
    # default calls pass no new keyword
    assert built[0] == (2, 8, 8, None, False, False, False)


class _FakeStaging:
    def __init__(self):
        self.buf = None

    def host(self, nbytes):
        self.buf = np.zeros(nbytes, np.uint8)
        return self.buf

    def upload(self, nbytes):
        return torch.from_numpy(self.buf[:nbytes].copy())


def _batch_detector(monkeypatch, arch):
    """A MultiPoseDetector without a model or a device for run_batch: the stages record their calls."""
    import __graft_entry__ as g
    g.build()                                              # cp_invert_warp is host code of the library
    from centerpose_amd import config, detector
    det = object.__new__(detector.MultiPoseDetector)
    det.cfg = config.get_cfg(arch)
    det.scales = det.cfg.TEST.TEST_SCALES
    det.num_classes = 1
    det.mean = np.array(det.cfg.DATASET.MEAN, dtype=np.float32).reshape(1, 1, 3)
    det.std = np.array(det.cfg.DATASET.STD, dtype=np.float32).reshape(1, 1, 3)
    det._staging_buffers = {"images": _FakeStaging(), "table": _FakeStaging()}
    nb = 2 if det.cfg.TEST.FLIP_TEST else 1
    log = []

    def process(images, return_time=False, dets_only=False):
        log.append(("process", tuple(images.shape), dets_only))
        return ["outs"], torch.zeros((images.shape[0] // nb, K, 56))

    def process_dets(images):
        log.append(("process_dets", tuple(images.shape)))
        return torch.ones((images.shape[0] // nb, K, 56))

    monkeypatch.setattr(det, "_launch_pre", lambda staging, table_dev, table, sb, h, w: torch.zeros((nb * len(table), 3, 2, 2)), raising=False)
    monkeypatch.setattr(det, "process", process, raising=False)
    monkeypatch.setattr(det, "process_dets", process_dets, raising=False)
    monkeypatch.setattr(det, "_launch_post", lambda dets, inv_dev, scale: dets + 0, raising=False)
    monkeypatch.setattr(det, "merge_outputs_batch", lambda detections: torch.cat(list(detections), 1), raising=False)
    det.model = type("Model", (), {"process": None})()
    return det, log


SIZES = [(96, 128), (217, 333), (96, 128), (100, 130), (217, 333)]        # (100, 130) pads to the input shape of (96, 128)


@pytest.mark.parametrize("arch", ["dla_34", "hrnet"])
def test_run_batch_dets_only_reaches_process_dets_once_per_group_and_scale(monkeypatch, arch):
    det, log = _batch_detector(monkeypatch, arch)
    assert det.cfg.TEST.FLIP_TEST and not det.cfg.TEST.FIX_RES
    S = len(det.scales)
    images = [(np.random.RandomState(i).rand(h, w, 3) * 255).astype(np.uint8) for i, (h, w) in enumerate(SIZES)]
    res = det.run_batch(images, dets_only=True)
    assert [e[0] for e in log] == ["process_dets"] * (2 * S)
    assert [e[1][0] for e in log] == [6] * S + [4] * S                    # groups [0, 2, 3] and [1, 4], as pairs
    assert len(res) == 5 and all(r[1][0][0] == 1.0 and len(r[1]) == S * K for r in res)
    log.clear()
    res = det.run_batch(images)
    assert [e[0] for e in log] == ["process"] * (2 * S) and all(e[2] is False for e in log)
    assert all(r[1][0][0] == 0.0 for r in res)
