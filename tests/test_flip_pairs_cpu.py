"""CPU: the batched flip test's host side -- the launch-function id shared by ops.py and the C plan runtime, the argument marshalling
of cp_flip_merge_pairs_f32, the new C-ABI symbols, the argument checks of Engine(flip_test=True) and the detector's routing of
FLIP_TEST batches (recording stand-ins for the device code)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flip_pairs_fn_id_matches_the_plan_runtime_enum():
    from centerpose_amd import ops
    src = open(os.path.join(ROOT, "centerpose_amd", "csrc", "plan_runtime.cpp")).read()
    body = re.search(r"enum \{ (FN_CONV = 1.*?)\};", src, re.S).group(1)
    enum = {n: int(v) for n, v in re.findall(r"(FN_[A-Z0-9]+) = (\d+)", body)}
    assert ops.FN_IDS["cp_flip_merge_pairs_f32"] == enum["FN_FLIPPAIRS"] == 20
    assert sorted(ops.FN_IDS.values()) == list(range(1, len(enum) + 1))
    assert len(re.findall(r"case FN_FLIPPAIRS:", src)) == 2


def test_flip_pairs_marshal_order():
    from centerpose_amd import ops
    ptrs = [ctypes.c_void_p(100 + i) for i in range(10)]
    ints = [3, 4, 32, 48, 17, 2, 0, 34, 2, 2, 3, 0, 0]
    args = ops.marshal("cp_flip_merge_pairs_f32", None, ptrs, ints)
    # cp_flip_merge_pairs_f32(n, in[4], out[4], meta[8], N, H, W, J, perm, stream)
    assert args[0] == 3
    assert list(args[1]) == [100, 101, 102, 103] and list(args[2]) == [104, 105, 106, 107]
    assert list(args[3]) == ints[5:13]
    assert args[4:8] == [4, 32, 48, 17] and args[8] is ptrs[8] and len(args) == 9


def test_flip_pairs_symbols_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from centerpose_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "centerpose_hip.h")).read()
    for sym in ("cp_flip_merge_pairs_f32", "cp_plan_flip_test"):
        assert re.search(r"\b%s\s*\(" % sym, hdr) and hasattr(L, sym)
    assert L.cp_plan_flip_test(None) == -1
    assert L.cp_abi_version() == 4


def test_engine_flip_test_argument_checks():
    from centerpose_amd import engine
    with pytest.raises(ValueError, match="even batch"):
        engine.Engine("dla_34", {}, 3, 128, 128, decode_k=100, flip_test=True)
    with pytest.raises(ValueError, match="decode_k"):
        engine.Engine("dla_34", {}, 4, 128, 128, flip_test=True)
    with pytest.raises(ValueError, match="dets_only"):
        engine.Engine("dla_34", {}, 4, 128, 128, decode_k=100, flip_test=True, dets_only=True)


class _RecordingModel:
    """model stand-in: `process` (the one-replay path) and `__call__` (the two-stage path's forward) record their calls."""

    def __init__(self):
        self.calls = []

    def process(self, x, K=100, **kw):
        self.calls.append(("process", tuple(x.shape), K, kw))
        return ["outs"], torch.zeros((x.shape[0] // 2, K, 56))

    def __call__(self, x):
        self.calls.append(("forward", tuple(x.shape)))
        return [torch.zeros((x.shape[0], c, 4, 4)) for c in (1, 2, 34, 2, 17, 2)]


def _detector(monkeypatch, **overrides):
    from centerpose_amd import config, detector
    det = object.__new__(detector.MultiPoseDetector)
    det.cfg = config.get_cfg("dla_34", **overrides)
    det.model = _RecordingModel()
    merged = []
    monkeypatch.setattr(det, "_flip_merge", lambda t, mode: merged.append(mode) or t[0:1], raising=False)
    monkeypatch.setattr(detector, "multi_pose_decode", lambda *a, **k: "two-stage dets")
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    return det, merged


def test_detector_flip_test_takes_one_replay(monkeypatch):
    det, merged = _detector(monkeypatch)
    assert det.cfg.TEST.FLIP_TEST and det.cfg.TEST.TOPK == 100
    outs, dets = det.process(torch.zeros((4, 3, 16, 16)))
    assert det.model.calls == [("process", (4, 3, 16, 16), 100, {"flip_test": True})]
    assert dets.shape == (2, 100, 56) and merged == []
    # process_stream under FLIP_TEST: process per batch, so every batch of pairs is one replay
    det.model.calls.clear()
    got = list(det.process_stream([torch.zeros((2, 3, 16, 16)), torch.zeros((6, 3, 16, 16))], depth=2))
    assert len(got) == 2 and [c[1][0] for c in det.model.calls] == [2, 6]
    assert all(c[0] == "process" and c[3] == {"flip_test": True} for c in det.model.calls)


def test_detector_flip_test_two_stage_paths(monkeypatch):
    # return_time=True: run()'s 'net' / 'dec' timers keep the two-stage path
    det, merged = _detector(monkeypatch)
    outputs, dets, t = det.process(torch.zeros((2, 3, 16, 16)), return_time=True)
    assert det.model.calls == [("forward", (2, 3, 16, 16))] and dets == "two-stage dets" and t > 0
    assert merged == [0, 0, 2, 1]
    # a head gated off by cfg.LOSS: the two-stage path as well
    det, merged = _detector(monkeypatch, LOSS__REG_OFFSET=False)
    det.process(torch.zeros((2, 3, 16, 16)))
    assert det.model.calls == [("forward", (2, 3, 16, 16))] and merged == [0, 0, 2, 1]
    # FLIP_TEST off: the non-flip one-replay path, no flip_test argument
    det, merged = _detector(monkeypatch, TEST__FLIP_TEST=False)
    det.process(torch.zeros((2, 3, 16, 16)))
    assert det.model.calls == [("process", (2, 3, 16, 16), 100, {})]


@pytest.mark.parametrize("B", [1, 3, 5])
def test_detector_flip_test_odd_batch_raises(monkeypatch, B):
    det, _ = _detector(monkeypatch)
    with pytest.raises(ValueError, match="pairs"):
        det.process(torch.zeros((B, 3, 16, 16)))
    assert det.model.calls == []


def test_flip_plan_replaces_the_forward_plan_of_its_shape(monkeypatch):
    """model.engine_for(..., flip_test=True): the flip-test plan holds the forward-only plan of its shape, so it replaces it in the
    cache and model.forward at that shape replays it (one plan per shape, whether run() or process() came first)."""
    from centerpose_amd import config, engine, model
    cfg = config.get_cfg("dla_34")
    m = model.create_model(cfg.MODEL.NAME, cfg.MODEL.HEAD_CONV, cfg)
    built = []

    class FakeEngine:
        def __init__(self, arch, sd, B, H, W, **kw):
            self.key = (B, H, W, kw.get("decode_k"), kw.get("flip_test", False))
            built.append(self.key)

        def __call__(self, x):
            return self.key

    monkeypatch.setattr(engine, "Engine", FakeEngine)
    x = torch.zeros((2, 3, 8, 8))
    assert m(x) == (2, 8, 8, None, False)
    m.engine_for(2, 8, 8, decode_k=100, flip_test=True)
    assert list(m._engines) == [(2, 8, 8, 100, "flip")]
    assert m(x) == (2, 8, 8, 100, True) and len(built) == 2          # forward replays the flip plan, nothing new is compiled
    assert m(torch.zeros((4, 3, 8, 8))) == (4, 8, 8, None, False)    # another shape: its own forward-only plan
