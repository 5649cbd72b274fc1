"""CPU: the detections-only mode's host side -- launch-function ids shared by ops.py and the C plan runtime, the packed weight
order of cp_head_points_f32, its argument marshalling and the argument check of Engine(dets_only=True)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fn_ids_match_the_plan_runtime_enum():
    from centerpose_amd import ops
    src = open(os.path.join(ROOT, "centerpose_amd", "csrc", "plan_runtime.cpp")).read()
    body = re.search(r"enum \{ (FN_CONV = 1.*?)\};", src, re.S).group(1)
    enum = {n: int(v) for n, v in re.findall(r"(FN_[A-Z0-9]+) = (\d+)", body)}
    assert sorted(enum.values()) == sorted(ops.FN_IDS.values()) == list(range(1, len(enum) + 1))
    assert ops.FN_IDS["cp_head_points_f32"] == enum["FN_POINTS"] == 19
    # every id has a run_op case and an arity_ok case
    for name in enum:
        assert len(re.findall(r"case %s:" % name, src)) == 2, name


def test_new_symbols_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from centerpose_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "centerpose_hip.h")).read()
    for sym in ("cp_head_points_f32", "cp_plan_dets_only"):
        assert re.search(r"\b%s\s*\(" % sym, hdr) and hasattr(L, sym)
    assert L.cp_plan_dets_only(None) == -1
    assert L.cp_abi_version() == 4


def test_pack_head_points_weight_order():
    from centerpose_amd import ops
    hc, C = 64, 32
    w3 = torch.randn(hc, C, 3, 3)
    packed = ops.pack_head_points_weight(w3).view(9 * C // 8, 2, hc, 4)
    wk = w3.permute(2, 3, 1, 0).reshape(9 * C, hc)            # k = (ky*3 + kx)*C + c
    for kb, h, n, s in ((0, 0, 0, 0), (3, 1, 17, 2), (9 * C // 8 - 1, 1, hc - 1, 3), (20, 0, 40, 1)):
        assert packed[kb, h, n, s] == wk[8 * kb + 4 * h + s, n]
    assert torch.equal(packed.permute(0, 1, 3, 2).reshape(9 * C, hc), wk)


def test_head_points_marshal_order():
    from centerpose_amd import ops
    ptrs = [ctypes.c_void_p(100 + i) for i in range(7)]
    ints = [64, 2, 16, 16, 64, 17, 100, 256]
    args = ops.marshal("cp_head_points_f32", None, ptrs, ints)
    # cp_head_points_f32(feat, featLd, ws_inds, w1, b1, w2, b2, out, B, H, W, C, J, K, hc, stream)
    assert args[0] is ptrs[0] and args[1] == 64 and args[2:8] == ptrs[1:] and args[8:] == ints[1:]


def test_engine_dets_only_needs_decode_k():
    from centerpose_amd import engine
    with pytest.raises(ValueError, match="decode_k"):
        engine.Engine("dla_34", {}, 1, 128, 128, dets_only=True)
