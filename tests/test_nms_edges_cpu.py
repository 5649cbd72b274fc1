"""CPU: soft_nms_39 at exact ties and limits -- the host C++ (csrc/host_nms.cpp) and the oracle's C restatement against vectors
produced by the reference's own source (tests/golden/soft_nms_39_edges.npz, make_golden_nms.py::edge_cases), all 56 columns and
`keep` bit for bit: every case is exact arithmetic (integer corners, dyadic scores, no Gaussian decay that changes a score)."""
import os
import sys

import numpy as np
import pytest


def _edge_golden(golden_dir):
    sys.path.insert(0, golden_dir)
    import make_golden_nms as mg
    return mg.edge_cases(), np.load(os.path.join(golden_dir, "soft_nms_39_edges.npz"))


def count_decisions(boxes, sigma=0.5, Nt=0.3, threshold=0.001, method=0):
    """Instrumented restatement of the soft_nms_39 loop (lib/external/nms.pyx:172-275) in float32 -> (rows, N, counts) with how often
    an arg-max had equal top scores, ov == Nt, a decayed score == threshold, and the last row was discarded."""
    b = boxes.copy()
    f32, one = np.float32, np.float32(1)
    sigma, Nt, threshold = f32(sigma), f32(Nt), f32(threshold)
    N = b.shape[0]
    cnt = dict(argmax_tie=0, ov_eq_nt=0, decayed_eq_threshold=0, discard_last=0, discards=0, decays=0)
    for i in range(b.shape[0]):
        maxpos = i
        for pos in range(i + 1, N):
            if b[maxpos, 4] < b[pos, 4]:
                maxpos = pos
        if i < N and int((b[i:N, 4] == b[maxpos, 4]).sum()) > 1:
            cnt["argmax_tie"] += 1
        t = b[i, :39].copy(); b[i, :39] = b[maxpos, :39]; b[maxpos, :39] = t
        tx1, ty1, tx2, ty2 = b[i, :4]
        pos = i + 1
        while pos < N:
            x1, y1, x2, y2 = b[pos, :4]
            area = (x2 - x1 + one) * (y2 - y1 + one)
            iw = min(tx2, x2) - max(tx1, x1) + one
            if iw > 0:
                ih = min(ty2, y2) - max(ty1, y1) + one
                if ih > 0:
                    ov = iw * ih / ((tx2 - tx1 + one) * (ty2 - ty1 + one) + area - iw * ih)
                    cnt["ov_eq_nt"] += int(ov == Nt and method != 2)
                    if method == 1:
                        w = one - ov if ov > Nt else one
                    elif method == 2:
                        w = f32(np.exp(np.float64(-(ov * ov) / sigma)))
                    else:
                        w = f32(0) if ov > Nt else one
                    cnt["decays"] += int(w != one)
                    b[pos, 4] = w * b[pos, 4]
                    cnt["decayed_eq_threshold"] += int(b[pos, 4] == threshold)
                    if b[pos, 4] < threshold:
                        cnt["discards"] += 1
                        cnt["discard_last"] += int(pos == N - 1)
                        b[pos, :5] = b[N - 1, :5]
                        q = b[pos, 5:39].copy(); b[pos, 5:39] = b[N - 1, 5:39]; b[N - 1, 5:39] = q
                        N -= 1
                        pos -= 1
            pos += 1
    return b, N, cnt


def test_soft_nms_39_edge_cases_match_reference_source_golden(golden_dir):
    import __graft_entry__ as g
    g.build()
    from centerpose_amd.detector import soft_nms_39
    from oracle import dcn as odcn
    cases, gold = _edge_golden(golden_dir)
    assert len(cases) == 25
    for name, (boxes, kw) in cases.items():
        for fn in (soft_nms_39, odcn.soft_nms_39):
            work = boxes.copy()
            keep = fn(work, **kw)
            assert keep == gold[name + "__keep"].tolist(), name
            assert np.array_equal(work, gold[name + "__out"]), name              # all 56 columns, column 4 included


def test_soft_nms_39_edge_cases_hit_every_decision(golden_dir):
    """The set is a test of strictness only if the decisions occur: counted by an instrumented run that itself reproduces the golden."""
    cases, gold = _edge_golden(golden_dir)
    total = {}
    for name, (boxes, kw) in cases.items():
        out, N, cnt = count_decisions(boxes, **kw)
        assert np.array_equal(out, gold[name + "__out"]) and N == len(gold[name + "__keep"]), name
        if kw["method"] == 2:
            assert cnt["decays"] == 0, name                                      # method 2 only where no score changes
        for k, v in cnt.items():
            total[k] = total.get(k, 0) + v
        # integer corners: the IoU operands are exact
        assert np.array_equal(boxes[:, :4], np.round(boxes[:, :4]))
    print("soft-NMS decisions over the edge set:", total)
    for k in ("argmax_tie", "ov_eq_nt", "decayed_eq_threshold", "discard_last"):
        assert total[k] >= 1, k
    # what the named cases are for, each from its own instrumented run
    one = lambda name: count_decisions(cases[name][0], **cases[name][1])
    for m in (0, 1):
        out, N, cnt = one("iou_on_nt_m%d" % m)
        assert cnt["ov_eq_nt"] == 1 and 0.5 in out[:N, 4].tolist()               # IoU == Nt: weight 1, the 0.5 row keeps its score
    assert one("decay_on_threshold_m1")[2]["decayed_eq_threshold"] == 1 and one("decay_on_threshold_m1")[1] == 3
    assert one("decay_below_threshold_m1")[1] == 2 and one("decay_above_threshold_m1")[1] == 3
    assert one("decay_below_threshold_m1")[2]["decayed_eq_threshold"] == 0 == one("decay_above_threshold_m1")[2]["decayed_eq_threshold"]
    out, N, cnt = one("threshold_zero_m0")
    assert N == 6 and cnt["discards"] == 0 and cnt["decays"] >= 3 and cnt["decayed_eq_threshold"] >= 3 and (out[:, 4] == 0).sum() == 2 and cnt["argmax_tie"] >= 2
    assert one("discard_last_row")[2]["discard_last"] == 1
    assert one("discard_chain")[2]["discards"] == 4 and one("discard_chain")[1] == 3
    assert one("discard_all_but_first")[1] == 1 and one("discard_down_to_i_plus_1")[1] == 2
    out, N, cnt = one("equal_across_stride")
    assert [int(v) for v in out[:5, 5]] == [6, 70, 71, 18, 82]                   # lowest index first, within a lane and across lanes
    out, N, cnt = one("equal_three_first_stays")
    assert [int(v) for v in out[:3, 5]] == [1, 3, 4] and [int(v) for v in out[:3, 39]] == [1001, 1002, 1003]
    assert one("equal_65")[2]["argmax_tie"] >= 64
