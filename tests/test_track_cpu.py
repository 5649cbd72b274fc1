"""Track association without a GPU: the host twins of csrc/track_host.h against tests/track_ref.py, the assignment against scipy, the
association step of track.DeepSortTracker driven through the host twins over the reference's recorded run
(tests/golden/track_sequence.npz), the ring, the refusals and the symbols."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import track_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p
SYMBOLS = ("cp_track_cost_f32", "cp_track_append_f32", "cp_track_cost_host", "cp_track_append_host", "cp_linear_assignment_host")


def _L():
    from centerpose_amd import _lib
    return _lib.lib()


def _err():
    return _L().cp_last_error().decode()


# ---------------------------------------------------------------- 1. host twins against track_ref
def _case(seed, S, Tcap, budget, q, M, glens, holes=True):
    r = np.random.RandomState(seed)
    gallery = tr.f16_features(r, S * Tcap * budget).reshape(S * Tcap, budget, tr.DIM)
    glen = np.array([glens[i % len(glens)] for i in range(S * Tcap)], np.int32)
    ginv = np.zeros((S * Tcap, budget), np.float32)
    for t in range(S * Tcap):
        n = min(int(glen[t]), budget)
        ginv[t, :n] = (1.0 / np.sqrt((gallery[t, :n].astype(np.float64) ** 2).sum(1))).astype(np.float32)
        gallery[t, n:], ginv[t, n:] = np.nan, np.nan                    # rows >= glen must not reach the result
    features = tr.f16_features(r, S * q)
    slots = np.full(S * q, -1, np.int32)
    rows = r.uniform(0, 300, (S, M, 56)).astype(np.float32)
    for s in range(S):
        ms = r.permutation(M)
        for d in range(q):
            if d < M and not (holes and d % 3 == 1):                    # unused slots interleaved with used ones
                slots[s * q + d] = s * M + ms[d]
            else:
                features[s * q + d] = np.nan
    # make some detections close to a gallery row so that the min is not ~1 everywhere
    for s in range(S):
        for d in range(q):
            t = s * Tcap + d % Tcap
            if slots[s * q + d] >= 0 and glen[t] > 0:
                g = gallery[t, (d * 7) % min(int(glen[t]), budget)]
                features[s * q + d] = (np.round((g * 0.5 + 0.1 * features[s * q + d]) * 8) / 8).astype(np.float16).astype(np.float32)
    return gallery, ginv, glen, features, slots, rows


@pytest.mark.parametrize("S,Tcap,budget,q,M,glens", [(1, 1, 1, 1, 1, (1,)), (2, 3, 5, 4, 6, (0, 1, 5, 3, 9)), (1, 4, 33, 7, 9, (33, 32, 0, 2))])
def test_cost_host_twin_against_the_float64_statement(S, Tcap, budget, q, M, glens):
    gallery, ginv, glen, features, slots, rows = _case(5, S, Tcap, budget, q, M, glens)
    want_cost, want_det = tr.cost_det(gallery, glen, features, slots, rows, S, Tcap, budget, q)
    rc, cost, det = tr.host_cost(_L(), gallery, ginv, glen, features, slots, rows, S, Tcap, budget, q)
    assert rc == 0, _err()
    tr.assert_cost(cost, want_cost, "host twin %s" % ((S, Tcap, budget, q),))
    assert np.array_equal(det, want_det)
    assert float(want_cost[np.isfinite(want_cost)].min()) < 0.9           # a nearest neighbour: unrelated vectors sit at ~1


def test_append_host_twin_is_bit_exact_and_wraps():
    r = np.random.RandomState(2)
    budget, slots_n = 3, 4
    features = tr.f16_features(r, 6)
    g1, i1 = np.zeros((slots_n, budget, tr.DIM), np.float32), np.zeros((slots_n, budget), np.float32)
    g2, i2 = g1.copy(), i1.copy()
    count = [0] * slots_n
    for step in range(5):                                                   # slot 1 gets 5 features into a ring of 3: it wraps
        table = [(step % 6, 1, count[1] % budget), ((step + 2) % 6, 3, count[3] % budget)]
        if step == 2:
            table += [(-1, 0, 0), (0, 0, budget), (0, -1, 0)]               # entries that write nothing
        count[1] += 1
        count[3] += 1
        assert tr.host_append(_L(), g1, i1, features, table, budget) == 0, _err()
        tr.append(g2, i2, features, table, budget)
        assert g1.tobytes() == g2.tobytes() and i1.tobytes() == i2.tobytes()
    assert np.array_equal(g1[1], features[[3, 4, 2]]) and not g1[0].any() and not g1[2].any()
    assert tr.host_append(_L(), g1, i1, features, np.zeros((0, 3), np.int32), budget) == 0


# ---------------------------------------------------------------- 2. the assignment against scipy
def _assign(cost):
    from centerpose_amd import track
    return track.linear_assignment(cost)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (5, 5), (12, 31), (31, 12)])
def test_linear_assignment_equals_scipy(shape):
    from scipy.optimize import linear_sum_assignment
    for seed in range(4):
        r = np.random.RandomState(100 * shape[0] + shape[1] + seed)
        cost = r.uniform(0, 1, shape)                                       # continuous values: tie-free
        rr, cc = linear_sum_assignment(cost)
        got = _assign(cost)
        assert len(got) == min(shape) and got[:, 0].tolist() == sorted(got[:, 0].tolist())
        assert cost[got[:, 0], got[:, 1]].sum() == pytest.approx(cost[rr, cc].sum(), rel=1e-12, abs=0)
        assert sorted(map(tuple, got.tolist())) == sorted(zip(rr.tolist(), cc.tolist()))
        # thresholded as the tracker does it: the total is unique and so is the set of pairs below the threshold
        thr = 0.25
        capped = cost.copy()
        capped[capped > thr] = thr + 1e-5
        rr, cc = linear_sum_assignment(capped)
        got = _assign(capped)
        assert capped[got[:, 0], got[:, 1]].sum() == pytest.approx(capped[rr, cc].sum(), rel=1e-12, abs=0)
        below = {(a, b) for a, b in zip(rr.tolist(), cc.tolist()) if capped[a, b] <= thr}
        assert {(a, b) for a, b in got.tolist() if capped[a, b] <= thr} == below


def test_linear_assignment_on_every_recorded_matrix():
    g = tr.sequence()
    assert len(g["cm_index"]) > 40
    for f, s, kind, r, c, off, poff, npair in g["cm_index"].tolist():
        cost = g["cm_values"][off:off + r * c].reshape(r, c)
        thr = g["kw"]["max_iou_distance"] if kind else g["kw"]["max_cosine_distance"]
        want = {tuple(p) for p in g["cm_pairs"][poff:poff + npair].tolist() if cost[p[0], p[1]] <= thr}
        assert {tuple(p) for p in _assign(cost).tolist() if cost[p[0], p[1]] <= thr} == want, (f, s, kind)


def test_linear_assignment_refusals_and_strides():
    L = _L()
    out = np.zeros(4, np.int32)
    cost = np.arange(12, dtype=np.float64).reshape(3, 4)
    assert L.cp_linear_assignment_host(cost.ctypes.data_as(VP), 3, 4, 3, out.ctypes.data_as(VP)) == 1 and "ld" in _err()
    assert L.cp_linear_assignment_host(None, 3, 4, 4, out.ctypes.data_as(VP)) == 1 and "null" in _err()
    assert L.cp_linear_assignment_host(cost.ctypes.data_as(VP), -1, 4, 4, out.ctypes.data_as(VP)) == 1
    bad = cost.copy()
    bad[1, 2] = np.inf
    assert L.cp_linear_assignment_host(bad.ctypes.data_as(VP), 3, 4, 4, out.ctypes.data_as(VP)) == 1 and "finite" in _err()
    # a 3 x 2 block of a matrix with row stride 4
    block = np.array([[5, 1, 9, 9], [2, 8, 9, 9], [1, 0.5, 9, 9]], np.float64)
    assert L.cp_linear_assignment_host(block.ctypes.data_as(VP), 3, 2, 4, out.ctypes.data_as(VP)) == 0
    assert out[:3].tolist() == [1, -1, 0]                                    # 1 + 1 = 2 beats 1 + 2 = 3
    assert L.cp_linear_assignment_host(None, 0, 0, 0, None) == 0


# ---------------------------------------------------------------- 3. the association step over the recording, through the host twins
class HostGallery:
    """The device side of an update, on the host: cp_track_cost_host / cp_track_append_host over NumPy buffers."""

    def __init__(self, trk):
        self.trk = trk
        n = trk.streams * trk.max_tracks
        self.gallery = np.full((n, trk.budget, tr.DIM), np.nan, np.float32)       # unwritten ring rows must never be read
        self.ginv = np.full((n, trk.budget), np.nan, np.float32)

    def update(self, rows, features, slots, sizes):
        t = self.trk
        glen = t.begin()
        rc, cost, det = tr.host_cost(_L(), self.gallery, self.ginv, glen, features, slots, rows, t.streams, t.max_tracks, t.budget, t.q)
        assert rc == 0, _err()
        outs, table = t.associate(cost, det, sizes)
        assert tr.host_append(_L(), self.gallery, self.ginv, features, table, t.budget) == 0, _err()
        return outs


def test_association_over_the_recorded_sequence():
    from centerpose_amd import track
    g = tr.sequence()
    trk = track.DeepSortTracker(g["S"] * g["q"], streams=g["S"], device=None, **g["kw"])
    host = HostGallery(trk)
    sizes = [tuple(x) for x in g["sizes"].tolist()]
    for f in range(g["F"]):
        outs = host.update(*tr.frame_inputs(g, f), sizes)
        tr.check_frame(g, f, trk, outs)
    assert trk.dropped == [0, 0] and max(t.track_id for t in trk.tracks[0]) >= 5


# ---------------------------------------------------------------- 4. the ring, slot reuse, dropped
def _person_frame(q, M, boxes, feats):
    """One stream: detection slot d holds box / feature d."""
    rows = np.zeros((1, M, 56), np.float32)
    features = np.zeros((q, tr.DIM), np.float32)
    slots = np.full(q, -1, np.int32)
    for d, (b, f) in enumerate(zip(boxes, feats)):
        rows[0, d, :4], rows[0, d, 4] = b, 0.9 - 0.1 * d
        features[d], slots[d] = f, d
    return rows, features, slots


def test_ring_holds_the_last_budget_features():
    from centerpose_amd import track
    budget = 4
    trk = track.DeepSortTracker(2, streams=1, max_tracks=2, budget=budget, device=None)
    host = HostGallery(trk)
    r = np.random.RandomState(4)
    base = r.standard_normal(tr.DIM)
    feats = [(np.round((base + 0.05 * r.standard_normal(tr.DIM)) * 16) / 16).astype(np.float32) for _ in range(budget + 4)]
    for i, f in enumerate(feats):                                            # initiated once, matched budget + 3 times
        host.update(*_person_frame(2, 3, [(100 + 2 * i, 50, 140 + 2 * i, 150)], [f]), [(640, 480)])
    t, = trk.tracks[0]
    assert t.track_id == 1 and t.hits == budget + 4 and t.appended == budget + 4 and t.state == track.CONFIRMED
    ring = host.gallery[t.slot]
    want = feats[-budget:]
    assert sorted(x.tobytes() for x in ring) == sorted(x.tobytes() for x in want)
    assert ring[(budget + 3) % budget].tobytes() == feats[-1].tobytes()
    assert trk.begin()[t.slot] == budget and trk.begin()[1 - t.slot] == 0


def test_freed_slot_is_reused_and_dropped_counts():
    from centerpose_amd import track
    trk = track.DeepSortTracker(3, streams=1, max_tracks=2, budget=4, max_age=2, device=None)
    host = HostGallery(trk)
    r = np.random.RandomState(6)
    fa, fb, fc = (np.round(r.standard_normal(tr.DIM) * 8).astype(np.float32) / 8 for _ in range(3))
    a, b, c = (10, 10, 50, 110), (300, 20, 340, 120), (500, 200, 540, 300)
    size = [(640, 480)]
    host.update(*_person_frame(3, 3, [a, b, c], [fa, fb, fc]), size)         # three detections, two track slots
    assert trk.dropped == [1] and [t.track_id for t in trk.tracks[0]] == [1, 2] and [t.slot for t in trk.tracks[0]] == [0, 1]
    host.update(*_person_frame(3, 3, [a], [fa]), size)                       # b's tentative track misses: deleted, slot 1 is free again
    assert [t.track_id for t in trk.tracks[0]] == [1] and trk.free == [[1]]
    host.update(*_person_frame(3, 3, [a, c], [fa, fc]), size)
    assert [(t.track_id, t.slot) for t in trk.tracks[0]] == [(1, 0), (3, 1)] and trk.dropped == [1]
    assert trk.tracks[0][1].appended == 1 and host.gallery[1, 0].tobytes() == fc.tobytes()
    assert trk.assignments.tolist() == [[1, -1, -1]]


# ---------------------------------------------------------------- 5. refusals
def _cost_args(**over):
    a = dict(gallery=64, ginv=64, glen=64, features=64, slots=64, rows=64, M=4, S=2, Tcap=3, budget=5, q=4, out=64)
    a.update(over)
    return [VP(a[k]) if k in ("gallery", "ginv", "glen", "features", "slots", "rows", "out") else a[k] for k in
            ("gallery", "ginv", "glen", "features", "slots", "rows", "M", "S", "Tcap", "budget", "q", "out")]


COST_REFUSALS = [(dict(budget=0), "budget"), (dict(budget=129), "budget"), (dict(Tcap=0), "Tcap"), (dict(Tcap=1025), "Tcap"),
                 (dict(q=0), "q = 0"), (dict(S=0), "S = 0"), (dict(M=-1), "M = -1"), (dict(S=20000, Tcap=1024, budget=128), "ring rows"),
                 (dict(gallery=0), "null"), (dict(ginv=0), "null"), (dict(glen=0), "null"), (dict(features=0), "null"),
                 (dict(slots=0), "null"), (dict(rows=0), "null"), (dict(out=0), "null")]


@pytest.mark.parametrize("over,word", COST_REFUSALS, ids=[w + str(i) for i, (_, w) in enumerate(COST_REFUSALS)])
def test_cost_launchers_refuse_before_anything_runs(over, word):
    """The pointers are never followed: every call is refused by its arguments alone (rc 1), the device launcher before any launch."""
    L = _L()
    assert L.cp_track_cost_f32(*_cost_args(**over), None) == 1 and word in _err(), _err()
    assert L.cp_track_cost_host(*_cost_args(**over)) == 1 and word in _err(), _err()


def test_alignment_and_append_refusals():
    L = _L()
    assert L.cp_track_cost_f32(*_cost_args(gallery=68), None) == 1 and "16-byte" in _err()
    assert L.cp_track_cost_f32(*_cost_args(features=72), None) == 1 and "16-byte" in _err()
    for fn, tail in ((L.cp_track_append_f32, (None,)), (L.cp_track_append_host, ())):
        assert fn(VP(64), VP(64), VP(64), VP(64), 1, 0, *tail) == 1 and "budget" in _err()
        assert fn(VP(64), VP(64), VP(64), VP(64), 1, 129, *tail) == 1 and "budget" in _err()
        assert fn(VP(64), VP(64), VP(64), VP(64), -1, 5, *tail) == 1 and "n = -1" in _err()
        assert fn(None, VP(64), VP(64), VP(64), 1, 5, *tail) == 1 and "null" in _err()
        assert fn(VP(64), None, VP(64), VP(64), 1, 5, *tail) == 1 and "null" in _err()
        assert fn(VP(64), VP(64), None, VP(64), 1, 5, *tail) == 1 and "null" in _err()
        assert fn(VP(64), VP(64), VP(64), None, 1, 5, *tail) == 1 and "null" in _err()
    assert L.cp_track_append_f32(VP(68), VP(64), VP(64), VP(64), 1, 5, None) == 1 and "16-byte" in _err()
    assert L.cp_track_append_f32(VP(64), VP(64), VP(64), None, 0, 5, None) == 0          # n = 0: nothing to do, nothing launched


def test_tracker_refusals_without_a_device():
    from centerpose_amd import detector, reid, track
    from centerpose_amd._lib import CenterposeHipError
    for bad in (dict(capacity=1, streams=2), dict(capacity=4, streams=0), dict(capacity=4, max_tracks=0), dict(capacity=4, max_tracks=1025),
                dict(capacity=4, budget=0), dict(capacity=4, budget=129)):
        with pytest.raises(ValueError):
            track.DeepSortTracker(device=None, **bad)
    with pytest.raises(CenterposeHipError, match="no CPU fallback"):
        track.DeepSortTracker(4, device="cpu")
    trk = track.DeepSortTracker(4, streams=2, device=None)
    res = reid.ReidResult(torch.zeros((4, 512)), torch.zeros((4,), dtype=torch.int32), torch.zeros((2,), dtype=torch.int32))
    with pytest.raises(CenterposeHipError, match="CUDA tensor"):              # host arrays raise
        trk.update(np.zeros((2, 3, 56), np.float32), res, [(64, 48)] * 2)
    with pytest.raises(CenterposeHipError, match="no CPU fallback"):          # so do host tensors
        trk.update(torch.zeros((2, 3, 56)), res, [(64, 48)] * 2)
    with pytest.raises(ValueError, match="ReidResult"):
        trk.update(torch.zeros((2, 3, 56)), (res.features, res.slots), [(64, 48)] * 2)
    with pytest.raises(ValueError, match="sizes"):
        trk.associate(np.zeros((2, 64, 2)), np.zeros((2, 2, 5)), [(64, 48)])
    # run_batch(track=) without embed=: refused before anything else happens (a detector without a model is enough to get there)
    with pytest.raises(ValueError, match="needs embed"):
        object.__new__(detector.BaseDetector).run_batch([], track=trk)


# ---------------------------------------------------------------- 6. symbols
def test_symbols_in_the_header_and_the_library():
    from centerpose_amd import _lib
    header = open(os.path.join(ROOT, "include", "centerpose_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in SYMBOLS:
        assert "int %s(" % sym in header, sym
        assert " T %s\n" % sym in nm, sym
        assert hasattr(_L(), sym)
