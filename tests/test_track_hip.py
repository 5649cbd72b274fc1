"""Track association on the GPU: cp_track_cost_f32 / cp_track_append_f32 against tests/track_ref.py and the host twins,
track.DeepSortTracker.update over the reference's recorded run, and run_batch(..., embed=, track=)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import track_ref as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p
GLENS = (0, 1, 31, 32, 33, 100, 128)


def _L():
    from centerpose_amd import _lib
    return _lib.lib()


def _err():
    return _L().cp_last_error().decode()


def _stream():
    return VP(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_cost(gallery, ginv, glen, features, slots, rows, S, Tcap, budget, q):
    """Device tensors in -> (cost float32 [S, Tcap, q], det float32 [S, q, 5]) on the host; the buffer starts as a sentinel."""
    out = torch.full((S * Tcap * q + S * q * 5,), -7.0, dtype=torch.float32, device="cuda")
    rc = _L().cp_track_cost_f32(VP(gallery.data_ptr()), VP(ginv.data_ptr()), VP(glen.data_ptr()), VP(features.data_ptr()), VP(slots.data_ptr()),
                                VP(rows.data_ptr()), int(rows.shape[1]), S, Tcap, budget, q, VP(out.data_ptr()), _stream())
    assert rc == 0, _err()
    out = out.cpu().numpy()
    return out[:S * Tcap * q].reshape(S, Tcap, q), out[S * Tcap * q:].reshape(S, q, 5)


def make_case(seed, S, Tcap, budget, q, M, glens=GLENS, every=1):
    """Host arrays of one launch.  Slot i has glen glens[i / every % len] when i % every == 0, else 0; only valid ring rows are filled,
    everything behind them is NaN (rows >= glen must not reach the result).  Every third detection slot is unused and holds NaN
    features; the used ones lie near one ring row of some track, so that the minimum is a nearest neighbour, not ~1 everywhere."""
    r = np.random.RandomState(seed)
    n = S * Tcap
    glen = np.zeros(n, np.int32)
    glen[::every] = [glens[i % len(glens)] for i in range(len(glen[::every]))]
    gallery = np.full((n, budget, tr.DIM), np.nan, np.float32)
    ginv = np.full((n, budget), np.nan, np.float32)
    for t in np.nonzero(glen)[0]:
        k = min(int(glen[t]), budget)
        gallery[t, :k] = tr.f16_features(r, k)
        ginv[t, :k] = (1.0 / np.sqrt((gallery[t, :k].astype(np.float64) ** 2).sum(1))).astype(np.float32)
    features = np.full((S * q, tr.DIM), np.nan, np.float32)
    slots = np.full(S * q, -1, np.int32)
    rows = r.uniform(-20, 700, (S, M, 56)).astype(np.float32)
    live = np.nonzero(glen)[0]
    for s in range(S):
        ms = r.permutation(max(M, q))
        mine = live[(live >= s * Tcap) & (live < (s + 1) * Tcap)]
        for d in range(q):
            if d % 3 == 1 and q > 1:
                continue
            slots[s * q + d] = s * M + ms[d] % M
            f = tr.f16_features(r, 1)[0]
            if len(mine):
                t = mine[d % len(mine)]
                f = gallery[t, (5 * d) % min(int(glen[t]), budget)] * 0.5 + 0.15 * f
            features[s * q + d] = (np.round(f * 8) / 8).astype(np.float16).astype(np.float32)
    return gallery, ginv, glen, features, slots, rows


# every listed glen runs in every case (capped at the budget); q, budget, Tcap and S each take all of their listed values
COST_CASES = [(1, 1, 1, 1), (2, 3, 100, 31), (1, 3, 128, 32), (2, 64, 128, 33), (1, 64, 100, 64), (2, 3, 1, 64), (1, 1, 128, 33), (2, 1, 100, 1)]


@pytest.mark.parametrize("S,Tcap,budget,q", COST_CASES)
def test_cost_kernel_against_the_float64_statement(S, Tcap, budget, q):
    M = 9
    glens = GLENS if Tcap > 1 else (GLENS[(budget + q) % 6 + 1],)               # one track slot: one non-zero glen
    case = make_case(11, S, Tcap, budget, q, M, glens)
    want_cost, want_det = tr.cost_det(*[case[i] for i in (0, 2, 3, 4, 5)], S, Tcap, budget, q)
    cost, det = dev_cost(*[_dev(a) for a in case], S, Tcap, budget, q)
    tr.assert_cost(cost, want_cost, "cost kernel %s" % ((S, Tcap, budget, q),))
    assert det.tobytes() == want_det.tobytes()
    assert np.isfinite(want_cost).any() and float(want_cost[np.isfinite(want_cost)].min()) < 0.9      # unrelated vectors sit at ~1
    if Tcap <= 3:                                                               # and the host twin says the same (the small cases)
        _, host, host_det = tr.host_cost(_L(), *case, S, Tcap, budget, q)
        tr.assert_cost(host, want_cost, "host twin")
        assert host_det.tobytes() == det.tobytes()


def test_cost_kernel_with_1024_blocks():
    S, Tcap, budget, q, M = 2, 512, 100, 33, 5
    case = make_case(12, S, Tcap, budget, q, M, every=37)                      # 28 live slots among 1024, all seven glen values
    want_cost, want_det = tr.cost_det(*[case[i] for i in (0, 2, 3, 4, 5)], S, Tcap, budget, q)
    cost, det = dev_cost(*[_dev(a) for a in case], S, Tcap, budget, q)
    tr.assert_cost(cost, want_cost, "1024 blocks")
    assert det.tobytes() == want_det.tobytes() and int(np.isfinite(want_cost).any(2).sum()) == 24       # 4 of the 28 have glen 0


def test_cost_kernel_streams_are_isolated():
    S, Tcap, budget, q, M = 2, 3, 100, 33, 9
    a = make_case(13, S, Tcap, budget, q, M)
    b = make_case(14, S, Tcap, budget, q, M)
    mixed = [x.copy() for x in a]
    mixed[0][Tcap:], mixed[1][Tcap:], mixed[3][q:] = b[0][Tcap:], b[1][Tcap:], b[3][q:]        # stream 1: another gallery, other features
    c0, d0 = dev_cost(*[_dev(x) for x in a], S, Tcap, budget, q)
    c1, d1 = dev_cost(*[_dev(x) for x in mixed], S, Tcap, budget, q)
    assert c0[0].tobytes() == c1[0].tobytes() and d0.tobytes() == d1.tobytes()
    assert c0[1].tobytes() != c1[1].tobytes()


def test_cost_kernel_beyond_2_to_the_31_floats():
    """S * Tcap * budget * 512 = 2.2e9 floats: the last track slot lies behind 2^31 floats (and 2^33 bytes).  Only that slot is live."""
    S, Tcap, budget, q, M = 33, 1024, 128, 2, 3
    small = make_case(15, 1, 1, budget, q, M, glens=(128,))
    want_cost, want_det = tr.cost_det(*[small[i] for i in (0, 2, 3, 4, 5)], 1, 1, budget, q)
    gallery = torch.empty((S * Tcap, budget, tr.DIM), dtype=torch.float32, device="cuda")       # 8.9 GB, not filled
    ginv = torch.empty((S * Tcap, budget), dtype=torch.float32, device="cuda")
    gallery[-1], ginv[-1] = _dev(small[0][0]), _dev(small[1][0])
    glen = torch.zeros((S * Tcap,), dtype=torch.int32, device="cuda")
    glen[-1] = 128
    features = torch.zeros((S * q, tr.DIM), dtype=torch.float32, device="cuda")
    features[-q:] = _dev(small[3])
    slots = torch.full((S * q,), -1, dtype=torch.int32, device="cuda")
    slots[-q:] = _dev(np.where(small[4] >= 0, small[4] + (S - 1) * M, -1).astype(np.int32))
    rows = torch.zeros((S, M, 56), dtype=torch.float32, device="cuda")
    rows[-1] = _dev(small[5][0])
    cost, det = dev_cost(gallery, ginv, glen, features, slots, rows, S, Tcap, budget, q)
    tr.assert_cost(cost[-1, -1:], want_cost[0], "last slot behind 2^31 floats")
    assert det[-1].tobytes() == want_det[0].tobytes() and not det[:-1].any()
    flat = cost.reshape(-1, q)
    assert np.all(np.isposinf(flat[:-1]))


def test_append_kernel_equals_its_host_twin_bit_for_bit():
    r = np.random.RandomState(2)
    budget, slots_n = 3, 4
    features = tr.f16_features(r, 6)
    g_host, i_host = np.zeros((slots_n, budget, tr.DIM), np.float32), np.zeros((slots_n, budget), np.float32)
    g_ref, i_ref = g_host.copy(), i_host.copy()
    g_dev, i_dev, f_dev = _dev(g_host), _dev(i_host), _dev(features)
    L = _L()
    count = [0] * slots_n
    for step in range(5):                                                   # slot 1 gets 5 features into a ring of 3: it wraps
        table = [(step % 6, 1, count[1] % budget), ((step + 2) % 6, 3, count[3] % budget)]
        if step == 2:
            table += [(-1, 0, 0), (0, 0, budget), (0, -1, 0)]               # entries that write nothing
        count[1] += 1
        count[3] += 1
        t_dev = _dev(np.array(table, np.int32))
        assert L.cp_track_append_f32(VP(g_dev.data_ptr()), VP(i_dev.data_ptr()), VP(f_dev.data_ptr()), VP(t_dev.data_ptr()), len(table),
                                     budget, _stream()) == 0, _err()
        assert tr.host_append(L, g_host, i_host, features, table, budget) == 0
        tr.append(g_ref, i_ref, features, table, budget)
        got_g, got_i = g_dev.cpu().numpy(), i_dev.cpu().numpy()
        assert got_g.tobytes() == g_host.tobytes() == g_ref.tobytes() and got_i.tobytes() == i_host.tobytes() == i_ref.tobytes()
    # features that are not float16 values: the device and the host twin still write the same bits (one summation order)
    wide = r.standard_normal((6, tr.DIM)).astype(np.float32) * 3
    table = [(i, i % slots_n, i % budget) for i in range(6) if i != 4]
    assert L.cp_track_append_f32(VP(g_dev.data_ptr()), VP(i_dev.data_ptr()), VP(_dev(wide).data_ptr()), VP(_dev(np.array(table, np.int32)).data_ptr()),
                                 len(table), budget, _stream()) == 0, _err()
    assert tr.host_append(L, g_host, i_host, wide, table, budget) == 0
    assert g_dev.cpu().numpy().tobytes() == g_host.tobytes() and i_dev.cpu().numpy().tobytes() == i_host.tobytes()
    # n = 0: nothing is launched, nothing changes
    assert L.cp_track_append_f32(VP(g_dev.data_ptr()), VP(i_dev.data_ptr()), VP(f_dev.data_ptr()), None, 0, budget, _stream()) == 0
    assert g_dev.cpu().numpy().tobytes() == g_host.tobytes()


# ---------------------------------------------------------------- DeepSortTracker.update on the device
def _result(features, slots, S):
    from centerpose_amd import reid
    counts = torch.tensor([int((slots.reshape(S, -1)[s] >= 0).sum()) for s in range(S)], dtype=torch.int32, device="cuda")
    return reid.ReidResult(_dev(features), _dev(slots), counts)


def test_update_over_the_recorded_sequence_on_the_device():
    from centerpose_amd import track
    g = tr.sequence()
    trk = track.DeepSortTracker(g["S"] * g["q"], streams=g["S"], **g["kw"])
    sizes = [tuple(x) for x in g["sizes"].tolist()]
    for f in range(g["F"]):
        rows, features, slots = tr.frame_inputs(g, f)
        outs = trk.update(_dev(rows), _result(features, slots, g["S"]), sizes)
        tr.check_frame(g, f, trk, outs)
    assert trk.dropped == [0, 0]
    # the gallery the device holds is the one the host twins build from the same tables
    t = trk.tracks[0][0]
    ring = trk.gallery[t.slot].cpu().numpy()
    assert t.appended > g["kw"]["budget"] and np.isfinite(ring).all() and bool((trk.ginv[t.slot] > 0).all())


@functools.lru_cache(maxsize=None)
def _sd():
    from centerpose_amd import synth
    g = np.load(os.path.join(ROOT, "tests", "golden", "reid_features.npz"))
    return synth.make_state_dict("reid", seed=int(g["seed"]))


def _frame(seed, H, W):
    """A B, G, R frame with large-scale structure, uint8 [H, W, 3]."""
    r = np.random.RandomState(seed)
    grid = torch.from_numpy(r.uniform(0, 255, (1, 3, 5, 6)))
    up = torch.nn.functional.interpolate(grid, size=(H, W), mode="bilinear", align_corners=False)[0].numpy()
    return np.clip(np.rint(up + r.uniform(-20, 20, up.shape)), 0, 255).astype(np.uint8).transpose(1, 2, 0).copy()


def _ids(tracks):
    return [t[:, 4].tolist() for t in tracks]


def test_run_batch_with_track_and_the_refusals():
    from centerpose_amd import config, detector, reid, track
    from centerpose_amd._lib import CenterposeHipError
    det = detector.MultiPoseDetector(config.get_cfg("dla_34", TEST__FIX_RES=False))
    ex = reid.ReidExtractor(_sd(), capacity=8)
    frames = [torch.from_numpy(_frame(31 + n, 96, 128)).cuda() for n in range(2)]
    sizes = [(128, 96)] * 2
    trk, twin = track.DeepSortTracker(8, streams=2), track.DeepSortTracker(8, streams=2)
    plain_rows, plain_res = det.run_batch(frames, return_device=True, embed=ex)
    plain_feats, plain_slots = plain_res.features.clone(), plain_res.slots.clone()
    assert int(plain_res.counts.sum()) > 0
    history = []
    for call in range(5):
        rows, res, tracks = det.run_batch(frames, return_device=True, embed=ex, track=trk)
        assert torch.equal(rows, plain_rows) and torch.equal(res.features, plain_feats) and torch.equal(res.slots, plain_slots)
        want = twin.update(rows, res, sizes)                                  # a second tracker on those rows says the same
        assert len(tracks) == 2 and all(a.dtype == np.int64 and np.array_equal(a, b) for a, b in zip(tracks, want))
        assert np.array_equal(trk.assignments, twin.assignments)
        history.append(([t.copy() for t in tracks], trk.assignments.copy()))
    used = plain_slots.cpu().numpy().reshape(2, 4) >= 0
    assert np.all(history[0][1] == -1)                                        # the first call starts tracks, it matches nothing
    for call in range(1, 5):                                                  # unchanged frames: every detection keeps its identity
        assert np.all(history[call][1][used] >= 1) and np.array_equal(history[call][1], history[1][1])
    assert sum(len(t) for t in history[4][0]) == int(used.sum()) > 0          # confirmed after n_init = 3 hits, and put out
    assert _ids(history[3][0]) == _ids(history[4][0])
    assert sorted(np.concatenate(history[4][0])[:, 4].tolist()) == sorted(history[4][1][used].tolist())
    # the host-list form and draw=True return the same tracks beside their usual results
    listed, _, tracks = det.run_batch(frames, embed=ex, track=trk)
    assert listed == det.run_batch(frames) and _ids(tracks) == _ids(history[4][0])
    painted = [f.clone() for f in frames]
    rows, _, tracks = det.run_batch(painted, return_device=True, embed=ex, track=trk, draw=True)
    assert torch.equal(rows, plain_rows) and _ids(tracks) == _ids(history[4][0])
    # refusals
    with pytest.raises(ValueError, match="needs embed"):
        det.run_batch(frames, track=trk)
    with pytest.raises(ValueError, match="tracker of 2 streams"):
        det.run_batch(frames[:1], embed=ex, track=trk)
    with pytest.raises(ValueError, match="capacity"):
        det.run_batch(frames, embed=ex, track=track.DeepSortTracker(6, streams=2))
    res = plain_res
    with pytest.raises(ValueError, match="sizes"):
        trk.update(plain_rows, res, sizes[:1])
    with pytest.raises(ValueError, match="streams"):
        trk.update(plain_rows[:1], res, sizes)
    with pytest.raises(CenterposeHipError, match="float32"):
        trk.update(plain_rows.double(), res, sizes)
    with pytest.raises(CenterposeHipError, match="56"):
        trk.update(plain_rows[..., :55], res, sizes)
    with pytest.raises(CenterposeHipError, match="no CPU fallback"):
        trk.update(plain_rows.cpu(), res, sizes)
    with pytest.raises(CenterposeHipError, match="CUDA tensor"):
        trk.update(plain_rows.cpu().numpy(), res, sizes)
    with pytest.raises(ValueError, match="capacity 8"):
        trk.update(plain_rows, reid.ReidResult(res.features[:6], res.slots[:6], res.counts), sizes)
    with pytest.raises(CenterposeHipError, match="int32"):
        trk.update(plain_rows, reid.ReidResult(res.features, res.slots.long(), res.counts), sizes)
