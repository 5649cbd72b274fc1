"""An independent float64 NumPy statement of the track-association stage (cp_track_cost_f32 / cp_track_append_f32: cost, det, the ring),
the recorded sequence of tests/golden/track_sequence.npz, and the driver both test files run a DeepSortTracker over it with."""
import ctypes
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p
DIM = 512
# a 512-term float32 dot of normalised vectors: 512 * 2^-24 * sum |a_i b_i| <= 3.1e-5, plus the two normalisations
COST_TOL = 4e-5


def cost_det(gallery, glen, features, slots, rows, S, Tcap, budget, q):
    """-> (cost float64 [S, Tcap, q], det float32 [S, q, 5]).  gallery [S * Tcap, budget, 512], features [>= S * q, 512], rows [S, M, 56].
    Rows >= glen are never touched (they may hold NaN)."""
    M = rows.shape[1]
    flat = rows.reshape(-1, 56)
    cost = np.full((S, Tcap, q), np.inf)
    det = np.zeros((S, q, 5), np.float32)
    for s in range(S):
        used = [d for d in range(q) if 0 <= int(slots[s * q + d]) < S * M]
        if not used:
            continue
        det[s, used] = flat[slots[s * q + np.array(used)], :5]
        f = features[s * q + np.array(used)].astype(np.float64)
        f = f / np.sqrt((f * f).sum(1, keepdims=True))
        for t in range(Tcap):
            n = min(int(glen[s * Tcap + t]), budget)
            if n <= 0:
                continue
            g = gallery[s * Tcap + t, :n].astype(np.float64)
            g = g / np.sqrt((g * g).sum(1, keepdims=True))
            cost[s, t, used] = (1.0 - g @ f.T).min(0)
    return cost, det


def append(gallery, ginv, features, table, budget):
    """The ring after the table's entries, in place: rows copied as they are, ginv = float32(1) / sqrt(float32(sum of squares)), the sum
    in float64 (exact, whatever its order, for features that are float16 values: 22-bit squares, 512 of them)."""
    for fs, ts, pos in np.asarray(table).reshape(-1, 3).tolist():
        if fs < 0 or ts < 0 or not 0 <= pos < budget:
            continue
        f = features[fs]
        gallery[ts, pos] = f
        ss = np.float32((f.astype(np.float64) ** 2).sum())
        ginv[ts, pos] = np.float32(1.0) / np.sqrt(ss)


def assert_cost(got, want, what=""):
    """got float32 against want float64: +inf exactly where wanted, finite entries within COST_TOL."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isposinf(got), np.isposinf(want)), what + ": +inf entries differ"
    fin = np.isfinite(want)
    assert np.all(np.isfinite(got[fin])), what + ": a finite entry is not finite"
    err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    print("%s: worst |cost - float64| = %.3e over %d entries (bar %.1e)" % (what, err, int(fin.sum()), COST_TOL))
    assert err <= COST_TOL, "%s: %.3e > %.1e" % (what, err, COST_TOL)


def f16_features(r, n, scale_lo=-1, scale_hi=3):
    """n feature rows of float16 values, not unit norm: quarter steps times a power of two."""
    v = np.round(r.standard_normal((n, DIM)) * 4) / 4 * 2.0 ** r.randint(scale_lo, scale_hi, (n, 1))
    return v.astype(np.float16).astype(np.float32)


# ---------------------------------------------------------------- host twins
def host_cost(L, gallery, ginv, glen, features, slots, rows, S, Tcap, budget, q):
    """-> (rc, cost float32 [S, Tcap, q], det float32 [S, q, 5]); the buffer starts as a sentinel."""
    M = rows.shape[1]
    out = np.full(S * Tcap * q + S * q * 5, -7.0, np.float32)
    a = [np.ascontiguousarray(x, t) for x, t in ((gallery, np.float32), (ginv, np.float32), (glen, np.int32), (features, np.float32),
                                                 (slots, np.int32), (rows, np.float32))]
    rc = L.cp_track_cost_host(*[x.ctypes.data_as(VP) for x in a], M, S, Tcap, budget, q, out.ctypes.data_as(VP))
    return rc, out[:S * Tcap * q].reshape(S, Tcap, q), out[S * Tcap * q:].reshape(S, q, 5)


def host_append(L, gallery, ginv, features, table, budget):
    """In place on float32 C-contiguous gallery / ginv -> rc."""
    assert gallery.dtype == np.float32 and gallery.flags.c_contiguous and ginv.dtype == np.float32 and ginv.flags.c_contiguous
    table = np.ascontiguousarray(table, np.int32).reshape(-1, 3)
    features = np.ascontiguousarray(features, np.float32)
    return L.cp_track_append_host(gallery.ctypes.data_as(VP), ginv.ctypes.data_as(VP), features.ctypes.data_as(VP), table.ctypes.data_as(VP),
                                  len(table), budget)


# ---------------------------------------------------------------- the recorded sequence
@functools.lru_cache(maxsize=None)
def sequence():
    g = np.load(os.path.join(ROOT, "tests", "golden", "track_sequence.npz"))
    g = {k: g[k] for k in g.files}
    p = g["params"]
    g["kw"] = dict(max_cosine_distance=float(p[0]), max_iou_distance=float(p[1]), max_age=int(p[2]), n_init=int(p[3]), budget=int(p[4]),
                   max_tracks=int(p[5]))
    g["q"], g["M"], g["S"], g["F"] = int(p[6]), int(p[7]), len(g["sizes"]), int(g["frames"])
    return g


def frame_inputs(g, f):
    """What frame f hands to an update: (rows float32 [S, M, 56], features float32 [S * q, 512], slots int32 [S * q]).  Detection slot d of
    stream s holds the recording's detection d; its row is M - 1 - d of the stream's block (not the identity on purpose)."""
    S, q, M = g["S"], g["q"], g["M"]
    rows = np.zeros((S, M, 56), np.float32)
    feats = np.full((S * q, DIM), np.nan, np.float32)           # unused slots are meaningless: NaN must not spread
    slots = np.full(S * q, -1, np.int32)
    for i in np.nonzero(g["det_index"][:, 0] == f)[0]:
        _, s, d = g["det_index"][i]
        m = M - 1 - d
        rows[s, m, :4], rows[s, m, 4] = g["det_box"][i], g["det_score"][i]
        feats[s * q + d] = g["det_feat"][i].astype(np.float32)
        slots[s * q + d] = s * M + m
    return rows, feats, slots


def check_frame(g, f, trk, outs):
    """The tracker's state after frame f against the recording: outputs, ids, states, counters, assignments exactly; means and
    covariances within 1e-9 of the largest entry (float64 on both sides, another factorisation; the 4 x 4 systems have condition ~1e4)."""
    for s in range(g["S"]):
        want = g["out"][(g["out"][:, 0] == f) & (g["out"][:, 1] == s)][:, 2:]
        assert outs[s].dtype == np.int64 and outs[s].shape == want.shape and np.array_equal(outs[s], want), (f, s, outs[s], want)
        sel = (g["state_index"][:, 0] == f) & (g["state_index"][:, 1] == s)
        idx = g["state_index"][sel][:, 2:]
        got = [(t.track_id, t.state, t.time_since_update, t.hits) for t in trk.tracks[s]]
        assert got == [tuple(r) for r in idx.tolist()], (f, s, got, idx)
        for t, mean, cov in zip(trk.tracks[s], g["state_mean"][sel], g["state_cov"][sel]):
            assert np.abs(t.mean - mean).max() <= 1e-9 * np.abs(mean).max(), (f, s, t.track_id)
            assert np.abs(t.covariance - cov).max() <= 1e-9 * np.abs(cov).max(), (f, s, t.track_id)
    assert np.array_equal(trk.assignments, g["assign"][f]), (f, trk.assignments, g["assign"][f])
