"""A recorded DeepSort run of the REFERENCE'S OWN tracker (build container only; the reference never travels, and this never runs on
the GPU machine).

The reference's `demo/tracking/sort` package is imported as it stands, with shims for what no longer exists around it: `np.float`,
`np.int`, an empty `cv2` module and `sklearn.utils.linear_assignment_.linear_assignment` (scipy.optimize.linear_sum_assignment).  The
steps of `DeepSort.update` around it (deep_sort.py:24-61: Detection objects, non_max_suppression at overlap 1.0, predict, update, the
output rule) are restated below -- that file cannot be imported without the torch extractor.  The boxes reach the tracker as the demo
hands them over (demo_main.py:185-190: truncated to int, then tlwh).

The sequence is synthetic: 2 streams, people on straight lines with misses of 1..3 frames, one leaving for good, one entering late, two
crossing, one single-frame false positive.  Features are float16 values, not unit norm.  Recorded per frame: the reference's outputs,
every track (id, state, time_since_update, hits, mean, covariance), the track matched to each detection slot, and every cost matrix
handed to the assignment with the pairs it chose.  The margins that make the recording decidable are asserted while it is made:
appearance costs >= 1e-3 away from max_cosine_distance, gate and IoU values >= 1e-6 (relative) away from their thresholds, distinct
scores within a frame, every assignment's optimum >= 1e-3 better than the best alternative (each chosen pair below the threshold is
forbidden in turn and the matrix re-solved), and detections that start tracks doing so in detection order.

    python tests/golden/make_golden_track.py <root of the reference checkout>
"""
import io
import os
import sys
import types
import zipfile

import numpy as np
from scipy.optimize import linear_sum_assignment

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "track_sequence.npz")

PARAMS = dict(max_cosine_distance=0.2, max_iou_distance=0.7, max_age=5, n_init=3, budget=6, max_tracks=6, q=6, M=7)
SIZES = [(640, 480), (512, 384)]              # (W, H) per stream
FRAMES = 24
GATE = 9.4877

LOG = {"cm": [], "ctx": (0, 0)}


def load_reference_sort(root):
    np.float, np.int = float, int                                                        # gone since NumPy 1.24
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sk, sku, skl = types.ModuleType("sklearn"), types.ModuleType("sklearn.utils"), types.ModuleType("sklearn.utils.linear_assignment_")

    def linear_assignment(cost):
        r, c = linear_sum_assignment(cost)
        pairs = np.stack([r, c], 1)
        check_assignment_margin(np.array(cost), pairs)
        LOG["cm"].append((LOG["ctx"], LOG["kind"], np.array(cost), pairs))
        return pairs

    skl.linear_assignment = linear_assignment
    sys.modules.update({"sklearn": sk, "sklearn.utils": sku, "sklearn.utils.linear_assignment_": skl})
    sys.path.insert(0, os.path.join(root, "demo", "tracking"))
    import sort.tracker  # noqa: F401
    import sort.detection  # noqa: F401
    import sort.nn_matching  # noqa: F401
    import sort.preprocessing  # noqa: F401
    return sys.modules["sort"]


def check_assignment_margin(cost, pairs):
    thr = LOG["thr"]
    best = cost[pairs[:, 0], pairs[:, 1]].sum()
    for r, c in pairs:
        if cost[r, c] > thr:
            continue
        alt = cost.copy()
        alt[r, c] = 1e9
        rr, cc = linear_sum_assignment(alt)
        assert alt[rr, cc].sum() >= best + 1e-3, ("assignment margin", LOG["ctx"], cost, (r, c), alt[rr, cc].sum() - best)


def instrument(sort):
    """Wrap the reference's functions where the margins are visible; the functions themselves run untouched."""
    from sort import iou_matching, kalman_filter, linear_assignment, nn_matching
    dist = nn_matching.NearestNeighborDistanceMetric.distance

    def distance(self, features, targets):
        c = dist(self, features, targets)
        assert np.all(np.abs(c - self.matching_threshold) >= 1e-3), ("appearance margin", LOG["ctx"], c)
        return c

    nn_matching.NearestNeighborDistanceMetric.distance = distance
    gate = kalman_filter.KalmanFilter.gating_distance

    def gating_distance(self, mean, covariance, measurements, only_position=False):
        d = gate(self, mean, covariance, measurements, only_position)
        assert np.all(np.abs(d - GATE) >= 1e-6 * GATE), ("gate margin", LOG["ctx"], d)
        return d

    kalman_filter.KalmanFilter.gating_distance = gating_distance
    iou_cost = iou_matching.iou_cost

    def iou_cost_checked(tracks, detections, track_indices=None, detection_indices=None):
        c = iou_cost(tracks, detections, track_indices, detection_indices)
        assert np.all(np.abs(c - PARAMS["max_iou_distance"]) >= 1e-6 * PARAMS["max_iou_distance"]), ("iou margin", LOG["ctx"], c)
        return c

    iou_matching.iou_cost = iou_cost_checked
    mcm = linear_assignment.min_cost_matching

    def min_cost_matching(distance_metric, max_distance, *a, **k):
        LOG["thr"], LOG["kind"] = max_distance, int(distance_metric is iou_cost_checked)
        return mcm(distance_metric, max_distance, *a, **k)

    linear_assignment.min_cost_matching = min_cost_matching


# ---------------------------------------------------------------- the synthetic sequence
def people(stream):
    """(first frame, last frame, missed frames, x0, y0, vx, vy, w, h) of the top-left corner at frame 0."""
    if stream == 0:
        return [(0, 23, (6,), 40.3, 60.2, 9.1, 1.2, 48.6, 120.4),           # left to right, crosses the next one
                (0, 23, (11, 12), 520.7, 80.5, -8.4, 0.7, 52.2, 131.8),     # right to left
                (0, 9, (), 250.4, 250.6, 0.6, -3.1, 40.9, 96.3),            # leaves for good after frame 9
                (13, 23, (17, 18, 19), 300.2, 200.8, -2.2, 1.9, 44.5, 101.7),   # enters late, missed for 3 frames
                (4, 4, (), 100.5, 300.5, 0.0, 0.0, 30.2, 60.9)]             # a single-frame false positive
    return [(0, 23, (3, 4), 30.8, 40.1, 6.3, 2.2, 38.4, 90.7),
            (2, 23, (15,), 400.6, 120.3, -5.2, 1.1, 42.7, 99.2),
            (0, 14, (), 200.1, 200.9, 1.4, -2.7, 36.8, 80.6),
            (8, 23, (), 120.9, 150.4, 4.8, -1.6, 40.2, 88.5)]


def sequence():
    """-> list over frames of list over streams of (slot rows: box [n, 4] float32, score [n] float32, feat [n, 512] float16)."""
    r = np.random.RandomState(1234)
    base = {(s, p): r.standard_normal(512) for s in range(2) for p in range(8)}
    frames = []
    for f in range(FRAMES):
        per = []
        for s in range(2):
            boxes, scores, feats = [], [], []
            for p, (a, b, miss, x0, y0, vx, vy, w, h) in enumerate(people(s)):
                if not a <= f <= b or f in miss:
                    continue
                jit = r.uniform(-0.6, 0.6, 4)
                x1, y1 = x0 + vx * f + jit[0], y0 + vy * f + jit[1]
                boxes.append([x1, y1, x1 + w + jit[2], y1 + h + jit[3]])
                scores.append(0.35 + 0.6 * ((0.377 * (p + 1) * (f + 3) + 0.11 * s) % 1.0))
                v = base[(s, p)] + 0.22 * r.standard_normal(512)
                feats.append(np.round(v * 4) / 4 * 2.0 ** r.randint(-1, 3))          # quarter steps times a power of two: exact in f16
            assert len(set(np.float32(scores).tolist())) == len(scores), ("distinct scores", f, s)
            per.append((np.array(boxes, np.float32).reshape(-1, 4), np.array(scores, np.float32), np.array(feats, np.float16).reshape(-1, 512)))
        frames.append(per)
    return frames


# ---------------------------------------------------------------- DeepSort.update around the reference's tracker
def deepsort_update(sort, tracker, box, score, feat, size):
    """-> (outputs int64 [k, 5], slot of every detection object in the order the tracker sees them)."""
    from sort.detection import Detection
    from sort.preprocessing import non_max_suppression
    W, H = size
    ib = box.astype(np.int32)                                                      # demo_main.py:185
    tlwh = np.stack([ib[:, 0], ib[:, 1], ib[:, 2] - ib[:, 0], ib[:, 3] - ib[:, 1]], 1).reshape(-1, 4)
    keep = [i for i in range(len(ib)) if score[i] > 0.3 and tlwh[i, 3] > 0]
    dets = [Detection(tlwh[i], score[i], feat[i].astype(np.float32)) for i in keep]
    order = non_max_suppression(np.array([d.tlwh for d in dets]), 1.0, np.array([d.confidence for d in dets]))
    assert sorted(order) == list(range(len(dets)))                                 # at overlap 1.0 nothing is suppressed
    dets, slots = [dets[i] for i in order], [keep[i] for i in order]
    tracker.predict()
    seen = {}
    match = tracker._match

    def _match(detections):
        m, ut, ud = match(detections)
        assert list(ud) == sorted(ud), ("tracks start in detection order", LOG["ctx"], ud)
        seen["matches"] = [(tracker.tracks[t].track_id, slots[d]) for t, d in m]
        return m, ut, ud

    tracker._match = _match
    tracker.update(dets)
    tracker._match = match
    out = []
    for t in tracker.tracks:
        if not t.is_confirmed() or t.time_since_update > 1:
            continue
        x1, y1, w, h = t.to_tlwh()
        x1, y1 = max(x1, 0), max(y1, 0)
        out.append([int(x1), int(y1), min(int(x1 + w), W - 1), min(int(y1 + h), H - 1), t.track_id])
    return np.array(out, np.int64).reshape(-1, 5), seen["matches"]


def npz_bytes(**arrays):
    """An .npz (deflate) with fixed member time stamps: two runs write identical bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.save(b, np.asarray(arrays[k]))
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), b.getvalue(), zipfile.ZIP_DEFLATED)
    return buf.getvalue()


def main(root):
    sort = load_reference_sort(root)
    instrument(sort)
    from sort.nn_matching import NearestNeighborDistanceMetric
    from sort.tracker import Tracker
    P = PARAMS
    trackers = [Tracker(NearestNeighborDistanceMetric("cosine", P["max_cosine_distance"], P["budget"]), P["max_iou_distance"], P["max_age"],
                        P["n_init"]) for _ in range(2)]
    det_index, det_box, det_score, det_feat = [], [], [], []
    out_rows, st_index, st_mean, st_cov = [], [], [], []
    assign = np.full((FRAMES, 2, P["q"]), -1, np.int64)
    for f, per in enumerate(sequence()):
        for s, (box, score, feat) in enumerate(per):
            assert len(box) <= P["q"]
            LOG["ctx"] = (f, s)
            for d in range(len(box)):
                det_index.append((f, s, d))
                det_box.append(box[d]), det_score.append(score[d]), det_feat.append(feat[d])
            out, matches = deepsort_update(sort, trackers[s], box, score, feat, SIZES[s])
            out_rows += [(f, s) + tuple(o) for o in out.tolist()]
            for tid, d in matches:
                assign[f, s, d] = tid
            assert len(trackers[s].tracks) <= P["max_tracks"]
            for t in trackers[s].tracks:
                st_index.append((f, s, t.track_id, t.state, t.time_since_update, t.hits))
                st_mean.append(t.mean), st_cov.append(t.covariance)
    cm_index, cm_values, cm_pairs = [], [], []
    for (f, s), kind, cost, pairs in LOG["cm"]:
        cm_index.append((f, s, kind, cost.shape[0], cost.shape[1], sum(len(v) for v in cm_values), sum(len(p) for p in cm_pairs), len(pairs)))
        cm_values.append(cost.reshape(-1)), cm_pairs.append(pairs.reshape(-1, 2))
    states = np.array(st_index, np.int64)
    ids = [sorted(set(states[states[:, 1] == s][:, 2].tolist())) for s in range(2)]
    print("frames %d, detections %d, track ids per stream %s, assignments recorded %d" % (FRAMES, len(det_index), ids, len(cm_index)))
    assert int((states[:, 3] == 2).sum()) > 0 and all(len(i) >= 4 for i in ids)
    data = npz_bytes(params=np.array([P["max_cosine_distance"], P["max_iou_distance"], P["max_age"], P["n_init"], P["budget"],
                                      P["max_tracks"], P["q"], P["M"]], np.float64),
                     sizes=np.array(SIZES, np.int64), frames=np.int64(FRAMES),
                     det_index=np.array(det_index, np.int64), det_box=np.array(det_box, np.float32), det_score=np.array(det_score, np.float32),
                     det_feat=np.array(det_feat, np.float16),
                     out=np.array(out_rows, np.int64).reshape(-1, 7), state_index=states, state_mean=np.array(st_mean, np.float64),
                     state_cov=np.array(st_cov, np.float64), assign=assign,
                     cm_index=np.array(cm_index, np.int64), cm_values=np.concatenate(cm_values), cm_pairs=np.concatenate(cm_pairs).astype(np.int64))
    assert len(data) < 222229, len(data)
    with open(OUT, "wb") as fh:
        fh.write(data)
    print("wrote %s: %d bytes" % (OUT, len(data)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
