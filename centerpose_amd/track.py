"""DeepSort association for the detections of `run_batch(..., embed=)`: identities across frames, the appearance gallery on the device.

Replaces the last step of the reference's video demo, ``DeepSort.update`` (demo/tracking/deep_sort.py:24-61) over the ``sort`` package
(tracker.py, track.py, kalman_filter.py, linear_assignment.py, iou_matching.py, nn_matching.py), and splits it where the data is:
  device -- the features (a ReidResult), the gallery (the last `budget` features of every track: tracks x budget x 2 KB, the only large
            data of the tracker) and the appearance cost matrix, a GEMM with a min-reduction (csrc/track_assoc.hip);
  host   -- the Kalman filters (8 floats of state per track, float64), the gating, the assignment (cp_linear_assignment_host, plain
            C++: no scipy, no sklearn) and the bookkeeping: sequential logic over a handful of boxes.
Per call one small table goes up (the ring lengths), one small buffer comes down (costs and boxes), a second small table goes up (which
feature goes into which ring row).  The host logic is this project's own statement of the behaviour, not the reference's text.
One rule is stated more narrowly than the reference behaves: unmatched detections start tracks in detection order (score descending).
The reference lists the detections its solver paired above the threshold after the unpaired ones, an order that depends on the
solver's tie-breaking among equal thresholded entries; the recording the tests use asserts that both orders coincide on every frame.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .frames import FrameIO, check_rows
from .reid import ReidResult

DIM = 512
MAX_BUDGET, MAX_TCAP = 128, 1024                 # TH_MAX_BUDGET, TH_MAX_TCAP (csrc/track_host.h)
GATE_4DOF = 9.4877                               # 0.95 quantile of chi-square with 4 degrees of freedom (kalman_filter.py:10-19)
GATED_COST = 1e5                                 # linear_assignment.py:9
TENTATIVE, CONFIRMED, DELETED = 1, 2, 3          # track.py:14-16
STD_POSITION, STD_VELOCITY = 1.0 / 20, 1.0 / 160

_MOTION = np.eye(8)
_MOTION[:4, 4:] = np.eye(4)
_OBSERVE = np.eye(4, 8)


def kf_initiate(xyah):
    """(mean [8], covariance [8, 8]) of a new track at the measurement (cx, cy, aspect, height); velocities start at 0."""
    h = xyah[3]
    std = np.array([2 * STD_POSITION * h, 2 * STD_POSITION * h, 1e-2, 2 * STD_POSITION * h,
                    10 * STD_VELOCITY * h, 10 * STD_VELOCITY * h, 1e-5, 10 * STD_VELOCITY * h])
    return np.concatenate([np.asarray(xyah, np.float64), np.zeros(4)]), np.diag(std * std)


def kf_predict(mean, cov):
    """One constant-velocity step; the process noise scales with the height."""
    h = mean[3]
    std = np.array([STD_POSITION * h, STD_POSITION * h, 1e-2, STD_POSITION * h, STD_VELOCITY * h, STD_VELOCITY * h, 1e-5, STD_VELOCITY * h])
    return _MOTION @ mean, np.linalg.multi_dot((_MOTION, cov, _MOTION.T)) + np.diag(std * std)


def kf_project(mean, cov):
    """The state in measurement space, with the measurement noise added."""
    h = mean[3]
    std = np.array([STD_POSITION * h, STD_POSITION * h, 1e-1, STD_POSITION * h])
    return _OBSERVE @ mean, np.linalg.multi_dot((_OBSERVE, cov, _OBSERVE.T)) + np.diag(std * std)


def kf_update(mean, cov, xyah):
    """The correction step for one measurement."""
    pm, pc = kf_project(mean, cov)
    gain = np.linalg.solve(pc, (cov @ _OBSERVE.T).T).T           # pc is symmetric positive definite: K = P H' S^-1
    return mean + (np.asarray(xyah, np.float64) - pm) @ gain.T, cov - np.linalg.multi_dot((gain, pc, gain.T))


def kf_gating_distance(mean, cov, xyah):
    """Squared Mahalanobis distances of measurements [n, 4] to the projected state."""
    pm, pc = kf_project(mean, cov)
    z = np.linalg.solve(np.linalg.cholesky(pc), (np.asarray(xyah, np.float64) - pm).T)
    return (z * z).sum(0)


def _xyah(tlwh):
    return np.array([tlwh[0] + tlwh[2] / 2, tlwh[1] + tlwh[3] / 2, tlwh[2] / tlwh[3], tlwh[3]])


def _iou(box, cands):
    """box [4], cands [n, 4], both (left, top, width, height)."""
    tl = np.maximum(box[:2], cands[:, :2])
    br = np.minimum(box[:2] + box[2:], cands[:, :2] + cands[:, 2:])
    inter = np.maximum(0.0, br - tl).prod(1)
    return inter / (box[2:].prod() + cands[:, 2:].prod(1) - inter)


def linear_assignment(cost):
    """Minimum-cost assignment of a float64 matrix [r, c] through cp_linear_assignment_host -> int array [min(r, c), 2] of (row, col)
    pairs in row order."""
    cost = np.ascontiguousarray(cost, np.float64)
    r, c = cost.shape
    out = np.full(max(r, 1), -1, np.int32)
    _lib.check(_lib.lib().cp_linear_assignment_host(cost.ctypes.data_as(ctypes.c_void_p), r, c, c, out.ctypes.data_as(ctypes.c_void_p)),
               "cp_linear_assignment_host")
    return np.array([(i, int(out[i])) for i in range(r) if out[i] >= 0], np.int64).reshape(-1, 2)


class Track:
    __slots__ = ("track_id", "slot", "state", "hits", "age", "time_since_update", "mean", "covariance", "appended")

    def __init__(self, track_id, slot, mean, covariance):
        self.track_id, self.slot, self.state, self.hits, self.age, self.time_since_update = track_id, slot, TENTATIVE, 1, 1, 0
        self.mean, self.covariance, self.appended = mean, covariance, 0        # appended: features written to the ring so far

    def tlwh(self):
        w = self.mean[2] * self.mean[3]
        return np.array([self.mean[0] - w / 2, self.mean[1] - self.mean[3] / 2, w, self.mean[3]])


class DeepSortTracker:
    """DeepSort identities for `streams` independent video streams; frame n of every call belongs to stream n.

    capacity: the ReidExtractor's; every stream owns q = capacity // streams detection slots.  max_tracks: track slots per stream
    (1..1024), tentative tracks included.  budget: features kept per track (1..128).  The other defaults are the reference's
    (deep_sort.py:14-22, tracker.py:40).  The gallery is `streams * max_tracks * budget * 2 KB` of device memory, allocated here.

    tracks[s]: the live tracks of stream s in creation order.  assignments: int64 [streams, q], the id of the track matched to each
    detection slot in the last update, -1 where none was (a detection that started a track is not a match).  dropped[s]: detections
    that could not start a track because every track slot of the stream was taken."""

    def __init__(self, capacity, streams=1, max_tracks=64, budget=100, max_cosine_distance=0.2, max_iou_distance=0.7, max_age=30,
                 n_init=3, device="cuda"):
        capacity, streams, max_tracks, budget = int(capacity), int(streams), int(max_tracks), int(budget)
        if streams < 1 or capacity < streams:
            raise ValueError("capacity %d for %d streams: every stream needs at least one detection slot" % (capacity, streams))
        if not 1 <= max_tracks <= MAX_TCAP:
            raise ValueError("max_tracks must lie in 1..%d (got %d)" % (MAX_TCAP, max_tracks))
        if not 1 <= budget <= MAX_BUDGET:
            raise ValueError("budget must lie in 1..%d (got %d)" % (MAX_BUDGET, budget))
        if streams * max_tracks * budget > 2 ** 31 - 1:
            raise ValueError("streams * max_tracks * budget = %d ring rows are too many" % (streams * max_tracks * budget))
        self.capacity, self.streams, self.max_tracks, self.budget = capacity, streams, max_tracks, budget
        self.q = capacity // streams
        self.max_cosine_distance, self.max_iou_distance = float(max_cosine_distance), float(max_iou_distance)
        self.max_age, self.n_init = int(max_age), int(n_init)
        self.tracks = [[] for _ in range(streams)]
        self.free = [list(range(max_tracks)) for _ in range(streams)]           # free track slots, lowest first
        self.next_id = [1] * streams
        self.dropped = [0] * streams
        self.assignments = np.full((streams, self.q), -1, np.int64)
        self.device = None
        if device is not None:                                                  # None: host logic only (begin / associate), no buffers
            dev = torch.device(device)
            if dev.type != "cuda":
                raise _lib.CenterposeHipError("the gallery lives on the GPU (got device %s): there is no CPU fallback" % dev)
            self.device = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
            self.gallery = torch.zeros((streams * max_tracks, budget, DIM), dtype=torch.float32, device=self.device)
            self.ginv = torch.zeros((streams * max_tracks, budget), dtype=torch.float32, device=self.device)
            self.out = torch.empty((streams * max_tracks * self.q + streams * self.q * 5,), dtype=torch.float32, device=self.device)
            self._io = FrameIO(self.device)

    # ------------------------------------------------------------------ host logic
    def begin(self):
        """Step 1 of an update: Kalman predict for every track -> glen int32 [streams * max_tracks], the valid ring rows of every track
        slot for the cost launch: 0 for a free slot and for a track that is not confirmed."""
        glen = np.zeros(self.streams * self.max_tracks, np.int32)
        for s, tracks in enumerate(self.tracks):
            for t in tracks:
                t.mean, t.covariance = kf_predict(t.mean, t.covariance)
                t.age += 1
                t.time_since_update += 1
                if t.state == CONFIRMED:
                    glen[s * self.max_tracks + t.slot] = min(t.appended, self.budget)
        return glen

    def _min_cost_matching(self, cost, max_distance, track_idx, det_idx):
        """Thresholded assignment of cost [len(track_idx), len(det_idx)] -> (matches, unmatched tracks, unmatched detections)."""
        if not track_idx or not det_idx:
            return [], list(track_idx), list(det_idx)
        cost = np.array(cost, np.float64)
        cost[cost > max_distance] = max_distance + 1e-5
        pairs = linear_assignment(cost)
        matches = [(track_idx[r], det_idx[c]) for r, c in pairs if cost[r, c] <= max_distance]
        hit_t, hit_d = {m[0] for m in matches}, {m[1] for m in matches}
        return matches, [k for k in track_idx if k not in hit_t], [k for k in det_idx if k not in hit_d]

    def associate_stream(self, s, cost, det, size):
        """Step 5 of an update for stream s.  cost: float [max_tracks, q] (cp_track_cost's block of the stream), det: float [q, 5],
        size: (W, H) of the frame.  -> (int64 [k, 5] of (x1, y1, x2, y2, track_id), list of (feature slot, track slot, ring position)
        entries, the indices global over the streams)."""
        q, Tcap = self.q, self.max_tracks
        cost, det = np.asarray(cost).reshape(Tcap, q), np.asarray(det, np.float64).reshape(q, 5)
        tracks = self.tracks[s]
        # detections: the boxes truncated toward zero as the demo does (demo_main.py:185-190), highest score first
        box = np.trunc(det[:, :4])
        tlwh_all = np.stack([box[:, 0], box[:, 1], box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]], 1)
        live = [d for d in range(q) if tlwh_all[d, 3] > 0]                      # an unused slot is all zeros: h = 0
        scores = det[live, 4]
        slots = [live[i] for i in np.argsort(scores)[::-1]]                     # detection index -> detection slot
        tlwh = tlwh_all[slots]
        xyah = np.array([_xyah(b) for b in tlwh]).reshape(-1, 4)
        nd = len(slots)
        # matching cascade over the confirmed tracks, most recently seen first
        confirmed = [i for i, t in enumerate(tracks) if t.state == CONFIRMED]
        matches, free_d = [], list(range(nd))
        for level in range(self.max_age):
            if not free_d:
                break
            idx = [i for i in confirmed if tracks[i].time_since_update == 1 + level]
            if not idx:
                continue
            c = np.array([[cost[tracks[i].slot, slots[d]] for d in free_d] for i in idx], np.float64)
            for r, i in enumerate(idx):
                c[r, kf_gating_distance(tracks[i].mean, tracks[i].covariance, xyah[free_d]) > GATE_4DOF] = GATED_COST
            m, _, free_d = self._min_cost_matching(c, self.max_cosine_distance, idx, free_d)
            matches += m
        matched_t = {m[0] for m in matches}
        left = [i for i in confirmed if i not in matched_t]
        # IoU matching: unconfirmed tracks and the confirmed ones missed for this frame only
        idx = [i for i, t in enumerate(tracks) if t.state != CONFIRMED] + [i for i in left if tracks[i].time_since_update == 1]
        missed = [i for i in left if tracks[i].time_since_update != 1]
        if idx and free_d:
            c = np.zeros((len(idx), len(free_d)))
            for r, i in enumerate(idx):
                c[r] = GATED_COST if tracks[i].time_since_update > 1 else 1.0 - _iou(tracks[i].tlwh(), tlwh[free_d])
            m, un_t, free_d = self._min_cost_matching(c, self.max_iou_distance, idx, free_d)
        else:
            m, un_t = [], idx
        matches += m
        missed += un_t
        # track updates
        table = []
        self.assignments[s] = -1

        def append(t, d):
            table.append((s * q + slots[d], s * Tcap + t.slot, t.appended % self.budget))
            t.appended += 1

        for i, d in matches:
            t = tracks[i]
            t.mean, t.covariance = kf_update(t.mean, t.covariance, xyah[d])
            t.hits += 1
            t.time_since_update = 0
            if t.state == TENTATIVE and t.hits >= self.n_init:
                t.state = CONFIRMED
            self.assignments[s, slots[d]] = t.track_id
            append(t, d)
        for i in missed:
            t = tracks[i]
            if t.state == TENTATIVE or t.time_since_update > self.max_age:
                t.state = DELETED
        for d in free_d:
            if not self.free[s]:
                self.dropped[s] += 1
                continue
            mean, cov = kf_initiate(xyah[d])
            t = Track(self.next_id[s], self.free[s].pop(0), mean, cov)
            self.next_id[s] += 1
            tracks.append(t)
            append(t, d)
        for t in tracks:
            if t.state == DELETED:
                self.free[s].append(t.slot)
        self.free[s].sort()
        self.tracks[s] = tracks = [t for t in tracks if t.state != DELETED]
        # what DeepSort.update returns (deep_sort.py:48-72)
        W, H = int(size[0]), int(size[1])
        out = []
        for t in tracks:
            if t.state != CONFIRMED or t.time_since_update > 1:
                continue
            x1, y1, w, h = t.tlwh()
            x1, y1 = max(x1, 0), max(y1, 0)
            out.append((int(x1), int(y1), min(int(x1 + w), W - 1), min(int(y1 + h), H - 1), t.track_id))
        return np.array(out, np.int64).reshape(-1, 5), table

    def associate(self, cost, det, sizes):
        """Step 5 of an update for every stream.  cost: host float [streams, max_tracks, q], det: host float [streams, q, 5], sizes:
        (W, H) per stream -> (list over streams of int64 [k, 5], append table int32 [n, 3])."""
        if len(sizes) != self.streams:
            raise ValueError("%d sizes for %d streams" % (len(sizes), self.streams))
        cost = np.asarray(cost).reshape(self.streams, self.max_tracks, self.q)
        det = np.asarray(det).reshape(self.streams, self.q, 5)
        outs, table = [], []
        for s in range(self.streams):
            o, t = self.associate_stream(s, cost[s], det[s], sizes[s])
            outs.append(o)
            table += t
        return outs, np.array(table, np.int32).reshape(-1, 3)

    # ------------------------------------------------------------------ the device call
    def _check(self, rows, result, sizes):
        if not isinstance(result, ReidResult):
            raise ValueError("result must be the ReidResult of the call's rows (got %s)" % type(result).__name__)
        rows = check_rows(rows, None, self.device, "the gallery is on %s; there is no CPU fallback", what="a CUDA tensor", one="stream",
                          f32="torch.float32")
        for name, t, dtype in (("result.features", result.features, torch.float32), ("result.slots", result.slots, torch.int32)):
            if not isinstance(t, torch.Tensor):
                raise _lib.CenterposeHipError("%s must be a CUDA tensor on the device (got %s): there is no CPU fallback"
                                              % (name, type(t).__name__))
            if not t.is_cuda or (self.device is not None and t.device != self.device):
                raise _lib.CenterposeHipError("%s on %s, the gallery is on %s; there is no CPU fallback" % (name, t.device, self.device))
            if t.dtype != dtype:
                raise _lib.CenterposeHipError("%s must be %s (got %s)" % (name, dtype, t.dtype))
        if self.device is None:
            raise _lib.CenterposeHipError("this tracker was built without a device (device=None): update needs the gallery on the GPU")
        if rows.shape[0] != self.streams:
            raise ValueError("rows hold %d frames, the tracker has %d streams: frame n of a call belongs to stream n"
                             % (rows.shape[0], self.streams))
        if tuple(result.features.shape) != (self.capacity, DIM) or tuple(result.slots.shape) != (self.capacity,):
            raise ValueError("the result holds features %s and slots %s, the tracker was built for capacity %d: [%d, %d] and [%d]"
                             % (tuple(result.features.shape), tuple(result.slots.shape), self.capacity, self.capacity, DIM, self.capacity))
        if len(sizes) != self.streams:
            raise ValueError("%d sizes for %d streams" % (len(sizes), self.streams))
        if rows.shape[0] * rows.shape[1] > 1 << 24:
            raise ValueError("%d x %d rows are too many for one call (at most 2^24)" % (rows.shape[0], rows.shape[1]))
        return rows.detach().contiguous()

    def update(self, rows, result, sizes):
        """One frame per stream -> list over streams of int64 [k, 5] arrays (x1, y1, x2, y2, track_id): what ``DeepSort.update`` returns,
        the confirmed tracks seen in this frame or the one before, boxes clipped to the frame.
        rows: CUDA float32 [streams, M, 56] in image coordinates (run_batch(..., return_device=True)); result: the ReidResult of these
        rows from an extractor of this tracker's capacity; sizes: (W, H) of every frame.  Host arrays raise: no CPU fallback.
        Steps: Kalman predict on the host; the ring lengths go up (the first of two small uploads); cp_track_cost_f32; ONE download of
        costs and boxes; association per stream on the host; the append table goes up; cp_track_append_f32.  The download is the
        call's one synchronisation and it is inherent: the identities are host data and the next frame's matching depends on them.
        `result.counts[n] > q` is not an error: rows beyond a stream's q slots were not embedded and are not tracked."""
        rows = self._check(rows, result, sizes)
        S, Tcap, q, M = self.streams, self.max_tracks, self.q, int(rows.shape[1])
        glen = self.begin()
        L, vp = _lib.lib(), ctypes.c_void_p
        features = result.features.detach().contiguous()
        with torch.cuda.device(self.device):
            glen_dev, = self._io.upload_table([glen])
            _lib.check(L.cp_track_cost_f32(vp(self.gallery.data_ptr()), vp(self.ginv.data_ptr()), vp(glen_dev.data_ptr()),
                                           vp(features.data_ptr()), vp(result.slots.data_ptr()), vp(rows.data_ptr()), M, S, Tcap,
                                           self.budget, q, vp(self.out.data_ptr()), _lib.stream()), "cp_track_cost_f32")
            host = self.out.cpu().numpy()                                          # the one download: costs and boxes
            outs, table = self.associate(host[:S * Tcap * q], host[S * Tcap * q:], sizes)
            if len(table):
                table_dev, = self._io.upload_table([table])
                _lib.check(L.cp_track_append_f32(vp(self.gallery.data_ptr()), vp(self.ginv.data_ptr()), vp(features.data_ptr()),
                                                 vp(table_dev.data_ptr()), len(table), self.budget, _lib.stream()), "cp_track_append_f32")
        return outs

    def row_ids(self, result, M):
        """The identities of the last `update`, per detection row -> CUDA int32 [streams, M]: the id of the track matched to row (n, m),
        -1 everywhere else (a detection that started a track is not a match: `assignments`' rule).  result: the ReidResult given to that
        update, M: its rows per frame.  `assignments` goes up as one small table, cp_track_row_ids fills and scatters in the current
        stream: nothing is downloaded and nothing synchronises."""
        if self.device is None:
            raise _lib.CenterposeHipError("this tracker was built without a device (device=None): row_ids needs the GPU")
        if not isinstance(result, ReidResult):
            raise ValueError("result must be the ReidResult of the last update (got %s)" % type(result).__name__)
        slots, M = result.slots, int(M)
        if not isinstance(slots, torch.Tensor) or not slots.is_cuda or slots.device != self.device:
            raise _lib.CenterposeHipError("result.slots must be a CUDA tensor on %s; there is no CPU fallback" % self.device)
        if slots.dtype != torch.int32 or tuple(slots.shape) != (self.capacity,):
            raise ValueError("result.slots must be int32 [%d] (got %s %s)" % (self.capacity, slots.dtype, tuple(slots.shape)))
        if M < 0 or self.streams * M > 1 << 24:
            raise ValueError("%d x %d rows are too many for one call (at most 2^24)" % (self.streams, M))
        ids = self.assignments.astype(np.int32)
        if not np.array_equal(ids, self.assignments):
            raise ValueError("a track id does not fit 32 bits")
        slots = slots.detach().contiguous()
        with torch.cuda.device(self.device):
            out = torch.empty((self.streams, M), dtype=torch.int32, device=self.device)
            ids_dev, = self._io.upload_table([ids])
            vp = ctypes.c_void_p
            _lib.check(_lib.lib().cp_track_row_ids(vp(slots.data_ptr()), vp(ids_dev.data_ptr()), self.capacity, self.streams, self.q, M,
                                                   vp(out.data_ptr()), _lib.stream()), "cp_track_row_ids")
        return out
