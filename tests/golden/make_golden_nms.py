"""Golden vectors for soft_nms_39 from the REFERENCE'S OWN SOURCE (build container only; the reference never travels).

`lib/external/nms.pyx` does not compile here (Cython 3 / numpy 2 reject `np.int_t`, `np.float` elsewhere in the file), but the body of
`soft_nms_39` (nms.pyx:172-275) is plain Python once its Cython-only syntax is gone.  `load_reference_soft_nms_39` reads the file where it
lies, cuts that one function out IN MEMORY, drops the `cdef` declaration lines (keeping the initialisers: `cdef unsigned int N =
boxes.shape[0]` becomes `N = boxes.shape[0]`), reduces the typed signature to its parameter names and exec()s the rest -- every
statement of the algorithm is the reference's, untouched.  What changes is the arithmetic type of the scalars: a `cdef float` variable is
a C float; here the values read from the float32 array are numpy float32 scalars and stay float32 through Python int / float operands
(NEP 50, numpy >= 2), so sums, products, comparisons and the discard / swap decisions are those of the C code.  One call differs in its
last bit: `np.exp(-(ov*ov)/sigma)` is evaluated in float32 here and in double-then-rounded there, so every Gaussian decay is pinned to
1 ulp (a score takes one decay per overlapping better box: the tests allow 5e-6 relative on column 4 for method 2), everything else --
box moves, the 0:39-only swap, discards, `keep`, and the scores of the hard / linear methods -- bit for bit.

    python tests/golden/make_golden_nms.py          # writes tests/golden/soft_nms_39.npz and soft_nms_39_edges.npz
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PYX = "/root/reference/lib/external/nms.pyx"


def load_reference_soft_nms_39(path=PYX):
    src = open(path).read()
    body = src[src.index("def soft_nms_39("):src.index("def soft_nms_merge(")]
    out = []
    for line in body.splitlines():
        m = re.match(r"^(\s*)cdef\s+(?:unsigned\s+)?\w+\s+(.*)$", line)
        if m:                                   # a declaration: keep a single-variable initialiser, drop the rest
            if "=" in m.group(2) and "," not in m.group(2):
                out.append(m.group(1) + m.group(2))
            continue
        out.append(line)
    # typed signature -> parameter names with their defaults: "np.ndarray[float, ndim=2] boxes, float sigma=0.5, ..., unsigned int method=0"
    sig = re.match(r"def soft_nms_39\((.*)\):", out[0]).group(1)
    sig = re.sub(r"np\.ndarray\[[^\]]*\]\s*", "", sig)
    sig = re.sub(r"\b(?:unsigned\s+int|float|int)\s+", "", sig)
    out[0] = "def soft_nms_39(%s):" % sig
    assert out[0] == "def soft_nms_39(boxes, sigma=0.5, Nt=0.3, threshold=0.001, method=0):", out[0]
    ns = {"np": np}
    exec("\n".join(out), ns)
    return ns["soft_nms_39"]


def cases():
    """name -> (boxes float32 [N,56], kwargs) -- seeded; the detector's own call is soft_nms_39(results, Nt=0.5, method=2)
    (lib/detectors/multi_pose.py:76-77)."""
    out = {}
    r = np.random.RandomState(317)
    for method in (0, 1, 2):
        b = r.rand(60, 56).astype(np.float32)
        b[:, 2:4] = b[:, 0:2] + r.rand(60, 2).astype(np.float32) * 0.8 + 0.05
        b[:, :4] *= 40
        out["rand60_m%d" % method] = (b, dict(sigma=0.5, Nt=0.5, threshold=0.05, method=method))
    # two scales of the same people merged (what merge_outputs stacks): boxes in clusters, default threshold
    centres = r.rand(12, 2).astype(np.float32) * 400 + 50
    rows = []
    for s in range(2):
        for c in centres:
            for _ in range(4):
                wh = (r.rand(2) * 60 + 40).astype(np.float32)
                j = (r.randn(2) * 6).astype(np.float32)
                row = r.rand(56).astype(np.float32)
                row[0:2] = c + j - wh / 2
                row[2:4] = c + j + wh / 2
                row[4] = r.rand() * 0.9 + 0.05
                rows.append(row)
    out["people_2scales_detector_call"] = (np.stack(rows).astype(np.float32), dict(Nt=0.5, method=2))
    b = np.zeros((5, 56), np.float32)                                        # hand-checkable: identical / nested / disjoint boxes
    b[:, :4] = [[0, 0, 10, 10], [0, 0, 10, 10], [2, 2, 8, 8], [50, 50, 60, 60], [0, 0, 10, 10]]
    b[:, 4] = [0.5, 0.9, 0.7, 0.8, 0.0011]
    for i in range(5):
        b[i, 5:39] = i + 1
        b[i, 39:] = 10 * (i + 1)
    for method in (0, 1, 2):
        out["hand_m%d" % method] = (b.copy(), dict(Nt=0.5, method=method))
    return out


def _rows(boxes, scores):
    """[R,56]: integer corners, the scores, and per row distinct values in columns 5..38 (moved with the box) and 39..55 (never moved)."""
    R = len(boxes)
    b = np.zeros((R, 56), np.float32)
    b[:, :4] = np.asarray(boxes, np.float32).reshape(R, 4)
    b[:, 4] = np.asarray(scores, np.float32)
    b[:, 5:39] = (np.arange(R) + 1)[:, None]
    b[:, 39:] = (np.arange(R) + 1001)[:, None]
    return b


def _disjoint(k):
    """Box k of a grid of pairwise disjoint 11 x 11 boxes."""
    x, y = (k % 32) * 20, (k // 32) * 20
    return [x, y, x + 10, y + 10]


def _clustered(seed, R, clusters=8, spread=3):
    """Integer boxes around a few centres (heavy overlaps: decays and discards) with scores k / 16 (many exactly equal)."""
    r = np.random.RandomState(seed)
    c = r.randint(0, 12, (clusters, 2)) * 40
    rows = []
    for _ in range(R):
        x, y = c[r.randint(clusters)] + r.randint(-spread, spread + 1, 2)
        w, h = r.choice([8, 10, 12], 2)
        rows.append([x, y, x + w, y + h])
    return _rows(rows, r.randint(1, 17, R) / 16.0)


def edge_cases():
    """name -> (boxes float32 [R,56], kwargs): exact ties and limits.  Integer corners and dyadic scores, methods 0 and 1 (and method 2
    on pairwise disjoint boxes, where no decay happens), so the areas, the IoU quotients named below, the decays and the thresholds
    are exact and every decision is hit exactly, not approached."""
    out = {}
    A, A_half, A_most = [0, 0, 9, 9], [0, 0, 9, 4], [0, 0, 9, 8]               # areas 100, 50, 90: IoU with A exactly 0.5 and 0.9
    C, C_above = [20, 20, 51, 51], [20, 20, 51, 36]                            # areas 1024, 544: IoU exactly 0.53125
    E, E_34 = [0, 0, 7, 7], [0, 0, 7, 5]                                       # areas 64, 48: IoU exactly 0.75
    far = [[100, 100, 110, 110], [200, 100, 210, 110], [300, 100, 310, 110]]
    up = lambda v, d: float(np.nextafter(np.float32(v), np.float32(d)))
    # IoU exactly on Nt: not greater, so the weight is 1; a pair just above Nt beside it
    for m in (0, 1):
        out["iou_on_nt_m%d" % m] = (_rows([A, A_half, C, C_above, far[0]], [0.875, 0.5, 0.75, 0.25, 0.375]), dict(Nt=0.5, method=m))
    # a decayed score exactly on the threshold (linear: 0.5 * (1 - 0.75) = 0.125): not below, so the row is kept; its neighbours
    for tag, sc in (("below", up(0.5, 0)), ("on", 0.5), ("above", up(0.5, 1))):
        out["decay_%s_threshold_m1" % tag] = (_rows([E, E_34, far[0]], [0.875, sc, 0.375]), dict(Nt=0.5, threshold=0.125, method=1))
    # hard NMS with threshold 0: nothing is below it, suppressed rows stay with score 0 -- and tie in every later arg-max
    out["threshold_zero_m0"] = (_rows([A, A_most, far[0], A_most, A_half, far[1]], [0.875, 0.5, 0.25, 0.75, 0.625, 0.25]),
                                dict(Nt=0.5, threshold=0.0, method=0))
    # equal scores: the lowest index wins; row i stays when it equals the best behind it
    out["equal_two"] = (_rows([_disjoint(k) for k in range(4)], [0.25, 0.5, 0.5, 0.125]), dict(Nt=0.5, method=0))
    out["equal_three_first_stays"] = (_rows([_disjoint(k) for k in range(6)], [0.5, 0.25, 0.5, 0.5, 0.125, 0.25]), dict(Nt=0.5, method=1))
    sc = np.full(66, 0.5)
    sc[0] = 0.25
    out["equal_65"] = (_rows([_disjoint(k) for k in range(66)], sc), dict(Nt=0.5, method=0))
    # the maximum at rows 69, 5 and 70 only: rows 5 and 69 are one lane's (64 apart), row 70 another's; the rest distinct and lower
    sc = (np.arange(130) + 1) / 512.0
    sc[[5, 69, 70]] = 0.75
    sc[[17, 81]] = 0.625
    out["equal_across_stride"] = (_rows([_disjoint(k) for k in range(130)], sc), dict(Nt=0.5, method=1))
    # method 2 on pairwise disjoint boxes: no decay ever happens, the order of equal scores is all there is
    r = np.random.RandomState(5)
    out["gaussian_disjoint_equal"] = (_rows([_disjoint(k) for k in range(70)], r.randint(1, 5, 70) / 8.0), dict(Nt=0.5, method=2))
    # discards
    hard = dict(Nt=0.5, method=0)
    out["discard_last_row"] = (_rows([A, far[0], A_most], [0.875, 0.5, 0.25]), hard)
    # row 1 is discarded; the row swapped in from the end is discarded at the same position, three times over
    out["discard_chain"] = (_rows([A, A_most, far[0], far[1], A_most, A_most, A_most], [0.875, 0.5, 0.625, 0.375, 0.25, 0.75, 0.125]), hard)
    out["discard_all_but_first"] = (_rows([A] + [A_most] * 5, [0.875, 0.5, 0.75, 0.25, 0.5, 0.125]), hard)
    # N shrinks down to i + 1 at i = 1: row 0 is disjoint and highest, every row behind the second overlaps it
    out["discard_down_to_i_plus_1"] = (_rows([far[0], A] + [A_most] * 4, [0.875, 0.75, 0.5, 0.25, 0.5, 0.125]), hard)
    # row counts around the 64 lanes, and the 512-row limit
    for R in (1, 2, 63, 64, 65):
        out["clustered_%d" % R] = (_clustered(900 + R, R), dict(Nt=0.5, method=R % 2))
    for m in (0, 1):
        out["clustered_512_m%d" % m] = (_clustered(77, 512, clusters=40), dict(Nt=0.5, threshold=0.0625, method=m))
    # three different 64-row images for ONE launch (same parameters): clustered, all disjoint with equal scores, one single cluster
    kw = dict(Nt=0.5, threshold=0.001, method=0)
    out["batch64_clustered"] = (_clustered(31, 64), kw)
    out["batch64_disjoint"] = (_rows([_disjoint(k) for k in range(64)], np.random.RandomState(32).randint(1, 4, 64) / 4.0), dict(kw))
    out["batch64_one_cluster"] = (_clustered(33, 64, clusters=1, spread=1), dict(kw))
    return out


def generate(which=cases):
    ref = load_reference_soft_nms_39()
    data = {}
    for name, (boxes, kw) in which().items():
        work = boxes.copy()
        keep = ref(work, **kw)
        data[name + "__out"] = work
        data[name + "__keep"] = np.asarray(keep, np.int32)
    return data


if __name__ == "__main__":
    d = generate()
    np.savez_compressed(os.path.join(HERE, "soft_nms_39.npz"), **d)
    e = generate(edge_cases)
    np.savez_compressed(os.path.join(HERE, "soft_nms_39_edges.npz"), **e)
    for k in sorted(d) + sorted(e):
        if k.endswith("__keep"):
            print(k[:-6], "kept", len(d[k] if k in d else e[k]))
