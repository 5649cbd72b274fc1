"""The head pose, independently of csrc/face_pose_arith.h: a NumPy float64 statement of estimate_pose (the reference's
demo/face/utils/estimate_pose.py:67-99) with np.linalg.svd and two-pass centring, the corners of plot_pose_box (cv_plot.py:48-70),
and the synthetic cases the recording (tests/golden/make_golden_face_pose.py) and the tests both build.

A case is built from stored numbers by elementwise IEEE operations only (no BLAS product, no libm call, uniform noise from
RandomState.random_sample), so the float32 vertices come out with the same bits wherever they are rebuilt; the recording carries a
checksum of them."""
import zlib
from math import asin, atan2, cos

import numpy as np

N_LANDMARKS = 68
LANDMARK_STEP = 40          # landmark k of a case is its vertex k * 40


def similarity(p0, p1):
    """compute_similarity_transform: p0 [V, 3] the vertices, p1 [V, 3] the canonical cloud, float64 -> (P [3, 4], s, R)."""
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    m0, m1 = p0.mean(axis=0), p1.mean(axis=0)
    a, b = p0 - m0, p1 - m1
    U, _, Vt = np.linalg.svd(a.T @ b)
    R = U @ Vt
    if np.linalg.det(R) < 0:
        R[:, 2] *= -1
    s = np.sqrt(np.mean(np.sum(a * a, axis=1))) / np.sqrt(np.mean(np.sum(b * b, axis=1)))
    return np.c_[s * R, m0 - m1], s, R


def angles(P):
    """P2sRt, then matrix2angle -> (x, y, z)."""
    r1, r2 = P[0, :3] / np.linalg.norm(P[0, :3]), P[1, :3] / np.linalg.norm(P[1, :3])
    r3 = np.cross(r1, r2)
    x = asin(min(1.0, max(-1.0, r3[0])))
    return np.asarray([x, atan2(r3[1] / cos(x), r3[2] / cos(x)), atan2(r2[0] / cos(x), r1[0] / cos(x))])


def box_float(P, landmarks):
    """The ten corners before truncation, float64 [10, 2]."""
    pts = []
    for size, depth in ((90.0, 0.0), (105.0, 110.0)):
        pts += [(-size, -size, depth), (-size, size, depth), (size, size, depth), (size, -size, depth), (-size, -size, depth)]
    homo = np.hstack([np.asarray(pts, np.float64), np.ones((10, 1))])
    p2 = homo.dot(np.asarray(P, np.float64).T)[:, :2]
    return p2 - p2[:4].mean(axis=0) + np.asarray(landmarks, np.float32).astype(np.float64)[:27, :2].mean(axis=0)


def box(P, landmarks):
    return np.trunc(np.clip(box_float(P, landmarks), -16384, 16383)).astype(np.int32)


def pose(vertices32, canonical, landmarks32):
    """-> dict(P, angles, scale, box, valid) for one slot's float32 vertices."""
    v = np.asarray(vertices32, np.float32).astype(np.float64)
    zero = dict(P=np.zeros((3, 4)), angles=np.zeros(3), scale=0.0, box=np.zeros((10, 2), np.int32), valid=0)
    if not np.isfinite(v).all() or not (np.abs(v - v.mean(axis=0)).max() > 0):
        return zero
    P, s, _ = similarity(v, canonical)
    return dict(P=P, angles=angles(P), scale=s, box=box(P, landmarks32), valid=1)


# ---- the synthetic cases ------------------------------------------------------------------------------------------------------------
def case_vertices(canonical, R, s, t, seed, amp):
    """float32 [V, 3]: (s * R canonical + t + uniform noise of width amp), elementwise float64, rounded once to float32."""
    c = np.asarray(canonical, np.float64)
    out = np.empty_like(c)
    for i in range(3):
        out[:, i] = ((c[:, 0] * R[i, 0] + c[:, 1] * R[i, 1]) + c[:, 2] * R[i, 2]) * s + t[i]
    noise = (np.random.RandomState(int(seed)).random_sample(c.shape) - 0.5) * amp
    return (out + noise).astype(np.float32)


def case_landmarks(vertices32):
    return np.ascontiguousarray(vertices32[::LANDMARK_STEP][:N_LANDMARKS])


def checksum(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def cases_of(g):
    """The recorded cases of tests/golden/face_pose.npz -> list of dicts with the rebuilt vertices (checksum verified)."""
    out = []
    for k in range(len(g["case_s"])):
        v = case_vertices(g["canonical_vertices"], g["case_R"][k], g["case_s"][k], g["case_t"][k], g["case_seed"][k], g["case_amp"][k])
        assert checksum(v) == int(g["case_crc"][k]), "case %d: the rebuilt vertices are not the recorded ones" % k
        out.append(dict(vertices=v, landmarks=case_landmarks(v), P=g["P"][k], s=g["s"][k], R=g["R"][k], angles=g["angles"][k]))
    return out


def place(vertices32, face_ind, fill=0.0):
    """A restored position map [256, 256, 3] float32 holding vertex v in cell face_ind[v] (face_ind without duplicates)."""
    pos = np.full((256 * 256, 3), fill, np.float32)
    pos[np.asarray(face_ind)] = vertices32
    return pos.reshape(256, 256, 3)
