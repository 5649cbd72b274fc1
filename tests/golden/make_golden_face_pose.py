"""Records tests/golden/face_pose.npz from the reference's own estimate_pose (demo/face/utils/estimate_pose.py), imported by path:

    python tests/golden/make_golden_face_pose.py [path of the reference checkout]

(default: $CP_REFERENCE, or a directory `reference` beside the repository).  The file holds every 16th entry of the reference's
face_ind and canonical_vertices (2 742 vertices), the numbers 24 synthetic cases are rebuilt from (tests/face_pose_ref.py: the canonical
cloud rotated by up to +-1.2 rad per axis, scaled 0.2..6, translated -500..8000 px, with uniform noise; case 1 is reflected) with a
checksum of their float32 vertices, and what the reference computes for each: compute_similarity_transform, P2sRt and matrix2angle
called the way estimate_pose() calls them (:94-97), fed FLOAT64 COPIES of the float32 vertices (the reference's vertices are float64;
fed float32 it would compute its means in float32).

Asserted here, on the reference alone, so that no test has to leave a case out: sigma_min / sigma_max of the covariance >= 0.05,
|R[2, 0]| <= 0.999, and every box corner before truncation at least 1e-6 from a whole number."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import face_pose_ref as ref  # noqa: E402

STEP, CASES = 16, 24


def rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def main():
    reference = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CP_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
    utils = os.path.join(reference, "demo", "face", "utils")
    spec = importlib.util.spec_from_file_location("reference_estimate_pose", os.path.join(utils, "estimate_pose.py"))
    ep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ep)
    face_ind = np.loadtxt(os.path.join(utils, "uv_data", "face_ind.txt")).astype(np.int32)[::STEP]
    canonical = np.load(os.path.join(utils, "uv_data", "canonical_vertices.npy")).astype(np.float64)[::STEP]
    assert face_ind.shape == (2742,) and canonical.shape == (2742, 3)

    r = np.random.RandomState(2025)
    out = {k: [] for k in ("case_R", "case_s", "case_t", "case_seed", "case_amp", "case_crc", "P", "s", "R", "angles")}
    worst_cond, worst_r20, worst_frac = 1.0, 0.0, 1.0
    for k in range(CASES):
        R = rotation(*r.uniform(-1.2, 1.2, 3))
        if k == 1:
            R = R @ np.diag([1.0, 1.0, -1.0])                     # a reflected cloud: the reference's det fix is taken
        s = float(np.exp(r.uniform(np.log(0.2), np.log(6.0))))
        t = r.uniform(-500.0, 8000.0, 3)
        seed, amp = 7000 + k, float(r.choice([0.0, 0.5, 2.0, 8.0])) * s
        v32 = ref.case_vertices(canonical, R, s, t, seed, amp)
        v64 = v32.astype(np.float64)
        # estimate_pose.py:94-97
        P = ep.compute_similarity_transform(v64, canonical)
        s_rec, R_rec, _ = ep.P2sRt(P)
        pose = ep.matrix2angle(R_rec)
        # the bars of the recording
        sv = np.linalg.svd((v64 - v64.mean(0)).T @ (canonical - canonical.mean(0)), compute_uv=False)
        frac = np.abs(ref.box_float(P, ref.case_landmarks(v32)) - np.rint(ref.box_float(P, ref.case_landmarks(v32)))).min()
        worst_cond, worst_r20, worst_frac = min(worst_cond, sv[-1] / sv[0]), max(worst_r20, abs(R_rec[2, 0])), min(worst_frac, frac)
        assert sv[-1] / sv[0] >= 0.05 and abs(R_rec[2, 0]) <= 0.999 and frac >= 1e-6, (k, sv, R_rec[2, 0], frac)
        for key, val in (("case_R", R), ("case_s", s), ("case_t", t), ("case_seed", seed), ("case_amp", amp), ("case_crc", ref.checksum(v32)),
                         ("P", P), ("s", s_rec), ("R", R_rec), ("angles", np.asarray(pose, np.float64))):
            out[key].append(val)
    arrays = {k: np.asarray(v) for k, v in out.items()}
    arrays["case_crc"] = arrays["case_crc"].astype(np.uint32)
    path = os.path.join(HERE, "face_pose.npz")
    np.savez_compressed(path, face_ind=face_ind, canonical_vertices=canonical, **arrays)
    size = os.path.getsize(path)
    assert size <= 225 * 1024, size
    print("face_pose.npz: %d bytes, %d cases; sigma_min / sigma_max >= %.3f, |R[2,0]| <= %.4f, box corners >= %.2e from a whole number"
          % (size, CASES, worst_cond, worst_r20, worst_frac))


if __name__ == "__main__":
    main()
