"""Same-process A/B of the head pose and the face overlays on the device against what a caller had to do without them:

  (a)  rows = run_batch(frames, return_device=True), then FaceAligner.align(frames, rows=rows) detection and alignment, all on the device
  (b)  (a) with align(..., pose=True), then FaceAligner.draw with the default style            + the two head-pose launches (csrc/face_pose.hip)
                                                                                               and the two overlay launches (csrc/face_draw.hip)
  (c)  (a), then FaceResult.vertices(face_ind), the 43 867 x 3 floats of every face to the host and estimate_pose in NumPy per face
       (np.linalg.svd; demo/face/utils/estimate_pose.py:67-99 restated), the frame and the landmarks to the host, the host painter
       (cp_face_draw_frames_host, default style) and the frame back to the device
  (c') (a), then a torch float64 restatement on the device (gather, means, covariance, torch.linalg.svd, batched over the faces) and
       the download of P only (no painting)

Every call aligns the detector's own rows of one 480 x 640 frame at its VIS_THRESH; the frames are such that all `capacity` slots are
taken (asserted), so all paths pose the same 8 faces.  (b) and (c) paint a scratch copy of the frame that is made before any timing, so
every call detects on clean frames; after the cross-check their pictures must be equal byte for byte.  Frames: random bytes with
large-scale structure, on the device before any timing; dla_34 preset as shipped; synthetic weights; stand-in tables (43 867 distinct
random cells and a random cloud: the product ships no reference data -- the work does not depend on their values).  Before timing,
(b)'s P is compared with (c)'s and (c')'s: 1e-9 of its largest entry, and its rotation part to 1e-6 of its own largest entry (the
covariance of random tables is badly conditioned next to a real face's; a wrong vertex order would be off by far more).  Every path is warmed, then timed for at least --seconds of work per
round; five or more rounds alternate the order of the paths.  Per path: wall ms per call as min / median over rounds and the spread
(max - min) / median; this - (a) from the medians.  There is no pass mark.

  --kernels K   instead of the A/B: K align(pose=True) + draw calls on given boxes (the default style and all three layers in turn)
                and nothing else, for a kernel trace of its own
                (rocprofv3 --kernel-trace --stats -- python tools/face_pose_ab.py --kernels 20)
usage: python tools/face_pose_ab.py [--capacity 8] [--vertices 43867] [--rounds 5] [--seconds 0.5]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def numpy_pose(p0, p1):
    m0, m1 = p0.mean(0), p1.mean(0)
    a, b = p0 - m0, p1 - m1
    U, _, Vt = np.linalg.svd(a.T @ b)
    R = U @ Vt
    if np.linalg.det(R) < 0:
        R[:, 2] *= -1
    s = np.sqrt(np.mean(np.sum(a * a, 1))) / np.sqrt(np.mean(np.sum(b * b, 1)))
    return np.c_[s * R, m0 - m1]


def torch_pose(v, can):
    """v [F, V, 3] float32 on the device, can [V, 3] float64 -> P [F, 3, 4] float64, batched."""
    p0 = v.double()
    m0, m1 = p0.mean(1, keepdim=True), can.mean(0, keepdim=True)
    a, b = p0 - m0, can - m1
    U, _, Vt = torch.linalg.svd(a.transpose(1, 2) @ b)
    R = U @ Vt
    flip = torch.linalg.det(R) < 0
    R[:, :, 2] = torch.where(flip[:, None], -R[:, :, 2], R[:, :, 2])
    s = torch.sqrt((a * a).sum(2).mean(1)) / torch.sqrt((b * b).sum(1).mean())
    return torch.cat([s[:, None, None] * R, (m0 - m1).transpose(1, 2)], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=8)
    ap.add_argument("--vertices", type=int, default=43867)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--kernels", type=int, default=0)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("at least five alternating rounds")
    import face_ab
    from centerpose_amd import config, detector, face, synth
    r = np.random.RandomState(11)
    face_ind = r.permutation(65536)[:a.vertices]
    canonical = r.normal(0.0, 60.0, (a.vertices, 3))
    al = face.FaceAligner(synth.make_state_dict("prnet", seed=317), face_ab.uv_table(), capacity=a.capacity, face_ind=face_ind,
                          canonical_vertices=canonical)
    sets = [face_ab.device_frames(1, 480, 640, 300 + 10 * i) for i in range(2)]
    boxes = torch.tensor([[[60.0 + 50 * k, 80.0 + 10 * k, 180.0 + 50 * k, 230.0 + 10 * k, 1.0] for k in range(a.capacity)]], device="cuda")
    from centerpose_amd import draw as _draw
    draw_all = _draw.FaceStyle(vertices=True, pose_box=True)
    if a.kernels:
        canvas = [f.clone() for f in sets[0]]
        for k in range(a.kernels):
            res = al.align(sets[0], boxes=boxes, pose=True)
            al.draw(canvas, res, style=None if k % 2 == 0 else draw_all)
        torch.cuda.synchronize()
        return
    det = detector.MultiPoseDetector(config.get_cfg("dla_34"))
    can_dev = torch.from_numpy(canonical).cuda()
    ind_dev = torch.from_numpy(face_ind.astype(np.int64)).cuda()

    vis = float(det.cfg.TEST.VIS_THRESH)

    def path_a(i):
        return al.align(sets[i & 1], rows=det.run_batch(sets[i & 1], return_device=True), vis_thresh=vis)

    canvas = [[f.clone() for f in s] for s in sets]                # what (b) and (c) paint: the detector always sees clean frames
    from centerpose_amd import _lib, draw, frames as fr
    L, style = _lib.lib(), draw.FaceStyle().struct()

    def path_b(i):
        res = al.align(sets[i & 1], rows=det.run_batch(sets[i & 1], return_device=True), vis_thresh=vis, pose=True)
        al.draw(canvas[i & 1], res)
        return res.pose.P

    def host_paint(frame, res):
        """the frame and the landmarks to the host, the host painter, the frame back"""
        pic, lm, slots = frame.cpu().numpy(), res.landmarks.cpu().numpy(), res.slots.cpu().numpy()
        d = np.zeros(1, fr.FRAME_DESC)
        d["base"], d["row_stride"], d["pix_stride"], d["ch_off"] = pic.ctypes.data, pic.strides[0], pic.strides[1], (0, 1, 2)
        d["H"], d["W"], d["NH"], d["NW"], d["mid_off"] = pic.shape[0], pic.shape[1], pic.shape[0], pic.shape[1], -1
        rc = L.cp_face_draw_frames_host(d.ctypes.data, 1, slots.ctypes.data, a.capacity, lm.ctypes.data, None, None, None, None, 0,
                                        style.ctypes.data)
        assert rc == 0, L.cp_last_error()
        frame.copy_(torch.from_numpy(pic))

    def path_c(i):
        res = path_a(i)
        v = res.vertices(face_ind).cpu().numpy().astype(np.float64)                # the download the device path does not have
        P = np.stack([numpy_pose(f, canonical) for f in v])
        host_paint(canvas[i & 1][0], res)
        return P

    def path_d(i):
        res = path_a(i)
        v = res.pos.reshape(a.capacity, 65536, 3)[:, ind_dev]
        return torch_pose(v, can_dev).cpu()

    res = path_b(0)
    torch.cuda.synchronize()
    for i in range(2):
        rows = det.run_batch(sets[i], return_device=True)
        valid = al.align(sets[i], rows=rows, vis_thresh=vis, pose=True).pose.valid.cpu().tolist()
        assert valid == [1] * a.capacity, "frame set %d: fewer than %d faces (%s)" % (i, a.capacity, valid)
    P = res.cpu().numpy()
    device_picture = canvas[0][0].clone()
    canvas[0][0].copy_(sets[0][0])
    for name, other in (("NumPy", path_c(0)), ("torch", path_d(0).numpy())):
        d = float(np.abs(P - other).max() / np.abs(P).max())
        d_r = float((np.abs(P - other)[:, :, :3].max(axis=(1, 2)) / np.abs(P[:, :, :3]).max(axis=(1, 2))).max())
        print("P of (b) against the %s path: %.2e of its largest entry, s R %.2e of its largest entry" % (name, d, d_r))
        assert d <= 1e-9 and d_r <= 1e-6
        if name == "NumPy":
            assert torch.equal(canvas[0][0], device_picture) and not torch.equal(device_picture, sets[0][0]), "the two painters disagree"
    paths = {"a": ("(a) run_batch + align", path_a), "b": ("(b) run_batch + align(pose=True) + draw", path_b),
             "c": ("(c) (a) + vertices to the host + NumPy estimate_pose + host painter", path_c),
             "d": ("(c') (a) + torch float64 restatement on the device + P to the host", path_d)}
    keys, steps = list("abcd"), {}
    for k in keys:
        for i in range(2):
            paths[k][1](i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(3):
            paths[k][1](i)
        torch.cuda.synchronize()
        steps[k] = max(3, int(math.ceil(a.seconds / ((time.perf_counter() - t0) / 3))))
    ms = {k: [] for k in keys}
    for rnd in range(a.rounds):
        for k in (keys if rnd % 2 == 0 else keys[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps[k]):
                paths[k][1](i)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps[k])
    med = {k: sorted(ms[k])[len(ms[k]) // 2] for k in keys}
    out = {}
    for k in keys:
        v, lo = med[k], min(ms[k])
        spread = 100.0 * (max(ms[k]) - lo) / v
        extra = None if k == "a" else v - med["a"]
        out[k] = {"path": paths[k][0], "ms_per_call_median": round(v, 4), "ms_per_call_min": round(lo, 4), "spread_pct": round(spread, 2),
                  "steps_per_round": steps[k], "minus_a_ms_per_call": None if extra is None else round(extra, 4),
                  "rounds_ms": [round(t, 4) for t in ms[k]]}
        print("480x640 N=1 cap=%-3d V=%-6d %-72s min %8.3f  median %8.3f ms/call  spread %5.1f %%  %s  (%d steps x %d rounds)"
              % (a.capacity, a.vertices, paths[k][0], lo, v, spread, "                     " if extra is None else "this - (a) = %+8.3f" % extra,
                 steps[k], len(ms[k])), flush=True)
    print(json.dumps({"rounds": a.rounds, "seconds": a.seconds, "capacity": a.capacity, "vertices": a.vertices, "paths": out}))


if __name__ == "__main__":
    main()
