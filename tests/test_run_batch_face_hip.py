"""GPU: run_batch(..., face=aligner) -- the call's own rows through FaceAligner.align (with the head pose where the aligner has its
tables) before anything is painted: equal to run_batch followed by align bit for bit, the FaceResult appended as the last element of
what the call returns, together with return_device, embed and draw; without face= the result is what it was."""
import functools
import os

import numpy as np
import pytest
import torch

import face_pose_util as fpu
import face_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _aligners():
    from centerpose_amd import face, synth
    prn = dict(np.load(os.path.join(ROOT, "tests", "golden", "prn_maps.npz")))
    uv = np.loadtxt(os.path.join(ROOT, "tests", "golden", "prn_uv_kpt_ind.txt")).astype(np.int32)
    g = fpu.golden()
    sd = synth.make_state_dict("prnet", seed=int(prn["seed"]))
    return (face.FaceAligner(sd, uv, capacity=4, face_ind=g["face_ind"], canonical_vertices=g["canonical_vertices"]),
            face.FaceAligner(sd, uv, capacity=4))


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def _same_result(a, b):
    ok = all(_same(getattr(a, k), getattr(b, k)) for k in ("pos", "landmarks", "slots", "counts", "xform"))
    if a.pose is None or b.pose is None:
        return ok and a.pose is None and b.pose is None
    return ok and all(_same(getattr(a.pose, k), getattr(b.pose, k)) for k in ("P", "angles", "scale", "box", "valid"))


def test_run_batch_with_face():
    from centerpose_amd import config, detector
    det = detector.MultiPoseDetector(config.get_cfg("dla_34", TEST__FIX_RES=False))
    with_pose, without = _aligners()
    vis = float(det.cfg.TEST.VIS_THRESH)
    pics = [np.ascontiguousarray((face_ref.make_input(31 + n, 96, 128)[::-1].transpose(1, 2, 0) * 255).round().astype(np.uint8)) for n in range(2)]
    frames = [torch.from_numpy(p).cuda() for p in pics]
    plain = det.run_batch(frames, return_device=True)
    listed = det.run_batch(frames)
    assert int((plain[..., 4] > vis).sum()) > 0                                 # the synthetic detector finds candidates
    for al in (with_pose, without):
        out = det.run_batch(frames, return_device=True, face=al)
        assert isinstance(out, tuple) and len(out) == 2 and torch.equal(out[0], plain)
        assert (out[1].pose is not None) == al.has_pose_tables
        assert int(out[1].counts.sum()) > 0
        assert _same_result(out[1], al.align(frames, rows=plain, vis_thresh=vis, pose=al.has_pose_tables))
    # the host-list form, and with draw=True the crops are taken before anything is painted
    want = with_pose.align(frames, rows=plain, vis_thresh=vis, pose=True)
    res, faces = det.run_batch(frames, face=with_pose)
    assert res == listed and _same_result(faces, want)
    painted = [f.clone() for f in frames]
    rows, faces = det.run_batch(painted, return_device=True, face=with_pose, draw=True)
    assert torch.equal(rows, plain) and _same_result(faces, want)
    assert any(not torch.equal(p, f) for p, f in zip(painted, frames))
    drawn = [f.clone() for f in frames]
    det.run_batch(drawn, draw=True)
    assert all(torch.equal(p, d) for p, d in zip(painted, drawn))                # ... and the painting is what it is without face=
    with pytest.raises(ValueError, match="capacity 4"):
        det.run_batch([frames[0]] * 5, face=with_pose)
    with pytest.raises(ValueError, match="frames on the device"):
        det.run_batch(pics, face=with_pose)


def test_run_batch_with_face_and_embed():
    from centerpose_amd import config, detector, reid, synth
    det = detector.MultiPoseDetector(config.get_cfg("dla_34", TEST__FIX_RES=False))
    al = _aligners()[0]
    ex = reid.ReidExtractor(synth.make_state_dict("reid", seed=5), capacity=8)
    frames = [torch.from_numpy(np.ascontiguousarray((face_ref.make_input(31 + n, 96, 128)[::-1].transpose(1, 2, 0) * 255).round().astype(np.uint8))).cuda()
              for n in range(2)]
    rows, res = det.run_batch(frames, return_device=True, embed=ex)
    feats = res.features.clone()
    want = al.align(frames, rows=rows, vis_thresh=float(det.cfg.TEST.VIS_THRESH), pose=True)
    out = det.run_batch(frames, return_device=True, embed=ex, face=al, dets_only=False)
    assert len(out) == 3 and torch.equal(out[0], rows) and torch.equal(out[1].features, feats) and _same_result(out[2], want)


def _frames():
    return [torch.from_numpy(np.ascontiguousarray((face_ref.make_input(31 + n, 96, 128)[::-1].transpose(1, 2, 0) * 255).round().astype(np.uint8))).cuda()
            for n in range(2)]


def test_run_batch_with_face_embed_and_track_keeps_the_tuple_order():
    """(rows, ReidResult, tracks, FaceResult): the FaceResult is the last element; rows, features and tracks are what they are without
    face=, in the device form, the host-list form and with draw="tracks"."""
    from centerpose_amd import config, detector, face, reid, synth, track
    det = detector.MultiPoseDetector(config.get_cfg("dla_34", TEST__FIX_RES=False))
    al = _aligners()[0]
    ex = reid.ReidExtractor(synth.make_state_dict("reid", seed=5), capacity=8)
    frames = _frames()
    trk, twin = track.DeepSortTracker(8, streams=2), track.DeepSortTracker(8, streams=2)
    for call in range(2):
        want_rows, want_res, want_tracks = det.run_batch(frames, return_device=True, embed=ex, track=twin)
        feats = want_res.features.clone()
        out = det.run_batch(frames, return_device=True, embed=ex, track=trk, face=al)
        assert isinstance(out, tuple) and len(out) == 4 and isinstance(out[1], reid.ReidResult) and isinstance(out[3], face.FaceResult)
        assert torch.equal(out[0], want_rows) and torch.equal(out[1].features, feats)
        assert len(out[2]) == 2 and all(np.array_equal(a, b) for a, b in zip(out[2], want_tracks))
        assert _same_result(out[3], al.align(frames, rows=want_rows, vis_thresh=float(det.cfg.TEST.VIS_THRESH), pose=True))
    want = al.align(frames, rows=want_rows, vis_thresh=float(det.cfg.TEST.VIS_THRESH), pose=True)
    painted, drawn = [f.clone() for f in frames], [f.clone() for f in frames]
    listed = det.run_batch(painted, embed=ex, track=trk, face=al, draw="tracks")
    plain = det.run_batch(drawn, embed=ex, track=twin, draw="tracks")
    assert len(listed) == 4 and len(plain) == 3 and listed[0] == plain[0] and _same_result(listed[3], want)   # crops from clean frames
    assert all(np.array_equal(a, b) for a, b in zip(listed[2], plain[2])) and all(torch.equal(p, d) for p, d in zip(painted, drawn))


def test_run_batch_with_face_and_dets_only():
    from centerpose_amd import config, detector
    det = detector.MultiPoseDetector(config.get_cfg("dla_34", TEST__FIX_RES=False))
    al = _aligners()[0]
    frames = _frames()
    plain = det.run_batch(frames, dets_only=True, return_device=True)
    rows, faces = det.run_batch(frames, dets_only=True, return_device=True, face=al)
    assert torch.equal(rows, plain) and int(faces.counts.sum()) > 0
    assert _same_result(faces, al.align(frames, rows=plain, vis_thresh=float(det.cfg.TEST.VIS_THRESH), pose=True))
