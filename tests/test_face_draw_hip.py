"""GPU: the face overlays on the device -- FaceAligner.draw (face_draw_build_kernel, face_draw_vertices_kernel<bgr|yuv>,
face_draw_kernel<bgr|yuv>) against the host painters, byte for byte over whole guarded buffers (a fourth channel, row padding and the
guard bytes keep their bytes): 37 x 53 and 64 x 96 frames in every BGR / RGB and 4:2:0 YUV form of tests/draw_ref.py, a face partly
outside, two overlapping faces, an unused slot, NaN / infinite landmarks, an invalid pose, the layers alone and together, radii 0 and 3,
vertex_step 1 and 7, two frames sharing the slots; the refusals; and run_batch(face=, face_style=) against run_batch, align and draw."""
import functools
import os

import numpy as np
import pytest
import torch

import draw_ref
import draw_util
import face_draw_ref as fdr
import face_draw_util as fdu
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


def _on_device(form):
    dev = torch.from_numpy(form["buf"].copy()).cuda()
    views = [torch.as_strided(dev, shape, strides, off) for off, shape, strides in form["views"]]
    return dev, (views[0] if len(views) == 1 else tuple(views))


def _result(faces, pose=True, positions=True):
    from centerpose_amd import face
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in faces.items()}
    cap = len(faces["slots"])
    fp = face.FacePose(torch.zeros((cap, 3, 4), dtype=torch.float64, device="cuda"), torch.zeros((cap, 3), dtype=torch.float64, device="cuda"),
                       torch.zeros((cap,), dtype=torch.float64, device="cuda"), t["box"], t["valid"]) if pose else None
    return face.FaceResult(t["pos"] if positions else None, t["landmarks"], t["slots"], torch.zeros((1,), dtype=torch.int32, device="cuda"),
                           torch.zeros((cap, 3), device="cuda"), fp)


def _style(st):
    from centerpose_amd import draw
    return draw.FaceStyle(**st)


@pytest.mark.parametrize("style", list(fdr.STYLES))
@pytest.mark.parametrize("H,W", [(37, 53), (64, 96)])
def test_device_equals_the_host_painters(H, W, style):
    L = draw_util.lib_loaded()
    al = _aligners()[0]
    st = fdr.style_of(style)
    faces = fdr.make_faces(H + len(style), H, W, 4, fpu.golden()["face_ind"])
    res = _result(faces)
    for forms in fdu.forms_of(H, W):
        for form in forms:
            rc, want = fdu.host_paint(L, [form], faces, st)
            assert rc == 0, L.cp_last_error()
            dev, frame = _on_device(form)
            assert al.draw([frame], res, layout=form["layout"], color=form["color"], style=_style(st)) is not None
            torch.cuda.synchronize()
            assert np.array_equal(dev.cpu().numpy(), want[0]), form["name"]
            assert L.cp_last_kernel() == (b"face_draw_kernel<bgr>" if form["color"] in ("bgr", "rgb") else b"face_draw_kernel<yuv>")


def test_two_frames_share_the_slots_and_bt709():
    L = draw_util.lib_loaded()
    al = _aligners()[0]
    st = fdr.style_of("all layers, radii 3, step 7")
    faces = fdr.make_faces(5, 37, 53, 4, fpu.golden()["face_ind"])
    res = _result(faces)
    for forms, matrix in (([draw_ref.bgr_forms(70, 37, 53)[0], draw_ref.bgr_forms(80, 64, 96)[0]], "bt601"),
                          ([draw_ref.yuv_forms(90, 37, 53)[2], draw_ref.yuv_forms(95, 64, 96)[2]], "bt709")):
        rc, want = fdu.host_paint(L, forms, faces, st, matrix)
        assert rc == 0, L.cp_last_error()
        devs, frames = zip(*[_on_device(f) for f in forms])
        al.draw(list(frames), res, layout=forms[0]["layout"], color=forms[0]["color"], matrix=matrix, style=_style(st))
        torch.cuda.synchronize()
        for n in range(2):
            assert np.array_equal(devs[n].cpu().numpy(), want[n]), n
            assert np.array_equal(want[n], fdr.reference(forms[n], 2, fdr.frame_faces(faces, n, 2), st, matrix))


def test_draw_refuses_before_any_launch():
    from centerpose_amd import _lib
    al, plain = _aligners()
    faces = fdr.make_faces(1, 37, 53, 4, fpu.golden()["face_ind"])
    res = _result(faces)
    form = draw_ref.bgr_forms(3, 37, 53)[0]
    dev, frame = _on_device(form)
    from centerpose_amd import draw
    with pytest.raises(ValueError, match="pose_box=True needs"):
        al.draw([frame], _result(faces, pose=False), style=draw.FaceStyle(pose_box=True))
    with pytest.raises(ValueError, match="vertices=True needs"):
        al.draw([frame], _result(faces, positions=False), style=draw.FaceStyle(vertices=True))
    with pytest.raises(ValueError, match="vertices=True needs"):
        plain.draw([frame], res, style=draw.FaceStyle(vertices=True))
    with pytest.raises(ValueError, match="host arrays"):
        al.draw([form["buf"][64:64 + 37 * 53 * 3].reshape(37, 53, 3)], res)
    with pytest.raises(_lib.CenterposeHipError, match="cannot be drawn on"):
        al.draw([frame], res, color="p010")
    with pytest.raises(_lib.CenterposeHipError):
        al.draw([frame.expand(37, 53, 3)[:, :, :1].expand(37, 53, 3)], res)                     # an expanded view
    with pytest.raises(_lib.CenterposeHipError):
        al.draw([torch.as_strided(dev, (37, 53, 3), (53 * 2, 3, 1), 64)], res)                # rows that overlap
    with pytest.raises(_lib.CenterposeHipError):
        al.draw([frame, frame], res)                                                          # one tensor twice
    with pytest.raises(ValueError, match="FaceStyle"):
        al.draw([frame], res, style=object())
    bad = _result(faces)
    bad.landmarks = bad.landmarks[:, :27]
    with pytest.raises(ValueError, match="not one of this aligner's: landmarks"):
        al.draw([frame], bad)
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), form["buf"])
    # the default style needs neither a pose nor the maps
    plain.draw([frame], _result(faces, pose=False, positions=False))
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), fdr.reference(form, 4, faces, fdr.style_of("default")))


def test_run_batch_with_face_style():
    """run_batch(face=, face_style=) == run_batch, then align, then draw -- bit for bit, also after draw=True's own painting."""
    from centerpose_amd import config, detector, draw
    det = detector.MultiPoseDetector(config.get_cfg("dla_34", TEST__FIX_RES=False))
    al = _aligners()[0]
    vis = float(det.cfg.TEST.VIS_THRESH)
    pics = [np.ascontiguousarray((face_ref.make_input(31 + n, 96, 128)[::-1].transpose(1, 2, 0) * 255).round().astype(np.uint8)) for n in range(2)]
    style = draw.FaceStyle(vertices=True, pose_box=True)
    for kw in ({}, dict(draw=True)):
        a, b = [torch.from_numpy(p).cuda() for p in pics], [torch.from_numpy(p).cuda() for p in pics]
        rows, faces = det.run_batch(a, return_device=True, face=al, face_style=style, **kw)
        want_rows = det.run_batch(b, return_device=True, **kw)
        clean = [torch.from_numpy(p).cuda() for p in pics]
        want = al.align(clean, rows=want_rows, vis_thresh=vis, pose=True)                    # crops from clean frames
        al.draw(b, want, style=style)
        assert torch.equal(rows, want_rows) and torch.equal(faces.landmarks, want.landmarks) and int(faces.counts.sum()) > 0
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and any(not torch.equal(x, c) for x, c in zip(a, clean))
    frames = [torch.from_numpy(p).cuda() for p in pics]
    with pytest.raises(ValueError, match="without `face`"):
        det.run_batch(frames, face_style=style)
    with pytest.raises(ValueError, match="face_ind"):
        det.run_batch(frames, face=_aligners()[1], face_style=style)
    assert all(torch.equal(f, torch.from_numpy(p).cuda()) for f, p in zip(frames, pics))
