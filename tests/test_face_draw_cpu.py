"""CPU: the face overlays without a device -- the host painters (cp_face_draw_frames_host / cp_face_draw_yuv_frames_host,
csrc/face_draw_host.h) against the independent NumPy painter of tests/face_draw_ref.py, byte for byte over whole guarded buffers:
37 x 53 and 64 x 96 frames in every BGR / RGB and 4:2:0 YUV form of tests/draw_ref.py (packed, pitched, 4-channel, chw, NV12 / NV21 /
I420 with odd sizes), a face partly outside the frame, two overlapping faces, an unused slot, NaN / infinite landmarks, an invalid
pose, every layer alone and together, radii 0 and 3, vertex_step 1 and 7; and the refusals of the style and of the call."""
import numpy as np
import pytest

import draw_ref
import draw_util
import face_draw_ref as fdr
import face_draw_util as fdu
import face_pose_util as fpu


@pytest.fixture(scope="module")
def L():
    return draw_util.lib_built()


@pytest.mark.parametrize("style", list(fdr.STYLES))
@pytest.mark.parametrize("H,W", [(37, 53), (64, 96)])
def test_host_painters_equal_the_numpy_painter(L, H, W, style):
    st = fdr.style_of(style)
    faces = fdr.make_faces(H + len(style), H, W, 4, fpu.golden()["face_ind"])
    painted = 0
    for forms in fdu.forms_of(H, W):
        for form in forms:
            rc, bufs = fdu.host_paint(L, [form], faces, st)
            assert rc == 0, L.cp_last_error()
            want = fdr.reference(form, 4, faces, st)
            assert np.array_equal(bufs[0], want), form["name"]
            assert not np.array_equal(want, form["buf"])                      # something was painted
            painted += 1
    assert painted == (10 if H % 2 else 12)


def test_two_frames_share_the_slots(L):
    """N = 2, capacity 4: frame n owns slots 2 n and 2 n + 1."""
    st = fdr.style_of("all layers, radii 3, step 7")
    faces = fdr.make_faces(5, 37, 53, 4, fpu.golden()["face_ind"])
    for forms in ([draw_ref.bgr_forms(70, 37, 53)[2], draw_ref.bgr_forms(80, 37, 53)[0]], [draw_ref.yuv_forms(90, 37, 53)[1], draw_ref.yuv_forms(95, 37, 53)[2]]):
        rc, bufs = fdu.host_paint(L, forms, faces, st)
        assert rc == 0, L.cp_last_error()
        for n in range(2):
            assert np.array_equal(bufs[n], fdr.reference(forms[n], 2, fdr.frame_faces(faces, n, 2), st)), n


def test_default_style_and_struct_size(L):
    from centerpose_amd import draw
    assert L.cp_sizeof_face_style() == draw.FACE_STYLE.itemsize == 48
    s = draw.FaceStyle()
    want = fdr.DEFAULT
    assert (s.landmarks, s.vertices, s.pose_box) == (True, False, False) and s.vertex_step == want["vertex_step"] == 2
    assert s.colors == [want["landmark_color"], want["line_color"], want["vertex_color"], want["box_color"]]
    assert s.radii == [want["landmark_radius"], want["line_radius"], want["box_radius"], want["vertex_radius"]] == [2, 1, 1, 1]
    assert s.struct().tobytes()[:32] == fdu.style_struct(want, False).tobytes()[:32]
    for bad in (dict(landmark_radius=4), dict(line_radius=-1), dict(box_radius=4), dict(vertex_radius=5), dict(vertex_step=0),
                dict(box_color=(0, 256, 0)), dict(line_color=(1, 2))):
        with pytest.raises(ValueError):
            draw.FaceStyle(**bad)
    assert L.cp_face_draw_scratch_bytes(4) == 4 * (48 + 144 * 16) and L.cp_face_draw_scratch_bytes(0) == L.cp_face_draw_scratch_bytes(257) == 0


def test_the_painters_refuse_bad_calls(L):
    form = draw_ref.bgr_forms(3, 37, 53)[0]
    faces = fdr.make_faces(1, 37, 53, 4, fpu.golden()["face_ind"])
    ok = fdr.style_of("all layers, radii 3, step 7")
    for change, kw, msg in ((dict(landmark_radius=4), {}, b"radius"), (dict(vertex_step=0), {}, b"vertex_step"), ({}, dict(with_pose=False), b"pose_box"),
                            ({}, dict(with_pos=False), b"vertices")):
        rc, bufs = fdu.host_paint(L, [form], faces, dict(ok, **change), **kw)
        assert rc == 1 and msg in L.cp_last_error() and np.array_equal(bufs[0], form["buf"]), change
    rc, bufs = fdu.host_paint(L, [form] * 5, faces, ok)
    assert rc == 1 and b"capacity" in L.cp_last_error()
    # without the layers that need them, a call without a pose and without maps paints
    rc, bufs = fdu.host_paint(L, [form], faces, fdr.style_of("default"), with_pose=False, with_pos=False)
    assert rc == 0 and np.array_equal(bufs[0], fdr.reference(form, 4, faces, fdr.style_of("default")))
