"""The NumPy reference of the face overlays: a sequential painter written from the rule, not from csrc/face_draw_arith.h (nothing here
reads that file or the library), over the frame forms and the disc / capsule masks of tests/draw_ref.py, and the cases the CPU and GPU
tests share.

The rule.  A landmark or vertex sits at np.round (half to even) of its float32 x and y clamped to [-16384, 16384]; a coordinate that is
not finite kills the primitives it belongs to.  Beneath everything, for every used face, a disc of vertex_radius at vertex
i * vertex_step of face_ind.  Then per used face in ascending slot order: a capsule k -> k + 1 of line_radius for every landmark k not
in END_LIST, a disc of landmark_radius on every landmark, and where the pose is valid the 13 capsules of the pose box (the closed
polyline over the ten corners, 1 -> 6, 2 -> 7, 3 -> 8) of box_radius.  Later paint wins; everything is clipped."""
import numpy as np

import draw_ref

END_LIST = (16, 21, 26, 30, 35, 41, 47, 67)          # cv_plot.py:9
BOX_LINES = [(j, (j + 1) % 10) for j in range(10)] + [(1, 6), (2, 7), (3, 8)]
PRIMS = 141
LANDMARK, LINE, VERTEX, BOX = 0, 1, 2, 3             # colour classes, the order of a style's colours


def point(xy):
    v = np.asarray(xy, np.float32)[:2]
    if not np.isfinite(v).all():
        return None
    r = np.round(np.clip(v, np.float32(-16384), np.float32(16384)))
    return int(r[0]), int(r[1])


def winners(H, W, q, faces, style):
    """int64 [H, W]: -1 where nothing is painted, 0 for a dense vertex, 1 + face * 141 + primitive for the last covering primitive.
    faces: dict of slots [q], landmarks [q, 68, 3], box [q, 10, 2] / valid [q] (or None), pos [q, 256, 256, 3] / face_ind (or None);
    style: dict with the FaceStyle fields."""
    Y, X = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    win = np.full((H, W), -1, np.int64)
    if style["vertices"]:
        for f in range(q):
            if faces["slots"][f] < 0:
                continue
            cells = np.asarray(faces["face_ind"])[::style["vertex_step"]]
            pts = {point(p) for p in faces["pos"][f].reshape(-1, 3)[cells]}
            for p in pts - {None}:
                if -4 <= p[0] < W + 4 and -4 <= p[1] < H + 4:
                    win[draw_ref.joint_mask(X, Y, p, style["vertex_radius"])] = 0
    for f in range(q):
        if faces["slots"][f] < 0:
            continue
        pts = [point(p) for p in faces["landmarks"][f]]
        base, i = 1 + f * PRIMS, 0
        for k in range(68):
            if k in END_LIST:
                continue
            if style["landmarks"] and pts[k] is not None and pts[k + 1] is not None:
                win[draw_ref.limb_mask(X, Y, pts[k], pts[k + 1], style["line_radius"])] = base + i
            i += 1
        for k in range(68):
            if style["landmarks"] and pts[k] is not None:
                win[draw_ref.joint_mask(X, Y, pts[k], style["landmark_radius"])] = base + 60 + k
        if style["pose_box"] and faces["valid"][f] == 1:
            b = [tuple(int(v) for v in c) for c in faces["box"][f]]
            for j, (a, e) in enumerate(BOX_LINES):
                win[draw_ref.limb_mask(X, Y, b[a], b[e], style["box_radius"])] = base + 128 + j
    return win


def classes(win):
    i = (win - 1) % PRIMS
    return np.where(win == 0, VERTEX, np.where(i < 60, LINE, np.where(i < 128, LANDMARK, BOX)))


def reference(form, q, faces, style, matrix="bt601"):
    """The buffer of `form` after the reference has painted the faces onto it (a copy)."""
    buf = form["buf"].copy()
    views = draw_ref.numpy_views(buf, form)
    H, W = draw_ref.frame_size(form)
    win = winners(H, W, q, faces, style)
    cls = classes(win)
    colors = [style["landmark_color"], style["line_color"], style["vertex_color"], style["box_color"]]
    if form["color"] in ("bgr", "rgb"):
        hwc = views[0] if form["layout"] == "hwc" else views[0].transpose(1, 2, 0)
        pal = np.asarray(colors, np.uint8)
        ys, xs = np.nonzero(win >= 0)
        for k in range(3):
            hwc[ys, xs, k if form["color"] == "bgr" else 2 - k] = pal[cls[ys, xs], k]
    else:
        y, u, v = draw_ref.yuv_planes(views, form["color"])
        pal = np.asarray(draw_ref.bgr_to_yuv(colors, matrix), np.uint8)
        ys, xs = np.nonzero(win >= 0)
        y[ys, xs] = pal[cls[ys, xs], 0]
        padded = np.full((2 * ((H + 1) // 2), 2 * ((W + 1) // 2)), -1, np.int64)
        padded[:H, :W] = win
        top = padded.reshape((H + 1) // 2, 2, (W + 1) // 2, 2).max(axis=(1, 3))
        cy, cx = np.nonzero(top >= 0)
        tc = classes(top)
        u[cy, cx] = pal[tc[cy, cx], 1]
        v[cy, cx] = pal[tc[cy, cx], 2]
    return buf


# ---------------------------------------------------------------------------------------------------------------- shared cases
DEFAULT = dict(landmarks=True, vertices=False, pose_box=False, landmark_color=(0, 0, 255), line_color=(255, 255, 255),
               vertex_color=(255, 0, 0), box_color=(0, 255, 0), landmark_radius=2, line_radius=1, box_radius=1, vertex_radius=1, vertex_step=2)

STYLES = {
    "default": {},
    "vertices alone, step 1": dict(landmarks=False, vertices=True, vertex_step=1),
    "box alone, radius 0": dict(landmarks=False, pose_box=True, box_radius=0),
    "all layers, radii 3, step 7": dict(vertices=True, pose_box=True, landmark_radius=3, line_radius=3, box_radius=3, vertex_radius=3, vertex_step=7,
                                        landmark_color=(10, 200, 30), line_color=(1, 2, 3), vertex_color=(250, 128, 7), box_color=(90, 0, 255)),
    "all layers, radii 0": dict(vertices=True, pose_box=True, landmark_radius=0, line_radius=0, box_radius=0, vertex_radius=0),
}


def style_of(name):
    return dict(DEFAULT, **STYLES[name])


def make_faces(seed, H, W, cap, face_ind):
    """cap = 4 slots of one frame, or 2 + 2 of two: slot 0 a face partly outside the frame, slot 1 one that overlaps it, slot 2 unused,
    slot 3 a face with a NaN and an infinite landmark, a NaN vertex and an invalid pose."""
    r = np.random.RandomState(seed)
    lm = np.zeros((cap, 68, 3), np.float32)
    pos = np.zeros((cap, 256, 256, 3), np.float32)
    box = np.zeros((cap, 10, 2), np.int32)
    centres = [(-0.1 * W, 0.3 * H), (0.25 * W, 0.45 * H), (0.6 * W, 0.6 * H), (0.7 * W, 0.4 * H)]
    for s in range(cap):
        cx, cy = centres[s % 4]
        size = 0.45 * min(H, W)
        lm[s, :, 0] = cx + r.uniform(-size, size, 68)
        lm[s, :, 1] = cy + r.uniform(-size, size, 68)
        lm[s, ::9, :2] = np.round(lm[s, ::9, :2]) + 0.5                 # ties: half to even
        pos[s].reshape(-1, 3)[:, 0] = cx + r.uniform(-size, size, 65536)
        pos[s].reshape(-1, 3)[:, 1] = cy + r.uniform(-size, size, 65536)
        box[s, :, 0] = (cx + r.uniform(-size, size, 10)).astype(np.int32)
        box[s, :, 1] = (cy + r.uniform(-size, size, 10)).astype(np.int32)
        box[s, 4], box[s, 9] = box[s, 0], box[s, 5]
    box[0, 2] = (-16384, 16383)                                          # a corner at the clamp
    lm[cap - 1, 5, 0], lm[cap - 1, 40, 1], lm[0, 67, 0] = np.nan, np.inf, 3e9
    pos[cap - 1].reshape(-1, 3)[face_ind[4], 1] = np.nan
    slots = np.arange(cap, dtype=np.int32) * 7
    slots[2 if cap > 2 else 1] = -1
    valid = np.ones(cap, np.int32)
    valid[cap - 1] = 0
    return dict(slots=slots, landmarks=lm, box=box, valid=valid, pos=pos, face_ind=np.asarray(face_ind, np.int32))


def frame_faces(faces, n, q):
    """The q slots of frame n."""
    sl = slice(n * q, n * q + q)
    return dict(faces, slots=faces["slots"][sl], landmarks=faces["landmarks"][sl], box=faces["box"][sl], valid=faces["valid"][sl],
                pos=faces["pos"][sl])
