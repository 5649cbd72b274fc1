"""The host side of drawing detections onto device frames: the style record, the palette (and its YUV form) and the launch of the
painters of csrc/draw_results.hip over an identity descriptor table; and of drawing tracks: the track style, the identity palette, the
item table of boxes and labels and the launch of csrc/draw_tracks.hip; and of blending heat maps over frames: the heat-map style, the
frame -> map matrices and the launch of csrc/draw_heat.hip.  `BaseDetector.draw_results` / `draw_tracks` / `draw_heatmaps` are the entry
points."""
import ctypes

import numpy as np
import torch

from . import _lib
from .frames import YUV_COLORS, identity_table

# cp_draw_style (include/centerpose_hip.h)
DRAW_STYLE = np.dtype([("box_thickness", "<i4"), ("limb_radius", "<i4"), ("joint_radius", "<i4"), ("palette", "u1", (36, 4))])
# cp_draw_overlay: what a DrawStyle holds beyond cp_draw_style -- the opacities of box, limbs and joints and the score label
DRAW_OVERLAY = np.dtype([("opacity", "<i4", (3,)), ("label_scale", "<i4"), ("nprefix", "<i4"), ("prefix", "u1", (12,)), ("text_color", "u1", (4,))])
MAX_LABEL_PREFIX = 9

# the limbs of a pose in paint order, as joint pairs (COCO keypoint order: 0 nose, odd = left, even = right)
DRAW_LIMBS = ((0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (4, 6), (5, 6), (5, 7), (7, 9), (6, 8), (8, 10), (5, 11), (6, 12), (11, 12), (11, 13),
              (13, 15), (12, 14), (14, 16))
# this project's palette, (B, G, R): one colour for left-side parts, one for right-side parts, one for mid-line parts and the box
DRAW_LEFT, DRAW_RIGHT, DRAW_MID = (0, 140, 255), (255, 160, 0), (60, 220, 60)


def _side_color(joints):
    sides = {j % 2 for j in joints if j > 0}                   # the nose is on the mid-line
    return DRAW_MID if len(sides) != 1 else (DRAW_LEFT if sides == {1} else DRAW_RIGHT)


class DrawStyle:
    """How draw_results paints: box_thickness 0..64 (0: no box), limb_radius -1 (no limbs) or 1..64, joint_radius -1 (no joints) or
    0..64, and the colours as (B, G, R): one for the box, one per limb (DRAW_LIMBS order), one per joint.  Defaults: thickness 2, limb
    radius 1, joint radius 2; a limb or joint on the left side DRAW_LEFT, on the right side DRAW_RIGHT, the box, the nose and the limbs
    that join the two sides DRAW_MID.
    labels=True writes label_prefix + '%.1f' % score on a filled bar on top of every box, in the box's colour, as the reference's
    add_coco_bbox does: label_scale 1..8 pixels per cell of the 5 x 7 font, at most 9 prefix characters of CHARSET (lower case is
    folded), the text in label_text_color.  box_opacity / limb_opacity / joint_opacity, 1..256: how much of its colour a primitive of
    that class puts on a pixel, p' = (p (256 - a) + c a + 128) >> 8 per covering primitive; 256 stores the colour as before, 51 and
    128 are the 0.2 and 0.5 of the reference's add_coco_hp.  A style that leaves these defaults paints through the plain entry points."""

    def __init__(self, box_thickness=2, limb_radius=1, joint_radius=2, box_color=None, limb_colors=None, joint_colors=None, labels=False,
                 label_prefix="person", label_scale=1, label_text_color=(0, 0, 0), box_opacity=256, limb_opacity=256, joint_opacity=256):
        self.box_thickness, self.limb_radius, self.joint_radius = int(box_thickness), int(limb_radius), int(joint_radius)
        self.box_color = tuple(box_color) if box_color is not None else DRAW_MID
        self.limb_colors = [tuple(c) for c in limb_colors] if limb_colors is not None else [_side_color(ab) for ab in DRAW_LIMBS]
        self.joint_colors = [tuple(c) for c in joint_colors] if joint_colors is not None else [_side_color((j,)) for j in range(17)]
        if not (0 <= self.box_thickness <= 64):
            raise _lib.CenterposeHipError("box_thickness %d outside 0..64" % self.box_thickness)
        if not (self.limb_radius == -1 or 1 <= self.limb_radius <= 64):
            raise _lib.CenterposeHipError("limb_radius %d is neither -1 nor in 1..64 (radius 0 would dot the lines)" % self.limb_radius)
        if not (-1 <= self.joint_radius <= 64):
            raise _lib.CenterposeHipError("joint_radius %d outside -1..64" % self.joint_radius)
        if len(self.limb_colors) != 18 or len(self.joint_colors) != 17:
            raise _lib.CenterposeHipError("a style has 18 limb colours and 17 joint colours")
        self.labels, self.label_prefix, self.label_scale = bool(labels), str(label_prefix), int(label_scale)
        self.label_text_color = tuple(int(v) for v in label_text_color)
        self.box_opacity, self.limb_opacity, self.joint_opacity = int(box_opacity), int(limb_opacity), int(joint_opacity)
        for c in self.palette() + [self.label_text_color]:
            if len(c) != 3 or any(not (0 <= int(v) <= 255) for v in c):
                raise _lib.CenterposeHipError("a colour is three values in 0..255, got %r" % (c,))
        if not 1 <= self.label_scale <= 8:
            raise _lib.CenterposeHipError("label_scale %d outside 1..8 (labels=False draws none)" % self.label_scale)
        for name in ("box_opacity", "limb_opacity", "joint_opacity"):
            if not 1 <= getattr(self, name) <= 256:
                raise _lib.CenterposeHipError("%s %d outside 1..256 (256: opaque)" % (name, getattr(self, name)))
        if len(self.label_prefix) > MAX_LABEL_PREFIX:
            raise _lib.CenterposeHipError("the label prefix %r has %d characters, at most %d are drawn"
                                          % (self.label_prefix, len(self.label_prefix), MAX_LABEL_PREFIX))
        try:
            self.prefix_glyphs = label_glyphs(self.label_prefix)       # a prefix the font cannot write raises here, not at the first frame
        except ValueError as e:
            raise _lib.CenterposeHipError(str(e))

    def needs_overlay(self):
        """Whether the style leaves the defaults of cp_draw_style alone: labels, or a primitive class that is not opaque."""
        return self.labels or (self.box_opacity, self.limb_opacity, self.joint_opacity) != (256, 256, 256)

    def overlay_struct(self, matrix=None):
        """One DRAW_OVERLAY record; `matrix`: the text colour as (Y, U, V) for YUV frames."""
        rec = np.zeros(1, DRAW_OVERLAY)
        rec["opacity"][0] = (self.box_opacity, self.limb_opacity, self.joint_opacity)
        rec["label_scale"] = self.label_scale if self.labels else 0
        rec["nprefix"] = len(self.prefix_glyphs)
        rec["prefix"][0, :len(self.prefix_glyphs)] = self.prefix_glyphs
        rec["text_color"][0, :3] = self.label_text_color if matrix is None else palette_to_yuv([self.label_text_color], matrix)[0]
        return rec

    def palette(self):
        """The 36 (B, G, R) colours in paint order: the box, the limbs, the joints."""
        return [self.box_color] + list(self.limb_colors) + list(self.joint_colors)

    def struct(self, matrix=None):
        """One DRAW_STYLE record; `matrix` ("bt601" / "bt709"): the palette as (Y, U, V) for YUV frames."""
        rec = np.zeros(1, DRAW_STYLE)
        rec["box_thickness"], rec["limb_radius"], rec["joint_radius"] = self.box_thickness, self.limb_radius, self.joint_radius
        pal = self.palette() if matrix is None else palette_to_yuv(self.palette(), matrix)
        rec["palette"][0, :, :3] = np.asarray(pal, np.uint8)
        return rec


# limited-range BGR -> (Y, U, V) rows of (R, G, B) weights, 8 fractional bits
YUV_FORWARD = {"bt601": ((66, 129, 25), (-38, -74, 112), (112, -94, -18)),
               "bt709": ((47, 157, 16), (-26, -87, 112), (112, -102, -10))}


def palette_to_yuv(colors, matrix="bt601"):
    """(B, G, R) colours -> (Y, U, V) by the usual limited-range 8-bit forms, e.g. bt601 Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16,
    U = ((-38 R - 74 G + 112 B + 128) >> 8) + 128, V = ((112 R - 94 G - 18 B + 128) >> 8) + 128 (arithmetic shifts).  This is NOT
    the inverse of csrc/yuv_arith.h's YUV -> BGR: a painted colour read back through the pre-process differs by a few levels."""
    if matrix not in YUV_FORWARD:
        raise _lib.CenterposeHipError("unknown matrix %r: one of %s" % (matrix, ", ".join(sorted(YUV_FORWARD))))
    ky, ku, kv = YUV_FORWARD[matrix]
    out = []
    for b, g, r in colors:
        b, g, r = int(b), int(g), int(r)
        out.append((((ky[0] * r + ky[1] * g + ky[2] * b + 128) >> 8) + 16, ((ku[0] * r + ku[1] * g + ku[2] * b + 128) >> 8) + 128,
                    ((kv[0] * r + kv[1] * g + kv[2] * b + 128) >> 8) + 128))
    return out


def _id_palette_struct(colors, matrix):
    """One DRAW_ID_PALETTE record of 1..64 (B, G, R) colours; `matrix`: as (Y, U, V) for YUV frames."""
    colors = [tuple(int(v) for v in c) for c in colors]
    if not 1 <= len(colors) <= 64:
        raise _lib.CenterposeHipError("an identity palette has 1..64 colours (got %d)" % len(colors))
    for c in colors:
        if len(c) != 3 or any(not (0 <= v <= 255) for v in c):
            raise _lib.CenterposeHipError("a colour is three values in 0..255, got %r" % (c,))
    rec = np.zeros(1, DRAW_ID_PALETTE)
    rec["count"] = len(colors)
    rec["colors"][0, :len(colors), :3] = np.asarray(colors if matrix is None else palette_to_yuv(colors, matrix), np.uint8)
    return rec


def draw_rows(io, frames, rows, color, matrix, vis_thresh, style, row_ids=None, id_palette=None):
    """cp_draw_rows_frames_u8 / cp_draw_rows_yuv_frames_u8 for checked frames (`io.frame` / `io.yuv_frame` per image) and device rows
    [N,M,56]: one table upload through `io` (a FrameIO), two launches in the current stream.  row_ids (CUDA int32 [N,M]): the
    cp_draw_rows_ids_* forms -- a row whose id is >= 0 is painted in id_palette[id % P] (default: TRACK_PALETTE).  A style with
    labels or an opacity below 256 (DrawStyle.needs_overlay) goes through cp_draw_overlay_frames_u8 / cp_draw_overlay_yuv_frames_u8."""
    yuv = color in YUV_COLORS
    style = DrawStyle() if style is None else style
    if not isinstance(style, DrawStyle):
        raise _lib.CenterposeHipError("style is a DrawStyle (got %s)" % type(style).__name__)
    N, M = len(frames), int(rows.shape[1])
    if row_ids is None and id_palette is not None:
        raise _lib.CenterposeHipError("id_palette= colours the rows named by row_ids=, which is missing")
    if row_ids is not None:
        if not isinstance(row_ids, torch.Tensor) or not row_ids.is_cuda or row_ids.device != rows.device:
            raise _lib.CenterposeHipError("row_ids must be a CUDA int32 tensor [N, M] on the rows' device: there is no CPU fallback")
        if row_ids.dtype != torch.int32 or tuple(row_ids.shape) != (N, M):
            raise _lib.CenterposeHipError("row_ids must be int32 [%d, %d] (got %s %s)" % (N, M, row_ids.dtype, tuple(row_ids.shape)))
        row_ids = row_ids.detach().contiguous()
        idp = _id_palette_struct(TRACK_PALETTE if id_palette is None else id_palette, matrix if yuv else None)
    if N == 0 or M == 0:
        return
    table = identity_table(frames, yuv)
    rec = style.struct(matrix if yuv else None)
    L = _lib.lib()
    overlay = style.overlay_struct(matrix if yuv else None) if style.needs_overlay() else None
    sizer = L.cp_draw_scratch_bytes if overlay is None else L.cp_draw_overlay_scratch_bytes
    sizer.restype = ctypes.c_size_t
    nbytes = int(sizer(N, M))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=rows.device)
    table_dev, = io.upload_table([table])
    vp = ctypes.c_void_p
    head = (vp(table_dev.data_ptr()), table.ctypes.data_as(vp), N, vp(rows.data_ptr()), M, ctypes.c_float(float(vis_thresh)),
            rec.ctypes.data_as(vp), vp(scratch.data_ptr()), ctypes.c_size_t(nbytes))
    if overlay is not None:
        name = "cp_draw_overlay_yuv_frames_u8" if yuv else "cp_draw_overlay_frames_u8"
        ids = (vp(row_ids.data_ptr()), idp.ctypes.data_as(vp)) if row_ids is not None else (None, None)
        rc = getattr(L, name)(*head, *ids, overlay.ctypes.data_as(vp), _lib.stream())
    elif row_ids is None:
        name = "cp_draw_rows_yuv_frames_u8" if yuv else "cp_draw_rows_frames_u8"
        rc = getattr(L, name)(*head, _lib.stream())
    else:
        name = "cp_draw_rows_ids_yuv_frames_u8" if yuv else "cp_draw_rows_ids_frames_u8"
        rc = getattr(L, name)(*head, vp(row_ids.data_ptr()), idp.ctypes.data_as(vp), _lib.stream())
    _lib.check(rc, name)


# ---------------------------------------------------------------------------------------------------------------- the face overlays
# cp_face_style (include/centerpose_hip.h); colours: landmark, line, vertex, box
FACE_STYLE = np.dtype([("landmarks", "<i4"), ("vertices", "<i4"), ("pose_box", "<i4"), ("landmark_radius", "<i4"), ("line_radius", "<i4"),
                       ("box_radius", "<i4"), ("vertex_radius", "<i4"), ("vertex_step", "<i4"), ("colors", "u1", (4, 4))])


class FaceStyle:
    """How FaceAligner.draw paints: the layers `landmarks` (the 68 points and the lines between them: plot_kpt, what the reference's
    live loop pastes back), `vertices` (every vertex_step-th vertex of face_ind: plot_vertices) and `pose_box` (plot_pose_box), their
    colours as (B, G, R) as in demo/face/utils/cv_plot.py, radii in 0..3 and vertex_step >= 1."""

    def __init__(self, landmarks=True, vertices=False, pose_box=False, landmark_color=(0, 0, 255), line_color=(255, 255, 255),
                 vertex_color=(255, 0, 0), box_color=(0, 255, 0), landmark_radius=2, line_radius=1, box_radius=1, vertex_radius=1,
                 vertex_step=2):
        self.landmarks, self.vertices, self.pose_box = bool(landmarks), bool(vertices), bool(pose_box)
        self.colors = [tuple(int(v) for v in c) for c in (landmark_color, line_color, vertex_color, box_color)]
        self.radii = [int(landmark_radius), int(line_radius), int(box_radius), int(vertex_radius)]
        self.vertex_step = int(vertex_step)
        for c in self.colors:
            if len(c) != 3 or any(not (0 <= v <= 255) for v in c):
                raise ValueError("a colour is three values in 0..255, got %r" % (c,))
        for name, r in zip(("landmark_radius", "line_radius", "box_radius", "vertex_radius"), self.radii):
            if not 0 <= r <= 3:
                raise ValueError("%s %d outside 0..3" % (name, r))
        if self.vertex_step < 1:
            raise ValueError("vertex_step %d below 1" % self.vertex_step)

    def struct(self, matrix=None):
        """One FACE_STYLE record; `matrix`: the colours as (Y, U, V) for YUV frames."""
        rec = np.zeros(1, FACE_STYLE)
        rec["landmarks"], rec["vertices"], rec["pose_box"] = int(self.landmarks), int(self.vertices), int(self.pose_box)
        rec["landmark_radius"], rec["line_radius"], rec["box_radius"], rec["vertex_radius"] = self.radii
        rec["vertex_step"] = self.vertex_step
        rec["colors"][0, :, :3] = np.asarray(self.colors if matrix is None else palette_to_yuv(self.colors, matrix), np.uint8)
        return rec


def draw_faces(io, frames, result, face_ind, color, matrix, style):
    """cp_face_draw_frames_u8 / cp_face_draw_yuv_frames_u8 for checked frames and a FaceResult on the device: one table upload through
    `io`, two or three launches in the current stream.  face_ind: the aligner's DEVICE int32 table or None."""
    yuv = color in YUV_COLORS
    style = FaceStyle() if style is None else style
    if not isinstance(style, FaceStyle):
        raise ValueError("style is a FaceStyle (got %s)" % type(style).__name__)
    if style.pose_box and result.pose is None:
        raise ValueError("pose_box=True needs a result with a pose (align(..., pose=True) or estimate_pose)")
    if style.vertices and (result.pos is None or face_ind is None):
        raise ValueError("vertices=True needs the position maps (positions=True) and an aligner built with face_ind=")
    N, cap = len(frames), int(result.slots.shape[0])
    if not 1 <= N <= cap:
        raise ValueError("%d frames for a result of capacity %d" % (N, cap))
    table = identity_table(frames, yuv)
    rec = style.struct(matrix if yuv else None)
    L = _lib.lib()
    nbytes = int(L.cp_face_draw_scratch_bytes(cap))
    dev = result.slots.device
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    table_dev, = io.upload_table([table])
    ptr = lambda t: None if t is None else t.data_ptr()
    pose = result.pose if style.pose_box else None
    name = "cp_face_draw_yuv_frames_u8" if yuv else "cp_face_draw_frames_u8"
    rc = getattr(L, name)(table_dev.data_ptr(), table.ctypes.data, N, result.slots.data_ptr(), cap, result.landmarks.data_ptr(),
                          ptr(pose and pose.box), ptr(pose and pose.valid), ptr(result.pos if style.vertices else None),
                          ptr(face_ind if style.vertices else None), int(face_ind.shape[0]) if style.vertices else 0, rec.ctypes.data,
                          scratch.data_ptr(), nbytes, _lib.stream())
    _lib.check(rc, name)


# ---------------------------------------------------------------------------------------------------------------- tracks: boxes and labels
# cp_draw_track_item / cp_draw_id_palette (include/centerpose_hip.h)
TRACK_ITEM = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("color", "u1", (4,)), ("text_color", "u1", (4,)),
                       ("nchars", "<i4"), ("glyph", "u1", (16,))])
DRAW_ID_PALETTE = np.dtype([("count", "<i4"), ("colors", "u1", (64, 4))])
# the label font's characters in glyph order (csrc/draw_text_arith.h); lower case is folded to upper case
CHARSET = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ #-.:_"
MAX_LABEL = 16


def _wheel():
    """24 (B, G, R) colours: the hue circle in steps of 15 degrees at full saturation, every second hue darker, listed so that
    neighbours in the list lie 105 degrees apart.  Integer arithmetic throughout."""
    out = []
    for i in range(24):
        j = (i * 7) % 24
        h, v = 15 * j, (255, 170)[j % 2]
        up, down = v * (h % 60) // 60, v * (60 - h % 60) // 60
        r, g, b = ((v, up, 0), (down, v, 0), (0, v, up), (0, down, v), (up, 0, v), (v, 0, down))[h // 60]
        out.append((b, g, r))
    return out


# this project's identity colours, (B, G, R): colour of track id i is TRACK_PALETTE[i % 24]
TRACK_PALETTE = _wheel()


def label_glyphs(text):
    """The glyph indices of a label: at most 16 characters of CHARSET, lower case folded.  ValueError otherwise."""
    text = str(text).upper()
    if len(text) > MAX_LABEL:
        raise ValueError("the label %r has %d characters, at most %d are drawn" % (text, len(text), MAX_LABEL))
    for ch in text:
        if ch not in CHARSET:
            raise ValueError("the label %r holds %r, which the font does not have: its characters are %r" % (text, ch, CHARSET))
    return [CHARSET.index(ch) for ch in text]


class TrackStyle:
    """How draw_tracks paints: box_thickness 0..64 (0: no box), font_scale 0..8 (pixels per font cell; 0: no bar and no label), the
    label `prefix` + str(track id), the text colour and the identity palette (1..64 (B, G, R) colours; a track's colour is
    palette[id % len(palette)], default TRACK_PALETTE)."""

    def __init__(self, box_thickness=3, font_scale=2, prefix="ID ", text_color=(255, 255, 255), palette=None):
        self.box_thickness, self.font_scale, self.prefix = int(box_thickness), int(font_scale), str(prefix)
        self.text_color = tuple(int(v) for v in text_color)
        self.palette = [tuple(int(v) for v in c) for c in (TRACK_PALETTE if palette is None else palette)]
        if not 0 <= self.box_thickness <= 64:
            raise _lib.CenterposeHipError("box_thickness %d outside 0..64" % self.box_thickness)
        if not 0 <= self.font_scale <= 8:
            raise _lib.CenterposeHipError("font_scale %d outside 0..8" % self.font_scale)
        if not 1 <= len(self.palette) <= 64:
            raise _lib.CenterposeHipError("an identity palette has 1..64 colours (got %d)" % len(self.palette))
        for c in self.palette + [self.text_color]:
            if len(c) != 3 or any(not (0 <= v <= 255) for v in c):
                raise _lib.CenterposeHipError("a colour is three values in 0..255, got %r" % (c,))
        label_glyphs(self.prefix)                              # a prefix the font cannot write raises here, not at the first frame


def track_items(tracks, style, matrix=None):
    """The item table of one draw_tracks call: tracks (per frame an integer array [k, 5] of (x1, y1, x2, y2, track_id), what
    DeepSortTracker.update returns) -> (TRACK_ITEM [N, Kmax], counts int32 [N]).  Coordinates are clamped to [-16384, 16383] and the
    corners sorted; `matrix`: colours as (Y, U, V)."""
    tracks = [np.asarray(t).reshape(-1, 5) for t in tracks]
    for t in tracks:
        if t.dtype.kind not in "iu":
            raise _lib.CenterposeHipError("tracks are integer arrays [k, 5] of (x1, y1, x2, y2, track_id), got dtype %s" % t.dtype)
    N, Kmax = len(tracks), max([len(t) for t in tracks] + [0])
    items, counts = np.zeros((N, Kmax), TRACK_ITEM), np.array([len(t) for t in tracks], np.int32)
    conv = (lambda c: c) if matrix is None else (lambda c: palette_to_yuv([c], matrix)[0])
    text = conv(style.text_color)
    for n, t in enumerate(tracks):
        for k, (x1, y1, x2, y2, tid) in enumerate(t.tolist()):
            glyphs = label_glyphs(style.prefix + str(tid))
            xa, ya, xb, yb = (min(max(int(v), -16384), 16383) for v in (x1, y1, x2, y2))
            it = items[n, k]
            it["x0"], it["y0"], it["x1"], it["y1"] = min(xa, xb), min(ya, yb), max(xa, xb), max(ya, yb)
            it["color"][:3] = conv(style.palette[tid % len(style.palette)])
            it["text_color"][:3] = text
            it["nchars"] = len(glyphs)
            it["glyph"][:len(glyphs)] = glyphs
    return items, counts


def draw_track_items(io, frames, tracks, color, matrix, style):
    """cp_draw_tracks_frames_u8 / cp_draw_tracks_yuv_frames_u8 for checked frames and the host `tracks` of those frames: the descriptor
    table, the items and their counts go up in ONE upload through `io`, one launch in the current stream."""
    yuv = color in YUV_COLORS
    style = TrackStyle() if style is None else style
    if not isinstance(style, TrackStyle):
        raise _lib.CenterposeHipError("style is a TrackStyle (got %s)" % type(style).__name__)
    if len(tracks) != len(frames):
        raise _lib.CenterposeHipError("tracks hold %d arrays for %d frames" % (len(tracks), len(frames)))
    items, counts = track_items(tracks, style, matrix if yuv else None)
    N, Kmax = items.shape
    if N == 0 or int(counts.sum()) == 0:
        return
    table = identity_table(frames, yuv)
    table_dev, items_dev, counts_dev = io.upload_table([table, items, counts])
    vp = ctypes.c_void_p
    name = "cp_draw_tracks_yuv_frames_u8" if yuv else "cp_draw_tracks_frames_u8"
    rc = getattr(_lib.lib(), name)(vp(table_dev.data_ptr()), table.ctypes.data_as(vp), N, vp(items_dev.data_ptr()), items.ctypes.data_as(vp),
                                   vp(counts_dev.data_ptr()), counts.ctypes.data_as(vp), Kmax, style.box_thickness, style.font_scale,
                                   _lib.stream())
    _lib.check(rc, name)


# ---------------------------------------------------------------------------------------------------------------- heat maps over frames
# cp_draw_heat_style (include/centerpose_hip.h)
DRAW_HEAT_STYLE = np.dtype([("channels", "<i4"), ("opacity", "<i4"), ("invert", "<i4"), ("palette", "u1", (32, 4))])
MAX_HEAT_CHANNELS = 32
HEAT_MATRIX_IDS = {"bt601": 0, "bt709": 1}


class HeatmapStyle:
    """How draw_heatmaps paints: `colors`, at least one (B, G, R) per map channel (default: white for one channel, else the first C
    entries of TRACK_PALETTE, cycling past its length); `opacity` 1..256, how much of the colour map a pixel takes, p' = (p (256 - a) +
    f a + 128) >> 8 (179: the reference's 0.7, 256: the colour map alone); `invert`: the reference's white theme -- colours and colour
    map are both taken from 255, so a silent map blends towards white and a peak towards its channel's colour."""

    def __init__(self, colors=None, opacity=179, invert=False):
        self.colors = None if colors is None else [tuple(int(v) for v in c) for c in colors]
        self.opacity, self.invert = int(opacity), bool(invert)
        if not 1 <= self.opacity <= 256:
            raise _lib.CenterposeHipError("opacity %d outside 1..256 (256: the colour map alone)" % self.opacity)
        if self.colors is not None and len(self.colors) > MAX_HEAT_CHANNELS:
            raise _lib.CenterposeHipError("a heat-map style has at most %d colours (got %d)" % (MAX_HEAT_CHANNELS, len(self.colors)))
        for c in self.colors or []:
            if len(c) != 3 or any(not (0 <= v <= 255) for v in c):
                raise _lib.CenterposeHipError("a colour is three values in 0..255, got %r" % (c,))

    def palette(self, channels):
        """The (B, G, R) colours of `channels` map channels."""
        if not 1 <= channels <= MAX_HEAT_CHANNELS:
            raise _lib.CenterposeHipError("%d map channels outside 1..%d" % (channels, MAX_HEAT_CHANNELS))
        if self.colors is None:
            return [(255, 255, 255)] if channels == 1 else [TRACK_PALETTE[c % len(TRACK_PALETTE)] for c in range(channels)]
        if len(self.colors) < channels:
            raise _lib.CenterposeHipError("the style has %d colours for %d map channels" % (len(self.colors), channels))
        return self.colors[:channels]

    def struct(self, channels):
        """One DRAW_HEAT_STYLE record for maps of `channels` channels; the colours stay (B, G, R) for every kind of frame."""
        rec = np.zeros(1, DRAW_HEAT_STYLE)
        rec["channels"], rec["opacity"], rec["invert"] = channels, self.opacity, int(self.invert)
        rec["palette"][0, :channels, :3] = np.asarray(self.palette(channels), np.uint8)
        return rec


def heat_transform(meta, height, width, new_h, new_w):
    """float64 [6]: the frame -> map matrix of one height x width frame that the pre-process resized to new_h x new_w
    (input_geometry) and whose meta is `meta`: get_affine_transform(c, s, 0, (out_width, out_height)), what maps the resized image onto
    the output map, with its columns scaled by the resize (new_w / width, new_h / height).  Not finite: CenterposeHipError."""
    from .post_process import get_affine_transform
    T = np.array(get_affine_transform(meta["c"], meta["s"], 0, (meta["out_width"], meta["out_height"])), np.float64)
    T[:, 0] *= float(new_w) / float(width)
    T[:, 1] *= float(new_h) / float(height)
    if not np.isfinite(T).all():
        raise _lib.CenterposeHipError("the frame -> map matrix of a %d x %d frame is not finite: %s" % (height, width, T.reshape(-1).tolist()))
    return T.reshape(6)


def check_heat_maps(maps, n_frames, device):
    """The maps of one draw_heatmaps call -> a view [N, C, h, w] of them (never a copy): a CUDA float32 tensor [N, C, h, w] ([C, h, w]:
    one frame) on `device` with 1..32 channels and any non-negative strides."""
    if not isinstance(maps, torch.Tensor):
        raise _lib.CenterposeHipError("maps must be a CUDA float32 tensor [N, C, h, w] (got %s): there is no CPU fallback" % type(maps).__name__)
    maps = maps.unsqueeze(0) if maps.dim() == 3 else maps
    if maps.dim() != 4 or maps.shape[2] < 1 or maps.shape[3] < 1:
        raise _lib.CenterposeHipError("maps must be [N, C, h, w] (or [C, h, w] for one frame) with h, w >= 1, got shape %s" % (tuple(maps.shape),))
    if not maps.is_cuda:
        raise _lib.CenterposeHipError("maps on %s: they must be on the model's GPU; there is no CPU fallback" % maps.device)
    device = device() if callable(device) else device
    if maps.device != device:
        raise _lib.CenterposeHipError("maps on %s, the model is on %s" % (maps.device, device))
    if maps.dtype != torch.float32:
        raise _lib.CenterposeHipError("maps must be float32 (got %s)" % maps.dtype)
    if maps.shape[0] != n_frames:
        raise _lib.CenterposeHipError("maps hold %d images for %d frames" % (maps.shape[0], n_frames))
    if not 1 <= maps.shape[1] <= MAX_HEAT_CHANNELS:
        raise _lib.CenterposeHipError("%d map channels outside 1..%d" % (maps.shape[1], MAX_HEAT_CHANNELS))
    return maps.detach()


def heat_table(frames, yuv, metas, geometry, h, w):
    """The identity table of `frames` with the frame -> map matrix of each in its `mi` field (free in an identity table).  metas: one per
    frame, each with c, s, out_height, out_width equal to the maps' (h, w); geometry: (height, width) -> (new_h, new_w)."""
    metas = list(metas)
    if len(metas) != len(frames):
        raise _lib.CenterposeHipError("metas hold %d entries for %d frames" % (len(metas), len(frames)))
    table = identity_table(frames, yuv)
    for d, meta in zip(table, metas):
        if (int(meta["out_height"]), int(meta["out_width"])) != (h, w):
            raise _lib.CenterposeHipError("a meta of a %d x %d map with maps of %d x %d: metas and maps come from one pre_process_batch call"
                                          % (meta["out_height"], meta["out_width"], h, w))
        new_h, new_w = geometry(int(d["H"]), int(d["W"]))
        d["mi"] = heat_transform(meta, int(d["H"]), int(d["W"]), new_h, new_w)
    return table


def draw_heat(io, frames, maps, metas, geometry, color, matrix, style):
    """cp_draw_heat_frames_u8 / cp_draw_heat_yuv_frames_u8 for checked frames and checked maps [N, C, h, w]: one table upload through `io`,
    two launches in the current stream.  The maps go in by pointer and their four element strides."""
    yuv = color in YUV_COLORS
    style = HeatmapStyle() if style is None else style
    if not isinstance(style, HeatmapStyle):
        raise _lib.CenterposeHipError("style is a HeatmapStyle (got %s)" % type(style).__name__)
    N, C, h, w = (int(v) for v in maps.shape)
    rec = style.struct(C)
    table = heat_table(frames, yuv, metas, geometry, h, w)
    if N == 0:
        return
    L = _lib.lib()
    L.cp_draw_heat_scratch_bytes.restype = ctypes.c_size_t
    nbytes = int(L.cp_draw_heat_scratch_bytes(N, h, w))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=maps.device)
    table_dev, = io.upload_table([table])
    vp, ll = ctypes.c_void_p, ctypes.c_longlong
    name = "cp_draw_heat_yuv_frames_u8" if yuv else "cp_draw_heat_frames_u8"
    rc = getattr(L, name)(vp(table_dev.data_ptr()), table.ctypes.data_as(vp), N, vp(maps.data_ptr()), *(ll(int(s)) for s in maps.stride()), C, h, w,
                          rec.ctypes.data_as(vp), *((HEAT_MATRIX_IDS[matrix],) if yuv else ()), vp(scratch.data_ptr()), ctypes.c_size_t(nbytes),
                          _lib.stream())
    _lib.check(rc, name)
