"""The host side of drawing detections onto device frames: the style record, the palette (and its YUV form) and the launch of the
painters of csrc/draw_results.hip over an identity descriptor table.  `BaseDetector.draw_results` is the entry point."""
import ctypes

import numpy as np
import torch

from . import _lib
from .frames import YUV_COLORS, identity_table

# cp_draw_style (include/centerpose_hip.h)
DRAW_STYLE = np.dtype([("box_thickness", "<i4"), ("limb_radius", "<i4"), ("joint_radius", "<i4"), ("palette", "u1", (36, 4))])

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
    that join the two sides DRAW_MID."""

    def __init__(self, box_thickness=2, limb_radius=1, joint_radius=2, box_color=None, limb_colors=None, joint_colors=None):
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
        for c in self.palette():
            if len(c) != 3 or any(not (0 <= int(v) <= 255) for v in c):
                raise _lib.CenterposeHipError("a colour is three values in 0..255, got %r" % (c,))

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


def draw_rows(io, frames, rows, color, matrix, vis_thresh, style):
    """cp_draw_rows_frames_u8 / cp_draw_rows_yuv_frames_u8 for checked frames (`io.frame` / `io.yuv_frame` per image) and device rows
    [N,M,56]: one table upload through `io` (a FrameIO), two launches in the current stream."""
    yuv = color in YUV_COLORS
    style = DrawStyle() if style is None else style
    if not isinstance(style, DrawStyle):
        raise _lib.CenterposeHipError("style is a DrawStyle (got %s)" % type(style).__name__)
    N, M = len(frames), int(rows.shape[1])
    if N == 0 or M == 0:
        return
    table = identity_table(frames, yuv)
    rec = style.struct(matrix if yuv else None)
    L = _lib.lib()
    L.cp_draw_scratch_bytes.restype = ctypes.c_size_t
    nbytes = int(L.cp_draw_scratch_bytes(N, M))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=rows.device)
    table_dev, = io.upload_table([table])
    fn = L.cp_draw_rows_yuv_frames_u8 if yuv else L.cp_draw_rows_frames_u8
    rc = fn(ctypes.c_void_p(table_dev.data_ptr()), table.ctypes.data_as(ctypes.c_void_p), N, ctypes.c_void_p(rows.data_ptr()), M,
            ctypes.c_float(float(vis_thresh)), rec.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(scratch.data_ptr()),
            ctypes.c_size_t(nbytes), _lib.stream())
    _lib.check(rc, "cp_draw_rows_yuv_frames_u8" if yuv else "cp_draw_rows_frames_u8")
