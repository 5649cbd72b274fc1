"""Detector entry points with the reference's names, arguments, return values and timing keys:
``BaseDetector`` (lib/detectors/base_detector.py:15-140) and ``MultiPoseDetector``
(lib/detectors/multi_pose.py:24-79), so the class drops in behind tools/demo.py:47-49,77 and
tools/evaluate.py:48-67 (``detector_factory['multi_pose'](cfg).run(path)``).

What is kept is the CONTRACT -- method names and signatures, the meta dict, the seven timing buckets and the result
dict of ``run`` -- not the reference's statement order: the stages are organised around a small stage clock and an input
source object, every pixel / tensor stage runs on the device:

* ``pre_process``: upload of the uint8 image, then cv2.resize / cv2.warpAffine / normalise / HWC->CHW (+ mirrored twin) as
  two HIP kernels that restate OpenCV's 8-bit fixed-point arithmetic (csrc/prepost.hip) -- cv2 is not a dependency;
* ``process``: fused HIP engine (hm / hm_hp leave the head kernel already sigmoided), device flip-test merge (the reference
  bounces through numpy, models/utils.py:30-47), HIP decode; any batch size when FLIP_TEST is off (the reference is batch-1
  by construction, multi_pose.py:63) -- that is the batched throughput path of BASELINE.json;
* ``post_process``: inverse affine of boxes / keypoints as one HIP kernel, one D2H copy;
* ``merge_outputs``: soft-NMS on the host (C++, csrc/host_nms.cpp).

``run_batch`` (not in the reference, which is one image at a time) takes N images through the same stages batched:
``pre_process_batch`` / ``process`` / ``post_process_batch`` / ``merge_outputs_batch`` (csrc/batch_stages.hip), soft-NMS included
on the device, with one upload and one download per call.

Frames that are ALREADY on the device (CUDA uint8 tensors: [H,W,C] or [C,H,W], C = 3 or 4, BGR or RGB, any strides) go through the
same entry points -- ``pre_process``, ``pre_process_batch``, ``run_batch``, ``run`` -- and are read in place by csrc/frame_sources.hip:
no staging copy, no upload, never a ``.contiguous()``; ``run_batch(..., return_device=True)`` hands the rows back without a download.
Frames in 4:2:0 YUV (``color="nv12"`` / ``"nv21"`` / ``"i420"``: a decoder's surface or a tuple of plane tensors, any strides) go the
same way through csrc/yuv_frames.hip, which converts to BGR (``matrix="bt601"`` / ``"bt709"``) where the pixels are loaded.
"""
import ctypes
import time

import numpy as np
import torch

from . import _lib
from .decode import multi_pose_decode
from .model import create_model, load_model
from .post_process import get_affine_transform

FLIP_IDX = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]   # multi_pose.py:27


class StageClock:
    """The seven wall-clock buckets of BaseDetector.run (base_detector.py:80-81,138-140).  `lap(key)` synchronises the
    device and charges the time since the previous mark to `key`; `split(key, at)` charges up to an externally taken
    time stamp (process() reports when the forward finished)."""
    KEYS = ("tot", "load", "pre", "net", "dec", "post", "merge")

    def __init__(self, sync):
        self._sync = sync
        self.t = dict.fromkeys(self.KEYS, 0)
        self._start = self._mark = time.time()

    def lap(self, key, sync=True):
        if sync:
            self._sync()
        now = time.time()
        self.t[key] += now - self._mark
        self._mark = now

    def split(self, key, at):
        self.t[key] += at - self._mark
        self._mark = at

    def report(self, results):
        self.t["tot"] += self._mark - self._start
        out = {"results": {1: results}}
        out.update(self.t)
        return out


class _ArraySource:
    """run() input that still needs pre-processing: an HxWx3 uint8 BGR array (what cv2.imread returns), or one frame on the device
    (a CUDA uint8 tensor in the given layout / colour order)."""

    def __init__(self, image, layout="hwc", color="bgr", matrix="bt601"):
        self.image, self.layout, self.color, self.matrix = image, layout, color, matrix

    def at_scale(self, det, scale, meta):
        return det.pre_process(self.image, scale, meta, self.layout, self.color, self.matrix)


class _PreparedSource:
    """run() input from the evaluation data loader: {'image', 'images': {scale: tensor}, 'meta': {scale: dict of tensors}}
    (base_detector.py:91-93,103-106)."""

    def __init__(self, item):
        self.item = item

    def at_scale(self, det, scale, meta):
        images = self.item["images"][scale][0]
        meta = {k: v.numpy()[0] for k, v in self.item["meta"][scale].items()}
        return images, meta


def _imread(path):
    try:
        import cv2
    except ImportError:
        if path.endswith(".npy"):
            return np.load(path)
        raise RuntimeError("cv2 is not available here: pass an HxWx3 uint8 numpy array (or a .npy path) to run()")
    return cv2.imread(path)


# cp_pre_desc (include/centerpose_hip.h): one source image of a batched pre-process
PRE_DESC = np.dtype([("src_off", "<i8"), ("mid_off", "<i8"), ("H", "<i4"), ("W", "<i4"), ("NH", "<i4"), ("NW", "<i4"),
                     ("mi", "<f8", (6,)), ("slot", "<i4"), ("pad", "<i4")])


# cp_frame_desc (include/centerpose_hip.h): one source frame on the device, addressed by pointer and strides
FRAME_DESC = np.dtype([("base", "<u8"), ("row_stride", "<i8"), ("pix_stride", "<i8"), ("ch_off", "<i8", (3,)), ("mid_off", "<i8"),
                       ("H", "<i4"), ("W", "<i4"), ("NH", "<i4"), ("NW", "<i4"), ("mi", "<f8", (6,)), ("slot", "<i4"), ("pad", "<i4")])

# cp_yuv_frame_desc (include/centerpose_hip.h): one source frame on the device in 4:2:0 YUV planes
YUV_FRAME_DESC = np.dtype([("y_base", "<u8"), ("y_row", "<i8"), ("y_pix", "<i8"), ("u_base", "<u8"), ("v_base", "<u8"), ("c_row", "<i8"),
                           ("c_pix", "<i8"), ("mid_off", "<i8"), ("H", "<i4"), ("W", "<i4"), ("NH", "<i4"), ("NW", "<i4"),
                           ("mi", "<f8", (6,)), ("slot", "<i4"), ("pad", "<i4")])

LAYOUTS, COLORS, YUV_COLORS = ("hwc", "chw"), ("bgr", "rgb"), ("nv12", "nv21", "i420")

# limited-range YUV -> BGR matrices (csrc/yuv_arith.h): (CY, CVR, CVG, CUG, CUB, YOFF), every entry round(k * 2^20)
YUV_MATRICES = {"bt601": (1220542, 1673527, -852492, -409993, 2116026, 16),       # 1.164, 1.596, -0.813, -0.391, 2.018
                "bt709": (1220542, 1880097, -558891, -223347, 2214593, 16)}       # 1.164, 1.793, -0.533, -0.213, 2.112


def _check_layout(layout, color, matrix="bt601"):
    if layout not in LAYOUTS:
        raise _lib.CenterposeHipError("unknown layout %r: one of %s" % (layout, ", ".join(LAYOUTS)))
    if color not in COLORS + YUV_COLORS:
        raise _lib.CenterposeHipError("unknown color %r: one of %s" % (color, ", ".join(COLORS + YUV_COLORS)))
    if matrix not in YUV_MATRICES:
        raise _lib.CenterposeHipError("unknown matrix %r: one of %s" % (matrix, ", ".join(sorted(YUV_MATRICES))))
    if color in YUV_COLORS and layout != "hwc":
        raise _lib.CenterposeHipError("layout=%r does not apply to color=%r: YUV frames are given as planes" % (layout, color))
    if color not in YUV_COLORS and matrix != "bt601":
        raise _lib.CenterposeHipError("matrix=%r applies to YUV frames (color %s) only, not to color=%r" % (matrix, " / ".join(YUV_COLORS), color))


def frame_geometry(shape, strides, layout="hwc", color="bgr"):
    """How a uint8 frame of the given shape and strides (in elements == bytes) is addressed: (H, W, row_stride, pix_stride, ch_off),
    channel k of the network (cv2's B, G, R) of pixel (y, x) at byte y * row_stride + x * pix_stride + ch_off[k] from the frame's first
    element.  layout "hwc": [H,W,C], "chw": [C,H,W]; C = 3 or 4 (a fourth channel is never read); color: the order of the first three
    channels in memory.  A pure function of its arguments: nothing is copied, any strides (crops, padded rows, expanded views) go."""
    _check_layout(layout, color)
    if color in YUV_COLORS:
        raise _lib.CenterposeHipError("color=%r frames are planes: yuv_frame_geometry" % color)
    shape, strides = tuple(int(v) for v in shape), tuple(int(v) for v in strides)
    if len(shape) != 3 or len(strides) != 3:
        raise _lib.CenterposeHipError("a frame is 3-D ([H,W,C] or [C,H,W]), got shape %s" % (shape,))
    (H, W, C), (sh, sw, sc) = (shape, strides) if layout == "hwc" else ((shape[1], shape[2], shape[0]), (strides[1], strides[2], strides[0]))
    if C not in (3, 4):
        raise _lib.CenterposeHipError("a frame has 3 or 4 channels (layout %r of shape %s has %d)" % (layout, shape, C))
    if H <= 0 or W <= 0:
        raise _lib.CenterposeHipError("a frame of shape %s has no pixels" % (shape,))
    if min(sh, sw, sc) < 0:
        raise _lib.CenterposeHipError("negative strides %s are not addressable" % (strides,))
    return H, W, sh, sw, ((0, sc, 2 * sc) if color == "bgr" else (2 * sc, sc, 0))


def yuv_frame_geometry(shapes, strides, color="nv12", dtypes=None):
    """How a 4:2:0 YUV frame given as uint8 planes is addressed.  shapes / strides (in elements == bytes): one entry per tensor of the
    frame -- (y [H,W], uv [ceil(H/2),ceil(W/2),2]) for "nv12" / "nv21", (y, u, v) with u, v [ceil(H/2),ceil(W/2)] of equal strides for
    "i420", or ONE 2-D surface [H*3/2, W] (H, W even, any row stride: the decoder's layout, chroma rows below the luma rows) for
    "nv12" / "nv21"; dtypes: the tensors' dtypes when known (anything but uint8 raises).
    -> (H, W, y_row, y_pix, u_off, v_off, c_row, c_pix): Y(r, c) at byte r * y_row + c * y_pix of the first tensor, U(r, c) at byte
    u_off + (r >> 1) * c_row + (c >> 1) * c_pix of the tensor that holds it, V(r, c) the same from v_off (the surface itself, the uv
    plane, or the u and the v plane, each from its own first element).  A pure function of its arguments: nothing is copied, any
    non-negative strides (pitched rows, crops at even origins, expanded planes) go."""
    _check_layout("hwc", color)
    if color not in YUV_COLORS:
        raise _lib.CenterposeHipError("color=%r frames are not planes: frame_geometry" % color)
    shapes = [tuple(int(v) for v in s) for s in shapes]
    strides = [tuple(int(v) for v in s) for s in strides]
    if len(shapes) != len(strides) or any(len(a) != len(b) for a, b in zip(shapes, strides)):
        raise _lib.CenterposeHipError("one stride per dimension of every plane: shapes %s, strides %s" % (shapes, strides))
    for dt in (dtypes or ()):
        if dt is not torch.uint8 and (isinstance(dt, torch.dtype) or np.dtype(dt) != np.uint8):
            raise _lib.CenterposeHipError("the planes of a YUV frame must be uint8 (got %s)" % (dt,))
    if any(v < 0 for s in strides for v in s):
        raise _lib.CenterposeHipError("negative strides %s are not addressable" % (strides,))
    if len(shapes) == 1:                                       # the decoder's surface: luma rows, then the interleaved chroma rows
        if color == "i420":
            raise _lib.CenterposeHipError("an i420 frame is three planes (y, u, v); one surface tensor is nv12 / nv21")
        if len(shapes[0]) != 2:
            raise _lib.CenterposeHipError("a %s surface is one 2-D tensor [H*3/2, W], got shape %s" % (color, shapes[0]))
        (rows, W), (pitch, pix) = shapes[0], strides[0]
        H = rows * 2 // 3
        if rows <= 0 or W <= 0:
            raise _lib.CenterposeHipError("a frame of shape %s has no pixels" % (shapes[0],))
        if rows % 3 or H % 2 or W % 2:
            raise _lib.CenterposeHipError("a %s surface [H*3/2, W] needs even H and W, got shape %s: pass the planes (y, uv) otherwise"
                                          % (color, shapes[0]))
        first = H * pitch                                      # t[H:].unflatten(1, (W // 2, 2)): strides (pitch, 2 * pix, pix)
        u_off, v_off = (first, first + pix) if color == "nv12" else (first + pix, first)
        return H, W, pitch, pix, u_off, v_off, pitch, 2 * pix
    want = 2 if color in ("nv12", "nv21") else 3
    if len(shapes) != want:
        raise _lib.CenterposeHipError("a %s frame is %s, got %d tensors" % (color, "(y, uv) or one surface" if want == 2 else "(y, u, v)",
                                                                          len(shapes)))
    if len(shapes[0]) != 2:
        raise _lib.CenterposeHipError("the y plane is 2-D [H,W], got shape %s" % (shapes[0],))
    H, W = shapes[0]
    if H <= 0 or W <= 0:
        raise _lib.CenterposeHipError("a frame of shape %s has no pixels" % (shapes[0],))
    ch, cw = (H + 1) // 2, (W + 1) // 2
    if want == 2:
        if shapes[1] != (ch, cw, 2):
            raise _lib.CenterposeHipError("the uv plane of a %d x %d %s frame is [%d,%d,2], got shape %s" % (H, W, color, ch, cw, shapes[1]))
        c_row, c_pix, sc = strides[1]
        u_off, v_off = (0, sc) if color == "nv12" else (sc, 0)
    else:
        if shapes[1] != (ch, cw) or shapes[2] != (ch, cw):
            raise _lib.CenterposeHipError("the u and v planes of a %d x %d i420 frame are [%d,%d], got shapes %s and %s"
                                          % (H, W, ch, cw, shapes[1], shapes[2]))
        if strides[1] != strides[2]:
            raise _lib.CenterposeHipError("the u and v planes must have equal strides (%s and %s)" % (strides[1], strides[2]))
        (c_row, c_pix), u_off, v_off = strides[1], 0, 0
    return H, W, strides[0][0], strides[0][1], u_off, v_off, c_row, c_pix


def frame_writable(shape, strides):
    """Whether a view of the given shape and strides (in elements == bytes) may be WRITTEN: no two of its indices address the same
    byte.  The dimensions with more than one index, sorted by stride: each stride must be at least the extent (last addressed offset
    + 1) of the dimensions below it.  Sufficient, not necessary: crops, padded rows, planar and permuted views pass; expanded (stride
    0) and overlapping (as_strided windows) views and negative strides do not.  A pure function of its arguments."""
    dims = sorted((int(st), int(n)) for n, st in zip(shape, strides) if int(n) > 1)
    if any(int(n) <= 0 for n in shape):
        return False
    extent = 1
    for st, n in dims:
        if st < extent:
            return False
        extent += (n - 1) * st
    return True


def byte_range(address, shape, strides):
    """[first, last + 1) of the bytes a uint8 view with non-negative strides addresses from `address`."""
    return int(address), int(address) + sum((int(n) - 1) * int(st) for n, st in zip(shape, strides)) + 1


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


class _Staging:
    """A pinned host buffer that grows on demand, and ONE stream-ordered upload of its first bytes per use.  `host()` waits for the
    previous upload to have left the buffer before handing it out again (an event on that copy alone, not a device synchronisation)."""

    def __init__(self):
        self.buf = None
        self.event = None

    def host(self, nbytes):
        if self.event is not None:
            self.event.synchronize()
            self.event = None
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, pin_memory=True)
        return self.buf.numpy()[:nbytes]

    def upload(self, nbytes):
        dev = torch.empty(int(nbytes), dtype=torch.uint8, device="cuda")
        dev.copy_(self.buf[:nbytes], non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()
        return dev


def invert_warp(M):
    """The inversion cv2.warpAffine applies to its 2x3 matrix, by the library's own double operations (cp_invert_warp: the ones
    cp_preprocess_u8_f32 uses) -> float64 [6]."""
    M = np.ascontiguousarray(M, np.float64).reshape(6)
    Mi = np.empty(6, np.float64)
    _lib.check(_lib.lib().cp_invert_warp(M.ctypes.data_as(ctypes.c_void_p), Mi.ctypes.data_as(ctypes.c_void_p)), "cp_invert_warp")
    return Mi


def post_merge_batch(dets, trans=None, scales=None, nms=False, sigma=0.5, Nt=0.3, threshold=0.001, method=0):
    """cp_post_merge_batch_f32: dets, a list of S device tensors [N,K,56] (one per scale) -> (rows [N,S*K,56], n_keep int32 [N]), both
    on the device.  trans: device float64 [S,N,6] feature-map -> image affines with `scales` (S floats), or None for rows that are
    mapped already; nms: soft_nms_39 per image with the given parameters (at most 512 rows per image)."""
    S = len(dets)
    if S < 1 or any(d.dim() != 3 or d.shape != dets[0].shape or d.shape[2] != 56 for d in dets):
        raise _lib.CenterposeHipError("post_merge_batch expects per scale one [N,K,56] tensor of the same shape")
    dets = [_lib.f32(d.detach(), "dets").contiguous() for d in dets]
    N, K = int(dets[0].shape[0]), int(dets[0].shape[1])
    if trans is not None and (trans.dtype != torch.float64 or tuple(trans.shape) != (S, N, 6) or scales is None or len(scales) != S):
        raise _lib.CenterposeHipError("post_merge_batch: trans must be float64 [S,N,6] with S scales")
    out = torch.empty((N, S * K, 56), dtype=torch.float32, device=dets[0].device)
    n_keep = torch.empty((N,), dtype=torch.int32, device=dets[0].device)
    ptrs = (ctypes.c_void_p * S)(*[_lib.ptr(d).value for d in dets])
    sc = (ctypes.c_float * S)(*[float(v) for v in (scales if trans is not None else [1.0] * S)])
    rc = _lib.lib().cp_post_merge_batch_f32(S, ptrs, _lib.ptr(trans.contiguous()) if trans is not None else None, sc, N, K, _lib.ptr(out),
                                            _lib.c_void_p(n_keep.data_ptr()), 1 if nms else 0, _lib.c_float(sigma), _lib.c_float(Nt),
                                            _lib.c_float(threshold), int(method), _lib.stream())
    _lib.check(rc, "cp_post_merge_batch_f32")
    return out, n_keep


class BaseDetector(object):
    def __init__(self, cfg):
        print("Creating model...")
        self.model = create_model(cfg.MODEL.NAME, cfg.MODEL.HEAD_CONV, cfg)
        if cfg.TEST.MODEL_PATH:
            self.model = load_model(self.model, cfg.TEST.MODEL_PATH)
        self.model = self.model.to(torch.device("cuda"))
        self.model.eval()
        self.mean = np.array(cfg.DATASET.MEAN, dtype=np.float32).reshape(1, 1, 3)
        self.std = np.array(cfg.DATASET.STD, dtype=np.float32).reshape(1, 1, 3)
        self.max_per_image = 100
        self.num_classes = cfg.MODEL.NUM_CLASSES
        self.scales = cfg.TEST.TEST_SCALES
        self.cfg = cfg
        self.pause = True

    # -- geometry of one (image, scale) ----------------------------------------------------------------------------------
    def input_geometry(self, height, width, scale):
        """(new_h, new_w, inp_h, inp_w, c, s) of base_detector.py:33-46: the resized image size, the network input size and
        the centre / extent the affine maps onto it.  FIX_RES: fixed INPUT_H x INPUT_W, longer image side fills it;
        otherwise the resized image is padded up to the next multiple of PAD + 1 and centred."""
        cfg = self.cfg
        new_h, new_w = int(height * scale), int(width * scale)
        if cfg.TEST.FIX_RES:
            return (new_h, new_w, cfg.MODEL.INPUT_H, cfg.MODEL.INPUT_W,
                    np.array([new_w / 2., new_h / 2.], dtype=np.float32), max(height, width) * 1.0)
        inp_h, inp_w = (new_h | cfg.MODEL.PAD) + 1, (new_w | cfg.MODEL.PAD) + 1
        return (new_h, new_w, inp_h, inp_w, np.array([new_w // 2, new_h // 2], dtype=np.float32),
                np.array([inp_w, inp_h], dtype=np.float32))

    def pre_process(self, image, scale, meta=None, layout="hwc", color="bgr", matrix="bt601"):
        """base_detector.py:32-62.  image: HxWx3 uint8 BGR host array -> (images float32 [1 or 2,3,inp_h,inp_w] ON THE
        DEVICE, meta).  cv2.resize + cv2.warpAffine + normalise + transpose (+ flipped twin) run as HIP kernels.
        image may also be one frame that is already on the device: a CUDA uint8 tensor [H,W,C] (layout="hwc") or [C,H,W] ("chw"),
        C = 3 or 4, channels in memory in `color` order ("bgr" / "rgb"), any strides.  It is read in place (no copy, no upload) by
        pre_process_batch's device path, whose stream-order and lifetime rules apply; the result is bit-identical to the same call
        on the equivalent HxWx3 BGR host array.  Host arrays are cv2's layout: another layout / color raises for them.
        color "nv12" / "nv21" / "i420": image is one 4:2:0 YUV frame on the device (a tuple of plane tensors or, for nv12 / nv21, one
        surface tensor), converted with `matrix` ("bt601" / "bt709") -- see pre_process_batch."""
        _check_layout(layout, color, matrix)
        if color in YUV_COLORS:
            x, metas = self.pre_process_batch([image], scale, layout, color, matrix)
            return x, metas[0]
        if isinstance(image, torch.Tensor):
            if image.dim() != 3:
                raise _lib.CenterposeHipError("pre_process takes one 3-D frame tensor, got shape %s (N frames: pre_process_batch)"
                                              % (tuple(image.shape),))
            x, metas = self.pre_process_batch([image], scale, layout, color)
            return x, metas[0]
        self._host_layout_only(layout, color)
        if not (isinstance(image, np.ndarray) and image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3):
            raise _lib.CenterposeHipError("pre_process expects an HxWx3 uint8 array (cv2.imread layout); there is no host fallback")
        height, width = image.shape[0:2]
        new_h, new_w, inp_h, inp_w, c, s = self.input_geometry(height, width, scale)
        L = _lib.lib()
        src = torch.from_numpy(np.ascontiguousarray(image)).cuda()
        if (new_h, new_w) != (height, width):                  # base_detector.py:47 (cv2.resize copies when the size is unchanged)
            resized = torch.empty((new_h, new_w, 3), dtype=torch.uint8, device="cuda")
            _lib.check(L.cp_resize_u8(ctypes.c_void_p(src.data_ptr()), height, width, ctypes.c_void_p(resized.data_ptr()),
                                      new_h, new_w, _lib.stream()), "cp_resize_u8")
            src = resized
        trans_input = np.ascontiguousarray(get_affine_transform(c, s, 0, [inp_w, inp_h]), np.float64)
        nb = 2 if self.cfg.TEST.FLIP_TEST else 1
        images = torch.empty((nb, 3, inp_h, inp_w), dtype=torch.float32, device="cuda")
        mean = np.ascontiguousarray(self.mean.reshape(3), np.float32)
        std = np.ascontiguousarray(self.std.reshape(3), np.float32)
        _lib.check(L.cp_preprocess_u8_f32(ctypes.c_void_p(src.data_ptr()), new_h, new_w, trans_input.ctypes.data_as(ctypes.c_void_p),
                                          _lib.ptr(images), inp_h, inp_w, mean.ctypes.data_as(ctypes.c_void_p),
                                          std.ctypes.data_as(ctypes.c_void_p), 1 if nb == 2 else 0, _lib.stream()),
                   "cp_preprocess_u8_f32")
        down = self.cfg.MODEL.DOWN_RATIO
        return images, {"c": c, "s": s, "out_height": inp_h // down, "out_width": inp_w // down}

    def process(self, images, return_time=False):
        raise NotImplementedError

    def post_process(self, dets, meta, scale=1):
        raise NotImplementedError

    def merge_outputs(self, detections):
        raise NotImplementedError

    # -- N images at once ------------------------------------------------------------------------------------------------
    def _staging(self, which):
        st = self.__dict__.setdefault("_staging_buffers", {})
        if which not in st:
            st[which] = _Staging()
        return st[which]

    @staticmethod
    def _check_batch(images):
        images = list(images)
        for im in images:
            if not (isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3 and im.shape[0] > 0
                    and im.shape[1] > 0):
                raise _lib.CenterposeHipError("run_batch / pre_process_batch expect HxWx3 uint8 arrays (cv2.imread layout); there is no host fallback")
        return images

    @staticmethod
    def _host_layout_only(layout, color, matrix="bt601"):
        _check_layout(layout, color, matrix)      # unknown names raise
        if (layout, color) != ("hwc", "bgr"):
            raise _lib.CenterposeHipError("host arrays are taken in cv2's layout (HxWx3, BGR): layout=%r / color=%r apply to frames "
                                          "on the device (CUDA uint8 tensors) only" % (layout, color))

    def _model_device(self):
        """The card the model's plans live on, with its index ("cuda" alone means the current device, as everywhere here)."""
        device = torch.device(self.model.device)
        return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())

    def _frame(self, t, layout, color):
        """One device frame -> (address of pixel (0,0), H, W, row_stride, pix_stride, ch_off), all from the tensor's own shape,
        strides and data pointer: a valid view cannot address outside its storage.  The tensor is never copied or made contiguous."""
        if not t.is_cuda:
            raise _lib.CenterposeHipError("a frame tensor on %s: frames given as tensors must be on the model's GPU (host frames are "
                                          "passed as numpy arrays); there is no host fallback" % t.device)
        if t.dtype != torch.uint8:
            raise _lib.CenterposeHipError("a frame tensor must be uint8 (got %s)" % t.dtype)
        geometry = frame_geometry(t.shape, t.stride(), layout, color)
        device = self._model_device()
        if t.device != device:
            raise _lib.CenterposeHipError("a frame tensor on %s, the model is on %s" % (t.device, device))
        return (t.data_ptr(),) + geometry

    def _yuv_frame(self, frame, color):
        """One device frame in 4:2:0 YUV -> (address of Y(0,0), H, W, y_row, y_pix, address of U(0,0), address of V(0,0), c_row, c_pix),
        all from the plane tensors' own shapes, strides and data pointers.  One 2-D surface tensor (nv12 / nv21) is split into the views
        t[:H] and t[H:].unflatten(1, (W // 2, 2)) by address alone.  Nothing is copied or made contiguous."""
        planes = [frame] if isinstance(frame, (torch.Tensor, np.ndarray)) else list(frame)
        if not planes:
            raise _lib.CenterposeHipError("a %s frame without planes" % color)
        if any(isinstance(t, np.ndarray) for t in planes):
            if all(isinstance(t, np.ndarray) for t in planes):
                raise _lib.CenterposeHipError("host arrays are taken in cv2's layout (HxWx3, BGR): color=%r applies to frames on the "
                                              "device (CUDA uint8 plane tensors) only" % color)
            raise _lib.CenterposeHipError("host arrays and device tensors mixed in one frame: pass all planes as CUDA tensors")
        if not all(isinstance(t, torch.Tensor) for t in planes):
            raise _lib.CenterposeHipError("a %s frame is a tuple of CUDA uint8 plane tensors (or one surface tensor for nv12 / nv21)" % color)
        for t in planes:
            if not t.is_cuda:
                raise _lib.CenterposeHipError("a plane tensor on %s: the planes of a frame must be on the model's GPU; there is no host "
                                              "fallback" % t.device)
        H, W, y_row, y_pix, u_off, v_off, c_row, c_pix = yuv_frame_geometry([t.shape for t in planes], [t.stride() for t in planes], color,
                                                                            [t.dtype for t in planes])
        device = self._model_device()
        for t in planes:
            if t.device != device:
                raise _lib.CenterposeHipError("a plane tensor on %s, the model is on %s" % (t.device, device))
        u_plane, v_plane = (planes[0], planes[0]) if len(planes) == 1 else (planes[1], planes[-1])
        return (planes[0].data_ptr(), H, W, y_row, y_pix, u_plane.data_ptr() + u_off, v_plane.data_ptr() + v_off, c_row, c_pix)

    def _batch_input(self, images, layout, color, matrix="bt601"):
        """What a batched call was given -> (images as a list, frames): frames is None for host arrays (the staging path), else one
        `_frame` per device tensor (`_yuv_frame` per frame with a YUV color).  One 4-D tensor means N frames ([N,H,W,C] or [N,C,H,W])."""
        _check_layout(layout, color, matrix)      # unknown names raise, whatever the input
        if color in YUV_COLORS:
            if isinstance(images, (torch.Tensor, np.ndarray)):
                raise _lib.CenterposeHipError("a batch of %s frames is a list of frames (plane tuples or surface tensors), got one %s of "
                                              "shape %s" % (color, type(images).__name__, tuple(images.shape)))
            images = list(images)
            host = sum(isinstance(im, np.ndarray) for im in images)
            if 0 < host < len(images):
                raise _lib.CenterposeHipError("host arrays and device tensors mixed in one call: pass all frames one way")
            return images, [self._yuv_frame(im, color) for im in images]
        if isinstance(images, torch.Tensor):
            if images.dim() != 4:
                raise _lib.CenterposeHipError("one tensor for N frames is 4-D ([N,H,W,C] or [N,C,H,W]), got shape %s; pass a list of "
                                              "3-D frames otherwise" % (tuple(images.shape),))
            images = images.unbind(0)
        images = list(images)
        tensors = sum(isinstance(im, torch.Tensor) for im in images)
        if tensors == 0:
            if images:
                self._host_layout_only(layout, color)
            return self._check_batch(images), None
        if tensors != len(images):
            raise _lib.CenterposeHipError("host arrays and device tensors mixed in one call: pass all frames one way")
        return images, [self._frame(t, layout, color) for t in images]

    @staticmethod
    def _batch_layout(shapes):
        """Byte offset of every image in the one staging buffer (images back to back) and the buffer's size."""
        offsets, pos = [], 0
        for h, w in shapes:
            offsets.append(pos)
            pos += h * w * 3
        return offsets, pos

    def _batch_groups(self, shapes):
        """Indices of the images grouped by the network input shape they get at every TEST_SCALES entry (one batch per group and scale),
        groups in order of first appearance, indices ascending.  FIX_RES: one group."""
        groups = {}
        for i, (h, w) in enumerate(shapes):
            key = tuple(self.input_geometry(h, w, scale)[2:4] for scale in self.scales)
            groups.setdefault(key, []).append(i)
        return list(groups.values())

    def _pre_table(self, shapes, offsets, idx, scale, frames=None, yuv=False):
        """The descriptor table of one batched pre-process: images `idx` at `scale`, which must share one network input shape
        -> (table, scratch_bytes, inp_h, inp_w, metas).  Geometry, matrix and meta per image are pre_process's.  PRE_DESC rows with the
        images' staging `offsets`, or, with `frames` (`_frame` per image), FRAME_DESC rows that address the frames where they lie
        (`yuv`: `_yuv_frame` per image, YUV_FRAME_DESC rows)."""
        nb = 2 if self.cfg.TEST.FLIP_TEST else 1
        down = self.cfg.MODEL.DOWN_RATIO
        table = np.zeros(len(idx), PRE_DESC if frames is None else (YUV_FRAME_DESC if yuv else FRAME_DESC))
        metas, scratch, inp = [], 0, None
        for j, i in enumerate(idx):
            height, width = shapes[i]
            new_h, new_w, inp_h, inp_w, c, s = self.input_geometry(height, width, scale)
            if new_h <= 0 or new_w <= 0:
                raise _lib.CenterposeHipError("image %d x %d at scale %s has no pixels" % (height, width, scale))
            if inp is None:
                inp = (inp_h, inp_w)
            elif inp != (inp_h, inp_w):
                raise _lib.CenterposeHipError("pre_process_batch needs one network input shape per call (%s and %s at scale %s): "
                                              "run_batch groups mixed sizes" % (inp, (inp_h, inp_w), scale))
            d = table[j]
            d["H"], d["W"], d["NH"], d["NW"], d["slot"] = height, width, new_h, new_w, nb * j
            if frames is None:
                d["src_off"] = offsets[i]
            elif yuv:
                d["y_base"], _, _, d["y_row"], d["y_pix"], d["u_base"], d["v_base"], d["c_row"], d["c_pix"] = frames[i]
            else:
                d["base"], _, _, d["row_stride"], d["pix_stride"], d["ch_off"] = frames[i]
            if (new_h, new_w) != (height, width):
                d["mid_off"] = scratch
                scratch += new_h * new_w * 3
            else:
                d["mid_off"] = -1
            d["mi"] = invert_warp(get_affine_transform(c, s, 0, [inp_w, inp_h]))
            metas.append({"c": c, "s": s, "out_height": inp_h // down, "out_width": inp_w // down})
        return table, scratch, inp[0], inp[1], metas

    @staticmethod
    def _inverse_affines(metas):
        """float64 [N,6]: post_process's feature-map -> image matrix per image."""
        return np.stack([np.ascontiguousarray(get_affine_transform(m["c"], m["s"], 0, (m["out_width"], m["out_height"]), inv=1),
                                              np.float64).reshape(6) for m in metas])

    def _upload_images(self, images, offsets, nbytes):
        """The N images into the pinned staging buffer, ONE host-to-device copy -> device uint8 [nbytes]."""
        st = self._staging("images")
        host = st.host(nbytes)
        for im, off in zip(images, offsets):
            host[off:off + im.size] = im.reshape(-1)
        return st.upload(nbytes)

    def _upload_table(self, parts):
        """Host arrays (descriptor tables, affines; 8-byte items) back to back in the pinned table buffer, ONE copy -> the device
        uint8 views of the parts."""
        raw = [np.ascontiguousarray(p).view(np.uint8).reshape(-1) for p in parts]
        st = self._staging("table")
        host = st.host(sum(r.size for r in raw))
        pos, spans = 0, []
        for r in raw:
            host[pos:pos + r.size] = r
            spans.append((pos, r.size))
            pos += r.size
        dev = st.upload(pos)
        return [dev[a:a + n] for a, n in spans]

    def _launch_pre(self, staging, table_dev, table, scratch_bytes, inp_h, inp_w):
        """cp_preprocess_batch_u8_f32 for one table -> float32 [nb * N, 3, inp_h, inp_w] on the device."""
        nb, n, x, scratch, mean, std, table = self._pre_buffers(table, scratch_bytes, inp_h, inp_w)
        rc = _lib.lib().cp_preprocess_batch_u8_f32(
            ctypes.c_void_p(staging.data_ptr()), ctypes.c_size_t(staging.numel()), ctypes.c_void_p(scratch.data_ptr()),
            ctypes.c_size_t(scratch_bytes), ctypes.c_void_p(table_dev.data_ptr()), table.ctypes.data_as(ctypes.c_void_p), n, _lib.ptr(x),
            nb * n, inp_h, inp_w, mean.ctypes.data_as(ctypes.c_void_p), std.ctypes.data_as(ctypes.c_void_p), 1 if nb == 2 else 0,
            _lib.stream())
        _lib.check(rc, "cp_preprocess_batch_u8_f32")
        return x

    def _pre_buffers(self, table, scratch_bytes, inp_h, inp_w):
        """What both pre-process launches need: (nb, N, the output batch, the scratch buffer, mean, std, the table contiguous)."""
        nb = 2 if self.cfg.TEST.FLIP_TEST else 1
        n = len(table)
        x = torch.empty((nb * n, 3, inp_h, inp_w), dtype=torch.float32, device="cuda")
        scratch = torch.empty((max(scratch_bytes, 1),), dtype=torch.uint8, device="cuda")
        mean = np.ascontiguousarray(self.mean.reshape(3), np.float32)
        std = np.ascontiguousarray(self.std.reshape(3), np.float32)
        return nb, n, x, scratch, mean, std, np.ascontiguousarray(table)

    def _launch_frames(self, table_dev, table, scratch_bytes, inp_h, inp_w, coef=None):
        """cp_preprocess_frames_u8_f32 for one FRAME_DESC table -> float32 [nb * N, 3, inp_h, inp_w] on the device.  With `coef` (six
        ints, YUV_MATRICES): cp_preprocess_yuv_frames_u8_f32 for one YUV_FRAME_DESC table."""
        nb, n, x, scratch, mean, std, table = self._pre_buffers(table, scratch_bytes, inp_h, inp_w)
        if coef is not None:
            rc = _lib.lib().cp_preprocess_yuv_frames_u8_f32(
                ctypes.c_void_p(table_dev.data_ptr()), table.ctypes.data_as(ctypes.c_void_p), n, (ctypes.c_int * 6)(*coef),
                ctypes.c_void_p(scratch.data_ptr()), ctypes.c_size_t(scratch_bytes), _lib.ptr(x), nb * n, inp_h, inp_w,
                mean.ctypes.data_as(ctypes.c_void_p), std.ctypes.data_as(ctypes.c_void_p), 1 if nb == 2 else 0, _lib.stream())
            _lib.check(rc, "cp_preprocess_yuv_frames_u8_f32")
            return x
        rc = _lib.lib().cp_preprocess_frames_u8_f32(
            ctypes.c_void_p(table_dev.data_ptr()), table.ctypes.data_as(ctypes.c_void_p), n, ctypes.c_void_p(scratch.data_ptr()),
            ctypes.c_size_t(scratch_bytes), _lib.ptr(x), nb * n, inp_h, inp_w, mean.ctypes.data_as(ctypes.c_void_p),
            std.ctypes.data_as(ctypes.c_void_p), 1 if nb == 2 else 0, _lib.stream())
        _lib.check(rc, "cp_preprocess_frames_u8_f32")
        return x

    def pre_process_batch(self, images, scale, layout="hwc", color="bgr", matrix="bt601"):
        """pre_process for N images that share one network input shape at `scale` (any sizes with FIX_RES) -> (float32
        [nb * N, 3, inp_h, inp_w] ON THE DEVICE, list of N meta dicts); nb = 2 with FLIP_TEST: image n at 2n, its mirrored twin at
        2n + 1, the layout `process` takes.  One upload of the images, one of the descriptor table, one resize launch (if any image
        is resized) and one warp launch; every image bit-identical to pre_process(image, scale).
        Frames on the device: `images` is a list of CUDA uint8 tensors, each [H,W,C] (layout="hwc") or [C,H,W] ("chw") with C = 3 or 4,
        channels in `color` order ("bgr" / "rgb") and any strides (crops, padded rows, planar, expanded), or one 4-D tensor of N such
        frames.  They are read where they lie (cp_preprocess_frames_u8_f32): the descriptor table is the only upload, there is no
        staging copy and no `.contiguous()`; bit-identical to the call on the equivalent HxWx3 BGR host arrays.  The launches go to
        the current stream: whatever produced the frames must be ordered before this call on that stream, and a frame must stay
        allocated until the launches have run -- a tensor that was allocated on another stream needs `record_stream` for the
        current one before it is released.  Host arrays and tensors cannot be mixed; host arrays take layout / color defaults only.
        Frames in 4:2:0 YUV: color "nv12" / "nv21" / "i420" (layout stays the default), `images` a list of frames, each a tuple of CUDA
        uint8 plane tensors -- (y [H,W], uv [ceil(H/2),ceil(W/2),2]) for nv12 (uv[..., 0] is U) and nv21 (uv[..., 0] is V), (y, u, v)
        with u, v [ceil(H/2),ceil(W/2)] of equal strides for i420 (YV12 is i420 with the planes passed in (y, u, v) order, i.e. the
        file's third plane second) -- or, for nv12 / nv21, one 2-D tensor [H*3/2, W] with even H, W and any row stride: a decoder's
        surface, split into its plane views here.  Any strides; nothing is copied.  cp_preprocess_yuv_frames_u8_f32 converts every
        pixel to BGR where it is loaded, with the limited-range `matrix` "bt601" (cv2's COLOR_YUV2BGR_NV12 arithmetic) or "bt709",
        nearest chroma: bit-identical to the call on the HxWx3 BGR host array that conversion gives (csrc/yuv_arith.h).  The
        stream-order and lifetime rules above hold for every plane.  Host YUV arrays are not taken."""
        images, frames = self._batch_input(images, layout, color, matrix)
        if not images:
            raise _lib.CenterposeHipError("pre_process_batch needs at least one image")
        if frames is not None:
            shapes = [f[1:3] for f in frames]
            coef = YUV_MATRICES[matrix] if color in YUV_COLORS else None
            table, scratch_bytes, inp_h, inp_w, metas = self._pre_table(shapes, None, list(range(len(frames))), scale, frames, coef is not None)
            table_dev, = self._upload_table([table])
            return self._launch_frames(table_dev, table, scratch_bytes, inp_h, inp_w, coef), metas
        shapes = [im.shape[0:2] for im in images]
        offsets, nbytes = self._batch_layout(shapes)
        table, scratch_bytes, inp_h, inp_w, metas = self._pre_table(shapes, offsets, list(range(len(images))), scale)
        staging = self._upload_images(images, offsets, nbytes)
        table_dev, = self._upload_table([table])
        return self._launch_pre(staging, table_dev, table, scratch_bytes, inp_h, inp_w), metas

    def _process_batch(self, images):
        raise NotImplementedError

    def process_dets(self, images):
        raise NotImplementedError

    def post_process_batch(self, dets, metas, scale=1):
        raise NotImplementedError

    def merge_outputs_batch(self, detections):
        raise NotImplementedError

    def run_batch(self, images, dets_only=False, layout="hwc", color="bgr", return_device=False, matrix="bt601", draw=False, embed=None,
                  track=None):
        """N images (HxWx3 uint8 BGR arrays, sizes may differ) -> list of N results, results[n] == run(images[n])["results"].
        One upload of the images and one of every descriptor table / affine of the call; per group of images with equal network input
        shapes and per TEST_SCALES entry a batched pre-process, ONE `process` of the whole group and a batched post-process; one merge
        launch per group (soft-NMS on the device when TEST.NMS or several scales); ONE download.  The download is the only
        synchronisation, so there are no stage timers: run() is the timed form.  With FLIP_TEST and a head gated off by cfg.LOSS
        `process` takes one pair at a time; the stages around it stay batched.
        dets_only=True: every group goes through `process_dets` (a detections-only plan, under FLIP_TEST too) instead of `process`;
        ValueError where `process_dets` raises it.
        Frames on the device: `images` as for pre_process_batch (a list of CUDA uint8 tensors or one 4-D tensor, `layout`, `color`);
        they are read in place, the descriptor tables are the call's only upload, and the results equal those of the same frames
        given as host arrays.  The same stream-order and lifetime rules hold.  Frames in 4:2:0 YUV (color "nv12" / "nv21" / "i420",
        `matrix`): a list of plane tuples or surface tensors as for pre_process_batch, the rules per plane; the results equal those of
        the converted BGR host arrays.
        return_device=True (host or device input): the rows as ONE device tensor float32 [N, S*K, 56] in input order instead of the
        list -- no download and no synchronisation; the tensor is ready in the current stream's order.
        draw=True (device frames only): once the rows are in input order the frames are painted with them, in place, as
        draw_results(images, rows, layout, color, matrix) does with the default threshold and style -- whose rules for writable frames
        apply and are checked before anything is launched.  The return value is exactly what it is without `draw`.
        embed=extractor (a reid.ReidExtractor; device frames only): -> (rows, result) with `rows` exactly what the call returns
        without `embed` and `result` the extractor's ReidResult for the call's own rows, once they are in input order, at
        TEST.VIS_THRESH -- what extractor.embed(images, rows, layout, color, matrix, vis_thresh=TEST.VIS_THRESH) gives.  With
        draw=True as well the crops are taken before anything is painted.  More frames than the extractor's capacity: ValueError,
        before anything is launched.
        track=tracker (a track.DeepSortTracker; needs embed=): -> (rows, result, tracks) with `rows` and `result` exactly what the call
        returns without `track` and `tracks` = tracker.update(rows, result, sizes) on the call's own rows in input order, frame n being
        stream n: a list of int64 [k, 5] arrays (x1, y1, x2, y2, track_id).  Taken before draw=True paints.  The tracker's download is
        a synchronisation of its own.  Without embed=, or with len(images) != tracker.streams: ValueError, before anything is launched."""
        given = images
        images, frames = self._batch_input(images, layout, color, matrix)
        coef = YUV_MATRICES[matrix] if color in YUV_COLORS else None
        if embed is not None:
            if frames is None:
                raise ValueError("embed= takes its crops from frames on the device (CUDA uint8 tensors): host arrays are not read, "
                                 "there is no CPU fallback")
            if not 1 <= len(images) <= embed.capacity:
                raise ValueError("%d frames for an extractor of capacity %d: every frame needs at least one slot" % (len(images), embed.capacity))
            if embed.device != self._model_device():
                raise _lib.CenterposeHipError("the extractor is on %s, the model is on %s" % (embed.device, self._model_device()))
        if track is not None:
            if embed is None:
                raise ValueError("track= needs embed=: the tracker matches the extractor's features")
            if len(images) != track.streams:
                raise ValueError("%d frames for a tracker of %d streams: frame n of a call belongs to stream n" % (len(images), track.streams))
            if track.capacity != embed.capacity:
                raise ValueError("the tracker was built for capacity %d, the extractor has %d" % (track.capacity, embed.capacity))
            if track.device != embed.device:
                raise _lib.CenterposeHipError("the tracker is on %s, the extractor is on %s" % (track.device, embed.device))
        if draw:
            if frames is None and images:
                raise _lib.CenterposeHipError("draw=True paints frames on the device (CUDA uint8 tensors): host arrays are not painted, "
                                              "there is no CPU fallback")
            self._check_writable(given, images, color)
        if not images:
            return torch.empty((0, 0, 56), dtype=torch.float32, device="cuda") if return_device else []
        shapes = [im.shape[0:2] for im in images] if frames is None else [f[1:3] for f in frames]
        offsets, nbytes = self._batch_layout(shapes) if frames is None else (None, 0)
        groups = self._batch_groups(shapes)
        work, parts = [], []
        for idx in groups:
            for scale in self.scales:
                table, scratch_bytes, inp_h, inp_w, metas = self._pre_table(shapes, offsets, idx, scale, frames, coef is not None)
                work.append((table, scratch_bytes, inp_h, inp_w))
                parts += [table, self._inverse_affines(metas)]
        order = [i for idx in groups for i in idx]               # merged row block r belongs to image order[r]
        if (return_device or draw or embed is not None) and len(groups) > 1:
            parts.append(np.argsort(np.asarray(order, np.int64)).astype(np.int64))       # rides in the one table upload
        staging = self._upload_images(images, offsets, nbytes) if frames is None else None
        parts = self._upload_table(parts)
        merged = []
        for g, idx in enumerate(groups):
            per_scale = []
            for k, scale in enumerate(self.scales):
                j = g * len(self.scales) + k
                table, scratch_bytes, inp_h, inp_w = work[j]
                if frames is None:
                    x = self._launch_pre(staging, parts[2 * j], table, scratch_bytes, inp_h, inp_w)
                else:
                    x = self._launch_frames(parts[2 * j], table, scratch_bytes, inp_h, inp_w, coef)
                dets = self.process_dets(x) if dets_only else self._process_batch(x)
                per_scale.append(self._launch_post(dets, parts[2 * j + 1].view(torch.float64).view(1, len(idx), 6), scale))
            merged.append(self.merge_outputs_batch(per_scale))
        rows = merged[0] if len(merged) == 1 else torch.cat(merged, 0)
        ordered = result = None
        if draw or return_device or embed is not None:
            ordered = rows if len(groups) == 1 else rows.index_select(0, parts[-1].view(torch.int64))
        if embed is not None:                                    # from the frames as they were given: before anything is painted
            result = embed._embed(frames, ordered.contiguous(), color, matrix, float(self.cfg.TEST.VIS_THRESH))
        tracks = None
        if track is not None:                                    # before anything is painted, like the crops
            tracks = track.update(ordered, result, [(int(w), int(h)) for h, w in shapes])
        if draw:
            self._draw(images, frames, ordered, color, matrix, None, None)
        if return_device:
            return ordered if embed is None else (ordered, result) if track is None else (ordered, result, tracks)
        rows = rows.cpu().numpy()                                                               # the one download
        results = [None] * len(images)
        for r, i in enumerate(order):
            results[i] = {1: rows[r].tolist()}
        return results if embed is None else (results, result) if track is None else (results, result, tracks)

    @staticmethod
    def _check_writable(given, images, color):
        """Raise unless every frame of a call may be written: every tensor a view without self-overlap (frame_writable), the luma
        bytes of a plane tuple apart from its chroma bytes, and no tensor given twice."""
        if isinstance(given, torch.Tensor) and not frame_writable(given.shape, given.stride()):
            raise _lib.CenterposeHipError("the frames tensor of shape %s and strides %s cannot be written: two of its indices address the "
                                          "same byte" % (tuple(given.shape), tuple(given.stride())))
        seen = set()
        for n, im in enumerate(images):
            planes = [im] if isinstance(im, torch.Tensor) else list(im)
            for t in planes:
                if not frame_writable(t.shape, t.stride()):
                    raise _lib.CenterposeHipError("frame %d: a view of shape %s and strides %s cannot be written: two of its indices address "
                                                  "the same byte (expanded or overlapping view)" % (n, tuple(t.shape), tuple(t.stride())))
                key = (t.data_ptr(), tuple(t.shape), tuple(t.stride()))
                if key in seen:
                    raise _lib.CenterposeHipError("frame %d: the same tensor is given twice in one call" % n)
                seen.add(key)
            if color in YUV_COLORS and len(planes) > 1:
                y0, y1 = byte_range(planes[0].data_ptr(), planes[0].shape, planes[0].stride())
                for t in planes[1:]:
                    c0, c1 = byte_range(t.data_ptr(), t.shape, t.stride())
                    if c0 < y1 and y0 < c1:
                        raise _lib.CenterposeHipError("frame %d: the luma plane and a chroma plane share bytes" % n)

    def _draw(self, images, frames, rows, color, matrix, vis_thresh, style):
        """cp_draw_rows_frames_u8 / cp_draw_rows_yuv_frames_u8 for checked frames (`_frame` / `_yuv_frame` per image) and device rows
        [N,M,56]: one table upload, two launches in the current stream."""
        yuv = color in YUV_COLORS
        style = DrawStyle() if style is None else style
        if not isinstance(style, DrawStyle):
            raise _lib.CenterposeHipError("style is a DrawStyle (got %s)" % type(style).__name__)
        vis_thresh = float(self.cfg.TEST.VIS_THRESH if vis_thresh is None else vis_thresh)
        N, M = len(images), int(rows.shape[1])
        if N == 0 or M == 0:
            return
        table = np.zeros(N, YUV_FRAME_DESC if yuv else FRAME_DESC)
        for n, f in enumerate(frames):
            d = table[n]
            if yuv:
                d["y_base"], d["H"], d["W"], d["y_row"], d["y_pix"], d["u_base"], d["v_base"], d["c_row"], d["c_pix"] = f
            else:
                d["base"], d["H"], d["W"], d["row_stride"], d["pix_stride"], d["ch_off"] = f
            d["NH"], d["NW"], d["mid_off"] = d["H"], d["W"], -1
        table = np.ascontiguousarray(table)
        rec = style.struct(matrix if yuv else None)
        L = _lib.lib()
        L.cp_draw_scratch_bytes.restype = ctypes.c_size_t
        nbytes = int(L.cp_draw_scratch_bytes(N, M))
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=rows.device)
        table_dev, = self._upload_table([table])
        fn = L.cp_draw_rows_yuv_frames_u8 if yuv else L.cp_draw_rows_frames_u8
        rc = fn(ctypes.c_void_p(table_dev.data_ptr()), table.ctypes.data_as(ctypes.c_void_p), N, ctypes.c_void_p(rows.data_ptr()), M,
                ctypes.c_float(vis_thresh), rec.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(scratch.data_ptr()),
                ctypes.c_size_t(nbytes), _lib.stream())
        _lib.check(rc, "cp_draw_rows_yuv_frames_u8" if yuv else "cp_draw_rows_frames_u8")

    def draw_results(self, frames, rows, layout="hwc", color="bgr", matrix="bt601", vis_thresh=None, style=None):
        """Paint the detections `rows` onto `frames`, in place, on the device, in the current stream -> `frames`.  What is drawn is
        what the reference's show_results draws, without the text: per row with score > vis_thresh (default cfg.TEST.VIS_THRESH) the
        box, the limbs whose two joints both score > 0 and the joints that score > 0, opaque, rows in ascending order, box then limbs
        then joints, the last painted wins.  The rule is this project's own, integer-only and bit-exact between the device, the host
        painter cp_draw_rows_frames_host and a NumPy restatement (csrc/draw_arith.h).
        frames: as for pre_process_batch -- a list of CUDA uint8 tensors or one 4-D tensor (`layout`, `color`, C = 3 or 4), or with
        color "nv12" / "nv21" / "i420" a list of plane tuples / surface tensors; for those the palette is converted to (Y, U, V) with
        `matrix` (palette_to_yuv), luma is written per pixel and a chroma sample takes the latest-painted colour among its 2x2 pixels.
        Three bytes per covered pixel: a fourth channel, row padding and everything outside a view keep their bytes.
        rows: CUDA float32 [N, M, 56] in image coordinates, as run_batch(..., return_device=True) returns them ([M, 56]: one frame).
        style: a DrawStyle.  The descriptor table is the only upload; nothing is downloaded and nothing synchronises.
        A frame is WRITTEN here, so beyond the stream-order and lifetime rules of pre_process_batch, which hold unchanged: every tensor
        must be a view in which no two indices address one byte (frame_writable: expanded and overlapping views raise), a plane
        tuple's luma bytes must lie apart from its chroma bytes, the same tensor may not be given twice -- and that the frames of one
        call share no bytes otherwise is the caller's promise.  Host arrays raise: there is no CPU fallback."""
        given = frames
        images, descs = self._batch_input(frames, layout, color, matrix)
        if descs is None and images:
            raise _lib.CenterposeHipError("draw_results paints frames on the device (CUDA uint8 tensors): host arrays are not painted, "
                                          "there is no CPU fallback")
        if isinstance(rows, np.ndarray) or not isinstance(rows, torch.Tensor):
            raise _lib.CenterposeHipError("rows must be a CUDA float32 tensor [N, M, 56] on the device (got %s): there is no CPU fallback"
                                          % type(rows).__name__)
        if rows.dim() == 2:
            rows = rows.unsqueeze(0)
        if rows.dim() != 3 or rows.shape[2] != 56:
            raise _lib.CenterposeHipError("rows must be [N, M, 56] (or [M, 56] for one frame), got shape %s" % (tuple(rows.shape),))
        if not rows.is_cuda:
            raise _lib.CenterposeHipError("rows on %s: they must be on the model's GPU; there is no CPU fallback" % rows.device)
        if rows.device != self._model_device():
            raise _lib.CenterposeHipError("rows on %s, the model is on %s" % (rows.device, self._model_device()))
        if rows.dtype != torch.float32:
            raise _lib.CenterposeHipError("rows must be float32 (got %s)" % rows.dtype)
        if rows.shape[0] != len(images):
            raise _lib.CenterposeHipError("rows hold %d blocks for %d frames" % (rows.shape[0], len(images)))
        self._check_writable(given, images, color)
        self._draw(images, descs or [], rows.detach().contiguous(), color, matrix, vis_thresh, style)
        return given

    def _source(self, x, layout="hwc", color="bgr", matrix="bt601"):
        if isinstance(x, (np.ndarray, torch.Tensor)) or (color in YUV_COLORS and isinstance(x, (tuple, list))):
            return _ArraySource(x, layout, color, matrix)
        if isinstance(x, str):
            return _ArraySource(_imread(x), layout, color, matrix)
        return _PreparedSource(x)

    def run(self, image_or_path_or_tensor, meta=None, layout="hwc", color="bgr", matrix="bt601"):
        """base_detector.py:79-140: every TEST_SCALES entry through pre_process -> process -> post_process, then
        merge_outputs; returns {'results': {1: rows}, 'tot', 'load', 'pre', 'net', 'dec', 'post', 'merge'}.
        A CUDA uint8 tensor is one frame on the device in the given `layout` / `color` (see pre_process): read in place, same results
        as the equivalent host array.  With color "nv12" / "nv21" / "i420": one 4:2:0 YUV frame on the device (plane tuple or surface
        tensor, `matrix`), as for pre_process."""
        _check_layout(layout, color, matrix)
        clock = StageClock(torch.cuda.synchronize)
        source = self._source(image_or_path_or_tensor, layout, color, matrix)
        clock.lap("load", sync=False)
        per_scale = []
        for scale in self.scales:
            images, meta = source.at_scale(self, scale, meta)
            images = images.to(torch.device("cuda"))
            clock.lap("pre")
            _, dets, forward_done = self.process(images, return_time=True)
            clock.split("net", forward_done)
            clock.lap("dec")
            per_scale.append(self.post_process(dets, meta, scale))
            clock.lap("post")
        results = self.merge_outputs(per_scale)
        clock.lap("merge")
        return clock.report(results)


class MultiPoseDetector(BaseDetector):
    def __init__(self, cfg):
        super(MultiPoseDetector, self).__init__(cfg)
        self.flip_idx = FLIP_IDX
        perm = list(range(17))
        for a, b in FLIP_IDX:
            perm[a], perm[b] = b, a
        self._perm = torch.tensor(perm, dtype=torch.int32, device="cuda")

    def _flip_merge(self, t, mode):
        if t.shape[0] != 2:      # the reference's hm[0:1] + flip(hm[1:2]) (multi_pose.py:45-53) is only defined for image + mirrored twin
            raise ValueError("FLIP_TEST needs a batch of exactly 2 (image + mirrored twin), got %d" % t.shape[0])
        out = torch.empty((1,) + tuple(t.shape[1:]), dtype=torch.float32, device=t.device)
        rc = _lib.lib().cp_flip_merge_f32(_lib.ptr(t.contiguous()), _lib.ptr(out), t.shape[1], t.shape[2], t.shape[3], mode,
                                          _lib.c_void_p(self._perm.data_ptr()), _lib.stream())
        _lib.check(rc, "cp_flip_merge_f32")
        return out

    def _one_replay_path(self):
        """forward + decode can be ONE graph replay: nothing to do between them (no flip merge, no head gated off)."""
        loss = self.cfg.LOSS
        return (not self.cfg.TEST.FLIP_TEST and loss.REG_OFFSET and loss.HM_HP and loss.REG_HP_OFFSET and not loss.MSE_LOSS
                and hasattr(self.model, "process"))

    def _flip_replay_path(self):
        """The flip test as ONE graph replay (model.process(..., flip_test=True)): FLIP_TEST on, every head enabled by cfg.LOSS (the
        plan merges and decodes all six), a model with the one-replay process().  `return_time` keeps the two-stage path."""
        loss = self.cfg.LOSS
        return (self.cfg.TEST.FLIP_TEST and loss.REG_OFFSET and loss.HM_HP and loss.REG_HP_OFFSET and not loss.MSE_LOSS
                and hasattr(self.model, "process"))

    def _dets_only_refusal(self, return_time=False):
        """Why `dets_only=True` cannot run here, or None.  The mode exists on the one-replay path only: the flip merge needs the
        mirrored maps at every pixel, a head gated off by cfg.LOSS changes what the decode reads, and the 'net' / 'dec' timers of
        `return_time` time a forward and a decode that a detections-only step does not separate."""
        loss = self.cfg.LOSS
        if return_time:
            return "dets_only=True cannot time 'net' / 'dec' separately (return_time=True)"
        if self.cfg.TEST.FLIP_TEST:
            return ("dets_only=True does not support TEST.FLIP_TEST here (this call hands out head maps, and the flip merge needs the "
                    "dense ones): use process_dets(images) or run_batch(images, dets_only=True)")
        if not (loss.REG_OFFSET and loss.HM_HP and loss.REG_HP_OFFSET and not loss.MSE_LOSS):
            return "dets_only=True needs every head enabled by cfg.LOSS (REG_OFFSET, HM_HP, REG_HP_OFFSET, no MSE_LOSS)"
        if not self._one_replay_path():
            return "dets_only=True needs a model with the one-replay process()"
        return None

    def process_stream(self, batches, depth=2, dets_only=False):
        """See `_stream`.  dets_only=True: detections-only plans (`process`); refused with ValueError where `process` refuses it --
        checked here, before the first batch is taken."""
        if dets_only:
            why = self._dets_only_refusal()
            if why:
                raise ValueError(why)
        return self._stream(batches, depth, dets_only)

    def _stream(self, batches, depth=2, dets_only=False):
        """`process` over an iterable of image batches with `depth` steps in flight (model.BackBoneWithHead.process_many): a
        generator of `(outputs, dets)` per batch, in order, each bit-identical to `process(batch)`.  Two consecutive batches are
        captured into one hipGraph so that one step's kernels fill the other's launch gaps: throughput up, a batch's result
        available only with its group (latency ~ depth x).  Configurations that need host logic between forward and decode
        (FLIP_TEST, a head gated off by cfg.LOSS) run batch by batch through `process`.  The batched-throughput entry point of
        BASELINE.json's metric; the reference has one image at a time (multi_pose.py:29-60, base_detector.py:79-140)."""
        extra = {"dets_only": True} if dets_only else {}      # the default calls stay exactly what they were
        if self._one_replay_path() and hasattr(self.model, "process_many"):
            # (no torch.no_grad() around the yields: a grad mode entered inside a generator leaks into the consumer between
            # yields; nothing on this path records autograd history anyway -- raw HIP launches and a clone of a plain tensor)
            for r in self.model.process_many(batches, self.cfg.TEST.TOPK, depth, **extra):
                yield r
            return
        for images in batches:
            yield self.process(images, **extra)

    def process(self, images, return_time=False, dets_only=False):
        """multi_pose.py:29-60.  images: float32 NCHW, mean/std-normalised, on the HIP device.
        FLIP_TEST: images are image / mirrored-twin pairs, image n at batch 2n and its twin at 2n + 1 (torch.cat of pre_process
        outputs) -> (the six un-merged maps, dets [B / 2, K, 56]) in one replay; return_time=True and heads gated off by cfg.LOSS keep
        the two-stage path with a batch of exactly 2.
        dets_only=True (opt-in): a detections-only plan -- hm / hm_hp dense, wh / hps / reg / hp_offset evaluated only at the
        decoded peaks -> ([hm, None, None, None, hm_hp, None], dets).  One-replay path only: FLIP_TEST, a head gated off by
        cfg.LOSS or return_time=True raise ValueError (there is no silent fall-back to the dense plan)."""
        if dets_only:
            why = self._dets_only_refusal(return_time)
            if why:
                raise ValueError(why)
            with torch.no_grad():
                return self.model.process(images, self.cfg.TEST.TOPK, dets_only=True)
        if not return_time and self._flip_replay_path():
            # the flip test for N = B / 2 image / mirrored-twin pairs in ONE replay: the merge and the decode of the merged maps are
            # inside the plan's schedule.  outputs: the six un-merged [B] maps (static buffers); dets: fresh, [N, K, 56].
            B = images.shape[0]
            if B < 2 or B % 2:
                raise ValueError("FLIP_TEST needs image / mirrored-twin pairs: an even batch [img0, twin0, img1, twin1, ...], got %d" % B)
            with torch.no_grad():
                return self.model.process(images, self.cfg.TEST.TOPK, flip_test=True)
        if not return_time and self._one_replay_path():
            # no stage timing asked for and nothing to do between forward and decode: both in ONE graph replay (the peak
            # extraction overlaps the last head convolutions).  `run()` keeps the two-stage form for its 'net' / 'dec' timers.
            # `dets` is a fresh tensor on both paths (the reference returns one); `outputs` are the plan's static buffers.
            with torch.no_grad():
                outputs, dets = self.model.process(images, self.cfg.TEST.TOPK)
            return outputs, dets
        with torch.no_grad():
            torch.cuda.synchronize()
            outputs = self.model(images)            # hm (and hm_hp) already sigmoided (fused epilogue)
            hm, wh, hps, reg, hm_hp, hp_offset = outputs
            reg = reg if self.cfg.LOSS.REG_OFFSET else None
            hm_hp = hm_hp if self.cfg.LOSS.HM_HP else None
            hp_offset = hp_offset if self.cfg.LOSS.REG_HP_OFFSET else None
            torch.cuda.synchronize()
            forward_time = time.time()
            if self.cfg.TEST.FLIP_TEST:             # batch of exactly 2: image + mirrored twin
                hm = self._flip_merge(hm, 0)
                wh = self._flip_merge(wh, 0)
                hps = self._flip_merge(hps, 2)
                hm_hp = self._flip_merge(hm_hp, 1) if hm_hp is not None else None
                reg = reg[0:1] if reg is not None else None
                hp_offset = hp_offset[0:1] if hp_offset is not None else None
            dets = multi_pose_decode(hm, wh, hps, reg=reg, hm_hp=hm_hp, hp_offset=hp_offset, K=self.cfg.TEST.TOPK)
        if return_time:
            return outputs, dets, forward_time
        return outputs, dets

    def process_dets(self, images):
        """Detections and nothing else, the way the config says: images as for `process` -> dets (fresh tensor).
        FLIP_TEST on: N = B / 2 image / mirrored-twin pairs (image n at 2n, twin at 2n + 1) through the detections-only flip-test plan
        (model.process(..., flip_dets_only=True)): hm / hm_hp dense and merged as always, wh / hps / reg / hp_offset evaluated and
        merged only at the peaks of the merged heat maps -> [N, K, 56].  FLIP_TEST off: `process(images, dets_only=True)[1]`,
        [B, K, 56].  A head gated off by cfg.LOSS raises ValueError (there is no silent fall-back to a dense plan)."""
        loss = self.cfg.LOSS
        if not (loss.REG_OFFSET and loss.HM_HP and loss.REG_HP_OFFSET and not loss.MSE_LOSS):
            raise ValueError("process_dets needs every head enabled by cfg.LOSS (REG_OFFSET, HM_HP, REG_HP_OFFSET, no MSE_LOSS)")
        if not hasattr(self.model, "process"):
            raise ValueError("process_dets needs a model with the one-replay process()")
        extra = {"dets_only": True}
        if self.cfg.TEST.FLIP_TEST:
            B = images.shape[0]
            if B < 2 or B % 2:
                raise ValueError("FLIP_TEST needs image / mirrored-twin pairs: an even batch [img0, twin0, img1, twin1, ...], got %d" % B)
            extra = {"flip_dets_only": True}
        with torch.no_grad():
            return self.model.process(images, self.cfg.TEST.TOPK, **extra)[1]

    def post_process(self, dets, meta, scale=1):
        """multi_pose.py:62-71 (batch-1 by construction, like the reference): feature-map pixels -> image pixels / scale,
        {1: float32 [N,56]}.  The per-point Python loop of utils/image.py:19-24 is one HIP kernel."""
        if self.num_classes != 1 or dets.shape[2] != 56:
            raise _lib.CenterposeHipError("multi_pose post_process handles one class and 17 joints (dets [..,56])")
        flat = dets.detach().reshape(1, -1, 56).contiguous()
        inv = get_affine_transform(meta["c"], meta["s"], 0, (meta["out_width"], meta["out_height"]), inv=1)
        inv_d = torch.from_numpy(np.ascontiguousarray(inv, np.float64)).cuda()
        mapped = torch.empty_like(flat)
        rc = _lib.lib().cp_transform_dets_f32(_lib.ptr(flat), _lib.ptr(mapped), _lib.c_void_p(inv_d.data_ptr()), 1, flat.shape[1], 17,
                                              _lib.c_float(float(scale)), _lib.stream())
        _lib.check(rc, "cp_transform_dets_f32")
        return {1: mapped[0].cpu().numpy()}

    def _process_batch(self, images):
        """`process` of a whole group -> dets [N,K,56].  FLIP_TEST with a head gated off by cfg.LOSS: the two-stage path takes exactly
        one image / twin pair, so the pairs go through it one by one."""
        if self.cfg.TEST.FLIP_TEST and not self._flip_replay_path():
            return torch.cat([self.process(images[2 * n:2 * n + 2])[1] for n in range(images.shape[0] // 2)], 0)
        return self.process(images)[1]

    def _launch_post(self, dets, inv_dev, scale):
        if self.num_classes != 1 or dets.dim() != 3 or dets.shape[2] != 56:
            raise _lib.CenterposeHipError("multi_pose post_process handles one class and 17 joints (dets [N,K,56])")
        return post_merge_batch([dets], trans=inv_dev, scales=[float(scale)])[0]

    def post_process_batch(self, dets, metas, scale=1):
        """post_process for N images: dets [N,K,56] on the device, one meta per image -> device float32 [N,K,56], row block n
        bit-identical to post_process(dets[n:n + 1], metas[n], scale)[1].  No download."""
        if dets.dim() != 3 or dets.shape[0] != len(metas):
            raise _lib.CenterposeHipError("post_process_batch needs dets [N,K,56] and N metas")
        inv_dev, = self._upload_table([self._inverse_affines(metas)])
        return self._launch_post(dets, inv_dev.view(torch.float64).view(1, len(metas), 6), scale)

    def merge_outputs_batch(self, detections):
        """merge_outputs for N images: a list with one device [N,K,56] per scale (post_process_batch) -> device [N,S*K,56], the scales
        stacked per image; soft_nms_39(Nt=0.5, method=2) per image ON THE DEVICE when TEST.NMS or several scales (multi_pose.py:73-79).
        All S*K rows come back, as merge_outputs returns them.  Against merge_outputs: every column but the score bit-equal, the score
        within the last float bit per Gaussian decay (the device's double exp).  At most 512 rows per image."""
        detections = list(detections)
        if self.cfg.TEST.NMS or len(self.cfg.TEST.TEST_SCALES) > 1:
            return post_merge_batch(detections, nms=True, Nt=0.5, method=2)[0]
        if len(detections) == 1:
            return detections[0]
        return post_merge_batch(detections)[0]

    def merge_outputs(self, detections):
        """multi_pose.py:73-79: rows of every scale stacked; soft-NMS when configured or when several scales were run."""
        rows = np.ascontiguousarray(np.concatenate([d[1] for d in detections], axis=0), dtype=np.float32)
        if self.cfg.TEST.NMS or len(self.cfg.TEST.TEST_SCALES) > 1:
            soft_nms_39(rows, Nt=0.5, method=2)
        return rows.tolist()


def soft_nms_39(boxes, sigma=0.5, Nt=0.3, threshold=0.001, method=0):
    """lib/external/nms.pyx:172-275 -- in place on a float32 [N,56] host array; returns keep list."""
    assert boxes.dtype == np.float32 and boxes.flags["C_CONTIGUOUS"] and boxes.ndim == 2 and boxes.shape[1] == 56
    n = ctypes.c_int(0)
    keep = np.zeros(boxes.shape[0], np.int32)
    rc = _lib.lib().cp_soft_nms_39(boxes.ctypes.data_as(ctypes.c_void_p), int(boxes.shape[0]), ctypes.c_float(sigma),
                                   ctypes.c_float(Nt), ctypes.c_float(threshold), int(method),
                                   keep.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n))
    _lib.check(rc, "cp_soft_nms_39")
    return keep[: n.value].tolist()


detector_factory = {"multi_pose": MultiPoseDetector}     # lib/detectors/detector_factory.py
