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
# frames.py and draw.py hold what used to be defined here: besides what this module uses, the names callers import from it stay
from .draw import DRAW_LEFT, DRAW_LIMBS, DRAW_MID, DRAW_OVERLAY, DRAW_RIGHT, DRAW_STYLE, DrawStyle, draw_rows, palette_to_yuv        # noqa: F401
from .draw import TRACK_ITEM, TRACK_PALETTE, TrackStyle, draw_track_items                                            # noqa: F401
from .draw import DRAW_HEAT_STYLE, HeatmapStyle, check_heat_maps, draw_heat                                          # noqa: F401
from .draw import FACE_STYLE, FaceStyle, draw_faces                                                                   # noqa: F401
from .frames import (FRAME_DESC, PRE_DESC, SURFACE_COLORS, SURFACE_MATRICES, YUV_COLORS, YUV_FRAME_DESC, YUV_MATRICES, FrameIO,      # noqa: F401
                     _check_layout, byte_range, check_drawable, check_rows, frame_geometry, frame_writable, identity_table, is_yuv, yuv_coef,
                     yuv_frame_geometry, yuv_surface_geometry)
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
        if is_yuv(color) or isinstance(image, torch.Tensor):
            if not is_yuv(color) and image.dim() != 3:
                raise _lib.CenterposeHipError("pre_process takes one 3-D frame tensor, got shape %s (N frames: pre_process_batch)"
                                              % (tuple(image.shape),))
            x, metas = self.pre_process_batch([image], scale, layout, color, matrix)      # (bt601, checked above, unless YUV)
            return x, metas[0]
        FrameIO.host_layout_only(layout, color)
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
    def _model_device(self):
        """The card the model's plans live on, with its index ("cuda" alone means the current device, as everywhere here)."""
        device = torch.device(self.model.device)
        return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())

    @property
    def _io(self):
        """This detector's FrameIO, made on first use; it asks `_model_device` per call.  A `_staging_buffers` dict set before stands in."""
        if "_frame_io" not in self.__dict__:
            self._frame_io = FrameIO(lambda: self._model_device(), self.__dict__.get("_staging_buffers"))
        return self._frame_io

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
        images' staging `offsets`, or, with `frames` (a frames.Frame per image), FRAME_DESC rows that address the frames where they lie
        (`yuv`: a frames.YuvFrame per image, YUV_FRAME_DESC rows): the identity table of these frames with the geometry filled in."""
        nb = 2 if self.cfg.TEST.FLIP_TEST else 1
        down = self.cfg.MODEL.DOWN_RATIO
        table = np.zeros(len(idx), PRE_DESC) if frames is None else identity_table([frames[i] for i in idx], yuv)
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
        name = "cp_preprocess_frames_u8_f32" if coef is None else "cp_preprocess_yuv_frames_u8_f32"      # the same arguments but for `coef`
        tables = (ctypes.c_void_p(table_dev.data_ptr()), table.ctypes.data_as(ctypes.c_void_p), n)
        rc = getattr(_lib.lib(), name)(
            *tables, *(() if coef is None else ((ctypes.c_int * 6)(*coef),)), ctypes.c_void_p(scratch.data_ptr()),
            ctypes.c_size_t(scratch_bytes), _lib.ptr(x), nb * n, inp_h, inp_w, mean.ctypes.data_as(ctypes.c_void_p),
            std.ctypes.data_as(ctypes.c_void_p), 1 if nb == 2 else 0, _lib.stream())
        _lib.check(rc, name)
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
        stream-order and lifetime rules above hold for every plane.  Host YUV arrays are not taken.
        Further YUV colours (frames.yuv_surface_geometry has the forms): "p010" / "p016" (uint16 or int16 planes or one surface, the
        samples as stored, MSB aligned), "i422", "i444", "i400" (grey), packed "yuyv" / "uyvy"; further matrices for every YUV colour:
        "bt601-full", "bt709-full" (JPEG / MJPEG), "bt2020-limited", "bt2020-full" (frames.SURFACE_MATRICES).  Same rules, same
        bit-identity to the converted BGR array (csrc/yuv_source.h); these colours and matrices are read, never drawn on."""
        io = self._io
        images, frames = io.batch_input(images, layout, color, matrix)
        if not images:
            raise _lib.CenterposeHipError("pre_process_batch needs at least one image")
        coef = yuv_coef(matrix) if is_yuv(color) else None
        shapes = [im.shape[0:2] for im in images] if frames is None else [(f.H, f.W) for f in frames]
        offsets, nbytes = self._batch_layout(shapes) if frames is None else (None, 0)
        table, scratch_bytes, inp_h, inp_w, metas = self._pre_table(shapes, offsets, list(range(len(images))), scale, frames, coef is not None)
        staging = io.upload_images(images, offsets, nbytes) if frames is None else None
        table_dev, = io.upload_table([table])
        if frames is not None:
            return self._launch_frames(table_dev, table, scratch_bytes, inp_h, inp_w, coef), metas
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
                  track=None, draw_style=None, face=None, face_style=None):
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
        the converted BGR host arrays; the further YUV colours and matrices of pre_process_batch go the same way, but raise with `draw`.
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
        a synchronisation of its own.  Without embed=, or with len(images) != tracker.streams: ValueError, before anything is launched.
        draw="tracks" (needs track=; ValueError before anything is launched otherwise): after the crops and tracker.update the frames
        are painted with the tracker's result -- draw_results with the call's rows at TEST.VIS_THRESH and row_ids =
        track.row_ids(result, M), so that every matched pose takes its identity colour, then draw_tracks with `tracks` on top, both
        with their default styles.  The return value is exactly what it is without `draw`; the painting adds no synchronisation and
        one table upload per painting call.
        draw_style (a DrawStyle; needs `draw`): what draw=True / draw="tracks" paint the rows with -- score labels, translucent limbs
        (DrawStyle(labels=True, limb_opacity=128)); None is the default style, exactly as before.  The return value does not change.
        face=aligner (a face.FaceAligner; device frames only): what the call returns without `face`, as a tuple, with the aligner's
        FaceResult for the call's own rows appended as its last element -- what aligner.align(images, rows=rows, layout, color, matrix,
        vis_thresh=TEST.VIS_THRESH, pose=<the aligner has its head-pose tables>) gives, once the rows are in input order and before
        anything is painted (the crops see clean frames, as for embed=).  Host arrays, or more frames than the aligner's capacity:
        ValueError, before anything is launched.  Goes with dets_only, return_device, embed, track and draw.
        face_style (a FaceStyle; needs face=): the faces are painted onto the frames with it, as aligner.draw(images, result, layout,
        color, matrix, style=face_style) does, after the other painting; the frames must be writable as for draw=True.  The return value
        does not change."""
        given, io = images, self._io
        if draw_style is not None:
            if not isinstance(draw_style, DrawStyle):
                raise _lib.CenterposeHipError("draw_style is a DrawStyle (got %s)" % type(draw_style).__name__)
            if not draw:
                raise ValueError("draw_style= is what draw=True / draw=\"tracks\" paint with: without `draw` nothing is painted")
        if draw:
            _check_layout(layout, color, matrix)
            check_drawable(color, matrix)
        images, frames = io.batch_input(images, layout, color, matrix)
        coef = yuv_coef(matrix) if is_yuv(color) else None
        if embed is not None:
            if frames is None:
                raise ValueError("embed= takes its crops from frames on the device (CUDA uint8 tensors): host arrays are not read, "
                                 "there is no CPU fallback")
            if not 1 <= len(images) <= embed.capacity:
                raise ValueError("%d frames for an extractor of capacity %d: every frame needs at least one slot" % (len(images), embed.capacity))
            if embed.device != self._model_device():
                raise _lib.CenterposeHipError("the extractor is on %s, the model is on %s" % (embed.device, self._model_device()))
        if face_style is not None:
            if face is None:
                raise ValueError("face_style= is what the faces of face= are painted with: without `face` there are none")
            if not isinstance(face_style, FaceStyle):
                raise ValueError("face_style is a FaceStyle (got %s)" % type(face_style).__name__)
            _check_layout(layout, color, matrix)
            check_drawable(color, matrix)
        if face is not None:
            if frames is None:
                raise ValueError("face= takes its crops from frames on the device (CUDA uint8 tensors): host arrays are not read, "
                                 "there is no CPU fallback")
            if not 1 <= len(images) <= face.capacity:
                raise ValueError("%d frames for an aligner of capacity %d: every frame needs at least one slot" % (len(images), face.capacity))
            if face.device != self._model_device():
                raise _lib.CenterposeHipError("the aligner is on %s, the model is on %s" % (face.device, self._model_device()))
        if track is not None:
            if embed is None:
                raise ValueError("track= needs embed=: the tracker matches the extractor's features")
            if len(images) != track.streams:
                raise ValueError("%d frames for a tracker of %d streams: frame n of a call belongs to stream n" % (len(images), track.streams))
            if track.capacity != embed.capacity:
                raise ValueError("the tracker was built for capacity %d, the extractor has %d" % (track.capacity, embed.capacity))
            if track.device != embed.device:
                raise _lib.CenterposeHipError("the tracker is on %s, the extractor is on %s" % (track.device, embed.device))
        if isinstance(draw, str) and draw != "tracks":
            raise ValueError("draw=%r: False, True or \"tracks\"" % (draw,))
        if draw == "tracks" and track is None:
            raise ValueError("draw=\"tracks\" needs track=: it paints the tracker's identities")
        if face_style is not None:
            if face_style.vertices and not face.has_pose_tables:
                raise ValueError("face_style.vertices needs an aligner built with face_ind=")
            if face_style.pose_box and not face.has_pose_tables:
                raise ValueError("face_style.pose_box needs an aligner built with face_ind= and canonical_vertices=")
            io.check_writable(given, images, color)
        if draw:
            if frames is None and images:
                raise _lib.CenterposeHipError("draw=True paints frames on the device (CUDA uint8 tensors): host arrays are not painted, "
                                              "there is no CPU fallback")
            io.check_writable(given, images, color)
        if not images:
            return torch.empty((0, 0, 56), dtype=torch.float32, device="cuda") if return_device else []
        shapes = [im.shape[0:2] for im in images] if frames is None else [(f.H, f.W) for f in frames]
        offsets, nbytes = self._batch_layout(shapes) if frames is None else (None, 0)
        groups = self._batch_groups(shapes)
        work, parts = [], []
        for idx in groups:
            for scale in self.scales:
                table, scratch_bytes, inp_h, inp_w, metas = self._pre_table(shapes, offsets, idx, scale, frames, coef is not None)
                work.append((table, scratch_bytes, inp_h, inp_w))
                parts += [table, self._inverse_affines(metas)]
        order = [i for idx in groups for i in idx]               # merged row block r belongs to image order[r]
        if (return_device or draw or embed is not None or face is not None) and len(groups) > 1:
            parts.append(np.argsort(np.asarray(order, np.int64)).astype(np.int64))       # rides in the one table upload
        staging = io.upload_images(images, offsets, nbytes) if frames is None else None
        parts = io.upload_table(parts)
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
        if draw or return_device or embed is not None or face is not None:
            ordered = rows if len(groups) == 1 else rows.index_select(0, parts[-1].view(torch.int64))
        if embed is not None:                                    # from the frames as they were given: before anything is painted
            result = embed._embed(frames, ordered.contiguous(), color, matrix, float(self.cfg.TEST.VIS_THRESH))
        faces = None
        if face is not None:                                     # likewise before anything is painted
            faces = face._align(frames, ordered.contiguous(), False, color, matrix, float(self.cfg.TEST.VIS_THRESH), True,
                                face.has_pose_tables)
        tracks = None
        if track is not None:                                    # before anything is painted, like the crops
            tracks = track.update(ordered, result, [(int(w), int(h)) for h, w in shapes])
        if draw == "tracks":
            ordered = ordered.contiguous()
            draw_rows(io, frames, ordered, color, matrix, self.cfg.TEST.VIS_THRESH, draw_style,
                      row_ids=track.row_ids(result, int(ordered.shape[1])))
            draw_track_items(io, frames, tracks, color, matrix, None)
        elif draw:
            draw_rows(io, frames, ordered, color, matrix, self.cfg.TEST.VIS_THRESH, draw_style)
        if face_style is not None:                               # after the other painting
            draw_faces(io, frames, faces, face.face_ind_device, color, matrix, face_style)
        more = () if embed is None else (result,) if track is None else (result, tracks)
        if face is not None:
            more += (faces,)
        if return_device:
            return (ordered,) + more if more else ordered
        rows = rows.cpu().numpy()                                                               # the one download
        results = [None] * len(images)
        for r, i in enumerate(order):
            results[i] = {1: rows[r].tolist()}
        return (results,) + more if more else results

    def draw_results(self, frames, rows, layout="hwc", color="bgr", matrix="bt601", vis_thresh=None, style=None, row_ids=None,
                     id_palette=None):
        """Paint the detections `rows` onto `frames`, in place, on the device, in the current stream -> `frames`.  What is drawn is
        what the reference's show_results draws: per row with score > vis_thresh (default cfg.TEST.VIS_THRESH) the box, the limbs
        whose two joints both score > 0 and the joints that score > 0, opaque, rows in ascending order, box then limbs then joints,
        the last painted wins; the score label on top of the box and translucent limbs are options of the style
        (DrawStyle(labels=True, limb_opacity=128): csrc/draw_overlay_arith.h).  The rule is this project's
        own, integer-only and bit-exact between the device, the host painter cp_draw_rows_frames_host and a NumPy restatement
        (csrc/draw_arith.h).
        frames: as for pre_process_batch -- a list of CUDA uint8 tensors or one 4-D tensor (`layout`, `color`, C = 3 or 4), or with
        color "nv12" / "nv21" / "i420" a list of plane tuples / surface tensors; for those the palette is converted to (Y, U, V) with
        `matrix` (palette_to_yuv), luma is written per pixel and a chroma sample takes the latest-painted colour among its 2x2 pixels.
        The colours of frames.SURFACE_COLORS and the matrices of frames.SURFACE_MATRICES raise before anything is launched.
        Three bytes per covered pixel: a fourth channel, row padding and everything outside a view keep their bytes.
        rows: CUDA float32 [N, M, 56] in image coordinates, as run_batch(..., return_device=True) returns them ([M, 56]: one frame).
        style: a DrawStyle.  The descriptor table is the only upload; nothing is downloaded and nothing synchronises -- the label's
        score is turned into glyphs on the device.
        A frame is WRITTEN here, so beyond the stream-order and lifetime rules of pre_process_batch, which hold unchanged: every tensor
        must be a view in which no two indices address one byte (frame_writable: expanded and overlapping views raise), a plane
        tuple's luma bytes must lie apart from its chroma bytes, the same tensor may not be given twice -- and that the frames of one
        call share no bytes otherwise is the caller's promise.  Host arrays raise: there is no CPU fallback.
        row_ids (CUDA int32 [N, M], e.g. DeepSortTracker.row_ids): a row whose id is >= 0 paints all 36 of its primitives in
        id_palette[id % P] (1..64 (B, G, R) colours, default TRACK_PALETTE); a row with id < 0 keeps the style's palette.  Without
        row_ids the call is what it was, bit for bit."""
        given, io = frames, self._io
        _check_layout(layout, color, matrix)
        check_drawable(color, matrix)
        images, descs = io.batch_input(frames, layout, color, matrix)
        if descs is None and images:
            raise _lib.CenterposeHipError("draw_results paints frames on the device (CUDA uint8 tensors): host arrays are not painted, "
                                          "there is no CPU fallback")
        rows = check_rows(rows, len(images), io.device, "the model is on %s",
                          on_host="rows on %s: they must be on the model's GPU; there is no CPU fallback")
        io.check_writable(given, images, color)
        draw_rows(io, descs or [], rows.detach().contiguous(), color, matrix, self.cfg.TEST.VIS_THRESH if vis_thresh is None else vis_thresh,
                  style, row_ids, id_palette)
        return given

    def draw_tracks(self, frames, tracks, layout="hwc", color="bgr", matrix="bt601", style=None):
        """Paint `tracks` onto `frames`, in place, on the device, in the current stream -> `frames`.  What the reference's draw_bboxes
        draws per track: the box in the track's colour (style.palette[id % P]), a filled bar of that colour at the box's top-left
        corner and the label style.prefix + str(id) on the bar, in this project's own 5 x 7 font (characters 0-9 A-Z space # - . : _,
        lower case folded; a longer label than 16 characters or any other character: ValueError).  Items in the given order, box then
        bar then text, the last painted wins; integer-only and bit-exact between the device, the host painter
        cp_draw_tracks_frames_host and a NumPy restatement (csrc/draw_text_arith.h).
        frames: as for draw_results, with the same rules for writable frames; host arrays raise.  tracks: per frame an int64 [k, 5]
        array (x1, y1, x2, y2, track_id), what DeepSortTracker.update returns -- host data, so the item table is built here and goes
        up with the descriptor table in the call's one upload.  style: a TrackStyle.  One launch, nothing is downloaded."""
        given, io = frames, self._io
        _check_layout(layout, color, matrix)
        check_drawable(color, matrix)
        images, descs = io.batch_input(frames, layout, color, matrix)
        if descs is None and images:
            raise _lib.CenterposeHipError("draw_tracks paints frames on the device (CUDA uint8 tensors): host arrays are not painted, "
                                          "there is no CPU fallback")
        io.check_writable(given, images, color)
        draw_track_items(io, descs or [], list(tracks), color, matrix, style)
        return given

    def draw_heatmaps(self, frames, maps, metas, scale=1, layout="hwc", color="bgr", matrix="bt601", style=None):
        """Blend the heat maps `maps` over `frames`, in place, on the device, in the current stream -> `frames`.  The reference's debug
        views pred_hm / pred_hmhp (MultiPoseDetector.debug): per image the maps become one colour map -- per component the maximum over
        the channels of value x channel colour -- which is sampled bilinearly at the map position of every frame pixel and blended
        over it, p' = (p (256 - a) + f a + 128) >> 8.  The rule is this project's own, bit-exact between the device, the host painter
        cp_draw_heat_frames_host and a NumPy restatement (csrc/draw_heat_arith.h): map cell (i, j) sits at map
        coordinate (i, j), where post_process puts a peak, so a blob lies under the joint draw_results paints for it.
        frames: as for draw_results, with the same rules for writable frames; host arrays raise.  Every pixel is read and written; a
        fourth channel, row padding and everything outside a view keep their bytes.  On color "nv12" / "nv21" / "i420" the colour goes
        to (Y, U, V) with `matrix`, luma per pixel, a chroma sample with the mean colour of its 2x2 pixels.
        maps: CUDA float32 [N, C, h, w] ([C, h, w]: one frame) on the model's device, 1 <= C <= 32, ANY non-negative strides -- never
        copied, so outputs[0], outputs[4][0::2] (the images of a FLIP_TEST batch, not their twins), a channel slice or a permuted view go
        in as they are.  metas: what pre_process_batch / pre_process returned for these frames at `scale`; their out_height / out_width
        are the maps' h / w.  style: a HeatmapStyle.
        The descriptor table is the only upload; nothing is downloaded and nothing synchronises.  Two launches."""
        given, io = frames, self._io
        _check_layout(layout, color, matrix)
        check_drawable(color, matrix)
        images, descs = io.batch_input(frames, layout, color, matrix)
        if descs is None and images:
            raise _lib.CenterposeHipError("draw_heatmaps paints frames on the device (CUDA uint8 tensors): host arrays are not painted, "
                                          "there is no CPU fallback")
        if isinstance(metas, dict):
            metas = [metas]
        maps = check_heat_maps(maps, len(images), io.device)
        io.check_writable(given, images, color)
        draw_heat(io, descs or [], maps, metas, lambda height, width: self.input_geometry(height, width, scale)[0:2], color, matrix, style)
        return given

    def _source(self, x, layout="hwc", color="bgr", matrix="bt601"):
        if isinstance(x, (np.ndarray, torch.Tensor)) or (is_yuv(color) and isinstance(x, (tuple, list))):
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
        inv_dev, = self._io.upload_table([self._inverse_affines(metas)])
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
