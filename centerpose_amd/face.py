"""3-D face alignment for detections: device crops, the PRNet plan and the restore, without the host.

Replaces the hot path behind ``face_3d_model.process`` and ``get_landmarks`` of the reference's video demo (demo/face/prnet.py:61-127):
per face a similarity crop to 256 x 256 with skimage on the host, an upload, ``PRNet(3, 3)`` (demo/face/resfcn256.py), a download of
the 256 x 256 x 3 position map and its restore to image coordinates in NumPy -- one face at a time.  Here the faces of N frames are cut
out of the frames where they lie on the device (csrc/face_stage.hip), written straight into the input tensor of ONE
``Engine("prnet", ...)`` plan, regressed in one graph replay and restored on the device.  The batch is static (`capacity` crops): a
data-dependent batch would need the number of selected faces on the host, i.e. a synchronisation.

The crop is a closed-form statement of the reference's pipeline (csrc/face_arith.h): skimage is not available to this project, so it is
not pinned to a recording of estimate_transform / warp.
"""
import ctypes

import numpy as np
import torch

from . import _lib, nets
from .engine import Engine
from .frames import FrameIO, check_rows, identity_table, is_yuv, yuv_coef
from .reid import _holds_host_array

# cp_face_rule (include/centerpose_hip.h)
FACE_RULE = np.dtype([("vis_thresh", "<f4"), ("expand", "<f4"), ("min_size", "<i4"), ("boxes", "<i4")])
RES, NKPT, MAX_CAPACITY, MAX_SIZE = 256, 68, 256, 32768


def load_prnet_state_dict(path):
    """The reference's checkpoint format (demo/face/prnet.py:27-28: the bare state dict), tensors only: nothing else is unpickled."""
    return torch.load(path, map_location="cpu", weights_only=True)


def load_uv_kpt_ind(path):
    """The reference's landmark table (utils/uv_data/uv_kpt_ind.txt, prnet.py:34): two rows of 68 numbers -> int32 [2, 68]."""
    return check_uv_kpt_ind(np.loadtxt(path))


def check_uv_kpt_ind(uv):
    """-> int32 [2, 68] with every entry in 0..255 (row 0: the column of a landmark's cell, row 1: its row), or ValueError."""
    a = np.asarray(uv)
    if a.shape != (2, NKPT):
        raise ValueError("uv_kpt_ind must be [2, %d] (got shape %s)" % (NKPT, tuple(a.shape)))
    if a.dtype.kind not in "iuf" or not np.isfinite(a.astype(np.float64)).all() or (a != np.floor(a)).any():
        raise ValueError("uv_kpt_ind must hold whole numbers")
    if (a < 0).any() or (a >= RES).any():
        raise ValueError("uv_kpt_ind entries must lie in 0..%d" % (RES - 1))
    return np.ascontiguousarray(a.astype(np.int32))


class FaceResult:
    """What one `align` call returns, all on the device, ready in the current stream's order:
    pos [capacity, 256, 256, 3] float32 or None (positions=False) -- slot s holds the position map of candidate `slots[s]` in image
    coordinates (x, y, z); zeros for an unused slot;
    landmarks [capacity, 68, 3] float32 -- its 68 landmarks (get_landmarks); zeros for an unused slot;
    slots [capacity] int32 -- n * M + m of the candidate in slot s, -1 for an unused slot; with q = capacity // N the first q selected
    candidates of frame n, in order, sit in slots n * q + 0, 1, ...;
    counts [N] int32 -- the selected candidates of every frame, NOT capped at q;
    xform [capacity, 3] float32 -- (x0, y0, size) of every slot's crop square: frame x = x0 + u * size / 255."""
    __slots__ = ("pos", "landmarks", "slots", "counts", "xform")

    def __init__(self, pos, landmarks, slots, counts, xform):
        self.pos, self.landmarks, self.slots, self.counts, self.xform = pos, landmarks, slots, counts, xform

    def vertices(self, face_ind):
        """-> [capacity, len(face_ind), 3]: the map's cells `face_ind` (indices into the flattened 256 x 256 map; get_vertices,
        prnet.py:130-140).  Plain torch indexing, not a hot path."""
        if self.pos is None:
            raise ValueError("this result was made with positions=False: it holds the landmarks only")
        idx = torch.as_tensor(np.asarray(face_ind), dtype=torch.long, device=self.pos.device)
        return self.pos.reshape(self.pos.shape[0], RES * RES, 3)[:, idx]


class FaceAligner:
    """One compiled PRNet plan of `capacity` crops with the crop stage that feeds it and the restore behind it.

    state_dict: the reference module's own keys (`input_conv.1.weight`, `down_conv_1.main.0.weight`, ...; `load_prnet_state_dict`).
    uv_kpt_ind: [2, 68] integers in 0..255 or the path of the reference's text file; the product ships no reference data.
    expand / min_size: the crop square has side int(old_size * expand) and is taken iff that is in min_size..32768."""

    def __init__(self, state_dict, uv_kpt_ind, capacity=8, device="cuda", expand=1.6, min_size=1):
        capacity = int(capacity)
        if not 1 <= capacity <= MAX_CAPACITY:
            raise ValueError("capacity must lie in 1..%d (got %d)" % (MAX_CAPACITY, capacity))
        # the launchers' 32-bit checks (conv2d: B * H * W * ld * 4 bytes of a source below 2^32; the widest map is 256 x 256 x 16)
        if capacity * RES * RES * 16 * 4 >= 1 << 32:
            raise ValueError("capacity %d: the plan's %d x %d x 16 maps exceed the launchers' 32-bit byte offsets" % (capacity, RES, RES))
        if not (isinstance(min_size, (int, np.integer)) and 1 <= int(min_size) <= MAX_SIZE):
            raise ValueError("min_size must be an integer in 1..%d (got %r)" % (MAX_SIZE, min_size))
        if not 0.0 < float(expand) <= 1024.0:
            raise ValueError("expand must lie in (0, 1024] (got %r)" % (expand,))
        uv = load_uv_kpt_ind(uv_kpt_ind) if isinstance(uv_kpt_ind, (str, bytes)) or hasattr(uv_kpt_ind, "__fspath__") else check_uv_kpt_ind(uv_kpt_ind)
        self.capacity, self.expand, self.min_size = capacity, float(expand), int(min_size)
        self.uv_kpt_ind = uv
        self.engine = Engine("prnet", state_dict, capacity, nets.PRNET_INPUT[0], nets.PRNET_INPUT[1], device=device)
        self.device = self.engine.device if self.engine.device.index is not None else torch.device("cuda", torch.cuda.current_device())
        self._io = FrameIO(self.device)
        with torch.cuda.device(self.device):
            self._uv = torch.from_numpy(uv).to(self.device)
            self.engine.capture()      # the one-off capture synchronises: here, not in the first align

    def align(self, frames, rows=None, boxes=None, layout="hwc", color="bgr", matrix="bt601", vis_thresh=0.3, positions=True):
        """Position maps and landmarks of the faces of `frames` -> FaceResult, on the device, in the current stream, no
        synchronisation; the descriptor table is the only upload.
        frames: as for ReidExtractor.embed -- a list of CUDA uint8 tensors or one 4-D tensor (`layout`, `color`, C = 3 or 4), or with a
        YUV color a list of plane tuples / surface tensors (`matrix`).  They are only read.  Host arrays raise ValueError.
        Exactly one of rows / boxes: rows CUDA float32 [N, M, 56] as run_batch(..., return_device=True) returns them (the face box is
        the extent of the five face joints), or boxes CUDA float32 [N, F, 5] = (x1, y1, x2, y2, score) (PRN.process(frame, box) on the
        whole frame).  A candidate gets a face iff its score is > vis_thresh and its square is valid (csrc/face_arith.h).
        positions=False: the 68 landmarks only; the maps are never written."""
        if (rows is None) == (boxes is None):
            raise ValueError("align takes exactly one of rows= and boxes=")
        if _holds_host_array(frames):
            raise ValueError("align takes its crops from device frames (CUDA uint8 tensors): host arrays are not read, there is no "
                             "CPU fallback")
        images, descs = self._io.batch_input(frames, layout, color, matrix)
        if rows is not None:
            cand = check_rows(rows, len(images), self.device, "the face plan is on %s; there is no CPU fallback")
        else:
            cand = self._check_boxes(boxes, len(images))
        return self._align(descs or [], cand.detach().contiguous(), boxes is not None, color, matrix, vis_thresh, positions)

    def _check_boxes(self, boxes, n_frames):
        if not isinstance(boxes, torch.Tensor):
            raise _lib.CenterposeHipError("boxes must be a CUDA float32 tensor [N, F, 5] on the device (got %s): there is no CPU fallback"
                                          % type(boxes).__name__)
        boxes = boxes.unsqueeze(0) if boxes.dim() == 2 else boxes
        if boxes.dim() != 3 or boxes.shape[2] != 5:
            raise _lib.CenterposeHipError("boxes must be [N, F, 5] (or [F, 5] for one frame), got shape %s" % (tuple(boxes.shape),))
        if not boxes.is_cuda or boxes.device != self.device:
            raise _lib.CenterposeHipError("boxes on %s, the face plan is on %s; there is no CPU fallback" % (boxes.device, self.device))
        if boxes.dtype != torch.float32:
            raise _lib.CenterposeHipError("boxes must be float32 (got %s)" % boxes.dtype)
        if boxes.shape[0] != n_frames:
            raise _lib.CenterposeHipError("boxes hold %d blocks for %d frames" % (boxes.shape[0], n_frames))
        return boxes

    def _align(self, descs, cand, boxes, color, matrix, vis_thresh, positions):
        """select + crop + one replay + restore for checked frames and device candidates [N, M, 56 | 5]."""
        yuv = is_yuv(color)
        N, M, cap = len(descs), int(cand.shape[1]), self.capacity
        if N < 1:
            raise ValueError("align needs at least one frame")
        if N > cap:
            raise ValueError("%d frames for a capacity of %d crops: every frame needs at least one slot (build the FaceAligner with a "
                             "larger capacity)" % (N, cap))
        if N * M > 1 << 24:
            raise ValueError("%d x %d candidates are too many for one call (at most 2^24)" % (N, M))
        table = identity_table(descs, yuv)
        rule = np.zeros(1, FACE_RULE)
        rule["vis_thresh"], rule["expand"], rule["min_size"], rule["boxes"] = vis_thresh, self.expand, self.min_size, int(boxes)
        L = _lib.lib()
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            slots = torch.empty((cap,), dtype=torch.int32, device=self.device)
            counts = torch.empty((N,), dtype=torch.int32, device=self.device)
            xform = torch.empty((cap, 3), dtype=torch.float32, device=self.device)
            landmarks = torch.empty((cap, NKPT, 3), dtype=torch.float32, device=self.device)
            pos = torch.empty((cap, RES, RES, 3), dtype=torch.float32, device=self.device) if positions else None
            table_dev, = self._io.upload_table([table])
            th = table.ctypes.data_as(vp)
            _lib.check(L.cp_face_select(N, vp(cand.data_ptr()), M, rule.ctypes.data_as(vp), cap, vp(slots.data_ptr()), vp(counts.data_ptr()),
                                        vp(xform.data_ptr()), _lib.stream()), "cp_face_select")
            x = self.engine.input
            if yuv:
                coef = (ctypes.c_int * 6)(*yuv_coef(matrix))
                _lib.check(L.cp_face_crop_yuv_frames_f32(vp(table_dev.data_ptr()), th, N, coef, M, vp(slots.data_ptr()), vp(xform.data_ptr()), cap,
                                                         vp(x.data_ptr()), _lib.stream()), "cp_face_crop_yuv_frames_f32")
            else:
                _lib.check(L.cp_face_crop_frames_f32(vp(table_dev.data_ptr()), th, N, M, vp(slots.data_ptr()), vp(xform.data_ptr()), cap,
                                                     vp(x.data_ptr()), _lib.stream()), "cp_face_crop_frames_f32")
            net = self.engine.forward(x)[0]                  # the plan's output buffer: read by the restore below, in stream order
            _lib.check(L.cp_face_restore_f32(vp(net.data_ptr()), vp(slots.data_ptr()), vp(xform.data_ptr()), cap, vp(self._uv.data_ptr()),
                                             vp(pos.data_ptr()) if positions else None, vp(landmarks.data_ptr()), _lib.stream()),
                       "cp_face_restore_f32")
        return FaceResult(pos, landmarks, slots, counts, xform)
