"""Re-id embeddings for detections: device crops and the DeepSort net, without the host.

Replaces the hot path behind ``DeepSort.update`` of the reference's video demo (demo/tracking/deep_sort.py:24-45): per box
``_xywh_to_xyxy_centernet`` (:66-72), a host slice + ``cv2.resize`` to 64 x 128 + ``Normalize`` (feature_extractor.py:15-33), an
upload, ``Net(reid=True)`` (model.py:49-93) and a download of the 512-vector -- one box at a time.  Here the boxes of N frames are cut
out of the frames where they lie on the device (csrc/reid_crops.hip, two launches), written straight into the input tensor of ONE
``Engine("reid", ...)`` plan and embedded in one graph replay.  The batch is static (`capacity` crops): a data-dependent batch would
need the number of selected rows on the host, i.e. a synchronisation.  The tracker that consumes the features is track.DeepSortTracker:
its gallery and cost matrix stay on the device with them, its sequential logic (Kalman filter, matching) runs on the host.
"""
import ctypes

import numpy as np
import torch

from . import _lib, nets
from .engine import Engine
from .frames import FrameIO, check_rows, identity_table, is_yuv, yuv_coef

# cp_reid_norm (include/centerpose_hip.h)
REID_NORM = np.dtype([("scale", "<f4"), ("mean", "<f4", (3,)), ("std", "<f4", (3,)), ("rgb", "<i4")])
# Extractor.__init__ (feature_extractor.py:15-18): ImageNet statistics in R, G, B order -- which the reference pairs with the B, G, R
# channels of a cv2 image, on a 0..255 scale (its `/ 255.` is commented out, :21).  The defaults below reproduce exactly that.
REID_MEAN, REID_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CHANNEL_ORDERS = ("bgr", "rgb")


def load_reid_state_dict(path):
    """The reference's checkpoint format (feature_extractor.py:11: torch.load(path)['net_dict']), tensors only: nothing else is
    unpickled."""
    return torch.load(path, map_location="cpu", weights_only=True)["net_dict"]


def _holds_host_array(frames):
    if isinstance(frames, np.ndarray):
        return True
    if isinstance(frames, (list, tuple)):
        return any(_holds_host_array(f) for f in frames)
    return False


class ReidResult:
    """What one `embed` call returns, all on the device, ready in the current stream's order:
    features [capacity, 512] float32 -- slot s holds the unit-norm embedding of row `slots[s]` (rows of unused slots are meaningless);
    slots [capacity] int32 -- n * M + m of the row embedded in slot s, -1 for an unused slot; with q = capacity // N the first q
    selected rows of frame n, in row order, sit in slots n * q + 0, 1, ...;
    counts [N] int32 -- the selected rows of every frame, NOT capped at q: counts[n] > q says that frame n had more than fit."""
    __slots__ = ("features", "slots", "counts")

    def __init__(self, features, slots, counts):
        self.features, self.slots, self.counts = features, slots, counts

    def dense(self, N, M):
        """-> (features [N, M, 512], zero where a row was not embedded; valid [N, M] bool).  Plain torch indexing, not a hot path."""
        dim = self.features.shape[1]
        idx = torch.where(self.slots >= 0, self.slots, torch.full_like(self.slots, N * M)).long()       # unused slots -> a spare row
        feats = torch.zeros((N * M + 1, dim), dtype=self.features.dtype, device=self.features.device)
        feats.index_copy_(0, idx, self.features)
        valid = torch.zeros((N * M + 1,), dtype=torch.bool, device=self.features.device)
        valid[idx] = True
        return feats[:-1].view(N, M, dim), valid[:-1].view(N, M)


class ReidExtractor:
    """One compiled re-id plan of `capacity` crops and the crop stage that feeds it.

    state_dict: the reference module's own keys (`conv.0.weight`, `layer2.0.downsample.1.running_var`, ...; `load_reid_state_dict`);
    `classifier.*` is ignored.  scale / mean / std / channel_order: output channel k of a crop is (v * scale - mean[k]) / std[k] with
    v the frame's B, G, R (channel_order "bgr") or R, G, B ("rgb") value; the defaults are the reference's, quirks included."""

    def __init__(self, state_dict, capacity=32, device="cuda", scale=1.0, mean=REID_MEAN, std=REID_STD, channel_order="bgr"):
        capacity = int(capacity)
        if not 1 <= capacity <= 4096:
            raise ValueError("capacity must lie in 1..4096 (got %d)" % capacity)
        if channel_order not in CHANNEL_ORDERS:
            raise ValueError("unknown channel_order %r: one of %s" % (channel_order, ", ".join(CHANNEL_ORDERS)))
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("mean and std have three entries each")
        self.capacity = capacity
        self.engine = Engine("reid", state_dict, capacity, nets.REID_INPUT[0], nets.REID_INPUT[1], device=device)
        self.device = self.engine.device if self.engine.device.index is not None else torch.device("cuda", torch.cuda.current_device())
        self.norm = np.zeros(1, REID_NORM)
        self.norm["scale"], self.norm["mean"], self.norm["std"], self.norm["rgb"] = scale, mean, std, CHANNEL_ORDERS.index(channel_order)
        self._io = FrameIO(self.device)
        with torch.cuda.device(self.device):
            self.engine.capture()      # the one-off capture synchronises: here, not in the first embed

    def embed(self, frames, rows, layout="hwc", color="bgr", matrix="bt601", vis_thresh=0.3):
        """Embeddings of the detections `rows` of `frames` -> ReidResult, on the device, in the current stream, no synchronisation;
        the descriptor table is the only upload.
        frames: as for draw_results -- a list of CUDA uint8 tensors or one 4-D tensor (`layout`, `color`, C = 3 or 4), or with color
        "nv12" / "nv21" / "i420" a list of plane tuples / surface tensors (`matrix`); the further YUV colours and matrices of
        pre_process_batch ("p010", "i422", "i444", "i400", "yuyv", ...; "bt601-full", ...) are taken too.  They are only read: expanded
        and overlapping views are fine.  Host arrays raise ValueError: the crops are taken from device frames, there is no CPU fallback.
        rows: CUDA float32 [N, M, 56] in image coordinates, as run_batch(..., return_device=True) returns them ([M, 56]: one frame).
        A row is embedded iff its score is > vis_thresh and its clamped box has pixels (csrc/reid_arith.h); N > capacity raises."""
        if _holds_host_array(frames):
            raise ValueError("embed takes its crops from device frames (CUDA uint8 tensors): host arrays are not read, there is no "
                             "CPU fallback")
        images, descs = self._io.batch_input(frames, layout, color, matrix)
        rows = check_rows(rows, len(images), self.device, "the re-id plan is on %s; there is no CPU fallback")
        return self._embed(descs or [], rows.detach().contiguous(), color, matrix, vis_thresh)

    def _embed(self, descs, rows, color, matrix, vis_thresh):
        """select + crop + one replay for checked frames (a frames.Frame / YuvFrame / YuvSurface per frame) and device rows [N, M, 56]."""
        yuv = is_yuv(color)
        N, M, cap = len(descs), int(rows.shape[1]), self.capacity
        if N < 1:
            raise ValueError("embed needs at least one frame")
        if N > cap:
            raise ValueError("%d frames for a capacity of %d crops: every frame needs at least one slot (build the ReidExtractor with "
                             "a larger capacity)" % (N, cap))
        if N * M > 1 << 24:
            raise ValueError("%d x %d rows are too many for one call (at most 2^24)" % (N, M))
        table = identity_table(descs, yuv)
        L = _lib.lib()
        vp = ctypes.c_void_p
        with torch.cuda.device(self.device):
            slots = torch.empty((cap,), dtype=torch.int32, device=self.device)
            counts = torch.empty((N,), dtype=torch.int32, device=self.device)
            table_dev, = self._io.upload_table([table])
            th, thr = table.ctypes.data_as(vp), ctypes.c_float(float(vis_thresh))
            _lib.check(L.cp_reid_select_rows(vp(table_dev.data_ptr()), th, int(yuv), N, vp(rows.data_ptr()), M, thr, cap,
                                             vp(slots.data_ptr()), vp(counts.data_ptr()), _lib.stream()), "cp_reid_select_rows")
            x = self.engine.input
            norm = self.norm.ctypes.data_as(vp)
            if yuv:
                coef = (ctypes.c_int * 6)(*yuv_coef(matrix))
                _lib.check(L.cp_reid_crop_yuv_frames_f32(vp(table_dev.data_ptr()), th, N, coef, vp(rows.data_ptr()), M, thr,
                                                         vp(slots.data_ptr()), cap, norm, vp(x.data_ptr()), _lib.stream()),
                           "cp_reid_crop_yuv_frames_f32")
            else:
                _lib.check(L.cp_reid_crop_frames_f32(vp(table_dev.data_ptr()), th, N, vp(rows.data_ptr()), M, thr, vp(slots.data_ptr()),
                                                     cap, norm, vp(x.data_ptr()), _lib.stream()), "cp_reid_crop_frames_f32")
            features = self.engine.forward(x)[0].clone()     # the plan's output buffer is overwritten by the next call
        return ReidResult(features, slots, counts)
