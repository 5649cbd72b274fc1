"""3-D face alignment for detections: device crops, the PRNet plan and the restore, without the host.

Replaces the hot path behind ``face_3d_model.process`` and ``get_landmarks`` of the reference's video demo (demo/face/prnet.py:61-127):
per face a similarity crop to 256 x 256 with skimage on the host, an upload, ``PRNet(3, 3)`` (demo/face/resfcn256.py), a download of
the 256 x 256 x 3 position map and its restore to image coordinates in NumPy -- one face at a time.  Here the faces of N frames are cut
out of the frames where they lie on the device (csrc/face_stage.hip), written straight into the input tensor of ONE
``Engine("prnet", ...)`` plan, regressed in one graph replay and restored on the device.  The batch is static (`capacity` crops): a
data-dependent batch would need the number of selected faces on the host, i.e. a synchronisation.

`FaceRenderer` renders the restored maps where they lie (csrc/face_render.hip): the depth image, the per-pixel triangle index and the
flat-shaded face of demo/face/utils/render.py, and the vertex colours of PRN.get_colors; it needs the two mesh tables only, no plan.

The crop is a closed-form statement of the reference's pipeline (csrc/face_arith.h): skimage is not available to this project, so it is
not pinned to a recording of estimate_transform / warp.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib, nets
from .engine import Engine
from .draw import FaceStyle, draw_faces
from .frames import FrameIO, _check_layout, check_drawable, check_rows, identity_table, is_yuv, yuv_coef
from .reid import _holds_host_array

# cp_face_rule (include/centerpose_hip.h)
FACE_RULE = np.dtype([("vis_thresh", "<f4"), ("expand", "<f4"), ("min_size", "<i4"), ("boxes", "<i4")])
RES, NKPT, MAX_CAPACITY, MAX_SIZE = 256, 68, 256, 32768
MIN_VERTICES, MAX_VERTICES = 3, 65536
MAX_TRIANGLES, MAX_WINDOW, MAX_ORIGIN, MAX_ATTRS = 1 << 22, 4096, 1 << 20, 4


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


def _is_path(x):
    return isinstance(x, (str, bytes)) or hasattr(x, "__fspath__")


def _load_table(x):
    """An array, or the reference's file of one: text (face_ind.txt) or .npy (canonical_vertices.npy)."""
    if not _is_path(x):
        return np.asarray(x)
    name = os.fsdecode(x)
    return np.load(name, allow_pickle=False) if name.endswith(".npy") else np.loadtxt(name)


def check_face_ind(face_ind):
    """get_vertices' table (prnet.py:130-140), an array or the path of the reference's text file -> int32 [V]: whole numbers in
    0..65535, 3 <= V <= 65536, or ValueError."""
    ind = _load_table(face_ind)
    if ind.ndim != 1 or not MIN_VERTICES <= ind.shape[0] <= MAX_VERTICES:
        raise ValueError("face_ind must be one row of %d..%d cells (got shape %s)" % (MIN_VERTICES, MAX_VERTICES, tuple(ind.shape)))
    if ind.dtype.kind not in "iuf" or not np.isfinite(ind.astype(np.float64)).all() or (ind != np.floor(ind)).any():
        raise ValueError("face_ind must hold whole numbers")
    if (ind < 0).any() or (ind >= RES * RES).any():
        raise ValueError("face_ind entries must lie in 0..%d" % (RES * RES - 1))
    return np.ascontiguousarray(ind.astype(np.int32))


def check_pose_tables(face_ind, canonical_vertices):
    """The two tables of estimate_pose (get_vertices' face_ind, prnet.py:130-140; canonical_vertices, estimate_pose.py:94), arrays or the
    paths of the reference's files -> (face_ind int32 [V], the canonical cloud centred in float64 [V, 3], float64 [4]: its mean and
    rms_d1, estimate_pose.py:73,86), or ValueError.  face_ind: V whole numbers in 0..65535 (cells of the flattened 256 x 256 map),
    3 <= V <= 65536, duplicates and any order allowed; canonical_vertices: finite [V, 3]."""
    ind, can = check_face_ind(face_ind), _load_table(canonical_vertices)
    if can.dtype.kind not in "iuf" or can.ndim != 2 or can.shape[1] != 3:
        raise ValueError("canonical_vertices must be numbers [V, 3] (got shape %s)" % (tuple(can.shape),))
    if can.shape[0] != ind.shape[0]:
        raise ValueError("canonical_vertices holds %d vertices for %d entries of face_ind" % (can.shape[0], ind.shape[0]))
    can = can.astype(np.float64)
    if not np.isfinite(can).all():
        raise ValueError("canonical_vertices must be finite")
    mean = can.mean(axis=0)
    centred = np.ascontiguousarray(can - mean)
    rms_d1 = float(np.sqrt(np.mean(np.sum(centred * centred, axis=1))))
    if not (np.isfinite(rms_d1) and rms_d1 > 0.0):
        raise ValueError("canonical_vertices must not be one point (rms distance from the mean %r)" % rms_d1)
    return ind, centred, np.asarray([mean[0], mean[1], mean[2], rms_d1], np.float64)


def check_triangles(triangles, V):
    """A mesh over V vertices, an array [T, 3] or the path of a text file of one (the reference's triangles.txt) -> int32 [T, 3]: whole
    numbers in 0..V-1, 1 <= T <= 2^22, or ValueError.  The kernels do not check the table again."""
    tri = _load_table(triangles)
    if tri.ndim != 2 or tri.shape[1] != 3 or not 1 <= tri.shape[0] <= MAX_TRIANGLES:
        raise ValueError("triangles must be [T, 3] with T in 1..%d (got shape %s)" % (MAX_TRIANGLES, tuple(tri.shape)))
    if tri.dtype.kind not in "iuf" or not np.isfinite(tri.astype(np.float64)).all() or (tri != np.floor(tri)).any():
        raise ValueError("triangles must hold whole numbers")
    if (tri < 0).any() or (tri >= V).any():
        raise ValueError("triangles must name vertices 0..%d" % (V - 1))
    return np.ascontiguousarray(tri.astype(np.int32))


def grid_triangles(face_ind):
    """A mesh for a caller without the reference's triangles.txt -> int32 [T, 3]: the two triangles (tl, bl, tr) and (bl, br, tr) of
    every 2 x 2 block of map cells whose four corners are in `face_ind`, blocks in row-major order, as indices into face_ind (the first
    entry of a cell that is listed twice).  ValueError when no block is complete."""
    ind = check_face_ind(face_ind)
    where = np.full(RES * RES, -1, np.int64)
    where[ind[::-1]] = np.arange(len(ind) - 1, -1, -1)
    grid = where.reshape(RES, RES)
    tl, bl, tr, br = grid[:-1, :-1], grid[1:, :-1], grid[:-1, 1:], grid[1:, 1:]
    full = (tl >= 0) & (bl >= 0) & (tr >= 0) & (br >= 0)
    if not full.any():
        raise ValueError("face_ind holds no 2 x 2 block of map cells: no triangle")
    tl, bl, tr, br = tl[full], bl[full], tr[full], br[full]
    return np.ascontiguousarray(np.stack([np.stack([tl, bl, tr], 1), np.stack([bl, br, tr], 1)], 1).reshape(-1, 3).astype(np.int32))


class FacePose:
    """The head pose of every slot (estimate_pose, demo/face/utils/estimate_pose.py:93-99; csrc/face_pose_arith.h), all on the device:
    P [capacity, 3, 4] float64 -- the affine camera matrix [s R | t] that takes the canonical cloud onto the slot's vertices;
    angles [capacity, 3] float64 -- matrix2angle's (x, y, z), which the reference calls yaw, pitch, roll;
    scale [capacity] float64 -- s;
    box [capacity, 10, 2] int32 -- the ten projected corners of plot_pose_box (cv_plot.py:48-70);
    valid [capacity] int32 -- 1 iff the slot is used, every vertex and moment is finite and the vertices are not one point.
    Unused slots and slots with valid == 0 are all zeros."""
    __slots__ = ("P", "angles", "scale", "box", "valid")

    def __init__(self, P, angles, scale, box, valid):
        self.P, self.angles, self.scale, self.box, self.valid = P, angles, scale, box, valid


class FaceResult:
    """What one `align` call returns, all on the device, ready in the current stream's order:
    pos [capacity, 256, 256, 3] float32 or None (positions=False) -- slot s holds the position map of candidate `slots[s]` in image
    coordinates (x, y, z); zeros for an unused slot;
    landmarks [capacity, 68, 3] float32 -- its 68 landmarks (get_landmarks); zeros for an unused slot;
    slots [capacity] int32 -- n * M + m of the candidate in slot s, -1 for an unused slot; with q = capacity // N the first q selected
    candidates of frame n, in order, sit in slots n * q + 0, 1, ...;
    counts [N] int32 -- the selected candidates of every frame, NOT capped at q;
    xform [capacity, 3] float32 -- (x0, y0, size) of every slot's crop square: frame x = x0 + u * size / 255;
    pose -- a FacePose (align(..., pose=True)) or None."""
    __slots__ = ("pos", "landmarks", "slots", "counts", "xform", "pose")

    def __init__(self, pos, landmarks, slots, counts, xform, pose=None):
        self.pos, self.landmarks, self.slots, self.counts, self.xform, self.pose = pos, landmarks, slots, counts, xform, pose

    def vertices(self, face_ind):
        """-> [capacity, len(face_ind), 3]: the map's cells `face_ind` (indices into the flattened 256 x 256 map; get_vertices,
        prnet.py:130-140).  Plain torch indexing, not a hot path."""
        if self.pos is None:
            raise ValueError("this result was made with positions=False: it holds the landmarks only")
        idx = torch.as_tensor(np.asarray(face_ind), dtype=torch.long, device=self.pos.device)
        return self.pos.reshape(self.pos.shape[0], RES * RES, 3)[:, idx]


class FaceRender:
    """What one `render` call returns, on the device, ready in the current stream's order:
    tri [capacity, h, w] int32 -- the index of the triangle seen at every pixel of the slot's window, -1 for none (get_triangle_buffer);
    image [capacity, h, w, C] float32 -- the mean of that triangle's three vertex attributes, 0 where nothing covers (render_texture;
    with attrs=None the depth image of get_depth_image, C = 1).  Unused slots are all -1 / 0."""
    __slots__ = ("tri", "image")

    def __init__(self, tri, image):
        self.tri, self.image = tri, image


class FaceRenderer:
    """The z-buffer rasteriser over the position maps of `capacity` slots and their vertex colours (csrc/face_render.hip; DESIGN.md
    section 4.17).  It needs no PRNet plan: only the two tables.
    face_ind: get_vertices' table (`check_face_ind`); triangles: [T, 3] whole numbers in 0..V-1 or the path of a text file of them
    (`check_triangles`; `grid_triangles(face_ind)` makes a mesh).  The product ships no reference data."""

    def __init__(self, face_ind, triangles, capacity, device="cuda"):
        capacity = int(capacity)
        if not 1 <= capacity <= MAX_CAPACITY:
            raise ValueError("capacity must lie in 1..%d (got %d)" % (MAX_CAPACITY, capacity))
        ind = check_face_ind(face_ind)
        tri = check_triangles(triangles, len(ind))
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("the renderer runs on the GPU (got device %s): there is no CPU fallback" % device)
        self.device = device if device.index is not None else torch.device("cuda", torch.cuda.current_device())
        self.capacity, self.face_ind, self.triangles = capacity, ind, tri
        self._io = FrameIO(self.device)
        with torch.cuda.device(self.device):
            self._ind = torch.from_numpy(ind).to(self.device)
            self._tri = torch.from_numpy(tri).to(self.device)
            self._zero_origin = torch.zeros((capacity, 2), dtype=torch.int32, device=self.device)

    def _check(self, t, name, shape, dtype):
        if isinstance(t, np.ndarray):
            raise ValueError("%s is a host array: the renderer reads CUDA tensors, there is no CPU fallback" % name)
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor %s on %s (got %s)"
                             % (name, str(dtype).replace("torch.", ""), list(shape), self.device,
                                "%s %s on %s" % (t.dtype, list(t.shape), t.device) if isinstance(t, torch.Tensor) else type(t).__name__))

    def _maps(self, result_or_pos, slots):
        """-> (pos, slots) of a FaceResult or of a pos tensor with its slots, checked."""
        if isinstance(result_or_pos, FaceResult):
            if slots is not None:
                raise ValueError("slots= goes with a pos tensor: a FaceResult brings its own")
            if result_or_pos.pos is None:
                raise ValueError("this result was made with positions=False: it holds no position maps")
            pos, slots = result_or_pos.pos, result_or_pos.slots
        else:
            pos = result_or_pos
            if slots is None:
                raise ValueError("a pos tensor needs slots= (int32 [capacity], -1 for an unused slot)")
        self._check(pos, "pos", (self.capacity, RES, RES, 3), torch.float32)
        self._check(slots, "slots", (self.capacity,), torch.int32)
        return pos, slots

    def render(self, result_or_pos, slots=None, size=None, origin=None, attrs=None):
        """Rasterise every slot's mesh into its window -> FaceRender(tri, image), on the device, in the current stream, no
        synchronisation and no upload.
        result_or_pos: a FaceResult with position maps, or a CUDA float32 tensor [capacity, 256, 256, 3] with slots= (CUDA int32
        [capacity], a slot is used iff >= 0).
        size: (h, w) of every window, 1..4096 each, capacity * h * w * 8 < 2^31.
        origin: None (every window starts at frame pixel (0, 0)) or CUDA int32 [capacity, 2] = (x0, y0): image pixel (r, c) of slot s is
        frame pixel (x0 + c, y0 + r).  A slot whose origin lies outside +-2^20 is rendered like an unused one.
        attrs: None (the vertices' z: the depth image) or CUDA float32 [capacity, V, C], 1 <= C <= 4, e.g. `vertex_colors`.
        The rule is csrc/face_render_arith.h: a triangle's box is clamped to the window, so the result is the reference's render of any
        frame that contains the window, cropped to it."""
        pos, slots = self._maps(result_or_pos, slots)
        if (not isinstance(size, (tuple, list)) or len(size) != 2
                or not all(isinstance(v, (int, np.integer)) and 1 <= int(v) <= MAX_WINDOW for v in size)):
            raise ValueError("size must be (h, w) with both in 1..%d (got %r)" % (MAX_WINDOW, size))
        h, w = int(size[0]), int(size[1])
        cap, V = self.capacity, len(self.face_ind)
        if cap * h * w * 8 >= 1 << 31:
            raise ValueError("%d windows of %d x %d: the key buffer reaches 2^31 bytes" % (cap, h, w))
        if origin is None:
            origin = self._zero_origin
        else:
            self._check(origin, "origin", (cap, 2), torch.int32)
        C = 1
        if attrs is not None:
            if isinstance(attrs, torch.Tensor) and attrs.dim() == 3 and 1 <= attrs.shape[2] <= MAX_ATTRS:
                C = int(attrs.shape[2])
            self._check(attrs, "attrs", (cap, V, C), torch.float32)
        L = _lib.lib()
        with torch.cuda.device(self.device):
            nbytes = int(L.cp_face_render_scratch_bytes(cap, h, w, int(self._tri.shape[0])))
            scratch = torch.empty((nbytes // 8,), dtype=torch.int64, device=self.device)
            tri = torch.empty((cap, h, w), dtype=torch.int32, device=self.device)
            image = torch.empty((cap, h, w, C), dtype=torch.float32, device=self.device)
            _lib.check(L.cp_face_render_f32(pos.data_ptr(), slots.data_ptr(), cap, self._ind.data_ptr(), V, self._tri.data_ptr(),
                                            int(self._tri.shape[0]), origin.data_ptr(), h, w, None if attrs is None else attrs.data_ptr(), C,
                                            scratch.data_ptr(), nbytes, tri.data_ptr(), image.data_ptr(), _lib.stream()), "cp_face_render_f32")
        return FaceRender(tri, image)

    def vertex_colors(self, frames, result, slots=None, layout="hwc", color="bgr", matrix="bt601"):
        """The colour of every vertex where it lies in its frame (PRN.get_colors, prnet.py:155-168) -> float32 [capacity, V, 3] =
        (B, G, R) in 0..255, on the device, in the current stream; the descriptor table is the only upload.  Per vertex x is clamped to
        [0, W - 1], y to [0, H - 1], both rounded half to even; zeros for a coordinate that is not finite and for unused slots.
        frames: as for FaceAligner.align (any layout, BGR / RGB, every YUV colour and matrix); they are only read.  Frame n owns the
        slots n * q .. n * q + q - 1, q = capacity // N, as align fills them.  result: as for `render` (a pos tensor with slots=)."""
        pos, slots = self._maps(result, slots)
        if _holds_host_array(frames):
            raise ValueError("vertex_colors reads device frames (CUDA uint8 tensors): host arrays are not read, there is no CPU fallback")
        images, descs = self._io.batch_input(frames, layout, color, matrix)
        N, cap, V = len(descs or []), self.capacity, len(self.face_ind)
        if not 1 <= N <= cap:
            raise ValueError("%d frames for a capacity of %d slots" % (N, cap))
        yuv = is_yuv(color)
        table = identity_table(descs, yuv)
        L = _lib.lib()
        with torch.cuda.device(self.device):
            colors = torch.empty((cap, V, 3), dtype=torch.float32, device=self.device)
            table_dev, = self._io.upload_table([table])
            tail = (pos.data_ptr(), slots.data_ptr(), cap, self._ind.data_ptr(), V, colors.data_ptr(), _lib.stream())
            if yuv:
                coef = (ctypes.c_int * 6)(*yuv_coef(matrix))
                _lib.check(L.cp_face_vertex_colors_yuv_f32(table_dev.data_ptr(), table.ctypes.data, N, coef, *tail), "cp_face_vertex_colors_yuv_f32")
            else:
                _lib.check(L.cp_face_vertex_colors_f32(table_dev.data_ptr(), table.ctypes.data, N, *tail), "cp_face_vertex_colors_f32")
        return colors


class FaceAligner:
    """One compiled PRNet plan of `capacity` crops with the crop stage that feeds it and the restore behind it.

    state_dict: the reference module's own keys (`input_conv.1.weight`, `down_conv_1.main.0.weight`, ...; `load_prnet_state_dict`).
    uv_kpt_ind: [2, 68] integers in 0..255 or the path of the reference's text file; the product ships no reference data.
    expand / min_size: the crop square has side int(old_size * expand) and is taken iff that is in min_size..32768.
    face_ind / canonical_vertices: the two tables of the head pose (`check_pose_tables`), both or neither; with them
    `align(..., pose=True)` and `estimate_pose` are available."""

    def __init__(self, state_dict, uv_kpt_ind, capacity=8, device="cuda", expand=1.6, min_size=1, face_ind=None, canonical_vertices=None):
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
        if (face_ind is None) != (canonical_vertices is None):
            raise ValueError("the head pose needs face_ind and canonical_vertices together (got only %s)"
                             % ("face_ind" if canonical_vertices is None else "canonical_vertices"))
        tables = check_pose_tables(face_ind, canonical_vertices) if face_ind is not None else None
        self.capacity, self.expand, self.min_size = capacity, float(expand), int(min_size)
        self.uv_kpt_ind = uv
        self.engine = Engine("prnet", state_dict, capacity, nets.PRNET_INPUT[0], nets.PRNET_INPUT[1], device=device)
        self.device = self.engine.device if self.engine.device.index is not None else torch.device("cuda", torch.cuda.current_device())
        self._io = FrameIO(self.device)
        with torch.cuda.device(self.device):
            self._uv = torch.from_numpy(uv).to(self.device)
            self.face_ind = self._pose_tables = None
            if tables is not None:
                self.face_ind = tables[0]
                scratch = _lib.lib().cp_face_pose_scratch_bytes(capacity, len(tables[0]))
                # the centred cloud, its mean and rms_d1: uploaded once; the moments' scratch is this aligner's own
                self._pose_tables = tuple(torch.from_numpy(t).to(self.device) for t in tables) + (
                    torch.empty((scratch // 8,), dtype=torch.float64, device=self.device),)
            self.engine.capture()      # the one-off capture synchronises: here, not in the first align

    @property
    def face_ind_device(self):
        """The aligner's face_ind on the device (int32 [V]) or None."""
        return self._pose_tables[0] if self._pose_tables is not None else None

    @property
    def has_pose_tables(self):
        """True iff the aligner was built with face_ind and canonical_vertices: pose=True and estimate_pose are available."""
        return self._pose_tables is not None

    def renderer(self, triangles):
        """A FaceRenderer over this aligner's face_ind and capacity, on its device.  triangles: as for FaceRenderer."""
        if self.face_ind is None:
            raise ValueError("renderer needs a FaceAligner built with face_ind= (and canonical_vertices=)")
        return FaceRenderer(self.face_ind, triangles, self.capacity, device=self.device)

    def align(self, frames, rows=None, boxes=None, layout="hwc", color="bgr", matrix="bt601", vis_thresh=0.3, positions=True, pose=False):
        """Position maps and landmarks of the faces of `frames` -> FaceResult, on the device, in the current stream, no
        synchronisation; the descriptor table is the only upload.
        frames: as for ReidExtractor.embed -- a list of CUDA uint8 tensors or one 4-D tensor (`layout`, `color`, C = 3 or 4), or with a
        YUV color a list of plane tuples / surface tensors (`matrix`).  They are only read.  Host arrays raise ValueError.
        Exactly one of rows / boxes: rows CUDA float32 [N, M, 56] as run_batch(..., return_device=True) returns them (the face box is
        the extent of the five face joints), or boxes CUDA float32 [N, F, 5] = (x1, y1, x2, y2, score) (PRN.process(frame, box) on the
        whole frame).  A candidate gets a face iff its score is > vis_thresh and its square is valid (csrc/face_arith.h).
        positions=False: the 68 landmarks only; the maps are never written.
        pose=True: `FaceResult.pose` is the head pose of every slot (FacePose), from the plan's output where it lies: with
        positions=False the maps are still never written.  Needs the aligner's face_ind and canonical_vertices."""
        if pose and self._pose_tables is None:
            raise ValueError("pose=True needs a FaceAligner built with face_ind= and canonical_vertices=")
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
        return self._align(descs or [], cand.detach().contiguous(), boxes is not None, color, matrix, vis_thresh, positions, pose)

    def estimate_pose(self, result):
        """The head pose of a FaceResult's slots from its position maps -> FacePose (also set as `result.pose`), on the device, in the
        current stream, no synchronisation.  The same bits as align(..., pose=True) gives."""
        if self._pose_tables is None:
            raise ValueError("estimate_pose needs a FaceAligner built with face_ind= and canonical_vertices=")
        if result.pos is None:
            raise ValueError("this result was made with positions=False: it holds no position maps (use align(..., pose=True))")
        self._check_result(result, ("pos", "slots", "xform", "landmarks"))
        with torch.cuda.device(self.device):
            result.pose = self._pose(result.pos, True, result.slots, result.xform, result.landmarks)
        return result.pose

    def _check_result(self, result, names):
        cap = self.capacity
        shapes = dict(pos=((cap, RES, RES, 3), torch.float32), slots=((cap,), torch.int32), xform=((cap, 3), torch.float32),
                      landmarks=((cap, NKPT, 3), torch.float32), P=((cap, 3, 4), torch.float64), box=((cap, 10, 2), torch.int32),
                      valid=((cap,), torch.int32))
        for name in names:
            t = getattr(result.pose if name in ("box", "valid") else result, name)
            shape, dtype = shapes[name]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device or not t.is_contiguous():
                raise ValueError("the result is not one of this aligner's: %s must be a contiguous %s tensor %s on %s (got %s)"
                                 % (name, str(dtype).replace("torch.", ""), list(shape), self.device,
                                    "%s %s on %s" % (t.dtype, list(t.shape), t.device) if isinstance(t, torch.Tensor) else type(t).__name__))

    def draw(self, frames, result, layout="hwc", color="bgr", matrix="bt601", style=None):
        """Paint the faces of `result` (a FaceResult of this aligner for these frames) onto `frames`, in place, on the device, in the
        current stream -> `frames`.  What is drawn is the content of the reference's plot_kpt, plot_vertices and plot_pose_box
        (demo/face/utils/cv_plot.py) by this project's own rule (csrc/face_draw_arith.h): per face the 60
        lines between neighbouring landmarks, a disc on each of the 68 landmarks, then the 13 lines of the pose box where the pose is
        valid; faces in ascending slot order, the last painter wins, opaque, clipped; the dense vertices beneath everything.
        style: a FaceStyle; the default paints what the live loop pastes (plot_kpt).  pose_box=True on a result without a pose, and
        vertices=True without position maps or face_ind, raise ValueError.
        frames: as for draw_results, whose rules for writable frames apply and are checked before anything is launched: expanded or
        overlapping views, host arrays and the surface colours beyond 8-bit 4:2:0 raise.  The descriptor table is the only upload."""
        given = frames
        _check_layout(layout, color, matrix)
        check_drawable(color, matrix)
        if _holds_host_array(frames):
            raise ValueError("draw paints frames on the device (CUDA uint8 tensors): host arrays are not painted, there is no CPU fallback")
        images, descs = self._io.batch_input(frames, layout, color, matrix)
        style = FaceStyle() if style is None else style
        if not isinstance(style, FaceStyle):
            raise ValueError("style is a FaceStyle (got %s)" % type(style).__name__)
        if style.pose_box and result.pose is None:
            raise ValueError("pose_box=True needs a result with a pose (align(..., pose=True) or estimate_pose)")
        if style.vertices and (result.pos is None or self._pose_tables is None):
            raise ValueError("vertices=True needs the position maps (positions=True) and an aligner built with face_ind=")
        self._check_result(result, ["slots", "landmarks"] + (["box", "valid"] if style.pose_box else []) + (["pos"] if style.vertices else []))
        self._io.check_writable(given, images, color)
        with torch.cuda.device(self.device):
            draw_faces(self._io, descs or [], result, self._pose_tables[0] if self._pose_tables is not None else None, color, matrix, style)
        return given

    def _pose(self, src, from_pos, slots, xform, landmarks):
        """The two head-pose launches for a source that is the plan's output (from_pos False) or the restored maps."""
        cap = self.capacity
        face_ind, canon, stats, scratch = self._pose_tables
        P = torch.empty((cap, 3, 4), dtype=torch.float64, device=self.device)
        angles = torch.empty((cap, 3), dtype=torch.float64, device=self.device)
        scale = torch.empty((cap,), dtype=torch.float64, device=self.device)
        box = torch.empty((cap, 10, 2), dtype=torch.int32, device=self.device)
        valid = torch.empty((cap,), dtype=torch.int32, device=self.device)
        _lib.check(_lib.lib().cp_face_pose_f32(src.data_ptr(), int(from_pos), slots.data_ptr(), xform.data_ptr(), cap, face_ind.data_ptr(),
                                               int(face_ind.shape[0]), canon.data_ptr(), stats.data_ptr(), landmarks.data_ptr(),
                                               scratch.data_ptr(), scratch.numel() * 8, P.data_ptr(), angles.data_ptr(), scale.data_ptr(),
                                               box.data_ptr(), valid.data_ptr(), _lib.stream()), "cp_face_pose_f32")
        return FacePose(P, angles, scale, box, valid)

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

    def _align(self, descs, cand, boxes, color, matrix, vis_thresh, positions, pose=False):
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
            face_pose = self._pose(net, False, slots, xform, landmarks) if pose else None
        return FaceResult(pos, landmarks, slots, counts, xform, face_pose)
