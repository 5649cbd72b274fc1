"""The device-frame layer: how frames that lie on the device (packed BGR / RGB tensors, YUV planes and surfaces) are described to the kernels
that read or write them in place -- layouts and stride geometry, plane splitting, writability, the descriptor tables and the pinned
staging buffers of their uploads.  The detector, the re-id extractor and the tracker each own one ``FrameIO``; none is known here."""
from collections import defaultdict, namedtuple

import numpy as np
import torch

from . import _lib

# cp_pre_desc (include/centerpose_hip.h): one source image of a batched pre-process
PRE_DESC = np.dtype([("src_off", "<i8"), ("mid_off", "<i8"), ("H", "<i4"), ("W", "<i4"), ("NH", "<i4"), ("NW", "<i4"),
                     ("mi", "<f8", (6,)), ("slot", "<i4"), ("pad", "<i4")])

# cp_frame_desc (include/centerpose_hip.h): one source frame on the device, addressed by pointer and strides
FRAME_DESC = np.dtype([("base", "<u8"), ("row_stride", "<i8"), ("pix_stride", "<i8"), ("ch_off", "<i8", (3,)), ("mid_off", "<i8"),
                       ("H", "<i4"), ("W", "<i4"), ("NH", "<i4"), ("NW", "<i4"), ("mi", "<f8", (6,)), ("slot", "<i4"), ("pad", "<i4")])

# cp_yuv_frame_desc (include/centerpose_hip.h): one source frame on the device in YUV planes; `pad` is its format word (FMT_*)
YUV_FRAME_DESC = np.dtype([("y_base", "<u8"), ("y_row", "<i8"), ("y_pix", "<i8"), ("u_base", "<u8"), ("v_base", "<u8"), ("c_row", "<i8"),
                           ("c_pix", "<i8"), ("mid_off", "<i8"), ("H", "<i4"), ("W", "<i4"), ("NH", "<i4"), ("NW", "<i4"),
                           ("mi", "<f8", (6,)), ("slot", "<i4"), ("pad", "<i4")])

LAYOUTS, COLORS, YUV_COLORS = ("hwc", "chw"), ("bgr", "rgb"), ("nv12", "nv21", "i420")

# limited-range YUV -> BGR matrices (csrc/yuv_arith.h): (CY, CVR, CVG, CUG, CUB, YOFF), every entry round(k * 2^20)
YUV_MATRICES = {"bt601": (1220542, 1673527, -852492, -409993, 2116026, 16),       # 1.164, 1.596, -0.813, -0.391, 2.018
                "bt709": (1220542, 1880097, -558891, -223347, 2214593, 16)}       # 1.164, 1.793, -0.533, -0.213, 2.112

# The YUV colours beyond 8-bit 4:2:0 (csrc/yuv_source.h), read but never drawn on: P010 / P016 (semi-planar 16-bit samples, MSB
# aligned), planar 4:2:2 and 4:4:4, grey, packed 4:2:2.  The bits of the descriptor's format word: chroma not subsampled horizontally /
# vertically, 16-bit little-endian samples, no chroma planes.
SURFACE_COLORS = ("p010", "p016", "i422", "i444", "i400", "yuyv", "uyvy")
FMT_FULL_X, FMT_FULL_Y, FMT_16BIT, FMT_GREY = 1, 2, 4, 8


# The matrices beyond YUV_MATRICES, for every YUV colour: full range (JPEG / MJPEG) and BT.2020.  The closed form from the luma weights
# (Kr, Kb), Kg = 1 - Kr - Kb, in double: CVR = 2(1-Kr)c, CUB = 2(1-Kb)c, CVG = -2Kr(1-Kr)/Kg c, CUG = -2Kb(1-Kb)/Kg c, CY = l; full range
# l = c = 1, YOFF 0; limited range l = 255/219, c = 255/224, YOFF 16.  "bt601" / "bt709" keep cv2's three-decimal rows above.
SURFACE_MATRICES = {"bt601-full": (1048576, 1470104, -748826, -360853, 1858077, 0),
                    "bt709-full": (1048576, 1651297, -490864, -196424, 1945738, 0),
                    "bt2020-limited": (1220945, 1760217, -682019, -196426, 2245811, 16),
                    "bt2020-full": (1048576, 1546230, -599107, -172546, 1972791, 0)}


def is_yuv(color):
    return color in YUV_COLORS or color in SURFACE_COLORS


def yuv_coef(matrix):
    """The six ints of a matrix name (YUV_MATRICES or SURFACE_MATRICES)."""
    return YUV_MATRICES[matrix] if matrix in YUV_MATRICES else SURFACE_MATRICES[matrix]


def check_drawable(color, matrix):
    """Raise for what the draw kernels do not take: they write 8-bit 4:2:0 chroma and know the forward matrices of YUV_MATRICES only."""
    if color in SURFACE_COLORS:
        raise _lib.CenterposeHipError("color=%r frames cannot be drawn on: drawing takes bgr, rgb and 8-bit 4:2:0 (%s) frames only"
                                      % (color, " / ".join(YUV_COLORS)))
    if matrix in SURFACE_MATRICES:
        raise _lib.CenterposeHipError("matrix=%r is not taken for drawing: the palette is converted with %s only"
                                      % (matrix, " / ".join(sorted(YUV_MATRICES))))


# one checked device frame (FrameIO.frame / FrameIO.yuv_frame): the address fields carry the names of their descriptor's; a frame of
# one of SURFACE_COLORS carries its format word as well
Frame = namedtuple("Frame", "base H W row_stride pix_stride ch_off")
YuvFrame = namedtuple("YuvFrame", "y_base H W y_row y_pix u_base v_base c_row c_pix")
YuvSurface = namedtuple("YuvSurface", YuvFrame._fields + ("fmt",))


def _check_layout(layout, color, matrix="bt601"):
    if layout not in LAYOUTS:
        raise _lib.CenterposeHipError("unknown layout %r: one of %s" % (layout, ", ".join(LAYOUTS)))
    if color not in COLORS + YUV_COLORS + SURFACE_COLORS:
        raise _lib.CenterposeHipError("unknown color %r: one of %s" % (color, ", ".join(COLORS + YUV_COLORS + SURFACE_COLORS)))
    if matrix not in YUV_MATRICES and matrix not in SURFACE_MATRICES:
        raise _lib.CenterposeHipError("unknown matrix %r: one of %s" % (matrix, ", ".join(sorted(YUV_MATRICES) + sorted(SURFACE_MATRICES))))
    if is_yuv(color) and layout != "hwc":
        raise _lib.CenterposeHipError("layout=%r does not apply to color=%r: YUV frames are given as planes" % (layout, color))
    if not is_yuv(color) and matrix != "bt601":
        raise _lib.CenterposeHipError("matrix=%r applies to YUV frames (color %s) only, not to color=%r"
                                      % (matrix, " / ".join(YUV_COLORS + SURFACE_COLORS), color))


def frame_geometry(shape, strides, layout="hwc", color="bgr"):
    """How a uint8 frame of the given shape and strides (in elements == bytes) is addressed: (H, W, row_stride, pix_stride, ch_off),
    channel k of the network (cv2's B, G, R) of pixel (y, x) at byte y * row_stride + x * pix_stride + ch_off[k] from the frame's first
    element.  layout "hwc": [H,W,C], "chw": [C,H,W]; C = 3 or 4 (a fourth channel is never read); color: the order of the first three
    channels in memory.  A pure function of its arguments: nothing is copied, any strides (crops, padded rows, expanded views) go."""
    _check_layout(layout, color)
    if is_yuv(color):
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
    if color in SURFACE_COLORS:
        raise _lib.CenterposeHipError("color=%r frames carry a format word: yuv_surface_geometry" % color)
    if color not in YUV_COLORS:
        raise _lib.CenterposeHipError("color=%r frames are not planes: frame_geometry" % color)
    shapes, strides = _plane_shapes(shapes, strides)
    for dt in (dtypes or ()):
        if not _is_dtype(dt, "uint8"):
            raise _lib.CenterposeHipError("the planes of a YUV frame must be uint8 (got %s)" % (dt,))
    return _geometry_420(shapes, strides, color, color)


def _plane_shapes(shapes, strides):
    shapes = [tuple(int(v) for v in s) for s in shapes]
    strides = [tuple(int(v) for v in s) for s in strides]
    if len(shapes) != len(strides) or any(len(a) != len(b) for a, b in zip(shapes, strides)):
        raise _lib.CenterposeHipError("one stride per dimension of every plane: shapes %s, strides %s" % (shapes, strides))
    return shapes, strides


def _is_dtype(dt, name):
    """Whether a torch or NumPy dtype is the one called `name` ("uint8", "int16", "uint16")."""
    if isinstance(dt, torch.dtype):
        return dt is getattr(torch, name, None)
    return np.dtype(dt) == np.dtype(name)


def _geometry_420(shapes, strides, color, kind):
    """yuv_frame_geometry's rule for checked shapes / strides; kind: the layout ("nv12": uv pairs, "nv21": vu pairs, "i420": two planes),
    color: the name the texts use."""
    if any(v < 0 for s in strides for v in s):
        raise _lib.CenterposeHipError("negative strides %s are not addressable" % (strides,))
    if len(shapes) == 1:                                       # the decoder's surface: luma rows, then the interleaved chroma rows
        if kind == "i420":
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
        u_off, v_off = (first, first + pix) if kind == "nv12" else (first + pix, first)
        return H, W, pitch, pix, u_off, v_off, pitch, 2 * pix
    want = 2 if kind in ("nv12", "nv21") else 3
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
        u_off, v_off = (0, sc) if kind == "nv12" else (sc, 0)
    else:
        if shapes[1] != (ch, cw) or shapes[2] != (ch, cw):
            raise _lib.CenterposeHipError("the u and v planes of a %d x %d i420 frame are [%d,%d], got shapes %s and %s"
                                          % (H, W, ch, cw, shapes[1], shapes[2]))
        if strides[1] != strides[2]:
            raise _lib.CenterposeHipError("the u and v planes must have equal strides (%s and %s)" % (strides[1], strides[2]))
        (c_row, c_pix), u_off, v_off = strides[1], 0, 0
    return H, W, strides[0][0], strides[0][1], u_off, v_off, c_row, c_pix


def yuv_surface_geometry(shapes, strides, color="p010", dtypes=None):
    """How a YUV frame of any colour is addressed, IN BYTES, with its format word.  shapes / strides (in elements): one entry per tensor
    of the frame; dtypes: the tensors' dtypes when known.
      "p010" / "p016" (synonyms)  uint16 or int16 tensors of one dtype (the bit pattern counts), the forms of "nv12": (y [H,W],
                                  uv [ceil(H/2),ceil(W/2),2]) or ONE 2-D surface [H*3/2, W] with even H and W
      "i422"                      uint8 (y [H,W], u, v [H,ceil(W/2)]), u and v of equal strides
      "i444"                      uint8 (y, u, v), all [H,W], u and v of equal strides
      "i400"                      uint8, one 2-D tensor [H,W] (or a 1-tuple of it): no chroma, U = V = 128
      "yuyv" / "uyvy"             uint8, one tensor [H,W,2] with even W: Y at element 0 / 1 of each pixel, U and V at the other element
                                  of the even and of the odd pixel
      "nv12" / "nv21" / "i420"    as yuv_frame_geometry, format word 0
    -> (H, W, y_off, y_row, y_pix, u_off, v_off, c_row, c_pix, fmt): Y(r, c) at byte y_off + r * y_row + c * y_pix of the first tensor,
    U(r, c) at byte u_off + (r >> sy) * c_row + (c >> sx) * c_pix of the tensor that holds it (the second of several tensors, else the
    first), V(r, c) the same from v_off (the last tensor); sx = 0 with FMT_FULL_X, sy = 0 with FMT_FULL_Y, else 1; u_off = v_off = None
    with FMT_GREY.  A pure function of its arguments: nothing is copied, any non-negative strides go."""
    _check_layout("hwc", color)
    if color in YUV_COLORS:
        H, W, y_row, y_pix, u_off, v_off, c_row, c_pix = yuv_frame_geometry(shapes, strides, color, dtypes)
        return H, W, 0, y_row, y_pix, u_off, v_off, c_row, c_pix, 0
    if color not in SURFACE_COLORS:
        raise _lib.CenterposeHipError("color=%r frames are not planes: frame_geometry" % color)
    shapes, strides = _plane_shapes(shapes, strides)
    dtypes = list(dtypes or ())
    if color in ("p010", "p016"):
        for dt in dtypes:
            if not (_is_dtype(dt, "uint16") or _is_dtype(dt, "int16")):
                raise _lib.CenterposeHipError("the planes of a %s frame must be uint16 or int16 (got %s)" % (color, dt))
        if any(not _is_dtype(dt, "uint16") for dt in dtypes) and any(not _is_dtype(dt, "int16") for dt in dtypes):
            raise _lib.CenterposeHipError("the planes of a %s frame must have the same dtype (got %s)" % (color, ", ".join(str(d) for d in dtypes)))
        H, W, y_row, y_pix, u_off, v_off, c_row, c_pix = _geometry_420(shapes, strides, color, "nv12")
        return H, W, 0, 2 * y_row, 2 * y_pix, 2 * u_off, 2 * v_off, 2 * c_row, 2 * c_pix, FMT_16BIT
    for dt in dtypes:
        if not _is_dtype(dt, "uint8"):
            raise _lib.CenterposeHipError("the planes of a %s frame must be uint8 (got %s)" % (color, dt))
    if any(v < 0 for s in strides for v in s):
        raise _lib.CenterposeHipError("negative strides %s are not addressable" % (strides,))
    if color in ("i422", "i444"):
        if len(shapes) != 3:
            raise _lib.CenterposeHipError("a %s frame is (y, u, v), got %d tensors" % (color, len(shapes)))
    elif len(shapes) != 1:
        raise _lib.CenterposeHipError("a %s frame is one tensor, got %d tensors" % (color, len(shapes)))
    packed = color in ("yuyv", "uyvy")
    if len(shapes[0]) != (3 if packed else 2) or (packed and shapes[0][2] != 2):
        raise _lib.CenterposeHipError("%s, got shape %s" % ("a %s frame is one tensor [H,W,2]" % color if packed else "the y plane is 2-D [H,W]",
                                                            shapes[0]))
    H, W = shapes[0][:2]
    if H <= 0 or W <= 0:
        raise _lib.CenterposeHipError("a frame of shape %s has no pixels" % (shapes[0],))
    if packed:
        if W % 2:
            raise _lib.CenterposeHipError("a %s frame [H,W,2] needs an even W, got shape %s: U and V come in pairs of pixels" % (color, shapes[0]))
        sh, sw, sc = strides[0]
        y_off, u_off, v_off = (0, sc, sw + sc) if color == "yuyv" else (sc, 0, sw)
        return H, W, y_off, sh, sw, u_off, v_off, sh, 2 * sw, FMT_FULL_Y
    if color == "i400":
        return H, W, 0, strides[0][0], strides[0][1], None, None, 0, 0, FMT_GREY
    cw = (W + 1) // 2 if color == "i422" else W
    if shapes[1] != (H, cw) or shapes[2] != (H, cw):
        raise _lib.CenterposeHipError("the u and v planes of a %d x %d %s frame are [%d,%d], got shapes %s and %s"
                                      % (H, W, color, H, cw, shapes[1], shapes[2]))
    if strides[1] != strides[2]:
        raise _lib.CenterposeHipError("the u and v planes must have equal strides (%s and %s)" % (strides[1], strides[2]))
    return H, W, 0, strides[0][0], strides[0][1], 0, 0, strides[1][0], strides[1][1], (FMT_FULL_Y if color == "i422" else FMT_FULL_X | FMT_FULL_Y)


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


def identity_table(frames, yuv):
    """The FRAME_DESC (`yuv`: YUV_FRAME_DESC) table that addresses `frames` (a Frame / YuvFrame / YuvSurface each, or plain tuples in
    that order) at their own size: NH = H, NW = W, mid_off = -1, the rest zero (a YuvSurface's format word goes to `pad`).  The one
    place that maps a frame onto a descriptor row."""
    table = np.zeros(len(frames), YUV_FRAME_DESC if yuv else FRAME_DESC)
    for d, f in zip(table, frames):
        if yuv:
            d["y_base"], d["H"], d["W"], d["y_row"], d["y_pix"], d["u_base"], d["v_base"], d["c_row"], d["c_pix"] = f[:9]
            d["pad"] = f[9] if len(f) > 9 else 0
        else:
            d["base"], d["H"], d["W"], d["row_stride"], d["pix_stride"], d["ch_off"] = f
        d["NH"], d["NW"], d["mid_off"] = d["H"], d["W"], -1
    return table


def check_rows(rows, n_frames, device, owner, on_host=None, what="a CUDA float32 tensor [N, M, 56]", one="frame", f32="float32"):
    """The check of detection rows that draw_results, embed and the tracker share -> the rows as [N, M, 56] ([M, 56] is one block).
    device: where they must lie, or a callable that says so (asked for CUDA rows only), None: any GPU; owner: the caller's words for what
    lives there; on_host: its text for rows off the GPU; what / one / f32: words its texts differ in; n_frames None: it counts itself."""
    if not isinstance(rows, torch.Tensor):
        raise _lib.CenterposeHipError("rows must be %s on the device (got %s): there is no CPU fallback" % (what, type(rows).__name__))
    rows = rows.unsqueeze(0) if rows.dim() == 2 else rows
    if rows.dim() != 3 or rows.shape[2] != 56:
        raise _lib.CenterposeHipError("rows must be [N, M, 56] (or [M, 56] for one %s), got shape %s" % (one, tuple(rows.shape)))
    if not rows.is_cuda and on_host is not None:
        raise _lib.CenterposeHipError(on_host % rows.device)
    device = device() if rows.is_cuda and callable(device) else device
    if not rows.is_cuda or (device is not None and rows.device != device):
        raise _lib.CenterposeHipError("rows on %s, " % rows.device + owner % device)
    if rows.dtype != torch.float32:
        raise _lib.CenterposeHipError("rows must be %s (got %s)" % (f32, rows.dtype))
    if n_frames is not None and rows.shape[0] != n_frames:
        raise _lib.CenterposeHipError("rows hold %d blocks for %d frames" % (rows.shape[0], n_frames))
    return rows


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


class FrameIO:
    """What one owner (a detector, an extractor, a tracker) needs to take frames on its device and to upload tables to it.  device: the
    owner's card as a torch.device with an index, or a callable that gives it per call (a detector's model may be moved).  buffers: the
    dict of its staging buffers by purpose ("images", "table"); never shared: a `_Staging.host()` only orders against its own uploads."""

    def __init__(self, device, buffers=None):
        self.device = device if callable(device) else lambda: device
        self.buffers = defaultdict(_Staging) if buffers is None else buffers

    @staticmethod
    def host_layout_only(layout, color, matrix="bt601"):
        _check_layout(layout, color, matrix)      # unknown names raise
        if (layout, color) != ("hwc", "bgr"):
            raise _lib.CenterposeHipError("host arrays are taken in cv2's layout (HxWx3, BGR): layout=%r / color=%r apply to frames "
                                          "on the device (CUDA uint8 tensors) only" % (layout, color))

    def frame(self, t, layout, color):
        """One device frame -> Frame(address of pixel (0,0), H, W, row_stride, pix_stride, ch_off), all from the tensor's own shape,
        strides and data pointer: a valid view cannot address outside its storage.  The tensor is never copied or made contiguous."""
        if not t.is_cuda:
            raise _lib.CenterposeHipError("a frame tensor on %s: frames given as tensors must be on the model's GPU (host frames are "
                                          "passed as numpy arrays); there is no host fallback" % t.device)
        if t.dtype != torch.uint8:
            raise _lib.CenterposeHipError("a frame tensor must be uint8 (got %s)" % t.dtype)
        geometry = frame_geometry(t.shape, t.stride(), layout, color)
        device = self.device()
        if t.device != device:
            raise _lib.CenterposeHipError("a frame tensor on %s, the model is on %s" % (t.device, device))
        return Frame(t.data_ptr(), *geometry)

    def yuv_frame(self, frame, color):
        """One device frame in 4:2:0 YUV -> YuvFrame(address of Y(0,0), H, W, y_row, y_pix, address of U(0,0), address of V(0,0), c_row,
        c_pix), all from the plane tensors' own shapes, strides and data pointers.  One 2-D surface tensor (nv12 / nv21) is split into
        the views t[:H] and t[H:].unflatten(1, (W // 2, 2)) by address alone.  Nothing is copied or made contiguous.  A frame of one of
        SURFACE_COLORS -> YuvSurface: the same fields in bytes and its format word (yuv_surface_geometry)."""
        planes = [frame] if isinstance(frame, (torch.Tensor, np.ndarray)) else list(frame)
        if not planes:
            raise _lib.CenterposeHipError("a %s frame without planes" % color)
        if any(isinstance(t, np.ndarray) for t in planes):
            if all(isinstance(t, np.ndarray) for t in planes):
                raise _lib.CenterposeHipError("host arrays are taken in cv2's layout (HxWx3, BGR): color=%r applies to frames on the "
                                              "device (CUDA uint8 plane tensors) only" % color)
            raise _lib.CenterposeHipError("host arrays and device tensors mixed in one frame: pass all planes as CUDA tensors")
        if not all(isinstance(t, torch.Tensor) for t in planes) and color in SURFACE_COLORS:
            raise _lib.CenterposeHipError("a %s frame is CUDA tensors (yuv_surface_geometry has the forms), got %s"
                                          % (color, ", ".join(type(t).__name__ for t in planes)))
        if not all(isinstance(t, torch.Tensor) for t in planes):
            raise _lib.CenterposeHipError("a %s frame is a tuple of CUDA uint8 plane tensors (or one surface tensor for nv12 / nv21)" % color)
        for t in planes:
            if not t.is_cuda:
                raise _lib.CenterposeHipError("a plane tensor on %s: the planes of a frame must be on the model's GPU; there is no host "
                                              "fallback" % t.device)
        H, W, y_off, y_row, y_pix, u_off, v_off, c_row, c_pix, fmt = yuv_surface_geometry([t.shape for t in planes], [t.stride() for t in planes],
                                                                                          color, [t.dtype for t in planes])
        device = self.device()
        for t in planes:
            if t.device != device:
                raise _lib.CenterposeHipError("a plane tensor on %s, the model is on %s" % (t.device, device))
        u_plane, v_plane = (planes[0], planes[0]) if len(planes) == 1 else (planes[1], planes[-1])
        u_base, v_base = (0, 0) if u_off is None else (u_plane.data_ptr() + u_off, v_plane.data_ptr() + v_off)
        if color in YUV_COLORS:
            return YuvFrame(planes[0].data_ptr(), H, W, y_row, y_pix, u_base, v_base, c_row, c_pix)
        return YuvSurface(planes[0].data_ptr() + y_off, H, W, y_row, y_pix, u_base, v_base, c_row, c_pix, fmt)

    def batch_input(self, images, layout, color, matrix="bt601"):
        """What a batched call was given -> (images as a list, frames): frames is None for host arrays (the staging path), else one
        `frame` per device tensor (`yuv_frame` per frame with a YUV color).  One 4-D tensor means N frames ([N,H,W,C] or [N,C,H,W])."""
        _check_layout(layout, color, matrix)      # unknown names raise, whatever the input
        if is_yuv(color):
            if isinstance(images, (torch.Tensor, np.ndarray)):
                raise _lib.CenterposeHipError("a batch of %s frames is a list of frames (plane tuples or surface tensors), got one %s of "
                                              "shape %s" % (color, type(images).__name__, tuple(images.shape)))
            images = list(images)
            host = sum(isinstance(im, np.ndarray) for im in images)
            if 0 < host < len(images):
                raise _lib.CenterposeHipError("host arrays and device tensors mixed in one call: pass all frames one way")
            return images, [self.yuv_frame(im, color) for im in images]
        if isinstance(images, torch.Tensor):
            if images.dim() != 4:
                raise _lib.CenterposeHipError("one tensor for N frames is 4-D ([N,H,W,C] or [N,C,H,W]), got shape %s; pass a list of "
                                              "3-D frames otherwise" % (tuple(images.shape),))
            images = images.unbind(0)
        images = list(images)
        tensors = sum(isinstance(im, torch.Tensor) for im in images)
        if tensors == 0:
            if images:
                self.host_layout_only(layout, color)
            for im in images:
                if not (isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3 and im.shape[0] > 0
                        and im.shape[1] > 0):
                    raise _lib.CenterposeHipError("run_batch / pre_process_batch expect HxWx3 uint8 arrays (cv2.imread layout); there is no "
                                                  "host fallback")
            return images, None
        if tensors != len(images):
            raise _lib.CenterposeHipError("host arrays and device tensors mixed in one call: pass all frames one way")
        return images, [self.frame(t, layout, color) for t in images]

    @staticmethod
    def check_writable(given, images, color):
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

    def upload_images(self, images, offsets, nbytes):
        """The N images into the pinned staging buffer, ONE host-to-device copy -> device uint8 [nbytes]."""
        st = self.buffers["images"]
        host = st.host(nbytes)
        for im, off in zip(images, offsets):
            host[off:off + im.size] = im.reshape(-1)
        return st.upload(nbytes)

    def upload_table(self, parts):
        """Host arrays (descriptor tables, affines; 8-byte items) back to back in the pinned table buffer, ONE copy -> the device
        uint8 views of the parts."""
        raw = [np.ascontiguousarray(p).view(np.uint8).reshape(-1) for p in parts]
        st = self.buffers["table"]
        host = st.host(sum(r.size for r in raw))
        pos, spans = 0, []
        for r in raw:
            host[pos:pos + r.size] = r
            spans.append((pos, r.size))
            pos += r.size
        dev = st.upload(pos)
        return [dev[a:a + n] for a, n in spans]
