"""ctypes binding of the C-ABI library ``libcenterpose_hip.so`` (see include/centerpose_hip.h).

There is deliberately no fallback: if the HIP library is missing or a tensor is not on the GPU
every entry point raises.  PyTorch is only used for device memory and the current HIP stream.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcenterpose_hip.so")
_lib = None

c_int, c_void_p, c_float, c_size_t = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_size_t


class CenterposeHipError(RuntimeError):
    pass


def lib():
    """Load (once) and return the ctypes handle.  Raises if the library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CenterposeHipError(
                "HIP library %s not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C centerpose_amd/csrc`).  There is no CPU fallback." % LIB_PATH)
        _lib = ctypes.CDLL(LIB_PATH)
        _lib.cp_last_error.restype = ctypes.c_char_p
        _lib.cp_target_arch.restype = ctypes.c_char_p
        _lib.cp_last_kernel.restype = ctypes.c_char_p
        # the head-pose stage (csrc/face_pose.hip): size_t crosses the boundary, so these are declared
        _lib.cp_face_pose_scratch_bytes.restype = c_size_t
        _lib.cp_face_pose_scratch_bytes.argtypes = [c_int, c_int]
        pose = [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int] + [c_void_p] * 4 + [c_size_t] + [c_void_p] * 5
        _lib.cp_face_pose_host.argtypes = pose
        _lib.cp_face_pose_f32.argtypes = pose + [c_void_p]
        # the face overlays (csrc/face_draw.hip)
        _lib.cp_face_draw_scratch_bytes.restype = c_size_t
        _lib.cp_face_draw_scratch_bytes.argtypes = [c_int]
        faces = [c_void_p, c_int, c_void_p, c_int] + [c_void_p] * 5 + [c_int, c_void_p]
        _lib.cp_face_draw_frames_host.argtypes = _lib.cp_face_draw_yuv_frames_host.argtypes = faces
        _lib.cp_face_draw_frames_u8.argtypes = _lib.cp_face_draw_yuv_frames_u8.argtypes = [c_void_p] + faces + [c_void_p, c_size_t, c_void_p]
        # the mesh rasteriser (csrc/face_render.hip)
        _lib.cp_face_render_scratch_bytes.restype = c_size_t
        _lib.cp_face_render_scratch_bytes.argtypes = [c_int] * 4
        render = [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_size_t,
                  c_void_p, c_void_p]
        _lib.cp_face_render_host.argtypes = render
        _lib.cp_face_render_f32.argtypes = render + [c_void_p]
        colors = [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p]
        _lib.cp_face_vertex_colors_host.argtypes = [c_void_p, c_int] + colors
        _lib.cp_face_vertex_colors_yuv_host.argtypes = [c_void_p, c_int, c_void_p] + colors
        _lib.cp_face_vertex_colors_f32.argtypes = [c_void_p, c_void_p, c_int] + colors + [c_void_p]
        _lib.cp_face_vertex_colors_yuv_f32.argtypes = [c_void_p, c_void_p, c_int, c_void_p] + colors + [c_void_p]
    return _lib


def check(rc, what):
    if rc != 0:
        raise CenterposeHipError("%s failed (rc=%d): %s" % (what, rc, lib().cp_last_error().decode()))


def ptr(t):
    """Device pointer of a contiguous float32/int32 CUDA(HIP) tensor, or NULL for None."""
    if t is None:
        return c_void_p(0)
    if not t.is_cuda:
        raise CenterposeHipError("centerpose_amd runs on the GPU only (got a %s tensor); "
                                 "the CPU path lives in oracle/ and is test infrastructure" % t.device)
    if not t.is_contiguous():
        raise CenterposeHipError("tensor must be contiguous")
    return c_void_p(t.data_ptr())


def vptr(t):
    """Device pointer of a strided NHWC *view* (layout is validated by the caller)."""
    if t is None:
        return c_void_p(0)
    if not t.is_cuda:
        raise CenterposeHipError("centerpose_amd runs on the GPU only (got a %s tensor)" % t.device)
    if t.dtype != torch.float32:
        raise CenterposeHipError("float32 tensor expected (got %s)" % t.dtype)
    return c_void_p(t.data_ptr())


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def f32(t, name="tensor"):
    if t is not None and t.dtype != torch.float32:
        raise CenterposeHipError("%s must be float32 (got %s)" % (name, t.dtype))
    return t
