"""What the render tests share on the library's side: the calls of the HOST twins (cp_face_render_host, cp_face_vertex_colors_host,
cp_face_vertex_colors_yuv_host) over guarded arrays, descriptor tables over YUV surfaces, and the recording."""
import ctypes
import functools
import os

import numpy as np

import face_render_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                 # elements behind every output that no call may touch
KEY_SENTINEL = 0x7777777777777777
VP = ctypes.c_void_p


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "face_render.npz")))


def outputs(cap, h, w, C):
    """Guarded, sentinel-filled outputs of one render call: the keys, tri and image, flat."""
    n = cap * h * w
    return dict(keys=np.full(n + GUARD, KEY_SENTINEL, np.uint64), tri=np.full(n + GUARD, -7, np.int32), image=np.full(n * C + GUARD, np.nan, np.float32))


def guards_intact(out, cap, h, w, C):
    n = cap * h * w
    return (out["keys"][n:] == KEY_SENTINEL).all() and (out["tri"][n:] == -7).all() and np.isnan(out["image"][n * C:]).all()


def shaped(out, cap, h, w, C):
    n = cap * h * w
    return dict(keys=out["keys"][:n].reshape(cap, h, w), tri=out["tri"][:n].reshape(cap, h, w), image=out["image"][:n * C].reshape(cap, h, w, C))


def host_render(L, pos, slots, face_ind, triangles, origin, h, w, attrs=None, scratch_bytes=None):
    """-> (rc, dict of keys [cap, h, w], tri [cap, h, w], image [cap, h, w, C]); guards checked."""
    cap, V, T = len(slots), len(face_ind), len(triangles)
    C = 1 if attrs is None else attrs.shape[2]
    a = [np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(face_ind, np.int32),
         np.ascontiguousarray(triangles, np.int32), np.ascontiguousarray(origin, np.int32)]
    at = None if attrs is None else np.ascontiguousarray(attrs, np.float32)
    out = outputs(cap, h, w, C)
    p = lambda x: x.ctypes.data
    rc = L.cp_face_render_host(p(a[0]), p(a[1]), cap, p(a[2]), V, p(a[3]), T, p(a[4]), h, w, None if at is None else p(at), C, p(out["keys"]),
                               cap * h * w * 8 if scratch_bytes is None else scratch_bytes, p(out["tri"]), p(out["image"]))
    assert guards_intact(out, cap, h, w, C)
    return rc, shaped(out, cap, h, w, C)


def host_colors(L, table, yuv, N, pos, slots, face_ind, matrix_coef=None):
    """-> (rc, colors [cap, V, 3]) over a host descriptor table; the guard behind the output is checked."""
    cap, V = len(slots), len(face_ind)
    a = [np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(face_ind, np.int32)]
    out = np.full(cap * V * 3 + GUARD, np.nan, np.float32)
    p = lambda x: x.ctypes.data
    if yuv:
        coef = (ctypes.c_int * 6)(*matrix_coef)
        rc = L.cp_face_vertex_colors_yuv_host(p(table), N, coef, p(a[0]), p(a[1]), cap, p(a[2]), V, p(out))
    else:
        rc = L.cp_face_vertex_colors_host(p(table), N, p(a[0]), p(a[1]), cap, p(a[2]), V, p(out))
    assert np.isnan(out[cap * V * 3:]).all()
    return rc, out[:cap * V * 3].reshape(cap, V, 3)


def surface_table(planes_list, color, address_of):
    """The YUV descriptor table over the planes of N frames of a surface colour (p010, yuyv, ...), each plane at address_of(plane)."""
    from centerpose_amd import frames
    rows = []
    for planes in planes_list:
        H, W, y_off, y_row, y_pix, u_off, v_off, c_row, c_pix, fmt = frames.yuv_surface_geometry(
            [p.shape for p in planes], [tuple(s // p.itemsize for s in p.strides) for p in planes], color, [p.dtype for p in planes])
        u_plane, v_plane = (planes[0], planes[0]) if len(planes) == 1 else (planes[1], planes[-1])
        rows.append(frames.YuvSurface(address_of(planes[0]) + y_off, H, W, y_row, y_pix, address_of(u_plane) + u_off, address_of(v_plane) + v_off,
                                      c_row, c_pix, fmt))
    return frames.identity_table(rows, True)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def color_vertices(seed, V, H, W):
    """float32 [V, 3] for the colour tests: inside the frame, outside on every side, exact .5 ties (np.round: half to even), +-1e30,
    NaN and inf."""
    r = np.random.RandomState(seed)
    v = np.empty((V, 3), np.float64)
    v[:, 0], v[:, 1], v[:, 2] = r.uniform(-6, W + 6, V), r.uniform(-6, H + 6, V), r.uniform(-5, 5, V)
    ties = np.arange(V) % 3 == 0
    v[ties, 0] = np.floor(v[ties, 0]) + 0.5
    v[ties, 1] = np.floor(v[ties, 1]) + 0.5
    v[0], v[1], v[2], v[3] = (np.nan, 3, 0), (3, np.inf, 0), (1e30, -1e30, 0), (0.5, 1.5, np.nan)
    v[4], v[5], v[6] = (W - 1.5, H - 1.5, 0), (W - 0.5, H - 0.5, 0), (-0.5, 2.5, 0)
    return v.astype(np.float32)


def fuzz_call(seed, C, h=21, w=27):
    """The arguments of one render call (C = 0: the z attributes): cap = 3 with slot 1 unused, a window origin per slot (one negative),
    V = 300, T = 700."""
    V, T = 300, 700
    face_ind = np.random.RandomState(seed).permutation(65536)[:V].astype(np.int32)
    origin = np.asarray([[0, 0], [5, 5], [-40, 1000]], np.int32)
    pos, tris = [], None
    for s in range(3):
        v, tris = ref.fuzz_mesh(seed, V, T, h, w, int(origin[s, 0]), int(origin[s, 1]))
        if s == 2:
            v = (v + np.float32(0.25)).astype(np.float32)
        pos.append(ref.place(v, face_ind))
    attrs = None if C == 0 else np.random.RandomState(seed + 1).uniform(-3, 300, (3, V, C)).astype(np.float32)
    return np.stack(pos), np.asarray([0, -1, 4], np.int32), face_ind, tris, origin, h, w, attrs


def golden_case(g, k):
    """Case k of the recording -> (pos [256, 256, 3], face_ind, triangles, origin (x0, y0), h, w, colors [V, 3])."""
    from centerpose_amd import face
    face_ind = g["face_ind"]
    return (ref.place(g["vertices"][k], face_ind), face_ind, face.grid_triangles(face_ind), g["origin"][k], int(g["size"][0]), int(g["size"][1]),
            g["colors"][k])
