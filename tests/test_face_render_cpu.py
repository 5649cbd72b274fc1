"""CPU: the mesh rasteriser without a device -- the host twin (cp_face_render_host, csrc/face_render_host.h) against the recording of
the reference's get_triangle_buffer / render_texture (tests/golden/face_render.npz) and against the independent NumPy statement
(tests/face_render_ref.py: the sequential strict `>` on a depth buffer, not the 64-bit key), the vertex colours' twins against
np.round / np.clip on the pictures the frames show, grid_triangles, and the refusals of the calls and of the tables.

Bars: tri equal, image equal bit for bit (the recording as reference.astype(float32)); the recording script asserts the margins that make
these bars fair (no barycentric within 1e-6 of an edge, no two depths on one pixel within 1e-3).  DESIGN.md section 4.17."""
import numpy as np
import pytest

import draw_ref
import draw_util
import face_render_ref as ref
import face_render_util as fru
import reid_ref
import yuv_ref
import yuv_surface_ref as ysr


@pytest.fixture(scope="module")
def L():
    return draw_util.lib_built()


def test_host_twin_equals_the_recording(L):
    g = fru.golden()
    K = len(g["vertices"])
    cases = [fru.golden_case(g, k) for k in range(K)]
    _, face_ind, tri, _, h, w, _ = cases[0]
    assert K == 3 and (h, w) == (40, 48) and tri.shape == (1058, 3)
    pos = np.stack([c[0] for c in cases] + [cases[0][0]])
    slots = np.asarray([5, 0, 7, -1], np.int32)                                  # the last slot is unused
    origin = np.concatenate([g["origin"], [[0, 0]]]).astype(np.int32)
    rc, depth = fru.host_render(L, pos, slots, face_ind, tri, origin, h, w)
    assert rc == 0, L.cp_last_error()
    colors = np.stack([c[6] for c in cases] + [cases[0][6]])
    rc, tex = fru.host_render(L, pos, slots, face_ind, tri, origin, h, w, colors)
    assert rc == 0, L.cp_last_error()
    for k in range(K):
        assert np.array_equal(depth["tri"][k], g["tri"][k]) and np.array_equal(tex["tri"][k], g["tri"][k])
        assert fru.same_bits(depth["image"][k], g["depth"][k]) and fru.same_bits(tex["image"][k], g["texture"][k])
        assert 600 < (g["tri"][k] >= 0).sum() < 40 * 48
    assert (depth["tri"][3] == -1).all() and not depth["image"][3].any() and not tex["image"][3].any() and not depth["keys"][3].any()
    # ... and the NumPy statement meets the recording too
    rt, ri = ref.render_slots(pos, slots, face_ind, tri, origin, h, w, colors)
    assert np.array_equal(rt, tex["tri"]) and fru.same_bits(ri, tex["image"])


@pytest.mark.parametrize("C", [0, 1, 2, 3, 4], ids=["z", "c1", "c2", "c3", "c4"])
def test_host_twin_equals_the_numpy_statement(L, C):
    args = fru.fuzz_call(900 + C, C)
    rc, out = fru.host_render(L, *args)
    assert rc == 0, L.cp_last_error()
    rt, ri = ref.render_slots(*args)
    assert np.array_equal(out["tri"], rt) and fru.same_bits(out["image"], ri)
    assert (out["tri"][1] == -1).all() and not out["image"][1].any()
    for s in (0, 2):
        seen = out["tri"][s]
        assert (seen >= 0).mean() > 0.5 and len(np.unique(seen)) > 20
    # the keys are the rule's: ordered(depth) above, 0xFFFFFFFF - index below, 0 for no triangle
    keys = out["keys"]
    assert np.array_equal(np.where(keys == 0, -1, 0xFFFFFFFF - (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)), out["tri"])


def _one_slot(vertices, tris, h, w, origin=(0, 0)):
    v = np.asarray(vertices, np.float32)
    face_ind = np.arange(len(v), dtype=np.int32) * 7
    return ref.place(v, face_ind)[None], np.asarray([0], np.int32), face_ind, np.asarray(tris, np.int32), np.asarray([origin], np.int32), h, w


def test_ties_degenerates_and_skipped_triangles(L):
    big = [(-1, -1, 2), (20, -1, 2), (-1, 20, 2)]                                # covers the 6 x 8 window
    v = big + [(-1, -1, 2), (20, -1, 2), (-1, 20, 2),                            # 3..5: the same triangle again
               (1, 1, 0.0), (4, 1, 0.0), (1, 4, -0.0), (1, 1, -0.0), (4, 1, -0.0), (1, 4, -0.0),     # 6..11: depth +0 and -0
               (2, 2, 9), (5, 4, 9),                                              # 12, 13: a segment
               (0, 0, np.nan), (0, 0, -3e6)]
    # an exact duplicate: the lower index wins wherever both cover
    rc, o = fru.host_render(L, *_one_slot(v, [(3, 4, 5), (0, 1, 2)], 6, 8))
    assert rc == 0 and (o["tri"] == 0).all() and (o["image"] == 2).all()
    # +0 against -0: a tie, the lower index wins; the image keeps the winner's own sign
    rc, o = fru.host_render(L, *_one_slot(v, [(9, 10, 11), (6, 7, 8)], 6, 8))
    assert rc == 0 and o["tri"][0, 2, 2] == 0 and np.signbit(o["image"][0, 2, 2, 0]) and set(np.unique(o["tri"])) == {-1, 0}
    rc, o = fru.host_render(L, *_one_slot(v, [(6, 7, 8), (9, 10, 11)], 6, 8))
    assert rc == 0 and o["tri"][0, 2, 2] == 0 and not np.signbit(o["image"][0, 2, 2, 0])
    # a degenerate triangle covers its whole box (inverDeno = 0: u = v = 0), nothing else
    rc, o = fru.host_render(L, *_one_slot(v, [(12, 12, 13)], 6, 8))
    want = np.full((6, 8), -1)
    want[2:5, 2:6] = 0
    assert rc == 0 and np.array_equal(o["tri"][0], want)
    # a vertex that is not finite, a depth at or below -999999: skipped; a window elsewhere sees its own pixels
    rc, o = fru.host_render(L, *_one_slot(v, [(14, 1, 2), (15, 15, 15), (0, 1, 2)], 6, 8))
    assert rc == 0 and (o["tri"] == 2).all()
    rc, o = fru.host_render(L, *_one_slot(v, [(0, 1, 2)], 6, 8, (15, 3)))
    assert rc == 0 and np.array_equal(o["tri"][0], ref.render(np.asarray(v, np.float32), [(0, 1, 2)], 15, 3, 6, 8)[0])
    assert o["tri"][0, 0, 0] == 0 and o["tri"][0, 5, 7] == -1                    # (15, 3) lies inside the hypotenuse x + y = 19, (22, 8) beyond
    # an origin beyond +-2^20: the slot is written like an unused one
    rc, o = fru.host_render(L, *_one_slot(v, [(0, 1, 2)], 6, 8, ((1 << 20) + 1, 0)))
    assert rc == 0 and (o["tri"] == -1).all() and not o["image"].any()
    rc, o = fru.host_render(L, *_one_slot(v, [(0, 1, 2)], 6, 8, (-(1 << 20), 1 << 20)))
    assert rc == 0 and (o["tri"] == -1).all()                                    # a legal origin, nothing there


def _color_call(forms, seed, cap):
    H, W = draw_ref.frame_size(forms[0])
    V = 200
    face_ind = np.random.RandomState(seed).permutation(65536)[:V].astype(np.int32)
    pos = np.stack([ref.place(fru.color_vertices(seed + s, V, H, W), face_ind) for s in range(cap)])
    slots = np.arange(cap, dtype=np.int32)
    slots[1] = -1
    return pos, slots, face_ind


COLOR_CASES = [("hwc bgr + hwc rgb4", lambda: draw_ref.bgr_forms(2100, 37, 53)[0:2], "bt601"),
               ("bgra padded + chw rgb", lambda: draw_ref.bgr_forms(2100, 37, 53)[2:4], "bt601"),
               ("chw bgr4 padded + roi rgb", lambda: draw_ref.bgr_forms(2100, 37, 53)[4:6], "bt601"),
               ("nv12 pitched odd + nv21 pitched", lambda: [reid_ref.nv12_pitched_odd(2140, 37, 53), draw_ref.yuv_forms(2130, 37, 53)[1]], "bt601"),
               ("i420 + i420 interleaved views, bt709", lambda: draw_ref.yuv_forms(2130, 37, 53)[2:4], "bt709")]


@pytest.mark.parametrize("case", COLOR_CASES, ids=[c[0] for c in COLOR_CASES])
def test_vertex_colors_twin_equals_numpy(L, case):
    _, make, matrix = case
    forms = make()
    before = [f["buf"].copy() for f in forms]
    yuv = forms[0]["color"] not in ("bgr", "rgb")
    cap = 5                                                                      # q = 2: slot 4 lies beyond N * q
    pos, slots, face_ind = _color_call(forms, 2200, cap)
    table = draw_util.table_of(forms, [f["buf"].ctypes.data for f in forms])
    rc, got = fru.host_colors(L, table, yuv, 2, pos, slots, face_ind, yuv_ref.COEF[matrix] if yuv else None)
    assert rc == 0, L.cp_last_error()
    want = ref.vertex_colors([reid_ref.picture(f, matrix) for f in forms], pos, slots, face_ind)
    assert fru.same_bits(got, want) and all(np.array_equal(f["buf"], b) for f, b in zip(forms, before))
    assert not got[1].any() and not got[4].any() and got[0].any() and got[3].any() and not got[0, :2].any()
    assert got.min() >= 0 and got.max() <= 255 and np.array_equal(got, np.round(got))


def test_vertex_colors_twin_on_p010(L):
    H, W, matrix = 36, 52, "bt2020-limited"
    planes_list = [tuple(np.ascontiguousarray(p) for p in ysr.random_planes(2300 + n, "p010", H, W)) for n in range(2)]
    table = fru.surface_table(planes_list, "p010", lambda p: p.ctypes.data)
    V = 200
    face_ind = np.arange(V, dtype=np.int32) * 300
    pos = np.stack([ref.place(fru.color_vertices(2310 + s, V, H, W), face_ind) for s in range(2)])
    slots = np.asarray([3, 9], np.int32)
    rc, got = fru.host_colors(L, table, True, 2, pos, slots, face_ind, ysr.COEF[matrix])
    assert rc == 0, L.cp_last_error()
    want = ref.vertex_colors([ysr.frame_to_bgr(p, "p010", matrix) for p in planes_list], pos, slots, face_ind)
    assert fru.same_bits(got, want) and got.any()


def test_round_half_to_even_and_the_clamp(L):
    form = draw_ref.bgr_forms(2400, 7, 5)[0]
    pic = reid_ref.picture(form)
    xs = [0.5, 1.5, 2.5, 3.5, -0.5, -7.0, 4.49, 4.5, 99.0, 2.0]                   # -> 0, 2, 2, 4, 0, 0, 4, 4, 4, 2
    v = np.asarray([(x, 6.5 if k % 2 else 5.5, 0.0) for k, x in enumerate(xs)], np.float32)     # y -> 6, 6 (6.5 is clamped to 6)
    face_ind = np.arange(len(xs), dtype=np.int32)
    table = draw_util.table_of([form], [form["buf"].ctypes.data])
    rc, got = fru.host_colors(L, table, False, 1, ref.place(v, face_ind)[None], np.asarray([0], np.int32), face_ind)
    assert rc == 0, L.cp_last_error()
    assert np.array_equal(got[0], pic[6, [0, 2, 2, 4, 0, 0, 4, 4, 4, 2]].astype(np.float32))


def test_grid_triangles_on_a_hand_made_mask():
    from centerpose_amd import face
    cell = lambda r, c: r * 256 + c
    #   . A B      rows 10..12, columns 20..22: the block (10..11, 21..22) and the block (11..12, 20..21) are complete
    #   C D E
    #   F G .
    ind = [cell(10, 21), cell(10, 22), cell(11, 20), cell(11, 21), cell(11, 22), cell(12, 20), cell(12, 21), cell(200, 5), cell(11, 21)]
    A, B, C, D, E, F, G_ = 0, 1, 2, 3, 4, 5, 6
    tri = face.grid_triangles(np.asarray(ind))
    assert tri.dtype == np.int32 and tri.tolist() == [[A, D, B], [D, E, B], [C, F, D], [F, G_, D]]      # (tl, bl, tr), (bl, br, tr); D's first entry
    assert face.grid_triangles(ref.block_ind(24)).shape == (2 * 23 * 23, 3)
    with pytest.raises(ValueError, match="no 2 x 2 block"):
        face.grid_triangles([cell(0, 0), cell(0, 1), cell(1, 0), cell(5, 5)])
    with pytest.raises(ValueError, match="0..65535"):
        face.grid_triangles([0, 1, 65536])


def test_the_launch_checks(L):
    assert L.cp_face_render_scratch_bytes(3, 40, 48, 1058) == 3 * 40 * 48 * 8
    for bad in ((0, 8, 8, 1), (257, 8, 8, 1), (1, 0, 8, 1), (1, 8, 4097, 1), (1, 8, 8, 0), (1, 8, 8, (1 << 22) + 1), (16, 4096, 4096, 1)):
        assert L.cp_face_render_scratch_bytes(*bad) == 0, bad
    assert L.cp_face_render_scratch_bytes(15, 4096, 4096, 1 << 22) == 15 * 4096 * 4096 * 8           # 15 * 2^27 < 2^31
    v = np.zeros((4, 3), np.float32)
    args = lambda **k: _one_slot(v, k.pop("tris", [(0, 1, 2)]), k.pop("h", 4), k.pop("w", 4))
    ok = args()

    def refused(text, call):
        rc = call()
        assert rc == 1 and text in L.cp_last_error().decode(), (text, rc, L.cp_last_error())

    refused("triangle 0 names vertex 4", lambda: fru.host_render(L, *args(tris=[(0, 1, 4)]))[0])
    refused("triangle 1 names vertex -1", lambda: fru.host_render(L, *args(tris=[(0, 1, 2), (0, -1, 2)]))[0])
    refused("face_ind[1]", lambda: fru.host_render(L, ok[0], ok[1], np.asarray([0, 65536, 2, 3]), *ok[3:])[0])
    refused("bytes of scratch", lambda: fru.host_render(L, *ok, scratch_bytes=4 * 4 * 8 - 1)[0])
    refused("with 2 channels", lambda: raw(C=2, attrs=False))
    p = ok[0].ctypes.data
    refused("attribute channels", lambda: raw(C=5))
    refused("attribute channels", lambda: raw(C=0))
    refused("capacity", lambda: raw(cap=0))
    refused("capacity", lambda: raw(cap=257))
    refused("vertices", lambda: raw(V=2))
    refused("vertices", lambda: raw(V=65537))
    refused("triangles", lambda: raw(T=0))
    refused("triangles", lambda: raw(T=(1 << 22) + 1))
    refused("window", lambda: raw(h=0))
    refused("window", lambda: raw(w=4097))
    refused("2^31", lambda: raw(cap=16, h=4096, w=4096))
    for k in (0, 1, 3, 5, 7, 12, 14, 15):
        refused("null pointer", lambda: raw(null=k))
    # the colour twins
    refused("capacity", lambda: L.cp_face_vertex_colors_host(p, 1, p, p, 0, p, 3, p))
    refused("frames", lambda: L.cp_face_vertex_colors_host(p, 0, p, p, 2, p, 3, p))
    refused("frames", lambda: L.cp_face_vertex_colors_host(p, 3, p, p, 2, p, 3, p))
    refused("vertices", lambda: L.cp_face_vertex_colors_host(p, 1, p, p, 2, p, 2, p))
    refused("null pointer", lambda: L.cp_face_vertex_colors_host(p, 1, None, p, 2, p, 3, p))
    refused("null pointer", lambda: L.cp_face_vertex_colors_yuv_host(None, 1, None, p, p, 2, p, 3, p))
    refused("null coef", lambda: L.cp_face_vertex_colors_yuv_host(p, 1, None, p, p, 2, p, 3, p))
    form = draw_ref.bgr_forms(2500, 7, 5)[0]
    table = draw_util.table_of([form], [form["buf"].ctypes.data])
    table["H"] = 0
    refused("bad size", lambda: fru.host_colors(L, table, False, 1, ok[0], ok[1], np.arange(3))[0])


def raw(cap=1, V=4, T=1, h=4, w=4, C=1, attrs=True, null=None):
    """cp_face_render_host with raw sizes over buffers large enough for the defaults (a refused call touches nothing)."""
    L = draw_util.lib_built()
    buf = np.zeros(65536 * 3, np.float32)
    a = [buf.ctypes.data, buf.ctypes.data, cap, buf.ctypes.data, V, buf.ctypes.data, T, buf.ctypes.data, h, w, buf.ctypes.data if attrs else None,
         C, buf.ctypes.data, 1 << 40, buf.ctypes.data, buf.ctypes.data]
    if null is not None:
        a[null] = None
    return L.cp_face_render_host(*a)


def test_the_tables_are_checked():
    from centerpose_amd import face
    ind = ref.block_ind(4)
    for bad, text in (([[0, 1]], r"\[T, 3\]"), (np.zeros((0, 3)), r"\[T, 3\]"), ([0, 1, 2], r"\[T, 3\]"), ([[0, 1, 16]], "0..15"), ([[0, -1, 2]], "0..15"),
                      ([[0, 1.5, 2]], "whole numbers"), ([[0, np.nan, 2]], "whole numbers"), ([["a", "b", "c"]], "whole numbers")):
        with pytest.raises(ValueError, match=text):
            face.check_triangles(bad, len(ind))
    assert face.check_triangles([[0.0, 1.0, 15.0]], 16).tolist() == [[0, 1, 15]]
    for bad, text in (([0, 1], "one row"), ([[0, 1, 2]], "one row"), ([0, 1, 2.5], "whole numbers"), ([0, 1, -1], "0..65535")):
        with pytest.raises(ValueError, match=text):
            face.check_face_ind(bad)
    tri = face.grid_triangles(ind)
    with pytest.raises(ValueError, match="capacity"):
        face.FaceRenderer(ind, tri, 0)
    with pytest.raises(ValueError, match="capacity"):
        face.FaceRenderer(ind, tri, 257)
    with pytest.raises(ValueError, match="0..15"):
        face.FaceRenderer(ind, tri + 1, 2)
    with pytest.raises(ValueError, match="no CPU fallback"):
        face.FaceRenderer(ind, tri, 2, device="cpu")


def test_triangles_from_a_text_file(tmp_path):
    from centerpose_amd import face
    path = tmp_path / "triangles.txt"
    np.savetxt(path, np.asarray([[0, 1, 2], [2, 1, 3]], np.float64))
    assert face.check_triangles(str(path), 4).tolist() == [[0, 1, 2], [2, 1, 3]]
    assert face.check_triangles(path, 4).dtype == np.int32
