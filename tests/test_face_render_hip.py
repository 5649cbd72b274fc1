"""GPU: the mesh rasteriser on the device -- cp_face_render_f32 (face_render_clear_kernel, face_render_raster_kernel,
face_render_resolve_kernel) and cp_face_vertex_colors[_yuv]_f32 against their host twins bit for bit over whole guarded buffers (keys,
tri, image; colours), against the recording of the reference's renderer, and through face.FaceRenderer / FaceAligner.renderer.

Shapes: the smallest at which the kernels can go wrong -- a 1 x 1 window with one triangle, the recording's 40 x 48 with T = 1058
(several blocks), 33 x 65 (ragged against a wave) with cap = 3, one unused slot and three origins, and a 64 x 64 window under one triangle
that covers it whole together with 500 one-pixel triangles: both paths of the raster kernel (a lane walks a box of at most 16 pixels,
the block walks a larger one together) and the ties between them.  DESIGN.md section 4.17."""
import ctypes

import numpy as np
import pytest
import torch

import draw_ref
import draw_util
import face_ref
import face_render_ref as ref
import face_render_util as fru
import reid_ref
import yuv_ref
import yuv_surface_ref as ysr

pytestmark = pytest.mark.gpu


def _dev(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()


def _device_render(L, pos, slots, face_ind, triangles, origin, h, w, attrs=None):
    """-> dict like face_render_util.host_render's, from the device; the guards behind the keys, tri and image are checked."""
    from centerpose_amd import _lib
    cap, V, T = len(slots), len(face_ind), len(triangles)
    C = 1 if attrs is None else attrs.shape[2]
    a = [_dev(pos, np.float32), _dev(slots, np.int32), _dev(face_ind, np.int32), _dev(triangles, np.int32), _dev(origin, np.int32)]
    at = None if attrs is None else _dev(attrs, np.float32)
    host = fru.outputs(cap, h, w, C)
    out = {k: torch.from_numpy(v.view(np.int64) if k == "keys" else v).cuda() for k, v in host.items()}
    rc = L.cp_face_render_f32(a[0].data_ptr(), a[1].data_ptr(), cap, a[2].data_ptr(), V, a[3].data_ptr(), T, a[4].data_ptr(), h, w,
                              None if at is None else at.data_ptr(), C, out["keys"].data_ptr(), cap * h * w * 8, out["tri"].data_ptr(),
                              out["image"].data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0, L.cp_last_error()
    assert L.cp_last_kernel() == b"face_render_clear_kernel+face_render_raster_kernel+face_render_resolve_kernel"
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["keys"] = got["keys"].view(np.uint64)
    assert fru.guards_intact(got, cap, h, w, C)
    return fru.shaped(got, cap, h, w, C)


def _same(dev, host):
    return np.array_equal(dev["keys"], host["keys"]) and np.array_equal(dev["tri"], host["tri"]) and fru.same_bits(dev["image"], host["image"])


def _both(L, *args):
    rc, host = fru.host_render(L, *args)
    assert rc == 0, L.cp_last_error()
    dev = _device_render(L, *args)
    assert _same(dev, host)
    return dev


def test_the_recording_on_the_device():
    """40 x 48, T = 1058 (five blocks of triangles), the three recorded meshes and an unused slot; twice: the same bytes."""
    L = draw_util.lib_loaded()
    g = fru.golden()
    cases = [fru.golden_case(g, k) for k in range(3)]
    _, face_ind, tri, _, h, w, _ = cases[0]
    pos = np.stack([c[0] for c in cases] + [cases[0][0]])
    slots = np.asarray([5, 0, 7, -1], np.int32)
    origin = np.concatenate([g["origin"], [[0, 0]]]).astype(np.int32)
    colors = np.stack([c[6] for c in cases] + [cases[0][6]])
    depth = _both(L, pos, slots, face_ind, tri, origin, h, w)
    tex = _both(L, pos, slots, face_ind, tri, origin, h, w, colors)
    for k in range(3):
        assert np.array_equal(depth["tri"][k], g["tri"][k]) and np.array_equal(tex["tri"][k], g["tri"][k])
        assert fru.same_bits(depth["image"][k], g["depth"][k]) and fru.same_bits(tex["image"][k], g["texture"][k])
    assert (tex["tri"][3] == -1).all() and not tex["image"][3].any()
    again = _device_render(L, pos, slots, face_ind, tri, origin, h, w, colors)
    assert all(again[k].tobytes() == tex[k].tobytes() for k in ("keys", "tri", "image"))


def test_one_triangle_in_a_one_pixel_window():
    L = draw_util.lib_loaded()
    v = np.asarray([(6.5, 2.5, 3.0), (9.5, 2.5, 4.0), (6.5, 5.5, -1.0), (0, 0, 0)], np.float32)
    face_ind = np.asarray([65535, 0, 300, 7], np.int32)
    for origin, want in (((7, 3), 0), ((9, 5), -1), ((6, 2), -1)):
        dev = _both(L, ref.place(v, face_ind)[None], np.asarray([0], np.int32), face_ind, np.asarray([(0, 1, 2)], np.int32),
                    np.asarray([origin], np.int32), 1, 1)
        assert dev["tri"].tolist() == [[[want]]] and dev["image"].tolist() == [[[[2.0 if want == 0 else 0.0]]]]


@pytest.mark.parametrize("C", [0, 3, 4], ids=["z", "c3", "c4"])
def test_ragged_window_three_slots_three_origins(C):
    """33 x 65: rows that end inside a wave; cap = 3 with slot 1 unused; degenerate triangles, duplicates, +-0, vertices that are not
    finite or +-1e30, triangles far larger than the window (the block's path) among small ones (the lane's)."""
    L = draw_util.lib_loaded()
    args = fru.fuzz_call(3100 + C, C, 33, 65)
    dev = _both(L, *args)
    rt, ri = ref.render_slots(*args)
    assert np.array_equal(dev["tri"], rt) and fru.same_bits(dev["image"], ri)
    assert (dev["tri"][1] == -1).all() and (dev["tri"][0] >= 0).mean() > 0.5


def _big_and_small(seed, n_small=500, side=64):
    """One triangle over the whole side x side window at depth 5, in the middle of the table, and n_small triangles of one pixel each at
    depths below, at and above 5: where a small one ties with the large one the lower index wins, whichever path walked it."""
    r = np.random.RandomState(seed)
    cells = r.permutation(side * side)[:n_small]
    v, tris = [(-10.0, -10.0, 5.0), (3.0 * side, -10.0, 5.0), (-10.0, 3.0 * side, 5.0)], []
    for k, cell in enumerate(cells):
        x, y, z = float(cell % side), float(cell // side), (4.0, 5.0, 6.0)[k % 3]
        v += [(x - 0.3, y - 0.3, z), (x + 0.6, y - 0.3, z), (x - 0.3, y + 0.6, z)]
        tris.append((3 * k + 3, 3 * k + 4, 3 * k + 5))
    tris.insert(n_small // 2, (0, 1, 2))
    return np.asarray(v, np.float32), np.asarray(tris, np.int32), cells


def test_a_window_filling_triangle_among_one_pixel_triangles():
    L = draw_util.lib_loaded()
    v, tris, cells = _big_and_small(3200)
    face_ind = np.random.RandomState(3201).permutation(65536)[:len(v)].astype(np.int32)
    dev = _both(L, ref.place(v, face_ind)[None], np.asarray([2], np.int32), face_ind, tris, np.zeros((1, 2), np.int32), 64, 64)
    big = 250
    want = np.full(64 * 64, big, np.int32)
    for k, cell in enumerate(cells):
        i = k if k < big else k + 1                                               # the small triangle's place in the table
        if k % 3 == 2 or (k % 3 == 1 and i < big):                                # nearer, or as near and earlier
            want[cell] = i
    assert np.array_equal(dev["tri"][0].reshape(-1), want)
    assert set(np.unique(dev["image"])) == {5.0, 6.0}


def _colors_on_device(L, table_dev_host, table_dev, yuv, N, pos, slots, face_ind, coef=None):
    from centerpose_amd import _lib
    cap, V = len(slots), len(face_ind)
    a = [_dev(pos, np.float32), _dev(slots, np.int32), _dev(face_ind, np.int32)]
    out = torch.from_numpy(np.full(cap * V * 3 + fru.GUARD, np.nan, np.float32)).cuda()
    tail = (a[0].data_ptr(), a[1].data_ptr(), cap, a[2].data_ptr(), V, out.data_ptr(), _lib.stream())
    if yuv:
        rc = L.cp_face_vertex_colors_yuv_f32(table_dev.data_ptr(), table_dev_host.ctypes.data, N, (ctypes.c_int * 6)(*coef), *tail)
    else:
        rc = L.cp_face_vertex_colors_f32(table_dev.data_ptr(), table_dev_host.ctypes.data, N, *tail)
    torch.cuda.synchronize()
    assert rc == 0, L.cp_last_error()
    got = out.cpu().numpy()
    assert np.isnan(got[cap * V * 3:]).all()
    return got[:cap * V * 3].reshape(cap, V, 3)


COLOR_CASES = [("hwc bgra padded + chw rgb", lambda: draw_ref.bgr_forms(3300, 37, 53)[2:4], "bt601", b"face_vertex_colors_kernel<bgr>"),
               ("nv12 pitched odd + nv21 pitched", lambda: [reid_ref.nv12_pitched_odd(3340, 37, 53), draw_ref.yuv_forms(3330, 37, 53)[1]], "bt601",
                b"face_vertex_colors_kernel<yuv>")]


@pytest.mark.parametrize("case", COLOR_CASES, ids=[c[0] for c in COLOR_CASES])
def test_vertex_colors_equal_the_host_twin(case):
    L = draw_util.lib_loaded()
    _, make, matrix, kernel = case
    forms = make()
    yuv = forms[0]["color"] not in ("bgr", "rgb")
    H, W = draw_ref.frame_size(forms[0])
    V, cap = 300, 5                                                              # two blocks of vertices; q = 2: slot 4 lies beyond N * q
    face_ind = np.random.RandomState(3350).permutation(65536)[:V].astype(np.int32)
    pos = np.stack([ref.place(fru.color_vertices(3360 + s, V, H, W), face_ind) for s in range(cap)])
    slots = np.asarray([0, -1, 2, 3, 4], np.int32)
    coef = yuv_ref.COEF[matrix] if yuv else None
    rc, host = fru.host_colors(L, draw_util.table_of(forms, [f["buf"].ctypes.data for f in forms]), yuv, 2, pos, slots, face_ind, coef)
    assert rc == 0, L.cp_last_error()
    devs = [torch.from_numpy(f["buf"].copy()).cuda() for f in forms]
    table = draw_util.table_of(forms, [d.data_ptr() for d in devs])
    got = _colors_on_device(L, table, torch.from_numpy(table.view(np.uint8).copy()).cuda(), yuv, 2, pos, slots, face_ind, coef)
    assert fru.same_bits(got, host) and L.cp_last_kernel() == kernel
    assert all(np.array_equal(d.cpu().numpy(), f["buf"]) for d, f in zip(devs, forms))                  # the frames are only read
    assert fru.same_bits(got, ref.vertex_colors([reid_ref.picture(f, matrix) for f in forms], pos, slots, face_ind))
    assert not got[1].any() and not got[4].any() and got[0].any() and got[3].any()


def test_vertex_colors_on_p010():
    L = draw_util.lib_loaded()
    H, W, matrix = 36, 52, "bt2020-limited"
    planes_list = [tuple(np.ascontiguousarray(p) for p in ysr.random_planes(3400 + n, "p010", H, W)) for n in range(2)]
    V = 200
    face_ind = np.arange(V, dtype=np.int32) * 300
    pos = np.stack([ref.place(fru.color_vertices(3410 + s, V, H, W), face_ind) for s in range(2)])
    slots = np.asarray([3, 9], np.int32)
    rc, host = fru.host_colors(L, fru.surface_table(planes_list, "p010", lambda p: p.ctypes.data), True, 2, pos, slots, face_ind, ysr.COEF[matrix])
    assert rc == 0, L.cp_last_error()
    devs = {id(p): torch.from_numpy(p.view(np.int16)).cuda() for planes in planes_list for p in planes}
    table = fru.surface_table(planes_list, "p010", lambda p: devs[id(p)].data_ptr())
    got = _colors_on_device(L, table, torch.from_numpy(table.view(np.uint8).copy()).cuda(), True, 2, pos, slots, face_ind, ysr.COEF[matrix])
    assert fru.same_bits(got, host) and got.any() and L.cp_last_kernel() == b"face_vertex_colors_kernel<surfaces>"


def test_face_renderer_on_a_hand_made_pos():
    """face.FaceRenderer without a PRNet plan: the recording's mesh in two slots through render and vertex_colors, and every ValueError."""
    from centerpose_amd import face
    L = draw_util.lib_loaded()
    g = fru.golden()
    pos0, face_ind, tri, _, h, w, colors0 = fru.golden_case(g, 0)
    pos2 = fru.golden_case(g, 2)[0]
    r = face.FaceRenderer(face_ind, tri, 3)
    assert r.capacity == 3 and r.triangles.shape == (1058, 3)
    pos = _dev(np.stack([pos0, pos0, pos2]), np.float32)
    slots = _dev([0, -1, 4], np.int32)
    origin = _dev([[0, 0], [0, 0], g["origin"][2]], np.int32)
    out = r.render(pos, slots=slots, size=(h, w), origin=origin)
    assert isinstance(out, face.FaceRender) and out.tri.dtype == torch.int32 and tuple(out.image.shape) == (3, h, w, 1)
    tri_out, image = out.tri.cpu().numpy(), out.image.cpu().numpy()
    assert np.array_equal(tri_out[0], g["tri"][0]) and np.array_equal(tri_out[2], g["tri"][2]) and (tri_out[1] == -1).all()
    assert fru.same_bits(image[0], g["depth"][0]) and fru.same_bits(image[2], g["depth"][2])
    # origin=None: every window at (0, 0); a FaceResult brings its own slots; attrs from vertex_colors
    result = face.FaceResult(pos, None, slots, None, None)
    zero = r.render(result, size=(h, w))
    assert np.array_equal(zero.tri[0].cpu().numpy(), g["tri"][0])
    form = draw_ref.bgr_forms(3500, 64, 72)[0]
    frame = torch.from_numpy(draw_ref.numpy_views(form["buf"], form)[0].copy()).cuda()
    colors = r.vertex_colors([frame], result)
    assert tuple(colors.shape) == (3, len(face_ind), 3) and colors.dtype == torch.float32
    want = ref.vertex_colors([reid_ref.picture(form)], pos.cpu().numpy(), [0, -1, 4], face_ind)
    assert fru.same_bits(colors.cpu().numpy(), want) and want[2].any() and not want[1].any()
    tex = r.render(result, size=(h, w), origin=origin, attrs=colors)
    rc, host = fru.host_render(L, pos.cpu().numpy(), [0, -1, 4], face_ind, tri, origin.cpu().numpy(), h, w, want)
    assert rc == 0 and np.array_equal(tex.tri.cpu().numpy(), host["tri"]) and fru.same_bits(tex.image.cpu().numpy(), host["image"])
    # the refusals of the Python layer
    for call, text in ((lambda: r.render(face.FaceResult(None, None, slots, None, None), size=(h, w)), "no position maps"),
                       (lambda: r.render(result, slots=slots, size=(h, w)), "brings its own"),
                       (lambda: r.render(pos, size=(h, w)), "needs slots="),
                       (lambda: r.render(pos.cpu(), slots=slots, size=(h, w)), "pos must be"),
                       (lambda: r.render(pos.cpu().numpy(), slots=slots, size=(h, w)), "host array"),
                       (lambda: r.render(pos.double(), slots=slots, size=(h, w)), "pos must be"),
                       (lambda: r.render(pos[:2], slots=slots, size=(h, w)), "pos must be"),
                       (lambda: r.render(pos, slots=slots.long(), size=(h, w)), "slots must be"),
                       (lambda: r.render(pos, slots=slots), "size must be"),
                       (lambda: r.render(pos, slots=slots, size=(0, w)), "size must be"),
                       (lambda: r.render(pos, slots=slots, size=(h, 4097)), "size must be"),
                       (lambda: face.FaceRenderer(face_ind, tri, 16).render(torch.zeros((16, 256, 256, 3), device="cuda"),
                                                                            slots=torch.zeros(16, dtype=torch.int32, device="cuda"),
                                                                            size=(4096, 4096)), "2\\^31"),
                       (lambda: r.render(pos, slots=slots, size=(h, w), origin=origin[:2]), "origin must be"),
                       (lambda: r.render(pos, slots=slots, size=(h, w), origin=origin.cpu().numpy()), "host array"),
                       (lambda: r.render(pos, slots=slots, size=(h, w), attrs=colors[:, :5]), "attrs must be"),
                       (lambda: r.render(pos, slots=slots, size=(h, w), attrs=torch.zeros((3, len(face_ind), 5), device="cuda")), "attrs must be"),
                       (lambda: r.vertex_colors([frame.cpu().numpy()], result), "host arrays"),
                       (lambda: r.vertex_colors([frame] * 4, result), "4 frames"),
                       (lambda: r.vertex_colors([frame], face.FaceResult(None, None, slots, None, None)), "no position maps")):
        with pytest.raises(ValueError, match=text):
            call()


def test_face_aligner_renderer():
    """FaceAligner.renderer reuses the aligner's face_ind and capacity: the maps of one align call rendered where they lie."""
    import face_pose_util as fpu
    import os
    from centerpose_amd import face, synth
    L = draw_util.lib_loaded()
    g = fpu.golden()
    prn = dict(np.load(os.path.join(fru.ROOT, "tests", "golden", "prn_maps.npz")))
    uv = np.loadtxt(os.path.join(fru.ROOT, "tests", "golden", "prn_uv_kpt_ind.txt")).astype(np.int32)
    sd = synth.make_state_dict("prnet", seed=int(prn["seed"]))
    with pytest.raises(ValueError, match="face_ind="):
        face.FaceAligner(sd, uv, capacity=2).renderer([[0, 1, 2]])
    al = face.FaceAligner(sd, uv, capacity=2, face_ind=g["face_ind"], canonical_vertices=g["canonical_vertices"])
    V = len(g["face_ind"])
    base = np.random.RandomState(3600).randint(0, V - 3, 2000)
    tri = np.stack([base, base + 1, base + 2], 1)
    r = al.renderer(tri)
    assert r.capacity == 2 and np.array_equal(r.face_ind, al.face_ind) and r.device == al.device
    pic = np.ascontiguousarray((face_ref.make_input(70, 96, 128)[::-1].transpose(1, 2, 0) * 255).round().astype(np.uint8))
    frame = torch.from_numpy(pic).cuda()
    rows = torch.from_numpy(np.stack([np.stack([face_ref.joints_row(30, 90, 20, 75)])]).astype(np.float32)).cuda()
    result = al.align([frame], rows=rows)
    colors = r.vertex_colors([frame], result)
    out = r.render(result, size=(96, 128), attrs=colors)
    torch.cuda.synchronize()
    pos, slots = result.pos.cpu().numpy(), result.slots.cpu().numpy()
    assert slots.tolist() == [0, -1]
    want = ref.vertex_colors([pic], pos, slots, al.face_ind)
    assert fru.same_bits(colors.cpu().numpy(), want)
    rc, host = fru.host_render(L, pos, slots, al.face_ind, tri, np.zeros((2, 2), np.int32), 96, 128, want)
    assert rc == 0 and np.array_equal(out.tri.cpu().numpy(), host["tri"]) and fru.same_bits(out.image.cpu().numpy(), host["image"])
    assert (host["tri"][0] >= 0).any() and (host["tri"][1] == -1).all()
