"""GPU: the face stage on the device -- cp_face_select, the crop kernels and cp_face_restore_f32 bit for bit against their host
twins (and the NumPy rules of tests/face_ref.py) over whole guarded buffers, every launch of the `prnet` plan per element against
float64 (tests/face_util.py), Engine("prnet") against the recorded float64 maps, the plan file through plan.py and the C runtime,
and FaceAligner.align end to end.  The crop rule is a closed-form statement of the reference's pipeline, not pinned to a recording of
skimage.

Measured on the MI355X: the float32 plan lies 1.46e-5 (64 x 64, in full) and 7.15e-5 (256 x 256 border lines, every 8th pixel, landmark
cells) from the recorded float64 maps (bar 1e-3; the module's own float32 / float64 gap is 5.4e-5); the worst error / tolerance of a
single launch is 0.099 (2 x 32 x 32) and 0.106 (2 x 64 x 96); end to end the landmarks are 1.5e-3 .. 9.3e-3 px off (bar 0.10 .. 0.13 px).
DESIGN.md section 4.15."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import draw_util
import face_ref
import face_util
import yuv_ref
import yuv_surface_ref as ysr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p
CROP = 3 * 256 * 256
GUARD = face_util.GUARD


def _stream():
    from centerpose_amd import _lib
    return _lib.stream()


def _tables(forms):
    devs = [torch.from_numpy(f["buf"].copy()).cuda() for f in forms]
    table = draw_util.table_of(forms, [d.data_ptr() for d in devs])
    return devs, table, torch.from_numpy(table.view(np.uint8).copy()).cuda()


def _device_select(L, cand, boxes, cap, **rule):
    N, M = cand.shape[:2]
    c = torch.from_numpy(np.ascontiguousarray(cand, np.float32)).cuda()
    slots = torch.full((cap + GUARD,), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((N + GUARD,), -7, dtype=torch.int32, device="cuda")
    xform = torch.full((3 * cap + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    rc = L.cp_face_select(N, VP(c.data_ptr()), M, face_util.rule_struct(boxes, **rule).ctypes.data_as(VP), cap, VP(slots.data_ptr()),
                          VP(counts.data_ptr()), VP(xform.data_ptr()), _stream())
    torch.cuda.synchronize()
    slots, counts, xform = slots.cpu().numpy(), counts.cpu().numpy(), xform.cpu().numpy()
    assert (slots[cap:] == -7).all() and (counts[N:] == -7).all() and np.isnan(xform[3 * cap:]).all()       # nothing behind the arrays
    return rc, slots[:cap], counts[:N], xform[:3 * cap].reshape(cap, 3)


def _device_crop(L, table, table_dev, yuv, N, M, slots, xform, matrix="bt601"):
    cap = len(slots)
    s = torch.from_numpy(np.ascontiguousarray(slots, np.int32)).cuda()
    x = torch.from_numpy(np.ascontiguousarray(xform, np.float32)).cuda()
    out = torch.full((cap * CROP + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    if yuv:
        coef = (ctypes.c_int * 6)(*ysr.COEF[matrix])
        rc = L.cp_face_crop_yuv_frames_f32(VP(table_dev.data_ptr()), table.ctypes.data_as(VP), N, coef, M, VP(s.data_ptr()), VP(x.data_ptr()), cap,
                                           VP(out.data_ptr()), _stream())
    else:
        rc = L.cp_face_crop_frames_f32(VP(table_dev.data_ptr()), table.ctypes.data_as(VP), N, M, VP(s.data_ptr()), VP(x.data_ptr()), cap,
                                       VP(out.data_ptr()), _stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


# ---------------------------------------------------------------- 1. select
@pytest.mark.parametrize("boxes", [False, True])
def test_select_kernel_equals_its_host_twin(boxes):
    L = draw_util.lib_loaded()
    cand = face_ref.select_cases(boxes)                        # N = 3, M = 7
    for cap, want in face_ref.SELECT_EXPECT.items():
        rc, hs, hc, hx = face_util.host_select(L, cand, boxes, cap)
        assert rc == 0 and hs.tolist() == want
        rc, ds, dc, dx = _device_select(L, cand, boxes, cap)
        assert rc == 0, L.cp_last_error()
        assert ds.tolist() == want and dc.tolist() == hc.tolist() == face_ref.SELECT_COUNTS and face_util.same_bits(dx, hx)
        assert face_util.same_bits(dx, face_ref.select(cand, boxes, face_ref.VIS, cap)[2])
    assert L.cp_last_kernel() == (b"face_select_kernel<boxes>" if boxes else b"face_select_kernel<rows>")


@pytest.mark.parametrize("boxes", [False, True])
def test_select_kernel_beyond_one_wave_of_candidates(boxes):
    """M = 150 candidates per frame: three trips of the wave, ranks carried from trip to trip."""
    L = draw_util.lib_loaded()
    r = np.random.RandomState(9)
    cand = np.zeros((2, 150, 5 if boxes else 56), np.float32)
    if boxes:
        cand[..., 0:2] = r.uniform(-30, 150, (2, 150, 2))
        cand[..., 2:4] = cand[..., 0:2] + r.uniform(-5, 60, (2, 150, 2))
    else:
        cand[..., 5:15] = r.uniform(-30, 200, (2, 150, 10))
        cand[0, 7, 9] = np.nan
    cand[..., 4] = r.choice([0.1, 0.3, 0.31, 0.9, np.nan], (2, 150))
    for cap, expand, min_size in ((2, 1.6, 1), (64, 1.6, 1), (256, 0.5, 3)):
        want_s, want_c, want_x = face_ref.select(cand, boxes, face_ref.VIS, cap, expand, min_size)
        rc, hs, hc, hx = face_util.host_select(L, cand, boxes, cap, expand=expand, min_size=min_size)
        assert rc == 0 and np.array_equal(hs, want_s) and np.array_equal(hc, want_c) and 10 < want_c.min() < 150
        rc, ds, dc, dx = _device_select(L, cand, boxes, cap, expand=expand, min_size=min_size)
        assert rc == 0 and np.array_equal(ds, want_s) and np.array_equal(dc, want_c) and face_util.same_bits(dx, want_x)


# ---------------------------------------------------------------- 2. crops
CASES = face_ref.crop_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_crop_kernels_equal_their_host_twins_bit_for_bit(case):
    L = draw_util.lib_loaded()
    name, forms, matrix = case
    boxes, cap = face_ref.case_candidates(forms)
    rc, slots, counts, xform = face_util.host_select(L, boxes, True, cap)
    assert rc == 0
    rc, host = face_util.host_crop(L, forms, 9, slots, xform, matrix)
    assert rc == 0
    devs, table, table_dev = _tables(forms)
    yuv = face_util.is_yuv(forms)
    rc, dev = _device_crop(L, table, table_dev, yuv, len(forms), 9, slots, xform, matrix)
    assert rc == 0, L.cp_last_error()
    assert all(np.array_equal(d.cpu().numpy(), f["buf"]) for d, f in zip(devs, forms))                      # frames unchanged
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))                                        # whole buffer, NaN guard included
    got = dev[:cap * CROP].reshape(cap, 3, 256, 256)
    assert not got[5].any() and not got[9].any() and got[0].any() and got[7].any()
    assert L.cp_last_kernel() == (b"face_crop_kernel<yuv>" if yuv else b"face_crop_kernel<bgr>")


def _surface_tables(planes_list, color):
    """(device tensors kept alive, host table over the host planes, host copy of the device table, the device table)"""
    from centerpose_amd import frames

    def table(address_of):
        rows = []
        for planes in planes_list:
            H, W, y_off, y_row, y_pix, u_off, v_off, c_row, c_pix, fmt = frames.yuv_surface_geometry(
                [p.shape for p in planes], [tuple(s // p.itemsize for s in p.strides) for p in planes], color, [p.dtype for p in planes])
            u_plane, v_plane = (planes[0], planes[0]) if len(planes) == 1 else (planes[1], planes[-1])
            rows.append(frames.YuvSurface(address_of(planes[0]) + y_off, H, W, y_row, y_pix, address_of(u_plane) + u_off, address_of(v_plane) + v_off,
                                          c_row, c_pix, fmt))
        return frames.identity_table(rows, True)
    devs = {}
    for planes in planes_list:
        for p in planes:
            a = np.ascontiguousarray(p)
            devs[id(p)] = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    host = table(lambda p: p.ctypes.data)
    dev = table(lambda p: devs[id(p)].data_ptr())
    return devs, host, dev, torch.from_numpy(dev.view(np.uint8).copy()).cuda()


@pytest.mark.parametrize("color,matrix", [("p010", "bt2020-limited"), ("yuyv", "bt601-full")])
def test_surface_crops_equal_the_host_twin(color, matrix):
    """One 16-bit and one packed surface colour through the general instantiation of the shared sampler (yuv_source.h)."""
    L = draw_util.lib_loaded()
    H, W = 36, 52
    planes_list = [tuple(np.ascontiguousarray(p) for p in ysr.random_planes(1500 + n, color, H, W)) for n in range(2)]
    devs, host_table, dev_table, table_dev = _surface_tables(planes_list, color)
    boxes = np.stack([np.stack([face_ref.box_of(*b) for b in face_ref.crop_boxes(H, W)]) for _ in range(2)]).astype(np.float32)
    cap = 20
    rc, slots, counts, xform = face_util.host_select(L, boxes, True, cap)
    assert rc == 0 and counts.tolist() == [9, 9]
    out = np.full(cap * CROP + GUARD, np.nan, np.float32)
    coef = (ctypes.c_int * 6)(*ysr.COEF[matrix])
    rc = L.cp_face_crop_yuv_frames_host(host_table.ctypes.data_as(VP), 2, coef, 9, slots.ctypes.data_as(VP), np.ascontiguousarray(xform).ctypes.data_as(VP),
                                        cap, out.ctypes.data_as(VP))
    assert rc == 0, L.cp_last_error()
    rc, dev = _device_crop(L, dev_table, table_dev, True, 2, 9, slots, xform, matrix)
    assert rc == 0, L.cp_last_error()
    assert np.array_equal(dev.view(np.uint32), out.view(np.uint32)) and L.cp_last_kernel() == b"face_crop_kernel<surfaces>"
    # ... and the twin is the NumPy rule on the converted picture
    pics = [ysr.frame_to_bgr(p, color, matrix) for p in planes_list]
    assert face_util.same_bits(out[:cap * CROP].reshape(cap, 3, 256, 256), face_ref.crops(pics, slots, xform, 9))


# ---------------------------------------------------------------- 3. the plan
@functools.lru_cache(maxsize=None)
def _golden():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "prn_maps.npz")))
    g["uv"] = np.loadtxt(os.path.join(ROOT, "tests", "golden", "prn_uv_kpt_ind.txt")).astype(np.int32)
    return g


@functools.lru_cache(maxsize=None)
def _sd():
    from centerpose_amd import synth
    return synth.make_state_dict("prnet", seed=int(_golden()["seed"]))


@pytest.mark.parametrize("B,H,W", [(2, 32, 32), (2, 64, 96)])
def test_every_launch_of_the_plan_per_element_against_float64(B, H, W):
    """Launch by launch: the inputs a launch reads on the device, evaluated in float64 from the launch record alone, against what it
    wrote -- every element of the output storage view, padding channels included.  32 x 32 has a 1 x 1 bottleneck where every 4 x 4
    tap but one is padding; 64 x 96 is not square."""
    from centerpose_amd import engine
    eng = engine.Engine("prnet", _sd(), B, H, W, use_graph=False)
    assert len(eng.launches) == 53
    x = torch.stack([torch.from_numpy(face_ref.make_input(50 + b, H, W)) for b in range(B)]).cuda()
    eng.input.copy_(x)
    worst = 0.0
    for kind, name, _, l in eng.launches:
        before = {id(t): t.detach().cpu().clone() for t in l.tensors if t is not None}
        l.run()
        torch.cuda.synchronize()
        got = l.out.detach().cpu().double()
        want, tol = face_util.conv_launch_f64(l, lambda t: before[id(t)])
        assert not torch.isnan(want).any(), name
        err = (got - want).abs()
        bad = err > tol
        assert not bad.any(), "%s: %d elements beyond their tolerance, worst %.3e (tolerance %.3e)" % (
            name, int(bad.sum()), float(err[bad].max()), float(tol[bad].min()))
        worst = max(worst, float((err / tol.clamp_min(1e-30)).max()))
    print("prnet %dx%dx%d: worst error / tolerance over all launches %.3f" % (B, H, W, worst))
    want = face_ref.net(_sd(), x.cpu().double())
    err = float((eng.outputs[0].cpu().double() - want).abs().max())
    print("prnet %dx%dx%d: plan vs float64 statement %.3e" % (B, H, W, err))
    assert err < 1e-3


def test_plan_meets_the_recorded_maps():
    """The 64 x 64 maps in full and the 256 x 256 map's border lines, every 8th pixel and landmark cells: 1e-3 absolute, the project's
    bar for a sigmoid map."""
    from centerpose_amd import engine
    g = _golden()
    uv = g["uv"]
    eng = engine.Engine("prnet", _sd(), 2, 64, 64)
    x = torch.stack([torch.from_numpy(face_ref.make_input(int(s), 64, 64)) for s in g["in_seeds"][:2]]).cuda()
    y = eng(x)[0].cpu().double().numpy()
    e_small = float(np.abs(y - g["small"]).max())
    big = engine.Engine("prnet", _sd(), 1, 256, 256)
    y = big(torch.from_numpy(face_ref.make_input(int(g["in_seeds"][2]), 256, 256))[None].cuda())[0].cpu().double().numpy()[0]
    lines = np.concatenate([y[:, (0, 1, 254, 255), :], y[:, :, (0, 1, 254, 255)].transpose(0, 2, 1)], 1)
    e_big = max(float(np.abs(lines - g["lines"]).max()), float(np.abs(y[:, ::8, ::8] - g["grid"]).max()),
                float(np.abs(y[:, uv[1], uv[0]] - g["landmarks"]).max()))
    print("prnet vs recorded float64 maps: 64x64 %.3e, 256x256 %.3e (gap32 %.3e)" % (e_small, e_big, float(g["gap32"])))
    assert e_small <= 1e-3 and e_big <= 1e-3


C_PLAN_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from centerpose_amd import cplan
x = torch.from_numpy(np.load(sys.argv[3])).cuda()
p = cplan.CPlan(sys.argv[2], use_graph=1)
for rep in range(3):                      # eager / capture / replay
    out = p.forward(x)
torch.cuda.synchronize()
assert p.n_outputs == 1
np.save(sys.argv[4], out[0].cpu().numpy())
p.close()
"""


def test_plan_file_round_trips_with_equal_bits(tmp_path):
    """Engine.save_plan -> plan.parse / Engine.from_plan and the C runtime (a fresh interpreter, cp_plan_load / cp_plan_forward)."""
    import subprocess
    import sys
    from centerpose_amd import engine, plan
    eng = engine.Engine("prnet", _sd(), 2, 64, 64, use_graph=False)
    x = torch.stack([torch.from_numpy(face_ref.make_input(60 + b, 64, 64)) for b in range(2)])
    ref = eng(x.cuda())[0].clone()
    path, xin, outp = str(tmp_path / "p.cpplan"), str(tmp_path / "x.npy"), str(tmp_path / "out.npy")
    eng.save_plan(path)
    assert torch.equal(eng(x.cuda())[0], ref)                            # the engine computes the same bits in the scheduled order
    p = plan.parse(memoryview(np.fromfile(path, dtype=np.uint8)))
    assert p["meta"]["arch"] == "prnet" and len(p["ops"]) == 53 and len(p["outputs"]) == 1 and tuple(p["outputs"][0][1]) == (2, 3, 64, 64)
    e2 = engine.Engine.from_plan(path)
    assert torch.equal(e2(x.cuda())[0], ref)
    np.save(xin, x.numpy())
    r = subprocess.run([sys.executable, "-c", C_PLAN_CHILD, ROOT, path, xin, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.load(outp), ref.cpu().numpy())


# ---------------------------------------------------------------- 4. restore
def test_restore_kernel_equals_its_host_twin():
    L = draw_util.lib_loaded()
    r = np.random.RandomState(13)
    cap = 3
    net = r.uniform(0, 1, (cap, 3, 256, 256)).astype(np.float32)
    slots = np.asarray([4, -1, 0], np.int32)
    xform = np.asarray([[-13.5, 7.25, 65.0], [0, 0, 0], [1000.5, -300.0, 32768.0]], np.float32)
    uv = face_util.uv_table()
    rc, hpos, hlm = face_util.host_restore(L, net, slots, xform, uv)
    assert rc == 0
    dn, ds, dx, du = (torch.from_numpy(a).cuda() for a in (net, slots, xform, uv))
    for positions in (True, False):
        pos = torch.full((cap * 256 * 256 * 3 + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        lm = torch.full((cap * 68 * 3 + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        rc = L.cp_face_restore_f32(VP(dn.data_ptr()), VP(ds.data_ptr()), VP(dx.data_ptr()), cap, VP(du.data_ptr()),
                                   VP(pos.data_ptr()) if positions else None, VP(lm.data_ptr()), _stream())
        torch.cuda.synchronize()
        assert rc == 0, L.cp_last_error()
        pos, lm = pos.cpu().numpy(), lm.cpu().numpy()
        assert np.isnan(lm[cap * 68 * 3:]).all() and face_util.same_bits(lm[:cap * 68 * 3].reshape(cap, 68, 3), hlm)
        if positions:
            assert np.isnan(pos[cap * 256 * 256 * 3:]).all() and face_util.same_bits(pos[:cap * 256 * 256 * 3].reshape(cap, 256, 256, 3), hpos)
        else:
            assert np.isnan(pos).all()                                    # positions=False: the map is never written
    assert not hpos[1].any() and not hlm[1].any()
    p64, l64 = face_ref.restore(net, slots, xform, uv, np.float64)
    for s in (0, 2):
        bound = 4 * np.spacing(np.float32(np.abs(p64[s]).max()))
        assert np.abs(hpos[s].astype(np.float64) - p64[s]).max() <= bound and np.abs(hlm[s].astype(np.float64) - l64[s]).max() <= bound


# ---------------------------------------------------------------- 5. end to end
@functools.lru_cache(maxsize=None)
def _aligner():
    from centerpose_amd import face
    return face.FaceAligner(_sd(), _golden()["uv"], capacity=2)


def _frames_96x128():
    """Two 96 x 128 pictures with large-scale structure: frame 0 as a B, G, R tensor, both also as NV12 planes."""
    pics = [np.ascontiguousarray((face_ref.make_input(70 + n, 96, 128)[::-1].transpose(1, 2, 0) * 255).round().astype(np.uint8)) for n in range(2)]
    return pics


def _reference(pics_bgr, cand, boxes, cap, uv, vis=face_ref.VIS):
    """host rule crop -> float64 net -> NumPy restore"""
    slots, counts, xform = face_ref.select(cand, boxes, vis, cap)
    x = face_ref.crops(pics_bgr, slots, xform, cand.shape[1])
    y = face_ref.net(_sd(), torch.from_numpy(x).double()).numpy()
    pos, lm = face_ref.restore(y, slots, xform, uv, np.float64)
    return slots, counts, xform, pos, lm


@pytest.mark.parametrize("color", ["bgr", "nv12"])
@pytest.mark.parametrize("boxes", [False, True])
def test_align_end_to_end(color, boxes):
    al = _aligner()
    uv = _golden()["uv"]
    pics = _frames_96x128()
    if color == "bgr":
        frames, seen = [torch.from_numpy(p).cuda() for p in pics], pics
    else:
        r = np.random.RandomState(80)
        planes = [(p[..., 1].copy(), r.randint(60, 200, (48, 64, 2)).astype(np.uint8)) for p in pics]
        frames = [tuple(torch.from_numpy(a).cuda() for a in pl) for pl in planes]
        seen = [yuv_ref.frame_to_bgr(pl, "nv12", "bt601") for pl in planes]
    if boxes:
        cand = np.stack([np.stack([face_ref.box_of(30, 90, 20, 75), face_ref.box_of(5, 40, 5, 40, 0.1)]),
                         np.stack([face_ref.box_of(60.5, 140, 40, 110.25), face_ref.box_of(0, 0, 0, 0)])]).astype(np.float32)
    else:
        cand = np.stack([np.stack([face_ref.joints_row(30, 90, 20, 75), face_ref.joints_row(5, 40, 5, 40, 0.1)]),
                         np.stack([face_ref.joints_row(60.5, 140, 40, 110.25), face_ref.joints_row(7, 7, 9, 9)])]).astype(np.float32)
    dev = torch.from_numpy(cand).cuda()
    res = al.align(frames, boxes=dev, color=color) if boxes else al.align(frames, rows=dev, color=color)
    keep = [t.clone() for t in (res.pos, res.landmarks, res.slots, res.counts, res.xform)]
    slots, counts, xform, pos, lm = _reference(seen, cand, boxes, 2, uv)
    assert res.slots.cpu().tolist() == slots.tolist() == [0, 2] and res.counts.cpu().tolist() == counts.tolist() == [1, 1]
    assert face_util.same_bits(res.xform.cpu().numpy(), xform)
    for s in range(2):
        bar = 1e-3 * 281.6 * float(xform[s, 2]) / 255.0                  # the plan's bar carried through the restore, in pixels
        e_lm = float(np.abs(res.landmarks[s].cpu().double().numpy() - lm[s]).max())
        e_pos = float(np.abs(res.pos[s].cpu().double().numpy() - pos[s]).max())
        print("align %s %s slot %d: landmarks %.3e px, map %.3e px (bar %.3e)" % (color, "boxes" if boxes else "rows", s, e_lm, e_pos, bar))
        assert e_lm <= bar and e_pos <= bar
    assert torch.equal(res.landmarks, res.pos[:, uv[1], uv[0]])
    # a second call with other candidates leaves the first result's tensors intact; positions=False gathers the same points
    other = dev.clone()
    other[:, 0, :4 if boxes else 15] += 3.0
    res2 = al.align(frames, boxes=other, color=color, positions=False) if boxes else al.align(frames, rows=other, color=color, positions=False)
    assert res2.pos is None and not torch.equal(res2.landmarks, res.landmarks)
    assert all(torch.equal(a, b) for a, b in zip(keep, (res.pos, res.landmarks, res.slots, res.counts, res.xform)))
    res3 = al.align(frames, boxes=dev, color=color, positions=False) if boxes else al.align(frames, rows=dev, color=color, positions=False)
    assert torch.equal(res3.landmarks, res.landmarks)
    assert torch.equal(res.vertices([0, 257, 65535])[:, 1], res.pos[:, 1, 1])


def test_align_refuses_before_any_launch():
    from centerpose_amd import _lib
    al = _aligner()
    pics = _frames_96x128()
    frames = [torch.from_numpy(p).cuda() for p in pics]
    rows = torch.zeros((2, 1, 56), device="cuda")
    before = al.engine.input.clone()
    with pytest.raises(ValueError, match="exactly one"):
        al.align(frames)
    with pytest.raises(ValueError, match="exactly one"):
        al.align(frames, rows=rows, boxes=torch.zeros((2, 1, 5), device="cuda"))
    with pytest.raises(ValueError, match="host arrays"):
        al.align(pics, rows=rows)
    with pytest.raises(_lib.CenterposeHipError, match="no CPU fallback"):
        al.align(frames, rows=rows.cpu())
    with pytest.raises(_lib.CenterposeHipError, match=r"\[N, F, 5\]"):
        al.align(frames, boxes=torch.zeros((2, 1, 4), device="cuda"))
    with pytest.raises(ValueError, match="capacity"):
        al.align(frames + frames[:1], rows=torch.zeros((3, 1, 56), device="cuda"))
    assert torch.equal(al.engine.input, before)
