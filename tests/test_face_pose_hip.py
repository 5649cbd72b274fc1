"""GPU: the head pose on the device -- cp_face_pose_f32 (face_pose_moments_kernel<net|pos>, face_pose_solve_kernel) against its host
twin over whole guarded buffers: the partial moments in the scratch, P, the scale, the box and valid bit for bit, the angles to
1e-12 rad (asin / atan2 / cos come from two math libraries; at |angle| <= pi that is about 2 000 ulps of room and three orders inside
the 1e-9 bar of the recording); the two instantiations against each other bit for bit; the recorded cases at the 1e-9 bars; and
FaceAligner.align(pose=True, positions=False) end to end against estimate_pose(align(positions=True)).  DESIGN.md section 4.16."""
import functools
import os

import numpy as np
import pytest
import torch

import draw_util
import face_pose_ref as ref
import face_pose_util as fpu
import face_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device_pose(L, src, from_pos, slots, xform, ind, centred, stats, lm):
    """-> dict like face_pose_util.host_pose's, from the device; guards checked."""
    from centerpose_amd import _lib
    cap, V = len(slots), len(ind)
    a = [torch.from_numpy(np.ascontiguousarray(x, dt)).cuda() for x, dt in ((src, np.float32), (slots, np.int32), (xform, np.float32),
                                                                            (ind, np.int32), (centred, np.float64), (stats, np.float64),
                                                                            (lm, np.float32))]
    out = {k: torch.from_numpy(v).cuda() for k, v in fpu.outputs(cap, V).items()}
    rc = L.cp_face_pose_f32(a[0].data_ptr(), int(from_pos), a[1].data_ptr(), a[2].data_ptr(), cap, a[3].data_ptr(), V, a[4].data_ptr(),
                            a[5].data_ptr(), a[6].data_ptr(), out["scratch"].data_ptr(), fpu.scratch_doubles(cap, V) * 8, out["P"].data_ptr(),
                            out["angles"].data_ptr(), out["scale"].data_ptr(), out["box"].data_ptr(), out["valid"].data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0, L.cp_last_error()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert fpu.guards_intact(out, cap, V)                                      # nothing behind P, angles, scale, box, valid or the scratch
    return fpu.shaped(out, cap)


def _equal(dev, host):
    for k in ("scratch", "P", "scale"):
        assert fpu.same_bits64(dev[k], host[k]), k
    assert np.array_equal(dev["box"], host["box"]) and np.array_equal(dev["valid"], host["valid"])
    e = float(np.abs(dev["angles"] - host["angles"]).max())
    assert e <= 1e-12, e
    return e


def _tables(V, seed):
    """Tables of V vertices: the fixture's own for V = 2742, else random cells (duplicates, any order) and the first V canonical
    vertices of the fixture, tiled with an offset beyond its 2 742."""
    from centerpose_amd import face
    g = fpu.golden()
    if V == len(g["face_ind"]):
        return face.check_pose_tables(g["face_ind"], g["canonical_vertices"])
    r = np.random.RandomState(seed)
    ind = r.randint(0, 65536, V)
    ind[0], ind[-1] = 65535, 0
    can = np.resize(g["canonical_vertices"], (V, 3)) + r.uniform(-1.0, 1.0, (V, 3))
    return face.check_pose_tables(ind, can)


@pytest.mark.parametrize("cap,used,V", [(1, (0,), 3), (3, (0, 2), 255), (3, (0, 2), 256), (8, (0, 1, 3, 6, 7), 257), (3, (0, 2), 2047),
                                        (1, (0,), 2048), (3, (0, 2), 2049), (8, (0, 1, 3, 6, 7), 2742), (3, (1, 2), 43867)])
def test_pose_kernels_equal_the_host_twin(cap, used, V):
    L = draw_util.lib_loaded()
    ind, centred, stats = _tables(V, 100 + V)
    net, slots, xform = fpu.synthetic(200 + V, cap, used)
    pos, lm = fpu.restored(L, net, slots, xform)
    want_valid = [int(s in used) for s in range(cap)]
    results = []
    for from_pos, src in ((0, net), (1, pos)):
        rc, host = fpu.host_pose(L, src, from_pos, slots, xform, ind, centred, stats, lm)
        assert rc == 0 and host["valid"].tolist() == want_valid
        dev = _device_pose(L, src, from_pos, slots, xform, ind, centred, stats, lm)
        assert L.cp_last_kernel() == (b"face_pose_moments_kernel<pos>+face_pose_solve_kernel" if from_pos
                                      else b"face_pose_moments_kernel<net>+face_pose_solve_kernel")
        e = _equal(dev, host)
        results.append(dev)
    print("cap %d V %d: device angles within %.2e rad of the host twin's" % (cap, V, e))
    for k in ("scratch", "P", "scale", "angles"):                                  # net and pos: the same bits
        assert fpu.same_bits64(results[0][k], results[1][k]), k
    assert np.array_equal(results[0]["box"], results[1]["box"])
    per = fpu.scratch_doubles(1, V)
    for s in range(cap):
        if s not in used:                                                      # an unused slot: zeros, its scratch not touched
            assert (dev["scratch"][s * per:(s + 1) * per] == fpu.SENTINEL).all()
            assert not dev["P"][s].any() and not dev["angles"][s].any() and dev["scale"][s] == 0 and not dev["box"][s].any()


def test_invalid_slots_on_the_device():
    L = draw_util.lib_loaded()
    g = fpu.golden()
    ind, centred, stats = _tables(2742, 0)
    case = ref.cases_of(g)[0]
    good = ref.place(case["vertices"], g["face_ind"])
    nan = good.copy()
    nan.reshape(-1, 3)[ind[2100], 0] = np.nan
    pos = np.stack([nan, good, np.full_like(good, -3.5)])
    slots, xform, lm = np.int32([0, 1, 2]), np.tile(np.float32([0, 0, 100]), (3, 1)), np.stack([case["landmarks"]] * 3)
    rc, host = fpu.host_pose(L, pos, 1, slots, xform, ind, centred, stats, lm)
    dev = _device_pose(L, pos, 1, slots, xform, ind, centred, stats, lm)
    assert rc == 0 and dev["valid"].tolist() == host["valid"].tolist() == [0, 1, 0]
    assert not dev["P"][0].any() and not dev["P"][2].any() and not dev["box"][0].any() and not dev["box"][2].any()
    assert fpu.same_bits64(dev["P"], host["P"]) and np.array_equal(dev["box"], host["box"])


def test_recorded_cases_on_the_device():
    L = draw_util.lib_loaded()
    g = fpu.golden()
    ind, centred, stats = _tables(2742, 0)
    cases = ref.cases_of(g)
    pos = np.stack([ref.place(c["vertices"], g["face_ind"]) for c in cases])
    lm = np.stack([c["landmarks"] for c in cases])
    cap = len(cases)
    dev = _device_pose(L, pos, 1, np.arange(cap), np.tile(np.float32([0, 0, 100]), (cap, 1)), ind, centred, stats, lm)
    assert dev["valid"].tolist() == [1] * cap
    worst_p = worst_a = 0.0
    for k, c in enumerate(cases):
        e_p = np.abs(dev["P"][k] - c["P"]).max() / np.abs(c["P"]).max()
        e_a = np.abs(dev["angles"][k] - c["angles"]).max()
        worst_p, worst_a = max(worst_p, e_p), max(worst_a, e_a)
        assert e_p <= 1e-9 and e_a <= 1e-9, (k, e_p, e_a)
        assert np.array_equal(dev["box"][k], ref.box(c["P"], c["landmarks"]))
    print("device vs the recording: P %.2e of its largest entry, angles %.2e rad" % (worst_p, worst_a))


def test_launcher_refuses_before_any_launch():
    L = draw_util.lib_loaded()
    from centerpose_amd import _lib
    x = torch.full((4096,), fpu.SENTINEL, dtype=torch.float64, device="cuda")
    p = x.data_ptr()
    call = lambda cap, V, nbytes, src=p, kind=1: L.cp_face_pose_f32(src, kind, p, p, cap, p, V, p, p, p, p, nbytes, p, p, p, p, p, _lib.stream())
    for args, msg in (((0, 100, 10 ** 6), b"capacity"), ((257, 100, 10 ** 6), b"capacity"), ((1, 2, 10 ** 6), b"vertices"),
                      ((1, 65537, 10 ** 6), b"vertices"), ((1, 100, 16 * 8 - 1), b"scratch"), ((1, 100, 10 ** 6, None), b"null pointer"),
                      ((1, 100, 10 ** 6, p, 2), b"source kind")):
        assert call(*args) == 1 and msg in L.cp_last_error(), args
    torch.cuda.synchronize()
    assert (x == fpu.SENTINEL).all()


@functools.lru_cache(maxsize=None)
def _prn():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "prn_maps.npz")))
    g["uv"] = np.loadtxt(os.path.join(ROOT, "tests", "golden", "prn_uv_kpt_ind.txt")).astype(np.int32)
    return g


def test_align_with_pose_end_to_end():
    """Two 96 x 128 frames as tests/test_face_hip.py builds them: align(pose=True, positions=False) never writes the maps and gives
    the bits of estimate_pose(align(positions=True)); the pose is the host twin's over the downloaded maps."""
    from centerpose_amd import face, synth
    L = draw_util.lib_loaded()
    g, prn = fpu.golden(), _prn()
    sd = synth.make_state_dict("prnet", seed=int(prn["seed"]))
    al = face.FaceAligner(sd, prn["uv"], capacity=3, face_ind=g["face_ind"], canonical_vertices=g["canonical_vertices"])
    plain = face.FaceAligner(sd, prn["uv"], capacity=3)
    pics = [np.ascontiguousarray((face_ref.make_input(70 + n, 96, 128)[::-1].transpose(1, 2, 0) * 255).round().astype(np.uint8)) for n in range(2)]
    frames = [torch.from_numpy(p).cuda() for p in pics]
    rows = torch.from_numpy(np.stack([np.stack([face_ref.joints_row(30, 90, 20, 75)]),
                                      np.stack([face_ref.joints_row(60.5, 140, 40, 110.25)])]).astype(np.float32)).cuda()
    lean = al.align(frames, rows=rows, pose=True, positions=False)
    assert lean.pos is None and isinstance(lean.pose, face.FacePose)
    keep = [t.clone() for t in (lean.pose.P, lean.pose.angles, lean.pose.scale, lean.pose.box, lean.pose.valid)]
    full = al.align(frames, rows=rows)
    assert full.pose is None and full.pos is not None
    pose = al.estimate_pose(full)
    assert pose is full.pose and lean.pose.valid.cpu().tolist() == [1, 1, 0] and lean.slots.cpu().tolist() == [0, 1, -1]
    for a, b in zip(keep, (pose.P, pose.angles, pose.scale, pose.box, pose.valid)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert tuple(pose.P.shape) == (3, 3, 4) and tuple(pose.angles.shape) == (3, 3) and tuple(pose.scale.shape) == (3,)
    assert tuple(pose.box.shape) == (3, 10, 2) and pose.box.dtype == torch.int32 and pose.valid.dtype == torch.int32
    # the same bits without the new arguments as from an aligner without the tables
    base = plain.align(frames, rows=rows)
    assert torch.equal(base.pos, full.pos) and torch.equal(base.landmarks, full.landmarks) and torch.equal(base.landmarks, lean.landmarks)
    # ... and the host twin over the downloaded maps
    rc, host = fpu.host_pose(L, full.pos.cpu().numpy(), 1, full.slots.cpu().numpy(), full.xform.cpu().numpy(), *face.check_pose_tables(
        g["face_ind"], g["canonical_vertices"]), full.landmarks.cpu().numpy())
    assert rc == 0 and fpu.same_bits64(pose.P.cpu().numpy(), host["P"]) and np.array_equal(pose.box.cpu().numpy(), host["box"])
    assert np.abs(pose.angles.cpu().numpy() - host["angles"]).max() <= 1e-12
    # the refusals
    with pytest.raises(ValueError, match="face_ind"):
        plain.align(frames, rows=rows, pose=True)
    with pytest.raises(ValueError, match="face_ind"):
        plain.estimate_pose(full)
    with pytest.raises(ValueError, match="positions=False"):
        al.estimate_pose(lean)
    # a result that is not this aligner's own is refused before the launcher sees a pointer
    parts = dict(pos=full.pos, landmarks=full.landmarks, slots=full.slots, counts=full.counts, xform=full.xform)
    for name, bad in (("slots", full.slots[:2]), ("slots", full.slots.long()), ("xform", full.xform[:, :2]), ("xform", full.xform.t().contiguous().t()),
                      ("landmarks", full.landmarks[:, :27]), ("landmarks", full.landmarks.cpu()), ("landmarks", None),
                      ("pos", full.pos[:2]), ("pos", full.pos.double())):
        with pytest.raises(ValueError, match="not one of this aligner's: %s" % name):
            al.estimate_pose(face.FaceResult(**dict(parts, **{name: bad})))
