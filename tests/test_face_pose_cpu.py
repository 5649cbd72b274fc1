"""CPU: the head pose without a device -- the host twin (cp_face_pose_host, csrc/face_pose_host.h) against the recording of the
reference's estimate_pose (tests/golden/face_pose.npz) and against the independent NumPy statement (tests/face_pose_ref.py:
np.linalg.svd, two-pass centring), its partial moments against a NumPy restatement of the header's summation order bit for bit, the
zeros of unused and invalid slots, and the refusals of the tables and of the call.

Bars: P to 1e-9 of its largest entry and the angles to 1e-9 rad, the project's bar for float64 host math (the tracker's).  Measured:
the twin lies 8.0e-18 (P, of its largest entry) and 1.2e-14 rad from the recording and the same from face_pose_ref.  DESIGN.md
section 4.16."""
import numpy as np
import pytest

import draw_util
import face_pose_ref as ref
import face_pose_util as fpu


@pytest.fixture(scope="module")
def L():
    return draw_util.lib_built()


@pytest.fixture(scope="module")
def tables():
    from centerpose_amd import face
    g = fpu.golden()
    return face.check_pose_tables(g["face_ind"], g["canonical_vertices"])


@pytest.fixture(scope="module")
def recorded(L, tables):
    """The 24 recorded cases as 24 slots of restored maps, through the host twin once."""
    g = fpu.golden()
    cases = ref.cases_of(g)
    pos = np.stack([ref.place(c["vertices"], g["face_ind"]) for c in cases])
    lm = np.stack([c["landmarks"] for c in cases])
    cap = len(cases)
    rc, out = fpu.host_pose(L, pos, 1, np.arange(cap), np.tile(np.float32([0, 0, 100]), (cap, 1)), *tables, lm)
    assert rc == 0, L.cp_last_error()
    return cases, out


def test_host_twin_meets_the_recording(recorded):
    cases, out = recorded
    assert len(cases) == 24 and out["valid"].tolist() == [1] * 24
    worst_p = worst_a = 0.0
    for k, c in enumerate(cases):
        e_p = np.abs(out["P"][k] - c["P"]).max() / np.abs(c["P"]).max()
        e_a = np.abs(out["angles"][k] - c["angles"]).max()
        worst_p, worst_a = max(worst_p, e_p), max(worst_a, e_a)
        assert e_p <= 1e-9 and e_a <= 1e-9, (k, e_p, e_a)
        assert abs(out["scale"][k] - c["s"]) <= 1e-9 * c["s"]
    print("host twin vs the recording: P %.2e of its largest entry, angles %.2e rad" % (worst_p, worst_a))
    # case 1 is the reflected cloud: the polar factor of its covariance has determinant -1 and the reference's fix (column 2 negated)
    # is what the recording holds; no other case takes that branch
    can = fpu.golden()["canonical_vertices"]
    for k, c in enumerate(cases):
        v = c["vertices"].astype(np.float64)
        U, _, Vt = np.linalg.svd((v - v.mean(0)).T @ (can - can.mean(0)))
        assert (np.linalg.det(U @ Vt) < 0) == (k == 1) and np.linalg.det(c["P"][:, :3]) > 0 and np.linalg.det(out["P"][k][:, :3]) > 0


def test_host_twin_meets_the_numpy_statement(recorded):
    g = fpu.golden()
    cases, out = recorded
    worst_p = worst_a = 0.0
    for k, c in enumerate(cases):
        want = ref.pose(c["vertices"], g["canonical_vertices"], c["landmarks"])
        e_p = np.abs(out["P"][k] - want["P"]).max() / np.abs(want["P"]).max()
        e_a = np.abs(out["angles"][k] - want["angles"]).max()
        worst_p, worst_a = max(worst_p, e_p), max(worst_a, e_a)
        assert e_p <= 1e-9 and e_a <= 1e-9 and abs(out["scale"][k] - want["scale"]) <= 1e-9 * want["scale"], (k, e_p, e_a)
        assert np.array_equal(out["box"][k], want["box"]), k                  # the recorder keeps every corner 1e-6 from a whole number
    print("host twin vs face_pose_ref: P %.2e of its largest entry, angles %.2e rad" % (worst_p, worst_a))


def _moments_numpy(vertices64, face_count, centred):
    """The header's summation order, restated: -> partial moments [chunks, 13] and the pivot."""
    V = face_count
    c = vertices64[0]
    d = vertices64 - c
    terms = np.empty((V, 13))
    terms[:, 0:3] = d
    for i in range(3):
        for j in range(3):
            terms[:, 3 + 3 * i + j] = d[:, i] * centred[:, j]
    terms[:, 12] = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    chunks = -(-V // 2048)
    parts = np.zeros((chunks, 13))
    for ch in range(chunks):
        lanes = np.zeros((256, 13))
        for i in range(8):
            v = ch * 2048 + i * 256 + np.arange(256)
            m = v < V
            lanes[m] = lanes[m] + terms[v[m]]
        stride = 128
        while stride >= 1:
            lanes[:stride] = lanes[:stride] + lanes[stride:2 * stride]
            stride //= 2
        parts[ch] = lanes[0]
    return parts, c


@pytest.mark.parametrize("V", [3, 255, 256, 257, 2047, 2048, 2049, 2742])
def test_partial_moments_follow_the_stated_order_bit_for_bit(L, V):
    """... for both sources: the plan's output restored on the fly and the restored map give the same bits."""
    g = fpu.golden()
    from centerpose_amd import face
    r = np.random.RandomState(V)
    face_ind = r.randint(0, 65536, V).astype(np.int32)                        # duplicates and any order
    face_ind[0] = 65535
    ind, centred, stats = face.check_pose_tables(face_ind, g["canonical_vertices"][:V])
    net, slots, xform = fpu.synthetic(40 + V, 3, (0, 2))
    pos, lm = fpu.restored(L, net, slots, xform)
    rc, a = fpu.host_pose(L, net, 0, slots, xform, ind, centred, stats, lm)
    assert rc == 0, L.cp_last_error()
    rc, b = fpu.host_pose(L, pos, 1, slots, xform, ind, centred, stats, lm)
    assert rc == 0
    for k in ("P", "angles", "scale", "scratch"):
        assert fpu.same_bits64(a[k], b[k]), k
    assert np.array_equal(a["box"], b["box"]) and a["valid"].tolist() == b["valid"].tolist() == [1, 0, 1]
    chunks = -(-V // 2048)
    per = chunks * 13 + 3
    for s in (0, 2):
        parts, c = _moments_numpy(pos[s].reshape(-1, 3)[ind].astype(np.float64), V, centred)
        got = a["scratch"][s * per:(s + 1) * per]
        assert fpu.same_bits64(got[:chunks * 13].reshape(chunks, 13), parts) and fpu.same_bits64(got[chunks * 13:], c)
        want = ref.pose(pos[s].reshape(-1, 3)[ind], g["canonical_vertices"][:V], lm[s])
        if V >= 255:                # (three random points: the covariance has rank two, the rotation is not unique)
            assert np.abs(a["P"][s] - want["P"]).max() <= 1e-9 * np.abs(want["P"]).max()
            assert np.array_equal(a["box"][s], want["box"])
    assert (a["scratch"][per:2 * per] == fpu.SENTINEL).all()                   # the unused slot's part is not touched
    assert not a["P"][1].any() and not a["angles"][1].any() and a["scale"][1] == 0 and not a["box"][1].any()


def test_unused_and_invalid_slots_are_zeros(L, tables):
    g = fpu.golden()
    cases = ref.cases_of(g)[:2]
    ind = tables[0]
    good = ref.place(cases[0]["vertices"], g["face_ind"])
    nan = good.copy()
    nan.reshape(-1, 3)[ind[1700], 1] = np.nan
    inf = good.copy()
    inf.reshape(-1, 3)[ind[0], 2] = np.inf                                     # the pivot itself
    one_point = np.full_like(good, 123.456)
    pos = np.stack([good, nan, good, one_point, inf])
    slots = np.asarray([0, 1, -1, 3, 4], np.int32)
    lm = np.stack([cases[0]["landmarks"]] * 5)
    rc, out = fpu.host_pose(L, pos, 1, slots, np.tile(np.float32([0, 0, 100]), (5, 1)), *tables, lm)
    assert rc == 0 and out["valid"].tolist() == [1, 0, 0, 0, 0]
    for s in range(1, 5):
        assert not out["P"][s].any() and not out["angles"][s].any() and out["scale"][s] == 0 and not out["box"][s].any()
    assert out["P"][0].any() and out["box"][0].any()


def test_bad_tables_are_refused():
    from centerpose_amd import face
    g = fpu.golden()
    ind, can = g["face_ind"], g["canonical_vertices"]
    face.check_pose_tables(ind.astype(np.float64), can.astype(np.float32))      # the text file's floats are whole numbers: fine
    for bad_ind, bad_can, match in ((ind[:2], can[:2], "one row"), (ind.reshape(2, -1), can, "one row"), (ind + 0.5, can, "whole numbers"),
                                    (np.where(np.arange(len(ind)) == 5, 65536, ind), can, "0..65535"),
                                    (np.where(np.arange(len(ind)) == 5, -1, ind), can, "0..65535"), (ind, can[:-1], "holds 2741"),
                                    (ind, can[:, :2], r"\[V, 3\]"), (ind, np.where(can == can[7, 1], np.nan, can), "finite"),
                                    (ind, np.where(can == can[7, 1], np.inf, can), "finite"), (ind, np.ones_like(can), "one point"),
                                    (np.full(len(ind), np.nan), can, "whole numbers"), (np.zeros(65537), np.zeros((65537, 3)), "one row")):
        with pytest.raises(ValueError, match=match):
            face.check_pose_tables(bad_ind, bad_can)
    uv = np.zeros((2, 68), np.int32)
    with pytest.raises(ValueError, match="together"):
        face.FaceAligner({}, uv, face_ind=ind)
    with pytest.raises(ValueError, match="together"):
        face.FaceAligner({}, uv, canonical_vertices=can)


def test_tables_load_from_the_reference_file_formats(tmp_path):
    from centerpose_amd import face
    g = fpu.golden()
    np.savetxt(str(tmp_path / "face_ind.txt"), g["face_ind"].astype(np.float64))
    np.save(str(tmp_path / "canonical_vertices.npy"), g["canonical_vertices"])
    a = face.check_pose_tables(str(tmp_path / "face_ind.txt"), tmp_path / "canonical_vertices.npy")
    b = face.check_pose_tables(g["face_ind"], g["canonical_vertices"])
    assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))
    assert a[0].dtype == np.int32 and a[1].dtype == np.float64 and a[2].shape == (4,) and abs(a[1].sum(axis=0)).max() < 1e-9


def test_the_twin_refuses_bad_calls(L, tables):
    ind, centred, stats = tables
    pos = np.zeros((1, 256, 256, 3), np.float32)
    lm = np.zeros((1, 68, 3), np.float32)
    x = np.float32([[0, 0, 100]])
    ok = lambda rc: rc == 0
    assert ok(fpu.host_pose(L, pos, 1, [0], x, ind, centred, stats, lm)[0])
    assert fpu.host_pose(L, pos, 1, [0], x, ind[:2], centred[:2], stats, lm)[0] == 1 and b"vertices" in L.cp_last_error()
    assert fpu.host_pose(L, pos, 2, [0], x, ind, centred, stats, lm)[0] == 1 and b"source kind" in L.cp_last_error()
    assert fpu.host_pose(L, pos, 1, [0], x, ind, centred, stats, lm, scratch_bytes=fpu.scratch_doubles(1, len(ind)) * 8 - 1)[0] == 1
    assert b"scratch" in L.cp_last_error()
    assert L.cp_face_pose_scratch_bytes(3, 2742) == fpu.scratch_doubles(3, 2742) * 8 == 3 * (2 * 13 + 3) * 8
    assert L.cp_face_pose_scratch_bytes(0, 2742) == L.cp_face_pose_scratch_bytes(257, 2742) == 0
    assert L.cp_face_pose_scratch_bytes(1, 2) == L.cp_face_pose_scratch_bytes(1, 65537) == 0
    assert L.cp_face_pose_host(None, 1, None, None, 1, None, 3, None, None, None, None, 10 ** 6, None, None, None, None, None) == 1
    assert b"null pointer" in L.cp_last_error()
    assert L.cp_face_pose_host(None, 1, None, None, 0, None, 3, None, None, None, None, 10 ** 6, None, None, None, None, None) == 1
    assert b"capacity" in L.cp_last_error()
