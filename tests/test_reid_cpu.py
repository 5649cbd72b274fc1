"""CPU: the re-id stage without a device -- the `reid` graph against the recorded key list of the reference module, the float64
restatement of the net against the recorded features, the box and slot rules against hand-worked rows, the HOST crop twins
(cp_reid_*_host, the statements of csrc/reid_arith.h the kernels compile) bit for bit against the independent NumPy rules of
tests/reid_ref.py over whole buffers, and every refusal that needs no device."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import draw_ref
import draw_util
import reid_ref
import reid_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
VP = ctypes.c_void_p


# ---------------------------------------------------------------- 1. the graph, the spec, the synthetic checkpoint
def test_param_spec_is_the_reference_modules_state_dict():
    from centerpose_amd import nets
    keys = [(k, tuple(s)) for k, s in json.load(open(os.path.join(GOLDEN, "reid_keys.json")))]
    assert len(keys) == 130
    want = [(k, s) for k, s in keys if not k.startswith("classifier.")]
    spec, flops = nets.param_spec("reid")
    assert [(k, tuple(s)) for k, s in spec.items()] == want                   # names, shapes and the module's order
    assert nets.param_spec("ReID", 128, 64, internal=True)[0] == spec         # no prefix either way
    assert 2.2e9 < flops < 2.3e9                                              # 2 * MAC of the eighteen convolutions of one crop


def test_canonical_arch_and_the_fixed_input():
    from centerpose_amd import nets
    assert nets.canonical_arch("reid") == nets.canonical_arch("REID") == "reid" and "reid" not in nets.ARCH_HEAD
    with pytest.raises(ValueError, match="reid"):
        nets.canonical_arch("no_such_net")
    for h, w in ((64, 128), (128, 128), (256, 128)):
        with pytest.raises(ValueError, match="128 x 64"):
            nets.param_spec("reid", h, w)
    g = nets.Graph()
    out = g.network("reid", nets.Act(128, 64, 3))
    assert (out.H, out.W, out.C) == (1, 1, 512)


def test_engine_refuses_the_detector_only_modes_for_reid():
    from centerpose_amd import engine
    for kw in (dict(decode_k=100), dict(dets_only=True), dict(flip_test=True), dict(flip_dets_only=True)):
        with pytest.raises(ValueError, match="reid"):
            engine.Engine("reid", {}, 2, 128, 64, **kw)


def test_synthetic_checkpoint():
    from centerpose_amd import nets, synth
    sd = synth.make_state_dict("reid", seed=317)
    spec, _ = nets.param_spec("reid")
    assert list(sd) == list(spec) and all(tuple(sd[k].shape) == tuple(s) for k, s in spec.items())
    again = synth.make_state_dict("reid", seed=317)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    damped = [k for k in sd if k.startswith("layer") and k.endswith(".bn2.weight")]
    plain = [k for k in sd if k.endswith((".bn1.weight", "conv.1.weight", ".downsample.1.weight"))]
    assert len(damped) == 8 and max(float(sd[k].max()) for k in damped) <= 0.45 + 1e-6          # gamma in [0.5, 1.5) * 0.3
    assert min(float(sd[k].min()) for k in plain) >= 0.5 * 0.85 - 1e-6


def test_plan_files_refuse_the_reid_plan():
    from centerpose_amd import ops, plan
    fake = type("E", (), {"arch": "reid", "launches": [], "stream_plan": None})()
    with pytest.raises(ValueError, match="reid"):
        plan.plan_blob(fake)
    # the launch is marshalled like cp_global_avgpool_nhwc_f32 but has no plan-file id
    assert "cp_pool_l2norm_nhwc_f32" not in ops.FN_IDS
    a = ops.marshal("cp_pool_l2norm_nhwc_f32", None, [VP(8), VP(16)], [512, 512, 2, 32, 512])
    assert [getattr(v, "value", v) for v in a] == [8, 512, 16, 512, 2, 32, 512]


# ---------------------------------------------------------------- 2. the recorded features
@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "reid_features.npz"))
    return {k: g[k] for k in g.files}


def test_fixture_features_are_far_apart(golden):
    f = golden["features"]
    assert f.shape == (8, 512) and f.dtype == np.float64 and golden["crops"].shape == (8, 128, 64, 3)
    assert np.allclose(np.linalg.norm(f, axis=1), 1.0, atol=1e-12)
    d = np.sqrt(((f[:, None] - f[None]) ** 2).sum(2))
    assert d[~np.eye(8, dtype=bool)].min() >= 0.02          # twenty times the parity bar: a crop in the wrong slot cannot pass
    assert golden["gap32"] < 1e-5


def test_float64_restatement_reproduces_the_recorded_features(golden):
    from centerpose_amd import synth
    sd = synth.make_state_dict("reid", seed=int(golden["seed"]))
    with torch.no_grad():
        f = reid_ref.net(sd, reid_ref.normalise(golden["crops"])).numpy()
    assert np.abs(f - golden["features"]).max() <= 1e-9


# ---------------------------------------------------------------- 3. box and slot rules by hand
H, W = 100, 200
R = reid_ref.row
NAN, INF = float("nan"), float("inf")
BOXES = [
    ("off the left edge: x1 < 0, the width is carried over", R(-10, 20, 30, 60), (0, 20, 40, 60)),
    ("off the top edge", R(50, -5, 80, 25), (50, 0, 80, 30)),
    ("off the right edge: clamped to W - 1", R(180, 10, 230, 50), (180, 10, 199, 50)),
    ("off the bottom edge: clamped to H - 1", R(10, 90, 40, 130), (10, 90, 40, 99)),
    ("wholly right of the frame", R(250, 10, 300, 50), None),
    ("wholly left of the frame: moved to column 0 with its width", R(-50, 10, -20, 40), (0, 10, 30, 40)),
    ("x2 == x1", R(50, 10, 50, 40), None),
    ("x2 < x1", R(60, 10, 50, 40), None),
    ("y2 == y1 after truncation", R(50, 10.2, 60, 10.9), None),
    ("one column", R(20.5, 30.2, 21.9, 99), (20, 30, 21, 99)),
    ("the whole frame loses its last column and row", R(0, 0, 200, 100), (0, 0, 199, 99)),
    ("truncation toward zero of a negative corner", R(-0.9, -0.9, 10.9, 10.9), (0, 0, 10, 10)),
    ("score == vis_thresh", R(10, 10, 50, 50, 0.3), None),
    ("score just above", R(10, 10, 50, 50, np.nextafter(np.float32(0.3), np.float32(1))), (10, 10, 50, 50)),
    ("NaN score", R(10, 10, 50, 50, NAN), None),
    ("NaN coordinate", R(10, NAN, 50, 50), None),
    ("infinite x2: clamped to 2^30", R(10, 10, INF, 50), (10, 10, 199, 50)),
    ("-infinite x1", R(-INF, 10, 30, 50), (0, 10, 199, 50)),
    ("huge corners", R(-3e9, -3e9, 3e9, 3e9), (0, 0, 199, 99)),
]


@pytest.mark.parametrize("name,row,want", BOXES, ids=[b[0] for b in BOXES])
def test_box_rule_by_hand(name, row, want):
    L = draw_util.lib_built()
    assert reid_ref.box(row, H, W, 0.3) == want
    form = draw_ref._form(5, "hwc bgr", "hwc", "bgr", [(0, (H, W, 3), (3 * W, 3, 1))])
    rc, slots, counts = reid_util.host_select(L, [form], row.reshape(1, 1, 56), 0.3, 1)
    assert rc == 0 and counts.tolist() == [int(want is not None)] and slots.tolist() == [0 if want is not None else -1]
    if want is not None:                    # the library's crop is the reference's crop of exactly that rectangle
        rc, out = reid_util.host_crop(L, [form], row.reshape(1, 1, 56), 0.3, slots, 1)
        assert rc == 0 and reid_util.same_bits(out[:3 * 128 * 64].reshape(3, 128, 64), reid_ref.crop(reid_ref.picture(form), want))


SLOT_CASES, _slot_rows = reid_ref.SLOT_CASES, reid_ref.slot_rows


@pytest.mark.parametrize("cap,want", SLOT_CASES)
def test_slot_rule_by_hand(cap, want):
    L = draw_util.lib_built()
    rows = _slot_rows()
    forms = [draw_ref._form(7 + n, "hwc bgr", "hwc", "bgr", [(0, (H, W, 3), (3 * W, 3, 1))]) for n in range(3)]
    slots, counts = reid_ref.select(rows, [(H, W)] * 3, 0.3, cap)
    assert slots.tolist() == want and counts.tolist() == [4, 0, 1]
    rc, got_slots, got_counts = reid_util.host_select(L, forms, rows, 0.3, cap)
    assert rc == 0 and got_slots.tolist() == want and got_counts.tolist() == [4, 0, 1]


def test_selection_looks_at_each_frames_own_size():
    L = draw_util.lib_built()
    forms = [draw_ref._form(3, "a", "hwc", "bgr", [(0, (40, 30, 3), (90, 3, 1))]), draw_ref._form(4, "b", "hwc", "bgr", [(0, (90, 120, 3), (360, 3, 1))])]
    rows = np.stack([np.stack([R(35, 5, 60, 30)]), np.stack([R(35, 5, 60, 30)])])             # right of frame 0, inside frame 1
    rc, slots, counts = reid_util.host_select(L, forms, rows, 0.3, 2)
    assert rc == 0 and slots.tolist() == [-1, 1] and counts.tolist() == [0, 1]
    for yuv_forms in (draw_ref.yuv_forms(11, 40, 30)[:1] + draw_ref.yuv_forms(12, 90, 120)[:1],):      # H, W of the YUV descriptor
        rc, slots, counts = reid_util.host_select(L, yuv_forms, rows, 0.3, 2)
        assert rc == 0 and slots.tolist() == [-1, 1] and counts.tolist() == [0, 1]


# ---------------------------------------------------------------- 4. the host crop twins, bit for bit
def test_taps_by_hand():
    # 5 source columns onto 64: the first and last destination pixels sit on one tap; the ratio 5 / 64 puts pixel 32 at 2.0390625
    s0, s1, f = reid_ref.taps(5, 64)
    assert (s0[0], s1[0], f[0]) == (0, 1, np.float32(0)) and f[5] == 0 and s0[6] == 0 and f[6] == np.float32(6.5 * 5 / 64 - 0.5)
    assert (s0[32], s1[32], f[32]) == (2, 3, np.float32(0.0390625)) and (s0[63], s1[63], f[63]) == (4, 4, np.float32(0))
    assert s0.min() == 0 and s1.max() == 4
    # shrinking 300 rows onto 128: no antialiasing, two taps around (o + 0.5) * 300 / 128 - 0.5
    s0, s1, f = reid_ref.taps(300, 128)
    assert (s0[0], s1[0]) == (0, 1) and f[0] == np.float32(0.671875) and (s0[127], s1[127]) == (298, 299)
    # one source column: every destination pixel is that column
    s0, s1, f = reid_ref.taps(1, 64)
    assert not s0.any() and not s1.any() and not f.any()


CASES = reid_ref.crop_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_crop_twins_equal_the_reference_bit_for_bit(case):
    L = draw_util.lib_built()
    name, forms, rows, matrix, norm = case
    cap, vis = reid_ref.CAP, reid_ref.VIS
    before = [f["buf"].copy() for f in forms]
    want_x, want_slots, want_counts = reid_ref.crops([reid_ref.picture(f, matrix) for f in forms], rows, vis, cap, **norm)
    rc, slots, counts = reid_util.host_select(L, forms, rows, vis, cap)
    assert rc == 0 and np.array_equal(slots, want_slots) and np.array_equal(counts, want_counts)
    assert (want_slots >= 0).any()
    rc, out = reid_util.host_crop(L, forms, rows, vis, slots, cap, matrix, **norm)
    assert rc == 0, L.cp_last_error()
    n = cap * 3 * 128 * 64
    assert np.isnan(out[n:]).all() and not np.isnan(out[:n]).any()            # every element written, nothing behind the buffer
    assert reid_util.same_bits(out[:n].reshape(cap, 3, 128, 64), want_x)
    assert all(np.array_equal(f["buf"], b) for f, b in zip(forms, before))    # frames are only read


def test_reference_defaults_and_channel_pairing():
    """scale 1, the RGB-ordered ImageNet statistics on the frame's B, G, R: a constant frame gives three constant planes."""
    L = draw_util.lib_built()
    form = draw_ref._form(1, "flat", "hwc", "bgr", [(0, (20, 20, 3), (60, 3, 1))])
    draw_ref.numpy_views(form["buf"], form)[0][:] = (10, 100, 200)
    rows = R(2, 2, 12, 17).reshape(1, 1, 56)
    rc, out = reid_util.host_crop(L, [form], rows, 0.3, np.array([0], np.int32), 1)
    x = out[:3 * 128 * 64].reshape(3, -1)
    for k, (v, m, s) in enumerate(zip((10, 100, 200), (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))):
        assert rc == 0 and (x[k] == (np.float32(v) - np.float32(m)) / np.float32(s)).all()
    rc, out = reid_util.host_crop(L, [form], rows, 0.3, np.array([0], np.int32), 1, channel_order="rgb", scale=1 / 255.)
    x = out[:3 * 128 * 64].reshape(3, -1)
    for k, (v, m, s) in enumerate(zip((200, 100, 10), (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))):
        assert rc == 0 and (x[k] == (np.float32(v) * np.float32(1 / 255.) - np.float32(m)) / np.float32(s)).all()


def test_slots_that_name_no_selected_row_become_zeros():
    L = draw_util.lib_built()
    form = draw_ref._form(2, "f", "hwc", "bgr", [(0, (30, 30, 3), (90, 3, 1))])
    rows = np.stack([np.stack([R(2, 2, 12, 17), R(2, 2, 12, 17, 0.1)])])
    rc, out = reid_util.host_crop(L, [form], rows, 0.3, np.array([1, 2, -1, 0], np.int32), 4)        # not selected, out of range, unused, fine
    x = out[:4 * 3 * 128 * 64].reshape(4, -1)
    assert rc == 0 and not x[:3].any() and x[3].any()


# ---------------------------------------------------------------- 5. symbols, the struct, refusals
def test_symbols_and_the_norm_struct():
    L = draw_util.lib_built()
    from centerpose_amd import reid
    hdr = open(os.path.join(ROOT, "include", "centerpose_hip.h")).read()
    for sym in ("cp_pool_l2norm_nhwc_f32", "cp_sizeof_reid_norm", "cp_reid_select_rows", "cp_reid_crop_frames_f32", "cp_reid_crop_yuv_frames_f32",
                "cp_reid_select_rows_host", "cp_reid_crop_frames_host", "cp_reid_crop_yuv_frames_host"):
        assert re.search(r"\b%s\s*\(" % sym, hdr) and hasattr(L, sym), sym
    assert L.cp_sizeof_reid_norm() == reid.REID_NORM.itemsize == 32
    body = re.search(r"typedef struct cp_reid_norm \{(.*?)\} cp_reid_norm;", hdr, re.S).group(1)
    fields = [re.sub(r"[\[\]\d\s]", "", f).rstrip("_") for f in re.findall(r"(?:float|int) ([^;]+);", body)]
    assert fields == list(reid.REID_NORM.names)
    assert reid.REID_MEAN == reid_ref.MEAN and reid.REID_STD == reid_ref.STD


def _bgr_form(seed=1, H=20, W=24):
    return draw_ref._form(seed, "f", "hwc", "bgr", [(0, (H, W, 3), (3 * W, 3, 1))])


def test_refusals_of_the_call_itself():
    L = draw_util.lib_built()
    rows = np.zeros((2, 3, 56), np.float32)
    forms = [_bgr_form(1), _bgr_form(2)]
    for cap, message in ((0, "capacity 0 outside 1..4096"), (4097, "capacity 4097 outside"), (1, "2 frames for a capacity of 1")):
        rc, slots, counts = reid_util.host_select(L, forms, rows, 0.3, cap)
        assert rc == 1 and message in L.cp_last_error().decode() and (slots == -7).all() and (counts == -7).all()
    rc, out = reid_util.host_crop(L, forms, rows, 0.3, np.full(1, -1, np.int32), 1)
    assert rc == 1 and "2 frames for a capacity of 1" in L.cp_last_error().decode() and np.isnan(out).all()
    table = draw_util.table_of(forms, [f["buf"].ctypes.data for f in forms])
    one = np.zeros(56, np.float32)
    rc = L.cp_reid_select_rows_host(table.ctypes.data_as(VP), 0, 2, one.ctypes.data_as(VP), (1 << 23) + 1, ctypes.c_float(0.3), 4, VP(8), VP(8))
    assert rc == 1 and "too many" in L.cp_last_error().decode()
    rc = L.cp_reid_select_rows_host(table.ctypes.data_as(VP), 0, 2, one.ctypes.data_as(VP), -1, ctypes.c_float(0.3), 4, VP(8), VP(8))
    assert rc == 1 and "negative row count" in L.cp_last_error().decode()
    rc = L.cp_reid_select_rows_host(None, 0, 2, one.ctypes.data_as(VP), 1, ctypes.c_float(0.3), 4, VP(8), VP(8))
    assert rc == 1 and "null pointer" in L.cp_last_error().decode()
    rc, out = reid_util.host_crop(L, forms, rows, 0.3, np.full(4, -1, np.int32), 4, channel_order="bgr")
    assert rc == 0 and not out[:4 * 3 * 128 * 64].any()                       # M rows of score 0: every slot unused, all zeros


@pytest.mark.parametrize("field,value,message", [("base", 0, "null base"), ("H", 0, "bad size"), ("W", -3, "bad size"), ("row_stride", -1, "negative stride"),
                                                 ("pix_stride", -1, "negative stride"), ("row_stride", 1 << 61, "2^62")])
def test_frame_checks_come_before_any_access(field, value, message):
    L = draw_util.lib_built()
    form = _bgr_form()
    table = draw_util.table_of([form], [form["buf"].ctypes.data])
    table[field][0] = value
    rows = R(1, 1, 9, 9).reshape(1, 1, 56)
    out = np.full(3 * 128 * 64, np.nan, np.float32)
    nm = reid_util.norm_struct()
    rc = L.cp_reid_crop_frames_host(table.ctypes.data_as(VP), 1, rows.ctypes.data_as(VP), 1, ctypes.c_float(0.3), np.zeros(1, np.int32).ctypes.data_as(VP), 1,
                                    nm.ctypes.data_as(VP), out.ctypes.data_as(VP))
    assert rc == 1 and message in L.cp_last_error().decode() and np.isnan(out).all()


def test_yuv_and_norm_refusals():
    L = draw_util.lib_built()
    form = draw_ref.yuv_forms(3, 20, 24)[0]
    table = draw_util.table_of([form], [form["buf"].ctypes.data])
    rows = R(1, 1, 9, 9).reshape(1, 1, 56)
    out = np.full(3 * 128 * 64, np.nan, np.float32)
    slots = np.zeros(1, np.int32)

    def call(tab, coef, nm):
        c = (ctypes.c_int * 6)(*coef) if coef is not None else None
        return L.cp_reid_crop_yuv_frames_host(tab.ctypes.data_as(VP), 1, c, rows.ctypes.data_as(VP), 1, ctypes.c_float(0.3), slots.ctypes.data_as(VP), 1,
                                              nm.ctypes.data_as(VP), out.ctypes.data_as(VP))
    import yuv_ref
    good = yuv_ref.COEF["bt601"]
    assert call(table, (0,) + good[1:], reid_util.norm_struct()) == 1 and "CY must be positive" in L.cp_last_error().decode()
    assert call(table, None, reid_util.norm_struct()) == 1 and "null coef" in L.cp_last_error().decode()
    bad = reid_util.norm_struct()
    bad["rgb"] = 2
    assert call(table, good, bad) == 1 and "channel order flag 2" in L.cp_last_error().decode()
    for field, message in (("u_base", "null base"), ("c_row", "negative stride")):
        t = table.copy()
        t[field][0] = 0 if field == "u_base" else -2
        assert call(t, good, reid_util.norm_struct()) == 1 and message in L.cp_last_error().decode()
    assert np.isnan(out).all()
    assert call(table, good, reid_util.norm_struct()) == 0 and not np.isnan(out).any()


def test_run_batch_embed_refuses_host_arrays_before_anything_runs():
    from centerpose_amd import config, detector
    det = object.__new__(detector.MultiPoseDetector)
    det.cfg = config.get_cfg("dla_34")
    det.scales = det.cfg.TEST.TEST_SCALES
    det.model = type("Model", (), {"process": None, "device": "cpu"})()
    fake = type("Extractor", (), {"capacity": 4})()
    with pytest.raises(ValueError, match="frames on the device"):
        det.run_batch([np.zeros((8, 8, 3), np.uint8)], embed=fake)


def test_embed_recognises_host_arrays_in_every_form():
    from centerpose_amd import reid
    a = np.zeros((8, 8, 3), np.uint8)
    assert reid._holds_host_array(a) and reid._holds_host_array([a]) and reid._holds_host_array([(a, a)])
    assert not reid._holds_host_array([torch.zeros(2)]) and not reid._holds_host_array(torch.zeros(2))
