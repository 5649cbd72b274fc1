"""CPU: the face stage without a device -- the `prnet` parameter spec against the recorded keys, the float64 statement of the net
(tests/face_ref.py) against the recorded maps (and the reference module where its checkout is present), the plan's repacked weights
evaluated record by record in float64 against that statement, the host twins (cp_face_*_host) bit for bit against the NumPy float32
rules, the crop rule against scipy's map_coordinates, and the argument checks of face.py and the twins."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import draw_ref
import draw_util
import face_ref
import face_util
import reid_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the reference checkout: $CP_REFERENCE, or a directory `reference` beside the repository
REFERENCE_MODEL = os.path.join(os.environ.get("CP_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference")), "demo", "face", "resfcn256.py")
VP = ctypes.c_void_p


@pytest.fixture(scope="module")
def L():
    return draw_util.lib_built()


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "prn_maps.npz")))
    g["uv"] = np.loadtxt(os.path.join(golden_dir, "prn_uv_kpt_ind.txt")).astype(np.int32)
    return g


@pytest.fixture(scope="module")
def sd(golden):
    from centerpose_amd import synth
    return synth.make_state_dict("prnet", seed=int(golden["seed"]))


def _input(seed, size):
    return torch.from_numpy(face_ref.make_input(int(seed), size, size))[None]


# ---------------------------------------------------------------- 1. the arch
def test_param_spec_equals_the_recorded_keys(golden_dir):
    from centerpose_amd import nets
    with open(os.path.join(golden_dir, "prn_keys.json")) as f:
        keys = json.load(f)
    spec, flops = nets.param_spec("prnet")
    assert [[k, list(v)] for k, v in spec.items()] == keys
    assert 8.0e9 < flops < 8.5e9                                  # "about 8 GFLOP per crop"
    assert nets.canonical_arch("PRNet") == "prnet"
    with pytest.raises(ValueError, match="multiples of 32"):
        nets.param_spec("prnet", 48, 64)
    with pytest.raises(ValueError, match="prnet"):
        nets.canonical_arch("no_such_net")


def test_float64_statement_reproduces_the_recorded_maps(golden, sd):
    uv = golden["uv"]
    small = torch.cat([_input(s, 64) for s in golden["in_seeds"][:2]]).double()
    y = face_ref.net(sd, small).numpy()
    assert np.abs(y - golden["small"]).max() < 1e-9
    big = face_ref.net(sd, _input(golden["in_seeds"][2], 256).double()).numpy()[0]
    lines = np.concatenate([big[:, (0, 1, 254, 255), :], big[:, :, (0, 1, 254, 255)].transpose(0, 2, 1)], 1)
    assert np.abs(lines - golden["lines"]).max() < 1e-9 and np.abs(big[:, ::8, ::8] - golden["grid"]).max() < 1e-9
    assert np.abs(big[:, uv[1], uv[0]] - golden["landmarks"]).max() < 1e-9
    assert golden["small"].min() < 0.2 and golden["small"].max() > 0.8 and golden["grid"].min() < 0.2 and golden["grid"].max() > 0.8
    assert 0 < float(golden["gap32"]) < 1e-3


@pytest.mark.skipif(not os.path.exists(REFERENCE_MODEL), reason="the reference checkout is not present")
def test_float64_statement_equals_the_reference_module(sd):
    import importlib.util
    spec = importlib.util.spec_from_file_location("reference_resfcn256", REFERENCE_MODEL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net = mod.PRNet(3, 3).eval()
    net.load_state_dict(sd)
    x = torch.cat([_input(31, 64), _input(32, 64)]).double()
    with torch.no_grad():
        want = net.double()(x)
    assert (face_ref.net(sd, x) - want).abs().max().item() < 1e-12


@pytest.mark.parametrize("H,W", [(32, 32), (64, 96)])
def test_plan_records_evaluated_in_float64_equal_the_statement(sd, H, W):
    """The plan builder on the CPU (records only, nothing is launched): flipped / swapped transposed weights, the after-pads, the
    shortcut folded into the residual, [W3 | I], eps 1e-3 and the zero-written padding channels, record by record."""
    from centerpose_amd import engine, nets
    inp = torch.zeros((2, 3, H, W))
    pb = engine.PlanBuilder(engine.normalize_state_dict(sd, "prnet"), 2, torch.device("cpu"))
    pb.bn_eps = nets.PRNET_BN_EPS
    pb.network("prnet", nets.Act(H, W, 3, inp))
    assert len(pb.launches) == 53 and all(l.fn == "cp_conv2d_f32" for _, _, _, l in pb.launches)
    assert tuple(pb.outputs[0].shape) == (2, 3, H, W)
    x = torch.stack([torch.from_numpy(face_ref.make_input(s, H, W)) for s in (41, 42)])
    got = face_util.run_plan_f64(pb.launches, inp, x)
    want = face_ref.net(sd, x.double())
    # 53 records, each with its BN folded in float32 (2^-24 relative on scale and shift) acting on activations of up to ~50, behind
    # a sigmoid of slope <= 1/4: 53 * 6e-8 * 50 / 4 = 4e-5 at the worst, 1e-5 is tighter than that and far below the 1e-3 bar
    assert (got - want).abs().max().item() < 1e-5
    # the three-channel tail: 16-channel maps whose padding channels every launch writes as zeros
    sh = face_util.Shadow()
    sh.put(inp, x.double())
    for _, name, _, l in pb.launches:
        v, _ = face_util.conv_launch_f64(l, sh.get)
        sh.put(l.out, v)
        assert not torch.isnan(v).any(), name                    # every element of every output is written
        if name in ("output_conv.1", "output_conv.5"):
            assert v.shape[3] == 16 and (v[..., 3:] == 0).all() and v[..., :3].abs().max() > 0


def test_other_archs_keep_their_eps():
    from centerpose_amd import nets, ops
    assert ops.BN_EPS == 1e-5 and nets.PRNET_BN_EPS == 1e-3
    g, b, m, v = (torch.tensor([x]) for x in (1.5, 0.25, 0.5, 2.0))
    sc, sh = ops.fold_bn(1, (g, b, m, v))
    assert sc[0].item() == (g / torch.sqrt(v + 1e-5))[0].item() and ops.fold_bn(1, (g, b, m, v), eps=1e-3)[0][0].item() != sc[0].item()


# ---------------------------------------------------------------- 2. the host twins
@pytest.mark.parametrize("boxes", [False, True])
def test_select_twin_equals_the_numpy_rule(L, boxes):
    cand = face_ref.select_cases(boxes)
    for cap, want in face_ref.SELECT_EXPECT.items():
        rc, slots, counts, xform = face_util.host_select(L, cand, boxes, cap)
        assert rc == 0, L.cp_last_error()
        rs, rc_, rx = face_ref.select(cand, boxes, face_ref.VIS, cap)
        assert slots.tolist() == want == rs.tolist() and counts.tolist() == face_ref.SELECT_COUNTS == rc_.tolist()
        assert face_util.same_bits(xform, rx)
    # the cases are what they say: size exactly 1, size exactly 32768
    rc, slots, counts, xform = face_util.host_select(L, cand, boxes, 21)
    assert xform[2, 2] == 1.0 and xform[7, 2] == 32768.0 and xform[0].tolist() == [-2.0, 8.0, 64.0]


def test_select_twin_beyond_one_wave_and_other_rules(L):
    r = np.random.RandomState(9)
    cand = np.zeros((2, 150, 56), np.float32)
    cand[..., 5:15] = r.uniform(-30, 200, (2, 150, 10))
    cand[..., 4] = r.choice([0.1, 0.3, 0.31, 0.9, np.nan], (2, 150))
    cand[0, 7, 9] = np.nan
    for cap, expand, min_size in ((2, 1.6, 1), (64, 1.6, 1), (256, 0.05, 6)):
        rc, slots, counts, xform = face_util.host_select(L, cand, False, cap, expand=expand, min_size=min_size)
        rs, rcn, rx = face_ref.select(cand, False, face_ref.VIS, cap, expand, min_size)
        assert rc == 0 and np.array_equal(slots, rs) and np.array_equal(counts, rcn) and face_util.same_bits(xform, rx)
        assert 10 < rcn.min() < 150


def _pictures(forms, matrix):
    return [reid_ref.picture(f, matrix) for f in forms]


crop_boxes, case_candidates = face_ref.crop_boxes, face_ref.case_candidates
CASES = face_ref.crop_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_crop_twin_equals_the_numpy_rule(L, case):
    name, forms, matrix = case
    boxes, cap = case_candidates(forms)
    rc, slots, counts, xform = face_util.host_select(L, boxes, True, cap)
    assert rc == 0 and counts.tolist() == [9] * len(forms) and (slots[9::10] == -1).all()
    before = [f["buf"].copy() for f in forms]
    rc, out = face_util.host_crop(L, forms, 9, slots, xform, matrix)
    assert rc == 0, L.cp_last_error()
    assert np.isnan(out[cap * 3 * 256 * 256:]).all() and all(np.array_equal(f["buf"], b) for f, b in zip(forms, before))
    got = out[:cap * 3 * 256 * 256].reshape(cap, 3, 256, 256)
    want = face_ref.crops(_pictures(forms, matrix), slots, xform, 9)
    assert face_util.same_bits(got, want)
    assert not got[5].any() and not got[9].any() and got[0].any() and got[7].any()         # wholly outside, unused
    assert got[1][:, :, 0].max() == 0 and got[1][:, :, -1].max() > 0                       # straddling the left border: zeros outside


def test_crop_rule_agrees_with_scipy_map_coordinates(L):
    pytest.importorskip("scipy.ndimage")
    form = draw_ref.bgr_forms(1300, 37, 53)[0]
    pic = reid_ref.picture(form)
    for b in crop_boxes(37, 53):
        t = face_ref.square(*b)
        want = face_ref.crop_scipy(pic, t)
        got = face_ref.crop(pic, t).astype(np.float64)
        # float32 coordinates near 100 carry 4e-6 px; times a slope of up to 1 grey level per px / 255, plus float32 blending: 1e-5
        assert np.abs(got - want).max() < 1e-5


def test_restore_twin_equals_the_numpy_rule(L):
    r = np.random.RandomState(11)
    cap = 3
    net = r.uniform(0, 1, (cap, 3, 256, 256)).astype(np.float32)
    slots = np.asarray([4, -1, 0], np.int32)
    xform = np.asarray([[-13.5, 7.25, 65.0], [0, 0, 0], [1000.5, -300.0, 32768.0]], np.float32)
    uv = face_util.uv_table()
    rc, pos, lm = face_util.host_restore(L, net, slots, xform, uv)
    assert rc == 0, L.cp_last_error()
    want_pos, want_lm = face_ref.restore(net, slots, xform, uv)
    assert face_util.same_bits(pos, want_pos) and face_util.same_bits(lm, want_lm) and not pos[1].any() and not lm[1].any()
    rc, none, lm2 = face_util.host_restore(L, net, slots, xform, uv, positions=False)
    assert rc == 0 and none is None and face_util.same_bits(lm2, want_lm)
    # against prnet.py:106-126 in float64: within 4 float32 ulps of the case's largest coordinate (three rounded operations)
    p64, l64 = face_ref.restore(net, slots, xform, uv, np.float64)
    for s in (0, 2):
        bound = 4 * np.spacing(np.float32(np.abs(p64[s]).max()))
        assert np.abs(pos[s].astype(np.float64) - p64[s]).max() <= bound and np.abs(lm[s].astype(np.float64) - l64[s]).max() <= bound


# ---------------------------------------------------------------- 3. argument checks
def test_twins_refuse_bad_arguments(L):
    cand = face_ref.select_cases(True)
    for kw, text in ((dict(min_size=0), b"min_size"), (dict(expand=0.0), b"expand"), (dict(expand=float("nan")), b"expand")):
        rc, *_ = face_util.host_select(L, cand, True, 6, **kw)
        assert rc == 1 and text in L.cp_last_error()
    assert face_util.host_select(L, cand, True, 2)[0] == 1 and b"every frame needs a slot" in L.cp_last_error()
    assert face_util.host_select(L, cand, True, 257)[0] == 1 and b"capacity" in L.cp_last_error()
    uv = face_util.uv_table()
    uv[1, 5] = 256
    net = np.zeros((1, 3, 256, 256), np.float32)
    rc, _, _ = face_util.host_restore(L, net, np.zeros(1, np.int32), np.ones((1, 3), np.float32), uv, positions=False)
    assert rc == 1 and b"uv_kpt_ind[1][5]" in L.cp_last_error()
    form = draw_ref.bgr_forms(1400, 7, 5)[0]
    table = draw_util.table_of([form], [form["buf"].ctypes.data])
    table["base"] = 0
    rc, _ = face_util.host_crop(L, [form], 1, np.zeros(1, np.int32), np.ones((1, 3), np.float32), table=table)
    assert rc == 1 and b"null base" in L.cp_last_error()


def test_face_module_checks_raise_before_anything_is_built(golden_dir, tmp_path):
    from centerpose_amd import face
    uv = face.load_uv_kpt_ind(os.path.join(golden_dir, "prn_uv_kpt_ind.txt"))
    assert uv.shape == (2, 68) and uv.dtype == np.int32 and uv.min() >= 0 and uv.max() < 256
    for bad, text in ((uv[:, :67], r"\[2, 68\]"), (uv.astype(np.float64) + 0.5, "whole numbers"), (np.where(uv == uv.max(), 256, uv), "0..255"),
                      (-uv - 1, "0..255")):
        with pytest.raises(ValueError, match=text):
            face.check_uv_kpt_ind(bad)
    for kw, text in ((dict(capacity=0), "capacity"), (dict(capacity=257), "capacity"), (dict(min_size=0), "min_size"), (dict(expand=0), "expand")):
        with pytest.raises(ValueError, match=text):
            face.FaceAligner({}, uv, **kw)
    with pytest.raises(ValueError, match=r"\[2, 68\]"):
        face.FaceAligner({}, uv[:1])
    path = str(tmp_path / "prn.pth")
    torch.save({"input_conv.1.weight": torch.zeros(16, 3, 4, 4)}, path)
    assert list(face.load_prnet_state_dict(path)) == ["input_conv.1.weight"]
    res = face.FaceResult(None, None, None, None, None)
    with pytest.raises(ValueError, match="positions=False"):
        res.vertices([0, 1])
    pos = torch.arange(2 * 256 * 256 * 3, dtype=torch.float32).view(2, 256, 256, 3)
    assert torch.equal(face.FaceResult(pos, None, None, None, None).vertices([0, 257])[1, 1], pos[1, 1, 1])
