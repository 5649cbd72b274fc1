"""GPU: the re-id stage on the device -- cp_reid_select_rows and the crop kernels bit for bit against their host twins (and the NumPy
rules of tests/reid_ref.py) over whole buffers, cp_pool_l2norm_nhwc_f32 per element against float64, every launch of the `reid` plan
per element through tests/layer_oracle.py, Engine("reid") against the recorded float64 features, and ReidExtractor.embed /
run_batch(embed=) end to end."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import draw_util
import layer_oracle as lo
import reid_ref
import reid_util
import yuv_ref

SLOT_CASES, _slot_rows = reid_ref.SLOT_CASES, reid_ref.slot_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p
CROP = 3 * 128 * 64


def _tables(forms):
    """(device buffers kept alive, host copy of the descriptor table with DEVICE addresses, the same table on the device)"""
    devs = [torch.from_numpy(f["buf"].copy()).cuda() for f in forms]
    table = draw_util.table_of(forms, [d.data_ptr() for d in devs])
    return devs, table, torch.from_numpy(table.view(np.uint8).copy()).cuda()


def _stream():
    from centerpose_amd import _lib
    return _lib.stream()


def _device_select(L, forms, rows, vis, cap):
    devs, table, table_dev = _tables(forms)
    N, M = rows.shape[:2]
    r = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
    slots = torch.full((cap + 5,), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((N + 5,), -7, dtype=torch.int32, device="cuda")
    rc = L.cp_reid_select_rows(VP(table_dev.data_ptr()), table.ctypes.data_as(VP), int(reid_util.is_yuv(forms)), N, VP(r.data_ptr()), M,
                               ctypes.c_float(vis), cap, VP(slots.data_ptr()), VP(counts.data_ptr()), _stream())
    torch.cuda.synchronize()
    return rc, slots.cpu().numpy(), counts.cpu().numpy()


def _device_crop(L, forms, rows, vis, slots, cap, matrix="bt601", **norm):
    devs, table, table_dev = _tables(forms)
    N, M = rows.shape[:2]
    r = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
    s = torch.from_numpy(np.ascontiguousarray(slots, np.int32)).cuda()
    out = torch.full((cap * CROP + reid_util.GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    nm = reid_util.norm_struct(**norm)
    if reid_util.is_yuv(forms):
        coef = (ctypes.c_int * 6)(*yuv_ref.COEF[matrix])
        rc = L.cp_reid_crop_yuv_frames_f32(VP(table_dev.data_ptr()), table.ctypes.data_as(VP), N, coef, VP(r.data_ptr()), M, ctypes.c_float(vis),
                                           VP(s.data_ptr()), cap, nm.ctypes.data_as(VP), VP(out.data_ptr()), _stream())
    else:
        rc = L.cp_reid_crop_frames_f32(VP(table_dev.data_ptr()), table.ctypes.data_as(VP), N, VP(r.data_ptr()), M, ctypes.c_float(vis),
                                       VP(s.data_ptr()), cap, nm.ctypes.data_as(VP), VP(out.data_ptr()), _stream())
    torch.cuda.synchronize()
    frames_unchanged = all(np.array_equal(d.cpu().numpy(), f["buf"]) for d, f in zip(devs, forms))
    return rc, out.cpu().numpy(), frames_unchanged


# ---------------------------------------------------------------- 1. the stage kernels
@pytest.mark.parametrize("cap,want", SLOT_CASES)
def test_select_kernel_equals_its_host_twin(cap, want):
    import draw_ref
    L = draw_util.lib_loaded()
    rows = _slot_rows()                                        # N = 3, M = 7
    forms = [draw_ref._form(7 + n, "hwc bgr", "hwc", "bgr", [(0, (100, 200, 3), (600, 3, 1))]) for n in range(3)]
    rc, hs, hc = reid_util.host_select(L, forms, rows, 0.3, cap)
    assert rc == 0 and hs.tolist() == want
    rc, ds, dc = _device_select(L, forms, rows, 0.3, cap)
    assert rc == 0, L.cp_last_error()
    assert ds[:cap].tolist() == want and dc[:3].tolist() == hc.tolist() == [4, 0, 1]
    assert (ds[cap:] == -7).all() and (dc[3:] == -7).all()    # nothing behind the arrays
    assert L.cp_last_kernel() == b"reid_select_kernel<bgr>"


def test_select_kernel_beyond_one_wave_of_rows():
    """M = 150 rows per frame: three trips of the wave, ranks carried from trip to trip."""
    import draw_ref
    L = draw_util.lib_loaded()
    r = np.random.RandomState(5)
    rows = np.zeros((2, 150, 56), np.float32)
    rows[..., 0:2] = r.uniform(-20, 150, (2, 150, 2))
    rows[..., 2:4] = rows[..., 0:2] + r.uniform(-5, 60, (2, 150, 2))
    rows[..., 4] = r.choice([0.1, 0.3, 0.31, 0.9, np.nan], (2, 150))
    forms = draw_ref.yuv_forms(40, 90, 120)[:2]
    for cap in (2, 64, 300):
        rc, hs, hc = reid_util.host_select(L, forms, rows, 0.3, cap)
        want_s, want_c = reid_ref.select(rows, [(90, 120)] * 2, 0.3, cap)
        assert rc == 0 and np.array_equal(hs, want_s) and np.array_equal(hc, want_c) and 20 < want_c.min() < 150
        rc, ds, dc = _device_select(L, forms, rows, 0.3, cap)
        assert rc == 0 and np.array_equal(ds[:cap], want_s) and np.array_equal(dc[:2], want_c)
    assert L.cp_last_kernel() == b"reid_select_kernel<yuv>"


CASES = reid_ref.crop_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_crop_kernels_equal_their_host_twins_bit_for_bit(case):
    L = draw_util.lib_loaded()
    name, forms, rows, matrix, norm = case
    cap, vis = reid_ref.CAP, reid_ref.VIS
    rc, slots, counts = reid_util.host_select(L, forms, rows, vis, cap)
    assert rc == 0
    rc, host = reid_util.host_crop(L, forms, rows, vis, slots, cap, matrix, **norm)
    assert rc == 0
    rc, ds, dc = _device_select(L, forms, rows, vis, cap)
    assert rc == 0 and np.array_equal(ds[:cap], slots) and np.array_equal(dc[:len(forms)], counts)
    rc, dev, unchanged = _device_crop(L, forms, rows, vis, ds[:cap], cap, matrix, **norm)
    assert rc == 0, L.cp_last_error()
    n = cap * CROP
    assert np.isnan(dev[n:]).all() and unchanged              # the guard floats behind the buffer, the frames
    assert reid_util.same_bits(dev[:n], host[:n])             # the zeros of unused slots included
    want, _, _ = reid_ref.crops([reid_ref.picture(f, matrix) for f in forms], rows, vis, cap, **norm)
    assert reid_util.same_bits(dev[:n].reshape(cap, 3, 128, 64), want)
    assert L.cp_last_kernel() == (b"reid_crop_kernel<yuv>" if reid_util.is_yuv(forms) else b"reid_crop_kernel<bgr>")


def test_crop_kernel_zeroes_slots_that_name_no_selected_row():
    import draw_ref
    L = draw_util.lib_loaded()
    form = draw_ref._form(2, "f", "hwc", "bgr", [(0, (30, 30, 3), (90, 3, 1))])
    rows = np.stack([np.stack([reid_ref.row(2, 2, 12, 17), reid_ref.row(2, 2, 12, 17, 0.1)])])
    rc, dev, _ = _device_crop(L, [form], rows, 0.3, np.array([1, 2, -1, 0], np.int32), 4)
    x = dev[:4 * CROP].reshape(4, -1)
    assert rc == 0 and not x[:3].any() and x[3].any() and not np.isnan(x).any()


def test_device_launchers_refuse_before_any_launch():
    import draw_ref
    L = draw_util.lib_loaded()
    forms = [draw_ref._form(1, "f", "hwc", "bgr", [(0, (20, 24, 3), (72, 3, 1))]) for _ in range(2)]
    rows = np.zeros((2, 3, 56), np.float32)
    rc, ds, dc = _device_select(L, forms, rows, 0.3, 1)
    assert rc == 1 and "2 frames for a capacity of 1" in L.cp_last_error().decode() and (ds == -7).all() and (dc == -7).all()
    devs, table, table_dev = _tables(forms)
    out = torch.full((CROP,), float("nan"), device="cuda")
    s = torch.zeros(4, dtype=torch.int32, device="cuda")
    r = torch.zeros((2, 3, 56), device="cuda")
    nm = reid_util.norm_struct()
    for cap in (0, 4097):
        rc = L.cp_reid_crop_frames_f32(VP(table_dev.data_ptr()), table.ctypes.data_as(VP), 2, VP(r.data_ptr()), 3, ctypes.c_float(0.3), VP(s.data_ptr()),
                                       cap, nm.ctypes.data_as(VP), VP(out.data_ptr()), _stream())
        assert rc == 1 and "capacity %d outside 1..4096" % cap in L.cp_last_error().decode()
    bad = table.copy()
    bad["base"][1] = 0
    rc = L.cp_reid_crop_frames_f32(VP(table_dev.data_ptr()), bad.ctypes.data_as(VP), 2, VP(r.data_ptr()), 3, ctypes.c_float(0.3), VP(s.data_ptr()), 4,
                                   nm.ctypes.data_as(VP), VP(out.data_ptr()), _stream())
    assert rc == 1 and "frame 1: null base" in L.cp_last_error().decode()
    rc = L.cp_reid_crop_frames_f32(VP(table_dev.data_ptr()), table.ctypes.data_as(VP), 2, VP(r.data_ptr()), (1 << 23) + 1, ctypes.c_float(0.3),
                                   VP(s.data_ptr()), 4, nm.ctypes.data_as(VP), VP(out.data_ptr()), _stream())
    assert rc == 1 and "too many" in L.cp_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ---------------------------------------------------------------- 2. cp_pool_l2norm_nhwc_f32 per element against float64
def pool_l2norm_oracle(x, dt):
    """x: logical NCHW float32 CPU tensor -> lo.Out of mean over H W, divided by its L2 norm over C, in `dt`.
    Bound (float64 only): out_c = m_c / n, m the means, n = sqrt(sum m_j^2).  The kernel sums the HW pixels of a channel one after the
    other and divides once: |dm_c| <= (HW + 1) u Am_c with Am_c = mean |x|.  The squares are positive terms summed at depth
    cdiv(C, 256) + 9 (a thread's own channels, six butterfly levels, four wave partials), then one root and one division:
    |dn| / n <= (sum_j |m_j| |dm_j|) / n^2 + (cdiv(C, 256) + 12) / 2 u.  Hence |d out_c| <= K u A_c with
    A_c = Am_c / n + |out_c| (sum_j |m_j| Am_j / n^2 + 1) and K = HW + cdiv(C, 256) + 10, judged with lo.c_for("direct", K) like
    every reducing helper."""
    B, C, H, W = x.shape
    v = x.to(dt).flatten(2)
    m = v.mean(2)
    n = m.norm(p=2, dim=1, keepdim=True)
    out = m / n
    A = None
    if dt == torch.float64:
        Am = v.abs().mean(2)
        A = (Am / n + out.abs() * ((m.abs() * Am).sum(1, keepdim=True) / n ** 2 + 1))[..., None, None]
    return lo.Out(out[..., None, None], A, H * W + -(-C // 256) + 10)


def _run_pool_l2norm(x, in_pad=0, out_pad=0):
    """x logical NCHW (CPU) -> the kernel's [B, C] through NaN-poisoned strided views; also checks that nothing else was written."""
    from centerpose_amd import ops
    B, C, H, W = x.shape
    src = torch.full((B, H, W, C + in_pad), float("nan"), device="cuda")
    src[..., :C] = x.permute(0, 2, 3, 1).cuda()
    dst = torch.full((B + 1, C + out_pad), float("nan"), device="cuda")
    ops.pool_l2norm(src[..., :C], dst[:B, :C] if out_pad else dst[:B])
    torch.cuda.synchronize()
    got = dst.cpu()
    assert bool(torch.isnan(got[B:]).all()) and bool(torch.isnan(got[:B, C:]).all())
    return got[:B, :C]


@pytest.mark.parametrize("B,HW,C,in_pad,out_pad", [(3, 32, 512, 0, 0), (1, 1, 4, 0, 0), (2, 32, 512, 16, 8), (2, 7, 300, 4, 0)])
def test_pool_l2norm_per_element(B, HW, C, in_pad, out_pad):
    L = draw_util.lib_loaded()
    r = np.random.RandomState(B * 1000 + C)
    x = torch.from_numpy((r.randn(B, C, HW, 1) * r.uniform(0.01, 10, (1, C, 1, 1)) + r.randn(1, C, 1, 1)).astype(np.float32))
    got = _run_pool_l2norm(x, in_pad, out_pad)[..., None, None]
    assert L.cp_last_kernel() == b"pool_l2norm_kernel"
    o64 = pool_l2norm_oracle(x, torch.float64)
    w, fail = lo.judge(got, pool_l2norm_oracle(x, torch.float32), o64, "direct")
    print("pool_l2norm [%d, %d, %d]: worst err / (u A) %.3f (c = %.2f)" % (B, HW, C, w.ratio, lo.c_for("direct", o64.K)))
    assert fail is None, fail
    assert np.allclose(got.double().flatten(1).norm(dim=1).numpy(), 1.0, atol=1e-6)


def test_pool_l2norm_zero_map_is_nan_and_refusals():
    L = draw_util.lib_loaded()
    got = _run_pool_l2norm(torch.zeros(1, 8, 2, 2))
    assert bool(torch.isnan(got).all())                        # no epsilon, as x.div(x.norm()) in the reference
    buf = torch.zeros(1 << 12, device="cuda")
    P, S = VP(buf.data_ptr()), _stream()
    for args, message in (((P, 8, P, 16, 2, 5, 16), "inLd=8"), ((P, 16, P, 12, 2, 5, 16), "outLd=12"), ((P, 16, P, 16, 0, 5, 16), "bad arguments"),
                          ((P, 16, P, 16, 2, 0, 16), "bad arguments"), ((P, 16, P, 16, 2, 5, 0), "C=0"), ((None, 16, P, 16, 2, 5, 16), "bad arguments"),
                          ((P, 16, P, 16, 65536, 5, 16), "bad arguments")):
        assert L.cp_pool_l2norm_nhwc_f32(*args, S) == 1 and message in L.cp_last_error().decode(), args
    torch.cuda.synchronize()
    assert not bool(buf.any())


# ---------------------------------------------------------------- 3. every launch of the plan, per element
def test_every_launch_of_the_reid_plan_per_element(monkeypatch):
    """layer_oracle.run_plan over the `reid` plan at B = 2: its own hooks judge the convolutions and the max-pool; the new launch is
    recorded through the same mix-in and judged by `pool_l2norm_oracle`."""
    monkeypatch.setattr(lo.Recording, "emit_pool_l2norm", lo._make_hook("emit_pool_l2norm"), raising=False)
    plain = lo.evaluate

    def evaluate(hook, sd, args, get, dt, wino=None, om=None):
        if hook == "emit_pool_l2norm":
            return [pool_l2norm_oracle(get(args[0]), dt)]
        return plain(hook, sd, args, get, dt, wino=wino, om=om)
    monkeypatch.setattr(lo, "evaluate", evaluate)
    rep = lo.run_plan("reid", 2, 128, 64)
    print(lo.format_report("reid B=2 128x64", rep))
    assert not rep["failures"], "\n".join(rep["failures"][:10])
    assert rep["checked"] == rep["launches"] >= 20 and "pool_l2norm_kernel" in rep["kernels"]
    assert all(ratio <= lo.LAYER_TOL[fam] for fam, (ratio, _) in rep["worst"].items())


# ---------------------------------------------------------------- 4. the engine against the recorded features
@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "reid_features.npz"))
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def _sd():
    from centerpose_amd import synth
    return synth.make_state_dict("reid", seed=int(_golden()["seed"]))


@pytest.mark.parametrize("cap", [8, 5])
def test_engine_reproduces_the_recorded_features(cap):
    from centerpose_amd import engine
    g = _golden()
    e = engine.Engine("reid", _sd(), cap, 128, 64)
    x = reid_ref.normalise(g["crops"][:cap], torch.float32).cuda()
    outs = e.forward(x)
    assert len(outs) == 1 and tuple(outs[0].shape) == (cap, 512) and outs[0].dtype == torch.float32
    f = outs[0].double().cpu().numpy()
    d = np.sqrt(((f - g["features"][:cap]) ** 2).sum(1))
    print("Engine('reid', cap=%d): worst L2 distance to the float64 features %.3e (the reference's own float32 gap %.3e); %s"
          % (cap, d.max(), float(g["gap32"]), e.capture_mode))
    assert d.max() <= 1e-3                                     # the project's forward bar (gate 3) on a unit-norm vector
    assert e.capture_mode == "2-stream"
    eager = engine.Engine("reid", _sd(), cap, 128, 64, use_graph=False)
    assert torch.equal(eager.forward(x)[0], outs[0])           # the captured two-stream schedule computes the eager bits
    with pytest.raises(ValueError, match="planned for input"):
        e.forward(x[:, :, :64])


def test_engine_refusals_on_the_device():
    from centerpose_amd import engine
    with pytest.raises(ValueError, match="128 x 64"):
        engine.Engine("reid", _sd(), 2, 64, 128)
    sd = {k: v for k, v in _sd().items() if k != "layer3.0.downsample.0.weight"}
    with pytest.raises(KeyError, match="missing"):
        engine.Engine("reid", sd, 2, 128, 64)
    extra = dict(_sd())
    extra["classifier.0.weight"] = torch.zeros(256, 512)       # accepted and ignored
    e = engine.Engine("reid", extra, 1, 128, 64, use_graph=False)
    with pytest.raises(ValueError, match="reid"):
        e.save_plan("/dev/null")


# ---------------------------------------------------------------- 5. ReidExtractor.embed
@functools.lru_cache(maxsize=None)
def _ex(cap=8):
    from centerpose_amd import reid
    return reid.ReidExtractor(_sd(), capacity=cap)


def _frame(seed, H, W):
    """A B, G, R frame with large-scale structure, uint8 [H, W, 3]."""
    r = np.random.RandomState(seed)
    grid = torch.from_numpy(r.uniform(0, 255, (1, 3, 5, 6)))
    up = torch.nn.functional.interpolate(grid, size=(H, W), mode="bilinear", align_corners=False)[0].numpy()
    return np.clip(np.rint(up + r.uniform(-20, 20, up.shape)), 0, 255).astype(np.uint8).transpose(1, 2, 0).copy()


def _rows2():
    rows = np.zeros((2, 4, 56), np.float32)
    for n in range(2):
        rows[n, 0] = reid_ref.row(5, 8, 60, 90)
        rows[n, 1] = reid_ref.row(40, 2, 100, 80, 0.2)         # below the threshold
        rows[n, 2] = reid_ref.row(-10, 30, 50, 140)
        rows[n, 3] = reid_ref.row(70, 20, 127, 95, 0.9)
    return rows


def test_embed_end_to_end_against_the_float64_net():
    """crops by the NumPy rule, the float64 net on them: embed's features are within the forward bar, slot by slot."""
    ex = _ex()
    frames = [_frame(1, 96, 128), _frame(2, 96, 128)]
    rows = _rows2()
    res = ex.embed([torch.from_numpy(f).cuda() for f in frames], torch.from_numpy(rows).cuda())
    want_x, want_slots, want_counts = reid_ref.crops(frames, rows, 0.3, 8)
    assert res.slots.cpu().tolist() == want_slots.tolist() == [0, 2, 3, -1, 4, 6, 7, -1] and res.counts.cpu().tolist() == [3, 3]
    assert reid_util.same_bits(ex.engine.input.cpu().numpy(), want_x)
    with torch.no_grad():
        want = reid_ref.net(_sd(), torch.from_numpy(want_x).double()).numpy()
    used = want_slots >= 0
    d = np.sqrt(((res.features.double().cpu().numpy() - want) ** 2).sum(1))[used]
    print("embed: worst L2 distance to the float64 net %.3e" % d.max())
    assert d.max() <= 1e-3
    feats, valid = res.dense(2, 4)
    assert valid.cpu().tolist() == [[True, False, True, True]] * 2 and tuple(feats.shape) == (2, 4, 512)
    assert torch.equal(feats[0, 2], res.features[1]) and torch.equal(feats[1, 3], res.features[6]) and not bool(feats[:, 1].any())


def test_identical_frames_give_identical_features():
    ex = _ex()
    f = torch.from_numpy(_frame(3, 96, 128)).cuda()
    rows = torch.from_numpy(_rows2()).cuda()
    res = ex.embed(f.unsqueeze(0).expand(2, -1, -1, -1), rows)             # an expanded view: frames are only read
    a, b = res.features[0:3], res.features[4:7]
    assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and res.slots.cpu().tolist() == [0, 2, 3, -1, 4, 6, 7, -1]
    one = ex.embed([f], rows[0])                                           # [M, 56] with one 3-D frame in a list
    assert torch.equal(one.features[0:3], a) and one.counts.cpu().tolist() == [3]


def test_embed_of_nv12_surfaces_equals_embed_of_the_converted_frames():
    ex = _ex()
    r = np.random.RandomState(9)
    H, W = 96, 128
    surfaces, converted = [], []
    for n in range(2):
        y = _frame(20 + n, H, W)[..., 0]
        uv = np.clip(128 + 60 * np.sin(np.arange(H // 2 * W).reshape(H // 2, W) / 97.0) + r.uniform(-8, 8, (H // 2, W)), 0, 255).astype(np.uint8)
        surf = np.concatenate([y, uv], 0)
        surfaces.append(torch.from_numpy(surf).cuda())
        converted.append(yuv_ref.frame_to_bgr((y, uv.reshape(H // 2, W // 2, 2)), "nv12", "bt709"))
    rows = torch.from_numpy(_rows2()).cuda()
    a = ex.embed(surfaces, rows, color="nv12", matrix="bt709")
    b = ex.embed([torch.from_numpy(c).cuda() for c in converted], rows)
    assert torch.equal(a.features, b.features) and torch.equal(a.slots, b.slots) and torch.equal(a.counts, b.counts)
    assert a.counts.cpu().tolist() == [3, 3]


def test_embed_refusals():
    from centerpose_amd import reid
    from centerpose_amd._lib import CenterposeHipError
    ex = _ex()
    rows = torch.from_numpy(_rows2()).cuda()
    with pytest.raises(ValueError, match="device frames"):
        ex.embed([_frame(1, 96, 128)] * 2, rows)
    with pytest.raises(ValueError, match="device frames"):
        ex.embed([(np.zeros((96, 128), np.uint8), np.zeros((48, 64, 2), np.uint8))] * 2, rows, color="nv12")
    f = torch.from_numpy(_frame(1, 96, 128)).cuda()
    with pytest.raises(ValueError, match="capacity of 8"):
        ex.embed([f] * 9, torch.zeros((9, 2, 56), device="cuda"))
    with pytest.raises(CenterposeHipError, match="rows hold 2 blocks for 1 frames"):
        ex.embed([f], rows)
    with pytest.raises(CenterposeHipError, match="float32"):
        ex.embed([f, f], rows.double())
    with pytest.raises(CenterposeHipError):
        ex.embed([f, f], rows.cpu())
    for bad in (dict(capacity=0), dict(capacity=4097), dict(channel_order="gbr")):
        with pytest.raises(ValueError):
            reid.ReidExtractor(_sd(), **bad)


# ---------------------------------------------------------------- 6. run_batch(embed=)
def test_run_batch_with_embed():
    from centerpose_amd import config, detector
    det = detector.MultiPoseDetector(config.get_cfg("dla_34", TEST__FIX_RES=False))
    ex = _ex()
    vis = float(det.cfg.TEST.VIS_THRESH)
    frames = [torch.from_numpy(_frame(31 + n, 96, 128)).cuda() for n in range(2)]
    plain = det.run_batch(frames, return_device=True)
    rows, res = det.run_batch(frames, return_device=True, embed=ex)
    assert torch.equal(rows, plain)
    assert int(res.counts.sum()) > 0 and int((plain[..., 4] > vis).sum()) > 0       # the synthetic detector finds something to embed
    feats, slots, counts = res.features.clone(), res.slots.clone(), res.counts.clone()
    direct = ex.embed(frames, plain, vis_thresh=vis)
    assert torch.equal(direct.features, feats) and torch.equal(direct.slots, slots) and torch.equal(direct.counts, counts)
    # the host-list form returns the same rows beside the result
    listed, res2 = det.run_batch(frames, embed=ex)
    assert listed == det.run_batch(frames) and torch.equal(res2.features, feats)
    # with draw=True the crops are taken before anything is painted
    painted = [f.clone() for f in frames]
    rows3, res3 = det.run_batch(painted, return_device=True, embed=ex, draw=True)
    assert torch.equal(rows3, plain) and torch.equal(res3.features, feats) and torch.equal(res3.slots, slots)
    assert any(not torch.equal(p, f) for p, f in zip(painted, frames))            # ... and the frames were painted
    with pytest.raises(ValueError, match="capacity"):
        det.run_batch([frames[0]] * 9, embed=ex)
