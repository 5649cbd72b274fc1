"""GPU: run_batch and its stages (csrc/batch_stages.hip) -- the batched pre-process bit for bit against the per-image oracle, the
batched post-process against post_process, soft-NMS on the device against the vectors of the reference's own source and the host
function, and run_batch against run() per image.

Criteria for soft-NMS on the device ("the NMS criteria" below): every column but 4 and the kept count bit-equal; column 4 bit-equal for
methods 0 / 1 and within 5e-6 relative for method 2 (the device's double exp may round its last bit differently from the host C
library's, once per decay -- the tolerance tests/golden/make_golden_nms.py documents for its own 1-ulp exp difference)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import prepost_np as pp

pytestmark = pytest.mark.gpu

MEAN, STD = [0.408, 0.447, 0.470], [0.289, 0.274, 0.278]


def _img(seed, h, w):
    return (np.random.RandomState(seed).rand(h, w, 3) * 255).astype(np.uint8)


def _det(arch, **over):
    from centerpose_amd import config, detector
    return detector.MultiPoseDetector(config.get_cfg(arch, **over))


def _assert_nms_equal(got, want, method, what=""):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    other = [c for c in range(56) if c != 4]
    assert np.array_equal(got[..., other], want[..., other]), what
    if method == 2:
        err = np.abs(got[..., 4].astype(np.float64) - want[..., 4]) / np.maximum(np.abs(want[..., 4].astype(np.float64)), 1e-30)
        print("%s: column 4 max relative difference %.3e" % (what, float(err.max())))
        assert float(err.max()) <= 5e-6, what
    else:
        assert np.array_equal(got[..., 4], want[..., 4]), what


def _margins(boxes, sigma=0.5, Nt=0.3, threshold=0.001, method=0):
    """Instrumented restatement of the host soft_nms_39 loop: (closest two candidates of any arg-max step, closest decayed score to the
    threshold), both relative -- how far the input is from a decision a last-bit exp difference could change."""
    b = boxes.copy()
    f32, one = np.float32, np.float32(1)
    sigma, Nt, threshold = f32(sigma), f32(Nt), f32(threshold)
    N, gap, thr = b.shape[0], np.inf, np.inf
    for i in range(b.shape[0]):
        if i < N - 1:
            sc = np.sort(b[i:N, 4].astype(np.float64))[::-1]
            gap = min(gap, (sc[0] - sc[1]) / max(abs(sc[0]), 1e-30))
        mp = i + int(np.argmax(b[i:N, 4])) if i < N else i
        t = b[i, :39].copy(); b[i, :39] = b[mp, :39]; b[mp, :39] = t
        tx1, ty1, tx2, ty2 = b[i, :4]
        pos = i + 1
        while pos < N:
            x1, y1, x2, y2 = b[pos, :4]
            area = (x2 - x1 + one) * (y2 - y1 + one)
            iw = min(tx2, x2) - max(tx1, x1) + one
            if iw > 0:
                ih = min(ty2, y2) - max(ty1, y1) + one
                if ih > 0:
                    ov = iw * ih / ((tx2 - tx1 + one) * (ty2 - ty1 + one) + area - iw * ih)
                    if method == 1:
                        w = one - ov if ov > Nt else one
                    elif method == 2:
                        w = f32(np.exp(np.float64(-(ov * ov) / sigma)))
                    else:
                        w = f32(0) if ov > Nt else one
                    b[pos, 4] = w * b[pos, 4]
                    thr = min(thr, abs(float(b[pos, 4]) - float(threshold)) / float(threshold))
                    if b[pos, 4] < threshold:
                        b[pos, :5] = b[N - 1, :5]
                        q = b[pos, 5:39].copy(); b[pos, 5:39] = b[N - 1, 5:39]; b[N - 1, 5:39] = q
                        N -= 1
                        pos -= 1
            pos += 1
    return gap, thr, b, N


def _device_nms(boxes_list, **kw):
    """[N images of [R,56]] through cp_post_merge_batch_f32 (one scale, rows already mapped) -> (rows [N,R,56], n_keep [N]) on the host."""
    from centerpose_amd import detector
    d = torch.from_numpy(np.stack(boxes_list)).cuda()
    out, keep = detector.post_merge_batch([d], nms=True, **kw)
    return out.cpu().numpy(), keep.cpu().numpy()


# ---------------------------------------------------------------- 1. pre_process_batch
SIZES = [(217, 333), (480, 640), (96, 128), (301, 200)]       # 333: odd width


@pytest.mark.parametrize("arch,fix_res,flip", [("res_50", True, True), ("res_50", True, False), ("dla_34", False, True), ("hrnet", False, False)])
@pytest.mark.parametrize("scale", [1, 0.5, 2, 0.75])
def test_pre_process_batch_bit_exact_vs_oracle(arch, fix_res, flip, scale):
    det = _det(arch, TEST__FIX_RES=fix_res, TEST__FLIP_TEST=flip)
    images = [_img(10 + i, h, w) for i, (h, w) in enumerate(SIZES)]
    nb = 2 if flip else 1
    if fix_res:
        batches = [images]                                   # every size lands in one input shape
    else:                                                    # one input shape per call: the same-shape runs of a mixed list
        by_shape = {}
        for im in images:
            by_shape.setdefault(det.input_geometry(im.shape[0], im.shape[1], scale)[2:4], []).append(im)
        batches = list(by_shape.values())
        batches.append([_img(20, 217, 333), _img(21, 220, 335), _img(22, 217, 333)])       # two sizes, one padded input shape
    for batch in batches:
        x, metas = det.pre_process_batch(batch, scale)
        assert x.is_cuda and x.shape[0] == nb * len(batch) and len(metas) == len(batch)
        got = x.cpu().numpy()
        for n, im in enumerate(batch):
            ref, rmeta = pp.pre_process(im, scale, MEAN, STD, fix_res=fix_res, flip_test=flip)
            assert np.array_equal(got[nb * n:nb * n + nb], ref), (n, im.shape)
            assert set(metas[n]) == set(rmeta) and all(np.array_equal(np.asarray(metas[n][k]), np.asarray(rmeta[k])) for k in rmeta)
            one, _ = det.pre_process(im, scale)
            assert np.array_equal(got[nb * n:nb * n + nb], one.cpu().numpy())


@pytest.mark.parametrize("flip", [True, False])
def test_pre_process_batch_scalar_store_path(flip):
    """A network input width that is not a multiple of 4 takes the scalar store path."""
    from centerpose_amd import _lib
    det = _det("res_50", TEST__FIX_RES=True, TEST__FLIP_TEST=flip, MODEL__INPUT_W=254, MODEL__INPUT_H=192)
    images = [_img(30 + i, h, w) for i, (h, w) in enumerate(SIZES[:3])]
    for scale in (1, 0.75):
        x, _ = det.pre_process_batch(images, scale)
        assert _lib.lib().cp_last_kernel() == b"preprocess_batch_kernel<scalar>"
        got = x.cpu().numpy()
        nb = 2 if flip else 1
        for n, im in enumerate(images):
            one, _ = det.pre_process(im, scale)
            assert one.shape[3] == 254 and np.array_equal(got[nb * n:nb * n + nb], one.cpu().numpy())
    x, _ = _det("res_50", TEST__FLIP_TEST=flip).pre_process_batch(images, 1)
    assert _lib.lib().cp_last_kernel() == b"preprocess_batch_kernel<vec4>"


def test_pre_process_batch_rejects_mixed_input_shapes_and_floats():
    from centerpose_amd._lib import CenterposeHipError
    det = _det("dla_34", TEST__FIX_RES=False)
    with pytest.raises(CenterposeHipError, match="input shape"):
        det.pre_process_batch([_img(1, 96, 128), _img(2, 217, 333)], 1)
    with pytest.raises(CenterposeHipError):
        det.pre_process_batch([np.zeros((10, 10, 3), np.float32)], 1)


# ---------------------------------------------------------------- 2. post_process_batch
def _metas(N):
    base = [{"c": np.array([320., 240.], np.float32), "s": 640.0, "out_height": 128, "out_width": 128},
            {"c": np.array([640., 480.], np.float32), "s": np.array([1312., 992.], np.float32), "out_height": 248, "out_width": 328},
            {"c": np.array([166., 108.], np.float32), "s": np.array([352., 224.], np.float32), "out_height": 56, "out_width": 88},
            {"c": np.array([100., 150.], np.float32), "s": 301.0, "out_height": 128, "out_width": 128},
            {"c": np.array([64., 48.], np.float32), "s": np.array([128., 96.], np.float32), "out_height": 24, "out_width": 32}]
    return base[:N]


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("scale", [1, 2, 0.75])
def test_post_process_batch_vs_post_process_and_oracle(N, scale):
    det = _det("res_50", TEST__FLIP_TEST=False)
    d = (np.random.RandomState(40 + N).rand(N, 100, 56) * 128).astype(np.float32)
    metas = _metas(N)
    dev = torch.from_numpy(d).cuda()
    got = det.post_process_batch(dev, metas, scale)
    assert got.is_cuda and tuple(got.shape) == (N, 100, 56)
    got = got.cpu().numpy()
    for n in range(N):
        one = det.post_process(dev[n:n + 1], metas[n], scale)[1]
        assert np.array_equal(got[n], one), n
        ref = pp.post_process(d[n:n + 1], metas[n], scale)
        assert np.array_equal(got[n][:, 4], ref[:, 4]) and np.array_equal(got[n][:, 39:], ref[:, 39:])
        assert np.abs(got[n] - ref).max() <= 2e-4


def test_post_process_batch_vs_reference_source_golden(golden_dir):
    sys.path.insert(0, golden_dir)
    import make_golden_post as mg
    gold = np.load(os.path.join(golden_dir, "post_process.npz"))
    det = _det("res_50", TEST__FLIP_TEST=False)
    by_shape = {}
    for name, (d, m, scale) in mg.cases().items():
        by_shape.setdefault((d.reshape(1, -1, 56).shape[1], float(scale)), []).append((name, d.reshape(-1, 56), m))
    seen = 0
    for (K, scale), items in by_shape.items():            # the cases of one row count and scale as ONE batch
        dets = torch.from_numpy(np.stack([d for _, d, _ in items])).cuda()
        got = det.post_process_batch(dets, [m for _, _, m in items], scale).cpu().numpy()
        for n, (name, _, _) in enumerate(items):
            exp = gold[name]
            assert got[n].shape == exp.shape and np.array_equal(got[n][:, 4], exp[:, 4]) and np.array_equal(got[n][:, 39:], exp[:, 39:]), name
            assert np.abs(got[n] - exp).max() <= 2e-4, (name, float(np.abs(got[n] - exp).max()))
            seen += 1
    assert seen == len(mg.cases())


# ---------------------------------------------------------------- 3. soft-NMS on the device
def _nms_golden(golden_dir):
    sys.path.insert(0, golden_dir)
    import make_golden_nms as mg
    return mg.cases(), np.load(os.path.join(golden_dir, "soft_nms_39.npz"))


def test_device_soft_nms_vs_reference_source_golden(golden_dir):
    cases, gold = _nms_golden(golden_dir)
    assert len(cases) == 7
    for name, (boxes, kw) in cases.items():
        out, keep = _device_nms([boxes], **kw)
        assert int(keep[0]) == len(gold[name + "__keep"]), name
        _assert_nms_equal(out[0], gold[name + "__out"], kw.get("method", 0), name)


def test_device_soft_nms_three_images_one_launch(golden_dir):
    """The three rand60 box sets in ONE launch with method 2: image 2 is the golden's own case, images 0 and 1 (the box sets of the
    method-0 and method-1 cases, here run with method 2) against the host function -- after asserting from the host run that no
    decision of theirs lies within 1e-4 relative of changing."""
    from centerpose_amd.detector import soft_nms_39
    cases, gold = _nms_golden(golden_dir)
    sets = [cases["rand60_m%d" % m][0] for m in (0, 1, 2)]
    kw = dict(sigma=0.5, Nt=0.5, threshold=0.05, method=2)
    assert cases["rand60_m2"][1] == kw
    out, keep = _device_nms(sets, **kw)
    _assert_nms_equal(out[2], gold["rand60_m2__out"], 2, "image 2 vs golden")
    assert int(keep[2]) == len(gold["rand60_m2__keep"])
    for n in (0, 1):
        gap, thr, _, _ = _margins(sets[n], **kw)
        print("image %d: arg-max gap %.3e, threshold distance %.3e" % (n, gap, thr))
        assert gap > 1e-4 and thr > 1e-4
        host = sets[n].copy()
        k = soft_nms_39(host, **kw)
        assert int(keep[n]) == len(k)
        _assert_nms_equal(out[n], host, 2, "image %d vs host" % n)


def _random_rows(seed, R, spread):
    r = np.random.RandomState(seed)
    b = r.rand(R, 56).astype(np.float32)
    b[:, 0:2] *= spread
    b[:, 2:4] = b[:, 0:2] + (r.rand(R, 2) * 60 + 20).astype(np.float32)
    # scores: a shuffled geometric ladder (2 % steps, jittered), so that neighbours in the ranking are far apart on the scale of a
    # float bit and the low end lies under the thresholds used here (discards happen)
    ladder = 0.97 * 0.98 ** (np.arange(R) * (400.0 / R)) * (1 + 0.004 * r.rand(R))
    b[:, 4] = r.permutation(ladder).astype(np.float32)
    return b


@pytest.mark.parametrize("method", [0, 1, 2])
def test_device_soft_nms_512_rows_and_the_limit(method):
    from centerpose_amd import _lib, detector
    from centerpose_amd.detector import soft_nms_39
    assert _lib.lib().cp_post_merge_max_rows() == 512
    kw = dict(sigma=0.5, Nt=0.5, threshold=0.01, method=method)
    b = _random_rows(71, 512, 900.0)                         # the seed is chosen so that the margins below hold
    gap, thr, _, kept = _margins(b, **kw)
    print("R = 512 method %d: arg-max gap %.3e, threshold distance %.3e, kept %d" % (method, gap, thr, kept))
    assert gap > 1e-4 and thr > 1e-4 and kept < 512
    host = b.copy()
    k = soft_nms_39(host, **kw)
    out, keep = _device_nms([b, b[::-1].copy()], **kw)
    assert int(keep[0]) == len(k)
    _assert_nms_equal(out[0], host, method, "R = 512")
    with pytest.raises(_lib.CenterposeHipError, match="at most 512 rows"):
        detector.post_merge_batch([torch.zeros((1, 513, 56), device="cuda")], nms=True)


# ---------------------------------------------------------------- 4. merge_outputs_batch
@pytest.mark.parametrize("arch,S", [("dla_34", 1), ("hrnet", 2), ("res_50", 1)])
def test_merge_outputs_batch_vs_merge_outputs(arch, S):
    det = _det(arch)
    nms = det.cfg.TEST.NMS or len(det.cfg.TEST.TEST_SCALES) > 1
    assert len(det.cfg.TEST.TEST_SCALES) == S and nms == (arch != "res_50")
    N, K = 3, 100
    per_scale = []
    for s in range(S):                                       # seeds chosen so that the margins asserted below hold
        rows = np.stack([_random_rows(seed + 1000 * s, K, 500.0) for seed in (104, 113, 150)])
        per_scale.append(rows)
    for n in range(N):                                       # new random inputs: far from any decision an exp bit could change
        gap, thr, _, _ = _margins(np.concatenate([p[n] for p in per_scale], 0), Nt=0.5, method=2)
        assert gap > 1e-4 and thr > 1e-4
    got = det.merge_outputs_batch([torch.from_numpy(p).cuda() for p in per_scale])
    assert got.is_cuda and tuple(got.shape) == (N, S * K, 56)
    got = got.cpu().numpy()
    for n in range(N):
        want = np.array(det.merge_outputs([{1: p[n]} for p in per_scale]), np.float32)
        if nms:
            _assert_nms_equal(got[n], want, 2, "%s image %d" % (arch, n))
        else:
            assert np.array_equal(got[n], want)


# ---------------------------------------------------------------- 5. run_batch == run per image (batch-invariant plans)
def _assert_results(got, want, nms, what):
    assert set(got) == {1}
    g, w = np.array(got[1], np.float32), np.array(want[1], np.float32)
    if nms:
        _assert_nms_equal(g, w, 2, what)
    else:
        assert np.array_equal(g, w), what


@pytest.mark.parametrize("arch,sizes", [("res_50", [(480, 640), (96, 128), (217, 333), (480, 640)]),
                                        ("dla_34", [(200, 264), (96, 128), (200, 264), (96, 128)]),
                                        ("hrnet", [(120, 160), (96, 128), (120, 160), (96, 128)])])
def test_run_batch_equals_run_per_image(arch, sizes, monkeypatch):
    from centerpose_amd import ops
    monkeypatch.setattr(ops, "BATCH_INVARIANT", True)
    det = _det(arch)
    nms = det.cfg.TEST.NMS or len(det.cfg.TEST.TEST_SCALES) > 1
    images = [_img(50 + i, h, w) for i, (h, w) in enumerate(sizes)]
    groups = det._batch_groups(sizes)
    assert len(groups) == (1 if det.cfg.TEST.FIX_RES else 2)
    got = det.run_batch(images)
    assert len(got) == 4
    for n, im in enumerate(images):
        _assert_results(got[n], det.run(im)["results"], nms, "%s image %d" % (arch, n))


# ---------------------------------------------------------------- 6. run_batch == its own stages (default mode, shipped dla_34, N = 8)
def test_run_batch_shipped_dla34_eight_images_stage_by_stage():
    det = _det("dla_34")
    assert det.cfg.TEST.FLIP_TEST and det.cfg.TEST.NMS and not det.cfg.TEST.FIX_RES
    images = [_img(60 + i, 480, 640) for i in range(8)]
    got = det.run_batch(images)
    x, metas = det.pre_process_batch(images, 1)
    assert tuple(x.shape) == (16, 3, 512, 672)
    _, dets = det.process(x)
    assert tuple(dets.shape) == (8, 100, 56)
    merged = det.merge_outputs_batch([det.post_process_batch(dets, metas, 1)]).cpu().numpy()
    for n in range(8):
        assert np.array_equal(np.array(got[n][1], np.float32), merged[n]), n
    assert len(det.model._engines) == 1


# ---------------------------------------------------------------- 7. no stale staging, no new plans
def test_run_batch_twice_fresh_results_and_no_new_plan(monkeypatch):
    from centerpose_amd import ops
    monkeypatch.setattr(ops, "BATCH_INVARIANT", True)
    det = _det("dla_34")
    a = [_img(70 + i, 96, 128) for i in range(3)]
    b = [_img(80 + i, 96, 128) for i in range(3)]
    ra = det.run_batch(a)
    plans = len(det.model._engines)
    rb = det.run_batch(b)
    assert len(det.model._engines) == plans
    assert all(x != y for x, y in zip(ra, rb))
    for imgs, res in ((a, ra), (b, rb)):
        for n, im in enumerate(imgs):
            _assert_results(res[n], det.run(im)["results"], True, "image %d" % n)
    assert det.run_batch(a) == ra
    assert det.run_batch([]) == []
