"""GPU: detections-only inference under the flip test -- cp_head_points_pairs_f32 (wh / hps / reg / hp_offset of N image / mirrored-twin
pairs evaluated and merged at the peaks of the merged heat maps) bit for bit against cp_head_points_f32 on both sides plus the merge on
the host, and against an fp64 CPU restatement; the flip_dets_only plans (Engine / plan files / the C plan runtime / the detector's
process_dets and run_batch(dets_only=True)) against the dense flip-test plans."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SPARSE = ("wh", "hps", "reg", "hp_offset")
NOUT = {"wh": 2, "hps": 34, "reg": 2, "hp_offset": 2}
N, J, K, H = 3, 17, 16, 20


def _perm():
    from centerpose_amd import engine
    perm = list(range(J))
    for a, b in engine.FLIP_IDX:
        perm[a], perm[b] = b, a
    return perm


def _branch_weights(C, hc, seed):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in SPARSE:
        n = NOUT[name]
        out[name] = (torch.randn(hc, C, 3, 3, generator=g) / (3.0 * C ** 0.5), torch.randn(hc, generator=g) * 0.1,
                     torch.randn(n, hc, 1, 1, generator=g) / hc ** 0.5, torch.randn(n, generator=g) * 0.1)
    return out


def _dense_fp64(feat_nhwc, wts):
    """the four dense maps in fp64 on the CPU: 3x3 (pad 1) + bias + ReLU -> 1x1 + bias (keypoint.py:14-37)."""
    x = feat_nhwc.double().permute(0, 3, 1, 2)
    maps = {}
    for name, (w3, b3, w2, b2) in wts.items():
        hid = torch.relu(torch.nn.functional.conv2d(x, w3.double(), b3.double(), padding=1))
        maps[name] = torch.nn.functional.conv2d(hid, w2.double(), b2.double())
    return maps


def _point_list(B, H, W, J, K, seed):
    """[B, 1+J, K] flat indices: every border and corner (so x = 0 <-> W - 1), duplicates, a joint index equal to a centre index, one
    centre index in the class plane above the first (taken % (H*W), as pose_assign_kernel does)."""
    r = np.random.RandomState(seed)
    HW = H * W
    special = [0, W - 1, (H - 1) * W, HW - 1, W // 2, (H // 2) * W, (H // 2) * W + W - 1, (H - 1) * W + W // 2]
    inds = r.randint(0, HW, size=(B, 1 + J, K))
    for b in range(B):
        inds[b, 0, :len(special)] = special
        inds[b, 0, len(special)] = inds[b, 0, len(special) + 1]           # duplicated centre
        inds[b, 0, len(special) + 2] = HW + 5                              # -> pixel 5
        inds[b, 1, 0] = inds[b, 0, 3]                                      # joint peak == centre peak
        inds[b, 2, 1] = inds[b, 3, 1] = inds[b, 4, 4]                      # one pixel, three joints
        inds[b, 1 + J - 1, :len(special)] = special[::-1]
    return torch.from_numpy(inds.astype(np.int32))


def _consts(wts, hc, dev):
    from centerpose_amd import ops
    w1 = torch.cat([ops.pack_head_points_weight(wts[n][0]) for n in SPARSE]).to(dev)
    b1 = torch.cat([wts[n][1] for n in SPARSE]).to(dev)
    w2 = torch.cat([wts[n][2].reshape(-1, hc) for n in SPARSE]).contiguous().to(dev)
    b2 = torch.cat([wts[n][3] for n in SPARSE]).to(dev)
    return w1, b1, w2, b2


def _split(out, B, H, W):
    maps, off = {}, 0
    for name in SPARSE:
        n = NOUT[name]
        maps[name] = out[off:off + B * n * H * W].view(B, n, H, W).cpu()
        off += B * n * H * W
    return maps


def _run_points(feat, wts, inds, hc, K):
    """cp_head_points_f32 on every image of `feat` (the existing kernel), NaN where nothing is written."""
    from centerpose_amd import ops
    B, H, W, _ = feat.shape
    out = torch.full((B * H * W * (6 + 2 * J),), float("nan"), device=feat.device)
    ws = inds.to(torch.int32).contiguous().view(torch.float32).to(feat.device)
    ops.head_points_launch(feat, ws, *_consts(wts, hc, feat.device), out, hc=hc, J=J, K=K).run()
    torch.cuda.synchronize()
    return _split(out, B, H, W)


def _run_pairs(feat, wts, inds, hc, K):
    """cp_head_points_pairs_f32 on the pairs of `feat`, NaN where nothing is written; -> (maps, kernel name)."""
    from centerpose_amd import ops
    B, H, W, _ = feat.shape
    out = torch.full((B // 2 * H * W * (6 + 2 * J),), float("nan"), device=feat.device)
    ws = inds.to(torch.int32).contiguous().view(torch.float32).to(feat.device)
    perm = torch.tensor(_perm(), dtype=torch.int32, device=feat.device).view(torch.float32)
    launch = ops.head_points_pairs_launch(feat, ws, perm, *_consts(wts, hc, feat.device), out, hc=hc, J=J, K=K)
    launch.run()
    torch.cuda.synchronize()
    return _split(out, B // 2, H, W), launch.kernel


def _merge(maps, dtype):
    """flip_merge_kernel's arithmetic on the [2N] maps of both sides (image rows of maps[0], twin rows of maps[1]) in `dtype`:
    (a + b * sign) / 2 with the joint permutation for wh / hps, the image's value for reg / hp_offset -> [N] maps."""
    img, twin = maps
    perm = _perm()
    cs = [2 * perm[c >> 1] + (c & 1) for c in range(2 * J)]
    sign = torch.tensor([-1.0 if c % 2 == 0 else 1.0 for c in range(2 * J)], dtype=dtype).view(1, -1, 1, 1)
    two = torch.tensor(2.0, dtype=dtype)
    out = {}
    a, b = img["wh"][0::2].to(dtype), torch.flip(twin["wh"][1::2].to(dtype), [3])
    out["wh"] = (a + b * 1.0) / two
    a, b = img["hps"][0::2].to(dtype), torch.flip(twin["hps"][1::2].to(dtype), [3])[:, cs]
    out["hps"] = (a + b * sign) / two
    out["reg"] = img["reg"][0::2].to(dtype)
    out["hp_offset"] = img["hp_offset"][0::2].to(dtype)
    return out


@functools.lru_cache(maxsize=None)
def _case(W, C, hc):
    """One shape, computed once and shared (read-only) by the tests below: the feature map of 2N images, the weights, the point list
    and the pairs kernel's output."""
    torch.manual_seed(C + hc + W)
    feat_cpu = torch.randn(2 * N, H, W, C)
    wts = _branch_weights(C, hc, seed=C * 7 + hc)
    inds = _point_list(N, H, W, J, K, seed=C + hc + W)
    got, kernel = _run_pairs(feat_cpu.cuda(), wts, inds, hc, K)
    return feat_cpu, wts, inds, got, kernel


def _addressed(inds, name, W):
    HW = H * W
    mask = torch.zeros(N, 1, H, W, dtype=torch.bool)
    for b in range(N):
        where = inds[b, 1:].reshape(-1) if name == "hp_offset" else inds[b, 0] % HW
        mask.view(N, HW)[b, where.long()] = True
    return mask.expand(-1, NOUT[name], -1, -1)


SHAPES = [(W, C, hc) for W in (24, 21) for C, hc in ((64, 256), (256, 64), (32, 64))]


@pytest.mark.parametrize("W,C,hc", SHAPES)
def test_pairs_kernel_bit_equal_to_both_sides_of_the_existing_kernel(W, C, hc):
    feat_cpu, wts, inds, got, kernel = _case(W, C, hc)
    assert kernel == ("head_points_pairs_kernel<2>" if hc >= 128 else "head_points_pairs_kernel<1>")
    HW = H * W
    feat = feat_cpu.cuda()
    # side by side on the 2N images with the existing kernel: the pair's indices on the image rows, the mirrored ones on the twin rows
    p = inds.long() % HW
    mirrored = ((p // W) * W + (W - 1 - p % W)).to(torch.int32)
    img_inds, twin_inds = torch.zeros(2 * N, 1 + J, K, dtype=torch.int32), torch.zeros(2 * N, 1 + J, K, dtype=torch.int32)
    img_inds[0::2] = inds
    img_inds[1::2] = inds                  # (the twin rows of this run and the image rows of the next are not read below)
    twin_inds[0::2] = mirrored
    twin_inds[1::2] = mirrored
    want = _merge((_run_points(feat, wts, img_inds, hc, K), _run_points(feat, wts, twin_inds, hc, K)), torch.float32)
    for name in SPARSE:
        g, w = got[name], want[name]
        mask = _addressed(inds, name, W)
        assert torch.isnan(g[~mask]).all(), name           # only the addressed pixels are written
        assert torch.isfinite(g[mask]).all() and torch.isfinite(w[mask]).all(), name
        assert torch.equal(g[mask], w[mask]), "%s: %d of %d values differ" % (name, int((g[mask] != w[mask]).sum()), int(mask.sum()))

    # the same pixels from a shuffled point list padded with duplicates: bit-identical values
    gen = torch.Generator().manual_seed(11)
    K2 = K + 9
    inds2 = torch.empty(N, 1 + J, K2, dtype=torch.int32)
    for b in range(N):
        for row in range(1 + J):
            order = torch.randperm(K, generator=gen)
            extra = torch.randint(0, K, (K2 - K,), generator=gen)
            inds2[b, row] = torch.cat([inds[b, row][order], inds[b, row][extra]])
    got2, _ = _run_pairs(feat, wts, inds2, hc, K2)
    for name in SPARSE:
        fin = torch.isfinite(got[name])
        assert torch.equal(fin, torch.isfinite(got2[name])), name
        assert torch.equal(got[name][fin], got2[name][fin]), name


@pytest.mark.parametrize("W,C,hc", SHAPES)
def test_pairs_kernel_vs_fp64(W, C, hc):
    feat_cpu, wts, inds, got, _ = _case(W, C, hc)
    dense = _dense_fp64(feat_cpu, wts)
    ref = _merge((dense, dense), torch.float64)
    for name in SPARSE:
        mask = _addressed(inds, name, W)
        g, r = got[name], ref[name]
        err = (g[mask].double() - r[mask]).abs().max().item()
        print("%s W=%d C=%d hc=%d: max error %.3e, bound %.3e" % (name, W, C, hc, err, 1e-4 * r.abs().max().item()))
        assert err <= 1e-4 * r.abs().max().item(), "%s: %.3e" % (name, err)


# ---------------------------------------------------------------- plans
def _pairs(n, h, w, seed):
    """n images and their mirrored twins, interleaved: image i at 2i, twin at 2i + 1."""
    from centerpose_amd import synth
    img = synth.make_images(n, h, w, seed=seed)
    return torch.stack([img, torch.flip(img, [3])], 1).reshape(2 * n, 3, h, w)


def _topk_ws(eng):
    topk = [l for _, _, _, l in eng.launches if l.fn == "cp_decode_topk_f32"][0]
    return topk.tensors[2], topk.tensors[3].view(torch.int32)


def _assert_dets_close(dd, ds, what):
    """the dense-against-points criteria of test_dets_only_engine_vs_dense on two dets tensors [N, K, 56]"""
    dd, ds = dd.cpu(), ds.cpu()
    assert dd.shape == ds.shape
    assert torch.equal(dd[..., 4], ds[..., 4]) and torch.equal(dd[..., 39:], ds[..., 39:]), what
    assert (dd[..., :4] - ds[..., :4]).abs().max().item() <= 1e-3, what
    kp_close = ((dd[..., 5:39] - ds[..., 5:39]).abs() <= 1e-3).float().mean().item()
    print("%s: keypoint coordinates within 1e-3: %.5f" % (what, kp_close))
    assert kp_close >= 0.995, (what, kp_close)


@pytest.mark.parametrize("arch,n", [("dla_34", 2), ("hrnet", 2), ("res_50", 1)])
def test_flip_dets_only_engine_vs_dense_flip_plan(arch, n):
    from centerpose_amd import engine, synth
    S = 256
    sd = synth.make_state_dict(arch, seed=317)
    x = _pairs(n, S, S, seed=21).cuda()
    dense = engine.Engine(arch, sd, 2 * n, S, S, decode_k=100, flip_test=True)
    sparse = engine.Engine(arch, sd, 2 * n, S, S, decode_k=100, flip_dets_only=True)
    assert sparse.flip_test and sparse.dets_only and sparse.dets.shape == (n, 100, 56)
    names = [name for _, name, _, _ in sparse.emission]
    assert "flip.merge_peaks" in names and "flip.merge_regress" not in names and names[-2:] == ["head_points_pairs", "decode.pose_assign"]
    assert names.index("flip.merge_peaks") < names.index("decode.nms_topk") < names.index("head_points_pairs")
    outs_d, dets_d = dense.process(x)
    outs_s, dets_s = sparse.process(x)
    torch.cuda.synchronize()
    assert [o is None for o in outs_s] == [False, True, True, True, False, True]
    assert outs_s[0].shape[0] == outs_s[4].shape[0] == 2 * n
    assert torch.equal(outs_d[0], outs_s[0]) and torch.equal(outs_d[4], outs_s[4])
    sc_d, in_d = _topk_ws(dense)
    sc_s, in_s = _topk_ws(sparse)
    assert tuple(in_s.shape) == (n, 18, 100)
    assert torch.equal(in_d, in_s) and torch.equal(sc_d, sc_s)
    _assert_dets_close(dets_d, dets_s, arch)
    # the dense merged maps at the decoded peaks vs the pairs kernel's values there
    regress = [l for _, name, _, l in dense.launches if name == "flip.merge_regress"][0]
    merged = dict(zip((1, 2, 3, 5), regress.tensors[4:8]))
    Hm, Wm = outs_d[0].shape[2:]
    ind = in_d.cpu().long()
    centre, joints = ind[:, 0] % (Hm * Wm), ind[:, 1:].reshape(n, -1)
    for i, name in ((1, "wh"), (2, "hps"), (3, "reg"), (5, "hp_offset")):
        d = merged[i].cpu().reshape(n, merged[i].shape[1], -1)
        assert tuple(sparse.head_maps[i].shape) == tuple(merged[i].shape)
        s = sparse.head_maps[i].cpu().reshape(n, merged[i].shape[1], -1)
        at = joints if name == "hp_offset" else centre
        idx = at[:, None, :].expand(-1, d.shape[1], -1)
        dv, sv = d.gather(2, idx), s.gather(2, idx)
        assert torch.isfinite(sv).all(), name
        err = (dv - sv).abs().max().item()
        assert err <= 1e-4 * max(d.abs().max().item(), 1.0), "%s %s: %.3e" % (arch, name, err)


def test_flip_dets_only_poisoned_storage():
    """NaN in every element of the sparse-map storage before a replay: the detections do not change (every pixel the decode reads is
    written in the same step), and further replays are bit-stable."""
    from centerpose_amd import engine, synth
    sd = synth.make_state_dict("dla_34", seed=317)
    x = _pairs(2, 256, 256, seed=4).cuda()
    eng = engine.Engine("dla_34", sd, 4, 256, 256, decode_k=100, flip_dets_only=True)
    want = eng.process(x)[1].clone()
    pts = [l for _, _, _, l in eng.launches if l.fn == "cp_head_points_pairs_f32"]
    assert len(pts) == 1 and not [l for _, _, _, l in eng.launches if l.fn == "cp_head_points_f32"]
    pts[0].out.fill_(float("nan"))
    got = [eng.process(x)[1].clone() for _ in range(3)]
    torch.cuda.synchronize()
    assert torch.isfinite(want).all()
    for g in got:
        assert torch.equal(g, want)


def test_flip_dets_only_plan_round_trip(tmp_path):
    from centerpose_amd import cplan, engine, plan, synth
    sd = synth.make_state_dict("dla_34", seed=317)
    n, S, Kd = 2, 128, 100
    x, x2 = _pairs(n, S, S, seed=9).cuda(), _pairs(n, S, S, seed=10).cuda()
    eng = engine.Engine("dla_34", sd, 2 * n, S, S, decode_k=Kd, flip_dets_only=True)
    want = eng.process(x)[1].clone()
    want2 = eng.process(x2)[1].clone()
    assert want.shape == (n, Kd, 56)
    path = str(tmp_path / "flip_dets_only.cpplan")
    eng.save_plan(path)
    blob = np.fromfile(path, dtype=np.uint8)
    assert bytes(blob[:8]) == b"CPPLAN04"
    meta = plan.parse(memoryview(blob))["meta"]
    assert meta.get("dets_only") is True and meta.get("flip_test") is True
    loaded = plan.load_plan(path)
    outs, d = loaded.process(x)
    assert loaded.dets_only and loaded.flip_test and [o is None for o in outs] == [False, True, True, True, False, True]
    assert torch.equal(d, want)
    cp = cplan.CPlan(path)
    assert cp.dets_only and cp.flip_test and cp.n_outputs == 6
    assert cp._L.cp_plan_dets_only(cp._h) == 1 and cp._L.cp_plan_flip_test(cp._h) == 1
    assert torch.equal(cp.process(x, K=Kd), want)
    with pytest.raises(Exception):
        cp.process(x, K=50)                 # a decode with another K would read pixels nobody wrote
    pipe = cplan.CPipeline(cp, depth=2)
    a, b = pipe.process([x, x2], K=Kd)
    assert torch.equal(a, want) and torch.equal(b, want2)
    pipe.close()
    # a dense flip plan still says dets_only == 0
    dense = engine.Engine("dla_34", sd, 2 * n, S, S, decode_k=Kd, flip_test=True, use_graph=False)
    dpath = str(tmp_path / "dense_flip.cpplan")
    dense.save_plan(dpath)
    assert "dets_only" not in plan.parse(memoryview(np.fromfile(dpath, dtype=np.uint8)))["meta"]
    cd = cplan.CPlan(dpath)
    assert cd.flip_test and not cd.dets_only and cd._L.cp_plan_dets_only(cd._h) == 0
    cp.close()
    cd.close()


# ---------------------------------------------------------------- detector
def test_process_dets_vs_process_under_flip_test():
    from centerpose_amd import config, detector
    det = detector.MultiPoseDetector(config.get_cfg("dla_34"))
    assert det.cfg.TEST.FLIP_TEST
    x = _pairs(2, 256, 256, seed=5).cuda()
    dets = det.process_dets(x)
    _, want = det.process(x)
    torch.cuda.synchronize()
    assert dets.shape == (2, 100, 56)
    eng = det.model._engines.get((4, 256, 256, 100, "flip_dets_only"))
    assert eng is not None and eng.flip_test and eng.dets_only and dets.data_ptr() != eng.dets.data_ptr()
    _assert_dets_close(want, dets, "process_dets")


def _img(seed, h, w):
    return (np.random.RandomState(seed).rand(h, w, 3) * 255).astype(np.uint8)


def test_run_batch_dets_only_equals_its_stages_and_the_dense_scores():
    from centerpose_amd import config, detector
    det = detector.MultiPoseDetector(config.get_cfg("res_50"))
    assert det.cfg.TEST.FLIP_TEST and not det.cfg.TEST.NMS and len(det.cfg.TEST.TEST_SCALES) == 1
    images = [_img(60, 96, 128), _img(61, 100, 130), _img(62, 96, 128)]
    assert len(det._batch_groups([im.shape[:2] for im in images])) == 1
    got = det.run_batch(images, dets_only=True)
    x, metas = det.pre_process_batch(images, 1)
    assert x.shape[0] == 6
    dets = det.process_dets(x)
    assert tuple(dets.shape) == (3, 100, 56)
    merged = det.merge_outputs_batch([det.post_process_batch(dets, metas, 1)]).cpu().numpy()
    dense = det.run_batch(images)
    for n in range(3):
        g = np.array(got[n][1], np.float32)
        assert np.array_equal(g, merged[n]), n
        assert np.array_equal(g[:, 4], np.array(dense[n][1], np.float32)[:, 4]), n
