"""GPU: detections-only inference -- cp_head_points_f32 (the wh / hps / reg / hp_offset branches evaluated at the decoded peaks) against
an fp64 CPU restatement of the dense head, and the detections-only plans (Engine / load_plan / the C plan runtime / the detector)
against the dense ones and the CPU oracle."""
import numpy as np
import pytest
import torch

from oracle import nets_torch

pytestmark = pytest.mark.gpu

SPARSE = ("wh", "hps", "reg", "hp_offset")
NOUT = {"wh": 2, "hps": 34, "reg": 2, "hp_offset": 2}


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


def _run_points(feat, wts, inds, hc, J, K):
    from centerpose_amd import ops
    B, H, W, C = feat.shape
    dev = feat.device
    w1 = torch.cat([ops.pack_head_points_weight(wts[n][0]) for n in SPARSE]).to(dev)
    b1 = torch.cat([wts[n][1] for n in SPARSE]).to(dev)
    w2 = torch.cat([wts[n][2].reshape(-1, hc) for n in SPARSE]).contiguous().to(dev)
    b2 = torch.cat([wts[n][3] for n in SPARSE]).to(dev)
    out = torch.full((B * H * W * (6 + 2 * J),), float("nan"), device=dev)
    ws = inds.to(torch.int32).contiguous().view(torch.float32).to(dev)
    ops.head_points_launch(feat, ws, w1, b1, w2, b2, out, hc=hc, J=J, K=K).run()
    torch.cuda.synchronize()
    maps, off = {}, 0
    for name in SPARSE:
        n = NOUT[name]
        maps[name] = out[off:off + B * n * H * W].view(B, n, H, W).cpu()
        off += B * n * H * W
    return maps


def _point_list(B, H, W, J, K, seed):
    """[B, 1+J, K] flat indices: every border and corner, duplicates, a joint index equal to a centre index, one centre index in
    the class plane above the first (taken % (H*W), as pose_assign_kernel does)."""
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


@pytest.mark.parametrize("C,hc", [(64, 256), (256, 64), (32, 64), (32, 256), (256, 256), (64, 64)])
def test_head_points_kernel_vs_fp64(C, hc):
    B, H, W, J, K = 3, 20, 24, 17, 16
    HW = H * W
    torch.manual_seed(C + hc)
    feat_cpu = torch.randn(B, H, W, C)
    feat = feat_cpu.cuda()
    wts = _branch_weights(C, hc, seed=C * 7 + hc)
    inds = _point_list(B, H, W, J, K, seed=C + hc)
    got = _run_points(feat, wts, inds, hc, J, K)
    ref = _dense_fp64(feat_cpu, wts)
    centre = [set((inds[b, 0] % HW).tolist()) for b in range(B)]
    joint = [set(inds[b, 1:].reshape(-1).tolist()) for b in range(B)]
    for name in SPARSE:
        where = joint if name == "hp_offset" else centre
        mask = torch.zeros(B, 1, H, W, dtype=torch.bool)
        for b in range(B):
            mask.view(B, HW)[b, list(where[b])] = True
        mask = mask.expand(-1, NOUT[name], -1, -1)
        g, r = got[name], ref[name]
        # only the addressed pixels are written, every one of them with a finite value
        assert torch.isnan(g[~mask]).all(), name
        assert torch.isfinite(g[mask]).all(), name
        err = (g[mask].double() - r[mask]).abs().max().item()
        assert err <= 1e-4 * r.abs().max().item(), "%s: %.3e" % (name, err)

    # the same pixels from a shuffled point list padded with duplicates: bit-identical values
    g = torch.Generator().manual_seed(11)
    K2 = K + 9
    inds2 = torch.empty(B, 1 + J, K2, dtype=torch.int32)
    for b in range(B):
        for row in range(1 + J):
            perm = torch.randperm(K, generator=g)
            extra = torch.randint(0, K, (K2 - K,), generator=g)
            inds2[b, row] = torch.cat([inds[b, row][perm], inds[b, row][extra]])
    got2 = _run_points(feat, wts, inds2, hc, J, K2)
    for name in SPARSE:
        fin = torch.isfinite(got[name])
        assert torch.equal(fin, torch.isfinite(got2[name])), name
        assert torch.equal(got[name][fin], got2[name][fin]), name


def _topk_ws(eng):
    topk = [l for _, _, _, l in eng.launches if l.fn == "cp_decode_topk_f32"][0]
    return topk.tensors[2], topk.tensors[3].view(torch.int32)


@pytest.mark.parametrize("arch,B,S", [("dla_34", 2, 512), ("res_50", 2, 256), ("hrnet", 2, 256), ("mobilenetv3", 2, 128),
                                      ("shufflenetV2", 2, 128), ("resdcn_18", 2, 128)])
def test_dets_only_engine_vs_dense(arch, B, S):
    from centerpose_amd import engine, synth
    sd = synth.make_state_dict(arch, seed=317)
    x = synth.make_images(B, S, S, seed=21).cuda()
    dense = engine.Engine(arch, sd, B, S, S, decode_k=100)
    sparse = engine.Engine(arch, sd, B, S, S, decode_k=100, dets_only=True)
    outs_d, dets_d = dense.process(x)
    outs_s, dets_s = sparse.process(x)
    torch.cuda.synchronize()
    assert [o is None for o in outs_s] == [False, True, True, True, False, True]
    assert torch.equal(outs_d[0], outs_s[0]) and torch.equal(outs_d[4], outs_s[4])
    sc_d, in_d = _topk_ws(dense)
    sc_s, in_s = _topk_ws(sparse)
    assert torch.equal(in_d, in_s) and torch.equal(sc_d, sc_s)
    dd, ds = dets_d.cpu(), dets_s.cpu()
    J = outs_d[4].shape[1]
    assert torch.equal(dd[..., 4], ds[..., 4]) and torch.equal(dd[..., 5 + 2 * J:], ds[..., 5 + 2 * J:])
    assert (dd[..., :4] - ds[..., :4]).abs().max().item() <= 1e-3
    kp_close = ((dd[..., 5:5 + 2 * J] - ds[..., 5:5 + 2 * J]).abs() <= 1e-3).float().mean().item()
    assert kp_close >= 0.995, kp_close
    # the dense maps at the decoded peaks vs the points kernel's values there
    H, W = outs_d[0].shape[2:]
    ind = in_d.cpu().long()
    centre, joints = ind[:, 0] % (H * W), ind[:, 1:].reshape(B, -1)
    for i, name in ((1, "wh"), (2, "hps"), (3, "reg"), (5, "hp_offset")):
        d = outs_d[i].cpu().reshape(B, outs_d[i].shape[1], -1)
        s = sparse.head_maps[i].cpu().reshape(B, outs_d[i].shape[1], -1)
        at = joints if name == "hp_offset" else centre
        idx = at[:, None, :].expand(-1, d.shape[1], -1)
        dv, sv = d.gather(2, idx), s.gather(2, idx)
        assert torch.isfinite(sv).all(), name
        err = (dv - sv).abs().max().item()
        assert err <= 1e-4 * max(d.abs().max().item(), 1.0), "%s %s: %.3e" % (arch, name, err)


def test_dets_only_poisoned_maps():
    """NaN in every element of the sparse-map storage before a replay: the detections do not change (every pixel the decode reads
    is written in the same step), and further replays are bit-stable."""
    from centerpose_amd import engine, synth
    sd = synth.make_state_dict("dla_34", seed=317)
    x = synth.make_images(2, 256, 256, seed=4).cuda()
    eng = engine.Engine("dla_34", sd, 2, 256, 256, decode_k=100, dets_only=True)
    want = eng.process(x)[1].clone()
    pts = [l for _, _, _, l in eng.launches if l.fn == "cp_head_points_f32"]
    assert len(pts) == 1
    pts[0].out.fill_(float("nan"))
    got = [eng.process(x)[1].clone() for _ in range(3)]
    torch.cuda.synchronize()
    assert torch.isfinite(want).all()
    for g in got:
        assert torch.equal(g, want)


def _oracle_check(arch, sd, dets, x, floor):
    _, ref = nets_torch.process(arch, sd, x, K=100)
    sc = ref[..., 4].astype(np.float64)
    gap = np.minimum(np.abs(np.diff(sc, axis=1, prepend=np.inf)), np.abs(np.diff(sc, axis=1, append=-np.inf)))
    stable = gap > 2e-4
    close = np.isclose(dets[..., 5:39][stable], ref[..., 5:39][stable], atol=2e-2)
    print("%s dets_only: stable fraction %.3f, keypoints within 2e-2 %.4f" % (arch, stable.mean(), close.mean()))
    assert stable.mean() > floor
    assert np.allclose(dets[..., 4][stable], ref[..., 4][stable], atol=1e-3)
    assert np.allclose(dets[..., :4][stable], ref[..., :4][stable], atol=2e-2)
    assert close.mean() > 0.995


@pytest.mark.parametrize("arch", ["dla_34", "res_50"])
def test_dets_only_detector_vs_oracle(arch):
    """test_process_end_to_end's criteria, through MultiPoseDetector.process(x, dets_only=True)."""
    from centerpose_amd import config, detector, synth
    det = detector.MultiPoseDetector(config.get_cfg(arch, TEST__FLIP_TEST=False))
    x = synth.make_images(2, 256, 256, seed=5)
    outputs, dets = det.process(x.cuda(), dets_only=True)
    torch.cuda.synchronize()
    assert [o is None for o in outputs] == [False, True, True, True, False, True]
    assert dets.shape == (2, 100, 56)
    _oracle_check(arch, det.model.state_dict(), dets.cpu().numpy(), x, {"dla_34": 0.93, "res_50": 0.83}[arch])


def test_dets_only_detector_b16_512():
    """dla_34 at the benchmark shape (B = 16, 512 x 512): images 0, 7 and 15 against the CPU oracle."""
    from centerpose_amd import config, detector, synth
    det = detector.MultiPoseDetector(config.get_cfg("dla_34", TEST__FLIP_TEST=False))
    x = synth.make_images(16, 512, 512, seed=6)
    outputs, dets = det.process(x.cuda(), dets_only=True)
    torch.cuda.synchronize()
    assert [o is None for o in outputs] == [False, True, True, True, False, True]
    pick = [0, 7, 15]
    # floor: the oracle's own stable fraction on these three images is 0.897, minus a margin (as in test_process_end_to_end)
    _oracle_check("dla_34", det.model.state_dict(), dets.cpu().numpy()[pick], x[pick], 0.85)


def test_dets_only_stream_matches_process():
    from centerpose_amd import config, detector, synth
    det = detector.MultiPoseDetector(config.get_cfg("dla_34", TEST__FLIP_TEST=False))
    batches = [synth.make_images(2, 256, 256, seed=30 + i).cuda() for i in range(5)]
    want = [det.process(b, dets_only=True)[1].clone() for b in batches]
    got = list(det.process_stream(batches, depth=2, dets_only=True))
    torch.cuda.synchronize()
    assert len(got) == 5
    for (outs, d), w in zip(got, want):
        assert [o is None for o in outs] == [False, True, True, True, False, True]
        assert torch.equal(d, w)


def test_dets_only_plan_round_trip(tmp_path):
    from centerpose_amd import cplan, engine, plan, synth
    sd = synth.make_state_dict("dla_34", seed=317)
    x = synth.make_images(2, 256, 256, seed=9).cuda()
    x2 = synth.make_images(2, 256, 256, seed=10).cuda()
    eng = engine.Engine("dla_34", sd, 2, 256, 256, decode_k=100, dets_only=True)
    want = eng.process(x)[1].clone()
    want2 = eng.process(x2)[1].clone()
    path = str(tmp_path / "dets_only.cpplan")
    eng.save_plan(path)
    meta = plan.parse(memoryview(np.fromfile(path, dtype=np.uint8)))["meta"]
    assert meta.get("dets_only") is True
    loaded = plan.load_plan(path)
    outs, d = loaded.process(x)
    assert loaded.dets_only and [o is None for o in outs] == [False, True, True, True, False, True]
    assert torch.equal(d, want)
    cp = cplan.CPlan(path)
    assert cp.dets_only and cp.n_outputs == 6
    assert cp._L.cp_plan_dets_only(cp._h) == 1
    assert torch.equal(cp.process(x, K=100), want)
    with pytest.raises(Exception):
        cp.process(x, K=50)                 # a decode with another K would read pixels nobody wrote
    pipe = cplan.CPipeline(cp, depth=2)
    a, b = pipe.process([x, x2], K=100)
    assert torch.equal(a, want) and torch.equal(b, want2)
    pipe.close()
    # a dense plan says 0
    dense = engine.Engine("dla_34", sd, 2, 256, 256, decode_k=100, use_graph=False)
    dpath = str(tmp_path / "dense.cpplan")
    dense.save_plan(dpath)
    assert "dets_only" not in plan.parse(memoryview(np.fromfile(dpath, dtype=np.uint8)))["meta"]
    cd = cplan.CPlan(dpath)
    assert not cd.dets_only and cd._L.cp_plan_dets_only(cd._h) == 0
    cp.close()
    cd.close()


def test_dets_only_pipeline_engine():
    """EnginePipeline over detections-only engines: per instance bit-identical to Engine.process."""
    from centerpose_amd import engine, synth
    sd = synth.make_state_dict("res_50", seed=317)
    xs = [synth.make_images(2, 256, 256, seed=40 + i).cuda() for i in range(2)]
    cc = {}
    engs = [engine.Engine("res_50", sd, 2, 256, 256, decode_k=100, dets_only=True, const_cache=cc) for _ in range(2)]
    want = [engs[0].process(x)[1].clone() for x in xs]
    pipe = engine.EnginePipeline.from_engines(engs)
    got = [d.clone() for _, d in pipe.process_all(xs)]
    torch.cuda.synchronize()
    assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_dets_only_refusals():
    from centerpose_amd import config, detector, engine, synth
    x = synth.make_images(2, 128, 128, seed=1).cuda()
    det = detector.MultiPoseDetector(config.get_cfg("dla_34", TEST__FLIP_TEST=False))
    with pytest.raises(ValueError, match="return_time"):
        det.process(x, return_time=True, dets_only=True)
    flip = detector.MultiPoseDetector(config.get_cfg("dla_34", TEST__FLIP_TEST=True))
    with pytest.raises(ValueError, match="FLIP_TEST"):
        flip.process(x, dets_only=True)
    with pytest.raises(ValueError, match="FLIP_TEST"):
        flip.process_stream([x, x], depth=2, dets_only=True)
    gated = detector.MultiPoseDetector(config.get_cfg("dla_34", TEST__FLIP_TEST=False, LOSS__REG_OFFSET=False))
    with pytest.raises(ValueError, match="LOSS"):
        gated.process(x, dets_only=True)
    with pytest.raises(ValueError, match="decode_k"):
        engine.Engine("dla_34", synth.make_state_dict("dla_34", seed=317), 2, 128, 128, dets_only=True)
    # the defaults are untouched: the dense path still hands out all six maps
    outs, _ = det.process(x)
    assert all(o is not None for o in outs)
