"""GPU: the batched flip test -- cp_flip_merge_pairs_f32 against the numpy oracle and the per-pair cp_flip_merge_f32, and flip-test
plans (Engine / MultiPoseDetector.process / plan files / the C plan runtime) against the two-stage path, each pair on its own and
the CPU oracle."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import decode_np, nets_torch

pytestmark = pytest.mark.gpu

CHANNELS = (1, 2, 34, 2, 17, 2)          # hm, wh, hps, reg, hm_hp, hp_offset
MODES = (0, 0, 2, 3, 1, 3)               # cp_flip_merge_pairs_f32 mode per head


def _perm():
    from centerpose_amd import engine
    perm = list(range(17))
    for a, b in engine.FLIP_IDX:
        perm[a], perm[b] = b, a
    return torch.tensor(perm, dtype=torch.int32, device="cuda")


def _pairs(N, H, W, seed):
    """N images and their mirrored twins, interleaved: image n at 2n, twin at 2n + 1."""
    from centerpose_amd import synth
    img = synth.make_images(N, H, W, seed=seed)
    return torch.stack([img, torch.flip(img, [3])], 1).reshape(2 * N, 3, H, W)


def _oracle_pair(o, n, K=100):
    """decode_np of flip_merge of pair n of the six [2N] maps (numpy)."""
    return decode_np.multi_pose_decode(*decode_np.flip_merge(*[m[2 * n:2 * n + 2] for m in o]), K=K)


@pytest.mark.parametrize("N", [1, 3, 8])
@pytest.mark.parametrize("W", [20, 21, 128])
@pytest.mark.parametrize("groups", [((0, 4), (1, 2, 3, 5)), ((2,), (0, 1, 4), (3, 5))])
def test_flip_pairs_kernel_bit_exact(N, W, groups):
    from centerpose_amd import _lib, ops
    H = 12
    g = torch.Generator().manual_seed(N * 1000 + W)
    maps = [torch.randn(2 * N, c, H, W, generator=g).cuda() for c in CHANNELS]
    perm = _perm()
    merged = [None] * 6
    for grp in groups:
        whole = torch.full((sum(N * CHANNELS[i] * H * W for i in grp),), float("nan"), device="cuda")
        specs, off = [], 0
        for i in grp:
            n = N * CHANNELS[i] * H * W
            merged[i] = whole[off:off + n].view(N, CHANNELS[i], H, W)
            specs.append((maps[i], merged[i], MODES[i]))
            off += n
        launch = ops.flip_pairs_launch(specs, whole, perm.view(torch.float32))
        launch.run()
        assert launch.kernel == ("flip_merge_pairs_kernel<vec4>" if W % 4 == 0 else "flip_merge_pairs_kernel<scalar>")
    torch.cuda.synchronize()
    host = [m.cpu().numpy() for m in maps]
    got = [m.cpu().numpy() for m in merged]
    L = _lib.lib()
    for n in range(N):
        want = decode_np.flip_merge(*[m[2 * n:2 * n + 2] for m in host])
        for i in range(6):
            assert np.array_equal(got[i][n:n + 1], want[i]), "pair %d head %d" % (n, i)
        for i in (0, 1, 2, 4):                          # the per-pair kernel of the two-stage path
            out = torch.empty((1, CHANNELS[i], H, W), device="cuda")
            src = maps[i][2 * n:2 * n + 2].contiguous()
            _lib.check(L.cp_flip_merge_f32(_lib.ptr(src), _lib.ptr(out), CHANNELS[i], H, W, MODES[i], ctypes.c_void_p(perm.data_ptr()),
                                           _lib.stream()), "cp_flip_merge_f32")
            torch.cuda.synchronize()
            assert torch.equal(out[0].cpu(), merged[i][n].cpu()), "pair %d head %d vs cp_flip_merge_f32" % (n, i)


@pytest.mark.parametrize("arch,S", [("res_50", 128), ("dla_34", 256)])
def test_one_replay_equals_two_stage_at_b2(arch, S):
    from centerpose_amd import config, detector
    det = detector.MultiPoseDetector(config.get_cfg(arch))
    assert det.cfg.TEST.FLIP_TEST
    x = _pairs(1, S, S, seed=11).cuda()
    # the two-stage path first: its maps come from the forward-only plan
    o2, d2, t = det.process(x, return_time=True)
    o2, d2 = [t_.clone() for t_ in o2], d2.clone()
    assert (2, S, S) in det.model._engines and t > 0
    o1, d1 = det.process(x)
    o1 = [t_.clone() for t_ in o1]
    eng = det.model._engines.get((2, S, S, 100, "flip"))
    assert eng is not None and eng.flip_test and d1.data_ptr() != eng.dets.data_ptr()
    torch.cuda.synchronize()
    assert d1.shape == (1, 100, 56)
    assert all(torch.equal(a, b) for a, b in zip(o1, o2))
    assert torch.equal(d1, d2)
    # the flip plan replaced the forward-only plan of its shape; the two-stage path now replays it, with the same results
    assert (2, S, S) not in det.model._engines
    o3, d3, _ = det.process(x, return_time=True)
    torch.cuda.synchronize()
    assert (2, S, S) not in det.model._engines
    assert all(torch.equal(a, b) for a, b in zip(o3, o2)) and torch.equal(d3, d2)


@pytest.mark.parametrize("arch,H,W", [("dla_34", 256, 256), ("res_50", 192, 256)])
def test_n_pairs_each_pair_exact(arch, H, W, monkeypatch):
    from centerpose_amd import config, detector, ops
    N = 4
    x = _pairs(N, H, W, seed=12).cuda()
    det = detector.MultiPoseDetector(config.get_cfg(arch))
    outputs, dets = det.process(x)
    torch.cuda.synchronize()
    assert dets.shape == (N, 100, 56) and all(o.shape[0] == 2 * N for o in outputs)
    o = [t.cpu().numpy() for t in outputs]
    d = dets.cpu().numpy()
    for n in range(N):
        assert np.array_equal(d[n:n + 1], _oracle_pair(o, n)), "pair %d" % n
    # batch-invariant plans: every pair bit-identical to that pair alone at B = 2
    monkeypatch.setattr(ops, "BATCH_INVARIANT", True)
    inv = detector.MultiPoseDetector(config.get_cfg(arch))
    full_o, full_d = inv.process(x)
    full_o, full_d = [t.clone() for t in full_o], full_d.clone()
    for n in range(N):
        po, pd = inv.process(x[2 * n:2 * n + 2].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(pd, full_d[n:n + 1]), "pair %d dets" % n
        assert all(torch.equal(a, b[2 * n:2 * n + 2]) for a, b in zip(po, full_o)), "pair %d maps" % n


def test_shipped_dla34_512_eight_pairs_vs_cpu_oracle():
    """The shipped dla_34 preset (flip on) at 512 x 512, 8 pairs in one replay: pairs 0, 3 and 7 against the all-CPU oracle (network,
    flip_merge, decode) with test_process_end_to_end's criteria."""
    from centerpose_amd import config, detector
    det = detector.MultiPoseDetector(config.get_cfg("dla_34"))
    x = _pairs(8, 512, 512, seed=13)
    _, dets = det.process(x.cuda())
    torch.cuda.synchronize()
    assert dets.shape == (8, 100, 56)
    dets = dets.cpu().numpy()
    sd = det.model.state_dict()
    for n in (0, 3, 7):
        outs = nets_torch.forward("dla_34", sd, x[2 * n:2 * n + 2])
        outs[0], outs[4] = torch.sigmoid(outs[0]), torch.sigmoid(outs[4])
        ref = decode_np.multi_pose_decode(*decode_np.flip_merge(*[t.numpy() for t in outs]), K=100)
        got = dets[n:n + 1]
        sc = ref[..., 4].astype(np.float64)
        gap = np.minimum(np.abs(np.diff(sc, axis=1, prepend=np.inf)), np.abs(np.diff(sc, axis=1, append=-np.inf)))
        stable = gap > 2e-4
        close = np.isclose(got[..., 5:39][stable], ref[..., 5:39][stable], atol=2e-2)
        print("pair %d: stable fraction %.3f, keypoints within 2e-2 %.4f" % (n, stable.mean(), close.mean()))
        # floor: the oracle's own stable fraction on these pairs is 0.870-0.880, minus a margin (as in test_process_end_to_end)
        assert stable.mean() > 0.84
        assert np.allclose(got[..., 4][stable], ref[..., 4][stable], atol=1e-3)
        assert np.allclose(got[..., :4][stable], ref[..., :4][stable], atol=2e-2)
        assert close.mean() > 0.995


def test_flip_graph_two_batches_and_fresh_dets():
    from centerpose_amd import config, detector
    det = detector.MultiPoseDetector(config.get_cfg("dla_34"))
    xa, xb = _pairs(2, 128, 128, seed=14).cuda(), _pairs(2, 128, 128, seed=15).cuda()
    oa, da = det.process(xa)
    oa = [t.cpu().numpy() for t in oa]
    ob, db = det.process(xb)
    ob = [t.cpu().numpy() for t in ob]
    torch.cuda.synchronize()
    eng = det.model._engines.get((4, 128, 128, 100, "flip"))
    assert eng.capture_mode == "2-stream"
    assert not torch.equal(da, db)
    for o, d in ((oa, da), (ob, db)):
        for n in range(2):
            assert np.array_equal(d.cpu().numpy()[n:n + 1], _oracle_pair(o, n))


def test_flip_plan_files_and_c_abi(tmp_path):
    from centerpose_amd import _ext, _lib, cplan, engine, plan, synth
    sd = synth.make_state_dict("dla_34", seed=317)
    N, S, K = 2, 128, 100
    x, x2 = _pairs(N, S, S, seed=16).cuda(), _pairs(N, S, S, seed=17).cuda()
    eng = engine.Engine("dla_34", sd, 2 * N, S, S, decode_k=K, flip_test=True)
    want = eng.process(x)[1].clone()
    want2 = eng.process(x2)[1].clone()
    assert want.shape == (N, K, 56)
    path = str(tmp_path / "flip.cpplan")
    eng.save_plan(path, deterministic=True)
    assert plan.parse(memoryview(np.fromfile(path, dtype=np.uint8)))["meta"].get("flip_test") is True
    loaded = engine.Engine.from_plan(path)
    assert loaded.flip_test and loaded.dets.shape == (N, K, 56)
    outs, d = loaded.process(x)
    assert torch.equal(d, want) and all(o.shape[0] == 2 * N for o in outs)
    # the C handle: ctypes and the torch extension
    cp = cplan.CPlan(path)
    assert cp.flip_test and cp._L.cp_plan_flip_test(cp._h) == 1
    assert torch.equal(cp.process(x, K=K), want)
    h = _ext.plan_create(path, True)
    try:
        got = _ext.plan_process(h, x, K)
        assert got.shape == (N, K, 56) and torch.equal(got, want)
    finally:
        _ext.plan_destroy(h)
    # the rows past N of a caller's buffer stay untouched
    buf = torch.full((N + 1, K, 56), 12345.0, device="cuda")
    _lib.check(cp._L.cp_plan_process(cp._h, _lib.ptr(x), K, _lib.ptr(buf), _lib.stream()), "cp_plan_process")
    torch.cuda.synchronize()
    assert torch.equal(buf[:N], want) and bool((buf[N] == 12345.0).all())
    with pytest.raises(Exception):
        cp.process(x, K=50)                 # a decode of the un-merged maps would not be the flip test
    pipe = cplan.CPipeline(cp, depth=2)
    a, b = pipe.process([x, x2], K=K)
    assert torch.equal(a, want) and torch.equal(b, want2)
    pipe.close()
    # a normal plan says 0
    dense = engine.Engine("dla_34", sd, 2, S, S, decode_k=K, use_graph=False)
    dpath = str(tmp_path / "dense.cpplan")
    dense.save_plan(dpath)
    assert "flip_test" not in plan.parse(memoryview(np.fromfile(dpath, dtype=np.uint8)))["meta"]
    cd = cplan.CPlan(dpath)
    assert not cd.flip_test and cd._L.cp_plan_flip_test(cd._h) == 0
    cp.close()
    cd.close()
