"""GPU: the two-stream schedules of the product, audited for data races by byte range (tests/schedule_audit.py).

Per row (B = 2, 128 x 128, synthetic weights, use_graph=True, two capture streams, after capture):
  static   `audit` of what the capture issued (`stream_of_launch`, `event_waits`) == [], and of what the C runtime derives for the same
           plan (`save_plan` -> `plan.parse` -> `cp_schedule_waits`), by the file's refs and by the engine's tensors;
  liveness both streams used, >= 1 cross-stream wait, >= 1 cross-stream conflict pair -- a pass is not vacuous;
  dynamic  the captured order run eagerly on ONE stream after `poison("A")` is the reference; the same order after `poison("B")` gives
           the same bits (no launch reads memory it did not get from a predecessor); then `asap(j)` for EVERY launch j, the two
           poisons alternating: every pair of launches the capture leaves concurrent runs in both orders, and every pass reproduces
           the reference bit for bit.
All comparisons are bit-equality.  Each row prints its figures (DESIGN.md has the table measured on an MI355X).
"""
import time

import numpy as np
import pytest
import torch

import schedule_audit as sa

pytestmark = pytest.mark.gpu

B, H, W, K = 2, 128, 128, 100
ARCHS = ["dla_34", "res_50", "hrnet", "mobilenetv3", "shufflenetV2", "resdcn_18"]
ROWS = [(a, {}) for a in ARCHS] + [
    ("dla_34", dict(decode_k=K)), ("dla_34", dict(decode_k=K, flip_test=True)), ("dla_34", dict(decode_k=K, dets_only=True)),
    ("dla_34", dict(decode_k=K, flip_dets_only=True)), ("res_50", dict(decode_k=K)), ("hrnet", dict(decode_k=K)),
    ("dla_34", dict(min_age=0))]                 # BufferPool hands a slot out again at once: the densest WAR edges
ROW_ID = lambda row: row[0] + "".join("-%s" % k for k in row[1]) if row[1] else row[0] + "-plain"
# launches that are neither DCN, decode, points nor flip: the only ones the device teeth run out of order
PLAIN_FNS = ("cp_conv2d_f32", "cp_conv3x3_winograd_f32", "cp_maxpool2d_nhwc_f32", "cp_dw_deconv_add_nhwc_f32", "cp_sum_up_nhwc_f32",
             "cp_splitk_reduce_f32")
STATS = {}


def build(row, monkeypatch, seed=5):
    """(engine after capture, storages the BufferPool handed out a second time)"""
    from centerpose_amd import engine, synth
    arch, kw = row[0], dict(row[1])
    if "min_age" in kw:
        monkeypatch.setenv("CP_BUFFER_MIN_AGE", str(kw.pop("min_age")))
    reused, take = set(), engine.BufferPool.take

    def spy(self, numel):
        before = self.bytes
        slot = take(self, numel)
        if self.bytes == before:
            reused.add(slot.untyped_storage().data_ptr())
        return slot
    monkeypatch.setattr(engine.BufferPool, "take", spy)
    e = engine.Engine(arch, synth.make_state_dict(arch), B, H, W, use_graph=True, **kw)
    x = synth.make_images(B, H, W, seed=seed).cuda()
    for _ in range(2):
        e.forward(x)
    torch.cuda.synchronize()
    assert e.capture_mode == "2-stream", e.capture_mode
    return e, reused


def static_audit(e, reused, tmp_path, label):
    """the static side of a row -> figures; asserts zero unordered conflicts in the capture's and in the C runtime's view"""
    from centerpose_amd import plan
    where, waits = e.stream_of_launch, e.event_waits
    found = sa.conflicts(e.launches)
    assert sa.audit(e.launches, where, waits, found) == []
    cross = [c for c in found if where[c.j] != where[c.i]]
    assert set(where) == {0, 1} and any(waits) and cross, "vacuous: streams %s, %d waits, %d cross-stream conflicts" % (
        set(where), sum(map(len, waits)), len(cross))
    assert all(where[j] != where[i] for i, w in enumerate(waits) for j in w)
    war = [c for c in cross if "WAR" in c.kinds and e.launches[c.i][3].tensors[c.slot_i].untyped_storage().data_ptr() in reused]
    # the C runtime's view of the same plan: the file's streams / out_index / refs through cp_schedule_waits
    path = str(tmp_path / "audit.cpplan")
    e.save_plan(path)
    p = plan.parse(memoryview(np.fromfile(path, dtype=np.uint8)))
    streams, cw = sa.plan_waits(p["ops"], len(p["buffers"]))
    assert streams == list(e.stream_plan) == where and [o[0] for o in p["ops"]] == [l.fn for _, _, _, l in e.launches]
    assert sa.audit(p["ops"], streams, cw) == []                        # conflicts by the file's (buffer id, offset, numel)
    assert sa.audit(e.launches, streams, cw, found) == []               # ... and by the byte hulls of the tensors behind them
    hb = sa.happens_before(where, waits)
    return dict(row=label, launches=len(where), waits=sum(map(len, waits)), c_waits=sum(map(len, cw)), conflicts=len(found),
                cross_conflicts=len(cross), cross_war_reused=len(war), concurrent_pairs=sa.concurrent_pairs(hb),
                concurrent_launches=len(sa.concurrent(hb))), hb


def snapshot(e):
    """what a run is judged by: the six heads, `dets` where the plan decodes; a detections-only plan: hm, hm_hp, dets, the peak
    indices and the four sparse maps AT the decoded peaks (elsewhere they are unspecified by contract)"""
    out = [t.clone() for t in e.outputs if t is not None]
    if e.dets is not None:
        out.append(e.dets.clone())
    if e.dets_only:
        topk = [l for _, _, _, l in e.launches if l.fn == "cp_decode_topk_f32"][0]
        inds = topk.tensors[3].view(torch.int32).clone()                                  # [N, 1 + J, K]
        out.append(inds)
        wh, hps, reg, hpo = (e.head_maps[i] for i in (1, 2, 3, 5))
        hw = wh.shape[2] * wh.shape[3]
        assert int(inds.min()) >= 0
        centre = (inds[:, 0, :] % hw).long()
        joints = (inds[:, 1:, :].reshape(inds.shape[0], -1) % hw).long()
        for m, at in ((wh, centre), (hps, centre), (reg, centre), (hpo, joints)):
            out.append(m.flatten(2).gather(2, at[:, None, :].expand(-1, m.shape[1], -1)))
    return out


def same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


def eager(e, order, pattern):
    sa.poison(e, pattern)
    sa.run_order(e, order)
    torch.cuda.synchronize()
    return snapshot(e)


@pytest.mark.parametrize("row", ROWS, ids=ROW_ID)
def test_schedule_is_race_free(row, monkeypatch, tmp_path):
    t0 = time.time()
    e, reused = build(row, monkeypatch)
    t_build = time.time() - t0
    replay = snapshot(e)
    t0 = time.time()
    stats, hb = static_audit(e, reused, tmp_path, ROW_ID(row))
    t_static = time.time() - t0
    t0 = time.time()
    n = len(e.launches)
    ref = eager(e, range(n), "A")
    assert same(ref, replay), "the captured order, eagerly, differs from the graph replay"
    assert same(eager(e, range(n), "B"), ref), "a launch reads memory no predecessor wrote: the outputs follow the poison"
    for j in range(n):
        got = eager(e, sa.asap(j, hb), "AB"[j % 2])
        assert same(got, ref), "launch %d (%s) as early as the capture allows changes the outputs" % (j, e.launches[j][1])
    sa.poison(e, "A")
    e.graph.replay()                                                    # the graph itself, on poisoned buffers
    torch.cuda.synchronize()
    assert same(snapshot(e), ref)
    stats.update(eager_passes=n + 2, seconds_build=round(t_build, 2), seconds_static=round(t_static, 2), seconds_dynamic=round(time.time() - t0, 2))
    STATS[ROW_ID(row)] = stats
    print("\nschedule audit:", stats)


@pytest.mark.parametrize("arch,depth", [("dla_34", 2), ("hrnet", 3)])
def test_pipeline_schedules_are_race_free(arch, depth, tmp_path):
    """Steps in flight (static only): the joint schedule of `EnginePipeline(depth)` as captured, and the C runtime's interleave of
    `depth` instances of the plan file (op by op, odd instances with the streams swapped)."""
    from centerpose_amd import engine, plan, synth
    t0 = time.time()
    pipe = engine.EnginePipeline(arch, synth.make_state_dict(arch), B, H, W, depth=depth, use_graph=True, decode_k=K)
    pipe.process_all([synth.make_images(B, H, W, seed=30 + i).cuda() for i in range(depth)])
    torch.cuda.synchronize()
    assert pipe.capture_mode == "2-stream"
    j = pipe.joint
    t1 = time.time()
    found = sa.conflicts(j.launches)
    assert sa.audit(j.launches, j.stream_of_launch, j.event_waits, found) == []
    owner = {id(l): k for k, e in enumerate(pipe.engines) for _, _, _, l in e.launches}
    assert all(owner[id(j.launches[c.j][3])] == owner[id(j.launches[c.i][3])] for c in found)       # instances share no written byte
    cross = [c for c in found if j.stream_of_launch[c.j] != j.stream_of_launch[c.i]]
    assert set(j.stream_of_launch) == {0, 1} and any(j.event_waits) and cross
    hb = sa.happens_before(j.stream_of_launch, j.event_waits)
    path = str(tmp_path / "pipe.cpplan")
    pipe.engines[0].save_plan(path)
    p = plan.parse(memoryview(np.fromfile(path, dtype=np.uint8)))
    ops_c = sa.pipeline_interleave(p["ops"], depth, len(p["buffers"]))
    streams, cw = sa.plan_waits(ops_c, depth * len(p["buffers"]))
    found_c = sa.conflicts(ops_c)
    assert sa.audit(ops_c, streams, cw, found_c) == []
    assert set(streams) == {0, 1} and any(cw) and any(streams[c.j] != streams[c.i] for c in found_c)
    print("\nschedule audit:", dict(row="%s-pipeline-depth%d" % (arch, depth), launches=len(j.launches), waits=sum(map(len, j.event_waits)),
                                   c_waits=sum(map(len, cw)), conflicts=len(found), cross_conflicts=len(cross), concurrent_pairs=sa.concurrent_pairs(hb),
                                   c_conflicts=len(found_c), seconds_build=round(t1 - t0, 2), seconds_static=round(time.time() - t1, 2)))


def test_table_has_a_cross_stream_war_on_a_reused_pool_slot(monkeypatch, tmp_path):
    """BufferPool reuse is what makes WAR edges depend on buffer sizes: somewhere in the table a launch on one stream overwrites a
    recycled slot that a launch on the OTHER stream still reads -- and the capture orders them (every row's audit is empty)."""
    rows = dict(STATS)
    last = ROWS[-1]
    if ROW_ID(last) not in rows:                                        # run on its own: the row built for this
        e, reused = build(last, monkeypatch)
        rows[ROW_ID(last)] = static_audit(e, reused, tmp_path, ROW_ID(last))[0]
    print("\ncross-stream WAR pairs on a reused pool slot:", {k: v["cross_war_reused"] for k, v in rows.items()})
    assert any(v["cross_war_reused"] for v in rows.values())


def test_teeth_one_dropped_wait_changes_the_outputs_on_the_device(monkeypatch):
    """dla_34 plain, ONE wait dropped whose producer and consumer are both convolution / elementwise launches: `audit` reports the
    pair, and the serial order the weakened relation newly allows -- the consumer as early as possible, before its producer -- gives
    other outputs than the reference.  Valid kernels on valid memory in an order the product never uses."""
    e, _ = build(ROWS[0], monkeypatch)
    where, waits = e.stream_of_launch, e.event_waits
    found = sa.conflicts(e.launches)
    hb = sa.happens_before(where, waits)
    n = len(e.launches)
    ref = eager(e, range(n), "A")
    pick = None
    for i, ws in enumerate(waits):
        for j in ws:
            raw = [c for c in found if (c.j, c.i) == (j, i) and "RAW" in c.kinds]
            if raw and e.launches[i][3].fn in PLAIN_FNS and e.launches[j][3].fn in PLAIN_FNS and pick is None:
                weak = sa.without_wait(waits, i, j)
                if any((c.j, c.i) == (j, i) for c in sa.unordered(e.launches, where, weak, found)):
                    pick = (i, j, weak)
    assert pick is not None, "no droppable wait between two plain launches"
    i, j, weak = pick
    hb2 = sa.happens_before(where, weak)
    order = sa.asap(i, hb2)
    assert sa.is_linear_extension(order, hb2) and not sa.is_linear_extension(order, hb) and order.index(i) < order.index(j)
    print("\ndropped the wait of launch %d (%s) for launch %d (%s)" % (i, e.launches[i][1], j, e.launches[j][1]))
    got = eager(e, order, "B")
    assert not same(got, ref), "the consumer ran before its producer and nothing changed"
    assert same(eager(e, range(n), "B"), ref)                           # the legal order again: the reference again


def test_c_pipeline_depth_one_on_a_single_stream_plan(tmp_path):
    """cp_pipeline_create(depth = 1) on a plan whose ops all carry stream 0: the side stream is never forked, so the capture ends
    joined; `CPipeline.process` equals `CPlan.process` bit for bit, on the capturing call and on replays."""
    from centerpose_amd import _lib, cplan, engine, plan, synth
    eng = engine.Engine("dla_34", synth.make_state_dict("dla_34"), B, H, W, use_graph=False, decode_k=K)
    blob = plan.serialize(eng.launches, {"arch": eng.arch, "flops_per_image": int(eng.flops_per_image)}, eng.input, eng.head_maps,
                          int(_lib.lib().cp_abi_version()), streams=None)
    assert not any(o[5] for o in plan.parse(memoryview(blob))["ops"])
    xs = [synth.make_images(B, H, W, seed=40 + i).cuda() for i in range(2)]
    want = [eng.process(x)[1].clone() for x in xs]
    cp = cplan.CPlan(blob)
    single = [cp.process(x, K).clone() for x in xs]
    pipe = cplan.CPipeline(cp, depth=1)
    got = [pipe.process([x], K)[0].clone() for x in (xs[0], xs[1], xs[0], xs[1])]       # warm-up + capture, then three replays
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(single, want))
    assert all(torch.equal(g, want[k % 2]) for k, g in enumerate(got))
    pipe.close()
    cp.close()
