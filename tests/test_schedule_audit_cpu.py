"""The schedule audit (tests/schedule_audit.py) and the two pure wait functions it judges -- `engine.capture_waits` and the library's
`cp_schedule_waits` -- without a GPU.

* WRITES against the header: per scheduled entry point, the pointer parameters include/centerpose_hip.h does not declare `const` are
  exactly the slots the table marks.
* Synthetic launch lists built by the real `ops.*_launch` constructors on CPU tensors (a group launch with its `whole`, the in-place
  IDAUp add, the decode pair sharing its workspace, a split-K workspace with its reduce, a recycled pool slot): the transitive closure
  of `Engine.dependencies` contains every byte-range conflict.
* 320 seeded random DAGs (n <= 60; 2 and 3 streams; greedy and explicit placement): the closure of `capture_waits` contains the DAG.
  Random op lists over buffer ids, also interleaved as `cp_pipeline_process` interleaves 2 and 3 plan instances with swapped streams:
  the closure of `cp_schedule_waits` contains every conflict, and orders the same pairs as `capture_waits` on the same input.
* Teeth: every wait that the rest does not imply is needed (its removal makes `audit` report a pair); a slot deleted from WRITES
  fails the header check; a group member moved to its own storage fails `audit` while `Engine.dependencies` sees nothing.
"""
import ctypes
import os
import random
import re
import types

import pytest
import torch

import schedule_audit as sa
from centerpose_amd import engine, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- header against table ----------------------------------------------------------------------------------------------------------------
# what a prototype cannot say: pointer parameters that are HOST integer arrays (not slots of the launch record), how many slots a
# pointer-to-pointer parameter covers, and which functions' records end with the storage all their outputs live in
HOST_ARRAYS = {("cp_sum_up_nhwc_f32", "ld"), ("cp_sum_up_nhwc_f32", "shift"), ("cp_sum_up_group_nhwc_f32", "meta"),
               ("cp_flip_merge_pairs_f32", "meta")}
ARRAY_WIDTH = {"cp_conv2d_f32": {"src": 4}, "cp_sum_up_nhwc_f32": {"src": 4}, "cp_sum_up_group_nhwc_f32": {"src": 16, "out": 4},
               "cp_flip_merge_pairs_f32": {"in": 4, "out": 4},
               "cp_conv3x3_winograd24_group_f32": dict.fromkeys(("src", "u", "scale", "shift", "res", "out"), 4),
               "cp_conv2d_group_f32": dict.fromkeys(("src", "w", "scale", "shift", "res", "out"), 8)}
HAS_WHOLE = ("cp_conv3x3_winograd24_group_f32", "cp_conv2d_group_f32", "cp_sum_up_group_nhwc_f32", "cp_flip_merge_pairs_f32")


def header_slots(fn):
    """[(parameter name, declared const, slots)] of the tensor parameters of `fn`, from its prototype in the header"""
    src = open(os.path.join(ROOT, "include", "centerpose_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % re.escape(fn), src)
    assert m, "no prototype of %s in the header" % fn
    out, slot = [], 0
    for prm in (p.strip() for p in m.group(1).split(",")):
        if "*" not in prm:
            continue
        name = re.search(r"(\w+)\s*$", prm).group(1)
        if name == "stream" or re.match(r"const\s+cp_\w+_desc\s*\*", prm) or (fn, name) in HOST_ARRAYS:
            continue
        assert re.match(r"(const\s+)?(float|int)\s*\*\s*(const\s*\*\s*)?\w+$", prm), prm
        width = ARRAY_WIDTH[fn][name] if prm.count("*") == 2 else 1
        out.append([name, prm.startswith("const"), list(range(slot, slot + width))])
        slot += width
    if fn in HAS_WHOLE:                                     # float* const* out: its member slots and the storage they live in
        assert out[[o[0] for o in out].index("out")][1] is False
        out[[o[0] for o in out].index("out")][2].append(slot)
    return out


def check_header_against(writes):
    assert set(writes) == set(ops.FN_IDS) and len(writes) == 21
    for fn in ops.FN_IDS:
        params = header_slots(fn)
        written = sorted(k for _, const, slots in params for k in slots if not const)
        assert written == sorted(writes[fn]), "%s: the header leaves %s non-const (slots %s), WRITES says %s" % (
            fn, [n for n, c, _ in params if not c], written, sorted(writes[fn]))


def test_writes_table_is_the_headers_non_const_pointers():
    check_header_against(sa.WRITES)
    # ... and the index slots are const int* parameters
    for fn, slots in sa.INDEX_READS.items():
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "centerpose_hip.h")).read(), flags=re.S)
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % fn, src).group(1)
        names = [n for n, _, s in header_slots(fn) if set(s) & set(slots)]
        assert names == ["ws_inds"] and re.search(r"const\s+int\s*\*\s*ws_inds", proto)


def test_teeth_a_slot_deleted_from_writes_fails_the_header_check():
    for fn, gone in (("cp_conv2d_group_f32", 48), ("cp_conv2d_group_f32", 41), ("cp_sum_up_group_nhwc_f32", 17), ("cp_decode_topk_f32", 3)):
        w = dict(sa.WRITES)
        w[fn] = tuple(k for k in w[fn] if k != gone)
        with pytest.raises(AssertionError, match=fn):
            check_header_against(w)


# ---- synthetic launch lists --------------------------------------------------------------------------------------------------------------
def _standin(launches):
    return types.SimpleNamespace(launches=[("k", "L%d" % i, 0, l) for i, l in enumerate(launches)])


def _deps_closure(deps):
    hb = []
    for i, d in enumerate(deps):
        m = 0
        for j in d:
            m |= hb[j] | (1 << j)
        hb.append(m)
    return hb


def synthetic_launches(split_member=False):
    """A small schedule with every bookkeeping convention in it, on CPU tensors.  split_member: member 1 of the group launch writes
    a storage of its own instead of a view of `whole` (what the constructors' assertion forbids; the record is built directly)."""
    z = lambda *s: torch.zeros(*s)
    B, H, W = 1, 8, 8
    x = z(B, H, W, 16)
    a = z(B, H, W, 64)
    w64, one64, zero64 = z(64, 64), z(64), z(64)
    conv = lambda src, out, **kw: ops.conv2d_launch([src], w64[:, :src.shape[3]].contiguous(), one64, zero64, out, kh=1, kw=1, cout=out.shape[-1],
                                                    split_bf16=False, **kw)
    L = [conv(x, a)]                                                                       # 0: x -> a
    whole = z(2 * B * H * W * 64)
    o1, o2 = (v.view(B, H, W, 64) for v in whole.split(B * H * W * 64))
    members = [dict(x=a, wp=w64, scale=one64, shift=zero64, out=o, cout=64, k=1, stride=1, pad=0, act=0) for o in (o1, o2)]
    if split_member:
        group = ops.conv2d_group_launch(members, whole)
        t = list(group.tensors)
        o2 = z(B, H, W, 64)
        t[41] = o2
        L.append(ops.Launch("cp_conv2d_group_f32", group.desc, t, group.ints))
    else:
        L.append(ops.conv2d_group_launch(members, whole))                                  # 1: a -> (o1, o2) in `whole`
    b, c = z(B, H // 2, W // 2, 64), z(B, H, W, 64)
    L.append(ops.maxpool2d_launch(o1, b, 2, 2, 0))                                         # 2: o1 -> b
    L.append(conv(o2, c))                                                                  # 3: o2 -> c
    L.append(ops.dw_deconv_add_launch(b, z(16, 64), c, c, 2))                              # 4: c += up(b), in place (add is out)
    L.append(conv(c, a))                                                                   # 5: c -> a again: a recycled slot (WAR with 1)
    ws = z(2, B * H * W, 64)
    L.append(ops.conv2d_launch([a], w64, one64, zero64, ws, kh=1, kw=1, cout=64, ksplit=2, split_bf16=False))    # 6: split-K partial sums
    d = z(B, H, W, 64)
    L.append(ops.splitk_reduce_launch(ws, one64, zero64, d, cout=64))                      # 7: ... and their reduction
    J, K = 17, 4
    heads = [z(B, n, H, W) for n in (1, 2, 2 * J, 2, J, 2)]
    nchw = lambda src, out: ops.conv2d_launch([src], w64, one64, zero64, out, kh=1, kw=1, cout=out.shape[1], out_nchw=True, split_bf16=False)
    L += [nchw(d, h) for h in heads]                                                       # 8..13: hm, wh, hps, reg, hm_hp, hp_offset
    wsd, dets = z(2, B, 1 + J, K), z(B, K, 5 + 3 * J)
    topk, assign = ops.decode_launches(heads[0], heads[1], heads[2], heads[3], heads[4], heads[5], K, wsd, dets)
    L.insert(8 + 5, topk)                                                                  # 13: right after hm, hm_hp (beside hp_offset)
    L.append(assign)                                                                       # 15
    return L


def test_dependencies_cover_every_byte_range_conflict_of_the_synthetic_schedule():
    L = synthetic_launches()
    found = sa.conflicts(L)
    pairs = {(c.j, c.i): c.kinds for c in found}
    # the conventions are all there: group + whole, in place, recycled slot, split-K, the decode pair through its workspace
    assert pairs[(1, 2)] == {"RAW"} and pairs[(1, 3)] == {"RAW"}                           # members of the group launch
    assert {"RAW", "WAW"} <= pairs[(3, 4)] and pairs[(1, 5)] == {"WAR"} and pairs[(6, 7)] == {"RAW"}
    assert pairs[(13, 15)] == {"RAW"} and (0, 5) in pairs and "WAW" in pairs[(0, 5)]
    assert sa.extent(L[1].tensors[48]) == (0, L[1].tensors[40].data_ptr(), L[1].tensors[41].data_ptr() + 4 * 8 * 8 * 64)
    deps = engine.Engine.dependencies(_standin(L))
    hb = _deps_closure(deps)
    missing = [sa.describe(L, c) for c in found if not (hb[c.i] >> c.j) & 1]
    assert not missing, missing
    for ns in (2, 3):
        for assign in (None, [i % ns for i in range(len(L))], [(i // 3) % ns for i in range(len(L))]):
            where, waits = engine.capture_waits(deps, ns, assign)
            assert sa.audit(L, where, waits, found) == []
            if assign is not None:
                assert where == assign and any(waits)


def test_teeth_a_group_member_in_its_own_storage_is_seen_by_the_audit_only():
    L = synthetic_launches(split_member=True)
    deps = engine.Engine.dependencies(_standin(L))
    assert all(all(j < i for j in d) for i, d in enumerate(deps))                          # what the engine tests assert: still true
    assert 1 not in deps[3]                                                                # the RAW edge group -> consumer is gone
    assign = [0, 0, 0, 1] + [0] * (len(L) - 4)
    where, waits = engine.capture_waits(deps, 2, assign)
    bad = sa.audit(L, where, waits)
    assert bad and any("launch 1 " in s and "launch 3 " in s and "slot 41" in s and "RAW" in s for s in bad), bad
    good = synthetic_launches()
    where, waits = engine.capture_waits(engine.Engine.dependencies(_standin(good)), 2, assign)
    assert sa.audit(good, where, waits) == []


def test_audit_names_launches_slot_and_bytes():
    L = synthetic_launches()
    n = len(L)
    where = [i % 2 for i in range(n)]
    bad = sa.audit(L, where, [[] for _ in range(n)])                                       # two streams, no waits at all
    assert bad
    c = [c for c in sa.conflicts(L) if (c.j, c.i) == (6, 7)][0]
    line = [s for s in bad if s.startswith("RAW: launch 6 ")][0]
    assert "cp_conv2d_f32" in line and "launch 7 cp_splitk_reduce_f32" in line and "slot 8" in line and "slot 0" in line
    assert "[%#x, %#x)" % (c.lo, c.hi) in line and c.hi - c.lo == 4 * L[6].tensors[8].numel()


def test_asap_orders_run_every_concurrent_pair_both_ways():
    L = synthetic_launches()
    deps = engine.Engine.dependencies(_standin(L))
    where, waits = engine.capture_waits(deps, 2, [(i // 2) % 2 for i in range(len(L))])
    hb = sa.happens_before(where, waits)
    conc = sa.concurrent(hb)
    assert conc and sa.concurrent_pairs(hb) > 0
    seen = set()
    for j in conc:
        order = sa.asap(j, hb)
        assert sa.is_linear_extension(order, hb)
        pos = {p: k for k, p in enumerate(order)}
        seen |= {(a, b) for a in range(len(L)) for b in range(len(L)) if a != b and pos[a] < pos[b]}
    unordered = [(a, b) for b in range(len(L)) for a in range(b) if not (hb[b] >> a) & 1]
    assert len(unordered) == sa.concurrent_pairs(hb) and all(where[a] != where[b] for a, b in unordered)
    assert all((a, b) in seen and (b, a) in seen for a, b in unordered)
    assert set(conc) == {p for pair in unordered for p in pair}


def test_poison_fills_written_storages_only_and_indices_with_ints():
    L = synthetic_launches()
    e = _standin(L)
    x, w = L[0].tensors[0], L[0].tensors[4]
    x.fill_(3.0)
    sa.poison(e, "A")
    assert torch.all(x == 3.0) and torch.all(w == 0.0)                                     # the input and the constants: untouched
    assert torch.all(L[1].tensors[48] == 1234.5) and torch.all(L[7].tensors[3] == 1234.5)
    wsd = L[15].tensors[5]
    st = torch.empty(0).set_(wsd.untyped_storage(), 0, (wsd.untyped_storage().nbytes() // 4,), (1,))
    assert torch.all(st.view(torch.int32) == 1)                                            # scores and indices: ONE storage, all ints
    sa.poison(e, "B")
    assert torch.all(L[15].tensors[6] == 77.25) and torch.all(st.view(torch.int32) == 1)


# ---- random DAGs: engine.capture_waits ---------------------------------------------------------------------------------------------------
def _random_dag(rng, n):
    deps = []
    for i in range(n):
        k = min(i, rng.choice((0, 1, 1, 2, 3)))
        near = [j for j in range(max(0, i - 8), i)]
        pick = set(rng.sample(near, min(k, len(near))))
        if i and rng.random() < 0.15:
            pick.add(rng.randrange(i))
        deps.append(sorted(pick))
    return deps


@pytest.mark.parametrize("nstreams", [2, 3])
def test_capture_waits_closure_contains_the_dag(nstreams):
    cases = 0
    for seed in range(160):
        rng = random.Random(1000 * nstreams + seed)
        n = rng.randint(1, 60)
        deps = _random_dag(rng, n)
        for assign in (None, [rng.randrange(nstreams) for _ in range(n)]):
            where, waits = engine.capture_waits(deps, nstreams, assign)
            assert len(where) == len(waits) == n and all(0 <= s < nstreams for s in where)
            assert assign is None or where == assign
            hb = sa.happens_before(where, waits)
            for i, d in enumerate(deps):
                assert all((hb[i] >> j) & 1 for j in d), (seed, i, d)
                assert all(j in d and where[j] != where[i] for j in waits[i])            # only real edges, only across streams
                assert len({where[j] for j in waits[i]}) == len(waits[i])                 # at most one per source stream
            cases += 1
    assert cases >= 300


# ---- random op lists: cp_schedule_waits ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from centerpose_amd import _lib
    L = _lib.lib()
    L.cp_schedule_waits.restype = ctypes.c_int
    return L


# entry points that write exactly their last pointer, by pointer count: a random op borrows the name so that WRITES applies to it
FN_BY_NPTR = {2: "cp_maxpool2d_nhwc_f32", 3: "cp_shuffle_concat_nhwc_f32", 4: "cp_splitk_reduce_f32", 5: "cp_sum_up_nhwc_f32",
              6: "cp_dcn_v2_f32", 7: "cp_head3x3_1x1_f32", 9: "cp_conv2d_f32"}
NUMEL = 64


def _random_ops(rng, n, nbuf):
    """ops over `nbuf` buffers in the form of `plan.parse`: (fn, desc, refs, ints, out_index, stream); whole-buffer refs, constants
    and NULLs in between, now and then in place (the written buffer is also read)"""
    out = []
    for _ in range(n):
        nptr = rng.choice(sorted(FN_BY_NPTR))
        oi = nptr - 1
        near = lambda: min(nbuf - 1, max(0, int(rng.gauss(len(out) * nbuf / max(n, 1), 2))))
        refs = []
        for k in range(nptr):
            r = rng.random()
            refs.append((1, near(), 0, NUMEL) if k == oi or r < 0.35 else (2, rng.randrange(4), 0, 8) if r < 0.7 else (0, 0, 0, 0))
        if rng.random() < 0.1:
            refs[0] = refs[oi]
        out.append((FN_BY_NPTR[nptr], b"", refs, [], oi, rng.randrange(2)))
    return out


def _as_tensor_launches(plan_ops, nbuf):
    """the same ops as ops.Launch records over CPU tensors (one storage per buffer id): what Engine.dependencies reads"""
    bufs = [torch.zeros(NUMEL) for _ in range(nbuf)]
    consts = [torch.zeros(8) for _ in range(4)]
    return [ops.Launch(fn, None, [None if r[0] == 0 else bufs[r[1]] if r[0] == 1 else consts[r[1]] for r in refs], (), oi)
            for fn, _, refs, _, oi, _ in plan_ops]


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_cp_schedule_waits_orders_every_conflict_and_agrees_with_capture_waits(depth):
    for seed in range(110):
        rng = random.Random(7000 + 10 * seed + depth)
        n, nbuf = rng.randint(1, 60 // depth), rng.randint(1, 12)
        plan_ops = sa.pipeline_interleave(_random_ops(rng, n, nbuf), depth, nbuf)
        streams, waits = sa.plan_waits(plan_ops, depth * nbuf)
        found = sa.conflicts(plan_ops)
        assert sa.audit(plan_ops, streams, waits, found) == [], seed
        assert all(len(w) <= 1 and all(streams[j] != streams[i] for j in w) for i, w in enumerate(waits))
        # instances share no buffer: no conflict ever connects two of them
        assert all((c.j - c.i) % depth == 0 for c in found)
        # the same input through the Python path: Engine.dependencies on one storage per buffer id, capture_waits on the plan's streams
        L = _as_tensor_launches(plan_ops, depth * nbuf)
        assert {(c.j, c.i) for c in sa.conflicts(L)} == {(c.j, c.i) for c in found}
        where, pw = engine.capture_waits(engine.Engine.dependencies(_standin(L)), 2, streams)
        assert where == streams and sa.happens_before(where, pw) == sa.happens_before(streams, waits), seed


def test_cp_schedule_waits_rejects_bad_arguments(lib):
    I = ctypes.c_int
    pairs = (I * 4)()
    assert lib.cp_schedule_waits(1, (I * 1)(0), (I * 1)(1), (I * 1)(3), (I * 1)(0), 3, pairs, 2) == -1      # buffer id == nbuf
    assert lib.cp_schedule_waits(1, (I * 1)(0), (I * 1)(1), (I * 1)(0), (I * 1)(1), 3, pairs, 2) == -1      # out_index past the pointers
    assert lib.cp_schedule_waits(0, None, None, None, None, 0, None, 0) == 0
    assert lib.cp_abi_version() == 4
    # more pairs than `cap`: the count is still the whole number
    assert lib.cp_schedule_waits(3, (I * 3)(0, 1, 0), (I * 3)(1, 2, 2), (I * 5)(0, 0, 1, 1, 2), (I * 3)(0, 1, 1), 3, pairs, 1) == 2
    assert list(pairs)[:2] == [1, 0]


# ---- teeth: every wait that is not implied by the rest is needed ---------------------------------------------------------------------------
def _every_needed_wait_is_caught(launches, where, waits, found):
    assert sa.audit(launches, where, waits, found) == []
    redundant = set(sa.redundant_waits(where, waits))
    needed = 0
    for i, ws in enumerate(waits):
        for j in ws:
            if (i, j) in redundant:
                continue
            bad = sa.unordered(launches, where, sa.without_wait(waits, i, j), found)
            assert bad and any((c.j, c.i) == (j, i) for c in bad), "dropping the wait of %d for %d goes unnoticed" % (i, j)
            needed += 1
    return needed


def test_teeth_dropping_any_needed_wait_is_reported():
    needed = 0
    L = synthetic_launches()
    deps = engine.Engine.dependencies(_standin(L))
    found = sa.conflicts(L)
    for ns in (2, 3):
        for assign in ([i % ns for i in range(len(L))], [(i // 3) % ns for i in range(len(L))], None):
            where, waits = engine.capture_waits(deps, ns, assign)
            needed += _every_needed_wait_is_caught(L, where, waits, found)
    assert needed >= 10


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_teeth_dropping_any_needed_wait_of_the_c_schedule_is_reported(depth):
    needed = 0
    for seed in range(40):
        rng = random.Random(9000 + 10 * seed + depth)
        n, nbuf = rng.randint(2, 45 // depth), rng.randint(1, 10)
        plan_ops = sa.pipeline_interleave(_random_ops(rng, n, nbuf), depth, nbuf)
        streams, waits = sa.plan_waits(plan_ops, depth * nbuf)
        needed += _every_needed_wait_is_caught(plan_ops, streams, waits, sa.conflicts(plan_ops))
    assert needed >= 100
