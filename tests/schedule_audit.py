"""Data-race audit of a multi-stream launch schedule, by byte range (pure Python; no GPU needed to import).

The product keeps three pieces of bookkeeping by hand: `Engine.dependencies` (edges per STORAGE, one written tensor per launch:
`Launch.out_index`), the wait elision of `engine.capture_waits` and its C twin `cp_schedule_waits` (plan_runtime.cpp), and the
`BufferPool` reuse that adds WAR edges.  This module judges their RESULT -- the stream of every launch and the event waits actually
issued -- from first principles and shares nothing with them:

  * `WRITES`: per C entry point, the slots of the flat `Launch.tensors` record the function writes through.  Written by hand from the
    prototypes of include/centerpose_hip.h (tests/test_schedule_audit_cpu.py checks it against the `const` qualifiers there).
  * `extent`: the byte hull of a tensor view; `conflicts`: every pair of launches whose hulls overlap with a write on at least one
    side -- plain interval overlap, never storage identity, never `out_index`.
  * `happens_before`: the transitive closure of per-stream FIFO order plus the waits; `audit`: the conflicts it does not order.
  * `asap` / `poison`: the dynamic side (tests/test_schedule_audit_hip.py).  Two launches that happens-before leaves unordered are on
    different streams and may run in either order; `asap(j)` is the legal serial order that runs launch j as early as possible, so
    the orders {asap(j)} execute every concurrent pair both ways round, deterministically, on ONE stream.

What it cannot see: a kernel that writes outside every tensor it is handed (the per-launch oracle's "no store past the channel count"
checks own that), and a hull is a hull -- two views interleaved in one range (the two halves of a channel-shuffled activation) count
as overlapping, which can only add a conflict, never hide one.
"""
import collections

# ---- the C functions' write sets ---------------------------------------------------------------------------------------------------------
# slot numbers of ops.Launch.tensors (the order ops.marshal / plan_runtime.cpp::run_op document), per entry point of ops.FN_IDS
WRITES = {
    "cp_conv2d_f32": (8,),                                  # src x4, w, scale, shift, res, OUT
    "cp_conv3x3_winograd_f32": (5,),                        # src, u, scale, shift, res, OUT
    "cp_dcn_v2_f32": (5,),                                  # x, om, w, scale, shift, OUT
    "cp_stem7x7_f32": (4,),                                 # x, w, scale, shift, OUT
    "cp_maxpool2d_nhwc_f32": (1,),                          # in, OUT
    "cp_dw_deconv_add_nhwc_f32": (3,),                      # in, w, add, OUT
    "cp_sum_up_nhwc_f32": (4,),                             # src x4, OUT
    "cp_dwconv2d_nhwc_f32": (4,),                           # in, w, scale, shift, OUT
    "cp_global_avgpool_nhwc_f32": (1,),                     # in, OUT
    "cp_scale_add_nhwc_f32": (3,),                          # x, se, add, OUT
    "cp_shuffle_concat_nhwc_f32": (2,),                     # x1, x2, OUT
    "cp_head3x3_1x1_f32": (6,),                             # src, u, scale, shift, w2, b2, OUT2
    "cp_decode_topk_f32": (2, 3),                           # heat, hm_hp, WS_SCORES, WS_INDS
    "cp_decode_assign_f32": (6,),                           # wh, kps, reg, hp_offset, ws_scores, ws_inds, DETS
    "cp_splitk_reduce_f32": (3,),                           # ws, scale, shift, OUT
    "cp_conv3x3_winograd24_group_f32": (20, 21, 22, 23, 24),            # (src, u, scale, shift, res) x4, OUT x4, the storage they live in
    "cp_conv2d_group_f32": (40, 41, 42, 43, 44, 45, 46, 47, 48),        # (src, w, scale, shift, res) x8, OUT x8, the storage they live in
    "cp_sum_up_group_nhwc_f32": (16, 17, 18, 19, 20),                   # src x16, OUT x4, the storage they live in
    "cp_head_points_f32": (6,),                             # feat, ws_inds, w1, b1, w2, b2, OUT
    "cp_flip_merge_pairs_f32": (4, 5, 6, 7, 9),             # in x4, OUT x4, perm, the storage the outputs live in
    "cp_head_points_pairs_f32": (7,),                       # feat, ws_inds, perm, w1, b1, w2, b2, OUT
}
# slots a function reads as int32 INDICES into its other arguments (the decode workspace): `poison` never puts a float pattern there
INDEX_READS = {"cp_decode_assign_f32": (5,), "cp_head_points_f32": (1,), "cp_head_points_pairs_f32": (1,)}

POISON = {"A": 1234.5, "B": 77.25}

Conflict = collections.namedtuple("Conflict", "j i slot_j slot_i space lo hi kinds")      # launches j < i; kinds: subset of RAW WAR WAW


# ---- launches, extents -------------------------------------------------------------------------------------------------------------------
def _record(item):
    """(label, fn, slots) of an engine launch tuple (kind, name, flops, ops.Launch), a bare ops.Launch, or an op of `plan.parse`
    (fn name, desc, refs, ints, out_index, stream)."""
    if isinstance(item, tuple) and len(item) == 4:
        return "%s [%s]" % (item[1], item[3].fn), item[3].fn, item[3].tensors
    if isinstance(item, tuple) and len(item) == 6:
        return item[0], item[0], item[2]
    return item.fn, item.fn, item.tensors


def extent(t):
    """Byte hull (space, lo, hi) of one argument, or None for NULL / an empty tensor / a plan constant.  A tensor: space 0 and
    [data_ptr, data_ptr + 4 (1 + sum (size - 1) stride)); a plan-file ref (kind, buffer id, offset, numel): space = ("buf", id) and
    the bytes [4 offset, 4 (offset + numel)) of that buffer."""
    if t is None:
        return None
    if isinstance(t, tuple):
        kind, i, off, n = t
        return (("buf", i), 4 * off, 4 * (off + n)) if kind == 1 and n > 0 else None
    if t.numel() == 0:
        return None
    assert t.element_size() == 4
    span = 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
    return (0, t.data_ptr(), t.data_ptr() + 4 * span)


def accesses(launches):
    """[(space, lo, hi, launch, slot, is_write)] of every non-NULL argument of every launch."""
    acc = []
    for i, item in enumerate(launches):
        _, fn, slots = _record(item)
        wr = WRITES[fn]
        assert all(k < len(slots) for k in wr), "%s: WRITES names slot %d of %d" % (fn, max(wr), len(slots))
        for k, t in enumerate(slots):
            # a plan file lists as buffers the storages of the `out_index` tensors: a written slot filed as a constant is a lost write
            assert not (isinstance(t, tuple) and t[0] == 2 and k in wr), "launch %d (%s) writes slot %d through a plan CONSTANT" % (i, fn, k)
            e = extent(t)
            if e is not None:
                acc.append(e + (i, k, k in wr))
    return acc


def conflicts(launches):
    """Every pair of launches j < i that touch overlapping bytes with a write on at least one side: one `Conflict` per pair (the
    first overlapping slots found, the union of the kinds RAW / WAR / WAW over all of them), sorted by (i, j)."""
    found = {}
    by_space = collections.defaultdict(list)
    for a in accesses(launches):
        by_space[a[0]].append(a)
    for space, acc in by_space.items():
        if not any(a[5] for a in acc):
            continue
        acc.sort(key=lambda a: (a[1], a[2]))
        for x, a in enumerate(acc):
            for y in range(x + 1, len(acc)):
                b = acc[y]
                if b[1] >= a[2]:
                    break                                   # sorted by lo: nothing further overlaps a
                if a[3] == b[3] or not (a[5] or b[5]):
                    continue
                first, second = (a, b) if a[3] < b[3] else (b, a)
                kind = "WAW" if first[5] and second[5] else "RAW" if first[5] else "WAR"
                key = (first[3], second[3])
                lo, hi = max(a[1], b[1]), min(a[2], b[2])
                if key in found:
                    found[key] = found[key]._replace(kinds=found[key].kinds | {kind})
                else:
                    found[key] = Conflict(first[3], second[3], first[4], second[4], space, lo, hi, frozenset([kind]))
    return sorted(found.values(), key=lambda c: (c.i, c.j))


# ---- the order the capture guarantees ----------------------------------------------------------------------------------------------------
def happens_before(where, waits):
    """hb[i] = bit set of the launches guaranteed to have finished before launch i starts: the previous launch of its stream and the
    launches it waits for, transitively.  Launches are numbered in issue order; a wait names an earlier launch."""
    hb, last = [], {}
    for i, s in enumerate(where):
        m = 0
        for p in ([last[s]] if s in last else []) + list(waits[i]):
            assert 0 <= p < i, "launch %d waits for launch %d, which is not issued before it" % (i, p)
            m |= hb[p] | (1 << p)
        hb.append(m)
        last[s] = i
    return hb


def unordered(launches, where, waits, found=None):
    """the conflicts (default: `conflicts(launches)`) that happens-before does not order"""
    hb = happens_before(where, waits)
    return [c for c in (conflicts(launches) if found is None else found) if not (hb[c.i] >> c.j) & 1]


def describe(launches, c, where=None):
    (lj, _, _), (li, _, _) = _record(launches[c.j]), _record(launches[c.i])
    st = (" (stream %d)" % where[c.j], " (stream %d)" % where[c.i]) if where is not None else ("", "")
    return "%s: launch %d %s%s slot %d <-> launch %d %s%s slot %d, bytes [%#x, %#x) of %s" % (
        "/".join(sorted(c.kinds)), c.j, lj, st[0], c.slot_j, c.i, li, st[1], c.slot_i, c.lo, c.hi,
        "the address space" if c.space == 0 else "buffer %d" % c.space[1])


def audit(launches, where, waits, found=None):
    """The data races of a schedule: one line per conflicting pair that the capture does not order.  [] = race-free."""
    assert len(where) == len(waits) == len(launches)
    return [describe(launches, c, where) for c in unordered(launches, where, waits, found)]


def concurrent(hb, where=None):
    """launches with at least one partner that happens-before orders in neither direction (always on another stream)"""
    n = len(hb)
    full = (1 << n) - 1
    desc = [0] * n
    for i in range(n):
        m = hb[i]
        while m:
            low = m & -m
            desc[low.bit_length() - 1] |= 1 << i
            m ^= low
    return [j for j in range(n) if (full & ~(hb[j] | desc[j] | (1 << j)))]


def concurrent_pairs(hb):
    """number of unordered pairs"""
    n = len(hb)
    return n * (n - 1) // 2 - sum(bin(m).count("1") for m in hb)


def asap(j, hb):
    """The linear extension of happens-before that runs launch j as early as possible: its ancestors in issue order, j, then the rest
    in issue order.  For an unordered pair (i, j), asap(j) runs j before i and asap(i) runs i before j."""
    anc = [p for p in range(j) if (hb[j] >> p) & 1]
    rest = [p for p in range(len(hb)) if p != j and not (hb[j] >> p) & 1]
    return anc + [j] + rest


def is_linear_extension(order, hb):
    pos = {p: k for k, p in enumerate(order)}
    return sorted(order) == list(range(len(hb))) and all(pos[p] < pos[i] for i in range(len(hb)) for p in range(i) if (hb[i] >> p) & 1)


def redundant_waits(where, waits):
    """the (launch, awaited launch) waits whose removal leaves happens-before unchanged"""
    hb = happens_before(where, waits)
    out = []
    for i, ws in enumerate(waits):
        for j in ws:
            if happens_before(where, without_wait(waits, i, j)) == hb:
                out.append((i, j))
    return out


def without_wait(waits, i, j):
    w = [list(x) for x in waits]
    w[i].remove(j)
    return w


# ---- the C runtime's view ---------------------------------------------------------------------------------------------------------------
def c_waits(streams, bufids, out_index, nbuf):
    """`cp_schedule_waits` of the library (host code: no device needed) on per-op lists -> waits in the form of
    engine.capture_waits (per op the list of awaited ops)"""
    import ctypes
    from centerpose_amd import _lib
    L = _lib.lib()
    L.cp_schedule_waits.restype = ctypes.c_int
    n = len(streams)
    arr = lambda v: (ctypes.c_int * max(len(v), 1))(*v)
    flat = [b for ids in bufids for b in ids]
    pairs = (ctypes.c_int * (2 * max(n, 1)))()
    cnt = L.cp_schedule_waits(n, arr(streams), arr([len(ids) for ids in bufids]), arr(flat), arr(out_index), nbuf, pairs, n)
    assert 0 <= cnt <= n, "cp_schedule_waits: %d" % cnt
    waits = [[] for _ in range(n)]
    for k in range(cnt):
        waits[pairs[2 * k]].append(pairs[2 * k + 1])
    return waits


def plan_waits(plan_ops, nbuf):
    """(streams, waits) the C runtime derives for the ops of `plan.parse` (or `pipeline_interleave` of them)"""
    streams = [o[5] for o in plan_ops]
    return streams, c_waits(streams, [[r[1] if r[0] == 1 else -1 for r in o[2]] for o in plan_ops], [o[4] for o in plan_ops], nbuf)


def pipeline_interleave(plan_ops, depth, nbuf):
    """the ops of `depth` instances of one plan as cp_pipeline_process enqueues them: op i of instance 0, of instance 1, ...; odd
    instances with the two streams swapped; buffer ids offset by the instance's base"""
    out = []
    for fn, desc, refs, ints, oi, st in plan_ops:
        for k in range(depth):
            out.append((fn, desc, [(kind, i + k * nbuf if kind == 1 else i, off, n) for kind, i, off, n in refs], ints, oi, st ^ (k & 1)))
    return out


# ---- the dynamic side --------------------------------------------------------------------------------------------------------------------
def written_storages(launches):
    """{storage address: (a tensor of it, holds indices)} of every storage some launch writes through (per WRITES); `holds indices`:
    some launch reads it as int32 indices (per INDEX_READS)."""
    out, index = {}, set()
    for item in launches:
        _, fn, slots = _record(item)
        for k in WRITES[fn]:
            if slots[k] is not None:
                out.setdefault(slots[k].untyped_storage().data_ptr(), slots[k])
        for k in INDEX_READS.get(fn, ()):
            index.add(slots[k].untyped_storage().data_ptr())
    return {p: (t, p in index) for p, t in out.items()}


def poison(engine, pattern):
    """Fill every storage some launch of `engine` writes before a run (the network input is not among them).  A storage that any
    launch reads as INDICES is filled with the int32 pattern 1 -- never with a float pattern; every other one with a finite float,
    POISON[pattern].  Every kernel reads its activation inputs as float data and keeps its addresses in range for any value there, so
    even a mis-ordered run reads valid memory."""
    import torch
    value = POISON[pattern]
    for t, is_index in written_storages(engine.launches).values():
        st = t.untyped_storage()
        flat = torch.empty(0, dtype=torch.float32, device=t.device).set_(st, 0, (st.nbytes() // 4,), (1,))
        if is_index:
            flat.view(torch.int32).fill_(1)
        else:
            flat.fill_(value)


def run_order(engine, order):
    """the engine's launches in `order`, eagerly, on the current stream"""
    for p in order:
        engine.launches[p][3].run()
