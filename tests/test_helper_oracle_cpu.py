"""CPU: the table of tests/helper_oracle.py is what it claims to be, and the oracle rejects what it is there to reject.

* every row is in the regime it names, by the launchers' geometry as `helper_oracle` restates it: x-block counts and the ragged tail,
  row-loop trip counts of 2 and 3, flat trip counts of 3 and 2, LIM exactly at the launcher's limit and one pixel more over it;
* `ew_split` emulated in 64-bit integers: exact over the whole LIM row, first wrong e = 987393 at width 226 for C4 = 4369;
* the float32 CPU evaluation of every tolerance row sits inside its bound (the bound is not tighter than float32 itself);
* stand-ins for a wrong kernel are rejected where they are wrong: tail x-segment unwritten, second pass of the row loop written to the
  first pass's rows, third flat iteration dropped, the one mis-split element at width 226, one average-pool pixel dropped, an
  up-sampling source row taken from the next image -- and the dense-tensor, global-max-norm style of tests/test_conv_hip.py accepts
  the mis-split (the stated gap);
* where no device is present, every refusal of `helper_oracle.REFUSALS` returns rc 1 and names launcher and argument.  No launch
  can happen there whichever way a check goes (an unrefused call returns rc 2), so the cases no buffer can back -- one pixel past
  LIM, a grid of 2^32 blocks -- run here and only here.
"""
import ctypes

import pytest
import torch

import helper_oracle as H
import layer_oracle as lo
from test_conv_hip import _close

NO_DEVICE = not torch.cuda.is_available()
LIM_C4 = H.LIM_C // 4
TOLERANCE_ROWS = [r.id for r in H.ROWS if not H.is_exact(r)]


def _geoms(row):
    return [(H.row_geometry(rows, wg, c4), rows, wg, wc, c4) for rows, wg, wc, c4 in H.launch_rows(row)]


# ---- the table's claims -------------------------------------------------------------------------------------------------------------
def test_every_pair_has_a_row():
    have = {(r.launcher, g) for r in H.ROWS for g in r.regimes}
    assert not [pair for pair in H.MUST_COVER if pair not in have]
    assert all(r.kernel for r in H.ROWS if r.launcher in H.ROW_MAJOR + ("sum_up_group", "global_avgpool", "shuffle_concat"))


@pytest.mark.parametrize("rid", [r.id for r in H.ROWS if r.launcher in H.ROW_MAJOR + ("sum_up_group",)])
def test_row_major_rows_are_in_their_regimes(rid):
    row = H.ROW[rid]
    gs = _geoms(row)
    assert set(row.regimes) <= {"XN", "YS", "LIM", "VIEW"}
    if "XN" in row.regimes:                              # >= 3 x-blocks, ragged last one, C4 no power of two
        assert any(g["rowElems"] > 512 and g["xblocks"] >= 3 and g["tail"] < H.EW_THREADS and c4 & (c4 - 1) for g, _, _, _, c4 in gs), gs
    if "YS" in row.regimes and row.launcher != "sum_up_group":
        (g, rows, _, _, c4), = gs
        assert row.p["B"] == 2 and c4 == 1 and H.Y_MAX < rows and g["ygrid"] == H.Y_MAX
        assert g["passes"] in (2, 3) and 0 < g["multi"] < g["ygrid"]            # some grid rows take one trip more than the others
        ho = rows // row.p["B"]                                                   # a second pass lands in another image than its first
        assert any((y + H.Y_MAX) // ho != y // ho for y in (0, min(rows - H.Y_MAX, H.Y_MAX) - 1))
    if "YS" in row.regimes and row.launcher == "sum_up_group":                  # no row loop: >= 65536 rows go through first[]
        assert any(rows >= 65536 for _, rows, _, _, _ in gs)
        assert sum(rows * g["xblocks"] for g, rows, _, _, _ in gs) < 1 << 31
    if "LIM" in row.regimes:
        lim = [(wg, wc, c4) for _, _, wg, wc, c4 in gs if c4 == LIM_C4]
        assert len(lim) == 1
        wg, wc, c4 = lim[0]
        assert H.accepts(wc, c4)
        nxt = wc + 1 if row.launcher == "sum_up_group" else H.next_checked_width(row)
        assert not H.accepts(nxt, c4) and nxt - wc == row.p.get("f", 1)          # one more pixel of the row is refused
        assert H.first_wrong_split(wg, c4) is None
    if "VIEW" in row.regimes:
        assert row.p["pad"] == 16
    if row.launcher == "sum_up_group":
        assert len({g["xblocks"] for g, _, _, _, _ in gs}) >= 2 and 2 <= len(gs) <= 4
    if row.launcher in ("sum_up", "sum_up_group"):
        ms = row.p["members"] if row.launcher == "sum_up_group" else [row.p]
        assert all(0 <= s <= 3 and m["H"] % (1 << s) == 0 and m["W"] % (1 << s) == 0 for m in ms for s in m["shifts"])


def test_row_major_table_as_a_whole():
    by = lambda l: [r for r in H.ROWS if r.launcher == l]
    passes = {g["passes"] for r in H.ROWS if "YS" in r.regimes and r.launcher != "sum_up_group" for g, _, _, _, _ in _geoms(r)}
    assert passes == {2, 3}
    assert {(r.p["k"], r.p["s"], r.p["p"]) for r in by("maxpool")} >= {(2, 2, 0), (3, 2, 1)}
    dec = by("dw_deconv") + by("dw_deconv2")
    assert {r.p["f"] for r in by("dw_deconv")} >= {2, 4, 8} and {r.p["f"] for r in by("dw_deconv2")} == {2}
    assert {bool(r.p["add"]) for r in dec} == {True, False} and any(r.p["add"] == "inplace" and "VIEW" in r.regimes for r in dec)
    for r in dec:                                        # twins: same data, the other kernel
        if "twin" in r.p:
            t = H.ROW[r.p["twin"]]
            assert (r.kernel, t.kernel, r.p["env"], t.p["env"]) == (H.GENERIC, H.DECONV2, "0", "1")
            assert {k: v for k, v in r.p.items() if k not in ("twin", "env")} == {k: v for k, v in t.p.items() if k != "env"}
    assert {len(r.p["shifts"]) for r in by("sum_up")} == {1, 2, 3, 4}
    assert {s for r in by("sum_up") for s in r.p["shifts"]} == {0, 1, 2, 3}
    assert {len(r.p["members"]) for r in by("sum_up_group")} == {2, 3, 4}
    assert {(r.p["k"], r.p["s"], r.p["act"]) for r in by("dwconv")} >= {(k, s, a) for k, s in ((3, 1), (5, 2)) for a in H.ACTS}
    assert {r.p["add"] for r in by("scale_add")} == {True, False}
    # the deconvolutions' two limits: the launcher checks W * f, the f = 2 kernel walks W
    assert H.accepts(112 * 2, LIM_C4) and not H.accepts(113 * 2, LIM_C4) and H.ROW["deconv-f1-LIM"].p["W"] == H.LIM_W


@pytest.mark.parametrize("rid", [r.id for r in H.ROWS if r.launcher in ("shuffle_concat", "flip_merge", "fill", "dcn_pack")])
def test_flat_rows_are_in_their_regimes(rid):
    row = H.ROW[rid]
    n = H.flat_count(row)
    g = H.flat_geometry(n)
    if "FLAT" in row.regimes:                            # some threads run three iterations, the others two
        assert n > 2 * H.FLAT_SPAN and n % H.FLAT_SPAN != 0 and g["grid"] == H.FLAT_MAX and (g["most"], g["fewest"]) == (3, 2)
    if "SPAN" in row.regimes:
        assert n > H.FLAT_SPAN and (g["most"], g["fewest"]) == (2, 1)
    if "PAD" in row.regimes:
        p = row.p
        assert p["C"] % p["dg"] == 0 and (p["C"] // p["dg"]) % 16 != 0 and p["Cp"] // p["dg"] > p["C"] // p["dg"] and p["ldw"] > p["Co"]
        assert (p["Cp"] // p["dg"]) % 16 == 0
    if row.launcher == "flip_merge":
        p = row.p
        assert p["W"] % 2 == 1 and p["C"] * (H.flip_height(p["C"], p["W"]) - 1) * p["W"] <= 2 * H.FLAT_SPAN        # the smallest H for this W
    if rid == "shuffle-29":
        assert n - 2 * row.p["hp"] <= 2 * H.FLAT_SPAN                                                              # the fewest pixels
    if row.launcher == "fill":
        assert n == {"N0": 0, "N1": 1, "FLAT": 2 * H.FLAT_SPAN + 1}[row.regimes[0]]


def test_flat_table_as_a_whole():
    by = lambda l: [r for r in H.ROWS if r.launcher == l]
    assert {(r.p["mode"], r.p["C"]) for r in by("flip_merge")} == {(0, 2), (1, 17), (2, 34)}
    assert {(r.p["h"], r.p["hp"]) for r in by("shuffle_concat")} == {(116, 128), (29, 32)}
    assert H.ROW["shuffle-116"].p["H"] * H.ROW["shuffle-116"].p["W"] == 129 * 128
    assert {r.p["dg"] for r in by("dcn_pack")} == {1, 2, 4}
    assert {r.p["H"] for r in by("global_avgpool")} == {1, 3, 13, 67, 1000, 4099}
    for r in by("global_avgpool"):                       # two channel-quad blocks, the second ragged; views wider than C
        assert r.p["B"] == 3 and H.cdiv(r.p["C"] // 4, 32) == 2 and (r.p["C"] // 4) % 32 and r.p["pad"] > 0
    for r in by("nchw_to_nhwc") + by("nhwc_to_nchw"):
        p = r.p
        assert (p["B"], p["C"], p["H"], p["W"], p["cOff"], p["ld"]) == (3, 33, 35, 37, 16, 64) and (p["H"] * p["W"]) % 32 and p["C"] % 32


# ---- the multiply-high --------------------------------------------------------------------------------------------------------------
def test_split_emulation_is_exact_up_to_the_limit_and_wrong_one_pixel_past_it():
    assert LIM_C4 == 17 * 257 and (1 << 32) % LIM_C4 == 1 and H.magic(LIM_C4) == 983056
    assert H.accepts(H.LIM_W, LIM_C4) and not H.accepts(H.LIM_W + 1, LIM_C4)
    assert H.first_wrong_split(H.LIM_W, LIM_C4) is None
    e = H.first_wrong_split(H.LIM_W + 1, LIM_C4)
    assert e == 987393 == H.LIM_W * LIM_C4 + LIM_C4 - 1
    assert H.split(e, LIM_C4) == (H.LIM_W + 1, -1)       # the last quad of the last pixel, taken for quad -1 of the pixel after it
    assert H.split(12345, 1) == (12345, 0)
    for c4 in sorted({c for r in H.ROWS if r.launcher in H.ROW_MAJOR + ("sum_up_group",) for _, _, _, _, c in _geoms(r)}):
        w = max(wg for r in H.ROWS if r.launcher in H.ROW_MAJOR + ("sum_up_group",) for _, _, wg, _, c in _geoms(r) if c == c4)
        assert H.first_wrong_split(w, c4) is None, (w, c4)


# ---- the bounds are not tighter than float32 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", TOLERANCE_ROWS)
def test_float32_evaluation_sits_inside_the_bound(rid):
    case = H.make_case(rid)
    o32, o64 = H.references(case)
    w, fails = H.judge(case, [o.val for o in o32], o32, o64)
    assert not fails and w.ratio <= H.bound(case, o64), (w, fails)
    assert H.bound(case, o64) <= lo.LAYER_TOL["direct"] and H.bound(case, o64) <= o64[0].K + 3
    assert float(o64[0].A.min()) > 0


# ---- stand-ins for a wrong kernel -----------------------------------------------------------------------------------------------------
def _ref(rid):
    case = H.make_case(rid)
    o32, o64 = H.references(case)
    return case, o32, o64


@pytest.mark.parametrize("rid", ["scale_add-XN-add", "maxpool-3x3-XN", "sum_up-4-XN", "dwconv-3x3s1-none-XN", "deconv-f8-XN-add"])
def test_unwritten_tail_segment_is_rejected(rid):
    case, o32, o64 = _ref(rid)
    (g, rows, wg, _, c4), = _geoms(case.row)
    ref = o32[0].val
    r = H.as_rows(ref).clone()
    e0 = (g["xblocks"] - 1) * H.EW_THREADS               # first element of the last x-block
    r[:, 4 * e0:] = float("nan")
    out = H.from_rows(r, ref.shape)
    w, fails = H.judge(case, [out], o32, o64)
    assert fails
    bad = out != ref
    assert not bool(H.as_rows(bad)[:, :4 * e0].any()) and bool(H.as_rows(bad)[:, 4 * e0:].all())
    if w is not None:                                    # a tolerance row: the worst element lies in the tail
        assert w.ratio == float("inf") and w.loc[3] * c4 * 4 + w.loc[1] >= 4 * e0


@pytest.mark.parametrize("rid", ["scale_add-YS", "maxpool-YS", "dwconv-YS"])
def test_second_pass_written_to_the_first_pass_rows_is_rejected(rid):
    case, o32, o64 = _ref(rid)
    (g, rows, _, _, _), = _geoms(case.row)
    ref = o32[0].val
    r = H.as_rows(ref).clone()
    r[:rows - H.Y_MAX] = r[H.Y_MAX:].clone()
    r[H.Y_MAX:] = float("nan")
    out = H.from_rows(r, ref.shape)
    w, fails = H.judge(case, [out], o32, o64)
    assert fails
    wrong = H.as_rows(out != ref).any(1)
    assert bool(wrong[:rows - H.Y_MAX].all()) and bool(wrong[H.Y_MAX:].all()) and not bool(wrong[rows - H.Y_MAX:H.Y_MAX].any())


@pytest.mark.parametrize("rid", ["fill-big", "flip_merge-m0"])
def test_dropped_third_flat_iteration_is_rejected(rid):
    case, o32, o64 = _ref(rid)
    ref = o32[0].val
    out = ref.clone()
    out.view(-1)[2 * H.FLAT_SPAN:] = float("nan")
    _, fails = H.judge(case, [out], o32, o64)
    assert fails
    first = lo.first_unequal(out.view(-1), ref.view(-1))
    assert first == (2 * H.FLAT_SPAN,) and 0 < ref.numel() - first[0] < H.FLAT_SPAN


def _mis_split_copy(x, ld):
    """a one-source, shift-0 cp_sum_up_nhwc_f32 with ReLU over ONE row of W pixels x C channels at pixel stride `ld`, every element's
    (pixel, quad) taken from the emulated multiply-high: element e reads and writes the four floats at x_e * ld + 4 c4_e.  -> [W, C]"""
    W, C = x.shape
    C4 = C // 4
    src = torch.full(((W + 1) * ld,), float("nan"))
    src[:W * ld].view(W, ld)[:, :C] = x
    dst = torch.full(((W + 1) * ld,), float("nan"))
    xe, ce = H.split(torch.arange(W * C4, dtype=torch.int64), C4)
    addr = xe * ld + 4 * ce
    for j in range(4):
        dst[addr + j] = torch.relu(src[addr + j])
    return dst[:W * ld].view(W, ld)[:, :C]


@pytest.fixture(scope="module")
def past_the_limit():
    """one row of width 226 at C = 17476: the shape the launchers refuse"""
    x = torch.randn(H.LIM_W + 1, H.LIM_C, generator=torch.Generator().manual_seed(7))
    return x, torch.relu(x)


def test_the_one_mis_split_element_is_rejected(past_the_limit):
    """on a view (ld > C) the mis-split element goes to the padding of its pixel: its own four channels stay unwritten"""
    x, ref = past_the_limit
    out = _mis_split_copy(x, H.LIM_C + 4)
    nchw = lambda v: v.t().reshape(1, H.LIM_C, 1, H.LIM_W + 1)
    o = [lo.Out(nchw(ref), exact=True)]
    w, fail = lo.judge(nchw(out), o[0], o[0], "direct")
    assert fail
    bad = (out != ref).nonzero()
    assert bad.tolist() == [[H.LIM_W, H.LIM_C - 4 + j] for j in range(4)]
    assert lo.first_unequal(nchw(out), nchw(ref)) == (0, H.LIM_C - 4, 0, H.LIM_W)


def test_dense_max_norm_style_accepts_the_mis_split(past_the_limit):
    """the stated gap: with dense tensors (ld == C, as tests/test_conv_hip.py allocates them) quad -1 of pixel x + 1 IS the last quad
    of pixel x, so the mis-split element reads and writes the right address and `_close(out, ref, 1e-5)` of test_sum_up passes"""
    x, ref = past_the_limit
    _close(_mis_split_copy(x, H.LIM_C), ref, 1e-5)


@pytest.mark.parametrize("rid", [r.id for r in H.ROWS if r.launcher == "global_avgpool"])
def test_dropped_avgpool_pixel_is_rejected(rid):
    """c u A is a worst-case bound (wider than LAYER_TOL's own c for a long sum): one pixel dropped from one partition is 1 / HW of a
    typical |x| and still far outside it, on every row"""
    case, o32, o64 = _ref(rid)
    x = case.t["x"].flatten(2)
    hw = x.shape[2]
    out = H.avgpool_partitions(x, drop=((hw - 1) % 8, (hw - 1) // 8))[..., None, None]       # the last trip of the last pixel's partition
    w, fails = H.judge(case, [out], o32, o64)
    assert fails and w.ratio > H.bound(case, o64)
    typical = float(x.abs().mean()) / hw
    assert typical > 10 * H.bound(case, o64) * lo.U * float(o64[0].A.max()), "a typical dropped pixel is not 10 x outside the bound"


def test_sum_up_source_row_from_the_next_image_is_rejected():
    """what an H the up-sampling factor does not divide does to the last rows of an image: source row y >> shift is row 0 of the next"""
    case, o32, o64 = _ref("sum_up-2-XN")
    xs = [x.clone() for x in case.t["xs"]]
    assert case.p["shifts"][0] == 1
    xs[0][0, :, -1] = case.t["xs"][0][1, :, 0]
    out = lo._sum_up(xs, case.p["shifts"], case.p["relu"]).val
    _, fails = H.judge(case, [out], o32, o64)
    assert fails
    wrong = (out != o32[0].val).flatten(3).any(3).any(1)                                     # [B, H]
    Hh = case.p["H"]
    assert wrong.nonzero().tolist() == [[0, Hh - 2], [0, Hh - 1]]


def test_ops_refuse_an_indivisible_map():
    from centerpose_amd import ops
    out, src = torch.zeros(2, 5, 4, 8), torch.zeros(2, 2, 2, 8)
    with pytest.raises(AssertionError, match="must divide"):
        ops.sum_up_launch([src], [1], out, True)
    with pytest.raises(AssertionError, match="must divide"):
        ops.sum_up_group_launch([([src], [1], out)], out, True)


# ---- refusals, where no launch can happen ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def no_launch_possible():
    """an UNREFUSED call must come back with rc 2 and nothing else: cp_fill_f32 with a dummy non-null pointer and n = 1"""
    if not NO_DEVICE:
        pytest.skip("a device is present: these calls carry dummy pointers and run only where no launch can happen")
    from centerpose_amd import _lib
    L = _lib.lib()
    rc = L.cp_fill_f32(ctypes.c_void_p(4096), ctypes.c_float(1.0), ctypes.c_longlong(1), ctypes.c_void_p(0))
    assert rc == 2 and "fill_kernel" in L.cp_last_error().decode(), (rc, L.cp_last_error())
    return True


@pytest.mark.parametrize("rid", [r.id for r in H.REFUSALS])
def test_launcher_refuses_without_a_device(rid, no_launch_possible):
    r = H.REFUSAL[rid]
    rc, msg = H.refuse(rid, device=False)
    assert rc == 1, (rc, msg)
    assert msg.startswith(r.launcher + ":") and r.arg in msg, msg
