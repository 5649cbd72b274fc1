"""The launch-level oracle (tests/launch_oracle.py) judged on its own, without a GPU.

* Every row of the table tests/test_variant_parity_hip.py runs on the device is evaluated here in float32 on the CPU -- direct for the
  direct and DCN families, the textbook F(2x2) / F(2x4) transform for the Winograd ones -- and must stay within 1.25 x C_REF32 of the
  float64 reference (the allowance `test_layer_tol_table_is_up_to_date` gives another CPU's summation order): the reference alone is
  inside the bound the kernels are held to, LAYER_TOL = 4 x C_REF32.  A row over it gets other data, never another table.  The same
  walk asserts the liveness floors of every DCN and sigmoid row and that the persistent rows are in the walking regime.
* The harness can fail: the float32 evaluation stands in for the kernel, one mutation is applied, and each is rejected at the mutated
  element; `_close(out, ref, 1e-4)` of tests/test_conv_hip.py::test_head3x3_1x1_fused lets the first one through.
"""
import collections

import pytest
import torch
import torch.nn.functional as F

import launch_oracle as L
import layer_oracle as lo
from test_layer_oracle_cpu import _close
from test_variant_parity_hip import MUST_COVER

f32, f64 = torch.float32, torch.float64
Ref = collections.namedtuple("Ref", "case o32 o64")


def _ref(rid):
    case = L.make_case(rid)
    with torch.no_grad():
        return Ref(case, L.evaluate(case, f32, L.yardstick_family(case.row)), L.evaluate(case, f64))


@pytest.mark.parametrize("rid", [r.id for r in L.ROWS])
def test_float32_yardstick_of_every_row_is_inside_the_calibration(rid):
    case, o32, o64 = _ref(rid)
    row = case.row
    w, fails = L.check(case, o32.val, o32, o64)
    live = L.live_fractions(case, o32.val)
    print("\n%-24s %-7s worst err / (u A) %.3f (1.25 x C_REF32 = %.2f) at %s  %s" % (rid, row.family, w.ratio, 1.25 * lo.C_REF32[row.family], w.loc, live))
    assert w.ratio <= 1.25 * lo.C_REF32[row.family], "change the row's data, not the table"
    assert not fails, fails
    assert set(live) == ({"dcn_samples", "dcn_masks"} if row.kind == "dcn" else {"sigmoid"} if row.p.get("sigmoid") else set())
    assert all(frac >= lo.LIVE_FLOOR[key] for key, frac in live.items())
    if row.p.get("walk"):
        assert L.walk_tiles(row.kernel, case.p["B"], case.Ho, case.Wo) >= L.walk_floor(row.kernel, L.NCU_DEFAULT)
        TH, TW, _ = L.walk_geometry(row.kernel)
        assert case.Ho % TH and case.Wo % TW and case.Wo > 3 * TW and case.Ho > 3 * TH          # ragged edges, interior tiles


def test_table_names_every_instantiation_and_every_asked_case():
    named = {r.kernel for r in L.ROWS}
    assert not [k for k in MUST_COVER if k not in named and k != "splitk_reduce_kernel"]
    heads = [r for r in L.ROWS if r.kind == "head"]
    per_inst = collections.defaultdict(set)
    for r in heads:
        per_inst[r.kernel].add(r.p["hc"])
        assert r.p["sigmoid"] == (r.p["cout"] in (1, 17)) and (r.p["B"], r.p["H"], r.p["W"]) == (2, 19, 37)
    assert len(per_inst) == 10 and all(len(v) >= 2 for v in per_inst.values())
    assert {r.p["hc"] for r in heads} == {32, 96, 256} and {r.p["cout"] for r in heads} == {1, 2, 3, 17, 32, 33, 34}
    splits = lambda kern: sorted(r.p["S"] for r in L.ROWS if r.p["S"] > 1 and r.kernel.startswith(kern))
    assert splits("igemm_conv_kernel") == [2, 3, 4] and splits("conv3x3_wino_kernel") == [2, 4, 8] and splits("dcn_igemm_kernel") == [3]
    for r in L.ROWS:
        if "<128," in r.kernel or "<256," in r.kernel:                                         # 128-row tiles: ragged M, >= 3 M blocks
            bm = int(r.kernel.split("<")[1].split(",")[0])
            c = L.make_case(r.id)
            M = r.p["B"] * c.Ho * c.Wo
            assert M % bm and M > 2 * bm


# ---- mutations -----------------------------------------------------------------------------------------------------------------------
HPS = "head-wino-n34-hc96"


@pytest.fixture(scope="module")
def head():
    """the 34-output F(2x2) head row: Ref + the float32 mid pre-activation and the weights of the 1x1"""
    ref = _ref(HPS)
    case = ref.case
    sd, hc = case.sd, case.p["hc"]
    pre = lo._affine(case.x, case.x.abs(), sd["h.0.weight"], *lo._fold(sd, None, "h.0.bias", hc, f32), act=None, pad=1, wino="wino").val
    return ref, pre, sd["h.2.weight"].reshape(-1, hc)


def _head_dropped_mid_channel(head):
    """mutation 1: at pixel (1, 7, 20) the largest single term of the 1x1 is dropped in the output row with the smallest |w2| spread"""
    ref, pre, w2 = head
    j = int(lo.spread_factors(w2.shape[0]).argmin())
    b, y, x = 1, 7, 20
    terms = w2[j] * F.relu(pre[b, :, y, x])
    out = ref.o32.val.clone()
    out[b, j, y, x] -= terms[int(terms.abs().argmax())]
    assert out[b, j, y, x] != ref.o32.val[b, j, y, x]
    return out, (b, j, y, x)


def test_head_dropped_mid_channel_is_rejected(head):
    out, loc = _head_dropped_mid_channel(head)
    w, fails = L.check(head[0].case, out, head[0].o32, head[0].o64)
    assert fails and w.loc == loc


def test_global_max_norm_passes_the_dropped_mid_channel(head):
    """the stated gap: `_close(out, ref, 1e-4)` of test_head3x3_1x1_fused accepts mutation 1"""
    out, _ = _head_dropped_mid_channel(head)
    _close(out, head[0].o64.val, 1e-4)


def test_head_missing_relu_is_rejected(head):
    """the ReLU between the two convolutions omitted for one mid channel at one pixel where its pre-activation is negative"""
    ref, pre, w2 = head
    b, y, x = 0, 18, 36                                                     # the ragged corner
    m = int(pre[b, :, y, x].argmin())
    assert float(pre[b, m, y, x]) < 0
    out = ref.o32.val.clone()
    out[b, :, y, x] += w2[:, m] * pre[b, m, y, x]
    w, fails = L.check(ref.case, out, ref.o32, ref.o64)
    assert fails and (w.loc[0], w.loc[2], w.loc[3]) == (b, y, x)


def test_head_swapped_outputs_are_rejected(head):
    ref = head[0]
    a, b_ = 1, 2                                                            # neither a fifth nor a seventh output: the same spread
    f = lo.spread_factors(34)
    assert f[a] == f[b_]
    out = ref.o32.val.clone()
    out[1, a, 3, 30], out[1, b_, 3, 30] = ref.o32.val[1, b_, 3, 30], ref.o32.val[1, a, 3, 30]
    w, fails = L.check(ref.case, out, ref.o32, ref.o64)
    assert fails and w.loc in ((1, a, 3, 30), (1, b_, 3, 30))


def test_dropped_partial_sum_of_one_split_is_rejected():
    """split launch (Winograd split-C, S = 4 over 13 stages): the partial sum of split 1 (stages 3 .. 5 = input channels 48 .. 95) never
    reaches the reduction for the first 64-channel tile of pixel row (1, 11, :); rejected inside that strip, and the strip's
    lowest-scale channel that the ReLU leaves alive there is outside its own bound as well"""
    case, o32, o64 = _ref("wino-split4")
    p, sd = case.p, case.sd
    S, sp, n = p["S"], 1, p["cin"] // 16
    c0, c1 = 16 * (sp * n // S), 16 * ((sp + 1) * n // S)
    scale, shift, _ = lo._fold(sd, "b", None, p["cout"], f32)
    part = F.conv2d(case.x[:, c0:c1], sd["c.weight"][:, c0:c1], None, 1, 1) * scale
    b, y = 1, 11
    out = o32.val.clone()
    pre = lo._conv_bn(sd, case.x, "c", "b", False, p["cout"], 3, 1, 1, False, None, f32, "wino").val      # before the ReLU
    out[b, :64, y, :] = F.relu(pre[b, :64, y, :] - part[b, :64, y, :])
    w, fails = L.check(case, out, o32, o64)
    assert fails and w.loc[0] == b and w.loc[1] < 64 and w.loc[2] == y
    alive = (o32.val[b, :64, y, :] > 0).any(1)
    c = int(torch.where(alive, scale.view(-1)[:64].abs(), torch.tensor(float("inf"))).argmin())
    assert lo.spread_factors(p["cout"])[c] == lo.spread_factors(p["cout"]).min()               # one of the x 1e-2 channels
    A = lo.tile_A(o64.A, "wino")
    wc = lo.worst_ratio(out[b:b + 1, c:c + 1, y:y + 1], o64.val[b:b + 1, c:c + 1, y:y + 1], A[b:b + 1, c:c + 1, y:y + 1])
    assert wc.ratio > lo.c_for("wino", o64.K)


def test_second_tile_from_the_first_tiles_patch_is_rejected():
    """persistent walk: block `slot` owns the tiles slot, slot + grid, ...; its second tile computed from the patch of its first --
    one 8 x 32 output tile taken from the wrong position -- is rejected inside that tile"""
    rid = "c16-s1-16"
    case, o32, o64 = _ref(rid)
    p, sd, kern = case.p, case.sd, case.row.kernel
    TH, TW, occ = L.walk_geometry(kern)
    tx_n, ty_n = -(-case.Wo // TW), -(-case.Ho // TH)
    grid = L.NCU_DEFAULT * occ
    assert L.walk_tiles(kern, p["B"], case.Ho, case.Wo) > 2 * grid
    where = lambda tl: (tl // tx_n // ty_n, (tl // tx_n) % ty_n * TH, tl % tx_n * TW)       # tile index -> (b, y0, x0)
    slot = tx_n + 1
    (b1, y1, x1), (b2, y2, x2) = where(slot), where(slot + grid)
    assert (b1, y1, x1) != (b2, y2, x2) and y2 + TH <= case.Ho and x2 + TW <= case.Wo and y1 + TH <= case.Ho and x1 + TW <= case.Wo
    scale, shift, _ = lo._fold(sd, "b", None, p["cout"], f32)
    pre1 = F.conv2d(F.pad(case.x, (1, 1, 1, 1))[b1:b1 + 1, :, y1:y1 + TH + 2, x1:x1 + TW + 2], sd["c.weight"]) * scale + shift
    out = o32.val.clone()
    out[b2, :, y2:y2 + TH, x2:x2 + TW] = F.relu(pre1[0] + case.res[b2, :, y2:y2 + TH, x2:x2 + TW])
    w, fails = L.check(case, out, o32, o64)
    assert fails and w.loc[0] == b2 and y2 <= w.loc[2] < y2 + TH and x2 <= w.loc[3] < x2 + TW
