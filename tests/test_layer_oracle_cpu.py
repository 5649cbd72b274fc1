"""The per-launch oracle (tests/layer_oracle.py) judged on its own, without a GPU: the float32 CPU evaluation of a hook stands in for
the kernel output.  Unmodified it passes; each single mutation the oracle exists for is rejected at the mutated element; the global
max-norm check of tests/test_conv_hip.py lets the first of them through (the gap this oracle closes, recorded as a test).

`RecordingBuilder` itself needs a device (PlanBuilder packs weights through the HIP library), so "every launch belongs to exactly one
record" is asserted in tests/test_layer_parity_hip.py; here the recording mix-in is checked on the shape-only walk.
"""
import pytest
import torch
import torch.nn.functional as F

import layer_oracle as lo
from centerpose_amd import nets
from centerpose_amd.nets import Act

CI, CO, H, W = 32, 24, 10, 12


def _close(out, ref, tol=2e-4):
    """tests/test_conv_hip.py::_close, restated (that module needs the HIP library to import)"""
    out, ref = out.detach().cpu().double(), ref.detach().cpu().double()
    err = (out - ref).abs().max().item()
    scale = max(ref.abs().max().item(), 1e-6)
    assert err <= tol * scale, "max err %.3e (scale %.3e)" % (err, scale)


@pytest.fixture(scope="module")
def conv_case():
    """one 3x3 conv + BN + residual + ReLU on post-ReLU data with the checkpoint's channel spread: (sd, args, o32, o64, pre32) with
    pre32 = the float32 value before residual and ReLU"""
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g)
    sd = {"c.weight": r(CO, CI, 3, 3) * 0.1, "b.weight": torch.rand(CO, generator=g) + 0.5, "b.bias": r(CO) * 0.1,
          "b.running_mean": r(CO) * 0.1, "b.running_var": torch.rand(CO, generator=g) + 0.5}
    sd = lo.spread_bn(sd)
    x, res = Act(H, W, CI, F.relu(r(2, CI, H, W))), Act(H, W, CO, F.relu(r(2, CO, H, W)))
    args = ([x], "c", "b", False, CO, 3, 1, 1, True, res, False)
    get = lambda a, nchw=False: a.t
    o32 = lo.evaluate("emit_conv", sd, args, get, torch.float32)[0]
    o64 = lo.evaluate("emit_conv", sd, args, get, torch.float64)[0]
    pre32 = lo.evaluate("emit_conv", sd, args[:8] + (False, None, False), get, torch.float32)[0].val
    return sd, args, o32, o64, pre32


def _scale(sd):
    return sd["b.weight"] / torch.sqrt(sd["b.running_var"] + lo.EPS)


def _dropped_tap(case):
    """mutation 1: the centre tap dropped at corner pixel (0, 0) of image 0 in the channel with the smallest folded-BN scale"""
    sd, args, o32, _, pre32 = case
    x, res = args[0][0].t, args[9].t
    c = int(_scale(sd).abs().argmin())
    tap = _scale(sd)[c] * (sd["c.weight"][c, :, 1, 1] * x[0, :, 0, 0]).sum()
    out = o32.val.clone()
    out[0, c, 0, 0] = F.relu(pre32[0, c, 0, 0] - tap + res[0, c, 0, 0])
    assert out[0, c, 0, 0] != o32.val[0, c, 0, 0]
    return out, (0, c, 0, 0)


def test_unmodified_float32_passes(conv_case):
    _, _, o32, o64, _ = conv_case
    w, fail = lo.judge(o32.val, o32, o64, "direct")
    assert fail is None and w.ratio <= lo.C_REF32["direct"]


def test_dropped_tap_in_lowest_scale_channel_is_rejected(conv_case):
    out, loc = _dropped_tap(conv_case)
    w, fail = lo.judge(out, conv_case[2], conv_case[3], "direct")
    assert fail is not None and w.loc == loc


def test_global_max_norm_passes_the_dropped_tap(conv_case):
    """the stated gap: `_close(out, ref, 2e-4)` of tests/test_conv_hip.py accepts mutation 1"""
    out, _ = _dropped_tap(conv_case)
    _close(out, conv_case[3].val)


def test_clamp_to_edge_on_one_border_row_is_rejected(conv_case):
    sd, args, o32, o64, _ = conv_case
    xp = F.pad(args[0][0].t, (1, 1, 1, 1))
    xp[:, :, 0, :] = xp[:, :, 1, :]                                        # top border: clamp to edge instead of zeros
    mut = lo._conv_bn(sd, xp, "c", "b", False, CO, 3, 1, 0, True, args[9].t, torch.float32).val
    out = o32.val.clone()
    out[:, :, 0, :] = mut[:, :, 0, :]
    w, fail = lo.judge(out, o32, o64, "direct")
    assert fail is not None and w.loc[2] == 0


def test_swapped_output_channels_are_rejected(conv_case):
    sd, _, o32, o64, _ = conv_case
    a, b = 1, 2                                                            # neither a fifth nor a seventh channel: the same spread
    assert 0.3 < float(_scale(sd)[a] / _scale(sd)[b]) < 3
    out = o32.val.clone()
    out[:, a], out[:, b] = o32.val[:, b], o32.val[:, a]
    w, fail = lo.judge(out, o32, o64, "direct")
    assert fail is not None and w.loc[1] in (a, b)


def test_nonzero_padding_channel_is_rejected():
    view = lo.View(H, W, CO, None, None)
    t = torch.zeros(2, H, W, 32)
    t[..., :CO] = 1.0
    assert lo.padding_violation(t, view) is None
    t[1, 3, 4, 27] = 1e-30
    assert lo.padding_violation(t, view) == (1, 3, 4, 27)
    split = lo.View(H, W, 2 * 10, None, (10, 16))                          # two halves of 10 logical in 16 physical channels
    t = torch.zeros(2, H, W, 32)
    t[..., 25] = 3.0                                                       # logical channel 19
    assert lo.padding_violation(t, split) is None
    t[0, 0, 0, 26] = 1.0
    assert lo.padding_violation(t, split) == (0, 0, 0, 26)
    hs = torch.full((2, 1, 1, 32), 0.5)
    assert lo.padding_violation(hs, lo.View(1, 1, CO, None, None), hsig=True) is None
    assert lo.padding_violation(hs, lo.View(1, 1, CO, None, None)) == (0, 0, 0, CO)


def test_residual_added_after_the_relu_is_rejected(conv_case):
    _, args, o32, o64, pre32 = conv_case
    out = F.relu(pre32) + args[9].t
    w, fail = lo.judge(out, o32, o64, "direct")
    assert fail is not None and float(pre32[w.loc]) < 0 and float(args[9].t[w.loc]) > 0


def test_exact_hooks_compare_bits():
    x = Act(6, 8, 16, torch.randn(2, 16, 6, 8, generator=torch.Generator().manual_seed(1)))
    get = lambda a, nchw=False: a.t
    o32 = lo.evaluate("emit_maxpool", {}, (x, 2, 2, 0), get, torch.float32)[0]
    o64 = lo.evaluate("emit_maxpool", {}, (x, 2, 2, 0), get, torch.float64)[0]
    assert lo.judge(o32.val, o32, o64, "direct") == (None, None)
    out = o32.val.clone()
    out[1, 3, 2, 1] = torch.nextafter(out[1, 3, 2, 1], torch.tensor(9.0))
    assert "(1, 3, 2, 1)" in lo.judge(out, o32, o64, "direct")[1]


def test_cap_of_a_short_sum():
    assert lo.c_for("direct", 2) == 5.0 and lo.c_for("direct", 10 ** 6) == lo.LAYER_TOL["direct"]
    assert lo.c_for("wino24", 2) == lo.LAYER_TOL["wino24"]                 # the dot-product bound does not hold in the transform domain


def test_winograd_restatement_is_a_convolution():
    g = torch.Generator().manual_seed(2)
    x, w = torch.randn(2, 5, 7, 11, generator=g).double(), torch.randn(4, 5, 3, 3, generator=g).double()
    ref = F.conv2d(x, w, None, 1, 1)
    for mw in (2, 4):
        assert float((lo.winograd3x3(x, w, 2, mw) - ref).abs().max()) < 1e-12


def test_layer_tol_table_is_up_to_date():
    """LAYER_TOL = MARGIN x the c_ref32 this machine measures.  c_ref32 is one element's ratio, and a CPU with another vector width
    sums in another order and moves it by tens of per cent: up to a quarter above the table is taken as the same table.  A table that
    is stale (another spread, a changed reference) is off by more, in either direction: under two thirds of it fails as well.  The
    same walk asserts that the data is live: activations O(1), every DCN and sigmoid head above `LIVE_FLOOR`."""
    c, where = lo.calibrate()
    print("\nc_ref32:", {k: round(v, 3) for k, v in c.items()}, where)
    for fam, v in c.items():
        assert lo.C_REF32[fam] / 1.5 <= v <= lo.C_REF32[fam] * 1.25, (fam, v, where[fam])
        assert lo.LAYER_TOL[fam] == lo.MARGIN * lo.C_REF32[fam]


def test_degenerate_dcn_and_head_data_is_noticed():
    """offsets that throw every sample off the map, saturated masks and saturated sigmoid maps are failures of the harness's own data"""
    om = torch.zeros(2, 27, 2, 3)
    assert lo.dcn_liveness(om) == (pytest.approx(14 / 27), 1.0)             # zero offsets on the 2 x 3 map: 2/3 of the rows x 7/9 of the columns
    live, fails = {}, []
    lo.note_liveness(live, fails, "ok", "emit_dcn", None, om)
    assert not fails and live["dcn_samples"][1] == "ok"
    far = om.clone()
    far[:, :18] = 1e5
    lo.note_liveness(live, fails, "far", "emit_dcn", None, far)
    assert len(fails) == 1 and "dcn_samples = 0.000" in fails[0] and live["dcn_samples"] == (0.0, "far")
    sat = om.clone()
    sat[:, 18:] = 40.0
    lo.note_liveness(live, fails, "sat", "emit_dcn", None, sat)
    assert len(fails) == 2 and "dcn_masks = 0.000" in fails[1]
    heads = [torch.full((1, n, 2, 3), 0.5) for _, n in nets.HEADS]
    lo.note_liveness(live, fails, "head", "emit_head", heads)
    assert len(fails) == 2 and live["sigmoid"][0] == 1.0
    heads[[h for h, _ in nets.HEADS].index("hm_hp")][:] = 1.0
    lo.note_liveness(live, fails, "head1", "emit_head", heads)
    assert len(fails) == 3 and "sigmoid = 0.000" in fails[2]


@pytest.mark.parametrize("arch", lo.ARCHS)
def test_recording_counts_every_hook_once(arch):
    """shape-only walk: nested hook calls (the grouped hooks' one-by-one fall-back) belong to the outermost record"""
    class Counter(nets.Graph):
        n = 0

        def emit_conv(self, *a):
            self.n += 1
            return super().emit_conv(*a)

    sr, ct = lo.SpecRecorder(), Counter()
    sr.network(arch, Act(64, 96, 3))
    ct.network(arch, Act(64, 96, 3))
    assert {r.hook for r in sr.records} <= set(lo.HOOKS) and sr.records[-1].hook == "emit_head"
    convs = sum(1 if r.hook == "emit_conv" else len(r.args[0]) if r.hook in ("emit_conv_group", "emit_conv_batch") else 0 for r in sr.records)
    assert convs == ct.n
    assert dict(sr.spec) == dict(ct.spec)
    lo.check_partition(sr.records, 0)
    with pytest.raises(AssertionError):
        lo.check_partition([lo.Record("emit_conv", (), None, 0, 2), lo.Record("emit_conv", (), None, 1, 3)], 4)
