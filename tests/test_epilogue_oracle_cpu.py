"""The epilogue oracle (tests/epilogue_oracle.py) judged on its own, without a GPU.

* `MUST_COVER`: the (instantiation, mode) pairs, (instantiation, mode, activation) and (instantiation, mode, residual) triples and the
  dispatcher's fall-back edges that tests/test_epilogue_parity_hip.py has to run, written out here from the launchers' switch
  statements; the table must hold them all.  What a table row EXPECTS -- the kernel name and the body of the epilogue
  (`expected_kernel`, `expected_path`) -- is a small Python restatement of the kernels' predicates.  On the device the only path
  evidence is the kernel name the launcher reports: a block that took the vector body where the restatement says scalar is caught only
  through its result (the untouched-memory rule, the per-element bound), not through a name.
* The float32 torch evaluation of every case -- direct, or the textbook F(2x2) / F(2x4) transform for the Winograd families -- stands in
  for the kernel, goes through the same flat NaN buffer and judge, and must pass: the reference alone is inside LAYER_TOL for all five
  activations, so no new calibration constant is needed.
* Liveness floors on the cases' own data (`epilogue_oracle.LIVE`, `layer_oracle.LIVE_FLOOR`).
* `reference` (scale / shift, residual, activation on the cached accumulation) is `lo._conv_bn` / `lo.dcn_stage` bit for bit.
* Mutations of the stand-in, each rejected on the row's own data.
"""
import collections

import pytest
import torch

import epilogue_oracle as E
import layer_oracle as lo

f32, f64 = torch.float32, torch.float64
IG = "igemm_conv_kernel<%s>"
GENERIC = (IG % "64, 64, 2, 2, 32, false", IG % "128, 32, 4, 1, 32, false", IG % "256, 16, 4, 1, 16, false", IG % "128, 128, 2, 2, 32, false",
           "igemm_bf16x3_kernel<128, 64>")
PATCHES = ("conv3x3_patch_kernel<16, 4, 1, 16>", "conv3x3_patch_kernel<32, 4, 1, 32>", "conv3x3_patch_kernel<64, 2, 2, 32>")
WINO = ("conv3x3_wino_kernel<1, 1, 16, 2>", "conv3x3_wino_kernel<1, 2, 16, 2>", "conv3x3_wino_vs64_kernel<0, 0>")
W24T, W24F = "conv3x3_wino24_kernel<true>", "conv3x3_wino24_kernel<false>"
DCN = ("dcn_igemm_kernel<64, 64, 2, 2, 32>", "dcn_igemm_kernel<64, 32, 4, 1, 16>")
HEADS = tuple(k % i for k in ("conv3x3_wino_vs64_kernel%s", "head_wino24_kernel%s") for i in ("<1, 0>", "<2, 0>", "<0, 1>", "<1, 1>", "<2, 1>"))
NHWC = ("V", "S-cout", "S-ld", "S-ptr", "S-res")
ALL5 = ("none", "relu", "sigmoid", "hswish", "hsigmoid")


def _must_cover():
    pairs, acts, ress = [], [], []
    for k in GENERIC:
        pairs += [(k, m) for m in NHWC + ("NCHW", "scatter")]
    for k in PATCHES + WINO:
        pairs += [(k, m) for m in NHWC]
    pairs += [(W24T, "V")] + [(W24F, m) for m in NHWC]
    for k in DCN:
        pairs += [(k, m) for m in ("V", "S-cout", "S-ld", "S-ptr", "NCHW")]
    pairs += [("splitk_reduce_kernel", "V"), ("splitk_reduce_kernel", "S-ptr")] + [(k, "heads") for k in HEADS]
    pairs += [(k, "V-pad") for k in (GENERIC[0], PATCHES[1], WINO[1], W24T, W24F, DCN[0])]
    for k, m in pairs:
        if k == W24T:                                       # the lean instantiation exists for no activation and ReLU only
            acts += [(k, m, a) for a in ("none", "relu")]
        elif k == W24F and m in ("V", "V-pad"):             # aligned, Cout % 4 == 0: generic only through the activation
            acts += [(k, m, a) for a in ("sigmoid", "hswish", "hsigmoid")]
        elif m == "heads":
            acts += [(k, m, a) for a in ("none", "sigmoid")]
        else:
            acts += [(k, m, a) for a in ALL5]
        has_res = k in GENERIC + PATCHES + WINO + (W24F,) and m not in ("NCHW",)
        if has_res and m == "S-res":
            ress.append((k, m, True))                       # the residual is what the mode misaligns: it is always there
        elif has_res and not (k == W24F and m in ("V", "V-pad")):
            ress += [(k, m, True), (k, m, False)]
        else:
            ress.append((k, m, k in (W24T, W24F)) if k in (W24T, W24F) else (k, m, False))
    return tuple(pairs), tuple(acts), tuple(ress)


PAIRS, ACT_TRIPLES, RES_TRIPLES = _must_cover()
P16, P32 = PATCHES[0], PATCHES[1]
G16, G32, G64, GSTEM = GENERIC[2], GENERIC[1], GENERIC[0], IG % "128, 64, 2, 2, 32, true"
C16 = {("c16-16-s1"): "conv3x3_c16_kernel<1, 1, 8, 32, 4, 2>", "c16-32-s1": "conv3x3_c16_kernel<2, 1, 8, 32, 2, 2>",
       "c16-16-s2": "conv3x3_c16_kernel<1, 2, 8, 16, 3, 2>", "c16-32-s2": "conv3x3_c16_kernel<2, 2, 8, 16, 3, 1>"}
# fall-back edges: (base, flipped predicate) -> the kernel the launch must land on (None: refused, nothing launched)
EDGES = dict(
    [((b, "eligible"), k) for b, k in C16.items()] +
    [((b, e), to) for b, to in (("c16-16-s1", P16), ("c16-32-s1", P32), ("c16-16-s2", G16), ("c16-32-s2", G32))
     for e in ("sigmoid", "hswish", "out+1", "outLd", "res+1", "src+1")] +
    [((b, "eligible"), "pw_conv_kernel<64, 64, 4>") for b in ("pw-44", "pw-88")] +
    [((b, e), G64) for b in ("pw-44", "pw-88") for e in ("sigmoid", "cout", "src+1", "out+1", "res+1")] +
    [(("stem3", "eligible"), "stem7x7_c16_kernel<64, 2, 3>")] + [(("stem3", e), GSTEM) for e in ("out+1", "outLd", "sigmoid", "res")] +
    [(("stem7-16", "eligible"), "stem7x7_c16_kernel<16, 1, 7>"), (("stem7-64", "eligible"), "stem7x7_c16_kernel<64, 2, 7>")] +
    [(("stem7-16", e), "stem7x7_kernel<16, 1, 8, 64>") for e in ("x+1", "out+1", "outLd")] +
    [(("stem7-64", e), "stem7x7_kernel<64, 2, 8, 32>") for e in ("x+1", "out+1", "outLd")] +
    [((b, e), None) for b in ("wino-1x1", "wino-1x2", "wino-vs64", "wino24", "head-wino", "head-wino24") for e in ("src+1", "u+1")] +
    [(("wino24", "eligible"), W24T)] + [(("wino24", e), W24F) for e in ("sigmoid", "hswish", "cout", "out+1", "res+1")] +
    [(("fb-bf16", "eligible"), "igemm_bf16x3_kernel<128, 64>"), (("fb-bf16", "src+1"), P32), (("dcn-64x64", "src+1"), DCN[0])])
# launches the launchers must refuse inside the modes
REFUSED = tuple((b, "NCHW") for b in ("ig-64x64", "ig-128x32", "ig-256x16", "ig-128x128", "bf16x3")) + (("splitk", "S-cout"), ("splitk", "S-ld"))
MUST_COVER = PAIRS + ACT_TRIPLES + RES_TRIPLES + tuple(EDGES.items()) + REFUSED


def test_table_holds_every_pair_triple_and_fallback_edge():
    live = [c for c in E.CASES if c.kernel is not None and c.mode != "fb"]
    have = {(c.kernel, c.mode) for c in live} | {(c.kernel, c.mode, c.act) for c in live} | {(c.kernel, c.mode, c.res) for c in live}
    have |= {((c.base, c.sub), c.kernel) for c in E.CASES if c.mode == "fb"}
    have |= {(c.base, c.mode) for c in E.CASES if c.kernel is None and c.mode != "fb"}
    missing = [k for k in MUST_COVER if k not in have]
    assert not missing, missing
    assert len(PAIRS) == 5 * 7 + 6 * 5 + 6 + 2 * 5 + 2 + 10 + 6
    # the F(2x4) fast -> generic edges the issue names are rows of the wino24 base
    assert all(c.tile == (E.BASE[c.base].p["tile"] if c.kernel is None or c.base == "wino24" else 0) for c in E.CASES if c.mode == "fb" and
               E.BASE[c.base].kind == "conv")
    w24 = {(c.mode, c.act, c.cout, c.off, c.roff): c.kernel for c in E.CASES if c.base == "wino24" and c.mode != "fb"}
    assert w24[("V", "relu", 44, 0, 0)] == W24T and w24[("V", "sigmoid", 44, 0, 0)] == W24F and w24[("V", "hswish", 44, 0, 0)] == W24F
    assert w24[("S-cout", "none", 43, 0, 0)] == W24F and w24[("S-ptr", "none", 44, 1, 0)] == W24F and w24[("S-res", "none", 44, 0, 1)] == W24F
    for gid, (kernel, members) in E.GROUPS.items():
        assert kernel == E.group_kernel(members)
    mixed = E.GROUPS["wino24-group-mixed"][1]
    assert [E.expected_path(m) for m in mixed] == ["vector", "vector", "mixed"] and [E.w24_fast(m) for m in mixed] == [True, True, False]
    assert [E.expected_path(m) for m in E.GROUPS["igemm-group"][1]] == ["vector", "scalar"]


def test_expected_paths_restate_the_predicates():
    path = {c.id: E.expected_path(c) for c in E.CASES}
    for c in E.CASES:
        fam, p = E.BASE[c.base].family, path[c.id]
        if c.base == "splitk":
            assert p == ("reject" if c.cout % 4 or c.ld % 4 else "vector"), c.id
            continue
        if c.mode in ("V", "V-pad"):
            assert p == "vector" and E.given(c) % 4 == 0 and E.given(c) == (c.cout + 4 if c.cpad else c.cout)
        if c.mode in ("S-ld", "S-ptr", "S-res"):
            assert p == "scalar", c.id
        if c.mode == "S-cout":
            assert p == ("mixed" if fam in ("wino", "wino24") else "scalar"), c.id
        if c.mode in ("NCHW", "heads"):
            assert p == ("reject" if c.res else "nchw")
        if c.mode == "scatter":
            assert p == ("vector" if c.cout % 4 == 0 else "scalar")
    # every mode reaches every base it applies to with all its sub-variants
    subs = collections.defaultdict(set)
    for c in E.CASES:
        subs[(c.base, c.mode)].add((c.cout, c.off, c.roff, c.ld, c.rld if c.res else 0, c.scatter))
    for bid in ("ig-64x64", "ig-128x32", "ig-256x16", "ig-128x128", "bf16x3", "dcn-64x64", "dcn-64x32"):
        assert {(s[0], s[1]) for s in subs[(bid, "NCHW")]} >= {(co, off) for co in (1, 17, 34) for off in (0, 1)}
    for bid in ("sc-64x64", "sc-128x32", "sc-256x16", "sc-128x128", "sc-bf16x3"):
        got = {(s[5], s[0] % 4 == 0) for s in subs[(bid, "scatter")]}
        assert {ph for ph, _ in got} == {(0, 0), (0, 1), (1, 0), (1, 1), "fused"}
        assert {("fused", True), ("fused", False)} <= got and {v for ph, v in got if ph != "fused"} == {True, False}
    for (bid, mode), s in subs.items():
        if mode == "S-ptr":
            assert {v[1] for v in s} == {1, 2, 3} and all(v[3] % 4 == 0 for v in s)
        if mode == "S-cout" and bid != "patch-16":
            assert {v[0] for v in s} == {43, 27}
        if mode == "S-res":
            assert {(v[2], v[4] % 4) for v in s} == {(1, 0), (0, 1)}
    assert {c.cout for c in E.CASES if c.mode == "heads"} == {1, 2, 17, 33, 34} and all(c.off == 1 for c in E.CASES if c.mode == "heads")


KEYS = list(dict.fromkeys((c.base, c.mode) for c in E.CASES)) + [("group", g) for g in E.GROUPS]
_worst = {}


@pytest.mark.parametrize("bid,mode", KEYS, ids=["%s-%s" % k for k in KEYS])
def test_float32_yardstick_of_every_case_passes_the_judge(bid, mode):
    cases = E.GROUPS[mode][1] if bid == "group" else [c for c in E.CASES if (c.base, c.mode) == (bid, mode)]
    for c in cases:
        o64, o32 = E.reference(c), E.yardstick(c)
        lay, flat = E.standin(c, o32.val)
        w, fails, out = E.judge_flat(c, lay, flat, o64)
        fam = E.BASE[c.base].family
        assert not fails, (c.id, fails)
        assert w.ratio <= lo.LAYER_TOL[fam]                 # the reference alone stays inside the bound (c_for may cap it further)
        assert not E.live_failures(c), (c.id, E.live_failures(c), E.liveness(c))
        assert bool(torch.isfinite(o64.val).all()) and bool((o64.A > 0).all())
        if w.ratio > _worst.get((fam, c.act), (-1.0, ""))[0]:
            _worst[(fam, c.act)] = (w.ratio, c.id)
    for (fam, act), (ratio, cid) in sorted(_worst.items()):
        if cid in {c.id for c in cases}:
            print("\nyardstick worst err / (u A) %-7s %-8s %.3f (C_REF32 %.2f, LAYER_TOL %.1f)  %s" % (fam, act, ratio, lo.C_REF32[fam], lo.LAYER_TOL[fam], cid))


def test_liveness_floors_speak_about_every_activation():
    seen = collections.Counter()
    for c in E.CASES:
        if not E.rejected(c):
            seen.update(E.liveness(c).keys())
    assert set(seen) == {"relu_neg", "h_low", "h_high", "h_in", "sigmoid", "res_nonzero", "dcn_samples", "dcn_masks"}
    # without the gain the clamps of h-swish / h-sigmoid would never fire: the floor would fail
    c = E.CASE["ig-64x64/V/c44/hswish"]
    v, _, _ = E.pre_activation(c._replace(act="none"), f64)
    assert float((v.abs() > 3).double().mean()) < 0.1 <= E.liveness(c)["h_low"]


@pytest.mark.parametrize("cid", ["ig-64x64/V/c44/relu", "ig-128x32/S-cout/c27/relu", "patch-64/S-res/roff1/none+res", "c16-16-s2/fb/eligible/relu+res",
                                 "stem3/fb/res/relu+res", "wino-1x1/V/c44/none+res"])
def test_reference_is_conv_bn_on_the_cached_accumulation(cid):
    c = E.CASE[cid]
    b, d = E.BASE[c.base], E.base_data(c.base)
    p = b.p
    sd = E.params(c.base, c.act, c.cout)
    res = d.res[:, :c.cout] if c.res else None
    for dt, wino in ((f64, None), (f32, E.yardstick_family(c))):
        want = lo._conv_bn(sd, d.x.to(dt), "c", "b", False, c.cout, p["k"], p["stride"], p["pad"], c.act == "relu", res.to(dt) if c.res else None, dt, wino)
        got = E.reference(c, dt, wino)
        # a convolution over a prefix of the output channels is the prefix of the convolution
        assert torch.allclose(got.val, want.val, rtol=0, atol=0 if dt == f64 and not wino else 1e-5), cid
        if dt == f64:
            assert torch.allclose(got.A, want.A, rtol=1e-12, atol=0) and got.K == want.K


def test_reference_is_dcn_stage_on_the_cached_accumulation():
    c = E.CASE["dcn-64x64/V/c44/relu"]
    d = E.base_data(c.base)
    want = lo.dcn_stage(E.params(c.base, c.act, c.cout), d.x.double(), d.om, "d", "b", c.cout, f64)
    got = E.reference(c)
    assert torch.allclose(got.val, want.val, rtol=1e-12, atol=1e-12) and torch.allclose(got.A, want.A, rtol=1e-12, atol=0) and got.K == want.K


def test_scatter_reference_is_the_transposed_convolution():
    """the sub-pixel packing of ops.pack_deconv4_subpixel against conv_transpose2d(k4, s2, p1): phase (py, px) of the reference is the
    2 x 2 convolution with that phase's weights"""
    import torch.nn.functional as F
    from centerpose_amd import ops
    c = E.CASE["sc-64x64/scatter/p01-c43/relu"]
    d = E.base_data(c.base)
    acc, _, _ = E.accumulate(c.base, f64)
    wd = d.sd["c.weight"].double()
    ci = wd.shape[0]
    for py in range(2):
        for px in range(2):
            wp = ops.pack_deconv4_subpixel(wd, py, px)[:wd.shape[1]].double()                  # [Co, 4 ci], k = (ty * 2 + tx) ci + c
            w2 = wp.view(-1, 2, 2, ci).permute(0, 3, 1, 2)
            xp = F.pad(d.x.double(), (1 - px, px, 1 - py, py))
            assert torch.allclose(F.conv2d(xp, w2), acc[:, :, py::2, px::2], rtol=0, atol=1e-12)


# ---- mutations: each is applied to the float32 stand-in and must be rejected on the row's own data -----------------------------------------
def _judge(c, out32, lay=None, flat=None):
    if flat is None:
        lay, flat = E.standin(c, out32, lay)
    return E.judge_flat(c, lay, flat, E.reference(c))


def _rejected(c, out32, **kw):
    w, fails, _ = _judge(c, out32, **kw)
    assert fails, c.id
    return w, fails


def _act32(c, v):
    return lo._activate(v, None, E._LO_ACT[c.act])[0]


RES_ROWS = ["ig-64x64/S-ld/ld45/sigmoid+res", "patch-32/S-ptr/off2/hsigmoid+res", "wino24/S-res/rld45/hswish+res", "ig-256x16/S-cout/c43/none+res",
            "sc-128x32/scatter/p00-c44/none+res"]


@pytest.mark.parametrize("cid", RES_ROWS)
def test_dropped_residual_is_rejected(cid):
    c = E.CASE[cid]
    _rejected(c, E.yardstick(c._replace(res=False)).val)


@pytest.mark.parametrize("cid", [r for r in RES_ROWS if "/none" not in r] + ["ig-128x128/S-res/rld45/relu+res"])
def test_residual_added_after_the_activation_is_rejected(cid):
    c = E.CASE[cid]
    d = E.base_data(c.base)
    _rejected(c, E.yardstick(c._replace(res=False)).val + d.res[:, :c.cout])


@pytest.mark.parametrize("cid", ["ig-128x32/S-ptr/off2/relu", "dcn-64x32/S-cout/c27/hswish", "bf16x3/NCHW/c34-off0/hsigmoid", "wino-1x2/S-ld/ld45/sigmoid+res",
                                 "head-wino/heads/n17/sigmoid"])
def test_activation_replaced_by_none_is_rejected(cid):
    c = E.CASE[cid]
    _rejected(c, E.yardstick(c._replace(act="none")).val)


@pytest.mark.parametrize("cid", ["patch-64/S-cout/c27/hswish", "wino-vs64/S-ptr/off2/hsigmoid+res", "dcn-64x64/V/c44/hswish"])
def test_hswish_and_hsigmoid_swapped_are_rejected(cid):
    c = E.CASE[cid]
    _rejected(c, E.yardstick(c._replace(act="hsigmoid" if c.act == "hswish" else "hswish")).val)


@pytest.mark.parametrize("cid", ["ig-64x64/S-cout/c43/none+res", "patch-16/S-ld/ld13/relu", "wino24/S-cout/c27/relu", "dcn-64x64/NCHW/c17-off0/hswish"])
def test_scale_and_shift_of_the_next_channel_are_rejected(cid):
    c = E.CASE[cid]
    b, d = E.BASE[c.base], E.base_data(c.base)
    acc, _, _ = E.accumulate(c.base, f32, E.yardstick_family(c))
    scale, shift, _ = lo._fold(E.params(c.base, c.act, c.cout), "b", "d.bias" if b.kind == "dcn" else None, c.cout, f32)
    v = acc[:, :c.cout] * scale.roll(-1, 1) + shift.roll(-1, 1)                                # channel n with scale[n + 1], shift[n + 1]
    if c.res:
        v = v + d.res[:, :c.cout]
    w, _ = _rejected(c, _act32(c, v))
    assert w.ratio > 100 * lo.LAYER_TOL[b.family]


@pytest.mark.parametrize("cid", ["ig-64x64/S-ptr/off1/none+res", "patch-32/V/c44/relu", "wino-1x1/S-cout/c43/none+res", "dcn-64x32/S-ld/ld45/sigmoid"])
def test_result_stored_one_channel_to_the_right_is_rejected(cid):
    c = E.CASE[cid]
    lay = E.layout(c)
    flat = E.new_flat(lay.size)
    flat[lay.idx + 1] = E.yardstick(c).val
    w, fails = _rejected(c, None, lay=lay, flat=flat)
    assert any("outside the output" in f for f in fails) and w.ratio == float("inf")


def test_swapped_scatter_phases_are_rejected():
    c01, c10 = E.CASE["sc-64x64/scatter/p01-c43/relu"], E.CASE["sc-64x64/scatter/p10-c44/sigmoid+res"]
    for c, other in ((c01, (1, 0)), (c10, (0, 1))):
        lay = E.layout(c)
        wrong = E.Layout(lay.B, lay.C, lay.OH, lay.OW, lay.ld, lay.off, False, other)
        flat = E.new_flat(lay.size)
        flat[wrong.idx] = E.logical(c, lay, E.yardstick(c).val)                                # the right values at the other phase's pixels
        w, fails = _rejected(c, None, lay=lay, flat=flat)
        assert any("outside the output" in f for f in fails) and w.ratio == float("inf")
    # and the right values of phase (1, 0) stored as phase (0, 1) in a buffer where both were to be written: judged by value alone
    full = E.yardstick(c10).val.clone()
    full[:, :, 1::2, 0::2], full[:, :, 0::2, 1::2] = full[:, :, 0::2, 1::2].clone(), full[:, :, 1::2, 0::2].clone()
    fused = E.CASE["sc-64x64/scatter/fused-c44/hsigmoid+res"]
    ok = E.yardstick(fused).val.clone()
    ok[:, :, 1::2, 0::2], ok[:, :, 0::2, 1::2] = ok[:, :, 0::2, 1::2].clone(), ok[:, :, 1::2, 0::2].clone()
    _rejected(fused, ok)


@pytest.mark.parametrize("cid", ["ig-128x128/NCHW/c17-off0/hswish", "dcn-64x64/NCHW/c34-off1/relu", "bf16x3/NCHW/c1-off1/sigmoid"])
def test_nchw_written_as_nhwc_is_rejected(cid):
    c = E.CASE[cid]
    lay = E.layout(c)
    b, ch, y, x = torch.meshgrid(*(torch.arange(n) for n in (lay.B, lay.C, lay.OH, lay.OW)), indexing="ij")
    flat = E.new_flat(lay.size)
    flat[lay.origin + lay.position(b, ch, y, x, nchw=False, ld=lay.C)] = E.yardstick(c).val
    w, fails, _ = _judge(c, None, lay=lay, flat=flat)
    if c.cout == 1:                                        # one channel: the two layouts are the same memory
        assert not fails
    else:
        assert fails and w.ratio > lo.LAYER_TOL[E.BASE[c.base].family]


@pytest.mark.parametrize("cid,where", [("ig-64x64/S-cout/c43/none+res", "past"), ("patch-16/S-cout/c7/relu", "past"), ("wino-1x2/S-ld/ld45/relu", "past"),
                                       ("ig-256x16/S-ptr/off3/sigmoid+res", "front"), ("dcn-64x64/NCHW/c17-off1/none", "front"),
                                       ("wino24/V/c44/relu", "guard"), ("head-wino24/heads/n34/none", "guard")])
def test_one_float_outside_the_output_is_rejected(cid, where):
    c = E.CASE[cid]
    lay, flat = E.standin(c, E.yardstick(c).val)
    assert not E.judge_flat(c, lay, flat, E.reference(c))[1]
    if where == "past":                                    # a fourth channel of the last float4: (b, y, x) = (1, 3, 5), channel Cout
        pos = lay.origin + int(lay.position(torch.tensor(1), torch.tensor(c.cout), torch.tensor(3), torch.tensor(5)))
    elif where == "front":                                 # the float in front of the slice / of the misaligned tensor
        pos = lay.origin - 1
    else:
        pos = lay.origin + lay.n + 3 if not lay.nchw else lay.origin + lay.n
    assert torch.isnan(flat[pos])
    flat[pos] = 0.0
    _, fails, _ = E.judge_flat(c, lay, flat, E.reference(c))
    assert len(fails) == 1 and "outside the output" in fails[0]


@pytest.mark.parametrize("cid", ["ig-64x64/V-pad/c44of48/relu", "wino24/V-pad/c44of48/hsigmoid+res", "dcn-64x64/V-pad/c44of48/sigmoid"])
def test_a_padding_channel_that_is_not_the_activation_of_zero_is_rejected(cid):
    c = E.CASE[cid]
    lay, flat = E.standin(c, E.yardstick(c).val)
    assert not E.judge_flat(c, lay, flat, E.reference(c))[1]
    pos = lay.origin + int(lay.position(torch.tensor(0), torch.tensor(c.cout + 1), torch.tensor(18), torch.tensor(36)))
    assert float(flat[pos]) == (0.5 if c.act in ("sigmoid", "hsigmoid") else 0.0)
    for wrong in (1e-30,) + ((0.0,) if c.act == "sigmoid" else ()):      # sigmoid(0) is 0.5 and nothing else; h-sigmoid keeps the existing rule
        flat[pos] = wrong
        _, fails, _ = E.judge_flat(c, lay, flat, E.reference(c))
        assert len(fails) == 1 and "padding channel" in fails[0]


def test_one_wrong_element_is_rejected_where_it_is():
    c = E.CASE["ig-64x64/S-ptr/off1/hswish"]
    out = E.yardstick(c).val.clone()
    o64 = E.reference(c)
    loc = (1, 43, 18, 36)                                  # last channel, ragged corner
    out[loc] += 64 * lo.U * float(o64.A[loc])
    w, fails = _rejected(c, out)
    assert w.loc == loc
