"""TEST INFRASTRUCTURE ONLY -- launch-level front end to the per-element fp64 oracle (tests/layer_oracle.py).

The network plans of tests/test_layer_parity_hip.py reach only the kernel instantiations their block counts select.  This module builds
ONE stand-alone launch through ``ops.*_launch`` with the variant forced (``tile`` / ``ksplit`` / ``wino24``), evaluates the same
operation in float32 and float64 with the pieces of ``layer_oracle`` (``_conv_bn`` -> ``_fold`` / ``_affine``, ``head_branch``,
``dcn_stage``, ``winograd3x3``, ``tile_A``, ``judge``, ``c_for``, ``padding_violation``, ``dcn_liveness``) and returns the ``Worst`` record
and the failure texts.  ``ROWS`` is the table both tests/test_variant_parity_hip.py (device) and tests/test_launch_oracle_cpu.py
(float32 CPU yardstick, mutations) walk.

Case data is fixed by seed and built on the CPU: post-ReLU inputs and residuals, `spread_bn`'s per-channel spread on every folded BN
scale (heads, which have no BN: on the rows of the 3x3 and, independently, of the 1x1 weights), sigmoid heads biased at the
reference's -2.19, offsets of a few pixels and unsaturated mask logits for the DCN rows.  Outputs go into NaN-filled buffers wider than
the channel count the launch is given: nothing may be stored past it, and the padding channels inside it must be exact zeros.

Nothing here reads device results or kernel sources to set a bound: every bound is `layer_oracle.c_for`.
"""
import collections
import functools

import torch
import torch.nn.functional as F

import layer_oracle as lo

NCU_DEFAULT = 256        # compute units of an MI355X: sizes the walking rows where no device is there to ask (the CPU yardstick)
SIGMOID_BIAS = -2.19     # the reference's initial bias of `hm`
Row = collections.namedtuple("Row", "id kind family kernel p")

# ---- the persistent kernels' geometry, as their launchers state it -----------------------------------------------------------------
# conv3x3_c16_kernel<NT, S, TH, TW, OCC, TBW> (cp_launch_conv3x3_c16): block tiles of TH x TW OUTPUT pixels, min(ntiles, CUs x OCC) blocks.
# stem7x7_c16_kernel<NOUT, S, KS> (S7C in stem7x7.hip): TH = 8 (NOUT = 16) / 4, TW = 64, OCC = 3 (NOUT = 16) / 4 (KS = 3) / 2.


def walk_geometry(kernel):
    """(TH, TW, OCC) of a persistent kernel instantiation, from its template arguments"""
    name, args = kernel.rstrip(">").split("<")
    a = [int(v) for v in args.split(",")]
    if name == "conv3x3_c16_kernel":
        return a[2], a[3], a[4]
    assert name == "stem7x7_c16_kernel", kernel
    return (8 if a[0] == 16 else 4), 64, (3 if a[0] == 16 else 4 if a[2] == 3 else 2)


def walk_tiles(kernel, B, Ho, Wo):
    TH, TW, _ = walk_geometry(kernel)
    return B * (-(-Ho // TH)) * (-(-Wo // TW))


def walk_floor(kernel, ncu):
    """ntiles >= 2 CUs OCC + 1: some blocks own three tiles (two chained prefetches), the others two"""
    return 2 * ncu * walk_geometry(kernel)[2] + 1


def _walk_shape(kernel, ncu, stride, B=2, tiles_x=5, quad=False):
    """smallest input (H, W) with `tiles_x` tile columns (interior tiles and all four borders), a ragged last tile in y and in x, that
    puts the launch into the walking regime; quad: W % 4 == 0 (the stems' float4 rows)"""
    TH, TW, _ = walk_geometry(kernel)
    tiles_y = -(-walk_floor(kernel, ncu) // (B * tiles_x))
    Ho, Wo = TH * (tiles_y - 1) + 3, TW * (tiles_x - 1) + (6 if quad else 5)
    if stride == 1:
        return Ho, Wo + (-Wo % 4 if quad else 0)
    return 2 * Ho - 1, 2 * Wo            # Ho = (H - 1) // 2 + 1, Wo = (W - 1) // 2 + 1 for 3x3 / p1 and 7x7 / p3 alike


def _r(id, kind, family, kernel, **p):
    d = dict(B=2, H=19, W=37, k=3, stride=1, pad=1, S=1, res=True, relu=True, tile=0)
    d.update(p)
    return Row(id, kind, family, kernel, d)


IG = "igemm_conv_kernel<%s>"
DCN = "dcn_igemm_kernel<%s>"
_HEADS = [(1, 32, True), (1, 256, True), (2, 96, False), (2, 256, False), (3, 32, False), (17, 96, True), (17, 256, True), (32, 256, False),
          (33, 32, False), (33, 96, False), (34, 96, False), (34, 256, False)]        # (n2, hc, sigmoid)


def _head_inst(n2):
    return "<1, 0>" if n2 == 1 else "<2, 0>" if n2 == 2 else "<0, 1>" if n2 <= 32 else "<1, 1>" if n2 == 33 else "<2, 1>"


# Every row: B = 2 and a map that is no multiple of any tile (19 x 37 against 8 x 16 and 16 x 16 blocks and 64 / 128 / 256 GEMM rows; 37 x 37
# where a 16-row block needs an interior tile as well), >= 2 blocks along the channels with a ragged last one, >= 3 stages of the
# reduction loop (per split where there are splits).  kind: conv = cp_conv2d_f32 (generic / stem / c16), wino = F(2x2) / F(2x4) through
# `wino=`, head, dcn, stem7 = cp_stem7x7_f32.  walk: sized at case time from the CU count (`_walk_shape`).
ROWS = [
    _r("igemm-64x64", "conv", "direct", IG % "64, 64, 2, 2, 32, false", cin=32, cout=100, tile=64064),
    _r("igemm-128x64", "conv", "direct", IG % "128, 64, 2, 2, 32, false", cin=32, cout=100, tile=128064),
    _r("igemm-128x128-s2", "conv", "direct", IG % "128, 128, 2, 2, 32, false", cin=32, cout=200, H=37, W=45, stride=2, tile=128128),
    _r("igemm-128x32", "conv", "direct", IG % "128, 32, 4, 1, 32, false", cin=16, cout=40, tile=128032),
    _r("igemm-256x16", "conv", "direct", IG % "256, 16, 4, 1, 16, false", cin=16, cout=24, tile=256016),
    _r("igemm-stem-256x16", "conv", "direct", IG % "256, 16, 4, 1, 16, true", cin=3, cout=24, k=5, pad=2, H=37, W=45, tile=256016, nchw=True),
    _r("igemm-stem-128x32", "conv", "direct", IG % "128, 32, 4, 1, 32, true", cin=3, cout=40, k=7, pad=3, stride=2, H=37, W=45, tile=128032, nchw=True),
    _r("igemm-stem-128x64", "conv", "direct", IG % "128, 64, 2, 2, 32, true", cin=3, cout=100, k=5, pad=2, H=37, W=45, tile=128064, nchw=True),
    # generic split-K: k-steps [s nk / S, (s + 1) nk / S) of 16; 3x3 x 32 channels = 18 steps, two per tap: S = 2 starts at step 9, S = 4 at
    # 4 / 9 / 13 (inside taps 4 and 6); 5x5 x 32 channels = 50 steps: S = 3 starts at 16 / 33 (inside tap 16).  K of `c_for` = the whole sum
    _r("igemm-split2", "conv", "direct", IG % "64, 64, 2, 2, 32, false", cin=32, cout=100, tile=64064, S=2, res=False),
    _r("igemm-split3-5x5", "conv", "direct", IG % "64, 64, 2, 2, 32, false", cin=32, cout=100, k=5, pad=2, tile=64064, S=3, res=False),
    _r("igemm-split4-128x64", "conv", "direct", IG % "128, 64, 2, 2, 32, false", cin=32, cout=100, tile=128064, S=4, res=False),
    _r("wino-1x1", "wino", "wino", "conv3x3_wino_kernel<1, 1, 16, 2>", cin=48, cout=44, tile=11),
    _r("wino-1x2", "wino", "wino", "conv3x3_wino_kernel<1, 2, 16, 2>", cin=48, cout=100, tile=12),
    _r("wino-2x1", "wino", "wino", "conv3x3_wino_kernel<2, 1, 16, 2>", cin=64, cout=44, H=37, W=37, tile=21),
    _r("wino-vs64", "wino", "wino", "conv3x3_wino_vs64_kernel<0, 0>", cin=64, cout=150, tile=6402),
    # Winograd split-C: stages [s n / S, (s + 1) n / S) of 16 channels; 7 stages in 2 = 3 + 4, 13 in 4 = 3 + 3 + 3 + 4, 25 in 8 = 7 x 3 + 4
    _r("wino-split2", "wino", "wino", "conv3x3_wino_kernel<1, 1, 16, 2>", cin=112, cout=44, tile=11, S=2, res=False),
    _r("wino-split4", "wino", "wino", "conv3x3_wino_kernel<1, 2, 16, 2>", cin=208, cout=100, tile=12, S=4, res=False),
    _r("wino-split8", "wino", "wino", "conv3x3_wino_kernel<1, 1, 16, 2>", cin=400, cout=40, tile=11, S=8, res=False),
    _r("wino24-fast", "wino", "wino24", "conv3x3_wino24_kernel<true>", cin=48, cout=44, H=37, W=37, tile=24),
    _r("wino24-scalar", "wino", "wino24", "conv3x3_wino24_kernel<false>", cin=48, cout=43, cpad=43, H=37, W=37, tile=24),
] + [
    _r("head-%s-n%d-hc%d" % (fam, n2, hc), "head", fam, (kn % _head_inst(n2)), cin=64, hc=hc, cout=n2, sigmoid=sig, wino24=fam == "wino24", res=False)
    for fam, kn in (("wino", "conv3x3_wino_vs64_kernel%s"), ("wino24", "head_wino24_kernel%s")) for n2, hc, sig in _HEADS
] + [
    _r("dcn-64x64", "dcn", "dcn", DCN % "64, 64, 2, 2, 32", cin=48, cout=100, tile=64064, res=False),
    _r("dcn-64x128", "dcn", "dcn", DCN % "64, 128, 2, 2, 32", cin=48, cout=200, tile=64128, res=False),
    _r("dcn-128x64", "dcn", "dcn", DCN % "128, 64, 2, 2, 32", cin=48, cout=100, tile=128064, res=False),
    _r("dcn-128x32", "dcn", "dcn", DCN % "128, 32, 4, 1, 32", cin=48, cout=40, tile=128032, res=False),
    _r("dcn-64x32", "dcn", "dcn", DCN % "64, 32, 4, 1, 16", cin=48, cout=40, tile=64032, res=False),
    _r("dcn-split3", "dcn", "dcn", DCN % "64, 64, 2, 2, 32", cin=48, cout=100, tile=64064, S=3, res=False),
    _r("c16-s1-16", "conv", "direct", "conv3x3_c16_kernel<1, 1, 8, 32, 4, 2>", cin=16, cout=16, tile=16, walk=True),
    _r("c16-s1-32", "conv", "direct", "conv3x3_c16_kernel<2, 1, 8, 32, 2, 2>", cin=16, cout=32, tile=16, walk=True),
    _r("c16-s2-16", "conv", "direct", "conv3x3_c16_kernel<1, 2, 8, 16, 3, 2>", cin=16, cout=16, stride=2, tile=16, walk=True),
    _r("c16-s2-32", "conv", "direct", "conv3x3_c16_kernel<2, 2, 8, 16, 3, 1>", cin=16, cout=32, stride=2, tile=16, walk=True),
    _r("stem7-c16-16-s1", "stem7", "direct", "stem7x7_c16_kernel<16, 1, 7>", cin=3, cout=16, k=7, pad=3, walk=True, res=False),
    _r("stem7-c16-64-s2", "stem7", "direct", "stem7x7_c16_kernel<64, 2, 7>", cin=3, cout=64, k=7, pad=3, stride=2, walk=True, res=False),
    _r("stem3-c16-64-s2", "conv", "direct", "stem7x7_c16_kernel<64, 2, 3>", cin=3, cout=64, stride=2, nchw=True, walk=True, res=False),
    # W % 4 != 0: the non-persistent stem (one block per 8 x 64 resp. 8 x 32 tile)
    _r("stem7-16-s1", "stem7", "direct", "stem7x7_kernel<16, 1, 8, 64>", cin=3, cout=16, k=7, pad=3, H=19, W=75, res=False),
    _r("stem7-64-s2", "stem7", "direct", "stem7x7_kernel<64, 2, 8, 32>", cin=3, cout=64, k=7, pad=3, stride=2, H=37, W=75, res=False),
    _r("stem7-64-s1", "stem7", "direct", "stem7x7_kernel<64, 1, 8, 32>", cin=3, cout=64, k=7, pad=3, H=19, W=37, res=False),
    _r("stem7-16-s2", "stem7", "direct", "stem7x7_kernel<16, 2, 8, 64>", cin=3, cout=16, k=7, pad=3, stride=2, H=37, W=150, res=False),
]
ROW = {r.id: r for r in ROWS}
assert len(ROW) == len(ROWS)

Case = collections.namedtuple("Case", "row p sd x res om Ho Wo cpad")


@functools.lru_cache(maxsize=2)
def make_case(rid, ncu=NCU_DEFAULT):
    """the row's data (CPU, float32, logical NCHW), fixed by seed"""
    row = ROW[rid]
    p = dict(row.p)
    if p.get("walk"):
        p["H"], p["W"] = _walk_shape(row.kernel, ncu, p["stride"], p["B"], quad=p["cin"] == 3)
    g = torch.Generator().manual_seed(1000 + ROWS.index(row))
    r = lambda *s: torch.randn(*s, generator=g)
    u01 = lambda n: torch.rand(n, generator=g)
    B, H, W, ci, co, k = p["B"], p["H"], p["W"], p["cin"], p["cout"], p["k"]
    x = F.relu(r(B, ci, H, W))
    Ho, Wo = (H + 2 * p["pad"] - k) // p["stride"] + 1, (W + 2 * p["pad"] - k) // p["stride"] + 1
    bn = lambda n: {"b.weight": u01(n) + 0.5, "b.bias": r(n) * 0.1, "b.running_mean": r(n) * 0.1, "b.running_var": u01(n) + 0.5}
    om = None
    if row.kind == "head":
        hc = p["hc"]
        sd = {"h.0.weight": r(hc, ci, 3, 3) * (2.0 / (9 * ci)) ** 0.5 * lo.spread_factors(hc).view(-1, 1, 1, 1), "h.0.bias": r(hc) * 0.1,
              "h.2.weight": r(co, hc, 1, 1) * (2.0 / hc) ** 0.5 * lo.spread_factors(co).view(-1, 1, 1, 1),
              "h.2.bias": torch.full((co,), SIGMOID_BIAS) if p["sigmoid"] else r(co) * 0.1}
    elif row.kind == "dcn":
        sd = dict(bn(co), **{"d.weight": r(co, ci, 3, 3) * (4.0 / (9 * ci)) ** 0.5, "d.bias": r(co) * 0.1})
        om = torch.cat([r(B, 18, H, W) * 2.5, r(B, 9, H, W) * 1.5], 1)      # offsets of a few pixels, mask logits mostly inside +-4.6
        sd = lo.spread_bn(sd)
    else:
        sd = lo.spread_bn(dict(bn(co), **{"c.weight": r(co, ci, k, k) * (2.0 / (k * k * ci)) ** 0.5}))
    res = F.relu(r(B, co, Ho, Wo)) if p["res"] else None
    return Case(row, p, sd, x, res, om, Ho, Wo, p.get("cpad", co if row.kind == "head" else -(-co // 16) * 16))


def evaluate(case, dt, wino=None):
    """the row's operation in plain torch, dtype `dt` -> lo.Out (A with float64).  wino: None = direct, "wino" / "wino24" = the textbook
    transform (float32 yardstick of the Winograd families)"""
    p, sd = case.p, case.sd
    x = case.x.to(dt)
    if case.row.kind == "head":
        return lo.head_branch(sd, x, "h.0", "h.2", p["hc"], p["cout"], "sigmoid" if p["sigmoid"] else None, dt, wino)
    if case.row.kind == "dcn":
        return lo.dcn_stage(sd, x, case.om, "d", "b", p["cout"], dt)
    return lo._conv_bn(sd, x, "c", "b", False, p["cout"], p["k"], p["stride"], p["pad"], p["relu"], case.res.to(dt) if case.res is not None else None,
                       dt, wino)


def yardstick_family(row):
    return row.family if row.family in ("wino", "wino24") else None


def live_fractions(case, val):
    """{key of lo.LIVE_FLOOR: fraction} of the row's own data (DCN and sigmoid rows)"""
    if case.row.kind == "dcn":
        return dict(zip(("dcn_samples", "dcn_masks"), lo.dcn_liveness(case.om)))
    if case.row.kind == "head" and case.p["sigmoid"]:
        return {"sigmoid": lo.sigmoid_liveness(val)}
    return {}


def check(case, out, o32, o64):
    """judge a stand-in or device result `out` (logical NCHW float32) -> (Worst or None, [failure text]); liveness floors included"""
    w, fail = lo.judge(out, o32, o64, case.row.family)
    fails = [fail] if fail else []
    for key, frac in live_fractions(case, out).items():
        if frac < lo.LIVE_FLOOR[key]:
            fails.append("degenerate test data: %s = %.3f < %.2f" % (key, frac, lo.LIVE_FLOOR[key]))
    return w, fails


# ---- device ------------------------------------------------------------------------------------------------------------------------
def _nhwc(t, c=None, ld=None):
    """logical NCHW CPU tensor -> device NHWC [B, H, W, c] (c >= C: zero padding channels), a view of a zero buffer with `ld` floats
    per pixel"""
    B, C, H, W = t.shape
    c = c or C
    buf = torch.zeros(B, H, W, ld or c, device="cuda")
    buf[..., :C] = t.permute(0, 2, 3, 1).cuda()
    return buf[..., :c]


def _guarded(B, H, W, c):
    """NaN-filled NHWC buffer wider than the `c` channels the launch is given, and the view the launch writes"""
    buf = torch.full((B, H, W, -(-c // 4) * 4 + 4), float("nan"), device="cuda")
    return buf, buf[..., :c]


def build_launches(case):
    """-> (launches in order, read() -> (physical NHWC [..., :cpad] or None, logical NCHW result, guard intact) after a run)"""
    from centerpose_amd import ops
    row, p, sd = case.row, case.p, case.sd
    B, H, W, co, cp, Ho, Wo, S = p["B"], p["H"], p["W"], p["cout"], case.cpad, case.Ho, case.Wo, p["S"]
    dev = lambda t: t.cuda()
    relu = ops.ACT_RELU if p["relu"] else ops.ACT_NONE
    if row.kind == "head":
        hc, G = p["hc"], 64
        n = B * co * H * W
        flat = torch.full((n + 2 * G,), float("nan"), device="cuda")
        out = flat[G:G + n].view(B, co, H, W)
        wp3 = ops.pack_conv_weight(dev(sd["h.0.weight"]))
        u = (ops.pack_wino24_weight if p["wino24"] else ops.pack_wino_weight)(wp3, 64, hc)
        sc, sh = ops.fold_bn(hc, None, dev(sd["h.0.bias"]))
        la = ops.head3x3_1x1_launch(_nhwc(case.x), u, sc, sh, dev(sd["h.2.weight"].reshape(co, hc).contiguous()), dev(sd["h.2.bias"]), out, hc=hc,
                                    act2=ops.ACT_SIGMOID if p["sigmoid"] else ops.ACT_NONE, wino24=p["wino24"])
        return [la], lambda: (None, out.cpu(), bool(torch.isnan(flat[:G]).all() and torch.isnan(flat[G + n:]).all()))
    bnp = tuple(dev(sd["b." + s]) for s in ("weight", "bias", "running_mean", "running_var"))
    buf, out = _guarded(B, Ho, Wo, cp)
    read = lambda: (out.cpu(), out[..., :co].permute(0, 3, 1, 2).contiguous().cpu(), bool(torch.isnan(buf[..., cp:]).all()))
    if row.kind == "stem7":
        sc, sh = ops.fold_bn(co, bnp)
        return [ops.stem7x7_launch(dev(case.x), ops.pack_stem7_weight(dev(sd["c.weight"])), sc, sh, out, p["stride"], relu=p["relu"])], read
    if row.kind == "dcn":
        wp = ops.pack_conv_weight(dev(sd["d.weight"]))
        sc, sh = ops.fold_bn(co, bnp, dev(sd["d.bias"]))
        xs, oms = _nhwc(case.x), _nhwc(case.om, 32)                           # 27 logits in 32 physical channels
        if S == 1:
            return [ops.dcn_v2_launch(xs, oms, wp, sc, sh, out, cout=cp, om_sigmoid=True, act=relu, tile=p["tile"])], read
        ldw = wp.shape[0]
        ws = torch.full((S, B * Ho * Wo, ldw), float("nan"), device="cuda")
        la = ops.dcn_v2_launch(xs, oms, wp, torch.ones(ldw, device="cuda"), torch.zeros(ldw, device="cuda"), ws, cout=ldw, om_sigmoid=True,
                               tile=p["tile"], ksplit=S)
        return [la, ops.splitk_reduce_launch(ws, sc, sh, out, cout=cp, act=relu)], read
    nchw = p.get("nchw", False)
    wp = ops.pack_conv_weight(dev(sd["c.weight"]), stem=nchw)
    sc, sh = ops.fold_bn(co, bnp)
    srcs = [dev(case.x)] if nchw else [_nhwc(case.x)]
    res = _nhwc(case.res, cp, -(-cp // 4) * 4 + 4) if case.res is not None else None      # its padding channels are zeros
    kw = dict(kh=p["k"], kw=p["k"], stride=p["stride"], pad=p["pad"], tile=p["tile"], in_nchw=nchw)
    u = None
    if row.kind == "wino":
        u = (ops.pack_wino24_weight if row.family == "wino24" else ops.pack_wino_weight)(wp, p["cin"], cp)
    # split_bf16=False: these rows name the f32 kernels whatever CP_SPLIT_BF16 says; igemm_bf16x3_kernel has rows of its own
    # (tests/bf16x3_oracle.py: all four instantiations forced, per element and with exact-answer cases)
    if S == 1:
        return [ops.conv2d_launch(srcs, wp, sc, sh, out, cout=cp, act=relu, res=res, wino=u, split_bf16=False, **kw)], read
    ld = cp if u is not None else wp.shape[0]                                      # the generic kernel stores whole N tiles of raw sums
    ws = torch.full((S, B * Ho * Wo, ld), float("nan"), device="cuda")
    n = sc.numel()
    la = ops.conv2d_launch(srcs, wp, torch.ones(n, device="cuda"), torch.zeros(n, device="cuda"), ws, cout=ld, wino=u, ksplit=S, split_bf16=False, **kw)
    return [la, ops.splitk_reduce_launch(ws, sc, sh, out, cout=cp, act=relu)], read


def run_row(rid, device_index=0):
    """Build the row for this device's CU count, run it twice and judge it.  -> dict(kernels [str], worst (lo.Worst or None), c,
    failures [text], walk (ntiles, floor) or None)"""
    ncu = torch.cuda.get_device_properties(device_index).multi_processor_count
    case = make_case(rid, ncu)
    row = case.row
    with torch.no_grad():
        launches, read = build_launches(case)
        for l in launches:
            l.run()
        torch.cuda.synchronize()
        phys, first, guard = read()
        for l in launches:
            l.run()
        torch.cuda.synchronize()
        phys2, second, guard2 = read()
        o64 = evaluate(case, torch.float64)
        w, fails = check(case, first, None, o64)
    if not (guard and guard2):
        fails.append("stored past the %d channels the launch was given (NaN guard overwritten)" % case.cpad)
    if not torch.equal(first, second) or (phys is not None and not torch.equal(phys, phys2)):
        fails.append("a second run gives other bits at %s" % (lo.first_unequal(first, second),))
    if phys is not None:
        loc = lo.padding_violation(phys, lo.View(case.Ho, case.Wo, case.p["cout"], None, None))
        if loc is not None:
            fails.append("padding channel not zero at (b, y, x, c) = %s: %r" % (loc, float(phys[loc])))
    walk = (walk_tiles(row.kernel, case.p["B"], case.Ho, case.Wo), walk_floor(row.kernel, ncu)) if case.p.get("walk") else None
    return dict(kernels=[l.kernel for l in launches], worst=w, c=lo.c_for(row.family, o64.K), failures=fails, walk=walk)
