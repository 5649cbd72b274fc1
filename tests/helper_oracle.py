"""TEST INFRASTRUCTURE ONLY -- per-element oracle of the bandwidth-bound helpers of csrc/elementwise.hip, one stand-alone launch per
row of ``ROWS``, in every launch-geometry regime (same role as tests/launch_oracle.py for the MFMA kernels).

The helpers' launch geometry changes with size exactly as the GEMM kernels' does, only along other axes.  It is restated here once
(``row_geometry``, ``flat_geometry``, ``magic`` / ``split``), from the launchers' own statements:

* row-major launchers (``EwRow`` / ``ew_row_grid`` / ``ew_split``): blockIdx.x walks 256-element segments of one row of Wo * C/4 float4s,
  blockIdx.y walks min(rows, 65535) rows with a stride loop above that, e / C4 is a multiply-high by ceil(2^32 / C4), and the launcher
  refuses Wo * C4 * C4 >= 2^32;
* flat launchers (``ew_grid``): clamp(ceil(n / 256), 1, 8192) blocks and a grid-stride loop above 2 097 152 elements;
* ``global_avgpool_kernel``: 32 channel quads per block, eight strided pixel partitions summed through LDS;
* the two layout transposes: 32 x 32 tiles.

Regimes a row can be in (``Row.regimes``; tests/test_helper_oracle_cpu.py checks every claim against the restated geometry):

  XN    >= 3 x-blocks with a ragged last one, C4 no power of two          B = 2, W(o) = 37, C = 72 / 240, odd H
  YS    65535 < rows: some grid rows take the row loop twice (or three times); C = 4 is the C4 == 1 branch of ew_split
  LIM   the last shape the launcher accepts: C = 17476 (C4 = 4369 = 17 * 257, 2^32 mod C4 = 1), checked width 225 -- the multiply-high
        is exact for every e < 225 * 4369 and wrong at e = 987393, which the width 226 would reach
  VIEW  every operand a channel slice of a wider buffer (ld = C + 16); the deconvolutions' addend IS the output (in place)
  FLAT  n > 2 * 8192 * 256, no multiple of 8192 * 256: some threads run three iterations, the others two
  (``fill`` adds N0 / N1: nothing to do / one element; ``dcn_pack`` PAD: padded groups and rows; avgpool HW*; the transposes TILE)

Data is built on the CPU from a fixed seed.  Every device input is a view into a larger buffer whose rest is poison -- channels
beyond C and one guard image before and after -- so that a read outside the view shows in the output: NaN everywhere except for the
max-pool, whose fmaxf would swallow it: +inf there.  Outputs are NaN-filled, wider than C and guarded the same way: nothing may be
stored outside the view.

References are plain torch on the CPU, taken from ``layer_oracle`` where it states the operation (``_sum_up``, the bodies of
``evaluate``), written in the same style otherwise.  Nothing here reads device results or kernel sources to set a bound: a row is
either bit-equal to the float32 evaluation or inside ``layer_oracle.c_for("direct", K) u A``.
"""
import collections
import functools
import os

import torch
import torch.nn.functional as F

import layer_oracle as lo

# ---- the launchers' geometry, as they state it --------------------------------------------------------------------------------------
EW_THREADS, Y_MAX, FLAT_MAX = 256, 65535, 8192
FLAT_SPAN = FLAT_MAX * EW_THREADS                        # elements one pass of a full flat grid covers
LIM_C, LIM_W = 17476, 225                                # C4 = 4369: 225 * 4369^2 < 2^32 <= 226 * 4369^2


def cdiv(a, b):
    return -(-a // b)


def row_geometry(rows, Wo, C4):
    """ew_row + ew_row_grid: dict(rowElems, xblocks, tail (elements of the last x-block), ygrid, passes (most trips of the row loop),
    multi (grid rows that take the most trips))"""
    re_ = Wo * C4
    xb, yg = cdiv(re_, EW_THREADS), min(rows, Y_MAX)
    passes = cdiv(rows, yg)
    return dict(rowElems=re_, xblocks=xb, tail=re_ - (xb - 1) * EW_THREADS, ygrid=yg, passes=passes, multi=rows - (passes - 1) * yg)


def flat_geometry(n):
    """ew_grid: dict(grid, span (elements per pass), most / fewest trips of a thread's grid-stride loop)"""
    grid = max(1, min(FLAT_MAX, cdiv(n, EW_THREADS)))
    span = grid * EW_THREADS
    return dict(grid=grid, span=span, most=cdiv(n, span), fewest=n // span)


def magic(C4):
    """ew_row's mC4"""
    return 0 if C4 <= 1 else ((1 << 32) + C4 - 1) // C4


def split(e, C4):
    """ew_split in 64-bit integers: (x, c4) as the kernel computes them (e: int or int64 tensor)"""
    x = e if C4 == 1 else (e * magic(C4)) >> 32
    return x, e - x * C4


def accepts(width, C4):
    """the launchers' "row too large" check for the width they check"""
    return width * C4 * C4 < (1 << 32)


def first_wrong_split(Wo, C4):
    """the first e < Wo * C4 at which the multiply-high differs from e // C4, or None"""
    e = torch.arange(Wo * C4, dtype=torch.int64)
    bad = split(e, C4)[0] != e // C4
    return int(torch.argmax(bad.to(torch.uint8))) if bool(bad.any()) else None


# ---- the table ----------------------------------------------------------------------------------------------------------------------
Row = collections.namedtuple("Row", "id launcher regimes kernel p")
ACTS = (None, "relu", "sigmoid", "hswish", "hsigmoid")                   # index = the library's ACT_* code
GENERIC, DECONV2 = "dw_deconv_add_kernel", "dw_deconv2_add_kernel"


def _r(id, launcher, regimes, kernel=None, **p):
    d = dict(B=2, H=11, W=37, C=72, pad=4)
    d.update(p)
    if "VIEW" in regimes.split():
        d["pad"] = 16
    return Row(id, launcher, tuple(regimes.split()), kernel, d)


_XN = dict(B=2, H=8, W=40, C=72)                                          # sum_up: maps every shift 0..3 divides; 40 * 18 = 720 = 2 * 256 + 208
_YS = dict(B=2, H=32772, W=4, C=4)
_LIM = dict(B=1, H=1, W=LIM_W, C=LIM_C)
_SMALL = dict(B=2, H=4, W=4, C=8)
ROWS = [
    # max-pool: the last window of (3, 2, 1) is cut by the border in y (H = 11) and x (W = 73); (2, 2, 0) drops the odd last row
    _r("maxpool-2x2-XN", "maxpool", "XN VIEW", "maxpool_nhwc_kernel", W=74, k=2, s=2, p=0),
    _r("maxpool-3x3-XN", "maxpool", "XN VIEW", "maxpool_nhwc_kernel", W=73, C=240, k=3, s=2, p=1),
    _r("maxpool-YS", "maxpool", "YS", "maxpool_nhwc_kernel", H=65540, W=6, C=4, k=2, s=2, p=0),
    _r("maxpool-LIM", "maxpool", "LIM", "maxpool_nhwc_kernel", B=1, H=1, W=449, C=LIM_C, k=3, s=2, p=1),
    # depthwise bilinear deconvolution + add.  `env`: CP_DWDECONV2; `twin`: the row that must give the same bits on the other kernel.
    # The launcher checks W * f whichever kernel runs, so f = 2 ends at W = 112 on both; the generic kernel reaches 225 with f = 1.
    _r("deconv2-XN-inplace", "dw_deconv2", "XN VIEW", DECONV2, f=2, add="inplace", env="1", seed=101),
    _r("deconv-f2-XN-inplace", "dw_deconv", "XN VIEW", GENERIC, f=2, add="inplace", env="0", seed=101, twin="deconv2-XN-inplace"),
    _r("deconv2-XN-noadd", "dw_deconv2", "XN VIEW", DECONV2, C=240, f=2, add=None, env="1", seed=102),
    _r("deconv-f2-XN-noadd", "dw_deconv", "XN VIEW", GENERIC, C=240, f=2, add=None, env="0", seed=102, twin="deconv2-XN-noadd"),
    _r("deconv-f4-XN-noadd", "dw_deconv", "XN VIEW", GENERIC, H=3, C=240, f=4, add=None),
    _r("deconv-f4-XN-inplace", "dw_deconv", "XN VIEW", GENERIC, H=3, f=4, add="inplace"),
    _r("deconv-f8-XN-add", "dw_deconv", "XN VIEW", GENERIC, H=3, W=5, f=8, add="own"),
    _r("deconv2-YS", "dw_deconv2", "YS", DECONV2, H=32770, W=3, C=4, f=2, add="own", env="1", seed=103),
    _r("deconv-f2-YS", "dw_deconv", "YS", GENERIC, H=32770, W=3, C=4, f=2, add="own", env="0", seed=103, twin="deconv2-YS"),
    _r("deconv-f4-YS", "dw_deconv", "YS", GENERIC, H=8193, W=2, C=4, f=4, add=None),
    _r("deconv2-LIM", "dw_deconv2", "LIM", DECONV2, B=1, H=1, W=112, C=LIM_C, f=2, add=None, env="1", seed=104),
    _r("deconv-f2-LIM", "dw_deconv", "LIM", GENERIC, B=1, H=1, W=112, C=LIM_C, f=2, add=None, env="0", seed=104, twin="deconv2-LIM"),
    _r("deconv-f1-LIM", "dw_deconv", "LIM", GENERIC, B=1, H=2, W=LIM_W, C=LIM_C, f=1, add="inplace"),
    # nearest up-sampling sums: 1..4 sources, shifts 0..3 in an order that is not sorted
    _r("sum_up-1-XN", "sum_up", "XN VIEW", "sum_up_kernel", shifts=(0,), relu=True),
    _r("sum_up-2-XN", "sum_up", "XN VIEW", "sum_up_kernel", H=8, W=24, C=240, shifts=(1, 0), relu=True),
    _r("sum_up-3-XN", "sum_up", "XN VIEW", "sum_up_kernel", shifts=(0, 2, 1), relu=False, **dict(_XN, C=72)),
    _r("sum_up-4-XN", "sum_up", "XN VIEW", "sum_up_kernel", shifts=(3, 0, 1, 2), relu=True, **_XN),
    _r("sum_up-YS", "sum_up", "YS", "sum_up_kernel", shifts=(0, 2), relu=True, **_YS),
    _r("sum_up-LIM", "sum_up", "LIM", "sum_up_kernel", shifts=(0, 0), relu=True, **_LIM),
    # the grouped sum: members with different xblocks in one launch (no row loop: the first[] arithmetic places every block)
    _r("sum_up_group-2", "sum_up_group", "XN VIEW", "sum_up_group_kernel", relu=True,
       members=(dict(_XN, H=8, W=24, C=240, shifts=(1, 0)), dict(_SMALL, shifts=(0,)))),
    _r("sum_up_group-3", "sum_up_group", "XN YS VIEW", "sum_up_group_kernel", relu=False,
       members=(dict(_SMALL, shifts=(1, 0)), dict(_YS, shifts=(0, 2)), dict(_XN, shifts=(0, 2, 1)))),
    _r("sum_up_group-4", "sum_up_group", "XN YS LIM", "sum_up_group_kernel", relu=True,
       members=(dict(_XN, shifts=(3, 0, 1, 2)), dict(_YS, shifts=(2, 0)), dict(_LIM, shifts=(0, 0)), dict(_SMALL, shifts=(0, 1, 2)))),
] + [
    _r("dwconv-3x3s1-%s-XN" % (a or "none"), "dwconv", "XN VIEW", "dwconv_nhwc_kernel", k=3, s=1, act=a) for a in ACTS
] + [
    _r("dwconv-5x5s2-%s-XN" % (a or "none"), "dwconv", "XN VIEW", "dwconv_nhwc_kernel", W=73, C=240, k=5, s=2, act=a) for a in ACTS
] + [
    _r("dwconv-YS", "dwconv", "YS", "dwconv_nhwc_kernel", H=32770, W=3, C=4, k=3, s=1, act="relu"),
    _r("dwconv-LIM", "dwconv", "LIM", "dwconv_nhwc_kernel", k=3, s=1, act="hswish", **_LIM),
    _r("scale_add-XN-add", "scale_add", "XN VIEW", "scale_add_kernel", add=True),
    _r("scale_add-XN-noadd", "scale_add", "XN VIEW", "scale_add_kernel", C=240, add=False),
    _r("scale_add-YS", "scale_add", "YS", "scale_add_kernel", H=32770, W=3, C=4, add=True),
    _r("scale_add-LIM", "scale_add", "LIM", "scale_add_kernel", add=True, **_LIM),
    # flat launchers
    _r("shuffle-116", "shuffle_concat", "FLAT", "shuffle_concat_kernel", B=1, H=129, W=128, h=116, hp=128),
    _r("shuffle-29", "shuffle_concat", "FLAT", "shuffle_concat_kernel", B=1, H=65537, W=1, h=29, hp=32),     # 65537 pixels x 64: the fewest
    _r("flip_merge-m0", "flip_merge", "FLAT", mode=0, C=2, W=1449),
    _r("flip_merge-m1", "flip_merge", "FLAT", mode=1, C=17, W=499),
    _r("flip_merge-m2", "flip_merge", "FLAT", mode=2, C=34, W=353),
    _r("fill-0", "fill", "N0", n=0),
    _r("fill-1", "fill", "N1", n=1),
    _r("fill-big", "fill", "FLAT", n=2 * FLAT_SPAN + 1),
    _r("dcn_pack-dg1", "dcn_pack", "PAD SPAN", Co=1130, C=200, dg=1, Cp=208, ldw=1152),          # 1152 * 9 * 208 = 2 156 544 > 2 097 152
    _r("dcn_pack-dg2", "dcn_pack", "PAD", Co=24, C=40, dg=2, Cp=64, ldw=32),
    _r("dcn_pack-dg4", "dcn_pack", "PAD", Co=50, C=72, dg=4, Cp=128, ldw=64),
] + [
    _r("avgpool-%d" % hw, "global_avgpool", "HW%d" % hw, "global_avgpool_kernel", B=3, H=hw, W=1, C=240) for hw in (1, 3, 13, 67, 1000, 4099)
] + [
    _r("nchw_to_nhwc", "nchw_to_nhwc", "TILE", B=3, C=33, H=35, W=37, cOff=16, ld=64),
    _r("nhwc_to_nchw", "nhwc_to_nchw", "TILE", B=3, C=33, H=35, W=37, cOff=16, ld=64),
]
ROW = {r.id: r for r in ROWS}
assert len(ROW) == len(ROWS)

ROW_MAJOR = ("maxpool", "dw_deconv", "dw_deconv2", "sum_up", "dwconv", "scale_add")
# every (launcher, regime) pair that must have a row that ran
MUST_COVER = tuple((l, g) for l in ROW_MAJOR for g in ("XN", "YS", "LIM", "VIEW")) + \
    tuple(("sum_up_group", g) for g in ("XN", "YS", "LIM")) + \
    tuple((l, "FLAT") for l in ("shuffle_concat", "flip_merge", "fill")) + (("fill", "N0"), ("fill", "N1"), ("dcn_pack", "PAD"), ("dcn_pack", "SPAN")) + \
    tuple(("global_avgpool", "HW%d" % hw) for hw in (1, 3, 13, 67, 1000, 4099)) + (("nchw_to_nhwc", "TILE"), ("nhwc_to_nchw", "TILE"))


def flip_height(C, W):
    """the smallest H at which C * H * W reaches the three-iteration regime"""
    return 2 * FLAT_SPAN // (C * W) + 1


def out_hw(row, p=None):
    """(Ho, Wo) of the row's output map"""
    p = p or row.p
    if row.launcher == "maxpool":
        return (p["H"] + 2 * p["p"] - p["k"]) // p["s"] + 1, (p["W"] + 2 * p["p"] - p["k"]) // p["s"] + 1
    if row.launcher == "dwconv":
        return (p["H"] + 2 * (p["k"] // 2) - p["k"]) // p["s"] + 1, (p["W"] + 2 * (p["k"] // 2) - p["k"]) // p["s"] + 1
    if row.launcher in ("dw_deconv", "dw_deconv2"):
        return p["H"] * p["f"], p["W"] * p["f"]
    return p["H"], p["W"]


def launch_rows(row, p=None):
    """[(rows, width the grid walks, width the launcher checks, C4)] of a row-major row, one entry per member for the group"""
    p = p or row.p
    if row.launcher == "sum_up_group":
        return [(m["B"] * m["H"], m["W"], m["W"], m["C"] // 4) for m in p["members"]]
    Ho, Wo = out_hw(row, p)
    if row.launcher == "dw_deconv2":                    # one thread per INPUT pixel column; the launcher still checks W * f
        return [(p["B"] * p["H"], p["W"], Wo, p["C"] // 4)]
    return [(p["B"] * Ho, Wo, Wo, p["C"] // 4)]


def next_checked_width(row, p=None):
    """the width the launcher would check with one more pixel in the row"""
    p = p or row.p
    if row.launcher in ("dw_deconv", "dw_deconv2"):
        return (p["W"] + 1) * p["f"]
    return out_hw(row, p)[1] + 1


def flat_count(row):
    """elements a flat launcher walks"""
    p = row.p
    if row.launcher == "shuffle_concat":
        return p["B"] * p["H"] * p["W"] * 2 * p["hp"]
    if row.launcher == "flip_merge":
        return p["C"] * flip_height(p["C"], p["W"]) * p["W"]
    if row.launcher == "fill":
        return p["n"]
    assert row.launcher == "dcn_pack"
    return p["ldw"] * 9 * p["Cp"]


# ---- data ----------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "row p t")       # t: dict of CPU float32 tensors (logical NCHW maps)


def _perm(J):
    """a left / right joint permutation: 0 stays, (1, 2), (3, 4), ... swap"""
    return torch.tensor([0] + [j + 1 if j % 2 else j - 1 for j in range(1, J)], dtype=torch.int32) if J > 1 else torch.zeros(1, dtype=torch.int32)


@functools.lru_cache(maxsize=2)
def make_case(rid):
    row = ROW[rid]
    p = dict(row.p)
    g = torch.Generator().manual_seed(p.get("seed", 5000 + ROWS.index(row)))
    r = lambda *s: torch.randn(*s, generator=g)
    B, H, W, C = p["B"], p["H"], p["W"], p["C"]
    t = {}
    kind = row.launcher
    if kind == "maxpool":
        t["x"] = r(B, C, H, W)
    elif kind in ("dw_deconv", "dw_deconv2"):
        f = p["f"]
        t["x"], t["w"] = r(B, C, H, W), r(C, 1, 2 * f, 2 * f) * 0.5
        if p["add"]:
            t["add"] = r(B, C, H * f, W * f)
    elif kind == "sum_up":
        t["xs"] = [r(B, C, H >> s, W >> s) for s in p["shifts"]]
    elif kind == "sum_up_group":
        t["xs"] = [[r(m["B"], m["C"], m["H"] >> s, m["W"] >> s) for s in m["shifts"]] for m in p["members"]]
    elif kind == "dwconv":
        k = p["k"]
        t["x"], t["w"] = r(B, C, H, W), r(C, 1, k, k) * (2.0 / (k * k)) ** 0.5
        t["scale"], t["shift"] = (torch.rand(C, generator=g) + 0.5) * lo.spread_factors(C), r(C) * 0.5
    elif kind == "scale_add":
        t["x"], t["se"] = r(B, C, H, W), torch.rand(B, C, 1, 1, generator=g)
        if p["add"]:
            t["add"] = r(B, C, H, W)
    elif kind == "shuffle_concat":
        t["x1"], t["x2"] = r(B, p["h"], H, W), r(B, p["h"], H, W)
    elif kind == "flip_merge":
        p["H"] = H = flip_height(C, W)
        t["x"] = r(2, C, H, W)
        t["perm"] = _perm(C if p["mode"] == 1 else C // 2 if p["mode"] == 2 else 1)
    elif kind == "dcn_pack":
        t["w"], t["bias"] = r(p["Co"], C, 3, 3), r(p["Co"])
    elif kind == "global_avgpool":
        t["x"] = r(B, C, H, W) + 0.25
    elif kind in ("nchw_to_nhwc", "nhwc_to_nchw"):
        t["x"] = r(B, C, H, W)
    else:
        assert kind == "fill", kind
    return Case(row, p, t)


# ---- plain-torch references ------------------------------------------------------------------------------------------------------------
def avgpool_partitions(x, drop=None):
    """the stated reduction of global_avgpool_kernel in x.dtype: partition pp sums the pixels pp, pp + 8, ... in order, the eight partial
    sums are added in order, then one division.  x [B, C, HW] -> [B, C].  drop = (partition, trip): that one pixel is left out."""
    B, C, HW = x.shape
    acc = torch.zeros(B, C, 8, dtype=x.dtype)
    for i in range(cdiv(HW, 8)):
        chunk = x[:, :, 8 * i:8 * i + 8]
        if drop is not None and drop[1] == i:
            chunk = chunk.clone()
            chunk[:, :, drop[0]] = 0
        acc[:, :, :chunk.shape[2]] += chunk
    tot = acc[:, :, 0].clone()
    for j in range(1, 8):
        tot = tot + acc[:, :, j]
    return tot / torch.tensor(float(HW), dtype=x.dtype)


def dcn_pack_reference(w, bias, dg, Cp, ldw):
    """cp_dcn_pack_weights_f32: w [Co, C, kh, kw] -> wp [ldw, kk * Cp] with k = (tap * dg + g) * cpgp + c, zero rows / columns for the
    padding; scale = 1 / shift = bias below Co, 0 above"""
    Co, C, kh, kw = w.shape
    kk, cpg, cpgp = kh * kw, C // dg, Cp // dg
    wp = torch.zeros(ldw, kk, dg, cpgp, dtype=w.dtype)
    wp[:Co, :, :, :cpg] = w.reshape(Co, dg, cpg, kk).permute(0, 3, 1, 2)
    scale, shift = torch.zeros(ldw, dtype=w.dtype), torch.zeros(ldw, dtype=w.dtype)
    scale[:Co], shift[:Co] = 1.0, bias
    return wp.reshape(ldw, kk * Cp), scale, shift


def flip_merge_reference(x, mode, perm):
    """cp_flip_merge_f32: (x[0] + sign * flip_w(x[1][cs])) / 2 -- one rounding"""
    C = x.shape[1]
    c = torch.arange(C)
    cs, sign = c, torch.ones(C, dtype=x.dtype)
    if mode == 1:
        cs = perm.long()[c]
    elif mode == 2:
        cs = 2 * perm.long()[c // 2] + (c % 2)
        sign[0::2] = -1.0
    return ((x[0] + x[1][cs].flip(-1) * sign.view(-1, 1, 1)) / 2).unsqueeze(0)


def _exact(v):
    return lo.Out(v, exact=True)


def evaluate(case, dt):
    """the row's operation in plain torch, dtype `dt` -> [lo.Out], one per output of the launch (A with float64 where the row is judged
    by a bound; exact rows are evaluated in float32 and ignore `dt`)"""
    row, p, t = case.row, case.p, case.t
    kind = row.launcher
    if kind == "maxpool":
        return [_exact(F.max_pool2d(t["x"], p["k"], p["s"], p["p"]))]
    if kind in ("dw_deconv", "dw_deconv2"):              # layer_oracle's emit_up_add, cropped to H f x W f (f = 1: k = 2, p = 0 gives one more)
        f, C, Ho, Wo = p["f"], p["C"], p["H"] * p["f"], p["W"] * p["f"]
        xv, w = t["x"].to(dt), t["w"].to(dt)
        ct = lambda a, ww: F.conv_transpose2d(a, ww, None, stride=f, padding=f // 2, groups=C)[:, :, :Ho, :Wo]
        v, A = ct(xv, w), ct(xv.abs(), w.abs()) if dt == torch.float64 else None
        if p["add"]:
            av = t["add"].to(dt)
            v, A = v + av, None if A is None else A + av.abs()
        return [lo.Out(v, A, 5)]
    if kind == "sum_up":                                  # only additions, in a fixed order: nothing can contract
        return [_exact(lo._sum_up(t["xs"], p["shifts"], p["relu"]).val)]
    if kind == "sum_up_group":
        return [_exact(lo._sum_up(xs, m["shifts"], p["relu"]).val) for xs, m in zip(t["xs"], p["members"])]
    if kind == "dwconv":
        v = lambda a: a.to(dt).view(1, -1, 1, 1)
        xv = t["x"].to(dt)
        return [lo._affine(xv, xv.abs(), t["w"], v(t["scale"]), v(t["shift"]), v(t["shift"]).abs(), None, p["act"], p["s"], p["k"] // 2, groups=p["C"])]
    if kind == "scale_add":                               # two roundings, as layer_oracle's emit_scale_add
        v = t["x"] * t["se"]
        return [_exact(v + t["add"] if p["add"] else v)]
    if kind == "shuffle_concat":
        c = torch.cat([t["x1"], t["x2"]], 1)
        b, ch, h, w = c.shape
        return [_exact(c.view(b, 2, ch // 2, h, w).transpose(1, 2).reshape(b, ch, h, w))]
    if kind == "flip_merge":
        return [_exact(flip_merge_reference(t["x"], p["mode"], t["perm"]))]
    if kind == "fill":
        return [_exact(torch.full((p["n"],), FILL_VALUE))]
    if kind == "dcn_pack":
        return [_exact(o) for o in dcn_pack_reference(t["w"], t["bias"], p["dg"], p["Cp"], p["ldw"])]
    if kind == "global_avgpool":
        x = t["x"].to(dt).flatten(2)
        hw = x.shape[2]
        if dt == torch.float64:
            return [lo.Out(x.mean(2)[..., None, None], x.abs().mean(2)[..., None, None], cdiv(hw, 8) + 8)]
        return [lo.Out(avgpool_partitions(x)[..., None, None], None, cdiv(hw, 8) + 8)]
    assert kind in ("nchw_to_nhwc", "nhwc_to_nchw"), kind
    return [_exact(t["x"])]


FILL_VALUE = 1.25
FAMILY = "direct"


def is_exact(row):
    return row.launcher not in ("dw_deconv", "dw_deconv2", "dwconv", "global_avgpool")


def references(case):
    """(o32, o64) lists for `lo.judge`: exact rows need the float32 evaluation alone"""
    if is_exact(case.row):
        o = evaluate(case, torch.float32)
        return o, o
    return evaluate(case, torch.float32), evaluate(case, torch.float64)


def judge(case, outs, o32, o64):
    """-> (worst lo.Worst over the outputs or None, [failure text])"""
    worst, fails = None, []
    for j, (out, a, b) in enumerate(zip(outs, o32, o64)):
        if out.shape != b.val.shape:
            fails.append("output %d: shape %s != %s" % (j, tuple(out.shape), tuple(b.val.shape)))
            continue
        if out.numel() == 0:
            continue
        w, fail = lo.judge(out, a, b, FAMILY)
        if w is not None and (worst is None or w.ratio > worst.ratio):
            worst = w
        if fail:
            fails.append("output %d: %s" % (j, fail))
    return worst, fails


def bound(case, o64):
    return None if is_exact(case.row) else lo.c_for(FAMILY, o64[0].K)


# ---- device ----------------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")


def _in_view(t, pad, poison=NAN):
    """logical NCHW CPU tensor -> device NHWC view [B, H, W, C] into a poison buffer [B + 2, H, W, C + pad]"""
    B, C, H, W = t.shape
    buf = torch.full((B + 2, H, W, C + pad), poison, device="cuda")
    buf[1:B + 1, ..., :C] = t.permute(0, 2, 3, 1).cuda()
    return buf[1:B + 1, ..., :C]


class _OutView:
    """NaN-filled device buffer [B + 2, H, W, C + pad] and the [B, H, W, C] view a launch writes; `init` (logical NCHW, CPU) preloads the
    view (the in-place addend)"""

    def __init__(self, B, H, W, C, pad, init=None, flat=None):
        n = (B + 2) * H * W * (C + pad)
        self.buf = (torch.empty(n, device="cuda") if flat is None else flat[:n]).view(B + 2, H, W, C + pad)
        self.view = self.buf[1:B + 1, ..., :C]
        self.init = None if init is None else init.permute(0, 2, 3, 1).cuda()
        self.reset()

    def reset(self):
        self.buf.fill_(NAN)
        if self.init is not None:
            self.view.copy_(self.init)

    def intact(self):
        C = self.view.shape[3]
        return bool(torch.isnan(self.buf[0]).all() and torch.isnan(self.buf[-1]).all() and torch.isnan(self.buf[1:-1, ..., C:]).all())

    def logical(self):
        return self.view.permute(0, 3, 1, 2).contiguous().cpu()


class _FlatOut:
    """NaN-filled flat device buffer with a guard of G floats on either side of the n a launch writes"""
    G = 64

    def __init__(self, n, shape=None):
        self.n, self.shape = n, shape
        self.buf = torch.empty(n + 2 * self.G, device="cuda")
        self.view = self.buf[self.G:self.G + n]
        self.reset()

    def reset(self):
        self.buf.fill_(NAN)

    def intact(self):
        return bool(torch.isnan(self.buf[:self.G]).all() and torch.isnan(self.buf[self.G + self.n:]).all())

    def logical(self):
        v = self.view.cpu()
        return v.view(self.shape) if self.shape else v


def _flat_in(t, poison=NAN):
    """contiguous CPU tensor -> the same on the device, inside a poison buffer with guards on either side"""
    G, n = _FlatOut.G, t.numel()
    buf = torch.full((n + 2 * G,), poison, device="cuda")
    buf[G:G + n] = t.reshape(-1).cuda()
    return buf[G:G + n].view(t.shape)


def _check_rc(rc, what):
    from centerpose_amd import _lib
    _lib.check(rc, what)


def build(case):
    """-> (launch() -> kernel name or None, [output holder], extra() -> [failure text] or None).  launch() enqueues the row once."""
    import ctypes

    from centerpose_amd import _lib, ops
    row, p, t = case.row, case.p, case.t
    kind, pad = row.launcher, p["pad"]
    B, H, W, C = p["B"], p["H"], p["W"], p["C"]
    Ho, Wo = out_hw(row, p)

    def of(launch):
        def go():
            launch.kernel = None
            launch.run()
            return launch.kernel
        return go

    def noted(call, what):
        def go():
            _check_rc(call(), what)
            return None
        return go
    if kind == "maxpool":
        out = _OutView(B, Ho, Wo, C, pad)
        return of(ops.maxpool2d_launch(_in_view(t["x"], pad, INF), out.view, p["k"], p["s"], p["p"])), [out], None
    if kind in ("dw_deconv", "dw_deconv2"):
        x, wk = _in_view(t["x"], pad), ops.pack_dw_deconv_weight(t["w"].cuda())
        out = _OutView(B, Ho, Wo, C, pad, init=t["add"] if p["add"] == "inplace" else None)
        add = out.view if p["add"] == "inplace" else _in_view(t["add"], pad + 4) if p["add"] else None
        la = ops.dw_deconv_add_launch(x, wk, add, out.view, p["f"])
        env = p.get("env")

        def go():
            old = os.environ.get("CP_DWDECONV2")
            if env is not None:
                os.environ["CP_DWDECONV2"] = env          # read by the launcher on every call
            try:
                return of(la)()
            finally:
                if old is None:
                    os.environ.pop("CP_DWDECONV2", None)
                else:
                    os.environ["CP_DWDECONV2"] = old
        return go, [out], None
    if kind == "sum_up":
        out = _OutView(B, H, W, C, pad)
        return of(ops.sum_up_launch([_in_view(x, pad) for x in t["xs"]], p["shifts"], out.view, p["relu"])), [out], None
    if kind == "sum_up_group":
        ms = p["members"]
        sizes = [(m["B"] + 2) * m["H"] * m["W"] * (m["C"] + pad) for m in ms]
        whole = torch.empty(sum(sizes), device="cuda")
        outs, singles, off = [], [], 0
        for m, n in zip(ms, sizes):
            outs.append(_OutView(m["B"], m["H"], m["W"], m["C"], pad, flat=whole[off:off + n]))
            singles.append(_OutView(m["B"], m["H"], m["W"], m["C"], pad))
            off += n
        srcs = [[_in_view(x, pad) for x in xs] for xs in t["xs"]]
        la = ops.sum_up_group_launch([(s, m["shifts"], o.view) for s, m, o in zip(srcs, ms, outs)], whole, p["relu"])

        def extra():
            """the same members through one cp_sum_up_nhwc_f32 launch each: bit-identical"""
            fails = []
            for k, (s, m, o, single) in enumerate(zip(srcs, ms, outs, singles)):
                ops.sum_up_launch(s, m["shifts"], single.view, p["relu"]).run()
                torch.cuda.synchronize()
                if not torch.equal(o.view, single.view):
                    fails.append("member %d differs from its own cp_sum_up_nhwc_f32 launch" % k)
            return fails
        return of(la), outs, extra
    if kind == "dwconv":
        out = _OutView(B, Ho, Wo, C, pad)
        la = ops.dwconv2d_launch(_in_view(t["x"], pad), ops.pack_dw_weight(t["w"].cuda()), t["scale"].cuda(), t["shift"].cuda(), out.view, p["k"],
                                 p["s"], p["k"] // 2, ACTS.index(p["act"]))
        return of(la), [out], None
    if kind == "scale_add":
        out = _OutView(B, H, W, C, pad)
        add = _in_view(t["add"], pad + 4) if p["add"] else None
        return of(ops.scale_add_launch(_in_view(t["x"], pad), _in_view(t["se"], 8), add, out.view)), [out], None
    if kind == "shuffle_concat":
        h, hp = p["h"], p["hp"]
        out = _OutView(B, H, W, 2 * hp, pad)
        out.logical = lambda: lo.logical(out.view.cpu(), lo.View(H, W, 2 * h, None, (h, hp)))
        out.physical = lambda: out.view.cpu()
        return of(ops.shuffle_concat_launch(_in_view(t["x1"], pad), _in_view(t["x2"], pad + 4), out.view, h, hp)), [out], None
    L = _lib.lib()
    vp = lambda a: ctypes.c_void_p(a.data_ptr())
    if kind == "flip_merge":
        x, perm = _flat_in(t["x"]), t["perm"].cuda()
        out = _FlatOut(C * H * W, (1, C, H, W))
        return noted(lambda: L.cp_flip_merge_f32(vp(x), vp(out.view), C, H, W, p["mode"], vp(perm), _lib.stream()), "cp_flip_merge_f32"), [out], None
    if kind == "fill":
        out = _FlatOut(p["n"])
        dst = ctypes.c_void_p(out.buf.data_ptr() + 4 * out.G)             # an empty view has no data pointer of its own
        return noted(lambda: L.cp_fill_f32(dst, ctypes.c_float(FILL_VALUE), ctypes.c_longlong(p["n"]), _lib.stream()), "cp_fill_f32"), [out], None
    if kind == "dcn_pack":
        w, bias = _flat_in(t["w"]), _flat_in(t["bias"])
        ldw, Cp = p["ldw"], p["Cp"]
        outs = [_FlatOut(ldw * 9 * Cp, (ldw, 9 * Cp)), _FlatOut(ldw), _FlatOut(ldw)]
        call = lambda: L.cp_dcn_pack_weights_f32(vp(w), vp(bias), p["Co"], C, 3, 3, p["dg"], Cp, ldw, vp(outs[0].view), vp(outs[1].view),
                                                 vp(outs[2].view), _lib.stream())
        return noted(call, "cp_dcn_pack_weights_f32"), outs, None
    if kind == "global_avgpool":
        out = _OutView(B, 1, 1, C, pad)
        return of(ops.global_avgpool_launch(_in_view(t["x"], pad), out.view)), [out], None
    if kind == "nchw_to_nhwc":
        ld, cOff = p["ld"], p["cOff"]
        x = _flat_in(t["x"])
        out = _OutView(B, H, W, ld, 0)

        def intact():
            b = out.buf
            return bool(torch.isnan(b[0]).all() and torch.isnan(b[-1]).all() and torch.isnan(b[1:-1, ..., :cOff]).all()
                        and torch.isnan(b[1:-1, ..., cOff + C:]).all())
        out.intact = intact
        out.logical = lambda: out.view[..., cOff:cOff + C].permute(0, 3, 1, 2).contiguous().cpu()

        def go():
            ops.nchw_to_nhwc(x, out.view, cOff)
            return None
        return go, [out], None
    assert kind == "nhwc_to_nchw", kind
    ld, cOff = p["ld"], p["cOff"]
    buf = torch.full((B + 2, H, W, ld), NAN, device="cuda")
    buf[1:B + 1, ..., cOff:cOff + C] = t["x"].permute(0, 2, 3, 1).cuda()
    out = _FlatOut(B * C * H * W, (B, C, H, W))
    call = lambda: L.cp_nhwc_to_nchw_f32(vp(buf[1:B + 1]), ld, cOff, vp(out.view), B, C, H, W, _lib.stream())
    return noted(call, "cp_nhwc_to_nchw_f32"), [out], None


def run_row(rid, keep=False):
    """Build the row, run it twice (from re-initialised outputs) and judge it.  -> dict(kernel, worst (lo.Worst or None), c (or None:
    bit-equal), failures [text], outs (the first run's logical outputs when `keep`))"""
    case = make_case(rid)
    with torch.no_grad():
        launch, holders, extra = build(case)
        runs = []
        for _ in range(2):
            for h in holders:
                h.reset()
            kernel = launch()
            torch.cuda.synchronize()
            runs.append(([h.logical() for h in holders], [h.intact() for h in holders]))
        fails = []
        for h in holders:
            if hasattr(h, "physical"):                 # the padding channels the kernel owns: exact zeros
                hh, hp_ = case.p["h"], case.p["hp"]
                loc = lo.padding_violation(h.physical(), lo.View(0, 0, 2 * hh, None, (hh, hp_)))
                if loc is not None:
                    fails.append("padding channel not zero at (b, y, x, c) = %s" % (loc,))
        if extra is not None:
            fails += extra()
        o32, o64 = references(case)
        worst, jf = judge(case, runs[0][0], o32, o64)
    fails += jf
    if not (all(runs[0][1]) and all(runs[1][1])):
        fails.append("stored outside the view the launch was given (NaN guard overwritten)")
    for a, b in zip(runs[0][0], runs[1][0]):
        if not torch.equal(a.view(torch.int32), b.view(torch.int32)):         # bit patterns: a NaN the first run left is no difference
            fails.append("a second run gives other bits at %s" % (lo.first_unequal(a, b),))
    return dict(kernel=kernel, worst=worst, c=bound(case, o64), failures=fails, outs=runs[0][0] if keep else None)


# ---- stand-ins for a wrong kernel (tests/test_helper_oracle_cpu.py) ------------------------------------------------------------------
def as_rows(v):
    """logical NCHW [B, C, H, W] -> [B * H, W * C]: the rows of the launch, channel fastest (4 floats per element e)"""
    B, C, H, W = v.shape
    return v.permute(0, 2, 3, 1).reshape(B * H, W * C)


def from_rows(rows, shape):
    B, C, H, W = shape
    return rows.view(B, H, W, C).permute(0, 3, 1, 2).contiguous()


# ---- refusals: argument checks of the launchers --------------------------------------------------------------------------------------
# Every entry calls one launcher with arguments it must refuse: rc == 1 and cp_last_error() names the launcher and the argument.
# `P(n)` hands out a pointer to n floats.  On the device every pointer is a real zeroed buffer large enough for whatever an
# unrefused launch would read or write (gpu=True rows only: sizes are chosen so).  Rows with gpu=False cannot be backed by any buffer
# (one pixel past LIM, a grid of 2^32 blocks) or would trap on the host (s = 0): they run where there is no device, with dummy
# pointers -- no launch can happen there, whichever way the check goes (an unrefused call returns rc 2: "no device").
Refusal = collections.namedtuple("Refusal", "id launcher arg call gpu")
BIG = 1 << 20


def _refusals():
    import ctypes
    c_int, vp = ctypes.c_int, ctypes.c_void_p
    arr = lambda ty, vals: (ty * len(vals))(*vals)
    S = vp(0)                                            # the null stream
    out = []
    add = lambda id, launcher, arg, call, gpu=True: out.append(Refusal(id, launcher, arg, call, gpu))
    C4 = LIM_C // 4
    assert accepts(LIM_W, C4) and not accepts(LIM_W + 1, C4)

    def maxpool(B=2, H=8, W=8, C=8, k=2, s=2, p=0):
        return lambda L, P: L.cp_maxpool2d_nhwc_f32(P(BIG), C, P(BIG), C, B, H, W, C, k, s, p, S)
    add("maxpool-B0", "maxpool", "B=0", maxpool(B=0))
    add("maxpool-H0", "maxpool", "H=0", maxpool(H=0, k=3, p=1))
    add("maxpool-W0", "maxpool", "W=0", maxpool(W=0, k=3, p=1))
    add("maxpool-k0", "maxpool", "k=0", maxpool(k=0, s=1))
    add("maxpool-p-ge-k", "maxpool", "p=2", maxpool(p=2))
    add("maxpool-p-negative", "maxpool", "p=-1", maxpool(k=3, p=-1))
    add("maxpool-window", "maxpool", "Ho", maxpool(H=2, W=2, k=5))
    add("maxpool-s0", "maxpool", "s=0", maxpool(s=0), gpu=False)
    add("maxpool-row", "maxpool", "row too large", maxpool(B=1, H=1, W=LIM_W + 1, C=LIM_C, k=1, s=1), gpu=False)

    def deconv(B=2, H=4, W=4, C=8, f=2):
        return lambda L, P: L.cp_dw_deconv_add_nhwc_f32(P(BIG), C, P(BIG), P(BIG), C, P(BIG), C, B, H, W, C, f, S)
    add("deconv-B0", "dw_deconv_add", "B=0", deconv(B=0))
    add("deconv-H0", "dw_deconv_add", "H=0", deconv(H=0))
    add("deconv-W0", "dw_deconv_add", "W=0", deconv(W=0))
    add("deconv-C0", "dw_deconv_add", "C=0", deconv(C=0))
    add("deconv-row-f1", "dw_deconv_add", "row too large", deconv(B=1, H=1, W=LIM_W + 1, C=LIM_C, f=1), gpu=False)
    add("deconv-row-f2", "dw_deconv_add", "row too large", deconv(B=1, H=1, W=LIM_W // 2 + 1, C=LIM_C, f=2), gpu=False)

    def sum_up(shifts, B=2, H=4, W=4, C=8):
        n = len(shifts)
        return lambda L, P: L.cp_sum_up_nhwc_f32(n, arr(vp, [P(BIG).value for _ in range(4)]), arr(c_int, [C] * 4), arr(c_int, list(shifts) + [0] * (4 - n)),
                                                 P(BIG), C, B, H, W, C, 1, S)
    # the sources of the indivisible cases are BIG floats each: more than one spare image behind the B the launch is given
    add("sum_up-H-indivisible", "sum_up", "H=5", sum_up((1,), H=5))
    add("sum_up-W-indivisible", "sum_up", "W=5", sum_up((0, 1), W=5))
    add("sum_up-second-source", "sum_up", "source 1", sum_up((1, 2), H=6, W=4))
    add("sum_up-B0", "sum_up", "B=0", sum_up((0,), B=0))
    add("sum_up-H0", "sum_up", "H=0", sum_up((0,), H=0))
    add("sum_up-shift-negative", "sum_up", "shift=-1", sum_up((-1,)), gpu=False)
    add("sum_up-row", "sum_up", "row too large", sum_up((0,), B=1, H=1, W=LIM_W + 1, C=LIM_C), gpu=False)

    def group(members):
        """members: [(shifts, B, H, W, C)]"""
        n = len(members)
        meta = []
        for sh, B, H, W, C in members:
            meta += [len(sh)] + [C] * 4 + list(sh) + [0] * (4 - len(sh)) + [C, B, H, W, C]
        meta += [0] * (14 * (4 - n))
        return lambda L, P: L.cp_sum_up_group_nhwc_f32(n, arr(vp, [P(BIG).value for _ in range(16)]), arr(c_int, meta),
                                                       arr(vp, [P(BIG).value for _ in range(4)]), 1, S)
    ok = ((0,), 2, 4, 4, 8)
    add("group-H-indivisible", "sum_up_group", "member 1 source 1", group([ok, ((0, 1), 2, 5, 4, 8)]))
    add("group-W-indivisible", "sum_up_group", "member 0 source 0", group([((2,), 2, 4, 6, 8), ok]))
    add("group-H0", "sum_up_group", "H=0", group([ok, ((0,), 2, 0, 4, 8)]))
    add("group-shift-negative", "sum_up_group", "shift=-1", group([ok, ((-1,), 2, 4, 4, 8)]), gpu=False)
    add("group-row", "sum_up_group", "member 1: row too large", group([ok, ((0,), 1, 1, LIM_W + 1, LIM_C)]), gpu=False)
    add("group-grid", "sum_up_group", "grid", group([((0,), 32768, 32768, 1, 4)] * 4), gpu=False)

    add("dwconv-row", "dwconv", "bad shape",
        lambda L, P: L.cp_dwconv2d_nhwc_f32(P(BIG), LIM_C, P(BIG), P(BIG), P(BIG), P(BIG), LIM_C, 1, 1, LIM_W + 1, LIM_C, 1, 1, 0, 0, S), gpu=False)
    add("scale_add-row", "scale_add", "row too large",
        lambda L, P: L.cp_scale_add_nhwc_f32(P(BIG), LIM_C, P(BIG), LIM_C, P(BIG), LIM_C, P(BIG), LIM_C, 1, 1, LIM_W + 1, LIM_C, S), gpu=False)

    def avgpool(inLd, outLd, C=16):
        return lambda L, P: L.cp_global_avgpool_nhwc_f32(P(BIG), inLd, P(BIG), outLd, 2, 5, C, S)
    add("avgpool-inLd", "global_avgpool", "inLd=8", avgpool(8, 16))
    add("avgpool-outLd", "global_avgpool", "outLd=12", avgpool(16, 12))

    def to_nhwc(B=2, C=3, H=4, W=4):
        return lambda L, P: L.cp_nchw_to_nhwc_f32(P(4 * BIG), P(4 * BIG), B, C, H, W, C, 0, S)

    def to_nchw(B=2, C=3, H=4, W=4):
        return lambda L, P: L.cp_nhwc_to_nchw_f32(P(4 * BIG), C, 0, P(4 * BIG), B, C, H, W, S)
    for name, f in (("nchw_to_nhwc", to_nhwc), ("nhwc_to_nchw", to_nchw)):
        add(name + "-B0", name, "B=0", f(B=0))
        add(name + "-C0", name, "C=0", f(C=0))
        add(name + "-H0", name, "H=0", f(H=0))
        add(name + "-HW", name, "2^31 pixels", f(B=1, C=1, H=65536, W=32768), gpu=False)
        add(name + "-B-grid", name, "B=65536", f(B=65536, C=1, H=1, W=1))                  # 65536 floats each way
        add(name + "-C-grid", name, "C=%d" % (32 * 65535 + 1), f(B=1, C=32 * 65535 + 1, H=1, W=1))     # 2 097 121 floats each way
    return out


REFUSALS = _refusals()
REFUSAL = {r.id: r for r in REFUSALS}
assert len(REFUSAL) == len(REFUSALS)


def refuse(rid, device):
    """call the refusal row -> (rc, cp_last_error() text).  device: real zeroed buffers; else dummy non-null pointers (no device only)."""
    import ctypes

    from centerpose_amd import _lib
    L = _lib.lib()
    keep = []

    def P(n):
        if not device:
            return ctypes.c_void_p(4096)
        keep.append(torch.zeros(n, device="cuda"))
        return ctypes.c_void_p(keep[-1].data_ptr())
    rc = REFUSAL[rid].call(L, P)
    if device:
        torch.cuda.synchronize()
    return rc, L.cp_last_error().decode()
