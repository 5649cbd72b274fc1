"""TEST INFRASTRUCTURE ONLY -- every epilogue path of the conv and DCN kernels, per element against float64.

The MFMA kernels pick their output code at run time from facts about the caller's pointers and strides: a float4 path through LDS, a
per-lane scalar NHWC path and an LDS-transposed NCHW path in `ig_epilogue` (igemm_conv_kernel, igemm_conv_group_kernel,
dcn_igemm_kernel, igemm_bf16x3_kernel), the same vector / scalar pair in conv3x3_patch_kernel, a per-item choice in the two Winograd
output functions, a host-side split between the two instantiations of the F(2x4) kernels, and the alignment-driven fall-backs of the
`tile = 0` dispatcher.  tests/launch_oracle.py pads every row to 16 channels on aligned buffers, so it reaches the vector path alone.

This module is the table of cases (`CASES`, `GROUPS`), the case builder (`build`, `build_group`) and the judging (`judge_flat`), on top of
`layer_oracle` (`_fold`, `_activate`, `head_branch`, `judge`, `c_for`, `tile_A`) and `launch_oracle` (`Row`-style bases, `_head_inst`):

* a BASE is one kernel instantiation at the smallest shape of launch_oracle (B = 2, 19 x 37, or 37 x 37 where a 16-row tile needs an
  interior tile; >= 3 reduction stages; >= 2 channel blocks where the instantiation has them);
* a MODE says where the output (and residual) live: V (aligned, Cout = 44), S-cout (43 / 27), S-ld (outLd = 45), S-ptr (a channel slice
  1 / 2 / 3 floats into an aligned buffer), S-res (residual 1 float in / resLd = 45), NCHW (Cout 1 / 17 / 34, aligned and 1 float in),
  V-pad (48 channels given of which 4 are padding: the exact-zero rule of launch_oracle, 0.5 after a sigmoid / h-sigmoid),
  scatter (the sub-pixel deconvolution: each phase on its own and the fused four), plus the dispatcher's fall-back edges (mode "fb");
  an instantiation whose N tile caps the channel count (conv3x3_patch_kernel<16, ...>: ldw = 16) takes 12 / 11 / 7 channels instead;
* every (base, mode) runs the five activations and residual on / off in a covering design (`DESIGN`), not the full product.

The float64 accumulation (convolution, transposed convolution, DCN sampling) and its magnitude sum are computed ONCE per base
(`accumulate`); `reference` applies scale / shift, residual and activation of one case to its first `cout` channels, which is
`lo._conv_bn` / `lo.dcn_stage` restated on the cached sum (tests/test_epilogue_oracle_cpu.py holds the two together bit for bit).

Outputs live in a NaN-filled FLAT buffer with a guard of 64 floats on both sides (`Layout`): every float the launch does not own --
channels from Cout to ld, floats in front of a slice, the other scatter phases, the guards -- must still be NaN afterwards.  Except in
mode V-pad the cases give the launch exactly `cout` channels, so there are no padding channels inside it.

`expected_path` is a small Python restatement of the kernels' predicates; on the device the only path evidence is the kernel name in
`Launch.kernel`.  Nothing here reads device results or kernel sources to set a bound: every bound is `layer_oracle.c_for`.
"""
import collections
import functools

import torch
import torch.nn.functional as F

import launch_oracle as L
import layer_oracle as lo
from oracle import dcn as oracle_dcn

G = 64                                                     # guard floats on both sides of every output
ACTS = ("none", "relu", "sigmoid", "hswish", "hsigmoid")
ACT_CODE = {a: i for i, a in enumerate(ACTS)}              # ops.ACT_*
_LO_ACT = {"none": None, "relu": "relu", "sigmoid": "sigmoid", "hswish": "hswish", "hsigmoid": "hsigmoid"}
# covering design: every activation, residual on and off; longer modes go round again with the residual flipped
DESIGN = (("none", True), ("relu", False), ("sigmoid", True), ("hswish", False), ("hsigmoid", True),
          ("none", False), ("relu", True), ("sigmoid", False), ("hswish", True), ("hsigmoid", False))
# Liveness: with launch_oracle's BN magnitudes a pre-activation stays inside +-3 and the clamps of h-swish / h-sigmoid never fire.  The
# folded scale of those rows is multiplied by H_GAIN (chosen on the CPU so that the floors of tests/test_epilogue_oracle_cpu.py hold:
# >= 10 % below -3, >= 10 % above +3, >= 30 % inside); the residual is ReLU(N(0.5, 1)) / 2: non-zero on about 69 % of the elements.
H_GAIN = 24.0
LIVE = {"relu_neg": (0.2, 0.8), "h_low": 0.1, "h_high": 0.1, "h_in": 0.3, "res_nonzero": 0.5}

Base = collections.namedtuple("Base", "id kind family kernel p")
IG = "igemm_conv_kernel<%s>"
PATCH = "conv3x3_patch_kernel<%s>"
W24 = "conv3x3_wino24_kernel<%s>"


def _b(id, kind, family, kernel, **p):
    d = dict(B=2, H=19, W=37, k=3, stride=1, pad=1, tile=0, ldw=0, couts=(44, 43, 27), nchw_in=False, bf16=False)
    d.update(p)
    return Base(id, kind, family, kernel, d)


BASES = [
    # generic implicit GEMM: ldw two N tiles wide (the second block lies wholly behind the `n < Cout` guard)
    _b("ig-64x64", "conv", "direct", IG % "64, 64, 2, 2, 32, false", cin=32, tile=64064, ldw=128),
    _b("ig-128x32", "conv", "direct", IG % "128, 32, 4, 1, 32, false", cin=16, tile=128032, ldw=64),
    _b("ig-256x16", "conv", "direct", IG % "256, 16, 4, 1, 16, false", cin=16, tile=256016, ldw=48),
    _b("ig-128x128", "conv", "direct", IG % "128, 128, 2, 2, 32, false", cin=32, tile=128128, ldw=256),
    _b("bf16x3", "conv", "direct", "igemm_bf16x3_kernel<128, 64>", cin=32, ldw=128, bf16=True),
    _b("patch-16", "conv", "direct", PATCH % "16, 4, 1, 16", cin=48, tile=3, ldw=16, couts=(12, 11, 7), H=37),
    _b("patch-32", "conv", "direct", PATCH % "32, 4, 1, 32", cin=48, tile=3, ldw=64, H=37),
    _b("patch-64", "conv", "direct", PATCH % "64, 2, 2, 32", cin=80, tile=3, ldw=128, H=37),
    _b("wino-1x1", "conv", "wino", "conv3x3_wino_kernel<1, 1, 16, 2>", cin=48, tile=11),
    _b("wino-1x2", "conv", "wino", "conv3x3_wino_kernel<1, 2, 16, 2>", cin=48, tile=12),
    _b("wino-vs64", "conv", "wino", "conv3x3_wino_vs64_kernel<0, 0>", cin=64, tile=6402),
    _b("wino24", "conv", "wino24", None, cin=48, tile=24, H=37),            # <true> / <false>: `expected_kernel`
    _b("dcn-64x64", "dcn", "dcn", "dcn_igemm_kernel<64, 64, 2, 2, 32>", cin=48, tile=64064, ldw=128),
    _b("dcn-64x32", "dcn", "dcn", "dcn_igemm_kernel<64, 32, 4, 1, 16>", cin=48, tile=64032, ldw=64),
    _b("splitk", "splitk", "direct", "splitk_reduce_kernel", cin=32, tile=64064, ldw=64, S=2),
    _b("head-wino", "head", "wino", "conv3x3_wino_vs64_kernel%s", cin=64, hc=32, couts=(34, 34, 34)),
    _b("head-wino24", "head", "wino24", "head_wino24_kernel%s", cin=64, hc=32, couts=(34, 34, 34)),
    # the sub-pixel deconvolution ConvTranspose2d(k4, s2, p1) as 2 x 2 convolutions (K = 4 cin)
    _b("sc-64x64", "deconv", "direct", IG % "64, 64, 2, 2, 32, false", cin=32, k=2, tile=64064, ldw=128),
    _b("sc-128x32", "deconv", "direct", IG % "128, 32, 4, 1, 32, false", cin=48, k=2, tile=128032, ldw=64),
    _b("sc-256x16", "deconv", "direct", IG % "256, 16, 4, 1, 16, false", cin=48, k=2, tile=256016, ldw=48),
    _b("sc-128x128", "deconv", "direct", IG % "128, 128, 2, 2, 32, false", cin=32, k=2, tile=128128, ldw=256),
    _b("sc-bf16x3", "deconv", "direct", "igemm_bf16x3_kernel<128, 64>", cin=32, k=2, ldw=128, bf16=True),
    # members of the grouped launches
    _b("grp-a", "conv", "direct", "igemm_conv_group_kernel", cin=48, ldw=64),
    _b("grp-b", "conv", "direct", "igemm_conv_group_kernel", cin=32, ldw=64),
    _b("g24-a", "conv", "wino24", None, cin=64, H=37),
    _b("g24-b", "conv", "wino24", None, cin=48, H=37),
    _b("g24-c", "conv", "wino24", None, cin=32, H=37),
    # dispatcher fall-backs (tile = 0)
    _b("c16-16-s1", "conv", "direct", "conv3x3_c16_kernel<1, 1, 8, 32, 4, 2>", cin=16, couts=(16, 16, 16)),
    _b("c16-32-s1", "conv", "direct", "conv3x3_c16_kernel<2, 1, 8, 32, 2, 2>", cin=16, couts=(32, 32, 32)),
    _b("c16-16-s2", "conv", "direct", "conv3x3_c16_kernel<1, 2, 8, 16, 3, 2>", cin=16, couts=(16, 16, 16), stride=2, H=37, W=45),
    _b("c16-32-s2", "conv", "direct", "conv3x3_c16_kernel<2, 2, 8, 16, 3, 1>", cin=16, couts=(32, 32, 32), stride=2, H=37, W=45),
    _b("pw-44", "conv", "direct", "pw_conv_kernel<64, 64, 4>", cin=64, k=1, pad=0),
    _b("pw-88", "conv", "direct", "pw_conv_kernel<64, 64, 4>", cin=64, k=1, pad=0, couts=(88, 87, 87)),
    _b("stem3", "conv", "direct", "stem7x7_c16_kernel<64, 2, 3>", cin=3, stride=2, H=19, W=40, couts=(64, 64, 64), nchw_in=True),
    _b("stem7-16", "stem7", "direct", "stem7x7_c16_kernel<16, 1, 7>", cin=3, k=7, pad=3, H=19, W=40, couts=(16, 16, 16), nchw_in=True),
    _b("stem7-64", "stem7", "direct", "stem7x7_c16_kernel<64, 2, 7>", cin=3, k=7, pad=3, stride=2, H=19, W=40, couts=(64, 64, 64), nchw_in=True),
    _b("fb-bf16", "conv", "direct", "igemm_bf16x3_kernel<128, 64>", cin=32, ldw=64, bf16=True),
]
BASE = {b.id: b for b in BASES}
assert len(BASE) == len(BASES)

_CASE_FIELDS = "id base mode sub act res cout ld off rld roff soff uoff nchw scatter kernel tile cpad"
Case = collections.namedtuple("Case", _CASE_FIELDS)


def _rup4(n):
    return -(-n // 4) * 4


def _case(bid, mode, sub, act, res, cout, **kw):
    """ld / off: output pixel stride and offset in floats from a 16-byte aligned address; rld / roff: the residual's; soff / uoff: offset
    of the source / the Winograd weights; scatter: None, (py, px) or "fused"; kernel: the expected `Launch.kernel`, None = rejected;
    cpad > cout: the launch is GIVEN cpad channels, the last cpad - cout of them padding (zero weights, scale, shift and residual)"""
    d = dict(ld=_rup4(cout) + 4, off=0, rld=_rup4(cout) + 8, roff=0, soff=0, uoff=0, nchw=False, scatter=None, tile=BASE[bid].p["tile"], kernel="",
             cpad=0)
    d.update(kw)
    if d["nchw"]:
        d["ld"] = 0
    c = Case("%s/%s/%s/%s%s" % (bid, mode, sub, act, "+res" if res else ""), bid, mode, sub, act, res, cout, **d)
    return c._replace(kernel=expected_kernel(c)) if c.kernel == "" else c


# ---- the kernels' predicates, restated ------------------------------------------------------------------------------------------------
def given(c):
    """the channel count the launch is given (its Cout)"""
    return c.cpad or c.cout


def vec_ok(c):
    """16-byte aligned NHWC output (and residual) with pixel strides that keep every pixel aligned"""
    return not c.nchw and c.ld % 4 == 0 and c.off % 4 == 0 and (not c.res or (c.rld % 4 == 0 and c.roff % 4 == 0))


def expected_path(c):
    """the body a block takes: vector / scalar / nchw, mixed (Winograd: items with n + 3 < Cout vector, the last one scalar) or reject"""
    b = BASE[c.base]
    if rejected(c):
        return "reject"
    if c.nchw:
        return "nchw"
    if b.kind == "head":
        return "nchw"
    if b.kind == "splitk":                                 # splitk_reduce_kernel has one body: float4 stores wherever `out` points
        return "vector"
    if b.family in ("wino", "wino24"):
        return "scalar" if not vec_ok(c) else "vector" if given(c) % 4 == 0 else "mixed"
    return "vector" if vec_ok(c) and given(c) % 4 == 0 else "scalar"


def rejected(c):
    """the launchers' own argument checks: NCHW output takes no residual (conv_args_from_desc); cp_splitk_reduce_f32 wants Cout and outLd
    multiples of four; the Winograd and head entry points want 16-byte aligned sources and weights"""
    b = BASE[c.base]
    if c.nchw and c.res:
        return True
    if b.kind == "splitk" and (c.cout % 4 or c.ld % 4):
        return True
    if (b.family in ("wino", "wino24")) and (c.soff % 4 or c.uoff % 4):
        return True
    return False


def w24_fast(c):
    """w24_fast_epilogue: the lean instantiation of the F(2x4) kernels"""
    return vec_ok(c) and given(c) % 4 == 0 and c.act in ("none", "relu")


def expected_kernel(c):
    b = BASE[c.base]
    if rejected(c):
        return None
    if b.kind == "head":
        return b.kernel % L._head_inst(c.cout)
    if b.kernel is None:
        return W24 % ("true" if w24_fast(c) else "false")
    return b.kernel


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
NHWC_MODES = ("V", "S-cout", "S-ld", "S-ptr", "S-res")
PAD_BASES = ("ig-64x64", "patch-32", "wino-1x2", "wino24", "dcn-64x64")         # one per implementation of the vector body


def _mode_cases(bid, mode, has_res=True):
    b = BASE[bid]
    cv, c1, c2 = b.p["couts"]
    out = []
    if mode == "V":
        for act, res in DESIGN[:5]:
            out.append(_case(bid, mode, "c%d" % cv, act, res and has_res, cv))
    elif mode == "V-pad":                                   # 44 channels and 4 padding channels: exact zeros (0.5 after a sigmoid / h-sigmoid)
        for act, res in DESIGN[:5]:
            out.append(_case(bid, mode, "c%dof%d" % (cv, cv + 4), act, res and has_res, cv, cpad=cv + 4, ld=cv + 8, rld=cv + 12))
    elif mode == "S-cout":
        for i, (act, res) in enumerate(DESIGN[:5]):
            co = (c1, c2)[i % 2]
            out.append(_case(bid, mode, "c%d" % co, act, res and has_res, co))
    elif mode == "S-ld":
        for act, res in DESIGN[:5]:
            out.append(_case(bid, mode, "ld%d" % (cv + 1), act, res and has_res, cv, ld=cv + 1))
    elif mode == "S-ptr":
        for i, (act, res) in enumerate(DESIGN[:5]):
            out.append(_case(bid, mode, "off%d" % (i % 3 + 1), act, res and has_res, cv, ld=_rup4(cv) + 8, off=i % 3 + 1))
    elif mode == "S-res":                                   # aligned output; the residual is what is off: always on
        for i, (act, _) in enumerate(DESIGN[:5]):
            kw = dict(roff=1) if i % 2 == 0 else dict(rld=cv + 1)
            out.append(_case(bid, mode, "roff1" if i % 2 == 0 else "rld%d" % (cv + 1), act, True, cv, **kw))
    elif mode == "NCHW":                                    # Ho Wo = 19 x 37 = 703, odd
        # (a single channel carries launch_oracle's smallest scale: it takes the activations that have no floor to meet)
        for co, off, act in ((1, 0, "none"), (34, 1, "relu"), (1, 1, "sigmoid"), (17, 0, "hswish"), (34, 0, "hsigmoid"), (17, 1, "none")):
            out.append(_case(bid, mode, "c%d-off%d" % (co, off), act, False, co, nchw=True, off=off))
        if has_res:
            out.append(_case(bid, mode, "c17-res", "relu", True, 17, nchw=True))          # rejected: no launch
    elif mode == "scatter":
        subs = (((0, 0), cv), ((0, 1), c1), ((1, 0), cv), ((1, 1), c2), ("fused", cv), ("fused", c1))
        for i, (ph, co) in enumerate(subs):
            act, res = DESIGN[i]
            name = "fused" if ph == "fused" else "p%d%d" % ph
            out.append(_case(bid, mode, "%s-c%d" % (name, co), act, res, co, scatter=ph))
    else:
        raise ValueError(mode)
    return out


def _head_cases(bid):
    out = []
    for n2 in (1, 2, 17, 33, 34):
        for act in ("none", "sigmoid"):
            out.append(_case(bid, "heads", "n%d" % n2, act, False, n2, nchw=True, off=1))
    return out


def _fallback_cases():
    out = []

    def fb(bid, sub, act="relu", res=True, tile=0, **kw):
        out.append(_case(bid, "fb", sub, act, res, kw.pop("cout", BASE[bid].p["couts"][0]), tile=tile, **kw))

    # c16: eligible, then one predicate at a time; stride 1 -> the patch kernel, stride 2 -> the generic kernel of the padded channel count
    for co, pk, gk in ((16, PATCH % "16, 4, 1, 16", IG % "256, 16, 4, 1, 16, false"), (32, PATCH % "32, 4, 1, 32", IG % "128, 32, 4, 1, 32, false")):
        for s, to in ((1, pk), (2, gk)):
            bid = "c16-%d-s%d" % (co, s)
            fb(bid, "eligible")
            fb(bid, "sigmoid", act="sigmoid", kernel=to)
            fb(bid, "hswish", act="hswish", kernel=to)
            fb(bid, "out+1", off=1, ld=co + 8, kernel=to)
            fb(bid, "outLd", ld=co + 1, kernel=to)
            fb(bid, "res+1", roff=1, kernel=to)
            fb(bid, "src+1", soff=1, kernel=to)
    g64 = IG % "64, 64, 2, 2, 32, false"
    for bid in ("pw-44", "pw-88"):
        co = BASE[bid].p["couts"][0]
        fb(bid, "eligible")
        fb(bid, "sigmoid", act="sigmoid", kernel=g64)
        fb(bid, "cout", cout=co - 1, kernel=g64)
        fb(bid, "src+1", soff=1, kernel=g64)
        fb(bid, "out+1", off=1, ld=co + 8, kernel=g64)
        fb(bid, "res+1", roff=1, kernel=g64)
    gs = IG % "128, 64, 2, 2, 32, true"
    fb("stem3", "eligible", res=False)
    fb("stem3", "out+1", res=False, off=1, ld=72, kernel=gs)
    fb("stem3", "outLd", res=False, ld=65, kernel=gs)
    fb("stem3", "sigmoid", act="sigmoid", res=False, kernel=gs)
    fb("stem3", "res", res=True, kernel=gs)
    for bid, to in (("stem7-16", "stem7x7_kernel<16, 1, 8, 64>"), ("stem7-64", "stem7x7_kernel<64, 2, 8, 32>")):
        co = BASE[bid].p["couts"][0]
        fb(bid, "eligible", res=False)
        fb(bid, "x+1", res=False, soff=1, kernel=to)
        fb(bid, "out+1", res=False, off=1, ld=co + 8, kernel=to)
        fb(bid, "outLd", res=False, ld=co + 1, kernel=to)
    # Winograd and head entry points: a source or U one float in is refused ("shape not eligible"), nothing is launched
    # (`tile` there names the transform and the block shape, 11 / 12 / 6402 / 24: the check sits in front of all of them)
    for bid in ("wino-1x1", "wino-1x2", "wino-vs64", "wino24"):
        fb(bid, "src+1", soff=1, tile=BASE[bid].p["tile"])
        fb(bid, "u+1", uoff=1, tile=BASE[bid].p["tile"])
    # F(2x4): tile = 24 says which transform the weights are in; lean or generic instantiation is the host's choice (w24_fast_epilogue)
    fb("wino24", "eligible", tile=24)
    fb("wino24", "sigmoid", act="sigmoid", tile=24)
    fb("wino24", "hswish", act="hswish", tile=24)
    fb("wino24", "cout", cout=43, tile=24)
    fb("wino24", "out+1", off=1, ld=52, tile=24)
    fb("wino24", "res+1", roff=1, tile=24)
    for bid in ("head-wino", "head-wino24"):
        out.append(_case(bid, "fb", "src+1", "none", False, 17, nchw=True, soff=1))
        out.append(_case(bid, "fb", "u+1", "none", False, 17, nchw=True, uoff=1))
    # split_bf16=True: ops.conv2d_launch leaves a launch with a misaligned source on the f32 path (tile = 0: the patch kernel)
    fb("fb-bf16", "eligible")
    fb("fb-bf16", "src+1", soff=1, kernel=PATCH % "32, 4, 1, 32")
    # DCN: the sampler's 16-byte gathers from a source one float in
    out.append(_case("dcn-64x64", "fb", "src+1", "relu", False, 44, soff=1))
    return out


def _all_cases():
    out = []
    for bid in ("ig-64x64", "ig-128x32", "ig-256x16", "ig-128x128", "bf16x3"):
        for mode in NHWC_MODES + ("NCHW",):
            out += _mode_cases(bid, mode)
    for bid in ("patch-16", "patch-32", "patch-64", "wino-1x1", "wino-1x2", "wino-vs64", "wino24"):
        for mode in NHWC_MODES:
            out += _mode_cases(bid, mode)
    for bid in ("dcn-64x64", "dcn-64x32"):
        for mode in ("V", "S-cout", "S-ld", "S-ptr", "NCHW"):
            out += _mode_cases(bid, mode, has_res=False)
    for bid in PAD_BASES:
        out += _mode_cases(bid, "V-pad", has_res=BASE[bid].kind != "dcn")
    for mode in ("V", "S-cout", "S-ld", "S-ptr"):
        out += _mode_cases("splitk", mode, has_res=False)
    for bid in ("sc-64x64", "sc-128x32", "sc-256x16", "sc-128x128", "sc-bf16x3"):
        out += _mode_cases(bid, "scatter")
    out += _head_cases("head-wino") + _head_cases("head-wino24")
    out += _fallback_cases()
    return out


CASES = _all_cases()
CASE = {c.id: c for c in CASES}
assert len(CASE) == len(CASES), [k for k, v in collections.Counter(c.id for c in CASES).items() if v > 1]

# grouped launches: (expected kernel, members).  A block's path follows its own member.
GROUPS = {
    "igemm-group": ("igemm_conv_group_kernel", [_case("grp-a", "group", "V", "relu", True, 44), _case("grp-b", "group", "S-cout", "hswish", True, 43)]),
    "wino24-group-mixed": ("conv3x3_wino24_group_kernel<false>", [_case("g24-a", "group", "V", "relu", True, 44, kernel=None),
                                                                 _case("g24-b", "group", "V", "relu", False, 44, kernel=None),
                                                                 _case("g24-c", "group", "S-cout", "relu", True, 43, kernel=None)]),
    "wino24-group-fast": ("conv3x3_wino24_group_kernel<true>", [_case("g24-a", "group", "V", "relu", True, 44, kernel=None),
                                                                _case("g24-b", "group", "V", "relu", False, 44, kernel=None),
                                                                _case("g24-c", "group", "V", "none", True, 44, kernel=None)]),
}


def group_kernel(members):
    """restated: an F(2x4) group launch is fast only if all members are"""
    if BASE[members[0].base].family == "wino24":
        return "conv3x3_wino24_group_kernel<%s>" % ("true" if all(w24_fast(m) for m in members) else "false")
    return "igemm_conv_group_kernel"


# ---- data and references ------------------------------------------------------------------------------------------------------------------
Data = collections.namedtuple("Data", "x sd res om Ho Wo cmax")


@functools.lru_cache(maxsize=None)
def base_data(bid):
    """the base's data (CPU, float32, logical NCHW), fixed by seed; `cmax` output channels, every case takes a prefix"""
    b = BASE[bid]
    p = b.p
    g = torch.Generator().manual_seed(7000 + BASES.index(b))
    r = lambda *s: torch.randn(*s, generator=g)
    u01 = lambda n: torch.rand(n, generator=g)
    B, H, W, ci, k = p["B"], p["H"], p["W"], p["cin"], p["k"]
    cmax = max(p["couts"])
    x = F.relu(r(B, ci, H, W))
    bn = lambda n: {"b.weight": u01(n) + 0.5, "b.bias": r(n) * 0.1, "b.running_mean": r(n) * 0.1, "b.running_var": u01(n) + 0.5}
    om = None
    if b.kind == "deconv":
        Ho, Wo = 2 * H, 2 * W
        sd = lo.spread_bn(dict(bn(cmax), **{"c.weight": r(ci, cmax, 4, 4) * (2.0 / (4 * ci)) ** 0.5}))
    elif b.kind == "head":
        Ho, Wo, hc = H, W, p["hc"]
        sd = {"h.0.weight": r(hc, ci, 3, 3) * (2.0 / (9 * ci)) ** 0.5 * lo.spread_factors(hc).view(-1, 1, 1, 1), "h.0.bias": r(hc) * 0.1,
              "h.2.weight": r(cmax, hc, 1, 1) * (2.0 / hc) ** 0.5 * lo.spread_factors(cmax).view(-1, 1, 1, 1), "h.2.bias": r(cmax) * 0.5 - 1.0}
    elif b.kind == "dcn":
        Ho, Wo = H, W
        sd = lo.spread_bn(dict(bn(cmax), **{"d.weight": r(cmax, ci, 3, 3) * (4.0 / (9 * ci)) ** 0.5, "d.bias": r(cmax) * 0.1}))
        om = torch.cat([r(B, 18, H, W) * 2.5, r(B, 9, H, W) * 1.5], 1)
    else:
        Ho, Wo = (H + 2 * p["pad"] - k) // p["stride"] + 1, (W + 2 * p["pad"] - k) // p["stride"] + 1
        sd = lo.spread_bn(dict(bn(cmax), **{"c.weight": r(cmax, ci, k, k) * (2.0 / (k * k * ci)) ** 0.5}))
    res = F.relu(r(B, cmax, Ho, Wo) + 0.5) * 0.5
    return Data(x, sd, res, om, Ho, Wo, cmax)


def params(bid, act, cout):
    """the case's parameters: the base's, first `cout` channels, the BN weight x H_GAIN for the h-swish / h-sigmoid rows"""
    sd = base_data(bid).sd
    out = {}
    for k, v in sd.items():
        if k.startswith("h.0"):
            out[k] = v
        elif k == "c.weight" and BASE[bid].kind == "deconv":
            out[k] = v[:, :cout]
        else:
            out[k] = v[:cout]
    if act in ("hswish", "hsigmoid") and "b.weight" in out:
        out["b.weight"] = out["b.weight"] * H_GAIN
    return out


@functools.lru_cache(maxsize=None)
def accumulate(bid, dt, wino=None):
    """the pre-activation accumulation of all `cmax` channels in dtype `dt` and, for float64, its magnitude sum -> (acc, Aacc or None, K).
    wino: the textbook transform (float32 yardstick of the Winograd families)"""
    b, d = BASE[bid], base_data(bid)
    p = b.p
    x = d.x.to(dt)
    f64 = dt == torch.float64
    with torch.no_grad():
        if b.kind == "deconv":
            w = d.sd["c.weight"].to(dt)
            return (F.conv_transpose2d(x, w, None, 2, 1), F.conv_transpose2d(x.abs(), w.abs(), None, 2, 1) if f64 else None, 4 * p["cin"] + 4)
        if b.kind == "dcn":
            om = d.om.to(dt)
            off, mask = om[:, :18].contiguous(), torch.sigmoid(om[:, 18:27]).contiguous()
            w = d.sd["d.weight"].to(dt)
            acc = oracle_dcn.dcn_v2_forward_torch(x, w, None, off, mask)
            A = None
            if f64:                                        # as lo.dcn_stage: the float32 sampling coordinate
                P = 2.0 * (max(p["H"], p["W"]) + 2)
                A = oracle_dcn.dcn_v2_forward_torch(x.abs() + P * F.max_pool2d(x.abs(), 3, 1, 1), w.abs(), None, off, mask)
            return acc, A, 9 * p["cin"] + 4
        w = d.sd["c.weight"].to(dt)
        acc = lo._conv(x, w, p["stride"], p["pad"], 1, wino, dt)
        return acc, F.conv2d(x.abs(), w.abs(), None, p["stride"], p["pad"]) if f64 else None, p["cin"] * p["k"] * p["k"] + 4


def pre_activation(c, dt, wino=None):
    """(v, A or None, K): scale / shift and residual applied to the cached accumulation, before the activation"""
    b, d = BASE[c.base], base_data(c.base)
    sd = params(c.base, c.act, c.cout)
    acc, Aacc, K = accumulate(c.base, dt, wino)
    scale, shift, ash = lo._fold(sd, "b", "d.bias" if b.kind == "dcn" else None, c.cout, dt)
    v = acc[:, :c.cout] * scale + shift
    A = scale.abs() * Aacc[:, :c.cout] + ash if Aacc is not None else None
    if c.res:
        res = d.res[:, :c.cout].to(dt)
        v = v + res
        A = A + res.abs() if A is not None else None
    return v, A, K


def yardstick_family(c):
    f = BASE[c.base].family
    return f if f in ("wino", "wino24") else None


@functools.lru_cache(maxsize=None)
def _head_ref(bid, n2, act, dt, wino):
    b, d = BASE[bid], base_data(bid)
    with torch.no_grad():
        return lo.head_branch(params(bid, "none", n2), d.x.to(dt), "h.0", "h.2", b.p["hc"], n2, None if act == "none" else act, dt, wino)


def reference(c, dt=torch.float64, wino=None):
    """the case's whole operation -> lo.Out over the FULL logical output [B, cout, Ho, Wo] (a single scatter phase is cut out by its
    Layout)"""
    if BASE[c.base].kind == "head":
        return _head_ref(c.base, c.cout, c.act, dt, wino)
    with torch.no_grad():
        v, A, K = pre_activation(c, dt, wino)
        v, A = lo._activate(v, A, _LO_ACT[c.act])
    return lo.Out(v, A, K, hsig=c.act == "hsigmoid")


def yardstick(c):
    """the float32 torch evaluation that stands in for the kernel on the CPU"""
    return reference(c, torch.float32, yardstick_family(c))


# ---- where an output lives --------------------------------------------------------------------------------------------------------------
class Layout:
    """One launch's output inside a flat NaN-filled buffer: `G` guard floats, `off` floats, the tensor, `G` guard floats, from float
    `start` of the buffer (a 16-byte aligned position).  NHWC [B, OH, OW, C] with `ld` floats per pixel, or NCHW [B, C, OH, OW].  phase
    (py, px): the launch owns only the pixels (2 y + py, 2 x + px).  `idx` [B, C, h, w]: flat position of every owned element."""

    def __init__(self, B, C, OH, OW, ld=0, off=0, nchw=False, phase=None, start=0):
        self.B, self.C, self.OH, self.OW, self.ld, self.off, self.nchw, self.phase, self.start = B, C, OH, OW, ld, off, nchw, phase, start
        assert nchw or ld >= C
        self.n = B * C * OH * OW if nchw else B * OH * OW * ld
        self.size = _rup4(G + off + self.n + G)
        self.origin = start + G + off
        py, px = phase if phase else (0, 0)
        step = 2 if phase else 1
        b, ch, y, x = torch.meshgrid(torch.arange(B), torch.arange(C), torch.arange(py, OH, step), torch.arange(px, OW, step), indexing="ij")
        self.idx = self.origin + self.position(b, ch, y, x)

    def position(self, b, ch, y, x, nchw=None, ld=None):
        if self.nchw if nchw is None else nchw:
            return ((b * self.C + ch) * self.OH + y) * self.OW + x
        return ((b * self.OH + y) * self.OW + x) * (ld or self.ld) + ch

    def view(self, flat):
        """the tensor the launch is given"""
        if self.nchw:
            return flat[self.origin:self.origin + self.n].view(self.B, self.C, self.OH, self.OW)
        return torch.as_strided(flat, (self.B, self.OH, self.OW, self.C), (self.OH * self.OW * self.ld, self.OW * self.ld, self.ld, 1), self.origin)


def layout(c, start=0):
    b, d = BASE[c.base], base_data(c.base)
    phase = c.scatter if isinstance(c.scatter, tuple) else None
    return Layout(b.p["B"], given(c), d.Ho, d.Wo, c.ld, c.off, c.nchw, phase, start)


def new_flat(size, dev="cpu"):
    return torch.full((size,), float("nan"), device=dev)


def logical(c, lay, full):
    """the elements of the full logical output that the launch owns (a scatter phase: every second pixel)"""
    if lay.phase:
        return full[:, :, lay.phase[0]::2, lay.phase[1]::2]
    return full


def judge_flat(c, lay, flat, o64):
    """flat: the CPU copy of the buffer after the run -> (lo.Worst, [failure text], logical output).  Every float of the layout's own
    stretch [start, start + size) outside `lay.idx` must still be NaN (the members of a group launch lie back to back: each judges its
    own stretch); every owned element inside c u A of the float64 reference."""
    fam = BASE[c.base].family
    fails = []
    free = torch.ones(flat.numel(), dtype=torch.bool)
    free[lay.idx.reshape(-1)] = False
    free[:lay.start] = False
    free[lay.start + lay.size:] = False
    stray = free & ~torch.isnan(flat)
    if bool(stray.any()):
        pos = int(torch.nonzero(stray)[0])
        fails.append("%d float(s) outside the output were written, the first %d floats from the tensor's origin (%r): Cout = %d, ld = %d"
                     % (int(stray.sum()), pos - lay.origin, float(flat[pos]), c.cout, c.ld))
    out = flat[lay.idx]
    if c.cpad:                                             # the existing exact-zero rule for the padding channels the launch was given
        phys = out.permute(0, 2, 3, 1)
        if c.act == "sigmoid":                             # sigmoid(0) is exactly 0.5; a zero there means the activation was skipped
            phys = torch.cat([phys[..., :c.cout], phys[..., c.cout:] - 0.5], 3)
        loc = lo.padding_violation(phys, lo.View(lay.OH, lay.OW, c.cout, None, None), hsig=c.act == "hsigmoid")
        if loc is not None:
            fails.append("padding channel not %s at (b, y, x, c) = %s: %r" % ("0.5" if c.act in ("sigmoid", "hsigmoid") else "zero", loc,
                                                                              float(out.permute(0, 2, 3, 1)[loc])))
        out = out[:, :c.cout]
    ref = lo.Out(logical(c, lay, o64.val), logical(c, lay, o64.A), o64.K)
    w, fail = lo.judge(out, None, ref, fam)
    if fail:
        fails.append(fail)
    return w, fails, out


def standin(c, out32, lay=None):
    """a CPU buffer that holds `out32` (full logical output) where the launch would have stored it"""
    lay = lay or layout(c)
    flat = new_flat(lay.size)
    val = logical(c, lay, out32).float()
    if c.cpad:                                             # act(0 * 0 + 0 + 0) in the padding channels
        fill = torch.full((val.shape[0], c.cpad - c.cout) + tuple(val.shape[2:]), 0.5 if c.act in ("sigmoid", "hsigmoid") else 0.0)
        val = torch.cat([val, fill], 1)
    flat[lay.idx] = val
    return lay, flat


def liveness(c):
    """fractions of the case's own data (CPU, float64 pre-activations) that the floors of `LIVE` / lo.LIVE_FLOOR speak about"""
    b, d = BASE[c.base], base_data(c.base)
    out = {}
    if b.kind == "head":
        if c.act == "sigmoid":
            out["sigmoid"] = lo.sigmoid_liveness(reference(c).val)
        return out
    v, _, _ = pre_activation(c, torch.float64)
    if c.act == "relu":
        out["relu_neg"] = float((v < 0).double().mean())
    if c.act in ("hswish", "hsigmoid"):
        out["h_low"], out["h_high"] = float((v < -3).double().mean()), float((v > 3).double().mean())
        out["h_in"] = float(((v > -3) & (v < 3)).double().mean())
    if c.act == "sigmoid":
        out["sigmoid"] = lo.sigmoid_liveness(torch.sigmoid(v))
    if c.res:
        out["res_nonzero"] = float((d.res[:, :c.cout] != 0).double().mean())
    if b.kind == "dcn":
        out["dcn_samples"], out["dcn_masks"] = lo.dcn_liveness(d.om)
    return out


def live_failures(c):
    fails = []
    if rejected(c):                                        # nothing is launched: the data is never used
        return fails
    for key, frac in liveness(c).items():
        floor = LIVE[key] if key in LIVE else lo.LIVE_FLOOR[key]
        lo_, hi = floor if isinstance(floor, tuple) else (floor, 1.0)
        if not lo_ <= frac <= hi:
            fails.append("degenerate test data: %s = %.3f outside [%.2f, %.2f]" % (key, frac, lo_, hi))
    return fails


# ---- device -------------------------------------------------------------------------------------------------------------------------------
def put_nhwc(t, dev, ld=None, off=0):
    """logical NCHW CPU tensor -> NHWC view [B, H, W, C] with `ld` floats per pixel, `off` floats into a 16-byte aligned zero buffer"""
    B, C, H, W = t.shape
    ld = ld or C
    flat = torch.zeros(_rup4(G + off + B * H * W * ld + G), device=dev)
    v = torch.as_strided(flat, (B, H, W, C), (H * W * ld, W * ld, ld, 1), G + off)
    v.copy_(t.permute(0, 2, 3, 1))
    return v


def put_flat(t, dev, off=0):
    """a contiguous tensor `off` floats into a 16-byte aligned buffer"""
    flat = torch.zeros(_rup4(G + off + t.numel() + G), device=dev)
    v = flat[G + off:G + off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


Built = collections.namedtuple("Built", "launches flat lays keep")


def _conv_member(c, lay, flat, dev):
    """the operands of one convolution case on the device -> dict(srcs, wp, scale, shift, out, res, u, kw)"""
    from centerpose_amd import ops
    b, d = BASE[c.base], base_data(c.base)
    p, co, cg = b.p, c.cout, given(c)
    sd = params(c.base, c.act, co)
    bnp = tuple(sd["b." + s].to(dev) for s in ("weight", "bias", "running_mean", "running_var"))
    ldw = max(p["ldw"], ops.ldw_for(cg))
    sc, sh = (ops.pad_vec(v, ldw) for v in ops.fold_bn(co, bnp))
    pad = lambda wp: ops.pad_rows(wp, ldw)
    kw = dict(kh=p["k"], kw=p["k"], stride=p["stride"], pad=p["pad"], tile=c.tile, in_nchw=p["nchw_in"], out_nchw=c.nchw, cout=cg,
              act=ACT_CODE[c.act])
    if b.kind == "deconv":
        wd = sd["c.weight"].to(dev)
        H, W = p["H"], p["W"]
        if c.scatter == "fused":
            wp = torch.cat([pad(ops.pack_deconv4_subpixel(wd, py, px)) for py in range(2) for px in range(2)], 0).contiguous()
            kw.update(stride=1, pad=0, pad_yx=(1, 1), Ho=H, Wo=W, out_scatter=(2, 2, 0, 0), nsub=4)
        else:
            py, px = c.scatter
            wp = pad(ops.pack_deconv4_subpixel(wd, py, px))
            kw.update(stride=1, pad=0, pad_yx=(1 - py, 1 - px), Ho=H, Wo=W, out_scatter=(2, 2, py, px))
    else:
        wp = pad(ops.pack_conv_weight(sd["c.weight"].to(dev), stem=p["nchw_in"]))
    srcs = [put_flat(d.x, dev, c.soff)] if p["nchw_in"] else [put_nhwc(d.x, dev, off=c.soff)]
    res = put_nhwc(F.pad(d.res[:, :co], (0, 0, 0, 0, 0, cg - co)), dev, c.rld, c.roff) if c.res else None
    u = None
    if b.family in ("wino", "wino24"):
        u = (ops.pack_wino24_weight if b.family == "wino24" else ops.pack_wino_weight)(wp, p["cin"], cg)
        if c.uoff:
            u = put_flat(u, dev, c.uoff)
    return dict(srcs=srcs, wp=wp, scale=sc, shift=sh, out=lay.view(flat), res=res, u=u, kw=kw)


def build(c, dev="cuda"):
    """-> Built(launches in order, flat NaN buffer, [Layout], tensors to keep alive)"""
    from centerpose_amd import ops
    b, d = BASE[c.base], base_data(c.base)
    p, co = b.p, c.cout
    lay = layout(c)
    flat = new_flat(lay.size, dev)
    out = lay.view(flat)
    if b.kind == "head":
        sd, hc = params(c.base, "none", co), p["hc"]
        wp3 = ops.pack_conv_weight(sd["h.0.weight"].to(dev))
        u = (ops.pack_wino24_weight if b.family == "wino24" else ops.pack_wino_weight)(wp3, 64, hc)
        if c.uoff:
            u = put_flat(u, dev, c.uoff)
        sc, sh = ops.fold_bn(hc, None, sd["h.0.bias"].to(dev))
        la = ops.head3x3_1x1_launch(put_nhwc(d.x, dev, off=c.soff), u, sc, sh, sd["h.2.weight"].reshape(co, hc).contiguous().to(dev), sd["h.2.bias"].to(dev),
                                    out, hc=hc, act2=ACT_CODE[c.act], wino24=b.family == "wino24")
        return Built([la], flat, [lay], None)
    if b.kind == "stem7":
        sd = params(c.base, c.act, co)
        sc, sh = ops.fold_bn(co, tuple(sd["b." + s].to(dev) for s in ("weight", "bias", "running_mean", "running_var")))
        la = ops.stem7x7_launch(put_flat(d.x, dev, c.soff), ops.pack_stem7_weight(sd["c.weight"].to(dev)), sc, sh, out, p["stride"], relu=c.act == "relu")
        return Built([la], flat, [lay], None)
    if b.kind == "dcn":
        sd = params(c.base, c.act, co)
        ldw = max(p["ldw"], ops.ldw_for(given(c)))
        wp = ops.pad_rows(ops.pack_conv_weight(sd["d.weight"].to(dev)), ldw)
        sc, sh = (ops.pad_vec(v, ldw) for v in ops.fold_bn(co, tuple(sd["b." + s].to(dev) for s in ("weight", "bias", "running_mean", "running_var")),
                                                           sd["d.bias"].to(dev)))
        la = ops.dcn_v2_launch(put_nhwc(d.x, dev, off=c.soff), put_nhwc(d.om, dev, ld=32), wp, sc, sh, out, cout=given(c), om_sigmoid=True, act=ACT_CODE[c.act],
                               out_nchw=c.nchw, tile=c.tile)
        return Built([la], flat, [lay], None)
    m = _conv_member(c, lay, flat, dev)
    if b.kind == "splitk":
        S, ldw = p["S"], m["wp"].shape[0]
        ws = torch.full((S, p["B"] * d.Ho * d.Wo, ldw), float("nan"), device=dev)
        kw = dict(m["kw"], cout=ldw, act=ops.ACT_NONE, ksplit=S)
        la = ops.conv2d_launch(m["srcs"], m["wp"], torch.ones(ldw, device=dev), torch.zeros(ldw, device=dev), ws, split_bf16=False, **kw)
        return Built([la, ops.splitk_reduce_launch(ws, m["scale"], m["shift"], out, cout=co, act=ACT_CODE[c.act])], flat, [lay], ws)
    la = ops.conv2d_launch(m["srcs"], m["wp"], m["scale"], m["shift"], m["out"], res=m["res"], wino=m["u"], split_bf16=p["bf16"], **m["kw"])
    return Built([la], flat, [lay], m)


def build_group(gid, dev="cuda"):
    """the members of GROUPS[gid] in ONE launch, their outputs back to back in one flat buffer"""
    from centerpose_amd import ops
    _, members = GROUPS[gid]
    lays, start = [], 0
    for c in members:
        lays.append(layout(c, start))
        start += lays[-1].size
    flat = new_flat(start, dev)
    ms = [_conv_member(c, lay, flat, dev) for c, lay in zip(members, lays)]
    if BASE[members[0].base].family == "wino24":
        la = ops.conv3x3_group_launch([dict(x=m["srcs"][0], wp=m["wp"], u24=m["u"], scale=m["scale"], shift=m["shift"], out=m["out"], cout=c.cout,
                                            act=ACT_CODE[c.act], res=m["res"]) for c, m in zip(members, ms)], flat)
    else:
        la = ops.conv2d_group_launch([dict(x=m["srcs"][0], wp=m["wp"], scale=m["scale"], shift=m["shift"], out=m["out"], cout=c.cout, k=BASE[c.base].p["k"],
                                           stride=1, pad=BASE[c.base].p["pad"], act=ACT_CODE[c.act], res=m["res"]) for c, m in zip(members, ms)], flat)
    return Built([la], flat, lays, ms)


def _run(built, expect_reject):
    """run the launches; -> (kernel names, error text or None)"""
    from centerpose_amd import _lib
    try:
        for l in built.launches:
            l.run()
        torch.cuda.synchronize()
    except _lib.CenterposeHipError as e:
        if not expect_reject:
            raise
        return [l.kernel for l in built.launches], str(e)
    return [l.kernel for l in built.launches], None


def run_case(cid):
    """Build the case, run it twice and judge it -> dict(kernel, path, worst, c, failures, out)"""
    c = CASE[cid]
    return _judge_run([c], build(c), c.kernel)


def run_group(gid):
    kernel, members = GROUPS[gid]
    return _judge_run(members, build_group(gid), kernel)


def _judge_run(members, built, kernel):
    rep = dict(kernel=None, failures=[], worst=[], out=[], c=[], path=[expected_path(c) for c in members])
    with torch.no_grad():
        names, err = _run(built, kernel is None)
        if kernel is None:
            if err is None:
                rep["failures"].append("the launcher accepted a launch it was expected to refuse (dispatched to %s)" % names[-1])
            elif "kernel launch failed" in err or not err.strip():
                rep["failures"].append("not a clean refusal: %s" % err)
            if not bool(torch.isnan(built.flat).all()):
                rep["failures"].append("a refused launch wrote to its output")
            rep["error"] = err
            return rep
        rep["kernel"] = names[-1]
        first = built.flat.cpu()
        _run(built, False)
        second = built.flat.cpu()
    if not torch.equal(first.view(torch.int32), second.view(torch.int32)):
        rep["failures"].append("a second run gives other bits")
    for c, lay in zip(members, built.lays):
        o64 = reference(c)
        w, fails, out = judge_flat(c, lay, first, o64)
        rep["worst"].append(w)
        rep["c"].append(lo.c_for(BASE[c.base].family, o64.K))
        rep["out"].append(out)
        rep["failures"] += ["%s: %s" % (c.id, f) for f in fails]
    return rep
