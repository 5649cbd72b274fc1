"""TEST INFRASTRUCTURE ONLY -- the hot-path launchers at the last shape their 32-bit offset checks accept (LIM).

The MFMA kernels do their address arithmetic in 32 bits and the launchers keep that safe with size checks.  This module

(a) restates every 32-bit quantity of those kernels as exact Python integers of the launch shape (`audit`: extreme values at the corner
    pixels, the last block, the last tap -- no thread enumeration) together with the launchers' checks (`checks`, `accepts`), the word
    width being a parameter: at 16 bits the same arithmetic drives numpy emulations of the generic producer and of the DCN record
    (`emulate_generic`, `emulate_dcn`) that tests/test_limit_oracle_cpu.py mutates;
(b) holds `ROWS`: one stand-alone launch per kernel family at LIM, the variant forced as in tests/launch_oracle.py (the opt-in split-bf16
    kernel with `split_bf16=True` and CP_SPLIT_BF16_TILE, as in tests/bf16x3_oracle.py);
(c) judges a row twice (`run_row`): crops against the float64 reference with `layer_oracle`'s unchanged per-element bound (`judged_crops`),
    and image 2 (image 1) of the LIM launch bit for bit against the same forced variant run on that image ALONE, copied to a fresh buffer
    where every offset is small.

LIM geometry: every NHWC source is a channel slice of a 64-float-wide buffer (ld = 64), B = 3, H = 1365, W = 4097: B H W = 4095 x 4097 =
2^24 - 1 pixels and B H W ld 4 = 2^32 - 256 bytes.  Image 1 straddles byte 2^31 of the source, image 2 lies wholly above it; 4097 and
1365 are ragged against every tile in use.

Every restated expression cites its source line (centerpose_amd/csrc/...), as tests/helper_oracle.py does.
"""
import collections
import gc
import time

import numpy as np
import torch
import torch.nn.functional as F

import launch_oracle as L
import layer_oracle as lo

LIM_B, LIM_H, LIM_W, LIM_LD = 3, 1365, 4097, 64
assert LIM_B * LIM_H * LIM_W == 2 ** 24 - 1 and LIM_B * LIM_H * LIM_W * LIM_LD * 4 == 2 ** 32 - 256
MEM_LIMIT = 12 * 2 ** 30          # bytes a row may hold at once


def cdiv(a, b):
    return -(-a // b)


# ======================================================================================================================================
# (a) the index audit
# ======================================================================================================================================
Q = collections.namedtuple("Q", "name where ctype lo hi fits")
Check = collections.namedtuple("Check", "name where value limit ok")


def c_range(ctype, w):
    """value range of a C type at word width w: int, unsigned, a packed field of `unsigned:<bits>`, grid (a dim3 x extent)"""
    if ctype == "int":
        return -(1 << (w - 1)), (1 << (w - 1)) - 1
    if ctype == "unsigned":
        return 0, (1 << w) - 1
    if ctype == "grid":
        return 1, (1 << (w - 1)) - 1
    assert ctype.startswith("field"), ctype
    return 0, (1 << int(ctype[5:])) - 1


def _q(name, where, ctype, lo_, hi, w):
    a, b = c_range(ctype, w)
    return Q(name, where, ctype, lo_, hi, a <= lo_ and hi <= b)


def wrap(v, ctype, w):
    """what a w-bit register of `ctype` holds after computing the exact integer(s) v (numpy int64 or int)"""
    m = (1 << w) - 1
    u = v & m
    if ctype == "unsigned":
        return u
    return np.where(u >> (w - 1), u - (1 << w), u) if isinstance(u, np.ndarray) else (u - (1 << w) if u >> (w - 1) else u)


def shape(B=LIM_B, H=LIM_H, W=LIM_W, ld=LIM_LD, C=32, k=3, stride=1, pad=1, cout=16, ldw=16, outLd=20, resLd=0, S=1, lds=None, nchw=False,
          nsub=1):
    """a launch shape; lds: the pixel strides of all sources (default [ld])"""
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return dict(B=B, H=H, W=W, ld=ld, lds=list(lds) if lds else [ld], C=C, k=k, stride=stride, pad=pad, cout=cout, ldw=ldw, outLd=outLd,
                resLd=resLd, S=S, nchw=nchw, nsub=nsub, Ho=Ho, Wo=Wo)


def magic(d, w=32):
    """wg_magic / w24_magic / hw_magic (conv3x3_wino.hip:696, conv3x3_wino24.hip:410, head_wino24.hip:436): ceil(2^w / d), 0 for d <= 1"""
    return 0 if d <= 1 else ((1 << w) + d - 1) // d


def magic_div(n, d, w=32):
    """wg_div / w24_div / hw_div (conv3x3_wino.hip:56, conv3x3_wino24.hip:52, head_wino24.hip:56): d == 1 ? n : umulhi(n, magic)"""
    return n if d == 1 else (n * magic(d, w)) >> w


def magic_exact_upto(d, w=32):
    """largest N such that magic_div(n, d) == n // d for every 0 <= n <= N, in closed form: with m d = 2^w + e (0 <= e < d),
    floor(n m / 2^w) = floor(n / d + n e / (d 2^w)), which first exceeds n // d at the smallest n = q d + (d - 1) with n e >= 2^w"""
    if d <= 1:
        return (1 << w) - 1
    e = magic(d, w) * d - (1 << w)
    if e == 0:
        return (1 << w) - 1
    n0 = cdiv(1 << w, e)                       # n e >= 2^w from here on; the first n >= n0 with n % d == d - 1 fails
    first_bad = n0 + ((d - 1 - n0) % d)
    return min(first_bad - 1, (1 << w) - 1)


# ---- the launchers' checks -----------------------------------------------------------------------------------------------------------
def checks(family, s, w=32, fixed=True):
    """the size checks on the path of `family`, as the sources state them -> [Check].  fixed=False: conv_args_from_desc as it stood before
    this audit (no check of the NCHW source's B C H W, none of B Ho Wo)."""
    B, H, W, Ho, Wo = s["B"], s["H"], s["W"], s["Ho"], s["Wo"]
    half, full = 1 << (w - 1), 1 << w
    out = []
    add = lambda name, where, value, limit: out.append(Check(name, where, value, limit, value < limit))
    if family == "dcn":                                                   # cp_dcn_v2_f32
        add("dcn pixels", "dcn.hip:282", B * H * W, 1 << (w - 3))
        add("dcn bytes", "dcn.hip:282", B * H * W * s["ld"] * 4, full)
        return out
    if family in ("stem7", "stem7_c16"):                                  # cp_stem7x7_f32 has no refusal: eligibility of the persistent kernel
        if family == "stem7_c16":
            add("stem floats", "stem7x7.hip:308", B * 3 * H * W, half)
            add("stem tiles", "stem7x7.hip:257", B * cdiv(Wo, 64) * cdiv(Ho, 8 if s["cout"] == 16 else 4), half)
        return out
    add("conv pixels", "conv_igemm.hip:341", B * H * W, half)             # conv_args_from_desc: every cp_conv2d* / Winograd / head / group entry
    if fixed:
        add("conv rows", "conv_igemm.hip:344", B * Ho * Wo + 255, half)
        if s["nchw"]:
            add("conv nchw floats", "conv_igemm.hip:348", B * s["C"] * H * W, half)
    if not s["nchw"]:
        for i, ld in enumerate(s["lds"]):
            add("conv bytes[%d]" % i, "conv_igemm.hip:351", B * H * W * ld * 4, full)
    if family in ("wino", "wino_vs64", "wino24", "head_wino", "head_wino24", "patch", "c16"):
        where = {"wino": "conv3x3_wino.hip:775", "wino_vs64": "conv3x3_wino.hip:775", "wino24": "conv3x3_wino24.hip:420",
                 "head_wino": "conv3x3_wino.hip:757", "head_wino24": "head_wino24.hip:466", "patch": "conv3x3_patch.hip:258",
                 "c16": "conv3x3_c16.hip:212"}[family]
        add("source floats", where, B * H * W * s["ld"], half)
    if family in ("wino", "wino_vs64", "wino24", "head_wino", "head_wino24"):
        g = wino_grid(family, s)
        add("grid x dmax", {"wino": "conv3x3_wino.hip:716", "wino_vs64": "conv3x3_wino.hip:743", "head_wino": "conv3x3_wino.hip:743",
                            "wino24": "conv3x3_wino24.hip:435", "head_wino24": "head_wino24.hip:452"}[family], g["grid"] * g["dmax"], full)
    if family == "wino24":                                                # w24_fast_epilogue: eligibility of the lean epilogue
        add("w24 out row x16", "conv3x3_wino24.hip:408", W * s["outLd"] * 16, half)
        add("w24 res row x16", "conv3x3_wino24.hip:408", W * s["resLd"] * 16, half)
    if family == "c16":
        add("c16 out row x16", "conv3x3_c16.hip:212", Wo * s["outLd"] * 16, half)
        add("c16 res row x16", "conv3x3_c16.hip:213", Wo * s["resLd"] * 16, half)
        TH, TW = 8, 32 // s["stride"]
        add("c16 tiles", "conv3x3_c16.hip:192", B * cdiv(Wo, TW) * cdiv(Ho, TH), half)
    if family == "pw":
        add("pw bytes", "conv_pointwise.hip:173", B * Ho * Wo * s["ld"] * 4, full)
    return out


def accepts(family, s, w=32, fixed=True):
    return all(c.ok for c in checks(family, s, w, fixed))


def wino_grid(family, s):
    """WgGrid / W24Grid / HwGrid of the launch (conv3x3_wino.hip:709-715, 733-742, conv3x3_wino24.hip:428-433, head_wino24.hip:447-451)"""
    th = {"wino": 8 * s.get("MT", 1), "wino_vs64": 8, "head_wino": 8, "wino24": 16, "head_wino24": 16}[family]
    tx, ty = cdiv(s["W"], 16), cdiv(s["H"], th)
    nt = cdiv(s["cout"], 32)
    if family == "wino":
        ntb = cdiv(nt, s.get("NT", 1))
    elif family == "wino_vs64":
        ng = max(1, min(s.get("ngroups", 1), nt))
        ntb = cdiv(nt, cdiv(nt, ng))
    elif family == "wino24":
        ntb = nt
    else:
        ntb = 1                                                            # the head kernels: one block per spatial tile
    grid = s["B"] * tx * ty * ntb * (s["S"] if family == "wino" else 1)
    return dict(tilesX=tx, tilesY=ty, ntb=ntb, grid=grid, dmax=max(ntb, tx, ty))


def group24_total(shapes, w=32):
    """cp_launch_conv3x3_wino24_group (conv3x3_wino24.hip:472): the sum of the members' blocks, `first[]` being int"""
    total = sum(wino_grid("wino24", s)["grid"] for s in shapes)
    return Check("group24 total blocks", "conv3x3_wino24.hip:472", total, 1 << (w - 1), total < 1 << (w - 1))


# ---- the device quantities -----------------------------------------------------------------------------------------------------------
def _grid_q(name, where, blocks, w):
    return _q(name, where, "grid", blocks, blocks, w)


def audit(family, s, w=32, BM=64, BN=16, field=None):
    """extreme values of every 32-bit quantity the kernels of `family` form for launch shape `s` -> [Q].  BM / BN: the GEMM tile of the
    generic and DCN kernels; field: bits of the DCN record's offset field (default w - 4: 28 of 32)."""
    B, H, W, ld, C, Ho, Wo = s["B"], s["H"], s["W"], s["ld"], s["C"], s["Ho"], s["Wo"]
    last = B * H * W - 1                                  # the last input pixel: image B - 1, row H - 1, column W - 1
    M = B * Ho * Wo
    q = []
    add = lambda name, where, ctype, lo_, hi: q.append(_q(name, where, ctype, lo_, hi, w))
    if family == "bf16x3":                                                # igemm_bf16x3_kernel<BM, BN>: its own producer, the generic epilogue
        mx = max(s["lds"])
        add("a.M = B*Ho*Wo", "conv_igemm.hip:335", "int", M, M)
        add("m = m0 + tid/QS + s*128", "conv_igemm_bf16x3.hip:161", "int", 0, (cdiv(M, BM) - 1) * BM + BM - 1)
        add("ps.boff = b*H*W", "conv_igemm_bf16x3.hip:164", "int", -1, (B - 1) * H * W)
        add("boff + iy*W + ix", "conv_igemm_bf16x3.hip:189", "int", 0, last)
        # q*8 floats (half of a pixel's k-step, BM = 128: the second float4 is 16 bytes past aoff, added to the 64-bit pointer) or q*4 (quarter)
        add("aoff", "conv_igemm_bf16x3.hip:189", "unsigned", 0, (last * mx + (12 if BM == 64 else 8)) * 4)
        q.append(_grid_q("grid", "conv_igemm_bf16x3.hip:280", cdiv(M, BM) * (s["ldw"] // BN) * s["nsub"] * s["S"], w))
    if family in ("generic", "generic_stem", "group", "dcn", "pw"):
        add("a.M = B*Ho*Wo", "conv_igemm.hip:335", "int", M, M)
        add("m = m0 + row", "conv_igemm.hip:70", "int", 0, (cdiv(M, BM) - 1) * BM + BM - 1)
        blocks = cdiv(M, BM) * (s["ldw"] // BN) * s["nsub"] * s["S"]
        q.append(_grid_q("grid", "conv_igemm.hip:282" if family != "pw" else "conv_pointwise.hip:156", blocks, w))
    if family in ("generic", "group"):
        mx = max(s["lds"])
        add("ps.boff = b*H*W", "conv_igemm.hip:73", "int", -1, (B - 1) * H * W)
        add("boff + iy*W + ix", "conv_igemm.hip:106", "int", 0, last)
        add("aoff", "conv_igemm.hip:106", "unsigned", 0, (last * mx + 12) * 4)      # q = 3: the last float4 of a 16-channel k-step
    if family == "generic_stem":
        add("boff = b*C*H*W", "conv_igemm.hip:166", "int", -1, (B - 1) * C * H * W)
    if family == "dcn":
        fb = field if field is not None else w - 4
        add("bpix + yl*W + xl", "dcn.hip:114", "int", 0, last)
        add("s_code offset field", "dcn.hip:114", "field%d" % fb, 0, last * (ld // 4))
        add("s_code", "dcn.hip:114", "int", 0, last * (ld // 4) + (3 << (w - 3)))          # both flag bits set: stays below the sign bit
        add("o00", "dcn.hip:152", "unsigned", 0, ((last * (ld // 4)) << 4) + 48)
        add("pixb", "dcn.hip:141", "unsigned", ld * 4, ld * 4)
        add("rowb", "dcn.hip:141", "unsigned", W * ld * 4, W * ld * 4)
        # dxb / dyb are set only while the right / lower neighbour is inside the image: the farthest corner is still the last pixel
        add("o01, o10, o11", "dcn.hip:153-155", "unsigned", 0, last * ld * 4 + 48)
        add("boff (weights)", "dcn.hip:192", "unsigned", 0, ((s["ldw"] - 1) * 9 * C + 12) * 4)
    if family in ("wino", "wino_vs64", "wino24", "head_wino", "head_wino24", "patch"):
        qmax = {"wino": 3, "wino24": 3, "patch": 3}.get(family, 15)               # CGS - 1 channel quads of a stage (KS = 16) or of all 64 channels
        where = {"wino": "conv3x3_wino.hip:310", "wino_vs64": "conv3x3_wino.hip:538", "head_wino": "conv3x3_wino.hip:538",
                 "wino24": "conv3x3_wino24.hip:234", "head_wino24": "head_wino24.hip:88", "patch": "conv3x3_patch.hip:84"}[family]
        add("go = ((b*H+gy)*W+gx)*ld + q*4", where, "int", -1, last * ld + qmax * 4)
    if family in ("wino", "wino_vs64", "wino24", "head_wino", "head_wino24"):
        g = wino_grid(family, s)
        gl, dl = {"wino": ("conv3x3_wino.hip:718", "conv3x3_wino.hip:285-287"), "wino_vs64": ("conv3x3_wino.hip:744", "conv3x3_wino.hip:516-518"),
                  "head_wino": ("conv3x3_wino.hip:744", "conv3x3_wino.hip:516-518"), "wino24": ("conv3x3_wino24.hip:436-437", "conv3x3_wino24.hip:213-215"),
                  "head_wino24": ("head_wino24.hip:453", "head_wino24.hip:68-69")}[family]
        q.append(_grid_q("grid", gl, g["grid"], w))
        n = g["grid"] // (s["S"] if family == "wino" else 1) - 1                 # the largest dividend: the last block's index
        for nm, d in (("ntb", g["ntb"]), ("tilesX", g["tilesX"]), ("tilesY", g["tilesY"])):
            if family.startswith("head_wino24") and nm == "ntb":
                continue
            upto = magic_exact_upto(d, w)
            q.append(Q("mulhi division by %s = %d" % (nm, d), dl, "magic", n, upto, n <= upto and magic(d, w) < (1 << w)))
            n //= d
    if family == "wino24":
        add("(4*it+aa) * ostep", "conv3x3_wino24.hip:195", "int", 0, 13 * W * s["outLd"])
        add("(4*it+aa) * rstep", "conv3x3_wino24.hip:177", "int", 0, 13 * W * s["resLd"])
    if family == "patch":
        bn = s["ldw"] if s["ldw"] in (16, 32) else BN                            # launch_patch<16 / 32 / 64>: conv3x3_patch.hip:260-265
        q.append(_grid_q("grid", "conv3x3_patch.hip:246", B * cdiv(W, 16) * cdiv(H, 8) * (s["ldw"] // bn), w))
    if family == "c16":
        st = s["stride"]
        TH, TW = 8, 32 // st
        PH, HF4 = (TH - 1) * st + 3, ((TW - 1) * st + 3 - 32) * 4
        add("m_g", "conv3x3_c16.hip:62", "unsigned", 0, (1 * W + 31) * ld + 12)
        add("h_g", "conv3x3_c16.hip:65", "unsigned", 0, ((255 // HF4) * W + (128 + HF4 - 1) // 4) * ld + 12)   # every thread forms it, rows >= PH unused
        add("(b*H + iy0)", "conv3x3_c16.hip:71", "int", -1, (B - 1) * H + (cdiv(Ho, TH) - 1) * TH * st - 1)
        add("orow = Wo*outLd", "conv3x3_c16.hip:106", "int", 0, Wo * s["outLd"])
        add("rrow = Wo*resLd", "conv3x3_c16.hip:106", "int", 0, Wo * s["resLd"])
        nt = B * cdiv(Wo, TW) * cdiv(Ho, TH)
        add("ntiles", "conv3x3_c16.hip:196", "int", nt, nt)
        add("nxt = tl + gridDim", "conv3x3_c16.hip:115", "int", 0, nt - 1 + min(nt, 256 * 4))
        assert PH <= 255 // HF4 + 1
    # family "pw": conv_pointwise.hip:63, 77, 141 form every row offset as (size_t)m * ld -- nothing of its own is 32-bit
    if family in ("stem7", "stem7_c16"):
        add("(b*3 + c)", "stem7x7.hip:43", "int", 0, B * 3 - 1)
        if family == "stem7_c16":
            TH = 8 if s["cout"] == 16 else 4
            PHs = (TH - 1) * s["stride"] + s["k"]
            add("s_g = (c*H + py)*W + f*4", "stem7x7.hip:163", "int", 0, (2 * H + PHs - 1) * W + 136)
            nt = B * cdiv(Wo, 64) * cdiv(Ho, TH)
            add("ntiles", "stem7x7.hip:260", "int", nt, nt)
            add("(b*Ho + oyw)", "stem7x7.hip:212", "int", 0, B * Ho + TH)
        else:
            TH, TW = 8, (64 if s["cout"] == 16 else 32)
            q.append(_grid_q("grid = B*tilesX*tilesY", "stem7x7.hip:292", B * cdiv(Wo, TW) * cdiv(Ho, TH), w))
            add("(b*Ho + oy)", "stem7x7.hip:102", "int", 0, B * Ho - 1)
    return q


def overflows(family, s, w=32, **kw):
    return [x for x in audit(family, s, w, **kw) if not x.fits]


# ---- tier two: decode, flip_pairs, head_points (CPU audit only: their LIM maps are far above MEM_LIMIT) --------------------------------------
def checks_tier2(kind, w=32, fixed=True, **p):
    half = 1 << (w - 1)
    out = []
    add = lambda name, where, value, limit: out.append(Check(name, where, value, limit, value < limit))
    if kind == "decode":
        add("cat*H*W", "decode.hip:393", p["cat"] * p["H"] * p["W"], half)
    elif kind == "flip_pairs":
        add("N*C*H*W", "flip_pairs.hip:74", p["N"] * p["C"] * p["H"] * p["W"], half)
        add("blocks", "flip_pairs.hip:84", cdiv(p["N"] * p["C"] * p["H"] * (p["W"] // 4 if p["W"] % 4 == 0 else p["W"]), 256), half)
    else:
        pairs = kind == "head_points_pairs"
        n = p["N"]
        add("rows", "head_points.hip:260", n * (1 + p["J"]) * p["K"], half)
        add("map elements", "head_points.hip:260", (2 if pairs else 1) * n * p["H"] * p["W"] * (6 + 2 * p["J"]), 1 << (w + 8))
        if pairs:
            add("2*N*H", "head_points.hip:298", 2 * n * p["H"], half)
        if fixed:
            add("H*W", "head_points.hip:262", p["H"] * p["W"], half)
            if not pairs:
                add("B*H", "head_points.hip:262", n * p["H"], half)
    return out


def audit_tier2(kind, w=32, **p):
    q = []
    add = lambda name, where, ctype, lo_, hi: q.append(_q(name, where, ctype, lo_, hi, w))
    if kind == "decode":
        n = p["cat"] * p["H"] * p["W"]
        add("nbig = cat*H*W", "decode.hip:399", "int", n, n)
        add("flat index c0 + e", "decode.hip:234", "unsigned", 0, n - 1)
    elif kind == "flip_pairs":
        Wq = p["W"] // 4 if p["W"] % 4 == 0 else p["W"]
        n = p["N"] * p["C"] * p["H"] * Wq
        add("N*C*H*Wq", "flip_pairs.hip:28", "int", n, n)
        add("t", "flip_pairs.hip:27", "int", 0, cdiv(n, 256) * 256 - 1)
    else:
        pairs = kind == "head_points_pairs"
        add("HW = H*W", "head_points.hip:40", "int", p["H"] * p["W"], p["H"] * p["W"])
        add("(b*H + yy)", "head_points.hip:78", "int", -1, (2 if pairs else 1) * p["N"] * p["H"])
        add("B*J*K", "head_points.hip:266", "int", 0, p["N"] * p["J"] * p["K"])
    return q


# ======================================================================================================================================
# the judged set (shared by the device rows and by the 16-bit emulations)
# ======================================================================================================================================
def crossing(H, W, ld, w=32):
    """(image, row, column) of the first source pixel whose byte offset is >= 2^(w-1)"""
    p = cdiv(1 << (w - 1), ld * 4)
    return p // (H * W), (p % (H * W)) // W, p % W


def judged_crops(B, Ho, Wo, th, tw, cross_oy, ends_only=False):
    """the judged set in OUTPUT pixels, [(b, y0, y1, x0, x1)]: the first and last two tile rows of image 0; the tile rows of image 1 on either
    side of output row `cross_oy` (the row whose source pixel crosses byte 2^(w-1)); the first two tile rows of image 2; its last two tile
    rows and its last tile column; the final pixel (inside the last crop).  ends_only: only the two ends of the tensor."""
    assert B == 3
    two, lastrow = min(2 * th, Ho), max(0, (cdiv(Ho, th) - 2) * th)
    ends = [(0, 0, two, 0, Wo), (2, lastrow, Ho, 0, Wo)]
    if ends_only:
        return ends
    t = cross_oy // th
    crops = [ends[0], (0, lastrow, Ho, 0, Wo), (1, max(0, (t - 1) * th), min(Ho, (t + 2) * th), 0, Wo), (2, 0, two, 0, Wo), ends[1],
             (2, 0, Ho, (cdiv(Wo, tw) - 1) * tw, Wo)]
    assert any(b == B - 1 and y1 == Ho and x1 == Wo for b, _, y1, _, x1 in crops)        # the final pixel
    return crops


def in_crops(crops, shape_):
    """bool mask [B, Ho, Wo] of the judged set"""
    m = np.zeros(shape_, dtype=bool)
    for b, y0, y1, x0, x1 in crops:
        m[b, y0:y1, x0:x1] = True
    return m


# ======================================================================================================================================
# numpy emulations at word width w (teeth)
# ======================================================================================================================================
def _gather(mem, byte_off, ok):
    """float at 64-bit byte offset `byte_off` of the flat float32 `mem`; an address outside the tensor reads NaN (a fault or foreign data)"""
    idx = byte_off // 4
    inside = (idx >= 0) & (idx < mem.size) & (byte_off % 4 == 0)
    v = np.where(inside, mem[np.clip(idx, 0, mem.size - 1)], np.float32("nan"))
    return np.where(ok, v, np.float32(0))


def emulate_generic(x, wts, w=16, mutate=None, slot=4):
    """the generic NHWC producer (conv_igemm.hip:70-113) of a 3x3 / stride 1 / pad 1 convolution at word width w: x [B, H, W, ld] float32
    (all ld channels are the source), wts [3, 3, ld] -> out [B, H, W] (one output channel, float64 sums of the gathered float32 values).
    aoff = ((unsigned)(boff + iy*W + ix) * ld + q*4) * 4 wraps at w bits and is ZERO-extended onto the 64-bit base.
    mutate: "signed" -- the offset register is an int, sign-extended; "narrow_base" -- the image's byte base b*H*W*ld*4 is formed in a w-bit
    int of its own and added to a small in-image offset.
    slot: floats a staging thread owns -- 4: one float4 (the generic kernel; the split-bf16 kernel's quarter staging, BM = 64), 8: the
    split-bf16 kernel's half staging (conv_igemm_bf16x3.hip:189, 196-197): aoff carries q*8 and the second float4 is 16 bytes further on,
    added to the 64-bit pointer."""
    B, H, W, ld = x.shape
    mem = x.reshape(-1)
    b, oy, ox = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    out = np.zeros((B, H, W))
    for ky in range(3):
        for kx in range(3):
            iy, ix = oy - 1 + ky, ox - 1 + kx
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            for c in range(ld):
                qq, e = c // slot, c % slot
                if mutate == "narrow_base":
                    off = wrap(b * H * W * ld * 4, "int", w) + wrap(((iy * W + ix) * ld + qq * slot) * 4, "unsigned", w)
                else:
                    off = wrap(((b * H * W + iy * W + ix) * ld + qq * slot) * 4, "int" if mutate == "signed" else "unsigned", w)
                out += wts[ky, kx, c] * _gather(mem, np.where(ok, off, 0) + 4 * e, ok).astype(np.float64)
    return out


def emulate_dcn(x, w=16, field=None):
    """the DCN record (dcn.hip:84-114, 141-155) for ONE tap with the constant offset (+0.5, +0.5) and mask 1: every output is the mean of
    its pixel and the right / lower / diagonal neighbours that exist (the record's clamped base and its dx / dy flags).  x [B, H, W, ld]
    float32 -> out [B, H, W] (channel sum, float64).  field: bits of the record's offset field (default w - 4)."""
    B, H, W, ld = x.shape
    fb = field if field is not None else w - 4
    mem = x.reshape(-1)
    b, oy, ox = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    dyb, dxb = oy < H - 1, ox < W - 1                                              # t_ok && b_ok, l_ok && r_ok with h_low = oy, w_low = ox
    code = wrap((b * H * W + oy * W + ox) * (ld // 4), "unsigned", w) | (dxb.astype(np.int64) << (w - 3)) | (dyb.astype(np.int64) << (w - 2))
    pixb, rowb = wrap(ld * 4, "unsigned", w), wrap(W * ld * 4, "unsigned", w)
    out = np.zeros((B, H, W))
    for c in range(ld):
        o00 = wrap(((code & ((1 << fb) - 1)) << 4) + (c // 4) * 16, "unsigned", w)
        o01 = wrap(o00 + ((code >> (w - 3)) & 1) * pixb, "unsigned", w)
        o10 = wrap(o00 + ((code >> (w - 2)) & 1) * rowb, "unsigned", w)
        o11 = wrap(o10 + (o01 - o00), "unsigned", w)
        yes = np.ones_like(dxb)
        for off, wt in ((o00, 0.25), (o01, np.where(dxb, 0.25, 0.0)), (o10, np.where(dyb, 0.25, 0.0)), (o11, np.where(dxb & dyb, 0.25, 0.0))):
            out += wt * _gather(mem, off + 4 * (c % 4), yes).astype(np.float64)
    return out


def reference_generic(x, wts):
    xp = np.pad(x.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    B, H, W, _ = x.shape
    return sum((xp[:, ky:ky + H, kx:kx + W, :] * wts[ky, kx]).sum(-1) for ky in range(3) for kx in range(3))


def reference_dcn(x):
    B, H, W, _ = x.shape
    xs = np.pad(x.astype(np.float64).sum(-1), ((0, 0), (0, 1), (0, 1)))
    return 0.25 * (xs[:, :H, :W] + xs[:, :H, 1:] + xs[:, 1:, :W] + xs[:, 1:, 1:])


def judge_emulation(run, ref, x, th=2, tw=8, w=16, ends_only=False, translate=True):
    """the rule of `run_row` at the emulation's scale: -> dict(crops=bool, translation=bool): True = the result PASSES that check.
    run(x) -> [B, H, W]; ref(x) likewise (exact up to float64 rounding)."""
    B, H, W, ld = x.shape
    out, want = run(x), ref(x)
    mask = in_crops(judged_crops(B, H, W, th, tw, crossing(H, W, ld, w)[1], ends_only), out.shape)
    good = np.isclose(out, want, rtol=1e-9, atol=1e-9) & np.isfinite(out)
    res = dict(crops=bool(good[mask].all()))
    if translate:
        res["translation"] = all(np.array_equal(run(np.ascontiguousarray(x[i:i + 1]))[0], out[i]) for i in (2, 1))
    return res


# ======================================================================================================================================
# (b) the rows
# ======================================================================================================================================
Row = collections.namedtuple("Row", "id kind family audit kernel p")


def _r(id, kind, family, audit_, kernel, **p):
    d = dict(B=LIM_B, H=LIM_H, W=LIM_W, k=3, stride=1, pad=1, S=1, res=False, relu=True, tile=0, c0=0, th=8, tw=16, images=(2, 1))
    d.update(p)
    return Row(id, kind, family, audit_, kernel, d)


IG, DCN = L.IG, L.DCN
SB = "igemm_bf16x3_kernel<%d, %d>"
# cin channels from channel c0 of the 64-wide buffer; th x tw: the kernel's tile in output pixels (GEMM kernels: 8 rows of M tiles)
ROWS = [
    _r("ig-1x1", "conv", "direct", "generic", IG % "128, 32, 4, 1, 32, false", cin=32, c0=16, cout=20, k=1, pad=0, tile=128032, res=True),
    _r("ig-3x3-s1", "conv", "direct", "generic", IG % "64, 64, 2, 2, 32, false", cin=16, c0=48, cout=40, tile=64064),
    _r("ig-3x3-s2", "conv", "direct", "generic", IG % "256, 16, 4, 1, 16, false", cin=32, c0=32, cout=16, stride=2, tile=256016, res=True),
    _r("ig-split2", "conv", "direct", "generic", IG % "256, 16, 4, 1, 16, false", cin=32, c0=0, cout=16, tile=256016, S=2),
    _r("ig-cat2", "conv", "direct", "generic", IG % "256, 16, 4, 1, 16, false", cin=48, c0=0, cout=16, k=1, pad=0, tile=256016, cat=((0, 16), (32, 32))),
    _r("pw", "conv", "direct", "pw", "pw_conv_kernel<64, 64, 4>", cin=64, cout=36, k=1, pad=0, tile=1),
    _r("patch", "conv", "direct", "patch", "conv3x3_patch_kernel<16, 4, 1, 16>", cin=32, c0=16, cout=16, tile=3, res=True),
    _r("c16-s1", "conv", "direct", "c16", "conv3x3_c16_kernel<1, 1, 8, 32, 4, 2>", cin=16, c0=32, cout=16, tile=16, res=True, tw=32),
    _r("c16-s2", "conv", "direct", "c16", "conv3x3_c16_kernel<2, 2, 8, 16, 3, 1>", cin=16, c0=16, cout=32, stride=2, tile=16, res=True),
    _r("wino", "wino", "wino", "wino", "conv3x3_wino_kernel<1, 1, 16, 2>", cin=32, c0=32, cout=24, tile=11, res=True),
    _r("wino-vs64", "wino", "wino", "wino_vs64", "conv3x3_wino_vs64_kernel<0, 0>", cin=64, cout=40, tile=6402),
    _r("wino24", "wino", "wino24", "wino24", "conv3x3_wino24_kernel<true>", cin=32, c0=16, cout=24, tile=24, res=True, th=16),
    _r("head-wino-n2", "head", "wino", "head_wino", "conv3x3_wino_vs64_kernel<2, 0>", cin=64, hc=32, cout=2, sigmoid=False, wino24=False),
    _r("head-wino24-n1", "head", "wino24", "head_wino24", "head_wino24_kernel<1, 0>", cin=64, hc=32, cout=1, sigmoid=True, wino24=True, th=16),
    _r("dcn-split3", "dcn", "dcn", "dcn", DCN % "64, 32, 4, 1, 16", cin=32, c0=0, cout=16, tile=64032, S=3, om_sigmoid=False, om_c0=32),
    _r("dcn-sigmoid", "dcn", "dcn", "dcn", DCN % "128, 32, 4, 1, 32", cin=32, c0=32, cout=24, tile=128032, om_sigmoid=True),
    # group launches: member 0 at LIM, member 1 small (B = 2, 19 x 37); the translation runs repeat the launch with image 2 / image 1 of member 0 alone
    _r("group-igemm", "group", "direct", "group", "igemm_conv_group_kernel", cin=16, c0=16, cout=40),
    _r("group-wino24", "group24", "wino24", "wino24", "conv3x3_wino24_group_kernel<true>", cin=32, c0=0, cout=24, th=16),
    # the split-bf16 kernel (opt-in), forced with split_bf16=True and CP_SPLIT_BF16_TILE = `sb`: half staging (BM = 128) and quarter staging
    # (BM = 64).  res_host: source + output + residual at 48 physical channels leave no room under MEM_LIMIT for a stand-alone image beside
    # them, so the residual of the translated images waits on the host while those run
    _r("sb-3x3-s1", "conv", "direct", "bf16x3", SB % (128, 64), cin=16, c0=48, cout=40, sb="128x64"),
    _r("sb-1x1", "conv", "direct", "bf16x3", SB % (64, 64), cin=32, c0=16, cout=40, k=1, pad=0, sb="64x64", res=True, res_host=True),
]
ROW = {r.id: r for r in ROWS}
assert len(ROW) == len(ROWS)

# Not run at LIM ("At the offset limits"): the NCHW stems.  The last shape B*3*H*W < 2^31 accepts at B = 3 is an 8 GiB input, and
# the narrowest output any stem kernel writes for it (16 channels at stride 2) another 10.7 GiB: over MEM_LIMIT.  `audit("stem7*")` and
# `audit("generic_stem")` cover them on the CPU.
STEM_LIM = dict(B=3, H=4098, W=58224)         # W % 4 == 0 (persistent kernel): four more columns are past 2^31 floats; ragged against 8 x 64 tiles
STEM_LIM_SCALAR = dict(B=3, H=4098, W=58225)  # W % 4 != 0 (stem7x7_kernel): one more column is past 2^31 floats


def _index(row):
    return [r.id for r in ROWS].index(row.id)


def row_shape(row, B=None):
    """the `shape` of a row's (LIM member's) launch for `checks` / `audit`"""
    p = row.p
    cp = p["cout"] if row.kind == "head" else cdiv(p["cout"], 16) * 16
    ldw = 64 if row.kind in ("group", "head") else max(_ldw(p["cout"]), 32) if row.kind == "dcn" else _ldw(p["cout"])
    lds = [LIM_LD] * len(p["cat"]) if p.get("cat") else None
    k = 3 if row.kind in ("group", "group24", "head", "dcn", "wino") else p["k"]
    pad = 1 if k == 3 else p["pad"]
    extra = dict(ngroups=2) if row.audit == "wino_vs64" else {}
    s = shape(B or p["B"], p["H"], p["W"], LIM_LD, p["cin"], k, p["stride"], pad, p.get("hc", cp), ldw, cp + 4 if row.kind != "head" else p["hc"],
              cp + 4 if p["res"] else 0, p["S"], lds)
    s.update(extra)
    return s


def _ldw(cout):
    return 16 if cout <= 16 else 32 if cout <= 32 else cdiv(cout, 64) * 64


def row_tile(row):
    """(BM, BN) of the row's GEMM instantiation, from its kernel name"""
    if "<" in row.kernel and row.kernel.split("<")[0] in ("igemm_conv_kernel", "dcn_igemm_kernel", "igemm_bf16x3_kernel"):
        a = row.kernel.rstrip(">").split("<")[1].split(",")
        return int(a[0]), int(a[1])
    return (64, 64)


# ======================================================================================================================================
# (c) device: build, run, judge
# ======================================================================================================================================
def _weights(row):
    """the row's parameters (CPU, float32), fixed by seed, under the key names of launch_oracle.evaluate"""
    p = row.p
    g = torch.Generator().manual_seed(7000 + _index(row))
    r = lambda *s: torch.randn(*s, generator=g)
    u01 = lambda n: torch.rand(n, generator=g)
    ci, co = p["cin"], p["cout"]
    k = 3 if row.kind in ("group", "group24", "head", "dcn", "wino") else p["k"]
    bn = lambda n: {"b.weight": u01(n) + 0.5, "b.bias": r(n) * 0.1, "b.running_mean": r(n) * 0.1, "b.running_var": u01(n) + 0.5}
    if row.kind == "head":
        hc = p["hc"]
        return {"h.0.weight": r(hc, ci, 3, 3) * (2.0 / (9 * ci)) ** 0.5 * lo.spread_factors(hc).view(-1, 1, 1, 1), "h.0.bias": r(hc) * 0.1,
                "h.2.weight": r(co, hc, 1, 1) * (2.0 / hc) ** 0.5 * lo.spread_factors(co).view(-1, 1, 1, 1),
                "h.2.bias": torch.full((co,), L.SIGMOID_BIAS) if p["sigmoid"] else r(co) * 0.1}
    if row.kind == "dcn":
        return lo.spread_bn(dict(bn(co), **{"d.weight": r(co, ci, 3, 3) * (4.0 / (9 * ci)) ** 0.5, "d.bias": r(co) * 0.1}))
    return lo.spread_bn(dict(bn(co), **{"c.weight": r(co, ci, k, k) * (2.0 / (k * k * ci)) ** 0.5}))


class _Flat:
    """NaN-filled flat buffer with G guard floats before and after an NHWC view [B, H, W, ld] (ld > c: NaN guard channels behind every
    pixel as well); `view` = the c channels a launch is given"""
    G = 256

    def __init__(self, B, H, W, c, nchw=False):
        self.ld = c if nchw else cdiv(c, 4) * 4 + 4
        self.n = B * H * W * self.ld
        self.flat = _alloc(lambda: torch.full((self.n + 2 * self.G,), float("nan"), device="cuda"), (self.n + 2 * self.G) * 4, "output")
        body = self.flat[self.G:self.G + self.n]
        self.c, self.nchw = c, nchw
        self.full = body.view(B, c, H, W) if nchw else body.view(B, H, W, self.ld)
        self.view = self.full if nchw else self.full[..., :c]

    def guards_intact(self):
        ok = bool(torch.isnan(self.flat[:self.G]).all()) and bool(torch.isnan(self.flat[self.G + self.n:]).all())
        return ok and (self.nchw or bool(torch.isnan(self.full[..., self.c:]).all()))


def _alloc(make, nbytes, what):
    """no skip for lack of memory: a row that cannot allocate fails with the sizes in the message"""
    try:
        return make()
    except RuntimeError as e:
        raise AssertionError("cannot allocate %.2f GiB for %s with %.2f GiB already held (limit per row %.0f GiB): %s" %
                             (nbytes / 2 ** 30, what, torch.cuda.memory_allocated() / 2 ** 30, MEM_LIMIT / 2 ** 30, e)) from None


def _source(row, B, seed):
    """the 64-wide post-ReLU source buffer [B, H, W, 64], generated on the device"""
    p = row.p
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = B * p["H"] * p["W"] * LIM_LD
    buf = _alloc(lambda: torch.empty(B, p["H"], p["W"], LIM_LD, device="cuda"), n * 4, "source")
    buf.normal_(generator=g).relu_()
    return buf


def _residual(B, Ho, Wo, co, cp, seed):
    """post-ReLU residual [B, Ho, Wo, cp] (padding channels zero) inside a buffer of cp + 4 floats per pixel"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    buf = _alloc(lambda: torch.empty(B, Ho, Wo, cp + 4, device="cuda"), B * Ho * Wo * (cp + 4) * 4, "residual")
    buf.normal_(generator=g).relu_()
    buf[..., co:] = 0
    return buf[..., :cp]


def _om(row, B, src, seed):
    """DCN offsets bounded by +-2 px and mask logits; `om_c0`: inside channels om_c0 .. om_c0 + 26 of the source buffer itself (ld 64), else
    a tensor of its own with 32 floats per pixel.  om_sigmoid False: the mask channels hold sigmoid(logits)."""
    p = row.p
    g = torch.Generator(device="cuda").manual_seed(seed)
    if p.get("om_c0") is not None:
        om = src[..., p["om_c0"]:p["om_c0"] + 27]
    else:
        om = _alloc(lambda: torch.zeros(B, p["H"], p["W"], 32, device="cuda"), B * p["H"] * p["W"] * 128, "offsets")[..., :27]
    for c in range(27):                                   # channel by channel: no temporary of the whole tensor
        t = torch.empty(B, p["H"], p["W"], device="cuda").normal_(generator=g)
        om[..., c] = (t * 1.5) if c >= 18 else t.clamp_(-2.0, 2.0)
    if not p["om_sigmoid"]:
        om[..., 18:27] = torch.sigmoid(om[..., 18:27])
    return om


_SMALL = dict(B=2, H=19, W=37)


class Built:
    """one row on the device: the LIM launch with its data generated in place (parent None), or image `image` of `parent` ALONE, copied
    to fresh buffers, under the same forced variant"""

    def __init__(self, row, sd, parent=None, image=None):
        from centerpose_amd import ops
        p = row.p
        self.row, self.sd = row, sd
        self.res_host = None                                               # {image: CPU residual}, once `run_row` has let the device buffer go
        B = p["B"] if parent is None else 1
        H, W, co = p["H"], p["W"], p["cout"]
        k = 3 if row.kind in ("group", "group24", "head", "dcn", "wino") else p["k"]
        pad = 1 if k == 3 else p["pad"]
        st = p["stride"]
        Ho, Wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
        self.B, self.Ho, self.Wo, self.k, self.pad = B, Ho, Wo, k, pad
        cp = co if row.kind == "head" else cdiv(co, 16) * 16
        self.cp = cp
        seed = 9000 + 10 * _index(row)
        if parent is None:
            self.src = _source(row, B, seed)
            self.res = _residual(B, Ho, Wo, co, cp, seed + 1) if p["res"] else None
            self.om = _om(row, B, self.src, seed + 2) if row.kind == "dcn" else None
        else:                                                              # the image ALONE, in fresh buffers: every offset is small
            self.src = parent.src[image:image + 1].clone()
            self.res = None
            if parent.res is not None or parent.res_host:
                rb = parent.res_host[image] if parent.res is None else parent.res[image:image + 1]
                self.res = torch.zeros(1, Ho, Wo, cp + 4, device="cuda")[..., :cp]
                self.res.copy_(rb)
            self.om = None
            if parent.om is not None:
                if p.get("om_c0") is not None:
                    self.om = self.src[..., p["om_c0"]:p["om_c0"] + 27]
                else:
                    self.om = torch.zeros(1, H, W, 32, device="cuda")[..., :27]
                    self.om.copy_(parent.om[image:image + 1])
        dev = lambda t: t.cuda()
        relu = ops.ACT_RELU if p["relu"] else ops.ACT_NONE
        x = self.src[..., p["c0"]:p["c0"] + p["cin"]]
        self.x = x
        if row.kind == "head":
            hc = p["hc"]
            self.out = _Flat(B, H, W, co, nchw=True)
            wp3 = ops.pack_conv_weight(dev(sd["h.0.weight"]))
            u = (ops.pack_wino24_weight if p["wino24"] else ops.pack_wino_weight)(wp3, 64, hc)
            sc, sh = ops.fold_bn(hc, None, dev(sd["h.0.bias"]))
            self.launches = [ops.head3x3_1x1_launch(x, u, sc, sh, dev(sd["h.2.weight"].reshape(co, hc).contiguous()), dev(sd["h.2.bias"]),
                                                    self.out.view, hc=hc, act2=ops.ACT_SIGMOID if p["sigmoid"] else ops.ACT_NONE, wino24=p["wino24"])]
            return
        self.out = _Flat(B, Ho, Wo, cp)
        out = self.out.view
        bnp = tuple(dev(sd["b." + s]) for s in ("weight", "bias", "running_mean", "running_var"))
        S = p["S"]
        if row.kind == "dcn":
            wp = ops.pack_conv_weight(dev(sd["d.weight"]))
            sc, sh = ops.fold_bn(co, bnp, dev(sd["d.bias"]))
            bn_ = row_tile(row)[1]                           # no DCN tile is narrower than 32 channels: zero rows up to the N tile
            if wp.shape[0] % bn_:
                wp, sc, sh = ops.pad_rows(wp, bn_), ops.pad_vec(sc, bn_), ops.pad_vec(sh, bn_)
            if S == 1:
                self.launches = [ops.dcn_v2_launch(x, self.om, wp, sc, sh, out, cout=cp, om_sigmoid=p["om_sigmoid"], act=relu, tile=p["tile"])]
                return
            ldw = wp.shape[0]
            ws = _alloc(lambda: torch.full((S, B * Ho * Wo, ldw), float("nan"), device="cuda"), S * B * Ho * Wo * ldw * 4, "split-K workspace")
            la = ops.dcn_v2_launch(x, self.om, wp, torch.ones(ldw, device="cuda"), torch.zeros(ldw, device="cuda"), ws, cout=ldw,
                                   om_sigmoid=p["om_sigmoid"], tile=p["tile"], ksplit=S)
            self.launches = [la, ops.splitk_reduce_launch(ws, sc, sh, out, cout=cp, act=relu)]
            return
        if row.kind in ("group", "group24"):
            self._build_group(ops, x, out, bnp, relu)
            return
        wp = ops.pack_conv_weight(dev(sd["c.weight"]))
        sc, sh = ops.fold_bn(co, bnp)
        srcs = [self.src[..., a:a + n] for a, n in p["cat"]] if p.get("cat") else [x]
        kw = dict(kh=k, kw=k, stride=st, pad=pad, tile=p["tile"])
        if p.get("sb"):
            self.launches = [_forced_sb(p["sb"], lambda: ops.conv2d_launch(srcs, wp, sc, sh, out, cout=cp, act=relu, res=self.res, split_bf16=True, **kw))]
            return
        u = None
        if row.kind == "wino":
            u = (ops.pack_wino24_weight if row.family == "wino24" else ops.pack_wino_weight)(wp, p["cin"], cp)
        if S == 1:
            self.launches = [ops.conv2d_launch(srcs, wp, sc, sh, out, cout=cp, act=relu, res=self.res, wino=u, split_bf16=False, **kw)]
            return
        ld = wp.shape[0]
        ws = _alloc(lambda: torch.full((S, B * Ho * Wo, ld), float("nan"), device="cuda"), S * B * Ho * Wo * ld * 4, "split-K workspace")
        n = sc.numel()
        la = ops.conv2d_launch(srcs, wp, torch.ones(n, device="cuda"), torch.zeros(n, device="cuda"), ws, cout=ld, ksplit=S, split_bf16=False, **kw)
        self.launches = [la, ops.splitk_reduce_launch(ws, sc, sh, out, cout=cp, act=relu)]

    def _build_group(self, ops, x, out, bnp, relu):
        """member 0: the LIM tensor; member 1: a small convolution of its own (B = 2, 19 x 37), judged whole against float64"""
        row, sd, p, co, cp = self.row, self.sd, self.row.p, self.row.p["cout"], self.cp
        g = torch.Generator().manual_seed(8000 + _index(row))
        ci2, co2 = 32, 40
        self.small_x = F.relu(torch.randn(_SMALL["B"], ci2, _SMALL["H"], _SMALL["W"], generator=g))
        self.small_sd = lo.spread_bn({"b.weight": torch.rand(co2, generator=g) + 0.5, "b.bias": torch.randn(co2, generator=g) * 0.1,
                                      "b.running_mean": torch.randn(co2, generator=g) * 0.1, "b.running_var": torch.rand(co2, generator=g) + 0.5,
                                      "c.weight": torch.randn(co2, ci2, 3, 3, generator=g) * (2.0 / (9 * ci2)) ** 0.5})
        whole = self.out.flat
        cp2 = cdiv(co2, 16) * 16
        self.small_out = torch.full((_SMALL["B"], _SMALL["H"], _SMALL["W"], cp2 + 4), float("nan"), device="cuda")
        # one storage for both outputs is what the dependency tracking wants; the C entry point takes the members' own pointers
        members = []
        for xx, s_, oo, c_o, c_p in ((x, sd, out, co, cp), (L._nhwc(self.small_x), self.small_sd, self.small_out[..., :cp2], co2, cp2)):
            wp = ops.pack_conv_weight(s_["c.weight"].cuda())
            b_ = tuple(s_["b." + n].cuda() for n in ("weight", "bias", "running_mean", "running_var"))
            sc, sh = ops.fold_bn(c_o, b_)
            if row.kind == "group":
                wp, sc, sh = ops.pad_rows(wp, 64), ops.pad_vec(sc, 64), ops.pad_vec(sh, 64)
                members.append(dict(x=xx, wp=wp, scale=sc, shift=sh, out=oo, cout=c_p, k=3, stride=1, pad=1, act=relu, res=None))
            else:
                members.append(dict(x=xx, wp=wp, u24=ops.pack_wino24_weight(wp, xx.shape[3], c_p), scale=sc, shift=sh, out=oo, cout=c_p, act=relu, res=None))
        self.launches = [_group_launch(ops, row.kind, members)]

    def run(self):
        for la in self.launches:
            la.run()
        torch.cuda.synchronize()

    def out_nhwc(self):
        """the physical output as [B, Ho, Wo, c] (heads: a permuted view of the NCHW map)"""
        return self.out.view.permute(0, 2, 3, 1) if self.out.nchw else self.out.view


def _forced_sb(tile, make):
    """make() with CP_SPLIT_BF16_TILE = tile: ops.split_bf16_tile reads the switch when the launch is BUILT"""
    import os
    saved = os.environ.get("CP_SPLIT_BF16_TILE")
    os.environ["CP_SPLIT_BF16_TILE"] = tile
    try:
        return make()
    finally:
        if saved is None:
            del os.environ["CP_SPLIT_BF16_TILE"]
        else:
            os.environ["CP_SPLIT_BF16_TILE"] = saved


def _group_launch(ops, kind, members):
    """ops.conv2d_group_launch / conv3x3_group_launch without their one-storage assertion (the members here own separate buffers)"""
    import ctypes
    n = len(members)
    if kind == "group":
        d, width, fn = ops.ConvDesc8(), 8, "cp_conv2d_group_f32"
        members = sorted(members, key=lambda mm: -mm["wp"].shape[1])
    else:
        d, width, fn = ops.ConvDesc4(), 4, "cp_conv3x3_winograd24_group_f32"
        members = sorted(members, key=lambda mm: -mm["x"].shape[3])
    cols = [[None] * width for _ in range(6)]
    for i, mm in enumerate(members):
        if kind == "group":
            one = ops.conv2d_launch([mm["x"]], mm["wp"], mm["scale"], mm["shift"], mm["out"], kh=3, kw=3, stride=1, pad=1, cout=mm["cout"],
                                    act=mm["act"], res=None, split_bf16=False)
            ts = (mm["x"], mm["wp"], mm["scale"], mm["shift"], None, mm["out"])
        else:
            one = ops.conv2d_launch([mm["x"]], mm["wp"], mm["scale"], mm["shift"], mm["out"], kh=3, kw=3, stride=1, pad=1, cout=mm["cout"],
                                    act=mm["act"], res=None, wino=mm["u24"], tile=ops.WINO24)
            ts = (mm["x"], mm["u24"], mm["scale"], mm["shift"], None, mm["out"])
        ctypes.memmove(ctypes.addressof(d[i]), ctypes.addressof(one.desc), ctypes.sizeof(ops.ConvDesc))
        for kk, t in enumerate(ts):
            cols[kk][i] = t
    return ops.Launch(fn, d, [t for col in cols for t in col] + [members[0]["out"]], [n])


def _crop_reference(built, crop, E=4, D=4):
    """float64 reference of output window `crop` = (b, y0, y1, x0, x1) from a host crop of the device inputs that holds the receptive field
    of the window grown by E outputs (the Winograd tile_A neighbourhood) and, for DCN, by D more input pixels (offsets of +-2 px and the
    bilinear corner).  Only the window itself is judged: its receptive fields lie inside the crop or outside the image.
    -> (device values, reference, tile_A, K) of the window, logical channels, [co, y1 - y0, x1 - x0]"""
    row, p = built.row, built.row.p
    b, y0, y1, x0, x1 = crop
    st, k, pad, H, W = p["stride"], built.k, built.pad, p["H"], p["W"]
    D = D if row.kind == "dcn" else 0
    ey0, ey1, ex0, ex1 = max(0, y0 - E), min(built.Ho, y1 + E), max(0, x0 - E), min(built.Wo, x1 + E)
    iy0, ix0 = max(0, ey0 * st - pad - D) // st * st, max(0, ex0 * st - pad - D) // st * st
    iy1, ix1 = min(H, (ey1 - 1) * st - pad + k + D), min(W, (ex1 - 1) * st - pad + k + D)
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous().cpu()
    if p.get("cat"):
        xc = torch.cat([nchw(built.src[b:b + 1, iy0:iy1, ix0:ix1, a:a + n]) for a, n in p["cat"]], 1)
    else:
        xc = nchw(built.x[b:b + 1, iy0:iy1, ix0:ix1])
    hc_, wc_ = iy1 - iy0, ix1 - ix0
    nj, ni = (hc_ + 2 * pad - k) // st + 1, (wc_ + 2 * pad - k) // st + 1
    oy, ox = iy0 // st, ix0 // st                              # output pixel of the crop's own output (0, 0)
    res = om = None
    if built.res is not None:
        res = nchw(built.res[b:b + 1, oy:oy + nj, ox:ox + ni, :p["cout"]])
    if row.kind == "dcn":
        om = nchw(built.om[b:b + 1, iy0:iy1, ix0:ix1]).double()
        if not p["om_sigmoid"]:                                # the reference takes logits: those of exactly the masks the device was given
            m = om[:, 18:27]
            om[:, 18:27] = torch.log(m) - torch.log1p(-m)
    kind = "conv" if row.kind in ("group", "group24") else row.kind
    pp = dict(p, k=k, pad=pad, relu=p["relu"])
    case = L.Case(row._replace(kind=kind), pp, built.sd, xc, res, om, nj, ni, built.cp)
    if row.kind == "dcn":
        o64 = lo.dcn_stage(built.sd, xc.double(), om, "d", "b", p["cout"], torch.float64, extent=max(H, W))
    else:
        o64 = L.evaluate(case, torch.float64)
    A = lo.tile_A(o64.A, row.family)
    sl = (0, slice(None), slice(y0 - oy, y1 - oy), slice(x0 - ox, x1 - ox))
    dev = built.out_nhwc()[b, y0:y1, x0:x1, :p["cout"]].permute(2, 0, 1).contiguous().cpu()
    return dev, o64.val[sl], A[sl], o64.K


def run_row(rid):
    """Build row `rid` at LIM, run it, judge it both ways and free it.  -> dict(kernels, worst (lo.Worst), c, translation {image: bool},
    failures [text], peak (bytes), seconds)"""
    row = ROW[rid]
    p = row.p
    t0 = time.time()
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    held_before = torch.cuda.memory_allocated()          # what earlier tests of the same process still hold is not this row's
    fails, worst, trans = [], None, {}
    sd = _weights(row)
    with torch.no_grad():
        big = Built(row, sd)
        big.run()
        kernels = [la.kernel for la in big.launches]
        # guards, padding channels
        if not big.out.guards_intact():
            fails.append("stored outside the %d channels the launch was given (NaN guard overwritten)" % big.cp)
        if not big.out.nchw and big.cp > p["cout"] and not bool((big.out.view[..., p["cout"]:] == 0).all()):
            fails.append("padding channel not zero")
        if bool(torch.isnan(big.out.view).any()):
            fails.append("NaN inside the output view")
        # the same bits from a second run, one image at a time (a whole second copy would not fit MEM_LIMIT)
        for b in range(big.B):
            snap = big.out.view[b].clone()
            big.run()
            if not torch.equal(big.out.view[b], snap):
                fails.append("a second run gives other bits in image %d" % b)
            del snap
        # crops against float64
        cy = crossing(p["H"], p["W"], LIM_LD)
        assert cy[0] == 1
        c = None
        for crop in judged_crops(big.B, big.Ho, big.Wo, p["th"], p["tw"], cy[1] // p["stride"]):
            dev, ref, A, K = _crop_reference(big, crop)
            w = lo.worst_ratio(dev, ref, A)
            c = lo.c_for(row.family, K)
            if worst is None or w.ratio > worst.ratio:
                worst = w._replace(loc=(crop[0], w.loc[0], w.loc[1] + crop[1], w.loc[2] + crop[3]))
            if not w.ratio <= c:
                fails.append("crop %s: err %.3e = %.1f u A (A = %.3e) > c = %.1f at (c, y, x) = %s" % (crop, w.err, w.ratio, w.A, c, w.loc))
        if row.kind in ("group", "group24"):
            fails += _judge_small(big)
        # translation: the image alone, bit for bit
        big.launches = None                                                    # a split-K workspace goes before the stand-alone launches
        if p.get("res_host"):
            big.res_host = {img: big.res[img:img + 1].cpu() for img in p["images"]}
            big.res = None                                                     # the device copy goes; Built takes the image from the host
        torch.cuda.empty_cache()
        for img in p["images"]:
            one = Built(row, sd, parent=big, image=img)
            one.run()
            if [la.kernel for la in one.launches] != kernels:
                fails.append("image %d alone dispatched to %s" % (img, [la.kernel for la in one.launches]))
            trans[img] = torch.equal(one.out.view, big.out.view[img:img + 1])
            if not trans[img]:
                loc = lo.first_unequal(one.out.view.cpu(), big.out.view[img:img + 1].cpu())
                fails.append("image %d of the LIM launch differs from the same image run alone, first at %s" % (img, loc))
            if not one.out.guards_intact():
                fails.append("image %d alone: NaN guard overwritten" % img)
            del one
            torch.cuda.empty_cache()
        peak = torch.cuda.max_memory_allocated() - held_before
        del big
        torch.cuda.empty_cache()
    if peak > MEM_LIMIT:
        fails.append("the row held %.2f GiB at once (limit %.0f GiB)" % (peak / 2 ** 30, MEM_LIMIT / 2 ** 30))
    return dict(kernels=kernels, worst=worst, c=c, translation=trans, failures=fails, peak=peak, seconds=time.time() - t0)


def _judge_small(big):
    """the small member of a group launch, whole, against float64"""
    co2 = big.small_sd["c.weight"].shape[0]
    case = L.Case(big.row._replace(kind="conv"), dict(k=3, stride=1, pad=1, relu=True, cout=co2), big.small_sd, big.small_x, None, None,
                  _SMALL["H"], _SMALL["W"], cdiv(co2, 16) * 16)
    o64 = L.evaluate(case, torch.float64)
    got = big.small_out[..., :co2].permute(0, 3, 1, 2).contiguous().cpu()
    w, fail = lo.judge(got, None, o64, big.row.family)
    out = ["small member: " + fail] if fail else []
    if not bool(torch.isnan(big.small_out[..., cdiv(co2, 16) * 16:]).all()):
        out.append("small member: NaN guard overwritten")
    return out


def format_row(rid, rep):
    w = rep["worst"]
    tr = ", ".join("image %d %s" % (i, "bit-equal" if ok else "DIFFERS") for i, ok in sorted(rep["translation"].items()))
    return "%-15s %-46s worst err / (u A) %7.3f (c = %5.1f) at %-22s translation: %-36s peak %5.2f GiB  %5.1f s" % (
        rid, " + ".join(rep["kernels"]), w.ratio, rep["c"], w.loc, tr, rep["peak"] / 2 ** 30, rep["seconds"])


# ======================================================================================================================================
# refusals: the first refused shape of every launcher, through the C ABI
# ======================================================================================================================================
Refusal = collections.namedtuple("Refusal", "id launcher arg call backed")      # backed: bytes of real buffers the call can be given on a device


def _conv_desc(ops, B, H, W, ld=LIM_LD, C=16, k=1, nchw=False, Ho=None, Wo=None):
    d = ops.ConvDesc()
    d.nsrc, d.B, d.H, d.W = 1, B, H, W
    d.srcC[0], d.srcLd[0] = C, (0 if nchw else ld)
    d.Ho, d.Wo = Ho or H, Wo or W
    d.kh = d.kw = k
    d.sy = d.sx = 1
    d.py = d.px = k // 2
    d.K, d.ldw, d.Cout = cdiv(k * k * C, 16) * 16, 64, 16
    d.resLd, d.outLd, d.outNCHW = 0, 16, 0
    d.OH, d.OW, d.osy, d.osx, d.ooy, d.oox = d.Ho, d.Wo, 1, 1, 0, 0
    d.act, d.inNCHW, d.tile, d.nsub, d.ksplit = 0, 1 if nchw else 0, 0, 1, 0
    return d


def _refusals():
    import ctypes
    from centerpose_amd import ops
    vp, c_int = ctypes.c_void_p, ctypes.c_int
    S = vp(0)
    out = []
    add = lambda id, launcher, arg, call, backed=0: out.append(Refusal(id, launcher, arg, call, backed))
    SMALL = 1 << 12                                                       # floats of an operand that is small whatever the shape
    P24 = 1 << 24                                                         # exactly 2^24 pixels at ld = 64: 4 GiB, the first refused source
    arr = lambda ptrs, n: (vp * n)(*[p.value for p in ptrs] + [None] * (n - len(ptrs)))
    byref = ctypes.byref

    def conv(d):
        return lambda Lb, P: Lb.cp_conv2d_f32(byref(d), arr([P(d.B * d.H * d.W * max(d.srcLd[0], d.srcC[0]))], 4), P(SMALL), P(SMALL), P(SMALL),
                                              vp(0), P(d.B * d.Ho * d.Wo * 16), S)
    add("conv2d-bytes", "conv2d", "source 0 exceeds 32-bit byte offsets", conv(_conv_desc(ops, 1, 4096, 4096)), backed=6 << 30)
    add("conv2d-columns", "conv2d", "source 0 exceeds 32-bit byte offsets", conv(_conv_desc(ops, LIM_B, LIM_H, LIM_W + 1)))
    add("conv2d-nchw", "conv2d", "NCHW source of B*C*H*W=4294980150", conv(_conv_desc(ops, 2, 26755, 26755, C=3, k=3, nchw=True)))
    add("conv2d-nchw-first", "conv2d", "NCHW source of B*C*H*W=2147483648", conv(_conv_desc(ops, 2, 32768, 8192, C=4, k=3, nchw=True)))
    add("conv2d-rows", "conv2d", "output pixels exceed the 32-bit row index", conv(_conv_desc(ops, 1, 1, 1 << 20, ld=16, Ho=2048, Wo=1 << 20)))
    dw = _conv_desc(ops, 1, 4096, 4096, C=32, k=3)
    add("winograd-bytes", "conv2d", "source 0 exceeds",
        lambda Lb, P: Lb.cp_conv3x3_winograd_f32(byref(dw), P(P24 * 64), P(SMALL), P(SMALL), P(SMALL), vp(0), P(P24 * 16), S), backed=6 << 30)
    dh = _conv_desc(ops, 1, 4096, 4096, C=64, k=3)
    dh.Cout, dh.ldw, dh.act = 32, 64, 1
    add("head-bytes", "conv2d", "source 0 exceeds",
        lambda Lb, P: Lb.cp_head3x3_1x1_f32(byref(dh), P(P24 * 64), P(SMALL), P(SMALL), P(SMALL), P(SMALL), P(SMALL), P(P24), 1, 32, 0, S), backed=5 << 30)
    d8, one8 = ops.ConvDesc8(), _conv_desc(ops, 1, 4096, 4096, C=16, k=3)
    ctypes.memmove(ctypes.addressof(d8[0]), ctypes.addressof(one8), ctypes.sizeof(ops.ConvDesc))
    add("group-bytes", "conv2d", "source 0 exceeds",
        lambda Lb, P: Lb.cp_conv2d_group_f32(d8, 1, arr([P(P24 * 64)], 8), arr([P(SMALL)], 8), arr([P(SMALL)], 8), arr([P(SMALL)], 8), arr([], 8),
                                             arr([P(P24 * 16)], 8), S), backed=6 << 30)
    d4, one4 = ops.ConvDesc4(), _conv_desc(ops, 1, 4096, 4096, C=32, k=3)
    ctypes.memmove(ctypes.addressof(d4[0]), ctypes.addressof(one4), ctypes.sizeof(ops.ConvDesc))
    d4[0].tile = 24
    add("group24-bytes", "conv2d", "source 0 exceeds",
        lambda Lb, P: Lb.cp_conv3x3_winograd24_group_f32(d4, 1, arr([P(P24 * 64)], 4), arr([P(SMALL)], 4), arr([P(SMALL)], 4), arr([P(SMALL)], 4),
                                                         arr([], 4), arr([P(P24 * 16)], 4), S), backed=6 << 30)
    # grid x dmax >= 2^32 behind the byte check: one row of 16 * 65535 + 1 pixels is 65536 tile columns.  Every single launcher but launch_wino reserves
    # its LDS before it looks at the grid, so these come back with rc 1 only where a device is present (`backed`, DEVICE_ONLY)
    WG = 16 * 65535 + 1

    def wide(C, tile, cout=32):
        d = _conv_desc(ops, 1, 1, WG, ld=C, C=C, k=3)
        d.tile, d.Cout, d.ldw, d.outLd = tile, cout, cdiv(cout, 64) * 64, cout
        return d
    dg11, dg64, dg24, dgh = wide(32, 11), wide(64, 6401, 128), wide(32, 24), wide(64, 0)
    dgh.act, dgh24 = 1, wide(64, 24)
    dgh24.act = 1
    wino = lambda d: (lambda Lb, P: Lb.cp_conv3x3_winograd_f32(byref(d), P(WG * d.srcLd[0]), P(1 << 20), P(SMALL), P(SMALL), vp(0), P(WG * d.Cout), S))
    head = lambda d: (lambda Lb, P: Lb.cp_head3x3_1x1_f32(byref(d), P(WG * 64), P(1 << 20), P(SMALL), P(SMALL), P(SMALL), P(SMALL), P(WG), 1, 32, 0, S))
    add("winograd-grid", "conv3x3_winograd", "grid 65536 too large", wino(dg11), backed=1 << 30)
    add("winograd-vs64-grid", "conv3x3_winograd", "grid 65536 too large", wino(dg64), backed=1 << 30)
    add("winograd24-grid", "conv3x3_winograd24", "grid 65536 too large", wino(dg24), backed=1 << 30)
    add("head-grid", "conv3x3_winograd", "grid 65536 too large", head(dgh), backed=1 << 30)
    add("head24-grid", "head_wino24", "grid 65536 too large", head(dgh24), backed=1 << 30)
    dg4 = ops.ConvDesc4()
    ctypes.memmove(ctypes.addressof(dg4[0]), ctypes.addressof(dg24), ctypes.sizeof(ops.ConvDesc))
    add("group24-grid", "conv3x3_winograd24_group", "member 0 too large",
        lambda Lb, P: Lb.cp_conv3x3_winograd24_group_f32(dg4, 1, arr([P(WG * 32)], 4), arr([P(1 << 20)], 4), arr([P(SMALL)], 4), arr([P(SMALL)], 4),
                                                         arr([], 4), arr([P(WG * 32)], 4), S), backed=1 << 30)

    def dcn(B, H, W, ld):
        d = ops.DcnDesc()
        d.B, d.H, d.W, d.C, d.srcLd, d.Ho, d.Wo = B, H, W, 16, ld, H, W
        d.kh = d.kw = 3
        d.sy = d.sx = d.py = d.px = d.dily = d.dilx = 1
        d.K, d.ldw, d.Cout, d.omLd, d.omSigmoid, d.outLd = 144, 32, 16, 32, 1, 16
        d.outNCHW, d.act, d.tile, d.ksplit, d.dg = 0, 0, 0, 0, 1
        return lambda Lb, P: Lb.cp_dcn_v2_f32(byref(d), P(B * H * W * ld), P(B * H * W * 32), P(SMALL * 4), P(SMALL), P(SMALL), P(B * H * W * 16), S)
    add("dcn-bytes", "dcn_v2", "input too large", dcn(1, 4096, 4096, 64), backed=8 << 30)
    add("dcn-columns", "dcn_v2", "input too large", dcn(LIM_B, LIM_H, LIM_W + 1, 64))
    # tier two
    add("decode-flat", "multi_pose_decode", "cat*H*W=2147483648",
        lambda Lb, P: Lb.cp_decode_topk_f32(P(SMALL), P(SMALL), 1, 2, 1, 32768, 32768, 1, P(SMALL), P(SMALL), S))
    meta = (c_int * 8)(2, 0, 0, 0, 0, 0, 0, 0)
    add("flip-pairs-map", "flip_merge_pairs", "map 0 too large",
        lambda Lb, P: Lb.cp_flip_merge_pairs_f32(1, arr([P(SMALL)], 4), arr([P(SMALL)], 4), meta, 1, 32768, 32768, 1, vp(0), S))
    add("head-points-plane", "head_points", "H*W=2147483648",
        lambda Lb, P: Lb.cp_head_points_f32(P(SMALL), 16, P(SMALL), P(SMALL), P(SMALL), P(SMALL), P(SMALL), P(SMALL), 1, 65536, 32768, 16, 1, 1, 32, S))
    add("head-points-rows", "head_points", "B*H=2147483648",
        lambda Lb, P: Lb.cp_head_points_f32(P(SMALL), 16, P(SMALL), P(SMALL), P(SMALL), P(SMALL), P(SMALL), P(SMALL), 1 << 16, 1 << 15, 1, 16, 1, 1, 32, S))
    add("head-points-pairs-plane", "head_points_pairs", "H*W=2147483648",
        lambda Lb, P: Lb.cp_head_points_pairs_f32(P(SMALL), 16, P(SMALL), P(SMALL), P(SMALL), P(SMALL), P(SMALL), P(SMALL), P(SMALL), 1, 65536, 32768,
                                                  16, 1, 1, 32, S))
    return out


def refuse(ref, device, fill=7.0):
    """call refusal row `ref` -> (rc, cp_last_error() text, [buffers]).  device: real buffers of the sizes an unrefused launch would need,
    filled with `fill`; else dummy non-null pointers (only where no device is present: no launch can happen there)."""
    import ctypes
    from centerpose_amd import _lib
    Lb = _lib.lib()
    keep = []

    def P(n):
        if not device:
            return ctypes.c_void_p(4096)
        keep.append(torch.full((n,), fill, device="cuda"))
        return ctypes.c_void_p(keep[-1].data_ptr())
    rc = ref.call(Lb, P)
    if device:
        torch.cuda.synchronize()
    return rc, Lb.cp_last_error().decode(), keep


REFUSAL_IDS = ("conv2d-bytes", "conv2d-columns", "conv2d-nchw", "conv2d-nchw-first", "conv2d-rows", "winograd-bytes", "head-bytes", "group-bytes",
               "group24-bytes", "winograd-grid", "winograd-vs64-grid", "winograd24-grid", "head-grid", "head24-grid", "group24-grid", "dcn-bytes", "dcn-columns", "decode-flat", "flip-pairs-map", "head-points-plane", "head-points-rows",
               "head-points-pairs-plane")
DEVICE_ONLY = ("winograd-vs64-grid", "winograd24-grid", "head-grid", "head24-grid")     # LDS reservation precedes the grid check
BACKED_IDS = ("conv2d-bytes", "winograd-bytes", "head-bytes", "group-bytes", "group24-bytes", "dcn-bytes", "winograd-grid", "group24-grid") + DEVICE_ONLY
_refusal_rows = {}


def refusal(rid):
    if not _refusal_rows:
        _refusal_rows.update((r.id, r) for r in _refusals())
        assert tuple(_refusal_rows) == REFUSAL_IDS and tuple(r for r in REFUSAL_IDS if _refusal_rows[r].backed) == tuple(
            r for r in REFUSAL_IDS if r in BACKED_IDS)
    return _refusal_rows[rid]


# ======================================================================================================================================
# the F(2x4) lean epilogue's own limit: (4*it + aa) * ostep reaches 13 output rows in `int` (conv3x3_wino24.hip:195, 408)
# ======================================================================================================================================
W24_EDGE_LD = 4096                                    # the output is a 32-channel slice of a 4096-float-wide buffer
W24_EDGE = {"general": 45000, "lean": (1 << 27) // W24_EDGE_LD - 1}
assert W24_EDGE["general"] * W24_EDGE_LD * 8 < 1 << 31 <= W24_EDGE["general"] * W24_EDGE_LD * 13      # the rule as it stood (x 8) took the lean epilogue
assert W24_EDGE["lean"] * W24_EDGE_LD * 16 < 1 << 31 <= (W24_EDGE["lean"] + 1) * W24_EDGE_LD * 16     # the last width the present rule (x 16) admits


def run_w24_edge(which):
    """B = 1, 14 x W, 16 -> 32 channels on the F(2x4) kernel, the output written into channels 64 .. 95 of a NaN-filled buffer of 4096 floats per
    pixel.  W = 45 000: 13 * W * outLd = 2 396 160 000 > INT_MAX, the launch must take the general epilogue (`<false>`, size_t rows);
    W = 32 767: the last width of the lean one (`<true>`).  Every output element against float64, every other float of the buffer still NaN.
    -> dict(kernel, worst, c, failures, peak)"""
    from centerpose_amd import ops
    W, H, ci, co, c0 = W24_EDGE[which], 14, 16, 32, 64
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    held_before = torch.cuda.memory_allocated()
    g = torch.Generator().manual_seed(4242)
    r = lambda *s_: torch.randn(*s_, generator=g)
    sd = lo.spread_bn({"b.weight": torch.rand(co, generator=g) + 0.5, "b.bias": r(co) * 0.1, "b.running_mean": r(co) * 0.1,
                       "b.running_var": torch.rand(co, generator=g) + 0.5, "c.weight": r(co, ci, 3, 3) * (2.0 / (9 * ci)) ** 0.5})
    x = F.relu(r(1, ci, H, W))
    fails = []
    with torch.no_grad():
        buf = _alloc(lambda: torch.full((1, H, W, W24_EDGE_LD), float("nan"), device="cuda"), H * W * W24_EDGE_LD * 4, "output")
        out = buf[..., c0:c0 + co]
        wp = ops.pack_conv_weight(sd["c.weight"].cuda())
        sc, sh = ops.fold_bn(co, tuple(sd["b." + n].cuda() for n in ("weight", "bias", "running_mean", "running_var")))
        la = ops.conv2d_launch([L._nhwc(x)], wp, sc, sh, out, kh=3, kw=3, stride=1, pad=1, cout=co, act=ops.ACT_RELU, wino=ops.pack_wino24_weight(wp, ci, co),
                               tile=ops.WINO24)
        la.run()
        torch.cuda.synchronize()
        got = out.permute(0, 3, 1, 2).contiguous().cpu()
        for y in range(H):                                 # row by row: no temporary of the whole 9.6 GiB
            if not (bool(torch.isnan(buf[0, y, :, :c0]).all()) and bool(torch.isnan(buf[0, y, :, c0 + co:]).all())):
                fails.append("row %d: stored outside the 32 channels the launch was given" % y)
        peak = torch.cuda.max_memory_allocated() - held_before
        kernel = la.kernel
        del buf, out, la
        torch.cuda.empty_cache()
    o64 = lo._conv_bn(sd, x.double(), "c", "b", False, co, 3, 1, 1, True, None, torch.float64)
    w, fail = lo.judge(got, None, o64, "wino24")
    if fail:
        fails.append(fail)
    if peak > MEM_LIMIT:
        fails.append("held %.2f GiB at once (limit %.0f GiB)" % (peak / 2 ** 30, MEM_LIMIT / 2 ** 30))
    return dict(kernel=kernel, worst=w, c=lo.c_for("wino24", o64.K), failures=fails, peak=peak)
