"""TEST INFRASTRUCTURE ONLY -- the split-bf16 implicit GEMM (csrc/conv_igemm_bf16x3.hip: igemm_bf16x3_kernel<BM, BN>, four instantiations)
under the per-element fp64 oracle of tests/layer_oracle.py, and under known-answer cases whose result is EXACT.

The kernel writes every fp32 operand as three bf16 terms and issues six of the nine cross products.  Its correctness rests on the
low-order terms: the third term is at most 2^-17 of the operand, and losing it on one staging lane, one LDS chunk or one k-group moves a
K-term sum by a few u A -- inside `layer_oracle.c_for("direct", K)` (44 for K >= 41), and far inside the max-norm criterion of
tests/test_conv_hip.py.  So this module holds

* ``ROWS``: forced launches (``split_bf16=True`` + CP_SPLIT_BF16_TILE) judged per element against float64 with the pieces of
  ``layer_oracle`` (``_conv_bn``, ``_affine``, ``_fold``, ``judge``, ``c_for``, ``padding_violation``, ``spread_bn``, ``first_unequal``):
  every producer (plain, stride 2, short K, tiny and boundary M, concatenation, fused sub-pixel deconvolution, split-K) and both
  epilogues on post-ReLU data; sources are channel slices of wider NaN buffers starting 16 bytes in, outputs NaN-guarded on every side;
* ``EXACT``: selection cases.  One operand is a scaled permutation (powers of two), the other holds full-24-bit values across 80 binades:
  every partial sum is representable, the result does not depend on the summation order and must come out BIT FOR BIT -- for every
  (slot, half / quarter, lane, term) of the activation path and every (n, k, term) of the weight path;
* ``split_weights_np``: the weight splitter (the same `sb_split2` the activation path runs) restated in NumPy integer arithmetic;
* ``emulate``: the kernel's arithmetic in NumPy (three RNE terms, the six products in the kernel's order, an exact 16-term product sum
  and one float32 rounding per MFMA) with the mutations tests/test_bf16x3_oracle_cpu.py proves the cases against;
* ``geometry``: the launch arithmetic of `launch_sb` and of the kernel's k-walk restated (blocks, k-steps per split, LDS bytes);
* ``refusals``: descriptors the launcher must turn away before any launch.

No bound is taken from device output: every bound is `layer_oracle.c_for`, every exact case is an identity of the operands.
"""
import collections
import ctypes
import functools

import numpy as np
import torch
import torch.nn.functional as F

import layer_oracle as lo
import launch_oracle as L

KERNEL = "igemm_bf16x3_kernel<%d, %d>"
TILES = ((128, 128), (128, 64), (64, 128), (64, 64))
SB_LDR, SB_ROW, IG_BK = 28, 24, 16            # LDS row stride and weight row in dwords, k per k-step (conv_igemm_bf16x3.hip, igemm.h)
MAXNORM_TOL = 2e-4                  # tests/test_conv_hip.py::_close: max|err| <= 2e-4 max|ref|
ORDER = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))      # (term of A, term of B) of the six MFMAs of a k-step, as sb_compute issues them
Row = collections.namedtuple("Row", "id kernel p")


def _r(id, tile, **p):
    d = dict(B=2, H=19, W=37, k=3, stride=1, pad=1, srcs=(32,), cout=100, S=1, res=True, relu=True, kind="conv", nchw=False, act=None, tile=tile)
    d.update(p)
    if d["S"] > 1:
        d["res"] = False
    bm, bn = (int(v) for v in tile.split("x"))
    return Row(id, KERNEL % (bm, bn), d)


def _rows():
    rows = []
    co = lambda t: 200 if t.endswith("x128") else 100           # ldw 256 resp. 128: two N blocks, the last one ragged
    for t in ("128x128", "64x128", "128x64", "64x64"):
        rows.append(_r("plain-" + t, t, cout=co(t)))
    for t in ("64x128", "128x128"):                             # 37 x 45 / s2 -> 19 x 23: M = 874 = 6 * 128 + 106 = 13 * 64 + 42
        rows.append(_r("s2-" + t, t, H=37, W=45, stride=2, cout=co(t)))
    rows.append(_r("shortk-64x64", "64x64", k=1, pad=0, srcs=(48,)))          # K = 48 <= 64: the tile of the launch rule; three k-steps
    for t, (h8, w8), (h9, w9) in (("64x64", (8, 8), (5, 13)), ("128x128", (8, 16), (3, 43))):
        kw = dict(k=1, pad=0, srcs=(48,), cout=co(t), B=1)
        rows.append(_r("m1-" + t, t, H=1, W=1, **kw))           # all but one staged row has boff = -1
        rows.append(_r("mBM-" + t, t, H=h8, W=w8, **kw))        # M = BM exactly
        rows.append(_r("mBM+1-" + t, t, H=h9, W=w9, **kw))      # one row in the second block
    for t in ("128x128", "64x64"):                              # half resp. quarter staging across a source switch, each source its own ld
        rows.append(_r("cat4-1x1-" + t, t, k=1, pad=0, srcs=(64, 32, 16, 48), cout=co(t)))
    for t in ("64x128", "128x64"):                              # advance() switches source inside every tap, with another srcC
        rows.append(_r("cat2-3x3-" + t, t, srcs=(16, 48), cout=co(t)))
    for t in ("128x64", "64x64"):                               # nsub = 4: 9 x 11 -> 18 x 22
        rows.append(_r("deconv-" + t, t, kind="deconv", H=9, W=11, k=2, pad=0, res=False))
    for t in ("64x64", "128x128"):
        rows.append(_r("split2-" + t, t, S=2, cout=co(t)))      # 18 k-steps: 9 + 9, the second split starts inside tap 4
        rows.append(_r("split4-" + t, t, S=4, cout=co(t)))      # starts 4 / 9 / 13
        rows.append(_r("split3-5x5-" + t, t, S=3, k=5, pad=2, cout=co(t)))     # 50 k-steps: starts 16 / 33
        rows.append(_r("splitmax-" + t, t, S=3, k=1, pad=0, srcs=(48,), cout=co(t)))   # S = K / 16: one k-step each
    for t in ("128x64", "64x64"):                               # cout = 34 in ldw = 64, no BN: bias -2.19 under the sigmoid
        rows.append(_r("nchw-sigmoid-" + t, t, k=1, pad=0, srcs=(64,), cout=34, nchw=True, act="sigmoid", relu=False, res=False))
        rows.append(_r("nchw-none-" + t, t, k=1, pad=0, srcs=(64,), cout=34, nchw=True, relu=False, res=False))
    return rows


ROWS = _rows()
ROW = {r.id: r for r in ROWS}
assert len(ROW) == len(ROWS)


# ---- launch arithmetic, restated ---------------------------------------------------------------------------------------------------------
def ldw_for(cout):
    return 16 if cout <= 16 else 32 if cout <= 32 else -(-cout // 64) * 64


def lds_bytes(bm, bn, nchw):
    """(bytes `launch_sb` reserves, which of main loop / epilogue decides).  Main loop: two stages of (BM + BN) rows of 28 dwords;
    epilogues of igemm.h: Cs[m][n + 4] (NHWC, vectorised) resp. Cs[n][m + 1] (NCHW)."""
    main = 2 * (bm + bn) * SB_LDR * 4
    epi = bn * (bm + 1) * 4 if nchw else bm * (bn + 4) * 4
    return max(main, epi), ("epilogue" if epi > main else "main")


def geometry(p):
    """what `launch_sb` and the kernel's k-walk make of the row: dict(M, Ho, Wo, BM, BN, ldw, K, nk, mblocks, nblocks, grid, lds, decides,
    splits [(ks0, ks1, tap, cl)]): a split with cl > 0 starts inside a tap"""
    bm, bn = (int(v) for v in p["tile"].split("x"))
    k, ct = p["k"], sum(p["srcs"])
    if p["kind"] == "deconv":
        Ho, Wo, nsub = p["H"], p["W"], 4
    else:
        Ho, Wo, nsub = (p["H"] + 2 * p["pad"] - k) // p["stride"] + 1, (p["W"] + 2 * p["pad"] - k) // p["stride"] + 1, 1
    M, K, ldw, S = p["B"] * Ho * Wo, k * k * ct, ldw_for(p["cout"]), p["S"]
    nk = K // IG_BK
    per_tap = ct // IG_BK
    splits = []
    for s in range(S):
        ks0, ks1 = s * nk // S, (s + 1) * nk // S
        splits.append((ks0, ks1, ks0 // per_tap, (ks0 % per_tap) * IG_BK))
    lds, decides = lds_bytes(bm, bn, p["nchw"])
    mb, nb = -(-M // bm), ldw // bn
    return dict(M=M, Ho=Ho, Wo=Wo, BM=bm, BN=bn, ldw=ldw, K=K, nk=nk, mblocks=mb, nblocks=nb, grid=mb * nb * nsub * S, lds=lds, decides=decides,
                splits=splits, nsub=nsub)


# ---- case data -----------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "row p sd xs res g cpad")


@functools.lru_cache(maxsize=4)
def make_case(rid):
    """the row's data (CPU, float32, logical NCHW), fixed by seed: post-ReLU inputs and residual, `spread_bn` on the folded scale (rows
    without BN: the spread on the rows of the weights)"""
    row = ROW[rid]
    p = row.p
    gen = torch.Generator().manual_seed(7000 + ROWS.index(row))
    r = lambda *s: torch.randn(*s, generator=gen)
    u01 = lambda n: torch.rand(n, generator=gen)
    g = geometry(p)
    B, H, W, co, k, ct = p["B"], p["H"], p["W"], p["cout"], p["k"], sum(p["srcs"])
    xs = [F.relu(r(B, c, H, W)) for c in p["srcs"]]
    bn = {"b.weight": u01(co) + 0.5, "b.bias": r(co) * 0.1, "b.running_mean": r(co) * 0.1, "b.running_var": u01(co) + 0.5}
    if p["kind"] == "deconv":
        sd = lo.spread_bn(dict(bn, **{"c.weight": r(ct, co, 4, 4) * (2.0 / (4 * ct)) ** 0.5}))
    elif p["nchw"]:
        sd = {"c.weight": r(co, ct, k, k) * (2.0 / (k * k * ct)) ** 0.5 * lo.spread_factors(co).view(-1, 1, 1, 1),
              "c.bias": torch.full((co,), L.SIGMOID_BIAS) if p["act"] == "sigmoid" else r(co) * 0.1}
    else:
        sd = lo.spread_bn(dict(bn, **{"c.weight": r(co, ct, k, k) * (2.0 / (k * k * ct)) ** 0.5}))
    OH, OW = (2 * H, 2 * W) if p["kind"] == "deconv" else (g["Ho"], g["Wo"])
    res = F.relu(r(B, co, OH, OW)) if p["res"] else None
    return Case(row, p, sd, xs, res, g, co if p["nchw"] else -(-co // 16) * 16)


def evaluate(case, dt):
    """the row's operation in plain torch, dtype `dt` -> lo.Out (A with float64)"""
    p, sd = case.p, case.sd
    x = torch.cat(case.xs, 1).to(dt)
    if p["kind"] == "deconv":
        w = sd["c.weight"].to(dt)
        scale, shift, ash = lo._fold(sd, "b", None, p["cout"], dt)
        v = F.conv_transpose2d(x, w, None, 2, 1) * scale + shift
        A = scale.abs() * F.conv_transpose2d(x.abs(), w.abs(), None, 2, 1) + ash if dt == torch.float64 else None
        return lo.Out(F.relu(v), A, 4 * w.shape[0] + 4)
    if p["nchw"]:
        return lo._affine(x, x.abs(), sd["c.weight"], *lo._fold(sd, None, "c.bias", p["cout"], dt), act=p["act"])
    return lo._conv_bn(sd, x, "c", "b", False, p["cout"], p["k"], p["stride"], p["pad"], p["relu"], case.res.to(dt) if case.res is not None else None, dt)


def folded(case):
    """(scale, shift) float32 [cout] as ops.fold_bn forms them"""
    sd, co = case.sd, case.p["cout"]
    if case.p["nchw"]:
        return torch.ones(co), sd["c.bias"].clone()
    scale = sd["b.weight"] / torch.sqrt(sd["b.running_var"] + lo.EPS)
    return scale, sd["b.bias"] - sd["b.running_mean"] * scale


def max_norm_accepts(out, o64):
    """the max-norm criterion of tests/test_conv_hip.py (`_close`): max|err| <= 2e-4 max|ref|"""
    return float((out.double() - o64.val).abs().max()) <= MAXNORM_TOL * max(float(o64.val.abs().max()), 1e-6)


def twice_f32_ratio(out, o32, o64):
    """max|err| over the float32 evaluation's max|err|: test_conv_split_bf16_matches_f32_kernel_tolerance also asks for <= 2 (+ 1e-7) against
    the f32 KERNEL's error, on randn inputs, one map and one tile per case.  Reported, not asserted: the losses of ACCEPTED_BY_BOUND give 1.9 .. 9.0 x on the plain rows, so
    that comparison would see most of them where it runs: plain convolutions, one tile per case."""
    return float((out.double() - o64.val).abs().max()) / float((o32.val.double() - o64.val).abs().max())


# ---- the splitter, restated ------------------------------------------------------------------------------------------------------------------
def bf16_rne_bits(x):
    """float32 ndarray -> uint32 ndarray holding the bf16 bits of round-to-nearest-even, by integer arithmetic (NaN stays NaN: quiet bit)"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7fff + ((b >> 16) & 1)) >> 16) & 0xffff
    nan = (b & 0x7fffffff) > 0x7f800000
    return np.where(nan, (b >> 16) | 0x40, r).astype(np.uint32)


def bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def split3(x):
    """x float32 ndarray -> [bits1, bits2, bits3] (uint32 arrays of bf16 bits): x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2), the
    residuals formed in float32 (exact for finite |x| < 2^127)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        b1 = bf16_rne_bits(x)
        r1 = (x - bf16_value(b1)).astype(np.float32)
        b2 = bf16_rne_bits(r1)
        r2 = (r1 - bf16_value(b2)).astype(np.float32)
        b3 = bf16_rne_bits(r2)
    return [b1, b2, b3]


def split_weights_np(w, ldw, swap_pairs=False):
    """packed weights [nsub * ldw][K] float32 -> uint32 [nsub][K / 16][ldw][3][8]: dword (term, pair) = bf16 term of k = 16 kc + 2 pair in
    the LOW half, of k + 1 in the high half.  swap_pairs: the mutation (halves exchanged)"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    rows, K = w.shape
    nsub, nk = rows // ldw, K // 16
    t = np.stack(split3(w), 0).reshape(3, nsub, ldw, nk, 8, 2)             # [term][sub][n][kc][pair][half]
    lo16, hi16 = (t[..., 1], t[..., 0]) if swap_pairs else (t[..., 0], t[..., 1])
    return np.ascontiguousarray((lo16 | (hi16 << 16)).transpose(1, 3, 2, 0, 4)).astype(np.uint32)


def bf16_is_nan(bits16):
    return (bits16 & 0x7fff) > 0x7f80


def splitter_mismatch(got, want):
    """first index where two dword arrays of bf16 pairs differ, NaN halves compared as NaN (the sign and payload of inf - inf are the
    hardware's), or None"""
    got, want = got.reshape(-1), want.reshape(-1)
    bad = np.zeros(got.shape, bool)
    for sh in (0, 16):
        a, b = (got >> sh) & 0xffff, (want >> sh) & 0xffff
        bad |= np.where(bf16_is_nan(b), ~bf16_is_nan(a), a != b)
    return int(np.argmax(bad)) if bad.any() else None


def full24(shape, gen, lo_e=-40, hi_e=40):
    """float32 values of both signs with full 24-bit significands, magnitudes spread over 2^lo_e .. 2^hi_e"""
    v = torch.randn(*shape, generator=gen) * torch.pow(2.0, torch.randint(lo_e, hi_e + 1, shape, generator=gen).float())
    return v.float()


def handmade():
    """the rounding cases by bit pattern: all significand bits set; exactly halfway between two bf16 values with an even and an odd lower
    neighbour (at both levels of the split); x1 rounding up so that x2 < 0; each in both signs and three binades"""
    pats = [0x3fffffff, 0x3f7fffff,               # all significand bits set
            0x3f808000, 0x3f818000,               # halfway, lower neighbour even (rounds down) / odd (rounds up)
            0x3f800080, 0x3f800180,               # the same tie at the second level
            0x3f80ffff, 0x3f80c000, 0x3f80ff80,   # x1 rounds up: x2 < 0 (and x3 < 0 in the last)
            0x3f808001, 0x3f807fff]               # one ulp on either side of the tie
    out = []
    for e in (0, 37, -33):
        for pat in pats:
            v = np.array([pat], np.uint32).view(np.float32)[0] * np.float32(2.0 ** e)
            out += [v, -v]
    return np.array(out, np.float32)


def domain_edges():
    """inputs of the splitter's domain edges (conv_igemm_bf16x3.hip header): +-0, the hand-made rounding cases, values below 2^-110 whose
    lower terms fall into bf16 subnormals, the top binade's upper half (x1 = +-inf, x2 = -+inf, x3 = NaN) and +-inf (x2 = NaN)"""
    tiny = np.array([0x08ffffff, 0x0880c001, 0x04abcdef, 0x00ffffff, 0x00800001, 0x007fffff, 0x00000001], np.uint32).view(np.float32)
    top = np.array([0x7f7fffff, 0x7f7f8000, 0x7f7f7fff], np.uint32).view(np.float32)
    v = np.concatenate([np.array([0.0, -0.0], np.float32), handmade(), tiny, -tiny, top, -top, np.array([np.inf, -np.inf], np.float32)])
    return v


# ---- the kernel's arithmetic, emulated -----------------------------------------------------------------------------------------------------
def im2col(x, kh, kw, stride, pt, pb, pl, pr):
    """x [B, C, H, W] float32 -> A [B Ho Wo][kh kw C], k = (ky kw + kx) C + c: the k order of ops.pack_conv_weight and of the kernel's walk
    (tap, then source, then channel: the sources concatenated along C)"""
    B, C = x.shape[:2]
    cols = F.unfold(F.pad(x, (pl, pr, pt, pb)), (kh, kw), stride=stride)
    Lc = cols.shape[2]
    return cols.view(B, C, kh * kw, Lc).permute(0, 3, 2, 1).reshape(B * Lc, kh * kw * C).contiguous()


def emulate_gemm(A, Wm, ks0=0, ks1=None, mut=None, a_cols=None):
    """acc [M][N] float32 of the k-steps [ks0, ks1): per k-step the six MFMAs of ORDER, each an exact 16-term sum of exact bf16 x bf16
    products added to the accumulator with ONE float32 rounding (the product sum is formed in float64: exact while the 16 products of a
    k-step span fewer than 2^20 in magnitude, and otherwise still far below u A; the device's own internal order is not modelled).
    mut: None or a mutation of MUTATIONS that acts on the operand terms; a_cols: None or a map k-step -> k-step the A operand is read from"""
    A, Wm = np.ascontiguousarray(A, np.float32), np.ascontiguousarray(Wm, np.float32)
    K = A.shape[1]
    nk = K // 16
    ks1 = nk if ks1 is None else ks1
    At = [bf16_value(b).astype(np.float64) for b in split3(A)]
    Bt = [bf16_value(b).astype(np.float64) for b in split3(Wm)]
    kin = np.arange(K) % 16
    if mut == "x3-quarter3":
        At[2][:, kin >= 12] = 0
    elif mut == "x3-upper8":
        s = min(ks0 + 1, ks1 - 1)
        At[2][:, s * 16 + 8:s * 16 + 16] = 0
    elif mut == "w-chunk5":
        Bt[2][:, kin >= 8] = 0
    elif mut == "pair-swap":
        Bt = [b[:, np.arange(K) ^ 1] for b in Bt]
    else:
        assert mut is None, mut
    acc = np.zeros((A.shape[0], Wm.shape[0]), np.float32)
    for ks in range(ks0, ks1):
        ka = a_cols.get(ks, ks) if a_cols else ks
        for ta, tb in ORDER:
            acc = (acc.astype(np.float64) + At[ta][:, ka * 16:ka * 16 + 16] @ Bt[tb][:, ks * 16:ks * 16 + 16].T).astype(np.float32)
    return acc


MUTATIONS = ("x3-quarter3", "x3-upper8", "w-chunk5", "pair-swap", "start-tap", "late-switch", "next-image")
ACCEPTED_BY_BOUND = MUTATIONS[:3]          # what `c_for` and the max-norm criterion let through on the plain rows: why EXACT exists


def _a_matrix(case, sub=0, mut=None):
    p = case.p
    xs = case.xs
    if mut == "next-image":                 # boff of the next image
        xs = [torch.roll(x, -1, 0) for x in xs]
    x = torch.cat(xs, 1)
    if p["kind"] == "deconv":
        py, px = 1 - (sub >> 1), 1 - (sub & 1)
        return im2col(x, 2, 2, 1, py, 1 - py, px, 1 - px).numpy()
    return im2col(x, p["k"], p["k"], p["stride"], p["pad"], p["pad"], p["pad"], p["pad"]).numpy()


def packed_weight(case):
    """[nsub * ldw][K] float32 as ops.pack_conv_weight / pack_deconv4_subpixel lay it out (rows past cout: zeros)"""
    p, w, ldw = case.p, case.sd["c.weight"], case.g["ldw"]
    pad = lambda m: torch.cat([m, torch.zeros(ldw - m.shape[0], m.shape[1])], 0)
    if p["kind"] == "deconv":
        subs = []
        for py in range(2):
            for px in range(2):
                s = w[:, :, [3 - py - 2 * t for t in range(2)]][:, :, :, [3 - px - 2 * t for t in range(2)]]
                subs.append(pad(s.permute(1, 2, 3, 0).reshape(w.shape[1], 4 * w.shape[0])))
        return torch.cat(subs, 0).contiguous()
    return pad(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)).contiguous()


def emulate(case, mut=None):
    """the row through the emulated kernel (and the split reduction / epilogue in float32) -> logical NCHW float32 tensor"""
    p, g = case.p, case.g
    co, ldw, S = p["cout"], g["ldw"], p["S"]
    wp = packed_weight(case).numpy()
    scale, shift = (t.numpy().astype(np.float32) for t in folded(case))
    gm = mut if mut in ("x3-quarter3", "x3-upper8", "w-chunk5", "pair-swap") else None
    outs = []
    for sub in range(g["nsub"]):
        A = _a_matrix(case, sub, mut)
        Wm = wp[sub * ldw:sub * ldw + co]
        acc = None
        for s, (ks0, ks1, tap, cl) in enumerate(g["splits"]):
            a_cols = None
            if mut == "start-tap" and s > 0:                 # per_tap of another source: the split's A walk starts at another (tap, channel)
                wrong = max(1, (sum(p["srcs"]) // IG_BK) // 2)
                shift_ks = (ks0 // wrong) * (sum(p["srcs"]) // IG_BK) + ks0 % wrong - ks0
                a_cols = {ks: min(max(ks + shift_ks, 0), g["nk"] - 1) for ks in range(ks0, ks1)}
            if mut == "late-switch":                         # the first k-step of every later source still reads the previous one
                per_tap, first = sum(p["srcs"]) // IG_BK, np.cumsum(p["srcs"])[:-1] // IG_BK
                a_cols = {ks: ks - 1 for ks in range(ks0, ks1) if ks % per_tap in first}
            part = emulate_gemm(A, Wm, ks0, ks1, gm if (gm != "x3-upper8" or s == 0) else None, a_cols)
            acc = part if acc is None else (acc + part).astype(np.float32)          # splitk_reduce: fixed order s = 0, 1, ...
        v = (acc * scale[None, :]).astype(np.float32) + shift[None, :]
        outs.append(v.astype(np.float32))
    B, Ho, Wo = p["B"], g["Ho"], g["Wo"]
    if p["kind"] == "deconv":
        full = np.zeros((B, 2 * Ho, 2 * Wo, co), np.float32)
        for sub, v in enumerate(outs):
            full[:, (sub >> 1)::2, (sub & 1)::2] = v.reshape(B, Ho, Wo, co)
        v = full
    else:
        v = outs[0].reshape(B, Ho, Wo, co)
    t = torch.from_numpy(v).permute(0, 3, 1, 2).contiguous()
    if case.res is not None:
        t = t + case.res
    if p["relu"]:
        t = F.relu(t)
    if p["act"] == "sigmoid":
        t = torch.sigmoid(t)
    return t


# ---- exact-answer cases --------------------------------------------------------------------------------------------------------------------
ExactCase = collections.namedtuple("ExactCase", "id kind k x w want")
EXACT_KINDS = ("select-1x1", "select-3x3", "transposed")
EX_B, EX_H, EX_W = 2, 19, 37                 # M = 1406: ragged against 64 and 128 rows; every slot, half / quarter and lane stages real pixels


@functools.lru_cache(maxsize=3)
def exact_case(kind):
    """x [B, C, H, W], w [Co, C, k, k] (float32, CPU) and the answer `want` [B, Co, H, W] that scale = 1, shift = 0, no activation must give
    bit for bit.
    select-1x1: w a permutation matrix with rows scaled by 2^e, e in [-8, 8]; x full-24-bit values over 2^-40 .. 2^40 and the hand-made
      rounding cases: want[m, n] = x[m, pi(n)] 2^e.  The kernel adds x3, then x2, then x1 (times the one bf16 term 2^e, zeros elsewhere);
      x3 + x2 and (x3 + x2) + x1 are float32 numbers, so every partial sum is exact.
    select-3x3: cin = 16, 256 outputs, output n selects (tap, channel) = n mod 144: shifted copies of x with exact zeros at the border.
    transposed: pixel m carries one non-zero channel k(m) = m mod K, a power of two; w holds the full-24-bit values: want[m, n] = w[n, k(m)] 2^e
      -- the weight splitter, the slab copy and the (idx / 6, idx % 6) LDS map for every (n, k, term)."""
    gen = torch.Generator().manual_seed(90210 + EXACT_KINDS.index(kind))
    B, H, W = EX_B, EX_H, EX_W
    M = B * H * W
    hm = torch.from_numpy(handmade())
    if kind == "select-1x1":
        C = Co = 128
        x = full24((B, C, H, W), gen)
        flat = x.permute(0, 2, 3, 1).reshape(M, C)
        for j in range(hm.numel()):                          # hand-made values on every channel residue and on rows of every block
            flat[(j * 97) % M, (j * 5 + j // 16) % C] = hm[j]
        x = flat.view(B, H, W, C).permute(0, 3, 1, 2).contiguous()
        pi = torch.randperm(C, generator=gen)
        e = torch.randint(-8, 9, (Co,), generator=gen).float()
        w = torch.zeros(Co, C, 1, 1)
        w[torch.arange(Co), pi, 0, 0] = torch.pow(2.0, e)
        want = x[:, pi] * torch.pow(2.0, e).view(1, -1, 1, 1)
        return ExactCase(kind, kind, 1, x, w, want)
    if kind == "select-3x3":
        C, Co = 16, 256
        x = full24((B, C, H, W), gen)
        flat = x.view(-1)
        flat[torch.arange(hm.numel()) * 331 % flat.numel()] = hm
        e = torch.randint(-8, 9, (Co,), generator=gen).float()
        w = torch.zeros(Co, C, 3, 3)
        want = torch.zeros(B, Co, H, W)
        xp = F.pad(x, (1, 1, 1, 1))
        for n in range(Co):
            tap, c = divmod(n % 144, 16)
            ky, kx = divmod(tap, 3)
            w[n, c, ky, kx] = 2.0 ** float(e[n])
            want[:, n] = xp[:, c, ky:ky + H, kx:kx + W] * 2.0 ** float(e[n])
        return ExactCase(kind, kind, 3, x, w, want)
    assert kind == "transposed"
    C = Co = 128
    w = full24((Co, C, 1, 1), gen)
    wf = w.view(-1)
    wf[torch.arange(hm.numel()) * 233 % wf.numel()] = hm
    m = torch.arange(M)
    km, e = m % C, ((m * 7) % 17 - 8).float()
    flat = torch.zeros(M, C)
    flat[m, km] = torch.pow(2.0, e)
    x = flat.view(B, H, W, C).permute(0, 3, 1, 2).contiguous()
    want = (w.view(Co, C)[:, km] * torch.pow(2.0, e).view(1, -1)).t().reshape(B, H, W, Co).permute(0, 3, 1, 2).contiguous()
    return ExactCase(kind, kind, 1, x, w, want)


def emulate_exact(ec, mut=None):
    pad = ec.k // 2
    A = im2col(ec.x, ec.k, ec.k, 1, pad, pad, pad, pad).numpy()
    Wm = ec.w.permute(0, 2, 3, 1).reshape(ec.w.shape[0], -1).numpy()
    acc = emulate_gemm(A, Wm, mut=mut)
    B, _, H, W = ec.x.shape
    return torch.from_numpy(acc.reshape(B, H, W, -1)).permute(0, 3, 1, 2).contiguous()


def bits_differ(a, b):
    """elementwise: other BITS (so that -0 != +0 and equal NaNs compare equal)"""
    return a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)


def ulp_distance(a, b):
    """largest distance in units of the last place between two finite float32 tensors (bit patterns mapped to a monotone integer line)"""
    def line(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    return int((line(a) - line(b)).abs().max())


# ---- device --------------------------------------------------------------------------------------------------------------------------------
def _src_slice(t, extra=0):
    """logical NCHW CPU tensor -> device NHWC view: a channel slice of a wider NaN buffer that starts 16 bytes in (the smallest offset the
    kernel's 16-byte alignment admits); ld = C + 8 + extra"""
    B, C, H, W = t.shape
    buf = torch.full((B, H, W, C + 8 + extra), float("nan"), device="cuda")
    v = buf[..., 4:4 + C]
    v.copy_(t.permute(0, 2, 3, 1))
    assert v.data_ptr() % 16 == 0 and v.data_ptr() - buf.data_ptr() == 16
    return v


class Guarded:
    """an output inside a NaN-filled buffer: NHWC [B, OH, OW, :c] of a buffer with a guard IMAGE before and after and guard channels past c,
    or NCHW [B, c, OH, OW] inside a flat buffer with a guard of one image before and after"""

    def __init__(self, B, OH, OW, c, nchw):
        self.nchw = nchw
        if nchw:
            n, G = B * c * OH * OW, c * OH * OW
            self.buf = torch.empty(n + 2 * G, device="cuda")
            self.out = self.buf[G:G + n].view(B, c, OH, OW)
        else:
            self.buf = torch.empty(B + 2, OH, OW, -(-c // 4) * 4 + 4, device="cuda")
            self.out = self.buf[1:B + 1, :, :, :c]
        self.fill()

    def fill(self):
        self.buf.fill_(float("nan"))

    def outside_untouched(self):
        n = torch.isnan
        if self.nchw:
            G = (self.buf.numel() - self.out.numel()) // 2
            return bool(n(self.buf[:G]).all() and n(self.buf[G + self.out.numel():]).all())
        return bool(n(self.buf[0]).all() and n(self.buf[-1]).all() and n(self.buf[1:-1, :, :, self.out.shape[3]:]).all())


def launch_kw(p, g):
    if p["kind"] == "deconv":
        return dict(kh=2, kw=2, stride=1, pad=0, pad_yx=(1, 1), Ho=g["Ho"], Wo=g["Wo"], out_scatter=(2, 2, 0, 0), nsub=4)
    return dict(kh=p["k"], kw=p["k"], stride=p["stride"], pad=p["pad"])


def build_launches(case, setenv):
    """-> (launches, Guarded, workspace or None).  setenv(name, value): the test's monkeypatch.setenv (the forced tile is read when the launch
    is BUILT)"""
    from centerpose_amd import ops
    p, g, sd = case.p, case.g, case.sd
    B, co, cp, S = p["B"], p["cout"], case.cpad, p["S"]
    setenv("CP_SPLIT_BF16_TILE", p["tile"])
    srcs = [_src_slice(x, 4 * i) for i, x in enumerate(case.xs)]
    if p["kind"] == "deconv":
        w = sd["c.weight"].cuda()
        wp = torch.cat([ops.pack_deconv4_subpixel(w, py, px) for py in range(2) for px in range(2)], 0).contiguous()
        OH, OW = 2 * g["Ho"], 2 * g["Wo"]
    else:
        wp = ops.pack_conv_weight(sd["c.weight"].cuda())
        OH, OW = g["Ho"], g["Wo"]
    assert torch.equal(wp.cpu(), packed_weight(case)) and wp.shape[0] == g["ldw"] * g["nsub"]
    if p["nchw"]:
        sc, sh = ops.fold_bn(co, None, sd["c.bias"].cuda())
    else:
        sc, sh = ops.fold_bn(co, tuple(sd["b." + s].cuda() for s in ("weight", "bias", "running_mean", "running_var")))
    act = ops.ACT_SIGMOID if p["act"] == "sigmoid" else ops.ACT_RELU if p["relu"] else ops.ACT_NONE
    gd = Guarded(B, OH, OW, cp, p["nchw"])
    res = L._nhwc(case.res, cp, -(-cp // 4) * 4 + 4) if case.res is not None else None        # its padding channels are zeros
    kw = launch_kw(p, g)
    if S == 1:
        la = ops.conv2d_launch(srcs, wp, sc, sh, gd.out, cout=cp, act=act, res=res, out_nchw=p["nchw"], split_bf16=True, **kw)
        return [la], gd, None
    ldw = g["ldw"]
    ws = torch.full((S, g["M"], ldw), float("nan"), device="cuda")                            # S M ldw exactly
    la = ops.conv2d_launch(srcs, wp, torch.ones(ldw, device="cuda"), torch.zeros(ldw, device="cuda"), ws, cout=ldw, ksplit=S, split_bf16=True, **kw)
    return [la, ops.splitk_reduce_launch(ws, sc, sh, gd.out, cout=cp, act=act)], gd, ws


def _read(case, gd):
    co = case.p["cout"]
    if case.p["nchw"]:
        return None, gd.out.cpu().clone()
    phys = gd.out.cpu()
    return phys, phys[..., :co].permute(0, 3, 1, 2).contiguous()


def run_row(rid, setenv):
    """Build the row, run it twice (the buffers NaN-filled again in between) and judge it.  -> dict(kernels, worst, c, failures)"""
    case = make_case(rid)
    fails = []
    with torch.no_grad():
        launches, gd, ws = build_launches(case, setenv)
        runs = []
        for _ in range(2):
            gd.fill()
            if ws is not None:
                ws.fill_(float("nan"))
            for la in launches:
                la.run()
            torch.cuda.synchronize()
            runs.append(_read(case, gd) + (gd.outside_untouched(),))
        o64 = evaluate(case, torch.float64)
    (phys, first, g1), (phys2, second, g2) = runs
    w, fail = lo.judge(first, None, o64, "direct")
    if fail:
        fails.append(fail)
    if not (g1 and g2):
        fails.append("stored outside the %d channels / %d images the launch was given (NaN guard overwritten)" % (case.cpad, case.p["B"]))
    if bool(bits_differ(first, second).any()) or (phys is not None and bool(bits_differ(phys, phys2).any())):
        fails.append("a second run gives other bits at %s" % (lo.first_unequal(first, second),))
    if phys is not None:
        loc = lo.padding_violation(phys, lo.View(phys.shape[1], phys.shape[2], case.p["cout"], None, None))
        if loc is not None:
            fails.append("padding channel not zero at (b, y, x, c) = %s: %r" % (loc, float(phys[loc])))
    if case.p["act"] == "sigmoid" and lo.sigmoid_liveness(first) < lo.LIVE_FLOOR["sigmoid"]:
        fails.append("degenerate test data: sigmoid")
    return dict(kernels=[la.kernel for la in launches], worst=w, c=lo.c_for("direct", o64.K), failures=fails)


def run_exact(kind, tile, setenv):
    """the exact case on tile "BMxBN" -> dict(kernel, mismatches, first (loc, got, want) or None, ulp, guard, pattern)"""
    from centerpose_amd import ops
    ec = exact_case(kind)
    setenv("CP_SPLIT_BF16_TILE", tile)
    B, C, H, W = ec.x.shape
    co = ec.w.shape[0]
    with torch.no_grad():
        gd = Guarded(B, H, W, co, False)
        wp = ops.pack_conv_weight(ec.w.cuda())
        la = ops.conv2d_launch([_src_slice(ec.x)], wp, torch.ones(wp.shape[0], device="cuda"), torch.zeros(wp.shape[0], device="cuda"), gd.out,
                               kh=ec.k, kw=ec.k, stride=1, pad=ec.k // 2, cout=co, split_bf16=True)
        la.run()
        torch.cuda.synchronize()
        got = gd.out.cpu().permute(0, 3, 1, 2).contiguous()
        guard = gd.outside_untouched()
    bad = bits_differ(got, ec.want) & ~((got == 0) & (ec.want == 0))          # a zero of either sign where zero is wanted
    n = int(bad.sum())
    first, pattern = None, ""
    if n:
        loc = lo.first_unequal(bad.to(torch.int32), torch.zeros_like(bad, dtype=torch.int32))
        first = (loc, float(got[loc]), float(ec.want[loc]))
        idx = bad.nonzero()
        m = (idx[:, 0] * H + idx[:, 2]) * W + idx[:, 3]
        pattern = "rows mod 128 hit: %d of 128, channels mod 16 hit: %d of 16" % (len(set((m % 128).tolist())), len(set((idx[:, 1] % 16).tolist())))
    finite = torch.isfinite(got).all()
    return dict(kernel=la.kernel, mismatches=n, first=first, ulp=ulp_distance(got, ec.want) if finite else -1, guard=guard, pattern=pattern,
                total=got.numel())


def device_split(w, ldw):
    """ops.split_bf16_weight of a CPU float32 matrix -> uint32 ndarray (flat)"""
    from centerpose_amd import ops
    wb = ops.split_bf16_weight(torch.from_numpy(np.ascontiguousarray(w)).cuda(), ldw)
    torch.cuda.synchronize()
    return wb.cpu().numpy().view(np.uint32)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
Refusal = collections.namedtuple("Refusal", "id text mod")
REFUSALS = (
    Refusal("splitk-two-sources", "split-K writes raw NHWC partial sums", dict(nsrc=2, ksplit=2)),
    Refusal("splitk-nsub4", "split-K writes raw NHWC partial sums", dict(nsub=4, ksplit=2)),
    Refusal("splitk-too-many", "at most K/16 = 3 splits", dict(ksplit=4)),
    Refusal("source-misaligned", "source 0 is not 16-byte aligned", dict(src_off=4)),
    Refusal("ld-not-4", "ld%4==0", dict(ld=50)),
    Refusal("ldw-not-BN", "ldw=64 is not a multiple of the N tile 128", dict(tile=3128128)),
    Refusal("unknown-tile", "unknown tile 3096064", dict(tile=3096064)),
)


def refuse(ref, device):
    """One 1x1 descriptor (B = 1, 8 x 8, 48 -> 64 channels, K = 48) with the one deviation `ref.mod`, handed to cp_conv2d_f32.  device: real
    NaN-filled buffers (they must stay NaN: nothing may be launched), else dummy non-null pointers.  -> (rc, cp_last_error text, [buffers])"""
    from centerpose_amd import _lib, ops
    Lb = _lib.lib()
    m = ref.mod
    B, H, W, C, ldw = 1, 8, 8, 48, 64
    nsrc, nsub, S, ld = m.get("nsrc", 1), m.get("nsub", 1), m.get("ksplit", 0), m.get("ld", 52)
    d = ops.ConvDesc()
    d.nsrc = nsrc
    for i in range(nsrc):
        d.srcC[i], d.srcLd[i] = (C if nsrc == 1 else 16 + 16 * i), ld
    d.B, d.H, d.W, d.Ho, d.Wo = B, H, W, H, W
    d.kh = d.kw = 2 if nsub == 4 else 1
    d.sy = d.sx = 1
    d.py = d.px = 1 if nsub == 4 else 0
    d.K, d.ldw, d.Cout, d.nsub = C * (4 if nsub == 4 else 1), ldw, ldw, nsub
    d.resLd, d.outNCHW, d.ksplit, d.act, d.inNCHW = 0, 0, S, 0, 0
    d.OH, d.OW, d.outLd = (2 * H, 2 * W, ldw) if nsub == 4 else (H, W, ldw)
    d.osy = d.osx = 2 if nsub == 4 else 1
    d.ooy = d.oox = 0
    d.tile = m.get("tile", 3064064)
    keep = []

    def P(n, off=0):
        if not device:
            return 4096 + off
        keep.append(torch.full((n + 4,), float("nan"), device="cuda"))
        return keep[-1].data_ptr() + off
    srcs = (ctypes.c_void_p * 4)(*([P(B * H * W * ld, m.get("src_off", 0)) for _ in range(nsrc)] + [0] * (4 - nsrc)))
    vp = ctypes.c_void_p
    wfloats = nsub * ldw * (d.K // 16) * SB_ROW
    rc = Lb.cp_conv2d_f32(ctypes.byref(d), srcs, vp(P(wfloats)), vp(P(ldw)), vp(P(ldw)), vp(0), vp(P(max(S, 1) * d.OH * d.OW * ldw)), vp(0))
    if device:
        torch.cuda.synchronize()
    return rc, Lb.cp_last_error().decode(), keep
