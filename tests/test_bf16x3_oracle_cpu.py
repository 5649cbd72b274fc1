"""CPU: the split-bf16 oracle's own claims (tests/bf16x3_oracle.py), with no device.

* every row's geometry, from the restated launch arithmetic: M against BM, the N blocks, the k-steps per split and which splits start inside
  a tap, the LDS reservation per tile and output mode;
* the yardstick: the float32 torch evaluation of every row within 1.25 x C_REF32["direct"], the NumPy emulation of the split arithmetic
  within `c_for("direct", K)`; no bound is taken from a device and no family key is added;
* the exactness identities of the selection cases hold in the emulation, on the committed inputs;
* teeth: every mutation of `bf16x3_oracle.MUTATIONS` (and the signed 16-bit offset) is rejected at the mutated elements by the case meant
  for it -- and the first three are ACCEPTED by the per-element bound and by the max-norm criterion on the plain rows, which is why the
  exact cases exist;
* the splitter restatement against torch's own bfloat16 rounding, and that three terms restore the operand;
* the kernel's 32-bit quantities at LIM and at 16 bits (tests/limit_oracle.py: `audit("bf16x3")`).

Run with -s for the yardstick table.
"""
import numpy as np
import pytest
import torch

import bf16x3_oracle as S
import layer_oracle as lo
import limit_oracle as M

PLAIN = [r.id for r in S.ROWS if r.id.startswith("plain-")]
_evals = {}


def _ev(rid):
    """(case, float32 evaluation, float64 evaluation, emulation) of a row, computed once"""
    if rid not in _evals:
        case = S.make_case(rid)
        with torch.no_grad():
            _evals[rid] = (case, S.evaluate(case, torch.float32), S.evaluate(case, torch.float64), S.emulate(case))
    return _evals[rid]


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------
def test_rows_cover_every_instantiation_and_every_producer():
    by = lambda pre: {r.kernel for r in S.ROWS if r.id.startswith(pre)}
    every = {S.KERNEL % t for t in S.TILES}
    assert by("plain-") == every and len(S.ROWS) == 31
    for pre in ("split", "cat", "nchw-", "deconv-", "m1-", "mBM-", "mBM+1-", "s2-"):
        assert len(by(pre)) >= 2, pre
    assert S.KERNEL % (64, 64) in by("shortk-")


@pytest.mark.parametrize("rid", [r.id for r in S.ROWS])
def test_row_geometry(rid):
    p = S.ROW[rid].p
    g = S.geometry(p)
    bm, bn = g["BM"], g["BN"]
    assert g["ldw"] % bn == 0, "ops.split_bf16_tile would fall back to BN = 64"
    assert g["ldw"] == S.ldw_for(p["cout"]) and g["K"] % 16 == 0 and all(c % 16 == 0 for c in p["srcs"])
    if rid.startswith(("m1-", "mBM-", "mBM+1-")):
        assert g["M"] == {"m1": 1, "mBM": bm, "mBM+1": bm + 1}[rid.split("-")[0]] and g["mblocks"] == (2 if rid.startswith("mBM+1") else 1)
    else:
        assert p["B"] == 2 and g["M"] % bm and g["M"] % 64 and g["M"] % 128 and g["mblocks"] >= 2       # ragged against 64 and 128 rows
    if p["nchw"]:
        assert (g["ldw"], g["nblocks"], p["cout"]) == (64, 1, 34)          # one N block, ragged: 34 of 64 columns
    else:
        assert g["nblocks"] == 2 and p["cout"] % bn and p["cout"] > bn     # two N blocks, the last one ragged
    per_split = [b - a for a, b, _, _ in g["splits"]]
    if rid.startswith("splitmax-"):
        assert per_split == [1, 1, 1] and p["S"] == g["K"] // 16            # the most the launcher accepts
    else:
        assert min(per_split) >= 3
    assert g["grid"] == g["mblocks"] * g["nblocks"] * g["nsub"] * p["S"]
    if rid.startswith("plain-"):
        assert g["M"] == 1406 == 10 * 128 + 126 == 21 * 64 + 62 and g["nk"] == 18
    if rid.startswith("s2-"):
        assert (g["Ho"], g["Wo"], g["M"]) == (19, 23, 874)
    if rid.startswith("shortk-"):
        assert g["K"] == 48 <= 64 and g["nk"] == 3
    if rid.startswith("deconv-"):
        assert g["nsub"] == 4 and (2 * g["Ho"], 2 * g["Wo"]) == (18, 22) and g["K"] == 4 * 32
    if rid.startswith("cat2-3x3-"):
        assert g["nk"] == 36 and p["srcs"] == (16, 48)                     # per tap: one k-step of source 0, three of source 1
    if rid.startswith("cat4-"):
        assert g["nk"] == 10 and p["srcs"] == (64, 32, 16, 48)


def test_split_starts():
    """which splits start inside a tap (cl > 0: the k-walk begins between two sources' worth of channels of one tap)"""
    sp = lambda rid: [(a, tap, cl) for a, _, tap, cl in S.geometry(S.ROW[rid].p)["splits"]]
    for t in ("64x64", "128x128"):
        assert sp("split2-" + t) == [(0, 0, 0), (9, 4, 16)]
        assert sp("split4-" + t) == [(0, 0, 0), (4, 2, 0), (9, 4, 16), (13, 6, 16)]
        assert sp("split3-5x5-" + t) == [(0, 0, 0), (16, 8, 0), (33, 16, 16)]
        assert sp("splitmax-" + t) == [(0, 0, 0), (1, 0, 16), (2, 0, 32)]


def test_lds_reservation():
    """main loop 2 (BM + BN) x 112 B against the epilogues' Cs[BM][BN + 4] (NHWC) and Cs[BN][BM + 1] (NCHW).  Only <128, 128> has an
    epilogue larger than its main loop (and larger than 64 KiB: the launcher's CpLdsGuard path); for the NCHW rows' tiles <128, 64> and
    <64, 64> the main loop decides in both modes."""
    want = {(128, 128, False): (67584, "epilogue"), (128, 128, True): (66048, "epilogue"), (128, 64, False): (43008, "main"),
            (128, 64, True): (43008, "main"), (64, 128, False): (43008, "main"), (64, 128, True): (43008, "main"),
            (64, 64, False): (28672, "main"), (64, 64, True): (28672, "main")}
    for (bm, bn, nchw), v in want.items():
        assert S.lds_bytes(bm, bn, nchw) == v
    assert all(S.lds_bytes(bm, bn, n)[0] <= 160 * 1024 for bm, bn in S.TILES for n in (False, True))
    for r in S.ROWS:
        g = S.geometry(r.p)
        assert (g["lds"], g["decides"]) == want[(g["BM"], g["BN"], r.p["nchw"])]


# ---- yardstick -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", [r.id for r in S.ROWS])
def test_yardstick(rid):
    case, o32, o64, emu = _ev(rid)
    c = lo.c_for("direct", o64.K)
    w32 = lo.worst_ratio(o32.val, o64.val, o64.A)
    wem, fail = lo.judge(emu, None, o64, "direct")
    print("\n%-22s K %4d  c %5.1f  float32 torch %6.3f   split emulation %6.3f" % (rid, o64.K, c, w32.ratio, wem.ratio))
    assert w32.ratio <= 1.25 * lo.C_REF32["direct"]
    assert fail is None, fail
    assert S.max_norm_accepts(emu, o64)
    assert bool((o64.A > 0).all()) and bool(torch.isfinite(o64.val).all())


def test_no_family_key_added():
    assert sorted(lo.LAYER_TOL) == ["dcn", "direct", "wino", "wino24"] and lo.MARGIN == 4.0


# ---- splitter ------------------------------------------------------------------------------------------------------------------------------
def test_rne_by_integer_arithmetic_is_torch_bfloat16():
    g = torch.Generator().manual_seed(3)
    x = torch.cat([S.full24((200000,), g), torch.from_numpy(S.handmade())])
    want = x.to(torch.bfloat16).view(torch.int16).numpy().astype(np.uint32) & 0xffff
    assert np.array_equal(S.bf16_rne_bits(x.numpy()), want)


def test_three_terms_restore_the_operand_and_the_kernel_order_is_exact():
    """x1 + x2 + x3 == x, and the kernel's order of the selection cases -- x3, then x2, then x1 -- passes through float32 numbers only"""
    g = torch.Generator().manual_seed(4)
    x = np.concatenate([S.full24((2000000,), g).numpy(), S.handmade()])
    t = [S.bf16_value(b).astype(np.float64) for b in S.split3(x)]
    assert np.array_equal(t[0] + t[1] + t[2], x.astype(np.float64))
    s32 = (t[2] + t[1]).astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), t[2] + t[1])
    assert np.array_equal((s32.astype(np.float64) + t[0]).astype(np.float32), x)
    hm = S.split3(S.handmade())
    neg2 = (S.bf16_value(hm[1]) * np.sign(S.handmade())) < 0
    assert neg2.any() and (S.bf16_value(hm[2]) != 0).any()                 # x1 rounded up: x2 of the other sign; third terms alive


def test_split_weights_layout():
    w = np.arange(2 * 64 * 32, dtype=np.float32).reshape(128, 32) + 1      # small integers: exact in bf16's first term up to 256
    wb = S.split_weights_np(w, 64)
    assert wb.shape == (2, 2, 64, 3, 8)
    for sub, kc, n, pair in ((0, 0, 0, 0), (1, 1, 63, 7), (0, 1, 5, 3)):
        k = kc * 16 + 2 * pair
        a, b = w[sub * 64 + n, k], w[sub * 64 + n, k + 1]
        t = [S.bf16_value(x) for x in S.split3(np.array([a, b], np.float32))]
        for term in range(3):
            d = int(wb[sub, kc, n, term, pair])
            assert S.bf16_value(np.array([d & 0xffff, d >> 16], np.uint32)).tolist() == t[term].tolist()
    assert S.splitter_mismatch(S.split_weights_np(w, 64, swap_pairs=True), wb) == 0       # the pair-swap mutation shows in the first dword


def test_domain_edges_are_what_the_header_says():
    v = S.domain_edges()
    b = S.split3(v)
    # the upper half of the top binade: x1 = +-inf; the first residual x - x1 is the OTHER infinity (x is finite), the second inf - inf = NaN.
    # For x = +-inf itself the first residual is already NaN.  Either way a NaN term reaches the MFMA, as the header says.
    top = np.isfinite(v) & (np.abs(v) >= np.float32(3.3961775e38))
    assert top.sum() == 4 and np.all((b[0][top] & 0x7fff) == 0x7f80) and np.all(b[1][top] == (b[0][top] ^ 0x8000)) and np.all(S.bf16_is_nan(b[2][top]))
    inf = np.isinf(v)
    assert inf.sum() == 2 and np.all((b[0][inf] & 0x7fff) == 0x7f80) and np.all(S.bf16_is_nan(b[1][inf])) and np.all(S.bf16_is_nan(b[2][inf]))
    top = top | inf
    assert np.all(np.isfinite(S.bf16_value(b[0][~top])))
    sub = lambda bits: ((bits & 0x7f80) == 0) & ((bits & 0x7f) != 0)
    assert sub(b[1][~top]).any() and sub(b[2][~top]).any()                  # lower terms in bf16's subnormal range
    assert b[0][0] == 0 and b[0][1] == 0x8000                              # +-0 keep their sign in the first term


# ---- exact cases ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.EXACT_KINDS)
def test_exact_identity_holds_in_the_emulation(kind):
    ec = S.exact_case(kind)
    got = S.emulate_exact(ec)
    bad = S.bits_differ(got, ec.want) & ~((got == 0) & (ec.want == 0))
    assert not bool(bad.any()), lo.first_unequal(got, ec.want)
    big = ec.x if kind != "transposed" else ec.w
    mag = big[big != 0].abs().log2()
    assert mag.min() < -30 and mag.max() > 30                              # the 80 binades are there
    if kind == "select-3x3":
        assert bool((ec.want[:, :, 0, :][:, :16] == 0).all())              # tap (0, *) at the top border: exact zeros
    t3 = S.bf16_value(S.split3(big.numpy())[2])
    assert (t3 != 0).mean() > 0.9                                          # third terms alive: a lost x3 shows


def _k_of(kind, ec):
    """per output element [B, Co, H, W]: the k (position in the K-term sum) the selection takes its one term from"""
    B, _, H, W = ec.x.shape
    co = ec.w.shape[0]
    if kind == "transposed":
        m = torch.arange(B * H * W).view(B, 1, H, W)
        return (m % 128).expand(B, co, H, W)
    wk = ec.w.permute(0, 2, 3, 1).reshape(co, -1)
    return wk.ne(0).float().argmax(1).view(1, co, 1, 1).expand(B, co, H, W)


@pytest.mark.parametrize("mut,kind,klass", [
    ("x3-quarter3", "select-1x1", lambda k: k % 16 >= 12), ("x3-quarter3", "select-3x3", lambda k: k % 16 >= 12),
    ("x3-upper8", "select-1x1", lambda k: (k >= 24) & (k < 32)), ("w-chunk5", "transposed", lambda k: k % 16 >= 8),
])
def test_low_order_mutation_is_rejected_at_exactly_the_mutated_elements(mut, kind, klass):
    ec = S.exact_case(kind)
    got = S.emulate_exact(ec, mut)
    bad = S.bits_differ(got, ec.want) & ~((got == 0) & (ec.want == 0))
    k = _k_of(kind, ec)
    # the third term of the value an element selects: elements whose third term is zero lose nothing
    third = torch.from_numpy(S.bf16_value(S.split3(ec.want.numpy())[2])) != 0
    expect = klass(k) & third & (ec.want != 0)
    assert bool(expect.any()) and torch.equal(bad, expect), (int(bad.sum()), int(expect.sum()))
    assert S.ulp_distance(got, ec.want) <= 256                             # ... by a few low bits: nothing a norm sees


@pytest.mark.parametrize("kind", S.EXACT_KINDS)
def test_pair_swap_is_rejected_by_every_exact_case(kind):
    ec = S.exact_case(kind)
    bad = S.bits_differ(S.emulate_exact(ec, "pair-swap"), ec.want)
    assert float(bad.float().mean()) > 0.4


@pytest.mark.parametrize("mut", S.ACCEPTED_BY_BOUND)
@pytest.mark.parametrize("rid", PLAIN)
def test_bound_and_max_norm_accept_a_lost_third_term(rid, mut):
    """the reason the exact cases exist: on the plain rows the per-element bound -- and the max-norm criterion of tests/test_conv_hip.py --
    let a third term lost on one quarter, one half k-step or one weight chunk through"""
    case, o32, o64, emu = _ev(rid)
    got = S.emulate(case, mut)
    assert bool(S.bits_differ(got, emu).any())                             # the mutation did change the result
    w, fail = lo.judge(got, None, o64, "direct")
    print("\n%-14s %-12s worst err / (u A) %6.3f against c = %.1f (unmutated %6.3f); max|err| = %.1f x the float32 evaluation's" % (
        rid, mut, w.ratio, lo.c_for("direct", o64.K), lo.judge(emu, None, o64, "direct")[0].ratio, S.twice_f32_ratio(got, o32, o64)))
    assert fail is None and S.max_norm_accepts(got, o64)


@pytest.mark.parametrize("mut,rid", [("pair-swap", "plain-128x128"), ("pair-swap", "plain-64x64"), ("next-image", "plain-64x128"),
                                     ("next-image", "plain-128x64"), ("start-tap", "split2-64x64"), ("start-tap", "split4-128x128"),
                                     ("start-tap", "split3-5x5-64x64"), ("start-tap", "splitmax-128x128"), ("late-switch", "cat2-3x3-64x128"),
                                     ("late-switch", "cat2-3x3-128x64"), ("late-switch", "cat4-1x1-64x64")])
def test_gross_mutation_is_rejected_by_the_bound(mut, rid):
    case, _, o64, _ = _ev(rid)
    w, fail = lo.judge(S.emulate(case, mut), None, o64, "direct")
    assert fail is not None and w.ratio > 100 * lo.c_for("direct", o64.K)


# ---- the 32-bit quantities -----------------------------------------------------------------------------------------------------------------
SB_LIM = ("sb-3x3-s1", "sb-1x1")


def test_lim_rows_are_as_stated():
    a, b = (M.ROW[r] for r in SB_LIM)
    assert (a.kernel, a.p["cin"], a.p["c0"], a.p["cout"], a.p["res"]) == ("igemm_bf16x3_kernel<128, 64>", 16, 48, 40, False)
    assert (b.kernel, b.p["cin"], b.p["c0"], b.p["cout"], b.p["res"], b.p["k"]) == ("igemm_bf16x3_kernel<64, 64>", 32, 16, 40, True, 1)
    for r in (a, b):
        assert (r.p["c0"] * 4) % 16 == 0 and M.row_shape(r)["ldw"] % 64 == 0 and M.cdiv(r.p["cout"], 16) * 16 > 32      # eligible, not the c16 shape
        # what the row holds at once: source, output and residual, one image's snapshot for the second run
        px = M.LIM_B * M.LIM_H * M.LIM_W
        held = px * 4 * (M.LIM_LD + 52 * (2 if r.p["res"] else 1)) + px // 3 * 48 * 4
        one = px // 3 * 4 * (M.LIM_LD + 52 * (2 if r.p["res"] else 1))
        assert held <= M.MEM_LIMIT and (held - (px * 52 * 4 if r.p.get("res_host") else 0)) + one <= M.MEM_LIMIT


@pytest.mark.parametrize("rid", SB_LIM)
def test_split_bf16_offsets_at_the_limit(rid):
    row = M.ROW[rid]
    bm, bn = M.row_tile(row)
    s = M.row_shape(row)
    q = {x.name: x for x in M.audit("bf16x3", s, BM=bm, BN=bn)}
    assert all(x.fits for x in q.values())
    last = 2 ** 24 - 2
    assert q["aoff"].hi == (last * 64 + (12 if bm == 64 else 8)) * 4 and (1 << 32) - q["aoff"].hi in (464, 480)
    assert q["ps.boff = b*H*W"].hi == 2 * M.LIM_H * M.LIM_W and q["grid"].hi == M.cdiv(s["B"] * s["Ho"] * s["Wo"], bm) * (64 // bn)
    # one more column is refused by the byte check before anything of the kernel's overflows: slack, by one pixel
    wider = M.row_shape(row._replace(p=dict(row.p, W=row.p["W"] + 1)))
    assert not M.accepts("bf16x3", wider)
    square = M.shape(1, 4096, 4096, 64, row.p["cin"], row.p["k"], 1, row.p["pad"], 48, 64, 52)
    assert not M.accepts("bf16x3", square) and not M.overflows("bf16x3", square, BM=bm, BN=bn)
    over = M.shape(1, 4096, 4097, 64, row.p["cin"], row.p["k"], 1, row.p["pad"], 48, 64, 52)
    assert [x.name for x in M.overflows("bf16x3", over, BM=bm, BN=bn)] == ["aoff"]


VERDICT_SB = "conv bytes, for igemm_bf16x3_kernel: slack by one pixel, as for the generic kernel (exactly 2^24 pixels at ld = 64 are refused; " \
             "the largest aoff there is 2^32 - 208 with quarter staging and 2^32 - 224 with half staging, whose second float4 lies 16 bytes " \
             "further on through the 64-bit pointer: the last byte read ends 192 bytes below 2^32 either way); conv pixels dead, conv rows slack"


def test_verdict_for_the_split_kernel():
    """`conv bytes` is slack, not tight, for this kernel as for the generic one: the first refused shape overflows nothing of it"""
    for bm, below in ((64, 208), (128, 224)):
        s = M.shape(1, 4096, 4096, 64, 16, 1, 1, 0, 48, 64, 52)
        assert [c.name for c in M.checks("bf16x3", s) if not c.ok] == ["conv bytes[0]"]
        q = {x.name: x for x in M.audit("bf16x3", s, BM=bm, BN=64)}
        assert q["aoff"].fits and (1 << 32) - q["aoff"].hi == below
        assert (1 << 32) - (q["aoff"].hi + (16 if bm == 64 else 32)) == 192                 # the end of the last float4 the thread loads
    assert "slack by one pixel" in VERDICT_SB and "2^32 - 208" in VERDICT_SB and "2^32 - 224" in VERDICT_SB


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(5)
    x = np.maximum(rng.standard_normal((3, 11, 31, 16)), 0).astype(np.float32) + np.float32(0.01)
    return x, rng.standard_normal((3, 3, 16))


@pytest.mark.parametrize("slot", [4, 8])
def test_offsets_at_16_bits(small, slot):
    """LIM scaled to 16 bits (3 x 11 x 31 pixels of 16 floats: 2^16 - 64 bytes): the kernel's unsigned offset, in quarter (slot 4) and half
    (slot 8) staging, passes crops and translation; the same offset made SIGNED is rejected by both"""
    x, wts = small
    s = M.shape(3, 11, 31, 16, 16, 3, 1, 1, 48, 64, 52, lds=[16])
    assert M.accepts("bf16x3", s, 16) and not M.overflows("bf16x3", s, 16, BM=64 if slot == 4 else 128, BN=64)
    ref = lambda t: M.reference_generic(t, wts)
    assert M.judge_emulation(lambda t: M.emulate_generic(t, wts, 16, slot=slot), ref, x) == dict(crops=True, translation=True)
    assert M.judge_emulation(lambda t: M.emulate_generic(t, wts, 16, "signed", slot=slot), ref, x) == dict(crops=False, translation=False)


def test_refusal_table():
    assert [r.id for r in S.REFUSALS] == ["splitk-two-sources", "splitk-nsub4", "splitk-too-many", "source-misaligned", "ld-not-4", "ldw-not-BN",
                                          "unknown-tile"]
