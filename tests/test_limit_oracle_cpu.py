"""The 32-bit offset checks of the hot-path launchers, held against the restated index arithmetic (tests/limit_oracle.py).  No device.

* every row of `limit_oracle.ROWS` sits at LIM: its shape is accepted, one more column is refused, and so is exactly 2^24 pixels at
  ld = 64 (the comparison is `<`); the audit reports no overflow there, for the stems' own LIM shapes and for tier two likewise;
* `VERDICTS` records for every check whether it is tight, conservative (and by how much) or dead behind another check, and every entry is
  asserted from the restated arithmetic, not taken as given;
* the defects the audit found are reproduced against the checks as they stood and shown closed by the present ones: the NCHW producer's
  `boff = b*C*H*W`, the F(2x4) lean epilogue's `(4*it + aa) * ostep`, head_points' `H*W`;
* teeth: at 16 bits numpy emulations of the generic producer and of the DCN record run at the correspondingly scaled limit shape
  (3 x 11 x 31 pixels at ld = 16: 2^10 - 1 pixels, 2^16 - 64 bytes); a signed offset, a field one bit short and a per-image base formed in
  the narrow type are each rejected by the judged set AND by the translation check, and an error in the interior of image 2 alone is
  caught by the translation check only;
* where no device is present, the first refused shape of every launcher comes back through the C ABI with rc 1 and its message.
"""
import ctypes

import numpy as np
import pytest
import torch

import limit_oracle as M

NO_DEVICE = not torch.cuda.is_available()
HALF, FULL = 1 << 31, 1 << 32


def _fam(row):
    return "generic" if row.audit == "group" else row.audit


# ---- LIM ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", [r.id for r in M.ROWS])
def test_row_sits_at_the_limit(rid):
    row = M.ROW[rid]
    s = M.row_shape(row)
    assert s["B"] * s["H"] * s["W"] == 2 ** 24 - 1 and all(ld == 64 for ld in s["lds"])
    assert M.accepts(_fam(row), s), [c for c in M.checks(_fam(row), s) if not c.ok]
    wider = dict(row.p, W=row.p["W"] + 1)                                  # the binding dimension's smallest step: one more column
    assert not M.accepts(_fam(row), M.row_shape(row._replace(p=wider)))
    square = dict(row.p, B=1, H=4096, W=4096)                              # exactly 2^24 pixels: the comparison is `<`
    refused = [c for c in M.checks(_fam(row), M.row_shape(row._replace(p=square))) if not c.ok]
    assert refused and all(c.value == c.limit for c in refused if "bytes" in c.name), refused


@pytest.mark.parametrize("rid", [r.id for r in M.ROWS])
def test_audit_reports_no_overflow_at_the_limit(rid):
    row = M.ROW[rid]
    bm, bn = M.row_tile(row)
    for B in (3, 1):                                                      # the LIM launch and the stand-alone image
        qs = M.audit(row.audit, M.row_shape(row, B), BM=bm, BN=bn)
        assert qs and not [q for q in qs if not q.fits], [q for q in qs if not q.fits]


def test_lim_straddles_byte_2_31():
    b, y, x = M.crossing(M.LIM_H, M.LIM_W, M.LIM_LD)
    assert (b, y, x) == (1, 682, 2049)                                    # image 1 straddles, image 2 lies wholly above
    assert 2 * M.LIM_H * M.LIM_W * M.LIM_LD * 4 > HALF
    for th, tw in ((8, 16), (8, 32), (16, 16), (8, 64)):
        assert M.LIM_H % th and M.LIM_W % tw
    crops = M.judged_crops(3, M.LIM_H, M.LIM_W, 8, 16, y)
    mask_rows = {(b_, y0, y1) for b_, y0, y1, _, _ in crops}
    assert (1, 672, 696) in mask_rows and (2, 0, 16) in mask_rows and (0, 0, 16) in mask_rows and (2, 1352, 1365) in mask_rows


def test_stem_limit_shapes():
    for p, fam in ((M.STEM_LIM, "stem7_c16"), (M.STEM_LIM_SCALAR, "stem7")):
        n = p["B"] * 3 * p["H"] * p["W"]
        step = 4 if fam == "stem7_c16" else 1                             # the persistent kernel takes whole float4 quads
        assert n < HALF <= p["B"] * 3 * p["H"] * (p["W"] + step) and p["H"] % 8 and p["W"] % 64 and (p["W"] % 4 == 0) == (fam == "stem7_c16")
        for cout, stride in ((16, 1), (64, 2), (16, 2), (64, 1)):
            s = M.shape(p["B"], p["H"], p["W"], 0, 3, 7, stride, 3, cout, cout, cout, nchw=True)
            assert M.accepts(fam, s) and not M.overflows(fam, s)
        # the narrowest output of a stem launch at this shape plus its input: why no stem row runs at LIM
        assert n * 4 + p["B"] * ((p["H"] + 1) // 2) * ((p["W"] + 1) // 2) * 16 * 4 > M.MEM_LIMIT
    s = M.shape(3, M.STEM_LIM_SCALAR["H"], M.STEM_LIM_SCALAR["W"], 0, 3, 3, 2, 1, 64, 64, 64, nchw=True)
    assert M.accepts("generic_stem", s) and not M.overflows("generic_stem", s, BM=128, BN=64)


# ---- the defects the audit found -------------------------------------------------------------------------------------------------------
def test_nchw_image_base_overflowed_at_an_accepted_shape():
    s = M.shape(2, 26755, 26755, 0, 3, 3, 2, 1, 64, 64, 64, nchw=True)
    assert M.accepts("generic_stem", s, fixed=False)                       # B*H*W = 1 431 660 050 < 2^31 was the only check
    bad = M.overflows("generic_stem", s, BM=128, BN=64)
    assert [q.name for q in bad] == ["boff = b*C*H*W"] and bad[0].hi == 2147490075 > HALF - 1
    assert M.wrap(bad[0].hi, "int", 32) < 0                                # `boff >= 0` fails: image 1 read as zeros, no error
    assert not M.accepts("generic_stem", s)                                # refused now
    # and whatever the present checks accept fits: the largest accepted NCHW source
    for B, C, H, W in ((2, 3, 26754, 13377), (1, 3, 26754, 26755), (3, 3, 4098, 58225), (1, 1, 46340, 46341)):
        s = M.shape(B, H, W, 0, C, 3, 1, 1, 16, 16, 16, nchw=True)
        assert M.accepts("generic_stem", s) and not M.overflows("generic_stem", s, BM=256, BN=16), (B, C, H, W)


def test_wino24_lean_epilogue_row_offset_overflowed_at_an_accepted_shape():
    """B = 1, 14 x 45 000, 16 -> 32 channels written into a 4096-float-wide buffer: 13 output rows further down is 13 * W * outLd =
    2 396 160 000 floats in `int`"""
    s = M.shape(1, 14, 45000, 16, 16, 3, 1, 1, 32, 64, 4096)
    assert all(c.ok for c in M.checks("wino24", s) if "x16" not in c.name)                       # every other check passes
    assert s["W"] * s["outLd"] * 8 < HALF                                  # ... and so did the lean epilogue's rule as it stood (x 8)
    bad = M.overflows("wino24", s)
    assert [q.name for q in bad] == ["(4*it+aa) * ostep"]
    assert not M.accepts("wino24", s)                                      # x 16 now: the launch takes the general epilogue (size_t rows)
    edge = M.shape(1, 14, (HALF // 16 - 1) // 4096, 16, 16, 3, 1, 1, 32, 64, 4096)
    assert M.accepts("wino24", edge) and not M.overflows("wino24", edge)


def test_head_points_plane_index_overflowed_at_an_accepted_shape():
    p = dict(N=1, H=65536, W=32768, J=1, K=1)
    for kind in ("head_points", "head_points_pairs"):
        assert all(c.ok for c in M.checks_tier2(kind, fixed=False, **p))
        assert [q.name for q in M.audit_tier2(kind, **p) if not q.fits] == ["HW = H*W"]
        assert not all(c.ok for c in M.checks_tier2(kind, **p))
    p = dict(N=1 << 16, H=1 << 15, W=1, J=1, K=1)
    assert all(c.ok for c in M.checks_tier2("head_points", fixed=False, **p)) and not all(c.ok for c in M.checks_tier2("head_points", **p))
    assert [q.name for q in M.audit_tier2("head_points", **p) if not q.fits] == ["(b*H + yy)"]


# ---- tight, conservative or dead: every check -------------------------------------------------------------------------------------------
# verdict: "tight" = the first refused shape overflows a quantity; "slack" = it does not (by how much: see the test); "dead" = another
# check of the same path always refuses first.
VERDICTS = {
    "conv bytes": "slack: one pixel (the last pixel's float4 ends 192 bytes below the limit when the count is refused)",
    "conv bytes (igemm_bf16x3_kernel)": "slack: one pixel, as above (largest aoff at the refused count 2^32 - 208 with quarter, 2^32 - 224 with half staging; "
                                        "tests/test_bf16x3_oracle_cpu.py::test_verdict_for_the_split_kernel)",
    "conv pixels": "dead: behind conv bytes (NHWC, ld >= 16: 2^26 pixels) and behind conv nchw floats (C >= 1)",
    "conv rows": "slack: 255 rows (a.M itself first overflows at 2^31; the last 256-row block's index stays below it until then)",
    "conv nchw floats": "slack: one image plane (boff = (B - 1) C H W); the stem kernels' s_g needs less",
    "dcn pixels": "dead: behind dcn bytes at ld >= 16 (2^26 pixels)",
    "dcn bytes": "slack: one pixel; the 28-bit field holds pixel * ld / 4 < 2^28 exactly when the bytes fit 32 bits",
    "source floats": "dead: conv bytes already keeps pixel * ld below 2^30",
    "grid x dmax": "tight within 0.4 % for divisors 2^k + 1 (257 tile columns), slack up to d / 2 otherwise",
    "c16 out row x16": "slack x 16: orow = Wo * outLd is the only int product",
    "w24 out row x16": "slack x 16 / 13: the lean epilogue reaches 13 rows down; x 8 (before) was WRONG",
    "pw bytes": "dead: the same product as conv bytes (H = Ho, W = Wo), and pw_conv_kernel forms every offset in size_t",
    "stem floats": "slack: the image base is 64-bit (stem7x7.hip:171); s_g needs only 3 H W < 2^31",
    "decode cat*H*W": "tight: the flat index is an int",
    "flip_pairs N*C*H*W": "tight: t reaches 2^31 - 1 in the last block",
    "head_points H*W": "tight: HW is an int (added by this audit; the 2^40 element check guarded another product)",
}


def test_byte_offset_check_has_one_pixel_of_slack():
    for fam, kw in (("generic", dict(BM=256, BN=16)), ("dcn", dict(BM=128, BN=32))):
        for ld in (16, 64, 256):
            n = FULL // (ld * 4)                                          # the first refused pixel count
            at = M.shape(1, 2, n // 2, ld, 16, 1, 1, 0, 16, 32, 20, lds=[ld])
            assert not M.accepts(fam, at) and not M.overflows(fam, at, **kw)      # refused, yet nothing would overflow
            assert M.accepts(fam, M.shape(1, 1, n - 1, ld, 16, 1, 1, 0, 16, 32, 20, lds=[ld]))
            over = M.shape(1, 1, n + 1, ld, 16, 1, 1, 0, 16, 32, 20, lds=[ld])
            names = {q.name for q in M.overflows(fam, over, **kw)}
            assert names and names <= {"aoff", "s_code offset field", "o00", "o01, o10, o11", "rowb"}, names
    q = {x.name: x for x in M.audit("generic", M.shape(1, 1, FULL // 256, 64, 16, 1, 1, 0), BM=256, BN=16)}
    assert FULL - (q["aoff"].hi + 16) == 256 - 64 == 192


def test_dead_checks_never_bind():
    for ld in (16, 20, 64, 1024):
        npix = (FULL - 1) // (ld * 4)                                      # the most pixels the byte checks accept
        assert npix < 1 << 26 < 1 << 29 < HALF                             # "dcn pixels", "conv pixels" (NHWC)
        assert npix * ld < 1 << 30                                        # "source floats" (Winograd, patch, c16, heads): limit 2^31
    # NCHW: B C H W < 2^31 with C >= 1 implies B H W < 2^31
    s = M.shape(1, 46341, 46341, 0, 1, 3, 1, 1, 16, 16, 16, nchw=True)
    failed = [c.name for c in M.checks("generic_stem", s) if not c.ok]
    assert "conv pixels" in failed and "conv nchw floats" in failed         # never the pixel check alone
    # pw: same product as conv bytes, and no 32-bit quantity of its own
    row = M.ROW["pw"]
    ch = {c.name: c for c in M.checks("pw", M.row_shape(row))}
    assert ch["pw bytes"].value == ch["conv bytes[0]"].value
    assert [q.name for q in M.audit("pw", M.row_shape(row), BM=64, BN=64)] == ["a.M = B*Ho*Wo", "m = m0 + row", "grid"]


def test_row_and_grid_checks():
    # conv rows: B*Ho*Wo + 255 < 2^31 is 255 rows short of what a.M and the last 256-row block need
    s = M.shape(1, 1, 1 << 20, 16, 16, 1, 1, 0, lds=[16])
    for M_, ok, bad in ((HALF - 256, True, []), (HALF - 255, False, []), (HALF - 1, False, []), (HALF, False, ["a.M = B*Ho*Wo"])):
        s.update(Ho=1, Wo=M_)
        assert M.accepts("generic", s) == ok
        assert [q.name for q in M.overflows("generic", s, BM=256, BN=16) if q.ctype == "int"] == bad, M_
    # mulhi divisions: exact up to magic_exact_upto(d), which the closed form gets right at both edges
    for d in (2, 3, 7, 86, 171, 257, 4097, 65537):
        up = M.magic_exact_upto(d)
        assert M.magic_div(up, d) == up // d and (up == FULL - 1 or M.magic_div(up + 1, d) != (up + 1) // d)
        assert up * d >= FULL - d                                           # n d < 2^32 is sufficient: what the launchers check
        for n in (0, 1, d - 1, d, up - 1, up // 2, FULL // d - 1):
            assert n > up or M.magic_div(n, d) == n // d
    assert M.magic_exact_upto(257) * 257 < 1.004 * FULL and M.magic_exact_upto(171) * 171 > 5 * FULL
    # c16 / wino24 row products
    s = M.shape(1, 8, (HALF // 16 - 1) // 20, 16, 16, 3, 1, 1, 16, 16, 20)
    assert M.accepts("c16", s) and M.audit("c16", s)[3].name == "orow = Wo*outLd" and M.audit("c16", s)[3].hi * 16 < HALF


def test_nchw_and_stem_float_checks_are_slack():
    """the first NCHW source the float check refuses overflows nothing: boff = (B - 1) C H W is one image short of the count; and the
    persistent stems, whose image base is 64-bit, need only s_g < 3 H W"""
    s = M.shape(2, 32768, 8192, 0, 4, 3, 1, 1, 16, 16, 16, nchw=True)      # B C H W = 2^31 exactly
    assert [c.name for c in M.checks("generic_stem", s) if not c.ok] == ["conv nchw floats"]
    assert not M.overflows("generic_stem", s, BM=256, BN=16)
    q = {x.name: x for x in M.audit("generic_stem", s, BM=256, BN=16)}
    assert q["boff = b*C*H*W"].hi == HALF // 2                             # (B - 1) / B of the count
    s = M.shape(2, 32768, 8192 + 2731, 0, 4, 3, 1, 1, 16, 16, 16, nchw=True)
    assert (s["B"] - 1) * 4 * s["H"] * s["W"] < HALF <= s["B"] * 4 * s["H"] * s["W"] and not M.overflows("generic_stem", s, BM=256, BN=16)
    p = M.STEM_LIM
    for W in (p["W"] + 4, 2 * p["W"]):                                     # refused for the persistent kernel, yet nothing of it would overflow
        s = M.shape(3, p["H"], W, 0, 3, 7, 1, 3, 16, 16, 16, nchw=True)
        assert not M.accepts("stem7_c16", s) and not M.overflows("stem7_c16", s)
    s = M.shape(1, 32768, 32768, 0, 3, 7, 1, 3, 16, 16, 16, nchw=True)      # (2 H + 13) W >= 2^31: s_g itself
    assert [x.name for x in M.overflows("stem7_c16", s)] == ["s_g = (c*H + py)*W + f*4"]


def test_group24_total_blocks_check():
    """conv3x3_wino24.hip:472: the members' blocks summed must stay below 2^31 (first[] and blockIdx are int); per member blocks * d < 2^32"""
    row = M.ROW["group-wino24"]
    lim, small = M.row_shape(row), M.shape(2, 19, 37, 32, 32, 3, 1, 1, 40, 64, 52)
    c = M.group24_total([lim, small])
    assert c.ok and c.value == 3 * 257 * 86 * 1 + 2 * 3 * 2 * 2
    # dead behind the members' own checks: a member has < 2^26 spatial tiles (byte check, ld >= 16) times ntb channel tiles, and
    # blocks * max(ntb, ..) < 2^32 -- either way fewer than 2^29 blocks, so four members stay below 2^31
    assert all(min((1 << 26) * ntb, (FULL - 1) // ntb) < 1 << 29 for ntb in range(1, 1 << 12))
    assert not M.group24_total([dict(lim, B=1 << 22)] * 4).ok               # the restated check itself does refuse


def test_tier_two_limits():
    """decode, flip_pairs, head_points: restated, tight-or-slack, no GPU row (their LIM maps are far above the memory condition)"""
    d = dict(cat=2, H=32768, W=32767)
    assert all(c.ok for c in M.checks_tier2("decode", **d)) and not [q for q in M.audit_tier2("decode", **d) if not q.fits]
    assert not all(c.ok for c in M.checks_tier2("decode", cat=2, H=32768, W=32768))
    assert [q.name for q in M.audit_tier2("decode", cat=2, H=32768, W=32768) if not q.fits] == ["nbig = cat*H*W"]        # tight
    assert d["cat"] * d["H"] * d["W"] * 4 * (1 + 34 / 2) > M.MEM_LIMIT     # hm alone is 8 GiB; hps drags 34 channels with it
    f = dict(N=1, C=1, H=1, W=HALF - 1)
    assert all(c.ok for c in M.checks_tier2("flip_pairs", **f))
    q = {x.name: x for x in M.audit_tier2("flip_pairs", **f)}
    assert q["t"].fits and q["t"].hi == HALF - 1                           # tight: the last thread of the last block
    assert not all(c.ok for c in M.checks_tier2("flip_pairs", N=1, C=2, H=32768, W=32768))
    h = dict(N=1, H=46340, W=46341, J=17, K=100)
    for kind in ("head_points", "head_points_pairs"):
        assert all(c.ok for c in M.checks_tier2(kind, **h)) and not [x for x in M.audit_tier2(kind, **h) if not x.fits]


def test_every_check_has_a_verdict():
    names = set()
    for row in M.ROWS:
        names |= {c.name.split("[")[0].replace("w24 res", "w24 out").replace("c16 res", "c16 out") for c in M.checks(_fam(row), M.row_shape(row))}
    names |= {c.name for c in M.checks("generic_stem", M.shape(nchw=True, C=3))} | {"stem floats"}
    names -= {"c16 tiles", "stem tiles"}                                   # tile counts: far below 2^31 whenever the pixel checks pass
    assert names <= set(VERDICTS), names - set(VERDICTS)


# ---- teeth: 16-bit emulations -----------------------------------------------------------------------------------------------------------
W16 = 16
SB, SH, SW, SLD = 3, 11, 31, 16            # 1023 = 2^10 - 1 pixels, 2^16 - 64 bytes: LIM scaled to 16 bits


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(5)
    x = np.maximum(rng.standard_normal((SB, SH, SW, SLD)), 0).astype(np.float32) + np.float32(0.01)      # no zeros: a wrong pixel shows
    wts = rng.standard_normal((3, 3, SLD))
    return x, wts


def test_scaled_limit_shape_is_the_16_bit_lim():
    s = M.shape(SB, SH, SW, SLD, 16, 3, 1, 1, lds=[SLD])
    assert SB * SH * SW == 2 ** 10 - 1 and SB * SH * SW * SLD * 4 == 2 ** 16 - 64
    assert M.accepts("generic", s, W16) and not M.accepts("generic", dict(s, W=SW + 1), W16)
    assert M.accepts("dcn", s, W16) and not M.overflows("generic", s, W16, BM=64, BN=16) and not M.overflows("dcn", s, W16, BM=64, BN=16)
    assert [q.name for q in M.overflows("dcn", s, W16, BM=64, BN=16, field=11)] == ["s_code offset field"]
    b, y, _ = M.crossing(SH, SW, SLD, W16)
    assert b == 1 and 0 < y < SH - 1


def test_faithful_emulations_pass_both_checks(small):
    x, wts = small
    assert M.judge_emulation(lambda t: M.emulate_generic(t, wts, W16), lambda t: M.reference_generic(t, wts), x) == dict(crops=True, translation=True)
    assert M.judge_emulation(lambda t: M.emulate_dcn(t, W16), M.reference_dcn, x) == dict(crops=True, translation=True)


@pytest.mark.parametrize("mutation", ["signed", "narrow_base"])
def test_generic_producer_mutation_is_rejected(small, mutation):
    x, wts = small
    got = M.judge_emulation(lambda t: M.emulate_generic(t, wts, W16, mutation), lambda t: M.reference_generic(t, wts), x)
    assert got == dict(crops=False, translation=False), got


def test_dcn_field_one_bit_short_is_rejected(small):
    x, _ = small
    got = M.judge_emulation(lambda t: M.emulate_dcn(t, W16, field=11), M.reference_dcn, x)
    assert got == dict(crops=False, translation=False), got
    # ... by wrong numbers, not by a fault: every wrapped offset lands inside the tensor
    assert np.isfinite(M.emulate_dcn(x, W16, field=11)).all()


def test_interior_error_of_image_2_is_caught_by_translation_only(small):
    x, wts = small
    crops = M.judged_crops(SB, SH, SW, 2, 8, M.crossing(SH, SW, SLD, W16)[1])
    y, xx = next((y, xx) for y in range(SH) for xx in range(SW) if not M.in_crops(crops, (SB, SH, SW))[2, y, xx])

    def run(t):
        out = M.emulate_generic(t, wts, W16)
        if t.shape[0] == SB:                                               # wrong only inside the 3-image launch, at one interior pixel of image 2
            out[2, y, xx] += 1.0
        return out
    ref = lambda t: M.reference_generic(t, wts)
    assert M.judge_emulation(run, ref, x) == dict(crops=True, translation=False)
    assert M.judge_emulation(run, ref, x, ends_only=True, translate=False) == dict(crops=True)


# ---- refusals through the C ABI, where no launch can happen ------------------------------------------------------------------------------
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


@pytest.mark.parametrize("rid", [r for r in M.REFUSAL_IDS if r not in M.DEVICE_ONLY])
def test_launcher_refuses_the_first_shape_past_its_limit(rid, no_launch_possible):
    r = M.refusal(rid)
    rc, msg, _ = M.refuse(r, device=False)
    assert rc == 1, (rc, msg)
    assert msg.startswith(r.launcher + ":") and r.arg in msg, msg


def test_ops_refuse_an_nchw_source_past_the_element_index():
    from centerpose_amd import ops
    x = torch.empty(1).expand(2, 3, 26755, 26755)                          # one float of storage: only the shape is looked at
    with pytest.raises(AssertionError, match="NCHW source"):
        ops.conv2d_launch([x], torch.zeros(64, 32), torch.zeros(64), torch.zeros(64), torch.zeros(1), kh=3, kw=3, stride=2, pad=1, cout=64, in_nchw=True)
