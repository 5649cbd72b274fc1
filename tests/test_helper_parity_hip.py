"""The bandwidth-bound helpers of csrc/elementwise.hip, one stand-alone launch per row of `helper_oracle.ROWS`, element by element
against a plain-torch CPU reference, in every launch-geometry regime (tests/helper_oracle.py).

The stand-alone helper tests of tests/test_conv_hip.py and the plans of tests/test_layer_parity_hip.py stay at maps where a row of
Wo * C/4 float4s fits one 256-element x-block, `rows` stays under the 65535 grid rows and no flat kernel takes a second grid-stride
iteration.  Here every launcher runs with >= 3 x-blocks and a ragged tail (XN), with the row loop taken twice and three times (YS), at
the last shape its "row too large" check accepts (LIM: the multiply-high division one pixel before it goes wrong), on channel slices of
wider buffers and in place (VIEW), and every flat launcher with two and three grid-stride iterations (FLAT).  Asserted per row:

* `Launch.kernel` names the kernel the row is for, where the launcher records one;
* bit-equality with the float32 CPU evaluation (max-pool, scale_add, shuffle_concat, the transposes, fill, dcn_pack, the up-sampling
  sums, flip_merge), or |out - ref64| <= c u A per element with c = layer_oracle.c_for("direct", K): K = 5 for the deconvolutions (as
  emit_up_add), k^2 + 4 for dwconv (`_affine`), ceil(HW / 8) + 8 for the average pool (its longest addition chain plus the division);
* nothing stored outside the view (NaN guards: channels past C, an image before and after), exact zeros in padding the kernel owns,
  no poison read (inputs are views into NaN / +inf buffers), the same bits from a second run;
* `CP_DWDECONV2` = 1 / 0 bit-identical (twin rows), the grouped up-sampling sum bit-identical to one launch per member.

`helper_oracle.MUST_COVER` lists every (launcher, regime) pair.  (`maxpool_nhwc_kernel` and the generic `dw_deconv_add_kernel` are
dispatched by the 64 x 96 plans of tests/test_layer_parity_hip.py too -- res_50's stem pool, DLA-34's one f > 2 up-sampling -- and are
in its MUST_COVER; here they run in the regimes those plans do not reach.)  The refusal tests give every call real
buffers large enough for whatever an unrefused launch would touch.  Run with -s for the worst err / (u A) per row and launcher.
"""
import pytest
import torch

import helper_oracle as H

pytestmark = pytest.mark.gpu

_reports = {}
_TWINNED = {r.p["twin"] for r in H.ROWS if "twin" in r.p} | {r.id for r in H.ROWS if "twin" in r.p}


def _report(rid):
    """the report of row `rid`, run once per module; a row that raised raises again for whoever asks"""
    if rid not in _reports:
        try:
            _reports[rid] = H.run_row(rid, keep=rid in _TWINNED)
        except Exception as e:                    # noqa: BLE001 -- kept, so that the coverage test fails with it rather than run it again
            _reports[rid] = e
    if isinstance(_reports[rid], Exception):
        raise _reports[rid]
    return _reports[rid]


def _line(rid, rep):
    w = rep["worst"]
    return "%-26s %-15s %-22s %s" % (rid, H.ROW[rid].launcher, rep["kernel"] or "-",
                                     "bit-equal" if w is None else "worst err / (u A) %.3f (c = %.1f) at %s" % (w.ratio, rep["c"], w.loc))


@pytest.mark.parametrize("rid", [r.id for r in H.ROWS])
def test_helper_matches_reference(rid):
    row, rep = H.ROW[rid], _report(rid)
    print("\n" + _line(rid, rep))
    assert rep["kernel"] == row.kernel
    assert (rep["worst"] is None) == H.is_exact(row)
    assert not rep["failures"], "\n".join(rep["failures"])


@pytest.mark.parametrize("rid", [r.id for r in H.ROWS if "twin" in r.p])
def test_deconv_kernels_are_bit_identical(rid):
    """CP_DWDECONV2 = 0 (generic kernel) against = 1 (the f = 2 kernel) on the same data"""
    a, b = _report(rid), _report(H.ROW[rid].p["twin"])
    assert (a["kernel"], b["kernel"]) == (H.GENERIC, H.DECONV2)
    assert torch.equal(a["outs"][0], b["outs"][0]), H.lo.first_unequal(a["outs"][0], b["outs"][0])


def test_every_launcher_regime_is_covered():
    """every (launcher, regime) pair of MUST_COVER has a row that ran; a row that has not run yet runs here, one that raised fails this
    test too"""
    reps = {r.id: _report(r.id) for r in H.ROWS}
    covered = {(H.ROW[rid].launcher, g) for rid in reps for g in H.ROW[rid].regimes}
    missing = [pair for pair in H.MUST_COVER if pair not in covered]
    assert not missing, missing
    worst = {}
    for rid, rep in reps.items():
        if rep["worst"] is not None and rep["worst"].ratio > worst.get(H.ROW[rid].launcher, (-1.0, "", 0))[0]:
            worst[H.ROW[rid].launcher] = (rep["worst"].ratio, rid, rep["c"])
    for launcher, (ratio, rid, c) in sorted(worst.items()):
        print("\nworst err / (u A) %-15s %8.3f (c = %.1f)  %s" % (launcher, ratio, c, rid))


@pytest.mark.parametrize("rid", [r.id for r in H.REFUSALS if r.gpu])
def test_launcher_refuses(rid):
    r = H.REFUSAL[rid]
    rc, msg = H.refuse(rid, device=True)
    assert rc == 1, (rc, msg)
    assert msg.startswith(r.launcher + ":") and r.arg in msg, msg


def test_ops_mirror_the_divisibility_check():
    from centerpose_amd import ops
    out = torch.zeros(2, 5, 4, 8, device="cuda")
    src = torch.zeros(3, 2, 2, 8, device="cuda")[:2]                      # one spare image
    with pytest.raises(AssertionError, match="must divide"):
        ops.sum_up_launch([src], [1], out, True)
    with pytest.raises(AssertionError, match="must divide"):
        ops.sum_up_group_launch([([src], [1], out)], out, True)
