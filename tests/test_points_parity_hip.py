"""The detections-only head kernels of csrc/head_points.hip -- head_points_kernel<1> / <2> (cp_head_points_f32) and
head_points_pairs_kernel<1> / <2> (cp_head_points_pairs_f32) -- one stand-alone launch per case of `points_oracle.CASES`, element by
element against float64, and the single points launch of the detections-only plans judged from its own device inputs.

tests/test_head_points_hip.py and tests/test_flip_dets_only_hip.py keep their max-norm criterion at one geometry on dense features.  Here
the one-wave block (hc = 32), block widths that are no power of two (192, 320, 448 threads), C = 16 and 48, the > 64 KiB LDS reservation
(C = hc = 512), K = 256, tiles with a single live point, J = 1 / 4 / 17, 1 x 1, 1 x 5 and 5 x 1 maps, a negative index, an index in class
plane 3 and a channel-slice `feat` (featLd > C, NaN on every side) run for both entry points.  Asserted per case:

* the dispatched kernel (`Launch.kernel`, i.e. cp_last_kernel) is the instantiation `points_oracle.geometry` names;
* |out - ref64| <= c_for("direct", K) u A at every addressed element, NaN at every element that is not addressed, NaN guards, the
  feature buffer untouched;
* the same bits from a second run and from a shuffled, duplicate-padded point list;
* the liveness floors of the row's own data.

MIRROR-3CYC additionally holds the pairs kernel bit for bit to cp_flip_merge_pairs_f32 applied to two dense sets of maps of
cp_head_points_f32 under a permutation that is not its own inverse.  Nothing here launches a block wider than 512 threads: the refused
head_conv values come back with rc 1 on real buffers that stay untouched.  Run with -s for the worst err / (u A) per case.
"""
import ctypes

import pytest
import torch

import layer_oracle as lo
import points_oracle as P

pytestmark = pytest.mark.gpu

_reports = {}


def _report(key, run):
    """the report of case `key`, run once per module; a case that raised raises again for whoever asks"""
    if key not in _reports:
        try:
            _reports[key] = run()
        except Exception as e:                    # noqa: BLE001 -- kept, so that the coverage test fails with it rather than run it again
            _reports[key] = e
    if isinstance(_reports[key], Exception):
        raise _reports[key]
    return _reports[key]


def _case_report(cid):
    return _report(cid, lambda: P.run_case(cid))


@pytest.mark.parametrize("cid", P.CASES)
def test_points_launch_matches_reference(cid):
    rep = _case_report(cid)
    case = P.make_case(cid)
    print("\n" + P.report_line(cid, rep))
    assert rep["kernel"] == case.geo["kernel"]
    assert not rep["failures"], "\n".join(rep["failures"])
    assert P.worst_of(rep).ratio <= rep["c"] == lo.LAYER_TOL["direct"]
    assert rep["rerun_equal"], "a second run gave other bits"
    assert rep["shuffle_equal"], "the shuffled, duplicate-padded point list (K = %d) gave other bits" % rep["K2"]
    assert rep["featbuf_intact"]
    assert P.RELU_SHARE[0] < rep["relu_share"] < P.RELU_SHARE[1] and rep["hps_live"] > P.HPS_LIVE[1]


def test_every_instantiation_is_covered():
    """every kernel of MUST_COVER was dispatched by a case that ran; a case that has not run yet runs here, one that raised fails this
    test too"""
    reps = {cid: _case_report(cid) for cid in P.CASES}
    seen = {rep["kernel"] for rep in reps.values()}
    assert set(P.MUST_COVER) <= seen, sorted(set(P.MUST_COVER) - seen)
    for kern in P.MUST_COVER:
        ratio, cid = max((P.worst_of(rep).ratio, cid) for cid, rep in reps.items() if rep["kernel"] == kern)
        print("\nworst err / (u A) %-30s %8.3f (c = %.2f)  %s" % (kern, ratio, lo.LAYER_TOL["direct"], cid))


def test_pairs_gather_direction_against_the_dense_merge():
    """J = 4 under the 3-cycle (1, 2, 0, 3): which way the permutation is applied shows (an involution hides it).  The merged values of
    the pairs kernel are the bits cp_flip_merge_pairs_f32 makes of the dense maps cp_head_points_f32 writes for all 2N images."""
    cid = "mirror-3cyc/pairs"
    case = P.make_case(cid)
    got = P.split_flat(_case_report(cid)["flat"], case.row)[0]
    want = P.dense_merged_by_existing_kernels(cid)
    for name in P.SPARSE:
        mask = P.addressed(case.row, case.inds, name).expand_as(got[name])
        assert bool(torch.isfinite(want[name]).all()), name
        assert torch.equal(got[name][mask], want[name][mask]), "%s: %d of %d values differ" % (
            name, int((got[name][mask] != want[name][mask]).sum()), int(mask.sum()))


# ---- plans ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,flip", P.PLAN_CASES)
def test_plan_points_launch_matches_reference(arch, flip):
    """the ONE points launch of a detections-only plan (B = 2 at 64 x 96, resp. 2N = 4 under the flip test) on the spread checkpoint:
    physical channel padding through expand_in, featLd from the pooled buffer, inds from the plan's own peak extraction"""
    rep = _report((arch, flip), lambda: P.run_plan_case(arch, flip))
    tag = "%s %s" % (arch, "flip_dets_only" if flip else "dets_only")
    print("\n%s  (physical C, hc, featLd) = %s" % (P.report_line(tag, rep), rep["geometry"]))
    assert rep["kernel"] == P.geometry(rep["row"], flip)["kernel"]
    assert rep["pad_weights_zero"], "the padding channels of feat did not take zero weights"
    assert rep["finite_feat"]
    assert not rep["failures"], "\n".join(rep["failures"])
    assert P.worst_of(rep).ratio <= rep["c"] == lo.LAYER_TOL["direct"]
    assert P.hps_liveness(rep["row"], rep["inds"], rep["ref"]) > P.HPS_LIVE[1]


def test_plans_cover_every_head_geometry():
    from centerpose_amd import nets
    reps = [_report((a, f), lambda a=a, f=f: P.run_plan_case(a, f)) for a, f in P.PLAN_CASES]
    geo = {rep["geometry"] for rep in reps}
    assert len(geo) == len(P.PLAN_ARCHS), geo
    assert {(rep["row"].C, rep["row"].hc) for rep in reps} == {nets.ARCH_HEAD[a] for a in lo.ARCHS}
    assert any(rep["geometry"][0] > rep["row"].C for rep in reps)           # a head whose input carries physical padding channels


# ---- the refusal ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", P.BOTH)
@pytest.mark.parametrize("hc", P.REFUSED_HC)
def test_launcher_refuses_an_over_wide_block_on_real_buffers(entry, hc):
    """rc 1, the message, and every buffer as it was: the check sits before any HIP call"""
    from centerpose_amd import _lib
    L = _lib.lib()
    C, J = 16, 1
    bufs = [torch.full((n,), 3.0, device="cuda") for n in (C, 2, 4 * 9 * C * hc, 4 * hc, (6 + 2 * J) * hc, 6 + 2 * J, 6 + 2 * J)]
    feat, inds, w1, b1, w2, b2, out = bufs
    inds.zero_()
    perm = torch.zeros(J, dtype=torch.int32, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    if entry == "pairs":
        feat = torch.full((2 * C,), 3.0, device="cuda")
        rc = L.cp_head_points_pairs_f32(vp(feat), C, vp(inds), vp(perm), vp(w1), vp(b1), vp(w2), vp(b2), vp(out), 1, 1, 1, C, J, 1, hc, _lib.stream())
    else:
        rc = L.cp_head_points_f32(vp(feat), C, vp(inds), vp(w1), vp(b1), vp(w2), vp(b2), vp(out), 1, 1, 1, C, J, 1, hc, _lib.stream())
    msg = L.cp_last_error().decode()
    torch.cuda.synchronize()
    assert rc == 1, (rc, msg)
    assert ("head_conv=%d needs a block of %d threads" % (hc, 2 * hc)) in msg and msg.startswith("head_points")
    assert bool((out == 3.0).all()) and bool((feat == 3.0).all()) and bool((w1 == 3.0).all())


def test_served_widths_were_launched():
    """hc = 256, 320, 448 and 512 are not refused: each is a row of the table that ran"""
    for entry in P.BOTH:
        ran = {P.make_case(cid).row.hc for cid in P.CASES if cid.endswith(entry) and _case_report(cid)["kernel"]}
        assert set(P.SERVED_HC) <= ran, (entry, sorted(ran))
