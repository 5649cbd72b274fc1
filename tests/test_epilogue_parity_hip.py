"""Every epilogue path of the conv and DCN kernels, one stand-alone launch each, against a float64 reference element by element
(tests/epilogue_oracle.py on top of tests/layer_oracle.py and tests/launch_oracle.py).

The kernels choose their output code from the caller's pointers and strides.  Each case of `epilogue_oracle.CASES` forces one
instantiation (or, for the dispatcher's fall-back edges, starts from an eligible `tile = 0` launch and flips one predicate) and asserts

* the launch dispatched to the kernel the table names (`Launch.kernel`) -- the only path evidence the device gives: which body of an
  epilogue a block takes is `epilogue_oracle.expected_path`, a restatement of the predicates, printed next to the result;
* every element inside `c_for(family, K) u A` (LAYER_TOL, calibrated on the CPU; `tile_A` for the Winograd families);
* every float of the NaN-filled flat buffer that the launch does not own is still NaN: the channels from Cout to ld, the floats in front
  of a channel slice, the other phases of a scatter launch, 64 guard floats on both sides;
* a second run gives the same bits;
* a launch the launcher must refuse raises a clean CenterposeHipError and leaves the buffer all NaN.

The F(2x4) kernels promise "same arithmetic, same bits" for their lean and generic instantiations, and that covers the whole generic
function: a <true> case and every <false> twin with the same activation, residual and data -- Cout = 43 / 27 (the vector items and the
scalar tail), outLd = 45, an output slice 1 / 2 floats in, a residual 1 float in (all channels on the scalar branch) -- and the aligned
members of a mixed group against the same members of an all-aligned group, must be bit-equal.  For the other families the agreement of
vector and scalar twins is printed (-s), not asserted.  -s also prints, per family and mode, the worst err / (u A).
"""
import collections

import pytest
import torch

import epilogue_oracle as E
import layer_oracle as lo

pytestmark = pytest.mark.gpu

KEYS = list(dict.fromkeys((c.base, c.mode) for c in E.CASES))
_reports = {}
_broken = []                                      # the first case that raised: nothing is built or launched after it


def _report(key, run):
    """the report of case / group `key`, run once per module; one that raised raises again for whoever asks.  A refusal the table
    expects is a report, not an exception (`_judge_run`): whatever does raise -- a refusal nobody expected, a HIP error -- may have left
    the device in any state, so every case that has not run yet fails without touching the GPU."""
    if key not in _reports:
        if _broken:
            pytest.fail("not launched: %s raised earlier in this module (%s)" % tuple(_broken[0]), pytrace=False)
        try:
            _reports[key] = run(key)
        except Exception as e:                    # noqa: BLE001 -- kept, so that the summary fails with it rather than run it again
            _reports[key] = e
            _broken.append((key, "%s: %s" % (type(e).__name__, str(e)[:200])))
    if isinstance(_reports[key], Exception):
        raise _reports[key]
    return _reports[key]


def _check(c, rep, kernel):
    fails = list(rep["failures"])
    if kernel is None:
        print("\n%-44s %-7s refused: %s" % (c.id, E.expected_path(c), rep.get("error")))
        return fails
    for w, cc in zip(rep["worst"], rep["c"]):
        print("\n%-44s %-7s %-46s worst err / (u A) %.3f (c = %.1f) at %s" % (c.id, E.expected_path(c), rep["kernel"], w.ratio, cc, w.loc))
    if rep["kernel"] != kernel:
        fails.append("%s: dispatched to %s, the table says %s" % (c.id, rep["kernel"], kernel))
    return fails


@pytest.mark.parametrize("bid,mode", KEYS, ids=["%s-%s" % k for k in KEYS])
def test_every_case_of_a_base_and_mode_matches_fp64(bid, mode):
    fails = []
    for c in E.CASES:
        if (c.base, c.mode) == (bid, mode):
            fails += _check(c, _report(c.id, E.run_case), c.kernel)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("gid", list(E.GROUPS))
def test_group_launch_blocks_follow_their_own_member(gid):
    kernel, members = E.GROUPS[gid]
    rep = _report(gid, E.run_group)
    print("\n%-24s %s  paths %s  worst err / (u A) %s" % (gid, rep["kernel"], rep["path"], ["%.3f" % w.ratio for w in rep["worst"]]))
    assert rep["kernel"] == kernel == E.group_kernel(members)
    assert not rep["failures"], "\n".join(rep["failures"])


def _twins():
    """{(base, act, res): {mode/sub: (case, logical output)}} of the NHWC cases that ran"""
    tw = collections.defaultdict(dict)
    for c in E.CASES:
        rep = _reports.get(c.id)
        if isinstance(rep, dict) and rep["kernel"] is not None and c.mode in E.NHWC_MODES and not c.nchw:
            tw[(c.base, c.act, c.res)]["%s/%s" % (c.mode, c.sub)] = (c, rep["out"][0])
    return tw


def test_wino24_lean_and_generic_instantiations_give_the_same_bits():
    for c in E.CASES:
        if c.base == "wino24" and c.mode in E.NHWC_MODES:
            _report(c.id, E.run_case)
    pairs, fails = collections.Counter(), []
    for (bid, act, res), d in _twins().items():
        if bid != "wino24" or "V/c44" not in d:
            continue
        cv, ov = d["V/c44"]
        if cv.kernel != E.W24 % "true":
            continue
        for name, (c, o) in d.items():              # same activation, residual and data; only Cout, a stride or a pointer differ
            if c.mode == "V":
                continue
            assert c.kernel == E.W24 % "false" and E.expected_path(c) == ("mixed" if c.mode == "S-cout" else "scalar")
            n = c.cout                              # S-cout: the vector items AND the scalar tail; the others: all 44 on the scalar branch
            if not torch.equal(o, ov[:, :n]):
                fails.append("%s and %s differ at %s" % (cv.id, c.id, lo.first_unequal(o, ov[:, :n])))
            pairs[c.mode] += 1
    assert not fails, "\n".join(fails)
    assert pairs == {"S-cout": 2, "S-ld": 2, "S-ptr": 2, "S-res": 1}, pairs
    mixed, fast = _report("wino24-group-mixed", E.run_group), _report("wino24-group-fast", E.run_group)
    for i in (0, 1):                                # the two aligned ReLU members: the same cases in both groups
        assert E.GROUPS["wino24-group-mixed"][1][i] == E.GROUPS["wino24-group-fast"][1][i]
        assert torch.equal(mixed["out"][i], fast["out"][i]), "member %d differs at %s" % (i, lo.first_unequal(mixed["out"][i], fast["out"][i]))


def test_report_worst_ratios_and_twin_agreement():
    """every case has run (one that has not runs here; one that raised fails this test too); prints the summary"""
    reps = {c.id: _report(c.id, E.run_case) for c in E.CASES}
    worst = {}
    for c in E.CASES:
        rep = reps[c.id]
        if rep["kernel"] is None:
            continue
        key = (E.BASE[c.base].family, c.mode)
        if rep["worst"][0].ratio > worst.get(key, (-1.0, ""))[0]:
            worst[key] = (rep["worst"][0].ratio, c.id)
    for (fam, mode), (ratio, cid) in sorted(worst.items()):
        print("\nworst err / (u A) %-7s %-8s %8.3f (LAYER_TOL %.1f)  %s" % (fam, mode, ratio, lo.LAYER_TOL[fam], cid))
    agree = collections.Counter()
    for (bid, act, res), d in sorted(_twins().items()):
        v = next((o for name, (c, o) in d.items() if c.mode == "V"), None)
        for name, (c, o) in d.items():
            if v is not None and c.mode in ("S-ld", "S-ptr", "S-res") and o.shape == v.shape:
                agree[(E.BASE[bid].family, bool(torch.equal(o, v)))] += 1
    for (fam, same), n in sorted(agree.items()):
        print("\nvector / scalar twins %-7s %s: %d" % (fam, "bit-equal" if same else "differ", n))
    assert len(reps) == len(E.CASES)
