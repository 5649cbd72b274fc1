"""CPU: the decode decisions at their limits -- the numpy oracle against the reference's recorded outputs
(tests/golden/decode_edges.npz, written by tests/golden/make_golden.py decode_edges), and the conditions that make the recorded
cases a test of strictness: every triplet (operand one float32 below / on / one above the limit) changes its decision exactly once,
and every comparison of the keypoint assignment that can see equal operands sees them.

Judged by the reference: every case whose `__specified` flag is true (all triplets, the plane without a candidate, the multi-class
and the signed cases).  Judged by the oracle's order rule (value descending then index ascending, first minimum): the three
equal-distance cases, where the flag is false; that this torch build agreed with the rule there is recorded (`__agrees`), not asserted."""
import os

import numpy as np
import pytest

import cases
from oracle import decode_np

EDGES = cases.decode_assign_edges()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "decode_edges.npz"))


_ORACLE = {}


def _oracle(name):
    if name not in _ORACLE:
        c = EDGES[name]
        i = c["inp"]
        _ORACLE[name] = decode_np.multi_pose_decode(i["hm"], i["wh"], i["hps"], i["reg"] if c["use_reg"] else None, i["hm_hp"],
                                                    i["hp_offset"] if c["use_off"] else None, K=c["K"], return_aux=True)
    return _ORACLE[name]


def _operands(cmp, which):
    """The two operands of a comparison over everything the decode evaluates, as flat arrays."""
    a, b = {"sx<l": ("sel_x", "l"), "sx>r": ("sel_x", "r"), "sy<t": ("sel_y", "t"), "sy>b": ("sel_y", "b"),
            "ss<0.1": ("sel_score", None), "best>lim": ("min_dist", "limit"), "s>0.1": ("cand_score", None)}[which]
    x = cmp[a].ravel()
    return x, (cmp[b].ravel() if b else np.full(x.shape, np.float32(0.1), np.float32))


def _main_operands(name):
    """Operands of the case's comparison at the decision under test: image 0, centre rank 0, joint j (for the candidate-side
    comparison: the planted candidate, the only one of the plane within one float32 of 0.1)."""
    c = EDGES[name]
    cmp = _oracle(name)[1]["cmp"]
    if c["cmp"] == "s>0.1":
        s = cmp["cand_score"][0, c["j"]]
        m = int(np.argmin(np.abs(s.astype(np.float64) - 0.1)))
        return s[m], np.float32(0.1)
    a, b = {"sx<l": ("sel_x", "l"), "sx>r": ("sel_x", "r"), "sy<t": ("sel_y", "t"), "sy>b": ("sel_y", "b"),
            "best>lim": ("min_dist", "limit")}[c["cmp"]]
    return cmp[a][0, c["j"], 0], cmp[b][0, c["j"], 0]


def _decision(name, dets):
    """What the OUTPUT says the decision was.  Candidate-side comparison: is the emitted keypoint score the planted candidate's
    (accepted as a candidate) or something else (-1, or the other candidate's).  All others: was the candidate rejected, i.e. does
    the row carry the regressed keypoint -- which every scene keeps apart from the candidate's position."""
    c = EDGES[name]
    j, J = c["j"], c["inp"]["hps"].shape[1] // 2
    cmp = _oracle(name)[1]["cmp"]
    row = dets[0, 0]
    if c["cmp"] == "s>0.1":
        s = cmp["cand_score"][0, j]
        planted = s[int(np.argmin(np.abs(s.astype(np.float64) - 0.1)))]
        return bool(row[5 + 2 * J + j] == planted)
    kx, ky = cmp["kp_x"][0, j, 0], cmp["kp_y"][0, j, 0]
    sx, sy = cmp["sel_x"][0, j, 0], cmp["sel_y"][0, j, 0]
    assert (kx, ky) != (sx, sy), name
    got = (row[5 + 2 * j], row[5 + 2 * j + 1])
    assert got in ((kx, ky), (sx, sy)), name
    return got == (kx, ky)


@pytest.mark.parametrize("name", sorted(EDGES))
def test_oracle_equals_reference_on_edge_cases(name, gold):
    dets, aux = _oracle(name)
    same = (np.array_equal(dets, gold[name + "__dets"]) and np.array_equal(aux["inds"], gold[name + "__inds"]) and
            np.array_equal(aux["hm_inds"], gold[name + "__hm_inds"]))
    assert bool(gold[name + "__agrees"]) == same
    if bool(gold[name + "__specified"]):
        assert same and dets.dtype == np.float32
    assert bool(gold[name + "__specified"]) == (EDGES[name]["group"] is not None or name == "no_candidate")


def test_every_triplet_flips_exactly_once(gold):
    groups = {}
    for name, c in EDGES.items():
        if c["group"]:
            groups.setdefault(c["group"], {})[c["side"]] = name
    assert len(groups) == 11
    for g, members in sorted(groups.items()):
        assert sorted(members) == [-1, 0, 1], g
        cmpname = EDGES[members[0]]["cmp"]
        assert all(EDGES[n]["cmp"] == cmpname for n in members.values())
        # the operands: equal on the middle member, adjacent float32 values in the expected order on the outer ones
        a0, b0 = _main_operands(members[0])
        assert a0 == b0, g
        am, bm = _main_operands(members[-1])
        ap, bp = _main_operands(members[1])
        assert am < bm and np.nextafter(am, np.float32(np.inf)) == bm, (g, am, bm)
        assert ap > bp and np.nextafter(bp, np.float32(np.inf)) == ap, (g, ap, bp)
        # the reference's outputs: the decision changes between "at" and exactly one neighbour
        d = {side: _decision(n, gold[n + "__dets"]) for side, n in members.items()}
        assert (d[-1] != d[0]) != (d[0] != d[1]), (g, d)
        # ... and on the side the comparison's strictness says: `<` and `>` are both false on equal operands
        want = {"sx<l": (True, False, False), "sy<t": (True, False, False), "sx>r": (False, False, True),
                "sy>b": (False, False, True), "best>lim": (False, False, True), "s>0.1": (False, False, True)}[cmpname]
        assert (d[-1], d[0], d[1]) == want, (g, d)


def test_every_comparison_sees_equal_operands():
    """Counted over everything the oracle evaluates on the whole set (all images, centres, joints, candidates)."""
    hits = dict.fromkeys(cases.ASSIGN_COMPARISONS, 0)
    ss_values = []
    for name in EDGES:
        cmp = _oracle(name)[1]["cmp"]
        for which in hits:
            a, b = _operands(cmp, which)
            hits[which] += int((a == b).sum())
        ss_values.append(cmp["sel_score"].ravel())
    print("equal-operand evaluations:", hits)
    for which in cases.ASSIGN_COMPARISONS:
        if which != "ss<0.1":
            assert hits[which] >= 1, which
    # `ss < 0.1f` (decode.py:301) cannot see equal operands: ss went through the `> 0.1` mask (:282-283), so it is -1 or above 0.1 --
    # its strictness is unobservable; the set still drives it with -1 and with the float32 next to 0.1
    ss = np.concatenate(ss_values)
    assert hits["ss<0.1"] == 0 and ((ss == -1) | (ss > np.float32(0.1))).all()
    assert (ss == -1).any() and (ss == np.nextafter(np.float32(0.1), np.float32(1))).any()


def test_equal_distance_cases_follow_the_first_minimum(gold):
    """Judged by the oracle's rule: the candidate that comes first in the joint's top-K (the higher score) wins an exact distance tie."""
    for name, want_x, n_tied in (("tie_left_first", 6.0, 2), ("tie_right_first", 10.0, 2), ("tie_three", 10.0, 3)):
        dets, aux = _oracle(name)
        cmp = aux["cmp"]
        assert int((cmp["dist"][0, 0, 0] == cmp["min_dist"][0, 0, 0]).sum()) == n_tied and cmp["min_ind"][0, 0, 0] == 0
        assert dets[0, 0, 5] == want_x and dets[0, 0, 6] == 8.0 and dets[0, 0, 7] == 0.75 and not cmp["rej"][0, 0, 0]
        assert not bool(gold[name + "__specified"])
    dets, aux = _oracle("no_candidate")
    cmp = aux["cmp"]
    assert (cmp["cand_x"][0, 1] == -10000).all() and (cmp["dist"][0, 1, 0] == cmp["min_dist"][0, 1, 0]).all()
    assert cmp["min_ind"][0, 1, 0] == 0 and dets[0, 0, 5 + 2 * 2 + 1] == -1 and cmp["rej"][0, 1, 0]


# ---------------------------------------------------------------- more than one centre class, signed maps
@pytest.mark.parametrize("name", sorted(cases.DECODE_MULTICAT_CASES))
def test_oracle_equals_reference_multiclass(name, gold):
    cat, H, W, K, J, seed, seam = cases.DECODE_MULTICAT_CASES[name]
    assert bool(gold[name + "__specified"])
    inp = cases.decode_multicat(cat, H, W, J, seed, seam)
    dets, aux = decode_np.multi_pose_decode(inp["hm"], inp["wh"], inp["hps"], inp["reg"], inp["hm_hp"], inp["hp_offset"], K=K,
                                            return_aux=True)
    assert np.array_equal(aux["inds"], gold[name + "__inds"]) and np.array_equal(aux["clses"], gold[name + "__clses"])
    assert np.array_equal(aux["hm_inds"], gold[name + "__hm_inds"]) and np.array_equal(dets, gold[name + "__dets"])
    assert len(np.unique(gold[name + "__clses"])) == cat
    if seam:                                            # the reference kept every peak planted beside a plane boundary
        got = set(zip(gold[name + "__clses"][0].tolist(), gold[name + "__inds"][0].tolist()))
        for (c, y, x, v) in cases.seam_peaks(cat, H, W):
            assert (c, y * W + x) in got, (name, c, y, x)


@pytest.mark.parametrize("name", sorted(cases.DECODE_SIGNED_CASES))
def test_oracle_equals_reference_signed_positive_peaks(name, gold):
    seed, H, W, K = cases.DECODE_SIGNED_CASES[name]
    assert bool(gold[name + "__specified"])
    inp = cases.decode_signed(seed, H, W)
    dets, aux = decode_np.multi_pose_decode(inp["hm"], inp["wh"], inp["hps"], inp["reg"], inp["hm_hp"], inp["hp_offset"], K=K,
                                            return_aux=True)
    assert (aux["scores"] > 0).all() and (aux["hm_score_topk"] > 0).all()           # K reaches no zero and no negative peak
    assert (inp["hm"] < 0).any() and (inp["hm_hp"] < 0).any()
    assert np.array_equal(aux["inds"], gold[name + "__inds"]) and np.array_equal(aux["hm_inds"], gold[name + "__hm_inds"])
    assert np.array_equal(dets, gold[name + "__dets"])
