"""GPU: the HIP decode (csrc/decode.hip) where its comparisons decide -- exact ties and limits of the keypoint assignment, more than
one centre class, zeros and negative values inside the top-K.  Everything is compared bit for bit.

Reference of each test: the recorded outputs of the reference's multi_pose_decode (tests/golden/decode_edges.npz) wherever the
reference's order is specified; the numpy oracle's documented rule (value descending then flat index ascending, first minimum)
where torch leaves the order open.  tests/test_decode_edges_cpu.py shows that the recorded cases discriminate: a kernel with the
wrong strictness in any comparison that can see equal operands disagrees with the golden on the middle member of a triplet."""
import os

import numpy as np
import pytest
import torch

import cases
from oracle import decode_np

pytestmark = pytest.mark.gpu

EDGES = cases.decode_assign_edges()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "decode_edges.npz"))


def _hip(inp, K, use_reg=True, use_off=True):
    import centerpose_amd as cp
    t = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
    dets, inds, hm_inds, scores = cp.decode.multi_pose_decode(
        t["hm"], t["wh"], t["hps"], t["reg"] if use_reg else None, t["hm_hp"],
        t["hp_offset"] if use_off else None, K=K, return_indices=True)
    torch.cuda.synchronize()
    return dets.cpu().numpy(), inds.cpu().numpy(), hm_inds.cpu().numpy(), scores.cpu().numpy()


def _oracle(inp, K):
    return decode_np.multi_pose_decode(inp["hm"], inp["wh"], inp["hps"], inp["reg"], inp["hm_hp"], inp["hp_offset"], K=K,
                                       return_aux=True)


def _assert_equals_oracle(inp, K):
    """dets, both index sets, and the peak scores of every plane.  `==` on floats: +0.0 and -0.0 compare equal (see the signed test)."""
    ref, aux = _oracle(inp, K)
    HW = inp["hm"].shape[2] * inp["hm"].shape[3]
    dets, inds, hm_inds, scores = _hip(inp, K)
    assert np.array_equal(inds % HW, aux["inds"]) and np.array_equal(inds // HW, aux["clses"])
    assert np.array_equal(hm_inds, aux["hm_inds"])
    assert np.array_equal(scores[:, 0], aux["scores"]) and np.array_equal(scores[:, 1:], aux["hm_score_topk"])
    assert np.array_equal(dets, ref)
    return aux


# ---------------------------------------------------------------- 1. the keypoint assignment's comparisons
@pytest.mark.parametrize("name", sorted(EDGES))
def test_hip_assign_decisions_match_reference(name, gold):
    """Every decision case against the reference's recorded output; the three equal-distance cases (flag false) against the oracle,
    whose first-minimum rule the kernel documents."""
    c = EDGES[name]
    dets, inds, hm_inds, _ = _hip(c["inp"], c["K"], c["use_reg"], c["use_off"])
    if bool(gold[name + "__specified"]):
        want, want_inds, want_hm = gold[name + "__dets"], gold[name + "__inds"], gold[name + "__hm_inds"]
    else:
        i = c["inp"]
        want, aux = decode_np.multi_pose_decode(i["hm"], i["wh"], i["hps"], i["reg"] if c["use_reg"] else None, i["hm_hp"],
                                                i["hp_offset"] if c["use_off"] else None, K=c["K"], return_aux=True)
        want_inds, want_hm = aux["inds"], aux["hm_inds"]
    assert np.array_equal(inds, want_inds) and np.array_equal(hm_inds, want_hm)
    assert np.array_equal(dets, want), (name, dets[0, 0], want[0, 0])


# ---------------------------------------------------------------- 2. more than one centre class
@pytest.mark.parametrize("name", sorted(cases.DECODE_MULTICAT_CASES))
def test_hip_decode_multiclass_matches_reference(name, gold):
    """cat > 1: the plane split of both NMS forms, a streamed chunk that ends inside a plane, the NMS window at the seam between two
    planes, and the class dropped by `% HW` in the assignment.  The kernel's centre index is flat over cat * H * W."""
    cat, H, W, K, J, seed, seam = cases.DECODE_MULTICAT_CASES[name]
    assert bool(gold[name + "__specified"])
    inp = cases.decode_multicat(cat, H, W, J, seed, seam)
    dets, inds, hm_inds, _ = _hip(inp, K)
    assert np.array_equal(inds % (H * W), gold[name + "__inds"])
    assert np.array_equal(inds // (H * W), gold[name + "__clses"])
    assert np.array_equal(hm_inds, gold[name + "__hm_inds"])
    assert np.array_equal(dets, gold[name + "__dets"])
    ref, aux = _oracle(inp, K)
    assert np.array_equal(dets, ref) and np.array_equal(inds // (H * W), aux["clses"])


# ---------------------------------------------------------------- 3. zeros inside the top-K, signed maps
@pytest.mark.parametrize("H,W", [(128, 129), (129, 256), (300, 437)])
@pytest.mark.parametrize("K", [100, 256])
def test_hip_decode_sparse_planes_zeros_in_topk(H, W, K):
    """20..60 positive peaks per plane, zeros elsewhere: the K-th key is the key of 0 and hundreds of equal keys are ranked by index
    across the wave ranges (16 512 keys: LDS path) and across chunks (2 and 5 chunks).  torch.topk leaves this order open: the
    oracle's rule is the reference."""
    inp = cases.decode_sparse(700 + H, H, W)
    aux = _assert_equals_oracle(inp, K)
    for s, i in ((aux["scores"], aux["inds"]), (aux["hm_score_topk"].reshape(-1, K), aux["hm_inds"].reshape(-1, K))):
        for row_s, row_i in zip(s, i):
            nz = int((row_s > 0).sum())
            assert 0 < nz <= 60 and (row_s[nz:] == 0).all() and (np.diff(row_i[nz:]) > 0).all()      # zeros in ascending flat index


@pytest.mark.parametrize("H,W", [(60, 70), (128, 129), (129, 256), (300, 437)])
def test_hip_decode_quantised_ties(H, W):
    """Maps rounded to 1/16: large groups of equal survivors on the register path with division index math (60 x 70), the LDS path
    and the streamed path."""
    _assert_equals_oracle(cases.decode_quantised(800 + H, H, W), 100)


@pytest.mark.parametrize("name", sorted(cases.DECODE_SIGNED_CASES))
def test_hip_decode_signed_maps_positive_peaks_match_reference(name, gold):
    """randn maps without a sigmoid (the drop-in multi_pose_decode takes any float): the negative branch of the key transform runs
    for most keys, K reaches only positive peaks, and the reference's order is specified."""
    seed, H, W, K = cases.DECODE_SIGNED_CASES[name]
    assert bool(gold[name + "__specified"])
    dets, inds, hm_inds, _ = _hip(cases.decode_signed(seed, H, W), K)
    assert np.array_equal(inds, gold[name + "__inds"]) and np.array_equal(hm_inds, gold[name + "__hm_inds"])
    assert np.array_equal(dets, gold[name + "__dets"])


def test_hip_decode_signed_map_whole_plane_selected():
    """16 x 16 randn maps with planted true zeros, K = 256: suppressed negative values (-0.0 in `heat * keep`), true zeros and
    negative peaks are all selected.  Zeros of either sign are one group ranked by index; negative peaks come after every zero,
    by value.  Compared with `==`: the SIGN of a selected zero is not pinned -- the kernel returns +0.0 where the reference's
    `heat * keep` gives -0.0 (the key transform maps both to one key, as torch.topk compares them equal)."""
    inp = cases.decode_signed(650, 16, 16, zeros=6)
    aux = _assert_equals_oracle(inp, 256)
    for row in np.concatenate([aux["scores"], aux["hm_score_topk"].reshape(-1, 256)]):
        npos, nzero, nneg = int((row > 0).sum()), int((row == 0).sum()), int((row < 0).sum())
        assert npos and nneg >= 2 and nzero > 6 and np.signbit(row[row == 0]).any() and not np.signbit(row[row == 0]).all()
        assert (row[:npos] > 0).all() and (row[npos:npos + nzero] == 0).all() and (np.diff(row[npos + nzero:]) <= 0).all()
