"""GPU: the device soft-NMS (post_merge_nms_kernel, csrc/batch_stages.hip) at exact ties and limits, against vectors produced by the
reference's own source (tests/golden/soft_nms_39_edges.npz): equal scores in the arg-max (within a lane's stride and across lanes),
IoU exactly on Nt, a decayed score exactly on the threshold, discards of the last row, chains of discards, N shrinking to i + 1.
All 56 columns and n_keep bit-equal, column 4 included: no case takes the exp path with a decay.  tests/test_nms_edges_cpu.py counts
how often each decision occurs in the set."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_nms as mg  # noqa: E402

CASES = mg.edge_cases()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "soft_nms_39_edges.npz"))


def _device_nms(boxes_list, **kw):
    from centerpose_amd import detector
    d = torch.from_numpy(np.stack(boxes_list)).cuda()
    out, keep = detector.post_merge_batch([d], nms=True, **kw)
    return out.cpu().numpy(), keep.cpu().numpy()


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_soft_nms_edge_case_matches_reference_source_golden(name, gold):
    boxes, kw = CASES[name]
    out, keep = _device_nms([boxes], **kw)
    assert int(keep[0]) == len(gold[name + "__keep"]), name
    assert np.array_equal(out[0], gold[name + "__out"]), name


def test_device_soft_nms_three_different_images_one_launch(gold):
    """23, 64 and 2 rows kept of 64: a per-image N that leaked into a neighbour would show."""
    names = ["batch64_clustered", "batch64_disjoint", "batch64_one_cluster"]
    kw = CASES[names[0]][1]
    assert all(CASES[n][1] == kw and CASES[n][0].shape == (64, 56) for n in names)
    for order in (names, names[::-1]):
        out, keep = _device_nms([CASES[n][0] for n in order], **kw)
        assert keep.tolist() == [len(gold[n + "__keep"]) for n in order]
        assert len(set(keep.tolist())) == 3
        for i, n in enumerate(order):
            assert np.array_equal(out[i], gold[n + "__out"]), n
