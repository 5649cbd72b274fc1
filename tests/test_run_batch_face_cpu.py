"""CPU: run_batch(face=) refuses host arrays before anything runs (a detector without a model is enough to get there)."""
import numpy as np
import pytest


def test_run_batch_face_refuses_host_arrays_before_anything_runs():
    from centerpose_amd import config, detector
    det = object.__new__(detector.MultiPoseDetector)
    det.cfg = config.get_cfg("dla_34")
    det.scales = det.cfg.TEST.TEST_SCALES
    det.model = type("Model", (), {"process": None, "device": "cpu"})()
    fake = type("Aligner", (), {"capacity": 4})()
    with pytest.raises(ValueError, match="face= takes its crops from frames on the device"):
        det.run_batch([np.zeros((8, 8, 3), np.uint8)], face=fake)
