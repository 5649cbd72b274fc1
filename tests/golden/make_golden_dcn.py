"""Golden vectors for the DCNv2 forward from the REFERENCE's own im2col text (build container only).

oracle/Makefile compiles dmcn_im2col_bilinear and modulated_deformable_im2col_gpu_kernel, cut out of the reference's
DCNv2/src/cuda/dcn_v2_im2col_cuda.cu, into oracle/_ref/libcp_refdcn.so; oracle.dcn.dcn_v2_forward_ref runs it and applies
weight . col + bias in float64.  This script stores the float32-rounded outputs, one file per case (tests/golden/dcn_ref_<name>.npz,
key `out`); the inputs are regenerated from seeds by tests/cases.py.  It also records the rounding yardstick A of the pin
(tests/test_dcn_reference_pin.py) in dcn_ref_yardstick.json.  Deterministic: two runs write identical bytes (fixed zip time stamps).

    python tests/golden/make_golden_dcn.py
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import cases  # noqa: E402
from oracle import dcn  # noqa: E402

A_NO_FMA = 2.0 ** -21       # four float32 roundings of half an ulp each (four-term blend, mask product), relative to the sampled value


def call_args(c):
    return (c["x"], c["w"], c["b"], c["off"], c["m"]) + c["args"]


def fixture_array(name, fx=None):
    """float32 output of the reference forward for one named case."""
    c = (fx or cases.dcn_fixtures())[name]()
    return dcn.dcn_v2_forward_ref(*call_args(c)).astype(np.float32)


def npz_bytes(**arrays):
    """An .npz (deflate) with fixed member time stamps -- numpy's own savez stamps the members with the wall clock."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), version=(1, 0), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, b.getvalue(), compresslevel=9)
    return buf.getvalue()


def fixture_path(name):
    return os.path.join(HERE, "dcn_ref_%s.npz" % name)


def yardstick(groups=None):
    """A = max over every case of the pin of max|ref(contract off) - ref(contract fast, FMA)| / max|ref(contract off)|: the
    reference's own rounding ambiguity (nvcc contracts by default, gcc does not).  -> (A, has_fma, number of cases)"""
    groups = groups or cases.dcn_pin_groups()
    n = sum(len(v) for v in groups.values())
    if not dcn.ref_available(contract=True):
        return A_NO_FMA, False, n
    a = 0.0
    for cs in groups.values():
        for c in cs:
            off = dcn.dcn_v2_forward_ref(*call_args(c))
            fast = dcn.dcn_v2_forward_ref(*call_args(c), contract=True)
            a = max(a, float(np.abs(off - fast).max() / np.abs(off).max()))
    return a, True, n


def main():
    assert dcn.ref_available(), "oracle/_ref/libcp_refdcn.so is not built: needs the reference tree (make -C oracle)"
    fx = cases.dcn_fixtures()
    total = 0
    for name in fx:
        data = npz_bytes(out=fixture_array(name, fx))
        with open(fixture_path(name), "wb") as f:
            f.write(data)
        total += len(data)
        print("dcn_ref_%s.npz %d bytes" % (name, len(data)))
    a, fma, n = yardstick()
    with open(os.path.join(HERE, "dcn_ref_yardstick.json"), "w") as f:
        json.dump({"A": a, "fma_twin": fma, "cases": n, "bound": "4 * A * max|ref| per case"}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d files, %d bytes; A = %.4e over %d cases (fma twin: %s)" % (len(fx), total, a, n, fma))


if __name__ == "__main__":
    main()
