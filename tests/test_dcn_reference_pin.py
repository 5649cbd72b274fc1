"""CPU: the DCNv2 restatements (oracle/dcn_ref.c, oracle/dcn.py::dcn_v2_forward_torch) pinned to the REFERENCE's own im2col text.

oracle/Makefile cuts dmcn_im2col_bilinear and modulated_deformable_im2col_gpu_kernel out of the reference's
DCNv2/src/cuda/dcn_v2_im2col_cuda.cu and compiles them for the CPU (oracle/_ref/libcp_refdcn.so; stand-ins: thread index, GEMM).
Where that library exists (the build container) the live tests below run, all of them; elsewhere they skip and the committed
outputs tests/golden/dcn_ref_*.npz (made by tests/golden/make_golden_dcn.py from the same library) carry the pin.

Inputs (tests/cases.py::dcn_pin_groups, 323 cases): every DCN input of the GPU suite (kernel 28, split_k 8, kernel_dg 4,
forward_dg 6, full_args 5, gpu_fuzz 24), the boundary lattice (8 configurations) and a seeded fuzz (240).

Tolerance.  Not chosen: the yardstick is the reference's own rounding ambiguity.  nvcc contracts a*b+c into FMAs by default, gcc
does not, so the same extract is built twice (-ffp-contract=off and -ffp-contract=fast -mfma) and
    A = max over all cases of max|ref_off - ref_fma| / max|ref_off|
(A = 2^-21 on a CPU without FMA: four float32 roundings of half an ulp each in the four-term blend and the mask product).  A
restatement must agree with the contract-off build within 4 * A * max|ref_off| per case; the factor 4 is room for another
summation order inside the GEMM and for the float32 rounding of the stored result.  The sampled columns must be bit-equal.

Measured in the build container (CPU with FMA; also in profiles/dcn_reference_pin.txt): A = 1.4148e-07, bound 4A = 5.6591e-07.
Worst |restatement - ref_off| / max|ref_off| per group:
    group        cases   A(group)    dcn_ref.c    dcn_v2_forward_torch (dg == 1)   columns
    kernel          28   3.092e-08   5.196e-08    3.184e-07                        bit-equal
    split_k          8   2.659e-08   3.892e-08    1.960e-07                        bit-equal
    kernel_dg        4   2.465e-08   4.131e-08    -                                -
    forward_dg       6   6.528e-08   3.777e-08    5.014e-07                        bit-equal
    full_args        5   4.236e-08   4.471e-08    3.690e-07                        bit-equal
    gpu_fuzz        24   4.561e-08   5.192e-08    1.556e-07                        bit-equal
    lattice          8   5.641e-08   5.156e-08    1.579e-07                        bit-equal
    pin_fuzz       240   1.415e-07   5.671e-08    9.651e-08                        bit-equal
dcn_ref.c sits at the float32 rounding of its stored output (2^-24 = 5.96e-08); the torch restatement's excess is its float32
GEMM.  dcn_ref.c's columns (read out through a one-hot weight) are bit-equal in every lattice, fuzz, forward_dg and full_args case.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import cases
from oracle import dcn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_dcn as mg  # noqa: E402

needs_ref = pytest.mark.skipif(not dcn.ref_available(),
                               reason="oracle/_ref/libcp_refdcn.so is not built: the reference tree was not readable at build time")
GROUPS = ("kernel", "split_k", "kernel_dg", "forward_dg", "full_args", "gpu_fuzz", "lattice", "pin_fuzz")
GROUP_SIZES = dict(kernel=28, split_k=8, kernel_dg=4, forward_dg=6, full_args=5, gpu_fuzz=24, lattice=8, pin_fuzz=240)
_CACHE = {}


def _groups():
    if "groups" not in _CACHE:
        _CACHE["groups"] = cases.dcn_pin_groups()
    return _CACHE["groups"]


def _yardstick():
    if "A" not in _CACHE:
        _CACHE["A"] = mg.yardstick(_groups())
    return _CACHE["A"]


def _recorded_yardstick(golden_dir):
    with open(os.path.join(golden_dir, "dcn_ref_yardstick.json")) as f:
        return json.load(f)


def _rel(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


def test_case_lists_are_those_of_the_gpu_suite():
    """The rows in tests/cases.py are the parameter rows of the GPU tests they claim to mirror."""
    import test_conv_hip as t

    def rows(fn, n):
        mark = [m for m in fn.pytestmark if m.name == "parametrize" and len(m.args[0].split(",")) == n]
        assert len(mark) == 1
        return [tuple(r) for r in mark[0].args[1]]
    assert rows(t.test_dcn_v2_vs_scalar_oracle, 6) == cases.DCN_KERNEL_SHAPES
    assert rows(t.test_dcn_v2_kernel_deformable_groups_vs_scalar_oracle, 5) == cases.DCN_KERNEL_DG_SHAPES
    assert rows(t.test_dcn_v2_forward_deformable_groups, 7) == cases.DCN_FORWARD_DG_ROWS
    assert rows(t.test_dcn_v2_forward_full_argument_space, 11) == cases.DCN_FULL_ARG_ROWS
    assert t._dcn_case is cases._dcn_case and t._dcn_mask_logits is cases._dcn_mask_logits
    g = _groups()
    assert {k: len(v) for k, v in g.items()} == GROUP_SIZES
    tiles = {r[5] for r in cases.DCN_KERNEL_SHAPES}
    assert tiles == {0, 64064, 64128, 128064, 128032, 64032} == {r[5] for r in cases.DCN_FIXTURE_LOGITS_SHAPES}


def test_pin_fuzz_spans_the_argument_space():
    cs = _groups()["pin_fuzz"]
    assert len(cs) >= 200
    a = np.array([c["args"] for c in cs])
    assert set(a[:, 0]) == set(a[:, 1]) == {1, 2, 3, 4, 5}                   # kh, kw
    assert set(a[:, 2]) == set(a[:, 3]) == {1, 2, 3}                         # stride
    assert set(a[:, 4]) == set(a[:, 5]) == {0, 1, 2, 3}                      # pad
    assert set(a[:, 6]) == set(a[:, 7]) == {1, 2, 3}                         # dilation
    assert set(a[:, 8]) == {1, 2, 3, 4}                                      # deformable groups
    assert {c["x"].shape[0] for c in cs} == {1, 2, 3}
    assert all(c["x"].shape[2] % 2 == 1 and c["x"].shape[3] % 2 == 1 for c in cs)
    # finite, and |coordinate| <= 1e6 (the lattice's offsets exceed 1e6 by the tap's integer part to land on it): floor -> int is defined
    assert all(np.isfinite(c["off"]).all() and np.abs(c["off"]).max() <= 1e6 + 32 for g in _groups().values() for c in g)


@pytest.mark.parametrize("cfg", cases.DCN_LATTICE_CONFIGS, ids=[c[0] for c in cases.DCN_LATTICE_CONFIGS])
def test_lattice_covers_every_coordinate(cfg):
    """Per tap (and per deformable group), for h and for w: the float32 coordinate the reference's expression evaluates to lands on
    -1, just above -1, -0.5, just below 0, 0, an interior integer, N-1, N-0.5, just below N, N, N+0.5, +-3N and +-1e6.  "just above /
    below" is the nearest float the rounded sum `int + offset` can reach for that tap: within 2^-20 of the target (one ulp of an
    offset below 16 in magnitude); the exact neighbours nextafter(-1, 0) and nextafter(N, 0) are reached by the taps whose integer
    part is 0 or -1.  The offsets hold a -0.0 where tap and target coincide at 0."""
    c = cases.dcn_lattice_case(*cfg)
    H, W = cases.DCN_LATTICE_HW
    f = np.float32
    assert c["h_im"].shape == c["m"].shape
    for axis, N in (("h_im", H), ("w_im", W)):
        v = c[axis]
        for ch in range(v.shape[1]):                                         # dg * 9 taps
            t = v[:, ch].reshape(-1)
            for point in (-1.0, -0.5, 0.0, 2.0, 2.25, N - 1.0, N - 0.5, float(N), N + 0.5, 3.0 * N, -3.0 * N, 1e6, -1e6):
                assert (t == f(point)).any(), (axis, ch, point)
            assert ((t > -1) & (t <= f(-1 + 2.0 ** -20))).any(), (axis, ch, "just above -1")
            assert ((t < 0) & (t >= f(-2.0 ** -20))).any(), (axis, ch, "just below 0")
            assert ((t < N) & (t >= f(N - 2.0 ** -20))).any(), (axis, ch, "just below N")
        assert (v == np.nextafter(f(-1), f(0))).any() and (v == np.nextafter(f(N), f(0))).any(), axis
    assert np.signbit(c["off"][c["off"] == 0]).any()
    assert np.abs(c["off"]).max() <= 1e6 + 16
    ws = c["w"].reshape(c["w"].shape[0], -1)
    assert all(len(np.unique(row)) == row.size for row in ws)               # a distinct weight per (c, i, j)


@needs_ref
def test_reference_rounding_yardstick(golden_dir):
    a, fma, n = _yardstick()
    rec = _recorded_yardstick(golden_dir)
    print("\nA = %.4e (fma twin %s) over %d cases; bound 4A = %.4e; recorded with the fixtures: A = %.4e" % (a, fma, n, 4 * a, rec["A"]))
    assert n == sum(GROUP_SIZES.values()) == rec["cases"]
    assert np.isfinite(a) and a > 0
    if fma and rec["fma_twin"]:
        assert 0.5 <= a / rec["A"] <= 2.0       # the same measurement as the one recorded next to the fixtures
    else:
        assert a == 2.0 ** -21 or rec["A"] == 2.0 ** -21


@needs_ref
@pytest.mark.parametrize("group", GROUPS)
def test_c_restatement_matches_reference(group):
    a = _yardstick()[0]
    worst = 0.0
    for i, c in enumerate(_groups()[group]):
        args = mg.call_args(c)
        ref = dcn.dcn_v2_forward_ref(*args)
        out = dcn.dcn_v2_forward_c(*args)
        assert out.shape == ref.shape
        e = _rel(out, ref)
        worst = max(worst, e)
        assert e <= 4 * a, (group, i, c["args"], e, 4 * a)
    print("\n%s: %d cases, dcn_ref.c worst %.3e of max|ref| (bound 4A = %.3e)" % (group, len(_groups()[group]), worst, 4 * a))


@needs_ref
@pytest.mark.parametrize("group", [g for g in GROUPS if g != "kernel_dg"])
def test_torch_restatement_matches_reference_outputs_and_columns(group):
    """dg == 1 cases (dcn_v2_forward_torch implements nothing else): output within 4A, sampled columns bit-equal to the reference's."""
    a = _yardstick()[0]
    worst, n = 0.0, 0
    for i, c in enumerate(_groups()[group]):
        if c["args"][8] != 1:
            continue
        ref, col = dcn.dcn_v2_forward_ref(*mg.call_args(c), return_col=True)
        out, tcol = dcn.dcn_v2_forward_torch(*(torch.from_numpy(c[k]) for k in ("x", "w", "b", "off", "m")), *c["args"], return_col=True)
        bad = np.flatnonzero(tcol.numpy().view(np.uint32).reshape(-1) != col.view(np.uint32).reshape(-1))
        assert bad.size == 0, (group, i, c["args"], "columns differ at", bad[:8])
        e = _rel(out.numpy(), ref)
        worst, n = max(worst, e), n + 1
        assert e <= 4 * a, (group, i, c["args"], e, 4 * a)
    assert n > 0
    print("\n%s: %d dg==1 cases, torch worst %.3e of max|ref| (bound 4A = %.3e), columns bit-equal" % (group, n, worst, 4 * a))


@needs_ref
@pytest.mark.parametrize("group", ["forward_dg", "full_args", "lattice", "pin_fuzz"])
def test_c_restatement_columns_bit_equal(group):
    """dcn_ref.c exposes no column buffer; a one-hot weight (Co = C*kh*kw, output o = column o, bias 0) reads it out exactly: the
    double accumulator holds one float32 product with 1.0 and zeros.  Every column equals the reference's bit for bit, so no channel,
    tap, group or offset-pair mix-up can hide behind the weights."""
    n = 0
    for i, c in enumerate(_groups()[group]):
        kh, kw = c["args"][:2]
        C = c["x"].shape[1]
        K = C * kh * kw
        eye = np.eye(K, dtype=np.float32).reshape(K, C, kh, kw)
        col = dcn.dcn_im2col_ref(c["x"], c["off"], c["m"], *c["args"])
        out = dcn.dcn_v2_forward_c(c["x"], eye, np.zeros(K, np.float32), c["off"], c["m"], *c["args"])
        got = out.reshape(col.shape)
        assert np.array_equal(got, col), (group, i, c["args"], np.argwhere(got != col)[:4])
        n += got.size
    print("\n%s: %d column values bit-equal" % (group, n))


# --- committed fixtures ------------------------------------------------------------------------------------------------------

FIXTURES = cases.dcn_fixtures()


def test_fixture_set_is_complete(golden_dir):
    names = sorted(f[len("dcn_ref_"):-len(".npz")] for f in os.listdir(golden_dir) if f.startswith("dcn_ref_") and f.endswith(".npz"))
    assert names == sorted(FIXTURES)
    assert sum(n.endswith("_mask") for n in names) == 14 and sum(n.endswith("_logits") for n in names) == 6
    for n in names:
        assert os.path.getsize(mg.fixture_path(n)) <= 225 * 1024


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_c_restatement_matches_reference_fixture(name, golden_dir):
    """Runs everywhere: oracle/dcn_ref.c against the committed output of the reference library, within the bound above (4A with the
    A recorded when the fixtures were made; the float32 rounding of the stored fixture is part of the factor 4)."""
    a = _recorded_yardstick(golden_dir)["A"]
    with np.load(mg.fixture_path(name)) as z:
        assert z.files == ["out"] and z["out"].dtype == np.float32
        ref = z["out"].astype(np.float64)
    c = FIXTURES[name]()
    out = dcn.dcn_v2_forward_c(*mg.call_args(c))
    assert out.shape == ref.shape
    e = _rel(out, ref)
    assert e <= 4 * a, (name, e, 4 * a)


@needs_ref
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixture_regenerates_bit_for_bit(name):
    """Where the files came from: the live reference library writes the same bytes."""
    with open(mg.fixture_path(name), "rb") as f:
        have = f.read()
    assert mg.npz_bytes(out=mg.fixture_array(name, FIXTURES)) == have
