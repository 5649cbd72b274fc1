"""Every hot-path kernel family at the last shape its launcher's 32-bit offset checks accept (tests/limit_oracle.py), on the device.

One stand-alone launch per row of `limit_oracle.ROWS` at LIM -- channel slices of a 64-float-wide buffer, B = 3, 1365 x 4097: 2^24 - 1
pixels, the source 256 bytes short of 2^32, image 1 astride byte 2^31 and image 2 above it -- with the variant forced, asserting

* the launch dispatched to exactly the kernel the row names,
* the judged crops (both ends of every image, the tile rows around the 2^31 crossing, the last tile column, the final pixel) inside
  `layer_oracle`'s unchanged bound `c_for(family, K) u A` against float64,
* image 2 -- and image 1 -- of the LIM launch bit-equal to the same forced variant run on that image alone in fresh buffers: every pixel
  above 2^31 without any host arithmetic,
* NaN guards before, behind and between the pixels of the output intact, exact zeros in the padding channels, the same bits from a
  second run, and at most 12 GiB held at once.

Besides the rows: the F(2x4) lean epilogue at its own limit (13 output rows times W * outLd in `int`): the first shape past it must report
`conv3x3_wino24_kernel<false>`, the last one inside `<true>`; and every refused shape a buffer can back, called with real buffers.

tests/test_limit_oracle_cpu.py predicts from the restated index arithmetic that LIM is safe to launch; it runs before this file.
The NCHW stems have no row: their LIM input alone is 8 GiB.  Run with -s for the per-row report (profiles/limit_parity_report.txt).
"""
import pytest
import torch

import limit_oracle as M

pytestmark = pytest.mark.gpu

# one family per line of the issue's table of size checks; the stems are audited on the CPU only (see the module docstring)
MUST_COVER = (
    "igemm_conv_kernel<", "splitk_reduce_kernel", "pw_conv_kernel<", "conv3x3_patch_kernel<", "conv3x3_c16_kernel<1, 1", "conv3x3_c16_kernel<2, 2",
    "conv3x3_wino_kernel<", "conv3x3_wino_vs64_kernel<0, 0>", "conv3x3_wino24_kernel<", "conv3x3_wino_vs64_kernel<2, 0>", "head_wino24_kernel<1, 0>",
    "dcn_igemm_kernel<64, 32", "dcn_igemm_kernel<128, 32", "igemm_conv_group_kernel", "conv3x3_wino24_group_kernel<",
    "igemm_bf16x3_kernel<128, 64>", "igemm_bf16x3_kernel<64, 64>",        # the opt-in split-bf16 kernel: half and quarter staging
)
_reports = {}


def _report(rid):
    """the report of row `rid`, run once per module; a row that raised raises again for whoever asks"""
    if rid not in _reports:
        try:
            _reports[rid] = M.run_row(rid)
        except Exception as e:                    # noqa: BLE001 -- kept, so that the coverage test fails with it rather than run it again
            _reports[rid] = e
            if isinstance(e, RuntimeError) and "hip" in str(e).lower():
                pytest.exit("device error in row %s, nothing more is launched: %s" % (rid, e), returncode=1)
    if isinstance(_reports[rid], Exception):
        raise _reports[rid]
    return _reports[rid]


@pytest.mark.parametrize("rid", [r.id for r in M.ROWS])
def test_row_at_the_offset_limit(rid):
    row, rep = M.ROW[rid], _report(rid)
    print("\n" + M.format_row(rid, rep))
    assert rep["kernels"][0] == row.kernel
    assert rep["kernels"][1:] == ["splitk_reduce_kernel"] * (row.p["S"] > 1)
    assert sorted(rep["translation"]) == sorted(row.p["images"]) and all(rep["translation"].values())
    assert rep["worst"].ratio <= rep["c"]
    assert not rep["failures"], "\n".join(rep["failures"])


def test_every_family_ran_at_the_limit():
    """the union of the dispatched names holds every entry of MUST_COVER; a row that has not run yet runs here, one that raised fails this
    test too"""
    reps = {r.id: _report(r.id) for r in M.ROWS}
    covered = set().union(*(rep["kernels"] for rep in reps.values()))
    missing = [k for k in MUST_COVER if not any(name.startswith(k) for name in covered)]
    assert not missing, missing


@pytest.mark.parametrize("which", ["general", "lean"])
def test_wino24_epilogue_choice_at_its_row_offset_limit(which):
    """14 x 45 000 into a 4096-float-wide buffer -- 13 rows down is past INT_MAX -- must leave the lean epilogue; one step inside
    W * outLd * 16 < 2^31 must still take it.  Both against float64 over the whole output, nothing stored outside the slice."""
    rep = M.run_w24_edge(which)
    print("\nwino24-edge-%-8s %-28s worst err / (u A) %7.3f (c = %5.1f) at %s  peak %5.2f GiB" % (
        which, rep["kernel"], rep["worst"].ratio, rep["c"], rep["worst"].loc, rep["peak"] / 2 ** 30))
    assert rep["kernel"] == "conv3x3_wino24_kernel<%s>" % ("true" if which == "lean" else "false")
    assert not rep["failures"], "\n".join(rep["failures"])


@pytest.mark.parametrize("rid", M.BACKED_IDS)
def test_first_refused_shape_is_refused_with_real_buffers(rid):
    """exactly 2^24 pixels at ld = 64 (4 GiB), or one row of 65536 tile columns: buffers large enough for an unrefused launch, rc 1,
    nothing written"""
    r = M.refusal(rid)
    assert r.backed
    torch.cuda.empty_cache()
    rc, msg, bufs = M.refuse(r, device=True, fill=7.0)
    assert rc == 1 and msg.startswith(r.launcher + ":") and r.arg in msg, (rc, msg)
    assert sum(b.numel() for b in bufs) * 4 <= r.backed
    assert all(bool((b == 7.0).all()) for b in bufs)
    del bufs
    torch.cuda.empty_cache()
