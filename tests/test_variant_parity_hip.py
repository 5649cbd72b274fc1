"""The kernel instantiations only large launches reach, one stand-alone launch each, against a float64 reference element by element
(tests/launch_oracle.py on top of tests/layer_oracle.py).

The launchers pick the instantiation from the block count, so the network plans of tests/test_layer_parity_hip.py never reach the
fused head kernels, the 128-row GEMM tiles, the 64 x 128 DCN tile, the 64-channel Winograd block, the V-stationary kernel or the tile
walk of the persistent kernels; tests/test_conv_hip.py forces them but judges by the global max norm.  Here every row of
`launch_oracle.ROWS` forces one variant at the smallest shape at which it can still go wrong and asserts

* the launch dispatched to exactly the instantiation the row names (`Launch.kernel`),
* every element inside `c_for(family, K) u A` (LAYER_TOL, calibrated on the CPU; `tile_A` for the Winograd families; K = the whole
  reduction for split launches, judged on the reduced output),
* nothing stored past the channels the launch was given, exact zeros in the padding channels, the same bits from a second run,
* live data (LIVE_FLOOR: DCN samples inside the map, unsaturated masks and sigmoid heads),
* for the persistent kernels, that the case is in the walking regime on THIS device: ntiles >= 2 CUs OCC + 1, so some blocks own
  three tiles (two chained prefetches) and the others two.

`MUST_COVER` lists every instantiation the switch statements of cp_conv2d_f32, cp_launch_conv3x3_wino, cp_launch_head3x3_1x1,
cp_launch_head3x3_1x1_w24, cp_dcn_v2_f32, cp_launch_conv3x3_c16, cp_stem7x7_f32 and cp_launch_stem3x3 can produce for NHWC inference.
Run with -s for the worst err / (u A) of every row and per family.
"""
import pytest

import launch_oracle as L
import layer_oracle as lo

pytestmark = pytest.mark.gpu

MUST_COVER = (
    "igemm_conv_kernel<64, 64, 2, 2, 32, false>", "igemm_conv_kernel<128, 64, 2, 2, 32, false>", "igemm_conv_kernel<128, 128, 2, 2, 32, false>",
    "igemm_conv_kernel<128, 32, 4, 1, 32, false>", "igemm_conv_kernel<256, 16, 4, 1, 16, false>",
    "igemm_conv_kernel<256, 16, 4, 1, 16, true>", "igemm_conv_kernel<128, 32, 4, 1, 32, true>", "igemm_conv_kernel<128, 64, 2, 2, 32, true>",
    "dcn_igemm_kernel<64, 64, 2, 2, 32>", "dcn_igemm_kernel<64, 128, 2, 2, 32>", "dcn_igemm_kernel<128, 64, 2, 2, 32>",
    "dcn_igemm_kernel<128, 32, 4, 1, 32>", "dcn_igemm_kernel<64, 32, 4, 1, 16>",
    "conv3x3_wino_kernel<1, 1, 16, 2>", "conv3x3_wino_kernel<1, 2, 16, 2>", "conv3x3_wino_kernel<2, 1, 16, 2>",
    "conv3x3_wino_vs64_kernel<0, 0>", "conv3x3_wino24_kernel<true>", "conv3x3_wino24_kernel<false>",
    "conv3x3_wino_vs64_kernel<1, 0>", "conv3x3_wino_vs64_kernel<2, 0>", "conv3x3_wino_vs64_kernel<0, 1>", "conv3x3_wino_vs64_kernel<1, 1>",
    "conv3x3_wino_vs64_kernel<2, 1>",
    "head_wino24_kernel<1, 0>", "head_wino24_kernel<2, 0>", "head_wino24_kernel<0, 1>", "head_wino24_kernel<1, 1>", "head_wino24_kernel<2, 1>",
    "conv3x3_c16_kernel<1, 1, 8, 32, 4, 2>", "conv3x3_c16_kernel<2, 1, 8, 32, 2, 2>", "conv3x3_c16_kernel<1, 2, 8, 16, 3, 2>",
    "conv3x3_c16_kernel<2, 2, 8, 16, 3, 1>",
    "stem7x7_c16_kernel<16, 1, 7>", "stem7x7_c16_kernel<64, 2, 7>", "stem7x7_c16_kernel<64, 2, 3>",
    "stem7x7_kernel<16, 1, 8, 64>", "stem7x7_kernel<64, 2, 8, 32>", "stem7x7_kernel<64, 1, 8, 32>", "stem7x7_kernel<16, 2, 8, 64>",
    "splitk_reduce_kernel",
)
WALKING = ("conv3x3_c16_kernel", "stem7x7_c16_kernel")
_reports = {}


def _report(rid):
    """the report of row `rid`, run once per module; a row that raised raises again for whoever asks"""
    if rid not in _reports:
        try:
            _reports[rid] = L.run_row(rid)
        except Exception as e:                    # noqa: BLE001 -- kept, so that the coverage test fails with it rather than run it again
            _reports[rid] = e
    if isinstance(_reports[rid], Exception):
        raise _reports[rid]
    return _reports[rid]


@pytest.mark.parametrize("rid", [r.id for r in L.ROWS])
def test_forced_variant_matches_fp64_reference(rid):
    row, rep = L.ROW[rid], _report(rid)
    w = rep["worst"]
    print("\n%-24s %-7s %s  worst err / (u A) %.3f (c = %.1f) at %s%s" % (rid, row.family, " + ".join(rep["kernels"]), w.ratio, rep["c"], w.loc,
                                                                        "  tiles %d >= %d" % rep["walk"] if rep["walk"] else ""))
    assert rep["kernels"][0] == row.kernel
    assert rep["kernels"][1:] == ["splitk_reduce_kernel"] * (row.p["S"] > 1)
    if row.kernel.startswith(WALKING):
        assert rep["walk"] is not None and rep["walk"][0] >= rep["walk"][1], "not in the walking regime: %d tiles, %d needed" % rep["walk"]
    assert not rep["failures"], "\n".join(rep["failures"])


def test_every_launcher_instantiation_is_covered():
    """the union of the dispatched names holds every entry of MUST_COVER, every persistent one from a row in the walking regime; a row
    that has not run yet runs here, one that raised fails this test too"""
    reps = {r.id: _report(r.id) for r in L.ROWS}
    covered = set().union(*(rep["kernels"] for rep in reps.values()))
    missing = [k for k in MUST_COVER if k not in covered]
    assert not missing, missing
    walked = {rep["kernels"][0] for rep in reps.values() if rep["walk"] and rep["walk"][0] >= rep["walk"][1]}
    assert not [k for k in MUST_COVER if k.startswith(WALKING) and k not in walked]
    worst = {}
    for rid, rep in reps.items():
        fam = L.ROW[rid].family
        if rep["worst"].ratio > worst.get(fam, (-1.0, ""))[0]:
            worst[fam] = (rep["worst"].ratio, rid)
    for fam, (ratio, rid) in sorted(worst.items()):
        print("\nworst err / (u A) %-7s %8.3f (LAYER_TOL %.1f)  %s" % (fam, ratio, lo.LAYER_TOL[fam], rid))
