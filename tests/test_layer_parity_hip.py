"""Every launch of every network plan against a float64 reference of its hook, element by element (tests/layer_oracle.py).

Each case builds the plan of one arch behind a RecordingBuilder, runs it one hook at a time from the hook's own device inputs and
asserts, per output element, |out - ref64| <= c u A (LAYER_TOL, calibrated on the CPU), bit-equality for the exact hooks, zero padding
channels, that the data is live (LIVE_FLOOR: DCN samples inside the map, unsaturated masks and sigmoid heads), and that every launch
of the plan belongs to exactly one record (the builder needs a device, so that bookkeeping is asserted here rather than in the CPU
file).  Run with -s for the per-arch report: launches checked, kernels covered, worst err / (u A) per family with its layer.

The single-launch conv3x3_wino24_kernel wants >= 256 blocks of 16 x 16 pixels x 32 channels (`ops.wino24_wanted`), which no layer has
at these sizes: two cases lift that floor with CP_WINO24_RULE=32,16,1, as tests/test_engine_hip.py does, so that the plans' 3x3 layers
run on it.  Not in MUST_COVER because it cannot be reached at these sizes: the fused head kernels (head3x3_1x1: `ops.head3x3_1x1_eligible`
wants >= 512 blocks of 8 x 16 pixels, the 40 x 24 head map of B = 3 has 30, and no switch lowers that floor).  They, and every other
instantiation the launchers pick only for large block counts (128-row GEMM tiles, the 64 x 128 DCN tile, the 64-channel and V-stationary
Winograd blocks, the tile walk of the persistent kernels), are judged by the same oracle one forced launch at a time in
tests/test_variant_parity_hip.py.
"""
import pytest

import layer_oracle as lo

pytestmark = pytest.mark.gpu

ENVS = {"default": {}, "nogroup_nowino": {"CP_GROUP": "0", "CP_WINOGRAD": "0"}, "wino24": {"CP_WINO24_RULE": "32,16,1"}}
SHAPES = [(a, 2, 64, 96) for a in lo.ARCHS] + [("dla_34", 3, 160, 96)]
CASES = [s + (e,) for s in SHAPES for e in ("default", "nogroup_nowino")] + [("dla_34", 3, 160, 96, "wino24"), ("res_50", 2, 64, 96, "wino24")]
MUST_COVER = ("igemm_conv_kernel", "pw_conv_kernel", "conv3x3_patch_kernel", "conv3x3_c16_kernel", "conv3x3_wino_kernel", "conv3x3_wino24_kernel",
              "conv3x3_wino24_group", "dcn_igemm_kernel", "stem7x7", "splitk_reduce_kernel", "dw_deconv2_add_kernel", "dw_deconv_add_kernel",
              "maxpool_nhwc_kernel", "sum_up",
              "dwconv_nhwc_kernel", "global_avgpool_kernel", "scale_add_kernel", "shuffle_concat_kernel")
_reports = {}


def _report(case):
    """the report of `case`, run once per module; a case that raised raises again for whoever asks"""
    if case not in _reports:
        arch, B, H, W, env = case
        with pytest.MonkeyPatch.context() as mp:
            for k, v in ENVS[env].items():
                mp.setenv(k, v)                   # before the builder is constructed: it reads the switches in __init__ / emit_*
            try:
                _reports[case] = lo.run_plan(arch, B, H, W)
            except Exception as e:                # noqa: BLE001 -- kept, so that the coverage test fails with it rather than run it again
                _reports[case] = e
    if isinstance(_reports[case], Exception):
        raise _reports[case]
    return _reports[case]


@pytest.mark.parametrize("case", CASES, ids=["%s-%dx%dx%d-%s" % c for c in CASES])
def test_every_launch_matches_fp64_reference(case):
    rep = _report(case)
    print("\n" + lo.format_report("%s B=%d %dx%d %s" % case, rep))
    assert rep["checked"] == rep["launches"] > 0
    assert None not in rep["kernels"]
    assert not rep["failures"], "%d of %d records fail:\n%s" % (len(rep["failures"]), rep["records"], "\n".join(rep["failures"][:20]))


def test_kernel_families_covered():
    """the union of the kernels of all cases holds at least one of every family; a case that has not run yet runs here, one that
    raised fails this test too"""
    covered = set().union(*(_report(c)["kernels"] for c in CASES))
    print("\nkernels covered:", ", ".join(sorted(covered)))
    missing = [f for f in MUST_COVER if not any(f in k for k in covered)]
    assert not missing, missing
