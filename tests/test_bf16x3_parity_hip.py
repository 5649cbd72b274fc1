"""The split-bf16 implicit GEMM (igemm_bf16x3_kernel<BM, BN>, opt-in) on the device, under tests/bf16x3_oracle.py.

* every row of `bf16x3_oracle.ROWS`: one forced launch (plus `splitk_reduce` where it is split) -- the exact kernel name, every element inside
  `c_for("direct", K) u A` of float64, nothing stored outside the launch's channels and images, zero padding channels, the same bits twice;
* the exact-answer cases on all four instantiations: BIT FOR BIT;
* the weight splitter against its NumPy restatement, every dword;
* the res_50 and dla_34 plans with the switch on (what bench.py's `res_50_b8_split_bf16` times): every launch against float64 at unchanged
  bounds, every eligible launch on the kernel and no other; a plan file compiled with the switch on through the C runtime;
* the launcher's refusals, with real buffers that must stay untouched.

tests/test_bf16x3_oracle_cpu.py proves what these cases can and cannot see.  The two rows at the 32-bit offset limit run with
tests/test_limit_parity_hip.py (`sb-3x3-s1`, `sb-1x1`).  Run with -s for the report (profiles/bf16x3_parity_report.txt).
"""
import time

import numpy as np
import pytest
import torch

import bf16x3_oracle as S
import layer_oracle as lo

pytestmark = pytest.mark.gpu


def _run(fn, *args):
    """fn(*args); a device error ends the session: nothing more is launched on a device that has faulted"""
    try:
        return fn(*args)
    except Exception as e:                        # noqa: BLE001
        if "hip" in ("%s %s" % (type(e).__name__, e)).lower():
            pytest.exit("device error, nothing more is launched: %s" % e, returncode=1)
        raise


# ---- 1. forced launches against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", [r.id for r in S.ROWS])
def test_row_matches_fp64_reference(rid, monkeypatch):
    row = S.ROW[rid]
    t0 = time.time()
    rep = _run(S.run_row, rid, monkeypatch.setenv)
    w = rep["worst"]
    print("\n%-20s %-52s worst err / (u A) %7.3f (c = %4.1f) at %-18s %4.1f s" % (rid, " + ".join(rep["kernels"]), w.ratio, rep["c"], w.loc,
                                                                               time.time() - t0))
    assert rep["kernels"][0] == row.kernel                                  # exactly: ops.split_bf16_tile falls back to BN = 64 silently
    assert rep["kernels"][1:] == ["splitk_reduce_kernel"] * (row.p["S"] > 1)
    assert w.ratio <= rep["c"]
    assert not rep["failures"], "\n".join(rep["failures"])


# ---- 2. exact answers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", ["%dx%d" % t for t in S.TILES])
@pytest.mark.parametrize("kind", S.EXACT_KINDS)
def test_exact_answer_bit_for_bit(kind, tile, monkeypatch):
    """scale = 1, shift = 0, no activation: the output IS the selected operand times a power of two.  Rests on the bf16 MFMA returning a
    representable sum exactly."""
    rep = _run(S.run_exact, kind, tile, monkeypatch.setenv)
    bm, bn = tile.split("x")
    print("\n%-11s %-30s %d of %d elements differ, largest distance %d ulp %s" % (kind, rep["kernel"], rep["mismatches"], rep["total"], rep["ulp"],
                                                                               rep["pattern"]))
    assert rep["kernel"] == S.KERNEL % (int(bm), int(bn))
    assert rep["guard"], "stored outside the channels / images the launch was given"
    assert rep["mismatches"] == 0, "first at (b, c, y, x) = %s: %r != %r; %s" % (rep["first"] + (rep["pattern"],))


# ---- 3. the splitter -----------------------------------------------------------------------------------------------------------------------
def _w(rows, K, seed):
    return S.full24((rows, K), torch.Generator().manual_seed(seed), -20, 20).numpy()


@pytest.mark.parametrize("name,rows,ldw,K", [("rows64-K48", 64, 64, 48), ("nsub4", 256, 64, 64), ("grid-stride", 512, 512, 4608)])
def test_splitter_bit_for_bit(name, rows, ldw, K):
    w = _w(rows, K, 11 + rows)
    got, want = _run(S.device_split, w, ldw), S.split_weights_np(w, ldw).reshape(-1)
    assert got.size == want.size == rows * (K // 16) * 24
    if name == "grid-stride":
        assert got.size > 8192 * 256                                        # more dwords than the launch has threads
    bad = S.splitter_mismatch(got, want)
    assert bad is None, "dword %d: %08x != %08x" % (bad, got[bad], want[bad])
    assert got[-1] == want[-1]


def test_splitter_domain_edges():
    """+-0, ties at both levels, x1 rounding up, terms in bf16's subnormal range, the top binade's upper half and +-inf: pinned through the
    splitter only (how the MFMA treats subnormal operands is not measured here)"""
    v = S.domain_edges()
    w = np.zeros((64, 112), np.float32)
    w.reshape(-1)[:v.size] = v
    w.reshape(-1)[v.size:2 * v.size] = v[::-1]                              # every value in an even and an odd half
    assert 2 * v.size <= w.size and v.size % 2 == 0
    got, want = _run(S.device_split, w, 64), S.split_weights_np(w, 64).reshape(-1)
    bad = S.splitter_mismatch(got, want)
    assert bad is None, "dword %d: %08x != %08x" % (bad, got[bad], want[bad])


# ---- 4. the plans bench.py times -----------------------------------------------------------------------------------------------------------
def _eligible(f):
    """the rule of ops.conv2d_launch, restated on the descriptor: generic, NHWC, ldw % 64 == 0, 16-byte-aligned sources, not the c16 shape"""
    c16 = f["kh"] == 3 and f["kw"] == 3 and f["nsrc"] == 1 and f["srcC0"] == 16 and f["Cout"] <= 32
    return f["fn"] == "cp_conv2d_f32" and not f["inNCHW"] and f["ldw"] % 64 == 0 and f["aligned"] and not c16


@pytest.mark.parametrize("arch", ["res_50", "dla_34"])
def test_plan_with_the_switch_on(arch, monkeypatch):
    from centerpose_amd import ops
    monkeypatch.setattr(ops, "SPLIT_BF16", True)                            # read when a plan is compiled
    monkeypatch.setenv("CP_SPLIT_BF16_MINBLOCKS", "0")
    rep = _run(lo.run_plan, arch, 2, 64, 96)
    print("\n" + lo.format_report("%s B=2 64x96 split-bf16" % arch, rep))
    assert rep["checked"] == rep["launches"] > 0 and not rep["failures"], "\n".join(rep["failures"][:20])
    on = [f for f in rep["launch_list"] if (f["kernel"] or "").startswith("igemm_bf16x3_kernel<")]
    print("  %d of %d launches on igemm_bf16x3_kernel: %s" % (len(on), rep["launches"], sorted({f["kernel"] for f in on})))
    assert on
    for f in rep["launch_list"]:
        # every cp_conv2d_f32 of these plans is built with tile = 0; a tile code in the descriptor now is the split kernel's
        split = f["kernel"].startswith("igemm_bf16x3_kernel<")
        if f["fn"] != "cp_conv2d_f32":
            assert not split, f
            continue
        assert split == _eligible(f) == (3000000 <= f["tile"] < 4000000), f


def test_plan_file_with_split_weights_through_the_c_runtime(tmp_path, monkeypatch):
    """the pre-split weights travel as a float32 tensor of bf16 bits: a plan compiled with the switch on, saved and loaded by the C runtime,
    gives the Python engine's outputs bit for bit"""
    from centerpose_amd import cplan, engine, ops, synth
    monkeypatch.setattr(ops, "SPLIT_BF16", True)
    monkeypatch.setenv("CP_SPLIT_BF16_MINBLOCKS", "0")
    B, H, W = 2, 64, 96
    eng = engine.Engine("res_50", synth.make_state_dict("res_50", seed=9), B, H, W, use_graph=False)
    x = synth.make_images(B, H, W, seed=81).cuda()
    want = [t.clone() for t in eng(x)]
    assert any((la.kernel or "").startswith("igemm_bf16x3_kernel<") for _, _, _, la in eng.launches)
    path = str(tmp_path / "sb.cpplan")
    eng.save_plan(path)
    plan = cplan.CPlan(path, use_graph=False)
    got = plan.forward(x)
    torch.cuda.synchronize()
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    plan.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", [r.id for r in S.REFUSALS])
def test_refused_before_any_launch(rid):
    ref = next(r for r in S.REFUSALS if r.id == rid)
    rc, msg, bufs = _run(S.refuse, ref, True)
    assert rc == 1 and msg.startswith("conv2d") and ref.text in msg, (rc, msg)
    assert bufs and all(bool(torch.isnan(b).all()) for b in bufs)
