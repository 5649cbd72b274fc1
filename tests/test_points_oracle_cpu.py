"""The points oracle (tests/points_oracle.py) judged on its own, without a GPU.

* Every row's claim -- waves and threads per block, LDS bytes, centre and joint tile counts, live points in the last tile, the special
  indices its point list holds -- is asserted against the launch geometry restated in `points_oracle.geometry`, and the table against
  the regimes and the four instantiations it is there to reach.
* Every row is evaluated in float32 on the CPU (`layer_oracle.head_branch`, merged in float32 under the flip test) and must stay within
  1.25 x C_REF32["direct"] of the float64 reference at the addressed pixels -- the condition of tests/test_launch_oracle_cpu.py: the
  reference alone is well inside the bound the kernels are held to.  The same walk asserts the liveness floors.
* `points_oracle.emulate`, a numpy restatement of the kernels' data path, passes every row unmutated; each mutation is rejected at the
  mutated element.  The dropped hidden channel passes `err <= 1e-4 max|ref|` of tests/test_head_points_hip.py: the stated gap.
* The launchers refuse, before any HIP call, a head_conv whose block would exceed 512 threads; ops and the plan builder say the same.
"""
import ctypes
import types

import pytest
import torch

import layer_oracle as lo
import points_oracle as P

NO_DEVICE = not torch.cuda.is_available()
FULL = [r for r in P.ROWS if r.K >= len(P.SPECIALS) and r.J >= 3]


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", [r.id for r in P.ROWS])
def test_row_reaches_what_it_claims(rid):
    row = P.ROW[rid]
    assert P.accepted(row) and set(row.regimes) <= set(P.REGIMES)
    HW = row.H * row.W
    for pairs in (False, True):
        g = P.geometry(row, pairs)
        assert g["nthr"] % 64 == 0 and g["nthr"] <= P.MAX_THREADS and g["lds"] <= P.MAX_LDS
        assert g["nthr"] // 64 * g["ns"] * 32 == row.hc                      # the waves' column tiles cover the hidden channels exactly
        for key, want in row.claim.items():
            if key in ("lds", "lds_pairs"):
                assert P.geometry(row, key == "lds_pairs")["lds"] == want
            else:
                assert g[key] == want, (key, g[key], want)
    g = P.geometry(row, False)
    if "W1" in row.regimes:
        assert (g["nthr"], g["ns"], row.C, g["kgroups"]) == (64, 1, 16, 2)
    if "ODD" in row.regimes:
        assert g["nthr"] & (g["nthr"] - 1) or row.C == 48                   # a block width that is no power of two
    if "LDS" in row.regimes:
        assert min(g["lds"], P.geometry(row, True)["lds"]) > P.LDS_RESERVE and (row.C, row.hc, row.J) == (512, 512, 17)
    if "ONE" in row.regimes:
        assert (row.B, row.K, row.J) == (1, 1, 1) and min(row.H, row.W) == 1 and (g["last_c"], g["last_j"], g["grid"]) == (1, 1, 4)
    if "K256" in row.regimes:
        assert row.K == 256 and HW - row.K == 16 and row.J == 2
    inds, where = P.point_list(row)
    assert tuple(inds.shape) == (row.B, 1 + row.J, row.K) and int(inds[:, 1:].min()) >= 0 and int(inds[:, 1:].max()) < HW
    if row in FULL:
        assert set(where) == set(P.SPECIALS) | {"three_joints", "joint_is_centre"}
        c = inds[0, 0].tolist()
        assert c[where["negative"][2]] < 0 and c[where["plane3"][2]] // HW == 3
        assert c[where["dup"][2]] == c[where["dup2"][2]]
        pix = set(P.pixel(inds[0, 0].long(), HW).tolist())
        edge = {0, row.W - 1, HW - row.W, HW - 1, row.W // 2, HW - row.W + row.W // 2, (row.H // 2) * row.W, (row.H // 2) * row.W + row.W - 1}
        assert edge <= pix and edge <= set(inds[0, row.J].tolist())
        k3, kj = where["three_joints"][2], where["joint_is_centre"][2]
        assert inds[0, 1, k3] == inds[0, 2, k3] == inds[0, 3, k3]
        assert int(inds[0, 1, kj]) == P.pixel(c[1], HW) == HW - 1
        inds2, K2 = P.shuffled(inds, HW)
        assert K2 > row.K and all(set(P.pixel(inds2[b, j].long(), HW).tolist()) == set(P.pixel(inds[b, j].long(), HW).tolist())
                                  for b in range(row.B) for j in range(1 + row.J))
    if "MIRROR" in row.regimes:
        xs = set((P.pixel(inds[0, 0].long(), HW) % row.W).tolist())
        assert row.W % 2 == 1 and {0, row.W // 2, row.W - 1} <= xs
    if "MIRROR-3CYC" in row.regimes:
        perm = row.perm
        assert sorted(perm) == list(range(row.J)) and any(perm[perm[j]] != j for j in range(row.J))      # not an involution
        assert sum(perm[j] != j for j in range(row.J)) == 3 and perm[perm[perm[0]]] == 0


def test_table_reaches_every_regime_and_instantiation():
    kernels = {P.geometry(P.ROW[c.split("/")[0]], c.endswith("pairs"))["kernel"] for c in P.CASES}
    assert kernels == set(P.MUST_COVER)
    assert {g for r in P.ROWS for g in r.regimes} == set(P.REGIMES)
    for entry in P.BOTH:
        rows = [r for r in P.ROWS if entry in r.entries]
        assert {r.J for r in rows if "J" in r.regimes} == {1, 4, 17} if entry == "pairs" else {1, 17} <= {r.J for r in rows}
        geo = [P.geometry(r, entry == "pairs") for r in rows]
        assert {g["nthr"] for g in geo} >= {64, 128, 192, 320, 448, 512} and {r.C for r in rows} >= {16, 48, 64, 512}
        assert any(g["last_c"] == 1 and g["ctiles"] == 2 for g in geo) and any(r.B * r.K == 32 for r in rows)
        assert any(r.B * r.J * r.K % 32 for r in rows)
    assert all(set(r.entries) == {"pairs"} for r in P.ROWS if r.regimes[0].startswith("MIRROR"))
    assert [r for r in P.ROWS if r.entries == P.BOTH] == [r for r in P.ROWS if not r.regimes[0].startswith("MIRROR")]
    # the four refused widths are exactly the accepted-by-divisibility values whose block exceeds the kernels' bound
    wide = [hc for hc in range(32, 513, 32) if P.geometry(P.ROW["w1-c16-hc32"]._replace(hc=hc), False)["nthr"] > P.MAX_THREADS]
    assert tuple(wide) == P.REFUSED_HC and not set(P.SERVED_HC) & set(wide)
    # plans: one arch per distinct logical head geometry
    from centerpose_amd import nets
    assert len({nets.ARCH_HEAD[a] for a in P.PLAN_ARCHS}) == len(P.PLAN_ARCHS)
    assert {nets.ARCH_HEAD[a] for a in lo.ARCHS} == {nets.ARCH_HEAD[a] for a in P.PLAN_ARCHS}


# ---- the float32 yardstick and the unmutated emulation -----------------------------------------------------------------------------------
def _flat_of(case, maps):
    """dense maps {name: [B, n, H, W]} -> the flat output a launch would leave: their values at the addressed pixels, NaN elsewhere"""
    parts = [torch.full((P.G,), float("nan"))]
    for name in P.SPARSE:
        m = P.addressed(case.row, case.inds, name).expand_as(maps[name])
        parts.append(torch.where(m, maps[name].float(), torch.full_like(maps[name], float("nan"), dtype=torch.float32)).reshape(-1))
    parts.append(torch.full((P.G,), float("nan")))
    return torch.cat(parts)


@pytest.mark.parametrize("cid", P.CASES)
def test_float32_yardstick_and_emulation_of_every_row(cid):
    case = P.make_case(cid)
    ref = P.reference(cid)
    o32 = P.evaluate(case.row, case.pairs, case.x, case.sd, torch.float32)
    rep = P.judge_flat(case.row, case.inds, ref, _flat_of(case, {n: o32[n].val for n in P.SPARSE}))
    w = P.worst_of(rep)
    share, live = P.relu_zero_share(case), P.hps_liveness(case.row, case.inds, ref)
    print("\n%-24s worst err / (u A) %.3f (1.25 x C_REF32 = %.2f, c = %.2f) at %s; ReLU zeroes %.3f, live hps share %.3f"
          % (cid, w.ratio, 1.25 * lo.C_REF32["direct"], rep["c"], w.loc, share, live))
    assert not rep["failures"], rep["failures"]
    assert w.ratio <= 1.25 * lo.C_REF32["direct"], "change the row's data, not the table"
    assert rep["c"] == lo.c_for("direct", ref["hps"].K) == lo.LAYER_TOL["direct"]
    assert P.RELU_SHARE[0] < share < P.RELU_SHARE[1] and live > P.HPS_LIVE[1]
    assert 0.3 < float((case.x == 0).float().mean()) < 0.7                  # post-ReLU features
    assert bool(torch.isnan(case.featbuf[0]).all()) and bool(torch.isnan(case.featbuf[-1]).all()) and case.ld > case.row.C
    emu = P.judge_flat(case.row, case.inds, ref, P.emulate(case))
    assert not emu["failures"], emu["failures"]
    if case.row.H * case.row.W > 1:
        inds2, _ = P.shuffled(case.inds, case.row.H * case.row.W)
        assert torch.equal(P.emulate(case, inds=inds2).view(torch.int32), P.emulate(case).view(torch.int32))


# ---- mutations ------------------------------------------------------------------------------------------------------------------------
PTS, WIDE, MIR, CYC = "w1-c16-hc32/points", "wide-c64-hc256/points", "mirror-w7/pairs", "mirror-3cyc/pairs"
MUTANTS = [(PTS, "wrap_border", "left"), (PTS, "next_image", "corner11"), (PTS, "no_modulo", "plane3"), (PTS, "ld_is_C", "corner11"),
           (PTS, "no_relu", "dup"), (PTS, "drop_hidden", "dup"), (WIDE, "drop_hidden", "dup"),
           (MIR, "wrap_border", "right"), (MIR, "next_image", "corner00"), (MIR, "no_relu", "dup"), (MIR, "drop_hidden", "dup"),
           (MIR, "twin_at_x", "corner00"), (MIR, "sign_on_odd", "dup"), (MIR, "no_perm", "dup"), (MIR, "parked_neighbour", "corner01"),
           (CYC, "no_perm", "dup"), (CYC, "perm_inverted", "dup"), (CYC, "twin_at_x", "corner11")]


def _mutant(cid, kind, special):
    case = P.make_case(cid)
    row = case.row
    b, j, k = case.where[special]
    p = int(P.pixel(int(case.inds[b, j, k]), row.H * row.W))
    return case, (b, p // row.W, p % row.W), P.emulate(case, (kind, b, p))


@pytest.mark.parametrize("cid,kind,special", MUTANTS)
def test_mutation_is_rejected_at_the_mutated_element(cid, kind, special):
    assert kind in P.MUTATIONS + P.MUTATIONS_PAIRS
    case, loc, flat = _mutant(cid, kind, special)
    rep = P.judge_flat(case.row, case.inds, P.reference(cid), flat)
    where = {(b, y, x) for _, b, _, y, x in rep["bad"]}
    assert rep["failures"] and loc in where, (loc, where)
    w = P.worst_of(rep)
    assert (w.loc[0], w.loc[2], w.loc[3]) == loc
    if kind != "no_modulo":                                                # (that one also leaves its value where nothing is addressed)
        assert where == {loc}
    if kind in ("sign_on_odd", "no_perm", "perm_inverted", "drop_hidden"):
        assert {n for n, *_ in rep["bad"]} == {"hps"}


def test_every_mutation_of_the_list_is_tried():
    assert {k for _, k, _ in MUTANTS} == set(P.MUTATIONS + P.MUTATIONS_PAIRS)
    assert [c for c, k, _ in MUTANTS if k == "perm_inverted"] == [CYC]


@pytest.mark.parametrize("cid", [WIDE, MIR])
def test_global_max_norm_passes_the_dropped_hidden_channel(cid):
    """the stated gap: `err <= 1e-4 * max|ref|` over the map (tests/test_head_points_hip.py, tests/test_flip_dets_only_hip.py) accepts
    the hps map of the `drop_hidden` mutant that the per-element bound rejects"""
    case, loc, flat = _mutant(cid, "drop_hidden", "dup")
    ref = P.reference(cid)["hps"]
    got = P.split_flat(flat, case.row)[0]["hps"]
    mask = P.addressed(case.row, case.inds, "hps").expand_as(got)
    assert bool(torch.isfinite(got[mask]).all())
    err = (got[mask].double() - ref.val[mask]).abs().max().item()
    j = P.lowest_spread_row(2 * case.row.J)
    assert got[loc[0], j, loc[1], loc[2]] != P.split_flat(P.emulate(case), case.row)[0]["hps"][loc[0], j, loc[1], loc[2]]
    assert err <= 1e-4 * ref.val.abs().max().item()


# ---- the refusal ------------------------------------------------------------------------------------------------------------------------
def _call(entry, hc):
    """the C entry point with dummy, aligned, non-null pointers on a 1 x 1 map: (rc, cp_last_error())"""
    from centerpose_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)
    if entry == "pairs":
        rc = L.cp_head_points_pairs_f32(p, 16, p, p, p, p, p, p, p, 1, 1, 1, 16, 1, 1, hc, ctypes.c_void_p(0))
    else:
        rc = L.cp_head_points_f32(p, 16, p, p, p, p, p, p, 1, 1, 1, 16, 1, 1, hc, ctypes.c_void_p(0))
    return rc, L.cp_last_error().decode()


@pytest.mark.parametrize("entry", P.BOTH)
@pytest.mark.parametrize("hc", P.REFUSED_HC)
def test_launcher_refuses_an_over_wide_block(entry, hc):
    """rc 1 before any HIP call (so no launch can happen, with or without a device), the message names hc and the thread count"""
    rc, msg = _call(entry, hc)
    name = "head_points_pairs" if entry == "pairs" else "head_points"
    assert rc == 1, (rc, msg)
    assert msg.startswith(name + ": head_conv=%d needs a block of %d threads" % (hc, 2 * hc)) and "512" in msg, msg
    assert "multiples of 32 up to 256, multiples of 64 up to 512" in msg


@pytest.mark.parametrize("entry", P.BOTH)
@pytest.mark.parametrize("hc", P.SERVED_HC)
def test_served_widths_pass_that_check(entry, hc):
    """where no device is present an unrefused call comes back with rc 2 (the first HIP call fails): these carry dummy pointers and run
    only there; on the device tests/test_points_parity_hip.py launches all four widths for real"""
    if not NO_DEVICE:
        pytest.skip("a device is present: the call would launch on dummy pointers")
    rc, msg = _call(entry, hc)
    assert rc == 2 and "threads" not in msg, (rc, msg)


def test_ops_and_plan_builder_mirror_the_refusal():
    from centerpose_amd import engine, ops
    for hc in range(32, 513, 32):
        served = hc not in P.REFUSED_HC
        assert (ops.check_head_points_hc(hc, "x") is None) == served
        g = P.geometry(P.ROW["w1-c16-hc32"]._replace(hc=hc), False)
        assert ops.head_points_block(hc) == (g["ns"], g["nthr"])
    for hc in (0, 16, 48, 544):
        assert "multiple of 32" in ops.check_head_points_hc(hc, "x")
    t = torch.zeros(1)
    for hc in P.REFUSED_HC:
        with pytest.raises(AssertionError, match="head_conv=%d needs a block of %d threads" % (hc, 2 * hc)):
            ops.head_points_launch(torch.zeros(1, 1, 1, 16), t, t, t, t, t, t, hc=hc, J=1, K=1)
        with pytest.raises(AssertionError, match="head_conv=%d needs a block of %d threads" % (hc, 2 * hc)):
            ops.head_points_pairs_launch(torch.zeros(2, 1, 1, 16), t, t, t, t, t, t, t, hc=hc, J=1, K=1)
        with pytest.raises(ValueError, match="head_conv=%d needs a block of %d threads" % (hc, 2 * hc)):
            engine.PlanBuilder.head_points_consts(None, types.SimpleNamespace(t=torch.zeros(1, 1, 1, 64)), "head", hc)
