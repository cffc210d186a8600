"""CPU suite: the cases of tests/test_gpu_resident_oracle.py without a device -- the restated plans of the resident
kernels (csrc/host_resident.h, csrc/host_resbatch.h) give the layout the case table names at 256 and 304 CUs (cases on at
most 64 workgroups: at 64 CUs too), the generator's own conditions on the oracle alone, the launch structure of the
single-chain cases, and how sharp every case is: one entry of A scaled by 1 + delta must move the oracle's trajectories
by more than 100 TOL_TRAJ, at the entries where a kernel changes what it does with a column or a row."""
import numpy as np
import pytest

import resident_oracle_cases as rc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _cu_counts(spec):
    return (256, 304) + ((64,) if spec.wgs <= 64 else ())


@pytest.mark.parametrize("cid", [s.id for s in rc.CASES])
def test_restated_plan_gives_the_layout_the_table_names(cid):
    s = rc.BY_ID[cid]
    plans = []
    for cus in _cu_counts(s):
        p = s.plan(cus)
        assert p is not None and rc.resident_usable(p, s.reg), (cid, cus)
        d = rc.derived(p, s.M)
        both = dict(p, **d)
        for k, v in s.expect.items():
            assert both[k] == v, (cid, cus, k, both[k], v)
        # the partition itself
        assert (p["nwg"] - 1) * p["cpw"] < s.M <= p["nwg"] * p["cpw"] and p["nwg"] <= min(s.wgs, rc.RES_MAX_WG)
        assert p["lds"] <= rc.LDS_MAX and p["lds"] == rc.chains_lds_bytes(p, 1)
        assert 64 * p["rc"] * 2 >= p["ld"] > 64 * (p["rc"] - 1) * 2 and p["ct"] * p["rc"] <= 20
        assert sum(d["cn"]) == p["nwg"] and max(d["cn"]) <= 32 and d["nch"] <= max(1, min(d["cn"][:d["ncl"]]))
        assert sum(d["chunk_rows"]) == p["ld"] and 0 < d["last_nc"] <= p["cpw"]
        assert not (p["split"] and p["stream"])
        if p["split"]:
            assert p["ct"] >= 1 and p["lds_cols"] == max(0, p["cpw"] - 8 * p["ct"])
            assert rc.resident_lds_doubles(p["ld"], p["cpw"], 1, p["cpw"], False) * 8 > rc.LDS_MAX
        if p["stream"]:
            assert p["ct"] == 0 and 0 < p["lds_cols"] < p["cpw"]
            assert rc.resident_lds_doubles(p["ld"], p["cpw"], 1, p["lds_cols"] + 1, False) * 8 > rc.LDS_MAX
        plans.append((p, d))
    assert all(pl == plans[0] for pl in plans[1:])          # GRAVHMC_RESIDENT_WGS: the same partition on every device
    p = plans[0][0]
    if s.group == "lockstep":
        ls = rc.resbatch_plan(p, s.reg, s.C, s.fix)
        if s.lockstep is False:
            assert ls is None and rc.chains_fit(p, s.reg, s.C)
        else:
            assert ls is not None and all(ls[k] == v for k, v in s.lockstep.items()), (cid, ls)
            assert ls["lds"] <= rc.LDS_MAX and 32 * ls["ks"] >= p["ld"] > 32 * (ls["ks"] - 5)
    if s.group in ("turns", "fit"):
        assert rc.resbatch_plan(p, s.reg, s.C, s.fix, env={"GRAVHMC_RESIDENT_BATCH": 0}) is None


def test_case_tables_cover_what_they_are_meant_to():
    plan = lambda cid: rc.BY_ID[cid].plan()
    der = lambda cid: rc.derived(plan(cid), rc.BY_ID[cid].M)
    assert len(rc.BY_ID) == len(rc.CASES)
    for cases in (rc.SINGLE, rc.LOCKSTEP):
        assert set(s.reg for s in cases) == {"Damping", "MS", "Smoothness", "TV"}
        assert abs(2 * sum(s.fix for s in cases) - len(cases)) <= 1
    # the stencil regularisers on true 3-D shapes whose rows (nx cells) and planes (nx ny cells) straddle workgroups
    for cases in (rc.SINGLE, rc.LOCKSTEP):
        for reg in ("Smoothness", "TV"):
            assert any(s.reg == reg and min(s.shape) > 1 and s.shape[2] % s.plan()["cpw"] != 0
                       and (s.shape[1] * s.shape[2]) % s.plan()["cpw"] != 0 and s.plan()["nwg"] > 1 for s in cases), reg
    assert sorted(set(s.reg for s in rc.SPLIT) & {"TV", "Smoothness"}) == ["Smoothness", "TV"]
    # every register / LDS instantiation the plans can reach without a switch: rc 1 .. 8, ct 0 .. 4
    assert set(s.plan()["rc"] for s in rc.SINGLE) == set(range(1, 9))
    assert set(s.plan()["ct"] for s in rc.SINGLE) == {0, 1, 2, 3, 4}
    assert max(s.plan()["ct"] * s.plan()["rc"] for s in rc.SINGLE) == 20
    # the exchange: fewer workgroups than clusters, clusters of unequal size, the second reducer slot (member 16) alone,
    # 32 members, owners without a row
    assert der("x-2x7")["ncl"] == 7 and der("x-16x9")["ncl"] == 5 and der("x-1x1")["ncl"] == 1
    assert der("x-129x130")["cn"][:2] == [17, 17] and der("x-250x256")["cn"] == [32] * 8
    assert der("x-130x137")["nch"] * der("x-130x137")["ch"] > plan("x-130x137")["ld"] and der("x-130x137")["chunk_rows"][-1] == 0
    assert der("x-384x255")["chunk_rows"][-2:] == [7, 0]
    assert der("x-16x2047")["chunk_rows"] == [1] * 16 + [0] * 16
    assert der("x-33x70")["passes"] == 2 and der("x-33x70")["ch"] % 32 != 0 and der("x-127x37")["ch"] == 4 * 32
    # rows: idle lanes of the last register chunk at ld = 400 (lanes 200 - 192 = 8 of 64 busy)
    assert plan("r-385x200")["ld"] // 2 - 64 * 3 == 8 and der("r-385x200")["nch"] == 2
    assert plan("r-256x330")["cpw"] > 32 and plan("r-1000x136")["rc"] * rc.cdiv(17, 8) == 24
    # split: register + LDS columns; a last workgroup without an LDS column whose waves 4 .. 7 have no second column
    assert (plan("s-641x330")["ct"] * 8, plan("s-641x330")["lds_cols"]) == (16, 17)
    assert (der("s-700x290")["last_nc"] - der("s-700x290")["last_nl"], der("s-700x290")["last_nl"]) == (24, 7)
    assert der("s-1023x145")["last_nc"] == 12 < 16 and der("s-1023x145")["last_nl"] == 0
    # stream: batches of eight and remainders of the streamed columns
    for cid, streamed, last in (("m-1024x203", 11, 11), ("m-1000x300", 20, 16), ("m-1024x305", 2, 0), ("m-1024x1737", 10, 0)):
        p, d = plan(cid), der(cid)
        assert p["cpw"] - p["lds_cols"] == streamed and d["last_nc"] - d["last_nl"] == last, (cid, p, d)
    # chains taking turns: C = 2, 5, 16 on four matrices.  By the restated fit test of gh_batch_init the stream case
    # holds at most six chains (its LDS is filled with columns for one chain): sixteen go to the MFMA batch, as five do
    # on 1024 x 203
    fits = dict((s.id, rc.chains_fit(s.plan(), s.reg, s.C)) for s in rc.TURNS + rc.FIT)
    assert [k for k, v in sorted(fits.items()) if not v] == ["f-1024x203-c5", "t-m-1000x300-c16"]
    p = plan("m-1000x300")
    assert rc.chains_fit(p, "TV", 6) and not rc.chains_fit(p, "TV", 7)
    p = plan("m-1024x203")
    assert rc.chains_fit(p, "MS", 4) and not rc.chains_fit(p, "MS", 5)
    # lock-step: every KS, both NT, the LDS refusal with and without grav_fix
    ls = [rc.resbatch_plan(s.plan(), s.reg, s.C, s.fix) for s in rc.LOCKSTEP]
    assert set((l["ks"], l["nt"]) for l in ls if l) >= {(5, 1), (10, 1), (10, 2), (15, 2), (20, 1), (20, 2)}
    assert [s.id for s, l in zip(rc.LOCKSTEP, ls) if l is None] == ["l-641x80", "l-256x330", "l-640x200"]
    p = plan("l-430x256")
    assert rc.resbatch_lds_doubles(432, 32, True) * 8 == 160656 <= rc.LDS_MAX < rc.resbatch_lds_doubles(448, 32, True) * 8
    p = plan("l-640x200")
    assert rc.resbatch_lds_doubles(640, 25, False) * 8 > rc.LDS_MAX >= rc.chains_lds_bytes(p, 16)
    assert rc.rb_ldp(432) == 434 and rc.rb_ldp(640) == 658 and rc.rb_ldp(16) == 18 and rc.rb_ldp(624, True) == 624


def test_resident_plan_switches():
    # GRAVHMC_RESIDENT_WGS is clamped to the CU count; _REGS=0 drops the register copy (and split with it); _CT forces
    # the register columns of the split mode; the stream budget refuses
    assert rc.resident_plan(600, 6000, 256)["cpw"] == 24 and rc.resident_plan(600, 6000, 256)["ct"] == 3
    assert rc.resident_plan(600, 6000, 256, env={"GRAVHMC_RESIDENT_WGS": 1000})["nwg"] == 250
    # (304 CUs: 20 columns per workgroup would make 300 workgroups, more than the exchange holds -- refused as the code
    # stands; with the workgroups limited to 256 the C1 partition is back)
    assert rc.resident_plan(600, 6000, 304) is None
    assert rc.resident_plan(600, 6000, 304, env={"GRAVHMC_RESIDENT_WGS": 256})["cpw"] == 24
    assert rc.resident_plan(600, 6000, 256, env={"GRAVHMC_RESIDENT_REGS": 0})["ct"] == 0
    assert rc.resident_plan(600, 6000, 256, env={"GRAVHMC_RESIDENT": 0}) is None
    assert rc.resident_plan(1025, 100, 256) is None and rc.resident_plan(16, 512 * 256 + 1, 256) is None
    p = rc.resident_plan(641, 330, 256, env={"GRAVHMC_RESIDENT_WGS": 10})
    assert (p["split"], p["ct"]) == (True, 2)
    p = rc.resident_plan(641, 330, 256, env={"GRAVHMC_RESIDENT_WGS": 10, "GRAVHMC_RESIDENT_CT": 3})
    assert (p["split"], p["ct"], p["lds_cols"]) == (True, 3, 9)
    p = rc.resident_plan(641, 330, 256, env={"GRAVHMC_RESIDENT_WGS": 10, "GRAVHMC_RESIDENT_REGS": 0})
    assert (p["split"], p["stream"], p["ct"]) == (False, True, 0) and p["lds_cols"] < 33
    assert rc.resident_plan(641, 330, 256, env={"GRAVHMC_RESIDENT_WGS": 10, "GRAVHMC_RESIDENT_REGS": 0,
                                                "GRAVHMC_RESIDENT_STREAM": 0}) is None
    assert rc.resident_plan(1024, 30000, 256, env={"GRAVHMC_RESIDENT_STREAM_MB": 100}) is None
    # the stencil regularisers: at most 44 cells per workgroup (12 doubles of the reduction buffer per cell)
    assert rc.resident_stencil_fits(44) and not rc.resident_stencil_fits(45)
    # the C layer's LDS arithmetic at C1, read off csrc/resident.hip.h and csrc/resbatch.hip.h
    assert rc.resident_lds_doubles(608, 24, 1, 24, False) == 24 * 608 + 608 + 528 + 16 + 8 * 24 + 48 + 8 + 16
    assert rc.resbatch_lds_doubles(608, 24, False) == 24 * 626 + 8 * 6 * 64 + 24 * 16 + 608 + 722


@pytest.mark.parametrize("cid", [s.id for s in rc.CASES])
def test_case_meets_the_generators_conditions_and_is_sharp(orc, cid):
    s = rc.BY_ID[cid]
    d = rc.make(cid)        # (asserts: decisions, lengths, cells on both bounds, the launch structure)
    ref = d.ref
    assert ref.acc.sum() >= 3 and (~ref.acc).sum() >= 3 and d.C * d.T >= 10
    assert (d.Ls >= 1).all() and (d.Ls <= 6).all() and (d.Ls == 1).any()
    assert (d.x0s >= d.low).all() and (d.x0s <= d.high).all()
    np.testing.assert_allclose(d.high - d.low, 3.0 * d.dt, rtol=1e-12)
    dH = ref.out5[:, :, 4] - ref.out5[:, :, 3]
    assert (dH[~ref.acc] > 0.01).all()
    edge = np.exp(-np.maximum(dH, 0.0))
    assert np.allclose(d.us[ref.acc], 0.5 * edge[ref.acc]) and np.allclose(d.us[~ref.acc], 0.5 * (1 + edge[~ref.acc]))
    assert abs(d.dobs.mean()) > 100 * max(d.dobs.std(), 1e-300) or d.N == 1
    acc_x = ref.xs[ref.acc]
    assert (acc_x == d.low).any() and (acc_x == d.high).any()
    assert rc.distance(d, ref, rc.replay(d.P, d)) == 0.0
    if d.C == 1:
        # five launches, tags running on; an odd number of evaluations in front of another launch; K = 1; L = 1
        ev = d.launch_evaluations()
        assert len(ev) == 5 and [b - a for a, b in d.launches()] == [3, 1, 4, 2, 2]
        assert ev[1] == 3 and d.Ls[0, 0] == 1
        k = d.stop_index()
        assert ref.acc[0, k] and ref.acc[0, :k + 1].sum() == rc.STOP_AT and k + 1 < d.T
    if s.delta is None:     # (the matrices of the turn-taking cases are those of single-chain cases)
        return
    assert s.delta <= 1e-3
    for what, entry in d.probes():
        assert 0 <= entry[0] < d.N and 0 <= entry[1] < d.M, (cid, what, entry)
        moved = rc.distance(d, ref, d.perturbed(orc, entry, s.delta))
        print("%s: %s A%r (1 + %.0e) moves the oracle by %.2e" % (cid, what, entry, s.delta, moved))
        assert moved > 100 * rc.TOL_TRAJ, (cid, what, entry, moved)


@pytest.mark.parametrize("dims", [1, 3])
@pytest.mark.parametrize("C", [1, 3])
def test_compressed_forward_spread_between_the_two_host_forms(dims, C):
    """F applied as a dense float64 matrix against DWT-then-SpMV on the case's own trajectories: the same decisions, and
    a distance that sets the device's bound (max(TOL_TRAJ, 10 x spread))."""
    d = rc.compressed(dims, C)
    assert d.ref.acc.sum() >= 3 and (~d.ref.acc).sum() >= 3 and (d.Ls == 1).any()
    assert d.F.shape == (42, 120) and d.csr.shape[1] >= 120 and 0 < d.csr.nnz < d.csr.shape[0] * d.csr.shape[1]
    # the dense form is the same operator: one forward to rounding
    x = d.x0s[0]
    a, b = d.P.misfit_and_grad(x)[2], d.P_dense.misfit_and_grad(x)[2]
    assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
    assert rc.distance(d, d.ref, rc.replay(d.P, d)) == 0.0
    s = d.spread()
    print("compressed forward %dD, %d chain(s): spread between the host forms %.2e, device bound %.2e" % (dims, C, s, d.bound()))
    assert 0.0 <= s < 1e-9 and d.bound() >= rc.TOL_TRAJ
    # the resident kernels' plan for it at 256 CUs: one cell per workgroup, a register copy (the dots' own operand)
    p = rc.resident_plan(d.N, d.M, 256)
    assert (p["cpw"], p["nwg"], p["ct"], p["ld"]) == (1, 120, 1, 48) and rc.rb_ldp(48, True) == 48


def test_probes_sit_on_the_edges_they_name():
    d = rc.make("s-700x290")
    pr = dict(d.probes())
    assert pr["last register-held column of a middle workgroup"][1] == 4 * 37 + 23
    assert pr["first LDS column of a middle workgroup"][1] == 4 * 37 + 24
    assert pr["column 8 of a workgroup"][1] == 4 * 37 + 8
    assert pr["first row of the last non-empty chunk, first column of the last workgroup"] == (0, 7 * 37)
    d = rc.make("m-1024x203")
    pr = dict(d.probes())
    assert [pr[k][1] - 3 * 29 for k in ("last LDS column", "first streamed column", "last streamed column")] == [17, 18, 28]
    d = rc.make("x-384x255")
    assert dict(d.probes())["first row of the last non-empty chunk, first column of the last workgroup"] == (29 * 13, 254)
