"""CPU suite: the cases of tests/test_gpu_lonsym_oracle.py without a device -- the restated plans of the shift-invariant
store (csrc/host_lonsym.h, csrc/host_lonres.h) give the layout the case table names at 64, 256 and 304 CUs (wherever the
case's workgroups fit), the table covers the edges it is meant to, the generator's own conditions on the oracle alone, and per
problem the two conditions that keep the device's bound honest: the oracle on K as the store holds it (every entry from
the class's entry at the same shift against the cell of longitude index 0, mirrored rows from their partners) agrees with the
oracle on its own K to TOL_TRAJ / 10, and one table entry's worth of K scaled by 1 + delta moves the oracle by more than
100 TOL_TRAJ at the entries where a kernel changes what it does."""
import numpy as np
import pytest

import lonsym_oracle_cases as lc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _cu_counts(spec):
    return [cus for cus in (64, 256, 304) if cus >= spec.cus_min]


@pytest.mark.parametrize("cid", [s.id for s in lc.CASES])
def test_restated_plan_gives_the_layout_the_table_names(cid):
    s = lc.BY_ID[cid]
    plans = []
    for cus in _cu_counts(s):
        p = s.plan(cus)
        assert "refused" not in p, (cid, cus, p)
        d = lc.derived(p)
        both = dict(p, **d)
        for k, v in s.expect.items():
            assert both[k] == v, (cid, cus, k, both[k], v)
        n, na, nc, nf = s.n, s.na, s.nc, p["nf"]
        assert (p["n"], p["na"], p["nc"]) == (n, na, nc) and nf == n // 2 + 1
        assert p["max_extra"] == s.max_extra == max(0, int(s.counts.max()) - 1) and p["n_xslots"] == int((s.counts > 1).sum())
        if p["form"] == "direct":
            assert p["direct_ok"] and p["KB"] * p["W"] >= n > (p["KB"] - 1) * p["W"] and p["AG"] * 64 >= na > (p["AG"] - 1) * 64
            assert p["AG"] * p["KB"] <= (p["thr"] // 64) * p["items"] and p["lds"] <= 160 * 1024 - 512 and na * n <= 8192
        if p["form"] == "registers":
            assert nf <= 64 and na <= 64 and p["hlds"] <= 160 * 1024 - 512 and 1 <= p["rw"] <= 4 and p["rw"] == min(p["rp"], 4)
            rows = sorted(c for it in range(d["passes"]) for c in range(nc))
            seen = sorted(w + b * p["hgrid"] * p["rw"] + r * p["hgrid"] for b in range(d["passes"]) for w in range(p["hgrid"])
                          for r in range(p["rw"]) if w + b * p["hgrid"] * p["rw"] + r * p["hgrid"] < nc
                          and w + b * p["hgrid"] * p["rw"] < nc)
            assert seen == list(range(nc)) and len(rows) == nc * d["passes"]     # every row once
            assert (d["passes"] > 1) == (p["hgrid"] * p["rw"] < nc)
        if p["form"] == "streamed":
            assert p["nfp"] % 8 == 0 and 0 <= p["nfp"] - nf < 8 and p["pairs"] == lc.cdiv(nf, lc.LW_THREADS)
            assert sum(d["part_rows"]) == p["witems"] and min(d["part_rows"]) > 0
            assert p["wparts"] == 1 or min(d["part_rows"][:-1]) >= 8
        if p["resident_planned"]:
            assert p["form"] == "registers" and na <= p["nwg"] <= min(cus, lc.LR_MAXWG) and p["nwg"] * p["rw"] >= nc
            assert n <= 126 and s.max_extra <= 2 and p["resident_lds"] <= lc.LDS_MAX
            assert sum(d["cn"]) == p["nwg"] and len(set(d["owners"])) == na      # one class per owner
        plans.append((p, d))
    # (the switches fix the layout: the same on every device that has the case's workgroups, but for the grids that follow
    # the CU count)
    drop = lambda p: dict((k, v) for k, v in p.items() if k not in ("grid", "wgrid"))
    assert all(drop(pl[0]) == drop(plans[0][0]) and pl[1] == plans[0][1] for pl in plans[1:]), cid


def test_case_tables_cover_what_they_are_meant_to():
    plan = lambda cid: lc.BY_ID[cid].plan()
    der = lambda cid: lc.derived(plan(cid))
    forms = lambda cases: [s.plan()["form"] for s in cases]
    assert max(s.N * s.M for s in lc.CASES) <= 8e6
    for cases in (lc.PAIRS + lc.PARTS, lc.REGISTERS, lc.RESIDENT, lc.SLOTS, lc.DIRECTS):
        assert set(s.reg for s in cases) == {"Damping", "MS", "Smoothness", "TV"}
        assert abs(2 * sum(s.fix for s in cases) - len(cases)) <= max(2, len(cases) // 4)
        assert any(s.shuffle for s in cases) and not all(s.shuffle for s in cases)
    # the streamed sweep's three instantiations at their edges (nf = 256 | 257, 512 | 513), 1025 refused
    assert [(s.n, s.plan()["pairs"]) for s in lc.PAIRS] == [(510, 1), (511, 1), (512, 2), (1022, 2), (1023, 2), (1024, 3)]
    assert set(forms(lc.PAIRS + lc.PARTS)) == {"streamed"}
    assert lc.REFUSALS[0].n == 1025 and lc.REFUSALS[0].plan() == {"refused": lc.DIRECT_WHY[1]}
    # mirror: none, a self-mirrored equator row among the pairs, switched off; parts around 8 rows with ragged ends, fixed by
    # GRAVHMC_LW_WAVES_PER_CU; na = 65; odd n
    assert not plan("w-asym-7")["wmirror"] and plan("w-mirror")["wmirror"] and not plan("w-mirror-off")["wmirror"]
    assert lc.mirror_items(lc.BY_ID["w-mirror"].rows, lc.BY_ID["w-mirror"].classes)[1] == [4, 3, -1, 9, 8, -1]
    assert [plan("w-asym-%d" % k)["witems"] for k in (7, 8, 9, 17)] == [7, 8, 9, 17]
    assert der("w-asym-17")["part_rows"] == [9, 8] and der("w-asym-33")["part_rows"] == [9, 9, 9, 6]
    assert plan("w-asym-33-one")["wparts"] == 1 and lc.BY_ID["w-asym-33-one"].data == "w-asym-33"
    assert plan("w-na65")["na"] == 65 and plan("w-na65")["form"] == "streamed" and plan("d-na64")["na"] == 64
    assert any(s.n % 2 == 1 for s in lc.PAIRS) and any(s.n % 2 == 1 and s.plan()["wmirror"] for s in lc.PARTS)
    # the register form on the launches per phase: n = 2, 3, 125, 126, 127 | 128; the class groups' edges; rw 1 .. 4 with
    # ragged ends under the stencil regularisers; the launches' loop; the one-launch epilogue on two
    reg = [s for s in lc.REGISTERS if s.plan()["form"] == "registers"]
    assert sorted(set(s.n for s in reg)) == [2, 3, 5, 9, 12, 16, 125, 126, 127] and plan("h-n128")["form"] == "streamed"
    assert all(not s.plan()["resident_planned"] for s in lc.REGISTERS)
    assert sorted(s.na for s in reg if s.id != "h-n127-on")[:9] == [1, 3, 16, 17, 32, 33, 48, 49, 64]
    assert set(s.plan()["rw"] for s in reg) == {1, 2, 3, 4}
    for rw in (2, 3, 4):
        assert any(s.plan()["rw"] == rw and lc.derived(s.plan())["ragged"] and s.reg in ("TV", "Smoothness") for s in reg), rw
    assert sorted(s.nc for s in reg if "GRAVHMC_LONSYM_ROWS" in s.env) == [7, 9, 10, 10, 10, 13, 13]
    assert plan("h-na49")["rp"] == 5 and der("h-na49")["passes"] == 2
    assert sum(1 for s in reg if s.env.get("GRAVHMC_LONSYM_FUSED") == 1) == 2
    assert plan("h-n127")["form"] == "registers" and not plan("h-n127-on")["resident_planned"]
    # the persistent launch: nwg = 1, 2, 7, 8, 9, 17, 40, 64, 256; clusters of one and two; E smaller than a cluster;
    # hgrid == na and na - 1; rw = 2, 3, 4 ragged under the stencil kinds; n = 126; na = 64; max_extra 0, 2, 3
    on = [s for s in lc.RESIDENT if s.plan()["resident_planned"]]
    assert sorted(s.plan()["nwg"] for s in on) == [1, 2, 3, 3, 4, 5, 7, 8, 9, 17, 40, 64, 256]
    assert der("p-7")["cn"] == [1] * 7 + [0] and der("p-9")["cn"][0] == 2 and der("p-256")["cn"] == [32] * 8
    assert der("p-40-e4")["E"] == 4 < 5 == der("p-40-e4")["cn"][0] and der("p-40-e4")["idle_members"] == 8
    assert [s.id for s in lc.RESIDENT if not s.plan()["resident_planned"]] == ["p-refused", "p-rp5-loop", "p-x3"]
    assert plan("p-refused")["hgrid"] == plan("p-refused")["na"] - 1 and plan("p-8")["nwg"] == plan("p-8")["na"]
    assert plan("p-2")["nwg"] == plan("p-2")["na"] and plan("p-na64")["nwg"] == 64 == plan("p-na64")["na"]
    for rw in (2, 3, 4):
        assert any(s.plan()["rw"] == rw and lc.derived(s.plan())["ragged"] and s.reg in ("TV", "Smoothness") for s in on), rw
    assert plan("p-n126")["n"] == 126 and plan("p-x3")["max_extra"] == 3
    assert set(s.max_extra for s in on) == {0, 1, 2}
    # the slots: four kinds on four forms, one problem per kind; empty slots, a class of one observation, 2 and 3 in a slot
    assert len(lc.SLOTS) == 16 and len(set(s.data for s in lc.SLOTS)) == 4
    for kind in ("ones", "empty", "single", "multi"):
        four = [s for s in lc.SLOTS if s.slots == kind]
        assert [s.plan()["form"] for s in four] == ["direct", "registers", "streamed", "registers"]
        assert [s.plan()["resident_planned"] for s in four] == [False, False, False, True]
    c = lc.BY_ID["s-empty-direct"].counts
    assert (c[-1] == 0).sum() == 4 and c[:-1].min() == 1
    assert lc.BY_ID["s-single-direct"].counts[0].sum() == 1
    c = lc.BY_ID["s-multi-direct"].counts
    assert sorted(c[c > 1]) == [2, 2, 3, 3] and len(set(np.nonzero(c > 1)[0])) >= 3
    assert lc.BY_ID["s-ones-direct"].max_extra == 0 and lc.BY_ID["s-ones-direct"].n_xslots == 0
    # three chains: turns in the persistent launch and own streams on the ragged rw = 3 layout, own streams on <2>
    assert [(s.C, s.T, s.plan()["resident_planned"]) for s in lc.CHAINS] == [(3, 5, True), (3, 5, False), (3, 5, False)]
    assert plan("c-rw3-turns")["rw"] == 3 and der("c-rw3-streams")["ragged"] and plan("c-w512-streams")["pairs"] == 2
    # the direct form: W 8 | 16, 512 | 1024 threads, AG 1 | 2, one and four items per wave, and its four refusals
    dp = [s.plan() for s in lc.DIRECTS]
    assert set(forms(lc.DIRECTS)) == {"direct"} and [s.n for s in lc.DIRECTS][:8] == [8, 16, 63, 64, 65, 128, 144, 512]
    assert set((p["W"], p["thr"]) for p in dp) == {(8, 1024), (16, 512), (16, 1024)}
    assert set(p["AG"] for p in dp) == {1, 2} and set(p["items"] for p in dp) == {1, 4}
    assert [r.plan()["refused"] for r in lc.REFUSALS[1:]] == [lc.DIRECT_WHY[k] for k in (1, 2, 2, 3, 4)]
    # (513 is the first n the direct form refuses for its work items: 512 runs with four per wave)
    assert lc.plan(512, lc.band(1, 1, 0.0, 1.0), lc.ASYM3, 0, 0, 256, lc.DIRECT)["items"] == 4


def test_plan_switches():
    rows, cl = lc.band(10, 5, -20.0, 4.0), lc.classes_at((-3.0, 2.0, 8.0))
    p = lc.plan(120, rows, cl, 1, 3, 256)
    assert (p["form"], p["rp"], p["rw"], p["hgrid"], p["resident_planned"]) == ("registers", 1, 1, 50, True)
    # GRAVHMC_LONSYM_ROWS: at least r rows per workgroup, never fewer than the CU count asks for
    for r, want in ((2, (2, 2, 25)), (3, (3, 3, 17)), (4, (4, 4, 13)), (5, (5, 4, 10))):
        p = lc.plan(120, rows, cl, 1, 3, 256, {"GRAVHMC_LONSYM_ROWS": r})
        assert (p["rp"], p["rw"], p["hgrid"]) == want and p["resident_planned"] == (r <= 4)
    assert lc.plan(120, rows, cl, 1, 3, 8, {"GRAVHMC_LONSYM_ROWS": 2})["rp"] == 7
    assert lc.plan(120, rows, cl, 1, 3, 256, {"GRAVHMC_LONSYM_RESIDENT": 0})["resident_planned"] is False
    assert lc.plan(120, rows, cl, 1, 3, 256, {"GRAVHMC_LONSYM_WIDE": 2})["form"] == "streamed"
    assert lc.plan(120, rows, cl, 1, 3, 256, {"GRAVHMC_LONSYM_HARMONIC": 0})["form"] == "direct"
    assert lc.plan(126, rows, cl, 1, 3, 256)["resident_planned"] and lc.plan(126, rows, cl, 3, 3, 256)["resident_planned"] is False
    p = lc.plan(127, rows, cl, 1, 3, 256)
    assert p["form"] == "registers" and not p["resident_planned"] and lc.plan(128, rows, cl, 1, 3, 256)["form"] == "streamed"
    # the C layer's LDS arithmetic, read off csrc/lonsymh.hip.h, lonsymw.hip.h and lonres.hip.h at C4 (n = 120, na = 61)
    assert lc.lonsymh_lds_doubles(120, 61, 61, 1) == 2 * 61 * 61 + 240 + (18 * 61 + 120) + 16
    assert lc.lonres_lds_doubles(120, 61, 61, 1) - lc.lonsymh_lds_doubles(120, 61, 61, 1) == 2 + 128 + 128 + 512 + 128 + 768 + 64
    assert lc.lonsymw_lds_doubles(360, 181) == 720 + 22 * 181 + 16


@pytest.mark.parametrize("cid", sorted(set(s.data for s in lc.CASES)))
def test_case_meets_the_generators_conditions_is_conditioned_and_sharp(orc, cid):
    s = lc.BY_ID[cid]
    d = lc.make(cid)        # (asserts: decisions, lengths, cells on both bounds, the launch structure)
    ref = d.ref
    assert ref.acc.sum() >= 3 and (~ref.acc).sum() >= 3 and d.C * d.T >= 8
    assert (d.Ls >= 1).all() and (d.Ls <= 6).all() and (d.Ls == 1).any()
    assert (d.x0s >= d.low).all() and (d.x0s <= d.high).all()
    dH = ref.out5[:, :, 4] - ref.out5[:, :, 3]
    assert (dH[~ref.acc] > 0.01).all()
    assert abs(d.dobs.mean()) > 100 * d.dobs.std() or d.N <= 4
    acc_x = ref.xs[ref.acc]
    assert (acc_x == d.low).any() and (acc_x == d.high).any()
    if d.C == 1:
        assert [b - a for a, b in d.launches()] == [3, 1, 4, 2, 2] and d.Ls[0, 0] == 1
    assert (d.gfix is not None) == s.fix and d.obs[0].size == s.N == d.a_of.size
    # the geometry is what the counts say, in the order the engine gets it
    got = np.zeros_like(s.counts)
    np.add.at(got, (d.a_of, d.m_of), 1)
    assert np.array_equal(got, s.counts)
    if s.shuffle:
        assert (np.diff(d.a_of * s.n + d.m_of) < 0).any()
    # K is shift-invariant to the oracle's own spread: rebuilt from the table it is the same problem
    users = [q for q in lc.CASES if q.data == cid]
    mirror = any(q.plan()["wmirror"] for q in users)
    assert lc.distance(d, ref, lc.replay(d.P, d)) == 0.0
    for m in sorted(set((False, mirror))):
        Ks = d.symmetrised(orc, m)
        spread = float((np.abs(Ks - d.K) / np.abs(d.K)).max())
        far = d.far(lc._problem(orc, d, Ks)[0])
        print("%s: K as the store holds it%s: entries differ by %.1e of themselves, the oracle's results by %.2e"
              % (cid, " (mirrored rows from their partners)" if m else "", spread, far))
        assert far <= lc.TOL_TRAJ / 10, (cid, m, far)
    assert s.delta <= 1e-3
    probes = d.probes()
    assert len(probes) >= 2
    for what, probe in probes:
        c, a, shifts, how = probe
        assert 0 <= c < s.nc and 0 <= a < s.na and all(0 <= q < s.n for q in shifts), (cid, what, probe)
        moved = d.far(d.perturbed(orc, probe, s.delta))
        print("%s: %s, T[%d][%d]%r (1 + %.0e) moves the oracle by %.2e" % (cid, what, c, a, shifts[:3], s.delta, moved))
        assert moved > 100 * lc.TOL_TRAJ, (cid, what, probe, moved)


def test_probes_sit_on_the_edges_they_name():
    pr = dict(lc.make("h-na49").probes())
    assert pr["last row, last class, last shift"] == (12, 48, [8], None)
    assert pr["first row of the last workgroup or part, first class of the last class group, shift 0"][:2] == (2, 48)
    pr = dict(lc.make("w-asym-17").probes())
    assert pr["first row of the last workgroup or part, first class of the last class group, shift 0"][:2] == (9, 0)
    assert pr["the highest frequency: alternating signs over the shifts"][2] == list(range(130))
    d = lc.make("p-17-rw3")
    pr = dict(d.probes())
    c, a, shifts, how = pr["a slot that holds three observations, against the cell under it"]
    assert d.spec.counts[a, how[1]] == 3 and pr["last row, last class, last shift"][0] == 49
