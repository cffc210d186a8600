"""CPU suite: the cases of tests/test_gpu_team_oracle.py without a device -- the restated plans of the team sweep and of
the row panels (csrc/host_sweep.h: team_shape, configure_sweep) give the layout the case tables name at 64, 256 and 304
CUs; the generator's own conditions on the oracle alone; how well conditioned every case is (the oracle against itself
with the observation rows reversed: the spread that sets the case's bound) and how sharp (a 16-row line in all columns
and the rows of one member or panel in one column, scaled by 1 + delta, move the oracle by more than 100 x the bound)."""
import numpy as np
import pytest

import team_oracle_cases as tc


@pytest.mark.parametrize("cid", [s.id for s in tc.CASES])
def test_restated_plans_give_the_layout_the_table_names(cid):
    s = tc.BY_ID[cid]
    for cus in (64, 256, 304):
        M = s.size(cus)
        ts, pp = s.plans(cus)
        ld = tc.roundup16(s.N)
        # the row panels: every context with more than 16384 rows has them, whatever runs the fused step
        assert pp["n_panels"] >= 2 and pp["rows_per_panel"] % 16 == 0 and pp["rows_per_panel"] <= tc.PANEL_MAX_ROWS
        assert 0 < pp["last_panel_rows"] <= pp["rows_per_panel"]
        assert (pp["n_panels"] - 1) * pp["rows_per_panel"] + pp["last_panel_rows"] == ld
        assert 2048 * (pp["ept2"] - 1) < pp["rows_per_panel"] <= 2048 * pp["ept2"] and pp["ept2"] in (4, 5)
        assert (pp["panel_teams"] - 1) * pp["panel_cols"] < M <= pp["panel_teams"] * pp["panel_cols"] and pp["panel_teams"] <= cus
        both = dict(pp, **ts)
        if not s.team:
            assert ts["refusal"] == "switch off" and not ts["on"]
        elif s.expect.get("refusal"):
            assert not ts["on"] and ts["grid"] == 0 and ts["panel_rows"] == 0
        else:
            assert ts["on"] and ts["refusal"] is None and ts["lag"] == s.lag
            d = tc.derived(ts, M)
            cap = tc.member_cap(s.lag)
            assert 2 <= ts["Q"] <= 8 and ts["Q"] == max(2, tc.cdiv(ld, cap)) and ts["panel_rows"] <= cap
            assert sum(d["member_rows"]) == ld and min(d["member_rows"]) > 0 and d["member_rows"][-1] == ts["last_rows"]
            assert ts["lds_bytes"] <= tc.LDS_MAX and ts["grid"] <= cus and ts["grid"] == 8 * ts["tpx"] * ts["Q"]
            assert sum(d["runs"]) == M and max(d["runs"]) == ts["cols_per_team"]
            if s.tpx:       # the cap: the same teams on every device
                assert (ts["tpx"], ts["n_teams"]) == (s.tpx, 8 * s.tpx)
            else:
                assert ts["tpx"] == min(32, cus // 8) // ts["Q"]
            both.update(d)
        for k, v in s.expect.items():       # the table's figures hold at every CU count
            assert both[k] == v, (cid, cus, k, both[k], v)


def test_case_tables_cover_what_they_are_meant_to():
    assert len(tc.BY_ID) == len(tc.CASES)
    assert tc.member_cap(2) == 10208 and tc.member_cap(1) == 10240
    for group in (tc.MEMBERS, tc.RUNS, tc.PANELS):
        assert set(s.reg for s in group) == {"Damping", "MS", "Smoothness", "TV"}
        assert abs(2 * sum(s.fix for s in group) - len(group)) <= 1
    sh = lambda cid: tc.BY_ID[cid].plans()[0]
    der = lambda cid: tc.derived(sh(cid), tc.BY_ID[cid].M)
    # every Q, and the refusal past the last
    assert sorted(set(s.plans()[0]["Q"] for s in tc.MEMBERS)) == [2, 3, 4, 5, 6, 7, 8, 9]
    assert sh("m-81665x40")["refusal"] == "Q > 8" and sh("m-81664x41")["Q"] == 8 and sh("m-81664x41")["grid"] == 64
    # a member at the cap of each lag: 16 idle threads in the fifth slot at lag 2, none at lag 1
    assert der("m-20416x15")["fifth_slot"] == [1008, 1008] and der("l-20480x15")["fifth_slot"] == [1024, 1024]
    # ld2 = 4104: 8 live threads in the fifth slot of member 0; the last member's fifth slot wholly idle
    assert der("m-16385x37")["member_rows"] == [8208, 8192] and der("m-16385x37")["fifth_slot"] == [8, 0]
    # a team without a column next to teams with seven; teams 5 .. 7 without one; one column in all
    assert der("m-61249x49")["runs"] == [7] * 7 + [0] and der("r-16385x49")["runs"] == [7] * 7 + [0]
    assert der("m-51041x5")["runs"] == [1] * 5 + [0] * 3 and der("r-16385x1")["runs"] == [1] + [0] * 7
    # every run length 1 .. 8 at lag 2 (the rotation of three buffers: prologue alone, one turn, a turn plus one and plus
    # two, two turns plus ...), each also as a team's LAST run; 1 .. 4 at lag 1
    assert set(r for s in tc.RUNS + tc.MEMBERS[:-1] for r in tc.derived(s.plans()[0], s.M)["runs"]) == set(range(9))
    assert set(r for s in tc.LAG1 for r in tc.derived(s.plans()[0], s.M)["runs"]) >= {1, 2, 3, 4}
    # the device's own team count: runs of 5 and a last team of 2; runs of 4, one of 1 and a quarter of the teams idle
    for cus, n2, n4 in ((64, 32, 16), (256, 128, 64), (304, 128, 64)):
        a, b = tc.BY_ID["g-16385x5T-3"], tc.BY_ID["g-30625x3T+1"]
        assert (a.plans(cus)[0]["n_teams"], b.plans(cus)[0]["n_teams"]) == (n2, n4)
        assert tc.derived(a.plans(cus)[0], a.size(cus))["runs"] == [5] * (n2 - 1) + [2]
        full = (3 * n4 + 1) // 4
        assert tc.derived(b.plans(cus)[0], b.size(cus))["runs"] == [4] * full + [1] + [0] * (n4 - full - 1)
        assert a.N * a.size(cus) * 8 <= 90e6 and b.N * b.size(cus) * 8 <= 90e6
    # too few CUs for the widest team without the cap playing a part
    assert tc.team_shape(81664, 41, 56)["refusal"] == "too few CUs" and tc.team_shape(16000, 41, 256)["refusal"] == "single panel"
    assert tc.team_shape(81664, 41, 256, env={"GRAVHMC_TEAM": 0})["refusal"] == "switch off"
    assert tc.team_shape(16385, 100, 256, tpx_cap=3)["tpx"] == 3 and tc.team_shape(16385, 100, 256, tpx_cap=99)["tpx"] == 16
    # the row panels: <16, 5> with two columns in flight, <16, 4> with one, 2 .. 8 panels, a short last panel
    pl = lambda cid: tc.BY_ID[cid].plans()[1]
    assert sorted(set(pl(s.id)["n_panels"] for s in tc.PANELS)) == [2, 3, 4, 8]
    assert set((pl(s.id)["ept2"], pl(s.id)["pf"]) for s in tc.PANELS) == {(5, 2), (4, 1)}
    # vec_update_kernel: a second block with ONE live thread; partials beyond its blocks zeroed up to 128
    assert pl("p-16385x257")["update_blocks"] == 2 and 257 - 256 == 1 and pl("p-16385x257")["n_pp"] == 129
    assert (pl("p-16385x300")["panel_cols"], pl("p-16385x300")["panel_teams"]) == (4, 75) and pl("p-16385x300")["n_pp"] == 128
    assert all(s.N * s.size(256) * 8 <= 90e6 for s in tc.CASES)


@pytest.mark.parametrize("cid", [s.id for s in tc.CASES])
def test_case_meets_the_generators_conditions_is_conditioned_and_sharp(cid):
    s = tc.BY_ID[cid]
    d = tc.make(cid)        # (asserts: decisions, lengths, cells on both bounds)
    ref = d.ref
    half = d.T // 2
    assert ref.acc.sum() == d.T - half and (~ref.acc).sum() == half and d.T >= 4
    assert (d.Ls >= 1).all() and (d.Ls <= 6).all() and d.Ls[0, 0] == 1
    assert (d.x0s >= d.low).all() and (d.x0s <= d.high).all()
    np.testing.assert_allclose(d.high - d.low, 3.0 * d.dt, rtol=1e-12)
    dH = ref.out5[:, :, 4] - ref.out5[:, :, 3]
    assert (dH[~ref.acc] > 0.01).all()
    edge = np.exp(-np.maximum(dH, 0.0))
    assert np.allclose(d.us[ref.acc], 0.5 * edge[ref.acc]) and np.allclose(d.us[~ref.acc], 0.5 * (1 + edge[~ref.acc]))
    assert abs(d.dobs.mean()) > 100 * d.dobs.std()
    acc_x = ref.xs[ref.acc]
    assert (acc_x == d.low).any() and (acc_x == d.high).any()
    assert tc.distance(d, ref, tc.replay(d.P, d)) == 0.0
    # conditioning: the oracle against itself with the rows reversed sets the bound; a spread beyond MAX_SPREAD is met
    # with a shorter list in the table, not with a looser bound
    spread, bound = d.spread(), d.bound()
    print("%s: %s%s, T = %d: spread %.2e, bound %.2e" % (cid, d.reg, " + grav_fix" if s.fix else "", d.T, spread, bound))
    assert 0.0 <= spread <= tc.MAX_SPREAD, (cid, spread)
    assert tc.TOL_TRAJ <= bound <= 1e-9
    # sharpness
    assert s.delta in (1e-4, 1e-3)
    for what, rows, cols in d.probes():
        assert 0 <= rows.start < rows.stop <= d.N and 0 <= cols.start < cols.stop <= d.M, (cid, what, rows, cols)
        moved = tc.distance(d, ref, d.perturbed(rows, cols, s.delta))
        print("%s: %s A[%d:%d, %d:%d] (1 + %.0e) moves the oracle by %.2e" % (cid, what, rows.start, rows.stop, cols.start,
                                                                             cols.stop, s.delta, moved))
        assert moved > 100 * bound, (cid, what, moved, bound)


def test_probes_sit_on_the_edges_they_name():
    d = tc.make("m-16385x37")
    pr = dict((k[:40], (r, c)) for k, r, c in d.probes())
    assert pr["a: the last valid 16-row line"[:40]] == (slice(16384, 16385), slice(0, 37))
    assert pr["a: the first line of the last member or panel"[:40]] == (slice(8208, 8224), slice(0, 37))
    assert pr["a: the last line of member or panel 0"[:40]] == (slice(8192, 8208), slice(0, 37))
    assert pr["b: member or panel 0, first column of team 0"[:40]] == (slice(0, 8208), slice(0, 1))
    assert pr["b: the last member or panel, last column of the last non-empty team"[:40]] == (slice(8208, 16385), slice(36, 37))
    # runs of 5: team 3 holds columns 15 .. 19, the column at cnt - 2 is 18
    assert pr["b: a middle member, the column at cnt - 2 of team 3 (finished from LDS)"[:40]] == (slice(8208, 16385), slice(18, 19))
    d = tc.make("p-16385x257")
    assert [c for k, r, c in d.probes() if k.startswith("b: the last")] == [slice(256, 257)]
