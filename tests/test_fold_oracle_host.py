"""CPU suite: the cases of tests/test_gpu_fold_oracle.py without a device -- per case (a) what gh_fold_detect and
gh_fold_detect_pair (csrc/host_fold.h) answer, against the permutations, orbit tables and work list that
tests/fold_oracle_cases.py builds from the coordinates, (b) the oracle on Aw against the oracle on Aw averaged over
each orbit (the store holds orbit means), (c) forced decisions far from the Metropolis edge, (d) cells clamped at
both bounds, (e) how sharp the case is: a folded row or a work item of Aw scaled by 1 + delta must move the oracle
by more than 100 TOL_TRAJ.  Then the table's coverage and the restated sweep plan at 64, 256 and 304 CUs against
values read off csrc/host_sweep.h and csrc/host_fold.h."""
import numpy as np
import pytest

import fold_oracle_cases as fc
from test_fold_host import FOLD_ON, detect
from test_fold_pair_host import PAIR_CELLS, PAIR_OBS, PAIR_ON, detect_pair

CUS = (64, 256, 304)
PAIR_CODES = {"on": PAIR_ON, "switched off": PAIR_ON, "observations not square": PAIR_OBS,
              "cells not square": PAIR_CELLS}


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def plan_runs(s, cus, wg_per_cu=None):
    lay = fc.dense_layout(s.N, s.M, cus, s.min_cols, wg_per_cu)
    return fc.fold_plan(s.items(), lay["grid"], cus)


def kinds(s, cus=256):
    """the work items of a paired case, workgroup by workgroup: "S" a single orbit, "P" a pair"""
    sym = fc.Symmetry(*fc.geometry(s), square=True)
    seq = "".join("S" if o2 < 0 else "P" for _, o2 in sym.work)
    out, at = [], 0
    for n in plan_runs(s, cus):
        out.append(seq[at:at + n])
        at += n
    return out


@pytest.mark.parametrize("cid", [s.id for s in fc.CASES])
def test_case_meets_its_conditions_and_is_sharp(orc, cid):
    s = fc.BY_ID[cid]
    d = fc.make(cid)                 # (asserts (c) and (d))
    sym, ref = d.sym, d.ref

    # (a) detection, and the tables restated from the coordinates
    rc, oi, co = detect(d.obs, d.b6)
    assert rc == FOLD_ON
    assert np.array_equal(oi, sym.obs_img) and np.array_equal(co, sym.cell_orbit)
    assert oi.shape == (s.nF, 4) and co.shape == (s.M // 4, 4)
    rc, pr, ot, ct, work = detect_pair(d.obs, d.b6)
    assert rc == FOLD_ON and pr == PAIR_CODES[s.pair_reason], (cid, pr)
    if s.square:
        assert np.array_equal(ot, sym.obs_tau) and np.array_equal(ct, sym.cell_tau)
        assert np.array_equal(work, sym.work)
        assert (int((work[:, 1] >= 0).sum()), int((work[:, 1] < 0).sum())) == s.counts()
    else:
        assert work.shape[0] == 0 and s.counts() == (0, 0)
    assert fc.fold_taken(s.N, s.paired) and s.rows <= fc.FOLD_MAX_ROWS
    # the heights: all images of an observation share theirs bit for bit, and a topography case is not flat
    z = d.obs[2]
    for g in range(4):
        assert np.array_equal(z[sym.obs_g[g]], z)
    assert (np.ptp(z) > 50.0) == s.topo
    if s.layers is not None:
        assert len(set(np.round(d.b6[:, 5] - d.b6[:, 4], 9))) == len(s.layers) > 1

    # (b) conditioning: the oracle on the orbit means
    Am = sym.mean(d.Aw)
    assert fc.relmax(Am, d.Aw) <= 1e-7           # (FOLD_MAX_DEV: the build's own sanity bound)
    cond = fc.distance(d, ref, fc.replay(d.problem(orc, Am), d))
    assert cond <= fc.TOL_TRAJ / 10, (cid, cond)

    # (c) decisions
    dH = ref.out5[:, 4] - ref.out5[:, 3]
    assert ref.acc.sum() >= 2 and (~ref.acc).sum() >= 2
    assert (dH[~ref.acc] > 0.01).all()
    edge = np.exp(-np.maximum(dH, 0.0))
    us = np.array([u for _, _, u in d.trajs])
    assert np.allclose(us[ref.acc], 0.5 * edge[ref.acc]) and np.allclose(us[~ref.acc], 0.5 * (1 + edge[~ref.acc]))
    assert all(1 <= L <= 6 for L, _, _ in d.trajs)
    # (d) bounds
    lo, hi = d.clamped()
    assert lo > 0 and hi > 0
    assert (d.x0 >= d.low).all() and (d.x0 <= d.high).all()
    # replaying gives the reference back, bit for bit
    assert fc.distance(d, ref, fc.replay(d.P, d)) == 0.0

    # (e) sharpness
    assert s.delta in (1e-4, 1e-3, 1e-2)
    runs = plan_runs(s, 256)
    probes = d.probes(runs)
    assert len(probes) == (4 if s.group == "runs" else 3)
    images = 8 if s.paired else 4
    for name, rows, cols in probes:
        n = len(rows if rows is not None else cols)
        assert n == images or (s.paired and n == 4), (name, n)     # (on the diagonal an orbit is its own partner)
        other = d.perturbed(orc, rows, cols, s.delta)
        moved = fc.distance(d, ref, other, mg=False)         # the trajectories alone: the stricter reading
        moved_mg = fc.mg_distance(other.mg, ref.mg)
        print("%s: %s (1 + %.0e) moves the oracle's trajectories by %.2e, its misfit and gradient by %.2e; orbit "
              "means: %.2e; clamped %d / %d" % (cid, name, s.delta, moved, moved_mg, cond, lo, hi))
        assert moved > 100 * fc.TOL_TRAJ and moved_mg > 100 * fc.TOL_TRAJ, (cid, name, moved, moved_mg)


def test_case_table_covers_what_it_is_meant_to():
    cases = fc.CASES
    assert len(fc.BY_ID) == len(cases)
    for paired in (False, True):
        mine = [s for s in cases if s.paired == paired]
        assert set(s.rows for s in mine) == {1, 2, 3, 4, 5}
        # a full last group (every thread's last row live) and a nearly empty one (fewer than a wave of 64 threads)
        assert any(s.nF % 512 == 0 for s in mine)
        assert any(s.rows > 1 and 0 < s.nF - (s.rows - 1) * 512 < 64 for s in mine)
        # no padding row (nF == ldF) under idle threads: the row they re-read is real, only the mask keeps it out
        assert any(s.nF == s.ldF and s.nF % 512 != 0 for s in mine)
    # (the paired kernel's LDS ends at nF = 2544: its fullest last group is the benchmark's)
    assert any(s.paired and s.nF == 1024 for s in cases) and any(s.paired and s.nF == 2500 for s in cases)
    assert any(s.nF == 2560 and not s.paired for s in cases)
    assert any(s.nF < 16 for s in cases) and any(s.nF == 1 for s in cases)
    assert max(s.nF for s in cases if s.paired) <= 2544
    assert fc.pair_lds(4 * 2544) <= fc.PAIR_MAX_LDS < fc.pair_lds(4 * 2545)
    # the shapes of the row edges
    want = {"U-2x2": (1, 16, 1), "U-6x6": (9, 16, 1), "U-32x64": (512, 512, 1), "U-24x86": (516, 528, 2),
            "U-64x64-off": (1024, 1024, 2), "U-64x96": (1536, 1536, 3), "U-70x88": (1540, 1552, 4),
            "U-80x128": (2560, 2560, 5), "P-44": (484, 496, 1), "P-46": (529, 544, 2), "P-64": (1024, 1024, 2),
            "P-90": (2025, 2032, 4), "P-92": (2116, 2128, 5), "P-100": (2500, 2512, 5)}
    for cid, rows in want.items():
        s = fc.BY_ID[cid]
        assert (s.nF, s.ldF, s.rows) == rows and s.paired == cid.startswith("P"), cid
    # regularisers round-robin, each at five rows
    count = dict((r, sum(s.reg == r for s in cases)) for r in fc.REGS)
    assert max(count.values()) - min(count.values()) <= 1, count
    assert set(s.reg for s in cases if s.rows == 5) == set(fc.REGS)
    # geometry: even counts (the group acts freely), small meshes
    for s in cases:
        assert s.cells[0] % 2 == 0 and s.cells[1] % 2 == 0 and s.obs[0] % 2 == 0 and s.obs[1] % 2 == 0
        assert 8 <= s.M <= 300 and s.N * s.M * 8 <= 8 << 20
        if s.paired:
            assert s.obs[0] == s.obs[1] and s.cells[0] == s.cells[1]
    # run lengths, on the 256 CUs of the MI355X
    runs = dict((s.id, plan_runs(s, 256)) for s in cases)
    lengths = set(n for r in runs.values() for n in r)
    assert {1, 2, 3, 4} <= lengths and any(n >= 5 for n in lengths)
    for paired in (False, True):
        mine = [s for s in cases if s.paired == paired and s.group == "runs"]
        assert any(len(runs[s.id]) == 1 and runs[s.id][0] == s.items() > 1 for s in mine)      # one workgroup takes all
        assert any(len(runs[s.id]) == s.items() for s in mine)                                 # one item each
    short = [r for r in runs.values() if len(r) > 1 and r[-1] < r[0]]
    assert any(r[-1] % 2 == 0 for r in short) and any(r[-1] % 2 == 1 for r in short)
    assert any(r[-1] % 2 != r[0] % 2 for r in short)
    assert [runs[k] for k in ("U-run5553", "U-run666", "U-run99", "U-run18")] == [[5, 5, 5, 3], [6, 6, 6], [9, 9], [18]]
    # work lists of the paired sweep: singles only; a single first, last, and between two pairs
    singles = [s for s in cases if s.paired and s.counts()[0] == 0]
    assert len(singles) == 2 and all(set("".join(kinds(s))) == {"S"} for s in singles)
    mixed = [k for s in cases if s.paired and s.group == "runs" and s.counts()[0] for k in kinds(s)]
    assert any(k[0] == "S" and "P" in k for k in mixed) and any(k[-1] == "S" and "P" in k for k in mixed)
    assert any("PSP" in k for k in mixed)
    assert kinds(fc.BY_ID["P-mix-22221"]) == ["SP", "SS", "PS", "SP", "S"]
    assert kinds(fc.BY_ID["P-mix-444"]) == ["SPPS", "PSSP", "PSPS"]
    assert kinds(fc.BY_ID["P-mix-54"]) == ["SPSSP", "SSPS"]
    # one shuffled and one topography case per kernel
    for group in ("shuffled", "topography"):
        assert sorted(s.paired for s in cases if s.group == group) == [False, True]
    assert all(s.shuffle for s in cases if s.group == "shuffled")
    assert all(s.topo for s in cases if s.group == "topography")


@pytest.mark.parametrize("cus", CUS)
def test_restated_plan_at_three_cu_counts(cus):
    for s in fc.CASES:
        lay = fc.dense_layout(s.N, s.M, cus, s.min_cols)
        # the dense grid of a case is within the CUs whatever the residency the grid is sized for, and the same:
        # the fold's grid is then min(dense grid, items) whatever its occupancy
        for wpc in (1, 2, 3, 4):
            assert fc.dense_layout(s.N, s.M, cus, s.min_cols, wpc)["grid"] == lay["grid"] <= cus, s.id
        runs = plan_runs(s, cus)
        assert sum(runs) == s.items() and len(runs) <= lay["grid"] and all(n == runs[0] for n in runs[:-1])
        assert 0 < runs[-1] <= runs[0]
        assert len(runs) <= lay["n_teams"]          # pp_part: one partial per launched workgroup, the rest zeroed
        if s.runs is not None:
            assert runs == s.runs, (s.id, runs)
        if s.N > 1024:
            # ld > 1024: one team per workgroup, GRAVHMC_MIN_COLS columns each
            assert lay["tw"] > 1 and lay["cols_per_team"] == s.min_cols and lay["grid"] == fc.cdiv(s.M, s.min_cols)
        else:
            assert lay["tw"] == 1 and lay["n_teams"] == 4 * lay["grid"]
    # values read off configure_sweep
    assert fc.dense_layout(2064, 72, cus, 18)["grid"] == 4 and fc.dense_layout(2064, 72, cus, 72)["grid"] == 1
    assert fc.dense_layout(36, 16, cus, 2) == {"tw": 1, "cols_per_team": 2, "n_teams": 8, "grid": 2, "wg_per_cu": 4}
    widths = [fc.dense_layout(n, 72, cus)["tw"] for n in (1024, 1025, 4096, 4097, 6144, 6145, 10240)]
    assert widths == [1, 4, 4, 8, 8, 16, 16]
    assert fc.dense_layout(2064, 72, cus)["wg_per_cu"] == (4 if cus == 64 else 2)
    assert fc.fold_plan(18, 4, cus) == [5, 5, 5, 3] and fc.fold_plan(9, 5, cus) == [2, 2, 2, 2, 1]
    assert fc.fold_plan(5, 10, cus) == [1] * 5 and fc.fold_plan(12, 3, cus) == [4, 4, 4]
    # the rows of host_fold.h and the refusals just past them
    assert fc.fold_rows(4 * 2560) == (2560, 2560, 5) and fc.fold_rows(4 * 2561)[2] == 6
    for obs, cells in fc.REFUSALS:
        N = obs[0] * obs[1]
        assert fc.fold_rows(N)[2] == 6 and not fc.fold_taken(N, False)
        assert obs[0] % 2 == 0 and obs[1] % 2 == 0
    # (100 x 100 is the largest square grid of five rows, nF = 2560 = 80 x 128 / 4 the largest of any; 84 x 122 lies
    # two rows past it, in the same ldF = 2576 as the first row past it)
    assert fc.fold_rows(100 * 100)[2] == 5 and fc.fold_rows(4 * 2561)[1] == 2576
    assert fc.fold_rows(102 * 102) == (2601, 2608, 6) and fc.fold_rows(84 * 122) == (2562, 2576, 6)
    assert fc.fold_taken(100 * 100, True) and not fc.fold_taken(102 * 102, True)
