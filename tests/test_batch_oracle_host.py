"""CPU suite: the cases of tests/test_gpu_batch_oracle.py without a device -- the generator's own conditions on the
oracle alone, how sharp every case is (one entry of A scaled by 1 + delta must move the oracle's results by more
than 100 TOL_TRAJ), the case table's coverage, and the restated partitions of batch_alloc / bteam_plan
(csrc/host_batch.h) at 64, 256 and 304 CUs against values read off that code."""
import numpy as np
import pytest

import batch_oracle_cases as bc

HOST_CUS = 64      # the CU count the host test sizes the run-time cases with (the smallest of the three)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.mark.parametrize("cid", [s.id for s in bc.CASES])
def test_case_meets_the_generators_conditions_and_is_sharp(orc, cid):
    spec = bc.BY_ID[cid]
    d = bc.make(cid, HOST_CUS)      # (asserts: both decisions, a mixed round, idle slots, cells clamped at both bounds)
    ref = d.ref
    assert ref.acc.any() and not ref.acc.all()
    assert d.clamped[0] > 0 and d.clamped[1] > 0
    assert (d.Ls >= 1).all() and (d.Ls <= 6).all()
    assert (d.x0s >= d.low).all() and (d.x0s <= d.high).all()
    np.testing.assert_allclose(d.high - d.low, 3.0 * d.dt, rtol=1e-12)
    # a rejection only where the oracle's H rose by > 0.01; u half-way between the edge and 0 or 1
    dH = ref.out5[:, :, 4] - ref.out5[:, :, 3]
    assert (dH[~ref.acc] > 0.01).all()
    edge = np.exp(-np.maximum(dH, 0.0))
    assert np.allclose(d.us[ref.acc], 0.5 * edge[ref.acc]) and np.allclose(d.us[~ref.acc], 0.5 * (1 + edge[~ref.acc]))
    # the data: a mean 10^3 times their spread
    assert abs(d.dobs.mean()) > 100 * max(d.dobs.std(), 1e-300) or d.N == 1
    # replaying the lists gives the reference back, bit for bit (the oracle is deterministic)
    assert bc.distance(d, ref, bc.replay(d.P, d)) == 0.0
    # sensitivity
    assert spec.delta is not None and spec.delta <= 1e-3
    probes = d.probes()
    assert probes[0] == (d.N - 1, d.M - 1)
    assert probes[1][0] % 16 == 0 and probes[1][0] < d.N <= probes[1][0] + 16
    assert probes[1][1] % 16 == 0 and probes[1][1] < d.M <= probes[1][1] + 16
    for entry in probes:
        moved = bc.distance(d, ref, d.perturbed(orc, entry, spec.delta))
        print("%s: A%r (1 + %.0e) moves the oracle by %.2e" % (cid, entry, spec.delta, moved))
        assert moved > 100 * bc.TOL_TRAJ, (cid, entry, moved)


def test_case_table_covers_what_it_is_meant_to():
    for cases in (bc.TWO_PASS, bc.TEAMS):
        assert set(s.reg for s in cases) == {"Damping", "MS", "Smoothness", "TV"}
        assert abs(2 * sum(s.fix for s in cases) - len(cases)) <= 1
        # Smoothness and TV on true 3-D shapes with M no multiple of 16: a 16-cell block of batch_reg_kernel
        # straddles rows and planes
        for reg in ("Smoothness", "TV"):
            assert any(s.reg == reg and s.size(cus)[0] % 16 != 0 and min(s.size(cus)[1]) > 1
                       for s in cases for cus in (64, 256, 304)), reg
    assert set(s.C for s in bc.TWO_PASS) == {1, 5, 16} and set(s.C for s in bc.TEAMS) == {5, 16}
    shapes = [s.size(256)[1] for s in bc.CASES]
    assert any(1 in sh and sum(n > 1 for n in sh) == 2 for sh in shapes) and any(2 in sh for sh in shapes)
    assert any(all(n > 1 for n in sh) for sh in shapes)
    ids = lambda group: [s for s in bc.TWO_PASS if s.group == group]
    assert [s.N for s in ids("patches")] == [1, 16, 17, 33, 49, 97] and all(s.M == 33 for s in ids("patches"))
    assert sorted(set(bc.roundup16(s.N) // 16 for s in ids("patches"))) == [1, 2, 3, 4, 7]
    assert [s.N for s in ids("rowblocks")] == [130, 496, 511, 513, 1025]
    assert [s.M for s in ids("tiles")] == [1, 15, 16, 17, 32, 33, 47, 48] and all(s.N == 49 for s in ids("tiles"))
    assert sorted(s.id for s in bc.CASES if s.colmajor) == ["c-m17", "c-m47", "r-n513"]
    assert len(bc.BY_ID) == len(bc.CASES)


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_restated_plans_at_three_cu_counts(cus):
    # bteam_plan: members = ceil(ceil(ld / 64) / 7) in 8 .. 32, nval = ceil(256 / members)
    for N, members, nval in ((3136, 0, 0), (3137, 8, 32), (3585, 9, 29), (14321, 32, 8), (14336, 32, 8), (14337, 0, 0)):
        p = bc.team_plan(N, 300, cus)
        assert (p["members"], p["nval"]) == (members, nval), (N, p)
        if members:
            assert p["ranges"] == min(19, cus // members) or p["tpr"] > 1
            assert p["members"] * p["ranges"] <= cus and (p["ranges"] - 1) * p["tpr"] < 19 <= p["ranges"] * p["tpr"]
    assert bc.team_plan(3136, 300, cus)["row_chunks"] == 7 and bc.team_plan(14337, 300, cus)["row_chunks"] == 33
    # N = 3137: the last member holds one row block, 16 valid rows of it; N = 3585: nine members, 29 pairs each --
    # the last one owns 256 - 8 * 29 = 24
    assert bc.roundup16(3137) - 7 * 448 == 16 and 256 - 8 * 29 == 24
    # tiles per range 1 .. 4, the last range one tile, the last tile partial
    for tpr in (1, 2, 3, 4):
        M = bc.team_tiles_M(3137, cus, tpr)
        p = bc.team_plan(3137, M, cus)
        assert p["tpr"] == tpr and p["ranges"] == cus // 8 and p["last_range"] == 1 and M % 16 != 0, (tpr, M, p)
    p = bc.team_plan(3585, 7, cus)
    assert (p["ranges"], p["tpr"]) == (1, 1)
    p = bc.team_plan(3585, 40, cus)
    assert (p["ranges"], p["tpr"]) == (3, 1) and p["ranges"] < cus // 9      # fewer tiles than ranges on offer
    # batch_alloc: column blocks of a multiple of 16 columns, the last one not empty
    for N, M in ((1, 33), (49, 1), (49, 48), (513, 110), (1025, 75), (5003, bc.column_block_M(5003, cus)),
                 (20, bc.more_pairs_M(cus)), (14337, 273)):
        p = bc.two_pass_plan(N, M, cus)
        assert p["cols_per_block"] % 16 == 0 and p["cols_per_block"] >= 16
        assert 0 < p["last_block"] <= p["cols_per_block"]
        assert (p["n_colblocks"] - 1) * p["cols_per_block"] + p["last_block"] == M
        assert p["n_colblocks"] <= max(1, -(-cus * 4 // p["rowblocks"]))
    p = bc.two_pass_plan(5003, bc.column_block_M(5003, cus), cus)
    assert p["rowblocks"] == 10 and p["cols_per_block"] == 32 and p["last_block"] == 7 and p["n_colblocks"] > 1
    p = bc.two_pass_plan(20, bc.more_pairs_M(cus), cus)
    assert p["n_waves"] == 16 * cus and p["npairs"] == p["n_waves"] + 2
    # the row edges: waves of 128 rows wholly past ld in the last 512-row block
    for N, idle_waves in ((130, 2), (496, 0), (511, 0), (513, 3), (1025, 3)):
        ld = bc.roundup16(N)
        assert sum(1 for w in range(4) if (bc.cdiv(ld, 512) - 1) * 512 + 128 * w >= ld) == idle_waves, N
