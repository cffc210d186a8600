"""CPU suite: the oracle's counts form of the bootstrap recurrence (oracle.cg_port.bootstrap_counts) against the
reference's own run, and the cases of tests/test_gpu_bscg_oracle.py without a device -- for every case, on the oracle
alone: conditioning (float64 and longdouble runs agree to TOL_BSCG / 10), branch margins (every alpha-rule margin
|.| >= 1e-6, every data value the stop test saw outside [0.05, 0.2]), sharpness (one entry of the weighted matrix
scaled by 1 + delta moves the results by more than 100 TOL_BSCG), the branch case's branches from the oracle's trace,
the table's coverage and the restated launch arithmetic of bscg_run at 64, 256 and 304 CUs."""
import numpy as np
import pytest

import bscg_oracle_cases as bc
from conftest import gold
from helpers import relmax

CUS = (64, 256, 304)
SIZED_BY_CUS = [s.id for s in bc.TABLE if isinstance(s.M, str)]
# every case at the smallest CU count, the cases whose M comes from the CU count at the other two as well
HOST_CASES = [(s.id, 64) for s in bc.TABLE + [bc.BRANCH]] + [(cid, cus) for cid in SIZED_BY_CUS for cus in CUS[1:]]


def test_counts_form_is_the_resampled_form_and_the_reference_run():
    """cg_small.npz with counts = bincount of the seeded draw and q = 0.9: cg_port.bootstrap and bs_small.npz (the
    reference's own BSCG) to the 1e-9 test_oracle_golden.py holds bootstrap to."""
    from oracle import cg_port, oracle
    g, b = gold("cg_small.npz"), gold("bs_small.npz")
    M = int(np.prod(g["shape"]))
    Aw, wm = oracle.col_weight(g["K"])
    N = Aw.shape[0]
    counts = np.zeros((3, N))
    for s in range(3):
        np.random.seed(s)
        counts[s] = np.bincount(np.random.choice(np.arange(N), size=N, replace=True, p=None), minlength=N)
    got = cg_port.bootstrap_counts(Aw, wm, counts, g["dobs"], wm * 0.001, (0.0, 1.0), 0.1 ** 2, 0.9, 5)
    port = cg_port.bootstrap(g["K"], g["dobs"], (0.0, 1.0), np.full(M, 0.001), samples=3, beta=0.1, maxk=5)
    assert list(got.n_entries) == [4, 4, 4] and list(got.n_alpha) == [5, 5, 5]
    for name, v, p in zip(bc.NAMES, got.results(), port):
        assert v.dtype == np.float64 and v.shape == b[name].shape
        assert relmax(v, p) < 1e-9, name
        assert relmax(v, b[name]) < 1e-9, name
    for tr in got.trace:
        assert sorted(tr["margin"]) == [2, 3, 4] and len(tr["seen"]) == 4 and len(tr["clamped"]) == 5
    # every operation in the type asked for
    ld = cg_port.bootstrap_counts(Aw, wm, counts[:1], g["dobs"], wm * 0.001, (0.0, 1.0), 0.1 ** 2, 0.9, 3,
                                  dtype=np.longdouble)
    assert all(v.dtype == np.longdouble for v in ld.results())
    # q is an argument: another q gives another alpha where the rule fires, and only there
    other = cg_port.bootstrap_counts(Aw, wm, counts, g["dobs"], wm * 0.001, (0.0, 1.0), 0.1 ** 2, 0.5, 5)
    fired = [[k for k, m in sorted(tr["margin"].items()) if m < 0] for tr in got.trace]
    for s in range(3):
        first = fired[s][0] if fired[s] else 5
        assert np.array_equal(other.alpha[s, :first], got.alpha[s, :first])
        if fired[s]:
            assert other.alpha[s, first] == 0.5 * got.alpha[s, first - 1]
            assert got.alpha[s, first] == 0.9 * got.alpha[s, first - 1]


@pytest.mark.parametrize("cid,cus", HOST_CASES)
def test_case_is_well_conditioned_off_its_branch_edges_and_sharp(cid, cus):
    d = bc.make(cid, cus)
    spec, ref = d.spec, d.ref
    # the generator: counts with rows dropped and rows drawn three times or more, the probed rows in every replicate
    ordinary = d.counts[1:] if cid == bc.BRANCH.id else d.counts
    assert (ordinary >= 0).all() and np.array_equal(ordinary, np.round(ordinary))
    if d.N >= 49:
        assert (ordinary == 0).mean() > 0.25 and (ordinary >= 3).any()
    probes = d.probes()
    assert probes[0] == (d.N - 1, d.M - 1)
    assert probes[1][0] % 16 == 0 and probes[1][0] < d.N <= probes[1][0] + 16
    assert probes[1][1] % 16 == 0 and probes[1][1] < d.M <= probes[1][1] + 16
    for row, _ in probes:
        assert (ordinary[:, row] >= 1).all()
    # conditioning: how far rounding alone moves the recurrence on this input
    ld = d.run(d.Aw, d.counts, dtype=np.longdouble)
    assert np.array_equal(ld.n_entries, ref.n_entries) and np.array_equal(ld.n_alpha, ref.n_alpha)
    spread = max(relmax(v, np.asarray(w, dtype=np.float64)) for v, w in zip(ref.results(), ld.results()))
    # branch margins
    margins = [abs(m) for tr in ref.trace for m in tr["margin"].values()]
    stopped = [b for b in range(d.B) if ref.n_alpha[b] < d.maxk or ref.n_entries[b] < d.maxk - 1]
    for b, tr in enumerate(ref.trace):
        assert len(tr["seen"]) == ref.n_alpha[b] - 1
        for k, v in enumerate(tr["seen"]):
            if b in stopped and k == len(tr["seen"]) - 1:
                assert v < 0.05, (cid, b, v)
            else:
                assert v > 0.2, (cid, b, v)
    assert bool(stopped) == spec.stops, (cid, stopped)
    # sharpness
    assert spec.delta <= 1e-3
    moved = [bc.distance(ref, d.perturbed(entry, spec.delta)) for entry in probes]
    print("%s at %d CUs (%d x %d, B = %d, maxk = %d, q = %g): float64 / longdouble spread %.2e, smallest alpha-rule "
          "margin %.2e, Aw%r and Aw%r (1 + %.0e) move the oracle by %.2e and %.2e"
          % (cid, cus, d.N, d.M, d.B, d.maxk, d.q, spread, min(margins) if margins else np.inf, probes[0], probes[1],
             spec.delta, moved[0], moved[1]))
    assert spread <= bc.TOL_BSCG / 10, (cid, spread)
    assert all(m >= 1e-6 for m in margins), (cid, min(margins))
    assert min(moved) > 100 * bc.TOL_BSCG, (cid, moved)
    # a probed cell that ends on a bound in every replicate cannot show its column
    for _, col in probes:
        assert ((ref.models[:, col] > d.low) & (ref.models[:, col] < d.high)).any(), (cid, col)


def test_branch_case_takes_every_branch():
    """From the oracle's trace, before a device is touched."""
    d = bc.make(bc.BRANCH.id, 64)
    ref, maxk = d.ref, d.maxk
    assert (d.B, maxk, d.q, (d.N, d.M)) == (16, 6, 0.5, (49, 47)) and (d.low, d.high) == (0.2, 0.8)
    took = dict((k, [b for b, tr in enumerate(ref.trace) if tr["margin"].get(k, 1.0) < 0]) for k in range(2, maxk))
    kept = dict((k, [b for b, tr in enumerate(ref.trace) if tr["margin"].get(k, -1.0) > 0]) for k in range(2, maxk))
    assert any(took[k] and kept[k] for k in range(2, maxk)), (took, kept)
    for b in sum(took.values(), []):     # ... and alpha shows it
        k = min(k for k in took if b in took[k])
        assert ref.alpha[b, k] == d.q * ref.alpha[b, k - 1]
    # slot 0 freezes at k = 1 -- no misfit entry, two regularisation factors -- and every other slot runs to the end
    assert (ref.n_entries[0], ref.n_alpha[0]) == (0, 2) and ref.trace[0]["seen"][0] < 0.05
    assert (ref.n_entries[1:] == maxk - 1).all() and (ref.n_alpha[1:] == maxk).all()
    # both clamps act, and cells end on both bounds
    assert sum(n for tr in ref.trace for n, _ in tr["clamped"]) > 0 and sum(n for tr in ref.trace for _, n in tr["clamped"]) > 0
    assert (ref.models == d.low).any() and (ref.models == d.high).any()
    # the group of 3 of the slot checks: a freeze at k = 3, one at k = 1, a full run
    three = d.run(d.Aw, d.group_of_three())
    assert list(three.n_entries) == [2, 0, maxk - 1] and list(three.n_alpha) == [4, 2, maxk]
    seen = three.trace[0]["seen"]
    assert seen[0] > 0.2 and seen[1] > 0.2 and seen[2] < 0.05
    # maxk = 2 on the same inputs: the lengths the reused result block is read with
    two = d.run(d.Aw, d.counts, maxk=2)
    assert list(two.n_entries) == [0] + [1] * 15 and (two.n_alpha == 2).all()


def test_case_table_covers_what_it_is_meant_to():
    ids = lambda group: [s for s in bc.TABLE if s.group == group]
    assert [s.N for s in ids("patches")] == [1, 15, 16, 17, 32, 33, 49, 97] and all(s.M == 33 for s in ids("patches"))
    assert [bc.roundup16(s.N) // 16 for s in ids("patches")] == [1, 1, 1, 2, 2, 3, 4, 7]
    assert [s.M for s in ids("tiles")] == [1, 15, 16, 17, 32, 33, 47, 48] and all(s.N == 49 for s in ids("tiles"))
    assert [s.N for s in ids("rowblocks")] == [511, 513, 1023, 1024, 1025, 2049]
    assert all(75 <= s.M <= 126 for s in ids("rowblocks"))
    assert [s.M for s in ids("stride")] == [16384, 16385, 16400, 32790] and all(s.N == 20 for s in ids("stride"))
    assert [(s.N, s.M) for s in ids("colblocks")] == [(5003, "colblocks"), (20, "pairs")]
    assert sorted((s.N, s.M) for s in bc.TABLE if s.colmajor) == [(49, 17), (49, 47), (513, 110)]
    assert [s.N for s in ids("teams")] == [3585, 14336] and all(abs(s.M - 200) <= 5 and s.team for s in ids("teams"))
    for group in ("patches", "tiles", "rowblocks", "stride"):
        assert set(s.B for s in ids(group)) == {1, 5, 15, 16}, group
        assert set(s.maxk for s in ids(group)) == {2, 3, 5} and set(s.q for s in ids(group)) == {0.9, 0.5}, group
    assert set(s.delta for s in bc.TABLE) == {bc.DELTA} and bc.TOL_BSCG == 1e-10
    assert len(bc.BY_ID) == len(bc.TABLE) == 30


@pytest.mark.parametrize("cus", CUS)
def test_restated_launch_arithmetic_at_three_cu_counts(cus):
    P = lambda cid: bc.plan(bc.BY_ID[cid].N, bc.BY_ID[cid].size(cus), cus, bc.BY_ID[cid].team)
    # the ring of three: np = 1, 2 (fewer patches than the ring), 3, 4, 7 (np mod 3 = 0, 1, 1)
    assert [P(s.id)["np"] for s in bc.TABLE if s.group == "patches"] == [1, 1, 1, 2, 2, 3, 4, 7]
    # tiles: a single tile, pairs without their second tile (ntiles odd), M a multiple of 16
    assert [P(s.id)["ntiles"] for s in bc.TABLE if s.group == "tiles"] == [1, 1, 1, 2, 2, 3, 3, 3]
    assert all(P(s.id)["npairs"] <= P(s.id)["n_waves"] == 4 for s in bc.TABLE if s.group in ("patches", "tiles"))
    # the 1024-thread loops: a second and third pass over N (bscg_kstep_kernel) and ld (bscg_residual_kernel)
    rows = dict((s.N, P(s.id)) for s in bc.TABLE if s.group == "rowblocks")
    assert [(N, p["ld"], p["n_passes"], p["ld_passes"], p["rowblocks"]) for N, p in sorted(rows.items())] == \
        [(511, 512, 1, 1, 1), (513, 528, 1, 1, 2), (1023, 1024, 1, 1, 2), (1024, 1024, 1, 1, 2), (1025, 1040, 2, 2, 3),
         (2049, 2064, 3, 3, 5)]
    # grid-stride of direction / step: nblk = 1024 exactly; one cell, one tile past it; the start of a third pass
    strides = [P(s.id) for s in bc.TABLE if s.group == "stride"]
    assert [(p["ntiles"], p["nblk"], p["cell_passes"]) for p in strides] == \
        [(1024, 1024, 1), (1025, 1024, 2), (1025, 1024, 2), (2050, 1024, 3)]
    assert all(P(s.id)["nblk"] == P(s.id)["ntiles"] < 1024 for s in bc.TABLE if s.group not in ("stride", "colblocks"))
    p = P("b-n5003")
    assert p["rowblocks"] == 10 and p["cols_per_block"] == 32 and p["last_block"] == 7 and p["n_colblocks"] > 1
    p = P("w-n20")
    assert p["n_waves"] == 16 * cus and p["npairs"] == p["n_waves"] + 2 and p["cell_passes"] >= 3
    # bteam_plan on: the adjoint's grid and the rows bscg_mu_kernel sums come from members x ranges
    for cid, members in (("t-n3585", 9), ("t-n14336", 32)):
        p = P(cid)
        assert p["members"] == members and p["adjoint_waves"] >= p["members"] * p["ranges"] > p["n_waves"] >= p["npairs"]
        assert p["adjoint_waves"] % 4 == 0
    assert all(P(s.id)["members"] == 0 for s in bc.TABLE if not s.team)
