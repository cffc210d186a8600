"""GPU suite (`-m gpu`): the folded sweeps (fold_sweep_kernel<1 .. 5>, fold_pair_sweep_kernel<1 .. 5>, csrc/fold.hip.h,
host_fold.h) against the CPU oracle at their row and work-list edges.

The cases, their inputs and the oracle's trajectories come from tests/fold_oracle_cases.py (generated before an
engine is touched; tests/test_fold_oracle_host.py checks the generator, the conditioning and how sharp each case is).
Every case runs with the fold forced (GRAVHMC_FOLD_MIN_MB=0, GRAVHMC_RESIDENT=0) and its own GRAVHMC_MIN_COLS /
GRAVHMC_FOLD_PAIR: the weights against the oracle's at 1e-11; the chain trajectory by trajectory against
oracle.Problem.leapfrog on the oracle's own Aw -- equal decisions, out5 and chain_get_x() to TOL_TRAJ = 1e-10 in
relmax; the same trajectories through run_chain(batch=4, overlap=True) and through stateless leapfrog bit for bit;
misfit_and_grad at a random model to TOL_TRAJ; fold_info() against the case's arithmetic, and the run lengths of the
sweep's workgroups restated from sweep_layout() and the CU count.

Row edges: nF = 1, nF < 16, nF an exact multiple of 512, nF a few rows past one, nF = ldF under idle threads (the row
they re-read is real, not padding: only the last_in mask keeps it out of the sums), the full 5 x 512 rows of the
unpaired kernel, 1 .. 5 rows per thread of both kernels.  Work lists: 1, 2, 3, 4, 5, 6, 9 and all items per
workgroup, short last workgroups of either parity, lists of singles only, a single first / last / between two pairs,
shuffled cells and observations, observations that are not flat over layers of unequal thickness.  Two refusals one
step past the largest panel the fold takes."""
import numpy as np
import pytest

import fold_oracle_cases as fc
from helpers import relmax

pytestmark = pytest.mark.gpu

TOL_TRAJ = fc.TOL_TRAJ
SWITCHES = ("GRAVHMC_FOLD", "GRAVHMC_FOLD_PAIR", "GRAVHMC_MIN_COLS", "GRAVHMC_WG_PER_CU")


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def _engine(G, monkeypatch, obs, b6, env):
    """The switches are read when the engine is made (the dense layout) and at its first sweep (the fold)."""
    monkeypatch.setenv("GRAVHMC_FOLD_MIN_MB", "0")
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    eng = G.Engine(obs.shape[1], b6.shape[0])
    eng.set_obs(*[np.ascontiguousarray(v) for v in obs])
    eng.set_cells(b6, 0)
    eng.build_G()
    return eng


def _block_bytes(s):
    return 4 * s.ldF * 8


@pytest.mark.parametrize("cid", [s.id for s in fc.CASES])
def test_folded_sweep_against_oracle(G, monkeypatch, cid):
    d = fc.make(cid)                # inputs and the oracle's trajectories, before an engine is touched
    s, ref = d.spec, d.ref
    eng = _engine(G, monkeypatch, d.obs, d.b6, s.env())
    wm = eng.weight(0.5)
    assert relmax(wm, d.wm) <= 1e-11
    eng.set_data(d.dobs)
    eng.set_reg(d.reg, d.alpha, d.beta, d.shape, d.mwapr)

    # the chain, trajectory by trajectory, against the oracle
    eng.chain_init(d.x0, d.low, d.high)
    plain, worst = [], 0.0
    for t, (L, p0, u) in enumerate(d.trajs):
        acc, o = eng.chain_trajectory(p0, d.dt, L, u)
        x = eng.chain_get_x()
        plain.append((bool(acc), o.copy(), x))
        e_o, e_x = relmax(o, ref.out5[t]), relmax(x, ref.xs[t])
        print("%s: trajectory %d (L = %d, %s): out5 %.2e, x %.2e"
              % (cid, t, L, "accepted" if ref.acc[t] else "rejected", e_o, e_x))
        worst = max(worst, e_o, e_x)
        where = (cid, "trajectory %d" % t, "L %d" % L)
        assert bool(acc) == bool(ref.acc[t]), where + (o, ref.out5[t])
        assert e_o <= TOL_TRAJ, where + (e_o, o, ref.out5[t])
        assert e_x <= TOL_TRAJ, where + (e_x, int(np.abs(x - ref.xs[t]).argmax()))

    # the layout the case was written for
    info = eng.fold_info()
    assert info["on"] and info["reason"] == "on", info
    assert info["pair_on"] == s.paired and info["pair_reason"] == s.pair_reason, info
    assert info["store_bytes"] == (s.M // 4) * _block_bytes(s)
    assert info["bytes_per_sweep"] == s.items() * _block_bytes(s)
    assert (info["pairs"], info["single_orbits"]) == (s.counts() if s.paired else (0, 0)), info
    assert info["max_dev"] <= 1e-7
    assert s.rows == -(-s.ldF // 512) <= 5 and s.ldF == (s.N // 4 + 15) // 16 * 16
    lay, cus = eng.sweep_layout(), eng.device_info()["cus"]
    assert lay["n_panels"] == 1 and lay["grid"] <= cus, (lay, cus)
    assert lay["grid"] == fc.dense_layout(s.N, s.M, cus, s.min_cols)["grid"], lay
    runs = fc.fold_plan(s.items(), lay["grid"], cus)
    if s.runs is not None:
        assert runs == s.runs, (cid, runs, lay)
    assert len(runs) <= lay["n_teams"]

    # the next trajectory's first step piped into the last sweep (run_chain, overlap): the same bits
    eng.chain_init(d.x0, d.low, d.high)
    piped, last = [], d.x0
    eng.run_chain(iter(d.trajs), d.dt, lambda L, a_, o_, x_: piped.append((bool(a_), o_.copy(), x_)), want_x=True,
                  batch=4, overlap=True)
    assert len(piped) == len(plain)
    for t, ((a1, o1, x1), (a2, o2, x2)) in enumerate(zip(plain, piped)):
        last = x2 if x2 is not None else last
        assert a1 == a2 and np.array_equal(o1, o2) and np.array_equal(x1, last), (cid, "run_chain", t)
    # stateless leapfrog on the same store: the same bits
    x = d.x0
    for t, ((L, p0, u), (acc, o, xs)) in enumerate(zip(d.trajs, plain)):
        x, acc2, o2, _ = eng.leapfrog(x, p0, d.dt, L, d.low, d.high, u)
        assert bool(acc2) == acc and np.array_equal(x, xs) and np.array_equal(o2, o), (cid, "leapfrog", t)

    # misfit and gradient at a random model
    out = eng.misfit_and_grad(d.xt)
    e_m = fc.mg_distance(out, ref.mg)
    print("%s: misfit_and_grad %.2e" % (cid, e_m))
    worst = max(worst, e_m)
    assert e_m <= TOL_TRAJ, (cid, "misfit_and_grad", e_m)
    assert eng.fold_info()["on"]
    eng.close()
    print("%s (%s): %d x %d observations, nF = %d, ldF = %d, %d rows per thread, %s, %s, %d items in runs of %s: worst "
          "relmax against the oracle %.2e"
          % (cid, s.group, s.obs[0], s.obs[1], s.nF, s.ldF, s.rows, "paired" if s.paired else "unpaired", s.reg,
             s.items(), runs, worst))


@pytest.mark.parametrize("obs,cells", fc.REFUSALS)
def test_fold_refuses_six_rows_per_thread(G, monkeypatch, obs, cells):
    """102 x 102 (nF = 2601) and 84 x 122 (nF = 2562, ldF = 2576) observations: one step past the five rows a thread
    holds: the dense sweep, reason "path"."""
    o, b6 = fc.geometry(obs, cells)
    N, M = o.shape[1], b6.shape[0]
    assert fc.fold_rows(N)[2] == 6
    eng = _engine(G, monkeypatch, o, b6, {})
    wm = eng.weight(0.5)
    eng.set_data(np.zeros(N))
    eng.set_reg("Damping", 1.0, 0.01, (cells[2], cells[1], cells[0]), 0.001 * wm)
    eng.misfit_and_grad(0.01 * wm)
    info = eng.fold_info()
    assert not info["on"] and info["reason"] == "path" and not info["pair_on"], info
    eng.close()
