"""GPU suite (`-m gpu`): the paired sweep with its rows folded over tau and two blocks in flight ahead
(fold_pair_sweep_kernel, fold_pair_rows_kernel, csrc/fold.hip.h; the row order of tests/test_fold_rows_host.py).

Observation grids n x n, n = 2, 4, 6, 44, 62, 64, 88, 90, 92, 100 (nF = 1; one pair of rows and two diagonal rows;
496 / 528 pairs around one pair slot per thread, 990 / 1035 around two, the benchmark's 201 split pairs), over cells
(4, 4, 3) (9 work items) and (6, 6, 2); at n = 64 and 100 cells (8, 8, 2) (20 work items) under GRAVHMC_MIN_COLS for
1, 2, 3, 4 and 7 items per workgroup: the prologue alone, one turn of the three-buffer loop, a turn and one or two
items behind it, two turns.  Inputs and oracle trajectories from fold_oracle_cases' generator (accepted, rejected
and clamped by construction), the fold forced (GRAVHMC_FOLD_MIN_MB=0, GRAVHMC_RESIDENT=0).

Per case: the chain against oracle.Problem at TOL_TRAJ with equal decisions, run_chain / leapfrog / a second engine
bit for bit, misfit_and_grad at TOL_TRAJ; every sweep mode against the dense sweep at 1e-10 (the bound of
test_paired_sweep_modes_against_dense); GRAVHMC_FOLD_PAIR=0 on the same engine: the unpaired kernel on a store of
the same size, the bits of an engine that never paired."""
import functools

import numpy as np
import pytest

import fold_oracle_cases as fc
from helpers import relmax
from test_gpu_fold_oracle import _engine as _oracle_engine
from test_gpu_fold_sweep import _engine, _problem, _run

pytestmark = pytest.mark.gpu

TOL_TRAJ = fc.TOL_TRAJ
SIDES = (2, 4, 6, 44, 62, 64, 88, 90, 92, 100)
REGS = ("Damping", "MS", "Smoothness", "TV")

SPECS = [fc.Spec("R-%d" % n, "rows", (n, n), (4, 4, 3), REGS[k % 4], 2, paired=True) for k, n in enumerate(SIDES)]
SPECS.append(fc.Spec("R-6-cells6", "rows", (6, 6), (6, 6, 2), "MS", 2, paired=True,
                     note="a cell grid that is not the observations'"))
# 20 work items (12 pairs, 8 single orbits) in runs of 1, 2, 3, 4 and 7
for n in (64, 100):
    for mc, runs in ((2, [1] * 20), (13, [2] * 10), (19, [3] * 6 + [2]), (26, [4] * 5), (43, [7, 7, 6])):
        SPECS.append(fc.Spec("R-%d-run%d" % (n, runs[0]), "runs", (n, n), (8, 8, 2), REGS[mc % 4], mc, paired=True,
                             runs=runs))
SPECS.append(fc.Spec("R-90-topo", "topography", (90, 90), (4, 4, 2), "Damping", 2, paired=True, topo=True,
                     layers=(0.3, 0.7)))
SPECS.append(fc.Spec("R-100-shuffled", "shuffled", (100, 100), (4, 4, 3), "TV", 16, paired=True, shuffle=True,
                     runs=[3, 3, 3]))
BY_ID = dict((s.id, s) for s in SPECS)


@functools.lru_cache(maxsize=2)
def _data(cid):
    from oracle import oracle
    return fc.Data(oracle, BY_ID[cid])


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def _setup(G, monkeypatch, d, env):
    eng = _oracle_engine(G, monkeypatch, d.obs, d.b6, env)
    wm = eng.weight(0.5)
    eng.set_data(d.dobs)
    eng.set_reg(d.reg, d.alpha, d.beta, d.shape, d.mwapr)
    return eng, wm


def _chain(eng, d):
    eng.chain_init(d.x0, d.low, d.high)
    out = []
    for L, p0, u in d.trajs:
        acc, o = eng.chain_trajectory(p0, d.dt, L, u)
        out.append((bool(acc), o.copy(), eng.chain_get_x()))
    return out


@pytest.mark.parametrize("cid", [s.id for s in SPECS])
def test_rows_chain_against_oracle(G, monkeypatch, cid):
    d = _data(cid)
    s, ref = d.spec, d.ref
    lo, hi = d.clamped()
    assert ref.acc.sum() >= 2 and (~ref.acc).sum() >= 2 and lo > 0 and hi > 0
    eng, wm = _setup(G, monkeypatch, d, s.env())
    assert relmax(wm, d.wm) <= 1e-11
    plain, worst = _chain(eng, d), 0.0
    for t, (acc, o, x) in enumerate(plain):
        e_o, e_x = relmax(o, ref.out5[t]), relmax(x, ref.xs[t])
        print("%s: trajectory %d (%s): out5 %.2e, x %.2e" % (cid, t, "accepted" if ref.acc[t] else "rejected", e_o, e_x))
        worst = max(worst, e_o, e_x)
        assert acc == bool(ref.acc[t]), (cid, t)
        assert e_o <= TOL_TRAJ and e_x <= TOL_TRAJ, (cid, t, e_o, e_x)

    info = eng.fold_info()
    assert info["on"] and info["pair_on"] and info["pair_reason"] == "on", info
    assert info["store_bytes"] == (s.M // 4) * 4 * s.ldF * 8
    assert info["bytes_per_sweep"] == s.items() * 4 * s.ldF * 8
    assert (info["pairs"], info["single_orbits"]) == s.counts()
    assert info["max_dev"] <= 1e-7
    lay, cus = eng.sweep_layout(), eng.device_info()["cus"]
    runs = fc.fold_plan(s.items(), lay["grid"], cus)
    if s.runs is not None:
        assert runs == s.runs, (cid, runs, lay)

    eng.chain_init(d.x0, d.low, d.high)
    piped, last = [], d.x0
    eng.run_chain(iter(d.trajs), d.dt, lambda L, a_, o_, x_: piped.append((bool(a_), o_.copy(), x_)), want_x=True,
                  batch=4, overlap=True)
    assert len(piped) == len(plain)
    for t, ((a1, o1, x1), (a2, o2, x2)) in enumerate(zip(plain, piped)):
        last = x2 if x2 is not None else last
        assert a1 == a2 and np.array_equal(o1, o2) and np.array_equal(x1, last), (cid, "run_chain", t)
    x = d.x0
    for t, ((L, p0, u), (acc, o, xs)) in enumerate(zip(d.trajs, plain)):
        x, acc2, o2, _ = eng.leapfrog(x, p0, d.dt, L, d.low, d.high, u)
        assert bool(acc2) == acc and np.array_equal(x, xs) and np.array_equal(o2, o), (cid, "leapfrog", t)
    out = eng.misfit_and_grad(d.xt)
    e_m = fc.mg_distance(out, ref.mg)
    worst = max(worst, e_m)
    assert e_m <= TOL_TRAJ, (cid, "misfit_and_grad", e_m)
    eng.close()

    # a second engine: the same bits
    eng2, wm2 = _setup(G, monkeypatch, d, s.env())
    assert np.array_equal(wm2, wm)
    for t, ((a1, o1, x1), (a2, o2, x2)) in enumerate(zip(plain, _chain(eng2, d))):
        assert a1 == a2 and np.array_equal(o1, o2) and np.array_equal(x1, x2), (cid, "second engine", t)
    out2 = eng2.misfit_and_grad(d.xt)
    assert all(np.array_equal(u, v) for u, v in zip(out, out2))
    eng2.close()
    print("%s: nF = %d, %d rows per thread, %d items in runs of %s: worst relmax against the oracle %.2e"
          % (cid, s.nF, s.rows, s.items(), runs, worst))


@pytest.mark.parametrize("n_obs,cells", [(n, (4, 4, 3)) for n in SIDES] + [(6, (6, 6, 2))])
def test_rows_sweep_modes_against_dense(G, monkeypatch, n_obs, cells):
    """misfit_and_grad (forward only, then the adjoint), chain trajectories (fused steps, the final half step), the
    piped chain (the final half step with the next trajectory's speculative step) and stateless leapfrog."""
    monkeypatch.setenv("GRAVHMC_FOLD_MIN_MB", "0")
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    mesh, obs, b6 = _problem(G, n_obs, cells)
    M = b6.shape[0]
    rng = np.random.default_rng(11)
    dt = 0.002
    trajs = [(int(rng.integers(2, 6)), rng.normal(size=M) * 0.01, float(rng.uniform())) for _ in range(5)]
    fold, wm = _engine(G, mesh, obs, b6, 5)
    res_f = _run(fold, wm, trajs, dt)
    info = fold.fold_info()
    assert info["on"] and info["pair_on"] and info["pair_reason"] == "on", info
    again = _run(fold, wm, trajs, dt)
    fold.close()
    monkeypatch.setenv("GRAVHMC_FOLD", "0")
    dense, wm_d = _engine(G, mesh, obs, b6, 5)
    assert np.array_equal(wm_d, wm)
    res_d = _run(dense, wm_d, trajs, dt)
    assert not dense.fold_info()["on"]
    dense.close()

    (mg_f, ch_f, pi_f, lf_f), (mg_d, ch_d, pi_d, lf_d) = res_f, res_d
    assert abs(mg_f[0] - mg_d[0]) <= 1e-10 * abs(mg_d[0])
    assert relmax(mg_f[1], mg_d[1]) <= 1e-10 and relmax(mg_f[2], mg_d[2]) <= 1e-10
    assert len(pi_f) == len(pi_d) == len(trajs)
    for run_f, run_d in ((ch_f, ch_d), (pi_f, pi_d), (lf_f, lf_d)):
        for (a1, o1, x1), (a2, o2, x2) in zip(run_f, run_d):
            assert a1 == a2 and relmax(o1, o2) <= 1e-10
            if x1 is not None and x2 is not None:
                assert relmax(x1, x2) <= 1e-10
    mg_a, ch_a, pi_a, lf_a = again
    assert all(np.array_equal(u, v) for u, v in zip(mg_f, mg_a))
    for run_f, run_a in ((ch_f, ch_a), (pi_f, pi_a), (lf_f, lf_a)):
        for (a1, o1, x1), (a2, o2, x2) in zip(run_f, run_a):
            assert a1 == a2 and np.array_equal(o1, o2)
            assert (x1 is None and x2 is None) or np.array_equal(x1, x2)


@pytest.mark.parametrize("cid", ["R-64", "R-100"])
def test_pairing_switched_off_on_the_same_engine(G, monkeypatch, cid):
    """A store rebuilt under GRAVHMC_FOLD_PAIR=0 after the paired sweep reordered it: four-image means in the mirror
    table's order, the unpaired kernel, the bits of an engine that never paired."""
    d = _data(cid)
    s = d.spec
    eng, _ = _setup(G, monkeypatch, d, s.env())
    paired = _chain(eng, d)
    on = eng.fold_info()
    assert on["pair_on"]
    monkeypatch.setenv("GRAVHMC_FOLD_PAIR", "0")
    eng.build_G()
    eng.weight(0.5)
    same = _chain(eng, d)
    info = eng.fold_info()
    assert info["on"] and not info["pair_on"] and info["pair_reason"] == "switched off", info
    assert info["store_bytes"] == on["store_bytes"] == info["bytes_per_sweep"]
    eng.close()
    off, _ = _setup(G, monkeypatch, d, dict(s.env(), GRAVHMC_FOLD_PAIR=0))
    fresh = _chain(off, d)
    assert not off.fold_info()["pair_on"]
    off.close()
    for t, ((a1, o1, x1), (a2, o2, x2), (a3, o3, x3)) in enumerate(zip(same, fresh, paired)):
        assert a1 == a2 and np.array_equal(o1, o2) and np.array_equal(x1, x2), (cid, t)
        assert a1 == a3 == bool(d.ref.acc[t])
        assert relmax(o1, d.ref.out5[t]) <= TOL_TRAJ and relmax(x1, d.ref.xs[t]) <= TOL_TRAJ
