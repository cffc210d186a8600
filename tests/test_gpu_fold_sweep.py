"""GPU suite (`-m gpu`): every mode of the folded sweep (csrc/fold.hip.h) against the dense sweep.

Small mirror-symmetric prism problems with the fold forced (GRAVHMC_FOLD_MIN_MB=0; GRAVHMC_RESIDENT=0 so that the
chain runs on the sweep path) against the same problem with GRAVHMC_FOLD=0, through the Engine calls that issue
the modes: misfit_and_grad (SW_FWD, then SW_ADJ | SW_GOUT), chain_trajectory and leapfrog (SW_FWD, the fused
SW_ADJ | SW_UPD | SW_FWD, the final SW_ADJ | SW_PFIN), run_chain with overlap (the final half step fused with the
next trajectory's first step: SW_SPEC).  Observation grids of 24 .. 100 points a side give every instantiation
EPT2 = 1 .. 5 (ldF = roundup(n^2 / 4, 16) folded rows, ceil(2 ldF / 1024) double2 per thread); 125 orbits leave
workgroups of one orbit each, 605 and 1183 leave the last workgroup short at 256 or 512 workgroups."""
import numpy as np
import pytest

from helpers import relmax

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def _problem(G, n_obs, cells):
    mesh = G.mesher.PrismMesh((0, 2000.0, 0, 2000.0, 0, 1000.0),
                              (1000.0 / cells[2], 2000.0 / cells[1], 2000.0 / cells[0]))
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 2000.0, n_obs), np.linspace(0, 2000.0, n_obs))]
    obs = np.stack([xp, yp, np.zeros_like(xp)])
    return mesh, obs, np.ascontiguousarray(mesh.cell_bounds())


def _engine(G, mesh, obs, b6, seed):
    eng = G.Engine(obs.shape[1], b6.shape[0])
    eng.set_obs(*[np.ascontiguousarray(v) for v in obs])
    eng.set_cells(b6, 0)
    eng.build_G()
    wm = eng.weight(0.5)
    rng = np.random.default_rng(seed)
    M = b6.shape[0]
    rho = np.zeros(M)
    rho[rng.choice(M, M // 10, replace=False)] = 1.0
    d = eng.forward(wm * rho)
    eng.set_data(d + 0.01 * np.abs(d).max() * rng.normal(size=d.size))
    eng.set_reg("Damping", 1.0, 0.01, mesh.shape, 0.001 * wm)
    return eng, wm


def _run(eng, wm, trajs, dt):
    """Every mode once: misfit and gradient, chain trajectories, the piped chain, stateless leapfrog."""
    xt = 0.02 * wm * np.linspace(0.1, 1.0, wm.size)
    mg = eng.misfit_and_grad(xt)
    low, high = 0.0 * wm, 0.05 * wm
    eng.chain_init(0.001 * wm, low, high)
    chain = []
    for L, p0, u in trajs:
        acc, o = eng.chain_trajectory(p0, dt, L, u)
        chain.append((bool(acc), o.copy(), eng.chain_get_x()))
    eng.chain_init(0.001 * wm, low, high)
    piped = []
    eng.run_chain(iter([(L, p0, u) for L, p0, u in trajs]), dt,
                  lambda L, a_, o_, x_: piped.append((bool(a_), o_.copy(), None if x_ is None else x_.copy())),
                  want_x=True, batch=4, overlap=True)
    x, lf = 0.001 * wm, []
    for L, p0, u in trajs:
        x, acc, o, _ = eng.leapfrog(x, p0, dt, L, low, high, u)
        lf.append((bool(acc), o.copy(), x.copy()))
    return mg, chain, piped, lf


@pytest.mark.parametrize("n_obs,cells", [
    (24, (10, 10, 5)),     # EPT2 1, 125 orbits: one per workgroup
    (48, (22, 22, 5)),     # EPT2 2, 605 orbits
    (70, (10, 10, 5)),     # EPT2 3
    (84, (26, 26, 7)),     # EPT2 4, 1183 orbits
    (100, (26, 26, 7)),    # EPT2 5 (C2's ldF = 2512), the largest the fold takes
])
def test_fold_sweep_modes_against_dense(G, monkeypatch, n_obs, cells):
    monkeypatch.setenv("GRAVHMC_FOLD_MIN_MB", "0")
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    mesh, obs, b6 = _problem(G, n_obs, cells)
    N, M = obs.shape[1], b6.shape[0]
    rng = np.random.default_rng(11)
    dt = 0.002
    trajs = [(int(rng.integers(2, 6)), rng.normal(size=M) * 0.01, float(rng.uniform())) for _ in range(5)]

    fold, wm = _engine(G, mesh, obs, b6, 5)
    res_f = _run(fold, wm, trajs, dt)
    info = fold.fold_info()
    assert info["on"], info
    assert info["store_bytes"] == (M // 4) * 4 * ((N // 4 + 15) // 16 * 16) * 8
    # the same trajectories again on the same engine: the same bits
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
            assert a1 == a2
            assert relmax(o1, o2) <= 1e-10
            if x1 is not None and x2 is not None:
                assert relmax(x1, x2) <= 1e-10

    mg_a, ch_a, pi_a, lf_a = again
    assert all(np.array_equal(u, v) for u, v in zip(mg_f, mg_a))
    for run_f, run_a in ((ch_f, ch_a), (pi_f, pi_a), (lf_f, lf_a)):
        for (a1, o1, x1), (a2, o2, x2) in zip(run_f, run_a):
            assert a1 == a2 and np.array_equal(o1, o2)
            assert (x1 is None and x2 is None) or np.array_equal(x1, x2)


def test_fold_refuses_panels_past_its_registers(G, monkeypatch):
    """104 x 104 observations: ldF = 2704 needs EPT2 = 6, more than the kernel holds without spilling: the dense
    sweep, reason "path"."""
    monkeypatch.setenv("GRAVHMC_FOLD_MIN_MB", "0")
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    mesh, obs, b6 = _problem(G, 104, (10, 10, 5))
    eng, wm = _engine(G, mesh, obs, b6, 5)
    eng.misfit_and_grad(0.01 * wm)
    info = eng.fold_info()
    assert not info["on"] and info["reason"] == "path", info
    eng.close()
