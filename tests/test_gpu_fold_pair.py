"""GPU suite (`-m gpu`): the folded sweep's paired form (fold_pair_sweep_kernel, csrc/fold.hip.h): one block of the
folded store per pair of cell orbits under the diagonal reflection tau.

Square problems on [0, 2000]^2 x [0, 1000] with the fold forced (GRAVHMC_FOLD_MIN_MB=0, GRAVHMC_RESIDENT=0):
trajectories with forced rejections against oracle.Problem at 1e-10 with equal decisions, chain / piped chain /
gh_leapfrog bitwise equal, the pairing against GRAVHMC_FOLD_PAIR=0 at 1e-10; every instantiation (1 .. 5 folded rows
per thread: observation grids of 24 .. 100 a side) in every mode against the dense sweep at 1e-10 and twice bitwise;
a mirror-symmetric problem that is not square (pairing off, the bits of GRAVHMC_FOLD_PAIR=0); fold_info()."""
import numpy as np
import pytest

from helpers import metropolis_u, relmax
from test_gpu_fold import _symmetric
from test_gpu_fold_sweep import _engine, _problem, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


WANT = (True, False, True, False, True, True, False, True)     # the decisions of the chain tests' trajectories


def _counts(cells):
    """pairs and single orbits of an n x n x nz column grid: the quadrant's columns off and on its diagonal"""
    q, nz = cells[0] // 2, cells[2]
    return q * (q - 1) // 2 * nz, q * nz


def _block_bytes(N):
    return 4 * ((N // 4 + 15) // 16 * 16) * 8


@pytest.mark.parametrize("reg", ["Damping", "MS", "Smoothness", "TV"])
@pytest.mark.parametrize("size", [(24, (10, 10, 5), False),    # 25 of 125 orbits self-paired, one work item per workgroup
                                  (48, (12, 12, 6), True)])    # shuffled: tau f is not the first of its orbit (c_f != 0)
def test_paired_chain_against_oracle_bitwise_paths_and_unpaired(G, orc, monkeypatch, reg, size):
    monkeypatch.setenv("GRAVHMC_FOLD_MIN_MB", "0")
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    n_obs, cells, shuffle = size
    mesh, obs, b6 = _symmetric(G, n_obs, cells, shuffle)
    N, M = obs.shape[1], b6.shape[0]
    rng = np.random.default_rng(17)
    Aw, _ = orc.col_weight(orc.prism_gz_kernel(obs[0], obs[1], obs[2], b6))
    shape = mesh.shape if not shuffle else (1, 1, M)
    rho = np.zeros(M)
    rho[rng.choice(M, M // 10, replace=False)] = 1.0
    dt = 0.002

    def engine(pair):
        monkeypatch.setenv("GRAVHMC_FOLD_PAIR", "1" if pair else "0")
        eng = G.Engine(N, M)
        eng.set_obs(*[np.ascontiguousarray(v) for v in obs])
        eng.set_cells(b6, 0)
        eng.build_G()
        wm = eng.weight(0.5)
        eng.set_data(Aw @ (wm * rho) + 0.01 * np.random.default_rng(18).normal(size=N))
        eng.set_reg(reg, 1.0, 0.01, shape, 0.001 * wm)
        return eng, wm

    def play(eng, pair):
        eng.chain_init(0.001 * wm, low, high)
        info = eng.fold_info()
        assert info["on"] and info["pair_on"] == pair, info
        out = []
        for L, p0, u in trajs:
            acc, o = eng.chain_trajectory(p0, dt, L, u)
            out.append((bool(acc), o.copy(), eng.chain_get_x()))
        return out

    eng, wm = engine(True)
    dobs = Aw @ (wm * rho) + 0.01 * np.random.default_rng(18).normal(size=N)
    P = orc.Problem(Aw, dobs, 0.001 * wm, reg, 1.0, 0.01, wm=wm, shape=shape)
    low, high = 0.0 * wm, 0.05 * wm
    # The oracle accepts wherever H falls, whatever u is, so a rejection has to be made: a momentum large enough that
    # the oracle's H rises by > 0.01 over the trajectory, and u half-way between exp(-dH) and 1 (accepted ones: the
    # small momentum of tests/test_gpu_fold.py and u half-way to 0).  Both far from the Metropolis edge.
    trajs, ref, xo = [], [], 0.001 * wm
    for want in WANT:
        for attempt in range(12):
            L = int(rng.integers(2, 7))
            p0 = rng.normal(size=M) * 0.01 * (0.7 ** attempt if want else 2.0 ** (attempt + 1))
            o = P.leapfrog(xo, p0, dt, L, low, high, 0.5)[2]
            dH = o[4] - o[3]
            if (want and dH < 5.0) or (not want and dH > 0.01):
                break
        else:
            raise AssertionError("no trajectory for the decision %r" % want)
        u = float(metropolis_u(dH, want))
        xo, acco, oo, _ = P.leapfrog(xo, p0, dt, L, low, high, u)
        assert acco == want
        trajs.append((L, p0, u))
        ref.append((acco, oo, xo))

    plain = play(eng, True)
    for (acc, o, x), (acco, oo, xo) in zip(plain, ref):
        assert acc == acco
        assert relmax(o, oo) <= 1e-10 and relmax(x, xo) <= 1e-10
    assert [a for a, _, _ in plain] == list(WANT)

    eng.chain_init(0.001 * wm, low, high)
    piped, last = [], 0.001 * wm
    eng.run_chain(iter(trajs), dt, lambda L, a_, o_, x_: piped.append((bool(a_), o_.copy(), x_)), want_x=True, batch=4,
                  overlap=True)
    assert len(piped) == len(plain)
    for (a1, o1, x1), (a2, o2, x2) in zip(plain, piped):
        last = x2 if x2 is not None else last
        assert a1 == a2 and np.array_equal(o1, o2) and np.array_equal(x1, last)
    x = 0.001 * wm
    for (L, p0, u), (acc, o, xs) in zip(trajs, plain):
        x, acc2, o2, _ = eng.leapfrog(x, p0, dt, L, low, high, u)
        assert bool(acc2) == acc and np.array_equal(x, xs) and np.array_equal(o2, o)
    eng.close()

    off, wm_off = engine(False)
    assert np.array_equal(wm_off, wm)
    plain_off = play(off, False)
    for (a1, o1, x1), (a2, o2, x2) in zip(plain, plain_off):
        assert a1 == a2 and relmax(o1, o2) <= 1e-10 and relmax(x1, x2) <= 1e-10
    off.close()


@pytest.mark.parametrize("n_obs,cells", [
    (24, (10, 10, 5)),     # 1 row per thread, one work item per workgroup
    (48, (22, 22, 5)),     # 2 rows (ldF = 576), 330 work items
    (70, (10, 10, 5)),     # 3 rows (ldF = 1232)
    (84, (26, 26, 7)),     # 4 rows (ldF = 1776), 637 work items: a short last workgroup
    (100, (26, 26, 7)),    # 5 rows (C2's nF = 2500, ldF = 2512)
])
def test_paired_sweep_modes_against_dense(G, monkeypatch, n_obs, cells):
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
    assert info["on"] and info["pair_on"] and info["pair_reason"] == "on", info
    assert (info["pairs"], info["single_orbits"]) == _counts(cells)
    assert info["bytes_per_sweep"] == (info["pairs"] + info["single_orbits"]) * _block_bytes(N)
    assert info["max_dev"] <= 1e-7
    again = _run(fold, wm, trajs, dt)
    fold.close()

    monkeypatch.setenv("GRAVHMC_FOLD", "0")
    dense, wm_d = _engine(G, mesh, obs, b6, 5)
    assert np.array_equal(wm_d, wm)
    res_d = _run(dense, wm_d, trajs, dt)
    info_d = dense.fold_info()
    assert not info_d["on"] and not info_d["pair_on"] and info_d["bytes_per_sweep"] == 0
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


def test_not_square_runs_the_mirror_fold_alone(G, monkeypatch):
    """20 x 30 cell columns on [0, 2000] x [0, 3000]: both mirrors, no tau: the bits of GRAVHMC_FOLD_PAIR=0."""
    monkeypatch.setenv("GRAVHMC_FOLD_MIN_MB", "0")
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    mesh = G.mesher.PrismMesh((0, 2000.0, 0, 3000.0, 0, 500.0), (100.0, 100.0, 100.0))
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 3000.0, 30), np.linspace(0, 2000.0, 20))]
    obs = np.stack([xp, yp, np.zeros_like(xp)])
    b6 = np.ascontiguousarray(mesh.cell_bounds())
    N, M = obs.shape[1], b6.shape[0]
    rng = np.random.default_rng(23)
    trajs = [(int(rng.integers(2, 6)), rng.normal(size=M) * 0.01, float(rng.uniform())) for _ in range(4)]
    results = []
    for pair in ("1", "0"):
        monkeypatch.setenv("GRAVHMC_FOLD_PAIR", pair)
        eng, wm = _engine(G, mesh, obs, b6, 5)
        results.append(_run(eng, wm, trajs, 0.002))
        info = eng.fold_info()
        assert info["on"] and not info["pair_on"], info
        assert info["pair_reason"] in ("observations not square", "cells not square"), info
        assert (info["pairs"], info["single_orbits"]) == (0, 0)
        assert info["bytes_per_sweep"] == info["store_bytes"] == (M // 4) * _block_bytes(N)
        eng.close()
    (mg1, ch1, pi1, lf1), (mg0, ch0, pi0, lf0) = results
    assert all(np.array_equal(u, v) for u, v in zip(mg1, mg0))
    for r1, r0 in ((ch1, ch0), (pi1, pi0), (lf1, lf0)):
        for (a1, o1, x1), (a2, o2, x2) in zip(r1, r0):
            assert a1 == a2 and np.array_equal(o1, o2)
            assert (x1 is None and x2 is None) or np.array_equal(x1, x2)


def test_fold_info_pair_keys_and_switch(G, monkeypatch):
    monkeypatch.setenv("GRAVHMC_FOLD_MIN_MB", "0")
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    cells = (20, 20, 6)
    mesh, obs, b6 = _problem(G, 20, cells)
    N, M = obs.shape[1], b6.shape[0]
    store = (M // 4) * _block_bytes(N)
    eng, wm = _engine(G, mesh, obs, b6, 5)
    before = eng.fold_info()
    assert not before["pair_on"] and before["pair_reason"] == "undecided" and before["bytes_per_sweep"] == 0
    eng.misfit_and_grad(0.01 * wm)
    info = eng.fold_info()
    assert info["on"] and info["pair_on"] and info["store_bytes"] == store
    assert (info["pairs"], info["single_orbits"]) == (270, 60) == _counts(cells)   # tests/test_fold_pair_host.py
    assert info["bytes_per_sweep"] == 330 * _block_bytes(N)
    eng.close()
    monkeypatch.setenv("GRAVHMC_FOLD_PAIR", "0")
    eng, wm = _engine(G, mesh, obs, b6, 5)
    eng.misfit_and_grad(0.01 * wm)
    info = eng.fold_info()
    assert info["on"] and not info["pair_on"] and info["pair_reason"] == "switched off"
    assert info["store_bytes"] == store == info["bytes_per_sweep"] and (info["pairs"], info["single_orbits"]) == (0, 0)
    eng.close()
