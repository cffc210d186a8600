"""GPU suite (`-m gpu`): the stored kernel folded over the grid's two mirrors (csrc/fold.hip.h, host_fold.h).

Small mirror-symmetric prism problems with the fold forced (GRAVHMC_FOLD_MIN_MB=0; GRAVHMC_RESIDENT=0 so that the
chain runs on the sweep path): trajectories against oracle.Problem (<= 1e-10, same decisions), the chain bitwise
against itself with the next trajectory's first step piped, and against stateless gh_leapfrog.  At BASELINE's C2
(40 GB) one chain folded against one dense, same draws."""
import numpy as np
import pytest

from helpers import relmax

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _symmetric(G, n_obs, cells, shuffle=False):
    """n_obs x n_obs observations and cells[0] x cells[1] x cells[2] prisms on [0, 2000]^2 x [0, 1000]."""
    mesh = G.mesher.PrismMesh((0, 2000.0, 0, 2000.0, 0, 1000.0),
                              (1000.0 / cells[2], 2000.0 / cells[1], 2000.0 / cells[0]))
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 2000.0, n_obs), np.linspace(0, 2000.0, n_obs))]
    obs = np.stack([xp, yp, np.zeros_like(xp)])
    b6 = mesh.cell_bounds()
    if shuffle:
        rng = np.random.default_rng(3)
        obs = obs[:, rng.permutation(obs.shape[1])]
        b6 = b6[rng.permutation(b6.shape[0])]
    return mesh, obs, np.ascontiguousarray(b6)


def _engine(G, obs, b6):
    eng = G.Engine(obs.shape[1], b6.shape[0])
    eng.set_obs(*[np.ascontiguousarray(v) for v in obs])
    eng.set_cells(b6, 0)
    eng.build_G()
    return eng


@pytest.mark.parametrize("reg", ["Damping", "MS", "Smoothness", "TV"])
@pytest.mark.parametrize("size", [(24, (10, 10, 5), False), (48, (12, 12, 6), True)])
def test_folded_chain_against_oracle_and_bitwise_paths(G, orc, monkeypatch, reg, size):
    monkeypatch.setenv("GRAVHMC_FOLD_MIN_MB", "0")
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    n_obs, cells, shuffle = size
    mesh, obs, b6 = _symmetric(G, n_obs, cells, shuffle)
    N, M = obs.shape[1], b6.shape[0]
    rng = np.random.default_rng(7)
    Aw, wm_o = orc.col_weight(orc.prism_gz_kernel(obs[0], obs[1], obs[2], b6))
    eng = _engine(G, obs, b6)
    wm = eng.weight(0.5)
    assert relmax(wm, wm_o) <= 1e-11
    # a density block in the middle and noise: data that is not itself symmetric
    rho = np.zeros(M)
    rho[rng.choice(M, M // 10, replace=False)] = 1.0
    dobs = Aw @ (wm * rho) + 0.01 * rng.normal(size=N)
    eng.set_data(dobs)
    shape = mesh.shape if not shuffle else (1, 1, M)  # (stencils follow the caller's cell order)
    eng.set_reg(reg, 1.0, 0.01, shape, 0.001 * wm)
    P = orc.Problem(Aw, dobs, 0.001 * wm, reg, 1.0, 0.01, wm=wm, shape=shape)
    low, high = 0.0 * wm, 0.05 * wm
    dt = 0.002
    trajs = [(int(rng.integers(2, 7)), rng.normal(size=M) * 0.01, float(rng.uniform())) for _ in range(10)]

    # chain trajectory by trajectory, against the oracle
    eng.chain_init(0.001 * wm, low, high)
    info = eng.fold_info()
    assert info["on"], info
    assert info["store_bytes"] == (M // 4) * 4 * ((N // 4 + 15) // 16 * 16) * 8
    assert info["max_dev"] <= 1e-7
    plain = []
    xo = 0.001 * wm
    for L, p0, u in trajs:
        acc, o = eng.chain_trajectory(p0, dt, L, u)
        x = eng.chain_get_x()
        plain.append((acc, o.copy(), x))
        xo, acco, oo, _ = P.leapfrog(xo, p0, dt, L, low, high, u)
        assert bool(acc) == bool(acco)
        assert relmax(o, oo) <= 1e-10 and relmax(x, xo) <= 1e-10
    assert 0 < sum(a for a, _, _ in plain)

    # the next trajectory's first step piped into the last sweep (run_chain, overlap): the same bits
    eng.chain_init(0.001 * wm, low, high)
    piped, last = [], 0.001 * wm
    eng.run_chain(iter(trajs), dt, lambda L, a_, o_, x_: piped.append((a_, o_.copy(), x_)), want_x=True, batch=4,
                  overlap=True)
    assert len(piped) == len(plain)
    for (a1, o1, x1), (a2, o2, x2) in zip(plain, piped):
        last = x2 if x2 is not None else last
        assert a1 == a2 and np.array_equal(o1, o2) and np.array_equal(x1, last)

    # stateless gh_leapfrog on the same store: the same bits as the chain
    x = 0.001 * wm
    for (L, p0, u), (acc, o, xs) in zip(trajs, plain):
        x, acc2, o2, _ = eng.leapfrog(x, p0, dt, L, low, high, u)
        assert acc2 == acc and np.array_equal(x, xs) and np.array_equal(o2, o)

    # misfit and gradient on the folded store against the oracle; forward and adjoint (the operator itself) read the
    # dense store: the same bits as with the fold switched off
    xt = rng.uniform(0, 0.05, M) * wm
    out = eng.misfit_and_grad(xt)
    ref = P.misfit_and_grad(xt)
    assert abs(out[0] - ref[0]) <= 1e-10 * abs(ref[0]) and relmax(out[1], ref[1]) <= 1e-10
    assert relmax(out[2], ref[2]) <= 1e-10
    r = rng.normal(size=N)
    fw, ad = eng.forward(xt), eng.adjoint(r)
    assert eng.fold_info()["on"]
    monkeypatch.setenv("GRAVHMC_FOLD", "0")
    dense = _engine(G, obs, b6)
    assert np.array_equal(dense.weight(0.5), wm)
    assert np.array_equal(dense.forward(xt), fw) and np.array_equal(dense.adjoint(r), ad)
    dense.close()
    eng.close()


def test_fold_refused_or_off(G, monkeypatch):
    """Below the size threshold, switched off, a non-gz component, an uploaded G: the dense sweep, with the reason."""
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    mesh, obs, b6 = _symmetric(G, 24, (10, 10, 5))
    N, M = obs.shape[1], b6.shape[0]
    x = np.full(M, 0.1)

    def forward_reason(eng):
        wm = eng.weight(0.5)
        eng.set_data(np.zeros(N))
        eng.set_reg("Damping", 1.0, 0.01, mesh.shape, 0.001 * wm)
        eng.misfit_and_grad(x)
        info = eng.fold_info()
        assert not info["on"]
        return info["reason"]

    monkeypatch.delenv("GRAVHMC_FOLD_MIN_MB", raising=False)
    assert forward_reason(_engine(G, obs, b6)) == "small"
    monkeypatch.setenv("GRAVHMC_FOLD_MIN_MB", "0")
    monkeypatch.setenv("GRAVHMC_FOLD", "0")
    assert forward_reason(_engine(G, obs, b6)) == "switched off"
    monkeypatch.delenv("GRAVHMC_FOLD")
    e = G.Engine(N, M)
    e.set_obs(*obs)
    e.set_cells(b6, 0, component="gzz")
    e.build_G()
    assert forward_reason(e) == "not gz prisms"
    e = G.Engine(N, M)
    e.set_obs(*obs)
    e.set_cells(b6, 0)
    e.upload_G(np.ones((N, M)))
    assert forward_reason(e) == "not gz prisms"
    obs2 = obs.copy()
    obs2[0, 5] += 1e-6
    assert forward_reason(_engine(G, obs2, b6)) == "observations not mirror-symmetric"
    # and the same problem folds, at its first sweep of the potential (not at gh_forward's)
    e = _engine(G, obs, b6)
    wm = e.weight(0.5)
    e.forward(x)
    assert e.fold_info()["reason"] == "undecided"
    e.set_data(np.zeros(N))
    e.set_reg("Damping", 1.0, 0.01, mesh.shape, 0.001 * wm)
    e.misfit_and_grad(x)
    assert e.fold_info()["on"]


def test_c2_full_size_folded_chain_against_dense(G, monkeypatch):
    """BASELINE configs[1] (10^4 x 5*10^5, dense G 40 GB): the folded store (10.05 GB) against the dense sweep,
    one chain each, the same draws: identical decisions, out5 and x within 1e-10."""
    nx = ny = 100
    nz = 50
    mesh = G.mesher.PrismMesh((0, 100.0 * nx, 0, 100.0 * ny, 0, 100.0 * nz), (100, 100, 100))
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 100.0 * ny, ny), np.linspace(0, 100.0 * nx, nx))]
    zp = np.zeros_like(xp)
    N, M = xp.size, mesh.size
    bounds = mesh.cell_bounds()
    rng = np.random.default_rng(4)

    def make():
        e = G.Engine(N, M)
        e.set_obs(xp, yp, zp)
        e.set_cells(bounds, 0)
        e.build_G()
        return e

    rho = np.zeros(mesh.shape)
    rho[10:25, 40:60, 40:60] = 1.0
    dt = 0.002
    trajs = [(int(rng.integers(3, 8)), rng.normal(size=M) * 0.001, float(rng.uniform())) for _ in range(4)]
    res = {}
    for mode in ("dense", "folded"):
        if mode == "dense":
            monkeypatch.setenv("GRAVHMC_FOLD", "0")
        else:
            monkeypatch.delenv("GRAVHMC_FOLD", raising=False)
        e = make()
        wm = e.weight(0.5)
        if mode == "dense":
            d_true = e.forward(wm * rho.ravel())
            dobs = d_true + 0.02 * np.abs(d_true).max() * np.random.default_rng(21).normal(size=N)
        e.set_data(dobs)
        e.set_reg("Damping", 1.0, 0.01, mesh.shape, 0.001 * wm)
        e.chain_init(0.001 * wm, 0.0 * wm, 1.0 * wm)
        out = []
        for L, p0, u in trajs:
            a, o = e.chain_trajectory(p0, dt, L, u)
            out.append((bool(a), o.copy()))
        res[mode] = (out, e.chain_get_x(), e.fold_info())
        e.close()
    (od, xd, fi_d), (of, xf, fi_f) = res["dense"], res["folded"]
    assert not fi_d["on"] and fi_d["reason"] == "switched off"
    assert fi_f["on"], fi_f
    assert fi_f["store_bytes"] == 125000 * 4 * 2512 * 8
    assert fi_f["max_dev"] <= 1e-7
    worst = 0.0
    for (a1, o1), (a2, o2) in zip(od, of):
        assert a1 == a2, (o1, o2)
        worst = max(worst, relmax(o1, o2))
    worst = max(worst, relmax(xd, xf))
    print("C2 full size, folded store (%.2f GB, max_dev %.2e, built in %.0f ms) vs dense: %.2e"
          % (fi_f["store_bytes"] / 1e9, fi_f["max_dev"], fi_f["build_ms"], worst))
    assert worst <= 1e-10
