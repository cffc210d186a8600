"""GPU suite of the multi-component inversion (MultiComponentModule, GH_CELL_PRISM_MULTI): the row blocks of the one
store against the single-component engines and the reference's entries, one component against
GravMagModule(component=c), three components against the NumPy restatement of the model (tests/multicomp_host.py) on
the downloaded store, the per-block mean removal, HMCSample end to end, the refusals and a carved mesh.

Tolerances: blocks against the single-component engines and C = 1 against GravMagModule 1e-12; against the reference's
entries the fixture's 1e-10 max|K|; against the restatement 1e-10, the project's tolerance for these quantities."""
import numpy as np
import pytest

from conftest import gold
from helpers import relmax
from multicomp_host import MultiProblem, std_weights

pytestmark = pytest.mark.gpu

REGS = ("Damping", "MS", "Smoothness", "TV")
MRANGE, MSPACING = (0, 2000, 0, 3000, 0, 900), (300, 750, 500)
SHAPE = (3, 4, 4)


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def _obs(nx=7, ny=5):
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(100, 2900, ny), np.linspace(50, 1950, nx))]
    return xp, yp, np.full(xp.size, -30.0)


def _kernels(G, comps, obs):
    mesh = G.mesher.PrismMesh(MRANGE, MSPACING)
    mesh.addprop("density", np.zeros(mesh.size))
    return [getattr(G.prism, c)(obs[0], obs[1], obs[2], mesh)[1] for c in comps]


def _data(G, comps, obs, seed=3):
    """Synthetic observations of a dense block in the mesh, plus noise, per component"""
    rng = np.random.default_rng(seed)
    rho = np.zeros(SHAPE)
    rho[1:, 1:3, 1:3] = 0.4
    out = []
    for K in _kernels(G, comps, obs):
        d = K @ rho.ravel()
        out.append(d + 0.02 * np.abs(d).max() * rng.normal(size=d.size))
    return out


def _module(G, comps, obs, dobs, **kw):
    return G.MultiComponentModule(dobs, MRANGE, MSPACING, obs, components=comps, verbose=False, **kw)


# ----------------------------------------------------------------------------- the blocks of the store

def test_blocks_are_the_single_component_kernels(G):
    comps = ("gz", "gzz", "gxx", "gxy")
    obs = _obs()
    n = obs[0].size
    mc = _module(G, comps, obs, _data(G, comps, obs))
    assert mc.Aw.shape == (4 * n, 48) and mc.mshape == SHAPE
    for c, K in zip(comps, _kernels(G, comps, obs)):
        B = mc.kernel(c)
        assert B.shape == (n, 48)
        err = np.abs(B - K).max() / np.abs(K).max()
        print("%s block against prism.%s: %.3e of the largest entry" % (c, c, err))
        assert err <= 1e-12
    assert relmax(mc.A, np.vstack([mc.kernel(c) for c in comps])) == 0.0
    with pytest.raises(ValueError):
        mc.kernel("gyy")
    mc._engine.close()
    # before the weighting the blocks hold the single-component engines' entries bit for bit
    from gravinv3dhmc_amd import _lib
    mesh = G.mesher.PrismMesh(MRANGE, MSPACING)
    eng = G.Engine(4 * n, 48)
    eng.set_cells_multi(mesh.cell_bounds(), comps, np.ones(4))
    eng.set_obs(*obs)
    eng.build_G()
    S = eng.download_G()
    for b, c in enumerate(comps):
        one = G.Engine(n, 48)
        one.set_obs(*obs)
        one.set_cells(mesh.cell_bounds(), _lib.CELL_PRISM_COMP, component=c)
        one.build_G()
        K = one.download_G()
        assert np.abs(S[b * n:(b + 1) * n] - K).max() <= 1e-12 * np.abs(K).max()
        print("%s block bitwise equal to its engine's: %s" % (c, np.array_equal(S[b * n:(b + 1) * n], K)))
        one.close()
    eng.close()


def test_blocks_against_the_reference(G):
    g = gold("prism_comp_cases.npz")
    xp, yp, zp, cells = g["xp"], g["yp"], g["zp"], g["cells"]
    comps = ("gz", "gzz", "gxx", "gxy", "potential", "geoid", "gx", "gy", "gxz", "gyy", "gyz")
    n = xp.size
    eng = G.Engine(len(comps) * n, cells.shape[0])
    eng.set_cells_multi(cells, comps, np.ones(len(comps)))
    eng.set_obs(xp, yp, zp)
    eng.build_G()
    S = eng.download_G()
    for b, c in enumerate(comps):
        Kref = g["K_" + c]
        err = np.abs(S[b * n:(b + 1) * n] - Kref).max() / np.abs(Kref).max()
        print("%s block against the reference: max |dK|/max|K| = %.3e" % (c, err))
        assert err <= 1e-10, (c, err)
    eng.close()


# ----------------------------------------------------------------------------- one component

@pytest.mark.parametrize("comp", ["gz", "gzz"])
def test_one_component_is_the_single_component_module(G, comp):
    obs = _obs()
    dobs = _data(G, (comp,), obs)[0]
    mc = _module(G, (comp,), obs, [dobs])
    gm = G.GravMagModule(dobs, MRANGE, MSPACING, obs, component=comp, verbose=False)
    wm = gm.Wm.diagonal()
    assert np.array_equal(mc.weights, [1.0]) and np.array_equal(mc.Wb.diagonal(), np.ones(dobs.size))
    assert relmax(mc.Wm.diagonal(), wm) <= 1e-12 and relmax(np.asarray(mc.Aw), np.asarray(gm.Aw)) <= 1e-12
    assert relmax(mc.WmInv.diagonal(), gm.WmInv.diagonal()) <= 1e-12
    assert relmax(mc.WmSquare.diagonal(), gm.WmSquare.diagonal()) <= 1e-12
    rng = np.random.default_rng(5)
    M = wm.size
    mwapr = 0.001 * wm
    worst = 0.0
    for reg in REGS:
        x = rng.uniform(0, 0.02, M) * wm
        a = mc.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        b = gm.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        errs = [abs(a[0] - b[0]) / abs(b[0]), relmax(a[1], b[1]), relmax(a[2], b[2]), abs(a[3] - b[3]) / abs(b[3]),
                abs(a[4] - b[4]) / max(abs(b[4]), 1e-300)]
        worst = max(worst, max(errs))
        assert max(errs) <= 1e-12, (reg, errs)
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(5)]
    outs = []
    for m in (mc, gm):
        e = m._engine
        e.set_reg("TV", 1.0, 0.001, SHAPE, mwapr)
        e.chain_init(mwapr, 0.0 * wm, 0.02 * wm)
        res = []
        e.run_chain(iter(trajs), 0.02, lambda L, acc, o, x, res=res: res.append((acc, o.copy(), x)), want_x=True)
        outs.append(res)
    assert len(outs[0]) == len(outs[1]) == 5
    for (a1, o1, x1), (a2, o2, x2) in zip(*outs):
        assert a1 == a2 and relmax(o1, o2) <= 1e-12 and (x1 is None) == (x2 is None)
        assert x1 is None or relmax(x1, x2) <= 1e-12
        worst = max(worst, relmax(o1, o2))
    print("%s alone against GravMagModule(component=%r): worst %.3e" % (comp, comp, worst))
    assert mc._engine.chain_stats()["resident_launches"] == 0     # (the store runs on the fused sweep)
    assert not mc._engine.fold_info()["on"]
    mc._engine.close()
    gm._engine.close()


# ----------------------------------------------------------------------------- three components

def _check_three(G, weights):
    comps = ("gz", "gzz", "gxx")
    obs = _obs()
    n = obs[0].size
    dobs = _data(G, comps, obs)
    mc = _module(G, comps, obs, dobs, weights=weights)
    w = std_weights(dobs) if isinstance(weights, str) else np.asarray(weights, dtype=float)
    assert relmax(mc.weights, w) <= 1e-10 and mc.weights[0] == w[0]
    wb = np.repeat(w, n)
    assert relmax(mc.Wb.diagonal(), wb) <= 1e-10
    eng = mc._engine
    Aw = np.array(eng.download_G())
    wm = mc.Wm.diagonal()
    # Wm: the column norms of Wb A, A being the single-component kernels
    WA = np.vstack(_kernels(G, comps, obs)) * wb[:, None]
    assert relmax(wm, np.sqrt((WA ** 2).sum(axis=0))) <= 1e-10
    assert relmax(Aw * wm[None, :], WA) <= 1e-10
    dobsw = wb * np.concatenate(dobs)
    assert relmax(mc.dobsw, dobsw) <= 1e-10
    rng = np.random.default_rng(7)
    M = wm.size
    mwapr = 0.001 * wm
    worst = 0.0
    for reg in REGS:
        P = MultiProblem(Aw, dobsw, 3, mwapr, reg, 0.7, 0.001, wm=wm, shape=SHAPE)
        for _ in range(2):
            x = rng.uniform(0, 0.02, M) * wm
            a = mc.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
            b = P.misfit_and_grad(x)
            pm, om = mc.block_means()
            errs = [abs(a[0] - b[0]) / abs(b[0]), relmax(a[1], b[1]), relmax(a[2], b[2]), abs(a[3] - b[3]) / abs(b[3]),
                    abs(a[4] - b[4]) / max(abs(b[4]), 1e-300), relmax(pm, P.pred_mean), relmax(om, P.obs_mean)]
            worst = max(worst, max(errs))
            assert max(errs) <= 1e-10, (reg, errs)
    # a chain: ordinary trajectories, and some that overshoot with a Metropolis variate next to 1
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(5)]
    trajs += [(8, rng.normal(size=M) * 3.0, 1.0 - 1e-9) for _ in range(5)]
    trajs += [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(2)]
    low, high = 0.0 * wm, 0.02 * wm
    P = MultiProblem(Aw, dobsw, 3, mwapr, "TV", 1.0, 0.001, wm=wm, shape=SHAPE)
    ref = P.chain(mwapr, trajs, 0.02, low, high)
    eng.set_reg("TV", 1.0, 0.001, SHAPE, mwapr)
    eng.chain_init(mwapr, low, high)
    res = []
    eng.run_chain(iter(trajs), 0.02, lambda L, acc, o, x: res.append((acc, o.copy(), x)), want_x=True)
    assert len(res) == len(ref)
    print("decisions:", [a for a, _, _ in ref])
    assert any(a for a, _, _ in ref) and any(not a for a, _, _ in ref)
    for (a1, o1, x1), (a2, o2, x2) in zip(res, ref):
        assert a1 == a2
        assert relmax(o1, o2) <= 1e-10
        assert x1 is None or relmax(x1, x2) <= 1e-10
        worst = max(worst, relmax(o1, o2))
    print("three components, weights %r: worst against the restatement %.3e" % (weights, worst))
    eng.close()


def test_three_components_std_weights_against_the_restatement(G):
    _check_three(G, "std")


def test_three_components_explicit_weights_against_the_restatement(G):
    _check_three(G, (2.0, 0.013, 0.07))


@pytest.mark.parametrize("nx,ny", [(28, 25), (60, 35)])
def test_three_components_on_the_multi_wave_sweeps(G, nx, ny):
    """The stacked store where a team is several waves and the slab has hundreds of rows: 3 x 700 = 2100 rows (4-wave
    teams) and 3 x 2100 = 6300 rows (16-wave teams) over 6 x 12 x 10 cells, against the restatement at 1e-10."""
    mrange, mspacing, shape = (0, 2000, 0, 3000, 0, 900), (150, 250, 200), (6, 12, 10)
    comps = ("gz", "gzz", "gxx")
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(100, 2900, ny), np.linspace(50, 1950, nx))]
    obs = (xp, yp, np.full(xp.size, -30.0))
    n = xp.size
    mesh = G.mesher.PrismMesh(mrange, mspacing)
    mesh.addprop("density", np.zeros(mesh.size))
    rng = np.random.default_rng(13)
    rho = np.zeros(shape)
    rho[2:, 4:8, 3:7] = 0.4
    dobs = []
    for c in comps:
        d = getattr(G.prism, c)(obs[0], obs[1], obs[2], mesh)[1] @ rho.ravel()
        dobs.append(d + 0.02 * np.abs(d).max() * rng.normal(size=n) + 7.0)
    mc = G.MultiComponentModule(dobs, mrange, mspacing, obs, components=comps, verbose=False)
    eng = mc._engine
    lay = eng.sweep_layout()
    print("rows %d, sweep layout %r" % (3 * n, lay))
    assert 3 * n >= 2048 and lay["tw"] == (4 if 3 * n <= 4096 else 16) and lay["n_panels"] == 1 and lay["grid"] > 64
    w = std_weights(dobs)
    wb = np.repeat(w, n)
    assert relmax(mc.weights, w) <= 1e-10
    Aw = np.array(eng.download_G())
    wm = mc.Wm.diagonal()
    M = wm.size
    assert Aw.shape == (3 * n, 720)
    dobsw = wb * np.concatenate(dobs)
    mwapr = 0.001 * wm
    worst = 0.0
    for reg in REGS:
        P = MultiProblem(Aw, dobsw, 3, mwapr, reg, 0.7, 0.001, wm=wm, shape=shape)
        x = rng.uniform(0, 0.02, M) * wm
        a = mc.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        b = P.misfit_and_grad(x)
        pm, om = mc.block_means()
        errs = [abs(a[0] - b[0]) / abs(b[0]), relmax(a[1], b[1]), relmax(a[2], b[2]), abs(a[3] - b[3]) / abs(b[3]),
                abs(a[4] - b[4]) / max(abs(b[4]), 1e-300), relmax(pm, P.pred_mean), relmax(om, P.obs_mean)]
        worst = max(worst, max(errs))
        assert max(errs) <= 1e-10, (reg, errs)
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(4)]
    trajs += [(8, rng.normal(size=M) * 3.0, 1.0 - 1e-9)]
    low, high = 0.0 * wm, 0.02 * wm
    P = MultiProblem(Aw, dobsw, 3, mwapr, "TV", 1.0, 0.001, wm=wm, shape=shape)
    ref = P.chain(mwapr, trajs, 0.02, low, high)
    eng.set_reg("TV", 1.0, 0.001, shape, mwapr)
    eng.chain_init(mwapr, low, high)
    res = []
    eng.run_chain(iter(trajs), 0.02, lambda L, acc, o, x: res.append((acc, o.copy(), x)), want_x=True)
    assert len(res) == len(ref)
    for (a1, o1, x1), (a2, o2, x2) in zip(res, ref):
        assert a1 == a2 and relmax(o1, o2) <= 1e-10 and (x1 is None or relmax(x1, x2) <= 1e-10)
        worst = max(worst, relmax(o1, o2))
    print("%d stacked rows: worst against the restatement %.3e, decisions %r" % (3 * n, worst, [a for a, _, _ in ref]))
    eng.close()


def test_the_mean_is_removed_per_block(G):
    comps = ("gz", "gzz", "gxx")
    obs = _obs()
    n = obs[0].size
    dobs = _data(G, comps, obs)
    w = std_weights(dobs)                       # (a constant added to a block leaves its std as it is)
    shifted = [d + k for d, k in zip(dobs, (5.0, -700.0, 300.0))]
    a, b = _module(G, comps, obs, dobs), _module(G, comps, obs, shifted)
    assert relmax(b.weights, w) <= 1e-12
    wm = a.Wm.diagonal()
    rng = np.random.default_rng(11)
    x = rng.uniform(0, 0.02, wm.size) * wm
    mwapr = 0.001 * wm
    ra = a.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization="MS", beta=0.001)
    rb = b.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization="MS", beta=0.001)
    assert abs(ra[0] - rb[0]) <= 1e-10 * abs(ra[0]) and relmax(rb[1], ra[1]) <= 1e-10
    assert relmax(b.block_means()[1] - a.block_means()[1], w * np.array([5.0, -700.0, 300.0])) <= 1e-10
    # one mean over all rows would have changed both: the restatement with a global mean says by how much
    Aw = np.array(a._engine.download_G())
    wb = np.repeat(w, n)
    ga = MultiProblem(Aw, wb * np.concatenate(dobs), 3, mwapr, "MS", 0.7, 0.001, wm=wm, global_mean=True).misfit_and_grad(x)
    gb = MultiProblem(Aw, wb * np.concatenate(shifted), 3, mwapr, "MS", 0.7, 0.001, wm=wm, global_mean=True).misfit_and_grad(x)
    assert abs(ga[0] - gb[0]) > 1e-3 * abs(ga[0]) and relmax(gb[1], ga[1]) > 1e-3
    # ... and the device agrees with neither of them
    assert abs(ra[0] - ga[0]) > 1e-6 * abs(ga[0])
    a._engine.close()
    b._engine.close()


# ----------------------------------------------------------------------------- the sampler

def _hmc(G, mc, folder, seed=100):
    M = mc.Wm.shape[0]
    return G.HMCSample(mc, 6, 2, 0.02, [3, 8], np.full(M, 0.001), np.full(M, 0.001),
                       np.c_[np.full(M, 0.0), np.full(M, 0.02)], "mandatory", 1000, mc.dobs,
                       "Fixed", 0.8, 1.0, "TV", 0.001, seed, 0.3, nbest=100, myrank=0, save_folder=folder)


def test_hmcsample_end_to_end_on_two_components(G, tmp_path, capsys):
    comps = ("gz", "gzz")
    obs = _obs()
    n = obs[0].size
    dobs = _data(G, comps, obs)
    files = []
    for run in ("a", "b"):
        mc = _module(G, comps, obs, {"gzz": dobs[1], "gz": dobs[0]})
        folder = str(tmp_path / ("run_%s_chain" % run))
        _hmc(G, mc, folder)
        capsys.readouterr()
        files.append((open(folder + "0/misfit.dat", "rb").read(), open(folder + "0/model.dat", "rb").read()))
        misfit, model = np.loadtxt(folder + "0/misfit.dat"), np.loadtxt(folder + "0/model.dat")
        assert misfit.shape == (6, 7) and model.shape == (6, 48)
        assert np.isfinite(misfit).all() and (model >= 0).all() and (model <= 0.02).all()
        last = model[-1]
        wm, wb = mc.Wm.diagonal(), mc.Wb.diagonal()
        fwd = mc.forward(last)
        assert fwd.shape == (2 * n,)
        assert relmax(fwd, (np.asarray(mc.Aw) @ (wm * last)) / wb) <= 1e-10
        # each block in its own units: against the component's own kernel
        assert relmax(fwd[n:], mc.kernel("gzz") @ last) <= 1e-10
        mc._engine.close()
    assert files[0] == files[1]          # the same seed: the same chain, bit for bit


# ----------------------------------------------------------------------------- refusals, a carved mesh

def test_refusals_name_the_store(G):
    comps = ("gz", "gzz")
    obs = _obs()
    dobs = _data(G, comps, obs)
    for kw in ({"coordinate": "spherical"}, {"wavelet": "3D"}, {"matrix_free": True}, {"shift_invariant": True},
               {"shard": object()}):
        with pytest.raises(NotImplementedError, match="multi-component store"):
            _module(G, comps, obs, dobs, **kw)
    mc = _module(G, comps, obs, dobs)
    eng = mc._engine
    wm = mc.Wm.diagonal()
    M = wm.size
    with pytest.raises(NotImplementedError, match="multi-component store"):
        G.HMCSampleBatch(mc, 2, 4, 0, 0.02, [3, 8], np.full(M, 0.001), np.full(M, 0.001),
                         np.c_[np.full(M, 0.0), np.full(M, 0.02)], "mandatory", 1000, mc.dobs,
                         "Fixed", 0.8, 1.0, "MS", 0.001, 100, 0.3, save_folder="unused_chain")
    with pytest.raises(NotImplementedError, match="multi-component store"):
        eng.batch_init(np.stack([0.001 * wm, 0.002 * wm]), 0.0 * wm, 0.02 * wm)
    with pytest.raises(NotImplementedError, match="multi-component store"):
        eng.compress_wavelet(3, SHAPE, 0.001, 2)
    with pytest.raises(NotImplementedError, match="multi-component store"):
        eng.upload_G(np.zeros((eng.N, eng.M)))
    with pytest.raises(NotImplementedError, match="multi-component store"):
        eng.set_matrix_free(True)
    with pytest.raises(NotImplementedError, match="multi-component store"):
        eng.set_shift_invariant(True)
    assert not eng.fold_info()["on"]                               # never folded, whatever the grid's symmetry
    eng.close()
    # the library's own checks: a fresh context, distinct components, positive weights, the row limit
    from gravinv3dhmc_amd import _lib
    cell = np.array([[0, 1, 0, 1, 0, 1.0]])
    e = G.Engine(4, 1)
    with pytest.raises(ValueError):
        e.set_cells_multi(cell, ("gz", "gz"), (1.0, 1.0))
    with pytest.raises(ValueError):
        e.set_cells_multi(cell, ("gz", "gzz"), (1.0, 0.0))
    with pytest.raises(ValueError):
        e.set_cells_multi(cell, ("gz", "gzz", "gxx"), (1.0, 1.0, 1.0))      # 4 rows are not 3 blocks
    e.set_cells_multi(cell, ("gz", "gzz"), (1.0, 1.0))
    with pytest.raises(NotImplementedError, match="gh_set_cells_multi"):
        e.set_cells(cell, _lib.CELL_PRISM)
    e.close()
    e = G.Engine(16386, 1)
    with pytest.raises(NotImplementedError, match="16384"):
        e.set_cells_multi(cell, ("gz", "gzz"), (1.0, 1.0))
    e.close()
    e = G.Engine(4, 1)
    e.set_obs(np.zeros(4), np.zeros(4), np.full(4, -1.0))
    with pytest.raises(ValueError, match="fresh context"):
        e.set_cells_multi(cell, ("gz", "gzz"), (1.0, 1.0))
    e.close()


def test_carved_mesh(G):
    comps = ("gz", "gzz")
    obs = _obs()
    dobs = _data(G, comps, obs)
    xs, ys = np.meshgrid(np.linspace(0, 2000, 9), np.linspace(0, 3000, 9))
    topo = np.where(xs.ravel() < 1000, -350.0, 100.0)             # the surface dips into the mesh on one side
    mc = _module(G, comps, obs, dobs, mtopo=(xs.ravel(), ys.ravel(), topo))
    M = mc.Wm.shape[0]
    assert mc.topocarve and 0 < M < 48 and mc.Aw.shape == (2 * obs[0].size, M)
    assert mc._engine.M == M and np.asarray(mc.Aw).shape == (2 * obs[0].size, M)
    wm = mc.Wm.diagonal()
    x, mwapr = 0.004 * wm, 0.001 * wm
    Aw = np.array(mc._engine.download_G())
    for reg in ("Damping", "MS"):
        a = mc.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        b = MultiProblem(Aw, mc.dobsw, 2, mwapr, reg, 0.7, 0.001, wm=wm).misfit_and_grad(x)
        assert abs(a[0] - b[0]) <= 1e-10 * abs(b[0]) and relmax(a[1], b[1]) <= 1e-10
    for reg in ("Smoothness", "TV"):
        with pytest.raises(ValueError):
            mc.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
    mc._engine.close()
