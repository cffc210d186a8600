"""GPU suite (`-m gpu`): the HIP path, called through the C-ABI (ctypes -> libgravhmc.so),
against the CPU oracle on the same seeded inputs, against the golden vectors generated from
the reference, and -- at BASELINE.json's full size -- through size-independent properties.

Tolerances (fp64, stated per test):
  * kernel entries: |dK| <= 1e-10 * max|K| (device libm vs glibc inside an 8-term
    alternating sum); forward data d = G rho: <= 1e-10 relative (north_star)
  * GEMV / potential / trajectories: 1e-11 .. 1e-9 relative (summation order differs)
"""
import os

import numpy as np
import pytest

from conftest import gold
from helpers import c1_inputs, relmax

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


# ----------------------------------------------------------------------------- assembly

def test_prism_entries_singular_geometries(G):
    g = gold("prism_cases.npz")
    eng = G.Engine(g["xp"].size, g["cells"].shape[0])
    eng.set_obs(g["xp"], g["yp"], g["zp"])
    eng.set_cells(g["cells"], 0)
    eng.build_G()
    K = eng.download_G()
    assert np.isfinite(K).all()
    err = np.abs(K - g["K"]).max() / np.abs(g["K"]).max()
    print("prism singular cases: max |dK|/max|K| = %.3e" % err)
    assert err < 1e-10
    eng.close()


def test_c1_kernel_and_forward(G, orc):
    g = gold("c1_spot.npz")
    mesh, xp, yp, zp = c1_inputs()
    mesh.addprop('density', g["rho"])
    gz, K = G.prism.gz(xp, yp, zp, mesh)
    assert K.shape == (600, 6000) and K.flags.f_contiguous
    e_entries = np.abs(K[g["ii"], g["jj"]] - g["Kij"]).max() / np.abs(g["Kij"]).max()
    e_col = relmax(np.sqrt((K ** 2).sum(0)), g["colnorm"])
    e_gz = np.abs(gz - g["gz"]).max() / np.abs(g["gz"]).max()
    e_gz_pt = np.abs((gz - g["gz"]) / g["gz"]).max()
    print("C1: entries %.3e colnorm %.3e d_obs %.3e (pointwise %.3e)" % (e_entries, e_col, e_gz, e_gz_pt))
    assert e_entries < 1e-10 and e_col < 1e-11
    assert e_gz_pt < 1e-10          # north_star: reference d_obs to <= 1e-10 relative
    Ko = orc.prism_gz_kernel(xp, yp, zp, mesh.cell_bounds())
    assert np.abs(K - Ko).max() / np.abs(Ko).max() < 1e-10


def test_tesseroid_entries(G):
    g = gold("tess_cases.npz")
    eng = G.Engine(g["lon"].size, g["bounds"].shape[0])
    eng.set_obs(g["lon"], g["lat"], g["h"])
    eng.set_cells(g["bounds"], 1, 1.6)
    eng.build_G()
    K = eng.download_G()
    st = eng.kernel_stats()
    err = np.abs(K - g["K"]).max() / np.abs(g["K"]).max()
    print("tess coarse-global: %.3e leaves %d (ref %d)" % (err, st["leaves"], int(g["leaves"])))
    assert err < 1e-10
    assert st["leaves"] == int(g["leaves"]) and st["warn_cells"] == 0   # same leaf SET
    d = eng.forward(g["rho"])
    assert np.abs((d - g["gz"]) / g["gz"]).max() < 1e-10
    eng.close()
    # near field / thin cells / poles
    eng = G.Engine(g["n_lon"].size, g["n_cells"].shape[0])
    eng.set_obs(g["n_lon"], g["n_lat"], g["n_h"])
    eng.set_cells(g["n_cells"], 1, 1.6)
    eng.build_G()
    K = eng.download_G()
    st = eng.kernel_stats()
    err = np.abs(K - g["n_K"]).max() / np.abs(g["n_K"]).max()
    print("tess near-field: %.3e leaves %d (ref %d)" % (err, st["leaves"], int(g["n_leaves"])))
    assert err < 1e-10
    assert st["leaves"] == int(g["n_leaves"])
    assert st["warn_cells"] == int((g["n_err"] != 0).sum())
    eng.close()


def test_tesseroid_frontend_warns_and_matches(G):
    g = gold("tess_cases.npz")
    mesh = G.mesher.TesseroidMesh((-180, 180, -90, 90, 0, -3e6), (-300000, 30, 30))
    mesh.addprop('density', g["rho"])
    res, K = G.tesseroid.gz(g["lon"], g["lat"], g["h"], mesh)
    assert np.abs((res - g["gz"]) / g["gz"]).max() < 1e-10 and K.shape == g["K"].shape


# ----------------------------------------------------------------------- GEMV primitives

@pytest.mark.parametrize("N,M", [(1, 1), (17, 5), (42, 120), (600, 257), (625, 1000), (1024, 64),
                                 (1025, 300), (2500, 123), (4097, 77), (5000, 200), (6144, 50), (6145, 50), (7381, 300),
                                 (10000, 513),
                                 (16384, 40), (16385, 21), (20000, 77), (40000, 33)])
def test_forward_adjoint_vs_numpy(G, N, M):
    rng = np.random.default_rng(N * 1000 + M)
    A = np.asfortranarray(rng.normal(size=(N, M)))
    x, r = rng.normal(size=M), rng.normal(size=N)
    eng = G.Engine(N, M)
    eng.upload_G(A)
    assert np.array_equal(eng.download_G(), A)
    d, g = eng.forward(x), eng.adjoint(r)
    scale_d = np.abs(A) @ np.abs(x)
    scale_g = np.abs(A.T) @ np.abs(r)
    assert (np.abs(d - A @ x) / scale_d).max() < 1e-14 * max(1, np.sqrt(M))
    assert (np.abs(g - A.T @ r) / scale_g).max() < 1e-14 * max(1, np.sqrt(N))
    # row-major upload path gives the same device matrix
    eng2 = G.Engine(N, M)
    eng2.upload_G(np.ascontiguousarray(A))
    assert np.array_equal(eng2.download_G(), A)
    eng.close()
    eng2.close()


def test_weighting_vs_oracle(G, orc):
    rng = np.random.default_rng(5)
    A = rng.normal(size=(333, 211)) * rng.uniform(0.01, 10, size=211)
    A[:, 7] = 0.0                                     # zero column: left untouched, wm = 0
    eng = G.Engine(333, 211)
    eng.upload_G(A)
    wm = eng.weight(0.5)
    Aw_o, wm_o = orc.col_weight(A, 0.5)
    assert relmax(wm, wm_o) < 1e-14 and wm[7] == 0.0
    assert relmax(eng.download_G(), Aw_o) < 1e-14
    eng.close()
    eng = G.Engine(333, 211)
    eng.upload_G(A)
    wm = eng.weight(0.3)
    _, wm_o = orc.col_weight(A, 0.3)
    assert relmax(wm, wm_o) < 1e-13
    eng.close()


# ----------------------------------------------------------------------------- potential

def _small_engine(G, p, fix=False):
    eng = G.Engine(*p["Aw"].shape)
    eng.upload_G(p["Aw"])
    eng.set_data(p["dobs"], p["gfix"] if fix else None)
    return eng


def test_misfit_and_grad_golden(G):
    p = gold("potential_small.npz")
    from gravinv3dhmc_amd import mesher
    mesh = mesher.PrismMesh(tuple(p["mrange"]), tuple(p["mspacing"]))
    worst = 0.0
    for fix, tag in ((False, ""), (True, "_fix")):
        eng = G.Engine(*p["Aw"].shape)
        eng.set_obs(p["xp"], p["yp"], p["zp"])
        eng.set_cells(mesh.cell_bounds(), 0)
        eng.build_G()
        wm = eng.weight(0.5)
        assert relmax(wm, p["wm"]) < 1e-11
        eng.set_data(p["dobs"], p["gfix"] if fix else None)
        for reg in ("Damping", "MS", "Smoothness", "TV"):
            eng.set_reg(reg, float(p["alpha"]), float(p["beta"]), p["shape"], p["mwapr"])
            for i, x in enumerate(p["xs"]):
                m, grad, dpre, dv, mv = eng.misfit_and_grad(x)
                errs = [abs(m - p[reg + tag + "_misfit"][i]) / abs(m),
                        relmax(grad, p[reg + tag + "_grad"][i]),
                        relmax(dpre, p[reg + tag + "_dpre"][i]),
                        abs(dv - p[reg + tag + "_data"][i]) / abs(dv),
                        abs(mv - p[reg + tag + "_model"][i]) / max(abs(mv), 1e-300)]
                worst = max(worst, max(errs))
                assert max(errs) < 1e-10, (reg, tag, i, errs)
        eng.close()
    print("misfit_and_grad worst rel err %.3e" % worst)


def test_error_behaviour(G):
    p = gold("potential_small.npz")
    eng = _small_engine(G, p)
    with pytest.raises(ValueError):
        eng.set_reg("Tikhonov", 1.0, 0.01, p["shape"], p["mwapr"])
    with pytest.raises(ValueError):                      # MS before weighting
        eng.set_reg("MS", 1.0, 0.01, p["shape"], p["mwapr"])
    with pytest.raises(ValueError):                      # TV on a shape that is not the mesh
        eng.set_reg("TV", 1.0, 0.01, (1, 1, 7), p["mwapr"])
    with pytest.raises(ValueError):                      # potential before the regulariser
        eng.misfit_and_grad(p["xs"][0])
    with pytest.raises(ValueError):
        eng.chain_trajectory(np.zeros(eng.M), 0.01, 5, 0.5)   # chain before chain_init
    eng.close()
    with pytest.raises(ValueError):
        G.Engine(10, 10).upload_G(np.zeros((9, 10)))     # wrong shape
    with pytest.raises(ValueError):
        G.Engine(0, 10)


# --------------------------------------------------------------------------- trajectories

def test_leapfrog_golden(G):
    g = gold("leapfrog_small.npz")
    p = gold("potential_small.npz")
    eng = _small_engine(G, p)
    eng._lib.gh_weight  # noqa: B018  (weights come from the fixture: Aw is already weighted)
    worst = 0.0
    for i in range(int(g["n"])):
        k = lambda s: g["%d_%s" % (i, s)]
        reg = str(k("reg"))
        if reg == "MS":
            continue  # needs wm on the device: covered by test_leapfrog_ms_via_module
        eng.set_reg(reg, 1.0, 0.001, p["shape"], k("mwapr"))
        x, acc, out, dsyn = eng.leapfrog(k("x_in"), k("p0"), float(k("dt")), int(k("L")),
                                         k("low"), k("high"), float(k("u")))
        assert acc == bool(k("acc")), i
        errs = [relmax(x, k("x_out")), abs(out[0] - float(k("U"))) / abs(out[0]),
                abs(out[1] - float(k("Ud"))) / abs(out[1]), relmax(dsyn, k("dsyn"))]
        worst = max(worst, max(errs))
        assert max(errs) < 1e-9, (i, reg, errs)
    print("leapfrog worst rel err %.3e" % worst)
    eng.close()


def _module_small(G, p, **kw):
    return G.GravMagModule(p["dobs"], tuple(p["mrange"]), tuple(p["mspacing"]),
                           (p["xp"], p["yp"], p["zp"]), verbose=False, **kw)


def test_leapfrog_ms_via_module(G):
    g = gold("leapfrog_small.npz")
    p = gold("potential_small.npz")
    gm = _module_small(G, p)
    eng = gm._engine
    n = 0
    for i in range(int(g["n"])):
        k = lambda s: g["%d_%s" % (i, s)]
        if str(k("reg")) != "MS":
            continue
        eng.set_reg("MS", 1.0, 0.001, p["shape"], k("mwapr"))
        x, acc, out, dsyn = eng.leapfrog(k("x_in"), k("p0"), float(k("dt")), int(k("L")),
                                         k("low"), k("high"), float(k("u")))
        assert acc == bool(k("acc")), i
        assert relmax(x, k("x_out")) < 1e-9 and abs(out[0] - float(k("U"))) < 1e-9 * abs(out[0])
        n += 1
    assert n == 8


def test_module_api_and_drop_in(G, orc):
    p = gold("potential_small.npz")
    gm = _module_small(G, p, fixed=True, grav_fix=p["gfix"])
    Aw, WmInv, Wm = gm.kernelw()
    assert Aw.shape == (42, 120) and relmax(np.asarray(Aw), p["Aw"]) < 1e-10
    assert relmax(Wm.diagonal(), p["wm"]) < 1e-11 and gm.mshape == tuple(p["shape"])
    assert relmax(WmInv @ (Wm @ np.arange(120.0)), np.arange(120.0)) < 1e-15
    x = p["xs"][1]
    for reg in ("Damping", "MS", "Smoothness", "TV"):
        out = gm.misfit_and_grad(x, p["mwapr"], None, None, 'mandatory', 1000, 0.7,
                                 regulization=reg, beta=0.001)
        assert abs(out[0] - p[reg + "_fix_misfit"][1]) < 1e-10 * abs(out[0])
        assert relmax(out[1], p[reg + "_fix_grad"][1]) < 1e-10
    with pytest.raises(ValueError):
        gm.misfit_and_grad(x, p["mwapr"], None, None, 'reflective', 1000, 0.7)
    with pytest.raises(ValueError):
        gm.misfit_and_grad(x, p["mwapr"], None, None, 'mandatory', 1000, 0.7, regulization="L1")
    # logarithmic constraint = logistic map on the host, same device evaluation
    lo, hi = -2.0 * p["wm"], 2.0 * p["wm"]
    xx = np.linspace(-0.003, 0.003, 120)
    mw = (lo + hi * np.e ** (1000 * xx)) / (1 + np.e ** (1000 * xx))
    a = gm.misfit_and_grad(xx, p["mwapr"], lo, hi, 'logarithmic', 1000, 0.7)
    b = gm.misfit_and_grad(mw, p["mwapr"], None, None, 'mandatory', 1000, 0.7)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


def test_chain_state_matches_stateless_and_is_deterministic(G):
    p = gold("potential_small.npz")
    gm = _module_small(G, p)
    eng = gm._engine
    wm = p["wm"]
    M = wm.size
    eng.set_reg("TV", 1.0, 0.001, p["shape"], 0.001 * wm)
    low, high = 0.0 * wm, 0.02 * wm
    rng = np.random.default_rng(11)
    trajs = [(rng.normal(size=M) * 0.3, int(rng.integers(5, 21)), float(rng.uniform())) for _ in range(12)]

    def run():
        eng.chain_init(0.001 * wm, low, high)
        out = []
        for p0, L, u in trajs:
            acc, o = eng.chain_trajectory(p0, 0.02, L, u)
            out.append((acc, o.copy(), eng.chain_get_x()))
        return out

    a, b = run(), run()
    n_acc = sum(t[0] for t in a)
    assert 0 < n_acc < len(trajs)                      # accept and reject both taken
    for (aa, ao, ax), (ba, bo, bx) in zip(a, b):
        assert aa == ba and np.array_equal(ao, bo) and np.array_equal(ax, bx)   # bitwise
    # the chain (device-resident state, cached evaluation) equals stateless gh_leapfrog calls
    x = 0.001 * wm
    for (p0, L, u), (acc, o, xs) in zip(trajs, a):
        x, acc2, o2, _ = eng.leapfrog(x, p0, 0.02, L, low, high, u)
        assert acc2 == acc and np.array_equal(x, xs) and np.array_equal(o2, o)


def test_hmcsample_end_to_end_small(G, tmp_path, capsys):
    """Whole chains against the reference's own runs (stdout lines + sample files)."""
    c = gold("chain_small.npz")
    p = gold("potential_small.npz")
    M = p["wm"].size
    for tag in ("a", "b"):
        dt, Sigma, lo, hi, n = c[tag + "_cfg"]
        gm = _module_small(G, p)
        folder = str(tmp_path / ("run_%s_chain" % tag))
        capsys.readouterr()
        G.HMCSample(gm, int(n), 0, float(dt), [5, 20], np.full(M, 0.001 + lo), np.full(M, 0.001),
                    np.c_[np.full(M, lo), np.full(M, hi)], "mandatory", 1000, p["dobs"],
                    "Fixed", 0.8, 1.0, str(c[tag + "_reg"]), 0.001, 100, float(Sigma), nbest=100,
                    myrank=0, save_folder=folder)
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("chain ")]
        ref_lines = [str(s) for s in c[tag + "_lines"]]
        assert len(lines) == len(ref_lines)               # same accept/reject sequence
        assert lines == ref_lines                         # 7 printed decimals, accept ratios
        mis = np.loadtxt(folder + "0/misfit.dat")
        mod = np.loadtxt(folder + "0/model.dat")
        np.testing.assert_allclose(mis, c[tag + "_misfit"], atol=2e-8, rtol=1e-9)
        np.testing.assert_allclose(mod, c[tag + "_model"], atol=2e-8)
        gm._engine.close()


def test_c1_chain_rows_and_posterior_stats(G, tmp_path, capsys):
    g = gold("c1_chain.npz")
    mesh, xp, yp, zp = c1_inputs()
    gm = G.GravMagModule(g["dobs"], (0, 2000, 0, 3000, 0, 1000), (100, 100, 100), (xp, yp, zp),
                         verbose=False)
    M = 6000
    folder = str(tmp_path / "c1_chain")
    G.HMCSample(gm, 5, 0, 0.01, [5, 20], np.full(M, 0.001), np.full(M, 0.001),
                np.c_[np.zeros(M), np.ones(M)], "mandatory", 1000, g["dobs"], "Fixed", 0.8, 1.0,
                "Damping", 0.001, 100, 0.001, save_folder=folder)
    capsys.readouterr()
    mis = np.loadtxt(folder + "0/misfit.dat")
    np.testing.assert_allclose(mis, g["misfit"], rtol=1e-8, atol=2e-8)
    mod = np.loadtxt(folder + "0/model.dat")
    np.testing.assert_allclose(mod[-1], g["model_last"], atol=2e-8)


def test_realdata_log_lines_on_gpu(G, tmp_path, capsys):
    """example/realdata/logout_T0.txt, chain 0: tesseroid assembly on the carved segment mesh,
    weighting, fixed cells, Damping and the trajectories all on the device."""
    e = gold("example_inputs.npz")
    obs, topo = e["real_obs"], e["real_topo"]
    gm = G.GravMagModule(obs[:, 3], (106.5, 118.5, 16, 28, 2000, -60000),
                         ([-1000, -2000, -5000], 0.5, 0.5), (obs[:, 0], obs[:, 1], obs[:, 2]),
                         fixed=True, grav_fix=e["real_gravsea"], mseg=True,
                         mdivisionsection=[2000, -5000, -15000, -60000], coordinate="spherical",
                         verbose=False, mtopo=(topo[:, 0], topo[:, 1], topo[:, 2]))
    assert gm.mshape == (21, 24, 24) and gm._engine.M == 10427
    keep = np.ones(gm.mesh.size, bool)
    keep[np.array(gm.mask)] = False
    M = 10427
    wm = gm.Wm.diagonal()
    np.testing.assert_allclose((0.01 * wm)[:3], e["real_T0_initial_mw_head"], rtol=5e-8)
    np.testing.assert_allclose((0.01 * wm)[-3:], e["real_T0_initial_mw_tail"], rtol=5e-8)
    capsys.readouterr()
    G.HMCSample(gm, 6, 0, 0.01, [5, 20], np.full(M, 0.01), e["real_aprior"][keep],
                np.c_[np.full(M, -0.5), np.full(M, 0.5)], "mandatory", 1000, obs[:, 3], "Fixed",
                0.8, 1.0, "Damping", 0.01, 100, 0.01, save_folder=str(tmp_path / "real_chain"))
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("chain 0")]
    import re
    pat = re.compile(r"=\(([-\d.]+),([-\d.]+),([-\d.]+),([-\d.]+)\)")
    got = np.array([[float(v) for v in pat.search(l).groups()] for l in lines])
    ref = e["real_T0_chain0"][:len(got)]
    np.testing.assert_allclose(got[:, [0, 1, 3]], ref[:, [0, 1, 3]], rtol=2e-9, atol=2e-7)


# ------------------------------------------------- BASELINE full size: size-independent laws

def _check_size_independent_laws(eng, mesh, reg, tag):
    """Laws that hold at any size (the oracle cannot run the full-size configs in seconds):
    linearity, adjoint consistency, superposition, unit column norms after weighting, gradient vs
    finite differences, bitwise reproducibility and the leapfrog's second order."""
    N, M = eng.N, eng.M
    rng = np.random.default_rng(0)
    x, y, r = rng.uniform(0, 1, M), rng.normal(size=M), rng.normal(size=N)
    # (1) linearity of the forward operator
    fx, fy = eng.forward(x), eng.forward(y)
    fz = eng.forward(2.5 * x - 0.75 * y)
    assert relmax(fz, 2.5 * fx - 0.75 * fy) < 1e-12
    # (2) adjoint consistency <G x, r> == <x, G^T r>
    gr = eng.adjoint(r)
    lhs, rhs = float(fx @ r), float(x @ gr)
    assert abs(lhs - rhs) <= 1e-11 * (np.abs(fx) @ np.abs(r))
    # (3) superposition over disjoint cell sets: layers 0..k and k+1.. add up to the whole
    top = np.zeros(M)
    top[: M // 2] = x[: M // 2]
    assert relmax(eng.forward(top) + eng.forward(x - top), fx) < 1e-12
    # (4) after weighting every column has unit 2-norm: ||Aw e_j|| == 1, and Aw (wm*x) == G x
    wm = eng.weight(0.5)
    assert (wm > 0).all()
    assert relmax(eng.forward(wm * x), fx) < 1e-12
    for j in (0, M // 3, M - 1):
        e = np.zeros(M)
        e[j] = 1.0
        assert abs(np.linalg.norm(eng.forward(e)) - 1.0) < 1e-12
    # (5) potential: finite-difference check of the gradient along a random direction, and a
    #     trajectory that must conserve H to O(dt^2) and be reproducible bit for bit
    dobs = fx + 0.02 * fx.max() * rng.normal(size=N)
    eng.set_data(dobs)
    eng.set_reg(reg, 1.0, 0.01, mesh.shape, 0.001 * wm)
    x0 = 0.001 * wm
    U0, g0, _, _, _ = eng.misfit_and_grad(x0)
    v = rng.normal(size=M)
    v /= np.linalg.norm(v)
    h = 1e-4
    Up = eng.misfit_and_grad(x0 + h * v)[0]
    Um = eng.misfit_and_grad(x0 - h * v)[0]
    assert abs((Up - Um) / (2 * h) - g0 @ v) < 1e-6 * abs(g0 @ v)
    low, high = -10.0 * wm, 10.0 * wm                 # wide bounds: no clamping below
    p0 = rng.normal(size=M) * 0.001
    eng.chain_init(x0, low, high)
    acc1, o1 = eng.chain_trajectory(p0, 0.001, 4, 0.5)
    x1 = eng.chain_get_x()
    eng.chain_init(x0, low, high)
    acc2, o2 = eng.chain_trajectory(p0, 0.001, 4, 0.5)
    assert acc1 == acc2 and np.array_equal(o1, o2) and np.array_equal(x1, eng.chain_get_x())
    # leapfrog is second order: halving dt at fixed trajectory length cuts the energy error ~4x
    eng.chain_init(x0, low, high)
    _, o3 = eng.chain_trajectory(p0, 0.0005, 8, 0.5)
    e1, e3 = abs(o1[4] - o1[3]), abs(o3[4] - o3[3])
    print("%s energy error dt=1e-3: %.4e  dt=5e-4: %.4e  ratio %.2f" % (tag, e1, e3, e1 / e3))
    assert 2.5 < e1 / e3 < 6.0


def test_c2_full_size_properties(G):
    """Config C2 (100x100x50 prisms, N = 10^4, M = 5*10^5, 40 GB G): the oracle cannot run
    this in seconds, so check laws that hold at any size."""
    nx = ny = 100
    nz = int(os.environ.get("GRAVHMC_TEST_C2_NZ", "50"))
    mesh = G.mesher.PrismMesh((0, 100.0 * nx, 0, 100.0 * ny, 0, 100.0 * nz), (100, 100, 100))
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 100.0 * ny, ny), np.linspace(0, 100.0 * nx, nx))]
    zp = np.zeros_like(xp)
    N, M = xp.size, mesh.size
    eng = G.Engine(N, M)
    eng.set_obs(xp, yp, zp)
    eng.set_cells(mesh.cell_bounds(), 0)
    eng.build_G()
    _check_size_independent_laws(eng, mesh, "Damping", "C2")
    eng.close()


def test_c5_per_gpu_share_full_size_properties(G):
    """Config C5 (200x200x60 prisms, N = 4*10^4, M = 2.4*10^6, G = 768 GB over 8 GPUs): the share
    ONE of the 8 GPUs holds (the first 3*10^5 cells, 96 GB of G, N above the 16384 rows a single
    workgroup keeps in registers), MS regulariser, through the laws that hold at any size."""
    nx = ny = 200
    frac = int(os.environ.get("GRAVHMC_TEST_C5_FRACTION", "8"))
    mesh = G.mesher.PrismMesh((0, 100.0 * nx, 0, 100.0 * ny, 0, 6000.0), (100, 100, 100))
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 100.0 * ny, ny), np.linspace(0, 100.0 * nx, nx))]
    zp = np.zeros_like(xp)
    bounds = mesh.cell_bounds()[: mesh.size // frac]
    N, M = xp.size, bounds.shape[0]
    assert N == 40000 and (frac != 8 or M == 300000)
    eng = G.Engine(N, M)
    eng.set_obs(xp, yp, zp)
    eng.set_cells(bounds, 0)
    eng.build_G()
    _check_size_independent_laws(eng, mesh, "MS", "C5 share")
    eng.close()


# ------------------------------------------------------------------ wavelet-compressed forward

@pytest.mark.parametrize("dims,shape", [(3, (19, 30, 30)), (3, (7, 9, 5)), (1, (1, 1, 1237)), (1, (1, 1, 16001))])
def test_wavelet_forward_one_launch_transform_is_bitwise_the_pass_per_launch_one(G, monkeypatch, dims, shape):
    """dwt_lds_kernel (the whole multi-level transform of a model vector in one launch, working block
    in LDS) against one launch per axis and level: same taps, same index arithmetic, same order of
    the products -> the same bits, odd lengths on both levels (the ratiogrid example's 19 x 30 x 30)
    and the 1-D variant included."""
    M = int(np.prod(shape))
    N = 23
    rng = np.random.default_rng(M)
    A = rng.normal(size=(N, M)) * np.exp(-np.arange(M) / (0.3 * M))[None, :]
    xs = [rng.normal(size=M) for _ in range(3)]
    out = {}
    monkeypatch.setenv("GRAVHMC_DWT_LDS_MAX", "20480")      # (by default only blocks <= 2048 take it)
    for mode in ("1", "0"):
        monkeypatch.setenv("GRAVHMC_DWT_LDS", mode)
        eng = G.Engine(N, M)
        eng.upload_G(A)
        eng.weight(0.5)
        eng.compress_wavelet(dims, shape if dims == 3 else None, 1e-3, 2)
        out[mode] = [eng.forward_wavelet(x) for x in xs] + [eng.model_coeffs(xs[0])]
        eng.close()
    for a, b in zip(out["1"], out["0"]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("dims,shape", [(3, (10, 30, 20)), (3, (7, 9, 5)), (3, (4, 6, 8)),
                                        (1, (1, 1, 6000)), (1, (1, 1, 1237))])
def test_wavelet_transform_and_csr_vs_oracle(G, dims, shape):
    """Device DWT (model and kernel rows), threshold and CSR against the numpy restatement of
    PyWavelets' db4/periodization transform (oracle/wavelet.py; pinned by the reference's logs)."""
    from oracle import wavelet as ow
    M = int(np.prod(shape))
    N = 37
    rng = np.random.default_rng(M)
    A = rng.normal(size=(N, M)) * np.exp(-np.arange(M) / (0.3 * M))[None, :]
    eng = G.Engine(N, M)
    eng.upload_G(A)
    eng.weight(0.5)
    Aw = eng.download_G()
    nnz, ncols = eng.compress_wavelet(dims, shape if dims == 3 else None, 1e-3, 2)
    x = rng.normal(size=M)
    co = ow.model_coeffs(x, dims, shape)
    assert ncols == co.size
    cg = eng.model_coeffs(x)
    assert relmax(cg, co) < 1e-14
    ref = ow.compress_kernel(Aw, dims, shape).toarray()
    got = eng.download_csr()
    assert got.has_sorted_indices or True
    got = got.toarray()
    # entries within rounding of the threshold may fall on either side
    edge = np.abs(np.abs(ow.wavedec3_packed(Aw, shape)[0] if dims == 3 else ow.wavedec1_packed(Aw)) - 1e-3) < 1e-12
    assert np.array_equal((got != 0) | edge, (ref != 0) | edge)
    assert np.abs(got - ref)[~edge].max() < 1e-14
    assert abs(nnz - (ref != 0).sum()) <= edge.sum()
    d = eng.forward_wavelet(x)
    assert relmax(d, ref @ co) < 1e-12
    eng.close()


def test_wavelet_potential_matches_reference_formulation(G, orc):
    """wavelet forward (thresholded CSR) + exact dense adjoint (potential.py:693-708)."""
    from oracle import wavelet as ow
    p = gold("potential_small.npz")
    gm = _module_small(G, p, wavelet='3D')
    shape = tuple(int(v) for v in p["shape"])
    Aw = np.asarray(gm.Aw)
    csr = gm.Awcp
    assert csr.shape == (42, ow.model_coeffs(np.zeros(120), 3, shape).size)
    x = p["xs"][1]
    for reg in ("MS", "TV"):
        out = gm.misfit_and_grad(x, p["mwapr"], None, None, 'mandatory', 1000, 0.7,
                                 regulization=reg, beta=0.001)
        P = orc.Problem(Aw, p["dobs"], p["mwapr"], reg, 0.7, 0.001, wm=gm.Wm.diagonal(), shape=shape,
                        csr=ow.compress_kernel(Aw, 3, shape), dwt=lambda v: ow.model_coeffs(v, 3, shape))
        ref = P.misfit_and_grad(x)
        assert abs(out[0] - ref[0]) < 1e-11 * abs(ref[0]) and relmax(out[1], ref[1]) < 1e-11
        assert relmax(out[2], ref[2]) < 1e-11


def test_uniformgrid_wavelet_log_lines_on_gpu(G, tmp_path, capsys):
    """example/uniformgrid/logout_T1.txt chains 0 and 1 (wavelet='3D', MS): the only pins of the
    PyWavelets convention the reference leaves (7 printed digits)."""
    e = gold("example_inputs.npz")
    obs = e["uni_obs"]
    M = 6000
    for rank, key in ((0, "uni_T1_chain0"), (1, "uni_T1_chain1")):
        gm = G.GravMagModule(obs[:, 3], (0, 2000, 0, 3000, 0, 1000), (100, 100, 100),
                             (obs[:, 0], obs[:, 1], obs[:, 2]), wavelet='3D', verbose=False)
        capsys.readouterr()
        G.HMCSample(gm, 8, 0, 0.01, [5, 20], np.full(M, 0.001), np.full(M, 0.001),
                    np.c_[np.zeros(M), np.ones(M)], "mandatory", 1000, obs[:, 3], "Fixed", 0.8, 1,
                    "MS", 0.001, 100, 0.001, myrank=rank, save_folder=str(tmp_path / "uni_chain"))
        import re
        pat = re.compile(r"=\(([-\d.]+),([-\d.]+),([-\d.]+),([-\d.]+)\)")
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("chain %d" % rank)]
        got = np.array([[float(v) for v in pat.search(l).groups()] for l in lines])
        ref = e[key][:len(got)]
        assert len(got) >= 8
        np.testing.assert_allclose(got[:, [0, 1, 3]], ref[:, [0, 1, 3]], rtol=0, atol=1.01e-7)
        gm._engine.close()


def test_segmentgrid_wavelet_log_lines_on_gpu(G, tmp_path, capsys):
    """example/segmentgrid/logout_T0.txt chain 0: segment mesh (dz 100/200/300), wavelet 3D, MS."""
    e = gold("example_inputs.npz")
    obs = e["seg_obs"]
    M = 6000
    gm = G.GravMagModule(obs[:, 3], (0, 2000, 0, 3000, 0, 2100), ([100, 200, 300], 100, 100),
                         (obs[:, 0], obs[:, 1], obs[:, 2]), mseg=True,
                         mdivisionsection=[0, 300, 900, 2100], wavelet='3D', verbose=False)
    capsys.readouterr()
    G.HMCSample(gm, 6, 0, 0.01, [5, 20], np.full(M, 0.001), np.full(M, 0.001),
                np.c_[np.zeros(M), np.ones(M)], "mandatory", 1000, obs[:, 3], "Fixed", 0.8, 1,
                "MS", 0.001, 100, 0.001, myrank=0, save_folder=str(tmp_path / "seg_chain"))
    import re
    pat = re.compile(r"=\(([-\d.]+),([-\d.]+),([-\d.]+),([-\d.]+)\)")
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("chain 0")]
    got = np.array([[float(v) for v in pat.search(l).groups()] for l in lines])
    np.testing.assert_allclose(got[:, [0, 1, 3]], e["seg_T0_chain0"][:len(got)][:, [0, 1, 3]],
                               rtol=0, atol=1.01e-7)


def test_speculative_chaining_is_bit_identical(G, monkeypatch):
    """gh_chain_prefetch_momentum (the next trajectory's first step rides on the last sweep)
    changes the execution order only: same bits as plain trajectories, through accepts and
    rejects, for the dense and the wavelet forward.  (Sweep-per-launch path: the resident chain
    kernel, which would take this small dense problem, is switched off.)"""
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    p = gold("potential_small.npz")
    for wavelet in (False, '3D'):
        gm = _module_small(G, p, wavelet=wavelet)
        eng = gm._engine
        wm = p["wm"]
        M = wm.size
        eng.set_reg("TV", 1.0, 0.001, p["shape"], 0.001 * wm)
        low, high = 0.0 * wm, 0.02 * wm
        rng = np.random.default_rng(5)
        trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, float(rng.uniform()))
                 for _ in range(20)]
        eng.chain_init(0.001 * wm, low, high)
        plain = []
        for L, p0, u in trajs:
            acc, o = eng.chain_trajectory(p0, 0.02, L, u)
            plain.append((acc, o.copy(), eng.chain_get_x()))
        assert 0 < sum(a for a, _, _ in plain) < len(trajs)
        eng.chain_init(0.001 * wm, low, high)
        before = eng.chain_stats()
        piped = []
        eng.run_chain(iter(trajs), 0.02, lambda L, acc, o, x: piped.append((acc, o.copy(), x)), want_x=True, batch=7)
        carried, last = [], 0.001 * wm          # x is only reported after accepted trajectories
        for a_, o_, x_ in piped:
            last = x_ if x_ is not None else last
            carried.append((a_, o_, last))
        piped = carried
        after = eng.chain_stats()
        assert after["spec_hits"] - before["spec_hits"] > 0
        assert after["spec_misses"] - before["spec_misses"] > 0       # rejected proposals
        assert len(piped) == len(plain)
        for (a1, o1, x1), (a2, o2, x2) in zip(plain, piped):
            assert a1 == a2 and np.array_equal(o1, o2) and np.array_equal(x1, x2)
        eng.close()


@pytest.mark.parametrize("resident", ["0", "1"])
def test_run_chain_overlap_keeps_the_stop_contract(G, monkeypatch, resident):
    """run_chain(overlap=True) starts the next batch before the finished one is handed to Python.
    With `stop_at_accepts` the library refuses the batch that was submitted ahead once the count is
    reached, also when it is reached on the last trajectory of a batch: same results, same final
    state and the same posterior window as without the overlap."""
    monkeypatch.setenv("GRAVHMC_RESIDENT", resident)
    p = gold("potential_small.npz")
    wm = p["wm"]
    M = wm.size
    rng = np.random.default_rng(31)
    trajs = [(int(rng.integers(1, 6)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(60)]
    for stop_at in (7, 8, 11):          # batch of 4: inside a batch, at its end, inside the next
        res = {}
        for overlap in (False, True):
            gm = _module_small(G, p)
            eng = gm._engine
            eng.set_reg("Damping", 1.0, 0.001, p["shape"], 0.001 * wm)
            eng.chain_init(0.001 * wm, 0.0 * wm, 0.02 * wm)
            eng.posterior_window(50)
            out = []

            def on_result(L, acc, o, x, out=out):
                out.append((acc, o.copy()))
                return sum(a_ for a_, _ in out) < stop_at

            eng.run_chain(iter(trajs), 0.02, on_result, stop_at_accepts=stop_at, batch=4, overlap=overlap)
            res[overlap] = (out, eng.chain_get_x(), eng.posterior_read()["total"])
            eng.close()
        (a, ax, an), (b, bx, bn) = res[False], res[True]
        assert sum(x[0] for x in a) == stop_at and an == bn == stop_at
        assert len(a) == len(b) and all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
        assert np.array_equal(ax, bx)


def test_two_contexts_share_a_kernel_instantiation(G):
    """The dynamic-LDS allowance is a property of the kernel, not of a context: a second context
    with a smaller request on the same sweep instantiation (N = 9000 and 10000: both 16-wave teams
    with five double2 per thread) must not take the first one's 80 KB away."""
    rng = np.random.default_rng(4)
    engs = []
    for N in (10000, 9000):
        A = np.asfortranarray(rng.normal(size=(N, 96)))
        e = G.Engine(N, 96)
        e.upload_G(A)
        engs.append((e, A))
    for e, A in engs + engs[::-1]:
        x = rng.normal(size=96)
        assert relmax(e.forward(x), A @ x) < 1e-13
    for e, _ in engs:
        e.close()


# ------------------------------------------------------------ resident chain kernel

@pytest.mark.parametrize("reg", ["Damping", "MS", "Smoothness", "TV"])
def test_resident_chain_kernel_matches_sweep_path(G, monkeypatch, reg):
    """Small dense problems run whole batches of trajectories inside one cooperative launch with
    G resident in LDS (csrc/resident.hip.h).  Same chain as the sweep-per-launch path through
    accepts and rejects (decisions identical, energies/models to 1e-12: the summation order over
    the cells differs), for every regulariser, with and without the fixed field; plus the
    stop-at-accepts contract, the accepted-model output and the posterior ring."""
    p = gold("potential_small.npz")
    wm = p["wm"]
    M = wm.size
    rng = np.random.default_rng(5)
    sigma = 0.02 if reg == "MS" else 0.3
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * sigma, float(rng.uniform())) for _ in range(40)]
    for fix in (False, True):
        res = {}
        for mode in ("0", "1"):
            monkeypatch.setenv("GRAVHMC_RESIDENT", mode)
            gm = _module_small(G, p, fixed=True, grav_fix=p["gfix"]) if fix else _module_small(G, p)
            eng = gm._engine
            eng.set_reg(reg, 1.0, 0.001, p["shape"], 0.001 * wm)
            eng.chain_init(0.001 * wm, 0.0 * wm, 0.02 * wm)
            eng.posterior_window(8)
            out = []
            eng.run_chain(iter(trajs), 0.02, lambda L, acc, o, x: out.append((acc, o.copy(), x)),
                          want_x=True, batch=7, record_from=3)
            st = eng.chain_stats()
            res[mode] = (out, eng.chain_get_x(), eng.chain_get_dsyn(), eng.posterior_read(), st)
            # a second call continues the chain from the device state; stops at the accept count
            more = []
            n_acc = sum(a_ for a_, _, _ in out)
            eng.run_chain(iter(trajs), 0.02, lambda L, acc, o, x: more.append(acc), batch=16,
                          stop_at_accepts=n_acc + 3)
            res[mode] += (more,)
            eng.close()
        (a, ax, ad, ap, ast, am), (b, bx, bd, bp, bst, bm) = res["0"], res["1"]
        assert ast["spec_hits"] > 0 and bst["spec_hits"] == 0       # the two paths were really taken
        assert len(a) == len(b) == len(trajs)
        n_acc = sum(t[0] for t in a)
        assert 0 < n_acc and (reg != "TV" or n_acc < len(trajs))
        for (a1, o1, x1), (a2, o2, x2) in zip(a, b):
            assert a1 == a2
            assert np.abs(o1 - o2).max() <= 1e-12 * np.abs(o1).max()
            assert (x1 is None) == (x2 is None)
            if x1 is not None:
                assert relmax(x2, x1) < 1e-12
        assert relmax(bx, ax) < 1e-12 and relmax(bd, ad) < 1e-12
        assert ap["total"] == bp["total"] == max(0, n_acc - 3)
        if ap["total"]:
            assert relmax(bp["mean"], ap["mean"]) < 1e-12
        assert am == bm and (reg == "MS" or (sum(bm) == 3 and bm[-1]))


@pytest.mark.parametrize("wavelet", ["1D", "3D"])
def test_resident_chain_kernel_with_wavelet_forward(G, monkeypatch, wavelet):
    """Wavelet-compressed forward inside the resident kernel: LDS holds the dense model-space form
    F = Awcp W of the compressed operator (column j = compressed forward of the unit model e_j,
    thresholding included), the dots read Aw from their register copy.  Same chain as the
    sweep path's DWT + SpMV to rounding, and F itself against gh_forward_wavelet."""
    p = gold("potential_small.npz")
    wm = p["wm"]
    M = wm.size
    rng = np.random.default_rng(21)
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(30)]
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("GRAVHMC_RESIDENT", mode)
        gm = _module_small(G, p, wavelet=wavelet)
        eng = gm._engine
        eng.set_reg("TV", 1.0, 0.001, p["shape"], 0.001 * wm)
        eng.chain_init(0.001 * wm, 0.0 * wm, 0.02 * wm)
        out = []
        eng.run_chain(iter(trajs), 0.02, lambda L, acc, o, x: out.append((acc, o.copy(), x)), want_x=True, batch=8)
        res[mode] = (out, eng.chain_get_x(), eng.chain_get_dsyn(), eng.chain_stats()["resident_launches"])
        eng.close()
    (a, ax, ad, la), (b, bx, bd, lb) = res["0"], res["1"]
    assert la == 0 and lb > 0
    n_acc = sum(t[0] for t in a)
    assert 0 < n_acc < len(trajs)
    for (a1, o1, x1), (a2, o2, x2) in zip(a, b):
        assert a1 == a2 and np.abs(o1 - o2).max() <= 1e-11 * np.abs(o1).max()
        assert (x1 is None) == (x2 is None) and (x1 is None or relmax(x2, x1) < 1e-11)
    assert relmax(bx, ax) < 1e-11 and relmax(bd, ad) < 1e-11


@pytest.mark.parametrize("N,M", [(1, 1), (2, 7), (15, 8), (16, 9), (17, 255), (100, 256), (257, 257),
                                 (1000, 1000), (1024, 3000), (64, 20000), (333, 4099),
                                 (625, 10427), (1024, 6000), (1000, 5000)])
def test_resident_chain_kernel_shapes(G, monkeypatch, N, M):
    """Edge shapes of the resident kernel's partition (fewer workgroups than clusters, one-cell
    workgroups, ragged last workgroup, row chunks of more than 32 rows, N at its limit) and, last
    three, kernels larger than the LDS (52, 49, 40 MB: one copy split between the waves' registers
    and LDS): same chain as the sweep path."""
    rng = np.random.default_rng(N * 100003 + M)
    A = np.asfortranarray(rng.normal(size=(N, M)) * rng.uniform(0.2, 2.0, size=M))
    dobs = rng.normal(size=N) * 3
    trajs = [(int(rng.integers(1, 6)), rng.normal(size=M) * 0.05, float(rng.uniform())) for _ in range(9)]
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("GRAVHMC_RESIDENT", mode)
        e = G.Engine(N, M)
        e.upload_G(A)
        w = e.weight(0.5)
        e.set_data(dobs)
        if (N, M) == (1000, 5000):          # one-copy mode with a stencil regulariser
            e.set_reg("TV", 0.7, 0.01, (10, 20, 25), 0.001 * w)
        else:
            e.set_reg("MS", 0.7, 0.01, None, 0.001 * w)
        e.chain_init(0.002 * w, 0.0 * w, 0.5 * w)
        out = []
        e.run_chain(iter(trajs), 0.01, lambda L, acc, o, x: out.append((acc, o.copy())), batch=4)
        res[mode] = (out, e.chain_get_x(), e.chain_stats()["resident_launches"])
        e.close()
    (a, ax, la), (b, bx, lb) = res["0"], res["1"]
    assert la == 0 and lb > 0
    assert len(a) == len(b) == len(trajs)
    for (a1, o1), (a2, o2) in zip(a, b):
        assert a1 == a2 and np.abs(o1 - o2).max() <= 1e-11 * np.abs(o1).max()
    assert relmax(bx, ax) < 1e-11


@pytest.mark.parametrize("switch", ["GRAVHMC_RESIDENT_LOCAL", "GRAVHMC_RESIDENT_REGS"])
@pytest.mark.parametrize("reg", ["Damping", "TV"])
def test_resident_chain_kernel_fallback_forms(G, monkeypatch, switch, reg):
    """The two forms of the resident kernel a placement or a shape can force: cluster-internal data
    written through to memory instead of kept in the XCD's L2 (what the kernel does when the
    workgroups of a cluster do not report the same XCC id), and the dots reading the columns from
    LDS instead of a register copy.  Bit for bit the chain of the default form (the reduction order is
    defined by logical indices only)."""
    p = gold("potential_small.npz")
    wm = p["wm"]
    M = wm.size
    rng = np.random.default_rng(77)
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(16)]
    res = {}
    for val in ("1", "0"):
        monkeypatch.setenv("GRAVHMC_RESIDENT", "1")
        monkeypatch.setenv(switch, val)
        gm = _module_small(G, p)
        eng = gm._engine
        eng.set_reg(reg, 1.0, 0.001, p["shape"], 0.001 * wm)
        eng.chain_init(0.001 * wm, 0.0 * wm, 0.02 * wm)
        out = []
        eng.run_chain(iter(trajs), 0.02, lambda L, acc, o, x: out.append((acc, o.copy())), batch=5)
        res[val] = (out, eng.chain_get_x(), eng.chain_stats()["resident_launches"])
        eng.close()
    (a, ax, la), (b, bx, lb) = res["1"], res["0"]
    assert la > 0 and lb > 0
    assert 0 < sum(t[0] for t in a)
    for (a1, o1), (a2, o2) in zip(a, b):
        assert a1 == a2 and np.array_equal(o1, o2)
    assert np.array_equal(ax, bx)


def test_resident_chain_kernel_leaves_wide_stencil_shapes_to_the_sweep_path(G, monkeypatch):
    """Smoothness / TV take one thread per (cell, neighbour) in the resident kernel: with more than 85
    cells per workgroup (few observations, many cells) such a chain runs on the sweep path -- same
    results as with the kernel switched off -- while a cell-local regulariser on the same context
    uses the resident kernel."""
    N, M, shape = 64, 24000, (10, 40, 60)       # 94 cells per workgroup
    rng = np.random.default_rng(4242)
    A = np.asfortranarray(rng.normal(size=(N, M)) * rng.uniform(0.2, 2.0, size=M))
    dobs = rng.normal(size=N) * 3
    trajs = [(int(rng.integers(1, 5)), rng.normal(size=M) * 0.05, float(rng.uniform())) for _ in range(6)]
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("GRAVHMC_RESIDENT", mode)
        e = G.Engine(N, M)
        e.upload_G(A)
        w = e.weight(0.5)
        e.set_data(dobs)
        e.set_reg("TV", 0.7, 0.01, shape, 0.001 * w)
        e.chain_init(0.002 * w, 0.0 * w, 0.5 * w)
        out = []
        e.run_chain(iter(trajs), 0.01, lambda L, acc, o, x: out.append((acc, o.copy())), batch=3)
        launches_tv = e.chain_stats()["resident_launches"]
        x_tv = e.chain_get_x()
        e.set_reg("Damping", 0.7, 0.01, None, 0.001 * w)
        e.chain_init(0.002 * w, 0.0 * w, 0.5 * w)
        e.run_chain(iter(trajs), 0.01, lambda L, acc, o, x: None, batch=3)
        res[mode] = (out, x_tv, launches_tv, e.chain_stats()["resident_launches"])
        e.close()
    (a, ax, la_tv, la_d), (b, bx, lb_tv, lb_d) = res["0"], res["1"]
    assert la_tv == 0 and la_d == 0
    assert lb_tv == 0 and lb_d > 0
    for (a1, o1), (a2, o2) in zip(a, b):
        assert a1 == a2 and np.array_equal(o1, o2)
    assert np.array_equal(ax, bx)


def test_resident_chain_kernel_times_out_cleanly(G, monkeypatch, capfd):
    """Every wait inside the resident kernel is bounded.  With the test hook the workgroups wait for
    partners that never run: the kernel gives up after 2 s without touching the chain and the batch
    is run on the sweep-per-launch path (same bits).  A transient stall does not downgrade the
    context: the next batch runs on the resident kernel again; three aborted launches do."""
    p = gold("potential_small.npz")
    wm = p["wm"]
    M = wm.size
    rng = np.random.default_rng(9)
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(12)]
    res = {}
    for mode in ("sweep", "transient", "aborting"):
        monkeypatch.setenv("GRAVHMC_RESIDENT", "0" if mode == "sweep" else "1")
        monkeypatch.setenv("GRAVHMC_RESIDENT_TEST_ABORT", "0" if mode == "sweep" else "1")
        gm = _module_small(G, p)
        eng = gm._engine
        eng.set_reg("TV", 1.0, 0.001, p["shape"], 0.001 * wm)
        eng.chain_init(0.001 * wm, 0.0 * wm, 0.02 * wm)
        out = []
        cb = lambda L, acc, o, x: out.append((acc, o.copy()))
        if mode == "transient":
            eng.run_chain(iter(trajs[:5]), 0.02, cb, batch=5)        # one aborted launch
            assert eng.chain_stats()["resident_launches"] == 0
            monkeypatch.setenv("GRAVHMC_RESIDENT_TEST_ABORT", "0")
            eng.run_chain(iter(trajs[5:]), 0.02, cb, batch=5)        # the stall is over
            assert eng.chain_stats()["resident_launches"] == 2
        else:
            eng.run_chain(iter(trajs), 0.02, cb, batch=4)            # three aborted launches
            if mode == "aborting":
                assert eng.chain_stats()["resident_launches"] == 0
        res[mode] = (out, eng.chain_get_x())
        eng.close()
    err = capfd.readouterr().err
    assert err.count("timed out") == 4 and "(3 of 3); continuing for good" in err
    (a, ax), (b, bx) = res["sweep"], res["aborting"]
    assert len(a) == len(b) == len(trajs)
    for (a1, o1), (a2, o2) in zip(a, b):
        assert a1 == a2 and np.array_equal(o1, o2)
    assert np.array_equal(ax, bx)
    # resident and sweep path agree to rounding, with identical decisions
    (t, tx) = res["transient"]
    assert len(t) == len(trajs)
    for (a1, o1), (a2, o2) in zip(a, t):
        assert a1 == a2 and np.allclose(o1, o2, rtol=1e-10, atol=0)
    assert relmax(tx, ax) < 1e-10


# ------------------------------------------------------------ one chain sharded over GPUs

def test_sharded_engine_rccl_world1_is_bitwise_unsharded(G, monkeypatch):
    """RCCL plumbing (unique id, ncclCommInitRank, ncclAllReduce on the stream) with a
    one-rank communicator: the sharded code path must reproduce the unsharded bits."""
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")   # bitwise comparison of the two sweep-per-launch paths
    from gravinv3dhmc_amd.dist import Ranks, make_sharded_engine
    p = gold("potential_small.npz")
    env = {k: os.environ.pop(k, None) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    try:
        ranks = Ranks()
    finally:
        for k, v in env.items():
            if v is not None:
                os.environ[k] = v
    wm = p["wm"]
    M = wm.size

    def setup(eng):
        eng.upload_G(np.asarray(p["Aw"]) * wm[None, :])      # unweighted kernel back
        w = eng.weight(0.5)
        eng.set_data(p["dobs"])
        eng.set_reg("MS", 1.0, 0.001, p["shape"], 0.001 * w)
        eng.chain_init(0.001 * w, 0.0 * w, 0.02 * w)
        return w

    a = make_sharded_engine(42, M, ranks, device=0, backend="rccl")
    b = G.Engine(42, M)
    wa, wb = setup(a), setup(b)
    assert np.array_equal(wa, wb)
    rng = np.random.default_rng(2)
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(10)]
    ra, rb = [], []
    a.run_chain(iter(trajs), 0.02, lambda L, acc, o, x: ra.append((acc, o.copy(), x)), want_x=True)
    b.run_chain(iter(trajs), 0.02, lambda L, acc, o, x: rb.append((acc, o.copy(), x)), want_x=True, batch=3)
    for (a1, o1, x1), (a2, o2, x2) in zip(ra, rb):
        assert a1 == a2 and np.array_equal(o1, o2)
        assert (x1 is None) == (x2 is None) == (not a1) and (x1 is None or np.array_equal(x1, x2))
    x = rng.uniform(0, 1, M) * wb
    assert np.array_equal(a.forward(x), b.forward(x))
    ma, mb = a.misfit_and_grad(x), b.misfit_and_grad(x)
    assert ma[0] == mb[0] and np.array_equal(ma[1], mb[1])
    # the stencil kinds take the halo path (here: no neighbours, second all-reduce for R)
    for reg in ("Smoothness", "TV"):
        a.set_reg(reg, 1.0, 0.001, p["shape"], 0.001 * wb)
        b.set_reg(reg, 1.0, 0.001, p["shape"], 0.001 * wb)
        ma, mb = a.misfit_and_grad(x), b.misfit_and_grad(x)
        assert abs(ma[0] - mb[0]) <= 1e-13 * abs(mb[0]) and relmax(ma[1], mb[1]) < 1e-13
    a.close()
    b.close()


def test_sharded_chain_three_ranks_one_gpu():
    """Three ranks (one process each, all on GPU 0) hold 4 + 3 + 3 of the 10 z-planes of the C1
    model; forward partials are summed over gloo once per evaluation, and for Smoothness/TV the
    boundary planes of the model travel with them (the stencil crosses the shard boundaries).
    Everything must agree with the unsharded engine to rounding for all four regularisers and all
    ranks must print the same chain; shards that cut through a plane refuse the stencil kinds."""
    import json
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "shard_worker.py"), "gloo"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert [r["rank"] for r in res] == [0, 1, 2] and [r["M_local"] for r in res] == [2400, 1800, 1800]
    assert [r["M_ragged"] for r in res] == [2000, 2000, 2000]
    for r in res:
        assert r["wm"] == 0.0                     # column norms are per cell: identical bits
        assert r["fwd"] < 1e-13 and r["adj"] == 0.0 and r["potential"] < 1e-12
        assert r["tv_refused"]
        assert r["lines_equal"] and r["misfit"] < 1e-9 and r["model"] < 2e-8
        assert r["tv_lines_equal"] and r["tv_misfit"] < 1e-9 and r["tv_model"] < 2e-8
        assert r["ref_rows"] < 1e-7               # and they are the reference's rows (8 decimals)
        assert r["spec"]["spec_hits"] > 0
        # regulariser cache keyed by content: no re-send for fresh temporaries, one after an edit
        assert r["resends_equal_content"] == 0 and r["resends_after_edit"] == 1 and r["edit_potential"] < 1e-12
        # batches of two through run_chain(overlap=True): nothing overlaps over gloo, same chain
        assert r["overlap_n"] == 9 and r["overlap_decisions"] and r["overlap_out5"] < 1e-9 and r["overlap_x"] < 1e-9
    print("sharded 3-rank check:", res[0])


def test_sharded_chain_rccl_one_gpu_per_rank():
    """The RCCL transport with more than one rank (ncclAllReduce over xGMI on the context streams):
    two ranks, one GPU each, the same checks as the gloo run above -- identical chain lines on all
    ranks, agreement with the unsharded engine.  Needs two GPUs: skipped on the 1-GPU boxes the suite
    normally runs on (multi-rank RCCL is then UNVERIFIED ON HARDWARE)."""
    import json
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    import ctypes
    # (not torch.cuda.device_count(): torch brings its own HIP runtime, and two of them in the
    # process that holds libgravhmc contexts corrupt the heap at exit)
    ndev = ctypes.c_int(0)
    ctypes.CDLL("libamdhip64.so").hipGetDeviceCount(ctypes.byref(ndev))
    if ndev.value < 2:
        pytest.skip("needs two GPUs (multi-rank RCCL cannot run on one)")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "shard_worker.py"), "rccl", "one-gpu-per-rank"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert [r["rank"] for r in res] == [0, 1] and [r["M_local"] for r in res] == [3000, 3000]
    for r in res:
        assert r["wm"] == 0.0 and r["fwd"] < 1e-13 and r["adj"] == 0.0 and r["potential"] < 1e-12
        assert r["lines_equal"] and r["misfit"] < 1e-9 and r["model"] < 2e-8
        assert r["tv_lines_equal"] and r["tv_misfit"] < 1e-9 and r["tv_model"] < 2e-8
        assert r["overlap_n"] == 9 and r["overlap_decisions"] and r["overlap_out5"] < 1e-9


# ------------------------------------------------------------------------------ matrix-free

def test_matrix_free_prism_matches_dense(G):
    """gh_set_matrix_free: entries re-evaluated in every pass instead of read from HBM; same
    potential, gradient and chain as the dense engine (<= 1e-12: summation order differs)."""
    p = gold("potential_small.npz")
    dense = _module_small(G, p)
    mf = _module_small(G, p, matrix_free=True)
    assert relmax(mf.Wm.diagonal(), dense.Wm.diagonal()) < 1e-13
    wm = dense.Wm.diagonal()
    x = p["xs"][1]
    with pytest.raises(ValueError):
        np.asarray(mf.Aw)                                 # nothing to copy back
    assert relmax(mf._engine.forward(x), dense._engine.forward(x)) < 1e-12
    r = np.random.default_rng(0).normal(size=42)
    assert relmax(mf._engine.adjoint(r), dense._engine.adjoint(r)) < 1e-12
    for reg in ("Damping", "MS", "TV"):
        a = mf.misfit_and_grad(x, p["mwapr"], None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        b = dense.misfit_and_grad(x, p["mwapr"], None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        assert abs(a[0] - b[0]) < 1e-12 * abs(b[0]) and relmax(a[1], b[1]) < 1e-11
    rng = np.random.default_rng(4)
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=120) * 0.3, float(rng.uniform())) for _ in range(8)]
    outs = []
    for m in (mf, dense):
        e = m._engine
        e.set_reg("TV", 1.0, 0.001, p["shape"], 0.001 * wm)
        e.chain_init(0.001 * wm, 0.0 * wm, 0.02 * wm)
        res = []
        e.run_chain(iter(trajs), 0.02, lambda L, acc, o, x, res=res: res.append((acc, o.copy(), x)), want_x=True)
        outs.append(res)
    for (a1, o1, x1), (a2, o2, x2) in zip(*outs):
        assert a1 == a2 and relmax(o1, o2) < 1e-10 and (x1 is None or relmax(x1, x2) < 1e-10)


@pytest.mark.parametrize("exact", ["1", "0"])
def test_matrix_free_tesseroid_and_many_rows(G, orc, monkeypatch, exact):
    """Matrix-free tesseroid entries against the dense engine and the reference's values.  exact=1:
    the root leaf in the reference's operation order (1e-12: summation order only); exact=0, the
    default: the root leaf re-arranged for throughput (addition theorem for cos(lon - lon'), rsq^3
    for 1/l^3) -- within the path's stated 1e-10, measured ~1e-14."""
    monkeypatch.setenv("GRAVHMC_MF_EXACT", exact)
    tol = 1e-12 if exact == "1" else 1e-10
    g = gold("tess_cases.npz")
    N, M = g["lon"].size, g["bounds"].shape[0]
    dense, mf = G.Engine(N, M), G.Engine(N, M)
    mf.set_matrix_free(True)
    for e in (dense, mf):
        e.set_obs(g["lon"], g["lat"], g["h"])
        e.set_cells(g["bounds"], 1, 1.6)
        e.build_G()
    assert np.abs((mf.forward(g["rho"]) - g["gz"]) / g["gz"]).max() < 1e-10     # unweighted forward
    wd, wmf = dense.weight(0.5), mf.weight(0.5)
    assert relmax(wmf, wd) < 1e-13
    x = g["rho"] * wd
    ef, ea = relmax(mf.forward(x), dense.forward(x)), 0.0
    r = np.random.default_rng(1).normal(size=N)
    ea = relmax(mf.adjoint(r), dense.adjoint(r))
    print("matrix-free tesseroid (exact=%s): forward %.2e adjoint %.2e, near-field table %r"
          % (exact, ef, ea, mf.matrix_free_stats()))
    assert ef < tol and ea < tol
    dense.close()
    mf.close()
    if exact == "0":
        return
    # more observations than the dense sweep holds in registers: matrix-free still works
    N2 = 20000
    rng = np.random.default_rng(2)
    xp, yp = rng.uniform(0, 2000, N2), rng.uniform(0, 3000, N2)
    zp = np.zeros(N2)
    mesh = G.mesher.PrismMesh((0, 2000, 0, 3000, 0, 1000), (500, 1000, 1000))
    b = mesh.cell_bounds()
    M2 = b.shape[0]
    e = G.Engine(N2, M2)
    e.set_matrix_free(True)
    e.set_obs(xp, yp, zp)
    e.set_cells(b, 0)
    e.build_G()
    K = orc.prism_gz_kernel(xp, yp, zp, b)
    rho = rng.uniform(0, 1, M2)
    assert relmax(e.forward(rho), K @ rho) < 1e-11
    wm = e.weight(0.5)
    assert relmax(wm, np.sqrt((K ** 2).sum(0))) < 1e-12
    r = rng.normal(size=N2)
    assert relmax(e.adjoint(r), (K / wm).T @ r) < 1e-11
    e.close()


# ----------------------------------------------------------- sample sink / posterior statistics

def test_posterior_window_and_sample_sinks(G, orc, tmp_path, capsys):
    """Device-side ring of accepted models against np.mean/np.std over the tail of model.dat
    (plot_uniform.py:44-55,103-104); binary and 'none' sinks; RMSD / RMSM (plot_uniform.py:152-153)."""
    from gravinv3dhmc_amd import posterior
    p = gold("potential_small.npz")
    M = p["wm"].size
    args = lambda: (np.full(M, 0.001), np.full(M, 0.001), np.c_[np.zeros(M), np.ones(M)], "mandatory",
                    1000, p["dobs"], "Fixed", 0.8, 1.0, "Damping", 0.001, 100, 0.001)
    runs = {}
    for sink in ("text", "binary", "none"):
        gm = _module_small(G, p)
        folder = str(tmp_path / ("sink_%s_chain" % sink))
        G.HMCSample(gm, 14, 2, 0.01, [5, 20], *args(), save_folder=folder, sample_sink=sink,
                    posterior_last=10)
        runs[sink] = (gm, folder + "0")
    capsys.readouterr()
    gm, folder = runs["text"]
    rows = np.loadtxt(folder + "/model.dat")
    assert rows.shape == (14, M)                       # ndraws = 2 burn-in samples are not written
    st = gm._engine.posterior_read()
    assert st["n"] == 10 and st["total"] == 14
    mean, sd, n = posterior.stats_from_file(folder + "/model.dat", last=10)
    np.testing.assert_allclose(st["mean"], mean, atol=1e-8)
    np.testing.assert_allclose(st["std"], sd, atol=1e-8)
    # binary sink: same models without the text formatting, same device statistics
    gmb, fb = runs["binary"]
    raw = np.fromfile(fb + "/model.bin").reshape(-1, M)
    np.testing.assert_allclose(raw, rows, atol=5.1e-9)
    assert not os.path.exists(fb + "/model.dat")
    stb = gmb._engine.posterior_read()
    assert np.array_equal(stb["mean"], st["mean"]) and np.array_equal(stb["std"], st["std"])
    gmn, fn = runs["none"]
    assert not os.path.exists(fn + "/model.dat") and not os.path.exists(fn + "/model.bin")
    assert np.array_equal(gmn._engine.posterior_read()["mean"], st["mean"])
    assert np.loadtxt(fn + "/misfit.dat").shape == (14, 7)
    # summary numbers
    rho_true = np.zeros(M)
    rho_true[40:50] = 1.0
    sm = posterior.summarize(gm, p["dobs"], rho_true)
    Aw = np.asarray(gm.Aw)
    d_mean = Aw @ (gm.Wm.diagonal() * st["mean"])
    assert abs(sm["RMSD"] - np.sqrt(np.linalg.norm(p["dobs"] - d_mean) ** 2 / 42)) < 1e-12
    assert abs(sm["RMSM"] - np.sqrt(np.linalg.norm(rho_true - st["mean"]) ** 2 / M)) < 1e-15


# --------------------------------------------------------- several chains per GPU (fp64 MFMA)

@pytest.mark.parametrize("case,resident", [("small_tv", "0"), ("small_tv", "1"), ("random_ms", "0"),
                                           ("random_ms", "1"), ("random_damping_big", "1"),
                                           ("small_tv_wavelet", "1")])
def test_batched_chains_match_single_chain_engines(G, monkeypatch, case, resident):
    """gh_batch_*: up to 16 chains share every sweep of G through v_mfma_f64_16x16x4 -- or, on
    problems small enough for the resident chain kernel (resident = "1": the first two cases),
    take turns inside one launch of that kernel per round of trajectories.  Every chain must
    reproduce a single-chain context fed the same momenta / lengths / variates (<= 1e-10: the
    MFMA contracts rows in another order than the wave reduction)."""
    monkeypatch.setenv("GRAVHMC_RESIDENT", resident)
    rng = np.random.default_rng(11)
    if case in ("small_tv", "small_tv_wavelet"):
        p = gold("potential_small.npz")
        A, dobs, shape, reg, beta = np.asarray(p["Aw"]) * p["wm"][None, :], p["dobs"], p["shape"], "TV", 0.001
        C, dt, sig, hi, ntraj = 5, 0.02, 0.3, 0.02, 6
    elif case == "random_ms":
        N, M = 1000, 700
        A = np.asfortranarray(rng.normal(size=(N, M)) * rng.uniform(0.1, 3, size=M))
        dobs, shape, reg, beta = rng.normal(size=N) * 5, (7, 10, 10), "MS", 0.01
        C, dt, sig, hi, ntraj = 16, 0.01, 0.05, 0.3, 3
    else:
        N, M = 5003, 1234
        A = np.asfortranarray(rng.normal(size=(N, M)))
        dobs, shape, reg, beta = rng.normal(size=N) * 20, (1, 1, M), "Damping", 0.01
        C, dt, sig, hi, ntraj = 3, 0.004, 0.02, 0.5, 2
    N, M = A.shape

    def make():
        e = G.Engine(N, M)
        e.upload_G(A)
        w = e.weight(0.5)
        e.set_data(dobs)
        e.set_reg(reg, 1.0, beta, shape, 0.001 * w)
        if case == "small_tv_wavelet":      # compressed forward: only the resident kernel batches it
            e.compress_wavelet(3, shape, 1e-3, 2)
        return e, w

    eb, wm = make()
    low, high = 0.0 * wm, hi * wm
    x0s = np.stack([(0.001 + 0.002 * c) * wm for c in range(C)])
    eb.batch_init(x0s, low, high)
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")     # the single-chain contexts: sweep path
    if case == "small_tv_wavelet":
        en, _ = make()
        with pytest.raises(NotImplementedError):    # (no compressed forward in the MFMA batch)
            en.batch_init(x0s, low, high)
        en.close()
    singles = []
    for c in range(C):
        e, _ = make()
        e.chain_init(x0s[c], low, high)
        singles.append(e)
    n_acc = n_rej = 0
    for it in range(ntraj):
        Ls = rng.integers(1, 9, size=C)
        p0s = rng.normal(size=(C, M)) * sig
        us = rng.uniform(size=C)
        acc, out5 = eb.batch_trajectory(p0s, dt, Ls, us)
        for c in range(C):
            a1, o1 = singles[c].chain_trajectory(p0s[c], dt, int(Ls[c]), float(us[c]))
            assert a1 == acc[c], (case, it, c, o1, out5[c])
            assert relmax(out5[c], o1) < 1e-10, (case, it, c, out5[c], o1)
            assert relmax(eb.batch_get_x(c), singles[c].chain_get_x()) < 1e-10
            n_acc += a1
            n_rej += not a1
    assert n_acc > 0
    if case in ("small_tv", "small_tv_wavelet"):
        assert n_rej > 0
    took_resident = eb.chain_stats()["resident_launches"] > 0
    assert took_resident == (resident == "1" and case != "random_damping_big")
    for e in singles + [eb]:
        e.close()


@pytest.mark.parametrize("case,resident", [("small_tv", "0"), ("small_tv", "1"), ("random_damping_big", "1")])
def test_batch_run_desynchronised_chains_match_lockstep_rounds(G, monkeypatch, case, resident):
    """gh_batch_run: T trajectories per chain in one call, every chain starting its next trajectory
    in the sweep after it finished the previous one (the others are in the middle of theirs).  Each
    chain must compute what it computes in lock-step rounds of gh_batch_trajectory, including the
    states reported after accepted trajectories."""
    monkeypatch.setenv("GRAVHMC_RESIDENT", resident)
    rng = np.random.default_rng(17)
    if case == "small_tv":
        p = gold("potential_small.npz")
        A, dobs, shape, reg, beta = np.asarray(p["Aw"]) * p["wm"][None, :], p["dobs"], p["shape"], "TV", 0.001
        C, T, dt, sig, hi = 5, 4, 0.02, 0.3, 0.02
    else:
        N, M = 5003, 1234
        A = np.asfortranarray(rng.normal(size=(N, M)))
        dobs, shape, reg, beta = rng.normal(size=N) * 20, (1, 1, M), "Damping", 0.01
        C, T, dt, sig, hi = 3, 3, 0.004, 0.02, 0.5
    N, M = A.shape

    def make():
        e = G.Engine(N, M)
        e.upload_G(A)
        w = e.weight(0.5)
        e.set_data(dobs)
        e.set_reg(reg, 1.0, beta, shape, 0.001 * w)
        return e, w

    Ls = rng.integers(1, 9, size=(C, T))
    ea, wm = make()
    p0s = rng.normal(size=(C, T, M)) * sig
    us = rng.uniform(size=(C, T))
    low, high = 0.0 * wm, hi * wm
    x0s = np.stack([(0.001 + 0.002 * c) * wm for c in range(C)])
    ea.batch_init(x0s, low, high)
    acc_a, out_a, xs_a = ea.batch_run(p0s, dt, Ls, us, want_x=True)
    eb, _ = make()
    eb.batch_init(x0s, low, high)
    n_acc = 0
    for t in range(T):
        acc, out5 = eb.batch_trajectory(p0s[:, t], dt, Ls[:, t], us[:, t])
        for c in range(C):
            assert bool(acc[c]) == bool(acc_a[c, t]), (case, c, t)
            assert relmax(out_a[c, t], out5[c]) < 1e-10
            if acc[c]:
                assert relmax(xs_a[c, t], eb.batch_get_x(c)) < 1e-10
                n_acc += 1
    assert 0 < n_acc
    for c in range(C):
        assert relmax(ea.batch_get_x(c), eb.batch_get_x(c)) < 1e-10
    ea.close()
    eb.close()


@pytest.mark.parametrize("form", ["teams_one_read", "teams_time_out", "teams_time_out_desync"])
@pytest.mark.parametrize("case", ["twelve_members_rows_of_16_lanes", "twenty_one_members_half_waves"])
def test_batch_on_teams_reads_G_once_and_matches_the_two_pass_batch(G, monkeypatch, case, form):
    """batch_team_kernel (csrc/batchteam.hip.h): the workgroups holding the row chunks of a column tile
    exchange their partial dots (reduce-scatter), update their share of the (cell, chain) pairs and
    collect the new positions (all-gather), so that adjoint, update and forward of ALL chains come from
    one read of G (hmc.py:114-152 per chain).  Against the two-pass MFMA batch (itself checked against
    single-chain engines above): same decisions, results <= 1e-10, in lock-step rounds and with
    desynchronised chains; every phase of a chain (update, final half step, idle, the speculative first
    step of gh_batch_run) passes through the team kernel.  A time-out (test hook: the members wait for a
    part that never comes) must leave the chains' states intact and repeat the work on the two passes."""
    rng = np.random.default_rng(23)
    if case == "twelve_members_rows_of_16_lanes":
        N, M, C = 5003, 1234, 5          # 79 row blocks of 64: 12 members, 22 pairs each, partial last tile
    else:
        N, M, C = 9001, 1000, 16         # 141 row blocks: 21 members, 13 pairs each (the last member: none)
    A = np.asfortranarray(rng.normal(size=(N, M)))
    dobs, shape = rng.normal(size=N) * 20, (1, 1, M)
    dt, sig, hi, T = 0.004, 0.02, 0.5, 3

    def make(team):
        monkeypatch.setenv("GRAVHMC_BATCH_TEAM", team)
        e = G.Engine(N, M)
        e.upload_G(A)
        w = e.weight(0.5)
        e.set_data(dobs)
        e.set_reg("Damping", 1.0, 0.01, shape, 0.001 * w)
        x0s = np.stack([(0.001 + 0.002 * c) * w for c in range(C)])
        e.batch_init(x0s, 0.0 * w, hi * w)
        return e

    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    if form != "teams_one_read":
        monkeypatch.setenv("GRAVHMC_BATCH_TEAM_TEST_ABORT", "1")
    et = make("1")
    e2 = make("0")
    st = et.batch_fused_stats()
    assert st["members"] == (12 if N == 5003 else 21) and st["ranges"] >= 1
    assert e2.batch_fused_stats()["members"] == 0
    Ls = rng.integers(1, 7, size=(C, T))
    p0s = rng.normal(size=(C, T, M)) * sig
    us = rng.uniform(size=(C, T))
    n_acc = 0
    if form == "teams_time_out_desync" or form == "teams_one_read":
        acc_t, out_t, xs_t = et.batch_run(p0s, dt, Ls, us, want_x=True)
        acc_2, out_2, xs_2 = e2.batch_run(p0s, dt, Ls, us, want_x=True)
        assert np.array_equal(acc_t, acc_2)
        assert relmax(out_t, out_2) < 1e-10
        for c in range(C):
            for t in range(T):
                if acc_2[c, t]:
                    assert relmax(xs_t[c, t], xs_2[c, t]) < 1e-10
                    n_acc += 1
    if form != "teams_time_out_desync":
        for t in range(T):
            p1 = rng.normal(size=(C, M)) * sig
            L1 = rng.integers(1, 7, size=C)
            u1 = rng.uniform(size=C)
            acc_t, out_t = et.batch_trajectory(p1, dt, L1, u1)
            acc_2, out_2 = e2.batch_trajectory(p1, dt, L1, u1)
            assert np.array_equal(acc_t, acc_2), (case, t)
            assert relmax(out_t, out_2) < 1e-10
            n_acc += int(np.sum(acc_2))
    assert n_acc > 0
    for c in range(C):
        assert relmax(et.batch_get_x(c), e2.batch_get_x(c)) < 1e-10
    st = et.batch_fused_stats()
    if form == "teams_one_read":
        assert st["timeouts"] == 0 and st["launches"] > 0 and st["members"] > 0
    else:
        assert st["timeouts"] == 1 and st["members"] == 0      # off for good after the time-out
    et.close()
    e2.close()


def test_batch_run_carry_over_continues_trajectories_across_calls(G, monkeypatch):
    """gh_batch_run in carry-over mode: a call ends when the first chain has used up its offer, the
    others keep their trajectory in flight and finish it in a later call.  Feeding the chains call
    by call (re-offering what was not started) must give every chain exactly the results of lock-step
    rounds, in order; T = 0 drains; the lock-step call refuses while something is in flight."""
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    rng = np.random.default_rng(23)
    p = gold("potential_small.npz")
    A, dobs, shape = np.asarray(p["Aw"]) * p["wm"][None, :], p["dobs"], p["shape"]
    N, M = A.shape
    C, n_traj, T, dt = 5, 14, 3, 0.02

    def make():
        e = G.Engine(N, M)
        e.upload_G(A)
        w = e.weight(0.5)
        e.set_data(dobs)
        e.set_reg("TV", 1.0, 0.001, shape, 0.001 * w)
        return e, w

    ea, wm = make()
    Ls = rng.integers(1, 9, size=(C, n_traj))
    p0s = rng.normal(size=(C, n_traj, M)) * 0.3
    us = rng.uniform(size=(C, n_traj))
    x0s = np.stack([(0.001 + 0.002 * c) * wm for c in range(C)])
    ea.batch_init(x0s, 0.0 * wm, 0.02 * wm)
    eb, _ = make()
    eb.batch_init(x0s, 0.0 * wm, 0.02 * wm)
    ref = [eb.batch_trajectory(p0s[:, t], dt, Ls[:, t], us[:, t]) for t in range(n_traj)]
    started = [0] * C
    got = [[] for _ in range(C)]
    calls = 0
    in_flight_seen = False
    while max(started) + T <= n_traj:            # while every chain can still be offered T trajectories
        off = [list(range(started[c], started[c] + T)) for c in range(C)]
        acc, out5, xs, ns, nd = ea.batch_run([[p0s[c, t] for t in off[c]] for c in range(C)], dt,
                                             [[Ls[c, t] for t in off[c]] for c in range(C)],
                                             [[us[c, t] for t in off[c]] for c in range(C)], want_x=True, carry=True)
        calls += 1
        for c in range(C):
            started[c] += int(ns[c])
            for i in range(int(nd[c])):
                got[c].append((bool(acc[c, i]), out5[c, i].copy(), xs[c, i].copy()))
        in_flight_seen = in_flight_seen or any(started[c] > len(got[c]) for c in range(C))
    assert calls >= 2 and in_flight_seen
    if any(started[c] > len(got[c]) for c in range(C)):
        with pytest.raises(ValueError):
            ea.batch_trajectory(p0s[:, 0], dt, Ls[:, 0], us[:, 0])
    acc, out5, xs, ns, nd = ea.batch_run([[] for _ in range(C)], dt, np.zeros((C, 0)), np.zeros((C, 0)),
                                         want_x=True, carry=True)
    for c in range(C):
        assert ns[c] == 0 and nd[c] <= 1
        if nd[c]:
            got[c].append((bool(acc[c, 0]), out5[c, 0].copy(), xs[c, 0].copy()))
        assert len(got[c]) == started[c] >= T
        for t, (a_, o_, x_) in enumerate(got[c]):
            assert a_ == bool(ref[t][0][c]) and relmax(o_, ref[t][1][c]) < 1e-10, (c, t)
    ea.close()
    eb.close()


def test_hmcsample_batch_reproduces_reference_chains(G, tmp_path, capsys):
    """HMCSampleBatch: chains 0..2 of one MFMA batch; chain 0 must print the reference's own
    chain-0 lines (chain_small fixtures), every chain must equal a separate HMCSample(myrank=r)."""
    c = gold("chain_small.npz")
    p = gold("potential_small.npz")
    M = p["wm"].size
    for tag in ("a", "b"):
        dt, Sigma, lo, hi, n = c[tag + "_cfg"]
        reg = str(c[tag + "_reg"])
        args = (np.full(M, 0.001 + lo), np.full(M, 0.001), np.c_[np.full(M, lo), np.full(M, hi)],
                "mandatory", 1000, p["dobs"], "Fixed", 0.8, 1.0, reg, 0.001, 100, float(Sigma))
        gm = _module_small(G, p)
        capsys.readouterr()
        G.HMCSampleBatch(gm, 3, int(n), 0, float(dt), [5, 20], *args,
                         save_folder=str(tmp_path / ("batch_%s_chain" % tag)))
        out = capsys.readouterr().out.splitlines()
        ref0 = [str(s) for s in c[tag + "_lines"]]
        got0 = [l for l in out if l.startswith("chain 0:")]
        assert got0 == ref0
        for r in (1, 2):
            gs = _module_small(G, p)
            capsys.readouterr()
            G.HMCSample(gs, int(n), 0, float(dt), [5, 20], *args, myrank=r,
                        save_folder=str(tmp_path / ("single_%s_chain" % tag)))
            single = [l for l in capsys.readouterr().out.splitlines() if l.startswith("chain %d:" % r)]
            assert [l for l in out if l.startswith("chain %d:" % r)] == single
            a = np.loadtxt(str(tmp_path / ("batch_%s_chain%d" % (tag, r))) + "/model.dat")
            b = np.loadtxt(str(tmp_path / ("single_%s_chain%d" % (tag, r))) + "/model.dat")
            np.testing.assert_allclose(a, b, atol=2e-8)
        np.testing.assert_allclose(np.loadtxt(str(tmp_path / ("batch_%s_chain0" % tag)) + "/model.dat"),
                                   c[tag + "_model"], atol=2e-8)


def test_row_panels_chain_matches_oracle(G, orc, monkeypatch, capfd):
    """N > 16384 observations: a column no longer fits one workgroup's registers.  The fused leapfrog
    step runs on teams of workgroups that share a column (one read of G, teamsweep.hip.h); with
    GRAVHMC_TEAM=0, and after a team timed out, in row panels (adjoint of all panels, update,
    forward of all panels).  Potential, gradient and trajectories against the CPU oracle on both
    paths; a time-out of the teams (test hook) repeats the trajectory in row panels: same bits as
    the row-panel run.  Bound: max(1e-10, 10 x the oracle's own spread under a reversal of the
    observation rows) -- 5.1e-16 under MS (all five rejected), 1.0e-14 under TV (all accepted), so
    1e-10; the state is compared after rejections too, and chain_get_x() at the end."""
    rng = np.random.default_rng(8)
    N, M = 17011, 150
    A = np.asfortranarray(rng.normal(size=(N, M)) * rng.uniform(0.2, 2, size=M))
    dobs = rng.normal(size=N) * 3
    seeds = {}
    runs = {}
    for path in ("team", "panels", "team-abort"):
        monkeypatch.setenv("GRAVHMC_TEAM", "0" if path == "panels" else "1")
        monkeypatch.setenv("GRAVHMC_TEAM_TEST_ABORT", "1" if path == "team-abort" else "0")
        rng = np.random.default_rng(80)
        eng = G.Engine(N, M)
        eng.upload_G(A)
        wm = eng.weight(0.5)
        Aw, wmo = orc.col_weight(A)
        assert relmax(wm, wmo) < 1e-13 and relmax(eng.download_G(), Aw) < 1e-13
        eng.set_data(dobs)
        runs[path] = []
        for reg, shape in (("MS", (1, 1, M)), ("TV", (5, 5, 6))):
            eng.set_reg(reg, 0.7, 0.01, shape, 0.001 * wm)
            P = orc.Problem(Aw, dobs, 0.001 * wm, reg, 0.7, 0.01, wm=wm, shape=shape)
            x = rng.uniform(0, 1, M) * wm
            a, b = eng.misfit_and_grad(x), P.misfit_and_grad(x)
            assert abs(a[0] - b[0]) < 1e-11 * abs(b[0]) and relmax(a[1], b[1]) < 1e-11 and relmax(a[2], b[2]) < 1e-11
            low, high = 0.0 * wm, 0.3 * wm
            xg = xo = 0.001 * wm
            eng.chain_init(xg, low, high)
            ntr = 2 if path == "team-abort" else 5          # (every aborted launch waits 2 s)
            trajs = [(int(rng.integers(1, 7)), rng.normal(size=M) * 0.02, float(rng.uniform())) for _ in range(5)][:ntr]
            # the bound: the oracle against itself with the observation rows reversed (every sum over the 17011
            # observations in another order) on these trajectories, times ten, and no less than 1e-10 -- the
            # rule of tests/team_oracle_cases.py
            Pr = orc.Problem(np.asfortranarray(Aw[::-1]), dobs[::-1].copy(), 0.001 * wm, reg, 0.7, 0.01, wm=wm, shape=shape)
            spread, xa, xb = 0.0, xo, xo
            for L, p0, u in trajs:
                xa, acca, oa, _ = P.leapfrog(xa, p0, 0.002, L, low, high, u)
                xb, accb, ob, _ = Pr.leapfrog(xb, p0, 0.002, L, low, high, u)
                assert acca == accb
                spread = max(spread, relmax(ob, oa), relmax(xb, xa))
            tol = max(1e-10, 10.0 * spread)
            assert tol <= 1e-9
            res = []
            eng.run_chain(iter(trajs), 0.002, lambda L, acc, o, xs: res.append((acc, o.copy(), xs)), want_x=True)
            xd, worst = xo, 0.0
            for (L, p0, u), (acc, o, xs) in zip(trajs, res):
                xo, acco, oo, _ = P.leapfrog(xo, p0, 0.002, L, low, high, u)
                assert (xs is not None) == bool(acc)
                xd = xs if acc else xd          # (after a rejection: the state before)
                worst = max(worst, relmax(o, oo), relmax(xd, xo))
                assert acc == acco and relmax(o, oo) <= tol, (path, reg, relmax(o, oo), tol)
                assert relmax(xd, xo) <= tol, (path, reg, relmax(xd, xo), tol)
            x_end = eng.chain_get_x()           # the state the chain is left in, after a rejection too
            assert np.array_equal(x_end, xd) and relmax(x_end, xo) <= tol
            print("%s, %s: spread %.2e, bound %.2e, worst relmax against the oracle %.2e" % (path, reg, spread, tol, worst))
            runs[path].append(res)
        eng.close()
    err = capfd.readouterr().err
    assert err.count("team sweep timed out") == 3 and "(3 of 3)" in err
    for ra, rb in zip(runs["team-abort"], runs["panels"]):
        for (a1, o1, x1), (a2, o2, x2) in zip(ra, rb):       # repeated in row panels: the panel run's bits
            assert a1 == a2 and np.array_equal(o1, o2) and (x1 is None or np.array_equal(x1, x2))


# ------------------------------------------------------------- conjugate gradient (reginv)

def test_conjugate_gradient_matches_reference(G, capsys):
    """ConjugateGradient.CG on the device primitives against the reference's own run
    (tests/golden/cg_small.npz, inversion/reginv.py:357-492), all four regularisers."""
    g = gold("cg_small.npz")
    cg = G.ConjugateGradient(g["dobs"], tuple(g["mrange"]), tuple(g["mspacing"]),
                             (g["xp"], g["yp"], g["zp"]), verbose=False)
    M = cg.msize
    assert (cg.dsize, M, cg.mshape) == (42, 120, tuple(g["shape"]))
    for reg in ("MS", "Damping", "Smoothness", "TV"):
        res = cg.CG(np.full(M, 0.001), np.full(M, 0.001), (0.0, 1.0), regularization=reg, beta=0.01,
                    q=0.9, maxk=8)
        capsys.readouterr()
        errs = {name: relmax(np.asarray(v, float), g[reg + "_" + name])
                for name, v in zip(("model", "data", "dmis", "mmis", "alpha"), res)}
        assert max(errs.values()) < 1e-7, (reg, errs)
    with pytest.raises(ValueError):
        cg.CG(np.full(M, 0.001), np.full(M, 0.001), (0.0, 1.0), regularization="L1")
    # the MS gradient quirk of reginv.py:288-292 is what gh_reg_eval(ms_grad_den_mw=1) computes
    rng = np.random.default_rng(0)
    wm = cg.Wm.diagonal()
    mw, apr = rng.uniform(0, 1, M) * wm, 0.3 * wm
    v, gq = cg._engine.reg_eval("MS", mw, apr, 0.01, cg.mshape, ms_grad_den_mw=True)
    assert relmax(gq, 2 * 0.01 * wm ** 2 * (mw - apr) / (mw * mw + 0.01) ** 2) < 1e-14
    v2, gp = cg._engine.reg_eval("MS", mw, apr, 0.01, cg.mshape, ms_grad_den_mw=False)
    assert v == v2 and relmax(gp, 2 * 0.01 * wm ** 2 * (mw - apr) / ((mw - apr) ** 2 + 0.01) ** 2) < 1e-14


def test_ratiogrid_wavelet_log_lines_on_gpu(G, tmp_path, capsys):
    """example/ratiogrid/logout_T1.txt chains 0 and 1 on the device: ratio mesh (19, 30, 30), odd
    wavelet lengths, MS, a rejected proposal on line 3 of chain 0."""
    e = gold("example_inputs.npz")
    obs = e["ratio_obs"]
    M = 17100
    import re
    pat = re.compile(r"=\(([-\d.]+),([-\d.]+),([-\d.]+),([-\d.]+)\) -- accept ratio ([\d.]+)%")
    for rank, key in ((0, "ratio_T1_chain0"), (1, "ratio_T1_chain1")):
        gm = G.GravMagModule(obs[:, 3], (0, 6000, 0, 6000, 0, 6000), (200, 200, 200),
                             (obs[:, 0], obs[:, 1], obs[:, 2]), mratio=1.05, wavelet='3D', verbose=False)
        assert gm.mshape == (19, 30, 30)
        capsys.readouterr()
        G.HMCSample(gm, 6, 0, 0.01, [5, 20], np.full(M, 0.001), np.full(M, 0.001),
                    np.c_[np.zeros(M), np.full(M, 0.4)], "mandatory", 1000, obs[:, 3], "Fixed", 0.8, 1,
                    "MS", 0.001, 100, 0.001, myrank=rank, save_folder=str(tmp_path / "ratio_chain"),
                    sample_sink="none")
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("chain %d" % rank)]
        got = np.array([[float(v) for v in pat.search(l).groups()] for l in lines])
        n = min(len(got), len(e[key]))          # the fixture keeps the first 40 lines of the log
        assert n >= 6
        got, ref = got[:n], e[key][:n]
        np.testing.assert_allclose(got[:, [0, 1, 3]], ref[:, [0, 1, 3]], rtol=0, atol=1.01e-7)
        np.testing.assert_allclose(got[:, 4], ref[:, 4], atol=0.006)
        assert (np.diff(got[:, 4]) < 0).any()  # rejected proposals occur, as in the reference's log
        gm._engine.close()


def test_global_c4_full_kernel_against_reference_log(G, orc):
    """Config C4 at full size (7381 x 72000 tesseroids, 5.3e8 adaptive-GLQ pairs, assembled on the
    device in ~0.1 s; the reference's log reports 246 s + 228 s of weighting): `initial mw` of
    example/global/logout_T1.txt to its 9 printed digits, and sampled columns against the oracle."""
    from test_oracle_golden import GLOBAL_MW_HEAD, GLOBAL_MW_TAIL, global_inputs
    mesh, lon, lat, h = global_inputs()
    gm = G.GravMagModule(np.zeros(lon.size), (-180, 180, -90, 90, 0, -3000000), (-300000, 3, 3),
                         (lon, lat, h), coordinate="spherical", verbose=False)
    assert gm.mshape == (10, 60, 120) and gm._engine.M == 72000
    wm = gm.Wm.diagonal()
    np.testing.assert_allclose(0.01 * wm[:3], GLOBAL_MW_HEAD, rtol=5e-9)
    np.testing.assert_allclose(0.01 * wm[-3:], GLOBAL_MW_TAIL, rtol=0, atol=5.1e-9)
    st = gm._engine.kernel_stats()
    assert st["warn_cells"] == 0 and st["leaves"] >= 7381 * 72000
    cols = np.r_[0, 1, 2, 35999, 36000, 71997, 71998, 71999]
    Ko = orc.tess_gz_kernel(lon, lat, h, mesh.cell_bounds()[cols])
    assert relmax(wm[cols], np.sqrt((Ko ** 2).sum(0))) < 1e-11
    # unit-norm columns: ||Aw e_j|| = 1
    for j in (0, 36000, 71999):
        e = np.zeros(72000)
        e[j] = 1.0
        d = gm._engine.forward(e)
        assert abs(np.linalg.norm(d) - 1.0) < 1e-12
        assert relmax(d, Ko[:, list(cols).index(j)] / wm[j]) < 1e-10
    gm._engine.close()


def test_bootstrap_matches_reference(G, capsys):
    """BootStrap.BSCG (row counts on the resident kernel instead of a resampled copy) against the
    reference's own run (tests/golden/bs_small.npz, inversion/reginv.py:715-755)."""
    g, b = gold("cg_small.npz"), gold("bs_small.npz")
    bs = G.BootStrap(tuple(g["mrange"]), tuple(g["mspacing"]), (g["xp"], g["yp"], g["zp"]), g["dobs"],
                     (0.0, 1.0), samples=3, beta=0.1, maxk=5, verbose=False)
    res = bs.BSCG(np.full(bs.msize, 0.001))
    capsys.readouterr()
    for name, v in zip(("models", "dmis", "mmis", "alpha"), res):
        assert relmax(v, b[name]) < 1e-7, name


def test_prism_assembly_against_the_reference_kernel_compiled_from_its_own_source(G, orc):
    """The reference's own Cython kernel (gravmag/_prism.pyx, compiled unmodified by oracle/build_ref.py)
    evaluated C1's 600 x 6000 kernel for 300 random cells (prism.py:291-316 -> _prism.pyx:265-290: kernel1D
    of every observation, times G * SI2MGAL); c1_prism_columns.npz holds the cells and the digest of that
    block (oracle/make_golden.py).  On the GPU box: the C restatement reproduces the block bit for bit, and
    the HIP assembly matches it."""
    g = gold("c1_prism_columns.npz")
    mesh = G.mesher.PrismMesh((0, 2000, 0, 3000, 0, 1000), (100, 100, 100))
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 3000, 30), np.linspace(0, 2000, 20))]
    zp = np.zeros_like(xp)
    bounds = mesh.cell_bounds()
    eng = G.Engine(xp.size, mesh.size)
    eng.set_obs(xp, yp, zp)
    eng.set_cells(bounds, 0)
    eng.build_G()
    K = eng.download_G()
    cols = g["cols"]
    assert cols.size == 300
    Kref = orc.prism_gz_kernel(xp, yp, zp, bounds[cols])
    assert orc.kernel_digest(Kref) == str(g["digest"])   # the oracle IS the reference's arithmetic
    assert np.abs(Kref).max() == g["absmax"]
    err = float(np.abs(K[:, cols] - Kref).max() / np.abs(Kref).max())
    print("HIP prism assembly vs the reference's compiled _prism.gz (600 x 300 entries of C1): %.2e" % err)
    assert err < 1e-12
    eng.close()


@pytest.mark.parametrize("wavelet", ["3D", "1D"])
def test_bootstrap_with_wavelet_forward_matches_the_port(G, capsys, wavelet):
    """BootStrap(wavelet=...) (reginv.py:546-553): the data term and its gradient predict the data with the
    compressed UNRESAMPLED operator (`modelcompressor(mw, self.Awcp)`, :590-593, :608-617) and compare them
    with the RESAMPLED observations, the step length keeps the resampled dense kernel (:655) -- the
    reference's behaviour as written, restated in oracle/cg_port.py (PyWavelets is not installed in the build
    container: no reference-generated fixture for this combination; the transform itself is pinned by the
    reference's wavelet logs)."""
    from oracle import cg_port
    g = gold("cg_small.npz")
    shape = tuple(int(v) for v in g["shape"])
    M = int(np.prod(shape))
    bs = G.BootStrap(tuple(g["mrange"]), tuple(g["mspacing"]), (g["xp"], g["yp"], g["zp"]), g["dobs"],
                     (0.0, 1.0), samples=3, beta=0.1, maxk=5, wavelet=wavelet, verbose=False)
    res = bs.BSCG(np.full(bs.msize, 0.001))
    capsys.readouterr()
    ref = cg_port.bootstrap(g["K"], g["dobs"], (0.0, 1.0), np.full(M, 0.001), samples=3, beta=0.1, maxk=5,
                            wavelet=wavelet, shape=shape)
    dense = cg_port.bootstrap(g["K"], g["dobs"], (0.0, 1.0), np.full(M, 0.001), samples=3, beta=0.1, maxk=5)
    for name, v, r in zip(("models", "dmis", "mmis", "alpha"), res, ref):
        assert relmax(v, r) < 1e-7, (wavelet, name)
    assert relmax(ref[0], dense[0]) > 1e-6     # (the compressed forward does change the replicates)


# ------------------------------------------------ BASELINE.json configs exactly as stated (round 2)

def test_c3_segmentgrid_wavelet3d_tv_as_baseline_states_it(G, orc, monkeypatch):
    """BASELINE configs[2] as written: segmentgrid mesh (dz 100/200/300 m on [0,300,900,2100], shape
    (10,30,20)), 600 observations, wavelet='3D' compressed forward (db4, level 2, periodization,
    threshold 1e-3) with the exact dense adjoint (potential.py:693-708) and the **TV** regulariser,
    on the resident chain kernel and on the sweep path (DWT + CSR SpMV), against
    oracle.Problem(csr=..., dwt=...) on the same 600 x 6000 kernel: potential, gradient, chain."""
    from oracle import wavelet as ow
    e = gold("example_inputs.npz")
    obs = e["seg_obs"]
    M, shape = 6000, (10, 30, 20)
    rng = np.random.default_rng(33)
    trajs = [(int(rng.integers(5, 21)), rng.normal(size=M) * 0.001, float(rng.uniform())) for _ in range(6)]
    ref = None
    for mode in ("1", "0"):
        monkeypatch.setenv("GRAVHMC_RESIDENT", mode)
        gm = G.GravMagModule(obs[:, 3], (0, 2000, 0, 3000, 0, 2100), ([100, 200, 300], 100, 100),
                             (obs[:, 0], obs[:, 1], obs[:, 2]), mseg=True,
                             mdivisionsection=[0, 300, 900, 2100], wavelet='3D', verbose=False)
        assert tuple(gm.mshape) == shape
        wm = gm.Wm.diagonal()
        mwapr, low, high = 0.001 * wm, 0.0 * wm, 1.0 * wm
        if ref is None:
            Aw = np.asarray(gm.Aw)
            csr = ow.compress_kernel(Aw, 3, shape)
            got = gm.Awcp
            assert got.shape == csr.shape == (600, 6820) and got.nnz == csr.nnz
            P = orc.Problem(Aw, obs[:, 3], mwapr, "TV", 1.0, 0.001, wm=wm, shape=shape, csr=csr,
                            dwt=lambda v: ow.model_coeffs(v, 3, shape))
            xs = [mwapr, rng.uniform(0, 1, M) * wm, 0.3 * wm * (1 + 0.1 * rng.normal(size=M))]
            ref = {"mg": [P.misfit_and_grad(x) for x in xs], "chain": []}
            xo = mwapr
            for (L, p0, u) in trajs:
                xo, acco, oo, _ = P.leapfrog(xo, p0, 0.01, L, low, high, u)
                ref["chain"].append((acco, oo.copy(), xo.copy()))
        for x, b in zip(xs, ref["mg"]):
            a = gm.misfit_and_grad(x, mwapr, None, None, "mandatory", 1000, 1.0, regulization="TV", beta=0.001)
            assert abs(a[0] - b[0]) < 1e-11 * abs(b[0]) and relmax(a[1], b[1]) < 1e-10
            assert relmax(a[2], b[2]) < 1e-10 and abs(a[4] - b[4]) < 1e-11 * abs(b[4])
        eng = gm._engine
        eng.chain_init(mwapr, low, high)
        out = []
        eng.run_chain(iter(trajs), 0.01, lambda L, acc, o, x: out.append((acc, o.copy(), x)), want_x=True, batch=3)
        assert (eng.chain_stats()["resident_launches"] > 0) == (mode == "1")
        assert len(out) == len(trajs)
        for (acc, o, x), (acco, oo, xo) in zip(out, ref["chain"]):
            assert acc == acco and relmax(o, oo) < 1e-9
            if acc:
                assert relmax(x, xo) < 1e-9
        print("C3 (TV, wavelet 3D) path resident=%s: nnz %d, accepted %d of %d" %
              (mode, got.nnz, sum(t[0] for t in out), len(out)))
        eng.close()


@pytest.mark.parametrize("exact", ["0", "1"])
def test_c4_matrix_free_full_size_against_dense(G, orc, monkeypatch, exact):
    """(exact: GRAVHMC_MF_EXACT, the root leaf in the reference's operation order instead of the
    throughput form -- both within the stated 1e-10, the former 100x tighter.)
    BASELINE configs[3] at full size (3-degree global tesseroid mesh 10 x 60 x 120 = 72000 cells,
    121 x 61 = 7381 observations at 5000 m, Damping 0.05): the matrix-free engine (entries
    re-evaluated, never stored) against the dense engine on the same problem: column norms,
    forward, potential + gradient, and a short chain with identical decisions."""
    monkeypatch.setenv("GRAVHMC_MF_EXACT", "1" if exact == "0" else "0")   # the ABI call below overrides it
    mesh = G.mesher.TesseroidMesh((-180, 180, -90, 90, 0, -3000000), (-300000, 3, 3))
    lon, lat = [a.ravel() for a in np.meshgrid(np.arange(-180, 181, 3.0), np.arange(-90, 91, 3.0), indexing="ij")]
    h = np.full_like(lon, 5000.0)
    N, M = lon.size, mesh.size
    assert (N, M) == (7381, 72000)
    rho = np.zeros(mesh.shape)
    rho[1:4, 20:30, 40:60] = 0.3
    rho = rho.ravel()
    rng = np.random.default_rng(44)
    engs = {}
    for tag in ("dense", "mf"):
        eng = G.Engine(N, M)
        if tag == "mf":
            eng.set_matrix_free(True, exact=(exact == "1"))      # gh_set_matrix_free_exact
        eng.set_obs(lon, lat, h)
        eng.set_cells(mesh.cell_bounds(), 1, 1.6)
        eng.build_G()
        engs[tag] = eng
    d, m = engs["dense"], engs["mf"]
    dt = d.forward(rho)
    e_fwd = relmax(m.forward(rho), dt)
    assert e_fwd < 1e-10                                       # unweighted forward = the reference's gz
    wd, wmf = d.weight(0.5), m.weight(0.5)
    assert relmax(wmf, wd) < 1e-12
    # ORACLE values for the matrix-free arithmetic at full-size geometry: 64 random observations and the
    # two polar rows (every cell of a polar cap is in their near field) x all 72000 cells from the C
    # restatement of gravmag/_tesseroid_numba.py:32-157,207-222, against row i of the matrix-free kernel,
    # K[i, :] = wm * (Aw^T e_i) -- the pass evaluates all 5.3e8 entries to deliver it
    rows = np.r_[rng.choice(N, 64, replace=False), [0, 60, 60 * 61 + 30, N - 1]]
    assert lat[0] == -90 and lat[60] == 90
    Ko = orc.tess_gz_kernel(lon[rows], lat[rows], h[rows], mesh.cell_bounds())
    st = m.matrix_free_stats()
    e_row, n_near_rows = 0.0, 0
    for q, i in enumerate(rows):
        ei = np.zeros(N)
        ei[i] = 1.0
        Ki = m.adjoint(ei) * wd
        e_row = max(e_row, float(np.abs(Ki - Ko[q]).max() / np.abs(Ko[q]).max()))
        e_col = np.abs(Ki - Ko[q]) / np.maximum(np.abs(Ko[q]), 1e-300)
        assert e_col.max() < 1e-9, (i, e_col.max())              # entry by entry (relative to the entry itself)
    print("C4 matrix-free (exact=%s) rows vs the ORACLE (68 rows x 72000 cells, polar rows included): %.2e of the "
          "row's largest entry; near-field table %r" % (exact, e_row, st))
    assert e_row < 1e-10 and st["near_entries"] > 0
    dobs = dt + 0.02 * np.abs(dt).max() * rng.normal(size=N)
    x = rng.uniform(0, 0.8, M) * wd
    for eng in (d, m):
        eng.set_data(dobs)
        eng.set_reg("Damping", 0.05, 0.01, mesh.shape, 0.001 * wd)
    a, b = m.misfit_and_grad(x), d.misfit_and_grad(x)
    print("C4 matrix-free (exact=%s) vs dense: forward %.2e U %.2e grad %.2e dpre %.2e" %
          (exact, e_fwd, abs(a[0] - b[0]) / abs(b[0]), relmax(a[1], b[1]), relmax(a[2], b[2])))
    assert abs(a[0] - b[0]) < 1e-10 * abs(b[0]) and relmax(a[1], b[1]) < 1e-10 and relmax(a[2], b[2]) < 1e-10
    trajs = [(int(rng.integers(2, 6)), rng.normal(size=M) * 0.001, float(rng.uniform())) for _ in range(3)]
    outs = {}
    for tag, eng in engs.items():
        eng.chain_init(0.001 * wd, 0.0 * wd, 0.8 * wd)
        res = []
        eng.run_chain(iter(trajs), 0.005, lambda L, acc, o, xx, res=res: res.append((acc, o.copy())))
        outs[tag] = (res, eng.chain_get_x())
    for (a1, o1), (a2, o2) in zip(outs["mf"][0], outs["dense"][0]):
        assert a1 == a2 and relmax(o1, o2) < 1e-9
    assert relmax(outs["mf"][1], outs["dense"][1]) < 1e-9
    d.close()
    m.close()


def test_c5_shaped_row_panels_and_column_shards_together():
    """BASELINE configs[4] in miniature, all of its ingredients at once: the full 200 x 200
    observation grid (N = 4*10^4 > 16384 rows: row panels / multi-workgroup column teams), MS
    regulariser, three z-layers of a 40 x 40 block of the 200 x 200 x 60 mesh (4800 cells, their
    true C5 bounds), the cells sharded over three ranks (gloo, one GPU) -- against oracle.Problem on
    the same cells: column norms, forward, potential, gradient and five trajectories; the unsharded
    engine on the same problem as well."""
    import json
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "shard_worker_c5.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    print("C5-shaped 3-rank check:", res)
    assert res["N"] == 40000 and res["M_local"] == [1600, 1600, 1600] and res["n_panels"] > 1
    assert res["wm"] < 1e-12 and res["fwd"] < 1e-10
    for tag in ("sharded", "single"):
        for reg in ("MS", "TV"):
            r = res[tag][reg]
            assert r["U"] < 1e-11 and r["grad"] < 1e-10 and r["dpre"] < 1e-10, (tag, reg, r)
        c = res[tag]["chain"]
        assert c["decisions_equal"] and c["n"] == 5 and c["out5"] < 1e-9 and c["x"] < 1e-9, (tag, c)
    # a team sweep that gives up on ONE rank: all ranks count the same time-outs (the decision is
    # collective) and the repeated chain is the chain
    ab = res["abort"]
    if ab["teams_in_use"]:
        assert len(set(ab["timeouts"])) == 1 and ab["timeouts"][0] >= 1, ab
    assert ab["decisions_equal"] and ab["out5"] < 1e-11 and ab["x"] < 1e-11, ab


@pytest.mark.parametrize("axis", ["cells", "rows"])
def test_bench_shard_rehearsal_two_ranks_one_gpu(axis):
    """(axis: column blocks -- the cells split -- or row blocks -- the observations split, BASELINE configs[4] as
    it is worded.)  The N > 1 launch path of bench.py as the driver starts it (torch.distributed.run, one rank per
    process), rehearsed on one GPU: ONE chain whose cells are sharded over two ranks
    (`--shard --shard-backend gloo --rehearse-on-one-gpu`) on a small C5-shaped workload (the full
    200 x 200 observation grid, 1/600 of the cells).  The JSON line must say strong scaling, count the
    chain's steps once, and the chain must end where the unsharded run of the same command ends."""
    import json
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    common = ["--workload", "c5_uniform_200x200x60", "--cells-fraction", "600", "--steps", "30", "--warmup", "10",
              "--no-cpu-baseline"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + common,
                         capture_output=True, text=True, timeout=600, env=env)
    assert one.returncode == 0, one.stderr[-2000:]
    single = json.loads(one.stdout.strip().splitlines()[-1])
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--shard", "--shard-axis", axis, "--shard-backend", "gloo", "--rehearse-on-one-gpu"] + common
    two = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert two.returncode == 0, (two.stdout[-1000:], two.stderr[-3000:])
    lines = [l for l in two.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                  # rank 0 prints, once
    sh = json.loads(lines[0])
    assert sh["scaling"] == "strong" and sh["n_gpus"] == 2 and sh["steps"] == 30
    assert abs(sh["value"] - 30 / (sh["ms_per_step"] * 30e-3)) < 1e-6 * sh["value"]   # steps counted once
    assert sh["config"]["M_cells"] == single["config"]["M_cells"] == 4000 and sh["config"]["N_obs"] == 40000
    assert sh["config"]["trajectories"] == single["config"]["trajectories"] == 3
    assert sh["config"]["accepted"] == single["config"]["accepted"]
    assert relmax(sh["config"]["final_U"], single["config"]["final_U"]) < 1e-9
    print("bench --shard --shard-axis %s rehearsal: %.1f steps/s on 2 ranks of one GPU (gloo), unsharded %.1f; final U %r"
          % (axis, sh["value"], single["value"], sh["config"]["final_U"]))


def test_bench_gpus_n_launches_its_own_ranks():
    """`python bench.py --gpus 2 ...` with no launcher around it (the shape of the driver's N = 1 command):
    the parent starts the two ranks as child processes before it has touched the GPU and relays rank 0's
    line.  Default mode = one independent chain per rank (weak scaling, no collective): rank 0 / 1 must be
    the seed-100 / seed-101 chains (hmc.py:369: seed + rank) -- the states single runs with those seeds
    end in.  `--shard --shard-backend gloo` = ONE chain over both ranks (strong scaling)."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    common = ["--workload", "c5_uniform_200x200x60", "--cells-fraction", "600", "--steps", "30", "--warmup", "10",
              "--no-cpu-baseline", "--no-extra"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)

    def run(extra):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra + common,
                             capture_output=True, text=True, timeout=900, env=env)
        assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1                              # rank 0 prints, once
        return json.loads(lines[0])

    singles = [run(["--gpus", "1", "--seed", str(100 + r)]) for r in range(2)]
    two = run(["--gpus", "2", "--rehearse-on-one-gpu"])
    assert two["n_gpus"] == 2 and two["scaling"] == "weak" and two["steps"] == 30
    assert abs(two["value"] - 2 * 30 / (two["ms_per_step"] * 30e-3)) < 1e-6 * two["value"]   # both chains counted
    per_rank = two["config"]["final_U_per_rank"]
    assert len(per_rank) == 2
    for r in range(2):
        assert relmax(per_rank[r], singles[r]["config"]["final_U"]) < 1e-9, (r, per_rank, singles[r]["config"])
    assert relmax(per_rank[0], per_rank[1]) > 1e-6          # (two different chains)
    sh = run(["--gpus", "2", "--rehearse-on-one-gpu", "--shard", "--shard-backend", "gloo"])
    assert sh["n_gpus"] == 2 and sh["scaling"] == "strong"
    assert relmax(sh["config"]["final_U"], singles[0]["config"]["final_U"]) < 1e-9
    print("bench --gpus 2 self-launched: chain-parallel %.1f steps/s, sharded %.1f steps/s, one rank %.1f"
          % (two["value"], sh["value"], singles[0]["value"]))


def test_one_launch_epilogue_matches_oracle_and_two_launch_form(G, orc, monkeypatch):
    """N > 8192: the sweep delivers the sums of its slab rows, so mean(d) is known before the slab is
    reduced and reduction, regulariser, residual and |r|^2 take ONE launch (reduce_finish_kernel)
    instead of two with a single-workgroup finish.  Potential, gradient and a chain against the
    oracle, with grav_fix, for a cell-local and a stencil regulariser; and against the two-launch
    form (GRAVHMC_EPILOGUE1=0), which differs only in the association of the mean."""
    rng = np.random.default_rng(77)
    N, M = 10007, 600
    A = np.asfortranarray(rng.normal(size=(N, M)) * rng.uniform(0.2, 2, size=M))
    dobs, gfix = rng.normal(size=N) * 3, rng.normal(size=N) * 5 + 40.0
    Aw, wmo = orc.col_weight(A)
    x = rng.uniform(0, 1, M) * wmo
    trajs = [(int(rng.integers(1, 7)), rng.normal(size=M) * 0.02, float(rng.uniform())) for _ in range(6)]
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("GRAVHMC_EPILOGUE1", mode)
        eng = G.Engine(N, M)
        eng.upload_G(A)
        wm = eng.weight(0.5)
        eng.set_data(dobs, gfix)
        got[mode] = []
        for reg, shape in (("MS", (1, 1, M)), ("TV", (6, 10, 10))):
            eng.set_reg(reg, 0.7, 0.01, shape, 0.001 * wm)
            P = orc.Problem(Aw, dobs, 0.001 * wm, reg, 0.7, 0.01, wm=wm, shape=shape, grav_fix=gfix)
            a, b = eng.misfit_and_grad(x), P.misfit_and_grad(x)
            assert abs(a[0] - b[0]) < 1e-11 * abs(b[0]) and relmax(a[1], b[1]) < 1e-11 and relmax(a[2], b[2]) < 1e-11
            low, high = 0.0 * wm, 0.3 * wm
            xo = 0.001 * wm
            eng.chain_init(xo, low, high)
            res = []
            eng.run_chain(iter(trajs), 0.002, lambda L, acc, o, xs: res.append((acc, o.copy(), xs)), want_x=True)
            for (L, p0, u), (acc, o, xs) in zip(trajs, res):
                xo, acco, oo, _ = P.leapfrog(xo, p0, 0.002, L, low, high, u)
                assert acc == acco and relmax(o, oo) < 1e-9
                if acc:
                    assert relmax(xs, xo) < 1e-9
            got[mode].append((a, res))
        eng.close()
    for (a1, r1), (a0, r0) in zip(got["1"], got["0"]):
        assert abs(a1[0] - a0[0]) <= 1e-13 * abs(a0[0]) and relmax(a1[1], a0[1]) < 1e-12
        for (c1, o1, x1), (c0, o0, x0) in zip(r1, r0):
            assert c1 == c0 and relmax(o1, o0) < 1e-11


@pytest.mark.parametrize("case", ["Damping", "TV", "wavelet3D-MS"])
def test_resident_chain_kernel_streams_columns_that_do_not_fit(G, monkeypatch, case):
    """Kernels larger than LDS + registers with N <= 1024 (the reference's ratiogrid example class):
    the resident chain kernel keeps as many columns per workgroup as fit in LDS and reads the rest
    from L2 / Infinity Cache in both passes of every evaluation (`stream` mode).  700 observations x
    16000 prisms (90 MB; with the wavelet forward also its dense compressed form; TV: 1024 x 11000):
    same chain as the
    sweep-per-launch path, decisions identical, energies and models to 1e-11."""
    # (the stencil regularisers need <= 44 cells per workgroup in this kernel: 1024 x 11000 there)
    zmax, nox, noy = (1100, 32, 32) if case == "TV" else (1600, 28, 25)
    mrange = (0, 4000, 0, 2500, 0, zmax)
    mesh = G.mesher.PrismMesh(mrange, (100, 100, 100))
    assert mesh.shape == (zmax // 100, 25, 40)
    yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 2500, noy), np.linspace(0, 4000, nox))]
    zp = np.zeros_like(xp)
    N, M = xp.size, mesh.size
    assert N * M * 8 > 85e6
    rng = np.random.default_rng(123)
    rho = np.zeros(mesh.shape)
    rho[3:7, 8:15, 12:24] = 0.6
    wav = "3D" if case.startswith("wavelet") else False
    reg = "MS" if case.startswith("wavelet") else case
    trajs = [(int(rng.integers(2, 9)), rng.normal(size=M) * 0.001, float(rng.uniform())) for _ in range(10)]
    res = {}
    for mode in ("stream", "sweep"):
        monkeypatch.setenv("GRAVHMC_RESIDENT", "1" if mode == "stream" else "0")
        eng0 = G.Engine(N, M)
        eng0.set_obs(xp, yp, zp)
        eng0.set_cells(mesh.cell_bounds(), 0)
        eng0.build_G()
        d_true = eng0.forward(rho.ravel())
        eng0.close()
        dobs = d_true + 0.02 * np.abs(d_true).max() * np.random.default_rng(5).normal(size=N)
        gm = G.GravMagModule(dobs, mrange, (100, 100, 100), (xp, yp, zp), wavelet=wav, verbose=False)
        wm = gm.Wm.diagonal()
        eng = gm._engine
        eng.set_reg(reg, 1.0, 0.001, mesh.shape, 0.001 * wm)
        eng.chain_init(0.001 * wm, 0.0 * wm, 1.0 * wm)
        out = []
        eng.run_chain(iter(trajs), 0.01, lambda L, acc, o, x: out.append((acc, o.copy(), x)), want_x=True, batch=4)
        st = eng.chain_stats()
        assert (st["resident_launches"] > 0) == (mode == "stream")
        res[mode] = (out, eng.chain_get_x(), eng.chain_get_dsyn())
        eng.close()
    (a, ax, ad), (b, bx, bd) = res["stream"], res["sweep"]
    assert len(a) == len(b) == len(trajs) and sum(t[0] for t in a) > 0
    for (a1, o1, x1), (a2, o2, x2) in zip(a, b):
        assert a1 == a2 and relmax(o1, o2) < 1e-11
        if x1 is not None:
            assert relmax(x1, x2) < 1e-11
    assert relmax(ax, bx) < 1e-11 and relmax(ad, bd) < 1e-11


@pytest.mark.parametrize("N,M,lag", [(16400, 7, 2), (20481, 50, 2), (40700, 301, 2), (40960, 90, 2), (40960, 301, 1),
                                     (20481, 1, 2), (16400, 2, 2), (16400, 3, 1)])
def test_team_sweep_odd_shapes_match_row_panels(G, monkeypatch, N, M, lag):
    """Teams of 2, 3, 4 and 5 workgroups per column, fewer columns than teams (idle teams; one, two
    and three columns in all: the pipeline's prologue and epilogue alone), a column
    count that does not divide: the chain on teams against the chain in row panels (1e-12), with the
    speculative first steps and a clamping bound in play."""
    rng = np.random.default_rng(N + M)
    A = np.asfortranarray(rng.normal(size=(N, M)) * rng.uniform(0.2, 2, size=M))
    dobs = rng.normal(size=N) * 3
    trajs = [(int(rng.integers(1, 6)), rng.normal(size=M) * 0.02, float(rng.uniform())) for _ in range(6)]
    res = {}
    monkeypatch.setenv("GRAVHMC_TEAM_LAG", str(lag))
    for team in ("1", "0"):
        monkeypatch.setenv("GRAVHMC_TEAM", team)
        eng = G.Engine(N, M)
        eng.upload_G(A)
        wm = eng.weight(0.5)
        eng.set_data(dobs)
        eng.set_reg("MS", 0.7, 0.01, (1, 1, M), 0.001 * wm)
        eng.chain_init(0.001 * wm, 0.0 * wm, 0.05 * wm)
        out = []
        eng.run_chain(iter(trajs), 0.002, lambda L, acc, o, xs: out.append((acc, o.copy(), xs)), want_x=True)
        st = eng.chain_stats()
        assert (st["team_launches"] > 0) == (team == "1") and st["team_timeouts"] == 0
        if team == "1":
            # rows a member holds: with a lag of two columns its part of r and the parked column share
            # the 160 KB of LDS
            cap = 10240 if lag == 1 else 10208
            assert st["team_members"] == -(-((N + 15) // 16 * 16) // cap)
            assert (N, lag, st["team_members"]) in ((16400, 2, 2), (16400, 1, 2), (20481, 2, 3), (40700, 2, 4),
                                                     (40960, 2, 5), (40960, 1, 4))
        res[team] = (out, eng.chain_get_x())
        eng.close()
    for (a1, o1, x1), (a0, o0, x0) in zip(res["1"][0], res["0"][0]):
        assert a1 == a0 and relmax(o1, o0) < 1e-12 and (x1 is None or relmax(x1, x0) < 1e-12)
    assert relmax(res["1"][1], res["0"][1]) < 1e-12


def test_matrix_free_tesseroid_fast_pass_variants_agree(G, monkeypatch):
    """The fast tesseroid pass in its three builds -- pipelined (next column's constants fetched
    ahead, r in LDS), plain, and the reference's operation order -- on a regional mesh with enough
    observations (9000: sixteen rows per thread, where the pipelined build does not fit the LDS and
    the plain one runs) and on a smaller one (2500: the pipelined build): forward, adjoint and a chain
    agree to 1e-11 (the decisions are the near-field table's in every build)."""
    mesh = G.mesher.TesseroidMesh((100, 130, 20, 50, 0, -200000), (-50000, 1.5, 1.5))
    M = mesh.size
    rng = np.random.default_rng(7)
    for nlon, nlat in ((50, 50), (100, 90)):
        lon, lat = [v.ravel() for v in np.meshgrid(np.linspace(100, 130, nlon), np.linspace(20, 50, nlat), indexing="ij")]
        h = np.full_like(lon, 200000.0)   # (high enough for the near-field pairs to stay below 1/64)
        N = lon.size
        x = rng.uniform(0, 1, M)
        r = rng.normal(size=N)
        trajs = [(int(rng.integers(2, 6)), rng.normal(size=M) * 0.001, float(rng.uniform())) for _ in range(3)]
        res = {}
        for tag, env in (("pipe", {"GRAVHMC_MF_PIPE": "1", "GRAVHMC_MF_EXACT": "0"}),
                         ("plain", {"GRAVHMC_MF_PIPE": "0", "GRAVHMC_MF_EXACT": "0"}),
                         ("exact", {"GRAVHMC_MF_PIPE": "0", "GRAVHMC_MF_EXACT": "1"})):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            eng = G.Engine(N, M)
            eng.set_matrix_free(True)
            eng.set_obs(lon, lat, h)
            eng.set_cells(mesh.cell_bounds(), 1, 1.6)
            eng.build_G()
            wm = eng.weight(0.5)
            st = eng.matrix_free_stats()
            assert st["near_entries"] > 0                      # the table is in use
            f, g = eng.forward(x * wm), eng.adjoint(r)
            eng.set_data(f + 0.01 * np.abs(f).max() * rng.normal(size=N) * 0 + 0.01 * np.abs(f).max())
            eng.set_reg("Damping", 0.05, 0.01, mesh.shape, 0.001 * wm)
            eng.chain_init(0.001 * wm, 0.0 * wm, 0.8 * wm)
            out = []
            eng.run_chain(iter(trajs), 0.005, lambda L, acc, o, xx: out.append((acc, o.copy())))
            res[tag] = (f, g, out, eng.chain_get_x())
            eng.close()
        for tag in ("pipe", "plain"):
            a, b = res[tag], res["exact"]
            assert relmax(a[0], b[0]) < 1e-11 and relmax(a[1], b[1]) < 1e-11 and relmax(a[3], b[3]) < 1e-10
            for (a1, o1), (a2, o2) in zip(a[2], b[2]):
                assert a1 == a2 and relmax(o1, o2) < 1e-10


@pytest.mark.parametrize("path", ["team_sweep", "matrix_free_tesseroid", "resident_stream"])
def test_round2_paths_are_bitwise_reproducible(G, path):
    """The inter-workgroup exchanges of the team sweep and of the resident kernel's stream mode, and
    the matrix-free pass with its near-field table, sum in an order fixed by indices alone: two runs
    of the same chain give the same bits."""
    rng = np.random.default_rng(31)
    runs = []
    for rep in range(2):
        if path == "team_sweep":
            N, M = 20481, 160
            r0 = np.random.default_rng(5)
            A = np.asfortranarray(r0.normal(size=(N, M)) * r0.uniform(0.2, 2, size=M))
            eng = G.Engine(N, M)
            eng.upload_G(A)
            wm = eng.weight(0.5)
            eng.set_data(r0.normal(size=N) * 3)
            shape, hi, dt, sig = (4, 5, 8), 0.3, 0.002, 0.02
        elif path == "matrix_free_tesseroid":
            mesh = G.mesher.TesseroidMesh((100, 130, 20, 50, 0, -200000), (-50000, 1.5, 1.5))
            lon, lat = [v.ravel() for v in np.meshgrid(np.linspace(100, 130, 50), np.linspace(20, 50, 50), indexing="ij")]
            N, M = lon.size, mesh.size
            eng = G.Engine(N, M)
            eng.set_matrix_free(True)
            eng.set_obs(lon, lat, np.full_like(lon, 200000.0))
            eng.set_cells(mesh.cell_bounds(), 1, 1.6)
            eng.build_G()
            wm = eng.weight(0.5)
            eng.set_data(eng.forward(np.random.default_rng(6).uniform(0, 1, M) * wm))
            shape, hi, dt, sig = mesh.shape, 0.8, 0.005, 0.001
        else:
            mesh = G.mesher.PrismMesh((0, 4000, 0, 2500, 0, 1600), (100, 100, 100))
            yp, xp = [a.ravel() for a in np.meshgrid(np.linspace(0, 2500, 25), np.linspace(0, 4000, 28))]
            N, M = xp.size, mesh.size
            eng = G.Engine(N, M)
            eng.set_obs(xp, yp, np.zeros_like(xp))
            eng.set_cells(mesh.cell_bounds(), 0)
            eng.build_G()
            wm = eng.weight(0.5)
            eng.set_data(eng.forward(np.random.default_rng(6).uniform(0, 1, M) * wm))
            shape, hi, dt, sig = mesh.shape, 1.0, 0.01, 0.001
        eng.set_reg("MS", 0.7, 0.01, shape, 0.001 * wm)
        eng.chain_init(0.001 * wm, 0.0 * wm, hi * wm)
        r1 = np.random.default_rng(9)
        trajs = [(int(r1.integers(2, 7)), r1.normal(size=M) * sig, float(r1.uniform())) for _ in range(6)]
        out = []
        eng.run_chain(iter(trajs), dt, lambda L, acc, o, x: out.append((acc, o.copy())), batch=3)
        st = eng.chain_stats()
        if path == "team_sweep":
            assert st["team_launches"] > 0 and st["team_members"] == 3
        if path == "resident_stream":
            assert st["resident_launches"] > 0
        runs.append((out, eng.chain_get_x(), eng.chain_get_dsyn()))
        eng.close()
    (a, ax, ad), (b, bx, bd) = runs
    assert len(a) == 6 and all(a1 == b1 and np.array_equal(o1, o2) for (a1, o1), (b1, o2) in zip(a, b))
    assert np.array_equal(ax, bx) and np.array_equal(ad, bd)


@pytest.mark.gpu
def test_profile_reports_the_one_read_sweeps_alone_where_panels_mix_in(G, monkeypatch):
    """N > 16384: a trajectory mixes team sweeps (the whole matrix each) with row-panel launches (a
    panel each).  gh_profile_read counts the launches that read the most bytes only, so that time and
    bytes per launch are those of ONE kernel (bench.py's roofline, comparable with a kernel trace);
    the team statistics say how many of a member's polls came before its team's parts."""
    N, M = 20481, 600
    rng = np.random.default_rng(5)
    A = np.asfortranarray(rng.normal(size=(N, M)))
    eng = G.Engine(N, M)
    eng.upload_G(A)
    wm = eng.weight(0.5)
    eng.set_data(rng.normal(size=N))
    eng.set_reg("Damping", 1.0, 0.01, (1, 1, M), 0.001 * wm)
    eng.chain_init(0.001 * wm, 0.0 * wm, 1.0 * wm)
    trajs = [(4, rng.normal(size=M) * 0.01, 0.5) for _ in range(3)]
    eng.profile_enable(True)
    eng.run_chain(iter(trajs), 0.002, lambda *a: None)
    prof = eng.profile_read()
    eng.profile_enable(False)
    st = eng.chain_stats()
    assert st["team_members"] == 3 and st["team_launches"] > 0 and st["team_timeouts"] == 0
    assert prof["bytes_per_sweep"] == N * M * 8          # a team sweep, not the average with the panels
    assert 0 < prof["sweeps"] <= st["team_launches"] and prof["sweep_ms"] > 0
    assert 0 <= st["team_late_parts"] <= st["team_launches"] * 256 * M
    eng.close()


@pytest.mark.gpu
def test_sampler_draws_from_the_library_are_np_randoms(G, tmp_path, capsys, monkeypatch):
    """HMCSample with the trajectories' random numbers drawn by the library (the default:
    inversion/rng.py, gh_rng_draw_trajectories) and by np.random itself (GRAVHMC_HOST_RNG=numpy):
    the same files byte for byte, the same printed lines, and the same generator state afterwards
    (the draws of the next np.random call agree)."""
    g = gold("c1_chain.npz")
    mesh, xp, yp, zp = c1_inputs()
    M = 6000
    out = {}
    for mode in ("native", "numpy"):
        monkeypatch.setenv("GRAVHMC_HOST_RNG", mode)
        gm = G.GravMagModule(g["dobs"], (0, 2000, 0, 3000, 0, 1000), (100, 100, 100), (xp, yp, zp), verbose=False)
        folder = str(tmp_path / ("chain_" + mode))
        capsys.readouterr()
        G.HMCSample(gm, 7, 0, 0.01, [5, 20], np.full(M, 0.001), np.full(M, 0.001),
                    np.c_[np.zeros(M), np.ones(M)], "mandatory", 1000, g["dobs"], "Fixed", 0.8, 1.0,
                    "MS", 0.001, 100, 0.001, save_folder=folder)
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("chain ")]
        out[mode] = (open(folder + "0/misfit.dat", "rb").read(), open(folder + "0/model.dat", "rb").read(), lines,
                     np.random.rand(3).tolist())
        gm._engine.close()
    assert out["native"][0] == out["numpy"][0] and out["native"][1] == out["numpy"][1]
    assert out["native"][2] == out["numpy"][2] and len(out["native"][2]) >= 7
    # both modes drew the same number of trajectories ahead of the last accepted one
    assert out["native"][3] == out["numpy"][3]
