"""GPU suite of the prism gravity components other than gz (GH_CELL_PRISM_COMP): entries and results
against the reference's _prism.<comp> / prism.<comp>, the gzz GravMagModule and HMCSample against the
reference's own code on the gzz kernel (tests/make_golden_grav.py), and the paths that consume a stored or
computed kernel against each other.

Tolerances are the gravity suite's (tests/test_gpu_parity.py): entries |dK| <= 1e-10 max|K|;
results and the potential 1e-10 relative; matrix-free against dense 1e-12 (summation order differs)."""
import os

import numpy as np
import pytest

from conftest import gold
from helpers import c1_inputs, relmax

pytestmark = pytest.mark.gpu

COMPS = ("potential", "geoid", "gx", "gy", "gz", "gxx", "gxy", "gxz", "gyy", "gyz", "gzz")


@pytest.fixture(scope="module")
def G(built_lib):
    import gravinv3dhmc_amd as g
    return g


def _comp_engine(G, xp, yp, zp, cells, comp, matrix_free=False):
    from gravinv3dhmc_amd import _lib
    eng = G.Engine(np.asarray(xp).size, np.asarray(cells).shape[0])
    if matrix_free:
        eng.set_matrix_free(True)
    eng.set_obs(xp, yp, zp)
    eng.set_cells(cells, _lib.CELL_PRISM_COMP, component=comp)
    return eng


def _module(G, p, **kw):
    return G.GravMagModule(p["dobs"], tuple(p["mrange"]), tuple(p["mspacing"]), (p["xp"], p["yp"], p["zp"]),
                           component=str(p["component"]), verbose=False, **kw)


# ----------------------------------------------------------------------------- entries / results

@pytest.mark.parametrize("comp", COMPS)
def test_component_entries_and_results_against_the_reference(G, comp):
    from gravinv3dhmc_amd import mesher
    g = gold("prism_comp_cases.npz")
    xp, yp, zp, cells, dens = g["xp"], g["yp"], g["zp"], g["cells"], g["dens"]
    Kref = g["K_" + comp]
    eng = _comp_engine(G, xp, yp, zp, cells, comp)
    res = eng.prism_result(dens)                             # gh_prism_result: needs no G
    eng.build_G()
    K = eng.download_G()
    assert np.isfinite(K).all() and np.isfinite(res).all()
    err = np.abs(K - Kref).max() / np.abs(Kref).max()
    print("%s entries: max |dK|/max|K| = %.3e" % (comp, err))
    assert err <= 1e-10, (comp, err)
    assert relmax(res, g["res_" + comp]) <= 1e-10
    assert relmax(eng.prism_result(dens), res) == 0.0     # works after G too, same bits
    eng.close()
    # prism.<comp> on a list of prisms: a cell without the property is skipped, dens overrides the property
    props = [{"density": float(dens[0])}, {"density": float(dens[1])}, None, {"density": float(dens[3])}]
    prisms = [mesher.Prism(*b, props=p) for b, p in zip(cells, props)]
    fn = getattr(G.prism, comp)
    r, K3 = fn(xp, yp, zp, prisms)
    assert relmax(r, g["res_mixed_" + comp]) <= 1e-10
    assert K3.shape == (xp.size, 3) and K3.flags.f_contiguous
    assert np.abs(K3 - Kref[:, [0, 1, 3]]).max() <= 1e-10 * np.abs(Kref).max()
    r, none = fn(xp, yp, zp, prisms, dens=2.5, return_kernel=False)
    assert relmax(r, g["res_dens_" + comp]) <= 1e-10 and none is None
    with pytest.raises(ValueError):
        fn(xp, yp, zp, [mesher.Prism(*cells[0])])          # no cell has the property


def test_c1_component_columns_against_the_reference(G):
    g = gold("c1_comp_columns.npz")
    mesh, xp, yp, zp = c1_inputs()
    mesh.addprop("density", np.zeros(mesh.size))
    for comp in ("gzz", "gxy", "gx"):
        res, K = getattr(G.prism, comp)(xp, yp, zp, mesh)
        assert K.shape == (600, 6000) and np.isfinite(K).all()
        assert np.array_equal(res, np.zeros(600))            # zero density
        err = np.abs(K[:, g["cols_" + comp]] - g["K_" + comp]).max() / np.abs(g["K_" + comp]).max()
        print("C1 %s columns: max |dK|/max|K| = %.3e" % (comp, err))
        assert err <= 1e-10


def test_gz_through_the_component_path_is_bitwise_the_prism_kind(G):
    from gravinv3dhmc_amd import _lib
    g = gold("prism_comp_cases.npz")
    xp, yp, zp, cells = g["xp"], g["yp"], g["zp"], g["cells"]
    a = G.Engine(xp.size, cells.shape[0])
    a.set_obs(xp, yp, zp)
    a.set_cells(cells, _lib.CELL_PRISM, component="gz")
    b = G.Engine(xp.size, cells.shape[0])
    b.set_obs(xp, yp, zp)
    b.set_cells(cells, _lib.CELL_PRISM)
    a.build_G()
    b.build_G()
    assert np.array_equal(a.download_G(), b.download_G())
    assert relmax(a.prism_result(g["dens"]), g["res_gz"]) <= 1e-10
    a.close()
    b.close()


def test_refusals_never_fall_back_to_gz(G):
    from gravinv3dhmc_amd import _lib
    eng = G.Engine(3, 1)
    cell = np.array([[0, 1, 0, 1, 0, 1.0]])
    with pytest.raises(ValueError):
        eng.set_cells(cell, _lib.CELL_PRISM_COMP)                          # no component
    with pytest.raises(ValueError):
        eng.set_cells(cell, _lib.CELL_PRISM_COMP, component="gzx")
    with pytest.raises(ValueError):
        eng.set_cells(cell, _lib.CELL_TESSEROID, component="gzz")
    with pytest.raises(ValueError):                                        # gh_set_cells keeps refusing kind 3
        eng._chk(eng._lib.gh_set_cells(eng._h, _lib.ptr(cell.ravel()), _lib.CELL_PRISM_COMP, 1.0))
    with pytest.raises(ValueError):
        eng._chk(eng._lib.gh_set_cells_prism(eng._h, _lib.ptr(cell.ravel()), 11))
    eng.set_cells(cell, _lib.CELL_PRISM_TF, direction=(0.0, 0.0, 1.0))
    eng.set_obs(np.zeros(3), np.zeros(3), np.full(3, -1.0))
    with pytest.raises(ValueError):
        eng.prism_result(np.ones(1))                                       # a magnetic context
    eng.close()


# ----------------------------------------------------------------------------- the module

def test_gzz_module_weights_and_potential_golden(G, capsys):
    p = gold("potential_small_gzz.npz")
    gm = G.GravMagModule(p["dobs"], tuple(p["mrange"]), tuple(p["mspacing"]), (p["xp"], p["yp"], p["zp"]),
                         component="gzz")
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "Calculating gravity field (gzz) in cartesian coordinate."
    assert "kernel.shape (42, 120)" in out
    assert "density" in gm.mesh.props and gm.component == "gzz"
    assert relmax(gm.Wm.diagonal(), p["wm"]) < 1e-11
    assert relmax(np.asarray(gm.Aw), p["Aw"]) < 1e-10
    worst = 0.0
    for reg in ("Damping", "MS", "Smoothness", "TV"):
        for i, x in enumerate(p["xs"]):
            m, grad, dpre, dv, mv = gm.misfit_and_grad(x, p["mwapr"], None, None, "mandatory", 1000,
                                                       float(p["alpha"]), regulization=reg, beta=float(p["beta"]))
            errs = [abs(m - p[reg + "_misfit"][i]) / abs(m), relmax(grad, p[reg + "_grad"][i]),
                    relmax(dpre, p[reg + "_dpre"][i]), abs(dv - p[reg + "_data"][i]) / abs(dv),
                    abs(mv - p[reg + "_model"][i]) / max(abs(mv), 1e-300)]
            worst = max(worst, max(errs))
            assert max(errs) < 1e-10, (reg, i, errs)
    print("gzz misfit_and_grad worst rel err %.3e" % worst)
    gm._engine.close()


def _hmc(G, gm, p, c, tag, folder):
    M = p["wm"].size
    dt, Sigma, lo, hi, n = c[tag + "_cfg"]
    G.HMCSample(gm, int(n), 0, float(dt), [5, 20], np.full(M, 0.001 + lo), np.full(M, 0.001),
                np.c_[np.full(M, lo), np.full(M, hi)], "mandatory", 1000, p["dobs"],
                "Fixed", 0.8, 1.0, str(c[tag + "_reg"]), 0.001, 100, float(Sigma), nbest=100,
                myrank=0, save_folder=folder)


@pytest.mark.parametrize("resident", ["1", "0"])
def test_gzz_hmcsample_end_to_end(G, tmp_path, capsys, monkeypatch, resident):
    """Whole chains on the gzz module against the reference's own runs on the gzz kernel; the resident
    chain kernel ("1") and the sweep path ("0") both give the reference's lines."""
    monkeypatch.setenv("GRAVHMC_RESIDENT", resident)
    c = gold("chain_small_gzz.npz")
    p = gold("potential_small_gzz.npz")
    for tag in ("a", "b"):
        gm = _module(G, p)
        folder = str(tmp_path / ("run_%s_chain" % tag))
        capsys.readouterr()
        _hmc(G, gm, p, c, tag, folder)
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("chain ")]
        assert lines == [str(s) for s in c[tag + "_lines"]]
        np.testing.assert_allclose(np.loadtxt(folder + "0/misfit.dat"), c[tag + "_misfit"], atol=2e-8, rtol=1e-9)
        np.testing.assert_allclose(np.loadtxt(folder + "0/model.dat"), c[tag + "_model"], atol=2e-8)
        gm._engine.close()


def test_gzz_lockstep_batch_matches_single_chain_engines(G):
    p = gold("potential_small_gzz.npz")
    gm = _module(G, p)
    eng = gm._engine
    wm = gm.Wm.diagonal()
    M = wm.size
    eng.set_reg("TV", 1.0, 0.001, p["shape"], 0.001 * wm)
    rng = np.random.default_rng(7)
    C, T = 3, 3
    x0s = np.stack([(0.001 + 0.002 * c) * wm for c in range(C)])
    low, high = 0.0 * wm, 0.02 * wm
    Ls = rng.integers(2, 9, size=(C, T))
    p0s = rng.normal(size=(C, T, M)) * 0.3
    us = rng.uniform(size=(C, T))
    eng.batch_init(x0s, low, high)
    accb, outb, _ = eng.batch_run(p0s, 0.02, Ls, us)
    single = _module(G, p)._engine
    single.set_reg("TV", 1.0, 0.001, p["shape"], 0.001 * wm)
    for c in range(C):
        x = x0s[c]
        for t in range(T):
            x, acc, o, _ = single.leapfrog(x, p0s[c, t], 0.02, int(Ls[c, t]), low, high, float(us[c, t]))
            assert bool(accb[c, t]) == acc and abs(outb[c, t, 0] - o[0]) <= 1e-10 * abs(o[0])
        assert relmax(eng.batch_get_x(c), x) <= 1e-10
    eng.close()
    single.close()


# ----------------------------------------------------------------------------- matrix-free

def _small(G, comp, **kw):
    p = gold("potential_small_gzz.npz")
    return G.GravMagModule(p["dobs"], tuple(p["mrange"]), tuple(p["mspacing"]), (p["xp"], p["yp"], p["zp"]),
                           component=comp, verbose=False, **kw), p


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("comp", ["gx", "gxy", "gzz", "potential"])
def test_matrix_free_component_matches_dense(G, monkeypatch, fused, comp):
    monkeypatch.setenv("GRAVHMC_MF_FUSED", fused)
    dense, p = _small(G, comp)
    mf, _ = _small(G, comp, matrix_free=True)
    assert relmax(mf.Wm.diagonal(), dense.Wm.diagonal()) < 1e-13
    wm = dense.Wm.diagonal()
    M = wm.size
    x = p["xs"][1]
    assert relmax(mf._engine.forward(x), dense._engine.forward(x)) < 1e-12
    r = np.random.default_rng(0).normal(size=p["dobs"].size)
    assert relmax(mf._engine.adjoint(r), dense._engine.adjoint(r)) < 1e-12
    for reg in ("Damping", "MS", "Smoothness", "TV"):
        a = mf.misfit_and_grad(x, p["mwapr"], None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        b = dense.misfit_and_grad(x, p["mwapr"], None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        assert abs(a[0] - b[0]) < 1e-12 * abs(b[0]) and relmax(a[1], b[1]) < 1e-11
    rng = np.random.default_rng(4)
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(8)]
    outs = []
    for m in (mf, dense):
        e = m._engine
        e.set_reg("TV", 1.0, 0.001, p["shape"], 0.001 * wm)
        e.chain_init(0.001 * wm, 0.0 * wm, 0.02 * wm)
        res = []
        e.run_chain(iter(trajs), 0.02, lambda L, acc, o, x, res=res: res.append((acc, o.copy(), x)), want_x=True)
        outs.append(res)
    for (a1, o1, x1), (a2, o2, x2) in zip(*outs):
        assert a1 == a2 and relmax(o1, o2) < 1e-12 and (x1 is None or relmax(x1, x2) < 1e-12)
    # the matrix-free batch of chains has no component kernels: refused, never run on gz entries
    with pytest.raises(NotImplementedError, match="component"):
        mf._engine.batch_init(np.stack([0.001 * wm, 0.002 * wm]), 0.0 * wm, 0.02 * wm)
    mf._engine.close()
    dense._engine.close()


def test_wavelet_forward_on_matrix_free_component_model_matches_dense(G):
    dense, p = _small(G, "gzz", wavelet="3D")
    mf, _ = _small(G, "gzz", wavelet="3D", matrix_free=True)
    cd, cm = dense.Awcp, mf.Awcp
    assert cd.nnz == cm.nnz and np.array_equal(cd.indices, cm.indices) and relmax(cm.data, cd.data) < 1e-12
    x = p["xs"][1]
    assert relmax(mf._engine.forward_wavelet(x), dense._engine.forward_wavelet(x)) < 1e-12
    for reg in ("Damping", "TV"):
        a = mf.misfit_and_grad(x, p["mwapr"], None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        b = dense.misfit_and_grad(x, p["mwapr"], None, None, "mandatory", 1000, 0.7, regulization=reg, beta=0.001)
        assert abs(a[0] - b[0]) < 1e-12 * abs(b[0]) and relmax(a[1], b[1]) < 1e-11
    mf._engine.close()
    dense._engine.close()


# ----------------------------------------------------------------------------- shards

def test_sharded_engine_rccl_world1_is_bitwise_unsharded_on_the_gzz_kernel(G, monkeypatch):
    monkeypatch.setenv("GRAVHMC_RESIDENT", "0")
    from gravinv3dhmc_amd import _lib, mesher
    from gravinv3dhmc_amd.dist import Ranks, make_sharded_engine
    p = gold("potential_small_gzz.npz")
    env = {k: os.environ.pop(k, None) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    try:
        ranks = Ranks()
    finally:
        for k, v in env.items():
            if v is not None:
                os.environ[k] = v
    bounds = mesher.PrismMesh(tuple(p["mrange"]), tuple(p["mspacing"])).cell_bounds()
    N, M = p["dobs"].size, bounds.shape[0]

    def setup(eng):
        eng.set_obs(p["xp"], p["yp"], p["zp"])
        eng.set_cells(bounds, _lib.CELL_PRISM_COMP, component="gzz")
        eng.build_G()
        w = eng.weight(0.5)
        eng.set_data(p["dobs"])
        eng.set_reg("MS", 1.0, 0.001, p["shape"], 0.001 * w)
        eng.chain_init(0.001 * w, 0.0 * w, 0.02 * w)
        return w

    a = make_sharded_engine(N, M, ranks, device=0, backend="rccl")
    b = G.Engine(N, M)
    wa, wb = setup(a), setup(b)
    assert np.array_equal(wa, wb) and relmax(wb, p["wm"]) < 1e-11
    rng = np.random.default_rng(2)
    trajs = [(int(rng.integers(1, 9)), rng.normal(size=M) * 0.3, float(rng.uniform())) for _ in range(10)]
    ra, rb = [], []
    a.run_chain(iter(trajs), 0.02, lambda L, acc, o, x: ra.append((acc, o.copy(), x)), want_x=True)
    b.run_chain(iter(trajs), 0.02, lambda L, acc, o, x: rb.append((acc, o.copy(), x)), want_x=True, batch=3)
    for (a1, o1, x1), (a2, o2, x2) in zip(ra, rb):
        assert a1 == a2 and np.array_equal(o1, o2)
        assert (x1 is None) == (x2 is None) and (x1 is None or np.array_equal(x1, x2))
    x = rng.uniform(0, 1, M) * wb
    assert np.array_equal(a.forward(x), b.forward(x))
    ma, mb = a.misfit_and_grad(x), b.misfit_and_grad(x)
    assert ma[0] == mb[0] and np.array_equal(ma[1], mb[1])
    a.close()
    b.close()
